// texture_views_kernels.hip -- texture baking from posed views (rf_texture_project_views of relu_field.h): what
// bake_texture_from_views of thr3ed_atom_amd/texture.py is built on.  DESIGN.md section 23 has the contract and the measurements,
// docs/texture_views_errors.md the error bound, tests/texture_views_model.py the float64 model.
//
// The texel.  The atlas, the texel's point p and its face's unit normal n are those of rf_texture_bake (texture_atlas.h: the same
// float32 operations, the same bits).  For each view k, in order, with R_k, t_k, f_k its pose and focal and H x W the image size:
//   c = R_k^T (p - t_k), z = -c_z                               rejected unless z is finite and z > near
//   x = W/2 + f c_x / z, y = H/2 - f c_y / z                    rejected unless 0 <= x < W and 0 <= y < H; j = floor x, i = floor y
//   cos = n . (t_k - p) / |t_k - p| (|cos| when two-sided)      rejected unless cos > min_cos; omega = cos^cos_power by multiplication
//   key = visibility[k, i, j], z_buf = the float in its high word   rejected when all ones or unless z <= z_buf + depth_bias
//   C = the bilinear fetch of image k at (x - 1/2, y - 1/2), taps clamped; m = the same fetch of the alpha plane, or 1
//   accum.rgb += omega m (C - (1 - m) background), accum.w += omega m m, count += 1
// -- the inverse of pixel_ray of rf_device.h (pixel (i, j) has its centre at (j + 1/2, i + 1/2)), a shadow-map test with a bias
// against the depth rf_mesh_raster_visibility wrote, the bilinear fetch of view_camera.h, and the least-squares texel of pixels read as
// C = m c + (1 - m) background.
//
// The kernel.  ONE launch per chunk of at most 16 views, one lane per texel, block-major like the bake (a wave covers at most four
// faces, so its texels project next to each other and its taps share lines).  The cameras travel BY VALUE in the kernel's argument
// struct: the view loop is wave-uniform, so they are scalar loads and the host uploads nothing.  The rejections that need registers
// only (near, image box, angle) come before any load; a texel-view that survives reads one 8-byte key and at most 16 taps.  The lane
// loads its accumulator, adds its views in order and stores it -- no atomics, two calls give the same bits, and successive calls over
// chunks of views do the float additions of one long loop.  Unowned texels are not touched.  A face index outside [0, V) stores 1 to
// the status word and leaves its texels as they were; it is never used as an address.
#include "texture_atlas.h"
#include "view_camera.h"

namespace {

constexpr int kViewsBlock = 256;
constexpr int kMinPatch = 2, kMaxPatch = 64;
constexpr int kMaxCosPower = 8;

struct ViewsArgs {
  const float* vertices;
  const long long* faces;
  long long num_vertices, num_faces;
  int patch, block, cols, rows;
  int num_views, H, W;
  const float* images;                // [n, H, W, 3]
  const unsigned long long* visibility;  // [n, H, W]
  const float* alphas;                // [n, H, W] or nullptr
  float near, depth_bias, min_cos, background;
  int cos_power, two_sided;
  float* accum;  // [rows B, cols B, 4]
  int* count;    // [rows B, cols B] or nullptr
  int* status;
  RFCamera cams[kMaxViews];  // (height and width are H and W in every one)
};

__global__ __launch_bounds__(kViewsBlock) void texture_project_views_kernel(ViewsArgs a) {
  const int B = a.block, P = a.patch;
  const long long total = ((long long)a.cols * B) * ((long long)a.rows * B);
  const long long t = (long long)blockIdx.x * kViewsBlock + threadIdx.x;
  if (t >= total) return;
  const AtlasTexel tx = atlas_texel(t, P, B, a.cols);
  if (tx.tri >= a.num_faces) return;  // unowned: not touched
  unsigned long long vi[3];
  if (!atlas_face(a.faces, a.num_vertices, tx.tri, vi)) {
    *a.status = 1;  // (a plain store of one value: whichever lane wins, the word reads 1)
    return;
  }
  float p[3], n[3];
  atlas_point(a.vertices, vi, P, tx, p, n);
  const int H = a.H, W = a.W;
  const long long plane = (long long)H * W;
  float* slot = a.accum + 4 * tx.pixel;
  float acc[4] = {slot[0], slot[1], slot[2], slot[3]};
  int seen = a.count ? a.count[tx.pixel] : 0;
  for (int k = 0; k < a.num_views; ++k) {  // (wave-uniform: the camera is read with scalar loads)
    const RFCamera& cam = a.cams[k];
    // pose is the row-major 3 x 4 [R | t]
    const float d[3] = {p[0] - cam.pose[3], p[1] - cam.pose[7], p[2] - cam.pose[11]};
    const float cx = (d[0] * cam.pose[0] + d[1] * cam.pose[4]) + d[2] * cam.pose[8];
    const float cy = (d[0] * cam.pose[1] + d[1] * cam.pose[5]) + d[2] * cam.pose[9];
    const float z = -((d[0] * cam.pose[2] + d[1] * cam.pose[6]) + d[2] * cam.pose[10]);
    if (!(z > a.near) || !(z <= 3.0e38f)) continue;  // (NaN fails the first test, +inf the second)
    const float x = (float)W * 0.5f + cam.focal * cx / z;
    const float y = (float)H * 0.5f - cam.focal * cy / z;
    if (!(x >= 0.0f && x < (float)W && y >= 0.0f && y < (float)H)) continue;
    const float len = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);  // > 0: z > near >= 0
    float cs = -((n[0] * d[0] + n[1] * d[1]) + n[2] * d[2]) / len;
    if (a.two_sided) cs = fabsf(cs);
    if (!(cs > a.min_cos)) continue;
    const int j = (int)x, i = (int)y;  // in [0, W) and [0, H): 0 <= x < W <= 16384
    const long long view = (long long)k * plane;
    const unsigned long long key = a.visibility[view + (long long)i * W + j];
    if (key == kNoHit) continue;
    const float zbuf = __uint_as_float((unsigned int)(key >> 32));
    if (!(z <= zbuf + a.depth_bias)) continue;
    float omega = 1.0f;
    for (int q = 0; q < a.cos_power; ++q) omega = omega * cs;
    const BilinearTaps s = bilinear_taps(x - 0.5f, y - 0.5f, H, W);
    const long long r0 = view + (long long)s.y0 * W, r1 = view + (long long)s.y1 * W;
    const long long o00 = r0 + s.x0, o01 = r0 + s.x1, o10 = r1 + s.x0, o11 = r1 + s.x1;
    const float m = a.alphas ? bilinear_blend(s, a.alphas[o00], a.alphas[o01], a.alphas[o10], a.alphas[o11]) : 1.0f;
    const float wm = omega * m;
    const float rest = (1.0f - m) * a.background;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float c = bilinear_blend(s, a.images[3 * o00 + ch], a.images[3 * o01 + ch], a.images[3 * o10 + ch], a.images[3 * o11 + ch]);
      acc[ch] = acc[ch] + wm * (c - rest);
    }
    acc[3] = acc[3] + wm * m;
    seen += 1;
  }
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) slot[ch] = acc[ch];
  if (a.count) a.count[tx.pixel] = seen;
}

}  // namespace

extern "C" {

int rf_texture_project_views(const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces, int32_t patch, int32_t cols,
                             int32_t rows, int32_t num_views, const RFCamera* cameras, const float* images_dev, const uint64_t* visibility_dev,
                             const float* alphas_dev, float near, float depth_bias, float min_cos, int32_t cos_power, float background, uint32_t flags,
                             float* accum_dev, int32_t* count_dev, int32_t* status_dev, void* stream) {
  if (!accum_dev || !status_dev) return RF_ERR_NULL_POINTER;
  if ((num_vertices > 0 && !vertices_dev) || (num_faces > 0 && !faces_dev)) return RF_ERR_NULL_POINTER;
  if (num_views > 0 && (!cameras || !images_dev || !visibility_dev)) return RF_ERR_NULL_POINTER;
  if (num_vertices < 0 || num_faces < 0) return RF_ERR_BAD_SHAPE;
  if (num_views < 0 || num_views > kMaxViews) return RF_ERR_BAD_SHAPE;
  if (patch < kMinPatch || patch > kMaxPatch) return RF_ERR_BAD_SHAPE;
  if (cols < 1 || rows < 1) return RF_ERR_BAD_SHAPE;
  const int block = patch + 4;
  if ((long long)cols * block > kMaxImageEdge || (long long)rows * block > kMaxImageEdge) return RF_ERR_BAD_SHAPE;
  if (2ll * cols * rows < num_faces) return RF_ERR_BAD_SHAPE;
  if (!view_cameras_ok(cameras, num_views)) return RF_ERR_BAD_SHAPE;
  if (!std::isfinite(near) || !(near >= 0.0f) || !std::isfinite(depth_bias) || !(depth_bias >= 0.0f)) return RF_ERR_BAD_SHAPE;
  if (!std::isfinite(background) || !(background >= 0.0f)) return RF_ERR_BAD_SHAPE;
  if (!(min_cos >= 0.0f) || !(min_cos < 1.0f)) return RF_ERR_BAD_SHAPE;
  if (cos_power < 0 || cos_power > kMaxCosPower) return RF_ERR_BAD_SHAPE;
  if (flags & ~(uint32_t)RF_TEXTURE_VIEWS_TWO_SIDED) return RF_ERR_UNSUPPORTED;
  if (num_views == 0 || num_faces == 0) return RF_OK;
  ViewsArgs a;
  a.vertices = vertices_dev, a.faces = (const long long*)faces_dev;
  a.num_vertices = num_vertices, a.num_faces = num_faces;
  a.patch = patch, a.block = block, a.cols = cols, a.rows = rows;
  a.num_views = num_views, a.H = cameras[0].height, a.W = cameras[0].width;
  a.images = images_dev, a.visibility = (const unsigned long long*)visibility_dev, a.alphas = alphas_dev;
  a.near = near, a.depth_bias = depth_bias, a.min_cos = min_cos, a.background = background;
  a.cos_power = cos_power, a.two_sided = (flags & RF_TEXTURE_VIEWS_TWO_SIDED) ? 1 : 0;
  a.accum = accum_dev, a.count = count_dev, a.status = status_dev;
  fill_view_cameras(a.cams, cameras, num_views);
  const long long total = (long long)cols * block * rows * block;  // <= 2^28
  hipLaunchKernelGGL(texture_project_views_kernel, dim3((unsigned)((total + kViewsBlock - 1) / kViewsBlock)), dim3(kViewsBlock), 0, (hipStream_t)stream, a);
  return launch_status();
}

}  // extern "C"
