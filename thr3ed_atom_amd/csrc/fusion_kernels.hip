// fusion_kernels.hip -- TSDF fusion of posed depth views into a node lattice (rf_fuse_depth_views of relu_field.h): what
// fuse_depth_views of thr3ed_atom_amd/fusion.py is built on.  DESIGN.md section 26 has the contract and the measurements,
// docs/fusion_errors.md the error bound, tests/fusion_model.py the float64 model.
//
// The node.  The lattice has dims = (X, Y, Z) nodes in the box [aabb_min, aabb_max], placed as a VoxelGrid's nodes are: node
// (ix, iy, iz) sits at aabb_min + (aabb_max - aabb_min) * ((2i + 1) / (2 dim)) per axis in float32 -- the operations of the interior
// lattice points of mesh_kernels.hip at subdivisions = 1 -- and has plain index (ix Y + iy) Z + iz.  For each view k, in order, with
// R_k, t_k, f_k its pose and focal and H x W the image size:
//   c = R_k^T (p - t_k), z = -c_z                               skipped unless z is finite and z > near
//   x = W/2 + f c_x / z, y = H/2 - f c_y / z                    skipped unless 0 <= x < W and 0 <= y < H; j = floor x, i = floor y
//   D = depths[k, i, j], A = alphas[k, i, j] (when given)       skipped when D is not finite; a MISS when D <= 0 or A < min_alpha
//   miss: s = 1 under RF_FUSE_CARVE, skipped without it         hit: sdf = D - z; sdf < -truncation: hidden += 1 and nothing else;
//                                                               otherwise s = min(1, sdf / truncation)
//   tsdf_sum += s, observed += 1; a hit with |sdf| <= truncation also adds images[k, i, j, :] to colour_sum.rgb and 1 to colour_sum.w
// -- the products and the sum order of texture_project_views_kernel for the camera, a NEAREST pixel fetch (interpolating depth across a
// discontinuity invents surfaces) and unit weights.
//
// The kernel.  ONE launch per chunk of at most 16 views, one lane per node.  The cameras travel BY VALUE in the kernel's argument
// struct: the view loop is wave-uniform, so they are scalar loads and the host uploads nothing.  The rejections that need registers
// only (near, image box) come before any load, and a pixel index is formed only after 0 <= x < W and 0 <= y < H held (NaN fails
// both).  The lane loads its accumulators, adds its views in order and stores them -- no atomics, no LDS, two calls give the same
// bits, and successive calls over chunks of views do the float additions of one long loop.
//
// Lane -> node.  A wavefront takes a 4 x 4 x 4-node block (lane = 16 dx + 4 dy + dz), blocks in z-fastest order: its nodes project into a
// few neighbouring pixels of every view and its accumulators are 16-byte segments that neighbouring wavefronts complete to lines.
// The other natural mapping, 64 consecutive iz per wavefront (coalesced accumulators, up to 64 scattered depth pixels per view), was
// measured 5.1 x slower on the 256^3 scene and is not kept (profiles/fusion_mapping_ab.md).  The contract fixes
// only the order of views per node, so the mapping changes no bit.
#include "view_camera.h"

namespace {

constexpr int kFuseBlock = 256;
constexpr int kMaxDim = 4096;

struct FuseArgs {
  float amin[3], ext[3];
  int X, Y, Z;
  unsigned int by, bz;      // 4-node blocks along y and z
  long long lanes;          // lanes of the launch: 64 x the number of blocks
  int num_views, H, W;
  const float* depths;      // [n, H, W]
  const float* alphas;      // [n, H, W] or nullptr
  const float* images;      // [n, H, W, 3] or nullptr
  float near, truncation, min_alpha;
  int carve;
  float* tsdf_sum;          // [N]
  int2* counts;             // [N] (observed, hidden)
  float4* colour_sum;       // [N] or nullptr
  RFCamera cams[kMaxViews]; // (height and width are H and W in every one)
};

// float32 position of node i of `dim` on one axis: the interior lattice point of mesh_kernels.hip at subdivisions = 1
__device__ __forceinline__ float node_coord(float amin, float ext, int i, int dim) {
  const float frac = (float)(2 * i + 1) / (float)(2 * dim);
  return amin + ext * frac;
}

__global__ __launch_bounds__(kFuseBlock) void fuse_depth_views_kernel(FuseArgs a) {
  const long long t = (long long)blockIdx.x * kFuseBlock + threadIdx.x;
  if (t >= a.lanes) return;
  const unsigned int block = (unsigned int)(t >> 6), lane = (unsigned int)t & 63u;  // (at most 1024^3 blocks)
  const unsigned int bz = block % a.bz, rest = block / a.bz;
  const int ix = (int)(4u * (rest / a.by) + (lane >> 4)), iy = (int)(4u * (rest % a.by) + ((lane >> 2) & 3u)), iz = (int)(4u * bz + (lane & 3u));
  if (ix >= a.X || iy >= a.Y || iz >= a.Z) return;  // a partial block
  const size_t node = ((size_t)ix * a.Y + iy) * a.Z + iz;
  const float p[3] = {node_coord(a.amin[0], a.ext[0], ix, a.X), node_coord(a.amin[1], a.ext[1], iy, a.Y), node_coord(a.amin[2], a.ext[2], iz, a.Z)};
  const int H = a.H, W = a.W;
  const long long plane = (long long)H * W;
  float sum = a.tsdf_sum[node];
  int2 seen = a.counts[node];
  float4 col = a.colour_sum ? a.colour_sum[node] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
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
    const int j = (int)x, i = (int)y;  // in [0, W) and [0, H): 0 <= x < W <= 16384
    const long long pixel = (long long)k * plane + (long long)i * W + j;
    const float D = a.depths[pixel];
    const float A = a.alphas ? a.alphas[pixel] : 1.0f;  // (issued with the depth: neither load waits for the other)
    if (!(fabsf(D) < INFINITY)) continue;  // not finite: no information
    const bool miss = !(D > 0.0f) || (a.alphas && A < a.min_alpha);
    float s = 1.0f;
    if (miss) {
      if (!a.carve) continue;
    } else {
      const float sdf = D - z;
      if (sdf < -a.truncation) {
        seen.y += 1;  // hidden
        continue;
      }
      s = fminf(1.0f, sdf / a.truncation);
      if (a.images && fabsf(sdf) <= a.truncation) {
        const float* rgb = a.images + 3 * pixel;
        col.x = col.x + rgb[0], col.y = col.y + rgb[1], col.z = col.z + rgb[2], col.w = col.w + 1.0f;
      }
    }
    sum = sum + s;
    seen.x += 1;  // observed
  }
  a.tsdf_sum[node] = sum;
  a.counts[node] = seen;
  if (a.colour_sum) a.colour_sum[node] = col;
}

}  // namespace

extern "C" {

int rf_fuse_depth_views(const float* aabb_min, const float* aabb_max, const int32_t* dims, int32_t num_views, const RFCamera* cameras,
                        const float* depths_dev, const float* alphas_dev, const float* images_dev, float near, float truncation, float min_alpha,
                        uint32_t flags, float* tsdf_sum_dev, int32_t* counts_dev, float* colour_sum_dev, void* stream) {
  if (!aabb_min || !aabb_max || !dims || !tsdf_sum_dev || !counts_dev) return RF_ERR_NULL_POINTER;
  if (num_views > 0 && (!cameras || !depths_dev)) return RF_ERR_NULL_POINTER;
  if (images_dev && !colour_sum_dev) return RF_ERR_NULL_POINTER;
  long long N = 1;
  for (int a = 0; a < 3; ++a) {
    if (dims[a] < 1 || dims[a] > kMaxDim) return RF_ERR_BAD_SHAPE;
    N *= dims[a];
  }
  if (N >= (1ll << 31)) return RF_ERR_BAD_SHAPE;
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(aabb_min[a]) || !std::isfinite(aabb_max[a]) || !(aabb_max[a] > aabb_min[a])) return RF_ERR_BAD_SHAPE;
    if (!std::isfinite(aabb_max[a] - aabb_min[a])) return RF_ERR_BAD_SHAPE;  // (the extent itself overflows)
  }
  if (num_views < 0 || num_views > kMaxViews) return RF_ERR_BAD_SHAPE;
  if (!view_cameras_ok(cameras, num_views)) return RF_ERR_BAD_SHAPE;
  if (!std::isfinite(near) || !(near >= 0.0f)) return RF_ERR_BAD_SHAPE;
  if (!std::isfinite(truncation) || !(truncation > 0.0f)) return RF_ERR_BAD_SHAPE;
  if (!(min_alpha >= 0.0f) || !(min_alpha <= 1.0f)) return RF_ERR_BAD_SHAPE;
  if (((uintptr_t)counts_dev & 7u) || ((uintptr_t)colour_sum_dev & 15u)) return RF_ERR_BAD_SHAPE;  // (loaded and stored as 8 and 16 bytes)
  if (flags & ~(uint32_t)RF_FUSE_CARVE) return RF_ERR_UNSUPPORTED;
  if (num_views == 0) return RF_OK;
  FuseArgs a;
  for (int i = 0; i < 3; ++i) a.amin[i] = aabb_min[i], a.ext[i] = aabb_max[i] - aabb_min[i];
  a.X = dims[0], a.Y = dims[1], a.Z = dims[2];
  const long long bx = (a.X + 3) / 4, by = (a.Y + 3) / 4, bz = (a.Z + 3) / 4;
  a.by = (unsigned int)by, a.bz = (unsigned int)bz;
  a.lanes = 64 * (bx * by * bz);  // <= 2^36
  a.num_views = num_views, a.H = cameras[0].height, a.W = cameras[0].width;
  a.depths = depths_dev, a.alphas = alphas_dev, a.images = images_dev;
  a.near = near, a.truncation = truncation, a.min_alpha = min_alpha;
  a.carve = (flags & RF_FUSE_CARVE) ? 1 : 0;
  a.tsdf_sum = tsdf_sum_dev, a.counts = (int2*)counts_dev, a.colour_sum = (float4*)colour_sum_dev;
  fill_view_cameras(a.cams, cameras, num_views);
  const dim3 grid((unsigned)((a.lanes + kFuseBlock - 1) / kFuseBlock)), block(kFuseBlock);  // <= 2^28 workgroups
  hipLaunchKernelGGL(fuse_depth_views_kernel, grid, block, 0, (hipStream_t)stream, a);
  return launch_status();
}

}  // extern "C"
