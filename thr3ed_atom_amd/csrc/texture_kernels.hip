// texture_kernels.hip -- texture baking of a field onto a triangle mesh (rf_texture_bake of relu_field.h): what
// thr3ed_atom_amd/texture.py is built on.  DESIGN.md section 21 has the contract, docs/texture_errors.md the error bound,
// tests/texture_model.py the float64 model.
//
// The atlas.  B = P + 4 texels square per BLOCK, block b at column (b % cols) B, row (b / cols) B of the image, triangles 2 b (lower)
// and 2 b + 1 (upper) in it.  Texel (i, j) of a block -- i the column, j the row, centre at (i, j) -- belongs to the lower triangle when
// i + j <= P + 3 and to the upper one otherwise; a triangle index >= T leaves the texel unowned (zeros in both images).  Along the
// patch's legs the texel sits at (a, b) = (i - 1, j - 1) from corner 0 of the lower patch and at (P + 2 - i, P + 2 - j) from corner 0 of
// the upper one (the lower patch turned by 180 degrees), beta1 = a / (P - 1), beta2 = b / (P - 1), beta0 = (1 - beta1) - beta2,
// p = (beta0 v0 + beta1 v1) + beta2 v2: the triangle's affine map, continued outside it.
//
// The texel.  n = the unit normal (v1 - v0) x (v2 - v0) or 0, S samples q_s = p + (reach - (s + 1/2) D) n, D = 2 reach / S, from outside
// inward; sigma_s = the renderer's activated density (0 on or outside the AABB), alpha_s = 1 - exp(-sigma_s D), w_s = alpha_s T_s,
// T_{s+1} = T_s (1 - alpha_s); colour c(x) = sigmoid(sum_k Y_k(-n) f_k(x)) on the zero-padded trilinear features (sigmoid(C0 f_0(x))
// under RF_FLAG_RENDER_DIFFUSE); texel = sum_s w_s c(q_s) + (1 - sum_s w_s) c(p), opacity = sum_s w_s.  No early termination; a
// sample with w_s == 0 skips its feature gathers (exactly nothing is lost).
//
// The kernel.  ONE launch, one lane per texel, block-major (lane order inside a block: j B + i), so that a wave covers at most four
// triangles of consecutive blocks and its gathers share cells (image-row-major lanes were measured and lost at the default patch:
// DESIGN.md section 21).  Every texel of both images is written once by its lane -- unowned ones with zeros, no memset, no atomics: two
// runs give the same bits.  The SH basis depends on the triangle alone and is evaluated once per lane.  Cell, corner and channel
// addressing are query_cell / query_corner / query_offset of rf_device.h; the kernel is instantiated per SH degree of the GRID so
// that query_offset's channel arithmetic folds at compile time, and under DIFFUSE only the k = 0 channels are addressed (the base
// record in split / bricked storage).  A face index outside [0, V) stores 1 to the status word and bakes zeros; it is never used
// as an address.
#include "texture_atlas.h"
#include "view_camera.h"

namespace {

constexpr int kBakeBlock = 256;
constexpr int kMinPatch = 2, kMaxPatch = 64;
constexpr int kMaxSamples = 256;

struct BakeArgs {
  const float* vertices;
  const long long* faces;
  long long num_vertices, num_faces;
  int patch, block, cols, rows;
  float reach;
  int samples;
  float* texture;
  float* opacity;  // or nullptr
  int* status;
};

struct TexelCell {
  int i0[3];
  float w0[3], w1[3];
};

// activated density of the cell's point (the density column of rf_grid_query)
__device__ __forceinline__ float bake_density(const GridArgs& g, const TexelCell& c) {
  float acc = 0.0f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const QueryCorner qc = query_corner(k, c.i0, c.w0, c.w1, g);
    if (qc.ok) {
      bool first;
      const long long off = query_offset(g.F, qc.lin, g, &first);
      float v = g.dens[off] * g.rho;
      if (g.mode == RF_DENSITY_ABS) v = fabsf(v);
      acc = acc + v * qc.w;
    }
  }
  return density_post(acc, g.mode);
}

// c(x) of the cell's point: KE = the coefficients per colour that enter (1 under DIFFUSE), K = the grid's
template <int K, int KE>
__device__ __forceinline__ void bake_colour(const GridArgs& g, const TexelCell& c, const float (&Y)[16], float (&rgb)[3]) {
  float raw[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const QueryCorner qc = query_corner(k, c.i0, c.w0, c.w1, g);
    if (qc.ok) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        float dot = 0.0f;
#pragma unroll
        for (int kk = 0; kk < KE; ++kk) {
          bool first;
          const long long off = query_offset(ch * K + kk, qc.lin, g, &first);
          const float v = first ? g.dens[off] : g.feat[off];
          dot = dot + Y[kk] * v;
        }
        raw[ch] = raw[ch] + dot * qc.w;
      }
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) rgb[ch] = sigmoidf_(raw[ch]);
}

template <int K, bool DIFFUSE>
__global__ __launch_bounds__(kBakeBlock) void texture_bake_kernel(GridArgs g_in, BakeArgs a) {
  constexpr int KE = DIFFUSE ? 1 : K;
  GridArgs g = g_in;
  g.F = 3 * K;  // (the host dispatched on it: a constant here, so that query_offset's divisions fold)
  const int B = a.block, P = a.patch;
  const long long total = ((long long)a.cols * B) * ((long long)a.rows * B);
  const long long t = (long long)blockIdx.x * kBakeBlock + threadIdx.x;
  if (t >= total) return;
  const AtlasTexel tx = atlas_texel(t, P, B, a.cols);  // texture_atlas.h: the map the view projection shares
  const long long pixel = tx.pixel;
  float out[3] = {0.0f, 0.0f, 0.0f}, opacity = 0.0f;
  bool owned = tx.tri < a.num_faces;
  unsigned long long vi[3] = {0ull, 0ull, 0ull};
  if (owned && !atlas_face(a.faces, a.num_vertices, tx.tri, vi)) {
    *a.status = 1;  // (a plain store of one value: whichever lane wins, the word reads 1)
    owned = false;
  }
  if (owned) {
    float p[3], n[3];
    atlas_point(a.vertices, vi, P, tx, p, n);
    float Y[16];
    sh_basis<KE>(-n[0], -n[1], -n[2], Y);  // d = -n: a camera that faces the surface
    const float delta = (2.0f * a.reach) / (float)a.samples;
    float T = 1.0f, wsum = 0.0f;
    for (int s = 0; s < a.samples; ++s) {
      const float ts = a.reach - ((float)s + 0.5f) * delta;
      float q[3];
#pragma unroll
      for (int x = 0; x < 3; ++x) q[x] = p[x] + ts * n[x];
      const bool inside = q[0] > g.amin[0] && q[0] < g.amax[0] && q[1] > g.amin[1] && q[1] < g.amax[1] && q[2] > g.amin[2] && q[2] < g.amax[2];
      if (!inside) continue;  // sigma = 0: alpha = 0, w = 0, T unchanged
      TexelCell c;
      query_cell(q, g, c.i0, c.w0, c.w1);
      const float sigma = bake_density(g, c);
      float E;
      const float alpha = occupancy_alpha(sigma * delta, E);
      const float w = alpha * T;
      T = T * E;
      if (w != 0.0f) {
        float rgb[3];
        bake_colour<K, KE>(g, c, Y, rgb);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out[ch] = out[ch] + w * rgb[ch];
        wsum = wsum + w;
      }
    }
    TexelCell c;
    query_cell(p, g, c.i0, c.w0, c.w1);
    float rgb[3];
    bake_colour<K, KE>(g, c, Y, rgb);
    const float rest = 1.0f - wsum;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out[ch] = out[ch] + rest * rgb[ch];
    opacity = wsum;
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) a.texture[3 * pixel + ch] = out[ch];
  if (a.opacity) a.opacity[pixel] = opacity;
}

}  // namespace

extern "C" {

int rf_texture_bake(const RFGrid* grid, const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces, int32_t patch,
                    int32_t cols, int32_t rows, float reach, int32_t samples, uint32_t flags, float* texture_dev, float* opacity_dev, int32_t* status_dev,
                    void* stream) {
  const int rc = check_grid(grid);
  if (rc == RF_ERR_NULL_POINTER) return rc;
  if (!texture_dev || !status_dev) return RF_ERR_NULL_POINTER;
  if ((num_vertices > 0 && !vertices_dev) || (num_faces > 0 && !faces_dev)) return RF_ERR_NULL_POINTER;
  if (rc == RF_ERR_BAD_SHAPE) return rc;
  if (num_vertices < 0 || num_faces < 0) return RF_ERR_BAD_SHAPE;
  if (patch < kMinPatch || patch > kMaxPatch) return RF_ERR_BAD_SHAPE;
  if (samples < 1 || samples > kMaxSamples) return RF_ERR_BAD_SHAPE;
  if (!(reach >= 0.0f) || !std::isfinite(reach)) return RF_ERR_BAD_SHAPE;
  if (cols < 1 || rows < 1) return RF_ERR_BAD_SHAPE;
  const int block = patch + 4;
  if ((long long)cols * block > kMaxImageEdge || (long long)rows * block > kMaxImageEdge) return RF_ERR_BAD_SHAPE;
  if (2ll * cols * rows < num_faces) return RF_ERR_BAD_SHAPE;
  if (rc != RF_OK) return rc;
  if (flags & ~(uint32_t)RF_FLAG_RENDER_DIFFUSE) return RF_ERR_UNSUPPORTED;
  BakeArgs a;
  a.vertices = vertices_dev, a.faces = (const long long*)faces_dev;
  a.num_vertices = num_vertices, a.num_faces = num_faces;
  a.patch = patch, a.block = block, a.cols = cols, a.rows = rows;
  a.reach = reach, a.samples = samples;
  a.texture = texture_dev, a.opacity = opacity_dev, a.status = status_dev;
  const GridArgs g = to_args(grid);
  const long long total = (long long)cols * block * rows * block;  // <= 2^28
  const dim3 blocks((unsigned)((total + kBakeBlock - 1) / kBakeBlock));
  const bool diffuse = (flags & RF_FLAG_RENDER_DIFFUSE) != 0;
  return dispatch_sh(g.F / 3, ShAll{}, [&](auto k) {
    constexpr int K = decltype(k)::value;
    if (diffuse)
      hipLaunchKernelGGL((texture_bake_kernel<K, true>), blocks, dim3(kBakeBlock), 0, (hipStream_t)stream, g, a);
    else
      hipLaunchKernelGGL((texture_bake_kernel<K, false>), blocks, dim3(kBakeBlock), 0, (hipStream_t)stream, g, a);
    return launch_status();
  });
}

}  // extern "C"
