// rf_device.h -- what the units of librelu_field_hip.so share: kernel argument structs, wave / math / sampling / cell helpers, the
// ray walk and sample-cache helpers of the per-ray kernels, and the host-side checks, marshalling and dispatch of the C ABI.
//
// PRIVATE to csrc/ (the public header is include/relu_field.h).  Included by relu_field_kernels.hip, grid_kernels.hip,
// ray_walk_kernels.hip, ray_grad_kernels.hip, mesh_kernels.hip and image_kernels.hip.  Everything lives in an anonymous namespace:
// each unit gets its own copy and every kernel keeps the mangled name it had when all of this was one file (profiles and
// tools/make_pmc_traffic.py key on those names).  A definition that only one unit uses belongs in that unit, not here.
//
// The traffic table profiles/pmc_traffic.json is tied to a hash of relu_field_kernels.hip ONLY.  A change here that alters a
// kernel of that file (tools/kernel_text_diff.py says whether it does) must regenerate the table (tools/profile_bench.sh).
//
// Numerics: the library is built with -ffp-contract=off, every multiply and add below rounds separately unless fmaf is written.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "relu_field.h"

namespace {

constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;
constexpr int kBlock = kWave * kWavesPerBlock;
constexpr float kInfinity = 1e10f;   // thre3d_atom/utils/constants.py:8
constexpr float kZeroPlus = 1e-10f;  // thre3d_atom/utils/constants.py:7

// real SH constants (utils/spherical_harmonics.py:33-52), rounded to float32 like torch does when a
// Python float multiplies a float32 tensor
constexpr float kC0 = 0.28209479177387814f;
constexpr float kC1 = 0.4886025119029199f;
constexpr float kC2_0 = 1.0925484305920792f;
constexpr float kC2_1 = -1.0925484305920792f;
constexpr float kC2_2 = 0.31539156525252005f;
constexpr float kC2_3 = -1.0925484305920792f;
constexpr float kC2_4 = 0.5462742152960396f;
constexpr float kC3_0 = -0.5900435899266435f;
constexpr float kC3_1 = 2.890611442640554f;
constexpr float kC3_2 = -0.4570457994644658f;
constexpr float kC3_3 = 0.3731763325901154f;
constexpr float kC3_4 = -0.4570457994644658f;
constexpr float kC3_5 = 1.445305721320277f;
constexpr float kC3_6 = -0.5900435899266435f;

struct GridArgs {
  const float* dens;
  const float* feat;
  const uint32_t* occ;
  int X, Y, Z, F;
  long long dstride, fstride;
  float amin[3], amax[3], nscale[3], nbias[3];
  float rho;
  int mode;
  int layout;  // channel arrangement. RF_LAYOUT_REFERENCE: dens[.,1] + feat[.,F];  RF_LAYOUT_SPLIT: dens = base[.,4], feat = rest[.,F-3]
  // node order: linear (x, y, z) with z fastest, or (RF_LAYOUT_BRICKED) brick-major: 8^3-node bricks stored contiguously,
  // brick (bx, by, bz) at ((bx * nby + by) * nbz + bz) * 512, node (x & 7, y & 7, z & 7) inside it with z fastest
  int bricked;
  int nby, nbz;
  unsigned int step[3];  // index step to the next node along x, y, z (inside a brick for the bricked order)
  unsigned int jump[3];  // bricked: step from the last node of a brick to the first node of the next brick on that axis
  // "near" addressing (host-checked: <= 2^24 nodes, byte strides < 2^24, both tensors inside one 4 GB window that starts at `base`):
  // a corner's address = uniform 64-bit base (scalar registers) + 32-bit byte offset built with full-rate 24-bit multiplies, instead
  // of a 64-bit multiply-add per corner -- the gathers of the render kernels are bound by vector-ALU issue, not by memory
  const char* base;
  unsigned int dens_off, feat_off;  // byte offsets of dens / feat from base
  int near32;
};

// index of node (x, y, z) in the grid tensors (to be multiplied by the tensor's channel stride)
__device__ __forceinline__ unsigned int node_lin(const GridArgs& g, int x, int y, int z) {
  if (g.bricked)
    return (__umul24(__umul24((unsigned)(x >> 3), (unsigned)g.nby) + (unsigned)(y >> 3), (unsigned)g.nbz) + (unsigned)(z >> 3)) * 512u +
           (unsigned)(((x & 7) << 6) | ((y & 7) << 3) | (z & 7));
  return __umul24(__umul24((unsigned)x, (unsigned)g.Y) + (unsigned)y, (unsigned)g.Z) + (unsigned)z;
}

struct RayArgs {
  const float* origins;
  const float* directions;
  long long n;
  int S;
  float near, far;
  const float* tvals;
  const float* trand;
  // keyed jitter (RF_FLAG_JITTER_KEYED, trand == NULL): u(ray, sample) = hash of (key, ray0 + ray, sample) -- no [N,S] tensor
  unsigned long long jkey;
  long long ray0;  // global index of ray 0 of this batch (jitter stream; pixel index when the camera generates the rays)
  int jitter;
  // rays generated in-kernel from a pinhole camera (origins == NULL): ray r = pixel ray0 + r, row-major
  int cam;
  int H, W;
  float focal;
  float pose[12];  // [3,4] = rotation | translation (camera-to-world)
};

struct OutArgs {
  float* colour;
  float* depth;
  float* acc;
  float* disparity;
  // per-sample cache of the samples that can carry gradient (`need`: inside, T != 0, sigma != 0 under ReLU), COMPACTED per chunk of
  // 64 samples: the j-th such sample of chunk c of ray r sits at slot r * S + 64 c + j, and bit l of cmask[r][c] says that sample
  // 64 c + l is one of them -- the adjoint kernels read nothing else (every other sample contributes exactly nothing)
  float* cache;                // [N,S,4] (raw r, g, b, sigma)
  float* tcache;               // [N,S] transmittance
  unsigned long long* cmask;   // [N, ceil(S / 64)]
  int* stop;                   // [N]
  // binned backward, fused binning: the forward pass counts, per (brick, flags) key, the samples that will emit a record
  int* hist;        // [8 * nbricks] or NULL
  int brick_shift;  // log2 of the brick edge (nodes)
  int nby, nbz;     // bricks along y and z
};

struct GradArgs {
  const float* gcolour;
  const float* gdepth;
  const float* gacc;
  float* gdens;
  float* gfeat;
  // emit mode (binned backward): per-sample records instead of a scatter
  short* keys;      // [N*S] brick id of the sample's cell, kNoBrick for samples without gradient
  float* records;   // [N*S, 4 * record_quads] the record of every keyed slot (formats: record_quads), in slot order
  int brick_shift;  // log2 of the brick edge (nodes)
  int nby, nbz;     // bricks along y and z
  int* hist;        // [8 * nbricks] records per key, added to (may be NULL)
  // direct mode (EMIT == 2): expanded records written straight to their final position
  int* cursor;      // [8 * nbricks] next free position per key
  float4* sorted;   // [capacity, record_quads(K)]
  int* hist_clear;  // counters of the forward pass to clear for the next iteration (may be NULL)
  int nkeys;
};

// ---------------------------------------------------------------------------------------------
// wave-level helpers (64 lanes)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void wave_lds_fence() {
  // LDS traffic of one wave is executed in order; this only stops the compiler from moving LDS accesses
  // across the phase boundary.
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// DPP cross-lane move: lanes without a source (or masked out by ROW_MASK) keep `old`
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_move(float old, float src) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, src),
                                                               CTRL, ROW_MASK, 0xf, false));
}
constexpr int kDppRowShr1 = 0x111, kDppRowShr2 = 0x112, kDppRowShr4 = 0x114, kDppRowShr8 = 0x118;
constexpr int kDppRowBcast15 = 0x142, kDppRowBcast31 = 0x143, kDppWaveShr1 = 0x138, kDppWaveShl1 = 0x130;

// Inclusive prefix of a chunk's transmittance factors E_j = 1 - alpha_j, carried in BOTH forms: e = prod E_j and a = 1 - prod E_j (joined
// as a' = a_prefix + a e_prefix).  The product alone is as accurate as torch.cumprod's sequential one in the worst case, but not on
// the rays that matter at high sample counts: with a slowly varying density the factors of neighbouring samples are (nearly) the SAME
// float, the first doubling step rounds all of them the same way and the later steps multiply that error by 32 per chunk -- coherent
// over a ray, where the sequential product's roundings are not: 1000 samples of alpha ~ 1e-4 left the transmittance 1e-5 low (accumulated
// weight of a ray that ends inside the volume 0.99999 instead of 1, depth 6e-5 off: tests/parity_fuzz.py kind "long"; the float32
// reference is within 1e-6 of the float64 value there).  In the `a` form the same roundings are relative to a ~ 1e-4 .. 1e-2, not to 1.
// prefix_transmittance() takes 1 - a while a < 1/4 and the product beyond (exact zeros behind an opaque sample stay exact; a ray
// passes through few chunks in that regime).  DPP (gfx9): 4 row_shr steps inside each row of 16 lanes, then row_bcast:15 / :31 to fold
// the rows; 24 VALU instructions per chunk (the product alone took 6), no LDS traffic.
__device__ __forceinline__ void wave_incl_scan_trans(float& e, float& a) {
  auto step = [&](auto ctrl_tag, auto mask_tag) {
    constexpr int CTRL = decltype(ctrl_tag)::value, MASK = decltype(mask_tag)::value;
    const float ep = dpp_move<CTRL, MASK>(1.0f, e), ap = dpp_move<CTRL, MASK>(0.0f, a);
    a = __builtin_fmaf(a, ep, ap);
    e = e * ep;
  };
  step(std::integral_constant<int, kDppRowShr1>{}, std::integral_constant<int, 0xf>{});
  step(std::integral_constant<int, kDppRowShr2>{}, std::integral_constant<int, 0xf>{});
  step(std::integral_constant<int, kDppRowShr4>{}, std::integral_constant<int, 0xf>{});
  step(std::integral_constant<int, kDppRowShr8>{}, std::integral_constant<int, 0xf>{});
  step(std::integral_constant<int, kDppRowBcast15>{}, std::integral_constant<int, 0xa>{});
  step(std::integral_constant<int, kDppRowBcast31>{}, std::integral_constant<int, 0xc>{});
}
__device__ __forceinline__ float prefix_transmittance(float e, float a) { return (a < 0.25f) ? 1.0f - a : e; }

__device__ __forceinline__ float read_lane(float x, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), lane));
}

// inclusive SUFFIX sum: result[lane] = sum_{l >= lane} x[l]
__device__ __forceinline__ float wave_incl_rscan_add(float x, int lane) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    float y = __shfl_down(x, off, kWave);
    if (lane + off < kWave) x = x + y;
  }
  return x;
}

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, kWave);
  return x;
}

// exp / sigmoid on the hardware transcendental units (v_exp_f32 is 2^x, v_rcp_f32; ~1 ulp each).  The reference's
// own CPU (SLEEF) and GPU (libdevice) paths differ from each other by as much; the parity bar is 1e-5.
__device__ __forceinline__ float exp_fast(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }
__device__ __forceinline__ float sigmoidf_(float x) { return __builtin_amdgcn_rcpf(1.0f + exp_fast(-x)); }
// alpha = 1 - exp(-x), x = sigma * delta (density2occupancy_pb, accumulate.py:24-28; x < 0 only under Identity/Identity densities, where
// alpha < 0 and the transmittance grows above 1), the way the REFERENCE's float32 arithmetic
// produces it: E = exp(-x) correctly rounded, alpha = 1 - E (an exact subtraction: alpha is a multiple of 2^-24 and 1 - alpha == E, so
// that weights alpha_i T_i and transmittances T_i E_i telescope without a bias).  v_exp_f32 is a one-ulp exponential: at the small x of
// densely sampled rays (1000+ samples: x ~ 1e-3) its errors in E near 1 showed as 3..8e-5 on depth at 4000 .. 5000 samples per ray, where the
// float32 reference stays within 2e-6 of the float64 value (tests/parity_fuzz.py, kind "long").  Below 1/16: E = 1 - (x - x^2/2 + ... ),
// the series to 2e-9 relative, i.e. the correctly rounded exponential in all but a handful of cases.  (alpha taken from the series
// itself is MORE accurate than the reference's -- and then 1 - alpha is rounded, with the same sign sample after sample where the
// density varies slowly: accumulated weights of opaque rays came out 1.5e-5 short of 1.  Measured, not kept.)  The series is taken for
// |x| < 1/16 only: truncated, it falls away from exp(-x) fast on the negative side (1.4e-5 relative at x = -0.5, 0.93 at x = -10), and
// exp_fast is right for either sign (+inf for a negative density over the last sample's 1e10-long interval, as in the reference).
__device__ __forceinline__ float occupancy_alpha(float x, float& E) {
  float t = __builtin_fmaf(-x, 1.0f / 120.0f, 1.0f / 24.0f);
  t = __builtin_fmaf(-x, t, 1.0f / 6.0f);
  t = __builtin_fmaf(-x, t, 0.5f);
  t = __builtin_fmaf(-x, t, 1.0f);
  const float big = exp_fast(-x);
  E = (__builtin_fabsf(x) < 0.0625f) ? __builtin_fmaf(-x, t, 1.0f) : big;
  return 1.0f - E;
}
// softplus'(x) = sigmoid(x) = 1 - exp(-softplus(x)), from the cached activated density s = softplus(x) >= 0, to RELATIVE accuracy: a
// sample far below the surface has s ~ 1e-9 and 1 - exp(-s) cancels to 0 in float32, but the last sample of a ray carries
// delta = 1e10 |d| (accumulate.py:49-52), so its d alpha / d sigma is ~1e10 and the product is an ordinary gradient that the reference
// (ATen's softplus backward: z / (z + 1), z = exp(x)) gets right.  Below 0.25 the alternating series, six terms (next term / s < 5e-8).
__device__ __forceinline__ float softplus_slope(float s) {
  if (s < 0.25f) return s * (1.0f - s * (0.5f - s * (1.0f / 6.0f - s * (1.0f / 24.0f - s * (1.0f / 120.0f - s * (1.0f / 720.0f))))));
  return 1.0f - exp_fast(-s);
}
// dL/d(pre-activation density) from dL/d(sigma) and the cached activated density: ReLU passes it where sigma > 0, softplus scales
// it by its slope, Abs (whose sign is applied per corner) and Identity pass it on
__device__ __forceinline__ float density_pre_grad(float g_sigma, float sigma, int mode) {
  if (mode == RF_DENSITY_RELU) return (sigma > 0.0f) ? g_sigma : 0.0f;
  if (mode == RF_DENSITY_SOFTPLUS) return g_sigma * softplus_slope(sigma);
  return g_sigma;
}

// The compositing weights of one 64-sample chunk, lanes = samples: alpha = 1 - exp(-sigma delta) of the lane's sample (E = 1 - alpha
// exactly; density2occupancy_pb, accumulate.py:24-28), the two-form transmittance scan over the chunk's valid samples, and
// T = T_carry * the product of the E in front of the lane, so that w = alpha * T.  `incl` is the inclusive prefix: lane 63's carries T
// into the next chunk.  The forward render and every walk that must reproduce its weights bit for bit go through here.
struct ChunkWeights {
  float alpha, E, incl, T;
};
__device__ __forceinline__ ChunkWeights chunk_weights(float sigma, float delta, bool valid, float T_carry) {
  ChunkWeights c;
  c.alpha = occupancy_alpha(sigma * delta, c.E);
  float incl_e = valid ? c.E : 1.0f, incl_a = valid ? c.alpha : 0.0f;
  wave_incl_scan_trans(incl_e, incl_a);
  c.incl = prefix_transmittance(incl_e, incl_a);
  const float excl = dpp_move<kDppWaveShr1, 0xf>(1.0f, c.incl);  // lane i <- lane i-1, lane 0 <- 1
  c.T = T_carry * excl;
  return c;
}

// ---------------------------------------------------------------------------------------------
// sampling (rendering/volumetric/sample.py:39-68)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float z_uniform(float near, float far, float t) { return near * (1.0f - t) + far * t; }

// jitter u in [0, 1) of sample s, or no jitter at all (have_u = false)
__device__ __forceinline__ float z_sample(const float* __restrict__ tv, bool have_u, float u, int s, int S, float near, float far) {
  const float zc = z_uniform(near, far, tv[s]);
  if (!have_u) return zc;
  // stratified jitter: lower/upper = neighbouring mid-points (sample.py:57-64).  (The neighbours are loaded unconditionally, with
  // clamped indices: a load under a lane condition is merged with a copy, and the copy waits for the load on the spot.)
  const float zm = z_uniform(near, far, tv[s > 0 ? s - 1 : 0]), zp = z_uniform(near, far, tv[s < S - 1 ? s + 1 : S - 1]);
  const float lo = (s > 0) ? 0.5f * (zc + zm) : zc;
  const float hi = (s < S - 1) ? 0.5f * (zp + zc) : zc;
  return lo + (hi - lo) * u;
}

// slab test of sample.py:71-184; returns true when the ray hits, writes the (clamped) bounds either way
__device__ __forceinline__ bool ray_box(const float o[3], const float d[3], const float bmin[3], const float bmax[3],
                                        float near, float far, float& t0, float& t1) {
  float lo_run = 0.f, hi_run = 0.f;
  bool hit = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float den = d[a] + kZeroPlus;
    const float ta = (bmin[a] - o[a]) / den;
    const float tb = (bmax[a] - o[a]) / den;
    const bool swap = ta > tb;
    const float lo = swap ? tb : ta;
    const float hi = swap ? ta : tb;
    if (a == 0) {
      lo_run = lo;
      hi_run = hi;
    } else {
      hit = hit && !((lo_run > hi) || (lo > hi_run));
      lo_run = (lo > lo_run) ? lo : lo_run;
      hi_run = (hi < hi_run) ? hi : hi_run;
    }
  }
  t0 = hit ? lo_run : near;
  t1 = hit ? hi_run : far;
  t0 = (t0 < 0.f) ? 0.f : t0;  // torch.clip(min=0): NaN stays NaN, like the reference
  t1 = (t1 < 0.f) ? 0.f : t1;
  return hit;
}

// ---------------------------------------------------------------------------------------------
// per-sample geometry (voxels.py:214-223 normalise, GridSampler.h:27-36 un-normalise)
// ---------------------------------------------------------------------------------------------
struct Cell {
  float idx[3];  // continuous index ((q + 1) * size - 1) / 2
  int i0[3];     // floor of the continuous index (may be -1)
  float w0[3];   // weight of the lower node along each axis  = (i0 + 1) - idx
  float w1[3];   // weight of the upper node                   = idx - i0
};

__device__ __forceinline__ Cell locate(const float p[3], const GridArgs& g) {
  Cell c;
  const int dims[3] = {g.X, g.Y, g.Z};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float q = p[a] * g.nscale[a] + g.nbias[a];
    const float idx = ((q + 1.0f) * (float)dims[a] - 1.0f) / 2.0f;
    const float fl = floorf(idx);
    c.idx[a] = idx;
    c.i0[a] = (int)fl;
    c.w1[a] = idx - fl;
    c.w0[a] = (fl + 1.0f) - idx;
  }
  return c;
}

__device__ __forceinline__ uint32_t pack_cell(const Cell& c) {
  return (uint32_t)(c.i0[0] + 1) | ((uint32_t)(c.i0[1] + 1) << 11) | ((uint32_t)(c.i0[2] + 1) << 22);
}

struct Corners {
  unsigned int lin[8];  // linear voxel index of the (clamped) corner k = dx + 2 dy + 4 dz
  unsigned int s[3];    // index steps from corner 000 to its x / y / z upper neighbour (0 where clamping collapses them)
  float w[8];           // trilinear weight, forced to 0 for corners outside the grid
};

// grid dims <= 2046, so every product below has 24-bit operands (v_mul_u32_u24 runs at full rate, v_mul_lo_u32 does
// not); voxel counts are limited to 2^32 / stride by the host-side check.
__device__ __forceinline__ Corners corners_of(uint32_t packed, const float wts[6], const GridArgs& g) {
  const int ix0 = (int)(packed & 0x7ffu) - 1, iy0 = (int)((packed >> 11) & 0x7ffu) - 1, iz0 = (int)(packed >> 22) - 1;
  const bool okx[2] = {ix0 >= 0, ix0 + 1 < g.X};  // the point is inside the box: ix0 in [-1, X-1]
  const bool oky[2] = {iy0 >= 0, iy0 + 1 < g.Y};
  const bool okz[2] = {iz0 >= 0, iz0 + 1 < g.Z};
  const int cx0 = max(ix0, 0), cy0 = max(iy0, 0), cz0 = max(iz0, 0);
  const unsigned int lin0 = node_lin(g, cx0, cy0, cz0);
  // step to the upper node: a whole voxel (a jump into the next brick when the lower node is a brick's last one), or 0
  // when the clamped upper node coincides with the lower one
  const unsigned int sx = (okx[0] && okx[1]) ? ((g.bricked && (cx0 & 7) == 7) ? g.jump[0] : g.step[0]) : 0u;
  const unsigned int sy = (oky[0] && oky[1]) ? ((g.bricked && (cy0 & 7) == 7) ? g.jump[1] : g.step[1]) : 0u;
  const unsigned int sz = (okz[0] && okz[1]) ? ((g.bricked && (cz0 & 7) == 7) ? g.jump[2] : g.step[2]) : 0u;
  // (a node outside the grid gets weight 0: masked per axis -- 0 times the finite weights of the other axes is the same +0)
  const float ax[2] = {okx[0] ? wts[0] : 0.0f, okx[1] ? wts[1] : 0.0f};
  const float ay[2] = {oky[0] ? wts[2] : 0.0f, oky[1] ? wts[3] : 0.0f};
  const float az[2] = {okz[0] ? wts[4] : 0.0f, okz[1] ? wts[5] : 0.0f};
  const float wxy[4] = {ax[0] * ay[0], ax[1] * ay[0], ax[0] * ay[1], ax[1] * ay[1]};  // [dx + 2 dy]
  Corners c;
  c.s[0] = sx;
  c.s[1] = sy;
  c.s[2] = sz;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
    c.lin[k] = lin0 + (dx ? sx : 0u) + (dy ? sy : 0u) + (dz ? sz : 0u);
    c.w[k] = wxy[dx + 2 * dy] * az[dz];
  }
  return c;
}

__device__ __forceinline__ float density_post(float pre, int mode) {
  if (mode == RF_DENSITY_RELU) return fmaxf(pre, 0.0f);
  if (mode == RF_DENSITY_SOFTPLUS) return (pre > 20.0f) ? pre : log1pf(expf(pre));
  return pre;
}

// density: post( interp( pre(D * rho) ) )  (voxels.py:292-309)
// v[k]: the 8 pre-activation corner values themselves (rf_render_geometry differentiates the interpolant with them)
__device__ __forceinline__ float interp_density_values(const Corners& c, const GridArgs& g, float v[8], float& pre_out) {
  float raw[8];
  if (g.near32) {  // (wave-uniform)
    const unsigned int sb = (unsigned int)g.dstride * 4u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const unsigned int o = __umul24(c.lin[k], sb);
      raw[k] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(g.dens) + (size_t)o);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) raw[k] = g.dens[c.lin[k] * g.dstride];
    asm volatile("" ::: "memory");  // (keeps the two branches' loads apart: merged, they lose the scalar-base addressing)
  }
  float acc = 0.0f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    v[k] = raw[k] * g.rho;
    if (g.mode == RF_DENSITY_ABS) v[k] = fabsf(v[k]);
    acc = acc + v[k] * c.w[k];
  }
  pre_out = acc;
  return density_post(acc, g.mode);
}
__device__ __forceinline__ float interp_density(const Corners& c, const GridArgs& g, float& pre_out) {
  float v[8];
  return interp_density_values(c, g, v, pre_out);
}

// signed SH basis in the reference's operation order (utils/spherical_harmonics.py:86-116)
template <int K>
__device__ __forceinline__ void sh_basis(float x, float y, float z, float Y[16]) {
  Y[0] = kC0;
  if (K > 1) {
    Y[1] = -(kC1 * y);
    Y[2] = kC1 * z;
    Y[3] = -(kC1 * x);
  }
  if (K > 4) {
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    Y[4] = kC2_0 * xy;
    Y[5] = kC2_1 * yz;
    Y[6] = kC2_2 * ((2.0f * zz - xx) - yy);
    Y[7] = kC2_3 * xz;
    Y[8] = kC2_4 * (xx - yy);
    if (K > 9) {
      Y[9] = (kC3_0 * y) * (3.0f * xx - yy);
      Y[10] = (kC3_1 * xy) * z;
      Y[11] = (kC3_2 * y) * ((4.0f * zz - xx) - yy);
      Y[12] = (kC3_3 * z) * ((2.0f * zz - 3.0f * xx) - 3.0f * yy);
      Y[13] = (kC3_4 * x) * ((4.0f * zz - xx) - yy);
      Y[14] = (kC3_5 * z) * (xx - yy);
      Y[15] = (kC3_6 * x) * (xx - 3.0f * yy);
    }
  }
}

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352dU;
  x ^= x >> 15;
  x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}

// Keyed jitter of the stratified sampler (sample.py:57-64 draws torch.rand(N, S)): a counter-based generator instead of a
// [N, S] tensor.  u = 24 random bits of mix32 over (per-ray seed, sample index); the per-ray seed hashes the 64-bit key with
// the global ray index.  Restated in oracle/relu_field_oracle.py:keyed_jitter (tests compare the two bit for bit).
__device__ __forceinline__ uint32_t jitter_ray_seed(unsigned long long key, long long gray) {
  const uint32_t a = mix32((uint32_t)gray ^ (uint32_t)key);
  const uint32_t b = mix32((uint32_t)((unsigned long long)gray >> 32) + (uint32_t)(key >> 32));
  return a ^ (b * 0x9E3779B9u + 0x85EBCA6Bu);
}
__device__ __forceinline__ float jitter_uniform(uint32_t ray_seed, int s) {
  const uint32_t h = mix32(ray_seed + (uint32_t)s * 0x9E3779B9u);
  return (float)(h >> 8) * 5.9604644775390625e-08f;  // [0, 1) on the 2^-24 lattice
}

__device__ __forceinline__ void pixel_ray(int i, int j, int H, int W, float focal, const float* R, float d[3]) {
  // pixel centres; camera looks along -z, y up
  const float cx = (((float)j + 0.5f) - (float)W * 0.5f) / focal;
  const float cy = -((((float)i + 0.5f) - (float)H * 0.5f) / focal);
  const float cz = -1.0f;
#pragma unroll
  for (int a = 0; a < 3; ++a) d[a] = (R[a * 3 + 0] * cx + R[a * 3 + 1] * cy) + R[a * 3 + 2] * cz;
}

// ---------------------------------------------------------------------------------------------
// per-ray state shared by forward and backward
// ---------------------------------------------------------------------------------------------
struct RayState {
  float o[3], d[3];
  float dnorm;
  float near, far;
  uint32_t jseed;  // keyed jitter: per-ray seed
};

__device__ __forceinline__ RayState load_ray(const RayArgs& r, const GridArgs& g, long long ray, uint32_t flags) {
  RayState st;
  if (r.cam) {  // cast_rays (utils/misc.py:12-50) fused: pixel p = ray0 + ray, row-major
    const long long pidx = r.ray0 + ray;
    const int i = (int)(pidx / r.W), j = (int)(pidx - (long long)i * r.W);
    const float R[9] = {r.pose[0], r.pose[1], r.pose[2], r.pose[4], r.pose[5], r.pose[6], r.pose[8], r.pose[9], r.pose[10]};
    pixel_ray(i, j, r.H, r.W, r.focal, R, st.d);
    st.o[0] = r.pose[3];
    st.o[1] = r.pose[7];
    st.o[2] = r.pose[11];
  } else {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      st.o[a] = r.origins[ray * 3 + a];
      st.d[a] = r.directions[ray * 3 + a];
    }
  }
  st.jseed = r.jitter ? jitter_ray_seed(r.jkey, r.ray0 + ray) : 0u;
  st.dnorm = sqrtf((st.d[0] * st.d[0] + st.d[1] * st.d[1]) + st.d[2] * st.d[2]);
  st.near = r.near;
  st.far = r.far;
  if (flags & RF_FLAG_AABB_SAMPLING) {
    float t0, t1;
    ray_box(st.o, st.d, g.amin, g.amax, r.near, r.far, t0, t1);
    st.near = t0;
    st.far = t1;
  }
  return st;
}

// everything P0 knows about one sample
struct Sample {
  float z, delta;
  bool valid, inside;
  Cell cell;
};

// the sample of lane-index s given its ray parameter z and the next sample's parameter z_next
__device__ __forceinline__ Sample sample_at(const RayState& st, const RayArgs& r, const GridArgs& g, int s, float z,
                                            float z_next) {
  Sample sm;
  sm.valid = s < r.S;
  sm.z = z;
  sm.delta = (s < r.S - 1) ? (z_next - z) * st.dnorm : kInfinity * st.dnorm;  // accumulate.py:50-55
  float p[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) p[a] = st.o[a] + st.d[a] * sm.z;
  sm.inside = sm.valid && p[0] > g.amin[0] && p[0] < g.amax[0] && p[1] > g.amin[1] && p[1] < g.amax[1] &&
              p[2] > g.amin[2] && p[2] < g.amax[2];  // strict, voxels.py:252-274
  sm.cell = locate(p, g);
  return sm;
}

__device__ __forceinline__ float z_of(const RayState& st, const RayArgs& r, long long ray, int s) {
  const int sc = min(s, r.S - 1);
  float u = 0.0f;
  if (r.trand)
    u = r.trand[ray * (long long)r.S + sc];
  else if (r.jitter)
    u = jitter_uniform(st.jseed, sc);
  return z_sample(r.tvals, r.trand != nullptr || r.jitter, u, sc, r.S, st.near, st.far);
}

// z_of in two halves, for kernels that want every load of several samples in flight before the first one is used:
// z_requests issues the (unconditional, clamped) t_vals reads, z_from does z_of's arithmetic on them -- bit for bit the same value.
struct ZRequests {
  float t0, tm, tp;
};
__device__ __forceinline__ ZRequests z_requests(const RayArgs& r, int s) {
  const int sc = min(s, r.S - 1);
  ZRequests q;
  q.t0 = r.tvals[sc];
  q.tm = r.tvals[sc > 0 ? sc - 1 : 0];
  q.tp = r.tvals[sc < r.S - 1 ? sc + 1 : r.S - 1];
  return q;
}
// (a jitter TABLE, if one is used instead of the keyed generator, is read here, synchronously)
__device__ __forceinline__ float z_from(const RayState& st, const RayArgs& r, const ZRequests& q, long long ray, int s) {
  const int sc = min(s, r.S - 1);
  const float zc = z_uniform(st.near, st.far, q.t0);
  if (!(r.trand != nullptr || r.jitter)) return zc;
  const float u = r.trand ? r.trand[ray * (long long)r.S + sc] : jitter_uniform(st.jseed, sc);
  const float zm = z_uniform(st.near, st.far, q.tm), zp = z_uniform(st.near, st.far, q.tp);
  const float lo = (sc > 0) ? 0.5f * (zc + zm) : zc;
  const float hi = (sc < r.S - 1) ? 0.5f * (zp + zc) : zc;
  return lo + (hi - lo) * u;
}

__device__ __forceinline__ Sample make_sample(const RayState& st, const RayArgs& r, const GridArgs& g, long long ray,
                                              int s) {
  return sample_at(st, r, g, s, z_of(st, r, ray, s), z_of(st, r, ray, s + 1));
}

__device__ __forceinline__ bool cell_occupied(const Cell& c, const GridArgs& g) {
  // bit index over the (X+1)(Y+1)(Z+1) cells whose lower node is i0 in [-1, dim-1]
  const long long bit = ((long long)(c.i0[0] + 1) * (g.Y + 1) + (c.i0[1] + 1)) * (g.Z + 1) + (c.i0[2] + 1);
  return (g.occ[bit >> 5] >> (bit & 31)) & 1u;
}

// Parameter interval of a ray inside the box (same slab test as the AABB sampler, reciprocal-based: only used with a generous
// margin, never for sample positions).  A chunk of 64 samples that lies outside it by that margin contributes exactly
// nothing -- sigma = 0 -> alpha = 0 -> w = 0, T unchanged, no gradient -- and is skipped without evaluating a single sample.
struct BoxSpan {
  float t_in, t_out, zpad, margin;
  bool hits;
};

__device__ __forceinline__ BoxSpan box_span(const RayState& st, const RayArgs& r, const GridArgs& g) {
  BoxSpan b;
  b.t_in = -kInfinity;
  b.t_out = kInfinity;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float inv = __builtin_amdgcn_rcpf(st.d[a] + kZeroPlus);
    const float ta = (g.amin[a] - st.o[a]) * inv, tb = (g.amax[a] - st.o[a]) * inv;
    b.t_in = fmaxf(b.t_in, fminf(ta, tb));
    b.t_out = fminf(b.t_out, fmaxf(ta, tb));
  }
  b.margin = 1e-3f * (1.0f + fabsf(b.t_in) + fabsf(b.t_out));
  b.hits = b.t_out >= b.t_in - b.margin;
  b.zpad = fabsf(st.far - st.near) / (float)(r.S > 1 ? r.S - 1 : 1);  // jitter stays within one stratum
  return b;
}

// wave-uniform: no sample of chunk `chunk` can be inside the box
__device__ __forceinline__ bool chunk_outside_box(const BoxSpan& b, const RayState& st, const RayArgs& r, int chunk) {
  const int s_first = chunk * kWave, s_last = min(r.S - 1, chunk * kWave + kWave - 1);
  const float za = z_uniform(st.near, st.far, r.tvals[s_first]), zb = z_uniform(st.near, st.far, r.tvals[s_last]);
  const float zlo = fminf(za, zb) - b.zpad, zhi = fmaxf(za, zb) + b.zpad;
  return !b.hits || zhi < b.t_in - b.margin || zlo > b.t_out + b.margin;
}

// The cached samples of a chunk (forward pass, SAVE): lane l of the adjoint handles sample 64 c + l like the forward pass did; its
// cache entry, if bit l of the chunk's mask is set, is entry rank(l) = popcount(mask below l) of the chunk's slots.  Lanes without
// an entry load entry 0 of the chunk (a line the wave touches anyway; a load under a lane condition would be followed by a
// register merge that waits for it) and are zeroed by the caller.
__device__ __forceinline__ long long cached_slot(long long ray, int S, int chunk, unsigned long long cm, int lane) {
  const bool has = (cm >> lane) & 1ull;
  const int rank = __popcll(cm & ((1ull << lane) - 1ull));
  return ray * (long long)S + chunk * kWave + (has ? rank : 0);
}
// wave-uniform mask of chunk `chunk` out of the per-lane copies (lane c holds chunk 64 g + c)
__device__ __forceinline__ unsigned long long chunk_mask_of(unsigned long long lanes_masks, int chunk) {
  const int c = chunk & (kWave - 1);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)lanes_masks, c);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(lanes_masks >> 32), c);
  return ((unsigned long long)hi << 32) | lo;
}

// cell and corner addressing of the stand-alone point query (grid_kernels.hip) and of its point adjoint (ray_grad_kernels.hip)
struct QueryCorner {
  long long lin;
  float w;
  bool ok;
};

__device__ __forceinline__ void query_cell(const float p[3], const GridArgs& g, int i0[3], float w0[3], float w1[3]) {
  const int dims[3] = {g.X, g.Y, g.Z};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float q = p[a] * g.nscale[a] + g.nbias[a];
    const float idx = ((q + 1.0f) * (float)dims[a] - 1.0f) / 2.0f;
    const float fl = floorf(idx);
    w1[a] = idx - fl;
    w0[a] = (fl + 1.0f) - idx;
    // far-away points: every corner is outside anyway; clamp so that the integer conversion is defined
    i0[a] = (int)fminf(fmaxf(fl, -2.0f), (float)dims[a]);
  }
}

__device__ __forceinline__ QueryCorner query_corner(int k, const int i0[3], const float w0[3], const float w1[3],
                                                    const GridArgs& g) {
  const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
  const int ix = i0[0] + dx, iy = i0[1] + dy, iz = i0[2] + dz;
  QueryCorner c;
  c.ok = ix >= 0 && ix < g.X && iy >= 0 && iy < g.Y && iz >= 0 && iz < g.Z;
  c.lin = node_lin(g, min(max(ix, 0), g.X - 1), min(max(iy, 0), g.Y - 1), min(max(iz, 0), g.Z - 1));
  c.w = ((dx ? w1[0] : w0[0]) * (dy ? w1[1] : w0[1])) * (dz ? w1[2] : w0[2]);
  return c;
}

// element offset of output channel c of voxel `lin` inside the tensor that holds it; *in_first = it is the
// densities/base tensor rather than the features/rest tensor
__device__ __forceinline__ long long query_offset(int c, long long lin, const GridArgs& g, bool* in_first) {
  const int F = g.F, K = F / 3;
  if (c == F) {
    *in_first = true;
    return lin * g.dstride;
  }
  if (g.layout == RF_LAYOUT_SPLIT) {
    const int ch = c / K, k = c % K;
    if (k == 0) {
      *in_first = true;
      return lin * g.dstride + 1 + ch;
    }
    *in_first = false;
    return lin * g.fstride + ch * (K - 1) + (k - 1);
  }
  *in_first = false;
  return lin * g.fstride + c;
}

// ---------------------------------------------------------------------------------------------
// host side of the C ABI
// ---------------------------------------------------------------------------------------------
// split / bricked storage at SH degree 0 keeps all four channels in the first tensor: the second tensor -- parameters or
// gradients -- may then be null
bool second_tensor_optional(const RFGrid* g) { return g->layout != RF_LAYOUT_REFERENCE && g->num_features == 3; }

// the node count, every axis padded to whole 8-node bricks where `whole_bricks` says so
unsigned long long node_count(const RFGrid* g, bool whole_bricks) {
  unsigned long long nodes = 1;
  for (int a = 0; a < 3; ++a) nodes *= (unsigned long long)(whole_bricks ? (g->dims[a] + 7) / 8 * 8 : g->dims[a]);
  return nodes;
}

// an A/B switch of the environment as an integer (`fallback` when unset); the callers that read one once per process keep it in a static
int env_int(const char* name, int fallback) {
  const char* e = getenv(name);
  return e ? atoi(e) : fallback;
}
bool env_flag(const char* name, bool fallback) { return env_int(name, fallback) != 0; }

int check_grid(const RFGrid* g) {
  if (!g || !g->densities_dev) return RF_ERR_NULL_POINTER;
  if (!g->features_dev && !second_tensor_optional(g)) return RF_ERR_NULL_POINTER;
  for (int a = 0; a < 3; ++a)
    if (g->dims[a] < 1 || g->dims[a] > 2046) return RF_ERR_BAD_SHAPE;
  const int F = g->num_features;
  if (!(F == 3 || F == 12 || F == 27 || F == 48)) return RF_ERR_UNSUPPORTED;  // SH degree 0..3
  if (g->density_mode < RF_DENSITY_RELU || g->density_mode > RF_DENSITY_IDENTITY) return RF_ERR_UNSUPPORTED;
  if (g->layout == RF_LAYOUT_REFERENCE) {
    if (g->density_stride < 1 || g->feature_stride < F) return RF_ERR_BAD_SHAPE;
  } else if (g->layout == RF_LAYOUT_SPLIT || g->layout == RF_LAYOUT_BRICKED) {
    if (g->density_stride < 4 || (F > 3 && g->feature_stride < F - 3)) return RF_ERR_BAD_SHAPE;
  } else {
    return RF_ERR_UNSUPPORTED;
  }
  // node indices are 32-bit in the kernels (node_lin: 24-bit multiplies into an unsigned int; element offsets are 64-bit):
  // the node count, padded to whole bricks for the bricked order, must stay below 2^32
  if (node_count(g, g->layout == RF_LAYOUT_BRICKED) >= (1ull << 32)) return RF_ERR_BAD_SHAPE;
  return RF_OK;
}

GridArgs to_args(const RFGrid* g) {
  GridArgs a;
  a.dens = g->densities_dev;
  a.feat = g->features_dev;
  a.occ = g->occupancy_dev;
  a.X = g->dims[0];
  a.Y = g->dims[1];
  a.Z = g->dims[2];
  a.F = g->num_features;
  a.dstride = g->density_stride;
  a.fstride = g->feature_stride;
  for (int i = 0; i < 3; ++i) {
    a.amin[i] = g->aabb_min[i];
    a.amax[i] = g->aabb_max[i];
    a.nscale[i] = g->norm_scale[i];
    a.nbias[i] = g->norm_bias[i];
  }
  a.rho = g->density_scale;
  a.mode = g->density_mode;
  a.layout = g->layout == RF_LAYOUT_REFERENCE ? RF_LAYOUT_REFERENCE : RF_LAYOUT_SPLIT;  // channel arrangement
  a.bricked = g->layout == RF_LAYOUT_BRICKED;
  a.nby = (a.Y + 7) / 8;
  a.nbz = (a.Z + 7) / 8;
  if (a.bricked) {
    a.step[0] = 64u;
    a.step[1] = 8u;
    a.step[2] = 1u;
    a.jump[0] = (unsigned)a.nby * (unsigned)a.nbz * 512u - 7u * 64u;
    a.jump[1] = (unsigned)a.nbz * 512u - 7u * 8u;
    a.jump[2] = 512u - 7u;
  } else {
    a.step[0] = a.jump[0] = (unsigned)a.Y * (unsigned)a.Z;
    a.step[1] = a.jump[1] = (unsigned)a.Z;
    a.step[2] = a.jump[2] = 1u;
  }
  {
    const unsigned long long nodes = node_count(g, a.bricked);
    const unsigned long long db = (unsigned long long)a.dstride * 4ull, fb = (unsigned long long)a.fstride * 4ull;
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(a.dens), f0 = a.feat ? reinterpret_cast<uintptr_t>(a.feat) : d0;
    const uintptr_t lo = d0 < f0 ? d0 : f0;
    const unsigned long long dend = (d0 - lo) + nodes * db, fend = a.feat ? (f0 - lo) + nodes * fb : 0ull;
    const unsigned long long span = (dend > fend ? dend : fend) + 16ull;
    a.base = reinterpret_cast<const char*>(lo);
    a.dens_off = (unsigned int)(d0 - lo);
    a.feat_off = (unsigned int)(f0 - lo);
    a.near32 = nodes <= (1ull << 24) && db < (1ull << 24) && fb < (1ull << 24) && span < (1ull << 32);
    // ($RF_FAR_ADDRESSING=1: the general 64-bit path on grids that would not need it -- tests compare the two)
    a.near32 = a.near32 && env_int("RF_FAR_ADDRESSING", 0) == 0;
  }
  return a;
}

int check_rays(const RFRayBatch* r) {
  if (!r) return RF_ERR_NULL_POINTER;
  if (r->num_rays < 0 || r->num_samples < 1) return RF_ERR_BAD_SHAPE;
  if (r->num_rays > 0 && !r->t_vals_dev) return RF_ERR_NULL_POINTER;
  if (r->num_rays > 0 && !r->camera && (!r->origins_dev || !r->directions_dev)) return RF_ERR_NULL_POINTER;
  if (r->camera) {
    if (r->camera->height < 1 || r->camera->width < 1 || r->first_ray < 0) return RF_ERR_BAD_SHAPE;
    if (r->first_ray + r->num_rays > (int64_t)r->camera->height * r->camera->width) return RF_ERR_BAD_SHAPE;
  }
  return RF_OK;
}

RayArgs to_args(const RFRayBatch* r, uint32_t flags = 0);
RayArgs to_args(const RFRayBatch* r, uint32_t flags) {
  RayArgs a;
  a.origins = r->origins_dev;
  a.directions = r->directions_dev;
  a.n = r->num_rays;
  a.S = r->num_samples;
  a.near = r->near;
  a.far = r->far;
  a.tvals = r->t_vals_dev;
  a.trand = r->t_rand_dev;
  a.jkey = r->jitter_key;
  a.ray0 = r->first_ray;
  a.jitter = (flags & RF_FLAG_JITTER_KEYED) && !r->t_rand_dev;
  a.cam = r->camera != nullptr;
  a.H = a.W = 1;
  a.focal = 1.0f;
  for (int i = 0; i < 12; ++i) a.pose[i] = 0.0f;
  if (r->camera) {
    a.H = r->camera->height;
    a.W = r->camera->width;
    a.focal = r->camera->focal;
    for (int i = 0; i < 12; ++i) a.pose[i] = r->camera->pose[i];
  }
  return a;
}

OutArgs to_args(const RFRenderOut* o) {
  OutArgs a;
  a.colour = o->colour_dev;
  a.depth = o->depth_dev;
  a.acc = o->acc_dev;
  a.disparity = o->disparity_dev;
  a.cache = o->sample_cache_dev;
  a.tcache = o->trans_cache_dev;
  a.cmask = reinterpret_cast<unsigned long long*>(o->chunk_mask_dev);
  a.stop = o->stop_cache_dev;
  a.hist = nullptr;
  a.brick_shift = 0;
  a.nby = a.nbz = 0;
  return a;
}

int launch_status() { return hipGetLastError() == hipSuccess ? RF_OK : RF_ERR_LAUNCH; }

// The one place that turns the SH degree into a kernel instantiation: f(std::integral_constant<int, K>) for the K = (degree + 1)^2
// coefficients per colour of the grid, if K is in the set the caller allows -- the set is what gets instantiated; RF_ERR_UNSUPPORTED
// otherwise.  f returns the call's return code.
template <int... Ks>
struct ShSet {};
using ShAll = ShSet<1, 4, 9, 16>;
using ShEven = ShSet<1, 9>;  // SH degree 0 / 2: 3 K + 1 channels are whole float4s
template <int... Ks, class F>
int dispatch_sh(int K, ShSet<Ks...>, F&& f) {
  int rc = RF_ERR_UNSUPPORTED;
  (void)(... || (K == Ks && ((rc = f(std::integral_constant<int, Ks>{})), true)));
  return rc;
}

// the render kernels <K, DIFFUSE>: a render_diffuse pass reads one coefficient per colour, like SH degree 0
template <class F>
int dispatch_render(int K, bool diffuse, F&& f) {
  if (diffuse || K == 1) return f(std::integral_constant<int, 1>{}, std::true_type{});
  return dispatch_sh(K, ShSet<4, 9, 16>{}, [&](auto k) { return f(k, std::false_type{}); });
}

// workgroups of a kernel that gives every ray one wave
unsigned ray_blocks(int64_t num_rays) { return (unsigned)((num_rays + kWavesPerBlock - 1) / kWavesPerBlock); }

unsigned grid_1d(long long n, int block, long long cap = 256LL * 16) {
  long long b = (n + block - 1) / block;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (unsigned)b;
}

// the sample cache of a saving forward render: all four arrays or none
bool has_caches(const RFRenderOut* o) { return o->sample_cache_dev && o->trans_cache_dev && o->stop_cache_dev && o->chunk_mask_dev; }

void set_grads(const RFRenderGrads* grads, GradArgs* gr) {
  gr->gcolour = grads->grad_colour_dev;
  gr->gdepth = grads->grad_depth_dev;
  gr->gacc = grads->grad_acc_dev;
}

}  // namespace
