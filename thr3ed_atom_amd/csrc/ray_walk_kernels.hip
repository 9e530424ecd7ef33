// ray_walk_kernels.hip -- density-only walks of a ray: rf_node_max_weight, rf_distortion, rf_render_geometry.  One wave per ray,
// lanes = the samples of a 64-sample chunk, the forward render's P0 (rf_device.h: load_ray .. chunk_weights) without anything that
// depends on colour, so that the compositing weights w_i = alpha_i T_i are the forward's floats bit for bit.
#include "rf_device.h"

namespace {

// The activated density of a sample the way render_forward_ray's P0 computes it (corners_of, the separately rounded sum in ATen's
// corner order, density_post), with the cell's corners and their 8 pre-activation values.  A sample that is not live (outside the
// box, or in a cell the occupancy mask calls empty) reads nothing: sigma 0, corners of weight 0 at node 0, values 0.  Only element 0
// of a node's density / base record is read: no feature is touched.
__device__ __forceinline__ float live_density(bool live, const Cell& cell, uint32_t packed, const GridArgs& g, Corners& cn, float v[8]) {
  float sigma = 0.0f;
#pragma unroll
  for (int k = 0; k < 8; ++k) cn.w[k] = 0.0f, cn.lin[k] = 0u, v[k] = 0.0f;
  cn.s[0] = cn.s[1] = cn.s[2] = 0u;
  if (live) {
    const float wts[6] = {cell.w0[0], cell.w1[0], cell.w0[1], cell.w1[1], cell.w0[2], cell.w1[2]};
    cn = corners_of(packed, wts, g);
    float pre;
    sigma = interp_density_values(cn, g, v, pre);
  }
  return sigma;
}

// =============================================================================================
// rf_node_max_weight: per grid node the largest compositing weight any sample ever gave it.  The walk is
// render_forward_ray's P0 without everything that depends on colour: one wave per ray, lanes = the samples of a 64-sample chunk, the
// same helpers in the same order (load_ray, box_span / chunk_outside_box, z_of / sample_at, corners_of, the separately rounded density
// sum in ATen's corner order, density_post, occupancy_alpha, the DPP transmittance scan), so w_i = alpha_i T_i is the forward's float
// bit for bit.  No SH basis, no LDS work list, no cache.  Every corner k of an inside sample's cell offers v = w_i * cn.w[k] to
// M[node]: an atomicMax on the bit pattern (integer order == float order for non-negative floats), behind a plain load that rejects
// what cannot raise the entry -- a stale value read there is only ever too SMALL (entries never fall), which costs a redundant atomic
// and never a wrong result.  A maximum does not depend on the order of arrival: bitwise reproducible.  M is in plain node order
// ((x * Y + y) * Z + z) whatever the grid's storage.
// GUARD / DEDUPE are measurement switches of tools/node_weights_time.py (compile-time: RF_NMW_GUARD, RF_NMW_DEDUPE).  DEDUPE: a
// lane whose predecessor sampled the same cell and offers at least as much to a corner drops that corner's update (the relation is
// transitive along a run of lanes, so the run's first lane still carries the maximum).
// =============================================================================================
#ifndef RF_NMW_GUARD
#define RF_NMW_GUARD 1
#endif
#ifndef RF_NMW_DEDUPE
#define RF_NMW_DEDUPE 0
#endif

template <bool GUARD, bool DEDUPE>
__global__ __launch_bounds__(kBlock) void node_max_weight_kernel(GridArgs g, RayArgs r, uint32_t flags, unsigned int* M) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long ray = (long long)blockIdx.x * kWavesPerBlock + wave;
  if (ray >= r.n) return;  // (wave-uniform)

  const RayState st = load_ray(r, g, ray, flags);
  const bool use_occ = (flags & RF_FLAG_OCCUPANCY_SKIP) && g.occ != nullptr;
  const BoxSpan span = box_span(st, r, g);
  const unsigned int px = (unsigned)g.Y * (unsigned)g.Z, py = (unsigned)g.Z;  // plain node order of M
  float T_carry = 1.0f;
  const int nchunks = (r.S + kWave - 1) / kWave;
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    if (chunk_outside_box(span, st, r, chunk)) continue;  // wave-uniform: sigma = 0 -> w = 0, T unchanged
    const int s = chunk * kWave + lane;
    const Sample sm = make_sample(st, r, g, ray, s);
    bool live = sm.inside;
    if (use_occ && live) live = cell_occupied(sm.cell, g);
    Corners cn;
    float v[8];
    const uint32_t packed = pack_cell(sm.cell);
    const float sigma = live_density(live, sm.cell, packed, g, cn, v);
    const ChunkWeights cw = chunk_weights(sigma, sm.delta, sm.valid, T_carry);
    const float w = live ? cw.alpha * cw.T : 0.0f;
    T_carry = T_carry * read_lane(cw.incl, kWave - 1);

    // the cell's lower node in plain order; the steps collapse where corners_of's do (clamped at the border)
    const int ix0 = (int)(packed & 0x7ffu) - 1, iy0 = (int)((packed >> 11) & 0x7ffu) - 1, iz0 = (int)(packed >> 22) - 1;
    const unsigned int lin0 = ((unsigned)max(ix0, 0) * (unsigned)g.Y + (unsigned)max(iy0, 0)) * (unsigned)g.Z + (unsigned)max(iz0, 0);
    const unsigned int sx = cn.s[0] ? px : 0u, sy = cn.s[1] ? py : 0u, sz = cn.s[2] ? 1u : 0u;
    uint32_t prev_cell = 0u;
    if constexpr (DEDUPE) {
      const uint32_t tag = live ? packed : 0xffffffffu;  // (a live cell never packs to all ones: dims <= 2046)
      prev_cell = (uint32_t)__builtin_amdgcn_update_dpp((int)0xfffffffeu, (int)tag, kDppWaveShr1, 0xf, 0xf, false);
      prev_cell = (prev_cell == tag) ? 1u : 0u;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float v = w * cn.w[k];
      bool offer = v > 0.0f;  // a product equal to 0 (or a NaN) updates nothing
      if constexpr (DEDUPE) {
        const float pv = dpp_move<kDppWaveShr1, 0xf>(0.0f, v);
        offer = offer && !(prev_cell && pv >= v);
      }
      if (offer) {
        unsigned int* p = M + (size_t)(lin0 + ((k & 1) ? sx : 0u) + ((k & 2) ? sy : 0u) + ((k & 4) ? sz : 0u));
        if (!GUARD || v > __uint_as_float(*p)) atomicMax(p, __float_as_uint(v));
      }
    }
    if (T_carry == 0.0f) break;  // every later weight is exactly 0
  }
}

// =============================================================================================
// rf_distortion: the distortion loss of a ray's compositing weights.  With the forward's samples and weights
// w_i = T_i alpha_i (the walk of node_max_weight_kernel: same helpers, same order, no colour), s_i = (z_i - near) / (far - near) of the
// batch's own bounds, and sample i standing for the interval it composites over (d_i = s_{i+1} - s_i, m_i = (s_i + s_{i+1}) / 2; the last
// sample: d = 0, m = s):
//   l = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i
// The m_i are sorted, so with the exclusive prefixes A_i = sum_{j<i} w_j, B_i = sum_{j<i} w_j m_j and the totals W, WM:
//   l = 2 sum_i w_i (m_i A_i - B_i) + (1/3) sum_i w_i^2 d_i                                           (prefixes only: pass 1)
//   e_i = dl/dw_i = 2 [ m_i (A_i - (W - A_i - w_i)) - (B_i - (WM - B_i - w_i m_i)) ] + (2/3) w_i d_i   (needs the totals: pass 2)
//   dl/dsigma_i = delta_i ( T_{i+1} e_i - sum_{j>i} w_j e_j )      -- render_backward_kernel's adjoint with this e_i
// One wave per ray, lanes = the samples of a 64-sample chunk.  Pass 1 walks near to far (stops where the carried T is exactly 0) and
// leaves each chunk's (T, A, B) carry in a per-wave LDS stash; pass 2 (GRAD) walks far to near with a true running suffix sum,
// evaluates each chunk again from its carry and scatters 8 float atomics per sample whose gradient is non-zero onto the density
// element.  Chunks beyond the stash (S > 64 kDistStash) get their carry by walking forward again from the last stashed one: correct
// for every S, quadratic only in the chunks above the capacity.
// =============================================================================================
constexpr int kDistStash = 16;  // chunks whose carry is kept in LDS: 1024 samples per ray

// inclusive PREFIX sum over the wave (DPP: four row_shr steps inside each row of 16 lanes, row_bcast:15 / :31 fold the rows)
__device__ __forceinline__ float wave_incl_scan_add(float x) {
  x += dpp_move<kDppRowShr1, 0xf>(0.0f, x);
  x += dpp_move<kDppRowShr2, 0xf>(0.0f, x);
  x += dpp_move<kDppRowShr4, 0xf>(0.0f, x);
  x += dpp_move<kDppRowShr8, 0xf>(0.0f, x);
  x += dpp_move<kDppRowBcast15, 0xa>(0.0f, x);
  x += dpp_move<kDppRowBcast31, 0xc>(0.0f, x);
  return x;
}

struct DistCarry {
  float T, A, B;  // transmittance in front of the chunk, sum of w and of w m over the samples in front of it
};

// everything one lane knows about its sample of a chunk, given the chunk's carry
struct DistChunk {
  float w, m, d, A, B;   // weight, interval mid-point and width, exclusive prefixes (carry included)
  float delta, sigma, Tn;  // interval length, activated density, T_{i+1} = T_i exp(-sigma_i delta_i)
  bool live;
  Corners cn;
  DistCarry next;  // the carry behind the chunk (wave-uniform)
};

__device__ __forceinline__ DistChunk dist_chunk(const GridArgs& g, const RayArgs& r, const RayState& st, long long ray, int chunk, int lane,
                                                bool use_occ, float inv_span, const DistCarry& in) {
  DistChunk c;
  const int s = chunk * kWave + lane;
  const float z = z_of(st, r, ray, s), zn = z_of(st, r, ray, s + 1);
  const Sample sm = sample_at(st, r, g, s, z, zn);  // == make_sample
  bool live = sm.inside;
  if (use_occ && live) live = cell_occupied(sm.cell, g);
  float v[8];
  const float sigma = live_density(live, sm.cell, pack_cell(sm.cell), g, c.cn, v);
  const ChunkWeights cw = chunk_weights(sigma, sm.delta, sm.valid, in.T);
  c.w = live ? cw.alpha * cw.T : 0.0f;
  c.Tn = cw.T * cw.E;
  c.delta = sm.delta;
  c.sigma = sigma;
  c.live = live;
  // the interval of the sample on the batch's own [near, far] (the camera bounds, also under AABB sampling)
  const float s0 = (z - r.near) * inv_span, s1 = (zn - r.near) * inv_span;
  const bool last = s >= r.S - 1;
  c.d = last ? 0.0f : s1 - s0;
  c.m = last ? s0 : 0.5f * (s0 + s1);
  const float wm = c.w * c.m;
  const float iw = wave_incl_scan_add(c.w), iwm = wave_incl_scan_add(wm);
  c.A = in.A + (iw - c.w);
  c.B = in.B + (iwm - wm);
  c.next.T = in.T * read_lane(cw.incl, kWave - 1);
  c.next.A = in.A + read_lane(iw, kWave - 1);
  c.next.B = in.B + read_lane(iwm, kWave - 1);
  return c;
}

template <bool GRAD>
__global__ __launch_bounds__(kBlock) void distortion_kernel(GridArgs g, RayArgs r, uint32_t flags, float scale, const float* __restrict__ gloss,
                                                            float* __restrict__ loss, float* __restrict__ gdens) {
  __shared__ float s_stash[GRAD ? kWavesPerBlock : 1][kDistStash][3];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long ray = (long long)blockIdx.x * kWavesPerBlock + wave;
  if (ray >= r.n) return;  // (wave-uniform)

  float factor = scale;
  if (GRAD && gloss) factor *= gloss[ray];
  const bool want_grad = GRAD && factor != 0.0f;
  if (!want_grad && !loss) return;

  const RayState st = load_ray(r, g, ray, flags);
  const bool use_occ = (flags & RF_FLAG_OCCUPANCY_SKIP) && g.occ != nullptr;
  const BoxSpan span = box_span(st, r, g);
  const float inv_span = 1.0f / (r.far - r.near);
  const int nchunks = (r.S + kWave - 1) / kWave;

  // pass 1, near to far: the loss from prefixes, the totals, every chunk's carry
  DistCarry carry = {1.0f, 0.0f, 0.0f};
  float part = 0.0f;  // this lane's share of l
  int last_chunk = -1;
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    if (GRAD && chunk < kDistStash && lane == 0) {
      s_stash[wave][chunk][0] = carry.T;
      s_stash[wave][chunk][1] = carry.A;
      s_stash[wave][chunk][2] = carry.B;
    }
    if (chunk_outside_box(span, st, r, chunk)) continue;  // wave-uniform: w = 0 for the whole chunk, the carry unchanged
    const DistChunk c = dist_chunk(g, r, st, ray, chunk, lane, use_occ, inv_span, carry);
    part += 2.0f * c.w * (c.m * c.A - c.B) + (1.0f / 3.0f) * (c.w * c.w) * c.d;
    carry = c.next;
    last_chunk = chunk;
    if (carry.T == 0.0f) break;  // every later weight is exactly 0
  }
  if (loss) {
    const float total = wave_sum(part);
    if (lane == 0) loss[ray] = total;
  }
  if (!want_grad) return;
  if constexpr (GRAD) {
    wave_lds_fence();
    const float W = carry.A, WM = carry.B;
    float suffix = 0.0f;  // sum of w_j e_j over all samples beyond the current chunk
    // pass 2, far to near
    for (int chunk = last_chunk; chunk >= 0; --chunk) {
      if (chunk_outside_box(span, st, r, chunk)) continue;
      const int have = min(chunk, kDistStash - 1);
      DistCarry in = {s_stash[wave][have][0], s_stash[wave][have][1], s_stash[wave][have][2]};
      for (int k = have; k < chunk; ++k) {  // beyond the stash: walk forward again from the last stashed carry
        if (chunk_outside_box(span, st, r, k)) continue;
        in = dist_chunk(g, r, st, ray, k, lane, use_occ, inv_span, in).next;
      }
      const DistChunk c = dist_chunk(g, r, st, ray, chunk, lane, use_occ, inv_span, in);
      const float wm = c.w * c.m;
      const float e = 2.0f * (c.m * (c.A - ((W - c.A) - c.w)) - (c.B - ((WM - c.B) - wm))) + (2.0f / 3.0f) * (c.w * c.d);
      const float we = c.w * e;  // (0 for lanes beyond the ray's last sample and for samples outside the box: w = 0)
      const float incl = wave_incl_rscan_add(we, lane);
      const float after = (incl - we) + suffix;  // sum over samples strictly behind this one
      suffix += __shfl(incl, 0, kWave);
      const float g_sigma = c.delta * (c.Tn * e - after);
      float g_pre;  // (density_pre_grad, written out: through the helper the compiler lays this kernel's branches out differently)
      if (g.mode == RF_DENSITY_RELU)
        g_pre = (c.sigma > 0.0f) ? g_sigma : 0.0f;
      else if (g.mode == RF_DENSITY_SOFTPLUS)
        g_pre = g_sigma * softplus_slope(c.sigma);
      else
        g_pre = g_sigma;
      g_pre *= factor;
      if (c.live && g_pre != 0.0f) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          // (a corner outside the grid has weight 0 and the clamped index of a real node: nothing is added, nothing out of range is read)
          const size_t at = (size_t)c.cn.lin[k] * (size_t)g.dstride;
          float gv = (c.cn.w[k] * g_pre) * g.rho;
          if (g.mode == RF_DENSITY_ABS) {
            const float dv = g.dens[at] * g.rho;
            gv = (dv > 0.f) ? gv : ((dv < 0.f) ? -gv : 0.0f);
          }
          if (gv != 0.0f) unsafeAtomicAdd(gdens + at, gv);
        }
      }
    }
  }
}

// =============================================================================================
// rf_render_geometry: surface normals and quantile depth of the rendered rays.  The walk of
// node_max_weight_kernel once more -- one wave per ray, lanes = the samples of a 64-sample chunk, the same helpers in the same order, so
// w_i = alpha_i T_i is the forward's float bit for bit -- compositing three per-sample quantities:
//   acc = sum_i w_i                    per-lane partial sums over the chunks, one wave sum at the end: render_forward_ray's order and bits
//   N   = sum_i w_i n_i                n_i = -g_i / |g_i| (0 where g_i = 0), g_i the world-space gradient of the interpolated
//                                      pre-activation density at the sample; per-lane products, a wave sum per chunk, a carry: no atomics
//   z_q = z of the first sample with 1 - T_{i+1} >= quantile (0 if none): a ballot over the chunk and its first set lane
// The gradient needs the 8 corner values themselves, not only their weighted sum: live_density hands them back.  No feature is
// read, nothing is written but one result per ray.
// =============================================================================================
__global__ __launch_bounds__(kBlock) void render_geometry_kernel(GridArgs g, RayArgs r, uint32_t flags, float quantile, float* __restrict__ normal,
                                                                 float* __restrict__ qdepth, float* __restrict__ acc_out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long ray = (long long)blockIdx.x * kWavesPerBlock + wave;
  if (ray >= r.n) return;  // (wave-uniform)

  const RayState st = load_ray(r, g, ray, flags);
  const bool use_occ = (flags & RF_FLAG_OCCUPANCY_SKIP) && g.occ != nullptr;
  const BoxSpan span = box_span(st, r, g);
  // d idx_a / d p_a (locate): world gradient = index gradient * dims_a * norm_scale_a / 2
  const float gscale[3] = {((float)g.X * g.nscale[0]) * 0.5f, ((float)g.Y * g.nscale[1]) * 0.5f, ((float)g.Z * g.nscale[2]) * 0.5f};
  float T_carry = 1.0f, part_acc = 0.0f, zq = 0.0f;
  float N[3] = {0.0f, 0.0f, 0.0f};
  bool found = false;  // (wave-uniform)
  const int nchunks = (r.S + kWave - 1) / kWave;
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    if (chunk_outside_box(span, st, r, chunk)) continue;  // wave-uniform: sigma = 0 -> w = 0, T unchanged
    const int s = chunk * kWave + lane;
    const Sample sm = make_sample(st, r, g, ray, s);
    bool live = sm.inside;
    if (use_occ && live) live = cell_occupied(sm.cell, g);
    Corners cn;
    float v[8];
    const uint32_t packed = pack_cell(sm.cell);
    const float sigma = live_density(live, sm.cell, packed, g, cn, v);
    const ChunkWeights cw = chunk_weights(sigma, sm.delta, sm.valid, T_carry);
    const float wf = cw.alpha * cw.T;  // the forward's w (alpha = 0 where the sample is not live)
    if (sm.valid) part_acc += wf;
    const float w = live ? wf : 0.0f;

    // quantile depth: C_i = 1 - T_{i+1}, T_{i+1} the transmittance the next sample is weighted with
    if (!found) {
      const float C = 1.0f - T_carry * cw.incl;
      const unsigned long long hit = __ballot(sm.valid && C >= quantile);
      if (hit) {
        found = true;
        zq = read_lane(sm.z, __builtin_amdgcn_readfirstlane(__ffsll((long long)hit) - 1));
      }
    }
    T_carry = T_carry * read_lane(cw.incl, kWave - 1);

    // index-space gradient of the trilinear interpolant: a corner outside the grid counts as 0 (corners_of masks its weight)
    const int ix0 = (int)(packed & 0x7ffu) - 1, iy0 = (int)((packed >> 11) & 0x7ffu) - 1, iz0 = (int)(packed >> 22) - 1;
    const bool okx[2] = {ix0 >= 0, ix0 + 1 < g.X}, oky[2] = {iy0 >= 0, iy0 + 1 < g.Y}, okz[2] = {iz0 >= 0, iz0 + 1 < g.Z};
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (okx[k & 1] && oky[(k >> 1) & 1] && okz[k >> 2]) ? v[k] : 0.0f;
    const float* w0 = sm.cell.w0;
    const float* w1 = sm.cell.w1;
    const float wyz[4] = {w0[1] * w0[2], w1[1] * w0[2], w0[1] * w1[2], w1[1] * w1[2]};  // [dy + 2 dz]
    const float wxz[4] = {w0[0] * w0[2], w1[0] * w0[2], w0[0] * w1[2], w1[0] * w1[2]};  // [dx + 2 dz]
    const float wxy[4] = {w0[0] * w0[1], w1[0] * w0[1], w0[0] * w1[1], w1[0] * w1[1]};  // [dx + 2 dy]
    float gw[3];
    gw[0] = (((v[1] - v[0]) * wyz[0] + (v[3] - v[2]) * wyz[1]) + ((v[5] - v[4]) * wyz[2] + (v[7] - v[6]) * wyz[3])) * gscale[0];
    gw[1] = (((v[2] - v[0]) * wxz[0] + (v[3] - v[1]) * wxz[1]) + ((v[6] - v[4]) * wxz[2] + (v[7] - v[5]) * wxz[3])) * gscale[1];
    gw[2] = (((v[4] - v[0]) * wxy[0] + (v[5] - v[1]) * wxy[1]) + ((v[6] - v[2]) * wxy[2] + (v[7] - v[3]) * wxy[3])) * gscale[2];
    // n = -g / |g|, scaled by the largest component first (neither the squares of a huge gradient nor those of a tiny one leave float32)
    const float big = fmaxf(fmaxf(fabsf(gw[0]), fabsf(gw[1])), fabsf(gw[2]));
    float part[3] = {0.0f, 0.0f, 0.0f};
    if (w != 0.0f && big > 0.0f) {  // a sample without weight contributes nothing, whatever its gradient
      const float u[3] = {gw[0] / big, gw[1] / big, gw[2] / big};
      const float len = sqrtf((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
#pragma unroll
      for (int a = 0; a < 3; ++a) part[a] = w * -(u[a] / len);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) N[a] += wave_sum(part[a]);
    if (T_carry == 0.0f) break;  // every later weight is exactly 0 (and 1 - T reached 1: the quantile is found)
  }
  const float acc = wave_sum(part_acc);
  if (lane == 0) {
    if (normal) normal[ray * 3 + 0] = N[0], normal[ray * 3 + 1] = N[1], normal[ray * 3 + 2] = N[2];
    if (qdepth) qdepth[ray] = zq;
    if (acc_out) acc_out[ray] = acc;
  }
}

}  // namespace

extern "C" {

int rf_node_max_weight(const RFGrid* grid, const RFRayBatch* rays, uint32_t flags, float* max_weight_dev, void* stream) {
  int rc = check_grid(grid);
  if (rc != RF_OK) return rc;
  rc = check_rays(rays);
  if (rc != RF_OK) return rc;
  if (!max_weight_dev) return RF_ERR_NULL_POINTER;
  if ((flags & RF_FLAG_OCCUPANCY_SKIP) && !grid->occupancy_dev) return RF_ERR_NULL_POINTER;
  if (rays->num_rays == 0) return RF_OK;
  const GridArgs g = to_args(grid);
  const RayArgs r = to_args(rays, flags);
  const unsigned blocks = ray_blocks(rays->num_rays);
  hipLaunchKernelGGL((node_max_weight_kernel<RF_NMW_GUARD != 0, RF_NMW_DEDUPE != 0>), dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, g, r, flags,
                     reinterpret_cast<unsigned int*>(max_weight_dev));
  return launch_status();
}

int rf_distortion(const RFGrid* grid, const RFRayBatch* rays, uint32_t flags, float scale, const float* grad_loss_dev, float* loss_dev,
                  float* grad_first_dev, void* stream) {
  int rc = check_grid(grid);
  if (rc != RF_OK) return rc;
  rc = check_rays(rays);
  if (rc != RF_OK) return rc;
  if (!std::isfinite(rays->near) || !std::isfinite(rays->far) || rays->far == rays->near || !std::isfinite(scale)) return RF_ERR_BAD_SHAPE;
  if ((flags & RF_FLAG_OCCUPANCY_SKIP) && !grid->occupancy_dev) return RF_ERR_NULL_POINTER;
  // the gradient is added to a tensor of its own, never to the parameters
  if (grad_first_dev && grad_first_dev == grid->densities_dev) return RF_ERR_BAD_SHAPE;
  const bool want_grad = grad_first_dev != nullptr && scale != 0.0f;
  if ((!want_grad && !loss_dev) || rays->num_rays == 0) return RF_OK;
  const GridArgs g = to_args(grid);
  const RayArgs r = to_args(rays, flags);
  const unsigned blocks = ray_blocks(rays->num_rays);
  if (want_grad)
    hipLaunchKernelGGL(distortion_kernel<true>, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, g, r, flags, scale, grad_loss_dev, loss_dev,
                       grad_first_dev);
  else
    hipLaunchKernelGGL(distortion_kernel<false>, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, g, r, flags, 0.0f, (const float*)nullptr, loss_dev,
                       (float*)nullptr);
  return launch_status();
}

int rf_render_geometry(const RFGrid* grid, const RFRayBatch* rays, uint32_t flags, float quantile, const RFGeometryOut* out, void* stream) {
  int rc = check_grid(grid);
  if (rc != RF_OK) return rc;
  rc = check_rays(rays);
  if (rc != RF_OK) return rc;
  if (!out || (!out->normal_dev && !out->quantile_depth_dev && !out->acc_dev)) return RF_ERR_NULL_POINTER;
  if (!(quantile > 0.0f && quantile < 1.0f)) return RF_ERR_BAD_SHAPE;  // (NaN fails the comparison too)
  if ((flags & RF_FLAG_OCCUPANCY_SKIP) && !grid->occupancy_dev) return RF_ERR_NULL_POINTER;
  if (rays->num_rays == 0) return RF_OK;
  const GridArgs g = to_args(grid);
  const RayArgs r = to_args(rays, flags);
  const unsigned blocks = ray_blocks(rays->num_rays);
  hipLaunchKernelGGL(render_geometry_kernel, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, g, r, flags, quantile, out->normal_dev,
                     out->quantile_depth_dev, out->acc_dev);
  return launch_status();
}

}  // extern "C"
