// ray_grad_kernels.hip -- gradients with respect to rays and points: dL/d(origins, directions) of a render from its sample cache
// (rf_render_backward_rays) and dL/d(points) of a grid query (rf_grid_query_backward_points).
#include "rf_device.h"

namespace {

// =============================================================================================
// ray and point adjoints: dL/d(origins, directions) of a render, dL/d(points) of a grid query
//
// Shared piece: the gradient of a trilinear interpolation with respect to the CONTINUOUS index.  With the corner weights
// w_k = wx_dx wy_dy wz_dz (w1_a = idx_a - floor, w0_a = floor + 1 - idx_a, so w1_a' = +1, w0_a' = -1) and q_k the per-corner value
// the upstream gradient sees, d/d idx_a sum_k w_k q_k = sum_k (d w_k / d idx_a) q_k.  The same floor cell, zero padding and corner
// skipping as the forward (corners outside the grid contribute nothing).  J = diag(nscale_a size_a / 2) maps index to world.
// =============================================================================================
// d w_k / d idx of corner k = dx + 2 dy + 4 dz (a corner inside the grid; the caller skips the others)
__device__ __forceinline__ void corner_index_grad(int k, const float w0[3], const float w1[3], float dw[3]) {
  const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
  const float wx = dx ? w1[0] : w0[0], wy = dy ? w1[1] : w0[1], wz = dz ? w1[2] : w0[2];
  const float sx = dx ? 1.0f : -1.0f, sy = dy ? 1.0f : -1.0f, sz = dz ? 1.0f : -1.0f;
  dw[0] = (sx * wy) * wz;
  dw[1] = (wx * sy) * wz;
  dw[2] = (wx * wy) * sz;
}

__device__ __forceinline__ void index_to_world(const GridArgs& g, float gi[3]) {
  const int dims[3] = {g.X, g.Y, g.Z};
#pragma unroll
  for (int a = 0; a < 3; ++a) gi[a] = gi[a] * (g.nscale[a] * (float)dims[a] * 0.5f);
}

// sum_k G_k dY_k/dv of the signed basis of sh_basis<K> (v = (x, y, z) unit)
template <int K>
__device__ __forceinline__ void sh_basis_vjp(float x, float y, float z, const float G[16], float gv[3]) {
  gv[0] = gv[1] = gv[2] = 0.0f;
  if (K > 1) {
    gv[1] += -kC1 * G[1];
    gv[2] += kC1 * G[2];
    gv[0] += -kC1 * G[3];
  }
  if (K > 4) {
    gv[0] += kC2_0 * y * G[4];
    gv[1] += kC2_0 * x * G[4];
    gv[1] += kC2_1 * z * G[5];
    gv[2] += kC2_1 * y * G[5];
    gv[0] += -2.0f * kC2_2 * x * G[6];
    gv[1] += -2.0f * kC2_2 * y * G[6];
    gv[2] += 4.0f * kC2_2 * z * G[6];
    gv[0] += kC2_3 * z * G[7];
    gv[2] += kC2_3 * x * G[7];
    gv[0] += 2.0f * kC2_4 * x * G[8];
    gv[1] += -2.0f * kC2_4 * y * G[8];
  }
  if (K > 9) {
    const float xx = x * x, yy = y * y, zz = z * z;
    gv[0] += 6.0f * kC3_0 * x * y * G[9];
    gv[1] += kC3_0 * (3.0f * xx - 3.0f * yy) * G[9];
    gv[0] += kC3_1 * y * z * G[10];
    gv[1] += kC3_1 * x * z * G[10];
    gv[2] += kC3_1 * x * y * G[10];
    gv[0] += -2.0f * kC3_2 * x * y * G[11];
    gv[1] += kC3_2 * (4.0f * zz - xx - 3.0f * yy) * G[11];
    gv[2] += 8.0f * kC3_2 * y * z * G[11];
    gv[0] += -6.0f * kC3_3 * x * z * G[12];
    gv[1] += -6.0f * kC3_3 * y * z * G[12];
    gv[2] += kC3_3 * (6.0f * zz - 3.0f * xx - 3.0f * yy) * G[12];
    gv[0] += kC3_4 * (4.0f * zz - 3.0f * xx - yy) * G[13];
    gv[1] += -2.0f * kC3_4 * x * y * G[13];
    gv[2] += 8.0f * kC3_4 * x * z * G[13];
    gv[0] += 2.0f * kC3_5 * x * z * G[14];
    gv[1] += -2.0f * kC3_5 * y * z * G[14];
    gv[2] += kC3_5 * (xx - yy) * G[14];
    gv[0] += kC3_6 * (3.0f * xx - 3.0f * yy) * G[15];
    gv[1] += -6.0f * kC3_6 * x * y * G[15];
  }
}

// feature k of colour ch at node `lin` (KG = coefficients per colour stored in the grid): reference [F] = colour * KG + k;
// split / bricked: k == 0 in the base record (sigma, r, g, b), k > 0 in the rest record at colour * (KG - 1) + k - 1
__device__ __forceinline__ float node_feature(const GridArgs& g, long long lin, int ch, int k, int KG) {
  if (g.layout == RF_LAYOUT_SPLIT) {
    if (k == 0) return g.dens[lin * g.dstride + 1 + ch];
    return g.feat[lin * g.fstride + ch * (KG - 1) + (k - 1)];
  }
  return g.feat[lin * g.fstride + ch * KG + k];
}

// The slab test of ray_box with the derivative of the bound each running max / min kept: bound = (plane - o_a) / (d_a + 1e-10) of
// axis `axis`, so d bound / d o_a = -1 / den, d bound / d d_a = -bound / den.  `ok` = the bound reaches the sampler (a hit, and not
// clipped to 0 -- torch.clamp passes the gradient at >= 0).  Selections follow ray_box (and the reference's torch.where order).
struct BoundGrad {
  int axis;
  float dd_o, dd_d;  // d bound / d o_axis, d bound / d d_axis
  bool ok;
};
__device__ __forceinline__ void ray_box_grad(const float o[3], const float d[3], const float bmin[3], const float bmax[3], BoundGrad& glo,
                                             BoundGrad& ghi) {
  float lo_run = 0.f, hi_run = 0.f, lo_den = 1.f, hi_den = 1.f;
  int lo_ax = 0, hi_ax = 0;
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
      lo_den = hi_den = den;
    } else {
      hit = hit && !((lo_run > hi) || (lo > hi_run));
      if (lo > lo_run) {
        lo_run = lo;
        lo_ax = a;
        lo_den = den;
      }
      if (hi < hi_run) {
        hi_run = hi;
        hi_ax = a;
        hi_den = den;
      }
    }
  }
  glo.axis = lo_ax;
  glo.dd_o = -1.0f / lo_den;
  glo.dd_d = -lo_run / lo_den;
  glo.ok = hit && lo_run >= 0.0f;
  ghi.axis = hi_ax;
  ghi.dd_o = -1.0f / hi_den;
  ghi.dd_d = -hi_run / hi_den;
  ghi.ok = hit && hi_run >= 0.0f;
}

// =============================================================================================
// dL/d(origins), dL/d(directions) of rf_render_forward (the reference gets them from autograd through _ray_aabb_intersection,
// grid_sample's grid gradient, the SH basis and the interval lengths).  Notation of render_backward_kernel: e_i, w_i, T_i,
// E_i = exp(-sigma_i delta_i); x_i = o + z_i d, delta_i = (z_{i+1} - z_i) |d| (1e10 |d| for the last sample), v = d / |d|.
//   g_delta_i = sigma_i (T_i E_i e_i - sum_{j>i} w_j e_j)            (the bracket of g_sigma_i, times sigma instead of delta)
//   g_x_i     = J^T [ g_pre_i grad interp(pre(rho D)) + sum_ch g_raw_i[ch] grad interp(sum_k Y_k(v) f_{ch,k}) ]
//   g_v       = sum_i sum_ch g_raw_i[ch] sum_k interp(f_{ch,k})(x_i) dY_k/dv
//   g_|d|     = sum_{i<S-1} g_delta_i (z_{i+1} - z_i) + 1e10 g_delta_{S-1}
//   g_o = sum_i g_x_i;   g_d = sum_i z_i g_x_i + g_|d| v + (I - v v^T) g_v / |d|
// and, under RF_FLAG_AABB_SAMPLING only, the z_i = lo (1 - tau_i) + hi tau_i chain through the per-ray bounds of the slab test:
//   g_z_i = g_x_i . d + gD w_i - |d| g_delta_i + |d| g_delta_{i-1};  g_lo = sum g_z_i (1 - tau_i), g_hi = sum g_z_i tau_i.
// One wavefront per ray, lanes = samples, the chunks walked far to near with the running suffix sum of render_backward_kernel and
// make_sample's arithmetic (bit-identical cells and weights); each cached sample's lane gathers its 8 corners itself.  Every
// per-ray sum is a wave reduction: no atomics, bitwise deterministic.
// Uncached samples (outside the box, behind T = 0, sigma = 0 under ReLU) contribute nothing to g_x, g_v or g_delta -- but a
// cached sample i still couples to z_{i+1} through delta_i: that +|d| g_delta_i term is attributed HERE, at sample i, with the
// recomputed tau_{i+1}, since sample i+1 (empty space behind a surface, say) may have no cache entry and no lane work at all.
// =============================================================================================
template <int K, bool DIFFUSE>
__global__ __launch_bounds__(kBlock) void render_backward_rays_kernel(GridArgs g, RayArgs r, OutArgs fwd, GradArgs gr, uint32_t flags,
                                                                      float* __restrict__ g_orig, float* __restrict__ g_dir) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long ray = (long long)blockIdx.x * kWavesPerBlock + wave;
  if (ray >= r.n) return;

  const RayState st = load_ray(r, g, ray, flags);
  const bool aabb = flags & RF_FLAG_AABB_SAMPLING;
  const float white = (flags & RF_FLAG_WHITE_BKGD) ? 1.0f : 0.0f;
  float gC[3] = {0.f, 0.f, 0.f};
  if (gr.gcolour) {
    gC[0] = gr.gcolour[ray * 3 + 0];
    gC[1] = gr.gcolour[ray * 3 + 1];
    gC[2] = gr.gcolour[ray * 3 + 2];
  }
  const float gD = gr.gdepth ? gr.gdepth[ray] : 0.0f;
  const float gA = gr.gacc ? gr.gacc[ray] : 0.0f;
  const float v[3] = {st.d[0] / st.dnorm, st.d[1] / st.dnorm, st.d[2] / st.dnorm};
  float Y[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) Y[k] = 0.0f;
  if (DIFFUSE || K == 1)
    Y[0] = kC0;
  else
    sh_basis<K>(v[0], v[1], v[2], Y);
  const int KG = g.F / 3;
  RayState st01 = st;  // the same sampler on [0, 1]: tau_i (z_uniform(0, 1, t) == t exactly)
  st01.near = 0.0f;
  st01.far = 1.0f;

  // per-lane partial sums
  float go[3] = {0.f, 0.f, 0.f}, gdz[3] = {0.f, 0.f, 0.f}, gdn = 0.0f, glo = 0.0f, ghi = 0.0f;
  float Gk[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) Gk[k] = 0.0f;

  const int processed = fwd.stop[ray];
  const int nchunks = (processed + kWave - 1) / kWave;
  const int mask_words = (r.S + kWave - 1) / kWave;
  float suffix = 0.0f;
  unsigned long long lane_masks = 0ull;
  int masks_group = -1;
  for (int chunk = nchunks - 1; chunk >= 0; --chunk) {
    const int s = chunk * kWave + lane;
    if ((chunk >> 6) != masks_group) {
      masks_group = chunk >> 6;
      const int c = masks_group * kWave + lane;
      lane_masks = fwd.cmask[ray * (long long)mask_words + min(c, mask_words - 1)];
    }
    const unsigned long long cm = chunk_mask_of(lane_masks, chunk);
    if (cm == 0ull) continue;
    const float z = z_of(st, r, ray, s), zn = z_of(st, r, ray, s + 1);
    const Sample sm = sample_at(st, r, g, s, z, zn);  // == make_sample
    const bool have = (cm >> lane) & 1ull;
    float raw[3] = {0.f, 0.f, 0.f};
    float sigma = 0.f, T = 0.f;
    {
      const long long idx = cached_slot(ray, r.S, chunk, cm, lane);
      const float4 cv = reinterpret_cast<const float4*>(fwd.cache)[idx];
      const float Tl = fwd.tcache[idx];
      if (have) {
        raw[0] = cv.x;
        raw[1] = cv.y;
        raw[2] = cv.z;
        sigma = cv.w;
        T = Tl;
      }
    }
    float E;
    const float alpha = occupancy_alpha(sigma * sm.delta, E);
    const float w = alpha * T;
    const float Tn = T * E;
    float c[3], e = gD * sm.z + gA;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      c[ch] = sigmoidf_(raw[ch]);
      e += gC[ch] * (c[ch] - white);
    }
    const float we = have ? w * e : 0.0f;
    const float incl = wave_incl_rscan_add(we, lane);
    const float after = (incl - we) + suffix;
    suffix += __shfl(incl, 0, kWave);
    if (!(have && sm.inside)) continue;

    const float bracket = Tn * e - after;
    const float g_sigma = sm.delta * bracket;
    const float g_delta = sigma * bracket;
    float g_pre = density_pre_grad(g_sigma, sigma, g.mode);
    float g_raw[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) g_raw[ch] = (w * gC[ch]) * (c[ch] * (1.0f - c[ch]));

    // the 8 corners: q_k = g_pre pre(rho D_k) + sum_ch g_raw[ch] sum_k' Y_k' f_{ch,k'}
    const Cell& cl = sm.cell;
    const bool okx[2] = {cl.i0[0] >= 0, cl.i0[0] + 1 < g.X};
    const bool oky[2] = {cl.i0[1] >= 0, cl.i0[1] + 1 < g.Y};
    const bool okz[2] = {cl.i0[2] >= 0, cl.i0[2] + 1 < g.Z};
    float gx[3] = {0.f, 0.f, 0.f};
#pragma unroll 1
    for (int k = 0; k < 8; ++k) {
      const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
      if (!(okx[dx] && oky[dy] && okz[dz])) continue;
      const long long lin = node_lin(g, cl.i0[0] + dx, cl.i0[1] + dy, cl.i0[2] + dz);
      float dv = g.dens[lin * g.dstride] * g.rho;
      if (g.mode == RF_DENSITY_ABS) dv = fabsf(dv);
      const float wk = ((dx ? cl.w1[0] : cl.w0[0]) * (dy ? cl.w1[1] : cl.w0[1])) * (dz ? cl.w1[2] : cl.w0[2]);
      float qk = g_pre * dv;
#pragma unroll
      for (int kk = 0; kk < (DIFFUSE ? 1 : K); ++kk) {
        const float f0 = node_feature(g, lin, 0, kk, KG), f1 = node_feature(g, lin, 1, kk, KG), f2 = node_feature(g, lin, 2, kk, KG);
        const float mix = (g_raw[0] * f0 + g_raw[1] * f1) + g_raw[2] * f2;
        qk += Y[kk] * mix;
        if (!DIFFUSE && K > 1) Gk[kk] += wk * mix;
      }
      float dw[3];
      corner_index_grad(k, cl.w0, cl.w1, dw);
#pragma unroll
      for (int a = 0; a < 3; ++a) gx[a] += dw[a] * qk;
    }
    index_to_world(g, gx);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      go[a] += gx[a];
      gdz[a] += sm.z * gx[a];
    }
    const bool last = s == r.S - 1;
    gdn += last ? kInfinity * g_delta : g_delta * (zn - sm.z);
    if (aabb) {
      const float own = ((gx[0] * st.d[0] + gx[1] * st.d[1]) + gx[2] * st.d[2]) + gD * w - (last ? 0.0f : st.dnorm * g_delta);
      const float tau = z_of(st01, r, ray, s);
      glo += own * (1.0f - tau);
      ghi += own * tau;
      if (!last) {  // +|d| g_delta_i on z_{i+1}, whether or not sample i+1 is cached
        const float nxt = st.dnorm * g_delta, tau1 = z_of(st01, r, ray, s + 1);
        glo += nxt * (1.0f - tau1);
        ghi += nxt * tau1;
      }
    }
  }

  // per-ray sums (every lane ends with the totals)
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    go[a] = wave_sum(go[a]);
    gdz[a] = wave_sum(gdz[a]);
  }
  gdn = wave_sum(gdn);
  glo = wave_sum(glo);
  ghi = wave_sum(ghi);
  float gv[3] = {0.f, 0.f, 0.f};
  if (!DIFFUSE && K > 1) {
#pragma unroll
    for (int k = 1; k < K; ++k) Gk[k] = wave_sum(Gk[k]);
    sh_basis_vjp<K>(v[0], v[1], v[2], Gk, gv);
  }
  if (lane != 0) return;
  const float vg = (v[0] * gv[0] + v[1] * gv[1]) + v[2] * gv[2];
  float gd[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) gd[a] = gdz[a] + gdn * v[a] + (gv[a] - vg * v[a]) / st.dnorm;
  if (aabb) {
    BoundGrad blo, bhi;
    ray_box_grad(st.o, st.d, g.amin, g.amax, blo, bhi);
    if (blo.ok) {
      go[blo.axis] += glo * blo.dd_o;
      gd[blo.axis] += glo * blo.dd_d;
    }
    if (bhi.ok) {
      go[bhi.axis] += ghi * bhi.dd_o;
      gd[bhi.axis] += ghi * bhi.dd_d;
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (g_orig) g_orig[ray * 3 + a] = go[a];
    if (g_dir) g_dir[ray * 3 + a] = gd[a];
  }
}

// dL/d(points) of grid_query_kernel: one thread per point, the corner values of every output channel folded with its upstream
// gradient (the density channel's after the activation slope: ReLU [interp > 0], softplus sigmoid below the threshold 20)
__global__ void grid_query_backward_points_kernel(GridArgs g, const float* __restrict__ points, long long n, const float* __restrict__ gout,
                                                  float* __restrict__ gpoints) {
  const int C = g.F + 1;
  for (long long pt = (long long)blockIdx.x * blockDim.x + threadIdx.x; pt < n; pt += (long long)gridDim.x * blockDim.x) {
    const float p[3] = {points[pt * 3], points[pt * 3 + 1], points[pt * 3 + 2]};
    int i0[3];
    float w0[3], w1[3];
    query_cell(p, g, i0, w0, w1);
    float gden = gout[pt * C + g.F];
    if (g.mode == RF_DENSITY_RELU || g.mode == RF_DENSITY_SOFTPLUS) {
      float pre = 0.0f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const QueryCorner qc = query_corner(k, i0, w0, w1, g);
        if (qc.ok) pre = pre + (g.dens[qc.lin * g.dstride] * g.rho) * qc.w;
      }
      if (g.mode == RF_DENSITY_RELU)
        gden = (pre > 0.0f) ? gden : 0.0f;
      else
        gden = gden * ((pre > 20.0f) ? 1.0f : 1.0f / (1.0f + expf(-pre)));
    }
    float gi[3] = {0.f, 0.f, 0.f};
#pragma unroll 1
    for (int k = 0; k < 8; ++k) {
      const QueryCorner qc = query_corner(k, i0, w0, w1, g);
      if (!qc.ok) continue;
      float dv = g.dens[qc.lin * g.dstride] * g.rho;
      if (g.mode == RF_DENSITY_ABS) dv = fabsf(dv);
      float acc = gden * dv;
      for (int c = 0; c < g.F; ++c) {
        bool first;
        const long long off = query_offset(c, qc.lin, g, &first);
        acc += gout[pt * C + c] * (first ? g.dens[off] : g.feat[off]);
      }
      float dw[3];
      corner_index_grad(k, w0, w1, dw);
#pragma unroll
      for (int a = 0; a < 3; ++a) gi[a] += dw[a] * acc;
    }
    index_to_world(g, gi);
#pragma unroll
    for (int a = 0; a < 3; ++a) gpoints[pt * 3 + a] = gi[a];
  }
}

}  // namespace

extern "C" {

int rf_grid_query_backward_points(const RFGrid* grid, const float* points_dev, int64_t num_points, const float* grad_out_dev,
                                  float* grad_points_dev, void* stream) {
  const int rc = check_grid(grid);
  if (rc != RF_OK) return rc;
  if (num_points < 0) return RF_ERR_BAD_SHAPE;
  if (num_points == 0) return RF_OK;
  if (!points_dev || !grad_out_dev || !grad_points_dev) return RF_ERR_NULL_POINTER;
  if (!grid->features_dev && grid->num_features > 3) return RF_ERR_NULL_POINTER;
  const GridArgs g = to_args(grid);
  hipLaunchKernelGGL(grid_query_backward_points_kernel, dim3(grid_1d(num_points, 256)), dim3(256), 0, (hipStream_t)stream, g, points_dev,
                     (long long)num_points, grad_out_dev, grad_points_dev);
  return launch_status();
}

int rf_render_backward_rays(const RFGrid* grid, const RFRayBatch* rays, uint32_t flags, const RFRenderOut* fwd, const RFRenderGrads* grads,
                            float* grad_origins_dev, float* grad_directions_dev, void* stream) {
  int rc = check_grid(grid);
  if (rc != RF_OK) return rc;
  rc = check_rays(rays);
  if (rc != RF_OK) return rc;
  if (!fwd || !grads) return RF_ERR_NULL_POINTER;
  if (rays->camera) return RF_ERR_UNSUPPORTED;
  if (rays->num_rays == 0 || (!grad_origins_dev && !grad_directions_dev)) return RF_OK;
  if (!has_caches(fwd)) return RF_ERR_NULL_POINTER;
  if (!grid->features_dev && grid->num_features > 3) return RF_ERR_NULL_POINTER;
  const GridArgs g = to_args(grid);
  const RayArgs r = to_args(rays, flags);
  const OutArgs o = to_args(fwd);
  GradArgs gr = {};
  set_grads(grads, &gr);
  const unsigned blocks = ray_blocks(rays->num_rays);
  return dispatch_render(grid->num_features / 3, flags & RF_FLAG_RENDER_DIFFUSE, [&](auto k, auto d) {
    hipLaunchKernelGGL((render_backward_rays_kernel<decltype(k)::value, decltype(d)::value>), dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, g, r, o, gr, flags,
                       grad_origins_dev, grad_directions_dev);
    return launch_status();
  });
}

}  // extern "C"
