// grid_kernels.hip -- node- and point-parallel utilities of a grid: stage-transition upsampling, storage re-layout, the stand-alone
// point query and its parameter adjoint, the occupancy mask, total variation, pruning, content bounds and resampling.  None of
// them walks a ray and none is on the training step's path (rf_train_step calls nothing defined here).
#include "rf_device.h"

#include <climits>

namespace {

// =============================================================================================
// stage transition: scale_voxel_grid_with_required_output_size (thre3d_reprs/voxels.py:334-373) = F.interpolate(mode="trilinear",
// align_corners=False) of the [F+1]-channel volume.  One thread per (destination node, channel), channel fastest; source and
// destination in any storage (the value lands in the destination's layout directly: no unified tensor, no permutes).  ATen's
// arithmetic (UpSampleKernel.cpp / UpSample.h): scale = in / out in float, src = fma(scale, dst + 0.5, -0.5) clamped at 0,
// i0 = min(floor(src), in - 1), i1 = i0 + (i0 < in - 1), lambda = clamp(src - i0, 0, 1); the 8 corners weighted by the products of
// the per-axis weights and summed in the order of ATen's channels-last CPU kernel (see below).
// =============================================================================================
__device__ __forceinline__ long long channel_offset(const GridArgs& g, unsigned int lin, int ch, int K, bool& in_first) {
  // ch: 0 = density, 1..3 = degree-0 coefficient of r, g, b, then colour-major higher degrees (the order of a node's accumulators)
  if (g.layout == RF_LAYOUT_REFERENCE) {
    in_first = ch == 0;
    if (ch == 0) return (long long)lin * g.dstride;
    if (ch < 4) return (long long)lin * g.fstride + (long long)(ch - 1) * K;
    const int j = ch - 4, colour = j / (K - 1), kk = 1 + j - colour * (K - 1);
    return (long long)lin * g.fstride + (long long)colour * K + kk;
  }
  in_first = ch < 4;
  return ch < 4 ? (long long)lin * g.dstride + ch : (long long)lin * g.fstride + (ch - 4);
}

// One axis of a destination node's place in the source lattice: the two source indices it lies between and their weights
// (upsample_axis / resample_axis: the two kernels' own rules), `outside` = beyond the source box (resampling only)
struct AxisLerp {
  int i0, i1;
  float w0, w1;
  bool outside;
};

// work item `it` of upsample_grid_kernel / resample_grid_kernel = (destination node, channel), channel fastest, nodes z fastest
struct NodeChannel {
  int x, y, z, ch;
};
__device__ __forceinline__ NodeChannel node_channel(long long it, const GridArgs& dst) {
  const int C = dst.F + 1;
  NodeChannel n;
  n.ch = (int)(it % C);
  long long node = it / C;
  n.z = (int)(node % dst.Z);
  node /= dst.Z;
  n.y = (int)(node % dst.Y), n.x = (int)(node / dst.Y);
  return n;
}

__device__ __forceinline__ AxisLerp upsample_axis(int dst, int in_size, float scale) {
  float src = fmaf(scale, (float)dst + 0.5f, -0.5f);  // (contracted in ATen's build)
  src = src < 0.0f ? 0.0f : src;
  AxisLerp a;
  a.outside = false;
  a.i0 = min((int)floorf(src), in_size - 1);
  a.i1 = a.i0 + (a.i0 < in_size - 1 ? 1 : 0);
  const float lambda = fminf(fmaxf(src - (float)a.i0, 0.0f), 1.0f);
  a.w0 = 1.0f - lambda;
  a.w1 = lambda;
  return a;
}

__global__ void upsample_grid_kernel(GridArgs src, GridArgs dst, float* dst_first, float* dst_second, long long total) {
  const int C = dst.F + 1, K = dst.F / 3;
  const float sx = (float)src.X / (float)dst.X, sy = (float)src.Y / (float)dst.Y, sz = (float)src.Z / (float)dst.Z;
  for (long long it = (long long)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (long long)gridDim.x * blockDim.x) {
    const NodeChannel n = node_channel(it, dst);
    const int ch = n.ch, x = n.x, y = n.y, z = n.z;
    const AxisLerp ax = upsample_axis(x, src.X, sx), ay = upsample_axis(y, src.Y, sy), az = upsample_axis(z, src.Z, sz);
    auto at = [&](int xi, int yi, int zi) -> float {
      bool first;
      const long long off = channel_offset(src, node_lin(src, xi, yi, zi), ch, K, first);
      return (first ? src.dens : src.feat)[off];
    };
    // corner k = (dx, dy, dz) with z fastest, weight = (wx * wy) * wz
    float val[8], wgt[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int dx = k >> 2, dy = (k >> 1) & 1, dz = k & 1;
      val[k] = at(dx ? ax.i1 : ax.i0, dy ? ay.i1 : ay.i0, dz ? az.i1 : az.i0);
      wgt[k] = ((dx ? ax.w1 : ax.w0) * (dy ? ay.w1 : ay.w0)) * (dz ? az.w1 : az.w0);
    }
    // The reference hands F.interpolate a channels-last volume (features in the reference order, density last), and ATen's
    // channels-last CPU kernel sums the 8 weighted corners right to left in its 8-wide vector body and left to right in the
    // scalar tail of the last C mod 8 channels, every step contracted to a fused multiply-add.  Both orders are reproduced per
    // channel, so that the result equals the reference's own output bit for bit (golden G3).
    int uc;  // index of this channel in the reference's unified [features, density] order
    if (ch == 0) {
      uc = dst.F;
    } else if (ch < 4) {
      uc = (ch - 1) * K;
    } else {
      const int j = ch - 4, colour = j / (K - 1);
      uc = colour * K + 1 + (j - colour * (K - 1));
    }
    float v;
    if (uc < (C & ~7)) {
      v = fmaf(val[7], wgt[7], val[6] * wgt[6]);
#pragma unroll
      for (int k = 5; k >= 0; --k) v = fmaf(val[k], wgt[k], v);
    } else {
      v = fmaf(val[0], wgt[0], val[1] * wgt[1]);
#pragma unroll
      for (int k = 2; k < 8; ++k) v = fmaf(val[k], wgt[k], v);
    }
    bool first;
    const long long off = channel_offset(dst, node_lin(dst, x, y, z), ch, K, first);
    (first ? dst_first : dst_second)[off] = v;
  }
}

// Re-layout of a whole grid: every (node, channel) of `src` copied to where `dst`'s storage keeps it (same dims, same F).  One
// thread per element, channel fastest.  Used to keep a split-layout SHADOW of a grid held in the reference's two tensors: the
// forward passes gather from the shadow (aligned 16-byte base records, density and degree-0 colour in one gather), the
// gradients are produced in the layout of the Parameters.
__global__ void convert_grid_kernel(GridArgs src, GridArgs dst, float* dst_first, float* dst_second, unsigned int nodes) {
  // threadIdx.x = channel (32 or 64 lanes per node, the ones beyond F + 1 idle), threadIdx.y = node within the block: no
  // division for the channel, 32-bit index arithmetic throughout (node counts are < 2^32)
  const int C = dst.F + 1, K = dst.F / 3;
  const int ch = threadIdx.x;
  const bool linear = !src.bricked && !dst.bricked;  // node index = linear index in both
  for (unsigned int node = blockIdx.x * blockDim.y + threadIdx.y; node < nodes; node += gridDim.x * blockDim.y) {
    if (ch >= C) continue;
    unsigned int ls = node, ld = node;
    if (!linear) {
      const unsigned int z = node % (unsigned)dst.Z, t = node / (unsigned)dst.Z;
      const unsigned int y = t % (unsigned)dst.Y, x = t / (unsigned)dst.Y;
      ls = node_lin(src, (int)x, (int)y, (int)z);
      ld = node_lin(dst, (int)x, (int)y, (int)z);
    }
    bool sf, df;
    const long long so = channel_offset(src, ls, ch, K, sf);
    const long long doff = channel_offset(dst, ld, ch, K, df);
    (df ? dst_first : dst_second)[doff] = (sf ? src.dens : src.feat)[so];
  }
}

// The common case of the re-layout -- reference tensors -> split tensors, both in linear node order, whole quads per node (SH degree
// 0 or 2) -- one thread per destination float4: quad 0 of a node = (density, degree-0 r, g, b), quad q >= 1 = rest[4 (q - 1) ..].
// The four source floats are 4-byte gathers inside the node's 108-byte feature record (cache hits); the store is a coalesced 16 B.
template <int K>
__global__ void reference_to_split_kernel(const float* __restrict__ dens, const float* __restrict__ feat, long long dstride, long long fstride,
                                          float4* __restrict__ base, float4* __restrict__ rest, unsigned int nodes) {
  constexpr int QN = (3 * K + 1) / 4;  // quads per node
  constexpr int KR = K > 1 ? K - 1 : 1;
  const unsigned int total = nodes * QN;
  for (unsigned int it = blockIdx.x * blockDim.x + threadIdx.x; it < total; it += gridDim.x * blockDim.x) {
    const unsigned int node = it / QN, q = it - node * QN;
    const float* f = feat + (long long)node * fstride;
    if (q == 0) {
      base[node] = make_float4(dens[(long long)node * dstride], f[0], f[K], f[2 * K]);
    } else {
      float v[4];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const unsigned int r = 4 * (q - 1) + x;
        const unsigned int colour = r / KR, k = r - colour * KR + 1;
        v[x] = f[colour * K + k];
      }
      rest[(long long)node * (QN - 1) + (q - 1)] = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

// ... and back: split tensors -> reference tensors, one thread per SOURCE float4 (coalesced 16-byte load, four 4-byte stores inside the
// node's feature record).  Used when the split shadow is the copy the optimizer updated (deferred gradients, optim.FlatGrid).
template <int K>
__global__ void split_to_reference_kernel(const float4* __restrict__ base, const float4* __restrict__ rest, float* __restrict__ dens,
                                          float* __restrict__ feat, long long dstride, long long fstride, unsigned int nodes) {
  constexpr int QN = (3 * K + 1) / 4;
  constexpr int KR = K > 1 ? K - 1 : 1;
  const unsigned int total = nodes * QN;
  for (unsigned int it = blockIdx.x * blockDim.x + threadIdx.x; it < total; it += gridDim.x * blockDim.x) {
    const unsigned int node = it / QN, q = it - node * QN;
    float* f = feat + (long long)node * fstride;
    if (q == 0) {
      const float4 v = base[node];
      dens[(long long)node * dstride] = v.x;
      f[0] = v.y;
      f[K] = v.z;
      f[2 * K] = v.w;
    } else {
      const float4 v4 = rest[(long long)node * (QN - 1) + (q - 1)];
      const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const unsigned int r = 4 * (q - 1) + x;
        const unsigned int colour = r / KR, k = r - colour * KR + 1;
        f[colour * K + k] = v[x];
      }
    }
  }
}

// The same re-layout with coalesced 16-byte STORES for contiguous reference tensors (features [nodes * F] and densities [nodes] written
// as float4s, each gathering its four source floats -- cache hits inside the nodes' base / rest records): 0.164 -> ms of the per-element
// store version on the 128^3 / SH-2 grid.
template <int K>
__global__ void split_to_reference_quads_kernel(const float* __restrict__ base, const float* __restrict__ rest, float4* __restrict__ dens4,
                                                float4* __restrict__ feat4, unsigned int nodes) {
  constexpr unsigned int F = 3 * K, R = F - 3;
  constexpr unsigned int KR = K > 1 ? K - 1 : 1;
  const unsigned int fq = nodes * F / 4, dq = nodes / 4;  // (host-checked: nodes % 4 == 0)
  for (unsigned int it = blockIdx.x * blockDim.x + threadIdx.x; it < fq + dq; it += gridDim.x * blockDim.x) {
    float v[4];
    if (it < fq) {
#pragma unroll
      for (unsigned int x = 0; x < 4; ++x) {
        const unsigned int f = 4 * it + x, node = f / F, c = f - node * F;
        const unsigned int colour = c / K, k = c - colour * K;
        v[x] = (k == 0) ? base[node * 4 + 1 + colour] : rest[node * R + colour * KR + (k - 1)];
      }
      feat4[it] = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      const unsigned int n0 = 4 * (it - fq);
      dens4[it - fq] = make_float4(base[n0 * 4], base[n0 * 4 + 4], base[n0 * 4 + 8], base[n0 * 4 + 12]);
    }
  }
}

// =============================================================================================
// standalone point query: VoxelGrid.forward (thre3d_reprs/voxels.py:276-331) and its adjoint.
// One thread per (point, output channel); channel c < F is feature c in the reference order (colour*K + k),
// channel F is the activated density.  Any point is allowed (zeros padding outside the grid, no AABB mask --
// the mask belongs to process_points).  Not a hot path: the renderer uses the fused kernels above.
// =============================================================================================
__global__ void grid_query_kernel(GridArgs g, const float* __restrict__ points, long long n, float* __restrict__ out) {
  const int C = g.F + 1;
  const long long total = n * C;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const long long pt = idx / C;
    const int c = (int)(idx % C);
    const float p[3] = {points[pt * 3], points[pt * 3 + 1], points[pt * 3 + 2]};
    int i0[3];
    float w0[3], w1[3];
    query_cell(p, g, i0, w0, w1);
    const bool dens = (c == g.F);
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const QueryCorner qc = query_corner(k, i0, w0, w1, g);
      if (qc.ok) {
        bool first;
        const long long off = query_offset(c, qc.lin, g, &first);
        float v = first ? g.dens[off] : g.feat[off];
        if (dens) {
          v = v * g.rho;
          if (g.mode == RF_DENSITY_ABS) v = fabsf(v);
        }
        acc = acc + v * qc.w;
      }
    }
    out[idx] = dens ? density_post(acc, g.mode) : acc;
  }
}

__global__ void grid_query_backward_kernel(GridArgs g, const float* __restrict__ points, long long n,
                                           const float* __restrict__ gout, float* gfirst, float* gsecond) {
  const int C = g.F + 1;
  const long long total = n * C;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const long long pt = idx / C;
    const int c = (int)(idx % C);
    float go = gout[idx];
    if (go == 0.0f) continue;
    const float p[3] = {points[pt * 3], points[pt * 3 + 1], points[pt * 3 + 2]};
    int i0[3];
    float w0[3], w1[3];
    query_cell(p, g, i0, w0, w1);
    const bool dens = (c == g.F);
    if (dens && (g.mode == RF_DENSITY_RELU || g.mode == RF_DENSITY_SOFTPLUS)) {
      float pre = 0.0f;  // the activation derivative needs the interpolated pre-activation
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const QueryCorner qc = query_corner(k, i0, w0, w1, g);
        if (qc.ok) pre = pre + (g.dens[qc.lin * g.dstride] * g.rho) * qc.w;
      }
      if (g.mode == RF_DENSITY_RELU)
        go = (pre > 0.0f) ? go : 0.0f;
      else
        go = go * ((pre > 20.0f) ? 1.0f : 1.0f / (1.0f + expf(-pre)));
      if (go == 0.0f) continue;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const QueryCorner qc = query_corner(k, i0, w0, w1, g);
      if (!qc.ok) continue;
      bool first;
      const long long off = query_offset(c, qc.lin, g, &first);
      float gv = qc.w * go;
      if (dens) {
        gv = gv * g.rho;
        if (g.mode == RF_DENSITY_ABS) {
          const float dv = g.dens[off] * g.rho;
          gv = (dv > 0.f) ? gv : ((dv < 0.f) ? -gv : 0.0f);
        }
      }
      if (gv != 0.0f) unsafeAtomicAdd((first ? gfirst : gsecond) + off, gv);
    }
  }
}

// =============================================================================================
// occupancy mask (exact empty-space skipping for the ReLU field)
// =============================================================================================
__global__ void build_occupancy_kernel(GridArgs g, float threshold, uint32_t* occ, long long nwords) {
  // one lane per cell, 64 consecutive cells (z fastest) per wave -> two mask words per __ballot; the 8 nodes of
  // neighbouring cells overlap, so the loads hit L1
  const long long ncell = (long long)(g.X + 1) * (g.Y + 1) * (g.Z + 1);
  const long long nwave_items = (ncell + 63) / 64;
  const int lane = threadIdx.x & 63;
  const long long wave0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long wave_stride = ((long long)gridDim.x * blockDim.x) >> 6;
  for (long long item = wave0; item < nwave_items; item += wave_stride) {
    const long long cell = item * 64 + lane;
    bool occ_cell = false;
    if (cell < ncell) {
      occ_cell = (g.mode != RF_DENSITY_RELU);
      if (!occ_cell) {
        const int cz = (int)(cell % (g.Z + 1));
        const long long t = cell / (g.Z + 1);
        const int cy = (int)(t % (g.Y + 1)), cx = (int)(t / (g.Y + 1));
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int x = cx - 1 + (k & 1), y = cy - 1 + ((k >> 1) & 1), z = cz - 1 + (k >> 2);
          if (x >= 0 && x < g.X && y >= 0 && y < g.Y && z >= 0 && z < g.Z)
            occ_cell = occ_cell || (g.dens[(long long)node_lin(g, x, y, z) * g.dstride] * g.rho > threshold);
        }
      }
    }
    const unsigned long long bits = __ballot(occ_cell);
    if (lane == 0 && item * 2 < nwords) occ[item * 2] = (uint32_t)bits;
    if (lane == 32 && item * 2 + 1 < nwords) occ[item * 2 + 1] = (uint32_t)(bits >> 32);
  }
}

// =============================================================================================
// rf_tv_grad: total variation of the raw grid parameters.  For node n and channel c, with
// d_a(n) = theta[n + e_a] - theta[n] (0 where n + e_a lies outside the grid) and r(n) = sqrt(eps + sum_a d_a(n)^2):
//   g(n) = w * [ -(d_x(n) + d_y(n) + d_z(n)) / r(n) + sum_a d_a(n - e_a) / r(n - e_a) ]      (terms outside the grid dropped)
// GATHER form: one thread owns V consecutive channels of one (y, z) column of an x-slab of kTvSlab nodes, reads the parameters
// only, and adds g to its own gradient elements -- no atomics on the gradient, bitwise reproducible.  Lanes run over the
// (z, channel) row, so every neighbour load of a wave is a contiguous row segment (split storage, SH degree 0 / 2: one float4 of a
// node per lane).  Walking x in registers, the centre, its -y and its -z neighbour are the +x loads of the plane before and the
// x term d_x(n - e_x) / r(n - e_x) is the plane before's own d_x / r: 7 parameter loads per element instead of 13, the rest
// served by L1 / L2 (the four waves of a workgroup are four neighbouring y rows).  Padding nodes of bricked storage are never
// addressed: every neighbour is tested against the grid's dims first.
// =============================================================================================
constexpr int kTvSlab = 8;   // x planes per workgroup
constexpr int kTvRows = 4;   // y rows per workgroup (one wave each)

template <int V>
struct TvVec {
  float v[V];
};
template <int V>
__device__ __forceinline__ TvVec<V> tv_load(const float* p) {
  TvVec<V> r;
  if constexpr (V == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    r.v[0] = q.x, r.v[1] = q.y, r.v[2] = q.z, r.v[3] = q.w;
  } else {
    r.v[0] = *p;
  }
  return r;
}
template <int V>
__device__ __forceinline__ void tv_store(float* p, const TvVec<V>& r) {
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  } else {
    *p = r.v[0];
  }
}
// 1 / r = 1 / sqrt(eps + dx^2 + dy^2 + dz^2): three fused multiply-adds, a correctly rounded square root and division
__device__ __forceinline__ float tv_inv_norm(float dx, float dy, float dz, float eps) {
  return 1.0f / sqrtf(fmaf(dz, dz, fmaf(dy, dy, fmaf(dx, dx, eps))));
}

template <int K, int V, bool SUMS>
__global__ __launch_bounds__(kWave * kTvRows) void tv_grad_kernel(GridArgs g, float wd, float wf, float eps, float* __restrict__ gfirst,
                                                                  float* __restrict__ gsecond, float* __restrict__ sums) {
  constexpr int C = 3 * K + 1, Q = C / V;  // channels per node in accumulator order (channel_offset), lanes per node
  const unsigned it = blockIdx.x * kWave + threadIdx.x;
  const int z = (int)(it / Q), ch = (int)(it - (unsigned)z * Q) * V;
  const int y = blockIdx.y * kTvRows + threadIdx.y;
  const int x0 = blockIdx.z * kTvSlab, x1 = min(x0 + kTvSlab, g.X);
  float sum_d = 0.0f, sum_f = 0.0f;
  float w[V];
  bool write = false;
#pragma unroll
  for (int c = 0; c < V; ++c) {
    w[c] = (ch + c == 0) ? wd : wf;
    write = write || w[c] != 0.0f;
  }
  if (y < g.Y && z < g.Z && (write || SUMS)) {
    bool first;
    const long long coff = channel_offset(g, 0u, ch, K, first);  // the channel's place inside a node's record
    const float* src = (first ? g.dens : g.feat) + coff;
    float* dst = (first ? gfirst : gsecond) + coff;
    const long long stride = first ? g.dstride : g.fstride;
    auto off = [&](int xi, int yi, int zi) { return (long long)node_lin(g, xi, yi, zi) * stride; };
    auto at = [&](int xi, int yi, int zi) { return tv_load<V>(src + off(xi, yi, zi)); };
    const bool ly = y > 0, lz = z > 0, hy = y + 1 < g.Y, hz = z + 1 < g.Z;
    TvVec<V> t = at(x0, y, z), my = t, mz = t, tx;
    if (ly) my = at(x0, y - 1, z);
    if (lz) mz = at(x0, y, z - 1);
    if (x0 > 0) {  // the x term of the slab's first plane, computed the way the loop computes it for the plane before
      const TvVec<V> m = at(x0 - 1, y, z), py = hy ? at(x0 - 1, y + 1, z) : m, pz = hz ? at(x0 - 1, y, z + 1) : m;
#pragma unroll
      for (int c = 0; c < V; ++c) {
        const float dx = t.v[c] - m.v[c];
        tx.v[c] = dx * tv_inv_norm(dx, py.v[c] - m.v[c], pz.v[c] - m.v[c], eps);
      }
    }
    for (int x = x0; x < x1; ++x) {
      const bool hx = x + 1 < g.X;
      // a missing upper neighbour is replaced by the node itself: its difference is then exactly 0
      const TvVec<V> fx = hx ? at(x + 1, y, z) : t, fy = hy ? at(x, y + 1, z) : t, fz = hz ? at(x, y, z + 1) : t;
      TvVec<V> myx = my, myz = my, mzx = mz, mzy = mz;
      if (ly) {
        if (hx) myx = at(x + 1, y - 1, z);
        if (hz) myz = at(x, y - 1, z + 1);
      }
      if (lz) {
        if (hx) mzx = at(x + 1, y, z - 1);
        if (hy) mzy = at(x, y + 1, z - 1);
      }
      TvVec<V> acc;
#pragma unroll
      for (int c = 0; c < V; ++c) {
        const float dx = fx.v[c] - t.v[c], dy = fy.v[c] - t.v[c], dz = fz.v[c] - t.v[c];
        const float inv = tv_inv_norm(dx, dy, dz, eps);
        const float px = dx * inv;
        float a = (-px - dy * inv) - dz * inv;
        if (x > 0) a += tx.v[c];
        if (ly) {
          const float e = t.v[c] - my.v[c];
          a += e * tv_inv_norm(myx.v[c] - my.v[c], e, myz.v[c] - my.v[c], eps);
        }
        if (lz) {
          const float e = t.v[c] - mz.v[c];
          a += e * tv_inv_norm(mzx.v[c] - mz.v[c], mzy.v[c] - mz.v[c], e, eps);
        }
        tx.v[c] = px;
        acc.v[c] = a;
        if (SUMS) {
          const float r = sqrtf(fmaf(dz, dz, fmaf(dy, dy, fmaf(dx, dx, eps))));
          if (ch + c == 0) sum_d += r; else sum_f += r;
        }
      }
      if (write) {  // (a channel whose weight is 0 keeps its bits; a tensor whose channels all have weight 0 is not touched)
        float* p = dst + off(x, y, z);
        TvVec<V> old = tv_load<V>(p);
#pragma unroll
        for (int c = 0; c < V; ++c)
          if (w[c] != 0.0f) old.v[c] += w[c] * acc.v[c];
        tv_store<V>(p, old);
      }
      t = fx, my = myx, mz = mzx;
    }
  }
  if (SUMS) {  // sum of r per kind: wave -> workgroup -> one atomic add each (the sums are for logging; the gradient has no atomics)
    __shared__ float s_part[2][kTvRows];
    sum_d = wave_sum(sum_d);
    sum_f = wave_sum(sum_f);
    if (threadIdx.x == 0) s_part[0][threadIdx.y] = sum_d, s_part[1][threadIdx.y] = sum_f;
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
      float a = 0.0f, b = 0.0f;
      for (int r = 0; r < kTvRows; ++r) a += s_part[0][r], b += s_part[1][r];
      unsafeAtomicAdd(sums + 0, a);
      unsafeAtomicAdd(sums + 1, b);
    }
  }
}

// rf_prune_grid: keep(n) = some node m of the grid with |m - n|_inf <= dilate has M[m] > threshold; a pruned node's raw density
// is lowered to the fill.  GATHER form: one thread owns a node, reads the (2 dilate + 1)^3 neighbourhood of M (plain node order,
// clipped to the grid) and writes only its own density element (node_lin: padding nodes of bricked storage are never addressed).
// The two counters take one atomic add per wave.
__global__ __launch_bounds__(256) void prune_grid_kernel(GridArgs g, const float* __restrict__ M, float threshold, int dilate, float fill,
                                                         float* __restrict__ dens, unsigned char* __restrict__ keep_out,
                                                         unsigned long long* __restrict__ counts, long long nodes) {
  const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool real = n < nodes;
  bool keep = false;
  if (real) {
    const int z = (int)(n % g.Z), y = (int)((n / g.Z) % g.Y), x = (int)(n / ((long long)g.Z * g.Y));
    const int x0 = max(x - dilate, 0), x1 = min(x + dilate, g.X - 1), y0 = max(y - dilate, 0), y1 = min(y + dilate, g.Y - 1);
    const int z0 = max(z - dilate, 0), z1 = min(z + dilate, g.Z - 1);
    for (int xi = x0; xi <= x1 && !keep; ++xi)
      for (int yi = y0; yi <= y1 && !keep; ++yi) {
        const float* row = M + ((long long)xi * g.Y + yi) * g.Z;
        for (int zi = z0; zi <= z1; ++zi) keep = keep || row[zi] > threshold;
      }
    if (keep_out) keep_out[n] = keep ? 1 : 0;
    if (!keep) {
      float* p = dens + (long long)node_lin(g, x, y, z) * g.dstride;
      const float D = *p;
      if (g.mode == RF_DENSITY_ABS) {
        *p = 0.0f;
      } else if (fill < D) {  // min(D, fill): pruning never raises a density (a density at or below the fill keeps its bits)
        *p = fill;
      }
    }
  }
  if (counts) {
    const unsigned long long kept = __popcll(__ballot(real && keep)), pruned = __popcll(__ballot(real && !keep));
    if ((threadIdx.x & (kWave - 1)) == 0) {
      if (kept) atomicAdd(counts + 0, kept);
      if (pruned) atomicAdd(counts + 1, pruned);
    }
  }
}

// rf_node_bounds: the index box of the nodes whose OWN activated density sigma_n = post(pre(D_n * rho)) exceeds the threshold (no
// interpolation), merged into bounds[0..2] (min) / bounds[3..5] (max), and their number added to count[0].  One thread per node, z
// fastest; only a node's density element is read (node_lin: padding nodes of bricked storage are never addressed).  A wave whose
// ballot is empty does nothing; otherwise its six values are reduced with xor shuffles (lanes that do not pass carry the neutral
// elements) and lane 0 issues six int32 atomicMin / atomicMax and one 64-bit add.  Integer atomics: the result does not depend on
// the order of arrival.
__global__ __launch_bounds__(256) void node_bounds_kernel(GridArgs g, float threshold, int* __restrict__ bounds,
                                                          unsigned long long* __restrict__ count, long long nodes) {
  const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {-1, -1, -1};
  bool pass = false;
  if (n < nodes) {
    const int z = (int)(n % g.Z), y = (int)((n / g.Z) % g.Y), x = (int)(n / ((long long)g.Z * g.Y));
    float pre = g.dens[(long long)node_lin(g, x, y, z) * g.dstride] * g.rho;
    if (g.mode == RF_DENSITY_ABS) pre = fabsf(pre);
    pass = density_post(pre, g.mode) > threshold;
    if (pass) {
      lo[0] = hi[0] = x;
      lo[1] = hi[1] = y;
      lo[2] = hi[2] = z;
    }
  }
  const unsigned long long ballot = __ballot(pass);
  if (ballot == 0ull) return;  // (wave-uniform)
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = min(lo[a], __shfl_xor(lo[a], off, kWave));
      hi[a] = max(hi[a], __shfl_xor(hi[a], off, kWave));
    }
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      atomicMin(bounds + a, lo[a]);
      atomicMax(bounds + 3 + a, hi[a]);
    }
    if (count) atomicAdd(count, (unsigned long long)__popcll(ballot));
  }
}

// rf_resample_grid: the RAW [F+1]-channel volume of `src` seen from another lattice.  Destination node i on axis a sits at the
// continuous source index s_a = fma(scale_a, i_a, offset_a); a node with some s_a outside [-0.5, n_a - 0.5] (the source BOX: nodes are
// voxel centres) is (fill, 0 ...), any other takes the trilinear sum of the 8 corners of its cell with s_a clamped to [0, n_a - 1],
// i0 = min(floor(s), n - 1), i1 = min(i0 + 1, n - 1), lambda = s - i0.  No density scale, no activation.  The thread shape of
// upsample_grid_kernel: one thread per (destination node, channel), channel fastest, any storage on either side.
// SUMMATION ORDER (fixed, part of the contract): corner k = dx * 4 + dy * 2 + dz ascending, weight (wx * wy) * wz,
// v = val[0] * w[0], then v = fma(val[k], w[k], v) for k = 1 .. 7.  With scale 1 and an integer offset every weight is exactly 1 or 0:
// a bit-exact copy of finite values.
__device__ __forceinline__ AxisLerp resample_axis(int dst, int in_size, float scale, float offset) {
  float s = fmaf(scale, (float)dst, offset);
  AxisLerp a;
  a.outside = s < -0.5f || s > (float)in_size - 0.5f;
  s = fminf(fmaxf(s, 0.0f), (float)(in_size - 1));
  a.i0 = min((int)floorf(s), in_size - 1);
  a.i1 = min(a.i0 + 1, in_size - 1);
  const float lambda = s - (float)a.i0;
  a.w0 = 1.0f - lambda;
  a.w1 = lambda;
  return a;
}

struct ResampleMap {
  float scale[3], offset[3];
};

__global__ __launch_bounds__(256) void resample_grid_kernel(GridArgs src, GridArgs dst, ResampleMap m, float fill, float* dst_first,
                                                            float* dst_second, long long total) {
  const int K = dst.F / 3;
  for (long long it = (long long)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (long long)gridDim.x * blockDim.x) {
    const NodeChannel n = node_channel(it, dst);
    const int ch = n.ch, x = n.x, y = n.y, z = n.z;
    const AxisLerp ax = resample_axis(x, src.X, m.scale[0], m.offset[0]), ay = resample_axis(y, src.Y, m.scale[1], m.offset[1]),
                   az = resample_axis(z, src.Z, m.scale[2], m.offset[2]);
    float v;
    if (ax.outside || ay.outside || az.outside) {
      v = ch == 0 ? fill : 0.0f;
    } else {
      auto at = [&](int xi, int yi, int zi) -> float {
        bool first;
        const long long off = channel_offset(src, node_lin(src, xi, yi, zi), ch, K, first);
        return (first ? src.dens : src.feat)[off];
      };
      float val[8], wgt[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int dx = k >> 2, dy = (k >> 1) & 1, dz = k & 1;
        val[k] = at(dx ? ax.i1 : ax.i0, dy ? ay.i1 : ay.i0, dz ? az.i1 : az.i0);
        wgt[k] = ((dx ? ax.w1 : ax.w0) * (dy ? ay.w1 : ay.w0)) * (dz ? az.w1 : az.w0);
      }
      v = val[0] * wgt[0];
#pragma unroll
      for (int k = 1; k < 8; ++k) v = fmaf(val[k], wgt[k], v);
    }
    bool first;
    const long long off = channel_offset(dst, node_lin(dst, x, y, z), ch, K, first);
    (first ? dst_first : dst_second)[off] = v;
  }
}

}  // namespace

extern "C" {

int rf_grid_query(const RFGrid* grid, const float* points_dev, int64_t num_points, float* out_dev, void* stream) {
  const int rc = check_grid(grid);
  if (rc != RF_OK) return rc;
  if (num_points == 0) return RF_OK;
  if (!points_dev || !out_dev) return RF_ERR_NULL_POINTER;
  if (num_points < 0) return RF_ERR_BAD_SHAPE;
  const GridArgs g = to_args(grid);
  const long long total = (long long)num_points * (g.F + 1);
  hipLaunchKernelGGL(grid_query_kernel, dim3(grid_1d(total, 256)), dim3(256), 0, (hipStream_t)stream, g, points_dev,
                     (long long)num_points, out_dev);
  return launch_status();
}

int rf_grid_query_backward(const RFGrid* grid, const float* points_dev, int64_t num_points, const float* grad_out_dev,
                           float* grad_densities_dev, float* grad_features_dev, void* stream) {
  const int rc = check_grid(grid);
  if (rc != RF_OK) return rc;
  if (num_points == 0) return RF_OK;
  if (!points_dev || !grad_out_dev || !grad_densities_dev) return RF_ERR_NULL_POINTER;
  if (!grad_features_dev && !second_tensor_optional(grid)) return RF_ERR_NULL_POINTER;
  if (num_points < 0) return RF_ERR_BAD_SHAPE;
  const GridArgs g = to_args(grid);
  const long long total = (long long)num_points * (g.F + 1);
  hipLaunchKernelGGL(grid_query_backward_kernel, dim3(grid_1d(total, 256)), dim3(256), 0, (hipStream_t)stream, g,
                     points_dev, (long long)num_points, grad_out_dev, grad_densities_dev, grad_features_dev);
  return launch_status();
}

int rf_build_occupancy(const RFGrid* grid, float threshold, uint32_t* occupancy_dev, void* stream) {
  const int rc = check_grid(grid);
  if (rc != RF_OK) return rc;
  if (!occupancy_dev) return RF_ERR_NULL_POINTER;
  const GridArgs g = to_args(grid);
  const long long ncell = (long long)(g.X + 1) * (g.Y + 1) * (g.Z + 1);
  const long long nwords = (ncell + 31) / 32;
  hipLaunchKernelGGL(build_occupancy_kernel, dim3(grid_1d(ncell, 256, 256LL * 32)), dim3(256), 0, (hipStream_t)stream, g,
                     threshold, occupancy_dev, nwords);
  return launch_status();
}

int rf_upsample_grid(const RFGrid* src, const RFGrid* dst, void* stream) {
  int rc = check_grid(src);
  if (rc != RF_OK) return rc;
  rc = check_grid(dst);
  if (rc != RF_OK) return rc;
  if (src->num_features != dst->num_features) return RF_ERR_BAD_SHAPE;
  if (src->densities_dev == dst->densities_dev || (dst->features_dev && src->features_dev == dst->features_dev)) return RF_ERR_BAD_SHAPE;
  const GridArgs gs = to_args(src), gd = to_args(dst);
  const long long total = (long long)gd.X * gd.Y * gd.Z * (gd.F + 1);
  hipLaunchKernelGGL(upsample_grid_kernel, dim3(grid_1d(total, 256, 256LL * 64)), dim3(256), 0, (hipStream_t)stream, gs, gd,
                     const_cast<float*>(dst->densities_dev), const_cast<float*>(dst->features_dev), total);
  return launch_status();
}

int rf_tv_grad(const RFGrid* grid, float weight_density, float weight_features, float epsilon, float* grad_first_dev,
               float* grad_second_dev, float* sums_dev, void* stream) {
  const int rc = check_grid(grid);
  if (rc != RF_OK) return rc;
  if (!(epsilon > 0.0f) || !std::isfinite(epsilon)) return RF_ERR_BAD_SHAPE;
  if (!(weight_density >= 0.0f) || !(weight_features >= 0.0f) || !std::isfinite(weight_density) || !std::isfinite(weight_features)) return RF_ERR_BAD_SHAPE;
  if (weight_density == 0.0f && weight_features == 0.0f) return RF_OK;
  // which gradient tensors the weights reach: split / bricked storage keeps the degree-0 coefficients beside the density
  const bool split = grid->layout != RF_LAYOUT_REFERENCE;
  const bool need_first = weight_density != 0.0f || split;
  const bool need_second = weight_features != 0.0f && !(split && grid->num_features == 3);
  if ((need_first && !grad_first_dev) || (need_second && !grad_second_dev)) return RF_ERR_NULL_POINTER;
  // the gradient is added to tensors of its own, never to the parameters
  if ((grad_first_dev && grad_first_dev == grid->densities_dev) || (grad_second_dev && grad_second_dev == grid->features_dev)) return RF_ERR_BAD_SHAPE;
  const GridArgs g = to_args(grid);
  const int K = g.F / 3, C = g.F + 1;
  // one float4 of a node per lane where every node record is whole, aligned float4s
  const uintptr_t ptrs = (uintptr_t)grid->densities_dev | (uintptr_t)grid->features_dev | (uintptr_t)grad_first_dev | (uintptr_t)grad_second_dev;
  const bool quads = split && C % 4 == 0 && g.dstride % 4 == 0 && g.fstride % 4 == 0 && (ptrs & 15u) == 0;
  const long long row = (long long)g.Z * (quads ? C / 4 : C);
  const dim3 blocks((unsigned)((row + kWave - 1) / kWave), (unsigned)((g.Y + kTvRows - 1) / kTvRows), (unsigned)((g.X + kTvSlab - 1) / kTvSlab));
  const dim3 threads(kWave, kTvRows);
  // the weights of the two MEANS as per-element factors: w = lambda_D / N, lambda_F / (N F)
  const double nodes = (double)g.X * g.Y * g.Z;
  const float wd = (float)((double)weight_density / nodes), wf = (float)((double)weight_features / (nodes * g.F));
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, blocks, threads, 0, (hipStream_t)stream, g, wd, wf, epsilon, grad_first_dev, grad_second_dev, sums_dev);
    return launch_status();
  };
  if (quads)
    return dispatch_sh(K, ShEven{}, [&](auto k) {
      constexpr int KK = decltype(k)::value;
      return sums_dev ? launch(tv_grad_kernel<KK, 4, true>) : launch(tv_grad_kernel<KK, 4, false>);
    });
  return dispatch_sh(K, ShAll{}, [&](auto k) {
    constexpr int KK = decltype(k)::value;
    return sums_dev ? launch(tv_grad_kernel<KK, 1, true>) : launch(tv_grad_kernel<KK, 1, false>);
  });
}

int rf_prune_grid(const RFGrid* grid, const float* max_weight_dev, float threshold, int32_t dilate, float fill_density, float* densities_dev,
                  uint8_t* keep_dev, int64_t* counts_dev, void* stream) {
  const int rc = check_grid(grid);
  if (rc != RF_OK) return rc;
  if (!max_weight_dev || !densities_dev) return RF_ERR_NULL_POINTER;
  if (dilate < 0 || dilate > 4) return RF_ERR_BAD_SHAPE;
  if (!(threshold >= 0.0f) || !std::isfinite(threshold)) return RF_ERR_BAD_SHAPE;
  if (fill_density != fill_density) return RF_ERR_BAD_SHAPE;
  if (grid->density_mode == RF_DENSITY_ABS && fill_density != 0.0f) return RF_ERR_BAD_SHAPE;  // |D| has one empty value
  const GridArgs g = to_args(grid);
  const long long nodes = (long long)g.X * g.Y * g.Z;
  hipLaunchKernelGGL(prune_grid_kernel, dim3((unsigned)((nodes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, max_weight_dev, threshold,
                     (int)dilate, fill_density, densities_dev, keep_dev, reinterpret_cast<unsigned long long*>(counts_dev), nodes);
  return launch_status();
}

int rf_node_bounds(const RFGrid* grid, float threshold, int32_t* bounds_dev, int64_t* count_dev, void* stream) {
  const int rc = check_grid(grid);
  if (rc != RF_OK) return rc;
  if (!bounds_dev) return RF_ERR_NULL_POINTER;
  if (!(threshold >= 0.0f)) return RF_ERR_BAD_SHAPE;  // (NaN fails the comparison too)
  const GridArgs g = to_args(grid);
  const long long nodes = (long long)g.X * g.Y * g.Z;
  hipLaunchKernelGGL(node_bounds_kernel, dim3((unsigned)((nodes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, threshold, bounds_dev,
                     reinterpret_cast<unsigned long long*>(count_dev), nodes);
  return launch_status();
}

int rf_resample_grid(const RFGrid* src, const RFGrid* dst, const float* scale, const float* offset, float fill_density, void* stream) {
  int rc = check_grid(src);
  if (rc != RF_OK) return rc;
  rc = check_grid(dst);
  if (rc != RF_OK) return rc;
  if (!scale || !offset) return RF_ERR_NULL_POINTER;
  if (src->num_features != dst->num_features) return RF_ERR_BAD_SHAPE;
  ResampleMap m;
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(scale[a]) || !(scale[a] > 0.0f) || !std::isfinite(offset[a])) return RF_ERR_BAD_SHAPE;
    m.scale[a] = scale[a];
    m.offset[a] = offset[a];
  }
  if (fill_density != fill_density) return RF_ERR_BAD_SHAPE;
  // the destination is written while the source is read: no tensor of one may be a tensor of the other
  const float* s[2] = {src->densities_dev, src->features_dev};
  const float* d[2] = {dst->densities_dev, dst->features_dev};
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j)
      if (s[i] && s[i] == d[j]) return RF_ERR_BAD_SHAPE;
  const GridArgs gs = to_args(src), gd = to_args(dst);
  const long long total = (long long)gd.X * gd.Y * gd.Z * (gd.F + 1);
  hipLaunchKernelGGL(resample_grid_kernel, dim3(grid_1d(total, 256, 256LL * 64)), dim3(256), 0, (hipStream_t)stream, gs, gd, m, fill_density,
                     const_cast<float*>(dst->densities_dev), const_cast<float*>(dst->features_dev), total);
  return launch_status();
}

int rf_convert_grid(const RFGrid* src, const RFGrid* dst, void* stream) {
  int rc = check_grid(src);
  if (rc != RF_OK) return rc;
  rc = check_grid(dst);
  if (rc != RF_OK) return rc;
  if (src->num_features != dst->num_features) return RF_ERR_BAD_SHAPE;
  for (int a = 0; a < 3; ++a)
    if (src->dims[a] != dst->dims[a]) return RF_ERR_BAD_SHAPE;
  if (src->densities_dev == dst->densities_dev || (dst->features_dev && src->features_dev == dst->features_dev)) return RF_ERR_BAD_SHAPE;
  const GridArgs gs = to_args(src), gd = to_args(dst);
  const unsigned int nodes = (unsigned)gd.X * (unsigned)gd.Y * (unsigned)gd.Z;
  const int K = gd.F / 3;
  if (src->layout == RF_LAYOUT_REFERENCE && dst->layout == RF_LAYOUT_SPLIT && (K == 1 || K == 9) && dst->density_stride == 4 &&
      (K == 1 || dst->feature_stride == gd.F - 3) && (((uintptr_t)dst->densities_dev | (uintptr_t)dst->features_dev) & 15u) == 0 &&
      (unsigned long long)nodes * 7ull < (1ull << 32)) {
    float4* base = reinterpret_cast<float4*>(const_cast<float*>(dst->densities_dev));
    float4* rest = reinterpret_cast<float4*>(const_cast<float*>(dst->features_dev));
    const unsigned blocks = grid_1d((long long)nodes * ((gd.F + 1) / 4), 256, 256LL * 64);
    return dispatch_sh(K, ShEven{}, [&](auto k) {
      hipLaunchKernelGGL((reference_to_split_kernel<decltype(k)::value>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, gs.dens, gs.feat, gs.dstride, gs.fstride, base, rest, nodes);
      return launch_status();
    });
  }
  if (src->layout == RF_LAYOUT_SPLIT && dst->layout == RF_LAYOUT_REFERENCE && (K == 1 || K == 9) && src->density_stride == 4 &&
      (K == 1 || src->feature_stride == gd.F - 3) && (((uintptr_t)src->densities_dev | (uintptr_t)src->features_dev) & 15u) == 0 &&
      (unsigned long long)nodes * 7ull < (1ull << 32)) {
    const float4* base = reinterpret_cast<const float4*>(src->densities_dev);
    const float4* rest = reinterpret_cast<const float4*>(src->features_dev);
    float* dd = const_cast<float*>(dst->densities_dev);
    float* df = const_cast<float*>(dst->features_dev);
    if (dst->density_stride == 1 && dst->feature_stride == gd.F && (nodes & 3u) == 0 && (((uintptr_t)dd | (uintptr_t)df) & 15u) == 0 &&
        (unsigned long long)nodes * (unsigned long long)gd.F < (1ull << 32)) {  // contiguous reference tensors: 16-byte stores
      const unsigned blocks4 = grid_1d((long long)nodes * gd.F / 4 + nodes / 4, 256, 256LL * 64);
      return dispatch_sh(K, ShEven{}, [&](auto k) {
        hipLaunchKernelGGL((split_to_reference_quads_kernel<decltype(k)::value>), dim3(blocks4), dim3(256), 0, (hipStream_t)stream, src->densities_dev, src->features_dev,
                           reinterpret_cast<float4*>(dd), reinterpret_cast<float4*>(df), nodes);
        return launch_status();
      });
    }
    const unsigned blocks = grid_1d((long long)nodes * ((gd.F + 1) / 4), 256, 256LL * 64);
    return dispatch_sh(K, ShEven{}, [&](auto k) {
      hipLaunchKernelGGL((split_to_reference_kernel<decltype(k)::value>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, base, rest, dd, df, gd.dstride, gd.fstride, nodes);
      return launch_status();
    });
  }
  const int cw = gd.F + 1 <= 32 ? 32 : 64, per_block = 256 / cw;
  hipLaunchKernelGGL(convert_grid_kernel, dim3(grid_1d(nodes, per_block, 256LL * 256)), dim3(cw, per_block), 0, (hipStream_t)stream, gs, gd,
                     const_cast<float*>(dst->densities_dev), const_cast<float*>(dst->features_dev), nodes);
  return launch_status();
}

}  // extern "C"
