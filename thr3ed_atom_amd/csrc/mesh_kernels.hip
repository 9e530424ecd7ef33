// mesh_kernels.hip -- iso-surface extraction of a ReLU field (rf_mesh_tiles / rf_mesh_count / rf_mesh_emit of relu_field.h).
//
// Contract (DESIGN.md "Iso-surface extraction"):
//   field     sigma(p) = post(interp(pre(D * rho))) under the grid's density mode: the density column of rf_grid_query
//             (grid_sample(align_corners=False) recipe, zeros padding); sigma = 0 for p on or outside the AABB.
//   lattice   subdivision m in [1, 8]; on axis a the index i in [-1, m * dim_a], stored shifted as u = i + 1 in [0, R_a),
//             R_a = m * dim_a + 2.  Interior points: aabb_min + (aabb_max - aabb_min) * ((2i + 1) / (2 m dim_a)) in float32;
//             the guards u = 0 and u = R_a - 1 sit on the AABB planes with sigma = 0, so every surface is closed.
//             lin(u) = (ux * Ry + uy) * Rz + uz (z fastest, int64).
//   inside    sigma > tau (strict).
//   tets      Kuhn split of each lattice cube: for the permutations pi of (x, y, z) in lexicographic order (xyz, xzy, yxz,
//             yzx, zxy, zyx) tet pi = (0, e_pi0, e_pi0 + e_pi1, (1,1,1)).  Every tet edge is a lattice edge (a, a + d),
//             d in {0,1}^3 \ {0}, with edge key 7 lin(a) + (4 dx + 2 dy + dz - 1).
//   vertices  one per crossing edge, at p_a + t (p_b - p_a), t = (tau - sigma_a) / (sigma_b - sigma_a), a the lower end.
//   faces     1-vs-3 tet: one triangle on the edges of the single vertex s to the others in tet-local order; 2-vs-2 tet:
//             quad (a0b0, a0b1, a1b1, a1b0) (a = inside pair, b = outside pair, tet-local order) split as (q0,q1,q2), (q0,q2,q3).
//             (v1 - v0) x (v2 - v0) points out of {sigma > tau}: decided from the permutation's parity and the case, never
//             from a float test (otherwise v1 and v2 swap).
//   order     vertices by ascending edge key, faces by ascending (lin(cube's lower corner), tet, triangle).
//   colour    sigmoid(C0 * interp(f[c * K + 0])); normal -(grad interp(pre(D * rho))) / |.| or 0 (floor cell convention).
//
// Decomposition.  A workgroup owns 256 CONSECUTIVE lattice points in lin order, one per thread; a thread owns the (up to 7)
// edges whose lower end is its point and the (up to 12) triangles of the cube whose lower corner it is.  The sigma values the
// workgroup needs are its points and their +x / +y / +z neighbours: four runs of 257 consecutive lin values (offsets 0, Rz,
// Ry Rz, Ry Rz + Rz), evaluated once into LDS.  Output slots inside a workgroup are exclusive prefix sums of the per-thread
// counts built from wave64 ballots of their bit planes (no atomics), and workgroups write in workgroup order: the output
// comes out in the canonical order above without a sort, and two extractions are bitwise identical.
#include "rf_device.h"

namespace {

constexpr int kMeshBlock = 256;  // lattice points per workgroup (4 waves)
constexpr int kMeshWaves = kMeshBlock / 64;
constexpr int kRun = kMeshBlock + 1;  // sigma values per run (the +z neighbour of the last point)

struct MeshArgs {
  const float* dens;  // reference: densities [.,1] (stride dstride); split / bricked: base [.,4] (stride dstride)
  const float* feat;  // reference: features [., F] (stride fstride); unused otherwise (colours come from the base record)
  int X, Y, Z, K;
  long long dstride, fstride;
  int split;    // the density and the three degree-0 coefficients are the 16-byte base record
  int bricked;  // 8^3-node bricks stored contiguously
  int nby, nbz;
  float amin[3], amax[3], ext[3], nscale[3], nbias[3];
  float rho;
  int mode;
  float tau;
  int m;
  int R[3];
  long long RyRz, total;  // lattice points
  long long nblocks;
};

__device__ __forceinline__ long long node_index(const MeshArgs& g, int x, int y, int z) {
  if (g.bricked)
    return ((((long long)(x >> 3) * g.nby + (y >> 3)) * g.nbz + (z >> 3)) << 9) + (((x & 7) << 6) | ((y & 7) << 3) | (z & 7));
  return ((long long)x * g.Y + y) * g.Z + z;
}

__device__ __forceinline__ float pre_density(const MeshArgs& g, long long node) {
  float v = g.dens[node * g.dstride] * g.rho;
  if (g.mode == RF_DENSITY_ABS) v = fabsf(v);
  return v;
}

__device__ __forceinline__ float post_density(float pre, int mode) {
  if (mode == RF_DENSITY_RELU) return fmaxf(pre, 0.0f);
  if (mode == RF_DENSITY_SOFTPLUS) return (pre > 20.0f) ? pre : log1pf(expf(pre));
  return pre;
}

// the grid_sample cell of point p: lower corner i0, weights of the lower (w0) and upper (w1) corner per axis (ATen's recipe)
__device__ __forceinline__ void mesh_cell(const MeshArgs& g, const float p[3], int i0[3], float w0[3], float w1[3]) {
  const int dims[3] = {g.X, g.Y, g.Z};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float q = p[a] * g.nscale[a] + g.nbias[a];
    const float idx = ((q + 1.0f) * (float)dims[a] - 1.0f) / 2.0f;
    const float fl = floorf(idx);
    w1[a] = idx - fl;
    w0[a] = (fl + 1.0f) - idx;
    i0[a] = (int)fminf(fmaxf(fl, -2.0f), (float)dims[a]);
  }
}

__device__ __forceinline__ bool corner_ok(const MeshArgs& g, int x, int y, int z) {
  return x >= 0 && x < g.X && y >= 0 && y < g.Y && z >= 0 && z < g.Z;
}

// interp(pre(D rho)) at p, corners in ATen's order (dx fastest), separate multiply and add
__device__ float interp_pre_density(const MeshArgs& g, const float p[3]) {
  int i0[3];
  float w0[3], w1[3];
  mesh_cell(g, p, i0, w0, w1);
  float acc = 0.0f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
    const int x = i0[0] + dx, y = i0[1] + dy, z = i0[2] + dz;
    if (corner_ok(g, x, y, z)) {
      const float w = ((dx ? w1[0] : w0[0]) * (dy ? w1[1] : w0[1])) * (dz ? w1[2] : w0[2]);
      acc = acc + pre_density(g, node_index(g, x, y, z)) * w;
    }
  }
  return acc;
}

// float32 position of lattice index u on axis a (guards on the AABB planes)
__device__ __forceinline__ float lattice_coord(const MeshArgs& g, int a, int u) {
  if (u <= 0) return g.amin[a];
  if (u >= g.R[a] - 1) return g.amax[a];
  const int dim = a == 0 ? g.X : (a == 1 ? g.Y : g.Z);
  const float frac = (float)(2 * (u - 1) + 1) / (float)(2 * g.m * dim);
  return g.amin[a] + g.ext[a] * frac;
}

__device__ float lattice_sigma(const MeshArgs& g, int ux, int uy, int uz) {
  const int u[3] = {ux, uy, uz};
  float p[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (u[a] <= 0 || u[a] >= g.R[a] - 1) return 0.0f;
    p[a] = lattice_coord(g, a, u[a]);
    if (!(p[a] > g.amin[a] && p[a] < g.amax[a])) return 0.0f;  // the renderer's strict inside test
  }
  return post_density(interp_pre_density(g, p), g.mode);
}

// lattice coordinates of lin value `base` (workgroup-uniform 64-bit division, once per run)
__device__ __forceinline__ void lattice_coords(const MeshArgs& g, long long base, int u[3]) {
  u[0] = (int)(base / g.RyRz);
  const long long rem = base - (long long)u[0] * g.RyRz;
  u[1] = (int)(rem / g.R[2]);
  u[2] = (int)(rem - (long long)u[1] * g.R[2]);
}

// base + j for 0 <= j <= 256, from the coordinates of base (32-bit carries)
__device__ __forceinline__ void advance_coords(const MeshArgs& g, const int u0[3], int j, int u[3]) {
  const int vz = u0[2] + j;
  u[2] = vz % g.R[2];
  const int vy = u0[1] + vz / g.R[2];
  u[1] = vy % g.R[1];
  u[0] = u0[0] + vy / g.R[1];
}

// sigma of the four runs of the workgroup starting at lin L0: run r = 2 dx + dy holds lin L0 + dx Ry Rz + dy Rz + j, j in [0, 256]
__device__ void stage_sigma(const MeshArgs& g, long long L0, float (*s)[kRun]) {
  for (int e = threadIdx.x; e < 4 * kRun; e += kMeshBlock) {
    const int r = e / kRun, j = e - r * kRun;
    const long long base = L0 + (r >> 1) * g.RyRz + (r & 1) * (long long)g.R[2];
    float v = 0.0f;
    if (base + j < g.total) {
      int u0[3], u[3];
      lattice_coords(g, base, u0);
      advance_coords(g, u0, j, u);
      v = lattice_sigma(g, u[0], u[1], u[2]);
    }
    s[r][j] = v;
  }
  __syncthreads();
}

__device__ __forceinline__ float sigma_at(float (*s)[kRun], int t, int dx, int dy, int dz) { return s[2 * dx + dy][t + dz]; }

// Kuhn tet `tet` (lexicographic permutation index): vertex k as a corner code 4 dx + 2 dy + dz of the cube
__device__ __forceinline__ int tet_vertex(int tet, int k) {
  // axes of the permutations xyz, xzy, yxz, yzx, zxy, zyx as bits x = 4, y = 2, z = 1
  const int a0 = (tet < 2) ? 4 : (tet < 4 ? 2 : 1);
  const int a1 = (tet == 0 || tet == 5) ? 2 : ((tet == 1 || tet == 3) ? 1 : 4);
  return k == 0 ? 0 : (k == 1 ? a0 : (k == 2 ? (a0 | a1) : 7));
}
__device__ __forceinline__ bool tet_even(int tet) { return tet == 0 || tet == 3 || tet == 4; }

// tet-local edge (x, y) as a nibble lo | hi << 2 (lo < hi)
__device__ __forceinline__ int edge_nibble(int x, int y) { return x < y ? (x | (y << 2)) : (y | (x << 2)); }

// the triangles of tet `tet` given which of its four vertices are inside (bit k = vertex k), packed into an int: bits 0-3 the
// number of triangles (0, 1 or 2), then 12 bits per triangle = three edge nibbles (vertex order of the triangle)
__device__ __forceinline__ int tet_case(int tet, int inside) {
  const int n = __popc(inside);
  const bool even_tet = tet_even(tet);
  if (n == 1 || n == 3) {
    const int single = (n == 1) ? (__ffs(inside) - 1) : (__ffs(~inside & 15) - 1);
    const int o0 = single == 0 ? 1 : 0, o1 = single <= 1 ? 2 : 1, o2 = single <= 2 ? 3 : 2;  // the others, ascending
    // (e(s,o0), e(s,o1), e(s,o2)) faces away from s iff det[o0 - s, o1 - s, o2 - s] > 0, i.e. iff the tet's orientation times the
    // parity of the sequence (s, o0, o1, o2) -- `single` inversions -- is positive
    const bool away = even_tet == ((single & 1) == 0);
    const bool flip = away != (n == 1);
    const int e0 = edge_nibble(single, o0), e1 = edge_nibble(single, o1), e2 = edge_nibble(single, o2);
    return 1 | ((e0 | ((flip ? e2 : e1) << 4) | ((flip ? e1 : e2) << 8)) << 4);
  }
  if (n == 2) {
    const int a0 = __ffs(inside) - 1, a1 = 31 - __clz(inside);
    const int out = ~inside & 15;
    const int b0 = __ffs(out) - 1, b1 = 31 - __clz(out);
    // the quad's normal points from the a pair to the b pair iff det[a1 - a0, b0 - a0, b1 - a0] > 0: the tet's orientation times
    // the parity of the sequence (a0, a1, b0, b1)
    const int inv = (a0 > b0) + (a0 > b1) + (a1 > b0) + (a1 > b1);
    const bool flip = even_tet != ((inv & 1) == 0);
    const int q0 = edge_nibble(a0, b0), q1 = edge_nibble(a0, b1), q2 = edge_nibble(a1, b1), q3 = edge_nibble(a1, b0);
    const int t0 = flip ? (q0 | (q2 << 4) | (q1 << 8)) : (q0 | (q1 << 4) | (q2 << 8));
    const int t1 = flip ? (q0 | (q3 << 4) | (q2 << 8)) : (q0 | (q2 << 4) | (q3 << 8));
    return 2 | (t0 << 4) | (t1 << 16);
  }
  return 0;
}

// per-thread counts: vertices (edges of its point that cross) and triangles (of its cube)
struct PointWork {
  int u[3];
  bool valid;
  int vmask;   // bit code-1 for each crossing edge direction code in 1..7
  int ncube;   // inside mask of the cube's 8 corners (corner code 4 dx + 2 dy + dz), -1 when the point is no cube corner
  int nfaces;
};

__device__ PointWork point_work(const MeshArgs& g, long long L0, float (*s)[kRun]) {
  PointWork w;
  const int t = threadIdx.x;
  const long long lin = L0 + t;
  w.valid = lin < g.total;
  w.vmask = 0;
  w.ncube = -1;
  w.nfaces = 0;
  if (!w.valid) return w;
  int u0[3];
  lattice_coords(g, L0, u0);
  advance_coords(g, u0, t, w.u);
  const bool in_a = sigma_at(s, t, 0, 0, 0) > g.tau;
  for (int code = 1; code < 8; ++code) {
    const int dx = code >> 2, dy = (code >> 1) & 1, dz = code & 1;
    if (w.u[0] + dx >= g.R[0] || w.u[1] + dy >= g.R[1] || w.u[2] + dz >= g.R[2]) continue;
    if ((sigma_at(s, t, dx, dy, dz) > g.tau) != in_a) w.vmask |= 1 << (code - 1);
  }
  if (w.u[0] + 1 < g.R[0] && w.u[1] + 1 < g.R[1] && w.u[2] + 1 < g.R[2]) {
    int ins = 0;
    for (int code = 0; code < 8; ++code)
      if (sigma_at(s, t, code >> 2, (code >> 1) & 1, code & 1) > g.tau) ins |= 1 << code;
    w.ncube = ins;
    if (ins != 0 && ins != 255) {
      for (int tet = 0; tet < 6; ++tet) {
        int tin = 0;
        for (int k = 0; k < 4; ++k) tin |= ((ins >> tet_vertex(tet, k)) & 1) << k;
        const int n = __popc(tin);
        w.nfaces += (n == 2) ? 2 : ((n == 1 || n == 3) ? 1 : 0);
      }
    }
  }
  return w;
}

// exclusive prefix (within the wave) and wave total of a count < 16, from the ballots of its four bit planes
__device__ __forceinline__ int wave_prefix(int count, int* total) {
  const int lane = threadIdx.x & 63;
  const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
  int prefix = 0, sum = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const unsigned long long bal = __ballot((count >> b) & 1);
    prefix += __popcll(bal & lt) << b;
    sum += __popcll(bal) << b;
  }
  *total = sum;
  return prefix;
}

// exclusive prefix over the workgroup of two counts (vertices, faces); wave totals meet in LDS
__device__ __forceinline__ void block_prefix(int nv, int nf, int* pv, int* pf, int* tv, int* tf) {
  __shared__ int wave_tot[2][kMeshWaves];
  int sv, sf;
  const int ev = wave_prefix(nv, &sv), ef = wave_prefix(nf, &sf);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    wave_tot[0][wave] = sv;
    wave_tot[1][wave] = sf;
  }
  __syncthreads();
  int ov = 0, of = 0, av = 0, af = 0;
  for (int w = 0; w < kMeshWaves; ++w) {
    if (w < wave) {
      ov += wave_tot[0][w];
      of += wave_tot[1][w];
    }
    av += wave_tot[0][w];
    af += wave_tot[1][w];
  }
  *pv = ov + ev;
  *pf = of + ef;
  *tv = av;
  *tf = af;
}

__global__ __launch_bounds__(kMeshBlock) void mesh_count_kernel(MeshArgs g, long long* __restrict__ counts) {
  __shared__ float s[4][kRun];
  for (long long blk = blockIdx.x; blk < g.nblocks; blk += gridDim.x) {
    const long long L0 = blk * kMeshBlock;
    stage_sigma(g, L0, s);
    const PointWork w = point_work(g, L0, s);
    int pv, pf, tv, tf;
    block_prefix(__popc(w.vmask), w.nfaces, &pv, &pf, &tv, &tf);
    if (threadIdx.x == 0) {
      counts[blk] = tv;
      counts[g.nblocks + blk] = tf;
    }
    __syncthreads();  // (LDS reused by the next block of the loop)
  }
}

struct EmitOut {
  const long long* offsets;  // [2, nblocks] exclusive prefix of the counts
  long long vcap, fcap;
  long long* keys;   // [V]
  float* pos;        // [V, 3]
  float* col;        // [V, 3] or NULL
  float* nrm;        // [V, 3] or NULL
  long long* fedge;  // [T, 3] edge keys of the face's vertices
};

__device__ __forceinline__ void vertex_attributes(const MeshArgs& g, const float p[3], bool want_col, bool want_nrm, float col[3], float nrm[3]) {
  int i0[3];
  float w0[3], w1[3];
  mesh_cell(g, p, i0, w0, w1);
  float c[3] = {0.0f, 0.0f, 0.0f}, gr[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
    const int x = i0[0] + dx, y = i0[1] + dy, z = i0[2] + dz;
    if (!corner_ok(g, x, y, z)) continue;
    const float wx = dx ? w1[0] : w0[0], wy = dy ? w1[1] : w0[1], wz = dz ? w1[2] : w0[2];
    const long long node = node_index(g, x, y, z);
    if (want_col) {
      const float w = (wx * wy) * wz;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float f = g.split ? g.dens[node * g.dstride + 1 + ch] : g.feat[node * g.fstride + ch * g.K];
        c[ch] = c[ch] + f * w;
      }
    }
    if (want_nrm) {
      const float v = pre_density(g, node);
      gr[0] = gr[0] + (dx ? v : -v) * (wy * wz);
      gr[1] = gr[1] + (dy ? v : -v) * (wx * wz);
      gr[2] = gr[2] + (dz ? v : -v) * (wx * wy);
    }
  }
  if (want_col)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) col[ch] = 1.0f / (1.0f + expf(-(kC0 * c[ch])));
  if (want_nrm) {
    const int dims[3] = {g.X, g.Y, g.Z};
    float n2 = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      gr[a] = gr[a] * ((float)dims[a] * 0.5f * g.nscale[a]);  // d idx / d p
      n2 += gr[a] * gr[a];
    }
    const float inv = n2 > 0.0f ? -1.0f / sqrtf(n2) : 0.0f;
    for (int a = 0; a < 3; ++a) nrm[a] = gr[a] * inv;
  }
}

__global__ __launch_bounds__(kMeshBlock) void mesh_emit_kernel(MeshArgs g, EmitOut o) {
  __shared__ float s[4][kRun];
  for (long long blk = blockIdx.x; blk < g.nblocks; blk += gridDim.x) {
    const long long L0 = blk * kMeshBlock;
    stage_sigma(g, L0, s);
    const PointWork w = point_work(g, L0, s);
    int pv, pf, tv, tf;
    block_prefix(__popc(w.vmask), w.nfaces, &pv, &pf, &tv, &tf);
    const int t = threadIdx.x;
    const long long lin = L0 + t;
    long long vslot = o.offsets[blk] + pv, fslot = o.offsets[g.nblocks + blk] + pf;
    // vertices: ascending direction code = ascending edge key
    for (int code = 1; code < 8; ++code) {
      if (!((w.vmask >> (code - 1)) & 1)) continue;
      const int d[3] = {code >> 2, (code >> 1) & 1, code & 1};
      if (vslot < o.vcap) {
        const float sa = sigma_at(s, t, 0, 0, 0), sb = sigma_at(s, t, d[0], d[1], d[2]);
        const float tt = (g.tau - sa) / (sb - sa);
        float p[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const float pa = lattice_coord(g, a, w.u[a]);
          const float diff = d[a] ? lattice_coord(g, a, w.u[a] + 1) - pa : 0.0f;
          p[a] = pa + tt * diff;
          o.pos[vslot * 3 + a] = p[a];
        }
        o.keys[vslot] = 7 * lin + (code - 1);
        if (o.col || o.nrm) {
          float c[3], n[3];
          vertex_attributes(g, p, o.col != nullptr, o.nrm != nullptr, c, n);
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            if (o.col) o.col[vslot * 3 + a] = c[a];
            if (o.nrm) o.nrm[vslot * 3 + a] = n[a];
          }
        }
      }
      ++vslot;
    }
    // triangles of the cube at this point, in (tet, triangle) order
    if (w.nfaces) {
      for (int tet = 0; tet < 6; ++tet) {
        int tin = 0;
        for (int k = 0; k < 4; ++k) tin |= ((w.ncube >> tet_vertex(tet, k)) & 1) << k;
        const int cc = tet_case(tet, tin);
        for (int f = 0; f < (cc & 15); ++f) {
          if (fslot < o.fcap) {
            for (int v = 0; v < 3; ++v) {
              const int nib = (cc >> (4 + 12 * f + 4 * v)) & 15;
              // tet-local k < l: the corner code of v_l covers that of v_k, and the edge's lower end is v_k
              const int cl = tet_vertex(tet, nib & 3), dcode = tet_vertex(tet, nib >> 2) & ~cl;
              const long long a = lin + (long long)(cl >> 2) * g.RyRz + (long long)((cl >> 1) & 1) * g.R[2] + (cl & 1);
              o.fedge[fslot * 3 + v] = 7 * a + (dcode - 1);
            }
          }
          ++fslot;
        }
      }
    }
    __syncthreads();  // (LDS reused by the next block of the loop)
  }
}

int mesh_args(const RFGrid* grid, int32_t subdivisions, float iso_level, MeshArgs* a) {
  if (!grid || !grid->densities_dev) return RF_ERR_NULL_POINTER;
  const int F = grid->num_features;
  if (!(F == 3 || F == 12 || F == 27 || F == 48)) return RF_ERR_UNSUPPORTED;
  if (grid->density_mode < RF_DENSITY_RELU || grid->density_mode > RF_DENSITY_IDENTITY) return RF_ERR_UNSUPPORTED;
  if (grid->layout == RF_LAYOUT_REFERENCE) {
    if (!grid->features_dev) return RF_ERR_NULL_POINTER;
    if (grid->density_stride < 1 || grid->feature_stride < F) return RF_ERR_BAD_SHAPE;
  } else if (grid->layout == RF_LAYOUT_SPLIT || grid->layout == RF_LAYOUT_BRICKED) {
    if (grid->density_stride < 4) return RF_ERR_BAD_SHAPE;
  } else {
    return RF_ERR_UNSUPPORTED;
  }
  if (subdivisions < 1 || subdivisions > 8) return RF_ERR_BAD_SHAPE;
  if (!(iso_level == iso_level) || iso_level > 3.4e38f || iso_level < -3.4e38f) return RF_ERR_BAD_SHAPE;  // finite
  for (int i = 0; i < 3; ++i)
    if (grid->dims[i] < 1 || grid->dims[i] > 2046) return RF_ERR_BAD_SHAPE;
  a->dens = grid->densities_dev;
  a->feat = grid->features_dev;
  a->X = grid->dims[0];
  a->Y = grid->dims[1];
  a->Z = grid->dims[2];
  a->K = F / 3;
  a->dstride = grid->density_stride;
  a->fstride = grid->feature_stride;
  a->split = grid->layout != RF_LAYOUT_REFERENCE;
  a->bricked = grid->layout == RF_LAYOUT_BRICKED;
  a->nby = (a->Y + 7) / 8;
  a->nbz = (a->Z + 7) / 8;
  for (int i = 0; i < 3; ++i) {
    a->amin[i] = grid->aabb_min[i];
    a->amax[i] = grid->aabb_max[i];
    a->ext[i] = grid->aabb_max[i] - grid->aabb_min[i];
    a->nscale[i] = grid->norm_scale[i];
    a->nbias[i] = grid->norm_bias[i];
    a->R[i] = subdivisions * grid->dims[i] + 2;
  }
  a->rho = grid->density_scale;
  a->mode = grid->density_mode;
  a->tau = iso_level;
  a->m = subdivisions;
  a->RyRz = (long long)a->R[1] * a->R[2];
  a->total = (long long)a->R[0] * a->RyRz;
  a->nblocks = (a->total + kMeshBlock - 1) / kMeshBlock;
  return RF_OK;
}

unsigned int mesh_grid(long long nblocks) { return (unsigned int)(nblocks < (1ll << 20) ? nblocks : (1ll << 20)); }

}  // namespace

extern "C" {

int64_t rf_mesh_tiles(const RFGrid* grid, int32_t subdivisions) {
  MeshArgs a;
  const int rc = mesh_args(grid, subdivisions, 0.0f, &a);
  return rc != RF_OK ? rc : a.nblocks;
}

int rf_mesh_count(const RFGrid* grid, int32_t subdivisions, float iso_level, int64_t* counts_dev, void* stream) {
  MeshArgs a;
  const int rc = mesh_args(grid, subdivisions, iso_level, &a);
  if (rc != RF_OK) return rc;
  if (!counts_dev) return RF_ERR_NULL_POINTER;
  hipLaunchKernelGGL(mesh_count_kernel, dim3(mesh_grid(a.nblocks)), dim3(kMeshBlock), 0, (hipStream_t)stream, a,
                     reinterpret_cast<long long*>(counts_dev));
  return launch_status();
}

int rf_mesh_emit(const RFGrid* grid, int32_t subdivisions, float iso_level, const int64_t* offsets_dev, int64_t num_vertices,
                 int64_t num_faces, int64_t* edge_keys_dev, float* positions_dev, float* colours_dev, float* normals_dev,
                 int64_t* face_edges_dev, void* stream) {
  MeshArgs a;
  const int rc = mesh_args(grid, subdivisions, iso_level, &a);
  if (rc != RF_OK) return rc;
  if (num_vertices < 0 || num_faces < 0) return RF_ERR_BAD_SHAPE;
  if (!offsets_dev || (num_vertices && (!edge_keys_dev || !positions_dev)) || (num_faces && !face_edges_dev)) return RF_ERR_NULL_POINTER;
  EmitOut o;
  o.offsets = reinterpret_cast<const long long*>(offsets_dev);
  o.vcap = num_vertices;
  o.fcap = num_faces;
  o.keys = reinterpret_cast<long long*>(edge_keys_dev);
  o.pos = positions_dev;
  o.col = colours_dev;
  o.nrm = normals_dev;
  o.fedge = reinterpret_cast<long long*>(face_edges_dev);
  hipLaunchKernelGGL(mesh_emit_kernel, dim3(mesh_grid(a.nblocks)), dim3(kMeshBlock), 0, (hipStream_t)stream, a, o);
  return launch_status();
}

}  // extern "C"
