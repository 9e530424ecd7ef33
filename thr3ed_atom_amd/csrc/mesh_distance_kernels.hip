// mesh_distance_kernels.hip -- the closest point on a triangle mesh for many query points (rf_mesh_grid_pairs /
// rf_mesh_closest_points of relu_field.h): what thr3ed_atom_amd/mesh_distance.py is built on.  DESIGN.md section 27 has the contract
// and the measurements, docs/mesh_distance_errors.md the rule, the error bound and the proof of the stop test,
// tests/mesh_distance_model.py the numpy model.
//
// The search structure is a lattice of n_x n_y n_z cubic cells of edge h from `origin` (the mesh's per-axis minimum); the cell of a
// coordinate is floor(fl32(fl32(v - o) r)), r = fl32(1 / h), clamped into the lattice (dist_cell of mesh_distance.h).  A face is
// registered in every cell of the cell range of its axis-aligned box.
//
// rf_mesh_grid_pairs.  One lane per face writes the (cell key, face) pairs of its box, x-major, from offsets[f] on; the caller
// computed the counts, and a face whose own count disagrees with offsets[f + 1] - offsets[f] writes nothing and raises status 2
// (never a store outside the arrays).  A face of more than kWideFace cells is left out by its lane and taken by the whole wavefront
// afterwards, 64 pairs per step.  No atomics: where a pair lands is a function of the input alone.
//
// rf_mesh_closest_points.  One lane per query for the first kLaneRings shells; a query still walking then is handed to the whole
// wavefront by ballot -- 64 lanes over the columns of each further shell, a butterfly minimum of the (d2 bits, face) pair, the lower
// face on ties: the same minimum, the same bits.  The query starts in the (clamped) cell of its position and visits the shells of
// growing Chebyshev radius R around it; every registered face goes through closest_on_face, the smallest d2 wins and the lowest
// face index on an exact tie, so a face met twice changes nothing.  After the shell R it stops when
//   * the cube [c - R, c + R] covers the lattice, or
//   * best d2 < bound2, where bound2 is the square of the smallest of the gaps from p to the (up to six) faces of the cube that lie
//     strictly inside the lattice, each plane moved towards p by the rounding of the cell assignment (plane_below / plane_above:
//     no float32 coordinate of a cell beyond the plane lies on p's side of it).  A face never seen has its whole box beyond one of
//     those planes, every candidate point of closest_on_face is clamped into that box, and rounding is monotone: its float32 d2 is
//     >= bound2 > best, so it cannot win and cannot tie.  Or
//   * bound2 exceeds max_distance^2 by more than rounding: nothing within max_distance is left.
// The result is therefore the minimum over ALL faces whatever the lattice: distance, face and point do not depend on h, bit for bit.
// The winner's point is recomputed from its face at the end (the same function, the same bits) instead of being carried along.
// Every index read from a list is checked against its array before it is used.
#include "mesh_distance.h"

namespace {

constexpr int kMaxGridCells = 1024;  // cells per axis (thr3ed_atom_amd/_lib.py MESH_DISTANCE_MAX_CELLS mirrors it)
constexpr int kWideFace = 64;        // cells of a face's box above which the wavefront writes its pairs (MESH_DISTANCE_WIDE_FACE)
constexpr int kLaneRings = 2;        // shells a lane walks alone before the wavefront takes its query (MESH_DISTANCE_LANE_RINGS; measured: DESIGN.md section 27)
constexpr int kDistBlock = 256;
constexpr long long kMaxTable = 1ll << 25;  // cells of the lattice (the dense cell_begin table)

struct Lattice {
  float o[3];
  float h, r;
  int n[3];
};

struct PairArgs {
  const float* vertices;
  const long long* faces;
  const long long* offsets;
  long long* keys;
  int* pair_faces;
  int* status;
  long long num_vertices, num_faces, num_pairs;
  Lattice g;
};

struct FaceCells {
  int lo[3], hi[3];
  long long begin, count;  // count 0: nothing to write
};

__device__ __forceinline__ FaceCells face_cells(const PairArgs& a, long long f) {
  FaceCells c = {{0, 0, 0}, {0, 0, 0}, 0, 0};
  const unsigned long long V = (unsigned long long)a.num_vertices;
  const unsigned long long i0 = (unsigned long long)a.faces[3 * f], i1 = (unsigned long long)a.faces[3 * f + 1], i2 = (unsigned long long)a.faces[3 * f + 2];
  if (i0 >= V || i1 >= V || i2 >= V) {
    *a.status = 1;
    return c;
  }
  const float *p0 = a.vertices + 3 * i0, *p1 = a.vertices + 3 * i1, *p2 = a.vertices + 3 * i2;
  long long count = 1;
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float lo = fminf(fminf(p0[k], p1[k]), p2[k]), hi = fmaxf(fmaxf(p0[k], p1[k]), p2[k]);
    finite = finite && isfinite(p0[k]) && isfinite(p1[k]) && isfinite(p2[k]);
    c.lo[k] = dist_cell(lo, a.g.o[k], a.g.r, a.g.n[k]), c.hi[k] = dist_cell(hi, a.g.o[k], a.g.r, a.g.n[k]);
    count *= (long long)(c.hi[k] - c.lo[k] + 1);
  }
  if (!finite) {
    *a.status = 1;
    return c;
  }
  const long long begin = a.offsets[f], end = a.offsets[f + 1];
  if (begin < 0 || end > a.num_pairs || end - begin != count) {
    *a.status = 2;
    return c;
  }
  c.begin = begin, c.count = count;
  return c;
}

// pair j of a face's box, x-major
__device__ __forceinline__ void write_pair(const PairArgs& a, const int (&lo)[3], const int (&hi)[3], long long begin, long long j, long long f) {
  const int sy = hi[1] - lo[1] + 1, sz = hi[2] - lo[2] + 1;
  const long long kz = lo[2] + j % sz, rest = j / sz;
  const long long ky = lo[1] + rest % sy, kx = lo[0] + rest / sy;
  a.keys[begin + j] = (kx * a.g.n[1] + ky) * a.g.n[2] + kz;
  a.pair_faces[begin + j] = (int)f;
}

__global__ __launch_bounds__(kDistBlock) void grid_pairs_kernel(PairArgs a) {
  const long long f = (long long)blockIdx.x * kDistBlock + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1);
  FaceCells c = {{0, 0, 0}, {0, 0, 0}, 0, 0};
  if (f < a.num_faces) c = face_cells(a, f);
  const bool is_wide = c.count > kWideFace;
  if (!is_wide)
    for (long long j = 0; j < c.count; ++j) write_pair(a, c.lo, c.hi, c.begin, j, f);
  unsigned long long wide_lanes = __ballot(is_wide);
  while (wide_lanes) {  // (wave-uniform)
    const int src = __ffsll((long long)wide_lanes) - 1;
    wide_lanes &= wide_lanes - 1;
    int lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) lo[k] = __shfl(c.lo[k], src, kWave), hi[k] = __shfl(c.hi[k], src, kWave);
    const long long begin = __shfl(c.begin, src, kWave), count = __shfl(c.count, src, kWave);
    const long long face = f - lane + src;
    for (long long j = lane; j < count; j += kWave) write_pair(a, lo, hi, begin, j, face);
  }
}

struct ClosestArgs {
  const float* vertices;
  const long long* faces;
  const int* cell_begin;
  const int* cell_faces;
  const float* points;
  const long long* order;  // or nullptr
  float* distance;
  long long* face;
  float* point;
  int* rings;  // or nullptr
  int* status;
  long long num_vertices, num_faces, num_pairs, num_points;
  float max_distance;
  Lattice g;
};

// a float32 that is <= every float32 coordinate whose cell index along the axis is >= K (K >= 1): such a coordinate is
// >= o + K h (1 - 3 u) in exact arithmetic (docs/mesh_distance_errors.md), the two corrections cover the roundings made here
__device__ __forceinline__ float plane_below(float o, float h, int K) {
  const float x = o + ((float)K * h) * (1.0f - 0x1p-21f);
  return x - fabsf(x) * 0x1p-22f;
}

// a float32 that is >= every float32 coordinate whose cell index along the axis is < K
__device__ __forceinline__ float plane_above(float o, float h, int K) {
  const float x = o + ((float)K * h) * (1.0f + 0x1p-21f);
  return x + fabsf(x) * 0x1p-22f;
}

struct Best {
  float d2;
  int face;
};

__device__ __forceinline__ FaceClosest face_distance(const ClosestArgs& a, int f, float px, float py, float pz, bool& ok) {
  const unsigned long long V = (unsigned long long)a.num_vertices;
  const long long* idx = a.faces + 3ll * f;
  const unsigned long long i0 = (unsigned long long)idx[0], i1 = (unsigned long long)idx[1], i2 = (unsigned long long)idx[2];
  ok = i0 < V && i1 < V && i2 < V;
  if (!ok) return {0.0f, 0.0f, 0.0f, 0.0f};
  const float *p0 = a.vertices + 3 * i0, *p1 = a.vertices + 3 * i1, *p2 = a.vertices + 3 * i2;
  return closest_on_face(px, py, pz, p0[0], p0[1], p0[2], p1[0], p1[1], p1[2], p2[0], p2[1], p2[2]);
}

__device__ __forceinline__ void visit_cell(const ClosestArgs& a, long long cell, float px, float py, float pz, Best& best) {
  const int b = max(a.cell_begin[cell], 0), e = (int)min((long long)a.cell_begin[cell + 1], a.num_pairs);
  for (int j = b; j < e; ++j) {
    const int f = a.cell_faces[j];
    if ((unsigned)f >= (unsigned long long)a.num_faces) {
      *a.status = 2;
      continue;
    }
    bool ok;
    const FaceClosest c = face_distance(a, f, px, py, pz, ok);
    if (!ok) {
      *a.status = 1;
      continue;
    }
    if (c.d2 < best.d2 || (c.d2 == best.d2 && f < best.face)) best.d2 = c.d2, best.face = f;
  }
}

// after shell R: true when the walk is over (the cube covers the lattice, the best is proven minimal, or nothing within max_distance is left)
__device__ __forceinline__ bool walk_is_over(const ClosestArgs& a, float px, float py, float pz, int cx, int cy, int cz, int R, float best_d2, float limit2) {
  const float p[3] = {px, py, pz};
  const int c[3] = {cx, cy, cz};
  bool covers = true;
  float gap = __builtin_inff();  // the smallest gap to a face of the cube strictly inside the lattice; <= 0: no statement
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    covers = covers && c[k] - R <= 0 && c[k] + R >= a.g.n[k] - 1;
    if (c[k] + R + 1 <= a.g.n[k] - 1) gap = fminf(gap, plane_below(a.g.o[k], a.g.h, c[k] + R + 1) - p[k]);
    if (c[k] - R >= 1) gap = fminf(gap, p[k] - plane_above(a.g.o[k], a.g.h, c[k] - R));
  }
  const float bound2 = gap > 0.0f ? gap * gap : 0.0f;
  return covers || best_d2 < bound2 || bound2 > limit2;
}

__device__ __forceinline__ unsigned long long pack_best(const Best& b) { return ((unsigned long long)__float_as_uint(b.d2) << 32) | (unsigned)b.face; }  // (d2 >= 0: its bits order as it does)

__global__ __launch_bounds__(kDistBlock) void closest_points_kernel(ClosestArgs a) {
  const long long i = (long long)blockIdx.x * kDistBlock + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1);
  long long q = -1;
  if (i < a.num_points) {
    q = a.order ? a.order[i] : i;
    if ((unsigned long long)q >= (unsigned long long)a.num_points) *a.status = 2, q = -1;
  }
  float px = 0.0f, py = 0.0f, pz = 0.0f;
  if (q >= 0) px = a.points[3 * q], py = a.points[3 * q + 1], pz = a.points[3 * q + 2];
  const float nan = __builtin_nanf(""), inf = __builtin_inff();
  Best best = {inf, 0x7fffffff};
  int R = 0;
  const int nx = a.g.n[0], ny = a.g.n[1], nz = a.g.n[2];
  const float limit2 = (a.max_distance * a.max_distance) * (1.0f + 0x1p-21f);  // d2 above it: sqrtf(d2) > max_distance
  bool walking = q >= 0;
  if (walking && !(isfinite(px) && isfinite(py) && isfinite(pz))) *a.status = 1, walking = false;
  const int cx = dist_cell(px, a.g.o[0], a.g.r, nx), cy = dist_cell(py, a.g.o[1], a.g.r, ny), cz = dist_cell(pz, a.g.o[2], a.g.r, nz);
  // one lane per query for the first kLaneRings shells
  for (; walking && R < kLaneRings; ++R) {
    const int x0 = max(cx - R, 0), x1 = min(cx + R, nx - 1), y0 = max(cy - R, 0), y1 = min(cy + R, ny - 1), z0 = max(cz - R, 0), z1 = min(cz + R, nz - 1);
    for (int x = x0; x <= x1; ++x)
      for (int y = y0; y <= y1; ++y) {
        // a column on the shell's x or y faces is visited whole, an inner one at its two ends
        const bool whole = R == 0 || x == cx - R || x == cx + R || y == cy - R || y == cy + R;
        const int step = whole ? 1 : 2 * R;
        for (int z = whole ? z0 : (cz - R >= 0 ? cz - R : cz + R); z <= z1; z += step) visit_cell(a, ((long long)x * ny + y) * nz + z, px, py, pz, best);
      }
    if (walk_is_over(a, px, py, pz, cx, cy, cz, R, best.d2, limit2)) {
      walking = false;
      break;
    }
  }
  // queries still walking go to the whole wavefront, one after the other: 64 lanes over the columns of each shell
  unsigned long long pending = __ballot(walking);
  while (pending) {  // (wave-uniform)
    const int src = __ffsll((long long)pending) - 1;
    pending &= pending - 1;
    const float sx = __shfl(px, src, kWave), sy = __shfl(py, src, kWave), sz = __shfl(pz, src, kWave);
    const int scx = __shfl(cx, src, kWave), scy = __shfl(cy, src, kWave), scz = __shfl(cz, src, kWave);
    int sR = __shfl(R, src, kWave);
    unsigned long long key = pack_best({__shfl(best.d2, src, kWave), __shfl(best.face, src, kWave)});
    for (;; ++sR) {
      const int x0 = max(scx - sR, 0), y0 = max(scy - sR, 0), z0 = max(scz - sR, 0), z1 = min(scz + sR, nz - 1);
      const int dx = min(scx + sR, nx - 1) - x0 + 1, dy = min(scy + sR, ny - 1) - y0 + 1;
      Best mine = {inf, 0x7fffffff};
      for (int j = lane; j < dx * dy; j += kWave) {  // the shell's columns over the lanes (sR >= kLaneRings >= 1; dx dy <= 2^20)
        const int x = x0 + j / dy, y = y0 + j % dy;
        const bool whole = x == scx - sR || x == scx + sR || y == scy - sR || y == scy + sR;
        const int step = whole ? 1 : 2 * sR;
        for (int z = whole ? z0 : (scz - sR >= 0 ? scz - sR : scz + sR); z <= z1; z += step) visit_cell(a, ((long long)x * ny + y) * nz + z, sx, sy, sz, mine);
      }
      unsigned long long m = pack_best(mine);
#pragma unroll
      for (int off = kWave / 2; off > 0; off >>= 1) m = min(m, __shfl_xor(m, off, kWave));
      key = min(key, m);  // the smaller d2, the lower face among equal ones
      if (walk_is_over(a, sx, sy, sz, scx, scy, scz, sR, __uint_as_float((unsigned)(key >> 32)), limit2)) break;
    }
    if (lane == src) best.d2 = __uint_as_float((unsigned)(key >> 32)), best.face = (int)(unsigned)key, R = sR;
  }
  if (q < 0) return;
  float d = inf, qx = nan, qy = nan, qz = nan;
  long long face = -1;
  if (best.face != 0x7fffffff && sqrtf(best.d2) <= a.max_distance) {
    bool ok;
    const FaceClosest w = face_distance(a, best.face, px, py, pz, ok);  // (ok: it was when the face won)
    d = sqrtf(best.d2), face = best.face, qx = w.x, qy = w.y, qz = w.z;
  }
  a.distance[q] = d, a.face[q] = face;
  a.point[3 * q] = qx, a.point[3 * q + 1] = qy, a.point[3 * q + 2] = qz;
  if (a.rings) a.rings[q] = R;
}

bool lattice_ok(const float* origin, float h, const int32_t* cells) {
  if (!(h > 0.0f) || !std::isfinite(h) || !(1.0f / h > 0.0f) || !std::isfinite(1.0f / h)) return false;
  long long table = 1;
  for (int k = 0; k < 3; ++k) {
    if (!std::isfinite(origin[k]) || cells[k] < 1 || cells[k] > kMaxGridCells) return false;
    table *= cells[k];
  }
  return table + 1 <= kMaxTable;
}

Lattice make_lattice(const float* origin, float h, const int32_t* cells) {
  Lattice g;
  for (int k = 0; k < 3; ++k) g.o[k] = origin[k], g.n[k] = cells[k];
  g.h = h, g.r = 1.0f / h;
  return g;
}

}  // namespace

extern "C" {

int rf_mesh_grid_pairs(const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces, const float* origin, float h,
                       const int32_t* cells, const int64_t* offsets_dev, int64_t num_pairs, int64_t* keys_dev, int32_t* pair_faces_dev, int32_t* status_dev,
                       void* stream) {
  if (!origin || !cells || !status_dev) return RF_ERR_NULL_POINTER;
  if (num_faces > 0 && (!vertices_dev || !faces_dev || !offsets_dev)) return RF_ERR_NULL_POINTER;
  if (num_pairs > 0 && (!keys_dev || !pair_faces_dev)) return RF_ERR_NULL_POINTER;
  if (num_vertices < 0 || num_faces < 0 || num_pairs < 0) return RF_ERR_BAD_SHAPE;
  if (num_vertices >= (1ll << 31) || num_faces >= (1ll << 31) || num_pairs >= (1ll << 31)) return RF_ERR_BAD_SHAPE;
  if (!lattice_ok(origin, h, cells)) return RF_ERR_BAD_SHAPE;
  if (num_faces == 0) return RF_OK;
  PairArgs a;
  a.vertices = vertices_dev, a.faces = (const long long*)faces_dev, a.offsets = (const long long*)offsets_dev;
  a.keys = (long long*)keys_dev, a.pair_faces = pair_faces_dev, a.status = status_dev;
  a.num_vertices = num_vertices, a.num_faces = num_faces, a.num_pairs = num_pairs;
  a.g = make_lattice(origin, h, cells);
  hipLaunchKernelGGL(grid_pairs_kernel, dim3((unsigned)((num_faces + kDistBlock - 1) / kDistBlock)), dim3(kDistBlock), 0, (hipStream_t)stream, a);
  return launch_status();
}

int rf_mesh_closest_points(const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces, const float* origin, float h,
                           const int32_t* cells, const int32_t* cell_begin_dev, const int32_t* cell_faces_dev, int64_t num_pairs, const float* points_dev,
                           const int64_t* order_dev, int64_t num_points, float max_distance, uint32_t flags, float* distance_dev, int64_t* face_dev,
                           float* point_dev, int32_t* rings_dev, int32_t* status_dev, void* stream) {
  if (!origin || !cells || !status_dev) return RF_ERR_NULL_POINTER;
  if (num_faces > 0 && (!vertices_dev || !faces_dev || !cell_begin_dev)) return RF_ERR_NULL_POINTER;
  if (num_pairs > 0 && !cell_faces_dev) return RF_ERR_NULL_POINTER;
  if (num_points > 0 && (!points_dev || !distance_dev || !face_dev || !point_dev)) return RF_ERR_NULL_POINTER;
  if (num_vertices < 0 || num_faces < 0 || num_pairs < 0 || num_points < 0) return RF_ERR_BAD_SHAPE;
  if (num_vertices >= (1ll << 31) || num_faces >= (1ll << 31) || num_pairs >= (1ll << 31) || num_points >= (1ll << 40)) return RF_ERR_BAD_SHAPE;
  if (!lattice_ok(origin, h, cells)) return RF_ERR_BAD_SHAPE;
  if (!(max_distance >= 0.0f)) return RF_ERR_BAD_SHAPE;  // (NaN fails; +inf: no limit)
  if (flags != 0) return RF_ERR_UNSUPPORTED;
  if (num_faces == 0 || num_points == 0) return RF_OK;
  ClosestArgs a;
  a.vertices = vertices_dev, a.faces = (const long long*)faces_dev, a.cell_begin = cell_begin_dev, a.cell_faces = cell_faces_dev;
  a.points = points_dev, a.order = (const long long*)order_dev;
  a.distance = distance_dev, a.face = (long long*)face_dev, a.point = point_dev, a.rings = rings_dev, a.status = status_dev;
  a.num_vertices = num_vertices, a.num_faces = num_faces, a.num_pairs = num_pairs, a.num_points = num_points;
  a.max_distance = max_distance;
  a.g = make_lattice(origin, h, cells);
  hipLaunchKernelGGL(closest_points_kernel, dim3((unsigned)((num_points + kDistBlock - 1) / kDistBlock)), dim3(kDistBlock), 0, (hipStream_t)stream, a);
  return launch_status();
}

}  // extern "C"
