// mesh_simplify_kernels.hip -- mesh simplification by vertex clustering with quadric-error representatives (rf_mesh_cluster_keys /
// rf_mesh_cluster_vertices of relu_field.h): what thr3ed_atom_amd/mesh_simplify.py is built on.  DESIGN.md section 20 has the
// contract, docs/mesh_simplify_errors.md the error bound, tests/mesh_simplify_model.py the float64 model.
//
// rf_mesh_cluster_keys.  One thread per vertex: k_a = floor(fl32(fl32(v_a - o_a) * r)) per axis (the unit is built without
// contraction, so that is two rounded float32 operations), key = (k_x n_y + k_y) n_z + k_z.  A vertex whose k_a is not in [0, n_a)
// on some axis -- below the origin, beyond the cells, NaN or infinite -- gets the key -1 and stores 1 to the status word (a plain
// store of one value: whichever thread wins, the word reads 1).
//
// rf_mesh_cluster_vertices.  Gather form, no atomics.  A GROUP of 16 lanes owns a cluster (four clusters per wave, sixteen per
// workgroup of 256 threads).  Lane l of the group takes the records l, l + 16, l + 32 ... of the cluster's corner segment and then
// of its member segment, adds them in that order to its own float64 accumulators, and the sixteen partial sums meet in an xor
// butterfly (offsets 8, 4, 2, 1: both partners of an exchange compute a + b from the same two values, so every lane ends with
// the same bits).  A cluster with kLongSegment records or more is left out by its group and taken by the WHOLE wave afterwards
// (stride 64, butterfly from 32 down): one cell that holds a whole object does not keep sixteen lanes busy while 48 idle.  Which
// path a cluster takes and the order of every sum depend on the segment lengths alone -- two runs give the same bits.
//   corner record 3 f + j of cluster c: the three vertices of face f relative to the centre m of c's cell, q_i = p_i - m in float64,
//     n = (q1 - q0) x (q2 - q0), d = n . q0;  A += n n^T (six terms), b += d n.  (Recomputed for every corner: no per-face
//     intermediates in memory, no scatter.)
//   member record v: the sum of q_v, of the colours and of the normals.
// Lane 0 of the group then places the representative: the mean xbar, or xbar + (A + lambda tr(A) I)^-1 (b - A xbar) by the
// adjugate over the determinant, clamped per axis to [-h/2, h/2], and writes float32(m + x), the mean colour and the normalised
// normal sum.  Every index read from a list is checked against its array before it is used (a bad list gives a wrong number,
// never an access outside the arrays).
#include "rf_device.h"

namespace {

constexpr int kKeysBlock = 256;
constexpr int kClusterGroup = 16;                                  // lanes per cluster
constexpr int kClusterBlock = 256;                                 // threads per workgroup of cluster_vertices_kernel
constexpr int kClustersPerBlock = kClusterBlock / kClusterGroup;   // 16 (thr3ed_atom_amd/_lib.py MESH_CLUSTERS_PER_BLOCK mirrors it)
constexpr int kGroupsPerWave = kWave / kClusterGroup;              // 4
constexpr long long kLongSegment = 256;                            // corner + member records from which the whole wave takes a cluster (measured: DESIGN.md section 20)
constexpr int kMaxCells = 1 << 20;
constexpr int kSums = 18;  // A (6: xx xy xz yy yz zz), b (3), position (3), colour (3), normal (3)

struct ClusterArgs {
  const float* vertices;
  const float* colours;  // or nullptr
  const float* normals;  // or nullptr
  const long long* faces;
  const long long* members;
  const long long* member_begin;
  const long long* corners;
  const long long* corner_begin;
  const long long* keys;
  float* vertices_out;
  float* colours_out;
  float* normals_out;
  long long num_vertices, num_faces, num_clusters;
  float origin[3];
  float h;
  int cells[3];
  int placement;
  float lambda;
};

__global__ __launch_bounds__(kKeysBlock) void cluster_keys_kernel(const float* __restrict__ vertices, long long num_vertices, float ox, float oy,
                                                                   float oz, float r, int nx, int ny, int nz, long long* __restrict__ keys,
                                                                   int* __restrict__ status) {
  const long long v = (long long)blockIdx.x * kKeysBlock + threadIdx.x;
  if (v >= num_vertices) return;
  const float tx = (vertices[3 * v] - ox) * r, ty = (vertices[3 * v + 1] - oy) * r, tz = (vertices[3 * v + 2] - oz) * r;
  const float kx = floorf(tx), ky = floorf(ty), kz = floorf(tz);
  // (NaN fails every comparison; n_a <= 2^20 is exact in float32)
  const bool inside = kx >= 0.0f && kx < (float)nx && ky >= 0.0f && ky < (float)ny && kz >= 0.0f && kz < (float)nz;
  long long key = -1;
  if (inside) key = ((long long)kx * ny + (long long)ky) * nz + (long long)kz;
  else *status = 1;
  keys[v] = key;
}

struct Centre {
  double x, y, z;
};

__device__ __forceinline__ Centre cell_centre(const ClusterArgs& a, long long key) {
  const long long kz = key % a.cells[2], rest = key / a.cells[2];
  const long long ky = rest % a.cells[1], kx = rest / a.cells[1];
  const double h = (double)a.h;
  return {(double)a.origin[0] + ((double)kx + 0.5) * h, (double)a.origin[1] + ((double)ky + 0.5) * h, (double)a.origin[2] + ((double)kz + 0.5) * h};
}

// lane `lane` of `W` lanes adds its share of cluster c's two segments to s
template <int W>
__device__ __forceinline__ void cluster_accumulate(const ClusterArgs& a, long long c, int lane, const Centre& m, double (&s)[kSums]) {
  const unsigned long long V = (unsigned long long)a.num_vertices, corners_total = 3ull * (unsigned long long)a.num_faces;
  const long long cb = max(a.corner_begin[c], 0ll), ce = min(a.corner_begin[c + 1], (long long)corners_total);
  for (long long i = cb + lane; i < ce; i += W) {
    const unsigned long long corner = (unsigned long long)a.corners[i];
    if (corner >= corners_total) continue;
    const long long* face = a.faces + corner / 3 * 3;
    const unsigned long long i0 = (unsigned long long)face[0], i1 = (unsigned long long)face[1], i2 = (unsigned long long)face[2];
    if (i0 >= V || i1 >= V || i2 >= V) continue;
    const float *p0 = a.vertices + 3 * i0, *p1 = a.vertices + 3 * i1, *p2 = a.vertices + 3 * i2;
    const double q0x = (double)p0[0] - m.x, q0y = (double)p0[1] - m.y, q0z = (double)p0[2] - m.z;
    const double ux = ((double)p1[0] - m.x) - q0x, uy = ((double)p1[1] - m.y) - q0y, uz = ((double)p1[2] - m.z) - q0z;
    const double wx = ((double)p2[0] - m.x) - q0x, wy = ((double)p2[1] - m.y) - q0y, wz = ((double)p2[2] - m.z) - q0z;
    const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    const double d = nx * q0x + ny * q0y + nz * q0z;
    s[0] += nx * nx, s[1] += nx * ny, s[2] += nx * nz, s[3] += ny * ny, s[4] += ny * nz, s[5] += nz * nz;
    s[6] += d * nx, s[7] += d * ny, s[8] += d * nz;
  }
  const long long mb = max(a.member_begin[c], 0ll), me = min(a.member_begin[c + 1], a.num_vertices);
  for (long long i = mb + lane; i < me; i += W) {
    const unsigned long long v = (unsigned long long)a.members[i];
    if (v >= V) continue;
    const float* p = a.vertices + 3 * v;
    s[9] += (double)p[0] - m.x, s[10] += (double)p[1] - m.y, s[11] += (double)p[2] - m.z;
    if (a.colours) s[12] += (double)a.colours[3 * v], s[13] += (double)a.colours[3 * v + 1], s[14] += (double)a.colours[3 * v + 2];
    if (a.normals) s[15] += (double)a.normals[3 * v], s[16] += (double)a.normals[3 * v + 1], s[17] += (double)a.normals[3 * v + 2];
  }
}

// xor butterfly over W consecutive lanes (W = 16: the group, W = 64: the wave); every lane ends with the same bits
template <int W>
__device__ __forceinline__ void cluster_reduce(double (&s)[kSums]) {
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1)
#pragma unroll
    for (int k = 0; k < kSums; ++k) s[k] += __shfl_xor(s[k], off, kWave);
}

__device__ __forceinline__ double clamp_to(double x, double half) { return x < -half ? -half : (x > half ? half : x); }

__device__ __forceinline__ void cluster_place(const ClusterArgs& a, long long c, const Centre& m, const double (&s)[kSums]) {
  const double count = (double)(a.member_begin[c + 1] - a.member_begin[c]);  // >= 1: a cluster is a key that some vertex has
  const double mx = s[9] / count, my = s[10] / count, mz = s[11] / count;
  double x = mx, y = my, z = mz;
  const double axx = s[0], axy = s[1], axz = s[2], ayy = s[3], ayz = s[4], azz = s[5];
  const double tr = axx + ayy + azz;
  if (a.placement == 0 && tr != 0.0) {
    const double reg = (double)a.lambda * tr;
    const double pxx = axx + reg, pyy = ayy + reg, pzz = azz + reg;
    const double rx = s[6] - (axx * mx + axy * my + axz * mz), ry = s[7] - (axy * mx + ayy * my + ayz * mz), rz = s[8] - (axz * mx + ayz * my + azz * mz);
    // adjugate of the symmetric M = [pxx axy axz; axy pyy ayz; axz ayz pzz]
    const double cxx = pyy * pzz - ayz * ayz, cxy = axz * ayz - axy * pzz, cxz = axy * ayz - axz * pyy;
    const double cyy = pxx * pzz - axz * axz, cyz = axy * axz - pxx * ayz, czz = pxx * pyy - axy * axy;
    const double det = pxx * cxx + axy * cxy + axz * cxz;
    x = mx + (cxx * rx + cxy * ry + cxz * rz) / det;
    y = my + (cxy * rx + cyy * ry + cyz * rz) / det;
    z = mz + (cxz * rx + cyz * ry + czz * rz) / det;
    const double half = 0.5 * (double)a.h;
    x = clamp_to(x, half), y = clamp_to(y, half), z = clamp_to(z, half);
  }
  a.vertices_out[3 * c] = (float)(m.x + x), a.vertices_out[3 * c + 1] = (float)(m.y + y), a.vertices_out[3 * c + 2] = (float)(m.z + z);
  if (a.colours) a.colours_out[3 * c] = (float)(s[12] / count), a.colours_out[3 * c + 1] = (float)(s[13] / count), a.colours_out[3 * c + 2] = (float)(s[14] / count);
  if (a.normals) {
    const double len = sqrt(s[15] * s[15] + s[16] * s[16] + s[17] * s[17]);
    const bool zero = len == 0.0;
    a.normals_out[3 * c] = zero ? 0.0f : (float)(s[15] / len), a.normals_out[3 * c + 1] = zero ? 0.0f : (float)(s[16] / len), a.normals_out[3 * c + 2] = zero ? 0.0f : (float)(s[17] / len);
  }
}

__device__ __forceinline__ long long cluster_records(const ClusterArgs& a, long long c) {
  return (a.corner_begin[c + 1] - a.corner_begin[c]) + (a.member_begin[c + 1] - a.member_begin[c]);
}

__global__ __launch_bounds__(kClusterBlock) void cluster_vertices_kernel(ClusterArgs a) {
  const int lane = threadIdx.x & (kWave - 1), sub = lane & (kClusterGroup - 1), group = lane / kClusterGroup;
  const long long first = ((long long)blockIdx.x * (kClusterBlock / kWave) + threadIdx.x / kWave) * kGroupsPerWave;  // the wave's first cluster
  if (first >= a.num_clusters) return;  // (wave-uniform)
  const long long c = first + group;
  const bool mine = c < a.num_clusters;
  double s[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) s[k] = 0.0;
  Centre m = {0.0, 0.0, 0.0};
  bool is_long = false;
  if (mine) {
    m = cell_centre(a, a.keys[c]);
    is_long = cluster_records(a, c) >= kLongSegment;
    if (!is_long) cluster_accumulate<kClusterGroup>(a, c, sub, m, s);
  }
  cluster_reduce<kClusterGroup>(s);  // (every lane of the wave takes part: lanes without a cluster carry zeros)
  const unsigned long long long_lanes = __ballot(is_long);
#pragma unroll
  for (int g = 0; g < kGroupsPerWave; ++g) {
    if (!((long_lanes >> (g * kClusterGroup)) & 1ull)) continue;  // (wave-uniform)
    const long long cg = first + g;
    const Centre mg = cell_centre(a, a.keys[cg]);
    double t[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) t[k] = 0.0;
    cluster_accumulate<kWave>(a, cg, lane, mg, t);
    cluster_reduce<kWave>(t);
    if (group == g) {
#pragma unroll
      for (int k = 0; k < kSums; ++k) s[k] = t[k];
    }
  }
  if (mine && sub == 0) cluster_place(a, c, m, s);
}

bool positive_finite(float x) { return x > 0.0f && std::isfinite(x); }

bool cells_ok(const int32_t* cells) {
  for (int a = 0; a < 3; ++a)
    if (cells[a] < 1 || cells[a] > kMaxCells) return false;
  return true;
}

}  // namespace

extern "C" {

int rf_mesh_cluster_keys(const float* vertices_dev, int64_t num_vertices, const float* origin, float r, const int32_t* cells, int64_t* keys_dev,
                         int32_t* status_dev, void* stream) {
  if (!vertices_dev || !origin || !cells || !keys_dev || !status_dev) return RF_ERR_NULL_POINTER;
  if (num_vertices < 0 || num_vertices >= (1ll << 31)) return RF_ERR_BAD_SHAPE;
  if (!positive_finite(r)) return RF_ERR_BAD_SHAPE;
  if (!std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2])) return RF_ERR_BAD_SHAPE;
  if (!cells_ok(cells)) return RF_ERR_BAD_SHAPE;
  if (num_vertices == 0) return RF_OK;
  hipLaunchKernelGGL(cluster_keys_kernel, dim3((unsigned)((num_vertices + kKeysBlock - 1) / kKeysBlock)), dim3(kKeysBlock), 0, (hipStream_t)stream,
                     vertices_dev, (long long)num_vertices, origin[0], origin[1], origin[2], r, cells[0], cells[1], cells[2], (long long*)keys_dev, status_dev);
  return launch_status();
}

int rf_mesh_cluster_vertices(const float* vertices_dev, const float* colours_dev, const float* normals_dev, int64_t num_vertices,
                             const int64_t* faces_dev, int64_t num_faces, const int64_t* members_dev, const int64_t* member_begin_dev,
                             const int64_t* corners_dev, const int64_t* corner_begin_dev, const int64_t* cluster_keys_dev, int64_t num_clusters,
                             const float* origin, float h, const int32_t* cells, int32_t placement, float regularisation,
                             float* vertices_out_dev, float* colours_out_dev, float* normals_out_dev, void* stream) {
  if (!vertices_dev || !faces_dev || !members_dev || !member_begin_dev || !corners_dev || !corner_begin_dev || !cluster_keys_dev || !origin || !cells ||
      !vertices_out_dev)
    return RF_ERR_NULL_POINTER;
  if ((colours_dev == nullptr) != (colours_out_dev == nullptr) || (normals_dev == nullptr) != (normals_out_dev == nullptr)) return RF_ERR_NULL_POINTER;
  if (num_vertices < 0 || num_faces < 0 || num_clusters < 0) return RF_ERR_BAD_SHAPE;
  if (num_vertices >= (1ll << 31) || num_clusters > num_vertices || num_faces >= (1ll << 40)) return RF_ERR_BAD_SHAPE;
  if (!positive_finite(h) || !positive_finite(1.0f / h)) return RF_ERR_BAD_SHAPE;
  if (!std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2])) return RF_ERR_BAD_SHAPE;
  if (!cells_ok(cells)) return RF_ERR_BAD_SHAPE;
  if (placement != RF_MESH_PLACEMENT_QUADRIC && placement != RF_MESH_PLACEMENT_MEAN) return RF_ERR_BAD_SHAPE;
  if (!(regularisation >= 1e-6f && regularisation <= 1.0f)) return RF_ERR_BAD_SHAPE;
  if (num_clusters == 0 || num_vertices == 0) return RF_OK;
  ClusterArgs a;
  a.vertices = vertices_dev, a.colours = colours_dev, a.normals = normals_dev;
  a.faces = (const long long*)faces_dev, a.members = (const long long*)members_dev, a.member_begin = (const long long*)member_begin_dev;
  a.corners = (const long long*)corners_dev, a.corner_begin = (const long long*)corner_begin_dev, a.keys = (const long long*)cluster_keys_dev;
  a.vertices_out = vertices_out_dev, a.colours_out = colours_out_dev, a.normals_out = normals_out_dev;
  a.num_vertices = num_vertices, a.num_faces = num_faces, a.num_clusters = num_clusters;
  for (int i = 0; i < 3; ++i) a.origin[i] = origin[i], a.cells[i] = cells[i];
  a.h = h, a.placement = placement, a.lambda = regularisation;
  hipLaunchKernelGGL(cluster_vertices_kernel, dim3((unsigned)((num_clusters + kClustersPerBlock - 1) / kClustersPerBlock)), dim3(kClusterBlock), 0,
                     (hipStream_t)stream, a);
  return launch_status();
}

}  // extern "C"
