// mesh_fit_kernels.hip -- the mesh render as a differentiable function of the VERTEX POSITIONS: an anti-aliased coverage image and a
// depth image (rf_mesh_raster_coverage) and their adjoint (rf_mesh_geometry_backward_pixels / rf_mesh_geometry_backward_gather of
// relu_field.h): what thr3ed_atom_amd/mesh_fit.py is built on.  DESIGN.md section 25 has the contract and the measurements,
// docs/mesh_fit_errors.md the error bound, tests/mesh_fit_model.py the float64 model.
//
// Every quantity of the rasteriser -- the pixel ray d, p_k = v_k - o, the edge values e_k, s, w_k, z -- comes from the device functions
// of mesh_raster.h (winning_key, load_face, raster_face, raster_edges, raster_hit), the ones the visibility and shade kernels call, so
// the depth image holds rf_mesh_raster_shade's bits.
//
// Coverage.  The edge-crossing rule of nvdiffrast (Laine et al. 2020) restricted to hit-against-miss pixel pairs.  For a hit pixel a
// with winning face F and a 4-neighbour b inside the image that nothing hit: sigma = sign(s(a)); over the k with sigma e_k(b) < 0,
// tau = min_k e_k(a) / (e_k(a) - e_k(b)) clamped to [0, 1] (the lowest k wins ties) is where F's silhouette crosses the segment from
// a's centre to b's; no such k, no contribution.  b gains max(tau - 1/2, 0), a loses max(1/2 - tau, 0).  In gather form, one lane per
// pixel, neighbours in the order left, right, up, down: a miss pixel holds min(1, sum of its gains), a hit pixel max(0, 1 - sum of
// its losses).
//
// Backward, stage 1.  One lane per pixel; a hit pixel writes ONE record of 9 floats, the gradient on the three corners of its own
// winning face: grad_depth w_k n / s with n = (v1 - v0) x (v2 - v0), plus, for every pair it owns (itself against each missed
// neighbour), G (dtau/de_k(a) de_k(a)/dv + dtau/de_k(b) de_k(b)/dv) on the two corners of the minimising edge, where
// G = [tau > 1/2][A(b) < 1] grad_coverage(b) + [tau < 1/2][A(a) > 0] grad_coverage(a): a saturated pixel, decided from the SAVED
// coverage image, passes nothing, and neither does tau = 1/2 exactly.  Miss pixels write nothing.
//
// Backward, stage 2.  Two segmented sums in gather form with segment_sum of segment_sum.h, which texture_sample_backward_kernel
// instantiates too: per face over its hit pixels (the host sorts them by face, stably), then per vertex over its (face, corner)
// slots.  No atomics, no LDS, no barrier; every output row is written, 0 for an empty segment.
#include "mesh_raster.h"
#include "segment_sum.h"

namespace {

constexpr int kLongSegment = 16;  // segments of more entries go to the wavefront (DESIGN.md section 25 has the A/B)

// the winning face of a visibility key (winning_key of the rasteriser), set up for the rays of the camera
__device__ __forceinline__ bool winning_face(const RasterArgs& a, unsigned long long key, long long& t, RasterFace& f) {
  unsigned long long vi[3];
  float v[3][3];
  if (!winning_key(a, key, t) || !load_face(a, t, vi, v, nullptr)) return false;
  f = raster_face(a.cam, vi, v);
  return true;
}

struct Crossing {
  bool any;  // some edge has b outside
  int k;     // the minimising edge
  float tau, ea, eb;
};

// where the silhouette of the face crosses the segment from the hit pixel (edge values ea, sum sa) to the missed one (eb)
__device__ __forceinline__ Crossing crossing(const float (&ea)[3], float sa, const float (&eb)[3]) {
  Crossing c;
  c.any = false, c.k = 0, c.tau = 0.0f, c.ea = 0.0f, c.eb = 0.0f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const bool outside = sa > 0.0f ? eb[k] < 0.0f : eb[k] > 0.0f;
    const float tk = ea[k] / (ea[k] - eb[k]);
    if (outside && (!c.any || tk < c.tau)) c.any = true, c.k = k, c.tau = tk, c.ea = ea[k], c.eb = eb[k];
  }
  c.tau = fminf(fmaxf(c.tau, 0.0f), 1.0f);
  return c;
}

__device__ __forceinline__ bool neighbour(int n, int i, int j, int H, int W, int& bi, int& bj) {  // left, right, up, down
  bi = i + (n == 2 ? -1 : n == 3 ? 1 : 0), bj = j + (n == 0 ? -1 : n == 1 ? 1 : 0);
  return bi >= 0 && bi < H && bj >= 0 && bj < W;
}

__global__ __launch_bounds__(kRasterBlock) void mesh_raster_coverage_kernel(RasterArgs a, const unsigned long long* __restrict__ vis, float* __restrict__ depth,
                                                                            float* __restrict__ coverage, int* __restrict__ face_ids) {
  const long long pix = (long long)blockIdx.x * kRasterBlock + threadIdx.x;
  const int H = a.cam.H, W = a.cam.W;
  if (pix >= (long long)H * W) return;
  const int i = (int)(pix / W), j = (int)(pix - (long long)i * W);
  long long t;
  RasterFace f;
  float z = 0.0f, cover, sum = 0.0f;
  int id = -1;
  if (winning_face(a, vis[pix], t, f)) {
    id = (int)t, z = raster_hit(a.cam, f, i, j, a.cull).z;
    float ea[3], eb[3];
    const float sa = raster_edges(a.cam, f, i, j, ea);
    for (int n = 0; n < 4; ++n) {
      int bi, bj;
      if (!neighbour(n, i, j, H, W, bi, bj)) continue;
      long long tb;
      RasterFace fb;
      if (winning_face(a, vis[(long long)bi * W + bj], tb, fb)) continue;  // hit against hit: no silhouette of this rule
      raster_edges(a.cam, f, bi, bj, eb);
      const Crossing c = crossing(ea, sa, eb);
      if (c.any) sum = sum + fmaxf(0.5f - c.tau, 0.0f);
    }
    cover = fmaxf(1.0f - sum, 0.0f);
  } else {
    for (int n = 0; n < 4; ++n) {
      int ai, aj;
      if (!neighbour(n, i, j, H, W, ai, aj)) continue;
      long long ta;
      RasterFace fa;
      if (!winning_face(a, vis[(long long)ai * W + aj], ta, fa)) continue;
      float ea[3], eb[3];
      const float sa = raster_edges(a.cam, fa, ai, aj, ea);
      raster_edges(a.cam, fa, i, j, eb);
      const Crossing c = crossing(ea, sa, eb);
      if (c.any) sum = sum + fmaxf(c.tau - 0.5f, 0.0f);
    }
    cover = fminf(sum, 1.0f);
  }
  depth[pix] = z;
  coverage[pix] = cover;
  face_ids[pix] = id;
}

__global__ __launch_bounds__(kRasterBlock) void mesh_geometry_backward_pixels_kernel(RasterArgs a, const int* __restrict__ face_ids, const float* __restrict__ coverage,
                                                                                     const float* __restrict__ grad_depth, const float* __restrict__ grad_coverage,
                                                                                     float* __restrict__ records, int* status) {
  const long long pix = (long long)blockIdx.x * kRasterBlock + threadIdx.x;
  const int H = a.cam.H, W = a.cam.W;
  if (pix >= (long long)H * W) return;
  const int i = (int)(pix / W), j = (int)(pix - (long long)i * W);
  const long long t = face_ids[pix];
  if (t < 0) return;  // a miss pixel owns nothing and writes nothing
  unsigned long long vi[3];
  float v[3][3], p[3][3], rec[3][3];
  bool known = t < a.num_faces;
  if (!known) *status = 1;  // (a plain store of one value: whichever lane wins, the word reads 1)
  known = known && load_face(a, t, vi, v, status);
  if (!known) {  // ids that are not this mesh's: the record the gather will read is 0, never what the buffer held before
#pragma unroll
    for (int x = 0; x < 9; ++x) records[9 * pix + x] = 0.0f;
    return;
  }
  const RasterFace f = raster_face(a.cam, vi, v);
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int x = 0; x < 3; ++x) p[k][x] = v[k][x] - a.cam.t[x], rec[k][x] = 0.0f;
  float ea[3], eb[3], da[3], db[3];
  const float sa = raster_edges(a.cam, f, i, j, ea);
  // depth: dz/dv_k = w_k n / s
  const float gz = grad_depth[pix];
  {
    float u1[3], u2[3], n[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) u1[x] = v[1][x] - v[0][x], u2[x] = v[2][x] - v[0][x];
    cross3(u1, u2, n);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float c = gz * ((ea[k] / sa) / sa);
#pragma unroll
      for (int x = 0; x < 3; ++x) rec[k][x] = c * n[x];
    }
  }
  // coverage: the pairs this pixel owns
  pixel_ray(i, j, H, W, a.cam.focal, a.cam.R, da);
  const float cover_a = coverage[pix], ga = grad_coverage[pix];
  for (int n = 0; n < 4; ++n) {
    int bi, bj;
    if (!neighbour(n, i, j, H, W, bi, bj)) continue;
    const long long b = (long long)bi * W + bj;
    if (face_ids[b] >= 0) continue;
    raster_edges(a.cam, f, bi, bj, eb);
    const Crossing c = crossing(ea, sa, eb);
    if (!c.any) continue;
    float G = 0.0f;
    if (c.tau > 0.5f && coverage[b] < 1.0f) G = grad_coverage[b];
    if (c.tau < 0.5f && cover_a > 0.0f) G = ga;
    if (G == 0.0f) continue;  // (the clamp of tau is never active where the pair counts: ea and -eb have one sign, so ea / (ea - eb) is in [0, 1])
    pixel_ray(bi, bj, H, W, a.cam.focal, a.cam.R, db);
    // tau = ea / q, q = ea - eb: dtau/dea = -eb / q^2, dtau/deb = ea / q^2; e_k = d . (p_k1 x p_k2) is linear in d
    const float q = c.ea - c.eb;
    const float ca = G * (-c.eb / (q * q)), cb = G * (c.ea / (q * q));
    float D[3], p1[3], p2[3], g1[3], g2[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
      D[x] = ca * da[x] + cb * db[x];
      p1[x] = c.k == 0 ? p[1][x] : c.k == 1 ? p[2][x] : p[0][x];
      p2[x] = c.k == 0 ? p[2][x] : c.k == 1 ? p[0][x] : p[1][x];
    }
    cross3(p2, D, g1);  // de_k/dp_k1 = p_k2 x d
    cross3(D, p1, g2);  // de_k/dp_k2 = d x p_k1
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const bool first = k == (c.k + 1) % 3, second = k == (c.k + 2) % 3;
#pragma unroll
      for (int x = 0; x < 3; ++x) rec[k][x] = rec[k][x] + (first ? g1[x] : second ? g2[x] : 0.0f);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int x = 0; x < 3; ++x) records[9 * pix + 3 * k + x] = rec[k][x];
}

// out[k, :] = the sum over segment k of rows[entries[e], :], C floats per row (an entry outside [0, num_rows) sets the status word
// and adds nothing; it is never dereferenced)
template <int C>
__device__ __forceinline__ void add_row(const float* __restrict__ rows, long long num_rows, int entry, float (&acc)[C], int* status) {
  if ((unsigned long long)(long long)entry >= (unsigned long long)num_rows) {
    *status = 1;
    return;
  }
  const float* g = rows + (long long)C * entry;
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = acc[c] + g[c];
}

// what segment_sum adds for entry e of the list
template <int C>
struct AddRow {
  const float* rows;
  long long num_rows;
  const int* entries;
  int* status;
  __device__ __forceinline__ void operator()(long long e, float (&acc)[C]) const { add_row<C>(rows, num_rows, entries[e], acc, status); }
};

template <int C>
__global__ __launch_bounds__(kRasterBlock) void segment_sum_kernel(const float* __restrict__ rows, long long num_rows, const int* __restrict__ entries, long long E,
                                                                   const long long* __restrict__ offsets, long long segments, int long_segment,
                                                                   float* __restrict__ out, int* status) {
  segment_sum<C, kRasterBlock>(offsets, E, segments, long_segment, out, AddRow<C>{rows, num_rows, entries, status});
}

}  // namespace

extern "C" {

int rf_mesh_raster_coverage(const RFCamera* camera, const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces,
                            const uint64_t* visibility_dev, uint32_t flags, float* depth_dev, float* coverage_dev, int32_t* face_ids_dev, void* stream) {
  if (!camera || !visibility_dev || !depth_dev || !coverage_dev || !face_ids_dev) return RF_ERR_NULL_POINTER;
  if ((num_vertices > 0 && !vertices_dev) || (num_faces > 0 && !faces_dev)) return RF_ERR_NULL_POINTER;
  const int rc = check_raster(camera, num_vertices, num_faces, 0.0f, 0u);
  if (rc != RF_OK) return rc;
  if (flags & ~(uint32_t)RF_RASTER_CULL_BACKFACES) return RF_ERR_UNSUPPORTED;
  const RasterArgs a = raster_args(camera, vertices_dev, num_vertices, faces_dev, num_faces, 0.0f, flags);
  const long long total = (long long)camera->height * camera->width;  // <= 2^28
  hipLaunchKernelGGL(mesh_raster_coverage_kernel, dim3((unsigned)((total + kRasterBlock - 1) / kRasterBlock)), dim3(kRasterBlock), 0, (hipStream_t)stream, a,
                     (const unsigned long long*)visibility_dev, depth_dev, coverage_dev, face_ids_dev);
  return launch_status();
}

int rf_mesh_geometry_backward_pixels(const RFCamera* camera, const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces,
                                     const int32_t* face_ids_dev, const float* coverage_dev, const float* grad_depth_dev, const float* grad_coverage_dev,
                                     uint32_t flags, float* records_dev, int32_t* status_dev, void* stream) {
  if (!camera || !face_ids_dev || !coverage_dev || !grad_depth_dev || !grad_coverage_dev || !records_dev || !status_dev) return RF_ERR_NULL_POINTER;
  if ((num_vertices > 0 && !vertices_dev) || (num_faces > 0 && !faces_dev)) return RF_ERR_NULL_POINTER;
  const int rc = check_raster(camera, num_vertices, num_faces, 0.0f, 0u);
  if (rc != RF_OK) return rc;
  if (flags & ~(uint32_t)RF_RASTER_CULL_BACKFACES) return RF_ERR_UNSUPPORTED;
  if (num_faces == 0) return RF_OK;  // every pixel is a miss: nothing is written
  const RasterArgs a = raster_args(camera, vertices_dev, num_vertices, faces_dev, num_faces, 0.0f, flags);
  const long long total = (long long)camera->height * camera->width;  // <= 2^28
  hipLaunchKernelGGL(mesh_geometry_backward_pixels_kernel, dim3((unsigned)((total + kRasterBlock - 1) / kRasterBlock)), dim3(kRasterBlock), 0, (hipStream_t)stream, a,
                     face_ids_dev, coverage_dev, grad_depth_dev, grad_coverage_dev, records_dev, status_dev);
  return launch_status();
}

int rf_mesh_geometry_backward_gather(const float* records_dev, int64_t num_pixels, const int32_t* hit_pixels_dev, int64_t num_hits, const int64_t* face_offsets_dev,
                                     int64_t num_faces, const int32_t* corner_slots_dev, const int64_t* vertex_offsets_dev, int64_t num_vertices,
                                     int32_t long_segment, uint32_t flags, float* face_grads_dev, float* grad_vertices_dev, int32_t* status_dev, void* stream) {
  if (!face_offsets_dev || !vertex_offsets_dev || !status_dev) return RF_ERR_NULL_POINTER;
  if ((num_hits > 0 && (!records_dev || !hit_pixels_dev)) || (num_faces > 0 && (!corner_slots_dev || !face_grads_dev)) || (num_vertices > 0 && !grad_vertices_dev))
    return RF_ERR_NULL_POINTER;
  if (num_pixels < 0 || num_pixels >= (1ll << 31) || num_hits < 0 || num_hits > num_pixels) return RF_ERR_BAD_SHAPE;
  if (num_faces < 0 || num_faces >= (1ll << 31) / 3 || num_vertices < 0 || num_vertices >= (1ll << 31) || long_segment < 0) return RF_ERR_BAD_SHAPE;
  if (flags) return RF_ERR_UNSUPPORTED;
  const int threshold = long_segment ? long_segment : kLongSegment;
  if (num_faces > 0) {
    hipLaunchKernelGGL(segment_sum_kernel<9>, dim3((unsigned)((num_faces + kRasterBlock - 1) / kRasterBlock)), dim3(kRasterBlock), 0, (hipStream_t)stream, records_dev,
                       (long long)num_pixels, hit_pixels_dev, (long long)num_hits, (const long long*)face_offsets_dev, (long long)num_faces, threshold, face_grads_dev,
                       status_dev);
    const int rc = launch_status();
    if (rc != RF_OK) return rc;
  }
  if (num_vertices > 0) {
    hipLaunchKernelGGL(segment_sum_kernel<3>, dim3((unsigned)((num_vertices + kRasterBlock - 1) / kRasterBlock)), dim3(kRasterBlock), 0, (hipStream_t)stream,
                       face_grads_dev, (long long)(3 * num_faces), corner_slots_dev, (long long)(3 * num_faces), (const long long*)vertex_offsets_dev,
                       (long long)num_vertices, threshold, grad_vertices_dev, status_dev);
    return launch_status();
  }
  return RF_OK;
}

}  // extern "C"
