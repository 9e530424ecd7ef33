// mesh_distance_grad_kernels.hip -- the adjoint of rf_mesh_closest_points (rf_mesh_closest_gradients of relu_field.h): what
// thr3ed_atom_amd/mesh_distance_grad.py is built on.  DESIGN.md section 28 has the contract and the measurements,
// docs/mesh_distance_grad_errors.md the rule, the envelope argument and the error bounds, tests/mesh_distance_grad_model.py the numpy
// model.
//
// One lane per query, 256-lane blocks, one launch.  The lane reads its query, the face the forward found and that face's three
// corners (every index is checked against its array first), runs closest_gradient_on_face of mesh_distance_grad.h and writes
//   grad_points[i]  = G u                 (3 floats)
//   records[i]      = -beta_k G u         (9 floats, corner-major)
//   barycentrics[i] = beta                (3 floats)
//   region[i]       = 0, 1, 2 (segments ab, bc, ca), 3 (the plane)
// with u = (p - q) / sqrt(d2), 0 when d2 is 0.  Each output may be NULL.  The records are summed per face and per vertex by
// rf_mesh_geometry_backward_gather (mesh_fit_kernels.hip), whose contract is stated on lists: nothing is added here.
// The corners are a gather of 36 bytes per query from three places; the branches of the rule are selects of a few registers: no lane
// runs a loop another lane of its wavefront does not.  Measured: 10^6 queries take 0.03 ms with all outputs;
// the stable sort by face that follows when vertices want a gradient takes 0.4 ms and is the cost of that path.
#include "mesh_distance_grad.h"

namespace {

constexpr int kGradBlock = 256;

struct GradientArgs {
  const float* vertices;
  const long long* faces;
  const float* points;
  const long long* face;
  const float* grad_distance;
  float* grad_points;
  float* records;
  float* barycentrics;
  int* region;
  int* status;
  long long num_vertices, num_faces, num_points;
};

__device__ __forceinline__ void write_rows(const GradientArgs& a, long long i, const float (&gp)[3], const float (&rec)[9], const float (&beta)[3], int region,
                                           bool with_record) {
  if (a.grad_points) a.grad_points[3 * i] = gp[0], a.grad_points[3 * i + 1] = gp[1], a.grad_points[3 * i + 2] = gp[2];
  if (a.records && with_record) {
#pragma unroll
    for (int j = 0; j < 9; ++j) a.records[9 * i + j] = rec[j];
  }
  if (a.barycentrics) a.barycentrics[3 * i] = beta[0], a.barycentrics[3 * i + 1] = beta[1], a.barycentrics[3 * i + 2] = beta[2];
  if (a.region) a.region[i] = region;
}

__global__ __launch_bounds__(kGradBlock) void closest_gradients_kernel(GradientArgs a) {
  const long long i = (long long)blockIdx.x * kGradBlock + threadIdx.x;
  if (i >= a.num_points) return;
  float gp[3] = {0.0f, 0.0f, 0.0f}, beta[3] = {0.0f, 0.0f, 0.0f};
  float rec[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  const long long f = a.face[i];
  if (f < 0) {  // nothing within max_distance: zero rows, no record
    write_rows(a, i, gp, rec, beta, -1, false);
    return;
  }
  if (f >= a.num_faces) {
    *a.status = 1;
    write_rows(a, i, gp, rec, beta, -1, true);
    return;
  }
  const unsigned long long V = (unsigned long long)a.num_vertices;
  const long long* idx = a.faces + 3 * f;
  const unsigned long long i0 = (unsigned long long)idx[0], i1 = (unsigned long long)idx[1], i2 = (unsigned long long)idx[2];
  if (i0 >= V || i1 >= V || i2 >= V) {
    *a.status = 1;
    write_rows(a, i, gp, rec, beta, -1, true);
    return;
  }
  const float *p0 = a.vertices + 3 * i0, *p1 = a.vertices + 3 * i1, *p2 = a.vertices + 3 * i2;
  const float px = a.points[3 * i], py = a.points[3 * i + 1], pz = a.points[3 * i + 2];
  const float G = a.grad_distance[i];
  const FaceGradient g = closest_gradient_on_face(px, py, pz, p0[0], p0[1], p0[2], p1[0], p1[1], p1[2], p2[0], p2[1], p2[2]);
  const float rx = px - g.best.x, ry = py - g.best.y, rz = pz - g.best.z;
  const float len = sqrtf(dist_dot(rx, ry, rz, rx, ry, rz));
  if (len > 0.0f) gp[0] = G * (rx / len), gp[1] = G * (ry / len), gp[2] = G * (rz / len);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    beta[k] = g.beta[k];
#pragma unroll
    for (int j = 0; j < 3; ++j) rec[3 * k + j] = -(g.beta[k] * gp[j]);
  }
  write_rows(a, i, gp, rec, beta, g.region, true);
}

}  // namespace

extern "C" {

int rf_mesh_closest_gradients(const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces, const float* points_dev,
                              const int64_t* face_dev, const float* grad_distance_dev, int64_t num_points, uint32_t flags, float* grad_points_dev,
                              float* records_dev, float* barycentrics_dev, int32_t* region_dev, int32_t* status_dev, void* stream) {
  if (!status_dev) return RF_ERR_NULL_POINTER;
  if (num_faces > 0 && (!vertices_dev || !faces_dev)) return RF_ERR_NULL_POINTER;
  if (num_points > 0 && (!points_dev || !face_dev || !grad_distance_dev)) return RF_ERR_NULL_POINTER;
  if (num_points > 0 && !grad_points_dev && !records_dev && !barycentrics_dev && !region_dev) return RF_ERR_NULL_POINTER;
  if (num_vertices < 0 || num_faces < 0 || num_points < 0) return RF_ERR_BAD_SHAPE;
  if (num_vertices >= (1ll << 31) || num_faces >= (1ll << 31) || num_points >= (1ll << 31)) return RF_ERR_BAD_SHAPE;
  if (flags != 0) return RF_ERR_UNSUPPORTED;
  if (num_points == 0 || num_faces == 0) return RF_OK;
  GradientArgs a;
  a.vertices = vertices_dev, a.faces = (const long long*)faces_dev, a.points = points_dev, a.face = (const long long*)face_dev;
  a.grad_distance = grad_distance_dev;
  a.grad_points = grad_points_dev, a.records = records_dev, a.barycentrics = barycentrics_dev, a.region = region_dev, a.status = status_dev;
  a.num_vertices = num_vertices, a.num_faces = num_faces, a.num_points = num_points;
  hipLaunchKernelGGL(closest_gradients_kernel, dim3((unsigned)((num_points + kGradBlock - 1) / kGradBlock)), dim3(kGradBlock), 0, (hipStream_t)stream, a);
  return launch_status();
}

}  // extern "C"
