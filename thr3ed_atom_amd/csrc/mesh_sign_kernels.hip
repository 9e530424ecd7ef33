// mesh_sign_kernels.hip -- the sign of the distance to a closed triangle mesh (rf_mesh_face_pseudonormals and
// rf_mesh_signed_distance of relu_field_ext.h): what thr3ed_atom_amd/mesh_sign.py is built on.  DESIGN.md section 29 has the contract
// and the measurements, docs/mesh_sign_errors.md the rule, the error bounds and the decision margin, tests/mesh_sign_model.py the numpy
// model.
//
// face_pseudonormals_kernel: one lane per face, 256-lane blocks.  The lane reads its three corners (every index is checked against the
// vertex array first) and writes the unit normal n^ (3 floats) and the record (alpha_a n^, alpha_b n^, alpha_c n^) (9 floats,
// corner-major).  The per-vertex sum of the records is rf_mesh_geometry_backward_gather's with every face as its own entry: an order
// fixed by the mesh, no atomics.
//
// signed_distance_kernel: one lane per query, 256-lane blocks.  The lane reads its query, the face the forward found and that face's
// corners, runs closest_gradient_on_face, names the feature that holds the closest point and reads that feature's pseudonormal: its own
// face's, a row of vertex_normals, or its own plus the partner face's across the edge (the partner's corners are a second gather of 36
// bytes, taken by the lanes whose closest point lies on an edge only).  It writes
//   signed[i]  = +-sqrt(d2)                (the forward's distance bits with the sign of dot(p - q, N))
//   feature[i] = (kind, index)             kind 0 face / 1 edge / 2 vertex / -1 none; index = the face, 3 face + edge, the vertex
//   normal[i]  = N                         (3 floats, not normalised)
// feature and normal may be NULL.  A query with face -1 writes +inf, (-1, -1) and zeros.  Every face id, vertex index and partner is
// checked against its array before it is used as an index; a bad one raises the status word and the lane writes nothing.
#include "mesh_sign.h"

namespace {

constexpr int kSignBlock = 256;

struct FaceNormalArgs {
  const float* vertices;
  const long long* faces;
  float* normals;
  float* records;
  int* status;
  long long num_vertices, num_faces;
};

__global__ __launch_bounds__(kSignBlock) void face_pseudonormals_kernel(FaceNormalArgs a) {
  const long long f = (long long)blockIdx.x * kSignBlock + threadIdx.x;
  if (f >= a.num_faces) return;
  const unsigned long long V = (unsigned long long)a.num_vertices;
  const long long* idx = a.faces + 3 * f;
  const unsigned long long i0 = (unsigned long long)idx[0], i1 = (unsigned long long)idx[1], i2 = (unsigned long long)idx[2];
  float n[3] = {0.0f, 0.0f, 0.0f}, alpha[3] = {0.0f, 0.0f, 0.0f};
  if (i0 >= V || i1 >= V || i2 >= V) {
    *a.status = 1;  // (zeros are written: the gather that follows reads every record)
  } else {
    const float *p0 = a.vertices + 3 * i0, *p1 = a.vertices + 3 * i1, *p2 = a.vertices + 3 * i2;
    const float ax = p0[0], ay = p0[1], az = p0[2], bx = p1[0], by = p1[1], bz = p1[2], cx = p2[0], cy = p2[1], cz = p2[2];
    const SignNormal u = unit_normal(ax, ay, az, bx, by, bz, cx, cy, cz);
    n[0] = u.x, n[1] = u.y, n[2] = u.z;
    alpha[0] = corner_angle(u.len, ax, ay, az, bx, by, bz, cx, cy, cz);
    alpha[1] = corner_angle(u.len, bx, by, bz, cx, cy, cz, ax, ay, az);
    alpha[2] = corner_angle(u.len, cx, cy, cz, ax, ay, az, bx, by, bz);
  }
  a.normals[3 * f] = n[0], a.normals[3 * f + 1] = n[1], a.normals[3 * f + 2] = n[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int j = 0; j < 3; ++j) a.records[9 * f + 3 * k + j] = alpha[k] * n[j];
  }
}

struct SignArgs {
  const float* vertices;
  const long long* faces;
  const int* partners;
  const float* vertex_normals;
  const float* points;
  const long long* face;
  float* signed_distance;
  int* feature;
  float* normal;
  int* status;
  long long num_vertices, num_faces, num_points;
};

__device__ __forceinline__ void write_sign(const SignArgs& a, long long i, float d, int kind, int index, float nx, float ny, float nz) {
  a.signed_distance[i] = d;
  if (a.feature) a.feature[2 * i] = kind, a.feature[2 * i + 1] = index;
  if (a.normal) a.normal[3 * i] = nx, a.normal[3 * i + 1] = ny, a.normal[3 * i + 2] = nz;
}

__global__ __launch_bounds__(kSignBlock) void signed_distance_kernel(SignArgs a) {
  const long long i = (long long)blockIdx.x * kSignBlock + threadIdx.x;
  if (i >= a.num_points) return;
  const long long f = a.face[i];
  if (f < 0) {  // nothing within max_distance
    write_sign(a, i, INFINITY, kSignNone, -1, 0.0f, 0.0f, 0.0f);
    return;
  }
  if (f >= a.num_faces) {
    *a.status = 1;
    return;
  }
  const unsigned long long V = (unsigned long long)a.num_vertices;
  const long long* idx = a.faces + 3 * f;
  const unsigned long long v0 = (unsigned long long)idx[0], v1 = (unsigned long long)idx[1], v2 = (unsigned long long)idx[2];
  if (v0 >= V || v1 >= V || v2 >= V) {
    *a.status = 1;
    return;
  }
  const float *p0 = a.vertices + 3 * v0, *p1 = a.vertices + 3 * v1, *p2 = a.vertices + 3 * v2;
  const float ax = p0[0], ay = p0[1], az = p0[2], bx = p1[0], by = p1[1], bz = p1[2], cx = p2[0], cy = p2[1], cz = p2[2];
  const float px = a.points[3 * i], py = a.points[3 * i + 1], pz = a.points[3 * i + 2];
  const FaceGradient g = closest_gradient_on_face(px, py, pz, ax, ay, az, bx, by, bz, cx, cy, cz);
  const SignFeature feature = sign_feature(g);
  float nx, ny, nz;
  int index;
  if (feature.kind == kSignVertex) {
    const unsigned long long w = feature.corner == 0 ? v0 : (feature.corner == 1 ? v1 : v2);
    const float* n = a.vertex_normals + 3 * w;
    nx = n[0], ny = n[1], nz = n[2], index = (int)w;
  } else {
    const SignNormal own = unit_normal(ax, ay, az, bx, by, bz, cx, cy, cz);
    nx = own.x, ny = own.y, nz = own.z, index = (int)f;
    if (feature.kind == kSignEdge) {
      index = 3 * (int)f + feature.corner;
      const long long h = a.partners[3 * f + feature.corner];
      if (h >= a.num_faces) {
        *a.status = 2;
        return;
      }
      if (h >= 0) {
        const long long* hidx = a.faces + 3 * h;
        const unsigned long long h0 = (unsigned long long)hidx[0], h1 = (unsigned long long)hidx[1], h2 = (unsigned long long)hidx[2];
        if (h0 >= V || h1 >= V || h2 >= V) {
          *a.status = 1;
          return;
        }
        const float *q0 = a.vertices + 3 * h0, *q1 = a.vertices + 3 * h1, *q2 = a.vertices + 3 * h2;
        const SignNormal other = unit_normal(q0[0], q0[1], q0[2], q1[0], q1[1], q1[2], q2[0], q2[1], q2[2]);
        nx = nx + other.x, ny = ny + other.y, nz = nz + other.z;
      }
    }
  }
  write_sign(a, i, signed_distance(px, py, pz, g.best, nx, ny, nz), feature.kind, index, nx, ny, nz);
}

}  // namespace

extern "C" {

int rf_ext_abi_version(void) { return 1; }

int rf_mesh_face_pseudonormals(const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces, uint32_t flags, float* normals_dev,
                               float* records_dev, int32_t* status_dev, void* stream) {
  if (!status_dev) return RF_ERR_NULL_POINTER;
  if (num_faces > 0 && (!vertices_dev || !faces_dev || !normals_dev || !records_dev)) return RF_ERR_NULL_POINTER;
  if (num_vertices < 0 || num_faces < 0) return RF_ERR_BAD_SHAPE;
  if (num_vertices >= (1ll << 31) || num_faces >= (1ll << 31) / 3) return RF_ERR_BAD_SHAPE;
  if (flags != 0) return RF_ERR_UNSUPPORTED;
  if (num_faces == 0) return RF_OK;
  FaceNormalArgs a;
  a.vertices = vertices_dev, a.faces = (const long long*)faces_dev, a.normals = normals_dev, a.records = records_dev, a.status = status_dev;
  a.num_vertices = num_vertices, a.num_faces = num_faces;
  hipLaunchKernelGGL(face_pseudonormals_kernel, dim3((unsigned)((num_faces + kSignBlock - 1) / kSignBlock)), dim3(kSignBlock), 0, (hipStream_t)stream, a);
  return launch_status();
}

int rf_mesh_signed_distance(const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces, const int32_t* partners_dev,
                            const float* vertex_normals_dev, const float* points_dev, const int64_t* face_dev, int64_t num_points, uint32_t flags,
                            float* signed_dev, int32_t* feature_dev, float* normal_dev, int32_t* status_dev, void* stream) {
  if (!status_dev) return RF_ERR_NULL_POINTER;
  if (num_faces > 0 && (!vertices_dev || !faces_dev || !partners_dev || !vertex_normals_dev)) return RF_ERR_NULL_POINTER;
  if (num_points > 0 && (!points_dev || !face_dev || !signed_dev)) return RF_ERR_NULL_POINTER;
  if (num_vertices < 0 || num_faces < 0 || num_points < 0) return RF_ERR_BAD_SHAPE;
  if (num_vertices >= (1ll << 31) || num_faces >= (1ll << 31) / 3 || num_points >= (1ll << 31)) return RF_ERR_BAD_SHAPE;
  if (flags != 0) return RF_ERR_UNSUPPORTED;
  if (num_points == 0 || num_faces == 0) return RF_OK;
  SignArgs a;
  a.vertices = vertices_dev, a.faces = (const long long*)faces_dev, a.partners = partners_dev, a.vertex_normals = vertex_normals_dev;
  a.points = points_dev, a.face = (const long long*)face_dev;
  a.signed_distance = signed_dev, a.feature = feature_dev, a.normal = normal_dev, a.status = status_dev;
  a.num_vertices = num_vertices, a.num_faces = num_faces, a.num_points = num_points;
  hipLaunchKernelGGL(signed_distance_kernel, dim3((unsigned)((num_points + kSignBlock - 1) / kSignBlock)), dim3(kSignBlock), 0, (hipStream_t)stream, a);
  return launch_status();
}

}  // extern "C"
