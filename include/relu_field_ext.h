/* relu_field_ext.h -- entry points of librelu_field_hip.so added after the list of relu_field.h was closed.
 *
 * relu_field.h, its RF_ABI_VERSION and its list of symbols are frozen: a host that was built against them keeps working.  Entry points
 * from here on are declared in THIS header, which has a version of its own.  The conventions are relu_field.h's: device pointers end in
 * _dev, every function returns RF_OK or a negative RF_ERR_* code and never throws, arguments are validated before any launch, `stream`
 * is a hipStream_t (NULL: the default stream), nothing synchronises with the host.
 */
#ifndef RELU_FIELD_EXT_H_
#define RELU_FIELD_EXT_H_

#include "relu_field.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RF_EXT_ABI_VERSION 1

/* RF_EXT_ABI_VERSION of the library that was loaded */
int rf_ext_abi_version(void);

/* ---- The sign of the distance to a closed triangle mesh (csrc/mesh_sign_kernels.hip over csrc/mesh_sign.h; DESIGN.md section 29;
 * docs/mesh_sign_errors.md; thr3ed_atom_amd/mesh_sign.py builds MeshSignGrid, mesh_to_sdf and signed_mesh_distance on it) -----------
 * The angle-weighted pseudonormal of Baerentzen and Aanaes (2005): for a query p, let q be the closest point rf_mesh_closest_points
 * found and F the mesh feature -- face, edge or vertex -- that holds q; then sign = sign((p - q) . N_F).  Exact for a closed,
 * consistently oriented, edge-manifold mesh whose face normals (v1 - v0) x (v2 - v0) point outward; negative is inside.  In float32,
 * with dot(x, y) = (x0 y0 + x1 y1) + x2 y2 and no contraction:
 *   unit_normal(a, b, c):  n = (b - a) x (c - a), nn = dot(n, n), len = sqrt(nn), n^ = n / len per component when nn > 0, else 0.
 *   Corner angles:  alpha_k = atan2f(len, dot(e1_k, e2_k)) with the two edges that leave corner k: (b - a, c - a) at a,
 *     (c - b, a - b) at b, (a - c, b - c) at c.
 *   Feature of (p, f), from the candidate of the rule of rf_mesh_closest_gradients that won: the plane is FACE f; a segment (x, y) --
 *     (a, b), (b, c), (c, a) for region 0, 1, 2 -- is VERTEX x when beta_x == 1, else VERTEX y when beta_y == 1, else EDGE region of f.
 *   N:  FACE: n^_f.  VERTEX v: vertex_normals_dev[v].  EDGE (f, k) with h = partners_dev[3 f + k]: n^_f + n^_h when h >= 0, else n^_f.
 *   r = p - q per component, s = dot(r, N), sign = s < 0 ? -1 : +1 (a NaN and a zero go to +: on the surface the result is +0),
 *   signed = sign * sqrt(d2) with q and d2 the bits of rf_mesh_closest_points.
 *
 * rf_mesh_face_pseudonormals: one lane per face.  normals_dev[f] = n^_f (3 floats), records_dev[f] = (alpha_a n^, alpha_b n^,
 * alpha_c n^) (9 floats, corner-major).  The vertex table is the per-vertex sum of the records, made by
 * rf_mesh_geometry_backward_gather with num_pixels = num_hits = num_faces, hit_pixels = 0 .. num_faces - 1 and face offsets
 * 0 .. num_faces: an order fixed by the mesh, no atomics.  A face with a vertex index outside [0, num_vertices) sets status_dev[0]
 * (int32, zeroed by the caller) to 1 and writes zeros.
 *
 * rf_mesh_signed_distance: one lane per query, one launch, no atomics, no LDS.  partners_dev is int32 [num_faces, 3]: the face across
 * edge k of face f (0, 1, 2 = ab, bc, ca), negative where there is none.  face_dev is the forward's closest face per query.  A query
 * with face_dev[i] >= 0 writes signed_dev[i], feature_dev[i] = (kind, index) (two int32: kind 0 face / 1 edge / 2 vertex; index = f,
 * 3 f + k, v) and normal_dev[i] = N (3 floats, not normalised).  A query with face -1 (nothing within max_distance) writes +inf,
 * (-1, -1) and zeros.  feature_dev and normal_dev may be NULL.  A face id >= num_faces or a vertex index outside [0, num_vertices)
 * sets status_dev[0] to 1, a partner >= num_faces sets it to 2; the query then writes nothing.
 *
 * Before any launch, in this order: RF_ERR_NULL_POINTER (status_dev; with num_faces > 0 the mesh arrays and tables, for
 * rf_mesh_face_pseudonormals both outputs; with num_points > 0 points_dev, face_dev and signed_dev), RF_ERR_BAD_SHAPE (a negative count;
 * num_vertices or num_points >= 2^31; 3 num_faces >= 2^31), RF_ERR_UNSUPPORTED (any flag bit: none is defined); then num_faces == 0
 * (or num_points == 0) return RF_OK without a launch. */
int rf_mesh_face_pseudonormals(const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces, uint32_t flags,
                               float* normals_dev, float* records_dev, int32_t* status_dev, void* stream);
int rf_mesh_signed_distance(const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces,
                            const int32_t* partners_dev, const float* vertex_normals_dev, const float* points_dev, const int64_t* face_dev,
                            int64_t num_points, uint32_t flags, float* signed_dev, int32_t* feature_dev, float* normal_dev,
                            int32_t* status_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RELU_FIELD_EXT_H_ */
