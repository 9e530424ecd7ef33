// mesh_sign.h -- the sign rule of rf_mesh_signed_distance and the tables of rf_mesh_face_pseudonormals (mesh_sign_kernels.hip): the
// angle-weighted pseudonormal of Baerentzen and Aanaes (2005) on top of closest_gradient_on_face (mesh_distance_grad.h), in float32,
// every operation and its order fixed (the library is built with -ffp-contract=off).  This is the only place the rule exists;
// docs/mesh_sign_errors.md restates it as the contract and tests/mesh_sign_model.py in numpy.
//
//   unit_normal(a, b, c):  u = b - a, v = c - a, n = u x v (the expression of closest_on_face), nn = dot(n, n), len = sqrt(nn),
//                          n^ = n / len per component when nn > 0, else 0.
//   Corner angles:         alpha_k = atan2f(len, dot(e1_k, e2_k)) with the two edges that leave corner k:
//                          a: (b - a, c - a),  b: (c - b, a - b),  c: (a - c, b - c).
//   Feature of (p, f):     g = closest_gradient_on_face(p, a, b, c).  Region 3 is FACE f.  Region r in {0, 1, 2} is the segment (x, y)
//                          = (a, b), (b, c), (c, a): beta_x == 1 gives VERTEX x, else beta_y == 1 gives VERTEX y, else EDGE r of f.
//   N of the feature:      FACE: n^_f.  VERTEX v: vertex_normals[v] (the sum of alpha n^ over the corners at v, made by the gather).
//                          EDGE (f, r) with partner h: n^_f + n^_h when h >= 0, else n^_f.
//   Signed distance:       r = p - q per component, s = dot(r, N), sign = s < 0 ? -1 : +1 (a NaN and a zero go to +),
//                          signed = sign * sqrt(d2) with q and d2 the forward's bits.
#pragma once

#include "mesh_distance_grad.h"

namespace {

constexpr int kSignFace = 0, kSignEdge = 1, kSignVertex = 2, kSignNone = -1;

struct SignNormal {
  float x, y, z, len;
};

__device__ __forceinline__ SignNormal unit_normal(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz) {
  const float ux = bx - ax, uy = by - ay, uz = bz - az;
  const float vx = cx - ax, vy = cy - ay, vz = cz - az;
  const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
  const float nn = dist_dot(nx, ny, nz, nx, ny, nz);
  const float len = sqrtf(nn);
  SignNormal n = {0.0f, 0.0f, 0.0f, len};
  if (nn > 0.0f) n.x = nx / len, n.y = ny / len, n.z = nz / len;
  return n;
}

// the angle at corner o between the edges to x and to y; len = |n| of the face
__device__ __forceinline__ float corner_angle(float len, float ox, float oy, float oz, float xx, float xy, float xz, float yx, float yy, float yz) {
  return atan2f(len, dist_dot(xx - ox, xy - oy, xz - oz, yx - ox, yy - oy, yz - oz));
}

struct SignFeature {
  int kind;    // kSignFace, kSignEdge, kSignVertex
  int corner;  // kSignEdge: the edge r of the face; kSignVertex: the corner (0, 1, 2 = a, b, c) of the face
};

__device__ __forceinline__ SignFeature sign_feature(const FaceGradient& g) {
  if (g.region == 3) return {kSignFace, 0};
  // the segment (x, y) of region r has beta_x = 1 - t, beta_y = t and the third 0: at most one of the three is 1, and it is x or y
  // (constant indices only: an array indexed by a register would be moved to LDS or scratch)
  if (g.beta[0] == 1.0f) return {kSignVertex, 0};
  if (g.beta[1] == 1.0f) return {kSignVertex, 1};
  if (g.beta[2] == 1.0f) return {kSignVertex, 2};
  return {kSignEdge, g.region};
}

// signed distance of p whose closest point g.best has pseudonormal N
__device__ __forceinline__ float signed_distance(float px, float py, float pz, const FaceClosest& best, float nx, float ny, float nz) {
  const float rx = px - best.x, ry = py - best.y, rz = pz - best.z;
  const float s = dist_dot(rx, ry, rz, nx, ny, nz);
  const float d = sqrtf(best.d2);
  return s < 0.0f ? -d : d;
}

}  // namespace
