// mesh_distance_grad.h -- the gradient rule of rf_mesh_closest_gradients (mesh_distance_grad_kernels.hip): which candidate of
// closest_on_face (mesh_distance.h) wins for ONE triangle and one query, and the barycentrics of its closest point.  It is built from
// the helpers of mesh_distance.h alone -- dist_segment, dist_candidate, dist_edge, dist_dot -- in the forward rule's order with the
// forward rule's strict <, so the selected point and its d2 are the forward's bits.  docs/mesh_distance_grad_errors.md restates it as
// the contract, tests/mesh_distance_grad_model.py in numpy.
//
//   Segment (x, y) won, parameter t (the t of dist_segment, the same operations):  beta_x = 1 - t, beta_y = t, the third 0.
//   The plane won:  E_ab, E_bc, E_ca = the three dist_edge values of the accept test at the UNCLAMPED q, S = (E_ab + E_bc) + E_ca,
//                   beta_c = E_ab / S, beta_a = E_bc / S, beta_b = E_ca / S.  S not > 0: the best segment stays.
//   region = 0, 1, 2 for the segments ab, bc, ca and 3 for the plane.
// With r = p - q per component, len = sqrt(dist_dot(r, r)) (= sqrt(d2), the same bits) and u = r / len (0 when len is not > 0):
// d(distance)/dp = u, d(distance)/d(corner k) = -beta_k u.
//
// KEEP IN STEP with mesh_distance.h: grad_segment_t repeats the parameter of dist_segment (which does not return it) and
// closest_gradient_on_face repeats the candidate order and the plane block of closest_on_face (which keeps neither the winner nor
// the edge values).  mesh_distance.h is pinned by its own ABI test and may not grow these outputs; a change of the rule there must be
// made here too.  The agreement is tested, not structural: tests/test_hip_mesh_distance_grad.py compares the point and the distance
// this rule selects with the forward's, bit for bit, on every query it runs.
#pragma once

#include "mesh_distance.h"

namespace {

struct FaceGradient {
  FaceClosest best;  // the forward's d2 and point
  int region;
  float beta[3];  // of the corners a, b, c
};

// the parameter dist_segment clamps to [0, 1]: the same operations in the same order
__device__ __forceinline__ float grad_segment_t(float px, float py, float pz, float ax, float ay, float az, float bx, float by, float bz) {
  const float ex = bx - ax, ey = by - ay, ez = bz - az;
  const float wx = px - ax, wy = py - ay, wz = pz - az;
  const float l = dist_dot(ex, ey, ez, ex, ey, ez);
  float t = 0.0f;
  if (l > 0.0f) t = fminf(fmaxf(dist_dot(wx, wy, wz, ex, ey, ez) / l, 0.0f), 1.0f);
  return t;
}

__device__ __forceinline__ FaceGradient closest_gradient_on_face(float px, float py, float pz, float ax, float ay, float az, float bx, float by, float bz, float cx,
                                                                 float cy, float cz) {
  const DistBox k = {fminf(fminf(ax, bx), cx), fminf(fminf(ay, by), cy), fminf(fminf(az, bz), cz),
                     fmaxf(fmaxf(ax, bx), cx), fmaxf(fmaxf(ay, by), cy), fmaxf(fmaxf(az, bz), cz)};
  FaceGradient g;
  g.best = dist_segment(px, py, pz, ax, ay, az, bx, by, bz, k);
  g.region = 0;
  float t = grad_segment_t(px, py, pz, ax, ay, az, bx, by, bz);
  FaceClosest c = dist_segment(px, py, pz, bx, by, bz, cx, cy, cz, k);
  if (c.d2 < g.best.d2) g.best = c, g.region = 1, t = grad_segment_t(px, py, pz, bx, by, bz, cx, cy, cz);
  c = dist_segment(px, py, pz, cx, cy, cz, ax, ay, az, k);
  if (c.d2 < g.best.d2) g.best = c, g.region = 2, t = grad_segment_t(px, py, pz, cx, cy, cz, ax, ay, az);
  const float s1 = 1.0f - t;
  g.beta[0] = g.region == 0 ? s1 : (g.region == 2 ? t : 0.0f);
  g.beta[1] = g.region == 1 ? s1 : (g.region == 0 ? t : 0.0f);
  g.beta[2] = g.region == 2 ? s1 : (g.region == 1 ? t : 0.0f);
  const float ux = bx - ax, uy = by - ay, uz = bz - az;
  const float vx = cx - ax, vy = cy - ay, vz = cz - az;
  const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
  const float nn = dist_dot(nx, ny, nz, nx, ny, nz);
  if (nn > 0.0f) {
    const float s = dist_dot(px - ax, py - ay, pz - az, nx, ny, nz) / nn;
    const float qx = px - s * nx, qy = py - s * ny, qz = pz - s * nz;
    const float e_ab = dist_edge(ax, ay, az, bx, by, bz, qx, qy, qz, nx, ny, nz);
    const float e_bc = dist_edge(bx, by, bz, cx, cy, cz, qx, qy, qz, nx, ny, nz);
    const float e_ca = dist_edge(cx, cy, cz, ax, ay, az, qx, qy, qz, nx, ny, nz);
    if (e_ab >= 0.0f && e_bc >= 0.0f && e_ca >= 0.0f) {
      c = dist_candidate(px, py, pz, qx, qy, qz, k);
      const float S = (e_ab + e_bc) + e_ca;
      if (c.d2 < g.best.d2 && S > 0.0f) {
        g.best = c, g.region = 3;
        g.beta[0] = e_bc / S, g.beta[1] = e_ca / S, g.beta[2] = e_ab / S;
      }
    }
  }
  return g;
}

}  // namespace
