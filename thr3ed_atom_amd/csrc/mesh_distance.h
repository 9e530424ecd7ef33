// mesh_distance.h -- the distance rule of rf_mesh_closest_points (mesh_distance_kernels.hip): the closest point of ONE triangle to
// one query, in float32, every operation and its order fixed (the library is built with -ffp-contract=off).  This is the only
// place the rule exists; docs/mesh_distance_errors.md restates it as the contract and tests/mesh_distance_model.py in numpy.
//
//   dot(x, y) = (x0 y0 + x1 y1) + x2 y2,  lo / hi = the per-axis minimum / maximum of the three corners (the face's box).
//   Segment (a, b):  e = b - a, w = p - a, l = dot(e, e), t = l > 0 ? min(max(dot(w, e) / l, 0), 1) : 0, q = a + t e.
//   Plane:           u = b - a, v = c - a, w = p - a, n = u x v, nn = dot(n, n); only when nn > 0: s = dot(w, n) / nn, q = p - s n, and
//                    the candidate counts only when dot((b - a) x (q - a), n), dot((c - b) x (q - b), n) and dot((a - c) x (q - c), n)
//                    are all >= 0.
//   Every candidate point is clamped per axis to [lo, hi] (no change in exact arithmetic; in float32 it keeps q inside the box the
//   face was registered with, which is what the stop test of the ring search rests on), then d = p - q, d2 = dot(d, d).
//   Order: segment ab is taken, then bc, ca and the plane replace it only when their d2 is strictly smaller.
// fmaxf / fminf drop a NaN operand, every comparison with NaN is false: a zero-length edge, a zero-area face or a repeated vertex
// contribute their segments or their point and never a NaN.
#pragma once

#include "rf_device.h"

namespace {

struct FaceClosest {
  float d2, x, y, z;
};

__device__ __forceinline__ float dist_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

__device__ __forceinline__ float dist_clamp(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

struct DistBox {
  float lx, ly, lz, hx, hy, hz;
};

__device__ __forceinline__ FaceClosest dist_candidate(float px, float py, float pz, float qx, float qy, float qz, const DistBox& k) {
  qx = dist_clamp(qx, k.lx, k.hx), qy = dist_clamp(qy, k.ly, k.hy), qz = dist_clamp(qz, k.lz, k.hz);
  const float dx = px - qx, dy = py - qy, dz = pz - qz;
  return {dist_dot(dx, dy, dz, dx, dy, dz), qx, qy, qz};
}

__device__ __forceinline__ FaceClosest dist_segment(float px, float py, float pz, float ax, float ay, float az, float bx, float by, float bz, const DistBox& k) {
  const float ex = bx - ax, ey = by - ay, ez = bz - az;
  const float wx = px - ax, wy = py - ay, wz = pz - az;
  const float l = dist_dot(ex, ey, ez, ex, ey, ez);
  float t = 0.0f;
  if (l > 0.0f) t = fminf(fmaxf(dist_dot(wx, wy, wz, ex, ey, ez) / l, 0.0f), 1.0f);
  return dist_candidate(px, py, pz, ax + t * ex, ay + t * ey, az + t * ez, k);
}

// dot((b - a) x (q - a), n)
__device__ __forceinline__ float dist_edge(float ax, float ay, float az, float bx, float by, float bz, float qx, float qy, float qz, float nx, float ny, float nz) {
  const float ex = bx - ax, ey = by - ay, ez = bz - az;
  const float rx = qx - ax, ry = qy - ay, rz = qz - az;
  return dist_dot(ey * rz - ez * ry, ez * rx - ex * rz, ex * ry - ey * rx, nx, ny, nz);
}

// THE rule: the closest point of triangle (a, b, c) to p and its squared distance
__device__ __forceinline__ FaceClosest closest_on_face(float px, float py, float pz, float ax, float ay, float az, float bx, float by, float bz, float cx, float cy,
                                                       float cz) {
  const DistBox k = {fminf(fminf(ax, bx), cx), fminf(fminf(ay, by), cy), fminf(fminf(az, bz), cz),
                     fmaxf(fmaxf(ax, bx), cx), fmaxf(fmaxf(ay, by), cy), fmaxf(fmaxf(az, bz), cz)};
  FaceClosest best = dist_segment(px, py, pz, ax, ay, az, bx, by, bz, k);
  FaceClosest c = dist_segment(px, py, pz, bx, by, bz, cx, cy, cz, k);
  if (c.d2 < best.d2) best = c;
  c = dist_segment(px, py, pz, cx, cy, cz, ax, ay, az, k);
  if (c.d2 < best.d2) best = c;
  const float ux = bx - ax, uy = by - ay, uz = bz - az;
  const float vx = cx - ax, vy = cy - ay, vz = cz - az;
  const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
  const float nn = dist_dot(nx, ny, nz, nx, ny, nz);
  if (nn > 0.0f) {
    const float s = dist_dot(px - ax, py - ay, pz - az, nx, ny, nz) / nn;
    const float qx = px - s * nx, qy = py - s * ny, qz = pz - s * nz;
    if (dist_edge(ax, ay, az, bx, by, bz, qx, qy, qz, nx, ny, nz) >= 0.0f && dist_edge(bx, by, bz, cx, cy, cz, qx, qy, qz, nx, ny, nz) >= 0.0f &&
        dist_edge(cx, cy, cz, ax, ay, az, qx, qy, qz, nx, ny, nz) >= 0.0f) {
      c = dist_candidate(px, py, pz, qx, qy, qz, k);
      if (c.d2 < best.d2) best = c;
    }
  }
  return best;
}

// the cell of a coordinate along one axis of n cells: floor(fl(fl(v - o) r)) clamped into [0, n - 1] (n <= 2^20 is exact in float32;
// NaN goes to 0).  Monotone in v: subtraction of a constant, multiplication by a positive constant, rounding and floor all are.
__device__ __forceinline__ int dist_cell(float v, float o, float r, int n) {
  const float t = floorf((v - o) * r);
  return (int)fminf(fmaxf(t, 0.0f), (float)(n - 1));
}

}  // namespace
