// texture_atlas.h -- the per-triangle atlas that texture_kernels.hip (rf_texture_bake) and texture_views_kernels.hip
// (rf_texture_project_views) share: lane -> texel -> block -> face -> beta -> point p and unit normal n.  The top of texture_kernels.hip
// describes the layout, tests/texture_model.py restates it.  The float32 operations and their order are part of the contract of both
// entry points (the library is built with -ffp-contract=off): both units see the same p and n bit for bit.
#pragma once

#include "rf_device.h"

namespace {

struct AtlasTexel {
  long long pixel;  // row-major index of the texel in the image
  long long tri;    // the face that owns it when tri < num_faces
  int i, j;         // column and row inside the block
  bool upper;
};

// lane t of a block-major launch (lane order inside a block: j B + i); the caller has checked t < cols B rows B
__device__ __forceinline__ AtlasTexel atlas_texel(long long t, int P, int B, int cols) {
  AtlasTexel x;
  const long long width = (long long)cols * B;
  const int bb = B * B;
  const long long blk = t / bb;
  const int r = (int)(t - blk * bb);
  x.j = r / B, x.i = r - x.j * B;
  const long long br = blk / cols, bc = blk - br * cols;
  const long long col = bc * B + x.i, row = br * B + x.j;
  x.pixel = row * width + col;
  x.upper = x.i + x.j > P + 3;
  x.tri = 2 * blk + (x.upper ? 1 : 0);
  return x;
}

// the three vertex indices of face tri: false when one lies outside [0, num_vertices) (the caller sets the status word; the index is
// never used as an address)
__device__ __forceinline__ bool atlas_face(const long long* faces, long long num_vertices, long long tri, unsigned long long (&vi)[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) vi[c] = (unsigned long long)faces[3 * tri + c];
  return !(vi[0] >= (unsigned long long)num_vertices || vi[1] >= (unsigned long long)num_vertices || vi[2] >= (unsigned long long)num_vertices);
}

// p = (beta0 v0 + beta1 v1) + beta2 v2 of the texel and n = the unit normal (v1 - v0) x (v2 - v0), 0 for a zero-area face
__device__ __forceinline__ void atlas_point(const float* vertices, const unsigned long long (&vi)[3], int P, const AtlasTexel& x, float (&p)[3], float (&n)[3]) {
  float v[3][3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int a = 0; a < 3; ++a) v[c][a] = vertices[3 * vi[c] + a];
  const float legs = (float)(P - 1);
  const float b1 = (float)(x.upper ? P + 2 - x.i : x.i - 1) / legs, b2 = (float)(x.upper ? P + 2 - x.j : x.j - 1) / legs;
  const float b0 = (1.0f - b1) - b2;
  float e1[3], e2[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    p[a] = (b0 * v[0][a] + b1 * v[1][a]) + b2 * v[2][a];
    e1[a] = v[1][a] - v[0][a];
    e2[a] = v[2][a] - v[0][a];
  }
  n[0] = e1[1] * e2[2] - e1[2] * e2[1], n[1] = e1[2] * e2[0] - e1[0] * e2[2], n[2] = e1[0] * e2[1] - e1[1] * e2[0];
  const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
#pragma unroll
  for (int a = 0; a < 3; ++a) n[a] = (len > 0.0f) ? n[a] / len : 0.0f;
}

}  // namespace
