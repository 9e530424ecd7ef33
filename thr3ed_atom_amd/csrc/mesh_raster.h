// mesh_raster.h -- the rasteriser's device functions and host checks, shared by mesh_raster_kernels.hip (visibility, shade, taps) and
// mesh_fit_kernels.hip (coverage and the geometry gradients).  DESIGN.md section 22 has the contract, tests/mesh_raster_model.py the
// float64 model.  The float32 operations and their order are part of the contract of every entry point of both units (the library is
// built with -ffp-contract=off): both see the same e, s, w and z bit for bit.
//
// The ray.  Pixel (i, j) has exactly the ray cast_rays gives it: o = t, d = pixel_ray(i, j) of rf_device.h (the same float32
// operations in the same order).  With p_k = v_k - o the edge values of the ray are the triple products e0 = d . (p1 x p2),
// e1 = d . (p2 x p0), e2 = d . (p0 x p1); s = (e0 + e1) + e2 = d . ((v1 - v0) x (v2 - v0)) up to rounding.
//
// Watertight edges.  Every component of a cross product is ONE subtraction of two products and the library is built with
// -ffp-contract=off, so p_a x p_b = -(p_b x p_a) holds bit for bit, and so does the dot product with d.  The kernels do not lean on
// the compiler keeping that symmetry through two differently ordered call sites: every edge is evaluated from its LOWER to its
// HIGHER vertex index and the sign is flipped afterwards when the face runs the other way.  Two faces that share an edge therefore
// see e and -e, never e and -e(1 + ulp): a ray is on the inner side of exactly one of them, or exactly on the edge of both -- no
// crack, no double cover away from the edge, and no fill-rule table.
//
// Coverage.  A ray hits when all three e are >= 0 or all three are <= 0, and s != 0 (edges inclusive; zero-area and edge-on faces
// have s == 0 and are never drawn).  Mesh.faces has (v1 - v0) x (v2 - v0) pointing OUT of the solid, so a face seen from outside has
// s < 0: under RF_RASTER_CULL_BACKFACES only s < 0 counts.  w_k = e_k / s.  z_k = the camera depth of corner k, the component of p_k
// along -R[:, 2]; z = z0 + (w1 (z1 - z0) + w2 (z2 - z0)) -- sum_k w_k z_k anchored at corner 0, so that a face at one camera depth has
// that depth exactly -- is the ray parameter of the hit, the quantity RenderOut.depth holds.
#pragma once

#include "rf_device.h"
#include "view_camera.h"

namespace {

constexpr int kRasterBlock = 256;
constexpr int kLaneBox = 8;  // boxes of at most kLaneBox x kLaneBox pixels stay on their lane; the wave path walks blocks of this edge

struct RasterCamera {
  int H, W;
  float focal;
  float R[9], t[3];
};

struct RasterArgs {
  RasterCamera cam;
  const float* vertices;
  const long long* faces;
  long long num_vertices, num_faces;
  float near;
  int cull;
};

// one face as a ray sees it: c[k] = the cross product of edge k's corners taken from the lower to the higher vertex index, flip[k]
// whether the face runs along that edge the other way; zk[k] the camera depths
struct RasterFace {
  float c[3][3];
  bool flip[3];
  float zk[3];
};

__device__ __forceinline__ void cross3(const float* a, const float* b, float* out) {
  out[0] = a[1] * b[2] - a[2] * b[1];
  out[1] = a[2] * b[0] - a[0] * b[2];
  out[2] = a[0] * b[1] - a[1] * b[0];
}

// vi: the three vertex indices (checked by the caller), v: their positions
__device__ __forceinline__ RasterFace raster_face(const RasterCamera& cam, const unsigned long long (&vi)[3], const float (&v)[3][3]) {
  RasterFace f;
  float p[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int x = 0; x < 3; ++x) p[k][x] = v[k][x] - cam.t[x];
    f.zk[k] = -((p[k][0] * cam.R[2] + p[k][1] * cam.R[5]) + p[k][2] * cam.R[8]);
  }
  // edge k runs from corner (k + 1) % 3 to corner (k + 2) % 3; evaluated from the lower to the higher vertex index (see the top)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int a = (k + 1) % 3, b = (k + 2) % 3;
    f.flip[k] = vi[a] > vi[b];
    if (f.flip[k])
      cross3(p[b], p[a], f.c[k]);
    else
      cross3(p[a], p[b], f.c[k]);
  }
  return f;
}

struct RasterHit {
  bool hit;
  float w[3], z;
};

// the edge values e_k of pixel (i, j) on one face and their sum s = (e0 + e1) + e2: the ONLY place they are computed
__device__ __forceinline__ float raster_edges(const RasterCamera& cam, const RasterFace& f, int i, int j, float (&e)[3]) {
  float d[3];
  pixel_ray(i, j, cam.H, cam.W, cam.focal, cam.R, d);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float t = (f.c[k][0] * d[0] + f.c[k][1] * d[1]) + f.c[k][2] * d[2];
    e[k] = f.flip[k] ? -t : t;
  }
  return (e[0] + e[1]) + e[2];
}

// the coverage rule, the barycentrics and the depth of pixel (i, j) on one face: the ONLY place they are computed
__device__ __forceinline__ RasterHit raster_hit(const RasterCamera& cam, const RasterFace& f, int i, int j, int cull) {
  float e[3];
  const float s = raster_edges(cam, f, i, j, e);
  const bool neg = e[0] <= 0.0f && e[1] <= 0.0f && e[2] <= 0.0f, pos = e[0] >= 0.0f && e[1] >= 0.0f && e[2] >= 0.0f;
  RasterHit h;
  h.hit = (neg || (pos && !cull)) && s != 0.0f;
#pragma unroll
  for (int k = 0; k < 3; ++k) h.w[k] = e[k] / s;
  h.z = f.zk[0] + (h.w[1] * (f.zk[1] - f.zk[0]) + h.w[2] * (f.zk[2] - f.zk[0]));
  h.hit = h.hit && h.z >= 0.0f && h.z <= 3.0e38f;  // (a depth whose bits would not order like the number is no hit; NaN fails both)
  return h;
}

// loads face t: false (and the status word set) when it indexes outside the vertices
__device__ __forceinline__ bool load_face(const RasterArgs& a, long long t, unsigned long long (&vi)[3], float (&v)[3][3], int* status) {
#pragma unroll
  for (int c = 0; c < 3; ++c) vi[c] = (unsigned long long)a.faces[3 * t + c];
  const unsigned long long V = (unsigned long long)a.num_vertices;
  if (vi[0] >= V || vi[1] >= V || vi[2] >= V) {
    if (status) *status = 1;  // (a plain store of one value: whichever lane wins, the word reads 1)
    return false;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int x = 0; x < 3; ++x) v[c][x] = a.vertices[3 * vi[c] + x];
  return true;
}

// the face index t a visibility key names: false when nothing was hit or the key names no face of this mesh (the shade pass then gives
// the face id -1)
__device__ __forceinline__ bool winning_key(const RasterArgs& a, unsigned long long key, long long& t) {
  t = (long long)(key & 0xffffffffull);
  return !(key == kNoHit || t >= a.num_faces);
}

// the winning face of a pixel as the visibility buffer recorded it: false when nothing was hit (or the key names no face of this
// mesh); else t, vi and the hit re-evaluated with the device functions of the visibility pass (the same bits)
__device__ __forceinline__ bool winning_hit(const RasterArgs& a, unsigned long long key, int i, int j, long long& t, unsigned long long (&vi)[3], RasterHit& h) {
  if (!winning_key(a, key, t)) return false;
  float v[3][3];
  if (!load_face(a, t, vi, v, nullptr)) return false;
  h = raster_hit(a.cam, raster_face(a.cam, vi, v), i, j, a.cull);
  return true;
}

// the four taps of the bilinear fetch at the interpolated UVs of a hit, texel coordinates (u W_t - 1/2, (1 - v) H_t - 1/2): the ONLY
// place they are computed (the shade kernel fetches through them, the taps kernel records them)
__device__ __forceinline__ BilinearTaps texel_taps(const float* uv, const float (&w)[3], int Ht, int Wt) {
  const float u = (w[0] * uv[0] + w[1] * uv[2]) + w[2] * uv[4];
  const float vv = (w[0] * uv[1] + w[1] * uv[3]) + w[2] * uv[5];
  return bilinear_taps(u * (float)Wt - 0.5f, (1.0f - vv) * (float)Ht - 0.5f, Ht, Wt);
}

// the checks the entry points of both units share, after their pointer checks: RF_ERR_BAD_SHAPE, then RF_ERR_UNSUPPORTED
inline int check_raster(const RFCamera* cam, int64_t num_vertices, int64_t num_faces, float near, uint32_t flags) {
  if (num_vertices < 0 || num_faces < 0 || num_faces >= (1ll << 31)) return RF_ERR_BAD_SHAPE;
  if (!camera_ok(*cam)) return RF_ERR_BAD_SHAPE;
  if (!std::isfinite(near) || !(near >= 0.0f)) return RF_ERR_BAD_SHAPE;
  if (flags & ~(uint32_t)(RF_FLAG_WHITE_BKGD | RF_RASTER_CULL_BACKFACES)) return RF_ERR_UNSUPPORTED;
  return RF_OK;
}

inline RasterArgs raster_args(const RFCamera* cam, const float* vertices, int64_t num_vertices, const int64_t* faces, int64_t num_faces, float near, uint32_t flags) {
  RasterArgs a;
  a.cam.H = cam->height, a.cam.W = cam->width, a.cam.focal = cam->focal;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) a.cam.R[3 * r + c] = cam->pose[4 * r + c];
    a.cam.t[r] = cam->pose[4 * r + 3];
  }
  a.vertices = vertices, a.faces = (const long long*)faces;
  a.num_vertices = num_vertices, a.num_faces = num_faces;
  a.near = near, a.cull = (flags & RF_RASTER_CULL_BACKFACES) ? 1 : 0;
  return a;
}

}  // namespace
