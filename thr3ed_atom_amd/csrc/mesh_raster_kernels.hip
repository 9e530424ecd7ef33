// mesh_raster_kernels.hip -- a rasteriser for exported triangle meshes (rf_mesh_raster_visibility / rf_mesh_raster_shade /
// rf_mesh_raster_taps of relu_field.h): what thr3ed_atom_amd/mesh_raster.py is built on.  DESIGN.md section 22 has the contract,
// docs/mesh_raster_errors.md the error bound, tests/mesh_raster_model.py the float64 model.  The ray, the watertight edge values, the
// coverage rule and the depth are the device functions of mesh_raster.h, which csrc/mesh_fit_kernels.hip
// includes too.  A face with any z_k < near is not drawn at all (the documented rule; not a clip).
//
// The visibility pass.  One uint64 per pixel, float_bits(z) << 32 | face, all ones = nothing; device-scope 64-bit atomicMin without
// a return value.  z >= 0, so its bits order like the number; the minimum does not depend on the order of arrival and the lower
// face index wins exact ties: two runs give the same bits.  A relaxed pre-read skips the atomic when the stored key is already
// smaller (the key only ever decreases).  Each lane sets up ONE face: bounds check (a bad face sets the status word and is skipped,
// never dereferenced), corners, depth rule, the conservative pixel box of the three projected corners clipped to the image.  A box
// of at most 8 x 8 pixels is walked by its own lane.  Larger boxes are handed to the whole wavefront one after another by ballot;
// its 64 lanes cover the box in blocks of 8 x 8 pixels.  No LDS, no barrier, no workgroup waits for another.  A face is only ever
// tested inside its box: a zero-area sliver whose edge values are rounding noise can be drawn at a pixel of its own projection, never
// across the frame.
//
// The shade pass.  One lane per pixel, no atomics: decode the key, re-evaluate e, w, z of the winning face with the SAME device
// functions (the same bits), write depth, face_ids, optionally the barycentrics, and the colour: a bilinear fetch of the bake's
// texture at the interpolated per-corner UVs (texel coordinates (u W_t - 1/2, (1 - v) H_t - 1/2), taps clamped to the image), or
// sum_k w_k colour_k of the vertex colours.  Pixels without a hit get the background, depth 0 and face id -1.
//
// The taps pass (rf_mesh_raster_taps).  One lane per pixel, the shade pass up to its fetch: winning_hit and
// texel_taps of mesh_raster.h are the two device functions both kernels call, so a tap record holds the bits the shade kernel
// fetches through.  thr3ed_atom_amd/texture_fit.py turns the records of many views into the sparse matrix whose adjoint
// csrc/texture_fit_kernels.hip sums.
#include "mesh_raster.h"

namespace {

// The conservative pixel box [j0, j1] x [i0, i1] of a face whose corners all have z_k >= near >= 0: the projected corners, widened by
// a bound on the float32 error of the projection plus one pixel, clipped to the image.  A corner whose depth is not safely positive
// (or anything not finite) gives the whole image: conservative is all the box has to be, the coverage rule decides.
__device__ __forceinline__ void raster_box(const RasterCamera& cam, const float (&v)[3][3], int& j0, int& j1, int& i0, int& i1) {
  float xlo = 3.0e38f, xhi = -3.0e38f, ylo = 3.0e38f, yhi = -3.0e38f;
  bool whole = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float p[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) p[x] = v[k][x] - cam.t[x];
    const float xc = (p[0] * cam.R[0] + p[1] * cam.R[3]) + p[2] * cam.R[6];
    const float yc = (p[0] * cam.R[1] + p[1] * cam.R[4]) + p[2] * cam.R[7];
    const float zc = -((p[0] * cam.R[2] + p[1] * cam.R[5]) + p[2] * cam.R[8]);
    const float mag = (fabsf(p[0]) + fabsf(p[1])) + fabsf(p[2]);
    const float rmax = fmaxf(fmaxf(fmaxf(fabsf(cam.R[0]), fabsf(cam.R[1])), fmaxf(fabsf(cam.R[2]), fabsf(cam.R[3]))),
                             fmaxf(fmaxf(fabsf(cam.R[4]), fabsf(cam.R[5])), fmaxf(fmaxf(fabsf(cam.R[6]), fabsf(cam.R[7])), fabsf(cam.R[8]))));
    const float del = 1.0e-6f * mag * rmax;  // > 4 ulp of every term of xc, yc, zc
    if (!(zc - del > 0.0f)) {
      whole = true;
      continue;
    }
    const float inv = 1.0f / (zc - del);
    const float x = cam.focal * xc / zc + (float)cam.W * 0.5f - 0.5f;
    const float y = (float)cam.H * 0.5f - 0.5f - cam.focal * yc / zc;
    const float ex = cam.focal * inv * (del + fabsf(xc) * inv * del) * 2.0f + 1.0e-6f * (fabsf(x) + (float)cam.W) + 1.0f;
    const float ey = cam.focal * inv * (del + fabsf(yc) * inv * del) * 2.0f + 1.0e-6f * (fabsf(y) + (float)cam.H) + 1.0f;
    if (!(fabsf(x) + ex < 1.0e9f) || !(fabsf(y) + ey < 1.0e9f)) {
      whole = true;
      continue;
    }
    xlo = fminf(xlo, x - ex), xhi = fmaxf(xhi, x + ex);
    ylo = fminf(ylo, y - ey), yhi = fmaxf(yhi, y + ey);
  }
  if (whole) {
    j0 = 0, j1 = cam.W - 1, i0 = 0, i1 = cam.H - 1;
    return;
  }
  // (clamped as floats first: every value that is converted lies in [-1, edge])
  j0 = (int)ceilf(fminf(fmaxf(xlo, 0.0f), (float)cam.W));
  j1 = (int)floorf(fminf(fmaxf(xhi, -1.0f), (float)(cam.W - 1)));
  i0 = (int)ceilf(fminf(fmaxf(ylo, 0.0f), (float)cam.H));
  i1 = (int)floorf(fminf(fmaxf(yhi, -1.0f), (float)(cam.H - 1)));
}

__device__ __forceinline__ void raster_pixel(const RasterCamera& cam, const RasterFace& f, int i, int j, int cull, unsigned int face,
                                             unsigned long long* vis) {
  const RasterHit h = raster_hit(cam, f, i, j, cull);
  if (!h.hit) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(h.z) << 32) | (unsigned long long)face;
  unsigned long long* slot = vis + ((long long)i * cam.W + j);
  if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= key) return;  // the key only ever decreases
  (void)__hip_atomic_fetch_min(slot, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ float shfl_f(float x, int src) { return __shfl(x, src, 64); }

__global__ __launch_bounds__(kRasterBlock) void mesh_raster_visibility_kernel(RasterArgs a, unsigned long long* vis, int* status) {
  const long long t = (long long)blockIdx.x * kRasterBlock + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63);
  // (no lane returns early: the ballot loop below needs the whole wavefront)
  RasterFace f;
  int j0 = 0, j1 = -1, i0 = 0, i1 = -1;
  bool live = t < a.num_faces;
  if (live) {
    unsigned long long vi[3];
    float v[3][3];
    live = load_face(a, t, vi, v, status);
    if (live) {
      f = raster_face(a.cam, vi, v);
      live = !(f.zk[0] < a.near) && !(f.zk[1] < a.near) && !(f.zk[2] < a.near);
      if (live) {
        raster_box(a.cam, v, j0, j1, i0, i1);
        live = j0 <= j1 && i0 <= i1;
      }
    }
  }
  const bool small = live && (j1 - j0) < kLaneBox && (i1 - i0) < kLaneBox;
  if (small) {
    for (int i = i0; i <= i1; ++i)
      for (int j = j0; j <= j1; ++j) raster_pixel(a.cam, f, i, j, a.cull, (unsigned int)t, vis);
  }
  unsigned long long todo = __ballot(live && !small);
  while (todo) {  // (wave-uniform)
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    RasterFace g;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
      for (int x = 0; x < 3; ++x) g.c[k][x] = shfl_f(f.c[k][x], src);
      g.flip[k] = __shfl((int)f.flip[k], src, 64) != 0;
      g.zk[k] = shfl_f(f.zk[k], src);
    }
    const int bj0 = __shfl(j0, src, 64), bj1 = __shfl(j1, src, 64), bi0 = __shfl(i0, src, 64), bi1 = __shfl(i1, src, 64);
    const unsigned int face = (unsigned int)(t - lane + src);
    for (int bi = bi0; bi <= bi1; bi += kLaneBox)
      for (int bj = bj0; bj <= bj1; bj += kLaneBox) {
        const int i = bi + (lane >> 3), j = bj + (lane & 7);
        if (i <= bi1 && j <= bj1) raster_pixel(a.cam, g, i, j, a.cull, face, vis);
      }
  }
}

struct ShadeArgs {
  const unsigned long long* vis;
  const float* uvs;      // [T, 3, 2] or nullptr
  const float* texture;  // [Ht, Wt, 3] or nullptr
  int Ht, Wt;
  const float* colours;  // [V, 3] or nullptr
  float background;
  float* colour;  // or nullptr
  float* depth;
  int* face_ids;
  float* bary;  // or nullptr
};

__global__ __launch_bounds__(kRasterBlock) void mesh_raster_shade_kernel(RasterArgs a, ShadeArgs s) {
  const long long pix = (long long)blockIdx.x * kRasterBlock + threadIdx.x;
  if (pix >= (long long)a.cam.H * a.cam.W) return;
  const int i = (int)(pix / a.cam.W), j = (int)(pix - (long long)i * a.cam.W);
  float rgb[3] = {s.background, s.background, s.background}, w[3] = {0.0f, 0.0f, 0.0f}, z = 0.0f;
  int id = -1;
  long long t;
  unsigned long long vi[3];
  RasterHit h;
  if (winning_hit(a, s.vis[pix], i, j, t, vi, h)) {
    id = (int)t, z = h.z;
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = h.w[k];
    if (s.colour && s.texture) {
      const BilinearTaps p = texel_taps(s.uvs + 6 * t, w, s.Ht, s.Wt);
      const float* r0 = s.texture + 3ll * ((long long)p.y0 * s.Wt);
      const float* r1 = s.texture + 3ll * ((long long)p.y1 * s.Wt);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) rgb[ch] = bilinear_blend(p, r0[3 * p.x0 + ch], r0[3 * p.x1 + ch], r1[3 * p.x0 + ch], r1[3 * p.x1 + ch]);
    } else if (s.colour && s.colours) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        rgb[ch] = (w[0] * s.colours[3 * vi[0] + ch] + w[1] * s.colours[3 * vi[1] + ch]) + w[2] * s.colours[3 * vi[2] + ch];
    }
  }
  s.depth[pix] = z;
  s.face_ids[pix] = id;
  if (s.colour) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) s.colour[3 * pix + ch] = rgb[ch];
  }
  if (s.bary) {
#pragma unroll
    for (int k = 0; k < 3; ++k) s.bary[3 * pix + k] = w[k];
  }
}

// one record per pixel: what the shade kernel computes before its fetch (x0 = 0xffff: no hit; texture edges are at most 16384)
__global__ __launch_bounds__(kRasterBlock) void mesh_raster_taps_kernel(RasterArgs a, const unsigned long long* vis, const float* uvs, int Ht, int Wt, RFTextureTap* taps) {
  const long long pix = (long long)blockIdx.x * kRasterBlock + threadIdx.x;
  if (pix >= (long long)a.cam.H * a.cam.W) return;
  const int i = (int)(pix / a.cam.W), j = (int)(pix - (long long)i * a.cam.W);
  RFTextureTap rec;
  rec.x0 = rec.x1 = rec.y0 = rec.y1 = 0xffffu;
  rec.fx = rec.fy = 0.0f;
  long long t;
  unsigned long long vi[3];
  RasterHit h;
  if (winning_hit(a, vis[pix], i, j, t, vi, h)) {
    const BilinearTaps p = texel_taps(uvs + 6 * t, h.w, Ht, Wt);
    rec.x0 = (uint16_t)p.x0, rec.x1 = (uint16_t)p.x1, rec.y0 = (uint16_t)p.y0, rec.y1 = (uint16_t)p.y1;
    rec.fx = p.fx, rec.fy = p.fy;
  }
  taps[pix] = rec;
}

}  // namespace

extern "C" {

int rf_mesh_raster_visibility(const RFCamera* camera, const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces,
                              float near, uint32_t flags, uint64_t* visibility_dev, int32_t* status_dev, void* stream) {
  if (!camera || !visibility_dev || !status_dev) return RF_ERR_NULL_POINTER;
  if ((num_vertices > 0 && !vertices_dev) || (num_faces > 0 && !faces_dev)) return RF_ERR_NULL_POINTER;
  const int rc = check_raster(camera, num_vertices, num_faces, near, flags);
  if (rc != RF_OK) return rc;
  if (num_faces == 0) return RF_OK;
  const RasterArgs a = raster_args(camera, vertices_dev, num_vertices, faces_dev, num_faces, near, flags);
  const dim3 blocks((unsigned)((num_faces + kRasterBlock - 1) / kRasterBlock));  // < 2^23
  hipLaunchKernelGGL(mesh_raster_visibility_kernel, blocks, dim3(kRasterBlock), 0, (hipStream_t)stream, a, (unsigned long long*)visibility_dev, status_dev);
  return launch_status();
}

int rf_mesh_raster_shade(const RFCamera* camera, const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces,
                         const uint64_t* visibility_dev, const float* uvs_dev, const float* texture_dev, int32_t texture_height, int32_t texture_width,
                         const float* colours_dev, uint32_t flags, float* colour_dev, float* depth_dev, int32_t* face_ids_dev, float* barycentrics_dev,
                         void* stream) {
  if (!camera || !visibility_dev || !depth_dev || !face_ids_dev) return RF_ERR_NULL_POINTER;
  if ((num_vertices > 0 && !vertices_dev) || (num_faces > 0 && !faces_dev)) return RF_ERR_NULL_POINTER;
  if ((uvs_dev == nullptr) != (texture_dev == nullptr)) return RF_ERR_NULL_POINTER;  // the bake's two halves come together
  if (colour_dev && !texture_dev && !colours_dev) return RF_ERR_NULL_POINTER;        // a colour image needs a source
  const int rc = check_raster(camera, num_vertices, num_faces, 0.0f, 0u);
  if (rc != RF_OK) return rc;
  if (texture_dev && !image_shape_ok(texture_height, texture_width)) return RF_ERR_BAD_SHAPE;
  if (flags & ~(uint32_t)(RF_FLAG_WHITE_BKGD | RF_RASTER_CULL_BACKFACES)) return RF_ERR_UNSUPPORTED;
  const RasterArgs a = raster_args(camera, vertices_dev, num_vertices, faces_dev, num_faces, 0.0f, flags);
  ShadeArgs s;
  s.vis = (const unsigned long long*)visibility_dev;
  s.uvs = uvs_dev, s.texture = texture_dev, s.Ht = texture_height, s.Wt = texture_width;
  s.colours = colours_dev;
  s.background = (flags & RF_FLAG_WHITE_BKGD) ? 1.0f : 0.0f;
  s.colour = colour_dev, s.depth = depth_dev, s.face_ids = face_ids_dev, s.bary = barycentrics_dev;
  const long long total = (long long)camera->height * camera->width;  // <= 2^28
  hipLaunchKernelGGL(mesh_raster_shade_kernel, dim3((unsigned)((total + kRasterBlock - 1) / kRasterBlock)), dim3(kRasterBlock), 0, (hipStream_t)stream, a, s);
  return launch_status();
}

int rf_mesh_raster_taps(const RFCamera* camera, const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces,
                        const uint64_t* visibility_dev, const float* uvs_dev, int32_t texture_height, int32_t texture_width, uint32_t flags,
                        void* taps_dev, void* stream) {
  if (!camera || !visibility_dev || !taps_dev) return RF_ERR_NULL_POINTER;
  if ((num_vertices > 0 && !vertices_dev) || (num_faces > 0 && (!faces_dev || !uvs_dev))) return RF_ERR_NULL_POINTER;
  const int rc = check_raster(camera, num_vertices, num_faces, 0.0f, 0u);
  if (rc != RF_OK) return rc;
  if (!image_shape_ok(texture_height, texture_width)) return RF_ERR_BAD_SHAPE;
  if (flags & ~(uint32_t)(RF_FLAG_WHITE_BKGD | RF_RASTER_CULL_BACKFACES)) return RF_ERR_UNSUPPORTED;
  const RasterArgs a = raster_args(camera, vertices_dev, num_vertices, faces_dev, num_faces, 0.0f, flags);
  const long long total = (long long)camera->height * camera->width;  // <= 2^28
  hipLaunchKernelGGL(mesh_raster_taps_kernel, dim3((unsigned)((total + kRasterBlock - 1) / kRasterBlock)), dim3(kRasterBlock), 0, (hipStream_t)stream, a,
                     (const unsigned long long*)visibility_dev, uvs_dev, texture_height, texture_width, (RFTextureTap*)taps_dev);
  return launch_status();
}

}  // extern "C"
