// view_camera.h -- what the units that look through an RFCamera share: the limits, the host checks of a camera and of an image
// shape, the by-value camera array of the view-loop kernels (texture_views_kernels.hip, fusion_kernels.hip) and the bilinear fetch
// (mesh_raster_kernels.hip, texture_fit_kernels.hip, texture_views_kernels.hip).  The float32 operations and their order are part of
// the contract of every entry point that goes through them (the library is built with -ffp-contract=off): units that call the same
// function here see the same bits.
#pragma once

#include "rf_device.h"

namespace {

constexpr int kMaxImageEdge = 16384;            // images, textures and atlases: at most this many pixels along an edge
constexpr int kMaxViews = 16;                   // cameras per call of a view-loop kernel
constexpr unsigned long long kNoHit = ~0ull;    // the visibility key of a pixel that nothing covers

inline bool image_shape_ok(int32_t height, int32_t width) { return height >= 1 && height <= kMaxImageEdge && width >= 1 && width <= kMaxImageEdge; }

inline bool camera_ok(const RFCamera& cam) {
  if (!image_shape_ok(cam.height, cam.width) || !std::isfinite(cam.focal) || !(cam.focal > 0.0f)) return false;
  for (int e = 0; e < 12; ++e)
    if (!std::isfinite(cam.pose[e])) return false;
  return true;
}

// n cameras of one image size (none is fine)
inline bool view_cameras_ok(const RFCamera* cameras, int n) {
  for (int k = 0; k < n; ++k)
    if (!camera_ok(cameras[k]) || cameras[k].height != cameras[0].height || cameras[k].width != cameras[0].width) return false;
  return true;
}

// the cameras of a view-loop kernel travel by value in its argument struct (the tail is never read; it is not left uninitialised)
inline void fill_view_cameras(RFCamera (&cams)[kMaxViews], const RFCamera* cameras, int n) {
  for (int k = 0; k < kMaxViews; ++k) cams[k] = cameras[k < n ? k : 0];
}

// the four taps and the two weights of a bilinear fetch at (x, y) of an H x W image, taps clamped to the image: the ONLY place they
// are computed
struct BilinearTaps {
  int x0, x1, y0, y1;
  float fx, fy;
};

__device__ __forceinline__ BilinearTaps bilinear_taps(float x, float y, int H, int W) {
  BilinearTaps s;
  const float xf = floorf(x), yf = floorf(y);
  s.fx = x - xf, s.fy = y - yf;
  // (clamped as floats first, so that the conversion is defined for every value; NaN goes to 0)
  s.x0 = (int)fminf(fmaxf(xf, 0.0f), (float)(W - 1)), s.x1 = (int)fminf(fmaxf(xf + 1.0f, 0.0f), (float)(W - 1));
  s.y0 = (int)fminf(fmaxf(yf, 0.0f), (float)(H - 1)), s.y1 = (int)fminf(fmaxf(yf + 1.0f, 0.0f), (float)(H - 1));
  return s;
}

// top, bot, then the fy blend of the four fetched values; Taps has the weights fx and fy (BilinearTaps, or the RFTextureTap record,
// by value: texture_sample_kernel's code is then what it was with the blend written out)
template <typename Taps>
__device__ __forceinline__ float bilinear_blend(const Taps s, float a00, float a01, float a10, float a11) {
  const float top = (1.0f - s.fx) * a00 + s.fx * a01;
  const float bot = (1.0f - s.fx) * a10 + s.fx * a11;
  return (1.0f - s.fy) * top + s.fy * bot;
}

}  // namespace
