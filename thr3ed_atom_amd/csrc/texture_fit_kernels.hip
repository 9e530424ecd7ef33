// texture_fit_kernels.hip -- the mesh render as a linear map of the texture, and its adjoint (rf_texture_sample /
// rf_texture_sample_backward of relu_field.h): what thr3ed_atom_amd/texture_fit.py is built on.  DESIGN.md section 24 has the contract
// and the measurements, docs/texture_fit_errors.md the error bound, tests/texture_fit_model.py the float64 model.
//
// Forward.  One lane per pixel over the tap records of all views (rf_mesh_raster_taps of mesh_raster_kernels.hip): the fetch of the
// shade kernel through the same bilinear_blend of view_camera.h (top, bot, then the fy blend; the library is built with
// -ffp-contract=off), so the colour is render_mesh's bit for bit.  Nothing is rasterised again.
//
// Backward.  The transposed map in gather form: one segment of (pixel, weight) entries per texel, built once per sampler, summed by
// segment_sum of segment_sum.h.  A segment longer than the threshold -- a face of a coarse patch that fills the frame of many views
// puts 10^5 entries on one texel -- goes to the whole wavefront, as the visibility kernel hands over its large boxes.
#include "segment_sum.h"
#include "view_camera.h"

namespace {

constexpr int kFitBlock = 256;
constexpr int kLongSegment = 16;  // segments of more entries go to the wavefront (DESIGN.md section 24 has the A/B that chose it)
constexpr unsigned int kNoTap = 0xffffu;

__global__ __launch_bounds__(kFitBlock) void texture_sample_kernel(const RFTextureTap* __restrict__ taps, long long P, const float* __restrict__ texture, int Ht, int Wt,
                                                                   float background, float* __restrict__ colour, int* status) {
  const long long pix = (long long)blockIdx.x * kFitBlock + threadIdx.x;
  if (pix >= P) return;
  const RFTextureTap p = taps[pix];
  float rgb[3] = {background, background, background};
  if (p.x0 != kNoTap) {
    if ((int)p.x0 >= Wt || (int)p.x1 >= Wt || (int)p.y0 >= Ht || (int)p.y1 >= Ht) {
      *status = 1;  // (a plain store of one value: whichever lane wins, the word reads 1)
    } else {
      const float* r0 = texture + 3ll * ((long long)p.y0 * Wt);
      const float* r1 = texture + 3ll * ((long long)p.y1 * Wt);
      const int x0 = p.x0, x1 = p.x1;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) rgb[ch] = bilinear_blend(p, r0[3 * x0 + ch], r0[3 * x1 + ch], r1[3 * x0 + ch], r1[3 * x1 + ch]);
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) colour[3 * pix + ch] = rgb[ch];
}

// acc += weight * grad_colour[pixel] for one entry (an entry outside the pixels sets the status word and adds nothing)
__device__ __forceinline__ void add_entry(const RFTextureTapEntry& e, const float* __restrict__ grad_colour, long long P, float (&acc)[3], int* status) {
  if ((unsigned long long)(long long)e.pixel >= (unsigned long long)P) {
    *status = 1;
    return;
  }
  const float* g = grad_colour + 3ll * e.pixel;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) acc[ch] = acc[ch] + e.weight * g[ch];
}

// what segment_sum adds for entry e of the list
struct AddTapEntry {
  const RFTextureTapEntry* entries;
  const float* grad_colour;
  long long P;
  int* status;
  __device__ __forceinline__ void operator()(long long e, float (&acc)[3]) const { add_entry(entries[e], grad_colour, P, acc, status); }
};

__global__ __launch_bounds__(kFitBlock) void texture_sample_backward_kernel(const float* __restrict__ grad_colour, long long P, const long long* __restrict__ offsets,
                                                                            const RFTextureTapEntry* __restrict__ entries, long long E, long long texels,
                                                                            int long_segment, float* __restrict__ grad_texture, int* status) {
  segment_sum<3, kFitBlock>(offsets, E, texels, long_segment, grad_texture, AddTapEntry{entries, grad_colour, P, status});
}

}  // namespace

extern "C" {

int rf_texture_sample(const void* taps_dev, int64_t num_pixels, const float* texture_dev, int32_t texture_height, int32_t texture_width,
                      float background, uint32_t flags, float* colour_dev, int32_t* status_dev, void* stream) {
  if (!texture_dev || !status_dev) return RF_ERR_NULL_POINTER;
  if (num_pixels > 0 && (!taps_dev || !colour_dev)) return RF_ERR_NULL_POINTER;
  if (num_pixels < 0 || num_pixels >= (1ll << 31) || !image_shape_ok(texture_height, texture_width)) return RF_ERR_BAD_SHAPE;
  if (!std::isfinite(background) || !(background >= 0.0f)) return RF_ERR_BAD_SHAPE;
  if (flags) return RF_ERR_UNSUPPORTED;
  if (num_pixels == 0) return RF_OK;
  const dim3 blocks((unsigned)((num_pixels + kFitBlock - 1) / kFitBlock));  // < 2^23
  hipLaunchKernelGGL(texture_sample_kernel, blocks, dim3(kFitBlock), 0, (hipStream_t)stream, (const RFTextureTap*)taps_dev, (long long)num_pixels, texture_dev, texture_height,
                     texture_width, background, colour_dev, status_dev);
  return launch_status();
}

int rf_texture_sample_backward(const float* grad_colour_dev, int64_t num_pixels, const int64_t* offsets_dev, const void* entries_dev,
                               int64_t num_entries, int32_t texture_height, int32_t texture_width, int32_t long_segment, uint32_t flags,
                               float* grad_texture_dev, int32_t* status_dev, void* stream) {
  if (!offsets_dev || !grad_texture_dev || !status_dev) return RF_ERR_NULL_POINTER;
  if ((num_pixels > 0 && !grad_colour_dev) || (num_entries > 0 && !entries_dev)) return RF_ERR_NULL_POINTER;
  if (num_pixels < 0 || num_pixels >= (1ll << 31) || !image_shape_ok(texture_height, texture_width)) return RF_ERR_BAD_SHAPE;
  if (num_entries < 0 || num_entries >= (1ll << 33) || long_segment < 0) return RF_ERR_BAD_SHAPE;
  if (flags) return RF_ERR_UNSUPPORTED;
  const long long texels = (long long)texture_height * texture_width;  // <= 2^28
  const dim3 blocks((unsigned)((texels + kFitBlock - 1) / kFitBlock));
  hipLaunchKernelGGL(texture_sample_backward_kernel, blocks, dim3(kFitBlock), 0, (hipStream_t)stream, grad_colour_dev, (long long)num_pixels,
                     (const long long*)offsets_dev, (const RFTextureTapEntry*)entries_dev, (long long)num_entries, texels, long_segment ? long_segment : kLongSegment, grad_texture_dev,
                     status_dev);
  return launch_status();
}

}  // extern "C"
