// image_kernels.hip -- SSIM of two images and its adjoint (rf_ssim_tiles / rf_ssim_forward / rf_ssim_backward of relu_field.h).
//
// Contract: Wang et al. 2004 per colour channel on float32 images of data range 1,
//   window   Gaussian 11 x 11, sigma 1.5, separable: g_k ~ exp(-(k - 5)^2 / (2 * 1.5^2)), normalised to sum 1 in double, rounded once;
//   moments  mu_x = G*x, mu_y = G*y, s_xx = G*x^2 - mu_x^2, s_yy = G*y^2 - mu_y^2, s_xy = G*xy - mu_x mu_y -- NO clamping of variances;
//   S        = (A1 * A2) / (B1 * B2), A1 = 2 mu_x mu_y + C1, A2 = 2 s_xy + C2, B1 = mu_x^2 + mu_y^2 + C1, B2 = s_xx + s_yy + C2,
//            C1 = 0.01^2, C2 = 0.03^2, in exactly this association: for y == x numerator and denominator are the same float, S == 1;
//   padding  RF_SSIM_VALID: only windows inside the image, map [H - 10, W - 10]; RF_SSIM_SAME: the image zero-padded by 5, map [H, W];
//   result   the mean of the map over pixels and channels.
//
// Decomposition.  A workgroup of 256 threads owns one 16 x 32 tile of ONE channel's map.  It stages the tile plus its halo (26 x 42
// pixels) of both images in LDS once -- the loader writes the zeros of the padding, and of everything else outside the image --,
// filters the five products (x, y, x^2, y^2, xy) along the rows into LDS (26 x 32 each) and then down the columns out of LDS.  Rows of
// 42 / 32 floats with consecutive lanes on consecutive columns: every LDS access of a wave is two runs of 32 consecutive words, one
// per 32-lane half -- conflict-free on the 32-bank ds_read_b32 / ds_write_b32 path without padding.  Every filter sum is a chain
// acc = fmaf(g_k, v_k, acc), k = 0 .. 10: a fixed order, so 23 roundings lie on the longest path of a second moment (1 product,
// 11 + 11 chain steps); this is where the kappa of the error bound comes from.  The tile's sum is reduced in a fixed order (two values
// per thread, a butterfly across the wave, the four waves in order) into one partial per workgroup; a second launch of ONE workgroup
// adds the partials in float64, again in a fixed order.  No atomics anywhere: map, mean and gradient are bitwise reproducible.
//
// The adjoint reads three derivative maps the forward wrote when asked to (d_mu = the TOTAL derivative of S with respect to mu_x,
// d_sxx = dS / d s_xx, d_sxy = dS / d s_xy) and gathers, per image pixel p,
//   dL/dx_p = (g / N) * [ (G*d_mu)_p + 2 x_p (G*d_sxx)_p + y_p (G*d_sxy)_p ]      (derivative maps are 0 outside the map's extent)
// with the same staging / row pass / column pass.  g is read from device memory by the kernel.
#include "rf_device.h"

namespace {

constexpr int kWin = 11;                    // window taps per axis
constexpr int kTileH = 16, kTileW = 32;     // map pixels per workgroup (rf_ssim_tiles counts these)
constexpr int kInH = kTileH + kWin - 1;     // staged rows: 26
constexpr int kInW = kTileW + kWin - 1;     // staged columns: 42
constexpr int kImgBlock = 256;
constexpr float kSsimC1 = 1e-4f, kSsimC2 = 9e-4f;  // 0.01^2, 0.03^2

struct ImgView {
  float* p;
  long long sh, sw, sc;  // element strides of row, column, channel
};

struct SsimArgs {
  ImgView x, y, gx;   // gx: the gradient image (adjoint only)
  int H, W, C;        // image
  int Hm, Wm;         // map extent
  int shift;          // staged row lr of a tile at r0 is row r0 - shift + lr of the SOURCE (forward: the image, shift = pad;
                      // adjoint: the derivative maps, shift = 10 - pad)
  int tiles_x, tiles_y;
  float g[kWin];
  float* map;         // [C, Hm, Wm] or nullptr
  float* dmaps;       // [3, C, Hm, Wm] or nullptr (forward: written; adjoint: read)
  float* partials;    // [C * tiles_y * tiles_x]
  const float* gout;  // adjoint: the upstream scalar
  float inv_n;        // adjoint: 1 / (Hm Wm C)
};

__device__ __forceinline__ void tile_of_block(const SsimArgs& a, int& ch, int& r0, int& c0) {
  unsigned b = blockIdx.x;
  const unsigned tx = b % (unsigned)a.tiles_x;
  b /= (unsigned)a.tiles_x;
  const unsigned ty = b % (unsigned)a.tiles_y;
  ch = (int)(b / (unsigned)a.tiles_y);
  r0 = (int)ty * kTileH;
  c0 = (int)tx * kTileW;
}

__global__ __launch_bounds__(kImgBlock) void ssim_forward_kernel(const SsimArgs a) {
  __shared__ float sx[kInH][kInW], sy[kInH][kInW];
  __shared__ float sh[5][kInH][kTileW];
  __shared__ float swave[kImgBlock / 64];
  const int tid = threadIdx.x;
  int ch, r0, c0;
  tile_of_block(a, ch, r0, c0);

  for (int i = tid; i < kInH * kInW; i += kImgBlock) {
    const int lr = i / kInW, lc = i - lr * kInW;
    const int ir = r0 - a.shift + lr, ic = c0 - a.shift + lc;
    float vx = 0.0f, vy = 0.0f;
    if (ir >= 0 && ir < a.H && ic >= 0 && ic < a.W) {
      vx = a.x.p[(long long)ir * a.x.sh + (long long)ic * a.x.sw + (long long)ch * a.x.sc];
      vy = a.y.p[(long long)ir * a.y.sh + (long long)ic * a.y.sw + (long long)ch * a.y.sc];
    }
    sx[lr][lc] = vx;
    sy[lr][lc] = vy;
  }
  __syncthreads();

  for (int i = tid; i < kInH * kTileW; i += kImgBlock) {
    const int lr = i / kTileW, lc = i % kTileW;
    float mx = 0.0f, my = 0.0f, xx = 0.0f, yy = 0.0f, xy = 0.0f;
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
      const float w = a.g[k], vx = sx[lr][lc + k], vy = sy[lr][lc + k];
      mx = fmaf(w, vx, mx);
      my = fmaf(w, vy, my);
      xx = fmaf(w, vx * vx, xx);
      yy = fmaf(w, vy * vy, yy);
      xy = fmaf(w, vx * vy, xy);
    }
    sh[0][lr][lc] = mx;
    sh[1][lr][lc] = my;
    sh[2][lr][lc] = xx;
    sh[3][lr][lc] = yy;
    sh[4][lr][lc] = xy;
  }
  __syncthreads();

  const long long plane = (long long)a.Hm * a.Wm;
  float local = 0.0f;
  for (int i = tid; i < kTileH * kTileW; i += kImgBlock) {
    const int lr = i / kTileW, lc = i % kTileW;
    const int r = r0 + lr, c = c0 + lc;
    if (r >= a.Hm || c >= a.Wm) continue;
    float mx = 0.0f, my = 0.0f, xx = 0.0f, yy = 0.0f, xy = 0.0f;
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
      const float w = a.g[k];
      mx = fmaf(w, sh[0][lr + k][lc], mx);
      my = fmaf(w, sh[1][lr + k][lc], my);
      xx = fmaf(w, sh[2][lr + k][lc], xx);
      yy = fmaf(w, sh[3][lr + k][lc], yy);
      xy = fmaf(w, sh[4][lr + k][lc], xy);
    }
    const float mxmy = mx * my, mx2 = mx * mx, my2 = my * my;
    const float sxx = xx - mx2, syy = yy - my2, sxy = xy - mxmy;
    const float A1 = 2.0f * mxmy + kSsimC1, A2 = 2.0f * sxy + kSsimC2;
    const float B1 = mx2 + my2 + kSsimC1, B2 = sxx + syy + kSsimC2;
    const float S = (A1 * A2) / (B1 * B2);
    local += S;
    const long long at = (long long)ch * plane + (long long)r * a.Wm + c;
    if (a.map) a.map[at] = S;
    if (a.dmaps) {
      const float inv = 1.0f / (B1 * B2);
      const float d_sxx = -S / B2, d_sxy = 2.0f * (A1 * inv);
      // the TOTAL derivative with respect to mu_x -- through A1, B1 and through s_xx = G*x^2 - mu_x^2, s_xy = G*xy - mu_x mu_y:
      // 2 mu_y A2 inv - 2 mu_x S / B1 - 2 mu_x d_sxx - mu_y d_sxy, collected so that only the last sum can cancel
      const float d_mu = (2.0f * inv) * (my * (A2 - A1) + (mx * S) * (B1 - B2));
      const long long maps = (long long)a.C * plane;
      a.dmaps[at] = d_mu;
      a.dmaps[maps + at] = d_sxx;
      a.dmaps[2 * maps + at] = d_sxy;
    }
  }
  // the tile's sum in a fixed order: (two values per thread) -> butterfly across the wave -> the four waves in order
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) local += __shfl_xor(local, off, 64);
  if ((tid & 63) == 0) swave[tid >> 6] = local;
  __syncthreads();
  if (tid == 0) a.partials[blockIdx.x] = ((swave[0] + swave[1]) + swave[2]) + swave[3];
}

// mean = (sum of the partials in float64, fixed order) / count, by ONE workgroup
__global__ __launch_bounds__(kImgBlock) void ssim_mean_kernel(const float* __restrict__ partials, long long n, double count, float* __restrict__ mean) {
  __shared__ double s[kImgBlock];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (long long i = tid; i < n; i += kImgBlock) acc += (double)partials[i];
  s[tid] = acc;
  __syncthreads();
  for (int off = kImgBlock / 2; off > 0; off >>= 1) {
    if (tid < off) s[tid] += s[tid + off];
    __syncthreads();
  }
  if (tid == 0) mean[0] = (float)(s[0] / count);
}

__global__ __launch_bounds__(kImgBlock) void ssim_backward_kernel(const SsimArgs a) {
  __shared__ float sd[3][kInH][kInW];
  __shared__ float sh[3][kInH][kTileW];
  const int tid = threadIdx.x;
  int ch, r0, c0;  // the tile's origin in IMAGE pixels
  tile_of_block(a, ch, r0, c0);
  const long long plane = (long long)a.Hm * a.Wm, maps = (long long)a.C * plane;

  for (int i = tid; i < kInH * kInW; i += kImgBlock) {
    const int lr = i / kInW, lc = i - lr * kInW;
    const int mr = r0 - a.shift + lr, mc = c0 - a.shift + lc;
    float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
    if (mr >= 0 && mr < a.Hm && mc >= 0 && mc < a.Wm) {
      const long long at = (long long)ch * plane + (long long)mr * a.Wm + mc;
      v0 = a.dmaps[at];
      v1 = a.dmaps[maps + at];
      v2 = a.dmaps[2 * maps + at];
    }
    sd[0][lr][lc] = v0;
    sd[1][lr][lc] = v1;
    sd[2][lr][lc] = v2;
  }
  __syncthreads();

  for (int i = tid; i < kInH * kTileW; i += kImgBlock) {
    const int lr = i / kTileW, lc = i % kTileW;
    float h0 = 0.0f, h1 = 0.0f, h2 = 0.0f;
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
      const float w = a.g[k];
      h0 = fmaf(w, sd[0][lr][lc + k], h0);
      h1 = fmaf(w, sd[1][lr][lc + k], h1);
      h2 = fmaf(w, sd[2][lr][lc + k], h2);
    }
    sh[0][lr][lc] = h0;
    sh[1][lr][lc] = h1;
    sh[2][lr][lc] = h2;
  }
  __syncthreads();

  const float scale = a.gout[0] * a.inv_n;
  for (int i = tid; i < kTileH * kTileW; i += kImgBlock) {
    const int lr = i / kTileW, lc = i % kTileW;
    const int r = r0 + lr, c = c0 + lc;
    if (r >= a.H || c >= a.W) continue;
    float gm = 0.0f, gs = 0.0f, gc = 0.0f;
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
      const float w = a.g[k];
      gm = fmaf(w, sh[0][lr + k][lc], gm);
      gs = fmaf(w, sh[1][lr + k][lc], gs);
      gc = fmaf(w, sh[2][lr + k][lc], gc);
    }
    const float xv = a.x.p[(long long)r * a.x.sh + (long long)c * a.x.sw + (long long)ch * a.x.sc];
    const float yv = a.y.p[(long long)r * a.y.sh + (long long)c * a.y.sw + (long long)ch * a.y.sc];
    a.gx.p[(long long)r * a.gx.sh + (long long)c * a.gx.sw + (long long)ch * a.gx.sc] = scale * (gm + 2.0f * xv * gs + yv * gc);
  }
}

void gaussian_window(float* g) {
  double w[kWin], sum = 0.0;
  for (int k = 0; k < kWin; ++k) {
    const double d = (double)(k - kWin / 2);
    w[k] = std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
    sum += w[k];
  }
  for (int k = 0; k < kWin; ++k) g[k] = (float)(w[k] / sum);
}

// a null pointer anywhere comes before a bad stride anywhere
int check_images(const RFImage* const* images, int count) {
  int rc = RF_OK;
  for (int i = 0; i < count; ++i) {
    const RFImage* im = images[i];
    if (!im || !im->data_dev) return RF_ERR_NULL_POINTER;
    if (im->stride_h == 0 || im->stride_w == 0 || im->stride_c == 0) rc = RF_ERR_BAD_SHAPE;
  }
  return rc;
}

ImgView view_of(const RFImage* im) { return ImgView{im->data_dev, (long long)im->stride_h, (long long)im->stride_w, (long long)im->stride_c}; }

// shapes and padding -> the fields of SsimArgs every launch shares; `over_image`: tiles cover the image (adjoint), else the map
int ssim_geometry(int32_t H, int32_t W, int32_t C, int32_t padding, bool over_image, SsimArgs& a) {
  if (H < 1 || W < 1 || C < 1) return RF_ERR_BAD_SHAPE;
  if (padding != RF_SSIM_VALID && padding != RF_SSIM_SAME) return RF_ERR_UNSUPPORTED;
  const int pad = padding == RF_SSIM_SAME ? kWin / 2 : 0;
  if (padding == RF_SSIM_VALID && (H < kWin || W < kWin)) return RF_ERR_BAD_SHAPE;
  a.H = H, a.W = W, a.C = C;
  a.Hm = padding == RF_SSIM_SAME ? H : H - (kWin - 1);
  a.Wm = padding == RF_SSIM_SAME ? W : W - (kWin - 1);
  a.shift = over_image ? (kWin - 1) - pad : pad;
  const int th = over_image ? H : a.Hm, tw = over_image ? W : a.Wm;
  a.tiles_y = (th + kTileH - 1) / kTileH;
  a.tiles_x = (tw + kTileW - 1) / kTileW;
  if ((long long)a.tiles_x * a.tiles_y * C > 0x7fffffffLL) return RF_ERR_BAD_SHAPE;
  gaussian_window(a.g);
  return RF_OK;
}

}  // namespace

extern "C" {

int64_t rf_ssim_tiles(int32_t height, int32_t width, int32_t channels, int32_t padding) {
  SsimArgs a{};
  const int rc = ssim_geometry(height, width, channels, padding, false, a);
  if (rc != RF_OK) return rc;
  return (int64_t)a.tiles_x * a.tiles_y * channels;
}

int rf_ssim_forward(const RFImage* image, const RFImage* target, int32_t height, int32_t width, int32_t channels, int32_t padding,
                    float* map_dev, float* dmaps_dev, float* partials_dev, float* mean_dev, void* stream) {
  if (!partials_dev || !mean_dev) return RF_ERR_NULL_POINTER;
  const RFImage* images[2] = {image, target};
  int rc = check_images(images, 2);
  if (rc != RF_OK) return rc;
  SsimArgs a{};
  rc = ssim_geometry(height, width, channels, padding, false, a);
  if (rc != RF_OK) return rc;
  a.x = view_of(image);
  a.y = view_of(target);
  a.map = map_dev;
  a.dmaps = dmaps_dev;
  a.partials = partials_dev;
  const long long blocks = (long long)a.tiles_x * a.tiles_y * channels;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ssim_forward_kernel, dim3((unsigned)blocks), dim3(kImgBlock), 0, st, a);
  rc = launch_status();
  if (rc != RF_OK) return rc;
  hipLaunchKernelGGL(ssim_mean_kernel, dim3(1), dim3(kImgBlock), 0, st, (const float*)partials_dev, blocks,
                     (double)a.Hm * (double)a.Wm * (double)channels, mean_dev);
  return launch_status();
}

int rf_ssim_backward(const RFImage* image, const RFImage* target, int32_t height, int32_t width, int32_t channels, int32_t padding,
                     const float* dmaps_dev, const float* grad_mean_dev, const RFImage* grad_image, void* stream) {
  if (!dmaps_dev || !grad_mean_dev) return RF_ERR_NULL_POINTER;
  const RFImage* images[3] = {image, target, grad_image};
  int rc = check_images(images, 3);
  if (rc != RF_OK) return rc;
  SsimArgs a{};
  rc = ssim_geometry(height, width, channels, padding, true, a);
  if (rc != RF_OK) return rc;
  a.x = view_of(image);
  a.y = view_of(target);
  a.gx = view_of(grad_image);
  a.dmaps = const_cast<float*>(dmaps_dev);
  a.gout = grad_mean_dev;
  a.inv_n = (float)(1.0 / ((double)a.Hm * (double)a.Wm * (double)channels));
  const long long blocks = (long long)a.tiles_x * a.tiles_y * channels;
  hipLaunchKernelGGL(ssim_backward_kernel, dim3((unsigned)blocks), dim3(kImgBlock), 0, (hipStream_t)stream, a);
  return launch_status();
}

}  // extern "C"
