// vq_kernels.hip -- vector quantisation of feature vectors against a codebook (rf_vq_assign / rf_vq_centroids of relu_field.h): the
// two halves of an importance-weighted Lloyd iteration.  DESIGN.md section 18 has the contract, the error bounds and the measurements.
//
// rf_vq_assign.  A workgroup of 256 threads (4 waves) owns 128 rows of `vectors`, each wave 32 of them, and walks the WHOLE codebook
// in LDS stages of 128 codes.  The ranking value of (row x, code c) is
//     s(x, c) = ||c||^2 - 2 x.c          (= the squared distance minus ||x||^2, which is the same for every code of a row)
// computed by v_mfma_f32_32x32x2_f32 as ONE k-ordered float32 fma chain per pair: the accumulator starts at ||c||^2 (summed in
// float64 from the staged tile and rounded once), the A operand is the code (lane l: code l & 31, k = 2 s + (l >> 5), read from the
// LDS tile whose rows are 65 floats apart: the 32 lanes of a half hit 32 different banks), the B operand is -2 x of the wave's row
// l & 31 (exact scaling; the row lives in KS registers for the whole kernel).  k is padded with zeros to 2 KS: fma(0, 0, acc) == acc,
// no rounding.  The result tile has the row on the lane (column l & 31) and 16 codes in the 16 accumulator registers (code
// (r & 3) + 8 (r >> 2) + 4 (l >> 5) of the 32), so the running (minimum, argument) is ONE pair of registers per lane, updated by a
// strict `<` in ascending code order; the two lanes of a row are combined once at the end, the lower index winning a tie.  Hence:
// among computed-equal values the lowest index wins, the distances are never in memory, there are no atomics, and the same inputs
// give the same bits.  dist_out is NOT s + ||x||^2: it is sum_k (x_k - c_jk)^2 of the winner j, recomputed in ascending k in plain
// float32 (the library is built with -ffp-contract=off).
// Budget per workgroup: LDS 128 x 65 + 128 floats = 33.8 KB (four workgroups per CU); registers: KS <= 32 for the row, 16 accumulators.
//
// rf_vq_centroids.  One workgroup of 256 threads per code: lane k of every wave owns dimension k (D <= 64), the segment of the code
// in `order` is dealt out in 16 streams -- entry j of the segment belongs to stream j mod 16, wave w holds the streams 4 w .. 4 w + 3
// in four independent accumulators -- each a sequential chain acc = acc + w * x in segment order; then the fixed tree
// ((a0 + a1) + (a2 + a3)) inside the wave and ((W0 + W1) + (W2 + W3)) across the waves through LDS, the same for the weight sum,
// and one division.  No atomics; the order depends on nothing but the segment.
#include "rf_device.h"

namespace {

constexpr int kVqBlock = 256;
constexpr int kVqRows = 128;    // rows of `vectors` per workgroup: 32 per wave
constexpr int kVqCodes = 128;   // codes per LDS stage: 4 MFMA tiles of 32
constexpr int kVqMaxDim = 64;
constexpr int kVqMaxCodes = 65536;
constexpr int kVqStride = kVqMaxDim + 1;  // floats between the rows of the LDS tile (odd: conflict-free column reads)

using vq_f32x16 = __attribute__((ext_vector_type(16))) float;

struct VqAssignArgs {
  const float* x;
  long long M, stride;
  int D, C;
  const float* cb;
  int* index;
  float* dist;
};

// KS: k-steps of the MFMA chain (2 dimensions each), D <= 2 KS
template <int KS>
__global__ __launch_bounds__(kVqBlock) void vq_assign_kernel(const VqAssignArgs a) {
  __shared__ float tile[kVqCodes * kVqStride];
  __shared__ float cnorm[kVqCodes];
  static_assert(kVqRows == kVqCodes, "the row block is staged through the code tile");
  constexpr int DP = 2 * KS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, half = lane >> 5;
  const long long row0 = (long long)blockIdx.x * kVqRows;

  // the workgroup's rows through LDS (coalesced reads), then -2 x into registers in the B-operand order
  for (int i = tid; i < kVqRows * DP; i += kVqBlock) {
    const int r = i / DP, k = i - r * DP;
    const long long row = row0 + r;
    tile[r * kVqStride + k] = (row < a.M && k < a.D) ? a.x[row * a.stride + k] : 0.0f;
  }
  __syncthreads();
  float xr[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) xr[s] = -2.0f * tile[(wave * 32 + col) * kVqStride + 2 * s + half];
  __syncthreads();

  const bool active = row0 + wave * 32 < a.M;  // (a wave without rows only helps staging)
  float best = INFINITY;
  int best_code = 0;
  for (int c0 = 0; c0 < a.C; c0 += kVqCodes) {
    for (int i = tid; i < kVqCodes * DP; i += kVqBlock) {
      const int r = i / DP, k = i - r * DP;
      const int code = c0 + r;
      tile[r * kVqStride + k] = (code < a.C && k < a.D) ? a.cb[(long long)code * a.D + k] : 0.0f;
    }
    __syncthreads();
    if (tid < kVqCodes) {
      double n = 0.0;
      for (int k = 0; k < a.D; ++k) {
        const double v = (double)tile[tid * kVqStride + k];
        n += v * v;
      }
      cnorm[tid] = c0 + tid < a.C ? (float)n : INFINITY;  // a code past the end never wins
    }
    __syncthreads();
    if (active) {
      const int tiles = min(kVqCodes / 32, (a.C - c0 + 31) / 32);
      for (int t = 0; t < tiles; ++t) {
        vq_f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = cnorm[t * 32 + (r & 3) + 8 * (r >> 2) + 4 * half];
        const float* arow = tile + (t * 32 + col) * kVqStride + half;
#pragma unroll
        for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[2 * s], xr[s], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float v = acc[r];
          if (v < best) {
            best = v;
            best_code = c0 + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          }
        }
      }
    }
    __syncthreads();
  }

  // the two lanes of a row hold disjoint codes: the smaller value, the lower index on a tie
  const float other = __shfl_xor(best, 32, 64);
  const int other_code = __shfl_xor(best_code, 32, 64);
  if (other < best || (other == best && other_code < best_code)) {
    best = other;
    best_code = other_code;
  }
  const long long row = row0 + wave * 32 + col;
  if (half == 0 && row < a.M) {
    const float* xp = a.x + row * a.stride;
    const float* cp = a.cb + (long long)best_code * a.D;
    float d = 0.0f;
    for (int k = 0; k < a.D; ++k) {
      const float t = xp[k] - cp[k];
      d = d + t * t;
    }
    a.index[row] = best_code;
    a.dist[row] = d;
  }
}

struct VqCentroidArgs {
  const float* x;
  long long stride;
  int D, C;
  const float* w;
  const int* order;
  const long long* offsets;
  float* cb;
  float* wsum;
};

__global__ __launch_bounds__(kVqBlock) void vq_centroid_kernel(const VqCentroidArgs a) {
  __shared__ float ssum[kVqBlock / 64][64];
  __shared__ float sw[kVqBlock / 64];
  const int tid = threadIdx.x, k = tid & 63, wave = tid >> 6;
  const int c = blockIdx.x;
  const long long b = a.offsets[c], e = a.offsets[c + 1];
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, wacc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (long long j = b + wave * 4; j < e; j += 16) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (j + u < e) {
        const long long v = a.order[j + u];
        const float wt = a.w[v];
        const float xv = k < a.D ? a.x[v * a.stride + k] : 0.0f;
        acc[u] = acc[u] + wt * xv;
        wacc[u] = wacc[u] + wt;
      }
    }
  }
  ssum[wave][k] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  if (k == 0) sw[wave] = (wacc[0] + wacc[1]) + (wacc[2] + wacc[3]);
  __syncthreads();
  if (wave == 0) {
    const float total = (ssum[0][k] + ssum[1][k]) + (ssum[2][k] + ssum[3][k]);
    const float weight = (sw[0] + sw[1]) + (sw[2] + sw[3]);
    if (k == 0 && a.wsum) a.wsum[c] = weight;
    if (e > b && weight > 0.0f && k < a.D) a.cb[(long long)c * a.D + k] = total / weight;
  }
}

int check_vq_sizes(int32_t dim, int32_t num_codes) {
  return (dim < 1 || dim > kVqMaxDim || num_codes < 1 || num_codes > kVqMaxCodes) ? RF_ERR_UNSUPPORTED : RF_OK;
}

}  // namespace

extern "C" {

int rf_vq_assign(const float* vectors_dev, int64_t num_vectors, int32_t dim, int64_t row_stride, const float* codebook_dev, int32_t num_codes,
                 int32_t* index_out_dev, float* dist_out_dev, void* stream) {
  if (!codebook_dev) return RF_ERR_NULL_POINTER;
  if (num_vectors != 0 && (!vectors_dev || !index_out_dev || !dist_out_dev)) return RF_ERR_NULL_POINTER;
  const int rc = check_vq_sizes(dim, num_codes);
  if (rc != RF_OK) return rc;
  if (num_vectors < 0 || row_stride < dim) return RF_ERR_BAD_SHAPE;
  if (num_vectors == 0) return RF_OK;
  const void* outs[2] = {index_out_dev, dist_out_dev};
  if (outs[0] == outs[1]) return RF_ERR_BAD_SHAPE;
  for (const void* o : outs)
    if (o == (const void*)vectors_dev || o == (const void*)codebook_dev) return RF_ERR_BAD_SHAPE;
  const long long blocks = ((long long)num_vectors + kVqRows - 1) / kVqRows;
  if (blocks > 0x7fffffffLL) return RF_ERR_BAD_SHAPE;
  VqAssignArgs a{vectors_dev, (long long)num_vectors, (long long)row_stride, dim, num_codes, codebook_dev, index_out_dev, dist_out_dev};
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), block(kVqBlock);
  if (dim <= 4) hipLaunchKernelGGL(vq_assign_kernel<2>, grid, block, 0, st, a);
  else if (dim <= 12) hipLaunchKernelGGL(vq_assign_kernel<6>, grid, block, 0, st, a);
  else if (dim <= 28) hipLaunchKernelGGL(vq_assign_kernel<14>, grid, block, 0, st, a);
  else if (dim <= 48) hipLaunchKernelGGL(vq_assign_kernel<24>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(vq_assign_kernel<32>, grid, block, 0, st, a);
  return launch_status();
}

int rf_vq_centroids(const float* vectors_dev, int64_t row_stride, int32_t dim, const float* weights_dev, const int32_t* order_dev,
                    const int64_t* offsets_dev, int32_t num_codes, float* codebook_inout_dev, float* weight_sum_out_dev, void* stream) {
  if (!vectors_dev || !weights_dev || !order_dev || !offsets_dev || !codebook_inout_dev) return RF_ERR_NULL_POINTER;
  const int rc = check_vq_sizes(dim, num_codes);
  if (rc != RF_OK) return rc;
  if (row_stride < dim) return RF_ERR_BAD_SHAPE;
  const void* outs[2] = {codebook_inout_dev, weight_sum_out_dev};
  if (outs[0] == outs[1]) return RF_ERR_BAD_SHAPE;
  for (const void* o : outs)
    if (o && (o == (const void*)vectors_dev || o == (const void*)weights_dev || o == (const void*)order_dev || o == (const void*)offsets_dev)) return RF_ERR_BAD_SHAPE;
  VqCentroidArgs a{vectors_dev, (long long)row_stride, dim, num_codes, weights_dev, order_dev, (const long long*)offsets_dev, codebook_inout_dev, weight_sum_out_dev};
  hipLaunchKernelGGL(vq_centroid_kernel, dim3((unsigned)num_codes), dim3(kVqBlock), 0, (hipStream_t)stream, a);
  return launch_status();
}

}  // extern "C"
