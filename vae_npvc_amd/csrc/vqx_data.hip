// Input pipeline (gfx950): training batches cut from a device-resident corpus.
#include "vqx_common.h"

#include <cstring>

namespace vqx {

// The per-item crop description travels by value in the kernel arguments (as
// vqx_gather_rows_host passes its rows): no copy on the stream.
constexpr int kCropArgItems = 192;
struct CropItems {
  int64_t row0[kCropArgItems];
  int32_t len[kCropArgItems];
  int32_t utt[kCropArgItems];
};
static_assert(sizeof(CropItems) + 64 <= 4096, "CropItems and the other arguments must fit the 4 KB kernel-argument segment");

// x[b][c][t] = corpus[row0[b] + t][c] (t < len[b]), 0 up to T; y[b] = spk_table[utt[b]].
// One 32 x 32 tile a block (x over T, y over mel, z the item): rows of the
// corpus are read along mel, transposed in a padded LDS tile and written along
// t, so both sides are coalesced.  A tile wholly past len[b] stores zeros
// without reading.  The host validated every index (vqx_crop_batch).
__global__ __launch_bounds__(256) void crop_batch_kernel(const float* __restrict__ corpus,
                                                         const int64_t* __restrict__ spk_table, CropItems I, int mel,
                                                         int T_, float* __restrict__ x, int64_t* __restrict__ y) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z;
  const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int len = I.len[b];
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) y[b] = spk_table[I.utt[b]];
  float* xb = x + (int64_t)b * mel * T_;
  if (t0 >= len) {  // block-uniform: the zero tail
    for (int i = ty; i < 32; i += 8) {
      const int c = c0 + i, t = t0 + tx;
      if (c < mel && t < T_) xb[(int64_t)c * T_ + t] = 0.f;
    }
    return;
  }
  const float* src = corpus + I.row0[b] * mel;
  for (int i = ty; i < 32; i += 8) {
    const int t = t0 + i, c = c0 + tx;
    tile[i][tx] = (t < len && c < mel) ? src[(int64_t)t * mel + c] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, t = t0 + tx;
    if (c < mel && t < T_) xb[(int64_t)c * T_ + t] = tile[tx][i];
  }
}

}  // namespace vqx

using namespace vqx;

extern "C" int vqx_crop_batch(const float* corpus, int64_t n_rows, int32_t mel, const int64_t* spk_table,
                              int32_t n_utts, const int64_t* row0, const int32_t* len, const int32_t* utt, int32_t B,
                              int32_t T, float* x, int64_t* y, vqx_stream_t stream) {
  if (B < 1 || T < 1 || mel < 1 || T > (1 << 20) || mel > (1 << 20) || n_rows < 0 || n_utts < 1) {
    set_error("vqx_crop_batch: bad sizes (B %d, T %d, mel %d, n_rows %lld, n_utts %d)", B, T, mel, (long long)n_rows,
              n_utts);
    return -1;
  }
  if (!corpus || !spk_table || !row0 || !len || !utt || !x || !y) {
    set_error("vqx_crop_batch: null pointer");
    return -1;
  }
  for (int b = 0; b < B; ++b) {  // every item before any launch: the kernel trusts the indices
    if (len[b] < 0 || len[b] > T) {
      set_error("vqx_crop_batch: item %d: len %d outside [0, T = %d]", b, len[b], T);
      return -1;
    }
    if (row0[b] < 0 || row0[b] > n_rows - len[b]) {
      set_error("vqx_crop_batch: item %d: rows [%lld, %lld + %d) outside the corpus's %lld rows", b,
                (long long)row0[b], (long long)row0[b], len[b], (long long)n_rows);
      return -1;
    }
    if (utt[b] < 0 || utt[b] >= n_utts) {
      set_error("vqx_crop_batch: item %d: utt %d outside [0, %d)", b, utt[b], n_utts);
      return -1;
    }
  }
  for (int b0 = 0; b0 < B; b0 += kCropArgItems) {
    CropItems I = {};
    const int n = std::min(kCropArgItems, B - b0);
    memcpy(I.row0, row0 + b0, sizeof(int64_t) * n);
    memcpy(I.len, len + b0, sizeof(int32_t) * n);
    memcpy(I.utt, utt + b0, sizeof(int32_t) * n);
    hipLaunchKernelGGL(crop_batch_kernel, dim3((T + 31) / 32, (mel + 31) / 32, n), dim3(256), 0, (hipStream_t)stream,
                       corpus, spk_table, I, mel, T, x + (int64_t)b0 * mel * T, y + b0);
  }
  return launch_status("vqx_crop_batch");
}
