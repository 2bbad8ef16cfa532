// Length-aware memory-bound kernels of the hierarchical model's batched
// conversion (include/vqx.h "A batch of different lengths"): a padded batch
// [B*T][ld] of frame-major rows in which utterance b owns rows t < len[b].
//
// The lengths are host values and travel by value in the kernel arguments (as
// vqx_crop_batch passes its items): no device table, no copy on the stream, no
// allocation.  A launch covers up to kLenItems utterances (kCatItems for the
// concatenation, whose table holds a length per level); a larger batch is cut
// into launches.  The utterance is blockIdx.y, so the table index is uniform
// over the workgroup: the compiler reads the entry with a scalar load from the
// argument segment (no scratch copy of the table; the resource-usage remark of
// every kernel here reports ScratchSize 0).
//
//   gn_len_partial_kernel  vqx_groupnorm_stats_len: the (count, mean, M2) of
//             gn_partial_vec_kernel over rows t < len[b], same two passes
//             (mean, then centred sum of squares), same 8 row parts; a part
//             without rows has count 0 and is skipped by the finalize.
//   gn_len_finalize_kernel the parts merged in part order in double (Chan), as
//             gn_finalize_kernel.
//   gn_lrelu_len_kernel / gn_glu_len_kernel  the element math of
//             gn_lrelu_fwd_kernel / gn_glu_fwd_vec_kernel on rows t < len[b]
//             (the same expressions, so the same bits), 16-byte zeros on the
//             rows from len[b] up, which are not read.
//   mask_tail_kernel       16-byte zero stores over rows len[b] <= t < T only.
//   codes_cat_len_kernel   hier_codes_cat_kernel with the stretch factor
//             n_b / m_{b,l} taken per utterance; rows t >= n_b are zeros.
//   segment_mean_kernel    out[b][c] = (sum_{t < len[b]} z[b*T + t][c]) / len[b]:
//             16 row groups (rows rg, rg + 16, ... added in ascending t from
//             0.f), the 16 sums added in ascending rg from 0.f, one division.
//   nct_to_ntc_len_kernel / ntc_to_nct_len_kernel  the flat model's two layout
//             changes with the tail mask folded in (the 32 x 32 LDS tile of
//             nct_to_ntc_tile; the utterance is blockIdx.z): frames t >= len[b]
//             are selected zeros and their source is never loaded.
//   nct_to_ntc_pad_len_kernel  nct_to_ntc_len_kernel for a source (B, C, T_in)
//             shorter than the T >= T_in rows an utterance gets: the input
//             layout change of vqvae2a / vqvae2b's batched conversion, whose
//             padded frame count is a multiple of the encoders' down-sampling.
//   index_mask_len_kernel  out[b][t] = t < len[b] ? idx[b*T + t] : 0 over
//             t < T_out <= T, int64: the codes of a padded batch as `encode`
//             returns them; entries from len[b] on are never loaded.
// No atomics anywhere; equal arguments give equal bits.
#include "vqx_common.h"
#include "vqx_vec.h"

#include <algorithm>
#include <cstring>

namespace vqx {
namespace {

constexpr int kLenItems = 896;  // utterances a launch of the per-length kernels
struct LenTable {
  int32_t len[kLenItems];
};
static_assert(sizeof(LenTable) + 256 <= 4096, "LenTable and the other arguments must fit the 4 KB kernel-argument segment");

constexpr int kVarParts = 8;  // row parts of the statistics, as kGnParts of vqx_gn.hip

template <typename T>
__global__ __launch_bounds__(256) void gn_len_partial_kernel(const T* __restrict__ x, int ldx, int T_, int C, int G,
                                                             LenTable L, float* __restrict__ part) {
  constexpr int V = Vec<T>::N;
  const int p = blockIdx.x, bg = blockIdx.y;
  const int b = bg / G, g = bg - b * G;
  const int len = L.len[b];
  const int cg = C / G, cpr = cg / V;
  const int r0 = p * len / kVarParts, r1 = (p + 1) * len / kVarParts;
  const int chunks = (r1 - r0) * cpr;
  __shared__ float red[16];
  const T* base = x + ((int64_t)b * T_ + r0) * ldx + g * cg;
  float s = 0.f;
  for (int i = threadIdx.x; i < chunks; i += 256) {
    const int rr = i / cpr, ch = i - rr * cpr;
    float f[V];
    Vec<T>::load(base + (int64_t)rr * ldx + ch * V, f);
#pragma unroll
    for (int k = 0; k < V; ++k) s += f[k];
  }
  s = block_sum(s, red);
  const int64_t cnt = (int64_t)(r1 - r0) * cg;
  const float mean = cnt ? s / (float)cnt : 0.f;
  float m2 = 0.f;
  for (int i = threadIdx.x; i < chunks; i += 256) {
    const int rr = i / cpr, ch = i - rr * cpr;
    float f[V];
    Vec<T>::load(base + (int64_t)rr * ldx + ch * V, f);
#pragma unroll
    for (int k = 0; k < V; ++k) { const float d = f[k] - mean; m2 = fmaf(d, d, m2); }
  }
  m2 = block_sum(m2, red);
  if (threadIdx.x == 0) {
    float* o = part + ((int64_t)bg * kVarParts + p) * 3;
    o[0] = (float)cnt;
    o[1] = mean;
    o[2] = m2;
  }
}

__global__ void gn_len_finalize_kernel(const float* __restrict__ part, int nbg, float eps, float* __restrict__ mr) {
  const int bg = blockIdx.x * blockDim.x + threadIdx.x;
  if (bg >= nbg) return;
  double n = 0.0, mean = 0.0, m2 = 0.0;
  for (int p = 0; p < kVarParts; ++p) {
    const float* o = part + ((int64_t)bg * kVarParts + p) * 3;
    const double nb = o[0];
    if (nb == 0.0) continue;
    const double d = (double)o[1] - mean;
    const double nn = n + nb;
    mean += d * nb / nn;
    m2 += (double)o[2] + d * d * n * nb / nn;
    n = nn;
  }
  const float var = n > 0.0 ? (float)(m2 / n) : 0.f;
  mr[2 * bg] = (float)mean;
  mr[2 * bg + 1] = 1.0f / sqrtf(var + eps);
}

// blockIdx.y = utterance, blockIdx.x strides over its T * cpr 16-byte chunks.
template <typename T>
__global__ __launch_bounds__(256) void gn_lrelu_len_kernel(const T* __restrict__ h, int ldh, T* __restrict__ g, int ldg,
                                                           int T_, int cpr, LenTable L, const float* __restrict__ mr,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ beta) {
  constexpr int V = Vec<T>::N;
  const int b = blockIdx.y;
  const int len = L.len[b];
  const float m = mr[2 * b], rs = mr[2 * b + 1];
  const int total = T_ * cpr;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int t = i / cpr;
    const int c = (i - t * cpr) * V;
    const int64_t r = (int64_t)b * T_ + t;
    float x[V];
    if (t < len) {
      Vec<T>::load(h + r * ldh + c, x);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float v = (x[k] - m) * rs * gamma[c + k] + beta[c + k];
        x[k] = v > 0.f ? v : 0.2f * v;
      }
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) x[k] = 0.f;
    }
    Vec<T>::store(g + r * ldg + c, x);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void gn_glu_len_kernel(const T* __restrict__ u, int ldu, T* __restrict__ g, int ldg,
                                                         int T_, int half, int cpr, LenTable L,
                                                         const float* __restrict__ mr, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta) {
  constexpr int V = Vec<T>::N;
  const int b = blockIdx.y;
  const int len = L.len[b];
  const float ma = mr[4 * b + 0], ra = mr[4 * b + 1], mb = mr[4 * b + 2], rb = mr[4 * b + 3];
  const int total = T_ * cpr;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int t = i / cpr;
    const int c = (i - t * cpr) * V;
    const int64_t r = (int64_t)b * T_ + t;
    float o[V];
    if (t < len) {
      float ua[V], ub[V];
      Vec<T>::load(u + r * ldu + c, ua);
      Vec<T>::load(u + r * ldu + c + half, ub);
#pragma unroll
      for (int k = 0; k < V; ++k)
        o[k] = ftanh<sizeof(T) == 2>((ua[k] - ma) * ra * gamma[c + k] + beta[c + k]) *
               fsigmoid<sizeof(T) == 2>((ub[k] - mb) * rb * gamma[c + half + k] + beta[c + half + k]);
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) o[k] = 0.f;
    }
    Vec<T>::store(g + r * ldg + c, o);
  }
}

// x as 16-byte words: row stride ldq words, cpr words a row.
__global__ __launch_bounds__(256) void mask_tail_kernel(uint4* __restrict__ x, int64_t ldq, int T_, int cpr, LenTable L) {
  const int b = blockIdx.y;
  const int len = L.len[b];
  const int total = (T_ - len) * cpr;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int tt = i / cpr;
    const int q = i - tt * cpr;
    x[((int64_t)b * T_ + len + tt) * ldq + q] = make_uint4(0u, 0u, 0u, 0u);
  }
}

constexpr int kCatLevels = 8;
constexpr int kCatItems = 96;  // utterances a launch of the concatenation
struct CatLevels {
  const float* src[kCatLevels];    // the dense level or the codebook
  const int64_t* idx[kCatLevels];  // nullptr: dense
  int T_l[kCatLevels], ld[kCatLevels], gran[kCatLevels], off[kCatLevels], normalize[kCatLevels];
  int n;
};
struct CatLens {
  int32_t n[kCatItems];              // target length of the utterance
  int32_t m[kCatItems][kCatLevels];  // its length at every level
};
static_assert(sizeof(CatLevels) + sizeof(CatLens) + 128 <= 4096,
              "CatLevels, CatLens and the other arguments must fit the 4 KB kernel-argument segment");
constexpr int kCatWaves = 4;  // output rows per workgroup

// One wavefront per output row (blockIdx.y the utterance of this launch, b0 the
// launch's first utterance): lane j moves granules j, j + 64, ... of each level
// with 16-byte loads and stores, as hier_codes_cat_kernel.  Row, level kind,
// lengths and the code index are wave-uniform.
template <bool BF16>
__global__ __launch_bounds__(kCatWaves * 64) void codes_cat_len_kernel(CatLevels L, CatLens N, int b0, int T, int total,
                                                                        void* __restrict__ out, int64_t ldo) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * kCatWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (t >= T) return;
  const int bl = blockIdx.y;
  const int64_t b = b0 + bl;
  const int64_t row = b * T + t;
  const int n_b = N.n[bl];
  if (t >= n_b) {  // the utterance's tail: zeros over the concatenated width
    for (int g = lane; g < total / 4; g += 64) {
      if constexpr (BF16) *(uint2*)((bf16_t*)out + row * ldo + 4 * g) = make_uint2(0u, 0u);
      else *(f32x4_t*)((float*)out + row * ldo + 4 * g) = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    return;
  }
#pragma unroll
  for (int l = 0; l < kCatLevels; ++l) {
    if (l >= L.n) break;
    const int m = N.m[bl][l];
    int s = t / (n_b / m);
    s = s < m ? s : m - 1;
    const int64_t frame = b * L.T_l[l] + s;
    const int64_t src_row = L.idx[l] ? L.idx[l][frame] : frame;
    const float* src = L.src[l] + src_row * L.ld[l];
    const int G = L.gran[l];
    const bool norm = L.idx[l] && L.normalize[l];
    float len = 1.f;
    if (norm) {
      float ss = 0.f;
      for (int g = lane; g < G; g += 64) {
        const f32x4_t x = *(const f32x4_t*)(src + 4 * g);
        ss += x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3];
      }
      len = sqrtf(wave_sum(ss));
    }
    const int64_t at = row * ldo + L.off[l];
    for (int g = lane; g < G; g += 64) {
      f32x4_t x = *(const f32x4_t*)(src + 4 * g);
      if (norm) x = {x[0] / len, x[1] / len, x[2] / len, x[3] / len};
      if constexpr (BF16) {
        *(uint2*)((bf16_t*)out + at + 4 * g) = make_uint2(pack_bf16x2(x[0], x[1]), pack_bf16x2(x[2], x[3]));
      } else {
        *(f32x4_t*)((float*)out + at + 4 * g) = x;
      }
    }
  }
}

// Workgroup = (utterance, 64 columns): thread = (16-byte chunk tid & 15, row group tid >> 4).
__global__ __launch_bounds__(256) void segment_mean_kernel(const float* __restrict__ z, int64_t ldz, int T_, int C,
                                                           LenTable L, float* __restrict__ out, int64_t ldo) {
  __shared__ f32x4_t part[16][16];
  const int b = blockIdx.y;
  const int len = L.len[b];
  const int ch = threadIdx.x & 15, rg = threadIdx.x >> 4;
  const int c = blockIdx.x * 64 + ch * 4;
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  if (c < C)
    for (int t = rg; t < len; t += 16) acc += *(const f32x4_t*)(z + ((int64_t)b * T_ + t) * ldz + c);
  part[rg][ch] = acc;
  __syncthreads();
  if (rg == 0 && c < C) {
    f32x4_t sum = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < 16; ++k) sum += part[k][ch];
    const float n = (float)len;
    *(f32x4_t*)(out + (int64_t)b * ldo + c) = f32x4_t{sum[0] / n, sum[1] / n, sum[2] / n, sum[3] / n};
  }
}

// nct_to_ntc_tile (vqx_common.h) with the tail mask folded in: one 32 x 32 tile
// a workgroup (blockIdx.x over T, .y over C, .z the utterance of this launch).
// A frame t >= len[b] gets a selected 0.f and is never loaded; a tile wholly
// past len[b] stores its zeros without touching x or the LDS.
template <typename T>
__global__ __launch_bounds__(256) void nct_to_ntc_len_kernel(const float* __restrict__ x, int C, int T_, LenTable L,
                                                             T* __restrict__ y, int64_t ldy) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z;
  const int len = L.len[b];
  const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 256 threads: 8 rows per pass
  if (t0 >= len) {  // workgroup-uniform
    for (int i = ty; i < 32; i += 8) {
      const int t = t0 + i, c = c0 + tx;
      if (c < C && t < T_) Elem<T>::st(y, ((int64_t)b * T_ + t) * ldy + c, 0.f);
    }
    return;
  }
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, t = t0 + tx;
    tile[i][tx] = (c < C && t < len) ? x[((int64_t)b * C + c) * T_ + t] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int t = t0 + i, c = c0 + tx;
    if (c < C && t < T_) Elem<T>::st(y, ((int64_t)b * T_ + t) * ldy + c, tile[tx][i]);
  }
}

// ntc_to_nct_kernel (vqx_layout.hip) with the tail mask folded in and the output
// cut to T_out <= T frames (blockIdx.x over T_out): rows t >= len[b] of y are
// never loaded, whatever they hold.
template <typename T>
__global__ __launch_bounds__(256) void ntc_to_nct_len_kernel(const T* __restrict__ y, int64_t ldy, int C, int T_,
                                                             LenTable L, float* __restrict__ x, int T_out) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z;
  const int len = L.len[b];
  const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  if (t0 >= len) {  // workgroup-uniform
    for (int i = ty; i < 32; i += 8) {
      const int c = c0 + i, t = t0 + tx;
      if (c < C && t < T_out) x[((int64_t)b * C + c) * T_out + t] = 0.f;
    }
    return;
  }
  for (int i = ty; i < 32; i += 8) {
    const int t = t0 + i, c = c0 + tx;
    tile[i][tx] = (c < C && t < len) ? Elem<T>::ld(y, ((int64_t)b * T_ + t) * ldy + c) : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, t = t0 + tx;
    if (c < C && t < T_out) x[((int64_t)b * C + c) * T_out + t] = tile[tx][i];
  }
}

// nct_to_ntc_len_kernel with the source's frame count T_in apart from the row
// count T_ >= T_in of an utterance (blockIdx.x over T_): len[b] <= T_in, so a
// frame past the source is past len[b] and is a selected zero like any other.
template <typename T>
__global__ __launch_bounds__(256) void nct_to_ntc_pad_len_kernel(const float* __restrict__ x, int C, int T_in, int T_,
                                                                 LenTable L, T* __restrict__ y, int64_t ldy) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z;
  const int len = L.len[b];
  const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  if (t0 >= len) {  // workgroup-uniform
    for (int i = ty; i < 32; i += 8) {
      const int t = t0 + i, c = c0 + tx;
      if (c < C && t < T_) Elem<T>::st(y, ((int64_t)b * T_ + t) * ldy + c, 0.f);
    }
    return;
  }
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, t = t0 + tx;
    tile[i][tx] = (c < C && t < len) ? x[((int64_t)b * C + c) * T_in + t] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int t = t0 + i, c = c0 + tx;
    if (c < C && t < T_) Elem<T>::st(y, ((int64_t)b * T_ + t) * ldy + c, tile[tx][i]);
  }
}

// blockIdx.y = utterance, blockIdx.x strides over its T_out entries.
__global__ __launch_bounds__(256) void index_mask_len_kernel(const int64_t* __restrict__ idx, int T_, LenTable L,
                                                             int64_t* __restrict__ out, int T_out) {
  const int b = blockIdx.y;
  const int len = L.len[b];
  for (int t = blockIdx.x * 256 + threadIdx.x; t < T_out; t += gridDim.x * 256)
    out[(int64_t)b * T_out + t] = t < len ? idx[(int64_t)b * T_ + t] : (int64_t)0;
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Every item before any launch: len[b] in 1..T.
int check_lens(const char* who, const int32_t* len, int64_t n_rows, int T, int& B) {
  if (!len) { set_error("%s: null len", who); return -1; }
  if (T < 1 || n_rows < T || n_rows % T || n_rows > INT32_MAX) {
    set_error("%s: n_rows = %lld is not a positive multiple of T = %d below 2^31", who, (long long)n_rows, T);
    return -1;
  }
  B = (int)(n_rows / T);
  for (int b = 0; b < B; ++b)
    if (len[b] < 1 || len[b] > T) { set_error("%s: item %d: len %d outside [1, T = %d]", who, b, len[b], T); return -1; }
  return 0;
}

LenTable table_at(const int32_t* len, int b0, int n) {
  LenTable L = {};
  memcpy(L.len, len + b0, sizeof(int32_t) * n);
  return L;
}

int blocks_for(int64_t chunks) { return (int)std::min<int64_t>(std::max<int64_t>((chunks + 255) / 256, 1), 1024); }

// Checks shared by the two layout changes (C channels of a [B*T][ldy] matrix): 0 when the launches may go.
int check_layout(const char* who, const void* x, const void* y, int B, int C, int T, int ldy, int dtype,
                 const int32_t* len, int& Bc) {
  if (B < 1) { set_error("%s: B = %d utterances", who, B); return -1; }
  if (check_lens(who, len, (int64_t)B * T, T, Bc)) return -1;
  if (dtype != VQX_F32 && dtype != VQX_BF16) { set_error("%s: bad dtype %d", who, dtype); return -1; }
  const uintptr_t ya = dtype == VQX_BF16 ? 1 : 3;
  if (!x || !y || ((uintptr_t)x & 3) || ((uintptr_t)y & ya)) {
    set_error("%s: null or unaligned pointer (f32 4 B, bf16 2 B)", who);
    return -1;
  }
  if (C < 1 || (C + 31) / 32 > 65535 || ldy < C) {
    set_error("%s: C = %d, ldy = %d (1 <= C <= %d, ldy >= C)", who, C, ldy, 65535 * 32);
    return -1;
  }
  return 0;
}

}  // namespace
}  // namespace vqx

using namespace vqx;

extern "C" int vqx_groupnorm_stats_len(const void* x, int32_t ldx, int32_t dtype, int64_t n_rows, int32_t T, int32_t C,
                                       int32_t G, const int32_t* len, float eps, float* partials, float* mean_rstd,
                                       vqx_stream_t stream) {
  const char* who = "vqx_groupnorm_stats_len";
  int B;
  if (check_lens(who, len, n_rows, T, B)) return -1;
  if (dtype != VQX_F32 && dtype != VQX_BF16) { set_error("%s: bad dtype %d", who, dtype); return -1; }
  const int V = dtype == VQX_BF16 ? 8 : 4;
  if (!x || !partials || !mean_rstd || !al16(x)) { set_error("%s: null or unaligned (16 B) pointer", who); return -1; }
  if ((G != 1 && G != 2) || C < G || C % G || (C / G) % V || ldx % V || ldx < C) {
    set_error("%s: G = %d (1 or 2), C = %d, ldx = %d: C/G and ldx must be multiples of %d, ldx >= C", who, G, C, ldx, V);
    return -1;
  }
  hipStream_t s = (hipStream_t)stream;
  const int64_t esz = dtype == VQX_BF16 ? 2 : 4;
  for (int b0 = 0; b0 < B; b0 += kLenItems) {
    const int n = std::min(kLenItems, B - b0);
    const LenTable L = table_at(len, b0, n);
    const char* xb = (const char*)x + (int64_t)b0 * T * ldx * esz;
    float* pb = partials + (int64_t)b0 * G * kVarParts * 3;
    if (dtype == VQX_BF16)
      hipLaunchKernelGGL(gn_len_partial_kernel<bf16_t>, dim3(kVarParts, n * G), dim3(256), 0, s, (const bf16_t*)xb, ldx,
                         T, C, G, L, pb);
    else
      hipLaunchKernelGGL(gn_len_partial_kernel<float>, dim3(kVarParts, n * G), dim3(256), 0, s, (const float*)xb, ldx, T,
                         C, G, L, pb);
  }
  hipLaunchKernelGGL(gn_len_finalize_kernel, dim3((B * G + 127) / 128), dim3(128), 0, s, partials, B * G, eps, mean_rstd);
  return launch_status(who);
}

extern "C" int vqx_gn_lrelu_fwd_len(const void* h, int32_t ldh, void* g, int32_t ldg, int32_t dtype, int64_t n_rows,
                                    int32_t T, int32_t C, const int32_t* len, const float* mean_rstd, const float* gamma,
                                    const float* beta, vqx_stream_t stream) {
  const char* who = "vqx_gn_lrelu_fwd_len";
  int B;
  if (check_lens(who, len, n_rows, T, B)) return -1;
  if (dtype != VQX_F32 && dtype != VQX_BF16) { set_error("%s: bad dtype %d", who, dtype); return -1; }
  const int V = dtype == VQX_BF16 ? 8 : 4;
  if (!h || !g || !mean_rstd || !gamma || !beta || C < V || C % V || ldh % V || ldg % V || ldh < C || ldg < C ||
      !al16(h) || !al16(g)) {
    set_error("%s: bad arguments (C, strides multiples of %d, ld >= C, 16-B aligned)", who, V);
    return -1;
  }
  const int cpr = C / V;
  hipStream_t s = (hipStream_t)stream;
  const int64_t esz = dtype == VQX_BF16 ? 2 : 4;
  const int gx = blocks_for((int64_t)T * cpr);
  for (int b0 = 0; b0 < B; b0 += kLenItems) {
    const int n = std::min(kLenItems, B - b0);
    const LenTable L = table_at(len, b0, n);
    const char* hb = (const char*)h + (int64_t)b0 * T * ldh * esz;
    char* gb = (char*)g + (int64_t)b0 * T * ldg * esz;
    const float* mr = mean_rstd + (int64_t)b0 * 2;
    if (dtype == VQX_BF16)
      hipLaunchKernelGGL(gn_lrelu_len_kernel<bf16_t>, dim3(gx, n), dim3(256), 0, s, (const bf16_t*)hb, ldh, (bf16_t*)gb,
                         ldg, T, cpr, L, mr, gamma, beta);
    else
      hipLaunchKernelGGL(gn_lrelu_len_kernel<float>, dim3(gx, n), dim3(256), 0, s, (const float*)hb, ldh, (float*)gb,
                         ldg, T, cpr, L, mr, gamma, beta);
  }
  return launch_status(who);
}

extern "C" int vqx_gn_glu_fwd_len(const void* u, int32_t ldu, void* g, int32_t ldg, int32_t dtype, int64_t n_rows,
                                  int32_t T, int32_t C, const int32_t* len, const float* mean_rstd, const float* gamma,
                                  const float* beta, vqx_stream_t stream) {
  const char* who = "vqx_gn_glu_fwd_len";
  int B;
  if (check_lens(who, len, n_rows, T, B)) return -1;
  if (dtype != VQX_F32 && dtype != VQX_BF16) { set_error("%s: bad dtype %d", who, dtype); return -1; }
  const int V = dtype == VQX_BF16 ? 8 : 4;
  if (!u || !g || !mean_rstd || !gamma || !beta || C < 2 * V || C % 2 || (C / 2) % V || ldu % V || ldg % V || ldu < C ||
      ldg < C / 2 || !al16(u) || !al16(g)) {
    set_error("%s: bad arguments (C/2, strides multiples of %d, ldu >= C, ldg >= C/2, 16-B aligned)", who, V);
    return -1;
  }
  const int half = C / 2, cpr = half / V;
  hipStream_t s = (hipStream_t)stream;
  const int64_t esz = dtype == VQX_BF16 ? 2 : 4;
  const int gx = blocks_for((int64_t)T * cpr);
  for (int b0 = 0; b0 < B; b0 += kLenItems) {
    const int n = std::min(kLenItems, B - b0);
    const LenTable L = table_at(len, b0, n);
    const char* ub = (const char*)u + (int64_t)b0 * T * ldu * esz;
    char* gb = (char*)g + (int64_t)b0 * T * ldg * esz;
    const float* mr = mean_rstd + (int64_t)b0 * 4;
    if (dtype == VQX_BF16)
      hipLaunchKernelGGL(gn_glu_len_kernel<bf16_t>, dim3(gx, n), dim3(256), 0, s, (const bf16_t*)ub, ldu, (bf16_t*)gb,
                         ldg, T, half, cpr, L, mr, gamma, beta);
    else
      hipLaunchKernelGGL(gn_glu_len_kernel<float>, dim3(gx, n), dim3(256), 0, s, (const float*)ub, ldu, (float*)gb, ldg,
                         T, half, cpr, L, mr, gamma, beta);
  }
  return launch_status(who);
}

extern "C" int vqx_mask_tail(void* x, int32_t ldx, int32_t dtype, int64_t n_rows, int32_t T, int32_t C,
                             const int32_t* len, vqx_stream_t stream) {
  const char* who = "vqx_mask_tail";
  int B;
  if (check_lens(who, len, n_rows, T, B)) return -1;
  if (dtype != VQX_F32 && dtype != VQX_BF16) { set_error("%s: bad dtype %d", who, dtype); return -1; }
  const int V = dtype == VQX_BF16 ? 8 : 4;
  if (!x || !al16(x) || C < V || C % V || ldx % V || ldx < C) {
    set_error("%s: bad arguments (C, ldx multiples of %d, ldx >= C, 16-B aligned)", who, V);
    return -1;
  }
  const int cpr = C / V;
  const int64_t ldq = ldx / V;
  hipStream_t s = (hipStream_t)stream;
  for (int b0 = 0; b0 < B; b0 += kLenItems) {
    const int n = std::min(kLenItems, B - b0);
    int longest = 0;
    for (int b = b0; b < b0 + n; ++b) longest = std::max(longest, T - len[b]);
    if (!longest) continue;  // no tail in this launch's utterances
    const LenTable L = table_at(len, b0, n);
    hipLaunchKernelGGL(mask_tail_kernel, dim3(blocks_for((int64_t)longest * cpr), n), dim3(256), 0, s,
                       (uint4*)x + (int64_t)b0 * T * ldq, ldq, T, cpr, L);
  }
  return launch_status(who);
}

extern "C" int vqx_codes_upsample_cat_len(const vqx_codes_level* levels, int32_t n_levels, int32_t B, int32_t T,
                                          const int32_t* n_len, const int32_t* m_len, void* out, int32_t ldo,
                                          int32_t out_dtype, vqx_stream_t stream) {
  const char* who = "vqx_codes_upsample_cat_len";
  if (!levels || !n_len || !m_len) { set_error("%s: null levels or lengths", who); return -1; }
  if (n_levels < 1 || n_levels > kCatLevels) { set_error("%s: n_levels = %d not in 1..%d", who, n_levels, kCatLevels); return -1; }
  if (out_dtype != VQX_F32 && out_dtype != VQX_BF16) { set_error("%s: bad dtype %d", who, out_dtype); return -1; }
  if (B < 1 || T < 1 || (int64_t)B * T > INT32_MAX) { set_error("%s: B = %d, T = %d (B*T must fit 31 bits)", who, B, T); return -1; }
  if (!out || !al16(out)) { set_error("%s: null or unaligned (16 B) out pointer", who); return -1; }
  CatLevels L = {};
  L.n = n_levels;
  int total = 0;
  for (int l = 0; l < n_levels; ++l) {
    const vqx_codes_level& v = levels[l];
    if (!v.z || !al16(v.z)) { set_error("%s: level %d: null or unaligned (16 B) %s pointer", who, l, v.idx ? "codebook" : "z"); return -1; }
    if (v.idx && !al16(v.idx)) { set_error("%s: level %d: unaligned (16 B) idx pointer", who, l); return -1; }
    if (v.T_l < 1 || v.T_l > T) { set_error("%s: level %d: T_l = %d not in 1..T = %d", who, l, v.T_l, T); return -1; }
    if (v.C < 4 || v.C % 4 || v.ld % 4 || v.ld < v.C) { set_error("%s: level %d: C = %d / ld = %d must be multiples of 4, ld >= C", who, l, v.C, v.ld); return -1; }
    if (v.idx && v.K < 1) { set_error("%s: level %d: K = %d codes", who, l, v.K); return -1; }
    if ((int64_t)total + v.C > INT32_MAX) { set_error("%s: channel sum overflows", who); return -1; }
    L.src[l] = (const float*)v.z;
    L.idx[l] = v.idx;
    L.T_l[l] = v.T_l;
    L.ld[l] = v.ld;
    L.gran[l] = v.C / 4;
    L.off[l] = total;
    L.normalize[l] = v.idx && v.normalize;
    total += v.C;
  }
  if (ldo % 4 || total > ldo) { set_error("%s: sum of C_l = %d exceeds ldo = %d (ldo a multiple of 4)", who, total, ldo); return -1; }
  for (int b = 0; b < B; ++b) {  // every item before any launch: the kernel trusts the lengths
    if (n_len[b] < 1 || n_len[b] > T) { set_error("%s: item %d: length %d outside [1, T = %d]", who, b, n_len[b], T); return -1; }
    for (int l = 0; l < n_levels; ++l) {
      const int m = m_len[(int64_t)b * n_levels + l];
      if (m < 1 || m > n_len[b] || m > levels[l].T_l) {
        set_error("%s: item %d: level %d: length %d outside [1, min(%d, T_l = %d)]", who, b, l, m, n_len[b], levels[l].T_l);
        return -1;
      }
    }
  }
  hipStream_t s = (hipStream_t)stream;
  auto* fn = out_dtype == VQX_BF16 ? codes_cat_len_kernel<true> : codes_cat_len_kernel<false>;
  for (int b0 = 0; b0 < B; b0 += kCatItems) {
    const int n = std::min(kCatItems, B - b0);
    CatLens N = {};
    for (int b = 0; b < n; ++b) {
      N.n[b] = n_len[b0 + b];
      for (int l = 0; l < n_levels; ++l) N.m[b][l] = m_len[(int64_t)(b0 + b) * n_levels + l];
      for (int l = n_levels; l < kCatLevels; ++l) N.m[b][l] = 1;
    }
    hipLaunchKernelGGL(fn, dim3((T + kCatWaves - 1) / kCatWaves, n), dim3(kCatWaves * 64), 0, s, L, N, b0, T, total, out,
                       (int64_t)ldo);
  }
  return launch_status(who);
}

extern "C" int vqx_segment_mean(const float* z, int32_t ldz, int64_t n_rows, int32_t T, int32_t C, const int32_t* len,
                                float* out, int32_t ldo, vqx_stream_t stream) {
  const char* who = "vqx_segment_mean";
  int B;
  if (check_lens(who, len, n_rows, T, B)) return -1;
  if (!z || !out || !al16(z) || !al16(out) || C < 4 || C % 4 || ldz % 4 || ldo % 4 || ldz < C || ldo < C) {
    set_error("%s: bad arguments (C, strides multiples of 4, ld >= C, 16-B aligned f32)", who);
    return -1;
  }
  hipStream_t s = (hipStream_t)stream;
  for (int b0 = 0; b0 < B; b0 += kLenItems) {
    const int n = std::min(kLenItems, B - b0);
    const LenTable L = table_at(len, b0, n);
    hipLaunchKernelGGL(segment_mean_kernel, dim3((C + 63) / 64, n), dim3(256), 0, s, z + (int64_t)b0 * T * ldz,
                       (int64_t)ldz, T, C, L, out + (int64_t)b0 * ldo, (int64_t)ldo);
  }
  return launch_status(who);
}

extern "C" int vqx_nct_to_ntc_len(const float* x_nct, int32_t B, int32_t C, int32_t T, const int32_t* len, void* y,
                                  int32_t ldy, int32_t dtype, vqx_stream_t stream) {
  const char* who = "vqx_nct_to_ntc_len";
  int Bc;
  if (check_layout(who, x_nct, y, B, C, T, ldy, dtype, len, Bc)) return -1;
  hipStream_t s = (hipStream_t)stream;
  const int64_t esz = dtype == VQX_BF16 ? 2 : 4;
  for (int b0 = 0; b0 < B; b0 += kLenItems) {
    const int n = std::min(kLenItems, B - b0);
    const LenTable L = table_at(len, b0, n);
    const dim3 grid((unsigned)((T + 31) / 32), (unsigned)((C + 31) / 32), (unsigned)n);
    const float* xb = x_nct + (int64_t)b0 * C * T;
    char* yb = (char*)y + (int64_t)b0 * T * ldy * esz;
    if (dtype == VQX_BF16)
      hipLaunchKernelGGL(nct_to_ntc_len_kernel<bf16_t>, grid, dim3(256), 0, s, xb, C, T, L, (bf16_t*)yb, (int64_t)ldy);
    else
      hipLaunchKernelGGL(nct_to_ntc_len_kernel<float>, grid, dim3(256), 0, s, xb, C, T, L, (float*)yb, (int64_t)ldy);
  }
  return launch_status(who);
}

extern "C" int vqx_ntc_to_nct_len(const void* y, int32_t ldy, int32_t dtype, int32_t B, int32_t C, int32_t T,
                                  const int32_t* len, float* x_nct, int32_t T_out, vqx_stream_t stream) {
  const char* who = "vqx_ntc_to_nct_len";
  int Bc;
  if (check_layout(who, x_nct, y, B, C, T, ldy, dtype, len, Bc)) return -1;
  if (T_out < 1 || T_out > T) { set_error("%s: T_out = %d outside [1, T = %d]", who, T_out, T); return -1; }
  hipStream_t s = (hipStream_t)stream;
  const int64_t esz = dtype == VQX_BF16 ? 2 : 4;
  for (int b0 = 0; b0 < B; b0 += kLenItems) {
    const int n = std::min(kLenItems, B - b0);
    const LenTable L = table_at(len, b0, n);
    const dim3 grid((unsigned)((T_out + 31) / 32), (unsigned)((C + 31) / 32), (unsigned)n);
    const char* yb = (const char*)y + (int64_t)b0 * T * ldy * esz;
    float* xb = x_nct + (int64_t)b0 * C * T_out;
    if (dtype == VQX_BF16)
      hipLaunchKernelGGL(ntc_to_nct_len_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)yb, (int64_t)ldy, C, T, L,
                         xb, T_out);
    else
      hipLaunchKernelGGL(ntc_to_nct_len_kernel<float>, grid, dim3(256), 0, s, (const float*)yb, (int64_t)ldy, C, T, L, xb,
                         T_out);
  }
  return launch_status(who);
}

extern "C" int vqx_nct_to_ntc_pad_len(const float* x_nct, int32_t B, int32_t C, int32_t T_in, int32_t T,
                                      const int32_t* len, void* y, int32_t ldy, int32_t dtype, vqx_stream_t stream) {
  const char* who = "vqx_nct_to_ntc_pad_len";
  int Bc;
  if (check_layout(who, x_nct, y, B, C, T_in, ldy, dtype, len, Bc)) return -1;  // len[b] in 1..T_in
  if (T < T_in || (int64_t)B * T > INT32_MAX) {
    set_error("%s: T = %d rows an utterance for T_in = %d frames (T >= T_in, B*T below 2^31)", who, T, T_in);
    return -1;
  }
  hipStream_t s = (hipStream_t)stream;
  const int64_t esz = dtype == VQX_BF16 ? 2 : 4;
  for (int b0 = 0; b0 < B; b0 += kLenItems) {
    const int n = std::min(kLenItems, B - b0);
    const LenTable L = table_at(len, b0, n);
    const dim3 grid((unsigned)((T + 31) / 32), (unsigned)((C + 31) / 32), (unsigned)n);
    const float* xb = x_nct + (int64_t)b0 * C * T_in;
    char* yb = (char*)y + (int64_t)b0 * T * ldy * esz;
    if (dtype == VQX_BF16)
      hipLaunchKernelGGL(nct_to_ntc_pad_len_kernel<bf16_t>, grid, dim3(256), 0, s, xb, C, T_in, T, L, (bf16_t*)yb,
                         (int64_t)ldy);
    else
      hipLaunchKernelGGL(nct_to_ntc_pad_len_kernel<float>, grid, dim3(256), 0, s, xb, C, T_in, T, L, (float*)yb,
                         (int64_t)ldy);
  }
  return launch_status(who);
}

extern "C" int vqx_index_mask_len(const int64_t* idx, int32_t B, int32_t T, const int32_t* len, int64_t* out,
                                  int32_t T_out, vqx_stream_t stream) {
  const char* who = "vqx_index_mask_len";
  if (B < 1 || T < 1) { set_error("%s: B = %d, T = %d", who, B, T); return -1; }
  if (T_out < 1 || T_out > T) { set_error("%s: T_out = %d outside [1, T = %d]", who, T_out, T); return -1; }
  if ((int64_t)B * T > INT32_MAX) { set_error("%s: B*T = %lld must fit 31 bits", who, (long long)B * T); return -1; }
  int Bc;
  if (check_lens(who, len, (int64_t)B * T_out, T_out, Bc)) return -1;  // len[b] in 1..T_out
  if (!idx || !out || ((uintptr_t)idx & 7) || ((uintptr_t)out & 7)) {
    set_error("%s: null or unaligned (8 B) pointer", who);
    return -1;
  }
  hipStream_t s = (hipStream_t)stream;
  for (int b0 = 0; b0 < B; b0 += kLenItems) {
    const int n = std::min(kLenItems, B - b0);
    const LenTable L = table_at(len, b0, n);
    hipLaunchKernelGGL(index_mask_len_kernel, dim3(blocks_for(T_out), n), dim3(256), 0, s, idx + (int64_t)b0 * T, T, L,
                       out + (int64_t)b0 * T_out, T_out);
  }
  return launch_status(who);
}
