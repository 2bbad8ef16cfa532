// Self-attention over latent frames (include/vqx.h vqx_attn_*; reference
// model/layers_gst.py:63-147 called as mha(x, x, x, key mask)): the softmax
// part between the q/k/v GEMM and the output GEMM, forward in 1 launch and
// backward in 3, on MFMA in both compute dtypes.
//
//   forward   attn_fwd_kernel    one workgroup per (64 queries, head, utterance):
//                                streams the keys in tiles of at_ts() rows with
//                                an online softmax; writes ctx and lse
//   backward  attn_delta_kernel  delta[b][h][t] = sum_d d_ctx . ctx
//             attn_dkv_kernel    one workgroup per (64 keys, head, utterance):
//                                dK and dV stay in its accumulators while it
//                                sweeps the query tiles
//             attn_dq_kernel     one workgroup per (64 queries, head,
//                                utterance): dQ stays in its accumulators while
//                                it sweeps the key tiles
// Each backward kernel owns its outputs and recomputes P = exp(S - lse), so
// nothing is summed across workgroups: no atomics, equal arguments give equal
// bits.
//
// A workgroup is 4 waves and a wave owns 16 of the workgroup's 64 rows; its
// operand of those rows (Q, or K and V, or Q and dO) lives in registers, read
// from global memory once.  The streamed tile goes through LDS, row-major for
// the products that sum over d and transposed ([d][row]) for those that sum
// over the tile's rows.  MFMA shapes: 16x16x32 bf16 and 16x16x4 f32; one
// "k-chunk" is 64 bytes of the summed index, of which the lane group
// g = lane >> 4 holds bytes [16g, 16g + 16) of both operands (the f32 form
// issues 4 instructions a chunk, element j of the 16 bytes in instruction j).
// The accumulator holds row 4g + i (i = register) and column lane & 15, so a
// query row's maximum and sum are reductions over the 16 lanes of a group.
// P and dS go from the accumulators to the next product's operand through a
// wave-private LDS tile.
//
// Lengths: host values, validated item by item, passed by value (AttnLens,
// 896 utterances a launch, as vqx_varlen.hip).  Rows t >= len[b] are selected
// zeros and never loaded; keys t2 >= len[b] get weight 0; ctx and d_qkv rows
// t >= len[b] are stored as zeros.
#include <math.h>

#include "vqx_common.h"

namespace vqx {
namespace {

constexpr int AT_THREADS = 256;
constexpr int AT_OWN = 64;  // rows a workgroup owns: 16 a wave
constexpr int kAttnItems = 896;
struct AttnLens {
  int32_t len[kAttnItems];
};
static_assert(sizeof(AttnLens) + 256 <= 4096, "AttnLens and the other arguments must fit the 4 KB kernel-argument segment");

struct AttnDev {
  const void* qkv;
  void* ctx;
  float* lse;
  const void* d_ctx;
  void* d_qkv;
  float* delta;
  int T, F, H, b0;
  int64_t ldqkv, ldc;
  float scale;
};

template <typename T> struct Mma;
template <> struct Mma<bf16_t> {
  static constexpr int V = 8;    // elements of a 16-byte chunk
  static constexpr int KC = 32;  // elements of a k-chunk (64 bytes)
  __device__ static __forceinline__ void mma(f32x4_t& acc, const uint4& a, const uint4& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), acc,
                                                  0, 0, 0);
  }
  __device__ static __forceinline__ bf16_t from(float f) { return f2bf(f); }
  __device__ static __forceinline__ bf16_t get(const uint4& u, int k) {  // element k of a chunk (k a constant)
    const unsigned w[4] = {u.x, u.y, u.z, u.w};
    return (bf16_t)(w[k >> 1] >> (16 * (k & 1)));
  }
  __device__ static __forceinline__ float getf(const uint4& u, int k) { return bf2f(get(u, k)); }
  __device__ static __forceinline__ float exp_(float x) { return __expf(x); }
};
template <> struct Mma<float> {
  static constexpr int V = 4;
  static constexpr int KC = 16;
  __device__ static __forceinline__ void mma(f32x4_t& acc, const uint4& a, const uint4& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
  }
  __device__ static __forceinline__ float from(float f) { return f; }
  __device__ static __forceinline__ float get(const uint4& u, int k) {
    const unsigned w[4] = {u.x, u.y, u.z, u.w};
    return __uint_as_float(w[k]);
  }
  __device__ static __forceinline__ float getf(const uint4& u, int k) { return get(u, k); }
  __device__ static __forceinline__ float exp_(float x) { return expf(x); }  // the parity mode
};

// rows of the streamed tile: 128 bytes of the compute dtype (2 k-chunks)
template <typename T> constexpr int at_ts() { return 128 / (int)sizeof(T); }
// row stride of an LDS image of `cols` elements: 16 bytes of padding, so that
// the 16 rows a lane group reads start 4 banks apart
template <typename T> constexpr int at_ld(int cols) { return cols + 16 / (int)sizeof(T); }

// acc[n] += A (16 rows x KCH k-chunks, the wave's fragments) . Bm^T, Bm an LDS
// image [16 * NB rows][ldb] whose rows are the product's columns
template <typename T, int NB, int KCH>
__device__ __forceinline__ void wave_mma(f32x4_t (&acc)[NB], const uint4 (&a)[KCH], const T* bm, int ldb, int lane) {
  const int r = lane & 15, g = lane >> 4;
#pragma unroll
  for (int kc = 0; kc < KCH; ++kc)
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      const uint4 b = *(const uint4*)(bm + (n * 16 + r) * ldb + kc * Mma<T>::KC + g * Mma<T>::V);
      Mma<T>::mma(acc[n], a[kc], b);
    }
}

// The wave's fragments of 16 rows x (KCH k-chunks) of a global row-major
// matrix: row `row` (this lane's, valid or a selected zero), columns from p.
template <typename T, int KCH>
__device__ __forceinline__ void load_frag(uint4 (&f)[KCH], const T* p, bool valid, int lane) {
  const int g = lane >> 4;
#pragma unroll
  for (int kc = 0; kc < KCH; ++kc)
    f[kc] = valid ? *(const uint4*)(p + kc * Mma<T>::KC + g * Mma<T>::V) : make_uint4(0u, 0u, 0u, 0u);
}

// The wave's fragments of its private LDS tile [16][ld] over NK k-chunks.
template <typename T, int NK>
__device__ __forceinline__ void lds_frag(uint4 (&f)[NK], const T* tile, int ld, int lane) {
  const int r = lane & 15, g = lane >> 4;
#pragma unroll
  for (int kc = 0; kc < NK; ++kc) f[kc] = *(const uint4*)(tile + r * ld + kc * Mma<T>::KC + g * Mma<T>::V);
}

// Rows t0 .. t0 + TS of head columns src (row stride ld elements) into the LDS
// images `rowm` [TS][LDR] (nullptr: none) and `tr` [D][LDT] (nullptr: none);
// rows t >= lim are selected zeros and not loaded.
template <typename T, int D>
__device__ __forceinline__ void stage_tile(const T* __restrict__ src, int64_t ld, int t0, int lim, T* rowm, T* tr) {
  constexpr int V = Mma<T>::V, TS = at_ts<T>(), CPR = D / V, LDR = at_ld<T>(D), LDT = at_ld<T>(TS);
  for (int i = threadIdx.x; i < TS * CPR; i += AT_THREADS) {
    const int row = i / CPR, ch = i - row * CPR;
    const int t = t0 + row;
    uint4 u = make_uint4(0u, 0u, 0u, 0u);
    if (t < lim) u = *(const uint4*)(src + (int64_t)t * ld + ch * V);
    if (rowm) *(uint4*)(rowm + row * LDR + ch * V) = u;
    if (tr) {
#pragma unroll
      for (int k = 0; k < V; ++k) tr[(ch * V + k) * LDT + row] = Mma<T>::get(u, k);
    }
  }
}

__device__ __forceinline__ float group_max(float v) {  // over the 16 lanes of a lane group
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// grid (ceil(T / 64), H, utterances of the launch)
template <typename T, int D>
__global__ __launch_bounds__(AT_THREADS) void attn_fwd_kernel(AttnDev a, AttnLens L) {
  constexpr int V = Mma<T>::V, KC = Mma<T>::KC, TS = at_ts<T>(), KD = D / KC, NS = TS / 16, ND = D / 16;
  constexpr int LDK = at_ld<T>(D), LDT = at_ld<T>(TS);
  __shared__ __attribute__((aligned(16))) T sK[TS * LDK];
  __shared__ __attribute__((aligned(16))) T sVt[D * LDT];
  __shared__ __attribute__((aligned(16))) T sP[4][16 * LDT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, bl = blockIdx.z;
  const int64_t b = a.b0 + bl;
  const int len = L.len[bl];
  const int q0 = blockIdx.x * AT_OWN + wave * 16;
  const T* qkv = (const T*)a.qkv + b * a.T * a.ldqkv + h * D;

  uint4 qf[KD];
  load_frag<T, KD>(qf, qkv + (int64_t)(q0 + r) * a.ldqkv, q0 + r < len, lane);
  f32x4_t o[ND];
#pragma unroll
  for (int n = 0; n < ND; ++n) o[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m[4], l[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { m[i] = -INFINITY; l[i] = 0.f; }

  const bool live = (int)blockIdx.x * AT_OWN < len;  // a tile wholly past the end only stores zeros
  for (int j0 = 0; live && j0 < len; j0 += TS) {
    __syncthreads();  // the previous tile's readers are done
    stage_tile<T, D>(qkv + a.F, a.ldqkv, j0, len, sK, nullptr);
    stage_tile<T, D>(qkv + 2 * a.F, a.ldqkv, j0, len, nullptr, sVt);
    __syncthreads();
    f32x4_t s[NS];
#pragma unroll
    for (int n = 0; n < NS; ++n) s[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    wave_mma<T, NS, KD>(s, qf, sK, LDK, lane);
    float mx[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) mx[i] = -INFINITY;
#pragma unroll
    for (int n = 0; n < NS; ++n) {
      const bool key = j0 + n * 16 + r < len;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s[n][i] = key ? s[n][i] * a.scale : -INFINITY;
        mx[i] = fmaxf(mx[i], s[n][i]);
      }
    }
    float alpha[4], sum[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float mn = fmaxf(m[i], group_max(mx[i]));  // finite: key j0 is valid
      alpha[i] = Mma<T>::exp_(m[i] - mn);
      m[i] = mn;
      sum[i] = 0.f;
    }
    T* pw = sP[wave];
#pragma unroll
    for (int n = 0; n < NS; ++n)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = Mma<T>::exp_(s[n][i] - m[i]);
        sum[i] += p;
        pw[(4 * g + i) * LDT + n * 16 + r] = Mma<T>::from(p);
      }
#pragma unroll
    for (int i = 0; i < 4; ++i) l[i] = l[i] * alpha[i] + group_sum(sum[i]);
#pragma unroll
    for (int n = 0; n < ND; ++n)
#pragma unroll
      for (int i = 0; i < 4; ++i) o[n][i] *= alpha[i];
    __syncthreads();  // P is in LDS
    uint4 pf[TS / KC];
    lds_frag<T, TS / KC>(pf, pw, LDT, lane);
    wave_mma<T, ND, TS / KC>(o, pf, sVt, LDT, lane);
  }

  T* ctx = (T*)a.ctx + b * a.T * a.ldc + h * D;
  float* lse = a.lse + (b * a.H + h) * a.T;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int t = q0 + 4 * g + i;
    if (t >= a.T) continue;
    const bool valid = t < len;
    const float inv = valid ? 1.f / l[i] : 0.f;
#pragma unroll
    for (int n = 0; n < ND; ++n) ctx[(int64_t)t * a.ldc + n * 16 + r] = Mma<T>::from(valid ? o[n][i] * inv : 0.f);
    if (r == 0) lse[t] = valid ? m[i] + logf(l[i]) : 0.f;
  }
}

// delta[b][h][t] = sum_d d_ctx . ctx, 0 for t >= len[b].  The sum is an fmaf
// chain from 0.f in the order Mma<float>::mma sums a k-chunk (element j of the
// lane groups g = 0..3, then j + 1), which is the order of the dP = dO . v
// products of the two kernels below: where ctx equals v (one key), dP - delta
// is exactly zero in the f32 mode, as the softmax over one key demands.
// grid (ceil(T * H / 256), 1, utterances)
template <typename T, int D>
__global__ __launch_bounds__(AT_THREADS) void attn_delta_kernel(AttnDev a, AttnLens L) {
  constexpr int V = Mma<T>::V, KC = Mma<T>::KC;
  const int bl = blockIdx.z;
  const int64_t b = a.b0 + bl;
  const int len = L.len[bl];
  const int i = blockIdx.x * AT_THREADS + threadIdx.x;  // T * H < 2^31 (attn_dims_ok)
  if (i >= a.T * a.H) return;
  const int t = i / a.H, h = i - t * a.H;
  float s = 0.f;
  if (t < len) {
    const T* c = (const T*)a.ctx + (b * a.T + t) * a.ldc + h * D;
    const T* d = (const T*)a.d_ctx + (b * a.T + t) * a.ldc + h * D;
#pragma unroll
    for (int kc = 0; kc < D / KC; ++kc) {
      uint4 cu[4], du[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        cu[g] = *(const uint4*)(c + kc * KC + g * V);
        du[g] = *(const uint4*)(d + kc * KC + g * V);
      }
#pragma unroll
      for (int k = 0; k < V; ++k)
#pragma unroll
        for (int g = 0; g < 4; ++g) s = fmaf(Mma<T>::getf(du[g], k), Mma<T>::getf(cu[g], k), s);
    }
  }
  a.delta[(b * a.H + h) * a.T + t] = s;
}

// rows t0 .. t0 + 64 (below T) of d_qkv's `part` (0 q, 1 k, 2 v), head h: zeros
template <typename T, int D>
__device__ __forceinline__ void zero_rows(const AttnDev& a, int64_t b, int h, int part, int t0) {
  constexpr int V = Mma<T>::V, CPR = D / V;
  T* dst = (T*)a.d_qkv + b * a.T * a.ldqkv + part * a.F + h * D;
  for (int i = threadIdx.x; i < AT_OWN * CPR; i += AT_THREADS) {
    const int row = i / CPR, ch = i - row * CPR;
    if (t0 + row < a.T) *(uint4*)(dst + (int64_t)(t0 + row) * a.ldqkv + ch * V) = make_uint4(0u, 0u, 0u, 0u);
  }
}

// The accumulators of the wave's 16 rows (first row t0) x D columns to dst
// (row stride ld); rows t >= len are zeros, rows t >= T are not stored.
template <typename T, int ND>
__device__ __forceinline__ void store_acc(const f32x4_t (&acc)[ND], T* dst, int64_t ld, int t0, int len, int T_,
                                          int lane) {
  const int r = lane & 15, g = lane >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int t = t0 + 4 * g + i;
    if (t >= T_) continue;
#pragma unroll
    for (int n = 0; n < ND; ++n) dst[(int64_t)t * ld + n * 16 + r] = Mma<T>::from(t < len ? acc[n][i] : 0.f);
  }
}

// grid (ceil(T / 64) key tiles, H, utterances)
template <typename T, int D>
__global__ __launch_bounds__(AT_THREADS) void attn_dkv_kernel(AttnDev a, AttnLens L) {
  constexpr int KC = Mma<T>::KC, TS = at_ts<T>(), KD = D / KC, NS = TS / 16, ND = D / 16;
  constexpr int LDR = at_ld<T>(D), LDT = at_ld<T>(TS);
  __shared__ __attribute__((aligned(16))) T sQ[TS * LDR];
  __shared__ __attribute__((aligned(16))) T sdO[TS * LDR];
  __shared__ __attribute__((aligned(16))) T sQt[D * LDT];
  __shared__ __attribute__((aligned(16))) T sdOt[D * LDT];
  __shared__ __attribute__((aligned(16))) T sPt[4][16 * LDT];
  __shared__ __attribute__((aligned(16))) T sdSt[4][16 * LDT];
  __shared__ float sLse[TS], sDel[TS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, bl = blockIdx.z;
  const int64_t b = a.b0 + bl;
  const int len = L.len[bl];
  const int k0 = blockIdx.x * AT_OWN;
  if (k0 >= len) {
    zero_rows<T, D>(a, b, h, 1, k0);
    zero_rows<T, D>(a, b, h, 2, k0);
    return;
  }
  const int kw = k0 + wave * 16;
  const T* qkv = (const T*)a.qkv + b * a.T * a.ldqkv + h * D;
  const T* dctx = (const T*)a.d_ctx + b * a.T * a.ldc + h * D;
  const float* lse = a.lse + (b * a.H + h) * a.T;
  const float* delta = a.delta + (b * a.H + h) * a.T;
  uint4 kf[KD], vf[KD];
  load_frag<T, KD>(kf, qkv + a.F + (int64_t)(kw + r) * a.ldqkv, kw + r < len, lane);
  load_frag<T, KD>(vf, qkv + 2 * a.F + (int64_t)(kw + r) * a.ldqkv, kw + r < len, lane);
  f32x4_t dk[ND], dv[ND];
#pragma unroll
  for (int n = 0; n < ND; ++n) dk[n] = dv[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  for (int i0 = 0; i0 < len; i0 += TS) {
    __syncthreads();
    stage_tile<T, D>(qkv, a.ldqkv, i0, len, sQ, sQt);
    stage_tile<T, D>(dctx, a.ldc, i0, len, sdO, sdOt);
    if (threadIdx.x < TS) {
      const int t = i0 + threadIdx.x;
      sLse[threadIdx.x] = t < len ? lse[t] : 0.f;
      sDel[threadIdx.x] = t < len ? delta[t] : 0.f;
    }
    __syncthreads();
    f32x4_t st[NS], dp[NS];  // rows: the wave's keys; columns: the tile's queries
#pragma unroll
    for (int n = 0; n < NS; ++n) st[n] = dp[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    wave_mma<T, NS, KD>(st, kf, sQ, LDR, lane);
    wave_mma<T, NS, KD>(dp, vf, sdO, LDR, lane);
    T* pw = sPt[wave];
    T* dw = sdSt[wave];
#pragma unroll
    for (int n = 0; n < NS; ++n) {
      const int qc = n * 16 + r;
      const bool qv = i0 + qc < len;
      const float ls = sLse[qc], de = sDel[qc];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool ok = qv && kw + 4 * g + i < len;
        const float p = ok ? Mma<T>::exp_(st[n][i] * a.scale - ls) : 0.f;
        const float ds = p * (dp[n][i] - de) * a.scale;
        pw[(4 * g + i) * LDT + qc] = Mma<T>::from(p);
        dw[(4 * g + i) * LDT + qc] = Mma<T>::from(ds);
      }
    }
    __syncthreads();
    uint4 pf[TS / KC], df[TS / KC];
    lds_frag<T, TS / KC>(pf, pw, LDT, lane);
    lds_frag<T, TS / KC>(df, dw, LDT, lane);
    wave_mma<T, ND, TS / KC>(dv, pf, sdOt, LDT, lane);
    wave_mma<T, ND, TS / KC>(dk, df, sQt, LDT, lane);
  }
  T* dqkv = (T*)a.d_qkv + b * a.T * a.ldqkv + h * D;
  store_acc<T, ND>(dk, dqkv + a.F, a.ldqkv, kw, len, a.T, lane);
  store_acc<T, ND>(dv, dqkv + 2 * a.F, a.ldqkv, kw, len, a.T, lane);
}

// grid (ceil(T / 64) query tiles, H, utterances)
template <typename T, int D>
__global__ __launch_bounds__(AT_THREADS) void attn_dq_kernel(AttnDev a, AttnLens L) {
  constexpr int KC = Mma<T>::KC, TS = at_ts<T>(), KD = D / KC, NS = TS / 16, ND = D / 16;
  constexpr int LDR = at_ld<T>(D), LDT = at_ld<T>(TS);
  __shared__ __attribute__((aligned(16))) T sK[TS * LDR];
  __shared__ __attribute__((aligned(16))) T sV[TS * LDR];
  __shared__ __attribute__((aligned(16))) T sKt[D * LDT];
  __shared__ __attribute__((aligned(16))) T sdS[4][16 * LDT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, bl = blockIdx.z;
  const int64_t b = a.b0 + bl;
  const int len = L.len[bl];
  const int q0 = blockIdx.x * AT_OWN;
  if (q0 >= len) {
    zero_rows<T, D>(a, b, h, 0, q0);
    return;
  }
  const int qw = q0 + wave * 16;
  const T* qkv = (const T*)a.qkv + b * a.T * a.ldqkv + h * D;
  const T* dctx = (const T*)a.d_ctx + b * a.T * a.ldc + h * D;
  uint4 qf[KD], dof[KD];
  load_frag<T, KD>(qf, qkv + (int64_t)(qw + r) * a.ldqkv, qw + r < len, lane);
  load_frag<T, KD>(dof, dctx + (int64_t)(qw + r) * a.ldc, qw + r < len, lane);
  float ls[4], de[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int t = qw + 4 * g + i;
    ls[i] = t < len ? a.lse[(b * a.H + h) * a.T + t] : 0.f;
    de[i] = t < len ? a.delta[(b * a.H + h) * a.T + t] : 0.f;
  }
  f32x4_t dq[ND];
#pragma unroll
  for (int n = 0; n < ND; ++n) dq[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  for (int j0 = 0; j0 < len; j0 += TS) {
    __syncthreads();
    stage_tile<T, D>(qkv + a.F, a.ldqkv, j0, len, sK, sKt);
    stage_tile<T, D>(qkv + 2 * a.F, a.ldqkv, j0, len, sV, nullptr);
    __syncthreads();
    f32x4_t s[NS], dp[NS];
#pragma unroll
    for (int n = 0; n < NS; ++n) s[n] = dp[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    wave_mma<T, NS, KD>(s, qf, sK, LDR, lane);
    wave_mma<T, NS, KD>(dp, dof, sV, LDR, lane);
    T* dw = sdS[wave];
#pragma unroll
    for (int n = 0; n < NS; ++n) {
      const bool key = j0 + n * 16 + r < len;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool ok = key && qw + 4 * g + i < len;
        const float p = ok ? Mma<T>::exp_(s[n][i] * a.scale - ls[i]) : 0.f;
        dw[(4 * g + i) * LDT + n * 16 + r] = Mma<T>::from(p * (dp[n][i] - de[i]) * a.scale);
      }
    }
    __syncthreads();
    uint4 df[TS / KC];
    lds_frag<T, TS / KC>(df, dw, LDT, lane);
    wave_mma<T, ND, TS / KC>(dq, df, sKt, LDT, lane);
  }
  store_acc<T, ND>(dq, (T*)a.d_qkv + b * a.T * a.ldqkv + h * D, a.ldqkv, qw, len, a.T, lane);
}

bool attn_dims_ok(const char* who, int64_t B, int64_t T, int F, int H, int dtype) {
  if (B < 1 || T < 1 || B * T > INT32_MAX) {
    set_error("%s: B = %lld and T = %lld must be >= 1 with B * T < 2^31", who, (long long)B, (long long)T);
    return false;
  }
  if (dtype != VQX_F32 && dtype != VQX_BF16) { set_error("%s: dtype %d is neither VQX_F32 nor VQX_BF16 (fp8 is not built)", who, dtype); return false; }
  if (F < 1 || H < 1 || F % H) { set_error("%s: F = %d must be a positive multiple of H = %d", who, F, H); return false; }
  if (F / H != 32 && F / H != 64) { set_error("%s: d_k = F / H = %d is not 32 or 64", who, F / H); return false; }
  if (H > 65535 || T * H > INT32_MAX) { set_error("%s: H = %d exceeds 65535 or T * H exceeds 2^31 - 1", who, H); return false; }
  return true;
}

bool attn_args_ok(const char* who, const vqx_attn_args* a, bool bwd) {
  if (!a) { set_error("%s: null args", who); return false; }
  if (!attn_dims_ok(who, a->B, a->T, a->F, a->H, a->dtype)) return false;
  const int esz = a->dtype == VQX_BF16 ? 2 : 4, chunk = 16 / esz;
  if (a->ldqkv < 3 * a->F || a->ldc < a->F || a->ldqkv % chunk || a->ldc % chunk) {
    set_error("%s: ldqkv = %d (>= 3F = %d) and ldc = %d (>= F) must be multiples of the 16-byte chunk (%d elements)", who,
              a->ldqkv, 3 * a->F, a->ldc, chunk);
    return false;
  }
  if (!a->qkv || !a->ctx || !a->lse || (bwd && (!a->d_ctx || !a->d_qkv || !a->ws))) {
    set_error("%s: null pointer (qkv, ctx, lse%s)", who, bwd ? ", d_ctx, d_qkv, ws" : "");
    return false;
  }
  const uintptr_t bits = (uintptr_t)a->qkv | (uintptr_t)a->ctx | (bwd ? (uintptr_t)a->d_ctx | (uintptr_t)a->d_qkv : 0);
  if (bits & 15) { set_error("%s: qkv, ctx, d_ctx and d_qkv must be 16-byte aligned", who); return false; }
  if (a->len)
    for (int b = 0; b < a->B; ++b)
      if (a->len[b] < 1 || a->len[b] > a->T) {
        set_error("%s: item %d: len %d outside [1, T = %d]", who, b, a->len[b], a->T);
        return false;
      }
  return true;
}

AttnDev attn_dev(const vqx_attn_args* a) {
  AttnDev d;
  d.qkv = a->qkv; d.ctx = a->ctx; d.lse = a->lse; d.d_ctx = a->d_ctx; d.d_qkv = a->d_qkv; d.delta = a->ws;
  d.T = a->T; d.F = a->F; d.H = a->H; d.b0 = 0; d.ldqkv = a->ldqkv; d.ldc = a->ldc;
  d.scale = 1.f / sqrtf((float)(a->F / a->H));
  return d;
}

template <typename T, int D>
void attn_launch(const vqx_attn_args* a, bool bwd, hipStream_t s) {
  AttnDev d = attn_dev(a);
  const int tiles = (a->T + AT_OWN - 1) / AT_OWN;
  for (int b0 = 0; b0 < a->B; b0 += kAttnItems) {
    const int n = a->B - b0 < kAttnItems ? a->B - b0 : kAttnItems;
    AttnLens L = {};
    for (int i = 0; i < n; ++i) L.len[i] = a->len ? a->len[b0 + i] : a->T;
    d.b0 = b0;
    const dim3 grid(tiles, a->H, n);
    if (!bwd) {
      hipLaunchKernelGGL((attn_fwd_kernel<T, D>), grid, dim3(AT_THREADS), 0, s, d, L);
    } else {
      const dim3 gd((int)(((int64_t)a->T * a->H + AT_THREADS - 1) / AT_THREADS), 1, n);
      hipLaunchKernelGGL((attn_delta_kernel<T, D>), gd, dim3(AT_THREADS), 0, s, d, L);
      hipLaunchKernelGGL((attn_dkv_kernel<T, D>), grid, dim3(AT_THREADS), 0, s, d, L);
      hipLaunchKernelGGL((attn_dq_kernel<T, D>), grid, dim3(AT_THREADS), 0, s, d, L);
    }
  }
}

int attn_run(const char* who, const vqx_attn_args* a, bool bwd, vqx_stream_t stream) {
  if (!attn_args_ok(who, a, bwd)) return -1;
  hipStream_t s = (hipStream_t)stream;
  const int dk = a->F / a->H;
  if (a->dtype == VQX_BF16) {
    if (dk == 32) attn_launch<bf16_t, 32>(a, bwd, s); else attn_launch<bf16_t, 64>(a, bwd, s);
  } else {
    if (dk == 32) attn_launch<float, 32>(a, bwd, s); else attn_launch<float, 64>(a, bwd, s);
  }
  return launch_status(who);
}

}  // namespace
}  // namespace vqx

using namespace vqx;

extern "C" int vqx_attn_workspace(int32_t B, int32_t T, int32_t F, int32_t H, int32_t dtype, int64_t* floats) {
  if (!floats) { set_error("vqx_attn_workspace: null output pointer"); return -1; }
  if (!attn_dims_ok("vqx_attn_workspace", B, T, F, H, dtype)) return -1;
  *floats = (int64_t)B * H * T;  // delta
  return 0;
}

extern "C" int vqx_attn_fwd(const vqx_attn_args* a, vqx_stream_t stream) { return attn_run("vqx_attn_fwd", a, false, stream); }

extern "C" int vqx_attn_bwd(const vqx_attn_args* a, vqx_stream_t stream) { return attn_run("vqx_attn_bwd", a, true, stream); }
