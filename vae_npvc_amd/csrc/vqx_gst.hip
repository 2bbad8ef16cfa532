// Style-token (GST) layer (include/vqx.h vqx_gst_*; reference
// model/layers_gst.py:10-147): time pooling + a 1-query x N-token multi-head
// attention over tanh(gst_embs), forward in 2 launches and backward in 3.
//
// The arithmetic is tiny (B <= 96 rows, ~10 tokens, 128-512 features), so the
// layout follows the data dependences, not the FLOPs:
//   forward   gst_kv_kernel        one workgroup per token:  tok, K, V
//             gst_attn_fwd_kernel  one workgroup per batch row: pool, q,
//                                  softmax, context, output linear
//   backward  gst_bwd_row_kernel   one workgroup per batch row: d_ctx, softmax
//                                  backward, dq, d_ref -> dz
//             gst_bwd_batch_kernel one workgroup per output row: the sums
//                                  over the batch (dWo, dbo, dWq, dbq, dK, dV)
//             gst_bwd_tok_kernel   one workgroup per output row: the sums
//                                  over the tokens (dWk, dWv, dbv, d gst_embs)
// A matrix-vector product whose matrix rows are contiguous along the summed
// index takes one wave per GST_ROWS outputs (lanes along the rows, wave_sum);
// one whose outputs are contiguous takes one thread per output.  Both read
// coalesced.
// Every sum has a fixed order and nothing is accumulated with atomics, so a
// call's results depend on its inputs alone.
#include <math.h>

#include "vqx_common.h"

namespace vqx {
namespace {

constexpr int GST_THREADS = 256;
constexpr int GST_WAVES = GST_THREADS / 64;
constexpr int GST_ROWS = 4;  // matrix rows one wave multiplies at a time (wave_dots)
constexpr int GST_MAX_DIM = 512;  // R and F: the per-row vectors staged in LDS
constexpr int GST_MAX_TOKENS = 32;  // one lane per token in the softmax
constexpr int GST_MAX_DK = 128;

// Workspace: what the forward saves, then the backward's scratch.
struct GstWs {
  float *tok, *K, *V;           // [N][E], [N][F], [N][F]
  float *ref, *q, *a, *ctx;     // [B][R], [B][F], [B][H][N], [B][F]
  float *dctx, *dq, *ds;        // [B][F], [B][F], [B][H][N] (ds / sqrt(d_k))
  float *dK, *dV;               // [N][F], [N][F]
  int64_t floats;
};

GstWs gst_ws(float* p, int64_t B, int64_t N, int64_t F, int64_t H, int64_t R, int64_t E) {
  GstWs w;
  int64_t o = 0;
  auto take = [&](int64_t n) { float* q = p ? p + o : nullptr; o += n; return q; };
  w.tok = take(N * E); w.K = take(N * F); w.V = take(N * F);
  w.ref = take(B * R); w.q = take(B * F); w.a = take(B * H * N); w.ctx = take(B * F);
  w.dctx = take(B * F); w.dq = take(B * F); w.ds = take(B * H * N);
  w.dK = take(N * F); w.dV = take(N * F);
  w.floats = o;
  return w;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// out[u] = m[u*ld + 0..n) . x[0..n) for u < rows (<= GST_ROWS, wave-uniform), the
// calling wave's lanes along the rows; valid in every lane.  The rows' loads
// are independent, so they are in flight together: these kernels are bound by
// the latency of one load after another, not by bandwidth or FLOPs.
__device__ __forceinline__ void wave_dots(const float* __restrict__ m, int64_t ld, const float* x, int n, int rows,
                                          float (&out)[GST_ROWS]) {
  float s[GST_ROWS];
#pragma unroll
  for (int u = 0; u < GST_ROWS; ++u) s[u] = 0.f;
  for (int i = threadIdx.x & 63; i < n; i += 64) {
    const float xv = x[i];
#pragma unroll
    for (int u = 0; u < GST_ROWS; ++u)
      if (u < rows) s[u] = fmaf(xv, m[u * ld + i], s[u]);
  }
#pragma unroll
  for (int u = 0; u < GST_ROWS; ++u) out[u] = wave_sum(s[u]);
}

// s[u] by selects: a dynamic index would put the array into scratch memory
__device__ __forceinline__ float pick(const float (&s)[GST_ROWS], int u) {
  float v = s[0];
#pragma unroll
  for (int k = 1; k < GST_ROWS; ++k) v = u == k ? s[k] : v;
  return v;
}

// tok[n] = tanh(gst_embs[n]); K[n] = tok[n] Wk^T + bk; V[n] = tok[n] Wv^T + bv.  grid N.
__global__ __launch_bounds__(GST_THREADS) void gst_kv_kernel(const float* __restrict__ emb,
                                                             const float* __restrict__ Wk, const float* __restrict__ bk,
                                                             const float* __restrict__ Wv, const float* __restrict__ bv,
                                                             GstWs w, int E, int F) {
  const int n = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float* tok = w.tok + (int64_t)n * E;
  for (int e = tid; e < E; e += GST_THREADS) tok[e] = tanhf(emb[(int64_t)n * E + e]);
  __syncthreads();  // the row just written is read by the whole workgroup
  float s[GST_ROWS];
  for (int isv = 0; isv < 2; ++isv) {
    const float* W = isv ? Wv : Wk;
    const float* bias = isv ? bv : bk;
    float* out = (isv ? w.V : w.K) + (int64_t)n * F;
    for (int f0 = wave * GST_ROWS; f0 < F; f0 += GST_WAVES * GST_ROWS) {
      const int rows = min(GST_ROWS, F - f0);
      wave_dots(W + (int64_t)f0 * E, E, tok, E, rows, s);
      if (lane < rows) out[f0 + lane] = pick(s, lane) + bias[f0 + lane];
    }
  }
}

// One batch row: ref = mean_t z, q, per-head softmax and context, style.  grid B.
__global__ __launch_bounds__(GST_THREADS) void gst_attn_fwd_kernel(const float* __restrict__ z, int64_t ldz, int T,
                                                                   const float* __restrict__ Wq,
                                                                   const float* __restrict__ bq,
                                                                   const float* __restrict__ Wo,
                                                                   const float* __restrict__ bo, GstWs w,
                                                                   float* __restrict__ style, int R, int N, int F,
                                                                   int H) {
  __shared__ float s_ref[GST_MAX_DIM], s_q[GST_MAX_DIM], s_ctx[GST_MAX_DIM];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, dk = F / H;
  const float* zb = z + b * T * ldz;
  for (int r = tid; r < R; r += GST_THREADS) {
    float s = 0.f;
    for (int t = 0; t < T; ++t) s += zb[(int64_t)t * ldz + r];  // frames in order
    s = s / (float)T;
    s_ref[r] = s;
    w.ref[b * R + r] = s;
  }
  __syncthreads();
  float s[GST_ROWS];
  for (int f0 = wave * GST_ROWS; f0 < F; f0 += GST_WAVES * GST_ROWS) {
    const int rows = min(GST_ROWS, F - f0);
    wave_dots(Wq + (int64_t)f0 * R, R, s_ref, R, rows, s);
    if (lane < rows) {
      const float v = pick(s, lane) + bq[f0 + lane];
      s_q[f0 + lane] = v;
      w.q[b * F + f0 + lane] = v;
    }
  }
  __syncthreads();
  const float sqrt_dk = sqrtf((float)dk);
  for (int h = wave; h < H; h += GST_WAVES) {
    const int c0 = h * dk;
    float sc = -INFINITY;  // lane n holds token n's score
    for (int n0 = 0; n0 < N; n0 += GST_ROWS) {
      const int rows = min(GST_ROWS, N - n0);
      wave_dots(w.K + (int64_t)n0 * F + c0, F, s_q + c0, dk, rows, s);
      if (lane >= n0 && lane < n0 + rows) sc = pick(s, lane - n0) / sqrt_dk;
    }
    const float m = wave_max(sc);
    const float e = lane < N ? expf(sc - m) : 0.f;
    const float a = e / wave_sum(e);
    if (lane < N) w.a[(b * H + h) * N + lane] = a;
    for (int d0 = 0; d0 < dk; d0 += 64) {  // uniform trip count: every lane takes part in the shuffles
      const int d = d0 + lane;
      float c = 0.f;
      for (int n = 0; n < N; ++n) {
        const float an = __shfl(a, n, 64);
        if (d < dk) c = fmaf(an, w.V[(int64_t)n * F + c0 + d], c);
      }
      if (d < dk) {
        s_ctx[c0 + d] = c;
        w.ctx[b * F + c0 + d] = c;
      }
    }
  }
  __syncthreads();
  for (int f0 = wave * GST_ROWS; f0 < F; f0 += GST_WAVES * GST_ROWS) {
    const int rows = min(GST_ROWS, F - f0);
    wave_dots(Wo + (int64_t)f0 * F, F, s_ctx, F, rows, s);
    if (lane < rows) style[b * F + f0 + lane] = pick(s, lane) + bo[f0 + lane];
  }
}

// One batch row of the backward: d_ctx = d_style Wo, the softmax backward
// (ds carries the 1/sqrt(d_k) of the scores), dq = ds K, d_ref = dq Wq and
// dz = d_ref / T on each of the row's frames.  grid B.
__global__ __launch_bounds__(GST_THREADS) void gst_bwd_row_kernel(const float* __restrict__ dstyle,
                                                                  const float* __restrict__ Wo,
                                                                  const float* __restrict__ Wq, GstWs w,
                                                                  float* __restrict__ dz, int64_t lddz, int T, int R,
                                                                  int N, int F, int H) {
  __shared__ float s_dy[GST_MAX_DIM], s_dctx[GST_MAX_DIM], s_dq[GST_MAX_DIM];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, dk = F / H;
  for (int f = tid; f < F; f += GST_THREADS) s_dy[f] = dstyle[b * F + f];
  __syncthreads();
  for (int j = tid; j < F; j += GST_THREADS) {
    float s = 0.f;
#pragma unroll 8
    for (int f = 0; f < F; ++f) s = fmaf(s_dy[f], Wo[(int64_t)f * F + j], s);
    s_dctx[j] = s;
    w.dctx[b * F + j] = s;
  }
  __syncthreads();
  const float sqrt_dk = sqrtf((float)dk);
  for (int h = wave; h < H; h += GST_WAVES) {
    const int c0 = h * dk;
    float da = 0.f;  // lane n holds token n's values
    float s[GST_ROWS];
    for (int n0 = 0; n0 < N; n0 += GST_ROWS) {
      const int rows = min(GST_ROWS, N - n0);
      wave_dots(w.V + (int64_t)n0 * F + c0, F, s_dctx + c0, dk, rows, s);
      if (lane >= n0 && lane < n0 + rows) da = pick(s, lane - n0);
    }
    const float a = lane < N ? w.a[(b * H + h) * N + lane] : 0.f;
    const float dot = wave_sum(a * da);
    const float ds = a * (da - dot) / sqrt_dk;
    if (lane < N) w.ds[(b * H + h) * N + lane] = ds;
    for (int d0 = 0; d0 < dk; d0 += 64) {
      const int d = d0 + lane;
      float c = 0.f;
      for (int n = 0; n < N; ++n) {
        const float dsn = __shfl(ds, n, 64);
        if (d < dk) c = fmaf(dsn, w.K[(int64_t)n * F + c0 + d], c);
      }
      if (d < dk) {
        s_dq[c0 + d] = c;
        w.dq[b * F + c0 + d] = c;
      }
    }
  }
  __syncthreads();
  float* dzb = dz + b * T * lddz;
  for (int r = tid; r < R; r += GST_THREADS) {
    float s = 0.f;
#pragma unroll 8
    for (int f = 0; f < F; ++f) s = fmaf(s_dq[f], Wq[(int64_t)f * R + r], s);
    s = s / (float)T;
    for (int t = 0; t < T; ++t) dzb[(int64_t)t * lddz + r] = s;
  }
}

// out[c] = sum_b x[b*ldx + ix] * y[b*ldy + c] for c < cols and, as column
// `cols`, bias_out = sum_b x[b*ldx + ix]: batch rows in order, one thread per column.
__device__ __forceinline__ void gst_batch_row(const float* __restrict__ x, int ldx, int ix,
                                              const float* __restrict__ y, int ldy, int B, int cols,
                                              float* __restrict__ out, float* __restrict__ bias_out) {
  for (int c = threadIdx.x; c <= cols; c += GST_THREADS) {
    float s = 0.f;
    if (c < cols) {
#pragma unroll 8
      for (int64_t b = 0; b < B; ++b) s = fmaf(x[b * ldx + ix], y[b * ldy + c], s);
      out[c] = s;
    } else if (bias_out) {
#pragma unroll 8
      for (int64_t b = 0; b < B; ++b) s += x[b * ldx + ix];
      *bias_out = s;
    }
  }
}

// The sums over the batch.  Workgroup roles by block id:
//   [0, F)        row f of dWo = d_style^T ctx, and dbo[f]
//   [F, 2F)       row f of dWq = dq^T ref, and dbq[f]
//   [2F, 2F+N)    dV[n][c] = sum_b a[b][head(c)][n] d_ctx[b][c]
//   [2F+N, 2F+2N) dK[n][c] = sum_b ds[b][head(c)][n] q[b][c]
__global__ __launch_bounds__(GST_THREADS) void gst_bwd_batch_kernel(const float* __restrict__ dstyle, GstWs w,
                                                                    float* __restrict__ dWo, float* __restrict__ dbo,
                                                                    float* __restrict__ dWq, float* __restrict__ dbq,
                                                                    int B, int R, int N, int F, int H) {
  int blk = blockIdx.x;
  if (blk < F) {
    gst_batch_row(dstyle, F, blk, w.ctx, F, B, F, dWo + (int64_t)blk * F, dbo + blk);
    return;
  }
  blk -= F;
  if (blk < F) {
    gst_batch_row(w.dq, F, blk, w.ref, R, B, R, dWq + (int64_t)blk * R, dbq + blk);
    return;
  }
  blk -= F;
  const bool isk = blk >= N;
  const int n = isk ? blk - N : blk, dk = F / H, HN = H * N;
  const float* coef = isk ? w.ds : w.a;    // [B][H][N]
  const float* vec = isk ? w.q : w.dctx;   // [B][F]
  float* out = (isk ? w.dK : w.dV) + (int64_t)n * F;
  for (int c = threadIdx.x; c < F; c += GST_THREADS) {
    const int hn = (c / dk) * N + n;
    float s = 0.f;
#pragma unroll 8
    for (int64_t b = 0; b < B; ++b) s = fmaf(coef[b * HN + hn], vec[b * F + c], s);
    out[c] = s;
  }
}

// The sums over the tokens.  Workgroup roles by block id:
//   [0, F)     row f of dWk = dK^T tok, and dbk[f] = 0 (see vqx.h)
//   [F, 2F)    row f of dWv = dV^T tok, and dbv[f]
//   [2F, 2F+N) d gst_embs[n] = (dK[n] Wk + dV[n] Wv) * (1 - tok[n]^2)
__global__ __launch_bounds__(GST_THREADS) void gst_bwd_tok_kernel(const float* __restrict__ Wk,
                                                                  const float* __restrict__ Wv, GstWs w,
                                                                  float* __restrict__ dWk, float* __restrict__ dbk,
                                                                  float* __restrict__ dWv, float* __restrict__ dbv,
                                                                  float* __restrict__ demb, int N, int E, int F) {
  int blk = blockIdx.x;
  if (blk < F) {
    gst_batch_row(w.dK, F, blk, w.tok, E, N, E, dWk + (int64_t)blk * E, nullptr);
    if (threadIdx.x == 0) dbk[blk] = 0.f;
    return;
  }
  blk -= F;
  if (blk < F) {
    gst_batch_row(w.dV, F, blk, w.tok, E, N, E, dWv + (int64_t)blk * E, dbv + blk);
    return;
  }
  const int n = blk - F;
  const float* dKn = w.dK + (int64_t)n * F;
  const float* dVn = w.dV + (int64_t)n * F;
  for (int e = threadIdx.x; e < E; e += GST_THREADS) {
    float sk = 0.f, sv = 0.f;
#pragma unroll 8
    for (int f = 0; f < F; ++f) {
      sk = fmaf(dKn[f], Wk[(int64_t)f * E + e], sk);
      sv = fmaf(dVn[f], Wv[(int64_t)f * E + e], sv);
    }
    const float t = w.tok[(int64_t)n * E + e];
    demb[(int64_t)n * E + e] = (sk + sv) * (1.f - t * t);
  }
}

// The envelope of vqx.h, checked before any launch.
bool gst_dims_ok(const char* who, int64_t B, int T, int R, int N, int E, int F, int H) {
  if (B < 1 || B > INT32_MAX || T < 1) { set_error("%s: B = %lld and T = %d must be >= 1", who, (long long)B, T); return false; }
  if (R < 4 || R % 4 || R > GST_MAX_DIM) { set_error("%s: R = %d must be a multiple of 4 in [4, %d]", who, R, GST_MAX_DIM); return false; }
  if (N < 1 || N > GST_MAX_TOKENS) { set_error("%s: N = %d tokens not in [1, %d]", who, N, GST_MAX_TOKENS); return false; }
  if (F < 1 || F > GST_MAX_DIM || H < 1 || F % H) { set_error("%s: F = %d must be a multiple of H = %d and <= %d", who, F, H, GST_MAX_DIM); return false; }
  if (F / H > GST_MAX_DK) { set_error("%s: d_k = F / H = %d exceeds %d", who, F / H, GST_MAX_DK); return false; }
  if (E < 1) { set_error("%s: E = %d must be >= 1", who, E); return false; }
  return true;
}

}  // namespace
}  // namespace vqx

using namespace vqx;

extern "C" int vqx_gst_workspace(int32_t B, int32_t N, int32_t F, int32_t H, int32_t R, int32_t E, int64_t* floats) {
  if (!floats) { set_error("vqx_gst_workspace: null output pointer"); return -1; }
  if (!gst_dims_ok("vqx_gst_workspace", B, 1, R, N, E, F, H)) return -1;
  *floats = gst_ws(nullptr, B, N, F, H, R, E).floats;
  return 0;
}

extern "C" int vqx_gst_fwd(const vqx_gst_args* a, vqx_stream_t stream) {
  if (!a) { set_error("vqx_gst_fwd: null args"); return -1; }
  if (!gst_dims_ok("vqx_gst_fwd", a->B, a->T, a->R, a->N, a->E, a->F, a->H)) return -1;
  if (a->ldz < a->R) { set_error("vqx_gst_fwd: ldz = %d is below R = %d", a->ldz, a->R); return -1; }
  if (!a->z || !a->gst_embs || !a->wq || !a->bq || !a->wk || !a->bk || !a->wv || !a->bv || !a->wo || !a->bo ||
      !a->style || !a->ws) {
    set_error("vqx_gst_fwd: null pointer (z, gst_embs, the eight weights and biases, style, ws)");
    return -1;
  }
  const GstWs w = gst_ws(a->ws, a->B, a->N, a->F, a->H, a->R, a->E);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(gst_kv_kernel, dim3(a->N), dim3(GST_THREADS), 0, s, a->gst_embs, a->wk, a->bk, a->wv, a->bv, w,
                     a->E, a->F);
  hipLaunchKernelGGL(gst_attn_fwd_kernel, dim3(a->B), dim3(GST_THREADS), 0, s, a->z, (int64_t)a->ldz, a->T, a->wq,
                     a->bq, a->wo, a->bo, w, a->style, a->R, a->N, a->F, a->H);
  return launch_status("vqx_gst_fwd");
}

extern "C" int vqx_gst_bwd(const vqx_gst_args* a, vqx_stream_t stream) {
  if (!a) { set_error("vqx_gst_bwd: null args"); return -1; }
  if (!gst_dims_ok("vqx_gst_bwd", a->B, a->T, a->R, a->N, a->E, a->F, a->H)) return -1;
  if (a->lddz < a->R) { set_error("vqx_gst_bwd: lddz = %d is below R = %d", a->lddz, a->R); return -1; }
  if (!a->d_style || !a->ws || !a->wq || !a->wk || !a->wv || !a->wo || !a->dz || !a->d_gst_embs || !a->dwq ||
      !a->dbq || !a->dwk || !a->dbk || !a->dwv || !a->dbv || !a->dwo || !a->dbo) {
    set_error("vqx_gst_bwd: null pointer (d_style, ws, the four weights, dz, the nine parameter gradients)");
    return -1;
  }
  const GstWs w = gst_ws(a->ws, a->B, a->N, a->F, a->H, a->R, a->E);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(gst_bwd_row_kernel, dim3(a->B), dim3(GST_THREADS), 0, s, a->d_style, a->wo, a->wq, w, a->dz,
                     (int64_t)a->lddz, a->T, a->R, a->N, a->F, a->H);
  hipLaunchKernelGGL(gst_bwd_batch_kernel, dim3(2 * a->F + 2 * a->N), dim3(GST_THREADS), 0, s, a->d_style, w, a->dwo,
                     a->dbo, a->dwq, a->dbq, a->B, a->R, a->N, a->F, a->H);
  hipLaunchKernelGGL(gst_bwd_tok_kernel, dim3(2 * a->F + a->N), dim3(GST_THREADS), 0, s, a->wk, a->wv, w, a->dwk,
                     a->dbk, a->dwv, a->dbv, a->d_gst_embs, a->N, a->E, a->F);
  return launch_status("vqx_gst_bwd");
}
