// Embedding, the three families of conditioning linears (plain, batched
// 64x64-tiled, MFMA fast path) and the fused step prologue (gfx950).
#include "vqx_common.h"
#include "vqx_wn_pack.h"

namespace vqx {

__global__ void embedding_fwd_kernel(const float* __restrict__ w, const int64_t* __restrict__ ids, int B, int D,
                                     float* __restrict__ out) {
  const int b = blockIdx.x;
  for (int d = threadIdx.x; d < D; d += blockDim.x) out[(int64_t)b * D + d] = w[ids[b] * D + d];
}

// dense embedding gradient, deterministic: one thread per (row used, d), summing the batch in order
__global__ void embedding_bwd_kernel(const float* __restrict__ dout, const int64_t* __restrict__ ids, int B, int D,
                                     float* __restrict__ dw) {
  const int b = blockIdx.x;
  // only the first occurrence of each id accumulates all occurrences (in batch order)
  for (int p = 0; p < b; ++p)
    if (ids[p] == ids[b]) return;
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    float s = 0.f;
    for (int q = b; q < B; ++q)
      if (ids[q] == ids[b]) s += dout[(int64_t)q * D + d];
    dw[ids[b] * D + d] += s;
  }
}

// vqx_embedding_bwd_rows: block r = embedding row r; the batch's ids staged in
// LDS, every thread scans them in batch order and adds the matching rows of
// dout (one or two per id in a batch: a short load chain, not B serial loads)
constexpr int kEmbMaxB = 1024;
__global__ __launch_bounds__(256) void embedding_bwd_rows_kernel(const float* __restrict__ dout,
                                                                 const int64_t* __restrict__ ids, int B, int D,
                                                                 float* __restrict__ dw, int accumulate) {
  __shared__ int sid[kEmbMaxB];
  const int r = blockIdx.x;
  // batches above kEmbMaxB ids run in LDS-sized chunks (each chunk's sum added
  // to the row in chunk order; one chunk for B <= kEmbMaxB, as before)
  for (int q0 = 0; q0 < B; q0 += kEmbMaxB) {
    const int nq = min(kEmbMaxB, B - q0);
    __syncthreads();
    for (int q = threadIdx.x; q < nq; q += blockDim.x) sid[q] = (int)ids[q0 + q];
    __syncthreads();
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
      float s = 0.f;
      for (int q = 0; q < nq; ++q)
        if (sid[q] == r) s += dout[(int64_t)(q0 + q) * D + d];
      float* o = dw + (int64_t)r * D + d;
      *o = (accumulate || q0 > 0) ? *o + s : s;
    }
  }
}

__global__ void linear_fwd_kernel(const float* __restrict__ c, const float* __restrict__ W, const float* __restrict__ bias,
                                  int B, int I, int O, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)B * O) return;
  const int b = (int)(e / O), o = (int)(e - (int64_t)b * O);
  float s = 0.f;
#pragma unroll 8
  for (int i = 0; i < I; ++i) s = fmaf(W[(int64_t)o * I + i], c[(int64_t)b * I + i], s);
  out[e] = s + (bias ? bias[o] : 0.f);
}

__global__ void linear_bwd_w_kernel(const float* __restrict__ dout, const float* __restrict__ c, int B, int I, int O,
                                    float* __restrict__ dW) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)O * I) return;
  const int o = (int)(e / I), i = (int)(e - (int64_t)o * I);
  float s = 0.f;
#pragma unroll 8
  for (int b = 0; b < B; ++b) s = fmaf(dout[(int64_t)b * O + o], c[(int64_t)b * I + i], s);
  dW[e] += s;
}

// dc[b][i] += sum_o dout[b][o] * W[o][i]: block (b, 64 columns i), 4 groups of o
__global__ __launch_bounds__(256) void linear_bwd_x_kernel(const float* __restrict__ dout, const float* __restrict__ W,
                                                           int B, int I, int O, float* __restrict__ dc) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  const int og = threadIdx.x >> 6;
  __shared__ float acc[4][64];
  float s = 0.f;
  if (i < I) {
    float s2 = 0.f;
    int o = og;
#pragma unroll 4
    for (; o + 4 < O; o += 8) {
      s = fmaf(dout[(int64_t)b * O + o], W[(int64_t)o * I + i], s);
      s2 = fmaf(dout[(int64_t)b * O + o + 4], W[(int64_t)(o + 4) * I + i], s2);
    }
    for (; o < O; o += 4) s = fmaf(dout[(int64_t)b * O + o], W[(int64_t)o * I + i], s);
    s += s2;
  }
  acc[og][threadIdx.x & 63] = s;
  __syncthreads();
  if (og == 0 && i < I) {
    const int l = threadIdx.x & 63;
    dc[(int64_t)b * I + i] += (acc[0][l] + acc[1][l]) + (acc[2][l] + acc[3][l]);
  }
}

// Batched speaker-conditioning linears (all ResSkip blocks per launch) as
// small LDS-tiled fp32 GEMMs: 64x64 output tiles, 256 threads x 16 outputs,
// K in chunks of 64.  Grid z carries (layer, tile of the third dimension).
constexpr int kLT = 64;

// out_l[b][o] = sum_i c[b][i] W_l[o][i] + bias_l[o].  grid (ceil(O/64), n, ceil(B/64))
__global__ __launch_bounds__(256) void linear_batched_fwd_kernel(const vqx_linear_layer* __restrict__ L,
                                                                 const float* __restrict__ c, int B, int I, int O) {
  const vqx_linear_layer& l = L[blockIdx.y];
  const int o0 = blockIdx.x * kLT, b0 = blockIdx.z * kLT;
  __shared__ float cs[kLT][kLT + 1];   // [b][i]
  __shared__ __attribute__((aligned(16))) float wt[kLT][kLT + 4];  // [i][o]
  const int t = threadIdx.x, tb = t >> 2, to = (t & 3) * 16;
  float acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = 0.f;
  for (int i0 = 0; i0 < I; i0 += kLT) {
    for (int e = t; e < kLT * kLT; e += 256) {
      const int r = e >> 6, q = e & 63;  // r: b or o row, q: i column (coalesced)
      cs[r][q] = (b0 + r < B && i0 + q < I) ? c[(int64_t)(b0 + r) * I + i0 + q] : 0.f;
      wt[q][r] = (o0 + r < O && i0 + q < I) ? l.W[(int64_t)(o0 + r) * I + i0 + q] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int i = 0; i < kLT; ++i) {
      const float x = cs[tb][i];
#pragma unroll
      for (int j = 0; j < 16; j += 4) {
        const f32x4_t w = *(const f32x4_t*)&wt[i][to + j];
        acc[j] = fmaf(x, w[0], acc[j]);
        acc[j + 1] = fmaf(x, w[1], acc[j + 1]);
        acc[j + 2] = fmaf(x, w[2], acc[j + 2]);
        acc[j + 3] = fmaf(x, w[3], acc[j + 3]);
      }
    }
    __syncthreads();
  }
  const int b = b0 + tb;
  if (b >= B) return;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int o = o0 + to + j;
    if (o < O) l.out[(int64_t)b * O + o] = acc[j] + (l.bias ? l.bias[o] : 0.f);
  }
}

// dW_l[o][i] = sum_b dout_l[b][o] c[b][i]; dbias_l[o] = sum_b dout_l[b][o].
// grid (ceil(O/64), n, ceil(I/64)); the i-tile-0 blocks also write dbias.
__global__ __launch_bounds__(256) void linear_batched_bwd_w_kernel(const vqx_linear_layer* __restrict__ L,
                                                                   const float* __restrict__ c, int B, int I, int O) {
  const vqx_linear_layer& l = L[blockIdx.y];
  const int o0 = blockIdx.x * kLT, i0 = blockIdx.z * kLT;
  __shared__ float ds[kLT][kLT + 1];   // [b][o]
  __shared__ __attribute__((aligned(16))) float cs[kLT][kLT + 4];  // [b][i]
  const int t = threadIdx.x, to = t >> 2, ti = (t & 3) * 16;
  float acc[16], db = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = 0.f;
  for (int b0 = 0; b0 < B; b0 += kLT) {
    for (int e = t; e < kLT * kLT; e += 256) {
      const int r = e >> 6, q = e & 63;
      ds[r][q] = (b0 + r < B && o0 + q < O) ? l.dout[(int64_t)(b0 + r) * O + o0 + q] : 0.f;
      cs[r][q] = (b0 + r < B && i0 + q < I) ? c[(int64_t)(b0 + r) * I + i0 + q] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int b = 0; b < kLT; ++b) {
      const float d = ds[b][to];
      db += d;
#pragma unroll
      for (int j = 0; j < 16; j += 4) {
        const f32x4_t x = *(const f32x4_t*)&cs[b][ti + j];
        acc[j] = fmaf(d, x[0], acc[j]);
        acc[j + 1] = fmaf(d, x[1], acc[j + 1]);
        acc[j + 2] = fmaf(d, x[2], acc[j + 2]);
        acc[j + 3] = fmaf(d, x[3], acc[j + 3]);
      }
    }
    __syncthreads();
  }
  const int o = o0 + to;
  if (o >= O) return;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int i = i0 + ti + j;
    if (i < I) l.dW[(int64_t)o * I + i] = acc[j];
  }
  if (blockIdx.z == 0 && (t & 3) == 0 && l.dbias) l.dbias[o] = db;
}

// Split-K partial of dc[b][i] = sum_l sum_o dout_l[b][o] W_l[o][i] over one
// 64-wide o chunk of one layer.  grid (ceil(O/64), n, ceil(B/64)*ceil(I/64));
// part[(l*nO + oc)][b][i].
__global__ __launch_bounds__(256) void linear_batched_bwd_x_kernel(const vqx_linear_layer* __restrict__ L, int B,
                                                                   int I, int O, float* __restrict__ part) {
  const vqx_linear_layer& l = L[blockIdx.y];
  const float* __restrict__ dout = l.dout;
  const float* __restrict__ W = l.W;
  const int nI = (I + kLT - 1) / kLT;
  const int o0 = blockIdx.x * kLT, b0 = (blockIdx.z / nI) * kLT, i0 = (blockIdx.z % nI) * kLT;
  __shared__ float ds[kLT][kLT + 1];   // [b][o]
  __shared__ __attribute__((aligned(16))) float ws[kLT][kLT + 4];  // [o][i]
  const int t = threadIdx.x, tb = t >> 2, ti = (t & 3) * 16;
  // every operand load of the thread issued before the first is used (indices
  // clamped in range, the out-of-range elements zeroed at the LDS write): a
  // predicated load per element serialised them, one memory latency each
  constexpr int NE = kLT * kLT / 256;
  float dv[NE], wv[NE];
#pragma unroll
  for (int u = 0; u < NE; ++u) {
    const int e = t + 256 * u, r = e >> 6, q = e & 63;
    const int br = min(b0 + r, B - 1), oq = min(o0 + q, O - 1), orr = min(o0 + r, O - 1), iq = min(i0 + q, I - 1);
    dv[u] = dout[(int64_t)br * O + oq];
    wv[u] = W[(int64_t)orr * I + iq];
  }
#pragma unroll
  for (int u = 0; u < NE; ++u) {
    const int e = t + 256 * u, r = e >> 6, q = e & 63;
    ds[r][q] = (b0 + r < B && o0 + q < O) ? dv[u] : 0.f;
    ws[r][q] = (o0 + r < O && i0 + q < I) ? wv[u] : 0.f;
  }
  __syncthreads();
  float acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = 0.f;
#pragma unroll 8
  for (int o = 0; o < kLT; ++o) {
    const float d = ds[tb][o];
#pragma unroll
    for (int j = 0; j < 16; j += 4) {
      const f32x4_t w = *(const f32x4_t*)&ws[o][ti + j];
      acc[j] = fmaf(d, w[0], acc[j]);
      acc[j + 1] = fmaf(d, w[1], acc[j + 1]);
      acc[j + 2] = fmaf(d, w[2], acc[j + 2]);
      acc[j + 3] = fmaf(d, w[3], acc[j + 3]);
    }
  }
  const int b = b0 + tb;
  if (b >= B) return;
  float* out = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * B * I;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int i = i0 + ti + j;
    if (i < I) out[(int64_t)b * I + i] = acc[j];
  }
}

// ---- speaker-conditioning fast path: I = 128 inputs, O % 64 == 0 (every
// recipe: cond dim 128); any B for the forward and the data gradient (their
// per-row results do not depend on B: data-parallel ranks and one process on
// the global batch agree row by row), B <= 64 for the weight gradient.  fp32 MFMA (v_mfma_f32_16x16x4f32, the
// reference's fp32): a workgroup is 4 waves x 16 output channels of one
// layer; the operands go straight from memory into the MFMA lane layout.  The
// K index is permuted so each lane's operands are contiguous: in step s, lane
// group q takes k = 32q + s (forward, K = I = 128) or b = 16q + s (weight
// gradient, K = B <= 64).  (Round 5: the LDS-blocked VALU kernels these
// replace took 11-12 us a launch, bound by three LDS reads per eight FMAs;
// the tiled kernels above, for other shapes, sum in a different order.)
constexpr int kCondI = 128, kCondB = 64, kCondO = 64;

// out_l[b][o] = bias_l[o] + sum_i c[b][i] W_l[o][i]; grid (O/64, n)
// ids != null: row b of c is row ids[b] of c (the embedding table: the lookup
// folded into the operand loads, vqx_linear_batched_fwd_ids)
__device__ __forceinline__ void linear_cond_fwd_block(const vqx_linear_layer* __restrict__ L,
                                                      const float* __restrict__ c, const int64_t* __restrict__ ids,
                                                      int B, int O, int bx, int layer) {
  const vqx_linear_layer& l = L[layer];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int q = lane >> 4, j = lane & 15;
  const int o0 = bx * kCondO + w * 16;
  // B operand (k = 32q + s, n = j): W[o0 + j][32q .. 32q + 31]
  f32x4_t wb[8];
  const float* wr = l.W + (int64_t)(o0 + j) * kCondI + 32 * q;
#pragma unroll
  for (int u = 0; u < 8; ++u) wb[u] = *(const f32x4_t*)(wr + 4 * u);
  const float bj = l.bias ? l.bias[o0 + j] : 0.f;
  for (int rt = 0; rt * 16 < B; ++rt) {
    // A operand (m = j, k = 32q + s): c[row][32q .. 32q + 31]; rows >= B read row B-1, not stored
    const int row = min(rt * 16 + j, B - 1);
    const float* cr = c + (ids ? ids[row] : (int64_t)row) * kCondI + 32 * q;
    f32x4_t ca[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) ca[u] = *(const f32x4_t*)(cr + 4 * u);
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f}, acc2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ca[u][0], wb[u][0], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(ca[u][1], wb[u][1], acc2, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ca[u][2], wb[u][2], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(ca[u][3], wb[u][3], acc2, 0, 0, 0);
    }
    // D[m = 4q + r][n = j]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = rt * 16 + 4 * q + r;
      if (b < B) l.out[(int64_t)b * O + o0 + j] = (acc[r] + acc2[r]) + bj;
    }
  }
}
__global__ __launch_bounds__(256) void linear_cond_fwd_kernel(const vqx_linear_layer* __restrict__ L,
                                                              const float* __restrict__ c,
                                                              const int64_t* __restrict__ ids, int B, int O) {
  linear_cond_fwd_block(L, c, ids, B, O, blockIdx.x, blockIdx.y);
}

// The training step's prologue in one launch (vqx_step_prologue): the
// conditioning linears (n_cond x O/64 blocks, latency-bound MFMA chains:
// first, so they start first), the input transpose (32 x 32 tiles), then the
// weight-norm pack units -- three independent jobs that ran as three
// launches in turn (11 + 5 + 22 us).  Each block runs the body of the
// launch it replaces, so the results are those launches' bits.
template <typename T>
__global__ __launch_bounds__(256) void step_prologue_kernel(const vqx_wn_layer* __restrict__ WL, WnUnits U,
                                                            const vqx_linear_layer* __restrict__ CL, int n_cond_blocks,
                                                            int cond_bx, const float* __restrict__ emb,
                                                            const int64_t* __restrict__ ids, int B, int O,
                                                            const float* __restrict__ x, int C, int T_, int tx_bx,
                                                            int tx_by, int n_tx_blocks, T* __restrict__ y, int ldy) {
  __shared__ __attribute__((aligned(16))) float buf[kWnBuf];
  __shared__ float red[16];
  int bid = (int)blockIdx.x;
  if (bid < n_cond_blocks) {
    linear_cond_fwd_block(CL, emb, ids, B, O, bid % cond_bx, bid / cond_bx);
    return;
  }
  bid -= n_cond_blocks;
  if (bid < n_tx_blocks) {
    const int r = bid / tx_bx;
    nct_to_ntc_tile<T>(x, C, T_, y, ldy, bid - r * tx_bx, r % tx_by, r / tx_by, (float(*)[33])buf);
    return;
  }
  wn_pack_block(WL, U, bid - n_tx_blocks, buf, red);
}

// dW_l[o][i] = sum_b dout_l[b][o] c[b][i], dbias_l[o] = sum_b dout_l[b][o]; grid (O/64, n)
// one workgroup (bx = output chunk, layer); cs: kCondB x kCondI floats of LDS (c, rows >= B zero)
__device__ __forceinline__ void linear_cond_bwd_w_block(const vqx_linear_layer* __restrict__ L,
                                                        const float* __restrict__ c, const int64_t* __restrict__ ids,
                                                        int B, int O, int bx, int layer, float (*cs)[kCondI]) {
  const vqx_linear_layer& l = L[layer];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int q = lane >> 4, j = lane & 15;
  const int o0 = bx * kCondO + w * 16;
  // A operand (m = j, k = b = 16q + s): dout[16q + s][o0 + j], zero past B
  float da[16];
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const int b = 16 * q + s;
    da[s] = l.dout[(int64_t)min(b, B - 1) * O + o0 + j];
  }
  constexpr int NC = kCondB * kCondI / 4 / 256;
  f32x4_t cv[NC];
#pragma unroll
  for (int u = 0; u < NC; ++u) {
    const int e = threadIdx.x + 256 * u, r = e / (kCondI / 4), i4 = e % (kCondI / 4);
    const int row = min(r, B - 1);
    cv[u] = *(const f32x4_t*)(c + (ids ? ids[row] : (int64_t)row) * kCondI + 4 * i4);
  }
#pragma unroll
  for (int u = 0; u < NC; ++u) {
    const int e = threadIdx.x + 256 * u, r = e / (kCondI / 4), i4 = e % (kCondI / 4);
    const f32x4_t z = {0.f, 0.f, 0.f, 0.f};
    *(f32x4_t*)&cs[r][4 * i4] = r < B ? cv[u] : z;
  }
  // dbias: the lane's 16 rows in order, then the four lane groups (q) in order
  float db = 0.f;
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    if (16 * q + s >= B) da[s] = 0.f;
    db += da[s];
  }
  {
    const float d1 = __shfl(db, j + 16, 64), d2 = __shfl(db, j + 32, 64), d3 = __shfl(db, j + 48, 64);
    if (q == 0 && l.dbias) l.dbias[o0 + j] = ((db + d1) + d2) + d3;
  }
  __syncthreads();
  for (int it = 0; it < kCondI / 16; ++it) {
    // B operand (k = b = 16q + s, n = j): c[16q + s][16 it + j]
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f}, acc2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 16; s += 2) {
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(da[s], cs[16 * q + s][16 * it + j], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(da[s + 1], cs[16 * q + s + 1][16 * it + j], acc2, 0, 0, 0);
    }
    // D[m = 4q + r][n = j]: dW[o0 + 4q + r][16 it + j]
#pragma unroll
    for (int r = 0; r < 4; ++r) l.dW[(int64_t)(o0 + 4 * q + r) * kCondI + 16 * it + j] = acc[r] + acc2[r];
  }
}
__global__ __launch_bounds__(256) void linear_cond_bwd_w_kernel(const vqx_linear_layer* __restrict__ L,
                                                                const float* __restrict__ c,
                                                                const int64_t* __restrict__ ids, int B, int O) {
  __shared__ float cs[kCondB][kCondI];
  linear_cond_bwd_w_block(L, c, ids, B, O, blockIdx.x, blockIdx.y, cs);
}

// dc partials: part[l * (O/64) + oc][b][i] = sum over the chunk's 64 outputs o
// of dout_l[b][o] W_l[o][i] (k = o = o0 + 16q + s); sum_slices_wide_kernel adds
// the slices in order.  Wave w covers inputs 32w .. 32w + 31.  grid (O/64, n)
__device__ __forceinline__ void linear_cond_bwd_x_block(const vqx_linear_layer* __restrict__ L, int B, int O,
                                                        float* __restrict__ part, int bx, int layer) {
  const vqx_linear_layer& l = L[layer];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int q = lane >> 4, j = lane & 15;
  const int o0 = bx * kCondO;
  const int64_t slice = (int64_t)layer * (O / kCondO) + bx;
  // B operand (k = 16q + s, n = j) of the wave's two 16-input tiles
  float wv[2][16];
#pragma unroll
  for (int it = 0; it < 2; ++it)
#pragma unroll
    for (int s = 0; s < 16; ++s) wv[it][s] = l.W[(int64_t)(o0 + 16 * q + s) * kCondI + 32 * w + 16 * it + j];
  for (int rt = 0; rt * 16 < B; ++rt) {
    // A operand (m = j, k = 16q + s): dout[row][o0 + 16q + s]; rows >= B read row B-1, not stored
    const float* dr = l.dout + (int64_t)min(rt * 16 + j, B - 1) * O + o0 + 16 * q;
    float da[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) da[s] = dr[s];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      f32x4_t acc = {0.f, 0.f, 0.f, 0.f}, acc2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 16; s += 2) {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(da[s], wv[it][s], acc, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(da[s + 1], wv[it][s + 1], acc2, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int b = rt * 16 + 4 * q + r;
        if (b < B) part[(slice * B + b) * kCondI + 32 * w + 16 * it + j] = acc[r] + acc2[r];
      }
    }
  }
}
__global__ __launch_bounds__(256) void linear_cond_bwd_x_kernel(const vqx_linear_layer* __restrict__ L, int B, int O,
                                                                float* __restrict__ part) {
  linear_cond_bwd_x_block(L, B, O, part, blockIdx.x, blockIdx.y);
}
// both in one grid (O/64, 2n): layers' dW / dbias in y < n, their dc slices in y >= n
__global__ __launch_bounds__(256) void linear_cond_bwd_kernel(const vqx_linear_layer* __restrict__ L,
                                                              const float* __restrict__ c,
                                                              const int64_t* __restrict__ ids, int B, int O, int n,
                                                              float* __restrict__ part) {
  __shared__ float cs[kCondB][kCondI];
  if ((int)blockIdx.y < n) linear_cond_bwd_w_block(L, c, ids, B, O, blockIdx.x, blockIdx.y, cs);
  else linear_cond_bwd_x_block(L, B, O, part, blockIdx.x, blockIdx.y - n);
}

// dc[e] = sum_p part[p][e] in a fixed order: each of the 4 waves of a
// workgroup sums a contiguous quarter of the slices (8 loads in flight) for
// 64 elements, then the quarters are added in order (deterministic).
__global__ __launch_bounds__(256) void sum_slices_wide_kernel(const float* __restrict__ part, int np, int64_t n,
                                                              float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
  const int q = threadIdx.x >> 6;
  const int p0 = (int)((int64_t)np * q / 4), p1 = (int)((int64_t)np * (q + 1) / 4);
  __shared__ float red[4][64];
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (e < n) {
    int p = p0;
    for (; p + 8 <= p1; p += 8) {
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = part[(int64_t)(p + u) * n + e];
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] += t[u];
    }
    for (int u = 0; p < p1; ++p, ++u) a[u] += part[(int64_t)p * n + e];
  }
  red[q][threadIdx.x & 63] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  __syncthreads();
  if (q == 0 && e < n) out[e] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

}  // namespace vqx

using namespace vqx;

extern "C" int vqx_embedding_fwd(const float* weight, const int64_t* ids, int32_t B, int32_t D, float* out,
                                 vqx_stream_t stream) {
  hipLaunchKernelGGL(embedding_fwd_kernel, dim3(B), dim3(128), 0, (hipStream_t)stream, weight, ids, B, D, out);
  return launch_status("vqx_embedding_fwd");
}

extern "C" int vqx_embedding_bwd(const float* dout, const int64_t* ids, int32_t B, int32_t D, float* dweight,
                                 vqx_stream_t stream) {
  hipLaunchKernelGGL(embedding_bwd_kernel, dim3(B), dim3(128), 0, (hipStream_t)stream, dout, ids, B, D, dweight);
  return launch_status("vqx_embedding_bwd");
}

extern "C" int vqx_embedding_bwd_rows(const float* dout, const int64_t* ids, int32_t B, int32_t D, int32_t n_rows,
                                      float* dweight, int32_t accumulate, vqx_stream_t stream) {
  if (!dout || !ids || !dweight || B < 1 || D < 1 || n_rows < 1) {
    set_error("vqx_embedding_bwd_rows: bad arguments");
    return -1;
  }
  hipLaunchKernelGGL(embedding_bwd_rows_kernel, dim3(n_rows), dim3(D >= 256 ? 256 : ((D + 63) / 64) * 64), 0,
                     (hipStream_t)stream, dout, ids, B, D, dweight, accumulate);
  return launch_status("vqx_embedding_bwd_rows");
}

extern "C" int vqx_linear_batched_fwd(const vqx_linear_layer* table_dev, int32_t n, const float* c, int32_t B,
                                      int32_t I, int32_t O, vqx_stream_t stream) {
  if (!table_dev || n < 1 || !c || B < 1 || I < 1 || O < 1) { set_error("vqx_linear_batched_fwd: bad arguments"); return -1; }
  if (I == kCondI && O % kCondO == 0 && ((uintptr_t)c & 15) == 0)  // any B: 16-row tiles in turn
    hipLaunchKernelGGL(linear_cond_fwd_kernel, dim3(O / kCondO, n), dim3(256), 0, (hipStream_t)stream, table_dev, c,
                       (const int64_t*)nullptr, B, O);
  else
    hipLaunchKernelGGL(linear_batched_fwd_kernel, dim3((O + kLT - 1) / kLT, n, (B + kLT - 1) / kLT), dim3(256), 0,
                       (hipStream_t)stream, table_dev, c, B, I, O);
  return launch_status("vqx_linear_batched_fwd");
}

extern "C" int vqx_linear_batched_bwd(const vqx_linear_layer* table_dev, int32_t n, const float* c, int32_t B,
                                      int32_t I, int32_t O, float* dc, float* partials, vqx_stream_t stream) {
  if (!table_dev || n < 1 || !c || B < 1 || I < 1 || O < 1) { set_error("vqx_linear_batched_bwd: bad arguments"); return -1; }
  if (dc && !partials) { set_error("vqx_linear_batched_bwd: dc needs partials [n*ceil(O/64)][B][I]"); return -1; }
  hipStream_t s = (hipStream_t)stream;
  const int nO = (O + kLT - 1) / kLT;
  if (I == kCondI && B <= kCondB && O % kCondO == 0 && ((uintptr_t)c & 15) == 0)
    hipLaunchKernelGGL(linear_cond_bwd_w_kernel, dim3(O / kCondO, n), dim3(256), 0, s, table_dev, c,
                       (const int64_t*)nullptr, B, O);
  else
    hipLaunchKernelGGL(linear_batched_bwd_w_kernel, dim3(nO, n, (I + kLT - 1) / kLT), dim3(256), 0, s,
                       table_dev, c, B, I, O);
  if (dc) {
    // any B (16-row tiles in turn), nO slices per layer as the tiled kernel: a row's dc does not depend on B
    if (I == kCondI && O % kCondO == 0 && kCondO == kLT)
      hipLaunchKernelGGL(linear_cond_bwd_x_kernel, dim3(O / kCondO, n), dim3(256), 0, s, table_dev, B, O, partials);
    else
      hipLaunchKernelGGL(linear_batched_bwd_x_kernel, dim3(nO, n, ((B + kLT - 1) / kLT) * ((I + kLT - 1) / kLT)),
                         dim3(256), 0, s, table_dev, B, I, O, partials);
    const int64_t ne = (int64_t)B * I;
    hipLaunchKernelGGL(sum_slices_wide_kernel, dim3((unsigned)((ne + 63) / 64)), dim3(256), 0, s, partials, n * nO, ne,
                       dc);
  }
  return launch_status("vqx_linear_batched_bwd");
}

static bool linear_ids_ok(const vqx_linear_layer* t, int n, const float* emb, const int64_t* ids, int B, int I, int O,
                          const char* who) {
  if (!t || n < 1 || !emb || !ids || B < 1 || B > kCondB || I != kCondI || O % kCondO || ((uintptr_t)emb & 15)) {
    set_error("%s: needs I = %d, 1 <= B <= %d, O %% %d == 0 and a 16-B aligned table", who, kCondI, kCondB, kCondO);
    return false;
  }
  return true;
}

extern "C" int vqx_linear_batched_fwd_ids(const vqx_linear_layer* table_dev, int32_t n, const float* emb,
                                          const int64_t* ids, int32_t B, int32_t I, int32_t O, vqx_stream_t stream) {
  if (!linear_ids_ok(table_dev, n, emb, ids, B, I, O, "vqx_linear_batched_fwd_ids")) return -1;
  hipLaunchKernelGGL(linear_cond_fwd_kernel, dim3(O / kCondO, n), dim3(256), 0, (hipStream_t)stream, table_dev, emb, ids,
                     B, O);
  return launch_status("vqx_linear_batched_fwd_ids");
}

extern "C" int vqx_step_prologue(const vqx_wn_layer* wn_host, const vqx_wn_layer* wn_dev, int32_t n_wn,
                                 const vqx_linear_layer* cond_table_dev, int32_t n_cond, const float* emb,
                                 const int64_t* ids, int32_t B, int32_t I, int32_t O, const float* x_nct, int32_t xB,
                                 int32_t C, int32_t T, void* y, int32_t ldy, int32_t y_dtype, vqx_stream_t stream) {
  WnUnits U;
  U.n = 0;
  U.off[0] = 0;
  if (n_wn < 0 || n_wn > kWnMaxL || (n_wn && (!wn_host || !wn_dev))) { set_error("vqx_step_prologue: 0 <= n_wn <= %d layers with both tables", kWnMaxL); return -1; }
  if (n_wn) {
    if (wn_fwd_check(wn_host, n_wn, "vqx_step_prologue") < 0) return -1;
    U.n = n_wn;
    for (int i = 0; i < n_wn; ++i) U.off[i + 1] = U.off[i] + wn_pack_units(wn_host[i]);
  }
  if (n_cond < 0 || (n_cond && !linear_ids_ok(cond_table_dev, n_cond, emb, ids, B, I, O, "vqx_step_prologue"))) return -1;
  if (x_nct && (xB < 1 || C < 1 || T < 1 || !y || ldy < C || (y_dtype != VQX_F32 && y_dtype != VQX_BF16))) { set_error("vqx_step_prologue: bad transpose arguments"); return -1; }
  const int cond_bx = n_cond ? O / kCondO : 1, n_cond_blocks = n_cond * (n_cond ? O / kCondO : 0);
  const int tx_bx = x_nct ? (T + 31) / 32 : 1, tx_by = x_nct ? (C + 31) / 32 : 1;
  const int64_t n_tx = x_nct ? (int64_t)tx_bx * tx_by * xB : 0;
  const int64_t grid = n_cond_blocks + n_tx + U.off[U.n];
  if (grid > INT32_MAX) { set_error("vqx_step_prologue: grid too large"); return -1; }
  if (grid == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (y_dtype == VQX_BF16)
    hipLaunchKernelGGL(step_prologue_kernel<bf16_t>, dim3((unsigned)grid), dim3(256), 0, s, wn_dev, U, cond_table_dev,
                       n_cond_blocks, cond_bx, emb, ids, B, O, x_nct, C, T, tx_bx, tx_by, (int)n_tx, (bf16_t*)y, ldy);
  else
    hipLaunchKernelGGL(step_prologue_kernel<float>, dim3((unsigned)grid), dim3(256), 0, s, wn_dev, U, cond_table_dev,
                       n_cond_blocks, cond_bx, emb, ids, B, O, x_nct, C, T, tx_bx, tx_by, (int)n_tx, (float*)y, ldy);
  return launch_status("vqx_step_prologue");
}

extern "C" int vqx_linear_batched_bwd_ids(const vqx_linear_layer* table_dev, int32_t n, const float* emb,
                                          const int64_t* ids, int32_t B, int32_t I, int32_t O, float* dc,
                                          float* partials, vqx_stream_t stream) {
  if (!linear_ids_ok(table_dev, n, emb, ids, B, I, O, "vqx_linear_batched_bwd_ids")) return -1;
  if (dc && !partials) { set_error("vqx_linear_batched_bwd_ids: dc needs partials [n*O/64][B][I]"); return -1; }
  hipStream_t s = (hipStream_t)stream;
  if (!dc || 2 * (int64_t)n > 65535) {  // (grid y: 2n)
    hipLaunchKernelGGL(linear_cond_bwd_w_kernel, dim3(O / kCondO, n), dim3(256), 0, s, table_dev, emb, ids, B, O);
    if (dc)
      hipLaunchKernelGGL(linear_cond_bwd_x_kernel, dim3(O / kCondO, n), dim3(256), 0, s, table_dev, B, O, partials);
  } else {  // the weight and data gradients in one grid (round 6: two launches)
    hipLaunchKernelGGL(linear_cond_bwd_kernel, dim3(O / kCondO, 2 * n), dim3(256), 0, s, table_dev, emb, ids, B, O, n,
                       partials);
  }
  if (dc) {
    const int64_t ne = (int64_t)B * I;
    hipLaunchKernelGGL(sum_slices_wide_kernel, dim3((unsigned)((ne + 63) / 64)), dim3(256), 0, s, partials,
                       n * (O / kCondO), ne, dc);
  }
  return launch_status("vqx_linear_batched_bwd_ids");
}

extern "C" int vqx_linear_f32(const float* c, const float* W, const float* bias, int32_t B, int32_t I, int32_t O,
                              float* out, vqx_stream_t stream) {
  hipLaunchKernelGGL(linear_fwd_kernel, dim3(grid_for((int64_t)B * O, 256, 1 << 20)), dim3(256), 0, (hipStream_t)stream, c, W, bias, B, I, O, out);
  return launch_status("vqx_linear_f32");
}

extern "C" int vqx_linear_bwd_f32(const float* dout, const float* c, const float* W, int32_t B, int32_t I, int32_t O,
                                  float* dW, float* dc, vqx_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (dW) hipLaunchKernelGGL(linear_bwd_w_kernel, dim3(grid_for((int64_t)O * I, 256, 1 << 20)), dim3(256), 0, s, dout, c, B, I, O, dW);
  if (dc) hipLaunchKernelGGL(linear_bwd_x_kernel, dim3((I + 63) / 64, B), dim3(256), 0, s, dout, W, B, I, O, dc);
  return launch_status("vqx_linear_bwd_f32");
}
