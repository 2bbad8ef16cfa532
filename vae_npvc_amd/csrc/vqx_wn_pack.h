// One unit of the weight-norm pack grid and the host check of its tables.
// Used by vqx_wn.hip (wn_pack_kernel), vqx_linear.hip (step_prologue_kernel)
// and vqx_optim.hip (adam_wn_kernel).
#pragma once
#include "vqx_common.h"

namespace vqx {

// Pack w = g*v/||v|| into the effective-conv layout wp[co][j][ci].
// kind 0 (Conv1d, v[co][ci][j]), K > 1: block = one row co: the row is read
//   contiguously into LDS, its norm reduced there (and saved), then written
//   transposed [j][ci] with coalesced stores.
// kind 0, K = 1: no transpose: block = 4 rows, one wave each (16-B loads, a
//   wave reduction, then the scaled row re-read from cache and stored 8 B a
//   lane) -- no LDS, no barriers.
// kind 1 (ConvT, v[ci][co][K-1-j]): block = a 64 ci x TCO co tile, read row
//   segments (TCO*K contiguous floats per ci; 384 B for K = 3) into LDS, write
//   wp[co][j][ci0..] rows of 64 consecutive ci, 16 B a lane.
// The grid is flat over every layer's units (WnUnits: per-layer prefix), so
// no workgroup of a small layer launches only to exit.
constexpr int kWnRow = 4096;
constexpr int kWnMaxL = 256;  // layers per launch (the host launches larger tables in chunks; 1 KiB of kernel argument)
struct WnUnits {
  int n;
  int off[kWnMaxL + 1];
};
// ConvT pack tile width in co: the LDS tile holds 64 ci x (TCO*K + pad) floats
__host__ __device__ inline int wn_tco(int K) { return K <= 3 ? 32 : K <= 4 ? 16 : (K <= 64 ? 64 / K : 1); }
constexpr int kWnBuf = 96 * 65;  // floats: the K = 3 ConvT tile (>= kWnRow + 64 for the Conv1d rows)
static_assert(kWnBuf >= kWnRow + 64, "wn pack LDS");
__host__ __device__ inline int wn_pack_units(const vqx_wn_layer& l) {
  if (l.kind == VQX_WN_RESAMPLE) return l.cout;
  if (l.kind == VQX_WN_RESAMPLE_T) return l.cin;
  if (l.kind == 0) return l.k == 1 ? (l.cout + 3) / 4 : l.cout;
  return ((l.cin + 63) / 64) * ((l.cout + wn_tco(l.k) - 1) / wn_tco(l.k));
}

// ---- the canonical row code.  wn_norm_kernel, wn_pack_block and
// adam_wn_kernel must give the same norm and the same packed weight from the
// same parameters, bit for bit: they differ in how a row is loaded (Adam
// updates it on the way) and share everything after that.
// Row norm: a 256-thread block per row (thread t the elements 4t + 1024u +
// (0..3)) or a wave per row (lane l the elements 4l + 256u + (0..3)), each
// 16-B group added to the thread's sum by sq4 in u order, then block_sum /
// wave_sum.
__device__ __forceinline__ float sq4(const f32x4_t x, float s) {
  return fmaf(x[0], x[0], fmaf(x[1], x[1], fmaf(x[2], x[2], fmaf(x[3], x[3], s))));
}
// Conv1d, k > 1: row co of v in LDS (buf[ci*K + j]), scaled by sc, into
// wp[co][j*cin + ci]; 256 threads, after the barrier that publishes buf
__device__ __forceinline__ void wn_store_row_lds(const vqx_wn_layer& l, int co, int cin, int K,
                                                 const float* __restrict__ buf, float sc) {
  const int cols = cin * K;
  bf16_t* wb = (bf16_t*)l.w_packed + (int64_t)co * cols;
  if (l.dtype == VQX_BF16 && (cin & 3) == 0 && (((uintptr_t)wb) & 7) == 0) {
    for (int e = threadIdx.x * 4; e < cols; e += 1024) {  // 4 consecutive ci of one tap, 8 B a lane
      const int j = e / cin, ci = e - j * cin;
      const float* b = buf + ci * K + j;
      *(uint2*)(wb + e) = make_uint2(pack_bf16x2(b[0] * sc, b[K] * sc), pack_bf16x2(b[2 * K] * sc, b[3 * K] * sc));
    }
    return;
  }
  for (int e = threadIdx.x; e < cols; e += 256) {  // e = j*cin + ci
    const int j = e / cin, ci = e - j * cin;
    st_dt(l.w_packed, (int64_t)co * cols + e, buf[ci * K + j] * sc, l.dtype);
  }
}
// Conv1d, k = 1 (a wave per row): the 16-B group x of row co at column i,
// scaled by sc, into wp[co][i .. i+3] (8 B of bf16 or 16 B of f32, aligned)
__device__ __forceinline__ void wn_store_row4(const vqx_wn_layer& l, int co, int cin, int i, const f32x4_t x,
                                              float sc) {
  if (l.dtype == VQX_BF16) {
    *(uint2*)((bf16_t*)l.w_packed + (int64_t)co * cin + i) =
        make_uint2(pack_bf16x2(x[0] * sc, x[1] * sc), pack_bf16x2(x[2] * sc, x[3] * sc));
  } else {
    *(f32x4_t*)((float*)l.w_packed + (int64_t)co * cin + i) = f32x4_t{x[0] * sc, x[1] * sc, x[2] * sc, x[3] * sc};
  }
}

// one unit of the flat grid (bid: the block's index in it); buf = kWnBuf
// floats of LDS (16-B aligned), red = 16
__device__ __forceinline__ void wn_pack_block(const vqx_wn_layer* __restrict__ L, const WnUnits& U, int bid,
                                              float* __restrict__ buf, float* __restrict__ red) {
  int lo = 0, hi = U.n - 1;  // the layer owning this block: largest li with off[li] <= bid
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (U.off[mid] <= bid) lo = mid; else hi = mid - 1;
  }
  const vqx_wn_layer& l = L[lo];
  const int unit = bid - U.off[lo];
  const int K = l.k, cin = l.cin, cout = l.cout;
  if (l.kind == VQX_WN_RESAMPLE || l.kind == VQX_WN_RESAMPLE_T) {
    // strided conv (include/vqx.h): row r of v, norm, then the folded 3-tap row
    // w_packed[r][m][q*C + c] = w[r][c][S*(m-1) + q + pad]
    const int rows = l.kind == VQX_WN_RESAMPLE ? cout : cin, C = l.kind == VQX_WN_RESAMPLE ? cin : cout;
    const int r = unit;
    if (r >= rows) return;
    const int cols = C * K;
    const float* v = l.v + (int64_t)r * cols;
    float s = 0.f;
    for (int i = threadIdx.x; i < cols; i += 256) {
      const float x = v[i];
      buf[i] = x;
      s = fmaf(x, x, s);
    }
    s = block_sum(s, red);
    float sc = 1.f;
    if (l.g) {
      const float nrm = sqrtf(s);
      if (threadIdx.x == 0) l.norm[r] = nrm;
      sc = l.g[r] / nrm;
    }
    const int S = l.stride, SC = S * C, W = 3 * SC;
    for (int e = threadIdx.x; e < W; e += 256) {
      const int m = e / SC, rem = e - m * SC, q = rem / C, c = rem - q * C;
      const int j = S * (m - 1) + q + l.pad;
      st_dt(l.w_packed, (int64_t)r * W + e, (j >= 0 && j < K) ? buf[c * K + j] * sc : 0.f, l.dtype);
    }
    return;
  }
  if (l.kind == 0 && K == 1) {
    const int co = unit * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (co >= cout) return;
    const float* v = l.v + (int64_t)co * cin;
    const bool vec = (cin & 3) == 0 && (((uintptr_t)v) & 15) == 0 &&
                     ((((uintptr_t)l.w_packed) + (int64_t)co * cin * (l.dtype == VQX_BF16 ? 2 : 4)) & 15) == 0;
    float s = 0.f;
    if (vec) {
      for (int i = lane * 4; i < cin; i += 256) {
        const f32x4_t x = *(const f32x4_t*)(v + i);
        s = sq4(x, s);
      }
    } else {
      for (int i = lane; i < cin; i += 64) s = fmaf(v[i], v[i], s);
    }
    s = wave_sum(s);
    float sc = 1.f;
    if (l.g) {
      const float nrm = sqrtf(s);
      if (lane == 0) l.norm[co] = nrm;
      sc = l.g[co] / nrm;
    }
    if (vec) {
      for (int i = lane * 4; i < cin; i += 256) wn_store_row4(l, co, cin, i, *(const f32x4_t*)(v + i), sc);
    } else {
      for (int i = lane; i < cin; i += 64) st_dt(l.w_packed, (int64_t)co * cin + i, v[i] * sc, l.dtype);
    }
    return;
  }
  if (l.kind == 0) {
    const int co = unit;
    if (co >= cout) return;
    const int cols = cin * K;
    const float* v = l.v + (int64_t)co * cols;
    float s = 0.f;
    // the row's loads all in flight before the first use (a load + use per
    // iteration of a runtime-bound loop paid one memory latency each)
    if ((cols & 3) == 0 && (((uintptr_t)v) & 15) == 0) {
      // 16-B partition: thread t holds elements 4t + 1024u + (0..3) (sq4: the canonical order)
      f32x4_t xv[kWnRow / 1024];
#pragma unroll
      for (int u = 0; u < kWnRow / 1024; ++u)
        xv[u] = 1024 * u < cols ? *(const f32x4_t*)(v + min((int)threadIdx.x * 4 + 1024 * u, cols - 4))
                                : f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < kWnRow / 1024; ++u) {
        const int i = (int)threadIdx.x * 4 + 1024 * u;
        if (i < cols) {
          const f32x4_t x = xv[u];
          *(f32x4_t*)(buf + i) = x;
          s = sq4(x, s);
        }
      }
    } else {
      float xr[kWnRow / 256];
#pragma unroll
      for (int u = 0; u < kWnRow / 256; ++u)
        xr[u] = 256 * u < cols ? v[min((int)threadIdx.x + 256 * u, cols - 1)] : 0.f;
#pragma unroll
      for (int u = 0; u < kWnRow / 256; ++u) {
        const int i = threadIdx.x + 256 * u;
        if (i < cols) {
          buf[i] = xr[u];
          s = fmaf(xr[u], xr[u], s);
        }
      }
    }
    s = block_sum(s, red);  // includes the barriers that publish buf
    float sc = 1.f;
    if (l.g) {
      const float nrm = sqrtf(s);
      if (threadIdx.x == 0) l.norm[co] = nrm;
      sc = l.g[co] / nrm;
    }
    wn_store_row_lds(l, co, cin, K, buf, sc);
    return;
  }
  // kind 1: tile of 64 ci x TCO co (x K taps) = 64 x TCO*K floats in LDS ([co_local*K + tap][ci], +1 pad)
  const int TCO = wn_tco(K);
  const int ntc = (cout + TCO - 1) / TCO;
  const int ci0 = (unit / ntc) * 64, co0 = (unit % ntc) * TCO;
  if (ci0 >= cin || K > 64) return;
  const int wseg = TCO * K;  // floats per ci row segment (contiguous in v)
  const bool full = ci0 + 64 <= cin && co0 + TCO <= cout;
  constexpr int kTileV4 = 6;  // 16-B loads per thread of a full tile: 64 x wseg floats, wseg <= 96
  if (full && (wseg & 3) == 0 && ((cout * K) & 3) == 0 && (((uintptr_t)l.v) & 15) == 0 && 64 * wseg <= kTileV4 * 1024) {
    const int w4 = wseg >> 2;
    // all of the thread's loads (row segments, gains, norms) in flight at once
    f32x4_t xv[kTileV4];
    float gs[kTileV4], ns[kTileV4];
    const float* __restrict__ gp = l.g;
    const float* __restrict__ np = l.norm;
#pragma unroll
    for (int u = 0; u < kTileV4; ++u) {
      const int e = min((int)threadIdx.x + 256 * u, 64 * w4 - 1), r = e / w4, q = (e - r * w4) * 4;
      const int ci = ci0 + r;
      xv[u] = 256 * u < 64 * w4 ? *(const f32x4_t*)(l.v + ((int64_t)ci * cout + co0) * K + q) : f32x4_t{0.f, 0.f, 0.f, 0.f};
      gs[u] = gp && 256 * u < 64 * w4 ? gp[ci] : 1.f;
      ns[u] = gp && 256 * u < 64 * w4 ? np[ci] : 1.f;
    }
#pragma unroll
    for (int u = 0; u < kTileV4; ++u) {
      const int e = threadIdx.x + 256 * u;
      if (e < 64 * w4) {
        const int r = e / w4, q = (e - r * w4) * 4;
        f32x4_t x = xv[u];
        if (gp) {
          const float sc = gs[u] / ns[u];
          x = f32x4_t{x[0] * sc, x[1] * sc, x[2] * sc, x[3] * sc};
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) buf[(q + k) * 65 + r] = x[k];
      }
    }
  } else {
    for (int e = threadIdx.x; e < 64 * wseg; e += 256) {
      const int r = e / wseg, q = e - r * wseg;  // r: ci offset, q = co_local*K + tap
      const int ci = ci0 + r, co = co0 + q / K;
      float x = 0.f;
      if (ci < cin && co < cout) {
        x = l.v[((int64_t)ci * cout + co0) * K + q];
        if (l.g) x *= l.g[ci] / l.norm[ci];
      }
      buf[q * 65 + r] = x;
    }
  }
  __syncthreads();
  const size_t es = l.dtype == VQX_BF16 ? 2 : 4;
  if (full && (cin & 7) == 0 && (((uintptr_t)l.w_packed) & 15) == 0) {
    for (int e = threadIdx.x; e < wseg * 8; e += 256) {  // e = (co_local*K + j)*8 + 8-ci chunk
      const int cj = e >> 3, r8 = (e & 7) * 8;
      const int cl = cj / K, j = cj - cl * K;
      const float* src = buf + (cl * K + (K - 1 - j)) * 65 + r8;
      const int64_t o = ((int64_t)(co0 + cl) * K + j) * cin + ci0 + r8;
      if (es == 2) {
        *(uint4*)((bf16_t*)l.w_packed + o) = make_uint4(pack_bf16x2(src[0], src[1]), pack_bf16x2(src[2], src[3]),
                                                        pack_bf16x2(src[4], src[5]), pack_bf16x2(src[6], src[7]));
      } else {
        *(f32x4_t*)((float*)l.w_packed + o) = f32x4_t{src[0], src[1], src[2], src[3]};
        *(f32x4_t*)((float*)l.w_packed + o + 4) = f32x4_t{src[4], src[5], src[6], src[7]};
      }
    }
  } else {
    for (int e = threadIdx.x; e < TCO * K * 64; e += 256) {  // e = (co_local*K + j)*64 + ci_local
      const int cj = e >> 6, r = e & 63;
      const int cl = cj / K, j = cj - cl * K;
      const int co = co0 + cl, ci = ci0 + r;
      if (co < cout && ci < cin)
        st_dt(l.w_packed, ((int64_t)co * K + j) * cin + ci, buf[(cl * K + (K - 1 - j)) * 65 + r], l.dtype);
    }
  }
}

// the pack kernel's limits on a host table; returns the most ConvT rows (the
// norm pre-pass's grid) or -1 with the error set
inline int wn_fwd_check(const vqx_wn_layer* lh, int32_t n_layers, const char* who) {
  int max_t_rows = 1;
  for (int i = 0; i < n_layers; ++i) {
    const vqx_wn_layer& l = lh[i];
    if (l.kind != 0 && l.kind != 1 && l.kind != VQX_WN_RESAMPLE && l.kind != VQX_WN_RESAMPLE_T) { set_error("%s: layer %d bad kind", who, i); return -1; }
    if (l.kind >= VQX_WN_RESAMPLE && !(l.stride >= 1 && l.pad >= 0 && l.pad <= l.stride && l.k - 1 - l.pad < 2 * l.stride)) { set_error("%s: layer %d: resampling conv needs 0 <= pad <= stride and k-1-pad < 2*stride", who, i); return -1; }
    const bool rsm = l.kind >= VQX_WN_RESAMPLE;
    const bool row_is_cout = l.kind == 0 || l.kind == VQX_WN_RESAMPLE;
    if ((row_is_cout ? l.cin : l.cout) * l.k > kWnRow || (!rsm && l.k > 64)) { set_error("%s: layer %d row too long", who, i); return -1; }
    if (l.kind == 1) max_t_rows = l.cin > max_t_rows ? l.cin : max_t_rows;
  }
  return max_t_rows;
}

}  // namespace vqx
