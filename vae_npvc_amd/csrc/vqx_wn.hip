// Weight norm of the VQ-VAE training step (gfx950): row norms, the packed
// effective weights and the backward over the split-K weight-gradient slabs.
#include "vqx_common.h"
#include "vqx_wn_pack.h"
#include <math.h>

namespace vqx {

// torch.nn.utils.weight_norm(dim=0): w = v * (g / ||v||), norm over all dims
// but 0.  Conv1d: v[cout][cin][k], row o = co.  ConvT: v[cin][cout][k], row
// o = ci, effective tap j' = k-1-j.  Packed effective weight:
// wp[co][j*cin + ci].
// Row norms of the ConvTranspose layers (rows = cin, contiguous cout*k):
// one 256-thread block per row in the canonical order (sq4, vqx_wn_pack.h).
// Conv1d layers get theirs in the pack.
__global__ __launch_bounds__(256) void wn_norm_kernel(const vqx_wn_layer* __restrict__ L, int n_layers) {
  const vqx_wn_layer& l = L[blockIdx.y];
  if (l.kind != 1 || !l.g) return;
  const int o = blockIdx.x;
  if (o >= l.cin) return;
  __shared__ float red[16];
  const int cols = l.cout * l.k;
  const float* v = l.v + (int64_t)o * cols;
  float s = 0.f;
  if ((cols & 3) == 0 && (((uintptr_t)v) & 15) == 0 && cols <= 4096) {
    // the thread's 16-B loads all in flight before the first add
    f32x4_t xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      xv[u] = 1024 * u < cols ? *(const f32x4_t*)(v + min((int)threadIdx.x * 4 + 1024 * u, cols - 4))
                              : f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const f32x4_t x = xv[u];
      if ((int)threadIdx.x * 4 + 1024 * u < cols)
        s = sq4(x, s);
    }
  } else {
    for (int i = threadIdx.x; i < cols; i += 256) s = fmaf(v[i], v[i], s);
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) l.norm[o] = sqrtf(s);
}

// the pack: one wn_pack_block (vqx_wn_pack.h) per unit of the flat grid
__global__ __launch_bounds__(256) void wn_pack_kernel(const vqx_wn_layer* __restrict__ L, WnUnits U) {
  __shared__ __attribute__((aligned(16))) float buf[kWnBuf];
  __shared__ float red[16];
  wn_pack_block(L, U, (int)blockIdx.x, buf, red);
}

// Sum over splits sp0, sp0+step, ... < splits of the 4 slab values at element
// offset p (slab stride `ss`): NF loads issued before any add, added in split
// order into one accumulator (fixed order: deterministic).
#ifndef VQX_WN_NF  // loads in flight per thread
#define VQX_WN_NF 4
#endif
#ifndef VQX_WN_THREADS  // threads per row block: the slab stream is bound by the loads in flight per CU
#define VQX_WN_THREADS 256
#endif
constexpr int kWnNF = VQX_WN_NF;
constexpr int kWnThreads = VQX_WN_THREADS;
static_assert(kWnThreads == 256, "vqx_gemm_kernel.h wgrad_tile_fixup reproduces the split grouping of 256-thread blocks");
template <bool BF>
__device__ __forceinline__ f32x4_t slab_sum(const void* slabs, int64_t p, int64_t ss, int sp0, int step, int splits) {
  typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
  auto cvt = [](u32x2_t u) -> f32x4_t {
    return {__uint_as_float(u[0] << 16), __uint_as_float(u[0] & 0xffff0000u), __uint_as_float(u[1] << 16),
            __uint_as_float(u[1] & 0xffff0000u)};
  };
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  int sp = sp0;
  if constexpr (BF) {
    const unsigned short* sl = (const unsigned short*)slabs;
    for (; sp + (kWnNF - 1) * step < splits; sp += kWnNF * step) {
      u32x2_t t[kWnNF];
#pragma unroll
      for (int u = 0; u < kWnNF; ++u) t[u] = *(const u32x2_t*)(sl + p + (int64_t)(sp + u * step) * ss);
#pragma unroll
      for (int u = 0; u < kWnNF; ++u) acc += cvt(t[u]);
    }
    u32x2_t t[kWnNF];
#pragma unroll
    for (int u = 0; u < kWnNF - 1; ++u)
      if (sp + u * step < splits) t[u] = *(const u32x2_t*)(sl + p + (int64_t)(sp + u * step) * ss);
#pragma unroll
    for (int u = 0; u < kWnNF - 1; ++u)
      if (sp + u * step < splits) acc += cvt(t[u]);
  } else {
    const float* sl = (const float*)slabs;
    for (; sp + (kWnNF - 1) * step < splits; sp += kWnNF * step) {
      f32x4_t t[kWnNF];
#pragma unroll
      for (int u = 0; u < kWnNF; ++u) t[u] = *(const f32x4_t*)(sl + p + (int64_t)(sp + u * step) * ss);
#pragma unroll
      for (int u = 0; u < kWnNF; ++u) acc += t[u];
    }
    f32x4_t t[kWnNF];
#pragma unroll
    for (int u = 0; u < kWnNF - 1; ++u)
      if (sp + u * step < splits) t[u] = *(const f32x4_t*)(sl + p + (int64_t)(sp + u * step) * ss);
#pragma unroll
    for (int u = 0; u < kWnNF - 1; ++u)
      if (sp + u * step < splits) acc += t[u];
  }
  return acc;
}
// slab_sum<true> (splits 0, 1, ... in order) of two column groups at once,
// p0 and p1: twice the loads in flight.  Buffer loads through one descriptor
// over the slabs (slab bytes < 2^31, caller-checked): a VGPR offset per
// column and the split's offset in an SGPR, where flat loads would hold a
// 64-bit address per load (84 VGPRs: five waves per SIMD instead of eight).
__device__ __forceinline__ void slab_sum2_bf(const void* slabs, int sbytes, int64_t p0, int64_t p1, int64_t ss,
                                             int splits, f32x4_t& a0, f32x4_t& a1) {
  typedef int i32x2_t __attribute__((ext_vector_type(2)));
  auto cvt = [](i32x2_t u) -> f32x4_t {
    return {__uint_as_float((unsigned)u[0] << 16), __uint_as_float((unsigned)u[0] & 0xffff0000u),
            __uint_as_float((unsigned)u[1] << 16), __uint_as_float((unsigned)u[1] & 0xffff0000u)};
  };
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)slabs, (short)0, sbytes, 0x00020000);
  const int v0 = (int)(p0 * 2), v1 = (int)(p1 * 2), sstep = (int)(ss * 2);
  a0 = f32x4_t{0.f, 0.f, 0.f, 0.f};
  a1 = a0;
  int sp = 0;
  for (; sp + kWnNF - 1 < splits; sp += kWnNF) {
    i32x2_t t0[kWnNF], t1[kWnNF];
#pragma unroll
    for (int u = 0; u < kWnNF; ++u) {
      t0[u] = __builtin_amdgcn_raw_buffer_load_b64(rs, v0, (sp + u) * sstep, 0);
      t1[u] = __builtin_amdgcn_raw_buffer_load_b64(rs, v1, (sp + u) * sstep, 0);
    }
#pragma unroll
    for (int u = 0; u < kWnNF; ++u) {
      a0 += cvt(t0[u]);
      a1 += cvt(t1[u]);
    }
  }
  i32x2_t t0[kWnNF], t1[kWnNF];
#pragma unroll
  for (int u = 0; u < kWnNF - 1; ++u)
    if (sp + u < splits) {
      t0[u] = __builtin_amdgcn_raw_buffer_load_b64(rs, v0, (sp + u) * sstep, 0);
      t1[u] = __builtin_amdgcn_raw_buffer_load_b64(rs, v1, (sp + u) * sstep, 0);
    }
#pragma unroll
  for (int u = 0; u < kWnNF - 1; ++u)
    if (sp + u < splits) {
      a0 += cvt(t0[u]);
      a1 += cvt(t1[u]);
    }
}

// Backward per weight-norm row o.  slabs[s][o][x] with x = j*cin+ci (Conv1d,
// row co) or x = j'*cout+co (ConvT, row ci); dW of the effective conv.
// The split-K slabs (fp32, or bf16 in bf16 runs) are summed in fp32 with
// 16-B (8-B) loads, several splits in flight per thread, scattered into the
// row's (c, j) order in LDS, then the norm gradient is formed from LDS and the
// row of v held in registers.  One kWnThreads-thread block per row over a flat
// grid of every layer's rows (WnUnits): the big layers have only 512-640 rows,
// so the block -- not the grid -- must carry the loads in flight.
constexpr int kWnVRegs = 4096 / kWnThreads;  // v row values per thread (row length <= 4096)
constexpr int kWnCrCols = 32;  // columns per column-reduce block
// 16-B column groups per lane on the wave-per-row path (rows <= 256 columns:
// the conditioning linears' 128).  Four (rows <= 1024) cost the whole kernel
// 86 VGPRs, i.e. five waves per SIMD and 5/8 of the slab loads in flight; one
// keeps it at 64 VGPRs, eight waves per SIMD (157.4 -> 136.8 us a step,
// profiles/r05/wn_bwd_vec_ab.txt).
constexpr int kWnWaveX4 = 1;
// wave-per-row path: Conv1d 1x1 rows of <= 256 columns whose split sums are
// at most one round of loads per lane
__host__ __device__ inline bool wn_bwd_wave_rows(const vqx_wn_layer& l) {
  return l.kind == 0 && l.k == 1 && l.cin <= 64 * 4 * kWnWaveX4 && (l.cin / 4) * l.splits <= 64 * kWnNF;
}
// sq (optional, vqx_weight_norm_bwd_sq): every wave of block b stores the sum of
// squares of the gradient values it wrote at sq[4*b + wave] (0 if none): the
// global gradient norm's partial sums without re-reading the gradient.
__device__ __forceinline__ void wn_sq_store(float* sq, float q) {
  if (!sq) return;
  q = wave_sum(q);
  if ((threadIdx.x & 63) == 0) sq[(int64_t)blockIdx.x * (kWnThreads / 64) + (threadIdx.x >> 6)] = q;
}
__global__ __launch_bounds__(kWnThreads) void wn_bwd_kernel(const vqx_wn_layer* __restrict__ L, WnUnits U,
                                                            float* __restrict__ sq) {
  int lo = 0, hi = U.n - 1;  // the layer owning this block
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (U.off[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const vqx_wn_layer& l = L[lo];
  const int unit = (int)blockIdx.x - U.off[lo];
  if (l.kind == VQX_WN_COLREDUCE) {
    // dv[c] = sum_r v[r][c] (bias / affine gradients from per-tile partials):
    // block = kWnCrCols columns x kWnCrRG row groups, row group g summing rows
    // g, g + kWnCrRG, ... (8 loads in flight), then the groups in order
    // through LDS -- a fixed order, deterministic.
    constexpr int CC = kWnCrCols, RG = kWnThreads / kWnCrCols;
    __shared__ float crs[RG][CC];
    const int cl = threadIdx.x % CC, g = threadIdx.x / CC;
    const int c = unit * CC + cl;
    float a = 0.f;
    if (c < l.cout) {
      const float* p = l.v + c;
      int r = g;
      for (; r + 7 * RG < l.cin; r += 8 * RG) {
        float t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = p[(int64_t)(r + u * RG) * l.cout];
#pragma unroll
        for (int u = 0; u < 8; ++u) a += t[u];
      }
      for (; r < l.cin; r += RG) a += p[(int64_t)r * l.cout];
    }
    crs[g][cl] = a;
    __syncthreads();
    float q2 = 0.f;
    if (g == 0 && c < l.cout) {
      float t = 0.f;
#pragma unroll
      for (int q = 0; q < RG; ++q) t += crs[q][cl];
      l.dv[c] = t;
      q2 = t * t;
    }
    wn_sq_store(sq, q2);
    return;
  }
  if (wn_bwd_wave_rows(l)) {
    // short 1x1 rows with little split-K work (the speaker-conditioning
    // linears: 128 columns, dW written directly): one wave per row, the row's
    // sums held in registers, wave reductions only (no LDS, no barriers)
    const int o = unit * (kWnThreads / 64) + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (o >= l.cout) {
      wn_sq_store(sq, 0.f);
      return;
    }
    const int cols = l.cin, nx4 = cols / 4;
    const int64_t ss = (int64_t)l.cout * cols, srow = (int64_t)o * cols;
    const bool sbf = l.slab_dtype == VQX_BF16;
    const float* vrow = l.v + (int64_t)o * cols;
    float* dv = l.dv + (int64_t)o * cols;
    f32x4_t sm[kWnWaveX4], vv[kWnWaveX4];
    float dot = 0.f;
#pragma unroll
    for (int u = 0; u < kWnWaveX4; ++u) {
      const int x4 = lane + 64 * u;
      if (x4 < nx4) {
        vv[u] = l.g ? *(const f32x4_t*)(vrow + 4 * x4) : f32x4_t{0.f, 0.f, 0.f, 0.f};
        sm[u] = sbf ? slab_sum<true>(l.slabs, srow + 4 * x4, ss, 0, 1, l.splits)
                    : slab_sum<false>(l.slabs, srow + 4 * x4, ss, 0, 1, l.splits);
        dot = fmaf(sm[u][0], vv[u][0], fmaf(sm[u][1], vv[u][1], fmaf(sm[u][2], vv[u][2], fmaf(sm[u][3], vv[u][3], dot))));
      }
    }
    float q2 = 0.f;
    if (!l.g) {
#pragma unroll
      for (int u = 0; u < kWnWaveX4; ++u)
        if (lane + 64 * u < nx4) {
          *(f32x4_t*)(dv + 4 * (lane + 64 * u)) = sm[u];
          q2 = fmaf(sm[u][0], sm[u][0], fmaf(sm[u][1], sm[u][1], fmaf(sm[u][2], sm[u][2], fmaf(sm[u][3], sm[u][3], q2))));
        }
      wn_sq_store(sq, q2);
      return;
    }
    dot = wave_sum(dot);
    const float nrm = l.norm[o];
    const float dg = dot / nrm;
    if (lane == 0) {
      l.dg[o] = dg;
      q2 = dg * dg;
    }
    const float sc = l.g[o] / nrm, t = dg / nrm;
#pragma unroll
    for (int u = 0; u < kWnWaveX4; ++u)
      if (lane + 64 * u < nx4) {
        const f32x4_t r = {sc * (sm[u][0] - vv[u][0] * t), sc * (sm[u][1] - vv[u][1] * t),
                           sc * (sm[u][2] - vv[u][2] * t), sc * (sm[u][3] - vv[u][3] * t)};
        *(f32x4_t*)(dv + 4 * (lane + 64 * u)) = r;
        q2 = fmaf(r[0], r[0], fmaf(r[1], r[1], fmaf(r[2], r[2], fmaf(r[3], r[3], q2))));
      }
    wn_sq_store(sq, q2);
    return;
  }
  const bool rsm = l.kind == VQX_WN_RESAMPLE || l.kind == VQX_WN_RESAMPLE_T;
  const bool row_is_cout = l.kind == 0 || l.kind == VQX_WN_RESAMPLE;
  const int rows = row_is_cout ? l.cout : l.cin;
  const int o = unit;
  if (o >= rows) {
    wn_sq_store(sq, 0.f);
    return;
  }
  const int other = row_is_cout ? l.cin : l.cout;  // multiple of 4 (host-checked)
  const int K = l.k;
  const int cols = other * K;
  const int S = l.stride, SC = S * other;
  const int scols = rsm ? 3 * SC : cols;  // slab row: folded 3-tap row for the strided kinds
  __shared__ __attribute__((aligned(16))) float dw[4096];
  __shared__ float red[16];
  const int64_t slab_stride = (int64_t)rows * scols;
  const int64_t srow = (int64_t)o * scols;  // element offset of this row in split 0
  const int splits = l.splits;
  const bool sbf = l.slab_dtype == VQX_BF16;
  // the row of v, loaded before the slabs so both latencies overlap (cols <= 4096,
  // 256 threads): thread t holds the 4-element chunks c = t + 256u, 16-B loads
  // when the row is 16-B aligned (cols % 4 == 0: the data path moves a quarter
  // of the lane requests of element loads; this kernel's TD is ~90% busy)
  constexpr int kV4 = kWnVRegs / 4;
  f32x4_t vr4[kV4];
  const float* vrow = l.v + (int64_t)o * cols;
  float* dv = l.dv + (int64_t)o * cols;
  const bool al16 = ((((uintptr_t)vrow) | ((uintptr_t)dv)) & 15) == 0;
#pragma unroll
  for (int u = 0; u < kV4; ++u) {
    const int i = 4 * ((int)threadIdx.x + u * kWnThreads);
    vr4[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if (l.g && i < cols) {
      if (al16) {
        vr4[u] = *(const f32x4_t*)(vrow + i);
      } else {
        vr4[u] = f32x4_t{vrow[i], vrow[i + 1], vrow[i + 2], vrow[i + 3]};
      }
    }
  }
  // Thread t sums the splits g, g+G, ... of column group x4 = t % nx4 (G = the
  // threads per group when a row has fewer than 256 groups), eight loads in
  // flight, then the G partial sums are added in g order through LDS: a fixed
  // order, so the result is deterministic.  The slab dtype is a template
  // argument of the summing loop (a dtype branch per load kept the loads from
  // being issued together).
  const int nx4 = scols / 4;
  const int G = nx4 >= (int)blockDim.x ? 1 : min(splits, (int)blockDim.x / nx4);
  const int gidx = threadIdx.x / nx4;  // split group (G == 1: every thread is group 0)
  f32x4_t* part = (f32x4_t*)dw;        // [G][nx4] partials (G > 1 only: nx4 * G <= kWnThreads -> <= 16 KiB)
  // slab column x -> dw[v index] (4 consecutive columns share the mapping)
  auto scatter = [&](int x4, const f32x4_t& sum) {
    const int x = 4 * x4;
    if (rsm) {  // slab col x = m*S*C + q*C + c -> v index c*K + S*(m-1) + q + pad (4 c's share m, q)
      const int m = x / SC, rem = x - m * SC, q = rem / other, c = rem - q * other;
      const int j = S * (m - 1) + q + l.pad;
      if (j >= 0 && j < K) {
#pragma unroll
        for (int e = 0; e < 4; ++e) dw[(c + e) * K + j] = sum[e];
      }
      return;
    }
    // slab col x = j*other + c  -> v index c*K + (kind==0 ? j : K-1-j)
    const int j = x / other, c = x - j * other;
    const int jj = l.kind == 0 ? j : K - 1 - j;
#pragma unroll
    for (int e = 0; e < 4; ++e) dw[(c + e) * K + jj] = sum[e];
  };
  const int64_t sbytes = (int64_t)splits * slab_stride * 2;
  if (G == 1 && sbf && sbytes < ((int64_t)1 << 31)) {
    // bf16 slabs: column groups x4 and x4 + 256 summed together (the 3-tap
    // rows have 384-768 groups and 4-8 splits: one pass of 8-16 loads)
    for (int x4 = threadIdx.x; x4 < nx4; x4 += 2 * kWnThreads) {
      const int x4b = x4 + kWnThreads;
      const bool hb = x4b < nx4;
      f32x4_t s0, s1;
      slab_sum2_bf(l.slabs, (int)sbytes, srow + 4 * x4, srow + 4 * (hb ? x4b : x4), slab_stride, splits, s0, s1);
      scatter(x4, s0);
      if (hb) scatter(x4b, s1);
    }
  } else {
    // G == 1: x4 = t, t + 256, ...;  G > 1: the one group x4 = t % nx4 (threads with gidx >= G idle)
    const int x4_0 = G == 1 ? (int)threadIdx.x : ((int)threadIdx.x % nx4 + (gidx < G ? 0 : nx4));
    for (int x4 = x4_0; x4 < nx4; x4 += (G == 1 ? (int)blockDim.x : nx4)) {
      const int64_t p = srow + 4 * x4;
      const int sp0 = G > 1 ? gidx : 0, step = G > 1 ? G : 1;
      const f32x4_t sum = sbf ? slab_sum<true>(l.slabs, p, slab_stride, sp0, step, splits)
                              : slab_sum<false>(l.slabs, p, slab_stride, sp0, step, splits);
      if (G > 1) part[gidx * nx4 + x4] = sum;
      else scatter(x4, sum);
    }
  }
  if (G > 1) {  // add the split groups' partials in group order, then scatter as above
    __syncthreads();
    f32x4_t sum = {0.f, 0.f, 0.f, 0.f};
    const int x4 = threadIdx.x;
    if (x4 < nx4)
      for (int g = 0; g < G; ++g) sum += part[g * nx4 + x4];
    __syncthreads();  // dw doubles as the partial buffer
    if (x4 < nx4) scatter(x4, sum);
  }
  __syncthreads();
  float q2 = 0.f;
  auto store4 = [&](int i, const f32x4_t& r) {
    if (al16) {
      *(f32x4_t*)(dv + i) = r;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) dv[i + k] = r[k];
    }
  };
  if (!l.g) {  // plain weight (weight norm removed): dv is the weight gradient itself
#pragma unroll
    for (int u = 0; u < kV4; ++u) {
      const int i = 4 * ((int)threadIdx.x + u * kWnThreads);
      if (i < cols) {
        const f32x4_t r = *(const f32x4_t*)(dw + i);
        store4(i, r);
#pragma unroll
        for (int k = 0; k < 4; ++k) q2 = fmaf(r[k], r[k], q2);
      }
    }
    wn_sq_store(sq, q2);
    return;
  }
  float dot = 0.f;
#pragma unroll
  for (int u = 0; u < kV4; ++u) {
    const int i = 4 * ((int)threadIdx.x + u * kWnThreads);
    if (i < cols) {
      const f32x4_t d4 = *(const f32x4_t*)(dw + i);
#pragma unroll
      for (int k = 0; k < 4; ++k) dot = fmaf(d4[k], vr4[u][k], dot);
    }
  }
  dot = block_sum(dot, red);
  const float nrm = l.norm[o];
  const float gg = l.g[o];
  const float dg = dot / nrm;
  if (threadIdx.x == 0) {
    l.dg[o] = dg;
    q2 = dg * dg;
  }
  const float sc = gg / nrm, t = dg / nrm;
#pragma unroll
  for (int u = 0; u < kV4; ++u) {
    const int i = 4 * ((int)threadIdx.x + u * kWnThreads);
    if (i < cols) {
      const f32x4_t d4 = *(const f32x4_t*)(dw + i);
      f32x4_t r;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        r[k] = sc * (d4[k] - vr4[u][k] * t);
        q2 = fmaf(r[k], r[k], q2);
      }
      store4(i, r);
    }
  }
  wn_sq_store(sq, q2);
}

}  // namespace vqx

using namespace vqx;

static int wn_fwd_launch(const vqx_wn_layer* lh, const vqx_wn_layer* ld, int32_t n_layers, int32_t flags,
                         vqx_stream_t stream) {
  if (!lh || !ld || n_layers <= 0) { set_error("vqx_weight_norm_fwd: bad tables"); return -1; }
  const int max_t_rows = wn_fwd_check(lh, n_layers, "vqx_weight_norm_fwd");
  if (max_t_rows < 0) return -1;
  hipStream_t s = (hipStream_t)stream;
  if (!(flags & VQX_WNF_NORMS_READY))
    hipLaunchKernelGGL(wn_norm_kernel, dim3(max_t_rows, n_layers), dim3(256), 0, s, ld, n_layers);
  for (int i0 = 0; i0 < n_layers; i0 += kWnMaxL) {  // flat grid over the layers' units, kWnMaxL layers a launch
    WnUnits U;
    U.n = n_layers - i0 < kWnMaxL ? n_layers - i0 : kWnMaxL;
    U.off[0] = 0;
    for (int i = 0; i < U.n; ++i) U.off[i + 1] = U.off[i] + wn_pack_units(lh[i0 + i]);
    if (U.off[U.n] > 0) hipLaunchKernelGGL(wn_pack_kernel, dim3(U.off[U.n]), dim3(256), 0, s, ld + i0, U);
  }
  return launch_status("vqx_weight_norm_fwd");
}

extern "C" int vqx_weight_norm_fwd(const vqx_wn_layer* lh, const vqx_wn_layer* ld, int32_t n_layers,
                                   vqx_stream_t stream) {
  return wn_fwd_launch(lh, ld, n_layers, 0, stream);
}

extern "C" int vqx_weight_norm_fwd_flags(const vqx_wn_layer* lh, const vqx_wn_layer* ld, int32_t n_layers,
                                         int32_t flags, vqx_stream_t stream) {
  return wn_fwd_launch(lh, ld, n_layers, flags, stream);
}

static int wn_bwd_units(const vqx_wn_layer& l) {
  return l.kind == VQX_WN_COLREDUCE ? (l.cout + kWnCrCols - 1) / kWnCrCols
         : wn_bwd_wave_rows(l)       ? (l.cout + kWnThreads / 64 - 1) / (kWnThreads / 64)
         : (l.kind == 0 || l.kind == VQX_WN_RESAMPLE) ? l.cout
                                                      : l.cin;
}

static int wn_bwd_launch(const vqx_wn_layer* lh, const vqx_wn_layer* ld, int32_t n_layers, float* sq,
                         int64_t sq_capacity, vqx_stream_t stream) {
  if (!lh || !ld || n_layers <= 0) { set_error("vqx_weight_norm_bwd: bad tables"); return -1; }
  if (sq) {
    int64_t need = 0;
    vqx_weight_norm_bwd_partials(lh, n_layers, &need);
    if (sq_capacity < need) { set_error("vqx_weight_norm_bwd_sq: %lld partials < %lld", (long long)sq_capacity, (long long)need); return -1; }
  }
  for (int i = 0; i < n_layers; ++i) {
    const vqx_wn_layer& l = lh[i];
    if (l.kind == VQX_WN_COLREDUCE) {
      if (!l.v || !l.dv || l.cin < 1 || l.cout < 1) { set_error("vqx_weight_norm_bwd: column-reduce entry %d", i); return -1; }
      continue;
    }
    if (l.kind != 0 && l.kind != 1 && l.kind != VQX_WN_RESAMPLE && l.kind != VQX_WN_RESAMPLE_T) { set_error("vqx_weight_norm_bwd: layer %d bad kind", i); return -1; }
    if (l.kind >= VQX_WN_RESAMPLE && !(l.stride >= 1 && l.pad >= 0 && l.pad <= l.stride && l.k - 1 - l.pad < 2 * l.stride)) { set_error("vqx_weight_norm_bwd: layer %d: bad resampling geometry", i); return -1; }
    const bool row_is_cout = l.kind == 0 || l.kind == VQX_WN_RESAMPLE;
    const int cols = (row_is_cout ? l.cin : l.cout) * l.k;
    if (cols > 4096) { set_error("vqx_weight_norm_bwd: row length %d > 4096", cols); return -1; }
    if (!l.slabs || !l.dv || (l.g && !l.dg) || l.splits < 1) { set_error("vqx_weight_norm_bwd: layer %d missing buffers", i); return -1; }
    if ((row_is_cout ? l.cin : l.cout) % 4 || ((uintptr_t)l.slabs & 15)) { set_error("vqx_weight_norm_bwd: layer %d: slab rows must be 16-B vectors", i); return -1; }
    if (l.slab_dtype != VQX_F32 && l.slab_dtype != VQX_BF16) { set_error("vqx_weight_norm_bwd: layer %d: slab_dtype %d", i, l.slab_dtype); return -1; }
  }
  for (int i0 = 0; i0 < n_layers; i0 += kWnMaxL) {  // flat grid over the layers' rows, kWnMaxL layers a launch
    WnUnits U;
    U.n = n_layers - i0 < kWnMaxL ? n_layers - i0 : kWnMaxL;
    U.off[0] = 0;
    for (int i = 0; i < U.n; ++i) U.off[i + 1] = U.off[i] + wn_bwd_units(lh[i0 + i]);
    if (U.off[U.n] > 0)
      hipLaunchKernelGGL(wn_bwd_kernel, dim3(U.off[U.n]), dim3(kWnThreads), 0, (hipStream_t)stream, ld + i0, U, sq);
    if (sq) sq += (int64_t)U.off[U.n] * (kWnThreads / 64);
  }
  return launch_status("vqx_weight_norm_bwd");
}

extern "C" int vqx_weight_norm_bwd(const vqx_wn_layer* lh, const vqx_wn_layer* ld, int32_t n_layers,
                                   vqx_stream_t stream) {
  return wn_bwd_launch(lh, ld, n_layers, nullptr, 0, stream);
}

extern "C" int vqx_weight_norm_bwd_partials(const vqx_wn_layer* lh, int32_t n_layers, int64_t* count) {
  if (!lh || n_layers <= 0 || !count) { set_error("vqx_weight_norm_bwd_partials: bad arguments"); return -1; }
  int64_t b = 0;
  for (int i = 0; i < n_layers; ++i) b += wn_bwd_units(lh[i]);
  *count = b * (kWnThreads / 64);
  return 0;
}

extern "C" int vqx_weight_norm_bwd_sq(const vqx_wn_layer* lh, const vqx_wn_layer* ld, int32_t n_layers,
                                      float* sq_partials, int64_t sq_capacity, vqx_stream_t stream) {
  if (!sq_partials) { set_error("vqx_weight_norm_bwd_sq: null partials"); return -1; }
  return wn_bwd_launch(lh, ld, n_layers, sq_partials, sq_capacity, stream);
}
