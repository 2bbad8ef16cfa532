// The global gradient norm and the optimizers (gfx950): Adam, RAdam, Adam
// fused with the next forward's weight-norm preparation, and the multi-tensor
// family for gradients that are separate tensors (flat p, m, v; the pack into
// one flat gradient for a collective).
#include "vqx_common.h"
#include "vqx_wn_pack.h"
#include <math.h>

namespace vqx {

constexpr int kNormBlocks = 1024;

__global__ __launch_bounds__(256) void sqnorm_partial_kernel(const float* __restrict__ g, int64_t n,
                                                             float* __restrict__ part) {
  __shared__ float red[16];
  float s = 0.f;
  const int64_t n4 = n / 4;
  const f32x4_t* g4 = (const f32x4_t*)g;
#pragma unroll 4
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const f32x4_t v = g4[i];
    s = fmaf(v[0], v[0], s); s = fmaf(v[1], v[1], s); s = fmaf(v[2], v[2], s); s = fmaf(v[3], v[3], s);
  }
  if (blockIdx.x == 0)
    for (int64_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) s = fmaf(g[i], g[i], s);
  s = block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// The global gradient norm from the weight-norm backward's partials
// (vqx_weight_norm_bwd_sq) and g^2 over the ranges [off, off+len) it did not
// write: kSqBlocks blocks each sum a fixed strided share of both into
// scratch[b], then one block adds the kSqBlocks values in order into out[0].
// Deterministic (fixed assignment and order).
constexpr int kSqBlocks = 256;  // one per CU: 64 left the pass at 9.6 us, latency-bound
__global__ __launch_bounds__(256) void sq_partial_sum_kernel(const float* __restrict__ part, int64_t np,
                                                             const float* __restrict__ g,
                                                             const int64_t* __restrict__ rng, int nr,
                                                             float* __restrict__ scratch) {
  __shared__ float red[16];
  const int64_t stride = (int64_t)kSqBlocks * 256;
  const int64_t j0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  // the first ranges' bounds load beside the partials (one latency, not one per range)
  constexpr int kR = 8;
  int64_t ro[kR], rl[kR];
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    const int rr = min(r, max(nr - 1, 0));
    ro[r] = nr ? rng[2 * rr] : 0;
    rl[r] = r < nr ? rng[2 * rr + 1] : 0;
  }
  float s = 0.f;
  // partials four at a time, clamped loads (no tail loop of single loads), added in index order
  for (int64_t i = j0; i < np; i += 4 * stride) {
    float t[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) t[u] = part[min(i + u * stride, np - 1)];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i + u * stride < np) s += t[u];
  }
  // each range's first element of this thread loaded together, then the ranges in order
  float gv[kR];
  if (nr > 0) {  // (g may be null without ranges)
#pragma unroll
    for (int r = 0; r < kR; ++r) gv[r] = g[ro[r] + min(j0, max(rl[r] - 1, (int64_t)0))];
  }
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    if (r >= nr) break;
    if (j0 < rl[r]) s = fmaf(gv[r], gv[r], s);
    for (int64_t j = j0 + stride; j < rl[r]; j += stride) s = fmaf(g[ro[r] + j], g[ro[r] + j], s);
  }
  for (int r = kR; r < nr; ++r) {
    const int64_t off = rng[2 * r], len = rng[2 * r + 1];
    for (int64_t j = j0; j < len; j += stride) s = fmaf(g[off + j], g[off + j], s);
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) scratch[blockIdx.x] = s;
}
// Adam's per-step scalars (StepLR'd lr, bias corrections) from the device step
// counter, which it advances; one thread
__device__ __forceinline__ void adam_hyper_eval(int64_t* __restrict__ step, double lr0, double gamma, int step_size,
                                                double b1, double b2, double eps, float* __restrict__ hyper) {
  const int64_t t = step[0] + 1;
  step[0] = t;
  const double lr = lr0 * pow(gamma, (double)((t - 1) / step_size));
  const double bc1 = 1.0 - pow(b1, (double)t);
  const double bc2 = 1.0 - pow(b2, (double)t);
  hyper[0] = (float)lr;
  hyper[1] = (float)(lr / bc1);
  hyper[2] = (float)sqrt(bc2);
  hyper[3] = (float)t;
  hyper[4] = (float)(1.0 - b1);
  hyper[5] = (float)b2;
  hyper[6] = (float)(1.0 - b2);
  hyper[7] = (float)eps;
}

__global__ void adam_hyper_kernel(int64_t* __restrict__ step, double lr0, double gamma, int step_size, double b1,
                                  double b2, double eps, float* __restrict__ hyper) {
  adam_hyper_eval(step, lr0, gamma, step_size, b1, b2, eps, hyper);
}

// the second level of vqx_sq_norm_finish; with hyper != null (vqx_sq_norm_finish_adam)
// thread 0 also evaluates Adam's per-step scalars: one launch fewer
struct AdamHyperArgs {
  int64_t* step;
  double lr0, gamma, b1, b2, eps;
  int step_size;
  float* hyper;
};
__global__ __launch_bounds__(kSqBlocks) void sq_final_kernel(const float* __restrict__ scratch, float* __restrict__ out,
                                                             AdamHyperArgs H) {
  __shared__ float red[16];
  const float s = block_sum(scratch[threadIdx.x], red);
  if (threadIdx.x == 0) {
    out[0] = s;
    if (H.hyper) adam_hyper_eval(H.step, H.lr0, H.gamma, H.step_size, H.b1, H.b2, H.eps, H.hyper);
  }
}

// RAdam (trainer/radam.py:15-78): rectification decided once per step on the
// device, in double like the reference's Python floats.
__global__ void radam_hyper_kernel(int64_t* __restrict__ step, double lr0, double gamma, int step_size, double b1,
                                   double b2, double eps, float* __restrict__ hyper) {
  const int64_t t = step[0] + 1;
  step[0] = t;
  const double lr = lr0 * pow(gamma, (double)((t - 1) / step_size));
  const double b2t = pow(b2, (double)t);
  const double nmax = 2.0 / (1.0 - b2) - 1.0;
  const double nsma = nmax - 2.0 * (double)t * b2t / (1.0 - b2t);
  const bool rect = nsma >= 5.0;
  const double ss = rect ? sqrt((1.0 - b2t) * (nsma - 4.0) / (nmax - 4.0) * (nsma - 2.0) / nsma * nmax / (nmax - 2.0)) /
                               (1.0 - pow(b1, (double)t))
                         : 1.0 / (1.0 - pow(b1, (double)t));
  hyper[0] = (float)lr;
  hyper[1] = (float)(-ss * lr);
  hyper[2] = rect ? 1.f : 0.f;
  hyper[3] = (float)t;
  hyper[4] = (float)b1;
  hyper[5] = (float)(1.0 - b1);
  hyper[6] = (float)b2;
  hyper[7] = (float)(1.0 - b2);
  hyper[8] = (float)eps;
}

// one RAdam element update (radam.py:41-42, 64-71), every operation rounded on its own
struct RAdamHyper {
  float coef, val, b1, omb1, b2, omb2, eps;
  bool rect;
};
__device__ __forceinline__ RAdamHyper radam_hyper_load(const float* hyper, const float* sumsq, float max_norm) {
  RAdamHyper h;
  h.coef = 1.f;
  if (max_norm > 0.f && sumsq) {
    const float tn = sqrtf(sumsq[0]);
    h.coef = max_norm / (tn + 1e-6f);
    h.coef = h.coef < 1.f ? h.coef : 1.f;
  }
  h.val = hyper[1];
  h.rect = hyper[2] != 0.f;
  h.b1 = hyper[4]; h.omb1 = hyper[5]; h.b2 = hyper[6]; h.omb2 = hyper[7]; h.eps = hyper[8];
  return h;
}
__device__ __forceinline__ void radam_elem(float& pi, float g, float& mi, float& vi, const RAdamHyper& h) {
  const float gi = __fmul_rn(g, h.coef);
  vi = __fmul_rn(vi, h.b2);
  vi = __fadd_rn(vi, __fmul_rn(__fmul_rn(h.omb2, gi), gi));      // addcmul_(g, g, value=1-b2)
  mi = __fadd_rn(__fmul_rn(mi, h.b1), __fmul_rn(h.omb1, gi));  // mul_(b1).add_(g, alpha=1-b1)
  const float upd = h.rect ? __fdiv_rn(mi, __fadd_rn(__fsqrt_rn(vi), h.eps)) : mi;
  pi = __fadd_rn(pi, __fmul_rn(h.val, upd));
}

__global__ __launch_bounds__(256) void radam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                    const float* __restrict__ hyper, const float* __restrict__ sumsq,
                                                    float max_norm) {
  const RAdamHyper h = radam_hyper_load(hyper, sumsq, max_norm);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float pi = p[i], mi = m[i], vi = v[i];
    radam_elem(pi, g[i], mi, vi, h);
    p[i] = pi;
    m[i] = mi;
    v[i] = vi;
  }
}

// One Adam element update in torch's op order (torch.optim.Adam single-tensor,
// trainer/basic.py:63-75).  Plain operators under contract(off): every product
// and sum is rounded on its own, so the 16-B path and the scalar path agree bit
// for bit.  The pragma holds because the library is built with
// -ffp-contract=fast-honor-pragmas (plain "fast" lets the backend fuse across
// it: the packed path then carried v_pk_fma_f32 and differed by an ulp).
// Against torch's CPU Adam the bound is 1e-6 relative (its vectorised
// lerp/addcmul may fuse).
__device__ __forceinline__ void adam_elem(float& pi, float gi, float& mi, float& vi, float w, float b2, float omb2,
                                          float bc2s, float eps, float step_size) {
#pragma clang fp contract(off)
  // torch.lerp: weight < 0.5 ? m + w*(g-m) : g - (g-m)*(1-w)
  mi = (w < 0.5f) ? mi + w * (gi - mi) : gi - (gi - mi) * (1.f - w);
  vi = vi * b2;
  vi = vi + (omb2 * gi) * gi;
  const float den = __fsqrt_rn(vi) / bc2s + eps;
  pi = pi + (-step_size) * (mi / den);
}

// 16-B accesses (4 elements per thread per step, 16 loads in flight) when all
// four buffers are 16-B aligned, else one element at a time; the tail is scalar.
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                   const float* __restrict__ hyper, const float* __restrict__ sumsq,
                                                   float max_norm) {
  float coef = 1.f;
  if (max_norm > 0.f && sumsq) {
    const float tn = sqrtf(sumsq[0]);
    coef = max_norm / (tn + 1e-6f);
    coef = coef < 1.f ? coef : 1.f;
  }
  const float step_size = hyper[1], bc2s = hyper[2];
  const float w = hyper[4], b2 = hyper[5], omb2 = hyper[6], eps = hyper[7];
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  int64_t done = 0;
  if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0) {
    const int64_t n4 = n >> 2;
    for (int64_t i = tid; i < n4; i += nth) {
      f32x4_t pv = ((const f32x4_t*)p)[i], gv = ((const f32x4_t*)g)[i];
      f32x4_t mv = ((const f32x4_t*)m)[i], vv = ((const f32x4_t*)v)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pi = pv[e], mi = mv[e], vi = vv[e];
        adam_elem(pi, __fmul_rn(gv[e], coef), mi, vi, w, b2, omb2, bc2s, eps, step_size);
        pv[e] = pi;
        mv[e] = mi;
        vv[e] = vi;
      }
      ((f32x4_t*)p)[i] = pv;
      ((f32x4_t*)m)[i] = mv;
      ((f32x4_t*)v)[i] = vv;
    }
    done = n4 << 2;
  }
  for (int64_t i = done + tid; i < n; i += nth) {
    float pi = p[i], mi = m[i], vi = v[i];
    adam_elem(pi, __fmul_rn(g[i], coef), mi, vi, w, b2, omb2, bc2s, eps, step_size);
    p[i] = pi;
    m[i] = mi;
    v[i] = vi;
  }
}

// Adam with the next forward's weight-norm preparation fused in
// (vqx_adam_step_wn).  Blocks [0, row_off[n_layers]) own the rows of the
// weight-normed convs in the table: each updates its rows of v = weight_v
// and their gains weight_g[o] (adam_elem, the bits of adam_kernel), reduces
// ||v_o|| of the NEW row in the canonical order (sq4, vqx_wn_pack.h: a block
// per row for kind 0 k > 1 and kind 1, a wave per row for kind 0 k = 1),
// stores it in norm[o] and, for kind 0 (Conv1d), writes the packed
// w = g*v/||v|| through the pack's own row stores (wn_store_row_lds,
// wn_store_row4).  The remaining blocks update the flat
// segments (start, len) of everything else, 4096 elements a block.
constexpr int kAdamMaxL = 128, kAdamMaxS = 128;
struct AdamWnPlan {
  int n_layers, n_segs;
  int row_off[kAdamMaxL + 1];  // block prefix of the row layers
  int seg_blk[kAdamMaxS + 1];  // block prefix of the flat segments (after the row blocks)
};
__host__ __device__ inline int adam_wn_units(const vqx_wn_layer& l) {
  return l.kind == 1 ? l.cin : l.k > 1 ? l.cout : (l.cout + 3) / 4;
}
struct AdamHyper {
  float coef, step_size, bc2s, w, b2, omb2, eps;
};
__device__ __forceinline__ AdamHyper adam_hyper_load(const float* hyper, const float* sumsq, float max_norm) {
  AdamHyper h;
  h.coef = 1.f;
  if (max_norm > 0.f && sumsq) {
    const float tn = sqrtf(sumsq[0]);
    h.coef = max_norm / (tn + 1e-6f);
    h.coef = h.coef < 1.f ? h.coef : 1.f;
  }
  h.step_size = hyper[1];
  h.bc2s = hyper[2];
  h.w = hyper[4];
  h.b2 = hyper[5];
  h.omb2 = hyper[6];
  h.eps = hyper[7];
  return h;
}
__device__ __forceinline__ f32x4_t adam4(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                         float* __restrict__ v, int64_t i, const AdamHyper& h) {
  f32x4_t pv = *(const f32x4_t*)(p + i), gv = *(const f32x4_t*)(g + i);
  f32x4_t mv = *(const f32x4_t*)(m + i), vv = *(const f32x4_t*)(v + i);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float pi = pv[e], mi = mv[e], vi = vv[e];
    adam_elem(pi, __fmul_rn(gv[e], h.coef), mi, vi, h.w, h.b2, h.omb2, h.bc2s, h.eps, h.step_size);
    pv[e] = pi;
    mv[e] = mi;
    vv[e] = vi;
  }
  *(f32x4_t*)(p + i) = pv;
  *(f32x4_t*)(m + i) = mv;
  *(f32x4_t*)(v + i) = vv;
  return pv;
}
__device__ __forceinline__ float adam1(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                       float* __restrict__ v, int64_t i, const AdamHyper& h) {
  float pi = p[i], mi = m[i], vi = v[i];
  adam_elem(pi, __fmul_rn(g[i], h.coef), mi, vi, h.w, h.b2, h.omb2, h.bc2s, h.eps, h.step_size);
  p[i] = pi;
  m[i] = mi;
  v[i] = vi;
  return pi;
}

__global__ __launch_bounds__(256, 4) void adam_wn_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                      float* __restrict__ m, float* __restrict__ v,
                                                      const float* __restrict__ hyper,
                                                      const float* __restrict__ sumsq, float max_norm,
                                                      const vqx_wn_layer* __restrict__ L,
                                                      const int64_t* __restrict__ segs, AdamWnPlan P) {
  const AdamHyper h = adam_hyper_load(hyper, sumsq, max_norm);
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (b >= P.row_off[P.n_layers]) {  // flat segment chunk: 4096 elements
    int lo = 0, hi = P.n_segs - 1;
    const int rb = b - P.row_off[P.n_layers];
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (P.seg_blk[mid] <= rb) lo = mid; else hi = mid - 1;
    }
    const int64_t s0 = segs[2 * lo], len = segs[2 * lo + 1];
    const int64_t c0 = (int64_t)(rb - P.seg_blk[lo]) * 4096;
    if ((s0 & 3) == 0 && (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t j = c0 + (int64_t)threadIdx.x * 4 + 1024 * u;
        if (j + 4 <= len) {
          adam4(p, g, m, v, s0 + j, h);
        } else {
          for (int64_t e = j; e < len && e < j + 4; ++e) adam1(p, g, m, v, s0 + e, h);
        }
      }
    } else {
      for (int64_t j = c0 + threadIdx.x; j < len && j < c0 + 4096; j += 256) adam1(p, g, m, v, s0 + j, h);
    }
    return;
  }
  int lo = 0, hi = P.n_layers - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (P.row_off[mid] <= b) lo = mid; else hi = mid - 1;
  }
  const vqx_wn_layer& l = L[lo];
  const int unit = b - P.row_off[lo];
  const int K = l.k, cin = l.cin, cout = l.cout;
  const int64_t voff = l.v - p, goff = l.g - p;
  if (l.kind == 1 || K > 1) {
    // one row per 256-thread block: Conv1d row co (packed [co][j*cin + ci]
    // through LDS) or ConvT row ci (norm only); every load of the thread's
    // elements is issued before the first update
    __shared__ __attribute__((aligned(16))) float buf[kWnRow];
    __shared__ float red[16];
    __shared__ float gnew;
    const int o = unit;
    const int cols = l.kind == 1 ? cout * K : cin * K;
    const int64_t r0 = voff + (int64_t)o * cols;
    constexpr int U = kWnRow / 1024, UC = 2;  // UC 16-B groups' loads in flight at a time (register budget)
    float s = 0.f;
#pragma unroll
    for (int u0 = 0; u0 < U; u0 += UC) {
      f32x4_t pv[UC], gv[UC], mv[UC], vv[UC];
#pragma unroll
      for (int uu = 0; uu < UC; ++uu) {
        const int i = (int)threadIdx.x * 4 + 1024 * (u0 + uu);
        if (i < cols) {
          pv[uu] = *(const f32x4_t*)(p + r0 + i);
          gv[uu] = *(const f32x4_t*)(g + r0 + i);
          mv[uu] = *(const f32x4_t*)(m + r0 + i);
          vv[uu] = *(const f32x4_t*)(v + r0 + i);
        }
      }
#pragma unroll
      for (int uu = 0; uu < UC; ++uu) {
        const int i = (int)threadIdx.x * 4 + 1024 * (u0 + uu);
        if (i < cols) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float pi = pv[uu][e], mi = mv[uu][e], vi = vv[uu][e];
            adam_elem(pi, __fmul_rn(gv[uu][e], h.coef), mi, vi, h.w, h.b2, h.omb2, h.bc2s, h.eps, h.step_size);
            pv[uu][e] = pi;
            mv[uu][e] = mi;
            vv[uu][e] = vi;
          }
          *(f32x4_t*)(p + r0 + i) = pv[uu];
          *(f32x4_t*)(m + r0 + i) = mv[uu];
          *(f32x4_t*)(v + r0 + i) = vv[uu];
          if (l.kind == 0) *(f32x4_t*)(buf + i) = pv[uu];
          s = sq4(pv[uu], s);
        }
      }
    }
    if (threadIdx.x == 0) gnew = adam1(p, g, m, v, goff + o, h);
    s = block_sum(s, red);  // its barriers publish buf and gnew
    const float nrm = sqrtf(s);
    if (threadIdx.x == 0) l.norm[o] = nrm;
    if (l.kind == 1) return;
    wn_store_row_lds(l, o, cin, K, buf, gnew / nrm);
    return;
  }
  // a wave per row: kind 0 k = 1 (row co of cin, packed = the row scaled)
  const int o = unit * 4 + wv;
  if (o >= cout) return;
  const int cols = cin;
  const int64_t r0 = voff + (int64_t)o * cols;
  float s = 0.f;
  {
    f32x4_t xs[2], gv[2], mv[2], vv[2];  // cols <= 512
#pragma unroll
    for (int u = 0; u < 2; ++u) {  // every load first
      const int i = lane * 4 + 256 * u;
      if (i < cols) {
        xs[u] = *(const f32x4_t*)(p + r0 + i);
        gv[u] = *(const f32x4_t*)(g + r0 + i);
        mv[u] = *(const f32x4_t*)(m + r0 + i);
        vv[u] = *(const f32x4_t*)(v + r0 + i);
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = lane * 4 + 256 * u;
      if (i < cols) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float pi = xs[u][e], mi = mv[u][e], vi = vv[u][e];
          adam_elem(pi, __fmul_rn(gv[u][e], h.coef), mi, vi, h.w, h.b2, h.omb2, h.bc2s, h.eps, h.step_size);
          xs[u][e] = pi;
          mv[u][e] = mi;
          vv[u][e] = vi;
        }
        *(f32x4_t*)(p + r0 + i) = xs[u];
        *(f32x4_t*)(m + r0 + i) = mv[u];
        *(f32x4_t*)(v + r0 + i) = vv[u];
        s = sq4(xs[u], s);
      }
    }
    float gn = 0.f;
    if (lane == 0) gn = adam1(p, g, m, v, goff + o, h);
    gn = __shfl(gn, 0, 64);
    s = wave_sum(s);
    const float nrm = sqrtf(s);
    if (lane == 0) l.norm[o] = nrm;
    const float sc = gn / nrm;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = lane * 4 + 256 * u;
      if (i < cols) wn_store_row4(l, o, cols, i, xs[u], sc);
    }
  }
}

// Multi-tensor pair (vqx_multi_sq_norm, vqx_multi_adam_step): the gradients are
// separate tensors whose addresses change every step, p / m / v stay flat.  A
// launch takes up to kMultiMax tensors; their gradient pointers, flat offsets,
// lengths and the block prefix of their 4096-element chunks travel by value in
// the kernel arguments (no device table to upload, nothing to race with).
constexpr int kMultiMax = 128, kMultiChunk = 4096;
struct MultiArgs {
  int n;
  int blk[kMultiMax + 1];  // block prefix: tensor i owns blocks [blk[i], blk[i+1])
  const float* g[kMultiMax];
  int64_t off[kMultiMax];
  int64_t numel[kMultiMax];
};
static_assert(sizeof(MultiArgs) + 64 <= 4096, "MultiArgs and the other arguments must fit the 4 KB kernel-argument segment");

__device__ __forceinline__ int multi_find(const MultiArgs& A, int b) {
  int lo = 0, hi = A.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (A.blk[mid] <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// part[b] = sum g^2 over chunk b.  Thread t adds its 16 elements (4 groups of 4,
// 1024 apart) in index order whether they are loaded 16 B at a time or singly,
// so the partial does not depend on the gradient's alignment.
__global__ __launch_bounds__(256) void multi_sq_kernel(MultiArgs A, float* __restrict__ part) {
  __shared__ float red[16];
  const int b = blockIdx.x;
  const int t = multi_find(A, b);
  const float* __restrict__ g = A.g[t];
  float s = 0.f;
  if (g) {  // (uniform across the block)
    const int64_t len = A.numel[t];
    const int64_t c0 = (int64_t)(b - A.blk[t]) * kMultiChunk;
    const bool al = (((uintptr_t)g) & 15) == 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t j = c0 + (int64_t)threadIdx.x * 4 + 1024 * u;
      if (al && j + 4 <= len) {
        const f32x4_t x = *(const f32x4_t*)(g + j);
        s = fmaf(x[0], x[0], s); s = fmaf(x[1], x[1], s); s = fmaf(x[2], x[2], s); s = fmaf(x[3], x[3], s);
      } else {
        for (int64_t e = j; e < len && e < j + 4; ++e) s = fmaf(g[e], g[e], s);
      }
    }
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) part[b] = s;
}

__device__ __forceinline__ void radam1(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                       float* __restrict__ v, int64_t i, const RAdamHyper& h) {
  float pi = p[i], mi = m[i], vi = v[i];
  radam_elem(pi, g[i], mi, vi, h);
  p[i] = pi;
  m[i] = mi;
  v[i] = vi;
}
__device__ __forceinline__ void radam4(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                       float* __restrict__ v, int64_t i, const RAdamHyper& h) {
  f32x4_t pv = *(const f32x4_t*)(p + i), gv = *(const f32x4_t*)(g + i);
  f32x4_t mv = *(const f32x4_t*)(m + i), vv = *(const f32x4_t*)(v + i);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float pi = pv[e], mi = mv[e], vi = vv[e];
    radam_elem(pi, gv[e], mi, vi, h);
    pv[e] = pi;
    mv[e] = mi;
    vv[e] = vi;
  }
  *(f32x4_t*)(p + i) = pv;
  *(f32x4_t*)(m + i) = mv;
  *(f32x4_t*)(v + i) = vv;
}

// Tensor t updates p/m/v[off_t, off_t + numel_t) from its own gradient, a block
// per 4096-element chunk: 16-B accesses when p + off, m + off, v + off and the
// gradient are all 16-B aligned (decided per tensor, so uniform in a block),
// one element at a time otherwise.  KIND 0: adam_elem (the bits of
// adam_kernel); 1: radam_elem (the bits of radam_kernel).
template <int KIND>
__global__ __launch_bounds__(256) void multi_adam_kernel(float* __restrict__ p, float* __restrict__ m,
                                                         float* __restrict__ v, const float* __restrict__ hyper,
                                                         const float* __restrict__ sumsq, float max_norm,
                                                         MultiArgs A) {
  const int b = blockIdx.x;
  const int t = multi_find(A, b);
  const float* __restrict__ g = A.g[t];
  const int64_t s0 = A.off[t], len = A.numel[t];
  const int64_t c0 = (int64_t)(b - A.blk[t]) * kMultiChunk;
  float* __restrict__ pp = p + s0;
  float* __restrict__ mm = m + s0;
  float* __restrict__ vv = v + s0;
  const bool al = ((((uintptr_t)pp) | ((uintptr_t)mm) | ((uintptr_t)vv) | ((uintptr_t)g)) & 15) == 0;
  if constexpr (KIND == 0) {
    const AdamHyper h = adam_hyper_load(hyper, sumsq, max_norm);
    if (al) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t j = c0 + (int64_t)threadIdx.x * 4 + 1024 * u;
        if (j + 4 <= len) {
          adam4(pp, g, mm, vv, j, h);
        } else {
          for (int64_t e = j; e < len && e < j + 4; ++e) adam1(pp, g, mm, vv, e, h);
        }
      }
    } else {
      for (int64_t j = c0 + threadIdx.x; j < len && j < c0 + kMultiChunk; j += 256) adam1(pp, g, mm, vv, j, h);
    }
  } else {
    const RAdamHyper h = radam_hyper_load(hyper, sumsq, max_norm);
    if (al) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t j = c0 + (int64_t)threadIdx.x * 4 + 1024 * u;
        if (j + 4 <= len) {
          radam4(pp, g, mm, vv, j, h);
        } else {
          for (int64_t e = j; e < len && e < j + 4; ++e) radam1(pp, g, mm, vv, e, h);
        }
      }
    } else {
      for (int64_t j = c0 + threadIdx.x; j < len && j < c0 + kMultiChunk; j += 256) radam1(pp, g, mm, vv, j, h);
    }
  }
}

// vqx_multi_pack: flat[off_t + j] = g_t[j], a block per 4096-element chunk; a
// tensor without a gradient has its range zero-filled.  16-B loads and stores
// when the gradient and flat + off_t are both 16-B aligned (decided per tensor,
// so uniform in a block), one element at a time otherwise.
__global__ __launch_bounds__(256) void multi_pack_kernel(float* __restrict__ flat, MultiArgs A) {
  const int b = blockIdx.x;
  const int t = multi_find(A, b);
  const float* __restrict__ g = A.g[t];
  const int64_t len = A.numel[t];
  const int64_t c0 = (int64_t)(b - A.blk[t]) * kMultiChunk;
  float* __restrict__ dst = flat + A.off[t];
  const bool al = ((((uintptr_t)dst) | ((uintptr_t)g)) & 15) == 0;  // (a null gradient counts as aligned)
  if (al) {
    f32x4_t x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // every load first
      const int64_t j = c0 + (int64_t)threadIdx.x * 4 + 1024 * u;
      x[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      if (g && j + 4 <= len) x[u] = *(const f32x4_t*)(g + j);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t j = c0 + (int64_t)threadIdx.x * 4 + 1024 * u;
      if (j + 4 <= len) {
        *(f32x4_t*)(dst + j) = x[u];
      } else {
        for (int64_t e = j; e < len && e < j + 4; ++e) dst[e] = g ? g[e] : 0.f;
      }
    }
  } else {
    for (int64_t j = c0 + threadIdx.x; j < len && j < c0 + kMultiChunk; j += 256) dst[j] = g ? g[j] : 0.f;
  }
}

}  // namespace vqx

using namespace vqx;

extern "C" int vqx_sq_norm_finish(const float* partials, int64_t n_partials, const float* g, const int64_t* ranges,
                                  int32_t n_ranges, float* scratch, float* out, vqx_stream_t stream) {
  if (n_partials < 0 || n_ranges < 0 || !out || !scratch || (n_partials && !partials) || (n_ranges && (!ranges || !g))) {
    set_error("vqx_sq_norm_finish: bad arguments");
    return -1;
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sq_partial_sum_kernel, dim3(kSqBlocks), dim3(256), 0, s, partials, n_partials, g, ranges, n_ranges,
                     scratch);
  hipLaunchKernelGGL(sq_final_kernel, dim3(1), dim3(kSqBlocks), 0, s, scratch, out, AdamHyperArgs{});
  return launch_status("vqx_sq_norm_finish");
}

extern "C" int vqx_sq_norm_finish_adam(const float* partials, int64_t n_partials, const float* g,
                                       const int64_t* ranges, int32_t n_ranges, float* scratch, float* out,
                                       int64_t* step, double lr0, double gamma, int32_t step_size, double beta1,
                                       double beta2, double eps, float* hyper, vqx_stream_t stream) {
  if (n_partials < 0 || n_ranges < 0 || !out || !scratch || (n_partials && !partials) || (n_ranges && (!ranges || !g)) ||
      !step || !hyper || step_size < 1) {
    set_error("vqx_sq_norm_finish_adam: bad arguments");
    return -1;
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sq_partial_sum_kernel, dim3(kSqBlocks), dim3(256), 0, s, partials, n_partials, g, ranges, n_ranges,
                     scratch);
  hipLaunchKernelGGL(sq_final_kernel, dim3(1), dim3(kSqBlocks), 0, s, scratch, out,
                     AdamHyperArgs{step, lr0, gamma, beta1, beta2, eps, step_size, hyper});
  return launch_status("vqx_sq_norm_finish_adam");
}

extern "C" int vqx_grad_sq_norm(const float* g, int64_t n, float* partials, float* out, vqx_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(kNormBlocks), dim3(256), 0, s, g, n, partials);
  sum_partials_scale_launch(partials, kNormBlocks, 1.0f, out, s);
  return launch_status("vqx_grad_sq_norm");
}

extern "C" int vqx_adam_hyper(int64_t* step, double lr0, double gamma, int32_t step_size, double beta1,
                              double beta2, double eps, float* hyper, vqx_stream_t stream) {
  if (step_size < 1) { set_error("vqx_adam_hyper: step_size < 1"); return -1; }
  hipLaunchKernelGGL(adam_hyper_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step, lr0, gamma, step_size, beta1,
                     beta2, eps, hyper);
  return launch_status("vqx_adam_hyper");
}

extern "C" int vqx_adam_step(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper,
                             const float* sumsq, float max_norm, vqx_stream_t stream) {
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for((n + 3) / 4, 256, 4096)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n,
                     hyper, sumsq, max_norm);
  return launch_status("vqx_adam_step");
}

extern "C" int vqx_adam_step_wn(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper,
                                const float* sumsq, float max_norm, const vqx_wn_layer* rows_host,
                                const vqx_wn_layer* rows_dev, int32_t n_layers, const int64_t* segs_host,
                                const int64_t* segs_dev, int32_t n_segs, vqx_stream_t stream) {
  if (!p || !g || !m || !v || !hyper || n_layers < 0 || n_segs < 0 || n_layers > kAdamMaxL || n_segs > kAdamMaxS ||
      (n_layers && (!rows_host || !rows_dev)) || (n_segs && (!segs_host || !segs_dev))) {
    set_error("vqx_adam_step_wn: bad arguments (at most %d layers and %d segments)", kAdamMaxL, kAdamMaxS);
    return -1;
  }
  // the row path moves 16-B vectors of p, g, m, v (the segment path checks its own alignment)
  if ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) {
    set_error("vqx_adam_step_wn: p, g, m and v must be 16-B aligned");
    return -1;
  }
  AdamWnPlan P;
  P.n_layers = n_layers;
  P.n_segs = n_segs;
  P.row_off[0] = 0;
  int64_t covered = 0;
  // every interval the launch updates (v and g rows of each layer, the flat
  // segments), to check that they do not overlap (with the coverage count
  // below: exactly once each of the n elements)
  int64_t iv[2 * (2 * kAdamMaxL + kAdamMaxS)];
  int niv = 0;
  for (int i = 0; i < n_layers; ++i) {
    const vqx_wn_layer& l = rows_host[i];
    const bool k3 = l.kind == 0 && l.k > 1;
    const int cols = l.kind == 0 ? l.cin * l.k : l.cout * l.k;
    const int rows = l.kind == 0 ? l.cout : l.cin;
    const int64_t vo = l.v - p, go = l.g - p;
    const bool ok = (l.kind == 0 || l.kind == 1) && l.g && l.norm && (l.kind == 1 || l.w_packed) && l.k >= 1 &&
                    cols % 4 == 0 && cols <= (k3 || l.kind == 1 ? kWnRow : 512) && vo >= 0 && vo % 4 == 0 &&
                    vo + (int64_t)rows * cols <= n && go >= 0 && go + rows <= n &&
                    (l.dtype == VQX_BF16 || l.dtype == VQX_F32) &&
                    (l.kind == 1 || k3 ||
                     ((((uintptr_t)l.w_packed) & 15) == 0 && (l.cin * (l.dtype == VQX_BF16 ? 2 : 4)) % 16 == 0));
    if (!ok) { set_error("vqx_adam_step_wn: layer %d cannot take the fused weight-norm preparation", i); return -1; }
    P.row_off[i + 1] = P.row_off[i] + adam_wn_units(l);
    covered += (int64_t)rows * cols + rows;
    iv[2 * niv] = vo; iv[2 * niv + 1] = vo + (int64_t)rows * cols; ++niv;
    iv[2 * niv] = go; iv[2 * niv + 1] = go + rows; ++niv;
  }
  P.seg_blk[0] = 0;
  for (int i = 0; i < n_segs; ++i) {
    const int64_t s0 = segs_host[2 * i], len = segs_host[2 * i + 1];
    if (s0 < 0 || len < 0 || s0 + len > n) { set_error("vqx_adam_step_wn: segment %d out of range", i); return -1; }
    P.seg_blk[i + 1] = P.seg_blk[i] + (int)((len + 4095) / 4096);
    covered += len;
    if (len > 0) { iv[2 * niv] = s0; iv[2 * niv + 1] = s0 + len; ++niv; }
  }
  // insertion sort by start (at most 2 * 128 + 128 intervals), then adjacent overlap test
  for (int i = 1; i < niv; ++i)
    for (int j = i; j > 0 && iv[2 * j] < iv[2 * (j - 1)]; --j) {
      const int64_t a0 = iv[2 * j], a1 = iv[2 * j + 1];
      iv[2 * j] = iv[2 * (j - 1)]; iv[2 * j + 1] = iv[2 * (j - 1) + 1];
      iv[2 * (j - 1)] = a0; iv[2 * (j - 1) + 1] = a1;
    }
  for (int i = 1; i < niv; ++i)
    if (iv[2 * i] < iv[2 * (i - 1) + 1]) {
      set_error("vqx_adam_step_wn: updated ranges overlap at element %lld", (long long)iv[2 * i]);
      return -1;
    }
  if (covered != n) { set_error("vqx_adam_step_wn: rows + segments cover %lld of %lld elements", (long long)covered, (long long)n); return -1; }
  const int grid = P.row_off[n_layers] + P.seg_blk[n_segs];
  if (grid > 0)
    hipLaunchKernelGGL(adam_wn_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, hyper, sumsq,
                       max_norm, rows_dev, segs_dev, P);
  return launch_status("vqx_adam_step_wn");
}

extern "C" int vqx_radam_hyper(int64_t* step, double lr0, double gamma, int32_t step_size, double beta1,
                               double beta2, double eps, float* hyper, vqx_stream_t stream) {
  if (step_size < 1) { set_error("vqx_radam_hyper: step_size < 1"); return -1; }
  if (!(beta2 > 0.0 && beta2 < 1.0) || !step || !hyper) { set_error("vqx_radam_hyper: bad arguments"); return -1; }
  hipLaunchKernelGGL(radam_hyper_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step, lr0, gamma, step_size, beta1,
                     beta2, eps, hyper);
  return launch_status("vqx_radam_hyper");
}

extern "C" int vqx_radam_step(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper,
                              const float* sumsq, float max_norm, vqx_stream_t stream) {
  if (n <= 0) return 0;
  if (!p || !g || !m || !v || !hyper) { set_error("vqx_radam_step: null pointer"); return -1; }
  hipLaunchKernelGGL(radam_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n,
                     hyper, sumsq, max_norm);
  return launch_status("vqx_radam_step");
}

extern "C" int vqx_multi_chunks(const int64_t* numel, int32_t n, int64_t* out) {
  if (n < 0 || (n && !numel) || !out) { set_error("vqx_multi_chunks: bad arguments"); return -1; }
  int64_t c = 0;
  for (int i = 0; i < n; ++i) {
    if (numel[i] < 0) { set_error("vqx_multi_chunks: tensor %d has a negative length", i); return -1; }
    c += (numel[i] + kMultiChunk - 1) / kMultiChunk;
  }
  *out = c;
  return 0;
}

extern "C" int vqx_multi_sq_norm(const float* const* grads, const int64_t* numel, int32_t n, float* partials,
                                 int64_t n_partials, vqx_stream_t stream) {
  if (n < 0 || (n && (!grads || !numel)) || n_partials < 0 || (n_partials && !partials)) {
    set_error("vqx_multi_sq_norm: bad arguments");
    return -1;
  }
  int64_t total = 0;
  for (int i = 0; i < n; ++i) {
    if (numel[i] < 0 || numel[i] > ((int64_t)1 << 40) || (((uintptr_t)grads[i]) & 3)) {
      set_error("vqx_multi_sq_norm: tensor %d: bad length or a gradient that is not 4-B aligned", i);
      return -1;
    }
    total += (numel[i] + kMultiChunk - 1) / kMultiChunk;
  }
  if (total != n_partials) {
    set_error("vqx_multi_sq_norm: %lld chunks for %lld partials", (long long)total, (long long)n_partials);
    return -1;
  }
  int64_t base = 0;
  for (int i0 = 0; i0 < n; i0 += kMultiMax) {
    MultiArgs A;
    A.n = 0;
    A.blk[0] = 0;
    for (int i = i0; i < n && i < i0 + kMultiMax; ++i) {
      const int64_t ch = (numel[i] + kMultiChunk - 1) / kMultiChunk;
      if (ch == 0) continue;
      if ((int64_t)A.blk[A.n] + ch > 0x7fffffff) { set_error("vqx_multi_sq_norm: too many chunks in one launch"); return -1; }
      A.g[A.n] = grads[i];
      A.off[A.n] = 0;
      A.numel[A.n] = numel[i];
      A.blk[A.n + 1] = A.blk[A.n] + (int)ch;
      ++A.n;
    }
    if (A.n == 0) continue;
    hipLaunchKernelGGL(multi_sq_kernel, dim3(A.blk[A.n]), dim3(256), 0, (hipStream_t)stream, A, partials + base);
    base += A.blk[A.n];
  }
  return launch_status("vqx_multi_sq_norm");
}

extern "C" int vqx_multi_adam_step(float* p, float* m, float* v, int64_t n_flat, const int64_t* offset,
                                   const int64_t* numel, const float* const* grads, int32_t n, const float* hyper,
                                   const float* sumsq, float max_norm, int32_t kind, vqx_stream_t stream) {
  if (!p || !m || !v || !hyper || n < 0 || n_flat < 0 || (n && (!offset || !numel || !grads)) ||
      (kind != 0 && kind != 1)) {
    set_error("vqx_multi_adam_step: bad arguments (kind 0 Adam, 1 RAdam)");
    return -1;
  }
  if ((((uintptr_t)p) | ((uintptr_t)m) | ((uintptr_t)v)) & 3) {
    set_error("vqx_multi_adam_step: p, m and v must be 4-B aligned");
    return -1;
  }
  int64_t end = 0;
  for (int i = 0; i < n; ++i) {  // ranges in order, inside [0, n_flat), not overlapping
    if (numel[i] < 0 || offset[i] < end || numel[i] > n_flat || offset[i] > n_flat - numel[i] ||
        (((uintptr_t)grads[i]) & 3)) {
      set_error("vqx_multi_adam_step: tensor %d: range out of order or out of [0, %lld), or a gradient that is "
                "not 4-B aligned", i, (long long)n_flat);
      return -1;
    }
    end = offset[i] + numel[i];
  }
  for (int i0 = 0; i0 < n; i0 += kMultiMax) {
    MultiArgs A;
    A.n = 0;
    A.blk[0] = 0;
    for (int i = i0; i < n && i < i0 + kMultiMax; ++i) {
      const int64_t ch = (numel[i] + kMultiChunk - 1) / kMultiChunk;
      if (ch == 0 || !grads[i]) continue;  // no gradient: p, m and v stay as they are
      if ((int64_t)A.blk[A.n] + ch > 0x7fffffff) { set_error("vqx_multi_adam_step: too many chunks in one launch"); return -1; }
      A.g[A.n] = grads[i];
      A.off[A.n] = offset[i];
      A.numel[A.n] = numel[i];
      A.blk[A.n + 1] = A.blk[A.n] + (int)ch;
      ++A.n;
    }
    if (A.n == 0) continue;
    if (kind == 0)
      hipLaunchKernelGGL(multi_adam_kernel<0>, dim3(A.blk[A.n]), dim3(256), 0, (hipStream_t)stream, p, m, v, hyper,
                         sumsq, max_norm, A);
    else
      hipLaunchKernelGGL(multi_adam_kernel<1>, dim3(A.blk[A.n]), dim3(256), 0, (hipStream_t)stream, p, m, v, hyper,
                         sumsq, max_norm, A);
  }
  return launch_status("vqx_multi_adam_step");
}

extern "C" int vqx_multi_pack(float* flat, int64_t n_flat, const int64_t* offset, const int64_t* numel,
                              const float* const* grads, int32_t n, vqx_stream_t stream) {
  if (!flat || n < 0 || n_flat < 0 || (n && (!offset || !numel || !grads))) {
    set_error("vqx_multi_pack: bad arguments");
    return -1;
  }
  if (((uintptr_t)flat) & 3) {
    set_error("vqx_multi_pack: flat must be 4-B aligned");
    return -1;
  }
  int64_t end = 0;
  for (int i = 0; i < n; ++i) {  // ranges in order, inside [0, n_flat), not overlapping
    if (numel[i] < 0) { set_error("vqx_multi_pack: tensor %d has a negative length", i); return -1; }
    if (offset[i] < end || numel[i] > n_flat || offset[i] > n_flat - numel[i]) {
      set_error("vqx_multi_pack: tensor %d: range out of order or out of [0, %lld)", i, (long long)n_flat);
      return -1;
    }
    if (((uintptr_t)grads[i]) & 3) {
      set_error("vqx_multi_pack: tensor %d: a gradient that is not 4-B aligned", i);
      return -1;
    }
    end = offset[i] + numel[i];
  }
  for (int i0 = 0; i0 < n; i0 += kMultiMax) {
    MultiArgs A;
    A.n = 0;
    A.blk[0] = 0;
    for (int i = i0; i < n && i < i0 + kMultiMax; ++i) {
      const int64_t ch = (numel[i] + kMultiChunk - 1) / kMultiChunk;
      if (ch == 0) continue;
      if ((int64_t)A.blk[A.n] + ch > 0x7fffffff) { set_error("vqx_multi_pack: too many chunks in one launch"); return -1; }
      A.g[A.n] = grads[i];  // null: the range is zero-filled
      A.off[A.n] = offset[i];
      A.numel[A.n] = numel[i];
      A.blk[A.n + 1] = A.blk[A.n] + (int)ch;
      ++A.n;
    }
    if (A.n == 0) continue;
    hipLaunchKernelGGL(multi_pack_kernel, dim3(A.blk[A.n]), dim3(256), 0, (hipStream_t)stream, flat, A);
  }
  return launch_status("vqx_multi_pack");
}
