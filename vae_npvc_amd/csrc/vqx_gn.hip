// GroupNorm with its gated unit (GLU) and LeakyReLU, forward and backward
// (gfx950).
#include "vqx_common.h"
#include "vqx_gn_math.h"
#include "vqx_vec.h"
#include <math.h>

#include <algorithm>

namespace vqx {

// Partial moments per (b, g, part): two-pass within the part (mean, then
// centred sum of squares), combined with Chan's formula in finalize.
constexpr int kGnParts = 8;
constexpr int kGnBwdParts = 32;  // row parts of the GroupNorm-backward reduction

template <typename T>
__global__ __launch_bounds__(256) void gn_partial_kernel(const T* __restrict__ x, int ldx, int T_, int C, int G,
                                                         float* __restrict__ part) {
  const int p = blockIdx.x, bg = blockIdx.y;
  const int b = bg / G, g = bg - b * G;
  const int cg = C / G;
  const int r0 = p * T_ / kGnParts, r1 = (p + 1) * T_ / kGnParts;
  const int64_t nrows = r1 - r0;
  const int64_t cnt = nrows * cg;
  __shared__ float red[16];
  const T* base = x + ((int64_t)b * T_ + r0) * ldx + g * cg;
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < cnt; i += blockDim.x) {
    const int64_t rr = i / cg, cc = i - rr * cg;
    s += Elem<T>::ld(base, rr * ldx + cc);
  }
  s = block_sum(s, red);
  const float mean = cnt ? s / (float)cnt : 0.f;
  float m2 = 0.f;
  for (int64_t i = threadIdx.x; i < cnt; i += blockDim.x) {
    const int64_t rr = i / cg, cc = i - rr * cg;
    const float d = Elem<T>::ld(base, rr * ldx + cc) - mean;
    m2 = fmaf(d, d, m2);
  }
  m2 = block_sum(m2, red);
  if (threadIdx.x == 0) {
    float* o = part + ((int64_t)bg * kGnParts + p) * 3;
    o[0] = (float)cnt;
    o[1] = mean;
    o[2] = m2;
  }
}

__global__ void gn_finalize_kernel(const float* __restrict__ part, int nbg, float eps, float* __restrict__ mr) {
  const int bg = blockIdx.x * blockDim.x + threadIdx.x;
  if (bg >= nbg) return;
  double n = 0.0, mean = 0.0, m2 = 0.0;
  for (int p = 0; p < kGnParts; ++p) {
    const float* o = part + ((int64_t)bg * kGnParts + p) * 3;
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

// Combine the GEMM GNSTATS tiles [N/128][ntn][4] = (count, mean, M2, -) of
// utterance b's row groups and group g's column tiles (double, fixed order).
__global__ void gn_finalize_tiles_kernel(const float* __restrict__ part, int B, int G, int rg_per_utt, int ntn,
                                         int tn_per_group, float eps, float* __restrict__ mr) {
  const int bg = blockIdx.x * blockDim.x + threadIdx.x;
  if (bg >= B * G) return;
  const int b = bg / G, g = bg - b * G;
  double n = 0.0, mean = 0.0, m2 = 0.0;
  for (int r = 0; r < rg_per_utt; ++r)
    for (int t = 0; t < tn_per_group; ++t) {
      const float* o = part + ((int64_t)(b * rg_per_utt + r) * ntn + g * tn_per_group + t) * 4;
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

// GroupNorm partial moments, vectorised: block (part p, utterance-group bg);
// thread = (chunk of the group's columns, row group).  Requires the group's
// chunk count cpr to divide 256.
template <typename T>
__global__ __launch_bounds__(256) void gn_partial_vec_kernel(const T* __restrict__ x, int ldx, int T_, int C, int G,
                                                             int cpr, float* __restrict__ part) {
  constexpr int V = Vec<T>::N;
  const int p = blockIdx.x, bg = blockIdx.y;
  const int b = bg / G, g = bg - b * G;
  const int cg = C / G;
  const int r0 = p * T_ / kGnParts, r1 = (p + 1) * T_ / kGnParts;
  const int ch = threadIdx.x % cpr, rg = threadIdx.x / cpr, nrg = 256 / cpr;
  __shared__ float red[16];
  const T* base = x + ((int64_t)b * T_) * ldx + g * cg + ch * V;
  float s = 0.f;
  for (int r = r0 + rg; r < r1; r += nrg) {
    float f[V];
    Vec<T>::load(base + (int64_t)r * ldx, f);
#pragma unroll
    for (int i = 0; i < V; ++i) s += f[i];
  }
  s = block_sum(s, red);
  const int64_t cnt = (int64_t)(r1 - r0) * cg;
  const float mean = cnt ? s / (float)cnt : 0.f;
  float m2 = 0.f;
  for (int r = r0 + rg; r < r1; r += nrg) {
    float f[V];
    Vec<T>::load(base + (int64_t)r * ldx, f);
#pragma unroll
    for (int i = 0; i < V; ++i) { const float d = f[i] - mean; m2 = fmaf(d, d, m2); }
  }
  m2 = block_sum(m2, red);
  if (threadIdx.x == 0) {
    float* o = part + ((int64_t)bg * kGnParts + p) * 3;
    o[0] = (float)cnt;
    o[1] = mean;
    o[2] = m2;
  }
}

// Gradient w.r.t. the GroupNorm output h for a chunk of V channels.
//   glu: channels [c, c+V) of the tanh half AND [c+half, c+half+V) of the
//        sigmoid half (dy = dL/dg has `half` columns);
//   else: channels [c, c+V) (dy = dL/dh), single group set by the caller.
template <typename T>
__device__ __forceinline__ void gn_dh_chunk(const T* dy, int lddy, const T* u, int ldu, int64_t n, int c, int half,
                                            bool glu, const float* mr4, const float* gamma, const float* beta,
                                            float* dha, float* xa, float* dhb, float* xb) {
  constexpr int V = Vec<T>::N;
  float g[V], ua[V];
  Vec<T>::load(dy + n * lddy + c, g);
  Vec<T>::load(u + n * ldu + c, ua);
  if (!glu) {
#pragma unroll
    for (int i = 0; i < V; ++i) { dha[i] = g[i]; xa[i] = (ua[i] - mr4[0]) * mr4[1]; }
    return;
  }
  float ub[V];
  Vec<T>::load(u + n * ldu + c + half, ub);
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const float xha = (ua[i] - mr4[0]) * mr4[1];
    const float xhb = (ub[i] - mr4[2]) * mr4[3];
    const float ha = xha * gamma[c + i] + beta[c + i];
    const float hb = xhb * gamma[c + half + i] + beta[c + half + i];
    const float ta = ftanh<sizeof(T) == 2>(ha);
    const float sb = fsigmoid<sizeof(T) == 2>(hb);
    dha[i] = g[i] * sb * (1.f - ta * ta);
    dhb[i] = g[i] * ta * (sb * (1.f - sb));
    xa[i] = xha;
    xb[i] = xhb;
  }
}

// pass 1 (vectorised): per (utterance, part) S1_g = sum gamma*dh, S2_g = sum gamma*dh*xhat
template <typename T>
__global__ __launch_bounds__(256) void gn_bwd_reduce_vec_kernel(const T* __restrict__ dy, int lddy,
                                                                const T* __restrict__ u, int ldu, int T_, int C, int G,
                                                                int glu, int cpr, const float* __restrict__ mr,
                                                                const float* __restrict__ gamma,
                                                                const float* __restrict__ beta,
                                                                float* __restrict__ part) {
  constexpr int V = Vec<T>::N;
  const int p = blockIdx.x, b = blockIdx.y;
  const int r0 = p * T_ / kGnBwdParts, r1 = (p + 1) * T_ / kGnBwdParts;
  const int ch = threadIdx.x % cpr, rg = threadIdx.x / cpr, nrg = 256 / cpr;
  const int half = C / 2;
  const int c = ch * V;
  const float* mr4 = mr + (int64_t)b * G * 2;
  __shared__ float red[16];
  float s1a = 0.f, s2a = 0.f, s1b = 0.f, s2b = 0.f;
  for (int r = r0 + rg; r < r1; r += nrg) {
    const int64_t n = (int64_t)b * T_ + r;
    float dha[V], xa[V], dhb[V], xb[V];
    gn_dh_chunk<T>(dy, lddy, u, ldu, n, c, half, glu, mr4, gamma, beta, dha, xa, dhb, xb);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float ga = gamma[c + i] * dha[i];
      s1a += ga;
      s2a = fmaf(ga, xa[i], s2a);
      if (glu) {
        const float gb = gamma[c + half + i] * dhb[i];
        s1b += gb;
        s2b = fmaf(gb, xb[i], s2b);
      }
    }
  }
  s1a = block_sum(s1a, red);
  __syncthreads();
  s2a = block_sum(s2a, red);
  __syncthreads();
  if (glu) {
    s1b = block_sum(s1b, red);
    __syncthreads();
    s2b = block_sum(s2b, red);
  }
  if (threadIdx.x == 0) {
    float* o = part + ((int64_t)b * kGnBwdParts + p) * G * 2;
    o[0] = s1a;
    o[1] = s2a;
    if (glu) { o[2] = s1b; o[3] = s2b; }
  }
}

// pass 2 (vectorised): du and per-(utterance, channel) sums of du (bias /
// conv_cond gradients), dh*xhat (dgamma) and dh (dbeta).  Block = one
// utterance x 64 channels x all T rows, so the per-utterance sums are complete
// inside the block (deterministic, no atomics).  A thread owns 4 channels
// (8-B bf16 / 16-B fp32 accesses; 16 lanes cover a 64-channel row segment)
// in one of 32 row groups and loads two rows before the math of either: the
// kernel is bound by the loads in flight per CU, and 4 channels a thread keep
// it at ~100 VGPRs (8 channels: 176, two waves per SIMD).
#ifndef VQX_GN_NR  // rows in flight per thread in gn_bwd_apply_vec_kernel
#define VQX_GN_NR 2
#endif
constexpr int kGnApplyRG = 32, kGnApplyW = 4, kGnApplyNR = VQX_GN_NR;

template <typename T, bool GLU>
__global__ __launch_bounds__(512) void gn_bwd_apply_vec_kernel(const T* __restrict__ dy, int lddy,
                                                               const T* __restrict__ u, int ldu, T* __restrict__ du,
                                                               int lddu, int T_, int C, int G, int, int cpr,
                                                               const float* __restrict__ mr,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ beta,
                                                               const float* __restrict__ part, int nparts,
                                                               int pstride, float* __restrict__ colsum_b,
                                                               float* __restrict__ dgamma_b, float* __restrict__ dbeta_b) {
  constexpr bool glu = GLU;
  constexpr int W = kGnApplyW, RG = kGnApplyRG;
  const int cpw = cpr * (Vec<T>::N / W);  // W-channel chunks per half row
  const int b = blockIdx.y;
  const int ch = blockIdx.x * 16 + (threadIdx.x & 15), rg = threadIdx.x >> 4;
  const bool active = ch < cpw;
  const int half = C / 2;
  const int c = ch * W;
  const float* mr4 = mr + (int64_t)b * G * 2;
  const int ng = glu ? 2 : 1;
  const int lane = threadIdx.x & 63;
  // The utterance's partials, one part per lane (nparts <= 64), loaded first,
  // then gamma / beta and the first two rows as raw chunks; every wave then
  // sums the partials in part order through shuffles (no LDS, no barrier), so
  // the sum waits on the partial loads only and runs under the rows' flight.
  // (The LDS-staged sum ran before any row load was issued.)
  const bool shfl_sum = nparts <= 64;
  float q0 = 0.f, q1 = 0.f, q2 = 0.f, q3 = 0.f;
  if (shfl_sum && lane < nparts) {
    const float* o = part + ((int64_t)b * nparts + lane) * pstride;
    q0 = o[0];
    q1 = o[1];
    if (glu) { q2 = o[2]; q3 = o[3]; }
  }
  float ga[W], ba[W], gb[W], bb[W];
  const int cc = active ? c : 0;  // inactive lanes load chunk 0 and discard it (no branch to join)
#pragma unroll
  for (int i = 0; i < W; ++i) {
    ga[i] = gamma[cc + i];
    ba[i] = beta[cc + i];
    gb[i] = glu ? gamma[cc + half + i] : 0.f;
    bb[i] = glu ? beta[cc + half + i] : 0.f;
  }
  // the first NR rows as raw chunks (rows clamped into the utterance), converted after the sums
  typedef typename Vec4<T>::raw_t raw_t;
  constexpr int NR = kGnApplyNR;
  const int64_t nb0 = (int64_t)b * T_;
  raw_t pg[NR], pa[NR], pb[NR];
  auto load_rows = [&](int r) {
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      const int64_t nc = nb0 + min(r + k * RG, T_ - 1);
      pg[k] = Vec4<T>::ld(dy + nc * lddy + cc);
      pa[k] = Vec4<T>::ld(u + nc * ldu + cc);
      pb[k] = glu ? Vec4<T>::ld(u + nc * ldu + cc + half) : raw_t{};
    }
  };
  load_rows(rg);
  float m1a = 0.f, m2a = 0.f, m1b = 0.f, m2b = 0.f;
  {
    const int cg = C / G;
    const float M = (float)T_ * (float)cg;
    float S1a = 0.f, S2a = 0.f, S1b = 0.f, S2b = 0.f;
    // two loops: a global load inside the shuffle loop would make every
    // iteration wait on all loads in flight
    if (shfl_sum) {
      for (int q = 0; q < nparts; ++q) {
        S1a += __shfl(q0, q, 64);
        S2a += __shfl(q1, q, 64);
        if (glu) { S1b += __shfl(q2, q, 64); S2b += __shfl(q3, q, 64); }
      }
    } else {
      for (int q = 0; q < nparts; ++q) {
        const float* o = part + ((int64_t)b * nparts + q) * pstride;
        S1a += o[0];
        S2a += o[1];
        if (glu) { S1b += o[2]; S2b += o[3]; }
      }
    }
    m1a = S1a / M; m2a = S2a / M; m1b = S1b / M; m2b = S2b / M;
  }
  float a_du[2][W], a_dg[2][W], a_db[2][W];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int i = 0; i < W; ++i) { a_du[s][i] = 0.f; a_dg[s][i] = 0.f; a_db[s][i] = 0.f; }
  auto row = [&](int64_t n, const float* g, const float* ua, const float* ub) {
    float dha[W], xa[W], dhb[W], xb[W], oa[W];
    gn_row_math<T, W>(g, ua, ub, glu, mr4, ga, ba, gb, bb, dha, xa, dhb, xb);
    gn_dx<W>(dha, xa, ga, mr4[1], m1a, m2a, oa);
#pragma unroll
    for (int i = 0; i < W; ++i) {
      a_du[0][i] += oa[i];
      a_dg[0][i] = fmaf(dha[i], xa[i], a_dg[0][i]);
      a_db[0][i] += dha[i];
    }
    Vec4<T>::store(du + n * lddu + c, oa);
    if (glu) {
      float ob[W];
      gn_dx<W>(dhb, xb, gb, mr4[3], m1b, m2b, ob);
#pragma unroll
      for (int i = 0; i < W; ++i) {
        a_du[1][i] += ob[i];
        a_dg[1][i] = fmaf(dhb[i], xb[i], a_dg[1][i]);
        a_db[1][i] += dhb[i];
      }
      Vec4<T>::store(du + n * lddu + c + half, ob);
    }
  };
  if (active) {
    // NR rows in flight, processed in row order (the column sums' order does
    // not depend on NR)
    for (int r = rg; r < T_; r += NR * RG) {
      if (r != rg) load_rows(r);
#pragma unroll
      for (int k = 0; k < NR; ++k) {
        if (r + k * RG < T_) {
          float g0[W], ua0[W], ub0[W];
          Vec4<T>::cvt(pg[k], g0);
          Vec4<T>::cvt(pa[k], ua0);
          if (glu) Vec4<T>::cvt(pb[k], ub0);
          row(nb0 + r + k * RG, g0, ua0, ub0);
        }
      }
    }
  }
  __shared__ float lds[RG][16][2 * W];
  auto dump = [&](const float (&a)[2][W], float* out) {
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < W; ++i) lds[rg][threadIdx.x & 15][s * W + i] = a[s][i];
    __syncthreads();
    // 128 threads finish 16 chunks x 2 halves x W columns
    for (int e = threadIdx.x; e < 16 * 2 * W; e += 512) {
      const int cl = e / (2 * W), rem = e - cl * 2 * W, s = rem / W, i = rem - s * W;
      const int chg = blockIdx.x * 16 + cl;
      if (chg >= cpw || s >= ng || !out) continue;
      float t = 0.f;
#pragma unroll
      for (int q = 0; q < RG; ++q) t += lds[q][cl][rem];
      out[(int64_t)b * C + chg * W + s * half + i] = t;
    }
  };
  dump(a_du, colsum_b);
  dump(a_dg, dgamma_b);
  dump(a_db, dbeta_b);
}

// g = tanh(GN(u)[:, :half]) * sigmoid(GN(u)[:, half:]), GroupNorm with G=2,
// one 16-B chunk of V channels per thread (layers.py:236-242).
template <typename T>
__global__ __launch_bounds__(256) void gn_glu_fwd_vec_kernel(const T* __restrict__ u, int ldu, T* __restrict__ g,
                                                             int ldg, int n_rows, int T_, int half, int cpr,
                                                             const float* __restrict__ mr,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta,
                                                             const float* __restrict__ tiles, float eps,
                                                             float* __restrict__ mr_out, int fpb) {
  // block = fpb frames; thread = (chunk, row slot); cpr divides 256
  constexpr int V = Vec<T>::N;
  const int ch = threadIdx.x % cpr, rs = threadIdx.x / cpr, nrs = 256 / cpr;
  const int c = ch * V;
  const int lane = threadIdx.x & 63;
  // In-launch statistics (tiles != null): this block's utterance (T % fpb == 0:
  // the fpb frames share one) merged from the producing GEMM's GNSTATS tiles,
  // as gn_finalize_tiles_kernel does, by wave 0: lane k loads tile k (group
  // k / nt), then the tiles are merged in order through shuffles, lane parity
  // choosing the group, in double, and lanes 0 / 1 leave the result in LDS
  // for the barrier.  The tile loads go out first, then gamma / beta and the
  // first rows as raw chunks: the merge waits on the tile loads only (vmcnt
  // counts in issue order) and the barrier (an LDS wait on gfx950) on the
  // merge, with the rows in flight.  (Round 5: with the rows loaded after the
  // barrier, as program order had them, the merge cost 2.6 us of a 13.2 us
  // launch against the precomputed-statistics path; loads converted as they
  // are issued would wait right there.  The merge in every wave, without the
  // barrier, cost as much in f64 issue as it saved.)
  const int b0 = blockIdx.x * fpb / T_, rg = T_ / 128, ntn = 2 * half / 128, tpg = ntn / 2, nt = rg * tpg;
  const bool shfl_merge = 2 * nt <= 64;  // every tile in one lane
  float tl0 = 0.f, tl1 = 0.f, tl2 = 0.f;
  if (tiles && shfl_merge && (int)threadIdx.x < 2 * nt) {
    const int gi = lane / nt, k = lane - gi * nt, r = k / tpg, t = k - r * tpg;
    const float* o = tiles + ((int64_t)(b0 * rg + r) * ntn + gi * tpg + t) * 4;
    tl0 = o[0];
    tl1 = o[1];
    tl2 = o[2];
  }
  float ga[V], ba[V], gb[V], bb[V];
#pragma unroll
  for (int i = 0; i < V; ++i) { ga[i] = gamma[c + i]; ba[i] = beta[c + i]; gb[i] = gamma[c + half + i]; bb[i] = beta[c + half + i]; }
  // two rows' loads in flight before the math of either; the first pair's
  // raw chunks are converted after the merge, so it does not wait on them
  typedef typename Vec<T>::raw_t raw_t;
  const int rend = min(n_rows, blockIdx.x * fpb + fpb);
  int r = blockIdx.x * fpb + rs;
  const bool pair = r + nrs < rend, one = r < rend;
  // clamped rows (every block holds at least one): the loads need no branch,
  // whose join would wait on them
  const int r0c = one ? r : rend - 1, r1c = pair ? r + nrs : r0c;
  const raw_t qa0 = Vec<T>::ld(u + (int64_t)r0c * ldu + c), qb0 = Vec<T>::ld(u + (int64_t)r0c * ldu + c + half);
  const raw_t qa1 = Vec<T>::ld(u + (int64_t)r1c * ldu + c), qb1 = Vec<T>::ld(u + (int64_t)r1c * ldu + c + half);
  float s_ma = 0.f, s_ra = 0.f, s_mb = 0.f, s_rb = 0.f;  // mean / rstd of groups a and b (tiles path)
  __shared__ float smr[4];
  if (tiles && threadIdx.x < 64) {
    const int gi = lane & 1;
    double n = 0.0, mean = 0.0, m2 = 0.0;
    auto merge = [&](float o0, float o1, float o2) {
      const double nb = o0;
      if (nb == 0.0) return;
      const double d = (double)o1 - mean;
      const double nn = n + nb;
      mean += d * nb / nn;
      m2 += (double)o2 + d * d * n * nb / nn;
      n = nn;
    };
    // two loops: a global load inside the shuffle loop would make every
    // iteration wait on all loads in flight
    if (shfl_merge) {
      for (int k = 0; k < nt; ++k) {
        const int src = gi * nt + k;
        merge(__shfl(tl0, src, 64), __shfl(tl1, src, 64), __shfl(tl2, src, 64));
      }
    } else {
      for (int rr = 0; rr < rg; ++rr)
        for (int t = 0; t < tpg; ++t) {
          const float* o = tiles + ((int64_t)(b0 * rg + rr) * ntn + gi * tpg + t) * 4;
          merge(o[0], o[1], o[2]);
        }
    }
    const float var = n > 0.0 ? (float)(m2 / n) : 0.f;
    const float mf = (float)mean, rf = 1.0f / sqrtf(var + eps);
    if (threadIdx.x < 2) {
      smr[2 * gi] = mf;
      smr[2 * gi + 1] = rf;
      if ((blockIdx.x * fpb) % T_ == 0) {  // the utterance's first block stores them
        mr_out[4 * b0 + 2 * gi] = mf;
        mr_out[4 * b0 + 2 * gi + 1] = rf;
      }
    }
  }
  if (tiles) {
    __syncthreads();  // (waits on LDS only: the rows' loads stay in flight)
    s_ma = smr[0];
    s_ra = smr[1];
    s_mb = smr[2];
    s_rb = smr[3];
  }
  auto row = [&](int r, const float* ua, const float* ub) {
    const int b = r / T_;
    float ma, ra, mb, rb;
    if (tiles) { ma = s_ma; ra = s_ra; mb = s_mb; rb = s_rb; }
    else { ma = mr[4 * b + 0]; ra = mr[4 * b + 1]; mb = mr[4 * b + 2]; rb = mr[4 * b + 3]; }
    float o[V];
#pragma unroll
    for (int i = 0; i < V; ++i)
      o[i] = ftanh<sizeof(T) == 2>((ua[i] - ma) * ra * ga[i] + ba[i]) *
             fsigmoid<sizeof(T) == 2>((ub[i] - mb) * rb * gb[i] + bb[i]);
    Vec<T>::store(g + (int64_t)r * ldg + c, o);
  };
  if (!one) return;
  float ua0[V], ub0[V], ua1[V], ub1[V];
  Vec<T>::cvt(qa0, ua0);
  Vec<T>::cvt(qb0, ub0);
  row(r, ua0, ub0);
  if (!pair) return;
  Vec<T>::cvt(qa1, ua1);
  Vec<T>::cvt(qb1, ub1);
  row(r + nrs, ua1, ub1);
  for (r += 2 * nrs; r + nrs < rend; r += 2 * nrs) {
    Vec<T>::load(u + (int64_t)r * ldu + c, ua0);
    Vec<T>::load(u + (int64_t)r * ldu + c + half, ub0);
    Vec<T>::load(u + (int64_t)(r + nrs) * ldu + c, ua1);
    Vec<T>::load(u + (int64_t)(r + nrs) * ldu + c + half, ub1);
    row(r, ua0, ub0);
    row(r + nrs, ua1, ub1);
  }
  if (r < rend) {
    Vec<T>::load(u + (int64_t)r * ldu + c, ua0);
    Vec<T>::load(u + (int64_t)r * ldu + c + half, ub0);
    row(r, ua0, ub0);
  }
}

// g = LeakyReLU_0.2(GroupNorm_{G=1}(h)): the LeakyReLU heading each further
// conv of a residual stack with stack_layers > 1 (layers.py:156-161), one
// 16-B chunk of V channels per thread.
template <typename T>
__global__ __launch_bounds__(256) void gn_lrelu_fwd_kernel(const T* __restrict__ h, int ldh, T* __restrict__ g, int ldg,
                                                           int64_t n_rows, int T_, int cpr,
                                                           const float* __restrict__ mr,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ beta) {
  constexpr int V = Vec<T>::N;
  const int64_t total = n_rows * cpr;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / cpr;
    const int c = (int)(i - r * cpr) * V;
    const int b = (int)(r / T_);
    const float m = mr[2 * b], rs = mr[2 * b + 1];
    float x[V];
    Vec<T>::load(h + r * ldh + c, x);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float v = (x[k] - m) * rs * gamma[c + k] + beta[c + k];
      x[k] = v > 0.f ? v : 0.2f * v;
    }
    Vec<T>::store(g + r * ldg + c, x);
  }
}

}  // namespace vqx

using namespace vqx;

extern "C" int vqx_groupnorm_stats(const void* x, int32_t ldx, int32_t dtype, int64_t n_rows, int32_t T, int32_t C,
                                   int32_t G, float eps, float* partials, float* mean_rstd, vqx_stream_t stream) {
  if (G < 1 || C % G || n_rows % T) { set_error("vqx_groupnorm_stats: bad shape"); return -1; }
  const int B = (int)(n_rows / T);
  hipStream_t s = (hipStream_t)stream;
  const int V = dtype == VQX_BF16 ? 8 : 4;
  const int cg = C / G, cpr = cg / V;
  const bool vec = (cg % V == 0) && (ldx % V == 0) && cpr <= 256 && (256 % cpr == 0) && (((uintptr_t)x & 15) == 0);
  if (dtype == VQX_BF16) {
    if (vec) hipLaunchKernelGGL(gn_partial_vec_kernel<bf16_t>, dim3(kGnParts, B * G), dim3(256), 0, s, (const bf16_t*)x, ldx, T, C, G, cpr, partials);
    else hipLaunchKernelGGL(gn_partial_kernel<bf16_t>, dim3(kGnParts, B * G), dim3(256), 0, s, (const bf16_t*)x, ldx, T, C, G, partials);
  } else {
    if (vec) hipLaunchKernelGGL(gn_partial_vec_kernel<float>, dim3(kGnParts, B * G), dim3(256), 0, s, (const float*)x, ldx, T, C, G, cpr, partials);
    else hipLaunchKernelGGL(gn_partial_kernel<float>, dim3(kGnParts, B * G), dim3(256), 0, s, (const float*)x, ldx, T, C, G, partials);
  }
  hipLaunchKernelGGL(gn_finalize_kernel, dim3((B * G + 127) / 128), dim3(128), 0, s, partials, B * G, eps, mean_rstd);
  return launch_status("vqx_groupnorm_stats");
}

static int gn_glu_fwd_impl(const void* u, int32_t ldu, void* g, int32_t ldg, int32_t dtype, int64_t n_rows,
                           int32_t T, int32_t C, const float* mean_rstd, const float* gamma, const float* beta,
                           const float* tiles, float eps, float* mr_out, vqx_stream_t stream);

extern "C" int vqx_gn_glu_fwd(const void* u, int32_t ldu, void* g, int32_t ldg, int32_t dtype, int64_t n_rows,
                              int32_t T, int32_t C, const float* mean_rstd, const float* gamma, const float* beta,
                              vqx_stream_t stream) {
  return gn_glu_fwd_impl(u, ldu, g, ldg, dtype, n_rows, T, C, mean_rstd, gamma, beta, nullptr, 0.f, nullptr, stream);
}

extern "C" int vqx_gn_glu_fwd_tiles(const void* u, int32_t ldu, void* g, int32_t ldg, int32_t dtype, int64_t n_rows,
                                    int32_t T, int32_t C, const float* parts, float eps, float* mean_rstd,
                                    const float* gamma, const float* beta, vqx_stream_t stream) {
  if (!parts || !mean_rstd || T % 128 || n_rows % T || C % 256) {
    set_error("vqx_gn_glu_fwd_tiles: needs T %% 128 == 0 and C %% 256 == 0");
    return -1;
  }
  return gn_glu_fwd_impl(u, ldu, g, ldg, dtype, n_rows, T, C, nullptr, gamma, beta, parts, eps, mean_rstd, stream);
}

static int gn_glu_fwd_impl(const void* u, int32_t ldu, void* g, int32_t ldg, int32_t dtype, int64_t n_rows,
                           int32_t T, int32_t C, const float* mean_rstd, const float* gamma, const float* beta,
                           const float* tiles, float eps, float* mr_out, vqx_stream_t stream) {
  if (C % 2) { set_error("vqx_gn_glu_fwd: odd C"); return -1; }
  const int V = dtype == VQX_BF16 ? 8 : 4;
  if ((C / 2) % V || ldu % V || ldg % V || (((uintptr_t)u | (uintptr_t)g) & 15)) {
    set_error("vqx_gn_glu_fwd: channels/strides must be multiples of %d", V);
    return -1;
  }
  const int cpr = (C / 2) / V;
  if (cpr > 256 || 256 % cpr) { set_error("vqx_gn_glu_fwd: C/2/%d must divide 256", V); return -1; }
  // frames per workgroup: every workgroup of the in-launch-statistics path
  // merges its utterance's GEMM tiles first, so larger blocks amortise that
  const int fpb = 16;  // frames per workgroup (4/8/32/64 measured slower: profiles/r02/glu_fpb_ab.txt)
  const int grid = (int)((n_rows + fpb - 1) / fpb);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == VQX_BF16)
    hipLaunchKernelGGL(gn_glu_fwd_vec_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, (const bf16_t*)u, ldu, (bf16_t*)g, ldg, (int)n_rows, T, C / 2, cpr, mean_rstd, gamma, beta, tiles, eps, mr_out, fpb);
  else
    hipLaunchKernelGGL(gn_glu_fwd_vec_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)u, ldu, (float*)g, ldg, (int)n_rows, T, C / 2, cpr, mean_rstd, gamma, beta, tiles, eps, mr_out, fpb);
  return launch_status("vqx_gn_glu_fwd");
}

extern "C" int vqx_gn_lrelu_fwd(const void* h, int32_t ldh, void* g, int32_t ldg, int32_t dtype, int64_t n_rows,
                                int32_t T, int32_t C, const float* mean_rstd, const float* gamma, const float* beta,
                                vqx_stream_t stream) {
  const int V = dtype == VQX_BF16 ? 8 : 4;
  if (!h || !g || !mean_rstd || !gamma || !beta || T < 1 || n_rows % T || C % V || ldh % V || ldg % V ||
      (((uintptr_t)h | (uintptr_t)g) & 15)) {
    set_error("vqx_gn_lrelu_fwd: bad arguments (C, strides multiples of %d, 16-B aligned)", V);
    return -1;
  }
  const int cpr = C / V;
  const int64_t total = n_rows * cpr;
  const int grid = (int)std::min<int64_t>((total + 255) / 256, 4096);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == VQX_BF16)
    hipLaunchKernelGGL(gn_lrelu_fwd_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, (const bf16_t*)h, ldh, (bf16_t*)g, ldg,
                       n_rows, T, cpr, mean_rstd, gamma, beta);
  else
    hipLaunchKernelGGL(gn_lrelu_fwd_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)h, ldh, (float*)g, ldg,
                       n_rows, T, cpr, mean_rstd, gamma, beta);
  return launch_status("vqx_gn_lrelu_fwd");
}

extern "C" int vqx_gn_bwd(const void* dy, int32_t lddy, const void* u, int32_t ldu, void* du, int32_t lddu,
                          int32_t dtype, int64_t n_rows, int32_t T, int32_t C, int32_t G, int32_t glu,
                          const float* mean_rstd, const float* gamma, const float* beta, float* partials,
                          int32_t nparts, float* colsum_p, float* dgamma_p, float* dbeta_p, vqx_stream_t stream) {
  if (nparts < 0) { set_error("vqx_gn_bwd: nparts < 0"); return -1; }
  if (glu && G != 2) { set_error("vqx_gn_bwd: glu requires G=2"); return -1; }
  if (!glu && G != 1) { set_error("vqx_gn_bwd: non-glu path supports G=1"); return -1; }
  if (C % G || n_rows % T) { set_error("vqx_gn_bwd: bad shape"); return -1; }
  const int B = (int)(n_rows / T);
  const int V = dtype == VQX_BF16 ? 8 : 4;
  const int span = glu ? C / 2 : C;  // channels covered by the chunk index
  const int cpr = span / V;
  if (span % V || lddy % V || ldu % V || lddu % V || cpr > 256 || 256 % cpr ||
      (((uintptr_t)dy | (uintptr_t)u | (uintptr_t)du) & 15)) {
    set_error("vqx_gn_bwd: channel count / strides must give a power-of-two chunk count <= 256 (C=%d)", C);
    return -1;
  }
  hipStream_t s = (hipStream_t)stream;
  // nparts == 0: reduce here (kGnBwdParts row parts per utterance, G*2 floats
  // each); nparts > 0: the producing GEMM's GNBWD epilogue already wrote
  // nparts tiles per utterance (4 floats each)
  const int np = nparts ? nparts : kGnBwdParts, ps = nparts ? 4 : G * 2;
  if (dtype == VQX_BF16) {
    if (!nparts) hipLaunchKernelGGL(gn_bwd_reduce_vec_kernel<bf16_t>, dim3(kGnBwdParts, B), dim3(256), 0, s, (const bf16_t*)dy, lddy, (const bf16_t*)u, ldu, T, C, G, glu, cpr, mean_rstd, gamma, beta, partials);
    auto* kfn = glu ? gn_bwd_apply_vec_kernel<bf16_t, true> : gn_bwd_apply_vec_kernel<bf16_t, false>;
    hipLaunchKernelGGL(kfn, dim3((cpr * 2 + 15) / 16, B), dim3(512), 0, s, (const bf16_t*)dy, lddy, (const bf16_t*)u, ldu, (bf16_t*)du, lddu, T, C, G, glu, cpr, mean_rstd, gamma, beta, partials, np, ps, colsum_p, dgamma_p, dbeta_p);
  } else {
    if (!nparts) hipLaunchKernelGGL(gn_bwd_reduce_vec_kernel<float>, dim3(kGnBwdParts, B), dim3(256), 0, s, (const float*)dy, lddy, (const float*)u, ldu, T, C, G, glu, cpr, mean_rstd, gamma, beta, partials);
    auto* kfn = glu ? gn_bwd_apply_vec_kernel<float, true> : gn_bwd_apply_vec_kernel<float, false>;
    hipLaunchKernelGGL(kfn, dim3((cpr + 15) / 16, B), dim3(512), 0, s, (const float*)dy, lddy, (const float*)u, ldu, (float*)du, lddu, T, C, G, glu, cpr, mean_rstd, gamma, beta, partials, np, ps, colsum_p, dgamma_p, dbeta_p);
  }
  return launch_status("vqx_gn_bwd");
}

extern "C" int vqx_gn_finalize_tiles(const float* parts, int64_t n_rows, int32_t T, int32_t C, int32_t G, float eps,
                                     float* mean_rstd, vqx_stream_t stream) {
  if (!parts || !mean_rstd || T % 128 || n_rows % T || G < 1 || C % G || (C / G) % 128) {
    set_error("vqx_gn_finalize_tiles: needs T %% 128 == 0 and C/G %% 128 == 0");
    return -1;
  }
  const int B = (int)(n_rows / T);
  hipLaunchKernelGGL(gn_finalize_tiles_kernel, dim3((B * G + 127) / 128), dim3(128), 0, (hipStream_t)stream, parts, B,
                     G, T / 128, C / 128, (C / G) / 128, eps, mean_rstd);
  return launch_status("vqx_gn_finalize_tiles");
}
