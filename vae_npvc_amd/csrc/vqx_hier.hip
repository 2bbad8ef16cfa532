// Level upsampling + channel concatenation of the hierarchical decoders
// (include/vqx.h vqx_upsample_cat_*; reference vqvae2.py:105-114 `upsample`,
// 130-143 the torch.cat of the stretched levels) and its adjoint.
//
// A level l is frame-major fp32 [B][T_l][C_l]; stretched to T frames, frame t
// reads source frame src_l(t) = min(t / (T / T_l), T_l - 1): repetition by
// T / T_l, the tail replicate-padded from the last frame.
//   forward   hier_cat_fwd_kernel  one thread per (output row, V channels):
//             out[b*T + t][off_l + c] = z_l[b][src_l(t)][c], converted to the
//             destination type.  Pure copy: V = 8 (two 16-B loads, 16-B or
//             2 x 16-B stores) when every width and offset allows, else V = 4.
//   backward  hier_cat_bwd_kernel  one (level, b, s, 4 channels) item per
//             thread column: dz_l[b][s][c] = sum of dout[b*T + t][off_l + c]
//             over the frames t of segment s.
// Summation order of the backward (fixed, no atomics): the segment's frames
// t0 .. t1-1 are cut into P contiguous chunks of ceil((t1 - t0) / P) frames;
// each chunk is added in ascending t starting from 0.f, and the chunk sums are
// added in ascending chunk order starting from 0.f.  P = 1 when the longest
// segment of the call (the tail segment T - (T_l - 1) * (T / T_l) of some
// level) is below 32 frames, else 8; it depends on the shapes alone, so two
// calls with the same shapes give the same bits.  vqx_upsample_cat_bwd_to runs
// the same kernel with the final store templated: the fp32 sum as it is, or
// rounded once to bf16 (nearest even) into a bf16 level of the same ld.
//
// The first decoder's input from codes (include/vqx.h vqx_codes_upsample_cat):
//   hier_codes_cat_kernel  one wavefront per output row; a level is dense (a
//             level of the forward above) or an int64 index into a codebook,
//             whose row is copied or divided by its own L2 norm.
//
// Masked layout change of the hierarchical encoder's backward (include/vqx.h
// vqx_nct_to_ntc_lrelu_bwd): the (B, C, T) f32 gradient autograd hands to the
// encoder's second output, through the LeakyReLU that produced it, as the
// frame-major operand of the next GEMM's residual epilogue:
//   hier_lrelu_bwd_kernel  one 32 x 32 (frames x channels) tile a workgroup,
//             transposed through LDS as nct_to_ntc_tile does (reads run along
//             T, writes along C): dst[b*T + t][c] = g[b][c][t] * (a[b*T + t][c]
//             > 0 ? 1 : slope), one f32 product rounded once to the
//             destination type.
#include "vqx_common.h"

namespace vqx {
namespace {

constexpr int HIER_MAX_LEVELS = 8;
constexpr int HIER_THREADS = 256;
constexpr int HIER_BWD_LANES = 64;   // items per workgroup of the backward
constexpr int HIER_BWD_PARTS = 8;    // chunks per long segment
constexpr int HIER_LONG_SEG = 32;    // segments from this length up are cut into chunks

// Passed by value (as vqx_gather_rows_host passes its rows): no device table.
struct HierLevels {
  float* z[HIER_MAX_LEVELS];       // fwd: source; bwd: destination
  int64_t start[HIER_MAX_LEVELS];  // bwd: first item of the level
  int T_l[HIER_MAX_LEVELS], rep[HIER_MAX_LEVELS], ld[HIER_MAX_LEVELS];
  int g0[HIER_MAX_LEVELS];         // first granule (V channels) of the level in an output row
  int off[HIER_MAX_LEVELS];        // first output column of the level
  int n;
};

struct HierPick {
  float* z;
  int64_t start;
  int T_l, rep, ld, g0, off;
};

// Level of granule g (fwd) or item i (bwd): the last level whose start is not
// above it.  Unrolled selects on uniform loads, no divergent table index.
template <bool BY_ITEM>
__device__ __forceinline__ HierPick hier_pick(const HierLevels& L, int64_t key) {
  HierPick p = {L.z[0], L.start[0], L.T_l[0], L.rep[0], L.ld[0], L.g0[0], L.off[0]};
#pragma unroll
  for (int l = 1; l < HIER_MAX_LEVELS; ++l) {
    const bool take = l < L.n && key >= (BY_ITEM ? L.start[l] : (int64_t)L.g0[l]);
    if (take) p = {L.z[l], L.start[l], L.T_l[l], L.rep[l], L.ld[l], L.g0[l], L.off[l]};
  }
  return p;
}

template <int V, bool BF16>
__global__ __launch_bounds__(HIER_THREADS) void hier_cat_fwd_kernel(HierLevels L, int64_t rows, int T, int gran,
                                                                     void* __restrict__ out, int64_t ldo) {
  const int64_t i = (int64_t)blockIdx.x * HIER_THREADS + threadIdx.x;
  if (i >= rows * gran) return;
  const int64_t row = i / gran;
  const int g = (int)(i - row * gran);
  const HierPick p = hier_pick<false>(L, g);
  const int b = (int)(row / T), t = (int)(row - (int64_t)b * T);
  int s = t / p.rep;
  s = s < p.T_l ? s : p.T_l - 1;
  const int c = (g - p.g0) * V;
  const float* src = p.z + ((int64_t)b * p.T_l + s) * p.ld + c;
  const int64_t at = row * ldo + p.off + c;
  float v[V];
#pragma unroll
  for (int q = 0; q < V / 4; ++q) {
    const f32x4_t x = *(const f32x4_t*)(src + 4 * q);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[4 * q + e] = x[e];
  }
  if constexpr (BF16) {
    unsigned w[V / 2];
#pragma unroll
    for (int e = 0; e < V / 2; ++e) w[e] = pack_bf16x2(v[2 * e], v[2 * e + 1]);
    bf16_t* dst = (bf16_t*)out + at;
    if constexpr (V == 8) *(uint4*)dst = make_uint4(w[0], w[1], w[2], w[3]);
    else *(uint2*)dst = make_uint2(w[0], w[1]);
  } else {
    float* dst = (float*)out + at;
#pragma unroll
    for (int q = 0; q < V / 4; ++q) {
      const f32x4_t x = {v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
      *(f32x4_t*)(dst + 4 * q) = x;
    }
  }
}

// The backward's one store of an item's four sums: fp32, or bf16 rounded once
// (the level is then bf16 [B][T_l][ld]; at is the element offset in either type).
template <bool OUT_BF16>
__device__ __forceinline__ void hier_store_sum(float* z, int64_t at, const f32x4_t& v) {
  if constexpr (OUT_BF16) {
    *(uint2*)((bf16_t*)z + at) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
  } else {
    *(f32x4_t*)(z + at) = v;
  }
}

// blockDim = (HIER_BWD_LANES, P): lane x owns one item, chunk y of its segment.
template <bool BF16, bool OUT_BF16>
__global__ __launch_bounds__(HIER_BWD_LANES* HIER_BWD_PARTS) void hier_cat_bwd_kernel(HierLevels L, int64_t items, int T,
                                                                                      const void* __restrict__ dout,
                                                                                      int64_t ldo) {
  __shared__ f32x4_t part[HIER_BWD_PARTS][HIER_BWD_LANES];
  const int64_t i = (int64_t)blockIdx.x * HIER_BWD_LANES + threadIdx.x;
  const int P = blockDim.y, y = threadIdx.y;
  const bool live = i < items;
  HierPick p = hier_pick<true>(L, live ? i : 0);
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  int64_t dst = 0;
  if (live) {  // items of a level are ordered (b, s, granule of 4 channels)
    const int gl = p.g0;  // the backward table's g0 is the level's granule count C_l / 4
    const int64_t j = i - p.start;
    const int g = (int)(j % gl);
    const int64_t bs = j / gl;
    const int s = (int)(bs % p.T_l);
    const int64_t b = bs / p.T_l;
    const int t0 = s * p.rep, t1 = s == p.T_l - 1 ? T : t0 + p.rep;
    const int len = t1 - t0, chunk = (len + P - 1) / P;
    const int a0 = t0 + y * chunk, a1 = a0 + chunk < t1 ? a0 + chunk : t1;
    const int64_t col = p.off + 4 * g;
    for (int t = a0; t < a1; ++t) {
      const int64_t at = (b * T + t) * ldo + col;
      if constexpr (BF16) {
        const uint2 w = *(const uint2*)((const bf16_t*)dout + at);
        acc[0] += __uint_as_float(w.x << 16);
        acc[1] += __uint_as_float(w.x & 0xffff0000u);
        acc[2] += __uint_as_float(w.y << 16);
        acc[3] += __uint_as_float(w.y & 0xffff0000u);
      } else {
        const f32x4_t x = *(const f32x4_t*)((const float*)dout + at);
        acc += x;
      }
    }
    dst = (b * p.T_l + s) * p.ld + 4 * g;
  }
  if (P == 1) {
    if (live) hier_store_sum<OUT_BF16>(p.z, dst, acc);
    return;
  }
  part[y][threadIdx.x] = acc;
  __syncthreads();
  if (y == 0 && live) {
    f32x4_t sum = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < P; ++k) sum += part[k][threadIdx.x];
    hier_store_sum<OUT_BF16>(p.z, dst, sum);
  }
}

// Levels of vqx_codes_upsample_cat, by value.  src is the dense level or the
// codebook; idx == nullptr marks a dense level.
struct CodeLevels {
  const float* src[HIER_MAX_LEVELS];
  const int64_t* idx[HIER_MAX_LEVELS];
  int T_l[HIER_MAX_LEVELS], rep[HIER_MAX_LEVELS], ld[HIER_MAX_LEVELS];
  int gran[HIER_MAX_LEVELS];       // C_l / 4: 16-byte granules of the level in an output row
  int off[HIER_MAX_LEVELS];        // first output column of the level
  int normalize[HIER_MAX_LEVELS];
  int n;
};

constexpr int CODES_WAVES = HIER_THREADS / 64;  // output rows per workgroup

// One wavefront per output row; lane j moves granules j, j + 64, ... of each
// level with 16-byte loads and stores (rows are 64 to 256 floats: one or two
// rounds).  Everything that selects a path (row, level kind, normalize) is
// wave-uniform, so the shuffles of wave_sum see all 64 lanes.  A normalised
// level reads its codebook row twice: once for sum of squares (each lane adds
// its granules' squares in column order, wave_sum adds the lanes), once to
// write E[k][c] / sqrt(sum); the second read hits the cache.
template <bool BF16>
__global__ __launch_bounds__(HIER_THREADS) void hier_codes_cat_kernel(CodeLevels L, int64_t rows, int T,
                                                                       void* __restrict__ out, int64_t ldo) {
  const int lane = threadIdx.x & 63;
  // the wave's index through readfirstlane: the compiler then keeps the row, the code index and the
  // row addresses in scalar registers and branches on them without exec masks
  const int64_t row = (int64_t)blockIdx.x * CODES_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (row >= rows) return;
  const int64_t b = row / T;
  const int t = (int)(row - b * T);
#pragma unroll
  for (int l = 0; l < HIER_MAX_LEVELS; ++l) {
    if (l >= L.n) break;
    int s = t / L.rep[l];
    s = s < L.T_l[l] ? s : L.T_l[l] - 1;
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

template <typename TA, typename TD>
__global__ __launch_bounds__(256) void hier_lrelu_bwd_kernel(const float* __restrict__ g, int C, int T,
                                                             const TA* __restrict__ a, int64_t lda, float slope,
                                                             TD* __restrict__ dst, int64_t ldd) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z;
  const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 256 threads: 8 rows per pass
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, t = t0 + tx;
    tile[i][tx] = (c < C && t < T) ? g[((int64_t)b * C + c) * T + t] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int t = t0 + i, c = c0 + tx;
    if (c < C && t < T) {
      const int64_t row = (int64_t)b * T + t;
      const float m = Elem<TA>::ld(a, row * lda + c) > 0.f ? 1.f : slope;
      Elem<TD>::st(dst, row * ldd + c, tile[tx][i] * m);
    }
  }
}

// x[b][c][t] = y[b*T + t][c] * g[0]: vqx_ntc_to_nct (vqx_layout.hip) with one device scalar folded in.
__global__ __launch_bounds__(256) void hier_ntc_to_nct_scale_kernel(const float* __restrict__ y, int64_t ldy, int C,
                                                                    int T, const float* __restrict__ g,
                                                                    float* __restrict__ x) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z;
  const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const float s = *g;
  for (int i = ty; i < 32; i += 8) {
    const int t = t0 + i, c = c0 + tx;
    tile[i][tx] = (c < C && t < T) ? y[((int64_t)b * T + t) * ldy + c] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, t = t0 + tx;
    if (c < C && t < T) x[((int64_t)b * C + c) * T + t] = tile[tx][i] * s;
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Checks shared by both directions; fills the by-value table.  `v8` = every
// width, offset and stride allows 8-channel granules.
int hier_prepare(const char* who, const vqx_hier_level* lv, int n, int B, int T, const void* out, int ldo, int dtype,
                 HierLevels& L, int& total, bool& v8, int& longest) {
  if (!lv) { set_error("%s: null levels", who); return -1; }
  if (n < 1 || n > HIER_MAX_LEVELS) { set_error("%s: n_levels = %d not in 1..%d", who, n, HIER_MAX_LEVELS); return -1; }
  if (dtype != VQX_F32 && dtype != VQX_BF16) { set_error("%s: bad dtype %d", who, dtype); return -1; }
  if (B < 1 || T < 1 || (int64_t)B * T > INT32_MAX) { set_error("%s: B = %d, T = %d (B*T must fit 31 bits)", who, B, T); return -1; }
  if (!out || !aligned16(out)) { set_error("%s: null or unaligned (16 B) full-rate pointer", who); return -1; }
  L = HierLevels{};
  L.n = n;
  total = 0;
  longest = 1;
  v8 = ldo % 8 == 0;
  for (int l = 0; l < n; ++l) {
    const vqx_hier_level& v = lv[l];
    if (!v.z || !aligned16(v.z)) { set_error("%s: level %d: null or unaligned (16 B) pointer", who, l); return -1; }
    if (v.T_l < 1 || v.T_l > T) { set_error("%s: level %d: T_l = %d not in 1..T = %d", who, l, v.T_l, T); return -1; }
    if (v.C < 4 || v.C % 4 || v.ld % 4 || v.ld < v.C) { set_error("%s: level %d: C = %d / ld = %d must be multiples of 4, ld >= C", who, l, v.C, v.ld); return -1; }
    L.z[l] = (float*)v.z;
    L.T_l[l] = v.T_l;
    L.rep[l] = T / v.T_l;
    L.ld[l] = v.ld;
    L.off[l] = total;
    if (v.C % 8) v8 = false;
    const int last = T - (v.T_l - 1) * (T / v.T_l);  // the tail segment is the longest
    if (last > longest) longest = last;
    if ((int64_t)total + v.C > INT32_MAX) { set_error("%s: channel sum overflows", who); return -1; }
    total += v.C;
  }
  if (ldo % 4 || total > ldo) { set_error("%s: sum of C_l = %d exceeds ldo = %d (ldo a multiple of 4)", who, total, ldo); return -1; }
  return 0;
}

}  // namespace
}  // namespace vqx

using namespace vqx;

extern "C" int vqx_upsample_cat_fwd(const vqx_hier_level* levels, int32_t n_levels, int32_t B, int32_t T, void* out,
                                    int32_t ldo, int32_t out_dtype, vqx_stream_t stream) {
  HierLevels L;
  int total, longest;
  bool v8;
  if (hier_prepare("vqx_upsample_cat_fwd", levels, n_levels, B, T, out, ldo, out_dtype, L, total, v8, longest)) return -1;
  const int V = v8 ? 8 : 4;
  for (int l = 0; l < n_levels; ++l) L.g0[l] = L.off[l] / V;
  const int gran = total / V;
  const int64_t rows = (int64_t)B * T, threads = rows * gran;
  const int64_t grid = (threads + HIER_THREADS - 1) / HIER_THREADS;
  if (grid > INT32_MAX) { set_error("vqx_upsample_cat_fwd: %lld workgroups", (long long)grid); return -1; }
  hipStream_t s = (hipStream_t)stream;
  const bool bf = out_dtype == VQX_BF16;
  auto* fn = v8 ? (bf ? hier_cat_fwd_kernel<8, true> : hier_cat_fwd_kernel<8, false>)
                : (bf ? hier_cat_fwd_kernel<4, true> : hier_cat_fwd_kernel<4, false>);
  hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(HIER_THREADS), 0, s, L, rows, T, gran, out, (int64_t)ldo);
  return launch_status("vqx_upsample_cat_fwd");
}

// Both backward entry points: the checks, the item table and the launch.
static int hier_cat_bwd(const char* who, const vqx_hier_level* levels, int n_levels, int B, int T, const void* dout,
                        int ldo, int dout_dtype, int level_dtype, vqx_stream_t stream) {
  if (level_dtype != VQX_F32 && level_dtype != VQX_BF16) { set_error("%s: bad level_dtype %d", who, level_dtype); return -1; }
  HierLevels L;
  int total, longest;
  bool v8;
  if (hier_prepare(who, levels, n_levels, B, T, dout, ldo, dout_dtype, L, total, v8, longest)) return -1;
  int64_t items = 0;
  for (int l = 0; l < n_levels; ++l) {
    L.start[l] = items;
    L.g0[l] = levels[l].C / 4;  // granules per source frame
    items += (int64_t)B * L.T_l[l] * L.g0[l];
  }
  const int64_t grid = (items + HIER_BWD_LANES - 1) / HIER_BWD_LANES;
  if (grid > INT32_MAX) { set_error("%s: %lld workgroups", who, (long long)grid); return -1; }
  const int P = longest >= HIER_LONG_SEG ? HIER_BWD_PARTS : 1;
  hipStream_t s = (hipStream_t)stream;
  const bool bf = dout_dtype == VQX_BF16;
  auto* fn = level_dtype == VQX_BF16 ? (bf ? hier_cat_bwd_kernel<true, true> : hier_cat_bwd_kernel<false, true>)
                                     : (bf ? hier_cat_bwd_kernel<true, false> : hier_cat_bwd_kernel<false, false>);
  hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(HIER_BWD_LANES, P), 0, s, L, items, T, dout, (int64_t)ldo);
  return launch_status(who);
}

extern "C" int vqx_upsample_cat_bwd(const vqx_hier_level* levels, int32_t n_levels, int32_t B, int32_t T,
                                    const void* dout, int32_t ldo, int32_t dout_dtype, vqx_stream_t stream) {
  return hier_cat_bwd("vqx_upsample_cat_bwd", levels, n_levels, B, T, dout, ldo, dout_dtype, VQX_F32, stream);
}

extern "C" int vqx_upsample_cat_bwd_to(const vqx_hier_level* levels, int32_t n_levels, int32_t B, int32_t T,
                                       const void* dout, int32_t ldo, int32_t dout_dtype, int32_t level_dtype,
                                       vqx_stream_t stream) {
  return hier_cat_bwd("vqx_upsample_cat_bwd_to", levels, n_levels, B, T, dout, ldo, dout_dtype, level_dtype, stream);
}

extern "C" int vqx_codes_upsample_cat(const vqx_codes_level* levels, int32_t n_levels, int32_t B, int32_t T, void* out,
                                      int32_t ldo, int32_t out_dtype, vqx_stream_t stream) {
  const char* who = "vqx_codes_upsample_cat";
  if (!levels) { set_error("%s: null levels", who); return -1; }
  if (n_levels < 1 || n_levels > HIER_MAX_LEVELS) { set_error("%s: n_levels = %d not in 1..%d", who, n_levels, HIER_MAX_LEVELS); return -1; }
  if (out_dtype != VQX_F32 && out_dtype != VQX_BF16) { set_error("%s: bad dtype %d", who, out_dtype); return -1; }
  if (B < 1 || T < 1 || (int64_t)B * T > INT32_MAX) { set_error("%s: B = %d, T = %d (B*T must fit 31 bits)", who, B, T); return -1; }
  if (!out || !aligned16(out)) { set_error("%s: null or unaligned (16 B) out pointer", who); return -1; }
  CodeLevels L = {};
  L.n = n_levels;
  int total = 0;
  for (int l = 0; l < n_levels; ++l) {
    const vqx_codes_level& v = levels[l];
    if (!v.z || !aligned16(v.z)) { set_error("%s: level %d: null or unaligned (16 B) %s pointer", who, l, v.idx ? "codebook" : "z"); return -1; }
    if (v.idx && !aligned16(v.idx)) { set_error("%s: level %d: unaligned (16 B) idx pointer", who, l); return -1; }
    if (v.T_l < 1 || v.T_l > T) { set_error("%s: level %d: T_l = %d not in 1..T = %d", who, l, v.T_l, T); return -1; }
    if (v.C < 4 || v.C % 4 || v.ld % 4 || v.ld < v.C) { set_error("%s: level %d: C = %d / ld = %d must be multiples of 4, ld >= C", who, l, v.C, v.ld); return -1; }
    if (v.idx && v.K < 1) { set_error("%s: level %d: K = %d codes", who, l, v.K); return -1; }
    if ((int64_t)total + v.C > INT32_MAX) { set_error("%s: channel sum overflows", who); return -1; }
    L.src[l] = (const float*)v.z;
    L.idx[l] = v.idx;
    L.T_l[l] = v.T_l;
    L.rep[l] = T / v.T_l;
    L.ld[l] = v.ld;
    L.gran[l] = v.C / 4;
    L.off[l] = total;
    L.normalize[l] = v.idx && v.normalize;
    total += v.C;
  }
  if (ldo % 4 || total > ldo) { set_error("%s: sum of C_l = %d exceeds ldo = %d (ldo a multiple of 4)", who, total, ldo); return -1; }
  const int64_t rows = (int64_t)B * T;
  const int64_t grid = (rows + CODES_WAVES - 1) / CODES_WAVES;
  auto* fn = out_dtype == VQX_BF16 ? hier_codes_cat_kernel<true> : hier_codes_cat_kernel<false>;
  hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(HIER_THREADS), 0, (hipStream_t)stream, L, rows, T, out, (int64_t)ldo);
  return launch_status(who);
}

extern "C" int vqx_nct_to_ntc_lrelu_bwd(const float* g_nct, int32_t B, int32_t C, int32_t T, const void* a, int32_t lda,
                                        int32_t a_dtype, float slope, void* dst, int32_t lddst, int32_t dst_dtype,
                                        vqx_stream_t stream) {
  const char* who = "vqx_nct_to_ntc_lrelu_bwd";
  if (!g_nct || !a || !dst) { set_error("%s: null pointer", who); return -1; }
  if ((a_dtype != VQX_F32 && a_dtype != VQX_BF16) || (dst_dtype != VQX_F32 && dst_dtype != VQX_BF16)) {
    set_error("%s: bad dtype %d / %d", who, a_dtype, dst_dtype);
    return -1;
  }
  if (B < 1 || C < 1 || T < 1 || B > 65535 || (C + 31) / 32 > 65535) {
    set_error("%s: B = %d, C = %d, T = %d (1 <= B <= 65535, 1 <= C <= 2097120, T >= 1)", who, B, C, T);
    return -1;
  }
  if (lda < C || lddst < C) { set_error("%s: lda = %d / lddst = %d below C = %d", who, lda, lddst, C); return -1; }
  const dim3 grid((unsigned)((T + 31) / 32), (unsigned)((C + 31) / 32), (unsigned)B);
  hipStream_t s = (hipStream_t)stream;
#define VQX_HIER_LRELU(TA, TD)                                                                                  \
  hipLaunchKernelGGL((hier_lrelu_bwd_kernel<TA, TD>), grid, dim3(256), 0, s, g_nct, C, T, (const TA*)a, (int64_t)lda, \
                     slope, (TD*)dst, (int64_t)lddst)
  if (a_dtype == VQX_BF16) {
    if (dst_dtype == VQX_BF16) VQX_HIER_LRELU(bf16_t, bf16_t); else VQX_HIER_LRELU(bf16_t, float);
  } else {
    if (dst_dtype == VQX_BF16) VQX_HIER_LRELU(float, bf16_t); else VQX_HIER_LRELU(float, float);
  }
#undef VQX_HIER_LRELU
  return launch_status(who);
}

extern "C" int vqx_ntc_to_nct_scale(const float* y, int32_t ldy, int32_t B, int32_t C, int32_t T, const float* g,
                                    float* x_nct, vqx_stream_t stream) {
  const char* who = "vqx_ntc_to_nct_scale";
  if (!y || !g || !x_nct) { set_error("%s: null pointer", who); return -1; }
  if (B < 1 || C < 1 || T < 1 || B > 65535 || (C + 31) / 32 > 65535 || ldy < C) {
    set_error("%s: B = %d, C = %d, T = %d, ldy = %d (1 <= B <= 65535, C, T >= 1, ldy >= C)", who, B, C, T, ldy);
    return -1;
  }
  const dim3 grid((unsigned)((T + 31) / 32), (unsigned)((C + 31) / 32), (unsigned)B);
  hipLaunchKernelGGL(hier_ntc_to_nct_scale_kernel, grid, dim3(256), 0, (hipStream_t)stream, y, (int64_t)ldy, C, T, g,
                     x_nct);
  return launch_status(who);
}
