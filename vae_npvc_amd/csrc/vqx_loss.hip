// The Gaussian log-likelihood loss and its gradient (gfx950).
#include "vqx_common.h"
#include "vqx_vec.h"

namespace vqx {

constexpr float kLog2Pi = 1.8378770664093453f;  // log(2*pi), layers.py:8

template <typename T>
__global__ __launch_bounds__(256) void logloss_kernel(const float* __restrict__ x, const float* __restrict__ xh, int ldxh,
                                                      int B, int C, int T_, float gscale, T* __restrict__ dx, int lddx,
                                                      float* __restrict__ part) {
  __shared__ float red[16];
  const int64_t total = (int64_t)B * T_ * C;
  float s = 0.f;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)e / C;  // 32-bit: total < 2^31 (host-checked)
    const int c = (int)e - n * C;
    const int b = (int)n / T_, t = (int)n - b * T_;
    const float xv = x[((int64_t)b * C + c) * T_ + t];
    const float d = xh[(int64_t)n * ldxh + c] - xv;
    s += 0.5f * (kLog2Pi + d * d);
    if (dx) Elem<T>::st(dx, (int64_t)n * lddx + c, d * gscale);
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// The same over (utterance, 64-frame tile) blocks: the tile of x (C channels
// x 64 frames, NCT) is read row by row (coalesced) into LDS, then xhat (f32)
// and dx move as whole 4-channel chunks of their frame-major rows (C % 4 ==
// 0), each chunk's channels taken from the LDS tile.  (The flat kernel above
// reads x with a stride of T floats between neighbouring lanes.)
constexpr int kLlTile = 64;
template <typename T>
__global__ __launch_bounds__(256) void logloss_tile_kernel(const float* __restrict__ x, const float* __restrict__ xh,
                                                           int ldxh, int C, int T_, float gscale, T* __restrict__ dx,
                                                           int lddx, float* __restrict__ part) {
  extern __shared__ float xs[];  // [C][kLlTile + 1]
  __shared__ float red[16];
  const int b = blockIdx.y, t0 = blockIdx.x * kLlTile;
  const int nt = min(kLlTile, T_ - t0);
  const float* xb = x + (int64_t)b * C * T_ + t0;
  // loads batched U at a time (clamped addresses, no branch), then their LDS writes:
  // a load-store pair per element paid one memory latency each
  constexpr int U = 16;
  for (int e0 = threadIdx.x; e0 < C * kLlTile; e0 += 256 * U) {
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = min(e0 + 256 * u, C * kLlTile - 1), c = e / kLlTile, t = min(e - c * kLlTile, nt - 1);
      v[u] = xb[(int64_t)c * T_ + t];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = e0 + 256 * u, c = e / kLlTile, t = e - c * kLlTile;
      if (e < C * kLlTile) xs[c * (kLlTile + 1) + t] = t < nt ? v[u] : 0.f;
    }
  }
  __syncthreads();
  const int cpr = C / 4;  // chunks per frame row
  const int64_t n0 = (int64_t)b * T_ + t0;
  const int nq = nt * cpr;
  float s = 0.f;
  constexpr int U2 = 8;
  for (int q0 = threadIdx.x; q0 < nq; q0 += 256 * U2) {
    f32x4_t h[U2];
#pragma unroll
    for (int u = 0; u < U2; ++u) {
      const int qq = min(q0 + 256 * u, nq - 1), t = qq / cpr, c0 = (qq - t * cpr) * 4;
      h[u] = *(const f32x4_t*)(xh + (n0 + t) * ldxh + c0);
    }
#pragma unroll
    for (int u = 0; u < U2; ++u) {
      const int q = q0 + 256 * u;
      if (q >= nq) break;
      const int t = q / cpr, c0 = (q - t * cpr) * 4;
      float o[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float d = h[u][k] - xs[(c0 + k) * (kLlTile + 1) + t];
        s += 0.5f * (kLog2Pi + d * d);
        o[k] = d * gscale;
      }
      if (dx) Vec4<T>::store(dx + (n0 + t) * lddx + c0, o);
    }
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// two such sums in one launch (the log-loss total and another partial set, e.g.
// the VQ kernel's commitment partials), each as sum_partials_scale_kernel
// (vqx_reduce.hip) sums it
__global__ void sum_partials2_kernel(const float* __restrict__ p, int n, float scale, float* __restrict__ out,
                                     const float* __restrict__ p2, int n2, float scale2, float* __restrict__ out2) {
  __shared__ float red[2][16];
  float v[2] = {0.f, 0.f};
  for (int i = threadIdx.x; i < n; i += blockDim.x) v[0] += p[i];
  for (int i = threadIdx.x; i < n2; i += blockDim.x) v[1] += p2[i];
  block_sum_n<2>(v, red);
  if (threadIdx.x == 0) {
    out[0] = v[0] * scale;
    out2[0] = v[1] * scale2;
  }
}

}  // namespace vqx

using namespace vqx;

// loss_out == NULL: the partials only (their count in *n_parts), summed by the caller's later launch
static int logloss_impl(const float* x, const float* xhat, int32_t ldxh, int32_t B, int32_t C, int32_t T,
                        float grad_scale, void* dxhat, int32_t lddx, int32_t dtype, float* loss_out, float* partials,
                        const float* extra_parts, int32_t n_extra, float* extra_out, vqx_stream_t stream,
                        int32_t* n_parts = nullptr) {
  const int64_t total = (int64_t)B * C * T;
  if (total <= 0 || total >= (1LL << 31)) { set_error("vqx_logloss_fwd_bwd: B*C*T must be in [1, 2^31)"); return -1; }
  hipStream_t s = (hipStream_t)stream;
  const int tiles = (T + kLlTile - 1) / kLlTile;
  const uintptr_t dx_align = dtype == VQX_BF16 ? 7 : 15;  // 4-element chunks: 8-B bf16 / 16-B f32 stores
  int grid;
  if (C % 4 == 0 && ldxh % 4 == 0 && (!dxhat || lddx % 4 == 0) && C <= 256 && (int64_t)tiles * B <= 1024 &&
      ((uintptr_t)xhat & 15) == 0 && (!dxhat || ((uintptr_t)dxhat & dx_align) == 0)) {
    grid = tiles * B;  // partials: at most 1024 (the caller's buffer)
    const size_t lds = (size_t)C * (kLlTile + 1) * sizeof(float);
    if (dtype == VQX_BF16)
      hipLaunchKernelGGL(logloss_tile_kernel<bf16_t>, dim3(tiles, B), dim3(256), lds, s, x, xhat, ldxh, C, T, grad_scale, (bf16_t*)dxhat, lddx, partials);
    else
      hipLaunchKernelGGL(logloss_tile_kernel<float>, dim3(tiles, B), dim3(256), lds, s, x, xhat, ldxh, C, T, grad_scale, (float*)dxhat, lddx, partials);
  } else {
    grid = grid_for(total, 256, 1024);
    if (dtype == VQX_BF16)
      hipLaunchKernelGGL(logloss_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, x, xhat, ldxh, B, C, T, grad_scale, (bf16_t*)dxhat, lddx, partials);
    else
      hipLaunchKernelGGL(logloss_kernel<float>, dim3(grid), dim3(256), 0, s, x, xhat, ldxh, B, C, T, grad_scale, (float*)dxhat, lddx, partials);
  }
  if (n_parts) *n_parts = grid;
  if (!loss_out) return launch_status("vqx_logloss_parts");
  if (extra_parts)
    hipLaunchKernelGGL(sum_partials2_kernel, dim3(1), dim3(1024), 0, s, partials, grid, 1.0f / ((float)B * (float)T),
                       loss_out, extra_parts, n_extra, 1.0f, extra_out);
  else
    sum_partials_scale_launch(partials, grid, 1.0f / ((float)B * (float)T), loss_out, s);
  return launch_status("vqx_logloss_fwd_bwd");
}

extern "C" int vqx_logloss_fwd_bwd(const float* x, const float* xhat, int32_t ldxh, int32_t B, int32_t C, int32_t T,
                                   float grad_scale, void* dxhat, int32_t lddx, int32_t dtype, float* loss_out,
                                   float* partials, vqx_stream_t stream) {
  return logloss_impl(x, xhat, ldxh, B, C, T, grad_scale, dxhat, lddx, dtype, loss_out, partials, nullptr, 0, nullptr,
                      stream);
}

extern "C" int vqx_logloss_fwd_bwd_x(const float* x, const float* xhat, int32_t ldxh, int32_t B, int32_t C, int32_t T,
                                     float grad_scale, void* dxhat, int32_t lddx, int32_t dtype, float* loss_out,
                                     float* partials, const float* extra_partials, int32_t n_extra, float* extra_out,
                                     vqx_stream_t stream) {
  if (!extra_partials || !extra_out || n_extra < 1) {
    set_error("vqx_logloss_fwd_bwd_x: needs extra partials and their output");
    return -1;
  }
  return logloss_impl(x, xhat, ldxh, B, C, T, grad_scale, dxhat, lddx, dtype, loss_out, partials, extra_partials,
                      n_extra, extra_out, stream);
}

extern "C" int vqx_logloss_parts(const float* x, const float* xhat, int32_t ldxh, int32_t B, int32_t C, int32_t T,
                                 float grad_scale, void* dxhat, int32_t lddx, int32_t dtype, float* partials,
                                 int32_t* n_parts, vqx_stream_t stream) {
  if (!partials || !n_parts) { set_error("vqx_logloss_parts: needs partials and n_parts"); return -1; }
  return logloss_impl(x, xhat, ldxh, B, C, T, grad_scale, dxhat, lddx, dtype, nullptr, partials, nullptr, 0, nullptr,
                      stream, n_parts);
}
