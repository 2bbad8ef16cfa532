// Column sums and the sum of a set of partials (gfx950): fixed-shape trees in
// a fixed order, no float atomics.
#include "vqx_common.h"
#include "vqx_vec.h"

namespace vqx {

// single-pass column sums for short inputs (rows <= ~2048): 64 columns x 4 row groups per block
template <typename T>
__global__ __launch_bounds__(256) void colsum_small_kernel(const T* __restrict__ x, int ldx, int64_t n_rows, int C,
                                                           float* __restrict__ out, int accum) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int rg = threadIdx.x >> 6;
  __shared__ float acc[4][64];
  float s = 0.f;
  if (c < C)
    for (int64_t r = rg; r < n_rows; r += 4) s += Elem<T>::ld(x, r * ldx + c);
  acc[rg][threadIdx.x & 63] = s;
  __syncthreads();
  if (rg == 0 && c < C) {
    const int l = threadIdx.x & 63;
    const float t = acc[0][l] + acc[1][l] + acc[2][l] + acc[3][l];
    out[c] = accum ? out[c] + t : t;
  }
}

// vectorised partial column sums: 32 chunks x 8 row groups per block
template <typename T>
// Lanes [0, L) of each row group cover L column chunks of V; 256/L row groups
// stride the rows, so narrow outputs (bias gradients of 64..128 columns) keep
// every lane of the block busy instead of 10 of 32.
__global__ __launch_bounds__(256) void colsum_partial_vec_kernel(const T* __restrict__ x, int ldx, int64_t n_rows,
                                                                 int C, int nparts, int L, float* __restrict__ part) {
  constexpr int V = Vec<T>::N;
  const int lane = threadIdx.x % L;
  const int rg = threadIdx.x / L, R = 256 / L;
  const int chunk = blockIdx.x * L + lane;
  const int p = blockIdx.y;
  const int64_t r0 = n_rows * p / nparts, r1 = n_rows * (p + 1) / nparts;
  const int c = chunk * V;
  float s[V];
#pragma unroll
  for (int i = 0; i < V; ++i) s[i] = 0.f;
  if (c < C)
#pragma unroll 4
    for (int64_t r = r0 + rg; r < r1; r += R) {
      float f[V];
      Vec<T>::load(x + r * ldx + c, f);
#pragma unroll
      for (int i = 0; i < V; ++i) s[i] += f[i];
    }
  __shared__ float lds[256 * V];
#pragma unroll
  for (int i = 0; i < V; ++i) lds[threadIdx.x * V + i] = s[i];
  __syncthreads();
  for (int e = threadIdx.x; e < L * V; e += 256) {
    const int cc = blockIdx.x * L * V + e;
    if (cc < C) {
      float t = 0.f;
      for (int q = 0; q < R; ++q) t += lds[q * L * V + e];
      part[(int64_t)p * C + cc] = t;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void colsum_partial_kernel(const T* __restrict__ x, int ldx, int64_t n_rows, int C,
                                                             int nparts, float* __restrict__ part) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int rg = threadIdx.x >> 6;
  const int p = blockIdx.y;
  const int64_t r0 = n_rows * p / nparts, r1 = n_rows * (p + 1) / nparts;
  __shared__ float acc[4][64];
  float s = 0.f;
  if (c < C)
    for (int64_t r = r0 + rg; r < r1; r += 4) s += Elem<T>::ld(x, r * ldx + c);
  acc[rg][threadIdx.x & 63] = s;
  __syncthreads();
  if (rg == 0 && c < C) {
    const int l = threadIdx.x & 63;
    part[(int64_t)p * C + c] = acc[0][l] + acc[1][l] + acc[2][l] + acc[3][l];
  }
}

// One wave per column: lanes stride the (<= 64) partials, then a fixed-order
// butterfly, so the result is deterministic and no lane walks 64 loads.
__global__ __launch_bounds__(256) void colsum_final_kernel(const float* __restrict__ part, int nparts, int C,
                                                           float* __restrict__ out, int accum) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (c >= C) return;
  float s = 0.f;
  for (int p = lane; p < nparts; p += 64) s += part[(int64_t)p * C + c];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) out[c] = accum ? out[c] + s : s;
}

__global__ void sum_partials_scale_kernel(const float* __restrict__ p, int n, float scale, float* __restrict__ out) {
  __shared__ float red[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += p[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[0] = s * scale;
}

void sum_partials_scale_launch(const float* p, int n, float scale, float* out, hipStream_t s) {
  hipLaunchKernelGGL(sum_partials_scale_kernel, dim3(1), dim3(1024), 0, s, p, n, scale, out);
}

}  // namespace vqx

using namespace vqx;

// row parts of the first colsum level and the vector kernel's lanes per row group
static int colsum_geometry(int64_t n_rows, int C, int dtype, int* lanes) {
  const int V = dtype == VQX_BF16 ? 8 : 4;
  int L = 1;  // lanes per row group in the vector kernel: pow2 >= C/V, <= 32
  while (L < 32 && L * V < C) L <<= 1;
  const int colblocks = (C + V * L - 1) / (V * L);  // >= 1 for any C > 0
  int nparts = (256 + colblocks - 1) / colblocks;
  if (nparts > 64) nparts = 64;
  if (nparts > n_rows / 8) nparts = (int)(n_rows / 8);
  if (nparts < 1) nparts = 1;
  if (lanes) *lanes = L;
  return nparts;
}

// first level: partials[p][c] over nparts row parts
static void colsum_partials_launch(const void* x, int ldx, int dtype, int64_t n_rows, int C, int nparts, int L,
                                   float* partials, hipStream_t s) {
  const int V = dtype == VQX_BF16 ? 8 : 4;
  const bool vec = (C % V == 0) && (ldx % V == 0) && (((uintptr_t)x & 15) == 0);
  if (vec) {
    const int nch = C / V;
    if (dtype == VQX_BF16)
      hipLaunchKernelGGL(colsum_partial_vec_kernel<bf16_t>, dim3((nch + L - 1) / L, nparts), dim3(256), 0, s, (const bf16_t*)x, ldx, n_rows, C, nparts, L, partials);
    else
      hipLaunchKernelGGL(colsum_partial_vec_kernel<float>, dim3((nch + L - 1) / L, nparts), dim3(256), 0, s, (const float*)x, ldx, n_rows, C, nparts, L, partials);
  } else if (dtype == VQX_BF16) {
    hipLaunchKernelGGL(colsum_partial_kernel<bf16_t>, dim3((C + 63) / 64, nparts), dim3(256), 0, s, (const bf16_t*)x, ldx, n_rows, C, nparts, partials);
  } else {
    hipLaunchKernelGGL(colsum_partial_kernel<float>, dim3((C + 63) / 64, nparts), dim3(256), 0, s, (const float*)x, ldx, n_rows, C, nparts, partials);
  }
}

extern "C" int vqx_colsum_parts(int64_t n_rows, int32_t C, int32_t dtype, int32_t* nparts) {
  if (n_rows <= 0 || C <= 0 || !nparts) { set_error("vqx_colsum_parts: bad arguments"); return -1; }
  *nparts = colsum_geometry(n_rows, C, dtype, nullptr);
  return 0;
}

extern "C" int vqx_colsum_partials(const void* x, int32_t ldx, int32_t dtype, int64_t n_rows, int32_t C,
                                   float* partials, vqx_stream_t stream) {
  if (!x || !partials || n_rows <= 0 || C <= 0 || ldx < C) { set_error("vqx_colsum_partials: bad arguments"); return -1; }
  int L = 1;
  const int nparts = colsum_geometry(n_rows, C, dtype, &L);
  colsum_partials_launch(x, ldx, dtype, n_rows, C, nparts, L, partials, (hipStream_t)stream);
  return launch_status("vqx_colsum_partials");
}

extern "C" int vqx_colsum(const void* x, int32_t ldx, int32_t dtype, int64_t n_rows, int32_t C, float* partials,
                          float* out, int32_t accumulate, vqx_stream_t stream) {
  if (n_rows <= 0 || C <= 0) { set_error("vqx_colsum: bad shape"); return -1; }
  hipStream_t s = (hipStream_t)stream;
  if (n_rows <= 64) {
    if (dtype == VQX_BF16)
      hipLaunchKernelGGL(colsum_small_kernel<bf16_t>, dim3((C + 63) / 64), dim3(256), 0, s, (const bf16_t*)x, ldx, n_rows, C, out, accumulate);
    else
      hipLaunchKernelGGL(colsum_small_kernel<float>, dim3((C + 63) / 64), dim3(256), 0, s, (const float*)x, ldx, n_rows, C, out, accumulate);
    return launch_status("vqx_colsum");
  }
  int L = 1;
  const int nparts = colsum_geometry(n_rows, C, dtype, &L);
  colsum_partials_launch(x, ldx, dtype, n_rows, C, nparts, L, partials, s);
  hipLaunchKernelGGL(colsum_final_kernel, dim3((C + 3) / 4), dim3(256), 0, s, partials, nparts, C, out, accumulate);
  return launch_status("vqx_colsum");
}
