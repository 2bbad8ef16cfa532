// Layout and dtype conversion (gfx950): NCT <-> NTC transposes, the frame
// gather, and the 2-D convert / scale / activation maps.
#include "vqx_common.h"
#include "vqx_vec.h"

namespace vqx {

// one 32 x 32 tile a block (x over T, y over C, z the batch row): nct_to_ntc_tile, vqx_common.h
template <typename T>
__global__ void nct_to_ntc_kernel(const float* __restrict__ x, int B, int C, int T_, T* __restrict__ y, int ldy) {
  __shared__ float tile[32][33];
  nct_to_ntc_tile<T>(x, C, T_, y, ldy, blockIdx.x, blockIdx.y, blockIdx.z, tile);
}

template <typename T>
__global__ void ntc_to_nct_kernel(const T* __restrict__ y, int ldy, int B, int C, int T_, float* __restrict__ x) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z;
  const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int t = t0 + i, c = c0 + tx;
    tile[i][tx] = (c < C && t < T_) ? Elem<T>::ld(y, ((int64_t)b * T_ + t) * ldy + c) : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, t = t0 + tx;
    if (c < C && t < T_) x[((int64_t)b * C + c) * T_ + t] = tile[tx][i];
  }
}

// ntc_to_nct_kernel with the jitter gather folded in: frame t of the output is
// row src[t] of the input (src NULL: row t).  A map entry is clamped into
// 0..T-1, so no map can send a read outside y.
template <typename T>
__global__ __launch_bounds__(256) void ntc_to_nct_gather_kernel(const T* __restrict__ y, int64_t ldy, int C, int T_,
                                                                const int* __restrict__ src, float* __restrict__ x) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z;
  const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int t = t0 + i, c = c0 + tx;
    float v = 0.f;
    if (c < C && t < T_) {
      int s = src ? src[t] : t;
      s = s < 0 ? 0 : (s >= T_ ? T_ - 1 : s);
      v = Elem<T>::ld(y, ((int64_t)b * T_ + s) * ldy + c);
    }
    tile[i][tx] = v;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, t = t0 + tx;
    if (c < C && t < T_) x[((int64_t)b * C + c) * T_ + t] = tile[tx][i];
  }
}

// nct_to_ntc_tile with the jitter's backward folded in: a frame whose map
// entry is not itself was overwritten by a detached copy and passes no
// gradient (src NULL: every frame kept).
template <typename T>
__global__ __launch_bounds__(256) void nct_to_ntc_keep_kernel(const float* __restrict__ g, int C, int T_,
                                                              const int* __restrict__ src, T* __restrict__ y,
                                                              int64_t ldy) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z;
  const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, t = t0 + tx;
    tile[i][tx] = (c < C && t < T_) ? g[((int64_t)b * C + c) * T_ + t] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int t = t0 + i, c = c0 + tx;
    if (c < C && t < T_) {
      const bool keep = !src || src[t] == t;
      Elem<T>::st(y, ((int64_t)b * T_ + t) * ldy + c, keep ? tile[tx][i] : 0.f);
    }
  }
}

template <typename T>
__global__ void time_gather_kernel(const T* __restrict__ x, T* __restrict__ y, int B, int T_, int C,
                                   const int* __restrict__ src) {
  const int64_t total = (int64_t)B * T_ * C;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)e / C;  // 32-bit: total < 2^31 (host-checked)
    const int c = (int)e - n * C;
    const int b = (int)n / T_, t = (int)n - b * T_;
    y[e] = x[((int64_t)b * T_ + src[t]) * C + c];
  }
}

__global__ __launch_bounds__(256) void scale_act_2d_kernel(const void* __restrict__ src, int lds, int sdt,
                                                           void* __restrict__ dst, int ldd, int ddt, int64_t rows,
                                                           int cols, float scale, int act) {
  const int64_t total = rows * cols;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / cols;
    const int c = (int)(e - r * cols);
    float v = scale * ld_dt(src, r * lds + c, sdt);
    if (act == VQX_PRO_RELU) v = v > 0.f ? v : 0.f;
    else if (act == VQX_PRO_LRELU) v = v > 0.f ? v : 0.2f * v;
    st_dt(dst, r * ldd + c, v, ddt);
  }
}

__global__ __launch_bounds__(256) void convert_2d_kernel(const void* __restrict__ src, int lds, int sdt,
                                                         void* __restrict__ dst, int ldd, int ddt, int64_t rows,
                                                         int cols) {
  const int64_t total = rows * cols;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / cols;
    const int c = (int)(e - r * cols);
    const float v = src ? ld_dt(src, r * lds + c, sdt) : 0.f;
    st_dt(dst, r * ldd + c, v, ddt);
  }
}

// convert_2d / scale_act_2d on 8-element chunks (cols, both leading
// dimensions multiples of 8, 16-B aligned rows): 16-B bf16 / 2 x 16-B f32
// accesses, four chunks' loads in flight per thread, 32-bit chunk indexing
// (the element kernels above divide 64-bit indices and move 2-4 B a lane);
// Chunk8: vqx_vec.h.
// zdst (optional): a second matrix (n8z chunks, cprz per row) set to zero in the
// same launch (vqx_convert_2d_zero2): chunk indices past n8 address it
template <typename S, typename D, bool ZERO>
__global__ __launch_bounds__(256) void map8_kernel(const S* __restrict__ src, int lds, D* __restrict__ dst, int ldd,
                                                   int n8, int cpr, float scale, int act, D* __restrict__ zdst,
                                                   int ldz, int n8z, int cprz) {
  constexpr int U = 4;
  const int stride = gridDim.x * 256;
  const int total = n8 + n8z;
  for (int q0 = blockIdx.x * 256 + threadIdx.x; q0 < total; q0 += U * stride) {
    float v[U][8];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = q0 + u * stride;
      if (ZERO || q >= n8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[u][k] = 0.f;
      } else {
        const int r = q / cpr, c = (q - r * cpr) * 8;
        Chunk8<S>::ld(src + (int64_t)r * lds + c, v[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = q0 + u * stride;
      if (q >= total) break;
      if (q < n8) {
        const int r = q / cpr, c = (q - r * cpr) * 8;
        if (!ZERO) {
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            float x = scale * v[u][k];
            if (act == VQX_PRO_RELU) x = x > 0.f ? x : 0.f;
            else if (act == VQX_PRO_LRELU) x = x > 0.f ? x : 0.2f * x;
            v[u][k] = x;
          }
        }
        Chunk8<D>::st(dst + (int64_t)r * ldd + c, v[u]);
      } else {
        const int qz = q - n8, r = qz / cprz, c = (qz - r * cprz) * 8;
        Chunk8<D>::st(zdst + (int64_t)r * ldz + c, v[u]);  // zeros
      }
    }
  }
}

}  // namespace vqx

using namespace vqx;

extern "C" int vqx_nct_to_ntc(const float* x, int32_t B, int32_t C, int32_t T, void* y, int32_t ldy, int32_t dtype,
                              vqx_stream_t stream) {
  dim3 grid((T + 31) / 32, (C + 31) / 32, B);
  if (dtype == VQX_BF16)
    hipLaunchKernelGGL(nct_to_ntc_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, x, B, C, T, (bf16_t*)y, ldy);
  else
    hipLaunchKernelGGL(nct_to_ntc_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, x, B, C, T, (float*)y, ldy);
  return launch_status("vqx_nct_to_ntc");
}

extern "C" int vqx_ntc_to_nct(const void* y, int32_t ldy, int32_t dtype, int32_t B, int32_t C, int32_t T, float* x,
                              vqx_stream_t stream) {
  dim3 grid((T + 31) / 32, (C + 31) / 32, B);
  if (dtype == VQX_BF16)
    hipLaunchKernelGGL(ntc_to_nct_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)y, ldy, B, C, T, x);
  else
    hipLaunchKernelGGL(ntc_to_nct_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)y, ldy, B, C, T, x);
  return launch_status("vqx_ntc_to_nct");
}

// host checks shared by the two jitter layout changes; 0 when the launch may go
static int jitter_layout_check(const char* who, const void* a, const void* b, int32_t B, int32_t C, int32_t T,
                               int32_t ldy, int32_t dtype) {
  if (!a || !b) { set_error("%s: null pointer", who); return -1; }
  if (dtype != VQX_F32 && dtype != VQX_BF16) { set_error("%s: bad dtype %d", who, dtype); return -1; }
  if (T < 1 || C < 1 || B < 1 || B > 65535 || ldy < C) {
    set_error("%s: B = %d, C = %d, T = %d, ldy = %d (1 <= B <= 65535, C, T >= 1, ldy >= C)", who, B, C, T, ldy);
    return -1;
  }
  if ((int64_t)B * T * C >= (1LL << 31)) { set_error("%s: B*T*C must be < 2^31", who); return -1; }
  return 0;
}

extern "C" int vqx_ntc_to_nct_gather(const void* y, int32_t ldy, int32_t dtype, int32_t B, int32_t C, int32_t T,
                                     const int32_t* src_t, float* x_nct, vqx_stream_t stream) {
  const char* who = "vqx_ntc_to_nct_gather";
  if (jitter_layout_check(who, y, x_nct, B, C, T, ldy, dtype)) return -1;
  const dim3 grid((unsigned)((T + 31) / 32), (unsigned)((C + 31) / 32), (unsigned)B);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == VQX_BF16)
    hipLaunchKernelGGL(ntc_to_nct_gather_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)y, (int64_t)ldy, C, T, src_t, x_nct);
  else
    hipLaunchKernelGGL(ntc_to_nct_gather_kernel<float>, grid, dim3(256), 0, s, (const float*)y, (int64_t)ldy, C, T, src_t, x_nct);
  return launch_status(who);
}

extern "C" int vqx_nct_to_ntc_keep(const float* g_nct, int32_t B, int32_t C, int32_t T, const int32_t* src_t, void* y,
                                   int32_t ldy, int32_t dtype, vqx_stream_t stream) {
  const char* who = "vqx_nct_to_ntc_keep";
  if (jitter_layout_check(who, g_nct, y, B, C, T, ldy, dtype)) return -1;
  const dim3 grid((unsigned)((T + 31) / 32), (unsigned)((C + 31) / 32), (unsigned)B);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == VQX_BF16)
    hipLaunchKernelGGL(nct_to_ntc_keep_kernel<bf16_t>, grid, dim3(256), 0, s, g_nct, C, T, src_t, (bf16_t*)y, (int64_t)ldy);
  else
    hipLaunchKernelGGL(nct_to_ntc_keep_kernel<float>, grid, dim3(256), 0, s, g_nct, C, T, src_t, (float*)y, (int64_t)ldy);
  return launch_status(who);
}

extern "C" int vqx_time_gather(const void* x, void* y, int32_t B, int32_t T, int32_t C, const int32_t* src_t,
                               int32_t dtype, vqx_stream_t stream) {
  if ((int64_t)B * T * C >= (1LL << 31)) { set_error("vqx_time_gather: B*T*C must be < 2^31"); return -1; }
  const int grid = grid_for((int64_t)B * T * C);
  if (dtype == VQX_BF16)
    hipLaunchKernelGGL(time_gather_kernel<bf16_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (bf16_t*)y, B, T, C, src_t);
  else
    hipLaunchKernelGGL(time_gather_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)x, (float*)y, B, T, C, src_t);
  return launch_status("vqx_time_gather");
}

// the 8-element chunk path when the shapes allow it (see map8_kernel); false: not taken
static bool map8_launch(const void* src, int32_t lds, int32_t sdt, void* dst, int32_t ldd, int32_t ddt, int64_t rows,
                        int32_t cols, float scale, int32_t act, hipStream_t s, void* zdst = nullptr, int32_t ldz = 0,
                        int64_t zrows = 0, int32_t zcols = 0) {
  if (cols % 8 || ldd % 8 || (src && lds % 8) || (rows * cols + zrows * zcols) / 8 >= (int64_t)1 << 31 ||
      ((uintptr_t)dst & 15) || ((uintptr_t)src & 15) || (zdst && (zcols % 8 || ldz % 8 || ((uintptr_t)zdst & 15))))
    return false;
  const int n8 = (int)(rows * cols / 8), cpr = cols / 8;
  const int n8z = zdst ? (int)(zrows * zcols / 8) : 0, cprz = zdst ? zcols / 8 : 1;
  const int grid = grid_for(n8 + n8z, 256, 2048);
  const bool sb = sdt == VQX_BF16, db = ddt == VQX_BF16;
  if (!src) {
    if (db) hipLaunchKernelGGL((map8_kernel<float, bf16_t, true>), dim3(grid), dim3(256), 0, s, nullptr, 0, (bf16_t*)dst, ldd, n8, cpr, 1.f, 0, (bf16_t*)zdst, ldz, n8z, cprz);
    else hipLaunchKernelGGL((map8_kernel<float, float, true>), dim3(grid), dim3(256), 0, s, nullptr, 0, (float*)dst, ldd, n8, cpr, 1.f, 0, (float*)zdst, ldz, n8z, cprz);
  } else if (sb && db) {
    hipLaunchKernelGGL((map8_kernel<bf16_t, bf16_t, false>), dim3(grid), dim3(256), 0, s, (const bf16_t*)src, lds, (bf16_t*)dst, ldd, n8, cpr, scale, act, (bf16_t*)zdst, ldz, n8z, cprz);
  } else if (sb) {
    hipLaunchKernelGGL((map8_kernel<bf16_t, float, false>), dim3(grid), dim3(256), 0, s, (const bf16_t*)src, lds, (float*)dst, ldd, n8, cpr, scale, act, (float*)zdst, ldz, n8z, cprz);
  } else if (db) {
    hipLaunchKernelGGL((map8_kernel<float, bf16_t, false>), dim3(grid), dim3(256), 0, s, (const float*)src, lds, (bf16_t*)dst, ldd, n8, cpr, scale, act, (bf16_t*)zdst, ldz, n8z, cprz);
  } else {
    hipLaunchKernelGGL((map8_kernel<float, float, false>), dim3(grid), dim3(256), 0, s, (const float*)src, lds, (float*)dst, ldd, n8, cpr, scale, act, (float*)zdst, ldz, n8z, cprz);
  }
  return true;
}

extern "C" int vqx_scale_act_2d(const void* src, int32_t ld_src, int32_t src_dtype, void* dst, int32_t ld_dst,
                                int32_t dst_dtype, int64_t rows, int32_t cols, float scale, int32_t act,
                                vqx_stream_t stream) {
  if (rows <= 0 || cols <= 0) return 0;
  if (!dst || !src) { set_error("vqx_scale_act_2d: null pointer"); return -1; }
  if (map8_launch(src, ld_src, src_dtype, dst, ld_dst, dst_dtype, rows, cols, scale, act, (hipStream_t)stream))
    return launch_status("vqx_scale_act_2d");
  hipLaunchKernelGGL(scale_act_2d_kernel, dim3(grid_for(rows * cols, 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                     src, ld_src, src_dtype, dst, ld_dst, dst_dtype, rows, cols, scale, act);
  return launch_status("vqx_scale_act_2d");
}

extern "C" int vqx_convert_2d(const void* src, int32_t ld_src, int32_t src_dtype, void* dst, int32_t ld_dst,
                              int32_t dst_dtype, int64_t rows, int32_t cols, vqx_stream_t stream) {
  if (rows <= 0 || cols <= 0) return 0;
  if (!dst) { set_error("vqx_convert_2d: null dst"); return -1; }
  if (map8_launch(src, ld_src, src_dtype, dst, ld_dst, dst_dtype, rows, cols, 1.f, VQX_PRO_NONE, (hipStream_t)stream))
    return launch_status("vqx_convert_2d");
  hipLaunchKernelGGL(convert_2d_kernel, dim3(grid_for(rows * cols, 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                     src, ld_src, src_dtype, dst, ld_dst, dst_dtype, rows, cols);
  return launch_status("vqx_convert_2d");
}

extern "C" int vqx_convert_2d_zero2(const void* src, int32_t ld_src, int32_t src_dtype, void* dst, int32_t ld_dst,
                                    int32_t dst_dtype, int64_t rows, int32_t cols, void* zero_dst, int32_t ld_zero,
                                    int64_t zero_rows, int32_t zero_cols, vqx_stream_t stream) {
  if (rows <= 0 || cols <= 0 || zero_rows < 0 || zero_cols < 0) { set_error("vqx_convert_2d_zero2: bad shape"); return -1; }
  if (!dst || (!zero_dst && zero_rows * zero_cols)) { set_error("vqx_convert_2d_zero2: null dst"); return -1; }
  hipStream_t s = (hipStream_t)stream;
  if (map8_launch(src, ld_src, src_dtype, dst, ld_dst, dst_dtype, rows, cols, 1.f, VQX_PRO_NONE, s, zero_dst, ld_zero,
                  zero_rows, zero_cols))
    return launch_status("vqx_convert_2d_zero2");
  // unaligned shapes: the two element passes
  const int rc1 = vqx_convert_2d(src, ld_src, src_dtype, dst, ld_dst, dst_dtype, rows, cols, stream);
  if (rc1 || !zero_rows || !zero_cols) return rc1;
  return vqx_convert_2d(nullptr, 0, 0, zero_dst, ld_zero, dst_dtype, zero_rows, zero_cols, stream);
}
