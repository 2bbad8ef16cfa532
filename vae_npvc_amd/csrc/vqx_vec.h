// Vector-access helpers of the element-wise kernels.  Used by vqx_gn.hip, vqx_reduce.hip, vqx_loss.hip and vqx_layout.hip.
#pragma once
#include "vqx_common.h"

namespace vqx {

// Vec<T>: a 16-byte chunk (8 bf16 or 4 f32)
template <typename T> struct Vec;
template <> struct Vec<bf16_t> {
  static constexpr int N = 8;
  typedef uint4 raw_t;  // the 16-B chunk as loaded (cvt: to floats where they are used)
  __device__ static __forceinline__ raw_t ld(const bf16_t* p) { return *(const uint4*)p; }
  __device__ static __forceinline__ void cvt(const raw_t& u, float* f) {
    const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { f[2 * i] = __uint_as_float(w[i] << 16); f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
  }
  __device__ static __forceinline__ void load(const bf16_t* p, float* f) { cvt(ld(p), f); }
  __device__ static __forceinline__ void store(bf16_t* p, const float* f) {
    unsigned w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = pack_bf16x2(f[2 * i], f[2 * i + 1]);
    *(uint4*)p = make_uint4(w[0], w[1], w[2], w[3]);
  }
};
template <> struct Vec<float> {
  static constexpr int N = 4;
  typedef f32x4_t raw_t;
  __device__ static __forceinline__ raw_t ld(const float* p) { return *(const f32x4_t*)p; }
  __device__ static __forceinline__ void cvt(const raw_t& v, float* f) { f[0] = v[0]; f[1] = v[1]; f[2] = v[2]; f[3] = v[3]; }
  __device__ static __forceinline__ void load(const float* p, float* f) { cvt(ld(p), f); }
  __device__ static __forceinline__ void store(float* p, const float* f) {
    f32x4_t v = {f[0], f[1], f[2], f[3]};
    *(f32x4_t*)p = v;
  }
};

// Vec4<T>: 4 elements (8 B of bf16 or 16 B of f32)
template <typename T> struct Vec4;
template <> struct Vec4<bf16_t> {
  typedef uint2 raw_t;
  __device__ static __forceinline__ raw_t ld(const bf16_t* p) { return *(const uint2*)p; }
  __device__ static __forceinline__ void cvt(const raw_t& u, float* f) {
    f[0] = __uint_as_float(u.x << 16); f[1] = __uint_as_float(u.x & 0xffff0000u);
    f[2] = __uint_as_float(u.y << 16); f[3] = __uint_as_float(u.y & 0xffff0000u);
  }
  __device__ static __forceinline__ void load(const bf16_t* p, float* f) { cvt(ld(p), f); }
  __device__ static __forceinline__ void store(bf16_t* p, const float* f) {
    *(uint2*)p = make_uint2(pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]));
  }
};
template <> struct Vec4<float> : Vec<float> {};

// Chunk8<T>: 8 elements (16 B of bf16 or 2 x 16 B of f32)
template <typename S> struct Chunk8;
template <> struct Chunk8<float> {
  __device__ static __forceinline__ void ld(const float* p, float* f) {
    const f32x4_t a = *(const f32x4_t*)p, b = *(const f32x4_t*)(p + 4);
    f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3]; f[4] = b[0]; f[5] = b[1]; f[6] = b[2]; f[7] = b[3];
  }
  __device__ static __forceinline__ void st(float* p, const float* f) {
    *(f32x4_t*)p = f32x4_t{f[0], f[1], f[2], f[3]};
    *(f32x4_t*)(p + 4) = f32x4_t{f[4], f[5], f[6], f[7]};
  }
};
template <> struct Chunk8<bf16_t> {
  __device__ static __forceinline__ void ld(const bf16_t* p, float* f) { Vec<bf16_t>::load(p, f); }
  __device__ static __forceinline__ void st(bf16_t* p, const float* f) { Vec<bf16_t>::store(p, f); }
};

}  // namespace vqx
