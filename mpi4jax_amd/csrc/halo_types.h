// Element <-> accumulate-type conversions of the typed halo kernels
// (halo.hip: halo_adjoint_acc_kernel; stencil.hip: halo_stencil_kernel).
// float16 / bfloat16 are accumulated in float32 and rounded once, to
// nearest even, at the store.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

struct Bf16 {
  uint16_t bits;
};

template <typename T, typename Acc>
__device__ inline Acc adj_load(const T* p) {
  return (Acc)*p;
}
template <>
__device__ inline float adj_load<Bf16, float>(const Bf16* p) {
  return __uint_as_float((uint32_t)p->bits << 16);
}

template <typename T, typename Acc>
__device__ inline void adj_store(T* p, Acc v) {
  *p = (T)v;  // float -> _Float16 rounds to nearest even
}
template <>
__device__ inline void adj_store<Bf16, float>(Bf16* p, float v) {
  uint32_t u = __float_as_uint(v);
  if ((u & 0x7fffffffu) > 0x7f800000u) {
    p->bits = 0x7fc0;  // NaN
  } else {
    u += 0x7fffu + ((u >> 16) & 1u);  // round to nearest even
    p->bits = (uint16_t)(u >> 16);
  }
}
