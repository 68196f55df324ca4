// common.h -- shared host/device helpers for libfhvae_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/fhvae_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16;

#define FH_CHECK_PTR(p) \
  do {                  \
    if ((p) == nullptr) return FHVAE_ERR_NULL; \
  } while (0)
#define FH_CHECK_POS(v) \
  do {                  \
    if ((v) <= 0) return FHVAE_ERR_SHAPE; \
  } while (0)
#define FH_CHECK_I32(v) \
  do {                  \
    if ((v) > 0x7fffffffLL) return FHVAE_ERR_LIMIT; \
  } while (0)

// after a kernel launch: surface launch-configuration errors as positive hipError_t codes
static inline int fh_launch_status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? FHVAE_OK : (int)e;
}

static inline int64_t fh_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- host side of the all-pairs kernels (allpairs_f32.h: disc_mfma.hip, sv.hip, tsne.hip)
// streamed rows per workgroup so that `want` workgroups cover ny rows: whole tiles of 64, at least `min_chunk`.  (How `want`
// follows from the workgroups aimed at differs per caller and stays there: the chunk fixes the grid, the grid the
// layout of the partials and the workspace sizes.)
static inline int64_t fh_allpairs_chunk(int64_t ny, int64_t want, int64_t min_chunk) {
  const int64_t chunk = fh_cdiv(fh_cdiv(ny, want), 64) * 64;
  return chunk < min_chunk ? min_chunk : chunk;
}
// the (rows, D) f32 matrix of an all-pairs call, leading dimension ld
static inline int fh_allpairs_check(const float* x, int64_t ld, int64_t D) {
  if (D < 16 || D > 128 || D % 16 != 0) return FHVAE_ERR_SHAPE;
  if (ld < D) return FHVAE_ERR_SHAPE;
  if (ld % 4 != 0 || ((uintptr_t)x & 15) != 0) return FHVAE_ERR_ALIGN;
  return FHVAE_OK;
}
// f(std::integral_constant<int, D>()) for a checked D = 16, 32 .. 128
template <class F>
static inline int fh_allpairs_dispatch(int64_t D, F f) {
  switch (D) {
    case 16: return f(std::integral_constant<int, 16>());
    case 32: return f(std::integral_constant<int, 32>());
    case 48: return f(std::integral_constant<int, 48>());
    case 64: return f(std::integral_constant<int, 64>());
    case 80: return f(std::integral_constant<int, 80>());
    case 96: return f(std::integral_constant<int, 96>());
    case 112: return f(std::integral_constant<int, 112>());
    default: return f(std::integral_constant<int, 128>());
  }
}

// f32 -> bf16 (round to nearest even; NaN stays NaN via the compiler's cvt)
__device__ __forceinline__ u16 f2bf(float f) {
  __bf16 b = (__bf16)f;
  return __builtin_bit_cast(u16, b);
}
__device__ __forceinline__ float bf2f(u16 h) {
  return __builtin_bit_cast(float, ((uint32_t)h) << 16);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
