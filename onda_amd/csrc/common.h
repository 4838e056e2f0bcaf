// Shared helpers for the gfx950 kernels of libonda_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "onda_hip.h"

// "f16x2" limb rows (limbs.h: the format and everything that converts to and from it): the second limb is stored times 2^11.
// A measurement build with -DONDA_LIMB2_SCALE=1.f stores it un-scaled (what a single-accumulator kernel would need; DESIGN.md
// section 7, "Next (0)").
#ifndef ONDA_LIMB2_SCALE
#define ONDA_LIMB2_SCALE 2048.f
#endif
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define ONDA_STREAM(s) (reinterpret_cast<hipStream_t>(s))
// Argument check at the top of every entry point.  It also drops any stale error another
// library left in this thread's HIP error slot, so that the hipGetLastError() after our own
// launches reports our launches only.
#define ONDA_REQUIRE(cond)                                                                              \
  do {                                                                                                  \
    (void)hipGetLastError();                                                                            \
    if (!(cond)) {                                                                                      \
      if (getenv("ONDA_DEBUG_REQUIRE")) fprintf(stderr, "onda_hip: %s:%d: requirement failed: %s\n", __FILE__, __LINE__, #cond); \
      return ONDA_EINVAL;                                                                               \
    }                                                                                                   \
  } while (0)
#define ONDA_ALIGNED16(p) ((reinterpret_cast<uintptr_t>(p) & 15u) == 0)
#define ONDA_LAUNCH_RESULT() static_cast<int>(hipGetLastError())

static inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

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
__device__ __forceinline__ f32x4 splat4(float x) { return f32x4{x, x, x, x}; }
__device__ __forceinline__ f32x4 relu4(f32x4 v) {
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = fmaxf(v[q], 0.f);
  return v;
}
// Running max|v| of a pass over four values a step (folded into the tensor's slots at the end of the kernel, below).
__device__ __forceinline__ float max_abs4(float mx, const f32x4 v) {
  return fmaxf(fmaxf(mx, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
}

// Running max|x| of a tensor for the "f16x2" convolutions.  The value lives in ONDA_AMAX_FLOATS device floats
// (all zero before the producer runs), used as ONDA_AMAX_SLOTS slots one 128-byte line apart: L2 serialises
// atomics per line, so the slots are what lets thousands of workgroups fold their maxima without queueing.
// A producer does one atomicMax on the bit pattern (monotonic for non-negative floats) per workgroup
// (tile_amax_publish) or per wave (amax_update); a consumer takes the maximum over the slots (amax_read).
// max is order-independent: the result is deterministic.  Every lane / thread must call these.
constexpr int AMAX_STRIDE = ONDA_AMAX_FLOATS / ONDA_AMAX_SLOTS;
__device__ __forceinline__ void amax_update(float* amax, float m) {
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0 && m > 0.f)
    atomicMax(reinterpret_cast<unsigned*>(amax) + ((blockIdx.x * 4 + (threadIdx.x >> 6)) & (ONDA_AMAX_SLOTS - 1)) * AMAX_STRIDE,
              __float_as_uint(m));
}
// max of N floats as a balanced tree: for N = 4 the expression fmaxf(fmaxf(v0, v1), fmaxf(v2, v3)) the 256-thread kernels have
// always had (a left-to-right loop gives them other code), the same shape for 8
template <int N>
__device__ __forceinline__ float max_of(const float* v) {
  if constexpr (N == 1) return v[0];
  else return fmaxf(max_of<N / 2>(v), max_of<N - N / 2>(v + N / 2));
}
// one atomic per workgroup of NW waves (4: the 256-thread kernels); `red`: NW floats of LDS
template <int NW = 4>
__device__ __forceinline__ void tile_amax_publish(float* amax, float m, float* red) {
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = max_of<NW>(red);
    if (m > 0.f)
      atomicMax(reinterpret_cast<unsigned*>(amax) + (blockIdx.x & (ONDA_AMAX_SLOTS - 1)) * AMAX_STRIDE, __float_as_uint(m));
  }
}
__device__ __forceinline__ float amax_read(const float* __restrict__ amax) {
  static_assert(ONDA_AMAX_SLOTS == 64, "one slot per lane");
  return wave_max(amax[(threadIdx.x & 63) * AMAX_STRIDE]);
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Sum over the 256 threads of a block; result valid in thread 0. `red` holds >= 4 floats.
__device__ __forceinline__ float block_sum_256(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// Multi-tensor launches are FLAT: entry i of a table in device memory owns the workgroups [first_block_i, first_block_{i+1}) of
// one 1-D grid.  The entry that owns workgroup `block` = the largest i with table[i].first_block <= block, by bisection.  The
// block starts go to LDS first (one load per thread): ten dependent global loads per workgroup were most of a 16 KB
// workgroup's life.
template <class E>
__device__ __forceinline__ int mt_entry_of(const E* __restrict__ table, int n, int block) {
  __shared__ int starts[1024];
  const bool in_lds = n <= 1024;
  if (in_lds) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) starts[i] = table[i].first_block;
    __syncthreads();
  }
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((in_lds ? starts[mid] : table[mid].first_block) <= block) lo = mid; else hi = mid - 1;
  }
  return lo;
}
