// The LIMB FORMAT, once: how an fp32 tensor lies in memory as an operand of the pre-split "f16x2" convolutions (conv_l2.hip),
// and the only code that converts to and from it.  Every producer (weight packers, split_h2, the stem's patch kernel,
// BatchNorm apply / backward, the conv limb epilogues, max-pool, SE gate, the discriminators' rearrangement passes) and every
// consumer goes through the helpers below; nothing else in csrc/ derives a scale or rounds to f16.
//
// fp32-accurate convolution on the f16 matrix pipe with TWO limbs: half the MFMA work of the three-limb bf16 split (round 1,
// retired: `git show c558d15:onda_amd/csrc/conv_bf3.hip`), which matters because that kernel is bound by a power-managed
// clock, not by issue slots or operand delivery.
//
//   x * s = h1 + h2 + e,   h1 = f16(x * s), h2 = f16(x * s - h1),   |e| <= 2^-22 |x * s|  (or <= 2^-25 absolute)
//
// with s a power of two per TENSOR chosen so that the largest |x * s| lies in [2^14, 2^15) (f16 tops out at 65504): f16 has 11
// significant bits but only 5 exponent bits, so unlike bf16 it needs the scale; a power of two keeps the scaling exact, and a
// per-tensor factor comes out of the whole contraction (a per-pixel one would not: an im2col row mixes pixels).  The second
// limb is stored times 2^11 (the residual of an f16 rounding is <= 2^-11 of the first limb), so both limbs keep 11 significant
// bits for every element down to 2^-28 of the tensor maximum; below that the limbs slide into f16 subnormals (nothing is
// flushed) and precision falls off gradually.  Measured on outputs that depend ONLY on small elements (a pixel far below the
// largest one, through a 1x1 conv; tests/test_hip_kernels.py::test_f16x2_interpixel_range): 1.3e-7 down to 2^-24 of the
// maximum, 6e-7 at 2^-28, 1e-5 at 2^-32 -- 7-8 decades of per-element range at full accuracy, against fp32's own 2^-126; the
// retired "bf16x3" mode had no such dependence.
// The product is evaluated as a1*b1 + (a1*b2 + a2*b1), each exact in fp32 (11 x 11 bits), accumulated in fp32 by
// v_mfma_f32_16x16x32_f16 -- a1*b1 in one accumulator set, the two cross products (2^11 too large) in a second one that is
// folded in with 2^-11 at the end; what is dropped (a2*b2 and the representation error) is ~2^-22 |a||b| per product.
// Measured on the GPU: 1.3-3e-7 relative L2 against fp64, where fp32 FMA chains give 3e-7 and the bf16x3 kernels 0.7-2.4e-7.
#pragma once
#include "common.h"

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// The second limb is stored times LIMB2_SCALE, so that it lives in the first limb's own exponent range instead of sliding into
// f16 subnormals for small elements; the cross products then carry that factor, live in accumulators of their own and are
// folded in with LIMB2_UNSCALE (exact).  The factor itself: ONDA_LIMB2_SCALE, common.h.
constexpr float LIMB2_SCALE = ONDA_LIMB2_SCALE, LIMB2_UNSCALE = 1.f / ONDA_LIMB2_SCALE;

// LIMB ROWS (round 5): how an operand of the pre-split convolutions lies in memory.  Row r -- a pixel of an activation, an
// output channel of a packed weight -- holds, for every block of 32 channels, the 32 FIRST limbs followed by the 32 SECOND
// limbs: 128 bytes = one cache line per (row, K-step of 32 channels).  Until round 4 the two limbs were separate planes
// ([2][rows][ld]); a K-step then fetched two HALF lines per row, and tools/micro/dma_rate.hip shows what that costs: the
// convolutions' LDS-DMA stream alone (no MFMA, no fragment read) takes as long as the whole 1024 -> 256 1x1 kernel, bound
// by cache-line REQUESTS per CU, and runs 22-30 % faster with the same bytes as whole lines.
//   f16 index of (row r, channel c, first limb) = r * 2 * ld + (c / 32) * 64 + c % 32;  second limb: + LIMB2_OFS
// ld = channels per row (a multiple of 32); a row is 2 * ld f16 = 4 * ld bytes, like an fp32 row.
constexpr int LIMB2_OFS = 32;
__host__ __device__ __forceinline__ size_t limb_at(size_t row, int c, int ld) {
  return row * 2 * (size_t)ld + (size_t)((c >> 5) << 6) + (size_t)(c & 31);
}

// ---- per-tensor scale --------------------------------------------------------------------------
// A tensor's scale travels as its max|x| (or an a-priori bound of it) in ONDA_AMAX_FLOATS device floats, written by the kernel
// that produced the tensor or by absmax_kernel (common.h amax_update / amax_read) -- no finalisation kernel, no host round
// trip.  Every producer and consumer derives s = 2^e, 1/s = 2^-e with max * 2^e in [2^14, 2^15) from it HERE: a few loads and
// scalar operations per wave.  An all-zero (or non-finite) tensor gets e = 0.
struct Scale2 {
  float s, inv;
};
__device__ __forceinline__ Scale2 scale_from(const float m) {
  int e = 0;
  if (m > 0.f && m < 3.0e38f) {
    int ex;
    frexpf(m, &ex);  // m = f * 2^ex, f in [0.5, 1)
    e = 15 - ex;
    e = e > 100 ? 100 : (e < -100 ? -100 : e);
  }
  return Scale2{ldexpf(1.f, e), ldexpf(1.f, -e)};
}
__device__ __forceinline__ Scale2 scale_of(const float* __restrict__ amax) { return scale_from(amax_read(amax)); }

// ---- split: scaled fp32 -> two limbs ------------------------------------------------------------
// two floats -> two f16 (round to nearest even) in one dword, and back
__device__ __forceinline__ unsigned cvt2h(float lo, float hi) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{lo, hi}, f16x2));
}
__device__ __forceinline__ f32x2 unpack2h(unsigned p) {
  return __builtin_convertvector(__builtin_bit_cast(f16x2, p), f32x2);
}
// second limbs of a pair, given its first limbs (a site that stores the first limbs before it goes on keeps that order)
__device__ __forceinline__ unsigned cvt2h_rest(float a, float b, unsigned l1) {
  const f32x2 f = unpack2h(l1);
  return cvt2h((a - f[0]) * LIMB2_SCALE, (b - f[1]) * LIMB2_SCALE);
}
// a pair of neighbouring elements: one dword per limb
struct LimbPair {
  unsigned l1, l2;
};
__device__ __forceinline__ LimbPair split2(float a, float b) {
  const unsigned p = cvt2h(a, b);
  return LimbPair{p, cvt2h_rest(a, b, p)};
}
// The widths the kernels use, on top of the pair.  They fill local vectors and assign them whole (element writes through a
// reference come out as other shuffles).  Two sites call split2 in a loop of their own instead -- the stem's patch kernel
// (conv_l2.hip) and max-pool (pointwise.hip): a helper is simplified on its own before it is inlined, its loop is gone by
// then, and the instruction order of those two kernels depends on the loop being theirs (same values, other assembly:
// docs/experiments.md, "The limb format, once").
// 4 scaled floats -> 4 + 4 f16 (8 bytes per limb)
__device__ __forceinline__ void split4(const f32x4 v, u32x2& l1, u32x2& l2) {
  u32x2 a, b;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const LimbPair p = split2(v[2 * h], v[2 * h + 1]);
    a[h] = p.l1;
    b[h] = p.l2;
  }
  l1 = a;
  l2 = b;
}
// 8 scaled floats -> 8 + 8 f16 (16 bytes per limb)
__device__ __forceinline__ void split8(const float (&v)[8], u32x4& l1, u32x4& l2) {
  u32x4 a, b;
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const LimbPair p = split2(v[2 * h], v[2 * h + 1]);
    a[h] = p.l1;
    b[h] = p.l2;
  }
  l1 = a;
  l2 = b;
}
__device__ __forceinline__ void split8(const f32x4 v0, const f32x4 v1, u32x4& l1, u32x4& l2) {
  const float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
  split8(v, l1, l2);
}
// one element (the element-per-thread weight packers): its first limb, and its second limb given the first
__device__ __forceinline__ _Float16 limb1(float v) { return (_Float16)v; }
__device__ __forceinline__ _Float16 limb2(float v, _Float16 l1) { return (_Float16)((v - (float)l1) * LIMB2_SCALE); }

// ---- join: two limbs -> fp32 (still scaled) -------------------------------------------------------
__device__ __forceinline__ f32x4 join4(const u32x2 l1, const u32x2 l2) {
  f32x4 v;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const f32x2 a = unpack2h(l1[h]), b = unpack2h(l2[h]);
    v[2 * h] = a[0] + b[0] * LIMB2_UNSCALE;
    v[2 * h + 1] = a[1] + b[1] * LIMB2_UNSCALE;
  }
  return v;
}
__device__ __forceinline__ void join8(const u32x4 l1, const u32x4 l2, f32x4& v0, f32x4& v1) {
  v0 = join4(u32x2{l1[0], l1[1]}, u32x2{l2[0], l2[1]});
  v1 = join4(u32x2{l1[2], l1[3]}, u32x2{l2[2], l2[3]});
}
