// ADVENT's discriminator convolutions (4 x 4 / stride 2 / pad 1) on the pre-split conv kernels: the two rearrangement passes.
//
// A 4 x 4 / stride 2 / pad 1 convolution of x[B,H,W,C] is a 2 x 2 / stride 1 / pad 0 convolution of the space-to-depth view of
// the zero-padded input,
//     S[b, i, j, (py*2 + px)*C + c] = xpad[b, 2i + py, 2j + px, c] = x[b, 2i + py - 1, 2j + px - 1, c]   (0 outside the image),
// with Hs = H/2 + 1 rows and Ws = W/2 + 1 columns (integer division): output row o reads S rows o and o + 1, so Hs = Ho + 1 rows
// are all the forward pass touches (for odd H the padded image has one more row pair, which holds the bottom border only and
// which no output reads; it is not written).  The rearranged weight is w2[o, a, b, (py*2 + px)*C + c] = w[o, c, 2a + py, 2b + px].
// Forward, data gradient and weight gradient of that 2 x 2 convolution are the library's stride-1 kernels (conv_l2.hip); the
// operand of a pre-split convolution has to be written as limb rows by some pass anyway, and these two kernels are that pass:
//
//   s2d_split_kernel   fp32 activation (NCHW: the entropy map; NHWC: the previous conv's output) -> [LeakyReLU] -> border +
//                      space-to-depth -> limb rows S[B*Hs*Ws][Cp/32][2][32] f16, Cp = 4C rounded up to 32 (zeros above 4C).
//                      Scale: a BOUND, not a reduction -- `amax` holds max|x| of the source, and with |slope| <= 1 that bounds
//                      max|LeakyReLU(x)| and therefore max|S| (S holds copies of those values and zeros).
//   d2s_bwd_kernel     the way back: fp32 gradient of S (what the stride-1 data gradient wrote) -> drop the border -> times the
//                      LeakyReLU derivative (1 where the forward input was > 0, slope elsewhere, x == 0 included) -> the
//                      gradient of x as limb rows [B*H*W][C/32][2][32] (operand of the layer below's data / weight gradient)
//                      and / or fp32 (NHWC: the bias gradient's column sum reads it; NCHW: layer 0, what the entropy map's
//                      backward consumes).  Limb scale: again a bound -- `gamax` is max|dS| as the data-gradient conv's
//                      epilogue left it, and |derivative| <= 1; the limb rows' max travels as that buffer.
//
// Both are gather kernels bound by memory: every thread of the NHWC forms moves 8 channels -- two 16-byte loads, and per limb one
// 16-byte store (limb rows: 8 f16 of limb 1, and 8 f16 of limb 2 64 bytes further) -- and neighbouring threads take neighbouring
// 8-channel pieces of one pixel, so a wave reads and writes whole 128-byte lines.
// The NCHW forms (layer 0: 19 planes H*W floats apart) run with the COLUMN as the fastest thread index instead:
//   forward  -- one thread per (b, i, 8-channel piece, j); for each of its 8 values the 64 lanes of a wave read one plane's row
//               at columns 2j + px - 1: every second float of a contiguous run, and the other px of the same piece (another of
//               the thread's 8 values) takes the floats in between, so every 64-byte sector fetched is used in full; the
//               16-byte stores of a wave lie Cp * 4 bytes apart (one per pixel) and the eight stores that complete a 128-byte
//               line come from the same workgroup a few iterations apart (L2 merges them);
//   backward -- one thread per (b, y, c, x), x fastest: 4-byte stores that cover a plane's row contiguously; the loads walk one
//               S row pair per image row (2 * Ws * Cp * 4 bytes, read by all C channels in turn: it stays in L2).
#include "limbs.h"

namespace {

// 8 scaled values -> 8 first limbs at o, 8 second limbs LIMB2_OFS further
__device__ __forceinline__ void store_limbs8(_Float16* o, const float (&v)[8]) {
  u32x4 l1, l2;
  split8(v, l1, l2);
  *reinterpret_cast<u32x4*>(o) = l1;
  *reinterpret_cast<u32x4*>(o + LIMB2_OFS) = l2;
}

struct DiscGeom {
  int B, C, H, W, Hs, Ws, Cp, ldx;
  float slope;  // LeakyReLU slope of the forward input; 1 = no activation
};

template <bool NCHW>
__global__ __launch_bounds__(256) void s2d_split_kernel(const float* __restrict__ x, DiscGeom g, const float* __restrict__ amax,
                                                        _Float16* __restrict__ dst) {
  const float s = scale_of(amax).s;
  const int c8 = g.Cp >> 3, C4 = 4 * g.C;
  const long long n = (long long)g.B * g.Hs * g.Ws * c8;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    int j, chunk;
    long long bi;  // b * Hs + i
    if (NCHW) {  // (b, i, piece, j), j fastest
      j = (int)(e % g.Ws);
      const long long q = e / g.Ws;
      chunk = (int)(q % c8);
      bi = q / c8;
    } else {  // (b, i, j, piece), piece fastest
      chunk = (int)(e % c8);
      const long long q = e / c8;
      j = (int)(q % g.Ws);
      bi = q / g.Ws;
    }
    const int i = (int)(bi % g.Hs), b = (int)(bi / g.Hs), k0 = chunk * 8;
    float v[8];
    if (NCHW) {
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int k = k0 + t, p = k / g.C, c = k - p * g.C;
        const int y = 2 * i + (p >> 1) - 1, xx = 2 * j + (p & 1) - 1;
        const bool ok = k < C4 && (unsigned)y < (unsigned)g.H && (unsigned)xx < (unsigned)g.W;
        v[t] = ok ? x[(((size_t)b * g.C + c) * g.H + y) * g.W + xx] : 0.f;
      }
    } else {  // C % 8 == 0: the 8 channels belong to one parity and one pixel
      const int p = k0 / g.C, c = k0 - p * g.C;
      const int y = 2 * i + (p >> 1) - 1, xx = 2 * j + (p & 1) - 1;
      f32x4 a = {0.f, 0.f, 0.f, 0.f}, bb = a;
      if (k0 < C4 && (unsigned)y < (unsigned)g.H && (unsigned)xx < (unsigned)g.W) {
        const float* src = x + (((size_t)b * g.H + y) * g.W + xx) * g.ldx + c;
        a = *reinterpret_cast<const f32x4*>(src);
        bb = *reinterpret_cast<const f32x4*>(src + 4);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        v[t] = a[t];
        v[4 + t] = bb[t];
      }
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = (v[t] > 0.f ? v[t] : v[t] * g.slope) * s;
    store_limbs8(dst + limb_at((size_t)(bi * g.Ws + j), k0, g.Cp), v);
  }
}

// NHWC: gs[B*Hs*Ws][Cp] -> gradient of x[B,H,W,C] as limb rows (dl, may be null) and / or fp32 NHWC (df, may be null)
__global__ __launch_bounds__(256) void d2s_bwd_nhwc_kernel(const float* __restrict__ gs, const float* __restrict__ gamax,
                                                           const float* __restrict__ x, DiscGeom g, _Float16* __restrict__ dl,
                                                           float* __restrict__ df) {
  const float s = dl != nullptr ? scale_of(gamax).s : 1.f;
  const int c8 = g.C >> 3;
  const long long n = (long long)g.B * g.H * g.W * c8;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    const int c = (int)(e % c8) * 8;
    const long long pix = e / c8;  // (b * H + y) * W + xx
    const int xx = (int)(pix % g.W);
    const long long by = pix / g.W;
    const int y = (int)(by % g.H), b = (int)(by / g.H);
    const int yp = y + 1, xp = xx + 1;  // position in the padded image: S row yp / 2, parity yp % 2
    const float* src = gs + (((size_t)b * g.Hs + (yp >> 1)) * g.Ws + (xp >> 1)) * g.Cp + ((yp & 1) * 2 + (xp & 1)) * g.C + c;
    const f32x4 a = *reinterpret_cast<const f32x4*>(src), bb = *reinterpret_cast<const f32x4*>(src + 4);
    float v[8];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      v[t] = a[t];
      v[4 + t] = bb[t];
    }
    if (x != nullptr) {
      const f32x4 xa = *reinterpret_cast<const f32x4*>(x + (size_t)pix * g.ldx + c);
      const f32x4 xb = *reinterpret_cast<const f32x4*>(x + (size_t)pix * g.ldx + c + 4);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        v[t] = xa[t] > 0.f ? v[t] : v[t] * g.slope;
        v[4 + t] = xb[t] > 0.f ? v[4 + t] : v[4 + t] * g.slope;
      }
    }
    if (df != nullptr) {
      *reinterpret_cast<f32x4*>(df + (size_t)pix * g.C + c) = f32x4{v[0], v[1], v[2], v[3]};
      *reinterpret_cast<f32x4*>(df + (size_t)pix * g.C + c + 4) = f32x4{v[4], v[5], v[6], v[7]};
    }
    if (dl != nullptr) {
#pragma unroll
      for (int t = 0; t < 8; ++t) v[t] *= s;
      store_limbs8(dl + limb_at((size_t)pix, c, g.C), v);
    }
  }
}

// NCHW (layer 0): gs[B*Hs*Ws][Cp] -> df[B,C,H,W] fp32; x (NCHW, may be null): the forward input under a LeakyReLU
__global__ __launch_bounds__(256) void d2s_bwd_nchw_kernel(const float* __restrict__ gs, const float* __restrict__ x, DiscGeom g,
                                                           float* __restrict__ df) {
  const long long n = (long long)g.B * g.H * g.C * g.W;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    const int xx = (int)(e % g.W);
    long long q = e / g.W;
    const int c = (int)(q % g.C);
    q /= g.C;
    const int y = (int)(q % g.H), b = (int)(q / g.H);
    const int yp = y + 1, xp = xx + 1;
    float v = gs[(((size_t)b * g.Hs + (yp >> 1)) * g.Ws + (xp >> 1)) * g.Cp + ((yp & 1) * 2 + (xp & 1)) * g.C + c];
    const size_t o = (((size_t)b * g.C + c) * g.H + y) * g.W + xx;
    if (x != nullptr) v = x[o] > 0.f ? v : v * g.slope;
    df[o] = v;
  }
}

bool disc_geom(DiscGeom& g, int B, int C, int H, int W, int ldx, float slope) {
  if (!(B > 0 && C > 0 && H >= 2 && W >= 2 && C <= (1 << 20))) return false;
  if (!(slope == slope) || !(slope >= -1.f && slope <= 1.f)) return false;  // finite, and |slope| <= 1: the scales are bounds
  g.B = B; g.C = C; g.H = H; g.W = W; g.ldx = ldx; g.slope = slope;
  g.Hs = H / 2 + 1;
  g.Ws = W / 2 + 1;
  g.Cp = (4 * C + 31) / 32 * 32;
  return (long long)B * g.Hs * g.Ws < (1ll << 31) && (long long)B * H * W < (1ll << 31);
}

int grid_for(long long n) {
  const long long b = (n + 256 * 4 - 1) / (256 * 4);
  return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}

}  // namespace

extern "C" {

int onda_s2d_split_h2(const float* x, int nchw, int B, int C, int H, int W, int ldx, float slope, const float* amax, void* dst,
                      onda_stream_t s) {
  DiscGeom g;
  ONDA_REQUIRE(x && amax && dst && disc_geom(g, B, C, H, W, ldx, slope));
  ONDA_REQUIRE(nchw || (C % 8 == 0 && ldx >= C && ldx % 4 == 0));
  if (!ONDA_ALIGNED16(dst) || (!nchw && !ONDA_ALIGNED16(x)) || (nchw && (reinterpret_cast<uintptr_t>(x) & 3u))) return ONDA_EALIGN;
  const long long n = (long long)B * g.Hs * g.Ws * (g.Cp / 8);
  if (nchw)
    hipLaunchKernelGGL(s2d_split_kernel<true>, dim3(grid_for(n)), dim3(256), 0, ONDA_STREAM(s), x, g, amax, static_cast<_Float16*>(dst));
  else
    hipLaunchKernelGGL(s2d_split_kernel<false>, dim3(grid_for(n)), dim3(256), 0, ONDA_STREAM(s), x, g, amax, static_cast<_Float16*>(dst));
  return ONDA_LAUNCH_RESULT();
}

int onda_d2s_bwd(const float* gs, const float* gamax, const float* x, int nchw, int B, int C, int H, int W, int ldx, float slope,
                 void* dst_limbs, float* dst_f32, onda_stream_t s) {
  DiscGeom g;
  ONDA_REQUIRE(gs && (dst_limbs || dst_f32) && disc_geom(g, B, C, H, W, ldx, slope));
  if (nchw) {
    ONDA_REQUIRE(dst_f32 && !dst_limbs);
    if ((reinterpret_cast<uintptr_t>(gs) & 3u) || (reinterpret_cast<uintptr_t>(dst_f32) & 3u) || (reinterpret_cast<uintptr_t>(x) & 3u))
      return ONDA_EALIGN;
    hipLaunchKernelGGL(d2s_bwd_nchw_kernel, dim3(grid_for((long long)B * C * H * W)), dim3(256), 0, ONDA_STREAM(s), gs, x, g, dst_f32);
    return ONDA_LAUNCH_RESULT();
  }
  ONDA_REQUIRE(C % 8 == 0 && (!x || (ldx >= C && ldx % 4 == 0)) && (!dst_limbs || (gamax && C % 32 == 0)));
  if (!ONDA_ALIGNED16(gs) || (x && !ONDA_ALIGNED16(x)) || (dst_limbs && !ONDA_ALIGNED16(dst_limbs)) ||
      (dst_f32 && !ONDA_ALIGNED16(dst_f32)))
    return ONDA_EALIGN;
  hipLaunchKernelGGL(d2s_bwd_nhwc_kernel, dim3(grid_for((long long)B * H * W * (C / 8))), dim3(256), 0, ONDA_STREAM(s), gs, gamax, x,
                     g, static_cast<_Float16*>(dst_limbs), dst_f32);
  return ONDA_LAUNCH_RESULT();
}

}  // extern "C"
