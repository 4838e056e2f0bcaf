// HBM-bound pointwise / stencil kernels of the hot path: ceil-mode max-pool, the SE gate,
// channel scaling, align_corners bilinear upsampling (plain, gradient, fused argmax / cross-entropy / calibration / entropy map /
// validation tail).
#include "limbs.h"
#include <type_traits>

namespace {

#define LD4(p) (*reinterpret_cast<const f32x4*>(p))

// ---- MaxPool 3x3 / s2 / p1 / ceil_mode, NHWC -------------------------------------------
// yl != nullptr: the result goes out as LIMB ROWS (the operand format of the convolutions that read it, conv_l2.hip; scale from
// `amax` = max|x|: a maximum over windows of x cannot pass it) instead of fp32 -- no fp32 copy, no split pass behind the pool
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                          uint8_t* __restrict__ idx, int B, int Hi, int Wi, int C,
                                                          int Ho, int Wo, _Float16* __restrict__ yl,
                                                          const float* __restrict__ amax) {
  const int c4 = C / 4;
  float so = 1.f;
  if (yl != nullptr) so = scale_of(amax).s;
  const size_t total = (size_t)B * Ho * Wo * c4;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int col = (int)(e % c4) * 4;
    size_t q = e / c4;
    const int wo = (int)(q % Wo);
    q /= Wo;
    const int ho = (int)(q % Ho), b = (int)(q / Ho);
    f32x4 best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int slot[4] = {0, 0, 0, 0};
    bool first = true;
    for (int r = 0; r < 3; ++r) {
      const int hi = ho * 2 - 1 + r;
      if ((unsigned)hi >= (unsigned)Hi) continue;
      for (int s = 0; s < 3; ++s) {
        const int wi = wo * 2 - 1 + s;
        if ((unsigned)wi >= (unsigned)Wi) continue;
        const f32x4 v = LD4(x + (((size_t)b * Hi + hi) * Wi + wi) * C + col);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          // ATen's scan: strict '>' keeps the first maximum, NaN always wins
          if (first || v[j] > best[j] || v[j] != v[j]) {
            best[j] = v[j];
            slot[j] = r * 3 + s;
          }
        }
        first = false;
      }
    }
    if (yl != nullptr) {
      u32x2 l1, l2;
      const f32x4 w = best * so;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const LimbPair p = split2(w[2 * h], w[2 * h + 1]);
        l1[h] = p.l1;
        l2[h] = p.l2;
      }
      _Float16* o = yl + limb_at(e / c4, col, C);
      *reinterpret_cast<u32x2*>(o) = l1;
      *reinterpret_cast<u32x2*>(o + LIMB2_OFS) = l2;
    } else {
      *reinterpret_cast<f32x4*>(y + e * 4) = best;
    }
    *reinterpret_cast<uint32_t*>(idx + e * 4) =
        (uint32_t)slot[0] | ((uint32_t)slot[1] << 8) | ((uint32_t)slot[2] << 16) | ((uint32_t)slot[3] << 24);
  }
}

__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ idx,
                                                          float* __restrict__ dx, int B, int Hi, int Wi, int C, int Ho,
                                                          int Wo) {
  const int c4 = C / 4;
  const size_t total = (size_t)B * Hi * Wi * c4;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int col = (int)(e % c4) * 4;
    size_t q = e / c4;
    const int wi = (int)(q % Wi);
    q /= Wi;
    const int hi = (int)(q % Hi), b = (int)(q / Hi);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int ho_lo = hi / 2, ho_hi = (hi + 1) / 2;  // windows with 2*ho-1 <= hi <= 2*ho+1
    const int wo_lo = wi / 2, wo_hi = (wi + 1) / 2;
    for (int ho = ho_lo; ho <= ho_hi; ++ho) {
      if (ho >= Ho) continue;
      for (int wo = wo_lo; wo <= wo_hi; ++wo) {
        if (wo >= Wo) continue;
        const int slot = (hi - (ho * 2 - 1)) * 3 + (wi - (wo * 2 - 1));
        const size_t o = (((size_t)b * Ho + ho) * Wo + wo) * C + col;
        const uint32_t pk = *reinterpret_cast<const uint32_t*>(idx + o);
        const f32x4 g = LD4(dy + o);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if ((int)((pk >> (8 * j)) & 0xff) == slot) acc[j] += g[j];
      }
    }
    *reinterpret_cast<f32x4*>(dx + e * 4) = acc;
  }
}

// ---- SE gate -------------------------------------------------------------------------------
// hidden = relu(W1 pooled + b1) (R rows), gate = sigmoid(W2 hidden + b2): two small launches that fill the chip (one wave
// per hidden unit and image; one thread per gate) instead of one workgroup per image walking both layers serially
// (193 us for a 0.8 MB problem).
__global__ __launch_bounds__(256) void se_fc1_kernel(const float* __restrict__ pooled, const float* __restrict__ w1,
                                                     const float* __restrict__ b1, float* __restrict__ hidden, int C, int R) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const float* p = pooled + (size_t)b * C;
  float s = 0.f;
  for (int ch = lane; ch < C; ch += 64) s += w1[(size_t)r * C + ch] * p[ch];  // same order of partial sums as before
  s = wave_sum(s);
  if (lane == 0) hidden[(size_t)b * R + r] = fmaxf(s + b1[r], 0.f);
}

__global__ __launch_bounds__(256) void se_fc2_kernel(const float* __restrict__ hidden, const float* __restrict__ w2,
                                                     const float* __restrict__ b2, float* __restrict__ gate, int C, int R) {
  extern __shared__ float hid[];
  const int b = blockIdx.y, t = threadIdx.x;
  for (int r = t; r < R; r += 256) hid[r] = hidden[(size_t)b * R + r];
  __syncthreads();
  const int ch = blockIdx.x * 256 + t;
  if (ch >= C) return;
  float s = b2[ch];
  for (int r = 0; r < R; ++r) s += w2[(size_t)ch * R + r] * hid[r];
  gate[(size_t)b * C + ch] = 1.f / (1.f + expf(-s));
}

// dpre2[b][c] = dgate*gate*(1-gate);  dw2[c][r] = sum_b dpre2[b][c]*hidden[b][r]; db2[c]
__global__ void se_bwd_w2_kernel(const float* __restrict__ dgate, const float* __restrict__ gate,
                                 const float* __restrict__ hidden, float* __restrict__ dw2, float* __restrict__ db2,
                                 int B, int C, int R) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C * R) return;
  const int ch = i / R, r = i % R;
  float s = 0.f, sb = 0.f;
  for (int b = 0; b < B; ++b) {
    const float g = gate[(size_t)b * C + ch];
    const float d = dgate[(size_t)b * C + ch] * g * (1.f - g);
    s += d * hidden[(size_t)b * R + r];
    sb += d;
  }
  dw2[i] = s;
  if (r == 0) db2[ch] = sb;
}

// dpre1[b][r] = (sum_c dpre2[b][c]*w2[c][r]) * (hidden>0)   -> ws[b][r]
__global__ __launch_bounds__(256) void se_bwd_hidden_kernel(const float* __restrict__ dgate,
                                                            const float* __restrict__ gate,
                                                            const float* __restrict__ hidden,
                                                            const float* __restrict__ w2, float* __restrict__ dpre1,
                                                            int C, int R) {
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int r = wave; r < R; r += 4) {
    float s = 0.f;
    for (int ch = lane; ch < C; ch += 64) {
      const float g = gate[(size_t)b * C + ch];
      s += dgate[(size_t)b * C + ch] * g * (1.f - g) * w2[(size_t)ch * R + r];
    }
    s = wave_sum(s);
    if (lane == 0) dpre1[(size_t)b * R + r] = hidden[(size_t)b * R + r] > 0.f ? s : 0.f;
  }
}

// dw1[r][c] = sum_b dpre1[b][r]*pooled[b][c]; db1[r]; dpooled[b][c] = scale * sum_r dpre1[b][r]*w1[r][c]
__global__ void se_bwd_w1_kernel(const float* __restrict__ dpre1, const float* __restrict__ pooled,
                                 const float* __restrict__ w1, float* __restrict__ dw1, float* __restrict__ db1,
                                 float* __restrict__ dpooled, int B, int C, int R, float scale) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < R * C) {
    const int r = i / C, ch = i % C;
    float s = 0.f, sb = 0.f;
    for (int b = 0; b < B; ++b) {
      s += dpre1[(size_t)b * R + r] * pooled[(size_t)b * C + ch];
      sb += dpre1[(size_t)b * R + r];
    }
    dw1[i] = s;
    if (ch == 0) db1[r] = sb;
  }
  if (i < B * C) {
    const int b = i / C, ch = i % C;
    float s = 0.f;
    for (int r = 0; r < R; ++r) s += dpre1[(size_t)b * R + r] * w1[(size_t)r * C + ch];
    dpooled[i] = s * scale;
  }
}

__global__ __launch_bounds__(256) void chan_scale_kernel(const float* __restrict__ x, const float* __restrict__ gate,
                                                         const float* __restrict__ add, float* __restrict__ out,
                                                         int64_t HW, int C, size_t total4) {
  const int c4 = C / 4;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total4; e += (size_t)gridDim.x * blockDim.x) {
    const int col = (int)(e % c4) * 4;
    const int b = (int)((e / c4) / HW);
    f32x4 v = LD4(x + e * 4) * LD4(gate + (size_t)b * C + col);
    if (add) v += LD4(add + (size_t)b * C + col);
    *reinterpret_cast<f32x4*>(out + e * 4) = v;
  }
}

// ---- bilinear, align_corners=True ----------------------------------------------------------
struct Lerp {
  int i0, i1;
  float l0, l1;
};
__device__ __forceinline__ Lerp lerp_index(int dst, float scale, int in_size) {
#pragma clang fp contract(off)  // the product is rounded before the subtraction below, as in ATen
  const float src = scale * (float)dst;
  Lerp o;
  o.i0 = (int)src;
  o.i1 = o.i0 + (o.i0 < in_size - 1 ? 1 : 0);
  o.l1 = src - (float)o.i0;
  o.l0 = 1.f - o.l1;
  return o;
}

// One output pixel of a [B][H][W] grid over rows[B][h][w][ldl]: where it is, the taps of both axes, the four rows it reads
struct Pixel {
  int b, Y, X;
  Lerp ly, lx;
  const float *p00, *p01, *p10, *p11;
};
__device__ __forceinline__ Pixel pixel_at(size_t e, const float* rows, int ldl, int h, int w, int H, int W, float sy, float sx) {
  Pixel p;
  p.X = (int)(e % W);
  const size_t q = e / W;
  p.Y = (int)(q % H), p.b = (int)(q / H);
  p.ly = lerp_index(p.Y, sy, h), p.lx = lerp_index(p.X, sx, w);
  p.p00 = rows + (((size_t)p.b * h + p.ly.i0) * w + p.lx.i0) * ldl;
  p.p01 = rows + (((size_t)p.b * h + p.ly.i0) * w + p.lx.i1) * ldl;
  p.p10 = rows + (((size_t)p.b * h + p.ly.i1) * w + p.lx.i0) * ldl;
  p.p11 = rows + (((size_t)p.b * h + p.ly.i1) * w + p.lx.i1) * ldl;
  return p;
}

// rows are ldl floats apart; whole 16-byte groups of classes when the padding allows (the head's rows are 32 floats: 5 loads
// per corner for 19 classes instead of 19).  A macro on purpose: as a function the three tests are folded into one block
// before they are inlined and every kernel that asks comes out with other code (docs/experiments.md, 2026-10-18)
#define ROWS_VEC(rows, ldl, K) (((ldl) & 3) == 0 && (((K) + 3) & ~3) <= (ldl) && (reinterpret_cast<uintptr_t>(rows) & 15) == 0)

// the interpolated value from its four corners (a, c: row i0 of y at columns i0, i1 of x; d, f: row i1): every kernel of the
// family takes it from here, so all of them round alike
__device__ __forceinline__ float bilerp(const Lerp& ly, const Lerp& lx, float a, float c, float d, float f) {
  return ly.l0 * (lx.l0 * a + lx.l1 * c) + ly.l1 * (lx.l0 * d + lx.l1 * f);
}

// the four classes k .. k + 3 of a pixel into o[0..4) (without `vec`, those >= K: 0, never looked at)
__device__ __forceinline__ void bilerp4(const Pixel& p, bool vec, int k, int K, float* o) {
  f32x4 a = {0.f, 0.f, 0.f, 0.f}, c = a, d = a, f = a;
  if (vec) {
    a = LD4(p.p00 + k), c = LD4(p.p01 + k), d = LD4(p.p10 + k), f = LD4(p.p11 + k);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (k + j < K) a[j] = p.p00[k + j], c[j] = p.p01[k + j], d[j] = p.p10[k + j], f[j] = p.p11[k + j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = bilerp(p.ly, p.lx, a[j], c[j], d[j], f[j]);
}

constexpr int UCE_KMAX = 32;  // classes the kernels that keep a pixel's whole K-vector in registers take

// m = max of v[0..K), v[k] = exp(v[k] - m) in place; returns the sum (ATen's softmax up to the division)
__device__ __forceinline__ float exp_sum(float* v, int K) {
  float m = -INFINITY, sum = 0.f;
#pragma unroll
  for (int k = 0; k < UCE_KMAX; ++k)
    if (k < K) m = fmaxf(m, v[k]);
#pragma unroll
  for (int k = 0; k < UCE_KMAX; ++k)
    if (k < K) {
      v[k] = expf(v[k] - m);
      sum += v[k];
    }
  return sum;
}

// The confusion matrix (ARGMAX with `hist`) is counted per workgroup in LDS and flushed once: one global atomic per non-empty
// cell and workgroup instead of one per pixel (K * K counters shared by every pixel of the batch: 4.2 M adds to 361 addresses
// took 2.1 of the 20.3 ms of an 8-frame evaluation pass).  Integer adds: the result does not depend on the order.
constexpr int UPS_HIST_LDS = 1024;  // cells a workgroup counts in LDS (K <= 32); larger K: global atomics per pixel

template <class T>
__device__ __forceinline__ void lds_zero(T* p, int n) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) p[i] = 0;
}

// one (ground truth g, prediction arg) pair into the workgroup's LDS counts or straight into `hist`; fast_hist
// (func.py:77-79): rows = ground truth in [0,K), columns = prediction
__device__ __forceinline__ void hist_count(unsigned* lh, unsigned long long* hist, bool local, int g, int arg, int K) {
  if (g < K) {
    if (local) atomicAdd(lh + g * K + arg, 1u);
    else atomicAdd(&hist[g * K + arg], 1ull);
  }
}

// global[0..n) += lds_counts[0..n), after a barrier.  Every workgroup starts its flush at a different cell: the adds of one
// moment go to different addresses
__device__ __forceinline__ void flush_rotated(const unsigned* lds_counts, unsigned long long* global, unsigned n) {
  const unsigned start = (blockIdx.x * 37u) % n;
  for (unsigned i = threadIdx.x; i < n; i += blockDim.x) {
    unsigned cell = i + start;
    if (cell >= n) cell -= n;
    const unsigned long long c = lds_counts[cell];
    if (c) atomicAdd(&global[cell], c);
  }
}

template <bool ARGMAX>
__global__ __launch_bounds__(256) void upsample_kernel(const float* __restrict__ logits, int ldl,
                                                       float* __restrict__ out, uint8_t* __restrict__ cls,
                                                       const uint8_t* __restrict__ gt, unsigned long long* __restrict__ hist,
                                                       int B, int h, int w, int K, int H, int W, float sy, float sx) {
  __shared__ unsigned lh[ARGMAX ? UPS_HIST_LDS : 1];
  const int KK = K * K;
  const bool local = ARGMAX && hist != nullptr && KK <= UPS_HIST_LDS;
  if (local) {
    lds_zero(lh, KK);
    __syncthreads();
  }
  const bool vec = ROWS_VEC(logits, ldl, K);
  const size_t total = (size_t)B * H * W;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const Pixel p = pixel_at(e, logits, ldl, h, w, H, W, sy, sx);
    float best = -INFINITY;
    int arg = 0;
    auto take = [&](int k, float v) {
      if (ARGMAX) {
        if (v > best) {
          best = v;
          arg = k;
        }
      } else {
        out[(((size_t)p.b * K + k) * H + p.Y) * W + p.X] = v;
      }
    };
    if (vec) {
      for (int k = 0; k < K; k += 4) {
        const f32x4 a = LD4(p.p00 + k), c = LD4(p.p01 + k), d = LD4(p.p10 + k), f = LD4(p.p11 + k);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (k + j < K) take(k + j, bilerp(p.ly, p.lx, a[j], c[j], d[j], f[j]));
      }
    } else {
      for (int k = 0; k < K; ++k) take(k, bilerp(p.ly, p.lx, p.p00[k], p.p01[k], p.p10[k], p.p11[k]));
    }
    if (ARGMAX) {
      if (cls) cls[e] = (uint8_t)arg;
      if (hist) hist_count(lh, hist, local, gt[e], arg, K);
    }
  }
  if (local) {
    __syncthreads();
    flush_rotated(lh, hist, KK);
  }
}

// ---- expected calibration error: upsample -> (softmax) -> (confidence, class) -> bin table, one pass ------------------------
// ECE.record(interp(pred).softmax(1), label) (monitoring.py:99-136, adaptation_model.py:145-149) without the upsampled tensor:
// one thread per output pixel interpolates its K values in registers (same weights, same expression, same first-maximum rule
// as upsample_kernel), reduces them to a confidence and a class, and counts into table[bins + 1][3] (int64):
//   [row][0] += round(conf * 2^32)   [row][1] += (class == label)   [row][2] += 1
// row = floor(conf / gap) for the float32 conf and gap (what ATen's fmod-based floor division yields), clamped to
// [0, bins - 1]; a non-finite conf counts (0, 0, 1) into row `bins`.  Every pixel is counted, whatever its label.
// Fixed point: integer adds give the same table for any order and grid.  conf * 2^32 is exact for conf >= 2^-9 (a float has
// 24 bits; the maximum of K <= 255 probabilities is >= 1/255) and rounds to nearest below; |conf| is taken down to 2^30
// first (probs mode accepts any number), so the conversion itself cannot overflow.
constexpr float ECE_FIX = 4294967296.f;      // 2^32: an int64 sum holds 2^31 pixels at conf = 1 (Cityscapes val at 1024x2048: 1.05e9)
constexpr float ECE_CONF_CAP = 1073741824.f; // 2^30
constexpr int ECE_BINS_LDS = 2047;           // bins a workgroup counts in LDS ((bins + 1) * 16 bytes <= 32 KB); more: global atomics
constexpr int ECE_KREG = 32;                 // classes kept in registers between the maximum and the exponentials; more: recomputed

__device__ __forceinline__ int ece_row(float conf, float gap, int bins) {
  if (!(fabsf(conf) <= 3.402823466e38f)) return bins;  // NaN, +-inf
  // correctly rounded division (no fast-math in this build), and bins <= 2^20 (host check), so q < 2^20 is within 2^-4 of the
  // quotient: its floor is off by one at the most
  const float q = conf / gap;
  if (!(q < (float)bins)) return bins - 1;
  if (q < 0.f) return 0;
  int n = (int)q;
  // the sign of conf - n * gap from one rounding of the exact value (monotonic; 0 and gap are floats)
  const float r = fmaf(-(float)n, gap, conf);
  if (r < 0.f) --n;
  else if (r >= gap) ++n;
  return n < 0 ? 0 : (n >= bins ? bins - 1 : n);
}

// LDS: sum[rows] (u64), then per row (correct << 32 | pixels) (u64): a workgroup sees fewer than 2^32 pixels (host check).
template <bool KREG>
__global__ __launch_bounds__(256) void upsample_ece_kernel(const float* __restrict__ rows, int ldl,
                                                           const uint8_t* __restrict__ gt, unsigned long long* __restrict__ table,
                                                           int bins, float gap, int probs, unsigned long long* __restrict__ hist,
                                                           int B, int h, int w, int K, int H, int W, float sy, float sx, int local) {
  extern __shared__ unsigned long long ece_lds[];
  __shared__ unsigned lh[UPS_HIST_LDS];
  const int R = bins + 1, KK = K * K;
  unsigned long long* lsum = ece_lds;
  unsigned long long* lcnt = ece_lds + R;
  const bool hlocal = hist != nullptr && KK <= UPS_HIST_LDS;
  if (local) lds_zero(ece_lds, 2 * R);
  if (hlocal) lds_zero(lh, KK);
  __syncthreads();
  const bool vec = ROWS_VEC(rows, ldl, K);
  const size_t total = (size_t)B * H * W;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    int arg = 0;
    const Pixel p = pixel_at(e, rows, ldl, h, w, H, W, sy, sx);
    float best = -INFINITY, v[KREG ? ECE_KREG : 4];
    bool bad = false;
    if (KREG) {
#pragma unroll
      for (int k = 0; k < ECE_KREG; k += 4)
        if (k < K) {
          bilerp4(p, vec, k, K, v + k);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (k + j < K) {
              bad |= v[k + j] != v[k + j];
              if (v[k + j] > best) best = v[k + j], arg = k + j;
            }
        }
    } else {
      for (int k = 0; k < K; k += 4) {
        bilerp4(p, vec, k, K, v);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (k + j < K) {
            bad |= v[j] != v[j];
            if (v[j] > best) best = v[j], arg = k + j;
          }
      }
    }
    float conf = bad ? NAN : best;  // (torch.max: a NaN among the K values is the maximum)
    if (!probs) {
      float sum = 0.f;
      if (KREG) {
#pragma unroll
        for (int k = 0; k < ECE_KREG; ++k)
          if (k < K) sum += expf(v[k] - best);
      } else {
        for (int k = 0; k < K; k += 4) {
          bilerp4(p, vec, k, K, v);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (k + j < K) sum += expf(v[j] - best);
        }
      }
      conf = 1.f / sum;  // softmax of the maximum: exp(0) / sum; NaN when a value is NaN or +inf
    }
    const int g = gt[e], row = ece_row(conf, gap, bins);
    long long fix = 0;
    if (row < bins) fix = __float2ll_rn(fminf(fmaxf(conf, -ECE_CONF_CAP), ECE_CONF_CAP) * ECE_FIX);
    const unsigned long long hit = row < bins && arg == g ? 1ull : 0ull;
    if (local) {
      if (fix) atomicAdd(&lsum[row], (unsigned long long)fix);
      atomicAdd(&lcnt[row], (hit << 32) | 1ull);
    } else {
      if (fix) atomicAdd(&table[(size_t)row * 3], (unsigned long long)fix);
      if (hit) atomicAdd(&table[(size_t)row * 3 + 1], 1ull);
      atomicAdd(&table[(size_t)row * 3 + 2], 1ull);
    }
    if (hist) hist_count(lh, hist, hlocal, g, arg, K);
  }
  __syncthreads();
  if (local) {
    // rotated like the confusion matrix's flush; a row unpacks into its three table columns, so the loop is its own
    const int start = (int)((blockIdx.x * 37u) % (unsigned)R);
    for (int i = threadIdx.x; i < R; i += blockDim.x) {
      int r = i + start;
      if (r >= R) r -= R;
      const unsigned long long c = lcnt[r];
      if (c) {
        const unsigned long long s = lsum[r];
        if (s) atomicAdd(&table[(size_t)r * 3], s);
        if (c >> 32) atomicAdd(&table[(size_t)r * 3 + 1], c >> 32);
        atomicAdd(&table[(size_t)r * 3 + 2], c & 0xffffffffull);
      }
    }
  }
  if (hlocal) flush_rotated(lh, hist, KK);
}

__global__ __launch_bounds__(256) void upsample_bwd_kernel(const float* __restrict__ dout, float* __restrict__ dl,
                                                           int ldl, int B, int h, int w, int K, int H, int W, float sy,
                                                           float sx, float inv_sy, float inv_sx) {
  const size_t total = (size_t)B * h * w * K;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(e % K);
    size_t q = e / K;
    const int x = (int)(q % w);
    q /= w;
    const int y = (int)(q % h), b = (int)(q / h);
    // destination rows whose source coordinate falls in (y-1, y+1), with one row of slack
    int Y0 = (int)floorf((float)(y - 1) * inv_sy) - 1, Y1 = (int)ceilf((float)(y + 1) * inv_sy) + 1;
    int X0 = (int)floorf((float)(x - 1) * inv_sx) - 1, X1 = (int)ceilf((float)(x + 1) * inv_sx) + 1;
    Y0 = max(Y0, 0);
    X0 = max(X0, 0);
    Y1 = min(Y1, H - 1);
    X1 = min(X1, W - 1);
    float acc = 0.f;
    for (int Y = Y0; Y <= Y1; ++Y) {
      const Lerp ly = lerp_index(Y, sy, h);
      const float wy = (ly.i0 == y ? ly.l0 : 0.f) + (ly.i1 == y ? ly.l1 : 0.f);
      if (wy == 0.f) continue;
      const float* row = dout + (((size_t)b * K + k) * H + Y) * W;
      float racc = 0.f;
      for (int X = X0; X <= X1; ++X) {
        const Lerp lx = lerp_index(X, sx, w);
        const float wx = (lx.i0 == x ? lx.l0 : 0.f) + (lx.i1 == x ? lx.l1 : 0.f);
        racc += wx * row[X];
      }
      acc += wy * racc;
    }
    dl[(((size_t)b * h + y) * w + x) * ldl + k] = acc;
  }
}

// ---- loss_calc(interp(logits), label): bilinear upsample (align_corners) -> cross-entropy, without the upsampled tensor ----
// The supervised step (segmentation.py:70-80) upsamples the [B,K,h,w] logits to the label resolution (159 MB at 512x1024,
// batch 4) only to reduce them to one scalar, and its backward pass writes and re-reads a gradient of the same size.  Here
// every output pixel's K logits are interpolated in registers from the low-resolution rows (4.3 MB: cache-resident) in both
// directions; only the labels (1 byte per pixel) are streamed.

// one thread per output pixel: -log softmax(v)[label] for valid labels; per-block partial (sum, count) into ws[block][2]
__global__ __launch_bounds__(256) void upsample_ce_fwd_kernel(const float* __restrict__ logits, int ldl,
                                                              const uint8_t* __restrict__ labels, float* __restrict__ ws, int B,
                                                              int h, int w, int K, int H, int W, float sy, float sx) {
  __shared__ float red[4];
  const size_t total = (size_t)B * H * W;
  float ce = 0.f, nv = 0.f;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int tl = labels[e];
    if (tl >= K) continue;  // 255 = ignore (loss.py:22-31)
    const Pixel p = pixel_at(e, logits, ldl, h, w, H, W, sy, sx);
    float v[UCE_KMAX], m = -INFINITY, vt = 0.f;
#pragma unroll
    for (int k = 0; k < UCE_KMAX; ++k)
      if (k < K) {
        v[k] = bilerp(p.ly, p.lx, p.p00[k], p.p01[k], p.p10[k], p.p11[k]);
        m = fmaxf(m, v[k]);
        if (k == tl) vt = v[k];
      }
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < UCE_KMAX; ++k)
      if (k < K) sum += expf(v[k] - m);
    ce += m + logf(sum) - vt;
    nv += 1.f;
  }
  float r = block_sum_256(ce, red);
  if (threadIdx.x == 0) ws[(size_t)blockIdx.x * 2] = r;
  r = block_sum_256(nv, red);
  if (threadIdx.x == 0) ws[(size_t)blockIdx.x * 2 + 1] = r;
}

__global__ __launch_bounds__(256) void upsample_ce_finalize_kernel(const float* __restrict__ ws, int nblocks, float* __restrict__ result) {
  // fixed order: thread t sums the blocks t, t + 256, ... in double, then a fixed tree over the 256 threads
  __shared__ double sh[2][256];
  const int t = threadIdx.x;
  double s = 0.0, n = 0.0;
  for (int b = t; b < nblocks; b += 256) {
    s += (double)ws[(size_t)b * 2];
    n += (double)ws[(size_t)b * 2 + 1];
  }
  sh[0][t] = s;
  sh[1][t] = n;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      sh[0][t] += sh[0][t + o];
      sh[1][t] += sh[1][t + o];
    }
    __syncthreads();
  }
  if (t == 0) {
    result[0] = (float)(sh[0][0] / sh[1][0]);  // mean over the kept pixels; 0/0 = NaN as in the reference (loss.py:38 never fires)
    result[1] = (float)sh[1][0];
  }
}

// ---- ADVENT's entropy map: prob_2_entropy(softmax(interp(logits))) (advent_da.py:94-128, func.py:71-74) ----------------------
// The discriminators read I_k = -p_k * log2(p_k + 1e-30) / log2(K), p = softmax over the K upsampled logits of a pixel.  Only the
// map itself has to exist: the upsampled logits and the softmax (159 MB each at 512x1024, batch 4) live in registers, in
// both directions.  p is exp(v - max) / sum as ATen's softmax; the constants are float32 as the reference's tensors.
constexpr float ENT_EPS = 1e-30f;
constexpr float ENT_LN2 = 0.6931471805599453f;

// p[k] = softmax(v)[k] in place over k < K
__device__ __forceinline__ void ent_softmax(float* v, int K) {
  const float sum = exp_sum(v, K);
#pragma unroll
  for (int k = 0; k < UCE_KMAX; ++k)
    if (k < K) v[k] = v[k] / sum;
}

// t[k] (the map's upstream gradient) -> the gradient with respect to the pixel's K logits, in place:
// t_k * dI/dp_k, dI/dp = -(log2(p + eps) + p / ((p + eps) ln 2)) / log2 K  (what autograd derives from the expression above),
// then the softmax Jacobian g_k = p_k * (t_k - sum_j p_j t_j)
__device__ __forceinline__ void ent_grad(const float* p, float* t, int K, float log2k) {
  float dot = 0.f;
#pragma unroll
  for (int k = 0; k < UCE_KMAX; ++k)
    if (k < K) {
      const float q = p[k] + ENT_EPS;
      t[k] = t[k] * (-(log2f(q) + p[k] / (q * ENT_LN2)) / log2k);
      dot += p[k] * t[k];
    }
#pragma unroll
  for (int k = 0; k < UCE_KMAX; ++k)
    if (k < K) t[k] = p[k] * (t[k] - dot);
}

// One thread per output pixel, consecutive threads along X: the loads of a `dout` plane and the stores of an `out` plane
// coalesce.  GRAD = false: out = the map.  GRAD = true: out = the per-pixel gradient g[B][K][H][W] with respect to the upsampled
// logits (the route of the width pairs the two-pass backward below does not take; upsample_bwd_kernel gathers it).
template <bool GRAD>
__global__ __launch_bounds__(256) void upsample_entropy_kernel(const float* __restrict__ logits, int ldl,
                                                               const float* __restrict__ dout, float* __restrict__ out, int B,
                                                               int h, int w, int K, int H, int W, float sy, float sx,
                                                               float log2k) {
  const bool vec = ROWS_VEC(logits, ldl, K);
  const size_t total = (size_t)B * H * W, plane = (size_t)H * W;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const Pixel p = pixel_at(e, logits, ldl, h, w, H, W, sy, sx);
    float v[UCE_KMAX];
    if (vec) {
#pragma unroll
      for (int k = 0; k < UCE_KMAX; k += 4)
        if (k < K) bilerp4(p, true, k, K, &v[k]);
    } else {
#pragma unroll
      for (int k = 0; k < UCE_KMAX; ++k)
        if (k < K) v[k] = bilerp(p.ly, p.lx, p.p00[k], p.p01[k], p.p10[k], p.p11[k]);
    }
    ent_softmax(v, K);
    const size_t o = (size_t)p.b * K * plane + (size_t)p.Y * W + p.X;
    if (GRAD) {
      float t[UCE_KMAX];
#pragma unroll
      for (int k = 0; k < UCE_KMAX; ++k)
        if (k < K) t[k] = dout[o + k * plane];
      ent_grad(v, t, K, log2k);
#pragma unroll
      for (int k = 0; k < UCE_KMAX; ++k)
        if (k < K) out[o + k * plane] = t[k];
    } else {
#pragma unroll
      for (int k = 0; k < UCE_KMAX; ++k)
        if (k < K) out[o + k * plane] = -(v[k] * log2f(v[k] + ENT_EPS)) / log2k;
    }
  }
}

// ---- evaluate_model's per-batch tail (eval_UDA.py:47-57): upsample -> argmax -> confusion matrix, and the batch's entropy ------
// prob_2_entropy(softmax(interp(x), 1)).mean() needs the sum of the entropy map, not the map: one thread per output pixel keeps
// its K interpolated logits in registers, takes the class (the first-maximum rule and the counting of upsample_kernel<true>:
// the same expression, so the same class map and the same matrix), then the softmax and e = sum_k I_k in index order, and adds
//   ent[0] += round(e * 2^32) for a finite e (0 <= e <= ~1: 2^31 pixels fit an int64), ent[1] += 1 otherwise (a NaN or +inf
// among the pixel's logits).  Every pixel counts, whatever its label.  The sums are taken per thread, then per wave, then per
// workgroup through LDS: one global atomic per workgroup and non-zero counter.  Integer adds: any grid, any order, one result.
__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void upsample_eval_kernel(const float* __restrict__ rows, int ldl, const uint8_t* __restrict__ gt,
                                                            unsigned long long* __restrict__ hist,
                                                            unsigned long long* __restrict__ ent, uint8_t* __restrict__ cls, int B,
                                                            int h, int w, int K, int H, int W, float sy, float sx, float log2k) {
  __shared__ unsigned lh[UPS_HIST_LDS];  // K <= UCE_KMAX: K * K cells always fit
  __shared__ long long red_sum[4];
  __shared__ long long red_bad[4];
  const int KK = K * K;
  if (hist) {
    lds_zero(lh, KK);
    __syncthreads();
  }
  const bool vec = ROWS_VEC(rows, ldl, K);
  const size_t total = (size_t)B * H * W;
  long long sum = 0, bad = 0;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const Pixel p = pixel_at(e, rows, ldl, h, w, H, W, sy, sx);
    float v[UCE_KMAX];
    if (vec) {
#pragma unroll
      for (int k = 0; k < UCE_KMAX; k += 4)
        if (k < K) bilerp4(p, true, k, K, &v[k]);
    } else {
#pragma unroll
      for (int k = 0; k < UCE_KMAX; ++k)
        if (k < K) v[k] = bilerp(p.ly, p.lx, p.p00[k], p.p01[k], p.p10[k], p.p11[k]);
    }
    float best = -INFINITY;
    int arg = 0;
#pragma unroll
    for (int k = 0; k < UCE_KMAX; ++k)
      if (k < K && v[k] > best) best = v[k], arg = k;
    if (cls) cls[e] = (uint8_t)arg;
    if (hist) hist_count(lh, hist, true, gt[e], arg, K);
    ent_softmax(v, K);
    float en = 0.f;
#pragma unroll
    for (int k = 0; k < UCE_KMAX; ++k)
      if (k < K) en += -(v[k] * log2f(v[k] + ENT_EPS)) / log2k;
    if (fabsf(en) <= 3.402823466e38f) sum += __float2ll_rn(en * ECE_FIX);
    else bad += 1;
  }
  sum = wave_sum_ll(sum);
  bad = wave_sum_ll(bad);
  if ((threadIdx.x & 63) == 0) red_sum[threadIdx.x >> 6] = sum, red_bad[threadIdx.x >> 6] = bad;
  __syncthreads();
  if (threadIdx.x == 0) {
    sum = red_sum[0] + red_sum[1] + red_sum[2] + red_sum[3];
    bad = red_bad[0] + red_bad[1] + red_bad[2] + red_bad[3];
    if (sum) atomicAdd(&ent[0], (unsigned long long)sum);
    if (bad) atomicAdd(&ent[1], (unsigned long long)bad);
  }
  if (hist) flush_rotated(lh, hist, KK);  // (behind the barrier above)
}

// ---- the two-pass backward of the fused heads -----------------------------------------------------------------------------
// Gradient with respect to the LOW-resolution logits.  The interpolation weights are separable, so
//     dl[y][x][k] = sum_Y wy(Y, y) * ( sum_X wx(X, x) * g[Y][X][k] ),   g = the head's gradient with respect to a pixel's
//     upsampled logits (cross-entropy: a * (softmax(v) - onehot) at the kept pixels; entropy map: ent_grad of its cotangent),
// is taken in two gather passes (fixed summation order: deterministic), each output pixel's softmax evaluated about once:
//   pass A, one workgroup per (image, output row Y, block of CW low-resolution columns): the row's interpolated low-res
//     rows r[x][k] = ly.l0 * p[y0][x][k] + ly.l1 * p[y1][x][k] go to LDS once, every output pixel of the block's span then
//     needs two of them (no global loads per pixel); its g[X][k] goes to LDS; threads (x, k) gather over their ~2 W/w
//     columns -> t[b][Y][x][k];
//   pass B, one thread per (b, y, x, k): gathers t over its ~2 H/h rows -> dl.
constexpr int UCE_SPAN = 640;  // output pixels of one pass-A workgroup (LDS: UCE_SPAN * K floats of g)

// What a head contributes to pass A (`Grad`): which pixels have a gradient, and how a pixel's interpolated logits v[0..K) become
// its gradient vector gi[0..K).  The structs carry the head's arguments; the two bodies stand in the kernel itself, under
// `if constexpr`: as member functions they are optimised on their own before they are inlined, and the K-vectors then leave
// the registers (496 VGPRs and 1.5 KB of scratch for the cross-entropy; docs/experiments.md, 2026-10-18).
// CeGrad: the cross-entropy of upsample_ce_fwd_kernel (result[1]: its kept pixels) times the upstream gradient *gscale
// (nullptr: 1) and w_ce.  EntGrad: the entropy map under the cotangent dout[B][K][H][W] (each thread reads its pixel's K values
// plane by plane: consecutive threads, consecutive addresses).
struct CeGrad {
  const uint8_t* labels;
  const float *result, *gscale;
  float w_ce;
};
struct EntGrad {
  const float* dout;
  float log2k;
};

template <class Grad>
__global__ __launch_bounds__(256) void upsample_bwd_rows_kernel(const Grad grad, const float* __restrict__ logits, int ldl,
                                                                float* __restrict__ tmp, int B, int h, int w, int K, int H, int W,
                                                                float sy, float sx, float inv_sx, int CW) {
  constexpr bool CE = std::is_same<Grad, CeGrad>::value;
  extern __shared__ float uce_lds[];
  float* r = uce_lds;                    // [CW + 2][K]
  float* g = r + (CW + 2) * K;           // [UCE_SPAN][K]
  float* lw = g + UCE_SPAN * K;          // [UCE_SPAN]: l1 of the pixel's column interpolation
  int* li = reinterpret_cast<int*>(lw + UCE_SPAN);  // [UCE_SPAN]: its i0 (i1 = i0 + 1, or i0 at the right edge: l1 = 0 there)
  const int t = threadIdx.x;
  const int xb = blockIdx.x * CW, xe = min(w, xb + CW);  // low-resolution columns of this workgroup
  const int Y = blockIdx.y % H, b = blockIdx.y / H;
  float a_ce = 0.f;  // cross-entropy: upstream * w_ce / number of kept pixels (none kept: 0, the gradient is zeros)
  if constexpr (CE) {
    const float nvalid = grad.result[1];
    a_ce = nvalid > 0.f ? (grad.gscale ? grad.gscale[0] : 1.f) * grad.w_ce / nvalid : 0.f;
  }
  const Lerp ly = lerp_index(Y, sy, h);
  // output columns that read a column of [xb, xe): source coordinate in (xb - 1, xe), with one of slack on either side
  int X0 = (int)floorf((float)(xb - 1) * inv_sx) - 1, X1 = (int)ceilf((float)xe * inv_sx) + 1;
  X0 = max(X0, 0);
  X1 = min(X1, W - 1);
  const int span = X1 - X0 + 1;          // <= UCE_SPAN (the host picks CW)
  const int x_lo = max(xb - 1, 0), nxr = min(w, xe + 1) - x_lo;  // low-res columns those pixels interpolate between
  const float* p0 = logits + ((size_t)b * h + ly.i0) * w * ldl;
  const float* p1 = logits + ((size_t)b * h + ly.i1) * w * ldl;
  for (int idx = t; idx < nxr * K; idx += 256) {
    const int x = idx / K, k = idx - x * K;
    r[idx] = ly.l0 * p0[(size_t)(x_lo + x) * ldl + k] + ly.l1 * p1[(size_t)(x_lo + x) * ldl + k];
  }
  __syncthreads();
  const size_t plane = (size_t)H * W;
  for (int i = t; i < span; i += 256) {
    const int X = X0 + i;
    const Lerp lx = lerp_index(X, sx, w);
    li[i] = lx.i0;
    lw[i] = lx.i1 != lx.i0 ? lx.l1 : 0.f;
    float* gi = g + i * K;
    int tl = 0;
    bool kept = lx.i0 >= x_lo && lx.i1 < x_lo + nxr;  // (slack pixels outside the block's rows contribute nothing)
    if constexpr (CE) {
      tl = grad.labels[((size_t)b * H + Y) * W + X];
      kept = kept && tl < K;
    }
    if (!kept) {
      for (int k = 0; k < K; ++k) gi[k] = 0.f;
      continue;
    }
    const float* r0 = r + (lx.i0 - x_lo) * K;
    const float* r1 = r + (lx.i1 - x_lo) * K;
    float v[UCE_KMAX];
    if constexpr (CE) {
      // the maximum comes out of the interpolation loop, not from exp_sum: the label test above tells the compiler K > 0, and
      // with the loops apart it then keeps v[] as one 32-wide vector (496 VGPRs, scratch)
      float m = -INFINITY, sum = 0.f;
#pragma unroll
      for (int k = 0; k < UCE_KMAX; ++k)
        if (k < K) {
          v[k] = lx.l0 * r0[k] + lx.l1 * r1[k];
          m = fmaxf(m, v[k]);
        }
#pragma unroll
      for (int k = 0; k < UCE_KMAX; ++k)
        if (k < K) {
          v[k] = expf(v[k] - m);
          sum += v[k];
        }
      const float inv = a_ce / sum;
#pragma unroll
      for (int k = 0; k < UCE_KMAX; ++k)
        if (k < K) gi[k] = v[k] * inv - (k == tl ? a_ce : 0.f);
    } else {
      const float* drow = grad.dout + (size_t)b * K * plane + (size_t)Y * W;
      float u[UCE_KMAX];
#pragma unroll
      for (int k = 0; k < UCE_KMAX; ++k)
        if (k < K) {
          v[k] = lx.l0 * r0[k] + lx.l1 * r1[k];
          u[k] = drow[k * plane + X];
        }
      ent_softmax(v, K);
      ent_grad(v, u, K, grad.log2k);
#pragma unroll
      for (int k = 0; k < UCE_KMAX; ++k)
        if (k < K) gi[k] = u[k];
    }
  }
  __syncthreads();
  float* out = tmp + (((size_t)b * H + Y) * w) * K;
  for (int idx = t; idx < (xe - xb) * K; idx += 256) {
    const int xr = idx / K, k = idx - xr * K, x = xb + xr;
    int A0 = (int)floorf((float)(x - 1) * inv_sx) - 1, A1 = (int)ceilf((float)(x + 1) * inv_sx) + 1;
    A0 = max(A0, X0);
    A1 = min(A1, X1);
    float acc = 0.f;
    for (int X = A0; X <= A1; ++X) {
      const int i = X - X0, i0 = li[i];
      const float l1 = lw[i];
      const float wx = i0 == x ? 1.f - l1 : (i0 + 1 == x ? l1 : 0.f);
      acc += wx * g[i * K + k];
    }
    out[(size_t)x * K + k] = acc;
  }
}

__global__ __launch_bounds__(256) void upsample_ce_bwd_cols_kernel(const float* __restrict__ tmp, float* __restrict__ dl, int ldl, int B,
                                                                   int h, int w, int K, int H, float sy, float inv_sy) {
  const size_t total = (size_t)B * h * w * ldl;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(e % ldl);
    size_t q = e / ldl;
    const int x = (int)(q % w);
    q /= w;
    const int y = (int)(q % h), b = (int)(q / h);
    float acc = 0.f;
    if (k < K) {
      int Y0 = (int)floorf((float)(y - 1) * inv_sy) - 1, Y1 = (int)ceilf((float)(y + 1) * inv_sy) + 1;
      Y0 = max(Y0, 0);
      Y1 = min(Y1, H - 1);
      for (int Y = Y0; Y <= Y1; ++Y) {
        const Lerp ly = lerp_index(Y, sy, h);
        const float wy = (ly.i0 == y ? ly.l0 : 0.f) + (ly.i1 == y ? ly.l1 : 0.f);
        if (wy != 0.f) acc += wy * tmp[(((size_t)b * H + Y) * w + x) * K + k];
      }
    }
    dl[e] = acc;  // (columns >= K: zero)
  }
}

static inline unsigned ew_grid(size_t total) {
  size_t g = (total + 255) / 256;
  if (g > 16384) g = 16384;
  if (g < 1) g = 1;
  return (unsigned)g;
}

// align_corners scale exactly as ATen computes it (float division, 0 when out size is 1)
static inline float ac_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

// low-resolution columns per pass-A workgroup of the fused head's backward: as many as keep its output span within UCE_SPAN
// pixels; below 1 (upsampling factors past ~211x along x) the fused head does not take the shape
static inline int uce_block_cols(int w, int W) {
  int CW = (int)((UCE_SPAN - 6) * ac_scale(w, W)) - 2;
  return CW > 64 ? 64 : CW;
}

// Both passes of a fused head's backward: pass A with the head's `Grad`, then upsample_ce_bwd_cols_kernel.  ws holds
// B * H * w * K floats.
template <class Grad>
int upsample_bwd_two_pass(const Grad& grad, const float* logits, int ldl, float* dlogits, float* ws, int B, int h, int w, int K,
                          int H, int W, onda_stream_t s) {
  const float sy = ac_scale(h, H), sx = ac_scale(w, W);
  const int CW = uce_block_cols(w, W);
  ONDA_REQUIRE(CW >= 1);
  const size_t lds = ((size_t)(CW + 2) * K + (size_t)UCE_SPAN * K + 2 * UCE_SPAN) * sizeof(float);
  // 19 classes: 59 KB.  Every K the forward accepts (<= UCE_KMAX = 32: 95 KB) has to run backward as well: above the default
  // 64 KB limit of dynamic LDS the kernel (each instantiation for itself) asks for its size once (a CU of gfx950 has 160 KB)
  ONDA_REQUIRE(lds <= 160 * 1024);
  if (lds > 64 * 1024) {
    static size_t granted = 0;
    if (lds > granted) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(upsample_bwd_rows_kernel<Grad>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return (int)e;
      granted = lds;
    }
  }
  hipLaunchKernelGGL(upsample_bwd_rows_kernel<Grad>, dim3((w + CW - 1) / CW, B * H), dim3(256), lds, ONDA_STREAM(s), grad, logits, ldl,
                     ws, B, h, w, K, H, W, sy, sx, 1.f / sx, CW);
  hipLaunchKernelGGL(upsample_ce_bwd_cols_kernel, dim3(ew_grid((size_t)B * h * w * ldl)), dim3(256), 0, ONDA_STREAM(s), ws, dlogits,
                     ldl, B, h, w, K, H, sy, 1.f / sy);
  return ONDA_LAUNCH_RESULT();
}

}  // namespace

extern "C" {

int onda_maxpool_fwd(const float* x, float* y, uint8_t* idx, int B, int Hi, int Wi, int C, int Ho, int Wo,
                     onda_stream_t s) {
  ONDA_REQUIRE(x && y && idx && C % 4 == 0);
  const size_t total = (size_t)B * Ho * Wo * (C / 4);
  hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(ew_grid(total)), dim3(256), 0, ONDA_STREAM(s), x, y, idx, B, Hi, Wi, C, Ho,
                     Wo, static_cast<_Float16*>(nullptr), static_cast<const float*>(nullptr));
  return ONDA_LAUNCH_RESULT();
}

int onda_maxpool_fwd_limbs(const float* x, const float* xamax, void* yl, uint8_t* idx, int B, int Hi, int Wi, int C, int Ho, int Wo,
                           onda_stream_t s) {
  ONDA_REQUIRE(x && xamax && yl && idx && C % 32 == 0);
  if (!ONDA_ALIGNED16(yl)) return ONDA_EALIGN;
  const size_t total = (size_t)B * Ho * Wo * (C / 4);
  hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(ew_grid(total)), dim3(256), 0, ONDA_STREAM(s), x, static_cast<float*>(nullptr), idx, B,
                     Hi, Wi, C, Ho, Wo, static_cast<_Float16*>(yl), xamax);
  return ONDA_LAUNCH_RESULT();
}

int onda_maxpool_bwd(const float* dy, const uint8_t* idx, float* dx, int B, int Hi, int Wi, int C, int Ho, int Wo,
                     onda_stream_t s) {
  ONDA_REQUIRE(dy && dx && idx && C % 4 == 0);
  const size_t total = (size_t)B * Hi * Wi * (C / 4);
  hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(ew_grid(total)), dim3(256), 0, ONDA_STREAM(s), dy, idx, dx, B, Hi, Wi, C,
                     Ho, Wo);
  return ONDA_LAUNCH_RESULT();
}

int onda_se_fc_fwd(const float* pooled, const float* w1, const float* b1, const float* w2, const float* b2,
                   float* hidden, float* gate, int B, int C, int R, onda_stream_t s) {
  ONDA_REQUIRE(pooled && w1 && b1 && w2 && b2 && hidden && gate && R <= 4096);
  hipLaunchKernelGGL(se_fc1_kernel, dim3((R + 3) / 4, B), dim3(256), 0, ONDA_STREAM(s), pooled, w1, b1, hidden, C, R);
  hipLaunchKernelGGL(se_fc2_kernel, dim3((C + 255) / 256, B), dim3(256), R * sizeof(float), ONDA_STREAM(s), hidden, w2, b2, gate, C,
                     R);
  return ONDA_LAUNCH_RESULT();
}

int onda_se_fc_bwd(const float* dgate, const float* pooled, const float* hidden, const float* gate, const float* w1,
                   const float* w2, float* dw1, float* db1, float* dw2, float* db2, float* dpooled, float* ws,
                   float dpooled_scale, int B, int C, int R, onda_stream_t s) {
  ONDA_REQUIRE(dgate && pooled && hidden && gate && w1 && w2 && dw1 && db1 && dw2 && db2 && dpooled && ws);
  hipLaunchKernelGGL(se_bwd_w2_kernel, dim3((C * R + 255) / 256), dim3(256), 0, ONDA_STREAM(s), dgate, gate, hidden, dw2,
                     db2, B, C, R);
  hipLaunchKernelGGL(se_bwd_hidden_kernel, dim3(B), dim3(256), 0, ONDA_STREAM(s), dgate, gate, hidden, w2, ws, C, R);
  const int n = (R > B ? R : B) * C;
  hipLaunchKernelGGL(se_bwd_w1_kernel, dim3((n + 255) / 256), dim3(256), 0, ONDA_STREAM(s), ws, pooled, w1, dw1, db1,
                     dpooled, B, C, R, dpooled_scale);
  return ONDA_LAUNCH_RESULT();
}

int onda_chan_scale(const float* x, const float* gate, const float* add, float* out, int B, int64_t HW, int C,
                    onda_stream_t s) {
  ONDA_REQUIRE(x && gate && out && C % 4 == 0);
  const size_t total4 = (size_t)B * HW * C / 4;
  hipLaunchKernelGGL(chan_scale_kernel, dim3(ew_grid(total4)), dim3(256), 0, ONDA_STREAM(s), x, gate, add, out, HW, C,
                     total4);
  return ONDA_LAUNCH_RESULT();
}

int onda_upsample_fwd(const float* logits, int ldl, float* out, int B, int h, int w, int K, int H, int W,
                      onda_stream_t s) {
  ONDA_REQUIRE(logits && out && K <= ldl);
  hipLaunchKernelGGL((upsample_kernel<false>), dim3(ew_grid((size_t)B * H * W)), dim3(256), 0, ONDA_STREAM(s), logits,
                     ldl, out, (uint8_t*)nullptr, (const uint8_t*)nullptr, (unsigned long long*)nullptr, B, h, w, K, H, W,
                     ac_scale(h, H), ac_scale(w, W));
  return ONDA_LAUNCH_RESULT();
}

int onda_upsample_argmax(const float* logits, int ldl, uint8_t* cls, int B, int h, int w, int K, int H, int W,
                         onda_stream_t s) {
  ONDA_REQUIRE(logits && cls && K <= ldl && K <= 255);
  hipLaunchKernelGGL((upsample_kernel<true>), dim3(ew_grid((size_t)B * H * W)), dim3(256), 0, ONDA_STREAM(s), logits,
                     ldl, (float*)nullptr, cls, (const uint8_t*)nullptr, (unsigned long long*)nullptr, B, h, w, K, H, W,
                     ac_scale(h, H), ac_scale(w, W));
  return ONDA_LAUNCH_RESULT();
}

int onda_upsample_argmax_hist(const float* logits, int ldl, const uint8_t* labels, int64_t* hist, uint8_t* cls, int B,
                              int h, int w, int K, int H, int W, onda_stream_t s) {
  ONDA_REQUIRE(logits && labels && hist && K <= ldl && K <= 255);
  unsigned grid = ew_grid((size_t)B * H * W);
  if (K * K <= UPS_HIST_LDS && grid > 1024u) grid = 1024u;  // one flush of the workgroup's counts each: fewer, longer workgroups
  hipLaunchKernelGGL((upsample_kernel<true>), dim3(grid), dim3(256), 0, ONDA_STREAM(s), logits,
                     ldl, (float*)nullptr, cls, labels, reinterpret_cast<unsigned long long*>(hist), B, h, w, K, H, W,
                     ac_scale(h, H), ac_scale(w, W));
  return ONDA_LAUNCH_RESULT();
}

int onda_ece_bins_local(void) { return ECE_BINS_LDS; }

int onda_upsample_ece(const float* rows, int ld, const uint8_t* labels, int64_t* table, int bins, int probs, int64_t* hist, int B,
                      int h, int w, int K, int H, int W, onda_stream_t s) {
  ONDA_REQUIRE(rows && labels && table && K >= 1 && K <= ld && K <= 255 && bins >= 1 && bins <= (1 << 20) && B >= 1 && h >= 1 &&
               w >= 1 && H >= 1 && W >= 1);
  if (!ONDA_ALIGNED16(table) || (hist && !ONDA_ALIGNED16(hist))) return ONDA_EALIGN;
  const size_t total = (size_t)B * H * W;
  const int local = bins <= ECE_BINS_LDS;
  unsigned grid = ew_grid(total);
  // one flush of the workgroup's rows each: two workgroups per CU of long-lived counters instead of one per 256 pixels
  if ((local || (hist && K * K <= UPS_HIST_LDS)) && grid > 512u) grid = 512u;
  ONDA_REQUIRE(total / grid < (1ull << 32) - 256);  // (correct << 32 | pixels) per workgroup
  const size_t lds = local ? (size_t)(bins + 1) * 16 : 0;
  const float gap = (float)(1.0 / bins);  // the reference's 1.0 / bins, rounded to float32 where it meets the confidences
  auto* t = reinterpret_cast<unsigned long long*>(table);
  auto* hh = reinterpret_cast<unsigned long long*>(hist);
  const float sy = ac_scale(h, H), sx = ac_scale(w, W);
  if (K <= ECE_KREG)
    hipLaunchKernelGGL((upsample_ece_kernel<true>), dim3(grid), dim3(256), lds, ONDA_STREAM(s), rows, ld, labels, t, bins, gap,
                       probs ? 1 : 0, hh, B, h, w, K, H, W, sy, sx, local);
  else
    hipLaunchKernelGGL((upsample_ece_kernel<false>), dim3(grid), dim3(256), lds, ONDA_STREAM(s), rows, ld, labels, t, bins, gap,
                       probs ? 1 : 0, hh, B, h, w, K, H, W, sy, sx, local);
  return ONDA_LAUNCH_RESULT();
}

int onda_upsample_eval(const float* rows, int ldl, const uint8_t* labels, int64_t* hist, int64_t* ent, uint8_t* cls, int B, int h,
                       int w, int K, int H, int W, onda_stream_t s) {
  ONDA_REQUIRE(rows && ent && (labels != nullptr) == (hist != nullptr) && K >= 2 && K <= UCE_KMAX && K <= ldl && B >= 1 && h >= 1 &&
               w >= 1 && H >= 1 && W >= 1);
  const size_t total = (size_t)B * H * W;
  ONDA_REQUIRE(total <= (1ull << 31));  // ent[0] in 2^-32 steps, e <= ~1; a workgroup's LDS counts are 32 bits wide
  unsigned grid = ew_grid(total);
  if (grid > 1024u) grid = 1024u;  // one flush of the workgroup's counts each (onda_upsample_argmax_hist)
  hipLaunchKernelGGL(upsample_eval_kernel, dim3(grid), dim3(256), 0, ONDA_STREAM(s), rows, ldl, labels,
                     reinterpret_cast<unsigned long long*>(hist), reinterpret_cast<unsigned long long*>(ent), cls, B, h, w, K, H, W,
                     ac_scale(h, H), ac_scale(w, W), (float)log2((double)K));
  return ONDA_LAUNCH_RESULT();
}

int onda_upsample_ce_fused(int w, int W) { return w > 1 && W > 1 && uce_block_cols(w, W) >= 1; }

int64_t onda_upsample_ce_ws(int B, int H, int W) { return 2 * (int64_t)ew_grid((size_t)B * H * W); }

int onda_upsample_ce_fwd(const float* logits, int ldl, const uint8_t* labels, float* result, float* ws, int B, int h, int w, int K,
                         int H, int W, onda_stream_t s) {
  ONDA_REQUIRE(logits && labels && result && ws && K <= ldl && K <= UCE_KMAX && h > 1 && w > 1 && H > 1 && W > 1);
  const unsigned nb = ew_grid((size_t)B * H * W);
  hipLaunchKernelGGL(upsample_ce_fwd_kernel, dim3(nb), dim3(256), 0, ONDA_STREAM(s), logits, ldl, labels, ws, B, h, w, K, H, W,
                     ac_scale(h, H), ac_scale(w, W));
  hipLaunchKernelGGL(upsample_ce_finalize_kernel, dim3(1), dim3(256), 0, ONDA_STREAM(s), ws, (int)nb, result);
  return ONDA_LAUNCH_RESULT();
}

int64_t onda_upsample_ce_bwd_ws(int B, int w, int K, int H) { return (int64_t)B * H * w * K; }

int onda_upsample_ce_bwd(const float* logits, int ldl, const uint8_t* labels, const float* result, const float* gscale, float w_ce,
                         float* dlogits, float* ws, int B, int h, int w, int K, int H, int W, onda_stream_t s) {
  ONDA_REQUIRE(logits && labels && result && dlogits && ws && K <= ldl && K <= UCE_KMAX && h > 1 && w > 1 && H > 1 && W > 1);
  return upsample_bwd_two_pass(CeGrad{labels, result, gscale, w_ce}, logits, ldl, dlogits, ws, B, h, w, K, H, W, s);
}

int onda_upsample_entropy_fwd(const float* logits, int ldl, float* out, int B, int h, int w, int K, int H, int W, onda_stream_t s) {
  ONDA_REQUIRE(logits && out && K >= 2 && K <= ldl && K <= UCE_KMAX && B >= 1 && h > 1 && w > 1 && H > 1 && W > 1);
  hipLaunchKernelGGL((upsample_entropy_kernel<false>), dim3(ew_grid((size_t)B * H * W)), dim3(256), 0, ONDA_STREAM(s), logits, ldl,
                     static_cast<const float*>(nullptr), out, B, h, w, K, H, W, ac_scale(h, H), ac_scale(w, W),
                     (float)log2((double)K));
  return ONDA_LAUNCH_RESULT();
}

int64_t onda_upsample_entropy_bwd_ws(int B, int w, int K, int H, int W) {
  return onda_upsample_ce_fused(w, W) ? (int64_t)B * H * w * K : (int64_t)B * K * H * W;
}

int onda_upsample_entropy_bwd(const float* logits, int ldl, const float* dout, float* dlogits, float* ws, int B, int h, int w, int K,
                              int H, int W, onda_stream_t s) {
  ONDA_REQUIRE(logits && dout && dlogits && ws && K >= 2 && K <= ldl && K <= UCE_KMAX && B >= 1 && h > 1 && w > 1 && H > 1 && W > 1);
  const float log2k = (float)log2((double)K);
  if (uce_block_cols(w, W) >= 1) return upsample_bwd_two_pass(EntGrad{dout, log2k}, logits, ldl, dlogits, ws, B, h, w, K, H, W, s);
  // past what pass A's span takes: per-pixel gradient into ws[B][K][H][W], then the plain upsample gather (which leaves the
  // padding columns alone: zero the rows first)
  const float sy = ac_scale(h, H), sx = ac_scale(w, W);
  if (ldl > K) {
    const hipError_t e = hipMemsetAsync(dlogits, 0, (size_t)B * h * w * ldl * sizeof(float), ONDA_STREAM(s));
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL((upsample_entropy_kernel<true>), dim3(ew_grid((size_t)B * H * W)), dim3(256), 0, ONDA_STREAM(s), logits, ldl,
                     dout, ws, B, h, w, K, H, W, sy, sx, log2k);
  hipLaunchKernelGGL(upsample_bwd_kernel, dim3(ew_grid((size_t)B * h * w * K)), dim3(256), 0, ONDA_STREAM(s), ws, dlogits, ldl, B,
                     h, w, K, H, W, sy, sx, 1.f / sy, 1.f / sx);
  return ONDA_LAUNCH_RESULT();
}

int onda_upsample_bwd(const float* dout, float* dlogits, int ldl, int B, int h, int w, int K, int H, int W,
                      onda_stream_t s) {
  ONDA_REQUIRE(dout && dlogits && K <= ldl && h > 1 && w > 1 && H > 1 && W > 1);
  const float sy = ac_scale(h, H), sx = ac_scale(w, W);
  hipLaunchKernelGGL(upsample_bwd_kernel, dim3(ew_grid((size_t)B * h * w * K)), dim3(256), 0, ONDA_STREAM(s), dout,
                     dlogits, ldl, B, h, w, K, H, W, sy, sx, 1.f / sy, 1.f / sx);
  return ONDA_LAUNCH_RESULT();
}

}  // extern "C"
