// Per-pixel class-vector kernels: softmax statistics, the fused target losses and their
// gradient, prototype distances / pseudo-labels, prototype statistics and EMA, plus the
// multi-tensor SGD and teacher-EMA updates.  All HBM-bound; reductions are two-stage with a
// fixed order (bitwise reproducible).
#include "common.h"

namespace {

constexpr int KMAX = 32;              // class vectors are kept in registers, K <= 32
constexpr float LOG_CLAMP = -9.21034037f;  // log(1e-4): loss.py:104-106 clamps the one-hot to [1e-4, 1]

// result[j] = scale * sum over blocks of ws[block][j]; one workgroup of 64 * nvals threads: a wave per value, lanes strided
// over the blocks, fixed order (lane-local sums in block order, then the wave tree): bitwise reproducible
__global__ void sum_partials_kernel(const float* __restrict__ ws, int nblocks, int nvals, float scale,
                                    float* __restrict__ result) {
  const int j = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (j >= nvals) return;
  double s = 0.0;
  for (int b = lane; b < nblocks; b += 64) s += (double)ws[(size_t)b * nvals + j];
  s = wave_sum_d(s);
  if (lane == 0) result[j] = (float)(s * (double)scale);
}

// ---- one pixel's class vector: the steps the loss kernels share ---------------------------------------------------------
// v[0..K) = the row's logits; returns their maximum
__device__ __forceinline__ float load_row_max(const float* __restrict__ row, int K, float* v) {
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) {
      v[k] = row[k];
      m = fmaxf(m, v[k]);
    }
  return m;
}

// sum_k exp(v[k] - m), and what stays in v[k]: the logit, exp(v - m), or v - m.  seg_loss forms log p = v - (m + log sum) from
// the logits; target_loss forms p = exp(v - m) / sum and log p = (v - m) - log(sum) from the shifted logits, as softmax /
// log_softmax do: v - (m + log(sum)) would carry the rounding of m + log(sum) (an ulp of the largest logit) into every p
enum { KEEP_LOGIT, KEEP_EXP, KEEP_SHIFTED };
template <int KEEP>
__device__ __forceinline__ float exp_sum_row(float* v, float m, int K) {
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) {
      const float x = v[k] - m, e = expf(x);
      if constexpr (KEEP == KEEP_EXP) v[k] = e;
      if constexpr (KEEP == KEEP_SHIFTED) v[k] = x;
      sum += e;
    }
  return sum;
}

// a hard label: cls is compared with class indices; valid = enters CE; mask = not the ignore value (enters RCE and JS)
struct PixelLabel {
  int cls;
  bool valid, mask;
};
__device__ __forceinline__ PixelLabel classify(int64_t tl, int K) {
  return {(int)tl, tl >= 0 && tl != 255 && tl < K, tl != 255};
}

// CE and RCE in the gradient: coefficients from the upstream gradient and the forward pass' pixel counts, and one class' term
struct CeRceCoef {
  float ce, rce;
};
__device__ __forceinline__ CeRceCoef ce_rce_coef(float gs, float w_ce, float w_rce, float nvalid, float nmask) {
  return {nvalid > 0.f ? gs * w_ce / nvalid : 0.f, gs * w_rce * (-LOG_CLAMP) / (nmask + 1e-6f)};
}
__device__ __forceinline__ float ce_rce_grad(CeRceCoef a, PixelLabel l, int k, float p, float pt) {
  const float onehot = (k == l.cls) ? 1.f : 0.f;
  float g = 0.f;
  if (l.valid) g += a.ce * (p - onehot);
  if (l.mask) g += a.rce * pt * (p - onehot);
  return g;
}

// ws[block][j] = sum of part[j] over the block's 256 threads, j < NV <= 8: wave sums, one barrier, the four added in wave order
template <int NV>
__device__ __forceinline__ void block_partials(const float (&part)[NV], float* red, float* __restrict__ ws) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const float r = wave_sum(part[j]);
    if (lane == 0) red[j * 4 + wave] = r;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    const int j = threadIdx.x;
    ws[(size_t)blockIdx.x * 8 + j] = red[j * 4 + 0] + red[j * 4 + 1] + red[j * 4 + 2] + red[j * 4 + 3];
  }
}

// s[j] = sum over blocks of ws[block][j], in block order, in double
template <int NV>
__device__ __forceinline__ void sum_block_partials(const float* __restrict__ ws, int nblocks, double (&s)[NV]) {
  for (int j = 0; j < NV; ++j) s[j] = 0.0;
  for (int b = 0; b < nblocks; ++b)
    for (int j = 0; j < NV; ++j) s[j] += (double)ws[(size_t)b * 8 + j];
}

// ---- softmax statistics ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void softmax_stats_kernel(const float* __restrict__ logits, int ldl,
                                                            float* __restrict__ probs, int ldp,
                                                            int32_t* __restrict__ argmax, float* __restrict__ ws,
                                                            int64_t N, int K) {
  __shared__ float red[4];
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float pmax = 0.f;
  if (n < N) {
    const float* row = logits + (size_t)n * ldl;
    float v[KMAX];
    float m = -INFINITY;
    int am = 0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)  // (not load_row_max: the first maximum with its index, by comparison)
      if (k < K) {
        v[k] = row[k];
        if (v[k] > m) {
          m = v[k];
          am = k;
        }
      }
    const float sum = exp_sum_row<KEEP_EXP>(v, m, K);
    const float inv = 1.f / sum;
    if (probs) {
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) probs[(size_t)n * ldp + k] = v[k] / sum;
    }
    if (argmax) argmax[n] = am;
    pmax = inv;  // exp(0)/sum at the maximum
  }
  const float tot = block_sum_256(pmax, red);
  if (threadIdx.x == 0) ws[blockIdx.x] = tot;
}

// ---- CE + RCE + MRKLD ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void seg_loss_fwd_kernel(const float* __restrict__ logits, int ldl,
                                                           const int64_t* __restrict__ labels,
                                                           float* __restrict__ ws, int64_t N, int K) {
  __shared__ float red[5 * 4];
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float part[5] = {0.f, 0.f, 0.f, 0.f, 0.f};  // ce, rce, kld, n_valid, n_mask
  if (n < N) {
    float v[KMAX];
    const float m = load_row_max(logits + (size_t)n * ldl, K, v);
    const float lse = m + logf(exp_sum_row<KEEP_LOGIT>(v, m, K));
    const PixelLabel l = classify(labels[n], K);
    float ce = 0.f, kld = 0.f, others = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        const float lp = v[k] - lse;
        kld -= lp;
        if (l.valid && k == l.cls) ce = -lp;
        if (l.mask && k != l.cls) others += expf(lp);
      }
    part[0] = ce;
    part[1] = l.mask ? -LOG_CLAMP * others : 0.f;
    part[2] = kld;
    part[3] = l.valid ? 1.f : 0.f;
    part[4] = l.mask ? 1.f : 0.f;
  }
  block_partials(part, red, ws);
}

__global__ void seg_loss_finalize_kernel(const float* __restrict__ ws, int nblocks, double total_elems,
                                         float* __restrict__ result) {
  if (threadIdx.x != 0) return;
  double s[5];
  sum_block_partials(ws, nblocks, s);
  result[0] = (float)(s[0] / s[3]);  // mean over kept pixels; 0/0 = NaN as in the reference
  result[1] = (float)(s[1] / (s[4] + 1e-6));
  result[2] = (float)(s[2] / total_elems);
  result[3] = (float)s[3];
  result[4] = (float)s[4];
}

__global__ __launch_bounds__(256) void seg_loss_bwd_kernel(const float* __restrict__ logits, int ldl,
                                                           const int64_t* __restrict__ labels,
                                                           const float* __restrict__ result,
                                                           const float* __restrict__ gscale, float w_ce, float w_rce,
                                                           float w_reg, float* __restrict__ dl, int64_t N, int K) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const float gs = gscale ? gscale[0] : 1.f;
  const CeRceCoef coef = ce_rce_coef(gs, w_ce, w_rce, result[3], result[4]);
  const float a_reg = gs * w_reg / ((float)N * (float)K);
  float v[KMAX];
  const float m = load_row_max(logits + (size_t)n * ldl, K, v);
  const float sum = exp_sum_row<KEEP_EXP>(v, m, K);
  const PixelLabel l = classify(labels[n], K);
  float pt = 0.f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) {
      v[k] = v[k] / sum;
      if (k == l.cls) pt = v[k];
    }
  float* out = dl + (size_t)n * ldl;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k >= ldl) break;
    float g = 0.f;
    if (k < K) g = ce_rce_grad(coef, l, k, v[k], pt) + a_reg * ((float)K * v[k] - 1.f);
    out[k] = g;
  }
}

// ---- CE + RCE + (MRKLD | MRENT) + JS ------------------------------------------------------------
// The general target loss of prototypes.py:299-333.  JS follows loss.py:48-85 term by term: y = one-hot clamped to
// [1e-4, 1] (all 1e-4 at an ignored pixel), mp = p * mask, a = (y + mp) / 2, v * log2(v + 1e-30) per entry; a pixel's
// numerator is sum_k [-a log2(a+eps) + (y log2(y+eps) + mp log2(mp+eps)) / 2] and JS = sum / (log2(K) * n_mask).
enum { REG_NONE = 0, REG_MRKLD = 1, REG_MRENT = 2 };
constexpr float JS_EPS = 1e-30f;
constexpr float JS_FLOOR = 1e-4f;

__device__ __forceinline__ float xlog2x(float x) { return x * log2f(x + JS_EPS); }
// d/dx [x log2(x + eps)]
__device__ __forceinline__ float dxlog2x(float x) { return log2f(x + JS_EPS) + x / ((x + JS_EPS) * 0.69314718056f); }

__global__ __launch_bounds__(256) void target_loss_fwd_kernel(const float* __restrict__ logits, int ldl,
                                                              const int64_t* __restrict__ labels, int reg_kind,
                                                              float* __restrict__ ws, int64_t N, int K) {
  __shared__ float red[6 * 4];
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float part[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // ce, rce, reg, js numerator, n_valid, n_mask
  if (n < N) {
    float v[KMAX];
    const float m = load_row_max(logits + (size_t)n * ldl, K, v);
    const float sum = exp_sum_row<KEEP_SHIFTED>(v, m, K);
    const float lsum = logf(sum);
    const PixelLabel l = classify(labels[n], K);
    const float fm = l.mask ? 1.f : 0.f;
    float ce = 0.f, others = 0.f, reg = 0.f, js = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        const float lp = v[k] - lsum;
        const float p = expf(v[k]) / sum;
        if (l.valid && k == l.cls) ce = -lp;
        if (l.mask && k != l.cls) others += p;
        if (reg_kind == REG_MRKLD) reg -= lp;
        if (reg_kind == REG_MRENT) reg += p * lp;
        const float y = (l.mask && k == l.cls) ? 1.f : JS_FLOOR;
        const float mp = p * fm;
        const float a = (y + mp) / 2.f;
        js += -xlog2x(a) + (xlog2x(y) + xlog2x(mp)) / 2.f;
      }
    part[0] = ce;
    part[1] = l.mask ? -LOG_CLAMP * others : 0.f;
    part[2] = reg;
    part[3] = js;
    part[4] = l.valid ? 1.f : 0.f;
    part[5] = fm;
  }
  block_partials(part, red, ws);
}

// result = {ce, rce, reg, js, n_valid, n_mask, total}
__global__ void target_loss_finalize_kernel(const float* __restrict__ ws, int nblocks, int reg_kind, int64_t N, int K,
                                            float w_ce, float w_rce, float w_reg, float w_js,
                                            float* __restrict__ result) {
  if (threadIdx.x != 0) return;
  double s[6];
  sum_block_partials(ws, nblocks, s);
  const double ce = s[0] / s[4];  // 0/0 = NaN as in the reference
  const double rce = s[1] / (s[5] + 1e-6);
  const double reg = reg_kind == REG_MRKLD ? s[2] / ((double)N * K) : reg_kind == REG_MRENT ? s[2] / (double)N : 0.0;
  const double js = s[3] / (log2((double)K) * s[5]);  // n_mask == 0: +inf, as the reference's division by mask.sum()
  // only the terms with a weight enter the total, as the reference adds them under `if weight > 0`
  double total = 0.0;
  if (w_ce != 0.f) total += (double)w_ce * ce;
  if (w_rce != 0.f) total += (double)w_rce * rce;
  if (w_reg != 0.f) total += (double)w_reg * reg;
  if (w_js != 0.f) total += (double)w_js * js;
  result[0] = (float)ce;
  result[1] = (float)rce;
  result[2] = (float)reg;
  result[3] = (float)js;
  result[4] = (float)s[4];
  result[5] = (float)s[5];
  result[6] = (float)total;
  result[7] = 0.f;
}

__global__ __launch_bounds__(256) void target_loss_bwd_kernel(const float* __restrict__ logits, int ldl,
                                                              const int64_t* __restrict__ labels, int reg_kind,
                                                              const float* __restrict__ result,
                                                              const float* __restrict__ gscale, float w_ce, float w_rce,
                                                              float w_reg, float w_js, float* __restrict__ dl, int64_t N,
                                                              int K) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const float gs = gscale ? gscale[0] : 1.f;
  const float nmask = result[5];
  const CeRceCoef coef = ce_rce_coef(gs, w_ce, w_rce, result[4], nmask);
  const float a_reg = reg_kind == REG_MRKLD   ? gs * w_reg / ((float)N * (float)K)
                      : reg_kind == REG_MRENT ? gs * w_reg / (float)N
                                              : 0.f;
  // n_mask == 0 makes this +inf and the gradient NaN, as in the reference; without JS nothing of it is used
  const bool use_js = w_js != 0.f;
  const float a_js = use_js ? gs * w_js / (log2f((float)K) * nmask) : 0.f;
  float v[KMAX];
  const float m = load_row_max(logits + (size_t)n * ldl, K, v);
  const float sum = exp_sum_row<KEEP_SHIFTED>(v, m, K);
  const float lsum = logf(sum);
  const PixelLabel l = classify(labels[n], K);
  const float fm = l.mask ? 1.f : 0.f;
  // r[k] = d(a_reg*MRENT + a_js*JS)/dp_k of this pixel; its softmax Jacobian is p_k (r_k - sum_j p_j r_j)
  float r[KMAX];
  float pt = 0.f, pr = 0.f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) {
      const float lp = v[k] - lsum;
      v[k] = expf(v[k]) / sum;  // p, as the forward pass has it
      if (k == l.cls) pt = v[k];
      float rk = reg_kind == REG_MRENT ? a_reg * lp : 0.f;
      if (use_js) {
        const float y = (l.mask && k == l.cls) ? 1.f : JS_FLOOR;
        const float mp = v[k] * fm;
        const float a = (y + mp) / 2.f;
        rk += a_js * (0.5f * (dxlog2x(mp) - dxlog2x(a))) * fm;
      }
      r[k] = rk;
      pr += v[k] * rk;
    }
  float* out = dl + (size_t)n * ldl;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k >= ldl) break;
    float g = 0.f;
    if (k < K) {
      g = ce_rce_grad(coef, l, k, v[k], pt);
      if (reg_kind == REG_MRKLD) g += a_reg * ((float)K * v[k] - 1.f);
      g += v[k] * (r[k] - pr);
    }
    out[k] = g;
  }
}

// ---- soft-label CE + RCE + (MRKLD | MRENT) ---------------------------------------------------------
// The SOFT_LABELS branch of prototypes.py:305-322 (loss.py:12-13, :32-34, :95-99): the target t[N][K] is the prototype soft
// map.  CE = -sum_k tc_k log(x_k + 1e-6) / N over the RAW logits x, as the reference writes it -- every entry is formed, so
// a negative x_k + 1e-6 gives NaN and a zero one -inf whatever tc_k is (0 * NaN = NaN) -- with tc = trunc(t) on the step's
// path (func.loss_calc's .long()) and tc = t for cross_entropy_2d called directly.  RCE = -sum_k p_k log(t_k + 1e-6) / N
// with the real soft values.  The regulariser is target_loss's.  Both normalisers are N: the backward pass needs nothing
// from the forward pass.
__device__ __forceinline__ float soft_ce_target(float t, int ce_trunc) { return ce_trunc ? truncf(t) : t; }

__global__ __launch_bounds__(256) void soft_loss_fwd_kernel(const float* __restrict__ logits, int ldl,
                                                            const float* __restrict__ soft, int lds, int ce_trunc,
                                                            int reg_kind, float* __restrict__ ws, int64_t N, int K) {
  __shared__ float red[3 * 4];
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float part[3] = {0.f, 0.f, 0.f};  // ce, rce, reg
  if (n < N) {
    float v[KMAX];
    const float* trow = soft + (size_t)n * lds;
    const float m = load_row_max(logits + (size_t)n * ldl, K, v);
    float ce = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) ce += soft_ce_target(trow[k], ce_trunc) * logf(v[k] + 1e-6f);  // no entry skipped: 0 * NaN stays NaN
    const float sum = exp_sum_row<KEEP_SHIFTED>(v, m, K);
    const float lsum = logf(sum);
    float rce = 0.f, reg = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        const float lp = v[k] - lsum;
        const float p = expf(v[k]) / sum;
        rce += p * logf(trow[k] + 1e-6f);
        if (reg_kind == REG_MRKLD) reg -= lp;
        if (reg_kind == REG_MRENT) reg += p * lp;
      }
    part[0] = -ce;
    part[1] = -rce;
    part[2] = reg;
  }
  block_partials(part, red, ws);
}

// result = {ce, rce, reg, total, 0, 0, 0, 0}
__global__ void soft_loss_finalize_kernel(const float* __restrict__ ws, int nblocks, int reg_kind, int64_t N, int K,
                                          float w_ce, float w_rce, float w_reg, float* __restrict__ result) {
  if (threadIdx.x != 0) return;
  double s[3];
  sum_block_partials(ws, nblocks, s);
  const double ce = s[0] / (double)N;
  const double rce = s[1] / (double)N;
  const double reg = reg_kind == REG_MRKLD ? s[2] / ((double)N * K) : reg_kind == REG_MRENT ? s[2] / (double)N : 0.0;
  // only the terms with a weight enter the total: the reference does not compute the others, and 0 * NaN would be NaN
  double total = 0.0;
  if (w_ce != 0.f) total += (double)w_ce * ce;
  if (w_rce != 0.f) total += (double)w_rce * rce;
  if (w_reg != 0.f) total += (double)w_reg * reg;
  result[0] = (float)ce;
  result[1] = (float)rce;
  result[2] = (float)reg;
  result[3] = (float)total;
  result[4] = result[5] = result[6] = result[7] = 0.f;
}

__global__ __launch_bounds__(256) void soft_loss_bwd_kernel(const float* __restrict__ logits, int ldl,
                                                            const float* __restrict__ soft, int lds, int ce_trunc,
                                                            int reg_kind, const float* __restrict__ gscale, float w_ce,
                                                            float w_rce, float w_reg, float* __restrict__ dl, int64_t N,
                                                            int K) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const float gs = gscale ? gscale[0] : 1.f;
  const bool use_ce = w_ce != 0.f, use_rce = w_rce != 0.f, use_reg = w_reg != 0.f && reg_kind != REG_NONE;
  const float a_ce = gs * w_ce / (float)N;
  const float a_rce = gs * w_rce / (float)N;
  const float a_reg = reg_kind == REG_MRKLD ? gs * w_reg / ((float)N * (float)K) : gs * w_reg / (float)N;
  float v[KMAX], c[KMAX], g[KMAX];
  const float* trow = soft + (size_t)n * lds;
  const float m = load_row_max(logits + (size_t)n * ldl, K, v);
  // CE: autograd's log backward on the raw logit, -(a * tc) / (x + 1e-6) as written: 0/0 = NaN and -inf where the
  // reference has them; without a weight the term is not formed at all
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) {
      const float t = trow[k];
      g[k] = use_ce ? -(a_ce * soft_ce_target(t, ce_trunc)) / (v[k] + 1e-6f) : 0.f;
      c[k] = logf(t + 1e-6f);
    }
  const float sum = exp_sum_row<KEEP_SHIFTED>(v, m, K);
  const float lsum = logf(sum);
  // r[k] = d(a_rce*RCE + a_reg*MRENT)/dp_k of this pixel, kept in c; its softmax Jacobian is p_k (r_k - sum_j p_j r_j)
  float pr = 0.f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) {
      const float lp = v[k] - lsum;
      v[k] = expf(v[k]) / sum;  // p, as the forward pass has it
      float rk = use_rce ? -a_rce * c[k] : 0.f;
      if (use_reg && reg_kind == REG_MRENT) rk += a_reg * lp;
      c[k] = rk;
      pr += v[k] * rk;
    }
  float* out = dl + (size_t)n * ldl;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k >= ldl) break;
    float gk = 0.f;
    if (k < K) {
      gk = g[k] + v[k] * (c[k] - pr);
      if (use_reg && reg_kind == REG_MRKLD) gk += a_reg * ((float)K * v[k] - 1.f);
    }
    out[k] = gk;
  }
}

// ---- prototypes ---------------------------------------------------------------------------
__global__ void proto_sigma_kernel(const float* __restrict__ proto, const float* __restrict__ sqmean,
                                   const float* __restrict__ counter, float* __restrict__ sigma, int K, int C) {
  const int ch = blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= C) return;
  float total = 0.f;
  for (int k = 0; k < K; ++k) total += counter[k];
  float gsq = 0.f, gm = 0.f;
  for (int k = 0; k < K; ++k) {
    gsq += sqmean[(size_t)k * C + ch] * counter[k] / total;
    gm += proto[(size_t)k * C + ch] * counter[k] / total;
  }
  sigma[ch] = sqrtf(gsq - gm * gm);
}

// ---- the steps the direct kernels share: one wave per pixel, lane l owns channels 4l..4l+3 (C == 256) ------------------------
// sp[K][256] = the prototypes, for the whole workgroup of 256 threads (16-byte copies)
__device__ __forceinline__ void stage_prototypes(float* sp, const float* __restrict__ proto, int K) {
  for (int i = threadIdx.x; i < K * 64; i += 256) reinterpret_cast<f32x4*>(sp)[i] = reinterpret_cast<const f32x4*>(proto)[i];
  __syncthreads();
}
// this lane's four sigmas; ones for the Euclidean metric
__device__ __forceinline__ f32x4 lane_sigma(const float* __restrict__ sigma, int mahalanobis, int lane) {
  f32x4 sg = {1.f, 1.f, 1.f, 1.f};
  if (mahalanobis) sg = *reinterpret_cast<const f32x4*>(sigma + lane * 4);
  return sg;
}
// |f - p_k| (per channel / sigma for Mahalanobis) over the wave's 256 channels, in every lane
__device__ __forceinline__ float proto_distance(const f32x4 f, const f32x4 sg, int mahalanobis, const float* sp, int k, int lane) {
  f32x4 df = f - reinterpret_cast<const f32x4*>(sp)[k * 64 + lane];
  if (mahalanobis) df = df / sg;
  return sqrtf(wave_sum(df[0] * df[0] + df[1] * df[1] + df[2] * df[2] + df[3] * df[3]));
}

// The posterior of one pixel from its K distances, in place: d[k] = softmax(-(d - dmin) / tau), times the prior when there is
// one, renormalised.  conf = max softmax, prmax = max prior, best = the first maximum of the posterior at class arg, second =
// the runner-up (RUNNER_UP only).  ONE definition for both assign kernels: the direct kernel redoes exactly the pixels the
// MFMA kernel does not trust, and has to decide them the same way.
struct Posterior {
  float conf, prmax, best, second;
  int arg;
};
template <bool RUNNER_UP>
__device__ __forceinline__ Posterior posterior(float* d, float dmin, float tau, bool has_prior, const float* pr, int K) {
  Posterior o = {0.f, 0.f, -INFINITY, -INFINITY, 0};
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) {
      d[k] = expf(-(d[k] - dmin) / tau);
      sum += d[k];
    }
  float psum = 0.f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) {
      float p = d[k] / sum;
      o.conf = fmaxf(o.conf, p);
      if (has_prior) {
        o.prmax = fmaxf(o.prmax, pr[k]);
        p *= pr[k];
      }
      d[k] = p;
      psum += p;
    }
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) {
      d[k] = d[k] / psum;
      if (d[k] > o.best) {
        if constexpr (RUNNER_UP) o.second = o.best;
        o.best = d[k];
        o.arg = k;
      } else if constexpr (RUNNER_UP) {
        if (d[k] > o.second) o.second = d[k];
      }
    }
  return o;
}

// ws[block][t] = sum over the workgroup's WAVES waves of the t-th of three per-wave values (held by lane 0), in wave order
template <int WAVES>
__device__ __forceinline__ void block_sum3(float a, float b, float c, float (*red)[WAVES], float* __restrict__ ws) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (lane == 0) {
    red[0][wave] = a;
    red[1][wave] = b;
    red[2][wave] = c;
  }
  __syncthreads();
  if (t < 3) {
    float s = 0.f;
#pragma unroll
    for (int w_ = 0; w_ < WAVES; ++w_) s += red[t][w_];
    ws[(size_t)blockIdx.x * 3 + t] = s;
  }
}

// The distance matrix by itself (prototype_handler.distance / mahalanobis_distance, :111-138): dist[n][k] = D[k] - min_k D,
// the direct form of proto_assign_kernel.
__global__ __launch_bounds__(256) void proto_distances_kernel(const float* __restrict__ feat, int ldf,
                                                              const float* __restrict__ proto,
                                                              const float* __restrict__ sigma, int mahalanobis,
                                                              float* __restrict__ dist, int64_t N, int K) {
  __shared__ __attribute__((aligned(16))) float sp[KMAX * 256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  stage_prototypes(sp, proto, K);
  const f32x4 sg = lane_sigma(sigma, mahalanobis, lane);
  for (int64_t n = (int64_t)blockIdx.x * 4 + wave; n < N; n += (int64_t)gridDim.x * 4) {
    const f32x4 f = *reinterpret_cast<const f32x4*>(feat + (size_t)n * ldf + lane * 4);
    float mine = 0.f, dmin = INFINITY;  // (no d[KMAX] here: lane k keeps the k-th distance only)
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        const float d = proto_distance(f, sg, mahalanobis, sp, k, lane);
        dmin = fminf(dmin, d);
        if (k == lane) mine = d;
      }
    if (lane < K) dist[(size_t)n * K + lane] = mine - dmin;
  }
}

__global__ __launch_bounds__(256) void proto_assign_kernel(const float* __restrict__ feat, int ldf,
                                                           const float* __restrict__ prior, int ldp,
                                                           const float* __restrict__ proto,
                                                           const float* __restrict__ sigma, int mahalanobis,
                                                           float tau, float thresh, int64_t* __restrict__ labels,
                                                           float* __restrict__ soft, float* __restrict__ ws, int64_t N,
                                                           int K, const int* __restrict__ list = nullptr,
                                                           const int* __restrict__ list_len = nullptr) {
  // (list != nullptr: only the pixels list[0 .. *list_len) -- the close decisions of proto_assign_mfma_kernel)
  __shared__ __attribute__((aligned(16))) float sp[KMAX * 256];
  __shared__ float red[3][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  stage_prototypes(sp, proto, K);
  const f32x4 sg = lane_sigma(sigma, mahalanobis, lane);
  float a_conf = 0.f, a_soft = 0.f, a_prior = 0.f;
  const int64_t wstride = (int64_t)gridDim.x * 4;
  const int64_t count = list ? (int64_t)*list_len : N;
  for (int64_t i_ = (int64_t)blockIdx.x * 4 + wave; i_ < count; i_ += wstride) {
    const int64_t n = list ? (int64_t)list[i_] : i_;
    const f32x4 f = *reinterpret_cast<const f32x4*>(feat + (size_t)n * ldf + lane * 4);
    float d[KMAX];
    float dmin = INFINITY;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        d[k] = proto_distance(f, sg, mahalanobis, sp, k, lane);
        dmin = fminf(dmin, d[k]);
      }
    const Posterior o = posterior<false>(d, dmin, tau, prior != nullptr, prior ? prior + (size_t)n * ldp : nullptr, K);
    if (lane == 0) labels[n] = o.best < thresh ? 255 : o.arg;
    if (soft) {
      float mine = 0.f;
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K && k == lane) mine = d[k];
      if (lane < K) soft[(size_t)n * K + lane] = mine;
    }
    a_conf += o.conf;
    a_soft += o.best;
    a_prior += o.prmax;
  }
  block_sum3(a_conf, a_soft, a_prior, red, ws);
}

// ---- the same assignment with the feature <-> prototype contraction on the matrix cores -------------------------------------
//   D^2[n][k] = |g_n|^2 - 2 g_n.q_k + |q_k|^2,   g_n = (f_n - c)/s,   q_k = (p_k - c)/s,
// with the [N x 256] x [256 x K<=32] product g.q on v_mfma_f32_32x32x2_f32
// (fp32 operands, fp32 accumulate: exact products).  A wave takes 32 pixels: their scaled features are staged through LDS
// in two 128-channel halves (coalesced 16-byte loads, rows padded to 129 floats: conflict-free operand reads), the scaled
// prototypes live in LDS for the whole workgroup (rows of 257 floats).  K order: MFMA step s of a half multiplies channel
// s (lanes 0-31) and channel 64+s (lanes 32-63) -- any order is a valid order of the sum.  The accumulator tile goes
// through LDS once more so that lane p < 32 holds pixel p's K products and runs the softmax / prior / argmax / threshold
// exactly like the direct kernel above.
// c[256] is ONE point subtracted from every feature and every prototype before the expansion -- distances are translation-
// invariant -- namely the unweighted mean of the K prototypes, summed per channel in class order by every workgroup (the same
// bits in every workgroup and launch).  Without it the three terms have the size of |f/s|^2, and a common offset of the
// channels (post-ReLU features have one) costs the difference ~2^-24 |f/s|^2 / D: 1e-3 of the soft map at an offset of 32.
// Centred, the terms have the size of the spread around the prototypes.  What remains: the error scales with
// |f - c|^2 / D, so a feature far from ALL prototypes and almost at one of them is still resolved worse than by the direct form.
// The product of each 128-channel half is accumulated from zero and the two halves are added at the end: for a pixel at a
// prototype g.q_k grows to |q_k|^2, and one chain over all 256 channels rounds at that size 128 times -- a Euclidean soft map
// at 1.3e-5 of float64 where two chains of 64 steps stay at 4.8e-6 (tests/proto_fp64.py, case off32-eucl).
// The expanded form cancels where the direct form (what the reference computes, prototype_handler.py:111-138) does
// not: its distances carry an absolute error of ~1e-5.  Decisions that close are not trusted: a pixel whose two largest
// posteriors, or whose largest posterior and the threshold, lie within `margin` goes on a list and is redone by the
// direct kernel (proto_assign_list_kernel); everything else -- labels, soft map, monitor sums -- is final here.
constexpr int PA_TS = 129, PA_PS = 257, PA_GS = 33;
constexpr int PA_WAVES = 6;  // 33 KB of prototypes + 6 x 16.6 KB of feature tiles = 133 KB: one workgroup per CU; 1 536 waves
                             // take the 1 049 pixel blocks of a 65 x 129 x 4 grid in ONE round (four waves per CU: two)
constexpr int PA_WAVE_FLOATS = 32 * PA_TS + 32;  // a wave's half-tile + its 32 squared feature norms

__global__ __launch_bounds__(64 * PA_WAVES) void proto_assign_mfma_kernel(const float* __restrict__ feat, int ldf,
                                                                const float* __restrict__ prior, int ldp,
                                                                const float* __restrict__ proto,
                                                                const float* __restrict__ sigma, int mahalanobis, float tau,
                                                                float thresh, float margin, int64_t* __restrict__ labels,
                                                                float* __restrict__ soft, float* __restrict__ ws,
                                                                int* __restrict__ flagged, int* __restrict__ nflagged,
                                                                int64_t N, int K) {
  __shared__ float sm[32 * PA_PS + 32 + PA_WAVES * PA_WAVE_FLOATS];
  __shared__ float red[3][PA_WAVES];
  __shared__ __attribute__((aligned(16))) float cen[256];  // c: the unweighted mean prototype
  float* ph = sm;                // [32][PA_PS]: (prototypes - c) / sigma, rows >= K zero
  float* pn = sm + 32 * PA_PS;   // [32]: their squared norms
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  float* tile = pn + 32 + wave * PA_WAVE_FLOATS;  // [32][PA_TS], later the product tile [32][PA_GS]
  for (int i = t; i < 32 * 256; i += 64 * PA_WAVES) {
    const int k = i >> 8, ch = i & 255;
    ph[k * PA_PS + ch] = k < K ? proto[k * 256 + ch] : 0.f;
  }
  __syncthreads();
  if (t < 256) {  // one thread per channel, classes in order: every workgroup of every launch gets the same c
    float a = 0.f;
    for (int k = 0; k < K; ++k) a += ph[k * PA_PS + t];
    cen[t] = a / (float)K;
  }
  __syncthreads();
  for (int i = t; i < K * 256; i += 64 * PA_WAVES) {
    const int k = i >> 8, ch = i & 255;
    const float v = ph[k * PA_PS + ch] - cen[ch];
    ph[k * PA_PS + ch] = mahalanobis ? v / sigma[ch] : v;
  }
  __syncthreads();
  if (t < 256) {  // squared norms: 8 threads per class, 32 channels each, fixed order
    const int k = t >> 3, part = t & 7;
    float a = 0.f;
#pragma unroll 8
    for (int ch = part * 32; ch < part * 32 + 32; ++ch) a += ph[k * PA_PS + ch] * ph[k * PA_PS + ch];
    a += __shfl_xor(a, 1, 64);
    a += __shfl_xor(a, 2, 64);
    a += __shfl_xor(a, 4, 64);
    if (part == 0) pn[k] = a;
  }
  __syncthreads();
  const int half_lane = lane >> 5, l32 = lane & 31;
  float a_conf = 0.f, a_soft = 0.f, a_prior = 0.f;
  const int64_t nblocks = (N + 31) / 32;
  for (int64_t blk = (int64_t)blockIdx.x * PA_WAVES + wave; blk < nblocks; blk += (int64_t)gridDim.x * PA_WAVES) {
    const int64_t n0 = blk * 32;
    float f2 = 0.f;  // lanes 0-31: squared norm of pixel l32's scaled features
    f32x16 acc, acc_h0;  // each 128-channel half accumulates from zero (see the header comment); acc_h0 keeps the first
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    // this lane's pixel's priors, requested now, used after the contraction
    float pr_[KMAX];
    {
      const int64_t n = n0 + l32;
#pragma unroll
      for (int k = 0; k < KMAX; ++k) pr_[k] = (prior != nullptr && k < K && n < N && half_lane == 0) ? prior[(size_t)n * ldp + k] : 1.f;
    }
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
      f32x4 sg = {1.f, 1.f, 1.f, 1.f};  // 1 / sigma (a reciprocal, not the direct kernel's division: close decisions are redone there)
      if (mahalanobis) sg = f32x4{1.f, 1.f, 1.f, 1.f} / *reinterpret_cast<const f32x4*>(sigma + half * 128 + l32 * 4);
      const f32x4 cv = *reinterpret_cast<const f32x4*>(cen + half * 128 + l32 * 4);
      // stage 32 pixels x 128 channels: a 16-byte load per lane covers two pixel rows per instruction; all 16 loads of
      // the half go out before the first is used (a wave has about one block: nothing else hides the latency)
      f32x4 fv[16];
#pragma unroll
      for (int it = 0; it < 16; ++it) {
        const int64_t n = n0 + 2 * it + half_lane;
        fv[it] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (n < N) fv[it] = *reinterpret_cast<const f32x4*>(feat + (size_t)n * ldf + half * 128 + l32 * 4);
      }
#pragma unroll
      for (int it = 0; it < 16; ++it) {
        const int row = 2 * it + half_lane;
        const f32x4 v = (fv[it] - cv) * sg;
        float* dst = tile + row * PA_TS + l32 * 4;
        dst[0] = v[0];
        dst[1] = v[1];
        dst[2] = v[2];
        dst[3] = v[3];
      }
      __builtin_amdgcn_wave_barrier();  // one wave: its LDS instructions execute in order
      if (half_lane == 0) {  // the pixel's squared norm from its staged row (conflict-free reads, no cross-lane traffic)
        float a0 = 0.f, a1 = 0.f;
#pragma unroll 8
        for (int ch = 0; ch < 128; ch += 2) {
          const float x0 = tile[l32 * PA_TS + ch], x1 = tile[l32 * PA_TS + ch + 1];
          a0 += x0 * x0;
          a1 += x1 * x1;
        }
        f2 += a0 + a1;
      }
      const float* ap = tile + l32 * PA_TS + half_lane * 64;
      const float* bp = ph + l32 * PA_PS + half * 128 + half_lane * 64;
#pragma unroll 8
      for (int s_ = 0; s_ < 64; ++s_) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[s_], bp[s_], acc, 0, 0, 0);
      __builtin_amdgcn_wave_barrier();
      if (half == 0) {
        acc_h0 = acc;
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[v] = 0.f;
      }
    }
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] += acc_h0[v];
    // accumulator (row 8*(v/4) + 4*(lane/32) + v%4, column lane%32) -> [pixel][class] in LDS
#pragma unroll
    for (int v = 0; v < 16; ++v) tile[(8 * (v >> 2) + 4 * half_lane + (v & 3)) * PA_GS + l32] = acc[v];
    __builtin_amdgcn_wave_barrier();
    const int64_t n = n0 + l32;
    if (half_lane == 0 && n < N) {
      float d[KMAX];
      float dmin = INFINITY;
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) {
          d[k] = sqrtf(fmaxf(f2 + pn[k] - 2.f * tile[l32 * PA_GS + k], 0.f));
          dmin = fminf(dmin, d[k]);
        }
      const Posterior o = posterior<true>(d, dmin, tau, prior != nullptr, pr_, K);
      if (o.best - o.second < margin || fabsf(o.best - thresh) < margin || !(o.best == o.best)) {
        flagged[atomicAdd(nflagged, 1)] = (int)n;  // redone in the direct form
      } else {
        labels[n] = o.best < thresh ? 255 : o.arg;
        if (soft) {
#pragma unroll
          for (int k = 0; k < KMAX; ++k)
            if (k < K) soft[(size_t)n * K + k] = d[k];
        }
        a_conf += o.conf;
        a_soft += o.best;
        a_prior += o.prmax;
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  block_sum3(wave_sum(a_conf), wave_sum(a_soft), wave_sum(a_prior), red, ws);
}

constexpr int SUMS_BLOCKS = 256;

__global__ __launch_bounds__(256) void proto_class_sums_kernel(const float* __restrict__ feat, int ldf,
                                                               const int32_t* __restrict__ cls,
                                                               float* __restrict__ ws, int64_t N, int C, int K,
                                                               int64_t rows_per_block) {
  extern __shared__ float acc[];  // [2][K][C] + [K]
  float* cnt = acc + (size_t)2 * K * C;
  const int t = threadIdx.x;
  for (int i = t; i < 2 * K * C + K; i += 256) acc[i] = 0.f;
  __syncthreads();
  const int64_t n0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t n1 = min(N, n0 + rows_per_block);
  for (int64_t n = n0; n < n1; ++n) {
    const int k = cls[n];
    if ((unsigned)k >= (unsigned)K) continue;
    for (int ch = t; ch < C; ch += 256) {
      const float v = feat[(size_t)n * ldf + ch];
      acc[(size_t)k * C + ch] += v;
      acc[(size_t)(K + k) * C + ch] += v * v;
    }
    if (t == 0) cnt[k] += 1.f;
  }
  __syncthreads();
  float* dst = ws + (size_t)blockIdx.x * (2 * K * C + K);
  for (int i = t; i < 2 * K * C + K; i += 256) dst[i] = acc[i];
}

__global__ void proto_sums_finalize_kernel(const float* __restrict__ ws, int nblocks, int KC2, int K,
                                           float* __restrict__ sums, float* __restrict__ counts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= KC2 + K) return;
  float s = 0.f;
  for (int b = 0; b < nblocks; ++b) s += ws[(size_t)b * (KC2 + K) + i];
  if (i < KC2)
    sums[i] = s;
  else
    counts[i - KC2] = s;
}

__global__ void proto_ema_kernel(float* __restrict__ proto, float* __restrict__ sqmean, const float* __restrict__ sums,
                                 const float* __restrict__ counts, float lam, int K, int C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= K * C) return;
  const int k = i / C;
  const float n = counts[k];
  const float keep = n > 0.f ? lam : 1.f;
  const float denom = n > 0.f ? n : 1.f;
  proto[i] = proto[i] * keep + (1.f - keep) * (sums[i] / denom);
  sqmean[i] = sqmean[i] * keep + (1.f - keep) * (sums[(size_t)K * C + i] / denom);
}

__global__ void proto_append_kernel(float* __restrict__ proto, float* __restrict__ sqmean, float* __restrict__ counter,
                                    const float* __restrict__ sums, const float* __restrict__ counts, int K, int C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= K * C) return;
  const int k = i / C;
  const float n = counts[k];
  const float tot = counter[k] + n;
  const float denom = tot > 0.f ? tot : 1.f;
  proto[i] += (sums[i] - proto[i] * n) / denom;
  sqmean[i] += (sums[(size_t)K * C + i] - sqmean[i] * n) / denom;
}
__global__ void proto_append_counter_kernel(float* __restrict__ counter, const float* __restrict__ counts, int K) {
  const int k = threadIdx.x;
  if (k < K) counter[k] += counts[k];
}

// ---- multi-tensor optimizer / teacher ---------------------------------------------------------
// FLAT launches (see pack_h2_multi_kernel): an entry owns the blocks [first_block, first_block + ceil(n / MT_BLOCK)) of a 1-D
// grid and is found by bisection (common.h mt_entry_of) -- a (largest tensor) x (217 tensors) grid is nine tenths empty workgroups.
constexpr int MT_BLOCK = 4096;  // elements per workgroup: four 16-byte vectors per thread
// The entry that owns this workgroup and its element range [i0, i1) of it
template <class E>
__device__ __forceinline__ E mt_block(const E* __restrict__ table, int n_entries, int64_t& i0, int64_t& i1) {
  const E e = table[mt_entry_of(table, n_entries, blockIdx.x)];
  i0 = (int64_t)(blockIdx.x - e.first_block) * MT_BLOCK;
  i1 = i0 + MT_BLOCK < e.n ? i0 + MT_BLOCK : e.n;
  return e;
}
// a full block of tensors that all start on a 16-byte boundary: four f32x4 per thread; anything else goes element by element
__device__ __forceinline__ bool mt_vector_block(int64_t i0, int64_t i1, const void* a, const void* b, const void* c = nullptr) {
  return ((reinterpret_cast<size_t>(a) | reinterpret_cast<size_t>(b) | reinterpret_cast<size_t>(c)) & 15) == 0 && i1 - i0 == MT_BLOCK;
}

__device__ __forceinline__ void sgd_one(float& p, float& b, float g, float lr, float momentum, float wd, int times, int fresh) {
  if (fresh) b = 0.f;
  for (int r = 0; r < times; ++r) {
    const float d = g + wd * p;
    b = fresh ? d : b * momentum + d;
    p = p - lr * b;
  }
}

// ---- EWC anchor (utils/ewc.py:47-54 with unit Fisher weights; prototypes.py:334-336) ----------------------------------------
// The penalty's gradient, as autograd leaves it in .grad under upstream 1, added to the scaled gradient: three roundings and
// one more for the sum, none of them fused (a fused multiply-add would skip the rounding of the product that ATen's
// elementwise kernels make).  The factors -2 are exact.
__device__ __forceinline__ float anchored_grad(float g, float grad_scale, float half_lambda, float anchor, float p) {
#pragma clang fp contract(off)
  const float d = anchor - p;
  const float h = half_lambda * d;
  const float c = -2.f * h;
  const float gs = g * grad_scale;
  return gs + c;
}

// One block of one entry, for both optimizer launches: an OndaSgdEntry, and an OndaSgdAnchorEntry without an anchor, take
// ANCHORED = false -- one expression, so the anchored launch updates an un-anchored entry with the bits onda_sgd_multi gives it.
// grad_scale: every gradient element is multiplied by it on the way in (1 / world: the exchanged buffer holds rank SUMS, the
// division never becomes a pass of its own over 184 MB)
template <bool ANCHORED, class Entry>
__device__ __forceinline__ void sgd_block(const Entry& e, int64_t i0, int64_t i1, float momentum, float wd, float grad_scale,
                                          float half_lambda) {
  bool vec = mt_vector_block(i0, i1, e.p, e.g, e.buf);
  if constexpr (ANCHORED) vec = vec && (reinterpret_cast<size_t>(e.anchor) & 15) == 0;
  if (vec) {
#pragma unroll
    for (int k = 0; k < MT_BLOCK / 1024; ++k) {
      const int64_t i = i0 + (k * 256 + threadIdx.x) * 4;
      f32x4 p = *reinterpret_cast<const f32x4*>(e.p + i), b = e.fresh ? f32x4{0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const f32x4*>(e.buf + i);
      const f32x4 g = !ANCHORED || e.g ? *reinterpret_cast<const f32x4*>(e.g + i) : f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      if constexpr (ANCHORED) a = *reinterpret_cast<const f32x4*>(e.anchor + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = p[j], bj = b[j];
        if (ANCHORED)
          sgd_one(pj, bj, anchored_grad(g[j], grad_scale, half_lambda, a[j], pj), e.lr, momentum, wd, e.times, e.fresh);
        else
          sgd_one(pj, bj, g[j] * grad_scale, e.lr, momentum, wd, e.times, e.fresh);
        p[j] = pj;
        b[j] = bj;
      }
      *reinterpret_cast<f32x4*>(e.p + i) = p;
      *reinterpret_cast<f32x4*>(e.buf + i) = b;
    }
    return;
  }
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    float p = e.p[i], b = e.fresh ? 0.f : e.buf[i];
    if constexpr (ANCHORED)
      sgd_one(p, b, anchored_grad(e.g ? e.g[i] : 0.f, grad_scale, half_lambda, e.anchor[i], p), e.lr, momentum, wd, e.times, e.fresh);
    else
      sgd_one(p, b, e.g[i] * grad_scale, e.lr, momentum, wd, e.times, e.fresh);
    e.p[i] = p;
    e.buf[i] = b;
  }
}

__global__ __launch_bounds__(256) void sgd_multi_kernel(const OndaSgdEntry* __restrict__ table, int n_entries, float momentum,
                                                        float wd, float grad_scale) {
  int64_t i0, i1;
  const OndaSgdEntry e = mt_block(table, n_entries, i0, i1);
  sgd_block<false>(e, i0, i1, momentum, wd, grad_scale, 0.f);
}

__global__ __launch_bounds__(256) void sgd_anchor_multi_kernel(const OndaSgdAnchorEntry* __restrict__ table, int n_entries,
                                                               float momentum, float wd, float grad_scale, float half_lambda) {
  int64_t i0, i1;
  const OndaSgdAnchorEntry e = mt_block(table, n_entries, i0, i1);
  if (e.anchor)
    sgd_block<true>(e, i0, i1, momentum, wd, grad_scale, half_lambda);
  else
    sgd_block<false>(e, i0, i1, momentum, wd, grad_scale, half_lambda);
}

// The penalty's value: one float32 partial per workgroup (differences and squares in float32, as the reference has them) ...
__global__ __launch_bounds__(256) void sqdiff_multi_kernel(const OndaSqdiffEntry* __restrict__ table, int n_entries,
                                                           float* __restrict__ ws) {
  __shared__ float red[4];
  int64_t i0, i1;
  const OndaSqdiffEntry e = mt_block(table, n_entries, i0, i1);
  float acc = 0.f;
  if (mt_vector_block(i0, i1, e.a, e.b)) {
#pragma unroll
    for (int k = 0; k < MT_BLOCK / 1024; ++k) {
      const int64_t i = i0 + (k * 256 + threadIdx.x) * 4;
      const f32x4 d = *reinterpret_cast<const f32x4*>(e.a + i) - *reinterpret_cast<const f32x4*>(e.b + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc += d[j] * d[j];
    }
  } else {
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
      const float d = e.a[i] - e.b[i];
      acc += d * d;
    }
  }
  const float r = block_sum_256(acc, red);
  if (threadIdx.x == 0) ws[blockIdx.x] = r;
}
// ... and their sum in a fixed order, in double: thread t takes the partials t, t + 256, ..., then a fixed tree over the threads
__global__ __launch_bounds__(256) void sqdiff_finalize_kernel(const float* __restrict__ ws, int64_t nblocks, float half_lambda,
                                                              float* __restrict__ result) {
  __shared__ double sh[256];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int64_t b = t; b < nblocks; b += 256) s += (double)ws[b];
  sh[t] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) sh[t] += sh[t + o];
    __syncthreads();
  }
  if (t == 0) result[0] = (float)((double)half_lambda * sh[0]);
}

__global__ __launch_bounds__(256) void ema_multi_kernel(const OndaEmaEntry* __restrict__ table, int n_entries) {
  int64_t i0, i1;
  const OndaEmaEntry e = mt_block(table, n_entries, i0, i1);
  if (mt_vector_block(i0, i1, e.k, e.q)) {
#pragma unroll
    for (int k = 0; k < MT_BLOCK / 1024; ++k) {
      const int64_t i = i0 + (k * 256 + threadIdx.x) * 4;
      *reinterpret_cast<f32x4*>(e.k + i) = *reinterpret_cast<const f32x4*>(e.k + i) * e.keep + *reinterpret_cast<const f32x4*>(e.q + i) * e.blend;
    }
    return;
  }
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) e.k[i] = e.k[i] * e.keep + e.q[i] * e.blend;
}

// a[i] <-> b[i] as 4-byte integer words (no float ever touches them: NaN payloads, -0.0 and the halves of an int64 survive).
// A thread holds both of its words (vectors) before it stores either; the ranges of a table are pairwise disjoint (the caller's
// contract), so no other thread reads what it writes.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void swap_multi_kernel(const OndaSwapEntry* __restrict__ table, int n_entries) {
  int64_t i0, i1;
  const OndaSwapEntry e = mt_block(table, n_entries, i0, i1);
  if (mt_vector_block(i0, i1, e.a, e.b)) {
#pragma unroll
    for (int k = 0; k < MT_BLOCK / 1024; ++k) {
      const int64_t i = i0 + (k * 256 + threadIdx.x) * 4;
      const u32x4 va = *reinterpret_cast<const u32x4*>(e.a + i), vb = *reinterpret_cast<const u32x4*>(e.b + i);
      *reinterpret_cast<u32x4*>(e.a + i) = vb;
      *reinterpret_cast<u32x4*>(e.b + i) = va;
    }
    return;
  }
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    const uint32_t wa = e.a[i], wb = e.b[i];
    e.a[i] = wb;
    e.b[i] = wa;
  }
}

// The entry points with one thread per pixel: the argument checks they share; the grid of 256-thread workgroups, or 0
int pixel_blocks(const float* logits, const void* out, int64_t N, int K) {
  return logits && out && K >= 1 && K <= KMAX && N >= 1 ? (int)((N + 255) / 256) : 0;
}
bool is_regularizer(int r) { return r >= REG_NONE && r <= REG_MRENT; }
// these kernels read and write single floats: the siblings' rule, a pointer at a float boundary
bool float_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

extern "C" {

int onda_softmax_stats(const float* logits, int ldl, float* probs, int ldp, int32_t* argmax, float* result, float* ws,
                       int64_t N, int K, onda_stream_t s) {
  const int nb = pixel_blocks(logits, result, N, K);
  ONDA_REQUIRE(nb && ws);
  hipLaunchKernelGGL(softmax_stats_kernel, dim3(nb), dim3(256), 0, ONDA_STREAM(s), logits, ldl, probs, ldp, argmax, ws,
                     N, K);
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(64), 0, ONDA_STREAM(s), ws, nb, 1, (float)(1.0 / (double)N),
                     result);
  return ONDA_LAUNCH_RESULT();
}

int onda_seg_loss_fwd(const float* logits, int ldl, const int64_t* labels, float* result, float* ws, int64_t N, int K,
                      onda_stream_t s) {
  const int nb = pixel_blocks(logits, result, N, K);
  ONDA_REQUIRE(nb && labels && ws);
  hipLaunchKernelGGL(seg_loss_fwd_kernel, dim3(nb), dim3(256), 0, ONDA_STREAM(s), logits, ldl, labels, ws, N, K);
  hipLaunchKernelGGL(seg_loss_finalize_kernel, dim3(1), dim3(64), 0, ONDA_STREAM(s), ws, nb, (double)N * K, result);
  return ONDA_LAUNCH_RESULT();
}

int onda_seg_loss_bwd(const float* logits, int ldl, const int64_t* labels, const float* result, const float* gscale,
                      float w_ce, float w_rce, float w_reg, float* dlogits, int64_t N, int K, onda_stream_t s) {
  const int nb = pixel_blocks(logits, dlogits, N, K);
  ONDA_REQUIRE(nb && labels && result && ldl <= KMAX);
  hipLaunchKernelGGL(seg_loss_bwd_kernel, dim3(nb), dim3(256), 0, ONDA_STREAM(s), logits, ldl, labels, result, gscale,
                     w_ce, w_rce, w_reg, dlogits, N, K);
  return ONDA_LAUNCH_RESULT();
}

int onda_target_loss_fwd(const float* logits, int ldl, const int64_t* labels, int regularizer, float w_ce, float w_rce,
                         float w_reg, float w_js, float* result, float* ws, int64_t N, int K, onda_stream_t s) {
  const int nb = pixel_blocks(logits, result, N, K);
  ONDA_REQUIRE(nb && labels && ws && ldl >= K && is_regularizer(regularizer));
  hipLaunchKernelGGL(target_loss_fwd_kernel, dim3(nb), dim3(256), 0, ONDA_STREAM(s), logits, ldl, labels, regularizer, ws,
                     N, K);
  hipLaunchKernelGGL(target_loss_finalize_kernel, dim3(1), dim3(64), 0, ONDA_STREAM(s), ws, nb, regularizer, N, K, w_ce,
                     w_rce, w_reg, w_js, result);
  return ONDA_LAUNCH_RESULT();
}

int onda_target_loss_bwd(const float* logits, int ldl, const int64_t* labels, int regularizer, float w_ce, float w_rce,
                         float w_reg, float w_js, const float* result, const float* gscale, float* dlogits, int64_t N,
                         int K, onda_stream_t s) {
  const int nb = pixel_blocks(logits, dlogits, N, K);
  ONDA_REQUIRE(nb && labels && result && ldl >= K && ldl <= KMAX && is_regularizer(regularizer));
  hipLaunchKernelGGL(target_loss_bwd_kernel, dim3(nb), dim3(256), 0, ONDA_STREAM(s), logits, ldl, labels, regularizer,
                     result, gscale, w_ce, w_rce, w_reg, w_js, dlogits, N, K);
  return ONDA_LAUNCH_RESULT();
}

int onda_soft_loss_fwd(const float* logits, int ldl, const float* soft, int lds, int ce_trunc, int regularizer, float w_ce,
                       float w_rce, float w_reg, float* result, float* ws, int64_t N, int K, onda_stream_t s) {
  const int nb = pixel_blocks(logits, result, N, K);
  ONDA_REQUIRE(nb && soft && ws && ldl >= K && lds >= K && is_regularizer(regularizer));
  if (!float_aligned(logits) || !float_aligned(soft) || !float_aligned(result) || !float_aligned(ws)) return ONDA_EALIGN;
  hipLaunchKernelGGL(soft_loss_fwd_kernel, dim3(nb), dim3(256), 0, ONDA_STREAM(s), logits, ldl, soft, lds, ce_trunc,
                     regularizer, ws, N, K);
  hipLaunchKernelGGL(soft_loss_finalize_kernel, dim3(1), dim3(64), 0, ONDA_STREAM(s), ws, nb, regularizer, N, K, w_ce,
                     w_rce, w_reg, result);
  return ONDA_LAUNCH_RESULT();
}

int onda_soft_loss_bwd(const float* logits, int ldl, const float* soft, int lds, int ce_trunc, int regularizer, float w_ce,
                       float w_rce, float w_reg, const float* gscale, float* dlogits, int64_t N, int K, onda_stream_t s) {
  const int nb = pixel_blocks(logits, dlogits, N, K);
  ONDA_REQUIRE(nb && soft && ldl >= K && ldl <= KMAX && lds >= K && is_regularizer(regularizer));
  if (!float_aligned(logits) || !float_aligned(soft) || !float_aligned(dlogits) || (gscale && !float_aligned(gscale)))
    return ONDA_EALIGN;
  hipLaunchKernelGGL(soft_loss_bwd_kernel, dim3(nb), dim3(256), 0, ONDA_STREAM(s), logits, ldl, soft, lds, ce_trunc,
                     regularizer, gscale, w_ce, w_rce, w_reg, dlogits, N, K);
  return ONDA_LAUNCH_RESULT();
}

int onda_proto_sigma(const float* proto, const float* sqmean, const float* counter, float* sigma, int K, int C,
                     onda_stream_t s) {
  ONDA_REQUIRE(proto && sqmean && counter && sigma);
  hipLaunchKernelGGL(proto_sigma_kernel, dim3((C + 255) / 256), dim3(256), 0, ONDA_STREAM(s), proto, sqmean, counter,
                     sigma, K, C);
  return ONDA_LAUNCH_RESULT();
}

// workspace of onda_proto_assign in units of 3 floats: partial sums of the MFMA pass (PA_GRID workgroups) and of the direct
// pass over the close decisions (PA_LIST_GRID), the list itself (N ints) and its length
constexpr int PA_GRID = 256, PA_LIST_GRID = 256;
static int64_t pa_direct_blocks(int64_t N) {  // the direct form alone: a wave per pixel, 2048 workgroups at most
  const int64_t nb = (N + 3) / 4;
  return nb < 2048 ? nb : 2048;
}
int onda_proto_assign_blocks(int64_t N) {
  const int64_t nb = pa_direct_blocks(N);
  const int64_t mfma = PA_GRID + PA_LIST_GRID + (N + 4 + 2) / 3;
  return (int)(nb > mfma ? nb : mfma);
}

int onda_proto_assign(const float* feat, int ldf, const float* prior, int ldp, const float* proto, const float* sigma,
                      int mahalanobis, float tau, float thresh, int64_t* labels, float* soft, float* result, float* ws,
                      int64_t N, int C, int K, onda_stream_t s) {
  ONDA_REQUIRE(feat && proto && labels && result && ws && C == 256 && K >= 1 && K <= KMAX && N >= 1 && ldf % 4 == 0);
  ONDA_REQUIRE(!mahalanobis || sigma);
  if (!ONDA_ALIGNED16(feat) || !ONDA_ALIGNED16(proto) || (sigma && !ONDA_ALIGNED16(sigma))) return ONDA_EALIGN;
  if (N >= (1ll << 31)) {  // the direct form everywhere: the list of close decisions holds 32-bit pixel indices
    const int64_t nb = pa_direct_blocks(N);
    hipLaunchKernelGGL(proto_assign_kernel, dim3((unsigned)nb), dim3(256), 0, ONDA_STREAM(s), feat, ldf, prior, ldp, proto, sigma,
                       mahalanobis, tau, thresh, labels, soft, ws, N, K, nullptr, nullptr);
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(192), 0, ONDA_STREAM(s), ws, (int)nb, 3, (float)(1.0 / (double)N),
                       result);
    return ONDA_LAUNCH_RESULT();
  }
  int* list = reinterpret_cast<int*>(ws + 3 * (PA_GRID + PA_LIST_GRID));
  int* list_len = list + N;
  hipError_t e = hipMemsetAsync(list_len, 0, sizeof(int), ONDA_STREAM(s));
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(proto_assign_mfma_kernel, dim3(PA_GRID), dim3(64 * PA_WAVES), 0, ONDA_STREAM(s), feat, ldf, prior, ldp, proto, sigma,
                     mahalanobis, tau, thresh, 1.0e-3f, labels, soft, ws, list, list_len, N, K);
  hipLaunchKernelGGL(proto_assign_kernel, dim3(PA_LIST_GRID), dim3(256), 0, ONDA_STREAM(s), feat, ldf, prior, ldp, proto, sigma,
                     mahalanobis, tau, thresh, labels, soft, ws + 3 * PA_GRID, N, K, list, list_len);
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(192), 0, ONDA_STREAM(s), ws, PA_GRID + PA_LIST_GRID, 3,
                     (float)(1.0 / (double)N), result);
  return ONDA_LAUNCH_RESULT();
}

int onda_proto_distances(const float* feat, int ldf, const float* proto, const float* sigma, int mahalanobis, float* dist,
                         int64_t N, int C, int K, onda_stream_t s) {
  ONDA_REQUIRE(feat && proto && dist && N >= 1 && C == 256 && K >= 1 && K <= KMAX && ldf % 4 == 0 && (!mahalanobis || sigma));
  if (!ONDA_ALIGNED16(feat) || !ONDA_ALIGNED16(proto) || (sigma && !ONDA_ALIGNED16(sigma))) return ONDA_EALIGN;
  int64_t nb = (N + 3) / 4;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(proto_distances_kernel, dim3((unsigned)nb), dim3(256), 0, ONDA_STREAM(s), feat, ldf, proto, sigma, mahalanobis,
                     dist, N, K);
  return ONDA_LAUNCH_RESULT();
}

int64_t onda_proto_sums_ws(int64_t N, int C, int K) { return (int64_t)SUMS_BLOCKS * (2 * K * C + K); }

int onda_proto_class_sums(const float* feat, int ldf, const int32_t* cls, float* sums, float* counts, float* ws,
                          int64_t N, int C, int K, onda_stream_t s) {
  ONDA_REQUIRE(feat && cls && sums && counts && ws && N >= 1);
  const size_t lds = ((size_t)2 * K * C + K) * sizeof(float);
  ONDA_REQUIRE(lds <= 64 * 1024);
  const int64_t rpb = (N + SUMS_BLOCKS - 1) / SUMS_BLOCKS;
  hipLaunchKernelGGL(proto_class_sums_kernel, dim3(SUMS_BLOCKS), dim3(256), lds, ONDA_STREAM(s), feat, ldf, cls, ws, N,
                     C, K, rpb);
  const int tot = 2 * K * C + K;
  hipLaunchKernelGGL(proto_sums_finalize_kernel, dim3((tot + 255) / 256), dim3(256), 0, ONDA_STREAM(s), ws, SUMS_BLOCKS,
                     2 * K * C, K, sums, counts);
  return ONDA_LAUNCH_RESULT();
}

int onda_proto_ema(float* proto, float* sqmean, const float* sums, const float* counts, float lam, int K, int C,
                   onda_stream_t s) {
  ONDA_REQUIRE(proto && sqmean && sums && counts);
  hipLaunchKernelGGL(proto_ema_kernel, dim3((K * C + 255) / 256), dim3(256), 0, ONDA_STREAM(s), proto, sqmean, sums,
                     counts, lam, K, C);
  return ONDA_LAUNCH_RESULT();
}

int onda_proto_append(float* proto, float* sqmean, float* counter, const float* sums, const float* counts, int K, int C,
                      onda_stream_t s) {
  ONDA_REQUIRE(proto && sqmean && counter && sums && counts && K <= 64);
  hipLaunchKernelGGL(proto_append_kernel, dim3((K * C + 255) / 256), dim3(256), 0, ONDA_STREAM(s), proto, sqmean,
                     counter, sums, counts, K, C);
  hipLaunchKernelGGL(proto_append_counter_kernel, dim3(1), dim3(64), 0, ONDA_STREAM(s), counter, counts, K);
  return ONDA_LAUNCH_RESULT();
}

int onda_sgd_multi(const OndaSgdEntry* table, int n, float momentum, float weight_decay, float grad_scale, int64_t max_n,
                   onda_stream_t s) {
  ONDA_REQUIRE(table && n >= 1 && max_n >= 1 && max_n < (1ll << 31));  // max_n: total blocks (flat launch)
  hipLaunchKernelGGL(sgd_multi_kernel, dim3((unsigned)max_n), dim3(256), 0, ONDA_STREAM(s), table, n, momentum, weight_decay, grad_scale);
  return ONDA_LAUNCH_RESULT();
}

int onda_multi_tensor_block(void) { return MT_BLOCK; }

int onda_ema_multi(const OndaEmaEntry* table, int n, int64_t max_n, onda_stream_t s) {
  ONDA_REQUIRE(table && n >= 1 && max_n >= 1 && max_n < (1ll << 31));  // max_n: total blocks (flat launch)
  hipLaunchKernelGGL(ema_multi_kernel, dim3((unsigned)max_n), dim3(256), 0, ONDA_STREAM(s), table, n);
  return ONDA_LAUNCH_RESULT();
}

int onda_swap_multi(const OndaSwapEntry* table, int n, int64_t max_n, onda_stream_t s) {
  ONDA_REQUIRE(table && n >= 1 && max_n >= 1 && max_n < (1ll << 31));  // max_n: total blocks (flat launch)
  hipLaunchKernelGGL(swap_multi_kernel, dim3((unsigned)max_n), dim3(256), 0, ONDA_STREAM(s), table, n);
  return ONDA_LAUNCH_RESULT();
}

int64_t onda_sqdiff_multi_ws(int64_t total_blocks) { return total_blocks > 0 ? total_blocks : 0; }

int onda_sqdiff_multi(const OndaSqdiffEntry* table, int n, float half_lambda, int64_t max_n, float* ws, float* result,
                      onda_stream_t s) {
  ONDA_REQUIRE(table && ws && result && n >= 1 && max_n >= 1 && max_n < (1ll << 31));  // max_n: total blocks (flat launch)
  hipLaunchKernelGGL(sqdiff_multi_kernel, dim3((unsigned)max_n), dim3(256), 0, ONDA_STREAM(s), table, n, ws);
  hipLaunchKernelGGL(sqdiff_finalize_kernel, dim3(1), dim3(256), 0, ONDA_STREAM(s), ws, max_n, half_lambda, result);
  return ONDA_LAUNCH_RESULT();
}

int onda_sgd_anchor_multi(const OndaSgdAnchorEntry* table, int n, float momentum, float weight_decay, float grad_scale,
                          float half_lambda, int64_t max_n, onda_stream_t s) {
  ONDA_REQUIRE(table && n >= 1 && max_n >= 1 && max_n < (1ll << 31));  // max_n: total blocks (flat launch)
  hipLaunchKernelGGL(sgd_anchor_multi_kernel, dim3((unsigned)max_n), dim3(256), 0, ONDA_STREAM(s), table, n, momentum, weight_decay,
                     grad_scale, half_lambda);
  return ONDA_LAUNCH_RESULT();
}

// ONDA_SRC_HASH: sha256 (first 16 hex digits) over csrc/*.hip, csrc/*.h and include/*.h at build time (onda_amd/build.py):
// whoever loads the library can check that it was compiled from the sources beside it (onda_amd.build.source_hash()).
#ifndef ONDA_SRC_HASH
#define ONDA_SRC_HASH "unknown"
#endif
float onda_limb2_scale(void) { return ONDA_LIMB2_SCALE; }

const char* onda_version(void) { return "onda_hip 0.2 (gfx950) src=" ONDA_SRC_HASH; }

}  // extern "C"
