// Shared between the fp32 and the split-precision convolution kernels: argument block, the XCD band
// order of workgroups, the stream-K schedule (StreamK), the stream-K partial-tile store and the
// common epilogue (statistics, scale/shift, residual, ReLU,
// slice / scatter store) for a 4-wave workgroup of 32x32 or 16x16 MFMA accumulator tiles.
#pragma once
#include "common.h"

struct ConvK {
  const float* x;
  const void* w;
  float* y;
  const float* scale;
  const float* shift;
  const float* res;
  float* stats;
  OndaConv c;
  int M, tilesM, tilesN, taps, kcper;
  float* ws;     // stream-K partial tiles [grid][2][BM*BN]
  int tiles_dp;  // tiles done one-per-workgroup before the stream-K remainder (multiple of the grid)
  float* amax = nullptr;  // optional: running max|y| of the stored output (amax_update, common.h)
  int skip_dead_taps = 1;  // whole tiles skip filter taps that only see padding (conv_l2.hip)
  int late_issue = 1;      // conv_l2x_kernel: second half of the waves issues its DMAs behind its MFMAs
  // ---- limb-plane OUTPUT (eval-mode conv + folded BatchNorm whose result feeds other convs; conv_l2.hip) ----------------
  _Float16* yl = nullptr;           // out planes [2][M][ldy] f16 (dense rows); when set, `y` is not written
  long long yplane = 0;             // f16 elements between the two planes
  float* ybound = nullptr;          // amax buffer that DEFINES the planes' scale: receives the a-priori bound
  const float* kb = nullptr;        // {max_c |scale_c| * sum_k |w_ck|, max_c |shift_c|}
  const float* xtrue = nullptr;     // amax buffer with the TRUE max|x| of the input (its planes may be scaled by a bound)
  const _Float16* resl = nullptr;   // residual as limb planes [2][M][ldr]
  long long resplane = 0;
  const float* res_amax = nullptr;  // scale-defining amax of the residual planes
  const float* res_true = nullptr;  // true max|residual|
  unsigned long long* stamps = nullptr;  // diagnostics (ONDA_L2X_STAMP=1, tools/l2x_stamps.py): s_memtime per workgroup,
                                         // [32] each: start, then (end of K loop, end of epilogue) per work item
  int stats_rows = 2;     // 2: stats[tile][sum, sumsq][Cout]; 4: also the per-channel min and max of the raw tile (conv_l2.hip)
  long long x_total = 0;  // conv_l2.hip: bytes of the whole input operand.  A tile addresses it with 32-bit offsets RELATIVE to the
                          // first image its rows touch (a window of < 2 GiB), so the operand itself may be larger
};

struct WgradK {
  const float* x;
  const float* dy;
  float* slabs;
  OndaConv c;
  int M, lddy, splitk, mchunk, tilesN, tilesC, taps;
  long long x_total = 0, dy_total = 0;  // bytes of the operands: a workgroup addresses them relative to its pixel range's start
  unsigned long long* stamps = nullptr;  // diagnostics (onda_debug_stamps, tools/wgrad_stamps.py): [8] s_memtime per workgroup
  // [taps][pix_stride] input pixel ((b*Hi + hi)*Wi + wi, or -1 in the padding) of output pixel m under each tap: a table per
  // convolution geometry, built once by the library (csrc/conv_l2.hip, wgrad_pixel_table)
  const int* pix = nullptr;
  long long pix_stride = 0;
};

constexpr int BK = 32;

// Workgroups are dealt round-robin over the 8 XCDs (blocks b and b + 8 share one): the place of block `bid` in an order that
// hands each XCD a contiguous band of the launch's nblk work items, so that neighbours in that order share an L2.
template <class B>  // (B: the block index as the kernel holds it, int or unsigned -- the shift below follows it)
__device__ __forceinline__ int xcd_band(B bid, int nblk) {
  const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// ---- the hybrid stream-K schedule: what its writers (conv_fwd_kernel, conv_l2_kernel, conv_l2x_kernel), its readers
// (conv_piece_sum_kernel, conv_fixup_kernel, conv_l2_fixup_kernel) and the host's workspace bounds agree on -----------------
// tiles_dp tiles (whole rounds of the grid) run one per workgroup and round.  The remaining tiles x KT K-steps are U units,
// cut into G equal contiguous ranges: workgroup w (its place in the XCD band order) has [begin(w), begin(w + 1)).  A range
// end inside a tile leaves a partial tile in the workspace [G][2][BM * BN]: a range meets at most two tiles in part, its
// first piece goes to slot 0 of its workgroup, a later one to slot 1.  A writer and a reader that disagree about any line of
// this give a wrong tile sum, not a crash: keep every one of them here.
struct SkItem {
  bool dp;  // a whole tile of the one-per-workgroup rounds
  int tile, k_begin, k_end;
};
struct SkTile {
  long long t0, t1;  // the units of one remainder tile
};
// A workgroup's cursor is (dp_tile, u): its next whole tile, the next unit of its remainder range [begin(w), u_end = begin(w + 1)).
struct StreamK {
  // Every member is forced inline, and written so that the kernels' code is what it was with these lines standing in them: a
  // helper is simplified on its own before it is inlined, so KT is widened ONCE, here, as a kernel does at its first use.
  int KT, tiles_dp, G;
  long long U, KTw;
  __host__ __device__ __forceinline__ StreamK(int tiles_all, int tiles_dp_, int KT_, int G_)
      : KT(KT_), tiles_dp(tiles_dp_), G(G_), U((long long)(tiles_all - tiles_dp_) * KT_), KTw(KT_) {}
  __device__ __forceinline__ long long begin(int w) const { return w * U / G; }
  __device__ __forceinline__ bool valid(const int& dp_tile, const long long& u, const long long& u_end) const { return dp_tile < tiles_dp || u < u_end; }
  // (selects, as conv_fwd_kernel and conv_l2_kernel had them; conv_l2x_kernel branches once and keeps its own text: experiments.md)
  __device__ __forceinline__ SkItem item(int dp_tile, long long u, long long u_end) const {
    const bool dp = dp_tile < tiles_dp;
    const int tile = dp ? dp_tile : tiles_dp + (int)(u / KTw);
    const int k_begin = dp ? 0 : (int)(u - (long long)(tile - tiles_dp) * KTw);
    const int k_end = dp ? KT : (int)min(KTw, k_begin + (u_end - u));
    return {dp, tile, k_begin, k_end};
  }
  __device__ __forceinline__ void advance(int& dp_tile, long long& u, const SkItem& it) const {
    if (it.dp) dp_tile += G; else u += it.k_end - it.k_begin;
  }
  // workspace slot of a piece of workgroup w: 0 for the piece that begins where its range does, 1 for a later one; the slots of G
  // workgroups end where slot(G, ..) would begin
  template <class I>
  __host__ __device__ __forceinline__ static I slot(I w, long long piece_begin, long long range_begin) {
    return w * 2 + (piece_begin == range_begin ? 0 : 1);
  }
  // where a writer stores that piece (TILE = BM * BN floats)
  template <int TILE>
  __device__ __forceinline__ static float* piece_of(float* ws, int w, long long piece_begin, long long range_begin) {
    return ws + slot((size_t)w, piece_begin, range_begin) * TILE;
  }
  __host__ __device__ __forceinline__ static size_t ws_floats(int G, int tile_floats) { return slot((size_t)G, 0, 0) * tile_floats; }
  // readers -- remainder tile lt (0 = tile tiles_dp) and the first and the last workgroup whose range meets its units (equal:
  // one workgroup computed the tile whole, its own epilogue ran) ...
  template <class I>  // (int or the unsigned block index: the widening follows it)
  __device__ __forceinline__ SkTile tile_units(I lt) const {
    const long long t0 = (long long)lt * KT, t1 = t0 + KT;
    return {t0, t1};
  }
  __device__ __forceinline__ int first_wg(const SkTile& tu) const { return (int)(((tu.t0 + 1) * G + U - 1) / U - 1); }
  __device__ __forceinline__ int last_wg(const SkTile& tu) const { return (int)((tu.t1 * G + U - 1) / U - 1); }
  // ... and the slot workgroup w left its piece of that tile in, -1 if its range is empty there
  __device__ __forceinline__ int piece(int w, const SkTile& tu) const {
    const long long b0 = begin(w), b1 = begin(w + 1);
    const long long g0 = max(b0, tu.t0), g1 = min(b1, tu.t1);
    return g1 > g0 ? slot(w, g0, b0) : -1;
  }
};

// Accumulator fragment of one MF x MF MFMA tile: which (row, column) of the tile register e of a
// lane holds (32x32x* and 16x16x* MFMA result layouts).
template <int MF>
struct AccTile;
template <>
struct AccTile<32> {
  using T = f32x16;
  static constexpr int E = 16;
  static __device__ __forceinline__ int row(int e, int lane) { return (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5); }
  static __device__ __forceinline__ int col(int lane) { return lane & 31; }
};
template <>
struct AccTile<16> {
  using T = f32x4;
  static constexpr int E = 4;
  static __device__ __forceinline__ int row(int e, int lane) { return 4 * (lane >> 4) + e; }
  static __device__ __forceinline__ int col(int lane) { return lane & 15; }
};

// raw accumulators of a partial (stream-K) tile -> slot[BM][BN]
template <int BN, int TM, int TN, int MF = 32>
__device__ __forceinline__ void conv_store_partial(float* slot, const typename AccTile<MF>::T (&acc)[TM][TN], int wm,
                                                   int wn, int lane) {
  using L = AccTile<MF>;
#pragma unroll
  for (int jn = 0; jn < TN; ++jn)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int e = 0; e < L::E; ++e) {
        const int row = (wm * TM + i) * MF + L::row(e, lane);
        slot[row * BN + (wn * TN + jn) * MF + L::col(lane)] = acc[i][jn][e];
      }
}

// ---- what every convolution does to a finished tile, piece by piece (the tile epilogues and the stream-K fix-ups of conv.hip
// and conv_l2.hip) ----
// row m of the GEMM is row m of y: every convolution but the strided data gradient
__device__ __forceinline__ bool dense_out(const OndaConv& c) { return c.out_os == 1 && c.Hf == c.Ho && c.Wf == c.Wo; }
// ... whose GEMM row m (an output pixel of the strided conv) goes to this row of y (the pixel it sampled)
__device__ __forceinline__ size_t out_row(const OndaConv& c, int m) {
  const int wo = m % c.Wo, tq = m / c.Wo;
  const int ho = tq % c.Ho, b = tq / c.Ho;
  return ((size_t)b * c.Hf + (size_t)ho * c.out_os) * c.Wf + (size_t)wo * c.out_os;
}
// the per-channel minimum and maximum of no rows at all (statistic rows 2 and 3; rows 0 and 1, the sums, start at 0)
constexpr float STAT_MIN_ID = 3.0e38f, STAT_MAX_ID = -3.0e38f;
// v * sc + sh.  FUSED: rounded once (the expression is contracted to an fma), what the tile epilogues and conv_fixup_kernel
// compute; not FUSED: the product is rounded before the shift is added -- conv_l2_fixup_kernel, which applied its scale and its
// shift under separate tests, keeps its bits that way
template <bool FUSED>
__device__ __forceinline__ f32x4 affine4(f32x4 v, f32x4 sc, f32x4 sh) {
  if constexpr (FUSED) {
    return v * sc + sh;
  } else {
#pragma clang fp contract(off)
    const f32x4 p = v * sc;
    return p + sh;
  }
}
// fp32 output of four columns: v in the operands' own units, sc / sh the columns' scale and shift (1 and 0: none), res: the
// residual's four values (null: none)
template <bool FUSED = true>
__device__ __forceinline__ f32x4 conv_out4(f32x4 v, f32x4 sc, f32x4 sh, const f32x4* res, bool relu) {
  v = affine4<FUSED>(v, sc, sh);
  if (res != nullptr) v += *res;
  if (relu) v = relu4(v);
  return v;
}

// `red`: >= WAVES_M*BN*2 + 2*WAVES_M floats of LDS that no wave is still reading.  (A lane of the 32 x 32 accumulator layout
// holds ONE column per MFMA tile, so the output expression stands here in scalar form, not as conv_out4.)
template <int BM, int BN, int TM, int TN, int WAVES_M, int MF = 32>
__device__ __forceinline__ void conv_epilogue(const ConvK& a, const typename AccTile<MF>::T (&acc)[TM][TN],
                                              float* red, int tile_m, int m0, int n0, int wm, int wn, int lane) {
  using L = AccTile<MF>;
  const OndaConv& c = a.c;
  const int t = threadIdx.x;
  if (a.stats != nullptr) {
#pragma unroll
    for (int jn = 0; jn < TN; ++jn) {
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int e = 0; e < L::E; ++e) {
          const float v = acc[i][jn][e];
          s1 += v;
          s2 += v * v;
        }
#pragma unroll
      for (int sh = MF; sh < 64; sh <<= 1) {  // lanes holding other rows of the same column
        s1 += __shfl_xor(s1, sh, 64);
        s2 += __shfl_xor(s2, sh, 64);
      }
      if (lane < MF) {
        const int col = (wn * TN + jn) * MF + lane;
        red[(wm * BN + col) * 2 + 0] = s1;
        red[(wm * BN + col) * 2 + 1] = s2;
      }
    }
    __syncthreads();
    if (t < BN && n0 + t < c.Cout) {
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int w_ = 0; w_ < WAVES_M; ++w_) {
        s1 += red[(w_ * BN + t) * 2 + 0];
        s2 += red[(w_ * BN + t) * 2 + 1];
      }
      a.stats[((size_t)tile_m * 2 + 0) * c.Cout + n0 + t] = s1;
      a.stats[((size_t)tile_m * 2 + 1) * c.Cout + n0 + t] = s2;
    }
  }

  const bool plain = dense_out(c);
  float mx = 0.f;
#pragma unroll
  for (int jn = 0; jn < TN; ++jn) {
    const int n = n0 + (wn * TN + jn) * MF + L::col(lane);
    if (n >= c.Cout) continue;
    const float sc = a.scale ? a.scale[n] : 1.f;
    const float sh = a.shift ? a.shift[n] : 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int e = 0; e < L::E; ++e) {
        const int m = m0 + (wm * TM + i) * MF + L::row(e, lane);
        if (m >= a.M) continue;
        float v = acc[i][jn][e] * sc + sh;
        if (a.res) v += a.res[(size_t)m * c.ldr + n];
        if (c.relu) v = fmaxf(v, 0.f);
        a.y[(plain ? (size_t)m : out_row(c, m)) * c.ldy + n] = v;
        mx = fmaxf(mx, fabsf(v));
      }
    }
  }
  // one atomic per tile: max over the workgroup's waves through LDS (past the statistics' scratch)
  if (a.amax != nullptr) tile_amax_publish<2 * WAVES_M>(a.amax, mx, red + WAVES_M * BN * 2);
}

// conv.hip: sums stream-K partial tiles and runs the epilogue for split tiles
int conv_launch_fixup(const ConvK& k, int G, bool wide, hipStream_t st);
int conv_launch_fixup_tile(const ConvK& k, int G, int BM, int BN, hipStream_t st);  // any of the tile shapes of conv_l2.hip
int conv_resident_workgroups();
int conv_sched_override();  // debugging aid: environment variable ONDA_CONV_SCHED (0 / unset = automatic)
