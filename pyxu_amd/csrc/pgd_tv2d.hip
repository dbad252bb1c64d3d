// Fused PGD step for 2-D TV-regularised deblurring, normal-operator form: one launch per iteration.
//
//   yk     = x + a (x - x_prev)                                            (pgd.py:179-181)
//   grad   = (G yk - b) + Grad^T q,   G = H^T H,  b = H^T y  (b precomputed once per solve)
//   q      = lam * v / max(|v|, mu)  ==  lam (v - prox_{mu L21}(v)) / mu,  v = Grad yk
//   x_new  = prox_{tau g}( grad * (-tau) + yk )                            (pgd.py:185-191)
//
// Reference dataflow: PGD.m_step (opt/solver/pgd.py:173-191) through AddRule.grad,
// ChainRule.grad, ScaleRule.grad, ArgShiftRule.grad (abc/arithmetic.py), Stencil.apply/adjoint
// (operator/linop/stencil/stencil.py:441-461), Gradient (operator/linop/diff.py:1113-1265), the
// moreau_envelope gradient (abc/operator.py:1053-1058), L21Norm.prox (operator/func/norm.py:352-364),
// PositiveOrthant.prox / L1Norm.prox.
//
// Why the normal form.  The reference evaluates H^T (H yk - y): two zero-boundary separable
// correlations in sequence, i.e. four 1-D passes of 2R+1 taps whose halos compound (a fused tile
// must recompute a 2R halo of H yk).  H is separable, H = H0 (x) H1, so G = H^T H = G0 (x) G1 with
// G_a = H_a^T H_a a banded n_a x n_a matrix: in rows R <= i < n_a - R it is the Toeplitz filter
// g[d] = sum_t k[t] k[t+d], |d| <= 2R (autocorrelation of the taps); in the R boundary rows on each
// side the zero-boundary truncation of the inner H changes the coefficients, and those rows are
// evaluated exactly as sum_t k[t] [0 <= i-t < n] sum_s k[s] yk[i-t+s].  G is therefore EXACTLY the
// reference's operator (fp64 trajectories agree to 1e-16); only fp32 rounding order differs
// (measured 1.5e-7 relative after 100 PGD iterations vs fp64, the same as the reference's own fp32
// path).  Two passes of 4R+1 taps replace four passes of 2R+1, one LDS round trip and two barriers
// disappear, and b = H^T y replaces y in the compulsory traffic (x, x_prev, b in; x_new out).
//
// One 256-thread workgroup owns a TY x TX output tile:
//   phase 0  A  = yk on rows [ty0-2R, ty0+TY+2R) x cols [tx0-CA, tx0+TX+CA), zero outside the image
//   pass A   PT = (G0 yk) on the tile rows, all A columns, stored TRANSPOSED ([col][row])   (V x V
//                 register blocks: ds_read_b128 rows, packed FMAs, ds_write_b128 columns)
//   pass B   out = G1 along each row (sweeps PT rows = image columns) - b + Grad^T q, prox, store;
//                 q is evaluated on the fly from yk in A.  fp32: one 2-row x 4-column block per thread, swept over
//                 ds_read_b64 rows of PT and finished in that thread's registers as two 16-B row vectors
//                 (pass_b_blocks); fp64: 2 x 1 items staged through LDS into a row-major epilogue (pass_b_staged).
// LDS pitches / lane orders are conflict-free for R = 6 fp32 under the MI355X_MICROARCH.md §LDS
// bank model (scripts/ldsbank.py, scripts/ldsbank_blocks.py).  The blockIdx -> tile map is XCD-aware: each of the
// 8 XCDs owns a contiguous band of tiles so that halo re-reads of x / x_prev hit its own L2.
// Tile classes (tile2d.hpp tile_class; fp32): a tile whose window lies inside the image is `interior` (no bounds tests);
// one that ends exactly on one border of an aligned image is `col` or `row` and runs the interior code on its interior
// axis, skipping the halo beyond the border and correcting the R boundary rows / columns of G from ghost terms with
// compile-time tap indices; one that ends on a row border and a column border at once is `corner` and runs the row
// class's code with the col class's column part (R <= 6); every other tile is `generic` (bounds tests, runtime-indexed
// corrections).
#include "tile2d.hpp"
#include <type_traits>

// Wave priority (s_setprio) of the window-load phase: its loads issue ahead of the passes of the other
// workgroups resident on the SIMD, so that the next round's windows are in flight sooner.  Interleaved A/B
// (profiles/r05zb_pgd_prio_ab.txt): 2048^2 24.4 -> 23.4 us on one box, no change on another (r05zc); C5 and
// 4096^2 unchanged within noise; priority 2 or 3, or also raising the epilogue, gave the same.  Scheduling
// only: the same bits.
#ifndef PXA_PGD_PRIO
#define PXA_PGD_PRIO 1
#endif
#ifndef PXA_PGD_PRIO_EPI
#define PXA_PGD_PRIO_EPI 0  // (A/B builds: the epilogue's H^T y loads too)
#endif
#ifndef PXA_PGD_PRIO_FIN
#define PXA_PGD_PRIO_FIN 0  // (A/B builds: the finishing row-major epilogue)
#endif

// Measurement probes (s_memtime phase trace, skip probes: PXA_TUNE_PGD_DIAG) exist only in the probe build
// (`make -C pyxu_amd/csrc probe`, scripts/ that time kernel phases); the production library compiles them out, so
// its kernel carries no probe branch.
#ifndef PXA_PROBES
#define PXA_PROBES 0
#endif

namespace pxa {
namespace {

using namespace tile2d;
constexpr bool kProbes = PXA_PROBES != 0;


template <typename T>
struct PgdParams {
  int64_t stack, y_images;
  int n0, n1;
  int tiles0, tiles1;
  unsigned ntiles;
  T k0[2 * kMaxR + 1], k1[2 * kMaxR + 1];  // H taps, dense window t = -R..R (index t + R)
  T g0[kMaxG], g1[kMaxG];                  // interior G taps, d = -2R..2R (index d + 2R)
  T g0a, g0b, g1a, g1b;                    // forward-difference taps per axis (-1/h, 1/h)
  T lam, mu, inv_mu, a, tau, pw;
  int prox;  // 0 none, 1 positive orthant, 2 l1 (uniform branch)
  bool tv;   // lam != 0 (uniform branch)
  bool vec_ok;
  int diag;       // PXA_TUNE_PGD_DIAG (bit 5: s_memtime phase trace of a few workgroups)
  const T* xref;  // RelError partials relative to this iterate (nullptr: relative to x)
  // last-workgroup fold of the RelError partials (pxa_pgd_tv2d_plan_step with rel_values): the workgroup
  // that finishes last folds them as pxa_tile_partials_fold does (same bits) into fold_vals (host-mapped,
  // (2, fold_rows)) and sets fold_flags[q] = fold_seq; `counter` (device, 0 between launches) counts the
  // finished workgroups.  fold_vals == nullptr: no fold.
  double* fold_vals;
  unsigned* fold_flags;
  unsigned* counter;
  unsigned fold_seq;
  int64_t fold_rows, fold_per_row;
  // window partials (pxa_pgd_tv2d_plan_step_wfold): the per-(tile, wave) partials are (sum (x - x_prev)^2, sum x_prev^2)
  // over the tile, from the window loads -- the RelError statistics of the PREVIOUS step's check -- instead of the
  // epilogue's (x_new - x_ref) statistics: no extra load of x
  int win_part;
  // publication of the PREVIOUS launch's partials (pxa_pgd_tv2d_plan_step_wpub): one extra workgroup (block ntiles)
  // folds pub_src as pxa_tile_partials_fold does (same bits) into pub_vals and sets pub_flags[q] = pub_seq, beside
  // the tile workgroups -- no fold launch, no cross-workgroup hand-off (pub_src is complete at launch)
  const double* pub_src;
  double* pub_vals;
  unsigned* pub_flags;
  unsigned pub_seq;
};

// Round 3 also measured a variant that carried yk as solver state (the epilogue writing the next
// iteration's yk, the window reading one array instead of two): equal at 2048^2 (25.4 vs 24.9 us) and
// slower at 4096^2 (79.6 vs 66.2 us), where the fifth compulsory stream costs more than the halved window
// saves; it was removed.

// Timing trace (PXA_TUNE_PGD_DIAG bit 5, read by pxa_pgd_tile_trace): s_memtime stamps of waves 0-3 of
// workgroups 0, 9, grid/2 + 8, grid-1 and 8, 8 points of their tile.  Staged in LDS beyond the kernel's own
// carve, dumped at exit.
constexpr int kTraceWords = 5 * 4 * 8;
__device__ unsigned long long g_tile_trace[kTraceWords];
// Launch timeline (the same bit, read by pxa_pgd_tile_timeline; probe build only): start stamp, end stamp and
// tile | class << 32 | XCC_ID << 36 | HW_ID[15:0] << 40 of every workgroup, in blockIdx order.  The counter's
// base differs between XCDs and, as measured, between CUs: scripts/tile_trace.py takes stamps relative to the first
// start on the same CU.
#if PXA_PROBES
constexpr unsigned kTimelineWgs = 1u << 14;
__device__ unsigned long long g_tile_timeline[3 * kTimelineWgs];
#endif

// Every multiply-add outside the Toeplitz sweeps is written as an explicit fma (the TV stencil's
// two-product sums as fma(a, b, c * d)): under fp-contract=fast the compiler fuses or not, and picks
// which product to fuse, per code position, so the tile and march kernels (different blocking, code
// layout per radius) would otherwise round differently at a few pixels.
// q-weight: lam / max(|v|, mu)  (so that q = w v = lam (v - prox_{mu L21}(v)) / mu).
template <typename T>
__device__ inline T tv_weight(T n2, T lam, T mu, T inv_mu) {
  const T n = sqrt(n2);
  return lam / (n > mu ? n : mu);
}
template <>
__device__ inline float tv_weight<float>(float n2, float lam, float mu, float inv_mu) {
  const float r = __builtin_amdgcn_rsqf(n2);  // 1/|v| (inf at 0), 1 ulp
  return lam * __builtin_fminf(r, inv_mu);      // one v_min_f32 (r is never NaN: n2 >= 0)
}

// ---- phase 0 of the tile kernel: yk = (x - x_prev) * a + x on the A window, zero outside the image.
// All K0 vector pairs of a thread are loaded before the first LDS store, so their latencies overlap.
// `lt`: the thread's index among the kThreads threads that share the window.
//
// Window order.  Thread (wave wv, lane ln) handles item k = 0 .. K0 - 1; window vector (row r, vector column g) of
// an item is a LANE part (rl, gl), a function of ln alone and the same for every item of a region, plus a
// WAVE-UNIFORM part (ru, gu), a function of k and wv: no per-item division, and every region choice is a scalar
// branch or resolved at compile time.
//   items k < KI     the tile's own TY x TX pixels, row-major: item k is item 0 shifted down by kThreads / TV rows.
//                    The RelError window partials (the tile's pixels only) are exactly these items of every thread.
//   halo wave-slots  hs = (k - KI) * NW + wv, in two regions with wave-aligned boundaries:
//     side  (hs < NSS)   the CV vectors left and right of ALL AR window rows.  Row-block form: a slot takes 64 / (2 CV)
//                        whole rows (lane -> row ln / (2 CV), side vector ln % (2 CV), once per thread), successive
//                        slots are that many rows apart.  Where the row blocks would need more slots than K0 leaves
//                        (fp64, R = 7) the column form: slot = side vector column, lane = window row.
//     vert  (< NSS+NVS)  the TV tile-column vectors of the 2R rows above and the 2R rows below the tile: 64 / TV rows
//                        per slot, alternately from the top and the bottom block (lane -> ln / TV: even top, odd
//                        bottom), successive slots 64 / TV / 2 rows further down in both blocks.
// Lanes of a side slot beyond its rows, and the slots beyond NSS + NVS, are idle.  Any bijection of window vectors to
// (thread, item) gives the same A (each vector's yk is computed alone): the order only moves work between threads.
template <typename T, int R>
struct Window {
  using L = Layout<T, R>;
  static constexpr int K0 = cdiv(L::N0, kThreads);
  static constexpr int NW = kThreads / 64;
  static constexpr int TV = TX / L::V, CV = L::CA / L::V;
  static constexpr int NI = TY * TV;
  static constexpr int KI = NI / kThreads;
  static constexpr int RPI = kThreads / TV;  // tile rows per own item
  static constexpr int RPW = 64 / TV;        // rows per wave (own items) / per vert slot
  static constexpr int SL = 2 * CV;          // side vectors per window row
  static constexpr int SRB = 64 / SL;        // side, row-block form: rows per slot
  static constexpr int NVS = 4 * R / RPW;    // vert slots
  static constexpr int HS = (K0 - KI) * NW;  // halo wave-slots that K0 items leave
  static constexpr bool SIDE_ROWS = cdiv(L::AR, SRB) + NVS <= HS;
  static constexpr int NSS = SIDE_ROWS ? cdiv(L::AR, SRB) : SL;  // side slots
  static_assert(NI % kThreads == 0, "every thread loads KI of the tile's own vectors");
  static_assert(64 % TV == 0 && RPW % 2 == 0 && (4 * R) % RPW == 0, "vert slots: whole rows, top / bottom pairs");
  static_assert(SL <= 64 && L::AR <= 64, "side slots: a row block or a column per wave");
  static_assert(NSS + NVS <= HS, "K0 must not grow");

  // item k of lane ln in wave wv -> window row rl + ru, vector column gl + gu; false: an idle slot
  __host__ __device__ static constexpr bool item(int k, int wv, int ln, int& rl, int& gl, int& ru, int& gu) {
    rl = gl = ru = gu = 0;
    if (k < KI) {
      rl = 2 * R + ln / TV;
      gl = CV + ln % TV;
      ru = k * RPI + wv * RPW;
      return true;
    }
    const int hs = (k - KI) * NW + wv;
    if (hs < NSS) {
      if (SIDE_ROWS) {
        const int q = ln % SL;
        rl = ln / SL;
        gl = q < CV ? q : q + TV;
        ru = hs * SRB;
        return ln < SRB * SL && rl + ru < L::AR;
      }
      rl = ln;
      gu = hs < CV ? hs : hs + TV;
      return ln < L::AR;
    }
    if (hs < NSS + NVS) {
      const int j = ln / TV;
      rl = (j >> 1) + (j & 1) * (2 * R + TY);
      gl = CV + ln % TV;
      ru = (hs - NSS) * (RPW / 2);
      return true;
    }
    return false;
  }
  // every one of the N0 window vectors is item (k, wv, ln) of exactly one thread
  static constexpr bool covers_once() {
    int cnt[L::N0] = {};
    for (int k = 0; k < K0; ++k)
      for (int wv = 0; wv < NW; ++wv)
        for (int ln = 0; ln < 64; ++ln) {
          int rl = 0, gl = 0, ru = 0, gu = 0;
          if (!item(k, wv, ln, rl, gl, ru, gu)) continue;
          const int r = rl + ru, g = gl + gu;
          if (r < 0 || r >= L::AR || g < 0 || g >= L::NGA) return false;
          ++cnt[r * L::NGA + g];
        }
    for (int i = 0; i < L::N0; ++i)
      if (cnt[i] != 1) return false;
    return true;
  }
  static_assert(covers_once(), "the window order is a bijection onto the AR x NGA window vectors");

  T xv[K0][L::V], pv[K0][L::V];
};

// (wave, lane) of thread lt; the wave index as a scalar, so that what Window::item derives from it is wave-uniform.
// This is all the range knowledge the window decode needs (lane < 64 by the mask, wave < 4 by the assume).  A range
// assumption on the thread index itself, visible to the passes and the epilogue too, removed nothing more from the fp32
// kernel and made every fp64 instantiation spill (R = 2 .. 8: 108 .. 1284 B of scratch per thread), so there is none.
__device__ inline void wave_lane(int lt, int& wv, int& ln) {
  wv = __builtin_amdgcn_readfirstlane(lt >> 6);
  __builtin_assume(wv >= 0 && wv < kThreads / 64);
  ln = lt & 63;
}

// Interior tiles: the address of a vector as a wave-uniform 64-bit base -- element (row0 + ru, col0) of the image,
// formed in scalar registers -- plus a zero-extended 32-bit byte offset per lane (the saddr + voffset form of the
// global loads / stores: no 64-bit address arithmetic in the vector unit).  The kernels' `interior` predicate bounds
// n1 (tile2d.hpp kMaxInteriorN1) so that the lane offsets, at most (AR n1 + AC) sizeof(T), fit in 32 bits.
template <typename T>
__device__ inline T* lane_ptr(T* img, int row0, int col0, int n1, int ru, unsigned voff) {
  T* base = img + ((int64_t)row0 * n1 + col0) + ru * n1;  // (ru n1 < 2^28: |ru| <= 64, n1 <= kMaxInteriorN1)
  using C = std::conditional_t<std::is_const_v<T>, const char, char>;
  return reinterpret_cast<T*>(reinterpret_cast<C*>(base) + (size_t)voff);
}

// The side of a tile that ends on a border (tile2d.hpp tile_class): 0 when it holds the image's first rows / columns,
// 1 its last.
__device__ inline int row_side(int ty0) { return __builtin_amdgcn_readfirstlane(ty0 == 0 ? 0 : 1); }
__device__ inline int col_side(int tx0) { return __builtin_amdgcn_readfirstlane(tx0 == 0 ? 0 : 1); }

// Corner tiles end on a row border and a column border at once.  They run the row class's body, which takes the column
// part (the skipped side vectors, ghost_cols_side, the col class's sweep corrections, the TV "first column") under the
// wave-uniform flag `corner`: the four workgroups of a launch that are corners then execute code that the row tiles of
// their XCD -- dispatched beside them, the top and bottom tile rows -- keep in the instruction cache, and only the
// column part is theirs alone.  A fifth copy of the tile body, measured beside this form, gave the same corner life
// (20.1 k against 20.3 k ticks median at 2048^2, R = 6; generic 30.3 k) from more code.
// Whether a tile run by class C's body has a border column (`corner`: wave-uniform).
template <int C>
__device__ inline bool has_col(bool corner) {
  if constexpr (C == kTileCol) return true;
  else if constexpr (C == kTileRow) return corner;
  else return false;
}
// The reaches whose kernel has the corner part.  R = 7 and 8 keep their corners on the generic path, as fp64 does:
// these two instantiations already spill (128 VGPRs at four workgroups per CU), and with the corner part they spill
// more (R = 7: 204 -> 296 B of scratch per thread, R = 8: 620 -> 624 B), which every tile of the launch would pay for.
template <int R>
constexpr bool kCornerPart = R <= 6;

// `C`: the tile's class.  Col and row tiles load as interior ones do, except that the halo vectors beyond their one
// border -- the CV side vectors of every window row / the 2R rows of one vertical block, side vectors included --
// are not loaded and stay zero; a corner tile skips both sets.  The own items (and so the window partials) are never
// among them.
template <typename T, int R, int C>
__device__ inline void win_issue(const PgdParams<T>& p, int ty0, int tx0, const T* __restrict__ xs,
                                 const T* __restrict__ xps, Window<T, R>& w, int lt, bool corner) {
  using L = Layout<T, R>;
  using W = Window<T, R>;
  constexpr int V = L::V;
  constexpr int CA = L::CA;
  constexpr bool EDGE = C == kTileGeneric;
  const int n0 = p.n0, n1 = p.n1;
  int wv, ln;
  wave_lane(lt, wv, ln);
  const int rside = row_side(ty0), cside = col_side(tx0);
  const bool colp = has_col<C>(corner);
#pragma unroll
  for (int k = 0; k < W::K0; ++k) {
    int rl, gl, ru, gu;
    if (W::item(k, wv, ln, rl, gl, ru, gu)) {
      if (!EDGE) {
        if ((C == kTileCol || C == kTileRow) && k >= W::KI) {
          const int r = rl + ru, g = gl + gu;
          bool outside = false;
          if constexpr (C == kTileRow) outside = rside == 0 ? r < 2 * R : r >= 2 * R + TY;
          if (colp) outside = outside || (cside == 0 ? g < W::CV : g >= W::CV + W::TV);
          if (outside) {
#pragma unroll
            for (int v = 0; v < V; ++v) w.xv[k][v] = w.pv[k][v] = T(0);
            continue;
          }
        }
        const unsigned voff = (unsigned)(rl * n1 + V * gl) * (unsigned)sizeof(T);
        ld_vec<T, V>(lane_ptr<const T>(xs, ty0 - 2 * R, tx0 - CA + V * gu, n1, ru, voff), w.xv[k]);
        if (kProbes && (p.diag & 256)) {  // timing probe only (WRONG results): one window array instead of two
#pragma unroll
          for (int v = 0; v < V; ++v) w.pv[k][v] = w.xv[k][v];
        } else {
          ld_vec<T, V>(lane_ptr<const T>(xps, ty0 - 2 * R, tx0 - CA + V * gu, n1, ru, voff), w.pv[k]);
        }
        continue;
      }
      const int gr = ty0 - 2 * R + rl + ru, gc = tx0 - CA + V * (gl + gu);
      if (gr >= 0 && gr < n0 && p.vec_ok && gc >= 0 && gc + V <= n1) {
        ld_vec<T, V>(xs + (int64_t)gr * n1 + gc, w.xv[k]);
        ld_vec<T, V>(xps + (int64_t)gr * n1 + gc, w.pv[k]);
      } else {
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const bool in = gr >= 0 && gr < n0 && gc + v >= 0 && gc + v < n1;
          w.xv[k][v] = in ? xs[(int64_t)gr * n1 + gc + v] : T(0);
          w.pv[k][v] = in ? xps[(int64_t)gr * n1 + gc + v] : T(0);
        }
      }
    }
  }
}

template <typename T, int R>
__device__ inline void win_store(const PgdParams<T>& p, T* A, const Window<T, R>& w, int lt) {
  using L = Layout<T, R>;
  using W = Window<T, R>;
  constexpr int V = L::V;
  int wv, ln;
  wave_lane(lt, wv, ln);
#pragma unroll
  for (int k = 0; k < W::K0; ++k) {
    int rl, gl, ru, gu;
    if (W::item(k, wv, ln, rl, gl, ru, gu)) {
      T out[V];
#pragma unroll
      for (int v = 0; v < V; ++v) out[v] = fma(w.xv[k][v] - w.pv[k][v], p.a, w.xv[k][v]);  // one rounding site
      st_vec<T, V>(A + (rl * L::AP + V * gl) + (ru * L::AP + V * gu), out);
    }
  }
}

// Pitch of PT: fp32 runs pass B on 2 x 4 row-major blocks (tile2d.hpp BlockB), fp64 on Layout's 2 x 1 items.
template <typename T, int R>
__host__ __device__ constexpr int pt_pitch() {
  if constexpr (sizeof(T) == 4) return BlockB<T, R>::PTP;
  else return Layout<T, R>::PTP;
}

// ---- pass A: PT[col][row] = (G0 yk)[row][col] for the TY tile rows and all A columns
// Bytes of the ghost-term region of the PGD tile kernel: the boundary-column terms of a col or generic tile (tile2d.hpp
// kGhBytes) or the boundary-row terms of a row tile (fp32: R rows of AC columns).  A corner tile has both, one after the
// other: its row terms are written and read inside pass A, wave by wave, and are dead at the barrier behind it; its
// column terms are written behind that barrier.  So the region is the larger of the two, not their sum, for every R.
template <typename T, int R>
constexpr size_t kPgdGhBytes =
    sizeof(T) == 4 && (size_t)R * Layout<T, R>::AC * sizeof(T) > kGhBytes<T, R> ? (size_t)R * Layout<T, R>::AC * sizeof(T)
                                                                                  : kGhBytes<T, R>;

// Row tiles: the R ghost rows of H0 yk beyond the tile's border (ghost_fix()'s gh, the same fma order: s ascending),
// computed once per column group instead of once per item that needs them.  The NA items of a column group are NA
// consecutive lanes of one wave: lane a < R evaluates ghost row m = a over the group's V columns and parks it in
// GH[group][m][V]; the items within R rows of the border read all R back (pass_a).  Within one wave LDS accesses execute
// in order, so no barrier stands between the stores and those reads.
template <typename T, int R>
__device__ inline void ghost_rows_coop(const PgdParams<T>& p, const T* A, T* GH, int side, int a, int b) {
  using L = Layout<T, R>;
  constexpr int V = L::V;
  static_assert(R <= L::NA, "one ghost row per lane of a column group");
  if (a < R) {
    const T* src = A + ((side == 0 ? 0 : TY + R) + a) * L::AP + V * b;  // window row of ghost row a's first tap
    T gh[V];
#pragma unroll
    for (int v = 0; v < V; ++v) gh[v] = T(0);
#pragma unroll
    for (int s = 0; s <= 2 * R; ++s) {
      T w[V];
      ld_vec<T, V>(src + s * L::AP, w);
#pragma unroll
      for (int v = 0; v < V; ++v) gh[v] = fma(p.k0[s], w[v], gh[v]);
    }
    st_vec<T, V>(GH + (b * R + a) * V, gh);
  }
}

// `C`: the tile's class.  Col tiles run the interior stream (their rows are interior); row and corner tiles correct the items
// within R rows of their border from the ghost rows of ghost_rows_coop, tap indices known at compile time per row group.
template <typename T, int R, int C, int D = 0>
__device__ inline void pass_a(const PgdParams<T>& p, const T* A, T* PT, const T* KT, T* GH, int ty0, int tid = threadIdx.x) {
  using L = Layout<T, R>;
  constexpr int V = L::V;
  constexpr int KA = cdiv(L::NPA, kThreads);
  constexpr bool EDGE = C == kTileGeneric;
  // one item per thread (fp32), in thread order: the 176 items of R = 6 fill waves 0, 1 and three quarters of wave 2; wave 3
  // has none.  Spreading them over four waves would issue four wave-passes instead of three for the same work.
  const bool edge_rows = EDGE && (ty0 < R || ty0 + TY > p.n0 - R);
#pragma unroll
  for (int k = 0; k < KA; ++k) {
    const int it = tid + k * kThreads;
    if (it < L::NPA) {
      const int a = it % L::NA, b = it / L::NA;  // row group fastest (conflict-free reads/writes)
      T acc[V][V];
      if constexpr (C == kTileRow) {
        static_assert(KA == 1 && L::NPA % L::NA == 0 && 64 % L::NA == 0, "a column group is NA lanes of one wave");
        static_assert(V == 4 && L::NA == 8 && R <= 8, "the row groups within R of a border: two on each side");
        const int side = row_side(ty0);
        ghost_rows_coop<T, R>(p, A, GH, side, a, b);
        sweep<T, R, V, L::AP, D>(A + (V * a) * L::AP + V * b, p.g0, acc);
        __builtin_amdgcn_wave_barrier();
        asm volatile("" ::: "memory");  // the compiler keeps the reads below behind the group's stores
        const T* gh = GH + b * R * V;
        if (side == 0) {
          if (a == 0) ghost_sub<T, R, V, V, V, false, 0>(p.k0, gh, acc);
          if (R > V && a == 1) ghost_sub<T, R, V, V, V, false, V>(p.k0, gh, acc);
        } else {
          if (a == L::NA - 1) ghost_sub<T, R, V, V, V, true, V - 1>(p.k0, gh, acc);
          if (R > V && a == L::NA - 2) ghost_sub<T, R, V, V, V, true, 2 * V - 1>(p.k0, gh, acc);
        }
      } else {
        sweep<T, R, V, L::AP, D>(A + (V * a) * L::AP + V * b, p.g0, acc);
      }
      if (edge_rows) ghost_fix<T, R, V, L::AP>(ty0 + V * a, p.n0, ty0 - 2 * R, A + V * b, p.k0, KT, acc);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        T colv[V];
#pragma unroll
        for (int u = 0; u < V; ++u) colv[u] = acc[u][v];
        st_vec<T, V>(PT + (V * b + v) * pt_pitch<T, R>() + V * a, colv);
      }
    }
  }
}

__device__ inline void st_pair(float* p, float a, float b) { *reinterpret_cast<float2*>(p) = make_float2(a, b); }

// ---- TV dual of a pass-B block (fp32): Grad^T q at the block's own 2 x 4 pixels needs q there, q0 one row above
// (4 values) and q1 one column to the left (2 values).
// Exchange form (R >= 6, where A's rows above / below the TV stencil's reach hold it): q is evaluated once per pixel.
// A block evaluates its own 8, writes its last row's q0 and last column's q1 to an exchange area in A's rows that
// pass B no longer reads, lanes 0..47 of the wave evaluate the wave's halo (32 q0 of the row above its 16 x 32
// region, 16 q1 of the column to its left), and every block reads its neighbours' values back.  Within one wave LDS
// accesses execute in order, so no barrier and no drain is needed between the stores and the reads.
// Window form (smaller R): q on the block's 3 x 5 window (15 evaluations for 8 pixels).
// Same q expressions in both, the same as the fp64 items': same bits.
// per wave: q0 [row pair + 1][32 cols at pitch 40: the row pairs of a ds_read_b128 lane group, two apart, are 16 banks
// apart], q1 [col item + 1][16 rows]
constexpr int kTvxP0 = 40;
template <typename T, int R>
constexpr int kTvxFloats = 9 * kTvxP0 + 9 * BlockB<T, R>::WR;

// `C`: the tile's class.  Generic tiles test every q's pixel against the image; in a col or row tile the only pixels
// outside are the column left of a first-column tile and the row above a top-row tile (q of the last column / row is
// evaluated from the zeros beyond it, as everywhere), so only those halo evaluations are zeroed (`zq`); a corner tile
// can have both.
template <typename T, int R, int C>
__device__ inline void tv_block(const PgdParams<T>& p, T* A, int ty0, int tx0, int wv, int ln, T (&yc)[2][4],
                                T (&tv)[2][4], bool corner) {
  using L = Layout<T, R>;
  using B = BlockB<T, R>;
  constexpr int CA = L::CA, AP = L::AP;
  constexpr bool EDGE = C == kTileGeneric;
  const bool first_row = C == kTileRow && row_side(ty0) == 0;             // the row above the tile is outside
  const bool first_col = has_col<C>(corner) && col_side(tx0) == 0;  // the column left of it is
  constexpr bool kExchange = (2 * R - 1) * AP >= 2 * kTvxFloats<T, R>;
  const int n0 = p.n0, n1 = p.n1;
  int rpl, cil, wr0, wc0;
  B::item(wv, ln, rpl, cil, wr0, wc0);
  const int r0 = wr0 + 2 * rpl, c0 = wc0 + 4 * cil;  // the block's first pixel (tile-relative)
  const T* own = A + (r0 + 2 * R) * AP + CA + c0;
  auto qat = [&](T yc_, T ydn, T yrt, int gr, int gc, T& q0, T& q1, bool zq = false) {
    const T v0 = fma(p.g0a, yc_, p.g0b * ydn);
    const T v1 = fma(p.g1a, yc_, p.g1b * yrt);
    T w = tv_weight<T>(fma(v0, v0, v1 * v1), p.lam, p.mu, p.inv_mu);
    if (EDGE && !(gr >= 0 && gr < n0 && gc >= 0 && gc < n1)) w = T(0);
    if (zq) w = T(0);
    q0 = v0 * w;
    q1 = v1 * w;
  };
  if constexpr (kExchange) {
    // own rows and the row below (16-B vectors), the column to the right of the own rows
    T y[3][5];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      T m[4];
      ld_vec<T, 4>(own + r * AP, m);
#pragma unroll
      for (int w = 0; w < 4; ++w) y[r][w] = m[w];
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      T hi[2];
      ld_pair<T>(own + r * AP + 4, hi);
      y[r][4] = hi[0];
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int w = 0; w < 4; ++w) yc[u][w] = y[u][w];
    if (!p.tv) return;
    T q0[2][4], q1[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int w = 0; w < 4; ++w)
        qat(y[u][w], y[u + 1][w], y[u][w + 1], ty0 + r0 + u, tx0 + c0 + w, q0[u][w], q1[u][w]);
    // exchange area of this wave: waves 0, 1 (tile rows 0..15) in A's top dead rows, 2, 3 in the bottom ones
    T* E0 = (wv < 2 ? A : A + (TY + 2 * R + 1) * AP) + (wv & 1) * kTvxFloats<T, R>;  // [row pair + 1][col of the 32]
    T* E1 = E0 + 9 * kTvxP0;                                                         // [col item + 1][row of the 16]
    if (ln < 48) {
      T hq0, hq1;
      if (ln < 32) {  // q0 of the row above the region
        const int tc = wc0 + ln;
        const T* h = A + (wr0 - 1 + 2 * R) * AP + CA + tc;
        qat(h[0], h[AP], h[1], ty0 + wr0 - 1, tx0 + tc, hq0, hq1, first_row && wr0 == 0);
        E0[ln] = hq0;
      } else {  // q1 of the column left of the region
        const int j = ln - 32, tc = wc0 - 1;
        const T* h = A + (wr0 + j + 2 * R) * AP + CA + tc;
        qat(h[0], h[AP], h[1], ty0 + wr0 + j, tx0 + tc, hq0, hq1, first_col && wc0 == 0);
        E1[j] = hq1;
      }
    }
    st_vec<T, 4>(E0 + (rpl + 1) * kTvxP0 + 4 * cil, q0[1]);
    st_pair(E1 + (cil + 1) * B::WR + 2 * rpl, q1[0][3], q1[1][3]);
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");  // the compiler keeps the reads below behind the stores above
    T up[4], left[2];
    ld_vec<T, 4>(E0 + rpl * kTvxP0 + 4 * cil, up);
    ld_pair<T>(E1 + cil * B::WR + 2 * rpl, left);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const T qa = u == 0 ? up[w] : q0[0][w];
        const T ql = w == 0 ? left[u] : q1[u][w - 1];
        const T t0 = fma(p.g0b, qa, p.g0a * q0[u][w]);
        const T t1 = fma(p.g1b, ql, p.g1a * q1[u][w]);
        tv[u][w] = t0 + t1;
      }
  } else {
    // yk window rows r0 - 1 .. r0 + 2, columns c0 - 1 .. c0 + 4, streamed two rows at a time so that the stencil keeps
    // ~25 values live instead of the whole 4 x 6 window
    auto yrow = [&](int r, T(&y)[6]) {
      const T* arow = own + (r - 1) * AP;
      T m[4];
      ld_vec<T, 4>(arow, m);
      y[0] = arow[-1];
#pragma unroll
      for (int w = 0; w < 4; ++w) y[w + 1] = m[w];
      y[5] = arow[4];
    };
    // q at window row r, columns c0 - 1 .. c0 + 3, from yk rows r (yr) and r + 1 (yn)
    auto qrow = [&](int r, const T(&yr)[6], const T(&yn)[6], T(&q0)[5], T(&q1)[5]) {
#pragma unroll
      for (int c = 0; c < 5; ++c)
        qat(yr[c], yn[c], yr[c + 1], ty0 + r0 - 1 + r, tx0 + c0 - 1 + c, q0[c], q1[c],
            (first_col && c == 0 && c0 == 0) || (first_row && r == 0 && r0 == 0));
    };
    T yr[6], yn[6];
    yrow(0, yr);
    yrow(1, yn);
    T qp0[5], qp1[5];
    if (p.tv) qrow(0, yr, yn, qp0, qp1);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int c = 0; c < 6; ++c) yr[c] = yn[c];  // window row u + 1
      yrow(u + 2, yn);
#pragma unroll
      for (int w = 0; w < 4; ++w) yc[u][w] = yr[w + 1];
      if (p.tv) {
        T qc0[5], qc1[5];
        qrow(u + 1, yr, yn, qc0, qc1);
        // Grad^T q: flipped 2-tap adjoints, (+1/h tap at i - e_d) then (-1/h tap at i), summed over d
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const T t0 = fma(p.g0b, qp0[w + 1], p.g0a * qc0[w + 1]);
          const T t1 = fma(p.g1b, qc1[w], p.g1a * qc1[w + 1]);
          tv[u][w] = t0 + t1;
        }
#pragma unroll
        for (int c = 0; c < 5; ++c) qp0[c] = qc0[c];
      }
    }
  }
}

// ---- pass B on Layout's items (fp64): G1 along rows + Grad^T q, handed per output row-run to
// `emit(k, u, gr, gc, g, yc)`: g = (G yk + Grad^T q) at row gr, columns gc .. gc + CW - 1 of item k,
// yc = yk there.  The emitter finishes the pixels in place (finish_run) or stages g for the
// coalesced epilogue (epilogue_staged).
template <typename T, int R, bool EDGE, typename Emit, int D = 0>
__device__ inline void pass_b(const PgdParams<T>& p, const T* A, const T* PT, const T* KT, const T* GH, int ty0, int tx0,
                              Emit&& emit, int tid = threadIdx.x) {
  using L = Layout<T, R>;
  constexpr int V = L::V;
  constexpr int CA = L::CA;
  constexpr int CW = L::CW;
  const int n0 = p.n0, n1 = p.n1;
  constexpr int KB = cdiv(L::NPB, kThreads);
  const bool edge_cols = EDGE && (tx0 < R || tx0 + TX > n1 - R);
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    const int it = tid + k * kThreads;
    if (it < L::NPB) {
      int a, cb;
      L::pass_b_item(it, a, cb);
      const int c0 = CW * cb;  // first output column of the item (tile-relative)
      // yk window rows V a - 1 .. V a + V, cols c0 - 1 .. c0 + CW, streamed two rows at a time so
      // that the TV stencil keeps ~20 values live instead of the whole (V+2) x (CW+2) window
      auto yrow = [&](int r, T(&y)[CW + 2]) {
        const T* arow = A + (V * a - 1 + r + 2 * R) * L::AP + CA + c0;
        if constexpr (CW == 2) {
          T lo[2], mid[2], hi[2];
          ld_pair<T>(arow - 2, lo);
          ld_pair<T>(arow, mid);
          ld_pair<T>(arow + 2, hi);
          y[0] = lo[1];
          y[1] = mid[0];
          y[2] = mid[1];
          y[3] = hi[0];
        } else {
#pragma unroll
          for (int c = 0; c < CW + 2; ++c) y[c] = arow[c - 1];
        }
      };
      // q = w v at window row r (0..V), cols c = 0..CW, from yk rows r (yr) and r + 1 (yn)
      auto qrow = [&](int r, const T(&yr)[CW + 2], const T(&yn)[CW + 2], T(&q0)[CW + 1], T(&q1)[CW + 1]) {
#pragma unroll
        for (int c = 0; c <= CW; ++c) {
          const T v0 = fma(p.g0a, yr[c], p.g0b * yn[c]);
          const T v1 = fma(p.g1a, yr[c], p.g1b * yr[c + 1]);
          T w = tv_weight<T>(fma(v0, v0, v1 * v1), p.lam, p.mu, p.inv_mu);
          if (EDGE) {
            const int gr = ty0 + V * a - 1 + r, gc = tx0 + c0 - 1 + c;
            if (!(gr >= 0 && gr < n0 && gc >= 0 && gc < n1)) w = T(0);
          }
          q0[c] = v0 * w;
          q1[c] = v1 * w;
        }
      };
      T yc[V][CW];  // yk at the item's own pixels
      T tv[V][CW];
      {
        T yr[CW + 2], yn[CW + 2];
        yrow(0, yr);
        yrow(1, yn);
        T qp0[CW + 1], qp1[CW + 1];
        if (p.tv) qrow(0, yr, yn, qp0, qp1);
#pragma unroll
        for (int u = 0; u < V; ++u) {
#pragma unroll
          for (int c = 0; c < CW + 2; ++c) yr[c] = yn[c];  // window row u + 1
          yrow(u + 2, yn);
#pragma unroll
          for (int w = 0; w < CW; ++w) yc[u][w] = yr[w + 1];
          if (p.tv) {
            T qc0[CW + 1], qc1[CW + 1];
            qrow(u + 1, yr, yn, qc0, qc1);
            // Grad^T q: flipped 2-tap adjoints, (+1/h tap at i - e_d) then (-1/h tap at i), summed over d
#pragma unroll
            for (int w = 0; w < CW; ++w) {
              const T t0 = fma(p.g0b, qp0[w + 1], p.g0a * qc0[w + 1]);
              const T t1 = fma(p.g1b, qc1[w], p.g1a * qc1[w + 1]);
              tv[u][w] = t0 + t1;
            }
#pragma unroll
            for (int c = 0; c <= CW; ++c) qp0[c] = qc0[c];
          }
        }
      }
      T acc[CW][V];            // acc[w][u]: column c0 + w, row V a + u
      sweep<T, R, CW, L::PTP, D>(PT + (CA - 2 * R + c0) * L::PTP + V * a, p.g1, acc);
      if (edge_cols) ghost_fix_pre<T, R, CW, TY>(tx0 + c0, n1, V * a, GH, KT + kKT, acc);
#pragma unroll
      for (int u = 0; u < V; ++u) {
        T g[CW], y[CW];
#pragma unroll
        for (int w = 0; w < CW; ++w) {
          g[w] = p.tv ? acc[w][u] + tv[u][w] : acc[w][u];
          y[w] = yc[u][w];
        }
        emit(k, u, ty0 + V * a + u, tx0 + c0, g, y);
      }
    }
  }
}

// ---- staged epilogue (fp64): every thread parks g = G yk + Grad^T q of its pass-B pixels in O (the PT
// region, free once all G1 sweeps are done), then the workgroup finishes the tile in row-major order:
// each 16-B vector of a row is one lane (16 lanes per fp32 row), so the H^T y / x loads and the x_new
// stores are full 128-B lines instead of the pass-B item order's 64-B row pieces (measured on MI355X: a
// 2048^2 fp32 store in the item order 7.2 us, row-major 5.2 us).  yk comes from A.
// StagedB: H^T y (and x, when the RelError partials need it) of this thread's epilogue vectors, zero
// outside the image; H^T y is issued before the O staging so that its latency overlaps it.
template <typename T, int R>
struct StagedB {
  static constexpr int NS = TY / Stage<T, R>::RPS;
  T v[NS][kVecN<T>];
  T x[NS][kVecN<T>];
};

// a whole 16-B vector of row gr at column gc lies inside the image and can be moved as one access
template <typename T>
__device__ inline bool vec_inside(const PgdParams<T>& p, int gr, int gc) {
  return p.vec_ok && gr < p.n0 && gc + kVecN<T> <= p.n1;
}

// byte offset of the row-major epilogue lane's vector of sweep s (Stage::lane: tile row r0 + s RPS, vector cq) from
// the tile's first pixel.  The sweep's row shift is added here, in 32 bits (one add per sweep, shared by the H^T y / x
// loads and the x_new store): as a shift of the uniform base the compiler re-associated it into 64-bit vector adds.
template <typename T, int R>
__device__ inline unsigned stage_voff(int r0, int cq, int n1, int s) {
  return (unsigned)((r0 + s * Stage<T, R>::RPS) * n1 + kVecN<T> * cq) * (unsigned)sizeof(T);
}

template <typename T, int R, bool EDGE>
__device__ inline void load_staged(const PgdParams<T>& p, int ty0, int tx0, const T* __restrict__ src, T (&v)[StagedB<T, R>::NS][kVecN<T>],
                                   int lt = threadIdx.x) {
  using S = Stage<T, R>;
  constexpr int V = kVecN<T>;
  const int n0 = p.n0, n1 = p.n1;
  int r0, cq;
  S::lane(lt, r0, cq);
#pragma unroll
  for (int s = 0; s < StagedB<T, R>::NS; ++s) {  // all loads first: one round trip
    const int gr = ty0 + r0 + s * S::RPS, gc = tx0 + V * cq;
    if (!EDGE) {  // (uniform base + 32-bit lane offset: lane_ptr)
      ld_vec<T, V>(lane_ptr<const T>(src, ty0, tx0, n1, 0, stage_voff<T, R>(r0, cq, n1, s)), v[s]);
    } else if (vec_inside(p, gr, gc)) {  // edge tile, but this vector is inside: one 16-B load
      ld_vec<T, V>(src + (int64_t)gr * n1 + gc, v[s]);
    } else {
#pragma unroll
      for (int w = 0; w < V; ++w) v[s][w] = (gr < n0 && gc + w < n1) ? src[(int64_t)gr * n1 + gc + w] : T(0);
    }
  }
}

// z = ((G yk + Grad^T q) - H^T y) * (-tau) + yk; x_new = prox(z); RelError partials sum (x_new - x)^2,
// sum x^2 in double.  One 16-B vector of one tile row; `vdst`: its address in x_new (interior tiles: from lane_ptr).
template <typename T, bool EDGE>
__device__ inline void finish_vec(const PgdParams<T>& p, int gr, int gc, const T (&g)[kVecN<T>], const T (&bv)[kVecN<T>],
                                  const T (&yc)[kVecN<T>], const T (&xv)[kVecN<T>], T* __restrict__ xns, T* vdst,
                                  bool want_part, double& part_d, double& part_x) {
  constexpr int V = kVecN<T>;
  const int n0 = p.n0, n1 = p.n1;
  T xo[V];
#pragma unroll
  for (int w = 0; w < V; ++w) {
    const T gsum = g[w] - bv[w];  // (G yk + Grad^T q) - H^T y
    const T z = fma(gsum, -p.tau, yc[w]);
    xo[w] = apply_prox<T>(p.prox, z, p.pw);
  }
  const bool whole = !EDGE || vec_inside(p, gr, gc);
  if (whole) {
    st_vec<T, V>(EDGE ? xns + ((int64_t)gr * n1 + gc) : vdst, xo);
    if (want_part) {
#pragma unroll
      for (int w = 0; w < V; ++w) {
        const double dd = (double)xo[w] - (double)xv[w];
        part_d = fma(dd, dd, part_d);  // explicit: the vector and scalar paths must contract alike
        part_x = fma((double)xv[w], (double)xv[w], part_x);
      }
    }
  } else if (gr < n0) {
#pragma unroll
    for (int w = 0; w < V; ++w) {
      if (gc + w < n1) {
        xns[(int64_t)gr * n1 + gc + w] = xo[w];
        if (want_part) {
          const double dd = (double)xo[w] - (double)xv[w];
          part_d = fma(dd, dd, part_d);
          part_x = fma((double)xv[w], (double)xv[w], part_x);
        }
      }
    }
  }
}

// RelError partials per wavefront: lane 0 of the wave writes its (sum (x_new - r)^2, sum r^2), r = x_ref or x, to
// partials[2 slot .. 2 slot + 1], slot = tile * kPartWaves + wave (fixed-order shuffle fold, no barrier).
constexpr int kPartWaves = kThreads / 64;

__device__ inline void wave_partials(double part_d, double part_x, double* partials, unsigned slot) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    part_d += __shfl_down(part_d, off, 64);
    part_x += __shfl_down(part_x, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    // relaxed device-scope atomic stores: written through to the memory side (past this XCD's L2), so that the
    // last-workgroup fold (tail_fold) on any XCD can read them without a release fence -- a device-scope fence
    // per workgroup writes back the whole L2 (r05f: the kernel took 242 us instead of 25 with one)
    __hip_atomic_store(partials + 2 * slot, part_d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(partials + 2 * slot + 1, part_x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- pass B and the epilogue of the fp32 tile on 2 x 4 row-major blocks (tile2d.hpp BlockB): one block per thread,
// G1 swept along the block's 4 columns over b64 rows of PT (its two tile rows), Grad^T q from tv_block, then the block's
// two 16-B row vectors are finished in registers: H^T y (and x for the RelError partials) loaded straight into the
// lane that stores x_new.  H^T y is loaded behind the TV chain, so that the sweep covers its latency; x (RelError
// partials only) behind the sweep.
// The sweep has two forms, chosen by what the kernel's registers allow (scripts/pgd_window_isa.py --all):
//   R >= 4  sweep_w: all 4R + 4 PT rows read back to back as single ds_read_b64 and held at once (2 VGPRs each), the FMAs
//           compiler-scheduled behind counted waits.  The fastest form measured at R = 6 (profiles/pgd_blocks_ab.txt).
//   R <= 3  RowSweep: a ring of 4 rows, FMAs row by row.  These kernels hold 60-80 VGPRs for 6-8 workgroups per CU; with
//           every row live they take 68 / 76 / 84 and lose an occupancy step.
template <int R>
constexpr bool kRowsLiveB = R >= 4;
constexpr int kRingB = 4;

template <typename T, int R, int C, typename Mark>
__device__ inline void pass_b_blocks(const PgdParams<T>& p, T* A, const T* PT, const T* KT, const T* GH, int ty0, int tx0,
                                     const T* __restrict__ bs, const T* __restrict__ xrs, T* __restrict__ xns,
                                     bool want_part, double& part_d, double& part_x, int tid, Mark&& tmark, bool corner) {
  using L = Layout<T, R>;
  using B = BlockB<T, R>;
  constexpr int CA = L::CA, PTP = B::PTP;
  constexpr bool EDGE = C == kTileGeneric;  // (col and row tiles: every own vector is inside, the interior's lane_ptr form)
  const int n0 = p.n0, n1 = p.n1;
  const bool edge_cols = EDGE && (tx0 < R || tx0 + TX > n1 - R);
  int wv, ln;
  wave_lane(tid, wv, ln);
  int rpl, cil, wr0, wc0;
  B::item(wv, ln, rpl, cil, wr0, wc0);
  const int r0 = wr0 + 2 * rpl, c0 = wc0 + 4 * cil;  // the block's first pixel (tile-relative)
  // interior tiles: wave-uniform base (the region's first pixel) + 32-bit lane offset (lane_ptr)
  auto voff = [&](int q) { return (unsigned)((2 * rpl + q) * n1 + 4 * cil) * (unsigned)sizeof(T); };
  auto load_rows = [&](const T* __restrict__ src, T(&v)[2][4]) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int gr = ty0 + r0 + q, gc = tx0 + c0;
      if (!EDGE) {
        ld_vec<T, 4>(lane_ptr<const T>(src, ty0, tx0 + wc0, n1, wr0, voff(q)), v[q]);
      } else if (vec_inside(p, gr, gc)) {  // edge tile, but this vector is inside: one 16-B load
        ld_vec<T, 4>(src + (int64_t)gr * n1 + gc, v[q]);
      } else {
#pragma unroll
        for (int w = 0; w < 4; ++w) v[q][w] = (gr < n0 && gc + w < n1) ? src[(int64_t)gr * n1 + gc + w] : T(0);
      }
    }
  };
  T bv[2][4], xv[2][4];
  auto load_epilogue = [&]() {
    if (kProbes && (p.diag & 512)) {  // timing probe only (WRONG results): no H^T y loads
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int w = 0; w < 4; ++w) bv[q][w] = T(0);
    } else {
      load_rows(bs, bv);
    }
  };
  T yc[2][4], tv[2][4], acc[4][2];  // acc[w][q]: column c0 + w, row r0 + q
  if (kProbes && (p.diag & 64)) {   // timing probe only (WRONG results): no TV chain, no sweep
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int w = 0; w < 4; ++w) yc[q][w] = tv[q][w] = acc[w][q] = A[tid + q * 64 + w];
    load_epilogue();
    tmark(5);
  } else {
    const T* src = PT + (CA - 2 * R + c0) * PTP + r0;
    if constexpr (kRowsLiveB<R>) {
      tv_block<T, R, C>(p, A, ty0, tx0, wv, ln, yc, tv, corner);
      tmark(5);
      load_epilogue();
      sweep_w<T, R, 4, 2, PTP>(src, p.g1, acc);
    } else {
      T g1[4 * R + 1];  // the G1 taps in scalar registers before the first PT read
#pragma unroll
      for (int k = 0; k <= 4 * R; ++k) {
        g1[k] = p.g1[k];
        asm volatile("" : "+s"(g1[k]));
      }
      RowSweep<T, R, 4, 2, PTP, kRingB> sw;
      tv_block<T, R, C>(p, A, ty0, tx0, wv, ln, yc, tv, corner);
      tmark(5);
      load_epilogue();
      sw.start(src);
      sw.run(src, g1, acc);
    }
    if (edge_cols) ghost_fix_pre_w<T, R, 4, 2, TY>(tx0 + c0, n1, r0, GH, KT + kKT, acc);
    if (has_col<C>(corner)) {
      // ghost_fix_pre_w specialised on the side and on the block's column: only the blocks that hold a column within
      // R of the border do anything, with constant tap indices (p.k1) and GH offsets
      static_assert(R <= 8, "columns within R of a border: two blocks on each side");
      if (col_side(tx0) == 0) {
        if (c0 == 0) ghost_sub<T, R, 4, 2, TY, false, 0>(p.k1, GH + r0, acc);
        if (R > 4 && c0 == 4) ghost_sub<T, R, 4, 2, TY, false, 4>(p.k1, GH + r0, acc);
      } else {
        if (c0 == TX - 4) ghost_sub<T, R, 4, 2, TY, true, 3>(p.k1, GH + R * TY + r0, acc);
        if (R > 4 && c0 == TX - 8) ghost_sub<T, R, 4, 2, TY, true, 7>(p.k1, GH + R * TY + r0, acc);
      }
    }
  }
  // x (RelError partials only) behind the sweep: issued under a branch ahead of it, its registers would be copied, and
  // so waited for, where the branches join
  if (want_part) load_rows(xrs, xv);
  tmark(6);
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    T g[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) g[w] = p.tv ? acc[w][q] + tv[q][w] : acc[w][q];
    if (kProbes && (p.diag & 1024)) {  // timing probe only (WRONG results): no x_new stores
      if (g[0] + yc[q][0] + bv[q][0] == T(-12345)) xns[0] = T(0);
      continue;
    }
    T* vdst = EDGE ? nullptr : lane_ptr<T>(xns, ty0, tx0 + wc0, n1, wr0, voff(q));
    finish_vec<T, EDGE>(p, ty0 + r0 + q, tx0 + c0, g, bv[q], yc[q], xv[q], xns, vdst, want_part, part_d, part_x);
  }
}

// ---- pass B and the staged epilogue of the fp64 tile (Layout's 2 x 1 items): every thread parks its results in
// registers, loads H^T y, stages them through O and the workgroup finishes the tile in row-major order.
template <typename T, int R, bool EDGE, int D, typename Mark>
__device__ inline void pass_b_staged(const PgdParams<T>& p, T* A, T* PT, const T* KT, const T* GH, int ty0, int tx0,
                                     const T* __restrict__ bs, const T* __restrict__ xrs, T* __restrict__ xns,
                                     bool want_part, double& part_d, double& part_x, int tid, Mark&& tmark) {
  using L = Layout<T, R>;
  using S = Stage<T, R>;
  constexpr int CW = L::CW;
  constexpr int V = L::V;
  constexpr int KB = cdiv(L::NPB, kThreads);
  const int n1 = p.n1;
  const bool skip_passes = kProbes && (p.diag & 64) != 0;  // timing probe only (WRONG results)
  T st[KB][V][CW];
  if (skip_passes) {
#pragma unroll
    for (int k = 0; k < KB; ++k)
#pragma unroll
      for (int u = 0; u < V; ++u)
#pragma unroll
        for (int w = 0; w < CW; ++w) st[k][u][w] = A[tid + u * 64 + w];
  } else
  {
    auto park = [&](int k, int u, int, int, const T(&g)[CW], const T(&)[CW]) {
#pragma unroll
      for (int w = 0; w < CW; ++w) st[k][u][w] = g[w];
    };
    pass_b<T, R, EDGE, decltype(park)&, D>(p, A, PT, KT, GH, ty0, tx0, park, tid);
  }
  StagedB<T, R> hb;
  if (kProbes && (p.diag & 512)) {  // timing probe only (WRONG results): no H^T y loads
#pragma unroll
    for (int s = 0; s < StagedB<T, R>::NS; ++s)
#pragma unroll
      for (int w = 0; w < kVecN<T>; ++w) hb.v[s][w] = T(0);
  } else {
#if PXA_PGD_PRIO_EPI
    __builtin_amdgcn_s_setprio(PXA_PGD_PRIO_EPI);
#endif
    load_staged<T, R, EDGE>(p, ty0, tx0, bs, hb.v, tid);  // in flight during the O staging
#if PXA_PGD_PRIO_EPI
    __builtin_amdgcn_s_setprio(0);
#endif
  }
  tmark(5);
  __syncthreads();  // every G1 sweep is done with PT: O may overwrite it
  T* O = PT;
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    const int it = tid + k * kThreads;
    if (it < L::NPB) {
      int a, cb;
      L::pass_b_item(it, a, cb);
#pragma unroll
      for (int u = 0; u < V; ++u) {
        T* o = O + S::idx(V * a + u, CW * cb);
        if constexpr (CW == 2) {
          const T pr[2] = {st[k][u][0], st[k][u][1]};
          if constexpr (sizeof(T) == 4) *reinterpret_cast<float2*>(o) = make_float2(pr[0], pr[1]);
          else st_vec<T, 2>(o, pr);
        } else {
          o[0] = st[k][u][0];
        }
      }
    }
  }
  // x (RelError partials only) is loaded once pass B's parked results are out of the registers
  if (want_part) load_staged<T, R, EDGE>(p, ty0, tx0, xrs, hb.x, tid);
  __syncthreads();
  tmark(6);
#if PXA_PGD_PRIO_FIN
  __builtin_amdgcn_s_setprio(PXA_PGD_PRIO_FIN);  // A/B builds: the finishing stores ahead of other passes
#endif
  {
    int r0, cq;
    S::lane(tid, r0, cq);
#pragma unroll
    for (int s = 0; s < StagedB<T, R>::NS; ++s) {
      const int r = r0 + s * S::RPS;
      T g[V], y[V];
      ld_vec<T, V>(O + S::idx(r, V * cq), g);
      ld_vec<T, V>(A + (r + 2 * R) * L::AP + L::CA + V * cq, y);
      if (kProbes && (p.diag & 1024)) {  // timing probe only (WRONG results): no x_new stores
        if (g[0] + y[0] + hb.v[s][0] == T(-12345)) xns[0] = T(0);  // keeps the loads and the O / A reads
        continue;
      }
      T* vdst = EDGE ? nullptr : lane_ptr<T>(xns, ty0, tx0, n1, 0, stage_voff<T, R>(r0, cq, n1, s));
      finish_vec<T, EDGE>(p, ty0 + r, tx0 + V * cq, g, hb.v[s], y, hb.x[s], xns, vdst, want_part, part_d, part_x);
    }
  }
}

// Rows in flight per G sweep (tile2d.hpp sweep's D): 0 = compiler-scheduled (default); A/B builds limit it
#ifndef PXA_PGD_SWEEP_DEPTH
#define PXA_PGD_SWEEP_DEPTH 0
#endif

// The phases of one output tile once its window is in A (behind a barrier): pass A, [ghost columns], then fp32: pass B
// and the epilogue on row-major blocks, no further barrier; fp64: pass B (parked in registers), the H^T y / x loads, O
// staging, row-major epilogue; [RelError partials].
template <typename T, int R, int C, int D>
__device__ inline void pgd_tile_body(const PgdParams<T>& p, unsigned char* smem, unsigned tile, int ty0, int tx0,
                                     const T* __restrict__ bs, T* __restrict__ xns, double* __restrict__ partials,
                                     const T* __restrict__ xrs, const int tid, bool corner) {
  using L = Layout<T, R>;
  T* A = reinterpret_cast<T*>(smem);
  T* PT = A + L::AR * L::AP;
  T* KT = PT + L::AC * L::PTP;  // H taps for runtime-indexed reads (boundary corrections)
  T* GH = reinterpret_cast<T*>(smem + kGhOff<T, R>);  // boundary-column ghost terms (edge-column tiles)
  constexpr bool EDGE = C == kTileGeneric;
  const int n1 = p.n1;
  const bool edge_cols = EDGE && (tx0 < R || tx0 + TX > n1 - R);
  double part_d = 0.0, part_x = 0.0;
  const bool want_part = partials != nullptr;
  const bool tracing = kProbes && (p.diag & 32) != 0;
  unsigned long long* ts = reinterpret_cast<unsigned long long*>(smem + kGhOff<T, R> + kPgdGhBytes<T, R>);
  auto tmark = [&](int pt) {
    if (tracing && (tid & 63) == 0) ts[(tid >> 6) * 8 + pt] = clock64();
  };
  tmark(2);
  const bool skip_passes = kProbes && (p.diag & 64) != 0;  // timing probe only (WRONG results)
  if (!skip_passes) pass_a<T, R, C, D>(p, A, PT, KT, GH, ty0, tid);
  tmark(3);
  __syncthreads();
  if (edge_cols) {
    ghost_cols_coop<T, R, pt_pitch<T, R>()>(p.k1, PT, GH, tx0, n1, tid);
    __syncthreads();
  }
  if (has_col<C>(corner)) {  // the one side that exists (a corner's row terms are dead behind the barrier above)
    ghost_cols_side<T, R, pt_pitch<T, R>()>(p.k1, PT, GH, col_side(tx0), tid);
    __syncthreads();
  }
  tmark(4);
  if constexpr (sizeof(T) == 4) {  // no barrier from here on: each thread finishes its own block
    pass_b_blocks<T, R, C>(p, A, PT, KT, GH, ty0, tx0, bs, xrs, xns, want_part, part_d, part_x, tid, tmark, corner);
  } else {
    pass_b_staged<T, R, EDGE, D>(p, A, PT, KT, GH, ty0, tx0, bs, xrs, xns, want_part, part_d, part_x, tid, tmark);
  }
  tmark(7);
  if (want_part) wave_partials(part_d, part_x, partials, tile * kPartWaves + (tid >> 6));
  const unsigned nb = gridDim.x, bid = blockIdx.x;
  // traced workgroups: 0 (a corner tile), 9 and grid/2 + 8 (at 2048^2 tiles (8, 1) and (4, 1): interior), grid-1 (a tile
  // of the image's first column: boundary-column corrections in the sweep of the waves that hold columns 0 .. 31),
  // 8 (at 2048^2 tile (0, 1): a top-row tile)
  if (tracing && (bid == 0 || bid == 9 || bid == nb / 2 + 8 || bid == nb - 1 || bid == 8)) {
    __syncthreads();
    const int slot = bid == 0 ? 0 : bid == 9 ? 1 : bid == nb / 2 + 8 ? 2 : bid == nb - 1 ? 3 : 4;
    if (tid < 32) g_tile_trace[slot * 32 + tid] = ts[tid];
  }
}


// The previous check's RelError statistics over this tile's pixels, from its window (win_part): sum (x - x_prev)^2,
// sum x_prev^2 per wave (outside the image both are 0: no contribution).
template <typename T, int R>
__device__ inline void win_partials(const Window<T, R>& w, double* __restrict__ partials, unsigned tile, const int tid) {
  using L = Layout<T, R>;
  double part_d = 0.0, part_x = 0.0;
#pragma unroll
  for (int k = 0; k < Window<T, R>::KI; ++k) {  // (items k < KI: the tile's own vectors, Window::item)
#pragma unroll
    for (int v = 0; v < L::V; ++v) {
      const double dd = (double)w.xv[k][v] - (double)w.pv[k][v];
      part_d = fma(dd, dd, part_d);
      part_x = fma((double)w.pv[k][v], (double)w.pv[k][v], part_x);
    }
  }
  // (DPP wave sums: the __shfl_down ladder of wave_partials is a chain of twelve LDS round trips, on the path to the
  // window's barrier here; the window statistics only have to agree with the epilogue ones to rounding)
  part_d = wave_sum_f64(part_d);
  part_x = wave_sum_f64(part_x);
  if ((tid & 63) == 0) {
    const unsigned slot = tile * kPartWaves + (tid >> 6);
    __hip_atomic_store(partials + 2 * slot, part_d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(partials + 2 * slot + 1, part_x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One output tile of the tile kernel: phase 0 (window) into A, then the body.
template <typename T, int R, int C>
__device__ inline void pgd_tile(const PgdParams<T>& p, unsigned char* smem, unsigned tile, int ty0, int tx0,
                                const T* __restrict__ xs, const T* __restrict__ xps, const T* __restrict__ bs,
                                T* __restrict__ xns, double* __restrict__ partials, const T* __restrict__ xrs,
                                bool corner = false) {
  using L = Layout<T, R>;
  T* A = reinterpret_cast<T*>(smem);
  T* KT = A + L::AR * L::AP + L::AC * L::PTP;
  const int tid = threadIdx.x;
  constexpr bool EDGE = C == kTileGeneric;
  if (EDGE && tid < 2 * R + 1) {
    KT[tid] = p.k0[tid];
    KT[kKT + tid] = p.k1[tid];
  }
  const bool tracing = kProbes && (p.diag & 32) != 0;
  unsigned long long* ts = reinterpret_cast<unsigned long long*>(smem + kGhOff<T, R> + kPgdGhBytes<T, R>);
  auto tmark = [&](int pt) {
    if (tracing && (tid & 63) == 0) ts[(tid >> 6) * 8 + pt] = clock64();
  };
  tmark(0);
#if PXA_PGD_PRIO
  __builtin_amdgcn_s_setprio(PXA_PGD_PRIO);  // the window loads issue ahead of other workgroups' passes
#endif
  if (kProbes && (p.diag & 128)) {  // timing probe only (WRONG results): no window loads, yk = 0
    for (int i = tid; i < L::AR * L::AP; i += kThreads) A[i] = T(0);
  } else {
    Window<T, R> w;
    win_issue<T, R, C>(p, ty0, tx0, xs, xps, w, tid, corner);
    win_store<T, R>(p, A, w, tid);
    if (p.win_part && partials != nullptr) win_partials<T, R>(w, partials, tile, tid);
  }
#if PXA_PGD_PRIO
  __builtin_amdgcn_s_setprio(0);
#endif
  tmark(1);
  __syncthreads();
  // fp64: the thread index laundered between the window and the body, so that the body derives its lane values afresh
  // instead of sharing them with the window phase and keeping them live across it: no scratch up to R = 6 and 84-117
  // VGPRs where sharing them spilled (profiles/pgd_window_isa.txt).  fp32 shares them: laundering there costs ~30
  // static VALU and changes nothing at R <= 6.
  int btid = tid;
  if constexpr (sizeof(T) == 8) asm volatile("" : "+v"(btid));
  pgd_tile_body<T, R, C, PXA_PGD_SWEEP_DEPTH>(p, smem, tile, ty0, tx0, bs, xns, p.win_part ? nullptr : partials, xrs,
                                                 btid, corner);
}

// (Opt-in: PXA_RELERR_SINK=1; gfx950-specific.)  The hand-off below uses no release / acquire: it is the first row
// of the measured write-through hand-off table of MI355X_MICROARCH.md ("Workgroup dispatch, XCD placement &
// inter-workgroup visibility": one lane per storing workgroup signals with an agent-scope atomic add behind every
// storing wave's s_waitcnt vmcnt(0) and a workgroup barrier; all payload stores and loads are sc1, i.e. relaxed
// agent-scope atomics; the workgroup whose add returned last reads).  That form is measured on gfx950 / ROCm 7.2,
// not an architectural guarantee of the HIP memory model, which is why the mode stays opt-in and the default fold is
// a separate launch (pxa_tile_partials_fold); A/B numbers with the mode on depend on it.
// The RelError statistics of this launch, folded by the workgroup that finishes last (saves the fold launch
// of a stop check: ~3.4 us of device time plus a launch gap per step at stop_rate 1).  No fences: a
// device-scope release fence writes back the whole L2 of the XCD, per workgroup.  Instead every wavefront's
// lane 0 has written its (tile, wave) partials with relaxed device-scope atomic stores (wave_partials: write-
// through to the memory side) and waits for them to complete (s_waitcnt vmcnt(0)) before the workgroup counts
// itself with one relaxed device-scope atomic add; the last workgroup reads the partials with device-scope
// atomic loads (memory side again), folds each (statistic, row) in the order of pxa_tile_partials_fold
// (fold_tile_stat: same bits), writes the values and then, once they have completed, the completion flags to
// the host buffer with system-scope atomic stores, and resets the counter for the next launch.
template <typename T>
__device__ inline void tail_fold(const PgdParams<T>& p, const double* __restrict__ partials) {
  __shared__ double red[kThreads / 64];
  __shared__ unsigned last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's partial stores have completed
  __syncthreads();
  if (threadIdx.x == 0)
    last = __hip_atomic_fetch_add(p.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1u : 0u;
  __syncthreads();
  if (!last) return;
  auto ld = [](const double* a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  for (int64_t q = 0; q < 2 * p.fold_rows; ++q) {
    const int64_t stat = q / p.fold_rows, r = q - stat * p.fold_rows;
    const double t = fold_tile_stat(partials + 2 * r * p.fold_per_row + stat, p.fold_per_row, red, ld);
    if (threadIdx.x == 0) __hip_atomic_store(p.fold_vals + q, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (threadIdx.x == 0) {
    __hip_atomic_store(p.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the values have reached host memory before the flags
    for (int64_t q = 0; q < 2 * p.fold_rows; ++q)
      __hip_atomic_store(p.fold_flags + q, p.fold_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// The extra workgroup of a pxa_pgd_tv2d_plan_step_wpub launch: the previous launch's partials folded in the order of
// pxa_tile_partials_fold (fold_tile_stat: same sum order, same bits; the narrow load form, so that this branch adds
// no registers to the tile kernel's allocation), the values stored write-through to host memory
// (system-scope relaxed atomic stores), then -- once they have completed -- the flags.
template <typename T>
__device__ inline void publish_prev(const PgdParams<T>& p, double* red) {
  for (int64_t q = 0; q < 2 * p.fold_rows; ++q) {
    const int64_t stat = q / p.fold_rows, r = q - stat * p.fold_rows;
    const double t = fold_tile_stat<false>(p.pub_src + 2 * r * p.fold_per_row + stat, p.fold_per_row, red);
    if (threadIdx.x == 0) __hip_atomic_store(p.pub_vals + q, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the values have reached host memory before the flags
    for (int64_t q = 0; q < 2 * p.fold_rows; ++q)
      __hip_atomic_store(p.pub_flags + q, p.pub_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

template <typename T, int R>
__global__ void __launch_bounds__(kThreads, 4) pgd_tv2d_kernel(PgdParams<T> p, const T* __restrict__ x,
                                                            const T* __restrict__ xp, const T* __restrict__ b,
                                                            T* __restrict__ xn, double* __restrict__ partials) {
  using L = Layout<T, R>;
  // the publishing workgroup is block 0: dispatched in the first round, its fold is done long before the last tiles
  // (as the last block it ran beside the second round and could outlast it); the tile workgroups' index is shifted by
  // one, which rotates the XCD bands by one XCD and keeps each band on one XCD
  const unsigned pub = p.pub_src != nullptr ? 1u : 0u;
  if (pub && blockIdx.x == 0) {  // (no barrier shared with the tile workgroups)
    __shared__ double red[kThreads / 64];
    publish_prev<T>(p, red);
    return;
  }
  const unsigned vb = blockIdx.x - pub;
  const bool timeline = kProbes && (p.diag & 32) != 0;
  [[maybe_unused]] const unsigned long long tl0 = timeline ? clock64() : 0ull;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  unsigned tile = xcd_tile(vb, p.ntiles);
  {  // the last XCD band walks backwards: an image's bottom-edge tiles (slower: boundary corrections)
     // are dispatched first instead of last, longest-first scheduling (2048^2: 29.2-29.3 -> 28.9-29.0 us)
    const unsigned nb = p.ntiles, q8 = nb >> 3, r8 = nb & 7u, g8 = vb & 7u;
    if (g8 == 7u) {
      const unsigned lo = 7u * q8 + (r8 < 7u ? r8 : 7u), len = q8 + (7u < r8 ? 1u : 0u);
      tile = lo + (len - 1u - (tile - lo));
    }
  }
  const unsigned tpi = (unsigned)p.tiles0 * (unsigned)p.tiles1;
  const unsigned s = tile / tpi;
  const unsigned tr = tile - s * tpi;
  const unsigned trow = tr / (unsigned)p.tiles1;
  const int ty0 = (int)trow * TY, tx0 = (int)(tr - trow * (unsigned)p.tiles1) * TX;
  const int64_t img = (int64_t)p.n0 * p.n1;
  const T* xs = x + (int64_t)s * img;
  const T* xps = xp + (int64_t)s * img;
  const T* bs = b + (int64_t)(s % (unsigned)p.y_images) * img;
  T* xns = xn + (int64_t)s * img;
  const T* xrs = (p.xref != nullptr ? p.xref : x) + (int64_t)s * img;
  // interior: the whole A window lies inside the image (so no boundary rows / columns of G either),
  // rows are 16-B aligned and a lane's 32-bit byte offset from the tile's window origin suffices (lane_ptr:
  // at most (AR n1 + AC) sizeof(T) < 2^32 for n1 <= kMaxInteriorN1) -> no bounds tests
  // col / row (fp32): the border cuts the window on one side only, along whole vectors / rows: the interior code on the
  // axis that is interior, the skipped halo and the boundary terms of G on the other (tile2d.hpp tile_class).  fp64 runs
  // them as generic tiles.
  [[maybe_unused]] int tl_cls = kTileGeneric;
  if constexpr (sizeof(T) == 4) {
    int cls = __builtin_amdgcn_readfirstlane(tile_class(p.n0, p.n1, ty0, tx0, R, L::CA, p.vec_ok));
    // measurement probe only: col, row and corner tiles on the generic path, as before the classes existed
    if (kProbes && (p.diag & 2048) && cls != kTileInterior) cls = kTileGeneric;
    // (A/B builds: corners alone on the generic path, the dispatch before the corner class)
    if (kProbes && (p.diag & 4096) && cls == kTileCorner) cls = kTileGeneric;
    if (kProbes) tl_cls = cls;
    if (cls == kTileInterior)
      pgd_tile<T, R, kTileInterior>(p, smem_raw, tile, ty0, tx0, xs, xps, bs, xns, partials, xrs);
    else if (cls == kTileCol)
      pgd_tile<T, R, kTileCol>(p, smem_raw, tile, ty0, tx0, xs, xps, bs, xns, partials, xrs);
    else if (cls == kTileRow || (kCornerPart<R> && cls == kTileCorner))  // one call: one copy of the row class's body
      pgd_tile<T, R, kTileRow>(p, smem_raw, tile, ty0, tx0, xs, xps, bs, xns, partials, xrs,
                               kCornerPart<R> && cls == kTileCorner);
    else
      pgd_tile<T, R, kTileGeneric>(p, smem_raw, tile, ty0, tx0, xs, xps, bs, xns, partials, xrs);
  } else {
    const bool interior = p.vec_ok && img <= 0x7fffffff && p.n1 <= kMaxInteriorN1 && ty0 - 2 * R >= 0 && ty0 + TY + 2 * R <= p.n0 &&
                          tx0 - L::CA >= 0 && tx0 + TX + L::CA <= p.n1;  // (tile_class() == kTileInterior)
    if (kProbes && interior) tl_cls = kTileInterior;
    if (interior)
      pgd_tile<T, R, kTileInterior>(p, smem_raw, tile, ty0, tx0, xs, xps, bs, xns, partials, xrs);
    else
      pgd_tile<T, R, kTileGeneric>(p, smem_raw, tile, ty0, tx0, xs, xps, bs, xns, partials, xrs);
  }
#if PXA_PROBES
  if (timeline) {
    __syncthreads();
    if (threadIdx.x == 0 && vb < kTimelineWgs) {
      g_tile_timeline[3 * vb] = tl0;
      g_tile_timeline[3 * vb + 1] = clock64();
      // XCC_ID (hwreg 20, bits 3:0) and HW_ID (hwreg 4, bits 15:0: wave, SIMD, pipe, CU, SH, SE) of this wave
      const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20), hw = __builtin_amdgcn_s_getreg((15 << 11) | 4);
      g_tile_timeline[3 * vb + 2] = (unsigned long long)tile | (unsigned long long)tl_cls << 32 |
                                    (unsigned long long)(xcc & 15u) << 36 | (unsigned long long)(hw & 0xffffu) << 40;
    }
  }
#endif
  if (p.fold_vals != nullptr) tail_fold<T>(p, partials);
}

thread_local int g_last_pgd_kernel = 0;  // pxa_pgd_tv2d_last_kernel

template <typename T, int R>
int launch_pgd(const PgdParams<T>& p, const void* x, const void* xp, const void* b, void* xn, double* partials,
               hipStream_t s) {
  g_last_pgd_kernel = 1;
  // Layout + the ghost terms (+ the timing trace under PXA_TUNE_PGD_DIAG bit 5)
  constexpr size_t kLds = 160 * 1024;  // per CU: the row tiles' ghost rows cost no resident workgroup
  static_assert(kLds / (kGhOff<T, R> + kPgdGhBytes<T, R>) == kLds / (kGhOff<T, R> + kGhBytes<T, R>), "LDS occupancy step lost");
  const size_t smem = kGhOff<T, R> + kPgdGhBytes<T, R> + ((p.diag & 32) ? 256 : 0);
  auto kern = pgd_tv2d_kernel<T, R>;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(kGhOff<T, R> + kPgdGhBytes<T, R> + 256));
    attr_set = true;
  }
  hipLaunchKernelGGL(kern, dim3(p.ntiles + (p.pub_src != nullptr ? 1u : 0u)), dim3(kThreads), smem, s, p, (const T*)x,
                     (const T*)xp, (const T*)b, (T*)xn, partials);
  return last_launch_status();
}


// Iteration-invariant parameters (taps folded per offset, G = k (*) k, geometry, prox kind); `R` the blur reach.
template <typename T>
int pgd_params(int64_t stack, int64_t y_images, int64_t n0, int64_t n1, int nt0, const int32_t* off0,
               const double* coef0, int nt1, const int32_t* off1, const double* coef1, double h0, double h1, double lam,
               double mu, int prox, PgdParams<T>& p, int& R) {
  PXA_CHECK_ARG(stack >= 1 && n0 >= 1 && n1 >= 1 && y_images >= 1 && stack % y_images == 0);
  PXA_CHECK_ARG(n0 <= 0x7fffffff && n1 <= 0x7fffffff);
  PXA_CHECK_ARG(prox >= 0 && prox <= 2);
  PXA_CHECK_ARG(nt0 >= 1 && nt1 >= 1 && off0 && off1 && coef0 && coef1);
  // H taps as dense windows in double (code-generation order folded per offset)
  TapWindow k0, k1;
  const int r0 = tap_window(nt0, off0, coef0, k0), r1 = tap_window(nt1, off1, coef1, k1);
  if (r0 < 0 || r1 < 0) return PXA_ERR_UNSUPPORTED;
  R = r0 > r1 ? r0 : r1;
  if (R < 1) R = 1;  // TV needs a 1-pixel halo even for a 1-tap blur
  p = PgdParams<T>{};
  p.stack = stack;
  p.y_images = y_images;
  p.n0 = (int)n0;
  p.n1 = (int)n1;
  p.tiles0 = (int)((n0 + TY - 1) / TY);
  p.tiles1 = (int)((n1 + TX - 1) / TX);
  const int64_t ntiles = stack * (int64_t)p.tiles0 * p.tiles1;
  PXA_CHECK_ARG(ntiles <= 0x7fffffff);
  p.ntiles = (unsigned)ntiles;
  // rows of the RelError statistics = rows of the solver state: y_images images each (batch-as-axis); the
  // slots of one image, hence of one row, are contiguous
  p.fold_rows = stack / y_images;
  p.fold_per_row = ntiles * (kThreads / 64) / p.fold_rows;
  tap_dense(k0, R, p.k0);
  tap_dense(k1, R, p.k1);
  tap_autocorr(k0, R, p.g0);  // G = k (*) k
  tap_autocorr(k1, R, p.g1);
  p.g0a = (T)(-1.0 / h0);
  p.g0b = (T)(1.0 / h0);
  p.g1a = (T)(-1.0 / h1);
  p.g1b = (T)(1.0 / h1);
  p.lam = (T)lam;
  p.mu = (T)mu;
  p.inv_mu = (T)(1.0 / mu);
  p.tv = lam != 0.0;
  p.prox = prox;
  return PXA_OK;
}

// One launch from prepared parameters: the per-step scalars and arrays, then the kernel of reach R.
template <typename T>
int pgd_run(PgdParams<T> p, int R, double a, double tau, double prox_w, const void* x, const void* x_prev,
            const void* hty, void* x_new, double* partials, const void* x_ref, double* rel_values, uint32_t* rel_flags,
            uint32_t seq, unsigned* counter, hipStream_t s, int win_part = 0, const double* pub_src = nullptr,
            double* pub_vals = nullptr, uint32_t* pub_flags = nullptr, uint32_t pub_seq = 0) {
  PXA_CHECK_ARG(x && x_prev && hty && x_new);
  PXA_CHECK_ARG(x_new != x && x_new != x_prev && x_new != x_ref);
  PXA_CHECK_ARG(rel_values == nullptr || (partials != nullptr && rel_flags != nullptr && counter != nullptr));
  p.a = (T)a;
  p.tau = (T)tau;
  p.pw = (T)prox_w;
  constexpr int V = kVecN<T>;
  p.vec_ok = (p.n1 % V == 0) && aligned16(x) && aligned16(x_prev) && aligned16(hty) && aligned16(x_new) &&
             (x_ref == nullptr || aligned16(x_ref));
  p.xref = (partials != nullptr && x_ref != nullptr && x_ref != x) ? (const T*)x_ref : nullptr;
  p.diag = kProbes ? tuning(PXA_TUNE_PGD_DIAG) : 0;
  p.fold_vals = rel_values;
  p.fold_flags = (unsigned*)rel_flags;
  p.fold_seq = (unsigned)seq;
  p.counter = counter;
  p.win_part = win_part;
  PXA_CHECK_ARG(!win_part || (partials != nullptr && rel_values == nullptr));
  PXA_CHECK_ARG(pub_src == nullptr || (pub_vals != nullptr && pub_flags != nullptr && pub_src != partials));
  p.pub_src = pub_src;
  p.pub_vals = pub_vals;
  p.pub_flags = (unsigned*)pub_flags;
  p.pub_seq = (unsigned)pub_seq;
  return with_radius<1>(R, [&](auto r) {
    return launch_pgd<T, decltype(r)::value>(p, x, x_prev, hty, x_new, partials, s);
  });
}

template <typename T>
int pgd_entry(int64_t stack, int64_t y_images, int64_t n0, int64_t n1, int nt0, const int32_t* off0,
              const double* coef0, int nt1, const int32_t* off1, const double* coef1, double h0, double h1, double lam,
              double mu, double a, double tau, int prox, double prox_w, const void* x, const void* x_prev,
              const void* hty, void* x_new, double* partials, const void* x_ref, hipStream_t s) {
  PgdParams<T> p;
  int R = 1;
  const int e = pgd_params<T>(stack, y_images, n0, n1, nt0, off0, coef0, nt1, off1, coef1, h0, h1, lam, mu, prox, p, R);
  if (e != PXA_OK) return e;
  return pgd_run<T>(p, R, a, tau, prox_w, x, x_prev, hty, x_new, partials, x_ref, nullptr, nullptr, 0, nullptr, s);
}

// pxa_pgd_tv2d_plan: the prepared parameters of one problem (both precisions' storage, one used) and the
// device counter of the last-workgroup fold
struct PgdPlan {
  int dtype;
  int R;
  PgdParams<float> pf;
  PgdParams<double> pd;
  int64_t fold_rows, fold_per_row;  // of the parameters in use: the shape pxa_tile_partials_fold folds
  unsigned* counter;
};

// One launch from a plan, `args` being pgd_run's arguments after (p, R): the dtype choice of every plan-step form.
template <typename... A>
int plan_run(const PgdPlan* pl, A... args) {
  return pl->dtype == PXA_F32 ? pgd_run<float>(pl->pf, pl->R, args...) : pgd_run<double>(pl->pd, pl->R, args...);
}

}  // namespace
}  // namespace pxa

using namespace pxa;

extern "C" {

int pxa_pgd_tv2d_last_kernel(void) { return g_last_pgd_kernel; }

int pxa_pgd_tile_trace(uint64_t* host_out, int n) {
  if (!kProbes) return PXA_ERR_UNSUPPORTED;  // the phase trace exists only in the probe build
  if (!host_out || n < 0 || n > kTraceWords) return PXA_ERR_ARG;
  if (hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_tile_trace), (size_t)n * 8, 0, hipMemcpyDeviceToHost) != hipSuccess)
    return PXA_ERR_UNSUPPORTED;
  return PXA_OK;
}

int pxa_pgd_tile_timeline(uint64_t* host_out, int nwg) {
#if PXA_PROBES
  if (!host_out || nwg < 0 || (unsigned)nwg > kTimelineWgs) return PXA_ERR_ARG;
  if (hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_tile_timeline), (size_t)nwg * 24, 0, hipMemcpyDeviceToHost) != hipSuccess)
    return PXA_ERR_UNSUPPORTED;
  return PXA_OK;
#else
  (void)host_out, (void)nwg;
  return PXA_ERR_UNSUPPORTED;  // the timeline exists only in the probe build
#endif
}

int pxa_pgd_tv2d_partials_count(int64_t stack, int64_t n0, int64_t n1) {
  int64_t t = stack * ((n0 + TY - 1) / TY) * ((n1 + TX - 1) / TX) * kPartWaves;
  return (int)t;
}

// the fp32 kernel's dispatch over every tile of the stack: by[c] = tiles of TileClass c
static int pgd_tile_census(int64_t stack, int64_t n0, int64_t n1, int R, int aligned, int64_t (&by)[5]) {
  PXA_CHECK_ARG(stack >= 1 && n0 >= 1 && n1 >= 1 && n0 <= 0x7fffffff && n1 <= 0x7fffffff);
  PXA_CHECK_ARG(R >= 1 && R <= kMaxR);
  // 4-element vectors, the column halo of Layout<float, R>
  constexpr int V = kVecN<float>;
  const bool vec_ok = aligned != 0 && n1 % V == 0;
  for (int64_t& c : by) c = 0;
  for (int64_t ty0 = 0; ty0 < n0; ty0 += TY)
    for (int64_t tx0 = 0; tx0 < n1; tx0 += TX) by[tile_class((int)n0, (int)n1, (int)ty0, (int)tx0, R, rup(2 * R, V), vec_ok)] += stack;
  return PXA_OK;
}

int pxa_pgd_tv2d_tile_classes(int64_t stack, int64_t n0, int64_t n1, int R, int aligned, int64_t* counts) {
  PXA_CHECK_ARG(counts != nullptr);
  int64_t by[5];
  if (const int e = pgd_tile_census(stack, n0, n1, R, aligned, by)) return e;
  counts[0] = by[kTileInterior];
  counts[1] = by[kTileCol];
  counts[2] = by[kTileRow];
  counts[3] = by[kTileGeneric] + by[kTileCorner];  // four counts: corners under generic
  return PXA_OK;
}

int pxa_pgd_tv2d_tile_census(int64_t stack, int64_t n0, int64_t n1, int R, int aligned, int64_t* counts) {
  PXA_CHECK_ARG(counts != nullptr);
  int64_t by[5];
  if (const int e = pgd_tile_census(stack, n0, n1, R, aligned, by)) return e;
  counts[0] = by[kTileInterior];
  counts[1] = by[kTileCol];
  counts[2] = by[kTileRow];
  counts[3] = by[kTileCorner];
  counts[4] = by[kTileGeneric];
  return PXA_OK;
}

int pxa_pgd_tv2d_plan(int dtype, int64_t stack, int64_t y_images, int64_t n0, int64_t n1, int nt0, const int32_t* off0,
                      const double* coef0, int nt1, const int32_t* off1, const double* coef1, double h0, double h1,
                      double lam, double mu, int prox, void** plan) {
  PXA_CHECK_ARG(plan != nullptr);
  *plan = nullptr;
  PgdPlan* pl = new PgdPlan();
  pl->dtype = dtype;
  int e = PXA_ERR_DTYPE;
  auto prepare = [&](auto& p) {
    e = pgd_params(stack, y_images, n0, n1, nt0, off0, coef0, nt1, off1, coef1, h0, h1, lam, mu, prox, p, pl->R);
    pl->fold_rows = p.fold_rows;
    pl->fold_per_row = p.fold_per_row;
  };
  if (dtype == PXA_F32)
    prepare(pl->pf);
  else if (dtype == PXA_F64)
    prepare(pl->pd);
  if (e == PXA_OK) {  // HIP failures: the positive hipError_t (the header's convention: HIP codes > 0, PXA_ERR_* < 0)
    hipError_t he = hipMalloc((void**)&pl->counter, sizeof(unsigned));
    if (he != hipSuccess) pl->counter = nullptr;
    else he = hipMemset(pl->counter, 0, sizeof(unsigned));
    if (he != hipSuccess) e = (int)he > 0 ? (int)he : PXA_ERR_UNSUPPORTED;
  }
  if (e != PXA_OK) {
    if (pl->counter) (void)hipFree(pl->counter);
    delete pl;
    return e;
  }
  *plan = pl;
  return PXA_OK;
}

int pxa_pgd_tv2d_plan_step(void* plan, double a, double tau, double prox_w, const void* x, const void* x_prev,
                           const void* hty, void* x_new, double* partials, const void* x_ref, double* rel_values,
                           uint32_t* rel_flags, uint32_t seq, void* stream) {
  PXA_CHECK_ARG(plan != nullptr);
  const PgdPlan* pl = (const PgdPlan*)plan;
  return plan_run(pl, a, tau, prox_w, x, x_prev, hty, x_new, partials, x_ref, rel_values, rel_flags, seq, pl->counter,
                  as_stream(stream));
}

int pxa_pgd_tv2d_plan_step_fold(void* plan, double a, double tau, double prox_w, const void* x, const void* x_prev,
                                const void* hty, void* x_new, double* partials, const void* x_ref, double* rel_values,
                                uint32_t* rel_flags, uint32_t seq, void* stream) {
  PXA_CHECK_ARG(plan != nullptr && partials != nullptr && rel_values != nullptr && rel_flags != nullptr);
  const PgdPlan* pl = (const PgdPlan*)plan;
  if (const int e = plan_run(pl, a, tau, prox_w, x, x_prev, hty, x_new, partials, x_ref, nullptr, nullptr, 0,
                             pl->counter, as_stream(stream)))
    return e;
  return pxa_tile_partials_fold(pl->fold_rows, pl->fold_per_row, partials, rel_values, rel_flags, seq, stream);
}

int pxa_pgd_tv2d_plan_step_wfold(void* plan, double a, double tau, double prox_w, const void* x, const void* x_prev,
                                 const void* hty, void* x_new, double* partials, double* rel_values, uint32_t* rel_flags,
                                 uint32_t seq, void* stream) {
  PXA_CHECK_ARG(plan != nullptr && partials != nullptr && rel_values != nullptr && rel_flags != nullptr);
  const PgdPlan* pl = (const PgdPlan*)plan;
  if (const int e = plan_run(pl, a, tau, prox_w, x, x_prev, hty, x_new, partials, nullptr, nullptr, nullptr, 0,
                             pl->counter, as_stream(stream), 1))
    return e;
  return pxa_tile_partials_fold(pl->fold_rows, pl->fold_per_row, partials, rel_values, rel_flags, seq, stream);
}

int pxa_pgd_tv2d_plan_step_wpub(void* plan, double a, double tau, double prox_w, const void* x, const void* x_prev,
                                const void* hty, void* x_new, double* partials, const double* prev_partials,
                                double* rel_values, uint32_t* rel_flags, uint32_t seq, void* stream) {
  PXA_CHECK_ARG(plan != nullptr && partials != nullptr);
  PXA_CHECK_ARG(prev_partials == nullptr || (rel_values != nullptr && rel_flags != nullptr));
  const PgdPlan* pl = (const PgdPlan*)plan;
  return plan_run(pl, a, tau, prox_w, x, x_prev, hty, x_new, partials, nullptr, nullptr, nullptr, 0, pl->counter,
                  as_stream(stream), 1, prev_partials, rel_values, rel_flags, seq);
}

int pxa_pgd_tv2d_plan_free(void* plan) {
  if (plan == nullptr) return PXA_OK;
  PgdPlan* pl = (PgdPlan*)plan;
  if (pl->counter) (void)hipFree(pl->counter);
  delete pl;
  return PXA_OK;
}

int pxa_pgd_tv2d_step(int dtype, int64_t stack, int64_t y_images, int64_t n0, int64_t n1, int nt0, const int32_t* off0,
                      const double* coef0, int nt1, const int32_t* off1, const double* coef1, double h0, double h1,
                      double lam, double mu, double a, double tau, int prox, double prox_w, const void* x,
                      const void* x_prev, const void* hty, void* x_new, double* partials, const void* x_ref,
                      void* stream) {
  PXA_DISPATCH(dtype, T,
               return pgd_entry<T>(stack, y_images, n0, n1, nt0, off0, coef0, nt1, off1, coef1, h0, h1, lam, mu, a,
                                   tau, prox, prox_w, x, x_prev, hty, x_new, partials, x_ref, as_stream(stream)));
}

}  // extern "C"
