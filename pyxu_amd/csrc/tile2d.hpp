// Shared machinery of the LDS-tiled 2-D separable-stencil kernels (pgd_tv2d.hip, pds3d.hip):
// tile geometry, LDS layout, register-blocked Toeplitz sweeps and the exact zero-boundary
// corrections of G = H^T H (see the derivation at the top of pgd_tv2d.hip).
#pragma once
#include "common.hpp"

namespace pxa {
namespace tile2d {

constexpr int TY = 32;
constexpr int TX = 64;
constexpr int kThreads = 256;
constexpr int kMaxR = 8;
constexpr int kMaxG = 4 * kMaxR + 1;
constexpr int kKT = 2 * kMaxR + 2;  // per-axis stride of the LDS tap copy (edge tiles)

__host__ __device__ constexpr int cdiv(int a, int b) { return (a + b - 1) / b; }
__host__ __device__ constexpr int rup(int a, int b) { return cdiv(a, b) * b; }

template <typename T, int R>
struct Layout {
  static constexpr int V = kVecN<T>;  // elements per 16-B vector (4 fp32, 2 fp64)
  static constexpr bool F32 = sizeof(T) == 4;
  static constexpr int CA = rup(2 * R, V);  // A column halo (vector aligned)
  static constexpr int AR = TY + 4 * R;     // A rows
  static constexpr int AC = TX + 2 * CA;    // A columns = PT rows
  static constexpr int NGA = AC / V;        // phase 0: AR x NGA vectors
  static constexpr int NA = TY / V;         // row groups (pass A and pass B)
  static constexpr int NB = AC / V;         // pass A column groups
  static constexpr int CW = F32 ? 2 : 1;    // pass B: output columns per item
  static constexpr int NCB = TX / CW;       // pass B column items
  static constexpr int pad_to(int w, int m, int res) {
    int p = w;
    while (F32 && (p % m) != res) p += V;
    return p;
  }
  static constexpr int AP = pad_to(AC, 32, 28);   // A pitch (elements)
  static constexpr int PTP = F32 ? TY + 8 : TY;  // PT pitch (elements): conflict-free with pass_b_item
  // pass B item of linear index `it`: row group a, column item cb.  fp32: each 32-lane half of a wave
  // takes 4 row groups x 8 column items, so that both the G1 sweep (ds_read_b128 of PT) and the yk
  // window reads of the TV stencil (ds_read_b64 of A, row groups 4 apart collide mod 64 banks) are
  // conflict-free under the MI355X_MICROARCH.md bank model (scripts/ldsbank.py)
  __device__ static inline void pass_b_item(int it, int& a, int& cb) {
    if constexpr (F32 && NA == 8) {
      a = (it & 3) + 4 * ((it >> 5) & 1);
      cb = ((it >> 2) & 7) + 8 * (it >> 6);
    } else {
      a = it % NA;
      cb = it / NA;
    }
  }
  static constexpr int N0 = AR * NGA, NPA = NA * NB, NPB = NA * NCB;
  static constexpr size_t BYTES = (size_t)(AR * AP + AC * PTP + 2 * kKT) * sizeof(T);
};

template <typename T, int V>
__device__ inline void ld_vec(const T* p, T (&v)[V]) {
  using VT = typename Vec4<T>::type;
  *reinterpret_cast<VT*>(v) = *reinterpret_cast<const VT*>(p);
}
template <typename T, int V>
__device__ inline void st_vec(T* p, const T (&v)[V]) {
  using VT = typename Vec4<T>::type;
  *reinterpret_cast<VT*>(p) = *reinterpret_cast<const VT*>(v);
}

template <typename T>
__device__ inline T apply_prox(int prox, T z, T pw) {
  if (prox == 1) return fmax(z, T(0));  // PositiveOrthant: clip(0, None)
  if (prox == 2) {                       // L1: sign(z) * max(|z| - pw, 0)
    T m = (z < T(0) ? -z : z) - pw;
    m = m > T(0) ? m : T(0);
    return z < T(0) ? -m : m;
  }
  return z;
}

// Packed-arithmetic unit: fp32 pairs (v_pk_fma_f32), fp64 scalars.
template <typename T>
struct Pk {
  using type = T;
  static constexpr int W = 1;
  __device__ static type splat(T v) { return v; }
};
template <>
struct Pk<float> {
  typedef float type __attribute__((ext_vector_type(2)));
  static constexpr int W = 2;
  __device__ static type splat(float v) { return type{v, v}; }
};

// Register-blocked sweep along the leading axis of a [m][pitch PS] source: for NO outputs along the
// sweep and one V-vector across it, out[o][v] = sum_{t=0}^{4R} g[t] src[(o + t) * PS + v].
// D = 0: the compiler schedules the NO + 4R row loads (it hoists most of them: ~4 VGPRs per row live at once).
// D > 0: at most D rows in flight -- row j + D is loaded when row j is consumed, and a scheduling barrier (only
// VALU / SALU may cross it) keeps the LDS reads in that order -- so a sweep holds ~4 (D + 1) row registers (A/B
// builds of the PGD tile kernel: PXA_PGD_SWEEP_DEPTH).  Same FMAs in the same order: same bits.
template <typename T, int R, int NO, int PS, int D = 0>
__device__ inline void sweep(const T* __restrict__ src, const T* __restrict__ g, T (&out)[NO][kVecN<T>]) {
  constexpr int V = kVecN<T>;
  using P = typename Pk<T>::type;
  constexpr int NP = V / Pk<T>::W;
  using VT = typename Vec4<T>::type;
  constexpr int NJ = NO + 4 * R;
  P acc[NO][NP];
#pragma unroll
  for (int o = 0; o < NO; ++o)
#pragma unroll
    for (int h = 0; h < NP; ++h) acc[o][h] = Pk<T>::splat(T(0));
  if constexpr (D > 0) {
    VT ring[D];
#pragma unroll
    for (int j = 0; j < D && j < NJ; ++j) ring[j] = *reinterpret_cast<const VT*>(src + j * PS);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const VT t = ring[j % D];
      if (j + D < NJ) ring[j % D] = *reinterpret_cast<const VT*>(src + (j + D) * PS);
      P row[NP];
      __builtin_memcpy(&row[0], &t, sizeof(VT));
#pragma unroll
      for (int o = 0; o < NO; ++o) {
        const int k = j - o;
        if (k >= 0 && k <= 4 * R) {
          const P gg = Pk<T>::splat(g[k]);
#pragma unroll
          for (int h = 0; h < NP; ++h) acc[o][h] = gg * row[h] + acc[o][h];
        }
      }
      __builtin_amdgcn_sched_barrier(0x6);  // VALU and SALU may move across, LDS reads may not
    }
#pragma unroll
    for (int o = 0; o < NO; ++o) __builtin_memcpy(&out[o][0], &acc[o][0], sizeof(T) * V);
    return;
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const VT t = *reinterpret_cast<const VT*>(src + j * PS);
    P row[NP];
    __builtin_memcpy(&row[0], &t, sizeof(VT));
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      const int k = j - o;
      if (k >= 0 && k <= 4 * R) {
        const P gg = Pk<T>::splat(g[k]);
#pragma unroll
        for (int h = 0; h < NP; ++h) acc[o][h] = gg * row[h] + acc[o][h];
      }
    }
  }
#pragma unroll
  for (int o = 0; o < NO; ++o) __builtin_memcpy(&out[o][0], &acc[o][0], sizeof(T) * V);
}

// Boundary rows of G along one axis, as a correction of the Toeplitz sweep.  The sweep evaluates
// sum_p k[i-p] (H y)[p] over ALL p, i.e. including the R "ghost" positions p outside [0, n) where the
// zero-padded H y is still non-zero; the exact G = H^T H only sums p inside [0, n), so
//   (G y)[i] = sweep[i] - sum_{ghost p, |i - p| <= R} k[i - p] (H y)[p].
// acc[o][v]: NO outputs along the sweep axis at positions i0 + o, one V-vector across it;
// the V-vector of position q along the sweep axis is at src + (q - q0) * PS (zero outside [0, n));
// k: the taps (compile-time indices), kt: the same taps in LDS (runtime indices).
template <typename T, int R, int NO, int PS>
__device__ inline void ghost_fix(int i0, int n, int q0, const T* __restrict__ src, const T* __restrict__ k,
                                 const T* __restrict__ kt, T (&acc)[NO][kVecN<T>]) {
  constexpr int V = kVecN<T>;
  using VT = typename Vec4<T>::type;
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const int pg = side == 0 ? -R : n;  // first ghost position on this side
    const bool hit = side == 0 ? (i0 < R) : (i0 + NO - 1 >= n - R && i0 < n);
    if (!hit) continue;
    T gh[R][V];  // (H y)[pg + m] across the vector
#pragma unroll
    for (int m = 0; m < R; ++m) {
      const int pp = pg + m;
#pragma unroll
      for (int v = 0; v < V; ++v) gh[m][v] = T(0);
      if (pp >= i0 - R && pp <= i0 + NO - 1 + R) {  // used by some output (keeps reads inside the window)
#pragma unroll
        for (int s = -R; s <= R; ++s) {
          T w[V];
          const VT t = *reinterpret_cast<const VT*>(src + (pp + s - q0) * PS);
          __builtin_memcpy(&w[0], &t, sizeof(VT));
#pragma unroll
          for (int v = 0; v < V; ++v) gh[m][v] = fma(k[s + R], w[v], gh[m][v]);
        }
      }
    }
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      const int i = i0 + o;
      if (i >= n || (side == 0 ? i >= R : i < n - R)) continue;
#pragma unroll
      for (int m = 0; m < R; ++m) {
        const int t = i - (pg + m);
        if (t < -R || t > R) continue;
        const T kk = kt[t + R];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[o][v] = fma(-kk, gh[m][v], acc[o][v]);
      }
    }
  }
}

// Boundary columns of the in-plane pass B (edge-column tiles), computed cooperatively into LDS:
// GH[side][m][r] = sum_s k[s] PT[ghost column pg + m + s][tile row r] for the R zero-padded ghost
// columns pg + m on each side (pg = -R, n) -- ghost_fix()'s gh with the same fma order.  With ghost_fix()
// the few lanes owning columns within R of the border compute them all, one 2R+1-tap sum per ghost
// column and lane: one wave then runs thousands of cycles past the others (measured by the PGD
// kernels' s_memtime trace).  Followed by a barrier, then ghost_fix_pre() in pass B.  PTP: the pitch of PT.
template <typename T, int R, int PTP = Layout<T, R>::PTP>
__device__ inline void ghost_cols_coop(const T* __restrict__ k, const T* PT, T* GH, int tx0, int n, int lt = threadIdx.x,
                                       int nthr = kThreads) {
  using L = Layout<T, R>;
  for (int t = lt; t < 2 * R * TY; t += nthr) {
    const int side = t / (R * TY), m = (t / TY) % R, r = t % TY;
    const int row = (side == 0 ? -R : n) + m - (tx0 - L::CA);  // PT row of the ghost column
    T g = T(0);
    if (row - R >= 0 && row + R < L::AC) {  // else no output of this tile uses it
#pragma unroll
      for (int q = -R; q <= R; ++q) g = fma(k[q + R], PT[(row + q) * PTP + r], g);
    }
    GH[(side * R + m) * TY + r] = g;
  }
}

// ghost_fix()'s correction step with precomputed ghost terms: outputs i0 .. i0 + NO - 1 along the sweep
// axis (n positions), one V-vector across it from position cc of the GH rows (pitch GP)
template <typename T, int R, int NO, int GP>
__device__ inline void ghost_fix_pre(int i0, int n, int cc, const T* __restrict__ GH, const T* __restrict__ kt,
                                     T (&acc)[NO][kVecN<T>]) {
  constexpr int V = kVecN<T>;
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const int pg = side == 0 ? -R : n;
    const bool hit = side == 0 ? (i0 < R) : (i0 + NO - 1 >= n - R && i0 < n);
    if (!hit) continue;
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      const int i = i0 + o;
      if (i >= n || (side == 0 ? i >= R : i < n - R)) continue;
#pragma unroll
      for (int m = 0; m < R; ++m) {
        const int t = i - (pg + m);
        if (t < -R || t > R) continue;
        const T kk = kt[t + R];
        T gh[V];
        const auto* src = GH + (side * R + m) * GP + cc;
#pragma unroll
        for (int v = 0; v < V; ++v) gh[v] = src[v];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[o][v] = fma(-kk, gh[v], acc[o][v]);
      }
    }
  }
}

// byte offset / size of the ghost-term region the tile kernels append to the Layout carve
template <typename T, int R>
constexpr size_t kGhOff = (Layout<T, R>::BYTES + 15) / 16 * 16;
template <typename T, int R>
constexpr size_t kGhBytes = (size_t)2 * R * TY * sizeof(T);

// Global V-vector load at an element offset whose alignment is known at compile time.
template <typename T>
__device__ inline void ld_pair(const T* __restrict__ p, T (&v)[2]) {
  if constexpr (sizeof(T) == 4) {
    const float2 t = *reinterpret_cast<const float2*>(p);
    v[0] = t.x;
    v[1] = t.y;
  } else {
    v[0] = p[0];
    v[1] = p[1];
  }
}

// Staged epilogue geometry: pass B parks its results in O (the PT region, free once all G sweeps are
// done), then the workgroup finishes the tile in row-major order, each 16-B vector of a tile row one
// lane (16 lanes per fp32 row): the global loads / stores of the epilogue are full 128-B lines instead
// of the pass-B item order's 64-B row pieces (measured on MI355X: a 2048^2 fp32 store in the item order
// 7.2 us, row-major 5.2 us).
template <typename T, int R>
struct Stage {
  using L = Layout<T, R>;
  static constexpr int V = L::V;
  static constexpr bool F32 = sizeof(T) == 4;
  // fp32: 64-dword rows with the 16-B chunks of row r XOR-swizzled by 2 (r / 4): the pass-B item-order
  // ds_write_b64 (rows 4a + u, column pairs of cb) hit 32 distinct banks per 16-lane group, and a
  // row-major ds_read_b128 group reads one whole row (64 contiguous dwords, permuted): both
  // conflict-free under the MI355X_MICROARCH.md §LDS bank model (scripts/ldsbank.py)
  static constexpr int OP = F32 ? TX : TX + 2;
  static constexpr int LPR = TX / V;          // lanes per tile row
  static constexpr int RPS = kThreads / LPR;  // rows per sweep
  static_assert(TY * OP <= L::AC * L::PTP, "O must fit in the PT region");
  __device__ static inline int idx(int r, int c) {
    if constexpr (F32) return r * OP + 4 * (((c >> 2) ^ (2 * (r >> 2))) & 15) + (c & 3);
    else return r * OP + c;
  }
  // row-major epilogue lane -> (tile row r0 of the first sweep, 16-B column vector cq).  fp32: each
  // ds_read_b128 lane group ({0-3,12-15,20-27}, {4-11,16-19,28-31}, +32) takes one row, so the reads
  // of O and of the yk window A are contiguous 64-dword runs whatever the pitch; global accesses of a
  // wave still cover 4 whole 256-B tile rows
  __device__ static inline void lane(int tid, int& r0, int& cq) {
    if constexpr (F32) {
      static_assert(TX == 64 && kThreads % 64 == 0, "fp32 lane map assumes 64-column tiles");
      const int ln = tid & 63, w = tid >> 6, h = ln >> 5, l = ln & 31;
      int g, pos;
      if (l < 4) g = 0, pos = l;
      else if (l < 12) g = 1, pos = l - 4;
      else if (l < 16) g = 0, pos = l - 8;
      else if (l < 20) g = 1, pos = l - 8;
      else if (l < 28) g = 0, pos = l - 12;
      else g = 1, pos = l - 16;
      r0 = 4 * w + 2 * h + g;
      cq = pos;
    } else {
      cq = tid % LPR;
      r0 = tid / LPR;
    }
  }
};

// Row-major pass-B blocks of the fp32 PGD tile kernel: an item is RB = 2 tile rows x CB = 4 columns, i.e. two 16-B row
// vectors of the tile, so the thread that sweeps G1 for them also loads H^T y, applies the prox and stores x_new from
// its registers (no O staging).  The G1 sweep runs along the item's 4-column side: 4 outputs share every PT row, read
// as one ds_read_b64 (the item's two tile rows).
//   PT pitch PTP = TY + 4 (4 PTP = 16 mod 64 dwords): a 32-lane ds_read_b64 group of 4 column items x 8 row pairs reads
//   dwords 16 ci + 2 rp + {0, 1} (+ const): 64 distinct banks; pass A's ds_write_b128 (8 lanes = 8 row groups of one PT
//   row) stay 32 contiguous dwords.
//   A wave is 8 column items x 8 row pairs = 16 tile rows x 32 columns: every global access of it covers whole 128-B
//   lines.  The row pair of a lane is permuted within its 8 so that each 16-lane ds_read_b128 group ({0-3, 12-15,
//   20-27}, ...) holds row pairs two apart: the yk reads of A (pitch AP = 28 mod 32, so 2 AP = -8 mod 64) are then four
//   disjoint 16-dword runs.  All conflict-free under the MI355X_MICROARCH.md §LDS bank model (scripts/ldsbank.py).
template <typename T, int R>
struct BlockB {
  using L = Layout<T, R>;
  static constexpr int RB = 2, CB = 4;
  static constexpr int PTP = TY + 4;
  static constexpr int WR = 16, WC = 32;      // tile rows x columns of one wave
  static constexpr int NRP = WR / RB, NCI = WC / CB;
  static_assert(sizeof(T) == 4 && TY == 2 * WR && TX == 2 * WC && kThreads == 256, "four waves, 2 x 2 over the tile");
  static_assert(PTP <= L::PTP, "PT keeps inside Layout's carve");
  // (wave, lane) -> row pair rpl and column item cil within the wave's region, and the region's first row / column
  __device__ static inline void item(int wv, int ln, int& rpl, int& cil, int& wr0, int& wc0) {
    const int l = ln & 31, k = l >> 2;
    rpl = k ^ (((k + 2) >> 2) & 1);  // 0 1 3 2 5 4 6 7
    cil = 4 * (ln >> 5) + (l & 3);
    wr0 = WR * (wv >> 1);
    wc0 = WC * (wv & 1);
  }
};

// sweep() with a W-element row vector (W a multiple of the packed width) and the ring in the caller's hands: start()
// issues the first D row reads, run() issues row j + D and then consumes row j, D rows in flight, the order fixed by
// scheduling barriers, so that the wait before the FMAs of a row counts the reads behind it (lgkmcnt(D)) instead of
// draining them.  `g`: the taps, already in registers (a scalar load among the reads would turn every counted wait into
// a drain).  Same FMAs in the same order per output as sweep(): same bits.
template <typename T, int R, int NO, int W, int PS, int D>
struct RowSweep {
  using P = typename Pk<T>::type;
  static constexpr int NP = W / Pk<T>::W;
  static constexpr int NJ = NO + 4 * R;
  static_assert(W % Pk<T>::W == 0 && D >= 1, "whole packed rows, a ring of at least one");
  typedef T Row __attribute__((ext_vector_type(W)));
  // (volatile: the compiler would pair the b64 reads of two PT rows into one ds_read2_b64, which the LDS serves at
  // half the rate of two ds_read_b64 -- MI355X_MICROARCH.md §LDS; the LDS address space is named because a volatile
  // access through a generic pointer stays a flat load)
  __device__ static inline Row ld(const T* p) {
    return *(const volatile __attribute__((address_space(3))) Row*)p;
  }
  Row ring[D];
  __device__ inline void start(const T* __restrict__ src) {
#pragma unroll
    for (int j = 0; j < D && j < NJ; ++j) ring[j] = ld(src + j * PS);
  }
  __device__ inline void run(const T* __restrict__ src, const T (&g)[4 * R + 1], T (&out)[NO][W]) {
    P acc[NO][NP];
#pragma unroll
    for (int o = 0; o < NO; ++o)
#pragma unroll
      for (int h = 0; h < NP; ++h) acc[o][h] = Pk<T>::splat(T(0));
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      P row[NP];
      __builtin_memcpy(&row[0], &ring[j % D], sizeof(Row));
      if (j + D < NJ) ring[j % D] = ld(src + (j + D) * PS);
      __builtin_amdgcn_sched_barrier(0);  // the read stays ahead of row j's FMAs ...
#pragma unroll
      for (int o = 0; o < NO; ++o) {
        const int k = j - o;
        if (k >= 0 && k <= 4 * R) {
          const P gg = Pk<T>::splat(g[k]);
#pragma unroll
          for (int h = 0; h < NP; ++h) acc[o][h] = gg * row[h] + acc[o][h];
        }
      }
      // ... and those ahead of the next read: row by row, NO independent chains.  (The empty statement takes the
      // accumulators through the ordered instruction chain: instruction selection would otherwise gather each
      // output's FMAs, which the scheduling barriers do not order, into one dependent run behind all reads.)
#pragma unroll
      for (int o = 0; o < NO; ++o)
#pragma unroll
        for (int h = 0; h < NP; ++h) asm volatile("" : "+v"(acc[o][h]));
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int o = 0; o < NO; ++o) __builtin_memcpy(&out[o][0], &acc[o][0], sizeof(T) * W);
  }
};

// sweep() with a W-element row vector, compiler-scheduled: every row read at once, then the FMAs.  The row reads are
// volatile LDS accesses: as plain loads the compiler pairs the b64 reads of two PT rows into one ds_read2_b64, which the
// LDS serves at half the rate of two ds_read_b64 (MI355X_MICROARCH.md §LDS; measured: 22.4-22.7 us per step paired
// against 21.4-21.7 single, profiles/pgd_blocks_ab.txt); the LDS address space is named because a volatile access through
// a generic pointer stays a flat load.  Same FMAs in the same order per output as sweep(): same bits.
template <typename T, int R, int NO, int W, int PS>
__device__ inline void sweep_w(const T* __restrict__ src, const T* __restrict__ g, T (&out)[NO][W]) {
  using P = typename Pk<T>::type;
  constexpr int NP = W / Pk<T>::W;
  constexpr int NJ = NO + 4 * R;
  typedef T Row __attribute__((ext_vector_type(W)));
  P acc[NO][NP];
#pragma unroll
  for (int o = 0; o < NO; ++o)
#pragma unroll
    for (int h = 0; h < NP; ++h) acc[o][h] = Pk<T>::splat(T(0));
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const Row t = *(const volatile __attribute__((address_space(3))) Row*)(src + j * PS);
    P row[NP];
    __builtin_memcpy(&row[0], &t, sizeof(Row));
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      const int k = j - o;
      if (k >= 0 && k <= 4 * R) {
        const P gg = Pk<T>::splat(g[k]);
#pragma unroll
        for (int h = 0; h < NP; ++h) acc[o][h] = gg * row[h] + acc[o][h];
      }
    }
  }
#pragma unroll
  for (int o = 0; o < NO; ++o) __builtin_memcpy(&out[o][0], &acc[o][0], sizeof(T) * W);
}

// ghost_fix_pre() for outputs that are W-vectors across the sweep axis
template <typename T, int R, int NO, int W, int GP>
__device__ inline void ghost_fix_pre_w(int i0, int n, int cc, const T* __restrict__ GH, const T* __restrict__ kt,
                                       T (&acc)[NO][W]) {
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const int pg = side == 0 ? -R : n;
    const bool hit = side == 0 ? (i0 < R) : (i0 + NO - 1 >= n - R && i0 < n);
    if (!hit) continue;
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      const int i = i0 + o;
      if (i >= n || (side == 0 ? i >= R : i < n - R)) continue;
#pragma unroll
      for (int m = 0; m < R; ++m) {
        const int t = i - (pg + m);
        if (t < -R || t > R) continue;
        const T kk = kt[t + R];
        const auto* src = GH + (side * R + m) * GP + cc;
#pragma unroll
        for (int v = 0; v < W; ++v) acc[o][v] = fma(-kk, src[v], acc[o][v]);
      }
    }
  }
}

// ---- tile classes of the PGD tile kernel.  A tile whose window touches the image border in exactly one way, on an
// aligned image, takes the interior code wherever its axis is interior:
//   interior  the whole A window (2R rows, CA columns around the tile) lies inside the image
//   col       the window's rows lie inside, the tile's own columns end exactly on one border (tx0 == 0 or tx0 + TX == n1)
//             and the other side's CA halo is inside
//   row       the mirror image: columns interior, ty0 == 0 or ty0 + TY == n0, the other side's 2R rows inside
//   corner    both at once: own rows end exactly on one horizontal border with the other side's 2R rows inside, own
//             columns end exactly on one vertical border with the other side's CA halo inside (all four orientations)
//   generic   everything else (ragged last tiles, a halo that only grazes the border, images one tile wide or
//             high, unaligned pointers or rows, images beyond the 32-bit lane offsets): bounds tests everywhere
// `CA`: Layout's column halo (rup(2R, V)); `vec_ok`: 16-B aligned pointers and rows.
// (kTileGeneric keeps its value: pxa_pgd_tv2d_tile_classes indexes its four counts by it.)
enum TileClass : int { kTileInterior = 0, kTileCol = 1, kTileRow = 2, kTileGeneric = 3, kTileCorner = 4 };
constexpr int kMaxInteriorN1 = 1 << 22;  // (64 rows x 2^22 columns x 8 B = 2^31: the 32-bit lane offsets of lane_ptr)
__host__ __device__ inline int tile_class(int n0, int n1, int ty0, int tx0, int R, int CA, bool vec_ok) {
  if (!vec_ok || (int64_t)n0 * n1 > 0x7fffffff || n1 > kMaxInteriorN1) return kTileGeneric;
  const bool up = ty0 - 2 * R >= 0, down = ty0 + TY + 2 * R <= n0;
  const bool left = tx0 - CA >= 0, right = tx0 + TX + CA <= n1;
  const bool row_end = (ty0 == 0 && down) || (ty0 + TY == n0 && up);
  const bool col_end = (tx0 == 0 && right) || (tx0 + TX == n1 && left);
  if (up && down && left && right) return kTileInterior;
  if (up && down && col_end) return kTileCol;
  if (left && right && row_end) return kTileRow;
  if (row_end && col_end) return kTileCorner;
  return kTileGeneric;
}

// ghost_cols_coop() for the one side a col tile has (side 0: the image's first columns, 1: its last): the same terms
// with the same fma order into the same GH rows.  Every ghost column lies inside the PT rows here (the tile's own
// columns end on the border, CA >= 2R).
template <typename T, int R, int PTP>
__device__ inline void ghost_cols_side(const T* __restrict__ k, const T* PT, T* GH, int side, int lt) {
  using L = Layout<T, R>;
  static_assert(L::CA >= 2 * R, "ghost columns and their taps inside the window");
  for (int t = lt; t < R * TY; t += kThreads) {
    const int m = t / TY, r = t % TY;
    const int row = (side == 0 ? L::CA - R : L::CA + TX) + m;  // PT row of the ghost column
    T g = T(0);
#pragma unroll
    for (int q = -R; q <= R; ++q) g = fma(k[q + R], PT[(row + q) * PTP + r], g);
    GH[(side * R + m) * TY + r] = g;
  }
}

// ghost_fix()'s correction step for NO outputs whose distance from the border is known at compile time, so that the
// tap indices are constants (`k`: the taps in scalar registers) and the ghost terms sit at fixed offsets: term m is the
// W-vector at gh + m * GP.  FAR = false: output o is position P0 + o of the axis (ghost positions -R + m, tap index
// i - (-R + m) + R); FAR = true: output o is P0 - o positions before the last one (ghost positions n + m).  Per output
// the same fma chain as ghost_fix(): m ascending, outputs beyond R of the border untouched.
template <typename T, int R, int NO, int W, int GP, bool FAR, int P0>
__device__ inline void ghost_sub(const T* __restrict__ k, const T* __restrict__ gh, T (&acc)[NO][W]) {
#pragma unroll
  for (int o = 0; o < NO; ++o) {
    const int d = FAR ? P0 - o : P0 + o;  // distance from the border position
    if (d < 0 || d >= R) continue;
#pragma unroll
    for (int m = 0; m < R; ++m) {
      const int t = FAR ? -(d + 1) - m : d + R - m;
      if (t < -R || t > R) continue;
      const T kk = k[t + R];
      T g[W];
#pragma unroll
      for (int v = 0; v < W; ++v) g[v] = gh[m * GP + v];
#pragma unroll
      for (int v = 0; v < W; ++v) acc[o][v] = fma(-kk, g[v], acc[o][v]);
    }
  }
}

// XCD-aware tile order (speed only): XCD group g = blockIdx % 8 owns a contiguous band of tiles.
__device__ inline unsigned xcd_tile(unsigned bid, unsigned nb) {
  const unsigned q8 = nb >> 3, r8 = nb & 7u, g8 = bid & 7u;
  return g8 * q8 + (g8 < r8 ? g8 : r8) + (bid >> 3);
}

// ------------------------------------------------------------------ host side: the taps of one axis
// Dense tap window in double (index t + kMaxR) from (offset, coefficient) lists, coefficients of one offset added in
// list order; returns the reach max |offset|, or -1 when it exceeds kMaxR (nothing is written then).
using TapWindow = double[2 * kMaxR + 1];
inline int tap_window(int nt, const int32_t* off, const double* coef, TapWindow& k) {
  for (double& v : k) v = 0.0;
  int R = 0;
  for (int q = 0; q < nt; ++q) R = abs(off[q]) > R ? abs(off[q]) : R;
  if (R > kMaxR) return -1;
  for (int q = 0; q < nt; ++q) k[off[q] + kMaxR] += coef[q];
  return R;
}

// The kernels' form of a window for radius R: w[t + R] = k[t], |t| <= R, zero beyond.
template <typename T, int N>
inline void tap_dense(const TapWindow& k, int R, T (&w)[N]) {
  for (T& v : w) v = T(0);
  for (int t = -R; t <= R; ++t) w[t + R] = (T)k[t + kMaxR];
}

// Interior taps of G = H^T H for radius R: g[d + 2 R] = sum_t k[t] k[t + d], |d| <= 2 R, zero beyond.  Summed in
// double over t ascending (terms outside [-R, R] skipped), then one cast: both fused steps derive G from here.
template <typename T>
inline void tap_autocorr(const TapWindow& k, int R, T (&g)[kMaxG]) {
  for (T& v : g) v = T(0);
  for (int d = -2 * R; d <= 2 * R; ++d) {
    double s = 0.0;
    for (int t = -R; t <= R; ++t) {
      if (t + d < -R || t + d > R) continue;
      s += k[t + kMaxR] * k[t + d + kMaxR];
    }
    g[d + 2 * R] = (T)s;
  }
}

}  // namespace tile2d
}  // namespace pxa
