// pyxu_amd — gridding NUFFT (what the reference delegates to FINUFFT for eps > 0,
// operator/linop/fft/nufft.py:1367-1400, 1660-1689): the three kernels around the FFT on the oversampled grid.
// Types 1 and 2 use them as they are; type 3 (spread the rescaled sources, then a type 2 of that grid to the rescaled
// targets) uses spread and interp with one complex factor per point (template parameter FAC, pxa_nufft_*_fac).
//
//   spread : grid[q, l]  = sum_j c[q, j] prod_d phi(2 (l_d - xi_jd) / w)     points -> fine grid (periodic)
//   interp : c[q, j]     = sum_l grid[q, l] prod_d phi(2 (l_d - xi_jd) / w)  fine grid -> points (its transpose)
//   deconv : modes <-> fine grid: scale by prod_d corr_d(k_d) and zero-embed, or extract and scale; mode k sits in
//            cell k mod nf, so no fftshift copy exists
// with phi(z) = exp(beta (sqrt(1 - z^2) - 1)) on |z| <= 1 and w cells of support per axis.
//
// Plan (built on the host, once per operator).  Per point and axis the first touched cell l0 = ceil(xi - w/2)
// (int32, may be negative or >= nf) and the offset xi - l0 in [w/2 - 1, w/2] in the working precision; both in the
// order of a stable sort by bin (`perm`: sorted position -> original index, `bin_start`: nbins + 1 offsets).  A bin
// is a tile of kTile<D> fine-grid cells, its id row-major over the per-axis bin counts, and a point belongs to the
// bin of floor(xi).
//
// Spread, owner-computes.  A workgroup owns one bin's cells for a chunk of stack rows, CPT cells per thread, the
// sums in registers.  A footprint reaches at most w/2 <= 8 cells past floor(xi) on either side; the workgroup lists,
// per axis, the bins that the cell interval [t0 - R, t1 - 1 + R] (R = w/2 + 1, taken modulo nf) meets, each bin
// once and in ascending order, and walks the points of those bins in ascending bin id, kBatch candidates at a time
// (one per thread: first cells, offsets and index, fetched one batch ahead within a bin).  A candidate survives if
// its footprint meets the tile on every axis (exact test, either side of the wrap); a survivor gathers its weights
// of the chunk's rows, and the survivors are compacted in order (ballot + prefix) into LDS, so that all global
// loads of a batch are in flight together.  Then, kSub survivors at a time, their D w kernel values are evaluated
// once, by the whole workgroup, into LDS, and every thread adds, for each of its cells and each staged point whose
// footprint holds the cell, the product into its own registers.  At the end it stores its cells with plain stores.
// (Letting a wave skip, by a scalar branch, the points whose footprint misses its cells along axis 0 was measured
// and lost: 3.50 -> 3.74 ms on 2^20 points into a 128^2 grid, 0.040 -> 0.045 ms on 2^16 into 512^2.)  Every cell of the fine grid has exactly one owner and
// is written exactly once (zeros included): no atomics, no partial slabs, no fold pass, no memset, and the same
// call gives the same bits.  nf >= 2 w, so a footprint wraps an axis at most once and never meets a cell twice.
//
// Interp.  One thread per point in sorted order (neighbouring threads read neighbouring cells).  The D w kernel
// values are computed once per point into the thread's own LDS column ([d][i][thread]: conflict-free) and reused by
// the rows of the chunk; the w^D terms are added in the fixed order of the nested loops; the result goes back
// through `perm`.
#include "common.hpp"

namespace pxa {
namespace {

constexpr int kGridQChunk = 4;       // stack rows per workgroup
constexpr int kBatch = kBlock;       // candidate points per batch (one per thread)
template <typename T>
constexpr int kSub = sizeof(T) == 4 ? 64 : 32;  // surviving points whose kernel values are staged per pass
constexpr int kWMax = 16;            // widest kernel
constexpr int kNbrMax = 8;           // neighbour bins per axis: <= ceil((E + 2 R) / E) + 2 <= 6 at E >= 8, R <= 9
constexpr int kInterpBlock = 128;    // points per workgroup of the gather
constexpr int64_t kNfMax = (int64_t)1 << 30;

template <int D>
struct Tile;
template <>
struct Tile<1> {
  static constexpr int e0 = 256, e1 = 1, e2 = 1;
};
template <>
struct Tile<2> {
  static constexpr int e0 = 16, e1 = 16, e2 = 1;
};
template <>
struct Tile<3> {
  static constexpr int e0 = 8, e1 = 8, e2 = 8;
};

// axes in slots 0 .. D - 1, the other slots of length 1 (cell = (c0 nf1 + c1) nf2 + c2)
struct Geom {
  int64_t nf[3];
  int64_t nb[3];  // bins per axis
  int64_t n[3];   // modes per axis (deconv)
};

__device__ inline float exp_t(float x) { return expf(x); }
__device__ inline double exp_t(double x) { return exp(x); }
__device__ inline float sqrt_t(float x) { return sqrtf(x); }
__device__ inline double sqrt_t(double x) { return sqrt(x); }
template <typename T>
__device__ inline T fma_g(T a, T b, T c) {
  return __builtin_fma(a, b, c);
}
template <>
__device__ inline float fma_g<float>(float a, float b, float c) {
  return __builtin_fmaf(a, b, c);
}

// (a + i b) (c + i d), each part one product and one fused multiply-add, spelled out so that every instantiation
// rounds alike
template <typename T>
__device__ inline T cmul_re(T a, T b, T c, T d) {
  return fma_g<T>(a, c, -(b * d));
}
template <typename T>
__device__ inline T cmul_im(T a, T b, T c, T d) {
  return fma_g<T>(a, d, b * c);
}

// phi(2 x / w), x = l - xi
template <typename T>
__device__ inline T es_phi(T x, T two_over_w, T beta) {
  const T z = x * two_over_w;
  T s = (T)1 - z * z;
  s = s > (T)0 ? s : (T)0;
  return exp_t(beta * (sqrt_t(s) - (T)1));
}

// l0 folded into [0, nf), nf <= kNfMax = 2^30: 32-bit arithmetic throughout
__device__ inline int fold_cell(int32_t l0, int nf) {
  int v = l0 % nf;
  if (v < 0) v += nf;
  return v;
}

// FAC: every point's weights are multiplied by its complex factor fac[s] (sorted order; conjugated if conj_fac)
template <typename T, int D, int QC, bool FAC>
__global__ __launch_bounds__(kBlock) void spread_kernel(Geom g, int64_t Q, int64_t M, int w, T two_over_w, T beta,
                                                        const int32_t* __restrict__ l0, const T* __restrict__ off,
                                                        const int64_t* __restrict__ perm,
                                                        const int64_t* __restrict__ bin_start,
                                                        const T* __restrict__ c, T* __restrict__ grid,
                                                        const T* __restrict__ fac, int conj_fac) {
  using Tl = Tile<D>;
  constexpr int E[3] = {Tl::e0, Tl::e1, Tl::e2};
  constexpr int CPT = Tl::e0 * Tl::e1 * Tl::e2 / kBlock;
  static_assert(Tl::e0 * Tl::e1 * Tl::e2 % kBlock == 0, "whole cells per thread");
  __shared__ int64_t s_nbr[3][kNbrMax];
  __shared__ int s_nbrn[3];
  __shared__ int s_wcnt[kBlock / kWave];
  // the survivors of a batch, in order: folded first cell, offset, the chunk's weights
  __shared__ int s_c0[kBatch][D];
  __shared__ T s_off[kBatch][D];
  __shared__ T s_cw[kBatch][QC][2];
  constexpr int SUB = kSub<T>;
  __shared__ T s_ker[SUB][D][kWMax];

  const int t = threadIdx.x;
  const int64_t bin = blockIdx.x, q0 = (int64_t)blockIdx.y * QC;
  const int64_t bc[3] = {bin / (g.nb[1] * g.nb[2]), (bin / g.nb[2]) % g.nb[1], bin % g.nb[2]};
  int t0[3], t1[3], nf[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    nf[d] = (int)g.nf[d];
    t0[d] = (int)(bc[d] * E[d]);
    t1[d] = t0[d] + E[d] < nf[d] ? t0[d] + E[d] : nf[d];
  }

  // the bins whose points can reach this tile, per axis: each once, ascending
  if (t == 0) {
    for (int d = 0; d < 3; ++d) {
      int n = 0;
      if (d >= D) {
        s_nbr[d][n++] = 0;
      } else {
        const int R = w / 2 + 1;
        const int64_t lo = (int64_t)t0[d] - R;
        int64_t hi = (int64_t)t1[d] - 1 + R;
        if (hi - lo + 1 >= nf[d]) hi = lo + nf[d] - 1;
        for (int64_t cc = lo; cc <= hi;) {
          const int64_t cm = cc < 0 ? cc + nf[d] : (cc >= nf[d] ? cc - nf[d] : cc);
          const int64_t b = cm / E[d];
          const int64_t end = (b + 1) * E[d] < nf[d] ? (b + 1) * E[d] : nf[d];
          int pos = 0;
          while (pos < n && s_nbr[d][pos] < b) ++pos;
          if ((pos == n || s_nbr[d][pos] != b) && n < kNbrMax) {
            for (int k = n; k > pos; --k) s_nbr[d][k] = s_nbr[d][k - 1];
            s_nbr[d][pos] = b;
            ++n;
          }
          cc += end - cm;
        }
      }
      s_nbrn[d] = n;
    }
  }

  int cell[CPT][3];
  bool valid[CPT];
  T acc[CPT][QC][2];
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    const int r = t + k * kBlock;
    const int rc[3] = {r / (E[1] * E[2]), (r / E[2]) % E[1], r % E[2]};
    valid[k] = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      cell[k][d] = t0[d] + rc[d];
      valid[k] = valid[k] && cell[k][d] < t1[d];
    }
#pragma unroll
    for (int q = 0; q < QC; ++q) acc[k][q][0] = acc[k][q][1] = (T)0;
  }
  __syncthreads();

  const int lane = t & (kWave - 1), wave = t / kWave;
  for (int a0 = 0; a0 < s_nbrn[0]; ++a0)
    for (int a1 = 0; a1 < s_nbrn[1]; ++a1)
      for (int a2 = 0; a2 < s_nbrn[2]; ++a2) {
        const int64_t nbin = (s_nbr[0][a0] * g.nb[1] + s_nbr[1][a1]) * g.nb[2] + s_nbr[2][a2];
        int64_t lo = bin_start[nbin], hi = bin_start[nbin + 1];
        lo = lo < 0 ? 0 : (lo > M ? M : lo);
        hi = hi < lo ? lo : (hi > M ? M : hi);
        // this thread's candidate of the batch at s0: first cells, offsets, index into `c` (fetched a batch ahead)
        int cl[D];
        T co[D];
        int64_t cp = 0;
        T cf[2] = {(T)1, (T)0};
        auto fetch = [&](int64_t s, int (&fl)[D], T (&fo)[D], int64_t& fp, T (&ff)[2]) {
          const bool in = s < hi;
          if constexpr (FAC) {
            ff[0] = in ? fac[s * 2] : (T)1;
            ff[1] = in ? fac[s * 2 + 1] : (T)0;
            if (conj_fac) ff[1] = -ff[1];
          }
#pragma unroll
          for (int d = 0; d < D; ++d) {
            fl[d] = in ? fold_cell(l0[s * D + d], nf[d]) : 0;
            fo[d] = in ? off[s * D + d] : (T)0;
          }
          fp = in ? perm[s] : 0;
        };
        fetch(lo + t, cl, co, cp, cf);
        for (int64_t s0 = lo; s0 < hi; s0 += kBatch) {
          // which candidates' footprints meet the tile
          bool meets = s0 + t < hi;
#pragma unroll
          for (int d = 0; d < D; ++d) {
            const int last = cl[d] + w - 1;
            meets = meets && ((cl[d] < t1[d] && last >= t0[d]) || (last >= nf[d] && last - nf[d] >= t0[d]));
          }
          T cw[QC][2];
#pragma unroll
          for (int q = 0; q < QC; ++q) {
            const bool ok = meets && q0 + q < Q && (uint64_t)cp < (uint64_t)M;
            cw[q][0] = ok ? c[((q0 + q) * M + cp) * 2] : (T)0;
            cw[q][1] = ok ? c[((q0 + q) * M + cp) * 2 + 1] : (T)0;
            if constexpr (FAC) {
              const T re = cmul_re<T>(cw[q][0], cw[q][1], cf[0], cf[1]);
              cw[q][1] = cmul_im<T>(cw[q][0], cw[q][1], cf[0], cf[1]);
              cw[q][0] = re;
            }
          }
          int ncl[D];
          T nco[D];
          int64_t ncp;
          T ncf[2] = {(T)1, (T)0};
          fetch(s0 + kBatch + t, ncl, nco, ncp, ncf);

          const unsigned long long bal = __ballot(meets);
          if (lane == 0) s_wcnt[wave] = __popcll(bal);
          __syncthreads();
          int base = 0, n_s = 0;
#pragma unroll
          for (int k = 0; k < kBlock / kWave; ++k) {
            if (k < wave) base += s_wcnt[k];
            n_s += s_wcnt[k];
          }
          if (meets) {
            const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
#pragma unroll
            for (int d = 0; d < D; ++d) {
              s_c0[pos][d] = cl[d];
              s_off[pos][d] = co[d];
            }
#pragma unroll
            for (int q = 0; q < QC; ++q) {
              s_cw[pos][q][0] = cw[q][0];
              s_cw[pos][q][1] = cw[q][1];
            }
          }
          __syncthreads();

          for (int p0 = 0; p0 < n_s; p0 += SUB) {
            const int np = n_s - p0 < SUB ? n_s - p0 : SUB;
            for (int idx = t; idx < np * D * w; idx += kBlock) {
              const int p = idx / (D * w), r = idx % (D * w);
              const int d = r / w, i = r % w;
              s_ker[p][d][i] = es_phi<T>((T)i - s_off[p0 + p][d], two_over_w, beta);
            }
            __syncthreads();
            for (int p = 0; p < np; ++p) {
              int pc[D];
#pragma unroll
              for (int d = 0; d < D; ++d) pc[d] = s_c0[p0 + p][d];
#pragma unroll
              for (int k = 0; k < CPT; ++k) {
                int i[D];
                bool hit = valid[k];
#pragma unroll
                for (int d = 0; d < D; ++d) {
                  i[d] = cell[k][d] - pc[d];
                  if (i[d] < 0) i[d] += nf[d];
                  hit = hit && i[d] < w;
                }
                if (hit) {
                  T kv = s_ker[p][0][i[0]];
#pragma unroll
                  for (int d = 1; d < D; ++d) kv *= s_ker[p][d][i[d]];
#pragma unroll
                  for (int q = 0; q < QC; ++q) {
                    acc[k][q][0] = fma_g<T>(kv, s_cw[p0 + p][q][0], acc[k][q][0]);
                    acc[k][q][1] = fma_g<T>(kv, s_cw[p0 + p][q][1], acc[k][q][1]);
                  }
                }
              }
            }
            __syncthreads();
          }
#pragma unroll
          for (int d = 0; d < D; ++d) {
            cl[d] = ncl[d];
            co[d] = nco[d];
          }
          cp = ncp;
          if constexpr (FAC) {
            cf[0] = ncf[0];
            cf[1] = ncf[1];
          }
        }
      }

  const int64_t nft = g.nf[0] * g.nf[1] * g.nf[2];
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    if (!valid[k]) continue;
    const int64_t lin = ((int64_t)cell[k][0] * g.nf[1] + cell[k][1]) * g.nf[2] + cell[k][2];
#pragma unroll
    for (int q = 0; q < QC; ++q) {
      if (q0 + q >= Q) break;
      T* o = grid + ((q0 + q) * nft + lin) * 2;
      o[0] = acc[k][q][0];
      o[1] = acc[k][q][1];
    }
  }
}

// FAC: every point's finished sum is multiplied by its complex factor fac[s] (sorted order; conjugated if conj_fac)
template <typename T, int D, int QC, bool FAC>
__global__ __launch_bounds__(kInterpBlock) void interp_kernel(Geom g, int64_t Q, int64_t M, int w, T two_over_w,
                                                              T beta, const int32_t* __restrict__ l0,
                                                              const T* __restrict__ off,
                                                              const int64_t* __restrict__ perm,
                                                              const T* __restrict__ grid, T* __restrict__ out,
                                                              const T* __restrict__ fac, int conj_fac) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  T* s_ker = (T*)s_raw;  // [d][i][thread]
  const int t = threadIdx.x;
  const int64_t s = (int64_t)blockIdx.x * kInterpBlock + t, q0 = (int64_t)blockIdx.y * QC;
  if (s >= M) return;
  const int64_t pm = perm[s];
  if ((uint64_t)pm >= (uint64_t)M) return;
  T f[2] = {(T)1, (T)0};
  if constexpr (FAC) {
    f[0] = fac[s * 2];
    f[1] = conj_fac ? -fac[s * 2 + 1] : fac[s * 2 + 1];
  }
  int c0[3] = {0, 0, 0};
#pragma unroll
  for (int d = 0; d < D; ++d) {
    c0[d] = fold_cell(l0[s * D + d], (int)g.nf[d]);
    const T o = off[s * D + d];
    for (int i = 0; i < w; ++i) s_ker[(d * w + i) * kInterpBlock + t] = es_phi<T>((T)i - o, two_over_w, beta);
  }
  const int w1 = D > 1 ? w : 1, w2 = D > 2 ? w : 1;
  const int nf0 = (int)g.nf[0], nf1 = (int)g.nf[1], nf2 = (int)g.nf[2];
  const int64_t nft = g.nf[0] * g.nf[1] * g.nf[2];
  T acc[QC][2];
#pragma unroll
  for (int q = 0; q < QC; ++q) acc[q][0] = acc[q][1] = (T)0;
  for (int i0 = 0; i0 < w; ++i0) {
    int a0 = c0[0] + i0;
    if (a0 >= nf0) a0 -= nf0;
    const T k0 = s_ker[i0 * kInterpBlock + t];
    for (int i1 = 0; i1 < w1; ++i1) {
      int a1 = c0[1] + i1;
      if (a1 >= nf1) a1 -= nf1;
      const T k01 = D > 1 ? k0 * s_ker[(w + i1) * kInterpBlock + t] : k0;
      for (int i2 = 0; i2 < w2; ++i2) {
        int a2 = c0[2] + i2;
        if (a2 >= nf2) a2 -= nf2;
        const T kv = D > 2 ? k01 * s_ker[(2 * w + i2) * kInterpBlock + t] : k01;
        const int64_t lin = ((int64_t)a0 * nf1 + a1) * nf2 + a2;
#pragma unroll
        for (int q = 0; q < QC; ++q) {
          if (q0 + q < Q) {
            const T* gp = grid + ((q0 + q) * nft + lin) * 2;
            acc[q][0] = fma_g<T>(kv, gp[0], acc[q][0]);
            acc[q][1] = fma_g<T>(kv, gp[1], acc[q][1]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < QC; ++q) {
    if (q0 + q >= Q) break;
    T* o = out + ((q0 + q) * M + pm) * 2;
    if constexpr (FAC) {
      o[0] = cmul_re<T>(acc[q][0], acc[q][1], f[0], f[1]);
      o[1] = cmul_im<T>(acc[q][0], acc[q][1], f[0], f[1]);
    } else {
      o[0] = acc[q][0];
      o[1] = acc[q][1];
    }
  }
}

// mode k of an axis with n modes and nf cells: cell k mod nf; array index k + n/2 (modeord 0) or k mod n (modeord 1);
// the correction vector is indexed k + n/2 in both orders
template <typename T>
__global__ __launch_bounds__(kBlock) void deconv_kernel(Geom g, int D, int64_t Q, int modeord, int to_grid,
                                                        const T* __restrict__ corr, const T* __restrict__ in,
                                                        T* __restrict__ out) {
  const int64_t nft = g.nf[0] * g.nf[1] * g.nf[2], nt = g.n[0] * g.n[1] * g.n[2];
  const int64_t coff[3] = {0, g.n[0], g.n[0] + g.n[1]};
  const int64_t total = Q * (to_grid ? nft : nt);
  for (int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kBlock) {
    const int64_t per = to_grid ? nft : nt;
    const int64_t q = idx / per, e = idx % per;
    const int64_t* dim = to_grid ? g.nf : g.n;
    const int64_t ec[3] = {e / (dim[1] * dim[2]), (e / dim[2]) % dim[1], e % dim[2]};
    int64_t other = 0;
    T scale = (T)1;
    bool inside = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const int64_t n = g.n[d], nf = g.nf[d], h = n / 2, p = (n - 1) / 2;
      int64_t k;
      if (to_grid) {
        const int64_t f = ec[d];
        if (f <= p)
          k = f;
        else if (f >= nf - h)
          k = f - nf;
        else {
          k = 0;
          inside = false;
        }
        other = other * n + (modeord ? (k >= 0 ? k : k + n) : k + h);
      } else {
        const int64_t a = ec[d];
        k = modeord ? (a <= p ? a : a - n) : a - h;
        other = other * nf + (k < 0 ? k + nf : k);
      }
      if (d < D) scale *= corr[coff[d] + k + h];
    }
    T re = (T)0, im = (T)0;
    if (inside) {
      const T* ip = in + (q * (to_grid ? nt : nft) + other) * 2;
      re = ip[0] * scale;
      im = ip[1] * scale;
    }
    out[idx * 2] = re;
    out[idx * 2 + 1] = im;
  }
}

template <int D>
void tile_shape(int64_t* e) {
  e[0] = Tile<D>::e0;
  e[1] = Tile<D>::e1;
  e[2] = Tile<D>::e2;
}

void tile_shape_rt(int D, int64_t* e) {
  if (D == 1)
    tile_shape<1>(e);
  else if (D == 2)
    tile_shape<2>(e);
  else
    tile_shape<3>(e);
}

// geometry of a call; false when outside the envelope
bool make_geom(int D, int64_t Q, int64_t M, const int64_t* nf, const int64_t* n, int w, Geom* g, int64_t* nbins) {
  if (D < 1 || D > 3 || Q < 0 || M < 0 || !nf) return false;
  if (w != 0 && (w < 2 || w > kWMax)) return false;
  int64_t e[3];
  tile_shape_rt(D, e);
  int64_t nft = 1, nb = 1;
  for (int d = 0; d < 3; ++d) {
    g->nf[d] = d < D ? nf[d] : 1;
    g->n[d] = d < D && n ? n[d] : 1;
    if (d < D && (g->nf[d] < (w ? 2 * w : 1) || g->nf[d] > kNfMax)) return false;
    if (d < D && n && (n[d] < 1 || n[d] > g->nf[d])) return false;
    g->nb[d] = (g->nf[d] + e[d] - 1) / e[d];
    nft *= g->nf[d];
    nb *= g->nb[d];
    if (nft > ((int64_t)1 << 40) || nb > 0x7fffffff) return false;
  }
  // 2 Q max(nft, M) scalars stay below 2^62
  const int64_t big = nft > M ? nft : M;
  if (Q > 0 && big > ((int64_t)1 << 60) / Q) return false;
  *nbins = nb;
  return true;
}

int q_chunk_for(int64_t Q) { return Q >= 3 ? kGridQChunk : (int)Q; }  // 3 rows run as a padded chunk of 4

template <typename T, int D, bool FAC>
int spread_launch(const Geom& g, int64_t nbins, int64_t Q, int64_t M, int w, double beta, const int32_t* l0,
                  const void* off, const int64_t* perm, const int64_t* bin_start, const void* c, void* grid,
                  const void* fac, int conj_fac, hipStream_t st) {
  const int qc = q_chunk_for(Q);
  const dim3 gr((unsigned)nbins, (unsigned)((Q + qc - 1) / qc));
  const T tw = (T)(2.0 / w), b = (T)beta;
  if (qc == 1)
    hipLaunchKernelGGL((spread_kernel<T, D, 1, FAC>), gr, dim3(kBlock), 0, st, g, Q, M, w, tw, b, l0, (const T*)off, perm,
                       bin_start, (const T*)c, (T*)grid, (const T*)fac, conj_fac);
  else if (qc == 2)
    hipLaunchKernelGGL((spread_kernel<T, D, 2, FAC>), gr, dim3(kBlock), 0, st, g, Q, M, w, tw, b, l0, (const T*)off, perm,
                       bin_start, (const T*)c, (T*)grid, (const T*)fac, conj_fac);
  else
    hipLaunchKernelGGL((spread_kernel<T, D, kGridQChunk, FAC>), gr, dim3(kBlock), 0, st, g, Q, M, w, tw, b, l0,
                       (const T*)off, perm, bin_start, (const T*)c, (T*)grid, (const T*)fac, conj_fac);
  return last_launch_status();
}

template <typename T, int D, bool FAC>
int interp_launch(const Geom& g, int64_t Q, int64_t M, int w, double beta, const int32_t* l0, const void* off,
                  const int64_t* perm, const void* grid, void* out, const void* fac, int conj_fac, hipStream_t st) {
  const int qc = q_chunk_for(Q);
  const dim3 gr((unsigned)((M + kInterpBlock - 1) / kInterpBlock), (unsigned)((Q + qc - 1) / qc));
  const size_t lds = (size_t)D * w * kInterpBlock * sizeof(T);  // <= 48 KiB
  const T tw = (T)(2.0 / w), b = (T)beta;
  if (qc == 1)
    hipLaunchKernelGGL((interp_kernel<T, D, 1, FAC>), gr, dim3(kInterpBlock), lds, st, g, Q, M, w, tw, b, l0,
                       (const T*)off, perm, (const T*)grid, (T*)out, (const T*)fac, conj_fac);
  else if (qc == 2)
    hipLaunchKernelGGL((interp_kernel<T, D, 2, FAC>), gr, dim3(kInterpBlock), lds, st, g, Q, M, w, tw, b, l0,
                       (const T*)off, perm, (const T*)grid, (T*)out, (const T*)fac, conj_fac);
  else
    hipLaunchKernelGGL((interp_kernel<T, D, kGridQChunk, FAC>), gr, dim3(kInterpBlock), lds, st, g, Q, M, w, tw, b, l0,
                       (const T*)off, perm, (const T*)grid, (T*)out, (const T*)fac, conj_fac);
  return last_launch_status();
}

template <bool FAC>
int spread_entry(int dtype, int D, int64_t Q, int64_t M, const int64_t* nf, int w, double beta, const int32_t* l0,
                 const void* off, const int64_t* perm, const int64_t* bin_start, const void* c, void* grid,
                 const void* fac, int conj_fac, void* stream) {
  if (dtype != PXA_F32 && dtype != PXA_F64) return PXA_ERR_DTYPE;
  if (D < 1 || D > 3) return PXA_ERR_UNSUPPORTED;
  Geom g;
  int64_t nbins = 0;
  PXA_CHECK_ARG(w >= 2 && beta > 0 && make_geom(D, Q, M, nf, nullptr, w, &g, &nbins));
  PXA_CHECK_ARG(!FAC || conj_fac == 0 || conj_fac == 1);
  if (Q == 0) return PXA_OK;
  if ((Q + kGridQChunk - 1) / kGridQChunk > 65535) return PXA_ERR_UNSUPPORTED;
  PXA_CHECK_ARG(grid && bin_start && (M == 0 || (l0 && off && perm && c && (!FAC || fac))));
  hipStream_t st = as_stream(stream);
  PXA_DISPATCH(dtype, T, {
    if (D == 1)
      return spread_launch<T, 1, FAC>(g, nbins, Q, M, w, beta, l0, off, perm, bin_start, c, grid, fac, conj_fac, st);
    if (D == 2)
      return spread_launch<T, 2, FAC>(g, nbins, Q, M, w, beta, l0, off, perm, bin_start, c, grid, fac, conj_fac, st);
    return spread_launch<T, 3, FAC>(g, nbins, Q, M, w, beta, l0, off, perm, bin_start, c, grid, fac, conj_fac, st);
  });
}

template <bool FAC>
int interp_entry(int dtype, int D, int64_t Q, int64_t M, const int64_t* nf, int w, double beta, const int32_t* l0,
                 const void* off, const int64_t* perm, const void* grid, void* out, const void* fac, int conj_fac,
                 void* stream) {
  if (dtype != PXA_F32 && dtype != PXA_F64) return PXA_ERR_DTYPE;
  if (D < 1 || D > 3) return PXA_ERR_UNSUPPORTED;
  Geom g;
  int64_t nbins = 0;
  PXA_CHECK_ARG(w >= 2 && beta > 0 && make_geom(D, Q, M, nf, nullptr, w, &g, &nbins));
  PXA_CHECK_ARG(!FAC || conj_fac == 0 || conj_fac == 1);
  if (Q == 0 || M == 0) return PXA_OK;
  if ((Q + kGridQChunk - 1) / kGridQChunk > 65535 || (M + kInterpBlock - 1) / kInterpBlock > 0x7fffffff)
    return PXA_ERR_UNSUPPORTED;
  PXA_CHECK_ARG(grid && out && l0 && off && perm && (!FAC || fac));
  hipStream_t st = as_stream(stream);
  PXA_DISPATCH(dtype, T, {
    if (D == 1) return interp_launch<T, 1, FAC>(g, Q, M, w, beta, l0, off, perm, grid, out, fac, conj_fac, st);
    if (D == 2) return interp_launch<T, 2, FAC>(g, Q, M, w, beta, l0, off, perm, grid, out, fac, conj_fac, st);
    return interp_launch<T, 3, FAC>(g, Q, M, w, beta, l0, off, perm, grid, out, fac, conj_fac, st);
  });
}

}  // namespace
}  // namespace pxa

using namespace pxa;

extern "C" {

int pxa_nufft_grid_tiles(int dtype, int D, int64_t* bin_shape, int64_t* q_chunk, int64_t* batch) {
  PXA_CHECK_ARG(bin_shape && q_chunk && batch);
  if (dtype != PXA_F32 && dtype != PXA_F64) return PXA_ERR_DTYPE;
  if (D < 1 || D > 3) return PXA_ERR_UNSUPPORTED;
  tile_shape_rt(D, bin_shape);
  *q_chunk = kGridQChunk;
  *batch = kBatch;
  return PXA_OK;
}

int pxa_nufft_spread(int dtype, int D, int64_t Q, int64_t M, const int64_t* nf, int w, double beta,
                     const int32_t* l0, const void* off, const int64_t* perm, const int64_t* bin_start,
                     const void* c, void* grid, void* stream) {
  return spread_entry<false>(dtype, D, Q, M, nf, w, beta, l0, off, perm, bin_start, c, grid, nullptr, 0, stream);
}

int pxa_nufft_spread_fac(int dtype, int D, int64_t Q, int64_t M, const int64_t* nf, int w, double beta,
                         const int32_t* l0, const void* off, const int64_t* perm, const int64_t* bin_start,
                         const void* c, void* grid, const void* fac, int conj_fac, void* stream) {
  return spread_entry<true>(dtype, D, Q, M, nf, w, beta, l0, off, perm, bin_start, c, grid, fac, conj_fac, stream);
}

int pxa_nufft_interp(int dtype, int D, int64_t Q, int64_t M, const int64_t* nf, int w, double beta,
                     const int32_t* l0, const void* off, const int64_t* perm, const void* grid, void* out,
                     void* stream) {
  return interp_entry<false>(dtype, D, Q, M, nf, w, beta, l0, off, perm, grid, out, nullptr, 0, stream);
}

int pxa_nufft_interp_fac(int dtype, int D, int64_t Q, int64_t M, const int64_t* nf, int w, double beta,
                         const int32_t* l0, const void* off, const int64_t* perm, const void* grid, void* out,
                         const void* fac, int conj_fac, void* stream) {
  return interp_entry<true>(dtype, D, Q, M, nf, w, beta, l0, off, perm, grid, out, fac, conj_fac, stream);
}

int pxa_nufft_deconv(int dtype, int D, int64_t Q, const int64_t* n, const int64_t* nf, int modeord, int to_grid,
                     const void* corr, const void* in, void* out, void* stream) {
  if (dtype != PXA_F32 && dtype != PXA_F64) return PXA_ERR_DTYPE;
  if (D < 1 || D > 3) return PXA_ERR_UNSUPPORTED;
  Geom g;
  int64_t nbins = 0;
  PXA_CHECK_ARG(n && (modeord == 0 || modeord == 1) && make_geom(D, Q, 0, nf, n, 0, &g, &nbins));
  if (Q == 0) return PXA_OK;
  PXA_CHECK_ARG(corr && in && out);
  const int64_t per = to_grid ? g.nf[0] * g.nf[1] * g.nf[2] : g.n[0] * g.n[1] * g.n[2];
  hipStream_t st = as_stream(stream);
  PXA_DISPATCH(dtype, T, {
    hipLaunchKernelGGL((deconv_kernel<T>), dim3(grid_for(Q * per)), dim3(kBlock), 0, st, g, D, Q, modeord,
                       to_grid ? 1 : 0, (const T*)corr, (const T*)in, (T*)out);
    return last_launch_status();
  });
}

}  // extern "C"
