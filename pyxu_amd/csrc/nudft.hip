// pyxu_amd — non-uniform DFT by direct evaluation (reference operator/linop/fft/nufft.py:2820-2880, the kernel
// behind NUFFT.type1/2/3 with eps = 0):
//   out[q, n] = sum_m w[q, m] exp(i isign <src_m, tgt_n>)
//
// Mapping.  A workgroup of kBlock threads owns kBlock * TPT targets (thread t: targets n0 + t + k kBlock) and one
// source split; a thread keeps its targets' coordinates (premultiplied by isign) and 2 QC accumulators per target
// in registers.  Sources are staged through LDS kTileM at a time (coordinates and QC weight rows), prefetched
// into registers one tile ahead; in the inner loop every lane reads the same LDS address (a broadcast: no bank
// conflicts).  Phase, range reduction and sine / cosine are computed once per (m, n) and feed 4 QC FMAs, issued as
// 2 QC two-wide ones: the (re, im) accumulator pair takes (wr, wr) x (cos, sin), then (-wi, wi) x (sin, cos), and
// the weight pairs are laid out that way in LDS so that the packed fp32 FMA needs no operand shuffling.  A stack of
// more than kQChunk rows runs in passes (one launch each).
//
// Splits.  The grid is target tiles x source splits; split s owns sources [s Ms, (s + 1) Ms), Ms = ceil(M / splits).
// With one split the kernel writes `out`; otherwise it writes a partial (splits, Q, N) slab into `work` and a
// second launch adds the partials in ascending split order.  No atomics: the same call gives the same bits.
#include "common.hpp"

namespace pxa {
namespace {

constexpr int kTileM = 256;  // sources per LDS tile (one per thread of the staging step)
constexpr int kQChunk = 4;   // stack rows per pass
static_assert(kTileM == kBlock, "thread t stages source t of the tile");

template <typename T>
constexpr int kTpt = sizeof(T) == 4 ? 2 : 1;  // targets per thread

// sin / cos of the phase p (radians).
//
// fp32: the phase is reduced in quarter revolutions against a two-term 2 / pi (= 4 x 1 / 2 pi): n = rint(p C_hi),
// r = p C_hi - n in one FMA (the product is not rounded), then the p C_lo correction, so the reduction costs two
// roundings of |r| <= 1/2 quarter revolutions, <= 0.4 u radians each, instead of ~u |p|.  The hardware sine and
// cosine (v_sin_f32 / v_cos_f32, argument in revolutions) are then taken of r / 4, |r / 4| <= 1/8, and n mod 4
// swaps / negates them.  Keeping the argument that small is what makes the hardware pair admissible: both are within
// 2.1 u of the true value over [-1/2, 1/2] (scripts/nudft_hw_sincos_probe.hip, measured on an MI355X), but a
// phase reduced to whole revolutions carries up to 1.6 u of rounding per step near 1/2 revolution.  Whole
// function, measured by the same probe: DESIGN.md §8h.  n is exact in fp32 up to |p| ~ 2^24.
__device__ inline void sincos_phase(float p, float& s, float& c) {
  constexpr double k2OverPi = 0.6366197723675814;
  constexpr float kHi = (float)k2OverPi;
  constexpr float kLo = (float)(k2OverPi - (double)kHi);
  const float n = __builtin_rintf(p * kHi);
  float r = __builtin_fmaf(p, kHi, -n);
  r = __builtin_fmaf(p, kLo, r);
  const float a = 0.25f * r;
  const float ps = __builtin_amdgcn_sinf(a), pc = __builtin_amdgcn_cosf(a);
  const int qi = (int)n;
  const bool swap = qi & 1;
  const float sa = swap ? pc : ps, ca = swap ? ps : pc;
  s = (qi & 2) ? -sa : sa;
  c = ((qi + 1) & 2) ? -ca : ca;
}

// fp64: the library's double sincos (exact reduction of the argument, Payne-Hanek for large phases).
__device__ inline void sincos_phase(double p, double& s, double& c) { sincos(p, &s, &c); }

template <typename T>
__device__ inline T fma_t(T a, T b, T c) {
  return __builtin_fma(a, b, c);
}
template <>
__device__ inline float fma_t<float>(float a, float b, float c) {
  return __builtin_fmaf(a, b, c);
}

// dst: `out` (Q, N) with one split, the partial slab (splits, Q, N) otherwise; the launch covers stack rows
// [q0, q0 + QC) (rows >= Q are padding: zero weights, not stored).
template <typename T, int D, int QC>
__global__ __launch_bounds__(kBlock) void nudft_kernel(int64_t Q, int64_t M, int64_t N, int64_t q0, int64_t Ms,
                                                       const T* __restrict__ src, const T* __restrict__ tgt,
                                                       T isign, const T* __restrict__ w, T* __restrict__ dst) {
  constexpr int TPT = kTpt<T>;
  constexpr int DP = D == 3 ? 4 : D;
  __shared__ __attribute__((aligned(16))) T s_c[kTileM][DP];
  __shared__ __attribute__((aligned(16))) T s_w[kTileM][4 * QC];  // per row (wr, wr, -wi, wi)
  typedef T V2 __attribute__((ext_vector_type(2)));

  const int t = threadIdx.x;
  const int64_t n_base = (int64_t)blockIdx.x * (kBlock * TPT);
  const int64_t split = blockIdx.y;
  const int64_t m_lo = split * Ms < M ? split * Ms : M;
  const int64_t m_hi = m_lo + Ms < M ? m_lo + Ms : M;

  T tc[TPT][D];
  V2 acc[TPT][QC];  // (re, im)
#pragma unroll
  for (int k = 0; k < TPT; ++k) {
    const int64_t n = n_base + t + (int64_t)k * kBlock;
#pragma unroll
    for (int d = 0; d < D; ++d) tc[k][d] = n < N ? isign * tgt[n * D + d] : (T)0;
#pragma unroll
    for (int j = 0; j < QC; ++j) acc[k][j] = V2{(T)0, (T)0};
  }

  // one source per thread, a tile ahead of the LDS copy
  T rc[D], rw[2 * QC];
  auto fetch = [&](int64_t m0) {
    const int64_t m = m0 + t;
    const bool in = m < m_hi;
#pragma unroll
    for (int d = 0; d < D; ++d) rc[d] = in ? src[m * D + d] : (T)0;
#pragma unroll
    for (int j = 0; j < QC; ++j) {
      const bool ok = in && q0 + j < Q;
      rw[2 * j] = ok ? w[((q0 + j) * M + m) * 2] : (T)0;
      rw[2 * j + 1] = ok ? w[((q0 + j) * M + m) * 2 + 1] : (T)0;
    }
  };

  if (m_lo < m_hi) fetch(m_lo);
  for (int64_t m0 = m_lo; m0 < m_hi; m0 += kTileM) {
    __syncthreads();  // the previous tile has been consumed
#pragma unroll
    for (int d = 0; d < D; ++d) s_c[t][d] = rc[d];
#pragma unroll
    for (int j = 0; j < QC; ++j) {
      s_w[t][4 * j] = s_w[t][4 * j + 1] = rw[2 * j];
      s_w[t][4 * j + 2] = -rw[2 * j + 1];
      s_w[t][4 * j + 3] = rw[2 * j + 1];
    }
    __syncthreads();
    if (m0 + kTileM < m_hi) fetch(m0 + kTileM);
    const int cnt = (int)(m_hi - m0 < kTileM ? m_hi - m0 : kTileM);
#pragma unroll 2
    for (int i = 0; i < cnt; ++i) {
      T sc[D];
      V2 sw[2 * QC];
#pragma unroll
      for (int d = 0; d < D; ++d) sc[d] = s_c[i][d];
#pragma unroll
      for (int j = 0; j < 2 * QC; ++j) sw[j] = V2{s_w[i][2 * j], s_w[i][2 * j + 1]};
#pragma unroll
      for (int k = 0; k < TPT; ++k) {
        T p = sc[0] * tc[k][0];
#pragma unroll
        for (int d = 1; d < D; ++d) p = fma_t<T>(sc[d], tc[k][d], p);
        T s, c;
        sincos_phase(p, s, c);
        const V2 cs = {c, s}, sn = {s, c};
#pragma unroll
        for (int j = 0; j < QC; ++j) {  // re: wr c - wi s, im: wr s + wi c, in this order
          acc[k][j] = __builtin_elementwise_fma(sw[2 * j], cs, acc[k][j]);
          acc[k][j] = __builtin_elementwise_fma(sw[2 * j + 1], sn, acc[k][j]);
        }
      }
    }
  }

  T* base = dst + split * Q * N * 2;  // split == 0 when dst is `out`
#pragma unroll
  for (int k = 0; k < TPT; ++k) {
    const int64_t n = n_base + t + (int64_t)k * kBlock;
    if (n >= N) continue;
#pragma unroll
    for (int j = 0; j < QC; ++j) {
      if (q0 + j >= Q) break;
      T* o = base + ((q0 + j) * N + n) * 2;
      o[0] = acc[k][j].x;
      o[1] = acc[k][j].y;
    }
  }
}

// out[i] = work[0][i] + work[1][i] + ... in ascending split order, i over the 2 Q N scalars of `out`
template <typename T>
__global__ __launch_bounds__(kBlock) void nudft_fold_kernel(int64_t len, int64_t splits, const T* __restrict__ work,
                                                            T* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < len; i += (int64_t)gridDim.x * kBlock) {
    T a = work[i];
    for (int64_t s = 1; s < splits; ++s) a += work[s * len + i];
    out[i] = a;
  }
}

template <typename T>
int64_t target_tiles(int64_t N) {
  return (N + kBlock * kTpt<T> - 1) / (kBlock * kTpt<T>);
}

// Source splits chosen from the shapes alone: none once the target tiles fill the chip (one per CU); otherwise
// enough for ~4 workgroups per CU, each split keeping at least 4 LDS tiles of sources.
template <typename T>
int64_t auto_splits(int64_t M, int64_t N) {
  const int64_t nt = target_tiles<T>(N);
  if (nt >= 256 || nt < 1) return 1;
  int64_t s = (1024 + nt - 1) / nt;
  const int64_t cap = M / (4 * kTileM);
  if (s > cap) s = cap;
  if (s > 256) s = 256;
  return s < 1 ? 1 : s;
}

template <typename T, int D>
int launch_pass(int qc, dim3 grid, hipStream_t st, int64_t Q, int64_t M, int64_t N, int64_t q0, int64_t Ms, const T* src,
                const T* tgt, T isign, const T* w, T* dst) {
  if (qc == 1)
    hipLaunchKernelGGL((nudft_kernel<T, D, 1>), grid, dim3(kBlock), 0, st, Q, M, N, q0, Ms, src, tgt, isign, w, dst);
  else if (qc == 2)
    hipLaunchKernelGGL((nudft_kernel<T, D, 2>), grid, dim3(kBlock), 0, st, Q, M, N, q0, Ms, src, tgt, isign, w, dst);
  else
    hipLaunchKernelGGL((nudft_kernel<T, D, kQChunk>), grid, dim3(kBlock), 0, st, Q, M, N, q0, Ms, src, tgt, isign, w,
                       dst);
  return last_launch_status();
}

template <typename T>
int nudft_entry(int D, int64_t Q, int64_t M, int64_t N, const void* src, const void* tgt, int isign, const void* w,
                void* out, int64_t splits, void* work, hipStream_t st) {
  if (splits == 0) splits = auto_splits<T>(M, N);
  if (Q == 0 || N == 0) return PXA_OK;
  PXA_CHECK_ARG(out && tgt && (M == 0 || (src && w)) && (splits == 1 || work));
  const int64_t nt = target_tiles<T>(N);
  if (nt > 0x7fffffff) return PXA_ERR_UNSUPPORTED;
  const int64_t Ms = (M + splits - 1) / splits;
  T* dst = splits == 1 ? (T*)out : (T*)work;
  const dim3 grid((unsigned)nt, (unsigned)splits);
  for (int64_t q0 = 0; q0 < Q;) {
    const int64_t rem = Q - q0;
    const int qc = rem >= 3 ? kQChunk : (int)rem;  // 3 rows run as a padded chunk of 4
    int rc;
    if (D == 1)
      rc = launch_pass<T, 1>(qc, grid, st, Q, M, N, q0, Ms, (const T*)src, (const T*)tgt, (T)isign, (const T*)w, dst);
    else if (D == 2)
      rc = launch_pass<T, 2>(qc, grid, st, Q, M, N, q0, Ms, (const T*)src, (const T*)tgt, (T)isign, (const T*)w, dst);
    else
      rc = launch_pass<T, 3>(qc, grid, st, Q, M, N, q0, Ms, (const T*)src, (const T*)tgt, (T)isign, (const T*)w, dst);
    if (rc != 0) return rc;
    q0 += qc;
  }
  if (splits > 1) {
    const int64_t len = 2 * Q * N;
    hipLaunchKernelGGL((nudft_fold_kernel<T>), dim3(grid_for(len)), dim3(kBlock), 0, st, len, splits, (const T*)work,
                       (T*)out);
    return last_launch_status();
  }
  return PXA_OK;
}

bool nudft_args_ok(int D, int64_t Q, int64_t M, int64_t N, int64_t splits) {
  if (D < 1 || D > 3 || Q < 0 || M < 0 || N < 0 || splits < 0 || splits > 65535) return false;
  // every index (2 Q max(M, N) splits scalars at most) stays below 2^62
  const int64_t big = M > N ? M : N;
  if (Q > 0 && big > 0 && big > ((int64_t)1 << 61) / Q / (splits > 0 ? splits : 256)) return false;
  return true;
}

}  // namespace
}  // namespace pxa

using namespace pxa;

extern "C" {

int pxa_nudft_tiles(int dtype, int64_t* tile_n, int64_t* tile_m, int64_t* q_chunk) {
  PXA_CHECK_ARG(tile_n && tile_m && q_chunk);
  if (dtype != PXA_F32 && dtype != PXA_F64) return PXA_ERR_DTYPE;
  *tile_n = dtype == PXA_F32 ? kBlock * kTpt<float> : kBlock * kTpt<double>;
  *tile_m = kTileM;
  *q_chunk = kQChunk;
  return PXA_OK;
}

size_t pxa_nudft_workspace_bytes(int dtype, int D, int64_t Q, int64_t M, int64_t N, int64_t splits) {
  if ((dtype != PXA_F32 && dtype != PXA_F64) || !nudft_args_ok(D, Q, M, N, splits)) return (size_t)-1;
  if (splits == 0) splits = dtype == PXA_F32 ? auto_splits<float>(M, N) : auto_splits<double>(M, N);
  if (splits == 1) return 0;
  return (size_t)splits * (size_t)Q * (size_t)N * 2 * (dtype == PXA_F32 ? sizeof(float) : sizeof(double));
}

int pxa_nudft(int dtype, int D, int64_t Q, int64_t M, int64_t N, const void* src, const void* tgt, int isign,
              const void* w, void* out, int64_t splits, void* work, void* stream) {
  if (dtype != PXA_F32 && dtype != PXA_F64) return PXA_ERR_DTYPE;
  if (D < 1 || D > 3) return PXA_ERR_UNSUPPORTED;
  PXA_CHECK_ARG((isign == 1 || isign == -1) && nudft_args_ok(D, Q, M, N, splits));
  PXA_DISPATCH(dtype, T, return nudft_entry<T>(D, Q, M, N, src, tgt, isign, w, out, splits, work, as_stream(stream)));
}

}  // extern "C"
