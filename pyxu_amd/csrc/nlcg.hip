// NLCG iteration tail (opt/solver/nlcg.py:213-227) after grad f(x_{k+1}), in two launches instead of the row-op
// chain (two norms or a difference, a product and a sum, the ratio, the clip, p * beta, - g1, and the <g, p> pass of
// the next line search, math/linesearch.py:72):
//   nlcg_dot   per-block partials of sum g1^2 and, for Polak-Ribiere, of sum g1 (g1 - g0): the difference in T (as
//              the reference forms it), product and sum in double.  Never sum g1^2 - sum g1 g0, which cancels.
//   nlcg_p     every block folds the partials in the same fixed order; beta = (T)(gg1 / gg0) (FR), (T)max(0, num /
//              gg0) (PR+), 0 on a restart; p_new = beta p - g1 out of place, per-block partials of <g1, p_new>;
//              block 0 stores gg1 for the next step (device) and into host memory with a completion flag, as
//              cg_p_kernel does
// and the Armijo test of one backtracking trial (math/linesearch.py:74-93) for every row in one launch:
//   ls_armijo  one wavefront per row: d_f = (T)c (T)<g, p>, rhs = f_x + a d_f (product, then sum, each rounded to T),
//              fail = f_trial > rhs, a *= r and ++trials on fail; the number of failing rows goes to host memory
//              with a completion flag (the `.any()` of the reference's loop as one four-byte host read)
// One row of the stacked problem per grid.y (direction update).  All sums in double with the partition of cg.hip
// (cg_blocks / cg_block_sum) and a fixed order, no atomics: bit-reproducible run to run.
#include "common.hpp"

namespace pxa {
namespace {

// fixed-order fold of the nb partials of row `row` (cg.hip: every thread of the wavefront gets the same bits)
__device__ inline double fold(const double* __restrict__ part, int64_t row, int nb) {
  const int lane = threadIdx.x & 63;
  const double* pr = part + row * nb;
  double s = 0.0;
  for (int k0 = 0; k0 < nb; k0 += 64) {
    const double v = k0 + lane < nb ? pr[k0 + lane] : 0.0;
    const int m = nb - k0 < 64 ? nb - k0 : 64;
    for (int j = 0; j < m; ++j) s += __shfl(v, j, 64);
  }
  return s;
}

constexpr int kVarFR = PXA_NLCG_FR, kVarPR = PXA_NLCG_PR;

template <typename T, int VAR>
__global__ void __launch_bounds__(kBlock) nlcg_dot_kernel(int64_t n, const T* __restrict__ g1, const T* __restrict__ g0,
                                                          double* __restrict__ part_gg, double* __restrict__ part_num) {
  __shared__ double sh[kBlock / 64];
  const int64_t row = blockIdx.y;
  const int64_t chunk = (n + gridDim.x - 1) / gridDim.x, lo = blockIdx.x * chunk;
  const int64_t hi = lo + chunk < n ? lo + chunk : n;
  const T* a = g1 + row * n;
  double gg = 0.0, num = 0.0;
  if (VAR == kVarPR) {
    const T* b = g0 + row * n;
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
      const T v = a[i];
      const T d = v - b[i];  // in T, as g_kp1 - g_k (nlcg.py:262)
      gg = fma((double)v, (double)v, gg);
      num = fma((double)v, (double)d, num);
    }
  } else {
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
      const T v = a[i];
      gg = fma((double)v, (double)v, gg);
    }
  }
  const double s = cg_block_sum(gg, sh);
  if (threadIdx.x == 0) part_gg[row * gridDim.x + blockIdx.x] = s;
  if (VAR == kVarPR) {
    const double t = cg_block_sum(num, sh);
    if (threadIdx.x == 0) part_num[row * gridDim.x + blockIdx.x] = t;
  }
}

// loads issued kNlBatch at a time, the first batch before the partial fold (cg.hip's cg_p_kernel)
constexpr int kNlBatch = 4;

template <typename T>
__global__ void __launch_bounds__(kBlock) nlcg_p_kernel(int64_t n, int var, int restart, const double* __restrict__ gg0,
                                                        const double* __restrict__ part_gg,
                                                        const double* __restrict__ part_num, const T* __restrict__ g1,
                                                        const T* __restrict__ p, T* __restrict__ p_new,
                                                        double* __restrict__ part_gp, double* __restrict__ gg_out,
                                                        double* __restrict__ gg_host, unsigned* __restrict__ flags,
                                                        unsigned seq) {
  __shared__ double sh[kBlock / 64];
  const int64_t row = blockIdx.y;
  const int64_t chunk = (n + gridDim.x - 1) / gridDim.x, lo = blockIdx.x * chunk;
  const int64_t hi = lo + chunk < n ? lo + chunk : n;
  const T* gr = g1 + row * n;
  const T* pr = p + row * n;
  T* pw = p_new + row * n;
  T gv[kNlBatch], pv[kNlBatch];
  auto load = [&](int64_t ib) {
#pragma unroll
    for (int k = 0; k < kNlBatch; ++k) {
      const int64_t i = ib + (int64_t)k * kBlock;
      if (i < hi) {
        gv[k] = gr[i];
        pv[k] = pr[i];
      }
    }
  };
  const int64_t i0 = lo + threadIdx.x;
  load(i0);
  const double gg = fold(part_gg, row, gridDim.x);
  T beta = (T)0;
  if (!restart) {
    double q = (var == kVarPR ? fold(part_num, row, gridDim.x) : gg) / gg0[row];  // plain IEEE division
    if (var == kVarPR && q < 0.0) q = 0.0;  // clip(min=0): a NaN stays a NaN (nlcg.py:264)
    beta = (T)q;
  }
  double acc = 0.0;
  for (int64_t ib = i0; ib < hi; ib += (int64_t)kNlBatch * kBlock) {
    if (ib != i0) load(ib);
#pragma unroll
    for (int k = 0; k < kNlBatch; ++k) {
      const int64_t i = ib + (int64_t)k * kBlock;
      if (i < hi) {
        const T pn = fma(beta, pv[k], -gv[k]);  // p_new = beta p - g1
        pw[i] = pn;
        acc = fma((double)gv[k], (double)pn, acc);
      }
    }
  }
  const double s = cg_block_sum(acc, sh);
  if (threadIdx.x == 0) {
    part_gp[row * gridDim.x + blockIdx.x] = s;
    if (blockIdx.x == 0) {
      gg_out[row] = gg;
      if (gg_host) gg_host[row] = gg;
      if (flags) {  // the stop check polls this flag instead of waiting for a stream event
        __threadfence_system();
        __hip_atomic_store(flags + row, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
}

constexpr int kLsBlock = 1024;  // 16 wavefronts, wavefront w takes rows w, w + 16, ...

// rhs = f_x + a * ((T)c * (T)gp): three operations, each rounded to T (no contraction into an fma)
template <typename T>
__device__ inline T armijo_rhs(T fx, T a, T c, T gp) {
#pragma clang fp contract(off)
  const T d_f = c * gp;
  const T ad = a * d_f;
  return fx + ad;
}

template <typename T>
__global__ void __launch_bounds__(kLsBlock) ls_armijo_kernel(int64_t rows, const T* __restrict__ f_trial,
                                                             const T* __restrict__ f_x, const double* __restrict__ gp,
                                                             int nb, T c, T r, T* __restrict__ a,
                                                             int32_t* __restrict__ trials, unsigned* __restrict__ nfail_host,
                                                             unsigned* __restrict__ flag, unsigned seq) {
  __shared__ unsigned cnt[kLsBlock / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned nfail = 0;  // wave-uniform
  for (int64_t row = w; row < rows; row += kLsBlock / 64) {
    const double s = nb > 0 ? fold(gp, row, nb) : gp[row];
    const T av = a[row];
    const bool fail = f_trial[row] > armijo_rhs<T>(f_x[row], av, c, (T)s);  // false when either side is NaN
    if (fail) {
      ++nfail;
      if (lane == 0) {
        a[row] = av * r;
        trials[row] += 1;
      }
    }
  }
  if (lane == 0) cnt[w] = nfail;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned t = 0;
    for (int k = 0; k < kLsBlock / 64; ++k) t += cnt[k];
    *nfail_host = t;
    __threadfence_system();
    __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

}  // namespace
}  // namespace pxa

using namespace pxa;

extern "C" {

size_t pxa_nlcg_workspace_bytes(int64_t rows) { return rows > 0 ? (size_t)rows * 3 * kCgBlocks * sizeof(double) : 0; }

int pxa_nlcg_direction(int dtype, int variant, int restart, int64_t rows, int64_t n, const void* g1, const void* g0,
                       const void* p, void* p_new, const double* gg0, double* gg_out, double* gg_host, uint32_t* flags,
                       uint32_t seq, void* work, void* stream) {
  PXA_CHECK_ARG(rows >= 1 && rows <= 65535 && n >= 1);
  PXA_CHECK_ARG(variant == kVarFR || variant == kVarPR);
  const bool pr = variant == kVarPR && !restart;
  PXA_CHECK_ARG(g1 && p && p_new && p_new != p && p_new != g1 && gg0 && gg_out && work && gg_out != gg0);
  PXA_CHECK_ARG(!pr || g0);
  hipStream_t st = as_stream(stream);
  const int nb = cg_blocks(n);
  double* part_gg = (double*)work;
  double* part_num = part_gg + rows * kCgBlocks;
  double* part_gp = part_num + rows * kCgBlocks;
  const dim3 grid((unsigned)nb, (unsigned)rows);
  PXA_DISPATCH(dtype, T, {
    if (pr)
      hipLaunchKernelGGL((nlcg_dot_kernel<T, kVarPR>), grid, dim3(kBlock), 0, st, n, (const T*)g1, (const T*)g0, part_gg,
                         part_num);
    else
      hipLaunchKernelGGL((nlcg_dot_kernel<T, kVarFR>), grid, dim3(kBlock), 0, st, n, (const T*)g1, (const T*)nullptr,
                         part_gg, part_num);
    int e = last_launch_status();
    if (e) return e;
    hipLaunchKernelGGL((nlcg_p_kernel<T>), grid, dim3(kBlock), 0, st, n, pr ? kVarPR : kVarFR, restart ? 1 : 0, gg0,
                       part_gg, part_num, (const T*)g1, (const T*)p, (T*)p_new, part_gp, gg_out, gg_host,
                       (unsigned*)flags, (unsigned)seq);
    return last_launch_status();
  });
}

int pxa_ls_armijo(int dtype, int64_t rows, const void* f_trial, const void* f_x, const double* gp, int32_t nb, double c,
                  double r, void* a, int32_t* trials, uint32_t* nfail_host, uint32_t* flag, uint32_t seq, void* stream) {
  PXA_CHECK_ARG(rows >= 1 && rows <= 65535 && nb >= 0 && nb <= kCgBlocks);
  PXA_CHECK_ARG(f_trial && f_x && gp && a && trials && nfail_host && flag);
  hipStream_t st = as_stream(stream);
  PXA_DISPATCH(dtype, T, {
    hipLaunchKernelGGL((ls_armijo_kernel<T>), dim3(1), dim3(kLsBlock), 0, st, rows, (const T*)f_trial, (const T*)f_x, gp,
                       (int)nb, (T)c, (T)r, (T*)a, trials, (unsigned*)nfail_host, (unsigned*)flag, (unsigned)seq);
    return last_launch_status();
  });
}

}  // extern "C"
