// Row threshold search and shrink: the proxes of LInfinityNorm, the l1 ball and SquaredL1Norm.
//
// Per row, with |x| the magnitudes, the root mu* of the convex, decreasing, piecewise-linear
//     h(mu) = a sum_i max(|x_i| - mu, 0) - b mu - c
// is found by Newton's iteration from the left (Michelot's algorithm):
//     S = sum |x_i|;  not finite -> mu = NaN;  a S - c <= 0 -> mu = 0;
//     mu = max(0, (a S - c) / (a n + b)), k_prev = n;
//     repeat: k = #{|x_i| > mu}, C = their sum;  k >= k_prev (or k == 0) -> done, keep mu;
//             mu = (a C - c) / (a k + b), k_prev = k.
// k strictly decreases until the end, so at most n + 1 passes run; every loop below carries that bound.  Counts
// are integers, sums are double with a partition and fold order that depend on (rows, n) only, and the rule's
// products and sums are rounded one by one (no contraction), so mu* is bitwise reproducible run to run.
//
// Rows of up to pxa_row_threshold_resident_max(dtype) elements: one workgroup per row holds the row in registers
// (16-byte loads, vectors-per-thread a template parameter), runs the whole loop in-kernel and writes the output
// once.  Longer rows: one pass is a (blocks_per_row x rows) partial launch plus a one-wavefront-per-row update
// launch; rows marked done in their state word cost an immediate return.  No workgroup waits for another.
#include "common.hpp"

namespace pxa {
namespace {

struct Coef {
  double a, b, c;
};

constexpr int kResVecs = 8;        // 16-byte vectors per thread of the largest resident instantiation
constexpr int kResThreads = 1024;  // its workgroup

template <typename T>
constexpr int64_t kResidentMax = (int64_t)kResThreads * kResVecs * kVecN<T>;

// (a s - c) / (a k + b), every operation rounded on its own
__device__ inline double newton_point(Coef q, double s, double k) {
  return __ddiv_rn(__dsub_rn(__dmul_rn(q.a, s), q.c), __dadd_rn(__dmul_rn(q.a, k), q.b));
}

// After the S pass: true when the row is finished (mu = NaN or 0).
__device__ inline bool start_rule(Coef q, int64_t n, double S, double& mu) {
  if (!(fabs(S) <= 1.79769313486231570e308)) {  // NaN or inf in the row
    mu = __builtin_nan("");
    return true;
  }
  if (__dsub_rn(__dmul_rn(q.a, S), q.c) <= 0.0) {
    mu = 0.0;
    return true;
  }
  const double t = newton_point(q, S, (double)n);
  mu = t > 0.0 ? t : 0.0;
  return false;
}

// After a count pass at mu: true when the active set no longer shrinks (mu is kept).
__device__ inline bool step_rule(Coef q, int64_t k, int64_t k_prev, double C, double& mu) {
  if (k >= k_prev || k == 0) return true;
  mu = newton_point(q, C, (double)k);
  return false;
}

// out element for threshold mu: CLAMP sign(x) min(|x|, mu), SOFT sign(x) max(|x| - mu, 0); one rounding to T.
template <typename T, int MODE>
__device__ inline T shrink(double x, double mu) {  // x: the element of dtype T, as a double
  const double m = fabs(x);
  if (MODE == PXA_SHRINK_CLAMP) return (T)(m > mu ? copysign(mu, x) : x);
  const double d = __dsub_rn(m, mu);
  return (T)copysign(d > 0.0 ? d : 0.0, x);  // sign(x) * 0 keeps x's sign, as NumPy's product does
}

// ------------------------------------------------------------------------------------------ resident path
// Thread t holds vectors t, t + THREADS, ...: element (j THREADS + t) V + e in v[j][e]; elements past n are 0
// (never above a threshold >= 0).  Per pass: per-thread sum in (j, e) order and the wave's count from the compare masks, a DPP wave sum, the NW wave
// results through LDS (two buffers, one barrier per pass) added in ascending wave order by every thread.
template <typename T, int THREADS, int VPT>
__global__ void __launch_bounds__(THREADS) resident_kernel(int64_t n, Coef q, int mode, bool vec, const T* x, T* out,
                                                           double* __restrict__ mu_out, int* __restrict__ passes_out) {
  constexpr int V = kVecN<T>;
  constexpr int NW = THREADS / kWave;
  using VT = typename Vec4<T>::type;
  __shared__ double s_sum[2][NW];
  __shared__ int s_cnt[2][NW];
  const int64_t row = blockIdx.x;
  const T* xr = x + row * n;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;

  double v[VPT][V];  // the row as doubles (exact): float32 rows would otherwise be converted again in every pass
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int64_t e0 = ((int64_t)j * THREADS + threadIdx.x) * V;
    T t[V];
    if (vec && e0 < n) {  // vec: n % V == 0 and 16-byte aligned rows
      *reinterpret_cast<VT*>(t) = *reinterpret_cast<const VT*>(xr + e0);
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) t[e] = (!vec && e0 + e < n) ? xr[e0 + e] : T(0);
    }
#pragma unroll
    for (int e = 0; e < V; ++e) v[j][e] = (double)t[e];
  }

  int buf = 0;
  auto fold = [&](double s, int cnt, double& C, int64_t& k) {  // cnt: the wave's count, the same in every lane
    s = wave_sum_f64(s);
    if (lane == 0) {
      s_sum[buf][w] = s;
      s_cnt[buf][w] = cnt;
    }
    __syncthreads();
    C = s_sum[buf][0];
    k = s_cnt[buf][0];
#pragma unroll
    for (int i = 1; i < NW; ++i) {
      C += s_sum[buf][i];
      k += s_cnt[buf][i];
    }
    buf ^= 1;
  };

  double C;
  int64_t k;
  {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < VPT; ++j)
#pragma unroll
      for (int e = 0; e < V; ++e) s += fabs(v[j][e]);
    fold(s, 0, C, k);
  }
  double mu;
  int passes = 1;
  bool done = start_rule(q, n, C, mu);
  int64_t k_prev = n;
  for (int64_t it = 0; !done && it < n + 1; ++it) {
    // per element: one compare, one select and one fma.  The count is the population count of the compare's lane
    // mask (scalar unit), already the wave's; m * 1 + s is the sum m + s, m * 0 + s is s (m is finite here)
    double s = 0.0;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < VPT; ++j)
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const double m = fabs(v[j][e]);
        const bool in = m > mu;
        cnt += __popcll(__ballot(in));
        s = fma(m, in ? 1.0 : 0.0, s);
      }
    fold(s, cnt, C, k);
    ++passes;
    done = step_rule(q, k, k_prev, C, mu);
    k_prev = k;
  }

  if (threadIdx.x == 0) {
    mu_out[row] = mu;
    passes_out[row] = passes;
  }
  if (out == nullptr) return;
  T* orow = out + row * n;
  const bool soft = mode == PXA_SHRINK_SOFT;
  const bool bad = mu != mu;
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int64_t e0 = ((int64_t)j * THREADS + threadIdx.x) * V;
    T o[V];
#pragma unroll
    for (int e = 0; e < V; ++e)
      o[e] = bad ? (T)mu : (soft ? shrink<T, PXA_SHRINK_SOFT>(v[j][e], mu) : shrink<T, PXA_SHRINK_CLAMP>(v[j][e], mu));
    if (vec && e0 < n) {
      *reinterpret_cast<VT*>(orow + e0) = *reinterpret_cast<VT*>(o);
    } else if (!vec) {
#pragma unroll
      for (int e = 0; e < V; ++e)
        if (e0 + e < n) orow[e0 + e] = o[e];
    }
  }
}

template <typename T, int THREADS, int VPT>
int launch_resident_as(int64_t rows, int64_t n, Coef q, int mode, bool vec, const void* x, void* out, double* mu,
                       int32_t* passes, void* stream) {
  hipLaunchKernelGGL((resident_kernel<T, THREADS, VPT>), dim3((unsigned)rows), dim3(THREADS), 0, as_stream(stream), n, q,
                     mode, vec, (const T*)x, (T*)out, mu, (int*)passes);
  return last_launch_status();
}

// workgroup by n alone: 256 threads while 8 vectors per thread hold the row, then 512, then 1024
template <typename T>
int launch_resident(int64_t rows, int64_t n, Coef q, int mode, const void* x, void* out, double* mu, int32_t* passes,
                    void* stream) {
  constexpr int V = kVecN<T>;
  const bool vec = n % V == 0 && aligned16(x) && (out == nullptr || aligned16(out));
  const int64_t nv = (n + V - 1) / V;
#define PXA_RES(TH, VP) return (launch_resident_as<T, TH, VP>(rows, n, q, mode, vec, x, out, mu, passes, stream))
  if (nv <= 256) PXA_RES(256, 1);
  if (nv <= 512) PXA_RES(256, 2);
  if (nv <= 1024) PXA_RES(256, 4);
  if (nv <= 2048) PXA_RES(256, 8);
  if (nv <= 4096) PXA_RES(512, 8);
  PXA_RES(1024, 8);
#undef PXA_RES
}

// ------------------------------------------------------------------------------------------ streaming path
// Same partition and per-thread order as row_partial_kernel (reduce.hip).  FIRST: the S pass (every element
// counts, NaN included); otherwise the count pass at mu[row] of a row whose state word is still 0.
template <typename T, bool FIRST>
__global__ void __launch_bounds__(kBlock) thr_partial_kernel(int64_t n, int nb, const T* __restrict__ x,
                                                             const double* __restrict__ mu,
                                                             const int* __restrict__ state, double* __restrict__ psum,
                                                             long long* __restrict__ pcnt) {
  const int64_t row = blockIdx.y;
  if (!FIRST && state[row] != 0) return;
  const double m0 = FIRST ? 0.0 : mu[row];
  const T* xr = x + row * n;
  const int64_t chunk = (n + nb - 1) / nb;
  const int64_t lo = (int64_t)blockIdx.x * chunk;
  const int64_t hi = lo + chunk < n ? lo + chunk : n;
  double acc = 0.0;
  long long cnt = 0;
#pragma unroll 4
  for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    const double m = fabs((double)xr[i]);
    if (FIRST) {
      acc += m;
    } else {
      const bool in = m > m0;
      cnt += in ? 1 : 0;
      acc += in ? m : 0.0;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    acc += __shfl_down(acc, off, 64);
    cnt += __shfl_down(cnt, off, 64);
  }
  __shared__ double sw[kBlock / kWave];
  __shared__ long long sc[kBlock / kWave];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
    sw[w] = acc;
    sc[w] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = sw[0];
    long long c = sc[0];
    for (int i = 1; i < kBlock / kWave; ++i) {
      r += sw[i];
      c += sc[i];
    }
    psum[row * nb + blockIdx.x] = r;
    pcnt[row * nb + blockIdx.x] = c;
  }
}

// One wavefront per row: the fold of row_final_kernel over the row's partials, then the rule.
template <bool FIRST>
__global__ void __launch_bounds__(kBlock) thr_update_kernel(int64_t rows, int64_t n, int nb, Coef q,
                                                            const double* __restrict__ psum,
                                                            const long long* __restrict__ pcnt, double* __restrict__ mu,
                                                            long long* __restrict__ k_prev, int* __restrict__ state,
                                                            int* __restrict__ passes) {
  const int lane = threadIdx.x & 63;
  const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (r >= rows) return;
  if (!FIRST && state[r] != 0) return;
  const double* ps = psum + r * nb;
  const long long* pc = pcnt + r * nb;
  double acc = lane < nb ? ps[lane] : 0.0;
  long long cnt = lane < nb ? pc[lane] : 0;
  for (int i = lane + 64; i < nb; i += 64) {
    acc += ps[i];
    cnt += pc[i];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    acc += __shfl_down(acc, off, 64);
    cnt += __shfl_down(cnt, off, 64);
  }
  if (lane != 0) return;
  if (FIRST) {
    double m;
    const bool done = start_rule(q, n, acc, m);
    mu[r] = m;
    k_prev[r] = n;
    state[r] = done ? 1 : 0;
    passes[r] = 1;
  } else {
    double m = mu[r];
    const bool done = step_rule(q, cnt, k_prev[r], acc, m);
    mu[r] = m;
    k_prev[r] = cnt;
    state[r] = done ? 1 : 0;
    passes[r] += 1;
  }
}

template <typename T>
int launch_stream(int64_t rows, int64_t n, Coef q, const void* x, int first, int64_t npasses, double* mu, int32_t* state,
                  int32_t* passes, void* work, void* stream) {
  const int nb = blocks_per_row(rows, n);
  double* psum = (double*)work;
  long long* pcnt = (long long*)(psum + rows * nb);
  long long* k_prev = pcnt + rows * nb;
  hipStream_t s = as_stream(stream);
  const dim3 pgrid(nb, (unsigned)rows), ugrid((unsigned)((rows + kBlock / kWave - 1) / (kBlock / kWave)));
  int e;
  if (first) {
    hipLaunchKernelGGL((thr_partial_kernel<T, true>), pgrid, dim3(kBlock), 0, s, n, nb, (const T*)x, mu, (const int*)state,
                       psum, pcnt);
    if ((e = last_launch_status())) return e;
    hipLaunchKernelGGL((thr_update_kernel<true>), ugrid, dim3(kBlock), 0, s, rows, n, nb, q, psum, pcnt, mu, k_prev,
                       (int*)state, (int*)passes);
    if ((e = last_launch_status())) return e;
  }
  for (int64_t p = 0; p < npasses; ++p) {
    hipLaunchKernelGGL((thr_partial_kernel<T, false>), pgrid, dim3(kBlock), 0, s, n, nb, (const T*)x, mu,
                       (const int*)state, psum, pcnt);
    if ((e = last_launch_status())) return e;
    hipLaunchKernelGGL((thr_update_kernel<false>), ugrid, dim3(kBlock), 0, s, rows, n, nb, q, psum, pcnt, mu, k_prev,
                       (int*)state, (int*)passes);
    if ((e = last_launch_status())) return e;
  }
  return PXA_OK;
}

// ------------------------------------------------------------------------------------------ shrink
// Element-wise structure (elementwise.hip): 16-byte vectors when every row is aligned, scalar otherwise; grid.y
// is the row, grid.x strides over it.  out may alias x (element i is read and written by one thread only).
template <typename T, int MODE>
__global__ void __launch_bounds__(kBlock) shrink_kernel(int64_t n, bool vec, const T* x, const double* __restrict__ mu,
                                                        T* out) {
  constexpr int V = kVecN<T>;
  using VT = typename Vec4<T>::type;
  const int64_t row = blockIdx.y;
  const double m = mu[row];
  const bool bad = m != m;
  const T* xr = x + row * n;
  T* orow = out + row * n;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nv = vec ? n / V : 0;
  for (int64_t i = tid; i < nv; i += stride) {
    T a[V], o[V];
    *reinterpret_cast<VT*>(a) = reinterpret_cast<const VT*>(xr)[i];
#pragma unroll
    for (int e = 0; e < V; ++e) o[e] = bad ? (T)m : shrink<T, MODE>((double)a[e], m);
    reinterpret_cast<VT*>(orow)[i] = *reinterpret_cast<VT*>(o);
  }
  for (int64_t i = nv * V + tid; i < n; i += stride) orow[i] = bad ? (T)m : shrink<T, MODE>((double)xr[i], m);
}

template <typename T, int MODE>
int launch_shrink(int64_t rows, int64_t n, const void* x, const double* mu, void* out, void* stream) {
  constexpr int V = kVecN<T>;
  const bool vec = aligned16(x) && aligned16(out) && (rows == 1 || n % V == 0);
  const int64_t items = vec ? (n + V - 1) / V : n;
  int64_t gx = (items + kBlock - 1) / kBlock;
  const int64_t cap = (kMaxGrid + rows - 1) / rows;
  if (gx > cap) gx = cap;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL((shrink_kernel<T, MODE>), dim3((unsigned)gx, (unsigned)rows), dim3(kBlock), 0, as_stream(stream), n,
                     vec, (const T*)x, mu, (T*)out);
  return last_launch_status();
}

inline bool coef_ok(double a, double b, double c) { return a > 0.0 && b >= 0.0 && c >= 0.0 && a + b + c < INFINITY; }

}  // namespace
}  // namespace pxa

using namespace pxa;

extern "C" {

int64_t pxa_row_threshold_resident_max(int dtype) {
  if (dtype == PXA_F32) return kResidentMax<float>;
  if (dtype == PXA_F64) return kResidentMax<double>;
  return 0;
}

int pxa_row_threshold_prox(int dtype, int mode, int64_t rows, int64_t n, const void* x, double a, double b, double c,
                           void* out, double* mu, int32_t* passes, void* stream) {
  PXA_CHECK_ARG(rows >= 0 && n >= 0);
  if (rows == 0 || n == 0) return PXA_OK;
  PXA_CHECK_ARG(rows <= 65535);
  PXA_CHECK_ARG(n <= pxa_row_threshold_resident_max(dtype) || (dtype != PXA_F32 && dtype != PXA_F64));
  PXA_CHECK_ARG(coef_ok(a, b, c));
  PXA_CHECK_ARG(mode == PXA_SHRINK_CLAMP || mode == PXA_SHRINK_SOFT);
  PXA_CHECK_ARG(x != nullptr && mu != nullptr && passes != nullptr);
  const Coef q{a, b, c};
  PXA_DISPATCH(dtype, T, return launch_resident<T>(rows, n, q, mode, x, out, mu, passes, stream));
}

size_t pxa_row_threshold_workspace_bytes(int64_t rows, int64_t n) {
  if (rows <= 0) return 0;
  return (size_t)rows * ((size_t)blocks_per_row(rows, n) * 16 + 8);
}

int pxa_row_threshold_stream(int dtype, int64_t rows, int64_t n, const void* x, double a, double b, double c, int first,
                             int64_t npasses, double* mu, int32_t* state, int32_t* passes, void* work, void* stream) {
  PXA_CHECK_ARG(rows >= 0 && n >= 0 && npasses >= 0);
  if (rows == 0 || n == 0) return PXA_OK;
  PXA_CHECK_ARG(rows <= 65535);  // grid.y limit
  PXA_CHECK_ARG(coef_ok(a, b, c));
  PXA_CHECK_ARG(x != nullptr && mu != nullptr && state != nullptr && passes != nullptr && work != nullptr);
  const Coef q{a, b, c};
  PXA_DISPATCH(dtype, T, return launch_stream<T>(rows, n, q, x, first, npasses, mu, state, passes, work, stream));
}

int pxa_row_shrink(int dtype, int mode, int64_t rows, int64_t n, const void* x, const double* mu, void* out,
                   void* stream) {
  PXA_CHECK_ARG(rows >= 0 && n >= 0);
  if (rows == 0 || n == 0) return PXA_OK;
  PXA_CHECK_ARG(rows <= 65535);  // grid.y limit
  PXA_CHECK_ARG(x != nullptr && mu != nullptr && out != nullptr);
  if (mode == PXA_SHRINK_CLAMP) PXA_DISPATCH(dtype, T, return (launch_shrink<T, PXA_SHRINK_CLAMP>(rows, n, x, mu, out, stream)));
  if (mode == PXA_SHRINK_SOFT) PXA_DISPATCH(dtype, T, return (launch_shrink<T, PXA_SHRINK_SOFT>(rows, n, x, mu, out, stream)));
  return PXA_ERR_ARG;
}

}  // extern "C"
