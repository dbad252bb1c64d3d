// Re-orthogonalisation of one Krylov vector against a row-major basis V (j <= 64 rows of n), the hot loop of the
// thick-restart Lanczos behind LinOp.svdvals (math/_lanczos.py).  Two classical Gram-Schmidt passes in three launches:
//   krylov_dots     c[i] = scale <V_i, w>                                   one pass over V
//   krylov_update   w' = w - sum_i c[i] V_i, c'[i] = <V_i, w'>              V read, then re-read from cache
//   krylov_update   w'' = w' - sum_i c'[i] V_i, ||w''||^2                   one pass over V
// plus krylov_normalize (x / sqrt(nrm2) from the device value, a zero row for nrm2 == 0).
//
// Partition: the columns are cut into chunks of kKrChunk<T> = 256 threads x 32 bytes; workgroup b of G =
// min(chunks, kKrMaxGrid) owns chunks b, b + G, ...  It keeps its chunk of w in registers while it walks the rows of
// V (16-byte loads, four rows in flight), forms each row's chunk dot in double (per thread in element order, then
// wave_sum_f64, then the four wave sums in order) and adds it to the row's running sum over its chunks, in chunk
// order.  The G partials of a row are folded by the workgroup that arrives last, lane l summing partials l, l + 64,
// ... in order, then wave_sum_f64: a fixed partition and order, no floating-point atomics, the same bits for the
// same call.  The arrival counter is an integer ticket; the partials travel by write-through agent-scope stores and
// are read by agent-scope loads behind one acquire (kr_publish_fold).
//
// The update accumulates w - sum c_i V_i in double with the coefficients in double and rounds once to T, so its
// error is one rounding of the result plus (j + 1) 2^-53 sum |c_i V_i| (the bound the tests use); for fp64 it is
// the plain fma chain.
//
// Rows that are not 16-byte aligned (V, w or w_out misaligned, or ldv not a whole number of vectors) take the scalar
// instantiation: thread t owns elements t, t + 256, ... of the chunk instead of two 16-byte vectors.
#include "common.hpp"

namespace pxa {
namespace {

constexpr int kKrMaxRows = 64;
constexpr int kKrMaxGrid = 2048;  // 8 workgroups per CU
constexpr int kKrRowBatch = 4;    // rows of V whose loads are issued before the first is used
constexpr int kKrHeader = 256;    // bytes in front of the partials: the arrival counter in its own 16-byte block
template <typename T>
constexpr int kKrEpt = 32 / (int)sizeof(T);  // elements of w a thread keeps
template <typename T>
constexpr int kKrChunk = kBlock * kKrEpt<T>;

inline int kr_grid(int64_t n, int chunk) {
  const int64_t c = (n + chunk - 1) / chunk;
  return (int)(c < kKrMaxGrid ? c : kKrMaxGrid);
}

// Offset inside the chunk of element k of this thread.
template <typename T, bool VEC>
__device__ inline int kr_off(int k) {
  constexpr int VN = kVecN<T>;
  return VEC ? ((k / VN) * kBlock + (int)threadIdx.x) * VN + k % VN : k * kBlock + (int)threadIdx.x;
}

// This thread's elements of the chunk starting at column lo of the row at p; columns >= n read as 0.
template <typename T, bool VEC>
__device__ inline void kr_load(const T* p, int64_t lo, int64_t n, T (&r)[kKrEpt<T>]) {
  constexpr int E = kKrEpt<T>, VN = kVecN<T>;
  if constexpr (VEC) {
    using V4 = typename Vec4<T>::type;
#pragma unroll
    for (int q = 0; q < E / VN; ++q) {
      const int64_t e = lo + (int64_t)(q * kBlock + (int)threadIdx.x) * VN;
      if (e + VN <= n) {
        const V4 v = *reinterpret_cast<const V4*>(p + e);
        const T* s = reinterpret_cast<const T*>(&v);
#pragma unroll
        for (int m = 0; m < VN; ++m) r[q * VN + m] = s[m];
      } else {
#pragma unroll
        for (int m = 0; m < VN; ++m) r[q * VN + m] = e + m < n ? p[e + m] : T(0);
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const int64_t e = lo + kr_off<T, false>(k);
      r[k] = e < n ? p[e] : T(0);
    }
  }
}

template <typename T, bool VEC>
__device__ inline void kr_store(T* p, int64_t lo, int64_t n, const T (&r)[kKrEpt<T>]) {
  constexpr int E = kKrEpt<T>, VN = kVecN<T>;
  if constexpr (VEC) {
    using V4 = typename Vec4<T>::type;
#pragma unroll
    for (int q = 0; q < E / VN; ++q) {
      const int64_t e = lo + (int64_t)(q * kBlock + (int)threadIdx.x) * VN;
      if (e + VN <= n) {
        V4 v;
        T* s = reinterpret_cast<T*>(&v);
#pragma unroll
        for (int m = 0; m < VN; ++m) s[m] = r[q * VN + m];
        *reinterpret_cast<V4*>(p + e) = v;
      } else {
#pragma unroll
        for (int m = 0; m < VN; ++m)
          if (e + m < n) p[e + m] = r[q * VN + m];
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const int64_t e = lo + kr_off<T, false>(k);
      if (e < n) p[e] = r[k];
    }
  }
}

// red[i][wave] = this wave's part of <V_i, w> over the chunk at lo, i < j (double, element order per thread).
template <typename T, bool VEC>
__device__ inline void kr_chunk_dots(int j, int64_t n, const T* __restrict__ V, int64_t ldv, int64_t lo,
                                     const T (&w)[kKrEpt<T>], double (*red)[kBlock / kWave]) {
  constexpr int E = kKrEpt<T>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i0 = 0; i0 < j; i0 += kKrRowBatch) {
    T v[kKrRowBatch][E];
#pragma unroll
    for (int b = 0; b < kKrRowBatch; ++b) {
      const int i = i0 + b < j ? i0 + b : j - 1;  // a short last batch re-reads row j - 1 and drops it
      kr_load<T, VEC>(V + (int64_t)i * ldv, lo, n, v[b]);
    }
#pragma unroll
    for (int b = 0; b < kKrRowBatch; ++b) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < E; ++k) a = fma((double)v[b][k], (double)w[k], a);
      a = wave_sum_f64(a);
      if (lane == 0 && i0 + b < j) red[i0 + b][wave] = a;
    }
  }
}

// Adds the chunk sums in red to the running sums: thread i keeps row i's.  Both barriers are needed: red is
// written again by the next chunk.
__device__ inline void kr_accumulate(int rows, double (*red)[kBlock / kWave], double& run) {
  __syncthreads();
  if ((int)threadIdx.x < rows) {
    const double* r = red[threadIdx.x];
    run += ((r[0] + r[1]) + r[2]) + r[3];
  }
  __syncthreads();
}

// Thread i < rows publishes its running sum as partial (i, blockIdx.x); the workgroup that arrives last folds
// every row in a fixed order and writes out[i] = fold * scale (i < nscaled) or out_tail[0] = fold (i == nscaled,
// the squared norm of the update).  The hand-off: the partials leave as write-through (agent-scope) stores, every
// wave waits for its stores to complete, and behind the workgroup barrier one lane counts the workgroup in with an
// agent-scope add; the lane whose add came last runs one agent-scope acquire, and the fold reads the partials
// with agent-scope loads.  No release fence: per workgroup it would write back the whole L2 of the XCD (measured:
// 0.558 against 0.151 ms for a step at n = 2^22, j = 8, fp32; profiles/svdvals_bench.txt).
__device__ inline void kr_publish_fold(int rows, double run, unsigned* counter, double* part, int nscaled,
                                       const double* scale, double* out, double* out_tail) {
  __shared__ unsigned last;
  const int G = gridDim.x;
  if ((int)threadIdx.x < rows)
    __hip_atomic_store(part + (int64_t)threadIdx.x * G + blockIdx.x, run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave: its partial stores have completed
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool l = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(G - 1);
    if (l) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the invalidate has completed before the barrier opens
    }
    last = l ? 1u : 0u;
  }
  __syncthreads();
  if (!last) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double sc = scale ? *scale : 1.0;
  constexpr int kPer = 16;  // partials of a row a lane loads before it adds them (kKrMaxGrid / 64 = two batches)
  for (int i = wave; i < rows; i += kBlock / kWave) {
    const double* pr = part + (int64_t)i * G;
    double s = 0.0;
    for (int b0 = lane; b0 < G; b0 += 64 * kPer) {
      double v[kPer];
#pragma unroll
      for (int q = 0; q < kPer; ++q)
        v[q] = b0 + 64 * q < G ? __hip_atomic_load(pr + b0 + 64 * q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
#pragma unroll
      for (int q = 0; q < kPer; ++q) s += v[q];
    }
    s = wave_sum_f64(s);
    if (lane == 0) {
      if (i < nscaled)
        out[i] = s * sc;
      else
        out_tail[0] = s;
    }
  }
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(kBlock) krylov_dots_kernel(int j, int64_t n, const T* __restrict__ V, int64_t ldv,
                                                             const T* __restrict__ w, const double* scale,
                                                             double* c_out, unsigned* counter, double* part) {
  __shared__ double red[kKrMaxRows + 1][kBlock / kWave];
  constexpr int C = kKrChunk<T>;
  const int64_t chunks = (n + C - 1) / C;
  double run = 0.0;
  for (int64_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const int64_t lo = ch * C;
    T wr[kKrEpt<T>];
    kr_load<T, VEC>(w, lo, n, wr);
    kr_chunk_dots<T, VEC>(j, n, V, ldv, lo, wr, red);
    kr_accumulate(j, red, run);
  }
  kr_publish_fold(j, run, counter, part, j, scale, c_out, nullptr);
}

// w and w_out may be the same row: a workgroup reads its chunk of w before it writes it, and chunks are disjoint.
template <typename T, bool VEC>
__global__ void __launch_bounds__(kBlock) krylov_update_kernel(int j, int64_t n, const T* __restrict__ V, int64_t ldv,
                                                               const T* w, const double* __restrict__ c, T* w_out,
                                                               double* c_next, double* nrm2_out, unsigned* counter,
                                                               double* part) {
  __shared__ double red[kKrMaxRows + 1][kBlock / kWave];
  constexpr int C = kKrChunk<T>, E = kKrEpt<T>;
  const int64_t chunks = (n + C - 1) / C;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rows = (c_next ? j : 0) + (nrm2_out ? 1 : 0);  // partial rows: c_next's j, then the squared norm
  double run = 0.0;
  for (int64_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const int64_t lo = ch * C;
    T wr[E];
    kr_load<T, VEC>(w, lo, n, wr);
    double acc[E];
#pragma unroll
    for (int k = 0; k < E; ++k) acc[k] = (double)wr[k];
    for (int i0 = 0; i0 < j; i0 += kKrRowBatch) {
      T v[kKrRowBatch][E];
      double ci[kKrRowBatch];
#pragma unroll
      for (int b = 0; b < kKrRowBatch; ++b) {
        const int i = i0 + b < j ? i0 + b : j - 1;
        kr_load<T, VEC>(V + (int64_t)i * ldv, lo, n, v[b]);
        ci[b] = i0 + b < j ? c[i] : 0.0;
      }
#pragma unroll
      for (int b = 0; b < kKrRowBatch; ++b)
        if (i0 + b < j) {  // (a dropped row must not touch acc: 0 * NaN)
#pragma unroll
          for (int k = 0; k < E; ++k) acc[k] = fma(-ci[b], (double)v[b][k], acc[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < E; ++k) wr[k] = (T)acc[k];
    kr_store<T, VEC>(w_out, lo, n, wr);
    if (rows == 0) continue;
    if (c_next) kr_chunk_dots<T, VEC>(j, n, V, ldv, lo, wr, red);  // the chunk's rows again, from cache
    if (nrm2_out) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const int64_t e = lo + kr_off<T, VEC>(k);
        if (e < n) a = fma((double)wr[k], (double)wr[k], a);
      }
      a = wave_sum_f64(a);
      if (lane == 0) red[rows - 1][wave] = a;
    }
    kr_accumulate(rows, red, run);
  }
  if (rows == 0) return;
  kr_publish_fold(rows, run, counter, part, c_next ? j : 0, nullptr, c_next, nrm2_out);
}

template <typename T>
__global__ void __launch_bounds__(kBlock) krylov_normalize_kernel(int64_t n, const T* x, const double* __restrict__ nrm2,
                                                                  T* out) {
  const double q = *nrm2;
  const double s = q == 0.0 ? 0.0 : 1.0 / sqrt(q);  // a zero vector stays zero; NaN stays NaN
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    out[i] = s == 0.0 ? T(0) : (T)((double)x[i] * s);
}

template <typename T>
bool kr_vec(const void* V, int64_t ldv, const void* w, const void* w_out) {
  return aligned16(V) && aligned16(w) && aligned16(w_out) && (ldv * (int64_t)sizeof(T)) % 16 == 0;
}

int kr_check(int dtype, int64_t j, int64_t n, const void* V, int64_t ldv, const void* w, const void* work) {
  if (dtype != PXA_F32 && dtype != PXA_F64) return PXA_ERR_DTYPE;
  PXA_CHECK_ARG(j >= 1 && n >= 1 && ldv >= n);
  if (j > kKrMaxRows) return PXA_ERR_UNSUPPORTED;
  PXA_CHECK_ARG(V && w && work && aligned16(work));
  return PXA_OK;
}

}  // namespace
}  // namespace pxa

using namespace pxa;

extern "C" {

int64_t pxa_krylov_chunk(int dtype) { return dtype == PXA_F32 ? kKrChunk<float> : dtype == PXA_F64 ? kKrChunk<double> : 0; }

size_t pxa_krylov_workspace_bytes(int64_t j, int64_t n) {
  if (j < 1 || j > kKrMaxRows || n < 1) return 0;
  // the grid of the smaller chunk (fp64) bounds both precisions
  return (size_t)kKrHeader + (size_t)(j + 1) * (size_t)kr_grid(n, kKrChunk<double>) * sizeof(double);
}

int pxa_krylov_dots(int dtype, int64_t j, int64_t n, const void* V, int64_t ldv, const void* w, const double* scale,
                    double* c_out, void* work, void* stream) {
  int e = kr_check(dtype, j, n, V, ldv, w, work);
  if (e) return e;
  PXA_CHECK_ARG(c_out != nullptr);
  hipStream_t st = as_stream(stream);
  e = (int)hipMemsetAsync(work, 0, 16, st);
  if (e) return e;
  unsigned* counter = (unsigned*)work;
  double* part = (double*)((char*)work + kKrHeader);
  PXA_DISPATCH(dtype, T, {
    const dim3 grid((unsigned)kr_grid(n, kKrChunk<T>));
    return with_bool(kr_vec<T>(V, ldv, w, w), [&](auto vec) {
      hipLaunchKernelGGL((krylov_dots_kernel<T, decltype(vec)::value>), grid, dim3(kBlock), 0, st, (int)j, n,
                         (const T*)V, ldv, (const T*)w, scale, c_out, counter, part);
      return last_launch_status();
    });
  });
}

int pxa_krylov_update(int dtype, int64_t j, int64_t n, const void* V, int64_t ldv, const void* w, const double* c,
                      void* w_out, double* c_next, double* nrm2_out, void* work, void* stream) {
  int e = kr_check(dtype, j, n, V, ldv, w, work);
  if (e) return e;
  PXA_CHECK_ARG(c != nullptr && w_out != nullptr && c_next != c);
  hipStream_t st = as_stream(stream);
  if (c_next || nrm2_out) {
    e = (int)hipMemsetAsync(work, 0, 16, st);
    if (e) return e;
  }
  unsigned* counter = (unsigned*)work;
  double* part = (double*)((char*)work + kKrHeader);
  PXA_DISPATCH(dtype, T, {
    const dim3 grid((unsigned)kr_grid(n, kKrChunk<T>));
    return with_bool(kr_vec<T>(V, ldv, w, w_out), [&](auto vec) {
      hipLaunchKernelGGL((krylov_update_kernel<T, decltype(vec)::value>), grid, dim3(kBlock), 0, st, (int)j, n,
                         (const T*)V, ldv, (const T*)w, c, (T*)w_out, c_next, nrm2_out, counter, part);
      return last_launch_status();
    });
  });
}

int pxa_krylov_normalize(int dtype, int64_t n, const void* x, const double* nrm2, void* out, void* stream) {
  PXA_CHECK_ARG(n >= 1 && x && nrm2 && out);
  PXA_DISPATCH(dtype, T, {
    hipLaunchKernelGGL((krylov_normalize_kernel<T>), dim3(grid_for(n)), dim3(kBlock), 0, as_stream(stream), n,
                       (const T*)x, nrm2, (T*)out);
    return last_launch_status();
  });
}

}  // extern "C"
