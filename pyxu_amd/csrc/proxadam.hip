// ProxAdam hot path (opt/solver/prox_adam.py:332-416), for `rows` stacked problems of n entries, one row per grid.y:
//   moments   everything between f.grad(x) and x' in one launch: m' = b1 m + (1 - b1) g, v' = max(b2 v + (1 - b2) g^2,
//             eps_var), vhat' = max(vhat, v') (v' on the first step), phi / psi of the variant, x' = x - a phi / psi out
//             of place; with a prox to follow also psi and the per-workgroup maxima of psi (about 10 array streams
//             instead of the ~45 of the reference's in-place chain)
//   sub_init  folds the maxima to psimax per row, clears the per-row state words and the counters
//   sub_step  one accelerated PGD iteration of the metric prox  min_z g(z) + 1/(2a) ||z - xt||^2_diag(psi)  on every
//             row that still runs: launch k first folds the partials launch k - 1 left (sum (z_{k-1} - z_{k-2})^2 and
//             sum z_{k-2}^2) and tests RelError; a row that passes copies z_{k-1} to the output buffer, records k in
//             its state word and does nothing from then on; the others form y = z + a_k (z - z_prev),
//             w = (1 - r) y + r xt with r = psi / psimax (= y - gamma grad f_sub(y), gamma = a / psimax; exactly xt where
//             r == 1), z_new = prox_g(w, gamma) and their own partials.  The number of rows still running goes to host
//             memory with a completion flag (as ls_armijo's failing-row count).
// Partition: blocks_per_row(rows, n) workgroups per row (up to 1024: one long row fills the device), workgroup b owns
// [b chunk, (b + 1) chunk) with chunk = ceil(n / blocks) rounded up to a whole 16-byte vector.  16-byte accesses where
// every pointer and the row pitch allow, scalar otherwise and for the tail.  All sums in double, folded in a fixed
// order; the only atomics are on integer counters: the same call gives the same bits.
#include "common.hpp"

namespace pxa {
namespace {

constexpr int kAdam = PXA_PROXADAM_ADAM, kAmsgrad = PXA_PROXADAM_AMSGRAD, kPadam = PXA_PROXADAM_PADAM;
constexpr int kProxL1 = PXA_PROX_L1, kProxPos = PXA_PROX_POS, kProxPosL1 = PXA_PROX_POSL1, kProxBox = PXA_PROX_BOX;

template <typename T>
inline int64_t pa_chunk(int64_t n, int nb) {
  const int64_t c = (n + nb - 1) / nb;
  return (c + kVecN<T> - 1) / kVecN<T> * kVecN<T>;
}

// numpy.maximum / numpy.clip: a NaN operand gives NaN (fmax drops it)
template <typename T>
__device__ inline T nanmax(T a, T b) {
  return (a != a || b != b) ? a + b : (a > b ? a : b);
}

template <typename T>
__device__ inline T wave_nanmax(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = nanmax(v, (T)__shfl_down(v, off, 64));
  return v;
}

// Fixed-order sum of the nb partials of one row by a whole workgroup; every thread returns the same bits.  `sh`:
// kBlock / 64 + 1 doubles.
__device__ inline double block_fold(const double* __restrict__ pr, int nb, double* sh) {
  double acc = 0.0;
  for (int k = threadIdx.x; k < nb; k += kBlock) acc += pr[k];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[w] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = sh[0];
    for (int k = 1; k < kBlock / kWave; ++k) r += sh[k];
    sh[kBlock / kWave] = r;
  }
  __syncthreads();
  return sh[kBlock / kWave];
}

template <typename T>
struct MomArgs {
  T b1, omb1, b2, omb2, eps_var, c1, c2, eps_adam, a, p;
  int first, p_half;
};

template <typename T, int VAR>
__device__ inline void mom_elem(const MomArgs<T>& A, T g, T m, T v, T vh, T x, T& mo, T& vo, T& vho, T& xo, T& psi) {
  mo = fma(A.b1, m, A.omb1 * g);
  const T vu = fma(A.b2, v, A.omb2 * (g * g));
  vo = vu < A.eps_var ? A.eps_var : vu;  // clip(eps_var, None): a NaN stays
  vho = A.first ? vo : nanmax(vh, vo);
  T phi;
  if (VAR == kAdam) {
    phi = mo / A.c1;
    psi = sqrt(vo) / A.c2 + A.eps_adam;
  } else {
    phi = mo;
    psi = (VAR == kAmsgrad || A.p_half) ? sqrt(vho) : pow(vho, A.p);
  }
  T q = phi / psi;
  q = q * A.a;
  xo = x - q;
}

// m_out / v_out / vh_out may be m / v / vh (element i is read and written by one thread): no __restrict__ on them
template <typename T, int VAR>
__global__ void __launch_bounds__(kBlock) moments_kernel(int64_t n, int64_t chunk, MomArgs<T> A, bool vec, const T* g,
                                                         const T* m, const T* v, const T* vh, const T* x, T* m_out,
                                                         T* v_out, T* vh_out, T* x_out, T* psi_out,
                                                         double* __restrict__ part_max) {
  constexpr int V = kVecN<T>;
  using VT = typename Vec4<T>::type;
  __shared__ T shm[kBlock / kWave];
  const int64_t row = blockIdx.y, base = row * n;
  const int64_t lo = (int64_t)blockIdx.x * chunk;
  const int64_t hi = lo + chunk < n ? lo + chunk : n;
  T pmax = -INFINITY;
  const int64_t len = hi > lo ? hi - lo : 0;
  const int64_t nv = vec ? len / V : 0;
  for (int64_t i = threadIdx.x; i < nv; i += kBlock) {
    const int64_t e = base + lo + i * V;
    T vg[V], vm[V], vv[V], vvh[V], vx[V], om[V], ov[V], ovh[V], ox[V], op[V];
    *reinterpret_cast<VT*>(vg) = *reinterpret_cast<const VT*>(g + e);
    *reinterpret_cast<VT*>(vm) = *reinterpret_cast<const VT*>(m + e);
    *reinterpret_cast<VT*>(vv) = *reinterpret_cast<const VT*>(v + e);
    *reinterpret_cast<VT*>(vx) = *reinterpret_cast<const VT*>(x + e);
    if (!A.first) *reinterpret_cast<VT*>(vvh) = *reinterpret_cast<const VT*>(vh + e);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      mom_elem<T, VAR>(A, vg[k], vm[k], vv[k], A.first ? T(0) : vvh[k], vx[k], om[k], ov[k], ovh[k], ox[k], op[k]);
      pmax = nanmax(pmax, op[k]);
    }
    *reinterpret_cast<VT*>(m_out + e) = *reinterpret_cast<VT*>(om);
    *reinterpret_cast<VT*>(v_out + e) = *reinterpret_cast<VT*>(ov);
    *reinterpret_cast<VT*>(vh_out + e) = *reinterpret_cast<VT*>(ovh);
    *reinterpret_cast<VT*>(x_out + e) = *reinterpret_cast<VT*>(ox);
    if (psi_out) *reinterpret_cast<VT*>(psi_out + e) = *reinterpret_cast<VT*>(op);
  }
  for (int64_t i = lo + nv * V + threadIdx.x; i < hi; i += kBlock) {
    const int64_t e = base + i;
    T om, ov, ovh, ox, op;
    mom_elem<T, VAR>(A, g[e], m[e], v[e], A.first ? T(0) : vh[e], x[e], om, ov, ovh, ox, op);
    pmax = nanmax(pmax, op);
    m_out[e] = om;
    v_out[e] = ov;
    vh_out[e] = ovh;
    x_out[e] = ox;
    if (psi_out) psi_out[e] = op;
  }
  if (part_max) {
    pmax = wave_nanmax(pmax);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) shm[w] = pmax;
    __syncthreads();
    if (threadIdx.x == 0) {
      T r = shm[0];
      for (int k = 1; k < kBlock / kWave; ++k) r = nanmax(r, shm[k]);
      part_max[row * gridDim.x + blockIdx.x] = (double)r;  // (-inf from a workgroup without elements)
    }
  }
}

// one wavefront per row: psimax[row] = max of the row's nb partial maxima (NaN-propagating), state[row] = 0
__global__ void __launch_bounds__(kBlock) sub_init_kernel(int64_t rows, int nb, const double* __restrict__ part_max,
                                                          double* __restrict__ psimax, int32_t* __restrict__ state,
                                                          int32_t* __restrict__ counters) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
  if (blockIdx.x == 0 && threadIdx.x < 2) counters[threadIdx.x] = 0;
  if (row >= rows) return;
  double mx = -INFINITY;
  for (int k = lane; k < nb; k += 64) mx = nanmax(mx, part_max[row * nb + k]);
  mx = wave_nanmax(mx);
  if (lane == 0) {
    psimax[row] = mx;
    state[row] = 0;
  }
}

template <typename T, int KIND>
__device__ inline T prox_elem(T w, T thr) {
  if (KIND == kProxL1) {  // L1Norm.prox (elementwise.hip soft)
    T mg = fabs(w) - thr;
    mg = mg > T(0) ? mg : T(0);
    const T s = w > T(0) ? T(1) : (w < T(0) ? T(-1) : T(0));
    return mg * s;
  }
  if (KIND == kProxPos) return w < T(0) ? T(0) : w;  // clip(w, 0, None)
  if (KIND == kProxPosL1) {                          // clip(w + (-thr), 0, None)
    const T u = w + (-thr);
    return u < T(0) ? T(0) : u;
  }
  const T lo = w < -thr ? -thr : w;  // clip(w, -r, r)
  return lo > thr ? thr : lo;
}

template <typename T, int KIND>
__device__ inline T sub_elem(T z, T zp, T xt, T psi, T mom, T pmaxT, T thr, double& num, double& den) {
  T d = z - zp;  // (z - z_prev) * a + z, as the PGD momentum step (elementwise.hip ExtrapOp)
  d = d * mom;
  const T y = d + z;
  const T r = psi / pmaxT;
  const T w = fma(r, xt, (T(1) - r) * y);
  const T zn = prox_elem<T, KIND>(w, thr);
  const double dz = (double)zn - (double)z;
  num = fma(dz, dz, num);
  den = fma((double)z, (double)z, den);
  return zn;
}

template <typename T, int KIND>
__global__ void __launch_bounds__(kBlock) sub_step_kernel(
    int64_t rows, int64_t n, int64_t chunk, int k, T mom, double eps, T a, T pw, bool vec, const T* __restrict__ xt,
    const T* __restrict__ psi, const T* __restrict__ zp, const T* __restrict__ z, T* __restrict__ zn,
    T* __restrict__ out, const double* __restrict__ psimax, const double* __restrict__ part_prev,
    double* __restrict__ part_cur, int32_t* state, int32_t* counters, unsigned* __restrict__ nrun_host,
    unsigned* __restrict__ flag, unsigned seq) {
  constexpr int V = kVecN<T>;
  using VT = typename Vec4<T>::type;
  __shared__ double sh[kBlock / kWave + 1];
  const int64_t row = blockIdx.y, base = row * n;
  const int nb = gridDim.x;
  const int64_t lo = (int64_t)blockIdx.x * chunk;
  const int64_t hi = lo + chunk < n ? lo + chunk : n;
  const int64_t len = hi > lo ? hi - lo : 0;
  const int64_t nv = vec ? len / V : 0;
  const int32_t st = state[row];  // 0, or the launch at which the row froze (this very launch: decide again)
  const bool frozen = st != 0 && st < k;
  bool running = false;
  if (!frozen) {
    bool stop = false;
    if (k >= 2) {  // (the first check defers: launch 1 left the first pair of statistics)
      const double num = block_fold(part_prev + row * nb, nb, sh);
      const double den = block_fold(part_prev + (rows + row) * nb, nb, sh);
      stop = sqrt(num) <= eps * sqrt(den);
    }
    if (stop) {  // z = z_{k-1} is the row's solution
      for (int64_t i = threadIdx.x; i < nv; i += kBlock) {
        const int64_t e = base + lo + i * V;
        *reinterpret_cast<VT*>(out + e) = *reinterpret_cast<const VT*>(z + e);
      }
      for (int64_t i = lo + nv * V + threadIdx.x; i < hi; i += kBlock) out[base + i] = z[base + i];
      if (blockIdx.x == 0 && threadIdx.x == 0) state[row] = k;
    } else {
      running = true;
      const T pmaxT = (T)psimax[row];
      const T gamma = a / pmaxT;
      const T thr = KIND == kProxBox ? pw : gamma * pw;
      double num = 0.0, den = 0.0;
      for (int64_t i = threadIdx.x; i < nv; i += kBlock) {
        const int64_t e = base + lo + i * V;
        T vz[V], vzp[V], vxt[V], vps[V], vo[V];
        *reinterpret_cast<VT*>(vz) = *reinterpret_cast<const VT*>(z + e);
        *reinterpret_cast<VT*>(vzp) = *reinterpret_cast<const VT*>(zp + e);
        *reinterpret_cast<VT*>(vxt) = *reinterpret_cast<const VT*>(xt + e);
        *reinterpret_cast<VT*>(vps) = *reinterpret_cast<const VT*>(psi + e);
#pragma unroll
        for (int j = 0; j < V; ++j) vo[j] = sub_elem<T, KIND>(vz[j], vzp[j], vxt[j], vps[j], mom, pmaxT, thr, num, den);
        *reinterpret_cast<VT*>(zn + e) = *reinterpret_cast<VT*>(vo);
      }
      for (int64_t i = lo + nv * V + threadIdx.x; i < hi; i += kBlock) {
        const int64_t e = base + i;
        zn[e] = sub_elem<T, KIND>(z[e], zp[e], xt[e], psi[e], mom, pmaxT, thr, num, den);
      }
      const double s0 = cg_block_sum(num, sh);
      const double s1 = cg_block_sum(den, sh);
      if (threadIdx.x == 0) {
        part_cur[row * nb + blockIdx.x] = s0;
        part_cur[(rows + row) * nb + blockIdx.x] = s1;
      }
    }
  }
  // rows still running: workgroup 0 of every row adds its bit, the last of them to arrive publishes the total
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (running) __hip_atomic_fetch_add(counters, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int ticket = __hip_atomic_fetch_add(counters + 1, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket == (int)rows - 1) {
      const int total = __hip_atomic_exchange(counters, 0, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(counters + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      *nrun_host = (unsigned)total;
      __threadfence_system();
      __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

template <typename T>
inline bool row_vec_ok(int64_t rows, int64_t n) {
  return rows == 1 || n % kVecN<T> == 0;  // every row starts on a 16-byte boundary
}

template <typename T>
int launch_moments(int variant, int first, int64_t rows, int64_t n, double b1, double omb1, double b2, double omb2,
                   double eps_var, double c1, double c2, double eps_adam, double a, double p, const void* g,
                   const void* m, const void* v, const void* vhat, const void* x, void* m_out, void* v_out,
                   void* vhat_out, void* x_out, void* psi_out, void* work, hipStream_t st) {
  const int nb = blocks_per_row(rows, n);
  const dim3 grid((unsigned)nb, (unsigned)rows);
  MomArgs<T> A{(T)b1, (T)omb1, (T)b2, (T)omb2, (T)eps_var, (T)c1, (T)c2, (T)eps_adam, (T)a, (T)p, first ? 1 : 0,
               p == 0.5 ? 1 : 0};
  const bool vec = row_vec_ok<T>(rows, n) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(x) &&
                   (first || aligned16(vhat)) && aligned16(m_out) && aligned16(v_out) && aligned16(vhat_out) &&
                   aligned16(x_out) && (!psi_out || aligned16(psi_out));
  const int64_t chunk = pa_chunk<T>(n, nb);
  double* part_max = psi_out ? (double*)work : nullptr;
  auto go = [&](auto var) {
    hipLaunchKernelGGL((moments_kernel<T, decltype(var)::value>), grid, dim3(kBlock), 0, st, n, chunk, A, vec,
                       (const T*)g, (const T*)m, (const T*)v, (const T*)vhat, (const T*)x, (T*)m_out, (T*)v_out,
                       (T*)vhat_out, (T*)x_out, (T*)psi_out, part_max);
  };
  if (variant == kAdam)
    go(std::integral_constant<int, kAdam>{});
  else if (variant == kAmsgrad)
    go(std::integral_constant<int, kAmsgrad>{});
  else
    go(std::integral_constant<int, kPadam>{});
  return last_launch_status();
}

template <typename T>
int launch_sub(int kind, int k, int64_t rows, int64_t n, double mom, double eps, double a, double pw, const void* xt,
               const void* psi, const void* z_prev, const void* z, void* z_new, void* out, void* work,
               uint32_t* nrun_host, uint32_t* flag, uint32_t seq, hipStream_t st) {
  const int nb = blocks_per_row(rows, n);
  double* parts = (double*)work + rows * nb;
  const double* part_prev = parts + (size_t)((k - 1) & 1) * 2 * rows * nb;
  double* part_cur = parts + (size_t)(k & 1) * 2 * rows * nb;
  const double* psimax = (double*)work + PXA_PROXADAM_PLANES * rows * nb;
  int32_t* state = (int32_t*)(psimax + rows);
  int32_t* counters = state + rows;
  const dim3 grid((unsigned)nb, (unsigned)rows);
  const bool vec = row_vec_ok<T>(rows, n) && aligned16(xt) && aligned16(psi) && aligned16(z_prev) && aligned16(z) &&
                   aligned16(z_new) && aligned16(out);
  const int64_t chunk = pa_chunk<T>(n, nb);
  auto go = [&](auto kd) {
    hipLaunchKernelGGL((sub_step_kernel<T, decltype(kd)::value>), grid, dim3(kBlock), 0, st, rows, n, chunk, k, (T)mom,
                       eps, (T)a, (T)pw, vec, (const T*)xt, (const T*)psi, (const T*)z_prev, (const T*)z, (T*)z_new,
                       (T*)out, psimax, part_prev, part_cur, state, counters, (unsigned*)nrun_host, (unsigned*)flag,
                       (unsigned)seq);
  };
  switch (kind) {
    case kProxL1:
      go(std::integral_constant<int, kProxL1>{});
      break;
    case kProxPos:
      go(std::integral_constant<int, kProxPos>{});
      break;
    case kProxPosL1:
      go(std::integral_constant<int, kProxPosL1>{});
      break;
    default:
      go(std::integral_constant<int, kProxBox>{});
  }
  return last_launch_status();
}

}  // namespace
}  // namespace pxa

using namespace pxa;

extern "C" {

int pxa_proxadam_blocks(int64_t rows, int64_t n) { return rows > 0 && n > 0 ? blocks_per_row(rows, n) : 0; }

// planes of rows * nb doubles: the psi maxima, two pairs of RelError partials used alternately; then psimax per row,
// the per-row state words and the two counters
size_t pxa_proxadam_workspace_bytes(int64_t rows, int64_t n) {
  if (rows <= 0 || n <= 0) return 0;
  const size_t nb = (size_t)blocks_per_row(rows, n), r = (size_t)rows;
  return (PXA_PROXADAM_PLANES * r * nb + r) * sizeof(double) + (r + 2 + (r & 1)) * sizeof(int32_t);
}

int pxa_proxadam_moments(int dtype, int variant, int first, int64_t rows, int64_t n, double b1, double omb1, double b2,
                         double omb2, double eps_var, double c1, double c2, double eps_adam, double a, double p,
                         const void* g, const void* m, const void* v, const void* vhat, const void* x, void* m_out,
                         void* v_out, void* vhat_out, void* x_out, void* psi_out, void* work, void* stream) {
  PXA_CHECK_ARG(rows >= 1 && rows <= 65535 && n >= 1);
  PXA_CHECK_ARG(variant == kAdam || variant == kAmsgrad || variant == kPadam);
  PXA_CHECK_ARG(g && m && v && x && m_out && v_out && vhat_out && x_out && (first || vhat));
  PXA_CHECK_ARG(x_out != x && x_out != g && x_out != m_out && x_out != v_out && x_out != vhat_out);
  PXA_CHECK_ARG(!psi_out || work);
  PXA_CHECK_ARG(!psi_out || (psi_out != x_out && psi_out != m_out && psi_out != v_out && psi_out != vhat_out));
  hipStream_t st = as_stream(stream);
  PXA_DISPATCH(dtype, T, return launch_moments<T>(variant, first, rows, n, b1, omb1, b2, omb2, eps_var, c1, c2, eps_adam,
                                                   a, p, g, m, v, vhat, x, m_out, v_out, vhat_out, x_out, psi_out, work,
                                                   st));
}

int pxa_proxadam_sub_init(int64_t rows, int64_t n, void* work, void* stream) {
  PXA_CHECK_ARG(rows >= 1 && rows <= 65535 && n >= 1 && work);
  const int nb = blocks_per_row(rows, n);
  double* part_max = (double*)work;
  double* psimax = part_max + PXA_PROXADAM_PLANES * rows * nb;
  int32_t* state = (int32_t*)(psimax + rows);
  int32_t* counters = state + rows;
  const int per = kBlock / kWave;
  hipLaunchKernelGGL(sub_init_kernel, dim3((unsigned)((rows + per - 1) / per)), dim3(kBlock), 0, as_stream(stream), rows,
                     nb, part_max, psimax, state, counters);
  return last_launch_status();
}

int pxa_proxadam_sub_step(int dtype, int kind, int k, int64_t rows, int64_t n, double mom, double eps, double a,
                          double pw, const void* xt, const void* psi, const void* z_prev, const void* z, void* z_new,
                          void* out, void* work, uint32_t* nrun_host, uint32_t* flag, uint32_t seq, void* stream) {
  PXA_CHECK_ARG(rows >= 1 && rows <= 65535 && n >= 1 && k >= 1);
  PXA_CHECK_ARG(kind >= kProxL1 && kind <= kProxBox);
  PXA_CHECK_ARG(xt && psi && z_prev && z && z_new && out && work && nrun_host && flag);
  PXA_CHECK_ARG(z_new != z && z_new != z_prev && z_new != xt && z_new != psi && z_new != out);
  PXA_CHECK_ARG(out != z && out != z_prev && out != xt && out != psi);
  hipStream_t st = as_stream(stream);
  PXA_DISPATCH(dtype, T, return launch_sub<T>(kind, k, rows, n, mom, eps, a, pw, xt, psi, z_prev, z, z_new, out, work,
                                               nrun_host, flag, seq, st));
}

}  // extern "C"
