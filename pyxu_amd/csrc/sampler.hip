// Langevin samplers (experimental/sampler/_sampler.py:105-488, statistics.py:126-171): everything of a ULA / MYULA step
// after grad f, and the Welford update of the online centred moments, as streaming kernels.
//   philox_normal   standard normals from Philox4x32-10 keyed by (seed, step, global element): counter = (group lo,
//                   group hi, step lo, step hi), key = (seed lo, seed hi); one counter gives one group of 16 bytes of
//                   normals by Box-Muller with the accurate log / sincospi (4 f32 from two pairs of words, 2 f64 from
//                   two 53-bit uniforms)
//   langevin_step   x' = (x - gamma (grad + m)) + sqrt(2 gamma) z with m the Moreau-Yosida gradient of an element-wise
//                   g and z read from memory or made in registers: 3 array streams with device noise, 4 with supplied
//   online_moments  sample k folded into the mean (T) and the order - 1 planes of double corrected sums
// Work is split by GLOBAL group: thread i of the grid-stride loop owns group e0 / G + i, whatever the buffer holds of it.
// A group that lies wholly inside the buffer is moved by 16-byte accesses when the host found every operand aligned at
// group boundaries; otherwise, and for the first and last group of a range that starts or ends inside one, element by
// element.  The arithmetic per element is one function for both, and nothing here is contracted into an FMA: the
// paths, any e0 and any n give the same bits.
#include "common.hpp"

#pragma clang fp contract(off)

namespace pxa {
namespace {

constexpr int kNone = 0, kProxL1 = PXA_PROX_L1, kProxPos = PXA_PROX_POS, kProxPosL1 = PXA_PROX_POSL1, kProxBox = PXA_PROX_BOX;

struct Words {
  uint32_t w[4];
};

__device__ inline Words philox4x32_10(uint64_t group, uint64_t step, uint64_t seed) {
  uint32_t c0 = (uint32_t)group, c1 = (uint32_t)(group >> 32), c2 = (uint32_t)step, c3 = (uint32_t)(step >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0;
    c1 = lo1;
    c2 = n2;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Words{{c0, c1, c2, c3}};
}

// the normals of one group: z[0 .. kVecN<T>)
__device__ inline void group_normals(uint64_t group, uint64_t step, uint64_t seed, float* z) {
  const Words r = philox4x32_10(group, step, seed);
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float u1 = (float)((r.w[2 * p] >> 8) + 1u) * 0x1p-24f;  // (0, 1], exact
    const float a = (float)(r.w[2 * p + 1] >> 8) * 0x1p-23f;      // 2 u2 in [0, 2), exact
    const float rad = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincospif(a, &s, &c);
    z[2 * p] = rad * c;
    z[2 * p + 1] = rad * s;
  }
}

__device__ inline void group_normals(uint64_t group, uint64_t step, uint64_t seed, double* z) {
  const Words r = philox4x32_10(group, step, seed);
  const uint64_t b1 = ((uint64_t)r.w[0] << 32 | r.w[1]) >> 11, b2 = ((uint64_t)r.w[2] << 32 | r.w[3]) >> 11;
  const double u1 = (double)(b1 + 1u) * 0x1p-53;  // (0, 1], exact
  const double a = (double)b2 * 0x1p-52;          // 2 u2 in [0, 2), exact
  const double rad = sqrt(-2.0 * log(u1));
  double s, c;
  sincospi(a, &s, &c);
  z[0] = rad * c;
  z[1] = rad * s;
}

// The part of global group g0 + i a buffer of n elements starting at global element e0 = G g0 + ph holds: local
// indices [l0, l0 + G) cut to [0, n).
template <typename T>
struct GroupRange {
  int64_t l0;
  bool whole;
  __device__ GroupRange(int64_t i, int ph, int64_t n) : l0(i * kVecN<T> - ph), whole(l0 >= 0 && l0 + kVecN<T> <= n) {}
};

template <typename T>
__global__ void __launch_bounds__(kBlock) normal_kernel(int64_t n, int64_t ngroups, uint64_t seed, uint64_t step,
                                                        uint64_t g0, int ph, bool vec, T* __restrict__ out) {
  constexpr int V = kVecN<T>;
  using VT = typename Vec4<T>::type;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ngroups; i += stride) {
    T z[V];
    group_normals(g0 + (uint64_t)i, step, seed, z);
    const GroupRange<T> gr(i, ph, n);
    if (vec && gr.whole) {
      *reinterpret_cast<VT*>(out + gr.l0) = *reinterpret_cast<VT*>(z);
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const int64_t l = gr.l0 + j;
        if (l >= 0 && l < n) out[l] = z[j];
      }
    }
  }
}

template <typename T>
struct StepArgs {
  T gamma, c, lam, t, pw;
};

// numpy.clip / numpy.minimum: a NaN operand stays
template <typename T>
__device__ inline T clip_sym(T x, T t) {
  return x < -t ? -t : (x > t ? t : x);
}

template <typename T, int KIND>
__device__ inline T step_elem(const StepArgs<T>& A, T x, T g, T z) {
  T gt = g;
  if (KIND != kNone) {
    T m;
    if (KIND == kProxL1)
      m = clip_sym(x, A.t);
    else if (KIND == kProxPos)
      m = x > T(0) ? T(0) : x;
    else if (KIND == kProxPosL1)
      m = x > A.t ? A.t : x;
    else
      m = x - clip_sym(x, A.pw);
    m = m / A.lam;
    gt = g + m;
  }
  const T gs = A.gamma * gt;
  const T d = x - gs;
  const T cz = A.c * z;
  return d + cz;
}

// x_out may be x (element i is read and written by one thread): no __restrict__ on the two
template <typename T, int KIND, bool DEVNOISE>
__global__ void __launch_bounds__(kBlock) step_kernel(int64_t n, int64_t ngroups, StepArgs<T> A, uint64_t seed,
                                                      uint64_t step, uint64_t g0, int ph, bool vec, const T* x,
                                                      const T* __restrict__ grad, const T* __restrict__ noise,
                                                      T* x_out) {
  constexpr int V = kVecN<T>;
  using VT = typename Vec4<T>::type;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ngroups; i += stride) {
    T z[V];
    if (DEVNOISE) group_normals(g0 + (uint64_t)i, step, seed, z);
    const GroupRange<T> gr(i, ph, n);
    if (vec && gr.whole) {
      T vx[V], vg[V], vo[V];
      *reinterpret_cast<VT*>(vx) = *reinterpret_cast<const VT*>(x + gr.l0);
      *reinterpret_cast<VT*>(vg) = *reinterpret_cast<const VT*>(grad + gr.l0);
      if (!DEVNOISE) *reinterpret_cast<VT*>(z) = *reinterpret_cast<const VT*>(noise + gr.l0);
#pragma unroll
      for (int j = 0; j < V; ++j) vo[j] = step_elem<T, KIND>(A, vx[j], vg[j], z[j]);
      *reinterpret_cast<VT*>(x_out + gr.l0) = *reinterpret_cast<VT*>(vo);
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const int64_t l = gr.l0 + j;
        if (l >= 0 && l < n) x_out[l] = step_elem<T, KIND>(A, x[l], grad[l], DEVNOISE ? z[j] : noise[l]);
      }
    }
  }
}

template <typename T>
struct MomArgs {
  T kT, kp1, ratio;  // k, k + 1 and k / (k + 1) (the quotient formed in double), each cast to T
  double kd;
};

// statistics.py:159-168 for one element: S[r - 2] is the corrected sum of order r
template <typename T, int ORDER>
__device__ inline void moment_elem(const MomArgs<T>& A, T x, T& mean, double* S) {
  const T temp = (x - mean) / A.kp1;
  const double a = (double)(-temp), b = (double)(A.kT * temp);
  const double a2 = a * a, b2 = b * b;
  if (ORDER >= 4) {
    const double a4 = a2 * a2, b4 = b2 * b2;
    S[2] += (6.0 * S[0]) * a2;
    S[2] += (4.0 * S[1]) * a;
    S[2] += A.kd * a4;
    S[2] += b4;
  }
  if (ORDER >= 3) {
    const double a3 = a2 * a, b3 = b2 * b;
    S[1] += (3.0 * S[0]) * a;
    S[1] += A.kd * a3;
    S[1] += b3;
  }
  S[0] += A.kd * a2;
  S[0] += b2;
  const T xs = x / A.kp1;
  mean = mean * A.ratio;
  mean = mean + xs;
}

template <typename T, int ORDER>
__global__ void __launch_bounds__(kBlock) moments_kernel(int64_t n, bool first, MomArgs<T> A, bool vec,
                                                         const T* __restrict__ x, T* __restrict__ mean,
                                                         double* __restrict__ sums) {
  constexpr int V = kVecN<T>, P = ORDER - 1;
  using VT = typename Vec4<T>::type;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nv = vec ? n / V : 0;
  for (int64_t i = tid; i < nv; i += stride) {
    const int64_t e = i * V;
    T vx[V], vm[V];
    double S[V][P];
    *reinterpret_cast<VT*>(vx) = *reinterpret_cast<const VT*>(x + e);
    if (!first) {
      *reinterpret_cast<VT*>(vm) = *reinterpret_cast<const VT*>(mean + e);
#pragma unroll
      for (int p = 0; p < P; ++p)
#pragma unroll
        for (int q = 0; q < V; q += 2) {
          const double2 v = *reinterpret_cast<const double2*>(sums + p * n + e + q);
          S[q][p] = v.x;
          S[q + 1][p] = v.y;
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (first) {
        vm[j] = vx[j];
#pragma unroll
        for (int p = 0; p < P; ++p) S[j][p] = 0.0;
      } else {
        moment_elem<T, ORDER>(A, vx[j], vm[j], S[j]);
      }
    }
    *reinterpret_cast<VT*>(mean + e) = *reinterpret_cast<VT*>(vm);
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
      for (int q = 0; q < V; q += 2)
        *reinterpret_cast<double2*>(sums + p * n + e + q) = make_double2(S[q][p], S[q + 1][p]);
  }
  for (int64_t e = nv * V + tid; e < n; e += stride) {
    T m;
    double S[P];
    if (first) {
      m = x[e];
#pragma unroll
      for (int p = 0; p < P; ++p) S[p] = 0.0;
    } else {
      m = mean[e];
#pragma unroll
      for (int p = 0; p < P; ++p) S[p] = sums[p * n + e];
      moment_elem<T, ORDER>(A, x[e], m, S);
    }
    mean[e] = m;
#pragma unroll
    for (int p = 0; p < P; ++p) sums[p * n + e] = S[p];
  }
}

// every operand sits on a 16-byte boundary at the start of a group: `ph` elements before its first one
template <typename T>
inline bool group_aligned(const void* p, int ph) {
  return (((uintptr_t)p - (uintptr_t)ph * sizeof(T)) & 15u) == 0;
}

template <typename T>
int launch_normal(int64_t n, uint64_t seed, uint64_t step, uint64_t e0, void* out, hipStream_t st) {
  constexpr int V = kVecN<T>;
  const int ph = (int)(e0 % V);
  const int64_t ngroups = (n + ph + V - 1) / V;
  hipLaunchKernelGGL((normal_kernel<T>), dim3(grid_for(ngroups)), dim3(kBlock), 0, st, n, ngroups, seed, step, e0 / V,
                     ph, group_aligned<T>(out, ph), (T*)out);
  return last_launch_status();
}

template <typename T, bool DEVNOISE>
int launch_step(int kind, int64_t n, double gamma, double lam, double pw, uint64_t seed, uint64_t step, uint64_t e0,
                const void* x, const void* grad, const void* noise, void* x_out, hipStream_t st) {
  constexpr int V = kVecN<T>;
  const int ph = DEVNOISE ? (int)(e0 % V) : 0;  // supplied noise: groups are counted from the buffer's start
  const int64_t ngroups = (n + ph + V - 1) / V;
  const T gT = (T)gamma;
  const StepArgs<T> A{gT, (T)sqrt(2.0 * (double)gT), (T)lam, (T)(lam * pw), (T)pw};
  const bool vec = group_aligned<T>(x, ph) && group_aligned<T>(grad, ph) && group_aligned<T>(x_out, ph) &&
                   (DEVNOISE || group_aligned<T>(noise, ph));
  auto go = [&](auto kd) {
    hipLaunchKernelGGL((step_kernel<T, decltype(kd)::value, DEVNOISE>), dim3(grid_for(ngroups)), dim3(kBlock), 0, st, n,
                       ngroups, A, seed, step, DEVNOISE ? e0 / V : 0, ph, vec, (const T*)x, (const T*)grad,
                       (const T*)noise, (T*)x_out);
  };
  switch (kind) {
    case kNone:
      go(std::integral_constant<int, kNone>{});
      break;
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

template <typename T>
int launch_moments(int order, int64_t k, int64_t n, const void* x, void* mean, double* sums, hipStream_t st) {
  constexpr int V = kVecN<T>;
  const MomArgs<T> A{(T)k, (T)(k + 1), (T)((double)k / (double)(k + 1)), (double)k};
  // a vector of T spans V doubles of every plane: the planes, n doubles apart, all start on a 16-byte boundary
  const bool vec = aligned16(x) && aligned16(mean) && aligned16(sums) && (order == 2 || n % 2 == 0);
  const dim3 grid(grid_for((n + V - 1) / V));
  auto go = [&](auto od) {
    hipLaunchKernelGGL((moments_kernel<T, decltype(od)::value>), grid, dim3(kBlock), 0, st, n, k == 0, A, vec,
                       (const T*)x, (T*)mean, sums);
  };
  if (order == 2)
    go(std::integral_constant<int, 2>{});
  else if (order == 3)
    go(std::integral_constant<int, 3>{});
  else
    go(std::integral_constant<int, 4>{});
  return last_launch_status();
}

inline bool range_ok(int64_t n, uint64_t e0) { return n >= 0 && e0 <= UINT64_MAX - (uint64_t)n - 16; }

}  // namespace
}  // namespace pxa

using namespace pxa;

extern "C" {

int pxa_philox_normal(int dtype, int64_t n, uint64_t seed, uint64_t step, uint64_t e0, void* out, void* stream) {
  PXA_CHECK_ARG(range_ok(n, e0));
  if (n == 0) return PXA_OK;
  PXA_CHECK_ARG(out);
  hipStream_t st = as_stream(stream);
  PXA_DISPATCH(dtype, T, return launch_normal<T>(n, seed, step, e0, out, st));
}

int pxa_langevin_step(int dtype, int kind, int64_t n, double gamma, double lam, double pw, uint64_t seed, uint64_t step,
                      uint64_t e0, const void* x, const void* grad, const void* noise, void* x_out, void* stream) {
  PXA_CHECK_ARG(range_ok(n, e0) && kind >= kNone && kind <= kProxBox);
  PXA_CHECK_ARG(gamma > 0 && (kind == kNone || lam > 0));
  if (n == 0) return PXA_OK;
  PXA_CHECK_ARG(x && grad && x_out && x_out != grad && x_out != noise);
  hipStream_t st = as_stream(stream);
  if (noise) {
    PXA_DISPATCH(dtype, T,
                 return (launch_step<T, false>(kind, n, gamma, lam, pw, seed, step, e0, x, grad, noise, x_out, st)));
  }
  PXA_DISPATCH(dtype, T,
               return (launch_step<T, true>(kind, n, gamma, lam, pw, seed, step, e0, x, grad, nullptr, x_out, st)));
}

int pxa_online_moments(int dtype, int order, int64_t k, int64_t n, const void* x, void* mean, double* sums,
                       void* stream) {
  PXA_CHECK_ARG(order >= 2 && order <= 4 && k >= 0 && n >= 0);
  if (n == 0) return PXA_OK;
  PXA_CHECK_ARG(x && mean && sums && x != mean);
  hipStream_t st = as_stream(stream);
  PXA_DISPATCH(dtype, T, return launch_moments<T>(order, k, n, x, mean, sums, st));
}

}  // extern "C"
