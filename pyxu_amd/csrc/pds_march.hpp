// Kernel D of the look-ahead PD3O / Condat-Vu step: the dual update of iteration k fused with the
// axis-0 march that opens iteration k + 1 (kernel A's job in the three-launch step of pds3d.hip).
//
// Iteration k ends with z_{k+1} = relax(fenchel_prox_h(z_k + sigma K w_k)) (kernel C); iteration k + 1
// starts with K^T z_{k+1}: PD3O builds v = x_{k+1} = prox_g(u_{k+1} - tau K^T z_{k+1}) and marches G0 v,
// Condat-Vu marches G0 x_{k+1} and kernel B needs K^T z_{k+1}.  Kernel D does both in one pass: at each
// plane of its march a thread updates z at its own position (stored) and recomputes z_{k+1} at the two
// in-plane backward neighbours K^T z needs (row - 1 for the axis-1 direction, column - 1 for the
// axis-2 one; the axis-0 neighbour is carried from the previous plane), so z_{k+1} is never re-read.
// It writes z_{k+1}, Q = G0 v and (PD3O) x_{k+1} or (Condat-Vu) K^T z_{k+1}.  DUAL = false is the
// first iteration's march (no dual update: z_{k+1} = z).
//
// Compulsory HBM traffic per voxel (fp32, R0 > 0): reads w, z (D fields), u or x; writes z, Q and x or
// K^T z: 40 B at D = 3, against kernel C (28 B) + kernel A (24 B PD3O / 8 B Condat-Vu) in the
// three-launch step.  Requires z_out != z: neighbours read z_k while other threads write z_{k+1}.
//
// One form of the kernel is kept, the one every measurement chose (C3 at 1024^3):
//  * one position per thread (occupancy 7 against 4 with two: profiles/r03z_pds_march_ring_ab.txt);
//  * one workgroup per work unit, dispatched as slots free up (a persistent grid marching in lockstep: kernel D
//    8.8 -> 11.0 ms, profiles/r05c_pds_march_persistent_ab.txt);
//  * the read-once / write-once streams (src, z_out, x_out or K^T z_out, Q) non-temporal, so that the re-read
//    neighbour rows of w and z stay in L2 (r04b: fetch 29 -> 25.7 B/voxel, PD3O step 15.3 -> 14.4 ms);
//  * every load of plane q + 1 issued before plane q is computed (r06ao: kernel D 8.78-8.84 -> 8.22-8.23 ms PD3O,
//    9.74-9.86 -> 8.24-8.25 ms Condat-Vu; two planes ahead no better, profiles/r06ap_pds_march_prefetch_ab.txt).
#pragma once
#include "pds3d.hpp"

namespace pxa {
namespace pds {

template <typename T>
struct PdsD {
  PdsA<T> a;  // march parameters: geometry, axis-0 taps, tau, prox, segments
  T sigma, lam, rho, omr;
};

// Every load of one plane of the dual march.  The march keeps two sets, so that each wave has two planes of loads
// in flight: plane qp + 1 is issued before plane qp is computed.
template <typename T>
struct PlaneLoads {
  T wf, w1, w2, zc[3];    // own position: w at plane + 1, row + 1, column + 1; z
  T rw, rz[3], rw0, rw2;  // row - 1 neighbour: w, z, w at plane + 1, w at column + 1
  T lw, lz[3], lw0, lw1;  // column - 1 neighbour: w, z, w at plane + 1, w at row + 1
  T u;                    // u (PD3O) or x (Condat-Vu)
};

// One work unit of kernel D: in-plane block `blk` (kAThreads consecutive positions, one per thread) of axis-0
// segment `segi` of volume `s`, marched over the segment's planes (+ the G0 halo planes).
template <typename T, int R0, bool PD3O, bool ISO, bool DUAL>
__device__ __forceinline__ void march_unit(const PdsD<T>& p, const T* __restrict__ w, const T* __restrict__ z,
                                           const T* __restrict__ src, T* __restrict__ zo, T* __restrict__ ao,
                                           T* __restrict__ q, unsigned blk, int segi, int64_t s) {
  constexpr int RING = 2 * R0 + 1;
  // kernel arguments copied to registers (the lambdas capture by reference; see pds_axis0_kernel)
  const PdsGeom<T> g = p.a.g;
  const T tau = p.a.tau, pw = p.a.pw;
  const int prox = p.a.prox;
  const T sigma = p.sigma, lam = p.lam, rho = p.rho, omr = p.omr;
  T k0[RING];
#pragma unroll
  for (int t = 0; t < RING; ++t) k0[t] = p.a.k0[t];
  const int n0 = g.n0, n1 = g.n1, n2 = g.n2;
  const int64_t M = (int64_t)n1 * n2;
  const int64_t j0 = (int64_t)blk * kAThreads + threadIdx.x;
  if (j0 >= M) return;  // no barriers below
  const int64_t N = M * n0;
  const int row = (int)(j0 / n2), col = (int)(j0 - (int64_t)row * n2);
  const T* ws = w + s * N + j0;
  const T* zs = z + s * g.D * N + j0;
  T* zw = zo + s * g.D * N + j0;
  const T* in = src + s * N + j0;
  T* aw = ao + s * N + j0;
  T* qw = q + s * N + j0;
  const int seg = p.a.seg;
  const int pb = segi * seg;
  const int pe = pb + seg < n0 ? pb + seg : n0;
  const int a_first = 3 - g.D;
  const bool row_nb = row + 1 < n1, col_nb = col + 1 < n2;

  // z_{k+1} (all directions; for aniso TV the unused ones are dead code) at one position, from its z (zc), its
  // w (wc) and w at its forward neighbour of each direction (wn)
  auto dual_at = [&](const T(&zc)[3], T wc, const T(&wn)[3], T(&n3)[3]) __attribute__((always_inline)) {
    T c3[3], i3[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (a < a_first) {
        c3[a] = i3[a] = T(0);
        continue;
      }
      c3[a] = zc[a];
      i3[a] = dual_in<T>(c3[a], wc, wn[a], g.c0[a], g.c1[a], sigma);
    }
    dual_out<T, ISO, PD3O>(c3, i3, a_first, lam, rho, omr, n3);
  };

  T wcar = T(0);  // DUAL: w at the next plane to process (own position), carried
  T zp0 = T(0);   // z_{k+1} of direction 0 at the previous plane (axis-0 backward neighbour of K^T z)
  const int f0 = pb - 2 * R0 > 0 ? pb - 2 * R0 : 0;  // first plane the march visits
  if constexpr (DUAL) {
    wcar = ws[(int64_t)f0 * M];
    if (g.D == 3 && f0 > 0) {
      const int64_t off = (int64_t)(f0 - 1) * M;
      const T wprev = ws[off];
      const T wn[3] = {wcar, row_nb ? ws[off + n2] : T(0), col_nb ? ws[off + 1] : T(0)};
      T zc[3], zt[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) zc[a] = a < a_first ? T(0) : zs[(int64_t)(a - a_first) * N + off];
      dual_at(zc, wprev, wn, zt);
      zp0 = zt[0];
    }
  } else {
    if (g.D == 3 && f0 > 0) zp0 = zs[(int64_t)(f0 - 1) * M];
  }

  // The tail of a plane (planes are visited in increasing order from f0), from z_{k+1} at the own position (zn),
  // of direction 1 at row - 1 (zr1) and of direction 2 at column - 1 (zl2): K^T z_{k+1} and v, stored on the
  // segment's own planes.  u = u (PD3O) or x (Condat-Vu) at the position.
  auto finish_v = [&](int qp, const T(&zn)[3], T zr1, T zl2, T u) __attribute__((always_inline)) -> T {
    const int64_t off = (int64_t)qp * M;
    const bool mine = qp >= pb && qp < pe;
    // K^T z_{k+1}: flipped 2-tap adjoint per direction, summed over directions in order
    // (pxa_gradient2_adjoint; the expression of pds_axis0_kernel and of kernel B's Condat-Vu epilogue)
    T kt;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (a < a_first) continue;
      const T zm = a == 0 ? zp0 : (a == 1 ? zr1 : zl2);
      const T term = kt_term<T>(g.c1[a], zm, g.c0[a], zn[a]);
      kt = (a == a_first) ? term : kt + term;
      if (a == 0) zp0 = zn[0];
    }
    if constexpr (PD3O) {
      const T one = T(1), mtau = -tau;
      const T v = apply_prox<T>(prox, fma(mtau, kt, one * u), pw);
      if (mine) __builtin_nontemporal_store(v, aw + off);
      return v;
    } else {
      if (mine) __builtin_nontemporal_store(kt, aw + off);
      return u;
    }
  };

  // DUAL = false, the priming march: z_{k+1} = z, read where the dual march computes it
  auto primed_v = [&](int qp) __attribute__((always_inline)) -> T {
    const int64_t off = (int64_t)qp * M;
    T zn[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (a < a_first) continue;
      zn[a] = zs[(int64_t)(a - a_first) * N + off];
    }
    const T zr1 = a_first <= 1 && row > 0 ? zs[(int64_t)(1 - a_first) * N + off - n2] : T(0);
    const T zl2 = col > 0 ? zs[(int64_t)(2 - a_first) * N + off - 1] : T(0);
    return finish_v(qp, zn, zr1, zl2, __builtin_nontemporal_load(in + off));
  };

  // DUAL = true: the loads of plane qp, then the plane from them
  auto issue = [&](int qp, PlaneLoads<T>& L) __attribute__((always_inline)) {
    const int64_t off = (int64_t)qp * M;
    L.wf = qp + 1 < n0 ? ws[off + M] : T(0);
    L.w1 = row_nb ? ws[off + n2] : T(0);
    L.w2 = col_nb ? ws[off + 1] : T(0);
#pragma unroll
    for (int a = 0; a < 3; ++a) L.zc[a] = a < a_first ? T(0) : zs[(int64_t)(a - a_first) * N + off];
    if (a_first <= 1 && row > 0) {
      const int64_t o = off - n2;
      L.rw = ws[o];
#pragma unroll
      for (int a = 0; a < 3; ++a) L.rz[a] = a < a_first ? T(0) : zs[(int64_t)(a - a_first) * N + o];
      L.rw0 = qp + 1 < n0 ? ws[o + M] : T(0);
      L.rw2 = col_nb ? ws[o + 1] : T(0);
    }
    if (col > 0) {
      const int64_t o = off - 1;
      L.lw = ws[o];
#pragma unroll
      for (int a = 0; a < 3; ++a) L.lz[a] = a < a_first ? T(0) : zs[(int64_t)(a - a_first) * N + o];
      L.lw0 = qp + 1 < n0 ? ws[o + M] : T(0);
      L.lw1 = row_nb ? ws[o + n2] : T(0);
    }
    L.u = __builtin_nontemporal_load(in + off);
  };
  auto dual_v = [&](int qp, const PlaneLoads<T>& L) __attribute__((always_inline)) -> T {
    const int64_t off = (int64_t)qp * M;
    const T wc = wcar;
    wcar = L.wf;
    T zn[3], n3[3];
    {
      const T wn[3] = {L.wf, L.w1, L.w2};
      dual_at(L.zc, wc, wn, zn);
    }
    // the forward neighbour of row - 1 along direction 1, and of column - 1 along direction 2, is the own position
    T zr1 = T(0), zl2 = T(0);
    if (a_first <= 1 && row > 0) {
      const T wn[3] = {L.rw0, wc, L.rw2};
      dual_at(L.rz, L.rw, wn, n3);
      zr1 = n3[1];
    }
    if (col > 0) {
      const T wn[3] = {L.lw0, L.lw1, wc};
      dual_at(L.lz, L.lw, wn, n3);
      zl2 = n3[2];
    }
    if (qp >= pb && qp < pe) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        if (a < a_first) continue;
        __builtin_nontemporal_store(zn[a], zw + (int64_t)(a - a_first) * N + off);
      }
    }
    return finish_v(qp, zn, zr1, zl2, L.u);
  };

  if constexpr (R0 == 0) {
    // no G0 march (2-D images: one plane per thread): a plane's loads are issued with its own arithmetic, as before
    // the non-prefetching plane body was removed; a plane ahead measured slower there
    // (profiles/pds_variants_pruned_ab.txt, scripts/pds_la_probe.py)
    for (int qp = pb; qp < pe; ++qp) {
      if constexpr (DUAL) {
        PlaneLoads<T> cur;
        issue(qp, cur);
        (void)dual_v(qp, cur);
      } else {
        (void)primed_v(qp);
      }
    }
  } else {
    T rv[RING], rh[RING];
#pragma unroll
    for (int r = 0; r < RING; ++r) rv[r] = rh[r] = T(0);
    const int first = pb - 2 * R0, last = pe - 1 + 2 * R0;
    // Q = G0 v (the plain two-pass form of pds_axis0_kernel, same taps in the same order) with the two
    // windows held as shift registers: one copy of the plane body.  rv[t] = v at plane qp - 2 R0 + t;
    // rh[t] = (H0 v) at plane qp - 3 R0 + t.  (Static ring slots as in pds_axis0_kernel, i.e. the plane
    // body unrolled RING times, measured no faster: profiles/r03z_pds_march_ring_ab.txt.)
    PlaneLoads<T> cur, nxt;  // (DUAL only; the plane loop below is shared with the priming march)
    if constexpr (DUAL) {
      const int q0 = first < 0 ? 0 : first;
      if (q0 < n0 && q0 <= last) issue(q0, cur);
    }
#pragma unroll 1
    for (int qp = first; qp <= last; ++qp) {
#pragma unroll
      for (int t = 0; t + 1 < RING; ++t) rv[t] = rv[t + 1];
      if (qp >= 0 && qp < n0) {
        if constexpr (DUAL) {
          if (qp + 1 < n0 && qp + 1 <= last) issue(qp + 1, nxt);  // in flight while this plane is computed
          rv[RING - 1] = dual_v(qp, cur);
          cur = nxt;
        } else {
          rv[RING - 1] = primed_v(qp);
        }
      } else {
        rv[RING - 1] = T(0);
      }
      // (H0 v)[qp - R0] = sum_t k0[t] v[qp - 2 R0 + t]; zero outside [0, n0) (Trim o S o Pad)
      const int ph = qp - R0;
      T h = T(0);
      if (ph >= 0 && ph < n0) {
#pragma unroll
        for (int t = 0; t < RING; ++t) h = fma(k0[t], rv[t], h);
      }
#pragma unroll
      for (int t = 0; t + 1 < RING; ++t) rh[t] = rh[t + 1];
      rh[RING - 1] = h;
      // Q[i] = sum_t k0[t] (H0 v)[i + R0 - t],  i = qp - 2 R0
      const int i = qp - 2 * R0;
      if (i >= pb) {
        T acc = T(0);
#pragma unroll
        for (int t = 0; t < RING; ++t) acc = fma(k0[t], rh[2 * R0 - t], acc);
        __builtin_nontemporal_store(acc, qw + (int64_t)i * M);
      }
    }
  }
}

// One workgroup per work unit.  Units are numbered (volume, segment, in-plane block) with the block fastest and
// the block index XCD-banded (tile2d::xcd_tile), so that the row - 1 / row + 1 neighbours of w and z are usually
// read from the L2 of the same XCD.
template <typename T, int R0, bool PD3O, bool ISO, bool DUAL>
__global__ void __launch_bounds__(kAThreads) pds_march_kernel(PdsD<T> p, const T* __restrict__ w,
                                                              const T* __restrict__ z, const T* __restrict__ src,
                                                              T* __restrict__ zo, T* __restrict__ ao,
                                                              T* __restrict__ q, unsigned blocks, unsigned nseg) {
  const unsigned r = blockIdx.x % blocks, rest = blockIdx.x / blocks;
  march_unit<T, R0, PD3O, ISO, DUAL>(p, w, z, src, zo, ao, q, xcd_tile(r, blocks), (int)(rest % nseg),
                                     (int64_t)(rest / nseg));
}

// ------------------------------------------------------------------ host side
template <typename T, int R0, bool PD3O, bool ISO, bool DUAL>
int launch_d(const PdsD<T>& pd, int64_t M, int nseg, const void* w, const void* z, const void* src, void* zo,
             void* ao, void* q, hipStream_t st) {
  const int64_t blocks = (M + kAThreads - 1) / kAThreads;
  const int64_t units = blocks * nseg * pd.a.g.stack;
  PXA_CHECK_ARG(units <= 0x7fffffff);
  hipLaunchKernelGGL((pds_march_kernel<T, R0, PD3O, ISO, DUAL>), dim3((unsigned)units), dim3(kAThreads), 0, st, pd,
                     (const T*)w, (const T*)z, (const T*)src, (T*)zo, (T*)ao, (T*)q, (unsigned)blocks,
                     (unsigned)nseg);
  return last_launch_status();
}

// kernel D of axis-0 radius R0 (0 .. 8); dual = false is the priming march (ISO irrelevant: one instantiation)
template <typename T>
int dispatch_d(const PdsD<T>& pd, bool pd3o, bool iso, bool dual, int R0, int64_t M, int nseg, const void* w,
               const void* z, const void* src, void* zo, void* ao, void* q, hipStream_t st) {
  auto go = [&](auto p, auto i, auto u) {
    return with_radius<0>(R0, [&](auto r) {
      return launch_d<T, decltype(r)::value, decltype(p)::value, decltype(i)::value, decltype(u)::value>(
          pd, M, nseg, w, z, src, zo, ao, q, st);
    });
  };
  if (!dual) return with_bool(pd3o, [&](auto p) { return go(p, std::false_type{}, std::false_type{}); });
  return with_bool(pd3o, [&](auto p) { return with_bool(iso, [&](auto i) { return go(p, i, std::true_type{}); }); });
}

// run_d: instantiated per dtype in pds_d_f32.hip / pds_d_f64.hip
#define PXA_PDS_RUN_D(T)                                                                                \
  int run_d(const PdsD<T>& pd, bool pd3o, bool iso, bool dual, int R0, int64_t M, int nseg, const void* w, \
            const void* z, const void* src, void* zo, void* ao, void* q, hipStream_t st)
PXA_PDS_RUN_D(float);
PXA_PDS_RUN_D(double);

}  // namespace pds
}  // namespace pxa
