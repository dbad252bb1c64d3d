// Fused primal-dual splitting iterations (PD3O, Condat-Vu) for TV-regularised deblurring of 2-D
// images and 3-D volumes: three launches per iteration instead of the reference's ~25 array passes.
//
// Problem:  f = 1/2 ||S . - y||^2 with S a separable zero-boundary
// stencil (Gaussian / Convolve / Stencil, operator/linop/stencil/stencil.py:441-461), K = Grad
// (forward differences over the D trailing axes, diff.py:1113-1265), h = lam L1 (anisotropic TV) or
// lam L21 over the D directions (isotropic TV), g in {None, PositiveOrthant, lam L1}.
//
// PD3O.m_step (opt/solver/pds.py:747-761):
//   x      = prox_g(u - tau K^T z)                            kernel A (with the axis-0 half of G x)
//   u_tmp  = x - tau grad f(x),  grad f(x) = G x - S^T y      kernel B (in-plane half of G x + update)
//   w      = x + u_tmp - u ;  u = (1 - rho) u + rho u_tmp     kernel B
//   z      = (1 - rho) z + rho fenchel_prox_h(z + sigma K w)  kernel C
// CondatVu.m_step (pds.py:429-442):
//   x_tmp  = prox_g(x - tau grad f(x) - tau K^T z)            kernels A (axis 0 of G x) + B
//   w      = 2 x_tmp - x ;  x = rho x_tmp + (1 - rho) x       kernel B
//   z      = rho fenchel_prox_h(z + sigma K w) + (1 - rho) z  kernel C
//
// G = S^T S is separable: G = G0 (x) G1 (x) G2 with G_a = H_a^T H_a (H_a the zero-boundary 1-D
// correlation of axis a), so G x is evaluated as G12 (G0 x):
//  * kernel A marches each pixel column along axis 0 and keeps the H0 and H0^T windows in two
//    register rings (2 R0 + 1 planes each): the plain two-pass form, exact at the boundary planes,
//    one HBM read of the input per voxel.  PD3O builds its input x = prox_g(u - tau K^T z) on the fly
//    (and stores it: x is the iterate the solver returns); Condat-Vu reads x.
//  * kernel B is the LDS-tiled in-plane normal-operator sweep of pgd_tv2d.hip (tile2d.hpp: two
//    register-blocked 4R+1-tap passes with exact boundary-row corrections) over every plane, with the
//    solver's point-wise update fused into its epilogue.
//  * kernel C is the dual update: K w (one forward neighbour per direction, from cache), fenchel_prox
//    (operator.py:905-944) as the projection onto the lam-ball of the dual norm that its Moreau form
//    equals (pds3d.hpp dual_out), and the relaxation.
//  * pxa_pds_step_la replaces kernels C and A by kernel D (pds_march.hpp): the dual update of iteration k
//    fused with the axis-0 march of iteration k + 1, two launches per iteration.
//  * pxa_pds_slab_primal (kernels A, B) + pxa_pds_slab_dual (kernel C) evaluate the three-launch step on one
//    rank's slab of axis-0 planes of a volume split over several devices: the state arrays are the compact slab,
//    the planes beyond it (2 R0 per side for the march, one lo plane of z_0, one hi plane of w) are read from
//    ghost buffers filled by the neighbours, a null ghost is the volume's edge.  The plane index of kernels A and
//    C is uniform per march step, so ghost or owned is a choice of base pointer; the ghost-aware forms are
//    separate instantiations (GhostA / PdsPtrsSlab / GhostC; pds_slab_f32.hip, pds_slab_f64.hip), and the
//    unsharded launches keep their code.  Same expressions per voxel: the bits of pxa_pds_step.
// Host side, one path for the five entry points: pds_setup (algorithm, make_geom, tap windows, scalars), step_arrays
// and the entry's own conditions, then the stages -- pxa_pds_step: stage_a, stage_b, run_c; pxa_pds_slab_primal: its
// ghost checks, stage_a with a GhostA, stage_b; pxa_pds_step_la: run_d (priming), stage_b, run_d.  pxa_tv_dual_update
// and pxa_pds_slab_dual are dual_entry (make_geom + run_c) without and with a GhostC.
// Compulsory HBM traffic per voxel (fp32): PD3O A 24 B + B 24 B + C 28 B = 76 B (80 B);
// Condat-Vu A 8 B + B 32 B + C 28 B = 68 B (SURVEY: 68 B).
//
// Parity: the step follows the reference's arithmetic per voxel except that G x replaces
// S^T (S x - y) + ... (same operator, different fp32 rounding order: see pgd_tv2d.hip).
#include "pds_march.hpp"

namespace pxa {
namespace pds {

// ------------------------------------------------------------------ kernel C: dual update
template <typename T>
struct PdsC {
  PdsGeom<T> g;
  T sigma, lam, rho, omr;
  int seg;               // planes per axis-0 segment
};

template <typename T, int NV>
__device__ inline void ldv(const T* p, T (&v)[NV]) {
  if constexpr (NV == kVecN<T>)
    *reinterpret_cast<typename Vec4<T>::type*>(v) = *reinterpret_cast<const typename Vec4<T>::type*>(p);
  else
    v[0] = p[0];
}

// Thread = NV consecutive in-plane positions of one row; it marches the planes of its segment, so the
// axis-0 forward neighbour w(p + 1) is loaded once and carried to the next step.  The in-plane block
// index is XCD-banded (tile2d::xcd_tile) so that the row+1 neighbour is usually read from the L2 of the
// same XCD, where the neighbouring block marches in step.
// PF (the default; PXA_TUNE_DUAL_ROWS = 1 turns it off): z and the row + 1 / column + 1 neighbours of plane p + 1 are
// loaded while plane p is computed (two planes of loads in flight per thread); the same values in the same expressions:
// the same bits.
// GH = GhostC<T> (pxa_pds_slab_dual): the n0 planes are one rank's slab, and w at plane n0 is plane 0 of w_hi, the
// next slab's first planes as (stack, dhi, n1, n2); null: the volume's edge.  The plane index is uniform over the
// workgroup: a choice of base pointer.
template <typename T>
struct GhostC {
  const T* w_hi;
  int64_t dhi;
};

template <typename T, int NV, bool ISO, bool PD3O, bool NT, bool PF = false, typename GH = NoGhost>
__global__ void __launch_bounds__(kBlock) pds_dual_kernel(PdsC<T> p, const T* __restrict__ w,
                                                          const T* __restrict__ z, T* __restrict__ zo, GH gh = GH()) {
  constexpr bool SLAB = !std::is_same<GH, NoGhost>::value;
  const PdsGeom<T> g = p.g;
  const T sigma = p.sigma, lam = p.lam, rho = p.rho, omr = p.omr;
  const int n0 = g.n0, n1 = g.n1, n2 = g.n2, D = g.D;
  const int64_t M = (int64_t)n1 * n2, N = M * n0;
  const int a_first = 3 - D;
  const unsigned blk = xcd_tile(blockIdx.x, gridDim.x);
  const int64_t j0 = ((int64_t)blk * kBlock + threadIdx.x) * NV;
  if (j0 >= M) return;  // no barriers below
  const int r = (int)(j0 / n2), c = (int)(j0 - (int64_t)r * n2);
  const int64_t s = blockIdx.z;
  const int pb = blockIdx.y * p.seg;
  const int pe = pb + p.seg < n0 ? pb + p.seg : n0;
  const T* ws = w + s * N + j0;
  const T* zs = z + s * (int64_t)D * N + j0;
  T* zos = zo + s * (int64_t)D * N + j0;
  const bool row_nb = r + 1 < n1, col_nb = c + NV < n2;
  T wn0[NV];  // w at the current plane (carried from the previous step)
  ldv<T, NV>(ws + (int64_t)pb * M, wn0);
  // PF: the next plane's z, w row + 1 and w column + 1 (the loads below, one plane early)
  T fz[3][NV], fr[NV], fcol;
  auto fetch = [&](int pl) {
    const int64_t off = (int64_t)pl * M;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      if (ax < a_first) continue;
      if (NT)
        ldn_nt<T, NV>(zs + (int64_t)(ax - a_first) * N + off, fz[ax]);
      else
        ldv<T, NV>(zs + (int64_t)(ax - a_first) * N + off, fz[ax]);
    }
    if (row_nb) {
      ldv<T, NV>(ws + off + n2, fr);
    } else {
#pragma unroll
      for (int e = 0; e < NV; ++e) fr[e] = T(0);
    }
    fcol = col_nb ? ws[off + NV] : T(0);
  };
  if (PF) fetch(pb);
  for (int pl = pb; pl < pe; ++pl) {
    const int64_t off = (int64_t)pl * M;
    T wc[NV], wp[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) wc[e] = wn0[e];
    bool ghost = false;
    if constexpr (SLAB) ghost = pl + 1 == n0 && gh.w_hi != nullptr;
    if (pl + 1 < n0) {
      ldv<T, NV>(ws + off + M, wp);
    } else if (ghost) {
      if constexpr (SLAB) ldv<T, NV>(gh.w_hi + s * gh.dhi * M + j0, wp);
    } else {
#pragma unroll
      for (int e = 0; e < NV; ++e) wp[e] = T(0);
    }
    T cz[3][NV], cr[NV], ccol = T(0);
    if (PF) {
#pragma unroll
      for (int ax = 0; ax < 3; ++ax)
#pragma unroll
        for (int e = 0; e < NV; ++e) cz[ax][e] = fz[ax][e];
#pragma unroll
      for (int e = 0; e < NV; ++e) cr[e] = fr[e];
      ccol = fcol;
      if (pl + 1 < pe) fetch(pl + 1);
    }
    T zin[3][NV], zc[3][NV];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      if (ax < a_first) continue;
      T wn[NV];
      if (ax == 0) {
#pragma unroll
        for (int e = 0; e < NV; ++e) wn[e] = wp[e];
      } else if (ax == 1) {
        if (PF) {
#pragma unroll
          for (int e = 0; e < NV; ++e) wn[e] = cr[e];
        } else if (row_nb) {
          ldv<T, NV>(ws + off + n2, wn);
        } else {
#pragma unroll
          for (int e = 0; e < NV; ++e) wn[e] = T(0);
        }
      } else {
#pragma unroll
        for (int e = 0; e + 1 < NV; ++e) wn[e] = wc[e + 1];
        wn[NV - 1] = PF ? ccol : (col_nb ? ws[off + NV] : T(0));
      }
      if (PF) {
#pragma unroll
        for (int e = 0; e < NV; ++e) zc[ax][e] = cz[ax][e];
      } else if (NT)
        ldn_nt<T, NV>(zs + (int64_t)(ax - a_first) * N + off, zc[ax]);
      else
        ldv<T, NV>(zs + (int64_t)(ax - a_first) * N + off, zc[ax]);
#pragma unroll
      for (int e = 0; e < NV; ++e) zin[ax][e] = dual_in<T>(zc[ax][e], wc[e], wn[e], g.c0[ax], g.c1[ax], sigma);
    }
#pragma unroll
    for (int e = 0; e < NV; ++e) wn0[e] = wp[e];
    T zo3[3][NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) {
      T zc1[3], zi1[3], zn1[3];
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) {
        zc1[ax] = ax < a_first ? T(0) : zc[ax][e];
        zi1[ax] = ax < a_first ? T(0) : zin[ax][e];
      }
      dual_out<T, ISO, PD3O>(zc1, zi1, a_first, lam, rho, omr, zn1);
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) zo3[ax][e] = zn1[ax];
    }
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      if (ax < a_first) continue;
      T zn[NV];
#pragma unroll
      for (int e = 0; e < NV; ++e) zn[e] = zo3[ax][e];
      T* zq = zos + (int64_t)(ax - a_first) * N + off;
      if (NT)
        stn_nt<T, NV>(zq, zn);
      else if constexpr (NV == kVecN<T>)
        *reinterpret_cast<typename Vec4<T>::type*>(zq) = *reinterpret_cast<const typename Vec4<T>::type*>(zn);
      else
        zq[0] = zn[0];
    }
  }
}

// Row-blocked form (RB >= 2 rows per thread): a thread owns NV positions of RB consecutive rows, so the row + 1
// neighbour of every row but its last is its own next row (already in registers at this plane) and only one
// neighbour row per RB rows is read from another thread's rows: w is read 1 + 1 / RB times per voxel instead of
// twice, and the HBM over-fetch of the neighbour rows that another workgroup has not kept in L2 shrinks with it
// (1024^3: 1.107 x compulsory with RB = 1; profiles/r06*_k4_rows.txt).  Same per-element expressions: the same bits.
template <typename T, int NV, int RB, bool ISO, bool PD3O, bool NT>
__global__ void __launch_bounds__(kBlock) pds_dual_rows_kernel(PdsC<T> p, const T* __restrict__ w,
                                                               const T* __restrict__ z, T* __restrict__ zo) {
  const PdsGeom<T> g = p.g;
  const T sigma = p.sigma, lam = p.lam, rho = p.rho, omr = p.omr;
  const int n0 = g.n0, n1 = g.n1, n2 = g.n2, D = g.D;
  const int64_t M = (int64_t)n1 * n2, N = M * n0;
  const int a_first = 3 - D;
  const int cgs = (n2 + NV - 1) / NV;  // column groups per row
  const unsigned blk = xcd_tile(blockIdx.x, gridDim.x);
  const int64_t t = (int64_t)blk * kBlock + threadIdx.x;
  const int64_t rg = t / cgs;
  if (rg * RB >= n1) return;  // no barriers below
  const int r = (int)(rg * RB), c = (int)(t - rg * cgs) * NV;
  const int nr = n1 - r < RB ? n1 - r : RB;  // rows of this thread inside the plane
  const int64_t s = blockIdx.z;
  const int pb = blockIdx.y * p.seg;
  const int pe = pb + p.seg < n0 ? pb + p.seg : n0;
  const int64_t j0 = (int64_t)r * n2 + c;
  const T* ws = w + s * N + j0;
  const T* zs = z + s * (int64_t)D * N + j0;
  T* zos = zo + s * (int64_t)D * N + j0;
  const bool row_nb = r + RB < n1, col_nb = c + NV < n2;
  T wcur[RB][NV];  // w at the current plane, rows r .. r + RB - 1 (carried from the previous step)
#pragma unroll
  for (int i = 0; i < RB; ++i) {
    if (i < nr) {
      ldv<T, NV>(ws + (int64_t)pb * M + (int64_t)i * n2, wcur[i]);
    } else {
#pragma unroll
      for (int e = 0; e < NV; ++e) wcur[i][e] = T(0);
    }
  }
  for (int pl = pb; pl < pe; ++pl) {
    const int64_t off = (int64_t)pl * M;
    T wnext[RB][NV], wrow[NV];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
      if (pl + 1 < n0 && i < nr) {
        ldv<T, NV>(ws + off + M + (int64_t)i * n2, wnext[i]);
      } else {
#pragma unroll
        for (int e = 0; e < NV; ++e) wnext[i][e] = T(0);
      }
    }
    if (row_nb) {
      ldv<T, NV>(ws + off + (int64_t)RB * n2, wrow);
    } else {
#pragma unroll
      for (int e = 0; e < NV; ++e) wrow[e] = T(0);
    }
#pragma unroll
    for (int i = 0; i < RB; ++i) {
      if (i >= nr) continue;
      const int64_t ro = off + (int64_t)i * n2;
      T zin[3][NV], zc[3][NV];
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) {
        if (ax < a_first) continue;
        T wn[NV];
        if (ax == 0) {
#pragma unroll
          for (int e = 0; e < NV; ++e) wn[e] = wnext[i][e];
        } else if (ax == 1) {
#pragma unroll
          for (int e = 0; e < NV; ++e) wn[e] = i + 1 < RB ? wcur[i + 1 < RB ? i + 1 : i][e] : wrow[e];
          if (i + 1 < RB && i + 1 >= nr) {  // the plane's last row inside this thread's block: zero neighbour
#pragma unroll
            for (int e = 0; e < NV; ++e) wn[e] = T(0);
          }
        } else {
#pragma unroll
          for (int e = 0; e + 1 < NV; ++e) wn[e] = wcur[i][e + 1];
          wn[NV - 1] = col_nb ? ws[ro + NV] : T(0);
        }
        if (NT)
          ldn_nt<T, NV>(zs + (int64_t)(ax - a_first) * N + ro, zc[ax]);
        else
          ldv<T, NV>(zs + (int64_t)(ax - a_first) * N + ro, zc[ax]);
#pragma unroll
        for (int e = 0; e < NV; ++e) zin[ax][e] = dual_in<T>(zc[ax][e], wcur[i][e], wn[e], g.c0[ax], g.c1[ax], sigma);
      }
      T zo3[3][NV];
#pragma unroll
      for (int e = 0; e < NV; ++e) {
        T zc1[3], zi1[3], zn1[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
          zc1[ax] = ax < a_first ? T(0) : zc[ax][e];
          zi1[ax] = ax < a_first ? T(0) : zin[ax][e];
        }
        dual_out<T, ISO, PD3O>(zc1, zi1, a_first, lam, rho, omr, zn1);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) zo3[ax][e] = zn1[ax];
      }
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) {
        if (ax < a_first) continue;
        T zn[NV];
#pragma unroll
        for (int e = 0; e < NV; ++e) zn[e] = zo3[ax][e];
        T* zq = zos + (int64_t)(ax - a_first) * N + ro;
        if (NT)
          stn_nt<T, NV>(zq, zn);
        else if constexpr (NV == kVecN<T>)
          *reinterpret_cast<typename Vec4<T>::type*>(zq) = *reinterpret_cast<const typename Vec4<T>::type*>(zn);
        else
          zq[0] = zn[0];
      }
    }
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
      for (int e = 0; e < NV; ++e) wcur[i][e] = wnext[i][e];
  }
}

// Plane-block form (3-D, 16-B vectors; PXA_TUNE_DUAL_ROWS = 8): a workgroup owns a block of kLdsRB rows x kLdsC columns
// of the plane and marches its axis-0 segment; at each plane every thread stores its own w vector into an LDS image
// of the block (double-buffered by plane parity), the block's halo -- the row below it and the column right of it,
// fetched one plane ahead -- goes in beside it, and the row + 1 / column + 1 neighbours are read from LDS: a w row is
// fetched from memory by its own workgroup only, plus once more as the halo of the block above it (1 + 1 / kLdsRB
// reads per voxel instead of up to 2 with the one-row kernel, whose neighbour rows other workgroups fetch at their
// own pace).  One barrier per plane.  Same per-element expressions: the same bits.
constexpr int kLdsRB = 8;    // rows per block
constexpr int kLdsC = 128;   // columns per block (32 threads x 4)
constexpr int kLdsP = kLdsC + 4;  // LDS pitch (floats): the halo column's vector at kLdsC

template <bool ISO, bool PD3O, bool ZA>
__global__ void __launch_bounds__(kBlock) pds_dual_lds_kernel(PdsC<float> p, const float* __restrict__ w,
                                                              const float* __restrict__ z, float* __restrict__ zo,
                                                              int tiles2) {
  static_assert(kBlock == kLdsRB * kLdsC / 4, "one 4-vector per thread");
  __shared__ __align__(16) float img[2][kLdsRB + 1][kLdsP];
  const PdsGeom<float> g = p.g;
  const float sigma = p.sigma, lam = p.lam, rho = p.rho, omr = p.omr;
  const int n0 = g.n0, n1 = g.n1, n2 = g.n2;
  const int64_t M = (int64_t)n1 * n2, N = M * n0;
  const unsigned blk = xcd_tile(blockIdx.x, gridDim.x);
  const int tr = (int)(blk / (unsigned)tiles2), tc = (int)(blk - (unsigned)tr * (unsigned)tiles2);
  const int t = threadIdx.x, lr = t >> 5, lc = 4 * (t & 31);
  const int r = tr * kLdsRB + lr, c = tc * kLdsC + lc;
  const bool live = r < n1 && c < n2;  // (n2 % 4 == 0: a vector is wholly inside or outside)
  const int64_t s = blockIdx.z;
  const int pb = blockIdx.y * p.seg;
  const int pe = pb + p.seg < n0 ? pb + p.seg : n0;
  const int64_t j0 = (int64_t)r * n2 + c;
  const float* wb = w + s * N;
  const float* zs = z + s * (int64_t)3 * N + j0;
  float* zos = zo + s * (int64_t)3 * N + j0;
  // halo lanes: threads 0..31 the row below the block (4 columns each), 32..39 the column right of it (one row each)
  const int hr = tr * kLdsRB + kLdsRB, hc = tc * kLdsC + lc;        // row halo position (t < 32)
  const int vr = tr * kLdsRB + (t - 32), vc = tc * kLdsC + kLdsC;   // column halo position (32 <= t < 40)
  const bool hrow = t < 32, hcol = t >= 32 && t < 32 + kLdsRB;
  const bool hin = hrow ? (hr < n1 && hc < n2) : hcol ? (vr < n1 && vc < n2) : false;
  const int64_t hoff = hrow ? (int64_t)hr * n2 + hc : (int64_t)vr * n2 + vc;
  auto load_w = [&](int pl, float (&v)[4]) {
    if (live && pl < n0) {
      ldv<float, 4>(wb + (int64_t)pl * M + j0, v);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = 0.f;
    }
  };
  auto load_h = [&](int pl, float (&v)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = 0.f;
    if (hin && pl < n0) {
      if (hrow)
        ldv<float, 4>(wb + (int64_t)pl * M + hoff, v);
      else
        v[0] = wb[(int64_t)pl * M + hoff];
    }
  };
  float wc[4], wp[4], hc4[4], hn4[4];
  load_w(pb, wc);
  load_h(pb, hc4);
  float zn[3][4];  // z of the next plane (ZA: loaded one plane ahead)
  auto load_z = [&](int pl, float (&v)[3][4]) {
    if (live && pl < pe) {
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) ldn_nt<float, 4>(zs + (int64_t)ax * N + (int64_t)pl * M, v[ax]);
    }
  };
  if (ZA) load_z(pb, zn);
  for (int pl = pb; pl < pe; ++pl) {
    const int par = pl & 1;
    const int64_t off = (int64_t)pl * M;
    float zc[3][4];
    if (ZA) {
#pragma unroll
      for (int ax = 0; ax < 3; ++ax)
#pragma unroll
        for (int e = 0; e < 4; ++e) zc[ax][e] = zn[ax][e];
    }
    load_w(pl + 1, wp);  // next plane: own vector and halo, in flight through this plane
    load_h(pl + 1, hn4);
    if (ZA)
      load_z(pl + 1, zn);
    else
      load_z(pl, zc);
    // this plane's w image: own vectors, the halo row / column (zeros outside the image)
    *reinterpret_cast<float4*>(&img[par][lr][lc]) = make_float4(wc[0], wc[1], wc[2], wc[3]);
    if (hrow) *reinterpret_cast<float4*>(&img[par][kLdsRB][lc]) = make_float4(hc4[0], hc4[1], hc4[2], hc4[3]);
    if (hcol) img[par][t - 32][kLdsC] = hc4[0];
    __syncthreads();  // (double buffer: the next plane writes the other image, so one barrier per plane)
    if (live) {
      float wr[4];
      const float4 q = *reinterpret_cast<const float4*>(&img[par][lr + 1][lc]);
      wr[0] = q.x, wr[1] = q.y, wr[2] = q.z, wr[3] = q.w;
      const float wcol = img[par][lr][lc + 4];
      float zin[3][4];
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) {
        float wn[4];
        if (ax == 0) {
#pragma unroll
          for (int e = 0; e < 4; ++e) wn[e] = wp[e];
        } else if (ax == 1) {
#pragma unroll
          for (int e = 0; e < 4; ++e) wn[e] = r + 1 < n1 ? wr[e] : 0.f;
        } else {
#pragma unroll
          for (int e = 0; e < 3; ++e) wn[e] = wc[e + 1];
          wn[3] = c + 4 < n2 ? wcol : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) zin[ax][e] = dual_in<float>(zc[ax][e], wc[e], wn[e], g.c0[ax], g.c1[ax], sigma);
      }
      float zo3[3][4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float zc1[3], zi1[3], zn1[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
          zc1[ax] = zc[ax][e];
          zi1[ax] = zin[ax][e];
        }
        dual_out<float, ISO, PD3O>(zc1, zi1, 0, lam, rho, omr, zn1);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) zo3[ax][e] = zn1[ax];
      }
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) stn_nt<float, 4>(zos + (int64_t)ax * N + off, zo3[ax]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      wc[e] = wp[e];
      hc4[e] = hn4[e];
    }
  }
}

template <bool PD3O, bool ZA>
int launch_c_lds(const PdsC<float>& pc, bool iso, int nseg, const void* w, const void* z, void* zo, hipStream_t st) {
  const int tiles1 = (pc.g.n1 + kLdsRB - 1) / kLdsRB, tiles2 = (pc.g.n2 + kLdsC - 1) / kLdsC;
  dim3 grid((unsigned)((int64_t)tiles1 * tiles2), (unsigned)nseg, (unsigned)pc.g.stack);
  if (iso)
    hipLaunchKernelGGL((pds_dual_lds_kernel<true, PD3O, ZA>), grid, dim3(kBlock), 0, st, pc, (const float*)w, (const float*)z,
                       (float*)zo, tiles2);
  else
    hipLaunchKernelGGL((pds_dual_lds_kernel<false, PD3O, ZA>), grid, dim3(kBlock), 0, st, pc, (const float*)w, (const float*)z,
                       (float*)zo, tiles2);
  return last_launch_status();
}

template <typename T, int NV, int RB, bool PD3O>
int launch_c_rows(const PdsC<T>& pc, bool iso, int nseg, const void* w, const void* z, void* zo, hipStream_t st) {
  const int64_t items = (int64_t)((pc.g.n1 + RB - 1) / RB) * ((pc.g.n2 + NV - 1) / NV);
  const int64_t blocks = (items + kBlock - 1) / kBlock;
  dim3 grid((unsigned)blocks, (unsigned)nseg, (unsigned)pc.g.stack);
  if (iso)
    hipLaunchKernelGGL((pds_dual_rows_kernel<T, NV, RB, true, PD3O, true>), grid, dim3(kBlock), 0, st, pc, (const T*)w,
                       (const T*)z, (T*)zo);
  else
    hipLaunchKernelGGL((pds_dual_rows_kernel<T, NV, RB, false, PD3O, true>), grid, dim3(kBlock), 0, st, pc, (const T*)w,
                       (const T*)z, (T*)zo);
  return last_launch_status();
}

template <typename T, int NV, bool PD3O>
int launch_c(const PdsC<T>& pc, bool iso, int64_t M, int nseg, const void* w, const void* z, void* zo,
             hipStream_t st) {
  // rows per thread (PXA_TUNE_DUAL_ROWS): 1 the one-row kernel, 2 / 4 the row-blocked kernel
  const int64_t rb = tuning(PXA_TUNE_DUAL_ROWS);
  if constexpr (sizeof(T) == 4 && NV == 4) {
    if (rb == 8 && pc.g.D == 3) return launch_c_lds<PD3O, false>(pc, iso, nseg, w, z, zo, st);
    if (rb == 9 && pc.g.D == 3) return launch_c_lds<PD3O, true>(pc, iso, nseg, w, z, zo, st);
  }
  if (rb == 2) return launch_c_rows<T, NV, 2, PD3O>(pc, iso, nseg, w, z, zo, st);
  if (rb == 4) return launch_c_rows<T, NV, 4, PD3O>(pc, iso, nseg, w, z, zo, st);
  const int64_t blocks = (M + (int64_t)kBlock * NV - 1) / ((int64_t)kBlock * NV);
  dim3 grid((unsigned)blocks, (unsigned)nseg, (unsigned)pc.g.stack);
  // z / z_out non-temporal (read / written once): w's row + 1 neighbours stay in L2 (1024^3, r04b: fetch 22.5
  // -> 19 B/voxel, 5.9 -> 5.1-5.7 ms)
  if (rb != 1) {  // the next plane's loads one plane early (default; 1: without, A/B -- 1024^3 r06ar: 5.00 -> 4.94 ms)
    if (iso)
      hipLaunchKernelGGL((pds_dual_kernel<T, NV, true, PD3O, true, true>), grid, dim3(kBlock), 0, st, pc, (const T*)w,
                         (const T*)z, (T*)zo);
    else
      hipLaunchKernelGGL((pds_dual_kernel<T, NV, false, PD3O, true, true>), grid, dim3(kBlock), 0, st, pc, (const T*)w,
                         (const T*)z, (T*)zo);
    return last_launch_status();
  }
  if (iso)
    hipLaunchKernelGGL((pds_dual_kernel<T, NV, true, PD3O, true>), grid, dim3(kBlock), 0, st, pc, (const T*)w,
                       (const T*)z, (T*)zo);
  else
    hipLaunchKernelGGL((pds_dual_kernel<T, NV, false, PD3O, true>), grid, dim3(kBlock), 0, st, pc, (const T*)w,
                       (const T*)z, (T*)zo);
  return last_launch_status();
}

// Kernel C over a whole (stack, n0, n1, n2) geometry: z_out = relax(fenchel_prox_h(z + sigma K w)).  The
// march is split into axis-0 segments so that about 2048 workgroups are in flight (no halo: w(p + 1) is a
// plain load; at 1024^3 2048 took 5.0-5.1 ms against 5.1-5.7 ms at 4096, profiles/r04_k4_wgs.txt).  pd3o selects the relaxation order: (1 - rho) z + rho z_t, else rho z_t + (1 - rho) z.
// Slab form: always the one-row kernel with the next plane's loads one plane early (launch_c's default).
template <typename T, int NV, bool PD3O>
int launch_c_slab(const PdsC<T>& pc, bool iso, int64_t M, int nseg, const void* w, const void* z, void* zo,
                  const GhostC<T>& gh, hipStream_t st) {
  const int64_t blocks = (M + (int64_t)kBlock * NV - 1) / ((int64_t)kBlock * NV);
  dim3 grid((unsigned)blocks, (unsigned)nseg, (unsigned)pc.g.stack);
  if (iso)
    hipLaunchKernelGGL((pds_dual_kernel<T, NV, true, PD3O, true, true, GhostC<T>>), grid, dim3(kBlock), 0, st, pc,
                       (const T*)w, (const T*)z, (T*)zo, gh);
  else
    hipLaunchKernelGGL((pds_dual_kernel<T, NV, false, PD3O, true, true, GhostC<T>>), grid, dim3(kBlock), 0, st, pc,
                       (const T*)w, (const T*)z, (T*)zo, gh);
  return last_launch_status();
}

template <typename T>
int run_c(const PdsGeom<T>& g, T sigma, T lam, T rho, T omr, bool pd3o, bool iso, const void* w, const void* z,
          void* z_out, hipStream_t st, const GhostC<T>* gh = nullptr) {
  constexpr int V = kVecN<T>;
  const int64_t M = (int64_t)g.n1 * g.n2;
  PdsC<T> pc;
  pc.g = g;
  pc.sigma = sigma;
  pc.lam = lam;
  pc.rho = rho;
  pc.omr = omr;
  const bool vec = (g.n2 % V == 0) && aligned16(w) && aligned16(z) && aligned16(z_out) && (!gh || aligned16(gh->w_hi));
  const int nv = vec ? V : 1;
  const int64_t rbt = gh ? 0 : tuning(PXA_TUNE_DUAL_ROWS);
  const int64_t rbk = rbt == 2 ? 2 : rbt == 4 ? 4 : 1;
  int64_t blocks = g.stack * ((M + (int64_t)kBlock * nv * rbk - 1) / ((int64_t)kBlock * nv * rbk));
  if ((rbt == 8 || rbt == 9) && vec && g.D == 3 && sizeof(T) == 4)  // (the plane-block kernel's block count)
    blocks = g.stack * (int64_t)((g.n1 + kLdsRB - 1) / kLdsRB) * ((g.n2 + kLdsC - 1) / kLdsC);
  const int64_t target = tuning(PXA_TUNE_DUAL_WGS) > 0 ? tuning(PXA_TUNE_DUAL_WGS) : 2048;  // A/B knob
  int cseg = (int)((target + blocks - 1) / blocks);
  if (cseg > g.n0) cseg = g.n0;
  if (cseg < 1) cseg = 1;
  pc.seg = (int)((g.n0 + cseg - 1) / cseg);
  cseg = (int)((g.n0 + pc.seg - 1) / pc.seg);
  if (gh) {
    if (vec)
      return pd3o ? launch_c_slab<T, V, true>(pc, iso, M, cseg, w, z, z_out, *gh, st)
                  : launch_c_slab<T, V, false>(pc, iso, M, cseg, w, z, z_out, *gh, st);
    return pd3o ? launch_c_slab<T, 1, true>(pc, iso, M, cseg, w, z, z_out, *gh, st)
                : launch_c_slab<T, 1, false>(pc, iso, M, cseg, w, z, z_out, *gh, st);
  }
  if (vec)
    return pd3o ? launch_c<T, V, true>(pc, iso, M, cseg, w, z, z_out, st) : launch_c<T, V, false>(pc, iso, M, cseg, w, z, z_out, st);
  return pd3o ? launch_c<T, 1, true>(pc, iso, M, cseg, w, z, z_out, st) : launch_c<T, 1, false>(pc, iso, M, cseg, w, z, z_out, st);
}

// The geometry every entry point hands to its kernels, validated: sizes, D in {2, 3}, forward-difference taps `diff`
// = (c0 per axis, c1 per axis).
template <typename T>
int make_geom(int64_t stack, int64_t y_images, int64_t n0, int64_t n1, int64_t n2, int64_t D, const double* diff,
              PdsGeom<T>& g) {
  PXA_CHECK_ARG(diff != nullptr);
  PXA_CHECK_ARG(stack >= 1 && stack <= 65535 && y_images >= 1 && stack % y_images == 0);
  PXA_CHECK_ARG(n0 >= 1 && n1 >= 1 && n2 >= 1 && n0 <= 0x7fffffff && n1 <= 0x7fffffff && n2 <= 0x7fffffff);
  PXA_CHECK_ARG(n0 * n1 * n2 <= ((int64_t)1 << 40));
  PXA_CHECK_ARG(D == 2 || D == 3);
  g.stack = stack;
  g.y_images = y_images;
  g.n0 = (int)n0;
  g.n1 = (int)n1;
  g.n2 = (int)n2;
  g.D = (int)D;
  for (int a = 0; a < 3; ++a) {
    g.c0[a] = (T)diff[a];
    g.c1[a] = (T)diff[3 + a];
  }
  return PXA_OK;
}

// Kernel C alone.  pxa_tv_dual_update (slab == nullptr; the "Gradient + prox" kernel of SURVEY §8(d), K4): a whole
// stack of volumes, or of images with D = 2.  pxa_pds_slab_dual: one rank's slab of a volume, w at plane n0 from the
// next slab (slab->w_hi as (stack, dhi, n1, n2); null: the volume's edge).
template <typename T>
int dual_entry(int relax, const int64_t* geom, const double* diff, double sigma, double lam, double rho, int h_kind,
               const void* w, const void* z, void* z_out, hipStream_t st, const GhostC<T>* slab = nullptr) {
  PXA_CHECK_ARG(geom && w && z && z_out && z_out != w);
  PXA_CHECK_ARG(relax == 0 || relax == 1);
  PXA_CHECK_ARG(h_kind == 0 || h_kind == 1);
  PdsGeom<T> g;
  if (const int e = make_geom<T>(geom[0], 1, geom[1], geom[2], geom[3], geom[4], diff, g)) return e;
  GhostC<T> gh{nullptr, 0};
  if (!slab) {
    PXA_CHECK_ARG(g.D == 3 || g.n0 == 1);
  } else {
    PXA_CHECK_ARG(g.D == 3 || g.n0 > 1);  // volumes only: an image has no axis-0 neighbour
    PXA_CHECK_ARG(slab->dhi >= 0 && slab->dhi <= 0x7fffffff);
    if (slab->w_hi != nullptr) {
      PXA_CHECK_ARG(g.D == 3);         // axis 0 not differentiated: no ghost is read
      PXA_CHECK_ARG(slab->dhi >= 1);   // kernel C reads one plane ahead
      PXA_CHECK_ARG(slab->w_hi != z_out);
      gh = *slab;
    }
  }
  return run_c<T>(g, (T)sigma, (T)lam, (T)rho, (T)(1.0 - rho), relax == 0, h_kind == 1, w, z, z_out, st,
                  slab ? &gh : nullptr);
}

// Measurement hook (PXA_TUNE_PDS_EVENTS > 0, bench.py's c3 record): HIP events recorded on the launch stream
// before kernel A and after kernels A, B and C of every step, so that the per-kernel times of the timed
// steps are read afterwards (pxa_pds_kernel_ms) without synchronising inside the timed region.
constexpr int kPdsEventSteps = 64;
struct PdsEvents {
  hipEvent_t ev[kPdsEventSteps][4];
  int created = 0;  // steps whose events exist
  int used = 0;     // steps recorded since the last read
};
static PdsEvents g_pds_ev;

static void pds_event(int k, hipStream_t st) {
  PdsEvents& E = g_pds_ev;
  if (E.used >= kPdsEventSteps) return;
  if (E.used == E.created) {
    for (int j = 0; j < 4; ++j) (void)hipEventCreate(&E.ev[E.created][j]);
    ++E.created;
  }
  (void)hipEventRecord(E.ev[E.used][k], st);
  if (k == 3) ++E.used;
}

// Validated algorithm, geometry, taps and scalars shared by the three-launch, the slab and the look-ahead step.
template <typename T>
struct PdsSetup {
  PdsGeom<T> g;
  TapWindow kw[3];
  int R0, R;  // axis-0 radius (0: axis 0 not blurred), in-plane radius
  bool pd3o, id0;
  T tau, sigma, rho, lam, pw, omr;
  int64_t M;
  int prox;
  bool iso;
};

template <typename T>
int pds_setup(int algo, const int64_t* geom, const int32_t* ntaps, const int32_t* offs, const double* coefs,
              const double* diff, const double* scal, int prox, int h_kind, PdsSetup<T>& S) {
  PXA_CHECK_ARG(algo == 0 || algo == 1);
  PXA_CHECK_ARG(geom && ntaps && offs && coefs && scal);
  if (const int e = make_geom<T>(geom[0], geom[1], geom[2], geom[3], geom[4], geom[5], diff, S.g)) return e;
  static_assert(PXA_PDS_TAP_SLOTS == 2 * kMaxR + 1, "the tap slots hold one dense window of reach kMaxR");
  PXA_CHECK_ARG(prox >= 0 && prox <= 2 && (h_kind == 0 || h_kind == 1));
  for (int a = 0; a < 3; ++a) PXA_CHECK_ARG(ntaps[a] >= 1 && ntaps[a] <= PXA_PDS_TAP_SLOTS);
  int Ra[3];
  for (int a = 0; a < 3; ++a) {
    Ra[a] = tap_window(ntaps[a], offs + a * PXA_PDS_TAP_SLOTS, coefs + a * PXA_PDS_TAP_SLOTS, S.kw[a]);
    if (Ra[a] < 0) return PXA_ERR_UNSUPPORTED;
  }
  // axis 0 is the identity iff its window is exactly [1] at offset 0
  S.id0 = Ra[0] == 0 && S.kw[0][kMaxR] == 1.0;
  S.R0 = S.id0 ? 0 : (Ra[0] > 0 ? Ra[0] : 1);
  S.R = Ra[1] > Ra[2] ? Ra[1] : Ra[2];
  if (S.R < 1) S.R = 1;
  S.pd3o = algo == 0;
  S.tau = (T)scal[0];
  S.sigma = (T)scal[1];
  S.rho = (T)scal[2];
  S.lam = (T)scal[3];
  S.pw = (T)scal[4];
  S.omr = (T)(1.0 - scal[2]);
  S.M = (int64_t)S.g.n1 * S.g.n2;
  S.prox = prox;
  S.iso = h_kind == 1;
  return PXA_OK;
}

// The array arguments every step needs: z, S^T y, x_out and w; PD3O its u pair; work_q when axis 0 is blurred.
template <typename T>
int step_arrays(const PdsSetup<T>& S, const void* u, const void* z, const void* hty, const void* x_out,
                const void* u_out, const void* work_q, const void* work_w) {
  PXA_CHECK_ARG(z && hty && x_out && work_w);
  PXA_CHECK_ARG(!S.pd3o || (u && u_out));
  PXA_CHECK_ARG(S.id0 || work_q != nullptr);
  return PXA_OK;
}

// axis-0 march parameters (kernels A and D); resolves nseg (< 1: auto)
template <typename T>
PdsA<T> make_a(const PdsSetup<T>& S, int& nseg) {
  PdsA<T> pa;
  pa.g = S.g;
  tap_dense(S.kw[0], S.R0, pa.k0);
  pa.tau = S.tau;
  pa.pw = S.pw;
  pa.prox = S.prox;
  const int64_t n0 = S.g.n0;
  if (nseg < 1) {
    // auto: about 4096 workgroups in flight, segments >= 4 rings deep (halo recompute <= 1/2)
    const int64_t blocks = S.g.stack * ((S.M + 2 * kAThreads - 1) / (2 * kAThreads));
    const int64_t want = (4096 + blocks - 1) / blocks;
    const int64_t cap = S.R0 > 0 ? n0 / (4 * (2 * S.R0 + 1)) : n0;
    nseg = (int)(want < cap ? want : cap);
    if (nseg < 1) nseg = 1;
  }
  if (nseg > n0) nseg = (int)n0;
  pa.seg = (int)((n0 + nseg - 1) / nseg);
  nseg = (int)((n0 + pa.seg - 1) / pa.seg);
  return pa;
}

template <typename T>
inline bool aligned_pair(const void* p) {
  return (uintptr_t)p % (2 * sizeof(T)) == 0;
}

// kernel A on src = u (PD3O: v = prox_g(u - tau K^T z) -> x_out) or x (Condat-Vu), Q = G0 v -> work_q; it runs
// unless Condat-Vu has nothing to march (axis 0 not blurred).  *q_src: kernel B's input plane stack.  gh: the slab
// form's ghost planes; pairs: the caller's ghost buffers allow kernel A's two-position path.
template <typename T>
int stage_a(const PdsSetup<T>& S, int nseg, const void* src, const void* z, void* x_out, void* work_q,
            const void** q_src, hipStream_t st, const GhostA<T>* gh = nullptr, bool pairs = true) {
  *q_src = !S.id0 ? work_q : S.pd3o ? x_out : src;
  if (!S.pd3o && S.id0) return PXA_OK;
  const PdsA<T> pa = make_a(S, nseg);
  const bool np2 = pairs && (S.g.n2 % 2 == 0) && aligned_pair<T>(src) && aligned_pair<T>(z) &&
                   aligned_pair<T>(x_out) && (S.id0 || aligned_pair<T>(work_q));
  void* q = S.id0 ? x_out : work_q;  // R0 == 0 never writes q
  return gh ? run_a_slab(pa, *gh, S.pd3o, S.R0, np2 ? 2 : 1, S.M, nseg, src, z, x_out, q, st)
            : run_a(pa, S.pd3o, S.R0, np2 ? 2 : 1, S.M, nseg, src, z, x_out, q, st);
}

// kernel B: mode 0 PD3O, 1 Condat-Vu (K^T z from z), 2 Condat-Vu (K^T z given in `z`)
template <typename T>
int stage_b(const PdsSetup<T>& S, int mode, const void* q_src, const void* xin, const void* u, const void* z,
            const void* hty, void* w, void* out, hipStream_t st, const PdsPtrsSlab* slab = nullptr) {
  constexpr int V = kVecN<T>;
  PdsB<T> pb;
  pb.g = S.g;
  pb.tiles1 = (int)((S.g.n1 + TY - 1) / TY);
  pb.tiles2 = (int)((S.g.n2 + TX - 1) / TX);
  const int64_t ntiles = S.g.stack * S.g.n0 * pb.tiles1 * pb.tiles2;
  PXA_CHECK_ARG(ntiles <= 0x7fffffff);
  pb.ntiles = (unsigned)ntiles;
  tap_dense(S.kw[1], S.R, pb.k1);
  tap_dense(S.kw[2], S.R, pb.k2);
  tap_autocorr(S.kw[1], S.R, pb.g1);
  tap_autocorr(S.kw[2], S.R, pb.g2);
  pb.tau = S.tau;
  pb.rho = S.rho;
  pb.omr = S.omr;
  pb.pw = S.pw;
  pb.prox = S.prox;
  pb.vec_ok = (S.g.n2 % V == 0) && aligned16(q_src) && aligned16(xin) && aligned16(hty) && aligned16(w) &&
              aligned16(out) && aligned16(z) && (mode != 0 || aligned16(u));
  PdsPtrs P{q_src, xin, u, z, hty, w, out};
  if (slab) {  // mode 1 on a slab: the z_0 ghost plane
    pb.vec_ok = pb.vec_ok && aligned16(slab->z_lo);
    PdsPtrsSlab PS{P, slab->z_lo, slab->z_dlo};
    return run_b_slab(pb, S.R, PS, st);
  }
  return run_b(pb, mode, S.R, P, st);
}

// pxa_pds_step: setup, checks, kernels A, B, C
template <typename T>
int pds_entry(int algo, const int64_t* geom, const int32_t* ntaps, const int32_t* offs, const double* coefs,
              const double* diff, const double* scal, int prox, int h_kind, const void* x, const void* u,
              const void* z, const void* hty, void* x_out, void* u_out, void* z_out, void* work_q, void* work_w,
              int nseg, hipStream_t st) {
  PdsSetup<T> S;
  if (const int e = pds_setup<T>(algo, geom, ntaps, offs, coefs, diff, scal, prox, h_kind, S)) return e;
  if (const int e = step_arrays(S, u, z, hty, x_out, u_out, work_q, work_w)) return e;
  PXA_CHECK_ARG(z_out != nullptr);
  PXA_CHECK_ARG(S.pd3o || (x && x_out != x));  // kernel B reads x windows (halos) while writing x_out
  const bool pd3o = S.pd3o;

  const bool evs = tuning(PXA_TUNE_PDS_EVENTS) > 0;
  if (evs) pds_event(0, st);
  const void* q_src;
  if (const int e = stage_a<T>(S, nseg, pd3o ? u : x, z, x_out, work_q, &q_src, st)) return e;
  if (evs) pds_event(1, st);
  if (const int e = stage_b(S, pd3o ? 0 : 1, q_src, pd3o ? (const void*)x_out : x, u, z, hty, work_w,
                            pd3o ? u_out : x_out, st))
    return e;
  if (evs) pds_event(2, st);
  if (const int e = run_c<T>(S.g, S.sigma, S.lam, S.rho, S.omr, pd3o, S.iso, work_w, z, z_out, st)) return e;
  if (evs) pds_event(3, st);
  return PXA_OK;
}

// pxa_pds_slab_primal: kernels A and B of pds_entry on one rank's slab.  ghost = {src_lo, src_hi, z_lo, z_hi}
// depths; src = u (PD3O) or x (Condat-Vu).  What the kernels read beyond the slab (R0 = axis-0 reach):
//   PD3O: kernel A builds v on planes [-2 R0, nl + 2 R0): u and z on 2 R0 planes per side, and z_0 on one more lo
//         plane (the backward neighbour of K^T z at the first plane of the march); kernel B nothing.
//   CV  : kernel A x on 2 R0 planes per side; kernel B z_0 on one lo plane (z_lo holds direction 0 only).
template <typename T>
int pds_slab_entry(int algo, const int64_t* geom, const int32_t* ntaps, const int32_t* offs, const double* coefs,
                   const double* diff, const double* scal, int prox, int h_kind, const void* x, const void* u,
                   const void* z, const void* hty, void* x_out, void* u_out, void* work_q, void* work_w,
                   const int64_t* ghost, const void* src_lo, const void* src_hi, const void* z_lo, const void* z_hi,
                   int nseg, hipStream_t st) {
  PdsSetup<T> S;
  if (const int e = pds_setup<T>(algo, geom, ntaps, offs, coefs, diff, scal, prox, h_kind, S)) return e;
  if (const int e = step_arrays(S, u, z, hty, x_out, u_out, work_q, work_w)) return e;
  PXA_CHECK_ARG(S.pd3o || (x && x_out != x));
  const bool pd3o = S.pd3o;
  const PdsGeom<T>& g = S.g;
  PXA_CHECK_ARG(g.n0 > 1 || g.D == 3);  // volumes only (n0 = 1 / D = 2 images have no axis-0 neighbour)
  const bool any = src_lo || src_hi || z_lo || z_hi;
  PXA_CHECK_ARG(ghost != nullptr || !any);
  int64_t d[4] = {0, 0, 0, 0};
  if (ghost)
    for (int i = 0; i < 4; ++i) {
      PXA_CHECK_ARG(ghost[i] >= 0 && ghost[i] <= 0x7fffffff);
      d[i] = ghost[i];
    }
  if (any) PXA_CHECK_ARG(g.D == 3);  // the batch-as-axis form (directions (1, 2)) needs no ghosts
  const int R2 = 2 * S.R0;
  // a side is either the volume's edge (no ghost) or has every ghost its kernels read, deep enough
  const bool need_src = S.R0 > 0, need_zhi = pd3o && S.R0 > 0;
  const bool lo = z_lo != nullptr, hi = need_src ? src_hi != nullptr : (z_hi != nullptr || src_hi != nullptr);
  if (need_src) PXA_CHECK_ARG((src_lo != nullptr) == lo);
  if (need_zhi) PXA_CHECK_ARG((z_hi != nullptr) == hi);
  if (lo) PXA_CHECK_ARG(d[2] >= (pd3o ? R2 + 1 : 1) && (!need_src || d[0] >= R2));
  if (hi) PXA_CHECK_ARG((!need_src || d[1] >= R2) && (!need_zhi || d[3] >= R2));
  const void* ghosts[4] = {src_lo, src_hi, z_lo, z_hi};
  bool pairs = true;
  for (const void* gp : ghosts) {
    if (gp) PXA_CHECK_ARG(gp != x_out && gp != u_out && gp != work_q && gp != work_w);
    pairs = pairs && aligned_pair<T>(gp);
  }

  GhostA<T> gh;
  gh.src_lo = need_src && lo ? (const T*)src_lo : nullptr;
  gh.src_hi = need_src && hi ? (const T*)src_hi : nullptr;
  gh.z_lo = pd3o && lo ? (const T*)z_lo : nullptr;
  gh.z_hi = need_zhi && hi ? (const T*)z_hi : nullptr;
  gh.src_dlo = (int)d[0];
  gh.src_dhi = (int)d[1];
  gh.z_dlo = (int)d[2];
  gh.z_dhi = (int)d[3];
  const void* q_src;
  if (const int e = stage_a<T>(S, nseg, pd3o ? u : x, z, x_out, work_q, &q_src, st, &gh, pairs)) return e;
  if (pd3o) return stage_b(S, 0, q_src, x_out, u, z, hty, work_w, u_out, st);
  const PdsPtrsSlab zl{{}, lo ? z_lo : nullptr, lo ? d[2] : 0};
  return stage_b(S, 1, q_src, x, u, z, hty, work_w, x_out, st, &zl);
}

// Look-ahead step (pds_march.hpp): [priming march] + kernel B + kernel D.  PD3O: x (current x; written by
// the priming march unless primed), u -> u_out, z -> z_out, x_out = x of the next iteration.  Condat-Vu:
// x -> x_out, z -> z_out, work_kt = K^T z (written by the priming march unless primed, then rewritten for
// the next iteration).  work_q = G0 v (same priming rule; rewritten by kernel D).
template <typename T>
int pds_la_entry(int algo, const int64_t* geom, const int32_t* ntaps, const int32_t* offs, const double* coefs,
                 const double* diff, const double* scal, int prox, int h_kind, int primed, void* x, const void* u,
                 const void* z, const void* hty, void* x_out, void* u_out, void* z_out, void* work_q, void* work_kt,
                 void* work_w, int nseg, hipStream_t st) {
  PdsSetup<T> S;
  if (const int e = pds_setup<T>(algo, geom, ntaps, offs, coefs, diff, scal, prox, h_kind, S)) return e;
  if (const int e = step_arrays(S, u, z, hty, x_out, u_out, work_q, work_w)) return e;
  PXA_CHECK_ARG(x && x_out != x && z_out && z_out != z);
  PXA_CHECK_ARG(S.pd3o || work_kt != nullptr);
  const bool pd3o = S.pd3o;
  const int64_t M = S.M;
  PdsD<T> pd;
  pd.a = make_a(S, nseg);
  pd.sigma = S.sigma;
  pd.lam = S.lam;
  pd.rho = S.rho;
  pd.omr = S.omr;
  // q is written only when axis 0 is blurred; kernel B then reads it, else v itself
  void* q = S.id0 ? work_w : work_q;

  const bool evs = tuning(PXA_TUNE_PDS_EVENTS) > 0;
  if (evs) pds_event(0, st);
  if (!primed) {  // the march of this iteration: v from (u or x, z) without a dual update
    const int e = run_d(pd, pd3o, S.iso, false, S.R0, M, nseg, work_w, z, pd3o ? u : x, z_out,
                        pd3o ? x : work_kt, q, st);
    if (e) return e;
  }
  if (evs) pds_event(1, st);
  {
    const void* q_src = S.id0 ? (const void*)x : work_q;
    const int e = pd3o ? stage_b(S, 0, q_src, x, u, z, hty, work_w, u_out, st)
                       : stage_b(S, 2, q_src, x, nullptr, work_kt, hty, work_w, x_out, st);
    if (e) return e;
  }
  if (evs) pds_event(2, st);
  {
    // dual update of this iteration + the next iteration's march
    const int e = run_d(pd, pd3o, S.iso, true, S.R0, M, nseg, work_w, z, pd3o ? (const void*)u_out : x_out,
                        z_out, pd3o ? x_out : work_kt, q, st);
    if (e) return e;
  }
  if (evs) pds_event(3, st);
  return PXA_OK;
}

}  // namespace pds
}  // namespace pxa

using namespace pxa::pds;
using namespace pxa;

extern "C" {

int pxa_pds_kernel_ms(double* ms_abc, int reset) {
  PdsEvents& E = g_pds_ev;
  if (!ms_abc) return PXA_ERR_ARG;
  ms_abc[0] = ms_abc[1] = ms_abc[2] = 0.0;
  const int n = E.used;
  if (n > 0 && hipEventSynchronize(E.ev[n - 1][3]) != hipSuccess) return PXA_ERR_UNSUPPORTED;
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, E.ev[i][k], E.ev[i][k + 1]) != hipSuccess) return PXA_ERR_UNSUPPORTED;
      ms_abc[k] += ms;
    }
  if (reset) E.used = 0;
  return n;
}

int pxa_pds_step(int dtype, int algo, const int64_t* geom, const int32_t* ntaps, const int32_t* offs,
                 const double* coefs, const double* diff, const double* scal, int prox, int h_kind, const void* x,
                 const void* u, const void* z, const void* hty, void* x_out, void* u_out, void* z_out, void* work_q,
                 void* work_w, int nseg, void* stream) {
  PXA_DISPATCH(dtype, T,
               return pds_entry<T>(algo, geom, ntaps, offs, coefs, diff, scal, prox, h_kind, x, u, z, hty, x_out, u_out,
                                   z_out, work_q, work_w, nseg, as_stream(stream)));
}

int pxa_tv_dual_update(int dtype, int relax, const int64_t* geom, const double* diff, double sigma, double lam,
                       double rho, int h_kind, const void* w, const void* z, void* z_out, void* stream) {
  PXA_DISPATCH(dtype, T,
               return dual_entry<T>(relax, geom, diff, sigma, lam, rho, h_kind, w, z, z_out, as_stream(stream)));
}

int pxa_pds_slab_primal(int dtype, int algo, const int64_t* geom, const int32_t* ntaps, const int32_t* offs,
                        const double* coefs, const double* diff, const double* scal, int prox, int h_kind,
                        const void* x, const void* u, const void* z, const void* hty, void* x_out, void* u_out,
                        void* work_q, void* work_w, const int64_t* ghost, const void* src_lo, const void* src_hi,
                        const void* z_lo, const void* z_hi, int nseg, void* stream) {
  PXA_DISPATCH(dtype, T,
               return pds_slab_entry<T>(algo, geom, ntaps, offs, coefs, diff, scal, prox, h_kind, x, u, z, hty, x_out,
                                        u_out, work_q, work_w, ghost, src_lo, src_hi, z_lo, z_hi, nseg,
                                        as_stream(stream)));
}

int pxa_pds_slab_dual(int dtype, int relax, const int64_t* geom, const double* diff, double sigma, double lam,
                      double rho, int h_kind, const void* w, const void* w_hi, int64_t w_hi_depth, const void* z,
                      void* z_out, void* stream) {
  PXA_DISPATCH(dtype, T, const GhostC<T> gh{(const T*)w_hi, w_hi_depth};
               return dual_entry<T>(relax, geom, diff, sigma, lam, rho, h_kind, w, z, z_out, as_stream(stream), &gh));
}

int pxa_pds_step_la(int dtype, int algo, const int64_t* geom, const int32_t* ntaps, const int32_t* offs,
                    const double* coefs, const double* diff, const double* scal, int prox, int h_kind, int primed,
                    void* x, const void* u, const void* z, const void* hty, void* x_out, void* u_out, void* z_out,
                    void* work_q, void* work_kt, void* work_w, int nseg, void* stream) {
  PXA_DISPATCH(dtype, T,
               return pds_la_entry<T>(algo, geom, ntaps, offs, coefs, diff, scal, prox, h_kind, primed, x, u, z, hty,
                                      x_out, u_out, z_out, work_q, work_kt, work_w, nseg, as_stream(stream)));
}

}  // extern "C"
