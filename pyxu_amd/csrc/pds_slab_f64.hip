// Slab-form instantiations of kernels A and B (double): ghost planes from the neighbouring slabs; see pds3d.hpp.
#include "pds3d.hpp"

namespace pxa {
namespace pds {

int run_a_slab(const PdsA<double>& pa, const GhostA<double>& gh, bool pd3o, int R0, int np, int64_t M, int nseg,
               const void* src, const void* z, void* xo, void* q, hipStream_t st) {
  return dispatch_a<double>(pd3o, R0, pa, np, M, nseg, src, z, xo, q, st, gh);
}

int run_b_slab(const PdsB<double>& pb, int R, const PdsPtrsSlab& P, hipStream_t st) {
  return dispatch_b<double, 1, PdsPtrsSlab>(R, pb, P, st);
}

}  // namespace pds
}  // namespace pxa
