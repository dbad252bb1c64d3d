// Kernel A instantiations (float); see pds3d.hpp.
#include "pds3d.hpp"

namespace pxa {
namespace pds {

int run_a(const PdsA<float>& pa, bool pd3o, int R0, int np, int64_t M, int nseg, const void* src, const void* z,
          void* xo, void* q, hipStream_t st) {
  return dispatch_a<float>(pd3o, R0, pa, np, M, nseg, src, z, xo, q, st);
}

}  // namespace pds
}  // namespace pxa
