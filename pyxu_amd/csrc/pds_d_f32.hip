// Kernel D instantiations (float); see pds_march.hpp.
#include "pds_march.hpp"

namespace pxa {
namespace pds {

PXA_PDS_RUN_D(float) { return dispatch_d<float>(pd, pd3o, iso, dual, R0, M, nseg, w, z, src, zo, ao, q, st); }

}  // namespace pds
}  // namespace pxa
