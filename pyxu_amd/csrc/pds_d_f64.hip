// Kernel D instantiations (double); see pds_march.hpp.
#include "pds_march.hpp"

namespace pxa {
namespace pds {

PXA_PDS_RUN_D(double) { return dispatch_d<double>(pd, pd3o, iso, dual, R0, M, nseg, w, z, src, zo, ao, q, st); }

}  // namespace pds
}  // namespace pxa
