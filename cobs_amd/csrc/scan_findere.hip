// cobs_amd/csrc/scan_findere.hip -- the findere (FZ = true, ScanArgs::findere = z > 0) instantiations of K2.  The kernel
// and its launch templates are in kernels.hip, included here without its host definitions; launch_scan comes here when z > 0.
#define COBS_SCAN_FINDERE_UNIT
#include "kernels.hip"

namespace cobs_amd {

hipError_t launch_scan_findere(const ScanArgs& a, int planes, int nw, bool multi_query, hipStream_t stream) {
    return launch_scan_fz<true>(a, planes, nw, multi_query, stream);
}

}  // namespace cobs_amd
