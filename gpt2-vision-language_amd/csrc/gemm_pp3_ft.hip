// gemm_pp3_kernel instances for A K-contiguous, B MN-contiguous (gemm_pp3.h).
#include "gemm_pp3.h"

namespace gvl {
int gemm_pp3_launch_ft(const GemmP& p, const GemmSink& k) { return launch_pp3_epi<PP3_NS, false, true>(p, k); }
}  // namespace gvl
