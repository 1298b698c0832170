// gemm_pp3_kernel instances for A MN-contiguous, B K-contiguous (gemm_pp3.h).
#include "gemm_pp3.h"

namespace gvl {
int gemm_pp3_launch_tf(const GemmP& p, const GemmSink& k) { return launch_pp3_epi<PP3_NS, true, false>(p, k); }
}  // namespace gvl
