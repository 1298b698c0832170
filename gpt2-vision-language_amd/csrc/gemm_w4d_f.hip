// gemm_w4d_kernel instances with a K-contiguous B (the weight in forward GEMMs) and the
// routing of the direct-A variant: gemm_w4d.h.
#include "gemm_w4d.h"

namespace gvl {

int gemm_w4d_launch_t(const GemmP& p, const GemmSink& k);  // gemm_w4d_t.hip

// A shape the four-wave planner accepted with 192-row tiles runs on the direct-A kernel when K
// is a multiple of six 64-deep steps and its epilogue is instantiated.  128-row tiles stay on
// gemm_w4m_kernel (the caller's choice, gemm_w4.hip): with 32 rows per wave the B fragment
// reads (all 128 columns per wave) fill the LDS again and a 128-row direct variant measured
// slower there (cross-att step: dX 24.4 vs 21.4 us; 192-row dX 35.9 vs 38.6 us,
// profiles/r3/w4d_ab_r3s2.txt).
bool gemm_w4d_ok(const GemmP& p) {
  return p.K % (6 * D_KS) == 0 && p.lda % 8 == 0 && epi_supported(gemm_epi_kind(p));
}

int gemm_w4d_launch(const GemmP& p, int b_mn, const GemmSink& s) {
  return b_mn ? gemm_w4d_launch_t(p, s) : launch_epi<false>(p, s);
}

}  // namespace gvl
