// TEST INFRASTRUCTURE ONLY — never linked into the product.
//
// The instance classification of the batched sensitivity calls (csrc/sens_plan.hpp: sens_classify_instances) on the
// caller's arrays: a pure host function, so tests/test_sensitivity_batch_cpu.py runs it without a device.
#include <cstdint>

#include "../../sleipnir_amd/csrc/sens_plan.hpp"

extern "C" {

void sbc_classify(int32_t B, int32_t n, int32_t m_e, int32_t m_i, int32_t n_p, const double* x, const double* s, const double* y,
                  const double* z, const double* mu, const double* params, const double* extra, int32_t n_extra, int32_t* status) {
  slpx::sens_classify_instances(B, n, m_e, m_i, n_p, x, s, y, z, mu, params, extra, n_extra, status);
}

}  // extern "C"
