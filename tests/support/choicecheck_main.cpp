// TEST INFRASTRUCTURE ONLY: the launch-mode stages as a stand-alone program, for a build with
// -fsanitize=address,undefined (host code only; never loaded into python).
//     choicecheck_bin < rows of 24 integers  > rows of 20 integers     (choicecheck.py: MODES_IN, MODES_OUT)
// Compiled with csrc/switches.cpp and csrc/system_choice.cpp alone: the plan builders choose_ldlt_plan calls are not
// part of what runs here.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

#include "choicecheck_modes.h"

namespace slpx {
LdltPlan build_ldlt_plan(const CscPattern&, int, const LdltOptions&, const std::vector<int32_t>*, const std::vector<uint8_t>*) { std::abort(); }
LdltPlan build_dense_ldlt_plan(const CscPattern&, int) { std::abort(); }
bool ldlt_plan_error_is_too_big(const std::exception&) { std::abort(); }
}  // namespace slpx

int main() {
  int64_t in[choicecheck::kModesIn], out[choicecheck::kModesOut];
  for (;;) {
    for (int i = 0; i < choicecheck::kModesIn; ++i) {
      long long v = 0;
      if (std::scanf("%lld", &v) != 1) return i == 0 ? 0 : 2;
      in[i] = v;
    }
    choicecheck::run_modes(in, out);
    for (int i = 0; i < choicecheck::kModesOut; ++i) std::printf("%lld%c", static_cast<long long>(out[i]), i + 1 == choicecheck::kModesOut ? '\n' : ' ');
  }
}
