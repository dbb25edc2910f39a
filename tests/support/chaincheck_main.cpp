// TEST INFRASTRUCTURE ONLY: the ledger of the chained-step protocol (csrc/chain_ledger.hpp) as a stand-alone program,
// built plain and with -fsanitize=address,undefined (host code only; never loaded into python).
//     chaincheck_bin < a script of events  > what the ledger answered, one line per event
// Events (tests/support/chaincheck.py says what the lines mean):
//     sweep W | step W | twin | touch | fail | break | save | restore | start HEADROOM [STEP_NUMBER]
// The program does what StepChain and DeviceNlp do around the ledger and nothing else: sweep_launched() after a
// chained sweep only, step_link() then step_launched() for a step.
#include <cstdio>
#include <cstring>

#include "../../sleipnir_amd/csrc/chain_ledger.hpp"

int main() {
  slpx::ChainLedger ledger;
  slpx::ChainLedger::Book book = ledger.save();
  auto state = [&](const char* what) {
    std::printf("%s: step_number %u sweep_total %u step_total %u last_step_chained %d pending %d touched %d failures %d\n", what,
                ledger.step_number(), ledger.sweep_total(), ledger.step_total(), ledger.last_step_chained() ? 1 : 0,
                ledger.pending() ? 1 : 0, ledger.touched() ? 1 : 0, ledger.failures());
  };
  char word[32];
  while (std::scanf("%31s", word) == 1) {
    if (!std::strcmp(word, "sweep")) {
      unsigned int w = 0;
      if (std::scanf("%u", &w) != 1) return 2;
      const slpx::ChainLedger::Sweep s = ledger.begin_sweep();
      if (s.where == slpx::ChainLedger::Sweep::Chained) {
        ledger.sweep_launched(w);
        std::printf("sweep: chained wait_step %u this_step %u order_by_event %d\n", s.wait_step, s.this_step, s.order_by_event ? 1 : 0);
      } else {
        std::printf("sweep: %s order_pending %d\n", s.where == slpx::ChainLedger::Sweep::Restart ? "restart" : "main", s.order_pending ? 1 : 0);
      }
    } else if (!std::strcmp(word, "step")) {
      unsigned int w = 0;
      if (std::scanf("%u", &w) != 1) return 2;
      const slpx::ChainLedger::StepLink l = ledger.step_link();
      ledger.step_launched(w);
      std::printf("step: chained %d wait_step %u this_step %u\n", l.chained ? 1 : 0, l.wait_step, l.this_step);
    } else if (!std::strcmp(word, "twin")) {
      ledger.twin_launched();
      state("twin");
    } else if (!std::strcmp(word, "touch")) {
      std::printf("touch: order_by_event %d\n", ledger.main_stream_used() ? 1 : 0);
    } else if (!std::strcmp(word, "fail")) {
      ledger.failed();
      state("fail");
    } else if (!std::strcmp(word, "break")) {
      ledger.break_next();
      state("break");
    } else if (!std::strcmp(word, "save")) {
      book = ledger.save();
      state("save");
    } else if (!std::strcmp(word, "restore")) {
      ledger.restore(book);
      state("restore");
    } else if (!std::strcmp(word, "start")) {
      unsigned int headroom = 0, seq = 0;
      if (std::scanf("%u", &headroom) != 1) return 2;
      int c;
      while ((c = std::getchar()) == ' ') {
      }
      if (c != '\n' && c != EOF) {
        std::ungetc(c, stdin);
        if (std::scanf("%u", &seq) != 1) return 2;
      }
      ledger.start(headroom, seq);
      state("start");
    } else {
      std::fprintf(stderr, "chaincheck: unknown event '%s'\n", word);
      return 2;
    }
  }
  return 0;
}
