// Chained steps on the device ("chained steps"): the sweep's own stream, the two events, the chain words
// and the first-use probe, around the ChainLedger (chain_ledger.hpp) whose answers StepChain carries out.  Nothing else
// writes chain state.  TrackedStream is the main stream of a DeviceNlp: every use of it as a hipStream_t tells the
// ledger.
//
// The words (unsigned int, 64-byte apart): 0 / 16 / 32 / 48 = workgroups of the sweep through, last step whose sweep is
// complete, workgroups of the step kernel through, last step whose kernel is complete; 96, 97: the probe.
#pragma once

#include "chain_ledger.hpp"
#include "device_base.hpp"

namespace slpx {

class StepChain {
 public:
  StepChain() = default;
  StepChain(const StepChain&) = delete;
  StepChain& operator=(const StepChain&) = delete;
  // Waits for the sweep's stream and gives it and the events back.  DeviceNlp declares its StepChain before its
  // buffers, so this runs AFTER they are freed: a chained sweep still in flight when the system is destroyed (its step
  // threw) is waited for by the hipFree of the first buffer, which synchronizes the device, not here.
  ~StepChain();

  // Where the sweep of a step goes, on a system whose steps can chain, with every wait it needs already enqueued.
  struct Route {
    // NotChained: kernels of two streams do not run at once here (the probe; `mode` is unchained for good): an
    // ordinary sweep.  MainStream: the main stream as it is (raw: the sweep is the step's own launch).  Chained:
    // tape_stream(), the generated kernel linked by (words, wait_step, this_step), then sweep_launched().
    enum Kind { NotChained, MainStream, Chained } kind = NotChained;
    unsigned int* words = nullptr;
    unsigned int wait_step = 0, this_step = 0;
  };
  Route begin_sweep(hipStream_t main, LaunchModes& mode);
  void sweep_launched(unsigned int workgroups) { m_ledger.sweep_launched(workgroups); }
  hipStream_t tape_stream() const { return m_tape_stream; }

  // the step kernel's half of the hand-over
  ChainLedger::StepLink step_link() const { return m_ledger.step_link(); }
  unsigned int* words() const { return m_words.p; }
  bool sweep_pending() const { return m_ledger.pending(); }
  void step_launched(unsigned int workgroups) { m_ledger.step_launched(workgroups); }
  void twin_launched() { m_ledger.twin_launched(); }

  // TrackedStream: `main` is handed to somebody
  void main_stream_used(hipStream_t main) {
    if (m_ledger.main_stream_used()) {
      (void)hipEventRecord(m_sweep_ev, m_tape_stream);
      (void)hipStreamWaitEvent(main, m_sweep_ev, 0);
    }
  }
  void main_stream_replaced() { m_ledger.main_stream_replaced(); }

  // A chained step reported kLdltChainFailure: drain both streams, clear the words.  (The caller unchains the system.)
  void recover(hipStream_t main);
  int failures() const { return m_ledger.failures(); }
  void debug_break_next() { m_ledger.break_next(); }

  ChainLedger::Book save() const { return m_ledger.save(); }
  void restore(const ChainLedger::Book& b) { m_ledger.restore(b); }

 private:
  bool first_use(hipStream_t main);  // makes the stream, the events and the words; false: the probe's verdict
  void drain_and_clear(hipStream_t main);

  ChainLedger m_ledger;
  hipStream_t m_tape_stream = nullptr;
  hipEvent_t m_step_ev = nullptr;   // main stream -> sweep: the step kernel before a chained sweep signals no word
  hipEvent_t m_sweep_ev = nullptr;  // sweep -> main stream: a pending sweep in front of whatever else comes
  DevBuf<unsigned int> m_words;
};

struct TrackedStream {
  explicit TrackedStream(StepChain& c) : chain(c) {}
  hipStream_t s = nullptr;
  StepChain& chain;
  operator hipStream_t() const {
    chain.main_stream_used(s);
    return s;
  }
  TrackedStream& operator=(hipStream_t v) {
    s = v;
    chain.main_stream_replaced();
    return *this;
  }
  hipStream_t raw() const { return s; }
};

}  // namespace slpx
