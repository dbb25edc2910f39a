// The host's book of the chained-step protocol ("chained steps"), as plain C++: no HIP, no allocation.
// Its methods say what to do; StepChain (step_chain.hpp) does it.  tests/support/chaincheck_main.cpp drives it alone.
//
// The rule.  A chained sweep and a chained step kernel order themselves through words in memory.  Both count the
// workgroups they have launched of each kind since the words were last cleared:
//   sweep k waits until every workgroup of the chained STEP kernels so far is through (step_total), or — where the
//   step kernel before it was not a chained one — for an event and no word (wait_step 0);
//   step k waits until every workgroup of the chained SWEEPS so far, its own included, is through (sweep_total).
// Step numbers stay in [1, 2^30) and the totals below 2^29 (the kernels compare numbers as signed differences, use 0
// for "no wait", and keep bits 30, 31 of the words for the failure flag): before either bound is reached, one sweep
// goes to the main stream behind a drain of both streams, and the counts start again from zero.
#pragma once

#include <algorithm>

namespace slpx {

class ChainLedger {
 public:
  static constexpr unsigned int kStepNumberEnd = (1u << 30) - 1u;
  static constexpr unsigned int kTotalEnd = 1u << 29;
  static constexpr unsigned int kBrokenWait = 1u << 20;  // (debug break) step kernels nobody launched

  struct Sweep {
    // MainStream: behind everything the main stream holds.  Restart: drain both streams, clear the words, then the
    // main stream.  Chained: the sweep's own stream, with (wait_step, this_step).
    enum Where { MainStream, Restart, Chained } where = MainStream;
    // first of all, the chained sweep no step consumed is ordered in front of the main stream by an event
    bool order_pending = false;
    unsigned int wait_step = 0, this_step = 0;
    bool order_by_event = false;  // Chained behind a step kernel that signals no word: wait_step is 0
  };
  struct StepLink {
    bool chained = false;
    unsigned int wait_step = 0, this_step = 0;
  };
  // what a speculative launch may change and restore() puts back (DeviceNlp::LaunchBook); the step number and the
  // totals count what the device has been handed and never go back
  struct Book {
    bool last_step_chained, pending, touched;
  };

  // (tests) the totals start `headroom` workgroups below their bound, the step numbers at `seq`
  void start(unsigned int headroom, unsigned int seq = 0) {
    m_sweep_total = m_step_total = kTotalEnd - std::min(headroom, 1u << 28);
    m_seq = seq;
  }

  // The sweep of a step on a system whose steps can chain.
  Sweep begin_sweep() {
    Sweep s;
    if (m_pending) {
      // The last chained sweep was never consumed (its step threw before the step kernel was launched, or the caller
      // swept twice): no step kernel will signal the word a chained sweep would wait for.
      s.order_pending = main_stream_used();
      m_last_step_chained = false;
    }
    if (m_seq >= kStepNumberEnd || m_sweep_total >= kTotalEnd || m_step_total >= kTotalEnd) {
      // every ~14 hours of chained steps, one unchained step and a fresh count
      m_seq = 0;
      m_sweep_total = m_step_total = 0;
      m_last_step_chained = false;
      m_touched = false;
      s.where = Sweep::Restart;
      return s;
    }
    if (m_touched) {
      // Something else went to the main stream since the last step (an upload of the state, a download of the result,
      // another kernel): this step's sweep goes there too, behind all of it — the pattern of a caller that looks at
      // every step costs nothing extra.  Only steps that FOLLOW a step directly chain.
      m_touched = false;
      return s;
    }
    // the step kernel before this sweep: a chained one tells the sweep itself when its last workgroup is through; any
    // other (the first step of a run, a re-attempt of the policy loop) through an event, once
    s.where = Sweep::Chained;
    s.wait_step = m_step_total;
    if (!m_last_step_chained) {
      s.order_by_event = true;
      s.wait_step = 0;
    }
    if (m_break_next && s.wait_step != 0u) {
      m_break_next = false;
      s.wait_step += kBrokenWait;
    }
    s.this_step = ++m_seq;
    return s;
  }
  // a Chained sweep went out: pending until the step kernel that waits for it is launched
  void sweep_launched(unsigned int workgroups) {
    m_sweep_total += workgroups;
    m_pending = true;
  }

  // The step kernel launched now: chained where a chained sweep is pending.  (this_step is handed over either way.)
  StepLink step_link() const { return StepLink{m_pending, m_pending ? m_sweep_total : 0u, m_seq}; }
  // (a step's own launches leave the main stream alone: what step_link() said still holds)
  void step_launched(unsigned int workgroups) {
    if (m_pending) m_step_total += workgroups;
    m_last_step_chained = m_pending;
    m_pending = false;
  }
  void twin_launched() { m_pending = m_last_step_chained = false; }

  // Something is handed the main stream.  true: a chained sweep is in flight whose step kernel was not launched — the
  // main stream has to wait for it (an event) first.
  bool main_stream_used() {
    m_touched = true;
    const bool order = m_pending;
    m_pending = false;
    return order;
  }
  void main_stream_replaced() { m_touched = true; }

  // a chained step lost its hand-over: both streams are drained and the words cleared; the step numbers go on
  void failed() {
    m_sweep_total = m_step_total = 0;
    m_last_step_chained = m_pending = false;
    m_touched = true;
    ++m_failures;
  }
  // test hook: the next chained sweep that waits for a word waits for one nobody will write
  void break_next() { m_break_next = true; }

  Book save() const { return Book{m_last_step_chained, m_pending, m_touched}; }
  void restore(const Book& b) {
    m_last_step_chained = b.last_step_chained;
    m_pending = b.pending;
    m_touched = b.touched;
  }

  unsigned int step_number() const { return m_seq; }
  unsigned int sweep_total() const { return m_sweep_total; }
  unsigned int step_total() const { return m_step_total; }
  bool last_step_chained() const { return m_last_step_chained; }
  bool pending() const { return m_pending; }
  bool touched() const { return m_touched; }
  int failures() const { return m_failures; }

 private:
  unsigned int m_seq = 0;  // number of the last chained step
  // running totals of the workgroups of chained sweeps / chained step kernels launched: what the kernels wait for in
  // words 16 / 48
  unsigned int m_sweep_total = 0, m_step_total = 0;
  bool m_last_step_chained = false;  // the last step kernel launched signals its end through the words
  bool m_pending = false;            // a chained sweep is in flight and its step kernel has not been launched
  bool m_touched = true;             // something was handed the main stream since the last step
  bool m_break_next = false;
  int m_failures = 0;
};

}  // namespace slpx
