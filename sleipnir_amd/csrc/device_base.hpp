// What DeviceNlp (device.hpp) and its linear solver DeviceLdlt (device_ldlt.hpp) are both made of: the error check,
// the plan arena and DevBuf, the plans on the device, the structs that ride in another kernel's launch (KktFuse,
// BacksubFuse), the scalars the interior-point kernels hand the host and the spin on a published word.
#pragma once

#include <chrono>

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "device_layout.h"
#include "kkt_plan.hpp"
#include "ldlt_symbolic.hpp"
#include "nlp.hpp"
#include "system_choice.hpp"

namespace slpx {

#define SLPX_HIP_CHECK(expr)                                                              \
  do {                                                                                    \
    hipError_t err__ = (expr);                                                            \
    if (err__ != hipSuccess)                                                              \
      throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(err__) +   \
                               " at " #expr);                                             \
  } while (0)

// The read-only plan arrays of a system (a hundred of them: tape tables, KKT maps, LDLT lists, task images) in a
// few large device allocations filled by ONE copy each, instead of a hipMalloc and a synchronous hipMemcpy per array
// (2-3 ms of a 7 ms upload at cart-pole N=1000): while an arena is the thread's current one (DeviceArena::Scope,
// DeviceNlp's constructor), DevBuf::upload() places its data in the arena — the device pointer is valid at once, the
// bytes arrive with commit(), before anything is launched.
class DeviceArena {
 public:
  DeviceArena() = default;
  DeviceArena(const DeviceArena&) = delete;
  DeviceArena& operator=(const DeviceArena&) = delete;
  ~DeviceArena() {
    for (Chunk& c : m_chunks)
      if (c.dev) (void)hipFree(c.dev);
  }
  void* place(const void* src, size_t bytes) {
    constexpr size_t kAlign = 256, kChunk = 2u << 20, kSlack = 128u << 10;  // (slack: kernels that request a padded round past an array's end)
    if (m_chunks.empty() || m_chunks.back().used + bytes + kSlack > m_chunks.back().cap) {
      Chunk c;
      c.cap = std::max(kChunk, bytes + 2 * kSlack);
      if (hipMalloc(reinterpret_cast<void**>(&c.dev), c.cap) != hipSuccess) throw std::runtime_error("slpx: hipMalloc of a plan arena failed");
      m_chunks.push_back(std::move(c));
    }
    Chunk& c = m_chunks.back();
    const size_t at = c.used;
    if (c.host.capacity() < c.cap) c.host.reserve(c.cap);
    if (c.host.size() < at + bytes) c.host.resize(at + bytes);
    std::memcpy(c.host.data() + at, src, bytes);
    c.used = (at + bytes + kAlign - 1) / kAlign * kAlign;
    return c.dev + at;
  }
  void commit() {
    for (Chunk& c : m_chunks) {
      if (c.host.size() > c.committed) {
        if (hipMemcpy(c.dev + c.committed, c.host.data() + c.committed, c.host.size() - c.committed, hipMemcpyHostToDevice) != hipSuccess)
          throw std::runtime_error("slpx: upload of a plan arena failed");
        c.committed = c.host.size();
      }
      if (&c != &m_chunks.back()) std::vector<char>().swap(c.host);
    }
    if (!m_chunks.empty()) {  // (the open chunk keeps no mirror either: later placements start a new one)
      std::vector<char>().swap(m_chunks.back().host);
      m_chunks.back().cap = m_chunks.back().used;
    }
  }
  static DeviceArena*& current() {
    static thread_local DeviceArena* arena = nullptr;
    return arena;
  }
  struct Scope {
    DeviceArena* prev;
    explicit Scope(DeviceArena* a) : prev(current()) { current() = a; }
    ~Scope() { current() = prev; }
  };

 private:
  struct Chunk {
    char* dev = nullptr;
    std::vector<char> host;  // mirror of [0, used) until commit()
    size_t used = 0, committed = 0, cap = 0;
  };
  std::vector<Chunk> m_chunks;
};

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  bool owned = true;  // false: a slice of a DeviceArena
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void swap(DevBuf& o) {
    std::swap(p, o.p);
    std::swap(n, o.n);
    std::swap(owned, o.owned);
  }
  void release() {
    if (p && owned) (void)hipFree(p);
    p = nullptr;
    n = 0;
    owned = true;
  }
  void alloc(size_t count) {
    release();
    n = count;
    if (count) SLPX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T)));
  }
  void upload(const std::vector<T>& h) {
    // (the small arrays — most of them — share an arena; a big one gains nothing from a second host copy)
    if (DeviceArena* arena = DeviceArena::current(); arena != nullptr && !h.empty() && h.size() * sizeof(T) <= (64u << 10)) {
      release();
      p = static_cast<T*>(arena->place(h.data(), h.size() * sizeof(T)));
      n = h.size();
      owned = false;
      return;
    }
    alloc(h.size());
    if (!h.empty()) SLPX_HIP_CHECK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  }
  void zero(hipStream_t s = nullptr) {
    if (n) SLPX_HIP_CHECK(hipMemsetAsync(p, 0, n * sizeof(T), s));
  }
};

struct LdltDev {
  const LdltTask* tasks;
  const int32_t* ent_src;
  const uint8_t* ent_flags;
  const uint16_t* ent_col;
  const uint32_t* ent_out;
  const uint32_t* ent_pair_ptr;
  const uint32_t* ent_contrib_ptr;
  const uint32_t* contrib_idx;
  const uint32_t* ext_dst;
  const uint32_t* lvl_ptr;
  const LdltPair* pairs;
  const uint32_t* col_perm;
  const uint32_t* col_lvl_ptr;
  const uint32_t* fwd_ptr;
  const uint32_t* fwd_contrib_ptr;
  const uint32_t* scontrib_idx;
  const LdltSolveItem* fwd_items;
  const uint32_t* sext_ptr;
  const uint32_t* sext_dst;
  const LdltSolveItem* sext_items;
  const uint32_t* bwd_ptr;
  const LdltSolveItem* bwd_items;
  const int32_t* perm;
  const uint32_t* round_ptr;  // n_rounds + 1, into tasks
  int n_rounds;
  // supernodes (ldlt_symbolic.hpp: LdltSn)
  const LdltSn* sn_desc;
  const uint32_t* sn_lvl_ptr;
  const uint32_t* col_sn;
  // the hot loops' own copies (one LDS word instead of two per level / per column):
  const uint32_t* lvl_pack;      // lvl_ptr | sn_lvl_ptr << 16
  const uint32_t* col_lvl_pack;  // col_lvl_ptr | sn_lvl_ptr << 16
  const uint2* bwd_range;        // per column {first item below its own chain, end}; shares col_off
  uint32_t clock_task;           // the task whose phase clocks are recorded (slpx_debug_ldlt_clocks); 0xffffffff: none
};

// n_bad bit of a chained step whose sweep / step kernel gave up waiting for the other (bounded spins)
constexpr int32_t kLdltChainFailure = 1 << 30;

struct LdltStats {   // one per batch item, written by the factor kernels
  int32_t n_pos, n_neg, n_zero, n_bad;  // n_bad: exactly-zero or non-finite pivots (+ 2^20 per hand-over that timed out; bit 30: kLdltChainFailure)
  unsigned long long min_abs_bits;      // bit pattern of min |D| (non-negative doubles order like integers)
};

struct KktDev {
  int n, m_e, m_i, dim, nnz_lhs;
  const int32_t* dptr;
  const int32_t* dsrc;
  const int32_t* pptr;
  const int32_t* pa;
  const int32_t* pb;
  const int32_t* pr;
  const int32_t* g_src;
  const int32_t* ae_colptr;
  const int32_t* ae_rowidx;
  const int32_t* ai_colptr;
  const int32_t* ai_rowidx;
  const int32_t* ai_rowptr;
  const int32_t* ai_col;
  const int32_t* ai_src;
  const int32_t* fast_src;
  int off_f, off_ce, off_ci, off_g, off_Ae, off_Ai;
};

// The KKT and LDLT plans on the device, like TapeDevice: the buffers, upload() from the host plan (the derived tables
// through the packers of device_images.hpp), view() = what the kernels take.
struct KktPlanDevice {
  DevBuf<int32_t> dptr, dsrc, pptr, pa, pb, pr, g_src, ae_colptr, ae_rowidx, ai_colptr, ai_rowidx, ai_rowptr, ai_col, ai_src,
      fast_src, diag_pos;
  int n = 0, m_e = 0, m_i = 0, dim = 0, nnz_lhs = 0;
  int off_f = 0, off_ce = 0, off_ci = 0, off_g = 0, off_Ae = 0, off_Ai = 0;
  void upload(const NlpStructure& s, const KktPlan& k);
  KktDev view() const;
};
struct LdltPlanDevice {
  DevBuf<LdltTask> tasks;
  DevBuf<int32_t> ent_src, perm;
  DevBuf<uint8_t> ent_flags;
  DevBuf<uint16_t> ent_col;
  DevBuf<uint32_t> ent_out, ent_pair_ptr, ent_contrib_ptr, contrib_idx, ext_dst, lvl_ptr, col_perm, col_lvl_ptr, fwd_ptr,
      fwd_contrib_ptr, scontrib_idx, sext_ptr, sext_dst, bwd_ptr, round_ptr;
  DevBuf<LdltPair> pairs;
  DevBuf<LdltSolveItem> fwd_items, sext_items, bwd_items;
  DevBuf<LdltSn> sn_desc;
  DevBuf<uint32_t> sn_lvl_ptr, col_sn, lvl_pack, col_lvl_pack;
  DevBuf<uint2> bwd_range;
  int n_rounds = 0;
  void upload(const LdltPlan& l);
  LdltDev view() const;  // (clock_task: nobody)
};

// Work that rides in another kernel's launch (one problem, single-launch factorization).  Every
// kernel boundary of a Newton step costs 1-2 us of idle GPU plus the consumer's start-up, and an
// assembly pass in front of the factorization is a chain of three dependent trips to memory
// with the result written out only to be gathered again; so
//  - KktFuse: the factorization's tasks evaluate the lhs / rhs entries they own straight from
//    the AD sweep's V (kkt_kernels.h: one more dependent load in their gather, no assembly pass,
//    no lhs / rhs in memory unless somebody asks: DeviceNlp::materialize_kkt); the tape's
//    separable sums, which only feed f, ride as n_blocks extra workgroups nobody waits for;
//  - BacksubFuse: the step's back-substitution (p_s, p_z; interior_point.hpp:479-480) is done by
//    the backward solve's tasks themselves.  The columns of a row of A_i are pairwise adjacent in
//    the lhs (A_i^T Sigma A_i), so they lie on one root path of the elimination tree: the task
//    that owns the DEEPEST of them has the others among its own columns or its ancestors', final
//    when it finishes.  Its rows (BsRow / BsTerm) are staged with its plan, their A_i, s, z, c_i
//    values fetched with the factor's values at the start, the ancestors' p with the fold-in —
//    nothing of it is left on the critical path.  The last workgroup of the launch also hands
//    the factorization's inertia counters to the host — at the START of the launch: the host
//    learns the verdict of the attempt while the solve is still running and has the next
//    launch queued by the time it ends.
// The static side of both — KktTerm, BsRow, BsTerm of device_layout.h — is made by build_inline_kkt and
// build_inline_backsub of device_images.cpp.
struct KktFuse {
  int inline_kkt = 0;
  int n_blocks = 0;  // separable sums riding along
  const double* V = nullptr;
  const double* s = nullptr;
  const double* y = nullptr;
  const double* z = nullptr;
  const double* mu = nullptr;
  // per entry of the factorization plan (same layout as LdltDev::ent_src): the V slot of a plain
  // copy (bit 30: negated), -1 a structural zero, <= -2 a sum: -(2 + (first term | count << 20)),
  // first term relative to the task's block
  const int32_t* ent_vsrc = nullptr;
  const uint4* terms = nullptr;        // KktTerm[], every task's block padded to 16 bytes
  const uint2* task_terms = nullptr;   // per task {offset of its block in uint4, its length in uint4}
  double* Vw = nullptr;
  double* store_lhs = nullptr;  // SLPX_FUSE_KKT_STORE=1 (tests): also write the evaluated system to memory
  double* store_rhs = nullptr;
  const NlpStructure::SumReduce* red = nullptr;
  const double* scales = nullptr;
};
struct BacksubFuse {
  int on = 0;
  const double* V = nullptr;
  const double* s = nullptr;
  const double* z = nullptr;
  const double* mu = nullptr;
  double* ps = nullptr;
  double* pz = nullptr;
  int off_ci = 0;
  const uint4* plan = nullptr;       // per task: BsRow[n_rows] (padded to 16 bytes), then BsTerm[]
  const uint4* task_plan = nullptr;  // per task {offset of its block in uint4, length in uint4, rows, uint4 of rows}
  const LdltStats* stats_src = nullptr;
  LdltStats* stats_host = nullptr;
  unsigned long long* seq_dev = nullptr;
  volatile unsigned long long* seq_host = nullptr;
};

struct IpmDirOut;
// the second attempt of a twin launch (ldlt_mf_twin_kernel), for the launch that takes the direction
struct IpmTwin {
  int mode = 0;  // 0: one attempt; 1: the policy loop's attempt and its delta x 10; 2: the unregularized attempt and the first guess; 3: the loop's attempt and its gamma x 10
  const double *p = nullptr, *ps = nullptr, *pz = nullptr;
  const LdltStats* stats = nullptr;
};
// ipm_lookahead_kernel (ipm_kernels.h): step sizes of the direction and the whole look-ahead iterate
struct IpmLookaheadArgs {
  int n = 0, m_e = 0, m_i = 0;
  const int32_t* g_src = nullptr;
  const double *V = nullptr, *in = nullptr, *s = nullptr, *y = nullptr, *z = nullptr, *p = nullptr, *ps = nullptr, *pz = nullptr,
               *mu = nullptr;
  double tau = 0.0;
  double *in_t = nullptr, *s_t = nullptr, *y_t = nullptr, *z_t = nullptr, *alpha_dev = nullptr;
  IpmDirOut* out = nullptr;
  const LdltStats* stats = nullptr;
  IpmTwin tw;
};

// Scalars the interior-point iteration kernels (ipm_kernels.h) hand to the host; the
// three blocks live side by side in pinned host memory and are written by the kernels.
struct IpmDirOut {
  double alpha_max, alpha_z, D_phi;
};
struct IpmTrialOut {
  double f, viol, logsum, finite;
};
struct IpmErrOut {
  // un-scaled quantities (kkt_error.hpp:216-251) for the termination test ...
  double dual_inf_u, sz_max_u, ce_inf_u, cis_inf_u, y1_u, z1_u;
  // ... and the scaled ones for the barrier-parameter test: ‖g − A_eᵀy − A_iᵀz‖∞,
  // min / max of s∘z, ‖c_e‖∞, ‖c_i − s‖∞, ‖y‖₁, ‖z‖₁
  double dual_inf, sz_min, sz_max, ce_inf, cis_inf, y1, z1;
  // filter entry of the current iterate: f, ‖c_e‖₁ + ‖c_i − s‖₁, Σ ln s
  double f, viol, logsum;
  // local infeasibility: ‖A_eᵀc_e‖₂², ‖c_e‖₂², ‖A_iᵀc_i⁻‖₂², ‖c_i⁻‖₂²
  double aetce_sq, ce_sq, aitcp_sq, cp_sq;
  double x_inf, s_inf, finite, ci_all_pos;
};
struct IpmHost {
  IpmDirOut dir;
  IpmTrialOut trial;
  IpmErrOut err;
  IpmErrOut err_ahead;  // the same quantities at the look-ahead iterate (ipm_lookahead)
  double go;            // a deciding error launch (ipm_errors_deciding): 1.0 = the device took the iteration's decisions
  // A riding error launch (IpmErrFinish::ride_verdict) hands over its scalars WITHOUT a sequence number: `go` = +- its
  // ticket is the host's word that err_ahead is in — and writes from the device to host memory may pass each other on
  // the way (seen: one solve in 1 500 read a half-arrived err_ahead).  `check` = the exclusive-or of err_ahead's 24
  // words and of `go`: the host takes the hand-over when what it reads adds up (DeviceNlp::ipm_ride_wait).
  unsigned long long check;
};

struct StepTimings {
  float sweep = 0, assemble = 0, rhs = 0, factor = 0, solve = 0, backsub = 0, total = 0;
};

// Spin on a word a kernel publishes into pinned host memory.  The stream itself is consulted only after two
// milliseconds without progress (so that a failed launch cannot hang the host): a hipStreamQuery puts a marker packet
// behind whatever is queued, and the device spends ~5 us on it in front of the NEXT launch — measured as the gap
// before every step kernel while the loops asked every few microseconds (profiles/r06_gap_probe.txt).
template <class Done>
inline void spin_on_published(Done done, hipStream_t stream, const char* what) {
  unsigned spins = 0;
  bool timing = false;
  std::chrono::steady_clock::time_point since;
  while (!done()) {
    if ((++spins & 0x3fffu) != 0) continue;
    const auto now = std::chrono::steady_clock::now();
    if (!timing) {
      timing = true;
      since = now;
    } else if (now - since > std::chrono::milliseconds(2)) {
      since = now;
      const hipError_t st = hipStreamQuery(stream);
      if (st != hipErrorNotReady) {
        if (st != hipSuccess) throw std::runtime_error(std::string("slpx: ") + hipGetErrorString(st));
        if (!done()) throw std::runtime_error(what);
      }
    }
  }
}

}  // namespace slpx
