#include "system_choice.hpp"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

namespace slpx {

bool interleaved_for(int batch, const Switches& sw) { return sw.ldlt_il && batch >= sw.il_min_batch; }

LdltOptions choose_ldlt_options(const LdltOptions& base, int batch, int dim, bool compiled_model, const Switches& sw) {
  // One problem: big tasks = few rounds and levels (latency).  A batch is throughput bound
  // by how many tasks fit a CU's LDS at once: half-size tasks (~30 KB instead of ~60 KB)
  // put five instead of two workgroups on a CU and have fewer levels each.
  LdltOptions lopt = base;
  if (batch >= 16 && lopt.task_entries == LdltOptions{}.task_entries) lopt.task_entries = 1024;
  // one lane per problem (ldlt_il_kernels.h): a task's values x 64 problems must fit LDS
  // (measured at 512 x N=1000, ms per factorization: 192 -> 0.55 but some problems then need a
  // second attempt, 384 -> 0.67, 768 -> 0.79, 1024 -> 1.25)
  // (below ~200 problems the rounds, not the chip, bound a factorization: fewer, bigger tasks — 64 x N=500:
  // 384 entries 242 k steps/s, 512: 251 k, 768: 247 k)
  if (interleaved_for(batch, sw) && lopt.task_entries >= 1024) lopt.task_entries = batch < 192 ? 512 : 384;
  // the interleaved kernels walk column levels; supernodal levels are the per-task kernels'
  if (interleaved_for(batch, sw)) lopt.supernodal = false;
  if (!compiled_model) return lopt;
  // one problem: the multifrontal step (ldlt_mf_kernels.h) — every supernode a dense front, so a chain
  // of two columns already saves a level (the pair-list kernels' chain pass only paid from four)
  if (batch == 1 && lopt.supernodal && sw.ldlt_mf) {
    lopt.multifrontal = true;
    lopt.min_supernode_width = 2;
    lopt.relax_zeros = 8;
    lopt.balance_supernode_cuts = true;
    lopt.chain_from_deepest_child = true;
    lopt.chain_from_deepest_min_round = 0;
  }
  if (sw.relax_zeros) lopt.relax_zeros = *sw.relax_zeros;
  if (sw.sn_min_width) lopt.min_supernode_width = *sw.sn_min_width;
  if (sw.mfma_min_entries) lopt.mfma_min_entries = *sw.mfma_min_entries;
  // One problem (or a handful: the same plan, so that a small batch and single problems agree to
  // the bit), smaller than the BASELINE horizon: smaller tasks (less plan to stage per
  // task, shorter level passes, more of the chip in the leaf round) — task size with the square
  // root of the system's order.  Measured (fused kernel, us): cart-pole N=300 1024 entries 47.9
  // vs 2048 54.6; N=500 1536 52.3 vs 2048 53.8; N=1000 2048 56.2 vs 1792 59.4.
  if (batch < 16 && lopt.task_entries == LdltOptions{}.task_entries && dim < 9000) {
    const double scaled = 2048.0 * std::sqrt(static_cast<double>(dim) / 9000.0);
    lopt.task_entries = std::clamp<uint32_t>(256u * static_cast<uint32_t>(std::lround(scaled / 256.0)), 1024u, 2048u);
  }
  if (sw.task_entries) lopt.task_entries = *sw.task_entries;
  // One problem, all rounds in one launch: about 512 of the 1024-thread task workgroups are
  // resident at a time (two per CU).  A plan with more tasks than that serializes its tail
  // and usually has a round more than necessary; twice the task size fixes both (cart-pole
  // N=5000: 547 tasks / 4 rounds -> 265 / 3, factorization 73 -> 62 us, backward solve 42 -> 38;
  // at N=1000 the 137 tasks of the default are the better choice: 39 vs 45 us).
  // (more than ~250 tasks take two workgroups per CU, 80 KB of LDS each: there the chains-from-the-deepest-
  // child rule stays out of the leaf tasks, where it only adds fronts — tables, arena — to full levels:
  // cart-pole N=5000 58.6 us against 62.1 without the rule and 96 (not resident: two launches) with it everywhere)
  // Both rules are applied inside the build, after its first task partition (LdltOptions::single_problem_task_rules).
  lopt.single_problem_task_rules = batch == 1 && !sw.task_entries;
  return lopt;
}

// the fronts were not built (a limit of their addressing, or a refused plan): the pair-list kernels run this
// system, with THEIR tuning — chains from four columns, exact structures — not the fronts'
LdltOptions pair_list_options(const LdltOptions& base, const LdltOptions& chosen) {
  LdltOptions pair = base;
  pair.task_entries = chosen.task_entries;
  pair.supernodal = chosen.supernodal;
  pair.single_problem_task_rules = false;
  return pair;
}

void require_dense_factors_fit(int batch, int dim) {
  const double bytes = 8.0 * static_cast<double>(std::max(1, batch)) * dim * dim;
  if (bytes > 64.0 * (1u << 30))
    throw std::runtime_error("slpx: the dense factorization of " + std::to_string(batch) + " systems of order " + std::to_string(dim) +
                             " needs " + std::to_string(static_cast<long long>(bytes / (1u << 30))) +
                             " GB of factors; SLPX_DENSE=0 keeps the sparse plan (or refuses the model), a smaller batch fits");
}

LdltPlan choose_ldlt_plan(const CscPattern& lhs, int n_dec, bool reference_takes_dense, const std::vector<int32_t>* user_perm,
                          const std::vector<uint8_t>* diag_has_source, int batch, const LdltOptions& options,
                          const LdltOptions* pair_retry, const Switches& sw, std::string* dense_because) {
  const bool never_dense = sw.dense && !*sw.dense, plain_dense = sw.dense && *sw.dense;
  auto dense_plan = [&](bool pivoted) {
    require_dense_factors_fit(batch, lhs.cols);
    LdltPlan plan = build_dense_ldlt_plan(lhs, n_dec);
    plan.dense_pivoted = pivoted;
    return plan;
  };
  // The reference's own choice (interior_point.hpp:340-352, sqp.hpp:238-240, newton.hpp:133-135): a system whose lower
  // triangle fills a quarter of it or more — the small problems of its unit tests, single shooting — is factored
  // dense, with Eigen::LDLT's diagonal pivoting (ldlt_dense_pivoted_factor_kernel).  SLPX_DENSE=0: the sparse plan
  // whatever the fill (the sparse kernels do not pivot: D, and with it the regularization the policy settles on, may
  // then differ from the reference's on such a system); a caller's elimination order asks for the sparse plan too.
  if (reference_takes_dense && user_perm == nullptr && !never_dense && lhs.cols <= kReferenceDenseMaxOrder)
    return dense_plan(!plain_dense);  // (SLPX_DENSE=1 keeps meaning the plain dense kernel)
  // The sparse plan, or — where a column of L does not fit the LDS of a task (a Hessian dense in hundreds of
  // variables: single shooting), or SLPX_DENSE=1 asks for it — the dense one: the reference's dense branch
  // (util/dense_regularized_ldlt.hpp) instead of a refusal.
  auto sparse_or_dense = [&](const LdltOptions& lopt) {
    if (plain_dense && lhs.cols <= kDenseMaxOrder) return dense_plan(false);
    try {
      return build_ldlt_plan(lhs, n_dec, lopt, user_perm, diag_has_source);
    } catch (const std::runtime_error& e) {
      if (!ldlt_plan_error_is_too_big(e) || lhs.cols > kDenseMaxOrder || never_dense) throw;
      if (dense_because) *dense_because = e.what();
      return dense_plan(false);
    }
  };
  LdltPlan plan = sparse_or_dense(options);
  if (pair_retry && options.multifrontal && !plan.mf && !plan.dense) plan = sparse_or_dense(*pair_retry);
  return plan;
}

LaunchModes initial_launch_modes(int batch, const PlanFacts& plan, size_t n_sums, int cus, const Switches& sw) {
  LaunchModes m;
  // Chained steps (DeviceNlp::sweep_full_for_step): for one problem whose multifrontal step kernel leaves the sweep
  // room on the chip (at most CUs - 64 workgroups: cart-pole N=5000's 265 do not, and there chaining costs
  // 25 %, profiles/r03_chain_ab.txt).  SLPX_CHAIN_TAPE=0: off.  (Chosen before the tapes are uploaded: their kernel
  // is generated for it.)
  if (batch == 1 && plan.mf && static_cast<int>(plan.tasks + n_sums) + 64 <= cus) m.chain_mode = 1;
  if (!sw.chain_tape) m.chain_mode = 0;
  // Rounds in one launch pay off while every task of the launch is resident at once (a
  // single problem: 137 tasks on 256 CUs).  With a batch the later-round workgroups would
  // spin on CUs the earlier rounds of other problems are waiting for (measured at batch
  // 512: factorization 0.93 -> 4.2 ms), so batches keep one launch per round.
  m.dense = plan.dense;
  m.dense_pivoted = plan.dense && plan.dense_pivoted;
  m.il = !m.dense && interleaved_for(batch, sw);
  m.single_launch = !m.il && static_cast<size_t>(batch) * plan.tasks <= 1024;
  if (sw.single_launch) m.single_launch = *sw.single_launch;
  // launch fusion (device.hpp: KktFuse / BacksubFuse): one problem, single-launch factorization
  m.fuse_launches = m.single_launch && batch == 1 && plan.factor_lds_bytes >= 64 * sizeof(double) && sw.fuse_launches;
  m.fuse_kkt = m.fuse_launches && sw.fuse_kkt;
  m.fuse_backsub = m.fuse_launches && sw.fuse_backsub;
  m.fuse_kkt_store = sw.fuse_kkt_store;
  // hand-overs through the data: the factorization's update slots (ldlt_kernels.h: slot_take) where each has exactly
  // one reader, the backward solve's x (slot_read)
  m.slot_handoff = m.single_launch && plan.update_slots_have_one_reader;
  m.xg_by_data = m.single_launch;
  return m;
}

void note_inline_images(LaunchModes& m, bool kkt_ok, bool backsub_ok) {
  m.fuse_kkt = m.fuse_kkt && kkt_ok;              // (the stand-alone assembly kernels then)
  m.fuse_backsub = m.fuse_backsub && backsub_ok;  // (the stand-alone back-substitution kernel then)
}

// (one problem's factorization and solve in one launch: the multifrontal step; the pair-list kernels — batches,
// plans without fronts — take a launch per round and phase.  SLPX_LDLT_MF=0: the pair lists)
bool wants_multifrontal(const LaunchModes& m, const PlanFacts& plan, const Switches& sw) {
  return m.fuse_launches && m.fuse_backsub && m.fuse_kkt && plan.mf && sw.ldlt_mf;
}

void choose_multifrontal(LaunchModes& m, const PlanFacts& plan, size_t n_sums, const MfFit& fit, const Switches& sw) {
  if (!fit.declined) {
    bool fits = false;
    if (fit.lds_bytes <= 160u * 1024u) {
      // (the tables hold LDS byte addresses from 0: no static LDS in front of the dynamic block)
      auto resident = [&](size_t workgroups) { return fit.static_lds_bytes == 0 && plan.tasks + n_sums <= workgroups; };
      m.mf_mfma = plan.mf_n_mfma > 0;
      m.mf_threads = 1024;
      fits = resident(fit.step.at_1024);
      if (sw.mf_threads) fits = fits && *sw.mf_threads == 1024;
      if (!fits) {
        m.mf_threads = 512;
        fits = resident(fit.step.at_512);
      }
    }
    m.mf = fits;
    // new right-hand sides through the fronts (one launch: every task resident, as the step kernel's)
    m.mf_solve = m.mf && sw.mf_solve && plan.tasks <= (m.mf_threads == 1024 ? fit.solve.at_1024 : fit.solve.at_512);
  }
  m.fuse_solve = m.mf;
  m.chain_on = m.mf && m.chain_mode != 0;
}

bool twin_worth_measuring(const LaunchModes& m, int batch, const Switches& sw) {
  return sw.twin && m.mf && !m.mf_mfma && batch == 1 && m.xg_by_data && m.fuse_solve;
}

void choose_twin(LaunchModes& m, int batch, const PlanFacts& plan, size_t n_sums, const Residency& twin, const Switches& sw) {
  m.twin = -1;
  if (!twin_worth_measuring(m, batch, sw)) return;
  // both attempts' workgroups resident at once (their tasks wait for each other inside the launch)
  auto resident = [&](size_t workgroups) { return 2 * plan.tasks + n_sums <= workgroups; };
  // (a 1024-thread workgroup of the step kernels is alone on its CU — 98 VGPRs x 16 waves; cart-pole N=1000 has 137
  // tasks, twice that is more than the 256 CUs.  Workgroups of 512 threads fit two to a CU and run the same image
  // 0.5 us slower at that horizon, to the same bits: a launch of two attempts takes those where the wide ones do not fit)
  m.twin_threads = m.mf_threads;
  bool fits = resident(m.mf_threads == 1024 ? twin.at_1024 : twin.at_512);
  if (!fits && m.mf_threads == 1024) {
    m.twin_threads = 512;
    fits = resident(twin.at_512);
  }
  if (fits) m.twin = 1;
}

size_t riding_workgroups(const PlanFacts& plan, size_t n_sums) { return 2 * plan.tasks + 64 + n_sums; }

// (the tasks of both attempts AND the riding workgroups resident at once: a task that asks for the verdict must
// never keep a riding workgroup from being dispatched)
void choose_ride(LaunchModes& m, const PlanFacts& plan, size_t n_sums, size_t riding, const Switches& sw) {
  m.ride = sw.ipm_ride && riding_workgroups(plan, n_sums) <= riding ? 1 : 0;
}

}  // namespace slpx
