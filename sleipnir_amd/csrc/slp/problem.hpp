// slp::Problem<double> — the user surface of the reference
// (include/sleipnir/optimization/problem.hpp:67-744) kept for the path's callers
// (ProblemF64 is the implementation, Problem<Scalar> at the end of this header the spelling):
// decision_variable(), minimize()/maximize(), subject_to(), solve(), add_callback().
// solve() compiles the model for the GPU (NewtonSystem) and runs the interior-point
// iteration around the device Newton step.
//
// Like the reference, solve() routes unconstrained problems to newton() and equality-only
// problems to sqp() (problem.hpp:335,403), everything else to interior_point() — all three on
// the same device Newton step (csrc/ipm.cpp).
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <fstream>
#include <functional>
#include <map>
#include <memory>
#include <optional>
#include <span>
#include <string>
#include <utility>
#include <vector>

#include "../ipm.hpp"
#include "../eq_batch.hpp"
#include "../fr_batch.hpp"
#include "../ipm_batch.hpp"
#include "../ipm_host.hpp"
#include "../newton.hpp"
#include "../sensitivity.hpp"
#include "../warm_start.h"
#include "variable.hpp"

namespace slp {

using ExitStatus = slpx::ExitStatus;
using Options = slpx::Options;
// slp::IterationInfo<Scalar> (solver/iteration_info.hpp:13): only fp64 exists
template <typename Scalar = double>
using IterationInfo = slpx::IterationInfo;
using SolveReport = slpx::SolveReport;

// util/spy.hpp:20-80: the file tools/spy.py plots — title, row label, column label (each a
// 32-bit little-endian length and the bytes), rows, columns, then per iteration the number of
// coordinates and (row, column, '+' | '-' | '0') for every stored entry, column by column.
class Spy {
 public:
  Spy(const std::string& filename, const std::string& title, const std::string& row_label,
      const std::string& col_label, int rows, int cols)
      : m_file{filename, std::ios::binary} {
    for (const std::string* text : {&title, &row_label, &col_label}) {
      write32le(static_cast<int32_t>(text->size()));
      m_file.write(text->data(), static_cast<std::streamsize>(text->size()));
    }
    write32le(rows);
    write32le(cols);
  }
  // the entries of `patterns` (same shape; values at V + offset, summed where two patterns meet)
  void add(std::initializer_list<std::pair<const slpx::CscPattern*, const double*>> patterns, int cols) {
    std::vector<std::map<int, double>> columns(static_cast<size_t>(cols));
    int32_t count = 0;
    for (const auto& [pat, values] : patterns)
      for (int c = 0; c < cols && c + 1 < static_cast<int>(pat->colptr.size()); ++c)
        for (int q = pat->colptr[c]; q < pat->colptr[c + 1]; ++q) {
          auto [it, fresh] = columns[c].try_emplace(pat->rowidx[q], 0.0);
          it->second += values[q];
          count += fresh;
        }
    write32le(count);
    for (int c = 0; c < cols; ++c)
      for (const auto& [row, value] : columns[c]) {
        write32le(row);
        write32le(c);
        m_file << (value > 0.0 ? '+' : value < 0.0 ? '-' : '0');
      }
    m_file.flush();
  }

 private:
  std::ofstream m_file;
  void write32le(int32_t num) {
    const unsigned char b[4] = {static_cast<unsigned char>(num), static_cast<unsigned char>(num >> 8),
                                static_cast<unsigned char>(num >> 16), static_cast<unsigned char>(num >> 24)};
    m_file.write(reinterpret_cast<const char*>(b), 4);
  }
};

class ProblemF64 {
 public:
  ProblemF64() noexcept = default;

  [[nodiscard]] VariableF64 decision_variable() {
    invalidate();
    m_decision_variables.emplace_back();
    return m_decision_variables.back();
  }

  // problem.hpp:91-104
  [[nodiscard]] VariableMatrixF64 decision_variable(int rows, int cols = 1) {
    invalidate();
    VariableMatrixF64 vars{detail::empty, rows, cols};
    for (int row = 0; row < rows; ++row)
      for (int col = 0; col < cols; ++col) {
        m_decision_variables.emplace_back();
        vars[row, col] = m_decision_variables.back();
      }
    return vars;
  }

  // FFI helper (no reference counterpart): make an already-created free VariableF64 a
  // decision variable of this problem.
  void adopt_decision_variable(const VariableF64& v) {
    invalidate();
    m_decision_variables.push_back(v);
  }

  // problem.hpp:118-140
  [[nodiscard]] VariableMatrixF64 symmetric_decision_variable(int rows) {
    invalidate();
    VariableMatrixF64 vars{detail::empty, rows, rows};
    for (int row = 0; row < rows; ++row)
      for (int col = 0; col <= row; ++col) {
        m_decision_variables.emplace_back();
        vars[row, col] = m_decision_variables.back();
        vars[col, row] = m_decision_variables.back();
      }
    return vars;
  }

  // The compiled system belongs to the model as it was when compile() ran: every change of
  // the model drops it (the reference rebuilds its evaluators in every solve(), problem.hpp:517-660).
  void minimize(const VariableF64& cost) {
    invalidate();
    m_f = cost;
  }
  void maximize(const VariableF64& objective) {
    invalidate();
    m_f = -objective;
  }
  void subject_to(const EqualityConstraintsF64& constraint) {
    invalidate();
    m_equality_constraints.insert(m_equality_constraints.end(), constraint.constraints.begin(),
                                  constraint.constraints.end());
  }
  void subject_to(const InequalityConstraintsF64& constraint) {
    invalidate();
    m_inequality_constraints.insert(m_inequality_constraints.end(),
                                    constraint.constraints.begin(), constraint.constraints.end());
  }

  ExpressionType cost_function_type() const { return m_f ? m_f->type() : ExpressionType::NONE; }
  ExpressionType equality_constraint_type() const { return max_type(m_equality_constraints); }
  ExpressionType inequality_constraint_type() const { return max_type(m_inequality_constraints); }

  template <typename F>
    requires requires(F cb, const slpx::IterationInfo& info) { { cb(info) } -> std::same_as<void>; }
  void add_callback(F&& callback) {
    m_iteration_callbacks.emplace_back([cb = std::forward<F>(callback)](const slpx::IterationInfo& info) {
      cb(info);
      return false;
    });
  }
  template <typename F>
    requires requires(F cb, const slpx::IterationInfo& info) { { cb(info) } -> std::same_as<bool>; }
  void add_callback(F&& callback) {
    m_iteration_callbacks.emplace_back(std::forward<F>(callback));
  }
  void clear_callbacks() { m_iteration_callbacks.clear(); }
  // problem.hpp:714-735: callbacks that survive clear_callbacks() and run after the others
  template <typename F>
    requires requires(F cb, const slpx::IterationInfo& info) { { cb(info) } -> std::same_as<void>; }
  void add_persistent_callback(F&& callback) {
    m_persistent_iteration_callbacks.emplace_back([cb = std::forward<F>(callback)](const slpx::IterationInfo& info) {
      cb(info);
      return false;
    });
  }
  template <typename F>
    requires requires(F cb, const slpx::IterationInfo& info) { { cb(info) } -> std::same_as<bool>; }
  void add_persistent_callback(F&& callback) {
    m_persistent_iteration_callbacks.emplace_back(std::forward<F>(callback));
  }

  // problem.hpp:281-679
  ExitStatus solve(const Options& options = Options{}, bool spy = false) { return solve_from(options, spy, nullptr); }
  // ... from a warm start (warm_start.h): the variables' values are x, `warm` the rest of the iterate in the user's
  // units — what iterate() returned after an earlier solve, typically of a neighbouring problem (set_parameters).
  ExitStatus solve(const Options& options, bool spy, const slpx::WarmStart& warm) { return solve_from(options, spy, &warm); }

  // The primal-dual iterate the last solve() ended at, in the user's units (warm_start.h): the duals are those of
  // f - y^T c_e - z^T c_i as written, whatever scaling the solve ran with.  (slack(), equality_duals(),
  // inequality_duals() keep returning the scaled ones.)
  struct Iterate {
    std::vector<double> x, s, y, z;
    double mu = 0.0;
  };
  bool has_iterate() const { return m_has_iterate; }
  Iterate iterate() const {
    if (!m_has_iterate) throw std::runtime_error("iterate: the problem has not been solved");
    const size_t m_e = m_y.size(), m_i = m_s.size();
    Iterate it;
    it.x = m_iterate_x;
    it.s.resize(m_i);
    it.y.resize(m_e);
    it.z.resize(m_i);
    const double d_f = m_scales[0];
    for (size_t j = 0; j < m_e; ++j) it.y[j] = slpx::warm_unscale_dual(m_y[j], m_scales[1 + j], d_f);
    for (size_t j = 0; j < m_i; ++j) {
      const double d = m_scales[1 + m_e + j];
      it.s[j] = slpx::warm_unscale_s(m_s[j], d);
      it.z[j] = slpx::warm_unscale_dual(m_z[j], d, d_f);
    }
    it.mu = slpx::warm_unscale_mu(m_warm_result.mu, d_f);
    return it;
  }
  // how many entries of the last solve's warm start the safeguard replaced or clamped (0 after a cold start)
  int warm_start_repaired() const { return m_warm_result.repaired; }

  // ---- solution sensitivities (sensitivity.hpp; include/slpx.h: solution sensitivities) ----
  // How the iterate() of the last solve() moves with the parameters (the order of parameters()), the iterate held as
  // the solve left it, everything in the user's units: iterate() + sensitivity_jvp(dp) is a warm start for the model
  // with parameters() + dp.  The first call compiles the extended structure (info.t_compile); calls between two solves
  // share one factorization (info.factorizations == 0 from the second on).  Every one throws before any solve, for a
  // model without parameters, after the parameters changed with no new solve, and without a device.  The status of
  // the solve is not judged: info.solve_status reports it.
  struct Sensitivities {
    std::vector<double> dx, ds, dy, dz;  // [n_p][n], [n_p][m_i], [n_p][m_e], [n_p][m_i]: row q = d(.)/dp_q
    slpx::SensitivityInfo info;
  };
  // every parameter's column: n_p solves
  Sensitivities sensitivity() {
    const slpx::Sensitivity::Point at = sensitivity_point();
    Sensitivities out;
    size_blocks(m_sys->structure(), m_iterate_parameters.size(), out.dx, out.ds, out.dy, out.dz);
    out.info.solve_status = m_iterate_status;
    m_sens->jacobian(at, out.dx.data(), out.ds.data(), out.dy.data(), out.dz.data(), out.info);
    return out;
  }
  // the tangent along dp [n_p], one solve: (dx, ds, dy, dz) as an Iterate with mu = 0
  Iterate sensitivity_jvp(std::span<const double> dp, slpx::SensitivityInfo* info = nullptr) {
    const slpx::Sensitivity::Point at = sensitivity_point();
    if (dp.size() != m_iterate_parameters.size()) throw std::runtime_error("sensitivity_jvp: wrong number of values in dp");
    Iterate d;
    size_blocks(m_sys->structure(), 1, d.x, d.s, d.y, d.z);
    slpx::SensitivityInfo local;
    local.solve_status = m_iterate_status;
    m_sens->jvp(at, dp.data(), d.x.data(), d.s.data(), d.y.data(), d.z.data(), local);
    if (info) *info = local;
    return d;
  }
  // (dx/dp)^T vx [n_p] for a cotangent vx [n] on x, one solve whatever n_p
  std::vector<double> sensitivity_vjp(std::span<const double> vx, slpx::SensitivityInfo* info = nullptr) {
    const slpx::Sensitivity::Point at = sensitivity_point();
    if (vx.size() != static_cast<size_t>(m_sys->structure().n)) throw std::runtime_error("sensitivity_vjp: wrong number of values in vx");
    slpx::SensCotangent c;
    c.vx = vx.data();
    return sensitivity_vjp_at(at, c, /*x_alone=*/true, info);
  }
  // Cotangents on the whole end iterate and on the optimal cost — cost: the value the solve reports, f as minimize()
  // or maximize() stored it, in the user's units.  An empty span is absent; at least one must be given.
  struct Cotangent {
    std::span<const double> x, s, y, z;  // [n], [m_i], [m_e], [m_i]
    std::span<const double> cost;        // [1]
  };
  // sum over the given blocks of (d block/dp)^T v_block, plus v_cost d cost/dp: [n_p], ONE solve whatever n_p and
  // whichever blocks (sens_plan.hpp: the adjoint).  With x alone: sensitivity_vjp(vx), bit for bit.
  std::vector<double> sensitivity_vjp(const Cotangent& v, slpx::SensitivityInfo* info = nullptr) {
    const slpx::Sensitivity::Point at = sensitivity_point();
    const slpx::SensCotangent c = cotangents_given(v.x, v.s, v.y, v.z, v.cost, 1, m_sys->structure(), "sensitivity_vjp",
                                                   ": wrong number of values in the cotangent on ", "");
    return sensitivity_vjp_at(at, c, /*x_alone=*/false, info);
  }
  // d cost/dp [n_p]: the cotangent 1 on the cost alone
  std::vector<double> cost_gradient(slpx::SensitivityInfo* info = nullptr) {
    const double one = 1.0;
    Cotangent v;
    v.cost = std::span<const double>(&one, 1);
    return sensitivity_vjp(v, info);
  }
  // M [n_p][n + m_e + m_i]: per parameter r_x = d(grad_x L)/dp_q, r_e = dc_e/dp_q, r_i = dc_i/dp_q at the iterate
  std::vector<double> sensitivity_rhs() {
    const slpx::Sensitivity::Point at = sensitivity_point();
    const auto& st = m_sys->structure();
    std::vector<double> M(m_iterate_parameters.size() * static_cast<size_t>(st.n + st.m_e + st.m_i));
    m_sens->unreduced(at, M.data());
    return M;
  }
  // Somebody else is about to use the problem's system (a caller's handle on it): the next sensitivity call evaluates
  // and factors again.
  void sensitivity_forget() {
    if (m_sens) m_sens->forget();
  }

  // ---- batched sensitivities (sensitivity.hpp: BatchSensitivity; include/slpx.h: batched sensitivities) ----
  // The same derivatives for `batch` iterates at once, instance b with respect to ITS parameter row: functions of the
  // rows they are given — what solve_batch(..., warm) returned in the user's units — not of any state of the problem,
  // since solve_batch leaves none.  They run on batch_system(batch) alone: the variables, the parameters, the batch-1
  // system's scaling and regularization memory and a kept single-problem sensitivity factorization are untouched, and a
  // following solve_batch keeps every bit.  An instance that cannot be differentiated does not throw: status says so
  // (sens_plan.hpp: kSensComputed, kSensSkipped, kSensNotFactored) and its output rows are NaN.  Calls with the same
  // rows share one factorization until the next solve_batch / restoration_steps_batch of that batch size.
  struct BatchIterate {
    std::span<const double> x, s, y, z, mu;  // [B][n], [B][m_i], [B][m_e], [B][m_i], [B]
  };
  struct BatchSensitivities {
    std::vector<double> dx, ds, dy, dz;  // the Jacobian: [B][n_p][n], ...; a product: [B][n], [B][m_i], [B][m_e], [B][m_i]
    std::vector<double> grad;            // the vjp: [B][n_p]
    std::vector<double> M;               // sensitivity_batch_rhs: [B][n_p][n + m_e + m_i]
    std::vector<int32_t> status;         // [B]
    std::vector<slpx::SensitivityInfo> info;  // [B]
  };
  BatchSensitivities sensitivity_batch(int batch, const BatchIterate& it, std::span<const double> params) {
    BatchCall c = batch_sensitivity_call(batch, it, params, "sensitivity_batch");
    BatchSensitivities out = c.outputs(c.n_p);
    m_batch_sens->jacobian(*c.sys, cost_root(), c.rows, out.dx.data(), out.ds.data(), out.dy.data(), out.dz.data(), out.status.data(),
                           out.info.data());
    return out;
  }
  BatchSensitivities sensitivity_batch_jvp(int batch, const BatchIterate& it, std::span<const double> params, std::span<const double> dp) {
    BatchCall c = batch_sensitivity_call(batch, it, params, "sensitivity_batch_jvp");
    if (dp.size() != c.B * c.n_p) throw std::runtime_error("sensitivity_batch_jvp: dp must have batch x n_p values");
    BatchSensitivities out = c.outputs(1);
    m_batch_sens->jvp(*c.sys, cost_root(), c.rows, dp.data(), out.dx.data(), out.ds.data(), out.dy.data(), out.dz.data(), out.status.data(),
                      out.info.data());
    return out;
  }
  BatchSensitivities sensitivity_batch_vjp(int batch, const BatchIterate& it, std::span<const double> params, std::span<const double> vx) {
    BatchCall c = batch_sensitivity_call(batch, it, params, "sensitivity_batch_vjp");
    if (vx.size() != c.B * c.n) throw std::runtime_error("sensitivity_batch_vjp: vx must have batch x n values");
    BatchSensitivities out = c.gradients();
    m_batch_sens->vjp(*c.sys, cost_root(), c.rows, vx.data(), out.grad.data(), out.status.data(), out.info.data());
    return out;
  }
  // the cotangents of a batch: rows per instance, an empty span is absent
  struct BatchCotangent {
    std::span<const double> x, s, y, z;  // [B][n], [B][m_i], [B][m_e], [B][m_i]
    std::span<const double> cost;        // [B]
  };
  BatchSensitivities sensitivity_batch_vjp(int batch, const BatchIterate& it, std::span<const double> params, const BatchCotangent& v) {
    BatchCall c = batch_sensitivity_call(batch, it, params, "sensitivity_batch_vjp");
    const slpx::SensCotangent sc = cotangents_given(v.x, v.s, v.y, v.z, v.cost, c.B, c.sys->structure(), "sensitivity_batch_vjp",
                                                    ": the cotangent on ", " must have batch rows of the model's size");
    BatchSensitivities out = c.gradients();
    m_batch_sens->vjp_full(*c.sys, cost_root(), c.rows, sc, out.grad.data(), out.status.data(), out.info.data());
    return out;
  }
  BatchSensitivities sensitivity_batch_rhs(int batch, const BatchIterate& it, std::span<const double> params) {
    BatchCall c = batch_sensitivity_call(batch, it, params, "sensitivity_batch_rhs");
    BatchSensitivities out;
    out.M.resize(c.B * c.n_p * (c.n + c.m_e + c.m_i));
    out.status.resize(c.B);
    m_batch_sens->unreduced(*c.sys, cost_root(), c.rows, out.M.data(), out.status.data());
    return out;
  }

 private:
  // the checks every batched sensitivity call makes, the batch system it runs on and the rows as the driver takes them
  struct BatchCall {
    slpx::NewtonSystem* sys = nullptr;
    slpx::BatchSensitivity::Rows rows;
    size_t B = 0, n = 0, m_e = 0, m_i = 0, n_p = 0;
    BatchSensitivities outputs(size_t columns) const {
      BatchSensitivities out;
      size_blocks(sys->structure(), B * columns, out.dx, out.ds, out.dy, out.dz);
      out.status.resize(B);
      out.info.resize(B);
      return out;
    }
    BatchSensitivities gradients() const {
      BatchSensitivities out;
      out.grad.resize(B * n_p);
      out.status.resize(B);
      out.info.resize(B);
      return out;
    }
  };
  // the four blocks of a result with `rows` rows: [rows][n], [rows][m_i], [rows][m_e], [rows][m_i]
  static void size_blocks(const slpx::NlpStructure& st, size_t rows, std::vector<double>& dx, std::vector<double>& ds, std::vector<double>& dy,
                          std::vector<double>& dz) {
    dx.resize(rows * st.n);
    ds.resize(rows * st.m_i);
    dy.resize(rows * st.m_e);
    dz.resize(rows * st.m_i);
  }
  // The cotangents of a call, `rows` rows per block (1: one problem), as the drivers take them: an empty span is absent,
  // at least one must be given, and one of the wrong size throws `who` + before + its name + after.
  static slpx::SensCotangent cotangents_given(std::span<const double> x, std::span<const double> s, std::span<const double> y,
                                              std::span<const double> z, std::span<const double> cost, size_t rows,
                                              const slpx::NlpStructure& st, const std::string& who, const char* before, const char* after) {
    const auto given = [&](std::span<const double> a, size_t count, const char* what) -> const double* {
      if (a.empty()) return nullptr;
      if (a.size() != rows * count) throw std::runtime_error(who + before + what + after);
      return a.data();
    };
    slpx::SensCotangent c;
    c.vx = given(x, st.n, "x");
    c.vs = given(s, st.m_i, "s");
    c.vy = given(y, st.m_e, "y");
    c.vz = given(z, st.m_i, "z");
    c.vcost = given(cost, 1, "the cost");
    if (!c.vx && !c.vs && !c.vy && !c.vz && !c.vcost) throw std::runtime_error(who + ": no cotangent");
    return c;
  }
  // the tail of both single-problem vjps: the gradient block, the info with the solve's status
  std::vector<double> sensitivity_vjp_at(const slpx::Sensitivity::Point& at, const slpx::SensCotangent& c, bool x_alone, slpx::SensitivityInfo* info) {
    std::vector<double> grad(m_iterate_parameters.size());
    slpx::SensitivityInfo local;
    local.solve_status = m_iterate_status;
    if (x_alone) m_sens->vjp(at, c.vx, grad.data(), local);
    else m_sens->vjp_full(at, c, grad.data(), local);
    if (info) *info = local;
    return grad;
  }
  NodeId cost_root() const { return m_f ? m_f->expr : slpx::kNull; }
  BatchCall batch_sensitivity_call(int batch, const BatchIterate& it, std::span<const double> params, const char* who) {
    const std::string name(who);
    if (batch <= 0 || batch > 65535) throw std::runtime_error(name + ": batch must be in 1 .. 65535 (one grid slice per instance)");
    slpx::NewtonSystem& model = compile();
    if (!model.has_device()) throw std::runtime_error(name + ": no HIP device");
    BatchCall c;
    const auto& st = model.structure();
    c.B = static_cast<size_t>(batch);
    c.n = st.n;
    c.m_e = st.m_e;
    c.m_i = st.m_i;
    c.n_p = st.parameter_nodes().size();
    if (c.n_p == 0) throw std::runtime_error(name + ": the model reaches no parameter");
    if (it.x.size() != c.B * c.n || it.s.size() != c.B * c.m_i || it.y.size() != c.B * c.m_e || it.z.size() != c.B * c.m_i ||
        it.mu.size() != c.B || params.size() != c.B * c.n_p)
      throw std::runtime_error(name + ": the iterate and parameter rows do not have batch x the model's sizes");
    c.sys = &batch_system(batch);
    c.rows = slpx::BatchSensitivity::Rows{batch, it.x.data(), it.s.data(), it.y.data(), it.z.data(), it.mu.data(), params.data()};
    if (!m_batch_sens) m_batch_sens = std::make_unique<slpx::BatchSensitivity>();
    return c;
  }
  void batch_sensitivity_forget(int batch) {
    if (m_batch_sens) m_batch_sens->forget(batch);
  }

  // the checks every sensitivity call makes, and where it differentiates
  slpx::Sensitivity::Point sensitivity_point() {
    if (!m_has_iterate) throw std::runtime_error("sensitivity: the problem has not been solved");
    if (!m_sys) throw std::runtime_error("sensitivity: the model was changed since the solve that produced the iterate");
    const std::vector<NodeId> nodes = m_sys->structure().parameter_nodes();
    if (nodes.empty()) throw std::runtime_error("sensitivity: the model reaches no parameter");
    auto& g = detail::G();
    for (size_t j = 0; j < nodes.size(); ++j)
      if (j >= m_iterate_parameters.size() || g.val[nodes[j]] != m_iterate_parameters[j])
        throw std::runtime_error("sensitivity: the parameters were changed since the solve that produced the iterate");
    if (!m_sys->has_device()) throw std::runtime_error("sensitivity: no HIP device");
    if (!m_sens) m_sens = std::make_unique<slpx::Sensitivity>(*m_sys, m_f ? m_f->expr : slpx::kNull);
    m_sens_iterate = iterate();
    return slpx::Sensitivity::Point{&m_sens_iterate.x, &m_sens_iterate.s, &m_sens_iterate.y, &m_sens_iterate.z, m_sens_iterate.mu,
                                    &m_iterate_parameters, &m_scales};
  }
  void remember_iterate_for_sensitivity(ExitStatus status) {
    m_iterate_status = static_cast<int>(status);
    m_iterate_parameters.clear();
    auto& g = detail::G();
    for (NodeId node : m_sys->structure().parameter_nodes()) m_iterate_parameters.push_back(g.val[node]);
  }

  ExitStatus solve_from(const Options& options, bool spy, const slpx::WarmStart* warm) {
    // (nothing given beside x: the cold start, as in a batch)
    if (warm && warm->s.empty() && warm->y.empty() && warm->z.empty() && warm->mu <= 0.0) warm = nullptr;
    m_has_iterate = false;
    sensitivity_forget();
    m_warm_result = slpx::WarmStartResult{};
    auto& g = detail::G();
    std::vector<double> x(m_decision_variables.size());
    for (size_t i = 0; i < x.size(); ++i) x[i] = m_decision_variables[i].value();

    // problem.hpp:304-313
    if (cost_function_type() <= ExpressionType::CONSTANT &&
        equality_constraint_type() <= ExpressionType::CONSTANT &&
        inequality_constraint_type() <= ExpressionType::CONSTANT) {
      return ExitStatus::SUCCESS;
    }

    compile();

    // get_bounds conflict test (util/bounds.hpp:55-190, problem.hpp:597-606)
    std::vector<double> V(m_sys->structure().nV);
    auto& dev = m_sys->device();
    dev.set_scaling(std::vector<double>(m_sys->structure().n_scales(), 1.0));
    std::vector<double> zeros_e(std::max<size_t>(1, m_equality_constraints.size()), 0.0);
    std::vector<double> ones_i(std::max<size_t>(1, m_inequality_constraints.size()), 1.0);
    dev.upload_x(x.data());
    dev.upload_duals(ones_i.data(), zeros_e.data(), ones_i.data());
    dev.sweep_full();
    dev.download_V(V.data());
    if (has_conflicting_bounds(V)) return ExitStatus::GLOBALLY_INFEASIBLE;

    // problem.hpp:615-616
    m_scales = slpx::compute_problem_scaling(m_sys->structure(), V);
    dev.set_scaling(m_scales);

    // problem.hpp:365-375, 453-470, 571-596: sparsity files of H (lower triangle of the Lagrangian's
    // Hessian), A_e, A_i — one record per iteration, written from a callback like the reference's
    std::vector<slpx::IterationCallback> callbacks = m_iteration_callbacks;
    callbacks.insert(callbacks.end(), m_persistent_iteration_callbacks.begin(), m_persistent_iteration_callbacks.end());
    std::unique_ptr<Spy> H_spy, A_e_spy, A_i_spy;
    if (spy) {
      const int n = static_cast<int>(x.size()), m_e = static_cast<int>(m_equality_constraints.size()),
                m_i = static_cast<int>(m_inequality_constraints.size());
      H_spy = std::make_unique<Spy>("H.spy", "Hessian", "Decision variables", "Decision variables", n, n);
      if (m_e || m_i) A_e_spy = std::make_unique<Spy>("A_e.spy", "Equality constraint Jacobian", "Constraints", "Decision variables", m_e, n);
      if (m_i) A_i_spy = std::make_unique<Spy>("A_i.spy", "Inequality constraint Jacobian", "Constraints", "Decision variables", m_i, n);
      callbacks.emplace_back([&](const slpx::IterationInfo& info) {
        const slpx::NlpStructure& st = info.structure ? *info.structure : m_sys->structure();
        const double* V = info.V.data();
        H_spy->add({{&st.Hf, V + st.off_Hf}, {&st.Hc, V + st.off_Hc}}, st.n);
        if (A_e_spy) A_e_spy->add({{&st.Ae, V + st.off_Ae}}, st.n);
        if (A_i_spy) A_i_spy->add({{&st.Ai, V + st.off_Ai}}, st.n);
        return false;
      });
    }

    // problem.hpp:335, 403, 512: the solver follows the kinds of constraints present
    ExitStatus status;
    if (m_equality_constraints.empty() && m_inequality_constraints.empty()) {
      m_s.clear();
      m_y.clear();
      m_z.clear();
      status = slpx::newton(*m_sys, m_scales, callbacks, options, x, &m_report);  // (a warm start: x only)
    } else if (m_inequality_constraints.empty()) {
      m_s.clear();
      m_z.clear();
      status = slpx::sqp(*m_sys, m_scales, callbacks, options, x, &m_y, &m_report, warm);
    } else {
      // (c_i at x0 for a warm start's slack repair: from the sweep at unit scales the scaling came from)
      status = slpx::interior_point(*m_sys, m_scales, callbacks, options, x, &m_s, &m_y, &m_z, &m_report, warm,
                                    V.data() + m_sys->structure().off_ci, &m_warm_result);
    }
    // problem.hpp:676
    for (size_t i = 0; i < x.size(); ++i) g.val[m_decision_variables[i].expr] = x[i];
    m_iterate_x = x;
    m_has_iterate = true;
    remember_iterate_for_sensitivity(status);
    return status;
  }

 public:

  bool has_callbacks() const { return !m_iteration_callbacks.empty() || !m_persistent_iteration_callbacks.empty(); }

  // `batch` instances of this problem from x0 = [batch][n] (decision-variable order), each as solve() would
  // run from that start (ipm_batch.hpp), all with the same options.  The variables' values are left as they
  // are.  The driver follows the kinds of constraints present, as solve() does (problem.hpp:335, 403, 512): Newton,
  // SQP (eq_batch.hpp) or interior point, every one of them a lockstep batch on the device.
  slpx::BatchSolveResult solve_batch(int batch, const double* x0, const Options& options) {
    return solve_batch(batch, x0, nullptr, options);
  }
  // ... and with params = [batch][n_p] (the order of parameters()): instance b is this problem with parameter row b,
  // solved from x0[b]; null: the problem as it is, exactly the overload above.  The rows live in a constant pool per
  // instance on the batch system (DeviceNlp::set_parameters) for the duration of the call: the variables' and the
  // parameters' values are left as they are, and the shared pool is in force again on return.
  // warm (null: every instance starts cold): the rest of each instance's first iterate in the user's units, and the
  // request for the end iterate in those units (batch_lockstep.hpp: BatchWarmStart).
  slpx::BatchSolveResult solve_batch(int batch, const double* x0, const double* params, const Options& options,
                                     const slpx::BatchWarmStart* warm = nullptr) {
    if (batch <= 0) throw std::runtime_error("solve_batch: batch must be positive");
    if (x0 == nullptr) throw std::runtime_error("solve_batch: x0 is null");
    if (has_callbacks()) throw std::runtime_error("solve_batch: the problem has callbacks registered");
    sensitivity_forget();  // (restoration hand-offs run on the batch-1 system)
    batch_sensitivity_forget(batch);
    auto& g = detail::G();
    const size_t B = static_cast<size_t>(batch), n = m_decision_variables.size(), m_e = m_equality_constraints.size(),
                 m_i = m_inequality_constraints.size();
    slpx::BatchSolveResult out;
    out.status.assign(B, ExitStatus::SUCCESS);
    out.x.assign(x0, x0 + B * n);
    out.s.assign(B * m_i, 0.0);
    out.y.assign(B * m_e, 0.0);
    out.z.assign(B * m_i, 0.0);
    out.cost.assign(B, m_f ? m_f->value() : 0.0);
    out.iterations.assign(B, 0);
    out.restorations.assign(B, 0);
    if (warm) {
      out.s_u.assign(B * m_i, 0.0);
      out.y_u.assign(B * m_e, 0.0);
      out.z_u.assign(B * m_i, 0.0);
      out.mu_u.assign(B, 0.0);
      out.repaired.assign(B, 0);
    }
    // problem.hpp:304-313
    if (cost_function_type() <= ExpressionType::CONSTANT && equality_constraint_type() <= ExpressionType::CONSTANT &&
        inequality_constraint_type() <= ExpressionType::CONSTANT)
      return out;
    std::vector<double> saved(n);
    for (size_t i = 0; i < n; ++i) saved[i] = g.val[m_decision_variables[i].expr];
    auto restore = [&] {
      for (size_t i = 0; i < n; ++i) g.val[m_decision_variables[i].expr] = saved[i];
    };
    compile();
    slpx::NewtonSystem& sys = batch_system(batch);
    const auto& st = sys.structure();
    auto& dev = sys.device();
    // per-instance parameters: a pool per instance on the batch system for this call; however the call ends, the
    // shared pool (the parameters' current values) is in force again on both systems
    std::vector<double> pv;
    if (params != nullptr) {
      const size_t n_p = st.parameter_nodes().size();
      if (n_p == 0) throw std::runtime_error("solve_batch: parameters given, but the model has none");
      pv.assign(params, params + B * n_p);
    }
    struct SharedPoolAgain {
      ProblemF64& p;
      slpx::NewtonSystem* batch_sys;
      void now() {
        if (batch_sys == nullptr) return;
        slpx::NewtonSystem* bsys = batch_sys;
        batch_sys = nullptr;
        p.install_current_parameters(*bsys);
        p.install_current_parameters(*p.m_sys);
      }
      ~SharedPoolAgain() {  // (an exception is on its way: a second one from here is dropped)
        try {
          now();
        } catch (...) {
        }
      }
    } shared_pool_again{*this, params != nullptr ? &sys : nullptr};
    if (params != nullptr) dev.set_parameters(pv.data(), /*per_instance=*/true);
    // get_bounds conflict test and problem scaling at each instance's x0 (problem.hpp:597-616), from one batched
    // sweep at unit scales
    std::vector<double> s1(B * std::max<size_t>(1, m_i), 1.0), y0(B * std::max<size_t>(1, m_e), 0.0);
    std::vector<double> V(B * st.nV);
    dev.upload_x(x0);
    dev.upload_duals(s1.data(), y0.data(), s1.data());
    dev.sweep_full();
    dev.download_V(V.data());
    const int ns = st.n_scales();
    std::vector<double> scales(B * ns);
    std::vector<uint8_t> run(B, 1);
    // (the test reads single-variable linear rows only: their coefficients do not depend on x0)
    // One model: one verdict, from the host graph as solve() reaches it.  Per-instance parameters: a bound x >= p is
    // another bound in every instance, so each instance's constant terms come from ITS V, and the verdict is its own.
    const bool conflict = params == nullptr && has_conflicting_bounds(std::vector<double>(V.begin(), V.begin() + st.nV));
    bool any_runs = false;
    for (size_t b = 0; b < B; ++b) {
      const std::vector<double> Vb(V.begin() + b * st.nV, V.begin() + (b + 1) * st.nV);
      const std::vector<double> sc = slpx::compute_problem_scaling(st, Vb);
      std::copy(sc.begin(), sc.end(), scales.begin() + b * ns);
      if (conflict || (params != nullptr && has_conflicting_bounds(Vb, x0 + b * n))) {
        out.status[b] = ExitStatus::GLOBALLY_INFEASIBLE;
        run[b] = 0;
        // (the cost an instance that is not solved reports: f at the variables' values — with ITS parameters)
        if (params != nullptr && m_f) out.cost[b] = cost_with_parameters(st.parameter_nodes(), pv.data() + b * (pv.size() / B));
      }
      any_runs = any_runs || run[b];
    }
    if (any_runs) {
      const std::vector<double> x0v(x0, x0 + B * n);
      const std::vector<double>* rows = params != nullptr ? &pv : nullptr;
      try {
        if (m_i > 0) slpx::interior_point_batch(sys, *m_sys, scales, options, x0v, run, out, m_batch_restoration, rows, warm);
        else if (m_e > 0) slpx::sqp_batch(sys, *m_sys, scales, options, x0v, run, out, m_batch_restoration, rows, warm);
        else slpx::newton_batch(sys, *m_sys, scales, options, x0v, run, out, rows, warm);
      } catch (...) {
        reinstall_scaling();
        throw;
      }
      reinstall_scaling();
    }
    shared_pool_again.now();
    restore();
    return out;
  }

  // feasibility_restoration (util/feasibility_restoration.hpp:347-628) from a caller-given
  // iterate, `steps` iterations of it, with the scaling solve() would use (at the variables'
  // current values): the seam the restoration parity tests compare with the oracle at.
  ExitStatus restoration_steps(const Options& options, std::vector<double>& x, std::vector<double>& s,
                               std::vector<double>& y, std::vector<double>& z, double mu, int steps) {
    auto& g = detail::G();
    sensitivity_forget();
    compile();
    std::vector<double> x0(m_decision_variables.size());
    for (size_t i = 0; i < x0.size(); ++i) x0[i] = g.val[m_decision_variables[i].expr];
    std::vector<double> V(m_sys->structure().nV);
    auto& dev = m_sys->device();
    dev.set_scaling(std::vector<double>(m_sys->structure().n_scales(), 1.0));
    std::vector<double> zeros_e(std::max<size_t>(1, m_equality_constraints.size()), 0.0);
    std::vector<double> ones_i(std::max<size_t>(1, m_inequality_constraints.size()), 1.0);
    dev.upload_x(x0.data());
    dev.upload_duals(ones_i.data(), zeros_e.data(), ones_i.data());
    dev.sweep_full();
    dev.download_V(V.data());
    m_scales = slpx::compute_problem_scaling(m_sys->structure(), V);
    m_has_iterate = false;  // (m_scales are no longer the last solve's)
    dev.set_scaling(m_scales);
    return slpx::feasibility_restoration_steps(*m_sys, m_scales, options, x, s, y, z, mu, steps, &m_report);
  }

  // how solve_batch() runs feasibility restoration: 0 the hand-off to the batch-1 system (default), 1 in lockstep on the
  // batch system (batch_lockstep.hpp)
  void set_batch_restoration(int mode) {
    if (mode != 0 && mode != 1) throw std::runtime_error("set_batch_restoration: mode must be 0 (hand-off) or 1 (lockstep)");
    m_batch_restoration = mode;
  }
  int batch_restoration() const { return m_batch_restoration; }

  // The batched twin of restoration_steps(): `steps` restoration iterations from each of `batch` iterates (x [B][n],
  // s [B][m_i], y [B][m_e], z [B][m_i], mu [B]), in lockstep on the batch system (fr_batch.hpp: restoration_phase), with
  // the one scaling restoration_steps() would use.  status [B]; stats: BatchRestorationStats of the phase.
  std::vector<ExitStatus> restoration_steps_batch(const Options& options, int batch, std::vector<double>& x,
                                                  std::vector<double>& s, std::vector<double>& y, std::vector<double>& z,
                                                  const std::vector<double>& mu, int steps, slpx::BatchRestorationStats& stats) {
    if (batch <= 0) throw std::runtime_error("restoration_steps_batch: batch must be positive");
    if (has_callbacks()) throw std::runtime_error("restoration_steps_batch: the problem has callbacks registered");
    sensitivity_forget();
    batch_sensitivity_forget(batch);
    auto& g = detail::G();
    compile();
    const auto& st = m_sys->structure();
    const size_t B = static_cast<size_t>(batch), n = st.n, m_e = st.m_e, m_i = st.m_i;
    if (x.size() != B * n || s.size() != B * m_i || y.size() != B * m_e || z.size() != B * m_i || mu.size() != B)
      throw std::runtime_error("restoration_steps_batch: wrong lengths");
    // the scaling of restoration_steps(): at the variables' current values
    std::vector<double> x0(n);
    for (size_t i = 0; i < n; ++i) x0[i] = g.val[m_decision_variables[i].expr];
    std::vector<double> V(st.nV);
    auto& dev = m_sys->device();
    dev.set_scaling(std::vector<double>(st.n_scales(), 1.0));
    std::vector<double> zeros_e(std::max<size_t>(1, m_e), 0.0), ones_i(std::max<size_t>(1, m_i), 1.0);
    dev.upload_x(x0.data());
    dev.upload_duals(ones_i.data(), zeros_e.data(), ones_i.data());
    dev.sweep_full();
    dev.download_V(V.data());
    m_scales = slpx::compute_problem_scaling(st, V);
    m_has_iterate = false;
    dev.set_scaling(m_scales);
    // c_e, c_i, g at every instance's x: one batched sweep at unit scales, scaled here as the tape would
    slpx::NewtonSystem& sys = batch_system(batch);
    auto& bdev = sys.device();
    std::vector<double> VB(B * st.nV), yb(std::max<size_t>(1, B * m_e), 0.0), sb(std::max<size_t>(1, B * m_i), 1.0);
    bdev.upload_x(x.data());
    bdev.upload_duals(sb.data(), yb.data(), sb.data());
    bdev.sweep_full();
    bdev.download_V(VB.data());
    std::vector<slpx::BatchRestorationRequest> requests(B);
    std::vector<int> iterations(B, 0);
    std::vector<SolveReport> reports(B);
    for (size_t b = 0; b < B; ++b) {
      slpx::BatchRestorationRequest& r = requests[b];
      r.b = static_cast<int>(b);
      r.scales = m_scales;
      r.mu = mu[b];
      r.x.assign(x.begin() + b * n, x.begin() + (b + 1) * n);
      r.s.assign(s.begin() + b * m_i, s.begin() + (b + 1) * m_i);
      r.y.assign(y.begin() + b * m_e, y.begin() + (b + 1) * m_e);
      r.z.assign(z.begin() + b * m_i, z.begin() + (b + 1) * m_i);
      std::vector<double> Vb(VB.begin() + b * st.nV, VB.begin() + (b + 1) * st.nV);
      for (int k = 0; k < st.nV; ++k)
        if (st.V_scale_idx[k] >= 0) Vb[k] *= m_scales[st.V_scale_idx[k]];
      slpx::ipm_host::VView cur{st, Vb};
      r.c_e.assign(cur.c_e(), cur.c_e() + m_e);
      r.c_i.assign(cur.c_i(), cur.c_i() + m_i);
      r.g = cur.g_dense();
      r.initial_violation = slpx::ipm_host::norm_1(r.c_e.data(), static_cast<int>(m_e));
      for (size_t j = 0; j < m_i; ++j) r.initial_violation += std::abs(r.c_i[j] - r.s[j]);
      r.outer_accepts = [](const slpx::FilterEntry&, double) { return false; };
      r.iterations = &iterations[b];
      r.rep = &reports[b];
    }
    slpx::BatchFrDevice frd(sys);
    stats = slpx::BatchRestorationStats{};
    try {
      slpx::restoration_phase(sys, *m_sys, frd, options, requests, steps, std::chrono::steady_clock::now(), stats);
    } catch (...) {
      reinstall_scaling();
      throw;
    }
    reinstall_scaling();
    std::vector<ExitStatus> status(B);
    for (size_t b = 0; b < B; ++b) {
      const slpx::BatchRestorationRequest& r = requests[b];
      status[b] = r.status;
      std::copy(r.x.begin(), r.x.end(), x.begin() + b * n);
      std::copy(r.s.begin(), r.s.end(), s.begin() + b * m_i);
      std::copy(r.y.begin(), r.y.end(), y.begin() + b * m_e);
      std::copy(r.z.begin(), r.z.end(), z.begin() + b * m_i);
    }
    return status;
  }

  // Compiles (once) the NLP for the device; exposed so harnesses can time setup
  // separately and drive the Newton step directly.
  slpx::NewtonSystem& compile(const slpx::NewtonOptions& opt = {}) {
    // Values of free Variables that are not decision variables ("parameters") are folded into
    // the compiled constants and the cached linear rows: a changed one means a new system.
    if (m_sys) {
      auto& g = detail::G();
      for (const auto& [node, value] : m_param_snapshot)
        if (g.val[node] != value) {
          invalidate();
          break;
        }
    }
    if (!m_sys) {
      std::vector<NodeId> xs, ce, ci;
      for (auto& v : m_decision_variables) xs.push_back(v.expr);
      for (auto& v : m_equality_constraints) ce.push_back(v.expr);
      for (auto& v : m_inequality_constraints) ci.push_back(v.expr);
      m_sys = std::make_unique<slpx::NewtonSystem>(detail::G(), xs, m_f ? m_f->expr : slpx::kNull, ce,
                                                   ci, opt);
      ++m_compile_count;
      m_param_snapshot.clear();
      for (const slpx::TapeProgram* prog : {&m_sys->structure().full, &m_sys->structure().values})
        for (const auto& [node, slot] : prog->params) m_param_snapshot.emplace_back(node, detail::G().val[node]);
    }
    return *m_sys;
  }
  // Why set_parameters() may rewrite constant slots instead of compiling again: a parameter's VALUE reaches the
  // compiled system through its slot in TapeProgram::consts and through nothing else.  The places where compile()
  // reads a node's value (every `.val[` under csrc/ outside slp/):
  //   * tape_compiler.cpp — the value of an OP_CONST node becomes a literal of the pool, the value of a free Variable
  //     that is no input becomes the initial content of a slot of ITS OWN (never shared with a literal), and the
  //     generated kernels never write such a slot's value into their source (tape_jit.cpp: `!any_param`);
  //   * nlp.cpp, linear_row_adjoints — the cached entries of a LINEAR row read the value of the OTHER operand of a
  //     product or of a divisor.  That operand is of type CONSTANT, or the row would not be LINEAR: a Variable is
  //     LINEAR whether a decision variable or not, LINEAR x LINEAR is QUADRATIC, a LINEAR divisor makes the row
  //     NONLINEAR (graph.hpp: mul, div) — both go through the tape.  A CONSTANT expression has no
  //     Variable under it, so no parameter;
  //   * nlp.cpp, the values baked into V_static_raw — roots and partial sums of type CONSTANT only, for the same
  //     reason free of parameters.  A root made of parameters alone (a bound p_lo <= p_hi) is LINEAR: on the tape;
  //   * capi.cpp — reads and writes of variables' values by the caller, not part of a compiled system.
  // The sparsity patterns, the KKT plan and the factorization plan depend on the graph's shape, never on a value.
  // What does read parameters' values OUTSIDE the compiled system is has_conflicting_bounds (the host graph, at
  // solve()): set_parameters() writes the values into the graph too, and solve_batch() with per-instance rows takes
  // each instance's bounds from its own V instead.
  //
  // The model's parameters: the free Variables that are not decision variables and that the cost or a constraint
  // reaches, in ascending node order — the order of every parameter vector here.  Compiles (once) if need be.
  std::vector<NodeId> parameters() { return compile().structure().parameter_nodes(); }
  // New values for all parameters, in place: the variables get them, and so do the constant slots of the compiled
  // system and of every batch system — nothing is compiled again (compile_count() stays), and handles to the system
  // stay valid.  Variable::set_value on a parameter, by contrast, is noticed by the next compile() and builds anew.
  void set_parameters(std::span<const double> values) {
    slpx::NewtonSystem& sys = compile();
    const std::vector<NodeId> nodes = sys.structure().parameter_nodes();
    if (values.size() != nodes.size()) throw std::runtime_error("set_parameters: wrong number of values");
    auto& g = detail::G();
    for (size_t j = 0; j < nodes.size(); ++j) g.val[nodes[j]] = values[j];
    for (auto& [node, value] : m_param_snapshot) value = g.val[node];
    install_current_parameters(sys);
    for (auto& [batch, bsys] : m_batch_sys)
      if (bsys) install_current_parameters(*bsys);
  }
  // how many times this problem built a system for solve() (compile()): what set_parameters() leaves alone
  int64_t compile_count() const { return m_compile_count; }
  // true when the next compile() / solve() will build a new system (handles from
  // slpx_problem_system taken before that are stale)
  bool needs_compile() const { return !m_sys; }
  // the system of the last compile(), null if the model changed since (or never compiled): nothing is built
  const slpx::NewtonSystem* compiled() const { return m_sys.get(); }

  const SolveReport& report() const { return m_report; }
  const VariableF64& cost() const { return *m_f; }
  const std::vector<VariableF64>& decision_variables() const { return m_decision_variables; }
  const std::vector<VariableF64>& equality_constraints() const { return m_equality_constraints; }
  const std::vector<VariableF64>& inequality_constraints() const { return m_inequality_constraints; }
  const std::vector<double>& scales() const { return m_scales; }
  const std::vector<double>& slack() const { return m_s; }
  const std::vector<double>& equality_duals() const { return m_y; }
  const std::vector<double>& inequality_duals() const { return m_z; }

 private:
  // solve_batch's restoration hand-off installs an instance's scaling on the batch-1 system: put the problem's back
  void reinstall_scaling() {
    if (!m_sys || !m_sys->has_device()) return;
    if (static_cast<int>(m_scales.size()) == m_sys->structure().n_scales()) m_sys->device().set_scaling(m_scales);
    else m_sys->device().set_scaling(std::vector<double>(m_sys->structure().n_scales(), 1.0));
  }

  // the batch system of solve_batch(): the same model compiled for `batch` instances, tape at unit scales
  slpx::NewtonSystem& batch_system(int batch) {
    auto& sys = m_batch_sys[batch];
    if (!sys) {
      std::vector<NodeId> xs, ce, ci;
      for (auto& v : m_decision_variables) xs.push_back(v.expr);
      for (auto& v : m_equality_constraints) ce.push_back(v.expr);
      for (auto& v : m_inequality_constraints) ci.push_back(v.expr);
      slpx::NewtonOptions opt;
      opt.batch = batch;
      sys = std::make_unique<slpx::NewtonSystem>(detail::G(), xs, m_f ? m_f->expr : slpx::kNull, ce, ci, opt);
    }
    return *sys;
  }

  void invalidate() {
    m_sens.reset();  // (it refers to m_sys)
    m_batch_sens.reset();  // (its extended systems are compiled from the same model)
    m_batch_sys.clear();
    m_sys.reset();
    m_param_snapshot.clear();
  }

  static ExpressionType max_type(const std::vector<VariableF64>& v) {
    ExpressionType t = ExpressionType::NONE;
    for (auto& e : v) t = std::max(t, e.type());
    return t;
  }

  // the parameters' current values (the graph's) into the one pool every instance of `sys` reads, which is then in
  // force: after set_parameters(), and after per-instance rows or one instance's row were installed for a batch
  void install_current_parameters(slpx::NewtonSystem& sys) {
    if (sys.has_device()) sys.device().refresh_params(detail::G());
  }

  // f at the variables' current values with `values` for the parameters `nodes` (which keep their own values)
  double cost_with_parameters(const std::vector<NodeId>& nodes, const double* values) {
    auto& g = detail::G();
    std::vector<double> saved(nodes.size());
    for (size_t j = 0; j < nodes.size(); ++j) {
      saved[j] = g.val[nodes[j]];
      g.val[nodes[j]] = values[j];
    }
    const double cost = m_f->value();
    for (size_t j = 0; j < nodes.size(); ++j) g.val[nodes[j]] = saved[j];
    (void)m_f->value();  // (values of interior nodes as they were)
    return cost;
  }

  // x0 (null: as solve() does it — the constant term of a bound row from the host graph, at the variables' and the
  // parameters' values there): the point V was swept at.  The constant term of row r is then c_i(x0) - coef x0[col],
  // from V alone: what an instance of a batch with parameters of its own has, and the graph has not.
  bool has_conflicting_bounds(const std::vector<double>& V, const double* x0 = nullptr) {
    const auto& st = m_sys->structure();
    auto& g = detail::G();
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<std::pair<double, double>> b(st.n, {-inf, inf});
    // row -> (count, col, value) from the CSC pattern of A_i
    std::vector<int> cnt(st.m_i, 0), col(st.m_i, -1);
    std::vector<double> coef(st.m_i, 0.0);
    for (int c = 0; c < st.n; ++c)
      for (int p = st.Ai.colptr[c]; p < st.Ai.colptr[c + 1]; ++p) {
        const int r = st.Ai.rowidx[p];
        ++cnt[r];
        col[r] = c;
        coef[r] = V[st.off_Ai + p];
      }
    bool conflict = false;
    for (int r = 0; r < st.m_i; ++r) {
      if (m_inequality_constraints[r].type() != ExpressionType::LINEAR || cnt[r] != 1) continue;
      double constant_term;
      if (x0 != nullptr) {
        constant_term = V[st.off_ci + r] - coef[r] * x0[col[r]];
      } else {
        const NodeId var = m_decision_variables[col[r]].expr;
        const double saved = g.val[var];
        g.val[var] = 0.0;
        constant_term = m_inequality_constraints[r].value();
        g.val[var] = saved;
      }
      const double detected = -constant_term / coef[r];
      auto& [lo, hi] = b[col[r]];
      if (coef[r] < 0.0 && detected < hi) hi = detected;
      else if (coef[r] > 0.0 && detected > lo) lo = detected;
      if (lo > hi) conflict = true;
    }
    return conflict;
  }

  std::vector<VariableF64> m_decision_variables;
  std::optional<VariableF64> m_f;
  std::vector<VariableF64> m_equality_constraints;
  std::vector<VariableF64> m_inequality_constraints;
  std::vector<slpx::IterationCallback> m_iteration_callbacks, m_persistent_iteration_callbacks;
  std::unique_ptr<slpx::NewtonSystem> m_sys;
  std::map<int, std::unique_ptr<slpx::NewtonSystem>> m_batch_sys;  // solve_batch(), keyed by the batch size
  int m_batch_restoration = 0;                                     // set_batch_restoration()
  std::vector<std::pair<NodeId, double>> m_param_snapshot;  // (parameter node, value the compiled system holds)
  int64_t m_compile_count = 0;                              // compile_count()
  std::vector<double> m_scales, m_s, m_y, m_z;
  // iterate(): x, the barrier parameter and the repair count of the last solve(); m_scales, m_s, m_y, m_z are its too
  // as long as m_has_iterate holds
  std::vector<double> m_iterate_x;
  slpx::WarmStartResult m_warm_result;
  bool m_has_iterate = false;
  // sensitivities: the extended system and its plan (made by the first call, dropped with m_sys), the parameters'
  // values and the status of the solve the iterate came from, and the iterate as a sensitivity call handed it down
  std::unique_ptr<slpx::Sensitivity> m_sens;
  std::unique_ptr<slpx::BatchSensitivity> m_batch_sens;  // the batched calls: plan, and an extended system per batch size
  std::vector<double> m_iterate_parameters;
  int m_iterate_status = 0;
  Iterate m_sens_iterate;
  SolveReport m_report;
};


// slp::Problem<Scalar> (include/sleipnir/optimization/problem.hpp:66-67): only double exists.
template <typename Scalar>
class Problem;
template <>
class Problem<double> : public ProblemF64 {
 public:
  using ProblemF64::ProblemF64;
};

}  // namespace slp
