// Solution sensitivities to the parameters (include/slpx.h: solution sensitivities): the derivative of the end
// iterate (x, s, y, z) of a solve with respect to the model's parameters, as a Jacobian, a Jacobian-vector product
// and a vector-Jacobian product.  sens_plan.hpp states the equations.
//
// What is new here is small: the derivative of the KKT residual with respect to the parameters — the EXTENDED
// structure, the model compiled once more with x' = [x ; p], whose tape is swept at the iterate — and the kernels of
// sensitivity.hip that gather it into right-hand sides and expand solutions.  Everything else is the model's own
// batch-1 system as it stands: its sweep and assembly at the iterate, NewtonSystem::compute() (the ordinary
// regularization policy loop), DeviceNlp::solve(), NewtonSystem::refine() and error_bounds().
//
// UNITS.  The model system is swept and assembled at UNIT scales with the iterate in the user's units (warm_start.h),
// and so is the extended one: the system that is factored, the right-hand sides and every output are in the user's
// units, whatever scaling the solve ran with.  The scaling the caller names is installed again afterwards.
//
// The extended system is a whole NewtonSystem (its KKT plan and symbolic factorization are made and never used: the
// shortest route, and the measured cost is in profiles/sensitivity.txt); it lives as long as the driver that made it,
// which the problem drops when the model is compiled again.
//
// TWO DRIVERS, ONE LAYER.  Sensitivity differentiates the problem's own iterate and throws where it cannot;
// BatchSensitivity differentiates B rows it is given and reports a status per instance.  The device work under both is
// written once (sensitivity.hip): the plan on the device (SensPlanDev), the extended system, the state of one system
// of B instances (SensState) and the stages that take it — gather after the sweeps, combine, adjoint right-hand side,
// vjp reduction, expand and download, factor from a cleared regularization memory, one round of solves.  The problem's
// own system is a state with B = 1.  What a driver owns is its contract: which rows it reads, what it does with the
// outcome of the factorization, and what it leaves on the model system.
#pragma once

#include <map>
#include <memory>
#include <vector>

#include "device.hpp"
#include "newton.hpp"
#include "sens_plan.hpp"

namespace slpx {

// slpx_sensitivity_info (include/slpx.h), of one call
struct SensitivityInfo {
  int32_t n_p = 0, solves = 0, factorizations = 0, refine_steps = 0;
  int32_t n_pos = 0, n_neg = 0, n_zero = 0;
  double delta = 0.0, gamma = 0.0;
  double berr_max = 0.0;
  int32_t solve_status = 0;
  double t_compile = 0.0, t_factor = 0.0, t_total = 0.0;
};

// the plan on the device: what the kernels of sensitivity.hip take (SensPlan's arrays by the same names)
struct SensDev {
  int n, n_p, m_e, m_i, dim, dimM;
  const int32_t *m_ptr, *m_src, *red_ptr, *red_src, *red_row, *ai_rowptr, *ai_col, *ai_src, *g_src, *fp_src;
};

// The plan and its tables on the device.  A function of the model alone: one serves every batch size.
struct SensPlanDev {
  SensPlan plan;
  DevBuf<int32_t> m_ptr, m_src, red_ptr, red_src, red_row, ai_rowptr, ai_col, ai_src, g_src, fp_src;
  bool built = false;
  // build_sens_plan of the two structures (the model's and the extended one's), uploaded
  void build(const NlpStructure& model, const NlpStructure& extended);
  SensDev view() const;
};

// The state of one system of B instances that is differentiated: its extended system over x' = [x ; p] and the working
// buffers, each with instance b's part at b times its size per instance.
struct SensState {
  int B = 0;
  int threads = 0;  // the workgroup size of the launches for this system: 256 for the problem's own, one wave for a batch system
  std::unique_ptr<NewtonSystem> ext;
  // M [n_p][dimM], R [n_p][dim]; the model's V, s, z at the iterate (copies: the model system's own are its caller's
  // again after a call); dp; the right-hand side and r_i of one product; grad [n_p]; the cotangents of the full vjp
  DevBuf<double> M, R, V, s, z, vec, rhs1, ri1, grad, cot;
  DevBuf<double> sol, dx, ds, dy, dz;  // `columns` solutions per instance and their expansion
  int columns = 0;
};

class Sensitivity {
 public:
  // Where the derivatives are taken: the iterate in the user's units, the parameters' values (the order of
  // NlpStructure::parameter_nodes()), and the scaling to leave on the model system.
  struct Point {
    const std::vector<double>*x, *s, *y, *z;
    double mu = 0.0;
    const std::vector<double>* parameters;
    const std::vector<double>* scales_after;
  };

  // `model`: the problem's batch-1 system, with its device; `f`: the cost's root (kNull: none).  Compiles the extended
  // structure for the model's device and builds and uploads the plan.  Throws where the model reaches no parameter.
  Sensitivity(NewtonSystem& model, NodeId f);
  ~Sensitivity();
  Sensitivity(const Sensitivity&) = delete;
  Sensitivity& operator=(const Sensitivity&) = delete;

  // seconds the constructor took; reported as t_compile by the first product and 0 afterwards
  double take_compile_seconds() {
    const double t = m_compile_seconds;
    m_compile_seconds = 0.0;
    return t;
  }

  // The model system was used by somebody else (a solve, a batch's hand-off, the caller's own handle), or the iterate
  // is another one: the next product sweeps, assembles and factors again.  Until then a product reuses what the last
  // one left — a Jacobian followed by a vjp factors once.
  void forget() { m_evaluated = m_factored = false; }

  // Any output may be null.  dx [n_p][n], ds [n_p][m_i], dy [n_p][m_e], dz [n_p][m_i]: one solve per parameter.
  void jacobian(const Point& at, double* dx, double* ds, double* dy, double* dz, SensitivityInfo& info);
  // The directional derivative along dp [n_p]: one solve.  dx [n], ds [m_i], dy [m_e], dz [m_i].
  void jvp(const Point& at, const double* dp, double* dx, double* ds, double* dy, double* dz, SensitivityInfo& info);
  // grad [n_p] = (dx/dp)^T vx for a cotangent vx [n] on x: one solve, K w = [vx; 0], then w^T R.  vjp_full with vx alone.
  void vjp(const Point& at, const double* vx, double* grad, SensitivityInfo& info);
  // grad [n_p] for cotangents on the whole iterate and on the cost (sens_plan.hpp: the adjoint; host arrays vx [n],
  // vs [m_i], vy [m_e], vz [m_i], vcost [1], null: absent, and one on rows the model does not have is ignored): ONE
  // solve, K w = [vx + A_i^T t + vcost g; -vy], then w^T R + t . r_i + vcost f_p.
  void vjp_full(const Point& at, const SensCotangent& v, double* grad, SensitivityInfo& info);
  // M [n_p][n + m_e + m_i]: r_x, r_e, r_i per parameter.  No factorization.
  void unreduced(const Point& at, double* M);

 private:
  void evaluate(const Point& at);
  void factor(const Point& at, SensitivityInfo& info);

  NewtonSystem& m_model;
  SensPlanDev m_plan;
  SensState m_state;  // B = 1, n_p columns
  double m_compile_seconds = 0.0;
  bool m_evaluated = false, m_factored = false;
  // of the factorization in memory (reported by every product that reuses it)
  int32_t m_n_pos = 0, m_n_neg = 0, m_n_zero = 0;
  double m_delta = 0.0, m_gamma = 0.0;
};

// The same derivatives for B iterates at once, instance b with respect to ITS parameter row (include/slpx.h: batched
// sensitivities): a function of the rows it is given, not of any state of the problem.  The expensive stages are the
// batch system's own (`model`: the problem's system compiled for B instances, tape at unit scales) — sweep, assemble,
// compute() with a mask and per-instance delta / gamma, solve(), refine() and error_bounds() with a mask; the extended
// system over [x ; p] is compiled once per batch size and kept here, where the parameters are variables: instance b's
// row is the tail of its x' row.  The plan and its device arrays are shared by every batch size.
//
// What a call leaves on `model`: the shared parameter pool with the parameters' current values (the graph's), as
// solve_batch leaves it, and the regularization memory it found.  The factorization stays in memory: a call with the
// same B and the same bits in every iterate and parameter row reuses it (factorizations == 0), until forget(B).
class BatchSensitivity {
 public:
  // B iterates in the user's units and their parameter rows: x [B][n], s [B][m_i], y [B][m_e], z [B][m_i], mu [B],
  // params [B][n_p].  s, y, z may be null where the row has no entries.
  struct Rows {
    int B = 0;
    const double *x = nullptr, *s = nullptr, *y = nullptr, *z = nullptr, *mu = nullptr, *params = nullptr;
  };

  BatchSensitivity() = default;
  BatchSensitivity(const BatchSensitivity&) = delete;
  BatchSensitivity& operator=(const BatchSensitivity&) = delete;

  // Somebody else used the batch system of that size (solve_batch, restoration_steps_batch): the next call of that size
  // evaluates and factors again.
  void forget(int batch);
  void forget_all();

  // `f`: the cost's root (kNull: none).  status [B] (sens_plan.hpp: kSensComputed, ...), info [B] (null: not wanted).
  // Rows of an instance whose status is not 0 are NaN in every output.  Any output may be null.
  // dx [B][n_p][n], ds [B][n_p][m_i], dy [B][n_p][m_e], dz [B][n_p][m_i]: n_p rounds of solves, round q column q of every instance
  void jacobian(NewtonSystem& model, NodeId f, const Rows& at, double* dx, double* ds, double* dy, double* dz, int32_t* status,
                SensitivityInfo* info);
  // dp [B][n_p] -> dx [B][n], ds [B][m_i], dy [B][m_e], dz [B][m_i]: one round
  void jvp(NewtonSystem& model, NodeId f, const Rows& at, const double* dp, double* dx, double* ds, double* dy, double* dz,
           int32_t* status, SensitivityInfo* info);
  // vx [B][n] -> grad [B][n_p]: one round.  vjp_full with vx alone.
  void vjp(NewtonSystem& model, NodeId f, const Rows& at, const double* vx, double* grad, int32_t* status, SensitivityInfo* info);
  // cotangents vx [B][n], vs [B][m_i], vy [B][m_e], vz [B][m_i], vcost [B] (null: absent) -> grad [B][n_p]: one round.
  // An instance with a value that is not finite in ANY given cotangent row is skipped (kSensSkipped).
  void vjp_full(NewtonSystem& model, NodeId f, const Rows& at, const SensCotangent& v, double* grad, int32_t* status,
                SensitivityInfo* info);
  // M [B][n_p][n + m_e + m_i]: neither factors nor solves
  void unreduced(NewtonSystem& model, NodeId f, const Rows& at, double* M, int32_t* status);

 private:
  // what belongs to one batch size: the state of its batch system, and what this driver knows about it
  struct PerBatch {
    SensState state;
    double compile_seconds = 0.0;
    bool evaluated = false, factored = false;
    std::vector<double> key;            // the rows `evaluated` / `factored` speak of: x, s, y, z, mu, params as given
    std::vector<int32_t> base_status;   // of those rows: classification, then kSensNotFactored from the factorization
    std::vector<SensitivityInfo> fact;  // per instance: inertia, delta, gamma of the factorization in memory
  };
  struct Call;  // one call's bookkeeping (sensitivity.hip)

  PerBatch& per_batch(NewtonSystem& model, NodeId f);
  // extras: the arrays beside the rows (dp; the cotangents), classified together and kept behind one another in c.extra;
  // columns: the solutions per instance the call needs room for
  void begin(Call& c, NewtonSystem& model, NodeId f, const Rows& at, const SensExtraRows* extras, int n_extras, int columns);
  void evaluate(Call& c);
  void factor(Call& c);
  void expand(Call& c, int columns, const double* r_i, long long r_i_column, long long r_i_instance, double* dx, double* ds, double* dy,
              double* dz);
  void finish(Call& c, int32_t* status, SensitivityInfo* info);

  SensPlanDev m_plan;  // built by the first call, shared by every batch size
  std::map<int, PerBatch> m_per_batch;
};

}  // namespace slpx
