// TEST INFRASTRUCTURE ONLY — never linked into the product.
//
// The sensitivity plan (csrc/sens_plan.hpp) of a problem's model, made on the host exactly as csrc/sensitivity.hip makes
// it — the model's structure over x, the extended one over [x ; parameters], build_sens_plan — with the plan's arrays
// and the two structures' patterns handed out by name, and the host executor run on the caller's arrays.  Nothing is
// checked here: tests/test_sensitivity_plan_cpu.py compares with a dense numpy evaluation.  No device is touched.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../sleipnir_amd/csrc/capi_internal.hpp"
#include "../../sleipnir_amd/csrc/sens_plan.hpp"

using namespace slpx;

struct sc_handle {
  NlpStructure model, ext;
  SensPlan plan;
  std::map<std::string, std::vector<int32_t>> arrays;
  std::map<std::string, int64_t> scalars;
};

extern "C" {

sc_handle* sc_create(slpx_problem* p) {
  auto* h = new sc_handle();
  try {
    std::vector<NodeId> xs, ce, ci;
    for (auto& v : p->problem.decision_variables()) xs.push_back(v.expr);
    for (auto& v : p->problem.equality_constraints()) ce.push_back(v.expr);
    for (auto& v : p->problem.inequality_constraints()) ci.push_back(v.expr);
    const NodeId f = p->problem.cost_function_type() == slp::ExpressionType::NONE ? kNull : p->problem.cost().expr;
    h->model = build_nlp_structure(graph(), xs, f, ce, ci, TapeCompileOptions{});
    const std::vector<NodeId> params = h->model.parameter_nodes();
    std::vector<NodeId> xp = xs;
    xp.insert(xp.end(), params.begin(), params.end());
    h->ext = build_nlp_structure(graph(), xp, f, ce, ci, TapeCompileOptions{});
    h->plan = build_sens_plan(h->model, h->ext);
    const SensPlan& pl = h->plan;
    h->scalars = {{"n", pl.n}, {"n_p", pl.n_p}, {"m_e", pl.m_e}, {"m_i", pl.m_i}, {"dim", pl.dim}, {"dimM", pl.dimM}, {"nV", pl.nV},
                  {"nVx", pl.nVx}, {"model.off_Ai", h->model.off_Ai}, {"ext.off_Ae", h->ext.off_Ae}, {"ext.off_Ai", h->ext.off_Ai},
                  {"ext.off_Hf", h->ext.off_Hf}, {"ext.off_Hc", h->ext.off_Hc}, {"ext.parameters", static_cast<int64_t>(h->ext.parameter_nodes().size())},
                  {"model.full.shared_tasks", h->model.full.shared_tasks}, {"ext.full.shared_tasks", h->ext.full.shared_tasks}};
    {
      // the host part of the system csrc/sensitivity.hip makes of the extended model (its KKT plan and symbolic
      // factorization are never used, but they must build): everything up to the device
      NewtonSystem ext_system(graph(), xp, f, ce, ci, NewtonOptions{}, nullptr, /*defer_device=*/true);
      h->scalars["ext.system.dim"] = ext_system.kkt().dim;
      h->scalars["ext.system.has_device"] = ext_system.has_device() ? 1 : 0;
    }
    h->arrays = {{"m_ptr", pl.m_ptr}, {"m_src", pl.m_src}, {"red_ptr", pl.red_ptr}, {"red_src", pl.red_src}, {"red_row", pl.red_row},
                 {"ai_rowptr", pl.ai_rowptr}, {"ai_col", pl.ai_col}, {"ai_src", pl.ai_src},
                 {"model.Ai.colptr", h->model.Ai.colptr}, {"model.Ai.rowidx", h->model.Ai.rowidx},
                 {"ext.Ae.colptr", h->ext.Ae.colptr}, {"ext.Ae.rowidx", h->ext.Ae.rowidx},
                 {"ext.Ai.colptr", h->ext.Ai.colptr}, {"ext.Ai.rowidx", h->ext.Ai.rowidx},
                 {"ext.Hf.colptr", h->ext.Hf.colptr}, {"ext.Hf.rowidx", h->ext.Hf.rowidx},
                 {"ext.Hc.colptr", h->ext.Hc.colptr}, {"ext.Hc.rowidx", h->ext.Hc.rowidx}};
  } catch (const std::exception& e) {
    std::fprintf(stderr, "sc_create: %s\n", e.what());
    delete h;
    return nullptr;
  }
  return h;
}

void sc_destroy(sc_handle* h) { delete h; }

int64_t sc_array(sc_handle* h, const char* name, const void** data) {
  const auto it = h->arrays.find(name);
  if (it == h->arrays.end()) return -1;
  *data = it->second.data();
  return static_cast<int64_t>(it->second.size());
}

int32_t sc_scalar(sc_handle* h, const char* name, int64_t* out) {
  const auto it = h->scalars.find(name);
  if (it == h->scalars.end()) return -1;
  *out = it->second;
  return 0;
}

void sc_rhs(sc_handle* h, const double* Vx, const double* V, const double* s, const double* z, double* M, double* R) {
  sens_host_rhs(h->plan, Vx, V, s, z, M, R);
}
void sc_combine(sc_handle* h, const double* M, const double* R, const double* dp, double* rhs, double* r_i) {
  sens_host_combine(h->plan, M, R, dp, rhs, r_i);
}
void sc_expand(sc_handle* h, const double* V, const double* s, const double* z, const double* sol, const double* r_i, double* dx,
               double* ds, double* dy, double* dz) {
  sens_host_expand(h->plan, V, s, z, sol, r_i, dx, ds, dy, dz);
}
void sc_vjp(sc_handle* h, const double* R, const double* w, double* grad) { sens_host_vjp(h->plan, R, w, grad); }

}  // extern "C"
