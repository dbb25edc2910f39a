// TEST INFRASTRUCTURE ONLY — never linked into the product.
//
// The adjoint part of the sensitivity plan (csrc/sens_plan.hpp: g_src, fp_src, sens_host_adjoint_rhs,
// sens_host_vjp_full, sens_classify_extras) of a problem's model, made on the host exactly as senscheck.cpp makes the
// rest: the two maps and the patterns of the cost's gradient by name, and the two host executors on the caller's arrays.
// Nothing is checked here: tests/test_sensitivity_adjoint_cpu.py compares with dense numpy.  No device is touched.
#include <cstdint>
#include <cstdio>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../sleipnir_amd/csrc/capi_internal.hpp"
#include "../../sleipnir_amd/csrc/sens_plan.hpp"

using namespace slpx;

struct sa_handle {
  NlpStructure model, ext;
  SensPlan plan;
  std::map<std::string, std::vector<int32_t>> arrays;
  std::map<std::string, int64_t> scalars;
};

extern "C" {

sa_handle* sa_create(slpx_problem* p) {
  auto* h = new sa_handle();
  try {
    std::vector<NodeId> xs, ce, ci;
    for (auto& v : p->problem.decision_variables()) xs.push_back(v.expr);
    for (auto& v : p->problem.equality_constraints()) ce.push_back(v.expr);
    for (auto& v : p->problem.inequality_constraints()) ci.push_back(v.expr);
    const NodeId f = p->problem.cost_function_type() == slp::ExpressionType::NONE ? kNull : p->problem.cost().expr;
    h->model = build_nlp_structure(graph(), xs, f, ce, ci, TapeCompileOptions{});
    std::vector<NodeId> xp = xs;
    for (NodeId node : h->model.parameter_nodes()) xp.push_back(node);
    h->ext = build_nlp_structure(graph(), xp, f, ce, ci, TapeCompileOptions{});
    h->plan = build_sens_plan(h->model, h->ext);
    h->scalars = {{"model.off_g", h->model.off_g}, {"ext.off_g", h->ext.off_g}};
    h->arrays = {{"g_src", h->plan.g_src}, {"fp_src", h->plan.fp_src}, {"model.g.colptr", h->model.g_pat.colptr},
                 {"ext.g.colptr", h->ext.g_pat.colptr}};
  } catch (const std::exception& e) {
    std::fprintf(stderr, "sa_create: %s\n", e.what());
    delete h;
    return nullptr;
  }
  return h;
}

void sa_destroy(sa_handle* h) { delete h; }

int64_t sa_array(sa_handle* h, const char* name, const void** data) {
  const auto it = h->arrays.find(name);
  if (it == h->arrays.end()) return -1;
  *data = it->second.data();
  return static_cast<int64_t>(it->second.size());
}

int32_t sa_scalar(sa_handle* h, const char* name, int64_t* out) {
  const auto it = h->scalars.find(name);
  if (it == h->scalars.end()) return -1;
  *out = it->second;
  return 0;
}

// a null cotangent is absent
void sa_adjoint_rhs(sa_handle* h, const double* V, const double* s, const double* z, const double* vx, const double* vs, const double* vy,
                    const double* vz, const double* vcost, double* rhs) {
  sens_host_adjoint_rhs(h->plan, V, s, z, SensCotangent{vx, vs, vy, vz, vcost}, rhs);
}
void sa_vjp_full(sa_handle* h, const double* Vx, const double* M, const double* R, const double* s, const double* z, const double* w,
                 const double* vx, const double* vs, const double* vy, const double* vz, const double* vcost, double* grad) {
  sens_host_vjp_full(h->plan, Vx, M, R, s, z, w, SensCotangent{vx, vs, vy, vz, vcost}, grad);
}
// arrays [count] of rows [B][widths[k]] (a null one is not looked at) -> status [B]
void sa_classify_extras(int32_t B, int32_t count, const double* const* arrays, const int32_t* widths, int32_t* status) {
  std::vector<SensExtraRows> extras(static_cast<size_t>(count));
  for (int k = 0; k < count; ++k) extras[k] = SensExtraRows{arrays[k], widths[k]};
  sens_classify_extras(B, extras.data(), count, status);
}

}  // extern "C"
