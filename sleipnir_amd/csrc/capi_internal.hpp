// Definitions behind the opaque handles of include/slpx.h (shared with the
// test-only host checker in tests/support/).
#pragma once

#include <memory>

#include "newton.hpp"
#include "slp/problem.hpp"

struct slpx_system {
  std::unique_ptr<slpx::NewtonSystem> sys;
  slpx::NewtonSystem* ref = nullptr;
  // a handle from slpx_problem_system follows its problem: a model change (or a changed
  // parameter value) makes the problem compile a new system, and the handle resolves to that
  slp::Problem<double>* owner = nullptr;
  slpx::NewtonSystem& get() { return owner ? owner->compile() : *ref; }
};

struct slpx_problem {
  slp::Problem<double> problem;
  double t_compile = 0.0;
  // slpx_problem_batch_stats: the last slpx_problem_solve_batch (batch = 0: none yet)
  int64_t batch_stats[4] = {0, 0, 0, 0};
  // slpx_problem_batch_restoration_stats: of the last batch (solve or restoration steps)
  int64_t batch_restoration_stats[4] = {0, 0, 0, 0};
  bool batch_restoration_stats_valid = false;
  std::unique_ptr<slpx_system> borrowed;  // slpx_problem_system()
};
