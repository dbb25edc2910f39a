// What crosses between the host drivers of the solvers — ipm.cpp (the interior-point dispatcher, its host-resident
// driver, interior_point()), ipm_resident.cpp (the device-resident, pipelined driver), ipm_restoration.cpp (feasibility
// restoration) and sqp_newton.cpp (SQP, Newton).  Internal: included by these four only, not installed.
#pragma once

#include <string>

#include "device.hpp"
#include "ipm.hpp"
#include "ipm_line_search.hpp"
#include "warm_start.h"

namespace slpx {

// interior_point.hpp:129-878: the iteration proper, on caller-owned iterates (the restoration phase of the reference
// re-enters it with in_feasibility_restoration = true).  ipm_core picks the driver: the device-resident one, or with
// SLPX_IPM_RESIDENT=0 the one that keeps the vectors on the host.
ExitStatus ipm_core(NewtonSystem& sys, const ipm_host::Vec& scales, const std::vector<IterationCallback>& callbacks,
                    const Options& options, bool in_feasibility_restoration, ipm_host::Vec& x, ipm_host::Vec& s, ipm_host::Vec& y,
                    ipm_host::Vec& z, double& mu, int& iterations, SolveReport& rep, ipm_host::clk::time_point solve_start);
ExitStatus ipm_core_host(NewtonSystem& sys, const ipm_host::Vec& scales, const std::vector<IterationCallback>& callbacks,
                         const Options& options, bool in_feasibility_restoration, ipm_host::Vec& x, ipm_host::Vec& s, ipm_host::Vec& y,
                         ipm_host::Vec& z, double& mu, int& iterations, SolveReport& rep, ipm_host::clk::time_point solve_start);
ExitStatus ipm_core_resident(NewtonSystem& sys, const ipm_host::Vec& scales, const std::vector<IterationCallback>& callbacks,
                             const Options& options, bool in_feasibility_restoration, ipm_host::Vec& x, ipm_host::Vec& s,
                             ipm_host::Vec& y, ipm_host::Vec& z, double& mu, int& iterations, SolveReport& rep,
                             ipm_host::clk::time_point solve_start);

// feasibility_restoration.hpp:347-628 (interior-point variant).  g = the outer problem's dense gradient at x.
ExitStatus feasibility_restoration(NewtonSystem& outer, const ipm_host::Vec& scales, const std::vector<IterationCallback>& user_callbacks,
                                   const std::function<bool(const FilterEntry&, double)>& outer_accepts, const Options& options,
                                   ipm_host::Vec& x, ipm_host::Vec& s, ipm_host::Vec& y, ipm_host::Vec& z, double mu, int& iterations,
                                   SolveReport& rep, ipm_host::clk::time_point solve_start, const ipm_host::Vec& c_e,
                                   const ipm_host::Vec& c_i, const ipm_host::Vec& g, double initial_violation);

// a warm start's blocks (ipm.hpp: WarmStart): an absent block is empty, a present one has the problem's length; no NaN, no Inf
inline void check_warm_length(const ipm_host::Vec& v, int want, const char* what) {
  if (!v.empty() && static_cast<int>(v.size()) != want)
    throw std::runtime_error(std::string("warm start: ") + what + " has the wrong length");
}
inline bool any_bad(const ipm_host::Vec& v) {
  for (double e : v)
    if (warm_bad(e)) return true;
  return false;
}

// The direction of the last solve, from the device: p = [p_x | -p_y] in one copy, and p_s, p_z where there are
// inequality rows.
inline void download_direction(DeviceNlp& dev, int n, int m_e, int m_i, ipm_host::Vec& p_x, ipm_host::Vec& p_y, ipm_host::Vec& p_s,
                               ipm_host::Vec& p_z) {
  ipm_host::Vec p(n + m_e);
  dev.download(dev.ldlt().d_p(), p.data(), n + m_e);
  p_x.assign(p.begin(), p.begin() + n);
  p_y.resize(m_e);
  for (int j = 0; j < m_e; ++j) p_y[j] = -p[n + j];
  if (m_i) {
    p_s.resize(m_i);
    p_z.resize(m_i);
    dev.download(dev.d_ps(), p_s.data(), m_i);
    dev.download(dev.d_pz(), p_z.data(), m_i);
  }
}

}  // namespace slpx
