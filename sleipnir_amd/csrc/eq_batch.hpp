// The device side of the batched SQP and Newton drivers: models without inequality constraints (batch_lockstep.hpp:
// the loop and the state every batched driver shares).
#pragma once

#include "batch_lockstep.hpp"

namespace slpx {

// What the SQP / Newton iterations add to BatchDevice (ipm_batch_launch.hip, kernels: eq_batch_kernels.h; the errors,
// scaling and input kernels of ipm_batch_kernels.h compute exactly what is needed here when m_i = 0): the direction
// (p_x, p_y), and stand-ins for what an iterate without inequality rows does not have.
struct BatchEqDevice : BatchDevice {
  explicit BatchEqDevice(NewtonSystem& sys);

  // an iterate here is (x, y): the base's set_iterate with the empty s and z
  using BatchDevice::set_iterate;
  void set_iterate(const std::vector<double>& x, const std::vector<double>& y) { set_iterate(x, {}, y, {}); }
  void direction(std::vector<double>& dphi);  // after compute(): keep p_x, p_y = -p[n..]; dphi [B] = g . p_x
  // trial point (x, y) + alpha d, d = Newton's (mode 0) or the correction's (mode 1), value sweep -> met [B][3]
  // (f, ||c_e||_1, count of non-finite f, c_e)
  void trial_values(std::vector<double>& met);
  void soc_step();  // second-order correction: rhs, solve on the instance's factor, its direction
  // KKT-error fallback: errors at the current point, then a full sweep at (x, y) + alpha p and its errors
  void kkt_fallback(std::vector<double>& err_cur, std::vector<double>& err_trial);
  void commit();

 private:
  friend struct BatchEqProbe;  // (the test-only probe, tests/support/eqbatchcheck.cpp, reads the buffers)
  DevBuf<double> m_px, m_py;     // Newton direction
  DevBuf<double> m_zero, m_none;  // the barrier parameter of the errors: none; s, z of an iterate: never read
  void launch_trial(int with_duals);
};

}  // namespace slpx
