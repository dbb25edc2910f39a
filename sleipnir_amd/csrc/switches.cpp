#include "switches.hpp"

#include <cstdlib>
#include <type_traits>

namespace slpx {

Switches Switches::from_environment() {
  Switches s;
  auto flag = [](const char* name, auto& v) {  // (bool: keeps its default when unset; optional: stays empty)
    if (const char* env = std::getenv(name)) v = env[0] != '0';
  };
  auto number = [](const char* name, auto& v) {
    if (const char* env = std::getenv(name)) v = static_cast<std::remove_cvref_t<decltype(*v)>>(std::atoi(env));
  };
  flag("SLPX_FUSE_LAUNCHES", s.fuse_launches);
  flag("SLPX_FUSE_KKT", s.fuse_kkt);
  flag("SLPX_FUSE_BACKSUB", s.fuse_backsub);
  flag("SLPX_FUSE_KKT_STORE", s.fuse_kkt_store);
  flag("SLPX_LDLT_MF", s.ldlt_mf);
  flag("SLPX_LDLT_IL", s.ldlt_il);
  flag("SLPX_CHAIN_TAPE", s.chain_tape);
  flag("SLPX_IPM_RESIDENT", s.ipm_resident);
  flag("SLPX_IPM_LOOKAHEAD", s.ipm_lookahead);
  flag("SLPX_IPM_PIPELINE", s.ipm_pipeline);
  flag("SLPX_TWIN", s.twin);
  flag("SLPX_IPM_RIDE", s.ipm_ride);
  flag("SLPX_MF_SOLVE", s.mf_solve);
  if (const char* env = std::getenv("SLPX_IL_MIN_BATCH")) s.il_min_batch = std::atoi(env);
  if (const char* env = std::getenv("SLPX_DENSE"))
    if (env[0] == '0' || env[0] == '1') s.dense = env[0] == '1';
  flag("SLPX_SINGLE_LAUNCH", s.single_launch);
  number("SLPX_TASK_ENTRIES", s.task_entries);
  number("SLPX_MF_THREADS", s.mf_threads);
  number("SLPX_RELAX_ZEROS", s.relax_zeros);
  number("SLPX_SN_MIN_WIDTH", s.sn_min_width);
  number("SLPX_MFMA_MIN_ENTRIES", s.mfma_min_entries);
  return s;
}

}  // namespace slpx
