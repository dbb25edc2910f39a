// The tapes of a DeviceNlp on the device: the two uploaded programs (full: values and derivatives; values: f, c_e,
// c_i only), the separable sums, the scaling vectors the sweeps apply, the parameter pools, and every launch of a tape
// kernel (device_tape.hip, the only file that includes tape_kernels.h and tape_ops.h).
//
// It knows nothing of the iterate, the KKT system or the chained-step protocol: what a sweep reads and writes, on which
// stream, with or without its sums, and how the generated kernel is linked to other kernels all come as arguments.
#pragma once

#include "device_base.hpp"

namespace slpx {

struct TrackedStream;  // step_chain.hpp

struct TapeDevice {
  DevBuf<TapeTask> tasks;
  DevBuf<uint32_t> small_list, large_list, global_list;
  DevBuf<uint32_t> leaf_src, node_rec, lvl_ptr, slot_edge_ptr, slvl_ptr, vout_src, vout_dst,
      jout_slot, jout_dst;
  DevBuf<int32_t> vout_scale, jout_scale;
  DevBuf<double> consts;
  // Per-instance parameters (DeviceTape::set_parameters): [batch][n_consts], the WHOLE pool of every instance —
  // parameter slots with the instance's values, literals replicated — allocated when per-instance values are first
  // installed; consts_stride = n_consts while it is in force, 0 while `consts` (shared) is.  Replicated rather than
  // split into "parameters per instance + literals shared": the kernels keep ONE base pointer, a leaf stays
  // "constant slot k" (no new leaf kind), and the leaf tables and generated index words do not change.
  DevBuf<double> consts_inst;
  uint32_t consts_stride = 0;
  DevBuf<TapeEdge> edges;
  DevBuf<uint16_t> node_rec16, slot_edge_ptr16, edges16;
  uint32_t n_small = 0, n_large = 0, n_global = 0;
  uint32_t small_lds = 0, large_lds = 0;
  uint64_t scratch_doubles = 0;
  bool basic_ops = false;
  // Tasks served by the run-time generated lane-per-task kernel (tape_jit.hpp); they are
  // NOT in the small/large lists above.  One launch covers every body: `tmpl_table[mode]`
  // (mode 0 = values only, 1 = with adjoints) holds (first block, instances, instance
  // offset, row-group mode) per body, `tmpl_blocks[mode]` the grid size.
  hipFunction_t tmpl_fn = nullptr;
  uint32_t tmpl_threads = 64;  // threads of a workgroup of tmpl_fn (TapeJitResult::block_threads)
  std::vector<unsigned char> tmpl_params;  // the model's numbers a generic code object reads (TemplateParams::blob)
  DevBuf<uint64_t> tmpl_params_dev;        // ... on the device: the kernel's last argument points here
  hipModule_t tmpl_mod = nullptr;
  uint32_t n_bodies = 0;
  DevBuf<uint32_t> tmpl_inst;  // per body: leaf bindings + output destinations, transposed (device_images.hpp: pack_template_tables)
  DevBuf<uint32_t> tmpl_table[2];
  uint32_t tmpl_blocks[2] = {0, 0};
  uint32_t n_templated_tasks = 0;
  bool tmpl_wide_for_chain = false;  // 256-thread workgroups only because the sweep runs beside the step kernel (tape_jit.cpp)
  double jit_seconds = 0.0;
  void upload(const TapeProgram& p, int batch, uint32_t n_unscaled_inputs, int chain_mode = 0);
  TapeDev view() const;
};

class DeviceTape {
 public:
  DeviceTape(const NlpStructure& s, int batch, const TrackedStream& stream) : m_s(s), m_batch(batch), m_stream(stream) {}
  DeviceTape(const DeviceTape&) = delete;
  DeviceTape& operator=(const DeviceTape&) = delete;

  // its share of the phases of DeviceNlp's constructor, called from that sequence
  void upload(int chain_mode);  // both programs (the full one's kernel is generated for the chain mode), the sums
  void raise_lds_limits();
  void alloc_scratch();
  // scales = [d_f, d_ce.., d_ci..]: applied to tape outputs, and d_ce / d_ci also to the dual inputs
  void set_scaling(const std::vector<double>& scales);

  enum Program { Full, Values };
  // How the generated kernel of a sweep is tied to other kernels:
  //   chain:   a chained step's sweep (step_chain.hpp) — the chain words, the total it waits for, its step number;
  //   skip_if: the kernel leaves at once when `flag` is set (the look-ahead chain's "rejected attempt" word).
  struct Link {
    enum Kind { None, Chain, SkipIf } kind = None;
    unsigned int* words = nullptr;
    unsigned int wait_step = 0, this_step = 0;
    static Link chain(unsigned int* words, unsigned int wait_step, unsigned int this_step) {
      return Link{Chain, words, wait_step, this_step};
    }
    static Link skip_if(unsigned int* flag) { return Link{SkipIf, flag, 0u, 0u}; }
  };
  struct Sweep {
    const double* in;    // [batch][n_inputs]
    double* V;           // [batch][nV]
    bool reduce;         // run the separable-sum reductions in this sweep
    hipStream_t stream;  // of every task class
    Link link;
  };
  // reverse: with the adjoint gather.  Returns grid x batch of the generated kernel (0 if the program has none).
  unsigned int launch(Program which, bool reverse, const Sweep& sweep);
  void reduce(double* V, hipStream_t stream);  // the separable sums on their own

  // one generated kernel is the whole full sweep (nothing interpreted beside it), in workgroups that share the chip
  // with the step kernel: what a chained step needs of the tape
  bool full_sweep_can_chain() const;
  bool full_has_generated_kernel() const { return m_full.n_bodies != 0; }
  const NlpStructure::SumReduce* reduces_dev() const { return m_reduces.p; }
  size_t n_reduces() const { return m_reduces.n; }
  const double* scales_dev() const { return m_scales.p; }

  // Re-reads the values of the tapes' parameter leaves (free Variables that are not decision variables) from the
  // graph and refreshes their constant slots.
  void refresh_params(const Graph& g);
  // Caller-given parameter values, in the order of NlpStructure::parameter_nodes() (ascending node id).
  // shared: values[n_p] into the parameter slots of the one pool every instance reads (and that pool is in force);
  // per instance: values[batch][n_p], instance b's row into its own pool (TapeDevice::consts_inst), in force until
  // the next shared install.  Buffers are rewritten in place: nothing that holds a pointer to them goes stale.
  void set_parameters(const double* values, bool per_instance);
  bool parameters_per_instance() const { return m_full.consts_stride != 0 || m_values.consts_stride != 0; }
  // bytes of the per-instance pools of both programs (0 until per-instance values were installed)
  size_t parameter_pool_bytes() const { return (m_full.consts_inst.n + m_values.consts_inst.n) * sizeof(double); }
  void debug_tape_clocks(unsigned long long* out16);
  // SLPX_TAPE_JIT_CLOCKS=1: 8 wall clocks (tape_jit.cpp) for each of the first `blocks` workgroups of the
  // generated kernel's last launch; returns the number of template workgroups, -1 if absent
  int debug_tmpl_clocks(unsigned long long* out, int blocks);

 private:
  const NlpStructure& m_s;
  const int m_batch;
  const TrackedStream& m_stream;  // DeviceNlp's: what the parameter pools and the debug reads synchronize with
  TapeDevice m_full, m_values;
  DevBuf<NlpStructure::SumReduce> m_reduces;
  DevBuf<double> m_in_scale, m_scales, m_scratch;
};

}  // namespace slpx
