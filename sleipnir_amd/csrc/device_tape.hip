// Every launch of a tape kernel, and the device half of the chained-step protocol.
//
//   tape_sweep     (tape_kernels.h) AD refresh: forward values + local partials, then
//                  the per-row adjoint gather, all inside LDS (one workgroup per task)
//                  replaces update_values/append_triplets/setFromTriplets
//                  (expression_graph.hpp:86-153, jacobian.hpp:134-156, hessian.hpp:132-157)
// and the run-time generated lane-per-task kernel (tape_jit.hpp) in front of it.  DeviceTape (device_tape.hpp) owns
// the uploaded programs and launches them; StepChain (step_chain.hpp) carries out what its ChainLedger answers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "device_images.hpp"
#include "device_tape.hpp"
#include "step_chain.hpp"
#include "tape_jit.hpp"
#include "tape_kernels.h"
#include "tape_ops.h"

namespace slpx {

// Separable sums on their own (tape_reduce_body, tape_kernels.h) — used when the reductions
// cannot ride along with the interpreted tail of the tape (DeviceTape::launch).
__global__ __launch_bounds__(64) void tape_reduce_kernel(const NlpStructure::SumReduce* __restrict__ red,
                                                         const double* __restrict__ scales,
                                                         double* __restrict__ V, int v_stride) {
  __shared__ double part[64];
  V += static_cast<size_t>(blockIdx.y) * v_stride;
  tape_reduce_body(red[blockIdx.x], scales, V, part, threadIdx.x);
}

// Can two kernels of this process run at once?  Chained steps (DeviceNlp::sweep_full_for_step) need the
// sweep and the step kernel resident together; a profiler collecting hardware counters (rocprofv3 --pmc)
// or AMD_SERIALIZE_KERNEL runs one kernel at a time, and a step kernel waiting for a sweep that cannot
// start would sit out its spin bound (seen: 247 ms per step under --pmc).  So, once per system: a kernel
// on the sweep's stream waits — a few milliseconds at most — for a word a kernel on the main stream sets.
__global__ void chain_probe_wait_kernel(unsigned int* w) {
  unsigned int seen = 0;
  for (int k = 0; k < 3000 && !seen; ++k) {
    seen = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_s_sleep(32);
  }
  w[1] = seen ? 1u : 2u;
}
__global__ void chain_probe_set_kernel(unsigned int* w) { __hip_atomic_store(w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ============================================================================
// DeviceTape
// ============================================================================

void TapeDevice::upload(const TapeProgram& p, int batch, uint32_t n_unscaled_inputs, int chain_mode) {
  tasks.upload(p.tasks);
  // families of structurally identical tasks and the big singles get a body in the
  // generated lane-per-task kernel; everything else is interpreted
  TapeJitOptions jit_opt;
  jit_opt.n_unscaled_inputs = n_unscaled_inputs;  // x: set_scaling leaves their factor at 1
  jit_opt.chain_mode = chain_mode;
  const TapeJitResult jit = build_tape_templates(p, jit_opt);
  jit_seconds = jit.compile_seconds;
  tmpl_fn = jit.fn;
  tmpl_params = jit.params;
  {
    std::vector<uint64_t> words((tmpl_params.size() + 7) / 8, 0);
    std::memcpy(words.data(), tmpl_params.data(), tmpl_params.size());
    tmpl_params_dev.upload(words);
  }
  tmpl_mod = jit.mod;
  tmpl_threads = jit.block_threads;
  n_bodies = static_cast<uint32_t>(jit.groups.size());
  n_templated_tasks = 0;
  tmpl_blocks[0] = tmpl_blocks[1] = 0;
  if (n_bodies) {
    const TemplateTables tt = pack_template_tables(p, jit.groups, batch, tmpl_threads);
    n_templated_tasks = tt.n_templated_tasks;
    tmpl_inst.upload(tt.inst);
    for (int m = 0; m < 2; ++m) {
      tmpl_table[m].upload(tt.table[m]);
      tmpl_blocks[m] = tt.blocks[m];
    }
  }
  auto interpreted = [&](const std::vector<uint32_t>& list) {
    std::vector<uint32_t> out;
    for (uint32_t ti : list)
      if (!jit.task_is_templated[ti]) out.push_back(ti);
    return out;
  };
  std::vector<uint32_t> small_rest = interpreted(p.small_tasks), large_rest = interpreted(p.large_tasks);
  uint32_t ride_lds = p.small_lds_bytes;
  tmpl_wide_for_chain = n_bodies && tmpl_threads == 256 && large_rest.empty() && chain_mode != 0;
  if (n_bodies && tmpl_threads == 256) {
    // (tape_jit.cpp: the generated kernel's workgroups are 256 threads: every interpreted task rides in its launch)
    small_rest.insert(small_rest.end(), large_rest.begin(), large_rest.end());
    large_rest.clear();
    ride_lds = std::max(p.small_lds_bytes, p.large_lds_bytes);
  }
  small_list.upload(small_rest);
  large_list.upload(large_rest);
  global_list.upload(p.global_tasks);
  if (std::getenv("SLPX_TAPE_JIT_VERBOSE") && jit.fn)
    std::fprintf(stderr, "slpx tape kernel: %zu bodies, %s code object (%zu bytes of model numbers), %.3f s\n",
                 jit.groups.size(), jit.specialized ? "specialized" : "generic", jit.params.size(), jit.compile_seconds);
  if (std::getenv("SLPX_TAPE_JIT_VERBOSE"))
    for (uint32_t ti : p.global_tasks)
      std::fprintf(stderr, "slpx tape GLOBAL task: leaf %u node %u slot %u vout %u jout %u levels %u+%u\n", p.tasks[ti].n_leaf,
                   p.tasks[ti].n_node, p.tasks[ti].n_slot, p.tasks[ti].n_vout, p.tasks[ti].n_jout, p.tasks[ti].n_lvl, p.tasks[ti].n_slvl);
  leaf_src.upload(p.leaf_src);
  // never empty: the generated bodies read consts[0] in lanes whose leaf is not a constant
  consts.upload(p.consts.empty() ? std::vector<double>{0.0} : p.consts);
  node_rec.upload(p.node_rec);
  lvl_ptr.upload(p.lvl_ptr);
  slot_edge_ptr.upload(p.slot_edge_ptr);
  slvl_ptr.upload(p.slvl_ptr);
  edges.upload(p.edges);
  vout_src.upload(p.vout_src);
  vout_dst.upload(p.vout_dst);
  vout_scale.upload(p.vout_scale);
  jout_slot.upload(p.jout_slot);
  jout_dst.upload(p.jout_dst);
  jout_scale.upload(p.jout_scale);
  node_rec16.upload(p.node_rec16);
  slot_edge_ptr16.upload(p.slot_edge_ptr16);
  edges16.upload(p.edges16);
  n_small = static_cast<uint32_t>(small_rest.size());
  n_large = static_cast<uint32_t>(large_rest.size());
  n_global = static_cast<uint32_t>(p.global_tasks.size());
  small_lds = ride_lds;
  large_lds = p.large_lds_bytes;
  scratch_doubles = p.global_scratch_doubles;
  basic_ops = p.basic_ops;
}

TapeDev TapeDevice::view() const {
  return TapeDev{tasks.p,         leaf_src.p,   consts_stride ? consts_inst.p : consts.p,   node_rec.p,   lvl_ptr.p,
                 slot_edge_ptr.p, slvl_ptr.p,   edges.p,    vout_src.p,   vout_dst.p,
                 vout_scale.p,    jout_slot.p,  jout_dst.p, jout_scale.p, node_rec16.p,
                 slot_edge_ptr16.p, edges16.p,  consts_stride};
}


void DeviceTape::upload(int chain_mode) {
  m_full.upload(m_s.full, m_batch, static_cast<uint32_t>(m_s.n), chain_mode);
  m_values.upload(m_s.values, m_batch, static_cast<uint32_t>(m_s.n));
  m_reduces.upload(m_s.reduces);
}

// allow > 64 KB dynamic LDS
void DeviceTape::raise_lds_limits() {
  for (const void* fn : {reinterpret_cast<const void*>(&tape_sweep_lds_kernel<256, true>),
                         reinterpret_cast<const void*>(&tape_sweep_lds_kernel<256, false>),
                         reinterpret_cast<const void*>(&tape_sweep_lds_kernel<64, true>),
                         reinterpret_cast<const void*>(&tape_sweep_lds_kernel<64, false>)})
    SLPX_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
}

void DeviceTape::alloc_scratch() {
  const uint64_t scratch = std::max(m_s.full.global_scratch_doubles, m_s.values.global_scratch_doubles);
  m_scratch.alloc(static_cast<size_t>(m_batch) * std::max<uint64_t>(1, scratch));
}

void DeviceTape::set_scaling(const std::vector<double>& scales) {
  const NlpStructure& s = m_s;
  m_scales.upload(scales);
  std::vector<double> in_scale(s.n_inputs(), 1.0);
  for (int j = 0; j < s.m_e; ++j) in_scale[s.n + j] = scales[1 + j];
  for (int j = 0; j < s.m_i; ++j) in_scale[s.n + s.m_e + j] = scales[1 + s.m_e + j];
  m_in_scale.upload(in_scale);
}

bool DeviceTape::full_sweep_can_chain() const {
  // (workgroups of single waves: g-fold's sweep, 256-thread workgroups interpreting its packs of rows, shares the
  // chip badly with the step kernel — 13.3 k steps/s chained against 13.6 k)
  const TapeDevice& t = m_full;
  return t.n_bodies > 0 && t.n_large == 0 && t.n_global == 0 && (t.tmpl_threads == 64 || t.tmpl_wide_for_chain);
}

// The task classes are independent launches on sweep.stream.
unsigned int DeviceTape::launch(Program which, bool reverse, const Sweep& sweep) {
  const TapeDevice& t = which == Full ? m_full : m_values;
  const TapeDev view = t.view();
  const int in_stride = m_s.n_inputs(), v_stride = m_s.nV;
  const unsigned long long sstride = m_scratch.n / m_batch;
  const double* in_p = sweep.in;
  double* V_p = sweep.V;
  const hipStream_t stream = sweep.stream;
  unsigned int generated_workgroups = 0;
  // basic_ops: the program only uses + - * / sin cos sqrt and the piecewise ops, so
  // the kernel specialization without pow/exp/log/erf/... (fewer VGPRs, less code)
  // generated template kernels: one lane per task instance (tape_jit.hpp)
  // interpreted 64-thread tasks ride along in the generated kernel's launch when there is one
  const bool small_rides = t.n_bodies > 0 && t.n_small > 0;
  if (t.n_bodies) {
    const int mode = reverse ? 1 : 0;
    const unsigned* table = t.tmpl_table[mode].p;
    int n_bodies = static_cast<int>(t.n_bodies);
    const unsigned* inst = t.tmpl_inst.p;
    const unsigned* leaf_src = view.leaf_src;
    const double* consts = view.consts;
    const double* in = in_p;
    int in_stride_arg = in_stride;
    const double* in_scale = m_in_scale.p;
    const double* scales = m_scales.p;
    double* V = V_p;
    int v_stride_arg = v_stride;
    const unsigned* vout_dst = view.vout_dst;
    const int* vout_scale = view.vout_scale;
    const unsigned* jout_dst = view.jout_dst;
    const int* jout_scale = view.jout_scale;
    TapeDev view_arg = view;
    const unsigned* task_list = t.small_list.p;
    int n_template_blocks = static_cast<int>(t.tmpl_blocks[mode]);
    int do_reverse = reverse ? 1 : 0;
    const uint64_t* params_dev = t.tmpl_params_dev.p;
    unsigned int* chain = sweep.link.words;
    unsigned int wait_step = sweep.link.wait_step, this_step = sweep.link.this_step;
    const unsigned grid = t.tmpl_blocks[mode] + (small_rides ? t.n_small : 0u);
    generated_workgroups = grid * static_cast<unsigned>(m_batch);
    // (`chain` with n_workgroups = 0 is the skip flag: tape_jit.cpp)
    unsigned int n_workgroups = sweep.link.kind == Link::SkipIf ? 0u : generated_workgroups;
    void* args[] = {&table,  &n_bodies, &inst,         &leaf_src, &consts,     &in,       &in_stride_arg,
                    &in_scale, &scales, &V,            &v_stride_arg, &vout_dst, &vout_scale, &jout_dst,
                    &jout_scale, &view_arg, &task_list, &n_template_blocks, &do_reverse,
                    &params_dev, &chain, &wait_step, &this_step, &n_workgroups};
    SLPX_HIP_CHECK(hipModuleLaunchKernel(t.tmpl_fn, grid, m_batch, 1, t.tmpl_threads, 1, 1, small_rides ? t.small_lds : 0u,
                                         stream, args, nullptr));
  }
  auto small_fn = t.basic_ops ? tape_sweep_lds_kernel<64, false> : tape_sweep_lds_kernel<64, true>;
  auto large_fn = t.basic_ops ? tape_sweep_lds_kernel<256, false> : tape_sweep_lds_kernel<256, true>;
  if (t.n_small && !small_rides)
    hipLaunchKernelGGL(small_fn, dim3(t.n_small, m_batch), dim3(64), t.small_lds, stream, view,
                       t.small_list.p, in_p, in_stride, m_in_scale.p, m_scales.p, V_p, v_stride,
                       reverse ? 1 : 0);
  if (t.n_large)
    hipLaunchKernelGGL(large_fn, dim3(t.n_large, m_batch), dim3(256), t.large_lds, stream, view,
                       t.large_list.p, in_p, in_stride, m_in_scale.p, m_scales.p, V_p, v_stride,
                       reverse ? 1 : 0);
  if (t.n_global)
    hipLaunchKernelGGL(tape_sweep_global_kernel, dim3(t.n_global, m_batch), dim3(1024), 0, stream,
                       view, t.global_list.p, in_p, in_stride, m_in_scale.p, m_scales.p, V_p,
                       v_stride, m_scratch.p, sstride, reverse ? 1 : 0);
  if (sweep.reduce) reduce(V_p, stream);
  SLPX_HIP_CHECK(hipGetLastError());
  return generated_workgroups;
}

void DeviceTape::reduce(double* V, hipStream_t stream) {
  if (m_reduces.n)
    hipLaunchKernelGGL(tape_reduce_kernel, dim3(static_cast<uint32_t>(m_reduces.n), m_batch), dim3(64), 0,
                       stream, m_reduces.p, m_scales.p, V, m_s.nV);
}

int DeviceTape::debug_tmpl_clocks(unsigned long long* out, int blocks) {
  SLPX_HIP_CHECK(hipStreamSynchronize(m_stream));
  hipDeviceptr_t p = nullptr;
  size_t bytes = 0;
  if (!m_full.tmpl_mod || hipModuleGetGlobal(&p, &bytes, m_full.tmpl_mod, "slpx_tmpl_clocks") != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  const size_t want = std::min<size_t>(bytes, static_cast<size_t>(blocks) * 8 * sizeof(unsigned long long));
  SLPX_HIP_CHECK(hipMemcpy(out, p, want, hipMemcpyDeviceToHost));
  return static_cast<int>(m_full.tmpl_blocks[1]);
}

void DeviceTape::debug_tape_clocks(unsigned long long* out16) {
  SLPX_HIP_CHECK(hipStreamSynchronize(m_stream));
  SLPX_HIP_CHECK(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_tape_clocks), 16 * sizeof(unsigned long long)));
}

void DeviceTape::refresh_params(const Graph& g) {
  std::vector<double> values;
  for (NodeId node : m_s.parameter_nodes()) values.push_back(g.val[node]);
  set_parameters(values.data(), /*per_instance=*/false);
}

void DeviceTape::set_parameters(const double* values, bool per_instance) {
  const std::vector<NodeId> nodes = m_s.parameter_nodes();
  if (nodes.empty()) {
    if (per_instance) throw std::runtime_error("slpx: set_parameters: the model has no parameters");
    return;
  }
  if (values == nullptr) throw std::runtime_error("slpx: set_parameters: values is null");
  SLPX_HIP_CHECK(hipStreamSynchronize(m_stream));  // (no sweep in flight reads the pool that is rewritten)
  const size_t n_p = nodes.size(), B = static_cast<size_t>(m_batch);
  auto install = [&](const TapeProgram& prog, TapeDevice& dev) {
    if (prog.params.empty()) return;
    const size_t nc = prog.consts.size();
    // where parameter j of the caller's vector sits in this program's pool (slot j: both programs claim
    // `param_order` first — looked up all the same, so that a program that reaches fewer parameters is served too)
    std::vector<std::pair<size_t, uint32_t>> slot_of;  // (j, slot)
    for (const auto& [node, slot] : prog.params) {
      const size_t j = static_cast<size_t>(std::lower_bound(nodes.begin(), nodes.end(), node) - nodes.begin());
      if (slot >= nc) throw std::runtime_error("slpx: set_parameters: a parameter slot outside the constant pool");
      slot_of.emplace_back(j, slot);
    }
    if (!per_instance) {
      std::vector<double> c = prog.consts;
      for (const auto& [j, slot] : slot_of) c[slot] = values[j];
      SLPX_HIP_CHECK(hipMemcpy(dev.consts.p, c.data(), nc * sizeof(double), hipMemcpyHostToDevice));
      dev.consts_stride = 0;
      return;
    }
    std::vector<double> c(B * nc);
    for (size_t b = 0; b < B; ++b) {
      std::copy(prog.consts.begin(), prog.consts.end(), c.begin() + b * nc);
      for (const auto& [j, slot] : slot_of) c[b * nc + slot] = values[b * n_p + j];
    }
    if (dev.consts_inst.n != c.size()) dev.consts_inst.alloc(c.size());
    SLPX_HIP_CHECK(hipMemcpy(dev.consts_inst.p, c.data(), c.size() * sizeof(double), hipMemcpyHostToDevice));
    dev.consts_stride = static_cast<uint32_t>(nc);
  };
  install(m_s.full, m_full);
  install(m_s.values, m_values);
  // (a program without parameters keeps its shared pool, stride 0, in either mode)
}

// ============================================================================
// StepChain
// ============================================================================

StepChain::~StepChain() {
  if (m_tape_stream) {
    (void)hipStreamSynchronize(m_tape_stream);
    (void)hipStreamDestroy(m_tape_stream);
  }
  if (m_step_ev) (void)hipEventDestroy(m_step_ev);
  if (m_sweep_ev) (void)hipEventDestroy(m_sweep_ev);
}

bool StepChain::first_use(hipStream_t main) {
  SLPX_HIP_CHECK(hipStreamCreateWithFlags(&m_tape_stream, hipStreamNonBlocking));
  SLPX_HIP_CHECK(hipEventCreateWithFlags(&m_step_ev, hipEventDisableTiming));
  SLPX_HIP_CHECK(hipEventCreateWithFlags(&m_sweep_ev, hipEventDisableTiming));
  {
    // (tests: the running totals start so far below their bound, so that a few thousand chained steps cross it —
    // SLPX_DEBUG_CHAIN_TOTALS_HEADROOM workgroups of headroom — and the restart of the counts is exercised)
    std::vector<unsigned int> words(128, 0u);
    if (const char* env = std::getenv("SLPX_DEBUG_CHAIN_TOTALS_HEADROOM")) {
      m_ledger.start(static_cast<unsigned int>(std::max(1L, std::atol(env))));
      words[16] = m_ledger.sweep_total();
      words[48] = m_ledger.step_total();
    }
    m_words.upload(words);
  }
  // (words 96, 97: the concurrency probe, see chain_probe_wait_kernel)
  hipLaunchKernelGGL(chain_probe_wait_kernel, dim3(1), dim3(1), 0, m_tape_stream, m_words.p + 96);
  hipLaunchKernelGGL(chain_probe_set_kernel, dim3(1), dim3(1), 0, main, m_words.p + 96);
  SLPX_HIP_CHECK(hipStreamSynchronize(m_tape_stream));
  SLPX_HIP_CHECK(hipStreamSynchronize(main));
  unsigned int verdict = 0;
  SLPX_HIP_CHECK(hipMemcpy(&verdict, m_words.p + 97, sizeof(verdict), hipMemcpyDeviceToHost));
  return verdict == 1u;
}

void StepChain::drain_and_clear(hipStream_t main) {
  if (m_tape_stream != nullptr) SLPX_HIP_CHECK(hipStreamSynchronize(m_tape_stream));
  SLPX_HIP_CHECK(hipStreamSynchronize(main));
  if (m_words.p != nullptr) SLPX_HIP_CHECK(hipMemset(m_words.p, 0, 64 * sizeof(unsigned int)));
}

StepChain::Route StepChain::begin_sweep(hipStream_t main, LaunchModes& mode) {
  if (m_tape_stream == nullptr && !first_use(main)) {
    unchain(mode);  // kernels run one at a time here: the sweep stays in the main stream
    if (std::getenv("SLPX_LDLT_VERBOSE")) std::fprintf(stderr, "slpx: kernels of two streams do not run at once here: steps are not chained\n");
    return Route{};
  }
  const ChainLedger::Sweep s = m_ledger.begin_sweep();
  if (s.order_pending) {
    SLPX_HIP_CHECK(hipEventRecord(m_sweep_ev, m_tape_stream));
    SLPX_HIP_CHECK(hipStreamWaitEvent(main, m_sweep_ev, 0));
  }
  if (s.where == ChainLedger::Sweep::Restart) drain_and_clear(main);
  if (s.where != ChainLedger::Sweep::Chained) return Route{Route::MainStream};
  if (s.order_by_event) {
    SLPX_HIP_CHECK(hipEventRecord(m_step_ev, main));
    SLPX_HIP_CHECK(hipStreamWaitEvent(m_tape_stream, m_step_ev, 0));
  }
  return Route{Route::Chained, m_words.p, s.wait_step, s.this_step};
}

void StepChain::recover(hipStream_t main) {
  drain_and_clear(main);
  m_ledger.failed();
}

}  // namespace slpx
