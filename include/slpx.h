/*
 * slpx — C-ABI of the MI355X-native interior-point Newton step.
 *
 * The reference (SleipnirGroup/Sleipnir) has no FFI boundary on this path: it is
 * a C++ header-template library.  The seam this library sits behind is made of
 * three reference C++ interfaces; every entry point below names
 * the reference interface it replaces.  Plain pointers and sizes only; opaque
 * handles; caller-owned host arrays; library-owned device memory; no exceptions
 * cross the ABI (functions return 0 on success, <0 on usage/HIP errors — see
 * slpx_last_error() — and >0 where documented).  One handle per host thread /
 * HIP stream, like the reference's thread_local pool (src/util/pool.cpp:5-8).
 *
 * All vectors are fp64, all indices int32, matrices are CSC (column-major
 * compressed, sorted row indices) with int32 indices — the layout of
 * Eigen::SparseMatrix<double> the reference passes around.  Batched buffers are
 * batch-major: buf[b * stride + i].
 *
 * There is NO CPU fallback: compute entry points fail with an error when no HIP
 * device is present.
 */
#ifndef SLPX_H_
#define SLPX_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slpx_problem slpx_problem;
typedef struct slpx_system slpx_system;

/* ---- library ------------------------------------------------------------ */
/* ABI history.  4: slpx_options.spy appended.  5: slpx_problem_solve() reads the options struct as it
 * was up to version 3 and therefore IGNORES `spy` — a caller that sets it must call
 * slpx_problem_solve_sized(p, &opt, sizeof opt, &report) (present since version 5: check
 * slpx_abi_version() >= 5 before binding it); the two benchmark-model constructors of versions <= 4
 * (slpx_problem_cart_pole / _flywheel) are gone: a model is the CALLER's program, built through the
 * slp:: surface or slpx_expr_* / slpx_problem_* (tests/support/models/ holds the benchmarks' as fixtures).
 * 6: SLPX_INFO_LDLT_DENSE appended to the info array (SLPX_INFO_COUNT grew by one). */
#define SLPX_ABI_VERSION 6
int slpx_abi_version(void);
const char* slpx_last_error(void);
int slpx_device_count(void);

/* Multi-GPU: a batch of independent problems is sharded over one process per GPU,
 * contiguous blocks, the first n_items % world ranks one item more — how multistart hands whole
 * solves to threads (optimization/multistart.hpp:52-62).  *lo, *hi = the half-open range of
 * `rank`.  No collective is needed inside a Newton step; a host joins the ranks only for
 * end-of-region reductions (RCCL).  Returns 0, -1 on a bad rank. */
int slpx_shard_range(int64_t n_items, int32_t rank, int32_t world, int64_t* lo, int64_t* hi);

/* ---- expression graph ------------------------------------------------------
 * Replaces: slp::Variable and the detail:: operator set
 * (include/sleipnir/autodiff/variable.hpp:52-295, expression.hpp:155-2080), i.e.
 * what python/cpp/autodiff/bind_variable.cpp binds for the reference's own FFI.
 * Op codes are slpx_op below.  Pruning/constant-folding/typing rules are the
 * reference's.  Ids index this thread's arena. */
typedef enum slpx_op {
  SLPX_OP_CONST = 0, SLPX_OP_VAR, SLPX_OP_ADD, SLPX_OP_SUB, SLPX_OP_NEG, SLPX_OP_MUL,
  SLPX_OP_DIV, SLPX_OP_POW, SLPX_OP_ABS, SLPX_OP_SIGN, SLPX_OP_SQRT, SLPX_OP_CBRT,
  SLPX_OP_EXP, SLPX_OP_LOG, SLPX_OP_LOG10, SLPX_OP_SIN, SLPX_OP_COS, SLPX_OP_TAN,
  SLPX_OP_ASIN, SLPX_OP_ACOS, SLPX_OP_ATAN, SLPX_OP_ATAN2, SLPX_OP_SINH, SLPX_OP_COSH,
  SLPX_OP_TANH, SLPX_OP_ERF, SLPX_OP_HYPOT, SLPX_OP_MAX, SLPX_OP_MIN, SLPX_OP_ISNONNEG,
  SLPX_OP_ISPOS
} slpx_op;

void slpx_graph_reset(void); /* frees this thread's arena; invalidates its problems */
int64_t slpx_graph_size(void);
int32_t slpx_expr_variable(double value);               /* Variable()          variable.hpp:289 */
int32_t slpx_expr_constant(double value);               /* Variable(double)    variable.hpp:64  */
int32_t slpx_expr_unary(int op, int32_t a);             /* sin(x), -x, ...                      */
int32_t slpx_expr_binary(int op, int32_t a, int32_t b); /* x*y, pow(x,y), ...                   */
int slpx_expr_type(int32_t id);                         /* Variable::type()    variable.hpp:153 */
double slpx_expr_value(int32_t id);                     /* Variable::value()   variable.hpp:143 */
void slpx_expr_set_value(int32_t id, double value);     /* Variable::set_value variable.hpp:125 */
/* Symbolic gradient: Gradient::get() / detail::gradient_tree (variable_matrix.hpp:1757-1805).
 * out[i] = expression id of d f / d wrt[i], or -1 when wrt[i] is unreachable from f. */
void slpx_expr_gradient_tree(int32_t f, const int32_t* wrt, int32_t n, int32_t* out);

/* ---- problem ------------------------------------------------------------------
 * Replaces: slp::Problem<double> (include/sleipnir/optimization/problem.hpp):
 * decision_variable :78, minimize :151, maximize :162, subject_to :196/:218,
 * cost_function_type :236, solve :281.  Constraint ids are `lhs - rhs`
 * expressions (variable.hpp:716-778); inequality convention c(x) >= 0. */
slpx_problem* slpx_problem_create(void);
void slpx_problem_destroy(slpx_problem* p);
int32_t slpx_problem_decision_variable(slpx_problem* p);
/* Registers an existing free variable (slpx_expr_variable) as a decision variable. */
void slpx_problem_adopt_variable(slpx_problem* p, int32_t var);
void slpx_problem_minimize(slpx_problem* p, int32_t cost);
void slpx_problem_maximize(slpx_problem* p, int32_t objective);
void slpx_problem_subject_to_eq(slpx_problem* p, int32_t c);
void slpx_problem_subject_to_ineq(slpx_problem* p, int32_t c);
int slpx_problem_cost_type(const slpx_problem* p);
int slpx_problem_eq_type(const slpx_problem* p);
int slpx_problem_ineq_type(const slpx_problem* p);
void slpx_problem_dims(const slpx_problem* p, int32_t* n, int32_t* m_e, int32_t* m_i);
void slpx_problem_get_x(const slpx_problem* p, double* x);
void slpx_problem_set_x(slpx_problem* p, const double* x);

/* slp::Options (solver/options.hpp:13-38) */
typedef struct slpx_options {
  double tolerance;    /* 1e-8 */
  int32_t max_iterations; /* 5000 */
  double timeout;      /* seconds; <= 0 means infinity */
  int32_t feasible_ipm;
  int32_t diagnostics;
  int32_t spy; /* Problem::solve(options, spy) (problem.hpp:281): write H.spy, A_e.spy, A_i.spy (util/spy.hpp) into the
                  working directory, one record per iteration; since ABI version 4.  Read ONLY through
                  slpx_problem_solve_sized: slpx_problem_solve takes the struct as it was up to ABI version 3
                  (a caller built against an older header passes a shorter one) */
} slpx_options;

/* Per-solve counters and wall-clock phases (names of interior_point.hpp:155-174) */
typedef struct slpx_report {
  int32_t iterations, factorizations, solves, value_sweeps;
  double delta, gamma, final_error;
  double t_setup, t_kkt_build, t_kkt_decomp, t_kkt_solve, t_line_search, t_ad_refresh, t_total;
  double t_compile; /* graph -> tape/KKT plan/symbolic LDLT + upload */
  int32_t restorations; /* feasibility-restoration phases entered (feasibility_restoration.hpp:347) */
  int32_t restoration_iterations; /* of `iterations`, those spent inside them */
  double t_restoration_setup; /* compiling the restoration system (first phase only); in t_total */
  double t_restoration;       /* the restoration iterations; in t_total */
} slpx_report;

/* Problem::add_callback / clear_callbacks (problem.hpp:690-712) with IterationInfo
 * (solver/iteration_info.hpp:13-41).  Called at the start of every iteration with the iterate
 * and the AD outputs the solver holds at that point: V = [f | c_e | c_i | g | A_e | A_i | H_f |
 * H_c], matrices as value arrays over the static CSC patterns (off[] = where each block
 * starts; patterns and counts from slpx_problem_system + slpx_system_pattern / _info).  The
 * Lagrangian Hessian of iteration_info.hpp:34 is H_f + H_c.  Return non-zero to stop the solve
 * with CALLBACK_REQUESTED_STOP (exit_status.hpp:17).  The pointers are valid during the call. */
typedef struct slpx_iteration_info {
  int32_t iteration;
  int32_t n, m_e, m_i; /* sizes of the arrays below */
  const double* x; /* n */
  const double* s; /* m_i */
  const double* y; /* m_e */
  const double* z; /* m_i */
  const double* V;
  int64_t off[8]; /* f, c_e, c_i, g, A_e, A_i, H_f, H_c */
  /* 1 inside feasibility restoration (feasibility_restoration.hpp:347-628): the arrays are then
   * the RESTORATION model's — n + 2 m_e + 2 m_i variables [x | p_e | n_e | p_i | n_i] and
   * m_i + 2 m_e + 2 m_i inequality rows, the user's x and s first — and n, m_e, m_i, off[] and V
   * describe that model (the reference calls the user's callbacks there too, :852) */
  int32_t in_restoration;
} slpx_iteration_info;
typedef int (*slpx_iteration_callback)(const slpx_iteration_info* info, void* user);
int slpx_problem_add_callback(slpx_problem* p, slpx_iteration_callback callback, void* user);
int slpx_problem_clear_callbacks(slpx_problem* p);
/* The system solve() runs on (compiled now if it was not yet); owned by the problem, do NOT
 * pass it to slpx_system_destroy.  NULL + slpx_last_error() without a HIP device. */
slpx_system* slpx_problem_system(slpx_problem* p);

/* Problem::solve.  Returns slp::ExitStatus (solver/exit_status.hpp:13-43):
 * 0 success, 1 callback stop, -1..-10 as in the reference; -100 on library error. */
int slpx_problem_solve(slpx_problem* p, const slpx_options* opt, slpx_report* report);
/* The same with the caller's sizeof(slpx_options): members beyond `options_bytes` keep their defaults
 * (spy, ABI version 4, is read only when the caller's struct holds it). */
int slpx_problem_solve_sized(slpx_problem* p, const slpx_options* opt, uint32_t options_bytes, slpx_report* report);
void slpx_problem_get_duals(const slpx_problem* p, double* s, double* y, double* z);
/* Batched whole solves: B instances of this problem from x0[B][n] (decision-variable order), each as
 * slpx_problem_solve would run from that start (its own scaling, barrier parameter, filter, regularization
 * memory, restoration, exit), with the options shared.  The solver follows the kinds of constraints present, as
 * slpx_problem_solve does (Newton without constraints, SQP with equality constraints only, interior point otherwise),
 * and each of the three runs all instances in lockstep on the device; options as slpx_problem_solve_sized, except that
 * `spy` and `diagnostics` are ignored.  The timeout applies to the whole batch: instances still running
 * when it expires report TIMEOUT.  The values of the problem's variables are not changed.  Outputs may be
 * NULL: status[B] (ExitStatus), x[B][n], s[B][m_i], y[B][m_e], z[B][m_i], cost[B] (unscaled f at the end),
 * iterations[B], restorations[B]; report = batch totals and wall-clock phases (delta, gamma, final_error: the
 * largest over the instances).  Returns 0, or -100 +
 * slpx_last_error() (no device, batch <= 0, x0 NULL, callbacks registered).  The batch system is compiled
 * on first use and kept with the problem, one per batch size.  An addition within ABI version 6: callers
 * detect it by the symbol's presence (dlsym). */
int slpx_problem_solve_batch(slpx_problem* p, int32_t batch, const double* x0, const slpx_options* opt,
                             uint32_t options_bytes, int32_t* status, double* x, double* s, double* y, double* z,
                             double* cost, int32_t* iterations, int32_t* restorations, slpx_report* report);
/* The last slpx_problem_solve_batch of this problem: out[4] = {batch, lockstep rounds (batched Newton-step
 * computations of the outer loop), instances handed to the batch-1 system for restoration,
 * driver: 0 none needed (constant problem / conflicting bounds), 1 interior point, 2 SQP, 3 Newton}.
 * Returns 0, -1 if no batch has been solved.  An addition within ABI version 6, detected like the one above. */
int slpx_problem_batch_stats(const slpx_problem* p, int64_t* out);
/* How the NEXT slpx_problem_solve_batch of this problem runs feasibility restoration
 * (interior_point.hpp:721-771, sqp.hpp:521-556 calling feasibility_restoration.hpp:347-628).  mode 0, the default:
 * an instance that asks for restoration is handed to the problem's batch-1 system, one instance after the other,
 * while the batch waits.  mode 1: every instance that asks in one round of the outer loop enters ONE restoration phase
 * together, on the batch system — the restoration iteration of each (its own barrier parameter, filter, line search,
 * regularization memory, exits) in lockstep with the others', one masked launch per phase of the iteration; the
 * multiplier estimate at exit (:606-617) and the KKT-error fallback of a line search (interior_point.hpp:691-716) still
 * use the batch-1 system, per instance.  Returns 0, or -100 + slpx_last_error() (null problem, a mode other than 0 / 1);
 * mode -1 changes nothing and returns the mode in force.  Needs no device.  An addition within ABI version 6, detected by the symbol's presence like slpx_problem_solve_batch. */
int slpx_problem_set_batch_restoration(slpx_problem* p, int mode);
/* The last slpx_problem_solve_batch (or slpx_problem_restoration_steps_batch) of this problem: out[4] = {instances
 * restored in lockstep, restoration phases, lockstep rounds of the restoration loop (batched Newton-step computations),
 * instances that used the batch-1 system for the KKT-error fallback}; all 0 after a solve in mode 0, whose hand-offs
 * slpx_problem_batch_stats counts (and which counts 0 hand-offs in mode 1).  Returns 0, -1 if no batch has been solved.
 * An addition within ABI version 6, detected like the one above. */
int slpx_problem_batch_restoration_stats(const slpx_problem* p, int64_t* out);
/* The batched twin of slpx_problem_restoration_steps (below): from B iterates x[B][n], s[B][m_i], y[B][m_e], z[B][m_i],
 * mu[B] — all in/out but mu — `steps` iterations of feasibility restoration per instance (feasibility_restoration.hpp:
 * 347-628) in lockstep on the batch system, left the way the reference leaves when its acceptance callback fires
 * (:729-752), y and z replaced by the least-squares multiplier estimate (lagrange_multiplier_estimate.hpp:56-133).
 * Scaling as in slpx_problem_restoration_steps (at the variables' current values, the same for every instance);
 * options as slpx_problem_solve_sized (tolerance, max_iterations, timeout are read).  status[B]: the ExitStatus of
 * that function per instance (0: restored).  Returns 0, or -100 + slpx_last_error() (no device, batch <= 0, a NULL
 * array, callbacks registered).  An addition within ABI version 6, detected like the ones above. */
int slpx_problem_restoration_steps_batch(slpx_problem* p, const slpx_options* opt, uint32_t options_bytes, int32_t batch,
                                         double* x, double* s, double* y, double* z, const double* mu, int32_t steps,
                                         int32_t* status);
/* feasibility_restoration (solver/util/feasibility_restoration.hpp:347-628) on its own: from the
 * iterate (x[n], s[m_i], y[m_e], z[m_i], mu) — all in/out but mu — build the restoration model,
 * run `steps` iterations of its interior-point loop, leave it the way the reference does when its
 * acceptance callback fires (:729-752), and replace y, z by the least-squares multiplier estimate
 * (lagrange_multiplier_estimate.hpp:56-133).  Scaling as in slpx_problem_solve (at the variables'
 * current values).  Returns the ExitStatus of that function (0: restored), -100 on library error. */
int slpx_problem_restoration_steps(slpx_problem* p, const slpx_options* opt, double* x, double* s, double* y,
                                   double* z, double mu, int32_t steps);

/* Build-time helper (no reference counterpart; needs NO device): compiles the model's structure
 * on the host, generates its tape kernels and cross-compiles them for gfx950 with hipRTC into
 * `dir` (NULL: <directory of libslpx.so>/jit_cache, where slpx_system_create looks before it
 * compiles anything).  Returns the number of generated bodies, < 0 on failure. */
int slpx_problem_prebuild_kernels(slpx_problem* p, const char* dir);

/* ---- parameters as runtime inputs -------------------------------------------------
 * A free variable (slpx_expr_variable) that is no decision variable of the problem and that the cost or a constraint
 * reaches is a PARAMETER of the model: an initial state, a reference, a bound, a weight.  Its value lives in a slot of
 * the compiled tapes' constant pool, so it can change without compiling anything again, and a batch can carry a pool
 * per instance.  (slpx_expr_set_value on a parameter keeps doing what it did: the next solve notices and compiles a
 * new system.)  The entry points of this section (and slpx_system_set_parameters / slpx_system_parameter_pool_bytes
 * below) are additions within ABI version 6, detected by the symbol's presence like slpx_problem_solve_batch.
 *
 * slpx_problem_parameters: the number n_p of parameters the model reaches; their expression ids, ascending, into
 * ids[0 .. min(n_p, capacity)) when ids is not NULL.  That order is the order of every parameter vector below.  Needs
 * NO device: where the problem has no compiled system the model's structure is compiled on the host for the answer
 * (the path of slpx_problem_prebuild_kernels).  < 0: -100 + slpx_last_error(). */
int32_t slpx_problem_parameters(slpx_problem* p, int32_t* ids, int32_t capacity);
/* Without a device: 1 if parameter j sits in constant slot j of both tape programs (full sweep and values only), which
 * the tape compiler promises (it hands out the parameters' slots first, in the order above), 0 if not; < 0 on error. */
int slpx_problem_parameter_slots_in_order(slpx_problem* p);
/* values[n_p] become the parameters' values: in the expression graph, and IN PLACE in the problem's compiled system
 * and every batch system it holds (compiled now if there was none).  The next slpx_problem_solve / _solve_batch /
 * slpx_problem_system does not compile again, and a handle from slpx_problem_system taken before stays valid.
 * Returns 0, or -100 + slpx_last_error() (null problem or values, no device). */
int slpx_problem_set_parameters(slpx_problem* p, const double* values);
/* How many times this problem has built the system slpx_problem_solve runs on. */
int64_t slpx_problem_compile_count(const slpx_problem* p);
/* slpx_problem_solve_batch where instance b is the problem with the parameter row params[b][n_p], solved from x0[b];
 * params NULL: exactly slpx_problem_solve_batch.  The bounds test (GLOBALLY_INFEASIBLE) is made per instance.  The
 * variables' and the parameters' values are left as they are, and on return every system of the problem reads the
 * parameters' current values again.  -100 + slpx_last_error() additionally for params given to a model without
 * parameters. */
int slpx_problem_solve_batch_parameters(slpx_problem* p, int32_t batch, const double* x0, const double* params,
                                        const slpx_options* opt, uint32_t options_bytes, int32_t* status, double* x,
                                        double* s, double* y, double* z, double* cost, int32_t* iterations,
                                        int32_t* restorations, slpx_report* report);

/* ---- warm starts --------------------------------------------------------------------
 * A solve may begin at a caller-given primal-dual iterate instead of s = 1, y = 0, z = 1, mu = 0.1 d_f: typically
 * the iterate the previous solve of a neighbouring problem ended at (an MPC loop around slpx_problem_set_parameters).
 * The entry points of this section are additions within ABI version 6, detected by the symbol's presence like
 * slpx_problem_solve_batch.
 *
 * UNITS.  A solve runs on a scaled problem (cost scale d_f, row scales d_ce, d_ci, computed anew at every solve's x0),
 * so scaled values do not carry over from one solve to the next.  Everything in this section is in the USER'S units:
 *     s_u = s / d_ci     y_u = y d_ce / d_f     z_u = z d_ci / d_f     mu_u = mu / d_f
 * — y_u, z_u are the multipliers of f - y^T c_e - z^T c_i as the model was written.  slpx_problem_get_duals and the
 * s, y, z outputs of slpx_problem_solve_batch[_parameters] return the SCALED iterate of the solve, as they always have:
 * callers that compare iterates with the reference's read them, and changing their units would change those callers.
 *
 * SAFEGUARD, per instance, in the scaled space of the new solve (mu_min = d_f tolerance / 10, c_i the constraint value
 * at x0): a NaN or Inf in x, in a given array or in mu ends the instance with NONFINITE_INITIAL_GUESS (-7) before any
 * iteration.  mu: the given one where > 0, floored at mu_min; else the mean of s_j z_j over the rows where both are
 * given and positive, within [mu_min, 0.1 d_f]; else 0.1 d_f.  s_j absent or <= 0: max(c_i_j, mu).  z_j absent or
 * <= 0: mu / s_j; then every z_j is clamped into [mu / (1e10 s_j), 1e10 mu / s_j], as after every step of the
 * iteration.  y absent: 0.  The number of entries replaced or moved by the clamp is reported (`repaired`); an iterate
 * this library returned for the same scales passes with 0 and every bit unchanged.  Filter, regularization memory
 * and counters start as in a cold solve.  Without inequality constraints only x and y are read (SQP), without any
 * constraints only x (Newton); the other members are accepted and ignored.  A warm start that gives nothing beside
 * x — no array, and no mu above 0 — is the cold start. */
typedef struct slpx_warm_start {
  const double *s, *y, *z; /* [m_i], [m_e], [m_i]; NULL: absent */
  double mu;               /* <= 0: choose */
} slpx_warm_start;
/* slpx_problem_solve_sized from the variables' values (slpx_problem_set_x) and *ws; ws NULL: exactly
 * slpx_problem_solve_sized. */
int slpx_problem_solve_warm(slpx_problem* p, const slpx_options* opt, uint32_t options_bytes, const slpx_warm_start* ws,
                            slpx_report* report);
/* The iterate the last slpx_problem_solve* ended at (any of the outputs may be NULL): x[n], s[m_i], y[m_e], z[m_i], *mu
 * (0 where the solver has no barrier).  Returns 0; -100 + slpx_last_error() for a null problem or before any solve
 * that ran a solver.  Needs no device. */
int slpx_problem_get_iterate(const slpx_problem* p, double* x, double* s, double* y, double* z, double* mu);
/* How many entries of its warm start the last slpx_problem_solve_warm repaired; < 0: null problem. */
int32_t slpx_problem_warm_start_repaired(const slpx_problem* p);
/* slpx_problem_solve_batch_parameters (params may be NULL) with instance b started from s0[b][m_i], y0[b][m_e],
 * z0[b][m_i], mu0[b] — each of the four may be NULL — and with the outputs s, y, z, mu[B] in the user's units: what the
 * next call takes as s0, y0, z0, mu0.  repaired[B] (may be NULL): the safeguard's count per instance.  With s0 = y0 =
 * z0 = mu0 = NULL every instance runs exactly as in slpx_problem_solve_batch_parameters; only the units of the dual
 * outputs differ.  The safeguard runs on the device, one workgroup per instance.  Returns 0, or -100 +
 * slpx_last_error() as slpx_problem_solve_batch_parameters. */
int slpx_problem_solve_batch_warm(slpx_problem* p, int32_t batch, const double* x0, const double* params, const double* s0,
                                  const double* y0, const double* z0, const double* mu0, const slpx_options* opt,
                                  uint32_t options_bytes, int32_t* status, double* x, double* s, double* y, double* z,
                                  double* mu, double* cost, int32_t* iterations, int32_t* restorations, int32_t* repaired,
                                  slpx_report* report);

/* ---- solution sensitivities ------------------------------------------------------------
 * How the end iterate of the last slpx_problem_solve* moves when a parameter moves (no reference counterpart): the
 * tangent predictor of an MPC loop — iterate + d(iterate)/dp dp as the warm start of the next solve — and the gradient
 * of anything downstream of x* with respect to the parameters.  The entry points of this section are additions within
 * ABI version 6, detected by the symbol's presence like slpx_problem_solve_batch.
 *
 * With L = f - y^T c_e - z^T c_i, Sigma = S^-1 Z and, for parameter q at the iterate (x, s, y, z) HELD FIXED,
 *     r_x = d(grad_x L)/dp_q      r_e = dc_e/dp_q      r_i = dc_i/dp_q
 * the KKT conditions differentiated, ds and dz eliminated as the Newton step eliminates p_s and p_z
 * (interior_point.hpp:426-481), give
 *     [H + A_i^T Sigma A_i  A_e^T] [ dx ]   [-r_x - A_i^T Sigma r_i]
 *     [       A_e            0   ] [-dy ] = [        -r_e          ]       ds = A_i dx + r_i      dz = -Sigma ds
 * — the matrix of the Newton step, assembled at the iterate and factored by the same inertia-correcting loop
 * (slpx_ldlt_compute, from a cleared memory), every right-hand side solved on that factorization and refined twice
 * (slpx_ldlt_refine).  The barrier parameter is held fixed: for an interior-point solve these are the sensitivities of
 * the barrier problem's solution, which differ from those of the model's by O(mu).  Without inequality constraints,
 * and without any constraints, the same equations with the blocks absent.
 *
 * UNITS: everything is in the USER'S units, those of slpx_problem_get_iterate (warm starts, above).  The model's own
 * system is swept, assembled and factored at unit scales for the call; the scaling of the last solve is installed again
 * before it returns.  ORDER: parameters as slpx_problem_parameters; outputs are parameter-major, row q = d(.)/dp_q.
 *
 * COST.  The first call compiles the model once more with the parameters as variables ("the extended structure":
 * t_compile; kept with the problem, dropped when the model is compiled again — slpx_problem_compile_count does not
 * count it).  The factorization is kept until the next slpx_problem_solve* / restoration call of the problem, the next
 * slpx_problem_system, or a model change: calls in between report factorizations = 0.  A caller that drives the
 * handle of slpx_problem_system itself between two calls asks for that handle again first.  The Jacobian takes n_p
 * solves; the two products take ONE each, whatever n_p.  A following solve is not affected in any bit: the
 * regularization memory, the scaling and the parameters of the problem's system are as they were.
 *
 * ERRORS: -100 + slpx_last_error() for a null problem, before any solve that ran a solver, for a model that reaches
 * no parameter, when the parameters' values are no longer those of the solve the iterate came from
 * (slpx_problem_set_parameters / slpx_expr_set_value with no new solve), without a HIP device, and when the system
 * cannot be factored at all.  The status of that solve is NOT judged (solve_status reports it), and a regularization
 * the factorization needed is no error: delta, gamma and the inertia are reported. */
typedef struct slpx_sensitivity_info {
  int32_t n_p, solves, factorizations, refine_steps;   /* of this call (solves: refinement's included) */
  int32_t n_pos, n_neg, n_zero;                        /* inertia of what was factored */
  double delta, gamma;                                 /* regularization it needed */
  double berr_max;                                     /* largest componentwise backward error over the solves
                                                          (slpx_ldlt_error_bounds: of the system as factored, delta and
                                                          gamma in it; it reaches O(1) where a whole row of a right-hand
                                                          side and its solution is at rounding level) */
  int32_t solve_status;                                /* ExitStatus of the solve the iterate came from */
  double t_compile, t_factor, t_total;                 /* seconds; t_compile > 0 on the first call only; t_total includes
                                                          both */
} slpx_sensitivity_info;
/* The Jacobian: dx[n_p][n], ds[n_p][m_i], dy[n_p][m_e], dz[n_p][m_i].  Any output, and info, may be NULL. */
int slpx_problem_sensitivity(slpx_problem* p, double* dx, double* ds, double* dy, double* dz, slpx_sensitivity_info* info);
/* The Jacobian-vector product along dp[n_p]: dx[n], ds[m_i], dy[m_e], dz[m_i] — iterate + these is a valid
 * slpx_warm_start of the model with parameters + dp (mu: that of the iterate). */
int slpx_problem_sensitivity_jvp(slpx_problem* p, const double* dp, double* dx, double* ds, double* dy, double* dz,
                                 slpx_sensitivity_info* info);
/* The vector-Jacobian product for a cotangent vx[n] on x: grad_p[q] = sum_i vx[i] dx_i/dp_q, from ONE solve K w = [vx; 0]
 * and grad_p[q] = w^T R[:, q], R the right-hand sides above (K is symmetric, also when regularized). */
int slpx_problem_sensitivity_vjp(slpx_problem* p, const double* vx, double* grad_p, slpx_sensitivity_info* info);
/* THE FULL VJP: cotangents on the whole end iterate and on the optimal cost, still ONE solve on the kept factorization.
 * `cost` is the value the solve reports as the cost: f as slpx_problem_minimize / slpx_problem_maximize stored it (a
 * maximized objective is stored negated, and so is reported and differentiated), in the user's units.  Forward, per
 * parameter q, beside the equations above:    dcost = g . dx + f_p[q]       g = grad_x f, f_p[q] = df/dp_q
 * Reverse, for cotangents vx[n], vs[m_i], vy[m_e], vz[m_i], vcost[1]:
 *     t = vs - Sigma o vz        u = vx + A_i^T t + vcost g        K w = [u; -vy]
 *     grad_p[q] = w^T R[:, q] + t . r_i[:, q] + vcost f_p[q]
 * the adjoint of ds = A_i dx + r_i, dz = -Sigma ds folded into the right-hand side of the one solve, refined like every
 * other; K is symmetric also when regularized and the forward products use the same K, so <v, J dp> = <J^T v, dp> holds
 * to the accuracy of the solves.  A member that is NULL is absent and its terms are skipped (not added as zeros): with
 * vx alone this is slpx_problem_sensitivity_vjp bit for bit.  All members NULL is an error ("no cotangent"); a cotangent
 * on rows the model does not have (vs with m_i = 0) is ignored.  vcost = 1 alone gives the gradient of the optimal cost
 * in one solve instead of the n_p of the Jacobian route.  For an interior-point model that is the derivative of f at the
 * barrier problem's solution, O(mu) from the model's — NOT the derivative of the barrier function f - mu sum log s.
 * cotangent_bytes: sizeof(slpx_cotangent) as the caller's header has it (members beyond it are absent), like
 * options_bytes.  Batched: vx[B][n], vs[B][m_i], vy[B][m_e], vz[B][m_i], vcost[B]; status[b] = 1 for an instance with a
 * value that is not finite in ANY given cotangent row (its gradient row is NaN, the others do not notice).  Everything
 * the two vjp entry points promise — factorizations = 0 on a kept factorization, nothing of the problem moved, a
 * following solve keeps every bit — holds for these. */
typedef struct slpx_cotangent {
  const double *vx, *vs, *vy, *vz, *vcost;
} slpx_cotangent;
int slpx_problem_sensitivity_vjp_full(slpx_problem* p, const slpx_cotangent* v, uint32_t cotangent_bytes, double* grad_p,
                                      slpx_sensitivity_info* info);
/* M[n_p][n + m_e + m_i]: r_x, r_e, r_i per parameter, at the iterate.  Neither factors nor solves. */
int slpx_problem_sensitivity_rhs(slpx_problem* p, double* M);

/* ---- batched sensitivities ----------------------------------------------------------------
 * The same derivatives for B iterates at once, instance b with respect to ITS parameter row — additions within ABI
 * version 6, detected by the symbol's presence.  slpx_problem_solve_batch* leaves no state in the problem, so these are
 * functions of the rows they are given, everything in the user's units:
 *     x[B][n], s[B][m_i], y[B][m_e], z[B][m_i], mu[B]   the end iterates, exactly what slpx_problem_solve_batch_warm
 *                                                       returns (and slpx_problem_get_iterate for one problem)
 *     params[B][n_p]                                    the parameter rows, the order of slpx_problem_parameters
 * s, y, z may be NULL where the model has no such rows.  Equations, units and policy are those of the section above:
 * unit scales, every instance factored from a cleared regularization memory, every right-hand side solved and refined
 * twice, the componentwise backward error reported.
 *
 * status[B] reports each instance instead of an error for the call:
 *     0  computed
 *     1  skipped: a NaN or an Inf in its iterate, its parameter row, dp or vx, or an s_j <= 0 with m_i > 0
 *     2  the KKT system at its iterate could not be factored
 * Every output row of an instance whose status is not 0 is NaN; the other instances do not notice it (it is left out of
 * the factorization, the refinement and the error bounds), and their bits depend neither on B nor on their position
 * nor on their neighbours.  info[B] is per instance: inertia (of a computed instance: what the policy accepts,
 * (n, m_e, 0), stated as such and not read back from the counters, which are those of the call's LAST factorization
 * launch), delta, gamma, solves, refine_steps, berr_max;
 * factorizations is the count of factorization launches of the call (0 for a skipped instance), solve_status is 0 (the
 * call is not told it), the times are the call's, repeated in every row.
 *
 * STATE.  A call runs on the batch system of size B (the one slpx_problem_solve_batch uses) and on an extended system
 * compiled for that B on the first call (t_compile; kept with the problem).  It changes neither the variables nor the
 * parameters, neither the scaling nor the regularization memory of the problem's own system, nor a kept single-problem
 * sensitivity factorization; the batch system has its shared parameter pool and its regularization memory back on
 * return, so a following slpx_problem_solve_batch* keeps every bit.  The factorization is kept: a call with the same B
 * and the same bits in every iterate and parameter row reports factorizations = 0, until the next
 * slpx_problem_solve_batch* or slpx_problem_restoration_steps_batch of that B or a model change.  The Jacobian takes n_p
 * rounds of solves, round q carrying column q of all B instances; the two products take ONE round.
 *
 * ERRORS: -100 + slpx_last_error() for a null problem, B <= 0 or B > 65535 (one grid slice per instance), a NULL
 * required input, a model that reaches no parameter, and without a HIP device.  Any output, status and info may be
 * NULL. */
/* The Jacobians: dx[B][n_p][n], ds[B][n_p][m_i], dy[B][n_p][m_e], dz[B][n_p][m_i]. */
int slpx_problem_sensitivity_batch(slpx_problem* p, int32_t B, const double* x, const double* s, const double* y, const double* z,
                                   const double* mu, const double* params, double* dx, double* ds, double* dy, double* dz,
                                   int32_t* status, slpx_sensitivity_info* info);
/* Along dp[B][n_p]: dx[B][n], ds[B][m_i], dy[B][m_e], dz[B][m_i] — iterate + these is the warm start of the next batch
 * with params + dp. */
int slpx_problem_sensitivity_batch_jvp(slpx_problem* p, int32_t B, const double* x, const double* s, const double* y,
                                       const double* z, const double* mu, const double* params, const double* dp, double* dx,
                                       double* ds, double* dy, double* dz, int32_t* status, slpx_sensitivity_info* info);
/* For cotangents vx[B][n] on x: grad_p[B][n_p]. */
int slpx_problem_sensitivity_batch_vjp(slpx_problem* p, int32_t B, const double* x, const double* s, const double* y,
                                       const double* z, const double* mu, const double* params, const double* vx, double* grad_p,
                                       int32_t* status, slpx_sensitivity_info* info);
/* The full vjp (above) per instance: cotangent rows per instance, grad_p[B][n_p]. */
int slpx_problem_sensitivity_batch_vjp_full(slpx_problem* p, int32_t B, const double* x, const double* s, const double* y,
                                            const double* z, const double* mu, const double* params, const slpx_cotangent* v,
                                            uint32_t cotangent_bytes, double* grad_p, int32_t* status, slpx_sensitivity_info* info);
/* M[B][n_p][n + m_e + m_i]: r_x, r_e, r_i per instance and parameter.  Neither factors nor solves. */
int slpx_problem_sensitivity_batch_rhs(slpx_problem* p, int32_t B, const double* x, const double* s, const double* y,
                                       const double* z, const double* mu, const double* params, double* M, int32_t* status);

/* ---- compiled Newton system ------------------------------------------------------
 * One problem structure compiled for one GPU, `batch` independent value sets.
 * Replaces, per Newton step:
 *   AD evaluator seam  Gradient/Jacobian/Hessian::value()
 *                      (autodiff/gradient.hpp:53, jacobian.hpp:134, hessian.hpp:132)
 *                      and the Problem lambdas problem.hpp:618-660
 *   KKT build          solver/interior_point.hpp:426-448
 *   linear solver seam RegularizedLDLT::compute/solve/info/hessian_regularization/
 *                      constraint_jacobian_regularization (util/regularized_ldlt.hpp:56-128)
 *   back-substitution  solver/interior_point.hpp:470-481 */
slpx_system* slpx_system_create(slpx_problem* p, int32_t batch, int32_t device,
                                const int32_t* perm, int32_t perm_len);
void slpx_system_destroy(slpx_system* s);
int slpx_system_set_stream(slpx_system* s, void* hip_stream);
int slpx_system_sync(slpx_system* s);

enum {
  SLPX_INFO_N = 0, SLPX_INFO_ME, SLPX_INFO_MI, SLPX_INFO_NV, SLPX_INFO_NNZ_G, SLPX_INFO_NNZ_AE,
  SLPX_INFO_NNZ_AI, SLPX_INFO_NNZ_HF, SLPX_INFO_NNZ_HC, SLPX_INFO_NNZ_LHS, SLPX_INFO_NNZ_L,
  SLPX_INFO_LDLT_ROUNDS, SLPX_INFO_LDLT_TASKS, SLPX_INFO_ETREE_HEIGHT, SLPX_INFO_LDLT_PAIRS,
  SLPX_INFO_TAPE_TASKS, SLPX_INFO_TAPE_NODES, SLPX_INFO_TAPE_SLOTS, SLPX_INFO_TAPE_EDGES,
  SLPX_INFO_TAPE_LEVELS, SLPX_INFO_TAPE_SLOT_LEVELS, SLPX_INFO_ASSEMBLE_BYTES,
  SLPX_INFO_RHS_BYTES, SLPX_INFO_FACTOR_BYTES, SLPX_INFO_SOLVE_BYTES, SLPX_INFO_SWEEP_BYTES,
  SLPX_INFO_STRUCT_SINGULAR, SLPX_INFO_OFF_G, SLPX_INFO_OFF_AE, SLPX_INFO_OFF_AI,
  SLPX_INFO_OFF_HF, SLPX_INFO_OFF_HC, SLPX_INFO_GRAPH_NODES, SLPX_INFO_NONLINEAR_ROWS,
  SLPX_INFO_TAPE_GLOBAL_TASKS, SLPX_INFO_TAPE_SHARED_TASKS, SLPX_INFO_TAPE_PROGRAM_BYTES,
  /* supernodal LDLT: levels on the critical path (sum over rounds of the deepest task),
   * supernodes (singletons included), widest supernode in columns */
  SLPX_INFO_LDLT_LEVELS, SLPX_INFO_LDLT_SUPERNODES, SLPX_INFO_LDLT_WIDEST,
  /* since ABI version 5: the multifrontal plan — 1 if the single-problem step runs on fronts, their
   * number, and how many of them send their update block through the matrix cores */
  SLPX_INFO_LDLT_MULTIFRONTAL, SLPX_INFO_LDLT_FRONTS, SLPX_INFO_LDLT_MFMA_FRONTS,
  /* since ABI version 6: non-zero if the system is factored as a dense matrix (the reference's dense branch,
   * util/dense_regularized_ldlt.hpp).  2: chosen by the reference's own rule (interior_point.hpp:340-352: the lower
   * triangle fills a quarter of the system or more) and factored with Eigen::LDLT's diagonal pivoting; 1: the plain
   * dense kernel, where a column of L does not fit a task of the sparse plan (or SLPX_DENSE=1) */
  SLPX_INFO_LDLT_DENSE,
  SLPX_INFO_COUNT
};
int slpx_system_info(const slpx_system* s, int64_t* out /* SLPX_INFO_COUNT */);

/* Static sparsity patterns (CSC).  which: 0 g (1 x n), 1 A_e, 2 A_i, 3 H_f (lower),
 * 4 H_c (lower), 5 KKT lhs (lower, full diagonal).  Pass NULL to query only nnz. */
int32_t slpx_system_pattern(const slpx_system* s, int which, int32_t* colptr, int32_t* rowidx);
int slpx_system_perm(const slpx_system* s, int32_t* perm); /* fill-reducing permutation, perm[new]=old */

/* scales = [d_f, d_ce(m_e), d_ci(m_i)] (util/problem_scaling.hpp:100-107) */
int slpx_system_set_scaling(slpx_system* s, const double* scales);
/* The parameters of the model (slpx_problem_parameters: count and order) at the compiled-system seam, for callers of
 * slpx_tape_sweep / slpx_newton_step.  per_instance 0: values[n_p] for every instance (one shared constant pool);
 * 1: values[batch][n_p], instance b reads row b (a pool per instance, in force until the next call with 0).  The
 * expression graph is not touched: a system borrowed from a problem is better served by slpx_problem_set_parameters.
 * Returns 0, or -100 + slpx_last_error() (null system or values; per_instance with a model without parameters).  An
 * addition within ABI version 6, detected by the symbol's presence like slpx_problem_solve_batch. */
int slpx_system_set_parameters(slpx_system* s, const double* values, int per_instance);
/* Device memory the per-instance constant pools of this system take: batch x (constants of the full program +
 * constants of the values-only program) x 8 bytes once per-instance values were installed, 0 before.  < 0: -100 +
 * slpx_last_error().  An addition within ABI version 6, detected like the one above. */
int64_t slpx_system_parameter_pool_bytes(slpx_system* s);
/* x[batch][n], s[batch][m_i], y[batch][m_e], z[batch][m_i], mu[batch] (any may be NULL = keep) */
int slpx_system_set_state(slpx_system* s, const double* x, const double* sl, const double* y,
                          const double* z, const double* mu);

int slpx_tape_sweep(slpx_system* s, int full); /* full=1: values + g, A_e, A_i, H; 0: f, c_e, c_i */
int slpx_kkt_assemble(slpx_system* s);
int slpx_kkt_rhs(slpx_system* s);
/* One numeric factorization with explicit per-problem (delta, gamma).
 * stats[batch][5] = {n_pos, n_neg, n_zero, n_bad, min|D|} */
int slpx_ldlt_factor(slpx_system* s, const double* delta, const double* gamma, double* stats);
/* The whole inertia-correcting loop of sparse_regularized_ldlt.hpp:64-152.
 * info[batch] (0 Success, 1 NumericalIssue), reg[batch][2] = {delta, gamma} used. */
int slpx_ldlt_compute(slpx_system* s, int32_t* info, double* reg, int32_t* factorizations);
int slpx_ldlt_reset(slpx_system* s, double gamma_min);
int slpx_ldlt_solve(slpx_system* s); /* rhs -> p, reusable after one compute */
int slpx_step_backsub(slpx_system* s);
/* r = rhs - (lhs + diag(delta, -gamma)) p of the factorization in memory, accumulated in
 * double-double; r[batch][dim] and norm_inf[batch] may be NULL.
 * lhs, rhs, p: what slpx_system_get(1 / 2 / 3) hands out (a matrix or right-hand side the caller set is used as
 * given; a Newton step that never stored its system has it assembled now, at the RESIDENT state); delta on the
 * first n rows, -gamma on the other m_e, per problem those of the last factorization of that problem — the pair
 * slpx_ldlt_compute / slpx_newton_step settled on, or the one given to slpx_ldlt_factor.  Every row is summed in one
 * fixed order, so r and norm_inf of a problem have the same bits at any batch size.  norm_inf = max |r_i|, non-finite
 * if any r_i is.  Returns 0, or -100 + slpx_last_error() (no factorization and solution in memory yet).  An
 * addition within ABI version 6, detected by the symbol's presence like slpx_problem_solve_batch. */
int slpx_ldlt_residual(slpx_system* s, double* r, double* norm_inf);
/* up to max_steps steps of iterative refinement of p on the factors in memory;
 * norms[batch][max_steps+1] (unused tail = NaN), accepted[batch]; either may be NULL.
 * A step solves (lhs + diag(delta, -gamma)) d = r with the factors in memory and takes p + d only if its residual
 * norm is finite and smaller than the one before — otherwise that problem keeps its p and stops; a problem whose
 * first norm is 0 takes no step (p keeps its bits).  norms = the norm before, then the one after every step taken or
 * tried; accepted = steps taken.  The right-hand side in memory is the same on return; p_s / p_z are not updated:
 * slpx_step_backsub does that.  Between slpx_newton_step and slpx_step_backsub, and BEFORE the iterate moves: a
 * system the step never stored is evaluated at the resident state.  An addition within ABI version 6. */
int slpx_ldlt_refine(slpx_system* s, int32_t max_steps, double* norms, int32_t* accepted);
/* The two above for the problems with mask[b] != 0 only (mask NULL: all): nothing of the others is touched — their
 * p, and their rows of r, norm_inf, norms and accepted keep what they held.  Additions within ABI version 6. */
int slpx_ldlt_residual_masked(slpx_system* s, const uint8_t* mask, double* r, double* norm_inf);
int slpx_ldlt_refine_masked(slpx_system* s, int32_t max_steps, const uint8_t* mask, double* norms, int32_t* accepted);
/* Error bounds of p on the factors in memory, per problem with mask[b] != 0 (mask NULL: all) — the outputs of
 * LAPACK's expert drivers (xSYRFS).  berr[batch]: the componentwise backward error max_i |r_i| / (|b| + |K'| |p|)_i
 * (0 where the denominator is 0), K' = lhs + diag(delta, -gamma) and r as in slpx_ldlt_residual.  ferr[batch]: an
 * estimate of || |K'^-1| (|r| + rho) ||_inf / ||p||_inf, rho_i a proven bound on the rounding error of the
 * double-double r_i — it bounds the relative forward error max |p - p*| / max |p| as far as Hager's / Higham's 1-norm
 * estimator (LAPACK's dlacn2) goes, which is a lower estimate, nearly always within a small factor.  ||p||_inf == 0:
 * ferr = 0 if |r| + rho is all zero, +inf otherwise.  solves[batch]: the solves each problem's estimate took, at most
 * 11; all problems share them.  Any output may be NULL; ferr == NULL: no estimator and no solve run.  A non-finite
 * entry in a problem's system, right-hand side or solution makes that problem's numbers NaN and leaves the others'
 * bits alone.  p and the right-hand side in memory have the bits on return that they had on entry, for every problem;
 * rows of the problems left out keep what they held.  When and errors as slpx_ldlt_refine.  Every number of a
 * problem has the same bits at any batch size, in any slot and under any mask.  An addition within ABI version 6,
 * detected by the symbol's presence. */
int slpx_ldlt_error_bounds(slpx_system* s, const uint8_t* mask, double* berr, double* ferr, int32_t* solves);
/* norm1[batch] = ||K'||_1 and inv_norm1[batch] ~ ||K'^-1||_1 (the same estimator: never above the true norm but for
 * the rounding of the solves); their product estimates the 1-norm condition number of what was factored.
 * solves[batch] as above.  Same contract as slpx_ldlt_error_bounds.  An addition within ABI version 6. */
int slpx_ldlt_condest(slpx_system* s, const uint8_t* mask, double* norm1, double* inv_norm1, int32_t* solves);
/* AD refresh (optional) + assemble + rhs + compute + solve + backsub */
int slpx_newton_step(slpx_system* s, int refresh_ad, int32_t* info);
/* `count` such steps one after the other on the resident state, each waited for like a single
 * one (the host reads the inertia before launching the next) — the loop a C++ harness writes
 * around slpx_newton_step, minus a foreign-function call per step.  forget_regularization != 0
 * clears the delta/gamma memory before every step (slpx_ldlt_reset keeps gamma_min), so each
 * step starts like the first iteration of a solve.  info[batch] = OR over the steps. */
int slpx_newton_steps(slpx_system* s, int32_t count, int refresh_ad, int forget_regularization, int32_t* info);
/* reg[batch][2] = {hessian_regularization(), constraint_jacobian_regularization()}
 * (util/regularized_ldlt.hpp:111,122) the last compute / Newton step settled on, per problem. */
int slpx_system_regularization(slpx_system* s, double* reg);

/* Device -> host copies.  which: 0 V, 1 lhs, 2 rhs, 3 p, 4 p_s, 5 p_z, 6 D (pivot order), 7 L values,
 * 8 x, 9 s, 10 y, 11 z (the resident iterate); for tests of the factorization kernels, per problem: 12 z = D^-1 L^-1 P rhs
 * of the right-hand side that rode in the last factorization (pivot order), 13 the update blocks its rounds handed
 * each other */
int64_t slpx_system_get(slpx_system* s, int which, double* out);
int slpx_system_set_rhs(slpx_system* s, const double* rhs);
/* RegularizedLDLT::compute(lhs) with a caller-assembled matrix (regularized_ldlt.hpp:72):
 * values in the order of pattern 5 (lower CSC, forced diagonal), [batch][nnz]. */
int slpx_system_set_lhs(slpx_system* s, const double* lhs);

/* ---- The linear-solver seam on its own (SURVEY.md §8b seam 3) ----
 * RegularizedLDLT<double>(use_sparse = true, n, m_e, gamma_min) (util/regularized_ldlt.hpp:45-51):
 * a system with no expression graph, made from the lower-triangular CSC pattern of the matrix
 * compute() will be given — the `lhs` of interior_point.hpp:434-440, same pattern on every call
 * (regularized_ldlt.hpp:66-68); diagonal entries may be absent, they are added like
 * sparse_regularized_ldlt.hpp:67 does.  The first n rows/columns are regularized with +delta, the
 * other m_e with -gamma (:217-224).  The handle serves
 *   slpx_ldlt_reset(gamma_min)                       the constructor's gamma_min      (:45-51)
 *   slpx_ldlt_set_matrix + slpx_ldlt_compute         compute(lhs), info()             (:72, :56)
 *   slpx_system_set_rhs + slpx_ldlt_solve + slpx_system_get(3)     solve(rhs)         (:87)
 * (reg[] of slpx_ldlt_compute = hessian_regularization(), constraint_jacobian_regularization(),
 * :111,:122).  NULL + slpx_last_error() on failure, e.g. without a HIP device. */
slpx_system* slpx_ldlt_create(int32_t n, int32_t m_e, const int32_t* colptr, const int32_t* rowidx,
                              int32_t batch, int32_t device);
/* values[batch][nnz] in the order of the pattern given to slpx_ldlt_create */
int slpx_ldlt_set_matrix(slpx_system* s, const double* values);

/* ---- The interior-point iteration AROUND the Newton step, on the resident iterate ----
 * (one problem per system).  What interior_point() does between two Newton steps with
 * O(n) host loops over Eigen vectors (interior_point.hpp:488-563, :775-832) as kernels on
 * the state already in HBM; only the scalars below cross PCIe.  slpx_problem_solve() runs
 * on these; a maintainer binding at the linear-solver or AD seam does not need them.
 *
 * slpx_ipm_direction: for the step left by slpx_newton_step —
 *   out[3] = {alpha_max = ftb(s, p_s, tau), alpha_z = ftb(z, p_z, tau)
 *             (util/fraction_to_the_boundary_rule.hpp:19-43),
 *             D_phi = g.p_x - mu sum(p_s / s) (interior_point.hpp:508-509)}
 * slpx_ipm_trial: trial x = x + alpha p_x, forward sweep of f, c_e, c_i there —
 *   out[4] = {f, |c_e|_1 + |c_i - s_trial|_1, sum ln s_trial, all finite (1/0)}
 *   (the filter entry of util/filter.hpp:30-60 is {f - mu out[2], out[1]});
 *   s_trial = s + alpha p_s, or the trial c_i when s_from_ci (feasible-IPM option, :520-526)
 * slpx_ipm_commit: x += alpha p_x, s := s_trial, y += alpha_z p_y, z += alpha_z p_z, then
 *   the z reset of interior_point.hpp:797-801 (mu = the value last set with set_state)
 * slpx_ipm_errors: at the resident iterate with V from the last FULL sweep; error_scales =
 *   [d_f, d_ce, d_ci] used for un-scaling (util/kkt_error.hpp:216-251) —
 *   out[24] = {un-scaled: |g - A_e^T y - A_i^T z|_inf, |s.z|_inf, |c_e|_inf, |c_i - s|_inf,
 *              |y|_1, |z|_1;  scaled: the same dual residual, min s.z, max s.z, |c_e|_inf,
 *              |c_i - s|_inf, |y|_1, |z|_1;  f, |c_e|_1 + |c_i - s|_1, sum ln s;
 *              |A_e^T c_e|_2^2, |c_e|_2^2, |A_i^T c_i^-|_2^2, |c_i^-|_2^2
 *              (util/is_locally_infeasible.hpp:17-60);  |x|_inf, |s|_inf, all finite,
 *              all c_i > 0}  (util/kkt_error.hpp:92-146 combines the first thirteen) */
int slpx_ipm_direction(slpx_system* s, double tau, double* out3);
int slpx_ipm_trial(slpx_system* s, double alpha, int s_from_ci, double* out4);
int slpx_ipm_commit(slpx_system* s, double alpha, double alpha_z, int s_from_ci);
int slpx_ipm_errors(slpx_system* s, const double* error_scales, double* out24);

/* Per-kernel-group durations with HIP events on the system's stream: every phase of the
 * step is enqueued `iters` times back to back between one pair of events (the phases are
 * idempotent on the resident state), so the figure is the kernel's own duration — the one
 * rocprofv3 --stats reports — without the ~20 us an event pair around a single launch adds.
 * (Batches of 16 or more: one launch per phase per iteration, events between the phases.)
 * ms[8] = {sweep, assemble, rhs, factor (x attempts the policy loop needs), backward solve,
 * backsub, sum, factorizations per step} */
int slpx_system_time_step(slpx_system* s, int iters, int refresh_ad, float* ms);

/* The same for the launches a single problem's Newton step actually makes (device.hpp: KktFuse,
 * BacksubFuse, ldlt_mf_step_kernel): ms[4] = {AD sweep launch, the launch that evaluates the
 * KKT system, factorizes, solves and back-substitutes (first attempt of the policy loop's
 * settled regularization), their sum, 1 if that single launch exists for this system — 0: the
 * step is made of the kernels slpx_system_time_step times and ms[1] is their sum} */
int slpx_system_time_fused_step(slpx_system* s, int iters, float* ms);

/* Profiling aid: wall_clock64() ticks (100 MHz) recorded by workgroup 0 of the last tape
 * sweep at {entry, staged, leaves, forward done, values out, adjoints done, exit};
 * out16[0..7] = 64-thread kernel, out16[8..15] = 256-thread kernel. */
int slpx_debug_tape_clocks(slpx_system* s, uint64_t* out16);
/* Same for the first task of one LDLT round: out24[0..7] factor {entry, staged, values
 * gathered, levels done, update blocks done, exit}, [8..15] forward solve, [16..23]
 * backward solve.  Returns what was recorded so far, then arms `next_round`. */
int slpx_debug_ldlt_clocks(slpx_system* s, uint32_t next_round, uint64_t* out24);
/* With SLPX_TAPE_JIT_CLOCKS=1 in the environment when the system was made: ticks of the first
 * `blocks` (<= 2048) workgroups of the generated tape kernel's last launch, out[8*blocks]: {entry,
 * exit, body entered, leaves loaded, forward part done, -, -, -} per workgroup.
 * Returns the number of workgroups that run generated bodies (the rest interpret), or -1. */
int slpx_debug_tmpl_clocks(slpx_system* s, uint64_t* out, int32_t blocks);
/* Test hook for chained steps (consecutive slpx_newton_step calls of one problem: the AD sweep and the
 * step kernel side by side, ordered through words in memory with BOUNDED spins).  action 1: the next
 * chained sweep is told to wait for a step kernel that does not exist — it gives up after its bound,
 * the step reports the failure instead of computing on a torn V, and the library redoes that step
 * unchained.  Returns the number of chain failures recovered from so far (action 0: just that). */
int slpx_debug_chain(slpx_system* s, int action);

#ifdef __cplusplus
}
#endif
#endif /* SLPX_H_ */
