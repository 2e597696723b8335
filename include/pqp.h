/*
 * pqp.h — C ABI of the MI355X-native batched path-QP engine (libpqp_hip.so).
 *
 * Drop-in boundary for the ONE hot path of LiJiangnanBit/path_optimizer_2: assembling and solving
 * the Frenet path QP behind PathOptimizer::optimizePath / BaseSolver.  Every entry point cites the
 * reference interface it replaces (file:line relative to the reference tree).
 *
 *   reference                                                     this ABI
 *   ------------------------------------------------------------  ---------------------------------
 *   BaseSolver::BaseSolver            src/solver/base_solver.cpp:15-39   pqp_path_sizes / pqp_path_pattern
 *   BaseSolver::setCost               src/solver/base_solver.cpp:119-148 pqp_path_assemble (P diagonal)
 *   BaseSolver::setConstraints        src/solver/base_solver.cpp:150-261 pqp_path_assemble (A values, l, u)
 *   BaseSolver::getSoftBounds         src/solver/base_solver.cpp:290-295 (inside the assemble kernel)
 *   BaseSolver::solve                 src/solver/base_solver.cpp:56-95   pqp_path_solve (warm = 0, passes = 0)
 *   BaseSolver::updateProblemFormulationAndSolve      :97-117            pqp_path_solve (warm = 1, lin = input)
 *   BaseSolver::getOptimizedPath      src/solver/base_solver.cpp:263-288 (unpack, fused into the solve kernel)
 *   PathOptimizer::optimizePath       src/path_optimizer.cpp:124-161     pqp_path_solve (passes = 1)
 *   OsqpEigen::Solver initSolver/solve (third party, called at base_solver.cpp:87-88,110)
 *                                                                 the ADMM loop inside the solve kernel
 *   TensionSmoother2::osqpSmooth      src/reference_path_smoother/tension_smoother_2.cpp:20-158   pqp_smooth_tension2
 *   TensionSmoother::osqpSmooth       src/reference_path_smoother/tension_smoother.cpp:49-177     pqp_smooth_tension
 *   ReferencePathSmoother::postSmooth src/reference_path_smoother/reference_path_smoother.cpp:526-636 (QP part) pqp_post_smooth
 *   ReferencePath::updateBounds -> ReferencePathImpl::updateBoundsImproved
 *                                     src/data_struct/reference_path.cpp:61, reference_path_impl.cpp:177-312    pqp_corridor_bounds
 *   ReferencePath::updateBoundsOnInputStates    reference_path.cpp:89-91, reference_path_impl.cpp:118-175   pqp_corridor_bounds_on_states
 *   ReferencePathImpl::buildReferenceFromSpline  reference_path_impl.cpp:314-338, PathOptimizer::processInitState path_optimizer.cpp:73-85
 *                                                                                                         pqp_reference_states
 *   ReferencePathSmoother::postSmooth (tail)    reference_path_smoother.cpp:559-573                         pqp_offsets_to_points
 *   PathOptimizer::setReferencePathLength       path_optimizer.cpp:87-104                                   pqp_reference_length
 *   getProjection + global2Local      src/tools/tools.cpp:57-126                                           pqp_project_points
 *   ReferencePathSmoother::bSpline              reference_path_smoother.cpp:490-521                         pqp_bspline_resample
 *   ReferencePathSmoother::segmentRawReference  reference_path_smoother.cpp:48-85                           pqp_segment_raw_reference
 *   tk::spline::set_points            src/tools/spline.cpp:161-249                                         pqp_spline_fit
 *   ReferencePathSmoother::graphSearchDp  src/reference_path_smoother/reference_path_smoother.cpp:142-295   pqp_dp_corridor
 *
 * Conventions
 *   - plain C, no C++/torch types; all reals are IEEE fp64, all indices int32.
 *   - every function returns 0 on success or a negative pqp_error; nothing throws across the ABI.
 *   - `*_device` entry points take DEVICE pointers and enqueue on the handle's HIP stream without
 *     synchronising; pqp_sync() waits.  The non-suffixed entry points take HOST pointers, copy in,
 *     run, copy out and synchronise (that is what the C++ BaseSolver shim uses with batch = 1).
 *   - the handle owns all device memory and its stream; callers own every buffer they pass; no
 *     caller pointer is retained after a call returns (device entry points: after pqp_sync()).
 *   - a handle is single-owner and not re-entrant; use one handle per GPU / host thread.
 *   - there is NO CPU fallback: if no HIP device is usable, pqp_create fails with PQP_ERR_NO_DEVICE.
 *
 * Array layouts (C-contiguous, fp64) — AoS per waypoint, the way State/SlState vectors are walked
 * (reference include/data_struct/data_struct.hpp:14-32,74-93):
 *   ref    [batch][n][5]   s, k, heading, x, y          ReferencePath::getReferenceStates()
 *   lin    [batch][n][3]   l, d_heading, k              input_path_ (the linearisation point); NULL =>
 *                                                       (0, 0, k_ref) as path_optimizer.cpp:128-137
 *   bounds [batch][n][6]   front lb, ub, rear lb, ub, center lb, ub      ReferencePath::getBounds()
 *   scal   [batch][6]      init_error[0], init_error[1], start_state.k, target_state.heading,
 *                          blocked (0/1: ReferencePath::isBlocked()!=nullptr), max_steering_angle
 *   out    [batch][n][7]   x, y, heading, l, d_heading, k, d_k           the SlState fields
 *                                                       getOptimizedPath fills (s, v, a stay 0 there)
 */
#ifndef PQP_H_
#define PQP_H_

#include <stdint.h>
#include "pqp_search_params.h"      /* pqp_search_params, the parameters of pqp_speed_search (below) */

#ifdef __cplusplus
extern "C" {
#endif

#define PQP_REF_STRIDE 5
#define PQP_LIN_STRIDE 3
#define PQP_BOUNDS_STRIDE 6
#define PQP_SCAL_STRIDE 6
#define PQP_OUT_STRIDE 7
#define PQP_INFO_STRIDE 8

typedef enum pqp_error {
    PQP_OK = 0,
    PQP_ERR_INVALID = -1,      /* bad argument (null pointer, n or batch out of range)            */
    PQP_ERR_NO_DEVICE = -2,    /* no usable HIP device: the product path has no CPU fallback      */
    PQP_ERR_HIP = -3,          /* a HIP runtime call failed; see pqp_last_error()                 */
    PQP_ERR_CAPACITY = -4      /* batch / n exceed what the handle was created for                */
} pqp_error;

/* Per-QP termination status written to status[batch] (osqp-eigen collapses this to bool). */
typedef enum pqp_status {
    PQP_STATUS_UNSOLVED = 0,
    PQP_STATUS_SOLVED = 1,         /* both residual tests passed (and, with polish on, the KKT-verified polish
                                      was accepted or ADMM reached 1e-10)             -> solve() == true  */
    PQP_STATUS_MAX_ITER = 2,       /* max_iter reached                                  -> solve() == false */
    PQP_STATUS_NUMERICAL = 3,      /* NaN/Inf in the iterates, or a scenario that is not a number: NaN / Inf among its reference states,
                                      bounds, linearisation point or start state, or an arclength s that does not increase (the reference
                                      divides by ds, base_solver.cpp:174,180).  Checked inside both path kernels (host- and device-pointer
                                      entry points alike): such a QP ends here before its first iteration, its output record is all
                                      zeros, the other QPs of the batch are not affected.  An absent bound is +-1e30 (OSQP_INFTY),
                                      not an IEEE infinity                              -> solve() == false */
    PQP_STATUS_PRIMAL_INFEASIBLE = 4   /* OSQP's primal infeasibility certificate holds  -> solve() == false */
} pqp_status;

/* The scalars the path reads.  Defaults (pqp_default_params) are the reference's gflags defaults
 * (src/config/planning_flags.cpp) and the constants hard-coded in base_solver.cpp. */
typedef struct pqp_params {
    /* car / planning flags */
    double front_length;              /* planning_flags.cpp:20   3.9   */
    double rear_length;               /* planning_flags.cpp:18  -1.0   */
    double wheel_base;                /* planning_flags.cpp:16   2.5   */
    double expected_safety_margin;    /* planning_flags.cpp:95   0.6   */
    double precise_planning_length;   /* planning_flags.cpp:114  30.0  */
    int32_t constraint_end_heading;   /* planning_flags.cpp:98   1     */
    int32_t rough_constraints_far_away; /* planning_flags.cpp:112 0    */
    /* constants of base_solver.cpp */
    double weight_l;                  /* :123  0    */
    double weight_kappa;              /* :124  20   */
    double weight_dkappa;             /* :125  100  */
    double weight_slack;              /* :126  10   */
    double end_l_bound;               /* :250-251  1.0   */
    double end_psi_tol;               /* :257-258  0.087 */
    double end_psi_max;               /* :256  70 deg    */
    double min_clearance;             /* :292  0.1       */
    /* solver settings (OSQP names; base_solver.cpp:59-62 sets eps to 2e-3, the rest are OSQP defaults) */
    double eps_abs;
    double eps_rel;
    double rho;                       /* 0.1   */
    double sigma;                     /* 1e-6  */
    double alpha;                     /* 1.6   */
    int32_t max_iter;                 /* 4000  */
    int32_t scaling;                  /* 10 Ruiz passes (OSQP's default).  k < 0 (path QP only; production: -4): |k| passes of the same equilibration
                                         evaluated on ONE interior waypoint's blocks and taken by every waypoint (no exchange, no reduction: ~1 us
                                         instead of ~2 us per pass).  A valid positive diagonal scaling - any is - that equals what |k| full passes
                                         give on the tested scenario families (uniform spacing, default flags, a pass linearised around the
                                         reference line); it ignores what only single waypoints carry (first / last waypoint's rows, rough rows,
                                         varied spacing).  Meant for handles with polish != 0, whose result does not depend on the metric: with
                                         polish == 0 the eps-accurate iterates then differ from OSQP's.  |k| <= 64 (pqp_set_params). */
    int32_t adaptive_rho;             /* 1     */
    int32_t adaptive_rho_interval;    /* 100 (OSQP's "auto" value without wall-clock profiling).  This field, check_termination and polish_every < 0
                                         (pqp_production_params: -1): by path length - 5 iterations for paths of up to 90 waypoints, 8 beyond
                                         (measured: profiles/r05x_polish_every_seeds_configs.txt; the smoother QPs: 8) */
    double adaptive_rho_tolerance;    /* 5     */
    int32_t check_termination;        /* 25    (< 0: see adaptive_rho_interval) */
    /* solution polishing (OSQP paper section 4.2; OSQP default and the reference: off).  When on, the active
     * set the ADMM iterate predicts is solved as an equality-constrained QP (regularised KKT + iterative
     * refinement) and ACCEPTED ONLY IF the polished point passes a KKT check (primal feasibility of inactive
     * rows, dual signs of active rows, stationarity) - i.e. it is then the exact optimum of the QP.  A
     * rejected polish resumes ADMM with a 10x tighter internal tolerance and tries again later. */
    int32_t polish;                   /* 0 (reference) ; bench and parity tests use 1.  Smoother QPs with polish != 0 return exact optima
                                         with iters = 0 where the QP's structure allows: TensionSmoother2's (equality rows only: a linear-
                                         quadratic control problem) by one Riccati sweep per scenario; with polish == 1 postSmooth's (a box
                                         QP in the offsets) and TensionSmoother's (a box QP in the lateral shifts) by a KKT-verified
                                         active-set solve, one wavefront per scenario (any count of layers / points: up to 1024 in the
                                         wavefront's registers, beyond with the lane state in an HBM workspace).  With polish == 2 QPs with inequality rows run the plain ADMM.  The path QP treats 2
                                         like 1 */
    int32_t polish_refine_iter;       /* 4     */
    int32_t polish_every;             /* 0: only when the residual test passes; k: also try every k iterations; < 0: see adaptive_rho_interval */
    int32_t polish_warm_set;          /* 1: a warm re-linearised re-solve starts with a polish on the previous pass's active set;
                                         2: ... and keeps that pass's equilibration (D, E, c) instead of re-running Ruiz */
    int32_t polish_max_rounds;        /* 40: active-set correction rounds per polish attempt; <= 0: max(24, n/5 - 8) (40 for the smoothers) */
    int32_t polish_reseed;            /* 1: a polish attempt that gives up hands its best point (smallest KKT failure) to ADMM as the
                                         new iterate when that failure is below polish_reseed_factor x the ADMM residuals */
    int32_t polish_diverge;           /* k > 0: an attempt gives up as soon as the KKT failure exceeds k x the smallest one seen in it */
    double polish_delta;              /* 1e-6  regularisation; active rows get penalty 1/delta */
    double polish_tol;                /* 1e-7  KKT acceptance tolerance of the polished point  */
    double polish_reseed_factor;      /* 1.0   */
    double eps_prim_inf;              /* 1e-4  OSQP's primal infeasibility tolerance; <= 0: no certificate test */
    int32_t polish_patience;          /* 0: a pass ends only with an accepted polish (or max_iter).  k > 0: once ADMM has met its
                                         residual test and the gap between polish attempts has doubled k times without an accepted
                                         polish, the ADMM point is returned as PQP_STATUS_SOLVED without polish - OSQP's behaviour when
                                         its polish fails (info[4] counts the polished passes).  With polish_every = 0: at once. */
    int32_t prim_inf_after;           /* 0: OSQP's certificate on y_k - y_{k-1} at every termination check (the kernel variant with the
                                         certificate in its loop, ~12 % slower iterations).  k > 0: the lean kernel; from iteration k on every
                                         termination check that neither converged nor started a polish evaluates the SAME certificate on
                                         dy = y_now - y_at_the_previous_such_check (any dy that passes it proves infeasibility): nothing in
                                         the ADMM loop, an infeasible QP stops about two checks after iteration k */
    int32_t polish_lazy;              /* 0: every active-set round refines its point with polish_refine_iter solves before it is looked at.
                                         k > 0: a round first looks after ONE solve; during the first k full rounds of an attempt rows that
                                         fail the test by more than 10 x that solve's residual change sides at once, the remaining
                                         refinement solves only run when nothing moves that far (they are what the KKT acceptance test
                                         needs, not what the set update needs).  The accepted point is always a fully refined one. */
    int32_t polish_final_refine;      /* 0.  k: an ACCEPTED polished point gets k more refinement solves (each followed by the KKT test again).  The path QP
                                         beyond 128 waypoints runs with at least 1, beyond 256 with at least 3: residuals of 1e-9 in the transition rows - a discrete double
                                         integrator - add up to 1e-4 in l over 300 waypoints, and a refinement solve shrinks them 100-1000x.  Honoured by the kernels of
                                         paths beyond 128 waypoints only (the shorter paths' kernels do not compile the feature in: nothing to refine away there); in a
                                         launch of mixed lengths (pqp_path_solve_var) this level and the three intervals above follow the launch's n_max, not the QP's own n */
    /* smoother QP weights (src/config/planning_flags.cpp:51-61) */
    double tension2_deviation_weight;        /* 0.005 */
    double tension2_curvature_weight;        /* 1     */
    double tension2_curvature_rate_weight;   /* 10    */
    double cartesian_curvature_weight;       /* 1     */
    double cartesian_curvature_rate_weight;  /* 50    */
    double cartesian_deviation_weight;       /* 0     */
} pqp_params;

typedef struct pqp_sizes {
    int32_t n, state, control, precise, slack, vars, cons, nnz_a, nnz_p;
} pqp_sizes;

typedef struct pqp_handle pqp_handle;

void pqp_default_params(pqp_params* p);
/* the defaults with the engine's production solver setting (1e-4 + KKT-verified polish; pqp_defaults.hpp) */
void pqp_production_params(pqp_params* p);
const char* pqp_last_error(void);
const char* pqp_version(void);

/* One handle per GPU.  max_batch / max_n size the device workspaces (they grow on demand). */
int pqp_create(pqp_handle** h, const pqp_params* params, int device, int max_batch, int max_n);
int pqp_destroy(pqp_handle* h);
int pqp_set_params(pqp_handle* h, const pqp_params* params);
/* Handle options (not solver settings: results never depend on them).
 *   PQP_OPT_STORE_WARM (default 1)     keep the final primal/dual iterate of every solve on the handle: what warm == 1 and
 *                                      pqp_path_get_solution read (BaseSolver keeps its OSQP workspace the same way,
 *                                      base_solver.hpp:62).  0 saves the write when every call is a complete optimizePath.
 *   PQP_OPT_ORDER_BY_COST (default 0)  start the QPs of a batch most-expensive-first, by the reduced-KKT solves and
 *                                      factorisations each QP needed in the handle's previous solve of the same batch and n
 *                                      (a planner re-solves nearly the same scenarios every cycle).  The first solve of a shape
 *                                      runs in index order.  On the lane-per-QP kernel (batches that put a wavefront on nearly every SIMD) the same option groups
 *                                      the QPs into wavefronts of similar work - see PQP_OPT_STREAM_BATCH below.
 *   PQP_OPT_RESERVE_CUS (default 0)    compute units the path QP's persistent workgroups leave free.  Their wavefronts own a SIMD's whole
 *                                      register file, so kernels of another stream (the smoother chain of the next batch, configs[4]) only
 *                                      get onto the chip when a unit is left to them.
 *   PQP_OPT_STREAM_BATCH (default -1 = by measurement: pqp_stream_batch_default(n) - the measured crossover of the two kernels on one MI355X, one launch after the
 *                                      other: 15 360 x max(1, n / 80)^1.5 up to 128 waypoints (15 k QPs at 80, 29 k at 120), 0.75 n^2 up to 256 (where the lane-per-
 *                                      waypoint kernel runs half as many QPs at a time), 48 n beyond; profiles/r06ay_*, r06az_*; 0: never)
 *                                      cold solves (warm == 0) of at least this many QPs on a handle with polish != 0 and
 *                                      PQP_OPT_STORE_WARM off run on the lane-per-QP kernel (one QP per lane, 64 per wavefront, the
 *                                      per-waypoint state streamed through a batch-interleaved workspace of 240 n bytes per QP in HBM;
 *                                      csrc/pqp_path_lq.hpp): the path QP as a linear-quadratic control problem, interior-point rounds +
 *                                      active-set rounds whose last round is the KKT test, i.e. the same exact optimum as the lane-per-
 *                                      waypoint kernel's verified polish.  It wins where the batch fills the chip's 65 536 lanes (65 536
 *                                      QPs of 80 waypoints: 1.9x); it keeps no warm state
 *                                      (hence the PQP_OPT_STORE_WARM condition), iters[] counts its interior-point iterations and info[] =
 *                                      {row residual, complementarity, iterations of the first pass, iterations, solved passes, active-set
 *                                      rounds of the first pass, Riccati sweeps, active-set rounds}.  PQP_OPT_ORDER_BY_COST on this kernel (round 5; batches of at least
 *                                      768 wavefronts, not with PQP_OPT_CARRY_CYCLES): the wavefronts of a solve hold QPs that ran the same interior-point iterations and
 *                                      active-set rounds per pass in the handle's previous solve of the shape - a wavefront runs every phase as often as its slowest lane:
 *                                      65 536 QPs 10.5 -> 9.7 ms with the identical batch's counts, 11.2 -> 10.4 ms on jittered planning cycles, 98 304 QPs 17.5 -> 13.0 ms
 *                                      (profiles/r05g_stream_sorted_probe.txt, r05i_*); HBM traffic 1.31x -> 1.03x the algorithmic bytes.
 *                                      Round 6: in such a sorted launch (the second solve of a shape onwards) a re-linearised pass first tries the previous pass's
 *                                      active set on the new transition rows - up to three active-set rounds, a confirmed set being the KKT test of that pass's
 *                                      QP - before the interior-point rounds get their turn (98 % of the bench's QPs confirm: 14.0 instead of 17.5 sweeps per path,
 *                                      65 536 QPs 7.7 -> 9.0 M paths/s with two launches in flight, profiles/r06ae_*).  The optimum is the same one; reached through other
 *                                      arithmetic it agrees with an unsorted launch's to the rounds' tolerances (< 5e-7 in l, psi, kappa), and a sorted launch
 *                                      reproduces the previous sorted launch bit for bit.
 *   PQP_OPT_CARRY_CYCLES (default 0)   a cold call (warm == 0, lin == NULL) starts the FIRST pass of QP k from the optimum QP k had in the handle's
 *                                      previous solve of the same batch and n instead of cold (lane-per-waypoint kernel: from the warm state it then keeps
 *                                      - final iterate, equilibration, active set, kept per waypoint: counts per QP may change between the calls; lane-per-QP kernel: from its workspace) - a planner re-solves
 *                                      nearly the same scenarios cycle after cycle; the reference constructs a fresh BaseSolver every cycle
 *                                      (path_optimizer.cpp:138).  The optimum returned is the same (unique; it agrees with the cold solve to the
 *                                      1e-7 of the KKT test); on scenarios that moved by 5 %: configs[1] 4.0 M instead of 3.1 M paths/s and no stragglers
 *                                      (profiles/r03n_seed_sweep.txt, r03y_seed_sweep.txt); lane-per-QP kernel 14 -> 9 interior-point iterations per path.
 *                                      (On that kernel the option switches the sorted launches of PQP_OPT_ORDER_BY_COST off - a slot's workspace belongs to the QP that sat there - and
 *                                      since round 6 those are the faster of the two from 768 wavefronts on: 65 536 QPs 7.8 M paths/s sorted against 6.6 M carried, profiles/r06am_bench_n1.json.)
 *                                      A QP that differs wildly from its slot's previous one is still solved (the start is then merely poor).
 *                                      Value k = 2..64 ("tails", lane-per-waypoint kernel, needs PQP_OPT_ORDER_BY_COST): only the QPs that were among the most
 *                                      expensive 1 / k of the handle's previous solve of the shape start from their previous optimum, all others start
 *                                      cold - a launch lasts as long as its slowest QPs, and those are the ones a cold active-set search wanders on
 *                                      (a carried QP keeps its cold cost key, one bin less per cycle, so that it stays among the carried ones).  configs[1], one
 *                                      launch at a time: k = 8 2.47 M against 2.01 M paths/s cold, the slowest QP 29 instead of 48 reduced solves
 *                                      (profiles/r05c_*).
 *                                      The exact TensionSmoother / postSmooth kernels (polish == 1) honour it too: a line's active-set rounds start from
 *                                      the set its slot ended with in the previous solve of the shape (16-31 rounds from the cold start, 2-3 from there).
 *   PQP_OPT_STREAM_STAGED (default -1 = by launch size)
 *                                      the lane-per-QP kernel has two forms.  A launch that fills the chip (768 wavefronts = 49 152 QPs or more) is bound by HBM's throughput:
 *                                      its workspace is laid out [field][lane], every access one contiguous line, a sweep's records prefetched one waypoint ahead in registers.
 *                                      A launch that leaves SIMDs idle waits for its loads: its workspace is laid out in 16-byte chunks per lane and the sweeps' records are staged in
 *                                      LDS two waypoints ahead by LDS-direct loads (global_load_lds_dwordx4) - +29 ... 33 % at 24 576 / 32 768 QPs of 80 waypoints one launch at a
 *                                      time, -3 ... 4 % where the chip is full (profiles/r06au_*).  Same arithmetic, same paths.  0 / 1 force one form (tests, measurements).
 *   PQP_OPT_CHAIN_GRAPH (default 0)    pqp_optimize_path_device replays a captured hipGraph: the third call with the same arguments (pointers, sizes, configuration,
 *                                      parameters of both handles) captures its ~25 launches on the handles' streams, later calls with those arguments are ONE
 *                                      hipGraphLaunch - the gaps between the launches were 13 % of the chain.  Results are bit-identical; any (re)allocation inside
 *                                      the library, or other arguments, falls back to plain launches (and a new capture).  Set it on the path handle.
 *                                      A replay runs on the path handle's stream; it is fenced against the smoother handle's stream on both sides
 *                                      (work the caller enqueues there stays ordered as with plain launches).  Value 2: no fences (-3.6 % time) -
 *                                      the caller guarantees that the smoother handle's stream carries no other work while chains are in flight.
 *   PQP_OPT_LONG_LINES (default 0)     lines of any length in the line-geometry steps (pqp_spline_fit*, pqp_reference_states, pqp_segment_raw_reference,
 *                                      pqp_reference_length, pqp_offsets_to_points, pqp_bspline_resample, pqp_dp_corridor, pqp_corridor_bounds*).  Their kernels
 *                                      stage a line's spline table (9 doubles per knot) and their per-element arrays in one CU's LDS, which caps the line
 *                                      (the DP search first, at about 880 m of smoothed line).  0: those kernels only, PQP_ERR_CAPACITY past their LDS.
 *                                      1: per launch, the LDS kernel where its LDS fits, otherwise a long form that reads the table from HBM (through the
 *                                      caches) and keeps the per-element arrays in a workspace of the handle.  2: the long forms always (tests, measurements).
 *                                      The long forms compute in the same order as the LDS kernels: the same bits.  Set it on the path handle for
 *                                      pqp_optimize_path_device: every line step of the chain runs there.   */
typedef enum pqp_option { PQP_OPT_STORE_WARM = 1, PQP_OPT_ORDER_BY_COST = 2, PQP_OPT_RESERVE_CUS = 3, PQP_OPT_STREAM_BATCH = 4, PQP_OPT_CARRY_CYCLES = 5, PQP_OPT_CHAIN_GRAPH = 6, PQP_OPT_STREAM_STAGED = 7,
                          PQP_OPT_LONG_LINES = 8 } pqp_option;
int pqp_set_option(pqp_handle* h, int option, int value);
int pqp_get_stream(pqp_handle* h, void** hip_stream);   /* hipStream_t */
/* The handle's stream is created non-blocking: work the caller enqueued on ANOTHER stream (the inputs of a *_device call produced by
 * its own kernels or copies; NULL = the default stream) is not ordered before the handle's launches unless the caller says so:
 * pqp_stream_wait makes everything enqueued on the handle from now on wait for what is enqueued on `hip_stream` up to now. */
int pqp_stream_wait(pqp_handle* h, void* hip_stream);
/* Ordering between two handles (= two streams) without the host waiting - BASELINE configs[4]: the smoother QP of scenario batch k on
 * one handle, the path QP of batch k on another, the smoother of batch k + 1 overlapping the path QP of batch k.  pqp_mark records
 * the handle's event `slot` (0..7) behind everything enqueued on it so far; pqp_wait_mark makes everything enqueued on `h` from
 * now on wait for `other`'s mark `slot` as it was recorded last. */
int pqp_mark(pqp_handle* h, int slot);
int pqp_wait_mark(pqp_handle* h, pqp_handle* other, int slot);
int pqp_sync(pqp_handle* h);

/* BaseSolver ctor (base_solver.cpp:15-39): problem sizes.  `s` = the n arclengths of the path
 * (only read when rough_constraints_far_away), may be NULL otherwise.  Pure integer host function. */
int pqp_path_sizes(const pqp_params* params, int n, const double* s, pqp_sizes* out);

/* Value-independent sparsity of A in CSC order (17N-5 slots when precise == n) and the columns of
 * the diagonal P, in the REFERENCE variable / row numbering (base_solver.cpp:154-209,127-143).
 * P's columns are the ones the reference's sparseView keeps (base_solver.cpp:145): k_i, u_i and the slacks - and, when the handle's weight_l is not zero, l_i
 * (pcols ascending, nnz_p = pqp_path_sizes' with the same parameters; with the default weight_l = 0 the l columns are absent as in the reference).
 * Computed by a HIP kernel.  rows[nnz_a], colptr[vars+1], pcols[nnz_p] are HOST buffers. */
int pqp_path_pattern(pqp_handle* h, int n, int precise, int32_t* rows, int32_t* colptr, int32_t* pcols);

/* setCost + setConstraints for a batch: values in the pattern's order.
 *   a_val [batch][nnz_a]   p_val [batch][nnz_p]   lower/upper [batch][cons]
 * All QPs of one call share n and `precise`.  Host-pointer and device-pointer variants. */
int pqp_path_assemble(pqp_handle* h, int batch, int n, int precise, const double* ref, const double* lin,
                      const double* bounds, const double* scal,
                      double* a_val, double* p_val, double* lower, double* upper);
int pqp_path_assemble_device(pqp_handle* h, int batch, int n, int precise, const double* ref,
                             const double* lin, const double* bounds, const double* scal,
                             double* a_val, double* p_val, double* lower, double* upper);

/* Assemble + ADMM solve + unpack, `passes` re-linearised warm re-solves fused in one launch
 * (PathOptimizer::optimizePath == passes 1).
 *   warm == 0: cold start (BaseSolver::solve).  warm == 1: start from the primal/dual/rho the handle
 *   kept from its previous pqp_path_solve* call with the same batch and n
 *   (BaseSolver::updateProblemFormulationAndSolve: pass the previous output as `lin`).
 *   status[batch], iters[batch] (total ADMM iterations over all passes) may be NULL.
 *   info (may be NULL) [batch][PQP_INFO_STRIDE]: primal residual, dual residual, final rho, ADMM iterations of the
 *   last pass, number of accepted polishes, total reduced-KKT solves (ADMM iterations + polish refinement),
 *   number of factorisations, reserved.
 *   n >= 2 waypoints, any batch.  Up to 512 waypoints: one lane per waypoint (1, 2, 4 or 8 wavefronts per QP); beyond (and for large batches,
 *   PQP_OPT_STREAM_BATCH): one lane per QP, which returns exact optima in every solver setting (zero residuals meet OSQP's termination test at
 *   any eps) and keeps no warm state: beyond 512 waypoints warm == 1 solves the QP around `lin` cold - same optimum - and
 *   pqp_path_get_solution is not available.  Which solver runs is decided
 *   by the handle's pqp_params: pqp_default_params = the reference's OSQP setting (eps 2e-3, no polish, infeasibility certificate),
 *   pqp_production_params = eps 1e-4 + KKT-verified polish.  When status[q] != SOLVED (the reference's solve() returns false there and
 *   leaves its output vector untouched) out[q] is defined but kernel-specific: the lane-per-waypoint kernel leaves its last iterate there;
 *   the lane-per-QP kernel the optimum of the last pass that WAS solved, or - when none was - the reference line itself (l = dpsi = 0).
 *   iters[] and info[] differ between the two kernels as well (above; PQP_OPT_STREAM_BATCH): pqp_last_path_kernel says which one served
 *   the handle's last solve, so that a caller can tell what it received.
 *   A start curvature scal[q][2] outside the curvature box by no more than OSQP's primal tolerance eps_abs + eps_rel * bound is projected onto the
 *   box by both kernels (strictly such a QP has no feasible point; OSQP at that eps calls it solved with a point that misses the row by that
 *   little); outside by more: PQP_STATUS_PRIMAL_INFEASIBLE.
 *   A QP with a collision box whose lower bound exceeds its upper bound is refused as OSQP refuses it at setup: the host-pointer
 *   entry points do not launch it and report PQP_STATUS_PRIMAL_INFEASIBLE (out[q] = 0); the *_device entry points do not
 *   validate their inputs (there such a row is pinned to its upper bound). */
int pqp_path_solve(pqp_handle* h, int batch, int n, const double* ref, const double* lin,
                   const double* bounds, const double* scal, int passes, int warm,
                   double* out, int32_t* status, int32_t* iters, double* info);
int pqp_path_solve_device(pqp_handle* h, int batch, int n, const double* ref, const double* lin,
                          const double* bounds, const double* scal, int passes, int warm,
                          double* out, int32_t* status, int32_t* iters, double* info);
/* The same with a waypoint count per QP: n_of[batch] (device pointer, each <= n_max); every array keeps the stride n_max.
 * This is what a road cut short by an obstacle needs (ReferencePathImpl::updateBoundsImproved resizes reference_states_ to the
 * blocked waypoint, reference_path_impl.cpp:225-228; pqp_corridor_bounds reports it as n_valid).  A QP with n_of < 2 is left
 * untouched with status PQP_STATUS_UNSOLVED. */
int pqp_path_solve_var_device(pqp_handle* h, int batch, int n_max, const int32_t* n_of, const double* ref, const double* lin,
                              const double* bounds, const double* scal, int passes, int warm, double* out, int32_t* status,
                              int32_t* iters, double* info);
/* host pointers (n_of included); rows of `out` beyond a QP's own count come back as zeros */
int pqp_path_solve_var(pqp_handle* h, int batch, int n_max, const int32_t* n_of, const double* ref, const double* lin, const double* bounds,
                       const double* scal, int passes, int warm, double* out, int32_t* status, int32_t* iters, double* info);

/* Primal / dual solution of the handle's last solve in the REFERENCE numbering (OsqpEigen::Solver::
 * getSolution(), base_solver.cpp:89,112): x [batch][vars], y [batch][cons].  HOST buffers; either may be NULL. */
int pqp_path_get_solution(pqp_handle* h, int batch, int n, int precise, double* x, double* y);

/* constrainAngle (include/tools/tools.hpp:24-35: wrap to [-pi, pi], both ends inclusive) exactly as the kernels of this library evaluate
 * it for the end-heading rule (base_solver.cpp:254-258) and the unpack (base_solver.cpp:272-275): out[i] = constrainAngle(in[i]).
 * DEVICE pointers.  It exists so that the helper can be pinned bit for bit against the reference's own template
 * (oracle/_ref/libref_types.so, tests/test_ref_types.py). */
int pqp_constrain_angle_device(pqp_handle* h, int count, const double* in, double* out);

/* ---- one node, several GPUs -----------------------------------------------------------------------------------
 * The QPs of a batch are independent: the batch is cut into contiguous shards (pqp_shard_range: the first total % world shards get one
 * QP more), every shard has its own handle - GPU, stream, workspaces - and its own host thread; pqp_multi_path_solve moves each
 * shard's slice of the caller's HOST arrays to its GPU, solves it there (pqp_path_solve / pqp_path_solve_var when n_of is given) and
 * brings the paths back.  No collective: with the consumer on the host, per-GPU copies beat a device-side gather.  devices[n_shards]
 * = the device ordinal of every shard (NULL: 0, 1, ...; the same ordinal may appear twice: two handles on one GPU).  The reference
 * has no counterpart (it solves one path per call, base_solver.cpp:56-95). */
typedef struct pqp_multi pqp_multi;
void pqp_shard_range(int total, int world, int rank, int* first, int* count);
int pqp_multi_create(pqp_multi** m, const pqp_params* params, int n_shards, const int* devices, int max_batch_per_shard, int max_n);
int pqp_multi_destroy(pqp_multi* m);
int pqp_multi_shards(const pqp_multi* m);
pqp_handle* pqp_multi_handle(pqp_multi* m, int shard);       /* a shard's own handle (device-resident use, options, timing) */
/* every shard's handle gets the option (PQP_OPT_CARRY_CYCLES: a call whose batch and n equal the previous call's - no lin - starts shard by shard
 * from what the shard's handle kept: the same scenarios one planning cycle later) */
int pqp_multi_set_option(pqp_multi* m, int option, int value);
int pqp_multi_path_solve(pqp_multi* m, int batch, int n, const int32_t* n_of, const double* ref, const double* lin, const double* bounds,
                         const double* scal, int passes, double* out, int32_t* status, int32_t* iters, double* info);
/* The exchange step of SURVEY.md 8e / north_star ("RCCL over xGMI only to gather results") in the C ABI: after pqp_multi_path_solve every shard's
 * paths are still in its GPU's memory; this gathers them over RCCL so that full_out[g] - a buffer of [batch][n][PQP_OUT_STRIDE] doubles in the memory
 * of shard g's GPU - holds the whole batch in the caller's order, for a consumer that lives on the GPUs (the host copy of pqp_multi_path_solve is
 * unaffected).  batch and n as in the preceding solve.  One device per shard; librccl.so is dlopen'ed by the first call, a caller that never
 * gathers does not need it.  The reference has no counterpart (one path per call). */
int pqp_multi_gather_paths(pqp_multi* m, int batch, int n, double* const* full_out);
/* ranks of that gather's communicator as RCCL counts them (ncclCommCount); 0 before the first gather, < 0: error */
int pqp_multi_gather_ranks(pqp_multi* m);

/* ---- reference-line smoothing QPs; the solver settings of the handle apply (the reference runs
 *      them at OSQP's default eps 1e-3: tension_smoother_2.cpp:32-36, tension_smoother.cpp:61-65, reference_path_smoother.cpp:533-537).
 *      All lists are [batch][n] fp64; out_s is the cumulative chord length of the smoothed points. ------------------------- */
/* TensionSmoother2::osqpSmooth   src/reference_path_smoother/tension_smoother_2.cpp:20-72 (default smoothing_method) */
int pqp_smooth_tension2(pqp_handle* h, int batch, int n, const double* x_list, const double* y_list, const double* angle_list,
                        const double* k_list, const double* s_list, double* out_x, double* out_y, double* out_s, int32_t* status,
                        int32_t* iters);
int pqp_smooth_tension2_device(pqp_handle* h, int batch, int n, const double* x_list, const double* y_list, const double* angle_list,
                               const double* k_list, const double* s_list, double* out_x, double* out_y, double* out_s,
                               int32_t* status, int32_t* iters, double* info);
/* TensionSmoother::osqpSmooth    src/reference_path_smoother/tension_smoother.cpp:49-100; clearance = Map::getObstacleDistance
 * at each input point (the distance-map lookup itself, tension_smoother.cpp:168, stays on the caller's side; pqp_clearance_device does it).
 * n >= 4 points, no upper bound (as the reference: one point per metre of line).  Up to 203 points a handle in the reference's ADMM setting
 * (polish == 0) runs OSQP's iteration on the 9 x 9-block core; beyond that core's LDS capacity - and for polish == 1 at any size - the QP is
 * solved exactly (iters = 0), which meets OSQP's termination test at any eps.  The same rule holds for the other two smoothers: where the
 * generic core cannot hold the QP (TensionSmoother2 and TensionSmoother: more than 203 points; postSmooth: more than 251 layers) every handle gets the exact kernel. */
int pqp_smooth_tension(pqp_handle* h, int batch, int n, const double* x_list, const double* y_list, const double* angle_list,
                       const double* clearance, double* out_x, double* out_y, double* out_s, int32_t* status, int32_t* iters);
int pqp_smooth_tension_device(pqp_handle* h, int batch, int n, const double* x_list, const double* y_list, const double* angle_list,
                              const double* clearance, double* out_x, double* out_y, double* out_s, int32_t* status, int32_t* iters,
                              double* info);
/* ReferencePathSmoother::postSmooth QP   src/reference_path_smoother/reference_path_smoother.cpp:526-558,582-636:
 * layers_s, lb, ub [batch][m] (layers_bounds_), vehicle_l [batch] (vehicle_l_wrt_smoothed_ref_); out_l [batch][m] = QPSolution(i) */
int pqp_post_smooth(pqp_handle* h, int batch, int m, const double* layers_s, const double* lb, const double* ub,
                    const double* vehicle_l, double* out_l, int32_t* status, int32_t* iters);
int pqp_post_smooth_device(pqp_handle* h, int batch, int m, const double* layers_s, const double* lb, const double* ub,
                           const double* vehicle_l, double* out_l, int32_t* status, int32_t* iters, double* info);

/* Which kernel served the handle's last pqp_path_solve* call (the dispatch depends on batch size, n, warm and the options above): a
 * pqp_path_kernel, 0 before the first solve; < 0: error. */
typedef enum pqp_path_kernel { PQP_KERNEL_NONE = 0, PQP_KERNEL_LANE_PER_WAYPOINT = 1, PQP_KERNEL_LANE_PER_QP = 2 } pqp_path_kernel;
int pqp_last_path_kernel(pqp_handle* h);
/* PQP_OPT_STREAM_BATCH's default for paths of n waypoints (above). */
int pqp_stream_batch_default(int n);
/* GPU time (ms, hipEvent) of the handle's last solve / assemble launch. */
int pqp_last_kernel_ms(pqp_handle* h, float* ms);
/* the same for the last `count` launches of this handle (oldest first; at most 256): the events are recorded on the handle's stream
 * around every launch and read here after a stream synchronise, so measuring puts nothing between the launches themselves */
int pqp_kernel_ms_history(pqp_handle* h, float* ms, int count);

/* ---- corridor bounds from the obstacle distance map ---------------------------------------------
 * ReferencePath::updateBounds(const Map&)  src/data_struct/reference_path.cpp:61  ->  ReferencePathImpl::updateBoundsImproved
 * (reference_path_impl.cpp:177-230), getClearanceWithDirectionStrict (:232-312), Map::getObstacleDistance (src/tools/Map.cpp:16-22),
 * getDirectionalProjectionByNewton (src/tools/tools.cpp:156-189).  Produces the `bounds` input of pqp_path_solve on the device. */
typedef struct pqp_grid_geometry {       /* grid_map::GridMap geometry of the "distance" layer */
    int32_t rows, cols;                  /* getSize(): cells along x, along y */
    double resolution;
    double length_x, length_y;           /* getLength() = size * resolution */
    double pos_x, pos_y;                 /* getPosition(): map centre */
} pqp_grid_geometry;

typedef struct pqp_corridor_params {
    double front_length, rear_length;    /* 3.9, -1.0   planning_flags.cpp:20,18 */
    double car_width, safety_margin;     /* 2.0, 0.3    planning_flags.cpp:10,14 */
    double epsilon;                      /* 1e-6        planning_flags.cpp:108 (isEqual) */
    double search_radius, delta_s, smaller_ds, search_range, min_space;   /* 0.5, 0.3, 0.05, 6.0, 0.2   reference_path_impl.cpp:238-304 */
    double projection_window;            /* 5.0         reference_path_impl.cpp:194 */
} pqp_corridor_params;

void pqp_corridor_default_params(pqp_corridor_params* p);
/* ref      [batch][n][5]  s, k, heading, x, y of the reference states (the layout pqp_path_solve takes)
 * spline   [batch][9][m]  row 0: knots s; rows 1-4: y, a, b, c of x(s); rows 5-8: y, a, b, c of y(s)  (tk::spline members m_y, m_a, m_b, m_c)
 * spline_ext [batch][4]   m_b0, m_c0 of x(s), then of y(s)
 * dist     [n_maps][cols][rows] float: the layer in Eigen's column-major order (grid_map::Matrix = Eigen::MatrixXf)
 * map_of   [batch] map index of each scenario, or NULL (all use map 0)
 * n_of     [batch] reference states of each scenario (<= n; n is then the array stride), or NULL (all have n)
 * bounds   [batch][n][6]  f_lb f_ub r_lb r_ub c_lb c_ub for every waypoint of the scenario;  n_valid [batch] = index of the first
 *          waypoint whose front or rear interval is empty (the reference cuts the path there and sets isBlocked(), :219-223),
 *          the scenario's own count if none.  n_valid is what pqp_path_solve_var_device takes as n_of. */
int pqp_corridor_bounds_device(pqp_handle* h, int batch, int n, int m, const double* ref, const int32_t* n_of, const double* spline,
                               const double* spline_ext, const float* dist, const int32_t* map_of, const pqp_grid_geometry* geom,
                               const pqp_corridor_params* prm, double* bounds, int32_t* n_valid);
int pqp_corridor_bounds(pqp_handle* h, int batch, int n, int m, const double* ref, const int32_t* n_of, const double* spline,
                        const double* spline_ext, const float* dist, int n_maps, const int32_t* map_of, const pqp_grid_geometry* geom,
                        const pqp_corridor_params* prm, double* bounds, int32_t* n_valid);
/* ReferencePath::updateBoundsOnInputStates (src/data_struct/reference_path.cpp:89-91 -> reference_path_impl.cpp:118-175): the corridor of
 * every waypoint recomputed from the states of a path that was already solved - the second pass PathOptimizer::optimizePath has commented
 * out (src/path_optimizer.cpp:147-151).  The front and rear circle centres of waypoint i sit at
 *   ref.xy + (L - L cos(d_heading_i)) (cos, sin)(ref.heading)        L = prm->front_length / prm->rear_length
 * and are projected on the line from the flag's length (Newton guess s + L, :139-150); the centre circle, the clearance walk and the
 * blocked rule are pqp_corridor_bounds' (the first waypoint whose front or rear interval is empty ends the scenario; its row is written).
 *   states [batch][n][stride]  d_heading at offset 4 (stride >= 5; stride = PQP_OUT_STRIDE reads a path solve's or the chain's `out` in place)
 *   n_of   [batch]             states of each scenario, e.g. the previous pass's n_valid or the chain's n_out (<= n: CHECK_LE, :119), or NULL
 *   ref, spline, spline_ext, dist, map_of, geom, prm, bounds, n_valid   as for pqp_corridor_bounds (ref = the reference states)
 * A d_heading that is not finite gives NaN front / rear rows for that waypoint (never blocked), as the reference's arithmetic does.
 * The host form also refuses (PQP_ERR_INVALID, nothing launched) a map_of value outside [0, n_maps) and an n_of outside [0, n]; with n_of its
 * rows beyond a scenario's states come back as zeros. */
int pqp_corridor_bounds_on_states_device(pqp_handle* h, int batch, int n, int m, const double* ref, const int32_t* n_of, const double* states,
                                         int stride, const double* spline, const double* spline_ext, const float* dist, const int32_t* map_of,
                                         const pqp_grid_geometry* geom, const pqp_corridor_params* prm, double* bounds, int32_t* n_valid);
int pqp_corridor_bounds_on_states(pqp_handle* h, int batch, int n, int m, const double* ref, const int32_t* n_of, const double* states, int stride,
                                  const double* spline, const double* spline_ext, const float* dist, int n_maps, const int32_t* map_of,
                                  const pqp_grid_geometry* geom, const pqp_corridor_params* prm, double* bounds, int32_t* n_valid);

/* ---- the obstacle distance layer from an occupancy grid --------------------------------------------------------------------------
 * cv::distanceTransform(obstacle, dist, CV_DIST_L2, CV_DIST_MASK_PRECISE); dist *= resolution   (src/test/demo.cpp:104-113), for n_maps maps
 * in one call: an exact Euclidean distance transform, in the layout the map-reading entry points take.
 * grid [n_maps][cols][rows] uint8, the layout of dist; a cell is an obstacle iff its byte is 0 (the reference's OCCUPY = 0, FREE = 255)
 * dist [n_maps][cols][rows] float, ready for pqp_corridor_bounds / pqp_dp_corridor / pqp_clearance_device / pqp_optimize_path_device
 * geom as for pqp_corridor_bounds (2 x 2 up to 2^30 cells per map, resolution > 0); only rows, cols and resolution are read.
 * Every cell gets, bit for bit, fl32(fl32(sqrt(d2)) * fl32(resolution)) with d2 the least (dr)^2 + (dc)^2 to an obstacle cell of its map
 * (0 on an obstacle; cells outside the map are not obstacles) and sqrt correctly rounded.  A map without any obstacle cell gets
 * d2 = rows^2 + cols^2 everywhere (hypot(rows, cols) cells: finite, beyond every distance inside the map): our choice, OpenCV's value for
 * that case is not pinned.
 * The _device form takes device pointers, allocates nothing and is asynchronous on the handle's stream (it can be enqueued right in front
 * of pqp_optimize_path_device); the host form copies in, runs, copies out and synchronises.  PQP_ERR_INVALID: a null pointer,
 * n_maps < 1, a bad geometry or a resolution that is not positive (NaN included). */
int pqp_distance_layer_device(pqp_handle* h, int n_maps, const pqp_grid_geometry* geom, const uint8_t* grid, float* dist);
int pqp_distance_layer(pqp_handle* h, int n_maps, const pqp_grid_geometry* geom, const uint8_t* grid, float* dist);

/* ---- reference states from the reference line's spline + the vehicle's initial error -------------------
 * ReferencePathImpl::buildReferenceFromSpline(delta_s_smaller, delta_s_larger)  src/data_struct/reference_path_impl.cpp:314-338
 *   (called with output_spacing / 2, output_spacing = 0.15, 0.3 at path_optimizer.cpp:119; dynamic = FLAGS_enable_dynamic_segmentation)
 * PathOptimizer::processInitState                                              src/path_optimizer.cpp:73-85
 * spline, spline_ext as above; max_s [batch] = ReferencePath::getLength(); start [batch][3] = vehicle start state x, y, heading (or NULL)
 * ref [batch][n_max][5] = s, k, heading, x, y;  count [batch] = states the loop produces (when it exceeds n_max only n_max rows
 * were written; 0 where |max_s| < 1e-6: "ref length is zero", :316-319, the reference returns false and builds none);
 * init_err [batch][2] = initial_offset, initial_heading_error (NULL or needs start): scal[0..1] of pqp_path_solve */
int pqp_reference_states_device(pqp_handle* h, int batch, int n_max, int m, const double* spline, const double* spline_ext,
                                const double* max_s, const double* start, double ds_small, double ds_large, int dynamic, double* ref,
                                int32_t* count, double* init_err);
int pqp_reference_states(pqp_handle* h, int batch, int n_max, int m, const double* spline, const double* spline_ext, const double* max_s,
                         const double* start, double ds_small, double ds_large, int dynamic, double* ref, int32_t* count,
                         double* init_err);

/* ---- lateral offsets on a line -> points with chord-length abscissae -----------------------------------------------------------
 * The tail of ReferencePathSmoother::postSmooth  src/reference_path_smoother/reference_path_smoother.cpp:559-573: x_list(i) =
 * x_s(s_i) + l_i cos(heading(s_i) + pi/2), y_list likewise, s_list = accumulated chord length - the knots of the final reference
 * line (pqp_spline_fit, :574-576; s_list.back() is its length).
 * spline [batch][9][m_spline], spline_ext [batch][4]: the smoothed line; at_s, l [batch][m] = layers_s_list_ and pqp_post_smooth's
 * out_l; m_of [batch] = points per scenario (pqp_dp_corridor's count) or NULL  ->  x, y, s [batch][m] (rows beyond m_of[q] untouched). */
int pqp_offsets_to_points_device(pqp_handle* h, int batch, int m_spline, int m, const double* spline, const double* spline_ext, const double* at_s,
                                 const double* l, const int32_t* m_of, double* x, double* y, double* s);
int pqp_offsets_to_points(pqp_handle* h, int batch, int m_spline, int m, const double* spline, const double* spline_ext, const double* at_s,
                          const double* l, const int32_t* m_of, double* x, double* y, double* s);

/* ---- length of the reference line up to the target state ----------------------------------------------------------------------
 * PathOptimizer::setReferencePathLength  src/path_optimizer.cpp:87-104 (called in processReferencePath, :117, before
 * buildReferenceFromSpline): when the target state lies behind the end of the line - x <= 0 in the frame of the line's end state,
 * global2Local tools.cpp:57-64 - the line is cut at the target's projection (getProjection tools.cpp:66-126).
 * length [batch] = ReferencePath::getLength(), target [batch][3] = x, y, heading  ->  length_out [batch], the max_s of
 * pqp_reference_states. */
int pqp_reference_length_device(pqp_handle* h, int batch, int m, const double* spline, const double* spline_ext, const double* length,
                                const double* target, double* length_out);
int pqp_reference_length(pqp_handle* h, int batch, int m, const double* spline, const double* spline_ext, const double* length,
                         const double* target, double* length_out);

/* ---- input points -> dense raw reference line ----------------------------------------------------------------------------------
 * ReferencePathSmoother::bSpline  src/reference_path_smoother/reference_path_smoother.cpp:490-521 (first step of
 * ReferencePathSmoother::solve, :31-45): the input points are the control points of a clamped B-spline of degree 3 / 4 / 5 (average
 * point spacing > 10 m / > 5 m / else), sampled at t = 0, 1/length, 2/length, ... while t < 1 and at t = 1 (about one point per
 * metre); s = accumulated chord length.  The spline itself is the third-party tinyspline (not in the reference tree): its clamped
 * knot vector and de Boor evaluation are restated, see oracle/corridor_oracle.py.
 * points [batch][p_max][2], n_points [batch] (fewer than 4: count = 0, the reference's "Few reference points"; no more points than the
 * degree: count = 0 as well, tinyspline refuses such a spline and the reference throws)
 *   ->  x, y, s [batch][n_max] = x_list_, y_list_, s_list_;  count [batch] = points the loop produces (when it exceeds n_max only
 * n_max were written).  pqp_spline_fit of (s, x, y) then gives the splines pqp_segment_raw_reference samples. */
int pqp_bspline_resample_device(pqp_handle* h, int batch, int p_max, int n_max, const double* points, const int32_t* n_points, double* x,
                                double* y, double* s, int32_t* count);
int pqp_bspline_resample(pqp_handle* h, int batch, int p_max, int n_max, const double* points, const int32_t* n_points, double* x, double* y,
                         double* s, int32_t* count);

/* ---- raw reference line -> the input lists of the smoother QPs ---------------------------------------------------------------
 * ReferencePathSmoother::segmentRawReference  src/reference_path_smoother/reference_path_smoother.cpp:48-85 (called by
 * TensionSmoother::smooth, tension_smoother.cpp:21-26): the splines of the raw point list (pqp_spline_fit of s_list_, x_list_,
 * y_list_) sampled at 0, delta_s, 2 delta_s, ... up to AND INCLUDING the first abscissa >= max_s (the reference's loop, :64-67, with
 * delta_s = 1.0: the last sample lies beyond the line and is extrapolated), angle = atan2(dy, dx), k = (dx ddy - dy ddx) / pow(dx^2 + dy^2, 1.5).
 * x, y, s, angle, k [batch][n_max] are exactly pqp_smooth_tension2 / pqp_smooth_tension's inputs; count [batch] = samples the
 * loop produces (when it exceeds n_max only n_max were written). */
int pqp_segment_raw_reference_device(pqp_handle* h, int batch, int n_max, int m, const double* spline, const double* spline_ext,
                                     const double* max_s, double delta_s, double* x, double* y, double* s, double* angle, double* k,
                                     int32_t* count);
int pqp_segment_raw_reference(pqp_handle* h, int batch, int n_max, int m, const double* spline, const double* spline_ext, const double* max_s,
                              double delta_s, double* x, double* y, double* s, double* angle, double* k, int32_t* count);

/* ---- natural cubic spline through the knots ----------------------------------------------------------
 * tk::spline::set_points  src/tools/spline.cpp:161-249 (behaviour: the natural cubic spline, f'' = 0 at both ends, linear continuation beyond
 * them), as called on the smoothed reference line
 * (tension_smoother.cpp:36-38, reference_path_smoother.cpp:58-59,574-576, reference_path_impl.cpp:349-350).
 * s, x, y [batch][m] (s strictly increasing, m >= 3)  ->  spline [batch][9][m], spline_ext [batch][4] in the layout
 * pqp_reference_states / pqp_corridor_bounds take.  The kernel solves the textbook moment equations by a Thomas recurrence of its own (not
 * the reference's band-matrix LU): the coefficients agree with the reference's to round-off (< 1e-13 of a row's largest, tested against the
 * reference's compiled tk::spline); knots and values are copied. */
int pqp_spline_fit_device(pqp_handle* h, int batch, int m, const double* s, const double* x, const double* y, double* spline,
                          double* spline_ext);
int pqp_spline_fit(pqp_handle* h, int batch, int m, const double* s, const double* x, const double* y, double* spline, double* spline_ext);

/* ---- layered DP corridor search --------------------------------------------------------------------
 * ReferencePathSmoother::graphSearchDp  src/reference_path_smoother/reference_path_smoother.cpp:142-295 (+ calculateCostAt :107-140),
 * between the smoother QP and the postSmooth QP: its outputs layers_s / lb / ub / vehicle_l are the inputs of pqp_post_smooth. */
typedef struct pqp_dp_params {
    double lateral_range;            /* 10.0  FLAGS_search_lateral_range        planning_flags.cpp:38 */
    double longitudinal_spacing;     /* 1.5   FLAGS_search_longitudial_spacing  :40 */
    double lateral_spacing;          /* 0.6   FLAGS_search_lateral_spacing      :42 */
    double car_width;                /* 2.0   :10  (search_threshold = car_width / 2 + 0.2) */
} pqp_dp_params;
void pqp_dp_default_params(pqp_dp_params* p);
/* spline, spline_ext, dist, map_of, geom as for pqp_corridor_bounds; length [batch] = reference->getLength(); start [batch][3] = vehicle
 * start state x, y, heading.  layers_s, lb, ub [batch][max_layers]; count [batch] = layers of the corridor (0: graphSearchDp returns
 * false or no node of the first layer is reachable; -1: the line needs more than max_layers layers); vehicle_l [batch]. */
int pqp_dp_corridor_device(pqp_handle* h, int batch, int m, int max_layers, const double* spline, const double* spline_ext,
                           const double* length, const double* start, const float* dist, const int32_t* map_of,
                           const pqp_grid_geometry* geom, const pqp_dp_params* prm, double* layers_s, double* lb, double* ub,
                           int32_t* count, double* vehicle_l);
int pqp_dp_corridor(pqp_handle* h, int batch, int m, int max_layers, const double* spline, const double* spline_ext, const double* length,
                    const double* start, const float* dist, int n_maps, const int32_t* map_of, const pqp_grid_geometry* geom,
                    const pqp_dp_params* prm, double* layers_s, double* lb, double* ub, int32_t* count, double* vehicle_l);

/* ---- the whole of PathOptimizer::solve as one device-resident call -----------------------------------------------------------------
 * PathOptimizer::solve  src/path_optimizer.cpp:34-71  =  ReferencePathSmoother::solve (reference_path_smoother.cpp:31-45: bSpline,
 * TensionSmoother2 QP, graphSearchDp, postSmooth QP) + processReferencePath (:106-122) + optimizePath (:124-161), for a batch of
 * scenarios that differ in every count (input points, raw-line points, smoother samples, DP layers, waypoints).  All pointers are DEVICE
 * pointers; nothing is copied to the host between the steps; the call returns when everything is enqueued (pqp_sync(h) waits).
 *   h  : the handle whose parameters the path QP uses (pqp_production_params or the reference's pqp_default_params);
 *   hs : the handle the two smoother QPs run on - the reference solves them at OSQP's default eps 1e-3 (tension_smoother_2.cpp:32-36),
 *        i.e. pqp_default_params with eps_abs = eps_rel = 1e-3 - or NULL: h's own parameters.  The two handles must live on the same device (PQP_ERR_INVALID otherwise); they are ordered by events of the chain's own (pqp_mark's slots stay the caller's).
 *   points [batch][p_max][2], n_points [batch]  PathOptimizer::solve's reference_points (fewer than 4, zero and negative counts included:
 *                                               "Few reference points", PQP_CHAIN_FEW_POINTS; so is every other count no raw line can be
 *                                               built from, see pqp_chain_stage)
 *   start, target [batch][3]                   x, y, heading of the vehicle's start and target state (the PathOptimizer constructor)
 *   start_k [batch] or NULL                     curvature of the start state (NULL: 0, State's default)
 *   dist / map_of / geom                        the obstacle distance layer(s), as for pqp_corridor_bounds
 *   out [batch][n_max][7], n_out [batch]        the path (the SlState fields getOptimizedPath fills) and its waypoint count
 *   status [batch]                              pqp_status of the path QP (PQP_STATUS_UNSOLVED when the scenario never got there)
 *   stage [batch] or NULL                       where a scenario stopped: the reference's `return false` sites
 *   iters [batch] or NULL                       ADMM iterations of the path QP
 * A scenario stops at the first of the stages below that applies to it, in the order of the steps; the others of its batch are not touched
 * by it.  A stopped scenario has n_out = 0 and status = PQP_STATUS_UNSOLVED (at PQP_CHAIN_PATH_QP_FAILED: the path QP's status).  Its
 * rows out[b] and its iters[b] are unspecified: the launches behind the stop still run for it, on counts clamped into the capacities,
 * and may write any of out[b]'s n_max rows (never anything outside out[b]); a caller reads out[b] up to n_out[b] only.
 * Which inputs end at PQP_CHAIN_FEW_POINTS - every scenario no raw line can be built from, whatever an earlier call left in the handle:
 *   n_points below 4 (the reference's test), n_points above p_max (points[b] holds no such polygon; it is not read), and n_points of
 *   4 or 5 on a polygon whose mean spacing does not ask for a B-spline of a degree below n_points (at most 5 m: degree 5; at most 10 m:
 *   degree 4, so 4 points need more than 10 m) - tinyspline refuses such a spline and the reference throws (pqp_bspline_resample: count 0).
 * A line too short for the smoother QP - fewer than 3 of the 1 m samples (TENSION: 4), i.e. a raw line of less than a metre (two) - ends
 * at PQP_CHAIN_CAPACITY, as a line with more samples than sample_max does: the count does not fit what the step can take. */
typedef enum pqp_chain_stage {
    PQP_CHAIN_OK = 0,
    PQP_CHAIN_FEW_POINTS = 1,            /* reference_path_smoother.cpp:33-36 */
    PQP_CHAIN_SMOOTHER_FAILED = 2,       /* tension_smoother.cpp:32-35 */
    PQP_CHAIN_SEARCH_FAILED = 3,         /* graphSearchDp returned false (:164-167, no reachable node) */
    PQP_CHAIN_SHORT_REFERENCE = 4,       /* postSmooth: fewer than 4 layers (:528-531) */
    PQP_CHAIN_POST_SMOOTH_FAILED = 5,    /* :555-558 */
    PQP_CHAIN_HEADING = 6,               /* initial heading error above 75 degrees (path_optimizer.cpp:113-116) */
    PQP_CHAIN_BLOCKED = 7,               /* the road is blocked before the second waypoint */
    PQP_CHAIN_PATH_QP_FAILED = 8,        /* "Solving failed!" (path_optimizer.cpp:143-156); status says why */
    PQP_CHAIN_CAPACITY = 9               /* a line needs more points / samples / layers / waypoints than pqp_chain_config allows */
} pqp_chain_stage;
typedef enum pqp_smoothing_method { PQP_SMOOTHING_TENSION2 = 0, PQP_SMOOTHING_TENSION = 1 } pqp_smoothing_method;
/* what follows the first path QP (pqp_chain_config.second_pass)
 *   RELINEARISE       PathOptimizer::optimizePath as it stands (path_optimizer.cpp:141-156): BaseSolver::solve, then
 *                     updateProblemFormulationAndSolve around its result - one pqp_path_solve with passes = 1
 *   BOUNDS_ON_STATES  the lines commented out there (:147-151): BaseSolver::solve (passes = 0); a scenario whose solve is not SOLVED stops
 *                     at PQP_CHAIN_PATH_QP_FAILED ("Pre solving failed!"); the others get pqp_corridor_bounds_on_states on that path
 *                     (n_of = its waypoint count) and a second cold solve (passes = 0) around it (lin = its l, d_heading, k) on the new
 *                     bounds.  The post_solver's waypoint count is left undefined by the commented reference (it keeps the first count
 *                     after the bounds were cut): here it is the new n_valid, which is also n_out; below 2 the stage is PQP_CHAIN_BLOCKED.
 *                     isBlocked() holds when either bounds pass was blocked (blocked_bound_ is never reset, reference_path_impl.cpp:167,222).
 *                     iters counts both solves.  Refused (PQP_ERR_INVALID, nothing enqueued) on a path handle with
 *                     rough_constraints_far_away: the reference's post_solver would see s = 0 on every input state (getOptimizedPath never
 *                     sets s, base_solver.cpp:266-289), so its precise-planning count would differ from the one computed here. */
typedef enum pqp_second_pass { PQP_SECOND_PASS_RELINEARISE = 0, PQP_SECOND_PASS_BOUNDS_ON_STATES = 1 } pqp_second_pass;
typedef struct pqp_chain_config {
    int32_t raw_max, sample_max, layer_max, n_max;   /* capacities per scenario: raw-line points (bSpline, about one per metre), 1 m samples of
                                                        the smoother QP, DP layers (1.5 m), waypoints of the path.  No upper bounds (the reference
                                                        has none).  A line whose spline table does not fit the LDS staging of the line steps
                                                        (about 880 m of smoothed line: the DP search) is refused there with
                                                        PQP_ERR_CAPACITY unless the path handle has PQP_OPT_LONG_LINES */
    double output_spacing;               /* 0.3   FLAGS_output_spacing, planning_flags.cpp:106 */
    int32_t dynamic_segmentation;        /* 1     FLAGS_enable_dynamic_segmentation, :110 */
    double max_steering_angle;           /* 35 degrees, :22 */
    double smoothed_length_margin;       /* 3.0   tension_smoother.cpp:40: the smoothed line is declared 3 m longer than its last point */
    pqp_corridor_params corridor;
    pqp_dp_params dp;
    int32_t smoothing_method;            /* PQP_SMOOTHING_TENSION2  FLAGS_smoothing_method, planning_flags.cpp:27 (ReferencePathSmoother::create,
                                            reference_path_smoother.cpp:18-29).  TENSION: the clearance of the raw line's samples is looked up on
                                            the device (tension_smoother.cpp:168); on a smoother handle without polish = 1 (the reference's ADMM on the 3n-variable
                                            formulation) sample_max is bounded by what one CU's LDS holds (about 190) */
    int32_t second_pass;                 /* PQP_SECOND_PASS_RELINEARISE (pqp_second_pass) */
} pqp_chain_config;
void pqp_chain_default_config(pqp_chain_config* c);
int pqp_optimize_path_device(pqp_handle* h, pqp_handle* hs, const pqp_chain_config* cfg, int batch, int p_max, const double* points,
                             const int32_t* n_points, const double* start, const double* target, const float* dist, const int32_t* map_of,
                             const pqp_grid_geometry* geom, const double* start_k, double* out, int32_t* n_out, int32_t* status, int32_t* stage,
                             int32_t* iters);
/* Map::getObstacleDistance (src/tools/Map.cpp:16-22) at the points x_list, y_list [batch][n]: the `clearance` input of pqp_smooth_tension
 * (tension_smoother.cpp:168), gathered on the device from the same distance layer(s) pqp_corridor_bounds takes */
int pqp_clearance_device(pqp_handle* h, int batch, int n, const double* x_list, const double* y_list, const float* dist, const int32_t* map_of,
                         const pqp_grid_geometry* geom, double* clearance);
/* the steps of the chain that share one size per launch elsewhere, with a count per scenario (device pointers): a scenario with
 * fewer points is the same QP padded with decoupled dummies (same optimum); the spline table is padded with knots far beyond the line,
 * whose cubic coefficient is zero - term by term tk::spline's right-hand extrapolation */
int pqp_smooth_tension2_var_device(pqp_handle* h, int batch, int n_max, const int32_t* n_of, const double* x_list, const double* y_list,
                                   const double* angle_list, const double* k_list, const double* s_list, double* out_x, double* out_y,
                                   double* out_s, int32_t* status, int32_t* iters, double* info);
/* TensionSmoother::osqpSmooth (tension_smoother.cpp:49-100) with a point count per scenario (at least 4); clearance as for pqp_smooth_tension */
int pqp_smooth_tension_var_device(pqp_handle* h, int batch, int n_max, const int32_t* n_of, const double* x_list, const double* y_list,
                                  const double* angle_list, const double* clearance, double* out_x, double* out_y, double* out_s, int32_t* status,
                                  int32_t* iters, double* info);
int pqp_post_smooth_var_device(pqp_handle* h, int batch, int m_max, const int32_t* m_of, const double* layers_s, const double* lb, const double* ub,
                               const double* vehicle_l, double* out_l, int32_t* status, int32_t* iters, double* info);
int pqp_spline_fit_var_device(pqp_handle* h, int batch, int m_max, const int32_t* m_of, const double* s, const double* x, const double* y,
                              double* spline, double* spline_ext);

/* ---- vehicle footprints of planned states against the distance layer ----------------------------------------------------------------
 * CollisionChecker (src/tools/collision_checker.cpp:9-58) with CarGeometry's six-circle footprint (src/tools/car_geometry.cpp:38-72) and
 * local2Global (src/tools/tools.cpp:50-55), for many states of many scenarios per call.  PathOptimizer builds such a checker from its map
 * (path_optimizer.cpp:29); the path QP's collision rows are soft, so a SOLVED path may still put a corner of the car into an obstacle. */
typedef struct pqp_car_geometry {        /* CollisionChecker ctor (collision_checker.cpp:9-14): car_(car_width, fabs(rear_length), front_length) */
    double width;                        /* 2.0   FLAGS_car_width     planning_flags.cpp:10 */
    double rear_length;                  /* -1.0  FLAGS_rear_length   planning_flags.cpp:18 (the flag's sign; the checker takes fabs) */
    double front_length;                 /* 3.9   FLAGS_front_length  planning_flags.cpp:20 */
} pqp_car_geometry;
typedef enum pqp_footprint_mode {
    PQP_FOOTPRINT_CIRCLES = 0,           /* isSingleStateCollisionFree          collision_checker.cpp:17-39: the six circles */
    PQP_FOOTPRINT_BOUNDING_FIRST = 1     /* isSingleStateCollisionFreeImproved  collision_checker.cpp:41-58: the bounding circle, the six when it is not clear */
} pqp_footprint_mode;
void pqp_car_default_geometry(pqp_car_geometry* c);
/* Pure host: CarGeometry::setCircles (car_geometry.cpp:38-57) in the vehicle frame, in the reference's expression order.
 * circles [7][3] = x, y, r of rr, rl, fr, fl, fm, rm (getCircles' order), then the bounding circle (getBoundingCircle).
 * PQP_ERR_INVALID: a null pointer or a geometry that is not finite. */
int pqp_car_circles(const pqp_car_geometry* c, double* circles);
/* states [batch][n][stride]  x, y, heading at offsets 0, 1, 2 (stride = PQP_OUT_STRIDE reads pqp_optimize_path_device's `out` in place)
 * n_of [batch] or NULL       states of each scenario (<= n), e.g. the chain's n_out; NULL: all have n
 * dist / map_of / geom       the distance layer(s), as for pqp_corridor_bounds; pqp_footprint_check takes n_maps after dist, as it does
 * car, mode                  the footprint and pqp_footprint_mode
 * free_out [batch][n]        1 when the state is collision-free in `mode`, else 0; a circle whose centre is outside the map is a collision
 *                            (:32-35, :56-57), so is a state that is not finite; 0 at index n_of[b] and beyond
 * first_collision [batch]    the first colliding index below n_of[b], n_of[b] when there is none (the convention of n_valid)
 * margin [batch][n] or NULL  min over the six circles of Map::getObstacleDistance(centre) - r (Map.cpp:16-22: 0 outside the map), whatever
 *                            the mode; 0 at index n_of[b] and beyond
 * In BOUNDING_FIRST mode a state can be free where CIRCLES says collision (the corner circles poke out of the bounding circle and the
 * layer is interpolated): each mode gives the reference's own answer.
 * The _device form takes device pointers and is asynchronous on the handle's stream (enqueue it right behind pqp_optimize_path_device);
 * it checks null pointers and sizes only.  The host form copies in, runs, copies out and synchronises; PQP_ERR_INVALID, with nothing
 * launched, also for a map_of value outside [0, n_maps), stride < 3, a car geometry that is not finite or a bad mode. */
int pqp_footprint_check_device(pqp_handle* h, int batch, int n, int stride, const double* states, const int32_t* n_of, const float* dist,
                               const int32_t* map_of, const pqp_grid_geometry* geom, const pqp_car_geometry* car, int mode, uint8_t* free_out,
                               int32_t* first_collision, double* margin);
int pqp_footprint_check(pqp_handle* h, int batch, int n, int stride, const double* states, const int32_t* n_of, const float* dist, int n_maps,
                        const int32_t* map_of, const pqp_grid_geometry* geom, const pqp_car_geometry* car, int mode, uint8_t* free_out,
                        int32_t* first_collision, double* margin);

/* ---- scores of candidate paths and each group's best ------------------------------------------------------------------------------
 * A planner launches many candidates per vehicle and drives one of them.  Behind pqp_optimize_path_device and pqp_footprint_check_device,
 * on the same stream, this scores every candidate and leaves the winner of every group - its index and its waypoints - so that only the
 * winners cross to the host.  The reference plans one path per call and has no counterpart; with the default weights the score is twice
 * the path QP's own objective without its slack terms (OSQP minimises 1/2 x'Px, P's diagonal 20 on k and 100 on dk,
 * base_solver.cpp:123-147), so "best" means what the solver means.  A group lives on one GPU. */
#define PQP_SCORE_STRIDE 8
typedef struct pqp_select_params {
    double weight_kappa;      /* 20   the path QP's own weight on k      (base_solver.cpp:124, pqp_params.weight_kappa)  */
    double weight_dkappa;     /* 100  on dk                              (base_solver.cpp:125) */
    double weight_offset;     /* 0    on l                               (base_solver.cpp:123: weight_l is 0) */
    double weight_length;     /* 0    on the path's length in metres */
    double weight_clearance;  /* 0    on sum_i max(0, clearance_want - margin_i)^2 */
    double clearance_want;    /* 0.6  FLAGS_expected_safety_margin, planning_flags.cpp:95 */
    int32_t per_waypoint;     /* 0    1: the three sums over waypoints and the clearance sum are divided by the path's count */
    int32_t require_free;     /* 1    with first_collision given, a path that collides cannot win */
} pqp_select_params;
void pqp_select_default_params(pqp_select_params* p);          /* pure host */
/* Inputs (device pointers for the _device form, host pointers for the other); every one marked "or NULL" is optional:
 *   paths [batch][n][stride]          stride >= 7, columns as PQP_OUT_STRIDE documents: x, y, heading, l, d_heading, k, dk;
 *                                     stride = PQP_OUT_STRIDE reads pqp_optimize_path_device's `out` where it is
 *   n_of [batch] or NULL              waypoints of each candidate, e.g. the chain's n_out, clamped to [0, n]; NULL: all have n.
 *                                     "count" below is this clamped value
 *   status, stage [batch] or NULL     what the chain wrote (pqp_status, pqp_chain_stage)
 *   first_collision [batch] or NULL   what the footprint check wrote
 *   margin [batch][n] or NULL         what the footprint check wrote
 *   group_start [groups + 1]          the candidates of group g are the rows group_start[g] .. group_start[g + 1] - 1: ascending, the first 0,
 *                                     the last `batch`; empty groups are allowed
 * A candidate is eligible when all of these hold: its count is at least 2; status is absent or PQP_STATUS_SOLVED; stage is absent or
 * PQP_CHAIN_OK; first_collision is absent, or require_free is 0, or first_collision[b] equals its count; its score is finite.
 * Outputs, fully overwritten:
 *   terms [batch][PQP_SCORE_STRIDE]   0 score, 1 sum k_i^2, 2 sum_{i < count - 1} dk_i^2, 3 sum l_i^2,
 *                                     4 length sum_{i < count - 1} sqrt(dx^2 + dy^2) of the chords between successive waypoints,
 *                                     5 the least margin over the path (0 when margin is NULL; NaN when one of them is NaN),
 *                                     6 the clearance sum sum_i max(0, clearance_want - margin_i)^2 (0 when margin is NULL),
 *                                     7 eligible as 1.0 / 0.0.  Sums without a range run over i < count.  Entries 1, 2, 3 and 6 are stored
 *                                     after the per_waypoint division, and
 *                                     score = weight_kappa t1 + weight_dkappa t2 + weight_offset t3 + weight_length t4 + weight_clearance t6.
 *                                     A candidate that is not eligible still gets its terms; one with a count below 2 gets eight zeros.
 *                                     The order of a candidate's additions depends on its count alone: the same candidate gives the same
 *                                     bits in any batch, at any position, in any group.
 *   best [groups]                     the row of the group's eligible candidate with the least score, the lowest row among equal scores;
 *                                     -1 when the group has none
 *   best_paths [groups][n][7], best_n [groups]   both or neither (NULL): the winner's seven columns and its count, zeros beyond the
 *                                     count; a group without a winner is all zeros with best_n 0
 * The _device form is asynchronous on the handle's stream (two launches: the scores, then the groups) and checks null pointers and sizes
 * only; with groups = 0 it scores the candidates and launches nothing else.  It cannot see group_start, so the kernel clamps every
 * group boundary to [0, batch] and takes a descending pair for an empty group: no array makes it read outside `paths`.  What a damaged
 * array yields follows from that rule alone: a group that starts at a value above batch, and the group of a descending pair, are empty
 * (best -1, zeros); a group that ends at a value above batch runs to the last row; a negative boundary counts as 0; every other group
 * is what its own two boundaries say.
 * The host form copies in, runs, copies out and synchronises; PQP_ERR_INVALID, with nothing launched and the outputs untouched, for
 * stride < 7, groups < 0, a group_start that is not ascending from 0 to batch (so, batch being at least 1, it needs one group or more),
 * a parameter that is not finite, or best_paths without best_n or the reverse. */
int pqp_select_paths_device(pqp_handle* h, const pqp_select_params* prm, int batch, int n, int stride, const double* paths, const int32_t* n_of,
                            const int32_t* status, const int32_t* stage, const int32_t* first_collision, const double* margin, int groups,
                            const int32_t* group_start, double* terms, int32_t* best, double* best_paths, int32_t* best_n);
int pqp_select_paths(pqp_handle* h, const pqp_select_params* prm, int batch, int n, int stride, const double* paths, const int32_t* n_of,
                     const int32_t* status, const int32_t* stage, const int32_t* first_collision, const double* margin, int groups,
                     const int32_t* group_start, double* terms, int32_t* best, double* best_paths, int32_t* best_n);

/* ---- points onto their reference line: Cartesian to Frenet -------------------------------------------------------------------------
 * Where does a point sit relative to a line?  The reference answers with getProjection / getProjectionByNewton (src/tools/tools.cpp:66-126)
 * and takes the signed offset from global2Local(projection, point).y (tools.cpp:57-64), as in processInitState (path_optimizer.cpp:73-85)
 * and graphSearchDp (reference_path_smoother.cpp:148-165).  This does it for many points per line in one launch - obstacle corners, agents,
 * goal candidates, last cycle's waypoints - and is the inverse of pqp_offsets_to_points.
 * Inputs:
 *   spline [batch][9][m], spline_ext [batch][4], length [batch]   as for pqp_reference_length: the tables pqp_spline_fit writes
 *   points [batch][q_max][stride]     x, y at offsets 0, 1 (stride >= 2); with has_heading a heading at offset 2 (stride >= 3):
 *                                     stride = PQP_OUT_STRIDE then reads a path solve's or the chain's `out` in place
 *   q_of [batch] or NULL              the points of each line, clamped to [0, q_max]; NULL: all have q_max
 * Outputs, fully overwritten: proj [batch][q_max][PQP_PROJ_STRIDE] and flags [batch][q_max]; rows beyond a line's count are eight zeros
 * with flag 0.  A row:
 *   0 s          exactly getProjection(xs, ys, x, y, length, 0.0).s: the scan at 0, 1, 2, ... <= length, the first strict minimum wins, the end
 *                point takes over only when it is strictly closer, Newton from min(best, length) with at most 20 steps until |ds| < 1e-5,
 *                then min(cur, length).  As in the reference s is NOT clamped at 0 (tk::spline extrapolates to the left,
 *                spline.cpp:251-272): PQP_PROJ_BEFORE_START says when s < 0.  Bit for bit what pqp_reference_length returns for a target
 *                behind the line's end.
 *                One consequence of the end-point rule to know: on a line whose length is no integer the end sample lies less than a metre
 *                behind the last grid sample, and a point nearer to it than to every grid sample - roughly, a point that belongs to the
 *                line's last metre - is handed to the end without a Newton step: s = length, PQP_PROJ_AT_END, and t says how far before
 *                the end the point lies.  To project a path onto the line through its own points, let `length` run a metre or two past
 *                the last knot (the spline extrapolates to the right as well, spline.cpp:262-266).
 *   1 l, 2 t     global2Local((x_p, y_p, heading_p), point).y and .x: l is positive to the left, the sign of vehicle_l and of
 *                initial_offset; t is the distance along the tangent, non-zero only where the projection was clipped (or not converged)
 *   3 d_heading  constrainAngle(point.heading - heading_p) as path_optimizer.cpp:83, or 0 without has_heading
 *   4 x_p, 5 y_p, 6 heading_p   the line's state at s, heading_p = getHeading (tools.cpp:32-36)
 *   7 k_p        getCurvature at s (tools.cpp:38-44)
 * flags: PQP_PROJ_AT_END s == length; PQP_PROJ_BEFORE_START s < 0; PQP_PROJ_NOT_CONVERGED the 20th Newton step was still >= 1e-5 (the
 * row is still the reference's); PQP_PROJ_NOT_FINITE see below.
 * Edge cases:
 *   length <= 0 or NaN     s = 0 and the other columns from the line's state at 0.  The reference returns a bare State{xs(0), ys(0)} there,
 *                          without a heading (tools.cpp:72-74); filling the row from the line is this library's choice.
 *   a point (x, y, or the heading that is read) or a Newton iterate that is not finite: eight NaNs and PQP_PROJ_NOT_FINITE alone; its
 *                          neighbours are untouched.  So is every point of a line whose length is infinite or 2^20 m (1049 km) and more:
 *                          the scan's floor(length) + 1 steps would not end, or would hold the GPU for a long time.
 * The _device form is asynchronous on the handle's stream (one launch), allocates nothing and checks null pointers and sizes only; it has
 * no knot-count cap and needs neither PQP_OPT_LONG_LINES nor a workspace: the kernel reads the table where it lies.  The host form copies
 * in, runs, copies out and synchronises.  PQP_ERR_INVALID, with nothing launched and the outputs untouched: a null pointer (q_of apart),
 * batch < 1, m < 2, q_max < 1 or q_max > 256 * 65535, stride < 2, or stride < 3 with has_heading. */
#define PQP_PROJ_STRIDE 8
#define PQP_PROJECT_TILE_SAMPLES 1024      /* coarse samples the kernel holds in LDS at a time (16 bytes each, and the end sample behind them) */
enum { PQP_PROJ_AT_END = 1, PQP_PROJ_BEFORE_START = 2, PQP_PROJ_NOT_CONVERGED = 4, PQP_PROJ_NOT_FINITE = 8 };
int pqp_project_points_device(pqp_handle* h, int batch, int m, const double* spline, const double* spline_ext, const double* length,
                              int q_max, int stride, int has_heading, const double* points, const int32_t* q_of, double* proj, int32_t* flags);
int pqp_project_points(pqp_handle* h, int batch, int m, const double* spline, const double* spline_ext, const double* length, int q_max,
                       int stride, int has_heading, const double* points, const int32_t* q_of, double* proj, int32_t* flags);

/* ---- planned paths to trajectories: arc length, speed, acceleration, time --------------------------------------------------------------
 * The reference's State carries s, v and a (include/data_struct/data_struct.hpp:14-26) and nothing fills them; getOptimizedPath adds the
 * chords of the path up in tmp_s and drops the sum (src/solver/base_solver.cpp:268,282-284).  A controller, a simulator or a scorer by
 * travel time needs each path as a trajectory: this gives every waypoint its arc length along the path itself, a speed that respects the
 * path's curvature and the car's acceleration limits, and a time stamp - behind the chain, the footprint check and the selection on the
 * same stream, reading `out` or `best_paths` where they lie.  The reference has no counterpart and no such flags: the defaults below are
 * this library's choice. */
#define PQP_SPEED_STRIDE 4
typedef struct pqp_speed_params {
    double v_max;             /* 10.0  m/s, finite, >= 0: the cap on every waypoint */
    double a_max;             /* 1.5   m/s^2, finite, > 0: the largest acceleration */
    double d_max;             /* 3.0   m/s^2, finite, > 0: the largest braking, as a positive number */
    double a_lat_max;         /* 2.0   m/s^2, > 0, +inf allowed: v^2 |k| stays below it */
} pqp_speed_params;
void pqp_speed_default_params(pqp_speed_params* p);            /* pure host */
enum { PQP_SPEED_START_TOO_FAST = 1, PQP_SPEED_STOPS_EARLY = 2, PQP_SPEED_NEVER_ARRIVES = 4, PQP_SPEED_EMPTY = 8, PQP_SPEED_NOT_FINITE = 16 };
/* Inputs (device pointers for the _device form, host pointers for the other); every one marked "or NULL" is optional:
 *   paths [batch][n][stride]          x, y at offsets 0, 1 and k at offset 5, stride >= 6; stride = PQP_OUT_STRIDE reads a path solve's or the
 *                                     chain's `out`, or pqp_select_paths' best_paths, in place
 *   n_of [batch] or NULL              waypoints of each path, clamped to [0, n]; NULL: all have n.  "count" below is this clamped value
 *   stop_before [batch] or NULL       e.g. the footprint check's first_collision: states at index >= stop_before[b] are not driven.  The
 *                                     driven count is c = min(count, max(stop_before[b], 0)); when c < count the profile ends at speed 0 at
 *                                     index c - 1 and PQP_SPEED_STOPS_EARLY is set
 *   v_limit [batch][n] or NULL        a speed cap per waypoint (m/s, >= 0, +inf allowed)
 *   v_start [batch]                   the vehicle's speed at waypoint 0, finite and >= 0
 *   v_end [batch] or NULL             the speed demanded at the last driven waypoint, finite and >= 0; NaN (or NULL): free.  Not read for a
 *                                     path that stops early
 *   prm                               pqp_speed_params
 * Outputs, fully overwritten: profile [batch][n][PQP_SPEED_STRIDE] = s, v, a, t and flags [batch]; rows at index >= c are zeros.
 * The definition, in fp64, for a path with driven count c:
 *   s   d_i = sqrt(dx^2 + dy^2) between waypoints i and i + 1; s_0 = 0, s_{i+1} = s_i + d_i - the chords, as pqp_select_paths' term 4 and
 *       the reference's tmp_s
 *   v   caps in v^2: cap_i = min(v_max^2, v_limit_i^2, a_lat_max / |k_i|) (a zero curvature gives no cap), then cap_0 = min(cap_0, v_start^2),
 *       cap_{c-1} = min(cap_{c-1}, v_end^2) when v_end is a number, cap_{c-1} = 0 when the path stops early.  w is the largest sequence with
 *       w_i <= cap_i, w_{i+1} <= w_i + 2 a_max d_i and w_i <= w_{i+1} + 2 d_max d_i - the textbook forward pass then backward pass - and
 *       v_i = sqrt(w_i).  In closed form
 *         w_i = min( cap_i, min_{j < i} (cap_j + 2 a_max (s_i - s_j)), min_{j > i} (cap_j + 2 d_max (s_j - s_i)) )
 *       which is what the kernel evaluates, by scans
 *   a   a_i = (w_{i+1} - w_i) / (2 d_i) for i < c - 1, 0 where d_i = 0, and a_{c-1} = 0
 *   t   t_0 = 0, t_{i+1} = t_i + 2 d_i / (v_i + v_{i+1}); the step is 0 where d_i = 0, and +inf, with PQP_SPEED_NEVER_ARRIVES, where both
 *       speeds are 0 and d_i > 0
 *   c = 1 gives the one row (0, sqrt(cap_0), 0, 0).
 * flags:
 *   PQP_SPEED_START_TOO_FAST   w_0 < v_start^2: the caps or the braking limit do not allow the start speed; the row is still the definition's
 *   PQP_SPEED_STOPS_EARLY      c < count
 *   PQP_SPEED_NEVER_ARRIVES    see t
 *   PQP_SPEED_EMPTY            c = 0: all zeros (together with PQP_SPEED_STOPS_EARLY when count > 0)
 *   PQP_SPEED_NOT_FINITE       a value that is read for the driven range is not what it must be: an x, y or k below index c that is not
 *                              finite, a v_limit below index c that is NaN or negative, a v_start that is not finite or negative, a v_end
 *                              (of a path that does not stop early) that is infinite or negative, or an arc length that overflows.  The
 *                              path's driven rows are NaN, this flag is set alone, and neighbouring paths are untouched
 * The order of a path's additions depends on its driven count alone: the same path gives the same bits at any position in any batch, as
 * pqp_select_paths promises.  (The sums are scans, so s and t agree with a sequential sum to (c - 1) ulp, not bit for bit.)
 * The _device form is one launch, asynchronous on the handle's stream; it allocates nothing and checks pointers, sizes and prm only
 * (the arrays are the device's: what they hold is judged by the kernel, path by path).  The host form copies in, runs, copies out and
 * synchronises.  Both forms: PQP_ERR_INVALID, with nothing launched and the outputs untouched, for a null pointer that is not optional,
 * batch < 1, n < 1, stride < 6, or a parameter outside the ranges pqp_speed_params states. */
int pqp_speed_profile_device(pqp_handle* h, const pqp_speed_params* prm, int batch, int n, int stride, const double* paths, const int32_t* n_of,
                             const int32_t* stop_before, const double* v_limit, const double* v_start, const double* v_end, double* profile,
                             int32_t* flags);
int pqp_speed_profile(pqp_handle* h, const pqp_speed_params* prm, int batch, int n, int stride, const double* paths, const int32_t* n_of,
                      const int32_t* stop_before, const double* v_limit, const double* v_start, const double* v_end, double* profile,
                      int32_t* flags);

/* ---- time-stamped trajectories at a fixed time step ------------------------------------------------------------------------------------
 * pqp_speed_profile's time stamps sit where the waypoints are: every 0.15 to 1 m of arc, at times that follow from the speed.  A tracking
 * controller, a simulator step, an MPC horizon or a comparison against predicted agents asks where the car is at t0 + k dt: this samples
 * every path at those times, behind the speed profile on the same stream, reading `out` (or `best_paths`) and `profile` where they lie.
 * Inside a segment the kinematics are the profile's own - a_i = (w_{i+1} - w_i) / (2 d_i) and t_{i+1} - t_i = 2 d_i / (v_i + v_{i+1}) are
 * constant acceleration along the chord - so a sample is their closed form.  The reference has no counterpart (nothing fills State::v). */
#define PQP_TRAJ_STRIDE 8          /* x, y, heading, k, s, v, a, t */
typedef struct pqp_sample_params {
    double dt;                /* 0.1   s, finite, > 0: the time step */
    int32_t hold_last;        /* 0     1: rows behind the arrival repeat the last driven waypoint at rest */
} pqp_sample_params;
void pqp_sample_default_params(pqp_sample_params* p);          /* pure host */
enum { PQP_TRAJ_HORIZON_SHORT = 1, PQP_TRAJ_STANDS = 2, PQP_TRAJ_ENDS_MOVING = 4, PQP_TRAJ_EMPTY = 8, PQP_TRAJ_NOT_FINITE = 16 };
/* Inputs (device pointers for the _device form, host pointers for the other); every one marked "or NULL" is optional:
 *   paths [batch][n][stride]          x, y, heading at offsets 0, 1, 2 and k at offset 5, stride >= 6; stride = PQP_OUT_STRIDE reads `out` or
 *                                     best_paths in place
 *   n_of, stop_before [batch] or NULL the driven count is c = min(clamp(n_of, 0, n), max(stop_before, 0)): pqp_speed_profile's expression,
 *                                     so the same two arrays give the same c
 *   profile [batch][n][PQP_SPEED_STRIDE]   s, v, a, t as pqp_speed_profile wrote them, or any array of that shape
 *   t0 [batch] or NULL (all 0)        the time of sample 0, finite and >= 0
 *   m >= 1                            samples per path
 *   prm                               pqp_sample_params
 * Outputs, fully overwritten: traj [batch][m][PQP_TRAJ_STRIDE], m_of [batch], flags [batch].
 * The definition, in fp64, for a path with driven count c; every product and sum is rounded on its own (no contraction), in this order:
 *   tau_k = t0 + (double)k * dt
 *   T_i = max_{j <= i} t_j, the running maximum of the t column (that column is a scan's prefix sum, monotone only up to its last bit; the
 *       running maximum is exact and monotone, so a count and a binary search find the same segment)
 *   sample k is on the path when tau_k <= T_{c-1}; m_of is the number of such samples - a prefix k < m_of, because tau ascends
 *   segment  i = #{ j < c : T_j <= tau_k } - 1; with t_0 = 0 that is >= 0 (a t column that starts later puts earlier samples in segment 0)
 *   i = c - 1: the row is waypoint c - 1 itself - its x, y, heading, k, s, v, then a = 0, t = tau_k.  Otherwise
 *     (dx, dy) = (x_{i+1} - x_i, y_{i+1} - y_i);  d = sqrt(dx*dx + dy*dy), the profile's chord;  u = tau_k - t_i
 *     e = min(max((v_i + (0.5 * a_i) * u) * u, 0), d);  lambda = d > 0 ? e / d : 0
 *     x = x_i + lambda * dx;  y = y_i + lambda * dy
 *     heading = constrain_angle(h_i + lambda * constrain_angle(h_{i+1} - h_i))     (include/tools/tools.hpp:24-35's wrap to [-pi, pi])
 *     k = k_i + lambda * (k_{i+1} - k_i);  s = s_i + e;  v = max(v_i + a_i * u, 0);  a = a_i;  t = tau_k
 *     (min and max as fmin and fmax)
 *   rows k >= m_of: zeros; with hold_last the last driven waypoint's x, y, heading, k, s with v = 0, a = 0, t = tau_k
 * flags:
 *   PQP_TRAJ_HORIZON_SHORT   tau_{m-1} < T_{c-1}: the path is not finished inside the horizon (also an arrival time of +inf)
 *   PQP_TRAJ_STANDS          some on-path sample has i < c - 1 and T_{i+1} = +inf: the car never leaves waypoint i (the profile's
 *                            PQP_SPEED_NEVER_ARRIVES)
 *   PQP_TRAJ_ENDS_MOVING     m_of < m and v_{c-1} > 0: the horizon passes the end of a path that does not end at rest
 *   PQP_TRAJ_EMPTY           c = 0: zeros, m_of = 0; nothing of the path is read, t0 neither
 *   PQP_TRAJ_NOT_FINITE      a value read below index c is not what it must be: an x, y, heading, k, s, v or a that is not finite, a t
 *                            that is NaN or negative (+inf is allowed), a t0 that is not finite or negative.  All m rows are NaN,
 *                            m_of = 0, this flag is set alone, and neighbouring paths are untouched.  A path that pqp_speed_profile
 *                            flagged PQP_SPEED_NOT_FINITE has NaN rows and arrives here that way
 * A sample's bits depend on its path's driven rows, t0, dt and k alone - not on the batch, the position in it, n, m or which form was
 * called.  The _device form is one launch, asynchronous on the handle's stream; it allocates nothing and checks pointers, sizes and prm
 * only; n and m have no cap.  The host form copies in, runs, copies out and synchronises.  Both forms: PQP_ERR_INVALID, with nothing
 * launched and the outputs untouched, for a null pointer that is not optional, batch < 1, n < 1, m < 1, stride < 6, a dt that is not
 * finite and positive, or a hold_last other than 0 / 1. */
int pqp_sample_trajectory_device(pqp_handle* h, const pqp_sample_params* prm, int batch, int n, int stride, const double* paths,
                                 const int32_t* n_of, const int32_t* stop_before, const double* profile, const double* t0, int m, double* traj,
                                 int32_t* m_of, int32_t* flags);
int pqp_sample_trajectory(pqp_handle* h, const pqp_sample_params* prm, int batch, int n, int stride, const double* paths, const int32_t* n_of,
                          const int32_t* stop_before, const double* profile, const double* t0, int m, double* traj, int32_t* m_of,
                          int32_t* flags);

/* ---- sampled trajectories against predicted moving agents -------------------------------------------------------------------------------
 * pqp_footprint_check tests planned states against what stands still: the distance layer.  What moves - predicted vehicles, pedestrians -
 * comes as a pose and a size per time step, and pqp_sample_trajectory puts every candidate on those time steps.  This tests every sample of
 * every trajectory against every predicted agent of the path's scene at the same step: the six-circle footprint of pqp_car_circles against
 * a rounded oriented rectangle, and says whether a candidate hits one, when, and which.  The reference has no counterpart (it plans one
 * path against a static map); the footprint is its CarGeometry's six circles placed by local2Global (src/tools/tools.cpp:50-55). */
#define PQP_AGENT_STRIDE 6         /* x, y, heading, half_length, half_width, radius */
#define PQP_AGENT_FRAME_STRIDE 8   /* x, y, cos h, sin h, half_length, half_width, radius, reach */
/* The check has one parameter, so it travels as itself and not in a struct: margin, in m, finite and >= 0 - the distance demanded beyond
 * touching.  pqp_agents_default_params writes this library's choice of it, 0.0, to *margin (pure host; NULL ignored). */
void pqp_agents_default_params(double* margin);
/* Inputs (device pointers for the _device form, host pointers for the other); every one marked "or NULL" is optional:
 *   traj [batch][m][stride]           x, y, heading at offsets 0, 1, 2, stride >= 3; stride = PQP_TRAJ_STRIDE reads pqp_sample_trajectory's
 *                                     traj in place
 *   m_of [batch] or NULL              the samples to check: count = clamp(m_of, 0, m); NULL: all m (pass NULL with hold_last to keep
 *                                     checking the parked car)
 *   agents [n_scenes][a_max][m][PQP_AGENT_STRIDE]   an agent's pose and size at the same m time steps.  half_length < 0 or half_width < 0:
 *                                     the agent is absent at that step - tested first, the rest of the row is not read.  radius rounds the
 *                                     rectangle; a disc is half_length = half_width = 0 with a radius.  a_max = 0 is allowed (agents and
 *                                     frames may then be NULL)
 *   a_of [n_scenes] or NULL           agents per scene: A = clamp(a_of, 0, a_max); NULL: all a_max
 *   scene_of [batch] or NULL (all 0)  the agent set a path is checked against (map_of's role); the host form refuses values outside
 *                                     [0, n_scenes), the device form clamps them
 *   car                               the footprint: the six circles (c_j, r_j) of pqp_car_circles
 *   margin                            see above; by value in both forms
 *   frames [n_scenes][a_max][m][PQP_AGENT_FRAME_STRIDE]   (_device form only) a workspace of the caller's, fully written by the first launch
 * Two launches on the handle's stream.  The first turns every agent row into a frame row: x, y, half_length, half_width, radius bit for
 * bit, (sin, cos) = sincos(heading) taken once, reach = sqrt(hl*hl + hw*hw) + radius.  An absent row becomes eight zeros with reach = -1;
 * a present row with a value that is not finite or with a negative radius is "bad": eight zeros with reach = NaN.
 * The second is the test.  The definition, in fp64, every product and sum rounded on its own (no contraction), in this order, for sample
 * k < count, agent a < A and circle j < 6:
 *   (sh, ch) = sincos(h_k);  gx = cx_j*ch - cy_j*sh + x_k;  gy = cx_j*sh + cy_j*ch + y_k      (pqp_footprint_check's expression)
 *   dx = gx - ax;  dy = gy - ay;  u = dx*c + dy*s;  w = dy*c - dx*s
 *   ex = fabs(u) - hl;  ey = fabs(w) - hw;  ox = fmax(ex, 0);  oy = fmax(ey, 0)
 *   d = sqrt(ox*ox + oy*oy) + fmin(fmax(ex, ey), 0) - radius;  clear_j = d - r_j
 *   clear(k, a) = min_j clear_j;  hit(k, a) = clear(k, a) < margin     (strict: touching at exactly `margin` is no hit; min as fmin)
 * An absent agent is skipped.  A bad agent hits every checked sample of its scene's paths at that step, with clear = -inf.  A sample
 * whose x, y or heading is not finite is a hit with hit_agent = -1 and clear = -inf whatever the agents are, as pqp_footprint_check
 * takes a state that is not finite for a collision.
 * Outputs, fully overwritten:
 *   first_hit [batch]                 the first hit sample below count, count when there is none (the convention of first_collision); a
 *                                     path with count = 0 therefore reports 0, as pqp_footprint_check does
 *   hit_agent [batch]                 the lowest agent index that hits at sample first_hit; -1 when there is no hit or the hit is the ego
 *                                     sample itself
 *   clearance [batch][m] or NULL      min_a clear(k, a) for k < count, +inf where the scene has no present agent at that step, 0 at
 *                                     k >= count
 * With clearance = NULL the test skips agents whose centre is too far from the footprint's bounding centre to come within `margin`, and
 * stops behind the 64 samples that hold the first hit; neither changes an output while the squares of the coordinates are finite (beyond
 * about 1e154 the exact test's products overflow to NaN and the two forms may differ).  The results depend on the path's own rows, its scene
 * and the parameters alone - not on the batch, the position in it or which form was called; no atomics, the same answer every run.
 * The _device form is asynchronous on the handle's stream and allocates nothing; m, a_max and n_scenes are held to n_scenes * a_max * m
 * <= 2^38 rows alone.  The host form stages
 * frames itself, copies in, runs, copies out and synchronises.  Both forms: PQP_ERR_INVALID, with nothing launched and the outputs
 * untouched, for a null pointer that is not optional, batch < 1, m < 1, stride < 3, n_scenes < 1, a_max < 0, n_scenes * a_max * m > 2^38, a margin that is not finite
 * or is negative, or a car geometry that is not finite. */
int pqp_agents_check_device(pqp_handle* h, double margin, const pqp_car_geometry* car, int batch, int m, int stride,
                            const double* traj, const int32_t* m_of, int n_scenes, int a_max, const double* agents, const int32_t* a_of,
                            const int32_t* scene_of, double* frames, int32_t* first_hit, int32_t* hit_agent, double* clearance);
int pqp_agents_check(pqp_handle* h, double margin, const pqp_car_geometry* car, int batch, int m, int stride,
                     const double* traj, const int32_t* m_of, int n_scenes, int a_max, const double* agents, const int32_t* a_of,
                     const int32_t* scene_of, int32_t* first_hit, int32_t* hit_agent, double* clearance);

/* ---- speeds past predicted agents: a search in the path-time plane -------------------------------------------------------------------------
 * pqp_agents_check says that a trajectory hits a predicted agent; most such hits are conflicts of timing on a good path.  This keeps the
 * path and plans the speed: for every path it marks which cells of the path-time plane - station j at arc length j ds against layer k at
 * time k dt - the car's footprint would share with an agent (the test of pqp_agents_check, unchanged), and finds by a layered dynamic
 * program the cheapest sequence of stations over the layers that stays out of marked cells, within the acceleration and braking limits
 * and under the envelope of pqp_speed_profile's v and a.  It is the coarse yield-or-pass decision of a path-speed decoupled planner,
 * batched over the candidates, behind the speed profile on the same stream.  The reference has no counterpart (it plans one path
 * against a static map and fills no State::v). */
/* The parameters, pqp_search_params, are declared in pqp_search_params.h, which this header includes: dt (1.0 s) and ds (0.5 m), the grid;
 * w_slow (1.0) and w_accel (1.0), the prices; margin (0.0 m), pqp_agents_check's; stations (128), S; q_max (20), Q <= 63; q_up (3) and
 * q_down (6), by how much a step may grow and shrink per layer. */
#define PQP_SEARCH_MAX_STATES 4096       /* stations * (q_max + 1) may not exceed it: two cost layers of that many doubles are 64 KiB of LDS */
/* Both pure host.  pqp_search_params_from_speed starts from the defaults and sets q_max = floor(v_max dt / ds), q_up = max(1, floor(a_max
 * dt^2 / ds)), q_down = max(1, floor(d_max dt^2 / ds)), the two held to 63 (beyond q_max they change nothing); PQP_ERR_INVALID for a null pointer, a dt or ds that is not finite and positive,
 * or q_max > 63 (*p is then untouched).  The defaults are that call on pqp_speed_default_params with dt = 1, ds = 0.5. */
void pqp_search_default_params(pqp_search_params* p);
int pqp_search_params_from_speed(const pqp_speed_params* sp, double dt, double ds, pqp_search_params* p);
enum { PQP_SEARCH_NO_PLAN = 1, PQP_SEARCH_START_BLOCKED = 2, PQP_SEARCH_GRID_SHORT = 4, PQP_SEARCH_ARRIVED = 8, PQP_SEARCH_EMPTY = 16, PQP_SEARCH_NOT_FINITE = 32 };
/* Inputs (device pointers for the _device form, host pointers for the other); every one marked "or NULL" is optional:
 *   paths [batch][n][stride]          x, y, heading at offsets 0, 1, 2 and k at offset 5, stride >= 6: `out` or best_paths in place
 *   n_of, stop_before [batch] or NULL the driven count c, by pqp_speed_profile's expression
 *   profile [batch][n][PQP_SPEED_STRIDE]   s, v, a, t as pqp_speed_profile wrote them: s places the waypoints, v and a are the envelope (it
 *                                     holds the curvature, the limits and the stop before a static collision); t is not read
 *   v_start [batch]                   finite, >= 0
 *   m >= 1                            layers
 *   n_scenes, a_max, agents [n_scenes][a_max][m][PQP_AGENT_STRIDE], a_of, scene_of, car   exactly pqp_agents_check's; the agents' m steps
 *                                     are the layers
 *   frames [n_scenes][a_max][m][PQP_AGENT_FRAME_STRIDE], blocked [batch][m][W] (W = ceil(S / 32)), parents [batch][m][S][Q + 1]
 *                                     (_device form only) workspaces of the caller's; nothing is allocated.  What they hold after the
 *                                     call is not specified, except blocked
 * The definition, in fp64, every product and sum rounded on its own (no contraction), min and max as fmin and fmax; every decision that can
 * be an integer is one.  For a path with driven count c:
 *   stations   sigma_j = (double)j * ds;  M_i = max_{i' <= i} s_i', the running maximum (as pqp_sample_trajectory takes T).  Station j is on
 *              the path when sigma_j <= M_{c-1}; J = the number of such j < S (a prefix), j_last = J - 1
 *   pose at sigma_j: the sampler's interpolation with e given.  i = max(#{ i' < c : M_i' <= sigma_j } - 1, 0).  At i = c - 1 the waypoint
 *              itself.  Otherwise (dx, dy) = (x_{i+1} - x_i, y_{i+1} - y_i); d = sqrt(dx*dx + dy*dy); e = min(max(sigma_j - s_i, 0), d);
 *              lambda = d > 0 ? e / d : 0; x, y, heading, k as pqp_sample_trajectory states them
 *   envelope   w = v_i*v_i + (2*a_i)*e, or v_{c-1}*v_{c-1} at i = c - 1;  venv_j = sqrt(max(w, 0));
 *              qenv_j = (int)min(floor(venv_j * dt / ds), (double)Q)
 *   blocked(k, j), k < m, j < J: the footprint posed at station j has clear(., a) < margin against some agent a < A of the path's scene at
 *              step k - the frames and the circle test of pqp_agents_check unchanged: an absent row is skipped, a bad row blocks every
 *              station of its layer, and a pose that is not finite (an overflow) is blocked at every layer.  Bit j & 31 of word j >> 5 of
 *              blocked[b][k] holds it; bits at j >= J are 0
 *   states     (j, q) at layer k: at station j, arrived by a step of q cells.  Layer 0 holds the one state (0, q0), q0 = (int)min(max(
 *              rint(v_start * dt / ds), 0), (double)Q), at cost 0; it lives unless blocked(0, 0) or J = 0.  From a living (j', q') at
 *              layer k - 1 the step q to (j' + q, q) at layer k is allowed when
 *                max(q' - q_down, 0) <= q <= min(q' + q_up, Q);   j' + q <= j_last;   q <= max(qenv_j', qenv_{j'+q})  (the envelope at
 *                the departure covers a braking step, the one at the arrival an accelerating step);   no station of j' .. j' + q is
 *                blocked at layer k - 1 or at layer k (the step must not jump over an agent that is crossing)
 *              qref_j' = max over r in 1 .. min(Q, j_last - j') of min(r, max(qenv_j', qenv_{j'+r})), 0 when there is no such r: the largest
 *                step the envelope admits from station j'.  An allowed q is never above it
 *              edge = w_accel * (double)((q - q')*(q - q')) + w_slow * (double)(qref_j' - q)
 *                (Priced against max(qenv_j', qenv_{j'+q}) itself, a car at rest - qenv_0 = 0 - would stand for nothing and pay for every
 *                step it takes, and no plan would leave station 0: the step is priced against what the envelope allows from where it
 *                starts, which is the same thing wherever the car runs along the envelope and is 0 at j_last.)
 *              cost_k(j, q) = min_{q'} (cost_{k-1}(j - q, q') + edge), q' ascending and the lowest q' wins a tie.  A state lives when
 *              its cost is below +inf
 *   reached    the number of layers with a living state (m when the search gets through).  The plan ends in the cheapest state of layer
 *              reached - 1, ties to the largest j, then the smallest q, and is followed back through the parents
 * Outputs, fully overwritten:
 *   steps [batch][m][2]               j_k, q_k for k < reached; -1, -1 behind
 *   traj [batch][m][PQP_TRAJ_STRIDE]  k < reached: the pose at station j_k (x, y, heading, k), s = sigma_{j_k}, v = (double)q_k * ds / dt,
 *                                     a = (double)(q_{k+1} - q_k) * ds / (dt*dt) and 0 at the last planned layer, t = (double)k * dt; zeros
 *                                     behind.  It is pqp_agents_check's input shape: the plan can be handed back to the checker
 *   cost [batch]                      the plan's cost; +inf when reached = 0
 *   reached [batch], flags [batch]
 *   blocked                           an output of the host form too, where NULL means not wanted
 * flags:
 *   PQP_SEARCH_NO_PLAN         reached < m
 *   PQP_SEARCH_START_BLOCKED   reached = 0 (with PQP_SEARCH_NO_PLAN)
 *   PQP_SEARCH_GRID_SHORT      M_{c-1} > sigma_{S-1}: the grid ends before the path
 *   PQP_SEARCH_ARRIVED         the plan's last station is j_last and PQP_SEARCH_GRID_SHORT is clear
 *   PQP_SEARCH_EMPTY           c = 0: set alone; traj zeros, steps -1, reached 0, cost +inf, the path's blocked words 0
 *   PQP_SEARCH_NOT_FINITE      an x, y, heading, k, s, v or a below index c that is not finite, or a v_start that is not finite or is
 *                              negative: set alone; traj NaN, steps -1, reached 0, cost NaN, the path's blocked words 0; neighbours untouched
 * Rules this text settles where the plain reading leaves a gap: a path whose s column lies below 0 throughout has J = 0 and no state at
 * layer 0 (PQP_SEARCH_START_BLOCKED); q0 is clamped as a double before it becomes an integer; a cost that overflows to +inf is a dead state.
 * A path's result depends on its own rows, its scene and the parameters alone: the same bits at any batch position and from either form;
 * no atomics, the same answer every run.  The _device form is three launches (the frames, the occupancy, the search), asynchronous on
 * the handle's stream.  The host form stages the workspaces itself, copies in, runs, copies out and synchronises, and refuses a scene_of
 * outside [0, n_scenes) where the device form clamps.  Both forms: PQP_ERR_INVALID, with nothing launched and the outputs untouched, for a
 * null pointer that is not optional, batch < 1, n < 1, m < 1, stride < 6, a parameter outside the ranges pqp_search_params states,
 * stations * (q_max + 1) > PQP_SEARCH_MAX_STATES, or what pqp_agents_check refuses. */
int pqp_speed_search_device(pqp_handle* h, const pqp_search_params* prm, const pqp_car_geometry* car, int batch, int n, int stride,
                            const double* paths, const int32_t* n_of, const int32_t* stop_before, const double* profile, const double* v_start,
                            int m, int n_scenes, int a_max, const double* agents, const int32_t* a_of, const int32_t* scene_of, double* frames,
                            int32_t* blocked, uint8_t* parents, int32_t* steps, double* traj, double* cost, int32_t* reached, int32_t* flags);
int pqp_speed_search(pqp_handle* h, const pqp_search_params* prm, const pqp_car_geometry* car, int batch, int n, int stride,
                     const double* paths, const int32_t* n_of, const int32_t* stop_before, const double* profile, const double* v_start, int m,
                     int n_scenes, int a_max, const double* agents, const int32_t* a_of, const int32_t* scene_of, int32_t* blocked,
                     int32_t* steps, double* traj, double* cost, int32_t* reached, int32_t* flags);

/* ---- searched speed plans made drivable: a jerk-limited speed QP ---------------------------------------------------------------------------
 * pqp_speed_search ends in a staircase: stations are whole cells of ds, speeds whole cells per layer, accelerations jump by ds / dt^2 from
 * layer to layer.  It decides who yields.  This turns the decision into a plan a car can drive, behind the search on the same stream: a
 * corridor in the path-time plane around the searched stations, taken from the search's own occupancy bits, and in it the QP over
 * (s_k, v_k, a_k) per layer under the sampler's constant-acceleration kinematics, solved exactly on the banded core of the smoothers.  The
 * reference has no counterpart. */
/* The grid comes as the search's pqp_search_params, of which dt, ds and stations are read.  The refine's own numbers are PQP_REFINE_PARAMS
 * doubles, prm[PQP_REFINE_W_REF] ... prm[PQP_REFINE_D_MAX], and an int `window` beside them.  pqp_refine_default_params (pure host; a NULL
 * pointer is ignored) writes the weights 1, 1, 1, pqp_speed_default_params' a_max and d_max, and window = 4. */
#define PQP_REFINE_PARAMS 5
enum { PQP_REFINE_W_REF = 0, PQP_REFINE_W_ACCEL = 1, PQP_REFINE_W_JERK = 2, PQP_REFINE_A_MAX = 3, PQP_REFINE_D_MAX = 4 };
void pqp_refine_default_params(double* prm, int* window);
enum { PQP_REFINE_REFINED = 1, PQP_REFINE_KEPT = 2, PQP_REFINE_INFEASIBLE = 4 };
/* Inputs (device pointers for the _device form, host pointers for the other); every one marked "or NULL" is optional:
 *   paths, n_of, stop_before, profile, v_start, m     exactly what pqp_speed_search got
 *   blocked [batch][m][W], steps [batch][m][2], reached [batch], search_traj [batch][m][PQP_TRAJ_STRIDE]   what it wrote (search_traj: its traj)
 * Outputs, fully overwritten:
 *   traj [batch][m][PQP_TRAJ_STRIDE]  the refined rows, or search_traj's for a path that is kept
 *   bounds [batch][m][3] or NULL      lo_k, hi_k, vcap_k; zeros for a path that is kept
 *   cost [batch]                      the QP's objective at the solver's (s, v, a), terms added in wavefront-scan order; NaN when kept
 *   excess [batch] or NULL            see below; NaN when kept
 *   status, iters [batch]             the banded core's; PQP_STATUS_UNSOLVED and 0 for a path that never went to it
 *   flags [batch]
 * The definition, in fp64; the corridor, the QP's numbers and the placement with every product and sum rounded on its own (no
 * contraction), min and max as fmin and fmax.
 *   refined or kept   A path is refined when m >= 2 and reached = m.  Every other path is kept: its traj rows are search_traj's bit for
 *              bit, flags = PQP_REFINE_KEPT, bounds zeros, status PQP_STATUS_UNSOLVED - this covers PQP_SEARCH_NO_PLAN, PQP_SEARCH_EMPTY
 *              and PQP_SEARCH_NOT_FINITE.  Kept too, because the arrays are the device's and are judged there: a path with c = 0 or with a
 *              value the search would flag PQP_SEARCH_NOT_FINITE, J = 0, a j_k outside 0 .. j_last, or a j_k that is not free in occ_k
 *              (no search wrote such steps)
 *   corridor   all integer.  J and j_last as the search defines them, recomputed from the running maximum of the s column; j_k = steps[k][0].
 *              occ_k = blocked[k] | blocked[max(k-1, 0)] | blocked[min(k+1, m-1)], word by word: what the car must stay out of at layer k
 *              and while it moves to and from it.  The search's swept-range rule makes j_k free in all three, so the corridor is never
 *              empty.  jlo_k = the smallest j >= max(j_k - min(window, S), 0) with j .. j_k free in occ_k; jhi_k = the largest
 *              j <= min(j_k + min(window, S), j_last) with j_k .. j free.  lo_k = (double)jlo_k * ds; hi_k = (double)jhi_k * ds;
 *              vcap_k = max over jlo_k .. jhi_k of venv_j, the search's envelope at a station (max in ascending j).  At layer 0 lo = hi = 0
 *   QP         variables (s_k, v_k, a_k) per layer; a_k is the constant acceleration over [k dt, (k+1) dt] - pqp_sample_trajectory's
 *              kinematics.  minimise  sum_k w_ref (s_k - sigma_{j_k})^2 + w_accel a_k^2  +  sum_{k < m-1} w_jerk ((a_{k+1} - a_k) / dt)^2
 *              over  s_0 = 0, lo_k <= s_k <= hi_k (k >= 1);  v_0 = v_start, 0 <= v_k <= vcap_k (k >= 1);  -d_max <= a_k <= a_max (k < m-1),
 *              a_{m-1} = 0 (the search's convention for the last layer);  s_{k+1} - s_k - dt v_k - (dt^2 / 2) a_k = 0;
 *              v_{k+1} - v_k - dt a_k = 0.  3m variables, 5m - 2 rows; with w_ref > 0 or w_accel > 0 the optimum is unique
 *   solve      always the exact optimum: the banded core with polish = 1 and the tolerances of pqp_production_params, whatever the handle's
 *              path-QP setting (plain ADMM at eps 1e-3 ends a decimetre from the optimum of this QP).  A solve that ends anything but
 *              PQP_STATUS_SOLVED keeps the path as above, with status the core's, and PQP_REFINE_INFEASIBLE beside PQP_REFINE_KEPT for
 *              PQP_STATUS_PRIMAL_INFEASIBLE.  Feasibility is not guaranteed: the staircase does not satisfy the constant-acceleration
 *              dynamics, and v_start is not a whole cell
 *   refined rows, flags = PQP_REFINE_REFINED:  s = min(max(s_k, lo_k), hi_k), so the corridor holds exactly (only the solver's tolerance
 *              is clamped away); v = max(v_k, 0); a = a_k, and 0 at k = m - 1, where the row pins it; t = (double)k * dt; x, y, heading, k
 *              by the search's "pose at sigma_j" with s in place of sigma_j
 *   excess     max_k (v - sqrt(max(w, 0))), w the search's envelope expression v_i*v_i + (2*a_i)*e at the placed pose: how far the plan
 *              runs above the envelope where it actually is.  vcap_k is the largest envelope speed of the window, it does not tie v_k to
 *              s_k inside it, so excess may be positive: a limit of this QP, reported and not hidden
 * What the refine does not promise: that the refined plan is clear of every agent (stations between two free cells are not tested, as in
 * the search; pqp_sample_plan puts the plan on a fine time step for pqp_agents_check to take that verdict), and that a feasible refinement
 * exists.
 * A path's result depends on its own rows and the parameters alone: the same bits at any batch position and from either form; no atomics.
 * The _device form is four launches (the corridor, the assembly, the solve, the placement), asynchronous on the handle's stream; its QP
 * arrays and the corridor are the handle's own, apart from the smoothers', sized on first use and reused, and the rows' sparsity is uploaded
 * once per m.  The host form copies in, runs, copies out and synchronises.  Both forms: PQP_ERR_INVALID, with nothing launched and the
 * outputs untouched, for a null pointer that is not optional, batch < 1, n < 1, m < 1, stride < 6, a dt or ds that is not finite and
 * positive, stations outside 1 .. PQP_SEARCH_MAX_STATES, a weight that is not finite or is negative, w_ref + w_accel = 0, an a_max or d_max
 * that is not finite and positive, or window < 0; PQP_ERR_CAPACITY, likewise, when the QP of m layers is beyond what the core holds in one
 * compute unit's LDS (m > 193). */
int pqp_speed_refine_device(pqp_handle* h, const pqp_search_params* grid, const double* prm, int window, int batch, int n, int stride,
                            const double* paths, const int32_t* n_of, const int32_t* stop_before, const double* profile, const double* v_start,
                            int m, const int32_t* blocked, const int32_t* steps, const int32_t* reached, const double* search_traj,
                            double* traj, double* bounds, double* cost, double* excess, int32_t* status, int32_t* iters, int32_t* flags);
int pqp_speed_refine(pqp_handle* h, const pqp_search_params* grid, const double* prm, int window, int batch, int n, int stride,
                     const double* paths, const int32_t* n_of, const int32_t* stop_before, const double* profile, const double* v_start, int m,
                     const int32_t* blocked, const int32_t* steps, const int32_t* reached, const double* search_traj, double* traj,
                     double* bounds, double* cost, double* excess, int32_t* status, int32_t* iters, int32_t* flags);

/* ---- speed plans on a fine time step --------------------------------------------------------------------------------------------------------
 * pqp_speed_search and pqp_speed_refine write a plan as m rows, one per layer, dt (a second, by default) apart.  A controller tracks a
 * trajectory at a tenth of that, and an agent that crosses the lane between two layers is seen by neither the occupancy nor a check of the
 * m rows.  This puts every plan on r sub-steps per layer with the plan's own kinematics and places those stations on the path by the walk
 * the search and the refine share; the rows are pqp_agents_check's input, so the last verdict is taken at the resolution the agents are
 * predicted at.  The reference has no counterpart: it has no time axis. */
enum { PQP_PLAN_EMPTY = 1, PQP_PLAN_NOT_FINITE = 2, PQP_PLAN_BACKWARD = 4 };
/* Inputs (device pointers for the _device form, host pointers for the other); every one marked "or NULL" is optional.  dt, r and linear
 * travel by value, as pqp_agents_check's margin does:
 *   paths, n_of, stop_before, profile    exactly what pqp_speed_search and pqp_speed_refine got; c, the driven count, by the same expression
 *   plan [batch][m][PQP_TRAJ_STRIDE]     pqp_speed_refine's traj, pqp_speed_search's traj or any array of that shape: s, v, a at 4, 5, 6 are
 *                                        read.  Layer k is at time (double)k * dt
 *   count_of [batch] or NULL             the planned layers, L = min(max(count_of, 0), m): the search's `reached`.  NULL: m
 *   refine_flags [batch] or NULL         NULL: every path has the kinematics `linear` says (0: constant acceleration, 1: linear).  Given: a
 *                                        path with PQP_REFINE_REFINED set has constant acceleration, every other path is linear, and
 *                                        `linear` is not read - pqp_speed_refine's output goes in as it is.  A refined path satisfies the
 *                                        constant-acceleration rows; a kept one is the search's staircase, which does not, and a step of q
 *                                        cells is a straight line in the path-time plane: the swept range the search tested
 *   r >= 1                               sub-steps per layer: M = (m - 1) * r + 1 fine samples per path
 * Outputs, fully overwritten:
 *   fine [batch][M][PQP_TRAJ_STRIDE]     x, y, heading, k, s, v, a, t
 *   m_of [batch]                         the samples on the plan; the rows behind them are zeros
 *   defect, excess [batch] or NULL       see below
 *   flags [batch]
 * The definition, in fp64, every product and sum rounded on its own (no contraction), min and max as fmin and fmax, for a path with c >= 1
 * and L >= 1 (s_k, v_k, a_k: columns 4, 5, 6 of plan row k):
 *   m_of       (L - 1) * r + 1
 *   sample f < m_of - 1   belongs to layer k = f / r at sub-step i = f % r;  u = ((double)i * dt) / (double)r
 *              constant acceleration:  sk = s_k + (v_k + (0.5 * a_k) * u) * u (pqp_sample_trajectory's expression);  v = max(v_k + a_k * u, 0);
 *                                      a = a_k
 *              linear:                 sk = s_k + ((s_{k+1} - s_k) * (double)i) / (double)r;  v = (s_{k+1} - s_k) / dt;  a = 0
 *              both:                   s = min(max(sk, s_k), max(s_{k+1}, s_k)) - of a refined plan only the solver's tolerance is clamped
 *                                      away; a layer with s_{k+1} < s_k stands at s_k and sets PQP_PLAN_BACKWARD;  t = (double)k * dt + u
 *   sample f = m_of - 1   is row L - 1 itself: its s, max(v, 0), a, and t = (double)(L - 1) * dt
 *   x, y, heading, k      pqp_speed_search's "pose at sigma_j" with s in place of sigma_j.  So at i = 0 a row has the plan row's x, y,
 *              heading, k, s and t bit for bit, and r = 1 under constant acceleration returns a refined plan in all eight columns
 *   defect     how far the plan is from its own kinematics: under constant acceleration max over k < L - 1 of
 *              |(s_k + (v_k + (0.5 * a_k) * dt) * dt) - s_{k+1}|; 0 for a linear path or L = 1.  Reported, as excess is, not hidden
 *   excess     max over the samples on the plan of v - sqrt(max(w, 0)), w the search's envelope expression at the placed pose:
 *              pqp_speed_refine's excess, taken between the layers as well
 *   flags      PQP_PLAN_EMPTY, alone: c = 0 or L = 0; the rows are zeros, m_of = 0, defect and excess NaN.  PQP_PLAN_NOT_FINITE, alone: a
 *              path row below c that is not finite in x, y, heading, k, s, v or a, or a plan row below L whose s, v or a is not; all M
 *              rows are NaN, m_of = 0, defect and excess NaN, and the neighbours are untouched.  PQP_PLAN_BACKWARD: as above
 * A path's result depends on its own rows and the parameters alone: the same bits at any batch position and from either form; no atomics.
 * The _device form is one launch, asynchronous on the handle's stream, and allocates nothing; n, m and r are bounded only by M fitting an
 * int.  The host form copies in, runs, copies out and synchronises.  Both forms: PQP_ERR_INVALID, with nothing launched and the outputs
 * untouched, for a null pointer that is not optional, batch < 1, n < 1, m < 1, r < 1, stride < 6, a dt that is not finite and positive, a
 * linear other than 0 or 1, or (m - 1) * r + 1 > INT_MAX. */
int pqp_sample_plan_device(pqp_handle* h, double dt, int r, int linear, int batch, int n, int stride, const double* paths,
                           const int32_t* n_of, const int32_t* stop_before, const double* profile, int m, const double* plan,
                           const int32_t* count_of, const int32_t* refine_flags, double* fine, int32_t* m_of, double* defect,
                           double* excess, int32_t* flags);
int pqp_sample_plan(pqp_handle* h, double dt, int r, int linear, int batch, int n, int stride, const double* paths, const int32_t* n_of,
                    const int32_t* stop_before, const double* profile, int m, const double* plan, const int32_t* count_of,
                    const int32_t* refine_flags, double* fine, int32_t* m_of, double* defect, double* excess, int32_t* flags);

/* ---- scores of finished trajectories and each group's best --------------------------------------------------------------------------------
 * pqp_select_paths chooses between the candidates of a vehicle before any speed is planned: by the path QP's own objective.  Since
 * pqp_speed_search that is too early - the straightest candidate wins and then waits behind a pedestrian its curvier neighbour would have
 * passed.  This is the last stage of the path-speed decoupled planner: behind pqp_speed_refine, pqp_sample_plan and the fine
 * pqp_agents_check, on the same stream, it scores every finished trajectory - the path and the speed plan on it together - and leaves the
 * winner of every group on the device: its index, its waypoints and its plan rows.  The reference has no counterpart: it plans one path
 * per call and has no time axis. */
/* The parameters are PQP_RANK_PARAMS doubles, prm[PQP_RANK_W_PATH] ... prm[PQP_RANK_CLEARANCE_WANT], and an int `require_free` beside them,
 * by value, as pqp_speed_refine's are: no struct.  pqp_rank_default_params (pure host; a NULL pointer is ignored) writes the weights
 * 1, 1, 1, 1, 1, 0, pqp_select_default_params' clearance_want 0.6, and require_free = 1. */
#define PQP_PLAN_SCORE_STRIDE 10
#define PQP_RANK_PARAMS 7
enum { PQP_RANK_W_PATH = 0, PQP_RANK_W_PROGRESS = 1, PQP_RANK_W_ACCEL = 2, PQP_RANK_W_JUMP = 3, PQP_RANK_W_LATERAL = 4, PQP_RANK_W_CLEARANCE = 5,
       PQP_RANK_CLEARANCE_WANT = 6 };
void pqp_rank_default_params(double* prm, int* require_free);
/* Inputs (device pointers for the _device form, host pointers for the other); every one marked "or NULL" is optional:
 *   traj [batch][m][stride]             stride >= 8, columns as PQP_TRAJ_STRIDE documents; k (3), s (4), v (5), a (6) and t (7) are read.
 *                                       pqp_sample_plan's fine, pqp_speed_refine's traj and pqp_speed_search's traj are read where they are
 *   m_of [batch] or NULL                the rows of each candidate, c = min(max(m_of, 0), m): pqp_sample_plan's m_of, or the search's
 *                                       reached.  NULL: m.  Rows at f >= c are not read
 *   path_terms [batch][PQP_SCORE_STRIDE] or NULL   what pqp_select_paths wrote (with groups = 0 it only scores): entry 0 is the path's
 *                                       score, entry 7 its eligibility
 *   search_flags [batch] or NULL        pqp_speed_search's flags
 *   first_hit [batch] or NULL, clearance [batch][m] or NULL   what pqp_agents_check wrote on these same rows
 *   paths [batch][n][path_stride] or NULL, n_of [batch] or NULL   path_stride >= 7: the waypoints to gather for the winner (the chain's
 *                                       `out` and n_out); n_of is clamped to [0, n], NULL: all have n.  Without paths, n, path_stride
 *                                       and n_of are not read
 *   group_start [groups + 1]            exactly as pqp_select_paths takes it
 * The definition, in fp64, every product and sum rounded on its own (no contraction), min and max as fmin and fmax, for a candidate with
 * c >= 1; h_f = t_{f+1} - t_f for f < c - 1; want = prm[PQP_RANK_CLEARANCE_WANT]:
 *   terms [batch][PQP_PLAN_SCORE_STRIDE]
 *     1  progress                s_{c-1} - s_0
 *     2  acceleration effort     sum_{f < c-1} (a_f * a_f) * h_f
 *     3  acceleration jumps      sum_{f < c-1} (a_{f+1} - a_f) * (a_{f+1} - a_f); not divided by time, so under piecewise-constant
 *                                acceleration it is the same for the m plan rows and for pqp_sample_plan's fine rows at any r
 *     4  lateral acceleration    sum_{f < c-1} ((k_f * (v_f * v_f)) * (k_f * (v_f * v_f))) * h_f: where the path and the speed meet
 *     5  least clearance         min over f < c of clearance_f: +inf when every one is, NaN when one is; 0 when clearance is NULL
 *     6  clearance shortfall     sum_{f < c-1} (max(0, want - clearance_f) * max(0, want - clearance_f)) * h_f; 0 when clearance is NULL;
 *                                a clearance of -inf makes it +inf
 *     7  the path's score        path_terms[b][0]; 0 when path_terms is NULL
 *     8  duration                t_{c-1} - t_0
 *     0  score                   w_path * e7 - w_progress * e1 + w_accel * e2 + w_jump * e3 + w_lateral * e4 + w_clearance * e6, added
 *                                from left to right
 *     9  eligible                1.0 or 0.0
 * A candidate is eligible when all of these hold: c >= 1; search_flags is absent or has none of PQP_SEARCH_NO_PLAN, PQP_SEARCH_EMPTY and
 * PQP_SEARCH_NOT_FINITE; first_hit is absent, or require_free is 0, or first_hit[b] equals c; path_terms is absent or path_terms[b][7] is
 * not 0; its score is finite.  A candidate that is not eligible still gets its terms; one with c = 0 gets ten zeros.  A lane adds its own
 * samples in ascending order and the 64 partial sums meet in a fixed order, so the order of a candidate's additions depends on c alone:
 * the same candidate gives the same bits at any batch position, in any group and from either form.  No atomics.
 * Outputs, fully overwritten:
 *   terms                               as above
 *   best [groups]                       the row of the group's eligible candidate with the least score, the lowest row among equal
 *                                       scores; -1 when the group has none
 *   best_traj [groups][m][PQP_TRAJ_STRIDE], best_m [groups]   both or neither (NULL): the winner's eight columns below its count c and
 *                                       zeros behind, and c; a group without a winner is all zeros with best_m 0
 *   best_paths [groups][n][7], best_n [groups]   both or neither (NULL), and only with paths: the winner's seven columns and its count,
 *                                       zeros beyond the count; a group without a winner is all zeros with best_n 0
 * The _device form is asynchronous on the handle's stream and allocates nothing: two launches, the scores, then the groups; with
 * groups = 0 it only scores.  It cannot see group_start, so, as in pqp_select_paths, the kernel clamps every group boundary to [0, batch]
 * and takes a descending pair for an empty group: no array makes it read outside its inputs.  What a damaged array yields follows from
 * that rule alone: a group that starts at a value above batch, and the group of a descending pair, are empty (best -1, zeros); a group
 * that ends at a value above batch runs to the last row; a negative boundary counts as 0; every other group is what its own two
 * boundaries say.
 * The host form copies in, runs, copies out and synchronises.  Both forms: PQP_ERR_INVALID, with nothing launched and the outputs
 * untouched, for a null pointer that is not optional (h, prm, traj, group_start, terms, best), batch < 1, m < 1, stride < 8, paths given
 * with n < 1 or path_stride < 7, best_traj without best_m or the reverse, best_paths without best_n or the reverse, best_paths without
 * paths, groups < 0, a parameter that is not finite, or a require_free other than 0 or 1.  The host form also refuses a group_start that
 * is not ascending from 0 to batch (so, batch being at least 1, it needs one group or more). */
int pqp_select_plans_device(pqp_handle* h, const double* prm, int require_free, int batch, int m, int stride, const double* traj,
                            const int32_t* m_of, const double* path_terms, const int32_t* search_flags, const int32_t* first_hit,
                            const double* clearance, int n, int path_stride, const double* paths, const int32_t* n_of, int groups,
                            const int32_t* group_start, double* terms, int32_t* best, double* best_traj, int32_t* best_m, double* best_paths,
                            int32_t* best_n);
int pqp_select_plans(pqp_handle* h, const double* prm, int require_free, int batch, int m, int stride, const double* traj, const int32_t* m_of,
                     const double* path_terms, const int32_t* search_flags, const int32_t* first_hit, const double* clearance, int n,
                     int path_stride, const double* paths, const int32_t* n_of, int groups, const int32_t* group_start, double* terms,
                     int32_t* best, double* best_traj, int32_t* best_m, double* best_paths, int32_t* best_n);

/* ---- tracked agents to predicted rows, on the layers' steps and on fine steps ---------------------------------------------------------
 * pqp_agents_check, pqp_speed_search and the fine check behind pqp_sample_plan read agents [n_scenes][a_max][steps][PQP_AGENT_STRIDE], a
 * pose and a size per agent per time step.  A perception stack delivers tracks: a pose, a speed, an acceleration, a yaw rate, a size and
 * usually the lane the agent is in.  This turns tracks into those rows on the device: one call with r = 1 fills the rows the search reads
 * at its m layers, a second with r > 1 fills the rows of the fine check on M = (m - 1) * r + 1 steps, and by the time expression below
 * the two agree at the layers bit for bit.  Only the tracks cross to the device.  The reference has no counterpart: it plans against a
 * static map. */
/* The parameters are PQP_PREDICT_PARAMS doubles, prm[PQP_PREDICT_V_CAP] ... prm[PQP_PREDICT_L_MAX], by value as pqp_speed_refine's are: no
 * struct.  pqp_predict_default_params (pure host; a NULL pointer is ignored) writes v_cap 40 m/s (no track accelerates beyond it), grow
 * 0 m/s (what a row's radius gains per second of prediction) and l_max 3 m (how far from its lane's line a track may lie and still follow
 * it). */
#define PQP_TRACK_STRIDE 9         /* x, y, heading, v, a, yaw_rate, half_length, half_width, radius */
#define PQP_ANCHOR_STRIDE 4        /* s0, l0, dir, heading error to the lane */
#define PQP_PREDICT_PARAMS 3
enum { PQP_PREDICT_V_CAP = 0, PQP_PREDICT_GROW = 1, PQP_PREDICT_L_MAX = 2 };
void pqp_predict_default_params(double* prm);
enum { PQP_PREDICT_ABSENT = 1, PQP_PREDICT_BAD = 2, PQP_PREDICT_ON_LANE = 4, PQP_PREDICT_LANE_FAR = 8, PQP_PREDICT_OFF_LANE = 16,
       PQP_PREDICT_STOPS = 32, PQP_PREDICT_CAPPED = 64 };
/* Inputs (device pointers for the _device form, host pointers for the other); every one marked "or NULL" is optional.  t0, dt, m and r
 * travel by value:
 *   tracks [n_scenes][a_max][PQP_TRACK_STRIDE]   x, y, heading, v >= 0 along the heading, a, yaw rate w, half_length, half_width, radius >= 0
 *   a_of [n_scenes] or NULL              agents per scene, min(max(a_of, 0), a_max); NULL: a_max.  A slot at or beyond it is not read
 *   lane_of [n_scenes][a_max] int32 or NULL   the lane a track follows.  Below 0, or NULL: the free model.  At or above n_lanes: the free model
 *                                        with PQP_PREDICT_LANE_FAR; the host form refuses it
 *   lane_spline [n_lanes][9][lane_m], lane_ext [n_lanes][4], lane_length [n_lanes]   spline tables as pqp_spline_fit writes and
 *                                        pqp_project_points reads them.  With n_lanes = 0 they may be NULL
 *   m >= 1 layers dt apart from t0 on, r >= 1 sub-steps per layer: M = (m - 1) * r + 1 steps
 * Outputs, fully overwritten:
 *   agents [n_scenes][a_max][M][PQP_AGENT_STRIDE]   x, y, heading, half_length, half_width, radius: pqp_agents_check's input
 *   anchor [n_scenes][a_max][PQP_ANCHOR_STRIDE] or NULL
 *   flags [n_scenes][a_max]
 * The definition, in fp64, every product, quotient and sum rounded on its own (no contraction), min as fmin, for one track (x0, y0, h0,
 * v, a, w, ...):
 *   time of step f       k = f / r, i = f % r;  tau = t0 + ((double)k * dt + ((double)i * dt) / (double)r): pqp_sample_plan's t.  The rows
 *                        of an r = 1 call are rows k * r of an r > 1 call bit for bit
 *   the speed            a acts for te seconds, then the speed is ve for tc = tau - te seconds:
 *                          a < 0:          ts = v / (-a); te = min(tau, ts); ve = 0 when tau >= ts (the stop is reached), else v + a * te
 *                          a > 0, v < v_cap:   tl = (v_cap - v) / a; te = min(tau, tl); ve = v_cap when tau >= tl (the cap is reached), else
 *                                          v + a * te
 *                          a > 0, v >= v_cap:  te = 0, ve = v, the cap is reached: it ends an acceleration and slows nobody down
 *                          a = 0, v > 0:   te = tau, ve = v
 *                          a = 0, v = 0:   te = 0, ve = 0, the stop is reached: the track stands from the start (*)
 *                        D = (v + (0.5 * a) * te) * te + ve * tc, the distance driven.  A stopped agent neither moves nor turns.
 *                        PQP_PREDICT_STOPS: some step has reached the stop; PQP_PREDICT_CAPPED: some step has reached the cap
 *   free model           constant turn rate and acceleration in closed form.  th = w * te;  vt = v * te;  at = a * (te * te);
 *                          p = vt * sinc(th) + at * f1(th);  q = vt * cosc(th) + at * f2(th)     in the frame of h0
 *                          h1 = h0 + th;  th2 = w * tc when ve > 0, else 0;  vt2 = ve * tc
 *                          p2 = vt2 * sinc(th2);  q2 = vt2 * cosc(th2)                          in the frame of h1
 *                          x = (x0 + (p * cos h0 - q * sin h0)) + (p2 * cos h1 - q2 * sin h1)
 *                          y = (y0 + (p * sin h0 + q * cos h0)) + (p2 * sin h1 + q2 * cos h1)    one sincos per frame
 *                          heading = constrainAngle(h1 + th2)
 *                        with, for |th| >= 2^-6 and sh = sin(0.5 * th), hv = 2 * (sh * sh):
 *                          sinc = sin th / th;  cosc = hv / th;  f1 = (th * sin th - hv) / (th * th);  f2 = (sin th - th * cos th) / (th * th)
 *                        and below it their Taylor polynomials through th^5, t2 = th * th:
 *                          sinc = 1 - t2 * (1/6 - t2 * (1/120));        cosc = th * (0.5 - t2 * (1/24 - t2 * (1/720)))
 *                          f1 = 0.5 - t2 * (1/8 - t2 * (1/144));        f2 = th * (1/3 - t2 * (1/30 - t2 * (1/840)))
 *                        (the quotients 1/6 ... as fp64 constants), so w = 0 needs no case of its own and nothing divides by a small
 *                        number.  At the switch the two forms of each function differ by less than 4e-15
 *   lane model           for 0 <= lane_of < n_lanes, once per track: s0 = the abscissa of (x0, y0) on its lane as pqp_project_points
 *                        finds it (the same search, bit for bit), the lane's point and heading hp = atan2(y', x') at s0, l0 by
 *                        global2Local exactly as pqp_project_points takes its l, dh = constrainAngle(h0 - hp), dir = +1 when
 *                        cos(h0 - hp) >= 0, else -1: oncoming traffic drives towards decreasing s.
 *                        The track is not on that lane when l0 is not finite, |l0| > l_max, or the lane's length is <= 0 or >= 2^20 m
 *                        (no search is made then: s0 = l0 = dh = 0).  It gets the free model, PQP_PREDICT_LANE_FAR, and anchor
 *                        (s0, l0, 0, dh).  Otherwise PQP_PREDICT_ON_LANE is set, the yaw rate is not read, and at every step
 *                          s_f = s0 + dir * D
 *                          x, y = pqp_offsets_to_points' expression at (s_f, l0): beyond the lane's ends the spline's own extrapolation
 *                          heading = the lane's at s_f, atan2(y', x'); for dir < 0 constrainAngle of that + pi
 *                        PQP_PREDICT_OFF_LANE: some s_f lies outside [0, length]
 *   rows                 half_length and half_width are copied bit for bit; radius_f = radius + grow * tau
 *   anchor               (s0, l0, dir, dh) of a track that was searched for on a lane; four zeros for every other
 *   absent               a slot at or beyond a_of, or a track with half_length < 0 or half_width < 0: (0, 0, 0, -1, -1, 0) at every step
 *                        and PQP_PREDICT_ABSENT alone
 *   bad                  a present track with a value that is not finite, v < 0 or radius < 0: x, y and heading are NaN at every step,
 *                        half_length, half_width and radius are the track's own (no growth), and PQP_PREDICT_BAD is set alone.
 *                        pqp_agents_check reads such a row as a bad frame that hits everything: the conservative reading.  The
 *                        neighbours are untouched
 * (*) the one rule the cases above leave open: with a = 0 a standing track would otherwise turn on the spot under its yaw rate.
 * A result depends on the track, its lane and the parameters alone: the same bits at any (scene, agent) position and from either form.
 * No atomics.  The _device form is one launch, asynchronous on the handle's stream, and allocates nothing; with a_max = 0 it launches
 * nothing.  The host form copies in, runs, copies out and synchronises.  Both forms: PQP_ERR_INVALID, with nothing launched and the
 * outputs untouched, for a null pointer that is not optional (h, prm; tracks, agents and flags unless a_max = 0; the three lane arrays
 * unless n_lanes = 0), n_scenes < 1, a_max < 0, m < 1, r < 1, M > INT_MAX, n_scenes * a_max * M > 2^38, a t0 that is not finite or
 * negative, a dt that is not finite and positive, a parameter that is not finite or negative, n_lanes < 0, or lane_m < 2 with
 * n_lanes > 0. */
int pqp_predict_agents_device(pqp_handle* h, const double* prm, double t0, double dt, int m, int r, int n_scenes, int a_max,
                              const double* tracks, const int32_t* a_of, const int32_t* lane_of, int n_lanes, int lane_m,
                              const double* lane_spline, const double* lane_ext, const double* lane_length, double* agents, double* anchor,
                              int32_t* flags);
int pqp_predict_agents(pqp_handle* h, const double* prm, double t0, double dt, int m, int r, int n_scenes, int a_max, const double* tracks,
                       const int32_t* a_of, const int32_t* lane_of, int n_lanes, int lane_m, const double* lane_spline,
                       const double* lane_ext, const double* lane_length, double* agents, double* anchor, int32_t* flags);

/* ---- standing agents laid over the distance layers, one layer per scene ------------------------------------------------------------------
 * The corridor bounds, the DP search, the path QP and pqp_footprint_check read one thing about obstacles: the float distance layer.  The
 * stages around moving agents only ever change the speed along a path that was planned as if the agents were not there, so a parked car
 * that intrudes into the lane stops every candidate behind it.  This lays a scene's standing agents over a base layer: the distance to a
 * union of obstacle sets is the minimum of the distances to each, and a rounded oriented rectangle - the agent shape of pqp_agents_check -
 * has a closed-form distance, so layer(scene) = min(base layer, distance to the scene's standing agents) in one streaming pass, and no
 * distance transform is run again.  The scenes' layers then go where layers go (dist and map_of of pqp_optimize_path_device,
 * pqp_corridor_bounds, pqp_footprint_check): the scenes become the maps.  Moving agents are not overlaid: they are the speed stages'.  The
 * reference has no counterpart: it plans against one static map. */
/* The one parameter travels by value, as pqp_agents_check's margin does: inflate, in m, finite and >= 0 - extra room around every agent.
 * The corridor and the footprint check already add the car's circles and the safety margin.  pqp_overlay_default_params writes this
 * library's choice of it, 0.0, to *inflate (pure host; NULL ignored). */
void pqp_overlay_default_params(double* inflate);
enum { PQP_OVERLAY_BAD = 1, PQP_OVERLAY_NONE = 2 };
/* Inputs (device pointers for the _device form, host pointers for the other); every one marked "or NULL" is optional:
 *   dist [n_maps][cols][rows] float   the base layers, in the layout every reader of a layer takes
 *   geom                              as for pqp_corridor_bounds; every field is read here, the cells' centres being needed
 *   agents [n_scenes][a_max][PQP_AGENT_STRIDE]   a row per agent, x, y, heading, half_length, half_width, radius: pqp_agents_check's agents
 *                                     with m = 1 and its readings - half_length < 0 or half_width < 0: absent, the rest of the row is not
 *                                     read; a present row with a value that is not finite or with a negative radius is bad.  a_max = 0 is
 *                                     allowed (agents and frames may then be NULL)
 *   a_of [n_scenes] or NULL           agents per scene: A = clamp(a_of, 0, a_max); NULL: all a_max
 *   base_of [n_scenes] or NULL        the base layer a scene starts from; the host form refuses values outside [0, n_maps), the device
 *                                     form clamps them.  NULL: layer 0 when n_maps = 1, else scene s starts from layer s, which needs
 *                                     n_scenes = n_maps
 *   frames [n_scenes][a_max][PQP_AGENT_FRAME_STRIDE]   (_device form only) a workspace of the caller's, fully written by the first launch
 * Outputs, fully overwritten:
 *   dist_out [n_scenes][cols][rows] float   the scenes' layers.  dist_out = dist is allowed exactly when base_of is NULL and n_scenes =
 *                                     n_maps: every cell is read and then written by the same lane, and nothing else of the layer is read
 *   flags [n_scenes]                  PQP_OVERLAY_BAD, PQP_OVERLAY_NONE or 0
 * Two launches on the handle's stream.  The first is pqp_agents_check's with one step per agent: every agent row becomes a frame row
 * (ax, ay, c, s, hl, hw, radius, reach), bit for bit what pqp_agents_check makes of it.  The second is the overlay.  The definition, in
 * fp64, every product and sum rounded on its own (no contraction), min and max as fmin and fmax, for cell (i, j) of scene s - index
 * j * rows + i of its layer - and agent a < A:
 *   cx = (pos_x + (0.5*length_x - 0.5*resolution)) + resolution * (double)(-i);  cy likewise with pos_y, length_y and j
 *                                     (GridMap::getPosition, the expression the readers of a layer place their cells by)
 *   dx = cx - ax;  dy = cy - ay;  u = dx*c + dy*s;  w = dy*c - dx*s
 *   ex = fabs(u) - hl;  ey = fabs(w) - hw;  ox = fmax(ex, 0);  oy = fmax(ey, 0)
 *   d = sqrt(ox*ox + oy*oy) + fmin(fmax(ex, ey), 0) - radius          (pqp_agents_check's d for one point, r_j = 0)
 *   da = fmax(d - inflate, 0)
 *   dmin = min over the scene's present agents of da, +inf when there is none
 *   out = (dmin < (double)b) ? (float)dmin : b          b: the base value of the cell; (float) rounds to nearest
 * A NaN base value therefore stays, and a cell the agents do not undercut is copied bit for bit.  A scene with a bad agent below its
 * count gets 0.0f in every cell and PQP_OVERLAY_BAD: the conservative reading - pqp_agents_check lets a bad agent hit everything, and
 * here the corridor is empty, so the chain reports the scenario blocked; the neighbouring scenes are untouched.  A scene with no present
 * agent is a copy of its base layer and gets PQP_OVERLAY_NONE.  Every other scene gets 0.
 * The overlay leaves out an agent that is too far from a tile of cells to undercut the largest base value in it (not where a base value
 * of the tile is NaN); that changes no output while the squares of the coordinates are finite.  A result depends on the cell, the
 * scene's rows, its base layer and inflate alone - not on the tiling, the position in the batch or which form was called; no atomics, the
 * same answer every run.
 * The _device form is asynchronous on the handle's stream and allocates nothing, so it can stand between pqp_distance_layer_device and
 * pqp_optimize_path_device; rows, cols, a_max and n_scenes have no cap beyond those below.  The host form stages frames itself, copies
 * in, runs, copies out and synchronises.  Both forms: PQP_ERR_INVALID, with nothing launched and the outputs untouched, for a null
 * pointer that is not optional, n_maps < 1, n_scenes < 1, a_max < 0, a geometry pqp_distance_layer refuses or one whose lengths or
 * position are not finite, an inflate that is not finite or is negative, n_scenes * rows * cols > 2^38, base_of = NULL with n_maps > 1
 * and n_scenes != n_maps, or dist_out = dist in any other case than the one allowed above. */
int pqp_overlay_agents_device(pqp_handle* h, double inflate, int n_maps, const pqp_grid_geometry* geom, const float* dist, int n_scenes,
                              int a_max, const double* agents, const int32_t* a_of, const int32_t* base_of, double* frames, float* dist_out,
                              int32_t* flags);
int pqp_overlay_agents(pqp_handle* h, double inflate, int n_maps, const pqp_grid_geometry* geom, const float* dist, int n_scenes, int a_max,
                       const double* agents, const int32_t* a_of, const int32_t* base_of, float* dist_out, int32_t* flags);

/* ---- the start of a cycle from the previous cycle's plan: trajectory stitching ------------------------------------------------------------
 * Every stage from the tracks to pqp_select_plans plans one cycle, from a start, a start curvature and a start speed the caller gives.  A
 * planner that starts every cycle from the measured pose feeds its own tracking error back into the plan: the path and the speed jump
 * at every cycle.  The new plan therefore starts on the old one, a little ahead of the car; it starts from the measurement only when the
 * car has left the plan, and the controller gets the piece of the old plan that bridges the gap.  This is that stage, in front of
 * pqp_optimize_path_device as pqp_overlay_agents is: per group it reads the previous cycle's winner where pqp_select_plans left it
 * (best_traj and best_m; pqp_sample_plan's and pqp_sample_trajectory's rows are the same rows), a measured state and the time since that
 * plan began, and writes the state the new cycle plans from, the verdict and its reasons, the deviations, the re-based piece of the old
 * plan that leads to the start, and that start spread over the group's candidates in the arrays the chain (start, start_k) and
 * pqp_speed_profile (v_start) read.  Only the measurements cross to the device.  The reference has no counterpart: it plans one path per
 * call from the state it is given. */
/* The parameters are PQP_STITCH_PARAMS doubles, prm[PQP_STITCH_T_AHEAD] ... prm[PQP_STITCH_V_CAP], and two ints beside them, keep and
 * prefix_max, by value as pqp_select_plans' are: no struct.  pqp_stitch_default_params (pure host; a NULL pointer is ignored) writes
 * t_ahead 0.1 s (how far ahead of the measurement's time the new plan starts), lat_max 0.5 m, lon_max 2.5 m and dh_max 0.5 rad (the
 * deviations beyond which the car has left the plan), v_still 0.1 m/s (at or below it a replanned start has curvature 0), v_cap +inf
 * (the cap of the free model of pqp_predict_agents), and keep = 20 (the rows of the old plan kept behind the car). */
#define PQP_STITCH_PARAMS 6
enum { PQP_STITCH_T_AHEAD = 0, PQP_STITCH_LAT_MAX = 1, PQP_STITCH_LON_MAX = 2, PQP_STITCH_DH_MAX = 3, PQP_STITCH_V_STILL = 4, PQP_STITCH_V_CAP = 5 };
void pqp_stitch_default_params(double* prm, int* keep);
enum { PQP_STITCH_BAD = 1, PQP_STITCH_NO_PREVIOUS = 2, PQP_STITCH_TIME = 4, PQP_STITCH_BAD_PLAN = 8, PQP_STITCH_LATERAL = 16,
       PQP_STITCH_LONGITUDINAL = 32, PQP_STITCH_HEADING = 64, PQP_STITCH_REPLAN = 128, PQP_STITCH_STITCHED = 256, PQP_STITCH_PREFIX_CUT = 512,
       PQP_STITCH_STANDING = 1024 };
/* Inputs (device pointers for the _device form, host pointers for the other); every one marked "or NULL" is optional:
 *   prev [groups][m][stride]            stride >= 8, the columns of PQP_TRAJ_STRIDE: x, y, heading, k, s, v, a, t.  Columns beyond 7 are not read
 *   m_of [groups] or NULL               the rows of each plan, M = min(max(m_of, 0), m): pqp_select_plans' best_m.  NULL: m.  Rows at
 *                                       f >= M are not read
 *   meas [groups][6]                    x, y, heading, v >= 0, a, yaw rate w: the first six columns of a row of PQP_TRACK_STRIDE
 *   t_now [groups]                      the time of the measurement in the previous plan's time base (its column t)
 *   batch, group_start [groups + 1] or NULL   the candidates of group g are group_start[g] .. group_start[g + 1] - 1, read exactly as
 *                                       pqp_select_paths reads them (every boundary clamped to [0, batch], a descending pair an empty
 *                                       group); NULL: candidate g is group g's, and batch = groups
 * The definition, in fp64, every product, quotient and sum rounded on its own (no contraction), for one group; x_f ... t_f are the
 * columns of row f < M, (x, y, hd, v, a, w) the measurement, tq = t_now + t_ahead:
 *   1  bad measurement   one of the six values or t_now is not finite, or v < 0: PQP_STITCH_BAD alone; the state row, dev and the prefix
 *                        are zeros, idx is (-1, -1, -1), prefix_n = 0, and the group's candidates get the zero start.  Nothing else is
 *                        evaluated: the flag tells the caller to ignore what the cycle makes of these candidates, and no NaN goes on
 *   2  no previous plan  M < 2: PQP_STITCH_NO_PREVIOUS.  3 to 5 are not evaluated: idx is (-1, -1, -1), dev zeros
 *   3  time match        i_now = the first f with t_f >= t_now;  i_start = the first f with t_f >= tq.  "First" is a plain scan from 0:
 *                        ascending rows are not assumed, and a comparison with a NaN is false.  -1 where there is none.
 *                        PQP_STITCH_TIME: t_now < t_0, or there is no i_start.  (t_ahead >= 0, so i_now <= i_start where both are)
 *   4  position match    d2_f = (x - x_f) * (x - x_f) + (y - y_f) * (y - y_f), +inf where that is not finite;  p = the lowest f with the
 *                        least d2_f, -1 when every d2_f is +inf.  PQP_STITCH_BAD_PLAN: p = -1, or one of the rows p, i_now, i_now - 1
 *                        and i_start - those that exist - holds a value that is not finite among its eight columns
 *   5  deviations        evaluated when PQP_STITCH_BAD_PLAN is not set and i_now exists, else dev is zeros and none of their three
 *                        flags is set.  In the frame of row p:  sh, ch = sincos(heading_p);  dx = x - x_p;  dy = y - y_p;
 *                          lat = -dx * sh + dy * ch                                            (global2Local's expression order)
 *                          s_ref = s_0 when i_now = 0, else with i = i_now
 *                                  s_{i-1} + (s_i - s_{i-1}) * ((t_now - t_{i-1}) / (t_i - t_{i-1}))  (t_{i-1} < t_now <= t_i: no division by 0)
 *                          lon = s_ref - (s_p + (dx * ch + dy * sh))
 *                          dh = constrainAngle(hd - heading_p)
 *                        PQP_STITCH_LATERAL: not |lat| <= lat_max;  PQP_STITCH_LONGITUDINAL: not |lon| <= lon_max;  PQP_STITCH_HEADING:
 *                        not |dh| <= dh_max - for numbers that is |.| > max, and a deviation that overflowed to NaN is flagged too
 *   6  verdict           one of NO_PREVIOUS, TIME, BAD_PLAN, LATERAL, LONGITUDINAL, HEADING: PQP_STITCH_REPLAN, else
 *                        PQP_STITCH_STITCHED.  Every reason that applies is set
 *   7  stitched          the state row is row i_start, its eight columns bit for bit.  i0 = max(0, i_now - keep); when prefix is given
 *                        and i_start - i0 + 1 > prefix_max: i0 = i_start - prefix_max + 1 and PQP_STITCH_PREFIX_CUT.
 *                        prefix_n = i_start - i0 + 1;  prefix row j < prefix_n is row i0 + j with s - s_{i_start} in column 4 and
 *                        t - t_{i_start} in column 7, every other column copied bit for bit: it ends at s = 0, t = 0
 *   8  replanned         the measurement advanced by tau = t_ahead under pqp_predict_agents' free model, v_cap its cap: (te, ve) and
 *                        whether the stop or the cap is reached by "the speed" there, tc = tau - te, (px, py, ph) by "free model".
 *                        The state row is (px, py, ph, k, 0, ve, ae, tq) with k = w / ve when ve > v_still, else 0, and ae = a, or
 *                        0 when the stop or the cap is reached (the acceleration no longer acts at tau).  PQP_STITCH_STANDING: ve = 0.
 *                        prefix_n = 1, and the one prefix row is the state row with t = 0
 *   9  candidates        for every candidate b of the group: start[b] = columns 0, 1, 2 of the state row, start_k[b] = column 3,
 *                        v_start[b] = column 5
 * Outputs, fully overwritten (start, start_k and v_start: at the candidates that are in a group):
 *   state [groups][PQP_TRAJ_STRIDE]     the state the new cycle plans from.  Column 7 is the instant, in the old time base, at which the
 *                                       new plan's t = 0 lies: the caller keeps its clock by it.  Column 6 is reported, no stage consumes it
 *   flags [groups]                      PQP_STITCH_*
 *   dev [groups][3]                     lon, lat, dh
 *   idx [groups][3] int32               i_now, p, i_start
 *   prefix [groups][prefix_max][PQP_TRAJ_STRIDE] or NULL   rows at and beyond prefix_n are zeros.  NULL: prefix_max is not read and nothing
 *                                       is cut; prefix_n is still the count
 *   prefix_n [groups]
 *   start [batch][3], start_k [batch], v_start [batch]   each or NULL
 * A group's result depends on its own inputs alone: the same bits at any position in any batch and from either form.  No atomics.  The
 * _device form is one launch, asynchronous on the handle's stream, and allocates nothing, so it can stand in front of
 * pqp_optimize_path_device with the previous call's best_traj as prev.  The host form copies in, runs, copies out and synchronises.
 * Both forms: PQP_ERR_INVALID, with nothing launched and the outputs untouched, for a null pointer that is not optional (h, prm, prev,
 * meas, t_now, state, flags, dev, idx, prefix_n), groups < 1, m < 1, stride < 8, batch < 0, keep < 0, prefix given with prefix_max < 1,
 * a parameter that is negative or NaN, a t_ahead or v_still that is not finite, or group_start = NULL with one of start, start_k and
 * v_start given and batch != groups.  The host form also refuses a group_start that is not ascending from 0 to batch. */
int pqp_stitch_trajectory_device(pqp_handle* h, const double* prm, int keep, int prefix_max, int groups, int m, int stride, const double* prev,
                                 const int32_t* m_of, const double* meas, const double* t_now, int batch, const int32_t* group_start,
                                 double* state, int32_t* flags, double* dev, int32_t* idx, double* prefix, int32_t* prefix_n, double* start,
                                 double* start_k, double* v_start);
int pqp_stitch_trajectory(pqp_handle* h, const double* prm, int keep, int prefix_max, int groups, int m, int stride, const double* prev,
                          const int32_t* m_of, const double* meas, const double* t_now, int batch, const int32_t* group_start, double* state,
                          int32_t* flags, double* dev, int32_t* idx, double* prefix, int32_t* prefix_n, double* start, double* start_k,
                          double* v_start);

/* ---- a plan for every group: braking fallbacks where no candidate wins ---------------------------------------------------------------
 * pqp_select_plans leaves a group none of whose candidates is eligible with best = -1, best_m = 0 and zero rows: a pedestrian stands in
 * every candidate's lane for the whole horizon, every search ends PQP_SEARCH_NO_PLAN, or every path QP fails.  The controller then has
 * nothing to track, and the next cycle's stitch reads best_m = 0 and replans from the raw measurement: the plan is lost in the cycle in
 * which continuity matters most.  These two stages, behind pqp_select_plans on the same stream, close that hole: the car brakes along the
 * plan it is already on - prev of pqp_stitch_trajectory, from the state that stitch chose - as gently as the agents and the distance
 * layers allow.  pqp_fallback_rows writes one braking plan per group and braking level; pqp_agents_check_device (m_of = NULL: the car is
 * checked while it stands too) and pqp_footprint_check_device (stride 8: x, y, heading lie where it reads them) test the groups *
 * n_levels plans as the batch of trajectories they are, unchanged; pqp_fallback_pick keeps a group's winner where it has one and else
 * takes the gentlest level that passed both.  Column 6 of the stitch's state row, the acceleration at the seam, is consumed here: the
 * braking starts from it and leaves it at a bounded jerk.  The reference has no counterpart: its solve returns false and the caller has
 * no path.
 * What this does not do: it does not steer away (the place is on the old plan or on the arc, never beside them), it does not re-plan the
 * path, it has no plan for a state flagged bad, and it has one jerk phase only: the release of the brake at the stop is a step, as in the
 * free model's "standing once stopped". */
/* The parameters: PQP_FALLBACK_PARAMS doubles (prm[PQP_FALLBACK_A_CAP], the cap on the acceleration the braking starts from) and the
 * levels [n_levels][2], each row (d, j): a braking d > 0 in m/s^2 and a jerk j > 0 in m/s^3, d ascending (equal neighbours are allowed),
 * 1 <= n_levels <= PQP_FALLBACK_MAX_LEVELS.  Both are host pointers in both forms, as prm is elsewhere; no struct.
 * pqp_fallback_default_params (pure host; a NULL pointer is ignored; levels must hold PQP_FALLBACK_DEFAULT_LEVELS rows) writes this
 * library's choice, around pqp_speed_default_params' d_max = 3.0 and a_max = 1.5:
 *   level 0  d = 1.5 (d_max / 2), j = 2.5   comfortable: inside the 2 m/s^2 and 2.5 m/s^3 ISO 15622 lets an adaptive cruise control use at speed
 *   level 1  d = 3.0 (d_max),     j = 5.0   what the speed stages plan with; 5 m/s^3 is ISO 15622's jerk bound at low speed
 *   level 2  d = 6.0 (2 d_max),   j = 15.0  emergency: above the 5 m/s^2 UN Regulation 152 demands of an emergency braking system, below what dry
 *                                           asphalt gives (8 to 10 m/s^2); the brake pressure of such a system builds up in a few tenths of a second
 *   a_cap = a_max = 1.5: a seam acceleration above what the speed stages plan with is a bad number, not a state to continue */
#define PQP_FALLBACK_PARAMS 1
#define PQP_FALLBACK_MAX_LEVELS 8
#define PQP_FALLBACK_DEFAULT_LEVELS 3
enum { PQP_FALLBACK_A_CAP = 0 };
void pqp_fallback_default_params(double* prm, double* levels, int* n_levels);
enum { PQP_FALLBACK_BAD = 1, PQP_FALLBACK_ARC = 2, PQP_FALLBACK_BAD_PLAN = 4, PQP_FALLBACK_PATH_SHORT = 8, PQP_FALLBACK_HORIZON = 16,
       PQP_FALLBACK_TAKEN = 32, PQP_FALLBACK_NOT_CLEAR = 64 };
/* pqp_fallback_rows.  Inputs (device pointers for the _device form, host pointers for the other); every one marked "or NULL" is optional:
 *   prev [groups][mp][stride] or NULL   the arrays pqp_stitch_trajectory reads: stride >= 8, columns 0 to 4 (x, y, heading, k, s) are read.
 *                                       NULL: every group brakes on its arc; mp and stride are then not read, and prev_m must be NULL
 *   prev_m [groups] or NULL             the rows of each plan, Mp = min(max(prev_m, 0), mp).  NULL: mp
 *   state [groups][PQP_TRAJ_STRIDE]     the stitch's state row: x0, y0, h0, k0, the station s on prev, v0, the acceleration a.  Column 7 is
 *                                       not read
 *   stitch_flags [groups] or NULL       pqp_stitch_trajectory's flags.  NULL: every group counts as PQP_STITCH_STITCHED and none as bad
 *   dt, r, m                            M = (m - 1) r + 1 rows per plan; row f lies at t_f = (double)(f / r) * dt + ((double)(f % r) * dt) / (double)r,
 *                                       pqp_sample_plan's expression: the agents' rows on the plan's fine steps and these rows share their
 *                                       instants bit for bit.  r = 1 gives the layers' steps
 * The definition, in fp64, every product, quotient, sum and square root rounded on its own (no contraction), for one group and one level
 * (d, j):
 *   1  bad state         one of the state's columns 0 to 6 is not finite, v0 < 0, or stitch_flags has PQP_STITCH_BAD: PQP_FALLBACK_BAD alone;
 *                        the rows and stop are zeros, stop_row = 0.  Nothing else is evaluated, and no NaN goes on
 *   2  the law           a0 = min(max(a, -d), a_cap).  The acceleration falls from a0 at -j until it is -d, holds -d until the car stands,
 *                        and is 0 from then on:
 *                          t1 = (a0 + d) / j                                     (the end of the ramp; 0 when a0 = -d)
 *                          ts = (a0 + sqrt(a0 * a0 + (2 * j) * v0)) / j          (where v0 + a0 t - j t^2 / 2 reaches 0)
 *                          E(t) = (v0 + (0.5 * a0 - (j * t) / 6) * t) * t;   V(t) = v0 + (a0 - (0.5 * j) * t) * t
 *                          v1 = max(V(t1), 0);   s1 = E(t1);   u1 = v1 / d
 *                          ts <= t1 (the car comes to rest inside the ramp):  T = ts, eT = max(E(ts), 0)
 *                          else:                                              T = t1 + u1, eT = max(s1 + (v1 - (0.5 * d) * u1) * u1, 0)
 *                        Row f, at t = t_f:
 *                          t >= T   at rest:   e = eT, v = 0, acc = 0
 *                          t < t1   the ramp:  e = E(t), v = V(t), acc = a0 - j * t
 *                          else     the hold:  u = t - t1;  e = s1 + (v1 - (0.5 * d) * u) * u;  v = v1 - d * u;  acc = -d
 *                        then e = min(max(e, 0), eT) and v = max(v, 0).  Columns 4, 5, 6, 7 of the row are e, v, acc, t: the plan starts at
 *                        s = 0, t = 0, where the stitch's prefix ends.  A car with v0 = 0 and a0 <= 0 has ts = 0 and stands from row 0
 *   3  the place         on the arc - PQP_FALLBACK_ARC - when stitch_flags is given without PQP_STITCH_STITCHED or Mp < 2; else the rows
 *                        below Mp are examined, and one whose columns 0 to 4 hold a value that is not finite sets PQP_FALLBACK_BAD_PLAN
 *                        and PQP_FALLBACK_ARC.  (A group that is on the arc for one of the first two reasons has no row read.)
 *      on the plan       sigma = s + e.  S_i = max(s_0 .. s_i), the exact running maximum of prev's s column (pqp_sample_trajectory's walk,
 *                        there over t); cnt = #{ i < Mp : S_i <= sigma }; i = max(cnt - 1, 0).
 *                          i < Mp - 1:  ds = s_{i+1} - s_i;  lambda = min(max((sigma - s_i) / ds, 0), 1) when ds > 0, else 0;
 *                                       x = x_i + lambda * (x_{i+1} - x_i), y likewise, k = k_i + lambda * (k_{i+1} - k_i),
 *                                       heading = constrainAngle(h_i + lambda * constrainAngle(h_{i+1} - h_i))   (pqp_sample_trajectory's chord)
 *                          else:        columns 0 to 3 of row Mp - 1, and PQP_FALLBACK_PATH_SHORT when sigma > S_{Mp-1}: the plan ends
 *                                       before the car stands
 *                        A sigma in front of row 0 has cnt = 0 and lambda = 0: it stands on row 0
 *      on the arc        th = k0 * e;  sinc, cosc = pqp_predict_agents' "free model" functions at th, with its Taylor switch at 2^-6;
 *                        sh0, ch0 = sincos(h0);  p = e * sinc;  q = e * cosc;
 *                          x = x0 + (p * ch0 - q * sh0);  y = y0 + (p * sh0 + q * ch0);  heading = constrainAngle(h0 + th);  k = k0
 *                        With k0 = 0 the heading, k and the columns 4 to 7 hold no sincos and are the same bits on any machine; x and y
 *                        are x0 + e * ch0 and y0 + e * sh0 and are so only where sincos(h0) is exact (h0 = 0): elsewhere the device's sincos
 *                        and a host's may differ in the last bits, as for every pose of the free model
 *   4  the records       stop = (T, eT).  stop_row = #{ f < M : t_f < T }, which is the first row at rest, or M - and
 *                        PQP_FALLBACK_HORIZON - when the stop lies beyond the horizon.  The rows at and behind stop_row are equal but for t
 * Outputs, fully overwritten:
 *   rows [groups][n_levels][M][PQP_TRAJ_STRIDE]   x, y, heading, k, s, v, a, t
 *   stop [groups][n_levels][2], stop_row [groups][n_levels], flags [groups][n_levels] of PQP_FALLBACK_BAD .. PQP_FALLBACK_HORIZON
 * A plan depends on its own group, its level and the parameters alone: the same bits at any position in any batch and from either form.
 * No atomics.  The _device form is one launch, asynchronous on the handle's stream, and allocates nothing.  Both forms: PQP_ERR_INVALID,
 * with nothing launched and the outputs untouched, for a null pointer that is not optional (h, prm, levels, state, rows, stop, stop_row,
 * flags), groups < 1, n_levels outside 1 .. 8, groups * n_levels beyond an int, a level whose d or j is not finite and positive, a d
 * below its predecessor's, an a_cap that is negative or NaN, a dt that is not finite and positive, r < 1, m < 1, (m - 1) r + 1 beyond
 * INT_MAX - 64 (a tile of 64 samples is indexed by an int), prev given with mp < 1 or stride < 8, or prev_m given without prev. */
int pqp_fallback_rows_device(pqp_handle* h, const double* prm, int n_levels, const double* levels, double dt, int r, int m, int groups, int mp,
                             int stride, const double* prev, const int32_t* prev_m, const double* state, const int32_t* stitch_flags, double* rows,
                             double* stop, int32_t* stop_row, int32_t* flags);
int pqp_fallback_rows(pqp_handle* h, const double* prm, int n_levels, const double* levels, double dt, int r, int m, int groups, int mp, int stride,
                      const double* prev, const int32_t* prev_m, const double* state, const int32_t* stitch_flags, double* rows, double* stop,
                      int32_t* stop_row, int32_t* flags);
/* pqp_fallback_pick: one trajectory per group, always.  Inputs, with m_rows = M:
 *   best [groups] or NULL               pqp_select_plans' winners.  NULL: every group falls back
 *   best_traj [groups][m_rows][PQP_TRAJ_STRIDE], best_m [groups]   both or neither: the winners' rows
 *   rows, row_flags                     pqp_fallback_rows' rows and flags
 *   first_hit [groups * n_levels] or NULL, first_collision [groups * n_levels] or NULL   pqp_agents_check's and pqp_footprint_check's
 *                                       verdicts on the plans, plan g * n_levels + l being level l of group g.  NULL: that check was not run
 * A group with best[g] >= 0 keeps its winner: final_traj is best_traj's rows bit for bit and final_m = best_m[g] (without best_traj: zeros
 * and 0 - the caller has the winner), level = -1, flags = 0.  Any other group falls back.  A level is usable when its flags have neither
 * PQP_FALLBACK_BAD nor PQP_FALLBACK_PATH_SHORT, first_hit is absent or equals m_rows, and first_collision is absent or equals m_rows.
 *   a bad group       a level flagged PQP_FALLBACK_BAD: level = -1, final_traj zeros, final_m = 0, flags = PQP_FALLBACK_BAD alone
 *   a usable level    the lowest one; flags = its flags | PQP_FALLBACK_TAKEN
 *   none usable       the level whose first contact min(first_hit, first_collision) - an absent one counting as m_rows - is latest, among
 *                     equal ones the highest; flags = its flags | PQP_FALLBACK_TAKEN | PQP_FALLBACK_NOT_CLEAR.  The verdicts are read as
 *                     they are, not clamped: a negative one is an earlier contact than any row, and the rule still names a level
 *   final_traj is that level's rows bit for bit and final_m = m_rows: the car is planned for the whole horizon, standing rows included
 * Outputs, fully overwritten: final_traj [groups][m_rows][PQP_TRAJ_STRIDE], final_m [groups], level [groups], flags [groups] - by shape and
 * by meaning what the next cycle passes to pqp_stitch_trajectory as prev and m_of.  A group's result depends on its own inputs alone; no
 * atomics; the _device form is one launch on the handle's stream and allocates nothing.  Both forms: PQP_ERR_INVALID, with nothing
 * launched and the outputs untouched, for a null pointer that is not optional (h, rows, row_flags, final_traj, final_m, level, flags),
 * groups < 1, n_levels outside 1 .. 8, groups * n_levels beyond an int, m_rows < 1 or beyond INT_MAX - 64, or one of best_traj and best_m
 * without the other. */
int pqp_fallback_pick_device(pqp_handle* h, int groups, int n_levels, int m_rows, const int32_t* best, const double* best_traj, const int32_t* best_m,
                             const double* rows, const int32_t* row_flags, const int32_t* first_hit, const int32_t* first_collision,
                             double* final_traj, int32_t* final_m, int32_t* level, int32_t* flags);
int pqp_fallback_pick(pqp_handle* h, int groups, int n_levels, int m_rows, const int32_t* best, const double* best_traj, const int32_t* best_m,
                      const double* rows, const int32_t* row_flags, const int32_t* first_hit, const int32_t* first_collision, double* final_traj,
                      int32_t* final_m, int32_t* level, int32_t* flags);

#ifdef __cplusplus
}
#endif
#endif /* PQP_H_ */
