/*
 * lqmpc.h -- C ABI of the MI355X batched LQ-MPC box-QP solver (liblqmpc_hip.so).
 *
 * The reference (lcrekko/lq_mpc) has no FFI: its operator boundary for this path is two
 * Python classes.  Each entry point below names the reference interface it replaces:
 *
 *   lqmpc_solve_batch    <- LQ_MPC_Controller.solve          /root/reference/utils_class.py:48-91
 *                           (one call per instance there; Bsz instances per call here)
 *   lqmpc_rollout_batch  <- LQ_MPC_Simulator.simulate        /root/reference/utils_class.py:245-285
 *   lqmpc_sweep_batch    <- one (error level | horizon) of data_generation: both of the following in one call
 *   lqmpc_bounds_batch   <- the rest of one pass of data_generation: control.dlqr + LQ_RDP_Calculator.energy_decreasing +
 *                           energy_bound + the bound               /root/reference/utils_class.py:837-859, 920-942
 *                                                                  (utils_class.py:308-373; utils.py:78-117, 186-584)
 *   lqmpc_max_vn_batch   <- the M_V loops of
 *                           LQ_RDP_Behavior_Multiple.data_generation
 *                                                            /root/reference/utils_class.py:813-824, 896-907
 *                           and LQ_RDP_Behavior.OL_energy_bound  utils_class.py:439-466
 *
 * Problem solved per instance (utils_class.py:59-91; n = N*nu; no 1/2 factor):
 *   min  sum_{i=0}^{N-2} |x_{i+1}-xref_i|^2_Q + |x_N-xref_{N-1}|^2_P + sum_{i=0}^{N-1} |u_i-uref_i|^2_R
 *   s.t. x_{i+1} = A x_i + B u_i,   lb <= u_i <= ub     (F_u u_i <= 1 with box rows, line 81)
 *   u_0 = u*[:,0],  V_N = cost* + x0' Q x0               (line 91)
 *
 * Data layout.  Per-instance arrays are instance-minor ("SoA", the layout of the reference's
 * error_{A,B}_f.npy files, utils_class.py:749-750):
 *     A[(r*nx + c)*Bsz + b]   B[(r*nu + k)*Bsz + b]   x0[a*Bsz + b]
 *     u0[k*Bsz + b]  VN[b]  JT[b]  MV[b]  status[b]  iters[b]
 *     X[(a*(T+1) + t)*Bsz + b]   U[(k*T + t)*Bsz + b]            (optional trajectories)
 * Shared by the whole batch (plain row-major, always HOST pointers, copied by the call):
 *     Q (nx,nx)  R (nu,nu)  P (nx,nx)  lb (nu)  ub (nu)
 *     x_ref (nx,N) / u_ref (nu,N) as the reference passes them; NULL means zeros
 *     A_true (nx,nx), B_true (nx,nu) when true_per_instance == 0
 *     x0s (nx,K): the K initial states of lqmpc_max_vn_batch
 * All floating point is IEEE fp64, as in the reference.
 *
 * Box limit: every kernel writes the box as u = v + c, |v| <= h (c = (lb+ub)/2, h = (ub-lb)/2), and scales its
 * stopping tests with the gradient of the shifted problem, which holds P c.  A centre far from the inputs' own
 * scale therefore costs accuracy in proportion to |c| (a one-sided limit written as [0, 1e6] is off by O(1)).  The
 * calls refuse, with LQMPC_ERR_BAD_ARG, a box whose centre has |lb_k + ub_k| / 2 > LQMPC_MAX_BOX_CENTRE for any
 * input k.  Symmetric boxes of any width (c = 0) are accepted; a one-sided limit is written with a finite other
 * side near the largest input expected (e.g. [0, 2 u_max] instead of [0, 1e6]).
 * Known inaccuracy inside the limit: with a one-sided box [0, b] and small states, many rows sit on or near the bound
 * with multipliers far below |P c|.  The generic kernel and the workgroup kernel's interior-point fall-back (taken when its
 * active-set solve cycles) then stop on the wrong face: relative errors up to 1e-7 measured at n = 120, 125 with the
 * default eps (1e-12); the packed kernel's interior-point path (warm_start = 0) shows 1e-8 at n = 40.  eps = 1e-14
 * reduces them (1e-14 at n = 125).  With default options the 16-lane-row kernels meet 1e-11 there (n = 20, 40).
 *
 * Two flavours of every batched call:
 *   lqmpc_*_batch      per-instance pointers are HOST memory; the call copies in, runs, copies
 *                      out and returns when the results are in the caller's buffers.
 *   lqmpc_*_batch_dev  per-instance pointers are DEVICE memory on the handle's GPU; the call
 *                      enqueues on the handle's stream and returns (use lqmpc_sync).
 *
 * Errors: every call returns 0 on success or a negative lqmpc_error; nothing is thrown
 * across the ABI.  lqmpc_last_error() gives a thread-local message.  Per instance,
 * status[b] is 0 converged, 1 iteration cap reached, 2 non-finite data; iters[b] counts the KKT-system
 * factorisations spent on instance b (interior-point iterations + active-set iterations).  The QP is always
 * feasible and strictly convex (R > 0, non-empty box), so "infeasible" cannot occur.
 *
 * Threading: a handle is bound to one device and one stream and is not thread-safe;
 * distinct handles may be used from distinct threads.
 */
#ifndef LQMPC_H
#define LQMPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lqmpc_handle lqmpc_handle;

#define LQMPC_MAX_BOX_CENTRE 1.0   /* largest |lb_k + ub_k| / 2 the solve / rollout / max-V_N / sweep calls accept */

enum lqmpc_error {
    LQMPC_OK = 0,
    LQMPC_ERR_BAD_ARG = -1,      /* NULL pointer, non-positive size, empty box, box centre over the limit, dims over the limits */
    LQMPC_ERR_HIP = -2,          /* a HIP runtime call failed (message in lqmpc_last_error) */
    LQMPC_ERR_NO_DEVICE = -3,    /* no usable GPU */
    LQMPC_ERR_ALLOC = -4,        /* device or host allocation failed */
    LQMPC_ERR_UNSUPPORTED = -5   /* requested kernel variant not built for these dims */
};

/* Which kernel family runs the batch. */
enum lqmpc_kernel {
    LQMPC_KERNEL_AUTO = 0,        /* register-resident specialisation when built for (nx,nu,N); else the 16-lane-row kernel
                                     compiled at run time where options.jit allows it (nx <= 8, nu <= 4, N*nu <= 48; with
                                     jit = 2 also 9 <= nx <= 16, nu <= 4, N*nu <= 32); else the workgroup kernel when it
                                     applies; else generic */
    LQMPC_KERNEL_GENERIC = 1,     /* any dims up to the limits; one instance per lane, workspace in HBM */
    LQMPC_KERNEL_SPECIALIZED = 2, /* fail with LQMPC_ERR_UNSUPPORTED if no specialisation exists */
    LQMPC_KERNEL_WORKGROUP = 3    /* one instance per 256-thread workgroup, matrices in LDS (32 < N*nu <= 128, nx <= 16,
                                     nu <= LQMPC_MAX_NU, LDS image within 160 KiB); LQMPC_ERR_UNSUPPORTED otherwise */
};

/* ABI note (library 0.2.0): the struct starts with its own size.  lqmpc_default_options / lqmpc_get_options fill it in;
 * lqmpc_set_options rejects a struct whose struct_size is not the library's sizeof(lqmpc_options) -- a caller built against another
 * version of this header gets LQMPC_ERR_BAD_ARG instead of the library reading past its struct.  Always start from
 * lqmpc_default_options() or lqmpc_get_options(). */
typedef struct lqmpc_options {
    uint32_t struct_size; /* sizeof(lqmpc_options) of the header the caller was built against */
    uint32_t reserved;    /* 0 */
    double eps;        /* relative tolerance on complementarity gap and dual residual (default 1e-12) */
    double tau;        /* fraction-to-the-boundary of the interior-point step (default 0.999) */
    double z0_scale;   /* initial multipliers = z0_scale * |q|_inf (default 0.1) */
    int32_t max_iter;  /* interior-point iteration cap per QP; also caps the <= 8 active-set warm-start iterations of the packed
                          kernel (default 50) */
    int32_t polish;    /* 1: finish with an exact solve on the identified active set (default 1) */
    int32_t kernel;    /* enum lqmpc_kernel (default AUTO) */
    int32_t presolve;  /* unconstrained-minimiser shortcut: the minimiser v = G x + v_r (G = -P^-1 Fq, built once
                          per instance) is tested against the box before any iteration; a QP whose minimiser is
                          interior is finished there, exactly.  -1 auto (= on), 0 off, 1 on.  Specialised kernels only; the generic kernel ignores it.  (default -1) */
    int32_t order;     /* processing order of a rollout batch.  1: a probe launch computes a difficulty key per instance
                          (largest stage gradient of the free response over the horizon, in units of what one input
                          can counter), the batch is bucket-sorted by its logarithm and the rollout walks it hardest-first, so the
                          instances that share a wavefront leave the constrained regime together; results are written
                          back to their original positions and do not depend on the order.  0: natural order.
                          -1 auto (1 for specialised rollouts with presolve, T >= 4 and a batch large enough to pay for the probe: 8192 instances in the 16-lane-row layout, 1024 in the packed one).  (default -1) */
    int32_t warm_start; /* primal-dual active-set warm start: before the interior-point loop, the QP is solved exactly on
                          the face guessed from the unconstrained minimiser (rows outside the box sit on their bound)
                          and the guess is corrected from the KKT signs, up to 8 times; a fixed point is the exact
                          optimum, otherwise the interior-point loop runs.  -1 auto (= presolve), 0 off, 1 on.
                          Specialised kernels only.  (default -1) */
    /* ---- layout / tuning selectors (the tests force every path through these; defaults are the measured best) ---- */
    int32_t layout;     /* which specialised family serves a shape that has both: -1 auto (lqmpc_api.hip: make_plan), 0 the
                          packed register-resident kernel (and its two-tier launch for sorted rollouts), 1 the 16-lane-row
                          kernel.  (default -1) */
    int32_t r16_maxit;  /* active-set iterations the 16-lane-row kernel spends on one QP before it hands the instance back to
                          the packed kernel's interior-point path (second launch over a device-side list); 0 hands every
                          constrained QP back.  In [0, 64].  (default 12) */
    int32_t r16_build;  /* build of the 16-lane-row kernel: -1 auto (the one-wave latency build up to 4 096 instances, the
                          two-waves throughput build above), 0 throughput build, 1 latency build.  (default -1) */
    int32_t nwide;      /* packed family, sorted rollouts: how many of the hardest instances get the 16-lane-row layout in
                          the two-tier launch; -1 auto (min(Bsz/8, 4096)), 0 none.  (default -1) */
    int32_t jit;        /* shapes (nx, nu, N) without a prebuilt instantiation: compile the 16-lane-row kernel for them at run time
                          (hiprtc; nx <= 8, nu <= 4, N*nu <= 48; about two seconds per shape and entry point on first use, then
                          cached) instead of falling back to the generic kernel.  -1 auto (= on), 0 off, 1 on, 2 as 1 and also
                          the wide-state shapes 9 <= nx <= 16, nu <= 4, N*nu <= 32 (a 12-state or 16-state model with a short
                          horizon: otherwise on the generic kernel; 10 - 50 s of compile per shape on first use).  Opt-in: the default
                          routing of those shapes is unchanged.  (default -1) */
    int32_t ctl_wg;     /* prepared controllers (lqmpc_controller_*) on the workgroup kernel's shapes: 0 every step is
                          lqmpc_solve_batch_dev (pass-through), 1 a controller created while this is set keeps one record per
                          instance there as well (kernel AUTO or WORKGROUP, presolve and warm start not switched off).  Opt-in
                          because of the memory: about 166 KB per instance at (8,4,30).  (default 0; the slot was reserved2) */
} lqmpc_options;

/* Limits of this build. */
#define LQMPC_MAX_NX 16
#define LQMPC_MAX_NU 8
#define LQMPC_MAX_N  64
#define LQMPC_MAX_NVAR 128   /* n = N*nu */

const char *lqmpc_version(void);
const char *lqmpc_last_error(void);
/* Number of GPUs the HIP runtime sees (0 if none; never fails). */
int lqmpc_device_count(void);

/* Handle life cycle.  lqmpc_create makes its own stream; lqmpc_create_on_stream borrows a
 * hipStream_t (passed as void*, may be NULL for the default stream). */
int lqmpc_create(int device, lqmpc_handle **out);
int lqmpc_create_on_stream(int device, void *hip_stream, lqmpc_handle **out);
int lqmpc_destroy(lqmpc_handle *h);
int lqmpc_sync(lqmpc_handle *h);

void lqmpc_default_options(lqmpc_options *opt);
int lqmpc_set_options(lqmpc_handle *h, const lqmpc_options *opt);
int lqmpc_get_options(const lqmpc_handle *h, lqmpc_options *opt);

/* Run-time compiled kernels (options.jit).  lqmpc_jit_cache_dir: directory where code objects are kept across processes (NULL or
 * "" = in memory only; process-wide).  lqmpc_jit_compile: compile (or find in that directory) every kernel of one shape now -- it needs
 * no GPU, so a build machine can fill the cache; returns the number of code objects available (5) or a negative lqmpc_error, with the
 * compiler's message in `log` if given.  It serves the whole domain of options.jit = 2, the wide-state shapes included. */
int lqmpc_jit_cache_dir(const char *dir);
int lqmpc_jit_compile(int nx, int nu, int N, char *log, int log_len);
/* ... and the two on-chip kernels of lqmpc_bounds_batch for a shape (returns 2). */
int lqmpc_jit_compile_bounds(int nx, int nu, int N, char *log, int log_len);

/* 1 if a register-resident specialisation for (nx,nu,N) is compiled in, else 0. */
int lqmpc_has_specialization(int nx, int nu, int N);
/* Name of the kernel the last batched call on this handle launched (for logs/profiles). */
const char *lqmpc_last_kernel(const lqmpc_handle *h);

/* Pre-size the handle's device scratch so later calls do no allocation (e.g. before timing). */
int lqmpc_reserve(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T);

/* ---- LQ_MPC_Controller.solve, batched (utils_class.py:48-91) ----
 * Accuracy (the solve, plan, controller-step and rollout calls): with status 0 the inputs are the optimum of the box QP on its optimal
 * face, and per instance  |u - u*| <= max(1e-10, c eps cond_2(H)) max(|u*|, h),  |V_N - V_N*| <= max(1e-11, c eps cond_2(H)) V_N*,
 * eps = 2^-52, H the condensed Hessian of the instance, h the half-width of the box, c = 16 (V_N: 32) -- sixteen times what the fp64
 * CPU oracle leaves against a long-double reference.  Where an active-set iteration runs on the dual side of the 16-lane-row and
 * workgroup kernels (free rows = unconstrained minimiser minus a correction through the explicit inverse W) the constant for u is 1e3.
 * Tested for cond_2(H) <= 1e8 (unstable models, integrator chains, cheap control with nearly collinear inputs:
 * tests/test_gpu_qp_hard.py); on well-conditioned models the floors apply, which is the "1e-10 / 1e-11" of the other tests.
 * A set-up whose 4 x 4 stage matrix R + B'Sg B cannot be inverted to |I - X Re|_F < 2^-32 (3 or 4 inputs, cond_2(R_e) of that stage
 * matrix beyond about 1e6) hands the instance to the generic kernel, at the generic kernel's throughput. */
int lqmpc_solve_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz,
                      const double *A, const double *B,
                      const double *Q, const double *R, const double *P,
                      const double *lb, const double *ub,
                      const double *x0, const double *x_ref, const double *u_ref,
                      double *u0, double *VN, int32_t *status, int32_t *iters);
int lqmpc_solve_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz,
                          const double *dA, const double *dB,
                          const double *Q, const double *R, const double *P,
                          const double *lb, const double *ub,
                          const double *dx0, const double *x_ref, const double *u_ref,
                          double *du0, double *dVN, int32_t *dstatus, int32_t *diters);

/* ---- the same solve, returning the whole optimal plan: the reference's decision variable LQ_MPC_Controller.u (utils_class.py:46),
 *      read there as controller.u.value after solve ----
 * Instance-minor, as the rollout's U / X:
 *     Uplan[(k*N + i)*Bsz + b]     = u_i[k]   i = 0..N-1   the optimal input sequence
 *     Xplan[(a*(N+1) + i)*Bsz + b] = x_i[a]   i = 0..N     x_0 the given state, x_{i+1} = A x_i + B u_i on the MODEL
 * Uplan is required (NULL: LQMPC_ERR_BAD_ARG before anything is enqueued); Xplan, status, iters may be NULL; VN stays required.
 * Contract: u0, VN, status, iters are bit for bit what lqmpc_solve_batch[_dev] returns for the same handle, options and data;
 * Uplan[:, 0, :] is bit for bit u0; Xplan[:, 0, :] is bit for bit x0; every entry of Uplan lies in [lb, ub] (the 16-lane-row and
 * workgroup kernels form a bound as centre +- half-width, for u0 as well: exactly lb / ub under a symmetric box, lb / ub to the
 * rounding of that sum, an ulp or two, under any other).  For an instance with
 * status 2 (non-finite data) the plan rows are unspecified, as u0 is.  Enqueued on the stream like lqmpc_solve_batch[_dev]: _dev
 * returns at once.  Every kernel family writes the plan where it writes u0, from the solution vector it already holds, and the states
 * from the roll of the model that gives V_N: no further arithmetic, N nu + (N + 1) nx more doubles stored per instance. */
int lqmpc_solve_plan_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz,
                           const double *A, const double *B,
                           const double *Q, const double *R, const double *P,
                           const double *lb, const double *ub,
                           const double *x0, const double *x_ref, const double *u_ref,
                           double *u0, double *VN, double *Uplan, double *Xplan, int32_t *status, int32_t *iters);
int lqmpc_solve_plan_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz,
                               const double *dA, const double *dB,
                               const double *Q, const double *R, const double *P,
                               const double *lb, const double *ub,
                               const double *dx0, const double *x_ref, const double *u_ref,
                               double *du0, double *dVN, double *dUplan, double *dXplan, int32_t *dstatus, int32_t *diters);

/* ---- the same solve, and its derivatives with respect to the measured state: the local feedback law and the value gradient ----
 * The law of a box-constrained MPC is piecewise affine: inside the critical region of x0 it is u_0 = K_0 x0 + k_0.  Instance-minor:
 *     K0[(k*nx + a)*Bsz + b]              = d u_0[k] / d x0[a]        the gain of the local law (k_0 = u_0 - K_0 x0 is the caller's)
 *     dVdx[a*Bsz + b]                     = d V_N / d x0[a]           (V_N includes x0'Q x0)
 *     Kplan[((k*N + i)*nx + a)*Bsz + b]   = d u_i[k] / d x0[a]        the same for the whole plan, i = 0..N-1
 * K0 and dVdx are required (NULL: LQMPC_ERR_BAD_ARG before anything is enqueued); Kplan, Uplan, Xplan, status, iters may be NULL.
 * The call is lqmpc_solve_plan_batch_dev followed by one launch of lqmpc_sens_kernel on the same stream (a post-pass: no solver
 * kernel holds any of it); where Uplan, Xplan or status is NULL the plan call writes to buffers of the handle, grown as needed.
 * Contract: u0, VN, status, iters, Uplan, Xplan are bit for bit those of lqmpc_solve_plan_batch[_dev] on the same handle, options and
 * data, and lqmpc_last_kernel names the solve kernel.  The derivatives are those of the FACE THE RETURNED PLAN REPORTS: an entry of
 * Uplan is on a bound when it equals, bit for bit, lb_k, ub_k, c_k - h_k or c_k + h_k (the forms the plan contract above names; no
 * tolerance), the inputs on a bound do not move and the others are free.  On that face d Uplan / d x0 is the solution of an
 * equality-constrained LQ problem, computed by one backward Riccati sweep with a free mask per stage and one forward product, never
 * from an n x n matrix: rows of Kplan (and K0) that belong to an input on a bound are exactly 0.0, and Kplan[:, 0] is bit for bit K0.
 * References and the centre of the box enter only k_0, never the gain.  dVdx follows from the envelope theorem by one costate
 * recursion over Xplan and holds on every face.  At the border of two critical regions (a weakly active bound) the derivative is
 * one-sided and the call returns that of the face the plan reports.  With options.polish = 0 the plan need not touch its bounds
 * bit for bit: the gain is then that of the free face.  An instance with status 2 (non-finite data) gets NaN in K0, dVdx and Kplan. */
int lqmpc_solve_sens_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz,
                           const double *A, const double *B,
                           const double *Q, const double *R, const double *P,
                           const double *lb, const double *ub,
                           const double *x0, const double *x_ref, const double *u_ref,
                           double *u0, double *VN, double *K0, double *dVdx, double *Kplan, double *Uplan, double *Xplan,
                           int32_t *status, int32_t *iters);
int lqmpc_solve_sens_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz,
                               const double *dA, const double *dB,
                               const double *Q, const double *R, const double *P,
                               const double *lb, const double *ub,
                               const double *dx0, const double *x_ref, const double *u_ref,
                               double *du0, double *dVN, double *dK0, double *ddVdx, double *dKplan, double *dUplan, double *dXplan,
                               int32_t *dstatus, int32_t *diters);

/* ---- the gradient of a loss on (u_0, V_N) with respect to the model matrices of every instance ----
 * Given what a plan or sens call wrote (Uplan, Xplan, status; status may be NULL = all 0) and the cotangents gu0 = d loss / d u_0
 * (nu, Bsz) and gVN = d loss / d V_N (Bsz) (either may be NULL = zero, not both), instance-minor like A and B:
 *     gA[(a*nx + c)*Bsz + b]  = d loss / d A[a][c] of instance b
 *     gB[(a*nu + k)*Bsz + b]  = d loss / d B[a][k] of instance b
 *     gx0[a*Bsz + b]          = d loss / d x0[a]   (optional, NULL is fine; = K_0'gu0 + gVN dV_N/dx0 of lqmpc_solve_sens_batch)
 * gA and gB are required (NULL, or both cotangents NULL: LQMPC_ERR_BAD_ARG before anything is enqueued).  The call is the post-pass
 * alone -- one launch of lqmpc_grad_kernel on the handle's stream, no solve: the cotangents are only known at backward time -- so A, B,
 * the weights, the box and the references must be those of the call that wrote the plan; lqmpc_last_kernel is left naming the solve
 * kernel.  The gradient is that of the FACE THE PLAN REPORTS, by the rule of lqmpc_solve_sens_batch: an entry of Uplan is on a bound
 * when it equals, bit for bit, lb_k, ub_k, c_k - h_k or c_k + h_k (no tolerance), the inputs on a bound do not move and the others are
 * free.  On that face the gradient is the adjoint of an equality-constrained LQ problem: one backward Riccati sweep with a free mask
 * per stage, one forward roll of N steps, two costate recursions and 2N rank-1 updates, never an n x n matrix.  The gVN part follows
 * from the envelope theorem and holds on every face.  At the border of two critical regions the gradient is one-sided.  An instance
 * whose stage-0 inputs all sit on bounds and whose gVN is 0 gets exact 0.0 everywhere; an instance with status 2 gets NaN in gA, gB
 * and gx0.  A shape whose LDS image would not fit 160 KiB is refused with LQMPC_ERR_UNSUPPORTED (none within the build limits). */
int lqmpc_model_grad_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz,
                           const double *A, const double *B,
                           const double *Q, const double *R, const double *P,
                           const double *lb, const double *ub,
                           const double *x_ref, const double *u_ref,
                           const double *Uplan, const double *Xplan, const int32_t *status,
                           const double *gu0, const double *gVN,
                           double *gA, double *gB, double *gx0);
int lqmpc_model_grad_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz,
                               const double *dA, const double *dB,
                               const double *Q, const double *R, const double *P,
                               const double *lb, const double *ub,
                               const double *x_ref, const double *u_ref,
                               const double *dUplan, const double *dXplan, const int32_t *dstatus,
                               const double *dgu0, const double *dgVN,
                               double *dgA, double *dgB, double *dgx0);

/* ---- the gradient of a loss on (u_0, V_N) with respect to the data the batch shares: weights, references, box ----
 * Inputs as lqmpc_model_grad_batch: what a plan or sens call wrote (Uplan, Xplan, status; status may be NULL = all 0) and the
 * cotangents gu0 (nu, Bsz) and gVN (Bsz) (either may be NULL = zero, not both).  With e_i = x_i - x_ref[:, i-1], d_i = u_i - u_ref[:, i],
 * the adjoint plan (ut, xt) and the costates l, lt of the model gradient, r_i = 2 R d_i + B'l_{i+1}, rt_i = 2 R ut_i + B'lt_{i+1}:
 *     gQ    = gVN x0 x0' + sum_{i=1}^{N-1} (gVN e_i e_i' - xt_i e_i' - e_i xt_i')     gP = the same term at i = N
 *     gR    = sum_{i=0}^{N-1} (gVN d_i d_i' - ut_i d_i' - d_i ut_i')
 *     gxref[:, i-1] = 2 Q (xt_i - gVN e_i)  (P at i = N)                               guref[:, i] = 2 R (ut_i - gVN d_i)
 *     gub[k] = sum over the entries (i, k) of the plan on the upper bound of gVN r_i[k] - rt_i[k] + (i == 0 ? gu0[k] : 0); glb likewise
 * gQ, gR, gP are the derivatives with the entries of the matrix taken as independent; they are symmetric, and a symmetric change dQ
 * changes the loss by <gQ, dQ>.  The face is the one the plan reports, by the rule of lqmpc_solve_sens_batch (an entry equal, bit
 * for bit, to lb_k or c_k - h_k is on the lower bound, to ub_k or c_k + h_k on the upper); the gVN parts hold on every face.
 * reduce == 0: every output per instance, instance-minor -- gQ[(a*nx + c)*Bsz + b], gR[(k*nu + l)*Bsz + b], gP like gQ, glb[k*Bsz + b],
 *   gub likewise, gxref[(a*N + i)*Bsz + b], guref[(k*N + i)*Bsz + b]; an instance with status 2 gets NaN in all of them; nskipped
 *   is not written.
 * reduce != 0: every output in the shape of its parameter, row-major (gQ nx x nx, ..., gxref nx x N), the SUM over the batch, formed
 *   on chip in a fixed order without atomics: the same data give the same bits.  An instance with status 2 adds nothing and is
 *   counted in *nskipped (may be NULL).
 * Any output may be NULL, not all (all NULL, or both cotangents NULL: LQMPC_ERR_BAD_ARG before anything is enqueued).  The call is the
 * post-pass alone -- one launch of lqmpc_cost_grad_kernel on the handle's stream (with reduce a second, small one), no solve -- so A,
 * B, the weights, the box and the references must be those of the call that wrote the plan; lqmpc_last_kernel is left naming the
 * solve kernel.  An instance whose stage-0 inputs all sit on bounds and whose gVN is 0 gets exact 0.0 in gQ, gR, gP, gxref, guref and
 * gu0[k] in glb[k] + gub[k].  A shape whose LDS image would not fit 160 KiB is refused with LQMPC_ERR_UNSUPPORTED: none within the
 * build limits with reduce == 0; with reduce != 0 the 48 shapes DESIGN.md section 4.12 lists (nx >= 14 with long horizons).
 * lqmpc_cost_grad_blocks: the number of wavefronts the kernel is launched with, a function of the shape and Bsz only (0: bad dims). */
int lqmpc_cost_grad_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz,
                          const double *A, const double *B,
                          const double *Q, const double *R, const double *P,
                          const double *lb, const double *ub,
                          const double *x_ref, const double *u_ref,
                          const double *Uplan, const double *Xplan, const int32_t *status,
                          const double *gu0, const double *gVN, int reduce,
                          double *gQ, double *gR, double *gP, double *glb, double *gub, double *gxref, double *guref,
                          int64_t *nskipped);
int lqmpc_cost_grad_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz,
                              const double *dA, const double *dB,
                              const double *Q, const double *R, const double *P,
                              const double *lb, const double *ub,
                              const double *x_ref, const double *u_ref,
                              const double *dUplan, const double *dXplan, const int32_t *dstatus,
                              const double *dgu0, const double *dgVN, int reduce,
                              double *dgQ, double *dgR, double *dgP, double *dglb, double *dgub, double *dgxref, double *dguref,
                              int64_t *dnskipped);
int64_t lqmpc_cost_grad_blocks(int nx, int nu, int N, int64_t Bsz, int reduce);

/* ---- the gradient of a loss on the whole plan -- every u_i, every x_i and V_N -- with respect to the model and the given state ----
 * Given what a plan or sens call wrote (Uplan, Xplan, status; status may be NULL = all 0) and the cotangents, laid out like what they
 * belong to:
 *     gUplan[(k*N + i)*Bsz + b]     = d loss / d u_i[k]   i = 0..N-1
 *     gXplan[(a*(N+1) + i)*Bsz + b] = d loss / d x_i[a]   i = 0..N     (row i = 0 acts on the given state and goes to gx0 as it is)
 *     gVN[b]                        = d loss / d V_N
 * any of them may be NULL = zero, not all three, the outputs are those of lqmpc_model_grad_batch, instance-minor like A and B:
 *     gA[(a*nx + c)*Bsz + b]  = d loss / d A[a][c] of instance b
 *     gB[(a*nu + k)*Bsz + b]  = d loss / d B[a][k] of instance b
 *     gx0[a*Bsz + b]          = d loss / d x0[a]
 * Any output may be NULL, not all; gA and gB are independent of each other.  All cotangents NULL, all outputs NULL, a NULL handle,
 * model or plan: LQMPC_ERR_BAD_ARG before anything is enqueued.  The call is the post-pass alone -- one launch of
 * lqmpc_plan_grad_kernel on the handle's stream, no solve: the cotangents are only known at backward time -- so A, B, the weights, the
 * box and the references must be those of the call that wrote the plan; lqmpc_last_kernel is left naming the solve kernel.
 * The gradient is that of the FACE THE PLAN REPORTS, by the rule of lqmpc_solve_sens_batch: an entry of Uplan is on a bound when it
 * equals, bit for bit, lb_k, ub_k, c_k - h_k or c_k + h_k (no tolerance), the inputs on a bound do not move and the others are free.
 * On that face the gradient is the adjoint of an equality-constrained LQ problem with a linear term at every stage: one backward
 * Riccati sweep with a free mask per stage and an affine part beside it, one forward roll of N steps, two costate recursions and 2N
 * rank-1 updates, never an n x n matrix.  The gVN part follows from the envelope theorem and holds on every face.  At the border of
 * two critical regions (a weakly active bound) the gradient is one-sided: the call returns that of the face the plan reports.
 * An entry of gUplan that belongs to an input on a bound changes no bit of any output, whatever it holds.  An instance whose
 * cotangents are all 0.0 gets exact 0.0 everywhere; an instance with status 2 gets NaN in gA, gB and gx0.  With gUplan zero behind
 * stage 0 and gXplan NULL the outputs are those of lqmpc_model_grad_batch to rounding.  A shape whose LDS image would not fit 160 KiB
 * is refused with LQMPC_ERR_UNSUPPORTED before anything is enqueued (none within the build limits: the largest, (16, 2, 64), takes
 * 153 568 bytes). */
int lqmpc_plan_grad_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz,
                          const double *A, const double *B,
                          const double *Q, const double *R, const double *P,
                          const double *lb, const double *ub,
                          const double *x_ref, const double *u_ref,
                          const double *Uplan, const double *Xplan, const int32_t *status,
                          const double *gUplan, const double *gXplan, const double *gVN,
                          double *gA, double *gB, double *gx0);
int lqmpc_plan_grad_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz,
                              const double *dA, const double *dB,
                              const double *Q, const double *R, const double *P,
                              const double *lb, const double *ub,
                              const double *x_ref, const double *u_ref,
                              const double *dUplan, const double *dXplan, const int32_t *dstatus,
                              const double *dgUplan, const double *dgXplan, const double *dgVN,
                              double *dgA, double *dgB, double *dgx0);

/* ---- LQ_MPC_Simulator.simulate, batched (utils_class.py:245-285) ----
 * The model (A,B) drives the QP, the plant (A_true,B_true) drives the state.
 * true_per_instance == 0: A_true/B_true are single HOST matrices shared by the batch
 * (the reference's usage, utils_class.py:830-832); != 0: SoA arrays like A/B (host for the
 * host flavour, device for the _dev flavour).  X, U, status, iters may be NULL. */
int lqmpc_rollout_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T,
                        const double *A, const double *B,
                        const double *Q, const double *R, const double *P,
                        const double *lb, const double *ub, const double *x0,
                        const double *A_true, const double *B_true, int true_per_instance,
                        const double *x_ref, const double *u_ref,
                        double *JT, double *X, double *U, int32_t *status, int32_t *iters);
int lqmpc_rollout_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T,
                            const double *dA, const double *dB,
                            const double *Q, const double *R, const double *P,
                            const double *lb, const double *ub, const double *dx0,
                            const double *A_true, const double *B_true, int true_per_instance,
                            const double *x_ref, const double *u_ref,
                            double *dJT, double *dX, double *dU, int32_t *dstatus, int32_t *diters);

/* ---- the same closed loop, leaving a tape: the whole plan of every step ----
 * Arguments as lqmpc_rollout_batch[_dev], plus
 *     Utape[t*(nu*N*Bsz) + (k*N + i)*Bsz + b] = u_i[k] of the plan solved at step t   (required)
 *     status_tape[t*Bsz + b]                  = the status of that solve              (may be NULL)
 * so slice t of Utape is a valid Uplan for every post-pass call above.  X, U, status, iters may be NULL.
 * THIS IS NOT THE FAST ROLLOUT.  Per step, on the handle's stream: the path of lqmpc_solve_plan_batch_dev on x_t, its plan written
 * straight into slice t, then one launch of lqmpc_plant_step_kernel (one lane per instance): x_{t+1} = A_true x_t + B_true u_0, the
 * cost in the order of the reference (x_0'Q x_0 first, then x_{t+1}'Q x_{t+1} + u_0'R u_0 per step), row t + 1 of X, row t of U, and
 * x_{t+1} into one of two (nx, Bsz) buffers of the handle for the next solve.  That is 2 T launches (more where a solve hands
 * instances back) against the one or two of lqmpc_rollout_batch_dev: the price of the tape (DESIGN.md section 4.14 has the figures).
 * Contract: U[:, t] is bit for bit Utape[t][:, 0]; slice t obeys the plan contract of lqmpc_solve_plan_batch, its forms of a bound
 * included; JT, X and U agree with lqmpc_rollout_batch[_dev] within the accuracy contract stated at lqmpc_solve_batch, not bit for
 * bit (the rollout kernels warm-start and sum in another order); status[b] is the largest status over the steps, iters[b] the sum.
 * _dev returns at once.  NULL handle, model, x0, JT, plant or Utape, T outside [1, 100000]: LQMPC_ERR_BAD_ARG before anything is
 * enqueued. */
int lqmpc_rollout_tape_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T,
                             const double *A, const double *B,
                             const double *Q, const double *R, const double *P,
                             const double *lb, const double *ub, const double *x0,
                             const double *A_true, const double *B_true, int true_per_instance,
                             const double *x_ref, const double *u_ref,
                             double *JT, double *X, double *U, int32_t *status, int32_t *iters,
                             double *Utape, int32_t *status_tape);
int lqmpc_rollout_tape_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T,
                                 const double *dA, const double *dB,
                                 const double *Q, const double *R, const double *P,
                                 const double *lb, const double *ub, const double *dx0,
                                 const double *A_true, const double *B_true, int true_per_instance,
                                 const double *x_ref, const double *u_ref,
                                 double *dJT, double *dX, double *dU, int32_t *dstatus, int32_t *diters,
                                 double *dUtape, int32_t *dstatus_tape);

/* ---- the gradient of a loss on the closed loop -- J_T, every x_t and every u_t -- with respect to the model, the plant and x_0 ----
 * Given what lqmpc_rollout_tape_batch wrote (X, Utape, status_tape; status_tape may be NULL = all 0) and the cotangents
 *     gJT[b] = d loss / d J_T     gX[(a*(T+1) + t)*Bsz + b] = d loss / d x_t[a]     gU[(k*T + t)*Bsz + b] = d loss / d u_t[k]
 * (any may be NULL = zero, not all), instance-minor:
 *     gA[(a*nx + c)*Bsz + b], gB[(a*nu + k)*Bsz + b]            = d loss / d the MODEL of instance b (it drives every QP)
 *     gA_true[(a*nx + c)*Bsz + b], gB_true[(a*nu + k)*Bsz + b]  = d loss / d the PLANT of instance b: always per instance, a caller
 *                                                                 with a shared plant (true_per_instance == 0) sums them
 *     gx0[a*Bsz + b]                                            = d loss / d x_0[a]
 * Any output may be NULL, not all.  The call is one launch of lqmpc_rollout_grad_kernel on the handle's stream and runs no solve; the
 * data must be those of the call that wrote the tape.  Per instance, with gam = gJT, the tape is walked backwards with the plant's costate:
 *     l_T = gX_T + 2 gam Q x_T;   t = T-1 .. 0:   w_t = gU_t + 2 gam R u_t + B_true'l_{t+1}
 *         (gA_t, gB_t, gx_t) = the gradient of lqmpc_model_grad_batch at step t for gu0 = w_t, gVN = 0, on the face slice t reports
 *         gA += gA_t, gB += gB_t, gA_true += l_{t+1} x_t', gB_true += l_{t+1} u_t',   l_t = gX_t + 2 gam Q x_t + A_true'l_{t+1} + gx_t
 *     gx0 = l_0
 * The face of a step is the one its slice reports, by the rule of lqmpc_solve_sens_batch (bit for bit lb_k, ub_k, c_k - h_k or
 * c_k + h_k; no tolerance); the states of a plan are re-rolled on the model from x_t and the slice.  At the border of two critical
 * regions the gradient is one-sided.  A step whose stage-0 inputs all sit on bounds adds exactly nothing from its QP; an instance
 * whose cotangents are all 0.0 gets exact 0.0 everywhere; an instance with status 2 at any step gets NaN in every output.  NULL
 * handle, model, plant, X or Utape, all cotangents NULL, all outputs NULL, T outside [1, 100000]: LQMPC_ERR_BAD_ARG; a shape whose LDS
 * image would not fit 160 KiB: LQMPC_ERR_UNSUPPORTED (the image is larger than that of lqmpc_plan_grad_kernel: the shapes DESIGN.md
 * section 4.14 lists); both before anything is enqueued. */
int lqmpc_rollout_grad_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T,
                             const double *A, const double *B,
                             const double *Q, const double *R, const double *P,
                             const double *lb, const double *ub,
                             const double *A_true, const double *B_true, int true_per_instance,
                             const double *x_ref, const double *u_ref,
                             const double *X, const double *Utape, const int32_t *status_tape,
                             const double *gJT, const double *gX, const double *gU,
                             double *gA, double *gB, double *gx0, double *gA_true, double *gB_true);
int lqmpc_rollout_grad_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T,
                                 const double *dA, const double *dB,
                                 const double *Q, const double *R, const double *P,
                                 const double *lb, const double *ub,
                                 const double *A_true, const double *B_true, int true_per_instance,
                                 const double *x_ref, const double *u_ref,
                                 const double *dX, const double *dUtape, const int32_t *dstatus_tape,
                                 const double *dgJT, const double *dgX, const double *dgU,
                                 double *dgA, double *dgB, double *dgx0, double *dgA_true, double *dgB_true);

/* ---- the gradient of the same loss on the closed loop with respect to the data the batch shares: Q, R, P, lb, ub, x_ref, u_ref ----
 * Inputs as lqmpc_rollout_grad_batch[_dev]: what lqmpc_rollout_tape_batch wrote (X, Utape, status_tape; status_tape may be NULL = all
 * 0) and the cotangents gJT, gX, gU (any may be NULL = zero, not all).  Outputs and `reduce` as lqmpc_cost_grad_batch[_dev]:
 *     reduce == 0, per instance, instance-minor:  gQ[(a*nx + c)*Bsz + b], gR[(k*nu + l)*Bsz + b], gP[(a*nx + c)*Bsz + b],
 *         glb[k*Bsz + b], gub[k*Bsz + b], gxref[(a*N + i)*Bsz + b], guref[(k*N + i)*Bsz + b]
 *     reduce != 0, the sum over the batch, every output in the shape of its parameter (row-major); *nskipped takes the number of
 *         instances with status 2 at any step, which add 0.0.  The sum is formed on chip in a fixed order without atomics: the same
 *         data give the same bits.
 * Any output may be NULL, not all.  The call is one launch of lqmpc_rollout_cost_grad_kernel on the handle's stream (with reduce, a
 * second small launch that adds one vector of partial sums per wavefront, kept in a block the handle owns) and runs no solve; the
 * data must be those of the call that wrote the tape.  Per instance, with gam = gJT, the tape is walked backwards with the plant's costate:
 *     l_T = gX_T + 2 gam Q x_T;   t = T-1 .. 0:   w_t = gU_t + 2 gam R u_t + B_true'l_{t+1}
 *         (gQ_t, gR_t, gP_t, glb_t, gub_t, gxref_t, guref_t) = the gradient of lqmpc_cost_grad_batch at step t for gu0 = w_t, gVN = 0,
 *                                                              on the face slice t reports, plan states re-rolled on the model from x_t
 *         gx_t = the gx0 of lqmpc_model_grad_batch for the same cotangents (the same adjoint plan)
 *         every output += its step-t term,   l_t = gX_t + 2 gam Q x_t + A_true'l_{t+1} + gx_t
 *     the direct part, because the one Q and R of the call also weigh J_T:  gQ += gam sum_{t=0}^{T} x_t x_t',  gR += gam sum_{t=0}^{T-1} u_t u_t'
 * With gVN = 0 the step-t terms are (xt, ut the adjoint plan, lt its costate, e_i = x_i - xref_{i-1}, d_i = u_i - uref_i):
 *     gQ_t = -sum_{i=1}^{N-1} (xt_i e_i' + e_i xt_i'),  gP_t the same term at i = N,   gR_t = -sum_i (ut_i d_i' + d_i ut_i')
 *     gxref_t[:, i-1] = 2 Q xt_i (P at i = N),   guref_t[:, i] = 2 R ut_i
 *     gub_t[k] = sum over the entries (i, k) on the upper bound of -rt_i[k] + (i == 0 ? w_t[k] : 0),  rt_i = 2 R ut_i + B'lt_{i+1};  glb_t likewise
 * gQ, gR and gP take the entries of the matrix as independent, as lqmpc_cost_grad_batch does: a caller who parametrises a symmetric
 * matrix contracts them with its own d Q.  The face rule is that of lqmpc_solve_sens_batch, bit for bit, no tolerance.  A step whose
 * stage-0 inputs all sit on bounds adds w_t[k] to glb[k] or gub[k] and exactly nothing else; cotangents that are all 0.0 give exact
 * 0.0 everywhere; per instance, an instance with status 2 at any step gets NaN in every output.
 * THE CONTROLLER'S WEIGHTS ONLY: a caller who wants the derivative in the weights the controller plans with, under fixed evaluation
 * weights, passes gJT = NULL and puts the evaluation cost into gX and gU (gX_t = 2 Q_eval x_t, gU_t = 2 R_eval u_t); there is no flag.
 * NULL handle, model, plant, X or Utape, all cotangents NULL, all outputs NULL, T outside [1, 100000]: LQMPC_ERR_BAD_ARG; a shape whose
 * LDS image would not fit 160 KiB: LQMPC_ERR_UNSUPPORTED (the shapes DESIGN.md section 4.15 lists); both before anything is enqueued. */
int lqmpc_rollout_cost_grad_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T,
                                  const double *A, const double *B,
                                  const double *Q, const double *R, const double *P,
                                  const double *lb, const double *ub,
                                  const double *A_true, const double *B_true, int true_per_instance,
                                  const double *x_ref, const double *u_ref,
                                  const double *X, const double *Utape, const int32_t *status_tape,
                                  const double *gJT, const double *gX, const double *gU, int reduce,
                                  double *gQ, double *gR, double *gP, double *glb, double *gub, double *gxref, double *guref,
                                  int64_t *nskipped);
int lqmpc_rollout_cost_grad_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T,
                                      const double *dA, const double *dB,
                                      const double *Q, const double *R, const double *P,
                                      const double *lb, const double *ub,
                                      const double *A_true, const double *B_true, int true_per_instance,
                                      const double *x_ref, const double *u_ref,
                                      const double *dX, const double *dUtape, const int32_t *dstatus_tape,
                                      const double *dgJT, const double *dgX, const double *dgU, int reduce,
                                      double *dgQ, double *dgR, double *dgP, double *dglb, double *dgub, double *dgxref,
                                      double *dguref, int64_t *dnskipped);

/* ---- polytopic input constraints: F_u u_i <= 1 for ANY matrix F_u (utils_class.py:81), not only the rows of a box ----
 * Per instance, with n = N nu and no 1/2 factor, as everywhere in this header:
 *     min  sum_{i=0}^{N-2} |x_{i+1} - xref_i|^2_Q + |x_N - xref_{N-1}|^2_P + sum_{i=0}^{N-1} |u_i - uref_i|^2_R
 *     s.t. x_{i+1} = A x_i + B u_i,   Fu u_i <= 1  (componentwise, i = 0..N-1);     u_0 = u*[:, 0],  V_N = cost* + x0'Q x0.
 * Fu is (m, nu), row-major, a HOST pointer shared by the batch and copied by the call, like Q, R, lb, ub.  u = 0 is strictly feasible
 * and R > 0, so the QP is feasible and strictly convex: "infeasible" cannot occur.  The polytope need not be bounded (one row
 * [[10.]] is a one-sided limit).  rho = max_j 1 / |Fu_j|_2, the distance of the farthest facet, stands where the box calls have the
 * half-width h.
 * METHOD: Goldfarb-Idnani, the dual active-set method from the unconstrained minimiser, on the rows normalised to unit length; exact and
 * finite, and it copes with dependent active rows (m > nu).  One instance per wavefront, one launch: lqmpc_last_kernel names
 * lqmpc_poly_solve_kernel / lqmpc_poly_rollout_kernel.  No options but eps are read: a row counts as satisfied within eps * rho.
 * DOMAIN: nx <= 16, nu <= LQMPC_MAX_NU, N <= LQMPC_MAX_N, n = N nu <= 64, 1 <= m <= 16, LDS image within 160 KiB (every shape of the
 * domain fits).  Outside: LQMPC_ERR_UNSUPPORTED with a message that names the domain; there is no fall-back to another kernel family.
 * LQMPC_ERR_BAD_ARG: m < 1, a NULL Fu, a row of Fu that is all zero or holds a non-finite entry, max_iter < 0, the usual NULL or size
 * errors.  Every refusal happens before anything is enqueued, from the arguments alone.
 * max_iter caps the passes (adds + drops) of one solve; 0 = 10 n + 20 (measured: at most 193 at n = 64 with a 16-gon, 43 at (4,2,10) with an octagon).  No loop of the
 * kernel depends on the data for its termination.
 * OUTPUTS of solve, instance-minor; u0 and VN are required, the others may be NULL, and leaving one out leaves the others bit for bit:
 *     u0[k*Bsz + b], VN[b];  Uplan[(k*N + i)*Bsz + b] = u_i[k] (Uplan[:, 0] is u0 bit for bit);  Xplan[(a*(N+1) + i)*Bsz + b] = x_i[a],
 *     the model's states under that plan (Xplan[:, 0] is x0 bit for bit; V_N is the cost of this roll);
 *     lam[(j*N + i)*Bsz + b] >= 0, the multiplier of row j at stage i of the rows AS GIVEN, of the Lagrangian
 *     V(U) + sum lam_ij (Fu_j u_i - 1):  2 (H U + g) + C'lam = 0 with C = I_N (x) Fu.  Where active rows depend on each other (a vertex
 *     with more than nu rows through it) the multipliers are one valid choice; the plan is unique.
 *     status[b]: 0 optimal; 1 max_iter reached, or no step left -- the outputs are the last iterate of a DUAL method, which may
 *     violate rows; 2 non-finite data (the outputs of that instance are not numbers; the other instances are untouched).
 *     iters[b] = adds + drops.
 * ACCURACY, on models with cond_2(H) <= 53 (tests/test_gpu_poly.py, against a long-double reference): |U - U*| <= 1e-10 max(|U*|, rho)
 * for the whole plan, |V_N - V_N*| <= 1e-11 V_N*, every row Fu_j u_i - 1 <= 1e-10, lam >= 0 exactly and > 0 only on rows within 1e-10
 * of equality, stationarity within 1e-10 (|2H| max(|U|, rho) + |2g|).
 * rollout: T closed-loop steps in one launch from one set-up, as lqmpc_rollout_batch: u_t = u_0 of the QP at x_t (cold start, from a
 * pristine factor at every step that follows a step with an add, so rounding does not accumulate over T), x_{t+1} = A_true x_t +
 * B_true u_t, J_T = x_0'Q x_0 + sum_t (x_{t+1}'Q x_{t+1} + u_t'R u_t) summed in that order; X (nx, T+1, Bsz) and U (nu, T, Bsz) may be
 * NULL; status = the largest over the steps, iters = the sum; T in [1, 100000]; A_true / B_true shared (host) or per instance.
 * NOT HERE (the prepared controller is lqmpc_poly_controller_* below): the sens / grad / tape calls, sweep, max_vn and the bound coefficients for a polytope; n > 64; a
 * per-instance Fu; state constraints; warm start across rollout steps. */
int lqmpc_solve_poly_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz,
                           const double *A, const double *B,
                           const double *Q, const double *R, const double *P,
                           const double *Fu, int m, const double *x0,
                           const double *x_ref, const double *u_ref, int max_iter,
                           double *u0, double *VN, double *Uplan, double *Xplan, double *lam,
                           int32_t *status, int32_t *iters);
int lqmpc_solve_poly_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz,
                               const double *dA, const double *dB,
                               const double *Q, const double *R, const double *P,
                               const double *Fu, int m, const double *dx0,
                               const double *x_ref, const double *u_ref, int max_iter,
                               double *du0, double *dVN, double *dUplan, double *dXplan, double *dlam,
                               int32_t *dstatus, int32_t *diters);
int lqmpc_rollout_poly_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T,
                             const double *A, const double *B,
                             const double *Q, const double *R, const double *P,
                             const double *Fu, int m, const double *x0,
                             const double *A_true, const double *B_true, int true_per_instance,
                             const double *x_ref, const double *u_ref, int max_iter,
                             double *JT, double *X, double *U, int32_t *status, int32_t *iters);
int lqmpc_rollout_poly_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T,
                                 const double *dA, const double *dB,
                                 const double *Q, const double *R, const double *P,
                                 const double *Fu, int m, const double *dx0,
                                 const double *A_true, const double *B_true, int true_per_instance,
                                 const double *x_ref, const double *u_ref, int max_iter,
                                 double *dJT, double *dX, double *dU, int32_t *dstatus, int32_t *diters);

/* ---- prepared controller for the polytope problem: factor once, then one polytope QP per instance and measured state ----
 * For a closed loop the caller owns (a torch plant, recorded data, hardware) whose input set is not a box: create runs the
 * per-instance set-up of lqmpc_solve_poly_batch once -- W_k = A^k B, the Riccati sums, G = 2H, its Cholesky factor, L^-1 -- and keeps
 * it in HBM; every step solves the QP at the states it is given from that, in ONE launch (lqmpc_poly_ctl_step_kernel), with no
 * host-to-device copy and no allocation.  None of the set-up depends on the state; only the linear term does.
 * A type of its own: the sens and grad calls of lqmpc_controller do not exist for a polytope.
 * CONTRACT: arguments, layouts, outputs, status and accuracy are those of lqmpc_solve_poly_batch / lqmpc_rollout_poly_batch above.
 * A, B as there (host; _dev: device), Q, R, P, Fu (m x nu), x_ref, u_ref HOST and copied by create; max_iter is fixed at create
 * (0 = 10 n + 20) and eps is the handle's option at create -- later lqmpc_set_options do not reach the controller.  The controller
 * keeps its OWN device copy of the shared block (Q, R, P, Fu, the references): the one-shot calls overwrite the handle's, so one-shot
 * calls and steps of several controllers may be mixed freely on one handle.  create waits for the stream: A and B are the caller's
 * again when it returns.
 * DOMAIN and refusals: those of lqmpc_solve_poly_batch, decided from the arguments before the handle is dereferenced or anything is
 * enqueued: N nu > 64, m > 16 or an LDS image over 160 KiB gives LQMPC_ERR_UNSUPPORTED with the domain in the message; m < 1, a
 * NULL Fu, a zero or non-finite row of Fu, max_iter < 0, a NULL handle, A, B, Q, R, P or out, Bsz < 1 give LQMPC_ERR_BAD_ARG.  step,
 * rollout and set_model refuse a NULL controller, a NULL required array (x, u0; x0, A_true, B_true, JT; A, B) and T outside
 * [1, 100000] with LQMPC_ERR_BAD_ARG before the controller is dereferenced.
 * LAYOUT: one record per instance, contiguous, [A (nx nx) | B (nx nu) | W_k, k < N (N nx nu) | Jp (n (n + 1) / 2)], Jp = L^-1 packed by
 * rows; the stride is rounded up to a multiple of 16 doubles, so records start on 128-byte lines and a wavefront reads its record
 * with consecutive lanes on consecutive addresses.  lqmpc_poly_controller_record_bytes(nx, nu, N) = 8 x stride is pure host
 * arithmetic (no handle): 2 560 bytes at (4,2,10), 27 008 at (16,1,64); a negative lqmpc_error outside nx <= 16, nu <= 8, N <= 64,
 * N nu <= 64.  bytes: the HBM the controller holds, Bsz records and the shared block.  The record's A and B are the controller's
 * copies of the models: it keeps no others.
 * BIT FOR BIT: every solve of the polytope kernels starts cold, from the pristine J = L^-T and an empty active set, and the step
 * runs the statements of the one-shot kernel on the record's values, which are the one-shot set-up's.  So step at x returns the
 * bits lqmpc_solve_poly_batch returns at x0 = x for the controller's models, weights, Fu and current references -- u0, VN, Uplan,
 * Xplan, lam, status, iters, and leaving an optional output out leaves the others bit for bit (here VN is optional too, as at
 * lqmpc_controller_step: the controller owns a buffer for it) -- and rollout returns the bits of
 * lqmpc_rollout_poly_batch.  A step leaves nothing behind: the records are read-only to step and rollout, so a step does not depend
 * on the steps or rollouts before it.
 * set_reference: new references for every later step and rollout, HOST, NULL = zeros.  No part of a record depends on the
 * references, so NO kernel runs: the two reference blocks of the controller's shared copy are rewritten by one copy on the handle's
 * stream, behind every step enqueued so far and in front of every later one.  The arrays are copied before the call returns.
 * set_model: new models for `count` instances, laid out and checked as lqmpc_controller_set_model states (instance-minor over the
 * update; idx == NULL needs count == Bsz; count == 0 does nothing; the host flavour checks idx for range and duplicates before
 * anything is enqueued and waits for the stream, the device flavour returns at once and its kernel skips an entry outside [0, Bsz)
 * whole, so a bad index never writes).  One launch of lqmpc_poly_ctl_factor_kernel over the update, workgroup j writing record
 * idx[j]; an unlisted record keeps every bit.
 * rollout: T closed-loop steps from the records in one launch (lqmpc_poly_ctl_rollout_kernel), read-only on the controller.  A
 * shared plant is a HOST pointer in both flavours, staged per call in memory the controller owns; a per-instance plant is a host
 * pointer in the host flavour and a device pointer in _dev.
 * Non-finite data: a non-finite model (at create or set_model) or state gives status 2 at that instance's steps and leaves the
 * other instances and the controller untouched.  kernel: "lqmpc_poly_ctl_step_kernel"; step, rollout and set_model set the
 * handle's lqmpc_last_kernel.  destroy: NULL is fine.
 * NOT HERE: warm start across steps (the dual method needs a dual-feasible start, and the cold start is what the bit-for-bit
 * equality rests on); the sens / grad / tape calls, MPCLayer, sweep, max_vn and the bound coefficients for a polytope; n > 64; a
 * per-instance Fu; state constraints. */
typedef struct lqmpc_poly_controller lqmpc_poly_controller;
int lqmpc_poly_controller_create(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz,
                                 const double *A, const double *B,
                                 const double *Q, const double *R, const double *P,
                                 const double *Fu, int m,
                                 const double *x_ref, const double *u_ref, int max_iter, lqmpc_poly_controller **out);
int lqmpc_poly_controller_create_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz,
                                     const double *dA, const double *dB,
                                     const double *Q, const double *R, const double *P,
                                     const double *Fu, int m,
                                     const double *x_ref, const double *u_ref, int max_iter, lqmpc_poly_controller **out);
int lqmpc_poly_controller_step(lqmpc_poly_controller *c, const double *x, double *u0, double *VN, double *Uplan, double *Xplan,
                               double *lam, int32_t *status, int32_t *iters);
int lqmpc_poly_controller_step_dev(lqmpc_poly_controller *c, const double *dx, double *du0, double *dVN, double *dUplan, double *dXplan,
                                   double *dlam, int32_t *dstatus, int32_t *diters);
int lqmpc_poly_controller_rollout(lqmpc_poly_controller *c, int T, const double *x0,
                                  const double *A_true, const double *B_true, int true_per_instance,
                                  double *JT, double *X, double *U, int32_t *status, int32_t *iters);
int lqmpc_poly_controller_rollout_dev(lqmpc_poly_controller *c, int T, const double *dx0,
                                      const double *A_true, const double *B_true, int true_per_instance,
                                      double *dJT, double *dX, double *dU, int32_t *dstatus, int32_t *diters);
int lqmpc_poly_controller_set_reference(lqmpc_poly_controller *c, const double *x_ref, const double *u_ref);
int lqmpc_poly_controller_set_model(lqmpc_poly_controller *c, int64_t count, const int32_t *idx, const double *A, const double *B);
int lqmpc_poly_controller_set_model_dev(lqmpc_poly_controller *c, int64_t count, const int32_t *didx, const double *dA, const double *dB);
int64_t lqmpc_poly_controller_record_bytes(int nx, int nu, int N);
int64_t lqmpc_poly_controller_bytes(const lqmpc_poly_controller *c);
const char *lqmpc_poly_controller_kernel(const lqmpc_poly_controller *c);
int lqmpc_poly_controller_destroy(lqmpc_poly_controller *c);

/* ---- M_V = max_k V_N(x0s[:,k]) per instance (utils_class.py:816-824, 899-907) ---- */
int lqmpc_max_vn_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int K,
                       const double *A, const double *B,
                       const double *Q, const double *R, const double *P,
                       const double *lb, const double *ub, const double *x0s,
                       const double *x_ref, const double *u_ref,
                       double *MV, int32_t *status, int32_t *iters);
int lqmpc_max_vn_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int K,
                           const double *dA, const double *dB,
                           const double *Q, const double *R, const double *P,
                           const double *lb, const double *ub, const double *x0s,
                           const double *x_ref, const double *u_ref,
                           double *dMV, int32_t *dstatus, int32_t *diters);

/* ---- one horizon of the reference's sweep in one call: M_V over the K states x0s AND the closed-loop cost J_T from x0,
 *      for the same (A,B,N) per instance (LQ_RDP_Behavior_Multiple.data_generation, utils_class.py:813-833, 896-916).
 *      One kernel launch (condensing once per instance) where the 16-lane-row layout serves the shape and the batch has
 *      at most 16 384 instances; otherwise lqmpc_max_vn_batch_dev followed by lqmpc_rollout_batch_dev on the stream.
 *      status = the worse of the two parts, iters = their sum. ---- */
int lqmpc_sweep_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T, int K,
                      const double *A, const double *B,
                      const double *Q, const double *R, const double *P,
                      const double *lb, const double *ub, const double *x0, const double *x0s,
                      const double *A_true, const double *B_true, int true_per_instance,
                      const double *x_ref, const double *u_ref,
                      double *JT, double *MV, int32_t *status, int32_t *iters);
int lqmpc_sweep_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz, int T, int K,
                          const double *dA, const double *dB,
                          const double *Q, const double *R, const double *P,
                          const double *lb, const double *ub, const double *dx0, const double *x0s,
                          const double *A_true, const double *B_true, int true_per_instance,
                          const double *x_ref, const double *u_ref,
                          double *dJT, double *dMV, int32_t *dstatus, int32_t *diters);

/* ---- the coefficients of the reference's performance bound, per system (utils_class.py:837-859, 920-942) ----
 * For every model (A, B) of the batch: K = control.dlqr(A, B, Q, R) (utils_class.py:840); with the gain -K, the error levels
 * e_A[b], e_B[b] and the energy bar M_V[b] (lqmpc_max_vn_batch's output; NULL = 0): xi, eta of
 * LQ_RDP_Calculator.energy_decreasing (utils_class.py:344-373) and eps = local_radius (utils.py:548-564); with the state x
 * (n_x, shared) and the parameter triple p (3, positive): alpha, beta of energy_bound (utils_class.py:308-342); and
 * bound = (alpha V_expert + beta) / (1 - xi - eta) (utils_class.py:858-859).  The box (lb, ub) stands for the rows of F_u
 * (e_k / ub_k, e_k / lb_k; bounds must be non-zero); bar_u and bar_d_u (two Gurobi QPs in utils.py:592-650) are closed forms for a box.
 * Outputs are per instance, any may be NULL: K[(k*nx + a)*Bsz + b] (dlqr's sign: u = -K x), alpha, beta, xi, eta, bound, eps [b],
 * aux[j*Bsz + b] for j < 8 = gamma, rho(A - BK), |A|_2, |B|_2, |Gamma|_2, |Phi|_2, lambda_min(hat H), |K|_2 (diagnostics),
 * status[b] = 0 ok, 1 the Riccati doubling did not settle in 64 steps, 2 not stabilisable / non-finite data (no gain; also a
 * doubling that settled on a gain with rho(A - BK) >= 1 - 1e-12: an unreachable eigenvalue on the unit circle), 3 the gain
 * and eps are valid but the bound's formulas leave the reals (gamma < 0 when rho(A - BK) + 0.4 > 1, utils.py:358-371).
 * Accuracy of the bound coefficients (tests/test_gpu_bounds_hard.py against a 50-digit reference, profiles/bounds_hard_spectra.json;
 * unstable, integrator, nilpotent, A = 0, weakly reachable, power-of-two scaled models, n = N nu up to 33, eps = 2^-52): the norms
 * |A|_2 |B|_2 |K|_2 |Gamma|_2 |Phi|_2 are within 3e-15 relative (bar max(m^2, 512) eps / 2, m the order of the Gram matrix) and
 * scale exactly with a power of two in the data; lambda_min(hat H) is accurate RELATIVE TO lambda_max(hat H), measured 4e-16
 * lambda_max (bar max(n^2, 512) eps lambda_max): at cond(hat H) = 1e7 that leaves nine digits of lambda_min itself, and no method
 * owes more; rho(A - BK) is within 5e-14 (on-chip kernels) and 1.1e-13 (workspace kernel, whose first 16 squarings accumulate in twice
 * the precision: a closed loop far from normal, the 9-state integrator chain, was off by up to 4e-11 without) of the spectral radius
 * of the returned gain's closed loop (bar max(10 e_numpy, 1e-12) absolute); the scalar formulas reproduce a host evaluation from aux and K to 2e-13 relative (bar 1e-12).
 * K is within max(10 e_scipy, 1e-12) |K|_max of the exact gain, e_scipy scipy's own error on the system, also under very cheap
 * control (R = 1e-6 I, B scaled by 2^20): the doubling iteration, which inverts H^-1 + B R^-1 B' explicitly and alone is off by
 * up to 4e-5 there, is followed by 24 Riccati steps P <- Q + A'P(A - BK) that restore K where the closed loop is fast.  Where the
 * doubling breaks down altogether (NaN) the steps start over from P = Q and run until the error left, estimated from the
 * contraction they show, is below 1e-14 |P|, 256 steps at most: a stabilisable system of that kind with rho(A - BK)^2 above about
 * 0.88 does not get there and keeps status 2.
 * Q, R (symmetric positive definite), lb, ub, x, p are HOST pointers in both flavours. */
int lqmpc_bounds_batch(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz,
                       const double *A, const double *B, const double *Q, const double *R,
                       const double *lb, const double *ub,
                       const double *e_A, const double *e_B, const double *MV,
                       const double *x, const double *p, double V_expert,
                       double *K, double *alpha, double *beta, double *xi, double *eta, double *bound, double *eps,
                       double *aux, int32_t *status);
int lqmpc_bounds_batch_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz,
                           const double *dA, const double *dB, const double *Q, const double *R,
                           const double *lb, const double *ub,
                           const double *de_A, const double *de_B, const double *dMV,
                           const double *x, const double *p, double V_expert,
                           double *dK, double *dalpha, double *dbeta, double *dxi, double *deta, double *dbound, double *deps,
                           double *daux, int32_t *dstatus);

/* ---- prepared batch controller: set up once, then one box QP per instance and call at a measured state ----
 * Every entry point above rebuilds the per-instance set-up (Riccati sweep, W = P^-1, the gain G of the unconstrained minimiser, P) in
 * every call, although only the state changes between the steps of a closed loop the caller owns.  A controller does that work once
 * and keeps it in HBM: one record per instance, [A | B | G | v_r | W | P] with W and P as packed lower triangles, padded to 256
 * bytes.  A step reads [A | B | G | v_r], forms v = G x + v_r and tests it against the box; W is read only by the instances that
 * have to iterate, P only when an iteration takes the primal side.  The active set a step ends on warm-starts the next step: shifted
 * by one stage, as in lqmpc_rollout_batch, when the new state is nearer to the model's prediction A x + B u_0 than to the previous
 * state x; as it is when the state did not advance (the same state asked again).  It never decides the answer.
 *
 * The controller takes a snapshot of the handle's options when it is created (eps, max_iter, r16_maxit, presolve, warm_start,
 * kernel, layout, jit, ctl_wg) and uses the handle's device, stream and scratch; later lqmpc_set_options calls do not reach it.  The record
 * kernels serve exactly the shapes and options for which lqmpc_solve_batch runs the 16-lane-row family (prebuilt or run-time
 * compiled).  With options.ctl_wg = 1 they also serve the shapes on which it runs the workgroup kernel (32 < N nu <= 128): there a
 * record is [A | B | G | v_r] and then W and P as the block images the kernel works on, a step is one launch of
 * lqmpc_wg_ctl_step_kernel, and W and P are read only by the instances that have to iterate.  Everywhere else the controller keeps
 * device copies of A and B and every step is lqmpc_solve_batch_dev on them, so the interface covers the library's whole domain.
 * The record kernels stop at nx <= 8: a controller created under options.jit = 2 on a wide-state shape (9 <= nx <= 16) is such a
 * pass-through, and its steps and rollouts run the run-time compiled 16-lane-row kernel of the shape instead of the generic one.
 * Destroy every controller BEFORE its handle.  Not thread-safe (as the handle).
 *
 * create: A, B per instance (instance-minor; host for _create, device for _create_dev), Q, R, P, lb, ub, x_ref, u_ref HOST (the
 *   references may be NULL).  Same argument checks and error codes as lqmpc_solve_batch.  Everything is copied: the caller may free
 *   or overwrite its arrays when the call returns (it waits for the stream).
 * step: x is nx x Bsz, instance-minor; u0 (nu x Bsz), VN, status, iters as lqmpc_solve_batch returns them; VN, status, iters may be
 *   NULL.  _dev: device pointers, enqueued on the handle's stream, returns at once.  A non-finite state gives status 2 for that
 *   instance and leaves no trace in the controller.  A step sets the handle's lqmpc_last_kernel.
 * step_plan: a step that also returns the whole plan, laid out and bound by the contract of lqmpc_solve_plan_batch: Uplan required,
 *   Xplan, VN, status, iters may be NULL; u0, VN, status, iters and the stored active set are bit for bit those of the plain step, and
 *   Xplan[:, 0, :] is x.  A pass-through controller runs lqmpc_solve_plan_batch_dev.
 * step_sens: a step_plan that also returns the derivatives with respect to x, laid out and bound by the contract of
 *   lqmpc_solve_sens_batch: K0 and dVdx required, Kplan, Uplan, Xplan, VN, status, iters may be NULL; u0, VN, status, iters, Uplan,
 *   Xplan and the stored active set are bit for bit those of step_plan, so the next plain step is the same after either.  It is
 *   lqmpc_controller_step_plan_dev followed by one launch of lqmpc_sens_kernel, which reads the controller's own copies of A and B
 *   (on workgroup records, which keep none, the heads of the records): record, workgroup and pass-through controllers alike, under
 *   every set_model and set_reference so far.
 * model_grad: lqmpc_model_grad_batch on the controller's own copies of A and B (on workgroup records the heads of the records) and its
 *   current references, for a plan one of its steps wrote since the last set_model / set_reference.  Read-only on the controller:
 *   the next step is bit for bit what it is without the call.
 * cost_grad: lqmpc_cost_grad_batch likewise, on the controller's models, weights, box and current references (those of the last
 *   set_reference).  Read-only on the controller as well.
 * plan_grad: lqmpc_plan_grad_batch likewise, on the controller's own copies of A and B (on workgroup records the heads of the
 *   records) and its current references: record, workgroup and pass-through controllers alike.  Read-only on the controller.
 * reset: forget the stored active sets (the next step starts cold).  bytes: HBM held by the controller.  kernel: the kernel its
 *   steps launch (contains "ctl"), or for a pass-through controller the kernel its last step ran.  destroy: NULL is fine.
 * set_reference: new references for every later step, x_ref (nx x N) and u_ref (nu x N) HOST, row-major, NULL = zeros -- for a loop
 *   that tracks a moving setpoint or slides its N-stage window along a trajectory.  Of a record only v_r depends on the references
 *   (v_r = -2 W g_ref - centre of the box, g_ref from an N-step costate recursion on the record's A and B): one launch rewrites it in
 *   place (lqmpc_ctl_retarget_kernel / lqmpc_wg_ctl_retarget_kernel), enqueued on the handle's stream, so it is ordered with the
 *   steps.  The arrays are copied before the call returns, and it does not wait for the stream.  A pass-through controller only
 *   stores them.  The stored active sets are kept (a warm-start hint that never decides the answer; reset forgets them).
 * set_model: new models for `count` instances, for a loop that re-estimates them: A (nx x nx x count) and B (nx x nu x count),
 *   instance-minor over the UPDATE -- A[(r*nx + c)*count + j], B[(r*nu + k)*count + j] belong to instance idx[j].  idx == NULL means
 *   instances 0..count-1 in order and needs count == Bsz (every model replaced); count == 0 does nothing and returns 0.  The entries
 *   of idx are distinct and lie in [0, Bsz): the host flavour checks that, before anything is enqueued (LQMPC_ERR_BAD_ARG); the
 *   device flavour cannot, and its kernels skip an entry outside [0, Bsz), so a bad index never writes outside the controller.  Every
 *   later step of a listed instance is the QP of the new (A, B) under the controller's Q, R, P, box and current references (those of
 *   the last set_reference); an unlisted instance keeps every bit of its record, its copies of A and B and its stored active set.
 *   The stored active sets of the listed instances are kept as well, as set_reference keeps them.  The records of the listed
 *   instances are rewritten by the factor launch of create, run over the update as a batch of `count` and redirected through idx;
 *   lqmpc_ctl_scatter_model_kernel refreshes the controller's copies of A and B (all a pass-through controller has).  Enqueued on
 *   the handle's stream: behind earlier steps, in front of later ones.  set_model has copied its arrays when it returns (it waits for
 *   the stream, as create does); set_model_dev returns at once, allocates nothing, and dA, dB, didx stay the caller's to keep alive
 *   until the stream has passed, as with step_dev.  Non-finite entries behave as at create: status 2 at those instances' steps.
 * rollout: T closed-loop steps of every instance from the controller's present state, in one launch -- what lqmpc_rollout_batch[_dev]
 *   returns for the controller's models (every set_model so far), its Q, R, P and box and the references of the last
 *   set_reference, without rebuilding the set-up the records already hold.  x0, JT, X, U, status, iters and A_true / B_true /
 *   true_per_instance are laid out and mean what they do for lqmpc_rollout_batch: a shared plant is a HOST pointer in both flavours,
 *   a per-instance plant a host pointer in the host flavour and a device pointer in _dev.  X, U, status, iters may be NULL.
 *   T < 1 (or > 100000) or a NULL c, x0, A_true, B_true or JT gives LQMPC_ERR_BAD_ARG before anything is enqueued.  A rollout is
 *   read-only on the controller: it starts cold, with empty faces, as lqmpc_rollout_batch does, carries its own face from step to
 *   step inside the kernel, neither reads nor writes the stored active sets and does not touch the records, so the steps before
 *   and after it are bit for bit what they would be without it.  Enqueued on the handle's stream, ordered with steps, set_reference
 *   and set_model; _dev returns at once, the host flavour copies in and out and waits, as step does.  It sets the handle's
 *   lqmpc_last_kernel: lqmpc_ctl_roll_r16_kernel<..> / lqmpc_ctl_roll_r64_kernel<..> / lqmpc_wg_ctl_rollout_kernel on a record
 *   controller (G and v_r from the record, W the first time an instance leaves the box, P the first time an iteration takes the
 *   primal side; an instance that reaches r16_maxit is redone by the hand-back pass of lqmpc_rollout_batch_dev from the
 *   controller's copies of A and B).  A pass-through controller runs lqmpc_rollout_batch_dev under its option snapshot on its
 *   copies of A and B; so does a 16-lane-row record controller of 4 096 instances or more, where the record kernel
 *   measured no faster than the one-shot call with its difficulty order (profiles/controller_rollout.json).
 * lqmpc_jit_compile_controller: the two kernels (factor, step) of a shape without prebuilt ones, compiled (or found in the cache
 *   directory) now; needs no GPU; returns 2 or a negative lqmpc_error.  lqmpc_jit_compile_controller_rollout: likewise the rollout
 *   kernel; returns 1, or LQMPC_ERR_UNSUPPORTED outside the 16-lane-row domain. */
typedef struct lqmpc_controller lqmpc_controller;
int lqmpc_controller_create(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz,
                            const double *A, const double *B,
                            const double *Q, const double *R, const double *P,
                            const double *lb, const double *ub,
                            const double *x_ref, const double *u_ref, lqmpc_controller **out);
int lqmpc_controller_create_dev(lqmpc_handle *h, int nx, int nu, int N, int64_t Bsz,
                                const double *dA, const double *dB,
                                const double *Q, const double *R, const double *P,
                                const double *lb, const double *ub,
                                const double *x_ref, const double *u_ref, lqmpc_controller **out);
int lqmpc_controller_step(lqmpc_controller *c, const double *x, double *u0, double *VN, int32_t *status, int32_t *iters);
int lqmpc_controller_step_dev(lqmpc_controller *c, const double *dx, double *du0, double *dVN, int32_t *dstatus, int32_t *diters);
int lqmpc_controller_step_plan(lqmpc_controller *c, const double *x, double *u0, double *VN, double *Uplan, double *Xplan,
                               int32_t *status, int32_t *iters);
int lqmpc_controller_step_plan_dev(lqmpc_controller *c, const double *dx, double *du0, double *dVN, double *dUplan, double *dXplan,
                                   int32_t *dstatus, int32_t *diters);
int lqmpc_controller_step_sens(lqmpc_controller *c, const double *x, double *u0, double *VN, double *K0, double *dVdx, double *Kplan,
                               double *Uplan, double *Xplan, int32_t *status, int32_t *iters);
int lqmpc_controller_step_sens_dev(lqmpc_controller *c, const double *dx, double *du0, double *dVN, double *dK0, double *ddVdx,
                                   double *dKplan, double *dUplan, double *dXplan, int32_t *dstatus, int32_t *diters);
int lqmpc_controller_model_grad(lqmpc_controller *c, const double *Uplan, const double *Xplan, const int32_t *status,
                                const double *gu0, const double *gVN, double *gA, double *gB, double *gx0);
int lqmpc_controller_model_grad_dev(lqmpc_controller *c, const double *dUplan, const double *dXplan, const int32_t *dstatus,
                                    const double *dgu0, const double *dgVN, double *dgA, double *dgB, double *dgx0);
int lqmpc_controller_cost_grad(lqmpc_controller *c, const double *Uplan, const double *Xplan, const int32_t *status,
                               const double *gu0, const double *gVN, int reduce,
                               double *gQ, double *gR, double *gP, double *glb, double *gub, double *gxref, double *guref,
                               int64_t *nskipped);
int lqmpc_controller_cost_grad_dev(lqmpc_controller *c, const double *dUplan, const double *dXplan, const int32_t *dstatus,
                                   const double *dgu0, const double *dgVN, int reduce,
                                   double *dgQ, double *dgR, double *dgP, double *dglb, double *dgub, double *dgxref, double *dguref,
                                   int64_t *dnskipped);
int lqmpc_controller_plan_grad(lqmpc_controller *c, const double *Uplan, const double *Xplan, const int32_t *status,
                               const double *gUplan, const double *gXplan, const double *gVN, double *gA, double *gB, double *gx0);
int lqmpc_controller_plan_grad_dev(lqmpc_controller *c, const double *dUplan, const double *dXplan, const int32_t *dstatus,
                                   const double *dgUplan, const double *dgXplan, const double *dgVN,
                                   double *dgA, double *dgB, double *dgx0);
int lqmpc_controller_rollout(lqmpc_controller *c, int T, const double *x0,
                             const double *A_true, const double *B_true, int true_per_instance,
                             double *JT, double *X, double *U, int32_t *status, int32_t *iters);
int lqmpc_controller_rollout_dev(lqmpc_controller *c, int T, const double *dx0,
                                 const double *A_true, const double *B_true, int true_per_instance,
                                 double *dJT, double *dX, double *dU, int32_t *dstatus, int32_t *diters);
int lqmpc_controller_reset(lqmpc_controller *c);
int lqmpc_controller_set_reference(lqmpc_controller *c, const double *x_ref, const double *u_ref);
int lqmpc_controller_set_model(lqmpc_controller *c, int64_t count, const int32_t *idx, const double *A, const double *B);
int lqmpc_controller_set_model_dev(lqmpc_controller *c, int64_t count, const int32_t *didx, const double *dA, const double *dB);
int64_t lqmpc_controller_bytes(const lqmpc_controller *c);
const char *lqmpc_controller_kernel(const lqmpc_controller *c);
int lqmpc_controller_destroy(lqmpc_controller *c);
int lqmpc_jit_compile_controller(int nx, int nu, int N, char *log, int log_len);
int lqmpc_jit_compile_controller_rollout(int nx, int nu, int N, char *log, int log_len);
/* ... and the kernels lqmpc_solve_plan_batch / lqmpc_controller_step_plan launch on a run-time compiled shape (the plan is written by
 * kernels of their own, so that the plain calls' kernels hold none of it; otherwise compiled on the first plan call): returns their
 * number, 2, or 1 on a wide-state shape (no record controller there). */
int lqmpc_jit_compile_plan(int nx, int nu, int N, char *log, int log_len);

/* ---- timing on the handle's stream (hipEvents), for bench.py's roofline ----
 * begin/end bracket any number of *_dev calls; end waits for the stream and returns the
 * elapsed milliseconds between the two events. */
int lqmpc_timer_begin(lqmpc_handle *h);
int lqmpc_timer_end(lqmpc_handle *h, float *ms);

#ifdef __cplusplus
}
#endif
#endif /* LQMPC_H */
