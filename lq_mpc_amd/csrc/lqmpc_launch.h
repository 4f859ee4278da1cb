// lqmpc_launch.h -- what the kernel files offer the host side (lqmpc_api.hip), declared once: the defining files include it as well,
// so a signature that drifts is a compile error.  Host only (not part of the run-time compiled text).
#pragma once
#include "lqmpc_common.h"
#include "lqmpc_bounds.h"

#include <string>

namespace lqmpc {

// one row of a table of prebuilt 16-lane-row instantiations (lqmpc_r16.hip, lqmpc_ctl.hip)
struct ShapeEntry {
    int nx, nu, N, lpi;
    const char *name;
    void (*launch)(const KParams &, hipStream_t);
};

// lqmpc_generic.hip: any shape within the build limits, workspace in HBM (ws_stride instances per entry row)
long long generic_ws_entries(int nx, int nu, int N);
void launch_generic(const KParams &p, hipStream_t stream);
// ... over a device-side list (p.perm, p.count_dev) with `cols` workspace columns
void launch_generic_list(const KParams &p, int cols, hipStream_t stream);

// lqmpc_spec.hip: the packed register-resident kernels; spec_available is false when no specialisation is built for (nx,nu,N)
bool spec_available(int nx, int nu, int N);
bool spec_tiered_available(int nx, int nu, int N);
bool launch_spec(const KParams &p, hipStream_t stream, const char **name);
void launch_order_scatter(const KParams &p, int *perm, hipStream_t stream);

// lqmpc_r16.hip: one instance per 16-lane row (n <= 32) or per wavefront; lqmpc_r16_lat.hip: the latency build of some of its shapes
bool r16_available(int nx, int nu, int N);
int r16_lanes(int nx, int nu, int N);       // 16, 64 (one instance per wavefront: n > 32) or 0
bool launch_r16(const KParams &p, hipStream_t stream, const char **name);
bool launch_r16_lat(const KParams &p, hipStream_t stream);

// lqmpc_wg.hip: one instance per workgroup, 32 < n <= 128
bool wg_supported(int nx, int nu, int N);
bool launch_wg(const KParams &p, hipStream_t stream, const char **name);
// ... its prepared controller: one record per instance (wg_ctl_rec_layout), p.mode = MODE_CTL_FACTOR / MODE_CTL_STEP
bool launch_wg_ctl(const KParams &p, hipStream_t stream, const char **name);

// lqmpc_jit.hip: the 16-lane-row kernel (and the probe) of a shape without a prebuilt instantiation, compiled at run time
// (wide: also the shapes with 9 <= nx <= 16, N nu <= 32 -- options.jit = 2; the prepared controller's record kernels never ask for them)
bool jit_r16_shape(int nx, int nu, int N, int *lpi, bool wide = false);
bool jit_available(int device, int nx, int nu, int N, int mode, std::string *why, bool wide = false);
bool launch_jit(int device, const KParams &p, hipStream_t stream, const char **name, std::string *why);
bool launch_jit_bounds(int device, const BoundsParams &p, hipStream_t stream, std::string *why);

// lqmpc_ctl.hip: the factor / step kernels of a prepared controller (p.mode = MODE_CTL_FACTOR / MODE_CTL_STEP), prebuilt shapes
bool ctl_available(int nx, int nu, int N);
bool launch_ctl(const KParams &p, hipStream_t stream, const char **name);

// lqmpc_ctl_ref.hip: new references for a prepared controller -- v_r of every record rewritten in place from the shared block
// (p.sh, p.has_ref) and the record's own A, B, W; run-time dimensions, so the run-time compiled shapes are served as well
bool launch_ctl_retarget(const KParams &p, hipStream_t stream);          // ctl_rec_layout records
bool launch_wg_ctl_retarget(const KParams &p, hipStream_t stream);       // wg_ctl_rec_layout records
// ... and new models for listed instances: the update's arrays (instance-minor over `count`) scattered into the controller's
// instance-minor copies at the columns idx[0..count) (device); an index outside [0, Bsz) writes nothing
void launch_ctl_scatter_model(double *A, double *B, const double *uA, const double *uB, const int *idx, int nx, int nu, long long count,
                              long long Bsz, hipStream_t stream);

// lqmpc_sens.hip: the post-pass of lqmpc_solve_sens_batch / lqmpc_controller_step_sens -- from a plan the solve kernels have written,
// the gain of the local feedback law on the plan's face and the gradient of V_N.  One kernel for every shape within the build limits.
struct SensParams {
    int nx, nu, N;
    long long Bsz;
    const double *A, *B;                  // element e (row-major) of instance b at A[e * sE + b * sI]: instance-minor arrays (sE = Bsz, sI = 1)
    long long sE, sI;                     // or the heads of a workgroup controller's records (sE = 1, sI = the record stride)
    const double *Uplan, *Xplan;          // the plan call's outputs, instance-minor
    const int *status;                    // the plan call's status; 2 gives NaN in every output of the instance
    const double *sh;                     // shared block (device) of the plan call
    SharedOff so;
    double *K0, *dVdx, *Kplan;            // outputs, instance-minor; Kplan may be null
};
bool launch_sens(const SensParams &p, hipStream_t stream);

// lqmpc_grad.hip: the post-pass of lqmpc_model_grad_batch / lqmpc_controller_model_grad -- from a plan the solve kernels have written and
// the cotangents of u_0 and V_N, the gradient with respect to A and B of every instance on the plan's face.  One kernel for every
// shape within the build limits; grad_fits says whether its LDS image does (launch_grad refuses, and launches nothing, where not).
struct GradParams {
    int nx, nu, N;
    long long Bsz;
    const double *A, *B;                  // as SensParams: element e of instance b at A[e * sE + b * sI]
    long long sE, sI;
    const double *Uplan, *Xplan;          // what a plan or sens call wrote, instance-minor
    const int *status;                    // its status (2 gives NaN in every output of the instance); null: all 0
    const double *sh;                     // shared block (device): Q, R, P, the box and x_ref at the offsets so
    SharedOff so;
    const double *gu0, *gVN;              // d loss / d u_0 (nu, Bsz) and d loss / d V_N (Bsz); either may be null = zero
    double *gA, *gB, *gx0;                // outputs, instance-minor; gx0 may be null
};
size_t grad_lds_bytes(int nx, int nu, int N);
bool grad_fits(int nx, int nu, int N);
bool launch_grad(const GradParams &p, hipStream_t stream);

// lqmpc_cgrad.hip: the post-pass of lqmpc_cost_grad_batch / lqmpc_controller_cost_grad -- from the same inputs, the gradient with
// respect to the data the batch shares: the weights Q, R, P, the box lb, ub and the references x_ref, u_ref.  Per instance
// (reduce = 0: every output instance-minor) or summed over the batch on chip (reduce = 1: every output in the shape of its parameter,
// row-major; cgrad_blocks wavefronts each leave one vector of partial sums in `part`, a second kernel adds them in a fixed order).
struct CGradParams {
    int nx, nu, N;
    long long Bsz;
    const double *A, *B;                  // as SensParams: element e of instance b at A[e * sE + b * sI]
    long long sE, sI;
    const double *Uplan, *Xplan;          // what a plan or sens call wrote, instance-minor
    const int *status;                    // its status (2: NaN in every output of the instance / left out of the sums); null: all 0
    const double *sh;                     // shared block (device): Q, R, P, the box, x_ref and u_ref at the offsets so
    SharedOff so;
    const double *gu0, *gVN;              // d loss / d u_0 (nu, Bsz) and d loss / d V_N (Bsz); either may be null = zero
    int reduce;
    double *out[7];                       // gQ, gR, gP, glb, gub, gxref, guref; any may be null, not all
    long long *nskipped;                  // reduce: the number of instances with status 2 (device); may be null
    double *part;                         // reduce: cgrad_part_bytes of the handle's own block, entry e of wavefront g at part[e * blocks + g]
};
size_t cgrad_lds_bytes(int nx, int nu, int N, int reduce);
bool cgrad_fits(int nx, int nu, int N, int reduce);
long long cgrad_blocks(int nx, int nu, int N, long long Bsz, int reduce);   // the grid: a function of the shape and Bsz only
size_t cgrad_part_bytes(int nx, int nu, int N, long long Bsz);
bool launch_cgrad(const CGradParams &p, hipStream_t stream);

// lqmpc_pgrad.hip: the post-pass of lqmpc_plan_grad_batch / lqmpc_controller_plan_grad -- from the same plan and the cotangents of
// every u_i, every x_i and V_N, the gradient with respect to A, B and x_0 of every instance on the plan's face.  One kernel for every
// shape within the build limits; pgrad_fits says whether its LDS image does (launch_pgrad refuses, and launches nothing, where not).
struct PGradParams {
    int nx, nu, N;
    long long Bsz;
    const double *A, *B;                  // as SensParams: element e of instance b at A[e * sE + b * sI]
    long long sE, sI;
    const double *Uplan, *Xplan;          // what a plan or sens call wrote, instance-minor
    const int *status;                    // its status (2 gives NaN in every output of the instance); null: all 0
    const double *sh;                     // shared block (device): Q, R, P, the box and x_ref at the offsets so
    SharedOff so;
    const double *gU, *gX, *gVN;          // d loss / d Uplan (nu, N, Bsz), d loss / d Xplan (nx, N + 1, Bsz), d loss / d V_N (Bsz); null = zero
    double *gA, *gB, *gx0;                // outputs, instance-minor; any may be null
};
size_t pgrad_lds_bytes(int nx, int nu, int N);
bool pgrad_fits(int nx, int nu, int N);
bool launch_pgrad(const PGradParams &p, hipStream_t stream);

// lqmpc_rgrad.hip: the closed loop with a tape and its gradient (lqmpc_rollout_tape_batch, lqmpc_rollout_grad_batch).
// The plant step behind the plan call of step t: x_{t+1} = A_true x_t + B_true u_0, the cost, row t + 1 of X, row t of U.
struct PlantStepParams {
    int nx, nu, N, T, t;
    long long Bsz;
    const double *At, *Bt;                // element e of the plant of instance b at At[e * sE + b * sI]: instance-minor arrays
    long long sE, sI;                     // (sE = Bsz, sI = 1) or the shared block's single matrices (sE = 1, sI = 0)
    const double *sh;                     // shared block (device): Q and R at the offsets so
    SharedOff so;
    const double *x;                      // x_t (nx, Bsz), instance-minor: x0 at t = 0, then the handle's buffer of the step before
    const double *Uslice;                 // slice t of the tape: u_0[k] at Uslice[k * N * Bsz + b]
    const int *st, *it;                   // status and iters of the solve of step t
    double *xn;                           // x_{t+1} (nx, Bsz): the handle's other buffer
    double *JT, *X, *U;                   // X, U may be null
    int *status, *iters;                  // the largest status and the sum of the iterations so far; may be null
};
void launch_plant_step(const PlantStepParams &p, hipStream_t stream);

// ... and the gradient of a loss on (J_T, X, U) of that loop with respect to the model, the plant and x_0, from the tape: one launch.
struct RGradParams {
    int nx, nu, N, T;
    long long Bsz;
    const double *A, *B;                  // the model, instance-minor
    const double *At, *Bt;                // the plant, as PlantStepParams
    long long sE, sI;
    const double *X, *Utape;              // (nx, T + 1, Bsz) and T plans (nu, N, Bsz)
    const int *status_tape;               // (T, Bsz); 2 at any step gives NaN in every output of the instance; null: all 0
    const double *sh;                     // shared block (device): Q, R, P, the box and x_ref at the offsets so
    SharedOff so;
    const double *gJT, *gX, *gU;          // d loss / d J_T (Bsz), d X (nx, T + 1, Bsz), d U (nu, T, Bsz); null = zero
    double *gA, *gB, *gx0, *gAt, *gBt;    // outputs, instance-minor; any may be null
};
size_t rgrad_lds_bytes(int nx, int nu, int N);
bool rgrad_fits(int nx, int nu, int N);
bool launch_rgrad(const RGradParams &p, hipStream_t stream);

// lqmpc_rcgrad.hip: the gradient of the same loss on the same tape with respect to the data the batch shares -- the weights Q, R, P, the
// box lb, ub and the references x_ref, u_ref (lqmpc_rollout_cost_grad_batch).  One launch per instance (reduce = 0: every output
// instance-minor); with reduce every wavefront leaves one vector of partial sums in `part` and a second small kernel adds them in a
// fixed order (every output in the shape of its parameter, row-major).
struct RCGradParams {
    int nx, nu, N, T;
    long long Bsz;
    const double *A, *B;                  // the model, instance-minor
    const double *At, *Bt;                // the plant, as PlantStepParams
    long long sE, sI;
    const double *X, *Utape;              // (nx, T + 1, Bsz) and T plans (nu, N, Bsz)
    const int *status_tape;               // (T, Bsz); 2 at any step: NaN in every output of the instance / left out of the sums; null: all 0
    const double *sh;                     // shared block (device): Q, R, P, the box, x_ref and u_ref at the offsets so
    SharedOff so;
    const double *gJT, *gX, *gU;          // d loss / d J_T (Bsz), d X (nx, T + 1, Bsz), d U (nu, T, Bsz); null = zero
    int reduce;
    double *out[7];                       // gQ, gR, gP, glb, gub, gxref, guref; any may be null, not all
    long long *nskipped;                  // reduce: the number of instances with status 2 at any step (device); may be null
    double *part;                         // reduce: rcgrad_part_bytes of the handle's own block, entry e of wavefront g at part[e * blocks + g]
};
size_t rcgrad_lds_bytes(int nx, int nu, int N);
bool rcgrad_fits(int nx, int nu, int N);
size_t rcgrad_part_bytes(int nx, int nu, int N, long long Bsz);
bool launch_rcgrad(const RCGradParams &p, hipStream_t stream);

// lqmpc_poly.hip: the problem with polytopic input constraints Fu u_i <= 1 (lqmpc_solve_poly_batch, lqmpc_rollout_poly_batch): one
// solve per instance (T = 0) or T closed-loop steps from one set-up (T >= 1), one instance per wavefront.  Run-time dimensions within
// N nu <= 64, m <= 16; poly_fits says whether the LDS image does (launch_poly refuses, and launches nothing, where not).
struct PolyOff {
    int Q, R, P, Fu, xref, uref, At, Bt;  // offsets (in doubles) into the shared block of a polytope call; Fu is (m, nu) row-major
};
struct PolyParams {
    int nx, nu, N, m, T;
    int max_iter;                         // cap on the passes of the active-set loop of one solve; 0: 10 N nu + 20
    double eps;                           // a row counts as satisfied within eps * rho, rho = max_j 1 / |Fu_j|
    long long Bsz;
    const double *A, *B, *x0;             // instance-minor (device)
    const double *At, *Bt;                // T >= 1: element e of the plant of instance b at At[e * sE + b * sI], as PlantStepParams
    long long sE, sI;
    const double *sh;                     // shared block (device)
    PolyOff so;
    double *u0, *VN, *Uplan, *Xplan, *lam;   // T = 0: u0 and VN required, the others may be null
    double *JT, *X, *U;                   // T >= 1: JT required, X and U may be null
    int *status, *iters;                  // may be null
    // the prepared controller (launch_poly_ctl); unused by launch_poly
    double *rec;                          // record r at rec + r * rstride (poly_rec_layout)
    long long rstride, nrec;              // doubles between records; records the controller holds
    const int *idx;                       // factor: wavefront j writes record idx[j] (device; null: record j), an entry outside [0, nrec) is skipped
};
size_t poly_lds_bytes(int nx, int nu, int N, int m);
bool poly_fits(int nx, int nu, int N, int m);
bool launch_poly(const PolyParams &p, hipStream_t stream, const char **name);

// ... its prepared controller (lqmpc_poly_controller_*).  One record per instance, contiguous, so that a wavefront reads it with
// consecutive lanes on consecutive addresses: [A (nx nx) | B (nx nu) | W_k = A^k B, k < N (N nx nu) | Jp (n (n + 1) / 2)], Jp = L^-1
// packed by rows, entry (j, t <= j) at j (j + 1) / 2 + t.  The stride is a multiple of 16 doubles: records start on 128-byte lines.
struct PolyRec {
    int A, B, W, Jp, stride;
};
__host__ __device__ constexpr PolyRec poly_rec_layout(int nx, int nu, int N)
{
    const int n = N * nu, A = 0, B = A + nx * nx, W = B + nx * nu, Jp = W + N * nx * nu, end = Jp + n * (n + 1) / 2;
    return PolyRec{A, B, W, Jp, (end + 15) / 16 * 16};
}
// what: the factor launch (p.Bsz wavefronts over p.A, p.B instance-minor over p.Bsz; records through p.idx), one step from the
// records (p.T = 0) or T closed-loop steps from them (p.T >= 1); p.sh holds Q, R, P, Fu and the references in every case
enum { POLY_CTL_FACTOR = 0, POLY_CTL_STEP = 1, POLY_CTL_ROLLOUT = 2 };
size_t poly_step_lds_bytes(int nx, int nu, int N, int m);
bool launch_poly_ctl(const PolyParams &p, int what, hipStream_t stream, const char **name);

}  // namespace lqmpc
