// lqmpc_rcgrad.hip -- the gradient of a loss on the closed loop -- J_T, every x_t and every u_t of a tape lqmpc_rollout_tape_batch wrote --
// with respect to the data the batch shares: the weights Q, R, P, the references x_ref, u_ref and the box lb, ub
// (lqmpc_rollout_cost_grad_batch).  The sibling of lqmpc_rgrad.hip, in a kernel of its own beside it; it touches no other kernel.
// gfx950 (MI355X) only.
//
// lqmpc_rollout_cost_grad_kernel: the tape walked backwards with the plant's costate.  Per instance, with gam = d loss / d J_T:
//     l_T = gX_T + 2 gam Q x_T
//     t = T-1 .. 0:   w_t = gU_t + 2 gam R u_t + B_true'l_{t+1}
//                     the plan of step t re-rolled on the model from x_t and slice t of the tape:  x_0 = x_t,  x_{i+1} = A x_i + B u_i
//                     the cost gradient of lqmpc_cgrad.hip for gu0 = w_t, gVN = 0, restated (f_j the free mask of stage j):
//                         S = P;  j = N-1 .. 0:  Re = R_j + B_j'S B_j,  K_j = Re^-1 B_j'S A,  S <- Q + A'S (A - B_j K_j)
//                         ut_0 = 1/2 f_0 Re_0^-1 f_0 w_t,  xt_0 = 0;  ut_j = -K_j xt_j (j > 0),  xt_{j+1} = A xt_j + B ut_j
//                         e_i = x_i - xref_{i-1},  d_i = u_i - uref_i;   lt_N = 2 P xt_N,  lt_i = 2 Q xt_i + A'lt_{i+1},  rt_i = 2 R ut_i + B'lt_{i+1}
//                         gQ -= sum_{i=1}^{N-1} xt_i e_i' + e_i xt_i'  (gP: the same term at i = N),   gR -= sum_i ut_i d_i' + d_i ut_i'
//                         gxref[:, i-1] += 2 Q xt_i  (P at i = N),   guref[:, i] += 2 R ut_i
//                         gub[k] += sum over the entries (i, k) on the upper bound of -rt_i[k] + (i == 0 ? w_t[k] : 0);  glb likewise
//                         gx_t = -A'lt_1
//                     gQ += gam x_t x_t' (and gam x_T x_T' first),  gR += gam u_t u_t':  the one Q and R of the call also weigh J_T
//                     l_t = gX_t + 2 gam Q x_t + A_true'l_{t+1} + gx_t
// Only the adjoint costate lt is needed; the plan's own costate is not.
//
// Mapping: that of lqmpc_rollout_grad_kernel -- one instance per 16-lane row, four per wavefront, one wavefront per workgroup, so every
// barrier below is a wave-local wait.  Lane a of a row owns row a of S and T = S A, column a of K_j, component a of the costates.  The
// M = 2 nx^2 + nu^2 + N (nx + nu) + 2 nu sums of an instance are carried over all T steps in LDS, every lane adding to its own entries
// only: lane a to row a of gQ, gP and gxref, lane k < nu to row k of gR and guref and to glb[k], gub[k].  The model and the plant of an
// instance, K_j of every stage, the plan of the step and its states sit in dynamic LDS, loaded once per instance; Q, R, P once per
// workgroup.  Slice t - 1 of the tape, x_{t-1} and the cotangents of step t - 1 are read from HBM into registers while step t is worked on.
// Two output modes.  Per instance: at the end every sum goes to HBM, instance-minor; no HBM workspace.  Reduced: the four rows' images
// are added in the order of the rows, the wavefront writes one vector of partial sums, and lqmpc_rollout_cost_grad_finish_kernel adds
// the vectors in a fixed order.  No atomics: the same data give the same bits.
// The face rule is that of lqmpc_sens.hip: bit for bit lb or c - h is lower, ub or c + h is upper.  Nothing branches on a computed
// value: NaN flows through; an instance with status 2 at any step gets NaN in every output (per instance) or adds 0.0 and is counted
// (reduced), by a select where the value is handed over.  The one skip is wave-uniform: a step at which every stage-0 input of all four
// instances of the wavefront sits on a bound (a ballot over the bits of the tape) has ut = 0, xt = 0 and lt = 0; its sweep and rolls are
// passed over, but w_t[k] still goes to glb[k] or gub[k] of every stage-0 entry, as it would have with them.  The gains of the all-free
// face do not depend on t: where all four plans of the wavefront are wholly free at a step and were at the step worked on before it,
// the sweep is not run again (the same bits).
#include "lqmpc_launch.h"

#include <cstdio>

namespace lqmpc {

namespace {

constexpr int RC_ROW = 16;                   // lanes per instance
constexpr int RC_IPB = 4;                    // instances per workgroup (one wavefront)
constexpr int RC_THREADS = RC_ROW * RC_IPB;
constexpr int RC_MAX_NX = 16, RC_MAX_NU = 8; // the build limits of include/lqmpc.h
constexpr int RC_SLICE = 8;                  // registers of a lane that hold its share of a slice: N nu <= 128 = 16 x 8
constexpr size_t RC_LDS_LIMIT = 160 * 1024;
enum { RC_Q, RC_R, RC_P, RC_LB, RC_UB, RC_XREF, RC_UREF, RC_OUTS };
// wavefronts per SIMD the register allocation is held to, chosen by measurement as section 4.14 did (C3 x 65 536, T = 30: 11.65 ms at
// two, 10.81 ms at three with 60 bytes of scratch, 11.55 ms at four with 216, 12.58 ms at five with 344; three is also ahead at C4, C5;
// measured on the layout before S, T, C, W, G shared their room with xt, ut).  -DRC_WAVES=n builds another, for
// tools/rollout_cost_grad_time.py --lib
#ifndef RC_WAVES
#define RC_WAVES 3
#endif
// 1: the sweep of the all-free face is kept across the steps (C3 x 65 536, T = 30: 11.55 ms with it, 17.52 ms without, at four waves)
#ifndef RC_REUSE
#define RC_REUSE 1
#endif

// LDS image in doubles: [Q | R | P] once, then per instance
// [A | At | B | Bt | (S | T | C | W | G) or (Xt | Ut) | Re | Di | F | Y | Wt | V | L | Kst | Xp | Up | the sums | the count of instances left out]
struct RcLds {
    int ld;                                  // row stride of the nx-wide matrices (odd)
    int Q, R, P, shared;
    int A, At, S, T, C, B, Bt, W, G, Re, Di, F, Y, Wt, V, L, K, Xt, Ut, Xp, Up, Acc, inst;
    int acc[RC_OUTS + 1];                    // offsets of the seven sums in the image of the sums; acc[RC_OUTS] = their number M
};

__host__ __device__ inline RcLds rcgrad_lds(int nx, int nu, int N)
{
    RcLds o;
    o.ld = nx | 1;
    int e = 0;
    o.Q = e; e += nx * nx;
    o.R = e; e += nu * nu;
    o.P = e; e += nx * nx;
    o.shared = e;
    e = 0;
    o.acc[RC_Q] = e; e += nx * nx;
    o.acc[RC_R] = e; e += nu * nu;
    o.acc[RC_P] = e; e += nx * nx;
    o.acc[RC_LB] = e; e += nu;
    o.acc[RC_UB] = e; e += nu;
    o.acc[RC_XREF] = e; e += nx * N;
    o.acc[RC_UREF] = e; e += nu * N;
    o.acc[RC_OUTS] = e;
    e = 0;
    o.A = e; e += nx * o.ld;                 // A, row-major
    o.At = e; e += nx * o.ld;                // A_true, row-major
    o.B = e; e += nx * nu;
    o.Bt = e; e += nx * nu;                  // B_true
    // what only the sweep uses -- S, T, C, W, G -- shares its room with the adjoint plan xt, ut, which is formed behind the sweep and is
    // dead before the next one: at (8,4,30) that brings the image under half a CU's LDS, so that two workgroups fit
    const int sweep0 = e;
    o.S = e; e += nx * o.ld;                 // the Riccati matrix
    o.T = e; e += nx * o.ld;                 // S A
    o.C = e; e += nx * o.ld;                 // Acl_j
    o.W = e; e += nx * nu;                   // S B
    o.G = e; e += nu * o.ld;                 // B_j'S A, then K_j in place
    const int sweep1 = e;
    e = sweep0;
    o.Xt = e; e += (N + 1) * nx;             // xt_0 .. xt_N
    o.Ut = e; e += N * nu;                   // ut_0 .. ut_{N-1}
    e = e > sweep1 ? e : sweep1;
    o.Re = e; e += nu * nu;                  // Re, then its Cholesky factor below the diagonal
    o.Di = e; e += nu;                       // reciprocals of the factor's diagonal
    o.F = e; e += nu;                        // free mask of the stage, 1.0 / 0.0
    o.Y = e; e += nu;                        // the solve for ut_0; backward pass: d_i
    o.Wt = e; e += nu;                       // w_t
    o.V = e; e += 3 * nx;                    // backward pass: e_i, and lt of two stages
    o.L = e; e += 2 * nx;                    // the plant's costate of two steps
    o.K = e; e += N * nu * nx;               // K_j of every stage
    o.Xp = e; e += (N + 1) * nx;             // the plan's states x_0 = x_t .. x_N, re-rolled on the model
    o.Up = e; e += N * nu;                   // slice t of the tape, as it lies in HBM: u_i[k] at k N + i
    o.Acc = e; e += o.acc[RC_OUTS] + 1;      // the sums over the steps, and 1.0 where the instance is left out of a reduced call
    o.inst = e;
    return o;
}

}  // namespace

__global__ void __launch_bounds__(RC_THREADS) __attribute__((amdgpu_waves_per_eu(RC_WAVES, RC_WAVES)))
lqmpc_rollout_cost_grad_kernel(const RCGradParams p)
{
    extern __shared__ double lds_rcgrad[];
    const int nx = p.nx, nu = p.nu, N = p.N, T = p.T;
    const int t0 = threadIdx.x, a = t0 & (RC_ROW - 1), row = t0 / RC_ROW;
    const RcLds o = rcgrad_lds(nx, nu, N);
    const int ld = o.ld, nv = nu * N, M = o.acc[RC_OUTS];
    const long long Bsz = p.Bsz;
    // the tail of the batch: a row past the end works on the last instance and hands nothing over
    const long long b0 = (long long)blockIdx.x * RC_IPB + row;
    const bool valid = b0 < Bsz;
    const long long b = valid ? b0 : Bsz - 1;
    const bool on = a < nx, inp = a < nu;
    const double *sh = p.sh;

    double *Qs = lds_rcgrad + o.Q, *Rs = lds_rcgrad + o.R, *Ps = lds_rcgrad + o.P;
    double *I = lds_rcgrad + o.shared + row * o.inst;
    double *Am = I + o.A, *Atm = I + o.At, *S = I + o.S, *Tm = I + o.T, *C = I + o.C, *Bm = I + o.B, *Btm = I + o.Bt, *W = I + o.W;
    double *G = I + o.G, *Re = I + o.Re, *Di = I + o.Di, *F = I + o.F, *Y = I + o.Y, *Wt = I + o.Wt, *V = I + o.V;
    double *Kst = I + o.K, *Xt = I + o.Xt, *Ut = I + o.Ut, *Xp = I + o.Xp, *Up = I + o.Up, *acc = I + o.Acc;
    double *Ln = I + o.L, *Lc = I + o.L + nx;   // the plant's costate of step t + 1 and of step t
    double *aQ = acc + o.acc[RC_Q] + a * nx, *aP = acc + o.acc[RC_P] + a * nx, *aR = acc + o.acc[RC_R] + a * nu;
    double *aXr = acc + o.acc[RC_XREF] + a * N, *aUr = acc + o.acc[RC_UREF] + a * N, *aLb = acc + o.acc[RC_LB] + a, *aUb = acc + o.acc[RC_UB] + a;

    for (int e = t0; e < nx * nx; e += RC_THREADS) { Qs[e] = sh[p.so.Q + e]; Ps[e] = sh[p.so.P + e]; }
    for (int e = t0; e < nu * nu; e += RC_THREADS) Rs[e] = sh[p.so.R + e];
    for (int e = a; e < nx * nx; e += RC_ROW) {
        const int r = e / nx, c = e - r * nx;
        Am[r * ld + c] = p.A[(long long)e * Bsz + b];
        Atm[r * ld + c] = p.At[(long long)e * p.sE + b * p.sI];
    }
    for (int e = a; e < nx * nu; e += RC_ROW) {
        Bm[e] = p.B[(long long)e * Bsz + b];
        Btm[e] = p.Bt[(long long)e * p.sE + b * p.sI];
    }
    for (int e = a; e <= M; e += RC_ROW) acc[e] = 0.0;
    const double nan = __builtin_nan("");
    const double gam = p.gJT ? p.gJT[b] : 0.0;
    // the four forms a bound can come out in (include/lqmpc.h, the plan's contract)
    double lbk = 0.0, ubk = 0.0, lo = 0.0, hi = 0.0;
    if (inp) {
        lbk = sh[p.so.lb + a]; ubk = sh[p.so.ub + a];
        const double ctr = 0.5 * (ubk + lbk), h = 0.5 * (ubk - lbk);
        lo = ctr - h; hi = ctr + h;
    }

    // what a lane holds of step t one step ahead: its share of slice t, x_t[a], gX_t[a], gU_t[a] and the status
    double sl[RC_SLICE], xr = 0.0, gxr = 0.0, gur = 0.0;
    int str = 0;
    auto fetch = [&](int t) {
        const double *slice = p.Utape + (long long)t * nv * Bsz;
#pragma unroll
        for (int q = 0; q < RC_SLICE; ++q) {
            const int e = a + q * RC_ROW;
            sl[q] = e < nv ? slice[(long long)e * Bsz + b] : 0.0;
        }
        if (on) {
            xr = p.X[((long long)a * (T + 1) + t) * Bsz + b];
            if (p.gX) gxr = p.gX[((long long)a * (T + 1) + t) * Bsz + b];
        }
        if (inp && p.gU) gur = p.gU[((long long)a * T + t) * Bsz + b];
        if (p.status_tape) str = p.status_tape[(long long)t * Bsz + b];
    };

    // l_T = gX_T + 2 gam Q x_T, and the direct part of x_T
    if (on) {
        Xp[a] = p.X[((long long)a * (T + 1) + T) * Bsz + b];
        if (p.gX) gxr = p.gX[((long long)a * (T + 1) + T) * Bsz + b];
    }
    __syncthreads();
    if (on) {
        double s = 0.0;
        for (int c = 0; c < nx; ++c) s = __builtin_fma(Qs[a * nx + c], Xp[c], s);
        Ln[a] = gxr + 2.0 * gam * s;
        const double px = gam * Xp[a];
        for (int c = 0; c < nx; ++c) aQ[c] = __builtin_fma(px, Xp[c], aQ[c]);
    }
    gxr = 0.0;
    fetch(T - 1);
    __syncthreads();

    bool bad = false, kfree = false;            // kfree: Kst, Re, Di and F hold the sweep of the all-free face
    double *d = V, *m0 = V + nx, *m1 = V + 2 * nx, *ds = Y;

    for (int t = T - 1; t >= 0; --t) {
        // ---- step t from the registers into LDS, step t - 1 on its way from HBM ----
        if (on) Xp[a] = xr;
#pragma unroll
        for (int q = 0; q < RC_SLICE; ++q) {
            const int e = a + q * RC_ROW;
            if (e < nv) Up[e] = sl[q];
        }
        const double gx = gxr, gu = gur;
        bad = bad || str == 2;
        if (t > 0) fetch(t - 1);
        __syncthreads();

        // ---- w_t, the direct part of step t, and whether any instance of the wavefront has a free input at stage 0 ----
        bool free0 = false, fixed_any = false;
        double wk = 0.0, u0 = 0.0;
        if (inp) {
            for (int j = 0; j < N; ++j) {
                const double v = Up[a * N + j];
                fixed_any = fixed_any || v == lbk || v == ubk || v == lo || v == hi;
            }
            u0 = Up[a * N];
            free0 = !(u0 == lbk || u0 == ubk || u0 == lo || u0 == hi);
            double r = 0.0;
            for (int l = 0; l < nu; ++l) r = __builtin_fma(Rs[a * nu + l], Up[l * N], r);
            double s = gu + 2.0 * gam * r;
            for (int m = 0; m < nx; ++m) s = __builtin_fma(Btm[m * nu + a], Ln[m], s);
            Wt[a] = s;
            wk = s;
            const double pu = gam * u0;
            for (int l = 0; l < nu; ++l) aR[l] = __builtin_fma(pu, Up[l * N], aR[l]);
        }
        if (on) {
            const double px = gam * Xp[a];
            for (int c = 0; c < nx; ++c) aQ[c] = __builtin_fma(px, Xp[c], aQ[c]);
        }
        const bool qp = __ballot(free0) != 0ull;    // wave-uniform: the bits of the tape, not a computed value
        // all four plans wholly free, as at the step worked on before this one: K_j, the factor of stage 0 and F are still those of the
        // all-free face, which does not depend on t, and the sweep is not run again
        const bool wave_free = __ballot(fixed_any) == 0ull;
        const bool sweep = !(RC_REUSE && wave_free && kfree);
        double gxt = 0.0;                           // component a of gx_t

        if (qp) {
            // ---- the plan's states on the model, from x_t and the slice; S = P ----
            if (on && sweep)
                for (int c = 0; c < nx; ++c) S[a * ld + c] = Ps[a * nx + c];
            for (int i = 0; i < N; ++i) {
                if (on) {
                    double s = 0.0;
                    for (int c = 0; c < nx; ++c) s = __builtin_fma(Am[a * ld + c], Xp[i * nx + c], s);
                    for (int k = 0; k < nu; ++k) s = __builtin_fma(Bm[a * nu + k], Up[k * N + i], s);
                    Xp[(i + 1) * nx + a] = s;
                }
                __syncthreads();
            }

            // ---- the masked Riccati sweep, backwards over the stages (lqmpc_cgrad.hip) ----
            for (int j = sweep ? N - 1 : -1; j >= 0; --j) {
                if (inp) {
                    const double u = Up[a * N + j];
                    F[a] = (u == lbk || u == ubk || u == lo || u == hi) ? 0.0 : 1.0;
                }
                if (on) {
                    // row a of T = S A and of W = S B
                    for (int c = 0; c < nx; ++c) {
                        double s = 0.0;
                        for (int m = 0; m < nx; ++m) s = __builtin_fma(S[a * ld + m], Am[m * ld + c], s);
                        Tm[a * ld + c] = s;
                    }
                    for (int k = 0; k < nu; ++k) {
                        double s = 0.0;
                        for (int m = 0; m < nx; ++m) s = __builtin_fma(S[a * ld + m], Bm[m * nu + k], s);
                        W[a * nu + k] = s;
                    }
                }
                __syncthreads();
                if (on) {
                    // column a of G = B_j'T
                    for (int k = 0; k < nu; ++k) {
                        double s = 0.0;
                        for (int r = 0; r < nx; ++r) s = __builtin_fma(Bm[r * nu + k], Tm[r * ld + a], s);
                        G[k * ld + a] = F[k] * s;
                    }
                }
                for (int e = a; e < nu * nu; e += RC_ROW) {
                    // Re = R_j + B_j'S B_j: a fixed input's row and column are those of the identity
                    const int k = e / nu, l = e - k * nu;
                    double s = Rs[e];
                    for (int r = 0; r < nx; ++r) s = __builtin_fma(Bm[r * nu + k], W[r * nu + l], s);
                    Re[e] = F[k] * F[l] * s + (k == l ? 1.0 - F[k] : 0.0);
                }
                __syncthreads();
                // Cholesky factor of Re, column by column: lane i holds row i.  A pivot that is not positive gives NaN, nothing waits on it.
                for (int q = 0; q < nu; ++q) {
                    double dq = Re[q * nu + q];
                    for (int m = 0; m < q; ++m) dq = __builtin_fma(-Re[q * nu + m], Re[q * nu + m], dq);
                    const double ri = 1.0 / sqrt(dq);
                    if (inp && a > q) {
                        double s = Re[a * nu + q];
                        for (int m = 0; m < q; ++m) s = __builtin_fma(-Re[a * nu + m], Re[q * nu + m], s);
                        Re[a * nu + q] = s * ri;
                    }
                    if (a == q) Di[q] = ri;
                    __syncthreads();
                }
                if (on) {
                    // column a of K_j = Re^-1 G, in place; then column a of Acl_j = A - B K_j
                    for (int k = 0; k < nu; ++k) {
                        double s = G[k * ld + a];
                        for (int m = 0; m < k; ++m) s = __builtin_fma(-Re[k * nu + m], G[m * ld + a], s);
                        G[k * ld + a] = s * Di[k];
                    }
                    for (int k = nu - 1; k >= 0; --k) {
                        double s = G[k * ld + a];
                        for (int m = k + 1; m < nu; ++m) s = __builtin_fma(-Re[m * nu + k], G[m * ld + a], s);
                        const double v = F[k] != 0.0 ? s * Di[k] : 0.0;
                        G[k * ld + a] = v;
                        Kst[(j * nu + k) * nx + a] = v;
                    }
                    for (int r = 0; r < nx; ++r) {
                        double s = Am[r * ld + a];
                        for (int k = 0; k < nu; ++k) s = __builtin_fma(-Bm[r * nu + k], G[k * ld + a], s);
                        C[r * ld + a] = s;
                    }
                }
                __syncthreads();
                if (on) {
                    // row a of S <- Q + A'S Acl_j = Q + T'Acl_j
                    for (int c = 0; c < nx; ++c) {
                        double s = Qs[a * nx + c];
                        for (int m = 0; m < nx; ++m) s = __builtin_fma(Tm[m * ld + a], C[m * ld + c], s);
                        S[a * ld + c] = s;
                    }
                }
                __syncthreads();
            }

            kfree = wave_free;
            // ---- ut_0 = 1/2 f_0 Re_0^-1 f_0 w_t from the factor of stage 0, which Re, Di and F still hold ----
            if (inp) Y[a] = F[a] != 0.0 ? Wt[a] : 0.0;
            if (on) Xt[a] = 0.0;
            __syncthreads();
            if (a == 0) {
                for (int k = 0; k < nu; ++k) {
                    double s = Y[k];
                    for (int m = 0; m < k; ++m) s = __builtin_fma(-Re[k * nu + m], Y[m], s);
                    Y[k] = s * Di[k];
                }
                for (int k = nu - 1; k >= 0; --k) {
                    double s = Y[k];
                    for (int m = k + 1; m < nu; ++m) s = __builtin_fma(-Re[m * nu + k], Y[m], s);
                    Y[k] = s * Di[k];
                }
            }
            __syncthreads();
            if (inp) Ut[a] = F[a] != 0.0 ? 0.5 * Y[a] : 0.0;

            // ---- the adjoint problem rolled forwards: lane k < nu forms ut_j[k], lane a < nx forms xt_{j+1}[a] ----
            for (int j = 0; j < N; ++j) {
                if (j > 0 && inp) {
                    double s = 0.0;
                    for (int c = 0; c < nx; ++c) s = __builtin_fma(Kst[(j * nu + a) * nx + c], Xt[j * nx + c], s);
                    Ut[j * nu + a] = 0.0 - s;
                }
                __syncthreads();
                if (on) {
                    double s = 0.0;
                    for (int c = 0; c < nx; ++c) s = __builtin_fma(Am[a * ld + c], Xt[j * nx + c], s);
                    for (int k = 0; k < nu; ++k) s = __builtin_fma(Bm[a * nu + k], Ut[j * nu + k], s);
                    Xt[(j + 1) * nx + a] = s;
                }
                __syncthreads();
            }

            // ---- the adjoint costate backwards, and the sums (gVN = 0): at step i the state terms of stage i, then, with the costate of
            //      stage i in place, the input terms of stage i - 1.  Every lane adds to its own entries of the row's image ----
            if (on) m0[a] = 0.0;
            for (int i = N; i >= 1; --i) {
                double u = 0.0;
                if (on) d[a] = Xp[i * nx + a] - sh[p.so.xref + a * N + i - 1];
                if (inp) {
                    u = Up[a * N + i - 1];
                    ds[a] = u - sh[p.so.uref + a * N + i - 1];
                }
                __syncthreads();
                const double *xti = Xt + i * nx, *utp = Ut + (i - 1) * nu;
                if (on) {
                    const double *Wm = i == N ? Ps : Qs;
                    double *dst = i == N ? aP : aQ;
                    double r = 0.0, r2 = 0.0;
                    for (int c = 0; c < nx; ++c) r = __builtin_fma(Wm[a * nx + c], xti[c], r);
                    for (int m = 0; m < nx; ++m) r2 = __builtin_fma(Am[m * ld + a], m0[m], r2);
                    m1[a] = 2.0 * r + r2;
                    aXr[i - 1] += 2.0 * r;
                    const double ea = d[a], pe = 0.0 - xti[a];
                    for (int c = 0; c < nx; ++c) dst[c] = __builtin_fma(pe, d[c], __builtin_fma(-ea, xti[c], dst[c]));
                }
                __syncthreads();
                if (inp) {
                    double r = 0.0, r2 = 0.0;
                    for (int l = 0; l < nu; ++l) r = __builtin_fma(Rs[a * nu + l], utp[l], r);
                    for (int m = 0; m < nx; ++m) r2 = __builtin_fma(Bm[m * nu + a], m1[m], r2);
                    aUr[i - 1] += 2.0 * r;
                    const double da = ds[a], pd = 0.0 - utp[a];
                    for (int l = 0; l < nu; ++l) aR[l] = __builtin_fma(pd, ds[l], __builtin_fma(-da, utp[l], aR[l]));
                    // the entry's own bound moves with it: -rt, and at stage 0 the entry is u_t[k] itself
                    double cb = 0.0 - (2.0 * r + r2);
                    if (i == 1) cb += wk;
                    *aLb += (u == lbk || u == lo) ? cb : 0.0;
                    *aUb += (u == ubk || u == hi) ? cb : 0.0;
                }
                __syncthreads();
                double *sw = m0; m0 = m1; m1 = sw;
            }
            // gx_t = -A'lt_1
            if (on) {
                double r2 = 0.0;
                for (int m = 0; m < nx; ++m) r2 = __builtin_fma(Am[m * ld + a], m0[m], r2);
                gxt = 0.0 - r2;
            }
        } else if (inp) {
            // every stage-0 input of the wavefront on a bound: the adjoint plan is zero, and what is left of the step's term is w_t[k]
            // at the bound u_t[k] sits on
            *aLb += (u0 == lbk || u0 == lo) ? wk : 0.0;
            *aUb += (u0 == ubk || u0 == hi) ? wk : 0.0;
        }

        // ---- l_t = gX_t + 2 gam Q x_t + A_true'l_{t+1} + gx_t ----
        if (on) {
            double s = 0.0, s2 = 0.0;
            for (int c = 0; c < nx; ++c) s = __builtin_fma(Qs[a * nx + c], Xp[c], s);
            for (int m = 0; m < nx; ++m) s2 = __builtin_fma(Atm[m * ld + a], Ln[m], s2);
            Lc[a] = ((gx + 2.0 * gam * s) + s2) + gxt;
        }
        __syncthreads();
        double *sw = Ln; Ln = Lc; Lc = sw;
    }

    // ---- what the row's image holds goes out ----
    if (!p.reduce) {
        if (valid) {
#pragma unroll
            for (int w = 0; w < RC_OUTS; ++w) {
                double *out = p.out[w];
                if (!out) continue;
                const int cnt = o.acc[w + 1] - o.acc[w];
                for (int e = a; e < cnt; e += RC_ROW) out[(long long)e * Bsz + b] = bad ? nan : acc[o.acc[w] + e];
            }
        }
        return;
    }
    // reduced: an instance left out (status 2 at a step, or a row past the end) adds 0.0; the four rows' images added in the order of
    // the rows, one vector of partial sums per wavefront
    const bool drop = bad || !valid;
    for (int e = a; e < M; e += RC_ROW) acc[e] = drop ? 0.0 : acc[e];
    if (a == 0) acc[M] = (bad && valid) ? 1.0 : 0.0;
    __syncthreads();
    const double *a0 = lds_rcgrad + o.shared + o.Acc;
    for (int e = t0; e <= M; e += RC_THREADS)
        p.part[(long long)e * gridDim.x + blockIdx.x] = ((a0[e] + a0[o.inst + e]) + a0[2 * o.inst + e]) + a0[3 * o.inst + e];
}

// entry e of the sums (the last one: the count of instances left out) = the partial sums of every wavefront in a fixed order: lane t adds
// those of the wavefronts t, t + 64, ... in ascending order, lane 0 then adds the 64 lanes' sums in ascending order
struct RCGradFinish {
    const double *part;
    long long blocks;
    int off[RC_OUTS + 1];
    double *out[RC_OUTS];
    long long *nskipped;
};

__global__ void __launch_bounds__(64) lqmpc_rollout_cost_grad_finish_kernel(const RCGradFinish f)
{
    __shared__ double lane_sum[64];
    const int e = blockIdx.x, t = threadIdx.x;
    double s = 0.0;
    for (long long g = t; g < f.blocks; g += 64) s += f.part[(long long)e * f.blocks + g];
    lane_sum[t] = s;
    __syncthreads();
    if (t != 0) return;
    double tot = 0.0;
    for (int q = 0; q < 64; ++q) tot += lane_sum[q];
    if (e == f.off[RC_OUTS]) {
        if (f.nskipped) *f.nskipped = (long long)tot;
        return;
    }
    double *dst = nullptr;
#pragma unroll
    for (int w = 0; w < RC_OUTS; ++w)
        if (e >= f.off[w] && e < f.off[w + 1] && f.out[w]) dst = f.out[w] + (e - f.off[w]);
    if (dst) *dst = tot;
}

size_t rcgrad_lds_bytes(int nx, int nu, int N)
{
    const RcLds o = rcgrad_lds(nx, nu, N);
    return sizeof(double) * ((size_t)o.shared + (size_t)RC_IPB * o.inst);
}

bool rcgrad_fits(int nx, int nu, int N) { return rcgrad_lds_bytes(nx, nu, N) <= RC_LDS_LIMIT; }

size_t rcgrad_part_bytes(int nx, int nu, int N, long long Bsz)
{
    return sizeof(double) * (size_t)(rcgrad_lds(nx, nu, N).acc[RC_OUTS] + 1) * (size_t)((Bsz + RC_IPB - 1) / RC_IPB);
}

bool launch_rcgrad(const RCGradParams &p, hipStream_t stream)
{
    if (p.Bsz < 1 || p.T < 1 || p.nx > RC_MAX_NX || p.nu > RC_MAX_NU || p.nu * p.N > RC_SLICE * RC_ROW || !rcgrad_fits(p.nx, p.nu, p.N) ||
        (p.reduce && !p.part))
        return false;
    const size_t bytes = rcgrad_lds_bytes(p.nx, p.nu, p.N);
    if (bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void *)lqmpc_rollout_cost_grad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) {
            fprintf(stderr, "lqmpc: hipFuncSetAttribute(%zu bytes of LDS): %s\n", bytes, hipGetErrorString(e));
            return false;
        }
    }
    const long long blocks = (p.Bsz + RC_IPB - 1) / RC_IPB;
    hipLaunchKernelGGL(lqmpc_rollout_cost_grad_kernel, dim3((unsigned)blocks), dim3(RC_THREADS), bytes, stream, p);
    if (!p.reduce) return true;
    const RcLds o = rcgrad_lds(p.nx, p.nu, p.N);
    RCGradFinish f;
    f.part = p.part; f.blocks = blocks; f.nskipped = p.nskipped;
    for (int w = 0; w <= RC_OUTS; ++w) f.off[w] = o.acc[w];
    for (int w = 0; w < RC_OUTS; ++w) f.out[w] = p.out[w];
    hipLaunchKernelGGL(lqmpc_rollout_cost_grad_finish_kernel, dim3((unsigned)(o.acc[RC_OUTS] + 1)), dim3(64), 0, stream, f);
    return true;
}

}  // namespace lqmpc
