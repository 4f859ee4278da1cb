// lqmpc_rgrad.hip -- the closed loop with a tape, and the gradient of a loss on that loop -- J_T, every x_t and every u_t -- with respect
// to the model matrices A and B, the plant matrices A_true and B_true and the initial state x_0 of every instance
// (lqmpc_rollout_tape_batch, lqmpc_rollout_grad_batch).  Two kernels beside the solver kernels, which they do not touch.  gfx950 only.
//
// lqmpc_plant_step_kernel: what the tape forward runs behind the plan call of step t.  One lane per instance:
//     x_{t+1} = A_true x_t + B_true u_0,   J_T += x_{t+1}'Q x_{t+1} + u_0'R u_0   (x_0'Q x_0 first, at t = 0),   row t + 1 of X, row t of U.
//
// lqmpc_rollout_grad_kernel: the tape walked backwards with the plant's costate.  Per instance, with gam = d loss / d J_T:
//     l_T = gX_T + 2 gam Q x_T
//     t = T-1 .. 0:   w_t = gU_t + 2 gam R u_t + B_true'l_{t+1}
//                     gA_true += l_{t+1} x_t',  gB_true += l_{t+1} u_t'
//                     the plan of step t re-rolled on the model from x_t and slice t of the tape:  x_0 = x_t,  x_{i+1} = A x_i + B u_i
//                     the model gradient of lqmpc_grad.hip for gu0 = w_t, gVN = 0, restated (f_j the free mask of stage j):
//                         S = P;  j = N-1 .. 0:  Re = R_j + B_j'S B_j,  K_j = Re^-1 B_j'S A,  S <- Q + A'S (A - B_j K_j)
//                         ut_0 = 1/2 f_0 Re_0^-1 f_0 w_t,  xt_0 = 0;  ut_j = -K_j xt_j (j > 0),  xt_{j+1} = A xt_j + B ut_j
//                         l_N = 2 P (x_N - xref_{N-1}),  l_i = 2 Q (x_i - xref_{i-1}) + A'l_{i+1};   lt_N = 2 P xt_N,  lt_i = 2 Q xt_i + A'lt_{i+1}
//                         gA -= sum_i lt_{i+1} x_i' + l_{i+1} xt_i',   gB -= sum_i lt_{i+1} u_i' + l_{i+1} ut_i',   gx_t = -A'lt_1
//                     l_t = gX_t + 2 gam Q x_t + A_true'l_{t+1} + gx_t
//     gx0 = l_0
//
// Mapping: that of lqmpc_plan_grad_kernel -- one instance per 16-lane row, four per wavefront, one wavefront per workgroup, so every
// barrier below is a wave-local wait.  Lane a of a row owns row a of S and T = S A, column a of K_j, component a of the costates, and
// row a of gA and gB, which it carries in registers across all T steps (the loops over their columns are unrolled to the build limits
// under uniform guards), and row a of gA_true and gB_true, which it keeps in LDS: 48 more registers would cost a wavefront per SIMD.
// The model and the plant of an instance, K_j of every stage, the plan of the step and its states sit in dynamic LDS, loaded once per
// instance; Q, R, P once per workgroup.  Slice t - 1 of the tape, x_{t-1} and the cotangents
// of step t - 1 are read from HBM into registers while step t is worked on.  No HBM workspace.
// The face rule is that of lqmpc_sens.hip: bit for bit lb, ub, c - h or c + h.  Nothing branches on a computed value: NaN flows through
// and is what gets stored; an instance with status 2 at any step gets NaN in every output.  The one skip is wave-uniform: a step at
// which every stage-0 input of all four instances of the wavefront sits on a bound (a ballot over the bits of the tape) has ut = 0,
// xt = 0 and lt = 0, adds exact zeros and is passed over.  The gains of the all-free face do not depend on t: where all four plans of
// the wavefront are wholly free at a step and were at the step worked on before it, the sweep is not run again (the same bits).
#include "lqmpc_launch.h"

#include <cstdio>

namespace lqmpc {

namespace {

constexpr int RG_ROW = 16;                   // lanes per instance
constexpr int RG_IPB = 4;                    // instances per workgroup (one wavefront)
constexpr int RG_THREADS = RG_ROW * RG_IPB;
constexpr int RG_MAX_NX = 16, RG_MAX_NU = 8; // the build limits of include/lqmpc.h: the register rows of gA and gB
constexpr int RG_SLICE = 8;                  // registers of a lane that hold its share of a slice: N nu <= 128 = 16 x 8
constexpr size_t RG_LDS_LIMIT = 160 * 1024;
// wavefronts per SIMD the register allocation is held to: the kernel waits on LDS and on its barriers, not on arithmetic, so more
// wavefronts pay even at the price of 43 spilled registers (C3 x 65 536, T = 30: 32.3 ms at one, 16.8 ms at two, 13.6 ms at three;
// DESIGN.md section 4.14)
#define RG_WAVES 3

// LDS image in doubles: [Q | R | P] once, then per instance
// [A | At | S | T | C | B | Bt | W | G | Re | Di | F | Y | Wt | V | L | Gat | Gbt | Kst | Xt | Ut | Xp | Up]
struct RGradLds {
    int ld;                                  // row stride of the nx-wide matrices (odd)
    int Q, R, P, shared;
    int A, At, S, T, C, B, Bt, W, G, Re, Di, F, Y, Wt, V, L, Gat, Gbt, K, Xt, Ut, Xp, Up, inst;
};

__host__ __device__ inline RGradLds rgrad_lds(int nx, int nu, int N)
{
    RGradLds o;
    o.ld = nx | 1;
    int e = 0;
    o.Q = e; e += nx * nx;
    o.R = e; e += nu * nu;
    o.P = e; e += nx * nx;
    o.shared = e;
    e = 0;
    o.A = e; e += nx * o.ld;                 // A, row-major
    o.At = e; e += nx * o.ld;                // A_true, row-major
    o.S = e; e += nx * o.ld;                 // the Riccati matrix
    o.T = e; e += nx * o.ld;                 // S A
    o.C = e; e += nx * o.ld;                 // Acl_j
    o.B = e; e += nx * nu;
    o.Bt = e; e += nx * nu;                  // B_true
    o.W = e; e += nx * nu;                   // S B
    o.G = e; e += nu * o.ld;                 // B_j'S A, then K_j in place
    o.Re = e; e += nu * nu;                  // Re, then its Cholesky factor below the diagonal
    o.Di = e; e += nu;                       // reciprocals of the factor's diagonal
    o.F = e; e += nu;                        // free mask of the stage, 1.0 / 0.0
    o.Y = e; e += nu;                        // the solve for ut_0
    o.Wt = e; e += nu;                       // w_t
    o.V = e; e += 5 * nx;                    // backward pass: the state error, and l, lt of two stages
    o.L = e; e += 2 * nx;                    // the plant's costate of two steps
    o.Gat = e; e += nx * nx;                 // the sum gA_true: lane a adds to its own row
    o.Gbt = e; e += nx * nu;                 // the sum gB_true, likewise
    o.K = e; e += N * nu * nx;               // K_j of every stage
    o.Xt = e; e += (N + 1) * nx;             // xt_0 .. xt_N
    o.Ut = e; e += N * nu;                   // ut_0 .. ut_{N-1}
    o.Xp = e; e += (N + 1) * nx;             // the plan's states x_0 = x_t .. x_N, re-rolled on the model
    o.Up = e; e += N * nu;                   // slice t of the tape, as it lies in HBM: u_i[k] at k N + i
    o.inst = e;
    return o;
}

}  // namespace

__global__ void __launch_bounds__(64) lqmpc_plant_step_kernel(const PlantStepParams p)
{
    const long long b = (long long)blockIdx.x * 64 + threadIdx.x;
    if (b >= p.Bsz) return;
    const int nx = p.nx, nu = p.nu, T = p.T, t = p.t;
    const long long Bsz = p.Bsz;
    const double *Q = p.sh + p.so.Q, *R = p.sh + p.so.R;
    const double *At = p.At + b * p.sI, *Bt = p.Bt + b * p.sI;
    double cost = 0.0;
    if (t == 0) {
        for (int a = 0; a < nx; ++a)
            for (int c = 0; c < nx; ++c) cost += p.x[a * Bsz + b] * Q[a * nx + c] * p.x[c * Bsz + b];
        if (p.X)
            for (int a = 0; a < nx; ++a) p.X[((long long)a * (T + 1)) * Bsz + b] = p.x[a * Bsz + b];
    } else {
        cost = p.JT[b];
    }
    double xn[RG_MAX_NX], u[RG_MAX_NU];
#pragma unroll
    for (int k = 0; k < RG_MAX_NU; ++k) u[k] = k < nu ? p.Uslice[(long long)k * p.N * Bsz + b] : 0.0;
#pragma unroll
    for (int a = 0; a < RG_MAX_NX; ++a) {
        double s = 0.0;
        if (a < nx) {
            for (int c = 0; c < nx; ++c) s += At[(long long)(a * nx + c) * p.sE] * p.x[c * Bsz + b];
#pragma unroll
            for (int k = 0; k < RG_MAX_NU; ++k)
                if (k < nu) s += Bt[(long long)(a * nu + k) * p.sE] * u[k];
            p.xn[a * Bsz + b] = s;
            if (p.X) p.X[((long long)a * (T + 1) + t + 1) * Bsz + b] = s;
        }
        xn[a] = s;
    }
#pragma unroll
    for (int a = 0; a < RG_MAX_NX; ++a)
#pragma unroll
        for (int c = 0; c < RG_MAX_NX; ++c)
            if (a < nx && c < nx) cost += xn[a] * Q[a * nx + c] * xn[c];
#pragma unroll
    for (int k = 0; k < RG_MAX_NU; ++k)
#pragma unroll
        for (int l = 0; l < RG_MAX_NU; ++l)
            if (k < nu && l < nu) cost += u[k] * R[k * nu + l] * u[l];
    p.JT[b] = cost;
    if (p.U) {
#pragma unroll
        for (int k = 0; k < RG_MAX_NU; ++k)
            if (k < nu) p.U[((long long)k * T + t) * Bsz + b] = u[k];
    }
    if (p.status) {
        const int s = p.st[b];
        p.status[b] = t == 0 ? s : (p.status[b] > s ? p.status[b] : s);
    }
    if (p.iters) p.iters[b] = t == 0 ? p.it[b] : p.iters[b] + p.it[b];
}

__global__ void __launch_bounds__(RG_THREADS) __attribute__((amdgpu_waves_per_eu(RG_WAVES, RG_WAVES)))
lqmpc_rollout_grad_kernel(const RGradParams p)
{
    extern __shared__ double lds_rgrad[];
    const int nx = p.nx, nu = p.nu, N = p.N, T = p.T;
    const int t0 = threadIdx.x, a = t0 & (RG_ROW - 1), row = t0 / RG_ROW;
    const RGradLds o = rgrad_lds(nx, nu, N);
    const int ld = o.ld, nv = nu * N;
    const long long Bsz = p.Bsz;
    // the tail of the batch: a row past the end works on the last instance and stores nothing
    const long long b0 = (long long)blockIdx.x * RG_IPB + row;
    const bool valid = b0 < Bsz;
    const long long b = valid ? b0 : Bsz - 1;
    const bool on = a < nx, inp = a < nu;
    const double *sh = p.sh;

    double *Qs = lds_rgrad + o.Q, *Rs = lds_rgrad + o.R, *Ps = lds_rgrad + o.P;
    double *I = lds_rgrad + o.shared + row * o.inst;
    double *Am = I + o.A, *Atm = I + o.At, *S = I + o.S, *Tm = I + o.T, *C = I + o.C, *Bm = I + o.B, *Btm = I + o.Bt, *W = I + o.W;
    double *G = I + o.G, *Re = I + o.Re, *Di = I + o.Di, *F = I + o.F, *Y = I + o.Y, *Wt = I + o.Wt, *V = I + o.V;
    double *Kst = I + o.K, *Xt = I + o.Xt, *Ut = I + o.Ut, *Xp = I + o.Xp, *Up = I + o.Up, *Gat = I + o.Gat, *Gbt = I + o.Gbt;
    double *Ln = I + o.L, *Lc = I + o.L + nx;   // the plant's costate of step t + 1 and of step t

    for (int e = t0; e < nx * nx; e += RG_THREADS) { Qs[e] = sh[p.so.Q + e]; Ps[e] = sh[p.so.P + e]; }
    for (int e = t0; e < nu * nu; e += RG_THREADS) Rs[e] = sh[p.so.R + e];
    for (int e = a; e < nx * nx; e += RG_ROW) {
        const int r = e / nx, c = e - r * nx;
        Am[r * ld + c] = p.A[(long long)e * Bsz + b];
        Atm[r * ld + c] = p.At[(long long)e * p.sE + b * p.sI];
    }
    for (int e = a; e < nx * nu; e += RG_ROW) {
        Bm[e] = p.B[(long long)e * Bsz + b];
        Btm[e] = p.Bt[(long long)e * p.sE + b * p.sI];
    }
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
    double sl[RG_SLICE], xr = 0.0, gxr = 0.0, gur = 0.0;
    int str = 0;
    auto fetch = [&](int t) {
        const double *slice = p.Utape + (long long)t * nv * Bsz;
#pragma unroll
        for (int q = 0; q < RG_SLICE; ++q) {
            const int e = a + q * RG_ROW;
            sl[q] = e < nv ? slice[(long long)e * Bsz + b] : 0.0;
        }
        if (on) {
            xr = p.X[((long long)a * (T + 1) + t) * Bsz + b];
            if (p.gX) gxr = p.gX[((long long)a * (T + 1) + t) * Bsz + b];
        }
        if (inp && p.gU) gur = p.gU[((long long)a * T + t) * Bsz + b];
        if (p.status_tape) str = p.status_tape[(long long)t * Bsz + b];
    };

    // l_T = gX_T + 2 gam Q x_T
    if (on) {
        Xp[a] = p.X[((long long)a * (T + 1) + T) * Bsz + b];
        if (p.gX) gxr = p.gX[((long long)a * (T + 1) + T) * Bsz + b];
    }
    __syncthreads();
    if (on) {
        double s = 0.0;
        for (int c = 0; c < nx; ++c) s = __builtin_fma(Qs[a * nx + c], Xp[c], s);
        Ln[a] = gxr + 2.0 * gam * s;
    }
    gxr = 0.0;
    fetch(T - 1);
    __syncthreads();

    double ga[RG_MAX_NX], gb[RG_MAX_NU];
#pragma unroll
    for (int c = 0; c < RG_MAX_NX; ++c) ga[c] = 0.0;
#pragma unroll
    for (int k = 0; k < RG_MAX_NU; ++k) gb[k] = 0.0;
    if (on) {
        for (int c = 0; c < nx; ++c) Gat[a * nx + c] = 0.0;
        for (int k = 0; k < nu; ++k) Gbt[a * nu + k] = 0.0;
    }
    bool bad = false, kfree = false;            // kfree: Kst, Re, Di and F hold the sweep of the all-free face
    double *d = V, *l0 = V + nx, *l1 = V + 2 * nx, *m0 = V + 3 * nx, *m1 = V + 4 * nx;

    for (int t = T - 1; t >= 0; --t) {
        // ---- step t from the registers into LDS, step t - 1 on its way from HBM ----
        if (on) Xp[a] = xr;
#pragma unroll
        for (int q = 0; q < RG_SLICE; ++q) {
            const int e = a + q * RG_ROW;
            if (e < nv) Up[e] = sl[q];
        }
        const double gx = gxr, gu = gur;
        bad = bad || str == 2;
        if (t > 0) fetch(t - 1);
        __syncthreads();

        // ---- w_t, the plant's two sums, and whether any instance of the wavefront has a free input at stage 0 ----
        bool free0 = false, fixed_any = false;
        if (inp) {
            for (int j = 0; j < N; ++j) {
                const double v = Up[a * N + j];
                fixed_any = fixed_any || v == lbk || v == ubk || v == lo || v == hi;
            }
            const double u = Up[a * N];
            free0 = !(u == lbk || u == ubk || u == lo || u == hi);
            double r = 0.0;
            for (int l = 0; l < nu; ++l) r = __builtin_fma(Rs[a * nu + l], Up[l * N], r);
            double s = gu + 2.0 * gam * r;
            for (int m = 0; m < nx; ++m) s = __builtin_fma(Btm[m * nu + a], Ln[m], s);
            Wt[a] = s;
        }
        if (on) {
            const double lam = Ln[a];
            for (int c = 0; c < nx; ++c) Gat[a * nx + c] = __builtin_fma(lam, Xp[c], Gat[a * nx + c]);
            for (int k = 0; k < nu; ++k) Gbt[a * nu + k] = __builtin_fma(lam, Up[k * N], Gbt[a * nu + k]);
        }
        const bool qp = __ballot(free0) != 0ull;    // wave-uniform: the bits of the tape, not a computed value
        // all four plans wholly free, as at the step worked on before this one: K_j, the factor of stage 0 and F are still those of the
        // all-free face, which does not depend on t, and the sweep is not run again
        const bool wave_free = __ballot(fixed_any) == 0ull;
        const bool sweep = !(wave_free && kfree);
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

            // ---- the masked Riccati sweep, backwards over the stages (lqmpc_grad.hip) ----
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
                for (int e = a; e < nu * nu; e += RG_ROW) {
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

            // ---- the two costate recursions backwards together, and the sums (gVN = 0: the envelope part is absent) ----
            if (on) { l0[a] = 0.0; m0[a] = 0.0; }
            for (int i = N; i >= 1; --i) {
                if (on) d[a] = Xp[i * nx + a] - sh[p.so.xref + a * N + i - 1];
                __syncthreads();
                if (on) {
                    const double *Wm = i == N ? Ps : Qs;
                    const double *xti = Xt + i * nx, *xtp = Xt + (i - 1) * nx, *utp = Ut + (i - 1) * nu, *xs = Xp + (i - 1) * nx;
                    double s = 0.0, s2 = 0.0, r = 0.0, r2 = 0.0;
                    for (int c = 0; c < nx; ++c) { s = __builtin_fma(Wm[a * nx + c], d[c], s); r = __builtin_fma(Wm[a * nx + c], xti[c], r); }
                    for (int m = 0; m < nx; ++m) { s2 = __builtin_fma(Am[m * ld + a], l0[m], s2); r2 = __builtin_fma(Am[m * ld + a], m0[m], r2); }
                    const double lam = 2.0 * s + s2, lamt = 2.0 * r + r2;
                    l1[a] = lam; m1[a] = lamt;
#pragma unroll
                    for (int c = 0; c < RG_MAX_NX; ++c)
                        if (c < nx) ga[c] = __builtin_fma(-lamt, xs[c], __builtin_fma(-lam, xtp[c], ga[c]));
#pragma unroll
                    for (int k = 0; k < RG_MAX_NU; ++k)
                        if (k < nu) gb[k] = __builtin_fma(-lamt, Up[k * N + i - 1], __builtin_fma(-lam, utp[k], gb[k]));
                }
                __syncthreads();
                double *sw = l0; l0 = l1; l1 = sw;
                sw = m0; m0 = m1; m1 = sw;
            }
            // gx_t = -A'lt_1
            if (on) {
                double r2 = 0.0;
                for (int m = 0; m < nx; ++m) r2 = __builtin_fma(Am[m * ld + a], m0[m], r2);
                gxt = 0.0 - r2;
            }
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

    // ---- stores: Ln holds l_0 ----
    if (on && valid) {
        if (p.gx0) p.gx0[(long long)a * Bsz + b] = bad ? nan : Ln[a];
        if (p.gA) {
#pragma unroll
            for (int c = 0; c < RG_MAX_NX; ++c)
                if (c < nx) p.gA[((long long)a * nx + c) * Bsz + b] = bad ? nan : ga[c];
        }
        if (p.gAt)
            for (int c = 0; c < nx; ++c) p.gAt[((long long)a * nx + c) * Bsz + b] = bad ? nan : Gat[a * nx + c];
        if (p.gB) {
#pragma unroll
            for (int k = 0; k < RG_MAX_NU; ++k)
                if (k < nu) p.gB[((long long)a * nu + k) * Bsz + b] = bad ? nan : gb[k];
        }
        if (p.gBt)
            for (int k = 0; k < nu; ++k) p.gBt[((long long)a * nu + k) * Bsz + b] = bad ? nan : Gbt[a * nu + k];
    }
}

void launch_plant_step(const PlantStepParams &p, hipStream_t stream)
{
    const long long blocks = (p.Bsz + 63) / 64;
    hipLaunchKernelGGL(lqmpc_plant_step_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, p);
}

size_t rgrad_lds_bytes(int nx, int nu, int N)
{
    const RGradLds o = rgrad_lds(nx, nu, N);
    return sizeof(double) * ((size_t)o.shared + (size_t)RG_IPB * o.inst);
}

bool rgrad_fits(int nx, int nu, int N) { return rgrad_lds_bytes(nx, nu, N) <= RG_LDS_LIMIT; }

bool launch_rgrad(const RGradParams &p, hipStream_t stream)
{
    if (p.Bsz < 1 || p.T < 1 || p.nx > RG_MAX_NX || p.nu > RG_MAX_NU || p.nu * p.N > RG_SLICE * RG_ROW || !rgrad_fits(p.nx, p.nu, p.N)) return false;
    const size_t bytes = rgrad_lds_bytes(p.nx, p.nu, p.N);
    if (bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void *)lqmpc_rollout_grad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) {
            fprintf(stderr, "lqmpc: hipFuncSetAttribute(%zu bytes of LDS): %s\n", bytes, hipGetErrorString(e));
            return false;
        }
    }
    const long long blocks = (p.Bsz + RG_IPB - 1) / RG_IPB;
    hipLaunchKernelGGL(lqmpc_rollout_grad_kernel, dim3((unsigned)blocks), dim3(RG_THREADS), bytes, stream, p);
    return true;
}

}  // namespace lqmpc
