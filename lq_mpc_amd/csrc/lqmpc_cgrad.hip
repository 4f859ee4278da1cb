// lqmpc_cgrad.hip -- the gradient of a loss on (u_0, V_N) with respect to the data a batch shares: the weights Q, R, P, the references
// x_ref, u_ref and the box lb, ub (lqmpc_cost_grad_batch, lqmpc_controller_cost_grad).  A post-pass in a kernel of its own: it reads
// what a plan call has written and touches no solver kernel.  gfx950 (MI355X) only.
//
// Per instance, with w = d loss / d u_0, gam = d loss / d V_N and f_j the free mask of stage j (the sweep, the adjoint plan and the
// costates are those of lqmpc_grad.hip, restated here):
//     S = P;  for j = N-1 .. 0:  Re = R_j + B_j'S B_j,  K_j = Re^-1 B_j'S A,  S <- Q + A'S (A - B_j K_j)          (K_j of all stages kept)
//     ut_0 = 1/2 f_0 Re_0^-1 f_0 w,  xt_0 = 0;  j = 0 .. N-1:  ut_j = -K_j xt_j (j > 0),  xt_{j+1} = A xt_j + B ut_j
//     e_i = x_i - xref_{i-1},  d_i = u_i - uref_i
//     l_N = 2 P e_N,  l_i = 2 Q e_i + A'l_{i+1};   lt_N = 2 P xt_N,  lt_i = 2 Q xt_i + A'lt_{i+1}
//     r_i = 2 R d_i + B'l_{i+1},  rt_i = 2 R ut_i + B'lt_{i+1}
//     gQ = gam x_0 x_0' + sum_{i=1}^{N-1} (gam e_i e_i' - xt_i e_i' - e_i xt_i'),   gP = the same term at i = N
//     gR = sum_{i=0}^{N-1} (gam d_i d_i' - ut_i d_i' - d_i ut_i')
//     gxref[:, i-1] = 2 Q (xt_i - gam e_i)  (P at i = N),   guref[:, i] = 2 R (ut_i - gam d_i)
//     gub[k] = sum over the entries (i, k) on the upper bound of gam r_i[k] - rt_i[k] + (i == 0 ? w_k : 0);  glb likewise
//
// Mapping: that of lqmpc_grad_kernel -- one instance per 16-lane row, four per wavefront, one wavefront per workgroup, so every barrier
// below is a wave-local wait.  Lane a of a row owns row a of S and T = S A, column a of K_j, component a of xt, l and lt, row a of gQ
// and gP and, where a < nu, row a of gR and entry a of glb and gub; gQ and gR are carried in registers (the loops over their columns
// are unrolled to the build limits under uniform guards), gP, gxref and guref are complete when they are formed.
// Two output modes.  Per instance: every value goes to HBM, instance-minor.  Reduced: the grid is bounded (cgrad_blocks), a wavefront
// walks its groups of four instances in ascending order, every row adds what it forms to an LDS image of the sums of its own, in the
// order it forms it; at the end the four images are added in the order of the rows and the wavefront writes one vector of partial sums,
// which lqmpc_cost_grad_finish_kernel adds in a fixed order.  No atomics: the same data give the same bits.
// The face rule is that of lqmpc_sens.hip: bit for bit lb or c - h is lower, ub or c + h is upper.  Nothing branches on a computed
// value: NaN flows through; an instance with status 2 gets NaN in every output (per instance) or adds nothing and is counted
// (reduced), by a select where the value is handed over; rows and right-hand sides of fixed inputs are selected to 0.0, so an
// instance whose stage 0 is saturated and whose gam is 0 has exact zeros in gQ, gP, gR, gxref and guref, and w_k in glb[k] + gub[k].
#include "lqmpc_launch.h"

#include <cstdio>

namespace lqmpc {

namespace {

constexpr int CG_ROW = 16;                   // lanes per instance
constexpr int CG_IPB = 4;                    // instances per workgroup (one wavefront)
constexpr int CG_THREADS = CG_ROW * CG_IPB;
constexpr int CG_MAX_NX = 16, CG_MAX_NU = 8; // the build limits of include/lqmpc.h: the register rows of gQ and gR
constexpr size_t CG_LDS_LIMIT = 160 * 1024;
constexpr int CG_CUS = 256;                  // the bounded grid of the reduced mode: CG_CUS * min(CG_WAVES, images that fit one CU's LDS)
constexpr int CG_WAVES = 16;
enum { CG_Q, CG_R, CG_P, CG_LB, CG_UB, CG_XREF, CG_UREF, CG_OUTS };

// LDS image in doubles: [Q | R | P] once, then per instance [A | S | T | C | B | W | G | Re | Di | F | Y | V | Kst | Xt | Ut] and, in the
// reduced mode, [the sums | the count of instances left out]
struct CgLds {
    int ld;                                  // row stride of the nx-wide matrices (odd)
    int Q, R, P, shared;
    int A, S, T, C, B, W, G, Re, Di, F, Y, V, K, Xt, Ut, Acc, inst;
    int acc[CG_OUTS + 1];                    // offsets of the seven sums in the image of the sums; acc[CG_OUTS] = their number
};

__host__ __device__ inline CgLds cg_lds(int nx, int nu, int N, int reduce)
{
    CgLds o;
    o.ld = nx | 1;
    int e = 0;
    o.Q = e; e += nx * nx;
    o.R = e; e += nu * nu;
    o.P = e; e += nx * nx;
    o.shared = e;
    e = 0;
    o.acc[CG_Q] = e; e += nx * nx;
    o.acc[CG_R] = e; e += nu * nu;
    o.acc[CG_P] = e; e += nx * nx;
    o.acc[CG_LB] = e; e += nu;
    o.acc[CG_UB] = e; e += nu;
    o.acc[CG_XREF] = e; e += nx * N;
    o.acc[CG_UREF] = e; e += nu * N;
    o.acc[CG_OUTS] = e;
    e = 0;
    o.A = e; e += nx * o.ld;                 // A, row-major
    o.S = e; e += nx * o.ld;                 // the Riccati matrix
    o.T = e; e += nx * o.ld;                 // S A
    o.C = e; e += nx * o.ld;                 // Acl_j
    o.B = e; e += nx * nu;
    o.W = e; e += nx * nu;                   // S B
    o.G = e; e += nu * o.ld;                 // B_j'S A, then K_j in place
    o.Re = e; e += nu * nu;                  // Re, then its Cholesky factor below the diagonal
    o.Di = e; e += nu;                       // reciprocals of the factor's diagonal
    o.F = e; e += nu;                        // free mask of the stage, 1.0 / 0.0
    o.Y = e; e += nu;                        // the solve for ut_0; backward pass: d_i
    o.V = e; e += 6 * nx;                    // backward pass: e_i, x_0, and l, lt of two stages
    o.K = e; e += N * nu * nx;               // K_j of every stage
    o.Xt = e; e += (N + 1) * nx;             // xt_0 .. xt_N
    o.Ut = e; e += N * nu;                   // ut_0 .. ut_{N-1}
    o.Acc = e; e += reduce ? o.acc[CG_OUTS] + 1 : 0;
    o.inst = e;
    return o;
}

// hands one value over: to HBM (NaN for an instance with status 2), or to the row's image of the sums (nothing for such an instance)
template <int WHICH>
__device__ __forceinline__ void cg_put(const CGradParams &p, const CgLds &o, double *acc, int idx, long long b, bool live, bool bad, double v)
{
    if (p.reduce) {
        acc[o.acc[WHICH] + idx] += (bad || !live) ? 0.0 : v;
    } else if (p.out[WHICH] && live) {
        p.out[WHICH][(long long)idx * p.Bsz + b] = bad ? __builtin_nan("") : v;
    }
}

}  // namespace

__global__ void __launch_bounds__(CG_THREADS) lqmpc_cost_grad_kernel(const CGradParams p)
{
    extern __shared__ double lds_cgrad[];
    const int nx = p.nx, nu = p.nu, N = p.N;
    const int t = threadIdx.x;
    const CgLds o = cg_lds(nx, nu, N, p.reduce);
    const int ld = o.ld;
    const double *sh = p.sh;
    double *Qs = lds_cgrad + o.Q, *Rs = lds_cgrad + o.R, *Ps = lds_cgrad + o.P;
    const int M = o.acc[CG_OUTS];

    for (int e = t; e < nx * nx; e += CG_THREADS) { Qs[e] = sh[p.so.Q + e]; Ps[e] = sh[p.so.P + e]; }
    for (int e = t; e < nu * nu; e += CG_THREADS) Rs[e] = sh[p.so.R + e];
    if (p.reduce)
        for (int r = 0; r < CG_IPB; ++r)
            for (int e = t; e <= M; e += CG_THREADS) lds_cgrad[o.shared + r * o.inst + o.Acc + e] = 0.0;
    __syncthreads();

    // a wavefront's groups of four instances in ascending order (per instance: the grid has one wavefront per group)
    const long long groups = (p.Bsz + CG_IPB - 1) / CG_IPB;
    for (long long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    // the lane's place is taken afresh in every turn, so that nothing of a group's work is kept in registers across the groups
    int lane = t;
    long long Bsz = p.Bsz;
    asm volatile("" : "+v"(lane), "+s"(Bsz));
    const int a = lane & (CG_ROW - 1), row = lane / CG_ROW;
    const bool on = a < nx, inp = a < nu;
    double *I = lds_cgrad + o.shared + row * o.inst;
    double *Am = I + o.A, *S = I + o.S, *T = I + o.T, *C = I + o.C, *Bm = I + o.B, *W = I + o.W, *G = I + o.G;
    double *Re = I + o.Re, *Di = I + o.Di, *F = I + o.F, *Y = I + o.Y, *V = I + o.V, *Kst = I + o.K, *Xt = I + o.Xt, *Ut = I + o.Ut;
    double *acc = I + o.Acc;
    // the four forms a bound can come out in (include/lqmpc.h, the plan's contract)
    double lbk = 0.0, ubk = 0.0, lo = 0.0, hi = 0.0;
    if (inp) {
        lbk = sh[p.so.lb + a]; ubk = sh[p.so.ub + a];
        const double ctr = 0.5 * (ubk + lbk), h = 0.5 * (ubk - lbk);
        lo = ctr - h; hi = ctr + h;
    }
    // the tail of the batch: a row past the end works on the last instance and hands nothing over
    const long long b0 = grp * CG_IPB + row;
    const bool valid = b0 < Bsz;
    const long long b = valid ? b0 : Bsz - 1;
    for (int e = a; e < nx * nx; e += CG_ROW) {
        const int r = e / nx, c = e - r * nx;
        Am[r * ld + c] = p.A[(long long)e * p.sE + b * p.sI];
        S[r * ld + c] = sh[p.so.P + e];
    }
    for (int e = a; e < nx * nu; e += CG_ROW) Bm[e] = p.B[(long long)e * p.sE + b * p.sI];
    const bool bad = p.status ? p.status[b] == 2 : false;
    const double gam = p.gVN ? p.gVN[b] : 0.0;
    double wk = 0.0;
    if (inp && p.gu0) wk = p.gu0[(long long)a * Bsz + b];
    if (p.reduce && a == 0 && valid && bad) acc[M] += 1.0;
    __syncthreads();

    // ---- the masked Riccati sweep, backwards over the stages (lqmpc_sens.hip) ----
    for (int j = N - 1; j >= 0; --j) {
        if (inp) {
            const double u = p.Uplan[((long long)a * N + j) * Bsz + b];
            F[a] = (u == lbk || u == ubk || u == lo || u == hi) ? 0.0 : 1.0;
        }
        if (on) {
            // row a of T = S A and of W = S B
            for (int c = 0; c < nx; ++c) {
                double s = 0.0;
                for (int m = 0; m < nx; ++m) s = __builtin_fma(S[a * ld + m], Am[m * ld + c], s);
                T[a * ld + c] = s;
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
                for (int r = 0; r < nx; ++r) s = __builtin_fma(Bm[r * nu + k], T[r * ld + a], s);
                G[k * ld + a] = F[k] * s;
            }
        }
        for (int e = a; e < nu * nu; e += CG_ROW) {
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
                for (int m = 0; m < nx; ++m) s = __builtin_fma(T[m * ld + a], C[m * ld + c], s);
                S[a * ld + c] = s;
            }
        }
        __syncthreads();
    }

    // ---- ut_0 = 1/2 f_0 Re_0^-1 f_0 w from the factor of stage 0, which Re, Di and F still hold: two short substitutions on one lane ----
    if (inp) Y[a] = F[a] != 0.0 ? wk : 0.0;
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

    // ---- the two costate recursions backwards together, and the sums: at step i the state terms of stage i, then, with the costates
    //      of stage i in place, the input terms of stage i - 1 ----
    double gq[CG_MAX_NX], gr[CG_MAX_NU], glb = 0.0, gub = 0.0;
#pragma unroll
    for (int c = 0; c < CG_MAX_NX; ++c) gq[c] = 0.0;
#pragma unroll
    for (int k = 0; k < CG_MAX_NU; ++k) gr[k] = 0.0;
    double *d = V, *xs = V + nx, *l0 = V + 2 * nx, *l1 = V + 3 * nx, *m0 = V + 4 * nx, *m1 = V + 5 * nx, *ds = Y;
    if (on) { l0[a] = 0.0; m0[a] = 0.0; }
    for (int i = N; i >= 1; --i) {
        double u = 0.0;
        if (on) d[a] = p.Xplan[((long long)a * (N + 1) + i) * Bsz + b] - sh[p.so.xref + a * N + i - 1];
        if (inp) {
            u = p.Uplan[((long long)a * N + i - 1) * Bsz + b];
            ds[a] = u - sh[p.so.uref + a * N + i - 1];
        }
        __syncthreads();
        const double *xti = Xt + i * nx, *utp = Ut + (i - 1) * nu;
        if (on) {
            const double *Wm = i == N ? Ps : Qs;
            double s = 0.0, s2 = 0.0, r = 0.0, r2 = 0.0;
            for (int c = 0; c < nx; ++c) { s = __builtin_fma(Wm[a * nx + c], d[c], s); r = __builtin_fma(Wm[a * nx + c], xti[c], r); }
            for (int m = 0; m < nx; ++m) { s2 = __builtin_fma(Am[m * ld + a], l0[m], s2); r2 = __builtin_fma(Am[m * ld + a], m0[m], r2); }
            l1[a] = 2.0 * s + s2; m1[a] = 2.0 * r + r2;
            cg_put<CG_XREF>(p, o, acc, a * N + i - 1, b, valid, bad, 2.0 * (r - gam * s));
            const double ea = d[a], pe = gam * ea - xti[a];
            if (i == N) {
                for (int c = 0; c < nx; ++c) cg_put<CG_P>(p, o, acc, a * nx + c, b, valid, bad, __builtin_fma(pe, d[c], 0.0 - ea * xti[c]));
            } else {
#pragma unroll
                for (int c = 0; c < CG_MAX_NX; ++c)
                    if (c < nx) gq[c] = __builtin_fma(pe, d[c], __builtin_fma(-ea, xti[c], gq[c]));
            }
        }
        __syncthreads();
        if (inp) {
            double s = 0.0, r = 0.0, s2 = 0.0, r2 = 0.0;
            for (int l = 0; l < nu; ++l) { s = __builtin_fma(Rs[a * nu + l], ds[l], s); r = __builtin_fma(Rs[a * nu + l], utp[l], r); }
            for (int m = 0; m < nx; ++m) { s2 = __builtin_fma(Bm[m * nu + a], l1[m], s2); r2 = __builtin_fma(Bm[m * nu + a], m1[m], r2); }
            cg_put<CG_UREF>(p, o, acc, a * N + i - 1, b, valid, bad, 2.0 * (r - gam * s));
            const double da = ds[a], pd = gam * da - utp[a];
#pragma unroll
            for (int l = 0; l < CG_MAX_NU; ++l)
                if (l < nu) gr[l] = __builtin_fma(pd, ds[l], __builtin_fma(-da, utp[l], gr[l]));
            // the entry's own bound moves with it: gam r - rt, and at stage 0 the entry is u_0[k] itself
            double cb = __builtin_fma(gam, 2.0 * s + s2, 0.0 - (2.0 * r + r2));
            if (i == 1) cb += wk;
            glb += (u == lbk || u == lo) ? cb : 0.0;
            gub += (u == ubk || u == hi) ? cb : 0.0;
        }
        __syncthreads();
        double *sw = l0; l0 = l1; l1 = sw;
        sw = m0; m0 = m1; m1 = sw;
    }

    // ---- what the registers hold: gQ takes gam x_0 x_0' ----
    if (on) xs[a] = p.Xplan[((long long)a * (N + 1)) * Bsz + b];
    __syncthreads();
    if (on) {
        const double px = gam * xs[a];
#pragma unroll
        for (int c = 0; c < CG_MAX_NX; ++c)
            if (c < nx) cg_put<CG_Q>(p, o, acc, a * nx + c, b, valid, bad, __builtin_fma(px, xs[c], gq[c]));
    }
    if (inp) {
#pragma unroll
        for (int l = 0; l < CG_MAX_NU; ++l)
            if (l < nu) cg_put<CG_R>(p, o, acc, a * nu + l, b, valid, bad, gr[l]);
        cg_put<CG_LB>(p, o, acc, a, b, valid, bad, glb);
        cg_put<CG_UB>(p, o, acc, a, b, valid, bad, gub);
    }
    __syncthreads();
    }

    // ---- reduced: the four rows' images added in the order of the rows, one vector of partial sums per wavefront ----
    if (p.reduce) {
        const double *a0 = lds_cgrad + o.shared + o.Acc;
        for (int e = t; e <= M; e += CG_THREADS)
            p.part[(long long)e * gridDim.x + blockIdx.x] = ((a0[e] + a0[o.inst + e]) + a0[2 * o.inst + e]) + a0[3 * o.inst + e];
    }
}

// entry e of the sums (the last one: the count of instances left out) = the partial sums of every wavefront in a fixed order: lane t adds
// those of the wavefronts t, t + 64, ... in ascending order, lane 0 then adds the 64 lanes' sums in ascending order
struct CGradFinish {
    const double *part;
    long long blocks;
    int off[CG_OUTS + 1];
    double *out[CG_OUTS];
    long long *nskipped;
};

__global__ void __launch_bounds__(64) lqmpc_cost_grad_finish_kernel(const CGradFinish f)
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
    if (e == f.off[CG_OUTS]) {
        if (f.nskipped) *f.nskipped = (long long)tot;
        return;
    }
    double *dst = nullptr;
#pragma unroll
    for (int w = 0; w < CG_OUTS; ++w)
        if (e >= f.off[w] && e < f.off[w + 1] && f.out[w]) dst = f.out[w] + (e - f.off[w]);
    if (dst) *dst = tot;
}

size_t cgrad_lds_bytes(int nx, int nu, int N, int reduce)
{
    const CgLds o = cg_lds(nx, nu, N, reduce);
    return sizeof(double) * ((size_t)o.shared + (size_t)CG_IPB * o.inst);
}

bool cgrad_fits(int nx, int nu, int N, int reduce) { return cgrad_lds_bytes(nx, nu, N, reduce) <= CG_LDS_LIMIT; }

long long cgrad_blocks(int nx, int nu, int N, long long Bsz, int reduce)
{
    const long long groups = (Bsz + CG_IPB - 1) / CG_IPB;
    if (!reduce) return groups;
    long long per_cu = (long long)(CG_LDS_LIMIT / cgrad_lds_bytes(nx, nu, N, 1));
    per_cu = per_cu < 1 ? 1 : per_cu > CG_WAVES ? CG_WAVES : per_cu;
    return groups < CG_CUS * per_cu ? groups : CG_CUS * per_cu;
}

size_t cgrad_part_bytes(int nx, int nu, int N, long long Bsz)
{
    return sizeof(double) * (size_t)(cg_lds(nx, nu, N, 1).acc[CG_OUTS] + 1) * (size_t)cgrad_blocks(nx, nu, N, Bsz, 1);
}

bool launch_cgrad(const CGradParams &p, hipStream_t stream)
{
    const int red = p.reduce ? 1 : 0;
    if (p.Bsz < 1 || p.nx > CG_MAX_NX || p.nu > CG_MAX_NU || !cgrad_fits(p.nx, p.nu, p.N, red) || (red && !p.part)) return false;
    const size_t bytes = cgrad_lds_bytes(p.nx, p.nu, p.N, red);
    if (bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void *)lqmpc_cost_grad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) {
            fprintf(stderr, "lqmpc: hipFuncSetAttribute(%zu bytes of LDS): %s\n", bytes, hipGetErrorString(e));
            return false;
        }
    }
    const long long blocks = cgrad_blocks(p.nx, p.nu, p.N, p.Bsz, red);
    hipLaunchKernelGGL(lqmpc_cost_grad_kernel, dim3((unsigned)blocks), dim3(CG_THREADS), bytes, stream, p);
    if (!red) return true;
    const CgLds o = cg_lds(p.nx, p.nu, p.N, 1);
    CGradFinish f;
    f.part = p.part; f.blocks = blocks; f.nskipped = p.nskipped;
    for (int w = 0; w <= CG_OUTS; ++w) f.off[w] = o.acc[w];
    for (int w = 0; w < CG_OUTS; ++w) f.out[w] = p.out[w];
    hipLaunchKernelGGL(lqmpc_cost_grad_finish_kernel, dim3((unsigned)(o.acc[CG_OUTS] + 1)), dim3(64), 0, stream, f);
    return true;
}

}  // namespace lqmpc
