// lqmpc_poly.hip -- the MPC problem with polytopic input constraints Fu u_i <= 1 (lqmpc_solve_poly_batch, lqmpc_rollout_poly_batch, and
// the prepared controller lqmpc_poly_controller_*): any (m, nu) matrix Fu, not only the rows of a box.  A kernel file of its own; it
// shares nothing with the box kernels but the parameter conventions.  gfx950 (MI355X) only.
//
// Per instance, with n = N nu:   min U'HU + 2g'U   s.t.  (I_N (x) Fu) U <= 1,   H = Gamma'Qbar Gamma + Rbar,  g = Gamma'Qbar (Phi x0 - xref) - Rbar uref.
// Method: Goldfarb-Idnani, the dual active-set method from the unconstrained minimiser.  With G = 2H = LL' and J = L^-T (J J' = G^-1),
// the active normals N_A are kept as J'N_A = [Rf; 0], Rf upper triangular.  A pass picks the most violated row p of the normalised
// constraints, forms d = J'n_p, the primal direction z = -J2 d2 (the columns of J past the active ones) and the dual direction
// r = Rf^-1 d1, and takes the shorter of the step t1 that brings a multiplier to zero (that row is dropped: Givens rotations on the
// columns of J and the rows of Rf) and the step t2 = violation / d2'd2 that makes row p active (it is added: one Householder reflection
// of J2).  d2'd2 <= 1e-13 d'd means the row depends on the active ones: the step is then in the multipliers alone.
//
// Mapping: one instance per wavefront, one wavefront per workgroup, so every barrier below is a wave-local wait (the idiom of
// lqmpc_sens.hip).  Lane i owns row i of J (n <= 64), lane k < q the multiplier and the row id of active row k.  The matrices sit in
// dynamic LDS (poly_lds: one layout function for host and device), J with row stride n | 1, the pristine J = L^-T and Rf packed.
// Set-up, once per instance: W_k = A^k B, S_c = Q + A'S_{c+1}A, block (c1, c2 <= c1) of G = 2 B'S_c1 W_{c1-c2} (+ 2R), Cholesky, L^-1.
// The linear term of a solve comes from one roll of the free response and the same W (no Fq matrix is kept).
//
// Prepared controller: the body has three phases -- the set-up, the solve at a state, the outputs or the plant step -- and five modes
// that pick among them (PolyMode).  The factor kernel runs the set-up and writes one record [A | B | W | Jp] per instance
// (poly_rec_layout); the step and the controller's rollout load the record where the one-shot kernels run the set-up, and from there
// every mode runs the same statements on the same values, so a step returns the bits of the one-shot solve at the same state.  The
// step solves once: it builds J straight from the record's Jp and keeps neither Jp, the plant nor the set-up's scratch in LDS
// (poly_step_lds).
//
// No loop depends on the data for its termination: every loop has a bound the host knows, the passes of the active-set loop are counted
// against max_iter, and the exits are written so that a NaN leaves the loop.  Non-finite data: status 2, found in the plan at the end.
#include "lqmpc_launch.h"

#include <cstdio>

namespace lqmpc {

namespace {

constexpr int POLY_THREADS = 64;             // one wavefront: one instance
constexpr size_t POLY_LDS_LIMIT = 160 * 1024;

// LDS image in doubles
struct PolyLds {
    int ld;                                  // row stride of J (odd)
    int Q, P, R, Fh, bh, A, B, At, Bt, W, J, Jp, Rf, X, av, U, d, xc, xn, act, total;
};

__host__ __device__ inline PolyLds poly_lds(int nx, int nu, int N, int m)
{
    PolyLds o;
    const int n = N * nu, tri = n * (n + 1) / 2;
    o.ld = n | 1;
    int e = 0;
    o.Q = e; e += nx * nx;
    o.P = e; e += nx * nx;
    o.R = e; e += nu * nu;
    o.Fh = e; e += m * nu;                   // the rows of Fu, normalised
    o.bh = e; e += m;                        // 1 / |Fu_j|: the right-hand side of the normalised row, and what scales its multiplier back
    o.A = e; e += nx * nx;
    o.B = e; e += nx * nu;
    o.At = e; e += nx * nx;                  // the plant (rollout)
    o.Bt = e; e += nx * nu;
    o.W = e; e += N * nx * nu;               // W_k = A^k B, k < N
    o.J = e; e += n * o.ld;                  // set-up: G, its Cholesky factor, L^-1; then J
    o.Jp = e; e += tri;                      // L^-1 packed by rows: the pristine J = L^-T every solve can start from
    int u = tri;                             // Rf packed by columns; set-up: S, T = S A, S B; linear term: y; V_N: the stage costs
    if (u < 2 * nx * nx + nx * nu) u = 2 * nx * nx + nx * nu;
    if (u < N * nx + 1) u = N * nx + 1;
    o.Rf = e; e += u;
    o.X = e; e += (N + 1) * nx;              // the free response, then the model's states under the plan
    o.av = e; e += n;                        // the linear term 2g
    o.U = e; e += n;
    o.d = e; e += n;                         // d = J'n_p; set-up: the reciprocals of the Cholesky diagonal
    o.xc = e; e += nx;
    o.xn = e; e += nx;
    o.act = e; e += (N * m + 7) / 8;         // one byte per (stage, row): 1 = active
    o.total = e;
    return o;
}

// The image of lqmpc_poly_ctl_step_kernel: poly_lds without the plant, the packed copy of L^-1 (read from the record, once), the
// next state and the set-up's scratch.  The offsets left out are -1.
__host__ __device__ inline PolyLds poly_step_lds(int nx, int nu, int N, int m)
{
    PolyLds o;
    const int n = N * nu, tri = n * (n + 1) / 2;
    o.ld = n | 1;
    int e = 0;
    o.Q = e; e += nx * nx;
    o.P = e; e += nx * nx;
    o.R = e; e += nu * nu;
    o.Fh = e; e += m * nu;
    o.bh = e; e += m;
    o.A = e; e += nx * nx;
    o.B = e; e += nx * nu;
    o.At = o.Bt = o.Jp = o.xn = -1;
    o.W = e; e += N * nx * nu;
    o.J = e; e += n * o.ld;
    int u = tri;                             // Rf packed by columns; linear term: y; V_N: the stage costs
    if (u < N * nx + 1) u = N * nx + 1;
    o.Rf = e; e += u;
    o.X = e; e += (N + 1) * nx;
    o.av = e; e += n;
    o.U = e; e += n;
    o.d = e; e += n;
    o.xc = e; e += nx;
    o.act = e; e += (N * m + 7) / 8;
    o.total = e;
    return o;
}

__device__ __forceinline__ double wave_sum(double v)
{
    // a butterfly: every lane adds the same pairs, so every lane ends with the same bits
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// the largest value and, among equals, the smallest index: the same pair in every lane.  A NaN is never taken.
__device__ __forceinline__ void wave_argmax(double &v, int &i)
{
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(i, off);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}

// What a kernel runs of the body's three phases (set-up | solve at a state | outputs or plant step):
enum PolyMode {
    POLY_SOLVE,                              // set-up, one solve, the outputs of a solve
    POLY_ROLL,                               // set-up, T times: solve, plant step
    POLY_FACTOR,                             // set-up, then the record [A | B | W | Jp] to HBM
    POLY_STEP,                               // the record in the set-up's place, one solve, the outputs of a solve
    POLY_CTL_ROLL                            // the record in the set-up's place, T times: solve, plant step
};

template <int MODE>
__device__ __forceinline__ void poly_body(const PolyParams &p)
{
    extern __shared__ double lds_poly[];
    constexpr bool ROLL = MODE == POLY_ROLL || MODE == POLY_CTL_ROLL;
    constexpr bool SETUP = MODE == POLY_SOLVE || MODE == POLY_ROLL || MODE == POLY_FACTOR;
    const int nx = p.nx, nu = p.nu, N = p.N, m = p.m, n = N * nu, Nm = N * m;
    const int t = threadIdx.x;
    const PolyLds o = MODE == POLY_STEP ? poly_step_lds(nx, nu, N, m) : poly_lds(nx, nu, N, m);
    const int ld = o.ld;
    const long long Bsz = p.Bsz, b = blockIdx.x;
    // the record of this wavefront: the factor kernel writes record idx[b] of the controller's nrec (an entry outside is skipped
    // whole, before anything is written), the step and the controller's rollout read record b
    const PolyRec ro = poly_rec_layout(nx, nu, N);
    long long slot = b;
    if (MODE == POLY_FACTOR) {
        if (p.idx) slot = p.idx[b];
        if (slot < 0 || slot >= p.nrec) return;
    }
    double *rec = SETUP && MODE != POLY_FACTOR ? nullptr : p.rec + slot * p.rstride;
    const double *sh = p.sh;
    const double inf = __builtin_inf();

    double *Qs = lds_poly + o.Q, *Ps = lds_poly + o.P, *Rs = lds_poly + o.R, *Fh = lds_poly + o.Fh, *bh = lds_poly + o.bh;
    double *Am = lds_poly + o.A, *Bm = lds_poly + o.B, *Atm = lds_poly + o.At, *Btm = lds_poly + o.Bt, *W = lds_poly + o.W;
    double *J = lds_poly + o.J, *Jp = lds_poly + o.Jp, *Rf = lds_poly + o.Rf, *X = lds_poly + o.X, *av = lds_poly + o.av;
    double *U = lds_poly + o.U, *d = lds_poly + o.d, *xc = lds_poly + o.xc, *xn = lds_poly + o.xn;
    unsigned char *act = (unsigned char *)(lds_poly + o.act);

    // ---- the data of the instance ----
    for (int e = t; e < nx * nx; e += POLY_THREADS) {
        Qs[e] = sh[p.so.Q + e]; Ps[e] = sh[p.so.P + e];
        Am[e] = SETUP ? p.A[(long long)e * Bsz + b] : rec[ro.A + e];
        if (ROLL) Atm[e] = p.At[(long long)e * p.sE + b * p.sI];
    }
    for (int e = t; e < nu * nu; e += POLY_THREADS) Rs[e] = sh[p.so.R + e];
    for (int e = t; e < nx * nu; e += POLY_THREADS) {
        Bm[e] = SETUP ? p.B[(long long)e * Bsz + b] : rec[ro.B + e];
        if (SETUP) W[e] = Bm[e];
        if (ROLL) Btm[e] = p.Bt[(long long)e * p.sE + b * p.sI];
    }
    if (!SETUP) {
        // consecutive lanes on consecutive addresses of the record
        for (int e = t; e < N * nx * nu; e += POLY_THREADS) W[e] = rec[ro.W + e];
        if (MODE == POLY_CTL_ROLL)
            for (int e = t; e < n * (n + 1) / 2; e += POLY_THREADS) Jp[e] = rec[ro.Jp + e];
    }
    if (MODE != POLY_FACTOR && t < m) {
        double s = 0.0;
#pragma unroll 4
        for (int c = 0; c < nu; ++c) s = __builtin_fma(sh[p.so.Fu + t * nu + c], sh[p.so.Fu + t * nu + c], s);
        const double inv = 1.0 / sqrt(s);
        for (int c = 0; c < nu; ++c) Fh[t * nu + c] = sh[p.so.Fu + t * nu + c] * inv;
        bh[t] = inv;
    }
    if (MODE != POLY_FACTOR) {
        if (t < nx) xc[t] = p.x0[(long long)t * Bsz + b];
        for (int e = t; e < Nm; e += POLY_THREADS) act[e] = 0;
    }
    __syncthreads();
    double rho = 0.0;                        // the distance of the farthest facet
    if (MODE != POLY_FACTOR)
        for (int j = 0; j < m; ++j) rho = bh[j] > rho ? bh[j] : rho;
    const double tol = p.eps * rho;

    if (SETUP) {
        // ---- set-up: W_k = A W_{k-1} ----
        for (int k = 1; k < N; ++k) {
            for (int e = t; e < nx * nu; e += POLY_THREADS) {
                const int a = e / nu, c = e - a * nu;
                double s = 0.0;
#pragma unroll 4
                for (int q = 0; q < nx; ++q) s = __builtin_fma(Am[a * nx + q], W[(k - 1) * nx * nu + q * nu + c], s);
                W[k * nx * nu + e] = s;
            }
            __syncthreads();
        }
        // ---- the lower triangle of G = 2H, block row c1 from S_c1 = sum_{r >= c1} (A^{r-c1})'Q_r A^{r-c1}: S_{N-1} = P, S_c = Q + A'S_{c+1}A ----
        {
            double *S = Rf, *Tm = Rf + nx * nx, *SB = Rf + 2 * nx * nx;
            for (int e = t; e < nx * nx; e += POLY_THREADS) S[e] = Ps[e];
            __syncthreads();
            for (int c1 = N - 1; c1 >= 0; --c1) {
                for (int e = t; e < nx * nu; e += POLY_THREADS) {
                    const int a = e / nu, k = e - a * nu;
                    double s = 0.0;
#pragma unroll 4
                    for (int q = 0; q < nx; ++q) s = __builtin_fma(S[a * nx + q], Bm[q * nu + k], s);
                    SB[e] = s;
                }
                __syncthreads();
                if (t < n && t / nu <= c1) {
                    const int c2 = t / nu, k2 = t - c2 * nu;
                    const double *Wd = W + (c1 - c2) * nx * nu;
                    for (int k1 = 0; k1 < nu; ++k1) {
                        double s = 0.0;
#pragma unroll 4
                        for (int a = 0; a < nx; ++a) s = __builtin_fma(SB[a * nu + k1], Wd[a * nu + k2], s);
                        if (c1 == c2) s += Rs[k1 * nu + k2];
                        J[(c1 * nu + k1) * ld + t] = 2.0 * s;
                    }
                }
                if (c1 > 0) {
                    for (int e = t; e < nx * nx; e += POLY_THREADS) {
                        const int a = e / nx, c = e - a * nx;
                        double s = 0.0;
#pragma unroll 4
                        for (int q = 0; q < nx; ++q) s = __builtin_fma(S[a * nx + q], Am[q * nx + c], s);
                        Tm[e] = s;
                    }
                    __syncthreads();
                    for (int e = t; e < nx * nx; e += POLY_THREADS) {
                        const int a = e / nx, c = e - a * nx;
                        double s = Qs[e];
#pragma unroll 4
                        for (int q = 0; q < nx; ++q) s = __builtin_fma(Am[q * nx + a], Tm[q * nx + c], s);
                        S[e] = s;
                    }
                }
                __syncthreads();
            }
        }
        // ---- Cholesky factor G = LL' in place, column by column: lane i holds row i; the reciprocals of the diagonal go to d.  A pivot
        // that is not positive gives NaN, nothing waits on it ----
        for (int q = 0; q < n; ++q) {
            double dq = J[q * ld + q];
#pragma unroll 4
            for (int k = 0; k < q; ++k) dq = __builtin_fma(-J[q * ld + k], J[q * ld + k], dq);
            const double ri = 1.0 / sqrt(dq);
            if (t < n && t > q) {
                double s = J[t * ld + q];
#pragma unroll 4
                for (int k = 0; k < q; ++k) s = __builtin_fma(-J[t * ld + k], J[q * ld + k], s);
                J[t * ld + q] = s * ri;
            }
            if (t == q) d[q] = ri;
            __syncthreads();
        }
        // ---- L^-1 in place, row by row: lane j holds column j ----
        for (int i = 0; i < n; ++i) {
            double s = 0.0;
            if (t < i) {
#pragma unroll 4
                for (int k = t; k < i; ++k) s = __builtin_fma(J[i * ld + k], J[k * ld + t], s);
                s = 0.0 - s * d[i];
            }
            __syncthreads();
            if (t < i) J[i * ld + t] = s;
            if (t == i) J[i * ld + i] = d[i];
            __syncthreads();
        }
        if (t < n)
            for (int j = t; j < n; ++j) Jp[j * (j + 1) / 2 + t] = J[j * ld + t];
        __syncthreads();
    }
    if (MODE == POLY_FACTOR) {
        // ---- the record: consecutive lanes on consecutive addresses ----
        for (int e = t; e < nx * nx; e += POLY_THREADS) rec[ro.A + e] = Am[e];
        for (int e = t; e < nx * nu; e += POLY_THREADS) rec[ro.B + e] = Bm[e];
        for (int e = t; e < N * nx * nu; e += POLY_THREADS) rec[ro.W + e] = W[e];
        for (int e = t; e < n * (n + 1) / 2; e += POLY_THREADS) rec[ro.Jp + e] = Jp[e];
        return;
    }

    // J = L^-T from the packed copy: what a solve starts from (the step reads the record's copy, once)
    const double *Jsrc = MODE == POLY_STEP ? rec + ro.Jp : Jp;
    auto pristine = [&]() {
        if (t < n)
#pragma unroll 4
            for (int j = 0; j < n; ++j) J[t * ld + j] = j >= t ? Jsrc[j * (j + 1) / 2 + t] : 0.0;
        __syncthreads();
    };
    pristine();

    const int cap = p.max_iter > 0 ? p.max_iter : 10 * n + 20;
    int status_all = 0, iters_all = 0;
    bool dirty = false;                      // J was rotated, rows are marked active
    double JT = 0.0;
    if (ROLL) {
        for (int a = 0; a < nx; ++a)
#pragma unroll 4
            for (int c = 0; c < nx; ++c) JT = __builtin_fma(xc[a] * Qs[a * nx + c], xc[c], JT);
        for (int e = t; e < nx; e += POLY_THREADS)
            if (p.X) p.X[(long long)e * (p.T + 1) * Bsz + b] = xc[e];
    }
    const int steps = ROLL ? p.T : 1;

    for (int step = 0; step < steps; ++step) {
        if (dirty) {
            for (int e = t; e < Nm; e += POLY_THREADS) act[e] = 0;
            pristine();
            dirty = false;
        }
        // ---- the linear term 2g at the state xc: the free response, y_r = Q_r (x_{r+1} - xref_r), g_(c,k) = sum_{r >= c} (W_{r-c} e_k)'y_r - (R uref_c)_k ----
        {
            double *y = Rf;
            if (t < nx) X[t] = xc[t];
            __syncthreads();
            for (int r = 0; r < N; ++r) {
                if (t < nx) {
                    double s = 0.0;
#pragma unroll 4
                    for (int c = 0; c < nx; ++c) s = __builtin_fma(Am[t * nx + c], X[r * nx + c], s);
                    X[(r + 1) * nx + t] = s;
                }
                __syncthreads();
            }
            for (int e = t; e < N * nx; e += POLY_THREADS) {
                const int r = e / nx, a = e - r * nx;
                const double *Wm = r == N - 1 ? Ps : Qs;
                double s = 0.0;
#pragma unroll 4
                for (int c = 0; c < nx; ++c) s = __builtin_fma(Wm[a * nx + c], X[(r + 1) * nx + c] - sh[p.so.xref + c * N + r], s);
                y[e] = s;
            }
            __syncthreads();
            if (t < n) {
                const int c = t / nu, k = t - c * nu;
                double s = 0.0;
                for (int r = c; r < N; ++r)
#pragma unroll 4
                    for (int a = 0; a < nx; ++a) s = __builtin_fma(W[(r - c) * nx * nu + a * nu + k], y[r * nx + a], s);
#pragma unroll 4
                for (int l = 0; l < nu; ++l) s = __builtin_fma(-Rs[k * nu + l], sh[p.so.uref + l * N + c], s);
                av[t] = 2.0 * s;
            }
            __syncthreads();
        }
        // ---- the unconstrained minimiser U = -J J'(2g) ----
        if (t < n) {
            double s = 0.0;
#pragma unroll 4
            for (int i = 0; i < n; ++i) s = __builtin_fma(J[i * ld + t], av[i], s);
            d[t] = s;
        }
        __syncthreads();
        if (t < n) {
            double s = 0.0;
#pragma unroll 4
            for (int k = 0; k < n; ++k) s = __builtin_fma(J[t * ld + k], d[k], s);
            U[t] = 0.0 - s;
        }
        __syncthreads();

        // ---- the active-set loop ----
        int q = 0, iters = 0, status = 1;    // status 1: the cap was reached
        double uk = 0.0;                     // lane k < q: the multiplier of active row k (normalised rows)
        int idk = 0;                         // ... and its id, stage * m + row
        bool have = false;                   // a violated row is being worked on
        int pe = 0;
        double viol = 0.0, up = 0.0;

        auto select = [&]() {
            double best = -inf;
            int bi = 0;
            for (int e = t; e < Nm; e += POLY_THREADS) {
                if (act[e]) continue;
                const int i = e / m, j = e - i * m;
                double v = -bh[j];
#pragma unroll 4
                for (int c = 0; c < nu; ++c) v = __builtin_fma(Fh[j * nu + c], U[i * nu + c], v);
                if (v > best) { best = v; bi = e; }
            }
            wave_argmax(best, bi);
            viol = best;
            pe = __builtin_amdgcn_readfirstlane(bi);
        };

        for (int pass = 0; pass < cap; ++pass) {
            if (!have) {
                select();
                if (!(viol > tol)) { status = 0; break; }
                up = 0.0;
                have = true;
            }
            const int pi = pe / m, pj = pe - pi * m;
            // d = J'n_p: the normal has nu non-zeros
            double dk = 0.0;
            if (t < n) {
#pragma unroll 4
                for (int c = 0; c < nu; ++c) dk = __builtin_fma(J[(pi * nu + c) * ld + t], Fh[pj * nu + c], dk);
                d[t] = dk;
            }
            __syncthreads();
            const double dd = wave_sum(t < n ? dk * dk : 0.0);
            const double d2 = wave_sum(t < n && t >= q ? dk * dk : 0.0);
            // r = Rf^-1 d1 by back-substitution: lane k carries its right-hand side
            double rk = 0.0, s = dk;
            for (int j = q - 1; j >= 0; --j) {
                const double rj = __shfl(s, j) / Rf[j * (j + 1) / 2 + j];
                if (t < j) s = __builtin_fma(-Rf[j * (j + 1) / 2 + t], rj, s);
                if (t == j) rk = rj;
            }
            double t1 = t < q && rk > 0.0 ? uk / rk : inf;
            int l = t;
            {
                // the smallest ratio, among equals the smallest index
                double neg = -t1;
                wave_argmax(neg, l);
                t1 = -neg;
                l = __builtin_amdgcn_readfirstlane(l);
            }
            const bool full = d2 > 1e-13 * dd;            // false: row p depends on the active rows (or the data is not finite)
            const double t2 = full ? viol / d2 : inf;
            if (!full && !(t1 < inf)) break;              // no step is left (cannot happen with finite data: u = 0 is strictly feasible)
            const bool add = full && !(t1 < t2);
            const double tt = add ? t2 : t1;
            if (full && t < n) {
                double z = 0.0;
#pragma unroll 4
                for (int k = q; k < n; ++k) z = __builtin_fma(J[t * ld + k], d[k], z);
                U[t] = __builtin_fma(-tt, z, U[t]);
            }
            if (t < q) {
                uk = __builtin_fma(-tt, rk, uk);
                uk = uk > 0.0 ? uk : 0.0;                  // a multiplier is never stored negative
            }
            up += tt;
            ++iters;
            dirty = true;
            if (add) {
                // one Householder reflection takes d2 to alpha e_1: J2 <- J2 (I - beta v v'), v = d2 - alpha e_1
                const double dq = d[q], nrm = sqrt(d2);
                const double alpha = dq > 0.0 ? -nrm : nrm;
                const double v0 = dq - alpha, beta = 1.0 / (nrm * (nrm + fabs(dq)));
                __syncthreads();
                if (t < n) {
                    double w = J[t * ld + q] * v0;
#pragma unroll 4
                    for (int k = q + 1; k < n; ++k) w = __builtin_fma(J[t * ld + k], d[k], w);
                    w *= beta;
                    J[t * ld + q] = __builtin_fma(-w, v0, J[t * ld + q]);
#pragma unroll 4
                    for (int k = q + 1; k < n; ++k) J[t * ld + k] = __builtin_fma(-w, d[k], J[t * ld + k]);
                }
                if (t < q) Rf[q * (q + 1) / 2 + t] = dk;
                if (t == q) { Rf[q * (q + 1) / 2 + q] = alpha; uk = up; idk = pe; }
                if (t == 0) act[pe] = 1;
                ++q;
                have = false;
                __syncthreads();
            } else {
                // drop active row l: column l leaves Rf, Givens rotations of rows (k, k + 1) make it triangular again, J follows
                const int gone = __shfl(idk, l);
                if (t == 0) act[gone] = 0;
                for (int k = l; k < q - 1; ++k) {
                    const int ck = (k + 1) * (k + 2) / 2;          // old column k + 1
                    const double ga = Rf[ck + k], gb = Rf[ck + k + 1];
                    const double h = sqrt(__builtin_fma(ga, ga, gb * gb));
                    const double gc = h > 0.0 ? ga / h : 1.0, gs = h > 0.0 ? gb / h : 0.0;
                    __syncthreads();
                    if (t > k && t < q) {
                        const int cj = t * (t + 1) / 2;
                        const double x0 = Rf[cj + k], x1 = Rf[cj + k + 1];
                        Rf[cj + k] = __builtin_fma(gc, x0, gs * x1);
                        Rf[cj + k + 1] = __builtin_fma(gc, x1, -gs * x0);
                    }
                    if (t < n) {
                        const double j0 = J[t * ld + k], j1 = J[t * ld + k + 1];
                        J[t * ld + k] = __builtin_fma(gc, j0, gs * j1);
                        J[t * ld + k + 1] = __builtin_fma(gc, j1, -gs * j0);
                    }
                    __syncthreads();
                }
                // the columns behind l move one to the left, row by row
                for (int row = 0; row < q - 1; ++row) {
                    const bool mine = t >= l && t < q - 1 && row <= t;
                    const double v = mine ? Rf[(t + 1) * (t + 2) / 2 + row] : 0.0;
                    __syncthreads();
                    if (mine) Rf[t * (t + 1) / 2 + row] = v;
                    __syncthreads();
                }
                const double un = __shfl_down(uk, 1);
                const int in = __shfl_down(idk, 1);
                if (t >= l && t < q - 1) { uk = un; idk = in; }
                --q;
                __syncthreads();
                // the violation of row p after the partial step
                double v = -bh[pj];
#pragma unroll 4
                for (int c = 0; c < nu; ++c) v = __builtin_fma(Fh[pj * nu + c], U[pi * nu + c], v);
                viol = v;
            }
        }
        if (status == 1 && !have) {
            // the cap fell on an add: the iterate may be optimal all the same
            select();
            if (!(viol > tol)) status = 0;
        }
        {
            const bool bad = t < n && !(U[t] - U[t] == 0.0);
            if (__any(bad)) status = 2;
        }
        status_all = status > status_all ? status : status_all;
        iters_all += iters;

        if (!ROLL) {
            // ---- the outputs of one solve ----
            if (t < n) {
                const int i = t / nu, k = t - i * nu;
                if (i == 0) p.u0[(long long)k * Bsz + b] = U[t];
                if (p.Uplan) p.Uplan[((long long)k * N + i) * Bsz + b] = U[t];
            }
            if (p.lam) {
                for (int e = t; e < Nm; e += POLY_THREADS)
                    if (!act[e]) { const int i = e / m, j = e - i * m; p.lam[((long long)j * N + i) * Bsz + b] = 0.0; }
                if (t < q) { const int i = idk / m, j = idk - i * m; p.lam[((long long)j * N + i) * Bsz + b] = uk * bh[j]; }
            }
            // the model's states under the plan, and V_N from that roll
            if (t < nx) X[t] = xc[t];
            __syncthreads();
            for (int i = 0; i < N; ++i) {
                if (t < nx) {
                    double s = 0.0;
#pragma unroll 4
                    for (int c = 0; c < nx; ++c) s = __builtin_fma(Am[t * nx + c], X[i * nx + c], s);
#pragma unroll 4
                    for (int k = 0; k < nu; ++k) s = __builtin_fma(Bm[t * nu + k], U[i * nu + k], s);
                    X[(i + 1) * nx + t] = s;
                }
                __syncthreads();
            }
            if (p.Xplan)
                for (int e = t; e < (N + 1) * nx; e += POLY_THREADS) {
                    const int i = e / nx, a = e - i * nx;
                    p.Xplan[((long long)a * (N + 1) + i) * Bsz + b] = X[e];
                }
            double *cost = Rf;
            for (int i = t; i <= N; i += POLY_THREADS) {
                const double *Wm = i == N ? Ps : Qs;
                double s = 0.0;
                for (int a = 0; a < nx; ++a) {
                    const double ea = X[i * nx + a] - (i > 0 ? sh[p.so.xref + a * N + i - 1] : 0.0);
                    double r = 0.0;
                    for (int c = 0; c < nx; ++c)
                        r = __builtin_fma(Wm[a * nx + c], X[i * nx + c] - (i > 0 ? sh[p.so.xref + c * N + i - 1] : 0.0), r);
                    s = __builtin_fma(ea, r, s);
                }
                if (i < N)
                    for (int k = 0; k < nu; ++k) {
                        const double ek = U[i * nu + k] - sh[p.so.uref + k * N + i];
                        double r = 0.0;
#pragma unroll 4
                        for (int c = 0; c < nu; ++c) r = __builtin_fma(Rs[k * nu + c], U[i * nu + c] - sh[p.so.uref + c * N + i], r);
                        s = __builtin_fma(ek, r, s);
                    }
                cost[i] = s;
            }
            __syncthreads();
            if (t == 0) {
                double s = 0.0;
                for (int i = 0; i <= N; ++i) s += cost[i];
                p.VN[b] = s;
            }
        } else {
            // ---- the plant step, the cost in the reference's order, the optional rows of X and U ----
            if (t < nx) {
                double s = 0.0;
#pragma unroll 4
                for (int c = 0; c < nx; ++c) s = __builtin_fma(Atm[t * nx + c], xc[c], s);
#pragma unroll 4
                for (int k = 0; k < nu; ++k) s = __builtin_fma(Btm[t * nu + k], U[k], s);
                xn[t] = s;
            }
            __syncthreads();
            double sx = 0.0, su = 0.0;
            for (int a = 0; a < nx; ++a)
#pragma unroll 4
                for (int c = 0; c < nx; ++c) sx = __builtin_fma(xn[a] * Qs[a * nx + c], xn[c], sx);
            for (int k = 0; k < nu; ++k)
#pragma unroll 4
                for (int c = 0; c < nu; ++c) su = __builtin_fma(U[k] * Rs[k * nu + c], U[c], su);
            JT += sx + su;
            if (t < nx && p.X) p.X[((long long)t * (p.T + 1) + step + 1) * Bsz + b] = xn[t];
            if (t < nu && p.U) p.U[((long long)t * p.T + step) * Bsz + b] = U[t];
            __syncthreads();
            if (t < nx) xc[t] = xn[t];
            __syncthreads();
        }
    }
    if (t == 0) {
        if (ROLL) p.JT[b] = JT;
        if (p.status) p.status[b] = status_all;
        if (p.iters) p.iters[b] = iters_all;
    }
}

}  // namespace

__global__ void __launch_bounds__(POLY_THREADS) lqmpc_poly_solve_kernel(const PolyParams p) { poly_body<POLY_SOLVE>(p); }
__global__ void __launch_bounds__(POLY_THREADS) lqmpc_poly_rollout_kernel(const PolyParams p) { poly_body<POLY_ROLL>(p); }
__global__ void __launch_bounds__(POLY_THREADS) lqmpc_poly_ctl_factor_kernel(const PolyParams p) { poly_body<POLY_FACTOR>(p); }
__global__ void __launch_bounds__(POLY_THREADS) lqmpc_poly_ctl_step_kernel(const PolyParams p) { poly_body<POLY_STEP>(p); }
__global__ void __launch_bounds__(POLY_THREADS) lqmpc_poly_ctl_rollout_kernel(const PolyParams p) { poly_body<POLY_CTL_ROLL>(p); }

size_t poly_lds_bytes(int nx, int nu, int N, int m) { return sizeof(double) * (size_t)poly_lds(nx, nu, N, m).total; }
size_t poly_step_lds_bytes(int nx, int nu, int N, int m) { return sizeof(double) * (size_t)poly_step_lds(nx, nu, N, m).total; }

bool poly_fits(int nx, int nu, int N, int m) { return poly_lds_bytes(nx, nu, N, m) <= POLY_LDS_LIMIT; }

// an image over 64 KiB needs the kernel function's leave
static bool poly_lds_attr(const void *fn, size_t bytes)
{
    if (bytes <= 64 * 1024) return true;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) {
        fprintf(stderr, "lqmpc: hipFuncSetAttribute(%zu bytes of LDS): %s\n", bytes, hipGetErrorString(e));
        return false;
    }
    return true;
}

bool launch_poly(const PolyParams &p, hipStream_t stream, const char **name)
{
    if (p.Bsz < 1 || p.N * p.nu > POLY_THREADS || !poly_fits(p.nx, p.nu, p.N, p.m)) return false;
    const bool roll = p.T > 0;
    const void *fn = roll ? (const void *)lqmpc_poly_rollout_kernel : (const void *)lqmpc_poly_solve_kernel;
    const size_t bytes = poly_lds_bytes(p.nx, p.nu, p.N, p.m);
    if (!poly_lds_attr(fn, bytes)) return false;
    if (roll) hipLaunchKernelGGL(lqmpc_poly_rollout_kernel, dim3((unsigned)p.Bsz), dim3(POLY_THREADS), bytes, stream, p);
    else hipLaunchKernelGGL(lqmpc_poly_solve_kernel, dim3((unsigned)p.Bsz), dim3(POLY_THREADS), bytes, stream, p);
    *name = roll ? "lqmpc_poly_rollout_kernel" : "lqmpc_poly_solve_kernel";
    return true;
}

bool launch_poly_ctl(const PolyParams &p, int what, hipStream_t stream, const char **name)
{
    if (p.Bsz < 1 || p.N * p.nu > POLY_THREADS || !poly_fits(p.nx, p.nu, p.N, p.m) || !p.rec || p.rstride < poly_rec_layout(p.nx, p.nu, p.N).stride)
        return false;
    const dim3 grid((unsigned)p.Bsz), block(POLY_THREADS);
    const size_t full = poly_lds_bytes(p.nx, p.nu, p.N, p.m), step = poly_step_lds_bytes(p.nx, p.nu, p.N, p.m);
    if (what == POLY_CTL_FACTOR) {
        if (p.nrec < 1 || !poly_lds_attr((const void *)lqmpc_poly_ctl_factor_kernel, full)) return false;
        hipLaunchKernelGGL(lqmpc_poly_ctl_factor_kernel, grid, block, full, stream, p);
        *name = "lqmpc_poly_ctl_factor_kernel";
    } else if (what == POLY_CTL_STEP) {
        if (p.T != 0 || !poly_lds_attr((const void *)lqmpc_poly_ctl_step_kernel, step)) return false;
        hipLaunchKernelGGL(lqmpc_poly_ctl_step_kernel, grid, block, step, stream, p);
        *name = "lqmpc_poly_ctl_step_kernel";
    } else if (what == POLY_CTL_ROLLOUT) {
        if (p.T < 1 || !poly_lds_attr((const void *)lqmpc_poly_ctl_rollout_kernel, full)) return false;
        hipLaunchKernelGGL(lqmpc_poly_ctl_rollout_kernel, grid, block, full, stream, p);
        *name = "lqmpc_poly_ctl_rollout_kernel";
    } else return false;
    return true;
}

}  // namespace lqmpc
