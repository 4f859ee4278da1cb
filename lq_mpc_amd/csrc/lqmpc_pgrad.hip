// lqmpc_pgrad.hip -- the gradient of a loss on the WHOLE plan -- every u_i, every x_i and V_N -- with respect to the model matrices A
// and B and the given state x_0 of every instance (lqmpc_plan_grad_batch, lqmpc_controller_plan_grad).  A post-pass in a kernel of its
// own, the sibling of lqmpc_grad.hip: it reads what a plan call has written and touches no solver kernel.  gfx950 (MI355X) only.
//
// Per instance, with w_i = d loss / d u_i, s_i = d loss / d x_i, gam = d loss / d V_N and f_j the free mask of stage j (the sweep of
// lqmpc_sens.hip and lqmpc_grad.hip is restated here, with an affine part carried beside S):
//     S = P, pi = s_N;  for j = N-1 .. 0:  Re = R_j + B_j'S B_j,  K_j = Re^-1 B_j'S A,  kap_j = 1/2 f_j Re^-1 f_j (w_j + B'pi),
//                                          pi <- s_j + (A - B_j K_j)'pi - K_j'f_j w_j,  S <- Q + A'S (A - B_j K_j)    (K_j, kap_j of all stages kept)
//     xt_0 = 0;  j = 0 .. N-1:  ut_j = -K_j xt_j + kap_j,  xt_{j+1} = A xt_j + B ut_j                               (the adjoint LQ problem)
//     l_N = 2 P (x_N - xref_{N-1}),  l_i = 2 Q (x_i - xref_{i-1}) + A'l_{i+1};   lt_N = 2 P xt_N - s_N,  lt_i = 2 Q xt_i - s_i + A'lt_{i+1}
//     gA  = sum_i (gam l_{i+1} - lt_{i+1}) x_i' - l_{i+1} xt_i'
//     gB  = sum_i (gam l_{i+1} - lt_{i+1}) u_i' - l_{i+1} ut_i'
//     gx0 = s_0 + gam (2 Q x_0 + A'l_1) - A'lt_1
//
// Mapping: that of lqmpc_grad_kernel -- one instance per 16-lane row, four per wavefront, one wavefront per workgroup, so every barrier
// below is a wave-local wait.  Lane a of a row owns row a of S and T = S A, column a of K_j, component a of pi, xt, l and lt, and row a
// of gA and gB, which it carries in registers (the loops over their columns are unrolled to the build limits under uniform guards).
// The right-hand side of kap_j rides the solve for K_j as one more column of G (column nx: lane nx, or lane 0 in a second turn where
// nx = 16), so the factor of Re_j is used once per stage by the same instructions.  The matrices of an instance, K_j and kap_j of every
// stage, xt and ut sit in dynamic LDS; Q, R, P once per workgroup.  w_j and s_j are read from HBM into registers, one stage ahead of the stage that uses them, never into an LDS copy.  No HBM
// workspace.  The face rule is that of lqmpc_sens.hip: bit for bit lb, ub, c - h or c + h.  Nothing branches on a computed value: NaN
// flows through and is what gets stored; an instance with status 2 gets NaN in every output; rows of K_j, kap_j and the right-hand
// sides of fixed inputs are selected to 0.0, so what gUplan holds at an input on a bound reaches no output, and an instance whose
// cotangents are all 0.0 comes out as exact zeros.  A NULL cotangent is read as 0.0 and goes through the same instructions.
#include "lqmpc_launch.h"

#include <cstdio>

namespace lqmpc {

namespace {

constexpr int PG_ROW = 16;                   // lanes per instance
constexpr int PG_IPB = 4;                    // instances per workgroup (one wavefront)
constexpr int PG_THREADS = PG_ROW * PG_IPB;
constexpr int PG_MAX_NX = 16, PG_MAX_NU = 8; // the build limits of include/lqmpc.h: the register rows of gA and gB
constexpr size_t PG_LDS_LIMIT = 160 * 1024;

// LDS image in doubles: [Q | R | P] once, then per instance [A | S | T | C | B | W | G | Re | Di | F | Wv | Y | Pi | V | Kst | Kap | Xt | Ut]
struct PGradLds {
    int ld;                                  // row stride of the nx-wide matrices (odd)
    int lg;                                  // row stride of G: nx columns and the right-hand side of kap_j
    int Q, R, P, shared;
    int A, S, T, C, B, W, G, Re, Di, F, Wv, Y, Pi, V, K, Kap, Xt, Ut, inst;
};

__host__ __device__ inline PGradLds pgrad_lds(int nx, int nu, int N)
{
    PGradLds o;
    o.ld = nx | 1;
    o.lg = nx + 1;
    int e = 0;
    o.Q = e; e += nx * nx;
    o.R = e; e += nu * nu;
    o.P = e; e += nx * nx;
    o.shared = e;
    e = 0;
    o.A = e; e += nx * o.ld;                 // A, row-major
    o.S = e; e += nx * o.ld;                 // the Riccati matrix
    o.T = e; e += nx * o.ld;                 // S A
    o.C = e; e += nx * o.ld;                 // Acl_j
    o.B = e; e += nx * nu;
    o.W = e; e += nx * nu;                   // S B
    o.G = e; e += nu * o.lg;                 // [B_j'S A | f_j (w_j + B'pi)], then [K_j | Re^-1 of that] in place
    o.Re = e; e += nu * nu;                  // Re, then its Cholesky factor below the diagonal
    o.Di = e; e += nu;                       // reciprocals of the factor's diagonal
    o.F = e; e += nu;                        // free mask of the stage, 1.0 / 0.0
    o.Wv = e; e += nu;                       // f_j w_j of the stage
    o.Y = e; e += nu;                        // backward pass: u_i
    o.Pi = e; e += 2 * nx;                   // pi of two stages
    o.V = e; e += 6 * nx;                    // backward pass: the state error, x_i, and l, lt of two stages
    o.K = e; e += N * nu * nx;               // K_j of every stage
    o.Kap = e; e += N * nu;                  // kap_j of every stage
    o.Xt = e; e += (N + 1) * nx;             // xt_0 .. xt_N
    o.Ut = e; e += N * nu;                   // ut_0 .. ut_{N-1}
    o.inst = e;
    return o;
}

}  // namespace

__global__ void __launch_bounds__(PG_THREADS) lqmpc_plan_grad_kernel(const PGradParams p)
{
    extern __shared__ double lds_pgrad[];
    const int nx = p.nx, nu = p.nu, N = p.N;
    const int t = threadIdx.x, a = t & (PG_ROW - 1), row = t / PG_ROW;
    const PGradLds o = pgrad_lds(nx, nu, N);
    const int ld = o.ld, lg = o.lg;
    const long long Bsz = p.Bsz;
    // the tail of the batch: a row past the end works on the last instance and stores nothing
    const long long b0 = (long long)blockIdx.x * PG_IPB + row;
    const bool valid = b0 < Bsz;
    const long long b = valid ? b0 : Bsz - 1;
    const bool on = a < nx, inp = a < nu;
    const double *sh = p.sh;

    double *Qs = lds_pgrad + o.Q, *Rs = lds_pgrad + o.R, *Ps = lds_pgrad + o.P;
    double *I = lds_pgrad + o.shared + row * o.inst;
    double *Am = I + o.A, *S = I + o.S, *T = I + o.T, *C = I + o.C, *Bm = I + o.B, *W = I + o.W, *G = I + o.G;
    double *Re = I + o.Re, *Di = I + o.Di, *F = I + o.F, *Wv = I + o.Wv, *Y = I + o.Y, *Pi = I + o.Pi, *V = I + o.V;
    double *Kst = I + o.K, *Kap = I + o.Kap, *Xt = I + o.Xt, *Ut = I + o.Ut;

    for (int e = t; e < nx * nx; e += PG_THREADS) { Qs[e] = sh[p.so.Q + e]; Ps[e] = sh[p.so.P + e]; }
    for (int e = t; e < nu * nu; e += PG_THREADS) Rs[e] = sh[p.so.R + e];
    for (int e = a; e < nx * nx; e += PG_ROW) {
        const int r = e / nx, c = e - r * nx;
        Am[r * ld + c] = p.A[(long long)e * p.sE + b * p.sI];
        S[r * ld + c] = sh[p.so.P + e];
    }
    for (int e = a; e < nx * nu; e += PG_ROW) Bm[e] = p.B[(long long)e * p.sE + b * p.sI];
    const bool bad = p.status ? p.status[b] == 2 : false;
    const double nan = __builtin_nan("");
    const double gam = p.gVN ? p.gVN[b] : 0.0;
    // the four forms a bound can come out in (include/lqmpc.h, the plan's contract)
    double lbk = 0.0, ubk = 0.0, lo = 0.0, hi = 0.0;
    if (inp) {
        lbk = sh[p.so.lb + a]; ubk = sh[p.so.ub + a];
        const double ctr = 0.5 * (ubk + lbk), h = 0.5 * (ubk - lbk);
        lo = ctr - h; hi = ctr + h;
    }
    double *pn = Pi, *pc = Pi + nx;           // pi of stage j + 1 and of stage j
    if (on) pn[a] = p.gX ? p.gX[((long long)a * (N + 1) + N) * Bsz + b] : 0.0;
    // u_j, w_j and s_j of a stage are fetched one stage ahead, so that the sweep does not wait for HBM at every stage
    double un = 0.0, wn = 0.0, sn = 0.0;
    if (inp) {
        un = p.Uplan[((long long)a * N + N - 1) * Bsz + b];
        if (p.gU) wn = p.gU[((long long)a * N + N - 1) * Bsz + b];
    }
    if (on && p.gX) sn = p.gX[((long long)a * (N + 1) + N - 1) * Bsz + b];
    __syncthreads();

    // ---- the masked Riccati sweep with its affine part, backwards over the stages ----
    for (int j = N - 1; j >= 0; --j) {
        const double u = un, wj = wn, sj = sn;
        if (j > 0) {
            if (inp) {
                un = p.Uplan[((long long)a * N + j - 1) * Bsz + b];
                if (p.gU) wn = p.gU[((long long)a * N + j - 1) * Bsz + b];
            }
            if (on && p.gX) sn = p.gX[((long long)a * (N + 1) + j - 1) * Bsz + b];
        }
        if (inp) {
            const bool fixed = u == lbk || u == ubk || u == lo || u == hi;
            F[a] = fixed ? 0.0 : 1.0;
            Wv[a] = fixed ? 0.0 : wj;
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
                G[k * lg + a] = F[k] * s;
            }
        }
        if (inp) {
            // column nx of G: the right-hand side of kap_j, f_j (w_j + B'pi_{j+1})
            double s = Wv[a];
            for (int r = 0; r < nx; ++r) s = __builtin_fma(Bm[r * nu + a], pn[r], s);
            G[a * lg + nx] = F[a] != 0.0 ? s : 0.0;
        }
        for (int e = a; e < nu * nu; e += PG_ROW) {
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
        // column c of Re^-1 G, in place: c < nx is column c of K_j, c = nx gives kap_j
        for (int c = a; c <= nx; c += PG_ROW) {
            for (int k = 0; k < nu; ++k) {
                double s = G[k * lg + c];
                for (int m = 0; m < k; ++m) s = __builtin_fma(-Re[k * nu + m], G[m * lg + c], s);
                G[k * lg + c] = s * Di[k];
            }
            for (int k = nu - 1; k >= 0; --k) {
                double s = G[k * lg + c];
                for (int m = k + 1; m < nu; ++m) s = __builtin_fma(-Re[m * nu + k], G[m * lg + c], s);
                const double v = F[k] != 0.0 ? s * Di[k] : 0.0;
                G[k * lg + c] = v;
                if (c < nx) Kst[(j * nu + k) * nx + c] = v;
                else Kap[j * nu + k] = 0.5 * v;
            }
        }
        if (on) {
            // column a of Acl_j = A - B K_j
            for (int r = 0; r < nx; ++r) {
                double s = Am[r * ld + a];
                for (int k = 0; k < nu; ++k) s = __builtin_fma(-Bm[r * nu + k], G[k * lg + a], s);
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
            // component a of pi_j = s_j + Acl_j'pi_{j+1} - K_j'f_j w_j
            double s = sj;
            for (int r = 0; r < nx; ++r) s = __builtin_fma(C[r * ld + a], pn[r], s);
            for (int k = 0; k < nu; ++k) s = __builtin_fma(-G[k * lg + a], Wv[k], s);
            pc[a] = s;
        }
        __syncthreads();
        double *sw = pn; pn = pc; pc = sw;
    }

    // ---- the adjoint problem rolled forwards: lane k < nu forms ut_j[k], lane a < nx forms xt_{j+1}[a] ----
    if (on) Xt[a] = 0.0;
    __syncthreads();
    for (int j = 0; j < N; ++j) {
        if (inp) {
            double s = 0.0;
            for (int c = 0; c < nx; ++c) s = __builtin_fma(Kst[(j * nu + a) * nx + c], Xt[j * nx + c], s);
            Ut[j * nu + a] = Kap[j * nu + a] - s;
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

    // ---- the two costate recursions backwards together, and the sums: at step i the costates of stage i meet x, u, xt, ut of stage i - 1 ----
    double ga[PG_MAX_NX], gb[PG_MAX_NU];
#pragma unroll
    for (int c = 0; c < PG_MAX_NX; ++c) ga[c] = 0.0;
#pragma unroll
    for (int k = 0; k < PG_MAX_NU; ++k) gb[k] = 0.0;
    double *d = V, *xs = V + nx, *l0 = V + 2 * nx, *l1 = V + 3 * nx, *m0 = V + 4 * nx, *m1 = V + 5 * nx, *us = Y;
    if (on) { l0[a] = 0.0; m0[a] = 0.0; }
    for (int i = N; i >= 1; --i) {
        double si = 0.0;
        if (on) {
            d[a] = p.Xplan[((long long)a * (N + 1) + i) * Bsz + b] - sh[p.so.xref + a * N + i - 1];
            xs[a] = p.Xplan[((long long)a * (N + 1) + i - 1) * Bsz + b];
            if (p.gX) si = p.gX[((long long)a * (N + 1) + i) * Bsz + b];
        }
        if (inp) us[a] = p.Uplan[((long long)a * N + i - 1) * Bsz + b];
        __syncthreads();
        if (on) {
            const double *Wm = i == N ? Ps : Qs;
            const double *xti = Xt + i * nx, *xtp = Xt + (i - 1) * nx, *utp = Ut + (i - 1) * nu;
            double s = 0.0, s2 = 0.0, r = 0.0, r2 = 0.0;
            for (int c = 0; c < nx; ++c) { s = __builtin_fma(Wm[a * nx + c], d[c], s); r = __builtin_fma(Wm[a * nx + c], xti[c], r); }
            for (int m = 0; m < nx; ++m) { s2 = __builtin_fma(Am[m * ld + a], l0[m], s2); r2 = __builtin_fma(Am[m * ld + a], m0[m], r2); }
            const double lam = 2.0 * s + s2, lamt = (2.0 * r + r2) - si;
            l1[a] = lam; m1[a] = lamt;
            const double pq = gam * lam - lamt;
#pragma unroll
            for (int c = 0; c < PG_MAX_NX; ++c)
                if (c < nx) ga[c] = __builtin_fma(pq, xs[c], __builtin_fma(-lam, xtp[c], ga[c]));
#pragma unroll
            for (int k = 0; k < PG_MAX_NU; ++k)
                if (k < nu) gb[k] = __builtin_fma(pq, us[k], __builtin_fma(-lam, utp[k], gb[k]));
        }
        __syncthreads();
        double *sw = l0; l0 = l1; l1 = sw;
        sw = m0; m0 = m1; m1 = sw;
    }

    // ---- stores: xs holds x_0, l0 and m0 the costates of stage 1 ----
    if (on && valid) {
        double s = 0.0, s2 = 0.0, r2 = 0.0;
        for (int c = 0; c < nx; ++c) s = __builtin_fma(Qs[a * nx + c], xs[c], s);
        for (int m = 0; m < nx; ++m) { s2 = __builtin_fma(Am[m * ld + a], l0[m], s2); r2 = __builtin_fma(Am[m * ld + a], m0[m], r2); }
        const double s0 = p.gX ? p.gX[(long long)a * (N + 1) * Bsz + b] : 0.0;
        if (p.gx0) p.gx0[(long long)a * Bsz + b] = bad ? nan : (s0 + gam * (2.0 * s + s2)) - r2;
        if (p.gA) {
#pragma unroll
            for (int c = 0; c < PG_MAX_NX; ++c)
                if (c < nx) p.gA[((long long)a * nx + c) * Bsz + b] = bad ? nan : ga[c];
        }
        if (p.gB) {
#pragma unroll
            for (int k = 0; k < PG_MAX_NU; ++k)
                if (k < nu) p.gB[((long long)a * nu + k) * Bsz + b] = bad ? nan : gb[k];
        }
    }
}

size_t pgrad_lds_bytes(int nx, int nu, int N)
{
    const PGradLds o = pgrad_lds(nx, nu, N);
    return sizeof(double) * ((size_t)o.shared + (size_t)PG_IPB * o.inst);
}

bool pgrad_fits(int nx, int nu, int N) { return pgrad_lds_bytes(nx, nu, N) <= PG_LDS_LIMIT; }

bool launch_pgrad(const PGradParams &p, hipStream_t stream)
{
    if (p.Bsz < 1 || p.nx > PG_MAX_NX || p.nu > PG_MAX_NU || !pgrad_fits(p.nx, p.nu, p.N)) return false;
    const size_t bytes = pgrad_lds_bytes(p.nx, p.nu, p.N);
    if (bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void *)lqmpc_plan_grad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) {
            fprintf(stderr, "lqmpc: hipFuncSetAttribute(%zu bytes of LDS): %s\n", bytes, hipGetErrorString(e));
            return false;
        }
    }
    const long long blocks = (p.Bsz + PG_IPB - 1) / PG_IPB;
    hipLaunchKernelGGL(lqmpc_plan_grad_kernel, dim3((unsigned)blocks), dim3(PG_THREADS), bytes, stream, p);
    return true;
}

}  // namespace lqmpc
