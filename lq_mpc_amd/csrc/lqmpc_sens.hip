// lqmpc_sens.hip -- the local feedback law and the value gradient of a solved plan (lqmpc_solve_sens_batch, lqmpc_controller_step_sens).
// A post-pass in a kernel of its own: it reads what the plan call has written and touches no solver kernel.  gfx950 (MI355X) only.
//
// Per instance, with f_j the free mask of stage j (an input of the plan that sits on a bound is fixed, the others are free):
//     B_j = B diag(f_j),  R_j = diag(f_j) R diag(f_j) + diag(1 - f_j)
//     S = P;  for j = N-1 .. 0:  Re = R_j + B_j'S B_j,  K_j = Re^-1 B_j'S A,  Acl_j = A - B_j K_j,  S <- Q + A'S Acl_j
//     Pi_0 = I;  for j = 0 .. N-1:  du_j/dx0 = -K_j Pi_j,  Pi_{j+1} = Acl_j Pi_j                      (only when Kplan is asked for)
//     l_N = 2 P (x_N - xref_{N-1}),  l_i = 2 Q (x_i - xref_{i-1}) + A'l_{i+1},  dV_N/dx0 = 2 Q x0 + A'l_1   (envelope theorem)
// Rows of K_j that belong to fixed inputs are exact zeros (the dummy-input device of lqmpc_r16_setup.h, per stage).
//
// Mapping: one instance per 16-lane row, four per wavefront, one wavefront per workgroup, so every barrier below is a wave-local wait.
// Lane a of a row owns row a of S and T = S A, and column a of K_j, Acl_j and Pi_j; the matrices of an instance sit in LDS (row
// stride nx | 1), Q, R, P once per workgroup; with Kplan the gains K_j of all stages are kept in LDS (N nu nx doubles) between the
// backward sweep and the forward products.  Loops have run-time bounds; no HBM workspace.  An input is on a bound when its plan entry
// equals, bit for bit, lb, ub, c - h or c + h (c = (ub + lb) / 2, h = (ub - lb) / 2 as every solver kernel forms them): no tolerance.
// Non-finite data: nothing branches on a computed value -- NaN flows through the factorisation and is what gets stored; an instance
// with status 2 gets NaN in every output.
#include "lqmpc_launch.h"

#include <cstdio>

namespace lqmpc {

namespace {

constexpr int SENS_ROW = 16;                 // lanes per instance
constexpr int SENS_IPB = 4;                  // instances per workgroup (one wavefront)
constexpr int SENS_THREADS = SENS_ROW * SENS_IPB;

// LDS image in doubles: [Q | R | P] once, then per instance [A | S | T | C | B | W | G | Re | Di | F | V | Kst]
struct SensLds {
    int ld;                                  // row stride of the nx-wide matrices (odd)
    int Q, R, P, shared;
    int A, S, T, C, B, W, G, Re, Di, F, V, K, inst;
};

__host__ __device__ inline SensLds sens_lds(int nx, int nu, int N, bool plan)
{
    SensLds o;
    o.ld = nx | 1;
    int e = 0;
    o.Q = e; e += nx * nx;
    o.R = e; e += nu * nu;
    o.P = e; e += nx * nx;
    o.shared = e;
    e = 0;
    o.A = e; e += nx * o.ld;                 // A, row-major
    o.S = e; e += nx * o.ld;                 // the Riccati matrix; forward pass: Pi
    o.T = e; e += nx * o.ld;                 // S A; forward pass: the next Pi
    o.C = e; e += nx * o.ld;                 // Acl_j
    o.B = e; e += nx * nu;
    o.W = e; e += nx * nu;                   // S B
    o.G = e; e += nu * o.ld;                 // B_j'S A, then K_j in place; forward pass: -K_j Pi_j
    o.Re = e; e += nu * nu;                  // Re, then its Cholesky factor below the diagonal
    o.Di = e; e += nu;                       // reciprocals of the factor's diagonal
    o.F = e; e += nu;                        // free mask of the stage, 1.0 / 0.0
    o.V = e; e += 3 * nx;                    // costate recursion: the state error and two costates
    o.K = e; e += plan ? N * nu * nx : 0;    // K_j of every stage
    o.inst = e;
    return o;
}

}  // namespace

__global__ void __launch_bounds__(SENS_THREADS) lqmpc_sens_kernel(const SensParams p)
{
    extern __shared__ double lds_sens[];
    const int nx = p.nx, nu = p.nu, N = p.N;
    const int t = threadIdx.x, a = t & (SENS_ROW - 1), row = t / SENS_ROW;
    const bool plan = p.Kplan != nullptr;
    const SensLds o = sens_lds(nx, nu, N, plan);
    const int ld = o.ld;
    const long long Bsz = p.Bsz;
    // the tail of the batch: a row past the end works on the last instance and stores nothing
    const long long b0 = (long long)blockIdx.x * SENS_IPB + row;
    const bool valid = b0 < Bsz;
    const long long b = valid ? b0 : Bsz - 1;
    const bool on = a < nx, inp = a < nu;
    const double *sh = p.sh;

    double *Qs = lds_sens + o.Q, *Rs = lds_sens + o.R, *Ps = lds_sens + o.P;
    double *I = lds_sens + o.shared + row * o.inst;
    double *Am = I + o.A, *S = I + o.S, *T = I + o.T, *C = I + o.C, *Bm = I + o.B, *W = I + o.W, *G = I + o.G;
    double *Re = I + o.Re, *Di = I + o.Di, *F = I + o.F, *V = I + o.V, *Kst = I + o.K;

    for (int e = t; e < nx * nx; e += SENS_THREADS) { Qs[e] = sh[p.so.Q + e]; Ps[e] = sh[p.so.P + e]; }
    for (int e = t; e < nu * nu; e += SENS_THREADS) Rs[e] = sh[p.so.R + e];
    for (int e = a; e < nx * nx; e += SENS_ROW) {
        const int r = e / nx, c = e - r * nx;
        Am[r * ld + c] = p.A[(long long)e * p.sE + b * p.sI];
        S[r * ld + c] = sh[p.so.P + e];
    }
    for (int e = a; e < nx * nu; e += SENS_ROW) Bm[e] = p.B[(long long)e * p.sE + b * p.sI];
    const bool bad = p.status[b] == 2;
    const double nan = __builtin_nan("");
    // the four forms a bound can come out in (include/lqmpc.h, the plan's contract)
    double lbk = 0.0, ubk = 0.0, lo = 0.0, hi = 0.0;
    if (inp) {
        lbk = sh[p.so.lb + a]; ubk = sh[p.so.ub + a];
        const double ctr = 0.5 * (ubk + lbk), h = 0.5 * (ubk - lbk);
        lo = ctr - h; hi = ctr + h;
    }
    __syncthreads();

    // ---- dV_N/dx0: the costate recursion over the predicted states ----
    {
        double *d = V, *l0 = V + nx, *l1 = V + 2 * nx;
        if (on) l0[a] = 0.0;
        for (int i = N; i >= 1; --i) {
            if (on) d[a] = p.Xplan[((long long)a * (N + 1) + i) * Bsz + b] - sh[p.so.xref + a * N + i - 1];
            __syncthreads();
            if (on) {
                const double *Wm = i == N ? Ps : Qs;
                double s = 0.0, s2 = 0.0;
                for (int c = 0; c < nx; ++c) s = __builtin_fma(Wm[a * nx + c], d[c], s);
                for (int m = 0; m < nx; ++m) s2 = __builtin_fma(Am[m * ld + a], l0[m], s2);
                l1[a] = 2.0 * s + s2;
            }
            __syncthreads();
            double *sw = l0; l0 = l1; l1 = sw;
        }
        if (on) d[a] = p.Xplan[(long long)a * (N + 1) * Bsz + b];
        __syncthreads();
        if (on) {
            double s = 0.0, s2 = 0.0;
            for (int c = 0; c < nx; ++c) s = __builtin_fma(Qs[a * nx + c], d[c], s);
            for (int m = 0; m < nx; ++m) s2 = __builtin_fma(Am[m * ld + a], l0[m], s2);
            if (valid) p.dVdx[(long long)a * Bsz + b] = bad ? nan : 2.0 * s + s2;
        }
    }

    // ---- the masked Riccati sweep, backwards over the stages ----
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
        for (int e = a; e < nu * nu; e += SENS_ROW) {
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
                if (plan) Kst[(j * nu + k) * nx + a] = v;
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

    if (!plan) {
        // K_0 = -K_0 Pi_0 with Pi_0 = I
        if (on && valid)
            for (int k = 0; k < nu; ++k) p.K0[((long long)k * nx + a) * Bsz + b] = bad ? nan : 0.0 - G[k * ld + a];
        return;
    }

    // ---- du_j/dx0 = -K_j Pi_j, forwards: lane a carries column a of Pi, nothing crosses lanes ----
    if (on) {
        double *Pi = S, *Pn = T;
        for (int m = 0; m < nx; ++m) Pi[m * ld + a] = m == a ? 1.0 : 0.0;
        for (int j = 0; j < N; ++j) {
            for (int k = 0; k < nu; ++k) {
                double s = 0.0;
                for (int m = 0; m < nx; ++m) s = __builtin_fma(Kst[(j * nu + k) * nx + m], Pi[m * ld + a], s);
                const double v = bad ? nan : 0.0 - s;
                G[k * ld + a] = 0.0 - s;
                if (valid) {
                    p.Kplan[(((long long)k * N + j) * nx + a) * Bsz + b] = v;
                    if (j == 0) p.K0[((long long)k * nx + a) * Bsz + b] = v;
                }
            }
            if (j + 1 < N) {
                for (int r = 0; r < nx; ++r) {
                    double s = 0.0;
                    for (int m = 0; m < nx; ++m) s = __builtin_fma(Am[r * ld + m], Pi[m * ld + a], s);
                    for (int k = 0; k < nu; ++k) s = __builtin_fma(Bm[r * nu + k], G[k * ld + a], s);
                    Pn[r * ld + a] = s;
                }
                double *sw = Pi; Pi = Pn; Pn = sw;
            }
        }
    }
}

bool launch_sens(const SensParams &p, hipStream_t stream)
{
    if (p.Bsz < 1) return false;
    const SensLds o = sens_lds(p.nx, p.nu, p.N, p.Kplan != nullptr);
    const size_t bytes = sizeof(double) * ((size_t)o.shared + (size_t)SENS_IPB * o.inst);
    if (bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void *)lqmpc_sens_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) {
            fprintf(stderr, "lqmpc: hipFuncSetAttribute(%zu bytes of LDS): %s\n", bytes, hipGetErrorString(e));
            return false;
        }
    }
    const long long blocks = (p.Bsz + SENS_IPB - 1) / SENS_IPB;
    hipLaunchKernelGGL(lqmpc_sens_kernel, dim3((unsigned)blocks), dim3(SENS_THREADS), bytes, stream, p);
    return true;
}

}  // namespace lqmpc
