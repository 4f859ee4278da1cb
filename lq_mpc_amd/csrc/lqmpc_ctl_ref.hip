// lqmpc_ctl_ref.hip -- new references for a prepared controller (lqmpc_controller_set_reference, include/lqmpc.h): the two kernels that
// rewrite v_r in the records, one per record layout.  At the end of the file: lqmpc_ctl_scatter_model_kernel, the part of
// lqmpc_controller_set_model that refreshes the controller's instance-minor copies of A and B.
//
// Of a record [A | B | G | v_r | W | P] only v_r depends on the references:
//   v_r = -W (2 gref + P centre) = -2 W gref - centre,
//   d_r = -xref_r,  lam_r = Q_r d_r + A' lam_{r+1} (Q_{N-1} = P_T),  gref_r = B' lam_r - R uref_r   (columns r <-> x_{r+1}, u_r)
// -- the constant part of the unconstrained minimiser as the factor launches compute it (lqmpc_r16_body.h, lqmpc_wg.hip), here from
// the record's own A, B and W instead of a set-up.  Everything else a step takes from the references (the model's V_N) it reads
// from the batch-shared block at run time.  nx, nu, N are run-time arguments: one kernel per layout serves the prebuilt and the
// run-time compiled shapes alike.  tools/proto/ctl_retarget.py is the same arithmetic and both indexings in numpy.
#include "lqmpc_wg_linalg.h"
#include "lqmpc_launch.h"

#include <stdio.h>

namespace lqmpc {

using namespace wg;                          // BS, LD, BLK, THREADS, blk_index: the block image of lqmpc_wg_linalg.h

constexpr int RT_IPB = 4;                    // 16-lane-row records: instances per workgroup (one wavefront)

// ---- 16-lane-row records (ctl_rec_layout, n <= 48, nx <= 8, nu <= 4) ----
// Sixteen lanes per instance; lane i owns rows i, i + 16, i + 32 of v_r, component i of lam and column i of A and of B.
// LDS: [Q_r d_r (N nx) | R uref_r (N nu)] once per workgroup, then per instance [q (n) | W (packed triangle)].
__global__ void __launch_bounds__(64) lqmpc_ctl_retarget_kernel(KParams p)
{
    extern __shared__ double lds_rt[];
    const int nx = p.nx, nu = p.nu, N = p.N, n = p.n;
    const int tid = threadIdx.x, i = tid & 15, g = tid >> 4;
    const CtlRec L = ctl_rec_layout(nx, nu, N);
    const long long braw = (long long)blockIdx.x * RT_IPB + g;
    const bool valid = braw < p.Bsz;         // the partial last wavefront: reads of the last instance, no writes
    const long long b = valid ? braw : p.Bsz - 1;
    double *rc = p.ctl_rec + b * p.ctl_stride;
    const double *sh = p.sh;
    double ctr[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int k = (i + 16 * s) % nu;
        ctr[s] = 0.5 * (sh[p.so.ub + k] + sh[p.so.lb + k]);
    }
    if (!p.has_ref) {                        // (uniform) no references: v_r = -centre, W is not read
        if (valid) {
#pragma unroll
            for (int s = 0; s < 3; ++s)
                if (i + 16 * s < n) rc[L.oV + i + 16 * s] = 0.0 - ctr[s];
        }
        return;
    }
    double *Qd = lds_rt, *Ru = Qd + N * nx;
    double *q = Ru + N * nu + g * (n + L.tri), *W = q + n;
    double Ac[8], Bc[8];                     // column i of A (lanes < nx) and of B (lanes < nu)
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        Ac[c] = (c < nx && i < nx) ? rc[L.oA + c * nx + i] : 0.0;
        Bc[c] = (c < nx && i < nu) ? rc[L.oB + c * nu + i] : 0.0;
    }
    // the triangle of my instance, element by element over its lanes (consecutive addresses), eight loads in flight per lane; used
    // after the recursion
    for (int e0 = i; e0 < L.tri; e0 += 16 * 8) {
        double w[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = (e0 + 16 * k < L.tri) ? rc[L.oW + e0 + 16 * k] : 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (e0 + 16 * k < L.tri) W[e0 + 16 * k] = w[k];
    }
    // what the recursion takes from the shared block, the same for every instance
    for (int e = tid; e < N * nx; e += 64) {
        const int r = e / nx, a = e - r * nx;
        const double *Qr = sh + ((r < N - 1) ? p.so.Q : p.so.P);
        double t = 0.0;
        for (int c = 0; c < nx; ++c) t = __builtin_fma(Qr[a * nx + c], -sh[p.so.xref + c * N + r], t);
        Qd[e] = t;
    }
    for (int e = tid; e < N * nu; e += 64) {
        const int r = e / nu, k = e - r * nu;
        double t = 0.0;
        for (int j = 0; j < nu; ++j) t = __builtin_fma(sh[p.so.R + k * nu + j], sh[p.so.uref + j * N + r], t);
        Ru[e] = t;
    }
    __syncthreads();
    double lam = 0.0;
    for (int r = N - 1; r >= 0; --r) {
        double t = (i < nx) ? Qd[r * nx + i] : 0.0;
#pragma unroll
        for (int c = 0; c < 8; ++c) t = __builtin_fma(Ac[c], __shfl(lam, c, 16), t);      // (Ac[c] = 0 beyond nx)
        lam = t;
        double gk = (i < nu) ? -Ru[r * nu + i] : 0.0;
#pragma unroll
        for (int a = 0; a < 8; ++a) gk = __builtin_fma(Bc[a], __shfl(lam, a, 16), gk);
        if (i < nu) q[r * nu + i] = 2.0 * gk;
    }
    __syncthreads();
    // the row owner's product with the packed triangle: W(row, j) at sym(row, j)
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int row = i + 16 * s;
        if (row < n) {
            const double *Wr = W + row * (row + 1) / 2;
            double t = 0.0;
            for (int j = 0; j <= row; ++j) t = __builtin_fma(Wr[j], q[j], t);
            for (int j = row + 1; j < n; ++j) t = __builtin_fma(W[j * (j + 1) / 2 + row], q[j], t);
            if (valid) rc[L.oV + row] = -t - ctr[s];
        }
    }
}

static size_t retarget_lds_bytes(int nx, int nu, int N)
{
    const int n = N * nu;
    return sizeof(double) * (size_t)(N * nx + n + RT_IPB * (n + n * (n + 1) / 2));
}

bool launch_ctl_retarget(const KParams &p, hipStream_t stream)
{
    if (!jit_r16_shape(p.nx, p.nu, p.N, nullptr) || p.nx > 8 || p.nu > 4 || p.Bsz < 1) return false;
    const dim3 grid((unsigned)((p.Bsz + RT_IPB - 1) / RT_IPB));
    hipLaunchKernelGGL(lqmpc_ctl_retarget_kernel, grid, dim3(64), retarget_lds_bytes(p.nx, p.nu, p.N), stream, p);
    return true;
}

// ---- workgroup records (wg_ctl_rec_layout, 32 < n <= 128, nx <= 16, nu <= 8) ----
// One instance per workgroup.  W is the block image (lower block triangle of 16 x 17 blocks, diagonal blocks in full), copied flat into
// LDS; thread t < np owns row t.  A record whose v_r holds NaN marks a failed set-up and keeps NaN in every row.
// LDS: [W image | q (np) | A | B | lam (2 nx) | flag].
__global__ void __launch_bounds__(256) lqmpc_wg_ctl_retarget_kernel(KParams p)
{
    extern __shared__ double lds_rt[];
    const int nx = p.nx, nu = p.nu, N = p.N, n = p.n, t = threadIdx.x;
    const int nb = (n + BS - 1) / BS, np = nb * BS;
    const WgCtlRec L = wg_ctl_rec_layout(nx, nu, N);
    double *rc = p.ctl_rec + (long long)blockIdx.x * p.ctl_stride;
    const double *sh = p.sh;
    double *K = lds_rt, *q = K + L.img, *Am = q + np, *Bm = Am + nx * nx, *lam = Bm + nx * nu, *lam2 = lam + nx;
    int *bad = (int *)(lam2 + nx);
    const bool own = t < n;
    const double old = (t < np) ? rc[L.oV + t] : 0.0;
    if (t == 0) *bad = 0;
    if (p.has_ref) {
        for (int e = t; e < L.img; e += THREADS) K[e] = rc[L.oW + e];
        for (int e = t; e < nx * nx + nx * nu; e += THREADS) Am[e] = rc[L.oA + e];
    }
    if (t < np) q[t] = 0.0;
    if (t < nx) lam[t] = 0.0;
    __syncthreads();
    if (old != old) *bad = 1;                // (every writer writes the same value)
    double acc = 0.0;
    if (p.has_ref) {
        const double *xr = sh + p.so.xref, *ur = sh + p.so.uref;
        for (int r = N - 1; r >= 0; --r) {
            const double *Qr = sh + ((r < N - 1) ? p.so.Q : p.so.P);
            if (t < nx) {
                double a = 0.0;
                for (int y = 0; y < nx; ++y) a = __builtin_fma(Qr[t * nx + y], -xr[y * N + r], a);
                for (int y = 0; y < nx; ++y) a = __builtin_fma(Am[y * nx + t], lam[y], a);
                lam2[t] = a;
            }
            __syncthreads();
            if (t < nx) lam[t] = lam2[t];
            if (t < nu) {
                double a = 0.0;
                for (int x = 0; x < nx; ++x) a = __builtin_fma(Bm[x * nu + t], lam2[x], a);
                for (int j = 0; j < nu; ++j) a = __builtin_fma(-sh[p.so.R + t * nu + j], ur[j * N + r], a);
                q[r * nu + t] = 2.0 * a;
            }
            __syncthreads();
        }
        if (own) {
            const int ib = t / BS, r = t % BS;
            for (int jb = 0; jb <= ib; ++jb) {                    // row t of the blocks left of and on the diagonal
                const double *B = K + blk_index(ib, jb) * BLK + r * LD;
#pragma unroll
                for (int c = 0; c < BS; ++c) acc = __builtin_fma(B[c], q[jb * BS + c], acc);
            }
            for (int kb = ib + 1; kb < nb; ++kb) {                // column t of the blocks below
                const double *B = K + blk_index(kb, ib) * BLK + r;
#pragma unroll
                for (int c = 0; c < BS; ++c) acc = __builtin_fma(B[c * LD], q[kb * BS + c], acc);
            }
        }
    } else {
        __syncthreads();
    }
    if (t < np) {
        const int k = t % nu;
        const double v = own ? -acc - 0.5 * (sh[p.so.ub + k] + sh[p.so.lb + k]) : 0.0;
        rc[L.oV + t] = *bad ? __builtin_nan("") : v;
    }
}

static size_t wg_retarget_lds_bytes(int nx, int nu, int N)
{
    const int np = (N * nu + BS - 1) / BS * BS;
    return sizeof(double) * (size_t)(wg_ctl_rec_layout(nx, nu, N).img + np + nx * nx + nx * nu + 2 * nx + 2);
}

bool launch_wg_ctl_retarget(const KParams &p, hipStream_t stream)
{
    if (!wg_supported(p.nx, p.nu, p.N) || p.Bsz < 1) return false;
    const size_t bytes = wg_retarget_lds_bytes(p.nx, p.nu, p.N);
    const hipError_t e = hipFuncSetAttribute((const void *)lqmpc_wg_ctl_retarget_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) {
        fprintf(stderr, "lqmpc: hipFuncSetAttribute(%zu bytes of LDS): %s\n", bytes, hipGetErrorString(e));
        return false;
    }
    hipLaunchKernelGGL(lqmpc_wg_ctl_retarget_kernel, dim3((unsigned)p.Bsz), dim3(256), bytes, stream, p);
    return true;
}

// ---- new models for listed instances (lqmpc_controller_set_model): the controller's instance-minor copies of A and B ----
// Element (e, j) of the update's arrays (instance-minor over the update: e * count + j) goes to e * Bsz + idx[j] of the copies: rows
// e < nA belong to A, the nB rows behind them to B.  Lane = j, one 8-byte element per lane: the reads are coalesced, the writes land
// wherever the list sends them.  An index outside [0, Bsz) writes nothing.
constexpr int SCATTER_WG = 256;

__global__ void __launch_bounds__(SCATTER_WG) lqmpc_ctl_scatter_model_kernel(double *A, double *B, const double *uA, const double *uB,
                                                                             const int *idx, int nA, int nB, long long count, long long Bsz)
{
    const long long j = (long long)blockIdx.x * SCATTER_WG + threadIdx.x;
    if (j >= count) return;
    const long long b = idx[j];
    if ((unsigned long long)b >= (unsigned long long)Bsz) return;
    const int e = blockIdx.y;                // (grid.y = nA + nB)
    if (e < nA) A[(long long)e * Bsz + b] = uA[(long long)e * count + j];
    else B[(long long)(e - nA) * Bsz + b] = uB[(long long)(e - nA) * count + j];
}

void launch_ctl_scatter_model(double *A, double *B, const double *uA, const double *uB, const int *idx, int nx, int nu, long long count,
                              long long Bsz, hipStream_t stream)
{
    const dim3 grid((unsigned)((count + SCATTER_WG - 1) / SCATTER_WG), (unsigned)(nx * nx + nx * nu));
    hipLaunchKernelGGL(lqmpc_ctl_scatter_model_kernel, grid, dim3(SCATTER_WG), 0, stream, A, B, uA, uB, idx, nx * nx, nx * nu, count, Bsz);
}

}  // namespace lqmpc
