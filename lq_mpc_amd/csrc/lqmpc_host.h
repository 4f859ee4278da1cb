// lqmpc_host.h -- the parts of the host side (lqmpc_api.hip) that need no HIP, so that a plain C++ program can test them
// (tests/host_units.cpp): the layout of the staging arena of a host-flavour call, and the small dense helpers behind the bound
// coefficients and the difficulty order.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace lqmpc {

constexpr size_t ARENA_ALIGN = 256;

// Where every array of one host-flavour call lies in its staging block.  add() each array once, then place(): the inputs come first
// in the order given, the outputs behind them, each at a multiple of ARENA_ALIGN.  [0, in_end) is what is uploaded, [in_end, total)
// what is copied back; an absent (NULL) array takes no room and keeps offset 0.
struct ArenaLayout {
    struct Slot {
        size_t bytes;
        bool out, present;
        size_t off;
    };
    std::vector<Slot> slots;
    size_t in_end = 0, total = 0;

    void add(size_t bytes, bool out, bool present) { slots.push_back(Slot{bytes, out, present, 0}); }
    void place()
    {
        size_t off = 0;
        for (int out = 0; out < 2; ++out) {
            for (Slot &s : slots)
                if (s.present && s.out == (out == 1)) {
                    s.off = off;
                    off = (off + s.bytes + ARENA_ALIGN - 1) / ARENA_ALIGN * ARENA_ALIGN;
                }
            if (!out) in_end = off;
        }
        total = off;
    }
};

}  // namespace lqmpc

// small host-side dense helpers for the batch-shared weights (lqmpc_bounds_batch): SPD inverse, extreme eigenvalues
static inline bool host_spd_inverse(std::vector<double> &M, int n)
{
    for (int k = 0; k < n; ++k) {
        const double d = M[k * n + k];
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        const double p = 1.0 / d;
        M[k * n + k] = 1.0;
        for (int j = 0; j < n; ++j) M[k * n + j] *= p;
        for (int i = 0; i < n; ++i) {
            if (i == k) continue;
            const double f = M[i * n + k];
            M[i * n + k] = 0.0;
            for (int j = 0; j < n; ++j) M[i * n + j] -= f * M[k * n + j];
        }
    }
    return true;
}

static inline bool host_sym_eig_extremes(const double *Min, int n, double &emax, double &emin)
{
    std::vector<double> M(Min, Min + n * n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j)
            if (std::fabs(M[i * n + j] - M[j * n + i]) > 1e-12 * (std::fabs(M[i * n + i]) + std::fabs(M[j * n + j]))) return false;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, dg = 0.0;
        for (int p = 0; p < n; ++p) {
            dg += M[p * n + p] * M[p * n + p];
            for (int q = p + 1; q < n; ++q) off += M[p * n + q] * M[p * n + q];
        }
        if (!(off > 1e-32 * (dg + off))) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = M[p * n + q];
                if (std::fabs(apq) < 1e-300) continue;
                const double theta = (M[q * n + q] - M[p * n + p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; ++k) {
                    const double akp = M[k * n + p], akq = M[k * n + q];
                    M[k * n + p] = c * akp - s * akq; M[k * n + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {
                    const double apk = M[p * n + k], aqk = M[q * n + k];
                    M[p * n + k] = c * apk - s * aqk; M[q * n + k] = s * apk + c * aqk;
                }
            }
    }
    emax = -1e308; emin = 1e308;
    for (int p = 0; p < n; ++p) { emax = std::max(emax, M[p * n + p]); emin = std::min(emin, M[p * n + p]); }
    return std::isfinite(emax) && std::isfinite(emin);
}

// First gain K_0 of the N-stage problem on (A, B): S_N = P, K_j = (R + B'S B)^-1 B'S A, S <- Q + A'S (A - B K_j).  Row-major, nu x nx.
// (Host, once per call of a rollout with a shared plant: the difficulty order's roll uses it; 10 x O(nx^3) flops.)
static inline bool host_first_gain(int nx, int nu, int N, const double *A, const double *B, const double *Q, const double *R, const double *P, double *K)
{
    std::vector<double> S(P, P + nx * nx), SA(nx * nx), SB(nx * nu), Re(nu * nu), F(nu * nx), Acl(nx * nx), T(nx * nx);
    for (int j = 0; j < N; ++j) {
        for (int a = 0; a < nx; ++a) {
            for (int c = 0; c < nx; ++c) { double t = 0.0; for (int k = 0; k < nx; ++k) t += S[a * nx + k] * A[k * nx + c]; SA[a * nx + c] = t; }
            for (int c = 0; c < nu; ++c) { double t = 0.0; for (int k = 0; k < nx; ++k) t += S[a * nx + k] * B[k * nu + c]; SB[a * nu + c] = t; }
        }
        for (int r = 0; r < nu; ++r) {
            for (int c = 0; c < nu; ++c) { double t = R[r * nu + c]; for (int k = 0; k < nx; ++k) t += B[k * nu + r] * SB[k * nu + c]; Re[r * nu + c] = t; }
            for (int c = 0; c < nx; ++c) { double t = 0.0; for (int k = 0; k < nx; ++k) t += B[k * nu + r] * SA[k * nx + c]; F[r * nx + c] = t; }
        }
        // K = Re^-1 F by Gaussian elimination with partial pivoting (nu <= 8)
        for (int col = 0; col < nu; ++col) {
            int piv = col;
            for (int r = col + 1; r < nu; ++r) if (std::fabs(Re[r * nu + col]) > std::fabs(Re[piv * nu + col])) piv = r;
            if (!(std::fabs(Re[piv * nu + col]) > 0.0)) return false;
            if (piv != col) {
                for (int c = 0; c < nu; ++c) std::swap(Re[piv * nu + c], Re[col * nu + c]);
                for (int c = 0; c < nx; ++c) std::swap(F[piv * nx + c], F[col * nx + c]);
            }
            const double inv = 1.0 / Re[col * nu + col];
            for (int r = 0; r < nu; ++r) {
                if (r == col) continue;
                const double f = Re[r * nu + col] * inv;
                for (int c = 0; c < nu; ++c) Re[r * nu + c] -= f * Re[col * nu + c];
                for (int c = 0; c < nx; ++c) F[r * nx + c] -= f * F[col * nx + c];
            }
        }
        for (int r = 0; r < nu; ++r) { const double inv = 1.0 / Re[r * nu + r]; for (int c = 0; c < nx; ++c) K[r * nx + c] = F[r * nx + c] * inv; }
        for (int a = 0; a < nx; ++a)
            for (int c = 0; c < nx; ++c) { double t = A[a * nx + c]; for (int k = 0; k < nu; ++k) t -= B[a * nu + k] * K[k * nx + c]; Acl[a * nx + c] = t; }
        for (int a = 0; a < nx; ++a)
            for (int c = 0; c < nx; ++c) { double t = 0.0; for (int k = 0; k < nx; ++k) t += S[a * nx + k] * Acl[k * nx + c]; T[a * nx + c] = t; }
        for (int a = 0; a < nx; ++a)
            for (int c = 0; c < nx; ++c) { double t = Q[a * nx + c]; for (int k = 0; k < nx; ++k) t += A[k * nx + a] * T[k * nx + c]; S[a * nx + c] = t; }
    }
    for (int e = 0; e < nu * nx; ++e) if (!std::isfinite(K[e])) return false;
    return true;
}
