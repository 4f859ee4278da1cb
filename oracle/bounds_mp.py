"""TEST INFRASTRUCTURE (50-digit reference of the spectral numbers behind lqmpc_bounds_batch; only tests/ may import it).

Written from the problem statement, as exact.py is: the inputs are the fp64 matrices taken as exact, every operation below runs in
mpmath at mp.dps = 50, and nothing here shares a method with the kernels (doubling, repeated squaring, Householder + Sturm counts)
or with the fp64 host oracle (LAPACK, scipy's DARE), so a disagreement says which side is wrong.

    dare(A, B, Q, R)             P, K (u = -K x) of the discrete algebraic Riccati equation, with its own certificate
    spectra(N, A, B, Q, R, K)    |A|_2 |B|_2 |K|_2 |Gamma|_2 |Phi|_2, lambda_min / lambda_max(hat H), rho(A - BK)

Everything is returned as mpmath numbers / matrices; the caller rounds.  Meant for N n_u <= 33 (mp.eigsy takes about a second
there)."""
import numpy as np
from mpmath import mp, mpf

DPS = 50


class CertificateError(ValueError):
    """dare() could not certify a stabilising solution: the DARE residual or rho(A - BK) < 1 failed."""


def _mat(M):
    M = np.atleast_2d(np.asarray(M, dtype=np.float64))
    return mp.matrix([[mpf(float(v)) for v in row] for row in M])


def _fro(M):
    return mp.sqrt(sum(M[i, j] ** 2 for i in range(M.rows) for j in range(M.cols)))


def _sym(M):
    return (M + M.T) / 2


def spectral_radius(M):
    if M.rows == 1:
        return abs(M[0, 0])
    ev = mp.eig(M, left=False, right=False)
    return max(abs(v) for v in ev)


def _gain(A, B, R, P):
    BtP = B.T * P
    M, F = _sym(R + BtP * B), BtP * A
    K = mp.zeros(F.rows, F.cols)
    for c in range(F.cols):                                # (mp.lu_solve takes one right-hand side)
        K[:, c] = mp.lu_solve(M, F[:, c])
    return K


def _residual(A, B, Q, R, P):
    K = _gain(A, B, R, P)
    return A.T * P * A - P - (A.T * P * B) * K + Q


def _lyapunov(Acl, W):
    """P = Acl' P Acl + W for rho(Acl) < 1: P = sum_k (Acl^k)' W Acl^k, summed by squaring (P <- P + M' P M, M <- M^2)."""
    P, M = W.copy(), Acl.copy()
    for _ in range(64):
        step = M.T * P * M
        P = _sym(P + step)
        if _fro(step) <= mpf(10) ** (-(DPS - 4)) * _fro(P):
            return P
        M = M * M
    raise CertificateError("the Lyapunov series does not converge: the closed loop is not strictly stable")


def dare(A, B, Q, R):
    """P, K of A'PA - P - A'PB (R + B'PB)^-1 B'PA + Q = 0 with rho(A - BK) < 1, K = (R + B'PB)^-1 B'PA.

    Newton-Kleinman steps in mp from scipy's fp64 solution (from K = 0 where A is stable and scipy gives up).  Every call checks
    the certificate |residual|_F <= 1e-30 |P|_F and rho(A - BK) < 1 and raises CertificateError if it fails."""
    import scipy.linalg
    with mp.workdps(DPS):
        Am, Bm, Qm, Rm = _mat(A), _mat(B), _mat(Q), _mat(R)
        A64, B64 = np.atleast_2d(np.asarray(A, float)), np.atleast_2d(np.asarray(B, float))
        try:
            P0 = scipy.linalg.solve_discrete_are(A64, B64, np.atleast_2d(np.asarray(Q, float)), np.atleast_2d(np.asarray(R, float)))
            K = _gain(Am, Bm, Rm, _mat(P0))
        except (np.linalg.LinAlgError, ValueError, ZeroDivisionError):
            K = mp.zeros(Bm.cols, Am.rows)
        P = None
        for _ in range(30):
            Acl = Am - Bm * K
            if not spectral_radius(Acl) < 1:
                raise CertificateError("no stabilising gain: rho(A - BK) >= 1")
            P = _lyapunov(Acl, _sym(Qm + K.T * Rm * K))
            K = _gain(Am, Bm, Rm, P)
            if _fro(_residual(Am, Bm, Qm, Rm, P)) <= mpf(10) ** (-(DPS - 10)) * _fro(P):
                break
        res, rho = _fro(_residual(Am, Bm, Qm, Rm, P)), spectral_radius(Am - Bm * K)
        if not (res <= mpf(10) ** (-30) * _fro(P) and rho < 1):
            raise CertificateError(f"DARE certificate failed: residual {mp.nstr(res / _fro(P), 5)} |P|, rho(A - BK) = {mp.nstr(rho, 8)}")
        return P, K


def gamma_phi(N, A, B):
    """Gamma ((N + 1) n_x rows, a leading zero block row; block (r, c) = A^(r-1-c) B for r > c) and Phi = [I; A; ...; A^N], the
    pairing of bounds_np.gamma_phi."""
    nx, nu = B.rows, B.cols
    pw = [mp.eye(nx)]
    for _ in range(N):
        pw.append(A * pw[-1])
    G = mp.zeros((N + 1) * nx, N * nu)
    Phi = mp.zeros((N + 1) * nx, nx)
    for r in range(N + 1):
        Phi[r * nx:(r + 1) * nx, 0:nx] = pw[r]
        for c in range(r):
            G[r * nx:(r + 1) * nx, c * nu:(c + 1) * nu] = pw[r - 1 - c] * B
    return G, Phi


def _kron_eye_right(M, k):
    """kron(M, I_k)"""
    m = M.rows
    O = mp.zeros(m * k, m * k)
    for a in range(m):
        for b in range(m):
            if M[a, b] != 0:
                for s in range(k):
                    O[a * k + s, b * k + s] = M[a, b]
    return O


def _sym_extremes(S):
    ev = mp.eigsy(_sym(S), eigvals_only=True)
    ev = [ev[i] for i in range(len(ev))]
    return min(ev), max(ev)


def _gram(M):
    """the smaller Gram matrix of M"""
    return M.T * M if M.cols <= M.rows else M * M.T


def spectra(N, A, B, Q, R, K):
    """The spectral numbers of one system: dict with norm_A, norm_B, norm_K, norm_Gamma, norm_Phi (mp.eigsy on the Gram matrices),
    min_eig_H, max_eig_H of hat H = kron(R, I_N) + Gamma' kron(Q, I_{N+1}) Gamma, rho_cl = rho(A - BK) (mp.eig), and lam_* = the
    largest eigenvalue of each Gram matrix (the scale of the bars)."""
    with mp.workdps(DPS):
        Am, Bm, Qm, Rm = _mat(A), _mat(B), _mat(Q), _mat(R)
        Km = K if isinstance(K, mp.matrix) else _mat(K)
        G, Phi = gamma_phi(N, Am, Bm)
        out = {}
        for name, M in (("A", Am), ("B", Bm), ("K", Km), ("Gamma", G), ("Phi", Phi)):
            lam = _sym_extremes(_gram(M))[1]
            out["lam_" + name] = lam
            out["norm_" + name] = mp.sqrt(max(lam, mpf(0)))
        QG = mp.zeros(G.rows, G.cols)                      # kron(Q, I_{N+1}) Gamma without forming the Kronecker product
        nx, k = Qm.rows, N + 1
        for a in range(nx):
            for b in range(nx):
                if Qm[a, b] != 0:
                    for s in range(k):
                        for j in range(G.cols):
                            QG[a * k + s, j] += Qm[a, b] * G[b * k + s, j]
        hatH = _kron_eye_right(Rm, N) + G.T * QG
        out["min_eig_H"], out["max_eig_H"] = _sym_extremes(hatH)
        out["rho_cl"] = spectral_radius(Am - Bm * Km)
        return out


def to_float(M):
    """an mp matrix rounded to fp64"""
    return np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)])
