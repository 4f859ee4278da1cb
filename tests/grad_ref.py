"""Shared by tests/test_grad_cpu.py, tests/test_gpu_grad.py and tests/test_gpu_torch_layer_grad.py (not a test module).

Given cotangents w = d loss / d u_0 (nu, Bsz) and gam = d loss / d V_N (Bsz,), the gradient of the loss with respect to the model
matrices A and B of every instance, on the face the plan reports:

  reference()   long double, dense, from oracle/exact.py: on the face F of the plan U~_F = 1/2 H_FF^-1 w_F (w at stage 0, zero
                elsewhere), x~ = Gamma U~, the two costate recursions over the exact optimum of the face and over x~, and the sums
                    g_A  = sum_i (gam l_{i+1} - l~_{i+1}) x_i' - l_{i+1} x~_i'
                    g_B  = sum_i (gam l_{i+1} - l~_{i+1}) u_i' - l_{i+1} u~_i'
                    g_x0 = -A'l~_1 + gam (2 Q x_0 + A'l_1)
                No Riccati sweep anywhere.
  face_loss()   long double: w'u_0 + gam V at the optimum of a FIXED face, U_F = -H_FF^-1 (g_F + H_FA U_A), for any model; what the
                central differences of tests/test_grad_cpu.py differentiate.
  adjoint()     the numpy restatement (fp64; long double on request) of what lqmpc_grad_kernel computes: the masked Riccati sweep of sens_ref.masked_sweep
                (the same recursion, keeping K_j and Re_0), one forward roll, one backward pass.
  cotangents()  seeded random w and gam for a batch.
"""
import numpy as np

import sens_ref as sr
from oracle import exact as ex

LD = np.longdouble


def cotangents(nu, Bsz, seed):
    rng = np.random.default_rng(1000 + seed)
    return rng.standard_normal((nu, Bsz)), rng.standard_normal(Bsz)


def _time_major(U):
    """(nu, N, Bsz) -> (Bsz, N * nu), as exact.condense orders the variables"""
    nu, N, Bsz = U.shape
    return np.moveaxis(U, -1, 0).transpose(0, 2, 1).reshape(Bsz, N * nu)


def _costates(N, Al, Ql, Pl, X, xr):
    """l_1 .. l_N (N, Bsz, nx) of the states X (Bsz, N + 1, nx): l_N = 2 P (x_N - xr_{N-1}), l_i = 2 Q (x_i - xr_{i-1}) + A'l_{i+1}"""
    Bsz, nx = X.shape[0], X.shape[2]
    lam = np.zeros((N + 1, Bsz, nx), dtype=X.dtype)
    lam[N] = 2 * np.einsum("ij,bj->bi", Pl, X[:, N] - xr[N - 1])
    for i in range(N - 1, 0, -1):
        lam[i] = 2 * np.einsum("ij,bj->bi", Ql, X[:, i] - xr[i - 1]) + np.einsum("bji,bj->bi", Al, lam[i + 1])
    return lam


def _sums(N, Al, Ql, lam, lamt, X, U, Xt, Ut, gam):
    """the three sums of the module docstring; X, Xt (Bsz, N + 1, nx), U, Ut (Bsz, N, nu), lam, lamt (N + 1, Bsz, nx)"""
    gA = np.zeros(Al.shape, dtype=Al.dtype)
    gB = np.zeros((Al.shape[0], Al.shape[1], U.shape[2]), dtype=Al.dtype)
    for i in range(N):
        pq = gam[:, None] * lam[i + 1] - lamt[i + 1]
        gA += pq[:, :, None] * X[:, i][:, None, :] - lam[i + 1][:, :, None] * Xt[:, i][:, None, :]
        gB += pq[:, :, None] * U[:, i][:, None, :] - lam[i + 1][:, :, None] * Ut[:, i][:, None, :]
    dV = 2 * np.einsum("ij,bj->bi", Ql, X[:, 0]) + np.einsum("bji,bj->bi", Al, lam[1])
    gx = -np.einsum("bji,bj->bi", Al, lamt[1]) + gam[:, None] * dV
    return np.moveaxis(gA, 0, -1), np.moveaxis(gB, 0, -1), gx.T


def reference(p, kw, x0, U_plan, w, gam):
    """Long double, on the face of U_plan (nu, N, Bsz) as exact.certify reports it: {'g_A' (nx, nx, Bsz), 'g_B' (nx, nu, Bsz),
    'g_x0' (nx, Bsz), 'free' (nu, N, Bsz) bool, 'U' the exact optimum on that face, 'ok' the certificate of the active set}."""
    N, nu, nx, Bsz = p["N"], p["B"].shape[1], p["A"].shape[0], x0.shape[1]
    n = N * nu
    xr, ur = kw.get("x_ref"), kw.get("u_ref")
    cert = ex.certify(*sr.qa(p), x0, U_plan, xr, ur)
    free = sr.face_of(cert["U"], p["lb"], p["ub"])
    Us, Ff = _time_major(cert["U"]), _time_major(free)
    H, _, _ = ex.condense(*sr.model(p), x0, xr, ur)
    Al, Bl = np.moveaxis(np.asarray(p["A"], dtype=LD), -1, 0), np.moveaxis(np.asarray(p["B"], dtype=LD), -1, 0)
    Phi, Gam = ex.prediction(N, Al, Bl)
    Ql, Pl = np.asarray(p["Q"], dtype=LD), np.asarray(p["P"], dtype=LD)
    wl, gl, x0l = np.asarray(w, dtype=LD).T, np.asarray(gam, dtype=LD), np.asarray(x0, dtype=LD).T
    xrl = np.zeros((N, nx), dtype=LD) if xr is None else np.asarray(xr, dtype=LD).T
    Ut = np.zeros((Bsz, n), dtype=LD)
    for b in range(Bsz):
        F = np.flatnonzero(Ff[b, :nu])                             # the free inputs of stage 0 carry w
        Fa = np.flatnonzero(Ff[b])
        if F.size:
            rhs = np.zeros(n, dtype=LD)
            rhs[F] = wl[b, F]
            L = ex.cholesky(H[b][np.ix_(Fa, Fa)])
            Ut[b, Fa] = ex.chol_solve(L[None], rhs[Fa][None])[0] / 2
    def states(first, Uv):
        X = np.zeros((Bsz, N + 1, nx), dtype=LD)
        X[:, 0] = first
        X[:, 1:] = (np.einsum("bij,bj->bi", Phi, first) + np.einsum("bij,bj->bi", Gam, Uv)).reshape(Bsz, N, nx)
        return X
    X, Xt = states(x0l, Us), states(np.zeros((Bsz, nx), dtype=LD), Ut)
    lam = _costates(N, Al, Ql, Pl, X, xrl)
    lamt = _costates(N, Al, Ql, Pl, Xt, np.zeros((N, nx), dtype=LD))
    gA, gB, gx = _sums(N, Al, Ql, lam, lamt, X, Us.reshape(Bsz, N, nu), Xt, Ut.reshape(Bsz, N, nu), gl)
    return dict(g_A=gA, g_B=gB, g_x0=gx, free=free, U=cert["U"], ok=cert["ok"])


def face_loss(p, kw, x0, free, U_bound, w, gam, A=None, B=None):
    """(Bsz,) long double: w'u_0 + gam V at the optimum of the face `free` (nu, N, Bsz) with the other entries held at U_bound, for
    the model A, B (default: p's), long double arrays allowed"""
    A, B = p["A"] if A is None else A, p["B"] if B is None else B
    H, g, c = ex.condense(p["N"], A, B, p["Q"], p["R"], p["P"], x0, kw.get("x_ref"), kw.get("u_ref"))
    Ff, Ub = _time_major(free), np.asarray(_time_major(U_bound), dtype=LD)
    nu, Bsz = B.shape[1], B.shape[2]
    U = Ub.copy()
    for b in range(Bsz):
        F, Ac = np.flatnonzero(Ff[b]), np.flatnonzero(~Ff[b])
        if F.size:
            rhs = g[b][F] + H[b][np.ix_(F, Ac)] @ Ub[b, Ac]
            U[b, F] = -ex.chol_solve(ex.cholesky(H[b][np.ix_(F, F)])[None], rhs[None])[0]
    return np.einsum("kb,bk->b", np.asarray(w, dtype=LD), U[:, :nu]) + np.asarray(gam, dtype=LD) * ex.value(H, g, c, U)


def adjoint(N, A, B, Q, R, P, free, X, U, w, gam, x_ref=None, dtype=np.float64, chol=False, stats=None):
    """numpy, the algebra of lqmpc_grad_kernel: free (nu, N, Bsz) the face, X (nx, N + 1, Bsz) and U (nu, N, Bsz) the plan,
    w (nu, Bsz), gam (Bsz,).  Returns {'g_A', 'g_B', 'g_x0'}.  dtype, chol, stats: see sens_ref.stage_solver (fp64 and LU by default).
        the sweep of sens_ref.masked_sweep, keeping K_j of every stage and Re_0
        u~_0 = 1/2 f_0 Re_0^-1 f_0 w,  x~_0 = 0;  j = 0 .. N-1: u~_j = -K_j x~_j (j > 0),  x~_{j+1} = A x~_j + B u~_j
        the costates l (of X, with references) and l~ (of x~, without), backwards together, and the sums of the module docstring"""
    cast = lambda a: np.asarray(a, dtype=dtype)
    Ab, Bb = np.moveaxis(cast(A), -1, 0), np.moveaxis(cast(B), -1, 0)
    Q, R, P = cast(Q), cast(R), cast(P)
    Bsz, nx, nu = Bb.shape
    S = np.broadcast_to(P, (Bsz, nx, nx)).copy()
    Ks = [None] * N
    eye = np.eye(nu, dtype=dtype)
    solve = None
    for j in range(N - 1, -1, -1):
        f = free[:, j, :].T.astype(dtype)
        Bj = Bb * f[:, None, :]
        Rj = f[:, :, None] * R[None] * f[:, None, :] + eye[None] * (1 - f)[:, :, None]
        BtS = np.einsum("bji,bjk->bik", Bj, S)
        solve = sr.stage_solver(Rj + BtS @ Bj, dtype, chol, stats)
        Ks[j] = solve(BtS @ Ab)
        S = Q[None] + np.einsum("bji,bjk->bik", Ab, S @ (Ab - Bj @ Ks[j]))
    f0 = free[:, 0, :].T.astype(dtype)
    Xt, Ut = np.zeros((Bsz, N + 1, nx), dtype=dtype), np.zeros((Bsz, N, nu), dtype=dtype)
    Ut[:, 0] = f0 * solve((f0 * cast(w).T)[:, :, None])[:, :, 0] / 2
    for j in range(N):
        if j:
            Ut[:, j] = -np.einsum("bki,bi->bk", Ks[j], Xt[:, j])
        Xt[:, j + 1] = np.einsum("bij,bj->bi", Ab, Xt[:, j]) + np.einsum("bik,bk->bi", Bb, Ut[:, j])
    xr = np.zeros((N, nx), dtype=dtype) if x_ref is None else cast(x_ref).T
    Xb, Ub = np.moveaxis(cast(X), -1, 0).transpose(0, 2, 1), np.moveaxis(cast(U), -1, 0).transpose(0, 2, 1)
    lam = _costates(N, Ab, Q, P, Xb, xr)
    lamt = _costates(N, Ab, Q, P, Xt, np.zeros((N, nx), dtype=dtype))
    gA, gB, gx = _sums(N, Ab, Q, lam, lamt, Xb, Ub, Xt, Ut, cast(gam))
    return dict(g_A=gA, g_B=gB, g_x0=gx)
