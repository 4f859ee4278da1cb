"""Shared by tests/test_pgrad_cpu.py, tests/test_gpu_pgrad.py and tests/test_gpu_torch_layer_plan.py (not a test module).

Given cotangents on the whole plan -- w = d loss / d U_plan (nu, N, Bsz), s = d loss / d X_plan (nx, N + 1, Bsz; s_0 acts on the given
state) and gam = d loss / d V_N (Bsz,) -- the gradient of the loss with respect to the model matrices A and B and the given state of
every instance, on the face the plan reports:

  reference()   long double, dense, from oracle/exact.py: on the face F of the plan U~_F = 1/2 H_FF^-1 (w + Gamma's_{1..N})_F,
                x~ = Gamma U~, the costates l of the exact optimum of the face and l~ of x~ (l~_N = 2 P x~_N - s_N,
                l~_i = 2 Q x~_i - s_i + A'l~_{i+1}) and the sums
                    g_A  = sum_i (gam l_{i+1} - l~_{i+1}) x_i' - l_{i+1} x~_i'
                    g_B  = sum_i (gam l_{i+1} - l~_{i+1}) u_i' - l_{i+1} u~_i'
                    g_x0 = s_0 - A'l~_1 + gam (2 Q x_0 + A'l_1)
                No Riccati sweep anywhere.
  face_loss()   long double: sum_i w_i'u_i + sum_i s_i'x_i + gam V at the optimum of a FIXED face, U_F = -H_FF^-1 (g_F + H_FA U_A), for
                any model and any given state; what the central differences of tests/test_pgrad_cpu.py differentiate.
  adjoint()     the numpy restatement (fp64; long double on request) of what lqmpc_plan_grad_kernel computes: the masked Riccati
                sweep of sens_ref.masked_sweep with an affine part carried beside S (pi_N = s_N,
                kap_j = 1/2 f_j Re_j^-1 f_j (w_j + B'pi_{j+1}), pi_j = s_j + (A - B_j K_j)'pi_{j+1} - K_j'f_j w_j), one forward roll
                u~_j = -K_j x~_j + kap_j, one backward pass.
  cotangents()  seeded random w, s and gam for a batch, gam exactly 0 on every third instance.
"""
import numpy as np

import grad_ref as gr
import sens_ref as sr
from oracle import exact as ex

LD = np.longdouble
KEYS = (("g_A", (0, 1)), ("g_B", (0, 1)), ("g_x0", 0))


def cotangents(nx, nu, N, Bsz, seed):
    rng = np.random.default_rng(2000 + seed)
    w, s, gam = rng.standard_normal((nu, N, Bsz)), rng.standard_normal((nx, N + 1, Bsz)), rng.standard_normal(Bsz)
    gam[::3] = 0.0
    return w, s, gam


def _stage_major(S):
    """(nx, N + 1, Bsz) -> (Bsz, N + 1, nx)"""
    return np.moveaxis(S, -1, 0).transpose(0, 2, 1)


def _costates_adj(N, Al, Ql, Pl, Xt, s):
    """l~_1 .. l~_N (N + 1, Bsz, nx) of the adjoint states Xt (Bsz, N + 1, nx) and the cotangents s (Bsz, N + 1, nx)"""
    lam = np.zeros((N + 1,) + Xt[:, 0].shape, dtype=Xt.dtype)
    lam[N] = 2 * np.einsum("ij,bj->bi", Pl, Xt[:, N]) - s[:, N]
    for i in range(N - 1, 0, -1):
        lam[i] = 2 * np.einsum("ij,bj->bi", Ql, Xt[:, i]) - s[:, i] + np.einsum("bji,bj->bi", Al, lam[i + 1])
    return lam


def reference(p, kw, x0, U_plan, w, s, gam):
    """Long double, on the face of U_plan (nu, N, Bsz) as exact.certify reports it: {'g_A' (nx, nx, Bsz), 'g_B' (nx, nu, Bsz),
    'g_x0' (nx, Bsz), 'free' (nu, N, Bsz) bool, 'U' the exact optimum on that face, 'ok' the certificate of the active set}."""
    N, nu, nx, Bsz = p["N"], p["B"].shape[1], p["A"].shape[0], x0.shape[1]
    n = N * nu
    xr, ur = kw.get("x_ref"), kw.get("u_ref")
    cert = ex.certify(*sr.qa(p), x0, U_plan, xr, ur)
    free = sr.face_of(cert["U"], p["lb"], p["ub"])
    Us, Ff = gr._time_major(cert["U"]), gr._time_major(free)
    H, _, _ = ex.condense(*sr.model(p), x0, xr, ur)
    Al, Bl = np.moveaxis(np.asarray(p["A"], dtype=LD), -1, 0), np.moveaxis(np.asarray(p["B"], dtype=LD), -1, 0)
    Phi, Gam = ex.prediction(N, Al, Bl)
    Ql, Pl = np.asarray(p["Q"], dtype=LD), np.asarray(p["P"], dtype=LD)
    wl, sl = np.asarray(gr._time_major(w), dtype=LD), np.asarray(_stage_major(s), dtype=LD)
    gl, x0l = np.asarray(gam, dtype=LD), np.asarray(x0, dtype=LD).T
    xrl = np.zeros((N, nx), dtype=LD) if xr is None else np.asarray(xr, dtype=LD).T
    rhs = wl + np.einsum("bij,bi->bj", Gam, sl[:, 1:].reshape(Bsz, N * nx))
    Ut = np.zeros((Bsz, n), dtype=LD)
    for b in range(Bsz):
        Fa = np.flatnonzero(Ff[b])
        if Fa.size:
            L = ex.cholesky(H[b][np.ix_(Fa, Fa)])
            Ut[b, Fa] = ex.chol_solve(L[None], rhs[b, Fa][None])[0] / 2

    def states(first, Uv):
        X = np.zeros((Bsz, N + 1, nx), dtype=LD)
        X[:, 0] = first
        X[:, 1:] = (np.einsum("bij,bj->bi", Phi, first) + np.einsum("bij,bj->bi", Gam, Uv)).reshape(Bsz, N, nx)
        return X
    X, Xt = states(x0l, Us), states(np.zeros((Bsz, nx), dtype=LD), Ut)
    lam = gr._costates(N, Al, Ql, Pl, X, xrl)
    lamt = _costates_adj(N, Al, Ql, Pl, Xt, sl)
    gA, gB, gx = gr._sums(N, Al, Ql, lam, lamt, X, Us.reshape(Bsz, N, nu), Xt, Ut.reshape(Bsz, N, nu), gl)
    return dict(g_A=gA, g_B=gB, g_x0=gx + sl[:, 0].T, free=free, U=cert["U"], ok=cert["ok"])


def face_loss(p, kw, x0, free, U_bound, w, s, gam, A=None, B=None):
    """(Bsz,) long double: sum_i w_i'u_i + sum_i s_i'x_i + gam V at the optimum of the face `free` (nu, N, Bsz) with the other entries
    held at U_bound, for the model A, B (default: p's) and the given state x0 (nx, Bsz), long double arrays allowed"""
    A, B = p["A"] if A is None else A, p["B"] if B is None else B
    N = p["N"]
    H, g, c = ex.condense(N, A, B, p["Q"], p["R"], p["P"], x0, kw.get("x_ref"), kw.get("u_ref"))
    Ff, Ub = gr._time_major(free), np.asarray(gr._time_major(U_bound), dtype=LD)
    nx, Bsz = B.shape[0], B.shape[2]
    U = Ub.copy()
    faces, which = np.unique(Ff, axis=0, return_inverse=True)      # the instances of one face are solved together
    for m, face in enumerate(faces):
        F, Ac, rows = np.flatnonzero(face), np.flatnonzero(~face), np.flatnonzero(which.reshape(-1) == m)
        if F.size:
            Hr = H[rows]
            rhs = g[rows][:, F] + np.einsum("bij,bj->bi", Hr[:, F][:, :, Ac], Ub[rows][:, Ac])
            U[np.ix_(rows, F)] = -ex.chol_solve(ex.cholesky(Hr[:, F][:, :, F]), rhs)
    Phi, Gam = ex.prediction(N, np.moveaxis(np.asarray(A, dtype=LD), -1, 0), np.moveaxis(np.asarray(B, dtype=LD), -1, 0))
    x0l = np.asarray(x0, dtype=LD).T
    X = np.einsum("bij,bj->bi", Phi, x0l) + np.einsum("bij,bj->bi", Gam, U)
    sl = np.asarray(_stage_major(s), dtype=LD)
    return (np.einsum("bi,bi->b", np.asarray(gr._time_major(w), dtype=LD), U) + np.einsum("bi,bi->b", sl[:, 0], x0l) +
            np.einsum("bi,bi->b", sl[:, 1:].reshape(Bsz, N * nx), X) + np.asarray(gam, dtype=LD) * ex.value(H, g, c, U))


def adjoint(N, A, B, Q, R, P, free, X, U, w, s, gam, x_ref=None, dtype=np.float64, chol=False, stats=None):
    """numpy, the algebra of lqmpc_plan_grad_kernel: free (nu, N, Bsz) the face, X (nx, N + 1, Bsz) and U (nu, N, Bsz) the plan,
    w (nu, N, Bsz), s (nx, N + 1, Bsz), gam (Bsz,).  Returns {'g_A', 'g_B', 'g_x0'}.  dtype, chol, stats: see sens_ref.stage_solver."""
    cast = lambda a: np.asarray(a, dtype=dtype)
    Ab, Bb = np.moveaxis(cast(A), -1, 0), np.moveaxis(cast(B), -1, 0)
    Q, R, P = cast(Q), cast(R), cast(P)
    Bsz, nx, nu = Bb.shape
    wb, sb = np.moveaxis(cast(w), -1, 0).transpose(0, 2, 1), cast(_stage_major(s))            # (Bsz, N, nu), (Bsz, N + 1, nx)
    S = np.broadcast_to(P, (Bsz, nx, nx)).copy()
    pi = sb[:, N].copy()
    Ks, kap = [None] * N, [None] * N
    eye = np.eye(nu, dtype=dtype)
    for j in range(N - 1, -1, -1):
        f = free[:, j, :].T.astype(dtype)
        Bj = Bb * f[:, None, :]
        Rj = f[:, :, None] * R[None] * f[:, None, :] + eye[None] * (1 - f)[:, :, None]
        BtS = np.einsum("bji,bjk->bik", Bj, S)
        solve = sr.stage_solver(Rj + BtS @ Bj, dtype, chol, stats)
        Ks[j] = solve(BtS @ Ab)
        fw = f * wb[:, j]
        kap[j] = f * solve((fw + np.einsum("bik,bi->bk", Bj, pi))[:, :, None])[:, :, 0] / 2
        Acl = Ab - Bj @ Ks[j]
        pi = sb[:, j] + np.einsum("bji,bj->bi", Acl, pi) - np.einsum("bki,bk->bi", Ks[j], fw)
        S = Q[None] + np.einsum("bji,bjk->bik", Ab, S @ Acl)
    Xt, Ut = np.zeros((Bsz, N + 1, nx), dtype=dtype), np.zeros((Bsz, N, nu), dtype=dtype)
    for j in range(N):
        Ut[:, j] = kap[j] - np.einsum("bki,bi->bk", Ks[j], Xt[:, j])
        Xt[:, j + 1] = np.einsum("bij,bj->bi", Ab, Xt[:, j]) + np.einsum("bik,bk->bi", Bb, Ut[:, j])
    xr = np.zeros((N, nx), dtype=dtype) if x_ref is None else cast(x_ref).T
    Xb, Ub = np.moveaxis(cast(X), -1, 0).transpose(0, 2, 1), np.moveaxis(cast(U), -1, 0).transpose(0, 2, 1)
    lam = gr._costates(N, Ab, Q, P, Xb, xr)
    lamt = _costates_adj(N, Ab, Q, P, Xt, sb)
    gA, gB, gx = gr._sums(N, Ab, Q, lam, lamt, Xb, Ub, Xt, Ut, cast(gam))
    return dict(g_A=gA, g_B=gB, g_x0=gx + sb[:, 0].T)
