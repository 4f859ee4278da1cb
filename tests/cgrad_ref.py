"""Shared by tests/test_cgrad_cpu.py, tests/test_gpu_cgrad.py and tests/test_gpu_torch_layer_refs.py (not a test module).

Given cotangents w = d loss / d u_0 (nu, Bsz) and gam = d loss / d V_N (Bsz,), the gradient of the loss with respect to the data the
batch shares -- the weights Q, R, P, the references x_ref, u_ref and the box lb, ub -- per instance, on the face the plan reports
(DESIGN.md section 4.12).  With e_i = x_i - xref_{i-1}, d_i = u_i - uref_i, the adjoint plan u~, x~ (x~_0 = 0) and the costates
l, l~ of tests/grad_ref.py, r_i = 2 R d_i + B'l_{i+1} and r~_i = 2 R u~_i + B'l~_{i+1}:

    g_Q = gam x0 x0' + sum_{i=1}^{N-1} (gam e_i e_i' - x~_i e_i' - e_i x~_i')       g_P = the same term at i = N
    g_R = sum_{i=0}^{N-1} (gam d_i d_i' - u~_i d_i' - d_i u~_i')
    g_xref[:, i-1] = 2 Q (x~_i - gam e_i)  (P at i = N)                              g_uref[:, i] = 2 R (u~_i - gam d_i)
    g_ub[k] = sum over the entries (i, k) held at the upper bound of gam r_i[k] - r~_i[k] + (i == 0 ? w_k : 0);  g_lb likewise

  reference()   long double, dense, from oracle/exact.py: on the face F of the plan U~_F = 1/2 H_FF^-1 w_F, x~ = Gamma U~, the
                stage gradients from the condensed problem itself, r = 2 (H U + g) and r~ = 2 H U~ (no costate, no Riccati sweep).
  face_loss()   long double: w'u_0 + gam V at the optimum of a FIXED face for overridden weights, references and bounds; the entries
                held at a bound move with the bound.  What the central differences of tests/test_cgrad_cpu.py differentiate.
  adjoint()     the numpy restatement (fp64; long double on request) of what lqmpc_cost_grad_kernel computes: the masked Riccati sweep, one forward roll, the
                two costate recursions and the sums.
"""
import numpy as np

import grad_ref as gr
import sens_ref as sr
from oracle import exact as ex

LD = np.longdouble
KEYS = (("g_Q", (0, 1)), ("g_R", (0, 1)), ("g_P", (0, 1)), ("g_lb", 0), ("g_ub", 0), ("g_xref", (0, 1)), ("g_uref", (0, 1)))


def sizes(nx, nu, N):
    """the shapes of the seven outputs without the instance axis, in the order of KEYS"""
    return dict(g_Q=(nx, nx), g_R=(nu, nu), g_P=(nx, nx), g_lb=(nu,), g_ub=(nu,), g_xref=(nx, N), g_uref=(nu, N))


def _sums(N, Q, R, P, X, U, Xt, Ut, xr, ur, r, rt, side, w, gam):
    """the seven formulas; X, Xt (Bsz, N + 1, nx), U, Ut, r, rt, side (Bsz, N, nu), xr (N, nx), ur (N, nu), w (Bsz, nu), gam (Bsz,)"""
    g1, g2 = gam[:, None], gam[:, None, None]
    E, D = X[:, 1:] - xr[None], U - ur[None]
    outer = lambda a, b: a[:, :, None] * b[:, None, :]
    term = lambda e, t: g2 * outer(e, e) - outer(t, e) - outer(e, t)
    gQ = g2 * outer(X[:, 0], X[:, 0])
    for i in range(1, N):
        gQ = gQ + term(E[:, i - 1], Xt[:, i])
    gP = term(E[:, N - 1], Xt[:, N])
    gR = 0
    for i in range(N):
        gR = gR + term(D[:, i], Ut[:, i])
    W = [Q] * (N - 1) + [P]
    gxr = np.stack([2 * np.einsum("ij,bj->bi", W[i - 1], Xt[:, i] - g1 * E[:, i - 1]) for i in range(1, N + 1)], axis=2)
    gur = np.stack([2 * np.einsum("ij,bj->bi", R, Ut[:, i] - g1 * D[:, i]) for i in range(N)], axis=2)
    c = g2 * r - rt
    c[:, 0] = c[:, 0] + w
    zero = np.zeros_like(c)
    glb, gub = np.where(side < 0, c, zero).sum(axis=1), np.where(side > 0, c, zero).sum(axis=1)
    mv = lambda a: np.moveaxis(a, 0, -1)
    return dict(g_Q=mv(gQ), g_R=mv(gR), g_P=mv(gP), g_lb=glb.T, g_ub=gub.T, g_xref=mv(gxr), g_uref=mv(gur))


def side_of(U_exact, lb, ub):
    """(nu, N, Bsz) int: -1 where an entry of a plan from exact.certify IS lb, +1 where it is ub, 0 where it is free"""
    lo, hi = np.asarray(lb, dtype=LD)[:, None, None], np.asarray(ub, dtype=LD)[:, None, None]
    return (U_exact == hi).astype(int) - (U_exact == lo).astype(int)


def side_bits(U, lb, ub):
    """the same from an fp64 plan by the bit-for-bit rule of include/lqmpc.h: lb or c - h is lower, ub or c + h is upper"""
    lb, ub = np.asarray(lb, dtype=np.float64)[:, None, None], np.asarray(ub, dtype=np.float64)[:, None, None]
    c, h = 0.5 * (ub + lb), 0.5 * (ub - lb)
    return ((U == ub) | (U == c + h)).astype(int) - ((U == lb) | (U == c - h)).astype(int)


def _refs(kw, nx, nu, N, dtype):
    xr, ur = kw.get("x_ref"), kw.get("u_ref")
    return (np.zeros((N, nx), dtype=dtype) if xr is None else np.asarray(xr, dtype=dtype).T,
            np.zeros((N, nu), dtype=dtype) if ur is None else np.asarray(ur, dtype=dtype).T)


def reference(p, kw, x0, U_plan, w, gam):
    """Long double, on the face of U_plan (nu, N, Bsz) as exact.certify reports it: the seven outputs of KEYS with the instance axis
    last, 'free' and 'side' (nu, N, Bsz), 'U' the exact optimum on that face, 'ok' the certificate of the active set."""
    N, nu, nx, Bsz = p["N"], p["B"].shape[1], p["A"].shape[0], x0.shape[1]
    n = N * nu
    xr, ur = kw.get("x_ref"), kw.get("u_ref")
    cert = ex.certify(*sr.qa(p), x0, U_plan, xr, ur)
    side = side_of(cert["U"], p["lb"], p["ub"])
    free = side == 0
    Us, Ff = gr._time_major(cert["U"]), gr._time_major(free)
    H, g, _ = ex.condense(*sr.model(p), x0, xr, ur)
    Al, Bl = np.moveaxis(np.asarray(p["A"], dtype=LD), -1, 0), np.moveaxis(np.asarray(p["B"], dtype=LD), -1, 0)
    Phi, Gam = ex.prediction(N, Al, Bl)
    wl, gl, x0l = np.asarray(w, dtype=LD).T, np.asarray(gam, dtype=LD), np.asarray(x0, dtype=LD).T
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
    r = 2 * (np.einsum("bij,bj->bi", H, Us) + g)
    rt = 2 * np.einsum("bij,bj->bi", H, Ut)
    xrl, url = _refs(kw, nx, nu, N, LD)
    out = _sums(N, *(np.asarray(p[k], dtype=LD) for k in "QRP"), X, Us.reshape(Bsz, N, nu), Xt, Ut.reshape(Bsz, N, nu), xrl, url,
                r.reshape(Bsz, N, nu), rt.reshape(Bsz, N, nu), np.moveaxis(side, -1, 0).transpose(0, 2, 1), wl, gl)
    out.update(free=free, side=side, U=cert["U"], ok=cert["ok"])
    return out


def face_loss(p, kw, x0, side, w, gam, **over):
    """(Bsz,) long double: w'u_0 + gam V at the optimum of the face `side` (nu, N, Bsz; -1 held at lb, +1 held at ub, 0 free) with
    any of Q, R, P, x_ref, u_ref, lb, ub overridden (long double arrays allowed); a held entry sits on the overridden bound"""
    nu, N, Bsz = side.shape
    nx = p["A"].shape[0]
    get = lambda k: over[k] if k in over else p[k]
    xr = over["x_ref"] if "x_ref" in over else kw.get("x_ref")
    ur = over["u_ref"] if "u_ref" in over else kw.get("u_ref")
    H, g, c = ex.condense(p["N"], p["A"], p["B"], get("Q"), get("R"), get("P"), x0, xr, ur)
    lb, ub = np.asarray(get("lb"), dtype=LD)[:, None, None], np.asarray(get("ub"), dtype=LD)[:, None, None]
    Ub = gr._time_major(np.where(side < 0, lb, np.where(side > 0, ub, LD(0))))
    Ff = gr._time_major(side == 0)
    U = Ub.copy()
    for b in range(Bsz):
        F, Ac = np.flatnonzero(Ff[b]), np.flatnonzero(~Ff[b])
        if F.size:
            rhs = g[b][F] + H[b][np.ix_(F, Ac)] @ Ub[b, Ac]
            U[b, F] = -ex.chol_solve(ex.cholesky(H[b][np.ix_(F, F)])[None], rhs[None])[0]
    return np.einsum("kb,bk->b", np.asarray(w, dtype=LD), U[:, :nu]) + np.asarray(gam, dtype=LD) * ex.value(H, g, c, U)


def adjoint(N, A, B, Q, R, P, side, X, U, w, gam, x_ref=None, u_ref=None, dtype=np.float64, chol=False, stats=None):
    """numpy, the algebra of lqmpc_cost_grad_kernel: side (nu, N, Bsz) the face, X (nx, N + 1, Bsz) and U (nu, N, Bsz) the plan,
    w (nu, Bsz), gam (Bsz,).  Returns the seven outputs of KEYS.  dtype, chol, stats: see sens_ref.stage_solver (fp64 and LU by default).
        the sweep of sens_ref.masked_sweep, keeping K_j of every stage and Re_0
        u~_0 = 1/2 f_0 Re_0^-1 f_0 w,  x~_0 = 0;  j = 0 .. N-1: u~_j = -K_j x~_j (j > 0),  x~_{j+1} = A x~_j + B u~_j
        the costates l (of X, with references) and l~ (of x~, without), r_i = 2 R d_i + B'l_{i+1}, r~_i = 2 R u~_i + B'l~_{i+1}"""
    cast = lambda a: np.asarray(a, dtype=dtype)
    Ab, Bb = np.moveaxis(cast(A), -1, 0), np.moveaxis(cast(B), -1, 0)
    Q, R, P = cast(Q), cast(R), cast(P)
    Bsz, nx, nu = Bb.shape
    free = side == 0
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
    wb, gb = cast(w).T, cast(gam)
    Xt, Ut = np.zeros((Bsz, N + 1, nx), dtype=dtype), np.zeros((Bsz, N, nu), dtype=dtype)
    Ut[:, 0] = f0 * solve((f0 * wb)[:, :, None])[:, :, 0] / 2
    for j in range(N):
        if j:
            Ut[:, j] = -np.einsum("bki,bi->bk", Ks[j], Xt[:, j])
        Xt[:, j + 1] = np.einsum("bij,bj->bi", Ab, Xt[:, j]) + np.einsum("bik,bk->bi", Bb, Ut[:, j])
    xr, ur = _refs(dict(x_ref=x_ref, u_ref=u_ref), nx, nu, N, dtype)
    Xb, Ub = np.moveaxis(cast(X), -1, 0).transpose(0, 2, 1), np.moveaxis(cast(U), -1, 0).transpose(0, 2, 1)
    lam = gr._costates(N, Ab, Q, P, Xb, xr)
    lamt = gr._costates(N, Ab, Q, P, Xt, np.zeros((N, nx), dtype=dtype))
    r = np.stack([2 * np.einsum("kl,bl->bk", R, Ub[:, i] - ur[i]) + np.einsum("bmk,bm->bk", Bb, lam[i + 1]) for i in range(N)], axis=1)
    rt = np.stack([2 * np.einsum("kl,bl->bk", R, Ut[:, i]) + np.einsum("bmk,bm->bk", Bb, lamt[i + 1]) for i in range(N)], axis=1)
    return _sums(N, Q, R, P, Xb, Ub, Xt, Ut, xr, ur, r, rt, np.moveaxis(side, -1, 0).transpose(0, 2, 1), wb, gb)
