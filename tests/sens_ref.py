"""Shared by tests/test_sens_cpu.py, tests/test_gpu_sens.py and tests/test_gpu_torch_layer.py (not a test module).

  problem(), case()   the problems of tests/test_gpu_plan.py (copied): spectral radius of A in [0.5, 1], dense SPD weights of condition
                      10, x0 scales {0.01, 0.3, 3}, a symmetric random box; with refs non-zero references and that file's off-centre box
  reference()         the long-double derivatives of a plan from oracle/exact.py: on the face F of the plan (the free entries),
                      Kplan[F] = -H_FF^-1 Fx[F] with Fx[:, a] = g(e_a) - g(0) (g is affine in x0), zero on the active rows;
                      dVdx = the central difference with step 1 of value(H, g(x), c(x), U*) at fixed U* (exact: V is quadratic in x)
  masked_sweep(), costate()
                      an fp64 numpy restatement of what lqmpc_sens_kernel computes: one backward Riccati sweep with a free mask per
                      stage and one forward product; one costate recursion over the predicted states.  With dtype = long double
                      the same operation as a reference (tests/postpass_hard.py)
  chol_factor(), chol_apply(), stage_solver()
                      how a stage matrix Re is solved with: numpy.linalg.solve by default (what the restatements have always
                      used, bit for bit), the kernels' own Cholesky on request, oracle/exact.py's in long double
"""
import numpy as np

from oracle import exact as ex
from oracle import oracle as orc

LD = np.longdouble
BSZ = 203


def problem(nx, nu, N, Bsz, seed, lb, ub, x_scale=1.0):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((nx, nx, Bsz))
    A *= rng.uniform(0.5, 1.0, Bsz) / np.abs(np.linalg.eigvals(A.transpose(2, 0, 1))).max(axis=1)
    B = rng.standard_normal((nx, nu, Bsz)) * rng.uniform(0.3, 1.0, (1, 1, Bsz))

    def spd(m, c):
        q, _ = np.linalg.qr(rng.standard_normal((m, m)))
        return (q * np.geomspace(1.0, c, m)) @ q.T
    Q, R, P = spd(nx, 10.0), spd(nu, 10.0), 3.0 * spd(nx, 10.0)
    # free, partly saturated and fully saturated initial states
    x0 = rng.standard_normal((nx, Bsz)) * x_scale * rng.choice([0.01, 0.3, 3.0], Bsz)
    return dict(N=N, A=np.ascontiguousarray(A), B=np.ascontiguousarray(B), Q=Q, R=R, P=P,
                lb=np.asarray(lb, dtype=float), ub=np.asarray(ub, dtype=float), x0=np.ascontiguousarray(x0))


def qa(p):
    return (p["N"], p["A"], p["B"], p["Q"], p["R"], p["P"], p["lb"], p["ub"])


def model(p):
    return (p["N"], p["A"], p["B"], p["Q"], p["R"], p["P"])


def oracle_plan(p, x0, kw):
    """the fp64 oracle's whole plan, (nu, N, Bsz)"""
    nu, Bsz = p["B"].shape[1], x0.shape[1]
    U = np.zeros((nu, p["N"], Bsz))
    for b in range(Bsz):
        U[:, :, b] = orc.solve(p["N"], p["A"][:, :, b], p["B"][:, :, b], p["Q"], p["R"], p["P"], p["lb"], p["ub"], x0[:, b],
                               kw.get("x_ref"), kw.get("u_ref"))["U"]
    return U


def model_roll(p, x0, U):
    """x_0 = x0, x_{i+1} = A x_i + B u_i in fp64: (nx, N + 1, Bsz)"""
    nx, Bsz = x0.shape
    X = np.zeros((nx, p["N"] + 1, Bsz))
    X[:, 0] = x0
    for i in range(p["N"]):
        X[:, i + 1] = np.einsum("acb,cb->ab", p["A"], X[:, i]) + np.einsum("akb,kb->ab", p["B"], U[:, i])
    return X


# ---------------- the problem of a shape and the oracle's plan, computed once and never changed ----------------
_CASES = {}


def case(shape, refs=False, off_centre=False, bsz=BSZ):
    key = (shape, refs, off_centre, bsz)
    if key in _CASES:
        return _CASES[key]
    nx, nu, N = shape
    rng = np.random.default_rng(sum(shape) + 100 * refs)
    lb, ub = -rng.uniform(0.1, 0.4, nu), rng.uniform(0.1, 0.4, nu)
    if not off_centre:
        lb = -ub                                                  # a symmetric random box: centre 0, half-width ub, both exact
    kw = {}
    if refs:
        if off_centre:
            lb, ub = lb + 0.3, ub + 0.45                          # centres in (0.3, 0.5), as tests/test_gpu_wide_state.py
        kw = dict(x_ref=0.05 * rng.standard_normal((nx, N)), u_ref=0.05 * rng.standard_normal((nu, N)))
    p = problem(nx, nu, N, bsz, 17 * nx + N, lb, ub)
    c = dict(shape=shape, p=p, kw=kw, h=0.5 * (ub - lb), U=oracle_plan(p, p["x0"], kw))
    for a in (p["A"], p["B"], p["x0"], c["U"]):
        a.setflags(write=False)
    _CASES[key] = c
    return c


# ---------------- the long-double reference ----------------
def face_of(U_exact, lb, ub):
    """free mask (nu, N, Bsz) of a plan from exact.certify: an entry is on a bound when it IS the bound (certify puts it there)"""
    lo, hi = np.asarray(lb, dtype=LD)[:, None, None], np.asarray(ub, dtype=LD)[:, None, None]
    return ~((U_exact == lo) | (U_exact == hi))


def reference(p, kw, x0, U_plan):
    """Long-double derivatives on the face of U_plan (nu, N, Bsz): {'K_plan' (nu, N, nx, Bsz), 'dV_dx' (nx, Bsz), 'free' (nu, N, Bsz)
    bool, 'U' the exact optimum on that face, 'ok' the certificate of U_plan's active set}."""
    N, nu, nx, Bsz = p["N"], p["B"].shape[1], p["A"].shape[0], x0.shape[1]
    n = N * nu
    xr, ur = kw.get("x_ref"), kw.get("u_ref")
    cert = ex.certify(*qa(p), x0, U_plan, xr, ur)
    free = face_of(cert["U"], p["lb"], p["ub"])
    Us = np.moveaxis(cert["U"], -1, 0).transpose(0, 2, 1).reshape(Bsz, n)              # time-major, as condense
    Ffree = np.moveaxis(free, -1, 0).transpose(0, 2, 1).reshape(Bsz, n)

    H, g_x0, c_x0 = ex.condense(*model(p), x0, xr, ur)
    # g(x) and c(x) of exact.condense at other states, from the prediction matrices built once (3 nx + 1 states are needed, and
    # condense rebuilds Phi, Gamma and H at every call): the same sums in the same order, checked against condense at x0 below
    Al, Bl = np.moveaxis(np.asarray(p["A"], dtype=LD), -1, 0), np.moveaxis(np.asarray(p["B"], dtype=LD), -1, 0)
    Phi, Gam = ex.prediction(N, Al, Bl)
    Ql, Rl = np.asarray(p["Q"], dtype=LD), np.asarray(p["R"], dtype=LD)
    Qs = [Ql] * (N - 1) + [np.asarray(p["P"], dtype=LD)]
    QG = [np.einsum("ij,bjk->bik", Qs[r], Gam[:, r * nx:(r + 1) * nx]) for r in range(N)]
    xrl = None if xr is None else np.asarray(xr, dtype=LD).T.reshape(1, N * nx)
    url = None if ur is None else np.asarray(ur, dtype=LD)

    def cond(x):
        x = np.moveaxis(np.asarray(x, dtype=LD), -1, 0)
        X0 = np.einsum("bij,bj->bi", Phi, x)
        if xrl is not None:
            X0 = X0 - xrl
        g = np.zeros((Bsz, n), dtype=LD)
        c = np.einsum("bi,ij,bj->b", x, Ql, x)
        for r in range(N):
            d = X0[:, r * nx:(r + 1) * nx]
            g += np.einsum("bji,bj->bi", QG[r], d)
            c += np.einsum("bi,ij,bj->b", d, Qs[r], d)
        if url is not None:
            for i in range(N):
                g[:, i * nu:(i + 1) * nu] -= (Rl @ url[:, i])[None, :]
                c += url[:, i] @ Rl @ url[:, i]
        return g, c
    g_chk, c_chk = cond(x0)
    assert np.max(np.abs(g_chk - g_x0)) <= 1e-17 * max(np.max(np.abs(g_x0)), 1) and np.max(np.abs(c_chk - c_x0)) <= 1e-17 * np.max(np.abs(c_x0))
    g0 = cond(np.zeros((nx, Bsz)))[0]
    Fx = np.zeros((Bsz, n, nx), dtype=LD)
    dV = np.zeros((nx, Bsz), dtype=LD)
    x0l = np.asarray(x0, dtype=LD)
    for a in range(nx):
        e = np.zeros((nx, Bsz), dtype=LD)
        e[a] = 1
        Fx[:, :, a] = cond(e)[0] - g0
        dV[a] = (ex.value(H, *cond(x0l + e), Us) - ex.value(H, *cond(x0l - e), Us)) / 2
    K = gain_on_face(H, Fx, Ffree)
    return dict(K_plan=K.reshape(Bsz, N, nu, nx).transpose(2, 1, 3, 0), dV_dx=dV, free=free, U=cert["U"], ok=cert["ok"])


def gain_on_face(H, Fx, Ffree):
    """(Bsz, n, nx) long double: K[F] = -H_FF^-1 Fx[F] on the face Ffree (Bsz, n) bool, time-major as exact.condense; zero elsewhere.
    It depends on the face alone, not on the plan that has it."""
    K = np.zeros(Fx.shape, dtype=LD)
    for b in range(Fx.shape[0]):
        F = np.flatnonzero(Ffree[b])
        if F.size:
            L = ex.cholesky(H[b][np.ix_(F, F)])
            K[b, F, :] = -ex.chol_solve(L[None], Fx[b, F, :].T).T
    return K


def oracle_face(p, kw, x0, U_oracle):
    """free mask of the oracle's own plan, certified in long double"""
    return face_of(ex.certify(*qa(p), x0, U_oracle, kw.get("x_ref"), kw.get("u_ref"))["U"], p["lb"], p["ub"])


def riccati_gain(p, idx):
    """the first gain of the unconstrained problem for the instances idx, (nu, nx, len(idx)) long double: exact.riccati's u_0 is
    affine in x0, so column a is u_0(e_a) - u_0(0)"""
    nx = p["A"].shape[0]
    A, B = np.ascontiguousarray(p["A"][:, :, idx]), np.ascontiguousarray(p["B"][:, :, idx])
    u = lambda x: ex.riccati(p["N"], A, B, p["Q"], p["R"], p["P"], x)["u_0"]
    u_zero = u(np.zeros((nx, len(idx))))
    cols = []
    for a in range(nx):
        e = np.zeros((nx, len(idx)))
        e[a] = 1.0
        cols.append(u(e) - u_zero)
    return np.stack(cols, axis=1)


def rel_err(got, ref, axes):
    """per instance: max |got - ref| / max(|ref|_max, 1), the maxima over `axes` (the instance axis is last)"""
    got, ref = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD)
    return np.asarray(np.max(np.abs(got - ref), axis=axes) / np.maximum(np.max(np.abs(ref), axis=axes), 1), dtype=np.float64)


# ---------------- numpy restatement of the kernel's algebra: fp64, or long double as a reference of the same operation ----------------
def face_bits(U, lb, ub):
    """free mask of an fp64 plan by the rule of include/lqmpc.h: an entry is on a bound when it equals, bit for bit, lb, ub,
    c - h or c + h with c = (ub + lb) / 2, h = (ub - lb) / 2"""
    lb, ub = np.asarray(lb, dtype=np.float64)[:, None, None], np.asarray(ub, dtype=np.float64)[:, None, None]
    c, h = 0.5 * (ub + lb), 0.5 * (ub - lb)
    return ~((U == lb) | (U == ub) | (U == c - h) | (U == c + h))


def chol_factor(Re, stats=None):
    """The factor the post-pass kernels form of a stack of stage matrices Re (Bsz, m, m), in Re's own dtype: Cholesky column by column
    from the LOWER triangle (the upper one is never read), (L, Di) with L below the diagonal and Di the reciprocals of the factor's
    diagonal.  A pivot that is not positive gives NaN, as in the kernels.  stats, a dict: 'pivot' takes the smallest pivot relative to
    its diagonal entry, 'positive' whether every pivot was positive."""
    m = Re.shape[-1]
    L, Di = np.zeros_like(Re), np.zeros(Re.shape[:-1], dtype=Re.dtype)
    for q in range(m):
        dq = Re[:, q, q] - np.sum(L[:, q, :q] * L[:, q, :q], axis=-1)
        if stats is not None:
            stats["pivot"] = min(stats.get("pivot", np.inf), float(np.min(dq / Re[:, q, q])))
            stats["positive"] = stats.get("positive", True) and bool(np.all(dq > 0))
        with np.errstate(invalid="ignore", divide="ignore"):
            Di[:, q] = 1 / np.sqrt(dq)
        L[:, q + 1:, q] = (Re[:, q + 1:, q] - np.einsum("bik,bk->bi", L[:, q + 1:, :q], L[:, q, :q])) * Di[:, q, None]
    return L, Di


def chol_apply(L, Di, G):
    """(L L')^-1 G for right-hand sides G (Bsz, m, c): the two substitutions of the kernels, multiplying by the reciprocal diagonal"""
    Y = np.array(G)
    m = L.shape[-1]
    for k in range(m):
        Y[:, k] = (Y[:, k] - np.einsum("bm,bmc->bc", L[:, k, :k], Y[:, :k])) * Di[:, k, None]
    for k in range(m - 1, -1, -1):
        Y[:, k] = (Y[:, k] - np.einsum("bm,bmc->bc", L[:, k + 1:, k], Y[:, k + 1:])) * Di[:, k, None]
    return Y


def stage_solver(Re, dtype=np.float64, chol=False, stats=None):
    """G (Bsz, m, c) -> Re^-1 G.  The default is numpy.linalg.solve (LU), what the restatements have always used; chol = True factors
    as the kernels do (chol_factor, chol_apply); long double goes through exact.cholesky / exact.chol_solve, numpy.linalg having no
    long double."""
    if np.dtype(dtype) == np.dtype(LD) and np.dtype(LD) != np.dtype(np.float64):
        L = ex.cholesky(Re)
        return lambda G: np.swapaxes(ex.chol_solve(L[:, None], np.swapaxes(G, 1, 2)), 1, 2)
    if chol:
        L, Di = chol_factor(Re, stats)
        return lambda G: chol_apply(L, Di, G)
    return lambda G: np.linalg.solve(Re, G)


def masked_sweep(N, A, B, Q, R, P, free, dtype=np.float64, chol=False, stats=None):
    """K_plan (nu, N, nx, Bsz) = d u_i / d x0 on the face `free` (nu, N, Bsz):
        B_j = B diag(f_j), R_j = diag(f_j) R diag(f_j) + diag(1 - f_j)
        S = P; j = N-1..0: Re = R_j + B_j'S B_j, K_j = Re^-1 B_j'S A, Acl_j = A - B_j K_j, S <- Q + A'S Acl_j
        Pi_0 = I; j = 0..N-1: du_j/dx0 = -K_j Pi_j, Pi_{j+1} = Acl_j Pi_j
    dtype, chol, stats: see stage_solver; rows of fixed inputs are exact zeros either way"""
    Ab, Bb = np.moveaxis(np.asarray(A, dtype=dtype), -1, 0), np.moveaxis(np.asarray(B, dtype=dtype), -1, 0)
    Q, R, P = (np.asarray(M, dtype=dtype) for M in (Q, R, P))
    Bsz, nx, nu = Bb.shape
    S = np.broadcast_to(P, (Bsz, nx, nx)).copy()
    Ks, Acl = [None] * N, [None] * N
    eye = np.eye(nu, dtype=dtype)
    for j in range(N - 1, -1, -1):
        f = free[:, j, :].T.astype(dtype)                                               # (Bsz, nu)
        Bj = Bb * f[:, None, :]
        Rj = f[:, :, None] * R[None] * f[:, None, :] + eye[None] * (1 - f)[:, :, None]
        BtS = np.einsum("bji,bjk->bik", Bj, S)
        Ks[j] = stage_solver(Rj + BtS @ Bj, dtype, chol, stats)(BtS @ Ab)
        Acl[j] = Ab - Bj @ Ks[j]
        S = Q[None] + np.einsum("bji,bjk->bik", Ab, S @ Acl[j])
    Pi = np.broadcast_to(np.eye(nx, dtype=dtype), (Bsz, nx, nx)).copy()
    out = np.zeros((nu, N, nx, Bsz), dtype=dtype)
    for j in range(N):
        out[:, j] = np.moveaxis(-Ks[j] @ Pi, 0, -1)
        Pi = Acl[j] @ Pi
    return out


def costate(N, A, Q, P, X, x_ref=None, dtype=np.float64):
    """dV_N/dx0 (nx, Bsz) from the predicted states X (nx, N + 1, Bsz):
        l_N = 2 P (x_N - xref_{N-1}), l_i = 2 Q (x_i - xref_{i-1}) + A'l_{i+1}, dV/dx0 = 2 Q x0 + A'l_1"""
    nx = X.shape[0]
    A, Q, P, X = (np.asarray(M, dtype=dtype) for M in (A, Q, P, X))
    xr = np.zeros((nx, N), dtype=dtype) if x_ref is None else np.asarray(x_ref, dtype=dtype)
    lam = 2 * P @ (X[:, N] - xr[:, N - 1][:, None])
    for i in range(N - 1, 0, -1):
        lam = 2 * Q @ (X[:, i] - xr[:, i - 1][:, None]) + np.einsum("mab,mb->ab", A, lam)
    return 2 * Q @ X[:, 0] + np.einsum("mab,mb->ab", A, lam)
