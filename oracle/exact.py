"""Extended-precision reference of the box-constrained LQ MPC problem (numpy, np.longdouble; CPU only).

TEST INFRASTRUCTURE ONLY, like oracle.py.  It is an independent restatement of the problem the oracle (lqmpc_oracle.c)
solves, written from the problem statement, not from the oracle's code, in 64-bit-mantissa arithmetic (x86 long double):

    x_{i+1} = A x_i + B u_i,  i = 0..N-1
    V_N(x0) = min  x0'Q x0 + sum_{i=0}^{N-2} |x_{i+1} - xref_i|_Q^2 + |x_N - xref_{N-1}|_P^2 + sum_{i=0}^{N-1} |u_i - uref_i|_R^2
              s.t. lb <= u_i <= ub           (no 1/2; xref column i pairs with x_{i+1}; terminal P on the last predicted state)

Condensed: X = Phi x0 + Gamma U with U time-major (U[i*nu + k] = u_i[k]), cost = U'HU + 2 g'U + c.

  condense(...)     H, g, c from the model (c includes x0'Q x0, so V = U'HU + 2g'U + c)
  certify(...)      takes the active set of a candidate U (the oracle's), solves the reduced system, checks primal
                    feasibility and multiplier signs; falls back to an active-set loop in long double where the check fails
  solve(...)        certify() with the oracle's U as the candidate
  rollout(...)      the closed loop (J_T, X, U) with every step's QP from solve()
  riccati(...)      closed form of the unconstrained problem (a backward Riccati recursion with the references)
  sequence_cost(...) the cost of a given input sequence by simulating the model (no condensing)

Array layout of the public functions is the library's (instance-minor): A (nx,nx,Bsz), B (nx,nu,Bsz), x0 (nx,Bsz),
Q, R, P, lb, ub, x_ref (nx,N), u_ref (nu,N) shared.  Results are long double.
"""
import numpy as np

LD = np.longdouble


def _ld(a):
    return None if a is None else np.asarray(a, dtype=LD)


def _inst(A, B, x0=None):
    """SoA (rows, cols, Bsz) -> instance-major (Bsz, rows, cols) long double."""
    A = np.moveaxis(_ld(A), -1, 0)
    B = np.moveaxis(_ld(B), -1, 0)
    return A, B, None if x0 is None else np.moveaxis(_ld(x0), -1, 0)


# ---------------- dense long-double linear algebra (np.linalg refuses long double) ----------------
def cholesky(H):
    """Lower Cholesky factor of a stack of SPD matrices (..., m, m).  Raises on a non-positive pivot."""
    H = np.asarray(H, dtype=LD)
    m = H.shape[-1]
    L = np.zeros_like(H)
    for j in range(m):
        d = H[..., j, j] - np.sum(L[..., j, :j] ** 2, axis=-1)
        if np.any(~(d > 0)):
            raise np.linalg.LinAlgError("matrix is not positive definite")
        d = np.sqrt(d)
        L[..., j, j] = d
        if j + 1 < m:
            s = H[..., j + 1:, j] - np.einsum("...ik,...k->...i", L[..., j + 1:, :j], L[..., j, :j])
            L[..., j + 1:, j] = s / d[..., None]
    return L


def chol_solve(L, b):
    """Solve (L L') x = b for a stack of factors (..., m, m) and right-hand sides (..., m)."""
    L = np.asarray(L, dtype=LD)
    y = np.array(b, dtype=LD)
    m = L.shape[-1]
    for i in range(m):
        y[..., i] = (y[..., i] - np.einsum("...k,...k->...", L[..., i, :i], y[..., :i])) / L[..., i, i]
    for i in range(m - 1, -1, -1):
        y[..., i] = (y[..., i] - np.einsum("...k,...k->...", L[..., i + 1:, i], y[..., i + 1:])) / L[..., i, i]
    return y


def spd_solve(H, b):
    return chol_solve(cholesky(H), b)


# ---------------- condensing ----------------
def prediction(N, A, B):
    """Phi (Bsz, N*nx, nx) and Gamma (Bsz, N*nx, N*nu) of X = Phi x0 + Gamma U, block row r predicting x_{r+1}."""
    Bsz, nx, nu = B.shape
    Phi = np.zeros((Bsz, N * nx, nx), dtype=LD)
    Gam = np.zeros((Bsz, N * nx, N * nu), dtype=LD)
    Ak = np.broadcast_to(np.eye(nx, dtype=LD), (Bsz, nx, nx))
    M = [B]                                       # M[k] = A^k B
    for k in range(1, N):
        M.append(A @ M[-1])
    for r in range(N):
        Ak = A @ Ak
        Phi[:, r * nx:(r + 1) * nx] = Ak
        for c in range(r + 1):
            Gam[:, r * nx:(r + 1) * nx, c * nu:(c + 1) * nu] = M[r - c]
    return Phi, Gam


def condense(N, A, B, Q, R, P, x0, x_ref=None, u_ref=None):
    """Condensed QP of every instance: H (Bsz,n,n), g (Bsz,n), c (Bsz,) with V(U) = U'HU + 2g'U + c (c holds x0'Q x0)."""
    A, B, x0 = _inst(A, B, x0)
    Q, R, P = _ld(Q), _ld(R), _ld(P)
    Bsz, nx, nu = B.shape
    n = N * nu
    Phi, Gam = prediction(N, A, B)
    Qs = [Q] * (N - 1) + [P]                                            # weights of x_1 .. x_N: terminal P on x_N
    X0 = np.einsum("bij,bj->bi", Phi, x0)                               # free response x_1..x_N
    if x_ref is not None:
        X0 = X0 - _ld(x_ref).T.reshape(1, N * nx)                       # column i pairs with x_{i+1}
    H = np.zeros((Bsz, n, n), dtype=LD)
    g = np.zeros((Bsz, n), dtype=LD)
    c = np.einsum("bi,ij,bj->b", x0, Q, x0)                             # + x0'Q x0
    for r in range(N):
        Gr = Gam[:, r * nx:(r + 1) * nx]                                 # (Bsz, nx, n)
        QG = np.einsum("ij,bjk->bik", Qs[r], Gr)
        H += np.einsum("bji,bjk->bik", Gr, QG)
        d = X0[:, r * nx:(r + 1) * nx]
        g += np.einsum("bji,bj->bi", QG, d)
        c += np.einsum("bi,ij,bj->b", d, Qs[r], d)
    for i in range(N):
        H[:, i * nu:(i + 1) * nu, i * nu:(i + 1) * nu] += R
    if u_ref is not None:
        ur = _ld(u_ref)
        for i in range(N):
            g[:, i * nu:(i + 1) * nu] -= (R @ ur[:, i])[None, :]
            c += ur[:, i] @ R @ ur[:, i]
    return H, g, c


def value(H, g, c, U):
    """U'HU + 2g'U + c; U (Bsz, n) time-major."""
    U = _ld(U)
    return np.einsum("bi,bij,bj->b", U, H, U) + 2 * np.einsum("bi,bi->b", g, U) + c


# ---------------- the box QP in long double ----------------
def _tol(H, g, u):
    return LD(1e-13) * (np.max(np.abs(H)) * max(np.max(np.abs(u)), LD(1)) + np.max(np.abs(g)) + LD(1e-300))


def _kkt_ok(H, g, lb, ub, u, st):
    """Primal feasibility and multiplier signs of u on the working set st (-1 lower, 0 free, +1 upper)."""
    w = ub - lb
    ftol = LD(1e-15) * np.maximum(np.maximum(np.abs(lb), np.abs(ub)), w)
    F = st == 0
    if np.any(u[F] < lb[F] - ftol[F]) or np.any(u[F] > ub[F] + ftol[F]):
        return False
    grad = H @ u + g
    t = _tol(H, g, u)
    return bool(np.all(grad[st < 0] >= -t) and np.all(grad[st > 0] <= t))


def _face_min(H, g, u, st):
    """Minimiser over the free coordinates with the others fixed at u."""
    F, A_ = st == 0, st != 0
    rhs = -g[F] - H[np.ix_(F, A_)] @ u[A_]
    return spd_solve(H[np.ix_(F, F)][None], rhs[None])[0]


def boxqp(H, g, lb, ub, u_start=None, st=None):
    """argmin u'Hu + 2g'u on lb <= u <= ub, one instance, long double, by a primal active-set loop.  Starts from the working set
    st with u_start clipped (default: the clipped unconstrained minimiser).  Returns (u, iterations)."""
    H, g, lb, ub = _ld(H), _ld(g), _ld(lb), _ld(ub)
    n = g.size
    if u_start is None:
        u = spd_solve(H[None], -g[None])[0]
        st = np.where(u <= lb, -1, np.where(u >= ub, 1, 0))
    else:
        u = _ld(u_start).copy()
        st = np.array(st)
    u = np.clip(u, lb, ub)
    u[st < 0], u[st > 0] = lb[st < 0], ub[st > 0]
    for it in range(1, 20 * n + 50):
        F = np.flatnonzero(st == 0)
        if F.size:
            uf = _face_min(H, g, u, st)
            p = uf - u[F]
            alpha, blk, side = LD(1), -1, 0
            for a, i in enumerate(F):
                if p[a] < 0 and uf[a] < lb[i]:
                    t = (lb[i] - u[i]) / p[a]
                    if t < alpha:
                        alpha, blk, side = t, i, -1
                if p[a] > 0 and uf[a] > ub[i]:
                    t = (ub[i] - u[i]) / p[a]
                    if t < alpha:
                        alpha, blk, side = t, i, 1
            if blk >= 0:
                u[F] += alpha * p
                u[blk] = lb[blk] if side < 0 else ub[blk]
                st[blk] = side
                continue
            u[F] = uf
        grad = H @ u + g
        viol = np.where(st < 0, -grad, np.where(st > 0, grad, -np.inf))
        k = int(np.argmax(viol))
        if not viol[k] > _tol(H, g, u):
            return u, it
        st[k] = 0
    raise RuntimeError("long-double active set did not terminate")


def certify_qp(H, g, lb, ub, u_cand):
    """One instance: the active set of u_cand (at a bound to within 1e-9 of the box width and 1e-15 of the bound's size), the
    reduced system solved in long
    double, then primal feasibility and multiplier signs checked.  Returns (u*, certified) -- certified is False where the
    candidate's active set was wrong and the long-double active-set loop had to finish the job."""
    H, g, lb, ub = _ld(H), _ld(g), _ld(lb), _ld(ub)
    uc = _ld(u_cand)
    w = ub - lb
    al = np.minimum(LD(1e-9) * w, LD(1e-15) * np.maximum(np.abs(lb), 1))
    au = np.minimum(LD(1e-9) * w, LD(1e-15) * np.maximum(np.abs(ub), 1))
    st = np.where(uc <= lb + al, -1, np.where(uc >= ub - au, 1, 0))
    u = np.where(st < 0, lb, np.where(st > 0, ub, uc))
    if np.any(st == 0):
        u[st == 0] = _face_min(H, g, u, st)
    if _kkt_ok(H, g, lb, ub, u, st):
        return u, True
    u, _ = boxqp(H, g, lb, ub, uc, st)
    return u, False


def _box(lb, ub, N):
    return np.tile(_ld(lb), N), np.tile(_ld(ub), N)


def certify(N, A, B, Q, R, P, lb, ub, x0, U_candidate, x_ref=None, u_ref=None):
    """Every instance of a batch: U_candidate (nu, N, Bsz) -> {'V': (Bsz,), 'U': (nu, N, Bsz), 'u_0': (nu, Bsz), 'ok': (Bsz,) bool}.
    ok = the candidate's active set passed the certificate as it was."""
    H, g, c = condense(N, A, B, Q, R, P, x0, x_ref, u_ref)
    Bsz, n = g.shape
    nu = n // N
    LB, UB = _box(lb, ub, N)
    Uc = np.moveaxis(np.asarray(U_candidate, dtype=np.float64), -1, 0).transpose(0, 2, 1).reshape(Bsz, n)
    U = np.zeros((Bsz, n), dtype=LD)
    ok = np.zeros(Bsz, dtype=bool)
    for b in range(Bsz):
        U[b], ok[b] = certify_qp(H[b], g[b], LB, UB, Uc[b])
    V = value(H, g, c, U)
    Uo = U.reshape(Bsz, N, nu).transpose(2, 1, 0)
    return {"V": V, "U": Uo, "u_0": Uo[:, 0, :].copy(), "ok": ok}


def _oracle_U(N, A, B, Q, R, P, lb, ub, x0, x_ref, u_ref):
    from . import oracle as orc
    Bsz = x0.shape[1]
    U = np.zeros((B.shape[1], N, Bsz))
    for b in range(Bsz):
        U[:, :, b] = orc.solve(N, A[:, :, b], B[:, :, b], Q, R, P, lb, ub, x0[:, b], x_ref, u_ref)["U"]
    return U


def solve(N, A, B, Q, R, P, lb, ub, x0, x_ref=None, u_ref=None):
    """certify() with the oracle's optimal U as the candidate."""
    A, B, x0 = (np.ascontiguousarray(a, dtype=np.float64) for a in (A, B, x0))
    Uc = _oracle_U(N, A, B, Q, R, P, lb, ub, x0, x_ref, u_ref)
    return certify(N, A, B, Q, R, P, lb, ub, x0, Uc, x_ref, u_ref)


def max_vn(N, A, B, Q, R, P, lb, ub, x0s, x_ref=None, u_ref=None):
    """M_V (Bsz,) = max over the K shared initial states x0s (nx, K) of V_N."""
    Bsz, K = A.shape[2], x0s.shape[1]
    best = np.full(Bsz, -np.inf, dtype=LD)
    for k in range(K):
        x0 = np.ascontiguousarray(np.repeat(np.asarray(x0s, dtype=np.float64)[:, k:k + 1], Bsz, axis=1))
        best = np.maximum(best, solve(N, A, B, Q, R, P, lb, ub, x0, x_ref, u_ref)["V"])
    return best


def rollout(T, N, A, B, Q, R, P, lb, ub, x0, A_true, B_true, x_ref=None, u_ref=None):
    """The closed loop: T steps of u_t = first input of the N-stage QP at x_t (model A, B), x_{t+1} = A_true x_t + B_true u_t;
    J_T = x0'Q x0 + sum_t (x_{t+1}'Q x_{t+1} + u_t'R u_t).  A_true, B_true shared (2-D) or per instance (3-D).
    Returns {'J_T', 'X' (nx,T+1,Bsz), 'U' (nu,T,Bsz), 'ok' (Bsz,) all certificates passed as given}."""
    nx, nu, Bsz = np.shape(B)
    Ql, Rl = _ld(Q), _ld(R)
    At, Bt = _ld(A_true), _ld(B_true)
    if At.ndim == 2:
        At, Bt = np.broadcast_to(At[:, :, None], (nx, nx, Bsz)), np.broadcast_to(Bt[:, :, None], (nx, nu, Bsz))
    At, Bt = np.moveaxis(At, -1, 0), np.moveaxis(Bt, -1, 0)
    x = np.moveaxis(_ld(x0), -1, 0).copy()
    X = np.zeros((Bsz, nx, T + 1), dtype=LD)
    U = np.zeros((Bsz, nu, T), dtype=LD)
    ok = np.ones(Bsz, dtype=bool)
    J = np.einsum("bi,ij,bj->b", x, Ql, x)
    X[:, :, 0] = x
    for t in range(T):
        # the QP at the long-double state: its candidate comes from the oracle at the rounded state, certified at the exact one
        xd = np.ascontiguousarray(x.T.astype(np.float64))
        Uc = _oracle_U(N, A, B, Q, R, P, lb, ub, xd, x_ref, u_ref)
        s = certify(N, A, B, Q, R, P, lb, ub, x.T, Uc, x_ref, u_ref)
        u = s["u_0"].T
        ok &= s["ok"]
        x = np.einsum("bij,bj->bi", At, x) + np.einsum("bij,bj->bi", Bt, u)
        J += np.einsum("bi,ij,bj->b", x, Ql, x) + np.einsum("bi,ij,bj->b", u, Rl, u)
        X[:, :, t + 1], U[:, :, t] = x, u
    return {"J_T": J, "X": np.moveaxis(X, 0, -1), "U": np.moveaxis(U, 0, -1), "ok": ok}


# ---------------- closed forms ----------------
def riccati(N, A, B, Q, R, P, x0, x_ref=None, u_ref=None):
    """The unconstrained problem (a box that is never active) by dynamic programming, long double.  The cost-to-go from x_k is
    x'S_k x + 2 s_k'x + q_k; the state term of x_k (k >= 1) is |x_k - xref_{k-1}|^2 with Q (P for k = N).
    Returns {'V': (Bsz,) including x0'Q x0, 'U': (nu, N, Bsz), 'u_0'}."""
    A, B, x0 = _inst(A, B, x0)
    Q, R, P = _ld(Q), _ld(R), _ld(P)
    Bsz, nx, nu = B.shape
    xr = np.zeros((nx, N), dtype=LD) if x_ref is None else _ld(x_ref)
    ur = np.zeros((nu, N), dtype=LD) if u_ref is None else _ld(u_ref)
    S = np.broadcast_to(P, (Bsz, nx, nx)).copy()
    s = np.broadcast_to(-(P @ xr[:, N - 1]), (Bsz, nx)).copy()
    q = np.full(Bsz, xr[:, N - 1] @ P @ xr[:, N - 1], dtype=LD)
    Ks, ks = [None] * N, [None] * N
    for k in range(N - 1, -1, -1):
        # min_u |u - ur_k|_R^2 + V_{k+1}(A x + B u):  (R + B'SB) u = R ur_k - B'S A x - B's
        BtS = np.einsum("bji,bjk->bik", B, S)
        Hk = R + BtS @ B
        L = cholesky(Hk)
        Kx = chol_solve(L[:, None], np.moveaxis(BtS @ A, -1, 1))            # (Bsz, nx, nu): columns of H^{-1} B'SA
        Kx = np.moveaxis(Kx, 1, -1)                                          # u = -Kx x + kk
        kk = chol_solve(L, (R @ ur[:, k])[None, :] - np.einsum("bji,bj->bi", B, s))
        Ks[k], ks[k] = Kx, kk
        # V_k(x) = |u|_R.. + V_{k+1}(Acl x + B kk) with u = -Kx x + kk (substituted exactly)
        Acl = A - B @ Kx
        c0 = np.einsum("bij,bj->bi", B, kk)
        du = -Kx                                                             # u = du x + kk
        Sn = np.einsum("bji,jk,bkl->bil", du, R, du) + np.einsum("bji,bjk,bkl->bil", Acl, S, Acl)
        sn = (np.einsum("bji,jk,bk->bi", du, R, kk - ur[:, k][None]) + np.einsum("bji,bjk,bk->bi", Acl, S, c0)
              + np.einsum("bji,bj->bi", Acl, s))
        qn = (np.einsum("bi,ij,bj->b", kk - ur[:, k][None], R, kk - ur[:, k][None]) + np.einsum("bi,bij,bj->b", c0, S, c0)
              + 2 * np.einsum("bi,bi->b", s, c0) + q)
        if k >= 1:                                                            # + |x_k - xref_{k-1}|_Q^2
            Sn = Sn + Q
            sn = sn - (Q @ xr[:, k - 1])[None]
            qn = qn + xr[:, k - 1] @ Q @ xr[:, k - 1]
        S, s, q = Sn, sn, qn
    V = np.einsum("bi,bij,bj->b", x0, S, x0) + 2 * np.einsum("bi,bi->b", s, x0) + q + np.einsum("bi,ij,bj->b", x0, Q, x0)
    x, U = x0.copy(), np.zeros((Bsz, nu, N), dtype=LD)
    for k in range(N):
        u = -np.einsum("bij,bj->bi", Ks[k], x) + ks[k]
        U[:, :, k] = u
        x = np.einsum("bij,bj->bi", A, x) + np.einsum("bij,bj->bi", B, u)
    Uo = np.moveaxis(U, 0, -1)
    return {"V": V, "U": Uo, "u_0": Uo[:, 0, :].copy()}


def sequence_cost(N, A, B, Q, R, P, x0, U, x_ref=None, u_ref=None):
    """V of a given input sequence U (nu, N, Bsz) by simulating the model, long double (a pinned input: every u_i on one bound).
    Includes x0'Q x0."""
    A, B, x0 = _inst(A, B, x0)
    Q, R, P = _ld(Q), _ld(R), _ld(P)
    Bsz, nx, nu = B.shape
    U = np.moveaxis(_ld(U), -1, 0)
    xr = np.zeros((nx, N), dtype=LD) if x_ref is None else _ld(x_ref)
    ur = np.zeros((nu, N), dtype=LD) if u_ref is None else _ld(u_ref)
    x = x0.copy()
    V = np.einsum("bi,ij,bj->b", x, Q, x)
    for i in range(N):
        u = U[:, :, i]
        x = np.einsum("bij,bj->bi", A, x) + np.einsum("bij,bj->bi", B, u)
        W = P if i == N - 1 else Q
        d, e = x - xr[:, i][None], u - ur[:, i][None]
        V += np.einsum("bi,ij,bj->b", d, W, d) + np.einsum("bi,ij,bj->b", e, R, e)
    return V
