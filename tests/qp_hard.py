"""Shared by tests/test_qp_hard_cpu.py and tests/test_gpu_qp_hard.py (not a test module): box QPs whose condensed Hessian H or stage
matrix R_e = R + B'Sigma B is ill-conditioned, their long-double referee (oracle/exact.py) and the bars they are held to.

  problem(family, shape)   one seeded, instance-minor batch: the dict the other modules' problem() returns, plus kw (the references)
                           and h (the half-width).  Every entry of A, B, x0 and the box is a multiple of 2^-24 (x0 of near_degenerate
                           excepted: its ladder moves x0 by 1e-15 relative), so the inputs, and every condition number, are the same
                           bits on every machine.  Box +-0.3 (on the grid: 5033165 / 2^24); the cases of OFF_CENTRE use lb + 0.3, ub + 0.45 with non-zero references.
                           x0 scales {0.01, 0.3, 3}.
  families
    unstable         A random, spectral radius RUNG[shape] from LADDER; B random with |B|_2 = B_NORM; Q = 2I, R = I, P = 3I.  The rung is the highest whose largest
                     cond_2(H) stays <= CAP (asserted by the CPU module, also that the next rung breaks the cap).
    integrator       A = I + superdiagonal (one Jordan block at 1), the last two rows of B driven (random), same weights.
    redundant        R = r I, r = R_CHEAP[shape] from {1e-3, 1e-4, 1e-6} (the smallest that keeps the cap); spectral radius 1;
                     n_u <= n_x: B[:, k] = (1 + 0.1 k) B[:, 0] + 1e-2 randn, n_u > n_x: plain random B.  cond_2(R + B'PB) >= 1e4.
    near_degenerate  well-conditioned models (spectral radius in [0.5, 1], SPD weights of condition 10) and x0 = s d with
                     s = s* (1 + k), k in LADDER_K, s* the scale at which the largest |v_unc,i| / h_i of the unconstrained minimiser
                     (exact.riccati, long double) is exactly 1: instance b is model b // 11 at rung b % 11.
  cond_H(p)          cond_2 of the condensed Hessian per instance (exact.condense, numpy.linalg.cond on the fp64 copy)
  exact_solve(p), exact_roll(p), exact_steps(p)   the referee's answers, computed once per process and never changed
  bar(quantity, entry, cond)                     max(floor, c eps cond_2(H_b)), per instance

The constants C (see test_qp_hard_cpu.py, which pins them): c = 16 x the worst ratio err / (eps cond_2(H_b)) of the fp64 oracle
(oracle/lqmpc_oracle.c) against the referee over every committed case, rounded up to a power of two -- from the oracle and the referee
only, never from a GPU result."""
import zlib

import numpy as np

from oracle import exact as ex
from oracle import oracle as orc

LD = np.longdouble
EPS = 2.0 ** -52
GRID = 2.0 ** 24
CAP = 1e8
LADDER = (1.1, 1.2, 1.3, 1.45, 1.6, 2.0)
R_LADDER = (1e-6, 1e-4, 1e-3)
LADDER_K = (0.0, 1e-15, -1e-15, 1e-13, -1e-13, 1e-12, -1e-12, 1e-11, -1e-11, 1e-9, -1e-9)
T_ROLL = 5
B_NORM = 8.0          # |B|_2 of the unstable family: at N = 4 a smaller B leaves cond_2(H) of some instances under 1e3 at every rung

# shape -> (families, instances); by what the shape switches, see PATHS in tests/test_gpu_qp_hard.py
CASES = {
    (4, 2, 10): (("unstable", "integrator", "redundant", "near_degenerate"), 37),
    (2, 1, 30): (("unstable", "integrator"), 37),
    (4, 2, 20): (("unstable", "redundant"), 13),                      # (integrator: cond_2(H) 1.1e8, over the cap)
    (3, 3, 4): (("unstable", "redundant"), 37),
    (4, 4, 4): (("unstable", "redundant"), 37),
    (2, 4, 8): (("redundant",), 37),
    (7, 3, 11): (("unstable", "integrator", "near_degenerate"), 13),
    (12, 2, 10): (("unstable", "redundant"), 37),
    (8, 4, 30): (("unstable", "redundant", "near_degenerate"), 13),
    (9, 5, 7): (("unstable", "redundant"), 13),
    (16, 4, 8): (("unstable", "redundant"), 37),
    (4, 6, 5): (("unstable", "redundant"), 37),
}
CASE_LIST = [(f, s) for s, (fams, _) in CASES.items() for f in fams]
OFF_CENTRE = {("integrator", (4, 2, 10)), ("unstable", (3, 3, 4))}

# the rung of LADDER per shape (unstable) and r per shape (redundant): tests/test_qp_hard_cpu.py asserts that each is the extreme one
# that keeps cond_2(H) <= CAP
RUNG = {(4, 2, 10): 2.0, (2, 1, 30): 1.2, (4, 2, 20): 1.3, (3, 3, 4): 2.0, (4, 4, 4): 2.0, (7, 3, 11): 1.6, (12, 2, 10): 2.0,
        (8, 4, 30): 1.2, (9, 5, 7): 2.0, (16, 4, 8): 2.0, (4, 6, 5): 2.0}
R_CHEAP = {(4, 2, 10): 1e-6, (4, 2, 20): 1e-6, (3, 3, 4): 1e-4, (4, 4, 4): 1e-4, (2, 4, 8): 1e-4, (12, 2, 10): 1e-6, (8, 4, 30): 1e-3,
           (9, 5, 7): 1e-4, (16, 4, 8): 1e-6, (4, 6, 5): 1e-4}

# the largest cond_2(R + B'PB) of each redundant case (three digits; tests/test_qp_hard_cpu.py holds the generator to them): each is
# >= 1e4, so the case tests what it is for
COND_RE = {(4, 2, 10): 3.017e6, (4, 2, 20): 1.494e5, (3, 3, 4): 8.650e5, (4, 4, 4): 1.979e6, (2, 4, 8): 4.460e5, (12, 2, 10): 2.164e5,
           (8, 4, 30): 2.721e5, (9, 5, 7): 2.832e6, (16, 4, 8): 9.809e5, (4, 6, 5): 7.887e5}

# a seed that left under a quarter of the instances partly saturated was changed (the caps were not)
SEED = {("unstable", (4, 2, 10)): 2, ("integrator", (2, 1, 30)): 1, ("unstable", (7, 3, 11)): 1, ("unstable", (4, 6, 5)): 1}

# bars: max(FLOOR, C eps cond_2(H_b)).  FLOOR: what the project holds the quantity to on easy problems (tests/test_gpu_domain_edges.py)
FLOOR = dict(U=1e-10, V=1e-11, J=1e-10)
HARD_COND = 1e3       # the ratios behind C are taken over the instances with cond_2(H_b) >= this (every instance of the three hard families)
C = {
    "solve": dict(U=16.0, V=32.0),
    "step": dict(U=16.0, V=32.0),
    "rollout": dict(U=16.0, J=4.0),
}


def bar(entry, quantity, cond):
    """per instance; the states (X_plan, a rollout's X) are held to the bar of U, relative to max |X*|"""
    return np.maximum(FLOOR[quantity], C[entry][quantity] * EPS * np.asarray(cond, dtype=float))


def grid(M):
    """onto multiples of 2^-24: the same bits wherever the generator runs"""
    return np.round(np.asarray(M, float) * GRID) / GRID


def _rho(A):
    return np.max(np.abs(np.linalg.eigvals(A)))


def _rand_A(rng, nx, rho):
    A = rng.standard_normal((nx, nx))
    return grid(A * (rho / _rho(A)))


def _spd(rng, m, c):
    q, _ = np.linalg.qr(rng.standard_normal((m, m)))
    M = grid((q * np.geomspace(1.0, c, m)) @ q.T)
    return 0.5 * (M + M.T)


_PROBLEMS = {}


def problem(family, shape, rho=None, r=None):
    """rho / r: another rung than the table's (the CPU module's cap checks); such a problem is not cached"""
    key = (family, shape)
    canonical = rho is None and r is None
    if canonical and key in _PROBLEMS:
        return _PROBLEMS[key]
    nx, nu, N = shape
    Bsz = CASES[shape][1]
    rng = np.random.default_rng(zlib.crc32(f"qp-{family}-{nx}-{nu}-{N}".encode()) + SEED.get(key, 0))
    Q, R, P = 2.0 * np.eye(nx), np.eye(nu), 3.0 * np.eye(nx)
    lb, ub = np.full(nu, -0.3), np.full(nu, 0.3)
    kw = {}
    rB = lambda: grid(rng.standard_normal((nx, nu)))
    if family == "unstable":
        rho = RUNG[shape] if rho is None else rho
        models = []
        for _ in range(Bsz):
            Am, Bm = _rand_A(rng, nx, rho), rng.standard_normal((nx, nu))
            models.append((Am, grid(Bm * (B_NORM / np.linalg.norm(Bm, 2)))))
    elif family == "integrator":
        models = []
        for _ in range(Bsz):
            Bm = np.zeros((nx, nu))
            Bm[-2:, :] = grid(rng.standard_normal((min(2, nx), nu)))
            models.append((np.eye(nx) + np.diag(np.ones(nx - 1), 1), Bm))
    elif family == "redundant":
        R = (R_CHEAP[shape] if r is None else r) * np.eye(nu)
        models = []
        for _ in range(Bsz):
            Bm = rB()
            if nu <= nx:
                for k in range(1, nu):
                    Bm[:, k] = grid((1 + 0.1 * k) * Bm[:, 0] + 1e-2 * rng.standard_normal(nx))
            models.append((_rand_A(rng, nx, 1.0), Bm))
    elif family == "near_degenerate":
        Q, R, P = _spd(rng, nx, 10.0), _spd(rng, nu, 10.0), 3.0 * _spd(rng, nx, 10.0)
        distinct = [(_rand_A(rng, nx, rng.uniform(0.5, 1.0)), grid(rB() * rng.uniform(0.3, 1.0)), grid(rng.standard_normal(nx)))
                    for _ in range(-(-Bsz // len(LADDER_K)))]
        models = [distinct[b // len(LADDER_K)][:2] for b in range(Bsz)]
    else:
        raise KeyError(family)
    A = np.ascontiguousarray(np.stack([m[0] for m in models], axis=2))
    B = np.ascontiguousarray(np.stack([m[1] for m in models], axis=2))
    if family == "near_degenerate":
        d = np.stack([distinct[b // len(LADDER_K)][2] for b in range(Bsz)], axis=1)
        Uunc = ex.riccati(N, A, B, Q, R, P, d)["U"]                                       # linear in x0: no references
        s_star = 1 / np.max(np.abs(Uunc) / np.asarray(grid(ub), dtype=LD)[:, None, None], axis=(0, 1))
        k = np.array([LADDER_K[b % len(LADDER_K)] for b in range(Bsz)], dtype=LD)
        x0 = np.ascontiguousarray((np.asarray(d, dtype=LD) * (s_star * (1 + k))[None, :]).astype(np.float64))
    else:
        x0 = grid(rng.standard_normal((nx, Bsz)) * rng.choice([0.01, 0.3, 3.0], Bsz))
        if key in OFF_CENTRE and canonical:
            lb, ub = lb + 0.3, ub + 0.45
            kw = dict(x_ref=grid(0.05 * rng.standard_normal((nx, N))), u_ref=grid(0.05 * rng.standard_normal((nu, N))))
    lb, ub = grid(lb), grid(ub)
    p = dict(family=family, shape=shape, N=N, A=A, B=B, Q=Q, R=R, P=P, lb=lb, ub=ub, x0=x0, kw=kw, h=0.5 * (ub - lb), canonical=canonical)
    for a in (A, B, x0):
        a.setflags(write=False)
    if canonical:
        _PROBLEMS[key] = p
    return p


def qa(p):
    return (p["N"], p["A"], p["B"], p["Q"], p["R"], p["P"], p["lb"], p["ub"])


def refs(p):
    return p["kw"].get("x_ref"), p["kw"].get("u_ref")


_MEMO = {}


def _memo(name, p, f):
    if not p["canonical"]:
        return f()
    key = (name, p["family"], p["shape"])
    if key not in _MEMO:
        _MEMO[key] = f()
    return _MEMO[key]


class Referee:
    """oracle/exact.py's solve, certify and rollout of one problem with the prediction matrices and H condensed once: H does not
    depend on the state, and exact.condense rebuilds it at every call (four seconds at (8, 4, 30)).  g(x) and c(x) are exact.condense's
    sums in its order, as tests/sens_ref.py restates them; the QPs are exact.certify_qp's.  tests/test_qp_hard_cpu.py holds solve and
    rollout to exact.solve and exact.rollout bit for bit."""

    def __init__(self, p):
        self.p = p
        N, (nx, nu, Bsz) = p["N"], p["B"].shape
        A, B, _ = ex._inst(p["A"], p["B"])
        self.Phi, Gam = ex.prediction(N, A, B)
        self.Q, self.R = np.asarray(p["Q"], dtype=LD), np.asarray(p["R"], dtype=LD)
        self.Qs = [self.Q] * (N - 1) + [np.asarray(p["P"], dtype=LD)]
        self.QG = [np.einsum("ij,bjk->bik", self.Qs[r], Gam[:, r * nx:(r + 1) * nx]) for r in range(N)]
        H = np.zeros((Bsz, N * nu, N * nu), dtype=LD)
        for r in range(N):
            H += np.einsum("bji,bjk->bik", Gam[:, r * nx:(r + 1) * nx], self.QG[r])
        for i in range(N):
            H[:, i * nu:(i + 1) * nu, i * nu:(i + 1) * nu] += self.R
        self.H = H
        xr, ur = refs(p)
        self.xr = None if xr is None else np.asarray(xr, dtype=LD).T.reshape(1, N * nx)
        self.ur = None if ur is None else np.asarray(ur, dtype=LD)
        self.LB, self.UB = ex._box(p["lb"], p["ub"], N)

    def gc(self, x):
        """g (Bsz, n) and c (Bsz,) at the states x (nx, Bsz)"""
        p, N, (nx, nu, Bsz) = self.p, self.p["N"], self.p["B"].shape
        x = np.moveaxis(np.asarray(x, dtype=LD), -1, 0)
        X0 = np.einsum("bij,bj->bi", self.Phi, x)
        if self.xr is not None:
            X0 = X0 - self.xr
        g = np.zeros((Bsz, N * nu), dtype=LD)
        c = np.einsum("bi,ij,bj->b", x, self.Q, x)
        for r in range(N):
            d = X0[:, r * nx:(r + 1) * nx]
            g += np.einsum("bji,bj->bi", self.QG[r], d)
            c += np.einsum("bi,ij,bj->b", d, self.Qs[r], d)
        if self.ur is not None:
            for i in range(N):
                g[:, i * nu:(i + 1) * nu] -= (self.R @ self.ur[:, i])[None, :]
                c += self.ur[:, i] @ self.R @ self.ur[:, i]
        return g, c

    def certify(self, x, U_candidate):
        """exact.certify: U_candidate (nu, N, Bsz) -> {'V', 'U' (nu, N, Bsz), 'u_0', 'ok'}, and 'X' the model rolled in long double"""
        N, (nx, nu, Bsz) = self.p["N"], self.p["B"].shape
        g, c = self.gc(x)
        Uc = np.moveaxis(np.asarray(U_candidate, dtype=np.float64), -1, 0).transpose(0, 2, 1).reshape(Bsz, N * nu)
        U = np.zeros((Bsz, N * nu), dtype=LD)
        ok = np.zeros(Bsz, dtype=bool)
        for b in range(Bsz):
            U[b], ok[b] = ex.certify_qp(self.H[b], g[b], self.LB, self.UB, Uc[b])
        Uo = U.reshape(Bsz, N, nu).transpose(2, 1, 0)
        return {"V": ex.value(self.H, g, c, U), "U": Uo, "u_0": Uo[:, 0, :].copy(), "ok": ok, "X": model_roll(self.p, x, Uo)}

    def solve(self, x):
        """exact.solve: certify with the fp64 oracle's plan at the rounded state as the candidate"""
        xd = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
        return self.certify(x, oracle_plan(self.p, xd)[0])

    def rollout(self, T, A_true, B_true):
        """exact.rollout from the problem's x0 on a per-instance plant"""
        p = self.p
        At, Bt = np.moveaxis(np.asarray(A_true, dtype=LD), -1, 0), np.moveaxis(np.asarray(B_true, dtype=LD), -1, 0)
        x = np.moveaxis(np.asarray(p["x0"], dtype=LD), -1, 0).copy()
        Bsz, nx = x.shape
        X, U = np.zeros((Bsz, nx, T + 1), dtype=LD), np.zeros((Bsz, p["B"].shape[1], T), dtype=LD)
        ok = np.ones(Bsz, dtype=bool)
        J = np.einsum("bi,ij,bj->b", x, self.Q, x)
        X[:, :, 0] = x
        for t in range(T):
            s = self.solve(x.T)
            u = s["u_0"].T
            ok &= s["ok"]
            x = np.einsum("bij,bj->bi", At, x) + np.einsum("bij,bj->bi", Bt, u)
            J += np.einsum("bi,ij,bj->b", x, self.Q, x) + np.einsum("bi,ij,bj->b", u, self.R, u)
            X[:, :, t + 1], U[:, :, t] = x, u
        return {"J_T": J, "X": np.moveaxis(X, 0, -1), "U": np.moveaxis(U, 0, -1), "ok": ok}


def referee(p):
    return _memo("referee", p, lambda: Referee(p))


def cond_H(p):
    """cond_2(H_b) per instance (H does not depend on x0 or the references): numpy.linalg.cond on the fp64 copy"""
    return _memo("cond", p, lambda: np.array([np.linalg.cond(Hb) for Hb in np.asarray(referee(p).H, dtype=np.float64)]))


def cond_Re(p):
    """cond_2(R + B'PB) per instance: the stage matrix of the last stage"""
    return np.array([np.linalg.cond(p["R"] + p["B"][:, :, b].T @ p["P"] @ p["B"][:, :, b]) for b in range(p["B"].shape[2])])


def model_roll(p, x0, U):
    """x_0 = x0, x_{i+1} = A x_i + B u_i in long double: (nx, N + 1, Bsz)"""
    A, B = np.asarray(p["A"], dtype=LD), np.asarray(p["B"], dtype=LD)
    X = np.zeros((x0.shape[0], p["N"] + 1, x0.shape[1]), dtype=LD)
    X[:, 0] = x0
    for i in range(p["N"]):
        X[:, i + 1] = np.einsum("acb,cb->ab", A, X[:, i]) + np.einsum("akb,kb->ab", B, np.asarray(U[:, i], dtype=LD))
    return X


def oracle_plan(p, x0):
    """the fp64 oracle's whole plan (nu, N, Bsz) and its V_N (Bsz,) at the states x0 (nx, Bsz)"""
    nu, Bsz = p["B"].shape[1], x0.shape[1]
    U, V = np.zeros((nu, p["N"], Bsz)), np.zeros(Bsz)
    for b in range(Bsz):
        s = orc.solve(p["N"], p["A"][:, :, b], p["B"][:, :, b], p["Q"], p["R"], p["P"], p["lb"], p["ub"], x0[:, b], *refs(p))
        U[:, :, b], V[b] = s["U"], s["V_N"]
    return U, V


def exact_solve(p):
    """the referee at x0"""
    return _memo("solve", p, lambda: referee(p).solve(p["x0"]))


def on_bound(p, U):
    """entries of a referee's plan that ARE a bound (certify puts them there)"""
    return (U == np.asarray(p["lb"], dtype=LD)[:, None, None]) | (U == np.asarray(p["ub"], dtype=LD)[:, None, None])


def partly(p):
    """share of the instances with some but not all entries of U* on a bound"""
    on = on_bound(p, exact_solve(p)["U"])
    return float(np.mean(on.any(axis=(0, 1)) & ~on.all(axis=(0, 1))))


def plant(p):
    """hard model, stable plant: A_true = A (0.9 / rho(A)) on the grid, B_true = B, per instance"""
    At = np.stack([grid(p["A"][:, :, b] * (0.9 / _rho(p["A"][:, :, b]))) for b in range(p["A"].shape[2])], axis=2)
    return np.ascontiguousarray(At), p["B"]


def exact_roll(p):
    return _memo("roll", p, lambda: referee(p).rollout(T_ROLL, *plant(p)))


def exact_steps(p):
    """the T_ROLL states of the referee's own closed-loop trajectory rounded to fp64, and the referee at each: a list of (x, dict)"""
    def f():
        X = exact_roll(p)["X"]
        out = []
        for t in range(T_ROLL):
            x = np.ascontiguousarray(np.asarray(X[:, t], dtype=np.float64))
            out.append((x, referee(p).solve(x)))
        return out
    return _memo("steps", p, f)


# ---------------- errors, per instance (the instance axis is last) ----------------
def u_err(u, ur, h):
    """max |u - u*| / max(|u*|, h) per instance; u (nu, ..., Bsz), each input row with its own half-width"""
    u, ur = np.asarray(u, dtype=LD), np.asarray(ur, dtype=LD)
    hh = np.asarray(h, dtype=LD).reshape((-1,) + (1,) * (u.ndim - 1))
    e = np.abs(u - ur) / np.maximum(np.abs(ur), hh)
    return np.asarray(e.max(axis=tuple(range(u.ndim - 1))), dtype=np.float64)


def rel_err(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return np.asarray(np.abs(a - b) / np.abs(b), dtype=np.float64)


def x_err(X, Xr):
    """max |X - X*| / max |X*| per instance"""
    X, Xr = np.asarray(X, dtype=LD), np.asarray(Xr, dtype=LD)
    ax = tuple(range(X.ndim - 1))
    return np.asarray(np.abs(X - Xr).max(axis=ax) / np.abs(Xr).max(axis=ax), dtype=np.float64)


# ---------------- the fp64 oracle against the referee: what the constants C come from ----------------
STEP_CASES = [("unstable", (4, 2, 10)), ("redundant", (4, 2, 10)), ("redundant", (4, 4, 4)), ("unstable", (7, 3, 11)), ("unstable", (8, 4, 30))]
ROLL_CASES = [("unstable", (4, 2, 10)), ("unstable", (2, 1, 30)), ("unstable", (4, 2, 20)), ("unstable", (7, 3, 11)), ("unstable", (8, 4, 30)),
              ("redundant", (4, 2, 10))]


def oracle_errors(p, entry):
    """per instance errors of the fp64 oracle against the referee: {'U': (Bsz,), 'V' or 'J': (Bsz,)}; for 'step' the worst of the steps"""
    if entry == "solve":
        U, V = oracle_plan(p, p["x0"])
        e = exact_solve(p)
        return dict(U=u_err(U, e["U"], p["h"]), V=rel_err(V, e["V"]))
    if entry == "step":
        out = dict(U=0.0, V=0.0)
        for x, e in exact_steps(p):
            U, V = oracle_plan(p, x)
            out = dict(U=np.maximum(out["U"], u_err(U, e["U"], p["h"])), V=np.maximum(out["V"], rel_err(V, e["V"])))
        return out
    At, Bt = plant(p)
    g = orc.rollout_batch(T_ROLL, *qa(p), p["x0"], At, Bt, *refs(p), want_traj=True)
    e = exact_roll(p)
    return dict(U=u_err(g["U"], e["U"], p["h"]), J=rel_err(g["J_T"], e["J_T"]))
