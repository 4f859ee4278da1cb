"""CPU: the hard QP cases of tests/qp_hard.py are what they claim to be, their referee is right, and the constants of their bars are
the oracle's own.

  * the caps, per (shape, family): cond_2(H) <= 1e8 on every instance; unstable: >= 1e3 on every instance and the next rung of the
    ladder breaks the cap; redundant: cond_2(R + B'PB) >= 1e4 and the next smaller r breaks the cap; at least a quarter of the
    instances partly saturated; every input a multiple of 2^-24
  * the referee: qp_hard.Referee (H condensed once) is oracle/exact.py's solve and rollout bit for bit; on the hardest instance (of those not saturated throughout) of each
    family at (4,2,10), (2,4,8) and (2,1,30) condensing and the solve on the certified face are restated in mpmath at 50 digits (with
    the KKT signs on that face), and the referee's U and V are within 2^-8 eps cond_2(H) of that: a sixteenth of what long double
    (2^-11 eps) times the ratios below should give
  * the constants qp_hard.C: the fp64 oracle against the referee, worst err / (eps cond_2(H_b)) over the instances with
    cond_2(H_b) >= 1e3 (below that the floor of the bar is a thousand times what c eps cond gives, and the ratio of an error of one ulp
    says nothing), per entry point and quantity; c = 16 x that, rounded up to a power of two.  Measured (gcc, x86-64):

        entry     quantity   worst ratio   c
        solve     U          0.557         16
        solve     V_N        1.93          32
        step      U          0.516         16
        step      V_N        1.15          32
        rollout   U          0.558         16
        rollout   J_T        0.224         4

    asserted: the oracle stays below c / 16, and above c / 32 (the constant is not looser than the rule gives).
"""
import numpy as np
import pytest

import qp_hard as qh
from oracle import exact as ex

LD = np.longdouble
IDS = [f"{f}-{'x'.join(map(str, s))}" for f, s in qh.CASE_LIST]


@pytest.mark.parametrize("family,shape", qh.CASE_LIST, ids=IDS)
def test_caps(family, shape):
    p = qh.problem(family, shape)
    c = qh.cond_H(p)
    e = qh.exact_solve(p)
    share = qh.partly(p)
    print(f"{family} {shape}: cond_2(H) {c.min():.2e} .. {c.max():.2e}, cond_2(R + B'PB) {qh.cond_Re(p).max():.2e}, partly {share:.2f}, "
          f"certified as given {e['ok'].mean():.2f}")
    assert c.max() <= qh.CAP
    assert share >= 0.25
    for a in (p["A"], p["B"], p["lb"], p["ub"]) + (() if family == "near_degenerate" else (p["x0"],)):
        assert np.array_equal(a * qh.GRID, np.round(a * qh.GRID))
    if family == "unstable":
        assert c.min() >= 1e3
        i = qh.LADDER.index(qh.RUNG[shape])
        if i + 1 < len(qh.LADDER):
            assert qh.cond_H(qh.problem(family, shape, rho=qh.LADDER[i + 1])).max() > qh.CAP
    if family == "redundant":
        assert qh.cond_Re(p).max() >= 1e4 and qh.COND_RE[shape] >= 1e4
        assert abs(qh.cond_Re(p).max() / qh.COND_RE[shape] - 1) < 1e-3              # the recorded figure is this generator's
        i = qh.R_LADDER.index(qh.R_CHEAP[shape])
        if i > 0:
            assert qh.cond_H(qh.problem(family, shape, r=qh.R_LADDER[i - 1])).max() > qh.CAP
    if family != "near_degenerate":
        assert e["ok"].all()                                 # the fp64 oracle's face is the optimal one on every instance
    else:
        # the ladder: the largest |v_unc,i| / h_i of the unconstrained minimiser is 1 + k to a few ulps
        U = ex.riccati(*qh.qa(p)[:6], p["x0"])["U"]
        m = np.max(np.abs(U) / np.asarray(p["h"], dtype=LD)[:, None, None], axis=(0, 1))
        k = np.array([qh.LADDER_K[b % len(qh.LADDER_K)] for b in range(m.size)], dtype=LD)
        assert np.max(np.abs(m - (1 + k))) <= 8 * qh.EPS, np.max(np.abs(m - (1 + k)))


def test_integrator_is_left_out_where_it_breaks_the_cap():
    assert "integrator" not in qh.CASES[(4, 2, 20)][0]
    assert qh.cond_H(qh.problem("integrator", (4, 2, 20))).max() > qh.CAP


@pytest.mark.parametrize("family,shape", [("unstable", (4, 2, 10)), ("redundant", (2, 4, 8)), ("near_degenerate", (7, 3, 11))], ids=str)
def test_referee_is_exact_py(family, shape):
    """H condensed once changes nothing: bit for bit exact.solve and exact.rollout"""
    p = qh.problem(family, shape)
    a, b = qh.exact_solve(p), ex.solve(*qh.qa(p), p["x0"], *qh.refs(p))
    for k in ("U", "V", "u_0", "ok"):
        assert np.array_equal(a[k], b[k]), k
    At, Bt = qh.plant(p)
    a, b = qh.exact_roll(p), ex.rollout(qh.T_ROLL, *qh.qa(p), p["x0"], At, Bt, *qh.refs(p))
    for k in ("J_T", "X", "U", "ok"):
        assert np.array_equal(a[k], b[k]), k
    H, g, c = ex.condense(*qh.qa(p)[:6], p["x0"], *qh.refs(p))
    assert np.array_equal(H, qh.referee(p).H)


# ---------------- the referee against 50 digits ----------------
def mp_solve(p, b, on):
    """Instance b at 50 digits: condensing restated from the problem statement of oracle/exact.py, the minimiser on the face `on`
    (nu, N) bool (those entries on the bound they are nearer to in the referee's plan), the KKT signs there.
    Returns (U time-major (n, 1), V, the worst multiplier of the wrong sign relative to |H|_max max(|u|_max, 1) + |g|_max, the worst bound violation)."""
    import mpmath as mp
    with mp.workdps(50):
        M = lambda a: mp.matrix(np.asarray(a, dtype=np.float64).tolist())
        N, (nx, nu, _) = p["N"], p["B"].shape
        A, B, Q, R, P = M(p["A"][:, :, b]), M(p["B"][:, :, b]), M(p["Q"]), M(p["R"]), M(p["P"])
        x0 = M(p["x0"][:, b].reshape(nx, 1))
        xr, ur = qh.refs(p)
        xr = mp.zeros(nx, N) if xr is None else M(xr)
        ur = mp.zeros(nu, N) if ur is None else M(ur)
        n = N * nu
        AkB = [B]
        for _ in range(1, N):
            AkB.append(A * AkB[-1])
        H, g, c = mp.zeros(n, n), mp.zeros(n, 1), (x0.T * Q * x0)[0]
        Ak = mp.eye(nx)
        for r in range(N):                                  # x_{r+1} = A^{r+1} x0 + sum_{j <= r} A^{r-j} B u_j
            Ak = A * Ak
            W = P if r == N - 1 else Q
            G = mp.zeros(nx, n)
            for j in range(r + 1):
                G[:, j * nu:(j + 1) * nu] = AkB[r - j]
            d = Ak * x0 - xr[:, r]
            WG = W * G
            H += G.T * WG
            g += WG.T * d
            c += (d.T * W * d)[0]
        for i in range(N):
            H[i * nu:(i + 1) * nu, i * nu:(i + 1) * nu] += R
            g[i * nu:(i + 1) * nu, 0] -= R * ur[:, i]
            c += (ur[:, i].T * R * ur[:, i])[0]
        lo, hi = [mp.mpf(float(v)) for v in p["lb"]], [mp.mpf(float(v)) for v in p["ub"]]
        u = mp.zeros(n, 1)
        act, free = [], []
        for i in range(N):
            for k in range(nu):
                if on[k, i] != 0:
                    u[i * nu + k] = lo[k] if on[k, i] < 0 else hi[k]
                    act.append(i * nu + k)
                else:
                    free.append(i * nu + k)
        if free:
            HFF = mp.matrix(len(free), len(free))
            rhs = mp.matrix(len(free), 1)
            for a_, i in enumerate(free):
                for b_, j in enumerate(free):
                    HFF[a_, b_] = H[i, j]
                rhs[a_] = -g[i] - sum(H[i, j] * u[j] for j in act)
            uf = mp.lu_solve(HFF, rhs)
            for a_, i in enumerate(free):
                u[i] = uf[a_]
        grad = H * u + g
        scale = max(abs(v) for v in H) * max(max(abs(v) for v in u), 1) + max(abs(v) for v in g)         # exact.py's _tol
        sign = max([mp.mpf(0)] + [(-grad[i] if on[i % nu, i // nu] < 0 else grad[i]) / scale for i in act])
        viol = max([mp.mpf(0)] + [max(lo[i % nu] - u[i], u[i] - hi[i % nu]) for i in free])
        V = (u.T * H * u)[0] + 2 * (g.T * u)[0] + c
        return u, V, sign, viol


REFEREE_CASES = [(f, s) for f, s in qh.CASE_LIST if s in ((4, 2, 10), (2, 4, 8), (2, 1, 30))]


@pytest.mark.parametrize("family,shape", REFEREE_CASES, ids=[f"{f}-{'x'.join(map(str, s))}" for f, s in REFEREE_CASES])
def test_referee_against_50_digits(family, shape):
    mp = pytest.importorskip("mpmath")
    p = qh.problem(family, shape)
    cond = qh.cond_H(p)
    e = qh.exact_solve(p)
    on = qh.on_bound(p, e["U"])
    b = int(np.argmax(np.where(on.all(axis=(0, 1)), 0.0, cond)))       # the hardest instance with a free entry to solve for
    Ue = e["U"][:, :, b]
    lbl, ubl = np.asarray(p["lb"], dtype=LD)[:, None], np.asarray(p["ub"], dtype=LD)[:, None]
    on = np.where(Ue == lbl, -1, np.where(Ue == ubl, 1, 0))
    u, V, sign, viol = mp_solve(p, b, on)
    nu, N = Ue.shape
    with mp.workdps(50):
        # the differences at 50 digits (a long double goes in as its exact sum of two doubles)
        two = lambda v: mp.mpf(float(v)) + mp.mpf(float(v - LD(float(v))))
        eu = max(abs(two(Ue[k, i]) - u[i * nu + k]) / max(abs(u[i * nu + k]), mp.mpf(float(p["h"][k]))) for i in range(N) for k in range(nu))
        ev = abs(two(e["V"][b]) - V) / abs(V)
        bar = 2.0 ** -8 * qh.EPS * cond[b]
        print(f"{family} {shape} instance {b}: cond {cond[b]:.2e}, U {float(eu):.2e} V {float(ev):.2e} bar {bar:.2e}, "
              f"multiplier sign {float(sign):.1e}, bound {float(viol):.1e}")
        # the face is the optimal one: no multiplier of the wrong sign beyond 1e-13 of the gradient's scale (exact.py's own test), no free entry
        # outside the box beyond 1e-15
        assert sign <= 1e-13 and viol <= 1e-15 * float(max(np.abs(p["ub"]).max(), np.abs(p["lb"]).max()))
        assert eu <= bar and ev <= bar


# ---------------- the constants ----------------
def worst_ratios():
    worst = {}
    for entry, cases in (("solve", qh.CASE_LIST), ("step", qh.STEP_CASES), ("rollout", qh.ROLL_CASES)):
        for family, shape in cases:
            p = qh.problem(family, shape)
            c = qh.cond_H(p)
            hard = c >= qh.HARD_COND
            for q, v in qh.oracle_errors(p, entry).items():
                r = float(np.max((v / (qh.EPS * c))[hard], initial=0.0))
                print(f"{entry} {family} {shape} {q}: worst error {v.max():.2e}, worst ratio {r:.3f}")
                worst[(entry, q)] = max(worst.get((entry, q), 0.0), r)
    return worst


def test_constants_of_the_bars():
    worst = worst_ratios()
    print({k: round(v, 3) for k, v in worst.items()})
    assert set(worst) == {(e, q) for e in qh.C for q in qh.C[e]}
    for (entry, q), r in worst.items():
        c = qh.C[entry][q]
        assert np.log2(c) == round(np.log2(c))
        assert c / 32 < r <= c / 16, (entry, q, r, c)
