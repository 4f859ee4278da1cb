"""CPU: the long-double reference (oracle/exact.py) against the fp64 oracle, scipy's BVLS, its own closed forms and the
reference's committed data.  It is the referee of tests/test_gpu_domain_edges.py, so it is pinned here first, also at the
shapes the golden npz has no data for (n_x up to 17, n_u up to 9, n up to 160)."""
import os

import numpy as np
import pytest

from oracle import exact as ex
from oracle import oracle as orc

A0 = np.array([[1.0, 0.7], [0.12, 0.4]])
B0 = np.array([[1.0], [1.2]])
Q2 = 2.0 * np.eye(2)
R1 = np.eye(1)
X_START = np.array([0.15916231240837822, 0.15916231240837819])


def rel(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def problem(nx, nu, N, Bsz, seed, refs=True, box=None):
    """Well-conditioned: spectral radius in [0.5, 1], SPD Q / R / P with condition <= 10 and P != Q, asymmetric box, references,
    x0 free / partly / fully saturated."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((nx, nx, Bsz))
    A *= rng.uniform(0.5, 1.0, Bsz) / np.abs(np.linalg.eigvals(A.transpose(2, 0, 1))).max(axis=1)
    B = rng.standard_normal((nx, nu, Bsz)) * rng.uniform(0.3, 1.0, (1, 1, Bsz))

    def spd(m, c):
        q, _ = np.linalg.qr(rng.standard_normal((m, m)))
        return (q * np.geomspace(1.0, c, m)) @ q.T
    Q, R, P = spd(nx, 10.0), spd(nu, 10.0), 3.0 * spd(nx, 10.0)
    lb, ub = box if box is not None else (-rng.uniform(0.1, 0.4, nu), rng.uniform(0.1, 0.4, nu))
    x0 = rng.standard_normal((nx, Bsz)) * rng.choice([0.01, 0.3, 3.0], Bsz)
    xr = 0.2 * rng.standard_normal((nx, N)) if refs else None
    ur = 0.05 * rng.standard_normal((nu, N)) if refs else None
    return dict(N=N, A=np.ascontiguousarray(A), B=np.ascontiguousarray(B), Q=Q, R=R, P=P, lb=np.asarray(lb, float),
                ub=np.asarray(ub, float), x0=np.ascontiguousarray(x0), x_ref=xr, u_ref=ur)


def qp_args(p):
    return (p["N"], p["A"], p["B"], p["Q"], p["R"], p["P"], p["lb"], p["ub"], p["x0"])


def test_condensed_hessian_and_gradient_match_the_oracle():
    p = problem(3, 2, 7, 3, 1, refs=False)
    H, g, c = ex.condense(p["N"], p["A"], p["B"], p["Q"], p["R"], p["P"], p["x0"])
    for b in range(3):
        Ho, Fo = orc.condense(p["A"][:, :, b], p["B"][:, :, b], p["Q"], p["R"], p["P"], p["N"])
        assert np.max(np.abs(H[b] - Ho)) < 1e-13 * np.max(np.abs(Ho))
        go = Fo @ p["x0"][:, b]
        assert np.max(np.abs(g[b] - go)) < 1e-13 * np.max(np.abs(go))


@pytest.mark.parametrize("nx,nu,N", [(2, 1, 10), (4, 2, 10), (8, 4, 30), (12, 2, 10), (17, 1, 10), (3, 9, 4), (10, 8, 16),
                                     (2, 1, 160)])
def test_agrees_with_the_oracle(nx, nu, N):
    """V_N, the whole of U and the closed loop against lqo_solve / lqo_rollout_batch: the two differ in arithmetic and
    algorithm (fp64 primal active set on the oracle's condensing vs long-double certificate on an independent condensing)."""
    p = problem(nx, nu, N, 6, 10 * nx + N)
    e = ex.solve(*qp_args(p), p["x_ref"], p["u_ref"])
    assert e["ok"].all()
    for b in range(6):
        r = orc.solve(p["N"], p["A"][:, :, b], p["B"][:, :, b], p["Q"], p["R"], p["P"], p["lb"], p["ub"], p["x0"][:, b],
                      p["x_ref"], p["u_ref"])
        assert rel(e["V"][b], r["V_N"]) < 1e-12
        assert np.max(np.abs(e["U"][:, :, b] - r["U"])) < 1e-12 * np.max(p["ub"] - p["lb"])
    saturated = np.isclose(e["U"], p["lb"][:, None, None]) | np.isclose(e["U"], p["ub"][:, None, None])
    assert saturated.any() and not saturated.all()          # the mix has active and free inputs
    if N * nu <= 40:
        T = 5
        er = ex.rollout(T, *qp_args(p), p["A"][:, :, 0], p["B"][:, :, 0], p["x_ref"], p["u_ref"])
        rr = orc.rollout_batch(T, *qp_args(p), p["A"][:, :, 0], p["B"][:, :, 0], p["x_ref"], p["u_ref"], want_traj=True)
        assert rel(er["J_T"], rr["J_T"]) < 1e-12
        assert np.max(np.abs(er["U"] - rr["U"])) < 1e-12 and np.max(np.abs(er["X"] - rr["X"])) < 1e-12 * np.max(np.abs(rr["X"]))


def test_agrees_with_oracle_boxqp_and_bvls():
    """The box QP itself against lqo_boxqp and scipy's bounded-variable least squares on u'Hu + 2g'u = |L'u + L^-1 g|^2 + const."""
    from scipy.optimize import lsq_linear
    p = problem(4, 2, 12, 4, 3)
    H, g, _ = ex.condense(*qp_args(p)[:6], p["x0"], p["x_ref"], p["u_ref"])
    lb, ub = np.tile(p["lb"], p["N"]), np.tile(p["ub"], p["N"])
    for b in range(4):
        Hd, gd = H[b].astype(np.float64), g[b].astype(np.float64)
        u, ok = ex.certify_qp(Hd, gd, lb, ub, np.zeros_like(gd))      # a wrong candidate: the long-double loop finishes it
        assert not ok
        f = lambda v: v @ Hd @ v + 2 * gd @ v
        uo, _ = orc.boxqp(Hd, gd, lb, ub)
        L = np.linalg.cholesky(Hd)
        ub_ = lsq_linear(L.T, -np.linalg.solve(L, gd), bounds=(lb, ub), method="bvls", tol=1e-15).x
        ud = u.astype(np.float64)
        assert np.max(np.abs(ud - uo)) < 1e-12 and np.max(np.abs(ud - ub_)) < 1e-12
        assert abs(f(ud) - f(uo)) <= 1e-12 * abs(f(uo))


def test_reproduces_the_golden_data(golden_dir):
    """V_expert of data_lq_mpc_multipleSys.npz (N = 30) to 1e-13, and a sample of its true_cost_error table (closed loop,
    T = 30, N = 7)."""
    d = np.load(os.path.join(golden_dir, "data_lq_mpc_multipleSys.npz"))
    e = ex.solve(30, A0[:, :, None], B0[:, :, None], Q2, R1, Q2, [-0.1], [0.1], X_START[:, None])
    assert e["ok"].all() and rel(e["V"][0], float(d["V_expert"])) < 1e-13
    eA = np.load(os.path.join(golden_dir, "error_A_f.npy"))
    eB = np.load(os.path.join(golden_dir, "error_B_f.npy"))
    idx = np.arange(0, 1000, 97)
    A = np.ascontiguousarray((A0[:, :, None, None] + eA).reshape(2, 2, 1000)[:, :, idx])
    B = np.ascontiguousarray((B0[:, :, None, None] + eB).reshape(2, 1, 1000)[:, :, idx])
    J = ex.rollout(30, 7, A, B, Q2, R1, Q2, [-0.1], [0.1], np.repeat(X_START[:, None], idx.size, 1), A0, B0)["J_T"]
    assert rel(J, d["true_cost_error"].reshape(-1)[idx]) < 1e-13


@pytest.mark.parametrize("nx,nu,N", [(4, 2, 10), (17, 1, 10), (3, 9, 4), (2, 1, 160)])
def test_riccati_closed_form(nx, nu, N):
    """A box that is never active: the condensed QP's optimum is the Riccati recursion's, and the recursion's input sequence,
    simulated, costs what the recursion says (three derivations of the same number: condensing, dynamic programming,
    simulation)."""
    p = problem(nx, nu, N, 5, 7 * N + nu, box=(-1e6 * np.ones(nu), 1e6 * np.ones(nu)))
    ric = ex.riccati(p["N"], p["A"], p["B"], p["Q"], p["R"], p["P"], p["x0"], p["x_ref"], p["u_ref"])
    assert np.max(np.abs(ric["U"])) < 1e3
    e = ex.solve(*qp_args(p), p["x_ref"], p["u_ref"])
    assert rel(e["V"], ric["V"]) < 1e-15 and np.max(np.abs(e["U"] - ric["U"])) < 1e-15 * max(1.0, float(np.abs(ric["U"]).max()))
    seq = ex.sequence_cost(p["N"], p["A"], p["B"], p["Q"], p["R"], p["P"], p["x0"], ric["U"], p["x_ref"], p["u_ref"])
    assert rel(seq, ric["V"]) < 1e-16


def test_pinned_box_closed_form():
    """A box 1e-9 wide: every input sits on a bound, and V_N is within |grad V(u_pin)|_1 * width of the cost of the input pinned
    at lb (convexity: 0 <= V(u_pin) - V* <= grad V(u_pin)'(u_pin - u*))."""
    w = 1e-9
    p = problem(4, 2, 10, 6, 5, box=(np.full(2, 0.05), np.full(2, 0.05 + w)))
    e = ex.solve(*qp_args(p), p["x_ref"], p["u_ref"])
    assert e["ok"].all()
    pin = np.broadcast_to(p["lb"][:, None, None], e["U"].shape)
    Vpin = ex.sequence_cost(p["N"], p["A"], p["B"], p["Q"], p["R"], p["P"], p["x0"], pin, p["x_ref"], p["u_ref"])
    H, g, _ = ex.condense(*qp_args(p)[:6], p["x0"], p["x_ref"], p["u_ref"])
    upin = np.moveaxis(pin, -1, 0).transpose(0, 2, 1).reshape(6, -1).astype(np.longdouble)
    grad = 2 * (np.einsum("bij,bj->bi", H, upin) + g)
    gap = Vpin - e["V"]
    assert np.all(gap >= -1e-18 * Vpin) and np.all(gap <= np.abs(grad).sum(axis=1) * w * (1 + 1e-9))
    seq = ex.sequence_cost(p["N"], p["A"], p["B"], p["Q"], p["R"], p["P"], p["x0"], e["U"], p["x_ref"], p["u_ref"])
    assert rel(seq, e["V"]) < 1e-16


def test_one_sided_and_zero_excluding_boxes():
    """Boxes the GPU tests use: [0, 0.2], [0.02, 0.3] and [-0.4, -0.01] (x0 = 0 included), [0, 1e6] and [-1e30, 0.2]."""
    for k, box in enumerate([(0.0, 0.2), (0.02, 0.3), (-0.4, -0.01), (0.0, 1e6), (-1e30, 0.2)]):
        p = problem(4, 2, 10, 5, 40 + k, box=(np.full(2, box[0]), np.full(2, box[1])))
        p["x0"][:, 0] = 0.0
        e = ex.solve(*qp_args(p), p["x_ref"], p["u_ref"])
        r = orc.solve_batch(*qp_args(p), p["x_ref"], p["u_ref"])
        assert e["ok"].all() and rel(e["V"], r["V_N"]) < 1e-12
        assert np.max(np.abs(e["u_0"] - r["u_0"])) < 1e-12 * max(1.0, float(np.abs(e["u_0"]).max()))
        assert np.all(e["U"] >= box[0]) and np.all(e["U"] <= box[1])
