"""GPU (-m gpu): closed-loop rollouts of a prepared batch controller (BatchController.rollout / lqmpc_controller_rollout*) against the
fp64 oracle's rollout_batch.

Problems: one base plant (A0 with spectral radius 0.95, B0 = 0.6 randn) and per-instance models around it
(A_b = A0 + 0.05 U(0,1) randn / nx, B_b = B0 + 0.05 U(0,1) randn / sqrt(nx nu)); Q, R, P and x0 as test_gpu_controller.problem()
draws them; box +-0.3, T = 8, seed 1.  Bars, the project's own for rollouts (tests/test_gpu_parity.py): J_T relative error <= 1e-5,
|u - u*| <= 1e-5 max(|u*|, 1e-3 * 0.3), |x - x*| <= 1e-5 max(|x*|, 1e-3 max_t |x*_t| of the instance), status 0 everywhere.
Every parity test first asserts, from the ORACLE's U, that at least 15 % of the (instance, step) pairs have an input on its bound,
at least 15 % have every input strictly inside, and at least 15 % of the instances have both kinds of step (the lazy load of W in
mid-rollout).  With this generator and seed 1 the smallest shares over the shapes below are 19 %, 56 % and 17 %.
"""
import numpy as np
import pytest

from test_gpu_controller import DevArray, opts  # noqa: F401  (opts: a fixture)
from lq_mpc_amd import BatchController
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

RTOL, U_MAX, T = 1e-5, 0.3, 8
# shape -> (batch size, ctl_wg, what the rollout must have launched)
RECORD = {(4, 2, 10): 67, (2, 1, 10): 67, (4, 2, 20): 35, (7, 3, 11): 37}
WG = {(9, 5, 7): 35, (6, 2, 33): 24, (8, 4, 30): 24}
CASES = ([(s, b, 0, "rec") for s, b in RECORD.items()] + [(s, b, 1, "wg") for s, b in WG.items()] +
         [((12, 2, 10), 24, 0, "pass"), ((8, 4, 30), 24, 0, "pass")])
_cache = {}


def problem(nx, nu, N, Bsz, seed=1, lb=-0.3, ub=0.3):
    rng = np.random.default_rng(seed)
    A0 = rng.standard_normal((nx, nx))
    A0 *= 0.95 / np.abs(np.linalg.eigvals(A0)).max()
    B0 = 0.6 * rng.standard_normal((nx, nu))
    A = A0[:, :, None] + 0.05 * rng.uniform(0, 1, Bsz) * rng.standard_normal((nx, nx, Bsz)) / nx
    B = B0[:, :, None] + 0.05 * rng.uniform(0, 1, Bsz) * rng.standard_normal((nx, nu, Bsz)) / np.sqrt(nx * nu)

    def spd(m, c):
        q, _ = np.linalg.qr(rng.standard_normal((m, m)))
        return (q * np.geomspace(1.0, c, m)) @ q.T
    Q, R, P = spd(nx, 10.0), spd(nu, 10.0), 3.0 * spd(nx, 10.0)
    x0 = rng.standard_normal((nx, Bsz)) * rng.choice([0.01, 0.3, 3.0], Bsz)
    return dict(N=N, A=np.ascontiguousarray(A), B=np.ascontiguousarray(B), Q=Q, R=R, P=P, lb=lb * np.ones(nu), ub=ub * np.ones(nu),
                x0=np.ascontiguousarray(x0), A0=A0, B0=B0, x_ref=None, u_ref=None)


def qa(p):
    return (p["N"], p["A"], p["B"], p["Q"], p["R"], p["P"], p["lb"], p["ub"])


def plant(p, per):
    return (p["A"], p["B"]) if per else (p["A0"], p["B0"])


def oracle_roll(p, per, steps=T, x0=None):
    return orc.rollout_batch(steps, *qa(p), p["x0"] if x0 is None else x0, *plant(p, per), p["x_ref"], p["u_ref"], want_traj=True)


def case(shape, Bsz, per):
    """the problem and the oracle's rollout on it, computed once and never modified"""
    key = (shape, Bsz, per)
    if key not in _cache:
        p = _cache.get((shape, Bsz, not per), [None])[0] or problem(*shape, Bsz)
        _cache[key] = (p, oracle_roll(p, per))
    return _cache[key]


def mix_shares(p, ref):
    ctr, h = 0.5 * (p["ub"] + p["lb"])[:, None, None], 0.5 * (p["ub"] - p["lb"])[:, None, None]
    v = np.abs(ref["U"] - ctr)
    sat = np.any(v >= h * (1 - 1e-9), axis=0)                   # (step, instance)
    inside = np.all(v < h * (1 - 1e-6), axis=0)
    both = sat.any(axis=0) & inside.any(axis=0)
    return sat.mean(), inside.mean(), both.mean()


def assert_mixed(p, ref, tag=""):
    s = mix_shares(p, ref)
    print(f"{tag} mix: on a bound {s[0]:.2f}  inside {s[1]:.2f}  instances with both {s[2]:.2f}")
    assert min(s) >= 0.15, s


def errors(got, ref, keep=None):
    k = slice(None) if keep is None else keep
    ld = np.longdouble
    ej = float(np.max(np.abs(got["J_T"][k].astype(ld) - ref["J_T"][k]) / np.abs(ref["J_T"][k])))
    eu = ex = 0.0
    if got.get("U") is not None:
        u, ur = got["U"][..., k].astype(ld), ref["U"][..., k]
        eu = float(np.max(np.abs(u - ur) / np.maximum(np.abs(ur), 1e-3 * U_MAX)))
        x, xr = got["X"][..., k].astype(ld), ref["X"][..., k]
        floor = 1e-3 * np.abs(xr).max(axis=(0, 1))
        ex = float(np.max(np.abs(x - xr) / np.maximum(np.abs(xr), floor)))
    return ej, eu, ex


def check(got, ref, tag, keep=None):
    ej, eu, ex = errors(got, ref, keep)
    print(f"{tag}: J_T relerr {ej:.2e}  U err {eu:.2e}  X err {ex:.2e}")
    if got.get("status") is not None:
        st = got["status"] if keep is None else got["status"][keep]
        assert np.all(st == 0), np.flatnonzero(st)[:10]
    assert ej <= RTOL and eu <= RTOL and ex <= RTOL, (tag, ej, eu, ex)


def controller(solver, p):
    return BatchController(solver, *qa(p), p["x_ref"], p["u_ref"])


@pytest.fixture
def wg(solver):
    def set_(v):
        solver.set_options(ctl_wg=v)
    yield set_
    solver.set_options(ctl_wg=0)


def dev_rollout(solver, ctl, p, per, want_traj, steps=T):
    nx, nu, Bsz = p["B"].shape
    dx = DevArray((nx, Bsz), init=p["x0"])
    dJ, dst, dit = DevArray(Bsz), DevArray(Bsz, np.int32), DevArray(Bsz, np.int32)
    dX = DevArray((nx, steps + 1, Bsz)) if want_traj else None
    dU = DevArray((nu, steps, Bsz)) if want_traj else None
    At, Bt = plant(p, per)
    if per:
        At, Bt = DevArray(At.shape, init=At), DevArray(Bt.shape, init=Bt)
    ctl.rollout_dev(steps, dx, At, Bt, dJ, dX, dU, dst, dit, true_per_instance=per)
    solver.sync()
    return {"J_T": dJ.numpy(), "X": dX.numpy() if want_traj else None, "U": dU.numpy() if want_traj else None,
            "status": dst.numpy(), "iters": dit.numpy()}


def assert_kernel(solver, ctl, kind, one_shot=None):
    k = solver.last_kernel()
    if kind == "pass":
        assert "ctl" not in k and k == one_shot, (k, one_shot)     # the kernel lqmpc_rollout_batch runs on this shape
    else:
        assert "ctl" in k and "roll" in k, k
        if kind == "wg":
            assert k == "lqmpc_wg_ctl_rollout_kernel"


# ---------------- 1. parity against the oracle's rollout_batch ----------------
@pytest.mark.parametrize("shape,Bsz,ctl_wg,kind", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_rollout_equals_the_oracle(solver, wg, shape, Bsz, ctl_wg, kind):
    wg(ctl_wg)
    for per in (False, True):
        p, ref = case(shape, Bsz, per)
        assert_mixed(p, ref, f"{shape} per={per}")
    p = case(shape, Bsz, False)[0]
    one_shot = None
    if kind == "pass":
        solver.rollout_batch(T, *qa(p), p["x0"], p["A0"], p["B0"])
        one_shot = solver.last_kernel()
    with controller(solver, p) as ctl:
        name = ctl.kernel
        assert ("ctl" in name) == (kind != "pass"), name
        for per in (False, True):
            ref = case(shape, Bsz, per)[1]
            for traj in (True, False):
                got = ctl.rollout(T, p["x0"], *plant(p, per), want_traj=traj)
                assert_kernel(solver, ctl, kind, one_shot)
                assert (got["X"] is None) == (not traj)
                check(got, ref, f"{shape} {kind} per={per} traj={traj} host")
                check(dev_rollout(solver, ctl, p, per, traj), ref, f"{shape} {kind} per={per} traj={traj} dev")
                assert_kernel(solver, ctl, kind, one_shot)
            assert ctl.kernel == name


# ---------------- 2. equal to the loop it replaces ----------------
@pytest.mark.parametrize("shape,Bsz,ctl_wg", [((4, 2, 10), 67, 0), ((7, 3, 11), 37, 0), ((9, 5, 7), 35, 1)], ids=str)
def test_rollout_equals_the_step_loop(solver, wg, shape, Bsz, ctl_wg):
    wg(ctl_wg)
    p, ref = case(shape, Bsz, True)
    assert_mixed(p, ref)
    with controller(solver, p) as ctl, controller(solver, p) as twin:
        got = ctl.rollout(T, p["x0"], p["A"], p["B"], want_traj=True)
        nx, nu, _ = p["B"].shape
        X, U = np.empty((nx, T + 1, Bsz)), np.empty((nu, T, Bsz))
        X[:, 0] = p["x0"]
        J = np.einsum("ai,ab,bi->i", X[:, 0], p["Q"], X[:, 0])
        for t in range(T):
            s = twin.step(np.ascontiguousarray(X[:, t]))
            assert np.all(s["status"] == 0)
            U[:, t] = s["u_0"]
            X[:, t + 1] = np.einsum("abi,bi->ai", p["A"], X[:, t]) + np.einsum("aki,ki->ai", p["B"], U[:, t])
            J += np.einsum("ai,ab,bi->i", X[:, t + 1], p["Q"], X[:, t + 1]) + np.einsum("ki,kj,ji->i", U[:, t], p["R"], U[:, t])
    check(got, {"J_T": J, "X": X, "U": U}, f"{shape} against the step loop")
    check({"J_T": J, "X": X, "U": U}, ref, f"{shape} step loop against the oracle")


# ---------------- 3. read-only ----------------
@pytest.mark.parametrize("shape,Bsz,ctl_wg", [((4, 2, 10), 67, 0), ((4, 2, 20), 35, 0), ((7, 3, 11), 37, 0), ((9, 5, 7), 35, 1)], ids=str)
def test_rollout_leaves_the_controller_alone(solver, wg, shape, Bsz, ctl_wg):
    wg(ctl_wg)
    p, _ = case(shape, Bsz, True)
    x1 = p["x0"]
    x2 = np.einsum("abi,bi->ai", p["A"], x1)                      # somewhere the carried face matters
    with controller(solver, p) as ctl, controller(solver, p) as twin:
        a1, b1 = ctl.step(x1), twin.step(x1)
        r1 = ctl.rollout(T, 0.5 * x1, p["A0"], p["B0"], want_traj=True)
        r2 = ctl.rollout(T, 0.5 * x1, p["A0"], p["B0"], want_traj=True)
        a2, b2 = ctl.step(x1), twin.step(x1)
        r3 = ctl.rollout(T, x1, p["A"], p["B"])
        a3, b3 = ctl.step(x2), twin.step(x2)
    for k in ("u_0", "V_N", "status", "iters"):
        assert np.array_equal(a1[k], b1[k]), k
        assert np.array_equal(a2[k], b2[k]), k
        assert np.array_equal(a3[k], b3[k]), k
    assert (a2["iters"] > 0).any() and (a3["iters"] > 0).any() and np.all(r3["status"] == 0)
    for k in ("J_T", "X", "U", "status", "iters"):
        assert np.array_equal(r1[k], r2[k]), k


# ---------------- 4. after set_reference and set_model ----------------
@pytest.mark.parametrize("shape,Bsz,ctl_wg", [((4, 2, 10), 67, 0), ((9, 5, 7), 35, 1)], ids=str)
def test_rollout_after_new_references_and_models(solver, wg, shape, Bsz, ctl_wg):
    wg(ctl_wg)
    nx, nu, N = shape
    base = case(shape, Bsz, False)[0]
    rng = np.random.default_rng(11)
    q = dict(base, lb=-0.2 * np.ones(nu), ub=0.4 * np.ones(nu))
    with controller(solver, q) as ctl:
        name = ctl.kernel
        q["x_ref"], q["u_ref"] = 0.1 * rng.standard_normal((nx, N)), 0.05 * rng.standard_normal((nu, N))
        ctl.set_reference(q["x_ref"], q["u_ref"])
        idx = np.arange(1, Bsz, 3)
        fresh = problem(*shape, Bsz, seed=5)
        q["A"], q["B"] = base["A"].copy(), base["B"].copy()
        q["A"][..., idx] = fresh["A"][..., idx]
        q["B"][..., idx] = fresh["B"][..., idx]
        ctl.set_model(np.ascontiguousarray(q["A"][..., idx]), np.ascontiguousarray(q["B"][..., idx]), idx)
        for per in (False, True):
            ref = oracle_roll(q, per)
            assert_mixed(q, ref, f"{shape} per={per}")
            got = ctl.rollout(T, q["x0"], *plant(q, per), want_traj=True)
            assert "ctl" in solver.last_kernel() and "roll" in solver.last_kernel()
            check(got, ref, f"{shape} new references and models, per={per}")
        assert ctl.kernel == name


# ---------------- 5. edges ----------------
@pytest.mark.parametrize("shape,Bsz,ctl_wg", [((4, 2, 10), 67, 0), ((9, 5, 7), 35, 1)], ids=str)
def test_rollout_edges(solver, wg, shape, Bsz, ctl_wg):
    wg(ctl_wg)
    p, ref = case(shape, Bsz, True)
    with controller(solver, p) as ctl:
        one = ctl.rollout(1, p["x0"], p["A"], p["B"], want_traj=True)
        check(one, oracle_roll(p, True, steps=1), f"{shape} T=1")
        xn = p["x0"].copy()
        bad = 5
        xn[1, bad] = np.nan
        keep = np.arange(Bsz) != bad
        got = ctl.rollout(T, xn, p["A"], p["B"], want_traj=True)
        assert got["status"][bad] == 2, got["status"][bad]
        check(got, ref, f"{shape} one NaN state", keep)
        check(ctl.rollout(T, p["x0"], p["A"], p["B"], want_traj=True), ref, f"{shape} after the NaN")
    # a batch of one: the instance of the full batch with the most steps on a bound and at least one inside
    s = np.abs(ref["U"]).max(axis=0) >= 0.3 * (1 - 1e-9)
    i = int(np.argmax(np.where(s.all(axis=0), -1, s.sum(axis=0))))
    assert 0 < s[:, i].sum() < T
    p1 = dict(p, A=np.ascontiguousarray(p["A"][..., i:i + 1]), B=np.ascontiguousarray(p["B"][..., i:i + 1]),
              x0=np.ascontiguousarray(p["x0"][..., i:i + 1]))
    with controller(solver, p1) as ctl:
        got = ctl.rollout(T, p1["x0"], p1["A"], p1["B"], want_traj=True)
        assert "roll" in solver.last_kernel()
        check(got, {k: ref[k][..., i:i + 1] for k in ("J_T", "X", "U")}, f"{shape} Bsz=1")


# ---------------- 6. hand-back ----------------
@pytest.mark.parametrize("shape,Bsz", [((4, 2, 10), 67), ((7, 3, 11), 37)], ids=str)
def test_rollout_hand_back(solver, opts, shape, Bsz):  # noqa: F811
    opts(r16_maxit=1)
    for per in (False, True):
        p, ref = case(shape, Bsz, per)
        assert_mixed(p, ref)
        with controller(solver, p) as ctl:
            assert "ctl" in ctl.kernel
            got = ctl.rollout(T, p["x0"], *plant(p, per), want_traj=True)
            assert "ctl" in solver.last_kernel() and "roll" in solver.last_kernel()
            check(got, ref, f"{shape} r16_maxit=1 per={per}")
