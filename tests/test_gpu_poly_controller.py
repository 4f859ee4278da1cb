"""GPU: the prepared controller for polytopic input constraints (PolyBatchController, lqmpc_poly_controller_*).

Two kinds of check.  Against tests/poly_ref.reference, the long-double optimum, through test_gpu_poly.check: the bars of the
contract (|U - U*| <= 1e-10 max(|U*|, rho), |V_N - V_N*| <= 1e-11 V_N*, rows <= 1e-10, stationarity <= 1e-10, status 0, iters <=
10 n + 20), no instance left out.  And bit for bit (np.array_equal) against the one-shot calls solve_poly_batch / rollout_poly_batch:
every solve of the polytope kernels starts cold, and a step runs the one-shot kernel's statements on the record's values.

Measured worst per case of test 1 on one MI355X (the columns of test_gpu_poly's table; the figures are the one-shot call's, as the
bits are; iters equal to the float64 reference's on every instance):
    small-triangle      u 1.94e-15  V 8.49e-16  row 2.42e-15  stat 4.25e-16  iters 4
    small-octagon       u 3.23e-15  V 3.72e-16  row 1.54e-15  stat 5.31e-16  iters 9
    c3-octagon-hard     u 1.13e-13  V 1.23e-15  row 4.46e-14  stat 1.44e-15  iters 43
    c3-octagon-refs     u 7.15e-15  V 4.40e-16  row 3.54e-15  stat 3.87e-16  iters 32
    c2-one-sided        u 3.16e-14  V 6.97e-15  row 2.91e-14  stat 2.49e-15  iters 10
    c5-cross-hard       u 2.11e-14  V 8.41e-16  row 4.20e-14  stat 9.02e-16  iters 40
    n64-16gon-hard      u 1.47e-13  V 1.07e-15  row 5.98e-14  stat 1.75e-15  iters 193
Caller-owned loop at c3-octagon-default, T = 10: constrained share per step 0.94 0.83 0.67 0.56 0.41 0.30 0.23 0.17 0.14 0.12.
"""
import numpy as np
import pytest

import poly_ref as pr
from lq_mpc_amd import _lib, mpc
from test_gpu_controller import DevArray
from test_gpu_poly import CASES, ROLLOUTS, XREF, UREF, check, plant, problem

pytestmark = pytest.mark.gpu

REFERENCE_CASES = ["small-triangle", "small-octagon", "c3-octagon-hard", "c3-octagon-refs", "c2-one-sided", "c5-cross-hard", "n64-16gon-hard"]
SOLVE_KEYS = ("u_0", "V_N", "U_plan", "X_plan", "lam", "status", "iters")
ROLL_KEYS = ("J_T", "X", "U", "status", "iters")


def controller(solver, name, **more):
    b, N, Fu, P, kw, _, _ = problem(name)
    return mpc.PolyBatchController(solver, N, b["A"], b["B"], b["Q"], b["R"], P, Fu, **kw, **more)


def one_shot(solver, name, x0=None, A=None, B=None, **more):
    b, N, Fu, P, kw, _, _ = problem(name)
    kw = dict(kw, **more)
    return solver.solve_poly_batch(N, b["A"] if A is None else A, b["B"] if B is None else B, b["Q"], b["R"], P, Fu,
                                   b["x0"] if x0 is None else x0, want_plan=True, want_lam=True, **kw)


def same(got, want, keys=SOLVE_KEYS, pick=None):
    for k in keys:
        g, w = (got[k], want[k]) if pick is None else (got[k][..., pick], want[k][..., pick])
        assert np.array_equal(g, w), k


@pytest.mark.parametrize("name", REFERENCE_CASES)
def test_step_against_the_reference(solver, name):
    b, N, Fu, P, kw, hard, ref = problem(name)
    with controller(solver, name) as c:
        got = c.step(b["x0"], want_plan=True, want_lam=True)
        assert "poly_ctl_step" in solver.last_kernel()
    check(name + " (step)", got, ref, Fu, N)


@pytest.mark.parametrize("name", list(CASES))
def test_step_is_the_one_shot_call_bit_for_bit(solver, name):
    b, N = problem(name)[:2]
    (nx, nu), Bsz = b["B"].shape[:2], b["x0"].shape[1]
    want = one_shot(solver, name)
    with controller(solver, name) as c:
        got = c.step(b["x0"], want_plan=True, want_lam=True)
        assert "poly_ctl_step" in c.kernel and "poly_ctl_step" in solver.last_kernel()
        assert c.nbytes >= Bsz * _lib.lib().lqmpc_poly_controller_record_bytes(nx, nu, N)
    same(got, want)


def test_no_state_between_steps(solver):
    name = "c3-octagon-hard"
    b = problem(name)[0]
    xa, xb = b["x0"], np.ascontiguousarray(0.7 * b["x0"][:, ::-1])
    with controller(solver, name) as c:
        first = c.step(xa, want_plan=True, want_lam=True)
        second = c.step(xb, want_plan=True, want_lam=True)
        third = c.step(xa, want_plan=True, want_lam=True)
    same(first, third)
    same(second, one_shot(solver, name, x0=xb))
    assert not np.array_equal(first["u_0"], second["u_0"])


def test_caller_owned_loop(solver):
    """the states come from outside: here from the one-shot rollout, whose u_t every step must return bit for bit"""
    make, N, Fu, T, per = ROLLOUTS["c3-octagon-default"]
    b = make()
    roll = solver.rollout_poly_batch(T, N, b["A"], b["B"], b["Q"], b["R"], b["P"], Fu, b["x0"], b["A_true"], b["B_true"], want_traj=True)
    share = []
    with mpc.PolyBatchController(solver, N, b["A"], b["B"], b["Q"], b["R"], b["P"], Fu) as c:
        for t in range(T):
            x = np.ascontiguousarray(roll["X"][:, t])
            got = c.step(x)
            assert np.array_equal(got["u_0"], roll["U"][:, t]), t
            assert np.all(got["status"] == 0)
            share.append(np.mean(pr.reference(N, b["A"], b["B"], b["Q"], b["R"], b["P"], Fu, x)["nact"] > 0))
    print(f"caller-owned loop: constrained share per step {np.round(share, 2)}")
    assert share[0] >= 0.5 and min(share) < 0.25


@pytest.mark.parametrize("name", list(ROLLOUTS))
def test_rollout_is_the_one_shot_rollout_bit_for_bit(solver, name):
    make, N, Fu, T, per = ROLLOUTS[name]
    b = make()
    At, Bt = plant(b, per)
    want = solver.rollout_poly_batch(T, N, b["A"], b["B"], b["Q"], b["R"], b["P"], Fu, b["x0"], At, Bt, want_traj=True)
    with mpc.PolyBatchController(solver, N, b["A"], b["B"], b["Q"], b["R"], b["P"], Fu) as c:
        before = c.step(b["x0"], want_plan=True, want_lam=True)
        got = c.rollout(T, b["x0"], At, Bt, want_traj=True)
        assert "poly_ctl_rollout" in solver.last_kernel()
        after = c.step(b["x0"], want_plan=True, want_lam=True)
        short = c.rollout(T, b["x0"], At, Bt)
    same(got, want, ROLL_KEYS)
    same(before, after)
    assert np.array_equal(short["J_T"], want["J_T"]) and short["X"] is None
    assert np.all(want["status"] == 0)


def test_set_reference(solver):
    name = "c3-octagon-default"
    b = problem(name)[0]
    plain, with_refs = one_shot(solver, name), one_shot(solver, name, x_ref=XREF, u_ref=UREF)
    assert not np.array_equal(plain["u_0"], with_refs["u_0"])
    with controller(solver, name) as c:
        same(c.step(b["x0"], want_plan=True, want_lam=True), plain)
        c.set_reference(XREF, UREF)
        same(c.step(b["x0"], want_plan=True, want_lam=True), with_refs)
        c.set_reference(None, None)
        same(c.step(b["x0"], want_plan=True, want_lam=True), plain)
        assert c.reference_version == 2


def test_set_model(solver):
    name = "c3-octagon-default"
    b, N, Fu, P, kw, _, _ = problem(name)
    Bsz = 65
    A, B, x0 = (np.ascontiguousarray(b[k][..., :Bsz]) for k in ("A", "B", "x0"))
    rng = np.random.default_rng(11)
    idx = np.array([0, 5, 64])
    An = np.ascontiguousarray(A[..., idx] * (1.0 + 0.02 * rng.standard_normal((4, 4, 3))))
    Bn = np.ascontiguousarray(B[..., idx] * (1.0 + 0.02 * rng.standard_normal((4, 2, 3))))
    Am, Bm = A.copy(), B.copy()
    Am[..., idx], Bm[..., idx] = An, Bn
    rest = np.setdiff1d(np.arange(Bsz), idx)
    step = lambda c: c.step(x0, want_plan=True, want_lam=True)
    with mpc.PolyBatchController(solver, N, A, B, b["Q"], b["R"], P, Fu) as c:
        before = step(c)
        c.set_model(An, Bn, idx)
        assert "poly_ctl_factor" in solver.last_kernel()
        merged = step(c)
        same(merged, one_shot(solver, name, x0=x0, A=Am, B=Bm))
        same(merged, before, pick=rest)
        assert not np.array_equal(merged["u_0"][:, idx], before["u_0"][:, idx])
        c.set_model(An[..., :0], Bn[..., :0], [])                                          # count = 0: a no-op
        same(step(c), merged)
        c.set_model(A, B)                                                                  # idx=None replaces all
        same(step(c), before)
        assert c.model_version == 3
        # device flavour: the same update; then a list with an entry outside [0, Bsz), which must change nothing
        dA, dB, di = DevArray(An.shape, init=An), DevArray(Bn.shape, init=Bn), DevArray(3, np.int32, init=idx)
        c.set_model(dA, dB, di)
        same(step(c), merged)
        wild = np.ascontiguousarray(np.stack([An[..., 1], An[..., 0]], -1)), np.ascontiguousarray(np.stack([Bn[..., 1], Bn[..., 0]], -1))
        dA2, dB2 = DevArray(wild[0].shape, init=wild[0]), DevArray(wild[1].shape, init=wild[1])
        for bad in ([Bsz, -1], [1 << 30, -(1 << 30)]):
            dj = DevArray(2, np.int32, init=np.array(bad))
            c.set_model(dA2, dB2, dj)
            same(step(c), merged)
            solver.sync()
            dj.free()
        for d in (dA, dB, di, dA2, dB2):
            d.free()
        with pytest.raises(ValueError):
            c.set_model(An, Bn, [0, 5, 65])
        with pytest.raises(ValueError):
            c.set_model(An, Bn, [0, 5, 5])


@pytest.mark.parametrize("bsz", [1, 3, 65])
def test_batch_sizes(solver, bsz):
    b, N, Fu, P, kw, _, _ = problem("small-octagon")
    reps = -(-bsz // b["x0"].shape[1])
    A, B, x0 = (np.ascontiguousarray(np.tile(b[k], reps)[..., :bsz]) for k in ("A", "B", "x0"))
    want = solver.solve_poly_batch(N, A, B, b["Q"], b["R"], P, Fu, x0, want_plan=True, want_lam=True)
    with mpc.PolyBatchController(solver, N, A, B, b["Q"], b["R"], P, Fu) as c:
        same(c.step(x0, want_plan=True, want_lam=True), want)
        assert c.nbytes >= bsz * _lib.lib().lqmpc_poly_controller_record_bytes(*B.shape[:2], N) and c.Bsz == bsz


def test_max_iter_one(solver):
    name = "c3-octagon-default"
    b = problem(name)[0]
    want = one_shot(solver, name, max_iter=1)
    assert np.any(want["status"] == 1) and np.any(want["status"] == 0)
    with controller(solver, name, max_iter=1) as c:
        same(c.step(b["x0"], want_plan=True, want_lam=True), want)


def test_nan_in_one_model_and_in_one_state(solver):
    name = "c3-octagon-default"
    b, N, Fu, P, kw, _, _ = problem(name)
    clean = one_shot(solver, name)
    keep = np.arange(b["x0"].shape[1]) != 5
    A = b["A"].copy()
    A[1, 2, 5] = np.nan
    with mpc.PolyBatchController(solver, N, A, b["B"], b["Q"], b["R"], P, Fu) as c:
        got = c.step(b["x0"], want_plan=True, want_lam=True)
        assert got["status"][5] == 2
        same(got, clean, pick=keep)
        c.set_model(np.ascontiguousarray(b["A"][..., 5:6]), np.ascontiguousarray(b["B"][..., 5:6]), [5])
        same(c.step(b["x0"], want_plan=True, want_lam=True), clean)
    x = b["x0"].copy()
    x[2, 5] = np.nan
    with controller(solver, name) as c:
        got = c.step(x, want_plan=True, want_lam=True)
        assert got["status"][5] == 2
        same(got, clean, pick=keep)
        same(c.step(b["x0"], want_plan=True, want_lam=True), clean)                         # the next clean step is unaffected


def test_optional_outputs_and_the_device_flavour(solver):
    name = "c3-octagon-default"
    b, N, Fu, P, kw, _, _ = problem(name)
    full = one_shot(solver, name)
    nx, nu, Bsz, m = 4, 2, b["x0"].shape[1], Fu.shape[0]
    with controller(solver, name) as c:
        for plan, lam in ((False, False), (True, False), (False, True)):
            part = c.step(b["x0"], want_plan=plan, want_lam=lam)
            same(part, full, keys=list(part))
    dA, dB, dx = (DevArray(b[k].shape, init=b[k]) for k in ("A", "B", "x0"))
    outs = dict(u_0=DevArray((nu, Bsz)), V_N=DevArray(Bsz), U_plan=DevArray((nu, N, Bsz)), X_plan=DevArray((nx, N + 1, Bsz)),
                lam=DevArray((m, N, Bsz)), status=DevArray(Bsz, np.int32), iters=DevArray(Bsz, np.int32))
    with mpc.PolyBatchController(solver, N, dA, dB, b["Q"], b["R"], P, Fu) as c:
        c.step_dev(dx, *(outs[k] for k in ("u_0", "V_N", "U_plan", "X_plan", "lam", "status", "iters")))
        solver.sync()
        assert "poly_ctl_step" in solver.last_kernel()
        same({k: d.numpy() for k, d in outs.items()}, full)
        # every optional output left out in turn: the others keep their bits
        for hole in ("V_N", "U_plan", "X_plan", "lam", "status", "iters"):
            fresh = {k: DevArray(d.shape, d.dtype) for k, d in outs.items() if k != hole}
            c.step_dev(dx, *(fresh.get(k) for k in ("u_0", "V_N", "U_plan", "X_plan", "lam", "status", "iters")))
            solver.sync()
            same({k: d.numpy() for k, d in fresh.items()}, full, keys=list(fresh))
            for d in fresh.values():
                d.free()
        T = 4
        want = solver.rollout_poly_batch(T, N, b["A"], b["B"], b["Q"], b["R"], P, Fu, b["x0"], b["A_true"], b["B_true"], want_traj=True)
        dJ, dX, dU = DevArray(Bsz), DevArray((nx, T + 1, Bsz)), DevArray((nu, T, Bsz))
        c.rollout_dev(T, dx, b["A_true"], b["B_true"], dJ, dX, dU, outs["status"], outs["iters"])
        solver.sync()
        same(dict(J_T=dJ.numpy(), X=dX.numpy(), U=dU.numpy(), status=outs["status"].numpy(), iters=outs["iters"].numpy()), want, ROLL_KEYS)
    for d in (dA, dB, dx, dJ, dX, dU, *outs.values()):
        d.free()


def test_rollout_on_an_image_over_64_kib(solver):
    """n = 64 with a 16-gon: the factor's and the rollout's images are over 64 KiB, so both launches need the kernel's leave"""
    name = "n64-16gon-hard"
    b, N, Fu, P, kw, _, _ = problem(name)
    T = 2
    want = solver.rollout_poly_batch(T, N, b["A"], b["B"], b["Q"], b["R"], P, Fu, b["x0"], b["A_true"], b["B_true"], want_traj=True)
    with controller(solver, name) as c:
        same(c.rollout(T, b["x0"], b["A_true"], b["B_true"], want_traj=True), want, ROLL_KEYS)
