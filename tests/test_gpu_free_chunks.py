"""GPU (-m gpu): the speculative chunks of iteration-free steps in the closed loop of the 16-lane-row kernels (lqmpc_r16_body.h).

A rollout WITHOUT trajectories takes up to FREE_KMAX iteration-free steps at a time, with one test of the box behind them, and goes
back to the single step when the test fails; a rollout WITH trajectories (want_traj=True) runs the single step only -- the loop as it
was before the chunks.  A committed chunk issues the FMAs of the single steps in their order, so the two must agree BIT FOR BIT in
J_T, status and iters; both are also held to the oracle with the bars of tests/test_gpu_parity.py (RTOL, TIGHT).

The chunks are in the C3 and C4 rollout kernels of the throughput build only (R16Build::CHUNKS; r16_build = 0 at C3).  The other cases
below -- the latency build, C2, (2,1,20), the run-time compiled shape, the fused sweep, the controller's rollout -- run kernels without
them: there the comparison is a control (the single-step loop with and without its stores), kept so that it holds unchanged the day
one of those kernels gets the chunks.
"""
import os
import re

import numpy as np
import pytest

from lq_mpc_amd import BatchController, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

RTOL = 1e-5
TIGHT = 1e-8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "lq_mpc_amd", "csrc", "lqmpc_r16_body.h")) as _f:
    KMAX = int(re.search(r"constexpr int FREE_KMAX = (\d+);", _f.read()).group(1))
STEPS = sorted({1, 2, 3, KMAX - 1, KMAX, KMAX + 1, 2 * KMAX + 1, 30})
_cache = {}


def rel(a, b):
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))


def qa(b):
    return (b["N"], b["A"], b["B"], b["Q"], b["R"], b["P"], b["lb"], b["ub"])


@pytest.fixture
def opts(solver):
    def set_(**kw):
        solver.set_options(**kw)
    yield set_
    solver.set_options(order=-1, r16_build=-1, r16_maxit=12)


def batch(name):
    """the batches of test 1, made once: C3, C2, C4 as the seeded generator draws them, C3's models with a horizon of 12 (a shape
    without a prebuilt kernel: compiled at run time) and C2's models with a horizon of 20 (two states, n > 10, both builds)"""
    if name not in _cache:
        golden = os.path.join(ROOT, "tests", "golden")
        if name == "C3":
            b = synth.make_batch(3, Bsz=515)
        elif name == "C2":
            b = synth.make_batch(2, Bsz=515, fixture_dir=golden)
        elif name == "C4":
            b = synth.make_batch(4, Bsz=259)
        elif name == "N20":
            b = dict(synth.make_batch(2, Bsz=515, fixture_dir=golden), N=20)
        else:
            b = dict(synth.make_batch(3, Bsz=515), N=12)
        _cache[name] = b
    return _cache[name]


def oracle(name, T):
    if (name, T) not in _cache:
        b = batch(name)
        _cache[(name, T)] = orc.rollout_batch(T, *qa(b), b["x0"], b["A_true"], b["B_true"])
    return _cache[(name, T)]


def assert_same(chunked, stepwise, tag):
    for k in ("J_T", "status", "iters"):
        assert np.array_equal(chunked[k], stepwise[k]), (tag, k, np.flatnonzero(chunked[k] != stepwise[k])[:8])


# ---------------- 1. chunked equals stepwise, bit for bit ----------------
CASES = [("C3", 1, -1, "lqmpc_r16_kernel<4,2,10>"), ("C3", 0, -1, "lqmpc_r16_kernel<4,2,10>"), ("C3", 0, 1, "lqmpc_r16_kernel<4,2,10>"),
         ("C2", -1, -1, "lqmpc_r16_kernel<2,1,10>"), ("C4", -1, -1, "lqmpc_r64_kernel<4,2,20>"), ("jit", -1, -1, "<4,2,12>"),
         ("N20", 1, -1, "lqmpc_r16_kernel<2,1,20>"), ("N20", 0, -1, "lqmpc_r16_kernel<2,1,20>")]


@pytest.mark.parametrize("name,build,order,kernel", CASES, ids=[f"{c[0]}-build{c[1]}-order{c[2]}" for c in CASES])
def test_chunked_rollout_equals_the_stepwise_loop(solver, opts, name, build, order, kernel):
    """Every horizon length around the chunk length: T = 1 (no chunk: at least two steps must remain), 2 and 3 (a chunk shorter than
    FREE_KMAX, bounded by T), FREE_KMAX +- 1 and 2 FREE_KMAX + 1 (a full chunk with nothing, one step or a second chunk behind it), 30."""
    b = batch(name)
    opts(r16_build=build, order=order)
    for T in STEPS:
        chunked = solver.rollout_batch(T, *qa(b), b["x0"], b["A_true"], b["B_true"])
        k1 = solver.last_kernel()
        stepwise = solver.rollout_batch(T, *qa(b), b["x0"], b["A_true"], b["B_true"], want_traj=True)
        assert kernel in k1 and kernel in solver.last_kernel(), (k1, solver.last_kernel())
        assert ("jit" in k1) == (name == "jit")
        assert_same(chunked, stepwise, (name, T))
        ref = oracle(name, T)
        assert np.all(chunked["status"] == 0)
        e = rel(chunked["J_T"], ref["J_T"])
        print(f"{name} build {build} order {order} T {T}: J_T relerr {e:.2e}, iters {int(chunked['iters'].sum())}")
        assert e < RTOL and e < TIGHT


# ---------------- 2. a step outside the box at every position of a chunk ----------------
def ladder():
    """C3's models on a plant whose closed loop grows (A_true = 1.6 A0: spectral radius 1.16 with the LQR gain), from states along the
    growing mode on a geometric ladder below the box: an instance starts iteration-free and meets its first constrained QP one step
    later per rung.  First half: the four instances of a wavefront share a rung.  Second half: one instance of the wavefront is on the
    rung and the other three start at 1e-9 and never leave the box."""
    if "ladder" not in _cache:
        T, Bsz, rungs = 30, 1024, 32
        b = synth.make_batch(3, Bsz=Bsz)
        A0, B0 = b["A_true"], b["B_true"]
        K = synth._dlqr_gain(A0, B0, b["Q"], b["R"])
        At = 1.6 * A0
        w, V = np.linalg.eig(At - B0 @ K)
        k = int(np.argmax(np.abs(w)))
        rho, d = abs(w[k]), np.real(V[:, k]) / np.linalg.norm(np.real(V[:, k]))
        j = np.arange(Bsz)
        scale = 0.9 * synth.U_MAX / np.max(np.abs(K @ d)) * rho ** (-(j // 4 % rungs).astype(float))
        x0 = d[:, None] * scale[None, :]
        lone = (j >= Bsz // 2) & (j % 4 != (j // 4) % 4)
        x0[:, lone] = d[:, None] * 1e-9
        b = dict(b, A_true=At, B_true=B0, x0=np.ascontiguousarray(x0))
        ref = orc.rollout_batch(T, *qa(b), b["x0"], b["A_true"], b["B_true"], want_traj=True)
        # first constrained step of every instance (T: none), by the criterion of synth.constrained_share: the unconstrained minimiser
        # of the QP at the oracle's state is outside the box
        lb, ub = np.tile(b["lb"], b["N"])[:, None], np.tile(b["ub"], b["N"])[:, None]
        first = np.full(Bsz, T)
        for i in range(Bsz):
            H, F = synth.condense_np(b["A"][:, :, i], b["B"][:, :, i], b["Q"], b["R"], b["P"], b["N"])
            v = -np.linalg.solve(H, F @ ref["X"][:, :-1, i])
            c = ((v < lb) | (v > ub)).any(axis=0)
            if c.any():
                first[i] = int(np.argmax(c))
        _cache["ladder"] = (b, ref, first, T)
    return _cache["ladder"]


@pytest.mark.parametrize("build", [1, 0])
def test_a_step_outside_the_box_at_every_position_of_a_chunk(solver, opts, build):
    """Natural order (order = 0), so that instances 4w .. 4w+3 share wavefront w.  A wavefront whose step 0 is iteration-free starts
    its chunks at steps 1, 1 + FREE_KMAX, ...: its first constrained step f (the earliest of its four instances) falls on position
    (f - 1) % FREE_KMAX of a chunk, which is then discarded.  The coverage is asserted from the oracle's trajectories."""
    b, ref, first, T = ladder()
    w = first.reshape(-1, 4)
    f = w.min(axis=1)
    leaves = (f >= 2) & (f < T)                                   # starts iteration-free, leaves the box later
    assert set(((f[leaves] - 1) % KMAX).tolist()) == set(range(KMAX))
    alone = leaves & (np.sort(w, axis=1)[:, 1] == T)              # exactly one of the four leaves, the other three never do
    assert set(((f[alone] - 1) % KMAX).tolist()) == set(range(KMAX))
    assert (f == T).any()                                         # and wavefronts that never leave
    opts(r16_build=build, order=0)
    chunked = solver.rollout_batch(T, *qa(b), b["x0"], b["A_true"], b["B_true"])
    assert "lqmpc_r16_kernel<4,2,10>" in solver.last_kernel()
    stepwise = solver.rollout_batch(T, *qa(b), b["x0"], b["A_true"], b["B_true"], want_traj=True)
    assert_same(chunked, stepwise, ("ladder", build))
    assert np.all(chunked["status"] == 0)
    e = rel(chunked["J_T"], ref["J_T"])
    print(f"ladder build {build}: J_T relerr {e:.2e}, {int(leaves.sum())} wavefronts leave the box, {int(alone.sum())} with one instance")
    assert e < RTOL and e < TIGHT
    assert (chunked["iters"][first < T] > 0).all() and (chunked["iters"][first == T] == 0).all()


# ---------------- 3. the fused sweep and the prepared controller's rollout ----------------
def test_sweep_and_controller_rollout_equal_their_stepwise_parts(solver, opts):
    b, T = batch("C3"), 2 * KMAX + 1
    ref = oracle("C3", T)
    x0s = np.ascontiguousarray(1.5 * b["x0"][:, :6])
    mv = orc.max_vn_batch(*qa(b), x0s)
    for build in (1, 0):
        opts(r16_build=build)
        g = solver.sweep_batch(T, *qa(b), b["x0"], x0s, b["A_true"], b["B_true"])
        assert "r16" in solver.last_kernel()
        m2 = solver.max_vn_batch(*qa(b), x0s)
        r2 = solver.rollout_batch(T, *qa(b), b["x0"], b["A_true"], b["B_true"], want_traj=True)      # (the single steps)
        assert np.all(g["status"] == 0)
        assert rel(g["M_V"], mv) < TIGHT and rel(g["J_T"], ref["J_T"]) < TIGHT
        assert np.array_equal(g["M_V"], m2["M_V"]) and np.array_equal(g["J_T"], r2["J_T"])
        assert np.array_equal(g["iters"], m2["iters"] + r2["iters"])
    opts(r16_build=-1)
    with BatchController(solver, *qa(b)) as ctl:
        for plant in ((b["A_true"], b["B_true"]), (b["A"], b["B"])):
            chunked = ctl.rollout(T, b["x0"], *plant)
            assert "ctl" in solver.last_kernel() and "roll" in solver.last_kernel()
            stepwise = ctl.rollout(T, b["x0"], *plant, want_traj=True)
            assert_same(chunked, stepwise, "controller")
            assert np.all(chunked["status"] == 0)
            want = ref if plant[0].ndim == 2 else orc.rollout_batch(T, *qa(b), b["x0"], b["A"], b["B"])
            assert rel(chunked["J_T"], want["J_T"]) < RTOL


# ---------------- 4. a NaN inside a chunk ----------------
def test_nan_in_one_model_inside_a_chunk(solver, opts):
    """Iteration-free instances only (x0 scaled to 1e-3), one of them with a NaN in its model: status 2 there as on the single-step
    path, and its three wavefront neighbours -- whose chunks are all discarded, the NaN counts as outside -- bit-equal to the batch
    without it."""
    b = batch("C3")
    T, bad = 30, 9
    x0 = np.ascontiguousarray(1e-3 * b["x0"])
    A2 = b["A"].copy()
    A2[1, 2, bad] = np.nan
    keep = np.arange(b["Bsz"]) != bad
    for build in (1, 0):
        opts(r16_build=build, order=0)
        good = solver.rollout_batch(T, *qa(b), x0, b["A_true"], b["B_true"])
        assert np.all(good["status"] == 0) and np.all(good["iters"] == 0)
        got = solver.rollout_batch(T, *qa(dict(b, A=A2)), x0, b["A_true"], b["B_true"])
        stepwise = solver.rollout_batch(T, *qa(dict(b, A=A2)), x0, b["A_true"], b["B_true"], want_traj=True)
        assert got["status"][bad] == 2 and stepwise["status"][bad] == 2, (got["status"][bad], stepwise["status"][bad])
        assert np.array_equal(got["status"], stepwise["status"]) and np.array_equal(got["iters"][keep], stepwise["iters"][keep])
        assert np.all(got["status"][keep] == 0)
        assert np.array_equal(got["J_T"][keep], good["J_T"][keep])
        assert np.array_equal(got["J_T"][keep], stepwise["J_T"][keep])
        # ... and in its PLANT (one per instance): step 0 is iteration-free everywhere, the state of the instance is a NaN from step 1
        # on, which the first chunk of its wavefront meets at its first position
        At = np.ascontiguousarray(np.repeat(b["A_true"][:, :, None], b["Bsz"], 2))
        Bt = np.ascontiguousarray(np.repeat(b["B_true"][:, :, None], b["Bsz"], 2))
        good = solver.rollout_batch(T, *qa(b), x0, At, Bt)
        At2 = At.copy()
        At2[1, 2, bad] = np.nan
        got = solver.rollout_batch(T, *qa(b), x0, At2, Bt)
        stepwise = solver.rollout_batch(T, *qa(b), x0, At2, Bt, want_traj=True)
        assert np.array_equal(got["status"], stepwise["status"]) and np.array_equal(got["iters"][keep], stepwise["iters"][keep])
        assert got["status"][bad] != 0 and np.all(got["status"][keep] == 0)
        assert np.array_equal(got["J_T"][keep], good["J_T"][keep])
        assert np.array_equal(got["J_T"][keep], stepwise["J_T"][keep])
