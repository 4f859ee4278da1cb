"""GPU (-m gpu): the prepared batch controller with records on the workgroup kernel's shapes (options.ctl_wg = 1) against the fp64 oracle.

Helpers, the bar (1e-10 relative on V_N, 1e-10 * max(|u*|, h) on u_0, status 0) and assert_mixed are those of tests/test_gpu_controller.py.
Shapes, each the smallest case of something:
    (9,5,7)    n = 35   three blocks, the last one partial, n_x > 8
    (6,2,33)   n = 66   inside the 16-lane-row family's n_x / n_u limits, but n > 48
    (10,3,24)  n = 72   five blocks, the last one half filled, run-time dimensions
    (8,4,30)   n = 120  the compile-time copy of the set-up
"""
import numpy as np
import pytest

from test_gpu_controller import BAR, DevArray, assert_mixed, check, controller, dev_step, head, oracle_at, plant_data, problem, qa, rel, u_err
from lq_mpc_amd import BatchController, LqmpcError, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

SHAPES = {(9, 5, 7): 203, (6, 2, 33): 48, (10, 3, 24): 64, (8, 4, 30): 64}
STEP_KERNEL = "lqmpc_wg_ctl_step_kernel"
_cache = {}


def case(shape, Bsz=None, seed=1, **kw):
    """problem() and the oracle's answer at its x0, computed once per (shape, size, seed, box) and never modified"""
    key = (shape, Bsz or SHAPES[shape], seed, tuple(sorted(kw.items())))
    if key not in _cache:
        p = problem(*shape, key[1], seed, **kw)
        _cache[key] = (p, oracle_at(p, p["x0"]))
    return _cache[key]


def record_bytes(shape):
    nx, nu, N = shape
    n = N * nu
    nb = (n + 15) // 16
    img = nb * (nb + 1) // 2 * 16 * 17
    return 8 * (nx * nx + nx * nu + 16 * nb * nx + 16 * nb + 2 * img)


@pytest.fixture
def wg(solver):
    def set_(**kw):
        solver.set_options(**kw)
    set_(ctl_wg=1)
    yield set_
    solver.set_options(ctl_wg=0, max_iter=50)


# ---------------- 1. one step equals a solve ----------------
@pytest.mark.parametrize("shape", list(SHAPES), ids=str)
def test_one_step_equals_a_solve(solver, wg, shape):
    full, ref_full = case(shape)
    assert_mixed(full, ref_full)
    for Bsz in ([1, 5, SHAPES[shape]] if shape == (9, 5, 7) else [SHAPES[shape]]):
        p = head(full, Bsz)
        ref = {k: ref_full[k][..., :Bsz] for k in ("u_0", "V_N")}
        with controller(solver, p) as ctl:
            assert ctl.kernel == STEP_KERNEL and "ctl" in ctl.kernel
            got = ctl.step(p["x0"])
            check(p, got, ref, f"{shape} x{Bsz} host")
            assert solver.last_kernel() == ctl.kernel
            assert ctl.nbytes >= record_bytes(shape) * Bsz
        dA, dB = DevArray(p["A"].shape, init=p["A"]), DevArray(p["B"].shape, init=p["B"])
        with BatchController(solver, p["N"], dA, dB, p["Q"], p["R"], p["P"], p["lb"], p["ub"]) as ctl:
            assert ctl.kernel == STEP_KERNEL
            check(p, dev_step(solver, ctl, p, p["x0"]), ref, f"{shape} x{Bsz} dev")
            ctl.reset()
            bare = dev_step(solver, ctl, p, p["x0"], outputs=False)
            assert u_err(bare["u_0"], ref["u_0"], 0.5 * (p["ub"] - p["lb"])) <= BAR


def test_ctl_wg_takes_0_or_1(solver, wg):
    for bad in (2, -1):
        with pytest.raises(LqmpcError):
            solver.set_options(ctl_wg=bad)
    assert solver.get_options()["ctl_wg"] == 1


# ---------------- 2. the default is unchanged ----------------
@pytest.mark.parametrize("shape", list(SHAPES), ids=str)
def test_default_is_the_pass_through(solver, wg, shape):
    p, ref = case(shape)
    wg(ctl_wg=0)
    with controller(solver, p) as ctl:
        check(p, ctl.step(p["x0"]), ref, f"{shape} ctl_wg=0")
        assert ctl.kernel == "lqmpc_wg_kernel" and solver.last_kernel() == ctl.kernel
    # neither do option sets under which lqmpc_solve_batch leaves the workgroup kernel's warm-started path keep records
    wg(ctl_wg=1, warm_start=0)
    try:
        with controller(solver, head(p, 5)) as ctl:
            assert "ctl" not in ctl.kernel
    finally:
        wg(warm_start=-1)


# ---------------- 3. the carried face never decides ----------------
@pytest.mark.parametrize("shape", [(9, 5, 7), (8, 4, 30)], ids=str)
def test_carried_face_never_decides(solver, wg, shape):
    p, ref = case(shape)
    Bsz = SHAPES[shape]
    assert_mixed(p, ref)
    with controller(solver, p) as ctl:
        assert ctl.kernel == STEP_KERNEL
        first = ctl.step(p["x0"])
        check(p, first, ref, "first")
        second = ctl.step(p["x0"])                          # (a) the same state again: the face stays where it is
        check(p, second, ref, "second")
        print("iters first / second:", first["iters"].sum(), second["iters"].sum())
        assert np.all(second["iters"] <= first["iters"]), np.flatnonzero(second["iters"] > first["iters"])[:10]
        ctl.reset()                                         # (b) cold again: bit-equal to the very first call
        again = ctl.step(p["x0"])
        for k in ("u_0", "V_N", "status", "iters"):
            assert np.array_equal(again[k], first[k]), k
        xm = -3.0 * p["x0"]                                 # (c) far away, then somewhere new
        check(p, ctl.step(xm), oracle_at(p, xm), "-3x")
        xr = problem(*shape, Bsz, 7)["x0"]
        check(p, ctl.step(xr), oracle_at(p, xr), "fresh")
        ctl.step(p["x0"])                                   # (d) one NaN state
        xn = p["x0"].copy()
        bad = 6
        xn[0, bad] = np.nan
        g = ctl.step(xn)
        assert g["status"][bad] == 2
        keep = np.arange(Bsz) != bad
        assert np.all(g["status"][keep] == 0)
        h = 0.5 * (p["ub"] - p["lb"])
        assert rel(g["V_N"][keep], ref["V_N"][keep]) <= BAR and u_err(g["u_0"][:, keep], ref["u_0"][:, keep], h) <= BAR
        check(p, ctl.step(p["x0"]), ref, "after NaN")


# ---------------- 4. a moving loop ----------------
@pytest.mark.parametrize("shape", [(9, 5, 7), (8, 4, 30), (10, 3, 24)], ids=str)
def test_a_moving_loop(solver, wg, shape):
    """8 steps around a perturbed plant with noise, on the host between the calls; every step against the oracle at the GPU's own
    state, so nothing compounds.  The face a step ends on is the next one's guess, shifted by a stage."""
    T, Bsz = 8, 64
    p = problem(*shape, Bsz, 3)
    A_true, B_true, W = plant_data(p, T)
    h = 0.5 * (p["ub"] - p["lb"])
    x = p["x0"].copy()
    sat = inside = 0
    with controller(solver, p) as ctl:
        assert ctl.kernel == STEP_KERNEL
        for t in range(T):
            got = ctl.step(x)
            r = oracle_at(p, x)
            check(p, got, r, f"{shape} t={t}")
            v = np.abs(r["u_0"])
            sat += np.any(v >= h[:, None] * (1 - 1e-9), axis=0).sum()
            inside += np.all(v < h[:, None] * (1 - 1e-6), axis=0).sum()
            x = np.einsum("abi,bi->ai", A_true, x) + np.einsum("aki,ki->ai", B_true, got["u_0"]) + W[t]
    print(f"{shape}: on the bound {sat / (T * Bsz):.2f}, inside {inside / (T * Bsz):.2f}")
    assert sat >= 0.25 * T * Bsz and inside >= 0.25 * T * Bsz, (sat, inside)


# ---------------- 5. linear term ----------------
def test_references_and_off_centre_box(solver, wg):
    shape = (9, 5, 7)
    nx, nu, N = shape
    p = dict(case(shape, lb=-0.2, ub=0.5)[0])
    rng = np.random.default_rng(5)
    p["x_ref"] = 0.1 * rng.standard_normal((nx, N))
    p["u_ref"] = 0.05 * rng.standard_normal((nu, N))
    ref = oracle_at(p, p["x0"])
    assert_mixed(p, ref)
    with controller(solver, p) as ctl:
        assert ctl.kernel == STEP_KERNEL
        check(p, ctl.step(p["x0"]), ref, "refs")
        x2 = problem(nx, nu, N, 203, 9)["x0"]
        check(p, ctl.step(x2), oracle_at(p, x2), "refs, second state")
        check(p, ctl.step(p["x0"]), ref, "refs, back")


# ---------------- 6. forced fall-back ----------------
def test_fall_back_inside_the_step(solver, wg):
    """The workgroup kernel leaves the warm-started active-set iterations for the interior-point method when the active set outgrows
    its workspace: at (8,4,30) that is more than 80 of the 120 rows, which states far outside the region where the box is inactive
    reach at once.  With max_iter = 1 the interior point cannot finish: the instances that end with status 1 in lqmpc_solve_batch end
    with status 1 in a step, with the same answer."""
    shape = (8, 4, 30)
    p, _ = case(shape)
    x = 1e4 * p["x0"]
    wg(max_iter=1)
    want = solver.solve_batch(*qa(p), x)
    assert solver.last_kernel() == "lqmpc_wg_kernel"
    with controller(solver, p) as ctl:
        wg(max_iter=50)                                     # the controller keeps the options it was made under
        assert ctl.kernel == STEP_KERNEL
        got = ctl.step(x)
    print("status 1:", int((want["status"] == 1).sum()), "of", want["status"].size)
    assert (want["status"] == 1).any() and np.all(want["status"] <= 1)
    h = 0.5 * (p["ub"] - p["lb"])
    assert np.array_equal(got["status"], want["status"])
    assert u_err(got["u_0"], want["u_0"], h) <= BAR and rel(got["V_N"], want["V_N"]) <= BAR


# ---------------- 7. life cycle ----------------
@pytest.mark.parametrize("order", [0, 1])
def test_life_cycle(solver, wg, order):
    (pa, ra), pb = case((9, 5, 7)), problem(4, 2, 10, 203, 1)
    rb = oracle_at(pb, pb["x0"])
    Aa, Ba = pa["A"].copy(), pa["B"].copy()
    ca = BatchController(solver, pa["N"], Aa, Ba, pa["Q"], pa["R"], pa["P"], pa["lb"], pa["ub"])
    Aa[:] = np.nan                                          # the controller has copied what it needs
    Ba[:] = np.nan
    cb = controller(solver, pb)
    assert ca.kernel == STEP_KERNEL and "ctl_r16" in cb.kernel
    per = ca.nbytes / 203
    assert record_bytes((9, 5, 7)) <= per <= record_bytes((9, 5, 7)) + 1024, per
    roll_ref = orc.rollout_batch(5, *qa(pa), pa["x0"], pa["A"], pa["B"])
    for k in range(2):
        check(pa, ca.step(pa["x0"]), ra, f"a{k}")
        check(pb, solver.solve_batch(*qa(pb), pb["x0"]), rb, f"solve b{k}")
        check(pb, cb.step(pb["x0"]), rb, f"b{k}")
        got = solver.rollout_batch(5, *qa(pa), pa["x0"], pa["A"], pa["B"])
        assert np.all(got["status"] == 0) and rel(got["J_T"], roll_ref["J_T"]) <= BAR
        check(pa, solver.solve_batch(*qa(pa), pa["x0"]), ra, f"solve a{k}")
    for c in ((ca, cb) if order == 0 else (cb, ca)):
        c.close()
    check(pa, solver.solve_batch(*qa(pa), pa["x0"]), ra, "after close")


# ---------------- 8. it has to pay ----------------
def test_a_step_is_cheaper_than_a_solve(solver, wg):
    """(8,4,30) x 2 048.  lqmpc_solve_batch_dev on the same handle is what a step costs without records (the pass-through is that call)."""
    b = synth.make_batch(5, Bsz=2048)
    nx, nu, Bsz = b["B"].shape
    N = b["N"]
    assert (nx, nu, N, Bsz) == (8, 4, 30, 2048)
    dA, dB, dx = (DevArray(b[k].shape, init=b[k]) for k in ("A", "B", "x0"))
    du, dv = DevArray((nu, Bsz)), DevArray(Bsz)
    solver.reserve(nx, nu, N, Bsz)
    with BatchController(solver, N, dA, dB, b["Q"], b["R"], b["P"], b["lb"], b["ub"]) as ctl:
        assert ctl.kernel == STEP_KERNEL

        def t_solve():
            solver.timer_begin()
            for _ in range(20):
                solver.solve_batch_dev(nx, nu, N, Bsz, dA, dB, b["Q"], b["R"], b["P"], b["lb"], b["ub"], dx, du, dv)
            return solver.timer_end() / 20

        def t_step(cold):
            solver.timer_begin()
            for _ in range(20):
                if cold:
                    ctl.reset()
                ctl.step_dev(dx, du, dv)
            return solver.timer_end() / 20

        for _ in range(3):
            t_solve(); t_step(True); t_step(False)
        rounds = [(t_solve(), t_step(True), t_step(False)) for _ in range(5)]
        ts, tc, tw = (float(np.median([r[k] for r in rounds])) for k in range(3))
        print(f"per call, ms: solve {ts:.4f}  step after reset {tc:.4f} (includes the reset's fill)  repeated step {tw:.4f}  "
              f"solve / repeated step {ts / tw:.2f}  bytes/instance {ctl.nbytes / Bsz:.0f}")
        assert tc < ts, (tc, ts)
        assert tw < ts, (tw, ts)
