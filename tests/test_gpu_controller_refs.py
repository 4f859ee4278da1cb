"""GPU (-m gpu): new references for a prepared controller (BatchController.set_reference / lqmpc_controller_set_reference) against
the fp64 oracle at the same states and references.

Inputs, helpers and bars are those of tests/test_gpu_controller.py: problem(nx, nu, N, 203, seed 1), 1e-10 relative on V_N,
1e-10 * max(|u*|, h) on u_0, status 0.  References: default_rng(5), x_ref = 0.1 randn, u_ref = 0.05 randn (R1; R2 is the next draw).
Every parity test first asserts, from the ORACLE alone, that at least a quarter of the instances have a saturated first move and
at least a quarter a strictly interior one, and that the references move u_0 of at least half of the instances by more than 1e-6
against the zero-reference answer -- a set_reference that does nothing fails.
Shapes: records with one, two and three row slots, nu = 3, n = 48, prebuilt and run-time compiled kernels; workgroup records
(ctl_wg = 1) with a partial last block (n = 52) and with n_x > 8; the pass-through.
"""
import numpy as np
import pytest

from test_gpu_controller import BAR, DevArray, assert_mixed, check, dev_step, oracle_at, problem, qa
from lq_mpc_amd import BatchController, LqmpcError, synth

pytestmark = pytest.mark.gpu

RECORDS = [(2, 1, 10), (4, 2, 10), (4, 2, 20), (3, 2, 6), (7, 3, 11), (8, 4, 12)]
WG = [(8, 4, 13), (12, 2, 20)]
PASS_THROUGH = [(9, 5, 7), (8, 4, 30)]
ALL = RECORDS + WG + PASS_THROUGH
CENTRED, OFF_CENTRE = (-0.3, 0.3), (-0.2, 0.5)
BSZ, SEED = 203, 1
_cache = {}


def refs(shape, cols=None):
    """R1 and R2, (x_ref, u_ref) each; with cols: one trajectory of that many columns"""
    nx, nu, N = shape
    rng = np.random.default_rng(5)
    if cols:
        return 0.1 * rng.standard_normal((nx, cols)), 0.05 * rng.standard_normal((nu, cols))
    return [(0.1 * rng.standard_normal((nx, N)), 0.05 * rng.standard_normal((nu, N))) for _ in range(2)]


def variants(shape):
    (x1, u1), (x2, u2) = refs(shape)
    return {"R1": (x1, u1), "R2": (x2, u2), "x only": (x1, None), "u only": (None, u1), "none": (None, None)}


def base(shape, box):
    key = (shape, box)
    if key not in _cache:
        _cache[key] = problem(*shape, BSZ, SEED, lb=box[0], ub=box[1])
    return _cache[key]


def case(shape, box, tag):
    """the problem with the references `tag` and the oracle's answer at its x0: computed once, never modified"""
    key = (shape, box, tag)
    if key not in _cache:
        xr, ur = variants(shape)[tag]
        p = dict(base(shape, box), x_ref=xr, u_ref=ur)
        _cache[key] = (p, oracle_at(p, p["x0"]))
    return _cache[key]


def assert_conditions(p, ref, ref0, sat_min=0.25):
    """From the oracle alone: both halves of a step are exercised, and the references matter."""
    h = 0.5 * (p["ub"] - p["lb"])[:, None]
    v = np.abs(ref["u_0"] - 0.5 * (p["ub"] + p["lb"])[:, None])
    sat = np.any(v >= h * (1 - 1e-9), axis=0).mean()
    inside = np.all(v < h * (1 - 1e-6), axis=0).mean()
    moved = np.any(np.abs(ref["u_0"] - ref0["u_0"]) > 1e-6, axis=0).mean()
    print(f"saturated {sat:.2f} interior {inside:.2f} moved by the references {moved:.2f}")
    assert sat >= sat_min and inside >= 0.25 and moved >= 0.5, (sat, inside, moved)


@pytest.fixture
def mode(solver):
    """the options a shape's controller is made under: ctl_wg = 1 for the workgroup records"""
    def set_(shape=None, **kw):
        solver.set_options(ctl_wg=1 if shape in WG else 0, **kw)
    yield set_
    solver.set_options(ctl_wg=0, r16_maxit=12)


def make(solver, shape, p):
    """a controller made WITHOUT references, of the kind the shape is listed under"""
    ctl = BatchController(solver, *qa(p))
    if shape in RECORDS:
        assert "ctl" in ctl.kernel and "wg" not in ctl.kernel, ctl.kernel
    elif shape in WG:
        assert ctl.kernel == "lqmpc_wg_ctl_step_kernel", ctl.kernel
    else:
        assert "ctl" not in ctl.kernel, ctl.kernel
    return ctl


# ---------------- 1. every step after set_reference is the oracle's with those references ----------------
@pytest.mark.parametrize("shape", ALL, ids=str)
def test_set_reference_then_step(solver, mode, shape):
    mode(shape)
    p0, ref0 = case(shape, CENTRED, "none")
    assert_conditions(*case(shape, CENTRED, "R1"), ref0)
    with make(solver, shape, p0) as ctl:
        for tag, (xr, ur) in variants(shape).items():
            p, ref = case(shape, CENTRED, tag)
            if tag == "none":
                ctl.set_reference()
            else:
                assert_mixed(p, ref)
                ctl.set_reference(xr, ur)
            check(p, ctl.step(p["x0"]), ref, f"{shape} {tag}, stored face")
            ctl.reset()
            check(p, ctl.step(p["x0"]), ref, f"{shape} {tag}, after reset")


# ---------------- 2. the centre of the box stays in v_r ----------------
@pytest.mark.parametrize("shape", ALL, ids=str)
def test_off_centre_box(solver, mode, shape):
    mode(shape)
    p0, ref0 = case(shape, OFF_CENTRE, "none")
    p, ref = case(shape, OFF_CENTRE, "R1")
    assert_conditions(p, ref, ref0)
    with make(solver, shape, p0) as ctl:
        check(p0, ctl.step(p0["x0"]), ref0, f"{shape} before")
        ctl.set_reference(p["x_ref"], p["u_ref"])
        check(p, ctl.step(p["x0"]), ref, f"{shape} R1")
        ctl.set_reference()
        check(p0, ctl.step(p0["x0"]), ref0, f"{shape} none again")


# ---------------- 3. ordered with the steps, and the arrays are the caller's again at once ----------------
@pytest.mark.parametrize("shape", ALL, ids=str)
def test_no_sync_needed_and_arrays_are_copied(solver, mode, shape):
    mode(shape)
    p0, ref0 = case(shape, CENTRED, "none")
    p, ref = case(shape, CENTRED, "R1")
    assert_conditions(p, ref, ref0)
    with make(solver, shape, p0) as ctl:
        ctl.step(p0["x0"])
        xr, ur = p["x_ref"].copy(), p["u_ref"].copy()
        ctl.set_reference(xr, ur)
        xr[:] = np.nan
        ur[:] = np.nan
        check(p, dev_step(solver, ctl, p, p["x0"]), ref, f"{shape} step_dev right behind set_reference")


# ---------------- 4. other calls on the handle in between ----------------
@pytest.mark.parametrize("shape", ALL, ids=str)
def test_a_solve_with_other_references_in_between(solver, mode, shape):
    mode(shape)
    p0, ref0 = case(shape, CENTRED, "none")
    p1, ref1 = case(shape, CENTRED, "R1")
    p2, ref2 = case(shape, CENTRED, "R2")
    assert_conditions(p1, ref1, ref0)
    with make(solver, shape, p0) as ctl:
        ctl.set_reference(p1["x_ref"], p1["u_ref"])
        check(p2, solver.solve_batch(*qa(p2), p2["x0"], p2["x_ref"], p2["u_ref"]), ref2, f"{shape} solve with R2")
        check(p1, ctl.step(p1["x0"]), ref1, f"{shape} step with R1")
        check(p0, solver.solve_batch(*qa(p0), p0["x0"]), ref0, f"{shape} solve without")
        check(p1, ctl.step(p1["x0"]), ref1, f"{shape} step with R1 again")


# ---------------- 5. the hand-back kernels see the new references ----------------
def test_hand_back_after_set_reference(solver, mode):
    shape = (4, 2, 10)
    p0, ref0 = case(shape, CENTRED, "none")
    p, ref = case(shape, CENTRED, "R1")
    assert_conditions(p, ref, ref0)
    mode(shape, r16_maxit=0)
    ctl = make(solver, shape, p0)
    mode(shape, r16_maxit=12)                               # the controller keeps the options it was made under
    with ctl:
        ctl.set_reference(p["x_ref"], p["u_ref"])
        check(p, ctl.step(p["x0"]), ref, "maxit=0, R1")
        check(p, dev_step(solver, ctl, p, p["x0"]), ref, "maxit=0, R1, dev")


# ---------------- 6. a window sliding along a trajectory ----------------
@pytest.mark.parametrize("shape", ALL, ids=str)
def test_tracking_loop(solver, mode, shape):
    mode(shape)
    nx, nu, N = shape
    p0, _ = case(shape, CENTRED, "none")
    xt, ut = refs(shape, cols=N + 4)
    x = p0["x0"].copy()
    with make(solver, shape, p0) as ctl:
        for t in range(4):
            p = dict(p0, x_ref=np.ascontiguousarray(xt[:, t:t + N]), u_ref=np.ascontiguousarray(ut[:, t:t + N]))
            ref, ref_zero = oracle_at(p, x), oracle_at(p0, x)
            assert_conditions(p, ref, ref_zero, sat_min=0.25 if t == 0 else 0.05)
            ctl.set_reference(p["x_ref"], p["u_ref"])
            got = ctl.step(x)
            check(p, got, ref, f"{shape} t={t}")
            # the model is the plant, driven by the controller's own first move
            x = np.einsum("abi,bi->ai", p0["A"], x) + np.einsum("aki,ki->ai", p0["B"], got["u_0"])


def test_closed_controller_raises(solver, mode):
    shape = (4, 2, 10)
    mode(shape)
    p0, _ = case(shape, CENTRED, "none")
    ctl = make(solver, shape, p0)
    ctl.close()
    with pytest.raises(LqmpcError):
        ctl.set_reference()
    with pytest.raises(LqmpcError):
        ctl.set_reference(*refs(shape)[0])


# ---------------- 7. it has to pay ----------------
def test_retarget_and_step_is_cheaper_than_a_solve(solver, mode):
    """Protocol of test_gpu_controller.py::test_a_step_is_cheaper_than_a_solve; both sides get new references in every call (R1 and
    R2 in turn), as a tracking loop gives them."""
    mode()
    b = synth.make_batch(3)
    nx, nu, Bsz = b["B"].shape
    N = b["N"]
    assert (nx, nu, N, Bsz) == (4, 2, 10, 65536)
    R = refs((nx, nu, N))
    dA, dB, dx = (DevArray(b[k].shape, init=b[k]) for k in ("A", "B", "x0"))
    du, dv = DevArray((nu, Bsz)), DevArray(Bsz)
    solver.reserve(nx, nu, N, Bsz)
    with BatchController(solver, N, dA, dB, b["Q"], b["R"], b["P"], b["lb"], b["ub"]) as ctl:
        assert "ctl" in ctl.kernel

        def t_solve():
            solver.timer_begin()
            for k in range(20):
                solver.solve_batch_dev(nx, nu, N, Bsz, dA, dB, b["Q"], b["R"], b["P"], b["lb"], b["ub"], dx, du, dv,
                                       x_ref=R[k & 1][0], u_ref=R[k & 1][1])
            return solver.timer_end() / 20

        def t_step(cold):
            solver.timer_begin()
            for k in range(20):
                ctl.set_reference(*R[k & 1])
                if cold:
                    ctl.reset()
                ctl.step_dev(dx, du, dv)
            return solver.timer_end() / 20

        def t_set():
            solver.timer_begin()
            for k in range(20):
                ctl.set_reference(*R[k & 1])
            return solver.timer_end() / 20

        for _ in range(3):
            t_solve(); t_step(True); t_step(False); t_set()
        rounds = [(t_solve(), t_step(True), t_step(False), t_set()) for _ in range(5)]
        ts, tc, tw, tr = (float(np.median([r[k] for r in rounds])) for k in range(4))
        print(f"per call, ms: solve with references {ts:.4f}  set_reference + step, face kept {tw:.4f}  "
              f"set_reference + reset + step {tc:.4f} (not asserted)  set_reference alone {tr:.4f}")
        assert tw < ts, (tw, ts)
