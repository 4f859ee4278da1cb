"""GPU (-m gpu): new models for some or all instances of a prepared controller, in place (BatchController.set_model /
lqmpc_controller_set_model, _dev) against the fp64 oracle of the merged models at the same states.

Inputs, helpers and bars are those of tests/test_gpu_controller.py: old models problem(nx, nu, N, 203, seed 1), new models A, B of
seed 2, states seed 1's x0; 1e-10 relative on V_N, 1e-10 * max(|u*|, h) on u_0, status 0.  The subset S: 37 distinct instances,
0 and 202 among them, in no order (SUBSET_SEED); 37 is no multiple of 4, so the last wavefront of the factor launch is partial.
Every parity test first asserts, from the ORACLE alone, that among the instances of S the new model moves u_0 by more than 1e-6 for at
least half, that at least 15 % of S has a saturated first move and at least 25 % a strictly interior one, and assert_mixed on the
whole merged problem -- a set_model that does nothing, or writes to the wrong place, fails.
Shapes as tests/test_gpu_controller_refs.py: 16-lane-row records prebuilt and run-time compiled, workgroup records (ctl_wg = 1),
the pass-through.
"""
import numpy as np
import pytest

from test_gpu_controller import BAR, DevArray, assert_mixed, check, dev_step, oracle_at, problem, qa
from test_gpu_controller_refs import refs
from lq_mpc_amd import BatchController, LqmpcError, _lib, synth

pytestmark = pytest.mark.gpu

RECORDS = [(2, 1, 10), (4, 2, 10), (4, 2, 20), (3, 2, 6), (7, 3, 11), (8, 4, 12)]
WG = [(8, 4, 13), (12, 2, 20)]
PASS_THROUGH = [(9, 5, 7), (8, 4, 30)]
ALL = RECORDS + WG + PASS_THROUGH
CENTRED, OFF_CENTRE = (-0.3, 0.3), (-0.2, 0.5)
BSZ, SEED_OLD, SEED_NEW, SUBSET_SEED = 203, 1, 2, 4
_cache = {}


def subset():
    """S: 37 of the 203 instances, the first and the last among them, shuffled"""
    rng = np.random.default_rng(SUBSET_SEED)
    S = np.concatenate(([0, BSZ - 1], 1 + rng.permutation(BSZ - 2)[:35]))
    rng.shuffle(S)
    assert S.size == 37 and np.unique(S).size == 37 and np.any(np.diff(S) < 0)
    return S.astype(np.int64)


def old(shape, box=CENTRED):
    key = ("old", shape, box)
    if key not in _cache:
        _cache[key] = problem(*shape, BSZ, SEED_OLD, lb=box[0], ub=box[1])
    return _cache[key]


def new_models(shape):
    key = ("new", shape)
    if key not in _cache:
        q = problem(*shape, BSZ, SEED_NEW)
        _cache[key] = (q["A"], q["B"])
    return _cache[key]


def merged(shape, idx, box=CENTRED, x_ref=None, u_ref=None):
    """the old problem with the new models at the instances idx (None: everywhere); not cached: the callers keep what they need"""
    p = old(shape, box)
    An, Bn = new_models(shape)
    A, B = p["A"].copy(), p["B"].copy()
    sel = slice(None) if idx is None else idx
    A[..., sel] = An[..., sel]
    B[..., sel] = Bn[..., sel]
    return dict(p, A=A, B=B, x_ref=x_ref, u_ref=u_ref)


def ref_of(key, p, x=None):
    """the oracle's answer for p at x (default: its x0), computed once per key and never modified"""
    key = ("oracle",) + key
    if key not in _cache:
        _cache[key] = oracle_at(p, p["x0"] if x is None else x)
    return _cache[key]


def update(shape, idx):
    """the compact arrays of an update: the new models of the instances idx, in that order"""
    An, Bn = new_models(shape)
    return np.ascontiguousarray(An[..., idx]), np.ascontiguousarray(Bn[..., idx])


def assert_conditions(p, ref, ref_before, S, moved_min=0.5):
    """From the oracle alone: among the updated instances the new model matters and both halves of a step are exercised; the whole
    batch is mixed."""
    h = 0.5 * (p["ub"] - p["lb"])[:, None]
    v = np.abs(ref["u_0"] - 0.5 * (p["ub"] + p["lb"])[:, None])[:, S]
    sat = np.any(v >= h * (1 - 1e-9), axis=0).mean()
    inside = np.all(v < h * (1 - 1e-6), axis=0).mean()
    moved = np.any(np.abs(ref["u_0"] - ref_before["u_0"])[:, S] > 1e-6, axis=0).mean()
    print(f"of the updated instances: saturated {sat:.2f} interior {inside:.2f} moved by the new model {moved:.2f}")
    assert moved >= moved_min and sat >= 0.15 and inside >= 0.25, (moved, sat, inside)
    assert_mixed(p, ref)


def same_bits(got, want, keep):
    for k in ("u_0", "V_N"):
        a, b = got[k][..., keep], want[k][..., keep]
        assert np.array_equal(a, b), (k, np.flatnonzero(np.any(np.atleast_2d(a != b), axis=0))[:10])


@pytest.fixture
def mode(solver):
    """the options a shape's controller is made under: ctl_wg = 1 for the workgroup records"""
    def set_(shape=None, **kw):
        solver.set_options(ctl_wg=1 if shape in WG else 0, **kw)
    yield set_
    solver.set_options(ctl_wg=0, r16_maxit=12)


def make(solver, shape, p):
    """a controller of the kind the shape is listed under"""
    ctl = BatchController(solver, *qa(p), p["x_ref"], p["u_ref"])
    if shape in RECORDS:
        assert "ctl" in ctl.kernel and "wg" not in ctl.kernel, ctl.kernel
    elif shape in WG:
        assert ctl.kernel == "lqmpc_wg_ctl_step_kernel", ctl.kernel
    else:
        assert "ctl" not in ctl.kernel, ctl.kernel
    return ctl


# ---------------- 1. a subset: the listed instances get the new model, the others keep every bit ----------------
@pytest.mark.parametrize("shape", ALL, ids=str)
def test_subset(solver, mode, shape):
    mode(shape)
    S = subset()
    p0, pm = old(shape), merged(shape, S)
    ref0, refm = ref_of(("old", shape, CENTRED), p0), ref_of(("S", shape, CENTRED), pm)
    assert_conditions(pm, refm, ref0, S)
    keep = np.setdiff1d(np.arange(BSZ), S)
    with make(solver, shape, p0) as ctl:
        check(p0, ctl.step(p0["x0"]), ref0, f"{shape} before")
        ctl.reset()
        before = ctl.step(p0["x0"])                          # a step after reset on a controller that was never updated
        ctl.set_model(*update(shape, S), S)
        check(pm, ctl.step(p0["x0"]), refm, f"{shape} subset, stored face")
        ctl.reset()
        after = ctl.step(p0["x0"])
        check(pm, after, refm, f"{shape} subset, after reset")
        same_bits(after, before, keep)                       # a wrong record address or a scatter that spills over shows here


# ---------------- 2. the whole batch ----------------
@pytest.mark.parametrize("shape", ALL, ids=str)
def test_whole_batch(solver, mode, shape):
    mode(shape)
    p0, pn = old(shape), merged(shape, None)
    ref0, refn = ref_of(("old", shape, CENTRED), p0), ref_of(("all", shape, CENTRED), pn)
    assert_conditions(pn, refn, ref0, np.arange(BSZ))
    with make(solver, shape, p0) as ctl:
        ctl.step(p0["x0"])
        ctl.set_model(pn["A"], pn["B"])
        check(pn, ctl.step(p0["x0"]), refn, f"{shape} idx=None")
    perm = np.random.default_rng(3).permutation(BSZ)
    with make(solver, shape, p0) as ctl:
        ctl.step(p0["x0"])
        ctl.set_model(*update(shape, perm), perm)
        check(pn, ctl.step(p0["x0"]), refn, f"{shape} a permutation")


# ---------------- 3. one instance ----------------
@pytest.mark.parametrize("shape", [(4, 2, 10), (4, 2, 20), (8, 4, 13), (9, 5, 7)], ids=str)
def test_one_instance(solver, mode, shape):
    mode(shape)
    one = np.array([BSZ - 1])
    p0, p1 = old(shape), merged(shape, one)
    ref0, ref1 = ref_of(("old", shape, CENTRED), p0), ref_of(("last", shape, CENTRED), p1)
    assert np.any(np.abs(ref1["u_0"] - ref0["u_0"])[:, one] > 1e-6)
    assert_mixed(p1, ref1)
    with make(solver, shape, p0) as ctl:
        before = ctl.step(p0["x0"])
        check(p0, before, ref0, f"{shape} before")
        ctl.set_model(*update(shape, one), [BSZ - 1])
        ctl.reset()                                          # (cold, as `before` was)
        after = ctl.step(p0["x0"])
        check(p1, after, ref1, f"{shape} one instance")
        same_bits(after, before, np.arange(BSZ - 1))


# ---------------- 4. the references and an off-centre box survive ----------------
@pytest.mark.parametrize("shape", ALL, ids=str)
def test_references_and_off_centre_box_survive(solver, mode, shape):
    mode(shape)
    S = subset()
    xr, ur = refs(shape)[0]
    p0 = old(shape, OFF_CENTRE)
    p0r, pmr, pm = dict(p0, x_ref=xr, u_ref=ur), merged(shape, S, OFF_CENTRE, xr, ur), merged(shape, S, OFF_CENTRE)
    ref0r = ref_of(("old R1", shape, OFF_CENTRE), p0r)
    refmr, refm = ref_of(("S R1", shape, OFF_CENTRE), pmr), ref_of(("S", shape, OFF_CENTRE), pm)
    assert_conditions(pmr, refmr, ref0r, S)
    assert_conditions(pm, refm, ref_of(("old", shape, OFF_CENTRE), p0), S)
    with make(solver, shape, p0) as ctl:                     # made without references
        ctl.set_reference(xr, ur)
        ctl.set_model(*update(shape, S), S)
        check(pmr, ctl.step(p0["x0"]), refmr, f"{shape} R1 and the new models")      # v_r from the references of NOW, not of create
        ctl.set_reference()
        check(pm, ctl.step(p0["x0"]), refm, f"{shape} no references and the new models")


# ---------------- 5. the hand-back kernels see the new model ----------------
def test_hand_back_sees_the_new_model(solver, mode):
    shape = (4, 2, 10)
    S = subset()
    p0, pm = old(shape), merged(shape, S)
    ref0, refm = ref_of(("old", shape, CENTRED), p0), ref_of(("S", shape, CENTRED), pm)
    assert_conditions(pm, refm, ref0, S)
    mode(shape, r16_maxit=0)
    ctl = make(solver, shape, p0)
    mode(shape, r16_maxit=12)                               # the controller keeps the options it was made under
    with ctl:
        ctl.set_model(*update(shape, S), S)
        check(pm, ctl.step(p0["x0"]), refm, "maxit=0, new models")     # they read the controller's copies of A and B
        check(pm, dev_step(solver, ctl, pm, p0["x0"]), refm, "maxit=0, new models, dev")


# ---------------- 6. the device flavour is ordered with the steps; the host flavour has copied its arrays ----------------
@pytest.mark.parametrize("shape", ALL, ids=str)
def test_device_flavour_is_ordered_and_host_arrays_are_copied(solver, mode, shape):
    mode(shape)
    nx, nu, N = shape
    S = subset()
    p0, pm = old(shape), merged(shape, S)
    ref0, refm = ref_of(("old", shape, CENTRED), p0), ref_of(("S", shape, CENTRED), pm)
    assert_conditions(pm, refm, ref0, S)
    uA, uB = update(shape, S)
    dA, dB, di = DevArray(uA.shape, init=uA), DevArray(uB.shape, init=uB), DevArray(S.shape, np.int32, init=S)
    dx = DevArray(p0["x0"].shape, init=p0["x0"])
    out = [(DevArray((nu, BSZ), init=np.full((nu, BSZ), np.nan)), DevArray(BSZ), DevArray(BSZ, np.int32)) for _ in range(2)]
    with make(solver, shape, p0) as ctl:
        ctl.step_dev(dx, *out[0])                           # back to back, no synchronisation in between
        ctl.set_model(dA, dB, di)
        ctl.step_dev(dx, *out[1])
        solver.sync()
        got = [{"u_0": u.numpy(), "V_N": v.numpy(), "status": s.numpy()} for u, v, s in out]
        check(p0, got[0], ref0, f"{shape} step before set_model (device)")
        check(pm, got[1], refm, f"{shape} step behind set_model (device)")
    with make(solver, shape, p0) as ctl:
        hA, hB, hS = uA.copy(), uB.copy(), S.astype(np.int32)
        ctl.set_model(hA, hB, hS)
        hA[:] = np.nan
        hB[:] = np.nan
        hS[:] = -1
        check(pm, ctl.step(p0["x0"]), refm, f"{shape} host arrays overwritten after set_model")


# ---------------- 7. an adaptive loop ----------------
@pytest.mark.parametrize("shape", [(4, 2, 10), (8, 4, 13), (9, 5, 7)], ids=str)
def test_adaptive_loop(solver, mode, shape):
    """Four steps; before each, every third instance (another residue each time) gets a new estimate A + 0.02 randn, B + 0.02 randn.
    The plant is the old model, driven by the controller's own first move."""
    mode(shape)
    p0 = old(shape)
    rng = np.random.default_rng(11)
    cur = dict(p0, A=p0["A"].copy(), B=p0["B"].copy())
    x = p0["x0"].copy()
    with make(solver, shape, p0) as ctl:
        for t in range(4):
            idx = np.arange(t % 3, BSZ, 3)
            was = oracle_at(cur, x) if t == 0 else None
            cur["A"][..., idx] += 0.02 * rng.standard_normal((*cur["A"].shape[:2], idx.size))
            cur["B"][..., idx] += 0.02 * rng.standard_normal((*cur["B"].shape[:2], idx.size))
            ref = oracle_at(cur, x)
            if t == 0:
                moved = np.any(np.abs(ref["u_0"] - was["u_0"])[:, idx] > 1e-6, axis=0).mean()
                print(f"moved by the new estimates: {moved:.2f}")
                assert moved >= 0.5, moved
                assert_mixed(cur, ref)
            ctl.set_model(np.ascontiguousarray(cur["A"][..., idx]), np.ascontiguousarray(cur["B"][..., idx]), idx)
            got = ctl.step(x)
            check(cur, got, ref, f"{shape} t={t}")
            x = np.einsum("abi,bi->ai", p0["A"], x) + np.einsum("aki,ki->ai", p0["B"], got["u_0"])


# ---------------- 8. argument errors leave the controller as it was ----------------
@pytest.mark.parametrize("shape", [(4, 2, 10), (8, 4, 13), (9, 5, 7)], ids=str)
def test_argument_errors(solver, mode, shape):
    mode(shape)
    p0 = old(shape)
    ref0 = ref_of(("old", shape, CENTRED), p0)
    assert_mixed(p0, ref0)
    uA, uB = update(shape, np.array([5, 7, 9]))
    L = _lib.lib()

    def raw(ctl, count, idx):
        i = None if idx is None else np.asarray(idx, dtype=np.int32)
        _lib.check(L.lqmpc_controller_set_model(ctl._c, count, None if i is None else i.ctypes.data, uA.ctypes.data, uB.ctypes.data))

    with make(solver, shape, p0) as ctl:
        for count, idx in ((3, [5, BSZ, 9]), (3, [5, 7, 5]), (3, [5, -1, 9]), (-1, [5, 7, 9]), (3, None)):
            with pytest.raises(LqmpcError):
                raw(ctl, count, idx)                         # refused by the library, before anything is enqueued
            check(p0, ctl.step(p0["x0"]), ref0, f"{shape} after a refused ({count}, {idx})")
        raw(ctl, 0, [5, 7, 9])                               # count = 0 changes nothing
        raw(ctl, 0, None)
        ctl.set_model(uA[..., :0], uB[..., :0], [])
        check(p0, ctl.step(p0["x0"]), ref0, f"{shape} after empty updates")
        for bad in ([5, 7, BSZ], [5, 7, 7]):
            with pytest.raises(ValueError):
                ctl.set_model(uA, uB, bad)                   # the binding's own check
        check(p0, ctl.step(p0["x0"]), ref0, f"{shape} after refused updates in the binding")
    ctl = make(solver, shape, p0)
    ctl.close()
    with pytest.raises(LqmpcError):
        ctl.set_model(uA, uB, [5, 7, 9])
    with pytest.raises(LqmpcError):
        ctl.set_model(p0["A"], p0["B"])


# ---------------- 9. it has to pay ----------------
def test_set_model_and_step_is_cheaper_than_recreating(solver, mode):
    """Protocol of test_gpu_controller_refs.py::test_retarget_and_step_is_cheaper_than_a_solve.  The other side is the only way
    there was before: destroy the controller and create it again from the device arrays."""
    mode()
    b = synth.make_batch(3)
    nx, nu, Bsz = b["B"].shape
    N = b["N"]
    assert (nx, nu, N, Bsz) == (4, 2, 10, 65536)
    dA, dB, dx = (DevArray(b[k].shape, init=b[k]) for k in ("A", "B", "x0"))
    du, dv = DevArray((nu, Bsz)), DevArray(Bsz)
    part = {}
    for m in (4096, 64):
        idx = np.random.default_rng(m).permutation(Bsz)[:m]
        part[m] = (DevArray((nx, nx, m), init=b["A"][..., idx]), DevArray((nx, nu, m), init=b["B"][..., idx]),
                   DevArray(m, np.int32, init=idx))
    solver.reserve(nx, nu, N, Bsz)
    box = [BatchController(solver, N, dA, dB, b["Q"], b["R"], b["P"], b["lb"], b["ub"])]
    try:
        assert "ctl" in box[0].kernel

        def timed(call):
            solver.timer_begin()
            for _ in range(20):
                call()
            return solver.timer_end() / 20

        def update_and_step():
            box[0].set_model(dA, dB)
            box[0].step_dev(dx, du, dv)

        def recreate_and_step():
            box[0].close()
            box[0] = BatchController(solver, N, dA, dB, b["Q"], b["R"], b["P"], b["lb"], b["ub"])
            box[0].step_dev(dx, du, dv)

        calls = [update_and_step, recreate_and_step, lambda: box[0].set_model(dA, dB), lambda: box[0].set_model(*part[4096]),
                 lambda: box[0].set_model(*part[64]), lambda: box[0].step_dev(dx, du, dv)]
        for _ in range(3):
            for c in calls:
                timed(c)
        rounds = [[timed(c) for c in calls] for _ in range(5)]
        ta, tb, tall, t4k, t64, tstep = (float(np.median([r[k] for r in rounds])) for k in range(len(calls)))
        print(f"per call, ms: set_model of all {Bsz} + step {ta:.4f}  destroy + create + step {tb:.4f}  |  not asserted: set_model alone, "
              f"all {tall:.4f}  4 096 listed {t4k:.4f}  64 listed {t64:.4f}  step {tstep:.4f}")
        assert ta < tb, (ta, tb)
    finally:
        box[0].close()
