"""GPU (-m gpu): the gradient of a loss on the whole plan -- every u_i, every x_i and V_N -- with respect to A, B and x0 of every instance
(lqmpc_plan_grad_batch, lqmpc_controller_plan_grad and their _dev flavours: one launch of lqmpc_plan_grad_kernel behind a plan call).

Problems: those of tests/sens_ref.py (problem, case), Bsz = 203 (a partial last wavefront), 24 at (8,4,30).  Cotangents: seeded random
w = d loss / d U_plan, s = d loss / d X_plan and gam = d loss / d V_N, gam exactly 0 on every third instance (pgrad_ref.cotangents).
Reference: long double, dense, from oracle/exact.py (pgrad_ref.reference) on the face of the GPU plan as exact.certify reports it.

Bar: g_A, g_B, g_x0 within BAR = 7.0e-12 of the reference relative to max(|ref|_max, 1), per instance: 100 times the worst error of the
fp64 numpy restatement of the kernel's algebra against the same reference (6.93e-14, g_A at (2,1,5), tests/test_pgrad_cpu.py), the
margin covering another summation order.  Every instance is compared unless the face the kernel reads off the plan bit for bit
differs from the certified one (at most 1 % of a case).
Measured on one MI355X (worst over the cases): g_A 1.6e-13 at (4,2,20), g_B 4.7e-14 (references and the off-centre box), g_x0 6.2e-14;
with the cotangent at stage 0 alone g_A and g_B are bit for bit those of lqmpc_model_grad_batch and g_x0 is within 2.2e-16; no
instance of any case was left out.  The largest LDS image of the domain, (16,2,64), is run on a made-up plan against the long-double
restatement of the kernel's algebra, with a bar formed by the same rule at that shape: 9.4e-16 against a bar of 6.5e-14."""
import ctypes

import numpy as np
import pytest

import pgrad_ref as pg
import sens_ref as sr
from lq_mpc_amd import BatchController, KERNEL_AUTO, _lib

pytestmark = pytest.mark.gpu

BAR = 7.0e-12
KEYS = pg.KEYS
DEFAULTS = dict(kernel=KERNEL_AUTO, warm_start=-1, presolve=-1, r16_maxit=12, r16_build=-1, layout=-1, jit=-1, ctl_wg=0)


@pytest.fixture
def opts(solver):
    """Option changes that every test undoes."""
    def set_(**kw):
        solver.set_options(**kw)
    yield set_
    solver.set_options(**DEFAULTS)


def check_pgrad(p, kw, g, out, w, s, gam, tag):
    """the bar of the module docstring on one call's outputs; every figure is printed before it is asserted"""
    assert np.all(g["status"] == 0), (tag, np.flatnonzero(g["status"]))
    ref = pg.reference(p, kw, p["x0"], g["U_plan"], w, s, gam)
    free = sr.face_bits(g["U_plan"], p["lb"], p["ub"])
    same = np.all(free == ref["free"], axis=(0, 1))
    e = {k: sr.rel_err(out[k], ref[k], ax)[same].max() for k, ax in KEYS}
    print(f"{tag}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) + f"; compared {int(same.sum())} of {same.size}; "
          f"free entries {free.mean():.2f}")
    assert np.mean(~same) <= 0.01, (tag, np.flatnonzero(~same))
    assert max(e.values()) < BAR, (tag, e)


_SOLVED = {}


def solved(solver, shape, bsz=sr.BSZ, **how):
    """the plan of a case from the GPU, its cotangents and the call's outputs: computed once per case and never changed"""
    key = (shape, bsz, tuple(sorted(how.items())))
    if key not in _SOLVED:
        c = sr.case(shape, bsz=bsz, **how)
        p, kw = c["p"], c["kw"]
        g = solver.solve_batch(*sr.qa(p), p["x0"], want_plan=True, **kw)
        w, s, gam = pg.cotangents(*shape, bsz, sum(shape))
        out = solver.plan_grad_batch(*sr.qa(p), g["U_plan"], g["X_plan"], g["status"], w, s, gam, **kw)
        for a in list(g.values()) + [w, s, gam] + list(out.values()):
            a.setflags(write=False)
        _SOLVED[key] = (c, g, w, s, gam, out)
    return _SOLVED[key]


SHAPES = [((2, 1, 5), 203), ((4, 2, 10), 203), ((4, 2, 20), 203), ((3, 3, 4), 203), ((2, 1, 1), 203), ((8, 4, 30), 24), ((16, 4, 8), 203)]


@pytest.mark.parametrize("shape,bsz", SHAPES, ids=str)
def test_plan_grad_against_the_dense_reference(solver, shape, bsz):
    """(2,1,1): the single stage, where s_1 meets P directly"""
    c, g, w, s, gam, out = solved(solver, shape, bsz)
    kernel = solver.last_kernel()
    assert "plan_grad" not in kernel                                # (the solve kernel's name, not the post-pass's)
    nx, nu, _ = shape
    assert out["g_A"].shape == (nx, nx, bsz) and out["g_B"].shape == (nx, nu, bsz) and out["g_x0"].shape == (nx, bsz)
    check_pgrad(c["p"], c["kw"], g, out, w, s, gam, f"{shape} x {bsz}")


def test_largest_lds_image_of_the_domain(solver):
    """(16,2,64), 153 568 bytes of LDS a workgroup: the post-pass alone on a made-up plan (random inputs, about a third of them on a
    bound, rolled through the model in fp64; no solve), 7 instances.  The kernel's algebra does not ask whether the plan is optimal,
    so its long-double numpy restatement on the same inputs is the reference.  Bar, by the rule of the module docstring at this
    shape: 100 times the worst error of the fp64 restatement against the long-double one, computed here."""
    nx, nu, N, bsz = 16, 2, 64, 7
    ub = np.array([0.25, 0.375])
    p = sr.problem(nx, nu, N, bsz, 5, -ub, ub)
    rng = np.random.default_rng(64)
    U = rng.uniform(-0.9, 0.9, (nu, N, bsz)) * ub[:, None, None]
    on_bound = rng.random((nu, N, bsz)) < 0.3
    U[on_bound] = (np.sign(U) * ub[:, None, None])[on_bound]
    X = sr.model_roll(p, p["x0"], U)
    w, s, gam = pg.cotangents(nx, nu, N, bsz, 64)
    free = sr.face_bits(U, p["lb"], p["ub"])
    assert np.array_equal(free, ~on_bound)
    ref = pg.adjoint(*sr.model(p), free, X, U, w, s, gam, dtype=np.longdouble)
    f64 = pg.adjoint(*sr.model(p), free, X, U, w, s, gam)
    out = solver.plan_grad_batch(*sr.qa(p), U, X, None, w, s, gam)
    own = max(sr.rel_err(f64[k], ref[k], ax).max() for k, ax in KEYS)
    e = {k: sr.rel_err(out[k], ref[k], ax).max() for k, ax in KEYS}
    print(f"(16,2,64) x {bsz}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) + f"; the fp64 restatement {own:.2e}, bar {100 * own:.2e}")
    assert max(e.values()) < 100 * own, e


def test_references_and_off_centre_box(solver):
    """non-zero x_ref / u_ref and a box centred in (0.3, 0.5): a bound comes out as centre +- half-width"""
    c, g, w, s, gam, out = solved(solver, (4, 2, 10), refs=True, off_centre=True)
    check_pgrad(c["p"], c["kw"], g, out, w, s, gam, "refs, off-centre box")
    assert not sr.face_bits(g["U_plan"], c["p"]["lb"], c["p"]["ub"]).all()


def test_stage_0_cotangent_alone_gives_the_model_gradient(solver):
    """gUplan non-zero at stage 0 only and gXplan NULL: the outputs of lqmpc_model_grad_batch for the same gu0, gVN"""
    for how in ({}, dict(refs=True, off_centre=True)):
        c, g, w, _, gam, _ = solved(solver, (4, 2, 10), **how)
        p, kw = c["p"], c["kw"]
        w0 = np.zeros_like(w)
        w0[:, 0] = w[:, 0]
        a = (*sr.qa(p), g["U_plan"], g["X_plan"], g["status"])
        mine = solver.plan_grad_batch(*a, w0, None, gam, **kw)
        theirs = solver.model_grad_batch(*a, np.ascontiguousarray(w[:, 0]), gam, **kw)
        e = {k: sr.rel_err(mine[k], theirs[k], ax).max() for k, ax in KEYS}
        print(f"stage-0 cotangent against model_grad_batch {how}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
        assert max(e.values()) < BAR, e
        assert np.any(theirs["g_A"] != 0.0)


def test_cotangent_on_the_given_state_alone_passes_through(solver):
    """gXplan non-zero only in its stage-0 rows and nothing else: g_x0 = s_0 and g_A = g_B = 0.0, exactly"""
    c, g, _, s, _, _ = solved(solver, (4, 2, 10))
    p = c["p"]
    s0 = np.zeros_like(s)
    s0[:, 0] = s[:, 0]
    out = solver.plan_grad_batch(*sr.qa(p), g["U_plan"], g["X_plan"], g["status"], None, s0, None)
    assert np.array_equal(out["g_x0"], s[:, 0])
    assert np.all(out["g_A"] == 0.0) and np.all(out["g_B"] == 0.0)


def test_bits_that_must_not_move(solver):
    c, g, w, s, gam, out = solved(solver, (4, 2, 10))
    p = c["p"]
    a = (*sr.qa(p), g["U_plan"], g["X_plan"], g["status"])
    call = lambda *cot: solver.plan_grad_batch(*a, *cot)
    # every cotangent of an instance 0.0: exact zeros there, and the others keep their bits
    quiet = np.arange(2, sr.BSZ, 5)
    wq, sq, gq = w.copy(), s.copy(), gam.copy()
    wq[..., quiet], sq[..., quiet], gq[quiet] = 0.0, 0.0, 0.0
    oq = call(wq, sq, gq)
    rest = np.setdiff1d(np.arange(sr.BSZ), quiet)
    for k, _ in KEYS:
        assert np.all(oq[k][..., quiet] == 0.0), k
        assert np.array_equal(oq[k][..., rest], out[k][..., rest]), k
    # what gUplan holds at an input on a bound reaches no output
    fixed = ~sr.face_bits(g["U_plan"], p["lb"], p["ub"])
    assert fixed.sum() >= 100
    wf = w.copy()
    wf[fixed] = np.where(np.arange(int(fixed.sum())) % 2 == 0, np.nan, 1e300)
    of = call(wf, s, gam)
    # a second call; a NULL cotangent against the explicit zero array; status NULL = all 0
    again = call(w, s, gam)
    pairs = [(call(None, s, gam), call(np.zeros_like(w), s, gam)), (call(w, None, gam), call(w, np.zeros_like(s), gam)),
             (call(w, s, None), call(w, s, np.zeros_like(gam))), (call(None, None, gam), call(np.zeros_like(w), np.zeros_like(s), gam))]
    no_st = solver.plan_grad_batch(*sr.qa(p), g["U_plan"], g["X_plan"], None, w, s, gam)
    for k, _ in KEYS:
        assert np.array_equal(of[k], out[k]), k
        assert np.array_equal(again[k], out[k]) and np.array_equal(no_st[k], out[k]), k
        for null, zero in pairs:
            assert np.array_equal(null[k], zero[k]), k
            assert not np.array_equal(null[k], out[k]), k


def test_non_finite_state_gives_nan_and_leaves_its_neighbours_alone(solver):
    c, _, w, s, gam, clean = solved(solver, (4, 2, 10))
    p = c["p"]
    bad = 5                                                       # shares its wavefront with instances 4, 6 and 7
    x0 = p["x0"].copy()
    x0[2, bad] = np.nan
    g = solver.solve_batch(*sr.qa(p), x0, want_plan=True)
    assert g["status"][bad] == 2
    out = solver.plan_grad_batch(*sr.qa(p), g["U_plan"], g["X_plan"], g["status"], w, s, gam)
    for k, _ in KEYS:
        assert np.all(np.isnan(out[k][..., bad])), k
        assert np.array_equal(np.delete(out[k], bad, axis=-1), np.delete(clean[k], bad, axis=-1)), k


def test_argument_checks(solver):
    """every refusal comes before anything is enqueued: the outputs keep their bits; each single output works alone"""
    c, g, w, s, gam, out = solved(solver, (4, 2, 10))
    p = c["p"]
    N, A, B, Q, R, P, lb, ub = sr.qa(p)
    plan = (g["U_plan"], g["X_plan"], g["status"])
    with pytest.raises(_lib.LqmpcError):
        solver.plan_grad_batch(*sr.qa(p), *plan, None, None, None)                     # no cotangent
    with pytest.raises(_lib.LqmpcError):
        solver.plan_grad_batch(N, A, B, Q, R, P, ub, lb, *plan, w, s, gam)             # lb >= ub
    with pytest.raises(ValueError):
        solver.plan_grad_batch(*sr.qa(p), g["U_plan"][:, :-1], g["X_plan"], g["status"], w, s, gam)
    with pytest.raises(ValueError):
        solver.plan_grad_batch(*sr.qa(p), *plan, w, s[:, :-1], gam)
    L, h = solver._L, solver._h
    bufs = dict(g_A=np.full((4, 4, sr.BSZ), 7.0), g_B=np.full((4, 2, sr.BSZ), 7.0), g_x0=np.full((4, sr.BSZ), 7.0))
    ptr = lambda a: None if a is None else a.ctypes.data
    base = [A, B, Q, R, P, lb, ub, None, None, g["U_plan"], g["X_plan"], g["status"], w, s, gam, bufs["g_A"], bufs["g_B"], bufs["g_x0"]]
    for f in (L.lqmpc_plan_grad_batch, L.lqmpc_plan_grad_batch_dev):
        for holes in ((0,), (1,), (2,), (3,), (4,), (5,), (6,), (9,), (10,), (12, 13, 14), (15, 16, 17), (12, 13, 14, 15, 16, 17)):
            a = list(base)
            for hole in holes:
                a[hole] = None
            assert f(h, 4, 2, 10, sr.BSZ, *[ptr(v) for v in a]) == -1, holes
        for dims in ((0, 2, 10, sr.BSZ), (17, 2, 10, sr.BSZ), (4, 9, 10, sr.BSZ), (4, 2, 65, sr.BSZ), (4, 2, 10, 0)):
            assert f(h, *dims, *[ptr(v) for v in base]) == -1, dims
    with BatchController(solver, *sr.qa(p)) as ctl:
        with pytest.raises(_lib.LqmpcError):
            ctl.plan_grad(*plan, None, None, None)
        with pytest.raises(ValueError):
            ctl.plan_grad(g["U_plan"], g["X_plan"][:, :-1], g["status"], w, s, gam)
        for f in (L.lqmpc_controller_plan_grad, L.lqmpc_controller_plan_grad_dev):
            cot, outs = [ptr(w), ptr(s), ptr(gam)], [ptr(v) for v in bufs.values()]
            assert f(ctl._c, ptr(g["U_plan"]), ptr(g["X_plan"]), ptr(g["status"]), None, None, None, *outs) == -1
            assert f(ctl._c, ptr(g["U_plan"]), ptr(g["X_plan"]), ptr(g["status"]), *cot, None, None, None) == -1
    solver.sync()
    for k, v in bufs.items():
        assert np.all(v == 7.0), k
    # each single output alone (host flavour): the bits of the full call
    for hole, k in ((15, "g_A"), (16, "g_B"), (17, "g_x0")):
        a = list(base)
        a[15] = a[16] = a[17] = None
        a[hole] = bufs[k]
        assert L.lqmpc_plan_grad_batch(h, 4, 2, 10, sr.BSZ, *[ptr(v) for v in a]) == 0, k
        assert np.array_equal(bufs[k], out[k]), k
        assert all(np.all(bufs[o] == 7.0) for o in bufs if o != k), k
        bufs[k][...] = 7.0


# ---------------- device flavours ----------------
class DevArray:
    """A float64 / int32 array in HBM, allocated through the HIP runtime the library itself has loaded (as tests/test_gpu_sens.py)."""
    _hip = None

    @classmethod
    def hip(cls):
        if cls._hip is None:
            path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
            cls._hip = ctypes.CDLL(path)
            cls._hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
            cls._hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
            cls._hip.hipFree.argtypes = [ctypes.c_void_p]
        return cls._hip

    def __init__(self, shape, dtype=np.float64, init=None):
        self.shape, self.dtype = tuple(np.atleast_1d(shape)), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self._p = ctypes.c_void_p()
        assert self.hip().hipMalloc(ctypes.byref(self._p), max(self.nbytes, 8)) == 0
        if init is not None:
            src = np.ascontiguousarray(init, dtype=self.dtype)
            assert src.shape == self.shape
            assert self.hip().hipMemcpy(self._p, src.ctypes.data, self.nbytes, 1) == 0

    def data_ptr(self):
        return self._p.value

    def numpy(self):
        out = np.empty(self.shape, dtype=self.dtype)
        assert self.hip().hipMemcpy(out.ctypes.data, self._p, self.nbytes, 2) == 0
        return out

    def free(self):
        if self._p.value:
            self.hip().hipFree(self._p)
            self._p = ctypes.c_void_p()

    def __del__(self):
        self.free()


def test_host_and_device_flavours_agree_bit_for_bit(solver):
    c, g, w, s, gam, out = solved(solver, (4, 2, 10), refs=True)
    p, kw = c["p"], c["kw"]
    nx, nu, N = c["shape"]
    B_ = sr.BSZ
    src = dict(A=p["A"], B=p["B"], U=g["U_plan"], X=g["X_plan"], st=g["status"], w=w, s=s, gam=gam)
    d = {k: DevArray(v.shape, v.dtype, init=v) for k, v in src.items()}
    o = dict(g_A=DevArray((nx, nx, B_)), g_B=DevArray((nx, nu, B_)), g_x0=DevArray((nx, B_)))
    solver.plan_grad_batch_dev(nx, nu, N, B_, d["A"], d["B"], p["Q"], p["R"], p["P"], p["lb"], p["ub"], d["U"], d["X"], o["g_A"], o["g_B"],
                               d["st"], d["w"], d["s"], d["gam"], o["g_x0"], **kw)
    solver.sync()
    for k, _ in KEYS:
        assert np.array_equal(o[k].numpy(), out[k]), k
    with BatchController(solver, *sr.qa(p), **kw) as ctl:
        o2 = dict(g_B=DevArray((nx, nu, B_)), g_x0=DevArray((nx, B_)))
        ctl.plan_grad_dev(d["U"], d["X"], None, o2["g_B"], d["st"], d["w"], d["s"], d["gam"], o2["g_x0"])      # g_A left out
        solver.sync()
        host = ctl.plan_grad(g["U_plan"], g["X_plan"], g["status"], w, s, gam)
        for k in ("g_B", "g_x0"):
            assert np.array_equal(o2[k].numpy(), out[k]), k
        for k, _ in KEYS:
            assert np.array_equal(host[k], out[k]), k
    for a in list(d.values()) + list(o.values()) + list(o2.values()):
        a.free()


# ---------------- the controller flavour ----------------
def controller_against_solve(solver, p, kw, ca, cb, x, seed, tag):
    """a plan step on two twin controllers; plan_grad on the first equals the batch call on the same data bit for bit, and the next
    plain step of the first is bit for bit that of the twin, which was never asked for a gradient"""
    ga, gb = ca.step(x, want_plan=True), cb.step(x, want_plan=True)
    assert np.array_equal(ga["U_plan"], gb["U_plan"])
    nx, nu = p["B"].shape[:2]
    w, s, gam = pg.cotangents(nx, nu, p["N"], x.shape[1], seed)
    kernel = solver.last_kernel()
    out = ca.plan_grad(ga["U_plan"], ga["X_plan"], ga["status"], w, s, gam)
    assert solver.last_kernel() == kernel
    want = solver.plan_grad_batch(*sr.qa(p), ga["U_plan"], ga["X_plan"], ga["status"], w, s, gam, **kw)
    for k, _ in KEYS:
        assert np.array_equal(out[k], want[k]), (tag, k)
    check_pgrad(dict(p, x0=x), kw, ga, out, w, s, gam, tag)
    x2 = np.ascontiguousarray(0.9 * x)
    sa, sb = ca.step(x2), cb.step(x2)
    for k in ("u_0", "V_N", "status", "iters"):
        assert np.array_equal(sa[k], sb[k]), (tag, k)


def test_record_controller_after_set_model_and_set_reference(solver):
    c = sr.case((4, 2, 10))
    p = dict(c["p"])
    with BatchController(solver, *sr.qa(p)) as ca, BatchController(solver, *sr.qa(p)) as cb:
        assert "ctl_r16" in ca.kernel
        idx = np.arange(1, sr.BSZ, 3)
        q = sr.problem(4, 2, 10, idx.size, 99, p["lb"], p["ub"])
        rng = np.random.default_rng(11)
        kw = dict(x_ref=0.05 * rng.standard_normal((4, 10)), u_ref=0.05 * rng.standard_normal((2, 10)))
        for ctl in (ca, cb):
            ctl.set_model(q["A"], q["B"], idx)
            ctl.set_reference(**kw)
        p["A"], p["B"] = p["A"].copy(), p["B"].copy()
        p["A"][:, :, idx], p["B"][:, :, idx] = q["A"], q["B"]
        controller_against_solve(solver, p, kw, ca, cb, p["x0"], 21, "record controller, after set_model and set_reference")


def test_workgroup_record_controller(solver, opts):
    """ctl_wg = 1: the controller keeps no copies of A and B, the post-pass reads the heads of its records"""
    c = sr.case((8, 4, 30), bsz=24)
    p = c["p"]
    opts(ctl_wg=1)
    with BatchController(solver, *sr.qa(p)) as ca, BatchController(solver, *sr.qa(p)) as cb:
        opts(**DEFAULTS)
        assert ca.kernel == "lqmpc_wg_ctl_step_kernel"
        controller_against_solve(solver, p, c["kw"], ca, cb, p["x0"], 22, "workgroup records")


def test_pass_through_controller(solver):
    c = sr.case((16, 4, 8))
    p = c["p"]
    with BatchController(solver, *sr.qa(p)) as ca, BatchController(solver, *sr.qa(p)) as cb:
        assert "ctl" not in ca.kernel
        controller_against_solve(solver, p, c["kw"], ca, cb, p["x0"], 23, "pass-through controller")
