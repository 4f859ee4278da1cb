"""GPU (-m gpu): the gradient of a loss on (u_0, V_N) with respect to the model matrices A and B of every instance
(lqmpc_model_grad_batch, lqmpc_controller_model_grad and their _dev flavours: one launch of lqmpc_grad_kernel behind a plan call).

Problems: those of tests/sens_ref.py (problem, case), Bsz = 203 (a partial last wavefront).  Cotangents: seeded random w = d loss / d u_0
and gam = d loss / d V_N, gam exactly 0 on every third instance (grad_ref.cotangents).  Reference: long double, dense, from
oracle/exact.py (grad_ref.reference) on the face of the GPU plan as exact.certify reports it.

Bar: g_A, g_B, g_x0 within 5.8e-12 of the reference relative to max(|ref|_max, 1), per instance: 100 times the worst error of the
fp64 numpy restatement of the kernel's algebra against the same reference (5.73e-14 at (2,1,5), tests/test_grad_cpu.py), the margin
covering another summation order; that is tighter than the sens tests' 1e-10, so nothing forces a looser one.  Every instance is
compared unless the face the kernel reads off the plan bit for bit differs from the certified one (at most 1 % of a case).
g_x0 equals K_0'w + gam dV_dx of the same sens call at 1e-12.  Where stage 0 is saturated and gam is 0 every output is exactly 0.0.
Measured on one MI355X (worst over the cases): g_A 1.7e-13 at (4,2,20), g_B 3.3e-14, g_x0 1.2e-13 (the record controller after
set_model and set_reference), g_x0 against the sens call 3.1e-15; no instance of any case was left out."""
import ctypes

import numpy as np
import pytest

import grad_ref as gr
import sens_ref as sr
from lq_mpc_amd import BatchController, KERNEL_AUTO, _lib

pytestmark = pytest.mark.gpu

BAR = 5.8e-12
CROSS = 1e-12
KEYS = (("g_A", (0, 1)), ("g_B", (0, 1)), ("g_x0", 0))
DEFAULTS = dict(kernel=KERNEL_AUTO, warm_start=-1, presolve=-1, r16_maxit=12, r16_build=-1, layout=-1, jit=-1, ctl_wg=0)


@pytest.fixture
def opts(solver):
    """Option changes that every test undoes."""
    def set_(**kw):
        solver.set_options(**kw)
    yield set_
    solver.set_options(**DEFAULTS)


def cotangents(nu, bsz, seed):
    w, gam = gr.cotangents(nu, bsz, seed)
    gam[::3] = 0.0
    return w, gam


def check_grad(p, kw, g, out, w, gam, tag):
    """the bars of the module docstring on one call's outputs; every figure is printed before it is asserted"""
    assert np.all(g["status"] == 0), (tag, np.flatnonzero(g["status"]))
    ref = gr.reference(p, kw, p["x0"], g["U_plan"], w, gam)
    free = sr.face_bits(g["U_plan"], p["lb"], p["ub"])
    same = np.all(free == ref["free"], axis=(0, 1))
    e = {k: sr.rel_err(out[k], ref[k], ax)[same].max() for k, ax in KEYS}
    cross = sr.rel_err(out["g_x0"], np.einsum("kab,kb->ab", g["K_0"], w) + gam * g["dV_dx"], 0).max()
    zero = ~free[:, 0].any(axis=0) & (gam == 0.0)
    print(f"{tag}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) + f"; g_x0 against the sens call {cross:.2e}; compared "
          f"{int(same.sum())} of {same.size}; stage 0 saturated {np.mean(~free[:, 0].any(axis=0)):.2f}, of those with gam = 0: {int(zero.sum())}")
    assert np.mean(~same) <= 0.01, (tag, np.flatnonzero(~same))
    assert max(e.values()) < BAR, (tag, e)
    assert cross < CROSS, (tag, cross)
    for k, _ in KEYS:
        assert np.all(out[k][..., zero] == 0.0), (tag, k)
    return zero


def solve_and_grad(solver, c, seed):
    p, kw = c["p"], c["kw"]
    nu, bsz = p["B"].shape[1], p["x0"].shape[1]
    g = solver.solve_batch(*sr.qa(p), p["x0"], want_sens=True, **kw)
    w, gam = cotangents(nu, bsz, seed)
    out = solver.model_grad_batch(*sr.qa(p), g["U_plan"], g["X_plan"], g["status"], w, gam, **kw)
    return g, w, gam, out


# (id, shape, instances, options, the kernel lqmpc_last_kernel must name)
PATHS = [
    ("(2,1,5) throughput build", (2, 1, 5), 203, dict(r16_build=0), lambda k: "r16" in k and "<2,1,5>" in k),
    ("(2,1,5) latency build", (2, 1, 5), 203, dict(r16_build=1), lambda k: "r16" in k and "<2,1,5>" in k),
    ("(4,2,10) throughput build", (4, 2, 10), 203, dict(r16_build=0), lambda k: "r16" in k and "<4,2,10>" in k),
    ("(4,2,10) latency build", (4, 2, 10), 203, dict(r16_build=1), lambda k: "r16" in k and "<4,2,10>" in k),
    ("(4,2,20) r64", (4, 2, 20), 203, {}, lambda k: "r64" in k and "<4,2,20>" in k),
    ("(3,3,4) run-time compiled", (3, 3, 4), 203, {}, lambda k: "jit" in k and "<3,3,4>" in k),
    ("(2,1,1) single stage", (2, 1, 1), 203, {}, None),
    ("(8,4,30) workgroup", (8, 4, 30), 24, {}, lambda k: k == "lqmpc_wg_kernel"),
    ("(16,4,8) generic", (16, 4, 8), 203, {}, lambda k: k == "lqmpc_generic_kernel"),
    ("(4,2,10) packed", (4, 2, 10), 203, dict(layout=0), lambda k: k == "lqmpc_spec_kernel<4,2,10,4>"),
]


@pytest.mark.parametrize("path", PATHS, ids=[q[0] for q in PATHS])
def test_model_grad_behind_every_kernel_family(solver, opts, path):
    name, shape, bsz, o, family = path
    c = sr.case(shape, bsz=bsz)
    opts(**o)
    g, w, gam, out = solve_and_grad(solver, c, sum(shape))
    assert family is None or family(solver.last_kernel()), solver.last_kernel()      # (the solve kernel's name, not the post-pass's)
    assert out["g_A"].shape == (shape[0], shape[0], bsz) and out["g_B"].shape == (shape[0], shape[1], bsz) and out["g_x0"].shape == (shape[0], bsz)
    check_grad(c["p"], c["kw"], g, out, w, gam, name)


def test_references_and_off_centre_box(solver):
    """non-zero x_ref / u_ref and a box centred in (0.3, 0.5): a bound comes out as centre +- half-width"""
    c = sr.case((4, 2, 10), refs=True, off_centre=True)
    g, w, gam, out = solve_and_grad(solver, c, 5)
    check_grad(c["p"], c["kw"], g, out, w, gam, "refs, off-centre box")
    assert not sr.face_bits(g["U_plan"], c["p"]["lb"], c["p"]["ub"]).all()


def test_saturated_stage_0_and_zero_gam_give_exact_zeros(solver):
    """a third of the initial states of sens_ref.problem are scaled by 3, far outside the region where stage 0 is free"""
    for shape in ((4, 2, 10), (2, 1, 5)):
        c = sr.case(shape)
        g, w, gam, out = solve_and_grad(solver, c, sum(shape))
        zero = check_grad(c["p"], c["kw"], g, out, w, gam, f"{shape} zeros")
        assert zero.sum() >= 10, zero.sum()
        # ... and with gam = 0 everywhere, on every instance whose stage 0 is saturated
        out0 = solver.model_grad_batch(*sr.qa(c["p"]), g["U_plan"], g["X_plan"], g["status"], w, np.zeros_like(gam))
        sat0 = ~sr.face_bits(g["U_plan"], c["p"]["lb"], c["p"]["ub"])[:, 0].any(axis=0)
        assert sat0.sum() >= 40
        for k, _ in KEYS:
            assert np.all(out0[k][..., sat0] == 0.0), k
            assert np.any(out0[k][..., ~sat0] != 0.0), k


def test_a_null_cotangent_is_the_zero_cotangent_and_a_second_call_gives_the_same_bits(solver):
    c = sr.case((4, 2, 10))
    p = c["p"]
    g, w, gam, out = solve_and_grad(solver, c, 16)
    a = (*sr.qa(p), g["U_plan"], g["X_plan"], g["status"])
    again = solver.model_grad_batch(*a, w, gam)
    no_w, zero_w = solver.model_grad_batch(*a, None, gam), solver.model_grad_batch(*a, np.zeros_like(w), gam)
    no_g, zero_g = solver.model_grad_batch(*a, w, None), solver.model_grad_batch(*a, w, np.zeros_like(gam))
    no_st = solver.model_grad_batch(*sr.qa(p), g["U_plan"], g["X_plan"], None, w, gam)      # status NULL = all 0
    for k, _ in KEYS:
        assert np.array_equal(out[k], again[k]), k
        assert np.array_equal(no_w[k], zero_w[k]) and np.array_equal(no_g[k], zero_g[k]), k
        assert np.array_equal(out[k], no_st[k]), k
        assert not np.array_equal(no_w[k], out[k]) and not np.array_equal(no_g[k], out[k]), k


def test_non_finite_state_gives_nan_and_leaves_its_neighbours_alone(solver):
    c = sr.case((4, 2, 10))
    p = c["p"]
    _, w, gam, clean = solve_and_grad(solver, c, 16)
    bad = 5                                                       # shares its wavefront with instances 4, 6 and 7
    x0 = p["x0"].copy()
    x0[2, bad] = np.nan
    g = solver.solve_batch(*sr.qa(p), x0, want_sens=True)
    assert g["status"][bad] == 2
    out = solver.model_grad_batch(*sr.qa(p), g["U_plan"], g["X_plan"], g["status"], w, gam)
    for k, _ in KEYS:
        assert np.all(np.isnan(out[k][..., bad])), k
        assert np.array_equal(np.delete(out[k], bad, axis=-1), np.delete(clean[k], bad, axis=-1)), k


def test_argument_checks(solver):
    """every refusal comes before anything is enqueued: the outputs keep their bits"""
    c = sr.case((4, 2, 10))
    p = c["p"]
    g = solver.solve_batch(*sr.qa(p), p["x0"], want_plan=True)
    w, gam = cotangents(2, sr.BSZ, 1)
    N, A, B, Q, R, P, lb, ub = sr.qa(p)
    plan = (g["U_plan"], g["X_plan"], g["status"])
    with pytest.raises(_lib.LqmpcError):
        solver.model_grad_batch(*sr.qa(p), *plan, None, None)                          # no cotangent
    with pytest.raises(_lib.LqmpcError):
        solver.model_grad_batch(N, A, B, Q, R, P, ub, lb, *plan, w, gam)               # lb >= ub
    with pytest.raises(_lib.LqmpcError):
        solver.model_grad_batch(N, A, B, Q, R, P, lb + 3.0, ub + 3.0, *plan, w, gam)   # box centre over the limit
    with pytest.raises(ValueError):
        solver.model_grad_batch(*sr.qa(p), g["U_plan"][:, :-1], g["X_plan"], g["status"], w, gam)
    with pytest.raises(ValueError):
        solver.model_grad_batch(*sr.qa(p), *plan, w[:, :-1], gam)
    L, h = solver._L, solver._h
    sentinel = np.full((4, 4, sr.BSZ), 7.0)
    gB, ptr = np.full((4, 2, sr.BSZ), 7.0), lambda a: None if a is None else a.ctypes.data
    base = [A, B, Q, R, P, lb, ub, None, None, g["U_plan"], g["X_plan"], g["status"], w, gam, sentinel, gB, None]
    for f in (L.lqmpc_model_grad_batch, L.lqmpc_model_grad_batch_dev):
        for hole in (0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15):
            a = list(base)
            a[hole] = None
            assert f(h, 4, 2, 10, sr.BSZ, *[ptr(v) for v in a]) == -1, hole
        for dims in ((0, 2, 10, sr.BSZ), (17, 2, 10, sr.BSZ), (4, 9, 10, sr.BSZ), (4, 2, 65, sr.BSZ), (4, 2, 10, 0)):
            assert f(h, *dims, *[ptr(v) for v in base]) == -1, dims
    solver.sync()
    assert np.all(sentinel == 7.0) and np.all(gB == 7.0)
    with BatchController(solver, *sr.qa(p)) as ctl:
        with pytest.raises(_lib.LqmpcError):
            ctl.model_grad(*plan, None, None)
        with pytest.raises(ValueError):
            ctl.model_grad(g["U_plan"], g["X_plan"][:, :-1], g["status"], w, gam)


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
    c = sr.case((4, 2, 10), refs=True)
    p, kw = c["p"], c["kw"]
    nx, nu, N = c["shape"]
    B_ = sr.BSZ
    g, w, gam, out = solve_and_grad(solver, c, 3)
    d = {k: DevArray(v.shape, v.dtype, init=v) for k, v in dict(A=p["A"], B=p["B"], U=g["U_plan"], X=g["X_plan"], st=g["status"], w=w, gam=gam).items()}
    o = dict(g_A=DevArray((nx, nx, B_)), g_B=DevArray((nx, nu, B_)), g_x0=DevArray((nx, B_)))
    solver.model_grad_batch_dev(nx, nu, N, B_, d["A"], d["B"], p["Q"], p["R"], p["P"], p["lb"], p["ub"], d["U"], d["X"], o["g_A"], o["g_B"],
                                d["st"], d["w"], d["gam"], o["g_x0"], **kw)
    solver.sync()
    for k, _ in KEYS:
        assert np.array_equal(o[k].numpy(), out[k]), k
    with BatchController(solver, *sr.qa(p), **kw) as ctl:
        o2 = dict(g_A=DevArray((nx, nx, B_)), g_B=DevArray((nx, nu, B_)))
        ctl.model_grad_dev(d["U"], d["X"], o2["g_A"], o2["g_B"], d["st"], d["w"], d["gam"])          # g_x0 is optional
        solver.sync()
        host = ctl.model_grad(g["U_plan"], g["X_plan"], g["status"], w, gam)
        for k in ("g_A", "g_B"):
            assert np.array_equal(o2[k].numpy(), out[k]) and np.array_equal(host[k], out[k]), k
        assert np.array_equal(host["g_x0"], out["g_x0"])
    for a in list(d.values()) + list(o.values()) + list(o2.values()):
        a.free()


# ---------------- the controller flavour ----------------
def controller_against_solve(solver, p, kw, ca, cb, x, seed, tag):
    """a sens step on two twin controllers; model_grad on the first equals the solve flavour on the same data bit for bit, and the
    next plain step of the first is bit for bit that of the twin, which was never asked for a gradient"""
    ga, gb = ca.step(x, want_sens=True), cb.step(x, want_sens=True)
    assert np.array_equal(ga["U_plan"], gb["U_plan"])
    w, gam = cotangents(p["B"].shape[1], x.shape[1], seed)
    kernel = solver.last_kernel()
    out = ca.model_grad(ga["U_plan"], ga["X_plan"], ga["status"], w, gam)
    assert solver.last_kernel() == kernel
    want = solver.model_grad_batch(*sr.qa(p), ga["U_plan"], ga["X_plan"], ga["status"], w, gam, **kw)
    for k, _ in KEYS:
        assert np.array_equal(out[k], want[k]), (tag, k)
    q = dict(p, x0=x)
    check_grad(q, kw, ga, out, w, gam, tag)
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
