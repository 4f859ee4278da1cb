"""GPU (-m gpu): the local feedback law K_0 = d u_0 / d x0, the gain of the whole plan K_plan and the value gradient dV_N / d x0
from solve and from the controller's step (lqmpc_solve_sens_batch, lqmpc_controller_step_sens), behind every kernel family.

Problems: those of tests/test_gpu_plan.py (tests/sens_ref.py: problem, case).  Reference: long double, from oracle/exact.py
(sens_ref.reference): on the face of the GPU plan as exact.certify reports it, K_plan[F] = -H_FF^-1 Fx[F], zero on the active rows;
dV_dx the exact central difference of the quadratic value at the fixed optimum.

Bars: K_0, K_plan and dV_dx within 1e-10 of the reference relative to max(|ref|_max, 1), per instance -- the bar the project holds
u_0 and the plan to on these problems; the fp64 numpy restatement of the kernel's algebra reaches 5e-15 on them
(tests/test_sens_cpu.py), so no case needs the wider bar the restatement's own error would give.  Every instance is compared unless the
GPU plan's face differs from the face of the oracle's own plan (at most 1 % of a case).  Rows of K_plan on a bound are exactly 0.0,
K_plan[:, 0] is bit for bit K_0, and u_0, V_N, status, iters, U_plan, X_plan are bit for bit those of the plan call.

The local law, end to end: with d = 1e-3 max|x0| randn per instance, on the instances whose face is the same at x0 + d,
|U(x0 + d) - U(x0) - K_plan d| <= 1e-10 max(|U|, h); at most 5 % of the instances may change face."""
import ctypes

import numpy as np
import pytest

import sens_ref as sr
from lq_mpc_amd import BatchController, LQ_MPC_Controller, KERNEL_AUTO, KERNEL_GENERIC

pytestmark = pytest.mark.gpu

BAR = 1e-10
PLAN_KEYS = ("u_0", "V_N", "status", "iters", "U_plan", "X_plan")
DEFAULTS = dict(kernel=KERNEL_AUTO, warm_start=-1, presolve=-1, r16_maxit=12, r16_build=-1, layout=-1, jit=-1, ctl_wg=0)


@pytest.fixture
def opts(solver):
    """Option changes that every test undoes."""
    def set_(**kw):
        solver.set_options(**kw)
    yield set_
    solver.set_options(**DEFAULTS)


def check_sens(p, kw, x0, g, U_oracle, tag, left_out=0.01):
    """the bars and conditions of the module docstring on one sens call's outputs; every figure is printed before it is asserted"""
    assert np.all(g["status"] == 0), (tag, np.flatnonzero(g["status"]))
    ref = sr.reference(p, kw, x0, g["U_plan"])
    free = ref["free"]
    same = np.all(free == sr.oracle_face(p, kw, x0, U_oracle), axis=(0, 1))
    e = dict(K_0=sr.rel_err(g["K_0"], ref["K_plan"][:, 0], (0, 1))[same].max(),
             K_plan=sr.rel_err(g["K_plan"], ref["K_plan"], (0, 1, 2))[same].max(),
             dV_dx=sr.rel_err(g["dV_dx"], ref["dV_dx"], 0)[same].max())
    partly = float(np.mean(~free.all(axis=(0, 1)) & free.any(axis=(0, 1))))
    print(f"{tag}: {e} compared {int(same.sum())} of {same.size}, partly saturated {partly:.2f}")
    assert np.mean(~same) <= left_out, (tag, np.flatnonzero(~same))
    assert e["K_0"] < BAR and e["K_plan"] < BAR and e["dV_dx"] < BAR, (tag, e)
    # the face the kernel reads off the plan bit for bit is the certified one; its rows are exact zeros
    assert np.array_equal(sr.face_bits(g["U_plan"], p["lb"], p["ub"])[..., same], free[..., same]), tag
    assert np.all(np.moveaxis(g["K_plan"], 2, 0)[..., same][:, ~free[..., same]] == 0.0), tag
    assert np.array_equal(g["K_plan"][:, 0], g["K_0"]), tag
    return ref


def check_local_law(solver, p, kw, h, g, seed, tag):
    """U(x0 + d) - U(x0) = K_plan d on the instances that keep their face: two plans of the plain plan call, no reference formula"""
    x0 = p["x0"]
    rng = np.random.default_rng(seed)
    d = 1e-3 * np.max(np.abs(x0), axis=0) * rng.standard_normal(x0.shape)
    g2 = solver.solve_batch(*sr.qa(p), x0 + d, want_plan=True, **kw)
    f1, f2 = sr.face_bits(g["U_plan"], p["lb"], p["ub"]), sr.face_bits(g2["U_plan"], p["lb"], p["ub"])
    same = np.all(f1 == f2, axis=(0, 1))
    lin = g["U_plan"] + np.einsum("kiab,ab->kib", g["K_plan"], d)
    err = np.abs(g2["U_plan"] - lin) / np.maximum(np.abs(g2["U_plan"]), h[:, None, None])
    e = float(err[..., same].max())
    print(f"{tag}: local law {e:.2e}, face changed on {int((~same).sum())} of {same.size}")
    assert np.mean(~same) <= 0.05, (tag, np.flatnonzero(~same))
    assert e <= BAR, (tag, e)


# (id, shape, instances, options, the kernel lqmpc_last_kernel must name)
PATHS = [
    ("(2,1,5)", (2, 1, 5), 203, {}, None),
    ("(2,1,5) one instance", (2, 1, 5), 1, {}, None),
    ("(4,2,10)", (4, 2, 10), 203, {}, lambda k: "r16" in k and "<4,2,10>" in k),
    ("(4,2,10) one instance", (4, 2, 10), 1, {}, None),
    ("(3,3,4)", (3, 3, 4), 203, {}, None),
    ("(3,3,4) one instance", (3, 3, 4), 1, {}, None),
    ("(4,2,10) packed", (4, 2, 10), 203, dict(layout=0), lambda k: k == "lqmpc_spec_kernel<4,2,10,4>"),
    ("(4,2,10) packed interior point", (4, 2, 10), 203, dict(warm_start=0), lambda k: k == "lqmpc_spec_kernel<4,2,10,4>"),
    ("(4,2,10) generic forced", (4, 2, 10), 203, dict(kernel=KERNEL_GENERIC), lambda k: k == "lqmpc_generic_kernel"),
    ("(4,2,20) r64", (4, 2, 20), 67, {}, lambda k: "r64" in k and "<4,2,20>" in k),
    ("(5,3,4) run-time compiled", (5, 3, 4), 67, {}, lambda k: "jit" in k and "<5,3,4>" in k),
    ("(8,4,30) workgroup", (8, 4, 30), 40, {}, lambda k: k == "lqmpc_wg_kernel"),
    ("(16,4,8) generic", (16, 4, 8), 203, {}, lambda k: k == "lqmpc_generic_kernel"),
    ("(12,8,4) generic", (12, 8, 4), 203, {}, lambda k: k == "lqmpc_generic_kernel"),
    ("(4,2,1) single stage", (4, 2, 1), 203, {}, None),
]


@pytest.mark.parametrize("path", PATHS, ids=[q[0] for q in PATHS])
def test_sens_behind_every_kernel_family(solver, opts, path):
    name, shape, bsz, o, family = path
    c = sr.case(shape, bsz=bsz)
    p, kw = c["p"], c["kw"]
    opts(**o)
    plan = solver.solve_batch(*sr.qa(p), p["x0"], want_plan=True)
    g = solver.solve_batch(*sr.qa(p), p["x0"], want_sens=True)
    assert family is None or family(solver.last_kernel()), solver.last_kernel()      # (the solve kernel's name, not the post-pass's)
    for k in PLAN_KEYS:
        assert np.array_equal(plan[k], g[k]), k
    assert g["K_0"].shape == (shape[1], shape[0], bsz) and g["dV_dx"].shape == (shape[0], bsz)
    assert g["K_plan"].shape == (shape[1], shape[2], shape[0], bsz)
    check_sens(p, kw, p["x0"], g, c["U"], name, left_out=0.01 if bsz > 1 else 0.0)
    if bsz > 1:
        check_local_law(solver, p, kw, c["h"], g, sum(shape), name)


def test_references_and_off_centre_box(solver):
    """non-zero x_ref / u_ref and a box centred in (0.3, 0.5): a bound comes out as centre +- half-width"""
    c = sr.case((4, 2, 10), refs=True, off_centre=True)
    p, kw = c["p"], c["kw"]
    plan = solver.solve_batch(*sr.qa(p), p["x0"], want_plan=True, **kw)
    g = solver.solve_batch(*sr.qa(p), p["x0"], want_sens=True, **kw)
    for k in PLAN_KEYS:
        assert np.array_equal(plan[k], g[k]), k
    ref = check_sens(p, kw, p["x0"], g, c["U"], "refs, off-centre box")
    assert not ref["free"].all()
    check_local_law(solver, p, kw, c["h"], g, 5, "refs, off-centre box")


def test_free_plan_gives_the_riccati_gain(solver):
    c = sr.case((4, 2, 10))
    p = c["p"]
    g = solver.solve_batch(*sr.qa(p), p["x0"], want_sens=True)
    idx = np.flatnonzero(sr.face_bits(g["U_plan"], p["lb"], p["ub"]).all(axis=(0, 1)))
    assert idx.size > 40
    e = sr.rel_err(g["K_0"][:, :, idx], sr.riccati_gain(p, idx), (0, 1)).max()
    print(f"free plans ({idx.size}): K_0 against the Riccati gain {e:.2e}")
    assert e < BAR


def test_non_finite_model_gives_nan_and_leaves_its_neighbours_alone(solver):
    c = sr.case((4, 2, 10))
    p = c["p"]
    clean = solver.solve_batch(*sr.qa(p), p["x0"], want_sens=True)
    bad = 5                                                       # shares its wavefront with instances 4, 6 and 7
    A = p["A"].copy()
    A[1, 2, bad] = np.nan
    g = solver.solve_batch(p["N"], A, *sr.qa(p)[2:], p["x0"], want_sens=True)
    assert g["status"][bad] == 2
    for k in ("K_0", "dV_dx", "K_plan"):
        assert np.all(np.isnan(g[k][..., bad])), k
        assert np.array_equal(np.delete(g[k], bad, axis=-1), np.delete(clean[k], bad, axis=-1)), k


# ---------------- device flavours ----------------
class DevArray:
    """A float64 / int32 array in HBM, allocated through the HIP runtime the library itself has loaded (as tests/test_gpu_plan.py)."""
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


def test_device_flavours_with_and_without_the_optional_arrays(solver):
    """solve_sens_batch_dev and step_sens_dev: everything asked for, then K_0 and dV_dx alone (the plan goes to the handle's buffers)"""
    c = sr.case((4, 2, 10))
    p = c["p"]
    nx, nu, N = c["shape"]
    B_ = sr.BSZ
    ref = solver.solve_batch(*sr.qa(p), p["x0"], want_sens=True)
    dA, dB, dx0 = DevArray(p["A"].shape, init=p["A"]), DevArray(p["B"].shape, init=p["B"]), DevArray(p["x0"].shape, init=p["x0"])
    out = dict(u_0=DevArray((nu, B_)), V_N=DevArray(B_), K_0=DevArray((nu, nx, B_)), dV_dx=DevArray((nx, B_)), K_plan=DevArray((nu, N, nx, B_)),
               U_plan=DevArray((nu, N, B_)), X_plan=DevArray((nx, N + 1, B_)), status=DevArray(B_, np.int32), iters=DevArray(B_, np.int32))
    w = (p["Q"], p["R"], p["P"], p["lb"], p["ub"])
    solver.solve_sens_batch_dev(nx, nu, N, B_, dA, dB, *w, dx0, out["u_0"], out["V_N"], out["K_0"], out["dV_dx"], out["K_plan"],
                                out["U_plan"], out["X_plan"], out["status"], out["iters"])
    solver.sync()
    for k, d in out.items():
        assert np.array_equal(d.numpy(), ref[k]), k
    K0, dV = DevArray((nu, nx, B_)), DevArray((nx, B_))
    solver.solve_sens_batch_dev(nx, nu, N, B_, dA, dB, *w, dx0, out["u_0"], out["V_N"], K0, dV)
    solver.sync()
    assert np.array_equal(K0.numpy(), ref["K_0"]) and np.array_equal(dV.numpy(), ref["dV_dx"])
    with BatchController(solver, *sr.qa(p)) as ctl:
        K0c, dVc = DevArray((nu, nx, B_)), DevArray((nx, B_))
        ctl.step_sens_dev(dx0, out["u_0"], K0c, dVc)
        solver.sync()
        e = max(sr.rel_err(K0c.numpy(), ref["K_0"], (0, 1)).max(), sr.rel_err(dVc.numpy(), ref["dV_dx"], 0).max())
        print(f"step_sens_dev against solve_sens_batch: {e:.2e}")
        assert e < BAR
    for d in list(out.values()) + [dA, dB, dx0, K0, dV, K0c, dVc]:
        d.free()


# ---------------- the controller's step ----------------
def step_pair(ca, cb, x):
    """a sens step on one controller, a plan step on its twin: bit for bit the same plan"""
    ga, gb = ca.step(x, want_sens=True), cb.step(x, want_plan=True)
    for k in PLAN_KEYS:
        assert np.array_equal(ga[k], gb[k]), k
    return ga


def test_controller_step_sens(solver):
    """a cold step, the same state again, a step after set_reference, a step after set_model on half of the instances; after every
    sens step the twin that took a plan step is in the same state (the next plain step is equal)"""
    c = sr.case((4, 2, 10))
    p, kw = dict(c["p"]), {}
    x = p["x0"]
    with BatchController(solver, *sr.qa(p)) as ca, BatchController(solver, *sr.qa(p)) as cb:
        assert "ctl_r16" in ca.kernel
        check_sens(p, kw, x, step_pair(ca, cb, x), c["U"], "controller, cold step")
        check_sens(p, kw, x, step_pair(ca, cb, x), c["U"], "controller, same state again")
        rng = np.random.default_rng(11)
        kw = dict(x_ref=0.05 * rng.standard_normal((4, 10)), u_ref=0.05 * rng.standard_normal((2, 10)))
        ca.set_reference(**kw); cb.set_reference(**kw)
        check_sens(p, kw, x, step_pair(ca, cb, x), sr.oracle_plan(p, x, kw), "controller, after set_reference")
        idx = np.arange(0, sr.BSZ, 2)
        q = sr.problem(4, 2, 10, idx.size, 99, p["lb"], p["ub"])
        ca.set_model(q["A"], q["B"], idx); cb.set_model(q["A"], q["B"], idx)
        p["A"], p["B"] = p["A"].copy(), p["B"].copy()
        p["A"][:, :, idx], p["B"][:, :, idx] = q["A"], q["B"]
        check_sens(p, kw, x, step_pair(ca, cb, x), sr.oracle_plan(p, x, kw), "controller, after set_model on half")
        x2 = np.ascontiguousarray(0.9 * x)
        ga, gb = ca.step(x2), cb.step(x2)
        for k in ("u_0", "V_N", "status", "iters"):
            assert np.array_equal(ga[k], gb[k]), k


def test_workgroup_record_controller_step_sens(solver, opts):
    """ctl_wg = 1: the controller keeps no copies of A and B, the post-pass reads the heads of its records"""
    c = sr.case((8, 4, 30), bsz=8)
    p, kw = c["p"], c["kw"]
    opts(ctl_wg=1)
    with BatchController(solver, *sr.qa(p)) as ca, BatchController(solver, *sr.qa(p)) as cb:
        opts(**DEFAULTS)
        assert ca.kernel == "lqmpc_wg_ctl_step_kernel"
        check_sens(p, kw, p["x0"], step_pair(ca, cb, p["x0"]), c["U"], "workgroup records, cold step", left_out=0.0)
        check_sens(p, kw, p["x0"], step_pair(ca, cb, p["x0"]), c["U"], "workgroup records, same state again", left_out=0.0)
        ga, gb = ca.step(p["x0"]), cb.step(p["x0"])
        for k in ("u_0", "V_N", "status", "iters"):
            assert np.array_equal(ga[k], gb[k]), k


def test_reference_class_local_law(solver):
    """LQ_MPC_Controller.local_law on the reference's single example: u_0 = K_0 x0 + k_0, and K_0 is the Riccati gain while the
    plan is free"""
    A0, B0 = np.array([[1.0, 0.7], [0.12, 0.4]]), np.array([[1.0], [1.2]])
    N = 20
    F_u = np.vstack((10 * np.eye(1), -10 * np.eye(1)))
    ctrl = LQ_MPC_Controller(N, A0, B0, 2.0 * np.eye(2), np.eye(1), 2.0 * np.eye(2), F_u, solver=solver)
    x0 = np.array([0.01, -0.02])
    K0, k0 = ctrl.local_law(x0, np.zeros((2, N)), np.zeros((1, N)))
    assert K0.shape == (1, 2) and k0.shape == (1,)
    u0 = ctrl.solve(x0, np.zeros((2, N)), np.zeros((1, N)))["u_0"]
    assert np.allclose(K0 @ x0 + k0, u0, rtol=0, atol=1e-15)
    assert np.all(np.abs(ctrl.u.value) < 0.1)
    p = dict(N=N, A=A0[:, :, None], B=B0[:, :, None], Q=2.0 * np.eye(2), R=np.eye(1), P=2.0 * np.eye(2))
    assert sr.rel_err(K0[:, :, None], sr.riccati_gain(p, np.array([0])), (0, 1)).max() < BAR
