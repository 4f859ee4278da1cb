"""GPU (-m gpu): the whole optimal plan and the predicted states from solve and from the controller's step
(lqmpc_solve_plan_batch, lqmpc_controller_step_plan), on every kernel family and every path that writes them.

Problems: problem() of tests/test_gpu_wide_state.py (copied): spectral radius of A in [0.5, 1], dense SPD Q / R / P of condition 10,
x0 scales {0.01, 0.3, 3} -- free, partly and fully saturated plans -- under a symmetric random box; 203 instances (a partial last
wavefront, no multiple of the four instances of a wavefront) and 1.  A second case per shape has non-zero x_ref / u_ref, and on the
16-lane-row shapes under default options that file's off-centre box (lb + 0.3, ub + 0.45); the generic, workgroup and warm_start = 0
selectors keep the symmetric box there (their one-sided-box inaccuracy is documented in include/lqmpc.h).  Every entry of a plan lies
in [lb, ub]: exactly under the symmetric box, to the rounding of centre + half-width under the off-centre one (inside_box).

Bars: those tests/test_gpu_domain_edges.py and tests/test_gpu_wide_state.py hold u_0 and V_N to on these problems -- the plan is the
same solution vector.  Against the fp64 oracle's plan on every instance u_err < 1e-10; on the first 4 instances against
oracle/exact.py certify(..., Uplan): u_err < 1e-10 and the GPU plan's own active set passes the long-double KKT certificate;
|Xplan - X_model| <= 1e-10 max|X_model| with X_model the fp64 roll of the model under Uplan on the host; and the long-double cost of
the plan (exact.sequence_cost) within 1e-11 of V_N."""
import ctypes

import numpy as np
import pytest

from lq_mpc_amd import BatchController, LQ_MPC_Controller, KERNEL_AUTO, KERNEL_GENERIC, _lib
from oracle import exact as ex
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

U_BAR, X_BAR, V_BAR = 1e-10, 1e-10, 1e-11
N_EXACT = 4
BSZ = 203


def rel(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def u_err(u, ur, h):
    """max |u - u*| / max(|u*|, h), per input row (axis 0) with its own half-width."""
    u, ur = np.asarray(u, dtype=np.longdouble), np.asarray(ur, dtype=np.longdouble)
    hh = np.asarray(h, dtype=np.longdouble).reshape((-1,) + (1,) * (u.ndim - 1))
    return float(np.max(np.abs(u - ur) / np.maximum(np.abs(ur), hh)))


def problem(nx, nu, N, Bsz, seed, lb, ub, x_scale=1.0):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((nx, nx, Bsz))
    A *= rng.uniform(0.5, 1.0, Bsz) / np.abs(np.linalg.eigvals(A.transpose(2, 0, 1))).max(axis=1)
    B = rng.standard_normal((nx, nu, Bsz)) * rng.uniform(0.3, 1.0, (1, 1, Bsz))

    def spd(m, c):
        q, _ = np.linalg.qr(rng.standard_normal((m, m)))
        return (q * np.geomspace(1.0, c, m)) @ q.T
    Q, R, P = spd(nx, 10.0), spd(nu, 10.0), 3.0 * spd(nx, 10.0)
    # free, partly saturated and fully saturated initial states
    x0 = rng.standard_normal((nx, Bsz)) * x_scale * rng.choice([0.01, 0.3, 3.0], Bsz)
    return dict(N=N, A=np.ascontiguousarray(A), B=np.ascontiguousarray(B), Q=Q, R=R, P=P,
                lb=np.asarray(lb, dtype=float), ub=np.asarray(ub, dtype=float), x0=np.ascontiguousarray(x0))


def qa(p):
    return (p["N"], p["A"], p["B"], p["Q"], p["R"], p["P"], p["lb"], p["ub"])


def head(a, m):
    return np.ascontiguousarray(a[..., :m])


def oracle_plan(p, x0, kw):
    """the fp64 oracle's whole plan, (nu, N, Bsz)"""
    nu, Bsz = p["B"].shape[1], x0.shape[1]
    U = np.zeros((nu, p["N"], Bsz))
    for b in range(Bsz):
        U[:, :, b] = orc.solve(p["N"], p["A"][:, :, b], p["B"][:, :, b], p["Q"], p["R"], p["P"], p["lb"], p["ub"], x0[:, b],
                               kw.get("x_ref"), kw.get("u_ref"))["U"]
    return U


def model_roll(p, x0, U):
    """x_0 = x0, x_{i+1} = A x_i + B u_i in fp64: (nx, N + 1, Bsz)"""
    nx, Bsz = x0.shape
    X = np.zeros((nx, p["N"] + 1, Bsz))
    X[:, 0] = x0
    for i in range(p["N"]):
        X[:, i + 1] = np.einsum("acb,cb->ab", p["A"], X[:, i]) + np.einsum("akb,kb->ab", p["B"], U[:, i])
    return X


# ---------------- the problem of a shape and the oracle's plan, computed once and never changed ----------------
_CASES = {}


def case(shape, refs=False, off_centre=False, bsz=BSZ):
    key = (shape, refs, off_centre, bsz)
    if key in _CASES:
        return _CASES[key]
    nx, nu, N = shape
    rng = np.random.default_rng(sum(shape) + 100 * refs)
    lb, ub = -rng.uniform(0.1, 0.4, nu), rng.uniform(0.1, 0.4, nu)
    if not off_centre:
        lb = -ub                                                  # a symmetric random box: centre 0, half-width ub, both exact
    kw = {}
    if refs:
        if off_centre:
            lb, ub = lb + 0.3, ub + 0.45                          # centres in (0.3, 0.5), as tests/test_gpu_wide_state.py
        kw = dict(x_ref=0.05 * rng.standard_normal((nx, N)), u_ref=0.05 * rng.standard_normal((nu, N)))
    p = problem(nx, nu, N, bsz, 17 * nx + N, lb, ub)
    c = dict(shape=shape, p=p, kw=kw, h=0.5 * (ub - lb), U=oracle_plan(p, p["x0"], kw))
    sat = np.any((c["U"] <= lb[:, None, None]) | (c["U"] >= ub[:, None, None]), axis=(0, 1))
    free = np.any((c["U"] > lb[:, None, None]) & (c["U"] < ub[:, None, None]), axis=(0, 1))
    c["partly"] = float(np.mean(sat & free))
    c["sat"] = sat                                              # instances whose optimal plan touches the box: their QP has to iterate
    for a in (p["A"], p["B"], p["x0"], c["U"]):
        a.setflags(write=False)
    _CASES[key] = c
    return c


def check_plan(p, kw, h, x0, g, U_oracle, tag):
    """the four bars of the module docstring on one plan call's outputs; every figure is printed before it is asserted"""
    m = min(N_EXACT, x0.shape[1])
    Up, Xp = g["U_plan"], g["X_plan"]
    assert np.all(g["status"] == 0), (tag, np.flatnonzero(g["status"]))
    s4 = dict(p, A=head(p["A"], m), B=head(p["B"], m))
    cert = ex.certify(*qa(s4), head(x0, m), head(Up, m), **kw)
    Xm = model_roll(p, x0, Up)
    e = dict(u_oracle=u_err(Up, U_oracle, h), u_exact=u_err(head(Up, m), cert["U"], h), ok=bool(cert["ok"].all()),
             x=float(np.max(np.abs(Xp - Xm)) / np.max(np.abs(Xm))),
             v=rel(ex.sequence_cost(p["N"], s4["A"], s4["B"], p["Q"], p["R"], p["P"], head(x0, m), head(Up, m), **kw), g["V_N"][:m]))
    print(f"{tag}: {e}")
    assert e["u_oracle"] < U_BAR and e["u_exact"] < U_BAR and e["ok"], (tag, e)
    assert e["x"] <= X_BAR and e["v"] < V_BAR, (tag, e)
    assert np.array_equal(Up[:, 0, :], g["u_0"]) and np.array_equal(Xp[:, 0, :], x0), tag
    assert inside_box(Up, p["lb"], p["ub"]), tag


def inside_box(Up, lb, ub):
    """Every entry in [lb, ub].  Exactly so for a symmetric box.  The row and workgroup kernels form a bound as centre +- half-width
    (u_0 of the plain call as well): off centre, fl(fl((ub - lb) / 2) + fl((ub + lb) / 2)) is ub up to the three roundings in it, each
    at most half an ulp of a number no larger than max(|lb|, |ub|) -- two ulps of that allowed there, none where lb = -ub."""
    slack = np.where(lb == -ub, 0.0, 2.0 * np.spacing(np.maximum(np.abs(lb), np.abs(ub))))[:, None, None]
    return bool(np.all(Up >= lb[:, None, None] - slack) and np.all(Up <= ub[:, None, None] + slack))


DEFAULTS = dict(kernel=KERNEL_AUTO, warm_start=-1, presolve=-1, r16_maxit=12, r16_build=-1, layout=-1, jit=-1, ctl_wg=0)


@pytest.fixture
def opts(solver):
    """Option changes that every test undoes."""
    def set_(**kw):
        solver.set_options(**kw)
    yield set_
    solver.set_options(**DEFAULTS)


def is_r16(shape, jit=False, lpi=16):
    tag = "<%d,%d,%d>" % shape
    return lambda k: ("r%d" % lpi) in k and tag in k and ("jit" in k) == jit and "ctl" not in k


# (id, shape, options, the kernel lqmpc_last_kernel must name, off-centre box in the reference case)
PATHS = [
    ("r16 n=20", (4, 2, 10), {}, is_r16((4, 2, 10)), True),                                     # rows in the second register block
    ("r16 throughput build", (4, 2, 10), dict(r16_build=0), is_r16((4, 2, 10)), True),         # constants in LDS (the build above 4 096 instances)
    ("packed", (4, 2, 10), dict(layout=0), lambda k: k == "lqmpc_spec_kernel<4,2,10,4>", True),
    ("packed interior point", (4, 2, 10), dict(warm_start=0), lambda k: k == "lqmpc_spec_kernel<4,2,10,4>", False),
    ("hand-back to the packed list pass", (4, 2, 10), dict(r16_maxit=0), is_r16((4, 2, 10)), True),
    ("r64", (4, 2, 20), {}, is_r16((4, 2, 20), lpi=64), True),
    ("r64 hand-back to the packed list kernel", (4, 2, 20), dict(r16_maxit=0), is_r16((4, 2, 20), lpi=64), True),
    ("r16 jit", (3, 2, 6), {}, is_r16((3, 2, 6), jit=True), True),
    ("r64 jit n=33", (7, 3, 11), {}, is_r16((7, 3, 11), jit=True, lpi=64), True),
    ("jit hand-back to the generic list pass", (3, 2, 6), dict(r16_maxit=0), is_r16((3, 2, 6), jit=True), True),
    ("wide (12,2,10)", (12, 2, 10), dict(jit=2), is_r16((12, 2, 10), jit=True), True),
    ("wide (13,3,5)", (13, 3, 5), dict(jit=2), is_r16((13, 3, 5), jit=True), True),
    ("workgroup (8,4,30)", (8, 4, 30), {}, lambda k: k == "lqmpc_wg_kernel", False),
    ("workgroup n=125", (8, 5, 25), {}, lambda k: k == "lqmpc_wg_kernel", False),
    ("generic (4,6,5)", (4, 6, 5), {}, lambda k: k == "lqmpc_generic_kernel", False),
    ("generic forced", (4, 2, 10), dict(kernel=KERNEL_GENERIC), lambda k: k == "lqmpc_generic_kernel", False),
]


@pytest.mark.parametrize("refs", [False, True], ids=["plain", "refs"])
@pytest.mark.parametrize("path", PATHS, ids=[q[0] for q in PATHS])
def test_plan_on_every_write_path(solver, opts, path, refs):
    name, shape, o, family, off = path
    c = case(shape, refs=refs, off_centre=refs and off)
    p, kw = c["p"], c["kw"]
    assert c["partly"] > 0.2, c["partly"]                         # the comparison is not vacuous: partly saturated plans
    opts(**o)
    g = solver.solve_batch(*qa(p), p["x0"], want_plan=True, **kw)
    assert family(solver.last_kernel()), solver.last_kernel()
    if "hand-back" in name:
        # r16_maxit = 0: the first pass spends no iteration and lists every QP that needs one; the iterations counted for those
        # instances are the second pass's, so it ran on each of them -- and the bars below hold its plan, not the first pass's
        assert c["sat"].any() and np.all(g["iters"][c["sat"]] > 0), g["iters"][c["sat"]]
    check_plan(p, kw, c["h"], p["x0"], g, c["U"], f"{name} refs={refs}")


@pytest.mark.parametrize("shape,bsz", [((2, 1, 5), 1), ((1, 1, 1), 1), ((1, 1, 1), BSZ), ((4, 2, 10), 1), ((8, 4, 30), 1), ((4, 6, 5), 1)], ids=str)
def test_one_instance_and_one_stage(solver, opts, shape, bsz):
    """N = 1: the plan is u_0; one instance: a wavefront with one valid group, a grid of one workgroup"""
    c = case(shape, bsz=bsz)
    p = c["p"]
    g = solver.solve_batch(*qa(p), p["x0"], want_plan=True)
    check_plan(p, {}, c["h"], p["x0"], g, c["U"], f"{shape} Bsz={bsz}")
    assert g["U_plan"].shape == (shape[1], shape[2], bsz) and g["X_plan"].shape == (shape[0], shape[2] + 1, bsz)


# ---------------- bit for bit the plain call ----------------
def solve_plan_raw(solver, p, kw, with_x):
    """lqmpc_solve_plan_batch itself, so that Xplan can be NULL"""
    nx, nu, Bsz = p["A"].shape[0], p["B"].shape[1], p["A"].shape[2]
    N = p["N"]
    u0, VN, Up = np.empty((nu, Bsz)), np.empty(Bsz), np.full((nu, N, Bsz), np.nan)
    Xp = np.full((nx, N + 1, Bsz), np.nan) if with_x else None
    st, it = np.empty(Bsz, dtype=np.int32), np.empty(Bsz, dtype=np.int32)
    ptr = lambda a: None if a is None else ctypes.c_void_p(np.ascontiguousarray(a).ctypes.data)
    keep = [np.ascontiguousarray(kw[k]) if k in kw else None for k in ("x_ref", "u_ref")]
    _lib.check(_lib.lib().lqmpc_solve_plan_batch(solver._h, nx, nu, N, Bsz, ptr(p["A"]), ptr(p["B"]), ptr(p["Q"]), ptr(p["R"]), ptr(p["P"]),
                                                 ptr(p["lb"]), ptr(p["ub"]), ptr(p["x0"]), ptr(keep[0]), ptr(keep[1]),
                                                 ptr(u0), ptr(VN), ptr(Up), ptr(Xp), ptr(st), ptr(it)))
    return dict(u_0=u0, V_N=VN, U_plan=Up, X_plan=Xp, status=st, iters=it)


@pytest.mark.parametrize("refs", [False, True], ids=["plain", "refs"])
@pytest.mark.parametrize("shape", [(4, 2, 10), (4, 2, 20), (3, 2, 6), (8, 4, 30), (4, 6, 5)], ids=str)
def test_plan_call_is_bit_equal_to_the_plain_call(solver, opts, shape, refs):
    c = case(shape, refs=refs, off_centre=refs and shape[0] != 8 and shape != (4, 6, 5))
    p, kw = c["p"], c["kw"]
    plain = solver.solve_batch(*qa(p), p["x0"], **kw)
    g = solver.solve_batch(*qa(p), p["x0"], want_plan=True, **kw)
    for k in ("u_0", "V_N", "status", "iters"):
        assert np.array_equal(plain[k], g[k]), k
    Up, Xp = g["U_plan"], g["X_plan"]
    assert np.array_equal(Up[:, 0, :], g["u_0"]) and np.array_equal(Xp[:, 0, :], p["x0"])
    assert inside_box(Up, p["lb"], p["ub"])
    nox = solve_plan_raw(solver, p, kw, with_x=False)
    both = solve_plan_raw(solver, p, kw, with_x=True)
    for k in ("u_0", "V_N", "status", "iters", "U_plan"):
        assert np.array_equal(nox[k], g[k]) and np.array_equal(both[k], g[k]), k
    assert np.array_equal(both["X_plan"], Xp)


def test_null_uplan_is_refused_before_anything_runs(solver):
    c = case((4, 2, 10))
    p = c["p"]
    L = _lib.lib()
    z = np.zeros(8 * BSZ)
    q = ctypes.c_void_p(z.ctypes.data)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    rc = L.lqmpc_solve_plan_batch(solver._h, 4, 2, 10, BSZ, ptr(p["A"]), ptr(p["B"]), ptr(p["Q"]), ptr(p["R"]), ptr(p["P"]), ptr(p["lb"]),
                                  ptr(p["ub"]), ptr(p["x0"]), None, None, q, q, None, None, None, None)
    assert rc == -1 and np.all(z == 0.0)
    with BatchController(solver, *qa(p)) as ctl:
        assert L.lqmpc_controller_step_plan(ctl._c, ptr(p["x0"]), q, q, None, None, None, None) == -1 and np.all(z == 0.0)


# ---------------- the controller's step ----------------
class DevArray:
    """A float64 / int32 array in HBM, allocated through the HIP runtime the library itself has loaded (as tests/test_gpu_controller.py)."""
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


# (id, shape, options at create, instances, what the controller's kernel name must satisfy)
CONTROLLERS = [
    ("record", (4, 2, 10), {}, BSZ, lambda k: "ctl_r16" in k and "jit" not in k),
    ("record, run-time compiled", (3, 2, 6), {}, BSZ, lambda k: "ctl_r16_jit" in k),
    # r16_maxit = 0 in the controller's snapshot: every step that has to iterate is handed back, plan pointers and all, to the packed
    # kernel's list pass / the generic kernel's list pass
    ("record, steps handed back to the packed list pass", (4, 2, 10), dict(r16_maxit=0), BSZ, lambda k: "ctl_r16" in k and "jit" not in k),
    ("record, steps handed back to the generic list pass", (3, 2, 6), dict(r16_maxit=0), BSZ, lambda k: "ctl_r16_jit" in k),
    ("workgroup records", (8, 4, 30), dict(ctl_wg=1), 48, lambda k: k == "lqmpc_wg_ctl_step_kernel"),
    ("pass-through on the wide kernel", (12, 2, 10), dict(jit=2), BSZ, lambda k: "jit" in k and "r16" in k and "ctl" not in k),
]


@pytest.mark.parametrize("refs", [False, True], ids=["plain", "refs"])
@pytest.mark.parametrize("ctl", CONTROLLERS, ids=[q[0] for q in CONTROLLERS])
def test_controller_step_plan(solver, opts, ctl, refs):
    """Two identical controllers over the same three states, one asked for the plan: the second and third steps are warm-started
    from the stored face (the model's own next state, then the same state again)."""
    name, shape, o, bsz, family = ctl
    c = case(shape, refs=refs, off_centre=refs and shape[0] != 8, bsz=bsz)
    p, kw = c["p"], c["kw"]
    opts(**o)
    with BatchController(solver, *qa(p), **kw) as ca, BatchController(solver, *qa(p), **kw) as cb:
        opts(**DEFAULTS)
        x = p["x0"]
        for step in range(3):
            ga = ca.step(x, want_plan=True)
            gb = cb.step(x)
            assert family(ca.kernel) and family(cb.kernel), (ca.kernel, cb.kernel)
            for k in ("u_0", "V_N", "status", "iters"):
                assert np.array_equal(ga[k], gb[k]), (step, k)
            U = c["U"] if step == 0 else oracle_plan(p, x, kw)
            check_plan(p, kw, c["h"], x, ga, U, f"{name} refs={refs} step {step}")
            if "handed back" in name and step == 0:
                assert c["sat"].any() and np.all(ga["iters"][c["sat"]] > 0)      # (the second pass ran on every listed instance)
            if step == 0:
                x = np.ascontiguousarray(ga["X_plan"][:, 1, :])      # the state the model expects next: the face is shifted
        # device flavour, V_N not asked for: the value function still runs for the states
        dx, du0 = DevArray(x.shape, init=x), DevArray((shape[1], bsz))
        dU, dX = DevArray(ga["U_plan"].shape), DevArray(ga["X_plan"].shape)
        ca.step_plan_dev(dx, du0, dU, dX)
        solver.sync()
        assert np.array_equal(dX.numpy(), ga["X_plan"]) and np.array_equal(dU.numpy(), ga["U_plan"]) and np.array_equal(du0.numpy(), ga["u_0"])
        for d in (dx, du0, dU, dX):
            d.free()


def test_solve_plan_batch_dev(solver):
    """the device flavour of the one-shot call, with and without Xplan"""
    c = case((4, 2, 10))
    p = c["p"]
    nx, nu, N = c["shape"]
    ref = solver.solve_batch(*qa(p), p["x0"], want_plan=True)
    dA, dB, dx0 = DevArray(p["A"].shape, init=p["A"]), DevArray(p["B"].shape, init=p["B"]), DevArray(p["x0"].shape, init=p["x0"])
    du0, dVN, dU, dX = DevArray((nu, BSZ)), DevArray(BSZ), DevArray((nu, N, BSZ)), DevArray((nx, N + 1, BSZ))
    dst, dit = DevArray(BSZ, np.int32), DevArray(BSZ, np.int32)
    w = (p["Q"], p["R"], p["P"], p["lb"], p["ub"])
    solver.solve_plan_batch_dev(nx, nu, N, BSZ, dA, dB, *w, dx0, du0, dVN, dU, dX, dst, dit)
    solver.sync()
    for d, k in ((du0, "u_0"), (dVN, "V_N"), (dU, "U_plan"), (dX, "X_plan"), (dst, "status"), (dit, "iters")):
        assert np.array_equal(d.numpy(), ref[k]), k
    dU2 = DevArray((nu, N, BSZ))
    solver.solve_plan_batch_dev(nx, nu, N, BSZ, dA, dB, *w, dx0, du0, dVN, dU2)
    solver.sync()
    assert np.array_equal(dU2.numpy(), ref["U_plan"])
    for d in (dA, dB, dx0, du0, dVN, dU, dX, dst, dit, dU2):
        d.free()


def test_reference_class_exposes_the_plan(solver):
    """LQ_MPC_Controller.u.value, as the reference's cp.Variable after solve (the reference's single example)"""
    A0, B0 = np.array([[1.0, 0.7], [0.12, 0.4]]), np.array([[1.0], [1.2]])
    N = 20
    F_u = np.vstack((10 * np.eye(1), -10 * np.eye(1)))
    ctrl = LQ_MPC_Controller(N, A0, B0, 2.0 * np.eye(2), np.eye(1), 2.0 * np.eye(2), F_u, solver=solver)
    assert ctrl.u.value is None
    x0 = np.array([0.15916231240837822, 0.15916231240837819])
    info = ctrl.solve(x0, np.zeros((2, N)), np.zeros((1, N)))
    assert set(info) == {"u_0", "V_N"}
    assert ctrl.u.value.shape == (1, N) and np.array_equal(ctrl.u.value[:, 0], info["u_0"])
    ref = orc.solve(N, A0, B0, 2.0 * np.eye(2), np.eye(1), 2.0 * np.eye(2), [-0.1], [0.1], x0)
    assert u_err(ctrl.u.value, ref["U"], [0.1]) < U_BAR
    many = ctrl.solve_many(np.stack([x0, 0.5 * x0, -x0], axis=1))
    assert ctrl.u.value.shape == (1, N, 3) and np.array_equal(ctrl.u.value[:, 0, :], many["u_0"])
