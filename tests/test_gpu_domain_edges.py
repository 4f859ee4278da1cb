"""GPU (-m gpu): the dispatch edges of lqmpc_api.hip:make_plan() and degenerate boxes, against the long-double reference
(oracle/exact.py) and the fp64 oracle.

Bars against exact.py on these well-conditioned problems (spectral radius <= 1, SPD Q / R / P with condition <= 10):
  V_N, M_V : relative error <= 1e-11
  J_T      : relative error <= 1e-10
  u, U     : |u - u*| <= 1e-10 * max(|u*|, h)       (h = half-width of the box)
Against the fp64 oracle (every instance) the bar is 1e-10 on all of these, and X is compared over all T steps.
"""
import ctypes

import numpy as np
import pytest

from lq_mpc_amd import BatchSolver, KERNEL_AUTO, KERNEL_GENERIC
from lq_mpc_amd._lib import KERNEL_WORKGROUP, LqmpcError
from oracle import exact as ex
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

V_BAR, J_BAR, U_BAR = 1e-11, 1e-10, 1e-10
ORC_BAR = 1e-10          # against the fp64 oracle, itself ~1e-12 off exact.py on some problems
N_EXACT = 8

# one row per dispatch edge: the kernel AUTO picks today (a routing change has to update this table deliberately)
DISPATCH = {
    (4, 4, 4): "r16_jit", (1, 1, 17): "r16_jit",                    # run-time compiled 16-lane row, n <= 32
    (7, 3, 11): "r64_jit", (8, 4, 12): "r64_jit",                   # run-time compiled, one instance per wavefront (n = 48: the corner)
    (9, 5, 7): "wg", (12, 6, 10): "wg", (1, 1, 49): "wg", (8, 5, 25): "wg", (10, 8, 16): "wg",
    (16, 8, 16): "generic", (12, 2, 10): "generic", (4, 6, 5): "generic",
}
# over the build limits (nx <= 16, nu <= 8, N <= 64, N*nu <= 128): refused by every selector, never a silent fall-back
REFUSED = [(6, 1, 112), (6, 1, 113), (17, 1, 10), (3, 9, 4), (2, 1, 160)]
# the workgroup selector is accepted exactly here (the LDS budget decided on the GPU, not restated)
WG_ACCEPTS = {s for s, k in DISPATCH.items() if k in ("wg", "r64_jit")}
# rows the workgroup kernel's dual-side active-set solve holds (smax blocks of 16, lqmpc_wg.hip wg_offsets().smax * 16); an
# optimum with more active rows than this can only come from its interior-point fall-back
NEAR_BUDGET = {(8, 5, 25): 96, (10, 8, 16): 80}


def kernel_family(name):
    if "jit" in name:
        return "r16_jit" if "r16" in name else "r64_jit"
    if name == "lqmpc_wg_kernel":
        return "wg"
    if name.startswith("lqmpc_generic"):
        return "generic"
    return name


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


def sub(p, m):
    return dict(p, A=head(p["A"], m), B=head(p["B"], m), x0=head(p["x0"], m))


@pytest.fixture
def opts(solver):
    """Selector / option changes that every test undoes."""
    def set_(**kw):
        solver.set_options(**kw)
    yield set_
    solver.set_options(kernel=KERNEL_AUTO, warm_start=-1, presolve=-1, r16_maxit=12, jit=-1, order=-1)


# ---------------- the dispatch map ----------------
@pytest.mark.parametrize("shape", list(DISPATCH) + REFUSED, ids=str)
def test_dispatch_map(solver, opts, shape):
    nx, nu, N = shape
    p = problem(nx, nu, N, 5, 1, -0.3 * np.ones(nu), 0.3 * np.ones(nu))
    if shape in REFUSED:
        for sel in (KERNEL_AUTO, KERNEL_GENERIC, KERNEL_WORKGROUP):
            opts(kernel=sel)
            with pytest.raises(LqmpcError, match="lqmpc error -1: dims over the build limits"):
                solver.solve_batch(*qa(p), p["x0"])
        return
    solver.solve_batch(*qa(p), p["x0"])
    assert kernel_family(solver.last_kernel()) == DISPATCH[shape], solver.last_kernel()
    opts(kernel=KERNEL_WORKGROUP)
    if shape in WG_ACCEPTS:
        solver.solve_batch(*qa(p), p["x0"])
        assert solver.last_kernel() == "lqmpc_wg_kernel"
    else:
        with pytest.raises(LqmpcError, match="lqmpc error -5: the workgroup kernel"):
            solver.solve_batch(*qa(p), p["x0"])


# ---------------- every entry point, every selector, at every accepted edge shape ----------------
_EXACT = {}


def exact_refs(key, p, T, x0s):
    """exact.py's answers on the first N_EXACT instances (cached per problem)."""
    if key not in _EXACT:
        s = sub(p, N_EXACT)
        _EXACT[key] = dict(
            solve=ex.solve(*qa(s), s["x0"]),
            roll=ex.rollout(T, *qa(s), s["x0"], s["A"], s["B"]),
            mv1=ex.max_vn(*qa(s), x0s[:, :1]),
        )
    return _EXACT[key]


def check_all_entry_points(solver, p, T, x0s, e, h):
    """solve / rollout (all T steps) / max_vn (K = 1, 7) / sweep against the oracle on every instance and exact.py on the first
    N_EXACT; returns the worst errors against exact.py."""
    m = N_EXACT
    g1 = solver.solve_batch(*qa(p), p["x0"]); k1 = solver.last_kernel()
    g2 = solver.rollout_batch(T, *qa(p), p["x0"], p["A"], p["B"], want_traj=True)
    g3 = solver.max_vn_batch(*qa(p), x0s[:, :1])
    g4 = solver.max_vn_batch(*qa(p), x0s)
    g5 = solver.sweep_batch(T, *qa(p), p["x0"], x0s, p["A"], p["B"])
    for g in (g1, g2, g3, g4, g5):
        assert np.all(g["status"] == 0)
    r1 = orc.solve_batch(*qa(p), p["x0"])
    r2 = orc.rollout_batch(T, *qa(p), p["x0"], p["A"], p["B"], want_traj=True)
    r4 = orc.max_vn_batch(*qa(p), x0s)
    assert rel(g1["V_N"], r1["V_N"]) < ORC_BAR and u_err(g1["u_0"], r1["u_0"], h) < ORC_BAR
    assert rel(g2["J_T"], r2["J_T"]) < ORC_BAR and u_err(g2["U"], r2["U"], h) < ORC_BAR
    assert np.max(np.abs(g2["X"] - r2["X"])) < ORC_BAR * np.max(np.abs(r2["X"]))
    assert rel(g4["M_V"], r4) < ORC_BAR and rel(g5["M_V"], r4) < ORC_BAR and rel(g5["J_T"], r2["J_T"]) < ORC_BAR
    errs = dict(V=rel(g1["V_N"][:m], e["solve"]["V"]), u=u_err(g1["u_0"][:, :m], e["solve"]["u_0"], h),
                J=rel(g2["J_T"][:m], e["roll"]["J_T"]), U=u_err(g2["U"][:, :, :m], e["roll"]["U"], h),
                MV=rel(g3["M_V"][:m], e["mv1"]))
    assert errs["V"] < V_BAR and errs["MV"] < V_BAR and errs["J"] < J_BAR, (k1, errs)
    assert errs["u"] < U_BAR and errs["U"] < U_BAR, (k1, errs)
    return k1, errs


@pytest.mark.parametrize("shape", list(DISPATCH), ids=str)
def test_edge_shape_every_entry_point_and_selector(solver, opts, shape):
    nx, nu, N = shape
    T, Bsz = 6, 203                                       # ragged: not a multiple of a wavefront or a workgroup tile
    rng = np.random.default_rng(sum(shape))
    lb, ub = -rng.uniform(0.1, 0.4, nu), rng.uniform(0.1, 0.4, nu)
    p = problem(nx, nu, N, Bsz, 17 * nx + N, lb, ub)
    x0s = np.ascontiguousarray(rng.standard_normal((nx, 7)))
    e = exact_refs(shape, p, T, x0s)
    assert e["solve"]["ok"].all()
    h = 0.5 * (ub - lb)
    selectors = [("auto", dict(kernel=KERNEL_AUTO)), ("auto, interior point", dict(kernel=KERNEL_AUTO, warm_start=0)),
                 ("generic", dict(kernel=KERNEL_GENERIC))]
    if shape in WG_ACCEPTS:
        selectors.append(("workgroup", dict(kernel=KERNEL_WORKGROUP)))
    for name, o in selectors:
        opts(kernel=KERNEL_AUTO, warm_start=-1)
        opts(**o)
        k, errs = check_all_entry_points(solver, p, T, x0s, e, h)
        print(f"{shape} {name}: {k} {errs}")
        if name == "auto":
            assert kernel_family(k) == DISPATCH[shape]


@pytest.mark.parametrize("shape", list(NEAR_BUDGET), ids=str)
def test_workgroup_near_lds_budget_far_out_x0(solver, opts, shape):
    """x0 3000x out: on several instances the optimum has more active rows than the dual-side active-set solve holds, so the
    workgroup kernel can only reach it through its interior-point fall-back.  Status 0 and the exact optimum."""
    nx, nu, N = shape
    lb, ub = -0.2 * np.ones(nu), 0.25 * np.ones(nu)
    p = problem(nx, nu, N, 40, 5, lb, ub, x_scale=3000.0)
    opts(kernel=KERNEL_WORKGROUP)
    g = solver.solve_batch(*qa(p), p["x0"])
    assert solver.last_kernel() == "lqmpc_wg_kernel" and np.all(g["status"] == 0)
    s = sub(p, N_EXACT)
    e = ex.solve(*qa(s), s["x0"])
    active = ((np.abs(e["U"] - lb[:, None, None]) < 1e-12) | (np.abs(e["U"] - ub[:, None, None]) < 1e-12)).reshape(-1, N_EXACT).sum(0)
    assert np.sum(active > NEAR_BUDGET[shape]) >= 2, active
    assert rel(g["V_N"][:N_EXACT], e["V"]) < V_BAR and u_err(g["u_0"][:, :N_EXACT], e["u_0"], 0.5 * (ub - lb)) < U_BAR
    r = orc.solve_batch(*qa(p), p["x0"])
    assert rel(g["V_N"], r["V_N"]) < ORC_BAR


# ---------------- degenerate boxes ----------------
BOX_SHAPES = [(4, 2, 10), (4, 2, 20), (8, 4, 30), (8, 5, 25), (12, 2, 10)]
BOXES = {
    "wide 1e6": ((-1e6, -1e6), (1e6, 1e6)),
    "wide 1e30": ((-1e30, -1e30), (1e30, 1e30)),
    "pinned": ((0.05, 0.05), (0.05 + 1e-9, 0.05 + 1e-9)),
    "positive": ((0.02, 0.02), (0.3, 0.3)),
    "negative": ((-0.4, -0.4), (-0.01, -0.01)),
    "lb zero": ((0.0, 0.0), (0.2, 0.2)),
    "wide and pinned": ((-1e6, 0.05), (1e6, 0.05 + 1e-9)),
    "centre at the limit": ((-0.1, -0.1), (2.1, 2.1)),
    "narrow at the limit": ((0.9, 0.9), (1.1, 1.1)),
}


def box_of(name, nu):
    lo, hi = BOXES[name]
    lb = np.resize(np.array(lo), nu)
    ub = np.resize(np.array(hi), nu)
    return lb, ub


# Known defect, kept visible as strict xfails: a one-sided box [0, b] at the n > 32 shapes.  Small states put many rows on or
# near the bound 0 with multipliers far smaller than the gradient's scale, which holds P * centre (include/lqmpc.h, "Box limit").
# The workgroup kernel's dual-side active-set solve cycles there and hands the QP to its interior-point fall-back, and the
# generic kernel runs the interior-point method itself; both scale their stopping and multiplier-sign tests with that gradient,
# stop with the wrong face, and miss the bars (measured: V_N 4e-8 against the oracle on (8, 4, 30), 1.5e-10 against exact.py on
# (8, 5, 25); the generic kernel 1e-7 on both).  options.eps = 1e-14 brings (8, 5, 25) to 1e-14.
KNOWN_LB_ZERO = {((8, 4, 30), "lb zero"), ((8, 5, 25), "lb zero")}
_XFAIL_LB_ZERO = pytest.mark.xfail(strict=True, reason="one-sided box [0, b]: interior-point stopping tests scaled by P * centre "
                                                       "pick the wrong face (known defect, see KNOWN_LB_ZERO)")


@pytest.mark.parametrize("shape,box", [pytest.param(s, b, marks=[_XFAIL_LB_ZERO] if (s, b) in KNOWN_LB_ZERO else [])
                                       for s in BOX_SHAPES for b in BOXES], ids=lambda v: str(v))
def test_degenerate_boxes(solver, opts, shape, box):
    nx, nu, N = shape
    T = 5
    lb, ub = box_of(box, nu)
    h = 0.5 * (ub - lb)
    big = shape == (4, 2, 10) and box == "wide 1e6"
    Bsz = 8192 + 3 if big else 67
    p = problem(nx, nu, N, Bsz, 3 * nx + N + len(box), lb, ub)
    # the big case rolls out on a shared plant with a centred box and no references: >= 8192 instances with T >= 4 order the
    # walk by the clipped-roll key (lqmpc_api.hip make_plan(): order_roll); elsewhere the plant is per instance
    At, Bt = (p["A"][:, :, 0], p["B"][:, :, 0]) if big else (p["A"], p["B"])
    ht = lambda a, m: a if a.ndim == 2 else head(a, m)
    if box in ("positive", "negative"):
        p["x0"][:, :3] = 0.0                            # x0 = 0 with a box that excludes 0: the optimum is not 0
    rng = np.random.default_rng(9)
    x0s = np.ascontiguousarray(rng.standard_normal((nx, 3)))
    s = sub(p, N_EXACT)
    e = ex.solve(*qa(s), s["x0"])
    er = ex.rollout(T, *qa(s), s["x0"], ht(At, N_EXACT), ht(Bt, N_EXACT))
    emv = ex.max_vn(*qa(s), x0s)
    if box.startswith("wide"):
        if box != "wide and pinned":                     # never active: the Riccati closed form is the answer
            ric = ex.riccati(*qa(s)[:6], s["x0"])
            assert rel(e["V"], ric["V"]) < 1e-15
    if box == "pinned":                                  # every input on a bound: within |grad|_1 * width of the pinned cost
        pin = np.broadcast_to(lb[:, None, None], e["U"].shape)
        Vpin = ex.sequence_cost(*qa(s)[:6], s["x0"], pin)
        assert np.all(Vpin - e["V"] >= -1e-17 * e["V"]) and np.all(Vpin - e["V"] < 1e-6 * Vpin)
    legs = [("auto", {})]
    if box.startswith("wide"):
        # presolve off too, so the interior-point start with a huge h runs where the kernel has the option (the workgroup kernel
        # always tests the unconstrained minimiser first: on its rows this leg repeats the presolve path)
        legs.append(("auto, interior point", dict(warm_start=0, presolve=0)))
    for name, o in legs:
        opts(kernel=KERNEL_AUTO, warm_start=-1, presolve=-1)
        opts(**o)
        g1 = solver.solve_batch(*qa(p), p["x0"]); k = solver.last_kernel()
        g2 = solver.rollout_batch(T, *qa(p), p["x0"], At, Bt, want_traj=True)
        g3 = solver.sweep_batch(T, *qa(p), p["x0"], x0s, At, Bt)
        if big and name == "auto":                       # the ordered walk is transparent: the natural order gives the same answer
            opts(order=0)
            g0 = solver.rollout_batch(T, *qa(p), p["x0"], At, Bt, want_traj=True)
            opts(order=-1)
            assert np.abs(g0["J_T"] - g2["J_T"]).max() <= 1e-12 * np.abs(g0["J_T"]).max()
        for g in (g1, g2, g3):
            assert np.all(g["status"] == 0), (name, k)
        m = N_EXACT
        errs = dict(V=rel(g1["V_N"][:m], e["V"]), u=u_err(g1["u_0"][:, :m], e["u_0"], h), J=rel(g2["J_T"][:m], er["J_T"]),
                    U=u_err(g2["U"][:, :, :m], er["U"], h), MV=rel(g3["M_V"][:m], emv), JS=rel(g3["J_T"][:m], er["J_T"]))
        print(f"{shape} {box} {name}: {k} {errs}")
        assert errs["V"] < V_BAR and errs["MV"] < V_BAR, (k, errs)
        assert errs["J"] < J_BAR and errs["JS"] < J_BAR, (k, errs)
        assert errs["u"] < U_BAR and errs["U"] < U_BAR, (k, errs)
        idx = np.arange(min(Bsz, 256))
        sp = sub(p, idx.size)
        r1 = orc.solve_batch(*qa(sp), sp["x0"])
        r2 = orc.rollout_batch(T, *qa(sp), sp["x0"], ht(At, idx.size), ht(Bt, idx.size), want_traj=True)
        assert rel(g1["V_N"][idx], r1["V_N"]) < ORC_BAR and rel(g2["J_T"][idx], r2["J_T"]) < ORC_BAR, (k, name)
        assert u_err(g2["U"][:, :, idx], r2["U"], h) < ORC_BAR, (k, name)


@pytest.mark.parametrize("lo,hi", [(0.0, 1e6), (-1e30, 0.2), (0.0, 1e3), (-1e6, 0.2), (1.5, 2.6)])
def test_far_centred_boxes_are_refused(solver, lo, hi):
    """A box whose centre lies beyond LQMPC_MAX_BOX_CENTRE would be solved in the shifted variable v = u - c with stopping tests
    scaled by P c: measured O(1) wrong before the limit existed.  Every entry point refuses it, with a message that names the
    limit, instead of answering."""
    p = problem(4, 2, 10, 16, 2, np.array([lo, -0.1]), np.array([hi, 0.1]))
    x0s = np.ascontiguousarray(p["x0"][:, :2])
    calls = [lambda: solver.solve_batch(*qa(p), p["x0"]),
             lambda: solver.rollout_batch(4, *qa(p), p["x0"], p["A"], p["B"]),
             lambda: solver.max_vn_batch(*qa(p), x0s),
             lambda: solver.sweep_batch(4, *qa(p), p["x0"], x0s, p["A"], p["B"])]
    for call in calls:
        with pytest.raises(LqmpcError, match=r"lqmpc error -1: box of input 0 is centred at .*LQMPC_MAX_BOX_CENTRE"):
            call()


# ---------------- data_generation's concurrent passes honour the caller's options ----------------
@pytest.mark.parametrize("opt", [dict(kernel=KERNEL_GENERIC), dict(jit=0)], ids=["generic", "jit0"])
def test_concurrent_data_generation_uses_the_callers_options(golden_dir, opt):
    import os
    from lq_mpc_amd.sweep import LQ_RDP_Behavior_Multiple
    A0 = np.array([[1.0, 0.7], [0.12, 0.4]]); B0 = np.array([[1.0], [1.2]])
    info_opc = {"A": A0, "B": B0, "Q": 2.0 * np.eye(2), "R": np.eye(1), "F_u": np.vstack((10 * np.eye(1), -10 * np.eye(1)))}
    info_N = {"N_min": 6, "N_max": 10, "N_nominal": 7, "N_opc": 30, "N_mpc": 30}
    info_e = {"e_min": 1e-3, "e_max": 1e-2, "e_nominal": 5e-3}
    info_ref = {"x_ref": np.zeros((2, 7)), "u_ref": np.zeros((1, 7)), "x_ref_long": np.zeros((2, 30)), "u_ref_long": np.zeros((1, 30))}
    s = BatchSolver(0, **opt)
    beh = LQ_RDP_Behavior_Multiple(info_opc, info_N, info_e, 20, "f", data_dir=golden_dir, solver=s)
    try:
        out = beh.data_generation(8, 1.5, info_ref, np.array([0.1, 1, 0.6]))
        want = {k: v for k, v in s.get_options().items()}
        for hd in beh._handles:
            assert hd.get_options() == want
            assert "r16" not in hd.last_kernel() and hd.last_kernel() != "", hd.last_kernel()
        seq = beh.data_generation(8, 1.5, info_ref, np.array([0.1, 1, 0.6]), concurrent=False)
        assert "r16" not in s.last_kernel()
        assert len([k for k in out if k not in ("M_V_error", "M_V_horizon", "x0_vec")]) == 13
        for k, v in out.items():
            assert np.array_equal(np.asarray(v), np.asarray(seq[k])), k
        d = np.load(os.path.join(golden_dir, "data_lq_mpc_multipleSys.npz"))
        assert rel(out["true_cost_error"], d["true_cost_error"]) < 1e-10
    finally:
        beh.close()
        s.close()
    assert not hasattr(beh, "_handles") and not hasattr(beh, "_executor")


# ---------------- device entry points with the optional outputs absent ----------------
def hip_runtime():
    """The HIP runtime liblqmpc_hip.so runs on, as mapped into this process (/proc/self/maps), for hipMalloc / hipMemcpy: the
    buffers come from the very runtime the library uses, whatever file the loader resolved it to.  (torch's allocator is not
    used: torch reports no HIP GPU in this process once the library has opened the device.)"""
    from lq_mpc_amd import _lib
    _lib.lib()
    with open("/proc/self/maps") as f:
        paths = sorted({ln.split()[-1] for ln in f if "/libamdhip64.so" in ln})
    assert len(paths) == 1, paths                        # one HIP runtime in the process: the library's
    return ctypes.CDLL(paths[0])



@pytest.mark.parametrize("shape,fam", [((4, 2, 10), "r16"), ((4, 2, 20), "r64"), ((3, 2, 6), "r16_jit"), ((8, 4, 30), "wg"),
                                       ((12, 2, 10), "generic")], ids=str)
def test_device_entry_points_without_status_and_iters(solver, opts, shape, fam):
    """rollout_batch_dev / sweep_batch_dev on device buffers (hipMalloc) with dstatus = diters = NULL, trajectories on: bit-equal
    to the host-pointer call, also through the hand-back (r16_maxit = 1) and the two-launch sweep."""
    nx, nu, N = shape
    T, Bsz = 6, 300
    p = problem(nx, nu, N, Bsz, 4, -0.2 * np.ones(nu), 0.15 * np.ones(nu))
    x0s = np.ascontiguousarray(np.random.default_rng(2).standard_normal((nx, 4)))
    hip = hip_runtime()
    bufs = []

    def dev(a_or_shape):
        a = a_or_shape if isinstance(a_or_shape, np.ndarray) else np.zeros(a_or_shape)
        ptr = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(ptr), ctypes.c_size_t(a.nbytes)) == 0
        bufs.append(ptr)
        assert hip.hipMemcpy(ptr, ctypes.c_void_p(a.ctypes.data), ctypes.c_size_t(a.nbytes), 1) == 0      # host to device
        return ptr.value, a.shape

    def host(d):
        out = np.empty(d[1])
        assert hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(d[0]), ctypes.c_size_t(out.nbytes), 2) == 0
        return out
    try:
        dA, dB, dx0 = dev(p["A"])[0], dev(p["B"])[0], dev(p["x0"])[0]
        _run_dev_checks(solver, opts, p, nx, nu, N, T, Bsz, x0s, dA, dB, dx0, dev, host, fam)
    finally:
        for b in bufs:
            hip.hipFree(b)


def _run_dev_checks(solver, opts, p, nx, nu, N, T, Bsz, x0s, dA, dB, dx0, dev, host, fam):
    for cap in (12, 1):
        opts(r16_maxit=cap)
        hr = solver.rollout_batch(T, *qa(p), p["x0"], p["A"][:, :, 0], p["B"][:, :, 0], want_traj=True)
        k = solver.last_kernel()
        hs = solver.sweep_batch(T, *qa(p), p["x0"], x0s, p["A"][:, :, 0], p["B"][:, :, 0])
        ks = solver.last_kernel()
        assert np.all(hr["status"] == 0) and np.all(hs["status"] == 0)
        dJ, dX, dU = dev((Bsz,)), dev((nx, T + 1, Bsz)), dev((nu, T, Bsz))
        solver.rollout_batch_dev(nx, nu, N, Bsz, T, dA, dB, p["Q"], p["R"], p["P"], p["lb"], p["ub"], dx0,
                                 p["A"][:, :, 0], p["B"][:, :, 0], dJ[0], dX=dX[0], dU=dU[0])
        solver.sync()
        assert solver.last_kernel() == k
        assert np.array_equal(host(dJ), hr["J_T"])
        assert np.array_equal(host(dX), hr["X"]) and np.array_equal(host(dU), hr["U"])
        dJ2, dMV = dev((Bsz,)), dev((Bsz,))
        solver.sweep_batch_dev(nx, nu, N, Bsz, T, dA, dB, p["Q"], p["R"], p["P"], p["lb"], p["ub"], dx0, x0s,
                               p["A"][:, :, 0], p["B"][:, :, 0], dJ2[0], dMV[0])
        solver.sync()
        assert solver.last_kernel() == ks
        assert np.array_equal(host(dJ2), hs["J_T"]) and np.array_equal(host(dMV), hs["M_V"])
    assert kernel_family(k) == fam or fam in k
