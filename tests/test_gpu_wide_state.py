"""GPU (-m gpu): the wide-state shapes (9 <= nx <= 16, nu <= 4, N nu <= 32) on the run-time compiled 16-lane-row kernels, options.jit = 2.

Shapes: TX = 3 with a one-row last tile (9, 1, 1: also N = 1) and exact (12, 2, 10); TX = 4 with a one-row last tile (13, 3, 5: also the
padded stage block of 3 inputs) and exact (16, 1, 20); the widest LDS image (16, 4, 8).  203 instances: the last wavefront is partial and
203 is no multiple of the four instances of a wavefront.  The problems are those of tests/test_gpu_domain_edges.py (problem(), copied):
spectral radius of A in [0.5, 1], dense SPD Q / R / P of condition 10, x0 scales {0.01, 0.3, 3} -- free, partly and fully saturated QPs.
Rollouts run T = 6 steps on the plant 0.95 A, B (of instance 0 where the plant is shared): strictly stable, boxed inputs, so every
trajectory is bounded and no instance is left out of a comparison.

Bars (those of tests/test_gpu_domain_edges.py, which the generic kernel meets on these shapes): against the fp64 oracle on every
instance 1e-10 on V_N, J_T, M_V and u; against oracle/exact.py on the first 4 instances V_N, M_V 1e-11, J_T 1e-10, u 1e-10."""
import numpy as np
import pytest

from lq_mpc_amd import BatchController, KERNEL_AUTO
from lq_mpc_amd._lib import LqmpcError
from oracle import exact as ex
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

V_BAR, J_BAR, U_BAR = 1e-11, 1e-10, 1e-10
ORC_BAR = 1e-10
N_EXACT = 4
T, BSZ = 6, 203
SHAPES = [(9, 1, 1), (12, 2, 10), (13, 3, 5), (16, 1, 20), (16, 4, 8)]


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
    """Option changes that every test undoes."""
    def set_(**kw):
        solver.set_options(**kw)
    yield set_
    solver.set_options(kernel=KERNEL_AUTO, warm_start=-1, presolve=-1, r16_maxit=12, jit=-1, order=-1)


def is_wide_jit(name, shape):
    return "jit" in name and "r16" in name and "<%d,%d,%d>" % shape in name and "ctl" not in name


# ---------------- the problem of a shape and its references, computed once and never changed ----------------
_CASES = {}


def case(shape, refs=False, per_instance=False):
    """Problem, plant and references of a shape.  refs: asymmetric box inside LQMPC_MAX_BOX_CENTRE and non-zero x_ref / u_ref."""
    key = (shape, refs, per_instance)
    if key in _CASES:
        return _CASES[key]
    nx, nu, N = shape
    rng = np.random.default_rng(sum(shape) + 100 * refs)
    lb, ub = -rng.uniform(0.1, 0.4, nu), rng.uniform(0.1, 0.4, nu)
    kw = {}
    if refs:
        lb, ub = lb + 0.3, ub + 0.45                          # centres in (0.3, 0.5): well inside the limit of 1, far from symmetric
        kw = dict(x_ref=0.05 * rng.standard_normal((nx, N)), u_ref=0.05 * rng.standard_normal((nu, N)))
    p = problem(nx, nu, N, BSZ, 17 * nx + N, lb, ub)
    if per_instance:
        At, Bt = np.ascontiguousarray(0.95 * p["A"]), p["B"]
        At4, Bt4 = head(At, N_EXACT), head(Bt, N_EXACT)
    else:
        At, Bt = np.ascontiguousarray(0.95 * p["A"][:, :, 0]), np.ascontiguousarray(p["B"][:, :, 0])
        At4, Bt4 = At, Bt
    x0s = np.ascontiguousarray(rng.standard_normal((nx, 7)))
    s = sub(p, N_EXACT)
    c = dict(shape=shape, p=p, At=At, Bt=Bt, x0s=x0s, kw=kw, h=0.5 * (ub - lb),
             o_solve=orc.solve_batch(*qa(p), p["x0"], **kw),
             o_roll=orc.rollout_batch(T, *qa(p), p["x0"], At, Bt, want_traj=True, **kw),
             o_mv=orc.max_vn_batch(*qa(p), x0s, **kw),
             e_solve=ex.solve(*qa(s), s["x0"], **kw),
             e_roll=ex.rollout(T, *qa(s), s["x0"], At4, Bt4, **kw),
             e_mv1=ex.max_vn(*qa(s), x0s[:, :1], **kw))
    assert c["e_solve"]["ok"].all()
    for a in (p["A"], p["B"], p["x0"], At, Bt, x0s):
        a.setflags(write=False)
    _CASES[key] = c
    return c


WORST = {}                                                  # largest errors seen, per quantity (printed: -s shows them)


def run_all(solver, c):
    p, kw = c["p"], c["kw"]
    g1 = solver.solve_batch(*qa(p), p["x0"], **kw); k1 = solver.last_kernel()
    g2 = solver.rollout_batch(T, *qa(p), p["x0"], c["At"], c["Bt"], want_traj=True, **kw); k2 = solver.last_kernel()
    g3 = solver.max_vn_batch(*qa(p), c["x0s"][:, :1], **kw)
    g4 = solver.max_vn_batch(*qa(p), c["x0s"], **kw); k4 = solver.last_kernel()
    g5 = solver.sweep_batch(T, *qa(p), p["x0"], c["x0s"], c["At"], c["Bt"], **kw); k5 = solver.last_kernel()
    return (g1, g2, g3, g4, g5), (k1, k2, k4, k5)


def check_all(c, got, tag):
    """every entry point against the oracle on every instance and against exact.py on the first N_EXACT"""
    g1, g2, g3, g4, g5 = got
    h, m = c["h"], N_EXACT
    for g in got:
        assert np.all(g["status"] == 0), (tag, np.flatnonzero(g["status"]))
    r1, r2, r4 = c["o_solve"], c["o_roll"], c["o_mv"]
    oe = dict(V=rel(g1["V_N"], r1["V_N"]), u=u_err(g1["u_0"], r1["u_0"], h), J=rel(g2["J_T"], r2["J_T"]), U=u_err(g2["U"], r2["U"], h),
              X=float(np.max(np.abs(g2["X"] - r2["X"])) / np.max(np.abs(r2["X"]))), MV=rel(g4["M_V"], r4), MVs=rel(g5["M_V"], r4),
              Js=rel(g5["J_T"], r2["J_T"]))
    e = dict(V=rel(g1["V_N"][:m], c["e_solve"]["V"]), u=u_err(g1["u_0"][:, :m], c["e_solve"]["u_0"], h),
             J=rel(g2["J_T"][:m], c["e_roll"]["J_T"]), U=u_err(g2["U"][:, :, :m], c["e_roll"]["U"], h), MV=rel(g3["M_V"][:m], c["e_mv1"]))
    print(f"{c['shape']} {tag}: oracle {oe} exact {e}")
    for k, v in list(oe.items()) + [("exact " + k, v) for k, v in e.items()]:
        WORST[k] = max(WORST.get(k, 0.0), v)
    assert all(v < ORC_BAR for v in oe.values()), (tag, oe)
    assert e["V"] < V_BAR and e["MV"] < V_BAR and e["J"] < J_BAR and e["u"] < U_BAR and e["U"] < U_BAR, (tag, e)


# ---------------- 1, 2: every entry point on the wide kernel, and through the hand-back ----------------
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_every_entry_point_on_the_wide_kernel(solver, opts, shape):
    c = case(shape)
    opts(jit=2)
    got, names = run_all(solver, c)
    for k in names:
        assert is_wide_jit(k, shape), names
    check_all(c, got, "jit=2")
    print("largest errors so far:", WORST)


@pytest.mark.parametrize("cap", [1, 0])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_hand_back_through_the_device_side_list(solver, opts, shape, cap):
    """r16_maxit = 1 / 0: the constrained instances leave the wide kernel with status 3 and are solved again by the generic kernel
    over the device-side list; the free ones keep the wide kernel's answer."""
    c = case(shape)
    opts(jit=2, r16_maxit=cap)
    got, names = run_all(solver, c)
    for k in names:
        assert is_wide_jit(k, shape), names
    check_all(c, got, f"jit=2 r16_maxit={cap}")
    assert got[0]["iters"].max() > 0                      # (the list was not empty: some QP needed iterations)


# ---------------- 3: the ordered rollout (the wide probe) ----------------
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_forced_order_is_bit_equal_to_the_natural_order(solver, opts, shape):
    c = case(shape)
    p = c["p"]
    opts(jit=2, order=0)
    g0 = solver.rollout_batch(T, *qa(p), p["x0"], c["At"], c["Bt"], want_traj=True)
    opts(order=1)
    g1 = solver.rollout_batch(T, *qa(p), p["x0"], c["At"], c["Bt"], want_traj=True)
    assert is_wide_jit(solver.last_kernel(), shape)
    for k in ("J_T", "X", "U", "status", "iters"):
        assert np.array_equal(g0[k], g1[k]), k
    assert rel(g1["J_T"], c["o_roll"]["J_T"]) < ORC_BAR


# ---------------- 4: asymmetric box, references ----------------
@pytest.mark.parametrize("shape", [(12, 2, 10), (16, 4, 8)], ids=str)
def test_asymmetric_box_and_references(solver, opts, shape):
    c = case(shape, refs=True)
    assert np.all(np.abs(0.5 * (c["p"]["lb"] + c["p"]["ub"])) < 1.0) and np.all(np.abs(c["p"]["lb"] + c["p"]["ub"]) > 0.5)
    opts(jit=2)
    got, names = run_all(solver, c)
    for k in names:
        assert is_wide_jit(k, shape), names
    check_all(c, got, "jit=2, asymmetric box and references")


# ---------------- 5: a plant per instance (and the free-response probe with staged records) ----------------
def test_per_instance_plant(solver, opts):
    shape = (12, 2, 10)
    c = case(shape, per_instance=True)
    p = c["p"]
    opts(jit=2)
    got, names = run_all(solver, c)
    for k in names:
        assert is_wide_jit(k, shape), names
    check_all(c, got, "jit=2, plant per instance")
    opts(order=1)                                         # (no shared plant: the probe's free-response key, records staged)
    g1 = solver.rollout_batch(T, *qa(p), p["x0"], c["At"], c["Bt"], want_traj=True)
    assert is_wide_jit(solver.last_kernel(), shape)
    for k in ("J_T", "X", "U", "status"):
        assert np.array_equal(got[1][k], g1[k]), k


# ---------------- 6: a NaN in one instance's model stays in that instance ----------------
def test_nan_in_one_model_does_not_leak_into_its_wavefront(solver, opts):
    """The four instances of a wavefront share every MFMA instruction of the set-up (one block each): instance 9's NaN must not
    reach 8, 10 or 11, nor anything else."""
    shape = (16, 4, 8)
    c = case(shape)
    p = c["p"]
    opts(jit=2)
    good, _ = run_all(solver, c)
    bad = 9
    A2 = p["A"].copy()
    A2[5, 14, bad] = np.nan
    p2 = dict(p, A=A2)
    keep = np.arange(BSZ) != bad
    g1 = solver.solve_batch(*qa(p2), p2["x0"])
    assert is_wide_jit(solver.last_kernel(), shape)
    g2 = solver.rollout_batch(T, *qa(p2), p2["x0"], c["At"], c["Bt"], want_traj=True)
    g5 = solver.sweep_batch(T, *qa(p2), p2["x0"], c["x0s"], c["At"], c["Bt"])
    for g, ref, keys in ((g1, good[0], ("V_N", "u_0")), (g2, good[1], ("J_T", "X", "U")), (g5, good[4], ("J_T", "M_V"))):
        assert g["status"][bad] == 2 and np.all(g["status"][keep] == 0), g["status"][[bad - 1, bad, bad + 1]]
        for k in keys:
            assert np.array_equal(g[k][..., keep], ref[k][..., keep]), k


# ---------------- 7: default options route as before, and agree ----------------
@pytest.mark.parametrize("shape", [(12, 2, 10), (16, 4, 8)], ids=str)
def test_default_options_still_take_the_generic_kernel(solver, opts, shape):
    c = case(shape)
    opts(jit=2)
    wide, _ = run_all(solver, c)
    opts(jit=-1)
    assert solver.get_options()["jit"] == -1
    got, names = run_all(solver, c)
    for k in names:
        assert k.startswith("lqmpc_generic"), names
    check_all(c, got, "defaults")
    h = c["h"]
    assert rel(wide[0]["V_N"], got[0]["V_N"]) < ORC_BAR and u_err(wide[0]["u_0"], got[0]["u_0"], h) < ORC_BAR
    assert rel(wide[1]["J_T"], got[1]["J_T"]) < ORC_BAR and u_err(wide[1]["U"], got[1]["U"], h) < ORC_BAR
    assert rel(wide[3]["M_V"], got[3]["M_V"]) < ORC_BAR and rel(wide[4]["J_T"], got[4]["J_T"]) < ORC_BAR


# ---------------- 8: a controller made under jit = 2 passes through to the wide kernel ----------------
def test_controller_under_jit_2_is_a_pass_through_on_the_wide_kernel(solver, opts):
    shape = (12, 2, 10)
    c = case(shape)
    p = c["p"]
    opts(jit=2)
    ref = solver.solve_batch(*qa(p), p["x0"])
    roll = solver.rollout_batch(T, *qa(p), p["x0"], c["At"], c["Bt"], want_traj=True)
    with BatchController(solver, *qa(p)) as ctl:
        opts(jit=-1)                                      # the controller runs under the options it was made with
        g = ctl.step(p["x0"])
        assert is_wide_jit(ctl.kernel, shape), ctl.kernel
        assert np.array_equal(g["u_0"], ref["u_0"]) and np.array_equal(g["V_N"], ref["V_N"]) and np.all(g["status"] == 0)
        r = ctl.rollout(T, p["x0"], c["At"], c["Bt"], want_traj=True)
        assert is_wide_jit(ctl.kernel, shape), ctl.kernel
        for k in ("J_T", "X", "U", "status", "iters"):
            assert np.array_equal(r[k], roll[k]), k


# ---------------- the option itself (needs a handle, hence here) ----------------
def test_option_round_trip_and_range(solver, opts):
    opts(jit=2)
    assert solver.get_options()["jit"] == 2
    for bad in (3, -2):
        with pytest.raises(LqmpcError, match="lqmpc error -1: jit must be -1, 0, 1 or 2"):
            solver.set_options(jit=bad)
    assert solver.get_options()["jit"] == 2
    from lq_mpc_amd import BatchSolver
    s = BatchSolver(0, jit=2)
    try:
        assert s.get_options()["jit"] == 2
    finally:
        s.close()
