"""GPU (-m gpu): the prepared batch controller (BatchController / lqmpc_controller_*) against the fp64 oracle.

Bars, as tests/test_gpu_domain_edges.py holds the one-shot entry points to on the same kind of problem (spectral radius <= 1, SPD
Q / R / P with condition <= 10): every instance, 1e-10 relative on V_N, |u - u*| <= 1e-10 * max(|u*|, h) on u_0, status 0.
Every parity test first asserts, from the ORACLE's answer, that its inputs exercise both halves of a step: at least a quarter of
the instances have a first move on the bound and at least a quarter have it strictly inside.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from lq_mpc_amd import BatchController, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

BAR = 1e-10
FAST = [(4, 2, 10), (2, 1, 10), (4, 2, 20), (3, 2, 6), (4, 4, 4), (7, 3, 11), (8, 4, 12)]
PASS_THROUGH = [(9, 5, 7), (8, 4, 30), (12, 2, 10)]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def u_err(u, ur, h):
    u, ur = np.asarray(u, dtype=np.longdouble), np.asarray(ur, dtype=np.longdouble)
    hh = np.asarray(h, dtype=np.longdouble).reshape((-1,) + (1,) * (u.ndim - 1))
    return float(np.max(np.abs(u - ur) / np.maximum(np.abs(ur), hh)))


def problem(nx, nu, N, Bsz, seed, lb=-0.3, ub=0.3):
    """Same kind as test_gpu_domain_edges.problem(): free, partly saturated and fully saturated initial states."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((nx, nx, Bsz))
    A *= rng.uniform(0.5, 1.0, Bsz) / np.abs(np.linalg.eigvals(A.transpose(2, 0, 1))).max(axis=1)
    B = rng.standard_normal((nx, nu, Bsz)) * rng.uniform(0.3, 1.0, (1, 1, Bsz))

    def spd(m, c):
        q, _ = np.linalg.qr(rng.standard_normal((m, m)))
        return (q * np.geomspace(1.0, c, m)) @ q.T
    Q, R, P = spd(nx, 10.0), spd(nu, 10.0), 3.0 * spd(nx, 10.0)
    x0 = rng.standard_normal((nx, Bsz)) * rng.choice([0.01, 0.3, 3.0], Bsz)
    return dict(N=N, A=np.ascontiguousarray(A), B=np.ascontiguousarray(B), Q=Q, R=R, P=P,
                lb=lb * np.ones(nu), ub=ub * np.ones(nu), x0=np.ascontiguousarray(x0), x_ref=None, u_ref=None)


def qa(p):
    return (p["N"], p["A"], p["B"], p["Q"], p["R"], p["P"], p["lb"], p["ub"])


def head(p, m):
    return dict(p, A=np.ascontiguousarray(p["A"][..., :m]), B=np.ascontiguousarray(p["B"][..., :m]),
                x0=np.ascontiguousarray(p["x0"][..., :m]))


def oracle_at(p, x):
    return orc.solve_batch(*qa(p), np.ascontiguousarray(x), p["x_ref"], p["u_ref"])


def assert_mixed(p, ref):
    """Both the shortcut and the iterations are exercised: judged from the oracle's first move, not from the code under test."""
    h = 0.5 * (p["ub"] - p["lb"])[:, None]
    v = np.abs(ref["u_0"] - 0.5 * (p["ub"] + p["lb"])[:, None])
    sat = np.any(v >= h * (1 - 1e-9), axis=0)
    inside = np.all(v < h * (1 - 1e-6), axis=0)
    assert sat.mean() >= 0.25 and inside.mean() >= 0.25, (sat.mean(), inside.mean())


def check(p, got, ref, tag=""):
    h = 0.5 * (p["ub"] - p["lb"])
    ev, eu = rel(got["V_N"], ref["V_N"]), u_err(got["u_0"], ref["u_0"], h)
    print(f"{tag} V_N relerr {ev:.2e}  u_0 err {eu:.2e}")
    if "status" in got and got["status"] is not None:
        assert np.all(got["status"] == 0), np.flatnonzero(got["status"])[:10]
    assert ev <= BAR and eu <= BAR, (tag, ev, eu)


def controller(solver, p):
    return BatchController(solver, *qa(p), p["x_ref"], p["u_ref"])


@pytest.fixture
def opts(solver):
    def set_(**kw):
        solver.set_options(**kw)
    yield set_
    solver.set_options(r16_maxit=12)


class DevArray:
    """A float64 / int32 array in HBM, allocated through the HIP runtime the library itself has loaded (torch cannot initialise
    its own in a process whose GPU the library opened first; the torch loop of test 2 therefore runs in a child process)."""
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

    def is_contiguous(self):
        return True

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


def dev_step(solver, ctl, p, x, outputs=True):
    """The device flavour; returns host arrays."""
    nu, Bsz = p["B"].shape[1], p["B"].shape[2]
    dx = DevArray(x.shape, init=x)
    du = DevArray((nu, Bsz), init=np.full((nu, Bsz), np.nan))
    dv = DevArray(Bsz) if outputs else None
    ds = DevArray(Bsz, np.int32) if outputs else None
    di = DevArray(Bsz, np.int32) if outputs else None
    ctl.step_dev(dx, du, dv, ds, di)
    solver.sync()
    return {"u_0": du.numpy(), "V_N": dv.numpy() if outputs else None,
            "status": ds.numpy() if outputs else None, "iters": di.numpy() if outputs else None}


# ---------------- 1. one step equals a solve ----------------
@pytest.mark.parametrize("shape", FAST + PASS_THROUGH, ids=str)
def test_one_step_equals_a_solve(solver, shape):
    nx, nu, N = shape
    big = 64 if shape == (8, 4, 30) else 203
    full = problem(nx, nu, N, big, 1 + (nx + nu + N) % 3)
    ref_full = oracle_at(full, full["x0"])
    assert_mixed(full, ref_full)
    sizes = [1, 5, 203, 4099] if shape == (4, 2, 10) else ([5, big] if shape in ((4, 2, 20), (3, 2, 6), (9, 5, 7)) else [big])
    for Bsz in sizes:
        if Bsz > big:
            p = problem(nx, nu, N, Bsz, 2)
            ref = oracle_at(p, p["x0"])
            assert_mixed(p, ref)
        else:
            p = head(full, Bsz)
            ref = {k: v[..., :Bsz] for k, v in ref_full.items() if k in ("u_0", "V_N")}
        with controller(solver, p) as ctl:
            got = ctl.step(p["x0"])
            check(p, got, ref, f"{shape} x{Bsz} host")
            if shape in FAST:
                assert "ctl" in ctl.kernel and solver.last_kernel() == ctl.kernel, ctl.kernel
            else:
                solver.solve_batch(*qa(p), p["x0"])
                assert ctl.kernel == solver.last_kernel()
            assert ctl.nbytes > 0
        # device flavour, controller made from device tensors; then V_N, status, iters left out
        dA, dB = DevArray(p["A"].shape, init=p["A"]), DevArray(p["B"].shape, init=p["B"])
        with BatchController(solver, p["N"], dA, dB, p["Q"], p["R"], p["P"], p["lb"], p["ub"]) as ctl:
            check(p, dev_step(solver, ctl, p, p["x0"]), ref, f"{shape} x{Bsz} dev")
            ctl.reset()
            bare = dev_step(solver, ctl, p, p["x0"], outputs=False)
            assert u_err(bare["u_0"], ref["u_0"], 0.5 * (p["ub"] - p["lb"])) <= BAR


# ---------------- 2. a controller in a loop it does not own ----------------
def plant_data(p, T, seed=11):
    rng = np.random.default_rng(seed)
    A_true = p["A"] + 0.02 * rng.standard_normal(p["A"].shape)
    B_true = p["B"] + 0.02 * rng.standard_normal(p["B"].shape)
    # a disturbance level per instance (as the generator scales its initial states): a contracting loop with small noise settles inside
    # the box within a few steps; with these levels the oracle finds 38 % of all (instance, step) pairs with a first move on the bound
    # and 62 % strictly inside (both shapes; computed on the CPU from the oracle alone)
    W = rng.standard_normal((T, p["A"].shape[0], p["A"].shape[2])) * rng.choice([0.01, 0.3, 1.5], p["A"].shape[2])
    return A_true, B_true, W


@pytest.mark.parametrize("shape", [(4, 2, 10), (4, 2, 20)], ids=str)
def test_closed_loop_around_a_torch_plant(shape, tmp_path):
    """The loop itself is tests/controller_loop_job.py, in a process of its own in which torch opens the GPU first: 30 step_dev calls
    with x+ = A_true x + B_true u + 0.2 sin(x) + w_t in torch between them, one stream, no synchronisation inside the loop; then
    the same loop on the linear shared plant without noise.  Here: its records against the oracle."""
    nx, nu, N = shape
    Bsz, T = 2048, 30
    p = problem(nx, nu, N, Bsz, 3)
    A_true, B_true, W = plant_data(p, T)
    inp, outp = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, T=T, A_true=A_true, B_true=B_true, W=W, **{k: v for k, v in p.items() if v is not None})
    job = os.path.join(os.path.dirname(os.path.abspath(__file__)), "controller_loop_job.py")
    r = subprocess.run([sys.executable, job, inp, outp], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = np.load(outp)
    h = 0.5 * (p["ub"] - p["lb"])
    assert "ctl" in str(out["kernel"])
    # non-linear plant with noise: per step, on the GPU's own states, so nothing compounds
    Xh, Uh, Vh = out["X_nl"], out["U_nl"], out["V_nl"]
    assert np.all(out["S_nl"] == 0) and np.all(out["S_lin"] == 0)
    sat = inside = 0
    for t in range(T):
        r = oracle_at(p, Xh[t])
        check(p, {"u_0": Uh[t], "V_N": Vh[t]}, r, f"{shape} t={t}")
        v = np.abs(r["u_0"])
        sat += np.any(v >= h[:, None] * (1 - 1e-9), axis=0).sum()
        inside += np.all(v < h[:, None] * (1 - 1e-6), axis=0).sum()
    assert sat >= 0.25 * T * Bsz and inside >= 0.25 * T * Bsz, (sat, inside)
    # linear shared plant, no noise: the oracle's own rollout
    At, Bt = np.ascontiguousarray(p["A"][:, :, 0]), np.ascontiguousarray(p["B"][:, :, 0])
    ref = orc.rollout_batch(T, *qa(p), p["x0"], At, Bt, want_traj=True)
    Xl, Ul = out["X_lin"], out["U_lin"]
    JT = np.einsum("tab,ac,tcb->b", Xl, p["Q"], Xl) + np.einsum("tkb,kj,tjb->b", Ul, p["R"], Ul)
    eu = u_err(Ul.transpose(1, 0, 2), ref["U"], h)
    ex = float(np.max(np.abs(Xl.transpose(1, 0, 2) - ref["X"]) / np.maximum(np.abs(ref["X"]), 1.0)))
    ej = rel(JT, ref["J_T"])
    print(f"{shape} linear loop: U {eu:.2e} X {ex:.2e} J_T {ej:.2e}")
    assert eu <= BAR and ex <= BAR and ej <= BAR


# ---------------- 3. the carried face never decides the answer ----------------
@pytest.mark.parametrize("shape", [(4, 2, 10), (4, 2, 20), (3, 2, 6)], ids=str)
def test_carried_face_never_decides(solver, shape):
    nx, nu, N = shape
    p = problem(nx, nu, N, 203, 2)
    ref = oracle_at(p, p["x0"])
    assert_mixed(p, ref)
    with controller(solver, p) as ctl:
        first = ctl.step(p["x0"])
        check(p, first, ref, "first")
        check(p, ctl.step(p["x0"]), ref, "second")          # (a) the same state again: test_same_state_twice below
        ctl.reset()                                         # (b) cold again: bit-equal to the very first call
        again = ctl.step(p["x0"])
        for k in ("u_0", "V_N", "status", "iters"):
            assert np.array_equal(again[k], first[k]), k
        xm = -3.0 * p["x0"]                                 # (c) far away, then somewhere new
        check(p, ctl.step(xm), oracle_at(p, xm), "-3x")
        xr = problem(nx, nu, N, 203, 7)["x0"]
        check(p, ctl.step(xr), oracle_at(p, xr), "fresh")
        # (d) one NaN state: status 2 there, its neighbours right, and right itself at the next finite state
        ctl.step(p["x0"])
        xn = p["x0"].copy()
        bad = 6
        xn[0, bad] = np.nan
        g = ctl.step(xn)
        assert g["status"][bad] == 2
        keep = np.arange(203) != bad
        assert np.all(g["status"][keep] == 0)
        h = 0.5 * (p["ub"] - p["lb"])
        assert rel(g["V_N"][keep], ref["V_N"][keep]) <= BAR and u_err(g["u_0"][:, keep], ref["u_0"][:, keep], h) <= BAR
        check(p, ctl.step(p["x0"]), ref, "after NaN")


@pytest.mark.parametrize("shape", [(4, 2, 10), (4, 2, 20), (3, 2, 6)], ids=str)
def test_same_state_twice(solver, shape):
    """(a) of the carried face: the second call at the same state gives the same answer to the bar, in no more iterations per
    instance than the first.  (A state that did not advance keeps its face unshifted: the controller stores the state a face
    was found at and the state the model expected next, and shifts the face only when the new state is nearer to the latter.)"""
    nx, nu, N = shape
    p = problem(nx, nu, N, 203, 2)
    ref = oracle_at(p, p["x0"])
    assert_mixed(p, ref)
    with controller(solver, p) as ctl:
        first = ctl.step(p["x0"])
        check(p, first, ref, "first")
        second = ctl.step(p["x0"])
        check(p, second, ref, "second")
        print("iters first / second:", first["iters"].sum(), second["iters"].sum())
        assert np.all(second["iters"] <= first["iters"]), np.flatnonzero(second["iters"] > first["iters"])[:10]


# ---------------- 4. hand-back ----------------
@pytest.mark.parametrize("maxit", [1, 0])
@pytest.mark.parametrize("shape", [(4, 2, 10), (3, 2, 6), (4, 2, 20)], ids=str)
def test_hand_back(solver, opts, shape, maxit):
    nx, nu, N = shape
    p = problem(nx, nu, N, 203, 3)
    ref = oracle_at(p, p["x0"])
    assert_mixed(p, ref)
    opts(r16_maxit=maxit)
    ctl = controller(solver, p)
    opts(r16_maxit=12)                                     # the controller keeps the options it was made under
    with ctl:
        assert "ctl" in ctl.kernel
        check(p, ctl.step(p["x0"]), ref, f"maxit={maxit}")
        check(p, ctl.step(p["x0"]), ref, f"maxit={maxit} again")
        check(p, dev_step(solver, ctl, p, p["x0"], outputs=True), ref, f"maxit={maxit} dev")
        bare = dev_step(solver, ctl, p, p["x0"], outputs=False)
        assert u_err(bare["u_0"], ref["u_0"], 0.5 * (p["ub"] - p["lb"])) <= BAR


# ---------------- 5. linear term ----------------
@pytest.mark.parametrize("shape", [(4, 2, 10), (7, 3, 11)], ids=str)
def test_references_and_off_centre_box(solver, shape):
    nx, nu, N = shape
    p = problem(nx, nu, N, 203, 1, lb=-0.2, ub=0.5)
    rng = np.random.default_rng(5)
    p["x_ref"] = 0.1 * rng.standard_normal((nx, N))
    p["u_ref"] = 0.05 * rng.standard_normal((nu, N))
    ref = oracle_at(p, p["x0"])
    assert_mixed(p, ref)
    with controller(solver, p) as ctl:
        assert "ctl" in ctl.kernel
        check(p, ctl.step(p["x0"]), ref, "refs")
        x2 = problem(nx, nu, N, 203, 9)["x0"]
        check(p, ctl.step(x2), oracle_at(p, x2), "refs, second state")


# ---------------- 6. life cycle ----------------
@pytest.mark.parametrize("order", [0, 1])
def test_life_cycle(solver, order):
    pa, pb = problem(4, 2, 10, 203, 1), problem(3, 2, 6, 77 + 203, 2)
    ra, rb = oracle_at(pa, pa["x0"]), oracle_at(pb, pb["x0"])
    assert_mixed(pa, ra)
    assert_mixed(pb, rb)
    Aa, Ba = pa["A"].copy(), pa["B"].copy()
    ca = BatchController(solver, pa["N"], Aa, Ba, pa["Q"], pa["R"], pa["P"], pa["lb"], pa["ub"])
    Aa[:] = np.nan                                          # the controller has copied what it needs
    Ba[:] = np.nan
    cb = controller(solver, pb)
    for c, q in ((ca, pa), (cb, pb)):
        nx, nu, Bsz = q["B"].shape
        n = q["N"] * nu
        assert 0 < c.nbytes <= (8 * (n * (n + 1) + n * nx + n + 2 * (nx * nx + nx * nu)) + 512) * Bsz, c.nbytes / Bsz
    roll_ref = orc.rollout_batch(10, *qa(pa), pa["x0"], pa["A"], pa["B"])
    for k in range(3):
        check(pa, ca.step(pa["x0"]), ra, f"a{k}")
        check(pb, solver.solve_batch(*qa(pb), pb["x0"]), rb, f"solve b{k}")
        check(pb, cb.step(pb["x0"]), rb, f"b{k}")
        got = solver.rollout_batch(10, *qa(pa), pa["x0"], pa["A"], pa["B"])
        assert np.all(got["status"] == 0) and rel(got["J_T"], roll_ref["J_T"]) <= BAR
        check(pa, solver.solve_batch(*qa(pa), pa["x0"]), ra, f"solve a{k}")
    for c in ((ca, cb) if order == 0 else (cb, ca)):
        c.close()
    check(pa, solver.solve_batch(*qa(pa), pa["x0"]), ra, "after close")


# ---------------- 7. it has to pay ----------------
def test_a_step_is_cheaper_than_a_solve(solver):
    b = synth.make_batch(3)
    nx, nu, Bsz = b["B"].shape
    N = b["N"]
    assert (nx, nu, N, Bsz) == (4, 2, 10, 65536)
    dA, dB, dx = (DevArray(b[k].shape, init=b[k]) for k in ("A", "B", "x0"))
    du, dv = DevArray((nu, Bsz)), DevArray(Bsz)
    solver.reserve(nx, nu, N, Bsz)
    with BatchController(solver, N, dA, dB, b["Q"], b["R"], b["P"], b["lb"], b["ub"]) as ctl:
        assert "ctl" in ctl.kernel

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
              f"bytes/instance {ctl.nbytes / Bsz:.0f}")
        assert tc < ts, (tc, ts)
        assert tw < ts, (tw, ts)
