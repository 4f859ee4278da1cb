"""GPU (-m gpu): the passes around an ordered rollout -- the difficulty probe (lqmpc_probe.h: 256 instances a workgroup, records
copied out through LDS, positions inside a bucket from an LDS histogram), the scatter (512 compact counters) and the packed
kernel's pass over a long hand-back list, whose count that probe zeroes -- through the C ABI.

The order only decides which instances share a wavefront, and order on / off run the same 16-lane-row code: the results must be
bit-identical.  Against the CPU oracle the tolerances are those of test_gpu_parity.py for rollouts (TIGHT on J_T, RTOL on U and X).
"""
import ctypes

import numpy as np
import pytest

from lq_mpc_amd import _lib, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

RTOL = 1e-5
TIGHT = 1e-8
U_MAX = 0.1
FIELDS = ("J_T", "U", "X", "status", "iters")
RESET = dict(order=-1, r16_maxit=12)


def rel(a, b):
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))


def u_err(u, ur, umax=U_MAX):
    return np.max(np.abs(u - ur) / np.maximum(np.abs(ur), 1e-3 * umax))


def cut(b, n):
    """The first n instances of a batch."""
    return dict(b, Bsz=n, A=np.ascontiguousarray(b["A"][:, :, :n]), B=np.ascontiguousarray(b["B"][:, :, :n]),
                x0=np.ascontiguousarray(b["x0"][:, :n]))


def rollout(s, b, T, order, **kw):
    s.set_options(order=order)
    return s.rollout_batch(T, b["N"], b["A"], b["B"], b["Q"], b["R"], b["P"], kw.pop("lb", b["lb"]), kw.pop("ub", b["ub"]), b["x0"],
                           kw.pop("A_true", b["A_true"]), kw.pop("B_true", b["B_true"]), want_traj=True, **kw)


def same(r0, r1, keep=None):
    for k in FIELDS:
        a, c = (r0[k], r1[k]) if keep is None else (r0[k][..., keep], r1[k][..., keep])
        assert np.array_equal(a, c), k


def against_oracle(g, ref):
    assert np.all(g["status"] == 0)
    assert rel(g["J_T"], ref["J_T"]) < TIGHT and u_err(g["U"], ref["U"]) < RTOL
    assert np.max(np.abs(g["X"] - ref["X"])) < RTOL * np.max(np.abs(ref["X"]))


@pytest.fixture(scope="module")
def batches(golden_dir):
    """C3 and C2 batches of 1 031 instances and their oracle rollouts (T = 6), computed once; the tests cut prefixes."""
    out = {}
    for cfg in (3, 2):
        b = synth.make_batch(cfg, Bsz=1031, fixture_dir=golden_dir)
        ref = orc.rollout_batch(6, b["N"], b["A"], b["B"], b["Q"], b["R"], b["P"], b["lb"], b["ub"], b["x0"], b["A_true"], b["B_true"],
                                want_traj=True)
        out[cfg] = (b, ref)
    return out


@pytest.mark.parametrize("cfg", [3, 2])
@pytest.mark.parametrize("bsz", [1, 63, 257, 1031])
def test_forced_order_ragged_batches(solver, batches, cfg, bsz):
    """Batches that are no multiple of 4, 64, 256 (the probe's workgroup), 512 (the scatter's) or 1 024."""
    b, ref = batches[cfg]
    c = cut(b, bsz)
    try:
        r0 = rollout(solver, c, 6, 0)
        r1 = rollout(solver, c, 6, 1)
    finally:
        solver.set_options(**RESET)
    same(r0, r1)
    against_oracle(r1, {k: ref[k][..., :bsz] for k in ("J_T", "U", "X")})


@pytest.mark.parametrize("case", ["per-instance plants", "references", "off-centre box"])
def test_free_response_key(solver, batches, case):
    """Each of these takes the free-response key instead of the clipped roll."""
    b = cut(batches[3][0], 257)
    rng = np.random.default_rng(7)
    kw = {}
    if case == "per-instance plants":
        kw = dict(A_true=np.ascontiguousarray(b["A_true"][:, :, None] + 1e-3 * rng.standard_normal((4, 4, 257))),
                  B_true=np.ascontiguousarray(b["B_true"][:, :, None] + 1e-3 * rng.standard_normal((4, 2, 257))))
    elif case == "references":
        kw = dict(x_ref=0.02 * rng.standard_normal((4, b["N"])), u_ref=0.01 * rng.standard_normal((2, b["N"])))
    else:
        kw = dict(lb=b["lb"] - 0.03, ub=b["ub"] - 0.03)
    try:
        r0 = rollout(solver, b, 6, 0, **dict(kw))
        r1 = rollout(solver, b, 6, 1, **dict(kw))
    finally:
        solver.set_options(**RESET)
    same(r0, r1)
    ref = orc.rollout_batch(6, b["N"], b["A"], b["B"], b["Q"], b["R"], b["P"], kw.get("lb", b["lb"]), kw.get("ub", b["ub"]), b["x0"],
                            kw.get("A_true", b["A_true"]), kw.get("B_true", b["B_true"]),
                            **{k: kw[k] for k in ("x_ref", "u_ref") if k in kw}, want_traj=True)
    against_oracle(r1, ref)


def test_one_bucket_and_many_buckets(solver, batches):
    """Every x0 equal (one bucket: 257 ranks from one LDS counter); x0 scaled geometrically over 2^-3 .. 2^12 so that the lanes
    of a wavefront land in different buckets, plus one instance with a NaN in x0 (last bucket)."""
    b = cut(batches[3][0], 257)
    one = dict(b, x0=np.ascontiguousarray(np.repeat(b["x0"][:, :1], 257, 1)))
    unit = b["x0"] / np.linalg.norm(b["x0"], axis=0) * np.linalg.norm(b["x0"][:, 0])
    many = dict(b, x0=np.ascontiguousarray(unit * 2.0 ** np.linspace(-3, 12, 257)))
    many["x0"][2, 100] = np.nan
    finite = np.arange(257) != 100
    try:
        for c, keep in ((one, None), (many, finite)):
            r0 = rollout(solver, c, 6, 0)
            r1 = rollout(solver, c, 6, 1)
            same(r0, r1, keep)
            assert r0["status"][100] == r1["status"][100]
    finally:
        solver.set_options(**RESET)


@pytest.mark.parametrize("order", [0, 1])
def test_hand_back_list_longer_than_the_grid(solver, golden_dir, order):
    """Hard mix, iteration cap 1: most of the 4 096 instances are handed back, and every one must be solved.  The premise is
    checked: `iters` sums the KKT solves of an instance's T steps, so an instance whose sum exceeds T under the default cap has a
    step that takes more than one, and under a cap of one that step hands it back."""
    T = 4
    b = synth.make_batch(3, Bsz=4096, fixture_dir=golden_dir, mix="hard")
    try:
        full = rollout(solver, b, T, 0)
        solver.set_options(r16_maxit=1)
        g = rollout(solver, b, T, order)
    finally:
        solver.set_options(**RESET)
    handed_back = int(np.sum(full["iters"] > T))
    print("instances handed back under a cap of one, at least:", handed_back)
    assert handed_back > 2048
    assert np.all(g["status"] == 0) and np.all(full["status"] == 0)
    assert rel(g["J_T"], full["J_T"]) < TIGHT and u_err(g["U"], full["U"]) < RTOL
    assert np.max(np.abs(g["X"] - full["X"])) < RTOL * np.max(np.abs(full["X"]))


def test_fused_sweep_under_order(solver, batches):
    b = cut(batches[3][0], 257)
    a = (b["N"], b["A"], b["B"], b["Q"], b["R"], b["P"], b["lb"], b["ub"])
    x0s = np.ascontiguousarray(1.5 * b["x0"][:, :6])
    try:
        solver.set_options(order=0)
        g0 = solver.sweep_batch(6, *a, b["x0"], x0s, b["A_true"], b["B_true"])
        solver.set_options(order=1)
        g1 = solver.sweep_batch(6, *a, b["x0"], x0s, b["A_true"], b["B_true"])
        assert "r16" in solver.last_kernel()
    finally:
        solver.set_options(**RESET)
    for k in ("M_V", "J_T", "status", "iters"):
        assert np.array_equal(g0[k], g1[k]), k
    assert np.all(g1["status"] == 0)


def hiprtc_loadable():
    """Whether the run-time compiler's library is on the machine (the names lqmpc_jit.hip tries); decided before any compile."""
    for name in ("libhiprtc.so", "libhiprtc.so.7", "/opt/rocm/lib/libhiprtc.so"):
        try:
            ctypes.CDLL(name)
            return True
        except OSError:
            pass
    return False


def test_run_time_compiled_shape_under_order(solver):
    """(4,2,12): the probe compiled at run time from the same header.  Skipped only where the machine has no hiprtc; with one, a
    compile error in any kernel of the shape (the probe is one of them) fails the test."""
    if not hiprtc_loadable():
        pytest.skip("run-time compile unavailable: libhiprtc.so cannot be loaded on this machine")
    assert _lib.jit_compile(4, 2, 12) == 5
    b = cut(synth.make_batch(3, Bsz=257), 257)
    b["N"] = 12
    try:
        r0 = rollout(solver, b, 6, 0)
        assert "jit" in solver.last_kernel() and "<4,2,12>" in solver.last_kernel()
        r1 = rollout(solver, b, 6, 1)
    finally:
        solver.set_options(**RESET)
    same(r0, r1)
    assert np.all(r1["status"] == 0)


def test_records_too_large_for_lds_under_order(solver):
    """(5,3,4): 256 records of 45 doubles exceed the probe's LDS piece, so every lane stores its own record, and the surplus lanes
    of the last workgroup (257 instances: 255 of them) must store nothing.  Order on / off bit for bit."""
    if not hiprtc_loadable():
        pytest.skip("run-time compile unavailable: libhiprtc.so cannot be loaded on this machine")
    nx, nu, N, Bsz = 5, 3, 4, 257
    rng = np.random.default_rng(534)
    A = rng.standard_normal((nx, nx, Bsz))
    A *= rng.uniform(0.4, 1.0, Bsz) / np.abs(np.linalg.eigvals(A.transpose(2, 0, 1))).max(axis=1)
    B = rng.standard_normal((nx, nu, Bsz)) * rng.uniform(0.2, 1.5, (1, 1, Bsz))
    b = dict(N=N, A=np.ascontiguousarray(A), B=np.ascontiguousarray(B), Q=np.eye(nx), R=0.3 * np.eye(nu), P=2.5 * np.eye(nx),
             lb=-np.full(nu, 0.2), ub=np.full(nu, 0.2), x0=rng.standard_normal((nx, Bsz)) * rng.choice([1e-2, 0.3, 1.0, 3.0], Bsz))
    b["A_true"], b["B_true"] = np.ascontiguousarray(0.95 * b["A"]), b["B"]
    try:
        r0 = rollout(solver, b, 6, 0)
        assert "jit" in solver.last_kernel() and "<5,3,4>" in solver.last_kernel()
        r1 = rollout(solver, b, 6, 1)
    finally:
        solver.set_options(**RESET)
    same(r0, r1)
    assert np.all(r1["status"] == 0)


def test_two_calls_back_to_back_on_one_handle(solver, batches):
    """1 031 then 257 instances: the second call counts into the set of counters the first call's probe zeroed, and its
    hand-back count is the one its own probe zeroes."""
    b, ref = batches[3]
    try:
        r0a, r0b = rollout(solver, b, 6, 0), rollout(solver, cut(b, 257), 6, 0)
        solver.set_options(order=1)
        r1a = rollout(solver, b, 6, 1)
        r1b = rollout(solver, cut(b, 257), 6, 1)
    finally:
        solver.set_options(**RESET)
    same(r0a, r1a)
    same(r0b, r1b)
    against_oracle(r1b, {k: ref[k][..., :257] for k in ("J_T", "U", "X")})
