"""GPU (-m gpu): the probe without its record staging (lqmpc_probe.h, build_order).  Under the roll key (shared plant, zero
references, centred box) a rollout on the 16-lane-row kernels with four instances a wavefront stages no records: the probe reads x0
alone, 256 instances a workgroup, and the sorted walk reads the instance-minor arrays through the permutation.  The free-response
key, the kernels with a wavefront per instance and the fused sweep keep the staged [A | B | x0] records.  Through the C ABI,
which does not tell which key or which staging a call took: a case is named after the path its inputs select in make_plan and
build_order, and what it verifies is the result of the call.

Every case compares order = 1 against order = 0 of the same call bit for bit on J_T, U, X, status and iters (trajectories wanted,
T = 6 unless the case is about T): the order only decides which instances share a wavefront, and a record staged for the wrong
instance or cut short, or an array read through the wrong slot of the permutation, changes X at step 1.  One size is also
checked against the CPU oracle with the tolerances of test_gpu_order_passes.py (TIGHT on J_T, RTOL on U and X).
"""
import ctypes

import numpy as np
import pytest

from lq_mpc_amd import synth
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


def cut(b, n, start=0):
    """n instances of a batch from `start` on."""
    sl = slice(start, start + n)
    return dict(b, Bsz=n, A=np.ascontiguousarray(b["A"][:, :, sl]), B=np.ascontiguousarray(b["B"][:, :, sl]),
                x0=np.ascontiguousarray(b["x0"][:, sl]))


def rollout(s, b, T, order, **kw):
    s.set_options(order=order)
    return s.rollout_batch(T, b["N"], b["A"], b["B"], b["Q"], b["R"], b["P"], b["lb"], b["ub"], b["x0"],
                           kw.pop("A_true", b["A_true"]), kw.pop("B_true", b["B_true"]), want_traj=True, **kw)


def same(r0, r1):
    for k in FIELDS:
        assert np.array_equal(r0[k], r1[k]), k


def hiprtc_loadable():
    """Whether the run-time compiler's library is on the machine (the names lqmpc_jit.hip tries); decided before any compile."""
    for name in ("libhiprtc.so", "libhiprtc.so.7", "/opt/rocm/lib/libhiprtc.so"):
        try:
            ctypes.CDLL(name)
            return True
        except OSError:
            pass
    return False


@pytest.fixture(scope="module")
def c3(golden_dir):
    """A C3 batch of 1 031 instances, computed once; the tests cut prefixes and leave it unchanged."""
    return synth.make_batch(3, Bsz=1031, fixture_dir=golden_dir)


@pytest.mark.parametrize("bsz", [255, 256, 257, 511, 513])
def test_sizes_around_the_probe_workgroup(solver, c3, bsz):
    """A probe workgroup takes 256 instances: the last one is partial (255, 257, 511, 513) or full (256), and a second or third
    one exists or not.  513 also against the CPU oracle."""
    b = cut(c3, bsz)
    try:
        r0 = rollout(solver, b, 6, 0)
        r1 = rollout(solver, b, 6, 1)
    finally:
        solver.set_options(**RESET)
    same(r0, r1)
    assert np.all(r1["status"] == 0)
    if bsz == 513:
        ref = orc.rollout_batch(6, b["N"], b["A"], b["B"], b["Q"], b["R"], b["P"], b["lb"], b["ub"], b["x0"], b["A_true"], b["B_true"],
                                want_traj=True)
        assert rel(r1["J_T"], ref["J_T"]) < TIGHT and u_err(r1["U"], ref["U"]) < RTOL
        assert np.max(np.abs(r1["X"] - ref["X"])) < RTOL * np.max(np.abs(ref["X"]))


def test_the_two_probe_paths_alternate_on_one_handle(solver, c3):
    """Roll key (1 031 instances), free-response key (257, per-instance plants), roll key (63), back to back with the order on:
    each call counts into the counters, and starts from the hand-back count, that the call before it zeroed, whichever path that
    took.  The three calls hold different instances at the same indices (the first 1 031, 257 from 700 on, the last 63 in
    reverse), so a roll-key call that read the records the free-response call staged, or the free-response call reading through
    the first call's slots, would change X at step 1."""
    rng = np.random.default_rng(7)
    mid, last = cut(c3, 257, 700), cut(c3, 63, 968)
    last = dict(last, A=np.ascontiguousarray(last["A"][:, :, ::-1]), B=np.ascontiguousarray(last["B"][:, :, ::-1]),
                x0=np.ascontiguousarray(last["x0"][:, ::-1]))
    assert not np.array_equal(last["x0"], c3["x0"][:, :63]) and not np.array_equal(last["x0"], mid["x0"][:, :63])
    assert not np.array_equal(last["A"], mid["A"][:, :, :63]) and not np.array_equal(mid["x0"], c3["x0"][:, :257])
    per = dict(A_true=np.ascontiguousarray(c3["A_true"][:, :, None] + 1e-3 * rng.standard_normal((4, 4, 257))),
               B_true=np.ascontiguousarray(c3["B_true"][:, :, None] + 1e-3 * rng.standard_normal((4, 2, 257))))
    try:
        r0 = [rollout(solver, c3, 6, 0), rollout(solver, mid, 6, 0, **dict(per)), rollout(solver, last, 6, 0)]
        r1 = [rollout(solver, c3, 6, 1), rollout(solver, mid, 6, 1, **dict(per)), rollout(solver, last, 6, 1)]
    finally:
        solver.set_options(**RESET)
    for a, c in zip(r0, r1):
        same(a, c)
        assert np.all(c["status"] == 0)


def test_large_records_under_the_roll_key(solver):
    """(5,3,4) x 257 on a shared plant, centred box, no references: the roll key on a run-time compiled shape whose records (45
    doubles) would not fit the probe's LDS piece; no record is staged, and the 255 surplus lanes of the last workgroup store no key."""
    if not hiprtc_loadable():
        pytest.skip("run-time compile unavailable: libhiprtc.so cannot be loaded on this machine")
    nx, nu, N, Bsz = 5, 3, 4, 257
    rng = np.random.default_rng(5341)
    A = rng.standard_normal((nx, nx, Bsz))
    A *= rng.uniform(0.4, 1.0, Bsz) / np.abs(np.linalg.eigvals(A.transpose(2, 0, 1))).max(axis=1)
    B = rng.standard_normal((nx, nu, Bsz)) * rng.uniform(0.2, 1.5, (1, 1, Bsz))
    At = rng.standard_normal((nx, nx))
    At *= 0.9 / np.abs(np.linalg.eigvals(At)).max()
    b = dict(N=N, A=np.ascontiguousarray(A), B=np.ascontiguousarray(B), Q=np.eye(nx), R=0.3 * np.eye(nu), P=2.5 * np.eye(nx),
             lb=-np.full(nu, 0.2), ub=np.full(nu, 0.2), x0=rng.standard_normal((nx, Bsz)) * rng.choice([1e-2, 0.3, 1.0, 3.0], Bsz),
             A_true=np.ascontiguousarray(At), B_true=np.ascontiguousarray(rng.standard_normal((nx, nu))))
    try:
        r0 = rollout(solver, b, 6, 0)
        assert "jit" in solver.last_kernel() and "<5,3,4>" in solver.last_kernel()
        r1 = rollout(solver, b, 6, 1)
        assert "jit" in solver.last_kernel() and "<5,3,4>" in solver.last_kernel()       # no fall-back under the order
    finally:
        solver.set_options(**RESET)
    same(r0, r1)


def test_c2_records_under_the_roll_key(solver, golden_dir):
    """(2,1,10) x 257: another record length (7 doubles, odd) and another stride of the arrays read through the permutation."""
    b = synth.make_batch(2, Bsz=257, fixture_dir=golden_dir)
    try:
        r0 = rollout(solver, b, 6, 0)
        r1 = rollout(solver, b, 6, 1)
    finally:
        solver.set_options(**RESET)
    same(r0, r1)
    assert np.all(r1["status"] == 0)


@pytest.mark.parametrize("T", [1, 40])
def test_shortest_and_long_rollouts(solver, c3, T):
    """The roll runs min(T, 31) steps: one step, and more steps than the roll follows; the key stays inside the buckets."""
    b = cut(c3, 257)
    try:
        r0 = rollout(solver, b, T, 0)
        r1 = rollout(solver, b, T, 1)
    finally:
        solver.set_options(**RESET)
    same(r0, r1)


def test_a_wavefront_per_instance_keeps_its_records(solver, golden_dir):
    """C4 (4,2,20: n = 40, one instance per wavefront) x 257 on a shared plant: build_order keeps the staged records for this
    kernel, so the probe computes the roll key and lays the records out in LDS in one body."""
    b = synth.make_batch(4, Bsz=257, fixture_dir=golden_dir)
    try:
        r0 = rollout(solver, b, 6, 0)
        r1 = rollout(solver, b, 6, 1)
    finally:
        solver.set_options(**RESET)
    same(r0, r1)
