"""GPU (-m gpu): the set-up of the 16-lane-row rollout kernels with one round of global loads and P built inside the sweep
(lqmpc_r16_setup.h, ONE_TRIP; switched on for the C3 rollout kernel of the throughput build, R16Build::ONE_TRIP).

What can go wrong there, at the smallest sizes at which it can: the instance of an MFMA block taken from the permutation's one load
(ragged last wavefronts, with and without a permutation), P read by the mixed iteration (hard mix), and the values parked in LDS
across the set-up (per-instance plant, x0, box, weights).  C2 runs the parent's set-up through the same cases.
Tolerances as in test_gpu_parity.py.
"""
import functools

import numpy as np
import pytest

from lq_mpc_amd import synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

RTOL = 1e-5
TIGHT = 1e-8
U_MAX = 0.1
T_ROLL = 5


def rel(a, b):
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))


def u_err(u, ur, umax=U_MAX):
    return np.max(np.abs(u - ur) / np.maximum(np.abs(ur), 1e-3 * umax))


def args(b):
    return (b["N"], b["A"], b["B"], b["Q"], b["R"], b["P"], b["lb"], b["ub"])


@functools.lru_cache(maxsize=None)
def case(cfg, bsz, mix):
    """One batch and its oracle results, computed once and shared (read only)."""
    b = synth.make_batch(cfg, Bsz=bsz, mix=mix)
    roll = orc.rollout_batch(T_ROLL, *args(b), b["x0"], b["A_true"], b["B_true"], want_traj=True)
    one = orc.solve_batch(*args(b), b["x0"])
    return b, roll, one


@pytest.fixture
def tsolver(solver):
    """The throughput build (two waves per SIMD) at every batch size: the build the changed set-up is in."""
    solver.set_options(r16_build=0)
    yield solver
    solver.set_options(r16_build=-1, order=-1)


@pytest.mark.parametrize("mix", ["default", "hard"])
@pytest.mark.parametrize("bsz", [1, 3, 5, 257])
@pytest.mark.parametrize("cfg", [3, 2])
def test_ragged_wavefronts_and_both_instance_lookups(tsolver, cfg, bsz, mix):
    b, roll, one = case(cfg, bsz, mix)
    got = {}
    for order in (0, 1):
        tsolver.set_options(order=order)
        g = tsolver.rollout_batch(T_ROLL, *args(b), b["x0"], b["A_true"], b["B_true"])              # the chunk path
        assert "r16" in tsolver.last_kernel()
        gt = tsolver.rollout_batch(T_ROLL, *args(b), b["x0"], b["A_true"], b["B_true"], want_traj=True)
        g1 = tsolver.solve_batch(*args(b), b["x0"])
        for r in (g, gt):
            assert r["J_T"].shape == (bsz,) and np.all(r["status"] == 0)
            assert rel(r["J_T"], roll["J_T"]) < TIGHT
        assert u_err(gt["U"], roll["U"]) < RTOL
        assert np.all(g1["status"] == 0)
        assert rel(g1["V_N"], one["V_N"]) < TIGHT and u_err(g1["u_0"], one["u_0"]) < RTOL
        if mix == "hard":
            # the batch takes the mixed (P-reading) iteration: a step-0 face of more than n/2 + 2 rows needs a second iteration at least
            assert g["iters"].max() >= 2
        got[order] = g
    # the order only decides who shares a wavefront
    assert np.array_equal(got[0]["J_T"], got[1]["J_T"]) and np.array_equal(got[0]["iters"], got[1]["iters"])


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("what", ["per-instance plant", "references", "off-centre box"])
def test_paths_whose_loads_move(tsolver, what, order):
    rng = np.random.default_rng(11)
    b = synth.make_batch(3, Bsz=65)
    nx, nu, N, Bsz = 4, 2, b["N"], 65
    lb, ub, At, Bt, ref_args = b["lb"], b["ub"], b["A_true"], b["B_true"], ()
    if what == "per-instance plant":
        At = np.ascontiguousarray(b["A_true"][:, :, None] + 1e-3 * rng.standard_normal((nx, nx, Bsz)))
        Bt = np.ascontiguousarray(b["B_true"][:, :, None] + 1e-3 * rng.standard_normal((nx, nu, Bsz)))
    elif what == "references":
        ref_args = (0.05 * rng.standard_normal((nx, N)), 0.02 * rng.standard_normal((nu, N)))
    else:
        lb, ub = b["lb"] - 0.02, b["ub"] - 0.02
    a = (N, b["A"], b["B"], b["Q"], b["R"], b["P"], lb, ub)
    ref = orc.rollout_batch(T_ROLL, *a, b["x0"], At, Bt, *ref_args, want_traj=True)
    tsolver.set_options(order=order)
    g = tsolver.rollout_batch(T_ROLL, *a, b["x0"], At, Bt, *ref_args)
    assert "r16" in tsolver.last_kernel()
    gt = tsolver.rollout_batch(T_ROLL, *a, b["x0"], At, Bt, *ref_args, want_traj=True)
    for r in (g, gt):
        assert np.all(r["status"] == 0) and rel(r["J_T"], ref["J_T"]) < TIGHT
    assert u_err(gt["U"], ref["U"]) < RTOL
