"""GPU (-m gpu): the host flavour of every entry point against its _dev twin, bit for bit, on both sides of the stager's PACK_LIMIT.

Shape (4, 2, 10), T = 5, K = 4.  67 instances: every call totals under 64 KiB and goes up and comes back as one packed block
(bounds_batch excepted, which copies array by array at every size).  2 051 instances for the calls that carry A and B, 16 387 for
the controller's step (64 bytes an instance): every call totals over PACK_LIMIT and is copied array by array.  The odd sizes leave the last wavefront and the last 256-byte slot partly filled.  Each
entry point runs once with all optional outputs and once with none; both flavours run on the same handle under the same options.
The twin's arrays are device buffers from the HIP runtime the library loaded (DevArray: torch sees no GPU in this process once the
library has opened the device).
"""
import ctypes

import numpy as np
import pytest

from lq_mpc_amd import BatchController, _lib
from lq_mpc_amd.mpc import _ptr
from test_gpu_controller import DevArray, problem

pytestmark = pytest.mark.gpu

NX, NU, N, T, K = 4, 2, 10, 5, 4
PACK_LIMIT = 256 * 1024
SMALL, LARGE, LARGE_STEP = 67, 2051, 16387
F8, I4 = np.float64, np.int32
UNWRITTEN = {F8: -1.2345e300, I4: -7}             # what the outputs hold before a call


class In:
    """a per-instance input array"""
    def __init__(self, a, dtype=F8):
        self.a = np.ascontiguousarray(a, dtype=dtype)


class Out:
    """a per-instance output array; want=False: the caller passes NULL"""
    def __init__(self, shape, dtype=F8, want=True):
        self.shape, self.dtype, self.want = shape, dtype, want


def call(solver, fn, args, dev):
    """fn(*args) with every In / Out as a host array (dev=False) or a device buffer; the outputs as host arrays, and the call's bytes"""
    cargs, outs, keep, total = [], [], [], 0
    for a in args:
        if isinstance(a, In):
            total += a.a.nbytes
            buf = DevArray(a.a.shape, a.a.dtype, init=a.a) if dev else a.a
        elif isinstance(a, Out):
            if not a.want:
                cargs.append(None)
                continue
            fill = np.full(a.shape, UNWRITTEN[a.dtype], dtype=a.dtype)
            total += fill.nbytes
            buf = DevArray(a.shape, a.dtype, init=fill) if dev else fill
            outs.append(buf)
        else:
            cargs.append(_ptr(a) if isinstance(a, np.ndarray) else a)
            continue
        keep.append(buf)
        cargs.append(_ptr(buf))
    _lib.check(fn(*cargs))
    if dev:
        solver.sync()
    return [o.numpy() if dev else o for o in outs], total


def same(solver, name, args, Bsz, between=lambda: None):
    L = solver._L
    host, total = call(solver, getattr(L, name), args, False)
    between()
    twin, _ = call(solver, getattr(L, name + "_dev"), args, True)
    assert total < 64 * 1024 if Bsz == SMALL else total > PACK_LIMIT, (name, Bsz, total)
    assert len(host) == len(twin)
    for k, (a, b) in enumerate(zip(host, twin)):
        assert not np.any(b == UNWRITTEN[b.dtype.type]), (name, Bsz, k)
        assert a.tobytes() == b.tobytes(), (name, Bsz, k, int(np.sum(a != b)))
    return host


@pytest.fixture(scope="module")
def batches():
    return {Bsz: problem(NX, NU, N, Bsz, 5) for Bsz in (SMALL, LARGE, LARGE_STEP)}


def shared(p):
    return [p[k] for k in ("Q", "R", "P", "lb", "ub")]


@pytest.mark.parametrize("opt", [True, False], ids=["all", "none"])
@pytest.mark.parametrize("Bsz", [SMALL, LARGE])
def test_one_shot_entry_points(solver, batches, Bsz, opt):
    p = batches[Bsz]
    h, dims, A, B, x0 = solver._h, [NX, NU, N, Bsz], In(p["A"]), In(p["B"]), In(p["x0"])
    st, it = Out((Bsz,), I4, opt), Out((Bsz,), I4, opt)
    rng = np.random.default_rng(3)
    x0s = np.ascontiguousarray(rng.standard_normal((NX, K)))
    At, Bt = np.ascontiguousarray(p["A"][..., 0]), np.ascontiguousarray(p["B"][..., 0])
    same(solver, "lqmpc_solve_batch", [h] + dims + [A, B] + shared(p) + [x0, None, None, Out((NU, Bsz)), Out((Bsz,)), st, it], Bsz)
    # the rollout with trajectories (shared plant) and without (a plant per instance: two more arrays)
    roll = [h] + dims + [T, A, B] + shared(p) + [x0]
    if opt:
        same(solver, "lqmpc_rollout_batch", roll + [At, Bt, 0, None, None, Out((Bsz,)), Out((NX, T + 1, Bsz)), Out((NU, T, Bsz)), st, it], Bsz)
    else:
        same(solver, "lqmpc_rollout_batch", roll + [In(p["A"]), In(p["B"]), 1, None, None, Out((Bsz,)), Out(0, want=False), Out(0, want=False),
                                                    st, it], Bsz)
    mv = same(solver, "lqmpc_max_vn_batch", [h] + dims + [K, A, B] + shared(p) + [x0s, None, None, Out((Bsz,)), st, it], Bsz)[0]
    same(solver, "lqmpc_sweep_batch", [h] + dims + [T, K, A, B] + shared(p) + [x0, x0s, At, Bt, 0, None, None, Out((Bsz,)), Out((Bsz,)), st, it], Bsz)
    e = In(rng.uniform(1e-3, 1e-2, Bsz))
    same(solver, "lqmpc_bounds_batch", [h] + dims + [A, B, p["Q"], p["R"], p["lb"], p["ub"], e, e, In(mv), 0.2 * x0s[:, 0].copy(),
                                                     np.array([0.3, 1.5, 0.7]), 1.7, Out((NU, NX, Bsz))] + [Out((Bsz,)) for _ in range(6)] +
         [Out((8, Bsz), want=opt), Out((Bsz,), I4, opt)], Bsz)


def controller(solver, p):
    return BatchController(solver, p["N"], p["A"], p["B"], p["Q"], p["R"], p["P"], p["lb"], p["ub"])


@pytest.mark.parametrize("opt", [True, False], ids=["all", "none"])
@pytest.mark.parametrize("Bsz", [SMALL, LARGE_STEP])
def test_controller_step(solver, batches, Bsz, opt):
    p = batches[Bsz]
    with controller(solver, p) as ctl:
        args = [ctl._c, In(p["x0"]), Out((NU, Bsz)), Out((Bsz,), want=opt), Out((Bsz,), I4, opt), Out((Bsz,), I4, opt)]
        same(solver, "lqmpc_controller_step", args, Bsz, between=ctl.reset)         # (both flavours from a cold start)


@pytest.mark.parametrize("opt", [True, False], ids=["all", "none"])
@pytest.mark.parametrize("Bsz", [SMALL, LARGE])
def test_controller_rollout_and_set_model(solver, batches, Bsz, opt):
    p = batches[Bsz]
    rng = np.random.default_rng(9)
    with controller(solver, p) as ctl:
        traj = [Out((NX, T + 1, Bsz), want=opt), Out((NU, T, Bsz), want=opt), Out((Bsz,), I4, opt), Out((Bsz,), I4, opt)]
        same(solver, "lqmpc_controller_rollout", [ctl._c, T, In(p["x0"]), In(p["A"]), In(p["B"]), 1, Out((Bsz,))] + traj, Bsz)
        # new models for all instances but three, in a shuffled order, through each flavour; then the same host-flavour step
        step = [ctl._c, In(p["x0"]), Out((NU, Bsz)), Out((Bsz,)), Out((Bsz,), I4), Out((Bsz,), I4)]
        ctl.reset()
        before = call(solver, solver._L.lqmpc_controller_step, step, False)[0]
        idx = rng.permutation(Bsz)[:Bsz - 3].astype(I4)
        A2 = p["A"][..., idx] + 0.05 * rng.standard_normal((NX, NX, idx.size))
        B2 = p["B"][..., idx] + 0.05 * rng.standard_normal((NX, NU, idx.size))
        got = []
        for dev in (False, True):
            ctl.set_model(p["A"], p["B"])
            fn = solver._L.lqmpc_controller_set_model_dev if dev else solver._L.lqmpc_controller_set_model
            _, total = call(solver, fn, [ctl._c, ctypes.c_int64(idx.size), In(idx, I4), In(A2), In(B2)], dev)
            assert total < 64 * 1024 if Bsz == SMALL else total > PACK_LIMIT, total
            ctl.reset()
            got.append(call(solver, solver._L.lqmpc_controller_step, step, False)[0])
        for a, b in zip(*got):
            assert a.tobytes() == b.tobytes()
        assert not np.array_equal(got[0][0], before[0])
