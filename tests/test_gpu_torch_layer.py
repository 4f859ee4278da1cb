"""GPU (-m gpu): lq_mpc_amd.torch_layer.MPCLayer, the controller's step as a differentiable torch layer, on (4,2,10) x 64 (the problems
of tests/test_gpu_plan.py).  The GPU part runs in tests/torch_layer_job.py, a process of its own in which torch opens the GPU first;
here its records are checked.

  loss = (u_0 ** 2).sum() + 0.1 * V_N.sum()
  x.grad = 2 K_0' u_0 + 0.1 dV_dx with K_0, dV_dx, u_0 from the NumPy interface, at 1e-12 relative to max(|grad|_max, 1);
  x.grad = the long-double central difference of the reference loss, exact.certify at x +- 1e-4 e_a, on the instances whose face is the
    same at all three states, at 1e-6 relative to max(|grad|_max, 1) (on a face u_0 is affine and V_N quadratic in x, so the loss is
    quadratic and the difference has no remainder of its own; measured 3.8e-15 on 64 of 64 instances);
  two forwards and one backward behind a busy stream leave an event recorded in front of them pending: nothing waited for the host."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sens_ref as sr
from oracle import exact as ex

pytestmark = pytest.mark.gpu

LD = np.longdouble
BSZ = 64
STEP = 1e-4


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    c = sr.case((4, 2, 10), bsz=BSZ)
    p = c["p"]
    tmp = tmp_path_factory.mktemp("torch_layer")
    inp, outp = str(tmp / "in.npz"), str(tmp / "out.npz")
    np.savez(inp, **p)
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "torch_layer_job.py")
    r = subprocess.run([sys.executable, script, inp, outp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return c, dict(np.load(outp))


def scale(g):
    return max(float(np.max(np.abs(g))), 1.0)


def test_gradient_equals_the_numpy_interface(job):
    c, out = job
    assert "ctl_r16" in str(out["kernel"]) and np.all(out["np_status"] == 0)
    assert np.array_equal(out["u_0"], out["np_u_0"])
    want = 2.0 * np.einsum("kab,kb->ab", out["np_K_0"], out["np_u_0"]) + 0.1 * out["np_dV_dx"]
    e = float(np.max(np.abs(out["x_grad"] - want))) / scale(want)
    print(f"x.grad against 2 K_0'u_0 + 0.1 dV_dx: {e:.2e}")
    assert e <= 1e-12
    # (a later step at the same state is warm-started from the stored face: the same optimum, to rounding)
    assert float(np.max(np.abs(out["x_grad_again"] - want))) / scale(want) <= 1e-12


def test_gradient_equals_a_long_double_central_difference(job):
    c, out = job
    p, x0 = c["p"], c["p"]["x0"]
    nx = x0.shape[0]

    def at(x):
        """loss per instance in long double, and the face, at the states x"""
        s = ex.certify(*sr.qa(p), x, sr.oracle_plan(p, x, {}))
        return np.sum(s["u_0"] ** 2, axis=0) + LD(0.1) * s["V"], sr.face_of(s["U"], p["lb"], p["ub"])
    _, f0 = at(x0)
    fd = np.zeros(x0.shape, dtype=LD)
    same = np.ones(BSZ, dtype=bool)
    for a in range(nx):
        e = np.zeros_like(x0)
        e[a] = STEP
        xp, xm = x0 + e, x0 - e
        (Lp, fp), (Lm, fm) = at(xp), at(xm)
        fd[a] = (Lp - Lm) / (np.asarray(xp[a], dtype=LD) - np.asarray(xm[a], dtype=LD))
        same &= np.all(fp == f0, axis=(0, 1)) & np.all(fm == f0, axis=(0, 1))
    err = float(np.max(np.abs(out["x_grad"] - fd)[:, same])) / scale(np.asarray(fd[:, same], dtype=np.float64))
    print(f"x.grad against the central difference: {err:.2e} on {int(same.sum())} of {BSZ} instances")
    assert same.sum() >= 0.8 * BSZ
    assert err <= 1e-6


def test_forward_and_backward_do_not_wait_for_the_host(job):
    _, out = job
    print(f"two forwards and one backward: {float(out['host_seconds']) * 1e3:.2f} ms on the host, event pending: {bool(out['event_pending'])}")
    assert bool(out["event_pending"])
