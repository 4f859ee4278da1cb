"""GPU (-m gpu): lq_mpc_amd.torch_layer.MPCLayer.plan differentiated with respect to the state and the model, layer.plan(x, A, B), on
(4,2,10) x 64 (the problems of tests/sens_ref.py).  The GPU part runs in tests/torch_layer_plan_job.py, a process of its own in which
torch opens the GPU first; here its records are checked.

  loss = ((Uplan - U_e) ** 2).sum() + ((Xplan[:, 1:] - X_e) ** 2).sum() + 0.1 * VN.sum()   for seeded targets U_e, X_e (0.1 x standard normal)
  x.grad, A.grad, B.grad = g_x0, g_A, g_B of the NumPy interface (BatchController.plan_grad) for gUplan = 2 (Uplan - U_e),
    gXplan = [0, 2 (Xplan[:, 1:] - X_e)], gVN = 0.1, at 1e-12 relative to max(|grad|_max, 1);
  <A.grad, dA> + <B.grad, dB> for one seeded random direction per instance (standard normal entries) = the long-double central
    difference of the reference loss, exact.certify at the models A +- STEP dA, B +- STEP dB, at 1e-6 relative to max(|fd|_max, 1), on
    the instances whose face is the same at all three models; those must be at least 80 % of the batch.  STEP = 1e-5 and SEED = 4 were
    chosen on the CPU with the oracle alone: the long-double formula (pgrad_ref.reference) meets the difference to 2.2e-9 on 64 of 64
    instances (the loss is not quadratic in the model, so the difference has a remainder of order STEP ** 2); the bar is that figure
    with the margin tests/test_gpu_torch_layer_grad.py gives its own 2.4e-9, 1e-6;
  backward after an intervening set_model raises;
  forward and backward behind a busy stream leave an event recorded in front of them pending: nothing waited for the host."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pgrad_ref as pg
import sens_ref as sr
from oracle import exact as ex

pytestmark = pytest.mark.gpu

LD = np.longdouble
BSZ = 64
STEP = 1e-5
SEED = 4
SHAPE = (4, 2, 10)


def scale(g):
    return max(float(np.max(np.abs(g))), 1.0)


def targets():
    nx, nu, N = SHAPE
    rng = np.random.default_rng(40 + SEED)
    return 0.1 * rng.standard_normal((nu, N, BSZ)), 0.1 * rng.standard_normal((nx, N, BSZ))


def direction(p):
    rng = np.random.default_rng(SEED)
    return rng.standard_normal(p["A"].shape), rng.standard_normal(p["B"].shape)


def exact_plan(q, x0, cert):
    """the certified plan and its states in long double, (nu, N, Bsz) and (nx, N + 1, Bsz)"""
    N, nx, Bsz = q["N"], q["A"].shape[0], x0.shape[1]
    Al, Bl = np.moveaxis(np.asarray(q["A"], dtype=LD), -1, 0), np.moveaxis(np.asarray(q["B"], dtype=LD), -1, 0)
    Phi, Gam = ex.prediction(N, Al, Bl)
    x0l = np.asarray(x0, dtype=LD).T
    Us = np.moveaxis(cert["U"], -1, 0).transpose(0, 2, 1).reshape(Bsz, -1)
    X = (np.einsum("bij,bj->bi", Phi, x0l) + np.einsum("bij,bj->bi", Gam, Us)).reshape(Bsz, N, nx)
    return cert["U"], np.concatenate([x0l[:, None, :], X], axis=1).transpose(2, 1, 0)


def reference_loss(q, x0, cert):
    U_e, X_e = targets()
    U, X = exact_plan(q, x0, cert)
    return np.sum((U - U_e) ** 2, axis=(0, 1)) + np.sum((X[:, 1:] - X_e) ** 2, axis=(0, 1)) + LD(0.1) * cert["V"]


def central_difference(p, dA, dB):
    """per instance: the long-double central difference of the reference loss along (dA, dB), and whether the face is the same at
    the three models"""
    def at(s):
        q = dict(p, A=np.ascontiguousarray(p["A"] + s * STEP * dA), B=np.ascontiguousarray(p["B"] + s * STEP * dB))
        c = ex.certify(*sr.qa(q), p["x0"], sr.oracle_plan(q, p["x0"], {}))
        # the step the perturbed fp64 models really took
        return reference_loss(q, p["x0"], c), sr.face_of(c["U"], p["lb"], p["ub"]), q
    (Lp, fp, qp), (Lm, fm, qm), (_, f0, _) = at(1), at(-1), at(0)
    # <g, d> with d the difference of the two models that were really used, in long double
    hA = (np.asarray(qp["A"], dtype=LD) - np.asarray(qm["A"], dtype=LD)) / 2
    hB = (np.asarray(qp["B"], dtype=LD) - np.asarray(qm["B"], dtype=LD)) / 2
    same = np.all(fp == f0, axis=(0, 1)) & np.all(fm == f0, axis=(0, 1))
    return (Lp - Lm) / 2, hA, hB, same


def test_step_and_seed_meet_the_condition_on_the_reference_alone():
    """no GPU in this one: the choice of STEP and SEED, checked with the oracle and the long-double formula"""
    c = sr.case(SHAPE, bsz=BSZ)
    p = c["p"]
    dA, dB = direction(p)
    dL, hA, hB, same = central_difference(p, dA, dB)
    U_e, X_e = targets()
    U, X = exact_plan(p, p["x0"], ex.certify(*sr.qa(p), p["x0"], c["U"]))
    gX = np.zeros(X.shape)
    gX[:, 1:] = np.asarray(2 * (X[:, 1:] - X_e), dtype=np.float64)
    ref = pg.reference(p, {}, p["x0"], c["U"], np.asarray(2 * (U - U_e), dtype=np.float64), gX, np.full(BSZ, 0.1))
    lin = np.sum(ref["g_A"] * hA, axis=(0, 1)) + np.sum(ref["g_B"] * hB, axis=(0, 1))
    err = float(np.max(np.abs(lin - dL)[same])) / (STEP * scale(np.asarray(dL[same] / STEP, dtype=np.float64)))
    print(f"the formula against the central difference: {err:.2e} on {int(same.sum())} of {BSZ} instances")
    assert same.sum() >= 0.8 * BSZ
    assert err <= 1e-6


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    c = sr.case(SHAPE, bsz=BSZ)
    p = c["p"]
    tmp = tmp_path_factory.mktemp("torch_layer_plan")
    inp, outp = str(tmp / "in.npz"), str(tmp / "out.npz")
    U_e, X_e = targets()
    np.savez(inp, U_e=U_e, X_e=X_e, **p)
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "torch_layer_plan_job.py")
    r = subprocess.run([sys.executable, script, inp, outp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return c, dict(np.load(outp))


def test_gradients_equal_the_numpy_interface(job):
    c, out = job
    assert "ctl_r16" in str(out["kernel"]) and np.all(out["np_status"] == 0)
    assert np.array_equal(out["U_plan"], out["np_U_plan"]) and np.array_equal(out["U_plan"], out["plain_U_plan"])
    assert np.array_equal(out["X_plan"][:, 0], c["p"]["x0"])
    for k, want in (("x_grad", out["np_g_x0"]), ("A_grad", out["np_g_A"]), ("B_grad", out["np_g_B"])):
        e = float(np.max(np.abs(out[k] - want))) / scale(want)
        print(f"{k} against the NumPy interface: {e:.2e}")
        assert e <= 1e-12
        assert float(np.max(np.abs(out[k + "_again"] - want))) / scale(want) <= 1e-12
    assert float(np.max(np.abs(out["plain_x_grad"] - out["np_g_x0"]))) / scale(out["np_g_x0"]) <= 1e-12


def test_model_gradient_equals_a_long_double_central_difference(job):
    c, out = job
    p = c["p"]
    dA, dB = direction(p)
    dL, hA, hB, same = central_difference(p, dA, dB)
    lin = np.sum(out["A_grad"] * hA, axis=(0, 1)) + np.sum(out["B_grad"] * hB, axis=(0, 1))
    err = float(np.max(np.abs(lin - dL)[same])) / (STEP * scale(np.asarray(dL[same] / STEP, dtype=np.float64)))
    print(f"<A.grad, dA> + <B.grad, dB> against the central difference: {err:.2e} on {int(same.sum())} of {BSZ} instances "
          f"({same.mean():.0%})")
    assert same.sum() >= 0.8 * BSZ
    assert err <= 1e-6


def test_backward_after_an_intervening_set_model_raises(job):
    _, out = job
    assert bool(out["raised"]) and "set_model" in str(out["raised_message"])


def test_forward_and_backward_do_not_wait_for_the_host(job):
    _, out = job
    print(f"plan forward and backward with A and B: {float(out['host_seconds']) * 1e3:.2f} ms on the host, event pending: {bool(out['event_pending'])}")
    assert bool(out["event_pending"])
