"""GPU (-m gpu): lq_mpc_amd.torch_layer.MPCLayer differentiated with respect to the references, layer(x, x_ref=, u_ref=), on
(4,2,10) x 64 with non-zero references (the problems of tests/sens_ref.py).  The GPU part runs in tests/torch_layer_refs_job.py, a
process of its own in which torch opens the GPU first; here its records are checked.

  loss = sum_b m_b (|u_0|^2 + 0.1 V_N)_b, m the 0 / 1 mask of the instances whose face, by the oracle alone, is the same at the
    references and at the references moved by +- STEP along one seeded random direction (at most 1 % are left out);
  x_ref.grad, u_ref.grad (CPU tensors) = g_xref, g_uref of the NumPy interface (BatchController.cost_grad, reduce=True) for
    w = 2 m u_0, gam = 0.1 m, bit for bit: the same kernel on the same data; with A and B given as well, the same, and A.grad, B.grad
    those of BatchController.model_grad;
  <x_ref.grad, dXr> + <u_ref.grad, dUr> = the long-double central difference of the reference loss, exact.certify at the references
    +- STEP (dXr, dUr).  On a fixed face the loss is quadratic in the references, so the difference has no remainder and its own
    error is its rounding, eps_ld |loss| / STEP; the bar is what the GPU tests allow the kernel, the bar of tests/test_gpu_cgrad.py
    on every instance's own gradient (per instance, relative to max(|g|_max, 1)), carried through the inner product, plus the
    same bound on the summation, plus that rounding;
  backward after an intervening set_reference raises."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sens_ref as sr
from oracle import exact as ex
from test_cgrad_cpu import GPU_BAR

pytestmark = pytest.mark.gpu

LD = np.longdouble
BSZ = 64
STEP = 1e-4
SEED = 6


def direction(kw):
    rng = np.random.default_rng(SEED)
    return rng.standard_normal(kw["x_ref"].shape), rng.standard_normal(kw["u_ref"].shape)


def central_difference(p, kw, dXr, dUr):
    """per instance: the long-double central difference of |u_0|^2 + 0.1 V along (dXr, dUr), half the difference of the two sets of
    references that were really used, and whether the face is the same at the three"""
    def at(s):
        k2 = dict(x_ref=kw["x_ref"] + s * STEP * dXr, u_ref=kw["u_ref"] + s * STEP * dUr)
        c = ex.certify(*sr.qa(p), p["x0"], sr.oracle_plan(p, p["x0"], k2), k2["x_ref"], k2["u_ref"])
        return np.sum(c["u_0"] ** 2, axis=0) + LD(0.1) * c["V"], sr.face_of(c["U"], p["lb"], p["ub"]), k2
    (Lp, fp, kp), (Lm, fm, km), (L0, f0, _) = at(1), at(-1), at(0)
    hX = (np.asarray(kp["x_ref"], dtype=LD) - np.asarray(km["x_ref"], dtype=LD)) / 2
    hU = (np.asarray(kp["u_ref"], dtype=LD) - np.asarray(km["u_ref"], dtype=LD)) / 2
    same = np.all(fp == f0, axis=(0, 1)) & np.all(fm == f0, axis=(0, 1))
    return (Lp - Lm) / 2, hX, hU, same, L0, f0


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    c = sr.case((4, 2, 10), refs=True, bsz=BSZ)
    p, kw = c["p"], c["kw"]
    dXr, dUr = direction(kw)
    fd = central_difference(p, kw, dXr, dUr)
    same = fd[3]
    assert np.mean(~same) <= 0.01, np.flatnonzero(~same)
    tmp = tmp_path_factory.mktemp("torch_layer_refs")
    inp, outp = str(tmp / "in.npz"), str(tmp / "out.npz")
    np.savez(inp, mask=same.astype(np.float64), **p, **kw)
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "torch_layer_refs_job.py")
    r = subprocess.run([sys.executable, script, inp, outp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return c, fd, dict(np.load(outp))


def test_reference_gradient_equals_the_reduced_cost_grad(job):
    c, _, out = job
    assert np.all(out["np_status"] == 0) and int(out["np_skipped"]) == 0
    assert np.array_equal(out["u_0"], out["np_u_0"])
    assert bool(out["xref_grad_is_cpu"]) and out["xref_grad"].shape == (4, 10) and out["uref_grad"].shape == (2, 10)
    assert np.any(out["xref_grad"] != 0.0) and np.any(out["uref_grad"] != 0.0)
    for k in ("xref", "uref"):
        assert np.array_equal(out[k + "_grad"], out["np_g_" + k]), k
        assert np.array_equal(out["both_" + k + "_grad"], out["np_g_" + k]), k
    assert np.array_equal(out["both_A_grad"], out["np_g_A"]) and np.array_equal(out["both_B_grad"], out["np_g_B"])
    e = float(np.max(np.abs(out["x_grad"] - out["np_x_grad"]))) / max(float(np.max(np.abs(out["np_x_grad"]))), 1.0)
    print(f"x.grad against K_0'w + gam dV_dx of the NumPy interface: {e:.2e}")
    assert e <= 1e-12
    assert tuple(out["only_xref_grad_shape"]) == (4, 10)


def test_reference_gradient_equals_a_long_double_central_difference(job):
    c, (dL, hX, hU, same, L0, f0), out = job
    p = c["p"]
    assert np.array_equal(sr.face_bits(out["np_U_plan"], p["lb"], p["ub"])[..., same], f0[..., same])    # the GPU plan is on the oracle's face
    lin = np.sum(np.asarray(out["xref_grad"], dtype=LD) * hX) + np.sum(np.asarray(out["uref_grad"], dtype=LD) * hU)
    want = np.sum(dL[same])
    # the bar: GPU_BAR max(|g_b|_max, 1) on every entry of every instance's gradient, through the inner product; the summation
    # over the batch, Bsz eps sum |g_b| per entry, through the inner product as well; the difference's own rounding
    per = np.concatenate([out["per_g_xref"], out["per_g_uref"]], axis=0)[..., same]
    h = np.abs(np.concatenate([hX, hU], axis=0)).astype(np.float64)
    kernel = GPU_BAR * float(np.sum(np.maximum(np.max(np.abs(per), axis=(0, 1)), 1.0))) * float(np.sum(h))
    summation = BSZ * np.finfo(np.float64).eps * float(np.sum(np.sum(np.abs(per), axis=-1) * h))
    rounding = float(np.finfo(LD).eps * np.sum(np.abs(L0[same])))
    err = float(abs(lin - want))
    print(f"<x_ref.grad, dXr> + <u_ref.grad, dUr> against the central difference: {err / STEP:.2e} of {float(abs(want)) / STEP:.2e} on "
          f"{int(same.sum())} of {BSZ} instances; bar {(kernel + summation + rounding) / STEP:.2e} (kernel {kernel / STEP:.2e}, "
          f"summation {summation / STEP:.2e}, rounding {rounding / STEP:.2e})")
    assert err <= kernel + summation + rounding


def test_backward_after_an_intervening_set_reference_raises(job):
    _, _, out = job
    assert bool(out["raised"]) and "set_reference" in str(out["raised_message"])
