"""GPU (-m gpu): lq_mpc_amd.torch_layer.MPCLayer.rollout differentiated with respect to x0, the model and the plant, on (4,2,10) x 64
with T = 6 (the problems of tests/sens_ref.py, the plant of tests/rgrad_ref.py).  The GPU part runs in
tests/torch_layer_rollout_job.py, a process of its own in which torch opens the GPU first, started under `timeout -k 10`; here its
records are checked.

  loss = sum gJT J_T + sum gX X + sum gU U for the seeded cotangents of rgrad_ref.cotangents
  x0.grad, A.grad, B.grad = g_x0, g_A, g_B of rgrad_ref.reference (long double) on the tape the NumPy interface leaves for the same
    data, A_true.grad, B_true.grad (a plant shared by the batch) = the sums of g_A_true, g_B_true over the batch: at rgrad_ref.GPU_BAR
    relative to max(|ref|_max, 1), on the instances whose faces read bit for bit are the certified ones (at least 99 %);
  the layer's X, U, J_T are bit for bit those of the NumPy interface; the layer's own model with a per-instance plant gives the same
    x0.grad and per-instance plant gradients;
  <grads, direction> for one seeded random direction in (x0, A, B, A_true, B_true) = the central difference, step STEP = 1e-5, of the
    per-instance loss of the NumPy loop, at 1e-6 relative to max(|fd|_max, 1) (the bar and step of tests/test_gpu_torch_layer_plan.py:
    the loss is not quadratic in the data, the remainder is of order STEP ** 2), on the instances whose tape keeps its faces at all
    three points; those must be at least 80 % of the batch;
  forward and backward behind a busy stream leave an event recorded in front of them pending: nothing waited for the host."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rgrad_ref as rg
import sens_ref as sr

pytestmark = pytest.mark.gpu

BSZ = 64
T = 6
STEP = 1e-5
SEED = 6
SHAPE = (4, 2, 10)


def scale(g):
    return max(float(np.max(np.abs(g))), 1.0)


def direction(c):
    rng = np.random.default_rng(SEED)
    p = c["p"]
    return {k: rng.standard_normal(a.shape) for k, a in (("A", p["A"]), ("B", p["B"]), ("x0", p["x0"]), ("At", c["At"]), ("Bt", c["Bt"]))}


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    c = rg.case(SHAPE, T, bsz=BSZ)
    p = c["p"]
    tmp = tmp_path_factory.mktemp("torch_layer_rollout")
    inp, outp = str(tmp / "in.npz"), str(tmp / "out.npz")
    gJT, gX, gU = rg.cotangents(SHAPE[0], SHAPE[1], T, BSZ, SEED)
    np.savez(inp, T=T, STEP=STEP, At=c["At"], Bt=c["Bt"], gJT=gJT, gX=gX, gU=gU, **{"d_" + k: v for k, v in direction(c).items()}, **p)
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "torch_layer_rollout_job.py")
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, script, inp, outp], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return c, (gJT, gX, gU), dict(np.load(outp))


def test_gradients_equal_the_long_double_reference(job):
    c, cot, out = job
    p = c["p"]
    assert np.all(out["np_status_tape"] == 0)
    for k in ("X", "U", "J_T"):
        assert np.array_equal(out[k], out["np_" + k]), k
    assert np.array_equal(out["own_X"], out["X"])
    ref = rg.reference(p, c["kw"], c["At"], c["Bt"], out["np_X"], out["np_U_tape"], *cot)
    same = np.all(rg.tape_faces(out["np_U_tape"], p["lb"], p["ub"]) == ref["free"], axis=(0, 1, 2))
    assert np.mean(~same) <= 0.01
    per = (("x_grad", "g_x0", 0), ("A_grad", "g_A", (0, 1)), ("B_grad", "g_B", (0, 1)), ("own_x_grad", "g_x0", 0),
           ("own_At_grad", "g_A_true", (0, 1)), ("own_Bt_grad", "g_B_true", (0, 1)), ("x_grad_again", "g_x0", 0), ("A_grad_again", "g_A", (0, 1)))
    for k, r, ax in per:
        e = sr.rel_err(out[k], ref[r], ax)[same].max()
        print(f"{k} against the long-double reference: {e:.2e}")
        assert e < rg.GPU_BAR, k
    assert same.all()                                               # (the sums below take every instance)
    for k, r in (("At_grad", "g_A_true"), ("Bt_grad", "g_B_true")):
        want = ref[r].sum(axis=-1)
        e = float(np.max(np.abs(out[k] - want))) / scale(want)
        print(f"{k} (shared plant) against the summed reference: {e:.2e}")
        assert e < rg.GPU_BAR, k


def test_gradient_along_a_direction_equals_a_central_difference(job):
    c, _, out = job
    p = c["p"]
    d = direction(c)
    faces = [rg.tape_faces(out[k], p["lb"], p["ub"]) for k in ("np_U_tape", "tape_plus", "tape_minus")]
    same = np.all(faces[0] == faces[1], axis=(0, 1, 2)) & np.all(faces[0] == faces[2], axis=(0, 1, 2))
    lin = (np.sum(out["x_grad"] * d["x0"], axis=0) + np.sum(out["A_grad"] * d["A"], axis=(0, 1)) + np.sum(out["B_grad"] * d["B"], axis=(0, 1)))
    # the plant is shared: its per-instance share of the directional derivative comes from the per-instance gradients of the second run
    lin = lin + np.sum(out["own_At_grad"] * d["At"][:, :, None], axis=(0, 1)) + np.sum(out["own_Bt_grad"] * d["Bt"][:, :, None], axis=(0, 1))
    err = float(np.max(np.abs(lin - out["fd"])[same])) / scale(out["fd"][same])
    print(f"<grads, direction> against the central difference: {err:.2e} on {int(same.sum())} of {BSZ} instances ({same.mean():.0%})")
    assert same.sum() >= 0.8 * BSZ
    assert err <= 1e-6


def test_forward_and_backward_do_not_wait_for_the_host(job):
    _, _, out = job
    print(f"rollout forward and backward: {float(out['host_seconds']) * 1e3:.2f} ms on the host, event pending: {bool(out['event_pending'])}")
    assert bool(out["event_pending"])
