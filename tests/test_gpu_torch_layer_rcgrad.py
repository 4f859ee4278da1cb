"""GPU (-m gpu): lq_mpc_amd.torch_layer.MPCLayer.rollout differentiated with respect to the data the batch shares -- Q, R, P, lb, ub,
x_ref, u_ref given with the call as CPU tensors -- on (4,2,10) x 64 with T = 6 (the problem of tests/rgrad_ref.py with references and
the off-centre box, so that every one of the seven matters).  The GPU part runs in tests/torch_layer_rcgrad_job.py, a process of its
own in which torch opens the GPU first, started under `timeout -k 10`; here its records are checked.

  loss = sum gJT J_T + sum gX X + sum gU U for the seeded cotangents of rgrad_ref.cotangents
  Q.grad, R.grad, P.grad, lb.grad, ub.grad, x_ref.grad, u_ref.grad are bit for bit the outputs of the reduced call of the NumPy
    interface on the tape the NumPy interface leaves for the same data (the layer was made with other weights: the call's count);
  <grads, direction> for one seeded direction in the seven (symmetric in Q, R, P: the solver takes them as symmetric) = the central
    difference, step STEP = 1e-5, of the layer's own forward, at 1e-6 relative to max(|fd|, 1) (the bar and step of
    tests/test_gpu_torch_layer_rollout.py: the loss is not quadratic in the data, the remainder is of order STEP ** 2), over the
    instances whose tape keeps its faces at all three points, which must be at least 90 % of the batch: the layer's gradients are
    sums over the batch, so the share of the instances left out, from the per-instance call, is taken off them; the same per instance;
  with none of the seven given the outputs and the five older gradients are bit for bit those of the NumPy interface's
    rollout_tape_batch and rollout_grad_batch, and bit for bit those of the call with all seven given as the layer's own data;
  forward under given data and backward into x0, A, B behind a busy stream leave an event recorded in front of them pending: nothing
    waited for the host.  (A gradient in the seven is host data and costs the one copy to the host, as the references of a step do.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

import rcgrad_ref as rc
import rgrad_ref as rg

pytestmark = pytest.mark.gpu

BSZ = 64
T = 6
STEP = 1e-5
SEED = 7
SHAPE = (4, 2, 10)
SEVEN = ("Q", "R", "P", "lb", "ub", "x_ref", "u_ref")
OUT_OF = dict(Q="g_Q", R="g_R", P="g_P", lb="g_lb", ub="g_ub", x_ref="g_xref", u_ref="g_uref")


def direction(data):
    rng = np.random.default_rng(SEED)
    d = {k: rng.standard_normal(data[k].shape) for k in SEVEN}
    for k in ("Q", "R", "P"):
        d[k] = 0.5 * (d[k] + d[k].T)
    return d


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    c = rg.case(SHAPE, T, bsz=BSZ, refs=True, off_centre=True)
    p = dict(c["p"])
    data = dict(p, x_ref=np.asarray(c["kw"]["x_ref"], dtype=np.float64), u_ref=np.asarray(c["kw"]["u_ref"], dtype=np.float64))
    tmp = tmp_path_factory.mktemp("torch_layer_rcgrad")
    inp, outp = str(tmp / "in.npz"), str(tmp / "out.npz")
    gJT, gX, gU = rg.cotangents(SHAPE[0], SHAPE[1], T, BSZ, SEED)
    d = direction(data)
    np.savez(inp, T=T, STEP=STEP, At=c["At"], Bt=c["Bt"], gJT=gJT, gX=gX, gU=gU, **{"d_" + k: v for k, v in d.items()}, **data)
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "torch_layer_rcgrad_job.py")
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, script, inp, outp], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return data, d, dict(np.load(outp))


def test_gradients_are_the_reduced_call_bit_for_bit(job):
    _, _, out = job
    assert np.all(out["np_status_tape"] == 0) and int(out["skipped"]) == 0
    for k in ("X", "U", "J_T"):
        assert np.array_equal(out[k], out["np_" + k]), k
    for k in SEVEN:
        assert out[k + "_grad"].shape == out["red_" + OUT_OF[k]].shape
        assert np.array_equal(out[k + "_grad"], out["red_" + OUT_OF[k]]), k
        assert np.any(out[k + "_grad"] != 0.0), k


def test_gradient_along_a_direction_equals_a_central_difference(job):
    data, d, out = job
    sides = [rc.tape_sides(out[k], data["lb"] + s * STEP * d["lb"], data["ub"] + s * STEP * d["ub"])
             for k, s in (("np_U_tape", 0.0), ("tape_plus", 1.0), ("tape_minus", -1.0))]
    same = np.all(sides[0] == sides[1], axis=(0, 1, 2)) & np.all(sides[0] == sides[2], axis=(0, 1, 2))
    per = sum(np.tensordot(d[k], out["per_" + OUT_OF[k]], axes=d[k].ndim) for k in SEVEN)           # (Bsz,)
    layer = sum(float(np.sum(d[k] * out[k + "_grad"])) for k in SEVEN)
    fd = out["fd"]
    e_inst = float(np.max(np.abs(per - fd)[same])) / max(float(np.max(np.abs(fd[same]))), 1.0)
    want, got = float(np.sum(fd[same])), layer - float(np.sum(per[~same]))
    e_sum = abs(got - want) / max(abs(want), 1.0)
    print(f"<grads, direction> against the central difference of the layer's forward: the layer's sums {e_sum:.2e} ({got:.6e} against "
          f"{want:.6e}), per instance {e_inst:.2e}, on {int(same.sum())} of {BSZ} instances ({same.mean():.0%})")
    assert same.sum() >= 0.9 * BSZ
    assert e_sum <= 1e-6
    assert e_inst <= 1e-6


def test_without_the_seven_nothing_changes(job):
    _, _, out = job
    for k in ("J_T", "X", "U") + tuple(f"grad{i}" for i in range(5)):
        assert np.array_equal(out["old_" + k], out["ref_" + k]), k
        assert np.array_equal(out["new_" + k], out["old_" + k]), k


def test_forward_and_backward_do_not_wait_for_the_host(job):
    _, _, out = job
    print(f"rollout forward and backward: {float(out['host_seconds']) * 1e3:.2f} ms on the host, event pending: {bool(out['event_pending'])}")
    assert bool(out["event_pending"])
    assert np.array_equal(out["busy_X"], out["X"])
