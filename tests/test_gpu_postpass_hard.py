"""GPU (-m gpu): the three post-pass kernels -- lqmpc_sens_kernel, lqmpc_grad_kernel, lqmpc_cost_grad_kernel -- on the hard models of
tests/qp_hard.py: unstable models with cond_2(H) up to 1e8, an integrator chain, cheap control with nearly collinear inputs
(cond_2(R_e) up to 3e6) and the near_degenerate ladder.  Each kernel runs its own masked Riccati sweep with a Cholesky factor of R_e
per stage; the other GPU modules hold them on spectral radius <= 1 and weights of condition 10 only.  DESIGN.md section 4.6b.

References and bars: tests/postpass_hard.py (module docstring) and tests/test_postpass_hard_cpu.py, which licenses reference (B) and
pins the constants; none comes from a GPU result.  bar_b = max(floor, c eps cond_2(H_b)) per instance and output, errors relative to
max(|ref|_max, 1) (sens_ref.rel_err).

  a. (A), model-grad and cost-grad at the referee's plan (U* and X* rounded to fp64, status 0) against the dense long-double
     references: every (family, shape) of qp_hard.CASE_LIST but postpass_hard.A_UNSERVED -- ("near_degenerate", (8, 4, 30)), where
     the dense references stand on the face the rounded plan has on 11 of 13 instances only (tests/test_postpass_hard_cpu.py) -- per
     instance mode, every instance, c[A].  Every output finite; where stage 0 is saturated and gam == 0 the outputs the other
     modules hold to exact zeros are exact zeros and g_lb + g_ub is w bit for bit.
  b. (B), all three behind solve_batch(want_sens): per shape the first path of test_gpu_qp_hard.PATHS, both workgroup paths at
     (8, 4, 30) and both paths of (12, 2, 10) (jit = 2 and the generic kernel); lqmpc_last_kernel asserted.  Every instance and
     output within bar_b with c[B] of the long-double restatement on the GPU's own U_plan, X_plan and bit-for-bit face; K_plan also
     within c[A] of the dense -H_FF^-1 Fx[F] on that face.  Except on near_degenerate, the face read bit for bit is the face
     Referee.certify reports, with ok true, on every instance; on near_degenerate a second call returns the same bits.
  c. The controller: step(want_sens) and step(want_plan) followed by model_grad and cost_grad on redundant and unstable (4, 2, 10),
     on unstable (8, 4, 30) with ctl_wg = 1, and after set_model on every third instance with the models of integrator (4, 2, 10):
     bit for bit the solve flavour on the same plan, and within the (B) bars.
  d. Reduced mode on redundant (4, 2, 10) and unstable (2, 1, 30): test_gpu_cgrad.check_reduced, skipped == 0, a second call the
     same bits.

Every figure is printed before it is asserted; the worst err / (eps cond_2(H_b)) and err / bar_b per output, case and path go to
profiles/postpass_hard.json (written by this module when LQMPC_POSTPASS_HARD_JSON names a file)."""
import json
import os

import numpy as np
import pytest

import cgrad_ref as cg
import postpass_hard as ph
import qp_hard as qh
from lq_mpc_amd import BatchController
from test_gpu_cgrad import check_reduced
from test_gpu_qp_hard import DEFAULTS, PATHS

pytestmark = pytest.mark.gpu

LD = np.longdouble
ZERO_WHEN_SATURATED = ("g_A", "g_B", "g_x0", "g_Q", "g_R", "g_P", "g_xref", "g_uref")


@pytest.fixture
def opts(solver):
    """Option changes that every test undoes."""
    def set_(**kw):
        solver.set_options(**kw)
    yield set_
    solver.set_options(**DEFAULTS)


# ---------------- measurements ----------------
MEASURED = {}
PROFILE_HEAD = {
    "what": "the post-pass kernels on the hard models of tests/qp_hard.py, measured by tests/test_gpu_postpass_hard.py (written by that "
            "module when LQMPC_POSTPASS_HARD_JSON names a file); key: reference / path / shape / family / output",
    "fields": "ratio = max_b err_b / (eps cond_2(H_b)); err = max_b err_b; over_bar = max_b err_b / bar_b (a bar is met when <= 1); "
              "c = the constant of the bar max(floor, c eps cond_2(H_b))",
    "references": "A: the dense long-double formulas at the referee's plan rounded to fp64; B: the long-double restatement of the "
                  "kernel's algebra on the plan and face the kernel read; A-face: K_plan against the dense gain on the face the kernel read",
    "bars": "a priori (tests/postpass_hard.py; constants pinned by tests/test_postpass_hard_cpu.py)",
}


@pytest.fixture(scope="module", autouse=True)
def _dump_measurements():
    yield
    path = os.environ.get("LQMPC_POSTPASS_HARD_JSON")
    if path and MEASURED:
        with open(path, "w") as f:
            json.dump(dict(PROFILE_HEAD, measured=MEASURED), f, indent=1, sort_keys=True)


def hold(p, cond, which, got, ref, keys, tag, label=None):
    """The outputs `keys` of one call against a reference under the bars of `which`: the list of misses.  Every figure is printed,
    with the condition number of the instance it belongs to, and recorded."""
    misses, line = [], []
    errs = ph.errors(got, ref, keys)
    for k in keys:
        e, b = errs[k], ph.bar(which, k, cond)
        if not np.all(np.isfinite(got[k])):
            misses.append(f"{k}: not finite on instances {np.flatnonzero(~np.isfinite(got[k]).reshape(-1, e.size).all(axis=0)).tolist()}")
        w = int(np.argmax(e / b))
        name = "/".join((label or which, tag, "x".join(map(str, p["shape"])), p["family"], k))
        m = MEASURED.setdefault(name, dict(ratio=0.0, err=0.0, over_bar=0.0, c=ph.C[which][k]))
        m["ratio"] = max(m["ratio"], float(np.max(e / (ph.EPS * cond))))
        m["err"], m["over_bar"] = max(m["err"], float(e.max())), max(m["over_bar"], float(np.max(e / b)))
        line.append(f"{k} {e[w]:.2e} / {b[w]:.2e} (cond {cond[w]:.1e}, ratio {e[w] / (ph.EPS * cond[w]):.3g})")
        if np.any(e > b):
            misses.append(f"{k}: {int(np.sum(e > b))} instances over their bar, worst {e[w]:.3e} > {b[w]:.3e} at instance {w}, cond {cond[w]:.2e}")
    print(f"({label or which}) {tag} {p['family']} {p['shape']}: " + "; ".join(line))
    return misses


def names(kernel):
    return [k for k, _ in ph.KERNELS[kernel]]


def saturated_zeros(out, side, w, gam, tag):
    """where stage 0 is saturated and gam == 0: exact zeros, and g_lb + g_ub == w bit for bit (as tests/test_gpu_grad.py and
    tests/test_gpu_cgrad.py assert them on easy problems)"""
    zero = (side[:, 0] != 0).all(axis=0) & (gam == 0.0)
    print(f"{tag}: stage 0 saturated and gam == 0 on {int(zero.sum())} of {zero.size} instances")
    misses = [f"{k}: not exactly zero where stage 0 is saturated and gam == 0" for k in ZERO_WHEN_SATURATED
              if k in out and not np.all(out[k][..., zero] == 0.0)]
    if "g_lb" in out:
        if not np.array_equal((out["g_lb"] + out["g_ub"])[:, zero], w[:, zero]):
            misses.append("g_lb + g_ub is not w where stage 0 is saturated and gam == 0")
        if not np.all((out["g_lb"][:, zero] == 0.0) | (out["g_ub"][:, zero] == 0.0)):
            misses.append("g_lb and g_ub both non-zero on a saturated input")
    return misses


def gradients(solver, p, plan, w, gam, **more):
    """model_grad_batch and cost_grad_batch of one plan (U, X, status), the ten outputs in one dict"""
    out = dict(solver.model_grad_batch(*qh.qa(p), *plan, w, gam, **p["kw"]))
    out.update(solver.cost_grad_batch(*qh.qa(p), *plan, w, gam, **p["kw"], **more))
    return out


def case_id(f, s):
    return f"{f}-{'x'.join(map(str, s))}"


# ---------------- a. reference (A): the dense formulas at the referee's plan ----------------
@pytest.mark.parametrize("family,shape", ph.A_CASES, ids=[case_id(f, s) for f, s in ph.A_CASES])
def test_gradients_at_the_referees_plan_against_the_dense_reference(solver, family, shape):
    p = qh.problem(family, shape)
    cond, rp, ref = qh.cond_H(p), ph.referee_plan(p), ph.dense(p)
    w, gam = ph.cotangents(p)
    # what tests/test_postpass_hard_cpu.py asserts of every case here: the rounded plan has the certified face, bit for bit
    assert np.array_equal(rp["side"], ref["side"]) and np.array_equal(rp["side"], rp["certified"]) and ref["ok"].all()
    status = np.zeros(cond.size, dtype=np.int32)
    out = gradients(solver, p, (rp["U"], rp["X"], status), w, gam)
    misses = hold(p, cond, "A", out, ref, names("grad") + names("cgrad"), "referee's plan")
    misses += saturated_zeros(out, rp["side"], w, gam, f"{family} {shape}")
    assert not misses, "\n".join(misses)


# ---------------- b. reference (B): behind real solves ----------------
def paths_of(shape):
    return PATHS[shape] if shape in ((8, 4, 30), (12, 2, 10)) else PATHS[shape][:1]


BEHIND = [(f, s, path) for s, (fams, _) in qh.CASES.items() for path in paths_of(s) for f in fams]


def against_restatement(p, cond, g, out, w, gam, tag):
    """(B): sens outputs of g and the gradients `out` of g's plan against the long-double restatement on that plan and the face read
    off it bit for bit; K_plan also against the dense gain on that face.  Returns (misses, side)."""
    misses = []
    if not np.all(g["status"] == 0):
        misses.append(f"status {g['status'][g['status'] != 0]} on instances {np.flatnonzero(g['status']).tolist()}")
    side = cg.side_bits(g["U_plan"], p["lb"], p["ub"])
    kernels = [k for k in ("sens", "grad", "cgrad") if all(n in {**g, **out} for n in names(k))]
    ref = ph.restate(p, g["U_plan"], g["X_plan"], side, w, gam, dtype=LD, kernels=kernels)
    got = {**{k: g[k] for k in names("sens") if k in g}, **out}
    misses += hold(p, cond, "B", got, ref, [n for k in kernels for n in names(k)], tag)
    if "sens" in kernels:
        misses += hold(p, cond, "A", got, dict(K_plan=ph.dense_gain(p, side == 0)), ["K_plan"], tag, label="A-face")
        if not np.all(np.moveaxis(g["K_plan"], 2, 0)[:, side != 0] == 0.0):
            misses.append("a row of K_plan on a bound is not exactly zero")
    return misses, side


@pytest.mark.parametrize("family,shape,path", BEHIND, ids=[f"{case_id(f, s)}-{path[0].replace(' ', '_')}" for f, s, path in BEHIND])
def test_post_passes_behind_the_solve_against_the_long_double_restatement(solver, opts, family, shape, path):
    name, o, kernel = path
    p = qh.problem(family, shape)
    cond = qh.cond_H(p)
    w, gam = ph.cotangents(p)
    opts(**o)

    def call():
        g = solver.solve_batch(*qh.qa(p), p["x0"], want_sens=True, **p["kw"])
        assert kernel(solver.last_kernel()), (name, solver.last_kernel())
        return g, gradients(solver, p, (g["U_plan"], g["X_plan"], g["status"]), w, gam)
    g, out = call()
    misses, side = against_restatement(p, cond, g, out, w, gam, name)
    misses += saturated_zeros(out, side, w, gam, f"{name} {family} {shape}")
    if family != "near_degenerate":
        cert = qh.referee(p).certify(p["x0"], g["U_plan"])
        same = np.all(cg.side_of(cert["U"], p["lb"], p["ub"]) == side, axis=(0, 1))
        print(f"{name} {family} {shape}: the face read bit for bit is the certified one on {int(same.sum())} of {same.size}, ok on {int(cert['ok'].sum())}")
        if not (same.all() and cert["ok"].all()):
            misses.append(f"the face read off the plan is not the certified one on instances {np.flatnonzero(~same | ~cert['ok']).tolist()}")
    else:
        g2, out2 = call()
        for k in ("U_plan", "X_plan", "K_plan", "K_0", "dV_dx", "status"):
            if not np.array_equal(g[k], g2[k]):
                misses.append(f"{k} of a second call differs")
        misses += [f"{k} of a second call differs" for k in out if not np.array_equal(out[k], out2[k])]
    assert not misses, "\n".join(misses)


# ---------------- c. the controller flavours ----------------
def controller_check(solver, ctl, p, tag):
    cond = qh.cond_H(p)
    x = p["x0"]
    w, gam = ph.cotangents(p)
    gs = ctl.step(x, want_sens=True)
    gp = ctl.step(x, want_plan=True)
    plan = (gp["U_plan"], gp["X_plan"], gp["status"])
    out = dict(ctl.model_grad(*plan, w, gam))
    out.update(ctl.cost_grad(*plan, w, gam))
    want = gradients(solver, p, plan, w, gam)
    misses = [f"{k}: the controller flavour is not the solve flavour bit for bit" for k in want if not np.array_equal(out[k], want[k])]
    misses += against_restatement(p, cond, gs, {}, w, gam, tag + ", sens step")[0]
    misses += against_restatement(p, cond, gp, out, w, gam, tag + ", plan step")[0]
    return misses


CONTROLLERS = [("redundant", (4, 2, 10), {}), ("unstable", (4, 2, 10), {}), ("unstable", (8, 4, 30), dict(ctl_wg=1))]


@pytest.mark.parametrize("family,shape,o", CONTROLLERS, ids=[case_id(f, s) for f, s, _ in CONTROLLERS])
def test_controller_flavours_on_hard_models(solver, opts, family, shape, o):
    p = qh.problem(family, shape)
    opts(**o)
    with BatchController(solver, *qh.qa(p), **p["kw"]) as ctl:
        opts(**DEFAULTS)
        assert ctl.kernel == "lqmpc_wg_ctl_step_kernel" if o else "ctl" in ctl.kernel, ctl.kernel
        misses = controller_check(solver, ctl, p, "controller")
    assert not misses, "\n".join(misses)


def test_controller_after_set_model_with_integrator_models(solver):
    """unstable (4, 2, 10) with every third instance's model replaced, in place, by that instance's of integrator (4, 2, 10)"""
    base, other = qh.problem("unstable", (4, 2, 10)), qh.problem("integrator", (4, 2, 10))
    idx = np.arange(0, base["x0"].shape[1], 3)
    A, B = base["A"].copy(), base["B"].copy()
    A[:, :, idx], B[:, :, idx] = other["A"][:, :, idx], other["B"][:, :, idx]
    p = dict(base, A=A, B=B, canonical=False)                    # (not cached by qp_hard: its condition numbers are computed here)
    with BatchController(solver, *qh.qa(base), **base["kw"]) as ctl:
        assert "ctl" in ctl.kernel, ctl.kernel
        ctl.set_model(np.ascontiguousarray(A[:, :, idx]), np.ascontiguousarray(B[:, :, idx]), idx)
        misses = controller_check(solver, ctl, p, "controller after set_model")
    assert not misses, "\n".join(misses)


# ---------------- d. reduced mode ----------------
REDUCED = [("redundant", (4, 2, 10)), ("unstable", (2, 1, 30))]


@pytest.mark.parametrize("family,shape", REDUCED, ids=[case_id(f, s) for f, s in REDUCED])
def test_reduced_mode_on_hard_models(solver, family, shape):
    p = qh.problem(family, shape)
    w, gam = ph.cotangents(p)
    g = solver.solve_batch(*qh.qa(p), p["x0"], want_plan=True, **p["kw"])
    assert np.all(g["status"] == 0)
    a = (*qh.qa(p), g["U_plan"], g["X_plan"], g["status"], w, gam)
    per = solver.cost_grad_batch(*a, **p["kw"])
    red, again = solver.cost_grad_batch(*a, **p["kw"], reduce=True), solver.cost_grad_batch(*a, **p["kw"], reduce=True)
    assert red["skipped"] == 0 and again["skipped"] == 0
    check_reduced(red, per, np.ones(gam.size, dtype=bool), f"{family} {shape}")
    for k, _ in cg.KEYS:
        assert np.array_equal(red[k], again[k]), k
