"""GPU (-m gpu): the three newer post-pass kernels -- lqmpc_plan_grad_kernel, lqmpc_rollout_grad_kernel, lqmpc_rollout_cost_grad_kernel
-- and the tape forward (lqmpc_rollout_tape_batch with lqmpc_plant_step_kernel) on the hard models of tests/qp_hard.py: unstable models
with cond_2(H) up to 1e8, an integrator chain, cheap control with nearly collinear inputs (cond_2(R_e) up to 3e6) and the
near_degenerate ladder.  Each kernel restates the masked Riccati sweep with a Cholesky factor of R_e per stage; the other GPU modules
hold them on spectral radius <= 1 and weights of condition 10 only, under single constants.  DESIGN.md section 4.6c.

References and bars: tests/loopgrad_hard.py (module docstring) and tests/test_loopgrad_hard_cpu.py, which licenses reference (B) and
pins the constants; none comes from a GPU result.  bar_b = max(floor, c eps cond_2(H_b)) per instance and output, errors relative to
max(|ref|_max, 1) (sens_ref.rel_err).  The closed loop has T = qp_hard.T_ROLL = 5 steps on the plant qp_hard.plant(p).

  a. (A): plan_grad_batch at the referee's plan, rollout_grad_batch and rollout_cost_grad_batch at the referee's tape (status 0, no
     solve) against the dense long-double references, every instance of every case loopgrad_hard.A_CASES serves, c[A].  Every output
     finite; on instances where stage 0 is saturated at every step and gJT == 0 the model-side outputs of the two rollout kernels
     are exact zeros.
  b. (B): plan_grad_batch behind solve_batch(want_plan) -- per shape the first path of test_gpu_qp_hard.PATHS, both paths at (8, 4, 30)
     and (12, 2, 10); lqmpc_last_kernel asserted -- and the two rollout kernels behind rollout_tape_batch under the first path's
     options, on the per-instance plant, every status_tape 0: every instance and output within bar_b with c[B] of the long-double
     restatement on the GPU's own plan or tape and the faces read off it bit for bit.  On near_degenerate a second call returns the
     same bits.
  c. The tape forward on qp_hard.ROLL_CASES: U, X and J_T against the referee's closed loop under qp_hard.bar("rollout", ...), and
     U_tape[t][:, 0] == U[:, t] bit for bit.
  d. Wavefront neighbours: on unstable and integrator (4, 2, 10) every instance of the GPU's tape repeated four times in a row, so that
     every wavefront is uniform and both shortcuts of lqmpc_rgrad.hip fire (a step passed over, a sweep not run again): every copy has,
     bit for bit, the outputs of its instance in the unrepeated batch, of both rollout kernels.
  e. The wide end, unstable and redundant (16, 4, 8): with the cotangent at stage 0 alone plan_grad_batch gives g_A and g_B of
     model_grad_batch bit for bit (pgrad's second turn for column nx of G at nx = 16; rgrad's full register rows are in a. and b.).
  f. Reduced mode of rollout_cost_grad_batch on redundant (4, 2, 10): test_gpu_cgrad.check_reduced, skipped == 0, a second call the
     same bits.

Measured on one MI355X (DESIGN.md section 4.6c has the table): every bar met, the worst err / bar_b 0.096 (pgrad), 0.049 (rgrad), 0.144
(rcgrad), 0.58 (the tape forward).  g_xref at unstable (8, 4, 30), whose c[B] = 128 comes from the fp64 numpy restatement's own ratio
of 4.63: on the GPU's tape the restatement is again at 4.63 (recorded, not asserted), the kernel at 0.0038 -- its order of summation
does some three orders better there than numpy's.

Every figure is printed before it is asserted; the worst err / (eps cond_2(H_b)) and err / bar_b per reference, kernel, shape, family
and output go to profiles/loopgrad_hard.json (written by this module when LQMPC_LOOPGRAD_HARD_JSON names a file)."""
import json
import os

import numpy as np
import pytest

import cgrad_ref as cg
import loopgrad_hard as lh
import postpass_hard as ph
import qp_hard as qh
import rcgrad_ref as rc
from test_gpu_cgrad import check_reduced
from test_gpu_qp_hard import DEFAULTS, PATHS

pytestmark = pytest.mark.gpu

LD = np.longdouble
T = lh.T
ZERO_WHEN_SATURATED = dict(rgrad=("g_A", "g_B"), rcgrad=("g_Q", "g_R", "g_P", "g_xref", "g_uref"))


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
    "what": "the plan-grad, rollout-grad and rollout-cost-grad kernels on the hard models of tests/qp_hard.py, measured by "
            "tests/test_gpu_loopgrad_hard.py (written by that module when LQMPC_LOOPGRAD_HARD_JSON names a file); key: reference / kernel "
            "/ path / shape / family / output",
    "fields": "ratio = max_b err_b / (eps cond_2(H_b)); err = max_b err_b; over_bar = max_b err_b / bar_b (a bar is met when <= 1); "
              "c = the constant of the bar max(floor, c eps cond_2(H_b))",
    "references": "A: the dense long-double formulas at the referee's plan or tape rounded to fp64; B: the long-double restatement of "
                  "the kernel's algebra on the plan or tape and the faces the kernel read",
    "bars": "a priori (tests/loopgrad_hard.py; constants pinned by tests/test_loopgrad_hard_cpu.py)",
}


@pytest.fixture(scope="module", autouse=True)
def _dump_measurements():
    yield
    path = os.environ.get("LQMPC_LOOPGRAD_HARD_JSON")
    if path and MEASURED:
        with open(path, "w") as f:
            json.dump(dict(PROFILE_HEAD, measured=MEASURED), f, indent=1, sort_keys=True)


def hold(p, cond, which, kernel, got, ref, tag):
    """Every output of one call of `kernel` against a reference under the bars of `which`: the list of misses.  Every figure is printed,
    with the condition number of the instance it belongs to, and recorded."""
    misses, line = [], []
    errs = lh.errors(kernel, got, ref)
    for k, e in errs.items():
        b = lh.bar(which, kernel, k, cond)
        if not np.all(np.isfinite(got[k])):
            misses.append(f"{kernel} {k}: not finite on instances {np.flatnonzero(~np.isfinite(got[k]).reshape(-1, e.size).all(axis=0)).tolist()}")
        w = int(np.argmax(e / b))
        name = "/".join((which, kernel, tag, "x".join(map(str, p["shape"])), p["family"], k))
        m = MEASURED.setdefault(name, dict(ratio=0.0, err=0.0, over_bar=0.0, c=lh.C[which][kernel][k]))
        m["ratio"] = max(m["ratio"], float(np.max(e / (lh.EPS * cond))))
        m["err"], m["over_bar"] = max(m["err"], float(e.max())), max(m["over_bar"], float(np.max(e / b)))
        line.append(f"{k} {e[w]:.2e} / {b[w]:.2e} (cond {cond[w]:.1e}, ratio {e[w] / (lh.EPS * cond[w]):.3g})")
        if np.any(e > b):
            misses.append(f"{kernel} {k}: {int(np.sum(e > b))} instances over their bar, worst {e[w]:.3e} > {b[w]:.3e} at instance {w}, cond {cond[w]:.2e}")
    print(f"({which}) {kernel} {tag} {p['family']} {p['shape']}: " + "; ".join(line))
    return misses


def case_id(f, s):
    return f"{f}-{'x'.join(map(str, s))}"


def plan_grad(solver, p, U, X, status):
    return solver.plan_grad_batch(*qh.qa(p), U, X, status, *lh.plan_cotangents(p), **p["kw"])


def loop_grads(solver, p, X, U_tape, status_tape, **more):
    """{'rgrad': outputs of rollout_grad_batch, 'rcgrad': outputs of rollout_cost_grad_batch} on one tape"""
    a = (T, *qh.qa(p), *qh.plant(p), X, U_tape, status_tape, *lh.loop_cotangents(p))
    return dict(rgrad=solver.rollout_grad_batch(*a, **p["kw"]), rcgrad=solver.rollout_cost_grad_batch(*a, **p["kw"], **more))


def saturated_zeros(out, side, gJT, tag):
    """where stage 0 is saturated at every step and gJT == 0, no step's QP moves with the model or the weights: exact zeros (as
    tests/test_gpu_rcgrad.py: test_every_step_saturated asserts them on easy models)"""
    sat, _ = lh.step_kinds(side)
    zero = sat.all(axis=0) & (gJT == 0.0)
    print(f"{tag}: stage 0 saturated at every step and gJT == 0 on {int(zero.sum())} of {zero.size} instances")
    return [f"{kernel} {k}: not exactly zero where every step is saturated and gJT == 0" for kernel, keys in ZERO_WHEN_SATURATED.items()
            for k in keys if not np.all(out[kernel][k][..., zero] == 0.0)]


# ---------------- a. reference (A): the dense formulas at the referee's plan and tape ----------------
A_PLAN, A_LOOP = lh.A_CASES["pgrad"], lh.A_CASES["rgrad"]


@pytest.mark.parametrize("family,shape", A_PLAN, ids=[case_id(f, s) for f, s in A_PLAN])
def test_plan_grad_at_the_referees_plan_against_the_dense_reference(solver, family, shape):
    p = qh.problem(family, shape)
    cond, rp, ref = qh.cond_H(p), ph.referee_plan(p), lh.dense("pgrad", p)
    # what tests/test_loopgrad_hard_cpu.py asserts of every case here: the rounded plan has the certified face, bit for bit
    assert np.array_equal(rp["side"] == 0, ref["free"]) and np.array_equal(rp["side"], rp["certified"]) and ref["ok"].all()
    out = plan_grad(solver, p, rp["U"], rp["X"], np.zeros(cond.size, dtype=np.int32))
    misses = hold(p, cond, "A", "pgrad", out, ref, "referee's plan")
    assert not misses, "\n".join(misses)


@pytest.mark.parametrize("family,shape", A_LOOP, ids=[case_id(f, s) for f, s in A_LOOP])
def test_rollout_grads_at_the_referees_tape_against_the_dense_references(solver, family, shape):
    assert lh.A_CASES["rcgrad"] == A_LOOP
    p = qh.problem(family, shape)
    cond, rt = qh.cond_H(p), lh.referee_tape(p)
    out = loop_grads(solver, p, rt["X"], rt["U_tape"], np.zeros((T, cond.size), dtype=np.int32))
    misses = []
    for kernel in ("rgrad", "rcgrad"):
        ref = lh.dense(kernel, p)
        # what tests/test_loopgrad_hard_cpu.py asserts of every case here: every slice has the certified face, bit for bit
        assert np.array_equal(rt["side"] == 0, ref["free"]) and np.array_equal(rt["side"], rt["certified"]) and ref["ok"].all()
        misses += hold(p, cond, "A", kernel, out[kernel], ref, "referee's tape")
    misses += saturated_zeros(out, rt["side"], lh.loop_cotangents(p)[0], f"{family} {shape}")
    assert not misses, "\n".join(misses)


# ---------------- b. reference (B): behind real solves and rollouts ----------------
def paths_of(shape):
    return PATHS[shape] if shape in ((8, 4, 30), (12, 2, 10)) else PATHS[shape][:1]


BEHIND = [(f, s, path) for s, (fams, _) in qh.CASES.items() for path in paths_of(s) for f in fams]


@pytest.mark.parametrize("family,shape,path", BEHIND, ids=[f"{case_id(f, s)}-{path[0].replace(' ', '_')}" for f, s, path in BEHIND])
def test_plan_grad_behind_the_solve_against_the_long_double_restatement(solver, opts, family, shape, path):
    name, o, kernel = path
    p = qh.problem(family, shape)
    cond = qh.cond_H(p)
    opts(**o)

    def call():
        g = solver.solve_batch(*qh.qa(p), p["x0"], want_plan=True, **p["kw"])
        assert kernel(solver.last_kernel()), (name, solver.last_kernel())
        return g, plan_grad(solver, p, g["U_plan"], g["X_plan"], g["status"])
    g, out = call()
    misses = []
    if not np.all(g["status"] == 0):
        misses.append(f"status {g['status'][g['status'] != 0]} on instances {np.flatnonzero(g['status']).tolist()}")
    side = cg.side_bits(g["U_plan"], p["lb"], p["ub"])
    ref = lh.restate_plan(p, g["U_plan"], g["X_plan"], side, dtype=LD)
    misses += hold(p, cond, "B", "pgrad", out, ref, name)
    if family == "near_degenerate":
        g2, out2 = call()
        misses += [f"{k} of a second call differs" for k in ("U_plan", "X_plan", "status") if not np.array_equal(g[k], g2[k])]
        misses += [f"{k} of a second call differs" for k in out if not np.array_equal(out[k], out2[k])]
    assert not misses, "\n".join(misses)


_TAPES = {}


def gpu_tape(solver, opts, p):
    """rollout_tape_batch of a problem under the first path of its shape, on the per-instance plant: computed once and never changed"""
    key = (p["family"], p["shape"])
    if key not in _TAPES:
        opts(**PATHS[p["shape"]][0][1])
        g = solver.rollout_tape_batch(T, *qh.qa(p), p["x0"], *qh.plant(p), **p["kw"])
        assert PATHS[p["shape"]][0][2](solver.last_kernel()), solver.last_kernel()
        opts(**DEFAULTS)
        for a in g.values():
            a.setflags(write=False)
        _TAPES[key] = g
    return _TAPES[key]


@pytest.mark.parametrize("family,shape", qh.CASE_LIST, ids=[case_id(f, s) for f, s in qh.CASE_LIST])
def test_rollout_grads_behind_the_tape_against_the_long_double_restatement(solver, opts, family, shape):
    p = qh.problem(family, shape)
    cond = qh.cond_H(p)
    g = gpu_tape(solver, opts, p)
    misses = []
    if not (np.all(g["status_tape"] == 0) and np.all(g["status"] == 0)):
        misses.append(f"status_tape not 0 on instances {np.flatnonzero(g['status_tape'].max(axis=0)).tolist()}")
    out = loop_grads(solver, p, g["X"], g["U_tape"], g["status_tape"])
    tape = lh.tape_of(g["X"], g["U_tape"], p)
    sat, allfree = lh.step_kinds(tape["side"])
    print(f"{family} {shape}: stage 0 on bounds / mixed / all free {sat.mean():.2f} / {(~sat & ~allfree).mean():.2f} / {allfree.mean():.2f}")
    for kernel in ("rgrad", "rcgrad"):
        ref = lh.restate_loop(kernel, p, tape, dtype=LD)
        misses += hold(p, cond, "B", kernel, out[kernel], ref, PATHS[shape][0][0])
        if (family, shape) == ("unstable", (8, 4, 30)):
            # recorded, not asserted: the fp64 numpy restatement on the same tape, whose g_xref sets c = 128 here -- does the kernel's
            # summation order do better or worse?
            hold(p, cond, "B", kernel, lh.restate_loop(kernel, p, tape), ref, "fp64 numpy restatement on the GPU's tape")
    misses += saturated_zeros(out, tape["side"], lh.loop_cotangents(p)[0], f"{family} {shape}")
    if family == "near_degenerate":
        opts(**PATHS[shape][0][1])
        g2 = solver.rollout_tape_batch(T, *qh.qa(p), p["x0"], *qh.plant(p), **p["kw"])
        opts(**DEFAULTS)
        out2 = loop_grads(solver, p, g2["X"], g2["U_tape"], g2["status_tape"])
        misses += [f"{k} of a second tape differs" for k in g if not np.array_equal(g[k], g2[k])]
        misses += [f"{kernel} {k} of a second call differs" for kernel in out for k in out[kernel] if not np.array_equal(out[kernel][k], out2[kernel][k])]
    assert not misses, "\n".join(misses)


# ---------------- c. the tape forward ----------------
@pytest.mark.parametrize("family,shape", qh.ROLL_CASES, ids=[case_id(f, s) for f, s in qh.ROLL_CASES])
def test_tape_forward_against_the_referees_closed_loop(solver, opts, family, shape):
    p = qh.problem(family, shape)
    ref, cond = qh.exact_roll(p), qh.cond_H(p)
    assert ref["ok"].all()
    g = gpu_tape(solver, opts, p)
    bu, bj = qh.bar("rollout", "U", cond), qh.bar("rollout", "J", cond)
    errs = {"U": (qh.u_err(g["U"], ref["U"], p["h"]), bu), "X": (qh.x_err(g["X"], ref["X"]), bu), "J_T": (qh.rel_err(g["J_T"], ref["J_T"]), bj)}
    misses, line = [], []
    if not (np.all(g["status_tape"] == 0) and np.all(g["status"] == 0)):
        misses.append(f"status_tape not 0 on instances {np.flatnonzero(g['status_tape'].max(axis=0)).tolist()}")
    for q, (e, b) in errs.items():
        e = np.where(np.isfinite(e), e, np.inf)
        w = int(np.argmax(e / b))
        m = MEASURED.setdefault("/".join(("referee", "tape forward", PATHS[shape][0][0], "x".join(map(str, shape)), family, q)),
                                dict(ratio=0.0, err=0.0, over_bar=0.0, c=qh.C["rollout"]["J" if q == "J_T" else "U"]))
        m["ratio"], m["err"] = max(m["ratio"], float(np.max(e / (qh.EPS * cond)))), max(m["err"], float(e.max()))
        m["over_bar"] = max(m["over_bar"], float(np.max(e / b)))
        line.append(f"{q} {e[w]:.2e} / bar {b[w]:.2e} (cond {cond[w]:.1e}, ratio {e[w] / (qh.EPS * cond[w]):.3f})")
        if np.any(e > b):
            misses.append(f"{q}: {int(np.sum(e > b))} instances over their bar, worst {e[w]:.3e} > {b[w]:.3e} at instance {w}, cond {cond[w]:.2e}")
    print(f"tape forward {family} {shape}: " + "; ".join(line))
    if not np.array_equal(g["U"], np.ascontiguousarray(g["U_tape"][:, :, 0].transpose(1, 0, 2))):
        misses.append("U is not the first stage of every slice of U_tape, bit for bit")
    if not np.array_equal(g["X"][:, 0], p["x0"]):
        misses.append("X[:, 0] is not x0")
    assert not misses, "\n".join(misses)


# ---------------- d. wavefront neighbours ----------------
NEIGHBOURS = [("unstable", (4, 2, 10)), ("integrator", (4, 2, 10))]


def test_wavefront_neighbours_do_not_matter(solver, opts):
    """A wavefront of lqmpc_rollout_grad_kernel holds four instances.  With every instance repeated four times in a row each wavefront
    is uniform: a step whose stage 0 is saturated is passed over, a wholly free step after a wholly free one reuses the sweep.  The
    kernel's header promises exact zeros for the one and the same bits for the other, so every copy must carry the bits its instance
    has in the unrepeated batch, where its neighbours are other instances and the shortcuts mostly do not fire."""
    misses, skipped, reused_from, free_pairs = [], 0, 0, 0
    for family, shape in NEIGHBOURS:
        p = qh.problem(family, shape)
        g = gpu_tape(solver, opts, p)
        assert np.all(g["status_tape"] == 0)
        out = loop_grads(solver, p, g["X"], g["U_tape"], g["status_tape"])
        rep = lambda a: np.ascontiguousarray(np.repeat(a, 4, axis=-1))
        At, Bt = qh.plant(p)
        a4 = (T, p["N"], rep(p["A"]), rep(p["B"]), p["Q"], p["R"], p["P"], p["lb"], p["ub"], rep(At), rep(Bt), rep(g["X"]), rep(g["U_tape"]),
              rep(g["status_tape"]), *[rep(c) for c in lh.loop_cotangents(p)])
        out4 = dict(rgrad=solver.rollout_grad_batch(*a4, **p["kw"]), rcgrad=solver.rollout_cost_grad_batch(*a4, **p["kw"]))
        sat, allfree = lh.step_kinds(rc.tape_sides(g["U_tape"], p["lb"], p["ub"]))
        n_sat, n_free, n_pairs = int(sat.sum()), int(allfree.sum()), int((allfree[1:] & allfree[:-1]).sum())
        print(f"{family} {shape}: of {sat.size} (wavefront, step) pairs of the repeated batch {n_sat} are uniformly saturated, {n_free} uniformly "
              f"free, {n_pairs} uniformly free after a uniformly free step")
        skipped, reused_from, free_pairs = skipped + n_sat, reused_from + n_free, free_pairs + n_pairs
        for kernel in out:
            for k in out[kernel]:
                for copy in range(4):
                    if not np.array_equal(out4[kernel][k][..., copy::4], out[kernel][k]):
                        bad = np.flatnonzero((out4[kernel][k][..., copy::4] != out[kernel][k]).reshape(-1, sat.shape[1]).any(axis=0))
                        misses.append(f"{family} {kernel} {k}: copy {copy} differs from the unrepeated batch on instances {bad.tolist()}")
    assert skipped > 0 and reused_from > 0 and free_pairs > 0, (skipped, reused_from, free_pairs)
    assert not misses, "\n".join(misses)


# ---------------- e. the wide end ----------------
WIDE = [("unstable", (16, 4, 8)), ("redundant", (16, 4, 8))]


@pytest.mark.parametrize("family,shape", WIDE, ids=[case_id(f, s) for f, s in WIDE])
def test_stage_0_cotangent_alone_gives_the_model_gradient_bit_for_bit(solver, family, shape):
    """nx = 16: every lane of a row owns a row of S, and column nx of G -- the right-hand side of kap_j -- has no lane left: it goes
    through the K_j solve on lane 0 in a second turn.  With g_Xplan and g_VN NULL and the cotangent at stage 0 alone the kernel computes
    what lqmpc_grad_kernel computes for gu0 = w_0."""
    p = qh.problem(family, shape)
    rp = ph.referee_plan(p)
    w = lh.plan_cotangents(p)[0]
    w0 = np.zeros_like(w)
    w0[:, 0] = w[:, 0]
    a = (*qh.qa(p), rp["U"], rp["X"], np.zeros(w.shape[-1], dtype=np.int32))
    mine = solver.plan_grad_batch(*a, w0, None, None, **p["kw"])
    theirs = solver.model_grad_batch(*a, np.ascontiguousarray(w[:, 0]), None, **p["kw"])
    e = {k: float(np.max(np.abs(mine[k] - theirs[k]))) for k in ("g_A", "g_B", "g_x0")}
    print(f"{family} {shape}: plan_grad_batch with the stage-0 cotangent alone against model_grad_batch, max |difference|: " +
          " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert np.any(theirs["g_A"] != 0.0) and np.all(np.isfinite(theirs["g_A"]))
    assert np.array_equal(mine["g_A"], theirs["g_A"]) and np.array_equal(mine["g_B"], theirs["g_B"]), e


# ---------------- f. reduced mode ----------------
def test_reduced_mode_on_a_hard_model(solver, opts):
    p = qh.problem("redundant", (4, 2, 10))
    g = gpu_tape(solver, opts, p)
    assert np.all(g["status_tape"] == 0)
    a = (T, *qh.qa(p), *qh.plant(p), g["X"], g["U_tape"], g["status_tape"], *lh.loop_cotangents(p))
    per = solver.rollout_cost_grad_batch(*a, **p["kw"])
    red, again = solver.rollout_cost_grad_batch(*a, **p["kw"], reduce=True), solver.rollout_cost_grad_batch(*a, **p["kw"], reduce=True)
    assert red["skipped"] == 0 and again["skipped"] == 0
    check_reduced(red, per, np.ones(p["x0"].shape[1], dtype=bool), "redundant (4, 2, 10)")
    for k, _ in rc.KEYS:
        assert np.array_equal(red[k], again[k]), k
