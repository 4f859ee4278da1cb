"""GPU (-m gpu): the QP kernels on models whose condensed Hessian H or stage matrix R_e = R + B'Sigma B is ill-conditioned, against
the long-double referee (oracle/exact.py through tests/qp_hard.py, itself held to 50 digits by tests/test_qp_hard_cpu.py).

Cases (tests/qp_hard.py: CASES): unstable models on the highest rung of the spectral-radius ladder that keeps cond_2(H) <= 1e8, an
integrator chain, cheap control with nearly collinear inputs (cond_2(R_e) 1e4 .. 3e6), and the near_degenerate ladder: x0 within
1e-15 .. 1e-9 of the scale at which the unconstrained minimiser touches the box.  Every kernel family serves at least two of them
(PATHS below; lqmpc_last_kernel is asserted).

Bars, per instance b and quantity, a priori: bar_b = max(floor, c eps cond_2(H_b)), eps = 2^-52.
  floor  what the project holds the quantity to on easy problems (tests/test_gpu_domain_edges.py): 1e-10 for u, U, X and J_T, 1e-11 for V_N
  c      16 x the worst ratio err / (eps cond_2(H_b)) of the fp64 oracle against the referee, rounded up to a power of two
         (tests/test_qp_hard_cpu.py measures and pins them; none comes from a GPU result):

             entry point               U, u_0, X    V_N / J_T
             solve_batch               16           32
             BatchController.step      16           32
             rollout_batch (T = 5)     16           4

  Five (path, shape, family) cases are held to c = 1e3 on U and u_0 instead (HELD_TO_A_PRIORI below, with the operation that carries
  the error and the ratios measured); every other case, and V_N and X_plan everywhere, to the table.
  U, u_0: |u - u*| / max(|u*|, h); V_N, J_T relative; X: max |X - X_ref| / max |X_ref| with the bar of U.
Asserted on every instance of every case and path: status 0; exact.certify on the GPU's plan reports ok (the kernel's face is the
optimal one, KKT in long double; not on near_degenerate, where either face is optimal); U_plan, u_0, V_N within bar_b of the certified
optimum and of the referee's own; U_plan inside the box; X_plan within bar_b max |X| of the model rolled in long double under
U_plan (as tests/test_gpu_plan.py holds it: against X* it would carry |Gamma| times the error of U, which no bar on U bounds); two paths of one shape within the
sum of their bars of each other.  iters and the number of instances over r16_maxit (a hand-back) are recorded, not asserted -- except
on the near_degenerate ladder, where the 16-lane-row paths must stay within r16_maxit and a second solve must give the same bits.

The worst ratios err / (eps cond_2(H_b)), per path, shape, family and quantity, are in profiles/qp_hard_models.json (written by this
module when LQMPC_QP_HARD_JSON names a file)."""
import json
import os

import numpy as np
import pytest

import qp_hard as qh
from lq_mpc_amd import BatchController, KERNEL_AUTO, KERNEL_GENERIC

pytestmark = pytest.mark.gpu

DEFAULTS = dict(kernel=KERNEL_AUTO, warm_start=-1, presolve=-1, r16_maxit=12, r16_build=-1, layout=-1, jit=-1, ctl_wg=0, order=-1)
R16_MAXIT = 12


@pytest.fixture
def opts(solver):
    """Option changes that every test undoes."""
    def set_(**kw):
        solver.set_options(**kw)
    yield set_
    solver.set_options(**DEFAULTS)


def rows(shape, jit=False, lpi=16):
    tag = "<%d,%d,%d>" % shape
    return lambda k: ("r%d" % lpi) in k and tag in k and ("jit" in k) == jit and "ctl" not in k


PACKED = lambda k: k == "lqmpc_spec_kernel<4,2,10,4>"
GENERIC = lambda k: k == "lqmpc_generic_kernel"
WG = lambda k: k == "lqmpc_wg_kernel"

# shape -> [(path, options, the kernel lqmpc_last_kernel must name)]
PATHS = {
    (4, 2, 10): [("r16 throughput build", dict(r16_build=0), rows((4, 2, 10))), ("r16 latency build", dict(r16_build=1), rows((4, 2, 10))),
                 ("packed", dict(layout=0), PACKED), ("packed interior point", dict(warm_start=0), PACKED),
                 ("generic forced", dict(kernel=KERNEL_GENERIC), GENERIC)],
    (2, 1, 30): [("r16 one input", {}, rows((2, 1, 30)))],                  # small_inverse<1>, the longest prebuilt horizon
    (4, 2, 20): [("r64", {}, rows((4, 2, 20), lpi=64))],
    (3, 3, 4): [("r16 jit three inputs", {}, rows((3, 3, 4), jit=True))],   # padded with the dummy input: the Schur-block inverse
    (4, 4, 4): [("r16 jit four inputs", {}, rows((4, 4, 4), jit=True))],
    (2, 4, 8): [("r16 jit nu > nx", {}, rows((2, 4, 8), jit=True))],        # B'Sigma B singular: R_e conditioned by R alone
    (7, 3, 11): [("r64 jit", {}, rows((7, 3, 11), jit=True, lpi=64))],
    (12, 2, 10): [("wide state", dict(jit=2), rows((12, 2, 10), jit=True)), ("generic", {}, GENERIC)],
    (8, 4, 30): [("workgroup", {}, WG), ("workgroup interior point", dict(warm_start=0), WG)],
    (9, 5, 7): [("workgroup", {}, WG)],                                      # stages straddle the 16-row blocks
    (16, 4, 8): [("generic", {}, GENERIC)],
    (4, 6, 5): [("generic", {}, GENERIC)],
}

# Cases held to the a-priori bar max(floor, 1e3 eps cond_2(H_b)) on U and u_0 (tests/test_host_units_cpu.py gives the dense helpers the
# same constant) instead of the oracle's; X_plan and V_N stay on the table's, and so does every other family on these paths.  The dual
# side of an active-set iteration of the 16-lane-row kernels (lqmpc_r16_body.h: "W_AA lam = r_A, v_F = v_unc,F - W_FA lam") takes the free
# rows as the difference of the unconstrained minimiser and a correction through the explicit inverse W = (2H)^-1, so the error of W
# (eps cond_2(H) |W|) enters times |v_unc| / h -- 1e2 .. 1e3 where control is cheap and x0 far out -- which no primal solve on the face
# pays.  The workgroup kernel's active-set solve is dual-side on the explicit W = P^-1 as well (lqmpc_wg.hip), at n = 120.
A_PRIORI_C = 1e3
HELD_TO_A_PRIORI = {          # (path, shape, family) -> worst ratio measured under the oracle's constant (|v_unc| / h of that instance)
    ("r16 throughput build", (4, 2, 10), "redundant"): "128 (850)", ("r16 latency build", (4, 2, 10), "redundant"): "128 (850)",
    ("controller", (4, 2, 10), "redundant"): "176, step 3", ("wide state", (12, 2, 10), "redundant"): "136 (140)",
    ("workgroup interior point", (8, 4, 30), "unstable"): "17.8 (7.4)",
}


def c_U(path, p, entry):
    return A_PRIORI_C if (path, p["shape"], p["family"]) in HELD_TO_A_PRIORI else qh.C[entry]["U"]


def inside_box(Up, lb, ub):
    """Every entry of a plan in [lb, ub]: exactly so for a symmetric box; off centre the row and workgroup kernels form a bound as
    centre +- half-width, two ulps of max(|lb|, |ub|) (tests/test_gpu_plan.py: inside_box)."""
    slack = np.where(lb == -ub, 0.0, 2.0 * np.spacing(np.maximum(np.abs(lb), np.abs(ub))))[:, None, None]
    return (Up >= lb[:, None, None] - slack) & (Up <= ub[:, None, None] + slack)


# ---------------- measurements ----------------
MEASURED = {}
PROFILE_HEAD = {
    "what": "worst err / (eps cond_2(H_b)) over the instances of a case, per path / shape / family / quantity, of tests/test_gpu_qp_hard.py "
            "(written by that module when LQMPC_QP_HARD_JSON names a file): the GPU against the long-double referee",
    "fields": "ratio = max err_b / (eps cond_2(H_b)); err = max err_b; c = the constant of the bar max(floor, c eps cond_2(H_b)); "
              "missed_by = max err_b / bar_b where a bar was missed (absent: none was); iters_max / over_r16_maxit: recorded only; "
              "answered_by_generic of instances (run-time compiled paths): instances whose iters > 0 and whose u, V_N and iters are bit for bit "
              "those of the same call under kernel = GENERIC, that is, redone by the generic kernel's list pass",
    "bars": "a priori (module docstring of tests/test_gpu_qp_hard.py, constants pinned by tests/test_qp_hard_cpu.py)",
}


def record(key, q, err, bar, cond, c):
    e = MEASURED.setdefault("/".join(key + (q,)), dict(ratio=0.0, err=0.0, c=c))
    e["ratio"] = max(e["ratio"], float(np.max(err / (qh.EPS * cond))))
    e["err"] = max(e["err"], float(np.max(err)))
    if np.any(err > bar):
        e["missed_by"] = max(e.get("missed_by", 0.0), float(np.max(err / bar)))


@pytest.fixture(scope="module", autouse=True)
def _dump_measurements():
    yield
    path = os.environ.get("LQMPC_QP_HARD_JSON")
    if path and MEASURED:
        with open(path, "w") as f:
            json.dump(dict(PROFILE_HEAD, measured=MEASURED), f, indent=1, sort_keys=True)


def key_of(path, p):
    return (path, "x".join(map(str, p["shape"])), p["family"])


def check_qp(p, x, g, ref, entry, key, face=True):
    """One call's plan at the states x against the referee there (ref = its own answer at x): the list of misses.  Every figure is
    printed, with the condition number of the instance it belongs to."""
    cond, R = qh.cond_H(p), qh.referee(p)
    misses = []
    bad = (g["status"] != 0) | ~np.isfinite(g["U_plan"]).all(axis=(0, 1))
    if bad.any():
        misses.append(f"status {g['status'][bad]} on instances {np.flatnonzero(bad)}")
    cand = np.where(bad[None, None, :], np.asarray(ref["U"], dtype=np.float64), g["U_plan"])      # (a NaN plan is no candidate)
    cert = R.certify(x, cand)
    if face and not cert["ok"][~bad].all():
        misses.append(f"the plan's face is not the optimal one on instances {np.flatnonzero(~cert['ok'] & ~bad)}")
    inside = inside_box(np.where(bad[None, None, :], 0.0, g["U_plan"]), p["lb"], p["ub"]).all(axis=(0, 1))
    if not inside.all():
        misses.append(f"U_plan leaves the box on instances {np.flatnonzero(~inside)}")
    cu = c_U(key[0], p, entry)
    bu, bx, bv = np.maximum(qh.FLOOR["U"], cu * qh.EPS * cond), qh.bar(entry, "U", cond), qh.bar(entry, "V", cond)
    errs = {
        "U": (np.maximum(qh.u_err(g["U_plan"], cert["U"], p["h"]), qh.u_err(g["U_plan"], ref["U"], p["h"])), bu, "U"),
        "u_0": (np.maximum(qh.u_err(g["u_0"], cert["u_0"], p["h"]), qh.u_err(g["u_0"], ref["u_0"], p["h"])), bu, "U"),
        "V_N": (np.maximum(qh.rel_err(g["V_N"], cert["V"]), qh.rel_err(g["V_N"], ref["V"])), bv, "V"),
        "X_plan": (qh.x_err(g["X_plan"], qh.model_roll(p, x, g["U_plan"])), bx, "X"),
    }
    line = []
    for q, (e, b, cq) in errs.items():
        e = np.where(np.isfinite(e), e, np.inf)
        record(key, q, e, b, cond, cu if cq == "U" else qh.C[entry]["U" if cq == "X" else cq])
        w = int(np.argmax(e / b))
        line.append(f"{q} {e[w]:.2e} / bar {b[w]:.2e} (cond {cond[w]:.1e}, ratio {e[w] / (qh.EPS * cond[w]):.3f})")
        if np.any(e > b):
            misses.append(f"{q}: {int(np.sum(e > b))} instances over their bar, worst {e[w]:.3e} > {b[w]:.3e} at instance {w}, cond {cond[w]:.2e}")
    m = MEASURED.setdefault("/".join(key + ("iters",)), dict(iters_max=0, over_r16_maxit=0))
    m["iters_max"] = max(m["iters_max"], int(g["iters"].max()))
    m["over_r16_maxit"] = max(m["over_r16_maxit"], int(np.sum(g["iters"] > R16_MAXIT)))
    print(f"{' / '.join(key)} [{entry}]: " + "; ".join(line) + f"; iters max {g['iters'].max()}, over r16_maxit {int(np.sum(g['iters'] > R16_MAXIT))}")
    return misses


def answered_by_generic(solver, opts, p, x, g, key):
    """Recorded, not asserted: how many instances of a run-time compiled path's call carry the generic kernel's answer -- a set-up whose
    inverse of R_e was refused (NaN) or an instance that reached r16_maxit is redone by the generic kernel's list pass, and
    lqmpc_last_kernel keeps the first pass's name.  Counted: iters > 0 and u_0, V_N, U_plan and iters bit for bit those of the same call
    under kernel = GENERIC (an instance the first pass finished without an iteration has iters = 0, the generic kernel never has)."""
    opts(**DEFAULTS)
    opts(kernel=KERNEL_GENERIC)
    gen = solver.solve_batch(*qh.qa(p), x, want_plan=True, **p["kw"])
    assert GENERIC(solver.last_kernel())
    opts(**DEFAULTS)
    same = (g["iters"] > 0) & (g["iters"] == gen["iters"]) & (g["V_N"] == gen["V_N"]) & np.all(g["U_plan"] == gen["U_plan"], axis=(0, 1))
    m = MEASURED.setdefault("/".join(key + ("iters",)), dict(iters_max=0, over_r16_maxit=0))
    m["answered_by_generic"] = max(m.get("answered_by_generic", 0), int(same.sum()))
    m["instances"] = int(same.size)
    print(f"{' / '.join(key)}: {int(same.sum())} of {same.size} instances carry the generic kernel's answer: instances {np.flatnonzero(same).tolist()}, "
          f"iters {g['iters'][same].tolist()}")
    return same


def run_paths(solver, opts, p, face=True):
    """solve_batch(want_plan) at x0 on every path of the shape: ({path: result}, misses)"""
    ref = qh.exact_solve(p)
    out, misses = {}, []
    for name, o, family in PATHS[p["shape"]]:
        opts(**DEFAULTS)
        opts(**o)
        g = solver.solve_batch(*qh.qa(p), p["x0"], want_plan=True, **p["kw"])
        assert family(solver.last_kernel()), (name, solver.last_kernel())
        out[name] = g
        misses += [f"{name}: {m}" for m in check_qp(p, p["x0"], g, ref, "solve", key_of(name, p), face)]
        if "jit" in name:
            answered_by_generic(solver, opts, p, p["x0"], g, key_of(name, p))
    # two paths of one shape: within the sum of their bars
    cond = qh.cond_H(p)
    names = list(out)
    for a in names[1:]:
        eu = qh.u_err(out[a]["U_plan"], out[names[0]]["U_plan"], p["h"])
        ev = qh.rel_err(out[a]["V_N"], out[names[0]]["V_N"])
        cs = [c_U(nm, p, "solve") for nm in (a, names[0])]
        both = sum(np.maximum(qh.FLOOR["U"], c_ * qh.EPS * cond) for c_ in cs)
        if np.any(eu > both) or np.any(ev > 2 * qh.bar("solve", "V", cond)):
            misses.append(f"{a} against {names[0]}: U {eu.max():.3e} V_N {ev.max():.3e}")
    return out, misses


# ---------------- a. one shot, every path ----------------
ONE_SHOT = [(f, s) for f, s in qh.CASE_LIST if f != "near_degenerate"]


@pytest.mark.parametrize("family,shape", ONE_SHOT, ids=[f"{f}-{'x'.join(map(str, s))}" for f, s in ONE_SHOT])
def test_one_shot_on_every_path(solver, opts, family, shape):
    p = qh.problem(family, shape)
    _, misses = run_paths(solver, opts, p)
    assert not misses, "\n".join(misses)


# ---------------- b. the near-degenerate ladder ----------------
LADDER = [(f, s) for f, s in qh.CASE_LIST if f == "near_degenerate"]


@pytest.mark.parametrize("family,shape", LADDER, ids=["x".join(map(str, s)) for _, s in LADDER])
def test_near_degenerate_ladder(solver, opts, family, shape):
    p = qh.problem(family, shape)
    out, misses = run_paths(solver, opts, p, face=False)
    for name, o, _ in PATHS[shape]:
        opts(**DEFAULTS)
        opts(**o)
        again = solver.solve_batch(*qh.qa(p), p["x0"], want_plan=True)
        k = solver.last_kernel()
        for q in ("U_plan", "X_plan", "u_0", "V_N", "status", "iters"):
            if not np.array_equal(out[name][q], again[q]):
                misses.append(f"{name}: {q} of a second solve differs")
        if ("r16" in k or "r64" in k) and np.any(out[name]["iters"] > R16_MAXIT):
            misses.append(f"{name}: iters {out[name]['iters'].max()} > r16_maxit")
    assert not misses, "\n".join(misses)


# ---------------- c. the prepared controller ----------------
@pytest.mark.parametrize("family,shape", qh.STEP_CASES, ids=[f"{f}-{'x'.join(map(str, s))}" for f, s in qh.STEP_CASES])
def test_controller_steps_on_exactly_known_states(solver, opts, family, shape):
    """five steps at the (rounded) states of the referee's own closed loop: each one QP at a known state, warm-started from the
    previous face, its set-up from the record factor kernel"""
    p = qh.problem(family, shape)
    steps = qh.exact_steps(p)
    if shape[1] * shape[2] > 48:
        opts(ctl_wg=1)
    misses = []
    with BatchController(solver, *qh.qa(p), **p["kw"]) as ctl:
        assert "ctl" in ctl.kernel, ctl.kernel
        for t, (x, ref) in enumerate(steps):
            g = ctl.step(x, want_plan=True)
            misses += [f"step {t}: {m}" for m in check_qp(p, x, g, ref, "step", key_of("controller", p))]
            if shape == (4, 4, 4):
                answered_by_generic(solver, opts, p, x, g, key_of("controller", p))
    assert not misses, "\n".join(misses)


# ---------------- d. closed loop ----------------
def check_rollout(p, g, key):
    ref, cond = qh.exact_roll(p), qh.cond_H(p)
    misses = []
    if not np.all(g["status"] == 0):
        misses.append(f"status {g['status'][g['status'] != 0]} on instances {np.flatnonzero(g['status'])}")
    bu, bj = qh.bar("rollout", "U", cond), qh.bar("rollout", "J", cond)
    errs = {"U": (qh.u_err(g["U"], ref["U"], p["h"]), bu, "U"), "X": (qh.x_err(g["X"], ref["X"]), bu, "U"),
            "J_T": (qh.rel_err(g["J_T"], ref["J_T"]), bj, "J")}
    line = []
    for q, (e, b, cq) in errs.items():
        e = np.where(np.isfinite(e), e, np.inf)
        record(key, q, e, b, cond, qh.C["rollout"][cq])
        w = int(np.argmax(e / b))
        line.append(f"{q} {e[w]:.2e} / bar {b[w]:.2e} (cond {cond[w]:.1e}, ratio {e[w] / (qh.EPS * cond[w]):.3f})")
        if np.any(e > b):
            misses.append(f"{q}: {int(np.sum(e > b))} instances over their bar, worst {e[w]:.3e} > {b[w]:.3e} at instance {w}, cond {cond[w]:.2e}")
    print(f"{' / '.join(key)} [rollout]: " + "; ".join(line) + f"; iters max {g['iters'].max()}")
    return misses


@pytest.mark.parametrize("family,shape", qh.ROLL_CASES, ids=[f"{f}-{'x'.join(map(str, s))}" for f, s in qh.ROLL_CASES])
def test_closed_loop_on_a_stable_plant(solver, opts, family, shape):
    """T = 5 with the hard model in the controller and the plant A (0.9 / rho(A)), B: U, X and J_T over all five steps"""
    p = qh.problem(family, shape)
    assert qh.exact_roll(p)["ok"].all()
    At, Bt = qh.plant(p)
    g = solver.rollout_batch(qh.T_ROLL, *qh.qa(p), p["x0"], At, Bt, want_traj=True, **p["kw"])
    assert PATHS[shape][0][2](solver.last_kernel()), solver.last_kernel()
    misses = check_rollout(p, g, key_of("rollout", p))
    assert not misses, "\n".join(misses)


def test_closed_loop_8192_instances_keep_their_bits(solver, opts):
    """8 192 instances of (4,2,10) unstable, instance b the model b mod 37: the difficulty order and the speculative free chunks.  Bit
    for bit the 37 models run on their own (the throughput build both times), which the referee holds to the bars."""
    p = qh.problem("unstable", (4, 2, 10))
    assert not p["kw"]
    At, Bt = qh.plant(p)
    idx = np.arange(8192) % p["x0"].shape[1]
    take = lambda a: np.ascontiguousarray(a[..., idx])
    opts(r16_build=0)
    small = solver.rollout_batch(qh.T_ROLL, *qh.qa(p), p["x0"], At, Bt, want_traj=True)
    assert "r16" in solver.last_kernel()
    misses = check_rollout(p, small, key_of("rollout throughput build", p))
    opts(**DEFAULTS)
    big = solver.rollout_batch(qh.T_ROLL, p["N"], take(p["A"]), take(p["B"]), p["Q"], p["R"], p["P"], p["lb"], p["ub"], take(p["x0"]),
                               take(At), take(Bt), want_traj=True)
    assert "r16" in solver.last_kernel()
    assert np.all(big["status"] == 0)
    for q in ("J_T", "U", "X", "status"):
        assert np.array_equal(big[q], small[q][..., idx]), q
    assert not misses, "\n".join(misses)
