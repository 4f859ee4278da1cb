"""CPU: what tests/test_gpu_loopgrad_hard.py rests on -- the two references of tests/loopgrad_hard.py and the constants of its bars,
for the plan-grad, rollout-grad and rollout-cost-grad post-passes on every (family, shape) of qp_hard.CASE_LIST.  Nothing here runs a
kernel; DESIGN.md section 4.6c.  Every figure is printed before it is asserted.

  1. Faces.  The referee's tape (loopgrad_hard.referee_tape: the referee's own closed loop, states and plans rounded to fp64) has, bit
     for bit (cgrad_ref.side_bits), the face the referee certified on every slice of every instance of the 24 cases off shape
     (8, 4, 30), and rgrad_ref.reference / rcgrad_ref.reference, which certify every slice again, report that face with ok true.  The
     rounded referee's plan does likewise for pgrad_ref.reference on the 26 cases of postpass_hard.A_CASES.  No instance is left out.
     What (A) does not serve is in loopgrad_hard.A_UNSERVED, with the reasons.
  2. The licence of reference (B): the long-double restatements against the dense references at the referee's plan or tape, every
     output, every instance, within 2^-64 2^10 cond_2(H_b) relative to max(|ref|, 1).  Measured worst, as a share of that bar:
     pgrad 0.34 (g_B), rgrad 0.53 (g_B), rcgrad 0.048 (g_R), all at near_degenerate (4,2,10), where cond_2(H) is 5 .. 26; on the three
     hard families 0.0019, 0.19 and 0.0036 (g_A, g_A, g_lb at unstable (2,1,30)).
  3. The constants.  The fp64 restatement that factors as the kernels do against (A) at the referee's plan or tape and against (B) at
     the fp64 oracle's; ratio = err_b / (eps cond_2(H_b)) over the instances with cond_2(H_b) >= qp_hard.HARD_COND of every case the
     reference serves; c = 16 x the worst, rounded up to a power of two.  loopgrad_hard.C must be exactly that.  Measured worst ratios
     (A | B):
       pgrad   g_A      0.398 | 0.398  redundant (12,2,10)     g_B      0.397 | 0.397  redundant (12,2,10)
               g_x0     0.326 | 0.326  redundant (12,2,10)
       rgrad   g_A      0.606 unstable (2,1,30) | 0.332 unstable (2,1,30)
               g_B      0.180 redundant (4,2,20) | 0.353 unstable (8,4,30)
               g_x0     0.849 | 0.844  redundant (3,3,4)
               g_A_true 0.134 redundant (3,3,4) | 0.248 unstable (8,4,30)
               g_B_true 0.178 redundant (3,3,4) | 0.259 unstable (8,4,30)
       rcgrad  g_Q      0.0987 | 0.0986 redundant (4,4,4)      g_R      0.247 | 0.248  redundant (4,2,10)
               g_P      0.0197 | 0.0197 redundant (4,4,4)      g_lb     0.143 | 0.128  unstable (3,3,4)
               g_ub     0.0964 | 0.0929 redundant (4,4,4)      g_xref   0.263 redundant (12,2,10) | 4.63 unstable (8,4,30)
               g_uref   0.196 redundant (3,3,4) | 0.629 unstable (8,4,30)
     Where (B)'s ratio is the larger one the case is (8, 4, 30), which (A) does not serve for the closed loop.  g_xref at unstable
     (8,4,30), 4.63 and so c = 128, is the numpy restatement's own rounding (120 terms a stage, five steps); the kernel's is
     recorded by the GPU module.  The easy-model bars cannot stand here: against its own long-double restatement the fp64 one is off
     by 3.5e-10 (pgrad, g_x0 at redundant (4,4,4)), 5.1e-10 (rgrad, g_B at unstable (8,4,30)) and 6.7e-9 (rcgrad, g_xref at unstable
     (8,4,30)): 51, 51 and 2200 times the floors.
  4. Pivots.  Every Cholesky pivot of the fp64 restatements is positive and every output finite, on both plans and both tapes.  The
     smallest pivot relative to its diagonal entry: 1.9e-6 (redundant (4,2,10); the redundant cases 1.9e-6 .. 2.7e-5, integrator
     (7,3,11) 8.5e-6, every other case above 6e-3) -- far from the eps at which a pivot could turn.
  5. The floor.  On near_degenerate (4,2,10) and (7,3,11), cond_2(H) <= 26, the errors of the fp64 restatements stay under every floor
     (at worst 1.9e-15) and every bar is the floor.
  6. The mix of steps on the fp64 oracle's tapes of the hard families: stage 0 on bounds / a mixed face / all free, e.g. integrator
     (4,2,10) 0.65 / 0.35 / 0.00, unstable (4,2,10) 0.18 / 0.23 / 0.59, redundant (8,4,30) 0.00 / 0.88 / 0.12; each kind has a share of
     at least 0.10 in some case.
"""
import numpy as np
import pytest

import loopgrad_hard as lh
import postpass_hard as ph
import qp_hard as qh
import rcgrad_ref as rc
import rgrad_ref as rg

LD = np.longdouble
IDS = [f"{f}-{'x'.join(map(str, s))}" for f, s in qh.CASE_LIST]
LOOP = ("rgrad", "rcgrad")
# the cases reference (A) serves for at least one kernel
SERVED = [c for c in qh.CASE_LIST if any(c in lh.A_CASES[k] for k in lh.KERNELS)]
SERVED_IDS = [f"{f}-{'x'.join(map(str, s))}" for f, s in SERVED]

_MEASURED = {}


def measure(family, shape):
    """Everything the tests below read of one case, computed once: the faces, the long-double restatements against the dense references
    at the referee's plan and tape, the fp64 restatements against (A) there and against (B) at the fp64 oracle's, the pivots."""
    key = (family, shape)
    if key in _MEASURED:
        return _MEASURED[key]
    p = qh.problem(family, shape)
    m = dict(p=p, cond=qh.cond_H(p))
    inputs = {"A": dict(pgrad=ph.referee_plan(p), rgrad=lh.referee_tape(p), rcgrad=lh.referee_tape(p)),
              "B": dict(pgrad=ph.oracle_plan(p), rgrad=lh.oracle_tape(p), rcgrad=lh.oracle_tape(p))}
    m["inputs"] = inputs

    def restate(kernel, which, **kw):
        d = inputs[which][kernel]
        if kernel == "pgrad":
            return lh.restate_plan(p, d["U"], d["X"], d["side"], **kw)
        return lh.restate_loop(kernel, p, d, **kw)
    for kernel in lh.KERNELS:
        for which in "AB":
            st = m[f"stats_{which}_{kernel}"] = {}
            f64 = m[f"f64_{which}_{kernel}"] = restate(kernel, which, chol=True, stats=st)
            ld = restate(kernel, which, dtype=LD)
            if which == "B":
                m[f"err_B_{kernel}"] = lh.errors(kernel, f64, ld)
            elif (family, shape) in lh.A_CASES[kernel]:
                d = m[f"dense_{kernel}"] = lh.dense(kernel, p)
                m[f"err_A_{kernel}"] = lh.errors(kernel, f64, d)
                m[f"licence_{kernel}"] = lh.errors(kernel, ld, d)
    _MEASURED[key] = m
    return m


def test_floors_are_the_easy_problems_bars():
    # (pgrad: BAR of tests/test_gpu_pgrad.py, which needs the library to import)
    assert lh.FLOOR == dict(pgrad=7.0e-12, rgrad=rg.GPU_BAR, rcgrad=rc.GPU_BAR)
    assert rg.GPU_BAR == 100 * 1.0e-13 and rc.GPU_BAR == 100 * 3.0e-14
    assert lh.LICENCE == 2.0 ** -54 and lh.T == 5
    for which in "AB":
        assert {k: list(v) for k, v in lh.C[which].items()} == {k: [n for n, _ in keys] for k, keys in lh.KERNELS.items()}


def test_what_reference_A_leaves_out():
    wide = [c for c in qh.CASE_LIST if c[1] == (8, 4, 30)]
    assert len(wide) == 3
    assert list(lh.A_UNSERVED["rgrad"]) == wide and list(lh.A_UNSERVED["rcgrad"]) == wide
    assert lh.A_CASES["pgrad"] == ph.A_CASES and len(lh.A_CASES["rgrad"]) == len(lh.A_CASES["rcgrad"]) == len(qh.CASE_LIST) - 3 == 24
    assert all(reason for table in lh.A_UNSERVED.values() for reason in table.values())


@pytest.mark.parametrize("family,shape", SERVED, ids=SERVED_IDS)
def test_referee_plan_and_tape_have_the_certified_face(family, shape):
    """no instance may be left out: the cap is zero"""
    m = measure(family, shape)
    p, n = m["p"], m["cond"].size
    if (family, shape) in lh.A_CASES["pgrad"]:
        rp, d = m["inputs"]["A"]["pgrad"], m["dense_pgrad"]
        a, b = np.all(rp["side"] == rp["certified"], axis=(0, 1)), np.all((rp["side"] == 0) == d["free"], axis=(0, 1))
        print(f"{family} {shape}: the rounded plan's face is the referee's on {int(a.sum())} of {n}, pgrad_ref.reference's on {int(b.sum())} of {n}")
        assert a.all() and b.all() and d["ok"].all()
    if (family, shape) in lh.A_CASES["rgrad"]:
        rt = m["inputs"]["A"]["rgrad"]
        a = np.all(rt["side"] == rt["certified"], axis=(0, 1, 2))
        line = [f"the referee's on {int(a.sum())} of {n}"]
        assert a.all()
        assert rt["ok"].all() or family == "near_degenerate"         # (the certificate of the fp64 oracle's face: on the ladder either is optimal)
        for kernel in LOOP:
            d = m["dense_" + kernel]
            b = np.all((rt["side"] == 0) == d["free"], axis=(0, 1, 2))
            line.append(f"{kernel}_ref.reference's on {int(b.sum())} of {n}")
            assert b.all() and d["ok"].all(), kernel
        print(f"{family} {shape}: every slice of the referee's tape has, bit for bit, " + ", ".join(line) +
              f"; entries on a bound {np.mean(rt['side'] != 0):.2f}")
        assert np.array_equal(rt["X"][:, 0], p["x0"])


@pytest.mark.parametrize("family,shape", SERVED, ids=SERVED_IDS)
def test_long_double_restatements_against_the_dense_references(family, shape):
    """what licenses reference (B)"""
    m = measure(family, shape)
    served = [k for k in lh.KERNELS if (family, shape) in lh.A_CASES[k]]
    for kernel in served:
        share = {k: float(np.max(e / (lh.LICENCE * m["cond"]))) for k, e in m["licence_" + kernel].items()}
        print(f"{family} {shape} {kernel}: error / (2^-54 cond_2(H_b)), worst instance: " + " ".join(f"{k} {v:.2e}" for k, v in share.items()))
        assert set(share) == set(lh.AXES[kernel])
        assert max(share.values()) <= 1.0, (kernel, share)


@pytest.mark.parametrize("family,shape", qh.CASE_LIST, ids=IDS)
def test_pivots_are_positive_and_outputs_finite(family, shape):
    m = measure(family, shape)
    for kernel in lh.KERNELS:
        sa, sb = m[f"stats_A_{kernel}"], m[f"stats_B_{kernel}"]
        print(f"{family} {shape} {kernel}: smallest Cholesky pivot / its diagonal entry: {sa['pivot']:.2e} at the referee's, "
              f"{sb['pivot']:.2e} at the oracle's")
        for which, st in (("A", sa), ("B", sb)):
            assert st["positive"] and st["pivot"] > 0, (kernel, which)
            for k in lh.AXES[kernel]:
                assert np.all(np.isfinite(m[f"f64_{which}_{kernel}"][k])), (kernel, which, k)


def worst_ratios():
    """{reference: {kernel: {output: (worst ratio, family, shape)}}} over the instances with cond_2(H_b) >= HARD_COND of every case the
    reference serves"""
    out = {w: {k: {} for k in lh.KERNELS} for w in "AB"}
    for which in "AB":
        for kernel in lh.KERNELS:
            for family, shape in (lh.A_CASES[kernel] if which == "A" else qh.CASE_LIST):
                m = measure(family, shape)
                hard = m["cond"] >= qh.HARD_COND
                if not hard.any():
                    continue
                for k, e in m[f"err_{which}_{kernel}"].items():
                    r = float(np.max(e[hard] / (lh.EPS * m["cond"][hard])))
                    if r > out[which][kernel].get(k, (0.0,))[0]:
                        out[which][kernel][k] = (r, family, shape)
    return out


def test_constants_are_16_times_the_worst_ratio_rounded_up_to_a_power_of_two():
    worst = worst_ratios()
    for which in "AB":
        for kernel in lh.KERNELS:
            for k, (r, family, shape) in worst[which][kernel].items():
                print(f"({which}) {kernel} {k}: worst ratio {r:.3g} at {family} {shape}; c = {lh.derive(r)} (pinned {lh.C[which][kernel][k]})")
    for which in "AB":
        for kernel in lh.KERNELS:
            assert {k: lh.derive(v[0]) for k, v in worst[which][kernel].items()} == lh.C[which][kernel], (which, kernel)
    # the easy-model bars cannot stand here: the fp64 restatement itself, against its own long-double restatement on the same tape
    # or plan, is over each of them somewhere
    for kernel in lh.KERNELS:
        e = max(float(measure(f, s)[f"err_B_{kernel}"][k].max()) for f, s in qh.CASE_LIST for k in lh.AXES[kernel])
        print(f"{kernel}: the fp64 restatement's worst error {e:.2e}, {e / lh.FLOOR[kernel]:.0f} x the easy-model bar")
        assert e > lh.FLOOR[kernel], kernel


LADDER = [(f, s) for f, s in qh.CASE_LIST if f == "near_degenerate" and s != (8, 4, 30)]


@pytest.mark.parametrize("family,shape", LADDER, ids=["x".join(map(str, s)) for _, s in LADDER])
def test_floor_on_the_near_degenerate_ladder(family, shape):
    m = measure(family, shape)
    cond = m["cond"]
    assert 5.0 <= cond.min() and cond.max() <= 26.0
    for kernel in lh.KERNELS:
        for which in "AB":
            for k in lh.AXES[kernel]:
                e = m[f"err_{which}_{kernel}"][k]
                print(f"near_degenerate {shape} ({which}) {kernel} {k}: the fp64 restatement's worst error {e.max():.2e}, floor {lh.FLOOR[kernel]:.1e}")
                assert e.max() < lh.FLOOR[kernel], (kernel, which, k, e.max())
                assert np.all(lh.bar(which, kernel, k, cond) == lh.FLOOR[kernel]), (kernel, which, k)


def test_every_kind_of_step_is_on_the_hard_tapes():
    """stage 0 on bounds (a step rgrad may skip), a mixed face, all free (a sweep rgrad may reuse): each with a share >= 0.10 of the
    (t, b) pairs of the fp64 oracle's tape in at least one case of the three hard families"""
    best = [0.0, 0.0, 0.0]
    for family, shape in qh.CASE_LIST:
        if family == "near_degenerate":
            continue
        mix = rg.kinds(measure(family, shape)["inputs"]["B"]["rgrad"]["side"] == 0)
        print(f"{family} {shape}: stage 0 on bounds / mixed / all free {mix[0]:.2f} / {mix[1]:.2f} / {mix[2]:.2f}")
        best = [max(a, b) for a, b in zip(best, mix)]
        if (family, shape) == ("integrator", (4, 2, 10)):
            assert [round(v, 2) for v in mix] == [0.65, 0.35, 0.00]
        if (family, shape) == ("unstable", (4, 2, 10)):
            assert [round(v, 2) for v in mix] == [0.18, 0.23, 0.59]
    assert min(best) >= 0.10, best
