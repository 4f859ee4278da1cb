"""CPU: what tests/test_gpu_postpass_hard.py rests on -- the two references of tests/postpass_hard.py and the constants of its bars,
on every (family, shape) of qp_hard.CASE_LIST.  Nothing here runs a kernel; DESIGN.md section 4.6b.

  1. The referee's plan.  U* rounded to fp64 has, bit for bit (cgrad_ref.side_bits), the face the referee certified, on every instance
     of every case but one, and grad_ref.reference / cgrad_ref.reference / sens_ref.reference, which certify the rounded plan again,
     report that face with ok true.  The one: ("near_degenerate", (8, 4, 30)).  There entry (3, 1) of the plan is free at the
     referee's optimum and 3.3e-17 h from its bound on instance 0 -- it rounds onto the bound, 12 of 13 bit-for-bit faces are the
     certified one -- and 9.6e-16 h and 9.9e-16 h from it on instances 1 and 2, where it stays off the bound in fp64 but exact.certify,
     which takes an entry within 1e-15 of a bound as active, puts it there: the dense references stand on the face the kernel reads
     on 11 of 13 instances.  Reference (A) cannot serve that case (A_UNSERVED; the numbers are asserted below); it stays in (B), and
     its K_plan, which needs the face alone, and dV_dx, which needs no face, stay in the licence.
  2. The licence of reference (B): the long-double restatements against the dense references at the rounded referee's plan, every
     output, every instance (at A_UNSERVED: K_plan and dV_dx on every instance, the gradients on the 11 instances above), within
     2^-64 2^10 cond_2(H_b) relative to max(|ref|, 1).  Measured worst, as a share of that bar: 0.48 (g_lb, near_degenerate
     (4,2,10), where cond_2(H) is 5 .. 26); on the three hard families 0.011 (dV_dx, unstable (2,1,30)).
  3. The constants.  The fp64 restatement that factors as the kernels do against (A) at the referee's plan and against (B) at the
     fp64 oracle's plan; ratio = err_b / (eps cond_2(H_b)) over the instances with cond_2(H_b) >= qp_hard.HARD_COND; c = 16 x the
     worst, rounded up to a power of two.  postpass_hard.C must be exactly that.  Measured worst ratios (A | B):
         K_plan 0.211 | 0.211  redundant (12,2,10)         dV_dx  0.0027 unstable (2,1,30) | 0.0010 integrator (2,1,30)
         g_A    0.117 | 0.117  integrator (7,3,11)         g_B    0.158 | 0.158  redundant (3,3,4)
         g_x0   0.155 | 0.155  redundant (3,3,4)           g_Q    0.0100 | 0.0100 redundant (3,3,4)
         g_R    0.161 | 0.161  redundant (3,3,4)           g_P    0.00081 unstable (4,4,4) | 0.00053 redundant (4,4,4)
         g_lb   0.101 | 0.101  redundant (3,3,4)           g_ub   0.026 | 0.026  redundant (4,4,4)
         g_xref 0.164 | 0.164  redundant (4,2,20)          g_uref 0.086 | 0.086  redundant (3,3,4)
     (B)'s ratios are (A)'s because the restatement's own rounding is what both see: the long-double restatement is within 2^-54 cond
     of the dense formula, and the plans differ by the oracle's error, which (B) takes out by construction.
  4. Pivots.  Every Cholesky pivot of the fp64 restatement is positive and every output finite, on both plans.  The smallest pivot
     relative to its diagonal entry: 1.9e-6 (redundant (4,2,10); the redundant cases 1.9e-6 .. 2.7e-5, integrator (7,3,11) 1.7e-4,
     every other case above 6e-3) -- far from the eps at which a pivot could turn.
  5. The floor.  On near_degenerate the errors of the fp64 restatement stay under every floor (at worst 1.0e-15 at (4,2,10), 4.6e-14
     at (8,4,30)), and the bar IS the
     floor wherever c eps cond_2(H_b) <= floor: every output at (4,2,10) and (7,3,11) (cond_2(H) <= 26), the outputs of sens at
     (8,4,30).  At (8,4,30) cond_2(H) reaches 3.64e4 on the instances of one model, and with c = 4 the scaled term, 3.2e-11, passes the
     floors of model-grad (5.8e-12) and cost-grad (1.7e-12): there the bar is the scaled one on the instances the test counts, and
     the floor on the others."""
import numpy as np
import pytest

import cgrad_ref as cg
import postpass_hard as ph
import qp_hard as qh
import sens_ref as sr
from test_cgrad_cpu import GPU_BAR as CGRAD_GPU_BAR

LD = np.longdouble
IDS = [f"{f}-{'x'.join(map(str, s))}" for f, s in qh.CASE_LIST]
GRADS = [k for name in ("grad", "cgrad") for k, _ in ph.KERNELS[name]]

_MEASURED = {}


def measure(family, shape):
    """Everything the tests below read of one case, computed once: the faces, the long-double restatement against the dense
    references, the fp64 restatement against (A) and (B), the pivots."""
    key = (family, shape)
    if key in _MEASURED:
        return _MEASURED[key]
    p = qh.problem(family, shape)
    w, gam = ph.cotangents(p)
    rp, d, op = ph.referee_plan(p), ph.dense(p), ph.oracle_plan(p)
    m = dict(p=p, cond=qh.cond_H(p), rp=rp, dense=d)
    m["bit_is_certified"] = np.all(rp["side"] == rp["certified"], axis=(0, 1))
    m["bit_is_dense"] = np.all(rp["side"] == d["side"], axis=(0, 1))
    m["licence"] = ph.errors(ph.restate(p, rp["U"], rp["X"], rp["side"], w, gam, dtype=LD), d)
    m["stats_A"], m["stats_B"] = {}, {}
    m["f64_A"] = ph.restate(p, rp["U"], rp["X"], rp["side"], w, gam, chol=True, stats=m["stats_A"])
    m["f64_B"] = ph.restate(p, op["U"], op["X"], op["side"], w, gam, chol=True, stats=m["stats_B"])
    m["err_A"] = ph.errors(m["f64_A"], d)
    m["err_B"] = ph.errors(m["f64_B"], ph.restate(p, op["U"], op["X"], op["side"], w, gam, dtype=LD))
    _MEASURED[key] = m
    return m


def served(m, k):
    """the instances of a case on which reference (A) serves output k: all of them, but at A_UNSERVED, for a gradient, those where
    the dense references stand on the face the rounded plan has bit for bit"""
    if (m["p"]["family"], m["p"]["shape"]) in ph.A_UNSERVED and k in GRADS:
        return m["bit_is_dense"]
    return np.ones(m["cond"].size, dtype=bool)


def test_floors_are_the_easy_problems_bars():
    assert ph.FLOOR["cgrad"] == CGRAD_GPU_BAR and ph.FLOOR["sens"] == 1e-10 and ph.FLOOR["grad"] == 5.8e-12
    assert ph.LICENCE == 2.0 ** -54
    assert list(ph.AXES) == ["K_plan", "dV_dx", "g_A", "g_B", "g_x0"] + [k for k, _ in cg.KEYS]


def test_kernel_like_cholesky_reads_the_lower_triangle_only():
    """chol_factor / chol_apply against numpy on a random SPD stack; the upper triangle may hold anything"""
    rng = np.random.default_rng(5)
    M = rng.standard_normal((7, 5, 5))
    Re = M @ M.transpose(0, 2, 1) + 0.1 * np.eye(5)
    G = rng.standard_normal((7, 5, 3))
    stats = {}
    L, Di = sr.chol_factor(Re, stats)
    Ln = np.linalg.cholesky(Re)
    assert np.allclose(L, np.tril(Ln, -1), rtol=1e-13, atol=0) and np.allclose(Di, 1 / np.einsum("bii->bi", Ln), rtol=1e-13, atol=0)
    assert np.allclose(sr.chol_apply(L, Di, G), np.linalg.solve(Re, G), rtol=1e-11, atol=0)
    assert stats["positive"] and 0 < stats["pivot"] <= 1
    junk = Re + np.triu(np.full((5, 5), np.nan), 1)
    L2, Di2 = sr.chol_factor(junk)
    assert np.array_equal(L, L2) and np.array_equal(Di, Di2)
    bad = {}
    sr.chol_factor(np.array([[[1.0, 2.0], [2.0, 1.0]]]), bad)
    assert not bad["positive"] and bad["pivot"] == -3.0
    # the three solvers of a stage agree; long double goes through oracle/exact.py and is the most accurate
    x_ld = sr.stage_solver(np.asarray(Re, dtype=LD), LD)(np.asarray(G, dtype=LD))
    for chol in (False, True):
        assert np.max(np.abs(sr.stage_solver(Re, np.float64, chol)(G) - x_ld)) < 1e-11


@pytest.mark.parametrize("family,shape", qh.CASE_LIST, ids=IDS)
def test_rounded_referee_plan_has_the_certified_face(family, shape):
    m = measure(family, shape)
    n = m["cond"].size
    a, b = int(m["bit_is_certified"].sum()), int(m["bit_is_dense"].sum())
    print(f"{family} {shape}: the rounded plan's face is the certified one on {a} of {n}, the dense references' on {b} of {n}; "
          f"entries on a bound {np.mean(m['rp']['side'] != 0):.2f}")
    assert m["dense"]["ok"].all() and m["dense"]["one_face"]
    # (the certificate of the fp64 oracle's face, which the referee started from: on the ladder either face is optimal)
    assert m["rp"]["ok"].all() or family == "near_degenerate"
    if (family, shape) in ph.A_UNSERVED:
        assert (a, b, n) == ph.A_UNSERVED[(family, shape)]
        assert np.flatnonzero(~m["bit_is_certified"]).tolist() == [0] and np.flatnonzero(~m["bit_is_dense"]).tolist() == [1, 2]
    else:
        assert a == n and b == n
    if (family, shape) in qh.OFF_CENTRE:
        # the bounds also come out as c +- h; side_bits reads either form
        assert not np.array_equal(m["p"]["lb"], -m["p"]["ub"]) and (m["rp"]["side"] != 0).any()
    # K_plan of the dense gain on the bit-for-bit face is sens_ref.reference's wherever the faces agree
    same = m["bit_is_dense"]
    assert np.array_equal(m["dense"]["K_plan"][..., same], m["dense"]["K_sens"][..., same])


def test_reference_A_is_unserved_at_exactly_one_case():
    assert list(ph.A_UNSERVED) == [("near_degenerate", (8, 4, 30))]
    assert ph.A_CASES == [c for c in qh.CASE_LIST if c not in ph.A_UNSERVED] and len(ph.A_CASES) == len(qh.CASE_LIST) - 1


@pytest.mark.parametrize("family,shape", qh.CASE_LIST, ids=IDS)
def test_long_double_restatements_against_the_dense_references(family, shape):
    """what licenses reference (B)"""
    m = measure(family, shape)
    share = {k: float(np.max((e / (ph.LICENCE * m["cond"]))[served(m, k)])) for k, e in m["licence"].items()}
    print(f"{family} {shape}: error / (2^-54 cond_2(H_b)), worst instance: " + " ".join(f"{k} {v:.2e}" for k, v in share.items()))
    assert set(share) == set(ph.AXES)
    assert max(share.values()) <= 1.0, share


@pytest.mark.parametrize("family,shape", qh.CASE_LIST, ids=IDS)
def test_pivots_are_positive_and_outputs_finite(family, shape):
    m = measure(family, shape)
    print(f"{family} {shape}: smallest Cholesky pivot / its diagonal entry: {m['stats_A']['pivot']:.2e} at the referee's plan, "
          f"{m['stats_B']['pivot']:.2e} at the oracle's")
    for which in "AB":
        assert m["stats_" + which]["positive"] and m["stats_" + which]["pivot"] > 0
        for k in ph.AXES:
            assert np.all(np.isfinite(m["f64_" + which][k])), (which, k)


def worst_ratios():
    """{reference: {output: (worst ratio, family, shape)}} over the instances with cond_2(H_b) >= HARD_COND of every case"""
    out = {"A": {}, "B": {}}
    for which, cases in (("A", ph.A_CASES), ("B", qh.CASE_LIST)):
        for family, shape in cases:
            m = measure(family, shape)
            hard = m["cond"] >= qh.HARD_COND
            if not hard.any():
                continue
            for k, e in m["err_" + which].items():
                r = float(np.max(e[hard] / (ph.EPS * m["cond"][hard])))
                if r > out[which].get(k, (0.0,))[0]:
                    out[which][k] = (r, family, shape)
    return out


def test_constants_are_16_times_the_worst_ratio_rounded_up_to_a_power_of_two():
    worst = worst_ratios()
    for which in "AB":
        for k, (r, family, shape) in worst[which].items():
            print(f"({which}) {k}: worst ratio {r:.3g} at {family} {shape}; c = {ph.derive(r)} (pinned {ph.C[which][k]})")
    for which in "AB":
        assert {k: ph.derive(v[0]) for k, v in worst[which].items()} == ph.C[which], which
    # every one of the three hard families is in the ratios whole
    for family, shape in qh.CASE_LIST:
        if family != "near_degenerate":
            assert qh.cond_H(qh.problem(family, shape)).min() >= qh.HARD_COND, (family, shape)


LADDER = [(f, s) for f, s in qh.CASE_LIST if f == "near_degenerate"]


@pytest.mark.parametrize("family,shape", LADDER, ids=["x".join(map(str, s)) for _, s in LADDER])
def test_floor_on_the_near_degenerate_ladder(family, shape):
    m = measure(family, shape)
    cond = m["cond"]
    assert 5.0 <= cond.min() and cond.max() <= 4e4
    for which in "AB":
        for k in ph.AXES:
            floor = ph.FLOOR[ph.KERNEL_OF[k]]
            e = m["err_" + which][k][served(m, k)] if which == "A" else m["err_" + which][k]
            assert e.max() < floor, (which, k, e.max())
            governs = ph.bar(which, k, cond) == floor
            assert np.array_equal(governs, ph.C[which][k] * ph.EPS * cond <= floor)
            if shape != (8, 4, 30) or ph.KERNEL_OF[k] == "sens":
                assert governs.all(), (which, k)
    worst = max(float(m["err_" + which][k][served(m, k)].max()) for which in "AB" for k in ph.AXES)
    print(f"near_degenerate {shape}: cond_2(H) {cond.min():.3g} .. {cond.max():.3g}; the fp64 restatement's worst error {worst:.2e}; "
          f"largest c eps cond {max(ph.C['B'].values()) * ph.EPS * cond.max():.2e}")
