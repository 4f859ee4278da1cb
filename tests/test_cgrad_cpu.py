"""CPU: the gradient of a loss on (u_0, V_N) with respect to the weights Q, R, P, the references x_ref, u_ref and the box lb, ub
(lqmpc_cost_grad_batch, lqmpc_controller_cost_grad and their _dev flavours; tests/cgrad_ref.py).

  (a) the formulas: cgrad_ref.reference (dense, long double) against Richardson-extrapolated central differences, in long double, of
      w'u_0 + gam V at the optimum of the plan's face held fixed (cgrad_ref.face_loss; an entry held at a bound moves with the
      bound), with respect to EVERY entry of Q, R, P, x_ref, u_ref, lb and ub; an off-diagonal weight entry is perturbed
      symmetrically and compared with g_ab + g_ba.  The eight cases of tests/test_grad_cpu.py: 8 instances of each spread over the
      batch; at (8,4,30) and (16,4,8), where one evaluation condenses 240 or 128 predicted states in long double, one instance,
      the one with the most entries on a bound among those whose stage 0 is not saturated.  Steps h = 1e-3, h / 2 and h / 4:
      D(h) = (f(+h) - f(-h)) / 2h, R(h) = (4 D(h/2) - D(h)) / 3.  Bar, per case and per parameter: 10 times the differences' own
      error estimate, both relative to max(|g|_max, 1) per instance.  That estimate has two parts: the remainder, max |R(h) -
      R(h/2)|, and the rounding, 5/3 eps_ld max |f| / (h / 4) -- one rounding of the loss divided by the smallest step and carried
      through R.  The second part is needed because the loss is quadratic in the references and the box: there the remainder is
      zero, both R are exact but for their rounding, and |R(h) - R(h/2)| alone is an accident of that rounding (0.0 at (2,1,1)).
      Measured worst over the cases: the formula against R(h/2) 6.1e-13 (g_P at (4,2,10) with references) where the differences'
      own error is 1.3e-12; for the references and the box 7e-14 at worst, against an own error of 1e-13 to 9e-13.
  (b) the restatement: cgrad_ref.adjoint (fp64 numpy, the algebra of lqmpc_cost_grad_kernel) against cgrad_ref.reference on the
      faces of the oracle's own plans, sens_ref.rel_err per instance and per output.  Bar 1e-12.  Measured worst over the eight
      cases: g_Q 7.9e-16, g_R 4.3e-16, g_P 1.7e-15, g_lb 1.68e-14 (at (16,4,8)), g_ub 1.2e-14, g_xref 3.6e-15, g_uref 2.0e-15.  The
      GPU tests' bar is 100 times the worst, rounded up to 1.7e-12 (GPU_BAR below, which tests/test_gpu_cgrad.py imports), the
      margin covering another summation order.
  (c) the four entry points are declared by include/lqmpc.h with their seven outputs, exported by the built library, and refuse
      NULL arguments before they touch a GPU."""
import os
import re

import numpy as np
import pytest

import cgrad_ref as cg
import grad_ref as gr
import sens_ref as sr
from lq_mpc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
CGRAD_SYMBOLS = ["lqmpc_cost_grad_batch", "lqmpc_cost_grad_batch_dev", "lqmpc_controller_cost_grad", "lqmpc_controller_cost_grad_dev"]
OUTPUTS = ["gQ", "gR", "gP", "glb", "gub", "gxref", "guref"]
BAR = 1e-12
WORST = 1.7e-14                    # (b), measured: the worst error of the restatement over the eight cases and the seven outputs
GPU_BAR = 100 * WORST              # 1.7e-12: the bar of tests/test_gpu_cgrad.py

# (shape, instances, refs, off-centre box): the cases of tests/test_grad_cpu.py
CASES = [((2, 1, 5), 203, False, False), ((4, 2, 10), 203, False, False), ((4, 2, 10), 203, True, False), ((4, 2, 10), 203, True, True),
         ((3, 3, 4), 203, False, False), ((2, 1, 1), 203, False, False), ((8, 4, 30), 24, False, False), ((16, 4, 8), 203, False, False)]


def test_cost_grad_symbols_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lqmpc.h")).read(), flags=re.S)
    L = _lib.lib()
    for name in CGRAD_SYMBOLS:
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        params = re.findall(r"(\w+)\s*(?:,|$)", m.group(1))
        dev = name.endswith("_dev")
        for o in OUTPUTS:
            assert ("d" + o if dev else o) in params, (name, o)
        assert "reduce" in params and ("dnskipped" if dev else "nskipped") in params, name
        assert name in _lib.EXPORTS and hasattr(L, name), name
    # dims, A, B, the shared block (7), the plan (3), the cotangents (2), reduce, the outputs (7), nskipped
    assert len(L.lqmpc_cost_grad_batch.argtypes) == 5 + 2 + 7 + 3 + 2 + 1 + 7 + 1
    assert len(L.lqmpc_controller_cost_grad.argtypes) == 1 + 3 + 2 + 1 + 7 + 1


def test_null_arguments_are_refused():
    """a NULL handle or controller, a NULL plan, both cotangents NULL, every output NULL: LQMPC_ERR_BAD_ARG, nothing is written"""
    L = _lib.lib()
    z = np.zeros(64)
    q = z.ctypes.data
    h = 1 << 20                                        # never dereferenced: the NULL checks come first
    outs = [q] * 7 + [None]
    none = [None] * 8
    for f in (L.lqmpc_cost_grad_batch, L.lqmpc_cost_grad_batch_dev):
        m = [2, 1, 5, 1, q, q, q, q, q, q, q, None, None]
        for red in (0, 1):
            assert f(None, *m, q, q, None, q, q, red, *outs) == -1
            assert b"NULL" in L.lqmpc_last_error()
            assert f(h, *m, None, q, None, q, q, red, *outs) == -1          # Uplan
            assert f(h, *m, q, None, None, q, q, red, *outs) == -1          # Xplan
            assert f(h, *m, q, q, None, None, None, red, *outs) == -1       # both cotangents
            assert f(h, *m, q, q, None, q, q, red, *none) == -1             # no output
            assert f(h, 2, 1, 5, 1, None, q, q, q, q, q, q, None, None, q, q, None, q, q, red, *outs) == -1   # A
    for f in (L.lqmpc_controller_cost_grad, L.lqmpc_controller_cost_grad_dev):
        assert f(None, q, q, None, q, q, 0, *outs) == -1
        assert b"NULL" in L.lqmpc_last_error()
        assert f(h, None, q, None, q, q, 0, *outs) == -1
        assert f(h, q, None, None, q, q, 0, *outs) == -1
        assert f(h, q, q, None, None, None, 0, *outs) == -1
        assert f(h, q, q, None, q, q, 1, *none) == -1
    assert np.all(z == 0.0)


def _richardson(f, h):
    """R(h), R(h/2) of the central differences of f(step)"""
    d = [(f(LD(s)) - f(-LD(s))) / (2 * LD(s)) for s in (h, h / 2, h / 4)]
    return (4 * d[1] - d[0]) / 3, (4 * d[2] - d[1]) / 3


@pytest.mark.parametrize("shape,bsz,refs,off", CASES, ids=str)
def test_formulas_against_richardson_central_differences(shape, bsz, refs, off):
    nx, nu, N = shape
    c = sr.case(shape, refs=refs, off_centre=off, bsz=bsz)
    idx = (np.arange(8) * (bsz // 8) + 3) % bsz
    if nx * N * nu >= 500:
        # one instance: of those whose stage 0 is not saturated, the one with the most entries on a bound
        on = sr.face_bits(c["U"], c["p"]["lb"], c["p"]["ub"]) == 0
        idx = np.array([int(np.argmax(np.where(on[:, 0].all(axis=0), -1, on.sum(axis=(0, 1)))))])
    p = dict(c["p"])
    for k in ("A", "B", "x0"):
        p[k] = np.ascontiguousarray(c["p"][k][..., idx])
    kw, x0, U = c["kw"], p["x0"], np.ascontiguousarray(c["U"][..., idx])
    w, gam = gr.cotangents(nu, idx.size, 7)
    ref = cg.reference(p, kw, x0, U, w, gam)
    assert ref["ok"].all()
    side = ref["side"]
    base = dict(Q=p["Q"], R=p["R"], P=p["P"], lb=p["lb"], ub=p["ub"],
                x_ref=kw.get("x_ref", np.zeros((nx, N))), u_ref=kw.get("u_ref", np.zeros((nu, N))))
    base = {k: np.asarray(v, dtype=LD) for k, v in base.items()}
    h = 1e-3
    # the rounding part of the differences' own error: one rounding of the loss, eps |f|, divided by the smallest step and carried
    # through D(h/4) = (f+ - f-) / (2 h/4) and R(h/2) = (4 D(h/4) - D(h/2)) / 3
    f0 = np.max(np.abs(cg.face_loss(p, kw, x0, side, w, gam)))
    floor = float(5 / 3 * np.finfo(LD).eps * f0 / (h / 4))
    worst = {}
    for name, key, sym in (("Q", "g_Q", True), ("R", "g_R", True), ("P", "g_P", True), ("x_ref", "g_xref", False),
                           ("u_ref", "g_uref", False), ("lb", "g_lb", False), ("ub", "g_ub", False)):
        M = base[name]
        want = np.array(ref[key])
        R1, R2 = np.zeros_like(want), np.zeros_like(want)
        for e in np.ndindex(M.shape):
            if sym and e[0] > e[1]:
                continue

            def f(s):
                M2 = M.copy()
                M2[e] += s
                if sym and e[0] != e[1]:
                    M2[e[::-1]] += s
                return cg.face_loss(p, kw, x0, side, w, gam, **{name: M2})
            R1[e], R2[e] = _richardson(f, h)
            if sym and e[0] != e[1]:
                # the symmetric perturbation sees g_ab + g_ba: both halves of the reference take the same comparison
                R1[e[::-1]], R2[e[::-1]] = R1[e], R2[e]
                want[e] = want[e[::-1]] = ref[key][e] + ref[key][e[::-1]]
        ax = tuple(range(want.ndim - 1))
        own, err = sr.rel_err(R1, R2, ax).max() + floor, sr.rel_err(want, R2, ax).max()
        worst[key] = (err, own)
        print(f"{shape} refs={refs} off={off} {key}: formula against R(h/2) {err:.2e}; the differences' own error {own:.2e}")
    for key, (err, own) in worst.items():
        assert err <= 10 * own, (key, err, own)


@pytest.mark.parametrize("shape,bsz,refs,off", CASES, ids=str)
def test_adjoint_restatement_against_the_dense_reference(shape, bsz, refs, off):
    c = sr.case(shape, refs=refs, off_centre=off, bsz=bsz)
    p, kw = c["p"], c["kw"]
    w, gam = gr.cotangents(shape[1], bsz, sum(shape))
    ref = cg.reference(p, kw, p["x0"], c["U"], w, gam)
    assert ref["ok"].all()
    U = np.asarray(ref["U"], dtype=np.float64)
    side = cg.side_bits(U, p["lb"], p["ub"])
    assert np.array_equal(side, ref["side"])
    X = sr.model_roll(p, p["x0"], U)
    ad = cg.adjoint(*sr.model(p), side, X, U, w, gam, kw.get("x_ref"), kw.get("u_ref"))
    e = {k: sr.rel_err(ad[k], ref[k], ax).max() for k, ax in cg.KEYS}
    print(f"{shape} x {bsz} refs={refs} off={off}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) +
          f"; entries on a bound {np.mean(side != 0):.2f}")
    assert max(e.values()) < BAR, e
    for k in ("g_Q", "g_P", "g_R"):
        assert np.array_equal(ad[k], ad[k].transpose(1, 0, 2)) or sr.rel_err(ad[k], ad[k].transpose(1, 0, 2), (0, 1)).max() < 1e-15, k
