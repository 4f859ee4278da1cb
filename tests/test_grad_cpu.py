"""CPU: the gradient of a loss on (u_0, V_N) with respect to the model matrices A and B (lqmpc_model_grad_batch,
lqmpc_controller_model_grad and their _dev flavours; tests/grad_ref.py).

  * the four entry points are declared, exported and refuse bad arguments before they touch a GPU;
  * the formula: grad_ref.reference (dense, long double) against Richardson-extrapolated central differences, in long double, of
    w'u_0 + gam V at the optimum of the plan's face held fixed (grad_ref.face_loss), with respect to every entry of A and B, on 8
    instances of (4,2,10) with references and the off-centre box.  Steps h = 1e-3 and h / 2: D(h) = (f(+h) - f(-h)) / 2h,
    R(h) = (4 D(h/2) - D(h)) / 3, whose error is O(h^4).  Bar 1e-9 relative to max(|g|_max, 1) per instance; the differences' own
    error, |R(h) - R(h/2)|, is asserted below 1e-10 (measured 1.9e-12; R(h/2) against the formula 1.3e-13 for g_A, 9.5e-15 for g_B);
  * the restatement: grad_ref.adjoint (fp64 numpy, the algebra of lqmpc_grad_kernel) against grad_ref.reference on the faces of the
    oracle's own plans, sens_ref.rel_err per instance.  Bar 1e-12.  Measured worst over the eight cases: g_A 5.7e-14, g_B 2.6e-14,
    g_x0 7.1e-15 (the worst is (2,1,5), where |x0| up to 9 meets a spectral radius near 1).  The GPU tests' bar is 100 times the
    worst, rounded up to 5.8e-12, which is tighter than the sens tests' 1e-10, so nothing forces a looser one: tests/test_gpu_grad.py
    uses 5.8e-12;
  * g_x0 of the restatement equals K_0'w + gam dV_dx of sens_ref.masked_sweep / costate at 1e-12."""
import re
import os

import numpy as np
import pytest

import grad_ref as gr
import sens_ref as sr
from lq_mpc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
GRAD_SYMBOLS = ["lqmpc_model_grad_batch", "lqmpc_model_grad_batch_dev", "lqmpc_controller_model_grad", "lqmpc_controller_model_grad_dev"]
BAR = 1e-12
FD_BAR, FD_OWN = 1e-9, 1e-10


def test_grad_symbols_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lqmpc.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lqmpc_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in GRAD_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    assert len(L.lqmpc_model_grad_batch.argtypes) == 5 + 9 + 3 + 2 + 3
    assert len(L.lqmpc_controller_model_grad.argtypes) == 1 + 3 + 2 + 3


def test_null_arguments_are_refused():
    """a NULL handle or controller, a NULL plan, both cotangents NULL, a NULL g_A or g_B: LQMPC_ERR_BAD_ARG, nothing is written"""
    L = _lib.lib()
    z = np.zeros(64)
    q = z.ctypes.data
    h = 1 << 20                                        # never dereferenced: the NULL checks come first
    for f in (L.lqmpc_model_grad_batch, L.lqmpc_model_grad_batch_dev):
        m = [2, 1, 5, 1, q, q, q, q, q, q, q, None, None]
        assert f(None, *m, q, q, None, q, q, q, q, None) == -1
        assert b"NULL" in L.lqmpc_last_error()
        assert f(h, *m, None, q, None, q, q, q, q, None) == -1          # Uplan
        assert f(h, *m, q, None, None, q, q, q, q, None) == -1          # Xplan
        assert f(h, *m, q, q, None, None, None, q, q, None) == -1       # both cotangents
        assert f(h, *m, q, q, None, q, q, None, q, None) == -1          # gA
        assert f(h, *m, q, q, None, q, q, q, None, None) == -1          # gB
        assert f(h, 2, 1, 5, 1, None, q, q, q, q, q, q, None, None, q, q, None, q, q, q, q, None) == -1   # A
    for f in (L.lqmpc_controller_model_grad, L.lqmpc_controller_model_grad_dev):
        assert f(None, q, q, None, q, q, q, q, None) == -1
        assert b"NULL" in L.lqmpc_last_error()
        assert f(h, None, q, None, q, q, q, q, None) == -1
        assert f(h, q, None, None, q, q, q, q, None) == -1
        assert f(h, q, q, None, None, None, q, q, None) == -1
        assert f(h, q, q, None, q, q, None, q, None) == -1
        assert f(h, q, q, None, q, q, q, None, None) == -1
    assert np.all(z == 0.0)


def test_formula_against_richardson_central_differences():
    c = sr.case((4, 2, 10), refs=True, off_centre=True)
    idx = np.arange(8) * 25 + 3                                    # 8 instances across the batch
    p = dict(c["p"])
    for k in ("A", "B", "x0"):
        p[k] = np.ascontiguousarray(c["p"][k][..., idx])
    kw, x0, U = c["kw"], p["x0"], np.ascontiguousarray(c["U"][..., idx])
    w, gam = gr.cotangents(2, idx.size, 7)
    ref = gr.reference(p, kw, x0, U, w, gam)
    assert ref["ok"].all() and not ref["free"].all() and ref["free"][:, 0].any()
    free, Ub = ref["free"], ref["U"]
    Al, Bl = np.asarray(p["A"], dtype=LD), np.asarray(p["B"], dtype=LD)

    def D(M, r, cc, h):
        """central difference of the loss with respect to entry (r, cc) of A (M = 0) or B (M = 1), every instance at once"""
        out = []
        for s in (1, -1):
            A2, B2 = Al.copy(), Bl.copy()
            (A2, B2)[M][r, cc] += s * LD(h)
            out.append(gr.face_loss(p, kw, x0, free, Ub, w, gam, A2, B2))
        return (out[0] - out[1]) / (2 * LD(h))
    h = 1e-3
    R1, R2 = [np.zeros(Al.shape, dtype=LD), np.zeros(Bl.shape, dtype=LD)], [np.zeros(Al.shape, dtype=LD), np.zeros(Bl.shape, dtype=LD)]
    for M, G in enumerate((Al, Bl)):
        for r in range(G.shape[0]):
            for cc in range(G.shape[1]):
                d1, d2, d4 = D(M, r, cc, h), D(M, r, cc, h / 2), D(M, r, cc, h / 4)
                R1[M][r, cc], R2[M][r, cc] = (4 * d2 - d1) / 3, (4 * d4 - d2) / 3
    own = max(sr.rel_err(R1[0], R2[0], (0, 1)).max(), sr.rel_err(R1[1], R2[1], (0, 1)).max())
    eA, eB = sr.rel_err(ref["g_A"], R2[0], (0, 1)).max(), sr.rel_err(ref["g_B"], R2[1], (0, 1)).max()
    print(f"formula against Richardson differences: g_A {eA:.2e} g_B {eB:.2e}; the differences' own error {own:.2e}")
    assert own < FD_OWN
    assert eA < FD_BAR and eB < FD_BAR


# (shape, instances, refs, off-centre box)
CASES = [((2, 1, 5), 203, False, False), ((4, 2, 10), 203, False, False), ((4, 2, 10), 203, True, False), ((4, 2, 10), 203, True, True),
         ((3, 3, 4), 203, False, False), ((2, 1, 1), 203, False, False), ((8, 4, 30), 24, False, False), ((16, 4, 8), 203, False, False)]


@pytest.mark.parametrize("shape,bsz,refs,off", CASES, ids=str)
def test_adjoint_restatement_against_the_dense_reference(shape, bsz, refs, off):
    c = sr.case(shape, refs=refs, off_centre=off, bsz=bsz)
    p, kw = c["p"], c["kw"]
    w, gam = gr.cotangents(shape[1], bsz, sum(shape))
    ref = gr.reference(p, kw, p["x0"], c["U"], w, gam)
    assert ref["ok"].all()
    U = np.asarray(ref["U"], dtype=np.float64)
    free = sr.face_bits(U, p["lb"], p["ub"])
    assert np.array_equal(free, ref["free"])
    X = sr.model_roll(p, p["x0"], U)
    ad = gr.adjoint(*sr.model(p), free, X, U, w, gam, kw.get("x_ref"))
    e = {k: sr.rel_err(ad[k], ref[k], ax).max() for k, ax in (("g_A", (0, 1)), ("g_B", (0, 1)), ("g_x0", 0))}
    # the free cross-check against the sens algebra: g_x0 = K_0'w + gam dV_dx
    K0 = sr.masked_sweep(*sr.model(p), free)[:, 0]
    dV = sr.costate(p["N"], p["A"], p["Q"], p["P"], X, kw.get("x_ref"))
    cross = sr.rel_err(ad["g_x0"], np.einsum("kab,kb->ab", K0, w) + gam * dV, 0).max()
    sat0 = ~free[:, 0].any(axis=0)
    print(f"{shape} x {bsz} refs={refs} off={off}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) +
          f"; g_x0 against K_0'w + gam dV_dx {cross:.2e}; stage 0 saturated {np.mean(sat0):.2f}")
    assert max(e.values()) < BAR, e
    assert cross < BAR
