"""CPU: the gradient of a loss on the whole plan (every u_i, every x_i, V_N) with respect to A, B and x0 (lqmpc_plan_grad_batch,
lqmpc_controller_plan_grad and their _dev flavours; tests/pgrad_ref.py), on the eight cases of tests/test_grad_cpu.py.

  * the four entry points are declared, exported and refuse bad arguments before they touch a GPU;
  * (a) the formula: pgrad_ref.reference (dense, long double) against Richardson-extrapolated central differences, in long double, of
    sum w_i'u_i + sum s_i'x_i + gam V at the optimum of the plan's face held fixed (pgrad_ref.face_loss), with respect to every entry
    of A, B and x0, on the FD_INST instances of every case whose face is the most mixed (two at nx = 16, one at (8,4,30): the
    long-double work).  Steps h = 1e-3 and h / 2: D(h) = (f(+h) - f(-h)) / 2h, R(h) = (4 D(h/2) - D(h)) / 3, whose error is O(h^4).
    As tests/test_grad_cpu.py: bar 1e-9 relative to max(|g|_max, 1) per instance, and the differences' own error, |R(h) - R(h/2)|,
    asserted below 1e-10.  Measured worst over the cases: own error 2.6e-11 at (4,2,10); R(h/2) against the formula g_A 1.7e-12,
    g_B 1.5e-12, g_x0 1.5e-14;
  * (b) the restatement: pgrad_ref.adjoint (fp64 numpy, the algebra of lqmpc_plan_grad_kernel, the sweep with its affine part) against
    pgrad_ref.reference on the faces of the oracle's own plans (the face read off the plan bit for bit is the certified one on every
    instance of every case), sens_ref.rel_err per instance.  Bar 1e-12.  Measured worst over the eight cases: g_A 6.93e-14 at
    (2,1,5), g_B 3.5e-14, g_x0 5.9e-15.  The GPU tests' bar is 100 times the worst, rounded up to 7.0e-12 (DESIGN.md section 4.11's
    rule: measured against the long-double reference, with margin for another summation order): tests/test_gpu_pgrad.py uses 7.0e-12;
  * (c) with cotangents on u_0 and V_N only, pgrad_ref.adjoint equals grad_ref.adjoint at 1e-12;
  * (d) g_x0 of a one-hot w at (i, k) (s = 0, gam = 0) equals row (k, i) of K_plan of sens_ref.masked_sweep at 1e-12, for every (i, k)."""
import re
import os

import numpy as np
import pytest

import grad_ref as gr
import pgrad_ref as pg
import sens_ref as sr
from lq_mpc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
PGRAD_SYMBOLS = ["lqmpc_plan_grad_batch", "lqmpc_plan_grad_batch_dev", "lqmpc_controller_plan_grad", "lqmpc_controller_plan_grad_dev"]
BAR = 1e-12
FD_BAR, FD_OWN = 1e-9, 1e-10
FD_INST = 4

# (shape, instances, refs, off-centre box): the cases of tests/test_grad_cpu.py
CASES = [((2, 1, 5), 203, False, False), ((4, 2, 10), 203, False, False), ((4, 2, 10), 203, True, False), ((4, 2, 10), 203, True, True),
         ((3, 3, 4), 203, False, False), ((2, 1, 1), 203, False, False), ((8, 4, 30), 24, False, False), ((16, 4, 8), 203, False, False)]


def test_pgrad_symbols_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lqmpc.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lqmpc_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in PGRAD_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    assert len(L.lqmpc_plan_grad_batch.argtypes) == 5 + 9 + 3 + 3 + 3
    assert len(L.lqmpc_controller_plan_grad.argtypes) == 1 + 3 + 3 + 3


def test_null_arguments_are_refused():
    """a NULL handle or controller, a NULL model or plan, every cotangent NULL, every output NULL: LQMPC_ERR_BAD_ARG, nothing is written"""
    L = _lib.lib()
    z = np.zeros(64)
    q = z.ctypes.data
    h = 1 << 20                                        # never dereferenced: the NULL checks come first
    for f in (L.lqmpc_plan_grad_batch, L.lqmpc_plan_grad_batch_dev):
        m = [2, 1, 5, 1, q, q, q, q, q, q, q, None, None]
        assert f(None, *m, q, q, None, q, q, q, q, q, q) == -1
        assert b"NULL" in L.lqmpc_last_error()
        assert f(h, *m, None, q, None, q, q, q, q, q, q) == -1             # Uplan
        assert f(h, *m, q, None, None, q, q, q, q, q, q) == -1             # Xplan
        assert f(h, *m, q, q, None, None, None, None, q, q, q) == -1       # every cotangent
        assert b"cotangent" in L.lqmpc_last_error()
        assert f(h, *m, q, q, None, q, q, q, None, None, None) == -1       # every output
        assert b"output" in L.lqmpc_last_error()
        assert f(h, 2, 1, 5, 1, None, q, q, q, q, q, q, None, None, q, q, None, q, q, q, q, q, q) == -1   # A
        assert f(h, 2, 1, 5, 1, q, None, q, q, q, q, q, None, None, q, q, None, q, q, q, q, q, q) == -1   # B
    for f in (L.lqmpc_controller_plan_grad, L.lqmpc_controller_plan_grad_dev):
        assert f(None, q, q, None, q, q, q, q, q, q) == -1
        assert b"NULL" in L.lqmpc_last_error()
    assert np.all(z == 0.0)


def _subset(c, idx):
    p = dict(c["p"])
    for k in ("A", "B", "x0"):
        p[k] = np.ascontiguousarray(c["p"][k][..., idx])
    return p, np.ascontiguousarray(c["U"][..., idx])


@pytest.mark.parametrize("shape,bsz,refs,off", CASES, ids=str)
def test_formula_against_richardson_central_differences(shape, bsz, refs, off):
    c = sr.case(shape, refs=refs, off_centre=off, bsz=bsz)
    nx, nu, N = shape
    # the instances whose face is the most mixed (the long-double work grows with instances x entries x n^3: one at n = 120, two at
    # the 336 entries of nx = 16)
    inst = 1 if nu * N > 100 else 2 if nx == 16 else FD_INST
    mixed = np.abs(sr.face_bits(c["U"], c["p"]["lb"], c["p"]["ub"]).mean(axis=(0, 1)) - 0.5)
    idx = np.sort(np.argsort(mixed, kind="stable")[:inst])
    p, U = _subset(c, idx)
    kw, x0 = c["kw"], p["x0"]
    w, s, gam = pg.cotangents(nx, nu, N, idx.size, sum(shape))
    gam[0] = 0.7                                                     # (every third is exactly 0: keep both kinds among the few)
    ref = pg.reference(p, kw, x0, U, w, s, gam)
    assert ref["ok"].all()
    free, Ub = ref["free"], ref["U"]
    base = [np.asarray(p["A"], dtype=LD), np.asarray(p["B"], dtype=LD), np.asarray(x0, dtype=LD)]

    h = 1e-3
    steps = [sg * LD(h) / k for k in (1, 2, 4) for sg in (1, -1)]
    entries = [(M, where) for M, G in enumerate(base) for where in np.ndindex(*G.shape[:-1])]
    R1, R2 = [np.zeros(a.shape, dtype=LD) for a in base], [np.zeros(a.shape, dtype=LD) for a in base]
    chunk = 8                                                        # entries per face_loss call: 8 * 6 * inst models at once
    tile = lambda a, m: np.concatenate([a] * m, axis=-1)
    for lo in range(0, len(entries), chunk):
        part = entries[lo:lo + chunk]
        m = len(part) * len(steps)
        v = [tile(a, m) for a in base]
        for e, (M, where) in enumerate(part):
            for t, st in enumerate(steps):
                col = (e * len(steps) + t) * inst
                v[M][where + (slice(col, col + inst),)] += st
        L = pg.face_loss(p, kw, v[2], tile(free, m), tile(Ub, m), tile(w, m), tile(s, m), tile(gam, m), v[0], v[1])
        L = L.reshape(len(part), 3, 2, inst)
        for e, (M, where) in enumerate(part):
            d1, d2, d4 = ((L[e, k, 0] - L[e, k, 1]) / (2 * LD(h) / 2 ** k) for k in range(3))
            R1[M][where], R2[M][where] = (4 * d2 - d1) / 3, (4 * d4 - d2) / 3
    axes = ((0, 1), (0, 1), 0)
    own = max(sr.rel_err(R1[M], R2[M], axes[M]).max() for M in range(3))
    e = {k: sr.rel_err(ref[k], R2[M], axes[M]).max() for M, k in enumerate(("g_A", "g_B", "g_x0"))}
    print(f"{shape} refs={refs} off={off}: formula against Richardson differences: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) +
          f"; the differences' own error {own:.2e}; free entries {free.mean():.2f}")
    assert own < FD_OWN
    assert max(e.values()) < FD_BAR, e


def _oracle_face(c):
    """the certified optimum of the oracle's plan in fp64, its face and its states"""
    p, kw = c["p"], c["kw"]
    from oracle import exact as ex
    cert = ex.certify(*sr.qa(p), p["x0"], c["U"], kw.get("x_ref"), kw.get("u_ref"))
    assert cert["ok"].all()
    U = np.asarray(cert["U"], dtype=np.float64)
    free = sr.face_bits(U, p["lb"], p["ub"])
    assert np.array_equal(free, sr.face_of(cert["U"], p["lb"], p["ub"]))
    return U, free, sr.model_roll(p, p["x0"], U)


@pytest.mark.parametrize("shape,bsz,refs,off", CASES, ids=str)
def test_adjoint_restatement_against_the_dense_reference(shape, bsz, refs, off):
    c = sr.case(shape, refs=refs, off_centre=off, bsz=bsz)
    p, kw = c["p"], c["kw"]
    nx, nu, N = shape
    w, s, gam = pg.cotangents(nx, nu, N, bsz, sum(shape))
    ref = pg.reference(p, kw, p["x0"], c["U"], w, s, gam)
    assert ref["ok"].all()
    U, free, X = _oracle_face(c)
    assert np.array_equal(free, ref["free"])
    ad = pg.adjoint(*sr.model(p), free, X, U, w, s, gam, kw.get("x_ref"))
    e = {k: sr.rel_err(ad[k], ref[k], ax).max() for k, ax in pg.KEYS}
    print(f"{shape} x {bsz} refs={refs} off={off}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) + f"; free entries {free.mean():.2f}")
    assert max(e.values()) < BAR, e


@pytest.mark.parametrize("shape,bsz,refs,off", CASES, ids=str)
def test_cotangents_on_u0_and_VN_alone_give_the_model_gradient(shape, bsz, refs, off):
    c = sr.case(shape, refs=refs, off_centre=off, bsz=bsz)
    p, kw = c["p"], c["kw"]
    nx, nu, N = shape
    U, free, X = _oracle_face(c)
    w0, gam = gr.cotangents(nu, bsz, sum(shape))
    w = np.zeros((nu, N, bsz))
    w[:, 0] = w0
    mine = pg.adjoint(*sr.model(p), free, X, U, w, np.zeros((nx, N + 1, bsz)), gam, kw.get("x_ref"))
    theirs = gr.adjoint(*sr.model(p), free, X, U, w0, gam, kw.get("x_ref"))
    e = {k: sr.rel_err(mine[k], theirs[k], ax).max() for k, ax in pg.KEYS}
    print(f"{shape} x {bsz}: against grad_ref.adjoint " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) < BAR, e


@pytest.mark.parametrize("shape,bsz,refs,off", CASES, ids=str)
def test_gx0_of_a_one_hot_w_is_a_row_of_K_plan(shape, bsz, refs, off):
    c = sr.case(shape, refs=refs, off_centre=off, bsz=bsz)
    p, kw = c["p"], c["kw"]
    nx, nu, N = shape
    U, free, X = _oracle_face(c)
    Kp = sr.masked_sweep(*sr.model(p), free)                       # (nu, N, nx, Bsz)
    zs, zg = np.zeros((nx, N + 1, bsz)), np.zeros(bsz)
    worst = 0.0
    for i in range(N):
        for k in range(nu):
            w = np.zeros((nu, N, bsz))
            w[k, i] = 1.0
            gx = pg.adjoint(*sr.model(p), free, X, U, w, zs, zg, kw.get("x_ref"))["g_x0"]
            worst = max(worst, sr.rel_err(gx, Kp[k, i], 0).max())
            assert np.all(gx[:, ~free[k, i]] == 0.0)
    print(f"{shape} x {bsz}: g_x0 of one-hot w against K_plan, worst over every (i, k): {worst:.2e}")
    assert worst < BAR
