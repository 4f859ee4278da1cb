"""CPU: the closed loop with a tape and its gradient (lqmpc_rollout_tape_batch, lqmpc_rollout_grad_batch and their _dev flavours;
tests/rgrad_ref.py), on the nine cases of rgrad_ref.CASES with tapes built by the CPU oracle.

  * the four entry points are declared, exported, have their argument lists and refuse bad arguments before they touch a GPU: a NULL
    handle, model, plant or tape, every cotangent NULL, every output NULL, T < 1 (LQMPC_ERR_BAD_ARG), a shape whose LDS image is over
    160 KiB (LQMPC_ERR_UNSUPPORTED; rgrad_ref.lds_bytes restates the image, and the list of refused shapes is that of DESIGN.md 4.14);
  * (a) the tapes: on every case the face each slice reports bit for bit is the certified one on at least 99 % of the instances, and at
    (4,2,10), T = 6 each kind of step -- stage 0 wholly on bounds, a mixed face, all free -- has at least 10 % of the (t, b) pairs
    (measured: 25 %, 28 %, 47 %);
  * (b) the restatement: rgrad_ref.adjoint (fp64 numpy, the algebra of lqmpc_rollout_grad_kernel) against rgrad_ref.reference (long
    double; per step the dense grad_ref.reference, no Riccati sweep), sens_ref.rel_err per instance.  Measured worst over the nine
    cases: g_B 9.67e-14 and g_A 2.17e-14 at (4,2,10) with references and the off-centre box, g_x0 2.8e-15, g_A_true 1.1e-15,
    g_B_true 1.1e-15.  Held to rgrad_ref.CPU_WORST = 1.0e-13; the GPU tests' bar is 100 times that figure, 1.0e-11 (the rule of
    tests/test_gpu_pgrad.py);
  * (c) the formula: rgrad_ref.adjoint against Richardson-extrapolated central differences, in long double, of rgrad_ref.loop_loss (the
    closed loop with every step's face held fixed) with respect to every entry of A, B, A_true, B_true and x0, on the FD_INST instances
    of three cases whose tape is the most mixed.  Steps h = 1e-3, h / 2, h / 4 as tests/test_pgrad_cpu.py: bar 1e-9 relative to
    max(|g|_max, 1) per instance, the differences' own error |R(h) - R(h/2)| asserted below 1e-10.  Measured worst: 6.0e-12 (g_B at
    (2,1,5)), own error 9.0e-11 there;
  * (d) T = 1 with cotangents on U and J_T only is one grad_ref.adjoint call with gu0 = w_0, to rounding."""
import os
import re

import numpy as np
import pytest

import grad_ref as gr
import rgrad_ref as rg
import sens_ref as sr
from lq_mpc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
RGRAD_SYMBOLS = ["lqmpc_rollout_tape_batch", "lqmpc_rollout_tape_batch_dev", "lqmpc_rollout_grad_batch", "lqmpc_rollout_grad_batch_dev"]
FD_BAR, FD_OWN = 1e-9, 1e-10
FD_INST = 4
FD_CASES = [0, 1, 2]                               # indices into rgrad_ref.CASES: (2,1,5) T = 3, (4,2,10) T = 6, (3,3,4) T = 4
_WORST = {}


def test_rgrad_symbols_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lqmpc.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lqmpc_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in RGRAD_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    assert len(L.lqmpc_rollout_tape_batch.argtypes) == len(L.lqmpc_rollout_batch.argtypes) + 2
    assert len(L.lqmpc_rollout_grad_batch.argtypes) == 6 + 9 + 1 + 2 + 3 + 3 + 5
    mk = open(os.path.join(ROOT, "lq_mpc_amd", "csrc", "Makefile")).read()
    assert "lqmpc_rgrad.hip" in re.search(r"^SRC\s*:=(.*)$", mk, flags=re.M).group(1)


def test_bad_arguments_are_refused():
    """LQMPC_ERR_BAD_ARG before anything is enqueued, nothing is written; the handle is never dereferenced"""
    L = _lib.lib()
    z = np.zeros(64)
    q = z.ctypes.data
    h = 1 << 20                                        # never dereferenced: the checks come first
    for f in (L.lqmpc_rollout_grad_batch, L.lqmpc_rollout_grad_batch_dev):
        def call(handle=h, T=3, **holes):
            a = dict(A=q, B=q, Q=q, R=q, P=q, lb=q, ub=q, At=q, Bt=q, tpi=0, xr=None, ur=None, X=q, Ut=q, st=None, gJ=q, gX=q, gU=q,
                     gA=q, gB=q, gx=q, gAt=q, gBt=q)
            a.update(holes)
            return f(handle, 2, 1, 5, 1, T, *a.values())
        assert call(handle=None) == -1
        assert b"NULL" in L.lqmpc_last_error()
        for hole in ("A", "B", "At", "Bt", "X", "Ut"):
            assert call(**{hole: None}) == -1, hole
            assert b"NULL" in L.lqmpc_last_error()
        assert call(gJ=None, gX=None, gU=None) == -1
        assert b"cotangent" in L.lqmpc_last_error()
        assert call(gA=None, gB=None, gx=None, gAt=None, gBt=None) == -1
        assert b"output" in L.lqmpc_last_error()
        assert call(T=0) == -1 and call(T=-1) == -1
        assert b"T must" in L.lqmpc_last_error()
    for f in (L.lqmpc_rollout_tape_batch, L.lqmpc_rollout_tape_batch_dev):
        def call(handle=h, T=3, **holes):
            a = dict(A=q, B=q, Q=q, R=q, P=q, lb=q, ub=q, x0=q, At=q, Bt=q, tpi=0, xr=None, ur=None, JT=q, X=q, U=q, st=None, it=None,
                     Ut=q, stt=None)
            a.update(holes)
            return f(handle, 2, 1, 5, 1, T, *a.values())
        assert call(handle=None) == -1
        for hole in ("A", "B", "x0", "At", "Bt", "JT", "Ut"):
            assert call(**{hole: None}) == -1, hole
            assert b"NULL" in L.lqmpc_last_error()
        assert call(T=0) == -1
        assert b"T must" in L.lqmpc_last_error()
    assert np.all(z == 0.0)


def test_shapes_over_the_lds_limit_are_refused():
    """LQMPC_ERR_UNSUPPORTED from the host's own image, before the handle is touched: every shape of the build limits is asked"""
    L = _lib.lib()
    lb, ub, eye = np.array([-1.0] * 8), np.array([1.0] * 8), np.eye(16)
    z = np.zeros(16 * 16 * 65)
    q = z.ctypes.data
    h = 1 << 20
    refused = set(rg.refused_shapes())
    assert (16, 2, 64) in refused and (16, 4, 8) not in refused and (8, 4, 30) not in refused
    for f in (L.lqmpc_rollout_grad_batch, L.lqmpc_rollout_grad_batch_dev):
        for nx, nu, N in sorted(refused):
            Q, R = np.ascontiguousarray(eye[:nx, :nx]), np.ascontiguousarray(eye[:nu, :nu])
            rc = f(h, nx, nu, N, 1, 2, q, q, Q.ctypes.data, R.ctypes.data, Q.ctypes.data, lb.ctypes.data, ub.ctypes.data, q, q, 0, None, None,
                   q, q, None, q, q, q, q, None, None, None, None)
            assert rc == -5, (nx, nu, N)
            assert b"LDS" in L.lqmpc_last_error()
    assert rg.lds_bytes(*rg.largest_admitted()) <= rg.LDS_LIMIT


def _restatement(shape, T, bsz, how):
    """the errors of the fp64 restatement on one case, the share of instances compared and the mix of its tape: computed once"""
    key = (shape, T, bsz, str(how))
    if key not in _WORST:
        c = rg.case(shape, T, bsz=bsz, **how)
        p, kw, tape = c["p"], c["kw"], c["tape"]
        gJT, gX, gU = rg.cotangents(shape[0], shape[1], T, bsz, sum(shape))
        ref = rg.reference(p, kw, c["At"], c["Bt"], tape["X"], tape["U_tape"], gJT, gX, gU)
        free = rg.tape_faces(tape["U_tape"], p["lb"], p["ub"])
        same = np.all(free == ref["free"], axis=(0, 1, 2))
        ad = rg.adjoint(*sr.model(p), c["At"], c["Bt"], free, tape["X"], tape["U_tape"], gJT, gX, gU, kw.get("x_ref"))
        e = {k: sr.rel_err(ad[k], ref[k], ax)[same].max() for k, ax in rg.KEYS}
        _WORST[key] = (e, same, rg.kinds(free), bool(ref["ok"].all()))
    return _WORST[key]


@pytest.mark.parametrize("shape,T,bsz,how", rg.CASES, ids=str)
def test_adjoint_restatement_against_the_dense_reference(shape, T, bsz, how):
    e, same, mix, ok = _restatement(shape, T, bsz, how)
    print(f"{shape} T={T} x {bsz} {how}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) +
          f"; compared {int(same.sum())} of {same.size}; stage 0 on bounds / mixed / all free {mix[0]:.2f} / {mix[1]:.2f} / {mix[2]:.2f}")
    assert ok
    assert np.mean(~same) <= 0.01
    if shape == (4, 2, 10) and not how:                             # (under the off-centre box with references no step is all free)
        assert min(mix) >= 0.10, mix
    assert max(e.values()) <= rg.CPU_WORST, e


def test_the_gpu_bar_is_a_hundred_times_the_worst_of_these_cases():
    """the figure the GPU bar is formed from is the worst over the nine cases, rounded up by less than a factor of two"""
    worst = max(max(_restatement(*case)[0].values()) for case in rg.CASES)
    print(f"worst of the fp64 restatement over the cases: {worst:.3e}; CPU_WORST {rg.CPU_WORST:.1e}; GPU bar {rg.GPU_BAR:.1e}")
    assert worst <= rg.CPU_WORST <= 2 * worst


@pytest.mark.parametrize("which", FD_CASES)
def test_adjoint_against_richardson_central_differences_of_the_loop(which):
    shape, T, bsz, how = rg.CASES[which]
    c = rg.case(shape, T, bsz=bsz, **how)
    p0, kw, tape = c["p"], c["kw"], c["tape"]
    nx, nu, N = shape
    faces = rg.tape_faces(tape["U_tape"], p0["lb"], p0["ub"])
    # the instances whose tape has the most steps on a mixed face, then the most kinds of step
    sat, allfree = ~faces[:, :, 0].any(axis=1), faces.all(axis=(1, 2))
    score = 2 * (~sat & ~allfree).sum(axis=0) + sat.any(axis=0) + allfree.any(axis=0)
    idx = np.sort(np.argsort(-score, kind="stable")[:FD_INST])
    inst = idx.size
    p = dict(p0)
    for k in ("A", "B", "x0"):
        p[k] = np.ascontiguousarray(p0[k][..., idx])
    X, Ut = np.ascontiguousarray(tape["X"][..., idx]), np.ascontiguousarray(tape["U_tape"][..., idx])
    gJT, gX, gU = rg.cotangents(nx, nu, T, inst, sum(shape))
    gJT[0] = 0.7                                                     # (every third is exactly 0: keep both kinds among the few)
    ref = rg.reference(p, kw, c["At"], c["Bt"], X, Ut, gJT, gX, gU)
    assert ref["ok"].all()
    free = ref["free"]
    assert np.array_equal(free, faces[..., idx])
    from oracle import exact as ex
    Ub = np.stack([ex.certify(*sr.qa(p), np.ascontiguousarray(X[:, t]), Ut[t], kw.get("x_ref"), kw.get("u_ref"))["U"] for t in range(T)])
    ad = rg.adjoint(*sr.model(p), c["At"], c["Bt"], free, X, Ut, gJT, gX, gU, kw.get("x_ref"))
    per = lambda M: np.ascontiguousarray(np.moveaxis(np.broadcast_to(M, (inst,) + M.shape), 0, -1))
    base = [np.asarray(a, dtype=LD) for a in (p["A"], p["B"], per(c["At"]), per(c["Bt"]), p["x0"])]

    h = 1e-3
    steps = [sg * LD(h) / k for k in (1, 2, 4) for sg in (1, -1)]
    entries = [(M, where) for M, G in enumerate(base) for where in np.ndindex(*G.shape[:-1])]
    R1, R2 = [np.zeros(a.shape, dtype=LD) for a in base], [np.zeros(a.shape, dtype=LD) for a in base]
    chunk = 8
    tile = lambda a, m: np.concatenate([a] * m, axis=-1)
    for lo in range(0, len(entries), chunk):
        part = entries[lo:lo + chunk]
        m = len(part) * len(steps)
        v = [tile(a, m) for a in base]
        for e, (M, where) in enumerate(part):
            for t, st in enumerate(steps):
                col = (e * len(steps) + t) * inst
                v[M][where + (slice(col, col + inst),)] += st
        L = rg.loop_loss(p, kw, v[2], v[3], v[4], tile(free, m), tile(Ub, m), tile(gJT, m), tile(gX, m), tile(gU, m), v[0], v[1])
        L = L.reshape(len(part), 3, 2, inst)
        for e, (M, where) in enumerate(part):
            d1, d2, d4 = ((L[e, k, 0] - L[e, k, 1]) / (2 * LD(h) / 2 ** k) for k in range(3))
            R1[M][where], R2[M][where] = (4 * d2 - d1) / 3, (4 * d4 - d2) / 3
    keys = ("g_A", "g_B", "g_A_true", "g_B_true", "g_x0")
    axes = ((0, 1), (0, 1), (0, 1), (0, 1), 0)
    own = max(sr.rel_err(R1[M], R2[M], axes[M]).max() for M in range(5))
    e = {k: sr.rel_err(ad[k], R2[M], axes[M]).max() for M, k in enumerate(keys)}
    print(f"{shape} T={T}: adjoint against Richardson differences of the loop: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) +
          f"; the differences' own error {own:.2e}; kinds of step {rg.kinds(free)}")
    assert own < FD_OWN
    assert max(e.values()) < FD_BAR, e


def test_one_step_is_one_model_gradient():
    """T = 1, gX NULL: g_A, g_B of the loop are those of grad_ref.adjoint for gu0 = gU_0 + 2 gJT (R u_0 + B_true'Q x_1), gVN = 0, to
    rounding"""
    shape, T, bsz, how = rg.CASES[3]
    assert T == 1
    c = rg.case(shape, T, bsz=bsz, **how)
    p, tape = c["p"], c["tape"]
    gJT, _, gU = rg.cotangents(shape[0], shape[1], T, bsz, 5)
    free = rg.tape_faces(tape["U_tape"], p["lb"], p["ub"])
    mine = rg.adjoint(*sr.model(p), c["At"], c["Bt"], free, tape["X"], tape["U_tape"], gJT, None, gU)
    u0 = tape["U_tape"][0][:, 0]
    w0 = gU[:, 0] + 2 * gJT * (p["R"] @ u0) + np.einsum("ik,ib->kb", c["Bt"], 2 * gJT * (p["Q"] @ tape["X"][:, 1]))
    Xp = sr.model_roll(p, p["x0"], tape["U_tape"][0])
    theirs = gr.adjoint(*sr.model(p), free[0], Xp, tape["U_tape"][0], w0, np.zeros(bsz))
    e = max(sr.rel_err(mine[k], theirs[k], (0, 1)).max() for k in ("g_A", "g_B"))
    print(f"one step against grad_ref.adjoint: {e:.2e}")
    assert e < 1e-14
    assert np.any(mine["g_A"] != 0.0)
