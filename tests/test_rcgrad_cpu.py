"""CPU: the gradient of the closed loop in the weights, the references and the box (lqmpc_rollout_cost_grad_batch and its _dev flavour;
tests/rcgrad_ref.py), on the nine cases of rgrad_ref.CASES with tapes built by the CPU oracle.

  * the two entry points are declared, exported, have their argument lists and refuse bad arguments before they touch a GPU: a NULL
    handle, model, plant or tape, every cotangent NULL, every output NULL, T < 1 (LQMPC_ERR_BAD_ARG), a shape whose LDS image is over
    160 KiB (LQMPC_ERR_UNSUPPORTED; rcgrad_ref.lds_bytes restates the image, and the list of refused shapes is that of DESIGN.md 4.15);
  * (a) the restatement: rcgrad_ref.adjoint (fp64 numpy, the algebra of lqmpc_rollout_cost_grad_kernel) against rcgrad_ref.reference
    (long double; per step the dense cgrad_ref.reference and grad_ref.reference, no Riccati sweep), sens_ref.rel_err per instance and
    output, over the instances whose tape reports the certified face at every step (at most 1 % are left out).  The measured worst
    over the nine cases is printed, and held to rcgrad_ref.CPU_WORST; the GPU tests' bar is 100 times that figure;
  * (b) the formula: rcgrad_ref.adjoint in long double against Richardson-extrapolated central differences, in long double, of
    rcgrad_ref.loop_loss (the closed loop with every step's face held fixed) with respect to every entry of Q, R, P, lb, ub, x_ref and
    u_ref (a weight matrix is perturbed symmetrically and the difference compared with g_ac + g_ca, as tests/test_cgrad_cpu.py does), on the FD_INST instances of three cases whose tape is the most mixed.  Steps h = 1e-3, h / 2, h / 4 as
    tests/test_rgrad_cpu.py: bar 1e-9 relative to max(|g|_max, 1) per instance, the differences' own error |R(h) - R(h/2)| asserted
    below 1e-10 (the loss is a rational function of the data on a fixed face; the remainder of the extrapolated difference is of order
    h^4 = 1e-12 times the fifth derivative, rounding of a long-double loss of order 1e2 over h / 4 is 1e-19 * 1e2 / 2.5e-4 = 4e-14);
  * (c) T = 1 with gJT = 0 is one cgrad_ref.adjoint call with w = gU_0 + B_true'gX_1, to rounding;
  * (d) gX = gU = 0, gJT = 1 where every step is all free and the model is the plant: g_P, which is not zero because P shapes the
    feedback law, against a central difference of the loop."""
import os
import re

import numpy as np
import pytest

import cgrad_ref as cg
import rcgrad_ref as rc
import rgrad_ref as rg
import sens_ref as sr
from lq_mpc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
RCGRAD_SYMBOLS = ["lqmpc_rollout_cost_grad_batch", "lqmpc_rollout_cost_grad_batch_dev"]
FD_BAR, FD_OWN = 1e-9, 1e-10
FD_INST = 4
FD_CASES = [0, 1, 2]                               # indices into rcgrad_ref.CASES: (2,1,5) T = 3, (4,2,10) T = 6, (3,3,4) T = 4
_WORST = {}


def test_rcgrad_symbols_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lqmpc.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lqmpc_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in RCGRAD_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    assert len(L.lqmpc_rollout_cost_grad_batch.argtypes) == 6 + 9 + 1 + 2 + 3 + 3 + 1 + 8
    assert L.lqmpc_rollout_cost_grad_batch_dev.argtypes == L.lqmpc_rollout_cost_grad_batch.argtypes
    mk = open(os.path.join(ROOT, "lq_mpc_amd", "csrc", "Makefile")).read()
    assert "lqmpc_rcgrad.hip" in re.search(r"^SRC\s*:=(.*)$", mk, flags=re.M).group(1)
    from lq_mpc_amd.mpc import BatchSolver
    assert hasattr(BatchSolver, "rollout_cost_grad_batch") and hasattr(BatchSolver, "rollout_cost_grad_batch_dev")


def test_bad_arguments_are_refused():
    """LQMPC_ERR_BAD_ARG before anything is enqueued, nothing is written; the handle is never dereferenced"""
    L = _lib.lib()
    z = np.zeros(64)
    q = z.ctypes.data
    h = 1 << 20                                        # never dereferenced: the checks come first
    outs = ("gQ", "gR", "gP", "glb", "gub", "gxr", "gur")
    for f in (L.lqmpc_rollout_cost_grad_batch, L.lqmpc_rollout_cost_grad_batch_dev):
        for reduce in (0, 1):
            def call(handle=h, T=3, **holes):
                a = dict(A=q, B=q, Q=q, R=q, P=q, lb=q, ub=q, At=q, Bt=q, tpi=0, xr=None, ur=None, X=q, Ut=q, st=None, gJ=q, gX=q, gU=q,
                         red=reduce, gQ=q, gR=q, gP=q, glb=q, gub=q, gxr=q, gur=q, ns=None)
                a.update(holes)
                return f(handle, 2, 1, 5, 1, T, *a.values())
            assert call(handle=None) == -1
            assert b"NULL" in L.lqmpc_last_error()
            for hole in ("A", "B", "At", "Bt", "X", "Ut"):
                assert call(**{hole: None}) == -1, hole
                assert b"NULL" in L.lqmpc_last_error()
            assert call(gJ=None, gX=None, gU=None) == -1
            assert b"cotangent" in L.lqmpc_last_error()
            assert call(**{k: None for k in outs}) == -1
            assert b"output" in L.lqmpc_last_error()
            assert call(T=0) == -1 and call(T=-1) == -1 and call(T=100001) == -1
            assert b"T must" in L.lqmpc_last_error()
    assert np.all(z == 0.0)


def test_shapes_over_the_lds_limit_are_refused():
    """LQMPC_ERR_UNSUPPORTED from the host's own image, before the handle is touched: every refused shape of the build limits is asked, and
    the largest admitted one gets past this check (its NULL tape stops it: LQMPC_ERR_BAD_ARG comes first, so a valid call is made up
    to the handle, which is NULL)"""
    L = _lib.lib()
    lb, ub, eye = np.array([-1.0] * 8), np.array([1.0] * 8), np.eye(16)
    z = np.zeros(16 * 16 * 65)
    q = z.ctypes.data
    h = 1 << 20
    refused = set(rc.refused_shapes())
    print(f"{len(refused)} shapes refused; the largest admitted {rc.largest_admitted()} takes {rc.lds_bytes(*rc.largest_admitted())} bytes")
    assert (16, 2, 64) in refused and (16, 8, 14) in refused and (16, 4, 8) not in refused and (8, 4, 30) not in refused
    assert 2 * rc.lds_bytes(8, 4, 30) <= rc.LDS_LIMIT                # two workgroups of the C5 shape fit a CU
    every = [(nx, nu, N) for nx in range(1, 17) for nu in range(1, 9) for N in range(1, 65) if nu * N <= 128]
    for f in (L.lqmpc_rollout_cost_grad_batch, L.lqmpc_rollout_cost_grad_batch_dev):
        for nx, nu, N in sorted(refused):
            Q, R = np.ascontiguousarray(eye[:nx, :nx]), np.ascontiguousarray(eye[:nu, :nu])
            rcode = f(h, nx, nu, N, 1, 2, q, q, Q.ctypes.data, R.ctypes.data, Q.ctypes.data, lb.ctypes.data, ub.ctypes.data, q, q, 0, None,
                      None, q, q, None, q, q, q, 0, q, None, None, None, None, None, None, None)
            assert rcode == -5, (nx, nu, N)
            assert b"LDS" in L.lqmpc_last_error()
    assert rc.lds_bytes(*rc.largest_admitted()) <= rc.LDS_LIMIT
    assert len(refused) < len(every)
    nx, nu, N = rc.largest_admitted()
    Q, R = np.ascontiguousarray(eye[:nx, :nx]), np.ascontiguousarray(eye[:nu, :nu])
    for f in (L.lqmpc_rollout_cost_grad_batch, L.lqmpc_rollout_cost_grad_batch_dev):
        rcode = f(None, nx, nu, N, 1, 2, q, q, Q.ctypes.data, R.ctypes.data, Q.ctypes.data, lb.ctypes.data, ub.ctypes.data, q, q, 0, None,
                  None, q, q, None, q, q, q, 0, q, None, None, None, None, None, None, None)
        assert rcode == -1 and b"LDS" not in L.lqmpc_last_error()


def _restatement(shape, T, bsz, how):
    """the errors of the fp64 restatement on one case, the instances compared and the mix of its tape: computed once"""
    key = (shape, T, bsz, str(how))
    if key not in _WORST:
        c = rg.case(shape, T, bsz=bsz, **how)
        p, kw, tape = c["p"], c["kw"], c["tape"]
        gJT, gX, gU = rg.cotangents(shape[0], shape[1], T, bsz, sum(shape))
        ref = rc.reference(p, kw, c["At"], c["Bt"], tape["X"], tape["U_tape"], gJT, gX, gU)
        side = rc.tape_sides(tape["U_tape"], p["lb"], p["ub"])
        same = np.all(side == ref["side"], axis=(0, 1, 2))
        ad = rc.adjoint(*sr.model(p), c["At"], c["Bt"], side, tape["X"], tape["U_tape"], gJT, gX, gU, kw.get("x_ref"), kw.get("u_ref"))
        e = {k: sr.rel_err(ad[k], ref[k], ax)[same].max() for k, ax in rc.KEYS}
        _WORST[key] = (e, same, rg.kinds(side == 0), bool(ref["ok"].all()))
    return _WORST[key]


@pytest.mark.parametrize("shape,T,bsz,how", rc.CASES, ids=str)
def test_adjoint_restatement_against_the_dense_reference(shape, T, bsz, how):
    e, same, mix, ok = _restatement(shape, T, bsz, how)
    print(f"{shape} T={T} x {bsz} {how}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) +
          f"; compared {int(same.sum())} of {same.size}, left out {int((~same).sum())}; stage 0 on bounds / mixed / all free "
          f"{mix[0]:.2f} / {mix[1]:.2f} / {mix[2]:.2f}")
    assert ok
    assert np.mean(~same) <= rc.LEFT_OUT_CAP
    if shape == (4, 2, 10) and not how:
        assert min(mix) >= 0.10, mix
    assert max(e.values()) <= rc.CPU_WORST, e


def test_the_gpu_bar_is_a_hundred_times_the_worst_of_these_cases():
    """the figure the GPU bar is formed from is the worst over the nine cases, rounded up by less than a factor of two"""
    worst = max(max(_restatement(*case)[0].values()) for case in rc.CASES)
    print(f"worst of the fp64 restatement over the cases: {worst:.3e}; CPU_WORST {rc.CPU_WORST:.1e}; GPU bar {rc.GPU_BAR:.1e}")
    assert worst <= rc.CPU_WORST <= 2 * worst
    assert rc.GPU_BAR == 100 * rc.CPU_WORST


SYMMETRIC = ("Q", "R", "P")


def _richardson(loss, base, h=1e-3):
    """Richardson-extrapolated central differences of loss(**{name: array}) in every entry of every array of `base` (a dict of long
    double arrays): two estimates, from (h, h/2) and from (h/2, h/4), each (entry shape + (inst,)).  A weight matrix stays symmetric:
    entries (a, c) and (c, a) move together, and what the difference sees is g_ac + g_ca (_fold), as tests/test_cgrad_cpu.py has it."""
    R1, R2 = {}, {}
    for k, v in base.items():
        inst = None
        r1, r2 = [], []
        for where in np.ndindex(*v.shape):
            d = []
            for m in (1, 2, 4):
                st = LD(h) / m
                up, dn = v.copy(), v.copy()
                up[where] += st
                dn[where] -= st
                if k in SYMMETRIC and where[0] != where[1]:
                    up[where[::-1]] += st
                    dn[where[::-1]] -= st
                d.append((loss(**{k: up}) - loss(**{k: dn})) / (2 * st))
            r1.append((4 * d[1] - d[0]) / 3)
            r2.append((4 * d[2] - d[1]) / 3)
            inst = d[0].shape[0]
        R1[k] = np.array(r1, dtype=LD).reshape(v.shape + (inst,))
        R2[k] = np.array(r2, dtype=LD).reshape(v.shape + (inst,))
    return R1, R2


def _fold(k, g):
    """what a difference of _richardson in parameter k sees of the gradient g (entry shape + (inst,))"""
    if k not in SYMMETRIC:
        return g
    gt = np.swapaxes(g, 0, 1)
    off = ~np.eye(g.shape[0], dtype=bool)[:, :, None]
    return g + np.where(off, gt, 0)


def _params(p, kw, nx, nu, N):
    z = lambda k, s: np.zeros(s, dtype=LD) if kw.get(k) is None else np.asarray(kw[k], dtype=LD)
    return dict(Q=np.asarray(p["Q"], dtype=LD), R=np.asarray(p["R"], dtype=LD), P=np.asarray(p["P"], dtype=LD),
                lb=np.asarray(p["lb"], dtype=LD), ub=np.asarray(p["ub"], dtype=LD), x_ref=z("x_ref", (nx, N)), u_ref=z("u_ref", (nu, N)))


OUT_OF = dict(Q="g_Q", R="g_R", P="g_P", lb="g_lb", ub="g_ub", x_ref="g_xref", u_ref="g_uref")


@pytest.mark.parametrize("which", FD_CASES)
def test_adjoint_against_richardson_central_differences_of_the_loop(which):
    shape, T, bsz, how = rc.CASES[which]
    c = rg.case(shape, T, bsz=bsz, **how)
    p0, kw, tape = c["p"], c["kw"], c["tape"]
    nx, nu, N = shape
    sides = rc.tape_sides(tape["U_tape"], p0["lb"], p0["ub"])
    faces = sides == 0
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
    ref = rc.reference(p, kw, c["At"], c["Bt"], X, Ut, gJT, gX, gU)
    assert ref["ok"].all()
    side = ref["side"]
    assert np.array_equal(side, sides[..., idx])
    ad = rc.adjoint(*sr.model(p), c["At"], c["Bt"], side, X, Ut, gJT, gX, gU, kw.get("x_ref"), kw.get("u_ref"), dtype=LD)
    loss = lambda **over: rc.loop_loss(p, kw, c["At"], c["Bt"], p["x0"], side, gJT, gX, gU, **over)
    R1, R2 = _richardson(loss, _params(p, kw, nx, nu, N))
    axes = dict(rc.KEYS)
    own = max(sr.rel_err(R1[k], R2[k], axes[OUT_OF[k]]).max() for k in R1)
    e = {OUT_OF[k]: sr.rel_err(_fold(k, ad[OUT_OF[k]]), R2[k], axes[OUT_OF[k]]).max() for k in R2}
    print(f"{shape} T={T}: adjoint against Richardson differences of the loop: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) +
          f"; the differences' own error {own:.2e}; kinds of step {rg.kinds(side == 0)}")
    assert own < FD_OWN
    assert max(e.values()) < FD_BAR, e
    assert all(np.any(ad[k] != 0) for k in ("g_Q", "g_R", "g_P", "g_xref", "g_uref"))
    assert np.any(ad["g_lb"] != 0) or np.any(ad["g_ub"] != 0)


def test_one_step_is_one_cost_gradient():
    """T = 1, gJT = 0: the seven outputs are those of cgrad_ref.adjoint for gu0 = gU_0 + B_true'gX_1, gVN = 0, to rounding"""
    shape, T, bsz, how = rc.CASES[3]
    assert T == 1
    c = rg.case(shape, T, bsz=bsz, **how)
    p, tape = c["p"], c["tape"]
    _, gX, gU = rg.cotangents(shape[0], shape[1], T, bsz, 5)
    side = rc.tape_sides(tape["U_tape"], p["lb"], p["ub"])
    mine = rc.adjoint(*sr.model(p), c["At"], c["Bt"], side, tape["X"], tape["U_tape"], np.zeros(bsz), gX, gU)
    w0 = gU[:, 0] + np.einsum("ik,ib->kb", c["Bt"], gX[:, 1])
    Xp = sr.model_roll(p, p["x0"], tape["U_tape"][0])
    theirs = cg.adjoint(*sr.model(p), side[0], Xp, tape["U_tape"][0], w0, np.zeros(bsz))
    e = max(sr.rel_err(mine[k], theirs[k], ax).max() for k, ax in rc.KEYS)
    print(f"one step against cgrad_ref.adjoint: {e:.2e}")
    assert e < 1e-14
    assert np.any(mine["g_R"] != 0.0)


def test_p_shapes_the_feedback_law_of_an_all_free_loop():
    """gX = gU = 0, gJT = 1, the model is the plant, every step all free: J_T depends on P only through the feedback law, and g_P
    meets a Richardson central difference of the loop, to FD_BAR times the size of the loop's own terms, for which |g_Q|_max stands
    (x0 is small here so that every step is free, and g_P is what a cancellation leaves, 1e-5 of those terms: a bar relative to
    max(|g|, 1) would pass with g_P = 0, and one relative to |g_P| would ask 1e-14 of the terms).  Measured: 1.6e-9 of |g_P|_max."""
    shape, T, inst = (2, 1, 5), 3, 4
    nx, nu, N = shape
    c0 = sr.case(shape, bsz=inst)
    p = dict(c0["p"])
    p["x0"] = np.ascontiguousarray(0.1 * c0["p"]["x0"])
    At, Bt = p["A"], p["B"]
    tape = rg.oracle_tape(p, c0["kw"], p["x0"], At, Bt, T)
    side = rc.tape_sides(tape["U_tape"], p["lb"], p["ub"])
    assert not side.any()
    gJT, gX, gU = np.ones(inst), np.zeros((nx, T + 1, inst)), np.zeros((nu, T, inst))
    # g_P is what is left of a cancellation (the law is nearly optimal for J_T): the fp64 tape's rounding would show at 1e-9 of it, so
    # the all-free loop is played again in long double and the adjoint taken there
    from oracle import exact as ex
    X, Ut = np.zeros((nx, T + 1, inst), dtype=LD), np.zeros((T, nu, N, inst), dtype=LD)
    X[:, 0] = p["x0"]
    for t in range(T):
        H, g, _ = ex.condense(N, p["A"], p["B"], p["Q"], p["R"], p["P"], X[:, t], None, None)
        Ut[t] = np.moveaxis(-ex.chol_solve(ex.cholesky(H), g).reshape(inst, N, nu), 0, -1).transpose(1, 0, 2)
        X[:, t + 1] = np.einsum("ijb,jb->ib", np.asarray(At, dtype=LD), X[:, t]) + np.einsum("ikb,kb->ib", np.asarray(Bt, dtype=LD), Ut[t][:, 0])
    assert np.abs(np.asarray(Ut, dtype=np.float64) - tape["U_tape"]).max() < 1e-14
    ad = rc.adjoint(*sr.model(p), At, Bt, side, X, Ut, gJT, gX, gU, dtype=LD)
    loss = lambda **over: rc.loop_loss(p, c0["kw"], At, Bt, p["x0"], side, gJT, gX, gU, **over)
    R1, R2 = _richardson(loss, dict(P=np.asarray(p["P"], dtype=LD)))
    own = sr.rel_err(R1["P"], R2["P"], (0, 1)).max()
    scale = np.abs(R2["P"]).max()
    nat = float(np.abs(ad["g_Q"]).max())
    e = np.abs(_fold("P", ad["g_P"]) - R2["P"]).max()
    print(f"g_P of an all-free loop: |g_P|_max {scale:.3e} beside |g_Q|_max {nat:.3e}; against the differences {e:.2e} absolute, "
          f"{e / scale:.2e} of |g_P|_max; the differences' own error {own:.2e}")
    assert scale > 0.0 and own < FD_OWN
    assert e < FD_BAR * nat
    assert e < 1e-3 * scale
