"""GPU (-m gpu): the gradient of a loss on the closed loop -- J_T, every x_t, every u_t -- with respect to the data the batch shares: the
weights Q, R, P, the box lb, ub and the references x_ref, u_ref (lqmpc_rollout_cost_grad_batch: one launch of
lqmpc_rollout_cost_grad_kernel on the tape of lqmpc_rollout_tape_batch; with reduce a second small launch).

Problems: those of tests/rgrad_ref.py (the nine cases of CASES), Bsz = 203 (a partial last wavefront), 24 at (8,4,30).  Cotangents:
seeded random gJT, gX, gU, gJT exactly 0 on every third instance.
References, every case against both: (1) rcgrad_ref.reference, long double, per step the dense cgrad_ref.reference and
grad_ref.reference on the certified face of the GPU's own slice; (2) the chain the kernel replaces: T lqmpc_cost_grad_batch calls and T
lqmpc_model_grad_batch calls (for gx_t) on the same tape, the recursion of the plant's costate and the direct part in numpy.

Bar: rcgrad_ref.GPU_BAR = 3.0e-12 relative to max(|ref|_max, 1), per instance and output: 100 times the worst error of the fp64 numpy
restatement of the kernel's algebra against the same reference on the same cases (2.6e-14, g_lb at (2,1,1), T = 2;
tests/test_rcgrad_cpu.py), the rule of DESIGN.md section 4.11.  An instance is left out only where some step's face read bit for bit
differs from the certified one (at most 1 % of a case; the number is printed).
The figures measured on one MI355X are in DESIGN.md section 4.15."""
import math

import numpy as np
import pytest

import cgrad_ref as cg
import rcgrad_ref as rc
import rgrad_ref as rg
import sens_ref as sr

pytestmark = pytest.mark.gpu

BAR = rc.GPU_BAR
KEYS = rc.KEYS
EPS = 2.0 ** -52
_RUN = {}


def rolled(solver, shape, T, bsz=sr.BSZ, **how):
    """the tape of a case from the GPU, its cotangents and the gradient call's outputs: computed once per case and never changed"""
    key = (shape, T, bsz, tuple(sorted(how.items())))
    if key not in _RUN:
        c = rg.case(shape, T, bsz=bsz, **how)
        p, kw = c["p"], c["kw"]
        g = solver.rollout_tape_batch(T, *sr.qa(p), p["x0"], c["At"], c["Bt"], **kw)
        cot = rg.cotangents(shape[0], shape[1], T, bsz, sum(shape))
        out = solver.rollout_cost_grad_batch(T, *sr.qa(p), c["At"], c["Bt"], g["X"], g["U_tape"], g["status_tape"], *cot, **kw)
        for a in list(g.values()) + list(cot) + list(out.values()):
            a.setflags(write=False)
        _RUN[key] = (c, g, cot, out)
    return _RUN[key]


def chain(solver, c, g, cot):
    """reference (2): per step one cost_grad_batch and one model_grad_batch call, newest step first, the plant's costate in numpy"""
    p, kw, T = c["p"], c["kw"], c["T"]
    gJT, gX, gU = cot
    X, Ut = g["X"], g["U_tape"]
    bsz = X.shape[2]
    Atb, Btb = rg._per_instance(c["At"], bsz, np.float64), rg._per_instance(c["Bt"], bsz, np.float64)
    lam = gX[:, T] + 2 * gJT * (p["Q"] @ X[:, T])
    acc = {k: 0.0 for k, _ in KEYS}
    acc["g_Q"] = gJT * X[:, T][:, None, :] * X[:, T][None, :, :]
    for t in range(T - 1, -1, -1):
        u = Ut[t][:, 0]
        w = np.ascontiguousarray(gU[:, t] + 2 * gJT * (p["R"] @ u) + np.einsum("bik,ib->kb", Btb, lam))
        pt = dict(p, x0=np.ascontiguousarray(X[:, t]))
        Xp = sr.model_roll(pt, pt["x0"], Ut[t])
        cgr = solver.cost_grad_batch(*sr.qa(p), Ut[t], Xp, g["status_tape"][t], w, None, **kw)
        m = solver.model_grad_batch(*sr.qa(p), Ut[t], Xp, g["status_tape"][t], w, None, **kw)
        for k, _ in KEYS:
            acc[k] = acc[k] + cgr[k]
        acc["g_Q"] = acc["g_Q"] + gJT * X[:, t][:, None, :] * X[:, t][None, :, :]
        acc["g_R"] = acc["g_R"] + gJT * u[:, None, :] * u[None, :, :]
        lam = gX[:, t] + 2 * gJT * (p["Q"] @ X[:, t]) + np.einsum("bij,ib->jb", Atb, lam) + m["g_x0"]
    return acc


@pytest.mark.parametrize("shape,T,bsz,how", rc.CASES, ids=str)
def test_rollout_cost_grad_against_both_references(solver, shape, T, bsz, how):
    c, g, cot, out = rolled(solver, shape, T, bsz, **how)
    p, kw = c["p"], c["kw"]
    nx, nu, N = shape
    tag = f"{shape} T={T} x {bsz} {how}"
    assert "cost_grad" not in solver.last_kernel()                   # (the solve kernel's name, not the post-pass's)
    for k, s in cg.sizes(nx, nu, N).items():
        assert out[k].shape == s + (bsz,), k
    assert np.all(g["status_tape"] == 0) and np.all(g["status"] == 0), tag
    ref = rc.reference(p, kw, c["At"], c["Bt"], g["X"], g["U_tape"], *cot)
    side = rc.tape_sides(g["U_tape"], p["lb"], p["ub"])
    same = np.all(side == ref["side"], axis=(0, 1, 2))
    mix = rg.kinds(side == 0)
    e = {k: sr.rel_err(out[k], ref[k], ax)[same].max() for k, ax in KEYS}
    ch = chain(solver, c, g, cot)
    e2 = {k: sr.rel_err(out[k], ch[k], ax).max() for k, ax in KEYS}
    print(f"{tag}: against the long-double reference " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) +
          f"; compared {int(same.sum())} of {same.size}, left out {int((~same).sum())}; against the chain of cost_grad_batch and "
          "model_grad_batch " + " ".join(f"{k} {v:.2e}" for k, v in e2.items()) +
          f"; stage 0 on bounds / mixed / all free {mix[0]:.2f} / {mix[1]:.2f} / {mix[2]:.2f}")
    assert ref["ok"][:, same].all()
    assert np.mean(~same) <= rc.LEFT_OUT_CAP, (tag, np.flatnonzero(~same))
    if shape == (4, 2, 10) and not how:
        assert min(mix) >= 0.10, mix
    assert max(e.values()) < BAR, (tag, e)
    assert max(e2.values()) < BAR, (tag, e2)


@pytest.mark.parametrize("shape,T", [((2, 1, 5), 3), ((4, 2, 10), 6)], ids=str)
@pytest.mark.parametrize("bsz", [1, 3, 4, 203])
def test_reduced_mode(solver, shape, T, bsz):
    """the sum over the batch against math.fsum of the per-instance outputs: a sum of Bsz terms in any order is within
    (Bsz - 1) eps sum |g_b| of the exact one to first order, Bsz eps sum |g_b| is asserted; the same bits from
    a second call in both modes; an instance with status 2 at one step adds nothing, is counted, and is NaN per instance"""
    c, g, cot, out = rolled(solver, shape, T, bsz)
    p, kw = c["p"], c["kw"]
    a = (T, *sr.qa(p), c["At"], c["Bt"], g["X"], g["U_tape"])
    red = solver.rollout_cost_grad_batch(*a, g["status_tape"], *cot, reduce=True, **kw)
    assert red["skipped"] == 0
    for k, _ in KEYS:
        flat, r = out[k].reshape(-1, bsz), red[k].reshape(-1)
        assert red[k].shape == out[k].shape[:-1], k
        for e in range(r.size):
            assert abs(r[e] - math.fsum(flat[e])) <= bsz * EPS * math.fsum(np.abs(flat[e])), (k, e)
    red2 = solver.rollout_cost_grad_batch(*a, g["status_tape"], *cot, reduce=True, **kw)
    per2 = solver.rollout_cost_grad_batch(*a, g["status_tape"], *cot, **kw)
    for k, _ in KEYS:
        assert np.array_equal(red2[k], red[k]) and np.array_equal(per2[k], out[k]), k
    # status 2 at one step of one instance
    bad, st = bsz // 2, g["status_tape"].copy()
    st[T // 2, bad] = 2
    per_b = solver.rollout_cost_grad_batch(*a, st, *cot, **kw)
    red_b = solver.rollout_cost_grad_batch(*a, st, *cot, reduce=True, **kw)
    assert red_b["skipped"] == 1
    for k, _ in KEYS:
        assert np.all(np.isnan(per_b[k][..., bad])), k
        assert np.array_equal(np.delete(per_b[k], bad, axis=-1), np.delete(out[k], bad, axis=-1)), k
        r = red_b[k].reshape(-1)
        flat = np.delete(out[k], bad, axis=-1).reshape(r.size, bsz - 1)
        assert np.all(np.isfinite(r)), k
        for e in range(r.size):
            assert abs(r[e] - math.fsum(flat[e])) <= bsz * EPS * math.fsum(np.abs(flat[e])), (k, e)


def _made_up_tape(shape, T, bsz, seed, ub, sat0, share=0.3):
    """a tape that no solve wrote: random plans inside the box with `share` of the entries on a bound (sat0: stage 0 of every step of
    every instance wholly on bounds), the states from the plant in fp64.  The kernel's algebra does not ask whether a plan is optimal."""
    nx, nu, N = shape
    p = sr.problem(nx, nu, N, bsz, seed, -ub, ub)
    At, Bt = rg.plant(shape, bsz)
    rng = np.random.default_rng(seed)
    Ut = rng.uniform(-0.9, 0.9, (T, nu, N, bsz)) * ub[None, :, None, None]
    on_bound = rng.random(Ut.shape) < share
    if sat0:
        on_bound[:, :, 0, :] = True
    Ut[on_bound] = (np.sign(Ut) * ub[None, :, None, None])[on_bound]

    def states(U):
        X = np.zeros((nx, T + 1, bsz))
        X[:, 0] = p["x0"]
        for t in range(T):
            X[:, t + 1] = rg.plant_step(At, Bt, X[:, t], U[t][:, 0])
        return X
    return p, At, Bt, Ut, on_bound, states


def test_every_step_saturated(solver):
    """a made-up tape, T = 3, gJT NULL, every stage-0 input of every instance on a bound at every step: the wavefronts pass over the
    sweep and the rolls, gQ, gR, gP, gxref and guref are exact 0.0, and glb[k] + gub[k] is the sum of w_t[k] over the steps (the plant's
    costate from the numpy recursion).  With one instance's stage-0 input made free its wavefront cannot skip: the other instances
    keep every bit."""
    shape, T, bsz = (4, 2, 10), 3, 11
    ub = np.array([0.25, 0.375])
    p, At, Bt, Ut, on_bound, states = _made_up_tape(shape, T, bsz, 41, ub, sat0=True)
    X = states(Ut)
    _, gX, gU = rg.cotangents(shape[0], shape[1], T, bsz, 41)
    side = rc.tape_sides(Ut, p["lb"], p["ub"])
    assert np.array_equal(side != 0, on_bound) and side[:, :, 0].all()
    out = solver.rollout_cost_grad_batch(T, *sr.qa(p), At, Bt, X, Ut, None, None, gX, gU)
    for k in ("g_Q", "g_R", "g_P", "g_xref", "g_uref"):
        assert np.all(out[k] == 0.0), k
    ad = rc.adjoint(*sr.model(p), At, Bt, side, X, Ut, None, gX, gU)
    wsum = ad["w"].sum(axis=0)
    e = sr.rel_err(out["g_lb"] + out["g_ub"], wsum, 0).max()
    e_lb, e_ub = sr.rel_err(out["g_lb"], ad["g_lb"], 0).max(), sr.rel_err(out["g_ub"], ad["g_ub"], 0).max()
    print(f"every step saturated: g_lb + g_ub against the sum of w_t {e:.2e}; g_lb {e_lb:.2e}, g_ub {e_ub:.2e} against the restatement")
    assert np.any(wsum != 0.0)
    assert max(e, e_lb, e_ub) < BAR
    # instance 1 (wavefront 0) gets a free stage-0 input at step 1; its own states move, nobody else's
    U2 = Ut.copy()
    U2[1, 0, 0, 1] = 0.1 * ub[0]
    X2 = states(U2)
    others = np.setdiff1d(np.arange(bsz), [1])
    assert np.array_equal(X2[..., others], X[..., others])
    out2 = solver.rollout_cost_grad_batch(T, *sr.qa(p), At, Bt, X2, U2, None, None, gX, gU)
    for k, _ in KEYS:
        assert np.array_equal(out2[k][..., others], out[k][..., others]), k
    assert np.any(out2["g_R"][..., 1] != 0.0)
    # ... and reduced, the skip keeps its term as well
    red = solver.rollout_cost_grad_batch(T, *sr.qa(p), At, Bt, X, Ut, None, None, gX, gU, reduce=True)
    tot = (out["g_lb"] + out["g_ub"]).sum(axis=-1)
    assert np.all(np.abs(red["g_lb"] + red["g_ub"] - tot) <= 2 * bsz * EPS * np.abs(out["g_lb"] + out["g_ub"]).sum(axis=-1) + BAR)
    assert np.all(red["g_Q"] == 0.0) and np.all(red["g_uref"] == 0.0)


def test_exact_zeros_and_ignored_cotangents(solver):
    shape, T = (4, 2, 10), 6
    c, g, (gJT, gX, gU), out = rolled(solver, shape, T)
    p = c["p"]
    a = (T, *sr.qa(p), c["At"], c["Bt"], g["X"], g["U_tape"], g["status_tape"])
    call = lambda *cot, **kw: solver.rollout_cost_grad_batch(*a, *cot, **kw)
    zj, zx, zu = np.zeros_like(gJT), np.zeros_like(gX), np.zeros_like(gU)
    # every cotangent 0.0: exact zeros everywhere, in both modes
    z, zr = call(zj, zx, zu), call(zj, zx, zu, reduce=True)
    for k, _ in KEYS:
        assert np.all(z[k] == 0.0) and np.all(zr[k] == 0.0), k
    # every cotangent of some instances 0.0: exact zeros there, and the others keep their bits
    quiet = np.arange(2, sr.BSZ, 5)
    jq, xq, uq = gJT.copy(), gX.copy(), gU.copy()
    jq[quiet], xq[..., quiet], uq[..., quiet] = 0.0, 0.0, 0.0
    oq = call(jq, xq, uq)
    rest = np.setdiff1d(np.arange(sr.BSZ), quiet)
    for k, _ in KEYS:
        assert np.all(oq[k][..., quiet] == 0.0), k
        assert np.array_equal(oq[k][..., rest], out[k][..., rest]), k
    # status_tape NULL = all 0; each cotangent alone against the explicit zero arrays of the others (gJT NULL is gJT all 0.0)
    no_st = solver.rollout_cost_grad_batch(*a[:-1], None, gJT, gX, gU)
    pairs = [(call(gJT, None, None), call(gJT, zx, zu)), (call(None, gX, None), call(zj, gX, zu)), (call(None, None, gU), call(zj, zx, gU)),
             (call(None, gX, gU), call(zj, gX, gU))]
    for k, _ in KEYS:
        assert np.array_equal(no_st[k], out[k]), k
        for null, zero in pairs:
            assert np.array_equal(null[k], zero[k]), k
            assert not np.array_equal(null[k], out[k]), k
    # the cotangent of the last step's input alone, where that input sits on bounds: it reaches the bound it sits on, whole, and
    # nothing else moves (the plant's costate is silent, the adjoint plan is zero)
    side = rc.tape_sides(g["U_tape"], p["lb"], p["ub"])
    sat_last = side[T - 1][:, 0].all(axis=0)
    assert sat_last.sum() >= 10
    ul = np.zeros_like(gU)
    ul[:, T - 1] = gU[:, T - 1]
    o = call(None, None, ul)
    s0 = side[T - 1][:, 0][:, sat_last]
    assert np.array_equal(o["g_lb"][:, sat_last], np.where(s0 < 0, ul[:, T - 1][:, sat_last], 0.0))
    assert np.array_equal(o["g_ub"][:, sat_last], np.where(s0 > 0, ul[:, T - 1][:, sat_last], 0.0))
    for k in ("g_Q", "g_R", "g_P", "g_xref", "g_uref"):
        assert np.all(o[k][..., sat_last] == 0.0), k
    assert np.any(o["g_R"][..., ~sat_last] != 0.0)


def test_non_finite_model_gives_nan_and_leaves_its_neighbours_alone(solver):
    shape, T = (4, 2, 10), 6
    c, clean_g, cot, clean = rolled(solver, shape, T)
    p = c["p"]
    bad = 5                                                       # shares its wavefront with instances 4, 6 and 7
    A = p["A"].copy()
    A[1, 2, bad] = np.nan
    q = (p["N"], A, p["B"], p["Q"], p["R"], p["P"], p["lb"], p["ub"])
    g = solver.rollout_tape_batch(T, *q, p["x0"], c["At"], c["Bt"])
    assert g["status"][bad] == 2 and np.any(g["status_tape"][:, bad] == 2)
    out = solver.rollout_cost_grad_batch(T, *q, c["At"], c["Bt"], g["X"], g["U_tape"], g["status_tape"], *cot)
    # ... and with the status hidden the NaN flows through the arithmetic, and still moves no bit elsewhere
    flow = solver.rollout_cost_grad_batch(T, *q, c["At"], c["Bt"], g["X"], g["U_tape"], None, *cot)
    for k, _ in KEYS:
        assert np.all(np.isnan(out[k][..., bad])), k
        assert np.array_equal(np.delete(out[k], bad, axis=-1), np.delete(clean[k], bad, axis=-1)), k
        assert np.array_equal(np.delete(flow[k], bad, axis=-1), np.delete(clean[k], bad, axis=-1)), k
    assert np.any(np.isnan(flow["g_Q"][..., bad]))
    red = solver.rollout_cost_grad_batch(T, *q, c["At"], c["Bt"], g["X"], g["U_tape"], g["status_tape"], *cot, reduce=True)
    assert red["skipped"] == 1 and all(np.all(np.isfinite(red[k])) for k, _ in KEYS)


def test_largest_lds_image_the_limit_admits(solver):
    """rcgrad_ref.largest_admitted(), (15,4,31): 163 728 of the 163 840 bytes.  The gradient call alone on a made-up tape with T = 2
    (random inputs, about a third of them on a bound, states from the plant in fp64; no solve), 7 instances.  The kernel's algebra
    does not ask whether a plan is optimal, so its long-double numpy restatement on the same inputs is the reference.  Bar, by the
    rule of the module docstring at this shape: 100 times the worst error of the fp64 restatement against the long-double one."""
    nx, nu, N = rc.largest_admitted()
    assert (nx, nu, N) == (15, 4, 31) and (nx, nu, N + 1) in rc.refused_shapes()
    T, bsz = 2, 7
    ub = np.array([0.25, 0.375, 0.3, 0.2])
    p, At, Bt, Ut, on_bound, states = _made_up_tape((nx, nu, N), T, bsz, 38, ub, sat0=False)
    on2 = on_bound.copy()
    Ut = Ut.copy()
    Ut[1, :, 0, :2] = ub[:, None]                                  # two instances with stage 0 of the last step wholly on bounds
    on2[1, :, 0, :2] = True
    X = states(Ut)
    cot = rg.cotangents(nx, nu, T, bsz, 38)
    side = rc.tape_sides(Ut, p["lb"], p["ub"])
    assert np.array_equal(side != 0, on2)
    ref = rc.adjoint(*sr.model(p), At, Bt, side, X, Ut, *cot, dtype=np.longdouble)
    f64 = rc.adjoint(*sr.model(p), At, Bt, side, X, Ut, *cot)
    out = solver.rollout_cost_grad_batch(T, *sr.qa(p), At, Bt, X, Ut, None, *cot)
    own = max(sr.rel_err(f64[k], ref[k], ax).max() for k, ax in KEYS)
    e = {k: sr.rel_err(out[k], ref[k], ax).max() for k, ax in KEYS}
    print(f"{(nx, nu, N)} T=2 x {bsz}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) + f"; the fp64 restatement {own:.2e}, bar {100 * own:.2e}")
    assert max(e.values()) < 100 * own, e
    red = solver.rollout_cost_grad_batch(T, *sr.qa(p), At, Bt, X, Ut, None, *cot, reduce=True)
    for k, _ in KEYS:
        assert np.all(np.abs(red[k] - out[k].sum(axis=-1)) <= 2 * bsz * EPS * np.abs(out[k]).sum(axis=-1)), k
    # ... and the next horizon is refused before anything is enqueued
    from lq_mpc_amd import _lib
    with pytest.raises(_lib.LqmpcError, match="LDS"):
        p2 = sr.problem(nx, nu, N + 1, bsz, 5, -ub, ub)
        solver.rollout_cost_grad_batch(T, *sr.qa(p2), At, Bt, X, np.zeros((T, nu, N + 1, bsz)), None, *cot)
