"""GPU (-m gpu): the closed loop with a tape and the gradient of a loss on it -- J_T, every x_t, every u_t -- with respect to the model,
the plant and x0 of every instance (lqmpc_rollout_tape_batch, lqmpc_rollout_grad_batch: T plan calls with a plant step behind each,
then one launch of lqmpc_rollout_grad_kernel).

Problems: those of tests/sens_ref.py (case) with the plants of tests/rgrad_ref.py, Bsz = 203 (a partial last wavefront), 24 at (8,4,30);
the nine cases of rgrad_ref.CASES.  Cotangents: seeded random gJT, gX, gU, gJT exactly 0 on every third instance.
References, every case against both: (1) rgrad_ref.reference, long double, per step the dense grad_ref.reference on the certified
face of the GPU's own slice; (2) the chain of T lqmpc_model_grad_batch calls on the same tape with the recursion of the plant's costate
in numpy (kernels already trusted).

Bar: rgrad_ref.GPU_BAR = 1.0e-11 relative to max(|ref|_max, 1), per instance: 100 times the worst error of the fp64 numpy restatement of
the kernel's algebra against the same reference on the same cases (9.67e-14, g_B under references and the off-centre box;
tests/test_rgrad_cpu.py), the rule of tests/test_gpu_pgrad.py.  An instance is left out only where some step's face read bit for bit
differs from the certified one (at most 1 % of a case).
Measured on one MI355X (worst over the cases) against the long-double reference: g_A 1.9e-14, g_B 5.5e-14 (both under references and the
off-centre box), g_x0 6.1e-15, g_A_true 1.5e-15, g_B_true 1.3e-15; against the chain of model_grad_batch calls 4.0e-15 at worst; no
instance of any case was left out; the (4,2,10) tape has 25 % / 28 % / 47 % of its steps with stage 0 on bounds / on a mixed face / all
free.  T = 1 against one model_grad_batch call: 8.9e-16.  The tape forward against rollout_batch: U 4.5e-15, X 2.6e-16, J_T 2.1e-15.
The largest LDS image the limit admits, (16,8,14), is run on a made-up tape against the long-double restatement of the kernel's
algebra, with a bar formed by the same rule at that shape."""
import numpy as np
import pytest

import rgrad_ref as rg
import sens_ref as sr

pytestmark = pytest.mark.gpu

BAR = rg.GPU_BAR
KEYS = rg.KEYS
_RUN = {}


def rolled(solver, shape, T, bsz=sr.BSZ, **how):
    """the tape of a case from the GPU, its cotangents and the gradient call's outputs: computed once per case and never changed"""
    key = (shape, T, bsz, tuple(sorted(how.items())))
    if key not in _RUN:
        c = rg.case(shape, T, bsz=bsz, **how)
        p, kw = c["p"], c["kw"]
        g = solver.rollout_tape_batch(T, *sr.qa(p), p["x0"], c["At"], c["Bt"], **kw)
        cot = rg.cotangents(shape[0], shape[1], T, bsz, sum(shape))
        out = solver.rollout_grad_batch(T, *sr.qa(p), c["At"], c["Bt"], g["X"], g["U_tape"], g["status_tape"], *cot, **kw)
        for a in list(g.values()) + list(cot) + list(out.values()):
            a.setflags(write=False)
        _RUN[key] = (c, g, cot, out)
    return _RUN[key]


def chain(solver, c, g, cot):
    """reference (2): T model_grad_batch calls, newest step first, the plant's costate in numpy"""
    p, kw, T = c["p"], c["kw"], c["T"]
    gJT, gX, gU = cot
    X, Ut = g["X"], g["U_tape"]
    bsz = X.shape[2]
    Atb, Btb = rg._per_instance(c["At"], bsz, np.float64), rg._per_instance(c["Bt"], bsz, np.float64)
    lam = gX[:, T] + 2 * gJT * (p["Q"] @ X[:, T])
    acc = {k: 0.0 for k, _ in KEYS if k != "g_x0"}
    for t in range(T - 1, -1, -1):
        u = Ut[t][:, 0]
        w = gU[:, t] + 2 * gJT * (p["R"] @ u) + np.einsum("bik,ib->kb", Btb, lam)
        pt = dict(p, x0=np.ascontiguousarray(X[:, t]))
        m = solver.model_grad_batch(*sr.qa(p), Ut[t], sr.model_roll(pt, pt["x0"], Ut[t]), g["status_tape"][t], np.ascontiguousarray(w), None, **kw)
        acc["g_A"], acc["g_B"] = acc["g_A"] + m["g_A"], acc["g_B"] + m["g_B"]
        acc["g_A_true"] = acc["g_A_true"] + lam[:, None, :] * X[:, t][None, :, :]
        acc["g_B_true"] = acc["g_B_true"] + lam[:, None, :] * u[None, :, :]
        lam = gX[:, t] + 2 * gJT * (p["Q"] @ X[:, t]) + np.einsum("bij,ib->jb", Atb, lam) + m["g_x0"]
    return dict(acc, g_x0=lam)


@pytest.mark.parametrize("shape,T,bsz,how", rg.CASES, ids=str)
def test_rollout_grad_against_both_references(solver, shape, T, bsz, how):
    c, g, cot, out = rolled(solver, shape, T, bsz, **how)
    p, kw = c["p"], c["kw"]
    nx, nu, _ = shape
    tag = f"{shape} T={T} x {bsz} {how}"
    assert "rollout_grad" not in solver.last_kernel()                # (the solve kernel's name, not the post-pass's)
    assert out["g_A"].shape == out["g_A_true"].shape == (nx, nx, bsz) and out["g_B"].shape == out["g_B_true"].shape == (nx, nu, bsz)
    assert out["g_x0"].shape == (nx, bsz)
    assert np.all(g["status_tape"] == 0) and np.all(g["status"] == 0), tag
    ref = rg.reference(p, kw, c["At"], c["Bt"], g["X"], g["U_tape"], *cot)
    free = rg.tape_faces(g["U_tape"], p["lb"], p["ub"])
    same = np.all(free == ref["free"], axis=(0, 1, 2))
    mix = rg.kinds(free)
    e = {k: sr.rel_err(out[k], ref[k], ax)[same].max() for k, ax in KEYS}
    ch = chain(solver, c, g, cot)
    e2 = {k: sr.rel_err(out[k], ch[k], ax).max() for k, ax in KEYS}
    print(f"{tag}: against the long-double reference " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) +
          f"; compared {int(same.sum())} of {same.size}; against the chain of model_grad_batch " +
          " ".join(f"{k} {v:.2e}" for k, v in e2.items()) + f"; stage 0 on bounds / mixed / all free {mix[0]:.2f} / {mix[1]:.2f} / {mix[2]:.2f}")
    assert np.mean(~same) <= 0.01, (tag, np.flatnonzero(~same))
    if shape == (4, 2, 10) and not how:
        assert min(mix) >= 0.10, mix
    assert max(e.values()) < BAR, (tag, e)
    assert max(e2.values()) < BAR, (tag, e2)


@pytest.mark.parametrize("shape,T,bsz,how", [rg.CASES[1], rg.CASES[7], rg.CASES[8], rg.CASES[5]], ids=str)
def test_tape_forward(solver, shape, T, bsz, how):
    """J_T, X, U against rollout_batch on the same data; U against the tape; every slice against the plan call at its state.
    Bounds: each of the two loops solves every QP within the header's contract (|u - u*| <= 1e-10 max(|u*|, h) on these
    well-conditioned models), so their inputs differ by at most twice that per step and the difference a step inherits through the
    state adds to it: 2 T times the contract for U, the same relative to max(|X|_max, 1) for X and to J_T for J_T (J_T is not an
    optimal value: it moves in first order with u, so the u contract applies, not V_N's)."""
    c, g, _, _ = rolled(solver, shape, T, bsz, **how)
    p, kw = c["p"], c["kw"]
    r = solver.rollout_batch(T, *sr.qa(p), p["x0"], c["At"], c["Bt"], want_traj=True, **kw)
    tol = 2 * T * 1e-10
    eu = np.max(np.abs(g["U"] - r["U"]) / np.maximum(np.abs(r["U"]), c_h(p)[:, None, None]))
    ex_ = sr.rel_err(g["X"], r["X"], (0, 1)).max()
    ej = np.max(np.abs(g["J_T"] - r["J_T"]) / np.abs(r["J_T"]))
    print(f"{shape} T={T} {how}: tape forward against rollout_batch: U {eu:.2e} X {ex_:.2e} J_T {ej:.2e} (bound {tol:.1e})")
    assert np.all(r["status"] == 0) and np.all(g["status"] == 0)
    assert max(eu, ex_, ej) < tol
    assert np.array_equal(g["U"], np.ascontiguousarray(g["U_tape"][:, :, 0].transpose(1, 0, 2)))
    assert np.array_equal(g["X"][:, 0], p["x0"])
    assert np.array_equal(g["status"], g["status_tape"].max(axis=0))
    for t in range(T):
        s = solver.solve_batch(*sr.qa(p), np.ascontiguousarray(g["X"][:, t]), want_plan=True, **kw)
        assert np.array_equal(s["U_plan"], g["U_tape"][t]), t
        assert np.array_equal(s["status"], g["status_tape"][t]), t
        assert np.all(np.isfinite(g["X"][:, t + 1]))
        w = np.ones_like(g["U_tape"][t])
        pg = solver.plan_grad_batch(*sr.qa(p), g["U_tape"][t], s["X_plan"], g["status_tape"][t], w, None, None, **kw)
        assert all(np.all(np.isfinite(v)) for v in pg.values()), t
    # the plant step itself, in fp64 numpy: a sum of nx + nu products per entry
    Xn = np.stack([rg.plant_step(c["At"], c["Bt"], g["X"][:, t], g["U"][:, t]) for t in range(T)], axis=1)
    assert sr.rel_err(g["X"][:, 1:], Xn, (0, 1)).max() < 64 * 2.0 ** -52


def c_h(p):
    return 0.5 * (p["ub"] - p["lb"])


def test_one_step_equals_one_model_gradient(solver):
    """T = 1, gU and gJT only: one model_grad_batch call with gu0 = w_0, to rounding"""
    c, g, (gJT, _, gU), _ = rolled(solver, (2, 1, 1), 1)
    p = c["p"]
    out = solver.rollout_grad_batch(1, *sr.qa(p), c["At"], c["Bt"], g["X"], g["U_tape"], g["status_tape"], gJT, None, gU)
    u0 = g["U_tape"][0][:, 0]
    lam = 2 * gJT * (p["Q"] @ g["X"][:, 1])
    w0 = gU[:, 0] + 2 * gJT * (p["R"] @ u0) + c["Bt"].T @ lam
    m = solver.model_grad_batch(*sr.qa(p), g["U_tape"][0], sr.model_roll(p, p["x0"], g["U_tape"][0]), g["status_tape"][0],
                                np.ascontiguousarray(w0), None)
    gx = 2 * gJT * (p["Q"] @ p["x0"]) + c["At"].T @ lam + m["g_x0"]
    e = dict(g_A=sr.rel_err(out["g_A"], m["g_A"], (0, 1)).max(), g_B=sr.rel_err(out["g_B"], m["g_B"], (0, 1)).max(),
             g_x0=sr.rel_err(out["g_x0"], gx, 0).max())
    print("T = 1 against one model_grad_batch call: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) < BAR, e
    assert np.any(m["g_A"] != 0.0)


def test_bits_that_must_not_move(solver):
    shape, T = (4, 2, 10), 6
    c, g, (gJT, gX, gU), out = rolled(solver, shape, T)
    p = c["p"]
    a = (T, *sr.qa(p), c["At"], c["Bt"], g["X"], g["U_tape"], g["status_tape"])
    call = lambda *cot, **kw: solver.rollout_grad_batch(*a, *cot, **kw)
    # every cotangent of an instance 0.0: exact zeros there, and the others keep their bits
    quiet = np.arange(2, sr.BSZ, 5)
    jq, xq, uq = gJT.copy(), gX.copy(), gU.copy()
    jq[quiet], xq[..., quiet], uq[..., quiet] = 0.0, 0.0, 0.0
    oq = call(jq, xq, uq)
    rest = np.setdiff1d(np.arange(sr.BSZ), quiet)
    for k, _ in KEYS:
        assert np.all(oq[k][..., quiet] == 0.0), k
        assert np.array_equal(oq[k][..., rest], out[k][..., rest]), k
    # a second call; status_tape NULL = all 0; each cotangent alone against the explicit zero arrays of the others
    again, no_st = call(gJT, gX, gU), solver.rollout_grad_batch(*a[:-1], None, gJT, gX, gU)
    zj, zx, zu = np.zeros_like(gJT), np.zeros_like(gX), np.zeros_like(gU)
    pairs = [(call(gJT, None, None), call(gJT, zx, zu)), (call(None, gX, None), call(zj, gX, zu)), (call(None, None, gU), call(zj, zx, gU))]
    for k, _ in KEYS:
        assert np.array_equal(again[k], out[k]) and np.array_equal(no_st[k], out[k]), k
        for null, zero in pairs:
            assert np.array_equal(null[k], zero[k]), k
            assert not np.array_equal(null[k], out[k]), k
    # every output but one NULL: the bits of the one that is left
    for k, _ in KEYS:
        one = call(gJT, gX, gU, want=(k,))
        assert list(one) == [k] and np.array_equal(one[k], out[k]), k
    # a step whose stage-0 inputs all sit on bounds adds nothing from its QP: with the cotangent on that step's input alone and the
    # plant's costate silent (T = 1 view: gU at the last step only), the model's gradient of a saturated instance is exactly 0.0
    free = rg.tape_faces(g["U_tape"], p["lb"], p["ub"])
    sat_last = ~free[T - 1][:, 0].any(axis=0)
    assert sat_last.sum() >= 10
    ul = np.zeros_like(gU)
    ul[:, T - 1] = gU[:, T - 1]
    o = call(None, None, ul)
    for k in ("g_A", "g_B", "g_x0", "g_A_true", "g_B_true"):
        assert np.all(o[k][..., sat_last] == 0.0), k
    assert np.any(o["g_A"][..., ~sat_last] != 0.0)


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
    assert np.array_equal(np.delete(g["U_tape"], bad, axis=-1), np.delete(clean_g["U_tape"], bad, axis=-1))
    out = solver.rollout_grad_batch(T, *q, c["At"], c["Bt"], g["X"], g["U_tape"], g["status_tape"], *cot)
    for k, _ in KEYS:
        assert np.all(np.isnan(out[k][..., bad])), k
        assert np.array_equal(np.delete(out[k], bad, axis=-1), np.delete(clean[k], bad, axis=-1)), k


def test_largest_lds_image_the_limit_admits(solver):
    """rgrad_ref.largest_admitted(), (16,8,14): 163 584 of the 163 840 bytes.  The gradient call alone on a made-up tape with T = 2
    (random inputs, about a third of them on a bound, states from the plant in fp64; no solve), 7 instances.  The kernel's algebra
    does not ask whether a plan is optimal, so its long-double numpy restatement on the same inputs is the reference.  Bar, by the
    rule of the module docstring at this shape: 100 times the worst error of the fp64 restatement against the long-double one."""
    nx, nu, N = rg.largest_admitted()
    assert (nx, nu, N) == (16, 8, 14) and (nx, nu, N + 1) in rg.refused_shapes()
    T, bsz = 2, 7
    ub = np.array([0.25, 0.375, 0.3, 0.2, 0.35, 0.275, 0.225, 0.325])
    p = sr.problem(nx, nu, N, bsz, 5, -ub, ub)
    At, Bt = rg.plant((nx, nu, N), bsz)
    rng = np.random.default_rng(38)
    Ut = rng.uniform(-0.9, 0.9, (T, nu, N, bsz)) * ub[None, :, None, None]
    on_bound = rng.random(Ut.shape) < 0.3
    on_bound[1, :, 0, :2] = True                                   # two instances with stage 0 of the last step wholly on bounds
    Ut[on_bound] = (np.sign(Ut) * ub[None, :, None, None])[on_bound]
    X = np.zeros((nx, T + 1, bsz))
    X[:, 0] = p["x0"]
    for t in range(T):
        X[:, t + 1] = rg.plant_step(At, Bt, X[:, t], Ut[t][:, 0])
    cot = rg.cotangents(nx, nu, T, bsz, 38)
    free = rg.tape_faces(Ut, p["lb"], p["ub"])
    assert np.array_equal(free, ~on_bound)
    ref = rg.adjoint(*sr.model(p), At, Bt, free, X, Ut, *cot, dtype=np.longdouble)
    f64 = rg.adjoint(*sr.model(p), At, Bt, free, X, Ut, *cot)
    out = solver.rollout_grad_batch(T, *sr.qa(p), At, Bt, X, Ut, None, *cot)
    own = max(sr.rel_err(f64[k], ref[k], ax).max() for k, ax in KEYS)
    e = {k: sr.rel_err(out[k], ref[k], ax).max() for k, ax in KEYS}
    print(f"{(nx, nu, N)} T=2 x {bsz}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) + f"; the fp64 restatement {own:.2e}, bar {100 * own:.2e}")
    assert max(e.values()) < 100 * own, e
    # ... and the next horizon is refused before anything is enqueued
    from lq_mpc_amd import _lib
    with pytest.raises(_lib.LqmpcError, match="LDS"):
        p2 = sr.problem(nx, nu, N + 1, bsz, 5, -ub, ub)
        solver.rollout_grad_batch(T, *sr.qa(p2), At, Bt, X, np.zeros((T, nu, N + 1, bsz)), None, *cot)
