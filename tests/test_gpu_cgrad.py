"""GPU (-m gpu): the gradient of a loss on (u_0, V_N) with respect to the weights Q, R, P, the references x_ref, u_ref and the box
lb, ub (lqmpc_cost_grad_batch, lqmpc_controller_cost_grad and their _dev flavours: one launch of lqmpc_cost_grad_kernel behind a plan
call, per instance or summed over the batch on chip).

Problems: those of tests/sens_ref.py (problem, case), Bsz = 203 (a partial last wavefront), the paths of tests/test_gpu_grad.py.
Cotangents: seeded random w = d loss / d u_0 and gam = d loss / d V_N, gam exactly 0 on every third instance.  Reference: long double,
dense, from oracle/exact.py (cgrad_ref.reference) on the face of the GPU plan as exact.certify reports it.

Bar: every output within 1.7e-12 of the reference relative to max(|ref|_max, 1), per instance and per output: 100 times the worst
error of the fp64 numpy restatement of the kernel's algebra against the same reference (1.68e-14, g_lb at (16,4,8): test (b) of
tests/test_cgrad_cpu.py, whose GPU_BAR is imported here), the margin covering another summation order.  Every instance is compared
unless the face the kernel reads off the plan bit for bit differs from the certified one (at most 1 % of a case).
Reduced mode: every entry within Bsz * eps * sum_b |g_b| (eps = 2^-52) of math.fsum over the per-instance outputs of the same data,
the bound of a sum of Bsz terms taken in any order.  Where stage 0 is saturated and gam is 0, g_Q, g_R, g_P, g_xref and g_uref are
exactly 0.0 and g_lb + g_ub is w bit for bit.
Measured on one MI355X (worst over the cases): g_ub 3.2e-13 at (4,2,20), g_lb 9.5e-14 (the record controller after set_model and
set_reference), the other outputs below 2.5e-14; no instance of any case was left out.  The reduced sums: at worst 4.4 % of their
bound ((8,4,30) x 24), 1 % at Bsz = 203, 7e-6 of it at Bsz = 32 770."""
import math

import numpy as np
import pytest

import cgrad_ref as cg
import grad_ref as gr
import sens_ref as sr
from lq_mpc_amd import BatchController, _lib
from test_cgrad_cpu import GPU_BAR
from test_gpu_grad import DEFAULTS, PATHS, DevArray

pytestmark = pytest.mark.gpu

BAR = GPU_BAR
KEYS = cg.KEYS
EPS = float(np.finfo(np.float64).eps)


@pytest.fixture
def opts(solver):
    """Option changes that every test undoes."""
    def set_(**kw):
        solver.set_options(**kw)
    yield set_
    solver.set_options(**DEFAULTS)


def cotangents(nu, bsz, seed):
    w, gam = gr.cotangents(nu, bsz, seed)
    gam[::3] = 0.0
    return w, gam


def check(p, kw, g, out, w, gam, tag):
    """the bar of the module docstring on one per-instance call's outputs; every figure is printed before it is asserted"""
    assert np.all(g["status"] == 0), (tag, np.flatnonzero(g["status"]))
    ref = cg.reference(p, kw, p["x0"], g["U_plan"], w, gam)
    side = cg.side_bits(g["U_plan"], p["lb"], p["ub"])
    same = np.all(side == ref["side"], axis=(0, 1))
    e = {k: sr.rel_err(out[k], ref[k], ax)[same].max() for k, ax in KEYS}
    print(f"{tag}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) + f"; compared {int(same.sum())} of {same.size}; "
          f"entries on a bound {np.mean(side != 0):.2f}, stage 0 saturated {np.mean((side[:, 0] != 0).all(axis=0)):.2f}")
    assert np.mean(~same) <= 0.01, (tag, np.flatnonzero(~same))
    assert max(e.values()) < BAR, (tag, e)
    return side


def solve_and_grad(solver, c, seed, **more):
    p, kw = c["p"], c["kw"]
    nu, bsz = p["B"].shape[1], p["x0"].shape[1]
    g = solver.solve_batch(*sr.qa(p), p["x0"], want_plan=True, **kw)
    w, gam = cotangents(nu, bsz, seed)
    out = solver.cost_grad_batch(*sr.qa(p), g["U_plan"], g["X_plan"], g["status"], w, gam, **kw, **more)
    return g, w, gam, out


def check_reduced(red, per, keep, tag):
    """every entry of the reduced outputs within Bsz eps sum |g_b| of math.fsum over the per-instance outputs of the kept instances"""
    n = int(np.sum(keep))
    worst = 0.0
    for k, _ in KEYS:
        assert red[k].shape == per[k].shape[:-1], (tag, k)
        for e in np.ndindex(red[k].shape):
            terms = per[k][e][keep]
            want, bound = math.fsum(terms), n * EPS * math.fsum(np.abs(terms))
            err = abs(red[k][e] - want)
            worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0.0 else np.inf))
            assert err <= bound, (tag, k, e, red[k][e], want, bound)
    print(f"{tag}: the reduced sums against math.fsum of {n} instances, worst error / bound {worst:.2e}")


@pytest.mark.parametrize("path", PATHS, ids=[q[0] for q in PATHS])
def test_cost_grad_behind_every_kernel_family(solver, opts, path):
    name, shape, bsz, o, family = path
    nx, nu, N = shape
    c = sr.case(shape, bsz=bsz)
    opts(**o)
    g, w, gam, out = solve_and_grad(solver, c, sum(shape))
    assert family is None or family(solver.last_kernel()), solver.last_kernel()      # (the solve kernel's name, not the post-pass's)
    for k, sh in cg.sizes(nx, nu, N).items():
        assert out[k].shape == sh + (bsz,), k
    check(c["p"], c["kw"], g, out, w, gam, name)
    if N == 1:                                                    # the sum of g_Q is empty: gam x0 x0'
        x0 = c["p"]["x0"]
        assert np.array_equal(out["g_Q"], gam * x0[:, None, :] * x0[None, :, :])
    red = solver.cost_grad_batch(*sr.qa(c["p"]), g["U_plan"], g["X_plan"], g["status"], w, gam, reduce=True)
    assert red["skipped"] == 0
    check_reduced(red, out, np.ones(bsz, dtype=bool), name)


def test_references_and_off_centre_box(solver):
    """non-zero x_ref / u_ref and a box centred in (0.3, 0.5): a bound comes out as centre +- half-width"""
    c = sr.case((4, 2, 10), refs=True, off_centre=True)
    g, w, gam, out = solve_and_grad(solver, c, 5)
    side = check(c["p"], c["kw"], g, out, w, gam, "refs, off-centre box")
    assert (side < 0).any() and (side > 0).any()
    red = solver.cost_grad_batch(*sr.qa(c["p"]), g["U_plan"], g["X_plan"], g["status"], w, gam, reduce=True, **c["kw"])
    check_reduced(red, out, np.ones(sr.BSZ, dtype=bool), "refs, off-centre box")


def test_saturated_stage_0_and_zero_gam_give_exact_zeros_and_w_on_the_bounds(solver):
    """a third of the initial states of sens_ref.problem are scaled by 3, far outside the region where stage 0 is free"""
    for shape in ((4, 2, 10), (2, 1, 5)):
        c = sr.case(shape)
        g, w, gam, out = solve_and_grad(solver, c, sum(shape))
        side = check(c["p"], c["kw"], g, out, w, gam, f"{shape} zeros")
        sat0 = (side[:, 0] != 0).all(axis=0)
        zero = sat0 & (gam == 0.0)
        assert zero.sum() >= 10, zero.sum()
        # gam = 0 everywhere: on every instance whose stage 0 is saturated the adjoint plan is zero, so the later stages' entries
        # on a bound add exact zeros and g_lb + g_ub is the stage-0 contribution alone, w
        out0 = solver.cost_grad_batch(*sr.qa(c["p"]), g["U_plan"], g["X_plan"], g["status"], w, np.zeros_like(gam))
        assert sat0.sum() >= 40
        for o_, sel in ((out, zero), (out0, sat0)):
            for k in ("g_Q", "g_R", "g_P", "g_xref", "g_uref"):
                assert np.all(o_[k][..., sel] == 0.0), k
            assert np.array_equal((o_["g_lb"] + o_["g_ub"])[:, sel], w[:, sel])
            assert np.all((o_["g_lb"][:, sel] == 0.0) | (o_["g_ub"][:, sel] == 0.0))
        for k in ("g_R", "g_xref", "g_uref"):
            assert np.any(out0[k][..., ~sat0] != 0.0), k


def test_null_cotangents_null_status_and_a_second_call(solver):
    """a NULL cotangent is the zero cotangent, status NULL is all zero, a second call gives the same bits -- in both modes"""
    c = sr.case((4, 2, 10))
    p = c["p"]
    for reduce in (False, True):
        g, w, gam, out = solve_and_grad(solver, c, 16, reduce=reduce)
        a = (*sr.qa(p), g["U_plan"], g["X_plan"], g["status"])
        call = lambda *cot, st=True: solver.cost_grad_batch(*(a if st else a[:-1] + (None,)), *cot, reduce=reduce)
        again = call(w, gam)
        no_w, zero_w = call(None, gam), call(np.zeros_like(w), gam)
        no_g, zero_g = call(w, None), call(w, np.zeros_like(gam))
        no_st = call(w, gam, st=False)
        for k, _ in KEYS:
            assert np.array_equal(out[k], again[k]), (reduce, k)
            assert np.array_equal(no_w[k], zero_w[k]) and np.array_equal(no_g[k], zero_g[k]), (reduce, k)
            assert np.array_equal(out[k], no_st[k]), (reduce, k)
            assert not np.array_equal(no_w[k], out[k]), (reduce, k)
        assert not np.array_equal(no_g["g_Q"], out["g_Q"])
        if reduce:
            assert out["skipped"] == again["skipped"] == no_st["skipped"] == 0


def test_reduced_mode_where_a_wavefront_walks_three_groups(solver):
    """(2,1,5): the reduced grid is bounded by G = cost_grad_blocks of a large batch; Bsz = 4 (2 G) + 2 gives 2 G + 1 groups of four, so
    wavefront 0 takes the groups 0, G and 2 G and the last group holds two instances.  The reference is the per-instance mode."""
    nx, nu, N = 2, 1, 5
    G = solver.cost_grad_blocks(nx, nu, N, 1 << 24)
    bsz = 4 * 2 * G + 2
    assert solver.cost_grad_blocks(nx, nu, N, bsz) == G and solver.cost_grad_blocks(nx, nu, N, bsz, reduce=False) == 2 * G + 1
    c = sr.case((nx, nu, N))
    p = sr.problem(nx, nu, N, bsz, 77, c["p"]["lb"], c["p"]["ub"])
    g = solver.solve_batch(*sr.qa(p), p["x0"], want_plan=True)
    assert np.all(g["status"] == 0)
    w, gam = cotangents(nu, bsz, 8)
    a = (*sr.qa(p), g["U_plan"], g["X_plan"], g["status"], w, gam)
    per, red, again = solver.cost_grad_batch(*a), solver.cost_grad_batch(*a, reduce=True), solver.cost_grad_batch(*a, reduce=True)
    assert red["skipped"] == 0
    check_reduced(red, per, np.ones(bsz, dtype=bool), f"(2,1,5) x {bsz}, {G} wavefronts")
    for k, _ in KEYS:
        assert np.array_equal(red[k], again[k]), k


def test_status_2_gives_nan_per_instance_and_is_left_out_of_the_sums(solver):
    c = sr.case((4, 2, 10))
    p = c["p"]
    _, w, gam, clean = solve_and_grad(solver, c, 16)
    bad = 5                                                       # shares its wavefront with instances 4, 6 and 7
    x0 = p["x0"].copy()
    x0[2, bad] = np.nan
    g = solver.solve_batch(*sr.qa(p), x0, want_plan=True)
    assert g["status"][bad] == 2 and np.count_nonzero(g["status"]) == 1
    a = (*sr.qa(p), g["U_plan"], g["X_plan"], g["status"], w, gam)
    out = solver.cost_grad_batch(*a)
    for k, _ in KEYS:
        assert np.all(np.isnan(out[k][..., bad])), k
        assert np.array_equal(np.delete(out[k], bad, axis=-1), np.delete(clean[k], bad, axis=-1)), k
    red = solver.cost_grad_batch(*a, reduce=True)
    assert red["skipped"] == 1
    keep = np.arange(sr.BSZ) != bad
    check_reduced(red, out, keep, "one instance with status 2")


def test_argument_checks(solver):
    """every refusal comes before anything is enqueued: the outputs keep their bits"""
    c = sr.case((4, 2, 10))
    p = c["p"]
    g = solver.solve_batch(*sr.qa(p), p["x0"], want_plan=True)
    w, gam = cotangents(2, sr.BSZ, 1)
    N, A, B, Q, R, P, lb, ub = sr.qa(p)
    plan = (g["U_plan"], g["X_plan"], g["status"])
    for reduce in (False, True):
        with pytest.raises(_lib.LqmpcError):
            solver.cost_grad_batch(*sr.qa(p), *plan, None, None, reduce=reduce)                          # no cotangent
        with pytest.raises(_lib.LqmpcError):
            solver.cost_grad_batch(N, A, B, Q, R, P, ub, lb, *plan, w, gam, reduce=reduce)               # lb >= ub
        with pytest.raises(_lib.LqmpcError):
            solver.cost_grad_batch(N, A, B, Q, R, P, lb + 3.0, ub + 3.0, *plan, w, gam, reduce=reduce)   # box centre over the limit
    with pytest.raises(ValueError):
        solver.cost_grad_batch(*sr.qa(p), g["U_plan"][:, :-1], g["X_plan"], g["status"], w, gam)
    with pytest.raises(ValueError):
        solver.cost_grad_batch(*sr.qa(p), *plan, w[:, :-1], gam)
    L, h = solver._L, solver._h
    outs = [np.full(sh + (sr.BSZ,), 7.0) for sh in cg.sizes(4, 2, 10).values()]
    skipped = np.full(1, 7, dtype=np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data
    base = [A, B, Q, R, P, lb, ub, None, None, g["U_plan"], g["X_plan"], g["status"], w, gam]
    tail = outs + [skipped]

    def raw(f, dims, head, reduce, tail_):
        return f(h, *dims, *[ptr(v) for v in head], reduce, *[ptr(v) for v in tail_])
    good = (4, 2, 10, sr.BSZ)
    for f in (L.lqmpc_cost_grad_batch, L.lqmpc_cost_grad_batch_dev):
        for reduce in (0, 1):
            for hole in (0, 1, 2, 3, 4, 5, 6, 9, 10):
                a = list(base)
                a[hole] = None
                assert raw(f, good, a, reduce, tail) == -1, hole
            a = list(base)
            a[12] = a[13] = None
            assert raw(f, good, a, reduce, tail) == -1                                       # both cotangents NULL
            assert raw(f, good, base, reduce, [None] * 7 + [skipped]) == -1                  # every output NULL
            for dims in ((0, 2, 10, sr.BSZ), (17, 2, 10, sr.BSZ), (4, 9, 10, sr.BSZ), (4, 2, 65, sr.BSZ), (4, 2, 10, 0)):
                assert raw(f, dims, base, reduce, tail) == -1, dims
            a = list(base)
            a[5], a[6] = ub, lb
            assert raw(f, good, a, reduce, tail) == -1                                       # lb >= ub
            a[5], a[6] = lb + 3.0, ub + 3.0
            assert raw(f, good, a, reduce, tail) == -1                                       # box centre over the limit
    solver.sync()
    assert all(np.all(o == 7.0) for o in outs) and skipped[0] == 7
    with BatchController(solver, *sr.qa(p)) as ctl:
        with pytest.raises(_lib.LqmpcError):
            ctl.cost_grad(*plan, None, None)
        with pytest.raises(ValueError):
            ctl.cost_grad(g["U_plan"], g["X_plan"][:, :-1], g["status"], w, gam)
        with pytest.raises(_lib.LqmpcError):
            ctl.cost_grad_dev(g["U_plan"], g["X_plan"], {}, dgu0=w)                            # every output NULL, before anything is read


def test_host_and_device_flavours_agree_bit_for_bit(solver):
    c = sr.case((4, 2, 10), refs=True)
    p, kw = c["p"], c["kw"]
    nx, nu, N = c["shape"]
    B_ = sr.BSZ
    d = None
    for reduce in (False, True):
        g, w, gam, out = solve_and_grad(solver, c, 3, reduce=reduce)
        if d is None:
            d = {k: DevArray(v.shape, v.dtype, init=v)
                 for k, v in dict(A=p["A"], B=p["B"], U=g["U_plan"], X=g["X_plan"], st=g["status"], w=w, gam=gam).items()}
        new = lambda: {k: DevArray(sh if reduce else sh + (B_,)) for k, sh in cg.sizes(nx, nu, N).items()}
        o, sk = new(), DevArray((1,), np.int64, init=np.full(1, -1, dtype=np.int64))
        solver.cost_grad_batch_dev(nx, nu, N, B_, d["A"], d["B"], p["Q"], p["R"], p["P"], p["lb"], p["ub"], d["U"], d["X"], o,
                                   d["st"], d["w"], d["gam"], reduce=reduce, dskipped=sk, **kw)
        solver.sync()
        for k, _ in KEYS:
            assert np.array_equal(o[k].numpy(), out[k]), (reduce, k)
        assert sk.numpy()[0] == (0 if reduce else -1)
        with BatchController(solver, *sr.qa(p), **kw) as ctl:
            o2 = new()
            some = {k: o2[k] for k in ("g_xref", "g_uref")}                                  # any output may be left out
            ctl.cost_grad_dev(d["U"], d["X"], some, d["st"], d["w"], d["gam"], reduce=reduce)
            solver.sync()
            host = ctl.cost_grad(g["U_plan"], g["X_plan"], g["status"], w, gam, reduce=reduce)
            for k in some:
                assert np.array_equal(o2[k].numpy(), out[k]), (reduce, k)
            for k, _ in KEYS:
                assert np.array_equal(host[k], out[k]), (reduce, k)
        for a in list(o.values()) + list(o2.values()) + [sk]:
            a.free()
    for a in d.values():
        a.free()


# ---------------- the controller flavour ----------------
def controller_against_solve(solver, p, kw, ca, cb, x, seed, tag):
    """a plan step on two twin controllers; cost_grad on the first equals the solve flavour on the same data bit for bit, in both
    modes, and the next plain step of the first is bit for bit that of the twin, which was never asked for a gradient"""
    ga, gb = ca.step(x, want_plan=True), cb.step(x, want_plan=True)
    assert np.array_equal(ga["U_plan"], gb["U_plan"])
    w, gam = cotangents(p["B"].shape[1], x.shape[1], seed)
    kernel = solver.last_kernel()
    plan = (ga["U_plan"], ga["X_plan"], ga["status"])
    out = ca.cost_grad(*plan, w, gam)
    red = ca.cost_grad(*plan, w, gam, reduce=True)
    assert solver.last_kernel() == kernel
    want = solver.cost_grad_batch(*sr.qa(p), *plan, w, gam, **kw)
    want_red = solver.cost_grad_batch(*sr.qa(p), *plan, w, gam, reduce=True, **kw)
    for k, _ in KEYS:
        assert np.array_equal(out[k], want[k]), (tag, k)
        assert np.array_equal(red[k], want_red[k]), (tag, k)
    assert red["skipped"] == want_red["skipped"] == 0
    check(dict(p, x0=x), kw, ga, out, w, gam, tag)
    x2 = np.ascontiguousarray(0.9 * x)
    sa, sb = ca.step(x2), cb.step(x2)
    for k in ("u_0", "V_N", "status", "iters"):
        assert np.array_equal(sa[k], sb[k]), (tag, k)


def test_record_controller_after_set_model_and_set_reference(solver):
    c = sr.case((4, 2, 10))
    p = dict(c["p"])
    with BatchController(solver, *sr.qa(p)) as ca, BatchController(solver, *sr.qa(p)) as cb:
        assert "ctl_r16" in ca.kernel
        idx = np.arange(1, sr.BSZ, 3)
        q = sr.problem(4, 2, 10, idx.size, 99, p["lb"], p["ub"])
        rng = np.random.default_rng(11)
        kw = dict(x_ref=0.05 * rng.standard_normal((4, 10)), u_ref=0.05 * rng.standard_normal((2, 10)))
        for ctl in (ca, cb):
            ctl.set_model(q["A"], q["B"], idx)
            ctl.set_reference(**kw)
        assert ca.reference_version == 1
        p["A"], p["B"] = p["A"].copy(), p["B"].copy()
        p["A"][:, :, idx], p["B"][:, :, idx] = q["A"], q["B"]
        controller_against_solve(solver, p, kw, ca, cb, p["x0"], 21, "record controller, after set_model and set_reference")


def test_workgroup_record_controller(solver, opts):
    """ctl_wg = 1: the controller keeps no copies of A and B, the post-pass reads the heads of its records"""
    c = sr.case((8, 4, 30), bsz=24)
    p = c["p"]
    opts(ctl_wg=1)
    with BatchController(solver, *sr.qa(p)) as ca, BatchController(solver, *sr.qa(p)) as cb:
        opts(**DEFAULTS)
        assert ca.kernel == "lqmpc_wg_ctl_step_kernel"
        controller_against_solve(solver, p, c["kw"], ca, cb, p["x0"], 22, "workgroup records")


def test_pass_through_controller(solver):
    c = sr.case((16, 4, 8))
    p = c["p"]
    with BatchController(solver, *sr.qa(p)) as ca, BatchController(solver, *sr.qa(p)) as cb:
        assert "ctl" not in ca.kernel
        controller_against_solve(solver, p, c["kw"], ca, cb, p["x0"], 23, "pass-through controller")
