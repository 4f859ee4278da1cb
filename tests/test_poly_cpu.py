"""CPU: polytopic input constraints Fu u <= 1 (lqmpc_solve_poly_batch, lqmpc_rollout_poly_batch and their _dev flavours).

Tests 1-3 hold the helper tests/poly_ref.py, which the GPU tests compare against, to references that do not share its code:
  1. poly_ref.gi (the kernel's method in float64) against poly_ref.brute (every independent active set) on (2,2,2) with a full 2 x 2 B,
     40 seeded instances each of a triangle, an octagon and box_plus.  Bar 1e-12 rho; measured 2.5e-16, 3.6e-16, 2.4e-16 (rho = 0.1 /
     0.1 / 0.2).  Active rows per instance span 0..4: histograms [7 8 8 12 5], [6 5 4 11 14], [6 7 4 9 14].
  2. poly_ref.reference on a sheared box (u = T v, |v| <= 0.1) against oracle.exact.solve on the box problem in v (B T, T'R T,
     T^-1 u_ref), mapped back by T, on synth's C3 models, default and hard mix, 64 instances.  Bar 1e-12 max(|U*|, rho); measured
     3.1e-16 (default) and 9.6e-16 (hard).
  3. box_plus (the box, a row through its corner, a loose row) at C3 hard against oracle.exact.solve on the plain box: the same bar;
     measured 1.2e-16.
Tests 4 and 5 fail without the feature:
  4. the four symbols are declared, exported and have their argument lists; on a fake handle every shape of the build limits outside
     the domain (N nu > 64, m > 16) is refused with LQMPC_ERR_UNSUPPORTED and a message that names the domain, and m < 1, a NULL Fu, a
     zero row, a non-finite row, max_iter < 0, T < 1 and NULL arrays with LQMPC_ERR_BAD_ARG -- before the handle is dereferenced.
  5. LQ_MPC_Controller / LQ_MPC_Simulator construct on an octagon (ValueError before); a one-sided box still raises, box_from_Fu still
     raises on a non-box row, local_law on a polytope raises NotImplementedError."""
import os
import re

import numpy as np
import pytest

import poly_ref as pr
from lq_mpc_amd import _lib, mpc, synth
from oracle import exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLY_SYMBOLS = {"lqmpc_solve_poly_batch": 23, "lqmpc_solve_poly_batch_dev": 23, "lqmpc_rollout_poly_batch": 25,
                "lqmpc_rollout_poly_batch_dev": 25}


@pytest.mark.parametrize("name", list(pr.SMALL_POLYTOPES))
def test_gi_against_enumeration(name):
    Fu = pr.SMALL_POLYTOPES[name]
    b = pr.small_batch(40)
    H, g, _ = exact.condense(2, b["A"], b["B"], b["Q"], b["R"], b["P"], b["x0"])
    C = pr.stage_C(Fu, 2)
    worst, counts = 0.0, []
    for i in range(40):
        Hd, gd = np.asarray(H[i], dtype=np.float64), np.asarray(g[i], dtype=np.float64)
        U, lam, iters, st = pr.gi(Hd, gd, C)
        assert st == 0 and iters <= 10 * 4 + 20
        worst = max(worst, np.abs(U - pr.brute(Hd, gd, C)).max())
        counts.append(int((lam > 0).sum()))
    hist = np.bincount(counts, minlength=5)
    print(f"{name}: |gi - brute| {worst:.2e} (rho {pr.rho(Fu):g}), active rows per instance {hist}")
    assert worst <= 1e-12 * pr.rho(Fu)
    assert hist[0] and hist[1] and hist[2] and hist[3:].sum()


def _box_problem_in_v(b, T, u_ref=None):
    Tm = np.asarray(T)
    BT = np.ascontiguousarray(np.einsum("ijb,jk->ikb", b["B"], Tm))
    return BT, Tm.T @ b["R"] @ Tm, None if u_ref is None else np.linalg.solve(Tm, u_ref)


@pytest.mark.parametrize("mix", ["default", "hard"])
def test_reference_on_a_sheared_box(mix):
    b = synth.make_batch(3, 64, mix=mix)
    N, T = b["N"], pr.T_SHEAR
    Fu = pr.sheared_box(T, [0.1, 0.1])
    ref = pr.reference(N, b["A"], b["B"], b["Q"], b["R"], b["P"], Fu, b["x0"])
    BT, RT, _ = _box_problem_in_v(b, T)
    ex = exact.solve(N, b["A"], BT, b["Q"], RT, b["P"], b["lb"], b["ub"], b["x0"])
    Uex = np.einsum("kl,lib->kib", np.asarray(T, dtype=pr.LD), ex["U"])
    err = np.abs(ref["U"] - Uex).max((0, 1)) / np.maximum(np.abs(Uex).max((0, 1)), pr.rho(Fu))
    print(f"sheared box, {mix}: |U - U*| / max(|U*|, rho) {float(err.max()):.2e}; constrained {np.mean(ref['nact'] > 0):.2f}")
    assert err.max() <= 1e-12
    assert np.abs(ref["V"] - ex["V"]).max() <= 1e-12 * np.abs(ex["V"]).max()


def test_reference_on_box_plus():
    b = synth.make_batch(3, 64, mix="hard")
    N, Fu = b["N"], pr.box_plus(2, 0.1)
    ref = pr.reference(N, b["A"], b["B"], b["Q"], b["R"], b["P"], Fu, b["x0"])
    ex = exact.solve(N, b["A"], b["B"], b["Q"], b["R"], b["P"], b["lb"], b["ub"], b["x0"])
    err = np.abs(ref["U"] - ex["U"]).max((0, 1)) / np.maximum(np.abs(ex["U"]).max((0, 1)), pr.rho(Fu))
    print(f"box_plus, hard: |U - U*| / max(|U*|, rho) {float(err.max()):.2e}")
    assert err.max() <= 1e-12
    assert np.all(ref["nact"] > 0)


def test_poly_symbols_and_refusals():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lqmpc.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lqmpc_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name, arity in POLY_SYMBOLS.items():
        assert name in declared and name in _lib.EXPORTS
        assert len(getattr(L, name).argtypes) == arity
    z = np.zeros(16 * 16 * 4)
    q, h = z.ctypes.data, 1 << 20
    eye = np.eye(16)
    Fu = np.ascontiguousarray(np.tile(np.eye(8), (3, 1))[:17])                 # 17 non-zero rows for any nu <= 8

    def solve(f, nx, nu, N, Bsz=1, handle=h, F=Fu, m=2, max_iter=0, **holes):
        Q, R = np.ascontiguousarray(eye[:nx, :nx]), np.ascontiguousarray(eye[:nu, :nu])
        Fm = None if F is None else np.ascontiguousarray(F[:max(m, 1), :nu])
        a = dict(A=q, B=q, Q=Q.ctypes.data, R=R.ctypes.data, P=Q.ctypes.data, Fu=None if Fm is None else Fm.ctypes.data, m=m, x0=q,
                 xr=None, ur=None, mi=max_iter, u0=q, VN=q, Up=None, Xp=None, lam=None, st=None, it=None)
        a.update(holes)
        return f(handle, nx, nu, N, Bsz, *a.values())

    def roll(f, nx, nu, N, T=3, handle=h, F=Fu, m=2, max_iter=0, **holes):
        Q, R = np.ascontiguousarray(eye[:nx, :nx]), np.ascontiguousarray(eye[:nu, :nu])
        Fm = None if F is None else np.ascontiguousarray(F[:max(m, 1), :nu])
        a = dict(A=q, B=q, Q=Q.ctypes.data, R=R.ctypes.data, P=Q.ctypes.data, Fu=None if Fm is None else Fm.ctypes.data, m=m, x0=q,
                 At=q, Bt=q, tpi=0, xr=None, ur=None, mi=max_iter, JT=q, X=None, U=None, st=None, it=None)
        a.update(holes)
        return f(handle, nx, nu, N, 1, T, *a.values())

    outside = [(nx, nu, N) for nx in range(1, 17) for nu in range(1, 9) for N in range(1, 65) if 64 < N * nu <= 128]
    assert (4, 2, 33) in outside and (16, 8, 9) in outside
    for call, fs in ((solve, (L.lqmpc_solve_poly_batch, L.lqmpc_solve_poly_batch_dev)),
                     (roll, (L.lqmpc_rollout_poly_batch, L.lqmpc_rollout_poly_batch_dev))):
        for f in fs:
            for nx, nu, N in outside:
                assert call(f, nx, nu, N) == -5, (nx, nu, N)
                assert b"N*nu<=64" in L.lqmpc_last_error() and b"m<=16" in L.lqmpc_last_error()
            assert call(f, 4, 2, 10, m=17) == -5
            assert b"m<=16" in L.lqmpc_last_error()
            assert call(f, 4, 2, 10, m=0) == -1 and call(f, 4, 2, 10, m=-3) == -1
            assert b"m must be positive" in L.lqmpc_last_error()
            assert call(f, 4, 2, 10, F=None) == -1
            assert b"Fu" in L.lqmpc_last_error()
            bad = np.array([[10.0, 1.0], [0.0, 0.0], [0.0, -10.0]])
            assert call(f, 4, 2, 10, F=bad, m=3) == -1
            assert b"row 1 of Fu is all zero" in L.lqmpc_last_error()
            for v in (np.nan, np.inf, -np.inf):
                bad = np.array([[10.0, 1.0], [0.0, -10.0], [1.0, v]])
                assert call(f, 4, 2, 10, F=bad, m=3) == -1
                assert b"row 2 of Fu holds a non-finite entry" in L.lqmpc_last_error()
            assert call(f, 4, 2, 10, max_iter=-1) == -1
            assert b"max_iter" in L.lqmpc_last_error()
            assert call(f, 4, 2, 10, handle=None) == -1
            for hole in ("A", "B", "x0", "Q", "R", "P"):
                assert call(f, 4, 2, 10, **{hole: None}) == -1, hole
            assert call(f, 0, 2, 10) == -1 and call(f, 4, 9, 2) == -1 and call(f, 17, 2, 2) == -1 and call(f, 4, 1, 65) == -1
    for f in (L.lqmpc_solve_poly_batch, L.lqmpc_solve_poly_batch_dev):
        assert solve(f, 4, 2, 10, u0=None) == -1 and solve(f, 4, 2, 10, VN=None) == -1
        assert solve(f, 4, 2, 10, Bsz=0) == -1
    for f in (L.lqmpc_rollout_poly_batch, L.lqmpc_rollout_poly_batch_dev):
        assert roll(f, 4, 2, 10, T=0) == -1 and roll(f, 4, 2, 10, T=100001) == -1
        assert b"T must" in L.lqmpc_last_error()
        for hole in ("At", "Bt", "JT"):
            assert roll(f, 4, 2, 10, **{hole: None}) == -1, hole
    assert np.all(z == 0.0)


def test_mirror_classes_route_by_the_shape_of_Fu():
    A0, B0 = synth.base_system(3)
    Q, R = 2.0 * np.eye(4), np.eye(2)
    octagon = pr.polygon(8, 0.1, 0.2)
    c = mpc.LQ_MPC_Controller(10, A0, B0, Q, R, Q, octagon)
    s = mpc.LQ_MPC_Simulator(5, 10, A0, B0, Q, R, Q, octagon)
    assert c.poly and s.poly and c.u.value is None
    with pytest.raises(NotImplementedError, match="box-shaped"):
        c.local_law(np.zeros(4), None, None)
    box = mpc.LQ_MPC_Controller(10, A0, B0, Q, R, Q, pr.box(2, 0.1))
    assert not box.poly and np.array_equal(box.ub, [0.1, 0.1]) and np.array_equal(box.lb, [-0.1, -0.1])
    for cls, head in ((mpc.LQ_MPC_Controller, (10,)), (mpc.LQ_MPC_Simulator, (5, 10))):
        with pytest.raises(ValueError, match="both sides"):
            cls(*head, A0, B0, Q, R, Q, np.array([[10.0, 0.0], [0.0, 10.0], [0.0, -10.0]]))      # a one-sided box stays an error
    with pytest.raises(ValueError, match="exactly one non-zero"):
        mpc.box_from_Fu(octagon)
    assert mpc.is_box_Fu(pr.box(4, 0.2)) and not mpc.is_box_Fu(pr.cross(2, 0.1))
