"""CPU: the prepared controller for polytopic input constraints (lqmpc_poly_controller_*): symbols, the record's size, and every
refusal that is decided from the arguments alone -- on a fake handle and a fake controller, neither of which may be dereferenced.
All of this fails without the feature: the symbols do not exist."""
import ctypes
import os
import re

import numpy as np

from lq_mpc_amd import _lib, mpc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"lqmpc_poly_controller_create": 16, "lqmpc_poly_controller_create_dev": 16, "lqmpc_poly_controller_step": 9,
           "lqmpc_poly_controller_step_dev": 9, "lqmpc_poly_controller_rollout": 11, "lqmpc_poly_controller_rollout_dev": 11,
           "lqmpc_poly_controller_set_reference": 3, "lqmpc_poly_controller_set_model": 5, "lqmpc_poly_controller_set_model_dev": 5,
           "lqmpc_poly_controller_record_bytes": 3, "lqmpc_poly_controller_bytes": 1, "lqmpc_poly_controller_kernel": 1,
           "lqmpc_poly_controller_destroy": 1}


def test_symbols_are_declared_exported_and_have_their_arity():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lqmpc.h")).read(), flags=re.S)
    declared = dict(re.findall(r"\b(lqmpc_[a-z0-9_]+)\s*\(([^;]*)\)\s*;", hdr))
    L = _lib.lib()
    for name, arity in SYMBOLS.items():
        assert name in declared and name in _lib.EXPORTS, name
        assert len(getattr(L, name).argtypes) == arity, name
        assert declared[name].count(",") + 1 == arity, name
    assert hasattr(mpc, "PolyBatchController")


def content(nx, nu, N):
    n = N * nu
    return nx * nx + nx * nu + N * nx * nu + n * (n + 1) // 2


def test_record_bytes():
    rb = _lib.lib().lqmpc_poly_controller_record_bytes
    shapes = [(nx, nu, N) for nx in (1, 2, 4, 7, 16) for nu in (1, 2, 3, 8) for N in (1, 2, 5, 8, 10, 21, 32, 64) if N * nu <= 64]
    assert (4, 2, 10) in shapes and (16, 1, 64) in shapes and (4, 2, 32) in shapes
    for nx, nu, N in shapes:
        b = rb(nx, nu, N)
        assert b > 0 and b % 8 == 0 and b // 8 >= content(nx, nu, N), (nx, nu, N)
        assert b // 8 < content(nx, nu, N) + 16                       # rounded up, by less than the 16 doubles of a 128-byte line
        # monotone in each dimension
        if nx < 16:
            assert rb(nx + 1, nu, N) >= b
        if nu < 8 and N * (nu + 1) <= 64:
            assert rb(nx, nu + 1, N) >= b
        if N < 64 and (N + 1) * nu <= 64:
            assert rb(nx, nu, N + 1) >= b
    assert rb(4, 2, 10) == 8 * 320 and content(4, 2, 10) == 314
    for bad in ((0, 2, 10), (4, 0, 10), (4, 2, 0), (-1, 2, 10), (17, 2, 10), (4, 9, 2), (4, 1, 65), (4, 2, 33), (16, 8, 9)):
        assert rb(*bad) < 0, bad
    assert rb(4, 2, 33) == -5 and rb(0, 2, 10) == -1


def test_refusals_on_a_fake_handle_and_a_fake_controller():
    L = _lib.lib()
    z = np.zeros(16 * 16 * 4)
    q, h = z.ctypes.data, 1 << 20
    eye = np.eye(16)
    Fu = np.ascontiguousarray(np.tile(np.eye(8), (3, 1))[:17])                 # 17 non-zero rows for any nu <= 8

    def create(f, nx, nu, N, Bsz=1, handle=h, F=Fu, m=2, max_iter=0, no_out=False, **holes):
        Q, R = np.ascontiguousarray(eye[:nx, :nx]), np.ascontiguousarray(eye[:nu, :nu])
        Fm = None if F is None else np.ascontiguousarray(F[:max(m, 1), :nu])
        c = ctypes.c_void_p(12345)
        a = dict(A=q, B=q, Q=Q.ctypes.data, R=R.ctypes.data, P=Q.ctypes.data, Fu=None if Fm is None else Fm.ctypes.data, m=m,
                 xr=None, ur=None, mi=max_iter, out=None if no_out else ctypes.byref(c))
        a.update(holes)
        rc = f(handle, nx, nu, N, Bsz, *a.values())
        assert no_out or c.value is None                                       # a refused create hands back NULL
        return rc

    outside = [(nx, nu, N) for nx in range(1, 17) for nu in range(1, 9) for N in range(1, 65) if 64 < N * nu <= 128]
    assert (4, 2, 33) in outside and (16, 8, 9) in outside
    for f in (L.lqmpc_poly_controller_create, L.lqmpc_poly_controller_create_dev):
        for nx, nu, N in outside:
            assert create(f, nx, nu, N) == -5, (nx, nu, N)
            assert b"N*nu<=64" in L.lqmpc_last_error() and b"m<=16" in L.lqmpc_last_error()
        assert create(f, 4, 2, 10, m=17) == -5
        assert b"m<=16" in L.lqmpc_last_error()
        assert create(f, 4, 2, 10, m=0) == -1 and create(f, 4, 2, 10, m=-3) == -1
        assert b"m must be positive" in L.lqmpc_last_error()
        assert create(f, 4, 2, 10, F=None) == -1
        assert b"Fu" in L.lqmpc_last_error()
        bad = np.array([[10.0, 1.0], [0.0, 0.0], [0.0, -10.0]])
        assert create(f, 4, 2, 10, F=bad, m=3) == -1
        assert b"row 1 of Fu is all zero" in L.lqmpc_last_error()
        for v in (np.nan, np.inf, -np.inf):
            bad = np.array([[10.0, 1.0], [0.0, -10.0], [1.0, v]])
            assert create(f, 4, 2, 10, F=bad, m=3) == -1
            assert b"row 2 of Fu holds a non-finite entry" in L.lqmpc_last_error()
        assert create(f, 4, 2, 10, max_iter=-1) == -1
        assert b"max_iter" in L.lqmpc_last_error()
        assert create(f, 4, 2, 10, handle=None) == -1
        for hole in ("A", "B", "Q", "R", "P"):
            assert create(f, 4, 2, 10, **{hole: None}) == -1, hole
        assert create(f, 4, 2, 10, no_out=True) == -1
        assert create(f, 4, 2, 10, Bsz=0) == -1
        assert create(f, 0, 2, 10) == -1 and create(f, 4, 9, 2) == -1 and create(f, 17, 2, 2) == -1 and create(f, 4, 1, 65) == -1

    fake = 1 << 20                                                             # a controller that must not be dereferenced
    for f in (L.lqmpc_poly_controller_step, L.lqmpc_poly_controller_step_dev):
        assert f(None, q, q, q, None, None, None, None, None) == -1
        assert f(fake, None, q, q, None, None, None, None, None) == -1
        assert f(fake, q, None, q, None, None, None, None, None) == -1
    for f in (L.lqmpc_poly_controller_rollout, L.lqmpc_poly_controller_rollout_dev):
        assert f(None, 3, q, q, q, 0, q, None, None, None, None) == -1
        for hole in (2, 3, 4, 6):
            a = [fake, 3, q, q, q, 0, q, None, None, None, None]
            a[hole] = None
            assert f(*a) == -1, hole
        for T in (0, -1, 100001):
            assert f(fake, T, q, q, q, 0, q, None, None, None, None) == -1
            assert b"T must" in L.lqmpc_last_error()
    for f in (L.lqmpc_poly_controller_set_model, L.lqmpc_poly_controller_set_model_dev):
        assert f(None, 1, None, q, q) == -1
        assert f(fake, 1, None, None, q) == -1 and f(fake, 1, None, q, None) == -1
        assert f(fake, 0, None, None, None) == 0                               # count == 0 is a no-op
    assert L.lqmpc_poly_controller_set_reference(None, None, None) == -1
    assert L.lqmpc_poly_controller_destroy(None) == 0
    assert L.lqmpc_poly_controller_bytes(None) == 0 and L.lqmpc_poly_controller_kernel(None) == b"none"
    assert np.all(z == 0.0)
