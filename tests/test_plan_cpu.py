"""CPU: the whole-plan entry points (lqmpc_solve_plan_batch, lqmpc_controller_step_plan and their _dev flavours) are declared,
exported and refuse NULL arguments before they touch a GPU; the reference's decision variable `u` exists on the mirror class; and the
device code that writes the plan compiles in every run-time compiled variant (hiprtc needs no GPU)."""
import os
import re

import numpy as np
import pytest

from lq_mpc_amd import LQ_MPC_Controller, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_SYMBOLS = ["lqmpc_solve_plan_batch", "lqmpc_solve_plan_batch_dev", "lqmpc_controller_step_plan", "lqmpc_controller_step_plan_dev",
                "lqmpc_jit_compile_plan"]


def test_plan_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "lqmpc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(lqmpc_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in PLAN_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name


def test_plan_arguments_follow_their_plain_twins():
    """... with Uplan, Xplan between VN and status, as the header declares them"""
    hdr = open(os.path.join(ROOT, "include", "lqmpc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)

    def args(name):
        body = re.search(r"\b%s\s*\((.*?)\);" % name, hdr, flags=re.S).group(1)
        return [re.sub(r"\s+", " ", a).strip().replace(" d", " ").replace("*d", "*") for a in body.split(",")]
    for plain, plan in (("lqmpc_solve_batch", "lqmpc_solve_plan_batch"), ("lqmpc_solve_batch_dev", "lqmpc_solve_plan_batch_dev"),
                        ("lqmpc_controller_step", "lqmpc_controller_step_plan"), ("lqmpc_controller_step_dev", "lqmpc_controller_step_plan_dev")):
        a, b = args(plain), args(plan)
        assert b[:-2] == a[:-2] + ["double *Uplan", "double *Xplan"] and b[-2:] == a[-2:], (plain, a, b)
    L = _lib.lib()
    assert len(L.lqmpc_solve_plan_batch.argtypes) == len(L.lqmpc_solve_batch.argtypes) + 2
    assert len(L.lqmpc_solve_plan_batch_dev.argtypes) == len(L.lqmpc_solve_batch_dev.argtypes) + 2
    assert len(L.lqmpc_controller_step_plan.argtypes) == len(L.lqmpc_controller_step.argtypes) + 2
    assert len(L.lqmpc_controller_step_plan_dev.argtypes) == len(L.lqmpc_controller_step_dev.argtypes) + 2


def test_null_handle_and_null_controller_are_refused():
    L = _lib.lib()
    z = np.zeros(64)
    q = z.ctypes.data
    for f in (L.lqmpc_solve_plan_batch, L.lqmpc_solve_plan_batch_dev):
        assert f(None, 2, 1, 5, 1, q, q, q, q, q, q, q, q, None, None, q, q, q, q, None, None) == -1
        assert b"NULL" in L.lqmpc_last_error()
    for f in (L.lqmpc_controller_step_plan, L.lqmpc_controller_step_plan_dev):
        assert f(None, q, q, q, q, q, None, None) == -1
        assert b"NULL" in L.lqmpc_last_error()


def test_u_value_is_none_before_any_solve():
    A, B = np.array([[1.0, 0.1], [0.0, 1.0]]), np.array([[0.0], [0.1]])
    ctrl = LQ_MPC_Controller(5, A, B, np.eye(2), np.eye(1), np.eye(2), np.array([[10.0], [-10.0]]))
    assert hasattr(ctrl.u, "value") and ctrl.u.value is None


@pytest.fixture
def plan_library():
    """the library whose run-time compiled source holds the plan's stores: one that exports the plan calls"""
    L = _lib.lib()
    for name in PLAN_SYMBOLS:
        assert hasattr(L, name), f"{name}: this library has no plan write-out to compile"
    return L


@pytest.mark.parametrize("shape", [(3, 2, 6), (7, 3, 11), (12, 2, 10)], ids=str)
def test_run_time_compiled_kernels_still_compile(plan_library, shape):
    """four instances a wavefront, one instance a wavefront and the wide-state roll: solve (with the plan's stores), rollout, max V_N,
    sweep, probe"""
    assert _lib.jit_compile(*shape) == 5


def test_run_time_compiled_controller_kernels_still_compile(plan_library):
    assert _lib.jit_compile_controller(3, 2, 6) == 2


@pytest.mark.parametrize("shape,count", [((3, 2, 6), 2), ((7, 3, 11), 2), ((12, 2, 10), 1)], ids=str)
def test_run_time_compiled_plan_kernels_compile(shape, count):
    """the kernels of their own that write the plan: solve, and the controller's step where a record controller serves the shape"""
    assert _lib.jit_compile_plan(*shape) == count
    L = _lib.lib()
    assert L.lqmpc_jit_compile_plan(17, 1, 1, None, 0) == -5 and L.lqmpc_jit_compile_plan(4, 5, 4, None, 0) == -5
