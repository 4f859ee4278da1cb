"""CPU: the entry points that return the local feedback law and the value gradient (lqmpc_solve_sens_batch,
lqmpc_controller_step_sens and their _dev flavours) are declared, exported and refuse NULL arguments before they touch a GPU; the
package imports without torch; and the algebra lqmpc_sens_kernel implements -- one backward Riccati sweep with a free mask per stage,
one costate recursion (tests/sens_ref.py: masked_sweep, costate, fp64 numpy) -- agrees with the dense long-double reference of
oracle/exact.py (sens_ref.reference) on the faces of the oracle's own plans.

Bar of the restatement: 1e-12 relative to max(|K_ref|_max, 1) per instance, for K_plan and dV_dx alike.  Measured on these seven
cases: K_plan 5.2e-16 .. 2.5e-15, dV_dx 4.6e-16 .. 4.7e-15."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import sens_ref as sr
from lq_mpc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENS_SYMBOLS = ["lqmpc_solve_sens_batch", "lqmpc_solve_sens_batch_dev", "lqmpc_controller_step_sens", "lqmpc_controller_step_sens_dev"]
BAR = 1e-12


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lqmpc.h")).read(), flags=re.S)


def test_sens_symbols_declared_and_exported():
    declared = set(re.findall(r"\b(lqmpc_[a-z0-9_]+)\s*\(", header()))
    L = _lib.lib()
    for name in SENS_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name


def test_sens_arguments_follow_their_plan_twins():
    """... with K0, dVdx, Kplan between VN and Uplan, as the header declares them"""
    hdr = header()

    def args(name):
        """the declared arguments; a _dev flavour's device pointers (dA, du0, ddVdx, ...) under their host names"""
        body = re.search(r"\b%s\s*\((.*?)\);" % name, hdr, flags=re.S).group(1)
        out = [re.sub(r"\s+", " ", a).strip() for a in body.split(",")]
        if name.endswith("_dev"):
            out = [re.sub(r"\*d(\w+)$", r"*\1", a) for a in out]
        return out
    for plan, sens in (("lqmpc_solve_plan_batch", "lqmpc_solve_sens_batch"), ("lqmpc_solve_plan_batch_dev", "lqmpc_solve_sens_batch_dev"),
                       ("lqmpc_controller_step_plan", "lqmpc_controller_step_sens"),
                       ("lqmpc_controller_step_plan_dev", "lqmpc_controller_step_sens_dev")):
        a, b = args(plan), args(sens)
        assert b[:-7] == a[:-4] and b[-4:] == a[-4:], (plan, a, b)
        assert b[-7:-4] == ["double *K0", "double *dVdx", "double *Kplan"], (sens, b)
    L = _lib.lib()
    assert len(L.lqmpc_solve_sens_batch.argtypes) == len(L.lqmpc_solve_plan_batch.argtypes) + 3
    assert len(L.lqmpc_solve_sens_batch_dev.argtypes) == len(L.lqmpc_solve_plan_batch_dev.argtypes) + 3
    assert len(L.lqmpc_controller_step_sens.argtypes) == len(L.lqmpc_controller_step_plan.argtypes) + 3
    assert len(L.lqmpc_controller_step_sens_dev.argtypes) == len(L.lqmpc_controller_step_plan_dev.argtypes) + 3


def test_null_arguments_are_refused():
    """a NULL handle, a NULL controller, a NULL K0 or dVdx: LQMPC_ERR_BAD_ARG, and nothing is written"""
    L = _lib.lib()
    z = np.zeros(64)
    q = z.ctypes.data
    h = 1 << 20                                        # never dereferenced: the NULL checks come first
    for f in (L.lqmpc_solve_sens_batch, L.lqmpc_solve_sens_batch_dev):
        assert f(None, 2, 1, 5, 1, q, q, q, q, q, q, q, q, None, None, q, q, q, q, None, None, None, None, None) == -1
        assert b"NULL" in L.lqmpc_last_error()
        assert f(h, 2, 1, 5, 1, q, q, q, q, q, q, q, q, None, None, q, q, None, q, None, None, None, None, None) == -1
        assert f(h, 2, 1, 5, 1, q, q, q, q, q, q, q, q, None, None, q, q, q, None, None, None, None, None, None) == -1
    for f in (L.lqmpc_controller_step_sens, L.lqmpc_controller_step_sens_dev):
        assert f(None, q, q, q, q, q, None, None, None, None, None) == -1
        assert b"NULL" in L.lqmpc_last_error()
        assert f(h, q, q, q, None, q, None, None, None, None, None) == -1
        assert f(h, q, q, q, q, None, None, None, None, None, None) == -1
    assert np.all(z == 0.0)


def test_package_imports_without_torch():
    code = ("import sys; sys.modules['torch'] = None; sys.path.insert(0, %r); import lq_mpc_amd; "
            "assert hasattr(lq_mpc_amd, 'BatchController'); print('ok')" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


# (shape, instances): the table of the feature's issue
CASES = [((2, 1, 5), 203), ((4, 2, 10), 203), ((3, 3, 4), 203), ((16, 4, 8), 203), ((12, 8, 4), 203), ((4, 2, 1), 203), ((8, 4, 30), 40)]


@pytest.mark.parametrize("shape,bsz", CASES, ids=str)
def test_masked_sweep_and_costate_against_the_dense_reference(shape, bsz):
    c = sr.case(shape, bsz=bsz)
    p = c["p"]
    ref = sr.reference(p, c["kw"], p["x0"], c["U"])
    assert ref["ok"].all()                                       # the oracle's own active set is the optimal one
    U = np.asarray(ref["U"], dtype=np.float64)                   # on a bound: the bound itself, bit for bit
    free = sr.face_bits(U, p["lb"], p["ub"])
    assert np.array_equal(free, ref["free"])
    sat, fr = ~free.all(axis=(0, 1)), free.any(axis=(0, 1))
    K = sr.masked_sweep(*sr.model(p), free)
    dV = sr.costate(p["N"], p["A"], p["Q"], p["P"], sr.model_roll(p, p["x0"], U))
    eK, eV = sr.rel_err(K, ref["K_plan"], (0, 1, 2)), sr.rel_err(dV, ref["dV_dx"], 0)
    print(f"{shape} x {bsz}: K_plan {eK.max():.2e} dV_dx {eV.max():.2e}; free {np.mean(~sat):.2f} partly {np.mean(sat & fr):.2f} "
          f"saturated {np.mean(~fr):.2f}")
    assert eK.max() < BAR and eV.max() < BAR, (eK.max(), eV.max())
    assert np.all(np.moveaxis(K, 2, 0)[:, ~free] == 0.0)                            # rows on a bound are exact zeros
