"""CPU: lqmpc_controller_set_reference in the C ABI and the binding, and the numpy prototype of the retarget kernels
(tools/proto/ctl_retarget.py: the costate recursion and both record indexings against the dense form -P^-1 (2 g_ref + P c))."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "proto"))
import ctl_retarget as proto  # noqa: E402

from lq_mpc_amd import BatchController, _lib  # noqa: E402


def test_header_declares_and_library_exports_set_reference():
    hdr = open(os.path.join(ROOT, "include", "lqmpc.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+lqmpc_controller_set_reference\s*\(\s*lqmpc_controller\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*x_ref\s*,"
                     r"\s*const\s+double\s*\*\s*u_ref\s*\)\s*;", code)
    assert " * set_reference:" in hdr                      # ... and documents it in the controller block's comment
    assert "lqmpc_controller_set_reference" in _lib.EXPORTS
    L = _lib.lib()
    assert L.lqmpc_controller_set_reference.argtypes == [ctypes.c_void_p] * 3
    a = np.zeros(4)
    assert L.lqmpc_controller_set_reference(None, None, None) == -1
    assert L.lqmpc_controller_set_reference(None, a.ctypes.data, a.ctypes.data) == -1


def test_batch_controller_has_set_reference():
    assert callable(getattr(BatchController, "set_reference"))
    # a controller that was never opened is a closed one
    c = BatchController.__new__(BatchController)
    c._c = None
    with pytest.raises(_lib.LqmpcError):
        c.set_reference()


@pytest.mark.parametrize("box", proto.BOXES, ids=str)
@pytest.mark.parametrize("shape", proto.RECORD_SHAPES, ids=str)
def test_prototype_packed_triangle(shape, box):
    e = proto.errors(shape, box)
    print(shape, box, e)
    assert max(e) <= 1e-12


@pytest.mark.parametrize("box", proto.BOXES, ids=str)
@pytest.mark.parametrize("shape", proto.WG_SHAPES, ids=str)
def test_prototype_block_image(shape, box):
    e = proto.errors(shape, box, wg=True)
    print(shape, box, e)
    assert max(e) <= 1e-12


def test_prototype_shapes_are_the_gpu_tests():
    src = open(os.path.join(ROOT, "tests", "test_gpu_controller_refs.py")).read()
    ns = {}
    exec("\n".join(ln for ln in src.splitlines() if re.match(r"(RECORDS|WG) = ", ln)), ns)
    assert ns["RECORDS"] == proto.RECORD_SHAPES and ns["WG"] == proto.WG_SHAPES
