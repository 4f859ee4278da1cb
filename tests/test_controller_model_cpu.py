"""CPU: lqmpc_controller_set_model / _dev in the C ABI and the binding, and the argument checks BatchController.set_model makes on the
host before the library is called (lq_mpc_amd.mpc._model_update_args)."""
import ctypes
import os
import re

import numpy as np
import pytest

from lq_mpc_amd import BatchController, _lib
from lq_mpc_amd.mpc import _model_update_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, NU, BSZ = 4, 2, 203


def test_header_declares_and_library_exports_set_model():
    hdr = open(os.path.join(ROOT, "include", "lqmpc.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, (i, a, b) in (("lqmpc_controller_set_model", ("idx", "A", "B")), ("lqmpc_controller_set_model_dev", ("didx", "dA", "dB"))):
        assert re.search(rf"\bint\s+{name}\s*\(\s*lqmpc_controller\s*\*\s*\w+\s*,\s*int64_t\s+count\s*,\s*const\s+int32_t\s*\*\s*{i}\s*,"
                         rf"\s*const\s+double\s*\*\s*{a}\s*,\s*const\s+double\s*\*\s*{b}\s*\)\s*;", code), name
        assert name in _lib.EXPORTS
    assert " * set_model:" in hdr                           # ... and documents it in the controller block's comment
    L = _lib.lib()
    args = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert L.lqmpc_controller_set_model.argtypes == args and L.lqmpc_controller_set_model_dev.argtypes == args
    assert L.lqmpc_controller_set_model(None, 0, None, None, None) == -1
    assert L.lqmpc_controller_set_model_dev(None, 0, None, None, None) == -1
    a, i = np.zeros(16), np.zeros(1, dtype=np.int32)
    assert L.lqmpc_controller_set_model(None, 1, i.ctypes.data, a.ctypes.data, a.ctypes.data) == -1


def test_options_struct_did_not_grow():
    assert ctypes.sizeof(_lib.Options) == 80


def test_batch_controller_has_set_model():
    assert callable(getattr(BatchController, "set_model"))
    # a controller that was never opened is a closed one
    c = BatchController.__new__(BatchController)
    c._c = None
    with pytest.raises(_lib.LqmpcError):
        c.set_model(np.zeros((NX, NX, 1)), np.zeros((NX, NU, 1)), [0])


def update(m, nx=NX, nu=NU):
    return np.zeros((nx, nx, m)), np.zeros((nx, nu, m))


@pytest.mark.parametrize("A, B, idx", [
    (np.zeros((NX, NX + 1, 3)), np.zeros((NX, NU, 3)), [0, 1, 2]),        # A is not nx x nx
    (np.zeros((NX, NX)), np.zeros((NX, NU, 3)), [0, 1, 2]),               # A has no instance axis
    (np.zeros((NX, NX, 3)), np.zeros((NX, NU + 1, 3)), [0, 1, 2]),        # B is not nx x nu
    (np.zeros((NX, NX, 3)), np.zeros((NX, NU, 4)), [0, 1, 2]),            # B holds another number of instances
    (*update(3), [0, 1]),                                                 # m != len(idx)
    (*update(3), [0, 1, 2, 3]),
    (*update(BSZ - 1), None),                                             # idx=None with m != Bsz
    (*update(3), [0, -1, 2]),                                             # an index -1
    (*update(3), [0, BSZ, 2]),                                            # an index Bsz
    (*update(3), [5, 7, 5]),                                              # a duplicate
    (*update(3), [0.0, 1.0, 2.0]),                                        # a float idx
    (*update(3), np.array([0.0, 1.0, 2.0])),
    (*update(4), np.array([[0, 1], [2, 3]])),                             # not one-dimensional
], ids=str)
def test_bad_updates_raise_before_the_library_is_called(A, B, idx):
    with pytest.raises(ValueError):
        _model_update_args(NX, NU, BSZ, A, B, idx)


def test_good_updates_pass():
    A, B, idx, m = _model_update_args(NX, NU, BSZ, *update(0), [])        # an empty update
    assert m == 0 and A.shape == (NX, NX, 0) and B.shape == (NX, NU, 0) and idx.size == 0 and idx.dtype == np.int32
    assert _model_update_args(NX, NU, BSZ, *update(0), np.zeros(0, dtype=np.int64))[3] == 0
    A, B, idx, m = _model_update_args(NX, NU, BSZ, *update(BSZ), None)    # every model
    assert m == BSZ and idx is None
    rng = np.random.default_rng(0)
    want = rng.permutation(BSZ)[:37]
    A0 = np.asfortranarray(rng.standard_normal((NX, NX, 37)))             # any memory order and any integer type come out as the ABI's
    A, B, idx, m = _model_update_args(NX, NU, BSZ, A0, np.zeros((NX, NU, 37), dtype=np.float32), want.astype(np.uint8))
    assert m == 37 and idx.dtype == np.int32 and np.array_equal(idx, want) and idx.flags.c_contiguous
    assert A.flags.c_contiguous and B.flags.c_contiguous and B.dtype == np.float64 and np.array_equal(A, A0)
    assert _model_update_args(NX, NU, BSZ, *update(2), (0, BSZ - 1))[2].tolist() == [0, BSZ - 1]
