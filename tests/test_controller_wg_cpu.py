"""CPU: options.ctl_wg (records of a prepared controller on the workgroup kernel's shapes) in the C ABI and its Python mirror."""
import ctypes

from lq_mpc_amd import _lib


def test_ctl_wg_is_off_by_default_and_the_struct_keeps_its_size():
    o = _lib.Options()
    _lib.lib().lqmpc_default_options(ctypes.byref(o))
    assert o.ctl_wg == 0
    assert ctypes.sizeof(_lib.Options) == 80 and o.struct_size == 80
    names = [k for k, _ in _lib.Options._fields_]
    assert names[-1] == "ctl_wg" and "reserved2" not in names         # the slot that was reserved2, not a new one
    assert _lib.Options.ctl_wg.offset == 76 and _lib.Options.jit.offset == 72
