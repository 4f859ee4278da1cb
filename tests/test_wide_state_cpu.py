"""CPU: the wide-state shapes (9 <= nx <= 16, nu <= 4, N nu <= 32) of the run-time compiled 16-lane-row kernels -- options.jit = 2.

What can be said without a GPU: which shapes lqmpc_jit_compile serves (the compile itself needs no device), that the domains of the
prepared controller's record kernels and of the on-chip bounds kernels did not move, the option's default and the struct's size, and
that the machine code compiled for the wide shapes keeps the DPP read-after-write rule (tools/dpp_check.py, as tests/test_isa_cpu.py).
lqmpc_set_options needs a handle and a handle needs a device: the round trip of jit = 2 and the refusal of 3 and -2 are in
tests/test_gpu_wide_state.py; here only the call without a handle."""
import ctypes
import glob
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dpp_check  # noqa: E402

from lq_mpc_amd import _lib  # noqa: E402

WIDE = [(9, 1, 1), (12, 2, 10), (13, 3, 5), (16, 1, 20), (16, 4, 8)]
# outside: nx over the build limit, nu > 4, n = 40 (stays with the workgroup kernel at these nx), n = 36
REFUSED = [(17, 1, 10), (9, 5, 7), (12, 2, 20), (16, 4, 9)]
ERR_BAD_ARG, ERR_UNSUPPORTED = -1, -5


def raw(fn, nx, nu, N):
    log = ctypes.create_string_buffer(4096)
    return getattr(_lib.lib(), fn)(nx, nu, N, log, len(log))


@pytest.mark.parametrize("shape", WIDE, ids=str)
def test_wide_shapes_compile_all_five_code_objects(shape):
    assert _lib.jit_compile(*shape) == 5


@pytest.mark.parametrize("shape", REFUSED, ids=str)
def test_shapes_outside_the_wide_domain_are_still_refused(shape):
    assert raw("lqmpc_jit_compile", *shape) < 0


def test_controller_and_bounds_domains_did_not_move():
    assert raw("lqmpc_jit_compile_controller", 12, 2, 10) == ERR_UNSUPPORTED
    assert raw("lqmpc_jit_compile_controller_rollout", 12, 2, 10) == ERR_UNSUPPORTED
    assert raw("lqmpc_jit_compile_controller", 16, 4, 8) == ERR_UNSUPPORTED
    # the on-chip bounds kernels stop at nx = 8 (lqmpc_bounds_chip.h): -5 before the solver's set-up went to nx = 16, and after
    assert raw("lqmpc_jit_compile_bounds", 12, 2, 10) == ERR_UNSUPPORTED
    assert raw("lqmpc_jit_compile_bounds", 9, 1, 1) == ERR_UNSUPPORTED


def test_option_default_size_and_null_handle():
    L = _lib.lib()
    o = _lib.Options()
    L.lqmpc_default_options(ctypes.byref(o))
    assert o.jit == -1 and ctypes.sizeof(_lib.Options) == 80 and o.struct_size == 80
    assert [k for k, _ in _lib.Options._fields_][-2:] == ["jit", "ctl_wg"]
    o.jit = 2
    assert L.lqmpc_set_options(None, ctypes.byref(o)) == ERR_BAD_ARG and L.lqmpc_get_options(None, ctypes.byref(o)) == ERR_BAD_ARG


# LDS image of a wavefront (R16<>::INST x 4 instances x 8 bytes, the kernel descriptor's group segment): it tells the solver kernels of
# a shape apart from everything else in the cache directory, whose file names are hashes
LDS_BYTES = {(12, 2, 10): 31488, (16, 4, 8): 64320}
READELF = os.path.join(os.path.dirname(dpp_check.OBJDUMP), "llvm-readelf")


@pytest.mark.parametrize("shape", list(LDS_BYTES), ids=str)
def test_no_dpp_hazard_in_the_wide_kernels(shape):
    assert _lib.jit_compile(*shape) == 5                  # (found in the cache directory after build(), compiled into it otherwise)
    objs = []
    for f in sorted(glob.glob(os.path.join(_lib.JIT_CACHE, "*.hsaco"))):
        notes = subprocess.run([READELF, "--notes", f], capture_output=True, text=True, check=True).stdout
        m = re.search(r"\.group_segment_fixed_size:\s*(\d+)", notes)
        if m and int(m.group(1)) == LDS_BYTES[shape]:
            objs.append(f)
    assert len(objs) >= 4, objs                           # solve, rollout, max V_N, sweep (the probe has no DPP instruction)
    n, bad = 0, []
    for o in objs:
        c, b = dpp_check.check_file(o)
        n += c
        bad += b
    assert n > 100 and not bad, "\n".join(bad[:20])
