"""ctypes binding of liblqmpc_hip.so (the C ABI in include/lqmpc.h).

The product path has no CPU fallback: if the HIP library cannot be loaded, or no GPU is
visible when a solver handle is requested, this module raises.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblqmpc_hip.so")
JIT_CACHE = os.path.join(_HERE, "_jit_cache")
CSRC = os.path.join(_HERE, "csrc")

_D = ctypes.POINTER(ctypes.c_double)
_I32 = ctypes.POINTER(ctypes.c_int32)
_H = ctypes.c_void_p

# every symbol include/lqmpc.h declares
EXPORTS = [
    "lqmpc_version", "lqmpc_last_error", "lqmpc_device_count",
    "lqmpc_create", "lqmpc_create_on_stream", "lqmpc_destroy", "lqmpc_sync",
    "lqmpc_default_options", "lqmpc_set_options", "lqmpc_get_options",
    "lqmpc_has_specialization", "lqmpc_last_kernel", "lqmpc_reserve",
    "lqmpc_solve_batch", "lqmpc_solve_batch_dev",
    "lqmpc_rollout_batch", "lqmpc_rollout_batch_dev",
    "lqmpc_max_vn_batch", "lqmpc_max_vn_batch_dev",
    "lqmpc_sweep_batch", "lqmpc_sweep_batch_dev",
    "lqmpc_bounds_batch", "lqmpc_bounds_batch_dev",
    "lqmpc_timer_begin", "lqmpc_timer_end",
    "lqmpc_jit_cache_dir", "lqmpc_jit_compile", "lqmpc_jit_compile_bounds",
    "lqmpc_controller_create", "lqmpc_controller_create_dev", "lqmpc_controller_step", "lqmpc_controller_step_dev",
    "lqmpc_controller_reset", "lqmpc_controller_set_reference",
    "lqmpc_controller_set_model", "lqmpc_controller_set_model_dev", "lqmpc_controller_bytes", "lqmpc_controller_kernel", "lqmpc_controller_destroy",
    "lqmpc_jit_compile_controller",
    "lqmpc_controller_rollout", "lqmpc_controller_rollout_dev", "lqmpc_jit_compile_controller_rollout",
    "lqmpc_solve_plan_batch", "lqmpc_solve_plan_batch_dev", "lqmpc_controller_step_plan", "lqmpc_controller_step_plan_dev",
    "lqmpc_jit_compile_plan",
    "lqmpc_solve_sens_batch", "lqmpc_solve_sens_batch_dev", "lqmpc_controller_step_sens", "lqmpc_controller_step_sens_dev",
    "lqmpc_model_grad_batch", "lqmpc_model_grad_batch_dev", "lqmpc_controller_model_grad", "lqmpc_controller_model_grad_dev",
    "lqmpc_cost_grad_batch", "lqmpc_cost_grad_batch_dev", "lqmpc_controller_cost_grad", "lqmpc_controller_cost_grad_dev",
    "lqmpc_cost_grad_blocks",
    "lqmpc_plan_grad_batch", "lqmpc_plan_grad_batch_dev", "lqmpc_controller_plan_grad", "lqmpc_controller_plan_grad_dev",
    "lqmpc_rollout_tape_batch", "lqmpc_rollout_tape_batch_dev", "lqmpc_rollout_grad_batch", "lqmpc_rollout_grad_batch_dev",
    "lqmpc_rollout_cost_grad_batch", "lqmpc_rollout_cost_grad_batch_dev",
    "lqmpc_solve_poly_batch", "lqmpc_solve_poly_batch_dev", "lqmpc_rollout_poly_batch", "lqmpc_rollout_poly_batch_dev",
    "lqmpc_poly_controller_create", "lqmpc_poly_controller_create_dev", "lqmpc_poly_controller_step", "lqmpc_poly_controller_step_dev",
    "lqmpc_poly_controller_rollout", "lqmpc_poly_controller_rollout_dev", "lqmpc_poly_controller_set_reference",
    "lqmpc_poly_controller_set_model", "lqmpc_poly_controller_set_model_dev", "lqmpc_poly_controller_record_bytes",
    "lqmpc_poly_controller_bytes", "lqmpc_poly_controller_kernel", "lqmpc_poly_controller_destroy",
]


class Options(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("eps", ctypes.c_double), ("tau", ctypes.c_double), ("z0_scale", ctypes.c_double),
                ("max_iter", ctypes.c_int32), ("polish", ctypes.c_int32), ("kernel", ctypes.c_int32),
                ("presolve", ctypes.c_int32), ("order", ctypes.c_int32), ("warm_start", ctypes.c_int32),
                ("layout", ctypes.c_int32), ("r16_maxit", ctypes.c_int32), ("r16_build", ctypes.c_int32),
                ("nwide", ctypes.c_int32), ("jit", ctypes.c_int32), ("ctl_wg", ctypes.c_int32)]


KERNEL_AUTO, KERNEL_GENERIC, KERNEL_SPECIALIZED, KERNEL_WORKGROUP = 0, 1, 2, 3


class LqmpcError(RuntimeError):
    pass


def build(force=False):
    """hipcc build of the shared library for gfx950 (cross-compiles without a GPU)."""
    args = ["make", "-C", CSRC, "-j4"]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        build()
    L = ctypes.CDLL(LIB_PATH)
    L.lqmpc_version.restype = ctypes.c_char_p
    L.lqmpc_last_error.restype = ctypes.c_char_p
    L.lqmpc_last_kernel.restype = ctypes.c_char_p
    L.lqmpc_last_kernel.argtypes = [_H]
    L.lqmpc_device_count.restype = ctypes.c_int
    L.lqmpc_create.argtypes = [ctypes.c_int, ctypes.POINTER(_H)]
    L.lqmpc_create_on_stream.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(_H)]
    L.lqmpc_destroy.argtypes = [_H]
    L.lqmpc_sync.argtypes = [_H]
    L.lqmpc_default_options.argtypes = [ctypes.POINTER(Options)]
    L.lqmpc_default_options.restype = None
    L.lqmpc_set_options.argtypes = [_H, ctypes.POINTER(Options)]
    L.lqmpc_get_options.argtypes = [_H, ctypes.POINTER(Options)]
    L.lqmpc_has_specialization.argtypes = [ctypes.c_int] * 3
    L.lqmpc_reserve.argtypes = [_H, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int]
    P = ctypes.c_void_p   # data pointers: host (numpy) or device (raw address), as void*
    dims = [_H, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64]
    solve_args = dims + [P] * 14
    L.lqmpc_solve_batch.argtypes = solve_args
    L.lqmpc_solve_batch_dev.argtypes = solve_args
    L.lqmpc_solve_plan_batch.argtypes = solve_args + [P] * 2
    L.lqmpc_solve_plan_batch_dev.argtypes = solve_args + [P] * 2
    L.lqmpc_solve_sens_batch.argtypes = solve_args + [P] * 5
    L.lqmpc_solve_sens_batch_dev.argtypes = solve_args + [P] * 5
    L.lqmpc_model_grad_batch.argtypes = dims + [P] * 17
    L.lqmpc_model_grad_batch_dev.argtypes = dims + [P] * 17
    L.lqmpc_cost_grad_batch.argtypes = dims + [P] * 14 + [ctypes.c_int] + [P] * 8
    L.lqmpc_cost_grad_batch_dev.argtypes = dims + [P] * 14 + [ctypes.c_int] + [P] * 8
    L.lqmpc_cost_grad_blocks.argtypes = [ctypes.c_int] * 3 + [ctypes.c_int64, ctypes.c_int]
    L.lqmpc_cost_grad_blocks.restype = ctypes.c_int64
    L.lqmpc_plan_grad_batch.argtypes = dims + [P] * 18
    L.lqmpc_plan_grad_batch_dev.argtypes = dims + [P] * 18
    roll_args = dims + [ctypes.c_int] + [P] * 10 + [ctypes.c_int] + [P] * 7
    L.lqmpc_rollout_batch.argtypes = roll_args
    L.lqmpc_rollout_batch_dev.argtypes = roll_args
    L.lqmpc_rollout_tape_batch.argtypes = roll_args + [P] * 2
    L.lqmpc_rollout_tape_batch_dev.argtypes = roll_args + [P] * 2
    rgrad_args = dims + [ctypes.c_int] + [P] * 9 + [ctypes.c_int] + [P] * 13
    L.lqmpc_rollout_grad_batch.argtypes = rgrad_args
    L.lqmpc_rollout_grad_batch_dev.argtypes = rgrad_args
    rcgrad_args = dims + [ctypes.c_int] + [P] * 9 + [ctypes.c_int] + [P] * 8 + [ctypes.c_int] + [P] * 8
    L.lqmpc_rollout_cost_grad_batch.argtypes = rcgrad_args
    L.lqmpc_rollout_cost_grad_batch_dev.argtypes = rcgrad_args
    poly_args = dims + [P] * 6 + [ctypes.c_int] + [P] * 3 + [ctypes.c_int] + [P] * 7
    L.lqmpc_solve_poly_batch.argtypes = poly_args
    L.lqmpc_solve_poly_batch_dev.argtypes = poly_args
    poly_roll_args = dims + [ctypes.c_int] + [P] * 6 + [ctypes.c_int] + [P] * 3 + [ctypes.c_int] + [P] * 2 + [ctypes.c_int] + [P] * 5
    L.lqmpc_rollout_poly_batch.argtypes = poly_roll_args
    L.lqmpc_rollout_poly_batch_dev.argtypes = poly_roll_args
    mv_args = dims + [ctypes.c_int] + [P] * 13
    L.lqmpc_max_vn_batch.argtypes = mv_args
    L.lqmpc_max_vn_batch_dev.argtypes = mv_args
    sweep_args = dims + [ctypes.c_int, ctypes.c_int] + [P] * 11 + [ctypes.c_int] + [P] * 6
    L.lqmpc_sweep_batch.argtypes = sweep_args
    L.lqmpc_sweep_batch_dev.argtypes = sweep_args
    bounds_args = dims + [P] * 11 + [ctypes.c_double] + [P] * 9
    L.lqmpc_bounds_batch.argtypes = bounds_args
    L.lqmpc_bounds_batch_dev.argtypes = bounds_args
    L.lqmpc_timer_begin.argtypes = [_H]
    L.lqmpc_timer_end.argtypes = [_H, ctypes.POINTER(ctypes.c_float)]
    L.lqmpc_jit_cache_dir.argtypes = [ctypes.c_char_p]
    L.lqmpc_jit_compile.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    L.lqmpc_jit_compile_bounds.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    L.lqmpc_jit_compile_controller.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    L.lqmpc_jit_compile_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    ctl_create_args = dims + [P] * 9 + [ctypes.POINTER(_H)]
    L.lqmpc_controller_create.argtypes = ctl_create_args
    L.lqmpc_controller_create_dev.argtypes = ctl_create_args
    L.lqmpc_controller_step.argtypes = [_H] + [P] * 5
    L.lqmpc_controller_step_dev.argtypes = [_H] + [P] * 5
    L.lqmpc_controller_step_plan.argtypes = [_H] + [P] * 7
    L.lqmpc_controller_step_plan_dev.argtypes = [_H] + [P] * 7
    L.lqmpc_controller_step_sens.argtypes = [_H] + [P] * 10
    L.lqmpc_controller_step_sens_dev.argtypes = [_H] + [P] * 10
    L.lqmpc_controller_model_grad.argtypes = [_H] + [P] * 8
    L.lqmpc_controller_model_grad_dev.argtypes = [_H] + [P] * 8
    L.lqmpc_controller_cost_grad.argtypes = [_H] + [P] * 5 + [ctypes.c_int] + [P] * 8
    L.lqmpc_controller_cost_grad_dev.argtypes = [_H] + [P] * 5 + [ctypes.c_int] + [P] * 8
    L.lqmpc_controller_plan_grad.argtypes = [_H] + [P] * 9
    L.lqmpc_controller_plan_grad_dev.argtypes = [_H] + [P] * 9
    ctl_roll_args = [_H, ctypes.c_int, P, P, P, ctypes.c_int] + [P] * 5
    L.lqmpc_controller_rollout.argtypes = ctl_roll_args
    L.lqmpc_controller_rollout_dev.argtypes = ctl_roll_args
    L.lqmpc_jit_compile_controller_rollout.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    L.lqmpc_controller_reset.argtypes = [_H]
    L.lqmpc_controller_set_reference.argtypes = [_H, P, P]
    L.lqmpc_controller_set_model.argtypes = [_H, ctypes.c_int64, P, P, P]
    L.lqmpc_controller_set_model_dev.argtypes = [_H, ctypes.c_int64, P, P, P]
    L.lqmpc_controller_bytes.argtypes = [_H]
    L.lqmpc_controller_bytes.restype = ctypes.c_int64
    L.lqmpc_controller_kernel.argtypes = [_H]
    L.lqmpc_controller_kernel.restype = ctypes.c_char_p
    L.lqmpc_controller_destroy.argtypes = [_H]
    pctl_create_args = dims + [P] * 6 + [ctypes.c_int] + [P] * 2 + [ctypes.c_int, ctypes.POINTER(_H)]
    L.lqmpc_poly_controller_create.argtypes = pctl_create_args
    L.lqmpc_poly_controller_create_dev.argtypes = pctl_create_args
    L.lqmpc_poly_controller_step.argtypes = [_H] + [P] * 8
    L.lqmpc_poly_controller_step_dev.argtypes = [_H] + [P] * 8
    L.lqmpc_poly_controller_rollout.argtypes = ctl_roll_args
    L.lqmpc_poly_controller_rollout_dev.argtypes = ctl_roll_args
    L.lqmpc_poly_controller_set_reference.argtypes = [_H, P, P]
    L.lqmpc_poly_controller_set_model.argtypes = [_H, ctypes.c_int64, P, P, P]
    L.lqmpc_poly_controller_set_model_dev.argtypes = [_H, ctypes.c_int64, P, P, P]
    L.lqmpc_poly_controller_record_bytes.argtypes = [ctypes.c_int] * 3
    L.lqmpc_poly_controller_record_bytes.restype = ctypes.c_int64
    L.lqmpc_poly_controller_bytes.argtypes = [_H]
    L.lqmpc_poly_controller_bytes.restype = ctypes.c_int64
    L.lqmpc_poly_controller_kernel.argtypes = [_H]
    L.lqmpc_poly_controller_kernel.restype = ctypes.c_char_p
    L.lqmpc_poly_controller_destroy.argtypes = [_H]
    # code objects of run-time compiled shapes are kept next to the library (falls back to memory only if not writable)
    L.lqmpc_jit_cache_dir(JIT_CACHE.encode())
    _lib = L
    return L


def jit_compile(nx, nu, N):
    """Compile (or find in the cache) every kernel of one shape now; needs no GPU.  Returns the number of code objects."""
    log = ctypes.create_string_buffer(4096)
    rc = lib().lqmpc_jit_compile(int(nx), int(nu), int(N), log, len(log))
    if rc < 0:
        raise LqmpcError(f"lqmpc_jit_compile({nx},{nu},{N}) -> {rc}: {log.value.decode(errors='replace')}")
    return rc


def jit_compile_bounds(nx, nu, N):
    """The two on-chip kernels of bounds_batch for one shape, compiled (or found in the cache) now; needs no GPU."""
    log = ctypes.create_string_buffer(4096)
    rc = lib().lqmpc_jit_compile_bounds(int(nx), int(nu), int(N), log, len(log))
    if rc < 0:
        raise LqmpcError(f"lqmpc_jit_compile_bounds({nx},{nu},{N}) -> {rc}: {log.value.decode(errors='replace')}")
    return rc


def jit_compile_controller(nx, nu, N):
    """The factor and step kernels of a prepared controller for one shape, compiled (or found in the cache) now; needs no GPU."""
    log = ctypes.create_string_buffer(4096)
    rc = lib().lqmpc_jit_compile_controller(int(nx), int(nu), int(N), log, len(log))
    if rc < 0:
        raise LqmpcError(f"lqmpc_jit_compile_controller({nx},{nu},{N}) -> {rc}: {log.value.decode(errors='replace')}")
    return rc


def jit_compile_plan(nx, nu, N):
    """The kernels that write the whole plan (solve; step where a record controller serves the shape), compiled (or found in the
    cache) now; needs no GPU.  Returns their number."""
    log = ctypes.create_string_buffer(4096)
    rc = lib().lqmpc_jit_compile_plan(int(nx), int(nu), int(N), log, len(log))
    if rc < 0:
        raise LqmpcError(f"lqmpc_jit_compile_plan({nx},{nu},{N}) -> {rc}: {log.value.decode(errors='replace')}")
    return rc


def jit_compile_controller_rollout(nx, nu, N):
    """The rollout kernel of a prepared controller for one shape, compiled (or found in the cache) now; needs no GPU."""
    log = ctypes.create_string_buffer(4096)
    rc = lib().lqmpc_jit_compile_controller_rollout(int(nx), int(nu), int(N), log, len(log))
    if rc < 0:
        raise LqmpcError(f"lqmpc_jit_compile_controller_rollout({nx},{nu},{N}) -> {rc}: {log.value.decode(errors='replace')}")
    return rc


def check(rc):
    if rc != 0:
        raise LqmpcError(f"lqmpc error {rc}: {lib().lqmpc_last_error().decode()}")
