"""Dev tool: what the whole plan costs on top of a one-shot solve and of a controller's step; prints one JSON line.

    python tools/plan_time.py [--configs 3 4 5] [--controller 3] [--calls 10] [--rounds 5] [--out FILE]
    python tools/plan_time.py --plain-only --tree OTHER_TREE      (a built tree without the plan calls, e.g. the parent commit: variant (a) alone)

Per config (default mix, the bench's batch size: C3 x 65 536, C4 x 262 144, C5 x 32 768), device-resident inputs and outputs, the
handle's own timer (lqmpc_timer_*) around `calls` calls, three warm-up rounds, the variants measured alternately in every round:
  (a) lqmpc_solve_batch_dev,
  (b) lqmpc_solve_plan_batch_dev with Xplan = NULL,
  (c) lqmpc_solve_plan_batch_dev with both outputs;
and for --controller the same three of lqmpc_controller_step_dev / lqmpc_controller_step_plan_dev (warm: the same state again).
Reported per variant: every round's time per call, their median, min and max, and the bytes a call writes (u0, V_N, status, iters;
+ N nu doubles per instance for Uplan; + (N + 1) nx for Xplan).  Comparing two trees: run this tool once per tree, alternately, in one
job on one GPU, and compare (a) of the one with (a) of the other against the spread (max - min over the rounds and runs) of either."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Dev:
    """An array in HBM through the HIP runtime the library has loaded (no other framework on the GPU: nothing else to warm up)."""
    hip = None

    def __init__(self, shape, dtype=np.float64, init=None):
        if Dev.hip is None:
            path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
            Dev.hip = ctypes.CDLL(path)
            Dev.hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
            Dev.hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
            Dev.hip.hipFree.argtypes = [ctypes.c_void_p]
        self.shape, self.dtype = tuple(np.atleast_1d(shape)), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self._p = ctypes.c_void_p()
        assert Dev.hip.hipMalloc(ctypes.byref(self._p), max(self.nbytes, 8)) == 0
        if init is not None:
            src = np.ascontiguousarray(init, dtype=self.dtype)
            assert src.shape == self.shape and Dev.hip.hipMemcpy(self._p, src.ctypes.data, self.nbytes, 1) == 0

    def data_ptr(self):
        return self._p.value

    def is_contiguous(self):
        return True

    def numpy(self):
        out = np.empty(self.shape, dtype=self.dtype)
        assert Dev.hip.hipMemcpy(out.ctypes.data, self._p, self.nbytes, 2) == 0
        return out

    def free(self):
        if self._p.value:
            Dev.hip.hipFree(self._p)
            self._p = ctypes.c_void_p()


def measure(s, variants, calls, rounds):
    """{name: [ms per call, one per round]}: the variants alternate inside every round"""
    def once(go):
        s.timer_begin()
        for _ in range(calls):
            go()
        return s.timer_end() / calls
    for _ in range(3):
        for go in variants.values():
            once(go)
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, go in variants.items():
            t[k].append(once(go))
    return t


def summary(ts, nbytes):
    return {k: {"ms": [round(x, 5) for x in v], "median_ms": round(float(np.median(v)), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5),
                "bytes_written_per_call": nbytes[k]} for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="*", default=[3, 4, 5])
    ap.add_argument("--controller", type=int, nargs="*", default=[3])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bsz", type=int, default=None, help="instances (default: the bench's batch size of each config)")
    ap.add_argument("--plain-only", action="store_true", help="variant (a) alone: for a tree without the plan calls")
    ap.add_argument("--tree", default=ROOT, help="the built tree whose lq_mpc_amd is measured (default: this one)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from lq_mpc_amd import BatchController, BatchSolver, synth
    s = BatchSolver(0)
    out = {"tool": "plan_time", "tree": os.path.relpath(os.path.abspath(a.tree), ROOT), "calls": a.calls, "rounds": a.rounds, "solve": {}, "step": {}}
    for cfg in sorted(set(a.configs) | set(a.controller)):
        b = synth.make_batch(cfg, Bsz=a.bsz)
        nx, nu, Bsz = b["B"].shape
        N = b["N"]
        w = (b["Q"], b["R"], b["P"], b["lb"], b["ub"])
        dA, dB, dx = Dev(b["A"].shape, init=b["A"]), Dev(b["B"].shape, init=b["B"]), Dev(b["x0"].shape, init=b["x0"])
        du, dv, dU, dX = Dev((nu, Bsz)), Dev(Bsz), Dev((nu, N, Bsz)), Dev((nx, N + 1, Bsz))
        dst, dit = Dev(Bsz, np.int32), Dev(Bsz, np.int32)
        base = Bsz * (8 * nu + 8 + 4 + 4)
        nbytes = {"a_plain": base, "b_uplan": base + 8 * Bsz * nu * N, "c_uplan_xplan": base + 8 * Bsz * (nu * N + nx * (N + 1))}
        s.reserve(nx, nu, N, Bsz)
        if cfg in a.configs:
            v = {"a_plain": lambda: s.solve_batch_dev(nx, nu, N, Bsz, dA, dB, *w, dx, du, dv, dst, dit)}
            if not a.plain_only:
                v["b_uplan"] = lambda: s.solve_plan_batch_dev(nx, nu, N, Bsz, dA, dB, *w, dx, du, dv, dU, None, dst, dit)
                v["c_uplan_xplan"] = lambda: s.solve_plan_batch_dev(nx, nu, N, Bsz, dA, dB, *w, dx, du, dv, dU, dX, dst, dit)
            r = summary(measure(s, v, a.calls, a.rounds), nbytes)
            s.sync()
            out["solve"][f"C{cfg}x{Bsz}"] = dict(r, kernel=s.last_kernel(), shape=[nx, nu, N], iters_per_qp=round(float(dit.numpy().mean()), 4),
                                                status_nonzero=int((dst.numpy() != 0).sum()))
        if cfg in a.controller:
            ctl = BatchController(s, N, dA, dB, *w)
            v = {"a_plain": lambda: ctl.step_dev(dx, du, dv, dst, dit)}
            if not a.plain_only:
                v["b_uplan"] = lambda: ctl.step_plan_dev(dx, du, dU, None, dv, dst, dit)
                v["c_uplan_xplan"] = lambda: ctl.step_plan_dev(dx, du, dU, dX, dv, dst, dit)
            r = summary(measure(s, v, a.calls, a.rounds), nbytes)
            s.sync()
            out["step"][f"C{cfg}x{Bsz}"] = dict(r, kernel=ctl.kernel, shape=[nx, nu, N])
            ctl.close()
        for d in (dA, dB, dx, du, dv, dU, dX, dst, dit):
            d.free()
    s.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
