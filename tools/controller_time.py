"""Times a prepared controller's step against a one-shot solve at the headline shape; prints one JSON line.

    python tools/controller_time.py [--config 3] [--calls 20] [--rounds 5] [--out FILE]
    python tools/controller_time.py --config 5          (records on the workgroup kernel's shapes, options.ctl_wg = 1;
                                                         also written to profiles/controller_c5.json)

Per mix (default, hard): 20 lqmpc_solve_batch_dev calls and 20 BatchController.step_dev calls on the same states, measured
alternately with the handle's own timer after three warm-up rounds, median of the rounds; the step both repeated (warm face)
and after reset() (cold; the figure includes the reset's fill of the stored faces)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file (default for --config 5: profiles/controller_c5.json)")
    a = ap.parse_args()
    if a.out is None and a.config == 5:
        a.out = os.path.join(ROOT, "profiles", "controller_c5.json")
    import torch
    from lq_mpc_amd import BatchController, BatchSolver, synth
    torch.cuda.init()                                     # torch opens the GPU before the library does
    s = BatchSolver(0)
    if a.config == 5:
        s.set_options(ctl_wg=1)                           # the workgroup kernel's shapes keep records only on request
    out = {"tool": "controller_time", "config": a.config, "calls": a.calls, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    for mix in ("default", "hard"):
        b = synth.make_batch(a.config, mix=mix)
        nx, nu, Bsz = b["B"].shape
        N = b["N"]
        dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
        dA, dB, dx = dev(b["A"]), dev(b["B"]), dev(b["x0"])
        du = torch.empty((nu, Bsz), dtype=torch.float64, device="cuda")
        dv = torch.empty(Bsz, dtype=torch.float64, device="cuda")
        di = torch.empty(Bsz, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        s.reserve(nx, nu, N, Bsz)
        t0 = time.perf_counter()
        ctl = BatchController(s, N, dA, dB, b["Q"], b["R"], b["P"], b["lb"], b["ub"])
        create_ms = (time.perf_counter() - t0) * 1e3

        def solve():
            s.timer_begin()
            for _ in range(a.calls):
                s.solve_batch_dev(nx, nu, N, Bsz, dA, dB, b["Q"], b["R"], b["P"], b["lb"], b["ub"], dx, du, dv)
            return s.timer_end() / a.calls

        def step(cold):
            s.timer_begin()
            for _ in range(a.calls):
                if cold:
                    ctl.reset()
                ctl.step_dev(dx, du, dv)
            return s.timer_end() / a.calls

        for _ in range(3):
            solve(); step(True); step(False)
        r = [(solve(), step(True), step(False)) for _ in range(a.rounds)]
        ts, tc, tw = (float(np.median([q[k] for q in r])) for k in range(3))
        # the same comparison at states deep inside the region where the box is inactive (what most steps of a settled loop look like)
        dx_far = dx
        dx = dev(0.02 * b["x0"])
        torch.cuda.synchronize()
        for _ in range(2):
            solve(); step(False)
        rf = [(solve(), step(False)) for _ in range(a.rounds)]
        tsf, twf = (float(np.median([q[k] for q in rf])) for k in range(2))
        dx = dx_far
        ctl.reset()
        ctl.step_dev(dx, du, dv, None, di)
        s.sync()
        it = di.cpu().numpy()
        out[mix] = {"shape": [nx, nu, N], "Bsz": Bsz, "kernel": ctl.kernel, "t_solve_ms": round(ts, 5), "t_step_cold_ms": round(tc, 5),
                    "t_step_warm_ms": round(tw, 5), "solve_over_step_warm": round(ts / tw, 3), "solve_over_step_cold": round(ts / tc, 3),
                    "bytes_per_instance": ctl.nbytes / Bsz, "create_ms": round(create_ms, 3),
                    "share_of_instances_iterating": round(float((it > 0).mean()), 4),
                    "free_states": {"t_solve_ms": round(tsf, 5), "t_step_ms": round(twf, 5), "solve_over_step": round(tsf / twf, 3)}}
        ctl.close()
    s.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
