"""Times a prepared controller's step against a one-shot solve at the headline shape; prints one JSON line.

    python tools/controller_time.py [--config 3] [--calls 20] [--rounds 5] [--out FILE]
    python tools/controller_time.py --config 5          (records on the workgroup kernel's shapes, options.ctl_wg = 1;
                                                         also written to profiles/controller_c5.json)

Per mix (default, hard): 20 lqmpc_solve_batch_dev calls and 20 BatchController.step_dev calls on the same states, measured
alternately with the handle's own timer after three warm-up rounds, median of the rounds; the step both repeated (warm face)
and after reset() (cold; the figure includes the reset's fill of the stored faces).

    python tools/controller_time.py --retarget [--config 3|5]
New references in every call (two sets taken in turn, default mix): set_reference alone, set_reference + step with the face kept,
set_reference + reset + step, destroy + create + step, and the one-shot solve with the same references; the result is kept under
"C<config>" in profiles/controller_retarget.json.

    python tools/controller_time.py --set-model [--config 3|5]
New models in place (BatchController.set_model, device flavour) against re-creating the controller: set_model of every instance
+ step, destroy + create + step, set_model alone for all, 4 096 and 64 listed instances, and the plain step; kept under "C<config>"
in profiles/controller_set_model.json.

    python tools/controller_time.py --rollout [--config 3|4|5] [--bsz 4096] [--steps 30]
A closed loop of T steps (default mix, the batch's own plant): lqmpc_rollout_batch_dev against the controller's rollout_dev on the
same data, measured alternately (one call per timing, three warm-up rounds, median of the rounds), and once the loop of T step_dev
calls the rollout replaces (at one state, without a plant update: a lower bound of that loop).  Kept under "C<config>" or
"C<config>x<bsz>" in profiles/controller_rollout.json, with the kernel each call ran."""
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
    ap.add_argument("--retarget", action="store_true", help="time set_reference against re-creating the controller and against a one-shot solve")
    ap.add_argument("--set-model", action="store_true", help="time set_model against re-creating the controller")
    ap.add_argument("--rollout", action="store_true", help="time the controller's rollout against lqmpc_rollout_batch_dev")
    ap.add_argument("--bsz", type=int, default=None, help="--rollout: instances (default: the bench's batch size of the config)")
    ap.add_argument("--steps", type=int, default=30, help="--rollout: closed-loop steps T")
    a = ap.parse_args()
    if a.out is None and a.config == 5 and not a.retarget and not a.set_model:
        a.out = os.path.join(ROOT, "profiles", "controller_c5.json")
    import torch
    from lq_mpc_amd import BatchController, BatchSolver, synth
    torch.cuda.init()                                     # torch opens the GPU before the library does
    s = BatchSolver(0)
    if a.config == 5:
        s.set_options(ctl_wg=1)                           # the workgroup kernel's shapes keep records only on request
    out = {"tool": "controller_time", "config": a.config, "calls": a.calls, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    if a.retarget:
        retarget(a, s, out, torch)
        return
    if a.set_model:
        set_model(a, s, out, torch)
        return
    if a.rollout:
        rollout(a, s, out, torch)
        return
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


def retarget(a, s, out, torch):
    from lq_mpc_amd import BatchController, synth
    b = synth.make_batch(a.config)
    nx, nu, Bsz = b["B"].shape
    N = b["N"]
    rng = np.random.default_rng(5)
    R = [(0.1 * rng.standard_normal((nx, N)), 0.05 * rng.standard_normal((nu, N))) for _ in range(2)]
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    dA, dB, dx = dev(b["A"]), dev(b["B"]), dev(b["x0"])
    du = torch.empty((nu, Bsz), dtype=torch.float64, device="cuda")
    dv = torch.empty(Bsz, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s.reserve(nx, nu, N, Bsz)
    fixed = (b["Q"], b["R"], b["P"], b["lb"], b["ub"])
    ctl = [BatchController(s, N, dA, dB, *fixed)]

    def timed(body):
        s.timer_begin()
        for k in range(a.calls):
            body(k)
        return s.timer_end() / a.calls

    def set_step(k, cold):
        ctl[0].set_reference(*R[k & 1])
        if cold:
            ctl[0].reset()
        ctl[0].step_dev(dx, du, dv)

    def recreate(k):
        ctl[0].close()
        ctl[0] = BatchController(s, N, dA, dB, *fixed, *R[k & 1])
        ctl[0].step_dev(dx, du, dv)

    legs = {"t_set_reference_ms": lambda k: ctl[0].set_reference(*R[k & 1]),
            "t_set_reference_step_warm_ms": lambda k: set_step(k, False),
            "t_set_reference_step_cold_ms": lambda k: set_step(k, True),
            "t_destroy_create_step_ms": recreate,
            "t_solve_with_references_ms": lambda k: s.solve_batch_dev(nx, nu, N, Bsz, dA, dB, *fixed, dx, du, dv, x_ref=R[k & 1][0], u_ref=R[k & 1][1])}
    for _ in range(3):
        for f in legs.values():
            timed(f)
    r = [{k: timed(f) for k, f in legs.items()} for _ in range(a.rounds)]
    res = {k: round(float(np.median([q[k] for q in r])), 5) for k in legs}
    rec = ctl[0].nbytes / Bsz
    res.update(shape=[nx, nu, N], Bsz=Bsz, kernel=ctl[0].kernel, bytes_per_instance=rec, device=out["device"], calls=a.calls, rounds=a.rounds)
    ctl[0].close()
    s.close()
    path = a.out or os.path.join(ROOT, "profiles", "controller_retarget.json")
    allr = json.load(open(path)) if os.path.exists(path) else {"tool": "controller_time --retarget"}
    allr[f"C{a.config}"] = res
    print(json.dumps({f"C{a.config}": res}))
    with open(path, "w") as f:
        f.write(json.dumps(allr, indent=1) + "\n")


def set_model(a, s, out, torch):
    from lq_mpc_amd import BatchController, synth
    b = synth.make_batch(a.config)
    nx, nu, Bsz = b["B"].shape
    N = b["N"]
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    dA, dB, dx = dev(b["A"]), dev(b["B"]), dev(b["x0"])
    du = torch.empty((nu, Bsz), dtype=torch.float64, device="cuda")
    dv = torch.empty(Bsz, dtype=torch.float64, device="cuda")
    part = {}
    for m in (4096, 64):
        idx = np.random.default_rng(m).permutation(Bsz)[:m]
        part[m] = (dev(b["A"][..., idx]), dev(b["B"][..., idx]), dev(idx.astype(np.int32)))
    torch.cuda.synchronize()
    s.reserve(nx, nu, N, Bsz)
    fixed = (b["Q"], b["R"], b["P"], b["lb"], b["ub"])
    ctl = [BatchController(s, N, dA, dB, *fixed)]

    def timed(body):
        s.timer_begin()
        for _ in range(a.calls):
            body()
        return s.timer_end() / a.calls

    def update_step():
        ctl[0].set_model(dA, dB)
        ctl[0].step_dev(dx, du, dv)

    def recreate():
        ctl[0].close()
        ctl[0] = BatchController(s, N, dA, dB, *fixed)
        ctl[0].step_dev(dx, du, dv)

    legs = {"t_set_model_all_step_ms": update_step,
            "t_destroy_create_step_ms": recreate,
            "t_set_model_all_ms": lambda: ctl[0].set_model(dA, dB),
            "t_set_model_4096_ms": lambda: ctl[0].set_model(*part[4096]),
            "t_set_model_64_ms": lambda: ctl[0].set_model(*part[64]),
            "t_step_ms": lambda: ctl[0].step_dev(dx, du, dv)}
    for _ in range(3):
        for f in legs.values():
            timed(f)
    r = [{k: timed(f) for k, f in legs.items()} for _ in range(a.rounds)]
    res = {k: round(float(np.median([q[k] for q in r])), 5) for k in legs}
    res.update(shape=[nx, nu, N], Bsz=Bsz, kernel=ctl[0].kernel, bytes_per_instance=ctl[0].nbytes / Bsz, device=out["device"], calls=a.calls,
               rounds=a.rounds)
    ctl[0].close()
    s.close()
    path = a.out or os.path.join(ROOT, "profiles", "controller_set_model.json")
    allr = json.load(open(path)) if os.path.exists(path) else {"tool": "controller_time --set-model"}
    allr[f"C{a.config}"] = res
    print(json.dumps({f"C{a.config}": res}))
    with open(path, "w") as f:
        f.write(json.dumps(allr, indent=1) + "\n")


def rollout(a, s, out, torch):
    from lq_mpc_amd import BatchController, synth
    b = synth.make_batch(a.config) if a.bsz is None else synth.make_batch(a.config, Bsz=a.bsz)
    nx, nu, Bsz = b["B"].shape
    N, T = b["N"], a.steps
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    dA, dB, dx = dev(b["A"]), dev(b["B"]), dev(b["x0"])
    per = np.ndim(b["A_true"]) == 3
    At, Bt = (dev(b["A_true"]), dev(b["B_true"])) if per else (b["A_true"], b["B_true"])
    dJ = [torch.empty(Bsz, dtype=torch.float64, device="cuda") for _ in range(2)]
    du = torch.empty((nu, Bsz), dtype=torch.float64, device="cuda")
    dst = torch.empty(Bsz, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s.reserve(nx, nu, N, Bsz, T)
    fixed = (b["Q"], b["R"], b["P"], b["lb"], b["ub"])
    ctl = BatchController(s, N, dA, dB, *fixed)
    names = {}

    def timed(body, calls=1):
        s.timer_begin()
        for _ in range(calls):
            body()
        return s.timer_end() / calls

    def one_shot():
        s.rollout_batch_dev(nx, nu, N, Bsz, T, dA, dB, *fixed, dx, At, Bt, dJ[0], dstatus=dst, true_per_instance=per)
        names["one_shot"] = s.last_kernel()

    def prepared():
        ctl.rollout_dev(T, dx, At, Bt, dJ[1], dstatus=dst, true_per_instance=per)
        names["controller"] = s.last_kernel()

    def step_loop():
        for _ in range(T):
            ctl.step_dev(dx, du)

    legs = {"t_rollout_batch_dev_ms": one_shot, "t_controller_rollout_dev_ms": prepared}
    for _ in range(3):
        for f in legs.values():
            timed(f)
    r = [{k: timed(f) for k, f in legs.items()} for _ in range(a.rounds)]
    res = {k: round(float(np.median([q[k] for q in r])), 5) for k in legs}
    s.sync()
    j0, j1 = dJ[0].cpu().numpy(), dJ[1].cpu().numpy()
    timed(step_loop)
    res["t_step_dev_loop_ms"] = round(timed(step_loop), 5)
    res.update(one_shot_over_controller=round(res["t_rollout_batch_dev_ms"] / res["t_controller_rollout_dev_ms"], 3),
               max_rel_diff_J_T=float(np.max(np.abs(j0 - j1) / np.abs(j0))), status_nonzero=int((dst.cpu().numpy() != 0).sum()),
               kernel_one_shot=names["one_shot"], kernel_controller=names["controller"], kernel_step=ctl.kernel,
               shape=[nx, nu, N], Bsz=Bsz, T=T, plant="per instance" if per else "shared", bytes_per_instance=ctl.nbytes / Bsz,
               device=out["device"], rounds=a.rounds)
    ctl.close()
    s.close()
    key = f"C{a.config}" if a.bsz is None else f"C{a.config}x{a.bsz}"
    path = a.out or os.path.join(ROOT, "profiles", "controller_rollout.json")
    allr = json.load(open(path)) if os.path.exists(path) else {"tool": "controller_time --rollout"}
    allr[key] = res
    print(json.dumps({key: res}))
    with open(path, "w") as f:
        f.write(json.dumps(allr, indent=1) + "\n")


if __name__ == "__main__":
    main()
