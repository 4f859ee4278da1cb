"""Dev tool: what the plan-gradient post-pass (lqmpc_plan_grad_kernel) costs, beside the model-gradient post-pass (lqmpc_grad_kernel),
which runs the same masked sweep without the affine part; prints one JSON line.

    python tools/pgrad_time.py [--cases C3 C4 C5 S3] [--calls 10] [--rounds 3] [--out FILE]

Cases: C3 x 65 536, C4 x 262 144, C5 x 32 768 (the bench's default mix and batch sizes) through lqmpc_model_grad_batch_dev /
lqmpc_plan_grad_batch_dev on the plan one lqmpc_solve_plan_batch_dev wrote; S3 = a prepared controller at C3, model_grad_dev /
plan_grad_dev on the plan of one step_plan_dev.
Variants per case: "grad" (cotangents of u_0 and V_N; g_A, g_B, g_x0) and "pgrad" (cotangents of every u_i, every x_i and V_N; the same
outputs).  Neither call does a solve, so both are timed directly.
Every measurement is a process of its own (this one never opens the GPU): device-resident arrays, three warm-up rounds, then `calls`
calls between lqmpc_timer_begin and lqmpc_timer_end.  The variants of a case alternate, `rounds` times, so that a drift of the clock
shows as spread inside every variant and not as a difference between them.  Reported: every round's ms per call and the median."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("grad", "pgrad")
CASES = {"C3": 3, "C4": 4, "C5": 5, "S3": 3}


def child(case, variant, calls):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from lq_mpc_amd import BatchController, BatchSolver, synth
    from plan_time import Dev
    s = BatchSolver(0)
    b = synth.make_batch(CASES[case])
    nx, nu, Bsz = b["B"].shape
    N = b["N"]
    w = (b["Q"], b["R"], b["P"], b["lb"], b["ub"])
    dA, dB, dx = Dev(b["A"].shape, init=b["A"]), Dev(b["B"].shape, init=b["B"]), Dev(b["x0"].shape, init=b["x0"])
    du, dv, dU, dX = Dev((nu, Bsz)), Dev(Bsz), Dev((nu, N, Bsz)), Dev((nx, N + 1, Bsz))
    dst, dit = Dev(Bsz, np.int32), Dev(Bsz, np.int32)
    s.reserve(nx, nu, N, Bsz)
    ctl = BatchController(s, N, dA, dB, *w) if case.startswith("S") else None
    rng = np.random.default_rng(5)
    dgv = Dev(Bsz, init=rng.standard_normal(Bsz))
    dgA, dgB, dgx = Dev((nx, nx, Bsz)), Dev((nx, nu, Bsz)), Dev((nx, Bsz))
    if ctl:
        ctl.step_plan_dev(dx, du, dU, dX, dv, dst, dit)
    else:
        s.solve_plan_batch_dev(nx, nu, N, Bsz, dA, dB, *w, dx, du, dv, dU, dX, dst, dit)
    if variant == "grad":
        dgu = Dev((nu, Bsz), init=rng.standard_normal((nu, Bsz)))
        go = ((lambda: ctl.model_grad_dev(dU, dX, dgA, dgB, dst, dgu, dgv, dgx)) if ctl else
              (lambda: s.model_grad_batch_dev(nx, nu, N, Bsz, dA, dB, *w, dU, dX, dgA, dgB, dst, dgu, dgv, dgx)))
    else:
        dgU, dgX = Dev((nu, N, Bsz), init=rng.standard_normal((nu, N, Bsz))), Dev((nx, N + 1, Bsz), init=rng.standard_normal((nx, N + 1, Bsz)))
        go = ((lambda: ctl.plan_grad_dev(dU, dX, dgA, dgB, dst, dgU, dgX, dgv, dgx)) if ctl else
              (lambda: s.plan_grad_batch_dev(nx, nu, N, Bsz, dA, dB, *w, dU, dX, dgA, dgB, dst, dgU, dgX, dgv, dgx)))
    kernel = s.last_kernel()
    for _ in range(3):
        go()
    s.timer_begin()
    for _ in range(calls):
        go()
    ms = s.timer_end() / calls
    st = dst.numpy()
    finite = bool(np.isfinite(dgA.numpy()).all() and np.isfinite(dgx.numpy()).all())
    print(json.dumps(dict(ms=ms, solve_kernel=kernel, shape=[nx, nu, N], Bsz=int(Bsz), status_nonzero=int((st != 0).sum()), finite=finite)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=list(CASES))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.calls)
    out = {"tool": "pgrad_time", "calls": a.calls, "rounds": a.rounds, "cases": {}}
    for case in a.cases:
        rec = {v: [] for v in VARIANTS}
        info = {}
        for _ in range(a.rounds):
            for v in VARIANTS:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, v, "--calls", str(a.calls)],
                                   capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    raise SystemExit(f"{case} {v}: exit {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-4000:]}")
                info = json.loads(r.stdout.strip().splitlines()[-1])
                rec[v].append(round(info.pop("ms"), 5))
        med = {v: round(float(np.median(rec[v])), 5) for v in VARIANTS}
        out["cases"][case] = dict(info, ms=rec, median_ms=med, grad_post_pass_ms=med["grad"], plan_grad_post_pass_ms=med["pgrad"])
        print(case, out["cases"][case], file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
