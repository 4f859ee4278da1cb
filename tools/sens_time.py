"""Dev tool: what the post-pass of the sens calls (lqmpc_sens_kernel) costs on top of the plan call it follows; prints one JSON line.

    python tools/sens_time.py [--cases C3 C4 C5 W16 S3] [--calls 10] [--rounds 3] [--lib OTHER.so] [--out FILE]

Cases: C3 x 65 536, C4 x 262 144, C5 x 32 768 (the bench's default mix and batch sizes), W16 = (16, 4, 8) x 65 536 on the default
generic routing (random models of spectral radius in [0.5, 1], as the tests' problems), all through lqmpc_solve_plan_batch_dev /
lqmpc_solve_sens_batch_dev; S3 = a prepared controller at C3, step_plan_dev / step_sens_dev (warm: the same state again).
Variants per case: "plan" (Uplan and Xplan written), "sens" (the same, and K_0, dV_dx), "sens_kplan" (and K_plan).
Every measurement is a process of its own (this one never opens the GPU): device-resident arrays, three warm-up rounds, then `calls`
calls between lqmpc_timer_begin and lqmpc_timer_end.  The variants of a case alternate, `rounds` times, so that a drift of the clock
shows as spread inside every variant and not as a difference between them.  Reported: every round's ms per call, the median, and the
post-pass as the difference of the medians."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("plan", "sens", "sens_kplan")
CASES = {"C3": 3, "C4": 4, "C5": 5, "W16": (16, 4, 8, 65536), "S3": 3}


def wide_batch(nx, nu, N, Bsz):
    rng = np.random.default_rng(17 * nx + N)
    A = rng.standard_normal((nx, nx, Bsz))
    A *= rng.uniform(0.5, 1.0, Bsz) / np.abs(np.linalg.eigvals(A.transpose(2, 0, 1))).max(axis=1)
    B = rng.standard_normal((nx, nu, Bsz)) * rng.uniform(0.3, 1.0, (1, 1, Bsz))

    def spd(m, c):
        q, _ = np.linalg.qr(rng.standard_normal((m, m)))
        return (q * np.geomspace(1.0, c, m)) @ q.T
    ub = rng.uniform(0.1, 0.4, nu)
    x0 = rng.standard_normal((nx, Bsz)) * rng.choice([0.01, 0.3, 3.0], Bsz)
    return dict(N=N, A=np.ascontiguousarray(A), B=np.ascontiguousarray(B), Q=spd(nx, 10.0), R=spd(nu, 10.0), P=3.0 * spd(nx, 10.0),
                lb=-ub, ub=ub, x0=np.ascontiguousarray(x0))


def child(case, variant, calls, lib):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from lq_mpc_amd import BatchController, BatchSolver, _lib, synth
    if lib:
        _lib.LIB_PATH = os.path.abspath(lib)
    from plan_time import Dev
    s = BatchSolver(0)
    b = synth.make_batch(CASES[case]) if isinstance(CASES[case], int) else wide_batch(*CASES[case])
    nx, nu, Bsz = b["B"].shape
    N = b["N"]
    w = (b["Q"], b["R"], b["P"], b["lb"], b["ub"])
    dA, dB, dx = Dev(b["A"].shape, init=b["A"]), Dev(b["B"].shape, init=b["B"]), Dev(b["x0"].shape, init=b["x0"])
    du, dv, dU, dX = Dev((nu, Bsz)), Dev(Bsz), Dev((nu, N, Bsz)), Dev((nx, N + 1, Bsz))
    dst, dit = Dev(Bsz, np.int32), Dev(Bsz, np.int32)
    dK0, ddV = Dev((nu, nx, Bsz)), Dev((nx, Bsz))
    dKp = Dev((nu, N, nx, Bsz)) if variant == "sens_kplan" else None
    s.reserve(nx, nu, N, Bsz)
    if case.startswith("S"):
        ctl = BatchController(s, N, dA, dB, *w)
        go = ((lambda: ctl.step_plan_dev(dx, du, dU, dX, dv, dst, dit)) if variant == "plan" else
              (lambda: ctl.step_sens_dev(dx, du, dK0, ddV, dKp, dU, dX, dv, dst, dit)))
    else:
        go = ((lambda: s.solve_plan_batch_dev(nx, nu, N, Bsz, dA, dB, *w, dx, du, dv, dU, dX, dst, dit)) if variant == "plan" else
              (lambda: s.solve_sens_batch_dev(nx, nu, N, Bsz, dA, dB, *w, dx, du, dv, dK0, ddV, dKp, dU, dX, dst, dit)))
    for _ in range(3):
        go()
    s.timer_begin()
    for _ in range(calls):
        go()
    ms = s.timer_end() / calls
    st = dst.numpy()
    print(json.dumps(dict(ms=ms, kernel=s.last_kernel(), shape=[nx, nu, N], Bsz=int(Bsz), status_nonzero=int((st != 0).sum()))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=list(CASES))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lib", default=None, help="another build of the library (default: the tree's), to compare two builds of the kernel")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.calls, a.lib)
    out = {"tool": "sens_time", "lib": a.lib, "calls": a.calls, "rounds": a.rounds, "cases": {}}
    for case in a.cases:
        rec = {v: [] for v in VARIANTS}
        info = {}
        for _ in range(a.rounds):
            for v in VARIANTS:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, v, "--calls", str(a.calls)] + (["--lib", a.lib] if a.lib else []),
                                   capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    raise SystemExit(f"{case} {v}: exit {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-4000:]}")
                info = json.loads(r.stdout.strip().splitlines()[-1])
                rec[v].append(round(info.pop("ms"), 5))
        med = {v: round(float(np.median(rec[v])), 5) for v in VARIANTS}
        out["cases"][case] = dict(info, ms=rec, median_ms=med, post_pass_ms=round(med["sens"] - med["plan"], 5),
                                  post_pass_with_kplan_ms=round(med["sens_kplan"] - med["plan"], 5))
        print(case, out["cases"][case], file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
