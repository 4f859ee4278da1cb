"""Dev tool: what the polytope kernels (lqmpc_poly_solve_kernel, lqmpc_poly_rollout_kernel) cost next to the box kernels; prints one
JSON line.

    python tools/poly_time.py [--cases C3 C3R C4] [--mixes default hard] [--calls 5] [--rounds 2] [--out FILE]

Cases: C3 = (4,2,10) x 65 536 one-shot, C3R = the same batch as a T = 30 rollout, C4 = (4,2,20) x 65 536 one-shot; synth's default
and hard mix.  The parent commit cannot solve a polytope, so the only baselines are the box kernels on a box-shaped Fu:
    box_auto     solve_batch_dev / rollout_batch_dev, options.kernel = AUTO
    box_generic  the same calls with options.kernel = GENERIC
    poly_box     solve_poly_batch_dev / rollout_poly_batch_dev on the rows of that box (m = 4)
    poly_oct     ... on the octagon of the same inradius (m = 8)
Every measurement is a process of its own (this one never opens the GPU): device-resident arrays, three warm-up calls, then `calls`
calls between lqmpc_timer_begin and lqmpc_timer_end.  The variants of a case alternate, `rounds` times, so that a drift of the clock
shows as spread inside every variant and not as a difference between them.  Reported: every round's ms per call, the medians and their
ratios to box_auto and box_generic, the sum of iters of the last call."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("box_auto", "box_generic", "poly_box", "poly_oct")
CASES = {"C3": (3, 0), "C3R": (3, 30), "C4": (4, 0)}
BSZ = 65536


def child(case, mix, variant, calls):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from lq_mpc_amd import BatchSolver, _lib, synth
    from plan_time import Dev
    cfg, T = CASES[case]
    s = BatchSolver(0)
    if variant == "box_generic":
        s.set_options(kernel=_lib.KERNEL_GENERIC)
    b = synth.make_batch(cfg, Bsz=BSZ, mix=mix)
    nx, nu, Bsz = b["B"].shape
    N, h = b["N"], synth.U_MAX
    th = 0.2 + np.arange(8) * 2 * np.pi / 8
    Fu = np.vstack([np.eye(nu) / h, -np.eye(nu) / h]) if variant == "poly_box" else np.stack([np.cos(th), np.sin(th)], 1) / h
    w = (b["Q"], b["R"], b["P"])
    dA, dB, dx = Dev(b["A"].shape, init=b["A"]), Dev(b["B"].shape, init=b["B"]), Dev(b["x0"].shape, init=b["x0"])
    du, dv, dJ = Dev((nu, Bsz)), Dev(Bsz), Dev(Bsz)
    dst, dit = Dev(Bsz, np.int32), Dev(Bsz, np.int32)
    poly = variant.startswith("poly")
    if not poly:
        s.reserve(nx, nu, N, Bsz, T)
    if T:
        go = ((lambda: s.rollout_poly_batch_dev(nx, nu, N, Bsz, T, dA, dB, *w, Fu, dx, b["A_true"], b["B_true"], dJ, None, None, dst, dit))
              if poly else
              (lambda: s.rollout_batch_dev(nx, nu, N, Bsz, T, dA, dB, *w, b["lb"], b["ub"], dx, b["A_true"], b["B_true"], dJ, None, None, dst, dit)))
    else:
        go = ((lambda: s.solve_poly_batch_dev(nx, nu, N, Bsz, dA, dB, *w, Fu, dx, du, dv, None, None, None, dst, dit)) if poly else
              (lambda: s.solve_batch_dev(nx, nu, N, Bsz, dA, dB, *w, b["lb"], b["ub"], dx, du, dv, dst, dit)))
    for _ in range(3):
        go()
    s.timer_begin()
    for _ in range(calls):
        go()
    ms = s.timer_end() / calls
    st, it = dst.numpy(), dit.numpy()
    print(json.dumps(dict(ms=ms, kernel=s.last_kernel(), shape=[nx, nu, N], Bsz=int(Bsz), T=T, status_nonzero=int((st != 0).sum()),
                          iters_sum=int(it.sum(dtype=np.int64)), iters_max=int(it.max()))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=list(CASES))
    ap.add_argument("--mixes", nargs="*", default=["default", "hard"])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(*a.child, a.calls)
    out = {"tool": "poly_time", "calls": a.calls, "rounds": a.rounds, "cases": {}}
    for case in a.cases:
        for mix in a.mixes:
            rec = {v: [] for v in VARIANTS}
            info = {}
            for _ in range(a.rounds):
                for v in VARIANTS:
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, mix, v, "--calls", str(a.calls)],
                                       capture_output=True, text=True, timeout=300)
                    if r.returncode != 0:
                        raise SystemExit(f"{case} {mix} {v}: exit {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-4000:]}")
                    info[v] = json.loads(r.stdout.strip().splitlines()[-1])
                    rec[v].append(round(info[v].pop("ms"), 5))
            med = {v: round(float(np.median(rec[v])), 5) for v in VARIANTS}
            out["cases"][f"{case}-{mix}"] = dict(
                ms=rec, median_ms=med, info=info,
                over_box_auto={v: round(med[v] / med["box_auto"], 2) for v in VARIANTS[2:]},
                over_box_generic={v: round(med[v] / med["box_generic"], 2) for v in VARIANTS[2:]})
            print(case, mix, med, file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
