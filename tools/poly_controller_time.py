"""Dev tool: what the prepared polytope controller (PolyBatchController) costs next to the one-shot polytope calls; prints one JSON
line and writes it to profiles/poly_controller.json.

    python tools/poly_controller_time.py [--cases ...] [--calls 5] [--rounds 2] [--out profiles/poly_controller.json]

Cases, all 65 536 instances: C3-box and C3-oct = (4,2,10) on the rows of the box (m = 4) and on the octagon of the same inradius
(m = 8), synth's default and hard mix; C4-oct = (4,2,20) on the octagon, default mix.  T = 30 for the closed loops.
Variants of a case (the protocol of tools/poly_time.py: data resident in HBM, three warm-up calls, then `calls` calls between
lqmpc_timer_begin and lqmpc_timer_end; the variants alternate, `rounds` times, and the median over the rounds is reported):
    solve        solve_poly_batch_dev at x0
    step         step_dev at x0 from a controller made once (create_ms: host clock around create_dev, which waits for the stream)
    rollout      rollout_poly_batch_dev(T)
    ctl_rollout  the controller's rollout_dev(T)
    steps        T step_dev calls at the states x_0 .. x_{T-1} of that rollout, resident in HBM (a loop the caller owns)
    set_model    set_model of all instances (device flavour)
    set_model64  set_model of 64 instances through a device index list
One process per case (this one never opens the GPU).  Every child checks that step and solve, and the two rollouts, agree bit for
bit before it times anything."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"C3-box-default": (3, "box", "default"), "C3-box-hard": (3, "box", "hard"), "C3-oct-default": (3, "oct", "default"),
         "C3-oct-hard": (3, "oct", "hard"), "C4-oct-default": (4, "oct", "default")}
VARIANTS = ("solve", "step", "rollout", "ctl_rollout", "steps", "set_model", "set_model64")
BSZ, T = 65536, 30


def child(case, calls, rounds):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from lq_mpc_amd import BatchSolver, PolyBatchController, _lib, synth
    from plan_time import Dev
    cfg, rows, mix = CASES[case]
    s = BatchSolver(0)
    b = synth.make_batch(cfg, Bsz=BSZ, mix=mix)
    nx, nu, Bsz = b["B"].shape
    N, h = b["N"], synth.U_MAX
    th = 0.2 + np.arange(8) * 2 * np.pi / 8
    Fu = np.vstack([np.eye(nu) / h, -np.eye(nu) / h]) if rows == "box" else np.stack([np.cos(th), np.sin(th)], 1) / h
    w = (b["Q"], b["R"], b["P"])
    dA, dB, dx = Dev(b["A"].shape, init=b["A"]), Dev(b["B"].shape, init=b["B"]), Dev(b["x0"].shape, init=b["x0"])
    du, dv, dJ = Dev((nu, Bsz)), Dev(Bsz), Dev(Bsz)
    du2, dv2, dJ2 = Dev((nu, Bsz)), Dev(Bsz), Dev(Bsz)
    dst, dit = Dev(Bsz, np.int32), Dev(Bsz, np.int32)
    dX = Dev((nx, T + 1, Bsz))
    s.sync()
    t0 = time.perf_counter()
    c = PolyBatchController(s, N, dA, dB, *w, Fu)
    create_ms = (time.perf_counter() - t0) * 1e3
    di = Dev(64, np.int32, init=np.arange(64) * (Bsz // 64))
    dA64, dB64 = Dev((nx, nx, 64), init=b["A"][..., ::Bsz // 64]), Dev((nx, nu, 64), init=b["B"][..., ::Bsz // 64])

    solve = lambda: s.solve_poly_batch_dev(nx, nu, N, Bsz, dA, dB, *w, Fu, dx, du, dv, None, None, None, dst, dit)
    step = lambda: c.step_dev(dx, du2, dv2, None, None, None, dst, dit)
    rollout = lambda: s.rollout_poly_batch_dev(nx, nu, N, Bsz, T, dA, dB, *w, Fu, dx, b["A_true"], b["B_true"], dJ, dX, None, dst, dit)
    ctl_rollout = lambda: c.rollout_dev(T, dx, b["A_true"], b["B_true"], dJ2, None, None, dst, dit)
    # outputs agree bit for bit before anything is timed
    solve(); step(); rollout(); ctl_rollout(); s.sync()
    assert np.array_equal(du.numpy(), du2.numpy()) and np.array_equal(dv.numpy(), dv2.numpy()), "step differs from solve"
    assert np.array_equal(dJ.numpy(), dJ2.numpy()), "the controller's rollout differs from the one-shot rollout"
    X = dX.numpy()
    states = [Dev((nx, Bsz), init=X[:, t]) for t in range(T)]

    def steps():
        for d in states:
            c.step_dev(d, du2, dv2, None, None, None, dst, dit)

    go = dict(solve=solve, step=step, rollout=rollout, ctl_rollout=ctl_rollout, steps=steps,
              set_model=lambda: c.set_model(dA, dB), set_model64=lambda: c.set_model(dA64, dB64, di))
    ms, info = {v: [] for v in VARIANTS}, {}
    for _ in range(rounds):
        for v in VARIANTS:
            for _ in range(3):
                go[v]()
            s.timer_begin()
            for _ in range(calls):
                go[v]()
            ms[v].append(round(s.timer_end() / calls, 5))
            info[v] = s.last_kernel()
    step(); s.sync()
    st, it = dst.numpy(), dit.numpy()
    print(json.dumps(dict(ms=ms, kernels=info, shape=[nx, nu, N], m=int(Fu.shape[0]), Bsz=int(Bsz), T=T, create_ms=round(create_ms, 3),
                          bytes_held=c.nbytes, record_bytes=int(_lib.lib().lqmpc_poly_controller_record_bytes(nx, nu, N)),
                          status_nonzero=int((st != 0).sum()), iters_sum=int(it.sum(dtype=np.int64)), iters_max=int(it.max()))))
    c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=list(CASES))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poly_controller.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.calls, a.rounds)
    out = {"tool": "poly_controller_time", "calls": a.calls, "rounds": a.rounds, "cases": {}}
    for case in a.cases:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--calls", str(a.calls), "--rounds", str(a.rounds)],
                           capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise SystemExit(f"{case}: exit {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-4000:]}")
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        med = {v: round(float(np.median(rec["ms"][v])), 5) for v in VARIANTS}
        rec["median_ms"] = med
        rec["step_over_solve"] = round(med["step"] / med["solve"], 3)
        rec["ctl_rollout_over_rollout"] = round(med["ctl_rollout"] / med["rollout"], 3)
        rec["steps_over_rollout"] = round(med["steps"] / med["rollout"], 3)
        out["cases"][case] = rec
        print(case, med, file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
