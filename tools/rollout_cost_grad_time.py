"""Dev tool: what the gradient of a closed loop in the weights, the references and the box costs; prints one JSON line
(profiles/rollout_cost_grad_speed.json).

    python tools/rollout_cost_grad_time.py [--cases C3 C4 C5] [--variants ...] [--calls 5] [--rounds 3] [--lib FILE ...] [--out FILE]

Cases: C3 x 65 536 with T = 30, C4 x 262 144 with T = 10, C5 x 32 768 with T = 5 (the bench's default mix and batch sizes, the plant
shared by the batch).  Variants per case, all on the same data and the same tape:
  "fused"          one lqmpc_rollout_cost_grad_batch_dev (lqmpc_rollout_cost_grad_kernel), per instance: the seven outputs
  "fused_reduced"  the same with reduce: the sums over the batch (a second small launch adds one vector per wavefront)
  "chain"          the composition it replaces: per step, newest first, one lqmpc_cost_grad_batch_dev (per instance) and one
                   lqmpc_model_grad_batch_dev (for g_x0 of the step), with the plant's costate, the cotangent of every step, the
                   direct part and the sums in torch between them (the states of every plan, which that composition's own forward
                   would have kept, are rolled once outside the timed part)
  "sibling"        lqmpc_rollout_grad_batch_dev on the same tape: the model's and the plant's gradients
--lib: other builds of the library (say with -DRC_WAVES=3 or -DRC_REUSE=0 for csrc/lqmpc_rcgrad.hip), each timed as a variant
"fused@FILE" beside the others: how the kernel's build constants were chosen.
Every measurement is a process of its own in which torch opens the GPU first and the solver borrows torch's stream (this one never
opens the GPU): device-resident tensors, two warm-up calls, then `calls` calls between two events.  The variants of a case alternate,
`rounds` times, so that a drift of the clock shows as spread inside every variant and not as a difference between them.  Reported:
every round's ms per call and the median."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("fused", "fused_reduced", "chain", "sibling")
CASES = {"C3": (3, 30), "C4": (4, 10), "C5": (5, 5)}
KEYS = ("g_Q", "g_R", "g_P", "g_lb", "g_ub", "g_xref", "g_uref")


def child(case, variant, calls, bsz):
    import torch
    sys.path.insert(0, ROOT)
    variant, _, libfile = variant.partition("@")
    if libfile:
        from lq_mpc_amd import _lib
        _lib.LIB_PATH = os.path.abspath(libfile)
    from lq_mpc_amd import BatchSolver, synth
    torch.cuda.init()
    cfg, T = CASES[case]
    b = synth.make_batch(cfg, Bsz=bsz or None)
    nx, nu, Bsz = b["B"].shape
    N = b["N"]
    w = (b["Q"], b["R"], b["P"], b["lb"], b["ub"])
    At, Bt = b["A_true"], b["B_true"]
    stream = torch.cuda.current_stream()
    s = BatchSolver(stream.device_index, stream=stream.cuda_stream)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    A, B, x0 = dev(b["A"]), dev(b["B"]), dev(b["x0"])
    JT, X, U, Ut = new(Bsz), new(nx, T + 1, Bsz), new(nu, T, Bsz), new(T, nu, N, Bsz)
    st, it = torch.empty(Bsz, dtype=torch.int32, device="cuda"), torch.empty(Bsz, dtype=torch.int32, device="cuda")
    stt = torch.empty((T, Bsz), dtype=torch.int32, device="cuda")
    s.reserve(nx, nu, N, Bsz, T)
    s.rollout_tape_batch_dev(nx, nu, N, Bsz, T, A, B, *w, x0, At, Bt, JT, Ut, dX=X, dU=U, dstatus=st, diters=it, dstatus_tape=stt)
    rng = np.random.default_rng(5)
    gJ, gX, gU = dev(rng.standard_normal(Bsz)), dev(rng.standard_normal((nx, T + 1, Bsz))), dev(rng.standard_normal((nu, T, Bsz)))
    shapes = dict(g_Q=(nx, nx), g_R=(nu, nu), g_P=(nx, nx), g_lb=(nu,), g_ub=(nu,), g_xref=(nx, N), g_uref=(nu, N))
    info = {}
    outs = None
    if variant == "fused":
        outs = {k: new(*shapes[k], Bsz) for k in KEYS}
        go = lambda: s.rollout_cost_grad_batch_dev(nx, nu, N, Bsz, T, A, B, *w, At, Bt, X, Ut, outs, dstatus_tape=stt, dgJT=gJ, dgX=gX, dgU=gU)
    elif variant == "fused_reduced":
        outs = {k: new(*shapes[k]) for k in KEYS}
        skipped = torch.zeros(1, dtype=torch.int64, device="cuda")
        go = lambda: s.rollout_cost_grad_batch_dev(nx, nu, N, Bsz, T, A, B, *w, At, Bt, X, Ut, outs, dstatus_tape=stt, dgJT=gJ, dgX=gX, dgU=gU,
                                                   reduce=True, dskipped=skipped)
    elif variant == "chain":
        Xp = new(T, nx, N + 1, Bsz)
        Xp[:, :, 0] = X[:, :T].permute(1, 0, 2)
        for i in range(N):
            Xp[:, :, i + 1] = torch.einsum("acb,tcb->tab", A, Xp[:, :, i]) + torch.einsum("akb,tkb->tab", B, Ut[:, :, i])
        Q, R, dAt, dBt = dev(b["Q"]), dev(b["R"]), dev(At), dev(Bt)
        outs = {k: new(*shapes[k], Bsz) for k in KEYS}
        step = {k: new(*shapes[k], Bsz) for k in KEYS}
        tA, tB, tx = new(nx, nx, Bsz), new(nx, nu, Bsz), new(nx, Bsz)

        def go():
            lam = gX[:, T] + 2 * gJ * (Q @ X[:, T])
            for k in KEYS:
                outs[k].zero_()
            outs["g_Q"].add_(gJ * X[:, T][:, None, :] * X[:, T][None, :, :])
            for t in range(T - 1, -1, -1):
                u = Ut[t, :, 0]
                wt = (gU[:, t] + 2 * gJ * (R @ u) + dBt.T @ lam).contiguous()
                s.cost_grad_batch_dev(nx, nu, N, Bsz, A, B, *w, Ut[t], Xp[t], step, dstatus=stt[t], dgu0=wt)
                s.model_grad_batch_dev(nx, nu, N, Bsz, A, B, *w, Ut[t], Xp[t], tA, tB, dstatus=stt[t], dgu0=wt, dgx0=tx)
                for k in KEYS:
                    outs[k].add_(step[k])
                outs["g_Q"].add_(gJ * X[:, t][:, None, :] * X[:, t][None, :, :])
                outs["g_R"].add_(gJ * u[:, None, :] * u[None, :, :])
                lam = gX[:, t] + 2 * gJ * (Q @ X[:, t]) + dAt.T @ lam + tx
    else:
        gA, gB, gx, gAt, gBt = new(nx, nx, Bsz), new(nx, nu, Bsz), new(nx, Bsz), new(nx, nx, Bsz), new(nx, nu, Bsz)
        go = lambda: s.rollout_grad_batch_dev(nx, nu, N, Bsz, T, A, B, *w, At, Bt, X, Ut, dstatus_tape=stt, dgJT=gJ, dgX=gX, dgU=gU, dgA=gA,
                                              dgB=gB, dgx0=gx, dgA_true=gAt, dgB_true=gBt)
    for _ in range(2):
        go()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        go()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / calls
    if outs is not None:
        # the sums over the batch of every variant's outputs: they agree between the variants to rounding
        red = (lambda v: v) if variant == "fused_reduced" else (lambda v: v.sum(dim=-1))
        info["abs_sum"] = {k: float(red(outs[k]).abs().sum()) for k in KEYS}
        info["finite"] = bool(all(torch.isfinite(outs[k]).all() for k in KEYS))
    free = ((Ut.abs() - dev(b["ub"])[None, :, None, None]).abs() > 0)
    sat, allfree = ~free[:, :, 0].any(dim=1), free.all(dim=1).all(dim=1)
    info["steps_stage0_on_bounds_mixed_all_free"] = [round(float(sat.double().mean()), 4), round(float((~sat & ~allfree).double().mean()), 4),
                                                     round(float(allfree.double().mean()), 4)]
    print(json.dumps(dict(ms=ms, solve_kernel=s.last_kernel(), shape=[nx, nu, N], Bsz=int(Bsz), T=T,
                          status_nonzero=int((stt != 0).sum()), **info)))
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=list(CASES))
    ap.add_argument("--variants", nargs="*", default=list(VARIANTS))
    ap.add_argument("--lib", nargs="*", default=[], help="other builds of the library, each timed as fused@FILE")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bsz", type=int, default=0, help="batch size (default: the bench's for the case)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.calls, a.bsz)
    variants = list(a.variants) + ["fused@" + f for f in a.lib]
    out = {"tool": "rollout_cost_grad_time", "calls": a.calls, "rounds": a.rounds, "cases": {}}
    for case in a.cases:
        rec = {v: [] for v in variants}
        info = {"abs_sum": {}, "finite": {}}
        for _ in range(a.rounds):
            for v in variants:
                r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", case, v, "--calls", str(a.calls),
                                    "--bsz", str(a.bsz)], capture_output=True, text=True)
                if r.returncode != 0:
                    raise SystemExit(f"{case} {v}: exit {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-4000:]}")
                got = json.loads(r.stdout.strip().splitlines()[-1])
                rec[v].append(round(got.pop("ms"), 4))
                print(case, v, rec[v][-1], "ms", file=sys.stderr, flush=True)
                for k in ("abs_sum", "finite"):
                    if k in got:
                        info[k][v] = got.pop(k)
                info.update(got)
        med = {v: round(float(np.median(rec[v])), 4) for v in variants}
        out["cases"][case] = dict(info, ms=rec, median_ms=med)
        print(case, out["cases"][case], file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
