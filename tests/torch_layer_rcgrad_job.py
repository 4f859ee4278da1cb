"""Child process of tests/test_gpu_torch_layer_rcgrad.py (not a test module).

    python tests/torch_layer_rcgrad_job.py in.npz out.npz

torch opens the GPU first (it cannot in a process whose GPU the library opened before it), the layer's solver borrows torch's stream.
The linear loss  sum gJT J_T + sum gX X + sum gU U  through lq_mpc_amd.torch_layer.MPCLayer.rollout:
  * with Q, R, P, lb, ub, x_ref, u_ref given as CPU tensors that require a gradient: the seven gradients, and the same from the NumPy
    interface on the tape the NumPy interface leaves (rollout_cost_grad_batch, reduced and per instance);
  * the layer's own forward at the seven moved by +-STEP along the seeded direction: the per-instance loss and the tapes;
  * with none of the seven given, and with all seven given as the layer's own data: the outputs and the five older gradients of both;
  * behind 100 large matrix products that keep the stream busy, a forward under given data and a backward into x0, A and B, with an
    event recorded in front of them and queried behind them: it is still pending unless something waited for the host."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lq_mpc_amd.torch_layer import MPCLayer  # noqa: E402

SEVEN = ("Q", "R", "P", "lb", "ub", "x_ref", "u_ref")


def main(inp, outp):
    d = np.load(inp)
    N, T, STEP = int(d["N"]), int(d["T"]), float(d["STEP"])
    torch.cuda.init()
    ts = torch.cuda.Stream()
    out = {}
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    host = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy())
    with torch.cuda.stream(ts):
        gJ, gX, gU = dev(d["gJT"]), dev(d["gX"]), dev(d["gU"])

        def loss_of(J, X, U):
            return (gJ * J).sum() + (gX * X).sum() + (gU * U).sum()
        w = (d["Q"], d["R"], d["P"], d["lb"], d["ub"])
        # the layer is made with other weights and no references: what the call is given must be what counts
        layer = MPCLayer(N, d["A"], d["B"], 2.0 * d["Q"], d["R"], d["P"], d["lb"], d["ub"])
        bsz = d["x0"].shape[1]
        x, A, B = dev(d["x0"]), dev(d["A"]), dev(d["B"])
        At = dev(np.repeat(d["At"][:, :, None], bsz, axis=2))
        Bt = dev(np.repeat(d["Bt"][:, :, None], bsz, axis=2))
        seven = {k: host(d[k]).requires_grad_(True) for k in SEVEN}
        J, X, U = layer.rollout(x, T, At, Bt, A, B, **seven)
        loss_of(J, X, U).backward()
        ts.synchronize()
        out.update(J_T=J.detach().cpu().numpy(), X=X.detach().cpu().numpy(), U=U.detach().cpu().numpy())
        out.update({k + "_grad": v.grad.numpy().copy() for k, v in seven.items()})
        # the NumPy interface on the same data: the tape, the reduced and the per-instance gradients
        s = layer.solver
        refs = dict(x_ref=d["x_ref"], u_ref=d["u_ref"])
        g0 = s.rollout_tape_batch(T, N, d["A"], d["B"], *w, d["x0"], d["At"], d["Bt"], **refs)
        a = (T, N, d["A"], d["B"], *w, d["At"], d["Bt"], g0["X"], g0["U_tape"], g0["status_tape"], d["gJT"], d["gX"], d["gU"])
        red, per = s.rollout_cost_grad_batch(*a, reduce=True, **refs), s.rollout_cost_grad_batch(*a, **refs)
        out.update(np_X=g0["X"], np_U=g0["U"], np_J_T=g0["J_T"], np_U_tape=g0["U_tape"], np_status_tape=g0["status_tape"], skipped=red["skipped"])
        out.update({"red_" + k: red[k] for k in per})
        out.update({"per_" + k: per[k] for k in per})

        # the layer's own forward, the seven moved along the direction: the per-instance loss, and the tape of the same data
        def moved(sg):
            q = {k: np.ascontiguousarray(d[k] + sg * STEP * d["d_" + k]) for k in SEVEN}
            with torch.no_grad():
                Jm, Xm, Um = layer.rollout(x, T, At, Bt, A, B, **{k: host(v) for k, v in q.items()})
                L = gJ * Jm + (gX * Xm).sum(dim=(0, 1)) + (gU * Um).sum(dim=(0, 1))
            ts.synchronize()
            tape = s.rollout_tape_batch(T, N, d["A"], d["B"], *(q[k] for k in SEVEN[:5]), d["x0"], d["At"], d["Bt"], x_ref=q["x_ref"],
                                        u_ref=q["u_ref"])
            assert np.array_equal(tape["X"], Xm.cpu().numpy())
            return L.cpu().numpy(), tape["U_tape"]
        (Lp, tp), (Lm, tm) = moved(1.0), moved(-1.0)
        out.update(fd=(Lp - Lm) / (2 * STEP), tape_plus=tp, tape_minus=tm)

        # none of the seven given against all seven given as the layer's own data: the launches of before, and the same bits
        plain = MPCLayer(N, d["A"], d["B"], *w, **refs)
        grad = lambda *tensors: [t.detach().clone().requires_grad_(True) for t in tensors]
        for tag, kw in (("old", {}), ("new", {k: host(d[k]) for k in SEVEN})):
            v = grad(x, A, B, At, Bt)
            Jo, Xo, Uo = plain.rollout(v[0], T, v[3], v[4], v[1], v[2], **kw)
            loss_of(Jo, Xo, Uo).backward()
            ts.synchronize()
            out.update({f"{tag}_J_T": Jo.detach().cpu().numpy(), f"{tag}_X": Xo.detach().cpu().numpy(), f"{tag}_U": Uo.detach().cpu().numpy()})
            out.update({f"{tag}_grad{i}": t.grad.cpu().numpy() for i, t in enumerate(v)})
        ps = plain.solver
        gt = ps.rollout_tape_batch(T, N, d["A"], d["B"], *w, d["x0"], np.repeat(d["At"][:, :, None], bsz, axis=2),
                                   np.repeat(d["Bt"][:, :, None], bsz, axis=2), **refs)
        gg = ps.rollout_grad_batch(T, N, d["A"], d["B"], *w, np.repeat(d["At"][:, :, None], bsz, axis=2),
                                   np.repeat(d["Bt"][:, :, None], bsz, axis=2), gt["X"], gt["U_tape"], gt["status_tape"], d["gJT"], d["gX"],
                                   d["gU"], **refs)
        out.update(ref_X=gt["X"], ref_U=gt["U"], ref_J_T=gt["J_T"])
        out.update({f"ref_grad{i}": gg[k] for i, k in enumerate(("g_x0", "g_A", "g_B", "g_A_true", "g_B_true"))})
        plain.close()

        # no host synchronisation: the stream is kept busy, the event in front of the layer's work must still be pending behind it
        M = torch.randn((4096, 4096), dtype=torch.float64, device="cuda")
        v = grad(x, A, B)
        given = {k: host(d[k]) for k in SEVEN}
        ts.synchronize()
        for _ in range(100):
            M2 = M @ M
        ev = torch.cuda.Event()
        ev.record(ts)
        t0 = time.perf_counter()
        J, X, U = layer.rollout(v[0], T, At, Bt, v[1], v[2], **given)
        loss_of(J, X, U).backward()
        out["host_seconds"] = time.perf_counter() - t0
        out["event_pending"] = not ev.query()
        ts.synchronize()
        out.update(busy_X=X.detach().cpu().numpy(), busy_x_grad=v[0].grad.cpu().numpy())
        del M2
        layer.close()
    np.savez(outp, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
