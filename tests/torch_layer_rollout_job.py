"""Child process of tests/test_gpu_torch_layer_rollout.py (not a test module).

    python tests/torch_layer_rollout_job.py in.npz out.npz

torch opens the GPU first (it cannot in a process whose GPU the library opened before it), the layer's solver borrows torch's stream.
One forward and backward of the linear loss  sum gJT J_T + sum gX X + sum gU U  through lq_mpc_amd.torch_layer.MPCLayer.rollout with
x0, the model and a plant shared by the batch given as tensors that require a gradient; the same loop from the NumPy interface
(rollout_tape_batch on the layer's solver), which also hands out the tape the reference needs; the layer's own model
(layer.rollout(x0, T, A_true, B_true)) with a per-instance plant; the per-instance loss of the NumPy loop at the data moved by
+-STEP along the seeded direction; then, behind 100 large matrix products that keep the stream busy, a forward and a backward with
an event recorded in front of them and queried behind them: it is still pending unless something waited for the host."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lq_mpc_amd.torch_layer import MPCLayer  # noqa: E402


def main(inp, outp):
    d = np.load(inp)
    N, T, STEP = int(d["N"]), int(d["T"]), float(d["STEP"])
    torch.cuda.init()
    ts = torch.cuda.Stream()
    out = {}
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    with torch.cuda.stream(ts):
        gJ, gX, gU = dev(d["gJT"]), dev(d["gX"]), dev(d["gU"])

        def loss_of(J, X, U):
            return (gJ * J).sum() + (gX * X).sum() + (gU * U).sum()
        w = (d["Q"], d["R"], d["P"], d["lb"], d["ub"])
        layer = MPCLayer(N, d["A"], d["B"], *w)
        grad = lambda *names: [dev(d[k]).requires_grad_(True) for k in names]
        x, A, B, At, Bt = grad("x0", "A", "B", "At", "Bt")
        J, X, U = layer.rollout(x, T, At, Bt, A, B)
        loss_of(J, X, U).backward()
        ts.synchronize()
        out.update(J_T=J.detach().cpu().numpy(), X=X.detach().cpu().numpy(), U=U.detach().cpu().numpy(), x_grad=x.grad.cpu().numpy(),
                   A_grad=A.grad.cpu().numpy(), B_grad=B.grad.cpu().numpy(), At_grad=At.grad.cpu().numpy(), Bt_grad=Bt.grad.cpu().numpy())
        # the layer's own model, a per-instance plant
        x1 = dev(d["x0"]).requires_grad_(True)
        At1 = dev(np.repeat(d["At"][:, :, None], x1.shape[1], axis=2)).requires_grad_(True)
        Bt1 = dev(np.repeat(d["Bt"][:, :, None], x1.shape[1], axis=2)).requires_grad_(True)
        J1, X1, U1 = layer.rollout(x1, T, At1, Bt1)
        loss_of(J1, X1, U1).backward()
        ts.synchronize()
        out.update(own_X=X1.detach().cpu().numpy(), own_x_grad=x1.grad.cpu().numpy(), own_At_grad=At1.grad.cpu().numpy(),
                   own_Bt_grad=Bt1.grad.cpu().numpy())
        # the NumPy interface: the tape, and the per-instance loss at the data moved along the direction
        s = layer.solver

        def tape(sg):
            q = {k: np.ascontiguousarray(d[k] + sg * STEP * d["d_" + k]) for k in ("A", "B", "x0", "At", "Bt")}
            g = s.rollout_tape_batch(T, N, q["A"], q["B"], *w, q["x0"], q["At"], q["Bt"])
            L = d["gJT"] * g["J_T"] + np.sum(d["gX"] * g["X"], axis=(0, 1)) + np.sum(d["gU"] * g["U"], axis=(0, 1))
            return g, L
        g0, _ = tape(0.0)
        (gp, Lp), (gm, Lm) = tape(1.0), tape(-1.0)
        out.update(np_X=g0["X"], np_U=g0["U"], np_J_T=g0["J_T"], np_U_tape=g0["U_tape"], np_status_tape=g0["status_tape"],
                   fd=(Lp - Lm) / (2 * STEP), tape_plus=gp["U_tape"], tape_minus=gm["U_tape"], kernel=s.last_kernel())
        # no host synchronisation: the stream is kept busy, the event in front of the layer's work must still be pending behind it
        M = torch.randn((4096, 4096), dtype=torch.float64, device="cuda")
        x2, A2, B2, At2, Bt2 = grad("x0", "A", "B", "At", "Bt")
        ts.synchronize()
        for _ in range(100):
            M2 = M @ M
        ev = torch.cuda.Event()
        ev.record(ts)
        t0 = time.perf_counter()
        J, X, U = layer.rollout(x2, T, At2, Bt2, A2, B2)
        loss_of(J, X, U).backward()
        out["host_seconds"] = time.perf_counter() - t0
        out["event_pending"] = not ev.query()
        ts.synchronize()
        out.update(A_grad_again=A2.grad.cpu().numpy(), x_grad_again=x2.grad.cpu().numpy())
        del M2
        layer.close()
    np.savez(outp, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
