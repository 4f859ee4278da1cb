"""Child process of tests/test_gpu_torch_layer_plan.py (not a test module).

    python tests/torch_layer_plan_job.py in.npz out.npz

torch opens the GPU first (it cannot in a process whose GPU the library opened before it), the layer's solver borrows torch's stream.
One forward and backward of  loss = ((Uplan - U_e) ** 2).sum() + ((Xplan[:, 1:] - X_e) ** 2).sum() + 0.1 * VN.sum()  through
lq_mpc_amd.torch_layer.MPCLayer.plan with the models given as tensors that require a gradient, layer.plan(x, A, B); the same
derivatives from the NumPy interface (step(want_plan=True) and plan_grad on a controller of the layer's solver) for the matching
cotangents; layer.plan(x) without models; a backward behind an intervening set_model, which must raise; then, behind 100 large matrix
products that keep the stream busy, a forward and a backward with an event recorded in front of them and queried behind them: it is
still pending unless something waited for the host."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lq_mpc_amd import BatchController  # noqa: E402
from lq_mpc_amd.torch_layer import MPCLayer  # noqa: E402


def main(inp, outp):
    d = np.load(inp)
    N = int(d["N"])
    torch.cuda.init()
    ts = torch.cuda.Stream()
    out = {}
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    with torch.cuda.stream(ts):
        U_e, X_e = dev(d["U_e"]), dev(d["X_e"])

        def loss_of(Up, Xp, VN):
            return ((Up - U_e) ** 2).sum() + ((Xp[:, 1:] - X_e) ** 2).sum() + 0.1 * VN.sum()
        w = (d["Q"], d["R"], d["P"], d["lb"], d["ub"])
        # the layer starts from other models: plan(x, A, B) has to put the right ones in place
        layer = MPCLayer(N, 0.5 * d["A"], 0.5 * d["B"], *w)
        x, A, B = dev(d["x0"]).requires_grad_(True), dev(d["A"]).requires_grad_(True), dev(d["B"]).requires_grad_(True)
        Up, Xp, VN = layer.plan(x, A, B)
        loss_of(Up, Xp, VN).backward()
        ts.synchronize()
        out.update(U_plan=Up.detach().cpu().numpy(), X_plan=Xp.detach().cpu().numpy(), V_N=VN.detach().cpu().numpy(),
                   x_grad=x.grad.cpu().numpy(), A_grad=A.grad.cpu().numpy(), B_grad=B.grad.cpu().numpy(), kernel=layer.controller.kernel)
        # without models: the controller keeps those of the call before
        x1 = dev(d["x0"]).requires_grad_(True)
        Up1, Xp1, VN1 = layer.plan(x1)
        loss_of(Up1, Xp1, VN1).backward()
        ts.synchronize()
        out.update(plain_U_plan=Up1.detach().cpu().numpy(), plain_x_grad=x1.grad.cpu().numpy())
        # the NumPy interface
        with BatchController(layer.solver, N, d["A"], d["B"], *w) as ctl:
            g = ctl.step(d["x0"], want_plan=True)
            gX = np.zeros_like(g["X_plan"])
            gX[:, 1:] = 2.0 * (g["X_plan"][:, 1:] - d["X_e"])
            mg = ctl.plan_grad(g["U_plan"], g["X_plan"], g["status"], 2.0 * (g["U_plan"] - d["U_e"]), gX, np.full(g["V_N"].shape, 0.1))
        out.update(np_U_plan=g["U_plan"], np_status=g["status"], np_g_A=mg["g_A"], np_g_B=mg["g_B"], np_g_x0=mg["g_x0"])
        # a set_model between forward and backward
        x3, A3, B3 = x.detach().clone().requires_grad_(True), A.detach().clone().requires_grad_(True), B.detach().clone().requires_grad_(True)
        Up, Xp, VN = layer.plan(x3, A3, B3)
        layer.controller.set_model(A3.detach(), B3.detach())
        try:
            loss_of(Up, Xp, VN).backward()
            out.update(raised=False, raised_message="")
        except RuntimeError as e:
            out.update(raised=True, raised_message=str(e))
        # no host synchronisation: the stream is kept busy, the event in front of the layer's work must still be pending behind it
        M = torch.randn((4096, 4096), dtype=torch.float64, device="cuda")
        x2, A2, B2 = x.detach().clone().requires_grad_(True), A.detach().clone().requires_grad_(True), B.detach().clone().requires_grad_(True)
        ts.synchronize()
        for _ in range(100):
            M2 = M @ M
        ev = torch.cuda.Event()
        ev.record(ts)
        t0 = time.perf_counter()
        Up, Xp, VN = layer.plan(x2, A2, B2)
        loss_of(Up, Xp, VN).backward()
        out["host_seconds"] = time.perf_counter() - t0
        out["event_pending"] = not ev.query()
        ts.synchronize()
        out.update(A_grad_again=A2.grad.cpu().numpy(), B_grad_again=B2.grad.cpu().numpy(), x_grad_again=x2.grad.cpu().numpy())
        del M2
        layer.close()
    np.savez(outp, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
