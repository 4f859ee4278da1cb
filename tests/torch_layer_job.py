"""Child process of tests/test_gpu_torch_layer.py (not a test module).

    python tests/torch_layer_job.py in.npz out.npz

torch opens the GPU first (it cannot in a process whose GPU the library opened before it), the layer's solver borrows torch's stream.
One forward and backward of  loss = (u_0 ** 2).sum() + 0.1 * V_N.sum()  through lq_mpc_amd.torch_layer.MPCLayer; the same derivatives
from the NumPy interface (BatchController.step(want_sens=True) on a second controller of the layer's solver); then, behind 100 large
matrix products that keep the stream busy, two forwards and one backward with an event recorded in front of them and queried behind
them: it is still pending unless something waited for the host."""
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
    with torch.cuda.stream(ts):
        layer = MPCLayer(N, d["A"], d["B"], d["Q"], d["R"], d["P"], d["lb"], d["ub"])
        x = torch.from_numpy(np.ascontiguousarray(d["x0"])).cuda().requires_grad_(True)
        u0, VN = layer(x)
        loss = (u0 ** 2).sum() + 0.1 * VN.sum()
        loss.backward()
        ts.synchronize()
        out.update(u_0=u0.detach().cpu().numpy(), V_N=VN.detach().cpu().numpy(), x_grad=x.grad.cpu().numpy(), kernel=layer.controller.kernel)
        with BatchController(layer.solver, N, d["A"], d["B"], d["Q"], d["R"], d["P"], d["lb"], d["ub"]) as ctl:
            g = ctl.step(d["x0"], want_sens=True)
        out.update(np_u_0=g["u_0"], np_K_0=g["K_0"], np_dV_dx=g["dV_dx"], np_status=g["status"])
        # no host synchronisation: the stream is kept busy, the event in front of the layer's work must still be pending behind it
        M = torch.randn((4096, 4096), dtype=torch.float64, device="cuda")
        x2 = x.detach().clone().requires_grad_(True)
        ts.synchronize()
        for _ in range(100):
            M2 = M @ M
        ev = torch.cuda.Event()
        ev.record(ts)
        t0 = time.perf_counter()
        layer(x2)
        u0, VN = layer(x2)
        ((u0 ** 2).sum() + 0.1 * VN.sum()).backward()
        out["host_seconds"] = time.perf_counter() - t0
        out["event_pending"] = not ev.query()
        ts.synchronize()
        out["x_grad_again"] = x2.grad.cpu().numpy()
        del M2
        layer.close()
    np.savez(outp, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
