"""Child process of tests/test_gpu_controller.py::test_closed_loop_around_a_torch_plant (not a test module).

    python tests/controller_loop_job.py in.npz out.npz

torch opens the GPU first, the solver borrows torch's stream; T step_dev calls with the plant computed in torch between them,
everything enqueued on that one stream and nothing waited for until the loop is over.  Records every (x_t, u_t, V_t, status_t)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lq_mpc_amd import BatchController, BatchSolver  # noqa: E402


def main(inp, outp):
    d = np.load(inp)
    T = int(d["T"])
    nx, nu, Bsz = d["B"].shape
    torch.cuda.init()
    ts = torch.cuda.Stream()
    s = BatchSolver(0, stream=ts.cuda_stream)
    out = {}
    with torch.cuda.stream(ts):
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        dA, dB = dev(d["A"]), dev(d["B"])
        ts.synchronize()
        with BatchController(s, int(d["N"]), dA, dB, d["Q"], d["R"], d["P"], d["lb"], d["ub"]) as ctl:
            out["kernel"] = ctl.kernel
            for tag in ("nl", "lin"):
                if tag == "nl":
                    At, Bt, W = dev(d["A_true"]), dev(d["B_true"]), dev(d["W"])
                else:
                    At, Bt = dev(d["A"][:, :, 0]), dev(d["B"][:, :, 0])
                X = torch.empty((T + 1, nx, Bsz), dtype=torch.float64, device="cuda")
                U = torch.empty((T, nu, Bsz), dtype=torch.float64, device="cuda")
                V = torch.empty((T, Bsz), dtype=torch.float64, device="cuda")
                S = torch.empty((T, Bsz), dtype=torch.int32, device="cuda")
                X[0] = dev(d["x0"])
                ctl.reset()
                for t in range(T):
                    ctl.step_dev(X[t], U[t], V[t], S[t])
                    if tag == "nl":
                        X[t + 1] = (torch.einsum("ijb,jb->ib", At, X[t]) + torch.einsum("ikb,kb->ib", Bt, U[t])
                                    + 0.2 * torch.sin(X[t]) + W[t])
                    else:
                        X[t + 1] = At @ X[t] + Bt @ U[t]
                ts.synchronize()
                for k, v in (("X", X), ("U", U), ("V", V), ("S", S)):
                    out[f"{k}_{tag}"] = v.cpu().numpy()
    s.close()
    np.savez(outp, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
