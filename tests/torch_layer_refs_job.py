"""Child process of tests/test_gpu_torch_layer_refs.py (not a test module).

    python tests/torch_layer_refs_job.py in.npz out.npz

torch opens the GPU first (it cannot in a process whose GPU the library opened before it), the layer's solver borrows torch's stream.
One forward and backward of  loss = sum_b m_b (|u_0|^2 + 0.1 V_N)_b  (m the 0 / 1 mask of the input file) through
lq_mpc_amd.torch_layer.MPCLayer with the references given as CPU tensors that require a gradient, layer(x, x_ref=, u_ref=), on a
layer made without references; the same derivatives from the NumPy interface (step(want_sens=True) and cost_grad, reduced and per
instance, on a controller of the layer's solver given these references the same way); the same through layer(x, A, B, x_ref=, u_ref=); and a
backward behind an intervening set_reference, which must raise."""
import os
import sys

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
    host = lambda a: torch.from_numpy(np.array(a, dtype=np.float64)).requires_grad_(True)
    with torch.cuda.stream(ts):
        w = (d["Q"], d["R"], d["P"], d["lb"], d["ub"])
        m = dev(d["mask"])
        loss_of = lambda u0, VN: ((u0 ** 2).sum(dim=0) * m).sum() + 0.1 * (VN * m).sum()
        # the layer starts without references: forward has to put them in place
        layer = MPCLayer(N, d["A"], d["B"], *w)
        x, xr, ur = dev(d["x0"]).requires_grad_(True), host(d["x_ref"]), host(d["u_ref"])
        u0, VN = layer(x, x_ref=xr, u_ref=ur)
        loss_of(u0, VN).backward()
        ts.synchronize()
        out.update(u_0=u0.detach().cpu().numpy(), V_N=VN.detach().cpu().numpy(), x_grad=x.grad.cpu().numpy(),
                   xref_grad=xr.grad.numpy(), uref_grad=ur.grad.numpy(), xref_grad_is_cpu=not xr.grad.is_cuda,
                   kernel=layer.controller.kernel)
        # the NumPy interface
        with BatchController(layer.solver, N, d["A"], d["B"], *w) as ctl:
            ctl.set_reference(d["x_ref"], d["u_ref"])                  # the layer's own path to these references
            g = ctl.step(d["x0"], want_sens=True)
            cot = (2.0 * d["mask"] * g["u_0"], 0.1 * d["mask"])
            red = ctl.cost_grad(g["U_plan"], g["X_plan"], g["status"], *cot, reduce=True)
            per = ctl.cost_grad(g["U_plan"], g["X_plan"], g["status"], *cot)
            mg = ctl.model_grad(g["U_plan"], g["X_plan"], g["status"], *cot)
        out.update(np_u_0=g["u_0"], np_status=g["status"], np_U_plan=g["U_plan"], np_g_xref=red["g_xref"], np_g_uref=red["g_uref"],
                   np_skipped=red["skipped"], per_g_xref=per["g_xref"], per_g_uref=per["g_uref"], np_g_A=mg["g_A"], np_g_B=mg["g_B"],
                   np_x_grad=np.einsum("kab,kb->ab", g["K_0"], cot[0]) + g["dV_dx"] * cot[1])
        # with the models as well
        x2, A2, B2, xr2, ur2 = dev(d["x0"]).requires_grad_(True), dev(d["A"]).requires_grad_(True), dev(d["B"]).requires_grad_(True), \
            host(d["x_ref"]), host(d["u_ref"])
        u0, VN = layer(x2, A2, B2, x_ref=xr2, u_ref=ur2)
        loss_of(u0, VN).backward()
        ts.synchronize()
        out.update(both_xref_grad=xr2.grad.numpy(), both_uref_grad=ur2.grad.numpy(), both_A_grad=A2.grad.cpu().numpy(),
                   both_B_grad=B2.grad.cpu().numpy())
        # only one of the two references: the other is zero and gets no gradient
        x4, xr4 = dev(d["x0"]).requires_grad_(True), host(d["x_ref"])
        u0, VN = layer(x4, x_ref=xr4)
        loss_of(u0, VN).backward()
        out.update(only_xref_grad_shape=np.array(xr4.grad.shape))
        # a set_reference between forward and backward
        x3, xr3, ur3 = dev(d["x0"]).requires_grad_(True), host(d["x_ref"]), host(d["u_ref"])
        u0, VN = layer(x3, x_ref=xr3, u_ref=ur3)
        layer.controller.set_reference(d["x_ref"], d["u_ref"])
        try:
            loss_of(u0, VN).backward()
            out.update(raised=False, raised_message="")
        except RuntimeError as e:
            out.update(raised=True, raised_message=str(e))
        layer.close()
    np.savez(outp, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
