"""The batched MPC controller as a differentiable torch layer (the only module of the package that imports torch).

    layer = MPCLayer(N, A, B, Q, R, P, lb, ub)          # A (nx, nx, Bsz), B (nx, nu, Bsz): numpy arrays or fp64 device tensors
    u0, VN = layer(x)                                    # x (nx, Bsz) fp64 device tensor -> u0 (nu, Bsz), VN (Bsz,)
    loss(u0, VN).backward()                              # x.grad through the local feedback law and the value gradient

Forward is one lqmpc_controller_step_sens_dev on the tensors' own pointers: the QP of every instance, then the post-pass that returns
K_0 = d u_0 / d x and dV_N / d x on the face the plan ends on.  Backward is  grad_x = K_0' grad_u0 + dV_dx grad_VN, a torch einsum.
The solver handle is created on torch's current stream (lqmpc_create_on_stream), so everything is ordered with the surrounding torch
work on that stream and nothing waits for the host, in forward or in backward.  Use the layer under the stream it was made under.

The law of a box-constrained MPC is piecewise affine: the gradient is that of the critical region x lies in, exact inside it and
one-sided on its border.  Parameters (A, B, weights, box, references) are data, not differentiated.
"""
import numpy as np
import torch

from .mpc import BatchController, BatchSolver


class _MPCStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ctl):
        if x.dtype != torch.float64 or not x.is_cuda or tuple(x.shape) != (ctl.nx, ctl.Bsz):
            raise ValueError(f"x must be a float64 device tensor of shape ({ctl.nx}, {ctl.Bsz})")
        x = x.detach().contiguous()
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=x.device)
        u0, VN, K0, dV = new(ctl.nu, ctl.Bsz), new(ctl.Bsz), new(ctl.nu, ctl.nx, ctl.Bsz), new(ctl.nx, ctl.Bsz)
        ctl.step_sens_dev(x, u0, K0, dV, dVN=VN)
        ctx.save_for_backward(K0, dV)
        return u0, VN

    @staticmethod
    def backward(ctx, grad_u0, grad_VN):
        K0, dV = ctx.saved_tensors
        grad_x = None
        if grad_u0 is not None:
            grad_x = torch.einsum("kab,kb->ab", K0, grad_u0)
        if grad_VN is not None:
            g = dV * grad_VN.unsqueeze(0)
            grad_x = g if grad_x is None else grad_x + g
        return grad_x, None


class MPCLayer(torch.nn.Module):
    """u0, VN = MPCLayer(N, A, B, Q, R, P, lb, ub)(x) around a BatchController; options are the solver's (BatchSolver.set_options)."""

    def __init__(self, N, A, B, Q, R, P, lb, ub, x_ref=None, u_ref=None, **options):
        super().__init__()
        stream = torch.cuda.current_stream()
        self.solver = BatchSolver(stream.device_index, stream=stream.cuda_stream, **options)
        if not hasattr(A, "data_ptr"):
            A, B = np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(B, dtype=np.float64)
        self.controller = BatchController(self.solver, N, A, B, Q, R, P, lb, ub, x_ref, u_ref)

    def forward(self, x):
        return _MPCStep.apply(x, self.controller)

    def close(self):
        self.controller.close()
        self.solver.close()
