"""The batched MPC controller as a differentiable torch layer (the only module of the package that imports torch).

    layer = MPCLayer(N, A, B, Q, R, P, lb, ub)          # A (nx, nx, Bsz), B (nx, nu, Bsz): numpy arrays or fp64 device tensors
    u0, VN = layer(x)                                    # x (nx, Bsz) fp64 device tensor -> u0 (nu, Bsz), VN (Bsz,)
    loss(u0, VN).backward()                              # x.grad through the local feedback law and the value gradient
    u0, VN = layer(x, A, B)                              # A, B fp64 device tensors, possibly requires_grad: the layer's new model
    loss(u0, VN).backward()                              # x.grad, and A.grad, B.grad through the model of every instance
    u0, VN = layer(x, x_ref=xr, u_ref=ur)                # xr (nx, N), ur (nu, N) fp64 CPU tensors, possibly requires_grad: the new references
    loss(u0, VN).backward()                              # x.grad, and xr.grad, ur.grad summed over the batch (with A, B: theirs too)
    Uplan, Xplan, VN = layer.plan(x, A, B)               # the whole plan (nu, N, Bsz), its states (nx, N + 1, Bsz) and VN; A, B optional
    loss(Uplan, Xplan, VN).backward()                    # x.grad, A.grad, B.grad for a loss on every u_i, every x_i and V_N
    JT, X, U = layer.rollout(x0, T, A_true, B_true)      # the closed loop of T steps on the plant A_true, B_true; A, B optional
    loss(JT, X, U).backward()                            # x0.grad, A_true.grad, B_true.grad (with A, B: theirs too) through the whole loop
    JT, X, U = layer.rollout(x0, T, A_true, B_true, Q=Q, lb=lb)   # ... under weights, a box or references given as fp64 CPU tensors
    loss(JT, X, U).backward()                            # Q.grad, lb.grad (any of Q, R, P, lb, ub, x_ref, u_ref), summed over the batch

Forward is one lqmpc_controller_step_sens_dev on the tensors' own pointers: the QP of every instance, then the post-pass that returns
K_0 = d u_0 / d x and dV_N / d x on the face the plan ends on.  Backward is  grad_x = K_0' grad_u0 + dV_dx grad_VN, a torch einsum.
With A and B given, forward first replaces the controller's models in place (set_model, device flavour) and keeps the plan, its
states and the status; backward adds one lqmpc_controller_model_grad_dev (csrc/lqmpc_grad.hip: the adjoint LQ problem on the plan's
face), which returns grad_A and grad_B.  That call reads the controller's own copies of the models, so backward raises if any
set_model, through the layer or on layer.controller, came between the forward and its backward.
With x_ref or u_ref given, forward first makes them the controller's references (set_reference; they are shared by the batch and
host data, as everywhere in the library, so they are CPU tensors; one left out is zero); backward adds one
lqmpc_controller_cost_grad_dev with reduce (csrc/lqmpc_cgrad.hip), which sums the gradient with respect to the references over the
batch on the GPU, and copies the two small results to the host: that copy is the one wait for the host in the layer, and it happens
on this path only.  Backward raises if a set_reference or a set_model came between the forward and its backward.
layer.plan is one lqmpc_controller_step_plan_dev forward (behind set_model where A and B are given) and one
lqmpc_controller_plan_grad_dev backward (csrc/lqmpc_pgrad.hip), which returns grad_x and, where asked for, grad_A and grad_B: no einsum,
no K_plan, no wait for the host; backward raises behind an intervening set_model or set_reference in the same way.
The solver handle is created on torch's current stream (lqmpc_create_on_stream), so everything is ordered with the surrounding torch
work on that stream and, but for that copy, nothing waits for the host, in forward or in backward.  Use the layer under the stream it
was made under.

The law of a box-constrained MPC is piecewise affine: the gradient is that of the critical region x lies in, exact inside it and
one-sided on its border.  The model (A, B) is differentiated per instance and the references for the batch as a whole.  The weights
and the box are fixed when the controller is made, so the step does not differentiate them: their gradients are those of
BatchController.cost_grad and BatchSolver.cost_grad_batch.  layer.rollout runs on the batch calls, not on the controller, and takes
all seven with the call (its docstring).
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


class _MPCStepModel(torch.autograd.Function):
    """the step under new models A, B: differentiable in x, A and B"""

    @staticmethod
    def forward(ctx, x, A, B, ctl):
        nx, nu, N, Bsz = ctl.nx, ctl.nu, ctl.N, ctl.Bsz
        if x.dtype != torch.float64 or not x.is_cuda or tuple(x.shape) != (nx, Bsz):
            raise ValueError(f"x must be a float64 device tensor of shape ({nx}, {Bsz})")
        for M, shape in ((A, (nx, nx, Bsz)), (B, (nx, nu, Bsz))):
            if M.dtype != torch.float64 or not M.is_cuda or tuple(M.shape) != shape:
                raise ValueError(f"A and B must be float64 device tensors of shapes ({nx}, {nx}, {Bsz}) and ({nx}, {nu}, {Bsz})")
        x = x.detach().contiguous()
        ctl.set_model(A.detach().contiguous(), B.detach().contiguous())
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=x.device)
        u0, VN, K0, dV = new(nu, Bsz), new(Bsz), new(nu, nx, Bsz), new(nx, Bsz)
        Up, Xp, st = new(nu, N, Bsz), new(nx, N + 1, Bsz), torch.empty(Bsz, dtype=torch.int32, device=x.device)
        ctl.step_sens_dev(x, u0, K0, dV, dUplan=Up, dXplan=Xp, dVN=VN, dstatus=st)
        ctx.save_for_backward(K0, dV, Up, Xp, st)
        ctx.ctl, ctx.model_version = ctl, ctl.model_version
        return u0, VN

    @staticmethod
    def backward(ctx, grad_u0, grad_VN):
        K0, dV, Up, Xp, st = ctx.saved_tensors
        ctl = ctx.ctl
        if ctl.model_version != ctx.model_version:
            raise RuntimeError("MPCLayer: the controller's models were replaced (set_model) between this forward and its backward; "
                               "the gradient with respect to A and B would be that of another model")
        grad_x = None
        if grad_u0 is not None:
            grad_x = torch.einsum("kab,kb->ab", K0, grad_u0)
        if grad_VN is not None:
            g = dV * grad_VN.unsqueeze(0)
            grad_x = g if grad_x is None else grad_x + g
        grad_A = grad_B = None
        if (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]) and (grad_u0 is not None or grad_VN is not None):
            grad_A = torch.empty((ctl.nx, ctl.nx, ctl.Bsz), dtype=torch.float64, device=Xp.device)
            grad_B = torch.empty((ctl.nx, ctl.nu, ctl.Bsz), dtype=torch.float64, device=Xp.device)
            ctl.model_grad_dev(Up, Xp, grad_A, grad_B, dstatus=st,
                               dgu0=None if grad_u0 is None else grad_u0.contiguous(), dgVN=None if grad_VN is None else grad_VN.contiguous())
        return grad_x, grad_A, grad_B, None


class _MPCStepRefs(torch.autograd.Function):
    """the step under new references x_ref, u_ref (and, where given, new models A, B): differentiable in all of them and in x"""

    @staticmethod
    def forward(ctx, x, A, B, x_ref, u_ref, ctl):
        nx, nu, N, Bsz = ctl.nx, ctl.nu, ctl.N, ctl.Bsz
        if x.dtype != torch.float64 or not x.is_cuda or tuple(x.shape) != (nx, Bsz):
            raise ValueError(f"x must be a float64 device tensor of shape ({nx}, {Bsz})")
        for M, shape in ((x_ref, (nx, N)), (u_ref, (nu, N))):
            if M is not None and (M.dtype != torch.float64 or M.is_cuda or tuple(M.shape) != shape):
                raise ValueError(f"x_ref and u_ref must be float64 CPU tensors of shapes ({nx}, {N}) and ({nu}, {N})")
        if A is not None:
            for M, shape in ((A, (nx, nx, Bsz)), (B, (nx, nu, Bsz))):
                if M.dtype != torch.float64 or not M.is_cuda or tuple(M.shape) != shape:
                    raise ValueError(f"A and B must be float64 device tensors of shapes ({nx}, {nx}, {Bsz}) and ({nx}, {nu}, {Bsz})")
            ctl.set_model(A.detach().contiguous(), B.detach().contiguous())
        x = x.detach().contiguous()
        ctl.set_reference(None if x_ref is None else x_ref.detach().contiguous().numpy(),
                          None if u_ref is None else u_ref.detach().contiguous().numpy())
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=x.device)
        u0, VN, K0, dV = new(nu, Bsz), new(Bsz), new(nu, nx, Bsz), new(nx, Bsz)
        Up, Xp, st = new(nu, N, Bsz), new(nx, N + 1, Bsz), torch.empty(Bsz, dtype=torch.int32, device=x.device)
        ctl.step_sens_dev(x, u0, K0, dV, dUplan=Up, dXplan=Xp, dVN=VN, dstatus=st)
        ctx.save_for_backward(K0, dV, Up, Xp, st)
        ctx.ctl, ctx.model_version, ctx.reference_version = ctl, ctl.model_version, ctl.reference_version
        return u0, VN

    @staticmethod
    def backward(ctx, grad_u0, grad_VN):
        K0, dV, Up, Xp, st = ctx.saved_tensors
        ctl = ctx.ctl
        if ctl.reference_version != ctx.reference_version:
            raise RuntimeError("MPCLayer: the controller's references were replaced (set_reference) between this forward and its "
                               "backward; the gradient would be that of other references")
        if ctl.model_version != ctx.model_version:
            raise RuntimeError("MPCLayer: the controller's models were replaced (set_model) between this forward and its backward; "
                               "the gradient would be that of another model")
        grad_x = None
        if grad_u0 is not None:
            grad_x = torch.einsum("kab,kb->ab", K0, grad_u0)
        if grad_VN is not None:
            g = dV * grad_VN.unsqueeze(0)
            grad_x = g if grad_x is None else grad_x + g
        grad_A = grad_B = grad_xr = grad_ur = None
        if grad_u0 is None and grad_VN is None:
            return grad_x, None, None, None, None, None
        gu0 = None if grad_u0 is None else grad_u0.contiguous()
        gVN = None if grad_VN is None else grad_VN.contiguous()
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            grad_A = torch.empty((ctl.nx, ctl.nx, ctl.Bsz), dtype=torch.float64, device=Xp.device)
            grad_B = torch.empty((ctl.nx, ctl.nu, ctl.Bsz), dtype=torch.float64, device=Xp.device)
            ctl.model_grad_dev(Up, Xp, grad_A, grad_B, dstatus=st, dgu0=gu0, dgVN=gVN)
        if ctx.needs_input_grad[3] or ctx.needs_input_grad[4]:
            g_xr = torch.empty((ctl.nx, ctl.N), dtype=torch.float64, device=Xp.device)
            g_ur = torch.empty((ctl.nu, ctl.N), dtype=torch.float64, device=Xp.device)
            ctl.cost_grad_dev(Up, Xp, dict(g_xref=g_xr, g_uref=g_ur), dstatus=st, dgu0=gu0, dgVN=gVN, reduce=True)
            # the references live on the host: the one wait for the host in the layer
            grad_xr = g_xr.cpu() if ctx.needs_input_grad[3] else None
            grad_ur = g_ur.cpu() if ctx.needs_input_grad[4] else None
        return grad_x, grad_A, grad_B, grad_xr, grad_ur, None


class _MPCPlan(torch.autograd.Function):
    """the step returning its whole plan (and, where given, under new models A, B): differentiable in x, A and B"""

    @staticmethod
    def forward(ctx, x, A, B, ctl):
        nx, nu, N, Bsz = ctl.nx, ctl.nu, ctl.N, ctl.Bsz
        if x.dtype != torch.float64 or not x.is_cuda or tuple(x.shape) != (nx, Bsz):
            raise ValueError(f"x must be a float64 device tensor of shape ({nx}, {Bsz})")
        if A is not None:
            for M, shape in ((A, (nx, nx, Bsz)), (B, (nx, nu, Bsz))):
                if M.dtype != torch.float64 or not M.is_cuda or tuple(M.shape) != shape:
                    raise ValueError(f"A and B must be float64 device tensors of shapes ({nx}, {nx}, {Bsz}) and ({nx}, {nu}, {Bsz})")
            ctl.set_model(A.detach().contiguous(), B.detach().contiguous())
        x = x.detach().contiguous()
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=x.device)
        u0, VN, Up, Xp = new(nu, Bsz), new(Bsz), new(nu, N, Bsz), new(nx, N + 1, Bsz)
        st = torch.empty(Bsz, dtype=torch.int32, device=x.device)
        ctl.step_plan_dev(x, u0, Up, dXplan=Xp, dVN=VN, dstatus=st)
        ctx.save_for_backward(Up, Xp, st)
        ctx.ctl, ctx.model_version, ctx.reference_version = ctl, ctl.model_version, ctl.reference_version
        return Up, Xp, VN

    @staticmethod
    def backward(ctx, grad_U, grad_X, grad_VN):
        Up, Xp, st = ctx.saved_tensors
        ctl = ctx.ctl
        if ctl.model_version != ctx.model_version:
            raise RuntimeError("MPCLayer: the controller's models were replaced (set_model) between this forward and its backward; "
                               "the gradient would be that of another model")
        if ctl.reference_version != ctx.reference_version:
            raise RuntimeError("MPCLayer: the controller's references were replaced (set_reference) between this forward and its "
                               "backward; the gradient would be that of other references")
        if grad_U is None and grad_X is None and grad_VN is None:
            return None, None, None, None
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=Xp.device)
        grad_x = new(ctl.nx, ctl.Bsz)
        grad_A = new(ctl.nx, ctl.nx, ctl.Bsz) if ctx.needs_input_grad[1] else None
        grad_B = new(ctl.nx, ctl.nu, ctl.Bsz) if ctx.needs_input_grad[2] else None
        cot = [None if g is None else g.contiguous() for g in (grad_U, grad_X, grad_VN)]
        ctl.plan_grad_dev(Up, Xp, grad_A, grad_B, dstatus=st, dgUplan=cot[0], dgXplan=cot[1], dgVN=cot[2], dgx0=grad_x)
        return grad_x, grad_A, grad_B, None


class _MPCRollout(torch.autograd.Function):
    """the closed loop of T steps on a plant of its own: differentiable in x0, the model A, B and the plant A_true, B_true"""

    @staticmethod
    def forward(ctx, x0, A, B, At, Bt, layer, T):
        ctl = layer.controller
        nx, nu, N, Bsz = ctl.nx, ctl.nu, ctl.N, ctl.Bsz
        if x0.dtype != torch.float64 or not x0.is_cuda or tuple(x0.shape) != (nx, Bsz):
            raise ValueError(f"x0 must be a float64 device tensor of shape ({nx}, {Bsz})")
        for M, shape in ((A, (nx, nx, Bsz)), (B, (nx, nu, Bsz)), (At, (nx, nx, Bsz)), (Bt, (nx, nu, Bsz))):
            if M.dtype != torch.float64 or not M.is_cuda or tuple(M.shape) != shape:
                raise ValueError(f"the model and the plant must be float64 device tensors of shapes ({nx}, {nx}, {Bsz}) and ({nx}, {nu}, {Bsz})")
        x0, A, B, At, Bt = (M.detach().contiguous() for M in (x0, A, B, At, Bt))
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=x0.device)
        JT, X, U, Ut = new(Bsz), new(nx, T + 1, Bsz), new(nu, T, Bsz), new(T, nu, N, Bsz)
        st = torch.empty((T, Bsz), dtype=torch.int32, device=x0.device)
        layer.solver.rollout_tape_batch_dev(nx, nu, N, Bsz, T, A, B, *layer._shared, x0, At, Bt, JT, Ut, dX=X, dU=U, dstatus_tape=st,
                                            true_per_instance=True, **layer._refs)
        ctx.save_for_backward(A, B, At, Bt, X, Ut, st)
        ctx.layer, ctx.T = layer, T
        return JT, X, U

    @staticmethod
    def backward(ctx, grad_J, grad_X, grad_U):
        A, B, At, Bt, X, Ut, st = ctx.saved_tensors
        layer, T = ctx.layer, ctx.T
        if grad_J is None and grad_X is None and grad_U is None:
            return None, None, None, None, None, None, None
        ctl = layer.controller
        nx, nu, N, Bsz = ctl.nx, ctl.nu, ctl.N, ctl.Bsz
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=X.device)
        need = ctx.needs_input_grad
        g_x = new(nx, Bsz)
        g_A = new(nx, nx, Bsz) if need[1] else None
        g_B = new(nx, nu, Bsz) if need[2] else None
        g_At = new(nx, nx, Bsz) if need[3] else None
        g_Bt = new(nx, nu, Bsz) if need[4] else None
        cot = [None if g is None else g.contiguous() for g in (grad_J, grad_X, grad_U)]
        layer.solver.rollout_grad_batch_dev(nx, nu, N, Bsz, T, A, B, *layer._shared, At, Bt, X, Ut, dstatus_tape=st, dgJT=cot[0], dgX=cot[1],
                                            dgU=cot[2], dgA=g_A, dgB=g_B, dgx0=g_x, dgA_true=g_At, dgB_true=g_Bt, true_per_instance=True,
                                            **layer._refs)
        return g_x, g_A, g_B, g_At, g_Bt, None, None


class _MPCRolloutShared(torch.autograd.Function):
    """the closed loop under weights, a box or references given with the call: differentiable in them (summed over the batch) as well
    as in x0, the model and the plant"""

    KEYS = ("g_Q", "g_R", "g_P", "g_lb", "g_ub", "g_xref", "g_uref")

    @staticmethod
    def forward(ctx, x0, A, B, At, Bt, Q, R, P, lb, ub, x_ref, u_ref, layer, T):
        ctl = layer.controller
        nx, nu, N, Bsz = ctl.nx, ctl.nu, ctl.N, ctl.Bsz
        if x0.dtype != torch.float64 or not x0.is_cuda or tuple(x0.shape) != (nx, Bsz):
            raise ValueError(f"x0 must be a float64 device tensor of shape ({nx}, {Bsz})")
        for M, shape in ((A, (nx, nx, Bsz)), (B, (nx, nu, Bsz)), (At, (nx, nx, Bsz)), (Bt, (nx, nu, Bsz))):
            if M.dtype != torch.float64 or not M.is_cuda or tuple(M.shape) != shape:
                raise ValueError(f"the model and the plant must be float64 device tensors of shapes ({nx}, {nx}, {Bsz}) and ({nx}, {nu}, {Bsz})")
        given = (Q, R, P, lb, ub, x_ref, u_ref)
        shapes = ((nx, nx), (nu, nu), (nx, nx), (nu,), (nu,), (nx, N), (nu, N))
        for M, shape in zip(given, shapes):
            if M is not None and (M.dtype != torch.float64 or M.is_cuda or tuple(M.shape) != shape):
                raise ValueError("Q, R, P, lb, ub, x_ref and u_ref must be float64 CPU tensors of the shapes of the layer's own")
        own = layer._shared + (layer._refs["x_ref"], layer._refs["u_ref"])
        data = tuple(o if M is None else M.detach().contiguous().numpy().copy() for M, o in zip(given, own))
        shared, refs = data[:5], dict(x_ref=data[5], u_ref=data[6])
        x0, A, B, At, Bt = (M.detach().contiguous() for M in (x0, A, B, At, Bt))
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=x0.device)
        JT, X, U, Ut = new(Bsz), new(nx, T + 1, Bsz), new(nu, T, Bsz), new(T, nu, N, Bsz)
        st = torch.empty((T, Bsz), dtype=torch.int32, device=x0.device)
        layer.solver.rollout_tape_batch_dev(nx, nu, N, Bsz, T, A, B, *shared, x0, At, Bt, JT, Ut, dX=X, dU=U, dstatus_tape=st,
                                            true_per_instance=True, **refs)
        ctx.save_for_backward(A, B, At, Bt, X, Ut, st)
        ctx.layer, ctx.T, ctx.shared, ctx.refs, ctx.shapes = layer, T, shared, refs, shapes
        return JT, X, U

    @staticmethod
    def backward(ctx, grad_J, grad_X, grad_U):
        A, B, At, Bt, X, Ut, st = ctx.saved_tensors
        layer, T = ctx.layer, ctx.T
        none = (None,) * 14
        if grad_J is None and grad_X is None and grad_U is None:
            return none
        ctl = layer.controller
        nx, nu, N, Bsz = ctl.nx, ctl.nu, ctl.N, ctl.Bsz
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=X.device)
        need = ctx.needs_input_grad
        cot = [None if g is None else g.contiguous() for g in (grad_J, grad_X, grad_U)]
        g_x = g_A = g_B = g_At = g_Bt = None
        if any(need[:5]):
            g_x = new(nx, Bsz)
            g_A = new(nx, nx, Bsz) if need[1] else None
            g_B = new(nx, nu, Bsz) if need[2] else None
            g_At = new(nx, nx, Bsz) if need[3] else None
            g_Bt = new(nx, nu, Bsz) if need[4] else None
            layer.solver.rollout_grad_batch_dev(nx, nu, N, Bsz, T, A, B, *ctx.shared, At, Bt, X, Ut, dstatus_tape=st, dgJT=cot[0],
                                                dgX=cot[1], dgU=cot[2], dgA=g_A, dgB=g_B, dgx0=g_x, dgA_true=g_At, dgB_true=g_Bt,
                                                true_per_instance=True, **ctx.refs)
        g_shared = [None] * 7
        if any(need[5:12]):
            outs = {k: new(*shape) for k, shape, n in zip(_MPCRolloutShared.KEYS, ctx.shapes, need[5:12]) if n}
            layer.solver.rollout_cost_grad_batch_dev(nx, nu, N, Bsz, T, A, B, *ctx.shared, At, Bt, X, Ut, outs, dstatus_tape=st, dgJT=cot[0],
                                                     dgX=cot[1], dgU=cot[2], true_per_instance=True, reduce=True, **ctx.refs)
            # the shared data live on the host: the one wait for the host on this path
            g_shared = [outs[k].cpu() if k in outs else None for k in _MPCRolloutShared.KEYS]
        return (g_x, g_A, g_B, g_At, g_Bt, *g_shared, None, None)


class MPCLayer(torch.nn.Module):
    """u0, VN = MPCLayer(N, A, B, Q, R, P, lb, ub)(x) around a BatchController; options are the solver's (BatchSolver.set_options).
    layer(x, A, B) steps under the models A, B (they become the controller's) and is differentiable in them as well;
    layer(x, x_ref=xr, u_ref=ur), with or without A and B, steps under the references xr, ur (CPU tensors; they become the
    controller's, one left out is zero) and is differentiable in them, summed over the batch."""

    def __init__(self, N, A, B, Q, R, P, lb, ub, x_ref=None, u_ref=None, **options):
        super().__init__()
        stream = torch.cuda.current_stream()
        self.solver = BatchSolver(stream.device_index, stream=stream.cuda_stream, **options)
        if not hasattr(A, "data_ptr"):
            A, B = np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(B, dtype=np.float64)
        self.controller = BatchController(self.solver, N, A, B, Q, R, P, lb, ub, x_ref, u_ref)
        # what rollout() passes to the batch calls: the data the layer was made with (the model goes to the device on first use)
        self._model0 = (A, B)
        self._shared = tuple(np.ascontiguousarray(M, dtype=np.float64) for M in (Q, R, P, lb, ub))
        self._refs = dict(x_ref=x_ref, u_ref=u_ref)

    def rollout(self, x0, T, A_true, B_true, A=None, B=None, *, Q=None, R=None, P=None, lb=None, ub=None, x_ref=None, u_ref=None):
        """J_T (Bsz,), X (nx, T + 1, Bsz), U (nu, T, Bsz) of the closed loop of T steps from x0 (nx, Bsz): the model drives every QP
        -- A, B where given, else those the layer was made with -- and the plant A_true, B_true drives the state: (nx, nx), (nx, nu)
        shared by the batch or (nx, nx, Bsz), (nx, nu, Bsz).  Differentiable in x0, A, B, A_true and B_true for a loss on all three
        outputs.  Forward is one lqmpc_rollout_tape_batch_dev (T plan calls with a plant step behind each: not the fast rollout),
        backward one lqmpc_rollout_grad_batch_dev (csrc/lqmpc_rgrad.hip) on the tape it left; a shared plant is expanded over the
        batch in torch, so its gradient is summed by autograd.  Nothing waits for the host.
        Any of Q, R, P, lb, ub, x_ref, u_ref may be given as a float64 CPU tensor (the data the batch shares are host data, as
        everywhere in the library): the loop then runs under them for this call, one left out is the layer's own, and one that
        requires grad gets the gradient summed over the batch, from one lqmpc_rollout_cost_grad_batch_dev with reduce
        (csrc/lqmpc_rcgrad.hip) and a copy of the small results to the host, the one wait for the host on this path.  Q and R weigh
        J_T as well as the QP, and their gradients hold both parts.  Q.grad, R.grad and P.grad take the entries of the matrix as
        independent: a caller who parametrises a symmetric Q gets <Q.grad, dQ> through autograd, and nothing is symmetrised on their
        behalf.  With none of the seven given the call runs exactly the launches it ran before they could be."""
        if (A is None) != (B is None):
            raise ValueError("give both A and B, or neither")
        ctl = self.controller
        if A is None:
            if not hasattr(self._model0[0], "data_ptr"):
                self._model0 = tuple(torch.from_numpy(M).to(x0.device) for M in self._model0)
            A, B = self._model0
        plant = []
        for M in (A_true, B_true):
            M = M.to(x0.device)
            plant.append(M.unsqueeze(-1).expand(*M.shape, ctl.Bsz) if M.dim() == 2 else M)
        if all(M is None for M in (Q, R, P, lb, ub, x_ref, u_ref)):
            return _MPCRollout.apply(x0, A, B, plant[0], plant[1], self, int(T))
        return _MPCRolloutShared.apply(x0, A, B, plant[0], plant[1], Q, R, P, lb, ub, x_ref, u_ref, self, int(T))

    def forward(self, x, A=None, B=None, *, x_ref=None, u_ref=None):
        if (A is None) != (B is None):
            raise ValueError("give both A and B, or neither")
        if x_ref is not None or u_ref is not None:
            return _MPCStepRefs.apply(x, A, B, x_ref, u_ref, self.controller)
        if A is None:
            return _MPCStep.apply(x, self.controller)
        return _MPCStepModel.apply(x, A, B, self.controller)

    def plan(self, x, A=None, B=None):
        """Uplan (nu, N, Bsz), Xplan (nx, N + 1, Bsz), VN (Bsz,) of one step at x, under the models A, B where given (they become the
        controller's, as in forward).  Differentiable in x, A and B for a loss on all three: backward is one
        lqmpc_controller_plan_grad_dev on the face the plan ends on."""
        if (A is None) != (B is None):
            raise ValueError("give both A and B, or neither")
        return _MPCPlan.apply(x, A, B, self.controller)

    def close(self):
        self.controller.close()
        self.solver.close()
