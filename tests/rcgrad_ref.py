"""Shared by tests/test_rcgrad_cpu.py, tests/test_gpu_rcgrad.py and tests/torch_layer_rcgrad_job.py (not a test module).

The gradient of a loss on the closed loop of T steps (tests/rgrad_ref.py) with respect to the data the batch shares -- the weights
Q, R, P, the references x_ref, u_ref and the box lb, ub -- per instance, every step on the face its plan reports (DESIGN.md section
4.15).  With gJT = d loss / d J_T (Bsz,), gX = d loss / d X (nx, T + 1, Bsz), gU = d loss / d U (nu, T, Bsz):

      l_T = gX_T + 2 gJT Q x_T;   t = T-1 .. 0:   w_t = gU_t + 2 gJT R u_t + B_true'l_{t+1}
          the seven cost gradients of step t (tests/cgrad_ref.py) for gu0 = w_t, gVN = 0, and gx_t, the g_x0 of the model gradient
          every output += its step-t term,   l_t = gX_t + 2 gJT Q x_t + A_true'l_{t+1} + gx_t
      the direct part (the one Q and R also weigh J_T):  g_Q += gJT sum_{t=0}^{T} x_t x_t',  g_R += gJT sum_{t=0}^{T-1} u_t u_t'

  reference()   long double: per step the dense cgrad_ref.reference on the certified face of slice t at x_t with w = w_t, gam = 0, and
                grad_ref.reference for gx_t; the recursion of l and the direct part in long double.  No Riccati sweep anywhere.
  adjoint()     the numpy restatement of what lqmpc_rollout_cost_grad_kernel computes (fp64; long double on request): per step the
                plan's states re-rolled on the model from x_t and the slice, then cgrad_ref.adjoint and grad_ref.adjoint for gx_t.
  loop_loss()   long double: sum gU.u + sum gX.x + gJT J_T of the closed loop with every step's face held fixed, for any Q, R, P, lb,
                ub, x_ref, u_ref; an entry on a bound moves with that bound.  What the central differences differentiate.
  lds_bytes()   the LDS image of lqmpc_rollout_cost_grad_kernel (csrc/lqmpc_rcgrad.hip: rcgrad_lds), restated.
"""
import numpy as np

import cgrad_ref as cg
import grad_ref as gr
import rgrad_ref as rg
import sens_ref as sr
from oracle import exact as ex

LD = np.longdouble
KEYS = cg.KEYS
NAMES = tuple(k for k, _ in KEYS)
LDS_LIMIT = 160 * 1024
CASES = rg.CASES
# the share of the instances a test may leave out because the face a slice reports bit for bit is not the certified one
LEFT_OUT_CAP = 0.01
# the worst error of the fp64 adjoint() against reference() over CASES, relative to max(|ref|_max, 1) per instance and output, rounded
# up (tests/test_rcgrad_cpu.py measures it and holds it to this figure); the GPU tests' bar is 100 times it
CPU_WORST = 3.0e-14
GPU_BAR = 100 * CPU_WORST


def _zeros(nx, nu, N, Bsz, dtype):
    return {k: np.zeros(s + (Bsz,), dtype=dtype) for k, s in cg.sizes(nx, nu, N).items()}


def _direct(gam, x):
    """gam x x' per instance: x (n, Bsz) -> (n, n, Bsz)"""
    return gam * x[:, None, :] * x[None, :, :]


def reference(p, kw, At, Bt, X, U_tape, gJT, gX, gU):
    """Long double: the seven outputs of KEYS (instance axis last), 'free' and 'side' (T, nu, N, Bsz) the certified face of every
    slice, 'ok' (T, Bsz) the certificates, 'w' (T, nu, Bsz) the cotangent every step's u_0 received"""
    T, nu, N, Bsz = U_tape.shape
    nx = X.shape[0]
    Ql, Rl = np.asarray(p["Q"], dtype=LD), np.asarray(p["R"], dtype=LD)
    Atl, Btl = rg._per_instance(At, Bsz, LD), rg._per_instance(Bt, Bsz, LD)
    Xl = np.asarray(X, dtype=LD)
    gam = np.zeros(Bsz, dtype=LD) if gJT is None else np.asarray(gJT, dtype=LD)
    gXl = np.zeros((nx, T + 1, Bsz), dtype=LD) if gX is None else np.asarray(gX, dtype=LD)
    gUl = np.zeros((nu, T, Bsz), dtype=LD) if gU is None else np.asarray(gU, dtype=LD)
    lam = gXl[:, T] + 2 * gam * (Ql @ Xl[:, T])
    out = _zeros(nx, nu, N, Bsz, LD)
    out["g_Q"] = out["g_Q"] + _direct(gam, Xl[:, T])
    free, side = np.zeros(U_tape.shape, dtype=bool), np.zeros(U_tape.shape, dtype=int)
    ok, ws = np.zeros((T, Bsz), dtype=bool), np.zeros((T, nu, Bsz), dtype=LD)
    zero = np.zeros(Bsz)
    for t in range(T - 1, -1, -1):
        u = np.asarray(U_tape[t][:, 0], dtype=LD)
        w = gUl[:, t] + 2 * gam * (Rl @ u) + np.einsum("bik,ib->kb", Btl, lam)
        xt = np.ascontiguousarray(X[:, t])
        c = cg.reference(p, kw, xt, U_tape[t], w, zero)
        m = gr.reference(p, kw, xt, U_tape[t], w, zero)
        free[t], side[t], ok[t], ws[t] = c["free"], c["side"], c["ok"] & m["ok"], w
        for k in NAMES:
            out[k] = out[k] + c[k]
        out["g_Q"] = out["g_Q"] + _direct(gam, Xl[:, t])
        out["g_R"] = out["g_R"] + _direct(gam, u)
        lam = gXl[:, t] + 2 * gam * (Ql @ Xl[:, t]) + np.einsum("bij,ib->jb", Atl, lam) + m["g_x0"]
    out.update(free=free, side=side, ok=ok, w=ws)
    return out


def adjoint(N, A, B, Q, R, P, At, Bt, side, X, U_tape, gJT, gX, gU, x_ref=None, u_ref=None, dtype=np.float64, chol=False,
            stats=None):
    """numpy, the algebra of lqmpc_rollout_cost_grad_kernel: side (T, nu, N, Bsz) the faces (-1 lower, +1 upper, 0 free), X
    (nx, T + 1, Bsz), U_tape (T, nu, N, Bsz).  Returns the seven outputs of KEYS and 'w' (T, nu, Bsz).  dtype, chol, stats: see
    sens_ref.stage_solver."""
    cast = lambda a: np.asarray(a, dtype=dtype)
    T, nu, _, Bsz = U_tape.shape
    nx = X.shape[0]
    Ac, Bc, Qc, Rc, Xc = cast(A), cast(B), cast(Q), cast(R), cast(X)
    Atb, Btb = rg._per_instance(At, Bsz, dtype), rg._per_instance(Bt, Bsz, dtype)
    gam = np.zeros(Bsz, dtype=dtype) if gJT is None else cast(gJT)
    gXc = np.zeros((nx, T + 1, Bsz), dtype=dtype) if gX is None else cast(gX)
    gUc = np.zeros((nu, T, Bsz), dtype=dtype) if gU is None else cast(gU)
    lam = gXc[:, T] + 2 * gam * (Qc @ Xc[:, T])
    out = _zeros(nx, nu, N, Bsz, dtype)
    out["g_Q"] = out["g_Q"] + _direct(gam, Xc[:, T])
    ws = np.zeros((T, nu, Bsz), dtype=dtype)
    zero = np.zeros(Bsz, dtype=dtype)
    for t in range(T - 1, -1, -1):
        Up = cast(U_tape[t])
        u = Up[:, 0]
        w = gUc[:, t] + 2 * gam * (Rc @ u) + np.einsum("bik,ib->kb", Btb, lam)
        ws[t] = w
        Xp = np.zeros((nx, N + 1, Bsz), dtype=dtype)
        Xp[:, 0] = Xc[:, t]
        for i in range(N):
            Xp[:, i + 1] = np.einsum("acb,cb->ab", Ac, Xp[:, i]) + np.einsum("akb,kb->ab", Bc, Up[:, i])
        c = cg.adjoint(N, A, B, Q, R, P, side[t], Xp, Up, w, zero, x_ref, u_ref, dtype=dtype, chol=chol, stats=stats)
        m = gr.adjoint(N, A, B, Q, R, P, side[t] == 0, Xp, Up, w, zero, x_ref, dtype=dtype, chol=chol, stats=stats)
        for k in NAMES:
            out[k] = out[k] + c[k]
        out["g_Q"] = out["g_Q"] + _direct(gam, Xc[:, t])
        out["g_R"] = out["g_R"] + _direct(gam, u)
        lam = gXc[:, t] + 2 * gam * (Qc @ Xc[:, t]) + np.einsum("bij,ib->jb", Atb, lam) + m["g_x0"]
    out["w"] = ws
    return out


def tape_sides(U_tape, lb, ub):
    """(T, nu, N, Bsz) int: the face every slice reports bit for bit (cgrad_ref.side_bits)"""
    return np.stack([cg.side_bits(U, lb, ub) for U in U_tape])


def loop_loss(p, kw, At, Bt, x0, side, gJT, gX, gU, **over):
    """(Bsz,) long double: sum_t gU_t'u_t + sum_t gX_t'x_t + gJT J_T of the closed loop from x0 in which step t plays the optimum of
    the face side[t] (nu, N, Bsz; -1 held at lb, +1 held at ub, 0 free), with any of Q, R, P, lb, ub, x_ref, u_ref overridden (long
    double allowed).  A held entry sits on the overridden bound; the overridden Q and R also weigh J_T."""
    T, nu, N, Bsz = side.shape
    get = lambda k: over[k] if k in over else p[k]
    xr = over["x_ref"] if "x_ref" in over else kw.get("x_ref")
    ur = over["u_ref"] if "u_ref" in over else kw.get("u_ref")
    Ql, Rl = np.asarray(get("Q"), dtype=LD), np.asarray(get("R"), dtype=LD)
    lb, ub = np.asarray(get("lb"), dtype=LD)[:, None, None], np.asarray(get("ub"), dtype=LD)[:, None, None]
    Atl, Btl = rg._per_instance(At, Bsz, LD), rg._per_instance(Bt, Bsz, LD)
    x = np.asarray(x0, dtype=LD)
    gam, gXl, gUl = np.asarray(gJT, dtype=LD), np.asarray(gX, dtype=LD), np.asarray(gU, dtype=LD)
    J = np.einsum("ab,ac,cb->b", x, Ql, x)
    loss = np.einsum("ab,ab->b", gXl[:, 0], x)
    for t in range(T):
        H, g, _ = ex.condense(N, p["A"], p["B"], get("Q"), get("R"), get("P"), x, xr, ur)
        Ff = gr._time_major(side[t] == 0)
        Ub = np.asarray(gr._time_major(np.where(side[t] < 0, lb, np.where(side[t] > 0, ub, LD(0)))), dtype=LD)
        U = Ub.copy()
        faces, which = np.unique(Ff, axis=0, return_inverse=True)      # the instances of one face are solved together
        for m, face in enumerate(faces):
            F, Ac, rows = np.flatnonzero(face), np.flatnonzero(~face), np.flatnonzero(which.reshape(-1) == m)
            if F.size:
                Hr = H[rows]
                rhs = g[rows][:, F] + np.einsum("bij,bj->bi", Hr[:, F][:, :, Ac], Ub[rows][:, Ac])
                U[np.ix_(rows, F)] = -ex.chol_solve(ex.cholesky(Hr[:, F][:, :, F]), rhs)
        u = U[:, :nu].T                                                # (nu, Bsz)
        x = (np.einsum("bij,jb->bi", Atl, x) + np.einsum("bik,kb->bi", Btl, u)).T
        J = J + np.einsum("ab,ac,cb->b", x, Ql, x) + np.einsum("kb,kl,lb->b", u, Rl, u)
        loss = loss + np.einsum("kb,kb->b", gUl[:, t], u) + np.einsum("ab,ab->b", gXl[:, t + 1], x)
    return loss + gam * J


def n_sums(nx, nu, N):
    """M: the number of sums an instance carries"""
    return 2 * nx * nx + nu * nu + N * (nx + nu) + 2 * nu


def lds_bytes(nx, nu, N):
    """bytes of dynamic LDS a workgroup of lqmpc_rollout_cost_grad_kernel asks for: Q, R, P once and four instances, each with its
    image of the M sums and the count of instances left out (csrc/lqmpc_rcgrad.hip)"""
    ld = nx | 1
    shared = 2 * nx * nx + nu * nu
    sweep = max(3 * nx * ld + nx * nu + nu * ld, (N + 1) * nx + N * nu)      # S, T, C, W, G share their room with xt, ut
    inst = (2 * nx * ld + 2 * nx * nu + sweep + nu * nu + 4 * nu + 5 * nx + N * nu * nx + (N + 1) * nx + N * nu + n_sums(nx, nu, N) + 1)
    return 8 * (shared + 4 * inst)


def refused_shapes():
    """every shape within the build limits of include/lqmpc.h whose image is over the limit"""
    return [(nx, nu, N) for nx in range(1, 17) for nu in range(1, 9) for N in range(1, 65)
            if nu * N <= 128 and lds_bytes(nx, nu, N) > LDS_LIMIT]


def largest_admitted():
    """the shape within the build limits with the largest image the limit admits"""
    fits = [(lds_bytes(nx, nu, N), nx, nu, N) for nx in range(1, 17) for nu in range(1, 9) for N in range(1, 65)
            if nu * N <= 128 and lds_bytes(nx, nu, N) <= LDS_LIMIT]
    return max(fits)[1:]
