"""Shared by tests/test_rgrad_cpu.py, tests/test_gpu_rgrad.py and tests/torch_layer_rollout_job.py (not a test module).

The closed loop of T steps -- the model (A, B) drives the QP, the plant (A_true, B_true) drives the state -- and the gradient of a loss
on it, given the cotangents gJT = d loss / d J_T (Bsz,), gX = d loss / d X (nx, T + 1, Bsz) and gU = d loss / d U (nu, T, Bsz), with
respect to the model, the plant and x_0 of every instance, every step on the face its plan reports:

      l_T = gX_T + 2 gJT Q x_T;   t = T-1 .. 0:   w_t = gU_t + 2 gJT R u_t + B_true'l_{t+1}
          (gA_t, gB_t, gx_t) = the model gradient of step t for gu0 = w_t, gVN = 0
          gA += gA_t, gB += gB_t, gA_true += l_{t+1} x_t', gB_true += l_{t+1} u_t',   l_t = gX_t + 2 gJT Q x_t + A_true'l_{t+1} + gx_t
      gx0 = l_0

  case()        the problem of sens_ref.case with the x0 scaling and the plant of this file, and the CPU oracle's own tape: computed
                once per case and never changed.
  oracle_tape() the loop with the CPU oracle's plan at every step, the plant step in fp64.
  reference()   long double: per step the dense grad_ref.reference on the certified face of slice t at x_t, the recursion of l in long
                double.  No Riccati sweep anywhere.
  adjoint()     the numpy restatement of what lqmpc_rollout_grad_kernel computes (fp64; long double on request): per step the plan's
                states re-rolled on the model from x_t and the slice, then grad_ref.adjoint (the masked sweep, one forward roll, one
                backward pass), and the same recursion.
  loop_loss()   long double: sum gU.u + sum gX.x + gJT J_T of the closed loop with every step's face held fixed, for any model, plant
                and x_0; what the central differences of tests/test_rgrad_cpu.py differentiate.
  cotangents()  seeded random gJT, gX, gU, gJT exactly 0 on every third instance.
  lds_bytes()   the LDS image of lqmpc_rollout_grad_kernel (csrc/lqmpc_rgrad.hip: rgrad_lds), restated.
"""
import numpy as np

import grad_ref as gr
import sens_ref as sr
from oracle import exact as ex

LD = np.longdouble
KEYS = (("g_A", (0, 1)), ("g_B", (0, 1)), ("g_x0", 0), ("g_A_true", (0, 1)), ("g_B_true", (0, 1)))
LDS_LIMIT = 160 * 1024

# x0 of sens_ref.case times this: chosen with the CPU oracle so that its own tape keeps the certified face bit for bit on at least
# 99 % of the instances and, at (4,2,10), each kind of step (stage 0 on a bound / a mixed face / all free) has at least 10 % of the
# (t, b) pairs (tests/test_rgrad_cpu.py asserts both)
X0_SCALE = {(2, 1, 5): 1.0, (4, 2, 10): 1.0, (3, 3, 4): 1.0, (2, 1, 1): 1.0, (8, 4, 30): 1.0, (16, 4, 8): 1.0}

# (shape, T, instances, how): the cases of tests/test_rgrad_cpu.py and tests/test_gpu_rgrad.py
CASES = [((2, 1, 5), 3, 203, {}), ((4, 2, 10), 6, 203, {}), ((3, 3, 4), 4, 203, {}), ((2, 1, 1), 1, 203, {}), ((2, 1, 1), 2, 203, {}),
         ((8, 4, 30), 3, 24, {}), ((16, 4, 8), 3, 203, {}), ((4, 2, 10), 6, 203, dict(refs=True, off_centre=True)),
         ((4, 2, 10), 6, 203, dict(per_instance=True))]
# the worst error of the fp64 adjoint() against reference() over CASES, relative to max(|ref|_max, 1) per instance, rounded up
# (tests/test_rgrad_cpu.py measures it and holds it to this figure); the GPU tests' bar is 100 times it
CPU_WORST = 1.0e-13
GPU_BAR = 100 * CPU_WORST


def cotangents(nx, nu, T, Bsz, seed):
    rng = np.random.default_rng(3000 + seed)
    gJT, gX, gU = rng.standard_normal(Bsz), rng.standard_normal((nx, T + 1, Bsz)), rng.standard_normal((nu, T, Bsz))
    gJT[::3] = 0.0
    return gJT, gX, gU


def plant(shape, Bsz, per_instance=False, seed=0):
    """a plant of spectral radius 0.9: one (nx, nx), (nx, nu) pair shared by the batch, or instance-minor arrays"""
    nx, nu, _ = shape
    rng = np.random.default_rng(500 + sum(shape) + seed)
    m = Bsz if per_instance else 1
    At = rng.standard_normal((nx, nx, m))
    At *= 0.9 / np.abs(np.linalg.eigvals(At.transpose(2, 0, 1))).max(axis=1)
    Bt = 0.6 * rng.standard_normal((nx, nu, m))
    if per_instance:
        return np.ascontiguousarray(At), np.ascontiguousarray(Bt)
    return np.ascontiguousarray(At[:, :, 0]), np.ascontiguousarray(Bt[:, :, 0])


def _per_instance(M, Bsz, dtype):
    """(r, c) or (r, c, Bsz) -> (Bsz, r, c)"""
    M = np.asarray(M, dtype=dtype)
    return np.broadcast_to(M, (Bsz,) + M.shape) if M.ndim == 2 else np.moveaxis(M, -1, 0)


def plant_step(At, Bt, x, u):
    """x_{t+1} = A_true x_t + B_true u_t in fp64, the sums in the order of the oracle: (nx, Bsz)"""
    Ab, Bb = _per_instance(At, x.shape[1], np.float64), _per_instance(Bt, x.shape[1], np.float64)
    return np.ascontiguousarray((np.einsum("bij,jb->bi", Ab, x) + np.einsum("bik,kb->bi", Bb, u)).T)


def oracle_tape(p, kw, x0, At, Bt, T):
    """{'X' (nx, T + 1, Bsz), 'U' (nu, T, Bsz), 'U_tape' (T, nu, N, Bsz), 'J_T' (Bsz,)} of the loop with the CPU oracle's plans"""
    nx, Bsz = x0.shape
    nu, N = p["B"].shape[1], p["N"]
    X, U, Ut = np.zeros((nx, T + 1, Bsz)), np.zeros((nu, T, Bsz)), np.zeros((T, nu, N, Bsz))
    X[:, 0] = x0
    J = np.einsum("ab,ac,cb->b", x0, p["Q"], x0)
    for t in range(T):
        Ut[t] = sr.oracle_plan(p, np.ascontiguousarray(X[:, t]), kw)
        U[:, t] = Ut[t][:, 0]
        X[:, t + 1] = plant_step(At, Bt, X[:, t], U[:, t])
        J = J + np.einsum("ab,ac,cb->b", X[:, t + 1], p["Q"], X[:, t + 1]) + np.einsum("kb,kl,lb->b", U[:, t], p["R"], U[:, t])
    return dict(X=X, U=U, U_tape=Ut, J_T=J)


_CASES = {}


def case(shape, T, refs=False, off_centre=False, bsz=sr.BSZ, per_instance=False):
    key = (shape, T, refs, off_centre, bsz, per_instance)
    if key not in _CASES:
        c = sr.case(shape, refs=refs, off_centre=off_centre, bsz=bsz)
        p = dict(c["p"])
        p["x0"] = np.ascontiguousarray(c["p"]["x0"] * X0_SCALE[shape])
        At, Bt = plant(shape, bsz, per_instance)
        tape = oracle_tape(p, c["kw"], p["x0"], At, Bt, T)
        for a in [p["x0"], At, Bt] + list(tape.values()):
            a.setflags(write=False)
        _CASES[key] = dict(shape=shape, T=T, p=p, kw=c["kw"], At=At, Bt=Bt, tape=tape)
    return _CASES[key]


def kinds(free):
    """of a face tape (T, nu, N, Bsz): the share of the (t, b) pairs with stage 0 wholly on bounds / a mixed face / all free"""
    sat = ~free[:, :, 0].any(axis=1)
    allfree = free.all(axis=(1, 2))
    return float(sat.mean()), float((~sat & ~allfree).mean()), float(allfree.mean())


def tape_faces(U_tape, lb, ub):
    """(T, nu, N, Bsz) bool: the face every slice reports bit for bit (sens_ref.face_bits)"""
    return np.stack([sr.face_bits(U, lb, ub) for U in U_tape])


def reference(p, kw, At, Bt, X, U_tape, gJT, gX, gU):
    """Long double: {'g_A', 'g_B', 'g_x0', 'g_A_true', 'g_B_true'} (instance axis last), 'free' (T, nu, N, Bsz) the certified face of
    every slice, 'ok' (T, Bsz) the certificates"""
    T, nu, N, Bsz = U_tape.shape
    nx = X.shape[0]
    Ql, Rl = np.asarray(p["Q"], dtype=LD), np.asarray(p["R"], dtype=LD)
    Atl, Btl = _per_instance(At, Bsz, LD), _per_instance(Bt, Bsz, LD)
    Xl = np.asarray(X, dtype=LD)
    gam = np.zeros(Bsz, dtype=LD) if gJT is None else np.asarray(gJT, dtype=LD)
    gXl = np.zeros((nx, T + 1, Bsz), dtype=LD) if gX is None else np.asarray(gX, dtype=LD)
    gUl = np.zeros((nu, T, Bsz), dtype=LD) if gU is None else np.asarray(gU, dtype=LD)
    lam = gXl[:, T] + 2 * gam * (Ql @ Xl[:, T])                                    # (nx, Bsz)
    gA, gB = np.zeros((nx, nx, Bsz), dtype=LD), np.zeros((nx, nu, Bsz), dtype=LD)
    gAt, gBt = np.zeros((nx, nx, Bsz), dtype=LD), np.zeros((nx, nu, Bsz), dtype=LD)
    free, ok = np.zeros(U_tape.shape, dtype=bool), np.zeros((T, Bsz), dtype=bool)
    zero = np.zeros(Bsz)
    for t in range(T - 1, -1, -1):
        u = np.asarray(U_tape[t][:, 0], dtype=LD)
        w = gUl[:, t] + 2 * gam * (Rl @ u) + np.einsum("bik,ib->kb", Btl, lam)
        r = gr.reference(p, kw, np.ascontiguousarray(X[:, t]), U_tape[t], w, zero)
        free[t], ok[t] = r["free"], r["ok"]
        gA, gB = gA + r["g_A"], gB + r["g_B"]
        gAt, gBt = gAt + lam[:, None, :] * Xl[:, t][None, :, :], gBt + lam[:, None, :] * u[None, :, :]
        lam = gXl[:, t] + 2 * gam * (Ql @ Xl[:, t]) + np.einsum("bij,ib->jb", Atl, lam) + r["g_x0"]
    return dict(g_A=gA, g_B=gB, g_x0=lam, g_A_true=gAt, g_B_true=gBt, free=free, ok=ok)


def adjoint(N, A, B, Q, R, P, At, Bt, free, X, U_tape, gJT, gX, gU, x_ref=None, dtype=np.float64, chol=False, stats=None):
    """numpy, the algebra of lqmpc_rollout_grad_kernel: free (T, nu, N, Bsz) the faces, X (nx, T + 1, Bsz), U_tape (T, nu, N, Bsz).
    Returns {'g_A', 'g_B', 'g_x0', 'g_A_true', 'g_B_true'}.  dtype, chol, stats: see sens_ref.stage_solver."""
    cast = lambda a: np.asarray(a, dtype=dtype)
    T, nu, _, Bsz = U_tape.shape
    nx = X.shape[0]
    Ac, Bc, Qc, Rc, Xc = cast(A), cast(B), cast(Q), cast(R), cast(X)
    Atb, Btb = _per_instance(At, Bsz, dtype), _per_instance(Bt, Bsz, dtype)
    gam = np.zeros(Bsz, dtype=dtype) if gJT is None else cast(gJT)
    gXc = np.zeros((nx, T + 1, Bsz), dtype=dtype) if gX is None else cast(gX)
    gUc = np.zeros((nu, T, Bsz), dtype=dtype) if gU is None else cast(gU)
    lam = gXc[:, T] + 2 * gam * (Qc @ Xc[:, T])
    gA, gB = np.zeros((nx, nx, Bsz), dtype=dtype), np.zeros((nx, nu, Bsz), dtype=dtype)
    gAt, gBt = np.zeros((nx, nx, Bsz), dtype=dtype), np.zeros((nx, nu, Bsz), dtype=dtype)
    zero = np.zeros(Bsz, dtype=dtype)
    for t in range(T - 1, -1, -1):
        Up = cast(U_tape[t])
        u = Up[:, 0]
        w = gUc[:, t] + 2 * gam * (Rc @ u) + np.einsum("bik,ib->kb", Btb, lam)
        Xp = np.zeros((nx, N + 1, Bsz), dtype=dtype)
        Xp[:, 0] = Xc[:, t]
        for i in range(N):
            Xp[:, i + 1] = np.einsum("acb,cb->ab", Ac, Xp[:, i]) + np.einsum("akb,kb->ab", Bc, Up[:, i])
        g = gr.adjoint(N, A, B, Q, R, P, free[t], Xp, Up, w, zero, x_ref, dtype=dtype, chol=chol, stats=stats)
        gA, gB = gA + g["g_A"], gB + g["g_B"]
        gAt, gBt = gAt + lam[:, None, :] * Xc[:, t][None, :, :], gBt + lam[:, None, :] * u[None, :, :]
        lam = gXc[:, t] + 2 * gam * (Qc @ Xc[:, t]) + np.einsum("bij,ib->jb", Atb, lam) + g["g_x0"]
    return dict(g_A=gA, g_B=gB, g_x0=lam, g_A_true=gAt, g_B_true=gBt)


def loop_loss(p, kw, At, Bt, x0, free, U_bound, gJT, gX, gU, A=None, B=None):
    """(Bsz,) long double: sum_t gU_t'u_t + sum_t gX_t'x_t + gJT J_T of the closed loop from x0 in which step t plays the optimum of
    the face free[t] (nu, N, Bsz), the other entries held at U_bound[t]; model A, B (default: p's), plant At, Bt and x0 may be long
    double"""
    A, B = p["A"] if A is None else A, p["B"] if B is None else B
    T, nu, N, Bsz = free.shape
    Ql, Rl = np.asarray(p["Q"], dtype=LD), np.asarray(p["R"], dtype=LD)
    Atl, Btl = _per_instance(At, Bsz, LD), _per_instance(Bt, Bsz, LD)
    x = np.asarray(x0, dtype=LD)
    gam, gXl, gUl = np.asarray(gJT, dtype=LD), np.asarray(gX, dtype=LD), np.asarray(gU, dtype=LD)
    J = np.einsum("ab,ac,cb->b", x, Ql, x)
    loss = np.einsum("ab,ab->b", gXl[:, 0], x)
    for t in range(T):
        H, g, _ = ex.condense(N, A, B, p["Q"], p["R"], p["P"], x, kw.get("x_ref"), kw.get("u_ref"))
        Ff, Ub = gr._time_major(free[t]), np.asarray(gr._time_major(U_bound[t]), dtype=LD)
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


def lds_bytes(nx, nu, N):
    """bytes of dynamic LDS a workgroup of lqmpc_rollout_grad_kernel asks for: Q, R, P once and four instances (csrc/lqmpc_rgrad.hip)"""
    ld = nx | 1
    shared = 2 * nx * nx + nu * nu
    inst = 5 * nx * ld + nx * nx + 4 * nx * nu + nu * ld + nu * nu + 4 * nu + 7 * nx + N * nu * nx + 2 * (N + 1) * nx + 2 * N * nu
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
