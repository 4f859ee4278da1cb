"""Shared by tests/test_loopgrad_hard_cpu.py and tests/test_gpu_loopgrad_hard.py (not a test module): the three newer post-pass kernels
-- lqmpc_plan_grad_kernel (pgrad), lqmpc_rollout_grad_kernel (rgrad), lqmpc_rollout_cost_grad_kernel (rcgrad) -- on the hard models of
tests/qp_hard.py (CASE_LIST as it stands: the same problems, seeds and instance counts), the closed loop on the plant qp_hard.plant(p),
T = qp_hard.T_ROLL steps.  Cotangents: pgrad_ref.cotangents and rgrad_ref.cotangents with the seed sum(shape); gam and gJT are exactly 0
on every third instance.  The rules are those of tests/postpass_hard.py (DESIGN.md sections 4.6b and 4.6c).

Each kernel takes a plan, or a tape of plans; on these models the plan of an fp64 solve carries an error that the gradient amplifies, so
a test must keep the solve's error out of the comparison.  Two references do:

  (A) an independent formulation at the referee's data, status 0: pgrad_ref.reference at postpass_hard.referee_plan(p); rgrad_ref.reference
      and rcgrad_ref.reference at the referee's tape (referee_tape): X[:, t] the states of the referee's own closed loop rounded to fp64,
      U_tape[t] the referee's plan at that rounded state, rounded (an entry on a bound is the bound's bits), X[:, T] the rounded last
      state.  Dense long-double formulas, no Riccati sweep.  The kernels take the plan or the tape as arguments: no GPU solve is involved.
      Why the referee's tape and not the fp64 oracle's: the dense references certify every slice and stand on the exact optimum of its
      face, not on the slice, so on an fp64 tape they carry the solve's error (up to 4.7e3 x 2^-64 cond_2(H_b)), and on near_degenerate an
      fp64 slice may show another face than the certified one.
  (B) the same operation in long double on what the kernel read: pgrad_ref.adjoint, rgrad_ref.adjoint and rcgrad_ref.adjoint with
      dtype = LD on the very plan or tape and the face read off it bit for bit (cgrad_ref.side_bits).  For all three kernels behind real
      solves and rollouts; no instance is ever left out.  What licenses it: tests/test_loopgrad_hard_cpu.py holds the long-double
      restatements to the dense references at the referee's plan or tape of every case (A) serves, on every output, within
      LICENCE cond_2(H_b).

Bars, per instance b and output: bar_b = max(floor, c eps cond_2(H_b)), eps = 2^-52, errors by sens_ref.rel_err (relative to
max(|ref|_max, 1)).  floor: what the kernel is held to on easy problems (FLOOR).  c = C[reference][kernel][output]: postpass_hard.derive
of the worst ratio err_b / (eps cond_2(H_b)) of the fp64 restatement that factors as the kernels do (dtype = float64, chol = True)
against that reference, over the instances with cond_2(H_b) >= qp_hard.HARD_COND of every case the reference serves: 16 x the worst,
rounded up to a power of two.  For (A) at the referee's plan or tape, for (B) at the fp64 oracle's (oracle_plan, oracle_tape).
tests/test_loopgrad_hard_cpu.py recomputes the ratios and asserts that the table below is exactly that rule's result; no constant
comes from a GPU run."""
import numpy as np

import cgrad_ref as cg
import pgrad_ref as pg
import postpass_hard as ph
import qp_hard as qh
import rcgrad_ref as rc
import rgrad_ref as rg
import sens_ref as sr

LD = np.longdouble
EPS = qh.EPS
T = qh.T_ROLL
KERNELS = {"pgrad": pg.KEYS, "rgrad": rg.KEYS, "rcgrad": rc.KEYS}
AXES = {kernel: dict(keys) for kernel, keys in KERNELS.items()}
# tests/test_gpu_pgrad.py: BAR; tests/rgrad_ref.py and tests/rcgrad_ref.py: GPU_BAR
FLOOR = dict(pgrad=7.0e-12, rgrad=rg.GPU_BAR, rcgrad=rc.GPU_BAR)
LICENCE = ph.LICENCE
derive = ph.derive

# c[reference][kernel][output]: derive() of the worst ratios tests/test_loopgrad_hard_cpu.py measures (its docstring has the ratios)
C = {
    "A": dict(pgrad=dict(g_A=8.0, g_B=8.0, g_x0=8.0),
              rgrad=dict(g_A=16.0, g_B=4.0, g_x0=16.0, g_A_true=4.0, g_B_true=4.0),
              rcgrad=dict(g_Q=2.0, g_R=4.0, g_P=0.5, g_lb=4.0, g_ub=2.0, g_xref=8.0, g_uref=4.0)),
    "B": dict(pgrad=dict(g_A=8.0, g_B=8.0, g_x0=8.0),
              rgrad=dict(g_A=8.0, g_B=8.0, g_x0=16.0, g_A_true=4.0, g_B_true=8.0),
              rcgrad=dict(g_Q=2.0, g_R=4.0, g_P=0.5, g_lb=4.0, g_ub=2.0, g_xref=128.0, g_uref=16.0)),
}

# The cases reference (A) does not serve, per kernel, each with its reason; reference (B) serves every case.
_DENSE_TOO_DEAR = ("the dense per-step references condense a 120-variable QP in long double fifteen times a case: minutes of CPU; "
                   "reference (B) serves the shape")
A_UNSERVED = {
    "pgrad": {c: "the dense references stand on the face the rounded plan has on 11 of 13 instances only (tests/postpass_hard.py)"
              for c in ph.A_UNSERVED},
    "rgrad": {c: _DENSE_TOO_DEAR for c in qh.CASE_LIST if c[1] == (8, 4, 30)},
    "rcgrad": {c: _DENSE_TOO_DEAR for c in qh.CASE_LIST if c[1] == (8, 4, 30)},
}
A_CASES = {kernel: [c for c in qh.CASE_LIST if c not in A_UNSERVED[kernel]] for kernel in KERNELS}


def bar(which, kernel, output, cond):
    """per instance: max(floor, c eps cond_2(H_b))"""
    return np.maximum(FLOOR[kernel], C[which][kernel][output] * EPS * np.asarray(cond, dtype=float))


def plan_cotangents(p):
    """w (nu, N, Bsz), s (nx, N + 1, Bsz), gam (Bsz,), gam exactly 0 on every third instance"""
    nx, nu, N = p["shape"]
    return pg.cotangents(nx, nu, N, p["x0"].shape[1], sum(p["shape"]))


def loop_cotangents(p):
    """gJT (Bsz,), gX (nx, T + 1, Bsz), gU (nu, T, Bsz), gJT exactly 0 on every third instance"""
    nx, nu, _ = p["shape"]
    return rg.cotangents(nx, nu, T, p["x0"].shape[1], sum(p["shape"]))


def tape_of(X, U_tape, p):
    """a tape as the kernels take it, with the face every slice has bit for bit"""
    X, U_tape = np.ascontiguousarray(X), np.ascontiguousarray(U_tape)
    return dict(X=X, U_tape=U_tape, side=rc.tape_sides(U_tape, p["lb"], p["ub"]))


def referee_tape(p):
    """(A)'s input for the closed loop: the states of the referee's own trajectory and its plan at each, rounded to fp64; 'certified'
    (T, nu, N, Bsz) the face the referee certified at every step, 'ok' (T, Bsz) its certificates"""
    def f():
        nx, nu, N = p["shape"]
        Bsz = p["x0"].shape[1]
        steps = qh.exact_steps(p)
        X, Ut = np.zeros((nx, T + 1, Bsz)), np.zeros((T, nu, N, Bsz))
        for t, (x, e) in enumerate(steps):
            X[:, t], Ut[t] = x, np.asarray(e["U"], dtype=np.float64)
        X[:, T] = np.asarray(qh.exact_roll(p)["X"][:, T], dtype=np.float64)
        out = tape_of(X, Ut, p)
        out.update(certified=np.stack([cg.side_of(e["U"], p["lb"], p["ub"]) for _, e in steps]), ok=np.stack([e["ok"] for _, e in steps]))
        return out
    return qh._memo("loopgrad-referee-tape", p, f)


def oracle_tape(p):
    """(B)'s input on the CPU: the loop of rgrad_ref.oracle_tape with the fp64 oracle's plan at every step (qp_hard.oracle_plan) and
    rgrad_ref.plant_step on qp_hard.plant(p)"""
    def f():
        nx, nu, N = p["shape"]
        Bsz = p["x0"].shape[1]
        At, Bt = qh.plant(p)
        X, Ut = np.zeros((nx, T + 1, Bsz)), np.zeros((T, nu, N, Bsz))
        X[:, 0] = p["x0"]
        for t in range(T):
            Ut[t] = qh.oracle_plan(p, np.ascontiguousarray(X[:, t]))[0]
            X[:, t + 1] = rg.plant_step(At, Bt, X[:, t], Ut[t][:, 0])
        return tape_of(X, Ut, p)
    return qh._memo("loopgrad-oracle-tape", p, f)


def restate_plan(p, U, X, side, dtype=np.float64, chol=True, stats=None):
    """pgrad_ref.adjoint on the plan U (nu, N, Bsz), X (nx, N + 1, Bsz) and the face side (nu, N, Bsz) under plan_cotangents(p).
    dtype = float64, chol = True: the kernel's algebra and factorisation; dtype = LD: reference (B)."""
    m = (p["N"], p["A"], p["B"], p["Q"], p["R"], p["P"])
    return pg.adjoint(*m, side == 0, X, U, *plan_cotangents(p), qh.refs(p)[0], dtype=dtype, chol=chol, stats=stats)


def restate_loop(kernel, p, tape, dtype=np.float64, chol=True, stats=None):
    """rgrad_ref.adjoint or rcgrad_ref.adjoint on a tape (X, U_tape, side) under loop_cotangents(p) on the plant qp_hard.plant(p)"""
    m = (p["N"], p["A"], p["B"], p["Q"], p["R"], p["P"], *qh.plant(p))
    xr, ur = qh.refs(p)
    if kernel == "rgrad":
        return rg.adjoint(*m, tape["side"] == 0, tape["X"], tape["U_tape"], *loop_cotangents(p), xr, dtype=dtype, chol=chol, stats=stats)
    return rc.adjoint(*m, tape["side"], tape["X"], tape["U_tape"], *loop_cotangents(p), xr, ur, dtype=dtype, chol=chol, stats=stats)


def dense(kernel, p):
    """Reference (A) of a kernel: the dense long-double formulas at the referee's plan or tape, every output, with 'side' the face the
    reference certified (of every slice, for the closed loop) and 'ok' its certificates"""
    def f():
        if kernel == "pgrad":
            r = pg.reference(p, p["kw"], p["x0"], ph.referee_plan(p)["U"], *plan_cotangents(p))
            face = r["free"]
        else:
            rt = referee_tape(p)
            ref = rg.reference if kernel == "rgrad" else rc.reference
            r = ref(p, p["kw"], *qh.plant(p), rt["X"], rt["U_tape"], *loop_cotangents(p))
            face = r["free"]
        out = {k: r[k] for k, _ in KERNELS[kernel]}
        out.update(free=face, ok=r["ok"])
        return out
    return qh._memo("loopgrad-dense-" + kernel, p, f)


def errors(kernel, got, ref):
    """{output: per-instance sens_ref.rel_err}; a non-finite error counts as infinite"""
    out = {}
    for k, ax in KERNELS[kernel]:
        e = sr.rel_err(got[k], ref[k], ax)
        out[k] = np.where(np.isfinite(e), e, np.inf)
    return out


def step_kinds(side):
    """of a face tape (T, nu, N, Bsz): per (t, b), stage 0 wholly on bounds / all free (bool arrays (T, Bsz)); a mixed face is neither"""
    free = side == 0
    return ~free[:, :, 0].any(axis=1), free.all(axis=(1, 2))
