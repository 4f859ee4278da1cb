"""Shared by tests/test_postpass_hard_cpu.py and tests/test_gpu_postpass_hard.py (not a test module): the three post-pass kernels --
lqmpc_sens_kernel, lqmpc_grad_kernel, lqmpc_cost_grad_kernel -- on the hard models of tests/qp_hard.py (CASE_LIST as it stands: the
same problems, seeds and instance counts), with the cotangents of grad_ref.cotangents, gam exactly 0 on every third instance.

A post-pass takes a plan; on these models the plan of an fp64 solve carries an error that the gradient amplifies (DESIGN.md section
4.6b), so a test must keep the solve's error out of the comparison.  Two references do:

  (A) an independent formulation at the referee's plan: the plan handed over is U* = qp_hard.exact_solve(p)["U"] rounded to fp64 (an
      entry on a bound is the bound's bits), X* the model rolled in long double and rounded, status 0 (referee_plan); the reference is
      the dense long-double grad_ref.reference / cgrad_ref.reference (no Riccati sweep), K_plan = -H_FF^-1 Fx[F] of sens_ref
      (dense_gain) and sens_ref.reference's dV_dx.  For model-grad and cost-grad, which take the plan as an argument.
  (B) the same operation in long double at the plan the kernel was given: restate(..., dtype=LD) runs sens_ref.masked_sweep,
      sens_ref.costate, grad_ref.adjoint and cgrad_ref.adjoint in long double (the stage matrices through exact.cholesky /
      exact.chol_solve) on the very U_plan, X_plan and bit-for-bit face the kernel read.  For all three kernels behind real solves and
      steps.  What licenses it: tests/test_postpass_hard_cpu.py holds the long-double restatements to the dense references at the
      referee's plan of every case, on every output, within LICENCE cond_2(H_b).

Bars, per instance b and output: bar_b = max(floor, c eps cond_2(H_b)), eps = 2^-52, errors by sens_ref.rel_err (relative to
max(|ref|_max, 1)).  floor: what the output is held to on easy problems (FLOOR).  c = C[reference][output]: 16 x the worst ratio
err_b / (eps cond_2(H_b)) of the fp64 restatement that factors as the kernels do (Cholesky, lower factor, reciprocal diagonal:
restate(..., dtype=float64, chol=True)) against that reference, over the instances with cond_2(H_b) >= qp_hard.HARD_COND of every
case, rounded up to a power of two.  For (A) the plan is the referee's, for (B) the fp64 oracle's (qp_hard.oracle_plan,
sens_ref.model_roll).  tests/test_postpass_hard_cpu.py recomputes the ratios and asserts that the table below is exactly that rule's
result; no constant comes from a GPU run."""
import numpy as np

import cgrad_ref as cg
import grad_ref as gr
import qp_hard as qh
import sens_ref as sr

LD = np.longdouble
EPS = qh.EPS
KERNELS = {
    "sens": (("K_plan", (0, 1, 2)), ("dV_dx", 0)),
    "grad": (("g_A", (0, 1)), ("g_B", (0, 1)), ("g_x0", 0)),
    "cgrad": cg.KEYS,
}
AXES = {k: ax for keys in KERNELS.values() for k, ax in keys}
KERNEL_OF = {k: name for name, keys in KERNELS.items() for k, _ in keys}
# tests/test_gpu_sens.py: BAR; tests/test_grad_cpu.py (100 x its worst, as tests/test_gpu_grad.py: BAR); tests/test_cgrad_cpu.py: GPU_BAR
FLOOR = dict(sens=1e-10, grad=5.8e-12, cgrad=1.7e-12)
# the long-double restatements against the dense references: 2^-64 (one rounding of a long double) x 2^10 x cond_2(H_b)
LICENCE = 2.0 ** -64 * 2.0 ** 10

# c[reference][output]: derive() of the worst ratios tests/test_postpass_hard_cpu.py measures (its docstring has the ratios themselves)
C = {
    "A": dict(K_plan=4.0, dV_dx=2.0 ** -4, g_A=2.0, g_B=4.0, g_x0=4.0, g_Q=0.25, g_R=4.0, g_P=2.0 ** -6, g_lb=2.0, g_ub=0.5, g_xref=4.0, g_uref=2.0),
    "B": dict(K_plan=4.0, dV_dx=2.0 ** -5, g_A=2.0, g_B=4.0, g_x0=4.0, g_Q=0.25, g_R=4.0, g_P=2.0 ** -6, g_lb=2.0, g_ub=0.5, g_xref=4.0, g_uref=2.0),
}

# The one (family, shape) reference (A) cannot serve: (instances whose rounded referee's plan has, bit for bit, the face the referee
# certified; instances on which the dense references, certifying that plan again, stand on the plan's bit-for-bit face; instances).
# tests/test_postpass_hard_cpu.py asserts the numbers and that no other case is short of either; its docstring has the distances.
A_UNSERVED = {("near_degenerate", (8, 4, 30)): (12, 11, 13)}
A_CASES = [c for c in qh.CASE_LIST if c not in A_UNSERVED]


def derive(worst_ratio):
    """the rule of the constants: 16 x the worst ratio, rounded up to a power of two"""
    return float(2.0 ** np.ceil(np.log2(16.0 * worst_ratio)))


def bar(which, output, cond):
    """per instance: max(floor, c eps cond_2(H_b))"""
    return np.maximum(FLOOR[KERNEL_OF[output]], C[which][output] * EPS * np.asarray(cond, dtype=float))


def cotangents(p):
    """w (nu, Bsz) and gam (Bsz,) of a problem, gam exactly 0 on every third instance (as tests/test_gpu_cgrad.py)"""
    w, gam = gr.cotangents(p["B"].shape[1], p["x0"].shape[1], sum(p["shape"]))
    gam[::3] = 0.0
    return w, gam


def referee_plan(p):
    """(A)'s input: U* rounded to fp64, X* the long-double roll rounded, and the face as the kernels read it bit for bit"""
    def f():
        e = qh.exact_solve(p)
        U = np.ascontiguousarray(np.asarray(e["U"], dtype=np.float64))
        X = np.ascontiguousarray(np.asarray(e["X"], dtype=np.float64))
        return dict(U=U, X=X, side=cg.side_bits(U, p["lb"], p["ub"]), certified=cg.side_of(e["U"], p["lb"], p["ub"]), ok=e["ok"])
    return qh._memo("postpass-referee-plan", p, f)


def oracle_plan(p):
    """(B)'s input on the CPU: the fp64 oracle's plan, the model rolled in fp64, the bit-for-bit face"""
    def f():
        U = np.ascontiguousarray(qh.oracle_plan(p, p["x0"])[0])
        return dict(U=U, X=sr.model_roll(p, p["x0"], U), side=cg.side_bits(U, p["lb"], p["ub"]))
    return qh._memo("postpass-oracle-plan", p, f)


def restate(p, U, X, side, w, gam, dtype=np.float64, chol=True, stats=None, kernels=("sens", "grad", "cgrad")):
    """The numpy restatements of the post-passes on the plan U (nu, N, Bsz), X (nx, N + 1, Bsz) and the face side (nu, N, Bsz): every
    output of `kernels`.  dtype = float64, chol = True: the kernels' algebra and factorisation; dtype = LD: reference (B)."""
    m = (p["N"], p["A"], p["B"], p["Q"], p["R"], p["P"])
    xr, ur = qh.refs(p)
    free = side == 0
    out = {}
    if "sens" in kernels:
        out["K_plan"] = sr.masked_sweep(*m, free, dtype=dtype, chol=chol, stats=stats)
        out["dV_dx"] = sr.costate(p["N"], p["A"], p["Q"], p["P"], X, xr, dtype=dtype)
    if "grad" in kernels:
        out.update(gr.adjoint(*m, free, X, U, w, gam, xr, dtype=dtype, chol=chol, stats=stats))
    if "cgrad" in kernels:
        out.update(cg.adjoint(*m, side, X, U, w, gam, xr, ur, dtype=dtype, chol=chol, stats=stats))
    return out


def dense_gain(p, free):
    """K_plan (nu, N, nx, Bsz) long double on the face `free` (nu, N, Bsz), evaluated on that face directly: sens_ref's dense
    -H_FF^-1 Fx[F] with the referee's H and g(x) (Fx[:, a] = g(e_a) - g(0)).  It depends on the face alone: no certificate is needed."""
    R = qh.referee(p)
    nx, nu, Bsz = p["B"].shape
    N = p["N"]
    g0 = R.gc(np.zeros((nx, Bsz)))[0]
    Fx = np.zeros((Bsz, N * nu, nx), dtype=LD)
    for a in range(nx):
        e = np.zeros((nx, Bsz))
        e[a] = 1.0
        Fx[:, :, a] = R.gc(e)[0] - g0
    K = sr.gain_on_face(R.H, Fx, gr._time_major(free))
    return K.reshape(Bsz, N, nu, nx).transpose(2, 1, 3, 0)


def dense(p):
    """Reference (A): the dense long-double formulas at the referee's plan under cotangents(p), every output, with 'side' (the face the
    references certified), 'ok' and 'one_face' (the three references certified one and the same face)"""
    def f():
        rp = referee_plan(p)
        w, gam = cotangents(p)
        out = dict(K_plan=dense_gain(p, rp["side"] == 0))
        s = sr.reference(p, p["kw"], p["x0"], rp["U"])
        out["dV_dx"] = s["dV_dx"]
        g = gr.reference(p, p["kw"], p["x0"], rp["U"], w, gam)
        c = cg.reference(p, p["kw"], p["x0"], rp["U"], w, gam)
        out.update({k: g[k] for k, _ in KERNELS["grad"]})
        out.update({k: c[k] for k, _ in KERNELS["cgrad"]})
        same = np.array_equal(s["free"], c["side"] == 0) and np.array_equal(g["free"], c["side"] == 0)
        out.update(side=c["side"], ok=s["ok"] & g["ok"] & c["ok"], one_face=same, K_sens=s["K_plan"])
        return out
    return qh._memo("postpass-dense", p, f)


def errors(got, ref, keys=None):
    """{output: per-instance sens_ref.rel_err}; a non-finite error counts as infinite"""
    out = {}
    for k in (keys or [k for k in AXES if k in got and k in ref]):
        e = sr.rel_err(got[k], ref[k], AXES[k])
        out[k] = np.where(np.isfinite(e), e, np.inf)
    return out
