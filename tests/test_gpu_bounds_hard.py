"""GPU (-m gpu): lqmpc_bounds_batch on hard spectra against a 50-digit reference (oracle/bounds_mp.py), on all three implementations:
the prebuilt chip pair, the run-time compiled chip pair and the HBM-workspace kernel.

The models come from one seeded, instance-minor generator (problem() below; tests/test_bounds_hard_cpu.py imports it): unstable,
integrator chain, cheap / expensive control, nilpotent (deadbeat closed loop), A = 0 and 0.9 I (repeated eigenvalues, exact zeros
below the subdiagonal), weakly reachable, unreachable, power-of-two scalings, and Q / R a hair away from a multiple of I.  Every
entry is a multiple of 2^-24 (or an exact power-of-two multiple of such), so the inputs are the same bits on every machine and the
committed 50-digit answers (tests/golden/bounds_hard_mp.json, keyed by a hash of the inputs; `PYTHONPATH=. python tests/test_gpu_bounds_hard.py`
rewrites it, a miss is recomputed) belong to them.  A batch repeats a family's few distinct models, instance b = model b mod M, at
batch sizes 1, 3, 5 and 67: ragged tails on the four-per-wavefront and the one-per-wavefront kernels.

The bars are a priori, none was chosen after a measurement (eps = 2^-52):
  * extreme eigenvalue of a symmetric S of order m (A'A, B'B, K'K, Gamma'Gamma, Phi'Phi, hat H):
        |lambda_gpu - lambda_mp| <= max(m^2, 512) eps lambda_max(S)
    -- what any backward-stable method owes; for a norm (sqrt lambda_max) that is half of it, relative; for lambda_min(hat H) it is
    absolute, relative to lambda_max(hat H).  The floor 512 eps covers exp / log and the 56 squarings of the repeated-squaring
    estimate, whose roundings enter with weights 2^-j.
    |K|_2 is held to the 2-norm of the kernel's own K (mp.eigsy on its Gram matrix): K's own error has its bar:
  * K: |K_gpu - K_mp|_max <= max(10 e_host, 1e-12) |K_mp|_max with e_host scipy's own relative error on the same system (doubling
    and the Schur method share the DARE's condition number).
  * rho(A - BK): absolute, max(10 e_host, 1e-12), e_host the error of numpy's eigvals on A - B K_mp against mp.eig; the kernel's rho
    is held to mp.eig on ITS closed loop A - B K_gpu (as |K|_2 is: what K's error does to rho is K's bar); on the deadbeat family the
    eigenvalue 0 is defective and only 0 <= rho <= 1e-3, finite, status 0 is asked.
  * the scalar formulas, evaluated on the host from the GPU's own aux and K (bounds_np.coefficients_from_spectra): 1e-12 relative.
  * power-of-two scalings move |B|_2, |Gamma|_2 (and |A|_2) by exactly that power: 4 ulp.
The worst measured errors, per quantity, family, shape and kernel, are in profiles/bounds_hard_spectra.json (written by this module
when LQMPC_BOUNDS_HARD_JSON names a file)."""
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

from oracle import bounds_np
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
GRID = 2.0 ** 24
BATCHES = (1, 3, 5, 67)
HERE = os.path.dirname(os.path.abspath(__file__))
MP_CACHE = os.path.join(HERE, "golden", "bounds_hard_mp.json")

CHIP = "lqmpc_bounds_small_kernel + lqmpc_bounds_big_kernel"
WORKSPACE = "lqmpc_bounds_kernel"

# shape -> families; by what the shape switches (see the issue's table): (2,1,7), (4,2,10) prebuilt chip kernels; (1,1,1), (1,1,2) an
# empty tridiagonalisation loop; (5,1,20) n_x straddles a 4 x 4 tile; (4,2,16), (8,4,8) n = 32, the last 16-lane shape; (3,3,11) n = 33,
# the first 64-lane shape; (2,4,32) n = 128 (fp64 host reference only); (9,2,5), (4,5,4), (16,8,4) outside the chip domain
ALL = ("unstable", "integrator", "cheap", "expensive", "shift", "zero", "weak", "unreachable", "scaling", "qr_scalar", "qr_qpert", "qr_rpert")
EDGE = ("unstable", "integrator", "zero", "scaling")
CASES = {
    (4, 2, 10): ALL,
    (2, 1, 7): ("unstable", "integrator", "weak", "unreachable"),
    (1, 1, 1): EDGE, (1, 1, 2): EDGE,
    (5, 1, 20): ("unstable", "integrator", "cheap"),
    (4, 2, 16): EDGE, (8, 4, 8): EDGE, (3, 3, 11): EDGE,
    (2, 4, 32): ("unstable", "integrator"),
    (9, 2, 5): ("unstable", "integrator"), (4, 5, 4): ("unstable",), (16, 8, 4): ("unstable",),
}
CASE_LIST = [(f, s) for s, fams in CASES.items() for f in fams]
MP_MAX_N = 33


def in_chip_domain(nx, nu, N):
    return nx <= 8 and nu <= 4 and N * nu <= 128


# ------------------------------------------------ the problem families ------------------------------------------------
def grid(M):
    """onto multiples of 2^-24: the same bits wherever the generator runs"""
    return np.round(np.asarray(M, float) * GRID) / GRID


def _rand_A(rng, nx, rho):
    A = rng.standard_normal((nx, nx))
    return grid(A * (rho / np.max(np.abs(np.linalg.eigvals(A)))))


def _spd(rng, m, lo, hi):
    M = rng.standard_normal((m, m))
    M = M @ M.T / m + np.eye(m)
    M = grid(M * rng.uniform(lo, hi))
    return 0.5 * (M + M.T)


def _unit_cols(nx, nu, first):
    """n_u distinct unit columns, the first one e_first, the others going up from there"""
    B = np.zeros((nx, nu))
    for k in range(nu):
        B[(first - k) % nx, k] = 1.0
    return B


def problem(family, nx, nu, N):
    """One family at one shape: dict(N, Q, R, models = [(A, B), ...], stabilisable = [bool, ...], deadbeat)."""
    rng = np.random.default_rng(zlib.crc32(f"{family}-{nx}-{nu}-{N}".encode()))
    Q, R = _spd(rng, nx, 0.5, 3.0), _spd(rng, nu, 0.2, 2.0)
    rB = lambda: grid(rng.standard_normal((nx, nu)))
    deadbeat, stab = False, None
    if family == "unstable":
        models = [(_rand_A(rng, nx, rho), rB()) for rho in (1.3, 2.0)]
    elif family == "integrator":                   # Jordan block at 1 (and a chain with weaker links); the input enters at the end
        models = [(np.eye(nx) + np.diag(np.full(nx - 1, c), 1), _unit_cols(nx, nu, nx - 1)) for c in (1.0, 0.5)]
    elif family == "cheap":
        R = 1e-6 * np.eye(nu)
        models = [(_rand_A(rng, nx, rho), rB()) for rho in (0.9, 1.2)]
    elif family == "expensive":
        Q, R = np.eye(nx), 1e6 * np.eye(nu)
        models = [(_rand_A(rng, nx, 1.05), rB()) for _ in range(2)]
    elif family == "shift":                        # nilpotent A, the optimal closed loop stays strictly upper triangular
        Q, R = 1.7 * np.eye(nx), 0.6 * np.eye(nu)
        models = [(np.diag(np.ones(nx - 1), 1), _unit_cols(nx, nu, nx - 1)), (np.diag(np.full(nx - 1, 0.5), 1), _unit_cols(nx, nu, nx - 2))]
        deadbeat = True
    elif family == "zero":                         # Gamma'Gamma diagonal / Kronecker: eigenvalues of multiplicity N and n_u
        Q, R = 1.7 * np.eye(nx), np.diag(0.6 + 0.3 * np.arange(nu))
        models = [(a * np.eye(nx), _unit_cols(nx, nu, nu - 1)) for a in (0.0, 0.9)]
    elif family == "weak":
        d = np.array([0.5, -0.3, 0.2, 0.4, -0.1, 0.3, -0.2, 0.1] * 2)[:nx - 1]
        models = []
        for top in (1.2, 1.5):
            B = rB()
            B[0, :] = 1e-4
            models.append((np.diag(np.concatenate(([top], d))), B))
    elif family == "unreachable":                  # eigenvalue exactly 1 with a zero row in B, and its reachable twin
        A = np.diag(np.concatenate(([1.0], np.array([0.5, -0.3, 0.2, 0.4, -0.1, 0.3, -0.2, 0.1] * 2)[:nx - 1])))
        A[1:, 1:] += grid(0.05 * rng.standard_normal((nx - 1, nx - 1)))
        B0 = rB()
        B1 = B0.copy()
        B0[0, :] = 0.0
        B1[0, :] = 1.0
        models, stab = [(A, B0), (A, B1)], [False, True]
    elif family == "scaling":
        A, B = _rand_A(rng, nx, 0.8), rB()
        models = [(A, B), (A, B * 2.0 ** 20), (A, B * 2.0 ** -20), (A * 0.25, B * 0.25), (A * 2.0, B * 2.0)]
    elif family in ("qr_scalar", "qr_qpert", "qr_rpert"):
        rng = np.random.default_rng(zlib.crc32(f"qr-{nx}-{nu}-{N}".encode()))     # the three variants share their models
        Q, R = 1.7 * np.eye(nx), 0.6 * np.eye(nu)
        if family == "qr_qpert":
            Q[0, nx - 1] = Q[nx - 1, 0] = 1e-16
        if family == "qr_rpert":
            R[0, nu - 1] = R[nu - 1, 0] = 1e-16
        models = [(_rand_A(rng, nx, rho), rB()) for rho in (0.5, 0.9, 1.1)]
    else:
        raise KeyError(family)
    return dict(family=family, shape=(nx, nu, N), N=N, Q=Q, R=R, models=models, deadbeat=deadbeat,
                stabilisable=stab if stab is not None else [True] * len(models))


def batch(prob, Bsz):
    """(A, B, model index) instance-minor: instance b is model b mod M"""
    idx = np.arange(Bsz) % len(prob["models"])
    A = np.ascontiguousarray(np.stack([prob["models"][j][0] for j in idx], axis=2))
    B = np.ascontiguousarray(np.stack([prob["models"][j][1] for j in idx], axis=2))
    return A, B, idx


def call_inputs(prob, Bsz):
    """the rest of a call: box, error levels, energy bars, state, parameter triple, V_expert"""
    nx, nu, N = prob["shape"]
    rng = np.random.default_rng(1000 * nx + 10 * nu + N)
    lb, ub = -rng.uniform(0.05, 0.5, nu), rng.uniform(0.05, 0.5, nu)
    eA, eB, MV = rng.uniform(1e-3, 1e-2, 67)[:Bsz], rng.uniform(1e-3, 1e-2, 67)[:Bsz], rng.uniform(0.1, 5.0, 67)[:Bsz]
    return dict(lb=lb, ub=ub, eA=eA.copy(), eB=eB.copy(), MV=MV.copy(), x=rng.standard_normal(nx) * 0.2, p=np.array([0.3, 1.5, 0.7]), V=1.7)


# ------------------------------------------------ references ------------------------------------------------
SPECTRAL = ("norm_A", "norm_B", "norm_K", "norm_Gamma", "norm_Phi", "min_eig_H")
_MP_KEYS = SPECTRAL + ("max_eig_H", "rho_cl")
_REF = {}
_DISK = None


def _key(N, A, B, Q, R):
    h = hashlib.sha1(str((int(N),) + A.shape + B.shape).encode())
    for M in (A, B, Q, R):
        h.update(np.ascontiguousarray(M, dtype="<f8").tobytes())
    return h.hexdigest()


def mp_compute(N, A, B, Q, R):
    """the 50-digit answers rounded to fp64, or None where dare() cannot certify a stabilising solution"""
    from oracle import bounds_mp
    try:
        _, K = bounds_mp.dare(A, B, Q, R)
    except bounds_mp.CertificateError:
        return None
    s = bounds_mp.spectra(N, A, B, Q, R, K)
    out = {k: float(s[k]) for k in _MP_KEYS}
    out["K"] = bounds_mp.to_float(K).tolist()
    return out


def mp_reference(N, A, B, Q, R):
    global _DISK
    if _DISK is None:
        _DISK = json.load(open(MP_CACHE)) if os.path.exists(MP_CACHE) else {}
    k = _key(N, A, B, Q, R)
    if k not in _DISK:
        pytest.importorskip("mpmath")
        _DISK[k] = mp_compute(N, A, B, Q, R)
    return _DISK[k]


def host_values(N, A, B, Q, R, K):
    """the fp64 host reference of the spectral numbers for the gain K (u = -K x): LAPACK on the matrices as bounds_np builds them"""
    G, Phi = bounds_np.gamma_phi(N, A, B)
    hatH = np.kron(R, np.eye(N)) + G.T @ np.kron(Q, np.eye(N + 1)) @ G
    ev = np.linalg.eigvalsh(0.5 * (hatH + hatH.T))
    return dict(norm_A=np.linalg.norm(A, 2), norm_B=np.linalg.norm(B, 2), norm_K=np.linalg.norm(K, 2), norm_Gamma=np.linalg.norm(G, 2),
                norm_Phi=np.linalg.norm(Phi, 2), min_eig_H=ev[0], max_eig_H=ev[-1], rho_cl=np.max(np.abs(np.linalg.eigvals(A - B @ K))), K=K)


_RHO = {}


def rho_exact(A, B, K):
    """rho(A - BK) of fp64 matrices by mp.eig at 50 digits, rounded (cached: a batch repeats its models)"""
    key = A.tobytes() + B.tobytes() + np.ascontiguousarray(K).tobytes()
    if key not in _RHO:
        pytest.importorskip("mpmath")
        from oracle import bounds_mp
        with bounds_mp.mp.workdps(bounds_mp.DPS):
            _RHO[key] = float(bounds_mp.spectral_radius(bounds_mp._mat(A) - bounds_mp._mat(B) * bounds_mp._mat(K)))
    return _RHO[key]


_NORMK = {}


def norm_exact(K):
    """|K|_2 of an fp64 matrix by mp.eigsy on its Gram matrix at 50 digits, rounded (cached)"""
    K = np.ascontiguousarray(K)
    key = K.tobytes()
    if key not in _NORMK:
        pytest.importorskip("mpmath")
        from oracle import bounds_mp
        with bounds_mp.mp.workdps(bounds_mp.DPS):
            lam = bounds_mp._sym_extremes(bounds_mp._gram(bounds_mp._mat(K)))[1]
            _NORMK[key] = float(bounds_mp.mp.sqrt(max(lam, 0)))
    return _NORMK[key]


def order_of(q, nx, nu, N):
    """order of the symmetric matrix whose extreme eigenvalue the quantity is"""
    return {"norm_A": nx, "norm_B": nu, "norm_K": nx, "norm_Phi": nx, "norm_Gamma": N * nu, "min_eig_H": N * nu}[q]


def spectral_error(q, got, ref, shape):
    """(error, bar), both in units of lambda_max(S): relative for a norm (half the eigenvalue's bar), absolute / lambda_max(hat H) for
    lambda_min(hat H)"""
    m = order_of(q, *shape)
    bar = max(m * m, 512) * EPS
    if q == "min_eig_H":
        return abs(got - ref["min_eig_H"]) / ref["max_eig_H"], bar
    r = ref[q]
    return (abs(got - r) / r if r > 0 else abs(got)), 0.5 * bar


def reference(prob, j):
    """dict(ref = the reference the GPU is held to (mp for N n_u <= 33, else the fp64 host's), host = the fp64 host's numbers,
    e_host_K, e_host_rho), or None for a model that is not stabilisable."""
    key = (prob["family"], prob["shape"], j)
    if key in _REF:
        return _REF[key]
    N, Q, R = prob["N"], prob["Q"], prob["R"]
    A, B = prob["models"][j]
    nx, nu, _ = prob["shape"]
    out = None
    if N * nu > MP_MAX_N:
        if prob["stabilisable"][j]:
            K = orc.dlqr_gain(A, B, Q, R)[0]
            h = host_values(N, A, B, Q, R, K)
            out = dict(ref=h, host=h, e_host_K=0.0, e_host_rho=0.0, mp=False)
    else:
        m = mp_reference(N, A, B, Q, R)
        if m is not None:
            m = dict(m, K=np.array(m["K"]).reshape(nu, nx))
            K = orc.dlqr_gain(A, B, Q, R)[0]
            kmax = np.abs(m["K"]).max()
            e_K = np.abs(K - m["K"]).max() / kmax if kmax > 0 else np.abs(K).max()
            e_rho = abs(np.max(np.abs(np.linalg.eigvals(A - B @ m["K"]))) - m["rho_cl"])
            out = dict(ref=m, host=host_values(N, A, B, Q, R, K), e_host_K=float(e_K), e_host_rho=float(e_rho), mp=True)
    _REF[key] = out
    return out


# ------------------------------------------------ measurements ------------------------------------------------
MEASURED = {}
PROFILE_HEAD = {
    "what": "worst error per kernel / family / shape / quantity of tests/test_gpu_bounds_hard.py, written by that module when "
            "LQMPC_BOUNDS_HARD_JSON names a file: gpu against the 50-digit reference (oracle/bounds_mp.py; the fp64 host's numbers at 2x4x32), "
            "host = the fp64 host reference against the same 50 digits, bar = the largest bar among the key's instances",
    "units": {
        "norm_*": "relative error of the norm (bar: half of max(m^2, 512) eps, m the order of the Gram matrix); norm_K against the norm of the kernel's own K",
        "min_eig_H": "absolute error over lambda_max(hat H) (bar: max(n^2, 512) eps)",
        "K": "max-norm error over |K_mp|_max (bar: max(10 e_host, 1e-12), host = e_host, scipy's error)",
        "rho_cl": "absolute error against mp.eig on the kernel's own closed loop (bar: max(10 e_host, 1e-12), host = e_host; 1e-3 on the deadbeat family)",
        "rho_cl_against_exact_gain": "absolute error against rho(A - B K_mp); recorded, not asserted (it carries K's error)",
        "formula_*": "relative error of the kernel's output against the host formulas evaluated on the kernel's own aux and K (bar 1e-12)",
        "scaling_ulp_*": "ulps between the norm of the power-of-two scaled model and the scaled norm of the base model (bar 4)",
    },
    "bars": "all a priori (module docstring of tests/test_gpu_bounds_hard.py)",
}


def record(kernel, prob, q, err, bar, host_err=None):
    """bar = None: recorded only"""
    key = "/".join((kernel, prob["family"], "x".join(map(str, prob["shape"])), q))
    e = MEASURED.setdefault(key, dict(gpu=0.0, bar=bar, host=None))
    e["gpu"] = max(e["gpu"], float(err))
    if bar is not None:
        e["bar"] = max(e["bar"], float(bar))         # (K and rho: the bar depends on the model; the largest one of the key)
        if err > bar:
            e["missed_by"] = max(e.get("missed_by", 0.0), float(err / bar) if bar > 0 else float("inf"))
    if host_err is not None:
        e["host"] = max(e["host"] or 0.0, float(host_err))


@pytest.fixture(scope="module", autouse=True)
def _dump_measurements():
    yield
    path = os.environ.get("LQMPC_BOUNDS_HARD_JSON")
    if path and MEASURED:
        with open(path, "w") as f:
            json.dump(dict(PROFILE_HEAD, measured=MEASURED), f, indent=1, sort_keys=True)


@pytest.fixture(params=[CHIP, WORKSPACE], ids=["chip", "workspace"])
def bsolver(request, solver):
    """both implementations of lqmpc_bounds_batch (a copy of test_gpu_bounds.py's)"""
    from lq_mpc_amd import KERNEL_GENERIC, KERNEL_AUTO
    solver.set_options(kernel=KERNEL_GENERIC if request.param == WORKSPACE else KERNEL_AUTO)
    solver.expected_bounds_kernel = request.param
    yield solver
    solver.set_options(kernel=KERNEL_AUTO)


def run(solver, prob, Bsz, want_aux=True):
    A, B, idx = batch(prob, Bsz)
    c = call_inputs(prob, Bsz)
    g = solver.bounds_batch(prob["N"], A, B, prob["Q"], prob["R"], c["lb"], c["ub"], c["eA"], c["eB"], c["MV"], c["x"], c["p"], c["V"],
                            want_aux=want_aux)
    return g, idx, c


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


FORMULA_KEYS = ("gamma", "xi", "eta", "alpha", "beta", "bound", "eps")
_SHARE = {"compared": 0, "all": 0}


def check_formulas(prob, g, c, b, kernel, failures):
    """The scalar formulas on the host from the GPU's own aux and K against the GPU's outputs: 1e-12 relative; status 3 exactly where
    they leave the reals.  gamma, xi, eta, bound only away from gamma's pole."""
    try:
        with np.errstate(all="ignore"):
            h = bounds_np.coefficients_from_spectra(prob["N"], prob["Q"], prob["R"], c["lb"], c["ub"], c["eA"][b], c["eB"][b], c["MV"][b], c["x"],
                                                    c["p"], c["V"], g["K"][:, :, b], *(g[k][b] for k in ("rho_cl", "norm_A", "norm_B", "norm_Gamma",
                                                                                                        "norm_Phi", "min_eig_H", "norm_K")))
        real = all(np.isfinite(h[k]) for k in ("alpha", "beta", "xi", "eta"))
    except (ValueError, OverflowError, ZeroDivisionError):
        h, real = None, False
    if (g["status"][b] == 3) != (not real):
        failures.append(f"instance {b}: status {g['status'][b]} but the host formulas {'stay in' if real else 'leave'} the reals")
    _SHARE["all"] += 1
    if h is None:
        return
    away = abs(1 - (g["rho_cl"][b] + 0.4) ** 2) > 1e-3 and g["status"][b] == 0
    _SHARE["compared"] += bool(away)
    for k in FORMULA_KEYS:
        if k in ("gamma", "xi", "eta", "bound") and not away:
            continue
        if h[k] == g[k][b]:                        # (eps = inf on both sides where K = 0)
            continue
        if not (np.isfinite(h[k]) and np.isfinite(g[k][b])):
            if not (k == "bound" or g["status"][b] == 3):
                failures.append(f"instance {b}: {k} gpu {g[k][b]} host formula {h[k]}")
            continue
        e = rel(g[k][b], h[k])
        record(kernel, prob, "formula_" + k, e, 1e-12)
        if not e <= 1e-12:
            failures.append(f"instance {b}: formula {k} gpu {g[k][b]!r} host-from-aux {h[k]!r} rel {e:.3e} > 1e-12")


def check_call(prob, g, idx, c, kernel):
    """every output of one call against the references; returns the list of misses"""
    shape, failures = prob["shape"], []
    for b, j in enumerate(idx):
        r = reference(prob, j)
        st = g["status"][b]
        if not prob["stabilisable"][j]:
            if st not in (1, 2):
                failures.append(f"instance {b} (model {j}, not stabilisable): status {st}, expected 1 or 2")
            continue
        if st not in (0, 3):
            failures.append(f"instance {b} (model {j}): status {st} on a stabilisable system")
            continue
        ref = r["ref"]
        for q in SPECTRAL:
            # |K|_2 is the eigen-solver's answer on the kernel's OWN gain (K has its bar below): against mp's norm of that gain
            own = dict(ref, norm_K=norm_exact(g["K"][:, :, b]) if r["mp"] else np.linalg.norm(g["K"][:, :, b], 2)) if q == "norm_K" else ref
            e, bar = spectral_error(q, g[q][b], own, shape)
            he = spectral_error(q, r["host"][q], ref, shape)[0] if r["mp"] and q != "norm_K" else None
            record(kernel, prob, q, e, bar, he)
            if not e <= bar:
                failures.append(f"instance {b} (model {j}): {q} gpu {g[q][b]!r} ref {ref[q]!r} err {e:.3e} > bar {bar:.3e}")
        kmax = np.abs(ref["K"]).max()
        eK = np.abs(g["K"][:, :, b] - ref["K"]).max() / kmax if kmax > 0 else np.abs(g["K"][:, :, b]).max()
        barK = max(10 * r["e_host_K"], 1e-12)
        record(kernel, prob, "K", eK, barK, r["e_host_K"])
        if not eK <= barK:
            failures.append(f"instance {b} (model {j}): K err {eK:.3e} > bar {barK:.3e} (e_host {r['e_host_K']:.3e})")
        rho = g["rho_cl"][b]
        if prob["deadbeat"]:
            record(kernel, prob, "rho_cl", abs(rho), 1e-3)
            if not (np.isfinite(rho) and 0.0 <= rho <= 1e-3 and st == 0):
                failures.append(f"instance {b} (model {j}): deadbeat closed loop, rho {rho!r} status {st}")
        else:
            # the spectral radius of the kernel's OWN closed loop (K has its bar above), by mp.eig where the reference is mp's
            exact = rho_exact(*prob["models"][j], g["K"][:, :, b]) if r["mp"] else ref["rho_cl"]
            e, bar = abs(rho - exact), max(10 * r["e_host_rho"], 1e-12)
            record(kernel, prob, "rho_cl", e, bar, r["e_host_rho"])
            # (for the record, not asserted: against the rho of the EXACT gain -- this one carries K's error as well)
            record(kernel, prob, "rho_cl_against_exact_gain", abs(rho - ref["rho_cl"]), None, abs(r["host"]["rho_cl"] - ref["rho_cl"]))
            if not e <= bar:
                failures.append(f"instance {b} (model {j}): rho_cl gpu {rho!r} ref {ref['rho_cl']!r} err {e:.3e} > bar {bar:.3e}")
        check_formulas(prob, g, c, b, kernel, failures)
    return failures


def expected_kernel(solver, shape):
    return solver.expected_bounds_kernel if in_chip_domain(*shape) else WORKSPACE


# ------------------------------------------------ the tests ------------------------------------------------
@pytest.mark.parametrize("family,shape", CASE_LIST, ids=[f"{f}-{'x'.join(map(str, s))}" for f, s in CASE_LIST])
def test_hard_family(bsolver, family, shape):
    """Every output of every instance within the bars of the module docstring, at batch sizes 1, 3, 5, 67 (n = 128: up to 5)."""
    prob = problem(family, *shape)
    kernel = "workspace" if expected_kernel(bsolver, shape) == WORKSPACE else "chip"
    failures = []
    for Bsz in BATCHES:
        if shape[2] * shape[1] > MP_MAX_N and in_chip_domain(*shape) and Bsz > 8:
            continue
        g, idx, c = run(bsolver, prob, Bsz)
        assert bsolver.last_kernel() == expected_kernel(bsolver, shape)
        failures += [f"Bsz {Bsz}: {m}" for m in check_call(prob, g, idx, c, kernel)]
    for k, v in sorted(MEASURED.items()):
        if k.startswith("/".join((kernel, family, "x".join(map(str, shape))))) and not k.split("/")[-1].startswith("formula_"):
            print(f"{k}: gpu {v['gpu']:.3e} bar {v['bar'] if v['bar'] is None else format(v['bar'], '.3e')} host {v['host'] if v['host'] is None else format(v['host'], '.3e')}")
    assert not failures, "\n".join(failures[:40])


def test_formulas_compared_on_enough_instances(bsolver):
    """gamma, xi, eta and the bound are compared only away from gamma's pole and where the formulas stay real: over the families at
    (4, 2, 10) that has to be at least 0.4 of the instances, as in test_gpu_bounds.py."""
    _SHARE["compared"] = _SHARE["all"] = 0
    kernel = "workspace" if bsolver.expected_bounds_kernel == WORKSPACE else "chip"
    for family in ALL:
        prob = problem(family, 4, 2, 10)
        g, idx, c = run(bsolver, prob, 5)
        failures = []
        for b, j in enumerate(idx):
            if prob["stabilisable"][j] and g["status"][b] in (0, 3):
                check_formulas(prob, g, c, b, kernel, failures)
        assert not failures, "\n".join(failures)
    assert _SHARE["compared"] >= 0.4 * _SHARE["all"], _SHARE


@pytest.mark.parametrize("shape", [(4, 2, 10), (4, 2, 16), (3, 3, 11)], ids=lambda s: "x".join(map(str, s)))
def test_power_of_two_scalings_are_exact(bsolver, shape):
    """B 2^+-20 moves |B|_2 and |Gamma|_2 by exactly that power, (A, B) 2^k moves |A|_2 and |B|_2 by 2^k: 4 ulp."""
    prob = problem("scaling", *shape)
    g, idx, _ = run(bsolver, prob, 5)
    kernel = "workspace" if bsolver.expected_bounds_kernel == WORKSPACE else "chip"
    failures = []
    for j, s, keys in ((1, 2.0 ** 20, ("norm_B", "norm_Gamma")), (2, 2.0 ** -20, ("norm_B", "norm_Gamma")), (3, 0.25, ("norm_A", "norm_B")),
                       (4, 2.0, ("norm_A", "norm_B"))):
        for k in keys:
            base, got = g[k][0] * s, g[k][j]
            ulps = abs(got - base) / np.spacing(base)
            record(kernel, prob, "scaling_ulp_" + k, ulps, 4.0)
            if not ulps <= 4:
                failures.append(f"{k} of model {j}: {got!r} against {base!r} = base * {s}: {ulps:.1f} ulp")
    assert not failures, "\n".join(failures)


def test_scalar_weight_shortcuts_agree_with_the_dense_path(bsolver):
    """Q = 1.7 I and R = 0.6 I take the q_scalar / r_scalar shortcuts of the chip kernels; one symmetric off-diagonal pair at 1e-16
    sends the same models down the dense path.  Each variant meets its own bars (test_hard_family); here the three agree with each
    other within twice the bars."""
    shape = (4, 2, 10)
    res = {f: run(bsolver, problem(f, *shape), 5)[0] for f in ("qr_scalar", "qr_qpert", "qr_rpert")}
    ref = reference(problem("qr_scalar", *shape), 0)
    assert ref is not None
    base = res["qr_scalar"]
    idx = np.arange(5) % 3
    for f in ("qr_qpert", "qr_rpert"):
        assert np.array_equal(res[f]["status"], base["status"])
        for b in range(5):
            r = reference(problem("qr_scalar", *shape), idx[b])
            for q in SPECTRAL:
                m = order_of(q, *shape)
                scale = r["ref"]["max_eig_H"] if q == "min_eig_H" else r["ref"][q]
                assert abs(res[f][q][b] - base[q][b]) <= 2 * max(m * m, 512) * EPS * scale, (f, q, b)
            kmax = np.abs(r["ref"]["K"]).max()
            assert np.abs(res[f]["K"][:, :, b] - base["K"][:, :, b]).max() <= 2 * max(10 * r["e_host_K"], 1e-12) * kmax, (f, b)


@pytest.mark.parametrize("shape", [(4, 2, 10), (3, 3, 11)], ids=lambda s: "x".join(map(str, s)))
def test_neighbours_keep_their_bits(bsolver, shape):
    """67 well-conditioned systems, and the same batch with an expensive-control model (R = 1e6 I is batch-shared, so B 1e-3 under
    R = I: the same closed loop at rho ~ 0.96, doubling's slow end), the unreachable eigenvalue 1 and a NaN model in wavefronts (and
    four-instance groups) they share with untouched instances: every output of an untouched instance is the same bits."""
    nx, nu, N = shape
    rng = np.random.default_rng(77)
    Bsz = 67
    A = np.stack([_rand_A(rng, nx, rho) for rho in rng.uniform(0.2, 0.9, Bsz)], axis=2)
    B = grid(rng.standard_normal((nx, nu, Bsz)))
    Q, R = _spd(rng, nx, 0.5, 3.0), np.eye(nu)
    c = call_inputs(dict(shape=shape), Bsz)
    A2, B2 = A.copy(), B.copy()
    slow, unreach = problem("expensive", *shape)["models"][0], problem("unreachable", *shape)["models"][0]
    swapped = {1: (slow[0], slow[1] * 1e-3), 6: unreach, 11: (np.full((nx, nx), np.nan), B[:, :, 11]), 14: (slow[0], slow[1] * 1e-3),
               15: unreach, 40: (A[:, :, 40], np.full((nx, nu), np.nan)), 65: unreach, 66: (slow[0], slow[1] * 1e-3)}
    for b, (Ab, Bb) in swapped.items():
        A2[:, :, b], B2[:, :, b] = Ab, Bb
    out = []
    for Ax, Bx in ((A, B), (A2, B2)):
        out.append(bsolver.bounds_batch(N, np.ascontiguousarray(Ax), np.ascontiguousarray(Bx), Q, R, c["lb"], c["ub"], c["eA"], c["eB"], c["MV"],
                                        c["x"], c["p"], c["V"], want_aux=True))
        assert bsolver.last_kernel() == bsolver.expected_bounds_kernel
    keep = np.array([b for b in range(Bsz) if b not in swapped])
    g0, g1 = out
    assert np.all((g0["status"] == 0) | (g0["status"] == 3))
    for k in g0:
        a0, a1 = np.take(g0[k], keep, axis=-1), np.take(g1[k], keep, axis=-1)
        assert np.array_equal(a0.view(np.int32 if k == "status" else np.int64), a1.view(np.int32 if k == "status" else np.int64)), k
    for b in (6, 15, 65):
        assert g1["status"][b] in (1, 2), (b, g1["status"][b])
    for b in (11, 40):
        assert g1["status"][b] != 0, (b, g1["status"][b])
    for b in (1, 14, 66):
        assert g1["status"][b] in (0, 3), (b, g1["status"][b])


def test_status_alone(bsolver):
    """Every optional output and M_V NULL except status, through the raw ABI: returns 0, and the status of the full call."""
    from lq_mpc_amd.mpc import _ptr
    shape = (4, 2, 10)
    prob = problem("unreachable", *shape)
    A, B, idx = batch(prob, 5)
    c = call_inputs(prob, 5)
    full = bsolver.bounds_batch(prob["N"], A, B, prob["Q"], prob["R"], c["lb"], c["ub"], c["eA"], c["eB"], None, c["x"], c["p"], c["V"], want_aux=True)
    status = np.full(5, -7, dtype=np.int32)
    Q, R = np.ascontiguousarray(prob["Q"]), np.ascontiguousarray(prob["R"])
    rc = bsolver._L.lqmpc_bounds_batch(bsolver._h, 4, 2, 10, 5, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(c["lb"]), _ptr(c["ub"]), _ptr(c["eA"]),
                                       _ptr(c["eB"]), None, _ptr(c["x"]), _ptr(c["p"]), float(c["V"]), None, None, None, None, None, None, None,
                                       None, _ptr(status))
    assert rc == 0
    assert bsolver.last_kernel() == bsolver.expected_bounds_kernel
    assert np.array_equal(status, full["status"])
    assert set(status[idx == 0]) <= {1, 2} and set(status[idx == 1]) <= {0, 3}


if __name__ == "__main__":                     # rewrite tests/golden/bounds_hard_mp.json: every model of CASES with N n_u <= 33
    cache = {}
    for fam, shp in CASE_LIST:
        if shp[2] * shp[1] > MP_MAX_N:
            continue
        pr = problem(fam, *shp)
        for Am, Bm in pr["models"]:
            kk = _key(pr["N"], Am, Bm, pr["Q"], pr["R"])
            if kk not in cache:
                cache[kk] = mp_compute(pr["N"], Am, Bm, pr["Q"], pr["R"])
        print(fam, shp, flush=True)
    with open(MP_CACHE, "w") as fh:
        json.dump(cache, fh, indent=0, sort_keys=True)
