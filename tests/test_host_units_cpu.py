"""CPU: the HIP-free host pieces of the library (lq_mpc_amd/csrc/lqmpc_host.h) through tests/host_units.cpp, a stand-alone program
built with the address and undefined-behaviour sanitizers and run as a child process: the layout of the staging arena, and the dense
helpers host_spd_inverse, host_sym_eig_extremes and host_first_gain against numpy.  A sanitizer report ends the program with a
non-zero status, which fails the test.

Bound of the dense helpers: relative error <= 1e3 * eps * cond, cond the condition number of the matrix inverted or decomposed -- the
forward error of a backward-stable method with a generous constant; for the gain, cond is that of R + B'SB at the last step and the
bound is multiplied by N (the error is carried through N steps).  Largest errors seen on these cases (printed, pytest -s), against
the bound's 1e3: host_spd_inverse 0.15 eps cond, host_sym_eig_extremes 5 eps cond, host_first_gain 0.42 N eps cond.
"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
ALIGN = 256


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_units") / "host_units")
    # (the sanitizers' runtimes linked into the program itself: a shared runtime refuses to start unless it is the first library
    # loaded, which depends on the environment the suite runs in)
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", os.path.join(ROOT, "tests", "host_units.cpp"), "-o", exe], check=True)

    def run(lines, tmp_path):
        src = tmp_path / "cases.txt"
        src.write_text("\n".join(lines) + "\n")
        r = subprocess.run([exe, str(src)], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        out = [ln.split() for ln in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


def nums(a):
    return " ".join(repr(float(v)) for v in np.asarray(a, dtype=np.float64).ravel())


# ---------------- arena layout ----------------
def arena_cases():
    rng = np.random.default_rng(0)
    cases = [[], [(40, 0, 1)], [(40, 1, 1)], [(8, 0, 0), (8, 1, 0)],                          # empty, input only, output only, all NULL
             [(256, 0, 1), (256, 1, 1)], [(257, 1, 1), (255, 0, 1), (0, 0, 1), (0, 1, 1)]]
    for _ in range(300):
        n = int(rng.integers(1, 17))
        side = rng.integers(0, 3)                                                             # mixed, inputs only, outputs only
        cases.append([(int(rng.choice([4, 8])) * int(rng.integers(0, 5001)), int(rng.integers(0, 2)) if side == 0 else int(side == 2),
                       int(rng.random() < 0.8)) for _ in range(n)])
    return cases


def test_arena_layout(program, tmp_path):
    cases = arena_cases()
    out = program([f"arena {len(c)} " + " ".join(f"{b} {o} {p}" for b, o, p in c) for c in cases], tmp_path)
    for c, ln in zip(cases, out):
        assert ln[0] == "arena" and len(ln) == 3 + len(c)
        in_end, total, offs = int(ln[1]), int(ln[2]), [int(v) for v in ln[3:]]
        live = [(off, b, o) for (b, o, p), off in zip(c, offs) if p]
        spans = sorted((off, off + b) for off, b, _ in live if b)
        assert all(off % ALIGN == 0 for off, _, _ in live)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (c, offs)                  # no two arrays overlap
        assert all(off + b <= in_end for off, b, o in live if not o), (c, offs, in_end)        # inputs below the boundary
        assert all(off >= in_end for off, b, o in live if o), (c, offs, in_end)                # outputs at or above it
        assert 0 <= in_end <= total and total >= max([e for _, e in spans], default=0)
        if not any(not o for _, _, o in live):
            assert in_end == 0
        if not any(o for _, _, o in live):
            assert total == in_end
        # no more room than the alignment asks for
        assert total <= sum((b + ALIGN - 1) // ALIGN * ALIGN for _, b, _ in live)


# ---------------- dense helpers ----------------
def spd(rng, n, cond):
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    M = (V * np.geomspace(1.0, 1.0 / cond, n)) @ V.T
    return 0.5 * (M + M.T)


def spd_cases():
    rng = np.random.default_rng(1)
    return [spd(rng, n, cond) for n in (1, 2, 3, 8, 16) for cond in (1.0, 1e4) for _ in range(4)]


def test_spd_inverse(program, tmp_path):
    Ms = spd_cases()
    out = program([f"inv {len(M)} {nums(M)}" for M in Ms], tmp_path)
    worst = 0.0
    for M, ln in zip(Ms, out):
        assert ln[:2] == ["inv", "1"]
        got, ref = np.array(ln[2:], dtype=np.float64).reshape(M.shape), np.linalg.inv(M)
        err = np.linalg.norm(got - ref, 2) / np.linalg.norm(ref, 2) / (EPS * np.linalg.cond(M))
        worst = max(worst, err)
        assert err <= 1e3, (len(M), err)
    print(f"host_spd_inverse: largest relative error {worst:.3g} x eps x cond")


def test_sym_eig_extremes(program, tmp_path):
    Ms = spd_cases()
    out = program([f"eig {len(M)} {nums(M)}" for M in Ms], tmp_path)
    worst = 0.0
    for M, ln in zip(Ms, out):
        assert ln[:2] == ["eig", "1"]
        w = np.linalg.eigvalsh(M)
        err = max(abs(float(ln[2]) - w[-1]) / w[-1], abs(float(ln[3]) - w[0]) / w[0]) / (EPS * np.linalg.cond(M))
        worst = max(worst, err)
        assert err <= 1e3, (len(M), err)
    print(f"host_sym_eig_extremes: largest relative error {worst:.3g} x eps x cond")


def riccati_first_gain(A, B, Q, R, P, N):
    """S_N = P, K_j = (R + B'S B)^-1 B'S A, S <- Q + A'S (A - B K_j); returns K_0 and cond(R + B'S B) of the last step"""
    S = P
    for _ in range(N):
        Re = R + B.T @ S @ B
        Kg = np.linalg.solve(Re, B.T @ S @ A)
        S = Q + A.T @ S @ (A - B @ Kg)
    return Kg, np.linalg.cond(Re)


def test_first_gain(program, tmp_path):
    rng = np.random.default_rng(2)
    cases = []
    for nx, nu, N in ((2, 1, 5), (4, 2, 10), (8, 4, 12), (16, 4, 8)):
        for _ in range(6):
            A = rng.standard_normal((nx, nx))
            A *= rng.uniform(0.3, 1.2) / np.abs(np.linalg.eigvals(A)).max()
            Q = spd(rng, nx, 10.0)
            cases.append((nx, nu, N, A, rng.standard_normal((nx, nu)), Q, np.eye(nu), 3.0 * spd(rng, nx, 10.0)))
    out = program([f"gain {c[0]} {c[1]} {c[2]} " + " ".join(nums(m) for m in c[3:]) for c in cases], tmp_path)
    worst = 0.0
    for (nx, nu, N, A, B, Q, R, P), ln in zip(cases, out):
        assert ln[:2] == ["gain", "1"]
        ref, cond = riccati_first_gain(A, B, Q, R, P, N)
        got = np.array(ln[2:], dtype=np.float64).reshape(nu, nx)
        err = np.linalg.norm(got - ref, 2) / np.linalg.norm(ref, 2) / (N * EPS * cond)
        worst = max(worst, err)
        assert err <= 1e3, ((nx, nu, N), err)
    print(f"host_first_gain: largest relative error {worst:.3g} x N x eps x cond")


def test_refusals(program, tmp_path):
    asym = np.array([[2.0, 0.5], [0.1, 1.0]])
    indef = np.array([[1.0, 2.0], [2.0, 1.0]])
    out = program([f"eig 2 {nums(asym)}", f"inv 2 {nums(indef)}", f"eig 2 {nums(indef)}"], tmp_path)
    assert out[0][:2] == ["eig", "0"]                     # not symmetric
    assert out[1][:2] == ["inv", "0"]                     # not positive definite
    assert out[2][:2] == ["eig", "1"] and float(out[2][3]) < 0.0 < float(out[2][2])
