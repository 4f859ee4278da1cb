"""Prototype of the controller's retarget kernels (lqmpc_ctl_ref.hip), in numpy: what set_reference rewrites in a record.

Of a record [A | B | G | v_r | W | P] only v_r depends on the references:
    v_r = -W (2 g_ref + P c) = -2 W g_ref - c,        W = P^-1, c the centre of the box (per input, repeated over the stages)
with g_ref from the costate recursion on the record's own A and B (columns r = 0..N-1 <-> x_{r+1}, u_r):
    d_r = -xref_r,   lam_r = Q_r d_r + A' lam_{r+1}  (Q_{N-1} = P_T, lam_N = 0),   g_r = B' lam_r - R uref_r,   q_r = 2 g_r.
The kernels never see a dense W: the 16-lane-row records keep the packed lower triangle (element r (r + 1) / 2 + c), the workgroup
records the block image (lower block triangle of 16 x 16 blocks, 16 rows x 17 doubles each, diagonal blocks stored in full).  This
file restates the recursion and both indexings and checks them against the dense form -P^-1 (2 g_ref + P c) with g_ref taken from
the condensed matrices, for the shapes the GPU tests step.

    python tools/proto/ctl_retarget.py          # prints the error per shape and box
"""
import sys

import numpy as np

BS, LD = 16, 17
BLK = BS * LD
RECORD_SHAPES = [(2, 1, 10), (4, 2, 10), (4, 2, 20), (3, 2, 6), (7, 3, 11), (8, 4, 12)]
WG_SHAPES = [(8, 4, 13), (12, 2, 20)]
BOXES = [(-0.3, 0.3), (-0.2, 0.5)]
TARGET = 1e-12


def instance(nx, nu, N, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((nx, nx))
    A *= rng.uniform(0.5, 1.0) / np.abs(np.linalg.eigvals(A)).max()
    B = rng.standard_normal((nx, nu)) * rng.uniform(0.3, 1.0)

    def spd(m, c):
        q, _ = np.linalg.qr(rng.standard_normal((m, m)))
        return (q * np.geomspace(1.0, c, m)) @ q.T
    Q, R, PT = spd(nx, 10.0), spd(nu, 10.0), 3.0 * spd(nx, 10.0)
    return A, B, Q, R, PT, 0.1 * rng.standard_normal((nx, N)), 0.05 * rng.standard_normal((nu, N))


def dense(A, B, Q, R, PT, xref, uref, lb, ub):
    """The condensed Hessian P (n x n), W = P^-1 and v_r = -P^-1 (2 g_ref + P c), g_ref = -Gamma' Qbar xref - Rbar uref."""
    nx, nu = B.shape
    N = xref.shape[1]
    n = N * nu
    Gam = np.zeros((N * nx, n))
    for r in range(N):                       # block row r <-> x_{r+1}
        for s in range(r + 1):
            Gam[r * nx:(r + 1) * nx, s * nu:(s + 1) * nu] = np.linalg.matrix_power(A, r - s) @ B
    Qb = np.kron(np.eye(N), Q)
    Qb[-nx:, -nx:] = PT
    Rb = np.kron(np.eye(N), R)
    P = 2.0 * (Gam.T @ Qb @ Gam + Rb)
    P = 0.5 * (P + P.T)
    g = -Gam.T @ Qb @ xref.T.reshape(-1) - Rb @ uref.T.reshape(-1)
    c = np.tile(0.5 * (lb + ub), N)
    return P, np.linalg.inv(P), -np.linalg.solve(P, 2.0 * g + P @ c)


def costate_q(A, B, Q, R, PT, xref, uref):
    """q = 2 g_ref (n,), row r * nu + k, by the recursion the kernels run."""
    nx, nu = B.shape
    N = xref.shape[1]
    lam = np.zeros(nx)
    q = np.zeros(N * nu)
    for r in range(N - 1, -1, -1):
        lam = (Q if r < N - 1 else PT) @ (-xref[:, r]) + A.T @ lam
        q[r * nu:(r + 1) * nu] = 2.0 * (B.T @ lam - R @ uref[:, r])
    return q


# ---- the 16-lane-row record: packed lower triangle ----
def pack_triangle(W):
    n = W.shape[0]
    return np.array([W[r, c] for r in range(n) for c in range(r + 1)])


def sym(i, j):
    return i * (i + 1) // 2 + j if i >= j else j * (j + 1) // 2 + i


def vr_from_triangle(tri, q, centre, nu):
    n = q.size
    v = np.zeros(n)
    for i in range(n):                       # the row owner's walk
        t = 0.0
        for j in range(n):
            t += tri[sym(i, j)] * q[j]
        v[i] = -t - centre[i % nu]
    return v


# ---- the workgroup record: block image ----
def blk_index(ib, jb):
    return ib * (ib + 1) // 2 + jb


def block_image(W):
    """Lower block triangle, every stored block in full; the padding rows carry a unit diagonal (as the factor kernel leaves them)."""
    n = W.shape[0]
    nb = (n + BS - 1) // BS
    Wp = np.eye(nb * BS)
    Wp[:n, :n] = W
    img = np.zeros(nb * (nb + 1) // 2 * BLK)
    for ib in range(nb):
        for jb in range(ib + 1):
            for r in range(BS):
                o = blk_index(ib, jb) * BLK + r * LD
                img[o:o + BS] = Wp[ib * BS + r, jb * BS:(jb + 1) * BS]
    return img, nb


def vr_from_image(img, nb, q, centre, nu):
    n, np_ = q.size, nb * BS
    qp = np.zeros(np_)
    qp[:n] = q
    v = np.zeros(np_)
    for t in range(n):                       # row t: the blocks left of and on the diagonal by rows, the blocks below by columns
        ib, r = divmod(t, BS)
        acc = 0.0
        for jb in range(ib + 1):
            o = blk_index(ib, jb) * BLK + r * LD
            acc += img[o:o + BS] @ qp[jb * BS:(jb + 1) * BS]
        for kb in range(ib + 1, nb):
            o = blk_index(kb, ib) * BLK + r
            acc += img[o:o + BS * LD:LD] @ qp[kb * BS:(kb + 1) * BS]
        v[t] = -acc - centre[t % nu]
    return v                                 # padding rows stay 0


def errors(shape, box, seed=1, wg=False):
    """(error with both references, x_ref only, u_ref only, none), each max |v - v_dense| / max |v_dense| (absolute when v_dense = 0)."""
    nx, nu, N = shape
    A, B, Q, R, PT, xref, uref = instance(nx, nu, N, seed)
    lb, ub = box[0] * np.ones(nu), box[1] * np.ones(nu)
    centre = 0.5 * (lb + ub)
    out = []
    for xr, ur in ((xref, uref), (xref, 0 * uref), (0 * xref, uref), (0 * xref, 0 * uref)):
        _, W, want = dense(A, B, Q, R, PT, xr, ur, lb, ub)
        q = costate_q(A, B, Q, R, PT, xr, ur)
        if wg:
            img, nb = block_image(W)
            got = vr_from_image(img, nb, q, centre, nu)
            assert np.all(got[N * nu:] == 0.0)
            got = got[:N * nu]
        else:
            got = vr_from_triangle(pack_triangle(W), q, centre, nu)
        scale = np.max(np.abs(want))
        out.append(float(np.max(np.abs(got - want)) / (scale if scale > 0 else 1.0)))
    return out


def main():
    worst = 0.0
    for wg, shapes in ((False, RECORD_SHAPES), (True, WG_SHAPES)):
        for shape in shapes:
            for box in BOXES:
                e = errors(shape, box, wg=wg)
                worst = max(worst, *e)
                print(f"{'block image' if wg else 'triangle   '} {shape} box {box}: " + "  ".join(f"{x:.1e}" for x in e))
    print(f"worst {worst:.2e} (target {TARGET:g})")
    return 0 if worst <= TARGET else 1


if __name__ == "__main__":
    sys.exit(main())
