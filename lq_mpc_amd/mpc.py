"""Host-side mirror of the reference's operator interface for the MPC hot path.

Same class names, positional signatures and return dictionaries as
/root/reference/utils_class.py:
    LQ_MPC_Controller(N, A, B, Q, R, P, F_u).solve(x0, x_ref, u_ref) -> {'u_0', 'V_N'}   (lines 18-91)
    LQ_MPC_Simulator(T, N, A, B, Q, R, P, F_u).simulate(x0, A_true, B_true, x_ref, u_ref)
        -> {'X', 'U', 'J_T'}                                                              (lines 213-285)
so callers written against the reference (LQ_RDP_Behavior*, mpc_test.py) run unchanged, plus the
batched entry points a GPU needs (the reference API is one instance per call):
    BatchSolver.solve_batch / rollout_batch / max_vn_batch  over instance-minor (SoA) arrays,
    BatchController(solver, ...).step(x): the set-up kept on the GPU, one QP per instance and call.
solve_batch and step return the whole optimal plan as well with want_plan=True (the reference's controller.u.value).
An F_u that is not a box (a row with two or more non-zeros) goes through BatchSolver.solve_poly_batch / rollout_poly_batch; the two
classes pick those calls by themselves.
Everything executes in the HIP library behind include/lqmpc.h; there is no CPU path here.
"""
import ctypes

import numpy as np

from . import _lib


def box_from_Fu(F_u):
    """F_u u <= 1 with one non-zero per row (utils_class.py:81) -> (lb, ub).

    The reference accepts any polytope; every caller uses the box [10 I; -10 I].  Only box rows are
    supported here; anything else raises ValueError."""
    F_u = np.atleast_2d(np.asarray(F_u, dtype=np.float64))
    nu = F_u.shape[1]
    lb = np.full(nu, -np.inf)
    ub = np.full(nu, np.inf)
    for row in F_u:
        nz = np.flatnonzero(row)
        if nz.size != 1:
            raise ValueError("F_u must describe a box: exactly one non-zero per row")
        k = nz[0]
        if row[k] > 0:
            ub[k] = min(ub[k], 1.0 / row[k])
        else:
            lb[k] = max(lb[k], 1.0 / row[k])
    if not (np.all(np.isfinite(lb)) and np.all(np.isfinite(ub)) and np.all(lb < ub)):
        raise ValueError("F_u must bound every input from both sides (finite, non-empty box)")
    return lb, ub


def is_box_Fu(F_u):
    """True where every row of F_u has exactly one non-zero: the rows of a box, which go through box_from_Fu; a row with two or
    more makes F_u a polytope, which the solve_poly / rollout_poly calls serve.  (A row of zeros is left to box_from_Fu's error.)"""
    F_u = np.atleast_2d(np.asarray(F_u, dtype=np.float64))
    return not np.any(np.count_nonzero(F_u, axis=1) >= 2)


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError(f"expected shape {tuple(shape)}, got {a.shape}")
    return a


def _ptr(a):
    """void* for the ABI: numpy array (host), int address (device), object with data_ptr() (torch)."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return ctypes.c_void_p(a.ctypes.data)
    if hasattr(a, "data_ptr"):
        return ctypes.c_void_p(a.data_ptr())
    return ctypes.c_void_p(int(a))


def _ref_or_none(r, rows, N):
    """References as the reference reads them: columns 0..N-1 of a (rows, >= N) array (utils_class.py:69, 75 index
    x_ref[:, i], u_ref[:, i] for i < N only, so wider arrays -- e.g. one long reference shared by several horizons -- are
    accepted and the tail is ignored).  All-zero references (every caller in the reference) are passed as NULL."""
    if r is None:
        return None
    r = np.asarray(r, dtype=np.float64)
    if r.ndim != 2 or r.shape[0] != rows or r.shape[1] < N:
        raise ValueError(f"expected a reference of shape ({rows}, >= {N}), got {r.shape}")
    r = np.ascontiguousarray(r[:, :N])
    return r if np.any(r) else None



def _model_update_args(nx, nu, Bsz, A, B, idx):
    """The host arguments of BatchController.set_model, checked before the library sees them: A (nx, nx, m) and B (nx, nu, m)
    float64, idx None (then m == Bsz) or m distinct integers in [0, Bsz).  Returns (A, B, idx as int32 or None, m)."""
    A, B = np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(B, dtype=np.float64)
    if A.ndim != 3 or A.shape[:2] != (nx, nx):
        raise ValueError(f"A must be ({nx}, {nx}, m), got {A.shape}")
    m = A.shape[2]
    if B.shape != (nx, nu, m):
        raise ValueError(f"B must be ({nx}, {nu}, {m}), got {B.shape}")
    if idx is None:
        if m != Bsz:
            raise ValueError(f"idx=None replaces every model: m must be Bsz = {Bsz}, got {m}")
        return A, B, None, m
    idx = np.asarray(idx)
    if idx.size == 0:
        idx = idx.astype(np.int64)                           # (an empty list has no integer type of its own)
    if idx.ndim != 1 or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError("idx must be a one-dimensional sequence of integers")
    if idx.size != m:
        raise ValueError(f"idx names {idx.size} instances, A and B hold {m}")
    if m and (idx.min() < 0 or idx.max() >= Bsz):
        raise ValueError(f"idx must lie in [0, {Bsz})")
    if np.unique(idx).size != m:
        raise ValueError("idx must not name an instance twice")
    return A, B, np.ascontiguousarray(idx, dtype=np.int32), m



_CGRAD_KEYS = ("g_Q", "g_R", "g_P", "g_lb", "g_ub", "g_xref", "g_uref")


def _cgrad_outputs(nx, nu, N, Bsz, reduce):
    """the seven host outputs of a cost-gradient call, per instance (instance axis last) or reduced (the parameter's own shape)"""
    shapes = ((nx, nx), (nu, nu), (nx, nx), (nu,), (nu,), (nx, N), (nu, N))
    return {k: np.empty(sh if reduce else sh + (Bsz,)) for k, sh in zip(_CGRAD_KEYS, shapes)}


def _cgrad_dev_ptrs(outs):
    """the seven device outputs of a cost-gradient call from a dict keyed like the host flavour's result; missing or None: NULL"""
    unknown = set(outs) - set(_CGRAD_KEYS)
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}: the keys are {_CGRAD_KEYS}")
    return [_ptr(outs.get(k)) for k in _CGRAD_KEYS]


class BatchSolver:
    """One handle = one GPU + one stream (include/lqmpc.h).  Not thread-safe."""

    def __init__(self, device=0, stream=None, **options):
        self._L = _lib.lib()
        if self._L.lqmpc_device_count() <= 0:
            raise _lib.LqmpcError("no MI355X/HIP device visible: the lq_mpc_amd product path is GPU-only")
        self._h = ctypes.c_void_p()
        if stream is None:
            _lib.check(self._L.lqmpc_create(int(device), ctypes.byref(self._h)))
        else:
            _lib.check(self._L.lqmpc_create_on_stream(int(device), ctypes.c_void_p(int(stream)), ctypes.byref(self._h)))
        self.device = int(device)
        if options:
            self.set_options(**options)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.lqmpc_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- options ----
    def get_options(self):
        o = _lib.Options()
        _lib.check(self._L.lqmpc_get_options(self._h, ctypes.byref(o)))
        return {k: getattr(o, k) for k, _ in o._fields_}

    def set_options(self, **kw):
        o = _lib.Options()
        _lib.check(self._L.lqmpc_get_options(self._h, ctypes.byref(o)))
        for k, v in kw.items():
            if not hasattr(o, k):
                raise TypeError(f"unknown option {k!r}")
            setattr(o, k, v)
        _lib.check(self._L.lqmpc_set_options(self._h, ctypes.byref(o)))

    def sync(self):
        _lib.check(self._L.lqmpc_sync(self._h))

    def last_kernel(self):
        return self._L.lqmpc_last_kernel(self._h).decode()

    def reserve(self, nx, nu, N, Bsz, T=0):
        _lib.check(self._L.lqmpc_reserve(self._h, nx, nu, N, Bsz, T))

    def timer_begin(self):
        _lib.check(self._L.lqmpc_timer_begin(self._h))

    def timer_end(self):
        ms = ctypes.c_float()
        _lib.check(self._L.lqmpc_timer_end(self._h, ctypes.byref(ms)))
        return ms.value

    # ---- host-array entry points (numpy in, numpy out) ----
    @staticmethod
    def _dims(A, B):
        A = _f64(A)
        B = _f64(B)
        if A.ndim != 3 or B.ndim != 3 or A.shape[0] != A.shape[1] or B.shape[0] != A.shape[0] or B.shape[2] != A.shape[2]:
            raise ValueError("A must be (nx,nx,Bsz) and B (nx,nu,Bsz), instance-minor")
        return A, B, A.shape[0], B.shape[1], A.shape[2]

    def solve_batch(self, N, A, B, Q, R, P, lb, ub, x0, x_ref=None, u_ref=None, want_plan=False, want_sens=False):
        """want_plan: also "U_plan" (nu, N, Bsz), the whole optimal input sequence, and "X_plan" (nx, N + 1, Bsz), the model's
        states under it from x0 (lqmpc_solve_plan_batch); the other entries are bit for bit those of the plain call.
        want_sens: the plan keys, and the derivatives with respect to x0 on the face the plan reports (lqmpc_solve_sens_batch):
        "K_0" (nu, nx, Bsz), the gain of the local law u_0 = K_0 x0 + k_0; "dV_dx" (nx, Bsz); "K_plan" (nu, N, nx, Bsz), the gain of
        every stage of the plan."""
        A, B, nx, nu, Bsz = self._dims(A, B)
        Q, R, P = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx))
        lb, ub, x0 = _f64(lb, (nu,)), _f64(ub, (nu,)), _f64(x0, (nx, Bsz))
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        u0 = np.empty((nu, Bsz)); VN = np.empty(Bsz)
        status = np.empty(Bsz, dtype=np.int32); iters = np.empty(Bsz, dtype=np.int32)
        if want_sens:
            Up = np.empty((nu, N, Bsz)); Xp = np.empty((nx, N + 1, Bsz))
            K0 = np.empty((nu, nx, Bsz)); dV = np.empty((nx, Bsz)); Kp = np.empty((nu, N, nx, Bsz))
            _lib.check(self._L.lqmpc_solve_sens_batch(self._h, nx, nu, N, Bsz, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(P),
                                                      _ptr(lb), _ptr(ub), _ptr(x0), _ptr(x_ref), _ptr(u_ref),
                                                      _ptr(u0), _ptr(VN), _ptr(K0), _ptr(dV), _ptr(Kp), _ptr(Up), _ptr(Xp),
                                                      _ptr(status), _ptr(iters)))
            return {"u_0": u0, "V_N": VN, "status": status, "iters": iters, "U_plan": Up, "X_plan": Xp,
                    "K_0": K0, "dV_dx": dV, "K_plan": Kp}
        if want_plan:
            Up = np.empty((nu, N, Bsz)); Xp = np.empty((nx, N + 1, Bsz))
            _lib.check(self._L.lqmpc_solve_plan_batch(self._h, nx, nu, N, Bsz, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(P),
                                                      _ptr(lb), _ptr(ub), _ptr(x0), _ptr(x_ref), _ptr(u_ref),
                                                      _ptr(u0), _ptr(VN), _ptr(Up), _ptr(Xp), _ptr(status), _ptr(iters)))
            return {"u_0": u0, "V_N": VN, "status": status, "iters": iters, "U_plan": Up, "X_plan": Xp}
        _lib.check(self._L.lqmpc_solve_batch(self._h, nx, nu, N, Bsz, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(P),
                                             _ptr(lb), _ptr(ub), _ptr(x0), _ptr(x_ref), _ptr(u_ref),
                                             _ptr(u0), _ptr(VN), _ptr(status), _ptr(iters)))
        return {"u_0": u0, "V_N": VN, "status": status, "iters": iters}

    def rollout_batch(self, T, N, A, B, Q, R, P, lb, ub, x0, A_true, B_true, x_ref=None, u_ref=None, want_traj=False):
        A, B, nx, nu, Bsz = self._dims(A, B)
        Q, R, P = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx))
        lb, ub, x0 = _f64(lb, (nu,)), _f64(ub, (nu,)), _f64(x0, (nx, Bsz))
        A_true, B_true = _f64(A_true), _f64(B_true)
        per_inst = 1 if A_true.ndim == 3 else 0
        if per_inst:
            A_true, B_true = _f64(A_true, (nx, nx, Bsz)), _f64(B_true, (nx, nu, Bsz))
        else:
            A_true, B_true = _f64(A_true, (nx, nx)), _f64(B_true, (nx, nu))
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        JT = np.empty(Bsz)
        X = np.empty((nx, T + 1, Bsz)) if want_traj else None
        U = np.empty((nu, T, Bsz)) if want_traj else None
        status = np.empty(Bsz, dtype=np.int32); iters = np.empty(Bsz, dtype=np.int32)
        _lib.check(self._L.lqmpc_rollout_batch(self._h, nx, nu, N, Bsz, T, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(P),
                                               _ptr(lb), _ptr(ub), _ptr(x0), _ptr(A_true), _ptr(B_true), per_inst,
                                               _ptr(x_ref), _ptr(u_ref), _ptr(JT), _ptr(X), _ptr(U),
                                               _ptr(status), _ptr(iters)))
        return {"J_T": JT, "X": X, "U": U, "status": status, "iters": iters}

    @staticmethod
    def _plant(A_true, B_true, nx, nu, Bsz):
        """the plant of a rollout: single matrices shared by the batch or instance-minor arrays; (A_true, B_true, per_instance)"""
        A_true, B_true = _f64(A_true), _f64(B_true)
        if A_true.ndim == 3:
            return _f64(A_true, (nx, nx, Bsz)), _f64(B_true, (nx, nu, Bsz)), 1
        return _f64(A_true, (nx, nx)), _f64(B_true, (nx, nu)), 0

    @staticmethod
    def _Fu(F_u, nu):
        F_u = np.ascontiguousarray(np.atleast_2d(np.asarray(F_u, dtype=np.float64)))
        if F_u.ndim != 2 or F_u.shape[1] != nu:
            raise ValueError(f"F_u must be (m, {nu}), got {F_u.shape}")
        return F_u

    def solve_poly_batch(self, N, A, B, Q, R, P, F_u, x0, x_ref=None, u_ref=None, want_plan=False, want_lam=False, max_iter=0):
        """solve_batch under F_u u_i <= 1 for any (m, nu) matrix F_u (lqmpc_solve_poly_batch; N nu <= 64, m <= 16).
        want_plan: also "U_plan" (nu, N, Bsz) and "X_plan" (nx, N + 1, Bsz); want_lam: also "lam" (m, N, Bsz), the multipliers of the
        rows as given.  max_iter caps the active-set passes of a solve (0: 10 N nu + 20); status 1 where it was reached."""
        A, B, nx, nu, Bsz = self._dims(A, B)
        Q, R, P = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx))
        F_u, x0 = self._Fu(F_u, nu), _f64(x0, (nx, Bsz))
        m = F_u.shape[0]
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        u0 = np.empty((nu, Bsz)); VN = np.empty(Bsz)
        status = np.empty(Bsz, dtype=np.int32); iters = np.empty(Bsz, dtype=np.int32)
        Up = np.empty((nu, N, Bsz)) if want_plan else None
        Xp = np.empty((nx, N + 1, Bsz)) if want_plan else None
        lam = np.empty((m, N, Bsz)) if want_lam else None
        _lib.check(self._L.lqmpc_solve_poly_batch(self._h, nx, nu, N, Bsz, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(P), _ptr(F_u), m,
                                                  _ptr(x0), _ptr(x_ref), _ptr(u_ref), int(max_iter), _ptr(u0), _ptr(VN), _ptr(Up),
                                                  _ptr(Xp), _ptr(lam), _ptr(status), _ptr(iters)))
        out = {"u_0": u0, "V_N": VN, "status": status, "iters": iters}
        if want_plan:
            out["U_plan"], out["X_plan"] = Up, Xp
        if want_lam:
            out["lam"] = lam
        return out

    def rollout_poly_batch(self, T, N, A, B, Q, R, P, F_u, x0, A_true, B_true, x_ref=None, u_ref=None, want_traj=False, max_iter=0):
        """rollout_batch under F_u u_i <= 1 for any (m, nu) matrix F_u (lqmpc_rollout_poly_batch): T closed-loop steps, one launch."""
        A, B, nx, nu, Bsz = self._dims(A, B)
        Q, R, P = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx))
        F_u, x0 = self._Fu(F_u, nu), _f64(x0, (nx, Bsz))
        A_true, B_true, per_inst = self._plant(A_true, B_true, nx, nu, Bsz)
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        JT = np.empty(Bsz)
        X = np.empty((nx, T + 1, Bsz)) if want_traj else None
        U = np.empty((nu, T, Bsz)) if want_traj else None
        status = np.empty(Bsz, dtype=np.int32); iters = np.empty(Bsz, dtype=np.int32)
        _lib.check(self._L.lqmpc_rollout_poly_batch(self._h, nx, nu, N, Bsz, T, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(P), _ptr(F_u),
                                                    F_u.shape[0], _ptr(x0), _ptr(A_true), _ptr(B_true), per_inst, _ptr(x_ref),
                                                    _ptr(u_ref), int(max_iter), _ptr(JT), _ptr(X), _ptr(U), _ptr(status), _ptr(iters)))
        return {"J_T": JT, "X": X, "U": U, "status": status, "iters": iters}

    def rollout_tape_batch(self, T, N, A, B, Q, R, P, lb, ub, x0, A_true, B_true, x_ref=None, u_ref=None):
        """The closed loop of rollout_batch, leaving a tape (lqmpc_rollout_tape_batch): "J_T" (Bsz,), "X" (nx, T + 1, Bsz),
        "U" (nu, T, Bsz), "U_tape" (T, nu, N, Bsz) -- the whole plan of every step, U_tape[t] a valid U_plan for every post-pass call
        -- "status" (Bsz,) the largest over the steps, "status_tape" (T, Bsz) and "iters".  Not the fast rollout: one solve and one
        plant-step launch per step.  What rollout_grad_batch differentiates."""
        A, B, nx, nu, Bsz = self._dims(A, B)
        Q, R, P = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx))
        lb, ub, x0 = _f64(lb, (nu,)), _f64(ub, (nu,)), _f64(x0, (nx, Bsz))
        A_true, B_true, per_inst = self._plant(A_true, B_true, nx, nu, Bsz)
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        JT = np.empty(Bsz); X = np.empty((nx, T + 1, Bsz)); U = np.empty((nu, T, Bsz)); Ut = np.empty((T, nu, N, Bsz))
        status = np.empty(Bsz, dtype=np.int32); iters = np.empty(Bsz, dtype=np.int32); stt = np.empty((T, Bsz), dtype=np.int32)
        _lib.check(self._L.lqmpc_rollout_tape_batch(self._h, nx, nu, N, Bsz, T, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(P),
                                                    _ptr(lb), _ptr(ub), _ptr(x0), _ptr(A_true), _ptr(B_true), per_inst,
                                                    _ptr(x_ref), _ptr(u_ref), _ptr(JT), _ptr(X), _ptr(U), _ptr(status), _ptr(iters),
                                                    _ptr(Ut), _ptr(stt)))
        return {"J_T": JT, "X": X, "U": U, "U_tape": Ut, "status": status, "status_tape": stt, "iters": iters}

    def rollout_grad_batch(self, T, N, A, B, Q, R, P, lb, ub, A_true, B_true, X, U_tape, status_tape=None, g_JT=None, g_X=None, g_U=None,
                           x_ref=None, u_ref=None, want=("g_A", "g_B", "g_x0", "g_A_true", "g_B_true")):
        """The gradient of a loss on the closed loop with respect to the model, the plant and x0 of every instance, from the tape of
        rollout_tape_batch (lqmpc_rollout_grad_batch): X (nx, T + 1, Bsz), U_tape (T, nu, N, Bsz), status_tape (T, Bsz) or None;
        g_JT (Bsz,) = d loss / d J_T, g_X (nx, T + 1, Bsz) = d loss / d X, g_U (nu, T, Bsz) = d loss / d U, any may be None (zero),
        not all.  Returns the keys of `want`: "g_A" (nx, nx, Bsz), "g_B" (nx, nu, Bsz), "g_x0" (nx, Bsz) and, always per instance (sum
        them for a shared plant), "g_A_true", "g_B_true".  One kernel launch, no solve."""
        A, B, nx, nu, Bsz = self._dims(A, B)
        Q, R, P = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx))
        lb, ub = _f64(lb, (nu,)), _f64(ub, (nu,))
        A_true, B_true, per_inst = self._plant(A_true, B_true, nx, nu, Bsz)
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        X, U_tape = _f64(X, (nx, T + 1, Bsz)), _f64(U_tape, (T, nu, N, Bsz))
        status_tape = None if status_tape is None else np.ascontiguousarray(status_tape, dtype=np.int32).reshape(T, Bsz)
        g_JT = None if g_JT is None else _f64(g_JT, (Bsz,))
        g_X = None if g_X is None else _f64(g_X, (nx, T + 1, Bsz))
        g_U = None if g_U is None else _f64(g_U, (nu, T, Bsz))
        shapes = {"g_A": (nx, nx, Bsz), "g_B": (nx, nu, Bsz), "g_x0": (nx, Bsz), "g_A_true": (nx, nx, Bsz), "g_B_true": (nx, nu, Bsz)}
        out = {k: np.empty(shapes[k]) for k in want}
        _lib.check(self._L.lqmpc_rollout_grad_batch(self._h, nx, nu, N, Bsz, T, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(P), _ptr(lb),
                                                    _ptr(ub), _ptr(A_true), _ptr(B_true), per_inst, _ptr(x_ref), _ptr(u_ref), _ptr(X),
                                                    _ptr(U_tape), _ptr(status_tape), _ptr(g_JT), _ptr(g_X), _ptr(g_U),
                                                    *[_ptr(out.get(k)) for k in shapes]))
        return out

    def rollout_cost_grad_batch(self, T, N, A, B, Q, R, P, lb, ub, A_true, B_true, X, U_tape, status_tape=None, g_JT=None, g_X=None,
                                g_U=None, x_ref=None, u_ref=None, reduce=False):
        """The gradient of a loss on the closed loop with respect to the data the batch shares -- the weights, the references and the
        box -- from the tape of rollout_tape_batch (lqmpc_rollout_cost_grad_batch); arguments as rollout_grad_batch.  Returns the dict
        of cost_grad_batch: {"g_Q", "g_R", "g_P", "g_lb", "g_ub", "g_xref", "g_uref"} per instance with the instance axis last, or with
        reduce=True the sum over the batch in the shape of the parameter, formed on the GPU in a fixed order, and "skipped", the
        number of instances with status 2 at any step, which add nothing.  g_Q and g_R hold the direct part as well (the one Q and R
        also weigh J_T); for the controller's weights alone under fixed evaluation weights pass g_JT=None and put the evaluation cost
        into g_X and g_U.  g_Q, g_R, g_P take the entries of the matrix as independent: nothing is symmetrised.  One kernel launch
        (two with reduce), no solve."""
        A, B, nx, nu, Bsz = self._dims(A, B)
        Q, R, P = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx))
        lb, ub = _f64(lb, (nu,)), _f64(ub, (nu,))
        A_true, B_true, per_inst = self._plant(A_true, B_true, nx, nu, Bsz)
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        X, U_tape = _f64(X, (nx, T + 1, Bsz)), _f64(U_tape, (T, nu, N, Bsz))
        status_tape = None if status_tape is None else np.ascontiguousarray(status_tape, dtype=np.int32).reshape(T, Bsz)
        g_JT = None if g_JT is None else _f64(g_JT, (Bsz,))
        g_X = None if g_X is None else _f64(g_X, (nx, T + 1, Bsz))
        g_U = None if g_U is None else _f64(g_U, (nu, T, Bsz))
        out = _cgrad_outputs(nx, nu, N, Bsz, reduce)
        skipped = np.zeros(1, dtype=np.int64)
        _lib.check(self._L.lqmpc_rollout_cost_grad_batch(self._h, nx, nu, N, Bsz, T, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(P),
                                                         _ptr(lb), _ptr(ub), _ptr(A_true), _ptr(B_true), per_inst, _ptr(x_ref),
                                                         _ptr(u_ref), _ptr(X), _ptr(U_tape), _ptr(status_tape), _ptr(g_JT), _ptr(g_X),
                                                         _ptr(g_U), int(bool(reduce)), *[_ptr(out[k]) for k in _CGRAD_KEYS],
                                                         _ptr(skipped)))
        if reduce:
            out["skipped"] = int(skipped[0])
        return out

    def max_vn_batch(self, N, A, B, Q, R, P, lb, ub, x0s, x_ref=None, u_ref=None):
        A, B, nx, nu, Bsz = self._dims(A, B)
        Q, R, P = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx))
        lb, ub = _f64(lb, (nu,)), _f64(ub, (nu,))
        x0s = _f64(x0s)
        if x0s.ndim != 2 or x0s.shape[0] != nx:
            raise ValueError("x0s must be (nx, K)")
        K = x0s.shape[1]
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        MV = np.empty(Bsz)
        status = np.empty(Bsz, dtype=np.int32); iters = np.empty(Bsz, dtype=np.int32)
        _lib.check(self._L.lqmpc_max_vn_batch(self._h, nx, nu, N, Bsz, K, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(P),
                                              _ptr(lb), _ptr(ub), _ptr(x0s), _ptr(x_ref), _ptr(u_ref),
                                              _ptr(MV), _ptr(status), _ptr(iters)))
        return {"M_V": MV, "status": status, "iters": iters}

    def sweep_batch(self, T, N, A, B, Q, R, P, lb, ub, x0, x0s, A_true, B_true, x_ref=None, u_ref=None):
        """One horizon of the reference's sweep (utils_class.py:813-833): M_V over the K columns of x0s and the closed-loop
        cost J_T from x0, for the same models, in one call (one launch where the 16-lane-row layout serves the shape)."""
        A, B, nx, nu, Bsz = self._dims(A, B)
        Q, R, P = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx))
        lb, ub, x0 = _f64(lb, (nu,)), _f64(ub, (nu,)), _f64(x0, (nx, Bsz))
        x0s = _f64(x0s)
        if x0s.ndim != 2 or x0s.shape[0] != nx:
            raise ValueError("x0s must be (nx, K)")
        A_true, B_true = _f64(A_true), _f64(B_true)
        per_inst = 1 if A_true.ndim == 3 else 0
        if per_inst:
            A_true, B_true = _f64(A_true, (nx, nx, Bsz)), _f64(B_true, (nx, nu, Bsz))
        else:
            A_true, B_true = _f64(A_true, (nx, nx)), _f64(B_true, (nx, nu))
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        JT = np.empty(Bsz); MV = np.empty(Bsz)
        status = np.empty(Bsz, dtype=np.int32); iters = np.empty(Bsz, dtype=np.int32)
        _lib.check(self._L.lqmpc_sweep_batch(self._h, nx, nu, N, Bsz, T, x0s.shape[1], _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(P),
                                             _ptr(lb), _ptr(ub), _ptr(x0), _ptr(x0s), _ptr(A_true), _ptr(B_true), per_inst,
                                             _ptr(x_ref), _ptr(u_ref), _ptr(JT), _ptr(MV), _ptr(status), _ptr(iters)))
        return {"J_T": JT, "M_V": MV, "status": status, "iters": iters}

    def bounds_batch(self, N, A, B, Q, R, lb, ub, e_A, e_B, M_V, x, p, V_expert, want_aux=False):
        """Per model of the batch: dlqr gain K and the coefficients alpha, beta, xi, eta, bound of the reference's performance
        bound (utils_class.py:837-859: control.dlqr + energy_decreasing + energy_bound), on the GPU (lqmpc_bounds_batch).
        e_A, e_B, M_V: (Bsz,) arrays (scalars are broadcast; M_V may be None = 0)."""
        A, B, nx, nu, Bsz = self._dims(A, B)
        Q, R, lb, ub = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(lb, (nu,)), _f64(ub, (nu,))
        e_A = np.ascontiguousarray(np.broadcast_to(np.asarray(e_A, dtype=np.float64), (Bsz,)))
        e_B = np.ascontiguousarray(np.broadcast_to(np.asarray(e_B, dtype=np.float64), (Bsz,)))
        M_V = None if M_V is None else np.ascontiguousarray(np.broadcast_to(np.asarray(M_V, dtype=np.float64), (Bsz,)))
        x, p = _f64(x, (nx,)), _f64(p, (3,))
        out = {k: np.empty(Bsz) for k in ("alpha", "beta", "xi", "eta", "bound", "eps")}
        out["K"] = np.empty((nu, nx, Bsz))
        out["status"] = np.empty(Bsz, dtype=np.int32)
        aux = np.empty((8, Bsz)) if want_aux else None
        _lib.check(self._L.lqmpc_bounds_batch(self._h, nx, nu, N, Bsz, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(lb), _ptr(ub),
                                              _ptr(e_A), _ptr(e_B), _ptr(M_V), _ptr(x), _ptr(p), float(V_expert),
                                              _ptr(out["K"]), _ptr(out["alpha"]), _ptr(out["beta"]), _ptr(out["xi"]),
                                              _ptr(out["eta"]), _ptr(out["bound"]), _ptr(out["eps"]), _ptr(aux), _ptr(out["status"])))
        if want_aux:
            out.update(dict(zip(("gamma", "rho_cl", "norm_A", "norm_B", "norm_Gamma", "norm_Phi", "min_eig_H", "norm_K"), aux)))
        return out

    # ---- device-pointer entry points (torch tensors / raw addresses already in HBM; asynchronous) ----
    def solve_batch_dev(self, nx, nu, N, Bsz, dA, dB, Q, R, P, lb, ub, dx0, du0, dVN, dstatus=None, diters=None,
                        x_ref=None, u_ref=None):
        Q, R, P, lb, ub = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx)), _f64(lb, (nu,)), _f64(ub, (nu,))
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        _lib.check(self._L.lqmpc_solve_batch_dev(self._h, nx, nu, N, Bsz, _ptr(dA), _ptr(dB), _ptr(Q), _ptr(R), _ptr(P),
                                                 _ptr(lb), _ptr(ub), _ptr(dx0), _ptr(x_ref), _ptr(u_ref),
                                                 _ptr(du0), _ptr(dVN), _ptr(dstatus), _ptr(diters)))

    def solve_plan_batch_dev(self, nx, nu, N, Bsz, dA, dB, Q, R, P, lb, ub, dx0, du0, dVN, dUplan, dXplan=None, dstatus=None,
                             diters=None, x_ref=None, u_ref=None):
        """solve_batch_dev, and the whole plan: dUplan (nu, N, Bsz) required, dXplan (nx, N + 1, Bsz) optional."""
        Q, R, P, lb, ub = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx)), _f64(lb, (nu,)), _f64(ub, (nu,))
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        _lib.check(self._L.lqmpc_solve_plan_batch_dev(self._h, nx, nu, N, Bsz, _ptr(dA), _ptr(dB), _ptr(Q), _ptr(R), _ptr(P),
                                                      _ptr(lb), _ptr(ub), _ptr(dx0), _ptr(x_ref), _ptr(u_ref),
                                                      _ptr(du0), _ptr(dVN), _ptr(dUplan), _ptr(dXplan), _ptr(dstatus), _ptr(diters)))

    def solve_sens_batch_dev(self, nx, nu, N, Bsz, dA, dB, Q, R, P, lb, ub, dx0, du0, dVN, dK0, ddVdx, dKplan=None, dUplan=None,
                             dXplan=None, dstatus=None, diters=None, x_ref=None, u_ref=None):
        """solve_plan_batch_dev, and the derivatives with respect to x0: dK0 (nu, nx, Bsz) and ddVdx (nx, Bsz) required, dKplan
        (nu, N, nx, Bsz) and the plan's arrays optional (lqmpc_solve_sens_batch_dev)."""
        Q, R, P, lb, ub = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx)), _f64(lb, (nu,)), _f64(ub, (nu,))
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        _lib.check(self._L.lqmpc_solve_sens_batch_dev(self._h, nx, nu, N, Bsz, _ptr(dA), _ptr(dB), _ptr(Q), _ptr(R), _ptr(P),
                                                      _ptr(lb), _ptr(ub), _ptr(dx0), _ptr(x_ref), _ptr(u_ref),
                                                      _ptr(du0), _ptr(dVN), _ptr(dK0), _ptr(ddVdx), _ptr(dKplan), _ptr(dUplan),
                                                      _ptr(dXplan), _ptr(dstatus), _ptr(diters)))

    def model_grad_batch(self, N, A, B, Q, R, P, lb, ub, U_plan, X_plan, status=None, g_u0=None, g_VN=None, x_ref=None, u_ref=None):
        """The gradient of a loss on (u_0, V_N) with respect to the model of every instance, on the face the plan reports
        (lqmpc_model_grad_batch): U_plan (nu, N, Bsz), X_plan (nx, N + 1, Bsz) and status as a want_plan / want_sens call returned
        them for the same data; g_u0 (nu, Bsz) = d loss / d u_0 and g_VN (Bsz,) = d loss / d V_N, either may be None (zero), not
        both.  Returns {"g_A": (nx, nx, Bsz), "g_B": (nx, nu, Bsz), "g_x0": (nx, Bsz)}.  The post-pass alone: no solve."""
        A, B, nx, nu, Bsz = self._dims(A, B)
        Q, R, P = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx))
        lb, ub = _f64(lb, (nu,)), _f64(ub, (nu,))
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        U_plan, X_plan = _f64(U_plan, (nu, N, Bsz)), _f64(X_plan, (nx, N + 1, Bsz))
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int32).reshape(Bsz)
        g_u0 = None if g_u0 is None else _f64(g_u0, (nu, Bsz))
        g_VN = None if g_VN is None else _f64(g_VN, (Bsz,))
        gA = np.empty((nx, nx, Bsz)); gB = np.empty((nx, nu, Bsz)); gx = np.empty((nx, Bsz))
        _lib.check(self._L.lqmpc_model_grad_batch(self._h, nx, nu, N, Bsz, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(P), _ptr(lb), _ptr(ub),
                                                  _ptr(x_ref), _ptr(u_ref), _ptr(U_plan), _ptr(X_plan), _ptr(status), _ptr(g_u0),
                                                  _ptr(g_VN), _ptr(gA), _ptr(gB), _ptr(gx)))
        return {"g_A": gA, "g_B": gB, "g_x0": gx}

    def model_grad_batch_dev(self, nx, nu, N, Bsz, dA, dB, Q, R, P, lb, ub, dUplan, dXplan, dgA, dgB, dstatus=None, dgu0=None, dgVN=None,
                             dgx0=None, x_ref=None, u_ref=None):
        """Device pointers / tensors; enqueued on the solver's stream, returns at once (lqmpc_model_grad_batch_dev)."""
        Q, R, P, lb, ub = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx)), _f64(lb, (nu,)), _f64(ub, (nu,))
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        _lib.check(self._L.lqmpc_model_grad_batch_dev(self._h, nx, nu, N, Bsz, _ptr(dA), _ptr(dB), _ptr(Q), _ptr(R), _ptr(P), _ptr(lb),
                                                      _ptr(ub), _ptr(x_ref), _ptr(u_ref), _ptr(dUplan), _ptr(dXplan), _ptr(dstatus),
                                                      _ptr(dgu0), _ptr(dgVN), _ptr(dgA), _ptr(dgB), _ptr(dgx0)))

    def plan_grad_batch(self, N, A, B, Q, R, P, lb, ub, U_plan, X_plan, status=None, g_Uplan=None, g_Xplan=None, g_VN=None, x_ref=None,
                        u_ref=None):
        """The gradient of a loss on the whole plan with respect to the model and the given state of every instance, on the face the
        plan reports (lqmpc_plan_grad_batch): U_plan, X_plan and status as a want_plan / want_sens call returned them for the same
        data; g_Uplan (nu, N, Bsz) = d loss / d U_plan, g_Xplan (nx, N + 1, Bsz) = d loss / d X_plan (its stage 0 acts on the given
        state) and g_VN (Bsz,) = d loss / d V_N, any may be None (zero), not all.  Returns {"g_A": (nx, nx, Bsz), "g_B": (nx, nu, Bsz),
        "g_x0": (nx, Bsz)}.  The post-pass alone: no solve."""
        A, B, nx, nu, Bsz = self._dims(A, B)
        Q, R, P = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx))
        lb, ub = _f64(lb, (nu,)), _f64(ub, (nu,))
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        U_plan, X_plan = _f64(U_plan, (nu, N, Bsz)), _f64(X_plan, (nx, N + 1, Bsz))
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int32).reshape(Bsz)
        g_Uplan = None if g_Uplan is None else _f64(g_Uplan, (nu, N, Bsz))
        g_Xplan = None if g_Xplan is None else _f64(g_Xplan, (nx, N + 1, Bsz))
        g_VN = None if g_VN is None else _f64(g_VN, (Bsz,))
        gA = np.empty((nx, nx, Bsz)); gB = np.empty((nx, nu, Bsz)); gx = np.empty((nx, Bsz))
        _lib.check(self._L.lqmpc_plan_grad_batch(self._h, nx, nu, N, Bsz, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(P), _ptr(lb), _ptr(ub),
                                                 _ptr(x_ref), _ptr(u_ref), _ptr(U_plan), _ptr(X_plan), _ptr(status), _ptr(g_Uplan),
                                                 _ptr(g_Xplan), _ptr(g_VN), _ptr(gA), _ptr(gB), _ptr(gx)))
        return {"g_A": gA, "g_B": gB, "g_x0": gx}

    def plan_grad_batch_dev(self, nx, nu, N, Bsz, dA, dB, Q, R, P, lb, ub, dUplan, dXplan, dgA=None, dgB=None, dstatus=None, dgUplan=None,
                            dgXplan=None, dgVN=None, dgx0=None, x_ref=None, u_ref=None):
        """Device pointers / tensors; enqueued on the solver's stream, returns at once (lqmpc_plan_grad_batch_dev).  Any of dgA, dgB,
        dgx0 may be None, not all."""
        Q, R, P, lb, ub = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx)), _f64(lb, (nu,)), _f64(ub, (nu,))
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        _lib.check(self._L.lqmpc_plan_grad_batch_dev(self._h, nx, nu, N, Bsz, _ptr(dA), _ptr(dB), _ptr(Q), _ptr(R), _ptr(P), _ptr(lb),
                                                     _ptr(ub), _ptr(x_ref), _ptr(u_ref), _ptr(dUplan), _ptr(dXplan), _ptr(dstatus),
                                                     _ptr(dgUplan), _ptr(dgXplan), _ptr(dgVN), _ptr(dgA), _ptr(dgB), _ptr(dgx0)))

    def cost_grad_batch(self, N, A, B, Q, R, P, lb, ub, U_plan, X_plan, status=None, g_u0=None, g_VN=None, x_ref=None, u_ref=None,
                        reduce=False):
        """The gradient of a loss on (u_0, V_N) with respect to the data the batch shares -- the weights, the references and the box
        -- on the face the plan reports (lqmpc_cost_grad_batch); arguments as model_grad_batch.  Returns {"g_Q", "g_R", "g_P", "g_lb",
        "g_ub", "g_xref", "g_uref"}: per instance with the instance axis last ((nx, nx, Bsz), ..., (nx, N, Bsz)), or with reduce=True
        the sum over the batch in the shape of the parameter, formed on the GPU in a fixed order, and "skipped", the number of
        instances with status 2, which add nothing.  g_Q, g_R, g_P take the entries of the matrix as independent (they are
        symmetric).  The post-pass alone: no solve."""
        A, B, nx, nu, Bsz = self._dims(A, B)
        Q, R, P = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx))
        lb, ub = _f64(lb, (nu,)), _f64(ub, (nu,))
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        U_plan, X_plan = _f64(U_plan, (nu, N, Bsz)), _f64(X_plan, (nx, N + 1, Bsz))
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int32).reshape(Bsz)
        g_u0 = None if g_u0 is None else _f64(g_u0, (nu, Bsz))
        g_VN = None if g_VN is None else _f64(g_VN, (Bsz,))
        out = _cgrad_outputs(nx, nu, N, Bsz, reduce)
        skipped = np.zeros(1, dtype=np.int64)
        _lib.check(self._L.lqmpc_cost_grad_batch(self._h, nx, nu, N, Bsz, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(P), _ptr(lb), _ptr(ub),
                                                 _ptr(x_ref), _ptr(u_ref), _ptr(U_plan), _ptr(X_plan), _ptr(status), _ptr(g_u0),
                                                 _ptr(g_VN), int(bool(reduce)), *[_ptr(out[k]) for k in _CGRAD_KEYS], _ptr(skipped)))
        if reduce:
            out["skipped"] = int(skipped[0])
        return out

    def cost_grad_batch_dev(self, nx, nu, N, Bsz, dA, dB, Q, R, P, lb, ub, dUplan, dXplan, outs, dstatus=None, dgu0=None, dgVN=None,
                            x_ref=None, u_ref=None, reduce=False, dskipped=None):
        """Device pointers / tensors; enqueued on the solver's stream, returns at once (lqmpc_cost_grad_batch_dev).  outs: a dict
        with any of the keys g_Q, g_R, g_P, g_lb, g_ub, g_xref, g_uref (at least one); dskipped: an int64 device scalar."""
        Q, R, P, lb, ub = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx)), _f64(lb, (nu,)), _f64(ub, (nu,))
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        _lib.check(self._L.lqmpc_cost_grad_batch_dev(self._h, nx, nu, N, Bsz, _ptr(dA), _ptr(dB), _ptr(Q), _ptr(R), _ptr(P), _ptr(lb),
                                                     _ptr(ub), _ptr(x_ref), _ptr(u_ref), _ptr(dUplan), _ptr(dXplan), _ptr(dstatus),
                                                     _ptr(dgu0), _ptr(dgVN), int(bool(reduce)), *_cgrad_dev_ptrs(outs), _ptr(dskipped)))

    def cost_grad_blocks(self, nx, nu, N, Bsz, reduce=True):
        """the number of wavefronts a cost-gradient call is launched with: a function of the shape and Bsz only"""
        return int(self._L.lqmpc_cost_grad_blocks(nx, nu, N, Bsz, int(bool(reduce))))

    def rollout_batch_dev(self, nx, nu, N, Bsz, T, dA, dB, Q, R, P, lb, ub, dx0, A_true, B_true, dJT,
                          dX=None, dU=None, dstatus=None, diters=None, true_per_instance=False, x_ref=None, u_ref=None):
        Q, R, P, lb, ub = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx)), _f64(lb, (nu,)), _f64(ub, (nu,))
        if not true_per_instance:
            A_true, B_true = _f64(A_true, (nx, nx)), _f64(B_true, (nx, nu))
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        _lib.check(self._L.lqmpc_rollout_batch_dev(self._h, nx, nu, N, Bsz, T, _ptr(dA), _ptr(dB), _ptr(Q), _ptr(R), _ptr(P),
                                                   _ptr(lb), _ptr(ub), _ptr(dx0), _ptr(A_true), _ptr(B_true),
                                                   1 if true_per_instance else 0, _ptr(x_ref), _ptr(u_ref),
                                                   _ptr(dJT), _ptr(dX), _ptr(dU), _ptr(dstatus), _ptr(diters)))

    def solve_poly_batch_dev(self, nx, nu, N, Bsz, dA, dB, Q, R, P, F_u, dx0, du0, dVN, dUplan=None, dXplan=None, dlam=None, dstatus=None,
                             diters=None, x_ref=None, u_ref=None, max_iter=0):
        """Device pointers / tensors; enqueued on the solver's stream, returns at once (lqmpc_solve_poly_batch_dev).  dlam is
        (m, N, Bsz)."""
        Q, R, P, F_u = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx)), self._Fu(F_u, nu)
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        _lib.check(self._L.lqmpc_solve_poly_batch_dev(self._h, nx, nu, N, Bsz, _ptr(dA), _ptr(dB), _ptr(Q), _ptr(R), _ptr(P), _ptr(F_u),
                                                      F_u.shape[0], _ptr(dx0), _ptr(x_ref), _ptr(u_ref), int(max_iter), _ptr(du0),
                                                      _ptr(dVN), _ptr(dUplan), _ptr(dXplan), _ptr(dlam), _ptr(dstatus), _ptr(diters)))

    def rollout_poly_batch_dev(self, nx, nu, N, Bsz, T, dA, dB, Q, R, P, F_u, dx0, A_true, B_true, dJT, dX=None, dU=None, dstatus=None,
                               diters=None, true_per_instance=False, x_ref=None, u_ref=None, max_iter=0):
        """Device pointers / tensors; enqueued on the solver's stream, returns at once (lqmpc_rollout_poly_batch_dev)."""
        Q, R, P, F_u = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx)), self._Fu(F_u, nu)
        if not true_per_instance:
            A_true, B_true = _f64(A_true, (nx, nx)), _f64(B_true, (nx, nu))
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        _lib.check(self._L.lqmpc_rollout_poly_batch_dev(self._h, nx, nu, N, Bsz, T, _ptr(dA), _ptr(dB), _ptr(Q), _ptr(R), _ptr(P),
                                                        _ptr(F_u), F_u.shape[0], _ptr(dx0), _ptr(A_true), _ptr(B_true),
                                                        1 if true_per_instance else 0, _ptr(x_ref), _ptr(u_ref), int(max_iter),
                                                        _ptr(dJT), _ptr(dX), _ptr(dU), _ptr(dstatus), _ptr(diters)))

    def rollout_tape_batch_dev(self, nx, nu, N, Bsz, T, dA, dB, Q, R, P, lb, ub, dx0, A_true, B_true, dJT, dUtape, dX=None, dU=None,
                               dstatus=None, diters=None, dstatus_tape=None, true_per_instance=False, x_ref=None, u_ref=None):
        """Device pointers / tensors; enqueued on the solver's stream, returns at once (lqmpc_rollout_tape_batch_dev).  dUtape
        (T, nu, N, Bsz) is required."""
        Q, R, P, lb, ub = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx)), _f64(lb, (nu,)), _f64(ub, (nu,))
        if not true_per_instance:
            A_true, B_true = _f64(A_true, (nx, nx)), _f64(B_true, (nx, nu))
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        _lib.check(self._L.lqmpc_rollout_tape_batch_dev(self._h, nx, nu, N, Bsz, T, _ptr(dA), _ptr(dB), _ptr(Q), _ptr(R), _ptr(P),
                                                        _ptr(lb), _ptr(ub), _ptr(dx0), _ptr(A_true), _ptr(B_true),
                                                        1 if true_per_instance else 0, _ptr(x_ref), _ptr(u_ref), _ptr(dJT), _ptr(dX),
                                                        _ptr(dU), _ptr(dstatus), _ptr(diters), _ptr(dUtape), _ptr(dstatus_tape)))

    def rollout_grad_batch_dev(self, nx, nu, N, Bsz, T, dA, dB, Q, R, P, lb, ub, A_true, B_true, dX, dUtape, dstatus_tape=None, dgJT=None,
                               dgX=None, dgU=None, dgA=None, dgB=None, dgx0=None, dgA_true=None, dgB_true=None, true_per_instance=False,
                               x_ref=None, u_ref=None):
        """Device pointers / tensors; enqueued on the solver's stream, returns at once (lqmpc_rollout_grad_batch_dev).  Any cotangent
        and any output may be None, not all of either; dgA_true and dgB_true are per instance also where the plant is shared."""
        Q, R, P, lb, ub = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx)), _f64(lb, (nu,)), _f64(ub, (nu,))
        if not true_per_instance:
            A_true, B_true = _f64(A_true, (nx, nx)), _f64(B_true, (nx, nu))
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        _lib.check(self._L.lqmpc_rollout_grad_batch_dev(self._h, nx, nu, N, Bsz, T, _ptr(dA), _ptr(dB), _ptr(Q), _ptr(R), _ptr(P),
                                                        _ptr(lb), _ptr(ub), _ptr(A_true), _ptr(B_true), 1 if true_per_instance else 0,
                                                        _ptr(x_ref), _ptr(u_ref), _ptr(dX), _ptr(dUtape), _ptr(dstatus_tape), _ptr(dgJT),
                                                        _ptr(dgX), _ptr(dgU), _ptr(dgA), _ptr(dgB), _ptr(dgx0), _ptr(dgA_true),
                                                        _ptr(dgB_true)))

    def rollout_cost_grad_batch_dev(self, nx, nu, N, Bsz, T, dA, dB, Q, R, P, lb, ub, A_true, B_true, dX, dUtape, outs, dstatus_tape=None,
                                    dgJT=None, dgX=None, dgU=None, true_per_instance=False, x_ref=None, u_ref=None, reduce=False,
                                    dskipped=None):
        """Device pointers / tensors; enqueued on the solver's stream, returns at once (lqmpc_rollout_cost_grad_batch_dev).  outs: a
        dict with any of the keys g_Q, g_R, g_P, g_lb, g_ub, g_xref, g_uref (at least one); dskipped: an int64 device scalar."""
        Q, R, P, lb, ub = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx)), _f64(lb, (nu,)), _f64(ub, (nu,))
        if not true_per_instance:
            A_true, B_true = _f64(A_true, (nx, nx)), _f64(B_true, (nx, nu))
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        _lib.check(self._L.lqmpc_rollout_cost_grad_batch_dev(self._h, nx, nu, N, Bsz, T, _ptr(dA), _ptr(dB), _ptr(Q), _ptr(R), _ptr(P),
                                                             _ptr(lb), _ptr(ub), _ptr(A_true), _ptr(B_true),
                                                             1 if true_per_instance else 0, _ptr(x_ref), _ptr(u_ref), _ptr(dX),
                                                             _ptr(dUtape), _ptr(dstatus_tape), _ptr(dgJT), _ptr(dgX), _ptr(dgU),
                                                             int(bool(reduce)), *_cgrad_dev_ptrs(outs), _ptr(dskipped)))

    def max_vn_batch_dev(self, nx, nu, N, Bsz, dA, dB, Q, R, P, lb, ub, x0s, dMV, dstatus=None, diters=None,
                         x_ref=None, u_ref=None):
        Q, R, P, lb, ub = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx)), _f64(lb, (nu,)), _f64(ub, (nu,))
        x0s = _f64(x0s)
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        _lib.check(self._L.lqmpc_max_vn_batch_dev(self._h, nx, nu, N, Bsz, x0s.shape[1], _ptr(dA), _ptr(dB), _ptr(Q), _ptr(R),
                                                  _ptr(P), _ptr(lb), _ptr(ub), _ptr(x0s), _ptr(x_ref), _ptr(u_ref),
                                                  _ptr(dMV), _ptr(dstatus), _ptr(diters)))

    def sweep_batch_dev(self, nx, nu, N, Bsz, T, dA, dB, Q, R, P, lb, ub, dx0, x0s, A_true, B_true, dJT, dMV,
                        dstatus=None, diters=None, true_per_instance=False, x_ref=None, u_ref=None):
        Q, R, P, lb, ub = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx)), _f64(lb, (nu,)), _f64(ub, (nu,))
        x0s = _f64(x0s)
        if x0s.ndim != 2 or x0s.shape[0] != nx:
            raise ValueError("x0s must be (nx, K)")
        if not true_per_instance:
            A_true, B_true = _f64(A_true, (nx, nx)), _f64(B_true, (nx, nu))
        x_ref, u_ref = _ref_or_none(x_ref, nx, N), _ref_or_none(u_ref, nu, N)
        _lib.check(self._L.lqmpc_sweep_batch_dev(self._h, nx, nu, N, Bsz, T, x0s.shape[1], _ptr(dA), _ptr(dB), _ptr(Q), _ptr(R),
                                                 _ptr(P), _ptr(lb), _ptr(ub), _ptr(dx0), _ptr(x0s), _ptr(A_true), _ptr(B_true),
                                                 1 if true_per_instance else 0, _ptr(x_ref), _ptr(u_ref),
                                                 _ptr(dJT), _ptr(dMV), _ptr(dstatus), _ptr(diters)))

    def bounds_batch_dev(self, nx, nu, N, Bsz, dA, dB, Q, R, lb, ub, de_A, de_B, dMV, x, p, V_expert, dK=None, dalpha=None,
                         dbeta=None, dxi=None, deta=None, dbound=None, deps=None, daux=None, dstatus=None):
        Q, R, lb, ub = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(lb, (nu,)), _f64(ub, (nu,))
        x, p = _f64(x, (nx,)), _f64(p, (3,))
        _lib.check(self._L.lqmpc_bounds_batch_dev(self._h, nx, nu, N, Bsz, _ptr(dA), _ptr(dB), _ptr(Q), _ptr(R), _ptr(lb), _ptr(ub),
                                                  _ptr(de_A), _ptr(de_B), _ptr(dMV), _ptr(x), _ptr(p), float(V_expert),
                                                  _ptr(dK), _ptr(dalpha), _ptr(dbeta), _ptr(dxi), _ptr(deta), _ptr(dbound),
                                                  _ptr(deps), _ptr(daux), _ptr(dstatus)))


class BatchController:
    """A prepared controller for a batch (include/lqmpc.h, lqmpc_controller_*): the per-instance set-up is computed once and
    kept in HBM, every step() solves one box QP per instance at the states it is given.  For closed loops the caller owns
    (a simulator in torch, recorded data, hardware): the states come from outside, only u_0 comes from here.

    A, B: numpy arrays (nx, nx, Bsz) / (nx, nu, Bsz) or device tensors of those shapes (anything with .shape and .data_ptr()).
    The controller runs under the solver's options as they are NOW; it keeps the solver alive and must be closed before it.

    Where the solver runs the 16-lane-row kernels the controller keeps one record per instance.  On the workgroup kernel's shapes
    (32 < N * nu <= 128, e.g. (8, 4, 30)) it does so only if the solver has ctl_wg=1 when the controller is made
    (solver.set_options(ctl_wg=1): 166 KB per instance at (8, 4, 30)); otherwise, and on every other shape, each step is a full
    solve_batch_dev.  `kernel` says which: a record controller's name contains "ctl"."""

    def __init__(self, solver, N, A, B, Q, R, P, lb, ub, x_ref=None, u_ref=None):
        self._c = None
        if not isinstance(solver, BatchSolver):
            raise _lib.LqmpcError("BatchController needs a BatchSolver (one GPU, one stream)")
        self._solver = solver
        self._L = solver._L
        on_device = hasattr(A, "data_ptr")
        if on_device:
            sa, sb = tuple(A.shape), tuple(B.shape)
            if len(sa) != 3 or len(sb) != 3 or sa[0] != sa[1] or sb[0] != sa[0] or sb[2] != sa[2]:
                raise ValueError("A must be (nx,nx,Bsz) and B (nx,nu,Bsz), instance-minor")
            if not (A.is_contiguous() and B.is_contiguous()) or "float64" not in str(A.dtype) or "float64" not in str(B.dtype):
                raise ValueError("device A and B must be contiguous float64")
            nx, nu, Bsz = sa[0], sb[1], sa[2]
        else:
            A, B, nx, nu, Bsz = BatchSolver._dims(A, B)
        self.N, self.nx, self.nu, self.Bsz = int(N), nx, nu, Bsz
        Q, R, P = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx))
        lb, ub = _f64(lb, (nu,)), _f64(ub, (nu,))
        x_ref, u_ref = _ref_or_none(x_ref, nx, self.N), _ref_or_none(u_ref, nu, self.N)
        c = ctypes.c_void_p()
        make = self._L.lqmpc_controller_create_dev if on_device else self._L.lqmpc_controller_create
        _lib.check(make(solver._h, nx, nu, self.N, Bsz, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(P), _ptr(lb), _ptr(ub),
                        _ptr(x_ref), _ptr(u_ref), ctypes.byref(c)))
        self._c = c
        self.model_version = 0                  # counts set_model calls: what a gradient taken later checks its plan against
        self.reference_version = 0              # ... and set_reference calls

    def _live(self):
        if self._c is None or not self._c.value:
            raise _lib.LqmpcError("the controller is closed")
        return self._c

    def step(self, x, want_plan=False, want_sens=False):
        """One QP per instance at the states x (nx, Bsz), host arrays in and out.  want_plan: also "U_plan" (nu, N, Bsz) and
        "X_plan" (nx, N + 1, Bsz) as BatchSolver.solve_batch returns them (lqmpc_controller_step_plan).  want_sens: the plan keys
        and "K_0" (nu, nx, Bsz), "dV_dx" (nx, Bsz), "K_plan" (nu, N, nx, Bsz), the derivatives with respect to x
        (lqmpc_controller_step_sens)."""
        x = _f64(x, (self.nx, self.Bsz))
        u0 = np.empty((self.nu, self.Bsz)); VN = np.empty(self.Bsz)
        status = np.empty(self.Bsz, dtype=np.int32); iters = np.empty(self.Bsz, dtype=np.int32)
        if want_sens:
            Up = np.empty((self.nu, self.N, self.Bsz)); Xp = np.empty((self.nx, self.N + 1, self.Bsz))
            K0 = np.empty((self.nu, self.nx, self.Bsz)); dV = np.empty((self.nx, self.Bsz))
            Kp = np.empty((self.nu, self.N, self.nx, self.Bsz))
            _lib.check(self._L.lqmpc_controller_step_sens(self._live(), _ptr(x), _ptr(u0), _ptr(VN), _ptr(K0), _ptr(dV), _ptr(Kp),
                                                          _ptr(Up), _ptr(Xp), _ptr(status), _ptr(iters)))
            return {"u_0": u0, "V_N": VN, "status": status, "iters": iters, "U_plan": Up, "X_plan": Xp,
                    "K_0": K0, "dV_dx": dV, "K_plan": Kp}
        if want_plan:
            Up = np.empty((self.nu, self.N, self.Bsz)); Xp = np.empty((self.nx, self.N + 1, self.Bsz))
            _lib.check(self._L.lqmpc_controller_step_plan(self._live(), _ptr(x), _ptr(u0), _ptr(VN), _ptr(Up), _ptr(Xp),
                                                          _ptr(status), _ptr(iters)))
            return {"u_0": u0, "V_N": VN, "status": status, "iters": iters, "U_plan": Up, "X_plan": Xp}
        _lib.check(self._L.lqmpc_controller_step(self._live(), _ptr(x), _ptr(u0), _ptr(VN), _ptr(status), _ptr(iters)))
        return {"u_0": u0, "V_N": VN, "status": status, "iters": iters}

    def step_dev(self, dx, du0, dVN=None, dstatus=None, diters=None):
        """Device pointers / tensors; enqueued on the solver's stream, returns at once."""
        _lib.check(self._L.lqmpc_controller_step_dev(self._live(), _ptr(dx), _ptr(du0), _ptr(dVN), _ptr(dstatus), _ptr(diters)))

    def step_plan_dev(self, dx, du0, dUplan, dXplan=None, dVN=None, dstatus=None, diters=None):
        """step_dev, and the whole plan: dUplan (nu, N, Bsz) required, dXplan (nx, N + 1, Bsz) optional."""
        _lib.check(self._L.lqmpc_controller_step_plan_dev(self._live(), _ptr(dx), _ptr(du0), _ptr(dVN), _ptr(dUplan), _ptr(dXplan),
                                                          _ptr(dstatus), _ptr(diters)))

    def step_sens_dev(self, dx, du0, dK0, ddVdx, dKplan=None, dUplan=None, dXplan=None, dVN=None, dstatus=None, diters=None):
        """step_plan_dev, and the derivatives with respect to x: dK0 (nu, nx, Bsz) and ddVdx (nx, Bsz) required, dKplan
        (nu, N, nx, Bsz) and the plan's arrays optional (lqmpc_controller_step_sens_dev)."""
        _lib.check(self._L.lqmpc_controller_step_sens_dev(self._live(), _ptr(dx), _ptr(du0), _ptr(dVN), _ptr(dK0), _ptr(ddVdx),
                                                          _ptr(dKplan), _ptr(dUplan), _ptr(dXplan), _ptr(dstatus), _ptr(diters)))

    def model_grad(self, U_plan, X_plan, status=None, g_u0=None, g_VN=None):
        """BatchSolver.model_grad_batch on the controller's own models and current references, for a plan one of its steps returned
        (lqmpc_controller_model_grad).  Read-only on the controller."""
        nx, nu, N, Bsz = self.nx, self.nu, self.N, self.Bsz
        U_plan, X_plan = _f64(U_plan, (nu, N, Bsz)), _f64(X_plan, (nx, N + 1, Bsz))
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int32).reshape(Bsz)
        g_u0 = None if g_u0 is None else _f64(g_u0, (nu, Bsz))
        g_VN = None if g_VN is None else _f64(g_VN, (Bsz,))
        gA = np.empty((nx, nx, Bsz)); gB = np.empty((nx, nu, Bsz)); gx = np.empty((nx, Bsz))
        _lib.check(self._L.lqmpc_controller_model_grad(self._live(), _ptr(U_plan), _ptr(X_plan), _ptr(status), _ptr(g_u0), _ptr(g_VN),
                                                       _ptr(gA), _ptr(gB), _ptr(gx)))
        return {"g_A": gA, "g_B": gB, "g_x0": gx}

    def model_grad_dev(self, dUplan, dXplan, dgA, dgB, dstatus=None, dgu0=None, dgVN=None, dgx0=None):
        """Device pointers / tensors; enqueued on the solver's stream, returns at once (lqmpc_controller_model_grad_dev)."""
        _lib.check(self._L.lqmpc_controller_model_grad_dev(self._live(), _ptr(dUplan), _ptr(dXplan), _ptr(dstatus), _ptr(dgu0), _ptr(dgVN),
                                                           _ptr(dgA), _ptr(dgB), _ptr(dgx0)))

    def plan_grad(self, U_plan, X_plan, status=None, g_Uplan=None, g_Xplan=None, g_VN=None):
        """BatchSolver.plan_grad_batch on the controller's own models and current references, for a plan one of its steps returned
        (lqmpc_controller_plan_grad).  Read-only on the controller."""
        nx, nu, N, Bsz = self.nx, self.nu, self.N, self.Bsz
        U_plan, X_plan = _f64(U_plan, (nu, N, Bsz)), _f64(X_plan, (nx, N + 1, Bsz))
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int32).reshape(Bsz)
        g_Uplan = None if g_Uplan is None else _f64(g_Uplan, (nu, N, Bsz))
        g_Xplan = None if g_Xplan is None else _f64(g_Xplan, (nx, N + 1, Bsz))
        g_VN = None if g_VN is None else _f64(g_VN, (Bsz,))
        gA = np.empty((nx, nx, Bsz)); gB = np.empty((nx, nu, Bsz)); gx = np.empty((nx, Bsz))
        _lib.check(self._L.lqmpc_controller_plan_grad(self._live(), _ptr(U_plan), _ptr(X_plan), _ptr(status), _ptr(g_Uplan), _ptr(g_Xplan),
                                                      _ptr(g_VN), _ptr(gA), _ptr(gB), _ptr(gx)))
        return {"g_A": gA, "g_B": gB, "g_x0": gx}

    def plan_grad_dev(self, dUplan, dXplan, dgA=None, dgB=None, dstatus=None, dgUplan=None, dgXplan=None, dgVN=None, dgx0=None):
        """Device pointers / tensors; enqueued on the solver's stream, returns at once (lqmpc_controller_plan_grad_dev).  Any of dgA,
        dgB, dgx0 may be None, not all."""
        _lib.check(self._L.lqmpc_controller_plan_grad_dev(self._live(), _ptr(dUplan), _ptr(dXplan), _ptr(dstatus), _ptr(dgUplan),
                                                          _ptr(dgXplan), _ptr(dgVN), _ptr(dgA), _ptr(dgB), _ptr(dgx0)))

    def cost_grad(self, U_plan, X_plan, status=None, g_u0=None, g_VN=None, reduce=False):
        """BatchSolver.cost_grad_batch on the controller's own models, weights, box and current references, for a plan one of its
        steps returned (lqmpc_controller_cost_grad).  Read-only on the controller."""
        nx, nu, N, Bsz = self.nx, self.nu, self.N, self.Bsz
        U_plan, X_plan = _f64(U_plan, (nu, N, Bsz)), _f64(X_plan, (nx, N + 1, Bsz))
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int32).reshape(Bsz)
        g_u0 = None if g_u0 is None else _f64(g_u0, (nu, Bsz))
        g_VN = None if g_VN is None else _f64(g_VN, (Bsz,))
        out = _cgrad_outputs(nx, nu, N, Bsz, reduce)
        skipped = np.zeros(1, dtype=np.int64)
        _lib.check(self._L.lqmpc_controller_cost_grad(self._live(), _ptr(U_plan), _ptr(X_plan), _ptr(status), _ptr(g_u0), _ptr(g_VN),
                                                      int(bool(reduce)), *[_ptr(out[k]) for k in _CGRAD_KEYS], _ptr(skipped)))
        if reduce:
            out["skipped"] = int(skipped[0])
        return out

    def cost_grad_dev(self, dUplan, dXplan, outs, dstatus=None, dgu0=None, dgVN=None, reduce=False, dskipped=None):
        """Device pointers / tensors; enqueued on the solver's stream, returns at once (lqmpc_controller_cost_grad_dev); outs and
        dskipped as BatchSolver.cost_grad_batch_dev."""
        _lib.check(self._L.lqmpc_controller_cost_grad_dev(self._live(), _ptr(dUplan), _ptr(dXplan), _ptr(dstatus), _ptr(dgu0), _ptr(dgVN),
                                                          int(bool(reduce)), *_cgrad_dev_ptrs(outs), _ptr(dskipped)))

    def rollout(self, T, x0, A_true, B_true, want_traj=False):
        """T closed-loop steps of every instance from x0 (nx, Bsz) in one launch, from the controller's present state (its models,
        weights, box and current references): the dict of BatchSolver.rollout_batch.  A_true (nx, nx) / B_true (nx, nu): one plant
        for the batch; (nx, nx, Bsz) / (nx, nu, Bsz): one per instance.  Read-only on the controller: the active sets carried from
        step to step are neither used nor changed."""
        c, nx, nu, Bsz, T = self._live(), self.nx, self.nu, self.Bsz, int(T)
        x0 = _f64(x0, (nx, Bsz))
        A_true, B_true = _f64(A_true), _f64(B_true)
        per_inst = 1 if A_true.ndim == 3 else 0
        if per_inst:
            A_true, B_true = _f64(A_true, (nx, nx, Bsz)), _f64(B_true, (nx, nu, Bsz))
        else:
            A_true, B_true = _f64(A_true, (nx, nx)), _f64(B_true, (nx, nu))
        JT = np.empty(Bsz)
        X = np.empty((nx, T + 1, Bsz)) if want_traj and T >= 1 else None
        U = np.empty((nu, T, Bsz)) if want_traj and T >= 1 else None
        status = np.empty(Bsz, dtype=np.int32); iters = np.empty(Bsz, dtype=np.int32)
        _lib.check(self._L.lqmpc_controller_rollout(c, T, _ptr(x0), _ptr(A_true), _ptr(B_true), per_inst,
                                                    _ptr(JT), _ptr(X), _ptr(U), _ptr(status), _ptr(iters)))
        return {"J_T": JT, "X": X, "U": U, "status": status, "iters": iters}

    def rollout_dev(self, T, dx0, A_true, B_true, dJT, dX=None, dU=None, dstatus=None, diters=None, true_per_instance=False):
        """Device pointers / tensors; enqueued on the solver's stream, returns at once.  A shared plant (true_per_instance=False)
        is a pair of HOST arrays (nx, nx) / (nx, nu); a per-instance plant a pair of device arrays (nx, nx, Bsz) / (nx, nu, Bsz)."""
        if not true_per_instance:
            A_true, B_true = _f64(A_true, (self.nx, self.nx)), _f64(B_true, (self.nx, self.nu))
        _lib.check(self._L.lqmpc_controller_rollout_dev(self._live(), int(T), _ptr(dx0), _ptr(A_true), _ptr(B_true),
                                                        1 if true_per_instance else 0, _ptr(dJT), _ptr(dX), _ptr(dU),
                                                        _ptr(dstatus), _ptr(diters)))

    def reset(self):
        """Forget the active sets carried from the previous step: the next step starts cold."""
        _lib.check(self._L.lqmpc_controller_reset(self._live()))

    def set_reference(self, x_ref=None, u_ref=None):
        """New references (nx, N) / (nu, N) for every later step; None means zeros.  On a record controller one launch rewrites
        the part of the records that depends on them, enqueued on the solver's stream like a step; the arrays are copied before
        this returns.  The carried active sets are kept: they only warm-start the next step (reset() forgets them).  Every call
        raises reference_version by one: a plan taken before it no longer belongs to the controller's references (cost_grad and
        model_grad read those)."""
        c = self._live()
        self.reference_version += 1
        x_ref, u_ref = _ref_or_none(x_ref, self.nx, self.N), _ref_or_none(u_ref, self.nu, self.N)
        _lib.check(self._L.lqmpc_controller_set_reference(c, _ptr(x_ref), _ptr(u_ref)))

    def set_model(self, A, B, idx=None):
        """New models for some or all instances, in place: A (nx, nx, m), B (nx, nu, m), instance-minor over the update, for the
        instances idx (m distinct integers in [0, Bsz); None: all of them in order, m == Bsz).  Numpy arrays: checked here, copied
        before this returns.  Device tensors (.shape, .data_ptr(), contiguous float64; idx an int32 device tensor of length m or
        None): enqueued like a step, returns at once, the caller keeps them alive until the stream has passed and answers for
        "distinct and in range".  Listed instances step with the new model under the current references; the others keep every
        bit, and all carried active sets are kept (reset() forgets them).  Every call raises model_version by one: a plan taken
        before it no longer belongs to the controller's models (model_grad reads those)."""
        c = self._live()
        if hasattr(A, "data_ptr") != hasattr(B, "data_ptr"):
            raise ValueError("A and B must both be numpy arrays or both be device tensors")
        self.model_version += 1
        if not hasattr(A, "data_ptr"):
            A, B, idx, m = _model_update_args(self.nx, self.nu, self.Bsz, A, B, idx)
            _lib.check(self._L.lqmpc_controller_set_model(c, m, _ptr(idx), _ptr(A), _ptr(B)))
            return
        sa, sb = tuple(A.shape), tuple(B.shape)
        if len(sa) != 3 or sa[:2] != (self.nx, self.nx) or sb != (self.nx, self.nu, sa[2]):
            raise ValueError(f"A must be ({self.nx}, {self.nx}, m) and B ({self.nx}, {self.nu}, m), got {sa} and {sb}")
        if not (A.is_contiguous() and B.is_contiguous()) or "float64" not in str(A.dtype) or "float64" not in str(B.dtype):
            raise ValueError("device A and B must be contiguous float64")
        m = sa[2]
        if idx is None:
            if m != self.Bsz:
                raise ValueError(f"idx=None replaces every model: m must be Bsz = {self.Bsz}, got {m}")
        elif not hasattr(idx, "data_ptr") or tuple(idx.shape) != (m,) or "int32" not in str(idx.dtype) or not idx.is_contiguous():
            raise ValueError(f"with device A and B, idx must be a contiguous int32 device tensor of length {m}")
        _lib.check(self._L.lqmpc_controller_set_model_dev(c, m, _ptr(idx), _ptr(A), _ptr(B)))

    @property
    def kernel(self):
        return self._L.lqmpc_controller_kernel(self._live()).decode()

    @property
    def nbytes(self):
        return int(self._L.lqmpc_controller_bytes(self._live()))

    def close(self):
        if getattr(self, "_c", None) is not None and self._c.value:
            if self._solver._h.value:                     # (a closed solver has taken its stream with it: nothing left to wait for)
                self._L.lqmpc_controller_destroy(self._c)
            self._c = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PolyBatchController:
    """A prepared controller for a batch under F_u u_i <= 1, any (m, nu) matrix F_u (include/lqmpc.h, lqmpc_poly_controller_*): the
    per-instance set-up of solve_poly_batch is computed once and kept in HBM, one record per instance; every step() solves one
    polytope QP per instance at the states it is given, in one launch.  For closed loops the caller owns.  A step returns the bits
    solve_poly_batch returns at the same state, and leaves nothing behind: no warm start across steps.

    A, B: numpy arrays (nx, nx, Bsz) / (nx, nu, Bsz) or device tensors of those shapes (anything with .shape and .data_ptr()).
    eps is the solver's option as it is NOW, max_iter is fixed here (0: 10 N nu + 20); the controller keeps the solver alive and
    must be closed before it."""

    def __init__(self, solver, N, A, B, Q, R, P, F_u, x_ref=None, u_ref=None, max_iter=0):
        self._c = None
        if not isinstance(solver, BatchSolver):
            raise _lib.LqmpcError("PolyBatchController needs a BatchSolver (one GPU, one stream)")
        self._solver = solver
        self._L = solver._L
        on_device = hasattr(A, "data_ptr")
        if on_device:
            sa, sb = tuple(A.shape), tuple(B.shape)
            if len(sa) != 3 or len(sb) != 3 or sa[0] != sa[1] or sb[0] != sa[0] or sb[2] != sa[2]:
                raise ValueError("A must be (nx,nx,Bsz) and B (nx,nu,Bsz), instance-minor")
            if not (A.is_contiguous() and B.is_contiguous()) or "float64" not in str(A.dtype) or "float64" not in str(B.dtype):
                raise ValueError("device A and B must be contiguous float64")
            nx, nu, Bsz = sa[0], sb[1], sa[2]
        else:
            A, B, nx, nu, Bsz = BatchSolver._dims(A, B)
        self.N, self.nx, self.nu, self.Bsz = int(N), nx, nu, Bsz
        Q, R, P = _f64(Q, (nx, nx)), _f64(R, (nu, nu)), _f64(P, (nx, nx))
        F_u = BatchSolver._Fu(F_u, nu)
        self.m = F_u.shape[0]
        x_ref, u_ref = _ref_or_none(x_ref, nx, self.N), _ref_or_none(u_ref, nu, self.N)
        c = ctypes.c_void_p()
        make = self._L.lqmpc_poly_controller_create_dev if on_device else self._L.lqmpc_poly_controller_create
        _lib.check(make(solver._h, nx, nu, self.N, Bsz, _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(P), _ptr(F_u), self.m,
                        _ptr(x_ref), _ptr(u_ref), int(max_iter), ctypes.byref(c)))
        self._c = c
        self.model_version = 0                  # counts set_model calls
        self.reference_version = 0              # ... and set_reference calls

    def _live(self):
        if self._c is None or not self._c.value:
            raise _lib.LqmpcError("the controller is closed")
        return self._c

    def step(self, x, want_plan=False, want_lam=False):
        """One polytope QP per instance at the states x (nx, Bsz), host arrays in and out: the dict of
        BatchSolver.solve_poly_batch, bit for bit what it returns at x0 = x."""
        c, nx, nu, N, Bsz = self._live(), self.nx, self.nu, self.N, self.Bsz
        x = _f64(x, (nx, Bsz))
        u0 = np.empty((nu, Bsz)); VN = np.empty(Bsz)
        status = np.empty(Bsz, dtype=np.int32); iters = np.empty(Bsz, dtype=np.int32)
        Up = np.empty((nu, N, Bsz)) if want_plan else None
        Xp = np.empty((nx, N + 1, Bsz)) if want_plan else None
        lam = np.empty((self.m, N, Bsz)) if want_lam else None
        _lib.check(self._L.lqmpc_poly_controller_step(c, _ptr(x), _ptr(u0), _ptr(VN), _ptr(Up), _ptr(Xp), _ptr(lam), _ptr(status),
                                                      _ptr(iters)))
        out = {"u_0": u0, "V_N": VN, "status": status, "iters": iters}
        if want_plan:
            out["U_plan"], out["X_plan"] = Up, Xp
        if want_lam:
            out["lam"] = lam
        return out

    def step_dev(self, dx, du0, dVN=None, dUplan=None, dXplan=None, dlam=None, dstatus=None, diters=None):
        """Device pointers / tensors; one launch enqueued on the solver's stream, returns at once.  dlam is (m, N, Bsz)."""
        _lib.check(self._L.lqmpc_poly_controller_step_dev(self._live(), _ptr(dx), _ptr(du0), _ptr(dVN), _ptr(dUplan), _ptr(dXplan),
                                                          _ptr(dlam), _ptr(dstatus), _ptr(diters)))

    def rollout(self, T, x0, A_true, B_true, want_traj=False):
        """T closed-loop steps of every instance from x0 (nx, Bsz) in one launch, from the controller's records and current
        references: the dict of BatchSolver.rollout_poly_batch, bit for bit.  A_true (nx, nx) / B_true (nx, nu): one plant for the
        batch; (nx, nx, Bsz) / (nx, nu, Bsz): one per instance.  Read-only on the controller."""
        c, nx, nu, Bsz, T = self._live(), self.nx, self.nu, self.Bsz, int(T)
        x0 = _f64(x0, (nx, Bsz))
        A_true, B_true, per_inst = BatchSolver._plant(A_true, B_true, nx, nu, Bsz)
        JT = np.empty(Bsz)
        X = np.empty((nx, T + 1, Bsz)) if want_traj and T >= 1 else None
        U = np.empty((nu, T, Bsz)) if want_traj and T >= 1 else None
        status = np.empty(Bsz, dtype=np.int32); iters = np.empty(Bsz, dtype=np.int32)
        _lib.check(self._L.lqmpc_poly_controller_rollout(c, T, _ptr(x0), _ptr(A_true), _ptr(B_true), per_inst,
                                                         _ptr(JT), _ptr(X), _ptr(U), _ptr(status), _ptr(iters)))
        return {"J_T": JT, "X": X, "U": U, "status": status, "iters": iters}

    def rollout_dev(self, T, dx0, A_true, B_true, dJT, dX=None, dU=None, dstatus=None, diters=None, true_per_instance=False):
        """Device pointers / tensors; enqueued on the solver's stream, returns at once.  A shared plant (true_per_instance=False)
        is a pair of HOST arrays (nx, nx) / (nx, nu); a per-instance plant a pair of device arrays (nx, nx, Bsz) / (nx, nu, Bsz)."""
        if not true_per_instance:
            A_true, B_true = _f64(A_true, (self.nx, self.nx)), _f64(B_true, (self.nx, self.nu))
        _lib.check(self._L.lqmpc_poly_controller_rollout_dev(self._live(), int(T), _ptr(dx0), _ptr(A_true), _ptr(B_true),
                                                             1 if true_per_instance else 0, _ptr(dJT), _ptr(dX), _ptr(dU),
                                                             _ptr(dstatus), _ptr(diters)))

    def set_reference(self, x_ref=None, u_ref=None):
        """New references (nx, N) / (nu, N) for every later step and rollout; None means zeros.  No record depends on them, so no
        kernel runs: one copy on the solver's stream, ordered with the steps; the arrays are copied before this returns.  Every call
        raises reference_version by one."""
        c = self._live()
        self.reference_version += 1
        x_ref, u_ref = _ref_or_none(x_ref, self.nx, self.N), _ref_or_none(u_ref, self.nu, self.N)
        _lib.check(self._L.lqmpc_poly_controller_set_reference(c, _ptr(x_ref), _ptr(u_ref)))

    def set_model(self, A, B, idx=None):
        """New models for some or all instances, in place, as BatchController.set_model takes them: A (nx, nx, m), B (nx, nu, m),
        instance-minor over the update, for the instances idx (m distinct integers in [0, Bsz); None: all of them in order).  Numpy
        arrays: checked here, copied before this returns.  Device tensors (idx an int32 device tensor of length m or None): enqueued
        like a step, returns at once.  The listed records are factored again; the others keep every bit.  Every call raises
        model_version by one."""
        c = self._live()
        if hasattr(A, "data_ptr") != hasattr(B, "data_ptr"):
            raise ValueError("A and B must both be numpy arrays or both be device tensors")
        self.model_version += 1
        if not hasattr(A, "data_ptr"):
            A, B, idx, m = _model_update_args(self.nx, self.nu, self.Bsz, A, B, idx)
            _lib.check(self._L.lqmpc_poly_controller_set_model(c, m, _ptr(idx), _ptr(A), _ptr(B)))
            return
        sa, sb = tuple(A.shape), tuple(B.shape)
        if len(sa) != 3 or sa[:2] != (self.nx, self.nx) or sb != (self.nx, self.nu, sa[2]):
            raise ValueError(f"A must be ({self.nx}, {self.nx}, m) and B ({self.nx}, {self.nu}, m), got {sa} and {sb}")
        if not (A.is_contiguous() and B.is_contiguous()) or "float64" not in str(A.dtype) or "float64" not in str(B.dtype):
            raise ValueError("device A and B must be contiguous float64")
        m = sa[2]
        if idx is None:
            if m != self.Bsz:
                raise ValueError(f"idx=None replaces every model: m must be Bsz = {self.Bsz}, got {m}")
        elif not hasattr(idx, "data_ptr") or tuple(idx.shape) != (m,) or "int32" not in str(idx.dtype) or not idx.is_contiguous():
            raise ValueError(f"with device A and B, idx must be a contiguous int32 device tensor of length {m}")
        _lib.check(self._L.lqmpc_poly_controller_set_model_dev(c, m, _ptr(idx), _ptr(A), _ptr(B)))

    @property
    def kernel(self):
        return self._L.lqmpc_poly_controller_kernel(self._live()).decode()

    @property
    def nbytes(self):
        return int(self._L.lqmpc_poly_controller_bytes(self._live()))

    def close(self):
        if getattr(self, "_c", None) is not None and self._c.value:
            if self._solver._h.value:                     # (a closed solver has taken its stream with it: nothing left to wait for)
                self._L.lqmpc_poly_controller_destroy(self._c)
            self._c = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PlanVariable:
    """Stands where the reference keeps its cp.Variable: `.value` is None before the first solve, then the optimal plan."""

    def __init__(self):
        self.value = None


_default_solver = None


def default_solver():
    """Process-wide solver on GPU 0 used by the single-instance classes below."""
    global _default_solver
    if _default_solver is None:
        _default_solver = BatchSolver(0)
    return _default_solver


class LQ_MPC_Controller:
    """Open-loop LQ MPC solve; drop-in for utils_class.py:18-91.  An F_u whose rows have one non-zero each is a box and runs on the
    box kernels; a row with two or more makes it a polytope, served by solve_poly_batch (local_law is not: NotImplementedError)."""

    def __init__(self, N, A, B, Q, R, P, F_u, solver=None):
        self.N = int(N)
        self.A = np.asarray(A, dtype=np.float64)
        self.B = np.asarray(B, dtype=np.float64)
        self.Q = np.asarray(Q, dtype=np.float64)
        self.R = np.asarray(R, dtype=np.float64)
        self.P = np.asarray(P, dtype=np.float64)
        self.F_u = np.asarray(F_u, dtype=np.float64)
        self.poly = not is_box_Fu(self.F_u)
        self.lb, self.ub = (None, None) if self.poly else box_from_Fu(self.F_u)
        self._solver = solver
        # the decision variable of utils_class.py:46: after solve(), u.value is the (nu, N) optimal plan of that call
        self.u = PlanVariable()

    def _s(self):
        return self._solver if self._solver is not None else default_solver()

    def solve(self, x0, x_ref, u_ref):
        """Returns {'u_0': (nu,) ndarray, 'V_N': float} as utils_class.py:91."""
        nx = self.A.shape[0]
        x0 = np.asarray(x0, dtype=np.float64).reshape(nx, 1)
        if self.poly:
            out = self._s().solve_poly_batch(self.N, self.A[:, :, None], self.B[:, :, None], self.Q, self.R, self.P, self.F_u, x0,
                                             x_ref, u_ref, want_plan=True)
        else:
            out = self._s().solve_batch(self.N, self.A[:, :, None], self.B[:, :, None], self.Q, self.R, self.P,
                                        self.lb, self.ub, x0, x_ref, u_ref, want_plan=True)
        self.last_status = int(out["status"][0])
        self.u.value = out["U_plan"][:, :, 0].copy()
        return {"u_0": out["u_0"][:, 0].copy(), "V_N": float(out["V_N"][0])}

    def local_law(self, x0, x_ref, u_ref):
        """Additive: the affine law the controller follows around x0, u_0 = K_0 x + k_0 for x in the critical region of x0.
        Returns (K_0, k_0) as (nu, nx) and (nu,) arrays; u.value becomes the plan at x0, as after solve()."""
        if self.poly:
            raise NotImplementedError("local_law serves a box-shaped F_u only: the sens calls do not cover a polytope (a row of F_u "
                                      "with two or more non-zeros)")
        nx = self.A.shape[0]
        x0 = np.asarray(x0, dtype=np.float64).reshape(nx, 1)
        out = self._s().solve_batch(self.N, self.A[:, :, None], self.B[:, :, None], self.Q, self.R, self.P,
                                    self.lb, self.ub, x0, x_ref, u_ref, want_sens=True)
        self.last_status = int(out["status"][0])
        self.u.value = out["U_plan"][:, :, 0].copy()
        K0 = out["K_0"][:, :, 0].copy()
        return K0, out["u_0"][:, 0] - K0 @ x0[:, 0]

    def solve_many(self, x0s, x_ref=None, u_ref=None):
        """Additive: K initial states of one system in one launch -> {'u_0': (nu,K), 'V_N': (K,)}; u.value becomes (nu, N, K)."""
        x0s = np.asarray(x0s, dtype=np.float64)
        K = x0s.shape[1]
        A = np.repeat(self.A[:, :, None], K, 2)
        B = np.repeat(self.B[:, :, None], K, 2)
        if self.poly:
            out = self._s().solve_poly_batch(self.N, A, B, self.Q, self.R, self.P, self.F_u, x0s, x_ref, u_ref, want_plan=True)
        else:
            out = self._s().solve_batch(self.N, A, B, self.Q, self.R, self.P, self.lb, self.ub, x0s, x_ref, u_ref, want_plan=True)
        self.u.value = out["U_plan"]
        return {"u_0": out["u_0"], "V_N": out["V_N"], "status": out["status"]}


class LQ_MPC_Simulator:
    """Closed-loop MPC rollout; drop-in for utils_class.py:213-285."""

    def __init__(self, T, N, A, B, Q, R, P, F_u, solver=None):
        self.T = int(T)
        self.N = int(N)
        self.A = np.asarray(A, dtype=np.float64)
        self.B = np.asarray(B, dtype=np.float64)
        self.Q = np.asarray(Q, dtype=np.float64)
        self.R = np.asarray(R, dtype=np.float64)
        self.P = np.asarray(P, dtype=np.float64)
        self.F_u = np.asarray(F_u, dtype=np.float64)
        self.poly = not is_box_Fu(self.F_u)          # a row with two or more non-zeros: rollout_poly_batch
        self.lb, self.ub = (None, None) if self.poly else box_from_Fu(self.F_u)
        self.U = np.zeros((self.B.shape[1], self.T))
        self.X = np.zeros((self.A.shape[1], self.T + 1))
        self._solver = solver

    def simulate(self, x0, A_true, B_true, x_ref, u_ref):
        """Returns {'X': (nx,T+1), 'U': (nu,T), 'J_T': float} as utils_class.py:285 (fresh arrays)."""
        s = self._solver if self._solver is not None else default_solver()
        nx = self.A.shape[0]
        x0 = np.asarray(x0, dtype=np.float64).reshape(nx, 1)
        if self.poly:
            out = s.rollout_poly_batch(self.T, self.N, self.A[:, :, None], self.B[:, :, None], self.Q, self.R, self.P, self.F_u, x0,
                                       np.asarray(A_true, dtype=np.float64), np.asarray(B_true, dtype=np.float64), x_ref, u_ref,
                                       want_traj=True)
        else:
            out = s.rollout_batch(self.T, self.N, self.A[:, :, None], self.B[:, :, None], self.Q, self.R, self.P,
                                  self.lb, self.ub, x0, np.asarray(A_true, dtype=np.float64),
                                  np.asarray(B_true, dtype=np.float64), x_ref, u_ref, want_traj=True)
        self.X = out["X"][:, :, 0].copy()
        self.U = out["U"][:, :, 0].copy()
        self.last_status = int(out["status"][0])
        return {"X": self.X, "U": self.U, "J_T": float(out["J_T"][0])}
