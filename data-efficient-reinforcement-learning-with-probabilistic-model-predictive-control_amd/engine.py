"""Thin object wrapper over the C ABI: device memory and streams come from PyTorch-ROCm,
all arithmetic happens in libgpmpc_hip.so."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L


def _host(a, shape=None):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if shape is not None and a.shape != tuple(shape):
        raise ValueError(f"expected shape {tuple(shape)}, got {a.shape}")
    return a


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


def _ptr(t):
    """The address of a device tensor, None (NULL) for None."""
    return t.data_ptr() if t is not None else None


def feedback_gains_layout(shape, B, H, A, D):
    """How a feedback-gain array of `shape` reaches gpmpc_rollout_linear_feedback: (per_candidate, every_step).  (A, D) is one
    gain for every step (every_step: broadcast over H, passed as shared), (H, A, D) a shared sequence, (B, H, A, D) one sequence
    per candidate; anything else raises ValueError."""
    shape = tuple(int(s) for s in shape)
    if shape == (A, D):
        return False, True
    if shape == (H, A, D):
        return False, False
    if shape == (B, H, A, D):
        return True, False
    raise ValueError(f"feedback gains must have shape (A, D) = {(A, D)}, (H, A, D) = {(H, A, D)} or (B, H, A, D) = "
                     f"{(B, H, A, D)}, got {shape}")


class _HostEvaluationPlan:
    """Per (H, A): staging arrays of gpmpc_objective_grad_host's inputs, the layout of its result buffer and a view of it."""

    def __init__(self, H, A, D):
        self.actions, self.mu0, self.S0 = np.empty((H, A)), np.empty(D), np.empty((D, D))
        self.p_actions, self.p_mu0, self.p_S0 = (C.c_void_p(a.ctypes.data) for a in (self.actions, self.mu0, self.S0))
        self.res = C.POINTER(C.c_double)()
        self.res_ref = C.byref(self.res)
        self.n = 1 + H * A + (H + 1) * (D + D * D + 2)
        o = [int(v) for v in np.cumsum([0, 1, H * A, (H + 1) * D, (H + 1) * D * D, H + 1, H + 1])]
        shapes = [(1,), (1, H, A), (1, H + 1, D), (1, H + 1, D, D), (1, H + 1), (1, H + 1)]
        self.fields = [(k, o[i], o[i + 1], shapes[i]) for i, k in enumerate(("J", "grad", "mu", "Sig", "cost_mu", "cost_var"))]
        self.addr, self.view = None, None

    def result(self):
        addr = C.cast(self.res, C.c_void_p).value
        if addr != self.addr:                  # the library's pinned buffer (moves only when it grows)
            self.addr, self.view = addr, np.ctypeslib.as_array(self.res, shape=(self.n,))
        flat = self.view.copy()                # the buffer is reused by the next evaluation
        return {k: flat[lo:hi].reshape(sh) for k, lo, hi, sh in self.fields}


class HipEngine:
    """One handle per GPU (gpmpc_create).  All tensors are fp64 on ``device``."""

    def __init__(self, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("HipEngine needs a ROCm GPU: the GP-MPC hot path has no CPU fallback")
        self.lib = L.lib()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        h = C.c_void_p()
        rc = self.lib.gpmpc_create(C.byref(h), self.device.index)
        if rc != L.GPMPC_OK:
            raise L.GpmpcError(rc, "gpmpc_create failed")
        self._h = h
        self._ogh_plans = {}
        self.N = self.D = self.E = 0
        self._cost = None

    def close(self):
        if getattr(self, "_h", None):
            self.lib.gpmpc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers ---------------------------------------------------------------------
    def _check(self, rc):
        if rc == L.GPMPC_OK:
            return
        msg = self.lib.gpmpc_last_error(self._h).decode()
        if rc == L.GPMPC_ERR_NOT_PD:
            raise L.NotPositiveDefiniteError(rc, msg)
        raise L.GpmpcError(rc, msg)

    def _dev(self, t, shape=None):
        t = torch.as_tensor(t, dtype=torch.float64).to(self.device).contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _rows(self, X, what, rows):
        """X on the device, checked to be a matrix: (`rows`, E) `what`."""
        X = self._dev(X)
        if X.dim() != 2:
            raise ValueError(f"expected {what} of shape ({rows}, E), got {tuple(X.shape)}")
        return X

    def set_option(self, name, value):
        self._check(self.lib.gpmpc_set_option(self._h, name.encode(), int(value)))

    # -- a1/a2 -------------------------------------------------------------------------
    def prepare(self, X, Y, lengthscales, outputscales, noises):
        X = self._dev(X)
        N, E = X.shape
        Y = self._dev(Y)
        D = Y.shape[1]
        ls = self._dev(lengthscales, (D, E))
        osc = self._dev(outputscales).reshape(D)
        nz = self._dev(noises).reshape(D)
        self._keep = (X, Y, ls, osc, nz)
        self._check(self.lib.gpmpc_prepare(self._h, X.data_ptr(), Y.data_ptr(), ls.data_ptr(), osc.data_ptr(),
                                           nz.data_ptr(), N, D, E, self._stream()))
        self.N, self.D, self.E = N, D, E

    def prepare_sparse(self, X, Y, Z, lengthscales, outputscales, noises, jitter_rel=1e-6):
        """A sparse GP (DTC / projected process) of the memory (X (N, E), Y (N, D)) on the inducing inputs Z (M, E)
        (gpmpc_prepare_sparse): afterwards the engine holds an M-point model -- `factors()` returns iK_eff (D, M, M) and
        beta_eff (D, M), and predict, moments, the rollouts, their gradients and the searches run on it unchanged at the cost of
        an M-point memory.  `jitter_rel` times the outputscale goes on the diagonal of k(Z, Z).  There is no (X, Y) record:
        `forget` raises GpmpcError(GPMPC_ERR_ARG) and the next `prepare` factorises in full.  `last_prepare_mode` is 4.
        Synchronises the current stream."""
        X = self._dev(X)
        N, E = X.shape
        Y = self._dev(Y)
        D = Y.shape[1]
        if Y.shape[0] != N:
            raise ValueError(f"expected targets of shape ({N}, D), got {tuple(Y.shape)}")
        Z = self._dev(Z)
        if Z.dim() != 2 or Z.shape[1] != E:
            raise ValueError(f"expected inducing inputs of shape (M, {E}), got {tuple(Z.shape)}")
        M = Z.shape[0]
        ls = self._dev(lengthscales, (D, E))
        osc = self._dev(outputscales).reshape(D)
        nz = self._dev(noises).reshape(D)
        self._keep = (X, Y, Z, ls, osc, nz)
        self._check(self.lib.gpmpc_prepare_sparse(self._h, X.data_ptr(), Y.data_ptr(), N, Z.data_ptr(), M, ls.data_ptr(),
                                                  osc.data_ptr(), nz.data_ptr(), float(jitter_rel), D, E, self._stream()))
        self.N, self.D, self.E = M, D, E

    def _sparse_update(self, entry, X, Y):
        """The argument checks and the call `sparse_append` and `sparse_forget` share; returns the device tensors passed."""
        X = self._dev(X)
        Y = self._dev(Y)
        if X.dim() != 2 or Y.dim() != 2 or X.shape[0] != Y.shape[0]:
            raise ValueError(f"expected inputs (k, E) and targets (k, D), got {tuple(X.shape)} and {tuple(Y.shape)}")
        k, E = X.shape
        D = Y.shape[1]
        self._check(entry(self._h, X.data_ptr(), Y.data_ptr(), int(k), int(D), int(E), self._stream()))
        return X, Y

    def sparse_append(self, X_new, Y_new):
        """Append the memory points (X_new (k, E), Y_new (k, D)) to the sparse model of the last `prepare_sparse`
        (gpmpc_sparse_append): same inducing inputs, hyper-parameters and jitter, O(k M^2) per output, nothing of size N touched.
        Afterwards the engine is in the state `prepare_sparse` would leave for the old memory followed by these rows, up to
        rounding; calls chain.  `last_prepare_mode` is 5.  Nothing synchronises: the update is ordered on the current stream.
        An engine without the record of a `prepare_sparse` (after `prepare`, `set_factors`, `mll`), k = 0 or other shapes than the
        model's: GpmpcError(GPMPC_ERR_ARG), the cached model untouched."""
        self._keep_append = self._sparse_update(self.lib.gpmpc_sparse_append, X_new, Y_new)    # inputs of launches that may still be in flight

    def sparse_forget(self, X_old, Y_old):
        """Remove the memory points whose VALUES are (X_old (k, E), Y_old (k, D)) from the sparse model of the last
        `prepare_sparse` / `sparse_append` (gpmpc_sparse_forget): same inducing inputs, hyper-parameters and jitter, O(k M^2) per
        output, nothing of size N touched.  Afterwards the engine is in the state `prepare_sparse` would leave for the memory
        without these rows, up to rounding; forgets and appends chain in any order.  `last_prepare_mode` is 6.  Synchronises the
        current stream, so the inputs need not be kept alive.  The engine cannot know whether a row is in the model: one that
        never was either loses the pivot or silently leaves the model of "the memory minus a phantom point".
        An engine without the record of a `prepare_sparse`, k = 0 or other shapes than the model's: GpmpcError(GPMPC_ERR_ARG), the
        cached model untouched.  A lost pivot: GpmpcError(GPMPC_ERR_NOT_PD), and the engine holds no model -- prepare again."""
        self._sparse_update(self.lib.gpmpc_sparse_forget, X_old, Y_old)

    def select_inducing(self, X, M, lengthscales, outputscales, jitter_rel=1e-6):
        """Choose M of the memory points X (N, E) as inducing inputs for `prepare_sparse` by greedy variance selection
        (gpmpc_select_inducing: a pivoted partial Cholesky of the D kernel matrices in lockstep, each step picking the point the
        inducing set so far explains worst).  Returns DEVICE tensors {"idx": int32 (M,) the picks, distinct, idx[0] == 0;
        "Z": (M, E) = X[idx] bit for bit; "trace": (M,) sum_a tr(K_a - Q_a) / outputscale_a after each pick}.  The choice depends
        on the inputs and the kernel alone (no targets, no noise); outputs whose residual at a pick is not above `jitter_rel`
        times their outputscale skip that step.  The cached model is neither needed nor touched, `last_prepare_mode` stays, and
        nothing synchronises: the results are ordered on the current stream."""
        X = self._dev(X)
        if X.dim() != 2:
            raise ValueError(f"expected inputs of shape (N, E), got {tuple(X.shape)}")
        N, E = X.shape
        ls = self._dev(lengthscales)
        if ls.dim() != 2 or ls.shape[1] != E:
            raise ValueError(f"expected lengthscales of shape (D, {E}), got {tuple(ls.shape)}")
        D = ls.shape[0]
        osc = self._dev(outputscales).reshape(-1)
        if osc.numel() != D:
            raise ValueError(f"expected {D} outputscales, got {osc.numel()}")
        M = int(M)
        idx = torch.empty(max(M, 0), dtype=torch.int32, device=self.device)
        Z = torch.empty((max(M, 0), E), dtype=torch.float64, device=self.device)
        trace = torch.empty(max(M, 0), dtype=torch.float64, device=self.device)
        self._check(self.lib.gpmpc_select_inducing(self._h, X.data_ptr(), N, M, ls.data_ptr(), osc.data_ptr(), float(jitter_rel),
                                                   D, E, idx.data_ptr(), Z.data_ptr(), trace.data_ptr(), self._stream()))
        self._keep_select = (X, ls, osc)               # inputs of launches that may still be in flight
        return {"idx": idx, "Z": Z, "trace": trace}

    def mll(self, X, Y, lengthscales, outputscales, noises):
        """Training loss of the D GPs and its gradient (gp_model.py:262-275): dict(loss (D,), d_lengthscale (D,E),
        d_outputscale (D,), d_noise (D,)) as numpy arrays.  Replaces the cached factors of this engine."""
        X = self._dev(X)
        N, E = X.shape
        Y = self._dev(Y)
        D = Y.shape[1]
        ls = self._dev(lengthscales, (D, E))
        osc = self._dev(outputscales).reshape(D)
        nz = self._dev(noises).reshape(D)
        out = np.empty((D, E + 3), dtype=np.float64)
        self._check(self.lib.gpmpc_mll(self._h, X.data_ptr(), Y.data_ptr(), ls.data_ptr(), osc.data_ptr(), nz.data_ptr(),
                                       N, D, E, out.ctypes.data_as(C.POINTER(C.c_double)), self._stream()))
        self.N, self.D, self.E = N, D, E
        return {"loss": out[:, 0].copy(), "d_lengthscale": out[:, 1:1 + E].copy(), "d_outputscale": out[:, 1 + E].copy(),
                "d_noise": out[:, 2 + E].copy()}

    def forget(self, indices):
        """Remove the memory points `indices` (strictly ascending rows of the X / Y of the last `prepare`) from the cached
        model (gpmpc_forget): afterwards the engine is in the state `prepare` would leave for the reduced memory, so a
        `prepare` of the reduced memory plus a few appended points is a border update.  O(k N^2), synchronises the current
        stream.  `last_prepare_mode` is 3 (downdate), or 0 where the reduced memory was factorised in full (refresh interval,
        "incremental" = 0).  Bad indices, or an engine without the record of a `prepare`: GpmpcError(GPMPC_ERR_ARG), the
        cached model untouched."""
        idx = np.asarray(indices).reshape(-1)
        if idx.size and not np.issubdtype(idx.dtype, np.integer):
            raise TypeError("forget: indices must be integers")
        # (clipped so that an index beyond 32 bits stays out of range instead of wrapping into it)
        idx = np.ascontiguousarray(np.clip(idx, -1, 2 ** 31 - 1), dtype=np.int32)
        self._check(self.lib.gpmpc_forget(self._h, idx.ctypes.data_as(C.POINTER(C.c_int)), int(idx.size), self._stream()))
        self.N -= int(idx.size)

    @property
    def last_prepare_mode(self):
        """0 = full factorisation, 1 = border update of the cached factors, 2 = cache hit, 3 = downdate (`forget`),
        4 = sparse model (`prepare_sparse`), 5 = points appended to a sparse model (`sparse_append`),
        6 = points removed from a sparse model (`sparse_forget`)."""
        return int(self.lib.gpmpc_last_prepare_mode(self._h))

    @property
    def last_rollout_path(self):
        """Kernels of the last forward pass: 0 = fused-horizon kernel, 1 = streaming kernel, 2 = batch-major tiles."""
        return int(self.lib.gpmpc_last_rollout_path(self._h))

    @property
    def last_cluster(self):
        """Workgroups per candidate of the last fused-horizon launch (1 = the plain kernel; > 1 = the few-candidate cooperative form)."""
        return int(self.lib.gpmpc_last_cluster(self._h))

    @property
    def last_pair_groups(self):
        """Groups of output pairs the last fused-horizon / batch-major launch walked per horizon step (1 = all pairs in one pass)."""
        return int(self.lib.gpmpc_last_pair_groups(self._h))

    @property
    def last_grad_path(self):
        """Moment passes of the last `rollout_grad` (bit mask): 1 separable off-diagonal pairs, 2 tile moments of the diagonal
        pairs, 4 streaming element-wise pass, 8 the 8 < D <= 16 pass, 16 tile moments formed inside the batch-major forward."""
        return int(self.lib.gpmpc_last_grad_path(self._h))

    @property
    def build_id(self):
        """Hash over the sources the loaded library was built from (gpmpc_build_id)."""
        return self.lib.gpmpc_build_id().decode()

    def set_factors(self, X, iK, beta, lengthscales, outputscales):
        X = self._dev(X)
        N, E = X.shape
        beta = self._dev(beta)
        D = beta.shape[0]
        iK = self._dev(iK, (D, N, N))
        ls = self._dev(lengthscales, (D, E))
        osc = self._dev(outputscales).reshape(D)
        self._check(self.lib.gpmpc_set_factors(self._h, X.data_ptr(), iK.data_ptr(), beta.data_ptr(), ls.data_ptr(),
                                               osc.data_ptr(), N, D, E, self._stream()))
        torch.cuda.current_stream(self.device).synchronize()
        self.N, self.D, self.E = N, D, E

    def factors(self):
        iK = torch.empty((self.D, self.N, self.N), dtype=torch.float64, device=self.device)
        beta = torch.empty((self.D, self.N), dtype=torch.float64, device=self.device)
        self._check(self.lib.gpmpc_read_factors(self._h, iK.data_ptr(), beta.data_ptr(), self._stream()))
        return iK, beta

    def predict(self, Xq, noises=None, mean=True, var=True):
        """GP posterior at the query inputs Xq (M, E) from the cached model: dict(mean (M, D), var (M, D)) of device tensors
        (only the requested ones).  `noises` (D,): added to the variance, as likelihood(model(x)) does.  Asynchronous on the
        current stream."""
        Xq = self._rows(Xq, "query inputs", "M")
        M, E = Xq.shape
        D = self.D
        nz = _host(noises, (D,)) if noises is not None else None
        out = {}
        if mean:
            out["mean"] = torch.empty((M, D), dtype=torch.float64, device=self.device)
        if var:
            out["var"] = torch.empty((M, D), dtype=torch.float64, device=self.device)
        self._check(self.lib.gpmpc_predict(self._h, Xq.data_ptr(), M, D, E, _hp(nz) if nz is not None else None,
                                           _ptr(out.get("mean")), _ptr(out.get("var")), self._stream()))
        self._keep_predict = Xq              # alive until the asynchronous call has read it
        return out

    def predict_backward(self, Xq, mean_bar=None, var_bar=None):
        """Reverse-mode product of `predict` (autograd through likelihood(model(x)) with respect to x): Xq (M, E), upstream
        gradients mean_bar (M, D) and var_bar (M, D), each None for zero -> Xq_bar (M, E), a device tensor.  The noise added
        by `predict` is a constant and takes no part.  Without var_bar no matrix product runs.  Asynchronous on the current
        stream."""
        Xq = self._rows(Xq, "query inputs", "M")
        M, E = Xq.shape
        D = self.D
        mb = self._dev(mean_bar, (M, D)) if mean_bar is not None else None
        vb = self._dev(var_bar, (M, D)) if var_bar is not None else None
        out = torch.empty((M, E), dtype=torch.float64, device=self.device)
        self._check(self.lib.gpmpc_predict_backward(self._h, Xq.data_ptr(), M, D, E, _ptr(mb), _ptr(vb), out.data_ptr(),
                                                    self._stream()))
        self._keep_predict_backward = (Xq, mb, vb)   # alive until the asynchronous call has read them
        return out

    def predict_cov(self, Xa, Xb=None, noises=None):
        """Joint GP posterior covariance between query points from the cached model (gpmpc_predict_cov), a device tensor.
        Cross form, Xa (Ma, E) and Xb (Mb, E): (D, Ma, Mb), element [a, i, j] the covariance of output a at xa_i and xb_j;
        `noises` must be None.  Joint form, Xb None: (D, Ma, Ma), the exactly symmetric covariance matrix of the set, whose
        diagonal is `predict`'s variance; `noises` (D,) is added to the diagonal, as likelihood(model(x)) does.  Not clamped,
        no jitter.  Asynchronous on the current stream."""
        Xa = self._rows(Xa, "query inputs", "Ma")
        Ma, E = Xa.shape
        D = self.D
        Mb = Ma
        if Xb is not None:
            Xb = self._dev(Xb)
            if Xb.dim() != 2 or Xb.shape[1] != E:
                raise ValueError(f"expected query inputs of shape (Mb, {E}), got {tuple(Xb.shape)}")
            Mb = Xb.shape[0]
        nz = _host(noises, (D,)) if noises is not None else None
        out = torch.empty((D, Ma, Mb), dtype=torch.float64, device=self.device)
        if Xb is not None and Mb == 0:       # an empty tensor has no address: the library would read the NULL as the joint form
            return out
        self._check(self.lib.gpmpc_predict_cov(self._h, Xa.data_ptr(), Ma, _ptr(Xb), Mb, D, E,
                                               _hp(nz) if nz is not None else None, out.data_ptr(), self._stream()))
        self._keep_predict_cov = (Xa, Xb)    # alive until the asynchronous call has read them
        return out

    def _moments(self, name, mu, var, S, V):
        """`moments` and `moments_linear`: the arguments and the dict are the same, `name` picks the library's entry."""
        mu = self._rows(mu, "input means", "P")
        P, E = mu.shape
        D = self.D
        vr = self._dev(var, (P, E, E)) if var is not None else None
        out = {"M": torch.empty((P, D), dtype=torch.float64, device=self.device)}
        if S:
            out["S"] = torch.empty((P, D, D), dtype=torch.float64, device=self.device)
        if V:
            out["V"] = torch.empty((P, E, D), dtype=torch.float64, device=self.device)
        self._check(getattr(self.lib, "gpmpc_" + name)(self._h, mu.data_ptr(), _ptr(vr), P, D, E, out["M"].data_ptr(),
                                                       _ptr(out.get("S")), _ptr(out.get("V")), self._stream()))
        setattr(self, "_keep_" + name, (mu, vr))             # alive until the asynchronous call has read them
        return out

    def _moments_backward(self, name, mu, var, M_bar, S_bar, V_bar, mu_bar, var_bar):
        """`moments_backward` and `moments_linear_backward`: as `_moments`."""
        mu = self._rows(mu, "input means", "P")
        P, E = mu.shape
        D = self.D
        vr = self._dev(var, (P, E, E)) if var is not None else None
        Mb = self._dev(M_bar, (P, D)) if M_bar is not None else None
        Sb = self._dev(S_bar, (P, D, D)) if S_bar is not None else None
        Vb = self._dev(V_bar, (P, E, D)) if V_bar is not None else None
        out = {}
        if mu_bar:
            out["mu_bar"] = torch.empty((P, E), dtype=torch.float64, device=self.device)
        if var_bar:
            out["var_bar"] = torch.empty((P, E, E), dtype=torch.float64, device=self.device)
        self._check(getattr(self.lib, "gpmpc_" + name)(self._h, mu.data_ptr(), _ptr(vr), P, D, E, _ptr(Mb), _ptr(Sb), _ptr(Vb),
                                                       _ptr(out.get("mu_bar")), _ptr(out.get("var_bar")), self._stream()))
        setattr(self, "_keep_" + name, (mu, vr, Mb, Sb, Vb))   # alive until the asynchronous call has read them
        return out

    def moments(self, mu, var=None, S=True, V=True):
        """Moment-matched one-step prediction (predict_next_state_change, gp_model.py:112-180) at P Gaussian inputs from the
        cached model: mu (P, E), var (P, E, E) or None (zero) -> dict(M (P, D), S (P, D, D), V (P, E, D)) of device tensors
        (S / V only when requested).  Asynchronous on the current stream."""
        return self._moments("moments", mu, var, S, V)

    def moments_linear(self, mu, var=None, S=True, V=True):
        """First-order (linearised) one-step prediction at P Gaussian inputs from the cached model (gpmpc_moments_linear): the
        posterior at the input mean, the input covariance pushed through the Jacobian of the posterior mean.  mu (P, E),
        var (P, E, E) or None (zero) -> dict(M (P, D), S (P, D, D) = V^T var V + diag(posterior variance), V (P, E, D) =
        dM/dmu) of device tensors (S / V only when requested).  Without S no matrix product runs: M and the whole mean
        Jacobian in one GEMV-class pass.  Asynchronous on the current stream."""
        return self._moments("moments_linear", mu, var, S, V)

    def moments_backward(self, mu, var=None, M_bar=None, S_bar=None, V_bar=None, mu_bar=True, var_bar=True):
        """Reverse-mode product of `moments` (autograd through predict_next_state_change, gp_model.py:112-180): mu (P, E),
        var (P, E, E) or None (zero), upstream gradients M_bar (P, D), S_bar (P, D, D), V_bar (P, E, D), each None for zero ->
        dict(mu_bar (P, E), var_bar (P, E, E)) of device tensors (each only when requested).  var_bar is the symmetric part of
        the covariance gradient.  Without S_bar the pairwise pass is skipped.  Asynchronous on the current stream."""
        return self._moments_backward("moments_backward", mu, var, M_bar, S_bar, V_bar, mu_bar, var_bar)

    def moments_linear_backward(self, mu, var=None, M_bar=None, S_bar=None, V_bar=None, mu_bar=True, var_bar=True):
        """Reverse-mode product of `moments_linear` (gpmpc_moments_linear_backward): mu (P, E), var (P, E, E) or None (zero),
        upstream gradients M_bar (P, D), S_bar (P, D, D), V_bar (P, E, D), each None for zero -> dict(mu_bar (P, E),
        var_bar (P, E, E)) of device tensors (each only when requested).  var_bar is the symmetric part of the covariance
        gradient, exactly symmetric.  Without S_bar no matrix product runs.  Asynchronous on the current stream."""
        return self._moments_backward("moments_linear_backward", mu, var, M_bar, S_bar, V_bar, mu_bar, var_bar)

    # -- a6 ----------------------------------------------------------------------------
    def set_cost(self, target, W, W_T, kappa, clip_to_zero=False, state_min=None, state_max=None):
        W_T = _host(W_T)
        D = W_T.shape[0]
        W = _host(W)
        A = W.shape[0] - D
        target = _host(target, (D + A,))
        smin = _host(state_min, (D,)) if state_min is not None else None
        smax = _host(state_max, (D,)) if state_max is not None else None
        self._cost_token = None        # whoever caches "my settings are loaded" (GpStateTransitionModel.set_cost) must re-key
        self._check(self.lib.gpmpc_set_cost(self._h, _hp(target), _hp(W), _hp(W_T), float(kappa), int(bool(clip_to_zero)),
                                            _hp(smin) if smin is not None else None,
                                            _hp(smax) if smax is not None else None, D, A))
        self._cost = (D, A)

    # -- a3-a5 -------------------------------------------------------------------------
    def _trajectory_out(self, out, B, H, D, A, trajectories, stage_costs):
        """The dict a forward rollout fills: allocated as asked for, or the caller's `out` once its shapes are checked."""
        if out is None:
            out = {}
            # the objective needs gpmpc_set_cost FOR THIS (D, A); a trajectory-only call passes no cost pointer at all
            if stage_costs or self._cost == (D, A):
                out["J"] = torch.empty(B, dtype=torch.float64, device=self.device)
            if trajectories:
                out["mu"] = torch.empty((B, H + 1, D), dtype=torch.float64, device=self.device)
                out["Sig"] = torch.empty((B, H + 1, D, D), dtype=torch.float64, device=self.device)
            if stage_costs:
                out["cost_mu"] = torch.empty((B, H + 1), dtype=torch.float64, device=self.device)
                out["cost_var"] = torch.empty((B, H + 1), dtype=torch.float64, device=self.device)
        elif ("J" in out and out["J"].shape != (B,)) or ("mu" in out and out["mu"].shape != (B, H + 1, D)):
            raise ValueError("`out` does not match the batch shape")
        return out

    def _gains(self, gains, B, H, A, D):
        """Feedback gains as the closed-loop entries take them: (device tensor (H, A, D) or (B, H, A, D), per_candidate), or
        (None, False)."""
        if gains is None:
            return None, False
        gains = torch.as_tensor(gains, dtype=torch.float64)
        per_candidate, every_step = feedback_gains_layout(gains.shape, B, H, A, D)
        if every_step:
            gains = gains.expand(H, A, D)
        return self._dev(gains), per_candidate

    def _rollout(self, name, actions, mu0, S0, include_time, time0, trajectories, stage_costs, out, closed_loop=False, gains=None):
        """`rollout`, `rollout_linear`, `rollout_linear_feedback` and `rollout_feedback`: `name` picks the library's entry; the
        closed-loop ones take (gains, per_candidate) behind the actions."""
        actions = self._dev(actions)
        B, H, A = actions.shape
        D = self.D
        mu0 = _host(mu0, (D,))
        S0 = _host(S0, (D, D))
        gain_args = ()
        if closed_loop:
            gains, per_candidate = self._gains(gains, B, H, A, D)
            gain_args = (_ptr(gains), int(per_candidate))
        out = self._trajectory_out(out, B, H, D, A, trajectories, stage_costs)
        self._check(getattr(self.lib, "gpmpc_" + name)(
            self._h, actions.data_ptr(), *gain_args, _hp(mu0), _hp(S0), B, H, A, int(bool(include_time)), float(time0),
            _ptr(out.get("mu")), _ptr(out.get("Sig")), _ptr(out.get("cost_mu")), _ptr(out.get("cost_var")), _ptr(out.get("J")),
            self._stream()))
        setattr(self, "_keep_" + name, (actions, gains))      # alive until the asynchronous call has read them
        return out

    def rollout(self, actions, mu0, S0, include_time=False, time0=0.0, trajectories=True, stage_costs=True, out=None):
        """actions (B,H,A) -> dict(J (B,), [mu (B,H+1,D), Sig (B,H+1,D,D)], [cost_mu, cost_var (B,H+1)]).
        `out` = the dict of a previous call with the same shapes: its tensors are overwritten (no allocation)."""
        return self._rollout("rollout", actions, mu0, S0, include_time, time0, trajectories, stage_costs, out)

    def rollout_linear(self, actions, mu0, S0, include_time=False, time0=0.0, trajectories=True, stage_costs=True, out=None):
        """`rollout` with the linearised step (gpmpc_rollout_linear) in place of moment matching: the same arguments, the same
        dict.  Asynchronous on the current stream."""
        return self._rollout("rollout_linear", actions, mu0, S0, include_time, time0, trajectories, stage_costs, out)

    def rollout_linear_feedback(self, actions, gains, mu0, S0, include_time=False, time0=0.0, trajectories=True, stage_costs=True,
                                out=None):
        """`rollout_linear` in closed loop (gpmpc_rollout_linear_feedback): the policy is u = actions_t + K_t (x - mu_t), and
        Sig and the stage costs are those of that policy; mu is `rollout_linear`'s.  `gains` (model space): (A, D) one gain for
        every step and candidate, (H, A, D) one sequence shared by the candidates, or (B, H, A, D); None: `rollout_linear`.
        The same dict.  Asynchronous on the current stream."""
        return self._rollout("rollout_linear_feedback", actions, mu0, S0, include_time, time0, trajectories, stage_costs, out,
                             closed_loop=True, gains=gains)

    def lqr_gains(self, actions, mu0, include_time=False, time0=0.0, reg=0.0, want_cost_to_go=False, want_flags=False):
        """The LQR feedback gains of the linearisation along each candidate's nominal trajectory on the loaded quadratic cost
        (gpmpc_lqr_gains; needs set_cost): dict of device tensors `gains` (B, H, A, D) -- the sign and layout
        `rollout_linear_feedback` takes per candidate --, with want_cost_to_go `P` (B, H + 1, D, D), with want_flags `flags` (B,)
        int32, the number of steps whose factorisation lost a pivot (their gain is zero).  `reg` >= 0 is added to the diagonal
        of Huu.  Certainty-equivalent; the action box is not modelled.  Asynchronous on the current stream."""
        actions = self._dev(actions)
        B, H, A = actions.shape
        D = self.D
        mu0 = _host(mu0, (D,))
        out = {"gains": torch.empty((B, H, A, D), dtype=torch.float64, device=self.device)}
        if want_cost_to_go:
            out["P"] = torch.empty((B, H + 1, D, D), dtype=torch.float64, device=self.device)
        if want_flags:
            out["flags"] = torch.empty(B, dtype=torch.int32, device=self.device)
        self._check(self.lib.gpmpc_lqr_gains(self._h, actions.data_ptr(), _hp(mu0), B, H, A, int(bool(include_time)), float(time0),
                                             float(reg), out["gains"].data_ptr(), _ptr(out.get("P")), _ptr(out.get("flags")),
                                             self._stream()))
        self._keep_lqr_gains = actions           # alive until the asynchronous call has read it
        return out

    def rollout_linear_lqr(self, actions, mu0, S0, include_time=False, time0=0.0, trajectories=True, stage_costs=True, out=None,
                           reg=0.0):
        """`rollout_linear_feedback` under each candidate's own LQR gains: `lqr_gains`, then the closed-loop rollout with those
        (B, H, A, D) gains, which never leave the device.  That call's dict plus "gains"; bit for bit the two calls made
        separately.  Asynchronous on the current stream."""
        actions = self._dev(actions)
        gains = self.lqr_gains(actions, mu0, include_time, time0, reg)["gains"]
        res = self.rollout_linear_feedback(actions, gains, mu0, S0, include_time, time0, trajectories, stage_costs, out)
        res["gains"] = gains
        return res

    def rollout_feedback(self, actions, gains, mu0, S0, include_time=False, time0=0.0, trajectories=True, stage_costs=True,
                         out=None):
        """`rollout` -- moment matching -- in closed loop (gpmpc_rollout_feedback): the policy is u = actions_t + K_t (x - mu_t),
        every step's moments are gpmpc_moments' at the policy's full input covariance, and mu, Sig and the stage costs are those
        of that policy (unlike `rollout_linear_feedback`, the gains move mu too).  `gains` (model space): (A, D), (H, A, D) or
        (B, H, A, D) as there; None: the all-zero gains through the same kernels (`rollout` to rounding, not bit for bit).  The
        same dict.  Asynchronous on the current stream."""
        return self._rollout("rollout_feedback", actions, mu0, S0, include_time, time0, trajectories, stage_costs, out,
                             closed_loop=True, gains=gains)

    def rollout_feedback_lqr(self, actions, mu0, S0, include_time=False, time0=0.0, trajectories=True, stage_costs=True, out=None,
                             reg=0.0):
        """`rollout_feedback` under each candidate's own LQR gains: `lqr_gains`, then the moment-matched closed-loop rollout with
        those (B, H, A, D) gains, which never leave the device.  That call's dict plus "gains"; bit for bit the two calls made
        separately.  Asynchronous on the current stream."""
        actions = self._dev(actions)
        gains = self.lqr_gains(actions, mu0, include_time, time0, reg)["gains"]
        res = self.rollout_feedback(actions, gains, mu0, S0, include_time, time0, trajectories, stage_costs, out)
        res["gains"] = gains
        return res

    def rollout_grad(self, actions, mu0, S0, include_time=False, time0=0.0, trajectories=False):
        """Objective and analytic gradient: dict(J (B,), grad (B,H,A) = dJ/d(actions), [mu, Sig, cost_mu, cost_var]).
        Raises GpmpcError(GPMPC_ERR_LIMIT) for shapes the gradient kernels do not cover (callers then
        difference `rollout`)."""
        actions = self._dev(actions)
        B, H, A = actions.shape
        D = self.D
        mu0 = _host(mu0, (D,))
        S0 = _host(S0, (D, D))
        # one allocation, views into it: a caller that wants everything on the host needs ONE copy (`host_views`)
        shapes = [("J", (B,)), ("grad", (B, H, A))]
        if trajectories:
            shapes += [("mu", (B, H + 1, D)), ("Sig", (B, H + 1, D, D)), ("cost_mu", (B, H + 1)), ("cost_var", (B, H + 1))]
        sizes = [int(np.prod(sh)) for _, sh in shapes]
        pack = torch.empty(sum(sizes), dtype=torch.float64, device=self.device)
        out, off = {"packed": pack, "layout": []}, 0
        for (k, sh), n in zip(shapes, sizes):
            out[k] = pack[off:off + n].view(sh)
            out["layout"].append((k, sh, off, n))
            off += n
        self._check(self.lib.gpmpc_rollout_grad(self._h, actions.data_ptr(), _hp(mu0), _hp(S0), B, H, A,
                                                int(bool(include_time)), float(time0), out["J"].data_ptr(),
                                                out["grad"].data_ptr(),
                                                out["mu"].data_ptr() if trajectories else None,
                                                out["Sig"].data_ptr() if trajectories else None,
                                                out["cost_mu"].data_ptr() if trajectories else None,
                                                out["cost_var"].data_ptr() if trajectories else None, self._stream()))
        return out

    def _seeds(self, B, H, D, mu_bar, Sig_bar, cost_mu_bar, cost_var_bar, J_bar):
        """The upstream gradients of a trajectory dict on the device, in the order the backward entries take them; None stays."""
        return (self._dev(mu_bar, (B, H + 1, D)) if mu_bar is not None else None,
                self._dev(Sig_bar, (B, H + 1, D, D)) if Sig_bar is not None else None,
                self._dev(cost_mu_bar, (B, H + 1)) if cost_mu_bar is not None else None,
                self._dev(cost_var_bar, (B, H + 1)) if cost_var_bar is not None else None,
                self._dev(J_bar, (B,)) if J_bar is not None else None)

    def _rollout_backward(self, name, actions, mu0, S0, include_time, time0, seeds, want_initial, closed_loop=False, gains=None,
                          want_gains=False):
        """`rollout_backward`, `rollout_linear_backward`, `rollout_linear_feedback_backward` and `rollout_feedback_backward`: `name`
        picks the library's entry; the closed-loop ones take (gains, per_candidate) behind the actions and gains_bar behind actions_bar."""
        actions = self._dev(actions)
        B, H, A = actions.shape
        D = self.D
        mu0 = _host(mu0, (D,))
        S0 = _host(S0, (D, D))
        gain_args = ()
        if closed_loop:
            gains, per_candidate = self._gains(gains, B, H, A, D)
            gain_args = (_ptr(gains), int(per_candidate))
        seeds = self._seeds(B, H, D, *seeds)
        out = {"actions_bar": torch.empty((B, H, A), dtype=torch.float64, device=self.device)}
        if want_gains and gains is not None:
            out["gains_bar"] = torch.empty((B, H, A, D), dtype=torch.float64, device=self.device)
        if want_initial:
            out["mu0_bar"] = torch.empty((B, D), dtype=torch.float64, device=self.device)
            out["S0_bar"] = torch.empty((B, D, D), dtype=torch.float64, device=self.device)
        gains_bar_arg = (_ptr(out.get("gains_bar")),) if closed_loop else ()
        self._check(getattr(self.lib, "gpmpc_" + name)(
            self._h, actions.data_ptr(), *gain_args, _hp(mu0), _hp(S0), B, H, A, int(bool(include_time)), float(time0),
            *map(_ptr, seeds), out["actions_bar"].data_ptr(), *gains_bar_arg, _ptr(out.get("mu0_bar")), _ptr(out.get("S0_bar")),
            self._stream()))
        setattr(self, "_keep_" + name, (actions, gains) + seeds)   # alive until the asynchronous call has read them
        return out

    def rollout_backward(self, actions, mu0, S0, include_time=False, time0=0.0, mu_bar=None, Sig_bar=None, cost_mu_bar=None,
                         cost_var_bar=None, J_bar=None, want_initial=True):
        """Reverse-mode product of `rollout` (autograd through predict_trajectory + get_rewards_trajectory, gp_model.py:60-110,
        setpoint_distance_reward_mapper.py:144-149): actions (B,H,A), the shared initial state mu0 (D,), S0 (D,D) and the upstream
        gradients mu_bar (B,H+1,D), Sig_bar (B,H+1,D,D), cost_mu_bar / cost_var_bar (B,H+1), J_bar (B,), each None for zero ->
        dict of device tensors actions_bar (B,H,A) and, with `want_initial`, mu0_bar (B,D) and S0_bar (B,D,D) per candidate
        (S0_bar the symmetric part).  The forward is recomputed inside the call (gpmpc_rollout_backward).  Cost / J seeds need
        set_cost; shapes outside the gradient kernels raise GpmpcError(GPMPC_ERR_LIMIT).  Asynchronous on the current stream."""
        return self._rollout_backward("rollout_backward", actions, mu0, S0, include_time, time0,
                                      (mu_bar, Sig_bar, cost_mu_bar, cost_var_bar, J_bar), want_initial)

    def rollout_linear_backward(self, actions, mu0, S0, include_time=False, time0=0.0, mu_bar=None, Sig_bar=None,
                                cost_mu_bar=None, cost_var_bar=None, J_bar=None, want_initial=True):
        """Reverse-mode product of `rollout_linear` (gpmpc_rollout_linear_backward), with the arguments and the result of
        `rollout_backward`: dict of device tensors actions_bar (B,H,A) and, with `want_initial`, mu0_bar (B,D) and S0_bar (B,D,D)
        per candidate (S0_bar the symmetric part).  The forward is recomputed inside the call.  Cost / J seeds need set_cost.
        Asynchronous on the current stream."""
        return self._rollout_backward("rollout_linear_backward", actions, mu0, S0, include_time, time0,
                                      (mu_bar, Sig_bar, cost_mu_bar, cost_var_bar, J_bar), want_initial)

    def rollout_linear_grad(self, actions, mu0, S0, include_time=False, time0=0.0):
        """Objective of the linearised rollout and its analytic gradient: dict(J (B,), grad (B,H,A) = dJ/d(actions)) of device
        tensors, from `rollout_linear` followed by `rollout_linear_backward` with J_bar = 1."""
        actions = self._dev(actions)
        B = actions.shape[0]
        J = torch.empty(B, dtype=torch.float64, device=self.device)
        self.rollout_linear(actions, mu0, S0, include_time, time0, trajectories=False, stage_costs=False, out={"J": J})
        ones = torch.ones(B, dtype=torch.float64, device=self.device)
        back = self.rollout_linear_backward(actions, mu0, S0, include_time, time0, J_bar=ones, want_initial=False)
        return {"J": J, "grad": back["actions_bar"]}

    def rollout_linear_feedback_backward(self, actions, gains, mu0, S0, include_time=False, time0=0.0, mu_bar=None, Sig_bar=None,
                                         cost_mu_bar=None, cost_var_bar=None, J_bar=None, want_initial=True, want_gains=True):
        """Reverse-mode product of `rollout_linear_feedback` (gpmpc_rollout_linear_feedback_backward): its arguments and the
        cotangents of `rollout_linear_backward` -> dict of device tensors actions_bar (B,H,A), with `want_gains` gains_bar
        (B,H,A,D), and with `want_initial` mu0_bar (B,D) and S0_bar (B,D,D) per candidate (S0_bar the symmetric part).
        `gains`: (A, D), (H, A, D) or (B, H, A, D) as in `rollout_linear_feedback`.  gains_bar is per candidate and per step
        whatever the layout of `gains`: reduce it as the gains were broadcast -- `gains_bar.sum(0)` for a shared (H, A, D)
        sequence, `gains_bar.sum((0, 1))` for one (A, D) gain.  gains None: `rollout_linear_backward` (no gains_bar).  The
        forward is recomputed inside the call.  Cost / J seeds need set_cost.  Asynchronous on the current stream."""
        return self._rollout_backward("rollout_linear_feedback_backward", actions, mu0, S0, include_time, time0,
                                      (mu_bar, Sig_bar, cost_mu_bar, cost_var_bar, J_bar), want_initial, closed_loop=True, gains=gains,
                                      want_gains=want_gains)

    def rollout_linear_feedback_grad(self, actions, gains, mu0, S0, include_time=False, time0=0.0):
        """Objective of the closed-loop linearised rollout and its analytic gradients: dict(J (B,), grad (B,H,A) = dJ/d(actions),
        gains_grad (B,H,A,D) = dJ/d(gains), per candidate: see `rollout_linear_feedback_backward`) of device tensors, from
        `rollout_linear_feedback` followed by `rollout_linear_feedback_backward` with J_bar = 1."""
        actions = self._dev(actions)
        B = actions.shape[0]
        J = torch.empty(B, dtype=torch.float64, device=self.device)
        self.rollout_linear_feedback(actions, gains, mu0, S0, include_time, time0, trajectories=False, stage_costs=False,
                                     out={"J": J})
        ones = torch.ones(B, dtype=torch.float64, device=self.device)
        back = self.rollout_linear_feedback_backward(actions, gains, mu0, S0, include_time, time0, J_bar=ones, want_initial=False)
        return {"J": J, "grad": back["actions_bar"], "gains_grad": back.get("gains_bar")}

    def rollout_feedback_backward(self, actions, gains, mu0, S0, include_time=False, time0=0.0, mu_bar=None, Sig_bar=None,
                                  cost_mu_bar=None, cost_var_bar=None, J_bar=None, want_initial=True, want_gains=True):
        """Reverse-mode product of `rollout_feedback` (gpmpc_rollout_feedback_backward): the arguments and the dict of
        `rollout_linear_feedback_backward` -- actions_bar (B,H,A), with `want_gains` gains_bar (B,H,A,D), with `want_initial`
        mu0_bar (B,D) and S0_bar (B,D,D) per candidate (S0_bar the symmetric part).  Under moment matching the gains move the mean
        as well, so gains_bar carries that path too.  gains_bar is per candidate and per step whatever the layout of `gains`:
        reduce it as the gains were broadcast.  gains None: the zero-gain policy through the same kernels (no gains_bar).  The
        forward is recomputed inside the call.  Cost / J seeds need set_cost.  Asynchronous on the current stream."""
        return self._rollout_backward("rollout_feedback_backward", actions, mu0, S0, include_time, time0,
                                      (mu_bar, Sig_bar, cost_mu_bar, cost_var_bar, J_bar), want_initial, closed_loop=True, gains=gains,
                                      want_gains=want_gains)

    def rollout_feedback_grad(self, actions, gains, mu0, S0, include_time=False, time0=0.0):
        """Objective of the closed-loop moment-matched rollout and its analytic gradients: dict(J (B,), grad (B,H,A) =
        dJ/d(actions), gains_grad (B,H,A,D) = dJ/d(gains), per candidate: see `rollout_feedback_backward`) of device tensors,
        from `rollout_feedback` followed by `rollout_feedback_backward` with J_bar = 1."""
        actions = self._dev(actions)
        B = actions.shape[0]
        J = torch.empty(B, dtype=torch.float64, device=self.device)
        self.rollout_feedback(actions, gains, mu0, S0, include_time, time0, trajectories=False, stage_costs=False, out={"J": J})
        ones = torch.ones(B, dtype=torch.float64, device=self.device)
        back = self.rollout_feedback_backward(actions, gains, mu0, S0, include_time, time0, J_bar=ones, want_initial=False)
        return {"J": J, "grad": back["actions_bar"], "gains_grad": back.get("gains_bar")}

    def objective_grad_host(self, actions, mu0, S0, include_time=False, time0=0.0):
        """ONE action sequence (H, A) on the host -> objective, gradient, trajectory and stage costs on the host
        (gpmpc_objective_grad_host: the sequence travels as a kernel argument, the results through a pinned host buffer,
        one synchronisation) -- what a host-side optimiser that evaluates one sequence per call needs (the reference's
        scipy L-BFGS-B loop, gp_mpc_controller.py:133-141).  Returns numpy arrays (copies: the buffer is reused)."""
        actions = np.asarray(actions, dtype=np.float64)
        H, A = actions.shape
        plan = self._ogh_plans.get((H, A))
        if plan is None:
            plan = self._ogh_plans[(H, A)] = _HostEvaluationPlan(H, A, self.D)
        # (staging arrays with known addresses: taking an array's address through ctypes costs more than copying 25 numbers)
        np.copyto(plan.actions, actions)
        np.copyto(plan.mu0, np.asarray(mu0, dtype=np.float64).reshape(plan.mu0.shape))
        np.copyto(plan.S0, np.asarray(S0, dtype=np.float64).reshape(plan.S0.shape))
        self._check(self.lib.gpmpc_objective_grad_host(self._h, plan.p_actions, plan.p_mu0, plan.p_S0, H, A, int(bool(include_time)),
                                                       float(time0), plan.res_ref, self._stream()))
        return plan.result()

    @staticmethod
    def host_views(out):
        """All tensors of a `rollout_grad` result on the host with a single device-to-host copy."""
        host = out["packed"].cpu()
        return {k: host[off:off + n].view(sh) for k, sh, off, n in out["layout"]}

    def rollout_timed(self, actions, mu0, S0, reps, include_time=False, time0=0.0):
        """Average kernel milliseconds per launch, measured with HIP events on the launch stream."""
        actions = self._dev(actions)
        B, H, A = actions.shape
        mu0 = _host(mu0, (self.D,))
        S0 = _host(S0, (self.D, self.D))
        J = torch.empty(B, dtype=torch.float64, device=self.device)
        ms = C.c_float(0.0)
        self._check(self.lib.gpmpc_rollout_timed(self._h, actions.data_ptr(), _hp(mu0), _hp(S0), B, H, A,
                                                 int(bool(include_time)), float(time0), J.data_ptr(), int(reps),
                                                 C.byref(ms), self._stream()))
        return float(ms.value), J

    def cem_search(self, mu0, S0, B, H, A, iterations, n_elite, seed=0, include_time=False, time0=0.0, first_candidate=None,
                   max_change=None, action_prev=None, noise=None):
        """Cross-entropy search over [0,1]^(H*A) with the whole loop on the device (gpmpc_cem_search): returns
        (best optimiser vector (H*A,) numpy, best J).  `max_change` / `action_prev` given => DerivativeActionMapper,
        else the identity mapper.  `noise` (iterations, B, H*A) device / host tensor replaces the Philox draws (tests).
        ONE host synchronisation, at the end."""
        D = self.D
        mu0 = _host(mu0, (D,))
        S0 = _host(S0, (D, D))
        n = H * A
        best = torch.empty(n + 1, dtype=torch.float64, device=self.device)
        first = _host(first_candidate, (n,)) if first_candidate is not None else None
        mapper = 0 if max_change is None else 1
        mc = _host(max_change, (A,)) if mapper else None
        ap = _host(action_prev, (A,)) if mapper else None
        nz = None if noise is None else self._dev(noise, (iterations, B, n))
        self._check(self.lib.gpmpc_cem_search(self._h, _hp(mu0), _hp(S0), B, H, A, int(bool(include_time)), float(time0),
                                              int(iterations), int(n_elite), int(seed) & (2 ** 64 - 1),
                                              _hp(first) if first is not None else None, mapper,
                                              _hp(mc) if mapper else None, _hp(ap) if mapper else None,
                                              nz.data_ptr() if nz is not None else None, best.data_ptr(), self._stream()))
        host = best.cpu().numpy()                               # the one synchronisation
        return host[:n].copy(), float(host[n])

    def cem_local(self, mu0, S0, B_total, first, B_local, H, A, iteration, n_elite, state, seed=0, include_time=False,
                  time0=0.0, first_candidate=None, max_change=None, action_prev=None, noise=None, out=None):
        """One iteration of the cross-entropy search for the slice [first, first + B_local) of B_total candidates
        (gpmpc_cem_local): returns the slice's elite records (n_elite, 2 + H*A) on the device.  `state` = the device tensor
        [mean | std | best | best J] (3 H A + 1) `cem_merge` maintains.  No synchronisation."""
        D = self.D
        mu0 = _host(mu0, (D,))
        S0 = _host(S0, (D, D))
        n = H * A
        if out is None:
            out = torch.empty((n_elite, n + 2), dtype=torch.float64, device=self.device)
        first_c = _host(first_candidate, (n,)) if first_candidate is not None else None
        mapper = 0 if max_change is None else 1
        mc = _host(max_change, (A,)) if mapper else None
        ap = _host(action_prev, (A,)) if mapper else None
        nz = None if noise is None else self._dev(noise)
        if nz is not None and (nz.dim() != 3 or nz.shape[1] != B_total or nz.shape[2] != n):
            raise ValueError("noise must be (iterations, B_total, H*A)")
        self._check(self.lib.gpmpc_cem_local(self._h, _hp(mu0), _hp(S0), int(B_total), int(first), int(B_local), H, A,
                                             int(bool(include_time)), float(time0), int(iteration), int(n_elite),
                                             int(seed) & (2 ** 64 - 1), _hp(first_c) if first_c is not None else None, mapper,
                                             _hp(mc) if mapper else None, _hp(ap) if mapper else None,
                                             nz.data_ptr() if nz is not None else None, state.data_ptr(), out.data_ptr(),
                                             self._stream()))
        self._keep_cem = (nz, state)
        return out

    def cem_merge(self, elites, n_elite, n, iteration, state):
        """Refit on the union of the slices' elite records (lists * n_elite, 2 + n) (gpmpc_cem_merge); updates `state`."""
        lists = elites.numel() // (n_elite * (n + 2))
        self._check(self.lib.gpmpc_cem_merge(self._h, elites.data_ptr(), lists, int(n_elite), int(n), int(iteration),
                                             state.data_ptr(), self._stream()))

    # -- device-resident L-BFGS (gpmpc_lbfgs_*) -----------------------------------------------------
    def lbfgs_state(self, B, n, history):
        """The caller-owned state of the device L-BFGS for B restarts of n coordinates and `history` pairs: dict of named views
        (x, g, d, xt, actions (B, n); J, alpha, status, pushes (B); S, Y (B, history, n); sy, yy (B, history) -- `pairs` is the
        tuple (S, Y, sy, yy)) into ONE device buffer (`buffer`), laid out as include/gpmpc.h documents."""
        B, n, m = int(B), int(n), int(history)
        size = int(self.lib.gpmpc_lbfgs_state_size(B, n, m))
        if size < 0:
            raise ValueError("lbfgs_state: need 1 <= B <= 4096, 1 <= n <= 4096, 1 <= history <= 32")
        buf = torch.zeros(size, dtype=torch.float64, device=self.device)
        st, off = {"buffer": buf, "B": B, "n": n, "history": m}, 0
        for k, sh in (("x", (B, n)), ("g", (B, n)), ("d", (B, n)), ("xt", (B, n)), ("actions", (B, n)), ("J", (B,)),
                      ("alpha", (B,)), ("status", (B,)), ("pushes", (B,)), ("S", (B, m, n)), ("Y", (B, m, n)), ("sy", (B, m)),
                      ("yy", (B, m))):
            cnt = int(np.prod(sh))
            st[k] = buf[off:off + cnt].view(sh)
            off += cnt
        assert off == size
        st["pairs"] = (st["S"], st["Y"], st["sy"], st["yy"])
        return st

    @staticmethod
    def _lbfgs_mapper(A, max_change, action_prev):
        """(mapper, max_change, action_prev) as the C entries take them: either array given => the derivative mapper (a missing
        partner is the library's GPMPC_ERR_ARG)."""
        if max_change is None and action_prev is None:
            return 0, None, None
        return 1, (None if max_change is None else _host(max_change, (A,))), (None if action_prev is None else _host(action_prev, (A,)))

    def lbfgs_init(self, state, x0, H, A, max_change=None, action_prev=None):
        """gpmpc_lbfgs_init: trial point = clip(x0 (B, H*A)), its model actions, everything else reset.  No synchronisation."""
        B, n, m = state["B"], state["n"], state["history"]
        if n != H * A:
            raise ValueError("the state was made for another number of coordinates")
        x0 = self._dev(x0, (B, n))
        mapper, mc, ap = self._lbfgs_mapper(A, max_change, action_prev)
        self._check(self.lib.gpmpc_lbfgs_init(self._h, x0.data_ptr(), B, H, A, m, mapper, None if mc is None else _hp(mc),
                                              None if ap is None else _hp(ap), state["buffer"].data_ptr(), self._stream()))
        self._keep_lbfgs = (x0, state["buffer"])

    def lbfgs_step(self, state, J, grad_model, H, A, iteration, c1=1e-4, pgtol=1e-5, max_change=None, action_prev=None):
        """gpmpc_lbfgs_step: iteration `iteration` from J (B) and dJ/d(model actions) (B, H, A) at the state's `actions`.  No
        synchronisation."""
        B, n, m = state["B"], state["n"], state["history"]
        if n != H * A:
            raise ValueError("the state was made for another number of coordinates")
        J = self._dev(J, (B,))
        G = self._dev(grad_model, (B, H, A))
        mapper, mc, ap = self._lbfgs_mapper(A, max_change, action_prev)
        self._check(self.lib.gpmpc_lbfgs_step(self._h, J.data_ptr(), G.data_ptr(), B, H, A, int(iteration), m, float(c1),
                                              float(pgtol), mapper, None if mc is None else _hp(mc),
                                              None if ap is None else _hp(ap), state["buffer"].data_ptr(), self._stream()))
        self._keep_lbfgs = (J, G, state["buffer"])

    def lbfgs_search(self, state, mu0, S0, H, A, iterations, x0=None, first_iteration=0, c1=1e-4, pgtol=1e-5, propagation="moment",
                     include_time=False, time0=0.0, max_change=None, action_prev=None, best_out=None):
        """gpmpc_lbfgs_search: the whole loop on the device -- with first_iteration == 0 the init from x0 (B, H*A), then
        `iterations` x [objective + gradient of the state's actions, step]; `propagation` "moment" or "linearized".  Returns the
        device record [best J | restart | best x (H*A)] (`best_out`, or a new tensor).  No synchronisation."""
        B, n, m = state["B"], state["n"], state["history"]
        if n != H * A:
            raise ValueError("the state was made for another number of coordinates")
        if propagation not in ("moment", "linearized"):
            raise ValueError("propagation must be 'moment' or 'linearized'")
        D = self.D
        mu0 = _host(mu0, (D,))
        S0 = _host(S0, (D, D))
        x0 = self._dev(x0, (B, n)) if x0 is not None else None
        if best_out is None:
            best_out = torch.empty(2 + n, dtype=torch.float64, device=self.device)
        mapper, mc, ap = self._lbfgs_mapper(A, max_change, action_prev)
        self._check(self.lib.gpmpc_lbfgs_search(self._h, _hp(mu0), _hp(S0), B, H, A, int(bool(include_time)), float(time0),
                                                0 if propagation == "moment" else 1, int(first_iteration), int(iterations), m,
                                                float(c1), float(pgtol), mapper, None if mc is None else _hp(mc),
                                                None if ap is None else _hp(ap), None if x0 is None else x0.data_ptr(),
                                                state["buffer"].data_ptr(), best_out.data_ptr(), self._stream()))
        self._keep_lbfgs = (x0, state["buffer"], best_out)
        return best_out

    def lbfgs_search_host(self, x0, mu0, S0, H, A, iterations, history=10, c1=1e-4, pgtol=1e-5, propagation="moment",
                          include_time=False, time0=0.0, max_change=None, action_prev=None):
        """The device L-BFGS from the starts x0 (B, H*A) -> (best x (H*A,), best J, per-restart J (B,), per-restart status (B,)) as
        numpy, with ONE host synchronisation (a single copy of the winner record and the per-restart values)."""
        x0 = np.asarray(x0, dtype=np.float64)
        B, n = x0.shape
        st = self.lbfgs_state(B, n, history)
        out = torch.empty(2 + n + 2 * B, dtype=torch.float64, device=self.device)
        self.lbfgs_search(st, mu0, S0, H, A, iterations, x0=x0, c1=c1, pgtol=pgtol, propagation=propagation,
                          include_time=include_time, time0=time0, max_change=max_change, action_prev=action_prev,
                          best_out=out[:2 + n])
        out[2 + n:2 + n + B].copy_(st["J"])
        out[2 + n + B:].copy_(st["status"])
        host = out.cpu().numpy()                                # the one synchronisation
        return host[2:2 + n].copy(), float(host[0]), host[2 + n:2 + n + B].copy(), host[2 + n + B:].astype(np.int64)

    # -- batched training loss and the multi-restart search on it (gpmpc_mll_batch, gpmpc_train_search) ---------------------
    def _training_data(self, X, Y):
        X = self._rows(X, "inputs", "N")
        N, E = X.shape
        Y = self._dev(Y)
        if Y.dim() != 2 or Y.shape[0] != N:
            raise ValueError(f"expected targets of shape ({N}, D), got {tuple(Y.shape)}")
        return X, Y, N, int(Y.shape[1]), E

    def _box(self, lo, hi, D, n, log_scale, required):
        """The box (lo, hi) of shape (D, n) on the device, checked: both or neither, lo <= hi, lo > 0 under the log map."""
        if lo is None and hi is None:
            if required:
                raise ValueError("train_search: the box (lo, hi) is required")
            return None, None
        if lo is None or hi is None:
            raise ValueError("lo and hi must both be given or both be None")
        lo_h, hi_h = _host(lo, (D, n)), _host(hi, (D, n))
        if not np.all(lo_h <= hi_h):
            raise ValueError("the box needs lo <= hi in every coordinate")
        if log_scale and not np.all(lo_h > 0.0):
            raise ValueError("the log map needs lo > 0 in every coordinate")
        return self._dev(lo_h), self._dev(hi_h)

    def mll_batch(self, X, Y, params, lo=None, hi=None, log_scale=True, out=None):
        """gpmpc_mll_batch: training loss and gradient of R hyper-parameter sets per GP, params (R, D, E + 2) rows
        [lengthscale (E) | outputscale | noise] -- or, with the box lo / hi (D, E + 2), x in [0, 1] mapped linearly or (log_scale)
        geometrically into it, the gradient then wrt x.  Returns dict of device tensors loss (R, D), grad (R, D, E + 2),
        theta (R, D, E + 2), info (R, D) int32 (0, or the order of the leading minor that is not positive definite: loss +inf,
        gradient 0).  No synchronisation; the cached model is neither read nor written."""
        X, Y, N, D, E = self._training_data(X, Y)
        n = E + 2
        params = self._dev(params)
        if params.dim() != 3 or tuple(params.shape[1:]) != (D, n):
            raise ValueError(f"expected parameters of shape (R, {D}, {n}), got {tuple(params.shape)}")
        R = int(params.shape[0])
        lo_d, hi_d = self._box(lo, hi, D, n, log_scale, False)
        if out is None:
            out = {"loss": torch.empty((R, D), dtype=torch.float64, device=self.device),
                   "grad": torch.empty((R, D, n), dtype=torch.float64, device=self.device),
                   "theta": torch.empty((R, D, n), dtype=torch.float64, device=self.device),
                   "info": torch.empty((R, D), dtype=torch.int32, device=self.device)}
        self._check(self.lib.gpmpc_mll_batch(self._h, X.data_ptr(), Y.data_ptr(), N, D, E, params.data_ptr(), R, _ptr(lo_d),
                                             _ptr(hi_d), int(bool(log_scale)), out["loss"].data_ptr(), out["grad"].data_ptr(),
                                             _ptr(out.get("theta")), _ptr(out.get("info")), self._stream()))
        self._keep_train = (X, Y, params, lo_d, hi_d, out)
        return out

    def train_search(self, state, X, Y, lo, hi, iterations, x0=None, first_iteration=0, c1=1e-4, pgtol=1e-5, log_scale=True,
                     best_out=None):
        """gpmpc_train_search: the whole multi-restart hyper-parameter search on the device -- with first_iteration == 0 the init
        from x0 (R, D, E + 2) in [0, 1], then `iterations` x [mll_batch of the state's actions with the box, lbfgs step].  `state`
        is lbfgs_state(R * D, E + 2, history).  Returns the device record (D, 3 + E + 2) = [loss | restart | status | theta] per GP
        (`best_out`, or a new tensor).  No synchronisation."""
        X, Y, N, D, E = self._training_data(X, Y)
        n, m = E + 2, state["history"]
        if state["n"] != n or state["B"] % D:
            raise ValueError("the state was made for another number of coordinates or of GPs")
        R = state["B"] // D
        lo_d, hi_d = self._box(lo, hi, D, n, log_scale, True)
        x0 = self._dev(x0, (R, D, n)) if x0 is not None else None
        if best_out is None:
            best_out = torch.empty((D, 3 + n), dtype=torch.float64, device=self.device)
        self._check(self.lib.gpmpc_train_search(self._h, X.data_ptr(), Y.data_ptr(), N, D, E, R, lo_d.data_ptr(), hi_d.data_ptr(),
                                                int(bool(log_scale)), int(first_iteration), int(iterations), m, float(c1),
                                                float(pgtol), _ptr(x0), state["buffer"].data_ptr(), best_out.data_ptr(),
                                                self._stream()))
        self._keep_train = (X, Y, lo_d, hi_d, x0, state["buffer"], best_out)
        return best_out

    def train_search_host(self, X, Y, x0, lo, hi, iterations, history=10, c1=1e-4, pgtol=1e-5, log_scale=True):
        """The device search from the starts x0 (R, D, E + 2) -> dict of numpy arrays theta (D, E + 2), loss (D,), restart (D,)
        (-1: every restart of that GP started non-finite), J (R, D), status (R, D), with ONE host synchronisation (a single copy
        of the winner records and the per-restart values)."""
        x0 = np.asarray(x0, dtype=np.float64)
        if x0.ndim != 3:
            raise ValueError(f"expected starts of shape (R, D, E + 2), got {x0.shape}")
        R, D, n = x0.shape
        P = R * D
        st = self.lbfgs_state(P, n, history)
        out = torch.empty(D * (3 + n) + 2 * P, dtype=torch.float64, device=self.device)
        nb = D * (3 + n)
        self.train_search(st, X, Y, lo, hi, iterations, x0=x0, c1=c1, pgtol=pgtol, log_scale=log_scale,
                          best_out=out[:nb].view(D, 3 + n))
        out[nb:nb + P].copy_(st["J"])
        out[nb + P:].copy_(st["status"])
        host = out.cpu().numpy()                                # the one synchronisation
        best = host[:nb].reshape(D, 3 + n)
        return {"theta": best[:, 3:].copy(), "loss": best[:, 0].copy(), "restart": best[:, 1].astype(np.int64),
                "J": host[nb:nb + P].reshape(R, D).copy(), "status": host[nb + P:].reshape(R, D).astype(np.int64)}

    # -- device-resident iLQR (gpmpc_ilqr_*) --------------------------------------------------------
    def ilqr_backward(self, actions, mu0, reg, include_time=False, time0=0.0):
        """gpmpc_ilqr_backward at `actions` (B, H, A) with the regularisation `reg` (a scalar or (B,)): dict of device tensors
        `gains` (B, H, A, D), `ff` (B, H, A), `mu` (B, H + 1, D), `info` (B, 5) = [cost | dV | step | flags | 0] and its columns
        `cost`, `dV`, `step`, `flags` as views.  Certainty-equivalent cost (needs set_cost).  Asynchronous on the current stream."""
        actions = self._dev(actions)
        B, H, A = actions.shape
        D = self.D
        mu0 = _host(mu0, (D,))
        reg = torch.as_tensor(reg, dtype=torch.float64).to(self.device)
        reg = reg.expand(B).contiguous() if reg.dim() == 0 else self._dev(reg, (B,))
        new = lambda *sh: torch.empty(sh, dtype=torch.float64, device=self.device)       # noqa: E731
        out = {"gains": new(B, H, A, D), "ff": new(B, H, A), "mu": new(B, H + 1, D), "info": new(B, 5)}
        self._check(self.lib.gpmpc_ilqr_backward(self._h, actions.data_ptr(), _hp(mu0), B, H, A, int(bool(include_time)),
                                                 float(time0), reg.data_ptr(), out["gains"].data_ptr(), out["ff"].data_ptr(),
                                                 out["mu"].data_ptr(), out["info"].data_ptr(), self._stream()))
        for i, k in enumerate(("cost", "dV", "step", "flags")):
            out[k] = out["info"][:, i]
        self._keep_ilqr = (actions, reg)
        return out

    def ilqr_forward(self, actions, gains, ff, mu_nom, mu0, alphas, include_time=False, time0=0.0, trajectories=True):
        """gpmpc_ilqr_forward: the closed-loop forward pass on the mean for the step sizes `alphas` (L,): dict of device tensors
        `trial_actions` (B, L, H, A), `trial_cost` (B, L) and, with `trajectories`, `trial_mu` (B, L, H + 1, D).  Asynchronous."""
        actions = self._dev(actions)
        B, H, A = actions.shape
        D = self.D
        gains, ff, mu_nom = self._dev(gains, (B, H, A, D)), self._dev(ff, (B, H, A)), self._dev(mu_nom, (B, H + 1, D))
        mu0 = _host(mu0, (D,))
        alphas = _host(alphas)
        L_ = int(alphas.size)
        new = lambda *sh: torch.empty(sh, dtype=torch.float64, device=self.device)       # noqa: E731
        out = {"trial_actions": new(B, L_, H, A), "trial_cost": new(B, L_)}
        if trajectories:
            out["trial_mu"] = new(B, L_, H + 1, D)
        self._check(self.lib.gpmpc_ilqr_forward(self._h, actions.data_ptr(), gains.data_ptr(), ff.data_ptr(), mu_nom.data_ptr(),
                                                _hp(mu0), B, H, A, int(bool(include_time)), float(time0), _hp(alphas), L_,
                                                out["trial_actions"].data_ptr(), out["trial_cost"].data_ptr(),
                                                _ptr(out.get("trial_mu")), self._stream()))
        self._keep_ilqr = (actions, gains, ff, mu_nom)
        return out

    def ilqr_state(self, B, H, A, L):
        """The caller-owned state of the device iLQR for B candidates and L line-search steps: dict of named views (actions
        (B, H, A); cost, reg, status, accepts, chosen, dV, step, flags, J (B); trial_cost (B, L); gains (B, H, A, D); ff (B, H, A);
        mu (B, H + 1, D); trial_actions (B, L, H, A)) into ONE device buffer (`buffer`), laid out as include/gpmpc.h documents."""
        B, H, A, L_, D = int(B), int(H), int(A), int(L), int(self.D)
        size = int(self.lib.gpmpc_ilqr_state_size(B, H, A, D, L_))
        if size < 0:
            raise ValueError("ilqr_state: need 1 <= B <= 4096, H >= 1, 1 <= A <= 8, 1 <= L <= 16 and a prepared model")
        buf = torch.zeros(size, dtype=torch.float64, device=self.device)
        st, off = {"buffer": buf, "B": B, "H": H, "A": A, "L": L_}, 0
        for k, sh in (("actions", (B, H, A)), ("cost", (B,)), ("reg", (B,)), ("status", (B,)), ("accepts", (B,)), ("chosen", (B,)),
                      ("dV", (B,)), ("step", (B,)), ("flags", (B,)), ("J", (B,)), ("trial_cost", (B, L_)), ("gains", (B, H, A, D)),
                      ("ff", (B, H, A)), ("mu", (B, H + 1, D)), ("trial_actions", (B, L_, H, A))):
            cnt = int(np.prod(sh))
            st[k] = buf[off:off + cnt].view(sh)
            off += cnt
        assert off == size
        return st

    def ilqr_init(self, state, x0, reg0=1e-3):
        """gpmpc_ilqr_init: actions = clip(x0 (B, H, A)), reg = reg0, chosen = -1, everything else 0.  No synchronisation."""
        B, H, A, L_ = state["B"], state["H"], state["A"], state["L"]
        x0 = self._dev(x0).reshape(B, H, A)
        self._check(self.lib.gpmpc_ilqr_init(self._h, x0.data_ptr(), B, H, A, L_, float(reg0), state["buffer"].data_ptr(),
                                             self._stream()))
        self._keep_ilqr = (x0, state["buffer"])

    def ilqr_step(self, state, mu0, reg0=1e-3, reg_factor=10.0, reg_max=1e6, tol=1e-9, include_time=False, time0=0.0):
        """gpmpc_ilqr_step: one iteration (backward, line search over alpha = 2^-l, accept rule) on the state.  No synchronisation."""
        B, H, A, L_ = state["B"], state["H"], state["A"], state["L"]
        mu0 = _host(mu0, (self.D,))
        self._check(self.lib.gpmpc_ilqr_step(self._h, _hp(mu0), B, H, A, int(bool(include_time)), float(time0), L_, float(reg0),
                                             float(reg_factor), float(reg_max), float(tol), state["buffer"].data_ptr(),
                                             self._stream()))

    def ilqr_search(self, state, mu0, S0, iterations, x0, reg0=1e-3, reg_factor=10.0, reg_max=1e6, tol=1e-9, include_time=False,
                    time0=0.0, best_out=None):
        """gpmpc_ilqr_search: init from x0 (B, H, A), `iterations` steps, the LCB objective J of the final sequences
        (gpmpc_rollout_linear) into the state's J.  Returns the device record [best J | candidate | its actions (H*A)] (`best_out`,
        or a new tensor).  No synchronisation."""
        B, H, A, L_ = state["B"], state["H"], state["A"], state["L"]
        D = self.D
        mu0 = _host(mu0, (D,))
        S0 = _host(S0, (D, D))
        x0 = self._dev(x0).reshape(B, H, A)
        if best_out is None:
            best_out = torch.empty(2 + H * A, dtype=torch.float64, device=self.device)
        self._check(self.lib.gpmpc_ilqr_search(self._h, _hp(mu0), _hp(S0), B, H, A, int(bool(include_time)), float(time0),
                                               int(iterations), L_, float(reg0), float(reg_factor), float(reg_max), float(tol),
                                               x0.data_ptr(), state["buffer"].data_ptr(), best_out.data_ptr(), self._stream()))
        self._keep_ilqr = (x0, state["buffer"], best_out)
        return best_out

    def ilqr_search_host(self, x0, mu0, S0, H, A, iterations, line_search_steps=8, reg0=1e-3, reg_factor=10.0, reg_max=1e6,
                         tol=1e-9, include_time=False, time0=0.0):
        """The device iLQR from the starts x0 (B, H*A) -> (best actions (H*A,), best J, per-candidate J (B,), per-candidate status
        (B,)) as numpy, with ONE host synchronisation (a single copy of the winner record and the per-candidate values)."""
        x0 = np.asarray(x0, dtype=np.float64)
        B, n = x0.shape[0], H * A
        st = self.ilqr_state(B, H, A, line_search_steps)
        out = torch.empty(2 + n + 2 * B, dtype=torch.float64, device=self.device)
        self.ilqr_search(st, mu0, S0, iterations, x0.reshape(B, H, A), reg0=reg0, reg_factor=reg_factor, reg_max=reg_max, tol=tol,
                         include_time=include_time, time0=time0, best_out=out[:2 + n])
        out[2 + n:2 + n + B].copy_(st["J"])
        out[2 + n + B:].copy_(st["status"])
        host = out.cpu().numpy()                                # the one synchronisation
        return host[2:2 + n].copy(), float(host[0]), host[2 + n:2 + n + B].copy(), host[2 + n + B:].astype(np.int64)

    # -- a8 ----------------------------------------------------------------------------
    # sharding.select_best_async looks for this attribute: argmin_async can deliver the record to pinned host memory itself
    argmin_exports_host = True

    def argmin_async(self, J, first_global_index=0, actions=None, out=None, host_out=None):
        """Device-side keep-the-best, no host synchronisation: returns the device record
        [best J, global index as double (-1: none), winning action sequence (H*A values, if `actions` given)].
        `host_out`: a pinned float64 host tensor of the record's length; the kernel stores the record there as well
        (gpmpc_argmin_export) -- complete once the stream has passed the launch, no copy behind it."""
        J = self._dev(J)
        ha = 0 if actions is None else int(actions[0].numel())
        if out is None:
            out = torch.empty(2 + ha, dtype=torch.float64, device=self.device)
        if host_out is None:
            self._check(self.lib.gpmpc_argmin_async(self._h, J.data_ptr(), J.numel(), int(first_global_index),
                                                    None if actions is None else actions.data_ptr(), ha,
                                                    out.data_ptr(), self._stream()))
            return out
        if (host_out.device.type != "cpu" or host_out.dtype != torch.float64 or not host_out.is_contiguous()
                or host_out.numel() != 2 + ha or not host_out.is_pinned()):
            raise ValueError("host_out must be a pinned contiguous float64 host tensor of 2 + H*A elements")
        self._check(self.lib.gpmpc_argmin_export(self._h, J.data_ptr(), J.numel(), int(first_global_index),
                                                 None if actions is None else actions.data_ptr(), ha,
                                                 out.data_ptr(), host_out.data_ptr(), self._stream()))
        return out

    def argmin(self, J, first_global_index=0):
        """Keep-the-best rule over J; returns (best_J, GLOBAL index) -- index -1 if nothing selectable."""
        J = self._dev(J)
        bj = C.c_double()
        bi = C.c_longlong()
        self._check(self.lib.gpmpc_argmin(self._h, J.data_ptr(), J.numel(), int(first_global_index), C.byref(bj),
                                          C.byref(bi), self._stream()))
        return float(bj.value), int(bi.value)
