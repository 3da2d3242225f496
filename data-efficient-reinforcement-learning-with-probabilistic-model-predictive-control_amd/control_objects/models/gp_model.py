"""GpStateTransitionModel -- drop-in for rl_gp_mpc/control_objects/models/gp_model.py:39-315 whose
arithmetic runs in the HIP library (C ABI of include/gpmpc.h):

    prepare_inference   -> gpmpc_prepare   (K build, Cholesky, iK, beta; reference :182-191, 400-431)
                           or gpmpc_prepare_sparse (ModelConfig.num_inducing_points: a sparse GP on inducing inputs)
    predict_trajectory  -> gpmpc_rollout   (H-step moment matching;     reference :60-180)

plus the batched entry points the reference lacks (`predict_trajectory_batch`,
`objective_and_gradient_batch`): B candidate action sequences per launch.

No gpytorch: the three hyper-parameters the hot path reads (lengthscale (1,E), outputscale (),
likelihood noise (1,), reference :189-190,427) live in small holder objects that keep the
reference's attribute paths and its `initialize(**{...})` contract
(controllers/gp_mpc_controller.py:223-224).  `train` (exact marginal likelihood, LBFGS, random
re-initialisation inside the constraint box; reference :193-306) keeps the reference's optimiser loop in the
spawned process the controller manages; its loss and gradient come from gpmpc_mll on the GPU.
"""
import time
from types import SimpleNamespace

import numpy as np
import torch

from .abstract_model import AbstractStateTransitionModel

F64 = torch.float64


def _t(v):
    return torch.as_tensor(np.asarray(v), dtype=F64) if not isinstance(v, torch.Tensor) else v.to(F64)


class _MomentsFunction(torch.autograd.Function):
    """engine.moments as an autograd node: (mu (P, E), var (P, E, E) or None) -> (M, S, V); its backward is
    engine.moments_backward (gpmpc_moments_backward).  The covariance's gradient is the symmetric part.  Once differentiable."""

    @staticmethod
    def forward(ctx, engine, mu, var):
        ctx.engine = engine
        ctx.set_materialize_grads(False)          # an unused output is a NULL upstream gradient (no S: no pairwise pass)
        ctx.save_for_backward(mu, var)
        out = engine.moments(mu, var)
        return out["M"], out["S"], out["V"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, M_bar, S_bar, V_bar):
        mu, var = ctx.saved_tensors
        want_mu, want_var = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if M_bar is None and S_bar is None and V_bar is None:
            return None, None, None
        g = ctx.engine.moments_backward(mu.detach(), var.detach() if var is not None else None, M_bar, S_bar, V_bar,
                                        mu_bar=want_mu, var_bar=want_var)
        mu_bar = g["mu_bar"].to(device=mu.device, dtype=mu.dtype) if want_mu else None
        var_bar = g["var_bar"].to(device=var.device, dtype=var.dtype) if want_var else None
        return None, mu_bar, var_bar


class _PredictFunction(torch.autograd.Function):
    """engine.predict as an autograd node: inputs (M, E) -> (mean, var) (M, D), the variance with `noises` (D,) added when they
    are given (a constant: no gradient); its backward is engine.predict_backward (gpmpc_predict_backward).  Once differentiable."""

    @staticmethod
    def forward(ctx, engine, noises, inputs):
        ctx.engine = engine
        ctx.set_materialize_grads(False)          # an unused output is a NULL upstream gradient (no var: no matrix product)
        ctx.save_for_backward(inputs)
        out = engine.predict(inputs, noises=noises)
        return out["mean"], out["var"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, mean_bar, var_bar):
        inputs, = ctx.saved_tensors
        if (mean_bar is None and var_bar is None) or not ctx.needs_input_grad[2]:
            return None, None, None
        g = ctx.engine.predict_backward(inputs.detach(), mean_bar, var_bar)
        return None, None, g.to(device=inputs.device, dtype=inputs.dtype)


class _TrajectoryFunction(torch.autograd.Function):
    """engine.rollout as an autograd node: (actions (B, H, A), obs_mu (D,), obs_var (D, D)) -> the rollout's outputs named by
    ctx.keys (mu, Sig and, where the rollout returns them, cost_mu, cost_var, J; copied into `keys_out`); its backward is engine.rollout_backward
    (gpmpc_rollout_backward, which recomputes the forward).  The shared initial state's gradients are the sums over the
    candidates; obs_var's is the symmetric part.  Once differentiable."""

    @staticmethod
    def forward(ctx, engine, include_time, time0, stage_costs, keys_out, actions, obs_mu, obs_var):
        ctx.engine, ctx.include_time, ctx.time0 = engine, include_time, time0
        ctx.set_materialize_grads(False)          # an unused output is a NULL upstream gradient
        ctx.save_for_backward(actions, obs_mu, obs_var)
        out = engine.rollout(actions, obs_mu.detach().cpu().numpy(), obs_var.detach().cpu().numpy(), include_time, time0,
                             True, stage_costs)
        ctx.keys = tuple(k for k in ("mu", "Sig", "cost_mu", "cost_var", "J") if k in out)
        keys_out[:] = ctx.keys
        return tuple(out[k] for k in ctx.keys)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        actions, obs_mu, obs_var = ctx.saved_tensors
        seeds = dict(zip(ctx.keys, grads))
        want_act, want_mu, want_var = ctx.needs_input_grad[5:8]
        if all(g is None for g in grads):
            return None, None, None, None, None, None, None, None
        g = ctx.engine.rollout_backward(actions.detach(), obs_mu.detach().cpu().numpy(), obs_var.detach().cpu().numpy(),
                                        ctx.include_time, ctx.time0, mu_bar=seeds.get("mu"), Sig_bar=seeds.get("Sig"),
                                        cost_mu_bar=seeds.get("cost_mu"), cost_var_bar=seeds.get("cost_var"),
                                        J_bar=seeds.get("J"), want_initial=want_mu or want_var)
        act_bar = g["actions_bar"].to(device=actions.device, dtype=actions.dtype) if want_act else None
        # one reduction over the candidates (a fixed order for a given B)
        mu_bar = g["mu0_bar"].sum(0).reshape(obs_mu.shape).to(device=obs_mu.device, dtype=obs_mu.dtype) if want_mu else None
        var_bar = g["S0_bar"].sum(0).reshape(obs_var.shape).to(device=obs_var.device, dtype=obs_var.dtype) if want_var else None
        return None, None, None, None, None, act_bar, mu_bar, var_bar


def _check_trajectory_grad_shape(D, A, include_time):
    """The shapes gpmpc_rollout_backward covers (D <= 8 with A (+ time) <= 6, and 8 < D <= 16): raised at the forward, not at
    backward()."""
    if (D <= 8 and A + int(bool(include_time)) <= 6) or 8 < D <= 16:
        return
    from ..._lib import GPMPC_ERR_LIMIT, GpmpcError
    raise GpmpcError(GPMPC_ERR_LIMIT, f"predict_trajectory gradients: D = {D}, A = {A}{' + time' if include_time else ''} is "
                     "outside the gradient kernels (D <= 8 with A (+ time) <= 6, or 8 < D <= 16); differentiate such shapes by "
                     "chaining predict_next_state_change, whose gradients cover them")


PROPAGATIONS = ("moment_matching", "linearized")


def inducing_rows(N, M):
    """The rows of an N-point memory that serve as the M inducing inputs of the sparse model (ModelConfig.num_inducing_points):
    round(i (N - 1) / (M - 1)), i = 0..M-1 (M = 1: row 0) -- deterministic, first and last point included, distinct for M <= N."""
    if M == 1:
        return [0]
    return [int(round(i * (N - 1) / (M - 1))) for i in range(M)]


def _renumber_inducing(inducing_idx, gone):
    """`inducing_idx` (a list, or an int32 device tensor) after the ascending memory rows `gone` have left: every entry moves down
    by the number of departed rows below it; an entry whose own row has left -- or had left before -- is -1."""
    if isinstance(inducing_idx, torch.Tensor):
        gone_t = torch.as_tensor(np.asarray(gone), dtype=torch.long, device=inducing_idx.device)
        old = inducing_idx.to(torch.long)
        new = torch.where(torch.isin(old, gone_t) | (old < 0), torch.full_like(old, -1), old - torch.searchsorted(gone_t, old))
        return new.to(inducing_idx.dtype)
    gone = np.asarray(gone, dtype=np.int64)
    old = np.asarray(inducing_idx, dtype=np.int64)
    new = np.where(np.isin(old, gone) | (old < 0), -1, old - np.searchsorted(gone, old))
    return [int(v) for v in new]


def _no_linearized_autograd(what, *tensors):
    """The linearised propagation has no backward kernels: refuse rather than return tensors without a grad_fn."""
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors):
        raise NotImplementedError(f"{what}: propagation='linearized' has no autograd; detach the inputs or run under "
                                  "torch.no_grad(), or use propagation='moment_matching'")


class SavedState:
    """In-memory snapshot shipped to the training process (reference gp_model.py:13-36)."""

    def __init__(self, inputs, states_change, parameters, constraints_hyperparams):
        self.inputs = inputs
        self.states_change = states_change
        self.parameters = parameters
        self.constraints_hyperparams = constraints_hyperparams

    def to_arrays(self):
        self.inputs = np.asarray(self.inputs)
        self.states_change = np.asarray(self.states_change)
        self.parameters = [{k: np.asarray(v) for k, v in p.items()} for p in self.parameters]
        self.constraints_hyperparams = {k: (v.numpy() if isinstance(v, torch.Tensor) else v)
                                        for k, v in self.constraints_hyperparams.items()}

    def to_tensors(self):
        self.inputs = _t(self.inputs)
        self.states_change = _t(self.states_change)
        self.parameters = [{k: _t(v) for k, v in p.items()} for p in self.parameters]
        self.constraints_hyperparams = {k: (_t(v) if isinstance(v, np.ndarray) else v)
                                        for k, v in self.constraints_hyperparams.items()}


class GpHyperParameters:
    """One ExactGP's hyper-parameters under the reference's attribute paths
    (covar_module.base_kernel.lengthscale (1,E), covar_module.outputscale (), likelihood.noise (1,))."""

    KEYS = ("covar_module.base_kernel.lengthscale", "covar_module.outputscale", "likelihood.noise")

    def __init__(self, lengthscale, outputscale, noise):
        self.covar_module = SimpleNamespace(base_kernel=SimpleNamespace(lengthscale=None), outputscale=None)
        self.likelihood = SimpleNamespace(noise=None)
        self.initialize(**{self.KEYS[0]: lengthscale, self.KEYS[1]: outputscale, self.KEYS[2]: noise})

    def initialize(self, **kwargs):
        for key, val in kwargs.items():
            v = _t(val)
            if key == self.KEYS[0]:
                self.covar_module.base_kernel.lengthscale = v.reshape(1, -1)
            elif key == self.KEYS[1]:
                self.covar_module.outputscale = v.reshape(())
            elif key == self.KEYS[2]:
                self.likelihood.noise = v.reshape(1)
            else:
                raise KeyError(key)
        return self

    def state_dict(self):
        return {self.KEYS[0]: self.covar_module.base_kernel.lengthscale.clone(),
                self.KEYS[1]: self.covar_module.outputscale.clone(),
                self.KEYS[2]: self.likelihood.noise.clone()}

    def eval(self):
        return self


def create_models(gp_init_dict, num_models, num_inputs):
    """Hyper-parameter holders initialised from ModelConfig.gp_init (reference :318-384)."""
    if isinstance(gp_init_dict, list):
        return [GpHyperParameters(p[GpHyperParameters.KEYS[0]], p[GpHyperParameters.KEYS[1]], p[GpHyperParameters.KEYS[2]])
                for p in gp_init_dict]
    ls = _t(gp_init_dict["base_kernel.lengthscale"])
    return [GpHyperParameters(ls[i].expand(num_inputs) if ls[i].ndim == 0 else ls[i],
                              _t(gp_init_dict["outputscale"])[i], _t(gp_init_dict["noise_covar.noise"])[i])
            for i in range(num_models)]


class TrainingFailed(list):
    """Answer of a training process that could not train: the list of the INCOMING parameter dicts (so a consumer
    that only wants parameters can use it as is) with the reason attached."""

    def __init__(self, parameters=(), reason=""):
        super().__init__(parameters)
        self.reason = reason

    def __reduce__(self):
        return (TrainingFailed, (list(self), self.reason))


_DEVICE_SEARCH_MAX_N = 256          # memory points one workgroup of gpmpc_mll_batch holds


class _LockstepMll:
    """Rendezvous of the per-GP optimiser threads of `train`: a thread asks for the loss of its GP and waits; when every
    unfinished GP is waiting, the last one to arrive evaluates ALL pending GPs with one gpmpc_mll call (the kernels
    batch over GPs).  If the batched call fails (a GP whose K is not positive definite at its trial point), the pending
    GPs are evaluated one by one so that only the failing GP sees the error."""

    WAIT_LIMIT = 600.0

    def __init__(self, engine, X_dev, Y_dev, n_gp):
        import threading
        self.engine, self.X, self.Y = engine, X_dev, Y_dev
        self.cond = threading.Condition()
        self.pending, self.results = {}, {}
        self.running = n_gp
        self.launches = 0

    def _flush(self):                                  # called with the lock held
        idx = sorted(self.pending)
        try:
            self._evaluate_pending(idx)
        except BaseException as e:                     # anything outside the per-GP handling below (stacking, indexing, ...):
            for i in idx:                              # every waiting GP gets a failure -- nobody may wait forever
                self.results.setdefault(i, e if isinstance(e, Exception) else RuntimeError(repr(e)))
            if not isinstance(e, Exception):           # KeyboardInterrupt / SystemExit: the waiters are served (above) and
                raise                                  # the interrupt itself goes on in the flushing thread, not swallowed
        finally:
            self.pending.clear()
            self.cond.notify_all()

    def _evaluate_pending(self, idx):
        ls = torch.stack([self.pending[i][0].reshape(-1) for i in idx])
        osc = torch.stack([self.pending[i][1].reshape(()) for i in idx])
        nz = torch.stack([self.pending[i][2].reshape(()) for i in idx])
        try:
            out = self.engine.mll(self.X, self.Y[:, idx].contiguous(), ls, osc, nz)
            self.launches += 1
            for k, i in enumerate(idx):
                self.results[i] = (float(out["loss"][k]), out["d_lengthscale"][k], float(out["d_outputscale"][k]),
                                   float(out["d_noise"][k]))
        except Exception:
            for k, i in enumerate(idx):
                try:
                    o = self.engine.mll(self.X, self.Y[:, i:i + 1].contiguous(), ls[k:k + 1], osc[k:k + 1], nz[k:k + 1])
                    self.launches += 1
                    self.results[i] = (float(o["loss"][0]), o["d_lengthscale"][0], float(o["d_outputscale"][0]),
                                       float(o["d_noise"][0]))
                except Exception as e:
                    self.results[i] = e

    def evaluate(self, a, ls, osc, nz):
        with self.cond:
            self.pending[a] = (ls, osc, nz)
            if len(self.pending) == self.running:
                self._flush()
            waited = 0.0
            while a not in self.results:
                # a rendezvous that never completes (a sibling thread died outside `finished`) must not hang the training
                # process: after WAIT_LIMIT seconds the evaluation fails and `train` reports TrainingFailed
                if not self.cond.wait(timeout=5.0):
                    waited += 5.0
                    if waited >= self.WAIT_LIMIT:
                        # withdraw the request: a stale entry would be counted by `finished` (premature flush that includes
                        # it, one wasted evaluation and a result nobody pops)
                        self.pending.pop(a, None)
                        raise TimeoutError(f"lockstep evaluation of GP {a} not served within {self.WAIT_LIMIT:.0f} s")
            r = self.results.pop(a)
        if isinstance(r, Exception):
            raise r
        return r

    def finished(self, a):
        with self.cond:
            self.running -= 1
            if self.pending and len(self.pending) == self.running:
                self._flush()


class _DeviceNegMll(torch.autograd.Function):
    """-log p(y | X, theta) / N with its gradient from gpmpc_mll (reference: gpytorch ExactMarginalLogLikelihood +
    autograd, gp_model.py:262-275); `shared` batches the evaluations of the GPs that are waiting (see _LockstepMll)."""

    @staticmethod
    def forward(ctx, ls, osc, nz, shared, a):
        loss, gl, go, gn = shared.evaluate(a, ls.detach(), osc.detach(), nz.detach())
        ctx.shapes = (ls.shape, osc.shape, nz.shape)
        ctx.grads = (gl, go, gn)
        return torch.tensor(loss, dtype=F64)

    @staticmethod
    def backward(ctx, gout):
        gl, go, gn = ctx.grads
        sl, so, sn = ctx.shapes
        return (gout * torch.as_tensor(gl, dtype=F64).reshape(sl), gout * torch.tensor(float(go), dtype=F64).reshape(so),
                gout * torch.tensor(float(gn), dtype=F64).reshape(sn), None, None)


class GpStateTransitionModel(AbstractStateTransitionModel):
    def __init__(self, config, dim_state, dim_action, engine=None, device=None):
        super().__init__(config, dim_state, dim_action)
        if self.config.include_time_model:
            self.dim_input += 1
        self.config.extend_dimensions_params(dim_state=self.dim_state, dim_input=self.dim_input)
        self.models = create_models(self.config.gp_init, self.dim_state, self.dim_input)
        self._engine = engine
        self._device = device
        self.x_mem = None
        self.y_mem = None
        self._cost_key = None
        self.is_sparse = False          # the cached model is the sparse one of gpmpc_prepare_sparse
        self.inducing_idx = None        # rows of the memory its inducing inputs are: a list (strided), a device tensor (greedy), or None
        self._sparse_record = None      # ModelConfig.inducing_refresh_every: hyper-parameters of the last sparse prepare, rows changed since

    last_training_launches = None       # gpmpc_mll calls of the last `train` in this process (lockstep: ~ the longest GP's count)

    # -- engine ------------------------------------------------------------------------
    @property
    def engine(self):
        if self._engine is None:
            from ...engine import HipEngine       # raises without a GPU / without the HIP library
            self._engine = HipEngine(self._device)
        return self._engine

    @property
    def lengthscales(self):
        return torch.stack([m.covar_module.base_kernel.lengthscale[0] for m in self.models])

    @property
    def variances(self):
        return torch.stack([m.covar_module.outputscale for m in self.models])

    @property
    def noises(self):
        return torch.stack([m.likelihood.noise[0] for m in self.models])

    @property
    def iK(self):
        return self.engine.factors()[0].cpu()

    @property
    def beta(self):
        return self.engine.factors()[1].cpu()

    # -- a1/a2 -------------------------------------------------------------------------
    def prepare_inference(self, inputs, state_changes, inducing_inputs=None):
        """Cache the model of the memory (inputs (N, E), state_changes (N, D)).  With ModelConfig.num_inducing_points = M and
        more than M memory points -- or with explicit `inducing_inputs` (M', E), which override the choice below -- the cached
        model is the sparse GP of gpmpc_prepare_sparse on the inducing inputs: the rows round(i (N - 1) / (M - 1)), i = 0..M-1,
        of `inputs` (M = 1: row 0), a deterministic spread over the memory in its order -- or, with
        ModelConfig.inducing_selection = "greedy", the M rows gpmpc_select_inducing picks under the current hyper-parameters,
        chosen afresh at every call (nothing is cached that training or a memory change could make stale) and handed to
        gpmpc_prepare_sparse on the device.  Otherwise (the option unset, or N <= M) it is the exact GP, as ever.
        `inducing_idx` records the chosen rows: a list (strided), an int32 device tensor (greedy), None otherwise.  x_mem /
        y_mem are the whole memory either way: training and save_state see all of it.
        With ModelConfig.inducing_refresh_every = R the sparse model the config chose is not rebuilt when the memory only grew:
        if `inputs` / `state_changes` are the previous memory followed by k >= 1 rows (compared by value), the hyper-parameters
        are those of the last sparse prepare and no more than R rows have been appended (or, with inducing_forget, forgotten)
        since it, the k rows go through gpmpc_sparse_append (O(k M^2), same inducing inputs, `inducing_idx` kept); with k = 0 no
        call is made at all.  Anything else -- and an engine that answers the append with GPMPC_ERR_ARG -- rebuilds as above and starts the count again."""
        if inducing_inputs is None and self._try_sparse_append(inputs, state_changes):
            return
        self._sparse_record = None
        self.x_mem = inputs
        self.y_mem = state_changes
        self.inducing_idx = None
        M = getattr(self.config, "num_inducing_points", None)
        if inducing_inputs is None and M is not None and len(inputs) > M:
            if getattr(self.config, "inducing_selection", "strided") == "greedy":
                sel = self.engine.select_inducing(inputs, M, self.lengthscales, self.variances,
                                                  getattr(self.config, "inducing_jitter", 1e-6))
                self.inducing_idx, inducing_inputs = sel["idx"], sel["Z"]
            else:
                self.inducing_idx = inducing_rows(len(inputs), M)
                inducing_inputs = _t(inputs)[self.inducing_idx]
        self.is_sparse = inducing_inputs is not None
        if self.is_sparse:
            self.engine.prepare_sparse(inputs, state_changes, inducing_inputs, self.lengthscales, self.variances, self.noises,
                                       getattr(self.config, "inducing_jitter", 1e-6))
            if self.inducing_idx is not None and getattr(self.config, "inducing_refresh_every", None) is not None:
                self._sparse_record = {"hyp": self._hyper_parameters(), "changed": 0}
        else:
            self.engine.prepare(inputs, state_changes, self.lengthscales, self.variances, self.noises)

    def _hyper_parameters(self):
        return tuple(t.detach().clone() for t in (self.lengthscales, self.variances, self.noises))

    def _try_sparse_append(self, inputs, state_changes):
        """The append policy of ModelConfig.inducing_refresh_every (see prepare_inference): True when the cached sparse model
        already is, or by gpmpc_sparse_append has become, the model of this memory."""
        rec = getattr(self, "_sparse_record", None)
        R = getattr(self.config, "inducing_refresh_every", None)
        if rec is None or R is None or not self.is_sparse or self.x_mem is None:
            return False
        if not all(torch.equal(a, b) for a, b in zip(rec["hyp"], self._hyper_parameters())):
            return False
        x_new, y_new, x_old, y_old = _t(inputs), _t(state_changes), _t(self.x_mem), _t(self.y_mem)
        n_prev, k = len(x_old), len(x_new) - len(x_old)
        if k < 0 or len(y_new) != len(x_new) or x_new.shape[1:] != x_old.shape[1:] or y_new.shape[1:] != y_old.shape[1:]:
            return False
        if not (torch.equal(x_new[:n_prev].cpu(), x_old.cpu()) and torch.equal(y_new[:n_prev].cpu(), y_old.cpu())):
            return False
        if k > 0:
            if rec["changed"] + k > R:
                return False
            from ..._lib import GPMPC_ERR_ARG, GpmpcError
            try:
                self.engine.sparse_append(inputs[n_prev:], state_changes[n_prev:])
            except GpmpcError as e:
                if e.code != GPMPC_ERR_ARG:
                    raise
                return False                     # the engine holds no record (any more): rebuild
            rec["changed"] += k
        self.x_mem = inputs
        self.y_mem = state_changes
        return True

    def forget(self, indices):
        """Drop the memory points `indices` (strictly ascending rows of the memory of the last prepare_inference) from the
        cached model (gpmpc_forget, O(k N^2)) and from x_mem / y_mem, so that save_state ships the reduced memory to training.
        A prepare_inference of the reduced memory plus a few appended points is then a border update, not a factorisation.
        A sparse model (ModelConfig.num_inducing_points) has no downdate -- its factors condense all memory points into the
        inducing ones: GpmpcError(GPMPC_ERR_ARG), with the model and x_mem / y_mem untouched; call prepare_inference on the
        reduced memory instead (the controller does: a capped memory re-prepares its window).
        With ModelConfig.inducing_forget = True and inducing_refresh_every = R the sparse model the config chose does have one:
        under the hyper-parameters of its last rebuild, fewer rows than the memory holds leave it through gpmpc_sparse_forget
        (O(k M^2), by their values, same inducing inputs) as long as no more than R rows have been appended or forgotten since
        that rebuild -- past R no call is made and GpmpcError(GPMPC_ERR_ARG) is raised as above, so that the caller's
        prepare_inference rebuilds: that is the refresh.  `inducing_idx` keeps its kind and is renumbered to the reduced memory,
        with -1 for an inducing input whose memory row has left (the input itself stays).  Where the engine loses a pivot
        (GPMPC_ERR_NOT_PD: it then holds no model) the rows leave x_mem / y_mem all the same and the model of the reduced memory is
        rebuilt by prepare_inference: the caller sees a successful forget.  An engine without a record re-raises its
        GPMPC_ERR_ARG with the memory untouched."""
        if self.x_mem is None:
            raise RuntimeError("call prepare_inference(inputs, state_changes) before forget")
        if getattr(self, "is_sparse", False):
            return self._sparse_forget(indices)
        idx = np.asarray(indices).reshape(-1)
        self.engine.forget(idx)
        keep = torch.ones(len(self.x_mem), dtype=torch.bool)
        keep[torch.as_tensor(idx, dtype=torch.long)] = False
        self.x_mem = _t(self.x_mem)[keep]
        self.y_mem = _t(self.y_mem)[keep]

    def _sparse_forget(self, indices):
        """`forget` on a sparse model: the policy of ModelConfig.inducing_forget (see forget)."""
        from ..._lib import GPMPC_ERR_ARG, GPMPC_ERR_NOT_PD, GpmpcError
        rec = getattr(self, "_sparse_record", None)
        R = getattr(self.config, "inducing_refresh_every", None)
        if not getattr(self.config, "inducing_forget", False) or R is None or rec is None:
            raise GpmpcError(GPMPC_ERR_ARG, "forget: the cached model is sparse (ModelConfig.num_inducing_points) and has no "
                             "downdate; call prepare_inference on the reduced memory")
        idx = np.asarray(indices).reshape(-1)
        n, k = len(self.x_mem), int(idx.size)
        if k and not np.issubdtype(idx.dtype, np.integer):
            raise TypeError("forget: indices must be integers")
        if k < 1 or k >= n or idx[0] < 0 or idx[-1] >= n or np.any(np.diff(idx) <= 0):
            raise GpmpcError(GPMPC_ERR_ARG, "forget: need 1 <= k < N strictly ascending rows in [0, N)")
        if not all(torch.equal(a, b) for a, b in zip(rec["hyp"], self._hyper_parameters())):
            raise GpmpcError(GPMPC_ERR_ARG, "forget: the hyper-parameters changed since the sparse model was built; call "
                             "prepare_inference on the reduced memory")
        if rec["changed"] + k > R:
            raise GpmpcError(GPMPC_ERR_ARG, f"forget: more than inducing_refresh_every = {R} rows changed since the sparse model "
                             "was built; call prepare_inference on the reduced memory")
        x_mem, y_mem = _t(self.x_mem), _t(self.y_mem)
        rows = torch.as_tensor(idx, dtype=torch.long)
        keep = torch.ones(n, dtype=torch.bool)
        keep[rows] = False
        rows, keep = rows.to(x_mem.device), keep.to(x_mem.device)
        lost_pivot = False
        try:
            self.engine.sparse_forget(x_mem[rows], y_mem[rows])
        except GpmpcError as e:
            if e.code != GPMPC_ERR_NOT_PD:
                raise                                # GPMPC_ERR_ARG: no record -- the memory stays, as on the exact path
            lost_pivot = True
        if lost_pivot:                               # the engine holds no model: the reduced memory through the full path
            self._sparse_record = None
            self.prepare_inference(x_mem[keep], y_mem[keep])
            return
        self.x_mem, self.y_mem = x_mem[keep], y_mem[keep]
        rec["changed"] += k
        self.inducing_idx = _renumber_inducing(self.inducing_idx, idx)

    def set_cost(self, reward_config):
        """Load the quadratic-cost / LCB settings into the engine.  The reference reads its reward config on every
        evaluation (setpoint_distance_reward_mapper.py:36-66), so in-place edits of the config must take effect:
        the (tiny) packed settings are compared by CONTENT with what this engine last received and re-sent when
        they differ -- a few hundred bytes of host work per call, no launch."""
        smin = reward_config.state_min if reward_config.use_constraints else None
        smax = reward_config.state_max if reward_config.use_constraints else None
        args = (reward_config.target_state_action_norm.numpy(), reward_config.weight_matrix_cost.numpy(),
                reward_config.weight_matrix_cost_terminal.numpy(), float(reward_config.exploration_factor),
                bool(reward_config.clip_lower_bound_cost_to_0),
                None if smin is None else smin.numpy(), None if smax is None else smax.numpy())
        key = tuple(None if a is None else (np.asarray(a, dtype=np.float64).tobytes()) for a in args)
        if getattr(self.engine, "_cost_token", None) == key:
            self._cost_key = key
            return
        self.engine.set_cost(*args)
        self._cost_key = key
        self.engine._cost_token = key          # engines can be shared between models: remember WHAT is loaded

    def propagation(self, propagation=None):
        """The uncertainty propagation a call uses: its own `propagation` argument, or ModelConfig.uncertainty_propagation."""
        if propagation is None:
            propagation = getattr(self.config, "uncertainty_propagation", "moment_matching")
        if propagation not in PROPAGATIONS:
            raise ValueError(f"propagation must be one of {PROPAGATIONS}, got {propagation!r}")
        return propagation

    # -- a3/a4 -------------------------------------------------------------------------
    def predict_trajectory_batch(self, actions, obs_mu, obs_var, len_horizon=None, current_time_idx=0,
                                 trajectories=True, stage_costs=True, propagation=None, feedback_gains=None, lqr_reg=0.0):
        """actions (B,H,A) -> dict of DEVICE tensors: J (B,), mu (B,H+1,D), Sig (B,H+1,D,D),
        cost_mu / cost_var (B,H+1).  Costs need set_cost() first.  Differentiable like the reference's predict_trajectory
        followed by get_rewards_trajectory: when grad mode is on and actions, obs_mu or obs_var requires grad, mu, Sig and
        (with set_cost) cost_mu, cost_var and J carry a grad_fn, and backward() reaches the inputs (CPU or device, each
        gradient in its input's dtype) through gpmpc_rollout_backward, which recomputes the forward.  obs_mu and obs_var are
        shared by the candidates: their gradients are the sums over the batch, obs_var's the symmetric part of the
        reference's.  The time input, hyper-parameters and memory get no gradient, and double backward raises.  Shapes outside
        the gradient kernels (D <= 8 with A (+ time) <= 6, or 8 < D <= 16) raise GpmpcError(GPMPC_ERR_LIMIT) here, before any
        launch; chain predict_next_state_change to differentiate those.
        `propagation` (None: ModelConfig.uncertainty_propagation): "linearized" runs gpmpc_rollout_linear instead -- the same
        dict, no autograd (NotImplementedError when grad mode is on and an input requires grad).
        `feedback_gains` (model space; (A, D), (H, A, D) or (B, H, A, D)): the linearised rollout in closed loop under
        u = actions_t + K_t (x - mu_t) (gpmpc_rollout_linear_feedback) -- Sig and the stage costs are the closed-loop ones, mu
        is unchanged.  Only with "linearized" (ValueError with moment matching, whose closed-loop rollout is
        predict_trajectory_feedback_batch), and without autograd like it.
        `feedback_gains="lqr"`: every candidate's own LQR gains, designed on the device along its nominal trajectory on the
        loaded cost (gpmpc_lqr_gains, `lqr_reg` added to the diagonal of Huu) and handed to the closed-loop rollout without
        leaving it; the dict then also holds "gains" (B, H, A, D).  Any other string is a ValueError."""
        if self._cost_key is None and stage_costs:
            raise RuntimeError("call set_cost(reward_config) before predicting costs")
        if isinstance(feedback_gains, str) and feedback_gains != "lqr":
            raise ValueError(f"feedback_gains must be an array or 'lqr', got {feedback_gains!r}")
        if feedback_gains is not None and self.propagation(propagation) != "linearized":
            raise ValueError("feedback_gains need propagation='linearized' here; the closed-loop rollout under moment matching "
                             "is predict_trajectory_feedback / predict_trajectory_feedback_batch")
        if self.propagation(propagation) == "linearized":
            _no_linearized_autograd("predict_trajectory", actions, obs_mu, obs_var, feedback_gains)
            actions = torch.as_tensor(np.asarray(actions) if not isinstance(actions, torch.Tensor) else actions, dtype=F64)
            if len_horizon is not None and actions.shape[1] != len_horizon:
                raise ValueError("actions.shape[1] != len_horizon")
            if isinstance(feedback_gains, str):           # "lqr"
                if self._cost_key is None:
                    raise RuntimeError("call set_cost(reward_config) before feedback_gains='lqr': the gains are designed on it")
                return self.engine.rollout_linear_lqr(actions, _t(obs_mu).numpy(), _t(obs_var).numpy(),
                                                      self.config.include_time_model, float(current_time_idx), trajectories,
                                                      stage_costs, reg=float(lqr_reg))
            if feedback_gains is not None:
                gains = feedback_gains if isinstance(feedback_gains, torch.Tensor) else np.asarray(feedback_gains)
                return self.engine.rollout_linear_feedback(actions, torch.as_tensor(gains, dtype=F64), _t(obs_mu).numpy(),
                                                           _t(obs_var).numpy(), self.config.include_time_model,
                                                           float(current_time_idx), trajectories, stage_costs)
            return self.engine.rollout_linear(actions, _t(obs_mu).numpy(), _t(obs_var).numpy(), self.config.include_time_model,
                                              float(current_time_idx), trajectories, stage_costs)
        grads = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (actions, obs_mu, obs_var))
        actions = torch.as_tensor(np.asarray(actions) if not isinstance(actions, torch.Tensor) else actions, dtype=F64)
        if len_horizon is not None and actions.shape[1] != len_horizon:
            raise ValueError("actions.shape[1] != len_horizon")
        if not grads:
            return self.engine.rollout(actions, _t(obs_mu).numpy(), _t(obs_var).numpy(), self.config.include_time_model,
                                       float(current_time_idx), trajectories, stage_costs)
        _check_trajectory_grad_shape(self.dim_state, actions.shape[2], self.config.include_time_model)
        keys = []
        outs = _TrajectoryFunction.apply(self.engine, self.config.include_time_model, float(current_time_idx), stage_costs, keys,
                                         actions, _t(obs_mu), _t(obs_var))
        out = dict(zip(keys, outs))
        if not trajectories:
            del out["mu"], out["Sig"]
        return out

    def objective_and_gradient_batch(self, actions, obs_mu, obs_var, current_time_idx=0, trajectories=False):
        """actions (B,H,A) -> dict of DEVICE tensors: J (B,), grad (B,H,A) = dJ/d(actions) (analytic; what the
        reference gets from autograd, gp_mpc_controller.py:277), optionally the trajectories and costs."""
        if self._cost_key is None:
            raise RuntimeError("call set_cost(reward_config) before predicting")
        actions = torch.as_tensor(np.asarray(actions) if not isinstance(actions, torch.Tensor) else actions, dtype=F64)
        return self.engine.rollout_grad(actions, _t(obs_mu).numpy(), _t(obs_var).numpy(), self.config.include_time_model,
                                        float(current_time_idx), trajectories)

    def feedback_objective_and_gradient_batch(self, actions, feedback_gains, obs_mu, obs_var, current_time_idx=0):
        """The closed-loop counterpart of objective_and_gradient_batch under moment matching (gpmpc_rollout_feedback, then
        gpmpc_rollout_feedback_backward with J_bar = 1): actions (B,H,A) and `feedback_gains` (model space; (A, D), (H, A, D) or
        (B, H, A, D)) -> dict of DEVICE tensors J (B,), grad (B,H,A) = dJ/d(actions) and gains_grad = dJ/d(feedback_gains) in the
        shape of `feedback_gains`: the per-candidate gradients summed the way the gains were broadcast -- over the candidates and
        steps for (A, D), over the candidates for (H, A, D) (the sum of the candidates' objectives is what such a gain moves).
        `feedback_gains="lqr"` is a ValueError: no gradient flows through the gain design."""
        if self._cost_key is None:
            raise RuntimeError("call set_cost(reward_config) before predicting")
        if feedback_gains is None or isinstance(feedback_gains, str):
            raise ValueError(f"feedback_gains must be an array (no gradient flows through a gain design), got {feedback_gains!r}")
        actions = torch.as_tensor(np.asarray(actions) if not isinstance(actions, torch.Tensor) else actions, dtype=F64)
        gains = torch.as_tensor(feedback_gains if isinstance(feedback_gains, torch.Tensor) else np.asarray(feedback_gains), dtype=F64)
        out = self.engine.rollout_feedback_grad(actions, gains, _t(obs_mu).numpy(), _t(obs_var).numpy(),
                                                self.config.include_time_model, float(current_time_idx))
        if gains.dim() == 2:
            out["gains_grad"] = out["gains_grad"].sum((0, 1))
        elif gains.dim() == 3:
            out["gains_grad"] = out["gains_grad"].sum(0)
        return out

    def objective_and_gradient_host(self, actions, obs_mu, obs_var, current_time_idx=0):
        """ONE sequence (H, A) -> dict of HOST (numpy) arrays J (1,), grad (1,H,A), mu, Sig, cost_mu, cost_var: the shape of call
        scipy's L-BFGS-B makes (gp_mpc_controller.py:133-141, 229-285), served by gpmpc_objective_grad_host with one
        synchronisation and no torch tensors in between."""
        if self._cost_key is None:
            raise RuntimeError("call set_cost(reward_config) before predicting")
        return self.engine.objective_grad_host(np.asarray(actions, dtype=np.float64), _t(obs_mu).numpy(), _t(obs_var).numpy(),
                                               self.config.include_time_model, float(current_time_idx))

    def predict_trajectory(self, actions, obs_mu, obs_var, len_horizon, current_time_idx, propagation=None,
                           feedback_gains=None, lqr_reg=0.0):
        """Same signature / return shapes as the reference (:60-110): ((H+1,D), (H+1,D,D)) CPU tensors.  Differentiable like
        the reference: when grad mode is on and actions, obs_mu or obs_var requires grad, both outputs carry a grad_fn and
        backward() reaches the inputs through gpmpc_rollout_backward (see predict_trajectory_batch); obs_var's gradient is the
        symmetric part of the reference's.  `propagation`, `feedback_gains` ((A, D), (H, A, D) or "lqr"), `lqr_reg`: see
        predict_trajectory_batch."""
        out = self.predict_trajectory_batch(_t(actions)[None], obs_mu, obs_var, len_horizon, current_time_idx,
                                            trajectories=True, stage_costs=False, propagation=propagation,
                                            feedback_gains=feedback_gains, lqr_reg=lqr_reg)
        return out["mu"][0].cpu(), out["Sig"][0].cpu()

    def predict_trajectory_feedback_batch(self, actions, feedback_gains, obs_mu, obs_var, len_horizon=None, current_time_idx=0,
                                          trajectories=True, stage_costs=True, lqr_reg=0.0):
        """The moment-matched rollout in closed loop under u = actions_t + K_t (x - mu_t) (gpmpc_rollout_feedback): the dict of
        predict_trajectory_batch, with mu, Sig and the stage costs those of the policy -- under moment matching the gains move
        mu as well.  Always moment-matched, whatever ModelConfig.uncertainty_propagation is.  `feedback_gains` (model space):
        (A, D), (H, A, D), (B, H, A, D), or "lqr": every candidate's own LQR gains (gpmpc_lqr_gains on the loaded cost, `lqr_reg`
        added to the diagonal of Huu), kept on the device; the dict then also holds "gains" (B, H, A, D).  No autograd
        (NotImplementedError when grad mode is on and an input requires grad); the realised action is not clipped."""
        if self._cost_key is None and stage_costs:
            raise RuntimeError("call set_cost(reward_config) before predicting costs")
        if feedback_gains is None or (isinstance(feedback_gains, str) and feedback_gains != "lqr"):
            raise ValueError(f"feedback_gains must be an array or 'lqr', got {feedback_gains!r}")
        if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad
                                           for t in (actions, obs_mu, obs_var, feedback_gains)):
            raise NotImplementedError("predict_trajectory_feedback: the closed-loop moment-matched rollout has no autograd; "
                                      "detach the inputs or run under torch.no_grad()")
        actions = torch.as_tensor(np.asarray(actions) if not isinstance(actions, torch.Tensor) else actions, dtype=F64)
        if len_horizon is not None and actions.shape[1] != len_horizon:
            raise ValueError("actions.shape[1] != len_horizon")
        args = (_t(obs_mu).numpy(), _t(obs_var).numpy(), self.config.include_time_model, float(current_time_idx), trajectories,
                stage_costs)
        if isinstance(feedback_gains, str):               # "lqr"
            if self._cost_key is None:
                raise RuntimeError("call set_cost(reward_config) before feedback_gains='lqr': the gains are designed on it")
            return self.engine.rollout_feedback_lqr(actions, *args, reg=float(lqr_reg))
        gains = feedback_gains if isinstance(feedback_gains, torch.Tensor) else np.asarray(feedback_gains)
        return self.engine.rollout_feedback(actions, torch.as_tensor(gains, dtype=F64), *args)

    def predict_trajectory_feedback(self, actions, feedback_gains, obs_mu, obs_var, len_horizon, current_time_idx, lqr_reg=0.0):
        """ONE action sequence (H, A) -> ((H+1,D), (H+1,D,D)) CPU tensors of the closed-loop moment-matched trajectory:
        predict_trajectory's shapes, predict_trajectory_feedback_batch's policy (`feedback_gains` (A, D), (H, A, D) or "lqr")."""
        out = self.predict_trajectory_feedback_batch(_t(actions)[None], feedback_gains, obs_mu, obs_var, len_horizon,
                                                     current_time_idx, trajectories=True, stage_costs=False, lqr_reg=lqr_reg)
        return out["mu"][0].cpu(), out["Sig"][0].cpu()

    def predict(self, inputs, include_noise=True):
        """GP posterior at the model inputs (M, E) -> (mean, var), DEVICE tensors (M, D): what the reference's model plot gets
        from likelihood(model(x)) (static_3d_graph.py:77-80, 116) -- the exact posterior, with each GP's noise added when
        `include_noise` (without it: the latent function's variance).  Differentiable in `inputs` like the reference's
        expression: when grad mode is on and `inputs` requires grad, both outputs carry a grad_fn and backward() reaches the
        inputs (CPU or device) through gpmpc_predict_backward.  The noise is a constant; hyper-parameters and the memory get no
        gradient, and double backward raises."""
        if self.x_mem is None:
            raise RuntimeError("call prepare_inference(inputs, state_changes) before predict")
        noises = self.noises.detach().cpu().numpy() if include_noise else None
        if not (torch.is_grad_enabled() and isinstance(inputs, torch.Tensor) and inputs.requires_grad):
            out = self.engine.predict(inputs, noises=noises)
            return out["mean"], out["var"]
        return _PredictFunction.apply(self.engine, noises, _t(inputs))

    def predict_cov(self, inputs, other=None, include_noise=True):
        """Joint GP posterior covariance at the model inputs, a DEVICE tensor: what the reference reads as
        likelihood(model(x)).covariance_matrix (static_3d_graph.py:77-80, gp_model.py:394-397), per output -- the exact
        posterior.  Joint form, `inputs` (M, E) alone: (D, M, M), exactly symmetric, diagonal = `predict`'s variance, each
        GP's noise added to the diagonal when `include_noise`.  Cross form, `other` (Mb, E) given: (D, M, Mb), the covariance
        between the two sets; no noise is ever added.  Not clamped and without jitter: regularise before factorising it.  No
        autograd: the result carries no grad_fn even when the inputs require grad."""
        if self.x_mem is None:
            raise RuntimeError("call prepare_inference(inputs, state_changes) before predict_cov")
        noises = self.noises.detach().cpu().numpy() if include_noise and other is None else None
        return self.engine.predict_cov(_t(inputs).detach(), None if other is None else _t(other).detach(), noises=noises)

    def predict_next_state_change(self, input_mu, input_var, propagation=None):
        """Same signature / return as the reference (:112-180): one Gaussian model input, mean (E,) and covariance (E, E) ->
        (M.t() (1, D), S (D, D), V.t() (E, D)) CPU float64 tensors -- the moment-matched mean state change, its covariance and
        Sigma^-1 Cov[x, delta].  Differentiable like the reference: when grad mode is on and input_mu or input_var requires
        grad, the outputs carry a grad_fn and backward() reaches the inputs (CPU or device) through gpmpc_moments_backward.
        input_var's gradient is the symmetric part of the reference's.  Hyper-parameters and the memory get no gradient, and
        double backward raises.  `propagation`: see predict_next_state_change_batch."""
        mu = _t(input_mu).reshape(1, -1)
        var = _t(input_var).reshape(1, mu.shape[1], mu.shape[1])
        out = self.predict_next_state_change_batch(mu, var, propagation=propagation)
        return out["M"].cpu(), out["S"][0].cpu(), out["V"][0].cpu()

    def predict_next_state_change_batch(self, input_mu, input_var=None, propagation=None):
        """predict_next_state_change at P independent inputs: input_mu (P, E), input_var (P, E, E) or None (deterministic
        inputs) -> dict of DEVICE tensors M (P, D), S (P, D, D), V (P, E, D).  Differentiable as predict_next_state_change is
        when grad mode is on and an input requires grad (input_var None: the mean's gradient only).
        `propagation` (None: ModelConfig.uncertainty_propagation): "linearized" returns the first-order propagation instead
        (gpmpc_moments_linear: M the posterior mean at input_mu, V its Jacobian, S = V^T input_var V + the posterior variance
        on the diagonal) -- no autograd (NotImplementedError when grad mode is on and an input requires grad)."""
        if self.x_mem is None:
            raise RuntimeError("call prepare_inference(inputs, state_changes) before predict_next_state_change")
        if self.propagation(propagation) == "linearized":
            _no_linearized_autograd("predict_next_state_change", input_mu, input_var)
            return self.engine.moments_linear(input_mu, input_var)
        grads = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (input_mu, input_var))
        if not grads:
            return self.engine.moments(input_mu, input_var)
        mu = _t(input_mu)
        var = _t(input_var) if input_var is not None else None
        M, S, V = _MomentsFunction.apply(self.engine, mu, var)
        return {"M": M, "S": S, "V": V}

    # -- state / training ------------------------------------------------------------------
    def save_state(self):
        return SavedState(inputs=self.x_mem, states_change=self.y_mem,
                          parameters=[m.state_dict() for m in self.models],
                          constraints_hyperparams={k: v for k, v in vars(self.config).items()
                                                   if k not in ("gp_init", "uncertainty_propagation", "num_inducing_points",
                                                                "inducing_jitter", "inducing_selection",
                                                                "inducing_refresh_every", "inducing_forget")})

    def load_state(self, saved_state):
        for m, p in zip(self.models, saved_state.parameters):
            m.initialize(**p)
        self.prepare_inference(_t(saved_state.inputs), _t(saved_state.states_change))

    @staticmethod
    def _device_search(engine, X, Y, lo, hi, start, incoming, restarts, iterations, history):
        """The "lbfgs_device" search of `train`: the list of parameter dicts from one train_search_host call."""
        n_gp, E = len(start), X.shape[1]
        n = E + 2
        K0, K1, K2 = GpHyperParameters.KEYS

        def rows(parts):
            return np.stack([np.concatenate([np.broadcast_to(np.asarray(p["ls"], dtype=np.float64).reshape(-1), (E,)),
                                             np.asarray(p["os"], dtype=np.float64).reshape(1),
                                             np.asarray(p["nz"], dtype=np.float64).reshape(1)]) for p in parts])
        lo_b, hi_b = rows(lo), rows(hi)
        theta_in = np.clip(rows(start), lo_b, hi_b)
        log_scale = bool(np.all(lo_b > 0.0))
        with np.errstate(divide="ignore", invalid="ignore"):
            x_in = np.log(theta_in / lo_b) / np.log(hi_b / lo_b) if log_scale else (theta_in - lo_b) / (hi_b - lo_b)
        x0 = np.empty((restarts, n_gp, n))
        x0[0] = np.clip(np.where(np.isfinite(x_in), x_in, 0.0), 0.0, 1.0)
        if restarts > 1:
            x0[1:] = torch.rand((restarts - 1, n_gp, n), dtype=F64).numpy()
        res = engine.train_search_host(torch.as_tensor(X, dtype=F64), torch.as_tensor(Y, dtype=F64), x0, lo_b, hi_b, iterations,
                                       history=history, log_scale=log_scale)
        out = []
        for a in range(n_gp):
            if int(res["restart"][a]) < 0:             # every start of this GP had a non-finite loss: the incoming parameters stay
                th = [incoming[a][K0], incoming[a][K1], incoming[a][K2]]
            else:
                th = [res["theta"][a, :E], res["theta"][a, E], res["theta"][a, E + 1]]
            out.append({K0: np.array(th[0], dtype=np.float64).reshape(1, E), K1: np.array(th[1], dtype=np.float64).reshape(()),
                        K2: np.array(th[2], dtype=np.float64).reshape(1)})
        return out

    @staticmethod
    def train(queue, saved_state, lr_train, num_iter_train, clip_grad_value, print_train=False, step_print_train=25,
              device="auto", loss_evaluator=None, optimizer="lbfgs", restarts=16, device_iterations=30, device_history=10):
        """Exact-MLL hyper-parameter search (reference :193-306): per GP a random restart inside the constraint box
        (drawn in the reference's order: outputscale, lengthscale, noise; GP after GP), LBFGS(strong_wolfe), keep the
        best, never return something worse than the incoming parameters.  Runs in the spawned training process, fp64.
        The loss and its gradient come from gpmpc_mll (K build + Cholesky + inverse + gradient contraction on the GPU)
        through an engine of this process's own; there is no CPU expression of the loss in this package.

        The D optimisations are independent, so they run as D threads advanced in LOCKSTEP: whenever every unfinished
        GP waits for a loss, ONE gpmpc_mll call evaluates all of them (the kernels batch over GPs; the reference runs
        them one after the other, :233-290).  Each GP sees the values its own sequential run would see.
        `loss_evaluator(X, y, ls, os, nz)` replaces the device loss in tests (the oracle's torch expression, as the
        checker of the driver logic); it is called per GP.

        optimizer="lbfgs_device" (TrainingConfig.optimizer) replaces that loop by ONE HipEngine.train_search_host call: `restarts`
        starts per GP advanced in lockstep on the GPU (gpmpc_train_search: `device_iterations` iterations of one trial point per
        start, `device_history` curvature pairs) over x in [0, 1]^(E + 2), mapped geometrically into the constraint box (linearly
        where a lower bound is not positive).  Start 0 of every GP is the incoming parameters, clipped into the box -- so the
        winner is never worse than them -- and starts 1 .. restarts - 1 are one torch.rand((restarts - 1, D, E + 2)) draw.  A GP
        whose every start has a non-finite loss keeps its incoming parameters.  The device search holds memories of up to 256
        points; a larger one takes the loop above on gpmpc_mll (a dispatch on size; with print_train it says so).

        Whatever happens in here, exactly ONE answer is put on the queue: the list of parameter dicts, or a
        `TrainingFailed` (a list holding the INCOMING parameters, with the reason attached) when the engine cannot be
        created, the device is not one this package computes on, or the search raised -- so the controller's
        check_and_close_processes never waits on a dead child and can tell a failed training from a finished one."""
        import threading
        t0 = time.time()
        incoming, out, engine, reason = None, None, None, "interrupted"
        try:
            incoming = [{k: np.asarray(v).copy() for k, v in p.items()} for p in saved_state.parameters]
            saved_state.to_tensors()
            X, Y = saved_state.inputs, saved_state.states_change
            cons = saved_state.constraints_hyperparams
            N, E = X.shape
            n_gp = len(saved_state.parameters)
            shared = None
            if optimizer not in ("lbfgs", "lbfgs_device"):
                raise ValueError(f"training optimizer {optimizer!r}: 'lbfgs' or 'lbfgs_device'")
            if optimizer == "lbfgs_device" and loss_evaluator is not None:
                raise ValueError("loss_evaluator replaces the device loss of the 'lbfgs' loop only")
            device_search = optimizer == "lbfgs_device" and N <= _DEVICE_SEARCH_MAX_N
            if optimizer == "lbfgs_device" and not device_search and print_train:
                print(f"training: {N} memory points > {_DEVICE_SEARCH_MAX_N}: the host L-BFGS loop on gpmpc_mll instead of the device search")
            if loss_evaluator is None:
                if device not in ("auto", "hip"):
                    raise ValueError(f"training device {device!r}: the loss runs on the GPU only ('auto' or 'hip')")
                from ...engine import HipEngine       # raises without a GPU / without the HIP library
                engine = HipEngine(0)
            if loss_evaluator is None and not device_search:
                shared = _LockstepMll(engine, torch.as_tensor(X, dtype=F64).to(engine.device).contiguous(),
                                      torch.as_tensor(Y, dtype=F64).to(engine.device).contiguous(), n_gp)
            K0, K1, K2 = GpHyperParameters.KEYS
            lo = [{"ls": _t(cons["min_lengthscale"])[a], "os": _t(cons["min_outputscale"])[a],
                   "nz": _t(cons["min_std_noise"])[a] ** 2} for a in range(n_gp)]
            hi = [{"ls": _t(cons["max_lengthscale"])[a], "os": _t(cons["max_outputscale"])[a],
                   "nz": _t(cons["max_std_noise"])[a] ** 2} for a in range(n_gp)]
            start = [{"ls": p[K0].reshape(-1), "os": p[K1].reshape(()), "nz": p[K2].reshape(())}
                     for p in saved_state.parameters]
            # the restarts, drawn up front in the order the reference's sequential loop consumes the generator (:236-252)
            raws = []
            for a in range(0 if device_search else n_gp):          # (the device search draws its own starts, below)
                raws.append({k: torch.logit(torch.rand(start[a][k].shape, dtype=F64).clamp(1e-6, 1 - 1e-6)).requires_grad_(True)
                             for k in ("os", "ls", "nz")})
            results = [None] * n_gp
            if device_search:
                results = GpStateTransitionModel._device_search(engine, X, Y, lo, hi, start, incoming, restarts, device_iterations,
                                                                device_history)

            def search(a):
                y = Y[:, a]

                def neg_mll(ls, osc, nz):
                    if shared is not None:
                        return _DeviceNegMll.apply(ls, osc, nz, shared, a)
                    return loss_evaluator(X, y, ls, osc, nz)

                best = dict(start[a])
                try:
                    best_loss = float(neg_mll(best["ls"], best["os"], best["nz"]))
                except Exception:
                    best_loss = float("inf")
                raw = raws[a]

                def val(k):
                    return lo[a][k] + (hi[a][k] - lo[a][k]) * torch.sigmoid(raw[k])
                opt = torch.optim.LBFGS([raw["ls"], raw["os"], raw["nz"]], lr=lr_train, line_search_fn="strong_wolfe")
                try:
                    for i in range(num_iter_train):
                        def closure():
                            opt.zero_grad()
                            loss = neg_mll(val("ls"), val("os"), val("nz"))
                            loss.backward()
                            return loss
                        loss = float(opt.step(closure).detach())
                        if print_train and i % step_print_train == 0:
                            print(f"train gp {a} iter {i + 1}/{num_iter_train} loss {loss:.5f}")
                        if loss < best_loss:
                            best_loss = loss
                            best = {k: val(k).detach().clone() for k in raw}
                except Exception as e:         # keep the best found so far, like the reference (:289-290)
                    print(e)
                return {K0: best["ls"].reshape(1, E).numpy(), K1: best["os"].reshape(()).numpy(),
                        K2: best["nz"].reshape(1).numpy()}

            def worker(a):
                try:
                    results[a] = search(a)
                except BaseException as e:
                    results[a] = e
                finally:
                    if shared is not None:
                        shared.finished(a)

            if device_search:
                pass
            elif shared is not None and n_gp > 1:
                threads = [threading.Thread(target=worker, args=(a,), daemon=True) for a in range(n_gp)]
                for th in threads:
                    th.start()
                for th in threads:
                    th.join()
            else:
                for a in range(n_gp):
                    worker(a)
            for r in results:
                if isinstance(r, BaseException):
                    raise r
            out = results
            if shared is not None:
                GpStateTransitionModel.last_training_launches = shared.launches
            if print_train:
                print(f"training process: {time.time() - t0:.2f} s")
        except Exception as e:
            reason = repr(e)
            print(f"training process failed ({reason}): keeping the incoming hyper-parameters")
            out = None
        finally:
            if engine is not None:
                engine.close()
            if out is not None and incoming is not None and len(out) == len(incoming):
                queue.put(out)
            else:
                keep = incoming if incoming is not None else [dict(p) for p in getattr(saved_state, "parameters", [])]
                queue.put(TrainingFailed(keep, reason))
