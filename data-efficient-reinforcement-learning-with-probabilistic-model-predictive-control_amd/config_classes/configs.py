"""Plain-Python configuration objects with the reference's class names, constructor keywords
and attribute names (rl_gp_mpc/config_classes/*.py), so the reference's example config files
(examples/*/config_*.py) build the same objects against this package.

Differences, on purpose: tensors are created with an explicit dtype=float64 instead of flipping
torch's global default dtype at import time (reference: total_config.py:11), and mutable default
arguments are copied.
"""
import copy

import torch

F64 = torch.float64


def _t(v):
    return torch.as_tensor(v, dtype=F64) if isinstance(v, (list, tuple)) else v


def _tensorise_lists(obj):
    for k, v in list(vars(obj).items()):
        if isinstance(v, (list, tuple)):
            setattr(obj, k, torch.as_tensor(v, dtype=F64))


class ObservationConfig:
    def __init__(self, obs_var_norm=(1e-6, 1e-6, 1e-6)):
        # diagonal covariance of the normalised observation (reference observation_config.py:11)
        self.obs_var_norm = torch.diag(torch.as_tensor(list(obs_var_norm), dtype=F64))


class RewardConfig:
    def __init__(self, target_state_norm=(1, 0.5, 0.5), weight_state=(1, 0.1, 0.1), weight_state_terminal=(10, 5, 5),
                 target_action_norm=(0.5,), weight_action=(0.05,), exploration_factor=3, use_constraints=False,
                 state_min=(-0.1, 0.05, 0.05), state_max=(1.1, 0.95, 0.925), area_multiplier=1,
                 clip_lower_bound_cost_to_0=False):
        self.target_state_norm = list(target_state_norm)
        self.weight_state = list(weight_state)
        self.weight_state_terminal = list(weight_state_terminal)
        self.target_action_norm = list(target_action_norm)
        self.weight_action = list(weight_action)
        self.exploration_factor = exploration_factor
        self.use_constraints = use_constraints
        self.state_min = list(state_min)
        self.state_max = list(state_max)
        self.area_multiplier = area_multiplier
        self.clip_lower_bound_cost_to_0 = clip_lower_bound_cost_to_0
        _tensorise_lists(self)
        # derived (reference reward_config.py:54-64)
        self.weight_matrix_cost = torch.block_diag(torch.diag(self.weight_state), torch.diag(self.weight_action))
        self.weight_matrix_cost_terminal = torch.diag(self.weight_state_terminal)
        self.target_state_action_norm = torch.cat((self.target_state_norm, self.target_action_norm))


class ActionsConfig:
    def __init__(self, limit_action_change=False, max_change_action_norm=(0.05,)):
        self.limit_action_change = limit_action_change
        self.max_change_action_norm = list(max_change_action_norm)
        _tensorise_lists(self)


class MemoryConfig:
    def __init__(self, check_errors_for_storage=True, min_error_prediction_state_for_memory=(3e-4, 3e-4, 3e-4),
                 min_prediction_state_std_for_memory=(3e-3, 3e-3, 3e-3), points_batch_memory=1500, max_points_model=None):
        self.check_errors_for_storage = check_errors_for_storage
        self.min_error_prediction_state_for_memory = list(min_error_prediction_state_for_memory)
        self.min_prediction_state_std_for_memory = list(min_prediction_state_std_for_memory)
        self.points_batch_memory = points_batch_memory
        # cap of the GP memory (None: it only grows, as in the reference): beyond it Memory.prepare_for_model evicts the oldest
        # model points -- a sliding window, the natural memory of time-varying dynamics modelled with a time input
        if max_points_model is not None and int(max_points_model) < 1:
            raise ValueError(f"MemoryConfig.max_points_model={max_points_model!r}: None or a positive number of points")
        self.max_points_model = None if max_points_model is None else int(max_points_model)
        _tensorise_lists(self)


class TrainingConfig:
    def __init__(self, lr_train=7e-3, iter_train=15, training_frequency=25, clip_grad_value=1e-3, print_train=False,
                 step_print_train=5, device="auto", optimizer="lbfgs", restarts=16, device_iterations=30, device_history=10):
        self.lr_train = lr_train
        self.iter_train = iter_train
        self.training_frequency = training_frequency
        self.clip_grad_value = clip_grad_value
        self.print_train = print_train
        self.step_print_train = step_print_train
        # where the training loss is evaluated: "auto" / "hip" = gpmpc_mll on the GPU of the training process.  There is no
        # CPU expression of the loss in this package (the reference's runs in gpytorch): anything else is refused HERE, in
        # the parent, instead of failing inside the spawned child
        if device not in ("auto", "hip"):
            raise ValueError(f"TrainingConfig.device={device!r}: the training loss runs on the GPU only ('auto' or 'hip')")
        self.device = device
        # how the hyper-parameters are searched: "lbfgs" = the reference's loop (one random restart per GP, torch LBFGS on the
        # host, every loss a gpmpc_mll call); "lbfgs_device" = `restarts` starts per GP in lockstep on the GPU
        # (gpmpc_train_search: `device_iterations` iterations of one trial point each, `device_history` curvature pairs), for
        # memories of up to 256 points -- larger ones take the "lbfgs" loop
        if optimizer not in ("lbfgs", "lbfgs_device"):
            raise ValueError(f"TrainingConfig.optimizer={optimizer!r}: 'lbfgs' or 'lbfgs_device'")
        for name, value, top in (("restarts", restarts, 4096), ("device_iterations", device_iterations, None),
                                 ("device_history", device_history, 32)):
            if isinstance(value, bool) or not isinstance(value, int) or value < 1 or (top is not None and value > top):
                raise ValueError(f"TrainingConfig.{name}={value!r}: an integer >= 1" + (f" and <= {top}" if top else ""))
        self.optimizer = optimizer
        self.restarts = restarts
        self.device_iterations = device_iterations
        self.device_history = device_history


_DEFAULT_OPTIMIZER = {"disp": None, "maxcor": 30, "ftol": 1e-99, "gtol": 1e-99, "eps": 1e-2, "maxfun": 30,
                      "maxiter": 30, "iprint": -1, "maxls": 30, "finite_diff_rel_step": None}


class ControllerConfig:
    """Reference keywords (controller_config.py:1-25) plus optional ones for the batched optimisers that replace
    the sequential scipy restarts: `candidate_optimizer="cem"` (cross-entropy search, one
    rollout launch per iteration) or `"lbfgs"` (the reference's scipy L-BFGS-B restarts advanced in lockstep: one
    objective + analytic-gradient launch serves every restart's pending evaluation; same result as the sequential
    loop, wall time of the longest restart) or `"lbfgs_device"` (a box-constrained L-BFGS whose whole loop stays on the
    GPU, gpmpc_lbfgs_search: `lbfgs_candidates` starts in lockstep, one objective + gradient launch and one trial point per
    restart and iteration, `lbfgs_device_iterations` of them with `lbfgs_device_history` curvature pairs; also the one
    gradient search of the linearised propagation) or `"ilqr_device"` (a clamped iLQR on the mean dynamics of the linearised
    propagation whose whole loop stays on the GPU, gpmpc_ilqr_search: `ilqr_candidates` starts in lockstep, `ilqr_iterations`
    iterations of a backward Riccati sweep and a line search over `ilqr_line_search_steps` step sizes, regularisation
    `ilqr_reg`; certainty-equivalent design, the winner chosen by the LCB objective; linearised propagation, open loop and the
    normalisation mapper only)."""

    def __init__(self, len_horizon=15, actions_optimizer_params=None, init_from_previous_actions=True,
                 restarts_optim=1, optimize=True, num_repeat_actions=1,
                 candidate_optimizer=None, cem_candidates=256, cem_iterations=4, cem_elite_fraction=0.1,
                 lbfgs_candidates=None, shard_over_ranks=False, feedback_gain=None, feedback_lqr_reg=0.0,
                 lbfgs_device_iterations=30, lbfgs_device_history=10,
                 ilqr_candidates=None, ilqr_iterations=8, ilqr_reg=1e-3, ilqr_line_search_steps=8):
        self.len_horizon = len_horizon
        self.actions_optimizer_params = dict(_DEFAULT_OPTIMIZER if actions_optimizer_params is None
                                             else actions_optimizer_params)
        self.init_from_previous_actions = init_from_previous_actions
        self.restarts_optim = restarts_optim      # with optimize=False: number of random candidates (one GPU launch)
        self.optimize = optimize
        self.num_repeat_actions = num_repeat_actions
        self.candidate_optimizer = candidate_optimizer      # None: scipy L-BFGS-B (reference behaviour); "cem"
        self.cem_candidates = cem_candidates                # candidates per iteration = one kernel launch
        self.cem_iterations = cem_iterations
        self.cem_elite_fraction = cem_elite_fraction
        self.lbfgs_candidates = lbfgs_candidates            # None: restarts_optim starting points
        # "lbfgs_device": evaluations per restart (mirrors maxfun = 30 of the scipy solver) and pairs of the L-BFGS memory
        self.lbfgs_device_iterations = lbfgs_device_iterations
        self.lbfgs_device_history = lbfgs_device_history
        # "ilqr_device": starts (None: restarts_optim), iterations, the initial (and smallest) regularisation of Huu and the step
        # sizes 1, 1/2, ... of the line search
        self.ilqr_candidates = ilqr_candidates
        self.ilqr_iterations = ilqr_iterations
        self.ilqr_reg = ilqr_reg
        self.ilqr_line_search_steps = ilqr_line_search_steps
        # one process per GPU (torch.distributed initialised by the launcher): split the candidates / restarts over the ranks.
        # Opt-in: every rank must then call get_action with the same observation (checked inside the exchange)
        self.shard_over_ranks = shard_over_ranks
        # ancillary feedback u = ubar_t + K (x - mu_t) the candidates are planned under (closed-loop covariance and costs,
        # gpmpc_rollout_linear_feedback): an (A, D) or (H, A, D) array in model space, or None (open loop).  Needs
        # ModelConfig.uncertainty_propagation = "linearized".  "lqr": every candidate's own LQR gains, designed on the device along
        # its nominal trajectory on the reward's quadratic cost (gpmpc_lqr_gains), feedback_lqr_reg >= 0 added to the diagonal of
        # Huu (certainty-equivalent; the action box is not modelled)
        self.feedback_gain = feedback_gain
        self.feedback_lqr_reg = feedback_lqr_reg


def _broadcast(v, shape):
    """Scalar / per-model vector -> tensor of `shape` (reference functions_process_config.py:29-36)."""
    t = v if isinstance(v, torch.Tensor) else torch.as_tensor(v, dtype=F64)
    t = t.to(F64)
    if t.ndim < len(shape):
        t = t.unsqueeze(-1)
    return t * torch.ones(shape, dtype=F64)


def _with_time_column(ls, ls_time, num_models, num_inputs):
    """Lengthscale table whose last column is the time lengthscale (functions_process_config.py:18-26)."""
    out = torch.empty((num_models, num_inputs), dtype=F64)
    t = ls if isinstance(ls, torch.Tensor) else torch.as_tensor(ls, dtype=F64)
    if t.ndim == 1:
        out[:, :-1] = t[:, None].expand(num_models, num_inputs - 1)
    else:
        out[:, :-1] = t
    out[:, -1] = ls_time
    return out


UNCERTAINTY_PROPAGATIONS = ("moment_matching", "linearized")
INDUCING_SELECTIONS = ("strided", "greedy")


class ModelConfig:
    def __init__(self, gp_init=None, init_lengthscale_time=100, min_std_noise=1e-3, max_std_noise=3e-1,
                 min_outputscale=1e-5, max_outputscale=0.95, min_lengthscale=4e-3, max_lengthscale=25.0,
                 min_lengthscale_time=10, max_lengthscale_time=10000, include_time_model=False,
                 uncertainty_propagation="moment_matching", num_inducing_points=None, inducing_jitter=1e-6,
                 inducing_selection="strided", inducing_refresh_every=None, inducing_forget=False):
        """num_inducing_points: None (the exact GP on the whole memory), or M >= 1 -- once the memory holds more than M points
        the model predicts with a sparse GP (DTC / projected process, gpmpc_prepare_sparse) on M inducing inputs, the rows
        round(i (N - 1) / (M - 1)), i = 0..M-1, of the N-point memory (M = 1: row 0): every prediction, rollout and gradient
        then costs what an M-point memory costs while all N points shape the model.  Training stays the exact marginal
        likelihood on the whole memory.  inducing_jitter: times the outputscale, added to the diagonal of k(Z, Z).
        inducing_selection: which M memory points those are -- "strided" (the rows above: they ignore the data and the kernel)
        or "greedy" (gpmpc_select_inducing, chosen afresh on the device at every prepare_inference: each pick is the point
        the inducing set so far explains worst under the current hyper-parameters, so a memory clustered round the setpoint
        keeps its few exploratory points).
        inducing_refresh_every: None (every prepare_inference rebuilds the sparse model: select or stride, then
        gpmpc_prepare_sparse), or R >= 1 -- a prepare_inference whose memory is the previous one followed by k new rows, under
        unchanged hyper-parameters, appends them to the cached sparse model in O(k M^2) (gpmpc_sparse_append: same inducing
        inputs) as long as no more than R rows have been appended since the last rebuild; the rebuild then chooses the
        inducing inputs afresh.  Rounding does not limit R; the age of the inducing inputs does.
        inducing_forget: False (`forget` is refused on a sparse model, and the evictions of a capped memory rebuild it every
        step), or True -- together with inducing_refresh_every = R, `forget` removes the rows from the cached sparse model in
        O(k M^2) (gpmpc_sparse_forget: same inducing inputs, the rows' values leave by the append's recurrence with the
        opposite sign), so a sliding-window step (MemoryConfig.max_points_model) is forget + append in place of a rebuild from
        all N points.  Removed rows count toward R together with appended ones: R is then "rows changed since the last
        rebuild".  Here rounding does limit R: a removal subtracts, and loses digits when most of the data behind an
        inducing input has left.
        uncertainty_propagation: how an uncertain state goes through the GP -- "moment_matching" (the reference's exact
        moment matching, gp_model.py:112-180) or "linearized" (first-order Taylor propagation at the input mean,
        gpmpc_moments_linear / gpmpc_rollout_linear: no D^2 pair pass, but a different approximation)."""
        if uncertainty_propagation not in UNCERTAINTY_PROPAGATIONS:
            raise ValueError(f"uncertainty_propagation must be one of {UNCERTAINTY_PROPAGATIONS}, got {uncertainty_propagation!r}")
        self.uncertainty_propagation = uncertainty_propagation
        if num_inducing_points is not None and (isinstance(num_inducing_points, bool) or int(num_inducing_points) != num_inducing_points
                                                or int(num_inducing_points) < 1):
            raise ValueError(f"ModelConfig.num_inducing_points={num_inducing_points!r}: None or a positive number of points")
        self.num_inducing_points = None if num_inducing_points is None else int(num_inducing_points)
        if not (float(inducing_jitter) >= 0.0 and float(inducing_jitter) < float("inf")):
            raise ValueError(f"ModelConfig.inducing_jitter={inducing_jitter!r}: a finite number >= 0")
        self.inducing_jitter = float(inducing_jitter)
        if inducing_selection not in INDUCING_SELECTIONS:
            raise ValueError(f"ModelConfig.inducing_selection must be one of {INDUCING_SELECTIONS}, got {inducing_selection!r}")
        self.inducing_selection = inducing_selection
        if inducing_refresh_every is not None and (isinstance(inducing_refresh_every, bool)
                                                   or int(inducing_refresh_every) != inducing_refresh_every
                                                   or int(inducing_refresh_every) < 1):
            raise ValueError(f"ModelConfig.inducing_refresh_every={inducing_refresh_every!r}: None or a positive number of rows")
        self.inducing_refresh_every = None if inducing_refresh_every is None else int(inducing_refresh_every)
        if not isinstance(inducing_forget, bool):
            raise ValueError(f"ModelConfig.inducing_forget={inducing_forget!r}: True or False")
        self.inducing_forget = inducing_forget
        if gp_init is None:
            gp_init = {"noise_covar.noise": [1e-4] * 3, "base_kernel.lengthscale": [[0.75] * 4] * 3,
                       "outputscale": [5e-2] * 3}
        self.include_time_model = include_time_model
        self.min_std_noise = min_std_noise
        self.max_std_noise = max_std_noise
        self.min_outputscale = min_outputscale
        self.max_outputscale = max_outputscale
        self.min_lengthscale = min_lengthscale
        self.max_lengthscale = max_lengthscale
        self.min_lengthscale_time = min_lengthscale_time
        self.max_lengthscale_time = max_lengthscale_time
        self.init_lengthscale_time = init_lengthscale_time
        self.gp_init = {k: _t(copy.deepcopy(v)) for k, v in gp_init.items()}

    def extend_dimensions_params(self, dim_state, dim_input):
        """Per-GP broadcasting of scalar settings (reference model_config.py:46-67)."""
        for name in ("min_std_noise", "max_std_noise", "min_outputscale", "max_outputscale"):
            setattr(self, name, _broadcast(getattr(self, name), (dim_state,)))
        self.gp_init["noise_covar.noise"] = _broadcast(self.gp_init["noise_covar.noise"], (dim_state,))
        self.gp_init["outputscale"] = _broadcast(self.gp_init["outputscale"], (dim_state,))
        if self.include_time_model:
            self.min_lengthscale = _with_time_column(self.min_lengthscale, self.min_lengthscale_time, dim_state, dim_input)
            self.max_lengthscale = _with_time_column(self.max_lengthscale, self.max_lengthscale_time, dim_state, dim_input)
            self.gp_init["base_kernel.lengthscale"] = _with_time_column(
                self.gp_init["base_kernel.lengthscale"], self.init_lengthscale_time, dim_state, dim_input)
        else:
            self.min_lengthscale = _broadcast(self.min_lengthscale, (dim_state, dim_input))
            self.max_lengthscale = _broadcast(self.max_lengthscale, (dim_state, dim_input))
            self.gp_init["base_kernel.lengthscale"] = _broadcast(self.gp_init["base_kernel.lengthscale"],
                                                                 (dim_state, dim_input))


class VisuConfig:
    """Accepted for call compatibility (reference visu_config.py); visualisation is out of scope."""

    def __init__(self, save_render_env=True, render_live_plot_2d=True, render_env=True, save_live_plot_2d=False):
        self.save_render_env = save_render_env
        self.render_live_plot_2d = render_live_plot_2d
        self.render_env = render_env
        self.save_live_plot_2d = save_live_plot_2d


class Config:
    def __init__(self, observation_config=None, reward_config=None, actions_config=None, model_config=None,
                 memory_config=None, training_config=None, controller_config=None):
        self.observation = observation_config or ObservationConfig()
        self.reward = reward_config or RewardConfig()
        self.actions = actions_config or ActionsConfig()
        self.model = model_config or ModelConfig()
        self.memory = memory_config or MemoryConfig()
        self.training = training_config or TrainingConfig()
        self.controller = controller_config or ControllerConfig()
