"""GpMpcController -- drop-in for rl_gp_mpc/control_objects/controllers/gp_mpc_controller.py.

Same constructor and method set as the reference (what run_env_function.py:18-47 calls):
get_action, get_iter_info, compute_cost_unnormalized, add_memory, check_and_close_processes,
compute_mean_lcb_trajectory; `compute_action` is an alias of get_action.

What changes is WHERE the work happens.  The reference evaluates one action sequence per Python
call (:229-285) inside a sequential restart loop (:125-148).  Here every evaluation is a batch in
ONE launch of the HIP rollout kernel:

  * optimize=False (random shooting, :142-144): all `restarts_optim` candidates at once, argmin on
    the device, candidates optionally sharded across GPUs (sharding.py);
  * optimize=True (scipy L-BFGS-B with jac=True, :132-141): value + ANALYTIC gradient per evaluation
    (gpmpc_rollout_grad: forward rollout + pairwise moment pass + reverse sweep, what the reference gets
    from `mean_cost.backward()`, :277).  Shapes outside the gradient kernels (GPMPC_ERR_LIMIT) fall
    back to a 4th-order central difference over the H*A model actions, 4*H*A + 1 candidates in one
    launch -- in `compute_mean_lcb_trajectory` and in the batched `objective_and_gradient_batch` alike.
    The reference's two pass-through clamps (action clamp of DerivativeActionMapper, optional clip of
    the UCB at 0) have identity backward; the finite difference is taken where those clamps are
    transparent so the returned gradient has the same meaning.

The candidate searches are functions of candidate_search.py, looked up in its table; this class keeps the skeleton around them
(`_get_optimal_actions`, `_adopt`) and the objective they evaluate.
"""
import multiprocessing

import numpy as np
import torch

from ..actions_mappers.action_init_functions import generate_mpc_action_init_random
from ..actions_mappers.mappers import DerivativeActionMapper, NormalizationActionMapper
from ..memories.gp_memory import Memory
from ..models.gp_model import GpStateTransitionModel, TrainingFailed
from ..observations_states_mappers.normalization_observation_state_mapper import NormalizationObservationStateMapper
from ..states_reward_mappers.setpoint_distance_reward_mapper import SetpointStateRewardMapper
from . import candidate_search
from .abstract_controller import BaseControllerObject
from .iteration_info_class import IterationInformation
from ..._lib import GPMPC_ERR_ARG, GPMPC_ERR_LIMIT, GpmpcError

F64 = torch.float64
FD_STEP = 1e-3           # 4th-order stencil: truncation ~ h^4, rounding ~ 1e-13 / h


class GpMpcController(BaseControllerObject):
    def __init__(self, observation_low, observation_high, action_low, action_high, config, engine=None, device=None):
        self.config = config
        self.observation_state_mapper = NormalizationObservationStateMapper(
            config=config.observation, observation_low=observation_low, observation_high=observation_high)
        Mapper = DerivativeActionMapper if config.actions.limit_action_change else NormalizationActionMapper
        self.actions_mapper = Mapper(config=config.actions, action_low=action_low, action_high=action_high,
                                     len_horizon=config.controller.len_horizon)
        self.transition_model = GpStateTransitionModel(config=config.model,
                                                       dim_state=self.observation_state_mapper.dim_observation,
                                                       dim_action=self.actions_mapper.dim_action,
                                                       engine=engine, device=device)
        self.state_reward_mapper = SetpointStateRewardMapper(config=config.reward)
        self.memory = Memory(config.memory, dim_input=self.transition_model.dim_input,
                             dim_state=self.transition_model.dim_state,
                             include_time_model=self.transition_model.config.include_time_model,
                             step_model=config.controller.num_repeat_actions)
        self.actions_mpc_previous_iter = None
        self.iter_ctrl = 0
        self.num_cores_main = multiprocessing.cpu_count()
        self.ctx = multiprocessing.get_context("spawn")
        self.queue_train = self.ctx.Queue()
        self.info_iters = {}
        self.num_rollouts = 0          # candidate trajectories evaluated so far (throughput accounting)
        self.analytic_gradient = True  # gradient kernels (gpmpc_rollout_grad); False: 4th-order differences of the rollout
        self.process_group = None      # torch.distributed group the candidates shard over (None: the default group)
        self._check_propagation_supported()

    LINEARIZED_OPTIMIZERS = candidate_search.linearized_optimizers()

    def _check_propagation_supported(self, what=None):
        """Refuse what the configured search does not support (the table of candidate_search.py): its
        uncertainty propagation, closed-loop planning under ControllerConfig.feedback_gain (which exists for the linearised
        propagation only), the DerivativeActionMapper.  `what` names a gradient-path entry point that asks for itself: the
        linearised propagation has objective values only, so it refuses them all."""
        key, search = candidate_search.lookup(self.config.controller)
        linearized = self.transition_model.propagation() == "linearized"
        closed_loop = getattr(self.config.controller, "feedback_gain", None) is not None

        def refuse(reason):                          # in the search's own words (no string is built on the way through)
            raise ValueError(f"{candidate_search.name_of(key)} {reason}")
        if "moment_matching" not in search.propagations:     # a search of the linearised propagation alone says what it needs first
            if not linearized:
                refuse("needs ModelConfig.uncertainty_propagation='linearized': " + search.why_not["propagation"])
            if closed_loop and not search.feedback:
                refuse(search.why_not["feedback"] + ": it does not support ControllerConfig.feedback_gain")
            if not search.derivative and isinstance(self.actions_mapper, DerivativeActionMapper):
                refuse(search.why_not["derivative"])
            if what is None:
                return
        if not linearized:
            if closed_loop:
                raise ValueError("ControllerConfig.feedback_gain needs ModelConfig.uncertainty_propagation='linearized': "
                                 "moment matching has no closed-loop rollout")
            return
        if what is None:
            if "linearized" in search.propagations:
                if closed_loop and not search.feedback:
                    refuse(search.why_not["feedback"] + ": it does not support ControllerConfig.feedback_gain")
                return
            what = f"{candidate_search.name_of(key)} with optimize=True"
        raise ValueError(f"uncertainty_propagation='linearized' does not support {what}: it has no gradient or device-search "
                         f"kernels; supported optimisers: {self.LINEARIZED_OPTIMIZERS}")

    def _ranks(self):
        """(world, rank) of the candidate sharding.  Sharding is OPT-IN (`ControllerConfig.shard_over_ranks`): a process that
        initialised torch.distributed for some other purpose must not have its candidates silently split over ranks that may
        sit at different states.  With the flag set and a process group initialised, every rank must call get_action with the
        SAME observation and the same numpy seed -- both are verified inside the exchanges (a mismatch raises on every rank)."""
        dist = torch.distributed
        if not getattr(self.config.controller, "shard_over_ranks", False) or not (dist.is_available() and dist.is_initialized()):
            return 1, 0
        return dist.get_world_size(self.process_group), dist.get_rank(self.process_group)

    # ------------------------------------------------------------------------------ public
    def get_action(self, obs_mu, obs_var=None, random=False):
        """Reference :52-112.  Returns the raw (denormalised) action for the environment, shape (A,)."""
        self.check_and_close_processes()
        cc = self.config.controller
        if self.iter_ctrl % cc.num_repeat_actions == 0:
            self.memory.prepare_for_model()
            state_mu, state_var = self.observation_state_mapper.get_state(obs=obs_mu, obs_var=obs_var, update_internals=True)
            actions_model = self._get_random_actions(state_mu, state_var) if random \
                else self._get_optimal_actions(state_mu, state_var)
            actions_raw = self.actions_mapper.transform_action_model_to_action_raw(actions_model, update_internals=True)
            next_action_raw = actions_raw[0]
            reward, reward_var = self.state_reward_mapper.get_reward(state_mu, state_var, actions_model[0])
            std_pred = torch.diagonal(self.states_var_pred, dim1=-2, dim2=-1).sqrt()
            idx_pred = np.arange(self.iter_ctrl, self.iter_ctrl + cc.len_horizon * cc.num_repeat_actions,
                                 cc.num_repeat_actions)
            self.iter_info = IterationInformation(
                iteration=self.iter_ctrl, state=self.states_mu_pred[0], cost=-reward.item(),
                cost_std=reward_var.sqrt().item(),
                mean_predicted_cost=np.min([-self.rewards_trajectory.mean().item(), 3]),
                mean_predicted_cost_std=self.rewards_traj_var.sqrt().mean().item(),
                lower_bound_mean_predicted_cost=self.cost_traj_mean_lcb.item(),
                predicted_idxs=idx_pred, predicted_states=self.states_mu_pred, predicted_states_std=std_pred,
                predicted_actions=actions_model, predicted_costs=-self.rewards_trajectory,
                predicted_costs_std=self.rewards_traj_var.sqrt())
            self.store_iter_info(self.iter_info)
            self.past_action = next_action_raw
        else:
            next_action_raw = self.past_action
        self.iter_ctrl += 1
        return next_action_raw.detach().cpu().numpy().copy() if isinstance(next_action_raw, torch.Tensor) \
            else np.array(next_action_raw)

    compute_action = get_action      # the name BASELINE.json's north_star uses

    def evaluate_candidates(self, actions_mpc_batch, obs_mu, obs_var, trajectories=False):
        """Objective of B optimiser vectors (B, H*A) in one launch -> dict of device tensors + 'actions_model'."""
        acts = self.actions_mapper.mpc_to_model_batch(np.asarray(actions_mpc_batch, dtype=np.float64))
        self.transition_model.set_cost(self.config.reward)
        gain = getattr(self.config.controller, "feedback_gain", None)
        if gain is not None:
            self._check_propagation_supported()
        if gain is None:
            kw = {}                                                                              # open loop: the call as ever
        elif isinstance(gain, str):                                                              # "lqr": designed per candidate
            kw = {"feedback_gains": gain, "lqr_reg": float(getattr(self.config.controller, "feedback_lqr_reg", 0.0))}
        else:
            kw = {"feedback_gains": self._feedback_gain_on_device(gain)}
        out = self.transition_model.predict_trajectory_batch(
            acts, obs_mu, obs_var, self.config.controller.len_horizon, self.iter_ctrl,
            trajectories=trajectories, stage_costs=True, **kw)
        self.num_rollouts += acts.shape[0]
        out["actions_model"] = acts
        return out

    def _feedback_gain_on_device(self, gain):
        """ControllerConfig.feedback_gain as a tensor on the engine's device, uploaded once: compared by CONTENT with what was
        uploaded last, as set_cost does, so that in-place edits of the config take effect."""
        host = np.ascontiguousarray(np.asarray(gain, dtype=np.float64))
        key = (host.shape, host.tobytes())
        if getattr(self, "_gain_key", None) != key:
            self._gain_dev = torch.as_tensor(host).to(self.transition_model.engine.device)
            self._gain_key = key
        return self._gain_dev

    def compute_mean_lcb_trajectory(self, actions_mpc, obs_mu, obs_var):
        """Reference :229-285: (mean-LCB cost, d cost / d actions_mpc) for ONE optimiser vector; also caches
        the predicted trajectory and its costs on `self` for IterationInformation (:279-283)."""
        self._check_propagation_supported("compute_mean_lcb_trajectory (the gradient path)")
        H, A = self.config.controller.len_horizon, self.actions_mapper.dim_action
        base = self.actions_mapper.mpc_to_model_batch(np.asarray(actions_mpc, dtype=np.float64).reshape(1, -1))[0]
        n = H * A
        self.transition_model.set_cost(self.config.reward)
        if self.analytic_gradient:
            try:
                host = self.transition_model.objective_and_gradient_host(base, obs_mu, obs_var, self.iter_ctrl)
            except GpmpcError as e:
                if e.code != GPMPC_ERR_LIMIT:
                    raise
                self.analytic_gradient = False         # shape outside the gradient kernels: difference the rollout
            else:
                self.num_rollouts += 1
                grad = self.actions_mapper.chain_grad_model_to_mpc(host["grad"][0])
                self._lazy_host = host                          # the caches of :279-283, made on first read
                return float(host["J"][0]), grad
        J, g_model, out = self._objective_and_gradient_by_differences(base[None], obs_mu, obs_var, trajectories=True)
        grad = self.actions_mapper.chain_grad_model_to_mpc(g_model[0])
        self._cache_trajectory(out, 0)
        return float(J[0]), grad

    def _objective_and_gradient_by_differences(self, bases, obs_mu, obs_var, trajectories=False):
        """Fallback for shapes outside the gradient kernels (GPMPC_ERR_LIMIT): J and dJ/d(model actions) of `bases`
        (C, H, A) from a 4th-order central difference of the rollout, all C * (4*H*A + 1) candidates in ONE launch
        ([base, +h, -h, +2h, -2h] per coordinate; the base candidates come first, so out[...][c] is candidate c)."""
        C, H, A = bases.shape
        n = H * A
        cand = np.empty((C, 4 * n + 1, n))
        cand[:] = bases.reshape(C, 1, n)
        k = np.arange(n)
        cand[:, 1 + k, k] += FD_STEP
        cand[:, 1 + n + k, k] -= FD_STEP
        cand[:, 1 + 2 * n + k, k] += 2 * FD_STEP
        cand[:, 1 + 3 * n + k, k] -= 2 * FD_STEP
        order = np.concatenate([np.arange(C) * (4 * n + 1)] + [c * (4 * n + 1) + 1 + np.arange(4 * n) for c in range(C)])
        flat = cand.reshape(C * (4 * n + 1), H, A)[order]
        self.transition_model.set_cost(self.config.reward)
        out = self.transition_model.predict_trajectory_batch(flat, obs_mu, obs_var, H, self.iter_ctrl,
                                                             trajectories=trajectories, stage_costs=True)
        self.num_rollouts += flat.shape[0]
        cm = out["cost_mu"].cpu().numpy()
        cv = out["cost_var"].cpu().numpy()
        J_clip = out["J"].cpu().numpy()[:C]
        J_free = np.mean(cm - self.config.reward.exploration_factor * np.sqrt(cv), axis=1)   # clamp transparent
        Jd = J_free[C:].reshape(C, 4, n)
        g_model = (8.0 * (Jd[:, 0] - Jd[:, 1]) - (Jd[:, 2] - Jd[:, 3])) / (12.0 * FD_STEP)
        return J_clip, g_model.reshape(C, H, A), out

    def compute_cost_unnormalized(self, obs, action, obs_var=None):
        """Reference :287-305: cost of an un-normalised (obs, action) pair -> (mean, variance)."""
        state_mu, state_var = self.observation_state_mapper.get_state(obs=obs, obs_var=obs_var, update_internals=False)
        action_model = self.actions_mapper.transform_action_raw_to_action_model(action)
        r, v = self.state_reward_mapper.get_reward(state_mu, state_var, action_model)
        return -r.item(), v.item()

    def add_memory(self, obs, action, obs_new, reward, predicted_state=None, predicted_state_std=None):
        """Reference :165-199."""
        state_mu, _ = self.observation_state_mapper.get_state(obs=obs, update_internals=False)
        state_mu_new, _ = self.observation_state_mapper.get_state(obs=obs_new, update_internals=False)
        action_model = self.actions_mapper.transform_action_raw_to_action_model(action)
        self.memory.add(state_mu, action_model, state_mu_new, reward, iter_ctrl=self.iter_ctrl - 1,
                        predicted_state=predicted_state, predicted_state_std=predicted_state_std)
        training_idle = not (hasattr(self, "p_train") and not self.p_train._closed)
        if self.iter_ctrl % self.config.training.training_frequency == 0 and training_idle:
            self.start_training_process()

    def start_training_process(self):
        saved_state = self.transition_model.save_state()
        saved_state.to_arrays()
        tc = self.config.training
        self.p_train = self.ctx.Process(target=GpStateTransitionModel.train,
                                        args=(self.queue_train, saved_state, tc.lr_train, tc.iter_train,
                                              tc.clip_grad_value, tc.print_train, tc.step_print_train,
                                              getattr(tc, "device", "auto")),
                                        kwargs=dict(optimizer=getattr(tc, "optimizer", "lbfgs"), restarts=getattr(tc, "restarts", 16),
                                                    device_iterations=getattr(tc, "device_iterations", 30),
                                                    device_history=getattr(tc, "device_history", 10)))
        self.p_train.start()

    def check_and_close_processes(self):
        """Reference :216-227: collect finished training, load the new hyper-parameters, refactorise."""
        if hasattr(self, "p_train") and not self.p_train._closed and not self.p_train.is_alive():
            # train() always queues exactly one result; a child that died before it could (killed, import error)
            # must not block the control loop: wait briefly, then keep the current hyper-parameters
            import queue as _queue
            try:
                params = self.queue_train.get(timeout=5.0 if self.p_train.exitcode == 0 else 0.5)
            except _queue.Empty:
                print(f"training process ended with exit code {self.p_train.exitcode} and no result: "
                      "keeping the current hyper-parameters")
                params = None
            self.p_train.join()
            if isinstance(params, TrainingFailed):
                # the child answered, but could not train (no GPU for it, unsupported device, search raised): say so
                # instead of silently carrying stale hyper-parameters (they are the incoming ones)
                self.training_failures = getattr(self, "training_failures", 0) + 1
                print(f"GP training failed ({params.reason}): keeping the current hyper-parameters "
                      f"({self.training_failures} failed training(s) so far)")
                params = None
            if params is not None:
                for model, p in zip(self.transition_model.models, params):
                    model.initialize(**p)
            self.p_train.close()
            self.memory.pop_evicted()          # new hyper-parameters: the whole memory is factorised anyway
            x_mem, y_mem = self.memory.get()
            self.transition_model.prepare_inference(x_mem, y_mem)

    def get_iter_info(self):
        return self.iter_info

    def store_iter_info(self, iter_info):
        for key, val in vars(iter_info).items():
            self.info_iters.setdefault(key, []).append(val)

    # ---------------------------------------------------------------------------- internals
    # The logging caches of the reference (:279-283) are written by EVERY objective evaluation but read once per control step
    # (get_action, :88-106): the sequential optimiser's evaluations keep the host arrays of their last call and the five
    # tensors are made when somebody looks.
    def _materialise_caches(self):
        host = self.__dict__.pop("_lazy_host", None)
        if host is not None:
            self._cache_trajectory({k: torch.from_numpy(v) for k, v in host.items()}, 0)

    def _lazy_cache_property(name):                    # noqa: N805 -- class-body helper
        def get(self):
            self._materialise_caches()
            return self.__dict__[name]

        def put(self, value):
            self.__dict__.pop("_lazy_host", None) if name == "states_mu_pred" else None
            self.__dict__[name] = value
        return property(get, put)

    states_mu_pred = _lazy_cache_property("states_mu_pred")
    states_var_pred = _lazy_cache_property("states_var_pred")
    rewards_trajectory = _lazy_cache_property("rewards_trajectory")
    rewards_traj_var = _lazy_cache_property("rewards_traj_var")
    cost_traj_mean_lcb = _lazy_cache_property("cost_traj_mean_lcb")
    del _lazy_cache_property

    def _cache_trajectory(self, out, idx):
        self.states_mu_pred = out["mu"][idx].cpu()
        self.states_var_pred = out["Sig"][idx].cpu()
        self.rewards_trajectory = -out["cost_mu"][idx].cpu()
        self.rewards_traj_var = out["cost_var"][idx].cpu()
        self.cost_traj_mean_lcb = -out["J"][idx].cpu()

    def _cache_packed_trajectory(self, packed, H, D):
        """The same caches from the [mu, Sig, cost_mu, cost_var, J] record another rank shipped (sharded shooting)."""
        n1, n2, n3 = (H + 1) * D, (H + 1) * D * D, H + 1
        o = np.cumsum([0, n1, n2, n3, n3])
        self.states_mu_pred = packed[o[0]:o[1]].view(H + 1, D).clone()
        self.states_var_pred = packed[o[1]:o[2]].view(H + 1, D, D).clone()
        self.rewards_trajectory = -packed[o[2]:o[3]].clone()
        self.rewards_traj_var = packed[o[3]:o[4]].clone()
        self.cost_traj_mean_lcb = -packed[o[4]].clone()

    def _prepare(self):
        # a capped memory (MemoryConfig.max_points_model) evicted its oldest points: they leave the cached factors by a
        # downdate, and the prepare below border-updates the appended ones -- no factorisation at steady state.  The downdate is
        # an economy, never a need: where it cannot be made -- evictions the model cannot match to rows it holds (nothing
        # prepared yet, points that came and went between two prepares), an engine without `forget`, or one that holds no
        # record to downdate from (GPMPC_ERR_ARG: e.g. after a failed factorisation) -- the prepare below sees a different
        # memory and factorises the window in full.
        evicted = self.memory.pop_evicted()
        x_old = self.transition_model.x_mem
        if len(evicted) and x_old is not None and len(evicted) < len(x_old) and hasattr(self.transition_model.engine, "forget"):
            try:
                self.transition_model.forget(evicted)
            except GpmpcError as e:
                if e.code != GPMPC_ERR_ARG:
                    raise
        x_mem, y_mem = self.memory.get()
        self.transition_model.prepare_inference(x_mem, y_mem)

    def _get_optimal_actions(self, state_mu, state_var):
        """Reference :114-153.  The searches and the table they are looked up in: candidate_search.py."""
        self._check_propagation_supported()
        self._prepare()
        _, search = candidate_search.lookup(self.config.controller)
        return self._adopt(search.run(self, state_mu, state_var))

    def _adopt(self, result):
        """Publish a search's winner (candidate_search.SearchResult): the diagnostics, the logging caches, the warm start of the
        next step; returns the winning sequence in model space."""
        for name, value in (result.diagnostics or {}).items():
            setattr(self, name, value)
        if result.index is not None:
            self.best_candidate_index = result.index
        if result.J is not None:
            self.best_candidate_J = result.J
        self.num_rollouts += result.rollouts
        kind = result.cache[0] if result.cache else None
        if kind == "evaluate":
            self._cache_trajectory(self.evaluate_candidates(result.x[None], *result.cache[1:], trajectories=True), 0)
        elif kind == "out":
            self._cache_trajectory(*result.cache[1:])
        elif kind == "packed":
            self._cache_packed_trajectory(result.cache[1], self.config.controller.len_horizon, self.transition_model.dim_state)
        self.actions_mpc_previous_iter = result.x.copy()
        return self.actions_mapper.transform_action_mpc_to_action_model(result.x)

    def objective_and_gradient_batch(self, actions_mpc_batch, obs_mu, obs_var):
        """(B, H*A) optimiser vectors -> (J (B,), dJ/d(actions_mpc) (B, H*A)) in one gpmpc_rollout_grad launch."""
        self._check_propagation_supported("objective_and_gradient_batch (the gradient path)")
        X = np.asarray(actions_mpc_batch, dtype=np.float64)
        acts = self.actions_mapper.mpc_to_model_batch(X)
        self.transition_model.set_cost(self.config.reward)
        if self.analytic_gradient:
            try:
                out = self.transition_model.objective_and_gradient_batch(acts, obs_mu, obs_var, self.iter_ctrl)
            except GpmpcError as e:
                if e.code != GPMPC_ERR_LIMIT:
                    raise
                self.analytic_gradient = False         # shape outside the gradient kernels: difference the rollout
            else:
                self.num_rollouts += X.shape[0]
                host = self.transition_model.engine.host_views(out)
                return host["J"].numpy(), self.actions_mapper.chain_grad_model_to_mpc_batch(host["grad"].numpy())
        J, g_model, _ = self._objective_and_gradient_by_differences(acts, obs_mu, obs_var)
        return J, self.actions_mapper.chain_grad_model_to_mpc_batch(g_model)

    def _get_random_actions(self, state_mu, state_var):
        """Reference :155-163: one random sequence, evaluated only to fill the logging caches."""
        H, A = self.config.controller.len_horizon, self.actions_mapper.dim_action
        actions_mpc = generate_mpc_action_init_random(len_horizon=H, dim_action=A)
        self._prepare()
        out = self.evaluate_candidates(actions_mpc[None], state_mu, state_var, trajectories=True)
        self._cache_trajectory(out, 0)
        return self.actions_mapper.transform_action_mpc_to_action_model(actions_mpc)
