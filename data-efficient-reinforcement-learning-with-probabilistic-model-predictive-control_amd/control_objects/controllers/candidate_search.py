"""The candidate searches of GpMpcController: one function per search, one table of what each supports.

A search takes (ctrl, state_mu, state_var), makes its draws from numpy's global generator, its launches and its collectives, and
returns a SearchResult; it sets nothing on the controller.  GpMpcController._get_optimal_actions looks the search up in SEARCHES
and hands the result to GpMpcController._adopt, the one place that publishes a winner.  The pieces every search used to carry a
copy of are here once: `draw_starts`, `derivative_mapper_kwargs`, `refuse_sharding`.  The exchanges between ranks and their
record layouts are in sharding.py."""
import functools
import threading
from typing import NamedTuple

import numpy as np
import torch
from scipy.optimize import minimize

from ... import sharding
from ..actions_mappers.action_init_functions import (generate_mpc_action_init_frompreviousiter,
                                                     generate_mpc_action_init_random)
from ..actions_mappers.mappers import DerivativeActionMapper


class SearchResult(NamedTuple):
    x: np.ndarray               # the winning optimiser vector (H*A,)
    cache: tuple                # what the logging caches take: ("evaluate", state_mu, state_var) = roll the winner out once more;
    #                             ("out", out, index) = this rollout's entry; ("packed", record) = the record another rank shipped;
    #                             None = the last objective evaluation left them (the sequential solver)
    J: float = None             # -> best_candidate_J / best_candidate_index, where the search has one
    index: int = None
    rollouts: int = 0           # candidate evaluations made inside the engine (those of evaluate_candidates count themselves)
    diagnostics: dict = None    # further attributes the search publishes on the controller (lbfgs_evaluations, ...)


# ------------------------------------------------------------------------------------------------------------ shared pieces
def draw_starts(ctrl, B, redraw=False):
    """B optimiser vectors in the order the reference draws them from numpy's global generator (:127-130): slot 0 is the shifted
    previous solution if init_from_previous_actions and there is one, every other slot a fresh random draw.  `redraw`: every start
    is thrown away for a second, fresh draw -- what the reference's optimize=False path evaluates (:143)."""
    cc = ctrl.config.controller
    H, A = cc.len_horizon, ctrl.actions_mapper.dim_action
    starts = []
    for b in range(B):
        if cc.init_from_previous_actions and ctrl.actions_mpc_previous_iter is not None and b == 0:
            x = generate_mpc_action_init_frompreviousiter(ctrl.actions_mpc_previous_iter, dim_action=A)
        else:
            x = generate_mpc_action_init_random(len_horizon=H, dim_action=A)
        starts.append(generate_mpc_action_init_random(len_horizon=H, dim_action=A) if redraw else x)
    return starts


def derivative_mapper_kwargs(ctrl):
    """What tells a device search to apply the DerivativeActionMapper itself; nothing for the normalisation mapper."""
    if not isinstance(ctrl.actions_mapper, DerivativeActionMapper):
        return {}
    return dict(max_change=np.asarray(ctrl.config.actions.max_change_action_norm, dtype=np.float64),
                action_prev=ctrl.actions_mapper.action_model_previous_iter.numpy())


def refuse_sharding(ctrl, what):
    """For a search that does not shard over ranks: every rank raises here, before any collective."""
    world, _ = ctrl._ranks()
    if world > 1:
        raise ValueError(f"candidate_optimizer={ctrl.config.controller.candidate_optimizer!r} does not shard its {what} over "
                         "ranks: switch ControllerConfig.shard_over_ranks off (every rank then runs the whole search)")


def _device_winner(best_x, best_J, J_all, status, what, state, rollouts, **diagnostics):
    """The result of a device search that returned (winner, its J, J and status of every start)."""
    if not np.isfinite(best_J):
        raise FloatingPointError(f"no finite objective among the {what}")
    best_i = int(np.flatnonzero(J_all == best_J)[0])          # the first strict minimum: gpmpc_argmin's rule
    return SearchResult(best_x, ("evaluate",) + state, float(best_J), best_i, rollouts,
                        dict(diagnostics, candidates_final_J=J_all, candidates_final_status=status))


# ----------------------------------------------------------------------------------------------------------------- searches
def scipy_restarts(ctrl, state_mu, state_var):
    """Reference :125-148: `restarts_optim` scipy L-BFGS-B solves one after the other, every evaluation one
    compute_mean_lcb_trajectory; the logging caches are those of the last evaluation (:279-283)."""
    cc = ctrl.config.controller
    results = []
    for x0 in draw_starts(ctrl, cc.restarts_optim):
        res = minimize(fun=ctrl.compute_mean_lcb_trajectory, x0=x0, jac=True, args=(state_mu, state_var),
                       method="L-BFGS-B", bounds=ctrl.actions_mapper.bounds, options=cc.actions_optimizer_params)
        results.append((res.fun, res.x))
    return SearchResult(sharding.keep_best(results)[1], None)


def random_shooting(ctrl, state_mu, state_var):
    """optimize=False: all `restarts_optim` random candidates in one launch, argmin on the device.  The reference draws TWO
    sequences per restart and evaluates the second (:127-130 then :143); reproduced so that a seeded run sees the same
    candidates.  With sharding, every rank draws the SAME B candidates (the global numpy generator, seeded identically on all
    ranks by the launcher; checked through a checksum inside the records) and evaluates its contiguous slice; a rank whose slice
    is empty (B < world) launches nothing and contributes an (inf, -1) record."""
    cc = ctrl.config.controller
    H, A = cc.len_horizon, ctrl.actions_mapper.dim_action
    cands = np.stack(draw_starts(ctrl, cc.restarts_optim, redraw=True))
    B = cands.shape[0]
    world, rank = ctrl._ranks()
    lo, hi = sharding.shard_bounds(B, world, rank)
    eng = ctrl.transition_model.engine
    failure = None
    try:
        out = ctrl.evaluate_candidates(cands[lo:hi], state_mu, state_var, trajectories=True) if hi > lo else None
    except Exception as e:                   # noqa: BLE001 -- world > 1: handed on after the collective
        if world == 1:
            raise
        # this rank must still enter the step's all_gather (its peers would wait in it until the watchdog fires): it
        # contributes an (inf, -1) record whose error flag every rank reads after the exchange
        failure, out = e, None
    local = torch.as_tensor(cands[lo:hi].reshape(hi - lo, H, A), device=eng.device)
    if failure is not None:
        local = local[:0]
    if world == 1:
        J, best, win = sharding.select_best_on_device(eng, out["J"], local, lo, B, group=sharding.LOCAL)
        cache = ("out", out, B - 1)          # the reference caches the LAST evaluated trajectory, not the winner's (:279-283)
    else:
        # ... and so must every rank here (get_action reads the caches on all of them): the exchange ships it
        J, best, win, last = sharding.shooting_exchange(eng, out, local, lo, B, ctrl.transition_model.dim_state, state_mu,
                                                        state_var, cands, failure, ctrl.process_group)
        cache = ("packed", last)
    return SearchResult(win.numpy().reshape(-1), cache, J, best)


def cross_entropy(ctrl, state_mu, state_var):
    """candidate_optimizer = "cem": batched replacement of the sequential scipy restarts: every iteration
    is ONE rollout launch over `cem_candidates` sequences drawn around the current mean (iteration 0: uniform, plus the shifted
    previous solution when init_from_previous_actions), the elites refit mean / std of a diagonal Gaussian over the optimiser
    vector in [0, 1]^(H*A); the best sequence ever evaluated wins."""
    cc = ctrl.config.controller
    H, A = cc.len_horizon, ctrl.actions_mapper.dim_action
    n, B = H * A, int(cc.cem_candidates)
    n_elite = max(2, int(round(B * cc.cem_elite_fraction)))
    rng = np.random                                        # the reference's global generator
    mean, std = np.full(n, 0.5), np.full(n, 0.5)
    best_x, best_J, cache = None, np.inf, None
    for it in range(int(cc.cem_iterations)):
        if it == 0:
            cands = rng.uniform(0.0, 1.0, size=(B, n))
            if cc.init_from_previous_actions and ctrl.actions_mpc_previous_iter is not None:
                cands[0] = generate_mpc_action_init_frompreviousiter(ctrl.actions_mpc_previous_iter, dim_action=A)
        else:
            cands = np.clip(mean + std * rng.standard_normal((B, n)), 0.0, 1.0)
            cands[0] = best_x                              # keep the incumbent
        out = ctrl.evaluate_candidates(cands, state_mu, state_var, trajectories=True)
        J = out["J"].cpu().numpy()
        J = np.where(np.isnan(J), np.inf, J)
        order = np.argsort(J, kind="stable")
        if J[order[0]] < best_J:
            best_J, best_x = float(J[order[0]]), cands[order[0]].copy()
            cache = ("out", out, int(order[0]))
        elites = cands[order[:n_elite]]
        mean, std = elites.mean(axis=0), elites.std(axis=0) + 1e-3
    if best_x is None:
        raise FloatingPointError("no finite objective among the candidates")
    return SearchResult(best_x, cache, best_J)


def cross_entropy_device(ctrl, state_mu, state_var):
    """candidate_optimizer = "cem_device": the cross-entropy search of `cross_entropy` with its whole loop on the GPU
    (gpmpc_cem_search: sampling, action mapper, rollout, elite selection and refit enqueued back to back, nothing read back
    between iterations).  Two host synchronisations per control step -- the winner, then its trajectory for the logging caches --
    instead of one per iteration; the draws are Philox, keyed by a seed taken from numpy's global generator (so `np.random.seed`
    still makes a run reproducible).  With sharding each rank draws its slice from the shared Philox key, one elite merge per
    iteration; the key, the state and the starting vector are rank 0's on every rank."""
    cc = ctrl.config.controller
    H, A = cc.len_horizon, ctrl.actions_mapper.dim_action
    B = int(cc.cem_candidates)
    n_elite = max(2, int(round(B * cc.cem_elite_fraction)))
    first = None
    if cc.init_from_previous_actions and ctrl.actions_mpc_previous_iter is not None:
        first = generate_mpc_action_init_frompreviousiter(ctrl.actions_mpc_previous_iter, dim_action=A)
    kw = derivative_mapper_kwargs(ctrl)
    seed = int(np.random.randint(0, 2 ** 62))          # the Philox key (np.random.seed keeps a run reproducible)
    tm = ctrl.transition_model
    tm.set_cost(ctrl.config.reward)
    world, _ = ctrl._ranks()
    if world > 1:
        seed, first, state_mu, state_var = sharding.cem_head_exchange(seed, first, state_mu, state_var, H * A, tm.engine.device,
                                                                      ctrl.process_group)
        search, kw = functools.partial(sharding.sharded_cem_search, tm.engine), dict(kw, group=ctrl.process_group)
    else:
        search = tm.engine.cem_search
    best_x, best_J = search(np.asarray(state_mu, dtype=np.float64), np.asarray(state_var, dtype=np.float64), B, H, A,
                            int(cc.cem_iterations), n_elite, seed=seed, include_time=tm.config.include_time_model,
                            time0=float(ctrl.iter_ctrl), first_candidate=first, **kw)
    if not np.isfinite(best_J):
        raise FloatingPointError("no finite objective among the candidates")
    return SearchResult(best_x, ("evaluate", state_mu, state_var), best_J, None, B * int(cc.cem_iterations))


def lockstep_restarts(ctrl, state_mu, state_var):
    """candidate_optimizer = "lbfgs": all restarts at once.  The reference runs `restarts_optim` scipy
    L-BFGS-B solves one after the other, every function evaluation a forward + autograd backward of ONE sequence (:125-141).
    Here the same scipy solver runs once per restart, each in its own thread, but the threads advance in lockstep: whenever
    every unfinished restart is waiting for an evaluation, ONE objective + analytic-gradient launch serves them all.  Each
    restart therefore sees exactly the values the sequential loop would hand it (the kernels are bitwise independent of the
    batch composition), ends at the same point, and the keep-the-best rule (:146-148) picks the same winner; the wall time is
    that of the longest restart instead of their sum.  With sharding, every rank solves its contiguous slice of rank 0's
    starting points and the winners meet in one all_gather (sharding.restart_winner_exchange)."""
    cc = ctrl.config.controller
    H, A = cc.len_horizon, ctrl.actions_mapper.dim_action
    B = int(cc.lbfgs_candidates or cc.restarts_optim)
    x0s = draw_starts(ctrl, B)
    world, rank = ctrl._ranks()
    if world > 1:
        # rank 0's starting points on every rank (one small broadcast per control step instead of trusting the launcher's seeds)
        x0s = list(sharding.broadcast_from_first(np.stack(x0s), ctrl.transition_model.engine.device, ctrl.process_group))
    r_lo, r_hi = sharding.shard_bounds(B, world, rank)
    x0s, B = x0s[r_lo:r_hi], r_hi - r_lo
    cond = threading.Condition()
    pending, results, state = {}, {}, {"running": B, "launches": 0, "error": None}

    def flush():                                   # called with the lock held, by the last thread to arrive
        idx = sorted(pending)
        J, G = np.full(len(idx), np.nan), np.zeros((len(idx), H * A))
        try:
            J, G = ctrl.objective_and_gradient_batch(np.stack([pending[i] for i in idx]), state_mu, state_var)
        except BaseException as e:                 # every waiting restart is served -- nobody may wait forever ...
            state["error"] = e if isinstance(e, Exception) else RuntimeError(repr(e))
            if not isinstance(e, Exception):       # ... and KeyboardInterrupt / SystemExit go on in the flushing thread
                raise
        finally:
            state["launches"] += 1
            for k, i in enumerate(idx):
                results[i] = (float(J[k]), G[k].copy())
            pending.clear()
            cond.notify_all()

    def make_fun(i):
        def fun(x):
            with cond:
                pending[i] = np.array(x, dtype=np.float64)
                if len(pending) == state["running"]:
                    flush()
                waited = 0.0
                while i not in results:
                    # a rendezvous that never completes (a sibling died outside `worker`'s bookkeeping) must not hang the step
                    if not cond.wait(timeout=5.0):
                        waited += 5.0
                        if waited >= 600.0:
                            pending.pop(i, None)
                            raise TimeoutError(f"lockstep evaluation of restart {i} not served within 600 s")
                out = results.pop(i)
            if state["error"] is not None:
                raise RuntimeError("batched evaluation failed") from state["error"]
            return out
        return fun

    solved = [None] * B

    def worker(i):
        try:
            solved[i] = minimize(fun=make_fun(i), x0=x0s[i], jac=True, method="L-BFGS-B",
                                 bounds=ctrl.actions_mapper.bounds, options=cc.actions_optimizer_params)
        except BaseException as e:
            solved[i] = e
        finally:
            with cond:
                state["running"] -= 1
                if pending and len(pending) == state["running"]:
                    flush()

    threads = [threading.Thread(target=worker, args=(i,), daemon=True) for i in range(B)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    failure = next((r for r in solved if isinstance(r, BaseException)), None)
    if failure is not None and world == 1:
        raise failure
    # world > 1: a rank whose solves failed must still enter the collective (the others would wait in it until the watchdog
    # fires); its record carries an error flag and every rank raises after the gather
    ends = [] if failure is not None else [(r.fun, r.x) for r in solved]
    if world > 1:
        opt_fun, best_i, best = sharding.restart_winner_exchange(ends, r_lo, H * A, state_mu, state_var,
                                                                 ctrl.transition_model.engine.device, failure, ctrl.process_group)
        final_J = None                             # only this rank's slice was solved here
    else:
        opt_fun, best, best_i = sharding.keep_best(ends)
        final_J = np.array([fun for fun, _ in ends])
    return SearchResult(best, ("evaluate", state_mu, state_var), float(opt_fun), best_i, 0,
                        dict(lbfgs_evaluations=state["launches"], candidates_final_J=final_J))


def lbfgs_device(ctrl, state_mu, state_var):
    """candidate_optimizer = "lbfgs_device": a box-constrained L-BFGS from `lbfgs_candidates` starts whose whole loop stays on
    the GPU (gpmpc_lbfgs_search: per iteration one objective + analytic-gradient launch over the restarts' trial points and one
    step kernel; the line search is spread over iterations, so nothing is read back until the winner).  Two host
    synchronisations per control step: the winner, then its trajectory for the logging caches.  Works for both uncertainty
    propagations (open loop)."""
    refuse_sharding(ctrl, "restarts")
    cc = ctrl.config.controller
    H, A = cc.len_horizon, ctrl.actions_mapper.dim_action
    B = int(cc.lbfgs_candidates or cc.restarts_optim)
    iterations = int(cc.lbfgs_device_iterations)
    starts = np.stack(draw_starts(ctrl, B)).astype(np.float64).reshape(B, H * A)
    tm = ctrl.transition_model
    tm.set_cost(ctrl.config.reward)
    found = tm.engine.lbfgs_search_host(
        starts, np.asarray(state_mu, dtype=np.float64), np.asarray(state_var, dtype=np.float64), H, A, iterations,
        history=int(cc.lbfgs_device_history), propagation="linearized" if tm.propagation() == "linearized" else "moment",
        include_time=tm.config.include_time_model, time0=float(ctrl.iter_ctrl), **derivative_mapper_kwargs(ctrl))
    return _device_winner(*found, "restarts", (state_mu, state_var), B * iterations,
                          lbfgs_device_starts=starts, lbfgs_evaluations=iterations)


def ilqr_device(ctrl, state_mu, state_var):
    """candidate_optimizer = "ilqr_device": a clamped iLQR on the mean dynamics of the linearised propagation from
    `ilqr_candidates` starts whose whole loop stays on the GPU (gpmpc_ilqr_search: per iteration a backward Riccati sweep along
    each candidate's nominal trajectory, a closed-loop forward pass for every step size of the line search, an accept rule;
    nothing is read back until the winner).  The design is certainty-equivalent; the winner is chosen by the LCB objective of
    gpmpc_rollout_linear.  Two host synchronisations per control step: the winner, then its trajectory for the logging caches."""
    refuse_sharding(ctrl, "starts")
    cc = ctrl.config.controller
    H, A = cc.len_horizon, ctrl.actions_mapper.dim_action
    B = int(cc.ilqr_candidates or cc.restarts_optim)
    iterations = int(cc.ilqr_iterations)
    starts = np.stack(draw_starts(ctrl, B)).astype(np.float64).reshape(B, H * A)
    tm = ctrl.transition_model
    tm.set_cost(ctrl.config.reward)
    found = tm.engine.ilqr_search_host(
        starts, np.asarray(state_mu, dtype=np.float64), np.asarray(state_var, dtype=np.float64), H, A, iterations,
        line_search_steps=int(cc.ilqr_line_search_steps), reg0=float(cc.ilqr_reg),
        include_time=tm.config.include_time_model, time0=float(ctrl.iter_ctrl))
    return _device_winner(*found, "starts", (state_mu, state_var), B * iterations * (1 + int(cc.ilqr_line_search_steps)),
                          ilqr_device_starts=starts, ilqr_iterations_run=iterations)


# -------------------------------------------------------------------------------------------------------------------- table
class Search(NamedTuple):
    run: callable
    propagations: tuple         # ModelConfig.uncertainty_propagation values it exists under
    feedback: bool              # plans under ControllerConfig.feedback_gain (closed loop; the linearised propagation only)
    derivative: bool            # works with the DerivativeActionMapper
    shards: bool                # splits its candidates over ranks; False: every rank runs the whole search, or refuse_sharding
    why_not: dict = {}          # its own words for what it refuses (a search without them gets the generic message)


_BOTH = ("moment_matching", "linearized")
# Keyed by what the config says: optimize=False -> False, otherwise ControllerConfig.candidate_optimizer.  A string that is not
# a key runs the scipy restarts, as it always has (`lookup`).
SEARCHES = {
    False: Search(random_shooting, _BOTH, feedback=True, derivative=True, shards=True),
    None: Search(scipy_restarts, ("moment_matching",), feedback=False, derivative=True, shards=False),
    "cem": Search(cross_entropy, _BOTH, feedback=True, derivative=True, shards=False),
    "cem_device": Search(cross_entropy_device, ("moment_matching",), feedback=False, derivative=True, shards=True),
    "lbfgs": Search(lockstep_restarts, ("moment_matching",), feedback=False, derivative=True, shards=True),
    "lbfgs_device": Search(lbfgs_device, _BOTH, feedback=False, derivative=True, shards=False,
                           why_not={"feedback": "searches the open-loop objective"}),
    "ilqr_device": Search(ilqr_device, ("linearized",), feedback=False, derivative=False, shards=False,
                          why_not={"propagation": "the iLQR runs on the mean dynamics of the linearised propagation, moment "
                                                  "matching has none",
                                   "feedback": "plans in open loop",
                                   "derivative": "optimises the model actions themselves: it needs the normalisation action "
                                                 "mapper, not the DerivativeActionMapper"}),
}


def name_of(key):
    """A table key in the words of the messages."""
    return "optimize=False (random shooting)" if key is False else f"candidate_optimizer={key!r}"


def lookup(controller_config):
    """(key as the config gives it, table entry) of the search a ControllerConfig asks for."""
    if not controller_config.optimize:
        return False, SEARCHES[False]
    opt = getattr(controller_config, "candidate_optimizer", None)
    return opt, SEARCHES[opt] if isinstance(opt, str) and opt in SEARCHES else SEARCHES[None]


def linearized_optimizers():
    """The searches of the linearised propagation, in the words of the refusal message."""
    have = [key for key, s in SEARCHES.items() if "linearized" in s.propagations]
    return (", ".join(name_of(k) for k in have if SEARCHES[k].feedback) + " or, in open loop, "
            + " or ".join(name_of(k) for k in have if not SEARCHES[k].feedback))
