"""What engine.py hands to the C ABI, recorded without a GPU: the real HipEngine methods run against a stand-in for the
library that notes every call and returns GPMPC_OK.  tests/test_engine_marshalling.py compares the record with
tests/golden/engine_calls.json, written by tools/gen_engine_calls_golden.py.

Per call: the C function's name, every integer and float by value, every pointer by ROLE -- ["in", name] an argument of the
case passed through unconverted, ["out", key] a tensor of the returned dict, ["host", name, values] a host array with what
it holds, ["dev", shape, values] a tensor the engine converted itself (expanded gains, a float32 input, the ones of a
`*_grad`), None a NULL.  Per case: the returned keys, shapes and dtypes, or the ValueError's text."""
import ctypes as C

import numpy as np
import torch

from gp_mpc_amd import _lib as L
from gp_mpc_amd.engine import HipEngine

B, H, D, A = 2, 3, 2, 1
P = 3                                   # query rows (M), Gaussian inputs (P) and rows of Xa (Ma)


class Recorder:
    """Stands where the loaded library stands: every gpmpc_* attribute is a function that notes its arguments."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("gpmpc_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return L.GPMPC_OK
        return fn


class RecordingEngine(HipEngine):
    def __init__(self, E, cost):
        self.lib = Recorder()
        self.device = torch.device("cpu")
        self._h = None
        self.N, self.D, self.E = 8, D, E
        self._cost = cost
        self.converted = []

    def _stream(self):
        return None

    def _dev(self, t, shape=None):
        t = super()._dev(t, shape)
        self.converted.append(t)         # kept alive, so that no address is handed out twice within a case
        return t


def make_inputs(E):
    """The arguments of every case by name; float64 and contiguous, so that the engine passes them on unconverted."""
    shapes = {
        "actions": (B, H, A), "Xq": (P, E), "mean_bar": (P, D), "var_bar_q": (P, D), "Xa": (P, E), "Xb": (2, E), "Xb0": (0, E),
        "mu": (P, E), "var": (P, E, E), "M_bar": (P, D), "S_bar": (P, D, D), "V_bar": (P, E, D),
        "mu_bar": (B, H + 1, D), "Sig_bar": (B, H + 1, D, D), "cost_mu_bar": (B, H + 1), "cost_var_bar": (B, H + 1),
        "J_bar": (B,), "gains_AD": (A, D), "gains_HAD": (H, A, D), "gains_BHAD": (B, H, A, D),
        # wrong shapes, for the ValueError paths
        "rank1": (E,), "Xb_wrongE": (2, E + 1), "bad_PD": (P + 1, D), "bad_var": (P, E), "bad_S_bar": (P, D), "bad_V_bar": (P, D, E),
        "bad_mu_bar": (B, H, D), "bad_Sig_bar": (B, H + 1, D), "bad_cost_bar": (B, H), "bad_J_bar": (B + 1,),
        "bad_gains": (H, D, A), "actions_rank2": (B, H),
    }
    ins = {}
    for k, (name, sh) in enumerate(shapes.items()):
        n = int(np.prod(sh))
        ins[name] = (torch.arange(n, dtype=torch.float64) * 0.5 + k).reshape(sh)
    ins["actions_f32"] = ins["actions"].to(torch.float32)
    ins["mu0"] = np.array([0.25, -0.5])
    ins["S0"] = np.array([[0.5, 0.125], [0.125, 0.75]])
    ins["noises"] = np.array([0.01, 0.02])
    ins["bad_mu0"] = np.zeros(D + 1)
    ins["bad_S0"] = np.zeros((D, D + 1))
    ins["bad_noises"] = np.zeros(D + 1)
    return ins


def _cases():
    """(id, E, cost, method, args, kwargs).  A string "@name" stands for make_inputs(E)[name]; the kwarg `out` takes "reuse"
    (the dict of a first, unrecorded call with the same arguments), "J_only", "bad_J" or "bad_mu"."""
    c = []

    def add(cid, method, *args, E=3, cost=(D, A), **kw):
        c.append((cid, E, cost, method, args, kw))

    for E in (3, 4):
        t = dict(E=E)
        s = f"E{E}"
        add(f"predict-{s}", "predict", "@Xq", **t)
        add(f"predict-noises-{s}", "predict", "@Xq", noises="@noises", **t)
        add(f"predict_backward-{s}", "predict_backward", "@Xq", mean_bar="@mean_bar", var_bar="@var_bar_q", **t)
        add(f"predict_cov-joint-{s}", "predict_cov", "@Xa", noises="@noises", **t)
        add(f"predict_cov-cross-{s}", "predict_cov", "@Xa", "@Xb", **t)
        for m in ("moments", "moments_linear"):
            add(f"{m}-{s}", m, "@mu", "@var", **t)
            add(f"{m}_backward-{s}", m + "_backward", "@mu", "@var", M_bar="@M_bar", S_bar="@S_bar", V_bar="@V_bar", **t)
        time = dict(include_time=(E == 4), time0=1.5 if E == 4 else 0.0)
        for m in ("rollout", "rollout_linear"):
            add(f"{m}-{s}", m, "@actions", "@mu0", "@S0", **time, **t)
            add(f"{m}_backward-{s}", m + "_backward", "@actions", "@mu0", "@S0", mu_bar="@mu_bar", Sig_bar="@Sig_bar",
                cost_mu_bar="@cost_mu_bar", cost_var_bar="@cost_var_bar", J_bar="@J_bar", **time, **t)
        add(f"rollout_linear_feedback-{s}", "rollout_linear_feedback", "@actions", "@gains_BHAD", "@mu0", "@S0", **time, **t)
        add(f"rollout_linear_feedback_backward-{s}", "rollout_linear_feedback_backward", "@actions", "@gains_BHAD", "@mu0", "@S0",
            mu_bar="@mu_bar", Sig_bar="@Sig_bar", cost_mu_bar="@cost_mu_bar", cost_var_bar="@cost_var_bar", J_bar="@J_bar",
            **time, **t)

    # -- query points ---------------------------------------------------------------------------------------------------------
    add("predict-mean_only", "predict", "@Xq", var=False)
    add("predict-var_only", "predict", "@Xq", mean=False)
    add("predict-rank", "predict", "@rank1")
    add("predict-bad_noises", "predict", "@Xq", noises="@bad_noises")
    add("predict_backward-no_seed", "predict_backward", "@Xq")
    add("predict_backward-mean_bar", "predict_backward", "@Xq", mean_bar="@mean_bar")
    add("predict_backward-var_bar", "predict_backward", "@Xq", var_bar="@var_bar_q")
    add("predict_backward-rank", "predict_backward", "@rank1")
    add("predict_backward-bad_mean_bar", "predict_backward", "@Xq", mean_bar="@bad_PD")
    add("predict_backward-bad_var_bar", "predict_backward", "@Xq", var_bar="@bad_PD")
    add("predict_cov-joint-plain", "predict_cov", "@Xa")
    add("predict_cov-cross-Mb0", "predict_cov", "@Xa", "@Xb0")
    add("predict_cov-rank", "predict_cov", "@rank1")
    add("predict_cov-Xb_rank", "predict_cov", "@Xa", "@rank1")
    add("predict_cov-Xb_wrongE", "predict_cov", "@Xa", "@Xb_wrongE")
    add("predict_cov-bad_noises", "predict_cov", "@Xa", noises="@bad_noises")
    for m in ("moments", "moments_linear"):
        add(f"{m}-no_var", m, "@mu")
        add(f"{m}-no_S", m, "@mu", "@var", S=False)
        add(f"{m}-no_V", m, "@mu", "@var", V=False)
        add(f"{m}-M_only", m, "@mu", S=False, V=False)
        add(f"{m}-rank", m, "@rank1")
        add(f"{m}-bad_var", m, "@mu", "@bad_var")
        b = m + "_backward"
        add(f"{b}-no_seed", b, "@mu")
        add(f"{b}-M_bar", b, "@mu", M_bar="@M_bar")
        add(f"{b}-S_bar", b, "@mu", "@var", S_bar="@S_bar")
        add(f"{b}-V_bar", b, "@mu", "@var", V_bar="@V_bar")
        add(f"{b}-no_mu_bar", b, "@mu", "@var", M_bar="@M_bar", mu_bar=False)
        add(f"{b}-no_var_bar", b, "@mu", "@var", M_bar="@M_bar", var_bar=False)
        add(f"{b}-rank", b, "@rank1")
        add(f"{b}-bad_var", b, "@mu", "@bad_var")
        add(f"{b}-bad_M_bar", b, "@mu", M_bar="@bad_PD")
        add(f"{b}-bad_S_bar", b, "@mu", S_bar="@bad_S_bar")
        add(f"{b}-bad_V_bar", b, "@mu", V_bar="@bad_V_bar")

    # -- forward rollouts -----------------------------------------------------------------------------------------------------
    fwd = [("rollout", ()), ("rollout_linear", ()), ("rollout_linear_feedback", ("@gains_HAD",))]
    for m, g in fwd:
        a = ("@actions",) + g + ("@mu0", "@S0")
        add(f"{m}-no_traj", m, *a, trajectories=False)
        add(f"{m}-no_costs", m, *a, stage_costs=False)
        add(f"{m}-J_alone", m, *a, trajectories=False, stage_costs=False)
        add(f"{m}-no_costs-no_set_cost", m, *a, stage_costs=False, cost=None)
        add(f"{m}-no_costs-other_cost", m, *a, stage_costs=False, cost=(D, A + 1))
        add(f"{m}-costs-no_set_cost", m, *a, trajectories=False, cost=None)
        add(f"{m}-out_reuse", m, *a, out="reuse")
        add(f"{m}-out_J_only", m, *a, out="J_only")
        add(f"{m}-out_bad_J", m, *a, out="bad_J")
        add(f"{m}-out_bad_mu", m, *a, out="bad_mu")
        add(f"{m}-actions_f32", m, "@actions_f32", *a[1:])
        add(f"{m}-actions_rank", m, "@actions_rank2", *a[1:])
        add(f"{m}-bad_mu0", m, *a[:-2], "@bad_mu0", "@S0")
        add(f"{m}-bad_S0", m, *a[:-2], "@mu0", "@bad_S0")
    for m in ("rollout_linear_feedback", "rollout_linear_feedback_backward"):
        for gname in ("None", "AD", "HAD", "BHAD"):
            g = None if gname == "None" else "@gains_" + gname
            add(f"{m}-gains_{gname}", m, "@actions", g, "@mu0", "@S0")
        add(f"{m}-bad_gains", m, "@actions", "@bad_gains", "@mu0", "@S0")
    add("lqr_gains", "lqr_gains", "@actions", "@mu0")
    add("lqr_gains-all", "lqr_gains", "@actions", "@mu0", True, 2.0, 0.5, True, True, E=4)
    add("rollout_linear_lqr", "rollout_linear_lqr", "@actions", "@mu0", "@S0", reg=0.25)
    add("rollout_linear_lqr-J_alone", "rollout_linear_lqr", "@actions", "@mu0", "@S0", trajectories=False, stage_costs=False)

    # -- backward rollouts ----------------------------------------------------------------------------------------------------
    bwd = [("rollout_backward", ()), ("rollout_linear_backward", ()), ("rollout_linear_feedback_backward", ("@gains_HAD",))]
    seeds = {"mu_bar": "@mu_bar", "Sig_bar": "@Sig_bar", "cost_mu_bar": "@cost_mu_bar", "cost_var_bar": "@cost_var_bar",
             "J_bar": "@J_bar"}
    bad = {"mu_bar": "@bad_mu_bar", "Sig_bar": "@bad_Sig_bar", "cost_mu_bar": "@bad_cost_bar", "cost_var_bar": "@bad_cost_bar",
           "J_bar": "@bad_J_bar"}
    for m, g in bwd:
        a = ("@actions",) + g + ("@mu0", "@S0")
        add(f"{m}-no_seed", m, *a)
        for k in seeds:
            add(f"{m}-only_{k}", m, *a, **{k: seeds[k]})
            add(f"{m}-bad_{k}", m, *a, **{k: bad[k]})
        add(f"{m}-no_initial", m, *a, J_bar="@J_bar", want_initial=False)
        add(f"{m}-actions_rank", m, "@actions_rank2", *a[1:])
        add(f"{m}-bad_mu0", m, *a[:-2], "@bad_mu0", "@S0")
        add(f"{m}-bad_S0", m, *a[:-2], "@mu0", "@bad_S0")
    add("rollout_linear_feedback_backward-no_gains_bar", "rollout_linear_feedback_backward", "@actions", "@gains_HAD", "@mu0", "@S0",
        J_bar="@J_bar", want_gains=False)
    add("rollout_linear_feedback_backward-no_gains_bar-no_initial", "rollout_linear_feedback_backward", "@actions", "@gains_AD",
        "@mu0", "@S0", mu_bar="@mu_bar", want_gains=False, want_initial=False)
    add("rollout_linear_grad", "rollout_linear_grad", "@actions", "@mu0", "@S0")
    add("rollout_linear_feedback_grad", "rollout_linear_feedback_grad", "@actions", "@gains_AD", "@mu0", "@S0")
    add("rollout_linear_feedback_grad-no_gains", "rollout_linear_feedback_grad", "@actions", None, "@mu0", "@S0", True, 3.0, E=4)
    return c


CASES = _cases()
IDS = [c[0] for c in CASES]
assert len(set(IDS)) == len(IDS)


def _values(t):
    return [float(v) for v in np.asarray(t, dtype=np.float64).reshape(-1)]


def _describe(res):
    if isinstance(res, torch.Tensor):
        return [list(res.shape), str(res.dtype)]
    return {k: (_describe(v) if isinstance(v, torch.Tensor) else type(v).__name__) for k, v in res.items()}


def run_case(case):
    """The record of one case: {"calls": [...], "result": ...} or {"calls": [...], "raises": text}."""
    cid, E, cost, method, args, kw = case
    ins = make_inputs(E)
    eng = RecordingEngine(E, cost)

    def value(v):
        return ins[v[1:]] if isinstance(v, str) and v.startswith("@") else v
    args = [value(v) for v in args]
    kw = {k: value(v) for k, v in kw.items()}
    f64 = dict(dtype=torch.float64)
    if kw.get("out") == "reuse":
        kw["out"] = getattr(eng, method)(*args, **{k: v for k, v in kw.items() if k != "out"})
        eng.lib.calls.clear()
    elif kw.get("out") == "J_only":
        kw["out"] = {"J": torch.empty(B, **f64)}
    elif kw.get("out") == "bad_J":
        kw["out"] = {"J": torch.empty(B + 1, **f64)}
    elif kw.get("out") == "bad_mu":
        kw["out"] = {"mu": torch.empty((B, H, D), **f64), "Sig": torch.empty((B, H + 1, D, D), **f64)}
    try:
        res = getattr(eng, method)(*args, **kw)
    except ValueError as e:
        return {"calls": [_call(eng, name, a, ins, {}) for name, a in eng.lib.calls], "raises": str(e)}
    outs = {"": res} if isinstance(res, torch.Tensor) else res
    rec = {"calls": [_call(eng, name, a, ins, outs) for name, a in eng.lib.calls], "result": _describe(res)}
    if "out" in kw:                      # the tensors handed in are the tensors written and returned
        rec["out_reused"] = res is kw["out"] or all(res[k] is t for k, t in kw["out"].items())
    return rec


def _call(eng, name, args, ins, outs):
    types = L.SIGNATURES[name][1]
    assert len(args) == len(types), (name, len(args), len(types))
    rec = []
    for i, (v, ty) in enumerate(zip(args, types)):
        if i == 0:
            assert v is None             # the handle
            continue
        if ty is C.c_int:
            rec.append(v if type(v) is int else f"{type(v).__name__}:{v}")
        elif ty is C.c_double:
            rec.append(v if type(v) is float else f"{type(v).__name__}:{v}")
        else:
            assert ty is C.c_void_p, (name, i, ty)
            rec.append(_role(eng, v, ins, outs))
    return {"fn": name, "args": rec}


def _role(eng, v, ins, outs):
    if v is None:
        return None
    if isinstance(v, C.c_void_p):        # a host array
        for k, a in ins.items():
            if isinstance(a, np.ndarray) and a.ctypes.data == v.value:
                held = np.ctypeslib.as_array((C.c_double * a.size).from_address(v.value))
                return ["host", k, _values(held)]
        return ["host", "?"]
    assert type(v) is int, type(v)
    for k, t in outs.items():
        if isinstance(t, torch.Tensor) and t.numel() and t.data_ptr() == v:
            return ["out", k]
    for k, t in ins.items():
        if isinstance(t, torch.Tensor) and t.numel() and t.data_ptr() == v:
            return ["in", k]
    for t in eng.converted:
        if t.numel() and t.data_ptr() == v:
            return ["dev", list(t.shape), _values(t)]
    return ["?"]


def run_all():
    return {c[0]: run_case(c) for c in CASES}
