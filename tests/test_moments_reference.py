"""Tier 1 (CPU): moment-matched prediction at uncertain inputs, pinned to the reference's own code.

tests/golden/moments_full_var*.npz hold predict_next_state_change (gp_model.py:112-180) at 24 Gaussian inputs each, with a
general input covariance: dense over state, action and time inputs, action block only, time variance only, zero and several
lengthscales wide (tools/gen_golden_moments.py).  The oracle's batched restatement must reproduce them, and
GpStateTransitionModel.predict_next_state_change must hand its engine the right shapes and return the reference's.
"""
import numpy as np
import pytest
import torch

from helpers import load, workload_of, rel_err
from oracle import gpmpc_oracle as orc
from stub_engine import OracleEngine

GOLDENS = ["moments_full_var", "moments_full_var_time"]


def _factors(g):
    w = workload_of(g)
    return orc.Factors(w.X, w.Y, w.lengthscales, w.outputscales, w.noises, iK=g["iK"], beta=g["beta"])


@pytest.mark.parametrize("name", GOLDENS)
def test_oracle_reproduces_reference(name):
    g = load(name)
    f = _factors(g)
    P, E = g["in_mean"].shape
    D = g["M"].shape[1]
    assert P == 24 and g["in_var"].shape == (P, E, E) and g["S"].shape == (P, D, D) and g["V"].shape == (P, E, D)
    M, S, V = orc.moment_match_step(f, g["in_mean"], g["in_var"])
    # the tolerances of test_oracle_vs_golden.py::test_single_step
    assert rel_err(M, g["M"]) < 1e-10
    assert rel_err(V, g["V"]) < 1e-10
    assert rel_err(S, g["S"]) < 1e-6
    for k in range(5):                                  # every kind of covariance, on its own scale
        sel = g["kind"] == k
        assert rel_err(S[sel], g["S"][sel]) < 1e-6, k
        assert rel_err(V[sel], g["V"][sel]) < 1e-10, k


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_covers_the_covariance_kinds(name):
    g = load(name)
    s, kind = g["in_var"], g["kind"]
    E = s.shape[1]
    D = g["M"].shape[1]
    A = E - D - int(bool(g["include_time"]))
    assert np.all(np.abs(s[kind == 0]) > 0)                                  # dense: every entry correlated
    blk = s[kind == 1].copy()
    assert np.all(np.abs(blk[:, D:D + A, D:D + A]) > 0)
    blk[:, D:D + A, D:D + A] = 0.0
    assert np.all(blk == 0.0)
    tv = s[kind == 2].copy()
    assert np.all(tv[:, -1, -1] > 0)
    tv[:, -1, -1] = 0.0
    assert np.all(tv == 0.0)
    assert np.all(s[kind == 3] == 0.0)
    # wide: input standard deviations of several lengthscales
    ls = load(name)["lengthscales"].min(axis=0)
    sd = np.sqrt(np.diagonal(s[kind == 4], axis1=1, axis2=2))
    assert np.all(sd.max(axis=1) > 2.0 * ls.max())
    # the action and time rows of V are not zero where those inputs carry variance
    assert np.all(np.abs(g["V"][kind == 0][:, D:, :]).max(axis=(1, 2)) > 0)


class MomentsStub(OracleEngine):
    """The CPU stand-in plus `moments`, by the oracle; it records what the model passed down."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def moments(self, mu, var=None, S=True, V=True):
        mu = np.asarray(mu, dtype=np.float64)
        P, E = mu.shape
        var = np.zeros((P, E, E)) if var is None else np.asarray(var, dtype=np.float64)
        self.calls.append((mu.shape, var.shape))
        M, Sm, Vm = orc.moment_match_step(self.f, mu, var)
        t = torch.as_tensor
        return {"M": t(M), "S": t(Sm), "V": t(Vm)}


@pytest.mark.parametrize("name", GOLDENS)
def test_transition_model_method(name):
    from gp_mpc_amd.config_classes import ModelConfig
    from gp_mpc_amd.control_objects.models.gp_model import GpStateTransitionModel
    g = load(name)
    w = workload_of(g)
    D = w.Y.shape[1]
    E = w.X.shape[1]
    tm = bool(g["include_time"])
    cfg = ModelConfig(gp_init={"noise_covar.noise": list(w.noises), "outputscale": list(w.outputscales),
                               "base_kernel.lengthscale": w.lengthscales[:, :E - int(tm)].tolist()}, include_time_model=tm)
    eng = MomentsStub()
    model = GpStateTransitionModel(cfg, D, E - D - int(cfg.include_time_model), engine=eng)
    assert model.dim_input == E
    with pytest.raises(RuntimeError):
        model.predict_next_state_change(torch.zeros(E), torch.zeros(E, E))
    model.prepare_inference(torch.as_tensor(w.X), torch.as_tensor(w.Y))
    eng.f = _factors(g)                       # the reference's hyper-parameters and factors
    for p in (0, 9, 13, 17, 21):
        Mt, S, Vt = model.predict_next_state_change(torch.as_tensor(g["in_mean"][p]), torch.as_tensor(g["in_var"][p]))
        assert eng.calls[-1] == ((1, E), (1, E, E))
        for t in (Mt, S, Vt):
            assert isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.device.type == "cpu"
        assert Mt.shape == (1, D) and S.shape == (D, D) and Vt.shape == (E, D)
        assert rel_err(Mt.numpy(), g["M"][p][None]) < 1e-10
        assert rel_err(Vt.numpy(), g["V"][p]) < 1e-10
        assert rel_err(S.numpy(), g["S"][p]) < 1e-6
    # numpy inputs are accepted as the reference's torch ones are
    Mt, S, Vt = model.predict_next_state_change(g["in_mean"][0], g["in_var"][0])
    assert Mt.shape == (1, D)
    out = model.predict_next_state_change_batch(torch.as_tensor(g["in_mean"]), torch.as_tensor(g["in_var"]))
    assert eng.calls[-1] == ((24, E), (24, E, E))
    assert out["M"].shape == (24, D) and out["S"].shape == (24, D, D) and out["V"].shape == (24, E, D)
    model.predict_next_state_change_batch(torch.as_tensor(g["in_mean"]))
    assert eng.calls[-1] == ((24, E), (24, E, E))


def test_abstract_model_default():
    from gp_mpc_amd.control_objects.models.abstract_model import AbstractStateTransitionModel

    class Minimal(AbstractStateTransitionModel):
        def prepare_inference(self, x, y):
            pass

        def predict_trajectory(self, actions, obs_mu, obs_var, len_horizon, current_time_idx):
            pass

        def save_state(self):
            return None

    m = Minimal(None, 3, 1)                   # existing subclasses need nothing new
    with pytest.raises(NotImplementedError):
        m.predict_next_state_change(torch.zeros(4), torch.zeros(4, 4))
