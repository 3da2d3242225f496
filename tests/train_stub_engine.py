"""A stand-in for HipEngine in GpStateTransitionModel.train, without a GPU: it notes how it is called, answers `train_search_host`
from a canned table or from the numpy restatement (tests/train_device_ref.py) and `mll` from the oracle's closed form.
TEST CODE ONLY."""
import importlib

import numpy as np
import torch

import train_device_ref as tref
from oracle import gp_training


def engine_module_of(model_class):
    """The module GpStateTransitionModel.train imports HipEngine from (the package is importable under two names)."""
    return importlib.import_module(model_class.__module__.rsplit(".control_objects", 1)[0] + ".engine")


class StubEngine:
    """`made` collects every instance; class attributes steer the next instances: `answer` (None: the restated search; a callable
    (stub, X, Y, x0, lo, hi) -> dict: canned), `fail` (an exception `train_search_host` raises)."""
    made = []
    answer = None
    fail = None

    def __init__(self, device=None):
        self.device = torch.device("cpu")
        self.calls = []
        self.closed = False
        StubEngine.made.append(self)

    @classmethod
    def reset(cls):
        cls.made, cls.answer, cls.fail = [], None, None

    def close(self):
        self.closed = True

    def train_search_host(self, X, Y, x0, lo, hi, iterations, history=10, c1=1e-4, pgtol=1e-5, log_scale=True):
        X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
        x0, lo, hi = (np.array(v, dtype=np.float64) for v in (x0, lo, hi))
        self.calls.append(("train_search_host", dict(X=X, Y=Y, x0=x0, lo=lo, hi=hi, iterations=iterations, history=history, c1=c1,
                                                     pgtol=pgtol, log_scale=log_scale)))
        if StubEngine.fail is not None:
            raise StubEngine.fail
        if StubEngine.answer is not None:
            return StubEngine.answer(self, X, Y, x0, lo, hi)
        R, D, n = x0.shape
        state, _ = tref.search(X, Y, x0, lo, hi, log_scale, iterations, history, c1, pgtol)
        best = tref.winner(state["J"], state["status"], state["x"], lo, hi, log_scale, D)
        return {"theta": best[:, 3:].copy(), "loss": best[:, 0].copy(), "restart": best[:, 1].astype(np.int64),
                "J": state["J"].reshape(R, D).copy(), "status": state["status"].reshape(R, D).astype(np.int64)}

    def mll(self, X, Y, lengthscales, outputscales, noises):
        X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
        ls, osc, nz = (np.asarray(v, dtype=np.float64) for v in (lengthscales, outputscales, noises))
        self.calls.append(("mll", dict(N=X.shape[0], D=Y.shape[1])))
        D, E = ls.shape
        out = {"loss": np.empty(D), "d_lengthscale": np.empty((D, E)), "d_outputscale": np.empty(D), "d_noise": np.empty(D)}
        for a in range(D):
            out["loss"][a], out["d_lengthscale"][a], out["d_outputscale"][a], out["d_noise"][a] = \
                gp_training.neg_mll_and_grad(X, Y[:, a], ls[a], float(osc[a]), float(nz[a]))
        return out
