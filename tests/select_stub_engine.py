"""CPU stand-in engine for the host-logic tests of ModelConfig.inducing_selection (tests/test_select_host_logic.py): the stand-in
of tests/sparse_stub_engine.py with `select_inducing` added, backed by the numpy restatement of tests/select_inducing_ref.py and
logged like the calls that change the model."""
import numpy as np
import torch

import select_inducing_ref as ref
from sparse_stub_engine import SparseStubEngine


class SelectStubEngine(SparseStubEngine):
    def select_inducing(self, X, M, lengthscales, outputscales, jitter_rel=1e-6):
        X = np.asarray(X, dtype=np.float64)
        ls = np.asarray(lengthscales.detach() if isinstance(lengthscales, torch.Tensor) else lengthscales, dtype=np.float64)
        osc = np.asarray(outputscales.detach() if isinstance(outputscales, torch.Tensor) else outputscales, dtype=np.float64).reshape(-1)
        out = ref.select(X, int(M), ls, osc, float(jitter_rel))
        self.log.append(("select_inducing", X.copy(), int(M), float(jitter_rel), out["idx"].copy()))
        return {"idx": torch.as_tensor(out["idx"], dtype=torch.int32), "Z": torch.as_tensor(X[out["idx"]].copy()),
                "trace": torch.as_tensor(out["trace"])}
