"""CPU stand-in engine for the host-logic tests of the sparse model option (tests/test_sparse_host_logic.py): the stand-in of
tests/stub_engine.py with `prepare_sparse` and `forget` added and a log of the calls that change the model.  Its `prepare_sparse`
keeps the EXACT model of (X, Y) -- the tests here are about which call the host makes and with what, not about the sparse
arithmetic (tests/test_sparse_reference.py, tests/test_gpu_prepare_sparse.py)."""
import numpy as np

from oracle import gpmpc_oracle as orc
from stub_engine import OracleEngine


class SparseStubEngine(OracleEngine):
    last_prepare_mode = 0

    def __init__(self):
        super().__init__()
        self.log = []

    def prepare(self, X, Y, lengthscales, outputscales, noises):
        self.log.append(("prepare", np.asarray(X, dtype=np.float64).copy()))
        super().prepare(X, Y, lengthscales, outputscales, noises)
        self.last_prepare_mode = 0

    def prepare_sparse(self, X, Y, Z, lengthscales, outputscales, noises, jitter_rel=1e-6):
        self.log.append(("prepare_sparse", np.asarray(X, dtype=np.float64).copy(), np.asarray(Z, dtype=np.float64).copy(),
                         float(jitter_rel)))
        super().prepare(X, Y, lengthscales, outputscales, noises)
        self.last_prepare_mode = 4

    def forget(self, indices):
        idx = np.asarray(indices).reshape(-1)
        self.log.append(("forget", idx.copy()))
        keep = np.setdiff1d(np.arange(len(self.f.X)), idx)
        self.f = orc.Factors(self.f.X[keep], self.f.Y[keep], self.f.lengthscales, self.f.variances, self.f.noises)
