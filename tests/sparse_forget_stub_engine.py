"""CPU stand-in engine for the host-logic tests of ModelConfig.inducing_forget (tests/test_sparse_forget_host_logic.py): the
stand-in of tests/sparse_append_stub_engine.py with `sparse_forget` added to the log of calls that change the model.  Like its
parents it keeps the EXACT model of the memory -- the tests here are about which call the host makes and with what, not about the
arithmetic (tests/test_sparse_forget_reference.py, tests/test_gpu_sparse_forget.py)."""
import numpy as np

from sparse_append_stub_engine import SparseAppendStubEngine
from sparse_stub_engine import SparseStubEngine


class SparseForgetStubEngine(SparseAppendStubEngine):
    refuse_forget = False            # answer sparse_forget as an engine without a record does
    lose_pivot = False               # answer sparse_forget with a lost pivot: no model and no record afterwards

    def sparse_forget(self, X_old, Y_old):
        from gp_mpc_amd import GpmpcError, _lib
        X_old, Y_old = np.asarray(X_old, dtype=np.float64), np.asarray(Y_old, dtype=np.float64)
        self.log.append(("sparse_forget", X_old.copy(), Y_old.copy()))
        if self.refuse_forget or getattr(self, "_sparse", None) is None or len(X_old) < 1:
            raise GpmpcError(_lib.GPMPC_ERR_ARG, "sparse_forget: the handle holds no record of a gpmpc_prepare_sparse")
        if self.lose_pivot:
            self._sparse = None
            raise _lib.NotPositiveDefiniteError(_lib.GPMPC_ERR_NOT_PD, "sparse_forget: point 0 of the call, output 0: the pivot is lost")
        X, Y, ls, osc, nz = self._sparse
        keep = np.ones(len(X), dtype=bool)
        for x, y in zip(X_old, Y_old):                             # by value: the first row still there that equals (x, y)
            hit = np.flatnonzero(keep & np.all(X == x, axis=1) & np.all(Y == y, axis=1))
            assert hit.size, "sparse_forget of a row that is not in the model"
            keep[hit[0]] = False
        self._sparse[0], self._sparse[1] = X[keep], Y[keep]
        log = self.log
        self.log = []                                              # the exact model of the reduced memory, without a log entry
        SparseStubEngine.prepare(self, self._sparse[0], self._sparse[1], ls, osc, nz)
        self.log = log
        self.last_prepare_mode = 6
