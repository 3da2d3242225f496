"""CPU stand-in engine for the host-logic tests of ModelConfig.inducing_refresh_every (tests/test_sparse_append_host_logic.py): the
stand-in of tests/sparse_stub_engine.py with `sparse_append` added to the log of calls that change the model.  Like its parent it
keeps the EXACT model of the memory -- the tests here are about which call the host makes and with what, not about the arithmetic
(tests/test_sparse_append_reference.py, tests/test_gpu_sparse_append.py)."""
import numpy as np

from sparse_stub_engine import SparseStubEngine


class SparseAppendStubEngine(SparseStubEngine):
    refuse_append = False            # answer sparse_append as an engine without a record does

    def prepare(self, X, Y, lengthscales, outputscales, noises):
        super().prepare(X, Y, lengthscales, outputscales, noises)
        self._sparse = None

    def prepare_sparse(self, X, Y, Z, lengthscales, outputscales, noises, jitter_rel=1e-6):
        super().prepare_sparse(X, Y, Z, lengthscales, outputscales, noises, jitter_rel)
        self._sparse = [np.asarray(X, dtype=np.float64).copy(), np.asarray(Y, dtype=np.float64).copy(),
                        np.asarray(lengthscales, dtype=np.float64).copy(), np.asarray(outputscales, dtype=np.float64).copy(),
                        np.asarray(noises, dtype=np.float64).copy()]

    def sparse_append(self, X_new, Y_new):
        from gp_mpc_amd import GpmpcError, _lib
        X_new, Y_new = np.asarray(X_new, dtype=np.float64), np.asarray(Y_new, dtype=np.float64)
        self.log.append(("sparse_append", X_new.copy(), Y_new.copy()))
        if self.refuse_append or getattr(self, "_sparse", None) is None or len(X_new) < 1:
            raise GpmpcError(_lib.GPMPC_ERR_ARG, "sparse_append: the handle holds no record of a gpmpc_prepare_sparse")
        X, Y, ls, osc, nz = self._sparse
        self._sparse[0], self._sparse[1] = np.concatenate([X, X_new]), np.concatenate([Y, Y_new])
        log = self.log
        self.log = []                                              # the exact model of the grown memory, without a log entry
        SparseStubEngine.prepare(self, self._sparse[0], self._sparse[1], ls, osc, nz)
        self.log = log
        self.last_prepare_mode = 5
