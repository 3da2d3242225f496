"""CPU restatement of gpmpc_predict_cov (include/gpmpc.h) in numpy, usable in float64 and longdouble: the joint posterior
covariance of the zero-mean RBF-ARD GPs between query points, from the factors iK the engine holds -- and the same matrix a
second, independent way (Schur complement of the joint prior covariance of memory and queries, no iK)."""
import numpy as np


def _kernel(A, B, ls_a, os_a):
    d = (A[:, None, :] - B[None, :, :]) / ls_a
    return os_a * np.exp(-0.5 * np.sum(d * d, axis=-1))


def closed_form_cov(X, ls, os_, iK, Xa, Xb=None, noises=None, dtype=np.float64):
    """(D, Ma, Mb) t_a(xa_i, xb_j) = k_a(xa_i, xb_j) - k_a(xa_i)^T iK_a k_a(xb_j) (cross form), or with Xb None the joint form
    (D, Ma, Ma): the average of t and its transpose (exactly symmetric), `noises` (D,) added to the diagonal."""
    joint = Xb is None
    if not joint and noises is not None:
        raise ValueError("the cross form takes no noise")
    X, ls, os_, Xa = (np.asarray(v, dtype=dtype) for v in (X, ls, os_, Xa))
    Xb = Xa if joint else np.asarray(Xb, dtype=dtype)
    D = ls.shape[0]
    out = np.empty((D, Xa.shape[0], Xb.shape[0]), dtype=dtype)
    for a in range(D):
        ka = _kernel(Xa, X, ls[a], os_[a])
        kb = ka if joint else _kernel(Xb, X, ls[a], os_[a])
        t = _kernel(Xa, Xb, ls[a], os_[a]) - (ka @ np.asarray(iK[a], dtype=dtype)) @ kb.T
        if joint:
            t = 0.5 * (t + t.T)
            if noises is not None:
                t[np.diag_indices_from(t)] += np.asarray(noises, dtype=dtype)[a]
        out[a] = t
    return out


def schur_cov(X, ls, os_, model_noises, Xq):
    """Joint form without iK: K(Xq, Xq) - K(Xq, X) solve(K(X, X) + noise I, K(X, Xq)) per output, numpy fp64."""
    D = ls.shape[0]
    out = np.empty((D, Xq.shape[0], Xq.shape[0]))
    for a in range(D):
        K = _kernel(X, X, ls[a], os_[a]) + model_noises[a] * np.eye(X.shape[0])
        kq = _kernel(Xq, X, ls[a], os_[a])
        t = _kernel(Xq, Xq, ls[a], os_[a]) - kq @ np.linalg.solve(K, kq.T)
        out[a] = 0.5 * (t + t.T)
    return out
