"""Longdouble central differences of the moment-matching step (oracle.extended_precision.moment_match_step): the independent
yardstick of the gradient tests (tests/test_moments_backward_reference.py, tests/test_gpu_moments_backward.py)."""
import numpy as np

from oracle import extended_precision as xp

LD = np.longdouble


def xfactors(X, lengthscales, outputscales, iK, beta):
    f = object.__new__(xp.Factors)
    f.X, f.lengthscales, f.variances = xp._ld(X), xp._ld(lengthscales), xp._ld(outputscales)
    f.iK, f.beta = xp._ld(iK), xp._ld(beta)
    return f


def loss(f, m, s, Mb, Sb, Vb):
    """<Mb, M> + <Sb, S> + <Vb, V> in longdouble at one input (m, s)."""
    M, S, V = xp.moment_match_step(f, xp._ld(m), xp._ld(s))
    return (M * xp._ld(Mb)).sum() + (S * xp._ld(Sb)).sum() + (V * xp._ld(Vb)).sum()


def directional(f, m, s, Mb, Sb, Vb, dm, ds, h):
    """Central difference of `loss` along (dm, ds) with step h, in longdouble."""
    m, s, dm, ds = (xp._ld(a) for a in (m, s, dm, ds))
    lp = loss(f, m + LD(h) * dm, s + LD(h) * ds, Mb, Sb, Vb)
    lm = loss(f, m - LD(h) * dm, s - LD(h) * ds, Mb, Sb, Vb)
    return float((lp - lm) / (2 * LD(h)))


def directions(E, ls, rng):
    """A mean direction on the lengthscales' scale and a symmetric covariance direction on their squares."""
    dm = rng.standard_normal(E) * ls
    A = rng.standard_normal((E, E))
    ds = 0.1 * (A + A.T) * np.outer(ls, ls)
    return dm, ds
