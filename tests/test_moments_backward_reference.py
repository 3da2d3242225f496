"""Tier 1 (CPU): gradients of moment matching, pinned to the reference's own autograd independently of autograd.

tests/golden/moments_grad_full_var*.npz hold torch autograd through the reference's predict_next_state_change
(gp_model.py:112-180) at the 24 inputs of moments_full_var*.npz, for three upstream sets each (tools/gen_golden_moments_grad.py):
the raw mu_bar and covariance gradient G.  Contracted with random directions, mu_bar and sym(G) must give the longdouble central
differences of oracle.extended_precision.moment_match_step.  Only the symmetric part of G is a gradient of a covariance: the
reference's formula is not symmetric in Sigma off symmetric matrices, so G itself is not symmetric.
"""
import numpy as np
import pytest

from helpers import load
from moments_fd import xfactors, directional, directions

GOLDENS = ["moments_full_var", "moments_full_var_time"]


def _sym(G):
    return 0.5 * (G + np.swapaxes(G, -1, -2))


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_covers_kinds_and_upstream_sets(name):
    g, gg = load(name), load(name.replace("moments_", "moments_grad_"))
    assert np.array_equal(g["in_mean"], gg["in_mean"]) and np.array_equal(g["in_var"], gg["in_var"])
    assert set(gg["kind"].tolist()) == {0, 1, 2, 3, 4}                  # dense, action block, time only, zero, wide
    P, E = gg["in_mean"].shape
    D = g["M"].shape[1]
    assert gg["mu_bar"].shape == (3, P, E) and gg["G"].shape == (3, P, E, E)
    # set 0: all of M_bar, S_bar, V_bar; set 1: M_bar and V_bar only; set 2: S_bar only
    assert np.all(gg["M_bar"][:2] != 0) and np.all(gg["S_bar"][0] != 0) and np.all(gg["V_bar"][:2] != 0)
    assert np.all(gg["S_bar"][1] == 0) and np.all(gg["M_bar"][2] == 0) and np.all(gg["V_bar"][2] == 0)
    assert np.all(gg["S_bar"][2] != 0) and gg["V_bar"].shape == (3, P, E, D)
    # the raw autograd gradient is not symmetric: the reason the library returns sym(G)
    G = gg["G"][0][gg["kind"] == 0]
    assert np.abs(G - np.swapaxes(G, -1, -2)).max() > 1e-3 * np.abs(G).max()


@pytest.mark.parametrize("name", GOLDENS)
@pytest.mark.parametrize("up", [0, 1, 2])
def test_gradients_match_longdouble_differences(name, up):
    g, gg = load(name), load(name.replace("moments_", "moments_grad_"))
    f = xfactors(g["X"], g["lengthscales"], g["outputscales"], g["iK"], g["beta"])
    ls = g["lengthscales"].min(axis=0)
    E = ls.shape[0]
    rng = np.random.default_rng(100 + up)
    rows = []
    for p in range(24):
        m, s = gg["in_mean"][p], gg["in_var"][p]
        Mb, Sb, Vb = gg["M_bar"][up, p], gg["S_bar"][up, p], gg["V_bar"][up, p]
        dm, ds = directions(E, ls, rng)
        fd_m = directional(f, m, s, Mb, Sb, Vb, dm, 0 * ds, 1e-6)
        fd_s = directional(f, m, s, Mb, Sb, Vb, 0 * dm, ds, 1e-6)
        an_m = float(gg["mu_bar"][up, p] @ dm)
        an_s = float((_sym(gg["G"][up, p]) * ds).sum())
        an_raw = float((gg["G"][up, p] * ds).sum())
        # the scale of the terms summed: |mu_bar| |dm|, |G| |ds|
        sc_m = float(np.abs(gg["mu_bar"][up, p]) @ np.abs(dm))
        sc_s = float((np.abs(gg["G"][up, p]) * np.abs(ds)).sum())
        rows.append((p, an_m, fd_m, sc_m, an_s, fd_s, sc_s))
        assert an_raw == pytest.approx(an_s, rel=1e-9, abs=1e-12)      # <G, ds> = <sym(G), ds> for symmetric ds
    # on the scale of the file's largest terms: the reference's own fp64 sums lose digits where S's terms cancel (Sigma = 0)
    top_m, top_s = max(r[3] for r in rows), max(r[6] for r in rows)
    for p, an_m, fd_m, sc_m, an_s, fd_s, sc_s in rows:
        assert abs(an_m - fd_m) <= 1e-6 * sc_m + 1e-7 * top_m, (p, gg["kind"][p], an_m, fd_m)
        assert abs(an_s - fd_s) <= 1e-6 * sc_s + 1e-7 * top_s, (p, gg["kind"][p], an_s, fd_s)
