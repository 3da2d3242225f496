"""Tier 2 (GPU): gpmpc_mll_batch (csrc/mll_batch.hip) -- the training loss and gradient of R hyper-parameter sets per GP in one
launch, left on the device -- against oracle.gp_training.neg_mll_and_grad, with the tolerances test_gpu_parity.py states for
gpmpc_mll: 1e-9 relative on the loss, 1e-7 on the gradient.  That tolerance is stated for cond(K + noise I) <= 1e6, so every
parameter row used here is checked against that bound on the CPU first (asserted, never skipped).

Parameter rows: the workload's hyper-parameters scaled by seeded factors, lengthscales and outputscale by U[0.8, 1.25], the noise
by U[2, 4] (cond ~ lambda_max / noise: with U[1, 2] the worst row over N = 1 .. 256 came to 9.4e5).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import train_device_ref as tref
from helpers import rel_err
from oracle import synth

pytestmark = pytest.mark.gpu

LD = np.longdouble
COND_MAX = 1e6
# (N, D, A, time, R): the panel (32), wavefront (64) and size (1, 256) limits of the kernel; E = 5 with the time column; the
# compiled limits D = 16, E = 24; a single problem
SHAPES = [(N, 3, 1, False, 3) for N in (1, 2, 31, 32, 33, 64, 65, 200, 256)] + [(65, 3, 1, True, 3), (40, 16, 8, False, 2),
                                                                                 (33, 1, 1, False, 1)]


@pytest.fixture(scope="module")
def engine():
    import gp_mpc_amd
    eng = gp_mpc_amd.HipEngine(0)
    yield eng
    eng.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items() if isinstance(v, torch.Tensor)}


def kernel_matrix(X, theta):
    E = X.shape[1]
    d = (X[:, None, :] - X[None, :, :]) / theta[:E]
    return theta[E] * np.exp(-0.5 * (d * d).sum(-1)) + theta[E + 1] * np.eye(X.shape[0])


def assert_regime(X, thetas):
    """The precondition of the tolerances: cond(K + noise I) <= 1e6 for every row."""
    worst = max(float(np.linalg.cond(kernel_matrix(X, th))) for th in thetas.reshape(-1, thetas.shape[-1]))
    assert worst <= COND_MAX, f"cond(K) = {worst:.3e} is outside the regime the tolerances are stated for"
    return worst


@functools.lru_cache(maxsize=None)
def case(N, D, A, tm, R):
    """Workload, parameter rows (R, D, n) and the oracle's loss (R, D) and gradient (R, D, n): computed once per shape."""
    w = synth.make_workload(N, D, A, 3, 2, include_time=tm, seed=N)
    E = w.X.shape[1]
    rng = np.random.default_rng(1000 + N)
    base = np.concatenate([w.lengthscales, w.outputscales[:, None], w.noises[:, None]], axis=1)
    f = np.concatenate([rng.uniform(0.8, 1.25, size=(R, D, E + 1)), rng.uniform(2.0, 4.0, size=(R, D, 1))], axis=2)
    thetas = base[None] * f
    assert_regime(w.X, thetas)
    return w, thetas, *oracle_of(w, thetas)


def oracle_of(w, thetas):
    R, D, n = thetas.shape
    loss, grad = np.empty((R, D)), np.empty((R, D, n))
    for r in range(R):
        for a in range(D):
            loss[r, a], grad[r, a] = tref.loss_and_grad_theta(w.X, w.Y[:, a], thetas[r, a])
    return loss, grad


def check_against(out, loss, grad, E, what):
    """The tolerances of test_gpu_parity.test_training_loss_and_gradient, per problem."""
    R, D = loss.shape
    for r in range(R):
        for a in range(D):
            got_l, got_g = out["loss"][r, a], out["grad"][r, a]
            print(f"{what} r={r} a={a}: loss rel {abs(got_l - loss[r, a]) / abs(loss[r, a]):.2e}  d_ls {rel_err(got_g[:E], grad[r, a, :E]):.2e}"
                  f"  d_os {abs(got_g[E] - grad[r, a, E]) / abs(grad[r, a, E]):.2e}  d_nz {abs(got_g[E + 1] - grad[r, a, E + 1]) / abs(grad[r, a, E + 1]):.2e}")
            assert abs(got_l - loss[r, a]) < 1e-9 * abs(loss[r, a]), (what, r, a)
            assert rel_err(got_g[:E], grad[r, a, :E]) < 1e-7, (what, r, a)
            assert abs(got_g[E] - grad[r, a, E]) < 1e-7 * abs(grad[r, a, E]), (what, r, a)
            assert abs(got_g[E + 1] - grad[r, a, E + 1]) < 1e-7 * abs(grad[r, a, E + 1]), (what, r, a)


@pytest.mark.parametrize("N,D,A,tm,R", SHAPES)
def test_loss_and_gradient_against_the_oracle(engine, N, D, A, tm, R):
    w, thetas, loss, grad = case(N, D, A, tm, R)
    E = w.X.shape[1]
    out = host(engine.mll_batch(w.X, w.Y, thetas))
    assert np.all(out["info"] == 0) and same_bits(out["theta"], thetas)
    check_against(out, loss, grad, E, f"mll_batch[N={N},D={D},E={E},R={R}]")
    again = host(engine.mll_batch(w.X, w.Y, thetas))                 # fixed-order sums: a repeated call agrees bit for bit
    for k in ("loss", "grad", "theta"):
        assert same_bits(out[k], again[k]), k


@pytest.mark.parametrize("log_scale", [False, True])
@pytest.mark.parametrize("N,D,A,tm,R", [(65, 3, 1, True, 3), (200, 3, 1, False, 3)])
def test_box_maps_and_their_chain_rule(engine, N, D, A, tm, R, log_scale):
    w, thetas, _, _ = case(N, D, A, tm, R)
    E = w.X.shape[1]
    lo, hi = 0.5 * thetas.min(axis=0), 2.0 * thetas.max(axis=0)
    x = np.clip(tref.box_unmap(thetas, lo[None], hi[None], log_scale), 0.0, 1.0)
    used = tref.box_map(x, lo[None], hi[None], log_scale)            # what the rows become after the round trip through x
    assert_regime(w.X, used)
    out = host(engine.mll_batch(w.X, w.Y, x, lo=lo, hi=hi, log_scale=log_scale))
    exact = tref.box_map(x, lo[None], hi[None], log_scale, dtype=LD)
    ulp = np.spacing(np.abs(used))
    assert np.all(np.abs(out["theta"].astype(LD) - exact) <= 4 * ulp), float(np.max(np.abs(out["theta"].astype(LD) - exact) / ulp))
    # the gradient in x: restated chain x oracle gradient at the theta the device used
    loss, grad = oracle_of(w, out["theta"])
    grad_x = grad * tref.box_chain(out["theta"], lo[None], hi[None], log_scale)
    check_against(out, loss, grad_x, E, f"mll_batch_box[N={N},log={int(log_scale)}]")
    assert np.all(out["info"] == 0)


def test_a_problem_does_not_depend_on_the_batch(engine):
    w, thetas, _, _ = case(65, 3, 1, False, 3)
    D, n = thetas.shape[1:]
    # R identical rows give identical results
    same = host(engine.mll_batch(w.X, w.Y, np.repeat(thetas[:1], 4, axis=0)))
    for r in range(1, 4):
        assert same_bits(same["loss"][r], same["loss"][0]) and same_bits(same["grad"][r], same["grad"][0])
    # a row alone against the same row as number 2 of 5
    rng = np.random.default_rng(5)
    five = thetas[rng.integers(0, 3, size=5)] * rng.uniform(0.95, 1.05, size=(5, D, n))
    five[2] = thetas[1]
    alone, among = host(engine.mll_batch(w.X, w.Y, thetas[1:2])), host(engine.mll_batch(w.X, w.Y, five))
    assert same_bits(alone["loss"][0], among["loss"][2]) and same_bits(alone["grad"][0], among["grad"][2])


def test_results_do_not_depend_on_the_chunk(engine):
    import gp_mpc_amd
    w, thetas, _, _ = case(65, 3, 1, False, 3)                       # P = 9 problems
    whole = host(engine.mll_batch(w.X, w.Y, thetas))
    eng = gp_mpc_amd.HipEngine(0)
    try:
        with pytest.raises(gp_mpc_amd.GpmpcError):
            eng.set_option("mll_batch_chunk", 0)
        eng.set_option("mll_batch_chunk", 4)                         # launches of 4, 4 and 1 problems
        parts = host(eng.mll_batch(w.X, w.Y, thetas))
    finally:
        eng.close()
    for k in ("loss", "grad", "theta", "info"):
        assert np.array_equal(whole[k], parts[k]) and same_bits(whole[k].astype(np.float64), parts[k].astype(np.float64)), k


def test_the_cached_model_is_untouched(engine):
    w = synth.make_workload(N=64, D=3, A=1, H=6, B=16, seed=3)
    engine.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
    engine.set_cost(w.target, w.W, w.W_T, w.kappa)
    before = host(engine.rollout(w.actions, w.mu0, w.S0))
    f_before = [t.cpu().numpy() for t in engine.factors()]
    mode = engine.last_prepare_mode
    other, thetas, _, _ = case(65, 3, 1, True, 3)                    # other data, another input dimension
    engine.mll_batch(other.X, other.Y, thetas)
    assert engine.last_prepare_mode == mode and (engine.N, engine.D, engine.E) == (64, 3, 4)
    after = host(engine.rollout(w.actions, w.mu0, w.S0))
    f_after = [t.cpu().numpy() for t in engine.factors()]
    for k in before:
        assert same_bits(before[k], after[k]), k
    for b, a in zip(f_before, f_after):
        assert same_bits(b, a)


def test_not_positive_definite_is_a_result(engine):
    w, thetas, loss, grad = case(65, 3, 1, False, 3)
    E = w.X.shape[1]
    bad = thetas.copy()
    bad[1, 2, E], bad[1, 2, E + 1] = 0.5, -1.0                       # first pivot 0.5 - 1 < 0
    out, good = host(engine.mll_batch(w.X, w.Y, bad)), host(engine.mll_batch(w.X, w.Y, thetas))
    assert out["loss"][1, 2] == np.inf and np.all(out["grad"][1, 2] == 0.0) and out["info"][1, 2] == 1
    mask = np.ones((3, 3), dtype=bool)
    mask[1, 2] = False
    assert np.all(out["info"][mask] == 0)
    assert same_bits(out["loss"][mask], good["loss"][mask]) and same_bits(out["grad"][mask], good["grad"][mask])
    # a pivot lost further down: duplicated points with a (barely) negative noise
    Xd = np.concatenate([w.X[:40], w.X[:40]])
    Yd = np.concatenate([w.Y[:40], w.Y[:40]])
    th = thetas[:1].copy()
    th[0, :, E + 1] = -1e-9
    lost = host(engine.mll_batch(Xd, Yd, th))
    assert np.all(lost["loss"] == np.inf) and np.all(lost["grad"] == 0.0) and np.all((lost["info"] > 1) & (lost["info"] <= 80))
    # a theta that is not finite
    th = thetas[:1].copy()
    th[0, 0, 0] = np.nan
    nan = host(engine.mll_batch(w.X, w.Y, th))
    assert nan["loss"][0, 0] == np.inf and np.all(nan["grad"][0, 0] == 0.0) and nan["info"][0, 0] == 1
    assert same_bits(nan["loss"][0, 1:], good["loss"][0, 1:])


def test_errors_are_reported_before_anything_is_written(engine):
    from gp_mpc_amd import _lib as L
    w, thetas, _, _ = case(33, 1, 1, False, 1)
    ARG, LIM = L.GPMPC_ERR_ARG, L.GPMPC_ERR_LIMIT
    dev = engine.device
    X = torch.zeros(300 * 25, dtype=torch.float64, device=dev)
    Y = torch.zeros(300 * 17, dtype=torch.float64, device=dev)
    prm = torch.ones(4100 * 27, dtype=torch.float64, device=dev)
    box = torch.ones(17 * 27, dtype=torch.float64, device=dev)

    def call(want, N=33, D=1, E=2, R=1, log_scale=1, X=X, Y=Y, prm=prm, lo=None, hi=None, no_loss=False, no_grad=False):
        outs = [torch.full((4100 * 27,), -7.0, dtype=torch.float64, device=dev) for _ in range(3)]
        info = torch.full((4100,), -7, dtype=torch.int32, device=dev)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
        rc = engine.lib.gpmpc_mll_batch(engine._h, p(X), p(Y), N, D, E, p(prm), R, p(lo), p(hi), log_scale,
                                        None if no_loss else p(outs[0]), None if no_grad else p(outs[1]), p(outs[2]), p(info),
                                        engine._stream())
        torch.cuda.synchronize()
        assert rc == want, (rc, engine.lib.gpmpc_last_error(engine._h))
        assert all(bool((o == -7.0).all()) for o in outs) and bool((info == -7).all())

    call(ARG, X=None)
    call(ARG, Y=None)
    call(ARG, prm=None)
    call(ARG, no_loss=True)
    call(ARG, no_grad=True)
    call(ARG, lo=box)                                                # only one of lo and hi
    call(ARG, hi=box)
    call(ARG, N=0)
    call(ARG, R=0)
    call(ARG, log_scale=2)
    call(ARG, log_scale=-1)
    call(LIM, N=257)
    call(LIM, D=17, E=18)
    call(LIM, E=25)
    call(LIM, D=16, E=17, R=257)                                     # R D = 4112 > 4096
    # the wrapper's own checks
    lo, hi = 0.5 * thetas[0], 2.0 * thetas[0]
    for kw in (dict(lo=lo), dict(hi=hi), dict(lo=hi, hi=lo), dict(lo=-lo, hi=hi, log_scale=True), dict(lo=lo[:, :2], hi=hi[:, :2])):
        with pytest.raises(ValueError):
            engine.mll_batch(w.X, w.Y, thetas, **kw)
    with pytest.raises(ValueError):
        engine.mll_batch(w.X, w.Y, thetas[:, :, :2])
    with pytest.raises(ValueError):
        engine.mll_batch(w.X, w.Y[:5], thetas)
    out = host(engine.mll_batch(w.X, w.Y, thetas))                   # the engine still works
    assert np.all(np.isfinite(out["loss"])) and np.all(out["info"] == 0)
