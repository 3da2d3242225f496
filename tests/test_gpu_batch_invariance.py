"""Tier 2 (GPU): candidate results across every batch-size dispatch switch of the rollout (csrc/rollout.hip, launch_rollout).

The kernel form of a rollout launch is chosen from the batch it is planned for, in four places, and each choice changes a
summation order (thresholds from the device's CU count, 256 on an MI355X):
  * threads      N <= 64: 1024 threads below 2 x CU candidates, 512 from there, 256 from 8 x CU (the row-chunk length follows
                 the wavefront count where the chunk is not clamped, i.e. without two columns per lane: D > 4);
  * shared CU    64 < N <= 256, D <= 4: from 8 x CU candidates two workgroups of 512 threads share a CU, half the LDS each;
  * tiles        4 D N^2 >= 6e6, D <= 4: from 2 x CU candidates the diagonal pairs take the batch-major tiles (path 2);
  * cooperative  16 ceil(B / 8) <= CU: a cluster of workgroups per candidate with the N-only chunk rule (last_cluster > 1).
Checked here, with the thresholds derived from the device:
  a. each form against the extended-precision oracle (same factors) on both sides of its switch and at B = 1, for a fixed set
     of candidates: the first, the last, and those on either side of a group-of-8, cluster or tile-chunk boundary;
  b. the sharded device search (slices through gpmpc_cem_local, then gpmpc_cem_merge) against gpmpc_cem_search bit for bit at
     populations whose slices sit on the other side of a switch: every slice must plan like the whole population;
  c. one candidate's objective and gradient alone and inside batches on both sides of the switches, bits where one kernel form
     serves both launches and against the numpy adjoint everywhere.
Every test asserts that its switch really was crossed: through last_cluster / last_rollout_path where the form shows there,
otherwise by reproducing the default launch bit for bit with the options that force each side's form (which differ in bits).
"""
import types

import numpy as np
import pytest
import torch

from helpers import rel_err, record
from oracle import adjoint, synth
from oracle import extended_precision as ep
from oracle import gpmpc_oracle as orc

pytestmark = pytest.mark.gpu

LDS_HALF_KB = 80          # half of the 160 KiB a gfx950 workgroup may use: the shared-CU layout's budget


@pytest.fixture(scope="module")
def engine():
    import gp_mpc_amd
    eng = gp_mpc_amd.HipEngine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _coop_last(ncu):
    """Largest batch that still takes the cooperative form: 16 ceil(B / 8) <= CU."""
    return 8 * (ncu // 16)


_MODELS = {}


def _model(engine, N, D, A, H, B, tm, seed=1):
    """Workload + factors formed in longdouble (ep.Factors) and rounded to fp64; the engine gets the fp64 factors and the
    extended-precision oracle the same values widened back, so both evaluate one model and what is compared is the rollout."""
    key = (N, D, A, H, B, tm, seed)
    if key not in _MODELS:
        # (noise variance 1e-3: cond(K) low enough that the fp64 floor of S - M M^T sits well under the tolerances)
        w = synth.make_workload(N, D, A, H, B, include_time=tm, seed=seed, time0=3.0, noise_var=1e-3)
        f = ep.Factors(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
        f64 = types.SimpleNamespace(X=np.asarray(w.X, float), lengthscales=np.asarray(w.lengthscales, float),
                                    variances=np.asarray(w.outputscales, float), iK=np.asarray(f.iK, float),
                                    beta=np.asarray(f.beta, float))
        f.iK, f.beta = ep._ld(f64.iK), ep._ld(f64.beta)
        _MODELS[key] = (w, f, f64, {})
    w, f, f64, cache = _MODELS[key]
    engine.set_factors(w.X, f64.iK, f64.beta, w.lengthscales, w.outputscales)
    engine.set_cost(w.target, w.W, w.W_T, w.kappa)
    return w, f, f64, cache


def _exact(w, f, cache, i):
    """Extended-precision trajectory of candidate i and its objective (stage costs of the exact trajectory, fp64)."""
    if i not in cache:
        mu, Sig = ep.predict_trajectory(f, w.actions[i], w.mu0, w.S0, w.include_time, w.time0)
        mu, Sig = np.asarray(mu, float), np.asarray(Sig, float)
        cm, cv = orc.stage_costs(mu[None], Sig[None], w.actions[i][None], w.target, w.W, w.W_T)
        cache[i] = (mu, Sig, float(orc.lcb_objective(cm, cv, w.kappa)[0]))
    return cache[i]


def _subset(B):
    """First, last, and either side of the boundaries of groups of 8 (cooperative placement), 16 / 64 (tile chunks)."""
    return sorted({i for i in (0, 7, 8, 15, 16, 63, 64, B - 2, B - 1) if 0 <= i < B})


def _check_against_exact(out, w, f, cache, B, tag):
    # Sig: 1e-7, or test_gpu_parity's SIG_TOL of the config-2 / config-4 memories (1e-6) from N = 200 on -- the fp64 floor of the
    # cancellation in S - M M^T grows with cond(K) there, in every form alike
    sig_tol = 1e-6 if w.X.shape[0] >= 200 else 1e-7
    worst = np.zeros(3)
    for i in _subset(B):
        mu, Sig, J = _exact(w, f, cache, i)
        e = np.array([rel_err(out["mu"][i].cpu().numpy(), mu), rel_err(out["Sig"][i].cpu().numpy(), Sig),
                      abs(float(out["J"][i]) - J) / abs(J)])
        assert e[0] < 1e-8 and e[1] < sig_tol and e[2] < 1e-7, (tag, B, i, e)
        worst = np.maximum(worst, e)
    record(f"batch_invariance[{tag},B={B}]", mu_vs_exact=worst[0], Sig_vs_exact=worst[1], J_vs_exact=worst[2])


def _run(engine, acts, w, opts=None):
    for k, v in (opts or {}).items():
        engine.set_option(k, v)
    try:
        out = engine.rollout(acts, w.mu0, w.S0, w.include_time, w.time0)
        form = (engine.last_cluster, engine.last_rollout_path)
    finally:
        for k in (opts or {}):
            engine.set_option(k, 0)
    return out, form


def _same_rows(out, rows, ref):
    """Candidates `rows` of a launch against the launch `ref` of exactly those candidates."""
    idx = torch.as_tensor(rows, device=out["Sig"].device)
    return all(torch.equal(out[k].index_select(0, idx), ref[k]) for k in ("mu", "Sig", "J"))


# ----------------------------------------------------------------------------------------------------- a. forms vs exact
# (label, N, D, A, H, include_time, rule)
FORM_CASES = [
    ("threads_n64_d5", 64, 5, 1, 3, False, "threads"),
    ("threads_n64_d5_time", 64, 5, 1, 3, True, "threads"),
    ("threads_n65_d5", 65, 5, 1, 3, False, "threads_off"),
    ("share_cu_n256_d2", 256, 2, 1, 3, False, "share_cu"),
    ("share_cu_n257_d2", 257, 2, 1, 3, False, "share_cu_off"),
    ("tiles_n620_d4", 620, 4, 1, 2, False, "tiles"),
    ("coop_n200_d3", 200, 3, 1, 3, False, "coop"),
    ("coop_n500_d2_time", 500, 2, 1, 3, True, "coop"),
]


def _batches(rule, ncu):
    """(batch, expected form) pairs: B = 1 and the last / first batch either side of the rule's switch(es)."""
    c = _coop_last(ncu)
    if rule in ("threads", "threads_off"):
        return [1, 2 * ncu - 1, 2 * ncu, 8 * ncu - 1, 8 * ncu]
    if rule in ("share_cu", "share_cu_off"):
        return [1, 8 * ncu - 1, 8 * ncu]
    if rule == "tiles":
        return [1, c, c + 1, 2 * ncu - 1, 2 * ncu]
    return [1, c, c + 1]


def _forcing_options(rule, B, ncu):
    """Options under which a launch of a few candidates takes the form the default dispatch gives a batch of B (plain side)."""
    if rule == "threads":
        return {"cluster": 1, "threads": 1024 if B < 2 * ncu else (512 if B < 8 * ncu else 256)}
    if rule == "share_cu":
        return {"cluster": 1, "threads": 512, "lds_limit_kb": LDS_HALF_KB} if B >= 8 * ncu else {"cluster": 1, "threads": 1024}
    return {"cluster": 1, "threads": 1024}           # *_off: no switch at any batch


@pytest.mark.parametrize("label,N,D,A,H,tm,rule", FORM_CASES, ids=[c[0] for c in FORM_CASES])
def test_each_form_matches_extended_precision_at_its_switch(engine, ncu, label, N, D, A, H, tm, rule):
    Bs = _batches(rule, ncu)
    w, f, _, cache = _model(engine, N, D, A, H, max(Bs), tm)
    acts = torch.as_tensor(w.actions, device=engine.device)
    forms = {}
    outs = {}
    for B in Bs:
        out, form = _run(engine, acts[:B], w)
        forms[B] = form
        _check_against_exact(out, w, f, cache, B, label)
        outs[B] = out
    c = _coop_last(ncu)
    if rule == "coop":
        assert forms[1][0] > 1 and forms[c][0] > 1 and forms[c + 1] == (1, 0), forms
    elif rule == "tiles":
        assert forms[c][1] == 0 and forms[c + 1] == (1, 0) and forms[2 * ncu - 1] == (1, 0) and forms[2 * ncu] == (1, 2), forms
    else:
        # the form does not show in last_cluster / last_rollout_path: each plain-side launch must equal, bit for bit, a launch
        # of its subset under the options that force the form the rule names -- and the forced forms must differ
        plain = [B for B in Bs if forms[B][0] == 1]
        assert all(forms[B] == (1, 0) for B in plain) and len(plain) >= 2, forms
        for B in plain:
            rows = _subset(B)
            opts = _forcing_options(rule, B, ncu)
            ref, _ = _run(engine, acts[rows], w, opts)
            assert _same_rows(outs[B], rows, ref), (label, B, opts)
        if rule in ("threads", "share_cu"):
            # two different forms on the two sides of the switch, told apart by their bits on the same candidates
            rows0 = _subset(plain[0])
            kinds = [_run(engine, acts[rows0], w, _forcing_options(rule, B, ncu))[0] for B in plain]
            assert len({tuple(sorted(_forcing_options(rule, B, ncu).items())) for B in plain}) >= 2
            assert not all(torch.equal(kinds[0]["Sig"], k["Sig"]) for k in kinds[1:]), label
    # the difference between forms, for the record (the project does not promise bits across forms)
    first = outs[Bs[0]]
    for B in Bs[1:]:
        record(f"batch_invariance[{label}]", **{f"Sig_B1_vs_B{B}": rel_err(outs[B]["Sig"][0].cpu().numpy(), first["Sig"][0].cpu().numpy())})


# ----------------------------------------------------------------------------------- b. sharded search vs single launch
def _sharded_cases(ncu):
    c = _coop_last(ncu)
    # (label, N, D, A, H, B_total, cuts, deriv, iterations, n_elite, the slices' own form differs because of ...)
    return [
        ("coop_n200_8x32", 200, 3, 1, 3, 256, tuple(range(0, 257, 32)), False, 3, 12),
        ("coop_n200_uneven_deriv", 200, 3, 1, 3, 256, (0, 1, c, c + 1, 256), True, 3, 12),
        ("tiles_n620_8x256", 620, 4, 1, 2, 2048, tuple(range(0, 2049, 256)), False, 2, 16),
        ("threads_n64_8x512", 64, 5, 1, 3, 4096, tuple(range(0, 4097, 512)), False, 2, 32),
        # (2 x 2048 does not cross on a 256-CU part: both halves already share a CU, so the cut is one candidate short of it)
        ("share_cu_n256_uneven", 256, 2, 1, 3, 4096, (0, 1, 8 * ncu - 1, 4096), True, 2, 32),
    ]


SHARDED_IDS = ["coop_n200_8x32", "coop_n200_uneven_deriv", "tiles_n620_8x256", "threads_n64_8x512", "share_cu_n256_uneven"]


@pytest.mark.parametrize("case", range(len(SHARDED_IDS)), ids=SHARDED_IDS)
def test_sharded_search_reaches_the_single_launch_state_across_switches(engine, ncu, case):
    label, N, D, A, H, Bt, cuts, deriv, iters, n_elite = _sharded_cases(ncu)[case]
    w, _, _, _ = _model(engine, N, D, A, H, Bt, False, seed=5)
    n = H * A
    acts = torch.as_tensor(w.actions, device=engine.device)
    # the switch is crossed: a plain launch of the population and one of some slice take different forms
    _, pop_form = _run(engine, acts, w)
    sizes = sorted({hi - lo for lo, hi in zip(cuts[:-1], cuts[1:]) if hi > lo})
    rule = label.split("_")[0]
    if rule in ("coop", "tiles"):
        slice_forms = {B: _run(engine, acts[:B], w)[1] for B in sizes}
        assert any(fm != pop_form for fm in slice_forms.values()), (pop_form, slice_forms)
    else:
        # (the form does not show: the population's bits and those of a launch of the largest slice under the switch differ)
        small = min(sizes) if rule == "threads" else max(B for B in sizes if B < 8 * ncu)
        idx = torch.as_tensor(_subset(small), device=engine.device)
        pop_out, _ = _run(engine, acts, w)
        small_out, small_form = _run(engine, acts[:small], w)
        assert pop_form == (1, 0) and small_form == (1, 0)
        assert not torch.equal(pop_out["Sig"].index_select(0, idx), small_out["Sig"].index_select(0, idx)), label
    rng = np.random.default_rng(6)
    noise = np.concatenate([rng.uniform(size=(1, Bt, n)), rng.standard_normal((iters - 1, Bt, n))])
    first = rng.uniform(size=n)
    kw = dict(max_change=np.full(A, 0.2), action_prev=np.full(A, 0.5)) if deriv else {}
    slice_took = set()
    for draws in (dict(noise=noise), dict(seed=11)):
        x_ref, J_ref = engine.cem_search(w.mu0, w.S0, Bt, H, A, iters, n_elite, first_candidate=first, **draws, **kw)
        state = torch.zeros(3 * n + 1, dtype=torch.float64, device=engine.device)
        for it in range(iters):
            recs = []
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                recs.append(engine.cem_local(w.mu0, w.S0, Bt, lo, hi - lo, H, A, it, n_elite, state, first_candidate=first,
                                             **draws, **kw))
                if hi > lo:
                    slice_took.add((engine.last_cluster, engine.last_rollout_path))
            engine.cem_merge(torch.cat(recs), n_elite, n, it, state)
        host = state.cpu().numpy()
        assert np.array_equal(host[2 * n:3 * n], x_ref) and host[3 * n] == J_ref, (label, list(draws), host[3 * n] - J_ref)
    assert slice_took == {pop_form}, (label, pop_form, slice_took)          # every slice planned like the population


# ------------------------------------------------------------------------------ c. objective + gradient across switches
GRAD_CASES = [("coop_n200_d3", 200, 3, 1, 4, False), ("tiles_n620_d4", 620, 4, 1, 2, False),
              ("threads_n64_d5_time", 64, 5, 1, 3, True)]


@pytest.mark.parametrize("label,N,D,A,H,tm", GRAD_CASES, ids=[c[0] for c in GRAD_CASES])
def test_objective_and_gradient_across_switches(engine, ncu, label, N, D, A, H, tm):
    """One candidate alone and inside batches on both sides of the switches: J and dJ/du against the numpy adjoint always, and
    bit for bit while both launches take the cooperative forward and the few-candidate moment launch (2 B H <= CUs) -- the
    range the lockstep L-BFGS restarts' promise covers (grad.hip).  Past it the bits change with the batch
    (recorded, not asserted): the forward's form and the moment pass's launch follow the batch."""
    c = _coop_last(ncu)
    if label.startswith("coop"):
        Bs = [2, 8, ncu // (2 * H), c, c + 1]
    elif label.startswith("tiles"):
        Bs = [2, c, c + 1, 2 * ncu - 1, 2 * ncu]
    else:
        Bs = [2, 2 * ncu - 1, 2 * ncu]
    w, _, f64, _ = _model(engine, N, D, A, H, max(Bs), tm, seed=7)
    acts = torch.as_tensor(w.actions, device=engine.device)
    cands = (0, 1)
    alone, alone_form = {}, {}
    for i in cands:
        alone[i] = engine.rollout_grad(acts[i:i + 1], w.mu0, w.S0, w.include_time, w.time0)
        alone_form[i] = (engine.last_cluster, engine.last_rollout_path)
        J0, g0, *_ = adjoint.lcb_and_gradient(f64, w.actions[i], w.mu0, w.S0, w.target, w.W, w.W_T, w.kappa, w.include_time,
                                              w.time0)
        assert abs(float(alone[i]["J"][0]) - J0) < 1e-7 * abs(J0)
        assert rel_err(alone[i]["grad"][0].cpu().numpy(), g0) < 1e-7
        alone[i] = (alone[i], J0, g0)
    forms = {}
    for B in Bs:
        out = engine.rollout_grad(acts[:B], w.mu0, w.S0, w.include_time, w.time0)
        forms[B] = (engine.last_cluster, engine.last_rollout_path)
        for i in cands:
            a, J0, g0 = alone[i]
            assert abs(float(out["J"][i]) - J0) < 1e-7 * abs(J0), (label, B, i)
            assert rel_err(out["grad"][i].cpu().numpy(), g0) < 1e-7, (label, B, i)
            same_bits = torch.equal(out["J"][i], a["J"][0]) and torch.equal(out["grad"][i], a["grad"][0])
            record(f"grad_batch_invariance[{label}]", **{f"bits_equal_alone_vs_B{B}": float(same_bits),
                                                          f"grad_rel_diff_alone_vs_B{B}": rel_err(out["grad"][i].cpu().numpy(),
                                                                                                  a["grad"][0].cpu().numpy())})
            if forms[B][0] > 1 and alone_form[i][0] > 1 and 2 * B * H <= ncu:
                assert same_bits, (label, B, i, forms[B])           # the lockstep restarts' promise (grad.hip)
    if label.startswith("coop"):
        assert alone_form[0][0] > 1 and forms[ncu // (2 * H)][0] > 1 and forms[c][0] > 1 and forms[c + 1] == (1, 0), forms
    elif label.startswith("tiles"):
        assert forms[2 * ncu - 1] == (1, 0) and forms[2 * ncu] == (1, 2), forms
    else:
        assert all(fm == (1, 0) for fm in forms.values()), forms
        lo, _ = _run(engine, acts[:2 * ncu - 1], w)                  # 1024 threads against 512: the forward's bits differ
        hi, _ = _run(engine, acts[:2 * ncu], w)
        assert not torch.equal(lo["Sig"][:8], hi["Sig"][:8]), label
