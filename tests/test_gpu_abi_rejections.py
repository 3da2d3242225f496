"""Every call the host API turns away, with its return code and the exact text of gpmpc_last_error: the query-point
entries (predict*, moments*), the forward and backward rollout entries and gpmpc_set_option.  The table is literal, copied
from csrc/abi.hip as it stood with one checked body per entry point, so that the shared checkers behind these entries answer
every rejected call as before.  Every row returns before anything is launched: the only device work here is one prepare
(N = 8, D = 2, E = 3) and one set_cost (A = 1).

Rows run in the order of their stage: 0 on a fresh handle, 1 after prepare, 2 after set_cost."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu

OK, ARG, LIMIT = 0, -1, -4
BUF = "buf"                  # stands for the scratch device buffer: any non-NULL device pointer
M0, S0, NZ = "mu0", "S0", "noises"   # the host arrays
BIG = (1 << 22) + 1
N_, D_, E_, A_ = 8, 2, 3, 1


# -- the raw calls: keyword arguments override one argument at a time ----------------------------------------------------------
def predict(c, Xq=BUF, M=3, D=2, E=3, nz=None, mean=BUF, var=BUF):
    return c.lib.gpmpc_predict(c.h, c.a(Xq), M, D, E, c.a(nz), c.a(mean), c.a(var), c.s)


def predict_backward(c, Xq=BUF, M=3, D=2, E=3, mean_bar=BUF, var_bar=BUF, out=BUF):
    return c.lib.gpmpc_predict_backward(c.h, c.a(Xq), M, D, E, c.a(mean_bar), c.a(var_bar), c.a(out), c.s)


def predict_cov(c, Xa=BUF, Ma=3, Xb=None, Mb=0, D=2, E=3, nz=None, out=BUF):
    return c.lib.gpmpc_predict_cov(c.h, c.a(Xa), Ma, c.a(Xb), Mb, D, E, c.a(nz), c.a(out), c.s)


def _moments(fn):
    def call(c, mu=BUF, var=BUF, P=3, D=2, E=3, M_out=BUF, S_out=BUF, V_out=BUF):
        return getattr(c.lib, fn)(c.h, c.a(mu), c.a(var), P, D, E, c.a(M_out), c.a(S_out), c.a(V_out), c.s)
    return call


def _moments_backward(fn):
    def call(c, mu=BUF, var=BUF, P=3, D=2, E=3, M_bar=BUF, S_bar=BUF, V_bar=BUF, mu_bar=BUF, var_bar=BUF):
        return getattr(c.lib, fn)(c.h, c.a(mu), c.a(var), P, D, E, c.a(M_bar), c.a(S_bar), c.a(V_bar), c.a(mu_bar), c.a(var_bar), c.s)
    return call


def _rollout(fn, feedback=False):
    def call(c, actions=BUF, gains=BUF, per=0, m0=M0, S=S0, B=2, H=3, A=1, time=0, mu=BUF, Sig=BUF, cm=None, cv=None, J=None):
        g = (c.a(gains), per) if feedback else ()
        return getattr(c.lib, fn)(c.h, c.a(actions), *g, c.a(m0), c.a(S), B, H, A, time, 0.0, c.a(mu), c.a(Sig), c.a(cm), c.a(cv),
                                  c.a(J), c.s)
    return call


def _rollout_backward(fn, feedback=False):
    def call(c, actions=BUF, gains=BUF, per=0, m0=M0, S=S0, B=2, H=3, A=1, time=0, mu_bar=BUF, Sig_bar=None, cm_bar=None,
             cv_bar=None, J_bar=None, out=BUF, gains_bar=None, mu0_bar=None, S0_bar=None):
        g = (c.a(gains), per) if feedback else ()
        gb = (c.a(gains_bar),) if feedback else ()
        return getattr(c.lib, fn)(c.h, c.a(actions), *g, c.a(m0), c.a(S), B, H, A, time, 0.0, c.a(mu_bar), c.a(Sig_bar), c.a(cm_bar),
                                  c.a(cv_bar), c.a(J_bar), c.a(out), *gb, c.a(mu0_bar), c.a(S0_bar), c.s)
    return call


def set_option(c, name, value):
    return c.lib.gpmpc_set_option(c.h, name.encode() if name is not None else None, value)


CALLS = {
    "predict": predict, "predict_backward": predict_backward, "predict_cov": predict_cov,
    "moments": _moments("gpmpc_moments"), "moments_linear": _moments("gpmpc_moments_linear"),
    "moments_backward": _moments_backward("gpmpc_moments_backward"),
    "moments_linear_backward": _moments_backward("gpmpc_moments_linear_backward"),
    "rollout": _rollout("gpmpc_rollout"), "rollout_linear": _rollout("gpmpc_rollout_linear"),
    "rollout_linear_feedback": _rollout("gpmpc_rollout_linear_feedback", True),
    "rollout_backward": _rollout_backward("gpmpc_rollout_backward"),
    "rollout_linear_backward": _rollout_backward("gpmpc_rollout_linear_backward"),
    "rollout_linear_feedback_backward": _rollout_backward("gpmpc_rollout_linear_feedback_backward", True),
}

NULL = "null argument"
NO_MODEL = "rollout before prepare / set_factors"
SHAPE = "need B >= 1, H >= 1"
DIMS = "D + A (+1 with time) must equal the model's input dim E"
NO_COST = "gpmpc_set_cost not called for this (D, A)"
GRAD_A = "gradient needs A >= 1"

# (entry, stage, keyword arguments, return code, gpmpc_last_error)
ROWS = [
    # -- gpmpc_predict: no compiled-limit check, D = 17 is a mismatch -----------------------------------------------------------
    ("predict", 0, {}, ARG, "predict before prepare / set_factors / mll"),
    ("predict", 1, dict(D=3), ARG, "predict: D / E differ from the cached model"),
    ("predict", 1, dict(E=4), ARG, "predict: D / E differ from the cached model"),
    ("predict", 1, dict(D=17), ARG, "predict: D / E differ from the cached model"),
    ("predict", 1, dict(E=25), ARG, "predict: D / E differ from the cached model"),
    ("predict", 1, dict(M=-1), ARG, "predict: M < 0"),
    ("predict", 1, dict(Xq=None), ARG, NULL),
    ("predict", 1, dict(M=0), OK, None),
    ("predict", 1, dict(M=0, Xq=None), OK, None),
    ("predict_backward", 0, {}, ARG, "predict_backward before prepare / set_factors / mll"),
    ("predict_backward", 1, dict(D=3), ARG, "predict_backward: D / E differ from the cached model"),
    ("predict_backward", 1, dict(E=4), ARG, "predict_backward: D / E differ from the cached model"),
    ("predict_backward", 1, dict(D=17), ARG, "predict_backward: D / E differ from the cached model"),
    ("predict_backward", 1, dict(M=-1), ARG, "predict_backward: M < 0"),
    ("predict_backward", 1, dict(Xq=None), ARG, NULL),
    ("predict_backward", 1, dict(out=None), ARG, NULL),
    ("predict_backward", 1, dict(M=0), OK, None),
    ("predict_backward", 1, dict(M=0, Xq=None, out=None), OK, None),
    ("predict_cov", 0, {}, ARG, "predict_cov before prepare / set_factors / mll"),
    ("predict_cov", 1, dict(D=3), ARG, "predict_cov: D / E differ from the cached model"),
    ("predict_cov", 1, dict(E=4), ARG, "predict_cov: D / E differ from the cached model"),
    ("predict_cov", 1, dict(E=25), ARG, "predict_cov: D / E differ from the cached model"),
    ("predict_cov", 1, dict(Ma=-1), ARG, "predict_cov: negative number of points"),
    ("predict_cov", 1, dict(Xb=BUF, Mb=-1), ARG, "predict_cov: negative number of points"),
    ("predict_cov", 1, dict(Xb=BUF, Mb=2, nz=NZ), ARG, "predict_cov: the cross form takes no noise"),
    ("predict_cov", 1, dict(Ma=BIG), ARG, "predict_cov: more than 2^22 points"),
    ("predict_cov", 1, dict(Xb=BUF, Mb=BIG), ARG, "predict_cov: more than 2^22 points"),
    ("predict_cov", 1, dict(Ma=-1, Xb=BUF, Mb=BIG, nz=NZ), ARG, "predict_cov: negative number of points"),
    ("predict_cov", 1, dict(Ma=BIG, Xb=BUF, Mb=2, nz=NZ), ARG, "predict_cov: the cross form takes no noise"),
    ("predict_cov", 1, dict(Xa=None), ARG, NULL),
    ("predict_cov", 1, dict(out=None), ARG, NULL),
    ("predict_cov", 1, dict(Xb=BUF, Mb=2, out=None), ARG, NULL),
    ("predict_cov", 1, dict(Ma=0), OK, None),
    ("predict_cov", 1, dict(Ma=0, Xa=None, out=None), OK, None),       # the empty call answers before the pointers are looked at
    ("predict_cov", 1, dict(Xb=BUF, Mb=0), OK, None),
    ("predict_cov", 1, dict(Xb=BUF, Mb=0, Xa=None), OK, None),
]
# -- the moments entries: the compiled limits first, GPMPC_ERR_LIMIT --------------------------------------------------------------
for _e in ("moments", "moments_linear", "moments_backward", "moments_linear_backward"):
    ROWS += [
        (_e, 0, {}, ARG, f"{_e} before prepare / set_factors / mll"),
        (_e, 0, dict(D=17), ARG, f"{_e} before prepare / set_factors / mll"),
        (_e, 1, dict(D=17), LIMIT, f"{_e}: D or E beyond the compiled limits"),
        (_e, 1, dict(E=25), LIMIT, f"{_e}: D or E beyond the compiled limits"),
        (_e, 1, dict(D=17, P=-1, mu=None), LIMIT, f"{_e}: D or E beyond the compiled limits"),
        (_e, 1, dict(D=16), ARG, f"{_e}: D / E differ from the cached model"),
        (_e, 1, dict(D=3), ARG, f"{_e}: D / E differ from the cached model"),
        (_e, 1, dict(E=24), ARG, f"{_e}: D / E differ from the cached model"),
        (_e, 1, dict(E=4, P=-1), ARG, f"{_e}: D / E differ from the cached model"),
        (_e, 1, dict(P=-1), ARG, f"{_e}: P < 0"),
        (_e, 1, dict(P=-1, mu=None), ARG, f"{_e}: P < 0"),
        (_e, 1, dict(mu=None), ARG, NULL),
        (_e, 1, dict(P=0), OK, None),
        (_e, 1, dict(P=0, mu=None), OK, None),
    ]
ROWS += [
    ("moments", 1, dict(M_out=None), ARG, NULL),                        # gpmpc_moments alone needs M_out
    ("moments", 1, dict(P=0, mu=None, M_out=None), OK, None),
]
# -- forward rollouts ---------------------------------------------------------------------------------------------------------------
for _e, _kw in (("rollout", {}), ("rollout_linear", {}), ("rollout_linear_feedback", {}), ("rollout_linear_feedback", dict(gains=None))):
    ROWS += [
        (_e, 0, dict(_kw), ARG, NO_MODEL),
        (_e, 0, dict(_kw, actions=None), ARG, NO_MODEL),
        (_e, 1, dict(_kw, actions=None), ARG, NULL),
        (_e, 1, dict(_kw, m0=None), ARG, NULL),
        (_e, 1, dict(_kw, S=None), ARG, NULL),
        (_e, 1, dict(_kw, B=0), ARG, SHAPE),
        (_e, 1, dict(_kw, H=0), ARG, SHAPE),
        (_e, 1, dict(_kw, A=-1), ARG, SHAPE),
        (_e, 1, dict(_kw, A=2), ARG, DIMS),
        (_e, 1, dict(_kw, time=1), ARG, DIMS),
        (_e, 1, dict(_kw, J=BUF), ARG, NO_COST),
        (_e, 1, dict(_kw, cm=BUF), ARG, NO_COST),
        (_e, 1, dict(_kw, cv=BUF), ARG, NO_COST),
        (_e, 2, dict(_kw, A=0, time=1, J=BUF), ARG, NO_COST),          # the cost is loaded for A = 1
        (_e, 2, dict(_kw, A=2, J=BUF), ARG, DIMS),
    ]
ROWS += [
    ("rollout_linear_feedback", 1, dict(A=0, time=1), ARG, "feedback gains need A >= 1"),
    ("rollout_linear_feedback", 2, dict(A=0, time=1), ARG, "feedback gains need A >= 1"),
    ("rollout_linear_feedback", 1, dict(A=0, time=1, per=1), ARG, "feedback gains need A >= 1"),
    ("rollout_linear_feedback", 1, dict(A=0, time=1, actions=None), ARG, NULL),        # the shared checks come first
    ("rollout_linear_feedback", 1, dict(A=0, time=0), ARG, DIMS),
    ("rollout_linear_feedback", 0, dict(A=0, time=1), ARG, NO_MODEL),
]
# -- backward rollouts --------------------------------------------------------------------------------------------------------------
for _e, _kw in (("rollout_backward", {}), ("rollout_linear_backward", {}), ("rollout_linear_feedback_backward", {}),
                ("rollout_linear_feedback_backward", dict(gains=None))):
    ROWS += [
        (_e, 0, dict(_kw), ARG, NO_MODEL),
        (_e, 0, dict(_kw, out=None), ARG, NULL),                        # the output is looked at before the model
        (_e, 1, dict(_kw, out=None), ARG, NULL),
        (_e, 1, dict(_kw, actions=None), ARG, NULL),
        (_e, 1, dict(_kw, m0=None), ARG, NULL),
        (_e, 1, dict(_kw, S=None), ARG, NULL),
        (_e, 1, dict(_kw, B=0), ARG, SHAPE),
        (_e, 1, dict(_kw, H=0), ARG, SHAPE),
        (_e, 1, dict(_kw, A=-1), ARG, SHAPE),
        (_e, 1, dict(_kw, A=2), ARG, DIMS),
        (_e, 1, dict(_kw, time=1), ARG, DIMS),
        (_e, 1, dict(_kw, J_bar=BUF), ARG, NO_COST),
        (_e, 1, dict(_kw, cm_bar=BUF), ARG, NO_COST),
        (_e, 1, dict(_kw, cv_bar=BUF), ARG, NO_COST),
        (_e, 1, dict(_kw, A=0, time=1), ARG, GRAD_A),
        (_e, 2, dict(_kw, A=0, time=1), ARG, GRAD_A),
        (_e, 1, dict(_kw, A=0, time=1, mu0_bar=BUF, S0_bar=BUF), ARG, GRAD_A),
        (_e, 2, dict(_kw, A=0, time=1, J_bar=BUF), ARG, NO_COST),      # the cost is loaded for A = 1
        (_e, 1, dict(_kw, A=0, time=1, actions=None), ARG, NULL),
    ]
ROWS += [
    ("rollout_linear_feedback_backward", 0, dict(gains=None, gains_bar=BUF), ARG, "gains_bar_out without gains"),
    ("rollout_linear_feedback_backward", 1, dict(gains=None, gains_bar=BUF), ARG, "gains_bar_out without gains"),
    ("rollout_linear_feedback_backward", 2, dict(gains=None, gains_bar=BUF, out=None), ARG, "gains_bar_out without gains"),
    ("rollout_linear_feedback_backward", 1, dict(gains_bar=BUF, A=0, time=1), ARG, GRAD_A),
    ("rollout_linear_feedback_backward", 1, dict(gains_bar=BUF, out=None), ARG, NULL),
]

# -- gpmpc_set_option -------------------------------------------------------------------------------------------------------------------
_T24 = 1 << 24
_M64 = "{}: 0 (auto) or a multiple of 64"
_PTS = "{}: 0 (auto) or a number of points"
CHECKED = {      # name: (message, rejected values, accepted values)
    "grad_chunk_rows": ("grad_chunk_rows: 0 (auto) or a multiple of 4 up to 64", (-1, -4, 65, 68, 1, 2, 62), (0, 4, 64, (1 << 32) + 8)),
    "predict_chunk_rows": (_M64.format("predict_chunk_rows"), (-1, -64, _T24 + 1, _T24 + 64, 1, 63, 1 << 32), (0, 64, _T24)),
    "predict_backward_chunk_rows": (_M64.format("predict_backward_chunk_rows"), (-1, -64, _T24 + 1, _T24 + 64, 1, 63, 1 << 32),
                                    (0, 64, _T24)),
    "predict_cov_chunk_rows": (_M64.format("predict_cov_chunk_rows"), (-1, -64, _T24 + 1, _T24 + 64, 1, 63, 1 << 32), (0, 64, _T24)),
    "sparse_chunk_points": (_M64.format("sparse_chunk_points"), (-1, -64, _T24 + 1, _T24 + 64, 1, 63, 1 << 32), (0, 64, _T24)),
    "moments_chunk_points": (_PTS.format("moments_chunk_points"), (-1, _T24 + 1, 1 << 32), (0, 1, 5, _T24)),
    "moments_backward_chunk_points": (_PTS.format("moments_backward_chunk_points"), (-1, _T24 + 1, 1 << 32), (0, 1, 5, _T24)),
    "moments_linear_chunk_points": (_PTS.format("moments_linear_chunk_points"), (-1, _T24 + 1, 1 << 32), (0, 1, 5, _T24)),
    "moments_linear_backward_chunk_points": (_PTS.format("moments_linear_backward_chunk_points"), (-1, _T24 + 1, 1 << 32),
                                             (0, 1, 5, _T24)),
    "lqr_gains_chunk_points": ("lqr_gains_chunk_points: 0 (auto) or a number of candidates", (-1, _T24 + 1, 1 << 32), (0, 1, 5, _T24)),
    "select_inducing_max_mb": ("select_inducing_max_mb: a number of MiB >= 1", (0, -1, -(1 << 40)), (1, 4096, 1 << 40)),
    "cluster": ("cluster: 0 (auto), 1 (never) or 2..32 workgroups per candidate", (-1, 33, 1 << 32), (0, 1, 2, 32)),
}
UNCHECKED = ["threads", "lds_limit_kb", "force_global_scratch", "rows_per_chunk", "force_path", "force_separable", "cols_per_lane",
             "grad_share_cu", "incremental", "grad_stream", "grad_separable", "grad_tiles", "grad_mean", "prepare_overlap",
             "prepare_fuse", "prepare_invcols", "prepare_inv_batch", "fused_prepare", "gram_shared", "outer_block", "tile128",
             "block128", "outer_min_n", "inner_left", "outer2", "refresh_every", "pair_tiles", "cluster_debug"]
OPTION_ROWS = [("no_such_option", 1, ARG, "unknown option"), ("", 0, ARG, "unknown option"), ("Threads", 0, ARG, "unknown option"),
               ("threads ", 0, ARG, "unknown option"), ("grad_chunk", 4, ARG, "unknown option"), (None, 0, ARG, None)]
for _n, (_msg, _no, _yes) in CHECKED.items():
    OPTION_ROWS += [(_n, _v, ARG, _msg) for _v in _no] + [(_n, _v, OK, None) for _v in _yes]
# the unchecked ones take any value through the (int) cast
OPTION_ROWS += [(_n, _v, OK, None) for _n in UNCHECKED for _v in (1, 0, -1, 1 << 40)]
assert len(CHECKED) == 12 and len(UNCHECKED) + len(CHECKED) == 40      # every name gpmpc_set_option knows


class _Ctx:
    def __init__(self, eng):
        self.eng, self.lib, self.h, self.s = eng, eng.lib, eng._h, eng._stream()
        self.buf = torch.full((4096,), 7.0, dtype=torch.float64, device=eng.device)
        self.host = {M0: np.array([0.1, -0.2]), S0: np.eye(2) * 0.01, NZ: np.array([0.01, 0.02])}

    def a(self, v):
        if v is None or isinstance(v, int):
            return v
        if v == BUF:
            return self.buf.data_ptr()
        return self.host[v].ctypes.data_as(C.c_void_p)

    def err(self):
        return self.lib.gpmpc_last_error(self.h).decode()


@pytest.fixture(scope="module")
def answers():
    """Every row's (return code, gpmpc_last_error), gathered stage by stage on one handle."""
    import gp_mpc_amd
    eng = gp_mpc_amd.HipEngine(0)
    c = _Ctx(eng)
    w = synth.make_workload(N=N_, D=D_, A=A_, H=3, B=2, seed=1)
    got = {}
    for stage in (0, 1, 2):
        if stage == 1:
            eng.prepare(w.X, w.Y, w.lengthscales, w.outputscales, w.noises)
            assert (eng.N, eng.D, eng.E) == (N_, D_, E_)
        if stage == 2:
            eng.set_cost(w.target, w.W, w.W_T, w.kappa)
        for i, (entry, st, kw, _, _) in enumerate(ROWS):
            if st == stage:
                rc = CALLS[entry](c, **kw)
                got[i] = (rc, c.err() if rc != OK else None)
    got["options"] = []
    for name, value, _, _ in OPTION_ROWS:
        rc = set_option(c, name, value)
        got["options"].append((rc, c.err() if rc != OK else None))
    torch.cuda.synchronize()
    got["buf_untouched"] = bool((c.buf == 7.0).all())
    got["null_handle"] = {e: CALLS[e](_NullHandle(c)) for e in CALLS}
    got["null_handle"]["set_option"] = eng.lib.gpmpc_set_option(None, b"threads", 0)
    eng.close()
    return got


class _NullHandle:
    def __init__(self, c):
        self.lib, self.h, self.s, self.a = c.lib, None, c.s, c.a


def _matches(got, rc, text):
    """`text` None: an accepted call, or a rejection that never reaches the handle's message (a NULL name)."""
    return got[0] == rc and (text is None or got[1] == text)


def _row_id(r):
    return f"{r[0]}-s{r[1]}-" + ",".join(f"{k}={v}" for k, v in r[2].items())


@pytest.mark.parametrize("i", range(len(ROWS)), ids=[_row_id(r) for r in ROWS])
def test_rejected_call(i, answers):
    _, _, _, rc, text = ROWS[i]
    print(ROWS[i], "->", answers[i])
    assert _matches(answers[i], rc, text)


def test_options(answers):
    assert len(answers["options"]) == len(OPTION_ROWS)
    wrong = [(row, got) for row, got in zip(OPTION_ROWS, answers["options"]) if not _matches(got, row[2], row[3])]
    assert not wrong, wrong


def test_null_handle_and_outputs_untouched(answers):
    assert answers["null_handle"] == {e: ARG for e in list(CALLS) + ["set_option"]}
    # no row launched or copied anything: the buffer every output pointer named still holds its fill
    assert answers["buf_untouched"]
