"""Runs of tests/test_gpu_sparse_update_bits.py and of tools/gen_sparse_update_golden.py (which pins their bits): the rank-one
recurrence of a sparse model (csrc/sparse_update.hip) with either sign, through every shape at which its two kernels take another
path.  One function, so that the fixture and the test can never disagree about the inputs; it uses nothing of the engine but
prepare_sparse / sparse_append / sparse_forget / factors / predict.

  append cases of tests/sparse_append_ref.py   build on the first N0 rows, append the others in one call
  forget cases of tests/sparse_forget_ref.py   build on the whole memory, forget the rows `gone` in one call
  window                                        sparse_forget_ref.sliding_window(): append and forget alternating, 8 steps, on one
                                                handle -- where a vector left in the shared scratch block by the other call would show
  lost_pivot                                    sparse_forget_ref.lost_pivot_setup(): code and text of the error, then prepare_sparse
                                                and the forget of `m1-1` on the same handle
  m961, m1700                                   D = 1; M = 961: 16 column tiles and one row group (the other branch of the group
                                                rule); M = 1700: the vectors kernel needs more than 64 KiB of LDS (both
                                                instantiations go through the raised limit).  One append, then one forget of a row
                                                that is in the model.

Per run: beta_eff (D, M), predict's mean and variance at the case's queries, and the SHA-256 of the bytes of iK_eff (D, M, M)."""
import hashlib

import numpy as np

import sparse_append_ref as ar
import sparse_forget_ref as fr
import sparse_gp_ref as ref

APPEND = ["m1", "n37_m16_29+8", "n150_m130", "d1", "d16_e20"]
FORGET = ["m1-1", "n37_m16-scattered", "n257_m70-64", "n150_m130-10", "d1-8", "d16_e20-8"]
LARGE = {"m961": 961, "m1700": 1700}                     # name -> M; D = 1
RUNS = (["append/" + n for n in APPEND] + ["forget/" + n for n in FORGET] + ["window", "lost_pivot"] + ["large/" + n for n in LARGE])
FIELDS = ("beta", "mean", "var", "iK_sha256")

LARGE_E = 4
LARGE_EXTRA = 20                                         # memory points beside the M that Z is strided over
LARGE_LS = 0.12                                          # about the spacing of 1000-2000 uniform points in [0, 1]^4: k(Z, Z) stays well conditioned


class Case:
    pass


def large_case(name):
    """Inputs of a large-M run: N = M + 20 uniform points in [0, 1]^4, Z strided over them, one output.  The model is built on all
    rows but the last, the last row is appended, then row 0 (= Z[0], in the model) is forgotten."""
    M = LARGE[name]
    c = Case()
    c.name, c.M, c.D, c.E, c.N = name, M, 1, LARGE_E, M + LARGE_EXTRA
    rng = np.random.default_rng(3000 + M)
    c.X = rng.uniform(0.0, 1.0, size=(c.N, c.E))
    c.Xq = rng.uniform(0.0, 1.0, size=(ref.N_QUERIES, c.E))
    c.ls = np.full((1, c.E), LARGE_LS)
    c.os = np.array([1.0])
    c.nz = np.full(1, ref.NOISE)
    c.Y = (np.sin(3.0 * c.X[:, 0]) + c.X[:, 1] * c.X[:, 2])[:, None] + np.sqrt(ref.NOISE) * rng.standard_normal((c.N, 1))
    c.Z = c.X[ref.strided_rows(c.N - 1, M)].copy()
    return c


def _state(engine, c):
    iK, beta = engine.factors()
    out = engine.predict(c.Xq)
    iK = np.ascontiguousarray(iK.cpu().numpy())
    return {"beta": beta.cpu().numpy().copy(), "mean": out["mean"].cpu().numpy().copy(), "var": out["var"].cpu().numpy().copy(),
            "iK_sha256": np.array(hashlib.sha256(iK.tobytes()).hexdigest())}


def _prepare(engine, c, rows):
    engine.prepare_sparse(c.X[rows], c.Y[rows], c.Z, c.ls, c.os, c.nz, ref.JITTER_REL)


def _forget_case(engine, name):
    c = fr.case(name)
    _prepare(engine, c, slice(None))
    engine.sparse_forget(c.X[c.gone], c.Y[c.gone])
    return _state(engine, c)


def run_all(engine):
    """Every run of RUNS on `engine`: {run: {field: numpy array}}; "lost_pivot" carries "code" and "message" besides."""
    out = {}
    for name in APPEND:
        c = ar.case(name)
        _prepare(engine, c, slice(0, c.N0))
        engine.sparse_append(c.X[c.N0:], c.Y[c.N0:])
        out["append/" + name] = _state(engine, c)
    for name in FORGET:
        out["forget/" + name] = _forget_case(engine, name)
    c = fr.sliding_window()
    _prepare(engine, c, slice(0, c.n0))
    for s in range(c.steps):
        engine.sparse_append(c.X[c.n0 + s:c.n0 + s + 1], c.Y[c.n0 + s:c.n0 + s + 1])
        engine.sparse_forget(c.X[s:s + 1], c.Y[s:s + 1])
    out["window"] = _state(engine, c)
    m1, built_on, gone = fr.lost_pivot_setup()
    _prepare(engine, m1, built_on)
    try:
        engine.sparse_forget(m1.X[gone], m1.Y[gone])
        code, message = 0, ""
    except Exception as e:                                   # GpmpcError: .code and the text of gpmpc_last_error
        code, message = int(getattr(e, "code", 1)), str(e)
    out["lost_pivot"] = dict(_forget_case(engine, "m1-1"), code=np.array(code), message=np.array(message))
    for name in LARGE:
        c = large_case(name)
        _prepare(engine, c, slice(0, c.N - 1))
        engine.sparse_append(c.X[c.N - 1:], c.Y[c.N - 1:])
        engine.sparse_forget(c.X[:1], c.Y[:1])
        out["large/" + name] = _state(engine, c)
    return out
