"""Numpy restatement of the device-resident L-BFGS of csrc/lbfgs_search.hip (gpmpc_lbfgs_init / gpmpc_lbfgs_step): the definition
the kernels are tested against.  TEST CODE ONLY.

Every function takes `dtype` (np.float64, or np.longdouble for the reference the float64 restatement's own error is measured
against).  A state is a dict of arrays with the restart as leading axis, named as HipEngine.lbfgs_state names its views:
    x g d xt actions (B, n) | J alpha status pushes (B) | S Y (B, m, n) | sy yy (B, m)
`pushes` counts the pairs pushed since the last drop: min(pushes, m) are held, the newest in ring slot (pushes - 1) mod m.

`step` also returns, per restart, what happened and how far every decision was from going the other way (relative margins; inf
where a decision is exact, e.g. on a non-finite value or an exact zero):
    branch    'frozen' | 'accept' | 'reject' | 'underflow' | 'converged' | 'nonfinite_start'
    pushed / skipped / reset / dropped_oldest, fixed_lo / fixed_hi (coordinates held at the faces of the box)
    margins   dict(armijo, curvature, descent, pgtol)

A dot product whose exact value is beyond the float64 range is +-inf on the device whatever the summation order; the longdouble
restatement saturates its dot products there too, so that it takes the decisions an exact float64 device would take.
"""
import numpy as np

LD = np.longdouble
F64_MAX = np.finfo(np.float64).max
ALPHA_MIN = 2.0 ** -40
CURVATURE_EPS = 1e-10


def clip01(v):
    """fmin(fmax(v, 0), 1): a NaN becomes 0, as on the device."""
    return np.fmin(np.fmax(v, 0.0), 1.0)


def _sat(v, dtype):
    if dtype is np.float64:
        return v
    if v > F64_MAX:
        return dtype(np.inf)
    if v < -F64_MAX:
        return dtype(-np.inf)
    return v


def _dot(a, b, dtype):
    with np.errstate(over="ignore", invalid="ignore"):
        return _sat(np.sum(a * b, dtype=dtype), dtype)


def to_model(X, H, A, max_change=None, action_prev=None, dtype=np.float64):
    """Optimiser vectors (..., H*A) -> model actions (..., H, A): identity reshape, or the running sum of x 2m - m started at
    action_prev with the OUTPUT clamped, summed in the order of cem_map_kernel (t ascending)."""
    X = np.asarray(X, dtype=dtype)
    lead = X.shape[:-1]
    x = X.reshape(lead + (H, A))
    if max_change is None:
        return x.copy()
    m = np.asarray(max_change, dtype=dtype)
    s = np.broadcast_to(np.asarray(action_prev, dtype=dtype), lead + (A,)).copy()
    out = np.empty_like(x)
    for t in range(H):
        s = s + (x[..., t, :] * dtype(2.0) * m - m)
        out[..., t, :] = clip01(s)
    return out


def chain(G, H, A, max_change=None, dtype=np.float64):
    """dJ/d(model actions) (H, A) -> dJ/d(optimiser vector) (H*A,): identity, or gt[s,a] = 2 m[a] sum_{t>=s} G[t,a] with the sum
    accumulated from the last step backwards (DerivativeActionMapper.chain_grad_model_to_mpc)."""
    G = np.asarray(G, dtype=dtype).reshape(H, A)
    if max_change is None:
        return G.reshape(-1).copy()
    two_m = dtype(2.0) * np.asarray(max_change, dtype=dtype)
    acc = np.zeros(A, dtype=dtype)
    out = np.empty((H, A), dtype=dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(H - 1, -1, -1):
            acc = acc + G[t]
            out[t] = two_m * acc
    return out.reshape(-1)


def init(x0, H, A, history, max_change=None, action_prev=None, dtype=np.float64):
    x0 = np.atleast_2d(np.asarray(x0, dtype=dtype))
    B, n = x0.shape
    assert n == H * A
    z = lambda *sh: np.zeros(sh, dtype=dtype)                    # noqa: E731
    xt = clip01(x0)
    return dict(x=z(B, n), g=z(B, n), d=z(B, n), xt=xt, actions=to_model(xt, H, A, max_change, action_prev, dtype).reshape(B, n),
                J=z(B), alpha=np.ones(B, dtype=dtype), status=z(B), pushes=z(B), S=z(B, history, n), Y=z(B, history, n),
                sy=z(B, history), yy=z(B, history))


def cast(state, dtype):
    return {k: np.array(v, dtype=dtype) for k, v in state.items()}


def _free(x, g):
    lo = (x <= 0.0) & (g > 0.0)
    hi = (x >= 1.0) & (g < 0.0)
    return ~(lo | hi), int(lo.sum()), int(hi.sum())


def _rel(num, den):
    den = abs(den)
    if not np.isfinite(num) or not np.isfinite(den) or den == 0.0:
        return np.inf
    return float(abs(num) / den)


def _step_one(st, b, Jt, Gt, k, H, A, m, c1, pgtol, max_change, action_prev, dtype):
    """One restart, in place.  Follows lbfgs_step_kernel statement by statement."""
    info = dict(branch="frozen", pushed=False, skipped=False, reset=False, dropped_oldest=False, fixed_lo=0, fixed_hi=0,
                margins=dict(armijo=np.inf, curvature=np.inf, descent=np.inf, pgtol=np.inf))
    if st["status"][b] != 0:
        return info
    n = H * A
    x, g, xt = st["x"][b], st["g"][b], st["xt"][b]
    remap = lambda: to_model(st["xt"][b], H, A, max_change, action_prev, dtype).reshape(n)       # noqa: E731
    # 1. chain rule
    gt = chain(Gt, H, A, max_change, dtype)
    # 2. accept or reject
    Jt = dtype(Jt)
    bad = not (np.isfinite(Jt) and np.all(np.isfinite(gt)))
    accept = True
    if k > 0:
        if bad:
            accept = False
        else:
            gs = _dot(g, xt - x, dtype)
            rhs = st["J"][b] + dtype(c1) * gs
            accept = bool(Jt <= rhs)
            info["margins"]["armijo"] = _rel(rhs - Jt, max(abs(st["J"][b]), abs(Jt), abs(dtype(c1) * gs)))
    if not accept:
        # 4. reject
        alpha = st["alpha"][b] * dtype(0.5)
        st["alpha"][b] = alpha
        if alpha < ALPHA_MIN:
            st["status"][b] = 2
            st["xt"][b] = x
            info["branch"] = "underflow"
        else:
            st["xt"][b] = clip01(x + alpha * st["d"][b])
            info["branch"] = "reject"
        st["actions"][b] = remap()
        return info
    # 3. accept
    pushes = int(st["pushes"][b])
    if k > 0:
        s, y = xt - x, gt - g
        sy, ss, yy = _dot(s, y, dtype), _dot(s, s, dtype), _dot(y, y, dtype)
        norms = np.sqrt(ss) * np.sqrt(yy)
        thr = dtype(CURVATURE_EPS) * norms
        info["margins"]["curvature"] = _rel(sy - thr, norms)
        if sy > thr:
            slot = pushes % m
            info["dropped_oldest"] = pushes >= m
            st["S"][b, slot], st["Y"][b, slot], st["sy"][b, slot], st["yy"][b, slot] = s, y, sy, yy
            pushes += 1
            info["pushed"] = True
        else:
            info["skipped"] = True
    st["x"][b], st["g"][b], st["J"][b] = xt.copy(), gt, Jt
    x, g = st["x"][b], st["g"][b]
    if k == 0 and bad:
        st["status"][b] = 3
        info["branch"] = "nonfinite_start"
        return info
    info["branch"] = "accept"
    # 5. new direction
    free, info["fixed_lo"], info["fixed_hi"] = _free(x, g)
    gf = np.where(free, g, dtype(0.0))
    gmax = np.max(np.abs(gf))
    info["margins"]["pgtol"] = _rel(gmax - dtype(pgtol), max(gmax, dtype(pgtol)))
    if gmax <= pgtol:
        st["status"][b] = 1
        st["pushes"][b] = pushes
        info["branch"] = "converged"
        return info
    gg = _dot(gf, gf, dtype)
    held = min(pushes, m)
    q = gf.copy()
    coef = []
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for j in range(held):                                    # newest -> oldest
            slot = (pushes - 1 - j) % m
            aj = _dot(st["S"][b, slot], q, dtype) / st["sy"][b, slot]
            coef.append(aj)
            q = q - aj * st["Y"][b, slot]
        if held > 0:
            newest = (pushes - 1) % m
            gamma = st["sy"][b, newest] / st["yy"][b, newest]
        else:
            gamma = dtype(1.0) / np.sqrt(gg)
        q = q * gamma
        for j in range(held - 1, -1, -1):                        # oldest -> newest
            slot = (pushes - 1 - j) % m
            bj = _dot(st["Y"][b, slot], q, dtype) / st["sy"][b, slot]
            q = q + (coef[j] - bj) * st["S"][b, slot]
        d = np.where(free, -q, dtype(0.0))
        dg = _dot(d, gf, dtype)
        info["margins"]["descent"] = _rel(dg, np.sqrt(_dot(d, d, dtype)) * np.sqrt(gg))
        if not dg < 0.0:                                         # no descent, or NaN
            d = -gf
            pushes = 0
            info["reset"] = True
        st["d"][b] = d
        st["alpha"][b] = 1
        st["pushes"][b] = pushes
        st["xt"][b] = clip01(x + d)
    st["actions"][b] = remap()
    return info


def step(state, Jt, Gt, k, H, A, history, c1, pgtol, max_change=None, action_prev=None, dtype=np.float64):
    """Step k for every restart from (Jt (B), Gt (B, H, A)): returns (new state, list of per-restart info)."""
    st = cast(state, dtype)
    B = st["x"].shape[0]
    Jt = np.asarray(Jt).reshape(B)
    Gt = np.asarray(Gt).reshape(B, H, A)
    infos = [_step_one(st, b, Jt[b], Gt[b], k, H, A, history, c1, pgtol, max_change, action_prev, dtype) for b in range(B)]
    return st, infos


def min_margin(infos, kinds=("armijo", "curvature", "descent")):
    return min([i["margins"][k] for i in infos for k in kinds] + [np.inf])


def search(fun, x0, H, A, iterations, history, c1, pgtol, max_change=None, action_prev=None, dtype=np.float64, first_iteration=0,
           state=None, trace=None):
    """init (first_iteration == 0) + `iterations` x [fun(actions (B, H, A)) -> (J (B), G (B, H, A)); step]: the final state.
    `trace` (a list) receives (k, state copy, infos) after every step."""
    st = init(x0, H, A, history, max_change, action_prev, dtype) if first_iteration == 0 else cast(state, dtype)
    B = st["x"].shape[0]
    for it in range(iterations):
        k = first_iteration + it
        J, G = fun(np.asarray(st["actions"], dtype=np.float64).reshape(B, H, A))
        st, infos = step(st, J, G, k, H, A, history, c1, pgtol, max_change, action_prev, dtype)
        if trace is not None:
            trace.append((k, cast(st, dtype), infos))
    return st


def winner(state):
    """[J | restart | x] by gpmpc_argmin's keep-the-best rule over the restarts' J."""
    J = np.asarray(state["J"], dtype=np.float64)
    best, val = -1, np.inf
    for b, v in enumerate(J):
        if b == 0 and np.isnan(v):
            best, val = 0, v
            break
        if v < val:
            best, val = b, v
    x = np.asarray(state["x"], dtype=np.float64)[max(best, 0)]
    return np.concatenate([[val, float(best)], x])


def search_host(fun, x0, H, A, iterations, history, c1, pgtol, max_change=None, action_prev=None):
    """What HipEngine.lbfgs_search_host returns: (best x, best J, per-restart J, per-restart status)."""
    st = search(fun, x0, H, A, iterations, history, c1, pgtol, max_change, action_prev)
    rec = winner(st)
    return rec[2:].copy(), float(rec[0]), np.array(st["J"], dtype=np.float64), np.array(st["status"], dtype=np.int64)


# -- the hand-made sequences of the CPU and GPU tests ------------------------------------------------------------------------------
def quadratic(n, seed, cond=40.0):
    """(Q, c): f(z) = (z - c)^T Q (z - c) / 2 with condition number `cond`; about a third of the minimiser's coordinates lie
    outside the box on either side."""
    rng = np.random.default_rng(seed)
    U, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = np.geomspace(1.0, cond, n) if n > 1 else np.array([cond])
    Q = (U * ev) @ U.T
    Q = 0.5 * (Q + Q.T)
    c = rng.uniform(-0.4, 1.4, size=n)
    return Q, c


def quad_value(Q, c, z):
    r = np.asarray(z, dtype=np.float64) - c
    return 0.5 * float(r @ Q @ r), Q @ r


def unchain(gt, H, A, max_change=None):
    """A G (H, A) whose chain rule is (up to rounding) gt: the hand-made tests choose gradients in optimiser space."""
    gt = np.asarray(gt, dtype=np.float64).reshape(H, A)
    if max_change is None:
        return gt.copy()
    tail = gt / (2.0 * np.asarray(max_change, dtype=np.float64))
    G = tail.copy()
    G[:-1] -= tail[1:]
    return G


# non-finite starts, one fault each: J = NaN / +inf / -inf beside a finite G, and one NaN / +inf / -inf entry of G beside a finite J
J_START_FAULTS = {"nan_start": np.nan, "posinf_J_start": np.inf, "neginf_J_start": -np.inf}
G_START_FAULTS = {"inf_start": -np.inf, "nan_G_start": np.nan, "posinf_G_start": np.inf}
START_FAULTS = tuple(J_START_FAULTS) + tuple(G_START_FAULTS)
SCRIPTS = ("natural", "events", "overflow") + START_FAULTS
EVENT_REJECTS = (2, 6, 7, 8, 9, 10, 11)      # steps at which "events" must be rejected (2: Armijo; the others: one non-finite value)
SCRIPT_STEPS = 44        # 'overflow' needs 41 rejects after its first step to reach the step underflow


def script_values(script, k, row, Q, c, H, A, max_change=None):
    """(Jt, Gt (H, A)) the hand-made sequence `script` feeds at step k to a restart whose state row is `row` (dict of that
    restart's x, g, xt, J as float64).  The values are a quadratic's at the trial point in OPTIMISER space, replaced where the
    script wants a particular branch."""
    n = H * A
    xt, x, g, J = (np.asarray(row[key], dtype=np.float64) for key in ("xt", "x", "g", "J"))
    f, grad = quad_value(Q, c, xt)
    if script == "natural":
        if k >= 8:                                   # well before the decreases get marginal: a zero gradient ends the restart
            return float(J) - 1.0, np.zeros((H, A))
    elif script == "events":
        if k == 2:                                   # forced reject
            return float(J) + 1.0 + abs(float(J)), unchain(grad, H, A, max_change)
        if k == 4:                                   # accepted, with negative curvature y = -s: the pair is skipped
            return float(J) - 1.0 - abs(float(J)), unchain(g - (xt - x), H, A, max_change)
        if k == 6:
            return np.nan, unchain(grad, H, A, max_change)
        if k == 7:
            G = unchain(grad, H, A, max_change)
            G[H - 1, A - 1] = np.inf
            return f, G
        # single faults, each alone beside finite values: only the finiteness test can reject a lone J = -inf
        if k == 8:
            return -np.inf, unchain(grad, H, A, max_change)
        if k == 9:
            return np.inf, unchain(grad, H, A, max_change)
        if k == 10:
            G = unchain(grad, H, A, max_change)
            G[0, 0] = np.nan
            return f, G
        if k == 11:
            G = unchain(grad, H, A, max_change)
            G[H // 2, 0] = -np.inf
            return f, G
        if k >= 16:
            return float(J) - 1.0, np.zeros((H, A))
    elif script == "overflow":
        if k == 0:                                   # gf.gf overflows: scaling 0, d = 0, d.gf = -0: the non-descent reset
            sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
            return 1.0, unchain(1e200 * sign, H, A, max_change)
    elif script in G_START_FAULTS:
        if k == 0:
            G = unchain(grad, H, A, max_change)
            G[H - 1, 0] = G_START_FAULTS[script]
            return f, G
    elif script in J_START_FAULTS:
        if k == 0:
            return J_START_FAULTS[script], unchain(grad, H, A, max_change)
    return f, unchain(grad, H, A, max_change)


def script_batch(scripts, k, state, Q, c, H, A, max_change=None):
    """(J (B), G (B, H, A)) of step k for restarts running `scripts` (one name per restart) from `state`."""
    B = len(scripts)
    J, G = np.empty(B), np.empty((B, H, A))
    for b, name in enumerate(scripts):
        row = {key: np.asarray(state[key], dtype=np.float64)[b] for key in ("xt", "x", "g", "J")}
        J[b], G[b] = script_values(name, k, row, Q, c, H, A, max_change)
    return J, G


def run_scripts(scripts, x0, Q, c, H, A, history, c1, pgtol, steps=SCRIPT_STEPS, max_change=None, action_prev=None,
                dtype=np.float64):
    """The restatement's own chain under the hand-made sequences: list of (k, state after step k, infos, J fed, G fed)."""
    st = init(x0, H, A, history, max_change, action_prev, dtype)
    trace = []
    for k in range(steps):
        J, G = script_batch(scripts, k, st, Q, c, H, A, max_change)
        st, infos = step(st, J, G, k, H, A, history, c1, pgtol, max_change, action_prev, dtype)
        trace.append((k, st, infos, J, G))
    return trace


# -- the chain on the model (CPU precheck and GPU test share starts and settings) ----------------------------------------------------
CHAIN_SHAPES = [(1, 1, False), (2, 3, False), (3, 4, False), (2, 3, True)]       # (A, H, include_time)
T_CHAIN, M_CHAIN, C1_CHAIN = 6, 3, 1e-4
# An accepted step's decrease is the Armijo decision's margin.  A Newton-like step from a point with |g| = p gains about
# p^2 / (2 lambda) (lambda: the curvature, O(1..10) on this workload, as is |J|), so the margin stays above 1e-6 |J| only while
# p >~ 1.4e-3 sqrt(lambda |J|) ~ 5e-3 .. 1.5e-2: the chain stops a restart (status 1) at 2e-2, before its decisions get marginal.
PGTOL_CHAIN = 2e-2


def chain_starts(A, H, B=65):
    """Rows of one seeded (65, H*A) draw: the start of restart b is the same whatever B."""
    return np.random.default_rng(100 * A + H).uniform(size=(65, H * A))[:B]


def chain_kw(A, deriv):
    return dict(max_change=np.array([0.3, 0.6, 0.45])[:A], action_prev=np.array([0.2, 0.7, 0.5])[:A]) if deriv else {}
