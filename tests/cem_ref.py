"""Plain numpy restatement of the device-resident cross-entropy search (csrc/search.hip), written from its contracts:

    draws      Philox4x32-10, counter = (global candidate * n + coordinate, iteration, 0x243F6A88, 0x9E3779B9), key = the two
               words of the seed; two 53-bit integers x -> u = (x + 0.5) 2^-53 in (0, 1]; iteration 0 uses u0, later iterations
               the Box-Muller normal sqrt(-2 log u0) cos(6.283185307179586 u1)
    sample     iteration 0: the uniforms (global slot 0 = the warm start if there is one); later: clip(mean + std * draw, 0, 1)
               with global slot 0 = the incumbent
    to_model   identity reshape, or scaled deltas + running sum + pass-through clamp
    records    the n_elite best of a slice as rows [J (NaN -> +inf) | global index | vector], ordered by (J, index), padded
               with (+inf, 2147483647, zeros)
    refit      order by (J, global index); mean and population std + 1e-3 of the n_elite leaders, summed in leader order; the
               incumbent is replaced on a strict improvement only, the first iteration always adopts its leader

No torch, no GPU.  `dtype` = np.float64 or np.longdouble: the longdouble forms start from the same float64 inputs (uniforms,
records, state) and are the yardstick the float64 forms and the kernels are measured against.
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0 = np.uint64(0xD2511F53)
PHILOX_M1 = np.uint64(0xCD9E8D57)
PHILOX_W0 = np.uint64(0x9E3779B9)            # key bumps (golden ratio, sqrt(3) - 1)
PHILOX_W1 = np.uint64(0xBB67AE85)
COUNTER_2 = 0x243F6A88
COUNTER_3 = 0x9E3779B9
TWO_PI = 6.283185307179586                  # the constant of the sampler, not a better one
PAD_INDEX = 2147483647
STD_FLOOR = 1e-3


def philox4x32_10(counter4, key2):
    """Philox4x32 with 10 rounds.  counter4: four uint64 arrays (values < 2^32) of one shape, key2: two; returns four."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in counter4)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & M32 for k in key2)
    for _ in range(10):
        p0 = PHILOX_M0 * c0                                       # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = PHILOX_M1 * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32)
        k0 = (k0 + PHILOX_W0) & M32
        k1 = (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def unit_from_53_bits(x):
    """(x + 0.5) 2^-53 in float64, evaluated in that order: x = 0 -> 2^-54, x = 2^53 - 1 -> 1.0 (the sum rounds to 2^53)."""
    return (np.asarray(x, dtype=np.uint64).astype(np.float64) + 0.5) * 2.0 ** -53


def uniform2(seed, idx, it):
    """The sampler's two uniforms of counter `idx` (array) at iteration `it`, float64."""
    idx = np.asarray(idx, dtype=np.uint64)
    seed = int(seed) & (2 ** 64 - 1)
    full = lambda v: np.full(idx.shape, v, dtype=np.uint64)
    c0, c1, c2, c3 = philox4x32_10((idx, full(int(it)), full(COUNTER_2), full(COUNTER_3)),
                                   (full(seed & 0xFFFFFFFF), full(seed >> 32)))
    x0 = (c0 << np.uint64(21)) ^ (c1 >> np.uint64(11))
    x1 = (c2 << np.uint64(21)) ^ (c3 >> np.uint64(11))
    return unit_from_53_bits(x0), unit_from_53_bits(x1)


def draws(seed, it, B_total, n, dtype=np.float64):
    """(B_total, n) draws of iteration `it`: uniforms at 0, standard normals later."""
    idx = np.arange(B_total * n, dtype=np.uint64).reshape(B_total, n)          # global candidate * n + coordinate
    u0, u1 = uniform2(seed, idx, it)
    if it == 0:
        return u0.astype(dtype)
    u0, u1 = u0.astype(dtype), u1.astype(dtype)
    return np.sqrt(dtype(-2.0) * np.log(u0)) * np.cos(dtype(TWO_PI) * u1)


def sample(it, b0, Bl, B_total, n, state, first, noise_or_seed, dtype=np.float64):
    """Optimiser vectors (Bl, n) of the slice [b0, b0 + Bl) at iteration `it`.  state = mean | std | best | best J (read for
    it > 0), first = the warm start or None, noise_or_seed = an (iterations, B_total, n) array of draws or an integer seed."""
    if isinstance(noise_or_seed, np.ndarray):
        d = noise_or_seed[it].astype(dtype)
    else:
        d = draws(noise_or_seed, it, B_total, n, dtype)
    d = d[b0:b0 + Bl]
    if it == 0:
        X = d.copy()
        if first is not None and b0 == 0 and Bl > 0:
            X[0] = np.asarray(first, dtype=np.float64).astype(dtype)
        return X
    state = np.asarray(state, dtype=np.float64)
    mean, std, best = state[:n].astype(dtype), state[n:2 * n].astype(dtype), state[2 * n:3 * n].astype(dtype)
    X = np.clip(mean + std * d, dtype(0.0), dtype(1.0))
    if b0 == 0 and Bl > 0:
        X[0] = best
    return X


def to_model(X, H, A, max_change=None, a_prev=None):
    """Optimiser vectors (B, H*A) -> model actions (B, H, A)."""
    a = np.asarray(X, dtype=np.float64).reshape(-1, H, A)
    if max_change is None:
        return a.copy()
    m = np.asarray(max_change, dtype=np.float64)
    out = np.empty_like(a)
    s = np.broadcast_to(np.asarray(a_prev, dtype=np.float64), (a.shape[0], A)).copy()
    for t in range(H):
        s = s + (a[:, t] * 2.0 * m - m)              # the running sum itself is not clamped
        out[:, t] = np.clip(s, 0.0, 1.0)
    return out


def elite_records(J, X, b0, n_elite):
    """(n_elite, 2 + n) records of a slice whose first candidate has global index b0."""
    J = np.asarray(J, dtype=np.float64).reshape(-1)
    X = np.asarray(X, dtype=np.float64)                           # (Bl, n), Bl = 0 for an empty slice
    assert X.ndim == 2 and X.shape[0] == J.size
    n = X.shape[1]
    Jc = np.where(np.isnan(J), np.inf, J)
    idx = np.arange(J.size)
    order = np.lexsort((idx, Jc))[:n_elite]                       # by J, then by index
    rec = np.zeros((n_elite, n + 2))
    rec[:, 0] = np.inf
    rec[:, 1] = PAD_INDEX
    rec[:order.size, 0] = Jc[order]
    rec[:order.size, 1] = order + b0
    rec[:order.size, 2:] = X[order]
    return rec


def refit(records, n_elite, state_in, first_iteration, dtype=np.float64):
    """state = mean | std | best | best J after a refit on `records` (R, 2 + n)."""
    rec = np.asarray(records, dtype=np.float64)
    n = rec.shape[1] - 2
    order = np.lexsort((rec[:, 1], rec[:, 0]))
    lead = rec[order[:n_elite], 2:].astype(dtype)
    s = np.zeros(n, dtype=dtype)
    for row in lead:                                              # summed in leader order
        s = s + row
    mean = s / dtype(n_elite)
    q = np.zeros(n, dtype=dtype)
    for row in lead:
        q = q + (row - mean) * (row - mean)
    std = np.sqrt(q / dtype(n_elite)) + dtype(STD_FLOOR)
    J_lead = rec[order[0], 0]
    state = np.empty(3 * n + 1, dtype=dtype)
    state[:n], state[n:2 * n] = mean, std
    if first_iteration or J_lead < float(np.asarray(state_in, dtype=np.float64)[3 * n]):
        state[2 * n:3 * n], state[3 * n] = rec[order[0], 2:], J_lead
    else:
        state[2 * n:] = np.asarray(state_in, dtype=np.float64)[2 * n:]
    return state
