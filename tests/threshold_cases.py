"""Case tables for the threshold statistics (K10 trail_min_max, K11
windowed_quantile, K12 row_quantile), shared by the CPU oracle
validation (test_threshold_oracle.py) and the device tests
(test_threshold_kernels_gpu.py).

Every builder is seeded and returns ``(names, X)``: fp32 rows stacked
as one ``[R, N]`` matrix, with one name per row for failure messages.
"""
import math

import numpy as np

NAN = np.float32(np.nan)

# ---------------------------------------------------------------------------
# K10
# ---------------------------------------------------------------------------
K10_N = (5, 255, 256, 257, 700)
K10_R = 37


def k10_windows(N):
    """w in {1, 2, 6, 144 (where it fits), N}."""
    return sorted({w for w in (1, 2, 6, 144, N) if w <= N})


K10_CASES = [(N, w) for N in K10_N for w in k10_windows(N)]


def _planted(rng, N, w, p):
    """Random row in [0, 1) whose window [p, p+w) alone lies in [5, 6):
    every other window holds a value < 1, so the maximum of minima
    comes from that window only."""
    row = rng.random(N, dtype=np.float32)
    row[p:p + w] = 5 + rng.random(w, dtype=np.float32)
    return row


def planted_nan_row(rng, N, w):
    """A run of w nines with a NaN inside it over a base in [0, 1):
    folding the window with a NaN-ignoring min reports 9 (for w >= 2),
    excluding the window reports a value below 1 (or NaN at w == N)."""
    row = rng.random(N, dtype=np.float32)
    p = (N - w) // 2
    row[p:p + w] = 9.0
    row[p + w // 2] = NAN
    return row


def k10_nan_rows(N, w, seed=0):
    """The NaN-bearing K10 rows."""
    rng = np.random.default_rng([seed, N, w, 10])
    rows = [("planted_nan", planted_nan_row(rng, N, w))]
    r = rng.random(N, dtype=np.float32)
    r[0] = NAN
    rows.append(("nan_first", r))
    r = rng.random(N, dtype=np.float32)
    r[N - 1] = NAN
    rows.append(("nan_last", r))
    r = rng.random(N, dtype=np.float32)
    r[0::w] = NAN  # every window of w holds exactly one of these
    rows.append(("nan_every_w", r))
    rows.append(("all_nan", np.full(N, NAN, dtype=np.float32)))
    # one clean window [p, p+w); a NaN every w positions on both sides
    r = rng.random(N, dtype=np.float32)
    p = (N - w) // 3
    if p >= 1:
        r[p - 1::-w] = NAN
    r[p + w::w] = NAN
    rows.append(("nan_all_but_one", r))
    return rows


def k10_case(N, w, R=K10_R, seed=0):
    rng = np.random.default_rng([seed, N, w, 11])
    rows = [
        ("first_window", _planted(rng, N, w, 0)),
        ("last_window", _planted(rng, N, w, N - w)),
    ]
    if 256 + w <= N:
        # window ending at i = 256 + w - 1: thread 0's second trip
        rows.append(("second_trip", _planted(rng, N, w, 256)))
    rows += k10_nan_rows(N, w, seed)
    rows.append(("all_negative", -1 - rng.random(N, dtype=np.float32)))
    r = rng.random(N, dtype=np.float32)
    r[N // 2] = -np.inf
    rows.append(("has_neg_inf", r))
    rows.append(("all_neg_inf", np.full(N, -np.inf, dtype=np.float32)))
    r = rng.random(N, dtype=np.float32)
    p = min(N - w, N // 4)
    r[p:p + w] = np.inf
    rows.append(("pos_inf_window", r))
    r = rng.random(N, dtype=np.float32)
    r[N // 2] = np.inf
    rows.append(("has_pos_inf", r))
    k = 0
    while len(rows) < R:
        rows.append((f"random{k}",
                     rng.normal(size=N).astype(np.float32)))
        k += 1
    rows = rows[:R]
    return [n for n, _ in rows], np.stack([r for _, r in rows])


# ---------------------------------------------------------------------------
# K11 / K12 row kinds
# ---------------------------------------------------------------------------
K11_W = (1, 2, 3, 7, 8, 144, 256, 257, 300, 1024)
K11_Q = (0.0, 0.25, 0.5, 0.99, 1.0)
K12_N = (1, 2, 3, 255, 256, 257, 4177, 8192, 8193, 16384)
K12_Q = (0.0, 0.1, 0.5, 0.95, 0.99, 1.0)


def k11_lengths(w):
    return (w, w + 1, w + 5)


def step_zeros(n, q):
    """Number of zeros k in a 0/1 multiset of n values such that the
    'linear' position q*(n-1) falls between the last 0 and the first 1
    (order statistics k-1 and k). q in {0, 1} has no interior position
    and uses the q = 0.99 count."""
    if not 0.0 < q < 1.0:
        q = 0.99
    return min(int(math.floor(q * (n - 1))) + 1, n)


def _step_pattern(rng, n, q):
    pat = np.ones(n, dtype=np.float32)
    pat[:step_zeros(n, q)] = 0.0
    rng.shuffle(pat)
    return pat


def _ties(rng, N):
    return rng.choice(np.array([-1.5, 0.25, 3.0], dtype=np.float32), size=N)


def k11_case(w, N, q, seed=0):
    """Two stacks of R = 4 rows. The step row repeats one shuffled
    0/1 pattern with period w, so every window holds the same multiset
    and its q-position falls between a 0 and a 1."""
    rng = np.random.default_rng([seed, w, N, 12])
    a = [
        ("random", rng.random(N, dtype=np.float32)),
        ("ascending", np.sort(rng.random(N, dtype=np.float32))),
        ("descending", np.sort(rng.random(N, dtype=np.float32))[::-1]),
        ("ties", _ties(rng, N)),
    ]
    pat = _step_pattern(rng, w, q)
    nf = rng.random(N, dtype=np.float32)
    nf[0] = NAN
    nl = rng.random(N, dtype=np.float32)
    nl[N - 1] = NAN
    b = [
        ("constant", np.full(N, 0.7, dtype=np.float32)),
        ("step", np.resize(pat, N)),
        ("nan_first", nf),
        ("nan_last", nl),
    ]
    return [
        ([n for n, _ in s], np.stack([r for _, r in s])) for s in (a, b)
    ]


def k11_big_case(seed=0, w=8192):
    """w = N = 8192, R = 2: a random row and a step row (q = 0.99)."""
    rng = np.random.default_rng([seed, w, 13])
    return ["random", "step"], np.stack([
        rng.random(w, dtype=np.float32), _step_pattern(rng, w, 0.99),
    ])


def k12_case(N, q, seed=0):
    """All K12 row kinds at one N as one [R, N] matrix."""
    rng = np.random.default_rng([seed, N, 14])

    def rnd():
        return rng.random(N, dtype=np.float32)

    rows = [
        ("random", rnd()),
        ("ascending", np.sort(rnd())),
        ("descending", np.sort(rnd())[::-1]),
        ("ties", _ties(rng, N)),
        ("constant", np.full(N, 0.7, dtype=np.float32)),
        ("step", _step_pattern(rng, N, q)),
    ]
    r = rnd()
    r[0] = NAN
    rows.append(("nan_first", r))
    r = rnd()
    r[N - 1] = NAN
    rows.append(("nan_last", r))
    r = rnd()
    r[int(rng.integers(N))] = NAN
    rows.append(("one_nan", r))
    r = np.full(N, NAN, dtype=np.float32)
    r[int(rng.integers(N))] = 0.3125
    rows.append(("one_valid", r))
    rows.append(("all_nan", np.full(N, NAN, dtype=np.float32)))
    r = rnd()
    r[:max(1, N // 5)] = NAN
    rows.append(("nan_head_run", r))
    r = rnd()
    r[N - max(1, N // 5):] = NAN
    rows.append(("nan_tail_run", r))
    r = rnd()
    r[::3] = NAN
    rows.append(("nan_every_third", r))
    # a step among NaNs: the valid count, not N, sets the position
    r = np.full(N, NAN, dtype=np.float32)
    nv = N - N // 3
    r[rng.permutation(N)[:nv]] = _step_pattern(rng, nv, q)
    rows.append(("step_with_nan", r))
    return [n for n, _ in rows], np.stack([r for _, r in rows])


def interp_bound(s_lo, s_hi, q):
    """Per-output bound for the fp32 interpolation
    ``s_lo + (s_hi - s_lo) * frac`` against the fp64 oracle on the same
    fp32 inputs: the subtract, the rounding of frac, the multiply and
    the add each contribute at most 2^-24 relative to an operand no
    larger than 2 * max(|s_lo|, |s_hi|), so 2^-21 * max covers them.
    Zero (exact equality) where nothing is interpolated: equal
    neighbours (constant rows, ties, w = 1) and q in {0, 1}, where
    frac is 0 and the expression returns s_lo itself."""
    bound = 2.0 ** -21 * np.maximum(np.abs(s_lo), np.abs(s_hi))
    if q in (0.0, 1.0):
        return np.zeros_like(bound)
    return np.where(s_lo == s_hi, 0.0, bound)
