"""Case tables for the smoothing op (ops.smooth: smm, sma, ewma;
csrc/smoothing.hip), shared by the CPU oracle validation
(test_smoothing_oracle.py) and the device tests
(test_smoothing_gpu.py).

Inputs are fp32 values built on the CPU; the oracle sees them widened
to fp64. ``case(w, N)`` is seeded and returns ``(names, X)``: R = 37
fp32 rows stacked as one ``[R, N]`` matrix (more rows than one
workgroup has waves) with one name per row for failure messages. Cases
and their oracle values are cached, so every test of a process shares
one copy; they are never written to.
"""
import functools

import numpy as np

from gordo_amd.ops import reference as ref

NAN = np.float32(np.nan)
METHODS = ("smm", "sma", "ewma")
R = 37
WINDOWS = (1, 2, 3, 63, 64, 65, 144, 257)

# the lengths at which the kernels change trips (csrc/smoothing.hip)
SMM_CHUNK = 64    # outputs per wave of smm_slide_kernel
SMA_TILE = 256    # outputs per workgroup of sma_window_kernel
SMA_SEG = 1024    # window positions staged per pass of sma_window_kernel
EWMA_BLOCK = 64   # positions per scan block of ewma_scan_kernel

OUTLIER_AT = 2    # index of the 1e30 value in the outlier row


def lengths(w):
    """N in {w-1 (w > 1), w, w+1, w+63, w+64, w+65, 700} plus, with
    d in {-1, 0, 1}: w-1 + SMM_CHUNK + d (one full smm chunk),
    w-1 + SMA_TILE + d (one full sma tile) and EWMA_BLOCK * k + d for
    k in {1, 2} (whole ewma blocks)."""
    ns = {w, w + 1, w + 63, w + 64, w + 65, 700}
    if w > 1:
        ns.add(w - 1)
    for d in (-1, 0, 1):
        ns.add(w - 1 + SMM_CHUNK + d)
        ns.add(w - 1 + SMA_TILE + d)
        ns.add(EWMA_BLOCK + d)
        ns.add(2 * EWMA_BLOCK + d)
    return tuple(sorted(n for n in ns if n >= 1))


def _rows(rng, N, w):
    def rnd():
        return rng.random(N, dtype=np.float32)

    rows = [
        ("gamma", rng.gamma(2.0, 0.5, size=N).astype(np.float32)),
        ("normal", rng.normal(size=N).astype(np.float32)),
        ("ascending", np.sort(rnd())),
        ("descending", np.sort(rnd())[::-1].copy()),
        ("constant", np.full(N, 0.7, dtype=np.float32)),
        ("ties", rng.choice(np.array([0, 1, 2], dtype=np.float32), size=N)),
    ]
    r = np.zeros(N, dtype=np.float32)
    r[N // 2:] = 1.0
    rows.append(("step", r))
    r = rnd()
    r[0] = NAN
    rows.append(("nan_first", r))
    r = rnd()
    r[N - 1] = NAN
    rows.append(("nan_last", r))
    r = rnd()
    r[0::w] = NAN  # every window of w holds exactly one of these
    rows.append(("nan_every_w", r))
    rows.append(("all_nan", np.full(N, NAN, dtype=np.float32)))
    # one clean window [p, p+w); a NaN every w positions on both sides
    r = rnd()
    p = max(N - w, 0) // 3
    if p >= 1:
        r[p - 1::-w] = NAN
    r[p + w::w] = NAN
    rows.append(("nan_all_but_one", r))
    r = rnd()
    r[:w + 3] = NAN  # what cross_validate leaves for a lookback model
    rows.append(("nan_lead_run", r))
    r = rnd()
    r[N // 2] = np.inf
    rows.append(("pos_inf", r))
    r = rnd()
    r[N // 3] = -np.inf
    rows.append(("neg_inf", r))
    # the sma own-window rule: windows past the outlier hold 1e-3 values
    r = (np.float32(1e-3) * (1 + rnd())).astype(np.float32)
    r[min(OUTLIER_AT, N - 1)] = np.float32(1e30)
    rows.append(("outlier", r))
    k = 0
    while len(rows) < R:
        kind = rng.gamma(2.0, 0.5, size=N) if k % 2 else rng.normal(size=N)
        rows.append((f"random{k}", kind.astype(np.float32)))
        k += 1
    return rows


@functools.lru_cache(maxsize=None)
def case(w, N, seed=0):
    rng = np.random.default_rng([seed, w, N, 21])
    rows = _rows(rng, N, w)
    assert len(rows) == R
    X = np.stack([r for _, r in rows])
    X.setflags(write=False)
    return tuple(n for n, _ in rows), X


@functools.lru_cache(maxsize=None)
def big_case(method, seed=0):
    """One large row per method: smm w = N = 8192 (the LDS limit), sma
    and ewma N = 16384, w = 144 (the longest KFCV series). Returns
    ``(w, names, X)``."""
    rng = np.random.default_rng([seed, 22])
    if method == "smm":
        w, N = 8192, 8192
    else:
        w, N = 144, 16384
    X = rng.gamma(2.0, 0.5, size=(1, N)).astype(np.float32)
    X.setflags(write=False)
    return w, ("gamma",), X


@functools.lru_cache(maxsize=None)
def long_window_case(seed=0):
    """sma windows around SMA_SEG (a second staging pass): w in
    {1023, 1024, 1025}, N = w + 5, three rows. Returns
    ``[(w, names, X)]``."""
    out = []
    for w in (SMA_SEG - 1, SMA_SEG, SMA_SEG + 1):
        rng = np.random.default_rng([seed, w, 23])
        N = w + 5
        X = np.stack([
            rng.gamma(2.0, 0.5, size=N).astype(np.float32),
            rng.normal(size=N).astype(np.float32),
            rng.random(N, dtype=np.float32),
        ])
        X[2, w + 2] = NAN
        X.setflags(write=False)
        out.append((w, ("gamma", "normal", "nan_late"), X))
    return out


@functools.lru_cache(maxsize=None)
def oracle(method, w, N, seed=0):
    """``reference.smooth_ref`` of ``case(w, N)``: (value, value_abs)."""
    _, X = case(w, N, seed)
    val, val_abs = ref.smooth_ref(X, w, method)
    val.setflags(write=False)
    val_abs.setflags(write=False)
    return val, val_abs


def sma_bound(w, val_abs):
    """|got - want| per output for sma against the fp64 oracle: a
    sequential fp64 sum of w terms plus the division,
    4 * 2^-53 * w * mean_w|x|."""
    return 4.0 * 2.0 ** -53 * w * val_abs


def ewma_bound(val_abs):
    """1e-12 * ewm|x|: the bar test_threshold_oracle.py uses for
    oracle-vs-pandas."""
    return 1e-12 * val_abs
