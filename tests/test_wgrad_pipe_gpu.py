"""The whole-tile weight-grad kernel (wgrad_pipe.hip: 16-byte loads,
row-major LDS images, transposed LDS reads) behind ``grouped_wgrad_xh``,
``grouped_linear_wgrad`` and ``grouped_linear_wgrad_hprev``.

Every case asserts ``ops.last_wgrad_launch()`` first, so a dispatch
change cannot quietly move a case to the other kernel. The oracles and
the fp32 bound are those of tests/gemm_cases.py: fp64 products of the
bf16-rounded inputs, ``max(atol, 2^-22 |want|)`` with ``atol`` = 4x the
error of the same product in fp32 on the CPU. Lattice inputs (ternary,
one-hot) make every product and every partial sum exact in any order,
so they allow no error at all; any difference is an addressing defect.
"""
import functools

import pytest
import torch

import gemm_cases as gc
from gordo_amd import ops

pytestmark = pytest.mark.gpu

MSTEP = 32

# (G, B, T, F, H), forced chunk rows (None: the host's own choice)
XH_CASES = [
    ((1, 1, 1, 8, 8), None),       # every h_prev is zero: dWh == 0
    ((2, 3, 2, 8, 8), None),
    ((2, 3, 47, 56, 48), 160),     # one chunk
    ((2, 3, 47, 56, 48), 64),      # 64 + 64 + ragged 13
    ((2, 3, 47, 56, 48), 32),      # boundaries 32..128, none a multiple of T
    ((1, 2, 5, 64, 64), None),     # K = 128, N = 256: the largest tile
    ((9, 5, 3, 32, 40), None),     # K = 72, N = 160: padded fragments
    ((3, 1, 13, 40, 32), None),    # M < one m-step, M % 8 != 0
]
LINEAR_CASES = [(2, 141, 56, 192), (1, 7, 8, 8)]  # (G, M, K, N)


def require_hip():
    assert ops.hip_available(), (
        "HIP extension not built — GPU tests must not fall back to eager"
    )


def dev(t):
    return t.to("cuda", torch.bfloat16)


def poison(numel, dtype=torch.float32):
    """The poison() idiom of test_gemm_kernels_gpu.py: make the block
    the op's ``torch::empty`` is likely to get read back NaN."""
    t = torch.full((numel,), float("nan"), dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    del t


def offset_view(t):
    flat = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    flat[1:] = t.reshape(-1)
    v = flat[1:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def set_env(monkeypatch, pipe=None, chunk=None):
    for name, val in (("GORDO_WGRAD_PIPE", pipe), ("GORDO_WGRAD_CHUNK", chunk)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))


def h_prev_of(hs):
    G, B, T, H = hs.shape
    return torch.cat(
        [torch.zeros_like(hs[:, :, :1]), hs[:, :, :-1]], dim=2
    ).reshape(G, B * T, H)


def forced_chunks(M, chunk):
    rows = -(-chunk // MSTEP) * MSTEP
    return -(-M // rows)


def assert_launch(family, chunks=None):
    rec = ops.last_wgrad_launch()
    assert rec["family"] == family, rec
    assert rec["mstep"] == MSTEP, rec
    if chunks is not None:
        assert rec["chunks"] == chunks, rec
    return rec


@functools.lru_cache(maxsize=None)
def xh_inputs(shape, kind):
    """(seq, hs, dG) on the CPU in fp32 (bf16-representable), and the
    fp64 oracle of the combined [dWx ; dWh] and of db."""
    G, B, T, F, H = shape
    make = gc.ternary if kind == "lattice" else gc.rand
    seq = make(G, B * T, F, seed=31)
    hs = make(G, B, T, H, seed=32)
    dG = make(G, B * T, 4 * H, seed=33)
    A = torch.cat([seq, h_prev_of(hs)], dim=2)
    return (seq, hs, dG), gc.wgrad_oracle(A, dG)


@functools.lru_cache(maxsize=None)
def linear_inputs(shape, kind):
    G, M, K, N = shape
    make = gc.ternary if kind == "lattice" else gc.rand
    X, dZ = make(G, M, K, seed=34), make(G, M, N, seed=35)
    return (X, dZ), gc.wgrad_oracle(X, dZ)


def run_xh(inputs, T):
    seq, hs, dG = inputs
    dWx, dWh, db = ops.grouped_wgrad_xh(dev(seq), dev(hs), dev(dG), T)
    assert dWx.dtype == dWh.dtype == db.dtype == torch.float32
    return torch.cat([dWx, dWh], dim=1), db


# ---------------------------------------------------------------------------
# 1. one-hot placement: the transposed-read address map, lane by lane
# ---------------------------------------------------------------------------
ONE_HOT_B, ONE_HOT_T, ONE_HOT_CHUNK = 5, 16, 64


@pytest.mark.parametrize("chunk", [ONE_HOT_CHUNK, None])
@pytest.mark.parametrize("F,H", [(56, 48), (8, 8)])
def test_one_hot_placement(monkeypatch, F, H, chunk):
    """One group per (m*, k*, n*): A has a single 1 at (m*, k*), dG a
    single 1 at (m*, n*); dW must be exactly one 1 at (k*, n*) and db
    one 1 at n*. In the hs half the 1 sits at row m*-1; where m* is a
    t == 0 row that is t == T-1 of the previous batch element (or
    nothing, for m* == 0) and must NOT reach dW."""
    require_hip()
    B, T = ONE_HOT_B, ONE_HOT_T
    M, K, N = B * T, F + H, 4 * H
    ms = [0, 3, 4, 7, 8, 15, 16, 31, 32, ONE_HOT_CHUNK - 1, ONE_HOT_CHUNK,
          M - 1]
    ks = sorted({0, 7, 8, F - 1, F, K - 1})
    ns = sorted({0, 15, 16, N - 1})
    cases = [(m, k, n) for m in ms for k in ks for n in ns]
    G = len(cases)
    seq = torch.zeros(G, M, F)
    hs = torch.zeros(G, M, H)
    dG = torch.zeros(G, M, N)
    want_W = torch.zeros(G, K, N)
    want_b = torch.zeros(G, N)
    leak_checks = 0
    for g, (m, k, n) in enumerate(cases):
        dG[g, m, n] = 1.0
        want_b[g, n] = 1.0
        if k < F:
            seq[g, m, k] = 1.0
            want_W[g, k, n] = 1.0
        elif m % T != 0:
            hs[g, m - 1, k - F] = 1.0
            want_W[g, k, n] = 1.0
        elif m > 0:
            hs[g, m - 1, k - F] = 1.0  # t = T-1 of the previous element
            leak_checks += 1
    assert leak_checks > 0
    set_env(monkeypatch, chunk=chunk)
    got_Wx, got_Wh, got_b = ops.grouped_wgrad_xh(
        dev(seq), dev(hs.view(G, B, T, H)), dev(dG), T
    )
    assert_launch("wgrad_pipe",
                  forced_chunks(M, chunk) if chunk else None)
    got_W = torch.cat([got_Wx, got_Wh], dim=1).cpu()
    bad = (got_W != want_W).flatten(1).any(dim=1).nonzero().flatten()
    assert bad.numel() == 0, (
        f"{bad.numel()} of {G} one-hot cases misplaced; first (m*, k*, n*) = "
        f"{cases[int(bad[0])]}, got nonzeros at "
        f"{got_W[int(bad[0])].nonzero().tolist()}"
    )
    assert torch.equal(got_b.cpu(), want_b)


# ---------------------------------------------------------------------------
# 2. lattice-exact against the fp64 oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape,chunk", XH_CASES)
def test_xh_lattice_exact(monkeypatch, shape, chunk):
    require_hip()
    G, B, T, F, H = shape
    inputs, ((want_W, atol_W), (want_b, atol_b)) = xh_inputs(shape, "lattice")
    assert atol_W == 0.0 and atol_b == 0.0
    set_env(monkeypatch, chunk=chunk)
    got_W, got_b = run_xh(inputs, T)
    assert_launch("wgrad_pipe",
                  forced_chunks(B * T, chunk) if chunk else None)
    assert torch.equal(got_W.double().cpu(), want_W)
    assert torch.equal(got_b.double().cpu(), want_b)
    if T == 1:
        assert not bool(got_W[:, F:].any())


@pytest.mark.parametrize("shape", LINEAR_CASES)
def test_linear_lattice_exact(monkeypatch, shape):
    require_hip()
    (X, dZ), ((want_W, _), (want_b, _)) = linear_inputs(shape, "lattice")
    set_env(monkeypatch)
    got_W, got_b = ops.grouped_linear_wgrad(dev(X), dev(dZ))
    assert_launch("wgrad_pipe")
    assert torch.equal(got_W.double().cpu(), want_W)
    assert torch.equal(got_b.double().cpu(), want_b)


@pytest.mark.parametrize("shape,chunk", XH_CASES)
def test_hprev_lattice_exact(monkeypatch, shape, chunk):
    require_hip()
    G, B, T, F, H = shape
    hs = gc.ternary(G, B, T, H, seed=36)
    dG = gc.ternary(G, B * T, 4 * H, seed=37)
    (want_W, _), (want_b, _) = gc.wgrad_oracle(h_prev_of(hs), dG)
    set_env(monkeypatch, chunk=chunk)
    got_W, got_b = ops.grouped_linear_wgrad_hprev(dev(hs), dev(dG), T)
    assert_launch("wgrad_pipe",
                  forced_chunks(B * T, chunk) if chunk else None)
    assert torch.equal(got_W.double().cpu(), want_W)
    assert torch.equal(got_b.double().cpu(), want_b)


# ---------------------------------------------------------------------------
# 3. random bf16 inputs against the fp64 oracle
# ---------------------------------------------------------------------------
ALIGNED_XH = [(s, c) for s, c in XH_CASES] + [
    (s, None) for s in gc.WGRAD_XH_CASES if s[3] % 8 == 0 and s[3] + s[4] <= 128
]
FALLBACK_XH = [
    s for s in gc.WGRAD_XH_CASES if s[3] % 8 != 0 or s[3] + s[4] > 128
]


@pytest.mark.parametrize("shape,chunk", ALIGNED_XH)
def test_xh_vs_fp64(monkeypatch, shape, chunk):
    require_hip()
    G, B, T, F, H = shape
    inputs, (oracle_W, oracle_b) = xh_inputs(shape, "random")
    set_env(monkeypatch, chunk=chunk)
    got_W, got_b = run_xh(inputs, T)
    assert_launch("wgrad_pipe",
                  forced_chunks(B * T, chunk) if chunk else None)
    gc.check_wgrad(f"xh {shape} chunk={chunk} dW", got_W, oracle_W)
    gc.check_wgrad(f"xh {shape} chunk={chunk} db", got_b, oracle_b)


@pytest.mark.parametrize("shape", FALLBACK_XH)
def test_xh_cases_outside_the_tile_vs_fp64(monkeypatch, shape):
    """The rows of gc.WGRAD_XH_CASES the whole-tile kernel does not
    serve (F % 8 != 0, K > 128) keep the tile kernel and the oracle."""
    require_hip()
    G, B, T, F, H = shape
    inputs, (oracle_W, oracle_b) = xh_inputs(shape, "random")
    set_env(monkeypatch)
    got_W, got_b = run_xh(inputs, T)
    assert_launch("wgrad_tile")
    gc.check_wgrad(f"xh {shape} dW", got_W, oracle_W)
    gc.check_wgrad(f"xh {shape} db", got_b, oracle_b)


@pytest.mark.parametrize("shape", LINEAR_CASES)
def test_linear_vs_fp64(monkeypatch, shape):
    require_hip()
    (X, dZ), (oracle_W, oracle_b) = linear_inputs(shape, "random")
    set_env(monkeypatch)
    got_W, got_b = ops.grouped_linear_wgrad(dev(X), dev(dZ))
    assert_launch("wgrad_pipe")
    gc.check_wgrad(f"linear {shape} dW", got_W, oracle_W)
    gc.check_wgrad(f"linear {shape} db", got_b, oracle_b)


# ---------------------------------------------------------------------------
# 4. old kernel against new on the same inputs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape,chunk", XH_CASES)
def test_old_vs_new(monkeypatch, shape, chunk):
    """Lattice inputs: bit-equal. Random inputs: each within the oracle
    bound (the two kernels order the 32 products of an MFMA, and the
    chunks, differently, so bit equality is not required)."""
    require_hip()
    G, B, T, F, H = shape
    lattice, _ = xh_inputs(shape, "lattice")
    random, (oracle_W, oracle_b) = xh_inputs(shape, "random")
    out = {}
    for arm, pipe, family in (("old", 0, "wgrad_tile"),
                              ("new", None, "wgrad_pipe")):
        set_env(monkeypatch, pipe=pipe, chunk=chunk)
        out[arm, "lattice"] = run_xh(lattice, T)
        assert_launch(family)
        out[arm, "random"] = run_xh(random, T)
        assert_launch(family)
    for i in range(2):
        assert torch.equal(out["old", "lattice"][i], out["new", "lattice"][i])
    for arm in ("old", "new"):
        gc.check_wgrad(f"{arm} {shape} dW", out[arm, "random"][0], oracle_W)
        gc.check_wgrad(f"{arm} {shape} db", out[arm, "random"][1], oracle_b)


# ---------------------------------------------------------------------------
# 5. fallback arms
# ---------------------------------------------------------------------------
def test_fallback_f_not_multiple_of_8(monkeypatch):
    require_hip()
    shape = (2, 3, 5, 34, 16)
    inputs, (oracle_W, oracle_b) = xh_inputs(shape, "random")
    set_env(monkeypatch)
    got_W, got_b = run_xh(inputs, shape[2])
    assert_launch("wgrad_tile")
    gc.check_wgrad("F=34 dW", got_W, oracle_W)
    gc.check_wgrad("F=34 db", got_b, oracle_b)


def test_fallback_k_136(monkeypatch):
    require_hip()
    shape = (1, 2, 5, 72, 64)
    inputs, (oracle_W, oracle_b) = xh_inputs(shape, "random")
    set_env(monkeypatch)
    got_W, got_b = run_xh(inputs, shape[2])
    assert_launch("wgrad_tile")
    gc.check_wgrad("K=136 dW", got_W, oracle_W)
    gc.check_wgrad("K=136 db", got_b, oracle_b)


def test_fallback_n_264(monkeypatch):
    require_hip()
    shape = (1, 40, 8, 264)
    (X, dZ), (oracle_W, oracle_b) = linear_inputs(shape, "random")
    set_env(monkeypatch)
    got_W, got_b = ops.grouped_linear_wgrad(dev(X), dev(dZ))
    assert_launch("wgrad_tile")
    gc.check_wgrad("N=264 dW", got_W, oracle_W)
    gc.check_wgrad("N=264 db", got_b, oracle_b)


@pytest.mark.parametrize("which", ["seq", "hs", "dG"])
def test_fallback_offset_view(monkeypatch, which):
    """A served shape whose operand starts one element off a 16-byte
    boundary: the shape alone must not select the 16-byte loads."""
    require_hip()
    shape = (2, 3, 5, 8, 8)
    (seq, hs, dG), (oracle_W, oracle_b) = xh_inputs(shape, "random")
    d = {"seq": dev(seq), "hs": dev(hs), "dG": dev(dG)}
    d[which] = offset_view(d[which])
    set_env(monkeypatch)
    dWx, dWh, db = ops.grouped_wgrad_xh(d["seq"], d["hs"], d["dG"], shape[2])
    assert_launch("wgrad_tile")
    gc.check_wgrad(f"offset {which} dW", torch.cat([dWx, dWh], 1), oracle_W)
    gc.check_wgrad(f"offset {which} db", db, oracle_b)


# ---------------------------------------------------------------------------
# 6. every element written, 7. determinism (single chunk: plain stores)
# ---------------------------------------------------------------------------
SINGLE_CHUNK = [(9, 5, 3, 32, 40), (1, 2, 5, 64, 64)]  # K,N = 72,160; 128,256


@pytest.mark.parametrize("shape", SINGLE_CHUNK)
def test_single_chunk_writes_every_element(monkeypatch, shape):
    require_hip()
    G, B, T, F, H = shape
    K, N = F + H, 4 * H
    lattice, ((want_W, _), (want_b, _)) = xh_inputs(shape, "lattice")
    random, (oracle_W, oracle_b) = xh_inputs(shape, "random")
    set_env(monkeypatch, chunk=4096)
    d_lat = [dev(t) for t in lattice]
    d_rnd = [dev(t) for t in random]
    poison(G * K * N)
    dWx, dWh, db = ops.grouped_wgrad_xh(*d_lat, T)
    assert_launch("wgrad_pipe", 1)
    got = torch.cat([dWx, dWh], dim=1)
    assert not bool(torch.isnan(got).any())
    assert torch.equal(got.double().cpu(), want_W)
    assert torch.equal(db.double().cpu(), want_b)
    poison(G * K * N)
    dWx, dWh, db = ops.grouped_wgrad_xh(*d_rnd, T)
    assert_launch("wgrad_pipe", 1)
    # check_wgrad compares through (err <= bound).all(): NaN fails it
    gc.check_wgrad(f"poisoned {shape} dW", torch.cat([dWx, dWh], 1), oracle_W)
    gc.check_wgrad(f"poisoned {shape} db", db, oracle_b)


@pytest.mark.parametrize("shape", SINGLE_CHUNK + [(2, 3, 47, 56, 48)])
def test_single_chunk_is_deterministic(monkeypatch, shape):
    require_hip()
    T = shape[2]
    random, _ = xh_inputs(shape, "random")
    d = [dev(t) for t in random]
    set_env(monkeypatch, chunk=4096)
    first = ops.grouped_wgrad_xh(*d, T)
    assert_launch("wgrad_pipe", 1)
    second = ops.grouped_wgrad_xh(*d, T)
    assert_launch("wgrad_pipe", 1)
    for a, b in zip(first, second):
        assert torch.equal(a.contiguous().view(torch.int32),
                           b.contiguous().view(torch.int32))
