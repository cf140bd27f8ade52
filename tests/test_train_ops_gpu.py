"""HIP train-step ops that honour compile settings: ``ops.loss_bwd``
(loss + grad + Keras accuracy count) and ``ops.optimizer_step``.

The oracle is always the CPU fp32 reference (gordo_amd.ops.reference,
itself checked against autograd / float64 numpy in
tests/test_compile_surface.py), fed the same bf16-rounded inputs upcast
to fp32. The default configuration (MSE + Adam) must stay bit-identical
to the kernels it used before.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gordo_amd import ops
from gordo_amd.ops import reference as ref

LOSSES = [("mse", 1.0), ("mae", 1.0), ("huber", 0.5), ("logcosh", 1.0)]

# (real_f, Fp): binary accuracy; scalar path; argmax must ignore pad
# columns; bench shape; 8 lanes per row; a row longer than one
# 64-lane x 8-element pass
WIDTHS = [(1, 1), (5, 5), (5, 8), (50, 56), (64, 64), (520, 520)]


def require_hip():
    assert ops.hip_available(), (
        "HIP extension not built — GPU tests must not fall back to eager"
    )


_INPUT_CACHE = {}


def _inputs(G, B, real_f, Fp):
    """bf16-rounded (Y, T) as fp32 CPU tensors with planted tie rows and
    all-negative rows; pad columns are zero. Built once per shape and
    never modified."""
    key = (G, B, real_f, Fp)
    if key in _INPUT_CACHE:
        return _INPUT_CACHE[key]
    gen = torch.Generator().manual_seed(1000 * Fp + 10 * B + G)
    Y = torch.zeros(G, B, Fp)
    T = torch.zeros(G, B, Fp)
    Y[..., :real_f] = torch.randn(G, B, real_f, generator=gen)
    T[..., :real_f] = torch.randn(G, B, real_f, generator=gen)
    if real_f == 1:
        # binary accuracy: targets in {0, 1}, outputs on both sides of 0.5
        T[..., 0] = (torch.rand(G, B, generator=gen) > 0.5).float()
        Y[..., 0] = torch.rand(G, B, generator=gen)
        Y[0, 0, 0] = 0.5  # not > 0.5
    if real_f >= 5:
        last = real_f - 1
        for g in range(G):
            rows = [0] if B == 1 else [1, 2, 3, B - 1]
            # exact two-way tie in Y (first and last column): lowest wins
            r = rows[0]
            Y[g, r, :real_f] = -1.0
            Y[g, r, 0] = Y[g, r, last] = 2.0
            T[g, r, :real_f] = 0.0
            T[g, r, 0 if g % 2 == 0 else last] = 1.0
            if B > 1:
                # tie in T between two lanes of one row (wide rows)
                T[g, rows[1], :real_f] = -0.5
                T[g, rows[1], 1] = T[g, rows[1], real_f * 3 // 4] = 4.0
                Y[g, rows[1], 1] = 9.0
                # all-negative rows: a padded 0 must not win (with the
                # pad columns counted this row would be a hit)
                Y[g, rows[2], :real_f] = -torch.arange(
                    1, real_f + 1, dtype=torch.float32)
                T[g, rows[2], :real_f] = -torch.arange(
                    2, real_f + 2, dtype=torch.float32)
                T[g, rows[2], 1] = -0.5
                Y[g, rows[3], :real_f] = -3.0
                Y[g, rows[3], last] = -1.0
                T[g, rows[3], :real_f] = -2.0
                T[g, rows[3], last] = -0.25
    Y = Y.to(torch.bfloat16).float()
    T = T.to(torch.bfloat16).float()
    _INPUT_CACHE[key] = (Y, T)
    return Y, T


def _dev(t):
    return t.to("cuda", torch.bfloat16)


@pytest.mark.parametrize("loss,delta", LOSSES)
@pytest.mark.parametrize("real_f,Fp", WIDTHS)
@pytest.mark.parametrize("G,B", [(1, 1), (3, 37), (1, 37), (3, 1)])
def test_loss_bwd_matches_reference(G, B, real_f, Fp, loss, delta):
    require_hip()
    Y, T = _inputs(G, B, real_f, Fp)
    want_loss, want_dY, want_correct = ref.loss_bwd(Y, T, loss, real_f, delta)
    got_loss, got_dY, got_correct = ops.loss_bwd(
        _dev(Y), _dev(T), loss, real_f, delta
    )
    assert got_correct.dtype == torch.int32
    assert got_correct.cpu().tolist() == want_correct.tolist()
    torch.testing.assert_close(got_loss.cpu(), want_loss, rtol=1e-4, atol=1e-7)
    # unnormalised gradient units: two bf16 roundings of the output
    n = B * real_f
    assert got_dY.dtype == torch.bfloat16 and got_dY.shape == Y.shape
    torch.testing.assert_close(
        got_dY.float().cpu() * n, want_dY * n, rtol=2.0 ** -7, atol=1e-5
    )
    # pad columns stay inert
    assert float(got_dY[..., real_f:].float().abs().sum()) == 0.0

    ev_loss, none, ev_correct = ops.loss_bwd(
        _dev(Y), _dev(T), loss, real_f, delta, want_grad=False
    )
    assert none is None
    assert ev_correct.cpu().tolist() == want_correct.tolist()
    # float atomics across blocks may reorder the sum between launches
    torch.testing.assert_close(ev_loss, got_loss, rtol=1e-6, atol=1e-9)


def test_loss_bwd_planted_rows_are_what_they_claim():
    """The fixtures really contain ties and all-negative rows whose
    answer depends on ignoring the pad columns."""
    Y, T = _inputs(3, 37, 5, 8)
    assert (Y[:, 1, 0] == Y[:, 1, 4]).all() and (Y[:, 1, 0] == 2.0).all()
    assert (Y[:, 3, :5] < 0).all() and (T[:, 36, :5] < 0).all()
    padded = torch.argmax(Y, -1) == torch.argmax(T, -1)
    real = torch.argmax(Y[..., :5], -1) == torch.argmax(T[..., :5], -1)
    assert padded.sum() != real.sum()


def test_correct_count_ranks_nan_as_the_reference_does():
    """torch.argmax ranks NaN above every number (first NaN wins); the
    kernel must count a diverged model's rows the same way."""
    require_hip()
    nan = float("nan")
    for real_f, Fp in [(5, 8), (50, 56), (520, 520)]:
        Y, T = (t.clone() for t in _inputs(3, 37, real_f, Fp))
        q = real_f * 3 // 4
        Y[:, 4, :real_f] = nan          # all-NaN in both: index 0 == 0
        T[:, 4, :real_f] = nan
        Y[:, 5, q] = nan                # NaN beats any number: q vs q
        T[:, 5, q] = nan
        T[:, 5, 0] = 100.0
        Y[:, 6, 1] = Y[:, 6, q] = nan   # first NaN wins: 1 vs q
        T[:, 6, q] = nan
        Y[:, 7, :real_f] = nan          # all-NaN vs numbers: 0 vs 2
        T[:, 7, :real_f] = 0.0
        T[:, 7, 2] = 1.0
        want = ref.loss_bwd(Y, T, "mse", real_f)[2]
        hit = torch.argmax(Y[..., :real_f], -1) == torch.argmax(
            T[..., :real_f], -1)
        assert hit[:, 4].all() and hit[:, 5].all()
        assert not hit[:, 6].any() and not hit[:, 7].any()
        got = ops.loss_bwd(_dev(Y), _dev(T), "mse", real_f)[2]
        assert got.cpu().tolist() == want.tolist()


@pytest.mark.parametrize("loss,delta", LOSSES)
def test_zero_difference_is_exactly_zero_loss_and_gradient(loss, delta):
    """l(0) = 0 and l'(0) = 0 exactly, the property that keeps zero
    padded columns out of the loss sum and the gradient."""
    require_hip()
    Y, _ = _inputs(3, 37, 50, 56)
    got_loss, got_dY, got_correct = ops.loss_bwd(
        _dev(Y), _dev(Y), loss, 50, delta
    )
    assert got_loss.cpu().tolist() == [0.0, 0.0, 0.0]
    assert float(got_dY.float().abs().sum()) == 0.0
    assert got_correct.cpu().tolist() == [37, 37, 37]
    ref_loss = ref.loss_bwd(Y, Y, loss, 50, delta)[0]
    assert ref_loss.tolist() == [0.0, 0.0, 0.0]


def test_loss_bwd_unaligned_view_takes_the_scalar_path():
    """Fp % 8 == 0 but the storage is offset by one element: the
    16-byte path is not legal, the guarded loop must serve it."""
    require_hip()
    Y, T = _inputs(3, 37, 50, 56)
    flat = torch.zeros(Y.numel() + 1, dtype=torch.bfloat16, device="cuda")
    flat[1:] = _dev(Y).reshape(-1)
    Yv = flat[1:].view(Y.shape)
    assert Yv.data_ptr() % 16 != 0
    want_loss, want_dY, want_correct = ref.loss_bwd(Y, T, "huber", 50, 0.5)
    got_loss, got_dY, got_correct = ops.loss_bwd(Yv, _dev(T), "huber", 50, 0.5)
    assert got_correct.cpu().tolist() == want_correct.tolist()
    torch.testing.assert_close(got_loss.cpu(), want_loss, rtol=1e-4, atol=1e-7)
    torch.testing.assert_close(
        got_dY.float().cpu() * (37 * 50), want_dY * (37 * 50),
        rtol=2.0 ** -7, atol=1e-5,
    )


@pytest.mark.parametrize("shape,real_f", [((3, 500, 50), 50),
                                          ((2, 64, 56), 50)])
def test_default_mse_gradient_is_bitwise_mse_bwd(shape, real_f):
    require_hip()
    gen = torch.Generator().manual_seed(13)
    Y = torch.rand(*shape, generator=gen) * 2 - 1
    T = torch.rand(*shape, generator=gen) * 2 - 1
    Y[..., real_f:] = 0
    T[..., real_f:] = 0
    Yd, Td = _dev(Y), _dev(T)
    old_loss, old_dY = ops.mse_bwd(Yd, Td, shape[1] * real_f)
    new_loss, new_dY, _ = ops.loss_bwd(Yd, Td, "mse", real_f)
    assert torch.equal(new_dY.view(torch.int16), old_dY.view(torch.int16))
    torch.testing.assert_close(new_loss, old_loss, rtol=1e-5, atol=1e-8)


def _opt_state(n, init0=0.0, seed=15):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(n, generator=g) * 2 - 1
    grads = [(torch.rand(n, generator=g) * 2 - 1) / t ** 2 for t in (1, 2, 3)]
    slots = [torch.full((n,), float(init0)), torch.zeros(n), torch.zeros(n)]
    return p, grads, slots


def test_default_adam_is_bitwise_adam_step():
    require_hip()
    from gordo_amd.engine.spec import resolve_optimizer

    kind, h = resolve_optimizer("Adam", {"learning_rate": 0.01})
    n = 10007
    p, grads, slots = _opt_state(n)
    a = [t.cuda() for t in (p, *slots[:2])]
    b = [t.cuda() for t in (p, *slots[:2])]
    a_lp, b_lp = a[0].to(torch.bfloat16), b[0].to(torch.bfloat16)
    a_buf = torch.zeros(1, dtype=torch.int32, device="cuda")
    b_buf = torch.zeros(1, dtype=torch.int32, device="cuda")
    for step, g in enumerate(grads, 1):
        gd = g.cuda()
        ops.adam_step(a[0], gd, a[1], a[2], 0.01, 0.9, 0.999, 1e-7, step,
                      a_lp, step_buf=a_buf)
        ops.optimizer_step(kind, b[0], gd, b[1], b[2], None, h, step, b_lp,
                           step_buf=b_buf)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.equal(a_lp.view(torch.int16), b_lp.view(torch.int16))
    assert int(b_buf) == 3


@pytest.mark.parametrize("n", [10007, 5])
@pytest.mark.parametrize(
    "optimizer,kwargs",
    [
        ("SGD", {}),
        ("SGD", {"momentum": 0.9}),
        ("SGD", {"momentum": 0.9, "nesterov": True}),
        ("RMSprop", {}),
        ("RMSprop", {"momentum": 0.8, "rho": 0.95}),
        ("Adagrad", {}),
        ("Adagrad", {"initial_accumulator_value": 0.3,
                     "learning_rate": 0.05}),
        ("Adam", {"amsgrad": True, "learning_rate": 0.01}),
        ("Adamax", {"learning_rate": 0.002}),
    ],
)
def test_optimizer_step_matches_reference(optimizer, kwargs, n):
    require_hip()
    from gordo_amd.engine.spec import resolve_optimizer

    kind, h = resolve_optimizer(optimizer, kwargs)
    init0 = h.get("initial_accumulator_value", 0.0)
    if optimizer == "Adagrad" and not kwargs:
        assert init0 == 0.1  # Keras default accumulator start
    p, grads, slots = _opt_state(n, init0)
    pd = p.cuda()
    sd = [s.cuda() for s in slots]
    plp = pd.to(torch.bfloat16)
    step_buf = torch.zeros(1, dtype=torch.int32, device="cuda")
    for step, g in enumerate(grads, 1):
        ref.optimizer_step(kind, p, g, slots[0], slots[1], slots[2], h, step)
        ops.optimizer_step(kind, pd, g.cuda(), sd[0], sd[1], sd[2], h, step,
                           plp, step_buf=step_buf)
    assert int(step_buf) == 3
    torch.testing.assert_close(pd.cpu(), p, rtol=1e-5, atol=1e-6)
    for got, want in zip(sd, slots):
        torch.testing.assert_close(got.cpu(), want, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(plp.float().cpu(), p, rtol=1e-2, atol=1e-2)
    assert not torch.equal(pd.cpu(), _opt_state(n, init0)[0])


def test_correct_count_is_deterministic():
    require_hip()
    Y, T = _inputs(3, 37, 50, 56)
    Yd, Td = _dev(Y), _dev(T)
    first = ops.loss_bwd(Yd, Td, "mse", 50)[2]
    second = ops.loss_bwd(Yd, Td, "mse", 50)[2]
    assert torch.equal(first, second)


def test_pack_on_gpu_allocates_the_configured_optimizer_state():
    require_hip()
    from gordo_amd.engine.pack import DensePack
    from gordo_amd.engine.spec import LayerSpec, ModelSpec

    def spec(**kw):
        return ModelSpec(
            model_type="feedforward", n_features=5, n_features_out=5,
            layers=[LayerSpec(kind="dense", units=3, activation="tanh"),
                    LayerSpec(kind="dense", units=5, activation="linear")],
            **kw,
        )

    ada = DensePack(spec(optimizer="Adagrad"), G=2, device="cuda")
    assert torch.all(ada.store.m == 0.1) and ada.store.vhat is None
    ams = DensePack(spec(optimizer="Adam",
                         optimizer_kwargs={"amsgrad": True}),
                    G=2, device="cuda")
    X = torch.rand(2, 32, 5, device="cuda").to(ams.compute_dtype)
    loss = ams.train_batch(X, X.clone())
    assert torch.isfinite(loss).all()
    assert ams.last_correct.dtype == torch.int32
    assert float(ams.store.vhat.max()) > 0.0
    # pad units stay exactly zero under every optimizer
    ada.train_batch(X, X.clone())
    for pack in (ada, ams):
        W0 = pack.store.views["W0"]
        assert float(W0[:, 5:, :].abs().sum()) == 0.0
        assert float(W0[:, :, 3:].abs().sum()) == 0.0


def _sine(n, f):
    t = np.linspace(0, 20, n)
    return np.stack(
        [np.sin(t + p) for p in np.linspace(0, 1, f)], axis=1
    ).astype("float32")


def test_estimator_rmsprop_logcosh_on_gpu_reports_real_accuracy():
    require_hip()
    from gordo_amd.machine.model import KerasAutoEncoder

    X = _sine(300, 20)
    model = KerasAutoEncoder(
        kind="feedforward_hourglass", optimizer="RMSprop",
        compile_kwargs={"loss": "logcosh"}, epochs=5, batch_size=64,
        shuffle=False,
    )
    seen = []
    make_pack = model._make_pack

    def recording_make_pack(spec, **kw):
        pack = make_pack(spec, **kw)
        train_batch = pack.train_batch

        def recording(Xb, Tb):
            out = pack.forward(pack._pad_io(Xb, Tb)[0])[-1]
            seen.append((out[..., :20].float().cpu(), Tb[..., :20].float().cpu()))
            return train_batch(Xb, Tb)

        pack.train_batch = recording
        return pack

    model._make_pack = recording_make_pack
    model.fit(X)
    assert model._pack.device.type == "cuda"
    assert model._spec.optimizer_kind == "rmsprop"
    assert model._spec.loss_kind == "logcosh"
    losses = model.history["loss"]
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    acc = model.history["accuracy"]
    assert len(acc) == 5 and any(a > 0.0 for a in acc)
    assert all(0.0 <= a <= 1.0 for a in acc)
    # host recomputation of the final epoch (5 batches of <= 64 rows)
    assert len(seen) == 25
    hits = sum(
        int((torch.argmax(o, -1) == torch.argmax(t, -1)).sum())
        for o, t in seen[-5:]
    )
    assert abs(acc[-1] - hits / 300.0) <= 1.0 / 300.0 + 1e-9


def test_lstm_estimator_sgd_momentum_huber_on_gpu():
    require_hip()
    from gordo_amd.machine.model import KerasLSTMAutoEncoder

    # uniform data: the output bias has a mean to learn, so two epochs
    # of SGD at the Keras default lr move the loss well clear of bf16
    # noise (a zero-mean sine moves it by ~1e-4 relative)
    X = np.random.default_rng(3).random((240, 12)).astype("float32")
    model = KerasLSTMAutoEncoder(
        kind="lstm_hourglass", lookback_window=12, optimizer="SGD",
        optimizer_kwargs={"momentum": 0.9},
        compile_kwargs={"loss": "huber"}, epochs=2,
    )
    model.fit(X)
    assert model._pack.device.type == "cuda"
    assert model._pack.store.optimizer_kind == "sgd"
    losses = model.history["loss"]
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert np.isfinite(model.predict(X)).all()
    assert all(0.0 <= a <= 1.0 for a in model.history["accuracy"])
