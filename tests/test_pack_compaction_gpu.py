"""Pack compaction on the GPU: a fit that goes on in a child pack of its
live models leaves every model, bit for bit, where the same fit without
compaction leaves it.

Shapes and data follow test_early_stopping_gpu.py: batches hold at most
512 rows, so every weight-grad launch is a single chunk (no fp32
atomics into dW) and a fit is reproducible bit for bit. No kernel on
the path reduces across models, so a model's arithmetic does not depend
on the G of the pack it trains in.

The expected compaction list is the replay of the policy function over
the off arm's ``epochs_run``; the data are chosen so that it is not
empty."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from compaction_cases import (
    assert_history_shape, fit_arm, replay_compactions,
)
from gordo_amd import ops
from gordo_amd.engine.pack import DensePack, LSTMPack
from test_early_stopping_gpu import _dense_spec, _lstm_spec, require_hip

G = 5
ES = {"monitor": "loss", "patience": 1, "min_delta": 0.01}
SEEDS = [1, 4, 5, 2, 3]


def _data():
    """Three sets of uniform noise (stall early) and the two sets of
    large sines of test_early_stopping_gpu.py (improve for many
    epochs)."""
    n, f = 260, 8
    t = np.linspace(0, 12, n)
    noise = [np.random.default_rng(s).random((n, f)) * 0.5
             for s in (42, 43, 44)]
    s1 = np.stack([np.sin(t + p) for p in np.linspace(0, 2, f)], axis=1) * 2
    s2 = np.stack(
        [np.cos(2 * t + p) for p in np.linspace(0, 3, f)], axis=1
    ) * 3
    return torch.tensor(
        np.stack(noise + [s1, s2]).astype("float32"), device="cuda"
    )


def _flat_buffers(pack):
    store = pack.store
    return [("p32", store.p32), ("mirror", store.plp)] + store.slots()


def _assert_packs_bit_equal(on, off):
    assert on.G == off.G == G
    for (name, a), (_, b) in zip(_flat_buffers(on), _flat_buffers(off)):
        view = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
        same = a.view(view) == b.view(view)
        if not bool(same.all()):
            bad = torch.nonzero(~same).reshape(-1)
            raise AssertionError(
                f"{name}: {bad.numel()} of {a.numel()} elements differ, "
                f"first at flat index {int(bad[0])}"
            )


_OFF = {}


def _arms(kind, shuffle, ratio, spec=None, es=ES, X=None, key=None):
    require_hip()
    cls = DensePack if kind == "dense" else LSTMPack
    if spec is None:
        spec = _dense_spec() if kind == "dense" else _lstm_spec()
    epochs, batch = (12, 128) if kind == "dense" else (6, 64)
    X = _data() if X is None else X
    fit = dict(epochs=epochs, batch_size=batch, shuffle=shuffle,
               early_stopping=es)
    key = (kind, shuffle, key)
    if key not in _OFF:
        snapshot = cls(spec, G, device="cuda", seeds=SEEDS).store.p32.clone()
        off, off_hist = fit_arm(
            lambda: cls(spec, G, device="cuda", seeds=SEEDS,
                        init_p32=snapshot), X, fit, None,
        )
        chunks = ops.last_wgrad_launch()["chunks"]
        _OFF[key] = (snapshot, off, off_hist, chunks)
    snapshot, off, off_hist, off_chunks = _OFF[key]
    on, on_hist = fit_arm(
        lambda: cls(spec, G, device="cuda", seeds=SEEDS, init_p32=snapshot),
        X, fit, ratio,
    )
    on_chunks = ops.last_wgrad_launch()["chunks"]
    print(kind, "shuffle", shuffle, "ratio", ratio, "epochs_run",
          off_hist.epochs_run, "best_epoch", off_hist.best_epoch,
          "compactions", on_hist.compactions)
    assert off_chunks == 1 and on_chunks == 1
    return off, off_hist, on, on_hist


def _assert_arms_agree(off, off_hist, on, on_hist, ratio):
    want = replay_compactions(off_hist.epochs_run, ratio)
    # the precondition: the off arm alone staggers enough to compact
    assert want, off_hist.epochs_run
    assert off_hist.compactions == []
    assert on_hist.compactions == want
    assert on_hist.epochs_run == off_hist.epochs_run
    assert on_hist.best_epoch == off_hist.best_epoch
    assert_history_shape(on_hist, G, want)
    for key in off_hist:
        for g in range(G):
            for e in range(off_hist.epochs_run[g]):
                assert on_hist[key][e][g] == pytest.approx(
                    off_hist[key][e][g], rel=1e-5, abs=1e-8
                ), (key, e, g)
    assert on.store.active is None
    assert on.store.step_count == off.store.step_count
    assert int(on.store.step_buf) == int(off.store.step_buf)
    _assert_packs_bit_equal(on, off)


@pytest.mark.parametrize("ratio", [0.5, 1.0])
@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("kind", ["dense", "lstm"])
def test_compacted_fit_is_bit_equal(kind, shuffle, ratio):
    off, off_hist, on, on_hist = _arms(kind, shuffle, ratio)
    _assert_arms_agree(off, off_hist, on, on_hist, ratio)


def _restore_case():
    """SGD at learning rate 3.0, as test_restore_best_weights_on_gpu:
    the loss rises again, so there is something to go back from."""
    spec = _dense_spec(optimizer="SGD",
                       optimizer_kwargs={"learning_rate": 3.0})
    es = {"monitor": "loss", "patience": 2, "restore_best_weights": True}
    return spec, es, _data() * RESTORE_SCALES.cuda().view(G, 1, 1)


# Per-model scale of _data() for the restore case. At this learning
# rate most data diverge at once (best epoch 0, stop after epoch 2);
# at these scales the second noise set recovers once (it stops later
# and goes back to weights captured before the compaction) and the
# first sines train on to the epoch cap.
RESTORE_SCALES = torch.tensor([1.5, 0.75, 1.5, 0.25, 1.5])


@pytest.mark.parametrize("ratio", [0.5, 1.0])
def test_restore_best_weights_crosses_a_compaction(ratio):
    spec, es, X = _restore_case()
    off, off_hist, on, on_hist = _arms(
        "dense", False, ratio, spec=spec, es=es, X=X, key="restore"
    )
    # some model does go back from its last weights
    assert any(
        b + 1 < r for b, r in zip(off_hist.best_epoch, off_hist.epochs_run)
    )
    _assert_arms_agree(off, off_hist, on, on_hist, ratio)


def test_no_callbacks_means_no_compaction_and_the_unmasked_step():
    require_hip()
    pack = DensePack(_dense_spec(), G, device="cuda", seeds=SEEDS)
    seen = []
    step = pack.store.optimizer_step
    pack.store.optimizer_step = lambda: (
        seen.append(pack.store.active), step()
    )
    X = _data()
    hist = pack.fit(X, X.clone(), epochs=2, batch_size=128, shuffle=False)
    assert seen and all(a is None for a in seen)
    assert hist.compactions is None and hist.best_epoch is None
    assert hist.epochs_run == [2] * G
