"""The per-model EarlyStopping rule (``engine.early_stop``) against a
scalar transcription of Keras 3's callback, and the config parser."""
import math

import numpy as np
import pytest

from gordo_amd.engine.early_stop import EarlyStopState, resolve_monitor
from gordo_amd.machine.model.models import _parse_early_stopping

G = 7
EPOCHS = 14


class ScalarEarlyStopping:
    """One model's Keras 3.3.3 ``EarlyStopping``, step by step.
    ``weights`` stands for the model's weights: the epoch index after
    which they were taken."""

    def __init__(self, monitor="loss", min_delta=0.0, patience=0,
                 mode="auto", baseline=None, restore_best_weights=False,
                 start_from_epoch=0):
        self.min_delta = abs(min_delta)
        self.patience = patience
        self.baseline = baseline
        self.restore = restore_best_weights
        self.start = start_from_epoch
        if mode == "auto":
            mode = "max" if monitor.endswith(("acc", "accuracy")) else "min"
        self.mode = mode
        self.best = math.inf if mode == "min" else -math.inf
        self.wait = 0
        self.best_epoch = 0
        self.best_weights = None
        self.stopped_epoch = None

    def improved(self, v, ref):
        if math.isnan(v):
            return False
        if self.mode == "min":
            return v + self.min_delta < ref
        return v - self.min_delta > ref

    def epoch_end(self, e, v):
        """(stops, improved, captured) at the end of epoch e."""
        captured = False
        if e < self.start:
            return False, False, False
        if self.restore and self.best_weights is None:
            self.best_weights = e
            self.best_epoch = e
            captured = True
        self.wait += 1
        if self.improved(v, self.best):
            self.best = v
            self.best_epoch = e
            if self.restore:
                self.best_weights = e
                captured = True
            if self.baseline is None or self.improved(v, self.baseline):
                self.wait = 0
            return False, True, captured
        if self.wait >= self.patience and e > 0:
            self.stopped_epoch = e
            return True, False, captured
        return False, False, captured


def _sequences(kind, mode, min_delta):
    """[EPOCHS, G] scripted monitor values."""
    rng = np.random.default_rng(5)
    sign = 1.0 if mode == "min" else -1.0
    if kind == "random":
        return rng.random((EPOCHS, G))
    if kind == "ties":
        # start at 1, then move by EXACTLY min_delta in the improving
        # direction (v + min_delta == best: a tie, no improvement), by
        # twice that, or not at all; binary fractions keep it exact
        seq = np.empty((EPOCHS, G))
        seq[0] = 1.0
        steps = rng.integers(0, 3, size=(EPOCHS, G))
        for e in range(1, EPOCHS):
            seq[e] = seq[e - 1] - sign * steps[e] * min_delta
        return seq
    if kind == "nan":
        seq = np.cumsum(-sign * rng.random((EPOCHS, G)) * 0.1, axis=0) + 5.0
        seq[0, ::2] = np.nan          # NaN at epoch 0
        seq[4, 1::3] = np.nan         # NaN mid-run
        seq[6:, 2] = np.nan           # NaN for good
        seq[8:, 5] = seq[7, 5]        # a plateau
        return seq
    raise AssertionError(kind)


def _check(cfg, seq):
    state = EarlyStopState(G, cfg)
    scalars = [ScalarEarlyStopping(**cfg) for _ in range(G)]
    ended = [False] * G
    n_stopped = 0
    for e in range(seq.shape[0]):
        upd = state.update(e, seq[e])
        for g in range(G):
            if ended[g]:
                assert not (upd.stop[g] or upd.improved[g] or upd.capture[g])
                continue
            stop, improved, captured = scalars[g].epoch_end(e, float(seq[e, g]))
            assert bool(upd.stop[g]) == stop, (e, g)
            assert bool(upd.improved[g]) == improved, (e, g)
            assert bool(upd.capture[g]) == captured, (e, g)
            assert state.wait[g] == scalars[g].wait, (e, g)
            assert state.best_epoch[g] == scalars[g].best_epoch, (e, g)
            assert bool(state.has_best[g]) == (
                scalars[g].best_weights is not None
            )
            if not math.isinf(scalars[g].best):
                assert state.best[g] == scalars[g].best, (e, g)
            if stop:
                ended[g] = True
                n_stopped += 1
                assert state.stopped_epoch[g] == e
        assert state.ended.tolist() == ended
    return n_stopped


@pytest.mark.parametrize("kind", ["random", "ties", "nan"])
@pytest.mark.parametrize("patience", [0, 1, 3])
@pytest.mark.parametrize("mode", ["min", "max"])
@pytest.mark.parametrize("start_from_epoch", [0, 2])
@pytest.mark.parametrize("restore", [False, True])
def test_state_matches_scalar_rule(kind, patience, mode, start_from_epoch,
                                   restore):
    min_delta = 0.25 if kind == "ties" else 0.01
    cfg = dict(monitor="loss", patience=patience, min_delta=min_delta,
               mode=mode, start_from_epoch=start_from_epoch,
               restore_best_weights=restore)
    n_stopped = _check(cfg, _sequences(kind, mode, min_delta))
    if kind != "nan" or patience < 3:
        assert n_stopped > 0  # the script does exercise stopping


def test_ties_do_not_improve():
    """v exactly at best - min_delta is no improvement."""
    state = EarlyStopState(1, dict(patience=1, min_delta=0.25))
    assert state.update(0, [1.0]).improved[0]
    upd = state.update(1, [0.75])
    assert not upd.improved[0] and upd.stop[0]
    state = EarlyStopState(1, dict(patience=1, min_delta=0.25))
    state.update(0, [1.0])
    assert state.update(1, [0.5]).improved[0]


@pytest.mark.parametrize("baseline", [2.0, 0.2])
@pytest.mark.parametrize("patience", [1, 3])
def test_baseline_above_and_below_first_value(baseline, patience):
    """A baseline the values do not beat keeps ``wait`` counting even
    through improving epochs."""
    rng = np.random.default_rng(11)
    # falling from ~1: above baseline 0.2 for a while, always below 2.0
    seq = 1.0 - np.cumsum(rng.random((EPOCHS, G)) * 0.12, axis=0)
    seq[9:] = seq[8]
    cfg = dict(monitor="val_loss", patience=patience, min_delta=0.0,
               baseline=baseline)
    _check(cfg, seq)
    state = EarlyStopState(G, cfg)
    state.update(0, seq[0])
    # first value ~0.9..1.0: beats 2.0 (wait reset), not 0.2 (wait kept)
    assert (state.wait == (0 if baseline == 2.0 else 1)).all()


def test_auto_mode_on_accuracy_is_max():
    rng = np.random.default_rng(3)
    seq = rng.random((EPOCHS, G))
    for monitor in ("val_accuracy", "acc", "val_acc", "accuracy"):
        state = EarlyStopState(G, dict(monitor=monitor, patience=1))
        assert state.mode == "max"
        _check(dict(monitor=monitor, patience=1, mode="auto"), seq)
    assert EarlyStopState(G, dict(monitor="val_loss")).mode == "min"
    assert EarlyStopState(G, dict(monitor="val_accuracy", mode="min")).mode \
        == "min"


def test_patience_zero_stops_at_first_non_improving_epoch():
    state = EarlyStopState(2, dict(patience=0))
    vals = [[3.0, 3.0], [2.0, 2.0], [1.0, 2.5], [0.5, 0.1]]
    stops = [state.update(e, v).stop.tolist() for e, v in enumerate(vals)]
    assert stops == [[False, False], [False, False], [False, True],
                     [False, False]]
    assert state.stopped_epoch[1] == 2


def test_patience_one_matches_the_group_loop_for_one_model():
    """patience >= 1 with only monitor/patience/min_delta: a single
    model's decisions are those of the former group-wide loop."""
    rng = np.random.default_rng(8)
    for patience in (1, 2, 3):
        for _ in range(20):
            seq = rng.random(EPOCHS)
            min_delta = 0.05
            best, wait, old_stop = np.inf, 0, None
            for e, v in enumerate(seq):
                improved = v < best - min_delta
                best = min(best, v)
                wait = 0 if improved else wait + 1
                if e > 0 and wait >= patience:
                    old_stop = e
                    break
            state = EarlyStopState(
                1, dict(monitor="loss", patience=patience,
                        min_delta=min_delta)
            )
            new_stop = None
            for e, v in enumerate(seq):
                if state.update(e, [v]).stop[0]:
                    new_stop = e
                    break
            assert new_stop == old_stop


def test_monitor_resolution():
    assert resolve_monitor("loss", True) == "loss"
    assert resolve_monitor("val_loss", True) == "val_loss"
    assert resolve_monitor("val_loss", False) == "loss"
    assert resolve_monitor("accuracy", True) == "accuracy"
    assert resolve_monitor("acc", False) == "accuracy"
    assert resolve_monitor("val_accuracy", True) == "val_accuracy"
    assert resolve_monitor("val_acc", True) == "val_accuracy"
    assert resolve_monitor("val_acc", False) == "accuracy"
    assert resolve_monitor("mae", True) == "loss"
    hist = {"loss": [[1.0, 2.0]], "accuracy": [[0.5, 0.25]],
            "val_loss": [[3.0, 4.0]], "val_accuracy": [[0.75, 1.0]]}
    state = EarlyStopState(2, dict(monitor="val_accuracy"))
    assert state.monitored(hist).tolist() == [0.75, 1.0]
    del hist["val_loss"], hist["val_accuracy"]
    assert state.monitored(hist).tolist() == [0.5, 0.25]


def test_bad_mode_raises():
    with pytest.raises(ValueError):
        EarlyStopState(2, dict(mode="best"))


# ---- the parser --------------------------------------------------------
_KEY = "tensorflow.keras.callbacks.EarlyStopping"


def test_parser_three_key_config_is_unchanged():
    assert _parse_early_stopping(None) is None
    assert _parse_early_stopping(
        [{_KEY: {"monitor": "val_loss", "patience": 10}}]
    ) == {"monitor": "val_loss", "patience": 10, "min_delta": 0.0}


def test_parser_new_keys_only_when_given():
    assert _parse_early_stopping(
        [{_KEY: {"monitor": "loss", "patience": 2, "min_delta": 0.5,
                 "restore_best_weights": True}}]
    ) == {"monitor": "loss", "patience": 2, "min_delta": 0.5,
          "restore_best_weights": True}
    full = _parse_early_stopping(
        [{_KEY: {"monitor": "val_accuracy", "patience": 3,
                 "restore_best_weights": 1, "mode": "max",
                 "baseline": 1, "start_from_epoch": 4}}]
    )
    assert full == {"monitor": "val_accuracy", "patience": 3,
                    "min_delta": 0.0, "restore_best_weights": True,
                    "mode": "max", "baseline": 1.0, "start_from_epoch": 4}
    assert isinstance(full["baseline"], float)
    assert _parse_early_stopping(
        [{_KEY: {"patience": 1, "baseline": None}}]
    ) == {"monitor": "val_loss", "patience": 1, "min_delta": 0.0,
          "baseline": None}
    # what the parser gives is what the state takes
    state = EarlyStopState(3, full)
    assert (state.mode, state.baseline, state.start_from_epoch,
            state.restore_best_weights) == ("max", 1.0, 4, True)


def test_parser_bad_mode_raises():
    with pytest.raises(ValueError):
        _parse_early_stopping([{_KEY: {"mode": "lowest"}}])
