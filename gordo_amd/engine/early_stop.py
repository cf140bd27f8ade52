"""
Per-model EarlyStopping bookkeeping for a pack of G models.

The rule is Keras 3's ``EarlyStopping`` callback, applied to every
model of the pack on its own, vectorised over G. With monitored value
``v`` at the end of epoch ``e``:

1. ``e < start_from_epoch``: nothing happens.
2. Otherwise, with ``restore_best_weights`` and no best weights held
   yet, the current weights are captured (``best_epoch = e``).
3. ``wait`` is incremented.
4. If ``v`` improved on ``best``: ``best = v``, ``best_epoch = e``, the
   weights are captured (``restore_best_weights``), ``wait = 0`` unless
   a ``baseline`` is set that ``v`` does not improve on — and the model
   does not stop this epoch.
5. Otherwise the model stops when ``wait >= patience`` and ``e > 0``.

``improved(v, ref)`` is ``v + min_delta < ref`` for mode ``min`` and
``v - min_delta > ref`` for ``max``; a NaN never improves. ``auto``
resolves to ``max`` for a monitor that ends in ``acc``/``accuracy``.

For ``patience >= 1`` and only ``monitor``/``patience``/``min_delta``
set, the decisions for a single model are those of the earlier
group-wide loop. For ``patience = 0`` that loop stopped after epoch 1
even while improving; this rule stops at the first epoch that does not
improve.
"""
from __future__ import annotations

from typing import Any, Dict, NamedTuple, Optional

import numpy as np

MODES = ("auto", "min", "max")


class EarlyStopUpdate(NamedTuple):
    """Per-model bool masks of one ``EarlyStopState.update``."""

    stop: np.ndarray      # stops at this epoch
    improved: np.ndarray  # improved on its best value
    capture: np.ndarray   # its current weights become its best weights


def resolve_monitor(monitor: str, has_validation: bool) -> str:
    """History key a monitor name reads: loss / accuracy, their val_*
    forms when a validation split exists (else the train quantity), and
    ``loss`` for any other name."""
    name = str(monitor)
    val = name.startswith("val_")
    base = name[4:] if val else name
    if base in ("acc", "accuracy"):
        key = "accuracy"
    else:
        key = "loss"
        val = name.startswith("val")  # any val* name reads val_loss
    return "val_" + key if (val and has_validation) else key


class EarlyStopState:
    """``update(epoch, values[G])`` applies the rule to every model that
    has not ended and returns an ``EarlyStopUpdate``."""

    def __init__(self, G: int, cfg: Optional[Dict[str, Any]] = None):
        cfg = dict(cfg or {})
        self.G = int(G)
        self.monitor = str(cfg.get("monitor", "loss"))
        self.patience = int(cfg.get("patience", 0))
        self.min_delta = abs(float(cfg.get("min_delta", 0.0)))
        mode = str(cfg.get("mode", "auto"))
        if mode not in MODES:
            raise ValueError(
                f"EarlyStopping mode must be one of {MODES}, got {mode!r}"
            )
        if mode == "auto":
            mode = (
                "max" if self.monitor.endswith(("acc", "accuracy")) else "min"
            )
        self.mode = mode
        baseline = cfg.get("baseline")
        self.baseline = None if baseline is None else float(baseline)
        self.restore_best_weights = bool(cfg.get("restore_best_weights", False))
        self.start_from_epoch = int(cfg.get("start_from_epoch", 0))
        self.best = np.full(G, np.inf if mode == "min" else -np.inf)
        self.wait = np.zeros(G, dtype=np.int64)
        self.best_epoch = np.zeros(G, dtype=np.int64)
        self.stopped_epoch = np.zeros(G, dtype=np.int64)
        self.has_best = np.zeros(G, dtype=bool)  # best weights are held
        self.ended = np.zeros(G, dtype=bool)

    def _improved(self, v: np.ndarray, ref) -> np.ndarray:
        # comparisons with NaN are False: a NaN never improves
        with np.errstate(invalid="ignore"):
            if self.mode == "min":
                return (v + self.min_delta) < ref
            return (v - self.min_delta) > ref

    def monitored(self, history: Dict[str, list]) -> np.ndarray:
        """The monitored values [G] of the latest history row."""
        key = resolve_monitor(self.monitor, "val_loss" in history)
        return np.asarray(history[key][-1], dtype=np.float64)

    def update(self, epoch: int, values) -> EarlyStopUpdate:
        v = np.asarray(values, dtype=np.float64)
        none = np.zeros(self.G, dtype=bool)
        if epoch < self.start_from_epoch:
            return EarlyStopUpdate(none, none.copy(), none.copy())
        live = ~self.ended
        capture = none.copy()
        if self.restore_best_weights:
            first = live & ~self.has_best
            self.best_epoch[first] = epoch
            capture |= first
        self.wait[live] += 1
        improved = live & self._improved(v, self.best)
        self.best[improved] = v[improved]
        self.best_epoch[improved] = epoch
        if self.restore_best_weights:
            capture |= improved
            self.has_best |= capture
        reset = improved
        if self.baseline is not None:
            reset = improved & self._improved(v, self.baseline)
        self.wait[reset] = 0
        stop = live & ~improved & (self.wait >= self.patience)
        if epoch <= 0:
            stop = none.copy()
        self.stopped_epoch[stop] = epoch
        self.ended |= stop
        return EarlyStopUpdate(stop, improved, capture)
