"""Training controls: EarlyStopping callbacks, validation_split and the
engine's val_loss history — the keras-config surface on the MI355X
engine.

Run: python examples/training_controls.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from gordo_amd.machine.model.models import KerasAutoEncoder


def main():
    rng = np.random.default_rng(0)
    X = rng.random((512, 16))

    model = KerasAutoEncoder(
        kind="feedforward_hourglass",
        epochs=100,                  # ceiling; EarlyStopping decides
        batch_size=64,
        validation_split=0.2,        # keras semantics: last 20% held out
        callbacks=[{
            "tensorflow.keras.callbacks.EarlyStopping": {
                "monitor": "val_loss",
                "patience": 3,
                "min_delta": 1e-3,
            }
        }],
    )
    model.fit(X)
    hist = model.get_metadata()["history"]
    print(f"stopped after {len(hist['loss'])} epochs (ceiling was 100)")
    print(f"final loss {hist['loss'][-1]:.5f}  "
          f"val_loss {hist['val_loss'][-1]:.5f}")
    assert len(hist["loss"]) < 100
    assert np.isfinite(hist["val_loss"]).all()
    per_model_stopping()


def per_model_stopping():
    """In a pack every model stops at its own patience: a noise model
    stalls long before a sine model does, and each keeps the history
    (and weights) of its own run. ``restore_best_weights`` goes back to
    each model's best epoch."""
    import torch

    from gordo_amd.engine.pack import DensePack
    from gordo_amd.machine.model.models import _history_for_model

    spec = KerasAutoEncoder(kind="feedforward_hourglass").build_pack_spec(8, 8)
    t = np.linspace(0, 12, 512)
    sines = np.stack([np.sin(t + p) for p in np.linspace(0, 2, 8)], axis=1)
    noise = np.random.default_rng(1).random((512, 8)) * 0.5
    X = torch.tensor(np.stack([noise, 2 * sines]).astype("float32"))
    pack = DensePack(spec, G=2, seeds=[1, 2])
    X = X.to(pack.device)
    hist = pack.fit(
        X, X.clone(), epochs=60, batch_size=64,
        early_stopping={"monitor": "loss", "patience": 2, "min_delta": 5e-3,
                        "restore_best_weights": True},
    )
    print(f"pack ran {len(hist['loss'])} epochs; per model: "
          f"{hist.epochs_run}, best epochs {hist.best_epoch}")
    # (epoch, G_before, G_after) per compaction; a pack of 2 never compacts
    print(f"compactions: {hist.compactions}")
    for g in range(2):
        assert len(_history_for_model(hist, g)["loss"]) == hist.epochs_run[g]


if __name__ == "__main__":
    main()
