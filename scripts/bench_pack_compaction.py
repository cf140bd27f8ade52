#!/usr/bin/env python3
"""Wall time of an early-stopping fit with and without pack compaction.

Builds the bench's LSTM pack (lstm_hourglass at 50 tags, lookback 144)
at G = 62 on synthetic series of which three quarters stall: uniform
noise for those, large sines for the rest. Fits it with EarlyStopping
(monitor loss, patience 1, min_delta 0.01) and reports the wall time of
``fit``, HIP-synchronised: one warm-up fit, then ``--fits`` timed fits,
each on a fresh pack from the same parameter snapshot. Prints one JSON
line with the times, their median and min-max, ``epochs_run`` (with its
histogram and the ideal ratio sum(epochs_run) / (G * max(epochs_run)))
and the compactions of the last fit.

``GORDO_PACK_COMPACT=0`` gives the arm without compaction. ``--root``
imports ``gordo_amd`` from another checkout (one built from the parent
commit, for the comparison across commits; a tree without compaction
reports ``compactions: null``).

    python scripts/bench_pack_compaction.py [--fits 3] [--root DIR]
"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

N_TAGS, LOOKBACK, G = 50, 144, 62
UNITS = [42, 33, 25, 25, 33, 42]  # lstm_hourglass at 50 tags (bench.py)
ROWS, BATCH, EPOCHS = 1440, 256, 12
ES = {"monitor": "loss", "patience": 1, "min_delta": 0.01}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--fits", type=int, default=3, help="timed fits")
    ap.add_argument("--root", default=None,
                    help="checkout to import gordo_amd from")
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    root = os.path.abspath(args.root) if args.root else os.path.dirname(
        os.path.dirname(os.path.abspath(__file__))
    )
    sys.path.insert(0, root)

    import numpy as np
    import torch

    from gordo_amd import ops
    from gordo_amd.engine.pack import LSTMPack
    from gordo_amd.engine.spec import LayerSpec, ModelSpec

    assert torch.cuda.is_available() and ops.hip_available()
    spec = ModelSpec(
        model_type="lstm", n_features=N_TAGS, n_features_out=N_TAGS,
        layers=[
            LayerSpec(kind="lstm", units=u, return_sequences=(i != 5))
            for i, u in enumerate(UNITS)
        ] + [LayerSpec(kind="dense", units=N_TAGS, activation="linear")],
        lookback_window=LOOKBACK,
    )
    t = np.linspace(0, 60, ROWS)
    series = []
    for g in range(G):
        if g % 4 == 3:  # one quarter keeps improving
            series.append(np.stack(
                [np.sin((1 + g / G) * t + p) * 3
                 for p in np.linspace(0, 3, N_TAGS)], axis=1,
            ))
        else:
            series.append(
                np.random.default_rng(g).random((ROWS, N_TAGS)) * 0.5
            )
    X = torch.tensor(np.stack(series).astype("float32"), device="cuda")
    seeds = list(range(G))
    snapshot = LSTMPack(spec, G=G, device="cuda", seeds=seeds).store.p32.clone()

    times, hist = [], None
    for it in range(1 + args.fits):
        pack = LSTMPack(spec, G=G, device="cuda", seeds=seeds,
                        init_p32=snapshot)
        torch.cuda.synchronize()
        start = time.perf_counter()
        hist = pack.fit(X, X.clone(), epochs=EPOCHS, batch_size=BATCH,
                        shuffle=True, early_stopping=ES)
        torch.cuda.synchronize()
        if it >= 1:
            times.append(time.perf_counter() - start)
        pack.release_graphs()
        del pack
    runs = hist.epochs_run
    print(json.dumps({
        "label": args.label, "root": root,
        "compact_env": os.environ.get("GORDO_PACK_COMPACT"),
        "fit_s": [round(v, 4) for v in times],
        "median_s": round(statistics.median(times), 4),
        "min_s": round(min(times), 4), "max_s": round(max(times), 4),
        "epochs_run": runs,
        "epochs_run_histogram": dict(sorted(collections.Counter(runs).items())),
        "ideal_ratio": round(sum(runs) / (G * max(runs)), 4),
        "compactions": getattr(hist, "compactions", None),
    }))


if __name__ == "__main__":
    main()
