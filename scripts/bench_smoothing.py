#!/usr/bin/env python3
"""Serving-path timing of device smoothing against pandas smoothing.

For each smoothing method (smm, sma, ewma) and each request shape
(n rows, F tags, window) in {(512, 50, 144), (1440, 50, 144),
(4320, 50, 144)} this times ``DiffBasedAnomalyDetector.anomaly(X, y)``
end to end (H2D, kernels, D2H and frame assembly included; the base
estimator is a MinMaxScaler, so the model itself costs nothing) in two
arms that alternate call by call in one process:

  pandas   GORDO_DEVICE_SMOOTH=0: raw families on the device, smoothing
           by pandas on the host
  device   the raw families stay resident and ops.smooth smooths them

5 warm-up and 20 timed calls per arm; prints the median and the
interquartile range in milliseconds. Then the kernel alone on the
serving matrix [2F+2, n] (HIP events, 5 + 20 launches), in
microseconds.

    python scripts/bench_smoothing.py [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
import torch  # noqa: E402
from sklearn.preprocessing import MinMaxScaler  # noqa: E402

from gordo_amd import ops  # noqa: E402
from gordo_amd.machine.model.anomaly.diff import (  # noqa: E402
    DiffBasedAnomalyDetector,
)

WARMUP, TIMED = 5, 20
SHAPES = ((512, 50, 144), (1440, 50, 144), (4320, 50, 144))
METHODS = ("smm", "sma", "ewma")
ARMS = {"pandas": "0", "device": "1"}


def quartiles(values):
    q1, med, q3 = statistics.quantiles(values, n=4)
    return {"median": round(med, 3), "iqr": round(q3 - q1, 3)}


def request(n, F, window, method):
    rng = np.random.default_rng([n, F, window])
    cols = [f"tag-{i}" for i in range(F)]
    index = pd.date_range("2020-01-01", periods=n, freq="10min")
    X = pd.DataFrame(rng.random((n, F)), columns=cols, index=index)
    y = X + rng.normal(0, 0.05, size=(n, F))
    det = DiffBasedAnomalyDetector(
        base_estimator=MinMaxScaler(), require_thresholds=False,
        window=window, smoothing_method=method,
    )
    det.fit(X, y)
    return det, X, y


def time_anomaly(det, X, y, method):
    """{arm: [ms per call]}: the arms alternate call by call."""
    times = {arm: [] for arm in ARMS}
    for it in range(WARMUP + TIMED):
        for arm, switch in ARMS.items():
            os.environ["GORDO_DEVICE_SMOOTH"] = switch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            det.anomaly(X, y)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if arm == "device":
                assert ops.last_smooth_launch()["method"] == method
            if it >= WARMUP:
                times[arm].append(dt)
    os.environ.pop("GORDO_DEVICE_SMOOTH", None)
    return times


def time_kernel(n, F, window, method):
    """[us per launch] of ops.smooth on a resident [2F+2, n] matrix."""
    M = torch.rand(2 * F + 2, n, device="cuda")
    out = []
    for it in range(WARMUP + TIMED):
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        start.record()
        ops.smooth(M, window, method)
        end.record()
        end.synchronize()
        if it >= WARMUP:
            out.append(start.elapsed_time(end) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="write the results as JSON")
    args = ap.parse_args()
    assert torch.cuda.is_available() and ops.hip_available()
    results = []
    for method in METHODS:
        for n, F, window in SHAPES:
            det, X, y = request(n, F, window, method)
            arms = {a: quartiles(v)
                    for a, v in time_anomaly(det, X, y, method).items()}
            kern = quartiles(time_kernel(n, F, window, method))
            ratio = arms["pandas"]["median"] / arms["device"]["median"]
            margin = arms["pandas"]["median"] - arms["device"]["median"]
            wins = margin > max(arms["pandas"]["iqr"], arms["device"]["iqr"])
            results.append({
                "method": method, "n": n, "F": F, "window": window,
                "anomaly_ms": arms, "kernel_us": kern,
                "ratio": round(ratio, 2), "device_wins": bool(wins),
            })
            print(
                f"{method:5s} n={n:5d} F={F} w={window}: pandas "
                f"{arms['pandas']['median']:8.3f} ms (IQR "
                f"{arms['pandas']['iqr']:.3f}) device "
                f"{arms['device']['median']:8.3f} ms (IQR "
                f"{arms['device']['iqr']:.3f}) ratio {ratio:5.2f} "
                f"{'win' if wins else 'NO WIN'}; kernel "
                f"{kern['median']:.1f} us (IQR {kern['iqr']:.1f})",
                flush=True,
            )
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
