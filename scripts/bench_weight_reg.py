#!/usr/bin/env python3
"""Isolated timing of the regularized optimizer step and the penalty launch.

Builds the bench's LSTM pack (lstm_hourglass at 50 tags, lookback 144)
at G = 31 and G = 62, with an l1 and an l2 coefficient on every kernel
and recurrent kernel (biases unregularized), and times on its own flat
buffers one ``ops.optimizer_step`` (Adam, the bench's optimizer; the
step-counter bump launch included) in four arms: the unmasked
``adam_kernel``, the masked entry with every model active, the
regularized step with the same all-ones mask and the regularized step
without a mask; and, as a fifth arm, ``ops.weight_penalty`` alone (its
two launches). HIP events, 3 warm-up + 20 timed launches per arm, the
arms alternating launch by launch. Prints the median (min-max) in
microseconds per arm.

    python scripts/bench_weight_reg.py [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gordo_amd import ops  # noqa: E402
from gordo_amd.engine.pack import LSTMPack  # noqa: E402
from gordo_amd.engine.spec import LayerSpec, ModelSpec  # noqa: E402

WARMUP, TIMED = 3, 20
N_TAGS, LOOKBACK = 50, 144
UNITS = [42, 33, 25, 25, 33, 42]  # lstm_hourglass at 50 tags (bench.py)
L1, L2 = 1e-5, 1e-4


def bench_pack(G):
    spec = ModelSpec(
        model_type="lstm", n_features=N_TAGS, n_features_out=N_TAGS,
        layers=[
            LayerSpec(kind="lstm", units=u, return_sequences=(i != 5),
                      kernel_l1=L1, kernel_l2=L2, recurrent_l1=L1,
                      recurrent_l2=L2)
            for i, u in enumerate(UNITS)
        ] + [LayerSpec(kind="dense", units=N_TAGS, activation="linear",
                       kernel_l1=L1, kernel_l2=L2)],
        lookback_window=LOOKBACK,
    )
    return LSTMPack(spec, G=G, device="cuda", seeds=list(range(G)))


def time_arms(arms):
    """{name: [us per launch]}: arms alternate launch by launch."""
    times = {name: [] for name in arms}
    for it in range(WARMUP + TIMED):
        for name, fn in arms.items():
            start = torch.cuda.Event(enable_timing=True)
            end = torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            end.record()
            end.synchronize()
            if it >= WARMUP:
                times[name].append(start.elapsed_time(end) * 1e3)
    return times


def summary(values):
    return {"median_us": round(statistics.median(values), 2),
            "min_us": round(min(values), 2), "max_us": round(max(values), 2)}


def run(G):
    store = bench_pack(G).store
    store.g32.uniform_(-1e-3, 1e-3)
    all_on = store.model_mask([True] * G)
    reg = store.reg_table
    assert reg is not None

    def step(active, reg):
        segment_aware = active is not None or reg is not None
        return lambda: ops.optimizer_step(
            store.optimizer_kind, store.p32, store.g32, store.m, store.v,
            store.vhat, store.optimizer_params, 1, store.plp,
            step_buf=store.step_buf, active=active,
            segments=store.segments if segment_aware else None,
            reg=reg, G=G,
        )

    times = time_arms({
        "unmasked": step(None, None),
        "masked_all_active": step(all_on, None),
        "reg_all_active": step(all_on, reg),
        "reg_no_mask": step(None, reg),
        "penalty": lambda: ops.weight_penalty(
            store.p32, store.segments, reg, G),
    })
    out = {"G": G, "elements": int(store.p32.numel()),
           "segments": int(store.segments.shape[1]),
           "regularized_segments": int((reg != 0).any(dim=0).sum())}
    for name, vals in times.items():
        out[name] = summary(vals)
        print(f"G={G:3d} {name:20s} {out[name]['median_us']:8.2f} us "
              f"({out[name]['min_us']:.2f}-{out[name]['max_us']:.2f})")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="write the results as JSON")
    args = ap.parse_args()
    assert torch.cuda.is_available() and ops.hip_available()
    results = [run(G) for G in (31, 62)]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
