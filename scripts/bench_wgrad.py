#!/usr/bin/env python3
"""Isolated A/B timing of the grouped weight-grad kernels.

Times ``ops.grouped_wgrad_xh`` (and one dense ``grouped_linear_wgrad``
shape) with HIP events: 3 warm-up + 20 timed launches per arm, the 64x64
tile kernel (``GORDO_WGRAD_PIPE=0``) and the whole-tile kernel
alternating launch by launch. Shapes: every (F, H) of the bench's LSTM
pack (read from ``LSTMPack.lstm_meta``) at G = 31 and G = 62, B = 256,
T = 144; the ragged last batch of a fold; one dense shape.

Per shape it prints the median (min-max) in microseconds per arm, the
TB/s of unique operand bytes the medians imply, and the largest
old-vs-new difference against the fp32 bound of
``tests/gemm_cases.check_wgrad`` (oracle computed for the first and the
last group). ``--chunks 512,1024,...`` adds arms of the new kernel with
``GORDO_WGRAD_CHUNK`` forced, to choose the host's default.

    python scripts/bench_wgrad.py [--chunks LIST] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import gemm_cases as gc  # noqa: E402
from gordo_amd import ops  # noqa: E402
from gordo_amd.engine.pack import LSTMPack  # noqa: E402
from gordo_amd.engine.spec import LayerSpec, ModelSpec  # noqa: E402

WARMUP, TIMED = 3, 20
N_TAGS, LOOKBACK, BATCH = 50, 144, 256
UNITS = [42, 33, 25, 25, 33, 42]  # lstm_hourglass at 50 tags (bench.py)


def bench_lstm_shapes():
    spec = ModelSpec(
        model_type="lstm", n_features=N_TAGS, n_features_out=N_TAGS,
        layers=[
            LayerSpec(kind="lstm", units=u, return_sequences=(i != 5))
            for i, u in enumerate(UNITS)
        ] + [LayerSpec(kind="dense", units=N_TAGS, activation="linear")],
        lookback_window=LOOKBACK,
    )
    pack = LSTMPack(spec, G=1, device="cuda", seeds=[0])
    seen = []
    for fin, H, _rs in pack.lstm_meta:
        if (fin, H) not in seen:
            seen.append((fin, H))
    return seen


def set_arm(pipe, chunk):
    for name, val in (("GORDO_WGRAD_PIPE", pipe), ("GORDO_WGRAD_CHUNK", chunk)):
        if val is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = str(val)


def time_arms(call, arms):
    """arms: {name: (pipe, chunk)}. Alternates the arms launch by launch;
    returns {name: ([us...], launch record, outputs of the last launch)}."""
    times = {a: [] for a in arms}
    rec, outs = {}, {}
    for it in range(WARMUP + TIMED):
        for name, (pipe, chunk) in arms.items():
            set_arm(pipe, chunk)
            start = torch.cuda.Event(enable_timing=True)
            stop = torch.cuda.Event(enable_timing=True)
            start.record()
            out = call()
            stop.record()
            stop.synchronize()
            if it >= WARMUP:
                times[name].append(start.elapsed_time(stop) * 1e3)
            rec[name] = ops.last_wgrad_launch()
            outs[name] = out
    set_arm(None, None)
    return {a: (times[a], rec[a], outs[a]) for a in arms}


def oracle_check(A_of_group, dZ, old, new, groups):
    """|old - new| against the check_wgrad bound, on ``groups``."""
    worst = 0.0
    for g in groups:
        (want_W, atol_W), (want_b, atol_b) = gc.wgrad_oracle(
            A_of_group(g).float().cpu(), dZ[g:g + 1].float().cpu()
        )
        for o, n, want, atol in ((old[0], new[0], want_W, atol_W),
                                 (old[1], new[1], want_b, atol_b)):
            diff = (o[g:g + 1].double().cpu() - n[g:g + 1].double().cpu()).abs()
            bound = torch.clamp(2.0 ** -22 * want.abs(), min=atol)
            worst = max(worst, (diff / bound.clamp_min(1e-30)).max().item())
    return worst  # <= 1: inside the bound


def fmt(ts):
    return f"{statistics.median(ts):.1f} ({min(ts):.1f}-{max(ts):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", default="",
                    help="comma-separated GORDO_WGRAD_CHUNK values to add")
    ap.add_argument("--out", default=None, help="write JSON lines here")
    args = ap.parse_args()
    extra = [int(c) for c in args.chunks.split(",") if c]

    cases = []
    shapes = bench_lstm_shapes()
    for G in (31, 62):
        for F, H in shapes:
            cases.append(("xh", G, BATCH, LOOKBACK, F, H))
    F0, H0 = shapes[0]
    cases.append(("xh", 31, 24, LOOKBACK, F0, H0))    # ragged last batch
    cases.append(("dense", 63, 256, 1, 56, 32))       # G, M, -, K, N

    arms = {"old": (0, None), "new": (None, None)}
    for c in extra:
        arms[f"new@{c}"] = (None, c)

    rows = []
    gen = torch.Generator(device="cuda").manual_seed(0)

    def rnd(*shape):
        return (torch.rand(*shape, device="cuda", generator=gen) * 2 - 1).to(
            torch.bfloat16)

    for kind, G, B, T, F, H in cases:
        if kind == "xh":
            M, K, N = B * T, F + H, 4 * H
            seq, hs, dZ = rnd(G, M, F), rnd(G, B, T, H), rnd(G, M, N)

            def call():
                dWx, dWh, db = ops.grouped_wgrad_xh(seq, hs, dZ, T)
                return torch.cat([dWx, dWh], dim=1), db

            def A_of_group(g):
                h = hs[g:g + 1]
                hp = torch.cat([torch.zeros_like(h[:, :, :1]), h[:, :, :-1]],
                               dim=2).reshape(1, M, H)
                return torch.cat([seq[g:g + 1], hp], dim=2)
        else:
            M, K, N = B, F, H
            X, dZ = rnd(G, M, K), rnd(G, M, N)

            def call():
                return tuple(ops.grouped_linear_wgrad(X, dZ))

            def A_of_group(g):
                return X[g:g + 1]

        res = time_arms(call, arms)
        unique = 2.0 * G * M * (K + N)
        old, new = res["old"][2], res["new"][2]
        ratio = oracle_check(A_of_group, dZ, old, new, sorted({0, G - 1}))
        row = {
            "kind": kind, "G": G, "M": M, "K": K, "N": N, "T": T,
            "unique_MB": unique / 1e6,
            "old_vs_new_over_bound": ratio,
            "old_vs_new_max_abs": (old[0] - new[0]).abs().max().item(),
            "non_overlapping": max(res["new"][0]) < min(res["old"][0]),
        }
        for name, (ts, rec, _out) in res.items():
            row[name] = {
                "us": [round(t, 1) for t in ts], "launch": rec,
                "median_us": statistics.median(ts),
                "TBps": unique / statistics.median(ts) / 1e6,
            }
        rows.append(row)
        line = (f"{kind} G={G} M={M} K={K} N={N}: " + "  ".join(
            f"{a} {fmt(r[0])} us [{r[1]['family']} x{r[1]['chunks']}, "
            f"{unique / statistics.median(r[0]) / 1e6:.2f} TB/s]"
            for a, r in res.items()
        ) + f"  |old-new|/bound {ratio:.3f}"
            f"  new max < old min: {row['non_overlapping']}")
        print(line, flush=True)
        del res, old, new
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
