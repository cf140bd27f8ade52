"""Isolated two-step GRU scan launches beside the big-H LSTM scans of the
same shape (both take the x-side GEMM's output, both stream Wh from L2).

HIP events around the ``ops`` call, 3 warm-up + 20 timed launches per
arm, the two cells alternating launch by launch. Prints one JSON line
per arm and cell: median, min and max in microseconds, and the median
per timestep. The "public" rows are ``ops.gru_seq_fwd`` / ``gru_seq_bwd``
with their GEMMs (mx before the scan, dX after it).

    python scripts/bench_gru_big_scan.py [--G 31 --B 256 --T 144 --H 128 --F 56]
"""
import argparse
import json
import statistics

import torch

from gordo_amd import ops


def main():
    ap = argparse.ArgumentParser()
    for name, default in dict(G=31, B=256, T=144, H=128, F=56).items():
        ap.add_argument(f"--{name}", type=int, default=default)
    a = ap.parse_args()
    G, B, T, H, F = a.G, a.B, a.T, a.H, a.F
    gen = torch.Generator().manual_seed(0)

    def rnd(*shape, scale=1.0, dtype=torch.bfloat16):
        t = (torch.rand(*shape, generator=gen) * 2 - 1) * scale
        return t.to("cuda", dtype)

    x, d_full, d_last = rnd(G, B, T, F), rnd(G, B, T, H), rnd(G, B, H)
    Wx = rnd(G, F, 3 * H, scale=1.2 / F ** 0.5)
    Wh = rnd(G, H, 3 * H, scale=1.2 / H ** 0.5)
    b = rnd(G, 2, 3 * H, scale=0.1, dtype=torch.float32)
    mx = ops.grouped_linear_fwd(x.view(G, B * T, F), Wx, b[:, 0],
                                "linear").view(G, B, T, 3 * H)
    bh = b[:, 1].contiguous()
    hs, gacts = ops.gru_seq_fwd_big(mx, Wh, bh)
    Wh4 = rnd(G, H, 4 * H, scale=1.2 / H ** 0.5)
    xW = rnd(G, B, T, 4 * H, scale=0.6)
    _, cs4, gacts4 = ops.lstm_seq_fwd(xW, Wh4)
    arms = {
        "fwd train": (lambda: ops.gru_seq_fwd_big(mx, Wh, bh),
                      lambda: ops.lstm_seq_fwd(xW, Wh4)),
        "bwd full": (lambda: ops.gru_seq_bwd_big(d_full, gacts, hs, Wh, False),
                     lambda: ops.lstm_seq_bwd(d_full, gacts4, cs4, Wh4, False)),
        "bwd last": (lambda: ops.gru_seq_bwd_big(d_last, gacts, hs, Wh, True),
                     lambda: ops.lstm_seq_bwd(d_last, gacts4, cs4, Wh4, True)),
        "public fwd": (lambda: ops.gru_seq_fwd(x, Wx, Wh, b), None),
        "public bwd dX full": (
            lambda: ops.gru_seq_bwd(d_full, gacts, hs, Wh, False, Wx=Wx),
            None),
    }
    for arm, fns in arms.items():
        cells = {c: f for c, f in zip(("gru", "lstm"), fns) if f}
        times = {c: [] for c in cells}
        for it in range(23):
            for cell, fn in cells.items():
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if it >= 3:
                    times[cell].append(e0.elapsed_time(e1) * 1e3)
        for cell, ts in times.items():
            launch = (ops.last_gru_launch() if cell == "gru"
                      else ops.last_scan_launch())
            med = statistics.median(ts)
            print(json.dumps(dict(
                arm=arm, cell=cell, family=launch["family"],
                rows=launch["rows"], us_median=round(med, 1),
                us_min=round(min(ts), 1), us_max=round(max(ts), 1),
                us_per_step=round(med / T, 2))))


if __name__ == "__main__":
    main()
