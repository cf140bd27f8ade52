"""Isolated GRU scan launches beside the LSTM scans of the same shape.

HIP events around the ``ops`` call, 3 warm-up + 20 timed launches per
arm, the two cells alternating launch by launch. Prints one JSON line
per arm: median, min and max in microseconds.

    python scripts/bench_gru_scan.py [--G 31 --B 256 --T 144 --H 48 --F 56]
"""
import argparse
import json
import statistics

import torch

from gordo_amd import ops


def main():
    ap = argparse.ArgumentParser()
    for name, default in dict(G=31, B=256, T=144, H=48, F=56).items():
        ap.add_argument(f"--{name}", type=int, default=default)
    a = ap.parse_args()
    G, B, T, H, F = a.G, a.B, a.T, a.H, a.F
    gen = torch.Generator().manual_seed(0)

    def rnd(*shape, scale=1.0, dtype=torch.bfloat16):
        t = (torch.rand(*shape, generator=gen) * 2 - 1) * scale
        return t.to("cuda", dtype)

    x, d_full, d_last = rnd(G, B, T, F), rnd(G, B, T, H), rnd(G, B, H)
    cells = {}
    for cell, ng in (("gru", 3), ("lstm", 4)):
        Wx = rnd(G, F, ng * H, scale=1.2 / F ** 0.5)
        Wh = rnd(G, H, ng * H, scale=1.2 / H ** 0.5)
        if cell == "gru":
            b = rnd(G, 2, ng * H, scale=0.1, dtype=torch.float32)
            hs, gacts = ops.gru_seq_fwd(x, Wx, Wh, b)
            cells[cell] = {
                "fwd train": lambda x=x, Wx=Wx, Wh=Wh, b=b:
                    ops.gru_seq_fwd(x, Wx, Wh, b),
                "bwd dX full": lambda g=gacts, h=hs, Wx=Wx, Wh=Wh:
                    ops.gru_seq_bwd(d_full, g, h, Wh, False, Wx=Wx),
                "bwd dX last": lambda g=gacts, h=hs, Wx=Wx, Wh=Wh:
                    ops.gru_seq_bwd(d_last, g, h, Wh, True, Wx=Wx),
                "bwd full": lambda g=gacts, h=hs, Wh=Wh:
                    ops.gru_seq_bwd(d_full, g, h, Wh, False),
            }
        else:
            b = rnd(G, ng * H, scale=0.1, dtype=torch.float32)
            hs, cs, gacts = ops.lstm_seq_fwd_fused(x, Wx, Wh, b)
            cells[cell] = {
                "fwd train": lambda x=x, Wx=Wx, Wh=Wh, b=b:
                    ops.lstm_seq_fwd_fused(x, Wx, Wh, b),
                "bwd dX full": lambda g=gacts, c=cs, Wx=Wx, Wh=Wh:
                    ops.lstm_seq_bwd_fused(d_full, g, c, Wh, Wx, False),
                "bwd dX last": lambda g=gacts, c=cs, Wx=Wx, Wh=Wh:
                    ops.lstm_seq_bwd_fused(d_last, g, c, Wh, Wx, True),
                "bwd full": lambda g=gacts, c=cs, Wh=Wh:
                    ops.lstm_seq_bwd_v3(d_full, g, c, Wh, False),
            }
    for arm in cells["gru"]:
        times = {"gru": [], "lstm": []}
        for it in range(23):
            for cell in ("gru", "lstm"):
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                cells[cell][arm]()
                e1.record()
                e1.synchronize()
                if it >= 3:
                    times[cell].append(e0.elapsed_time(e1) * 1e3)
        for cell, ts in times.items():
            launch = (ops.last_gru_launch() if cell == "gru"
                      else ops.last_scan_launch())
            print(json.dumps(dict(
                arm=arm, cell=cell, family=launch["family"],
                rows=launch["rows"], us_median=round(statistics.median(ts), 1),
                us_min=round(min(ts), 1), us_max=round(max(ts), 1))))


if __name__ == "__main__":
    main()
