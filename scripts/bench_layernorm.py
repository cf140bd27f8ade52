"""Isolated grouped LayerNormalization launches beside
``torch.nn.functional.layer_norm`` looped over the G models on the same
tensors (bf16 activations, fp32 gamma / beta; its backward is
``torch.ops.aten.native_layer_norm_backward`` per model).

HIP events around the call, 3 warm-up + 20 timed launches per arm, the
two arms alternating launch by launch. Prints one JSON line per kernel
and arm: median, min and max in microseconds and the achieved bytes/s
over the operation's compulsory traffic (each operand once).

    python scripts/bench_layernorm.py
"""
import json
import statistics

import torch
import torch.nn.functional as F

from gordo_amd import ops

SHAPES = [(31, 256, 56, 50), (31, 256, 256, 256)]  # (G, B, Fp, real_f)
EPS = 1e-3


def main():
    gen = torch.Generator().manual_seed(0)
    for G, B, Fp, real_f in SHAPES:
        x = torch.randn(G, B, Fp, generator=gen).to("cuda", torch.bfloat16)
        dy = torch.randn(G, B, Fp, generator=gen).to("cuda", torch.bfloat16)
        gamma = torch.randn(G, Fp, generator=gen).cuda()
        beta = torch.randn(G, Fp, generator=gen).cuda()
        _y, mean, rstd = ops.layer_norm_fwd(x, gamma, beta, real_f, EPS)
        # the torch arm normalises all Fp columns: same traffic, its own
        # statistics
        gb, bb = gamma.bfloat16(), beta.bfloat16()
        stats = [torch.ops.aten.native_layer_norm(x[g], (Fp,), gb[g], bb[g],
                                                  EPS)[1:] for g in range(G)]

        def torch_fwd():
            return [F.layer_norm(x[g], (Fp,), gb[g], bb[g], EPS)
                    for g in range(G)]

        def torch_bwd():
            return [torch.ops.aten.native_layer_norm_backward(
                dy[g], x[g], (Fp,), stats[g][0], stats[g][1], gb[g], bb[g],
                (True, True, True)) for g in range(G)]

        act = 2 * G * B * Fp
        arms = {
            "fwd": (lambda: ops.layer_norm_fwd(x, gamma, beta, real_f, EPS),
                    torch_fwd, 2 * act + 8 * G * Fp + 8 * G * B),
            "bwd": (lambda: ops.layer_norm_bwd(dy, x, mean, rstd, gamma,
                                               real_f),
                    torch_bwd, 3 * act + 12 * G * Fp + 8 * G * B),
        }
        for kernel, (hip_fn, torch_fn, nbytes) in arms.items():
            cells = {"hip": hip_fn, "torch": torch_fn}
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
            hip_fn()
            plan = ops.last_layer_norm_launch()
            for cell, ts in times.items():
                med = statistics.median(ts)
                print(json.dumps(dict(
                    kernel=kernel, arm=cell, shape=[G, B, Fp, real_f],
                    plan=plan if cell == "hip" else None,
                    us_median=round(med, 1), us_min=round(min(ts), 1),
                    us_max=round(max(ts), 1),
                    gbytes_per_s=round(nbytes / med * 1e-3, 1))), flush=True)


if __name__ == "__main__":
    main()
