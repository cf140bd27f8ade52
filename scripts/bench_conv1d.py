"""Isolated grouped Conv1D launches beside the same operation through
torch-ROCm: ``torch.nn.functional.conv1d`` (and its input / weight
gradients) with ``groups=G`` on the channels-first view, bf16, including
the layout copies of the activations it needs. The weights of the torch
arm are laid out once, outside the timed region.

HIP events around the call, 3 warm-up + 20 timed launches per arm, the
two arms alternating launch by launch. Prints one JSON line per kernel
and arm: median, min and max in microseconds and the achieved bytes/s
over the operation's compulsory traffic (each operand once).

    python scripts/bench_conv1d.py [--G 31 --B 256 --T 144]
"""
import argparse
import json
import statistics

import torch
import torch.nn.functional as F

from gordo_amd import ops

SHAPES = [(56, 48, 3, 1), (48, 48, 2, 16)]  # (Cin, Cout, k, d)


def main():
    ap = argparse.ArgumentParser()
    for name, default in dict(G=31, B=256, T=144).items():
        ap.add_argument(f"--{name}", type=int, default=default)
    ap.add_argument("--padding", default="same")
    a = ap.parse_args()
    G, B, T, padding = a.G, a.B, a.T, a.padding
    gen = torch.Generator().manual_seed(0)

    def rnd(*shape, scale=1.0, dtype=torch.bfloat16):
        t = (torch.rand(*shape, generator=gen) * 2 - 1) * scale
        return t.to("cuda", dtype)

    for Cin, Cout, k, d in SHAPES:
        x, dZ = rnd(G, B, T, Cin), rnd(G, B, T, Cout)
        W = rnd(G, k, Cin, Cout, scale=(k * Cin) ** -0.5)
        b = rnd(G, Cout, scale=0.1, dtype=torch.float32)
        halo = (k - 1) * d
        left = ops.reference.conv1d_left(k, d, padding)
        # torch: [G*Cout, Cin, k] weights, [B, G*C, T] activations
        w_t = W.permute(0, 3, 2, 1).reshape(G * Cout, Cin, k).contiguous()
        b_t = b.reshape(-1).to(torch.bfloat16)

        def cf(t):  # [G,B,T,C] -> padded channels-first [B, G*C, T + halo]
            return F.pad(t.permute(1, 0, 3, 2).reshape(B, -1, T),
                         (left, halo - left))

        def cl(t, C):  # [B, G*C, T] -> [G,B,T,C]
            return t.reshape(B, G, C, T).permute(1, 0, 3, 2).contiguous()

        def torch_fwd():
            return cl(F.conv1d(cf(x), w_t, b_t, dilation=d, groups=G), Cout)

        def torch_bwd_data():
            g = dZ.permute(1, 0, 3, 2).reshape(B, G * Cout, T)
            dx = torch.nn.grad.conv1d_input(
                (B, G * Cin, T + halo), w_t, g, dilation=d, groups=G)
            return cl(dx[:, :, left:left + T], Cin)

        def torch_wgrad():
            g = dZ.permute(1, 0, 3, 2).reshape(B, G * Cout, T)
            dw = torch.nn.grad.conv1d_weight(
                cf(x), w_t.shape, g, dilation=d, groups=G)
            return dw, g.float().sum(dim=(0, 2))

        act_bytes = 2 * G * B * T
        w_bytes = 2 * G * k * Cin * Cout
        arms = {
            "fwd": (lambda: ops.conv1d_fwd(x, W, b, "linear", padding, d),
                    torch_fwd, act_bytes * (Cin + Cout) + w_bytes),
            "bwd_data": (lambda: ops.conv1d_bwd_data(dZ, W, padding, d),
                         torch_bwd_data, act_bytes * (Cin + Cout) + w_bytes),
            "wgrad": (lambda: ops.conv1d_wgrad(x, dZ, k, padding, d),
                      torch_wgrad, act_bytes * (Cin + Cout) + 2 * w_bytes),
        }
        for kernel, (hip_fn, torch_fn, nbytes) in arms.items():
            cells = {"hip": hip_fn, "torch": torch_fn}
            try:
                torch_fn()
                torch.cuda.synchronize()
            except Exception as e:  # an operation torch-ROCm cannot run
                print(json.dumps(dict(kernel=kernel, arm="torch",
                                      shape=[Cin, Cout, k, d],
                                      error=str(e)[:200])))
                del cells["torch"]
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
            plan = ops.last_conv1d_launch()
            for cell, ts in times.items():
                med = statistics.median(ts)
                print(json.dumps(dict(
                    kernel=kernel, arm=cell, shape=[Cin, Cout, k, d],
                    plan=plan if cell == "hip" else None,
                    us_median=round(med, 1), us_min=round(min(ts), 1),
                    us_max=round(max(ts), 1),
                    gbytes_per_s=round(nbytes / med * 1e-3, 1))), flush=True)


if __name__ == "__main__":
    main()
