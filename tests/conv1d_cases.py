"""The one case table of the grouped Conv1D tests: the CPU validation
of the oracles (test_conv1d_oracle.py) and the device tests
(test_conv1d_gpu.py). Bounds and input builders are those of
gemm_cases.py.

Every row is the smallest shape that reaches what its last column
names. T = 1, 5 and 70 plan the 16-row tile, T = 17 and 96 the 32-row
one (a tie in padded rows goes to the larger tile), T = 64 the 64-row one.
"""
import functools

import torch

from gemm_cases import rand, rand_f32
from gordo_amd.ops import reference as ref

# (G, B, T, Cin, Cout, k, d, padding, act), rows, taps_resident, wgrad
# chunks, what it reaches
CASES = [
    ((1, 1, 1, 8, 8, 1, 1, "same", "linear"), 16, True, 1,
     "smallest: one row, one tap"),
    ((3, 5, 5, 8, 8, 2, 1, "same", "relu"), 16, True, 1,
     "even k under 'same': one zero row at the END of the window only"),
    ((3, 5, 17, 24, 40, 3, 2, "causal", "tanh"), 32, True, 1,
     "ragged 32-row tile, K tail (24 of 32), half n-fragment (40)"),
    ((1, 1, 70, 64, 128, 5, 4, "same", "sigmoid"), 16, True, 1,
     "five tiles, both n-fragments of every wave"),
    ((3, 5, 5, 128, 64, 2, 64, "causal", "linear"), 16, True, 1,
     "(k-1)*d = 64: the halo is longer than T, tap 0 reads zeros only"),
    ((1, 1, 70, 128, 128, 8, 1, "causal", "tanh"), 16, False, 1,
     "k = 8 at 128 x 128: the two-tap ring, four wgrad tap groups"),
    ((1, 40, 17, 24, 40, 3, 1, "same", "linear"), 32, True, 2,
     "two wgrad chunks (atomics), 40 one-item forward workgroups"),
    ((2, 3, 96, 40, 24, 2, 4, "causal", "linear"), 32, True, 1,
     "three full 32-row tiles per window"),
    ((2, 3, 64, 8, 8, 3, 1, "same", "relu"), 64, True, 1,
     "the 64-row tile"),
    ((3, 70, 70, 8, 16, 2, 1, "same", "relu"), 16, True, 9,
     "three items per workgroup: image and staging buffers both reused"),
    ((1, 1100, 5, 128, 128, 8, 1, "causal", "linear"), 16, False, 11,
     "three items per workgroup on the ring (restaged per item)"),
]
IDS = [f"{i}-" + "x".join(map(str, c[0][:7])) + f"-{c[0][7]}-{c[0][8]}"
       for i, c in enumerate(CASES)]
# the rows of the further properties: NaN containment, determinism,
# exact lattice sums (one chunk and two)
NAN_ROW, LATTICE_ROWS = 2, (2, 6)


@functools.lru_cache(maxsize=None)
def reference(i):
    """Inputs of case i (bf16 values held in fp32; the bias is fp32) and
    the three oracles on them, built once."""
    (G, B, T, Cin, Cout, k, d, padding, act) = CASES[i][0]
    x = rand(G, B, T, Cin, seed=10 * i)
    W = rand(G, k, Cin, Cout, seed=10 * i + 1, scale=(k * Cin) ** -0.5)
    b = rand_f32(G, Cout, seed=10 * i + 2, scale=0.5)
    dZ = rand(G, B, T, Cout, seed=10 * i + 3)
    return dict(
        x=x, W=W, b=b, dZ=dZ,
        fwd=ref.conv1d_fwd_ref(x, W, b, act, padding, d),
        bwd_data=ref.conv1d_bwd_data_ref(dZ, W, padding, d),
        wgrad=ref.conv1d_wgrad_ref(x, dZ, k, padding, d),
    )
