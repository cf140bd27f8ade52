#!/usr/bin/env python3
"""
Flagship benchmark: machines built/hour on the 1000-machine mixed
feedforward/LSTM fleet config (BASELINE.json config #4), weak-scaled at
125 machines per GPU (N=8 GPUs -> the full 1000-machine config).

One step = one complete build of this rank's fleet shard: synthetic
sine-tag data fetch, TimeSeriesSplit(3) cross-validation (3 fold fits +
scoring + DiffBased thresholds), the final full fit, metadata assembly
and model serialization — i.e. exactly what `gordo build` does per
machine, through the packed grouped-MFMA engine.

Contract (driver): python bench.py --gpus N --steps K --warmup W
  * launched under torch.distributed.run for N>1 (one rank per GPU,
    RCCL); reads RANK/LOCAL_RANK/WORLD_SIZE from env.
  * W untimed warmup steps, then exactly K timed steps bracketed by
    barrier + torch.cuda.synchronize; MAX elapsed over ranks; rank 0
    prints ONE JSON line.
  * --dump-outputs DIR writes what the last timed step produced (trained
    weights, loss histories, anomaly thresholds, CV scores) as
    DIR/<name>.npy so two builds of the project can be compared output
    for output; the inputs are a pure function of the arguments.
  * --full is reserved for measurements beyond the headline figure; a
    plain run does only setup, warmup, the timed steps and the result
    line. Today it adds the per-phase build ledger (as --verbose).
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

REPO_ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO_ROOT)

N_TAGS = 50
ROWS_DAYS = 30          # 30 days @ 10min = 4320 rows
LOOKBACK = 144
EPOCHS = 5
BATCH_DENSE = 256
BATCH_LSTM = 256
MACHINES_PER_GPU = 125  # x8 GPUs = the 1000-machine config
DUMP_BYTES_MAX = 64 << 20  # --dump-outputs budget over all arrays


def make_machine_cfg(i: int, kind: str) -> dict:
    tags = [f"sine-{i}-{j}" for j in range(N_TAGS)]
    dataset = {
        "type": "SineWaveDataset",
        "tag_list": tags,
        "train_start_date": "2019-01-01T00:00:00+00:00",
        "train_end_date": f"2019-01-{1 + ROWS_DAYS:02d}T00:00:00+00:00",
    }
    if kind == "lstm":
        model = {
            "gordo_amd.machine.model.anomaly.diff.DiffBasedAnomalyDetector": {
                "require_thresholds": True,
                "base_estimator": {
                    "sklearn.pipeline.Pipeline": {
                        "steps": [
                            "sklearn.preprocessing.MinMaxScaler",
                            {
                                "gordo_amd.machine.model.models.KerasLSTMAutoEncoder": {
                                    "kind": "lstm_hourglass",
                                    "lookback_window": LOOKBACK,
                                    "epochs": EPOCHS,
                                    "batch_size": BATCH_LSTM,
                                }
                            },
                        ]
                    }
                },
            }
        }
    else:
        model = {
            "gordo_amd.machine.model.anomaly.diff.DiffBasedAnomalyDetector": {
                "require_thresholds": True,
                "base_estimator": {
                    "sklearn.pipeline.Pipeline": {
                        "steps": [
                            "sklearn.preprocessing.MinMaxScaler",
                            {
                                "gordo_amd.machine.model.models.KerasAutoEncoder": {
                                    "kind": "feedforward_hourglass",
                                    "epochs": EPOCHS,
                                    "batch_size": BATCH_DENSE,
                                }
                            },
                        ]
                    }
                },
            }
        }
    return {"name": f"bench-{kind}-{i}", "model": model, "dataset": dataset}


def _numeric_leaves(obj, out: list):
    """Numeric leaves of a nested dict/list in sorted-key order."""
    if isinstance(obj, dict):
        for k in sorted(obj):
            _numeric_leaves(obj[k], out)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _numeric_leaves(v, out)
    elif isinstance(obj, (int, float, np.integer, np.floating)) and not (
        isinstance(obj, bool)
    ):
        out.append(float(obj))


def _fit_dump_budget(arrays: dict, max_bytes: int) -> dict:
    """Keep [n_machines, n] arrays within max_bytes in all: the small
    ones stay whole; the weight matrices share what is left, sampled by
    column with a fixed seed (the same columns in every run)."""
    big = [k for k in arrays if k.startswith("weights_")]
    left = max_bytes - sum(
        a.nbytes for k, a in arrays.items() if k not in big
    )
    if sum(arrays[k].nbytes for k in big) <= left:
        return arrays
    out = dict(arrays)
    rng = np.random.default_rng(0)
    for k in big:
        a = arrays[k]
        keep = max(left, 0) // len(big) // (a.shape[0] * a.itemsize)
        if keep < a.shape[1]:
            cols = np.sort(rng.choice(a.shape[1], keep, replace=False))
            out[k] = np.ascontiguousarray(a[:, cols])
    return out


def dump_outputs(dump_dir: str, results, model_dir: str, suffix: str = ""):
    """Write what a caller of the timed build received in its last step:
    per machine (config order) the saved model's trained weights, loss
    history and DiffBased thresholds, and the CV scores of the returned
    Machine metadata. One [n_machines, ...] array per quantity and model
    kind; arrays that would exceed the budget keep a fixed seeded sample
    of their columns."""
    from gordo_amd import serializer
    from gordo_amd.parallel.packed_builder import _classify

    rows: dict = {}
    for name, machine in results:
        kind = "lstm" if "-lstm-" in name else "dense"
        model = serializer.load(os.path.join(model_dir, name))
        detector, _, inner = _classify(model)
        weights = inner._weights
        cv = machine.metadata.build_metadata.model.cross_validation
        scores: list = []
        _numeric_leaves(cv.scores, scores)
        per_machine = {
            f"weights_{kind}": np.concatenate(
                [np.asarray(weights[k], np.float32).ravel()
                 for k in sorted(weights)]
            ),
            f"loss_history_{kind}": np.asarray(
                inner.history["loss"], np.float64
            ),
            f"feature_thresholds_{kind}": np.asarray(
                detector.feature_thresholds_, np.float64
            ).ravel(),
            f"aggregate_threshold_{kind}": np.asarray(
                [detector.aggregate_threshold_], np.float64
            ),
            f"cv_scores_{kind}": np.asarray(scores, np.float64),
        }
        for k, v in per_machine.items():
            rows.setdefault(k, []).append(v)

    arrays = _fit_dump_budget(
        {k: np.stack(v) for k, v in rows.items()}, DUMP_BYTES_MAX
    )
    os.makedirs(dump_dir, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(dump_dir, f"{k}{suffix}.npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--machines-per-gpu", type=int, default=MACHINES_PER_GPU)
    ap.add_argument("--verbose", action="store_true",
                    help="log per-phase build timings to stderr")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as "
                         "DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also report what is not needed for the headline "
                         "figure (today: the per-phase build ledger)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    import logging

    logging.basicConfig(
        level=logging.INFO if args.verbose else logging.WARNING,
        stream=sys.stderr,
    )

    from gordo_amd.machine import Machine
    from gordo_amd.parallel import init_distributed, shard_machines
    from gordo_amd.parallel.packed_builder import PackedFleetBuilder

    rank, world = init_distributed()
    n_gpus = max(args.gpus, world)
    on_gpu = torch.cuda.is_available()
    device = f"cuda:{os.environ.get('LOCAL_RANK', 0)}" if on_gpu else "cpu"

    total_machines = args.machines_per_gpu * n_gpus
    n_lstm = total_machines // 2
    cfgs = [
        make_machine_cfg(i, "lstm" if i < n_lstm else "dense")
        for i in range(total_machines)
    ]
    machines_all = [Machine.from_config(c, project_name="bench") for c in cfgs]
    shards = shard_machines(machines_all, world)
    my_machines = [machines_all[i] for i in shards[rank]] if world > 1 else (
        machines_all
    )

    out_dir = tempfile.mkdtemp(prefix=f"gordo-bench-r{rank}-")

    phase_acc: dict = {}

    # at 8 ranks per node, per-rank thread pools must share the host:
    # 16 fetch threads x 8 ranks oversubscribes the CPUs during the
    # data phase (ROADMAP r1 flagged this for the SCALE run)
    workers = max(4, 16 // max(world, 1))

    def one_step(timed: bool = False):
        builder = PackedFleetBuilder(
            my_machines, output_dir=out_dir, model_register_dir=None,
            device=device, save_models=True, data_workers=workers,
        )
        results = builder.build_all()
        failed = [n for n, r in results if isinstance(r, BaseException)]
        if failed:
            errs = {n: repr(r) for n, r in results if isinstance(r, BaseException)}
            raise RuntimeError(f"bench build failures: {errs}")
        if timed:
            for k, v in builder.phase_times.items():
                phase_acc[k] = phase_acc.get(k, 0.0) + v
        return results

    import torch.distributed as dist

    def barrier_sync():
        if world > 1:
            dist.barrier()
        if on_gpu:
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        one_step()

    barrier_sync()
    t0 = time.time()
    for _ in range(args.steps):
        last_results = one_step(timed=True)
    barrier_sync()
    elapsed = time.time() - t0

    # MAX over ranks
    if world > 1:
        t = torch.tensor(
            [elapsed],
            device=device if on_gpu else "cpu",
            dtype=torch.float64,
        )
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    if args.dump_outputs:
        dump_outputs(
            args.dump_outputs, last_results, out_dir,
            suffix=f"_rank{rank}" if world > 1 else "",
        )

    shutil.rmtree(out_dir, ignore_errors=True)

    if rank == 0 and (args.verbose or args.full):
        # per-step phase budget (seconds averaged over the timed steps;
        # 'total' is the sequential wall — overlapped keys are informational)
        budget = {k: round(v / args.steps, 3) for k, v in
                  sorted(phase_acc.items())}
        print(json.dumps({"phase_budget_s_per_step": budget}),
              file=sys.stderr)

    if rank == 0:
        ms_per_step = elapsed * 1000.0 / args.steps
        built = total_machines * args.steps
        machines_per_hour = built * 3600.0 / elapsed
        print(json.dumps({
            "metric": "machines built/hour (1000-model config)",
            "value": machines_per_hour,
            "unit": "machines/hour",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if on_gpu else "fp32",
            "data": "synthetic sine-wave tags, random-init weights",
            "config": {
                "model": "mixed KerasLSTMAutoEncoder(lookback=144) + "
                         "feedforward_hourglass AE fleet, "
                         "DiffBasedAnomalyDetector, cv=TimeSeriesSplit(3)",
                "global_batch": total_machines,
                "machines_per_gpu": args.machines_per_gpu,
                "seq_len": LOOKBACK,
                "rows": ROWS_DAYS * 144,
                "n_tags": N_TAGS,
                "epochs": EPOCHS,
                "parallelism": f"fleet-dp{n_gpus} (RCCL shard, grouped "
                               f"MFMA packs per rank)",
            },
        }))


if __name__ == "__main__":
    main()
