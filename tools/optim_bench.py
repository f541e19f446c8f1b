#!/usr/bin/env python3
"""What the optimizer kind costs a training step: an AdamW plan and a Lion plan of one workload side by side, one process.
  python tools/optim_bench.py [--cases c3:bf16,r0:bf16,c2:bf16] [--steps K] [--warmup W] [--reps R] [--out profiles/lion/optim_bench.jsonl]
    adamw    the default step (torch.optim.AdamW's update fused into the gradient producers; p, m, v read and written)
    lion     Engine(optimizer="lion"): the same launches with the Lion instantiations (p and m only; no exp_avg_sq is allocated)
Each plan gets its own engine and bench.py's inputs; after the warm-up the two take turns, R rounds of K device-synchronised
training steps each (afr_train_step), so that clock and thermal drift fall on both alike.  ms_per_step is the median round.
Prints one JSON line per (workload, dtype) -- ms/step of the two (median and every round), the AdamW plan's own min-max spread,
and for each plan the event-timed launch that carries the optimizer (afr_profile_*: name, ms, algorithmic bytes, TB/s) -- and
appends it to --out.  The launch that carries the optimizer (CARRIER: a tag prefix per workload, the match with the most algorithmic
bytes): R0's weight-gradient GEMM with the fused update, a grouped 256x256 launch of C3 (cooperative split-K tail), the grouped
reduce of the small nets."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import make_inputs  # noqa: E402
from ai_font_renderer_amd import synth  # noqa: E402
from ai_font_renderer_amd.config import WORKLOADS  # noqa: E402
from ai_font_renderer_amd.engine import Engine  # noqa: E402

STEPS = {"c3": (50, 5), "r0": (10, 2), "c2": (200, 20), "c1": (200, 20)}     # steps per round, warm-up
KINDS = ("adamw", "lion")
# the launch of a step that carries the optimizer, by workload: a prefix of its profile tag
CARRIER = {"r0": "gemm_bf16<1,1,2>", "c3": "gemm_bf16_group256", "c2": "reduce_group", "c1": "reduce_group"}


def setup(name, dtype, kind):
    cfg, B = WORKLOADS[name]["cfg"], WORKLOADS[name]["batch"]
    eng = Engine(cfg, dtype=dtype, max_batch=B, optimizer=kind)
    eng.load_params(synth.make_params(cfg))
    x, font, tgt = make_inputs(name, cfg, B, 0)
    x, tgt = x.cuda(), tgt.cuda()
    font = font.cuda() if font is not None else None
    return eng, B, (lambda: eng.train_step(x, tgt, font=font))


def carrier_launch(eng, step, name, reps=5):
    """The launch that carries the optimizer in `reps` profiled steps: its tag, launches per step, mean ms, algorithmic bytes, TB/s."""
    eng.profile(1)
    for _ in range(reps):
        step()
    torch.cuda.synchronize()
    rows = [r for r in eng.profile_table() if r["kernel"].startswith(CARRIER[name])]
    eng.profile(0)
    if not rows:
        return None
    r = max(rows, key=lambda r: r["algo_bytes"])
    return dict(kernel=r["kernel"], launches_per_step=r["launches"] / reps, ms=round(r["avg_ms"], 4), algo_bytes=r["algo_bytes"],
                tb_per_s=round(r["algo_bytes"] / (r["avg_ms"] * 1e-3) / 1e12, 3) if r["avg_ms"] > 0 else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c3:bf16,r0:bf16,c2:bf16")
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for case in a.cases.split(","):
        name, dtype = case.split(":")
        K = a.steps or STEPS[name][0]
        W = a.warmup if a.warmup is not None else STEPS[name][1]
        runs = {}
        for kind in KINDS:
            eng, B, step = setup(name, dtype, kind)
            for _ in range(W):
                step()
            runs[kind] = dict(eng=eng, B=B, step=step, carrier=carrier_launch(eng, step, name), ms=[])
        for _ in range(a.reps):
            for kind in KINDS:
                r = runs[kind]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(K):
                    r["step"]()
                torch.cuda.synchronize()
                r["ms"].append((time.perf_counter() - t0) * 1e3 / K)
        med = {k: statistics.median(runs[k]["ms"]) for k in KINDS}
        for k in KINDS:
            runs[k]["eng"].read_loss()
            assert runs[k]["eng"].error_flags() == 0, k
        assert runs["lion"]["eng"].exp_avg_sq is None
        spread = max(runs["adamw"]["ms"]) - min(runs["adamw"]["ms"])
        line = {"workload": name, "dtype": dtype, "batch": runs["adamw"]["B"], "steps_per_round": K, "rounds": a.reps,
                "ms_per_step": {k: round(med[k], 4) for k in KINDS}, "ms_rounds": {k: [round(v, 4) for v in runs[k]["ms"]] for k in KINDS},
                "lion_over_adamw": round(med["lion"] / med["adamw"], 4), "adamw_spread_ms": round(spread, 4),
                "lion_not_slower_than_adamw_plus_its_spread": bool(med["lion"] <= med["adamw"] + spread),
                "param_bytes": runs["adamw"]["eng"].n_flat * 4, "optimizer_launch": {k: runs[k]["carrier"] for k in KINDS}}
        print(json.dumps(line), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del runs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
