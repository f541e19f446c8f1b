#!/usr/bin/env python3
"""What clipping by global gradient norm costs a training step: three plans of one workload side by side, one process.
  python tools/clip_bench.py [--cases c3:bf16,r0:bf16,c2:bf16] [--steps K] [--warmup W] [--reps R] [--out profiles/clip/clip_bench.jsonl]
    off      the default step (optimizer fused into the gradient producers)
    clip     Engine(max_grad_norm=1e30): the clip never bites (coef = 1), the step pays for the path -- every gradient
             materialised, the norm kernel's pass over them, the stand-alone AdamW kernel reading the norm
    unfused  AFR_CFG_UNFUSED_OPTIMIZER without clipping: the same path without the norm pass
Each plan gets its own engine and bench.py's inputs; after the warm-up the three take turns, R rounds of K device-synchronised
training steps each (afr_train_step), so that clock and thermal drift fall on all alike.  ms_per_step is the median round.
Prints one JSON line per (workload, dtype) -- ms/step of the three, their ratios, and the norm kernel's and the AdamW kernel's
time in a profiled clipped step (afr_profile_*) -- and appends it to --out."""
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
MODES = {"off": dict(), "clip": dict(max_grad_norm=1e30), "unfused": dict(flags=1)}


def setup(name, dtype, mode):
    cfg, B = WORKLOADS[name]["cfg"], WORKLOADS[name]["batch"]
    eng = Engine(cfg, dtype=dtype, max_batch=B, **MODES[mode])
    eng.load_params(synth.make_params(cfg))
    x, font, tgt = make_inputs(name, cfg, B, 0)
    x, tgt = x.cuda(), tgt.cuda()
    font = font.cuda() if font is not None else None
    return eng, B, (lambda: eng.train_step(x, tgt, font=font))


def profiled(eng, step):
    """Per-kernel times of one profiled step: (grad_sumsq ms, adamw ms, whole step ms as the sum of its launches)."""
    eng.profile(1)
    step()
    torch.cuda.synchronize()
    rows = eng.profile_table()
    eng.profile(0)
    pick = lambda pre: round(sum(r["total_ms"] for r in rows if r["kernel"].startswith(pre)), 4)
    return dict(grad_sumsq_ms=pick("grad_sumsq"), adamw_ms=pick("adamw"), profiled_step_ms=round(sum(r["total_ms"] for r in rows), 4))


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
        for mode in MODES:
            eng, B, step = setup(name, dtype, mode)
            for _ in range(W):
                step()
            runs[mode] = dict(eng=eng, B=B, step=step, prof=profiled(eng, step), ms=[])
        for _ in range(a.reps):
            for mode in MODES:
                r = runs[mode]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(K):
                    r["step"]()
                torch.cuda.synchronize()
                r["ms"].append((time.perf_counter() - t0) * 1e3 / K)
        med = {m: statistics.median(runs[m]["ms"]) for m in MODES}
        for m in MODES:
            runs[m]["eng"].read_loss()
            assert runs[m]["eng"].error_flags() == 0, m
        assert runs["clip"]["eng"].clip_coef() == 1.0
        line = {"workload": name, "dtype": dtype, "batch": runs["off"]["B"], "steps_per_round": K, "rounds": a.reps,
                "ms_per_step": {m: round(med[m], 4) for m in MODES}, "ms_rounds": {m: [round(v, 4) for v in runs[m]["ms"]] for m in MODES},
                "clip_over_off": round(med["clip"] / med["off"], 4), "clip_over_unfused": round(med["clip"] / med["unfused"], 4),
                "unfused_over_off": round(med["unfused"] / med["off"], 4), "grad_norm": runs["clip"]["eng"].grad_norm(),
                "flat_grad_bytes": runs["off"]["eng"].n_flat * 4, "clipped_step_kernels": runs["clip"]["prof"],
                "unfused_step_kernels": runs["unfused"]["prof"]}
        print(json.dumps(line), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del runs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
