#!/usr/bin/env python3
"""What the weight EMA costs a training step: three plans of one workload side by side, one process.
  python tools/ema_bench.py [--cases c3:bf16,r0:bf16,c2:bf16] [--steps K] [--warmup W] [--reps R] [--out profiles/ema/ema_bench.jsonl]
    off      the default step (no EMA: the parent's launches)
    every1   Engine(ema_decay=0.999): one more streaming launch over the flat buffer behind every optimizer step (12 B / parameter)
    every8   Engine(ema_decay=0.999, ema_every=8): the same launch behind every 8th step
Each plan gets its own engine and bench.py's inputs; after the warm-up the three take turns, R rounds of K device-synchronised
training steps each (afr_train_step; K a multiple of 8), so that clock and thermal drift fall on all alike.  ms_per_step is the
median round.  Prints one JSON line per (workload, dtype) -- ms/step of the three (median and every round), the EMA-off plan's own
min-max spread, the event-timed `ema` launch of the every1 plan (afr_profile_*: ms, algorithmic bytes = 12 x elements, TB/s) and, timed
the same way in the same process, the stand-alone `adamw` kernel (afr_adamw_step of a plan without clipping: 28 (+2 with the bf16
shadow) B / parameter) on the same buffers -- and appends it to --out.  Both are pure streaming kernels; the condition the EMA kernel
is held to is that its TB/s is not below the adamw kernel's less that kernel's min-max spread over the rounds."""
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

STEPS = {"c3": (48, 5), "r0": (8, 2), "c2": (200, 20), "c1": (200, 20)}     # steps per round (multiples of 8), warm-up
PLANS = {"off": {}, "every1": dict(ema_decay=0.999), "every8": dict(ema_decay=0.999, ema_every=8)}


def setup(name, dtype, kw):
    cfg, B = WORKLOADS[name]["cfg"], WORKLOADS[name]["batch"]
    eng = Engine(cfg, dtype=dtype, max_batch=B, **kw)
    eng.load_params(synth.make_params(cfg))
    x, font, tgt = make_inputs(name, cfg, B, 0)
    x, tgt = x.cuda(), tgt.cuda()
    font = font.cuda() if font is not None else None
    return eng, B, (lambda: eng.train_step(x, tgt, font=font))


def timed_launch(eng, run, tag, rounds, per_round):
    """The launch tagged `tag` in `rounds` profiled rounds of `per_round` calls of run(): per round its mean ms; then the median round,
    the min-max spread, algorithmic bytes and TB/s (median; spread in TB/s between the slowest and the fastest round)."""
    ms, by = [], 0.0
    for _ in range(rounds):
        eng.profile(1)
        for _ in range(per_round):
            run()
        torch.cuda.synchronize()
        rows = [r for r in eng.profile_table() if r["kernel"] == tag]
        eng.profile(0)
        if not rows:
            return None
        ms.append(rows[0]["avg_ms"])
        by = rows[0]["algo_bytes"]
    med = statistics.median(ms)
    tbs = lambda v: by / (v * 1e-3) / 1e12 if v > 0 else None
    return dict(kernel=tag, ms=round(med, 4), ms_rounds=[round(v, 4) for v in ms], algo_bytes=by, tb_per_s=round(tbs(med), 3),
                tb_per_s_spread=round(tbs(min(ms)) - tbs(max(ms)), 3))


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
        for plan, kw in PLANS.items():
            eng, B, step = setup(name, dtype, kw)
            for _ in range(W):
                step()
            runs[plan] = dict(eng=eng, B=B, step=step, ms=[])
        for _ in range(a.reps):
            for plan in PLANS:
                r = runs[plan]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(K):
                    r["step"]()
                torch.cuda.synchronize()
                r["ms"].append((time.perf_counter() - t0) * 1e3 / K)
        med = {k: statistics.median(runs[k]["ms"]) for k in PLANS}
        spread = max(runs["off"]["ms"]) - min(runs["off"]["ms"])
        # the two streaming launches, event-timed in turn: the EMA pass inside training steps of the every1 plan, the stand-alone
        # optimizer kernel over the same buffers (gradients as the last step left them; lr = 0 keeps the weights where they are)
        ema = timed_launch(runs["every1"]["eng"], runs["every1"]["step"], "ema", a.reps, 4)
        eng = runs["every1"]["eng"]
        adamw = timed_launch(eng, lambda: eng._call(eng.lib.afr_adamw_step, eng._plan, 0.0, 0.9, 0.99, 1e-8, 0.0, 1, 1.0), "adamw", a.reps, 4)
        torch.cuda.synchronize()
        for k in PLANS:
            runs[k]["eng"].read_loss()
            assert runs[k]["eng"].error_flags() == 0, k
        ok = None
        if ema and adamw:
            ok = bool(ema["tb_per_s"] >= adamw["tb_per_s"] - adamw["tb_per_s_spread"])
        line = {"workload": name, "dtype": dtype, "batch": runs["off"]["B"], "steps_per_round": K, "rounds": a.reps,
                "ms_per_step": {k: round(med[k], 4) for k in PLANS}, "ms_rounds": {k: [round(v, 4) for v in runs[k]["ms"]] for k in PLANS},
                "every1_over_off": round(med["every1"] / med["off"], 4), "every8_over_off": round(med["every8"] / med["off"], 4),
                "off_spread_ms": round(spread, 4), "param_elems": runs["off"]["eng"].n_flat, "ema_launch": ema, "adamw_launch": adamw,
                "ema_tb_per_s_not_below_adamw_less_its_spread": ok}
        print(json.dumps(line), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del runs, eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
