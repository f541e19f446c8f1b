#!/usr/bin/env python3
"""The two parity modes side by side: f32 (exact-f32 MFMA) against bf16x3 (split-bf16 MFMA products), one process.
  python tools/parity_bench.py [--workloads c3,r0] [--modes f32,bf16x3] [--steps K] [--warmup W] [--reps R]
Each (workload, mode) gets its own engine and bench.py's inputs; after the warm-up the modes take turns, R rounds of K
device-synchronised training steps each (forward + MSE + backward + AdamW, afr_train_step), so that clock and thermal drift
fall on both alike.  ms_per_step is the median round.  Prints one JSON line per (workload, mode) with the dominant kernel of
a profiled warm-up step (afr_profile_*) and its algorithmic rate as a fraction of the bf16x3 ceiling (2.5 PF / 3)."""
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
from ai_font_renderer_amd.config import WORKLOADS, SheetConfig  # noqa: E402
from ai_font_renderer_amd.engine import Engine  # noqa: E402

BF16X3_CEIL_TF = 2500.0 / 3
F32_PEAK_TF = 157.3
DEFAULTS = {"c3": (50, 5, 8192), "r0": (10, 2, 1024), "c5": (5, 1, 32)}     # steps per round, warm-up, batch


def setup(name, dtype):
    cfg = WORKLOADS[name]["cfg"]
    B = DEFAULTS[name][2]
    eng = Engine(cfg, dtype=dtype, max_batch=B)
    eng.load_params(synth.make_params(cfg))
    x, font, tgt = make_inputs(name, cfg, B, 0)
    x, tgt = x.cuda(), tgt.cuda()
    font = font.cuda() if font is not None else None
    return eng, B, (lambda: eng.train_step(x, tgt, font=font))


def dominant(eng, step):
    eng.profile(1)
    step()
    torch.cuda.synchronize()
    rows = eng.profile_table()
    eng.profile(0)
    top = rows[0]
    tf = top["algo_flops"] / (top["avg_ms"] * 1e-3) / 1e12 if top["avg_ms"] > 0 else 0.0
    step_ms = sum(r["total_ms"] for r in rows)
    return dict(kernel=top["kernel"], avg_ms=round(top["avg_ms"], 4), launches=top["launches"], tflops=round(tf, 1),
                share_of_profiled_step=round(top["total_ms"] / step_ms, 3) if step_ms else None), rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c3,r0")
    ap.add_argument("--modes", default="f32,bf16x3")
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--table", action="store_true", help="also print each profiled step's per-kernel table to stderr")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    modes = a.modes.split(",")
    for name in a.workloads.split(","):
        K = a.steps or DEFAULTS[name][0]
        W = a.warmup if a.warmup is not None else DEFAULTS[name][1]
        runs = {}
        for m in modes:
            eng, B, step = setup(name, m)
            for _ in range(W):
                step()
            dom, rows = dominant(eng, step)
            if a.table:
                for r in rows:
                    print(f"{name} {m}\t{r['kernel']}\t{r['launches']}\t{r['total_ms']:.3f}", file=sys.stderr)
            runs[m] = dict(eng=eng, B=B, step=step, dom=dom, ms=[])
        for _ in range(a.reps):
            for m in modes:
                r = runs[m]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(K):
                    r["step"]()
                torch.cuda.synchronize()
                r["ms"].append((time.perf_counter() - t0) * 1e3 / K)
        for m in modes:
            r = runs[m]
            r["eng"].read_loss()
            assert r["eng"].error_flags() == 0
            ms = statistics.median(r["ms"])
            unit = "sheets_per_s" if isinstance(WORKLOADS[name]["cfg"], SheetConfig) else "glyphs_per_s"
            dom = dict(r["dom"])
            dom["fraction_of_bf16x3_ceiling"] = round(dom["tflops"] / BF16X3_CEIL_TF, 3)
            dom["fraction_of_f32_peak"] = round(dom["tflops"] / F32_PEAK_TF, 3)
            print(json.dumps({"workload": name, "mode": m, "batch": r["B"], "steps_per_round": K, "rounds": a.reps,
                              "ms_per_step": round(ms, 4), "ms_rounds": [round(v, 4) for v in r["ms"]],
                              unit: round(r["B"] / (ms * 1e-3), 1), "dominant": dom}), flush=True)
        del runs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
