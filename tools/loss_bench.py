#!/usr/bin/env python3
"""The two loss kinds side by side: an MSE plan (clamp head) against a BCE plan (sigmoid head, afr_config.loss), one process.
  python tools/loss_bench.py [--cases c3:bf16,c3:f32,r0:bf16,c2:bf16] [--steps K] [--warmup W] [--reps R] [--table]
Each (workload, dtype, loss) gets its own engine and bench.py's inputs; after the warm-up the two plans of a case take turns,
R rounds of K device-synchronised training steps each (afr_train_step: forward + loss + backward + AdamW), so that clock and
thermal drift fall on both alike.  ms_per_step is the median round.  Prints one JSON line per (workload, dtype, loss) with the
launch that carries the loss in a profiled step (afr_profile_*: the last forward product with its fused loss epilogue, or the
fused small-net step) and its time, and `bce_over_mse` on the BCE line."""
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

STEPS = {"c3": (50, 5), "r0": (10, 2), "c2": (200, 20), "c1": (200, 20)}     # steps per round, warm-up


def setup(name, dtype, loss):
    cfg, B = WORKLOADS[name]["cfg"], WORKLOADS[name]["batch"]
    eng = Engine(cfg, dtype=dtype, max_batch=B, loss=loss)
    eng.load_params(synth.make_params(cfg))
    x, font, tgt = make_inputs(name, cfg, B, 0)
    x, tgt = x.cuda(), tgt.cuda()
    font = font.cuda() if font is not None else None
    return eng, B, (lambda: eng.train_step(x, tgt, font=font))


def loss_launch(eng, step, cfg, B):
    """The profiled step's launch that computes the loss: the fused small-net step, else the forward product of the output
    layer, whose tag carries its shape [B x pixels x K] (a grouped launch of gradient products has a `+` in its tag)."""
    eng.profile(1)
    step()
    torch.cuda.synchronize()
    rows = eng.profile_table()
    eng.profile(0)
    total = sum(r["total_ms"] for r in rows)
    pick = [r for r in rows if r["kernel"].startswith("glyph1_step")] or \
           [r for r in rows if f"[{B}x{cfg.pixels}x" in r["kernel"] and "+" not in r["kernel"]]
    top = pick[0] if pick else rows[0]
    return dict(kernel=top["kernel"], avg_ms=round(top["avg_ms"], 4), launches=top["launches"], profiled_step_ms=round(total, 4)), rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c3:bf16,c3:f32,r0:bf16,c2:bf16")
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--table", action="store_true", help="also print each profiled step's per-kernel table to stderr")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    kinds = ("mse", "bce")
    for case in a.cases.split(","):
        name, dtype = case.split(":")
        cfg = WORKLOADS[name]["cfg"]
        K = a.steps or STEPS[name][0]
        W = a.warmup if a.warmup is not None else STEPS[name][1]
        runs = {}
        for k in kinds:
            eng, B, step = setup(name, dtype, k)
            for _ in range(W):
                step()
            dom, rows = loss_launch(eng, step, cfg, B)
            if a.table:
                for r in rows:
                    print(f"{name} {dtype} {k}\t{r['kernel']}\t{r['launches']}\t{r['total_ms']:.4f}", file=sys.stderr)
            runs[k] = dict(eng=eng, B=B, step=step, dom=dom, ms=[])
        for _ in range(a.reps):
            for k in kinds:
                r = runs[k]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(K):
                    r["step"]()
                torch.cuda.synchronize()
                r["ms"].append((time.perf_counter() - t0) * 1e3 / K)
        med = {k: statistics.median(runs[k]["ms"]) for k in kinds}
        for k in kinds:
            r = runs[k]
            r["eng"].read_loss()
            assert r["eng"].error_flags() == 0
            unit = "sheets_per_s" if isinstance(cfg, SheetConfig) else "glyphs_per_s"
            line = {"workload": name, "dtype": dtype, "loss": k, "batch": r["B"], "steps_per_round": K, "rounds": a.reps,
                    "ms_per_step": round(med[k], 4), "ms_rounds": [round(v, 4) for v in r["ms"]],
                    unit: round(r["B"] / (med[k] * 1e-3), 1), "loss_launch": r["dom"]}
            if k == "bce":
                line["bce_over_mse"] = round(med["bce"] / med["mse"], 4)
            print(json.dumps(line), flush=True)
        del runs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
