#!/usr/bin/env python3
"""What optimizer groups cost: two plans of one workload side by side, and the range-aware flat kernel beside the plain one.
  python tools/groups_bench.py [--cases c3:bf16,r0:bf16,c2:bf16] [--steps K] [--warmup W] [--reps R] [--out profiles/groups/groups_bench.jsonl]
    off       the default step (no groups: the parent's launches)
    nodecay   Engine(wd_mult={name: 0 for name in config.no_decay_names(cfg)}): the default rule
  Each plan gets its own engine and bench.py's inputs; after the warm-up the two take turns, R rounds of K device-synchronised training
  steps each (afr_train_step), so that clock and thermal drift fall on both alike.  ms_per_step is the median round.  One JSON line per
  (workload, dtype): ms/step of the two (median and every round), their ratio, the groups-off plan's own min-max spread.
  python tools/groups_bench.py --flat r0,c5 [--reps R] [--inner N] [--out ...]
  The flat update alone at a model's size, on buffers of its own, one range per parameter tensor (every tensor its own multipliers:
  nothing merges; R0 12 ranges, C5 55): afr_op_adamw (the plain kernel), afr_op_opt_groups, afr_op_adamw again, in turns, R rounds of N
  event-timed launches each with a bf16 shadow (28 + 2 bytes per element).  One JSON line per model: us per launch of the three
  (median round and every round), TB/s, and the condition the grouped kernel is held to -- its median is not above the plain
  kernel's by more than the plain kernel's own A/A spread (the larger of |A - A'| of the medians and A's min-max over the rounds)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import make_inputs  # noqa: E402
from ai_font_renderer_amd import _lib, synth  # noqa: E402
from ai_font_renderer_amd.config import C5, WORKLOADS, flat_layout, no_decay_names  # noqa: E402
from ai_font_renderer_amd.engine import Engine  # noqa: E402

STEPS = {"c3": (48, 5), "r0": (8, 2), "c2": (200, 20), "c1": (200, 20)}     # steps per round, warm-up
PLANS = ("off", "nodecay")


def setup(name, dtype, plan):
    cfg, B = WORKLOADS[name]["cfg"], WORKLOADS[name]["batch"]
    kw = dict(wd_mult={k: 0.0 for k in no_decay_names(cfg)}) if plan == "nodecay" else {}
    eng = Engine(cfg, dtype=dtype, max_batch=B, **kw)
    eng.load_params(synth.make_params(cfg))
    x, font, tgt = make_inputs(name, cfg, B, 0)
    x, tgt = x.cuda(), tgt.cuda()
    font = font.cuda() if font is not None else None
    return eng, B, (lambda: eng.train_step(x, tgt, font=font))


def emit(line, out):
    print(json.dumps(line), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(json.dumps(line) + "\n")


def steps(a):
    for case in a.cases.split(","):
        name, dtype = case.split(":")
        K = a.steps or STEPS[name][0]
        W = a.warmup if a.warmup is not None else STEPS[name][1]
        runs = {}
        for plan in PLANS:
            eng, B, step = setup(name, dtype, plan)
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
        for k in PLANS:
            runs[k]["eng"].read_loss()
            assert runs[k]["eng"].error_flags() == 0, k
        med = {k: statistics.median(runs[k]["ms"]) for k in PLANS}
        emit({"workload": name, "dtype": dtype, "batch": runs["off"]["B"], "steps_per_round": K, "rounds": a.reps,
              "ranges": len(runs["nodecay"]["eng"].param_group_ranges()), "ms_per_step": {k: round(med[k], 4) for k in PLANS},
              "ms_rounds": {k: [round(v, 4) for v in runs[k]["ms"]] for k in PLANS}, "nodecay_over_off": round(med["nodecay"] / med["off"], 4),
              "off_spread_ms": round(max(runs["off"]["ms"]) - min(runs["off"]["ms"]), 4), "param_elems": runs["off"]["eng"].n_flat}, a.out)
        del runs
        torch.cuda.empty_cache()


def flat(a):
    lib = _lib.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name in a.flat.split(","):
        cfg = C5 if name == "c5" else WORKLOADS[name]["cfg"]
        table, n = flat_layout(cfg)
        ends = [table[i + 1][2] if i + 1 < len(table) else n for i in range(len(table))]
        ranges = (_lib.AfrOptRange * len(ends))(*[_lib.AfrOptRange(e, 1.0 + 0.01 * i, 0.5 + 0.01 * i) for i, e in enumerate(ends)])
        gen = torch.Generator(device="cuda").manual_seed(1)
        p, g, m = (torch.randn(n, device="cuda", generator=gen) * s for s in (0.5, 0.01, 0.01))
        v = torch.rand(n, device="cuda", generator=gen) * 1e-4 + 1e-8
        sh = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
        hyper = (1e-6, 0.9, 0.99, 1e-8, 0.5)
        launch = {
            "plain": lambda: _lib.check(lib.afr_op_adamw(ptr(p), ptr(g), ptr(m), ptr(v), ptr(sh), n, *hyper, 2, 1.0, stream())),
            "grouped": lambda: _lib.check(lib.afr_op_opt_groups(0, ptr(p), ptr(g), ptr(m), ptr(v), ptr(sh), n, 0, ranges, len(ends), *hyper, 2, 1.0,
                                                                None, 0.0, stream())),
        }
        order = (("plain", "plain"), ("grouped", "grouped"), ("plain_again", "plain"))
        for _ in range(3):
            for f in launch.values():
                f()
        us = {k: [] for k, _ in order}
        for _ in range(a.reps):
            for key, which in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.inner):
                    launch[which]()
                e1.record()
                torch.cuda.synchronize()
                us[key].append(e0.elapsed_time(e1) * 1e3 / a.inner)
        med = {k: statistics.median(v) for k, v in us.items()}
        spread = max(abs(med["plain"] - med["plain_again"]), max(us["plain"]) - min(us["plain"]))
        by = 30.0 * n
        emit({"flat": name, "elements": n, "ranges": len(ends), "rounds": a.reps, "launches_per_round": a.inner, "bytes_per_launch": by,
              "us": {k: round(v, 2) for k, v in med.items()}, "us_rounds": {k: [round(x, 2) for x in v] for k, v in us.items()},
              "tb_per_s": {k: round(by / (v * 1e-6) / 1e12, 3) for k, v in med.items()}, "plain_aa_spread_us": round(spread, 2),
              "grouped_minus_plain_us": round(med["grouped"] - min(med["plain"], med["plain_again"]), 2),
              "grouped_within_plain_aa_spread": bool(med["grouped"] - max(med["plain"], med["plain_again"]) <= spread)}, a.out)
        del p, g, m, v, sh
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c3:bf16,r0:bf16,c2:bf16")
    ap.add_argument("--flat", default=None, help="comma list of r0 | c5 | c3 ...: time the flat kernels at that model's size instead")
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=8)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    flat(a) if a.flat else steps(a)


if __name__ == "__main__":
    main()
