#!/usr/bin/env python3
"""The training LOOP, timed: by row index against gather-then-step, one process.
  python tools/epoch_bench.py [--cases r0,c3] [--dtypes bf16,f32] [--sheets 30720] [--distinct 2048] [--reps 5]
r0: the sheet model (BASELINE R0) on an HBM-resident data set of --sheets synthetic sheets (synth.dataset_strings /
    encode_strings / synth_sheet_targets, uint8; --distinct different sheets generated on the host, repeated on the device to
    the full row count -- every row is its own memory), batch 1024, dropout as configured.  One epoch = the training loop over
    80 % + the validation loop over 20 % (model._run_epoch, what train_attention_model runs).  Two forms take turns for R
    rounds of one epoch each: "rows" (Engine.bind_dataset, step_rows / forward_rows + loss_grad_rows) and "gather"
    (index_select + the dense calls).  Reports sheets/s per epoch for both (median round, with the minimum and maximum), and
    the ratio to the step-level rate measured in the same process on one contiguous resident batch (eng.train_step, what
    bench.py --workload r0 times).
c3: the C3 glyph net, 8192 glyphs, bf16: the 190-row FiraCode + Montserrat table bound as the data set with
    rows = font * 95 + (x - 32), against the dense 8 MB of expanded targets; ms/step both ways, taking turns.
One JSON line per case."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import make_inputs  # noqa: E402
from ai_font_renderer_amd import synth  # noqa: E402
from ai_font_renderer_amd.config import WORKLOADS  # noqa: E402
from ai_font_renderer_amd.engine import Engine  # noqa: E402


def _stats(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def r0_loop(dtype, sheets, distinct, reps, batch=1024):
    from ai_font_renderer_amd import model as M
    from ai_font_renderer_amd.parallel import DataParallelStepper
    m = M.AttentionFontRenderer(max_length=M.MAX_CHARS_PER_SHEET, dtype=dtype, max_batch=batch, init=False)
    cfg, eng = m.config, m.engine
    eng.load_params(synth.make_params(cfg))
    distinct = min(distinct, sheets)
    x0 = torch.from_numpy(synth.encode_strings(synth.dataset_strings(distinct), cfg.max_length)).cuda()
    t0 = torch.from_numpy(synth.synth_sheet_targets(distinct, cfg.sheet_h, cfg.sheet_w, tensor_id=970)).cuda()
    k = (sheets + distinct - 1) // distinct
    inputs, targets = x0.repeat(k, 1)[:sheets].contiguous(), t0.repeat(k, 1, 1)[:sheets].contiguous()
    del x0, t0
    eng.bind_dataset(inputs, targets)
    order = M._EpochOrder(sheets)
    stepper = DataParallelStepper(eng, None, 1)

    def epoch(by_rows):
        M._run_epoch(m, stepper, order, inputs, targets, batch, M.LEARNING_RATE, 0, 1, by_rows=by_rows)

    # step level: one contiguous resident batch, as bench.py hands it to the step
    xb, tb = inputs[:batch].contiguous(), targets[:batch].contiguous()
    for _ in range(3):
        eng.train_step(xb, tb, step=m._next_step())
    K = 20
    step_s = []
    for _ in range(reps):
        step_s.append(_timed(lambda: [eng.train_step(xb, tb, step=m._next_step()) for _ in range(K)]) / K)
    step_rate = batch / statistics.median(step_s)
    for form in (True, False):             # warm-up: one epoch of each form
        epoch(form)
    secs = {True: [], False: []}
    for _ in range(reps):
        for form in (True, False):
            secs[form].append(_timed(lambda: epoch(form)))
    eng.read_loss()
    assert eng.error_flags() == 0
    rate = {f: [sheets / s for s in v] for f, v in secs.items()}
    rows_med, gather_med = statistics.median(rate[True]), statistics.median(rate[False])
    return dict(case="r0_loop", dtype=dtype, sheets=sheets, distinct_sheets=distinct, batch=batch, rounds=reps,
                train_batches=M._num_batches(order.train_size, batch), val_batches=M._num_batches(order.val_size, batch),
                sheets_per_s_rows=_stats(rate[True]), sheets_per_s_gather=_stats(rate[False]),
                epoch_ms_rows=_stats([s * 1e3 for s in secs[True]]), epoch_ms_gather=_stats([s * 1e3 for s in secs[False]]),
                rows_over_gather=round(rows_med / gather_med, 4),
                step_level=dict(ms_per_step=_stats([s * 1e3 for s in step_s]), sheets_per_s=round(step_rate, 1)),
                epoch_over_step_rows=round(rows_med / step_rate, 4), epoch_over_step_gather=round(gather_med / step_rate, 4))


def c3_step(reps, steps=50, B=8192):
    cfg = WORKLOADS["c3"]["cfg"]
    eng = Engine(cfg, dtype="bf16", max_batch=B)
    eng.load_params(synth.make_params(cfg))
    x, font, tgt = make_inputs("c3", cfg, B, 0)
    x, font, tgt = x.cuda(), font.cuda(), tgt.cuda()
    codes = np.tile(np.arange(32, 127, dtype=np.int64), cfg.n_fonts)
    fonts = np.repeat(np.arange(cfg.n_fonts, dtype=np.int64), 95)
    table = synth.glyph_bitmap_targets(cfg.out_h, codes, fonts)
    if table is None:
        raise SystemExit("tests/golden/glyph_bitmaps.npz is missing: no glyph table to bind")
    eng.bind_dataset(torch.from_numpy(codes), torch.from_numpy(table), font=torch.from_numpy(fonts))
    rows = (font * 95 + (x - 32)).contiguous()
    assert torch.equal(torch.from_numpy(table).cuda()[rows], tgt)
    forms = {"rows": lambda: eng.train_step_rows(rows), "dense": lambda: eng.train_step(x, tgt, font=font)}
    for f in forms.values():
        for _ in range(5):
            f()
    ms = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            ms[k].append(_timed(lambda: [f() for _ in range(steps)]) * 1e3 / steps)
    eng.read_loss()
    assert eng.error_flags() == 0
    return dict(case="c3_step", dtype="bf16", batch=B, table_rows=int(table.shape[0]), steps_per_round=steps, rounds=reps,
                ms_per_step_rows=_stats(ms["rows"]), ms_per_step_dense=_stats(ms["dense"]),
                rows_over_dense=round(statistics.median(ms["rows"]) / statistics.median(ms["dense"]), 4),
                target_bytes_per_step=dict(rows=int(table.size), dense=int(tgt.numel())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="r0,c3")
    ap.add_argument("--dtypes", default="bf16,f32")
    ap.add_argument("--sheets", type=int, default=30720)
    ap.add_argument("--distinct", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    cases = a.cases.split(",")
    if "r0" in cases:
        for dt in a.dtypes.split(","):
            print(json.dumps(r0_loop(dt, a.sheets, a.distinct, a.reps)), flush=True)
            torch.cuda.empty_cache()
    if "c3" in cases:
        print(json.dumps(c3_step(a.reps)), flush=True)


if __name__ == "__main__":
    main()
