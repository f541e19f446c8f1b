#!/usr/bin/env python3
"""What the weighted text source and the steering cost, one process, one GPU.
  python tools/text_bench.py [--rows 120000] [--n 150000] [--reps 7] [--no-epoch] [--out profiles/alphabet/text_bench.jsonl]
(a) launch: afr_op_dataset_text_w for --rows rows of 100 codes -- with equal weights on A-Z (the bytes of afr_op_dataset_text), with
    equal weights on all 94 codes, and with a steered A-Z table -- beside afr_op_dataset_text, and the one-workgroup afr_op_text_weights
    launch, taking turns for --reps rounds after two warm ones; every launch is timed with events on its stream.
(b) rewrite: what AFR_FRESH_DATA does before an epoch (model._fresh_rows: texts by rows, gather, compose by rows; the 80 % training rows
    of --n), event-timed, three forms taking turns: the plain source (the parent's rewrite), AFR_ALPHABET=upper (table + weighted
    texts) and AFR_STEER=0.5 (table from a by-code table on the device + weighted texts).
(c) epoch: one R0 epoch (bf16, batch 1024, by row index) of --n device-composed rows under AFR_FRESH_DATA -- the rewrite, the training
    pass and the validation pass -- without steering and with AFR_STEER=0.5 (every validation batch evaluated to bitmaps and measured
    by afr_op_sheet_char_errors, the table fed to the next rewrite), taking turns, wall clock around a synchronised epoch.
One JSON line per part; medians with the rounds' minimum and maximum."""
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
from ai_font_renderer_amd import devdata, synth  # noqa: E402


def _stats(v, nd=4):
    return dict(median=round(statistics.median(v), nd), min=round(min(v), nd), max=round(max(v), nd))


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _turns(forms, reps, timer=_event_ms):
    ms = {k: [] for k in forms}
    for r in range(reps + 2):
        for k, f in forms.items():
            t = timer(f)
            if r >= 2:
                ms[k].append(t)
    return ms


def _steer_table(device):
    """a by-code table with every letter's error of its own, W some fifteen times the rest (the table of tests/text_cases.py)"""
    by = torch.zeros((128, 5), dtype=torch.int64)
    for c in range(65, 91):
        pixels = 2000 + 397 * ((c * c) % 26)
        by[c, 1], by[c, 2] = pixels, pixels * (6000 if c == ord("W") else 40 + (c * 7919) % 391)
    return by.to(device)


def launch_part(n, reps):
    codes = torch.empty((n, 100), dtype=torch.int64, device="cuda")
    lens = torch.empty(n, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    lib, s, p = devdata._lib.lib(), devdata._stream(codes.device), devdata._ptr
    table = _steer_table("cuda")
    cums = {"upper": devdata.text_weights("upper", device="cuda")[0], "ascii": devdata.text_weights("ascii", device="cuda")[0],
            "steered": devdata.text_weights("upper", table, 2048, 2048)[0]}
    cum, w = torch.empty(94, dtype=torch.int32, device="cuda"), torch.empty(94, dtype=torch.int32, device="cuda")
    words = (C.c_uint32 * 3)(*synth.members_words(synth.alphabet_members("upper")))

    def text_w(c):
        return lambda: devdata._lib.check(lib.afr_op_dataset_text_w(42, None, None, n, 10, 100, p(c), p(codes), 100, p(lens), p(err), s))
    forms = {"text": lambda: devdata._lib.check(lib.afr_op_dataset_text(42, None, None, n, 10, 100, p(codes), 100, p(lens), s)),
             **{"text_w_" + k: text_w(c) for k, c in cums.items()},
             "weights": lambda: devdata._lib.check(lib.afr_op_text_weights(p(table), 127, words, 2048, 2048, p(cum), p(w), s))}
    ms = _turns(forms, reps)
    assert int(err) == 0
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = dict(part="launch", rows=n, rounds=reps, **{k + "_ms": _stats(v) for k, v in ms.items()})
    for k in cums:
        out[f"text_w_{k}_over_text"] = round(med["text_w_" + k] / med["text"], 3)
    return out


def rewrite_part(atlas, n, reps):
    from ai_font_renderer_amd import model as M
    codes, _ = devdata.generate_codes(n, device="cuda")
    sheets = devdata.compose_sheets(atlas, codes)
    rows = M._EpochOrder(n).train_idx.cuda()
    table = _steer_table("cuda")
    plain, upper, steer = M._fresh_rows(atlas, n), M._fresh_rows(atlas, n, "upper"), M._fresh_rows(atlas, n, None, 0.5)
    epoch = iter(range(1, 1 << 20))
    forms = {"plain": lambda: plain(next(epoch), rows, codes, sheets), "alphabet_upper": lambda: upper(next(epoch), rows, codes, sheets),
             "steer": lambda: steer(next(epoch), rows, codes, sheets, by_code=table)}
    ms = _turns(forms, reps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    return dict(part="rewrite", n=n, train_rows=int(rows.numel()), rounds=reps, **{k + "_ms": _stats(v, 3) for k, v in ms.items()},
                alphabet_over_plain=round(med["alphabet_upper"] / med["plain"], 4), steer_over_plain=round(med["steer"] / med["plain"], 4))


def epoch_part(atlas, n, reps):
    from ai_font_renderer_amd import model as M
    from ai_font_renderer_amd.parallel import DataParallelStepper
    ds = devdata.reference_dataset(n, atlas)
    x, t = ds.tensors
    m = M.AttentionFontRenderer(max_length=M.MAX_CHARS_PER_SHEET, dtype="bf16", max_batch=1024)
    eng = m.engine
    eng.bind_dataset(x, t)
    order, stepper = M._EpochOrder(n), DataParallelStepper(eng, None, 1)
    plain, steer = M._fresh_rows(atlas, n), M._fresh_rows(atlas, n, None, 0.5)
    state = dict(epoch=0, table=None)

    def epoch(steered):
        def run():
            state["epoch"] += 1
            errors = M._CharErrorPass(atlas, x) if steered else None
            if steered:
                steer(state["epoch"], order.train_idx, x, t, by_code=state["table"])
            else:
                plain(state["epoch"], order.train_idx, x, t)
            M._run_epoch(m, stepper, order, x, t, 1024, M.LEARNING_RATE, 0, 1, by_rows=True, reports=[errors] if steered else ())
            if steered:
                state["table"] = errors.by_code
        return run

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    ms = _turns({"off": epoch(False), "steer": epoch(True)}, reps, wall_ms)
    med = {k: statistics.median(v) for k, v in ms.items()}
    heavy = M._steer_line(0.5, steer.w)
    return dict(part="epoch", workload="r0", dtype="bf16", n=n, train_rows=order.train_size, val_rows=order.val_size, batch=1024, rounds=reps,
                epoch_off_ms=_stats(ms["off"], 2), epoch_steer_ms=_stats(ms["steer"], 2), steer_over_off=round(med["steer"] / med["off"], 4),
                added_ms=round(med["steer"] - med["off"], 2), last_rewrite=heavy)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=120000)
    ap.add_argument("--n", type=int, default=150000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-epoch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    atlas = devdata.GlyphAtlas.from_font(None).to("cuda")
    lines = [dict(part="setup", font="Pillow built-in", cells=list(atlas.cells.shape), device=torch.cuda.get_device_name(0)),
             launch_part(a.rows, a.reps), rewrite_part(atlas, a.n, a.reps)]
    torch.cuda.empty_cache()
    if not a.no_epoch:
        lines.append(epoch_part(atlas, a.n, max(3, a.reps // 2)))
    for rec in lines:
        print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(rec) + "\n" for rec in lines)


if __name__ == "__main__":
    main()
