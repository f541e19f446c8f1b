#!/usr/bin/env python3
"""What the pair tables and the Markov text source cost, one process, one GPU.
  python tools/pair_bench.py [--rows 120000] [--n 150000] [--reps 7] [--no-epoch] [--out profiles/pairs/pair_bench.jsonl]
(a) launch: afr_op_dataset_text_m for --rows rows of 100 codes -- with equal weights on the pairs of A-Z (the bytes of
    afr_op_dataset_text) and with a table whose diagonal is 64 times the rest -- beside afr_op_dataset_text_w with equal weights;
    afr_op_pair_errors beside afr_op_sheet_char_errors (which writes the per_pos it reads) at 1024 and 30 000 sheets of device-composed
    texts measured against their neighbours' sheets; and the one-workgroup afr_op_pair_weights launch.  The forms take turns for --reps
    rounds after two warm ones; every launch is timed with events on its stream.
(b) rewrite: what AFR_FRESH_DATA does before an epoch (model._fresh_rows; the 80 % training rows of --n), event-timed, three forms
    taking turns: the plain source, AFR_STEER=0.5 (the parent's steered rewrite: letter table from a by-code table + weighted texts)
    and AFR_STEER_PAIRS=0.5 (pair table from a by-pair table on the device + Markov texts).
(c) epoch: one R0 epoch (bf16, batch 1024, by row index) of --n device-composed rows under AFR_FRESH_DATA without steering and with
    AFR_STEER_PAIRS=0.5 (every validation batch evaluated to bitmaps, measured by afr_op_sheet_char_errors with per_pos and scattered
    by afr_op_pair_errors, the table fed to the next rewrite), taking turns, wall clock around a synchronised epoch.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ai_font_renderer_amd import devdata, synth  # noqa: E402
from text_bench import _stats, _steer_table, _turns  # noqa: E402


def _run_table(factor, device):
    """cum2 of A-Z with every live pair at 4096 and the same letter again at 4096 * factor (tests/pair_ref.py run_table)"""
    members = synth.alphabet_members("upper")
    w2 = [[0] * 94 for _ in range(95)]
    for p in [0] + [1 + i for i in range(94) if members[i]]:
        for c in range(94):
            if members[c]:
                w2[p][c] = 4096 * (factor if p == c + 1 else 1)
    return torch.tensor(synth.pair_table(w2), dtype=torch.int64).to(torch.int32).to(device)


def _pair_table(atlas, n=4096):
    """a by-pair table on the device: n device-composed sheets measured against their neighbours'"""
    codes, _ = devdata.generate_codes(n, device="cuda")
    sheets = devdata.compose_sheets(atlas, codes)
    return devdata.pair_errors(codes, devdata.char_errors(atlas, codes, sheets.roll(-1, 0).contiguous()).per_pos)


def launch_part(atlas, n, reps):
    codes = torch.empty((n, 100), dtype=torch.int64, device="cuda")
    lens = torch.empty(n, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    lib, s, p = devdata._lib.lib(), devdata._stream(codes.device), devdata._ptr
    check = devdata._lib.check
    cum = devdata.text_weights("upper", device="cuda")[0]
    tables = {"flat": devdata.pair_weights("upper", device="cuda")[0], "runs64": _run_table(64, "cuda")}
    by_pair = _pair_table(atlas)
    cum2, w2 = torch.empty((95, 94), dtype=torch.int32, device="cuda"), torch.empty((95, 94), dtype=torch.int32, device="cuda")
    words = (C.c_uint32 * 3)(*synth.members_words(synth.alphabet_members("upper")))

    def text_m(c2):
        return lambda: check(lib.afr_op_dataset_text_m(42, None, None, n, 10, 100, p(c2), p(codes), 100, p(lens), p(err), s))
    forms = {"text_w": lambda: check(lib.afr_op_dataset_text_w(42, None, None, n, 10, 100, p(cum), p(codes), 100, p(lens), p(err), s)),
             **{"text_m_" + k: text_m(c2) for k, c2 in tables.items()},
             "pair_weights": lambda: check(lib.afr_op_pair_weights(p(by_pair), words, 2048, 2048, 8, p(cum2), p(w2), s))}
    a, g = atlas._struct(), devdata.sheet_geometry(80, 240, 14.4, atlas)
    keep = []
    for sheets_n in (1024, 30000):
        x, _ = devdata.generate_codes(sheets_n, device="cuda")
        pred = devdata.compose_sheets(atlas, x).roll(-1, 0).contiguous()
        per_pos = torch.empty((sheets_n, 101, 4), dtype=torch.int32, device="cuda")
        by_code = torch.zeros((atlas.n_codes + 1, 5), dtype=torch.int64, device="cuda")
        table = torch.zeros((95, 94, 4), dtype=torch.int64, device="cuda")
        keep.append((x, pred, per_pos, by_code, table))
        forms[f"char_errors_{sheets_n}"] = (lambda x=x, pred=pred, per_pos=per_pos, by_code=by_code, m=sheets_n: check(
            lib.afr_op_sheet_char_errors(C.byref(a), C.byref(g), p(x), 100, None, m, p(pred), p(per_pos), p(by_code), p(err), s)))
        forms[f"pair_errors_{sheets_n}"] = (lambda x=x, per_pos=per_pos, table=table, m=sheets_n: check(
            lib.afr_op_pair_errors(p(x), 100, None, m, p(per_pos), p(table), s)))
    ms = _turns(forms, reps)
    assert int(err) == 0
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = dict(part="launch", rows=n, rounds=reps, **{k + "_ms": _stats(v) for k, v in ms.items()})
    for k in tables:
        out[f"text_m_{k}_over_text_w"] = round(med["text_m_" + k] / med["text_w"], 3)
    for sheets_n in (1024, 30000):
        out[f"pair_errors_{sheets_n}_over_char_errors"] = round(med[f"pair_errors_{sheets_n}"] / med[f"char_errors_{sheets_n}"], 4)
        out[f"pair_errors_{sheets_n}_contributions"] = int(keep[0 if sheets_n == 1024 else 1][4][:, :, 0].sum()) // (reps + 2)
    return out


def rewrite_part(atlas, n, reps):
    from ai_font_renderer_amd import model as M
    codes, _ = devdata.generate_codes(n, device="cuda")
    sheets = devdata.compose_sheets(atlas, codes)
    rows = M._EpochOrder(n).train_idx.cuda()
    by_code, by_pair = _steer_table("cuda"), _pair_table(atlas)
    plain, steer, pairs = M._fresh_rows(atlas, n), M._fresh_rows(atlas, n, None, 0.5), M._fresh_rows(atlas, n, None, 0.0, 0.5)
    epoch = iter(range(1, 1 << 20))
    forms = {"plain": lambda: plain(next(epoch), rows, codes, sheets), "steer": lambda: steer(next(epoch), rows, codes, sheets, by_code=by_code),
             "steer_pairs": lambda: pairs(next(epoch), rows, codes, sheets, by_pair=by_pair)}
    ms = _turns(forms, reps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    return dict(part="rewrite", n=n, train_rows=int(rows.numel()), rounds=reps, **{k + "_ms": _stats(v, 3) for k, v in ms.items()},
                steer_over_plain=round(med["steer"] / med["plain"], 4), steer_pairs_over_steer=round(med["steer_pairs"] / med["steer"], 4),
                last_rewrite=M._steer_pairs_line(0.5, pairs.w2))


def epoch_part(atlas, n, reps):
    from ai_font_renderer_amd import model as M
    from ai_font_renderer_amd.parallel import DataParallelStepper
    ds = devdata.reference_dataset(n, atlas)
    x, t = ds.tensors
    m = M.AttentionFontRenderer(max_length=M.MAX_CHARS_PER_SHEET, dtype="bf16", max_batch=1024)
    eng = m.engine
    eng.bind_dataset(x, t)
    order, stepper = M._EpochOrder(n), DataParallelStepper(eng, None, 1)
    plain, pairs = M._fresh_rows(atlas, n), M._fresh_rows(atlas, n, None, 0.0, 0.5)
    state = dict(epoch=0, table=None)

    def epoch(steered):
        def run():
            state["epoch"] += 1
            errors = M._CharErrorPass(atlas, x, by_code=False, pairs=True) if steered else None
            if steered:
                pairs(state["epoch"], order.train_idx, x, t, by_pair=state["table"])
            else:
                plain(state["epoch"], order.train_idx, x, t)
            M._run_epoch(m, stepper, order, x, t, 1024, M.LEARNING_RATE, 0, 1, by_rows=True, reports=[errors] if steered else ())
            if steered:
                state["table"] = errors.by_pair
        return run

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    ms = _turns({"off": epoch(False), "steer_pairs": epoch(True)}, reps, wall_ms)
    med = {k: statistics.median(v) for k, v in ms.items()}
    return dict(part="epoch", workload="r0", dtype="bf16", n=n, train_rows=order.train_size, val_rows=order.val_size, batch=1024, rounds=reps,
                epoch_off_ms=_stats(ms["off"], 2), epoch_steer_pairs_ms=_stats(ms["steer_pairs"], 2),
                steer_pairs_over_off=round(med["steer_pairs"] / med["off"], 4), added_ms=round(med["steer_pairs"] - med["off"], 2),
                last_rewrite=M._steer_pairs_line(0.5, pairs.w2))


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
             launch_part(atlas, a.rows, a.reps)]
    torch.cuda.empty_cache()
    lines.append(rewrite_part(atlas, a.n, a.reps))
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
