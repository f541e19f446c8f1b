#!/usr/bin/env python3
"""What composing the sheet data set on the device costs, one process, one GPU.
  python tools/compose_bench.py [--n 150000] [--font FILE] [--reps 7] [--host-sheets 200] [--no-epoch] [--out profiles/compose/compose_bench.jsonl]
(a) device: the text launch (afr_op_dataset_text) and the compose launch (afr_op_compose_sheets) for n sheets of 80 x 240, and beside
    them a device fill (Tensor.fill_) of the same n * 19200 bytes, taking turns for --reps rounds after two warm rounds; every launch
    is timed with events on its stream.  The fill is the yardstick: the composer writes each byte once and reads cache-resident data.
    Two more compose launches take the same turns to show where its time goes: "blank" (every text empty: the per-sheet barriers and
    the stores alone) and "short" (every text cut to its first 10 characters: one short line to lay out and to paint).
(b) host: datagen.render_sheet (PIL, one core) over --host-sheets texts of the same source, per sheet and scaled to n.
(c) fresh data: the rewrite of the training rows that AFR_FRESH_DATA does before an epoch (model._fresh_rows: text by rows, gather,
    compose by rows; 80 % of n), event-timed, against one R0 epoch of the same n rows by row index (tools/epoch_bench.py r0_loop,
    bf16, batch 1024, same process and build).
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
from ai_font_renderer_amd import datagen, devdata, synth  # noqa: E402


def _stats(v, nd=3):
    return dict(median=round(statistics.median(v), nd), min=round(min(v), nd), max=round(max(v), nd))


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def device_part(atlas, n, reps):
    codes = torch.empty((n, 100), dtype=torch.int64, device="cuda")
    lens = torch.empty(n, dtype=torch.int32, device="cuda")
    sheets = torch.empty((n, 80, 240), dtype=torch.uint8, device="cuda")
    other = torch.empty_like(sheets)
    lib, a, g = devdata._lib.lib(), atlas._struct(), devdata.sheet_geometry(atlas=atlas)
    s = devdata._stream(sheets.device)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    blank = torch.zeros_like(codes)

    def compose(c):
        return lambda: devdata._lib.check(lib.afr_op_compose_sheets(C.byref(a), C.byref(g), devdata._ptr(c), 100, None, n, devdata._ptr(sheets),
                                                                    devdata._ptr(err), s))
    devdata._lib.check(lib.afr_op_dataset_text(42, None, None, n, 10, 100, devdata._ptr(codes), 100, devdata._ptr(lens), s))
    short = codes.clone()
    short[:, 10:] = 0
    forms = {
        "compose_blank": compose(blank), "compose_short": compose(short),
        "text": lambda: devdata._lib.check(lib.afr_op_dataset_text(42, None, None, n, 10, 100, devdata._ptr(codes), 100, devdata._ptr(lens), s)),
        "compose": compose(codes),
        "fill": lambda: other.fill_(0x5A),
    }
    ms = {k: [] for k in forms}
    for r in range(reps + 2):
        for k, f in forms.items():
            t = _event_ms(f)
            if r >= 2:
                ms[k].append(t)
    assert int(err) == 0
    nbytes = sheets.numel()
    med = {k: statistics.median(v) for k, v in ms.items()}
    return dict(part="device", n=n, sheet_bytes=nbytes, rounds=reps, text_ms=_stats(ms["text"]), compose_ms=_stats(ms["compose"]),
                fill_ms=_stats(ms["fill"]), compose_blank_ms=_stats(ms["compose_blank"]), compose_short_ms=_stats(ms["compose_short"]),
                text_plus_compose_ms=round(med["text"] + med["compose"], 3),
                compose_over_fill=round(med["compose"] / med["fill"], 3), compose_gb_per_s=round(nbytes / med["compose"] / 1e6, 1),
                fill_gb_per_s=round(nbytes / med["fill"] / 1e6, 1), sheets_per_s=round(n / (med["text"] + med["compose"]) * 1e3, 0))


def host_part(font_path, n, k):
    from PIL import ImageFont
    font = ImageFont.truetype(font_path, datagen.FONT_SIZE) if font_path else ImageFont.load_default(datagen.FONT_SIZE)
    texts = [synth.lcg_text(42 + i) for i in range(k)]
    datagen.render_sheet(texts[0], font)
    per = []
    for t in texts:
        t0 = time.perf_counter()
        datagen.render_sheet(t, font)
        per.append((time.perf_counter() - t0) * 1e3)
    return dict(part="host", sheets=k, render_sheet_ms=_stats(per), scaled_to_n_s=round(statistics.median(per) * n / 1e3, 1), n=n)


def fresh_part(atlas, n, reps, with_epoch):
    from ai_font_renderer_amd import model as M
    codes, lens = devdata.generate_codes(n, device="cuda")
    sheets = devdata.compose_sheets(atlas, codes)
    rows = M._EpochOrder(n).train_idx.cuda()
    refresh = M._fresh_rows(atlas, n)
    ms = []
    for r in range(reps + 2):
        t = _event_ms(lambda: refresh(r + 1, rows, codes, sheets))
        if r >= 2:
            ms.append(t)
    out = dict(part="fresh", n=n, train_rows=int(rows.numel()), rounds=reps, rewrite_ms=_stats(ms))
    del codes, sheets
    torch.cuda.empty_cache()
    if with_epoch:
        from epoch_bench import r0_loop
        ep = r0_loop("bf16", n, 2048, max(3, reps // 2))
        out.update(epoch_ms_rows=ep["epoch_ms_rows"], sheets_per_s_rows=ep["sheets_per_s_rows"],
                   rewrite_share_of_epoch=round(statistics.median(ms) / ep["epoch_ms_rows"]["median"], 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=150000)
    ap.add_argument("--font", default=None, help="TTF file (default: Pillow's built-in font)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-sheets", type=int, default=200)
    ap.add_argument("--no-epoch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    atlas = devdata.GlyphAtlas.from_font(a.font).to("cuda")
    head = dict(part="setup", font=a.font or "Pillow built-in", cells=list(atlas.cells.shape), origin=[atlas.origin_x, atlas.origin_y],
                device=torch.cuda.get_device_name(0))
    lines = [head, device_part(atlas, a.n, a.reps), host_part(a.font, a.n, a.host_sheets), fresh_part(atlas, a.n, a.reps, not a.no_epoch)]
    for rec in lines:
        print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(rec) + "\n" for rec in lines)


if __name__ == "__main__":
    main()
