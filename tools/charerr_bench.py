#!/usr/bin/env python3
"""What attributing the rendering error to characters costs, one process, one GPU.
  python tools/charerr_bench.py [--reps 7] [--val 30000] [--out profiles/charerr/charerr_bench.jsonl]
(a) launch: afr_op_sheet_char_errors (both outputs) at 1024 and at 30 000 sheets of 80 x 240 beside afr_op_compose_sheets on the same
    codes -- the nearest existing kernel: the same layout and paint, a load in the place of the store and the LDS adds on top -- the
    forms taking turns for --reps rounds after two warm rounds, every launch timed with events on its stream.  The prediction is the
    composed sheet of the next text, so owned pixels carry error as a bad rendering's do.  Both kernels also run compose_bench.py's two
    variants: "blank" (every text empty: the per-sheet head and the loads / stores alone) and "short" (every text cut to 10 characters).
(b) validation: one validation pass of R0 (bf16, batch 1024, --val rows of a bound data set composed on the device, by row index: forward,
    loss) as model._run_epoch runs it, with AFR_CHAR_REPORT's work in it (evaluate_last with bitmaps + the launch per batch) and without,
    taking turns in the same way.
One JSON line per part; medians with the rounds' minimum and maximum."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ai_font_renderer_amd import devdata  # noqa: E402


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


def _turns(forms, reps):
    ms = {k: [] for k in forms}
    for r in range(reps + 2):
        for k, f in forms.items():
            t = _event_ms(f)
            if r >= 2:
                ms[k].append(t)
    return ms


def launch_part(atlas, n, reps):
    codes, _ = devdata.generate_codes(n, device="cuda")
    sheets = torch.empty((n, 80, 240), dtype=torch.uint8, device="cuda")
    lib, a, g = devdata._lib.lib(), atlas._struct(), devdata.sheet_geometry(atlas=atlas)
    s = devdata._stream(sheets.device)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    per_pos = torch.empty((n, 101, 4), dtype=torch.int32, device="cuda")
    by_code = torch.zeros((atlas.n_codes + 1, 5), dtype=torch.int64, device="cuda")
    pred = devdata.compose_sheets(atlas, codes).roll(-1, 0).contiguous()
    blank, short = torch.zeros_like(codes), codes.clone()
    short[:, 10:] = 0

    def compose(c):
        return lambda: devdata._lib.check(lib.afr_op_compose_sheets(C.byref(a), C.byref(g), devdata._ptr(c), 100, None, n, devdata._ptr(sheets),
                                                                    devdata._ptr(err), s))

    def charerr(c):
        return lambda: devdata._lib.check(lib.afr_op_sheet_char_errors(C.byref(a), C.byref(g), devdata._ptr(c), 100, None, n, devdata._ptr(pred),
                                                                       devdata._ptr(per_pos), devdata._ptr(by_code), devdata._ptr(err), s))
    forms = {"compose_blank": compose(blank), "charerr_blank": charerr(blank), "compose_short": compose(short), "charerr_short": charerr(short),
             "compose": compose(codes), "charerr": charerr(codes)}
    ms = _turns(forms, reps)
    assert int(err) == 0
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = dict(part="launch", n=n, rounds=reps, **{k + "_ms": _stats(v) for k, v in ms.items()})
    for k in ("", "_blank", "_short"):
        out["charerr_over_compose" + k] = round(med["charerr" + k] / med["compose" + k], 3)
    out["sheets_per_s"] = round(n / med["charerr"] * 1e3, 0)
    return out


def validation_part(atlas, n_val, reps):
    from ai_font_renderer_amd import model as M
    ds = devdata.reference_dataset(n_val, atlas)
    x, t = ds.tensors
    m = M.AttentionFontRenderer(max_length=100, max_batch=1024, dtype="bf16")
    eng = m.engine
    eng.bind_dataset(x, t)
    m.eval()
    rows_all, pixels, bs = torch.arange(n_val, device="cuda"), t[0].numel(), 1024

    def val_pass(with_report):
        def run():
            errors = M._CharErrorPass(atlas, x) if with_report else None
            for b in range((n_val + bs - 1) // bs):
                rows = rows_all[b * bs:(b + 1) * bs]
                calls = M._batch_calls(eng, None, None, None, rows)
                calls.forward(training=False, want_output=False)
                if errors is not None:
                    errors.add(calls.evaluate_last(want_u8=True), rows)
                calls.loss_grad(mean_elems=rows.numel() * pixels)
            eng.read_loss()
        return run
    ms = _turns({"off": val_pass(False), "on": val_pass(True)}, reps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    return dict(part="validation", workload="r0", dtype="bf16", val_rows=n_val, batch=bs, rounds=reps, pass_off_ms=_stats(ms["off"]),
                pass_on_ms=_stats(ms["on"]), on_over_off=round(med["on"] / med["off"], 4), added_ms=round(med["on"] - med["off"], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--val", type=int, default=30000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    atlas = devdata.GlyphAtlas.from_font(None).to("cuda")
    lines = [dict(part="setup", font="Pillow built-in", cells=list(atlas.cells.shape), origin=[atlas.origin_x, atlas.origin_y],
                  device=torch.cuda.get_device_name(0))]
    for n in (1024, 30000):
        lines.append(launch_part(atlas, n, a.reps))
    lines.append(validation_part(atlas, a.val, a.reps))
    for rec in lines:
        print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(rec) + "\n" for rec in lines)


if __name__ == "__main__":
    main()
