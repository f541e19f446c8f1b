#!/usr/bin/env python3
"""What the per-tensor statistics cost, bf16, one process.
  python tools/tstats_bench.py [--cases r0,c5] [--loop r0] [--reps 5] [--launches 20] [--out profiles/tstats/tstats_bench.jsonl]
(a) pair: the two launches of afr_tensor_stats on the gradient buffer of R0 (12 tensors, 123 M elements) and of C5 (55 tensors) take
    turns with afr_grad_sumsq over the same buffer: R rounds of N event-timed calls each, median and min-max.  Both move 4 bytes per
    element; the bar, at R0's size only: the pair's median is at most 1.25 x afr_grad_sumsq's median ("within_bar").
(b) minus: the same with a second buffer (8 bytes per element), no bar.
(c) loop: model._run_epoch in miniature (a few training batches by rows and a validation pass over the batch as the data set) with
    the AFR_TENSOR_REPORT gatherer on and off, taking turns; the ratio, no bar.
One JSON line per case and leg."""
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
from ai_font_renderer_amd import _lib, synth  # noqa: E402
from ai_font_renderer_amd import model as M  # noqa: E402
from ai_font_renderer_amd.config import WORKLOADS  # noqa: E402
from ai_font_renderer_amd.engine import Engine, _ptr, _stream  # noqa: E402
from ai_font_renderer_amd.parallel import DataParallelStepper  # noqa: E402

BAR = 1.25


def _stats(v, nd=3):
    return dict(median=round(statistics.median(v), nd), min=round(min(v), nd), max=round(max(v), nd))


def _take_turns(forms, reps, launches):
    """us per call of every form: `reps` rounds, in each round every form gets `launches` event-timed calls in a row."""
    for f in forms.values():
        for _ in range(launches):
            f()
    us = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(launches):
                f()
            b.record()
            torch.cuda.synchronize()
            us[k].append(a.elapsed_time(b) * 1e3 / launches)
    return us


def kernel_legs(name, reps, launches):
    cfg = WORKLOADS[name]["cfg"]
    eng = Engine(cfg, dtype="bf16", max_batch=1)                # the buffers are what is measured: the smallest plan will do
    eng.load_params(synth.make_params(cfg))
    g = torch.Generator(device="cuda").manual_seed(3)
    eng.flat_grads.copy_(torch.randn(eng.n_flat, device="cuda", generator=g) * 1e-3)
    minus = torch.randn(eng.n_flat, device="cuda", generator=g) * 1e-3
    elems = sum(k for _, _, _, k in eng.layout)
    chunk = int(eng.lib.afr_tensor_stats_chunk())
    chunks = sum(max(1, -(-k // chunk)) for _, _, _, k in eng.layout)
    lib, plan, s = eng.lib, eng._plan, _stream(eng.device)     # the C calls themselves, outputs allocated once
    rec = torch.empty(len(eng.layout), 8, dtype=torch.int32, device="cuda")
    ss = torch.empty(1, device="cuda")
    us = _take_turns({"pair": lambda: _lib.check(lib.afr_tensor_stats(plan, _lib.STAT_KINDS["grads"], None, _ptr(rec), s)),
                      "minus": lambda: _lib.check(lib.afr_tensor_stats(plan, _lib.STAT_KINDS["grads"], _ptr(minus), _ptr(rec), s)),
                      "grad_sumsq": lambda: _lib.check(lib.afr_grad_sumsq(plan, 0, eng.n_flat, _ptr(ss), s))}, reps, launches)
    # both saw the same data: the records' sums of squares add up to the global one
    tot, ref = float(eng.tensor_stats("grads").cpu().sumsq.astype("float64").sum()), float(eng.grad_sumsq())
    assert abs(tot - ref) <= 1e-4 * ref, (tot, ref)
    pm, mm, sm = (statistics.median(us[k]) for k in ("pair", "minus", "grad_sumsq"))
    base = dict(workload=name, dtype="bf16", tensors=len(eng.layout), elements=elems, chunks=chunks, rounds=reps, calls_per_round=launches,
                grad_sumsq_us=_stats(us["grad_sumsq"]))
    a = dict(leg="pair", **base, pair_us=_stats(us["pair"]), pair_over_grad_sumsq=round(pm / sm, 4), pair_GBps=round(4 * elems / pm / 1e3, 1),
             grad_sumsq_GBps=round(4 * elems / sm / 1e3, 1))
    if name == "r0":
        a.update(bar=BAR, within_bar=bool(pm <= BAR * sm))
    b = dict(leg="minus", **base, minus_us=_stats(us["minus"]), minus_over_grad_sumsq=round(mm / sm, 4), minus_GBps=round(8 * elems / mm / 1e3, 1))
    return [a, b]


class _Order:
    def __init__(self, train_rows, val_rows):
        self.train_size, self.val_size, self._train, self._val = train_rows.numel(), val_rows.numel(), train_rows, val_rows

    def train_epoch(self):
        return self._train

    def val_epoch(self):
        return self._val


class _Model:
    """What _run_epoch and the report's gatherer ask of a model, around any engine."""

    def __init__(self, eng):
        self.engine, self._steps, self._tensor_snapshot = eng, 0, None

    def train(self):
        pass

    eval = train

    def _next_step(self):
        self._steps += 1
        return self._steps


def loop_leg(name, reps, train_batches, val_batches):
    cfg, B = WORKLOADS[name]["cfg"], WORKLOADS[name]["batch"]
    eng = Engine(cfg, dtype="bf16", max_batch=B)
    eng.load_params(synth.make_params(cfg))
    x, font, tgt = make_inputs(name, cfg, B, 0)
    t8 = M.helpers.targets_as_uint8(tgt)
    x, font, t8 = x.cuda(), None if font is None else font.cuda(), t8.cuda().reshape(B, -1).contiguous()
    eng.bind_dataset(x, t8, font=font)                          # the batch as the data set, walked in a seeded order
    g = torch.Generator().manual_seed(7)
    order = _Order(torch.cat([torch.randperm(B, generator=g) for _ in range(train_batches)]),
                   torch.cat([torch.randperm(B, generator=g) for _ in range(val_batches)]))
    model, stepper = _Model(eng), DataParallelStepper(eng, None, 1)

    def run(on):
        tr = M._TensorReport(model) if on else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        M._run_epoch(model, stepper, order, x, t8, B, M.LEARNING_RATE, 0, 1, by_rows=True, reports=[tr] if on else ())
        if tr is not None:
            tr.lines()                                          # (its device-to-host reads happened in the probe)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for on in (False, True):
        run(on)
    ms = {False: [], True: []}
    for _ in range(reps):
        for on in (False, True):
            ms[on].append(run(on))
    assert eng.error_flags() == 0
    return dict(leg="loop", workload=name, dtype="bf16", batch=B, train_batches=train_batches, val_batches=val_batches, rounds=reps,
                epoch_ms_off=_stats(ms[False]), epoch_ms_on=_stats(ms[True]),
                on_over_off=round(statistics.median(ms[True]) / statistics.median(ms[False]), 4),
                on_minus_off_ms=round(statistics.median(ms[True]) - statistics.median(ms[False]), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="r0,c5")
    ap.add_argument("--loop", default="r0", help="workloads of leg (c), comma separated; empty: none")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--train-batches", type=int, default=8)
    ap.add_argument("--val-batches", type=int, default=2)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    torch.cuda.set_device(0)

    def emit(line):
        print(json.dumps(line), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")

    for name in [n for n in a.cases.split(",") if n]:
        for line in kernel_legs(name, a.reps, a.launches):
            emit(line)
        torch.cuda.empty_cache()
    for name in [n for n in a.loop.split(",") if n]:
        emit(loop_leg(name, a.reps, a.train_batches, a.val_batches))
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
