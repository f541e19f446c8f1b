#!/usr/bin/env python3
"""Every libafr call the Python driver makes for a fixed script of Engine calls, one line each: python tools/engine_calls.py > calls.txt
Two trees whose outputs are byte-identical call the library with the same entries, arguments and order.  eng.lib is replaced by a
recording proxy; pointers print as what they point into (0, plan, stream, an engine buffer + byte offset, a tensor of this script +
byte offset, tmp for anything the engine allocated for the call), byref arguments as out."""
import ctypes as C
import sys
import numpy as np
import torch
sys.path.insert(0, '.')
from ai_font_renderer_amd import synth
from ai_font_renderer_amd.config import GlyphConfig, PixelConfig, SheetConfig
from ai_font_renderer_amd.engine import Engine

OWNED = dict(flat_params='flat_params', flat_grads='flat_grads', exp_avg='exp_avg', exp_avg_sq='exp_avg_sq', flat_ema='flat_ema',
             loss_accum='loss_accum', workspace='workspace', _grad_acc='grad_acc', _clip_stats='clip_stats')
MINE = {}          # label -> tensor made by this script


def mk(label, t):
    MINE[label] = t.cuda().contiguous()
    return MINE[label]


class Recorder:
    def __init__(self, eng):
        self.eng, self.lib = eng, eng.lib

    def name(self, a):
        if type(a).__name__ == 'CArgObject':
            return 'out'
        if isinstance(a, C.Array):
            return f'{type(a)._type_.__name__}[{len(a)}]' + (str([round(v, 6) for v in a]) if type(a)._type_ is C.c_float else '')
        if isinstance(a, C.c_void_p):
            p = a.value or 0
            if p == 0:
                return '0'
            if p == self.eng._plan.value:
                return 'plan'
            if p == torch.cuda.current_stream(self.eng.device).cuda_stream:
                return 'stream'
            for label, t in [(lb, getattr(self.eng, at, None)) for at, lb in OWNED.items()] + list(MINE.items()):
                if t is not None and t.data_ptr() <= p < t.data_ptr() + max(1, t.numel() * t.element_size()):
                    return f'{label}+{p - t.data_ptr()}'
            return 'tmp'
        return repr(a)

    def __getattr__(self, entry):
        fn = getattr(self.lib, entry)

        def call(*args):
            print(f'{entry}({", ".join(self.name(a) for a in args)})')
            return fn(*args)
        return call


def say(what, fn):
    print(f'# {what}')
    try:
        fn()
    except Exception as e:                     # a refusal is part of the record
        print(f'raised {type(e).__name__}: {e}')


def data(cfg, n, tid):
    if isinstance(cfg, SheetConfig):
        x, font = 32 + synth.hash_u8(tid, (n, cfg.max_length)).astype(np.int64) % 95, None
        h, w = cfg.sheet_h, cfg.sheet_w
    else:
        x, font = synth.hash_u8(tid, (n,)).astype(np.int64) % cfg.vocab, synth.hash_u8(tid + 1, (n,)).astype(np.int64) % cfg.n_fonts
        h, w = cfg.out_h, cfg.out_w
    return torch.from_numpy(x), None if font is None else torch.from_numpy(font), torch.from_numpy(synth.hash_u8(tid + 2, (n, h, w)))


def script(cfg, dtype, B, micro):
    MINE.clear()
    eng = Engine(cfg, dtype=dtype, max_batch=8, micro_batch=micro)
    eng.load_params(synth.make_params(cfg))
    eng.lib = Recorder(eng)
    x, font, t = (None if v is None else mk(lb, v) for lb, v in zip(('x', 'font', 't'), data(cfg, B, 11)))
    tf = mk('tf', t.float() / 255.0)
    rows = mk('rows', torch.arange(B - 1, -1, -1))
    x8, font8, t8, rows8 = x[:8], None if font is None else font[:8], t[:8], rows[:8]       # what forward_loss takes under micro_batch
    say('bind_dataset', lambda: eng.bind_dataset(x, t, font))
    for wo in (True, False):
        say(f'forward want_output={wo}', lambda: eng.forward(x, font, training=True, step=3, want_output=wo))
        say(f'forward_rows want_output={wo}', lambda: eng.forward_rows(rows, training=True, step=3, want_output=wo))
    say('loss_grad', lambda: (eng.forward(x8, font8, want_output=False), eng.loss_grad(t8), eng.loss_grad(tf[:8], mean_elems=77)))
    say('loss_grad_rows', lambda: (eng.forward_rows(rows8, want_output=False), eng.loss_grad_rows(rows8), eng.loss_grad_rows(rows8, mean_elems=77)))
    say('forward_loss whole batch', lambda: eng.forward_loss(x, t, font))
    say('forward_loss_rows whole batch', lambda: eng.forward_loss_rows(rows))
    say('forward_loss + backward', lambda: (eng.forward_loss(x8, tf[:8], font8, step=5, mean_elems=77), eng.backward()))
    say('forward_loss_rows + backward stages', lambda: (eng.forward_loss_rows(rows8), [eng.backward_stage(s) for s in range(eng.backward_stages)]))
    for do_step in (True, False):
        for step in (9, None):
            say(f'train_step do_step={do_step} step={step}', lambda: eng.train_step(x, t, font, step=step, lr=2e-3, do_step=do_step))
            say(f'train_step_rows do_step={do_step} step={step}', lambda: eng.train_step_rows(rows, step=step, weight_decay=1e-3, mean_elems=99, do_step=do_step))
    say('evaluate', lambda: (eng.evaluate(x, t, font), eng.evaluate(x, tf, font, want_u8=True)))
    say('evaluate_rows', lambda: eng.evaluate_rows(rows, want_u8=True))
    say('evaluate_last', lambda: (eng.forward(x8, font8, want_output=False), eng.evaluate_last(target=t8), eng.evaluate_last(),
                                  eng.forward_rows(rows8, want_output=False), eng.evaluate_last(rows=rows8, want_u8=True)))
    say('render_u8', lambda: eng.render_u8(x, font))
    say('adamw_step', lambda: eng.adamw_step(lr=3e-3))
    say('clip', lambda: (eng.set_grad_clip(1.0), eng.train_step(x8, t8, font8), eng.grad_sumsq(), eng.grad_sumsq(4, 8), eng.set_grad_clip(None)))
    snap = mk('snap', eng.flat_params.clone())
    say('tensor_stats', lambda: (eng.tensor_stats('grads'), eng.tensor_stats('params', minus=snap)))
    say('ema', lambda: (eng.set_ema(0.9, 2), eng.train_step(x8, t8, font8), eng.ema_update(), eng.ema_update(sumsq=mk('ss', torch.ones(1)))))

    def in_ema():
        with eng.ema_weights():
            eng.forward(x8, font8)
            eng.train_step(x8, t8, font8)
    say('ema_weights', in_ema)
    if micro is None:
        x12, font12, t12 = (None if v is None else mk(lb, v) for lb, v in zip(('x12', 'font12', 't12'), data(cfg, 12, 21)))
        say('above max_batch', lambda: (eng.forward(x12, font12, want_output=False), eng.train_step(x12, t12, font12)))
    eng.lib = eng.lib.lib                      # (the proxy and the engine refer to each other)


def ranges(cfg):
    for opt in ('adamw', 'lion'):
        MINE.clear()
        eng = Engine(cfg, max_batch=8, optimizer=opt, max_grad_norm=1.0)
        eng.lib = Recorder(eng)
        ss = mk('ss', torch.ones(1))
        for groups in (False, True):
            eng.set_param_groups(*(({eng.layout[0][0]: 0.5}, None) if groups else (None, None)))
            for s in (None, ss):
                say(f'adamw_range {opt} groups={groups} sumsq={"given" if s is not None else None}', lambda: eng.adamw_range(8, 16, lr=2e-3, sumsq=s))
        eng.lib = eng.lib.lib


if __name__ == '__main__':
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):       # a stream of its own: its handle is not 0, so it prints apart from NULL
        glyph = GlyphConfig(hidden=(48, 40), out_h=4, out_w=6, n_fonts=2)
        for cfg in (glyph, PixelConfig(out_h=2, out_w=4, d_model=64, heads=1, layers=1, ff_dim=32, n_fonts=2),
                    SheetConfig(max_length=10, sheet_h=8, sheet_w=24)):
            for dtype in ('f32', 'bf16'):
                for B, micro in ((8, None), (20, 8)):
                    print(f'## {type(cfg).__name__} {dtype} batch {B} micro_batch {micro}')
                    script(cfg, dtype, B, micro)
        print('## adamw_range')
        ranges(glyph)
        torch.cuda.synchronize()
