"""The optimizer paths, stated once for the GPU tests of every feature that touches the step (clip, Lion, EMA, groups, BCE, rows): the
four step forms -- fused, unfused, split, rows (forms, steps_of) --, micro-batch accumulation (ACC_CASE), the cooperative split-K tail
(COOP_CASE) and the data-parallel schedules at a world of one (DP_CASES, rccl_world_one); and what two engines that took such paths are
compared on (assert_same_state).  DESIGN.md 4 has the table.  A plain module: the test files import what they use, the fixture included."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

from ai_font_renderer_amd.config import C5_MINI, WORKLOADS

from .op_harness import bits  # the bit patterns: -0.0 is not +0.0, and a NaN equals itself
from .util import MINI, GlyphConfig, glyph_inputs, synth

UNFUSED = 1                                    # AFR_CFG_UNFUSED_OPTIMIZER
SMALL = GlyphConfig(hidden=(48, 40), out_h=4, out_w=6, n_fonts=2)       # the glyph twin's small net

_made = []


@pytest.fixture(autouse=True)
def no_error_bits_left_behind():
    """error_flags() == 0 after every test, on every engine the test made with engine()."""
    _made.clear()
    yield
    engines = list(_made)
    _made.clear()
    for eng in engines:
        assert eng.error_flags() == 0


def engine(cfg, dtype="f32", max_batch=64, *, load=True, **kw):
    from ai_font_renderer_amd.engine import Engine
    eng = Engine(cfg, dtype=dtype, max_batch=max_batch, **kw)
    if load:
        eng.load_params(synth.make_params(cfg))
    _made.append(eng)
    return eng


# ----------------------------------------------------------------------------- what two engines are compared on
def same(a, b):
    return torch.equal(bits(a), bits(b))


def shadows(eng):
    """The bf16 weight shadow(s) that lead the workspace of a bf16 plan, whole.  A glyph plan keeps TWO, 256-byte aligned one behind the
    other, whose roles swap after every fused step."""
    if eng.dtype != "bf16":
        return []
    n2 = eng.n_flat * 2
    bufs = [eng.workspace[:n2].view(torch.bfloat16)]
    if eng.cfg.kind == "glyph":
        o2 = (n2 + 255) // 256 * 256
        bufs.append(eng.workspace[o2:o2 + n2].view(torch.bfloat16))
    return bufs


def state(eng):
    """(params, exp_avg, and exp_avg_sq where the engine keeps it) as name -> a copy of the tensor's elements."""
    flats = [f for f in (eng.flat_params, eng.exp_avg, eng.exp_avg_sq) if f is not None]
    return tuple({nm: f[o:o + k].clone() for nm, _, o, k in eng.layout} for f in flats)


def _flats(a, b, ema, with_shadows):
    """(tag, a's flat buffer, b's) of everything an optimizer step writes."""
    out = [("param", a.flat_params, b.flat_params), ("exp_avg", a.exp_avg, b.exp_avg)]
    assert (a.exp_avg_sq is None) == (b.exp_avg_sq is None)
    if a.exp_avg_sq is not None:
        out.append(("exp_avg_sq", a.exp_avg_sq, b.exp_avg_sq))
    if ema is None:
        ema = a.flat_ema is not None and b.flat_ema is not None
    if ema:
        out.append(("ema", a.flat_ema, b.flat_ema))
    if with_shadows:
        sa, sb = shadows(a), shadows(b)
        assert len(sa) == len(sb)
        out += [(f"shadow{i}", x, y) for i, (x, y) in enumerate(zip(sa, sb))]
    return out


def _assert_spans_same(a, b, what, spans, ema, with_shadows):
    for tag, fa, fb in _flats(a, b, ema, with_shadows):
        for nm, o, k in spans:
            k = fa.numel() if k is None else k
            xa, xb = bits(fa[o:o + k]), bits(fb[o:o + k])
            assert torch.equal(xa, xb), (what, tag, nm, int((xa != xb).sum()))


def assert_same_state(a, b, what, ema=None, shadows=True, padding=False):
    """Two engines hold the same state bit for bit: parameters, exp_avg, exp_avg_sq (AdamW), the EMA (ema=None: when both keep one), the
    bf16 shadow(s) of bf16 engines, and t.  Over the tensor elements (the padding between tensors is nobody's), or with padding=True
    over the whole flat buffers: for engines that took the same path.  shadows=False: for two engines whose step FORMS differ -- the
    fused step writes a glyph plan's other shadow and swaps the two, the flat kernel updates the current one in place."""
    spans = [("whole", 0, None)] if padding else [(nm, o, k) for nm, _, o, k in a.layout]
    _assert_spans_same(a, b, what, spans, ema, shadows)
    assert a.t == b.t, (what, a.t, b.t)


def assert_tensor_same(a, b, name, what):
    """Tensor `name` of engine a bit-identical to that of engine b: p, m, v, the EMA and the bf16 shadows over the tensor's elements."""
    (o, k), = [(o, k) for nm, _, o, k in a.layout if nm == name]
    _assert_spans_same(a, b, what, [(name, o, k)], None, True)


def assert_shadow_is_bf16_of_masters(eng, x, font):
    """One of the engine's shadows equals bf16 of the f32 masters, tensor by tensor, and -- the functional half -- a forward equals, bit
    for bit, that of a fresh engine whose shadow load_params derived from the same masters."""
    want = eng.flat_params.to(torch.bfloat16)
    assert any(all(same(b[o:o + k], want[o:o + k]) for _, _, o, k in eng.layout) for b in shadows(eng))
    fresh = engine(eng.cfg, "bf16", eng.max_batch)
    fresh.load_params(eng.state_dict())
    assert same(eng.forward(x, font), fresh.forward(x, font))


# ----------------------------------------------------------------------------- a state to step from
def probe_grads(cfg, dtype, x, t, font, step=1, **kw):
    """({name: gradient} on the CPU, global norm) of the batch at the initial parameters: what a seeded state and a max_norm are scaled by."""
    probe = engine(cfg, dtype, x.shape[0], **kw)
    probe.train_step(x, t, font=font, step=step, do_step=False)
    return {nm: probe.grads[nm].detach().cpu().clone() for nm, _, _, _ in probe.layout}, float(probe.grad_sumsq().sqrt())


def norm1(cfg, dtype, x, t, font, step=None, **kw):
    """The global gradient norm of the first step: the tests clip at 0.25 x this, so that the clip bites."""
    return probe_grads(cfg, dtype, x, t, font, step=step, **kw)[1]


def seed_moments(eng, M, V=None):
    """exp_avg (and exp_avg_sq, where the engine keeps it and V is given) from {name: tensor}."""
    for nm, _, o, k in eng.layout:
        eng.exp_avg[o:o + k].copy_(M[nm].reshape(-1))
        if V is not None and eng.exp_avg_sq is not None:
            eng.exp_avg_sq[o:o + k].copy_(V[nm].reshape(-1))


# ----------------------------------------------------------------------------- the shared cases: (cfg, B)
# data parallel: a glyph net and the sheet MINI model with its dropouts on (the step index keys the masks)
DP_CASES = ((SMALL, 300), (MINI, 37))
# accumulation: C5-mini, micro_batch 8 of 27 glyphs (test_gradient_accumulation_over_micro_batches_equals_the_whole_batch's case): three
# full micro-batches and a ragged one of 3
ACC_CASE = (C5_MINI, 27)
ACC_MICRO_BATCH = 8
# the cooperative split-K tail: C3's own layers at its batch of 8192.  afr_op_gemm_pair_plan reports the cooperative form for
# (8192, 1024, 1024) with a split of 8 (input-gradient tiles 32 x 4 + weight-gradient tiles 16 x 8 slices = 256 workgroups).  The form
# needs a split of 2, 4 or 8, N >= B / 8, at least 192 workgroups and 232 input-gradient tiles of 256 x 128: (6144, 768, 1024) is the only
# smaller shape in steps of 256 that qualifies, 0.56 of the work, and no workload has it -- so C3's own layer it is.
COOP_CASE = (WORKLOADS["c3"]["cfg"], 8192)


def inputs(case, device="cpu"):
    """(cfg, B, x, font, target u8) of a shared case."""
    cfg, B = case
    if cfg.kind == "glyph":
        x, font, t = glyph_inputs(cfg, B)
    elif cfg.kind == "sheet":
        x, font = synth.encode_strings(synth.dataset_strings(B), cfg.max_length), None
        t = synth.synth_sheet_targets(B, cfg.sheet_h, cfg.sheet_w, tensor_id=931)
    else:
        x = (32 + (np.arange(B) * 11) % 95).astype(np.int64)
        font = (np.arange(B) % 2).astype(np.int64)
        t = np.random.default_rng(9).integers(0, 256, (B, cfg.out_h, cfg.out_w), dtype=np.uint8)
    x, font, t = (None if a is None else torch.from_numpy(a).to(device) for a in (x, font, t))
    return cfg, B, x, font, t


def coop_inputs():
    """inputs(COOP_CASE), after asking the library that this shape takes the cooperative form and half of it does not."""
    from ai_font_renderer_amd import _lib
    sk, need = C.c_int(), C.c_size_t()
    assert _lib.lib().afr_op_gemm_pair_plan(COOP_CASE[1], 1024, 1024, C.byref(sk), C.byref(need)) == 0 and sk.value == 8
    assert _lib.lib().afr_op_gemm_pair_plan(4096, 1024, 1024, C.byref(sk), C.byref(need)) != 0
    return inputs(COOP_CASE)


def ran_coop_tail(eng):      # (eng.profile(1) before the step) the grouped 256 x 256 launch that carries the cooperative tail
    return any(r["kernel"].startswith("gemm_bf16_group256[") for r in eng.profile_table())


@contextlib.contextmanager
def rccl_world_one(schedule, monkeypatch):
    """A process group over RCCL with this process alone, and the stepper's schedule: "one-allreduce", "overlapped" (no minimum bucket
    size) or "shard-force" (the sharded update, which a world of one would not choose).  Yields torch.distributed."""
    import torch.distributed as dist
    from ai_font_renderer_amd import parallel
    monkeypatch.setattr(parallel, "OVERLAP_MIN_BYTES", 0 if schedule == "overlapped" else 1 << 40)
    if schedule == "shard-force":
        monkeypatch.setenv("AFR_DP_SCHEDULE", "shard-force")
    else:
        monkeypatch.delenv("AFR_DP_SCHEDULE", raising=False)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29600 + os.getpid() % 300))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        yield dist
    finally:
        dist.destroy_process_group()


def dp_steppers(dist, schedule, make):
    """(engine, its stepper on the schedule, a second engine, its single-process stepper) from make(), which builds one engine."""
    from ai_font_renderer_amd.parallel import DataParallelStepper
    eng, one = make(), make()
    st = DataParallelStepper(eng, dist, world=1 if schedule == "shard-force" else 2)      # (2: force the multi-rank code path)
    assert st.sharded() == (schedule == "shard-force")
    return eng, st, one, DataParallelStepper(one, None, 1)


# ----------------------------------------------------------------------------- the four step forms
def forms(cfg, dtype, B, x, t, font, **engine_kw):
    """(fused, unfused, split, rows): four engines in the same state, the last with the batch bound as its data set."""
    quartet = tuple(engine(cfg, dtype, B, flags=fl, **engine_kw) for fl in (0, UNFUSED, 0, 0))
    quartet[3].bind_dataset(x, t, font=font)
    return quartet


def steps_of(quartet, x, t, font, hyper, steps=3, same_loss=True):
    """Steps the four forms on the same batch and yields the step's index after each; the four losses are equal (same_loss=False: where
    the forms agree to the last bit only and the caller says which pairs it holds to what)."""
    fused, unfused, split, rows = quartet
    idx = torch.arange(x.shape[0])
    for i in range(steps):
        fused.train_step(x, t, font=font, step=i + 1, **hyper)
        unfused.train_step(x, t, font=font, step=i + 1, **hyper)
        split.train_step(x, t, font=font, step=i + 1, do_step=False)
        split.adamw_step(**hyper)
        rows.train_step_rows(idx, step=i + 1, **hyper)
        if same_loss:
            assert fused.read_loss() == unfused.read_loss() == split.read_loss() == rows.read_loss(), i
        yield i


def step_forms(cfg, dtype, B, x, t, font, hyper, steps=3, **engine_kw):
    """The quartet of forms() after `steps` steps of steps_of()."""
    quartet = forms(cfg, dtype, B, x, t, font, **engine_kw)
    for _ in steps_of(quartet, x, t, font, hyper, steps):
        pass
    return quartet
