"""GPU: the weight EMA (afr_set_ema / afr_ema_update / afr_op_ema / afr_use_ema, Engine.set_ema / ema_weights) through every optimizer
path: the kernel against fp64, the skip on a non-finite sum of squares, the hook (once per due step, after the update), the paths and
data-parallel schedules that must end in the same EMA, evaluation from the EMA, the training loop, and a long replay.

"Bit for bit" below is the comparison of the 32-bit patterns (the padding between tensors may hold anything, NaN included).  Shapes:
the fixtures of tests/lion_ref.py, the smallest at which each optimizer path exists."""
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

from . import ema_ref, lion_ref
from . import opt_paths as OP
from .gpu_util import ptr, stream
from .opt_paths import assert_same_state, no_error_bits_left_behind  # noqa: F401
from .opt_paths import engine as _engine
from .opt_paths import same as _same
from .util import MINI, load, synth

pytestmark = pytest.mark.gpu

HYPER = {"adamw": dict(lr=1e-3), "lion": dict(lr=lion_ref.LR, betas=(lion_ref.B1, lion_ref.B2), weight_decay=lion_ref.WD)}
CASE_DTYPES = [(n, d) for n in lion_ref.CASES for d in ("f32", "bf16")]


def _op_ema(e, p, decay, sumsq=None, n=None):
    from ai_font_renderer_amd import _lib
    _lib.check(_lib.lib().afr_op_ema(ptr(e), ptr(p), p.numel() if n is None else n, decay, ptr(sumsq), stream()))
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 1. the kernel against fp64, every element
@pytest.mark.parametrize("decay", [0.999, 0.5])
@pytest.mark.parametrize("n", [64, 4 * (4096 * 256 + 3)])
def test_op_ema_vs_fp64_every_element(n, decay):
    """n = 64, and more than one sweep of the 4096-block grid plus a ragged tail of three quads.  Bound per element (ema_ref.bound):
    2^-22 max(|p|, |e_old|).  An eighth of the elements have p == e and must come back bit-identical; 64 sentinels behind e[n] stay."""
    p, e0, same = ema_ref.mixed(n, 40 + n % 5)
    buf = torch.full((n + 64,), -7.25, dtype=torch.float32)
    buf[:n] = e0
    buf, pd = buf.cuda(), p.cuda()
    _op_ema(buf, pd, decay, n=n)
    got = buf.cpu()
    assert torch.equal(got[n:], torch.full((64,), -7.25))
    err = (got[:n].double() - ema_ref.ema_step(e0, p, decay)).abs()
    bar = ema_ref.bound(p, e0)
    worst = float((err / bar.clamp_min(1e-300)).max())
    print(f"afr_op_ema n = {n}, decay = {decay}: worst error {worst:.3f} of the bound")
    assert bool((err <= bar).all()), worst
    assert _same(got[:n][same], e0[same]) and int(same.sum()) == (n + 4) // 8         # the indices 3, 11, 19, ... below n
    assert not _same(got[:n][~same], e0[~same])


# ----------------------------------------------------------------------------- 2. sumsq_dev
def test_op_ema_sumsq_finite_equals_null_and_non_finite_leaves_e_bit_identical():
    n = 4 * 4099
    p, e0, _ = ema_ref.mixed(n, 7)
    pd = p.cuda()
    plain = e0.clone().cuda()
    _op_ema(plain, pd, 0.9)
    assert not _same(plain, e0.cuda())
    gated = e0.clone().cuda()
    _op_ema(gated, pd, 0.9, torch.tensor([3.5e7], dtype=torch.float32).cuda())
    assert _same(gated, plain)
    for bad in (float("inf"), float("-inf"), float("nan")):
        e = e0.clone().cuda()
        _op_ema(e, pd, 0.9, torch.tensor([bad], dtype=torch.float32).cuda())
        assert _same(e, e0.cuda()), bad


# ----------------------------------------------------------------------------- 3. the hook: once per due step, after the update
@pytest.mark.parametrize("optimizer", ["adamw", "lion"])
@pytest.mark.parametrize("name,dtype", CASE_DTYPES)
def test_hook_fires_once_per_due_step_after_the_update_and_changes_nothing_else(name, dtype, optimizer):
    """Three engines take the same seven one-call steps: every = 1, every = 3, no EMA.  After each step the first one's flat_ema equals
    afr_op_ema applied by the test to its own copy with the engine's post-step parameters (the whole flat buffer, padding included);
    the second one's is unchanged after steps 1, 2, 4, 5, 7 and equals its replay after 3 and 6; parameters, moments, bf16 shadows
    and the loss of both equal the engine without an EMA throughout."""
    cfg, x, font, t = lion_ref.case(name)
    B, decay, hyper = x.shape[0], 0.9, HYPER[optimizer]
    e1, e3, off = (_engine(cfg, dtype, B, optimizer=optimizer, **kw) for kw in (dict(ema_decay=decay), dict(ema_decay=decay, ema_every=3), {}))
    assert _same(e1.flat_ema, e1.flat_params) and off.flat_ema is None and e3.ema_every == 3
    mine1, mine3 = e1.flat_ema.clone(), e3.flat_ema.clone()
    for i in range(1, 8):
        for e in (e1, e3, off):
            e.train_step(x, t, font=font, step=i, **hyper)
        assert e1.read_loss() == e3.read_loss() == off.read_loss(), i
        _op_ema(mine1, e1.flat_params, decay)
        assert _same(e1.flat_ema, mine1), i
        before = mine3.clone()
        if i % 3 == 0:
            _op_ema(mine3, e3.flat_params, decay)
            assert not _same(mine3, before)
        assert _same(e3.flat_ema, mine3), i
        for e in (e1, e3):
            assert_same_state(e, off, (i, "against the engine without an EMA"), ema=False)
    assert not _same(e1.flat_ema, e1.flat_params) and not _same(e1.flat_ema, e3.flat_ema)


# ----------------------------------------------------------------------------- 4. every path ends in the same EMA
def _norm1(cfg, dtype, x, t, font, optimizer):
    return OP.norm1(cfg, dtype, x, t, font, step=1, optimizer=optimizer)


def _paths_agree_bitwise(name, optimizer, clip):
    """Whether the parent's own suite holds the parameters of the un-fused step to the one-call step bit for bit: every Lion site does
    (test_gpu_lion), every clipped step ends in the one elementwise kernel (test_gpu_clip), the glyph nets' AdamW does
    (test_gpu_bench_shapes) -- but the sheet model's one-call AdamW step updates fc_output.weight inside its weight-gradient product,
    which agrees with the stand-alone kernel to the last bit only (test_gpu_bce says so).  There the parameters themselves differ in the
    last bit, so the two engines that step with the stand-alone kernel are compared with each other, the step by rows with the one-call
    step, and every engine's EMA with the replay from its own parameters (the hook fired once, after the update)."""
    return optimizer == "lion" or clip or not name.startswith("sheet")


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("optimizer", ["adamw", "lion"])
@pytest.mark.parametrize("name,dtype", CASE_DTYPES)
def test_every_path_ends_in_the_same_ema(name, dtype, optimizer, clip):
    """The one-call step, AFR_CFG_UNFUSED_OPTIMIZER, train_step(do_step=False) + adamw_step, and train_step_rows on a bound data set:
    three steps each with decay 0.9, clipping off and at 0.25 x the step-1 norm.  Every engine's EMA equals the replay of afr_op_ema
    over its own post-step parameters; and the whole state, EMA included, equals the one-call engine's bit for bit (_paths_agree_bitwise
    names the one exception the parent's arithmetic makes)."""
    cfg, x, font, t = lion_ref.case(name)
    B, decay, hyper = x.shape[0], 0.9, HYPER[optimizer]
    kw = dict(ema_decay=decay)
    if clip:
        kw["max_grad_norm"] = 0.25 * _norm1(cfg, dtype, x, t, font, optimizer)
    agree = _paths_agree_bitwise(name, optimizer, clip)
    engines = OP.forms(cfg, dtype, B, x, t, font, optimizer=optimizer, **kw)
    fused, unfused, split, rows = engines
    mine = [e.flat_ema.clone() for e in engines]
    for i in OP.steps_of(engines, x, t, font, hyper, same_loss=agree):
        for e, m in zip(engines, mine):
            _op_ema(m, e.flat_params, decay)
            assert _same(e.flat_ema, m), i
        if clip and i == 0:
            assert fused.clip_coef() < 0.26                               # the clip bites (later norms may have fallen below it)
    if agree:
        pairs = ((fused, unfused, "AFR_CFG_UNFUSED_OPTIMIZER"), (fused, split, "train_step(do_step=0) + adamw_step"), (fused, rows, "train_step_rows"))
    else:
        pairs = ((fused, rows, "train_step_rows"), (unfused, split, "train_step(do_step=0) + adamw_step against AFR_CFG_UNFUSED_OPTIMIZER"))
    for one, other, what in pairs:
        assert_same_state(one, other, what, shadows=False)


@pytest.mark.parametrize("clip", [False, True])
def test_micro_batch_accumulation_ends_in_the_same_ema(clip):
    """glyph-small, micro_batch 128 of 300: the accumulation path ends in adamw_step.  The whole-batch engine is handed the accumulated
    gradient buffer (another order of summation moves its own by last bits, test_gpu_lion) and steps from it: the optimizer step and
    the EMA behind it must be bit-equal, and the EMA equals its replay."""
    cfg, x, font, t = lion_ref.case("glyph-small")
    B, decay = x.shape[0], 0.9
    kw = dict(ema_decay=decay)
    if clip:
        kw["max_grad_norm"] = 0.25 * _norm1(cfg, "f32", x, t, font, "adamw")
    whole, acc = _engine(cfg, "f32", B, **kw), _engine(cfg, "f32", B, micro_batch=128, **kw)
    assert acc.max_batch == 128
    mine = acc.flat_ema.clone()
    for i in range(3):
        acc.train_step(x, t, font=font)
        whole.train_step(x, t, font=font, do_step=False)
        whole.flat_grads.copy_(acc.flat_grads)
        whole.adamw_step()
        _op_ema(mine, acc.flat_params, decay)
        assert _same(acc.flat_ema, mine), i
    assert_same_state(acc, whole, "micro-batch accumulation")
    assert acc.t == 3


def test_cooperative_split_k_tail_ends_in_the_same_ema():
    """C3's own layers at 8192 rows in bf16, the smallest shape that takes the cooperative split-K tail (opt_paths.COOP_CASE says why): the
    tail applies the optimizer inside the weight-gradient launch, the EMA pass follows the step's grouped reduce.  One-call step against
    AFR_CFG_UNFUSED_OPTIMIZER, two Lion steps with every = 2: unchanged after the first, the replay after the second, states bit-equal."""
    decay = 0.9
    cfg, B, x, font, t = OP.coop_inputs()
    a, b = (_engine(cfg, "bf16", B, optimizer="lion", flags=fl, ema_decay=decay, ema_every=2) for fl in (0, OP.UNFUSED))
    a.profile(1)
    start = a.flat_ema.clone()
    for e in (a, b):
        e.train_step(x, t, font=font, **HYPER["lion"])
    assert _same(a.flat_ema, start) and _same(b.flat_ema, start)
    for e in (a, b):
        e.train_step(x, t, font=font, **HYPER["lion"])
    table = a.profile_table()
    assert OP.ran_coop_tail(a)
    ema = [r for r in table if r["kernel"] == "ema"]
    assert len(ema) == 1 and ema[0]["launches"] == 1                       # one launch in two steps; 12 B per element (the table prints 6 digits)
    assert abs(ema[0]["algo_bytes"] - 12.0 * a.n_flat) <= 1e-5 * 12.0 * a.n_flat
    _op_ema(start, a.flat_params, decay)
    assert _same(a.flat_ema, start)
    assert_same_state(a, b, "cooperative tail", shadows=False)             # (the un-fused step updates its shadow in place, the fused one swaps two)
    assert _same(a.forward(x[:256], font[:256]), b.forward(x[:256], font[:256]))


# ----------------------------------------------------------------------------- 5. data-parallel schedules over world-1 RCCL
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("schedule", ["one-allreduce", "overlapped", "shard-force"])
def test_data_parallel_schedules_end_in_the_single_gpu_ema(schedule, clip, monkeypatch):
    """test_gpu_lion's data-parallel case with an EMA: a glyph net and the sheet MINI model (dropout on), f32 and bf16, Lion (whose
    schedules all equal the single-GPU step bit for bit), and AdamW where clipping makes them (every step then ends in the one
    elementwise kernel).  After three steps flat_ema and the whole state equal the single-GPU engine's."""
    with OP.rccl_world_one(schedule, monkeypatch) as dist:
        for optimizer in ("lion", "adamw") if clip else ("lion",):
            for (cfg, B, x, font, t) in (OP.inputs(c, "cuda") for c in OP.DP_CASES):
                for dtype in ("f32", "bf16"):
                    kw = dict(ema_decay=0.9)
                    if clip:
                        kw["max_grad_norm"] = 0.25 * _norm1(cfg, dtype, x, t, font, optimizer)
                    me = B * cfg.pixels
                    eng, st, one, st1 = OP.dp_steppers(dist, schedule, lambda: _engine(cfg, dtype, B, optimizer=optimizer, **kw))
                    for i in range(3):
                        st.step(x, t, font, mean_elems=me, step=i + 1, **HYPER[optimizer])
                        st1.step(x, t, font, mean_elems=me, step=i + 1, **HYPER[optimizer])
                    assert st.global_loss() == st1.global_loss(), (cfg.kind, dtype)
                    assert_same_state(eng, one, (schedule, optimizer, cfg.kind, dtype), shadows=False)
                    assert not _same(eng.flat_ema, eng.flat_params)
                    with eng.ema_weights(), one.ema_weights():
                        assert _same(eng.forward(x, font), one.forward(x, font))
                    assert _same(eng.forward(x, font), one.forward(x, font))       # (bf16: the shadow was re-synced)


# ----------------------------------------------------------------------------- 6. a skipped step
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_skipped_step_leaves_the_ema_bit_identical_and_still_counts(dtype):
    """A clipping plan with inf / NaN in flat_grads, as test_gpu_clip plants them: the step is skipped, bit 3 of the error word is set,
    and flat_ema stays bit-identical; the next finite step updates it.  With every = 2 the skipped step still advances the count (the
    host cannot know it was skipped): skipped step + one finite step make the EMA due."""
    cfg, x, font, t = lion_ref.case("glyph-small")
    B, decay = x.shape[0], 0.5
    eng = _engine(cfg, dtype, B, max_grad_norm=1.0, ema_decay=decay)
    eng.train_step(x, t, font=font)                                       # a first real step: the EMA differs from the parameters
    assert not _same(eng.flat_ema, eng.flat_params) and eng.error_flags() == 0
    eng.train_step(x, t, font=font, do_step=False)
    good = eng.flat_grads.clone()
    for bad in (float("inf"), float("nan")):
        eng.flat_grads.copy_(good)
        eng.flat_grads[eng.layout[2][2] + 5] = bad
        before = [v.clone() for v in (eng.flat_ema, eng.flat_params, eng.exp_avg, eng.exp_avg_sq)]
        eng.adamw_step()
        assert eng.error_flags() & 8
        for v, w in zip((eng.flat_ema, eng.flat_params, eng.exp_avg, eng.exp_avg_sq), before):
            assert _same(v, w), bad
    eng.flat_grads.copy_(good)
    mine = eng.flat_ema.clone()
    eng.adamw_step()
    _op_ema(mine, eng.flat_params, decay)
    assert _same(eng.flat_ema, mine) and not _same(mine, before[0]) and eng.error_flags() == 0
    # every = 2: [skipped, finite] -> due at the finite one; [finite] alone would not be
    eng.set_ema(decay, every=2)
    assert _same(eng.flat_ema, eng.flat_params)
    eng.flat_grads.copy_(good)
    eng.flat_grads[3] = float("nan")
    eng.adamw_step()
    assert eng.error_flags() & 8 and _same(eng.flat_ema, eng.flat_params)
    eng.flat_grads.copy_(good)
    mine = eng.flat_ema.clone()
    eng.adamw_step()
    _op_ema(mine, eng.flat_params, decay)
    assert _same(eng.flat_ema, mine) and not _same(eng.flat_ema, eng.flat_params) and eng.error_flags() == 0


# ----------------------------------------------------------------------------- 7. evaluation from the EMA
@pytest.mark.parametrize("name,dtype", CASE_DTYPES + [("sheet-mini", "bf16x3")])
def test_evaluation_from_the_ema(name, dtype):
    from ai_font_renderer_amd import _lib
    cfg, x, font, t = lion_ref.case(name)
    B = x.shape[0]
    eng, twin = (_engine(cfg, dtype, B, ema_decay=0.5) for _ in range(2))
    for e in (eng, twin):
        e.bind_dataset(x, t, font=font)
        for i in range(3):
            e.train_step(x, t, font=font, step=i + 1)
        e.read_loss()
    idx = torch.arange(B - 1, -1, -1)
    y_raw = eng.forward(x, font).clone()
    u_raw = eng.debug_read("u")
    other = _engine(cfg, dtype, B)
    other.load_params(eng.ema_state_dict())
    other.bind_dataset(x, t, font=font)
    y_want = other.forward(x, font).clone()
    u_want = other.debug_read("u")
    yr_want = other.forward_rows(idx).clone()
    other.loss_grad_rows(idx)
    loss_want = other.read_loss()
    # decay 0.5: the EMA differs visibly from the weights -- in the pre-activation output everywhere, in the clamped output wherever
    # the model does not saturate it (C5-mini's is 1.0 in every pixel at these parameters)
    assert not _same(eng.flat_ema, eng.flat_params) and not _same(u_want, u_raw)
    assert name == "c5-mini" or not _same(y_want, y_raw)
    saved = [v.clone() for v in (eng.flat_params, eng.flat_ema, eng.exp_avg, eng.exp_avg_sq, eng.flat_grads)]
    with eng.ema_weights():
        assert _same(eng.forward(x, font), y_want)
        assert _same(eng.debug_read("u"), u_want)                         # afr_debug_copy sees the EMA forward
        assert _same(eng.forward_rows(idx), yr_want)
        eng.loss_grad_rows(idx)
        assert eng.read_loss() == loss_want
        for call in (lambda: eng.train_step(x, t, font=font), lambda: eng.train_step_rows(idx), lambda: eng.forward_loss(x, t, font=font),
                     lambda: eng.forward_loss_rows(idx), lambda: eng.backward(), lambda: eng.backward_stage(0), lambda: eng.adamw_step(),
                     lambda: eng.ema_update(), lambda: eng.forward(x, font, training=True, step=1), lambda: eng.forward_rows(idx, training=True, step=1),
                     lambda: eng.set_ema(0.9), lambda: eng.load_params(eng.state_dict())):
            with pytest.raises(_lib.AfrError) as err:
                call()
            assert err.value.code == _lib.AFR_ESTATE, str(err.value)
        assert eng.lib.afr_set_optimizer(eng._plan, _lib.AFR_OPT_LION) == _lib.AFR_ESTATE
        assert eng.lib.afr_use_ema(eng._plan, 1, None) == _lib.AFR_OK      # the current state: a no-op
        assert _same(eng.forward(x, font), y_want)                        # nothing changed
        with pytest.raises(_lib.AfrError):                                # (no nesting)
            with eng.ema_weights():
                pass
        assert _same(eng.forward(x, font), y_want)
    assert eng.t == 3 and eng.read_loss() == 0.0
    for v, w in zip((eng.flat_params, eng.flat_ema, eng.exp_avg, eng.exp_avg_sq, eng.flat_grads), saved):
        assert _same(v, w)
    assert _same(eng.forward(x, font), y_raw) and _same(eng.debug_read("u"), u_raw)
    eng.loss_grad_rows(idx)
    eng.read_loss()
    with eng.ema_weights():
        pass
    with pytest.raises(_lib.AfrError):                                    # a forward saved before the switch is not followed by a backward
        eng.backward()
    for e in (eng, twin):
        for i in range(3, 6):
            e.train_step(x, t, font=font, step=i + 1)
    assert eng.read_loss() == twin.read_loss()
    assert_same_state(eng, twin, "after the context")


def test_replan_inside_and_outside_the_context_keeps_the_ema():
    """ensure_batch re-creates the plan: the EMA setting and buffer are applied to the new one (as clip and optimizer kind are) -- on a
    training step of 300 rows through a plan made for 64, and on a forward of 300 rows inside ema_weights()."""
    cfg, x, font, t = lion_ref.case("glyph-small")
    a, b = _engine(cfg, "bf16", 64, ema_decay=0.5), _engine(cfg, "bf16", 300, ema_decay=0.5)
    buf = a.flat_ema.data_ptr()
    for e in (a, b):
        e.train_step(x[:64], t[:64], font=font[:64])
    with a.ema_weights(), b.ema_weights():
        ya, yb = a.forward(x, font), b.forward(x, font)                   # a: 300 rows > 64 -- a new plan, inside the context
        assert a.max_batch >= 300 and _same(ya, yb)
    assert _same(a.forward(x, font), b.forward(x, font)) and not _same(ya, a.forward(x, font))
    for e in (a, b):
        e.train_step(x, t, font=font)
    assert a.flat_ema.data_ptr() == buf
    assert_same_state(a, b, "after the re-plan", shadows=False)            # (a's new plan starts with its first shadow current, b's has swapped)
    c = _engine(cfg, "f32", 64, ema_decay=0.5)
    mine = c.flat_ema.clone()
    c.train_step(x, t, font=font)                                         # the re-plan happens inside the training step
    _op_ema(mine, c.flat_params, 0.5)
    assert c.max_batch >= 300 and _same(c.flat_ema, mine) and not _same(mine, c.flat_params)
    c.reset_optimizer()
    assert _same(c.flat_ema, mine)                                        # reset_optimizer leaves the EMA alone
    c.load_params(c.state_dict())
    assert _same(c.flat_ema, c.flat_params)                               # load_params restarts it
    c.set_ema(None)
    assert c.flat_ema is None and c.ema_decay is None
    with pytest.raises(Exception):
        with c.ema_weights():
            pass
    p0 = c.flat_params.clone()
    c.train_step(x, t, font=font)
    assert not _same(c.flat_params, p0) and c.error_flags() == 0
    from ai_font_renderer_amd.engine import Engine
    for kw in (dict(ema_decay=0.0), dict(ema_decay=1.0), dict(ema_decay=0.9, ema_every=0)):
        with pytest.raises(ValueError):
            Engine(cfg, **kw)
    with pytest.raises(ValueError):
        c.set_ema(1.5)


# ----------------------------------------------------------------------------- 8. the loop
KEYS = ["positional_encoding", "embedding.weight", "attention.in_proj_weight", "attention.in_proj_bias", "attention.out_proj.weight",
        "attention.out_proj.bias", "layer_norm.weight", "layer_norm.bias", "fc1.weight", "fc1.bias", "fc_output.weight", "fc_output.bias"]


def _mini_model(M, monkeypatch, **kw):
    """The facade in miniature with the three dropouts off (as test_gpu_host builds it): an engine with zero rates, parameters re-pointed."""
    from ai_font_renderer_amd.engine import Engine
    for k, v in dict(SHEET_HEIGHT=8, SHEET_WIDTH=24, MAX_CHARS_PER_SHEET=10).items():
        monkeypatch.setattr(M, k, v)
    m = M.AttentionFontRenderer(max_length=10, max_batch=16, init=False, **kw)
    old = m.engine
    m.engine = Engine(replace(m.config, p_embed=0.0, p_attn=0.0, p_fc=0.0), dtype="f32", max_batch=16, device=M.device, ema_decay=old.ema_decay,
                      ema_every=old.ema_every)
    m.engine.load_params(synth.make_params(MINI))
    P = {k: torch.nn.Parameter(v) for k, v in m.engine.params.items()}
    for name in KEYS:
        mod_, _, attr = name.rpartition(".")
        (m.get_submodule(mod_) if mod_ else m)._parameters[attr] = P[name]
    return m


@pytest.mark.parametrize("by_rows", [True, False])
def test_run_epoch_validates_from_the_ema(by_rows, monkeypatch):
    """_run_epoch on the 80 sheets of the training-loop fixture (sheet-mini shapes, no dropout), batches of 16: the validation loss it
    returns is the loss of a fresh engine loaded with ema_state_dict() on the same rows, and not the raw weights'."""
    from ai_font_renderer_amd import model as M
    from ai_font_renderer_amd.parallel import DataParallelStepper
    fx = load("train_loop.npz")
    inputs = torch.from_numpy(fx["a/x"]).to(M.device)
    targets = torch.from_numpy(fx["a/target_u8"]).to(M.device)
    m = _mini_model(M, monkeypatch, ema_decay=0.5)
    eng = m.engine
    assert eng.ema_decay == 0.5 and eng.ema_every == 1
    eng.bind_dataset(inputs, targets)
    order = M._EpochOrder(inputs.shape[0])
    _, val = M._run_epoch(m, DataParallelStepper(eng, None, 1), order, inputs, targets, 16, 1e-2, 0, 1, by_rows=by_rows)
    assert not _same(eng.flat_ema, eng.flat_params)

    def val_loss(e):
        rows = order.val_idx.to(M.device)
        nvb = (rows.numel() + 15) // 16
        for b in range(nvb):
            r = rows[b * 16:(b + 1) * 16]
            e.forward_rows(r, want_output=False)
            e.loss_grad_rows(r)
        return e.read_loss() / nvb

    fresh = _engine(eng.cfg, "f32", 16)
    fresh.load_params(eng.ema_state_dict())
    fresh.bind_dataset(inputs, targets)
    raw = val_loss(eng)
    print(f"validation loss from the EMA {val:.7f}, from the raw weights {raw:.7f}")
    assert val == val_loss(fresh) and val != raw
    assert eng.error_flags() == 0


def test_facade_takes_the_ema_from_its_arguments_and_the_environment(monkeypatch):
    from ai_font_renderer_amd import model as M
    monkeypatch.setattr(M, "SHEET_HEIGHT", 8)
    monkeypatch.setattr(M, "SHEET_WIDTH", 24)
    monkeypatch.delenv("AFR_EMA", raising=False)
    m = M.AttentionFontRenderer(max_length=10, max_batch=8)
    assert m.engine.ema_decay is None and m.engine.flat_ema is None
    m = M.AttentionFontRenderer(max_length=10, max_batch=8, ema_decay=0.99, ema_every=4)
    assert (m.engine.ema_decay, m.engine.ema_every) == (0.99, 4) and _same(m.engine.flat_ema, m.engine.flat_params)
    monkeypatch.setenv("AFR_EMA", "0.9:2")
    m = M.AttentionFontRenderer(max_length=10, max_batch=8)
    assert (m.engine.ema_decay, m.engine.ema_every) == (0.9, 2)
    m = M.AttentionFontRenderer(max_length=10, max_batch=8, ema_decay=0.5)          # the argument wins
    assert (m.engine.ema_decay, m.engine.ema_every) == (0.5, 1)
    monkeypatch.setenv("AFR_EMA", "2")
    with pytest.raises(ValueError):
        M.AttentionFontRenderer(max_length=10, max_batch=8)


def test_training_ends_with_the_ema_in_the_model(tmp_path, monkeypatch):
    """Two epochs of train_attention_model on the 80 sheets: the EMA the loop took when training ended is what the model holds (and
    would save), it is not the raw weights of the last step, and config.txt carries the two lines."""
    from ai_font_renderer_amd import model as M
    fx = load("train_loop.npz")
    monkeypatch.chdir(tmp_path)
    for k, v in dict(NUM_EPOCHS=2, LEARNING_RATE=1e-2, OUTPUT_DIR="ema_out").items():
        monkeypatch.setattr(M, k, v)
    monkeypatch.setenv("AFR_EMA", "0.9:2")
    m = _mini_model(M, monkeypatch)
    eng = m.engine
    assert (eng.ema_decay, eng.ema_every) == (0.9, 2)
    taken = {}
    orig = eng.ema_state_dict

    def recording():
        taken["raw"] = eng.state_dict()
        taken["ema"] = orig()
        return taken["ema"]

    monkeypatch.setattr(eng, "ema_state_dict", recording)
    ds = torch.utils.data.TensorDataset(torch.from_numpy(fx["a/x"]), torch.from_numpy(fx["a/target_u8"].astype(np.float32) / 255.0))
    M.train_attention_model(m, ds, 16)
    sd = m.state_dict()
    assert list(sd.keys()) == KEYS
    for k in KEYS:
        assert _same(sd[k], taken["ema"][k]), k
    assert any(not _same(taken["ema"][k], taken["raw"][k]) for k in KEYS)
    assert _same(eng.flat_ema, eng.flat_params)                           # loading the average restarted it there
    lines = (tmp_path / "ema_out" / "config.txt").read_text().splitlines()
    assert "ema_decay = 0.9" in lines and "ema_every = 2" in lines
    assert sorted(os.listdir(tmp_path / "ema_out" / "epoch_0")) == sorted(f"string_{i}.bmp" for i in range(15))
    assert eng.error_flags() == 0


# ----------------------------------------------------------------------------- 9. a long replay
def test_thirty_lion_steps_stay_within_the_bound_of_the_fp64_replay():
    """glyph-small, 30 Lion steps, decay 0.99: the engine's EMA against ema_ref.ema_step in fp64 over the recorded post-step parameters.
    Each step adds at most 2^-22 max(|p|, |e|) of rounding, and earlier errors are carried with a factor decay < 1: within
    30 x 2^-22 x max|p| per tensor (max over the recorded parameters and the start)."""
    cfg, x, font, t = lion_ref.case("glyph-small")
    decay = 0.99
    eng = _engine(cfg, "f32", x.shape[0], optimizer="lion", ema_decay=decay)
    ref = eng.flat_ema.cpu().double()
    top = eng.flat_params.abs().cpu().double()
    for _ in range(30):
        eng.train_step(x, t, font=font, **HYPER["lion"])
        p = eng.flat_params.cpu()
        ref = ema_ref.ema_step(ref, p, decay)
        top = torch.maximum(top, p.abs().double())
    got = eng.flat_ema.cpu().double()
    worst = 0.0
    for nm, _, o, k in eng.layout:
        bar = 30 * 2.0 ** -22 * float(top[o:o + k].max())
        err = float((got[o:o + k] - ref[o:o + k]).abs().max())
        worst = max(worst, err / bar)
        assert err <= bar, (nm, err, bar)
    print(f"30 Lion steps, decay 0.99: worst tensor at {worst:.3f} of the bound")
    assert not _same(eng.flat_ema, eng.flat_params) and eng.error_flags() == 0
