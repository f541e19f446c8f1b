"""GPU: the Lion optimizer kind (afr_set_optimizer / afr_op_lion / Engine(optimizer="lion")) through every optimizer path: the
elementwise kernel against fp64, one training step of every fused site against the CPU oracle (tests/lion_ref.py), the cooperative
split-K tail, the bitwise equalities between the paths that end in the optimizer, the state and surface, and that it trains.

The sign makes Lion discontinuous; lion_ref.compare therefore checks EVERY element -- the moment everywhere, decided parameters
against the reference, undecided ones against the three legal outcomes -- and the undecided share is capped at 2 % of the model
(tests/test_lion_cpu.py holds the reference alone to that cap for every input used here)."""
import functools

import numpy as np
import pytest
import torch

from . import clip_ref, lion_ref
from . import opt_paths as OP
from .gpu_util import ptr, stream
from .lion_ref import B1, B2, LR, WD
from .opt_paths import assert_same_state, no_error_bits_left_behind  # noqa: F401
from .opt_paths import assert_shadow_is_bf16_of_masters as _assert_shadow_is_bf16_of_masters
from .opt_paths import state as _state
from .util import MINI

pytestmark = pytest.mark.gpu

HYPER = dict(lr=LR, betas=(B1, B2), weight_decay=WD)
_engine = functools.partial(OP.engine, optimizer="lion")


# ----------------------------------------------------------------------------- 1. the elementwise kernel (site 1), op level
def _op_lion(p, g, m, shadow, lr, b1, b2, wd, gscale, sumsq, max_norm):
    from ai_font_renderer_amd import _lib
    _lib.check(_lib.lib().afr_op_lion(ptr(p), ptr(g), ptr(m), ptr(shadow), p.numel(), lr, b1, b2, wd, gscale, ptr(sumsq), max_norm, stream()))
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [64, 4 * (4096 * 256 + 3)])
def test_op_lion_vs_fp64_every_element(n):
    """n = 64, and the first size at which the 4096-block grid cap makes lanes loop.  With and without the bf16 shadow, without
    sumsq_dev and with one that clips (coef < 1) and one that does not (coef = 1), grad_scale 1 and 0.5.  Reference: lion_step in
    fp64 on the f32 product g * fl32(grad_scale * coef) the kernel forms.  tau = 4 x 2^-24 x max(|g|, |m|) per element: c is two
    f32 operations on values of that size.  Bounds, per element: the moment 4 x 2^-24 x max(|g|, |m|) likewise; the parameter
    4 x 2^-24 x (|p| + lr): p decay - lr s is one FMA on a decay that carries two roundings."""
    gen = torch.Generator().manual_seed(20 + n % 7)
    p0 = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * 0.37
    m0 = torch.randn(n, generator=gen) * 0.37
    g[5], m0[5] = 0.0, 0.0                                                # c exactly zero: decay only
    m0[9] = -g[9] / 9.0                                                   # c within rounding of zero
    u = 2.0 ** -24
    lr, b1, b2, wd = (float(np.float32(v)) for v in (LR, B1, B2, WD))
    sumsq_of_g = float((g.double() ** 2).sum())
    undecided_total = 0
    for with_shadow, gscale, clip in ((False, 1.0, None), (True, 1.0, None), (True, 0.5, "bites"), (False, 0.5, "idle"), (True, 1.0, "idle")):
        p, m = p0.clone().cuda(), m0.clone().cuda()
        shadow = torch.zeros(n, dtype=torch.bfloat16, device="cuda") if with_shadow else None
        factor, ss, max_norm = np.float32(gscale), None, 0.0
        if clip:
            max_norm = (0.25 if clip == "bites" else 4.0) * abs(gscale) * sumsq_of_g ** 0.5
            ss = torch.tensor([sumsq_of_g], dtype=torch.float32).cuda()
            coef = clip_ref.clip_coef(float(ss), max_norm, gscale)[1]
            assert (coef < 0.5) if clip == "bites" else (coef == 1.0)
            factor = np.float32(gscale) * np.float32(coef)
        _op_lion(p, g.cuda(), m, shadow, LR, B1, B2, WD, gscale, ss, max_norm)
        ge = (g * torch.tensor(factor)).float()                          # one rounded product, as the kernel forms it
        rp, rm, c = lion_ref.lion_step(p0, ge, m0, lr, b1, b2, wd)
        size = torch.maximum(ge.abs(), m0.abs()).double()
        dm = (m.cpu().double() - rm).abs()
        assert bool((dm <= 4 * u * size).all()), (with_shadow, clip, float((dm - 4 * u * size).max()))
        pbar = 4 * u * (p0.abs().double() + lr)
        und = c.abs() <= 4 * u * size
        got = p.cpu().double()
        assert bool(((got - rp).abs() <= pbar)[~und].all()), (with_shadow, clip)
        base = p0.double() * (1.0 - lr * wd)
        legal = torch.stack([(got - (base - lr * s)).abs() for s in (-1.0, 0.0, 1.0)]).min(0).values
        assert bool((legal <= pbar)[und].all()), (with_shadow, clip)
        assert bool(und[5]) and abs(float(got[5]) - float(base[5])) <= float(pbar[5])     # s = 0 where c = 0
        if with_shadow:
            assert torch.equal(shadow, p.to(torch.bfloat16))
        undecided_total += int(und.sum())
    print(f"afr_op_lion n = {n}: {undecided_total} undecided of {5 * n}")
    assert undecided_total <= lion_ref.CAP * 5 * n + 10                  # (n = 64: the two planted ones per variant)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_op_lion_non_finite_sumsq_leaves_everything_bit_identical(bad):
    gen = torch.Generator().manual_seed(5)
    n = 4096
    p, g, m = (torch.randn(n, generator=gen).cuda() for _ in range(3))
    shadow = torch.full((n,), 3.0, dtype=torch.bfloat16, device="cuda")
    before = [t.clone() for t in (p, m, shadow)]
    _op_lion(p, g, m, shadow, LR, B1, B2, WD, 1.0, torch.tensor([bad], dtype=torch.float32).cuda(), 1.0)
    for t, w in zip((p, m, shadow), before):
        assert torch.equal(t, w)
    _op_lion(p, g, m, shadow, LR, B1, B2, WD, 1.0, torch.tensor([1.0], dtype=torch.float32).cuda(), 1.0)
    assert not torch.equal(p, before[0]) and not torch.equal(m, before[1]) and torch.equal(shadow, p.to(torch.bfloat16))


# ----------------------------------------------------------------------------- 2. one training step per fused site, against the oracle
ORACLE_CASES = [("glyph-small", "f32"), ("glyph-small", "bf16"),        # the generic per-layer kernels (grouped reduce + the Lion kernel)
                ("glyph-c1", "f32"), ("glyph-c1", "bf16"),              # the fused small-net step: grouped reduce with shT copies
                ("sheet-mini", "f32"), ("sheet-mini", "bf16x3"), ("sheet-mini", "bf16"),     # the three weight-gradient epilogues
                ("sheet-deep", "f32"), ("sheet-deep", "bf16"),          # 37 partial slabs: the grouped reduce's deep branch
                ("c5-mini", "f32")]                                      # backward + the Lion kernel


# (the clipped step takes the same elementwise kernel in every dtype: the f32 cases cover it)
@pytest.mark.parametrize("name,dtype,clipped", [(n, d, False) for n, d in ORACLE_CASES] + [(n, d, True) for n, d in ORACLE_CASES if d == "f32"])
def test_one_lion_step_from_a_seeded_moment_vs_the_oracle(name, dtype, clipped):
    """tau: the existing absolute gradient bound of the model per tensor (lion_ref.grad_bar x max|g_ref|); parameters within the
    existing parameter bound, capped at lr / 4 (lion_ref.param_bar); exp_avg within lion_ref.moment_bar.  bf16: at the bf16 gradient
    bound (3e-2) every fixture leaves more than the cap undecided (test_lion_cpu.py: 21 % on sheet-mini), so only exp_avg is
    compared with the oracle there; the bf16 parameters are covered bit for bit by the path equalities and the shadow checks
    below.  sheet-deep: B = 37 strings leave min(B, 256) = 37 partial slabs, past the 32 from which the grouped reduce goes deep.
    clipped: max_norm = 0.25 x the step's own norm; the clipping plan materialises every gradient and ends in the CLIP kernel."""
    ref = lion_ref.reference(name, "f32" if dtype == "bf16x3" else dtype, clipped)
    cfg, x, font, t = lion_ref.case(name)
    eng = _engine(cfg, dtype, x.shape[0], max_grad_norm=ref["max_norm"])
    assert eng.exp_avg_sq is None
    OP.seed_moments(eng, ref["M"])
    p_old = _state(eng)[0]
    if name == "glyph-c1":
        eng.profile(1)
    eng.train_step(x, t, font=font, **HYPER)
    loss = eng.read_loss()
    ltol = 3e-2 * ref["loss"] if dtype == "bf16" else 1e-5 * ref["loss"] if dtype == "bf16x3" else 5e-6 if name == "c5-mini" else 3e-6
    assert abs(loss - ref["loss"]) <= ltol, (loss, ref["loss"])
    if name == "glyph-c1":
        assert any(r["kernel"].startswith("glyph1_step") for r in eng.profile_table())      # the fused small-net step ran
        eng.profile(0)
    if clipped:
        assert abs(eng.clip_coef() - ref["coef"]) <= 1e-5 * ref["coef"] and ref["coef"] < 0.5
    gp, gm = _state(eng)
    moment_only = dtype == "bf16"
    assert moment_only == (dtype == "bf16" and name in lion_ref.BF16_MOMENT_ONLY)
    und = total = 0
    for k in ref["P"]:
        und += lion_ref.compare(ref, k, p_old[k].view_as(ref["P"][k]), gp[k].view_as(ref["P"][k]), gm[k].view_as(ref["P"][k]),
                                lion_ref.param_bar(name, dtype, ref["new_p"][k]), lion_ref.moment_bar(name, dtype, ref, k), check_p=not moment_only)
        total += ref["P"][k].numel()
    print(f"{name}/{dtype} clipped={clipped}: loss {loss:.7f} (ref {ref['loss']:.7f}), undecided {und} of {total} = {und / total:.2e}")
    if not moment_only:
        assert und <= lion_ref.CAP * total
    if dtype == "bf16":                                                   # the shadow the next forward reads is bf16 of the new masters
        _assert_shadow_is_bf16_of_masters(eng, x, font)


# ----------------------------------------------------------------------------- 3. the cooperative split-K tail (site 5)
def test_cooperative_split_k_tail_equals_the_unfused_lion_step_bitwise():
    """C3's own layers at its batch of 8192 (opt_paths.COOP_CASE says why that shape).  One Lion step from a seeded moment, fused (the
    tail applies lion_quad) against AFR_CFG_UNFUSED_OPTIMIZER (the tail stores the gradient, the Lion kernel follows): parameters,
    moment and shadow bit for bit."""
    cfg, B, x, font, t = OP.coop_inputs()
    gen = torch.Generator().manual_seed(11)
    a, b = _engine(cfg, "bf16", B), _engine(cfg, "bf16", B, flags=OP.UNFUSED)
    m0 = (torch.randn(a.n_flat, generator=gen) * 1e-4).cuda()
    for e in (a, b):
        e.exp_avg.copy_(m0)
    a.profile(1)
    for e in (a, b):
        e.train_step(x, t, font=font, **HYPER)
    assert a.read_loss() == b.read_loss()
    assert OP.ran_coop_tail(a)
    assert_same_state(a, b, "cooperative tail", shadows=False)             # (each engine's current shadow is checked below)
    assert not torch.equal(a.exp_avg, m0)
    for e in (a, b):
        _assert_shadow_is_bf16_of_masters(e, x[:256], font[:256])


# ----------------------------------------------------------------------------- 4. path equalities, bitwise, three steps each
_norm1 = OP.norm1


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("name,dtype", [("glyph-small", "f32"), ("glyph-small", "bf16"), ("glyph-c1", "f32"), ("glyph-c1", "bf16"),
                                        ("sheet-mini", "f32"), ("sheet-mini", "bf16x3"), ("sheet-mini", "bf16"), ("sheet-deep", "bf16"),
                                        ("c5-mini", "f32")])
def test_fused_step_equals_unfused_step_and_the_step_by_rows_bitwise(name, dtype, clip):
    """The one-call step (optimizer fused into the grouped reduce / the weight-gradient epilogue), the same under
    AFR_CFG_UNFUSED_OPTIMIZER (every gradient materialised, then the Lion kernel), train_step(do_step=False) + adamw_step, and
    train_step_rows: given the same p, m, g every Lion site applies the same operations, so parameters and moment agree bit for
    bit after three steps -- with clipping off, and with a max_grad_norm of 0.25 x the step-1 norm (every path then ends in the CLIP
    kernel).  The sheet model runs with its dropouts here: the step index keys the masks."""
    cfg, x, font, t = lion_ref.case(name)
    if name.startswith("sheet"):
        cfg = MINI
    B = x.shape[0]
    kw = dict(max_grad_norm=0.25 * _norm1(cfg, dtype, x, t, font, step=1, optimizer="lion")) if clip else {}
    quartet = OP.forms(cfg, dtype, B, x, t, font, optimizer="lion", **kw)
    fused, unfused, split, rows = quartet
    for _ in OP.steps_of(quartet, x, t, font, HYPER):
        if clip:
            assert fused.clip_coef() == unfused.clip_coef() == split.clip_coef() == rows.clip_coef() < 1.0
    assert_same_state(fused, unfused, "AFR_CFG_UNFUSED_OPTIMIZER", shadows=False)
    assert_same_state(fused, split, "train_step(do_step=0) + adamw_step", shadows=False)
    assert_same_state(fused, rows, "train_step_rows")
    assert fused.t == 3
    if dtype == "bf16":
        for e in (fused, unfused):
            _assert_shadow_is_bf16_of_masters(e, x, font)


@pytest.mark.parametrize("clip", [False, True])
def test_micro_batch_accumulation_ends_in_the_same_lion_step_bitwise(clip):
    """C5-mini, micro_batch 8 of 27 glyphs.  Accumulated gradients differ from the whole batch's in the last bits (another order of
    summation: test_gpu_clip holds them to 2e-5), and a sign does not forgive that -- so the whole-batch engine is handed the
    accumulated gradient buffer and steps from it: what must be bit-equal is the optimizer step the accumulation path ends in."""
    cfg, B, x, font, tgt = OP.inputs(OP.ACC_CASE)
    kw = dict(max_grad_norm=0.25 * _norm1(cfg, "f32", x, tgt, font, optimizer="lion")) if clip else {}
    whole, acc = _engine(cfg, "f32", B, **kw), _engine(cfg, "f32", B, micro_batch=OP.ACC_MICRO_BATCH, **kw)
    assert acc.max_batch == 8 and acc.exp_avg_sq is None
    for i in range(3):
        acc.train_step(x, tgt, font=font, **HYPER)
        whole.train_step(x, tgt, font=font, do_step=False)
        scale = float(whole.flat_grads.abs().max())
        assert float((whole.flat_grads - acc.flat_grads).abs().max()) <= 2e-5 * scale      # (the accumulation itself, at its existing bound)
        whole.flat_grads.copy_(acc.flat_grads)
        whole.adamw_step(**HYPER)
        if clip:
            assert acc.clip_coef() == whole.clip_coef() < 1.0
    assert_same_state(acc, whole, "micro-batch accumulation")
    assert acc.t == 3


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("schedule", ["one-allreduce", "overlapped", "shard-force"])
def test_data_parallel_schedules_equal_the_single_gpu_lion_step_bitwise(schedule, clip, monkeypatch):
    """test_gpu_clip's data-parallel case with a Lion engine: a glyph net and the sheet MINI model (dropout on), f32 and bf16, over
    world-1 RCCL.  Every schedule ends in the Lion kernel on the same gradients as the single-GPU step (sharded: afr_op_lion on the
    slice, with the all-reduced sum of squares when clipping) -- the stepper needs no schedule of its own for the kind."""
    with OP.rccl_world_one(schedule, monkeypatch) as dist:
        for (cfg, B, x, font, t) in (OP.inputs(c, "cuda") for c in OP.DP_CASES):
            for dtype in ("f32", "bf16"):
                kw = dict(max_grad_norm=0.25 * _norm1(cfg, dtype, x, t, font, step=1, optimizer="lion")) if clip else {}
                me = B * cfg.pixels
                eng, st, one, st1 = OP.dp_steppers(dist, schedule, lambda: _engine(cfg, dtype, B, **kw))
                for i in range(3):
                    st.step(x, t, font, mean_elems=me, step=i + 1, **HYPER)
                    st1.step(x, t, font, mean_elems=me, step=i + 1, **HYPER)
                    if clip:
                        assert one.clip_coef() < 0.5
                assert st.global_loss() == st1.global_loss(), (cfg.kind, dtype)
                assert_same_state(eng, one, (schedule, cfg.kind, dtype), shadows=False)
                assert torch.equal(eng.forward(x, font), one.forward(x, font))   # (bf16: the shadow was re-synced)


# ----------------------------------------------------------------------------- 5. state and surface
def test_lion_engine_state_surface_and_switching_kinds(monkeypatch):
    from ai_font_renderer_amd import _lib, model as M
    from ai_font_renderer_amd.engine import Engine
    cfg, x, font, t = lion_ref.case("glyph-small")
    with pytest.raises(ValueError):
        Engine(cfg, optimizer="sgd")
    eng = _engine(cfg, "f32", 64)
    assert eng.exp_avg_sq is None and eng.optimizer == "lion"
    p0 = eng.flat_params.clone()
    eng.train_step(x, t, font=font, **HYPER)                              # 300 rows > 64: ensure_batch's new plan is a Lion plan again
    assert eng.max_batch >= 300 and not torch.equal(eng.flat_params, p0) and float(eng.exp_avg.abs().max()) > 0
    step = (eng.flat_params - p0 * (1.0 - LR * WD)).abs()
    live = torch.zeros_like(step, dtype=torch.bool)
    for _, _, o, k in eng.layout:
        live[o:o + k] = True
    assert float(step[live].max()) <= LR * 1.01 and float((step[live] > LR / 2).float().mean()) > 0.5      # |update| is lr or 0, mostly lr
    eng.reset_optimizer()                                                 # copes with the missing second moment
    assert eng.t == 0 and float(eng.exp_avg.abs().max()) == 0.0
    # Lion -> AdamW on a plan without exp_avg_sq: the next step is AFR_ESTATE, whichever entry point takes it
    _lib.check(eng.lib.afr_set_optimizer(eng._plan, _lib.AFR_OPT_ADAMW))
    before = eng.flat_params.clone()
    for call in (lambda: eng.train_step(x, t, font=font), lambda: eng.adamw_step()):
        with pytest.raises(_lib.AfrError, match="both moments"):
            call()
    assert torch.equal(eng.flat_params, before)
    _lib.check(eng.lib.afr_set_optimizer(eng._plan, _lib.AFR_OPT_LION))
    eng.train_step(x, t, font=font, **HYPER)
    assert not torch.equal(eng.flat_params, before)
    # AdamW -> Lion -> AdamW on a plan that has both moments: Lion steps leave exp_avg_sq alone
    both = _engine(cfg, "f32", 300, optimizer="adamw")
    both.train_step(x, t, font=font)
    v1 = both.exp_avg_sq.clone()
    assert float(v1.abs().max()) > 0
    _lib.check(both.lib.afr_set_optimizer(both._plan, _lib.AFR_OPT_LION))
    both.train_step(x, t, font=font, **HYPER)
    assert torch.equal(both.exp_avg_sq, v1)
    _lib.check(both.lib.afr_set_optimizer(both._plan, _lib.AFR_OPT_ADAMW))
    both.train_step(x, t, font=font)
    assert not torch.equal(both.exp_avg_sq, v1)
    with pytest.raises(_lib.AfrError):
        _lib.check(both.lib.afr_set_optimizer(both._plan, 2))
    # the facade
    monkeypatch.setattr(M, "SHEET_HEIGHT", 8)
    monkeypatch.setattr(M, "SHEET_WIDTH", 24)
    m = M.AttentionFontRenderer(max_length=10, max_batch=8)
    assert m.optimizer == "adamw" and m.engine.exp_avg_sq is not None and M._step_hyper(m.engine, 1e-3) == (1e-3, M.WEIGHT_DECAY)
    monkeypatch.setattr(M, "COMPUTE_OPTIMIZER", "lion")                   # what AFR_OPTIMIZER=lion sets at import
    m = M.AttentionFontRenderer(max_length=10, max_batch=8)
    assert m.optimizer == "lion" and m.engine.exp_avg_sq is None
    lr, wd = M._step_hyper(m.engine, M.LEARNING_RATE)
    assert abs(lr * wd - M.LEARNING_RATE * M.WEIGHT_DECAY) <= 1e-12 and abs(lr - M.LEARNING_RATE / 10) <= 1e-12
    m = M.AttentionFontRenderer(max_length=10, max_batch=8, optimizer="adamw")
    assert m.optimizer == "adamw"


def test_bf16_shadow_and_transposed_copies_follow_the_masters():
    """After a fused Lion step of the small net in bf16 the shadow and the transposed operand copies W1^T / W2^T the fused step
    reads (debug_read) equal bf16 of the new f32 masters; two steps, so that the second one has read what the first one left."""
    cfg, x, font, t = lion_ref.case("glyph-c1")
    eng = _engine(cfg, "bf16", x.shape[0])
    for _ in range(2):
        eng.train_step(x, t, font=font, **HYPER)
        _assert_shadow_is_bf16_of_masters(eng, x, font)
        for which, nm in (("w1t", "fc1.weight"), ("w2t", "fc_output.weight")):
            w = eng.params[nm]
            got = eng.debug_read(which)
            assert torch.equal(got.view(w.shape[1], w.shape[0]), w.to(torch.bfloat16).float().t()), which


# ----------------------------------------------------------------------------- 6. it trains
def test_thirty_lion_steps_of_glyph_small_lower_the_loss():
    """lr = 1e-4, wd = 5e-3 from a zero moment; the CPU reference does the same in test_lion_cpu.py.  No tighter relation between the
    two final losses is asserted: the trajectories part at the first undecided sign."""
    cfg, x, font, t = lion_ref.case("glyph-small")
    eng = _engine(cfg, "f32", x.shape[0])
    losses = []
    for _ in range(30):
        eng.train_step(x, t, font=font, **HYPER)
        losses.append(eng.read_loss())
    tf = t.float() / 255.0
    P = {k: v.cpu() for k, v in eng.state_dict().items()}
    ref_first, _ = lion_ref.forward_backward(lion_ref.tparams(cfg), x, tf, cfg, font=font)
    print(f"engine, glyph-small, 30 Lion steps: loss {losses[0]:.6f} -> {losses[-1]:.6f} (oracle's first loss {float(ref_first):.6f})")
    assert abs(losses[0] - float(ref_first)) <= 3e-6
    assert losses[-1] < losses[0] and all(np.isfinite(losses))
    assert all(bool(torch.isfinite(v).all()) for v in P.values())
