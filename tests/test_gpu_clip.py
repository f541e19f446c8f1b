"""GPU: clipping by global gradient norm through the optimizer step (afr_set_grad_clip / afr_grad_sumsq / afr_op_adamw_clip):
the norm kernel against fp64, the clipped step against tests/clip_ref.py on the CPU oracle, and every path that ends in the
optimizer -- the one-call step, step by rows, gradient accumulation, the three data-parallel schedules.

Adam's update m / sqrt(v) is almost invariant to a scale of the gradient, so every trajectory check here asserts exp_avg and
exp_avg_sq (which carry coef and coef^2), not only the parameters: the parameters alone would pass without the feature."""
import functools

import numpy as np
import pytest
import torch

from . import clip_ref, lion_ref
from . import opt_paths as OP
from .opt_paths import UNFUSED, assert_same_state, no_error_bits_left_behind  # noqa: F401
from .opt_paths import engine as _engine
from .opt_paths import state as _state
from .util import MINI, glyph_inputs, load, maxabs, tparams

pytestmark = pytest.mark.gpu


def _case(name):
    """(cfg, x, font, target u8, lr) of a fixture's inputs: lion_ref.case's, with the fixture's own learning rate."""
    lr = float(load("pixel_twin.npz")["lr"]) if name == "c5-mini" else 1e-3
    return (*lion_ref.case("glyph-c1" if name == "c1" else name), lr)


# ----------------------------------------------------------------------------- 1. the norm kernel
def _chain(eng, lo, hi):
    """d: the longest chain of additions between one g^2 and the kernel's result for the range [lo, hi) (grad_sumsq_kernel).  A
    block belongs to one tensor and its lanes take q float4 each, q the smallest power of two for which the blocks of all
    tensors -- ceil(float4s / (256 q)), at least one per tensor in the range -- fit the 1024-block grid: per lane one
    accumulator per float4 component takes q terms, plus a tail element; then (a0 + a1) + (a2 + a3): 2; the wave shuffle: 6; the
    four waves: 2; the finisher: ceil(blocks / 256) per lane and 8 levels of its LDS tree.  All terms are non-negative, so each
    addition loses at most 2^-24 of the total."""
    sizes = [min(o + k, hi) - max(o, lo) for _, _, o, k in eng.layout if min(o + k, hi) > max(o, lo)]
    q = 1
    while True:
        blocks = sum(max(1, -(-(n // 4) // (256 * q))) for n in sizes)
        if blocks <= 1024:
            break
        q *= 2
    return q + 1 + 2 + 6 + 2 + -(-max(blocks, 1) // 256) + 8


@pytest.mark.parametrize("model", ["c5-mini", "c3"])
def test_grad_sumsq_vs_fp64_ranges_and_padding(model):
    """C5-mini has a 1-element tensor (the head's bias) and many tensors whose size is no multiple of 64; C3 has 2.1 M elements:
    more than the 1024-block grid covers with one float4 per lane.  Gradients seeded, EVERY padding element 1e3 (one of them in the sum would be
    off by orders of magnitude)."""
    from ai_font_renderer_amd.config import C5_MINI, WORKLOADS
    cfg = C5_MINI if model == "c5-mini" else WORKLOADS["c3"]["cfg"]
    eng = _engine(cfg, max_batch=8, with_optimizer=False)
    gen = torch.Generator().manual_seed(1234)
    g = torch.full((eng.n_flat,), 1e3, dtype=torch.float32)
    ref = 0.0
    for _, _, o, k in eng.layout:
        g[o:o + k] = torch.randn(k, generator=gen) * 0.37
        ref += float((g[o:o + k].double() ** 2).sum())
    assert any(k == 1 for _, _, _, k in eng.layout) or model == "c3"
    assert any(k % 4 for _, _, _, k in eng.layout) or model == "c3"
    if model == "c3":
        assert sum(k for _, _, _, k in eng.layout) > 4 * 1024 * 256
    eng.flat_grads.copy_(g)
    u = 2.0 ** -24
    n = eng.n_flat
    a, b = eng.grad_sumsq(), eng.grad_sumsq(0, n)
    assert torch.equal(a, b)                                              # two consecutive calls: bit-equal
    d = _chain(eng, 0, n)
    rel = abs(float(a) - ref) / ref
    print(f"grad_sumsq {model}: {n} flat elements, d = {d}, relative error {rel / u:.2f} x 2^-24")
    assert rel <= d * u, (rel, d)

    def fp64_range(lo, hi):
        return sum(float((g[max(o, lo):min(o + k, hi)].double() ** 2).sum()) for _, _, o, k in eng.layout if min(o + k, hi) > max(o, lo))

    big = max(eng.layout, key=lambda r: r[3])
    cut = big[2] + (big[3] // 2) // 4 * 4                                  # inside the largest tensor
    assert big[2] < cut < big[2] + big[3]
    eighth = [n * i // 8 // 4 * 4 for i in range(8)] + [n]
    for cuts in ([0, cut, n], eighth):
        parts, dmax = [], 0
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            got = float(eng.grad_sumsq(lo, hi - lo))
            want = fp64_range(lo, hi)
            dd = _chain(eng, lo, hi)
            assert abs(got - want) <= dd * u * max(want, 1e-30), (lo, hi)
            parts.append(got)
            dmax = max(dmax, dd)
        assert abs(sum(parts) - ref) <= dmax * u * ref, len(cuts)
        assert abs(sum(parts) - float(a)) <= (dmax + d) * u * ref, len(cuts)
    # a range wholly inside padding: exactly zero
    pads = [((o + k + 3) // 4 * 4, (o + k + 63) // 64 * 64) for _, _, o, k in eng.layout if (o + k + 63) // 64 * 64 - (o + k + 3) // 4 * 4 >= 4]
    assert pads or model == "c3"                                           # (every C3 tensor is a multiple of 64 elements: no padding)
    for lo, hi in pads[:3] + pads[-1:]:
        assert float(eng.grad_sumsq(lo, hi - lo)) == 0.0, (lo, hi)
    assert float(eng.grad_sumsq(0, 0)) == 0.0
    assert eng.error_flags() == 0
    from ai_font_renderer_amd import _lib
    for off, cnt in ((2, 64), (0, n + 4)):
        with pytest.raises(_lib.AfrError):
            eng.grad_sumsq(off, cnt)


# ----------------------------------------------------------------------------- 2. a clip that does not bite changes no bit
@pytest.mark.parametrize("model,dtype", [("c1", "f32"), ("c3-shaped", "bf16"), ("sheet-mini", "f32"), ("c5-mini", "f32")])
def test_inactive_clip_equals_the_unfused_optimizer_step_bitwise(model, dtype):
    """max_norm = 4 x the step-1 norm: coef = 1, the factor is grad_scale itself and g * 1 is g.  The clipping plan takes the path
    AFR_CFG_UNFUSED_OPTIMIZER takes (C1: the fused glyph step + the plain grouped reduce; C3's shapes: cooperative split-K
    that stores its gradient), so three steps equal that flag's trajectory bit for bit: parameters and both moments."""
    from ai_font_renderer_amd.config import WORKLOADS
    if model == "c3-shaped":
        cfg, B = WORKLOADS["c3"]["cfg"], 256
        x, font, t = glyph_inputs(cfg, B)
        x, font, t, lr = torch.from_numpy(x), torch.from_numpy(font), torch.from_numpy(t), 1e-3
    else:
        cfg, x, font, t, lr = _case(model)
        B = x.shape[0]
    ref = _engine(cfg, dtype, B, flags=UNFUSED)
    ref.train_step(x, t, font=font, do_step=False)
    norm1 = float(ref.grad_sumsq().sqrt())
    assert np.isfinite(norm1) and norm1 > 0
    ref = _engine(cfg, dtype, B, flags=UNFUSED)
    clip = _engine(cfg, dtype, B, max_grad_norm=4.0 * norm1)
    for i in range(3):
        ref.train_step(x, t, font=font, lr=lr)
        clip.train_step(x, t, font=font, lr=lr)
        assert clip.clip_coef() == 1.0, i
        assert ref.read_loss() == clip.read_loss(), i
    assert_same_state(clip, ref, model)
    assert abs(clip.grad_norm() - float(clip.grad_sumsq().sqrt())) <= 1e-6 * clip.grad_norm()


# ----------------------------------------------------------------------------- 3. a clip that bites, against the oracle
@functools.lru_cache(maxsize=None)
def _clipped_reference(name):
    """Three clipped oracle steps (f32 on the CPU) at max_norm = 0.25 x the step-1 oracle norm; computed once per fixture."""
    cfg, x, font, t, lr = _case(name)
    tf = t.float() / 255.0
    P = tparams(cfg)
    M = {k: torch.zeros_like(v) for k, v in P.items()}
    V = {k: torch.zeros_like(v) for k, v in P.items()}
    _, G1 = clip_ref.forward_backward(P, x, tf, cfg, font=font)
    max_norm = 0.25 * float(np.sqrt(clip_ref.grad_sumsq(G1)))
    steps = []
    for i in range(3):
        loss, G, P, M, V, total, coef = clip_ref.clipped_train_step(P, M, V, i + 1, x, tf, cfg, max_norm, font=font, lr=lr)
        steps.append((float(loss), total, coef))
    return max_norm, G1, steps, P, M, V


@pytest.mark.parametrize("name,dtype", [("glyph-small", "f32"), ("glyph-c1", "f32"), ("sheet-mini", "f32"), ("sheet-mini", "bf16x3"),
                                        ("c5-mini", "f32")])
def test_active_clip_three_steps_vs_the_clipped_oracle(name, dtype):
    """Bounds: those of the unclipped trajectory tests of the same fixture -- glyph twin and sheet MINI in f32: losses 3e-6,
    parameters 2e-5 (test_golden_glyph_fixtures_through_the_engine, test_mini_three_adamw_steps_match_reference); MINI in
    bf16x3: losses 1e-5 relative, parameters 1e-4 (test_gpu_bf16x3); C5-mini: losses 5e-6, parameters 2e-5 of the largest
    entry with the floor of 3.2 lr (test_c5_mini_backward_and_adamw_trajectory_match_the_torch_nn_twin).  Those tests hold no
    moments; the moments are sums of (clipped) gradients and of their squares, so exp_avg is held to the same fixture's
    GRADIENT bar -- 1e-4 of the tensor's largest entry (4e-3 for C5-mini against an f32 reference, where a ReLU gate within
    rounding of zero flips) -- and exp_avg_sq to twice that.  grad_norm() / clip_coef(): 1e-5 relative per step."""
    cfg, x, font, t, lr = _case(name)
    B = x.shape[0]
    max_norm, G1, steps, P, M, V = _clipped_reference(name)
    eng = _engine(cfg, dtype, B, max_grad_norm=max_norm)
    plain = _engine(cfg, dtype, B)
    plain.train_step(x, t, font=font, do_step=False)
    loss_tol = {"c5-mini": 5e-6}.get(name, 3e-6)
    for i, (loss, total, coef) in enumerate(steps):
        eng.train_step(x, t, font=font, lr=lr)
        got = eng.read_loss()
        print(f"{name}/{dtype} step {i + 1}: loss {got:.7f} (ref {loss:.7f}), norm {eng.grad_norm():.6e} (ref {total:.6e}), coef {eng.clip_coef():.6f} (ref {coef:.6f})")
        assert abs(got - loss) <= (1e-5 * loss if dtype == "bf16x3" else loss_tol), i
        assert coef < 0.5 and abs(eng.clip_coef() - coef) <= 1e-5 * coef, i
        assert abs(eng.grad_norm() - total) <= 1e-5 * total, i
        if i == 0:        # the gradient buffer is left UNSCALED: it is what a step without clipping leaves, bit for bit
            for nm, _, o, k in eng.layout:
                assert torch.equal(eng.flat_grads[o:o + k], plain.flat_grads[o:o + k]), nm
                assert maxabs(eng.grads[nm].cpu().numpy(), G1[nm].numpy()) <= (4e-3 if name == "c5-mini" else 1e-4) * float(G1[nm].abs().max()), nm
    gp, gm, gv = _state(eng)
    gbar = 4e-3 if name == "c5-mini" else 1e-4
    E = getattr(cfg, "embed_dim", 0)
    for k in P:
        got = [d[k].cpu().numpy().reshape(-1) for d in (gp, gm, gv)]
        ref = [d[k].numpy().reshape(-1) for d in (P, M, V)]
        if name == "sheet-mini" and k == "attention.in_proj_bias":      # k-bias gradient is analytically 0: Adam amplifies rounding noise
            got, ref = [np.delete(a, np.s_[E:2 * E]) for a in got], [np.delete(a, np.s_[E:2 * E]) for a in ref]
        pbar = 1e-4 if dtype == "bf16x3" else max(2e-5 * float(np.abs(ref[0]).max()), 3.2 * lr) if name == "c5-mini" else 2e-5
        assert maxabs(got[0], ref[0]) <= pbar, (k, maxabs(got[0], ref[0]))
        assert maxabs(got[1], ref[1]) <= gbar * max(float(np.abs(ref[1]).max()), 1e-30), ("exp_avg", k)
        assert maxabs(got[2], ref[2]) <= 2 * gbar * max(float(np.abs(ref[2]).max()), 1e-30), ("exp_avg_sq", k)


# ----------------------------------------------------------------------------- 4. entry points agree
@pytest.mark.parametrize("name,dtype", [("glyph-small", "f32"), ("glyph-c1", "bf16"), ("sheet-mini", "f32")])
def test_one_call_step_equals_backward_plus_adamw_step_and_the_step_by_rows(name, dtype):
    cfg, x, font, t, lr = _case(name)
    if name == "sheet-mini":
        cfg = MINI                                                         # with its dropouts: the step index keys the masks
    B = x.shape[0]
    max_norm = _clipped_reference(name)[0]                                # 0.25 x the step-1 norm: the clip bites
    quartet = OP.forms(cfg, dtype, B, x, t, font, max_grad_norm=max_norm)
    a, u, b, c = quartet                                                  # (every form of a clipping plan ends in the CLIP kernel)
    for _ in OP.steps_of(quartet, x, t, font, {}, steps=2):
        assert a.clip_coef() == u.clip_coef() == b.clip_coef() == c.clip_coef() < 1.0
    assert_same_state(a, u, "AFR_CFG_UNFUSED_OPTIMIZER")
    assert_same_state(a, b, "train_step(do_step=0) + adamw_step")
    assert_same_state(a, c, "train_step_rows")
    assert a.t == 2


# ----------------------------------------------------------------------------- 5. grad_scale
def test_grad_scale_enters_the_norm_and_the_update():
    """Gradients pre-multiplied by 8 with adamw_step(grad_scale=1/8): the norm |grad_scale| * sqrt(sumsq) and the factor
    fl32(grad_scale * coef) are those of the unscaled call up to one ulp (powers of two commute with every rounding except in
    the subnormal range of single g^2 terms), so the moments agree within a few ulps and the parameters within two."""
    cfg, x, font, t, lr = _case("glyph-small")
    B = x.shape[0]
    max_norm = _clipped_reference("glyph-small")[0]
    a, b = (_engine(cfg, "f32", B, max_grad_norm=max_norm) for _ in range(2))
    for e in (a, b):
        e.train_step(x, t, font=font, do_step=False)
    b.flat_grads.mul_(8.0)
    a.adamw_step()
    b.adamw_step(grad_scale=0.125)
    ulp = 2.0 ** -23
    assert abs(a.grad_norm() - b.grad_norm()) <= ulp * a.grad_norm()
    assert abs(a.clip_coef() - b.clip_coef()) <= ulp * a.clip_coef() and a.clip_coef() < 0.5
    (pa, ma, va), (pb, mb, vb) = _state(a), _state(b)
    for k in pa:
        assert float((ma[k] - mb[k]).abs().max()) <= 4 * ulp * float(ma[k].abs().max()), k
        assert float((va[k] - vb[k]).abs().max()) <= 8 * ulp * float(va[k].abs().max()), k
        assert float((pa[k] - pb[k]).abs().max()) <= 2 * ulp * float(pa[k].abs().max()), k
    # a negative scale: the norm takes |grad_scale|, the update the signed factor
    c = _engine(cfg, "f32", B, max_grad_norm=max_norm)
    c.train_step(x, t, font=font, do_step=False)
    c.flat_grads.mul_(-1.0)
    c.adamw_step(grad_scale=-1.0)
    assert c.grad_norm() == a.grad_norm() and c.clip_coef() == a.clip_coef()
    assert_same_state(c, a, "grad_scale = -1 on negated gradients")


# ----------------------------------------------------------------------------- 6. non-finite gradients skip the step
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_non_finite_gradients_skip_the_step_and_set_bit_3(dtype):
    cfg, x, font, t, lr = _case("glyph-small")
    B = x.shape[0]
    eng = _engine(cfg, dtype, B, max_grad_norm=1.0)
    eng.train_step(x, t, font=font, do_step=False)
    good = eng.flat_grads.clone()
    for bad in (float("inf"), float("nan")):
        eng.flat_grads.copy_(good)
        eng.flat_grads[eng.layout[2][2] + 5] = bad
        shadow = lambda: eng.workspace[:eng.n_flat * 2].clone()           # bf16: the weight shadow leads the workspace
        before = [v.clone() for v in (eng.flat_params, eng.exp_avg, eng.exp_avg_sq)] + [shadow()]
        eng.adamw_step()
        flags = eng.error_flags()
        assert flags & 8, flags
        for v, w in zip((eng.flat_params, eng.exp_avg, eng.exp_avg_sq, shadow()), before):
            assert torch.equal(v, w)
        assert eng.error_flags() == 0                                      # read-and-clear
    eng.flat_grads.copy_(good)
    p0 = eng.flat_params.clone()
    eng.adamw_step()
    assert eng.error_flags() == 0
    assert not torch.equal(eng.flat_params, p0) and bool(torch.isfinite(eng.flat_params).all())
    assert float(eng.exp_avg.abs().max()) > 0 and np.isfinite(eng.grad_norm())


# ----------------------------------------------------------------------------- 7. gradient accumulation
def test_clipped_step_over_micro_batches_equals_the_one_pass_clipped_step():
    """C5-mini, micro_batch 8 of 27 glyphs (test_gradient_accumulation_over_micro_batches_equals_the_whole_batch's case and its
    bound: gradients within 2e-5 of each tensor's largest entry).  The norm of a vector moves by at most the norm of its
    change, |norm_acc - norm_whole| <= sqrt(sum_k n_k (2e-5 max|g_k|)^2); the coefficient by that relative amount; exp_avg by
    the gradient's bound plus the coefficient's; two further steps at lr = 1e-5 keep the losses within 1e-5 (as there)."""
    cfg, B, x, font, tgt = OP.inputs(OP.ACC_CASE)
    probe = _engine(cfg, "f32", B)
    probe.train_step(x, tgt, font=font, do_step=False)
    norm1 = float(probe.grad_sumsq().sqrt())
    slack = float(np.sqrt(sum(k * (2e-5 * float(probe.flat_grads[o:o + k].abs().max())) ** 2 for _, _, o, k in probe.layout)))
    whole = _engine(cfg, "f32", B, max_grad_norm=0.25 * norm1)
    acc = _engine(cfg, "f32", B, max_grad_norm=0.25 * norm1, micro_batch=OP.ACC_MICRO_BATCH)
    assert acc.max_batch == 8
    for e in (whole, acc):
        e.train_step(x, tgt, font=font, lr=1e-5)
    assert abs(whole.read_loss() - acc.read_loss()) < 1e-6 * probe.read_loss()
    assert abs(whole.grad_norm() - norm1) <= 1e-6 * norm1
    assert abs(acc.grad_norm() - whole.grad_norm()) <= slack, (acc.grad_norm(), whole.grad_norm(), slack)
    crel = slack / norm1
    assert abs(acc.clip_coef() - whole.clip_coef()) <= (crel + 1e-6) * whole.clip_coef() and whole.clip_coef() < 0.26
    (_, mw, _), (_, ma, _) = _state(whole), _state(acc)
    for k in mw:
        assert float((mw[k] - ma[k]).abs().max()) <= (2e-5 + crel) * float(mw[k].abs().max()), k
    for e in (whole, acc):
        for _ in range(2):
            e.train_step(x, tgt, font=font, lr=1e-5)
    assert abs(whole.read_loss() - acc.read_loss()) < 1e-5
    assert acc.t == whole.t == 3 and acc.clip_coef() < 1.0


# ----------------------------------------------------------------------------- 8. data parallel, RCCL world 1
@pytest.mark.parametrize("schedule", ["one-allreduce", "overlapped", "shard-force"])
def test_data_parallel_schedules_equal_the_single_gpu_clipped_step_bitwise(schedule, monkeypatch):
    """A glyph net and the sheet MINI model (dropout on), f32 and bf16, through the multi-rank code path at a world of one:
    every schedule ends in the same norm kernel and the same clipped update as the single-GPU step (sharded: the shard's range
    is the whole buffer, its walk is identical; its sum goes through all_reduce and afr_op_adamw_clip)."""
    with OP.rccl_world_one(schedule, monkeypatch) as dist:
        for (cfg, B, x, font, t) in (OP.inputs(c, "cuda") for c in OP.DP_CASES):
            for dtype in ("f32", "bf16"):
                max_norm = 0.25 * OP.norm1(cfg, dtype, x, t, font, step=1)
                me = B * cfg.pixels
                eng, st, one, st1 = OP.dp_steppers(dist, schedule, lambda: _engine(cfg, dtype, B, max_grad_norm=max_norm))
                for i in range(3):
                    st.step(x, t, font, mean_elems=me, step=i + 1)
                    st1.step(x, t, font, mean_elems=me, step=i + 1)
                    assert one.clip_coef() < 0.5
                    if schedule != "shard-force":                            # (the sharded update has no plan to leave statistics with)
                        assert eng.clip_coef() == one.clip_coef() and eng.grad_norm() == one.grad_norm()
                assert st.global_loss() == st1.global_loss(), (cfg.kind, dtype)
                assert_same_state(eng, one, (schedule, cfg.kind, dtype), shadows=False)
                assert torch.equal(eng.forward(x, font), one.forward(x, font))   # (bf16: the shadow was re-synced)


# ----------------------------------------------------------------------------- the Python surface
def test_engine_surface_replanning_and_the_facade(monkeypatch):
    from ai_font_renderer_amd import _lib, model as M
    cfg, x, font, t, lr = _case("glyph-small")
    eng = _engine(cfg, "f32", 64, max_grad_norm=0.5)
    eng.train_step(x, t, font=font)                                        # 300 rows > 64: ensure_batch re-creates the plan
    assert eng.max_batch >= 300 and eng.max_grad_norm == 0.5
    c1 = eng.clip_coef()
    assert 0.0 < c1 <= 1.0 and abs(c1 - min(1.0, 0.5 / (eng.grad_norm() + 1e-6))) <= 1e-6
    with pytest.raises(ValueError):
        eng.set_grad_clip(-1.0)
    eng.set_grad_clip(None)                                                # off: the fused default step again, no statistics
    with pytest.raises(_lib.AfrError):
        eng.grad_norm()
    off = _engine(cfg, "f32", 300)
    off.train_step(x, t, font=font)
    off.train_step(x, t, font=font)
    eng2 = _engine(cfg, "f32", 300, max_grad_norm=0.5)
    eng2.set_grad_clip(0)
    eng2.train_step(x, t, font=font)
    eng2.train_step(x, t, font=font)
    assert_same_state(eng2, off, "clipping switched off")
    monkeypatch.setattr(M, "SHEET_HEIGHT", 8)
    monkeypatch.setattr(M, "SHEET_WIDTH", 24)
    monkeypatch.setattr(M, "CLIP_NORM", 0.75)                              # what AFR_CLIP_NORM=0.75 sets at import
    m = M.AttentionFontRenderer(max_length=10, max_batch=8)
    assert m.max_grad_norm == 0.75 and m.engine.max_grad_norm == 0.75
    m = M.AttentionFontRenderer(max_length=10, max_batch=8, max_grad_norm=0)
    assert m.max_grad_norm is None
