"""GPU: the BCE loss kind (AFR_LOSS_BCE: sigmoid output head, binary cross-entropy on the logits) through every loss path --
the loss kernel, the f32 / bf16x3 tile epilogue, the bf16 ring epilogue, the fused small-net step, the pixel head, the
caller-side-loss entry, by rows, data parallel and the training CLI.

References: tests/bce_ref.py (the explicit formula, equal to F.binary_cross_entropy_with_logits: test_bce_cpu.py) on the CPU
oracle, and tests/golden/sheet_mini_bce.npz (the reference's own module graph with that loss; make_golden_bce.py).
Tolerances are the project's: f32 / bf16x3 bitmaps 2e-5 max-abs, gradients 1e-4 relative, losses 1e-5
relative; bf16 3e-2 relative against the oracle rounded at the engine's points (util.engine_rounding, u and du in bf16)."""
import functools
import os
from dataclasses import replace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from . import bce_ref
from . import opt_paths as OP
from .opt_paths import no_error_bits_left_behind  # noqa: F401
from .util import MINI, GlyphConfig, engine_rounding, fused1_eligible, glyph_inputs, load, maxabs, oracle, rnd_du, synth, tparams

pytestmark = pytest.mark.gpu


_engine = functools.partial(OP.engine, loss="bce")


def _rel(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return maxabs(got, ref) / max(1e-7, float(np.abs(ref).max()))


def _grads(eng):
    return {k: v.detach().cpu().numpy() for k, v in eng.grads.items()}


# ----------------------------------------------------------------------------- the loss kernel itself
@pytest.mark.parametrize("act", ["f32", "bf16"])
@pytest.mark.parametrize("tgt", ["u8", "f32"])
def test_op_bce_grad_vs_fp64_with_torchs_own_f32_deviation_as_the_yardstick(act, tgt):
    """afr_op_bce_grad on logits spread over [-30, 30] plus a ramp to +-104, 37 x 19200 (88 800 groups of 8 pixels: the last
    of the launch's 347 blocks is ragged).  du * mean_elems against the fp64 formula on the u the kernel read: the engine may
    deviate 4x as far as torch's own CPU f32 path (binary_cross_entropy_with_logits + autograd) does on the same inputs -- the
    same precision class with another exp and reciprocal; with bf16 activations du is stored as bf16: one rounding of 2^-8
    relative on top.  The loss: 1e-5 relative.  *loss_accum is added to; two runs are bitwise equal; du may alias u."""
    from ai_font_renderer_amd import _lib
    from .gpu_util import dev, ptr, stream
    rows, cols = 37, 19200
    me = rows * cols * 3
    u = torch.from_numpy(synth.hash_uniform(61, (rows, cols), 30.0))
    u[0, :] = torch.linspace(-104.0, 104.0, cols)
    u.view(-1)[cols:cols + 4] = torch.tensor([0.0, -0.0, 1e-8, -1e-8])
    tu8 = synth.hash_u8(62, (rows, cols))
    tf = torch.from_numpy(tu8.astype(np.float32) / 255.0)
    ud = dev(u, torch.float32 if act == "f32" else torch.bfloat16)
    uref = ud.float().cpu()                                             # the values the kernel reads
    loss64, du64 = bce_ref.bce_logits_loss_grad(uref.double(), tf.double(), total_elems=me)
    want = du64 * me                                                    # sigmoid(u) - t in fp64
    ua = uref.clone().requires_grad_(True)
    lt = F.binary_cross_entropy_with_logits(ua, tf)
    lt.backward()
    torch_dev = float((ua.grad.double() * ua.numel() - want).abs().max())
    torch_loss_dev = abs(float(lt.detach()) / 3.0 - float(loss64)) / float(loss64)       # (lt is the mean over n, loss64 over 3 n)
    td = dev(torch.from_numpy(tu8)) if tgt == "u8" else dev(tf)
    adt, tdt = (_lib.AFR_F32 if act == "f32" else _lib.AFR_BF16), (_lib.AFR_TARGET_U8 if tgt == "u8" else _lib.AFR_TARGET_F32)

    def run(accum, u_in, du_out):
        scratch = torch.zeros(1040, device="cuda")
        _lib.check(_lib.lib().afr_op_bce_grad(adt, ptr(u_in), ptr(td), tdt, ptr(du_out), rows, cols, me, ptr(accum), ptr(scratch), stream()))
        torch.cuda.synchronize()

    la, lb = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    dua, dub = torch.empty_like(ud), torch.full_like(ud, float("nan"))
    run(la, ud, dua)
    run(lb, ud, dub)
    assert torch.equal(dua, dub) and torch.equal(la, lb)                # bitwise reproducible
    got = dua.float().cpu().double() * me
    err = (got - want).abs()
    allow = 4.0 * torch_dev + (2.0 ** -8 * want.abs() if act == "bf16" else 0.0)
    eng_dev = float((err - (2.0 ** -8 * want.abs() if act == "bf16" else 0.0)).max())
    lrel = abs(float(la.item()) - float(loss64)) / float(loss64)
    print(f"bce op {act}/{tgt}: engine max |du*n - fp64| = {float(err.max()):.3e} ({eng_dev / 2.0 ** -24:.2f} x 2^-24 beyond the bf16 rounding), "
          f"torch f32 {torch_dev:.3e} ({torch_dev / 2.0 ** -24:.2f} x 2^-24); loss rel dev engine {lrel:.3e}, torch f32 {torch_loss_dev:.3e}")
    assert bool((err <= allow).all()), (float(err.max()), torch_dev)
    assert bool(torch.isfinite(dua.float()).all())
    assert lrel < 1e-5
    # added to, not overwritten: the same launch into an accumulator that already holds L gives exactly L + L
    run(la, ud, dub)
    assert float(la.item()) == 2.0 * float(lb.item())
    # du may alias u
    uu = ud.clone()
    run(lb, uu, uu)
    assert torch.equal(uu, dua)


# ----------------------------------------------------------------------------- sheet MINI against the reference-derived fixture
def _check_vs_fixture(fx, prefix, T, tol):
    """name -> numpy array against the fixture's full tensors, or its row sums, column sums and samples (test_gpu_pixel's rule:
    a sum is held to the size of what it adds up)."""
    for k, got in T.items():
        if prefix + k in fx.files:
            assert _rel(got, fx[prefix + k]) < tol, (prefix, k)
        else:
            g2 = got.reshape(got.shape[0], -1)
            for part, val, sc in (("rowsum", g2.sum(1), np.abs(g2).sum(1).max()), ("colsum", g2.sum(0), np.abs(g2).sum(0).max()),
                                  ("samples", got.reshape(-1)[fx[f"{prefix}{k}/idx"]], np.abs(got).max())):
                assert maxabs(val, fx[f"{prefix}{k}/{part}"]) <= tol * max(float(sc), 1e-12), (prefix, k, part)


@pytest.mark.parametrize("dtype", ["f32", "bf16x3"])
def test_sheet_mini_matches_the_reference_graph_with_bce(dtype):
    """Sigmoid bitmaps on the three length branches, loss + the 12 gradients without and with injected dropout, 3 AdamW steps."""
    fx, base = load("sheet_mini_bce.npz"), load("sheet_mini.npz")
    tu8 = torch.from_numpy(base["target_u8"])
    eng = _engine(MINI, dtype)
    for key in ("10", "6", "14"):
        y = eng.forward(torch.from_numpy(base["x" + key])).cpu().numpy()
        assert maxabs(y, fx["sheet/eval_y" + key]) < 2e-5, key
    assert eng.error_flags() == 0
    nodrop = replace(MINI, p_embed=0.0, p_attn=0.0, p_fc=0.0)
    eng = _engine(nodrop, dtype)
    for key, pre in (("x10", "nodrop"), ("x6", "nodrop6")):
        eng.train_step(torch.from_numpy(base[key]), tu8, do_step=False)
        ref = float(fx[f"sheet/{pre}_loss"])
        assert abs(eng.read_loss() - ref) <= 1e-5 * ref
        _check_vs_fixture(fx, f"sheet/{pre}_grad/", _grads(eng), 1e-4)
    eng = _engine(MINI, dtype, seed=42)
    eng.train_step(torch.from_numpy(base["x10"]), tu8, step=7, do_step=False)
    ref = float(fx["sheet/drop_loss"])
    assert abs(eng.read_loss() - ref) <= 1e-5 * ref
    _check_vs_fixture(fx, "sheet/drop_grad/", _grads(eng), 1e-4)
    y = eng.forward(torch.from_numpy(base["x10"]), training=True, step=7).cpu().numpy()
    assert maxabs(y, fx["sheet/drop_y"]) < 2e-5
    eng = _engine(nodrop, dtype)
    for i in range(3):
        eng.train_step(torch.from_numpy(base["x10"]), tu8)            # lr 1e-3, wd 5e-4, betas (0.9, 0.99): model.py:273
        ref = float(fx["sheet/adamw_losses"][i])
        assert abs(eng.read_loss() - ref) <= 1e-5 * ref, i
    E, bar = MINI.embed_dim, (2e-5 if dtype == "f32" else 1e-4)         # the bars of the MSE trajectories in these modes
    for k, v in eng.state_dict().items():
        got = v.cpu().numpy()
        if "sheet/adamw_param/" + k not in fx.files:                   # fc_output.weight: samples, and sums of n entries within n bars
            g2 = got.reshape(got.shape[0], -1)
            assert maxabs(got.reshape(-1)[fx[f"sheet/adamw_param/{k}/idx"]], fx[f"sheet/adamw_param/{k}/samples"]) < bar, k
            assert maxabs(g2.sum(1), fx[f"sheet/adamw_param/{k}/rowsum"]) < bar * g2.shape[1], k
            assert maxabs(g2.sum(0), fx[f"sheet/adamw_param/{k}/colsum"]) < bar * g2.shape[0], k
            continue
        ref = fx["sheet/adamw_param/" + k]
        if k == "attention.in_proj_bias":     # k-bias gradient is analytically 0: Adam amplifies rounding noise
            got, ref = np.delete(got, np.s_[E:2 * E]), np.delete(ref, np.s_[E:2 * E])
        assert maxabs(got, ref) < bar, k


# ----------------------------------------------------------------------------- fused epilogues == the loss kernel
def _fused_equals_unfused(cfg, dtype, B, x, font, target):
    """afr_forward_loss against afr_forward + afr_loss_grad: du (AFR_BUF_U) bit for bit, the loss to 2e-6 relative (its partial
    sums are cut differently), and du against the formula on the engine's own u; afr_train_step(do_step=0) then gives that loss
    and, bit for bit, the gradients afr_backward makes of that du."""
    eng = _engine(cfg, dtype=dtype, max_batch=B)
    eng.forward(x, font, training=True, step=3, want_output=False)
    u = eng.debug_read("u").view(B, -1).cpu()
    eng.loss_grad(target)
    du_unfused, l_unfused = eng.debug_read("u").view(B, -1).cpu(), eng.read_loss()
    eng.forward_loss(x, target, font=font, step=3)
    du_fused, l_fused = eng.debug_read("u").view(B, -1).cpu(), eng.read_loss()
    assert torch.equal(du_fused, du_unfused), (dtype, int((du_fused != du_unfused).sum()))
    assert abs(l_fused - l_unfused) <= 2e-6 * l_unfused
    eng.backward()
    g_fused = eng.flat_grads.clone()
    eng.train_step(x, target, font=font, step=3, do_step=False)      # the same fused forward + backward in one call
    assert abs(eng.read_loss() - l_unfused) <= 2e-6 * l_unfused
    assert torch.equal(eng.flat_grads, g_fused)
    tf = target.double() / 255.0 if target.dtype == torch.uint8 else target.double()
    lref, du_ref = bce_ref.bce_logits_loss_grad(u.double(), tf.view(B, -1))
    assert abs(l_fused - float(lref)) < 1e-5 * float(lref)
    tol = 1e-2 if dtype == "bf16" else 1e-6                            # du is stored as bf16 in bf16 mode
    assert float((du_fused.double() - du_ref).abs().max()) <= tol * float(du_ref.abs().max())
    assert eng.error_flags() == 0


@pytest.mark.parametrize("dtype", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("float_targets", [False, True])
def test_fused_bce_epilogue_equals_the_loss_kernel_on_a_c3_shaped_net(dtype, float_targets):
    """C3's layer shapes; bf16 at the benchmark batch (the 256x128 ring kernel with the early uint8 / late float32 target
    loads), f32 and bf16x3 at a ragged batch on the 128x128 tile epilogue."""
    from ai_font_renderer_amd.config import WORKLOADS
    cfg = WORKLOADS["c3"]["cfg"]
    B = 8192 if dtype == "bf16" else 1000
    x, font, tu8 = glyph_inputs(cfg, B)
    t = torch.from_numpy(tu8)
    _fused_equals_unfused(cfg, dtype, B, torch.from_numpy(x), torch.from_numpy(font), t.float() / 255.0 if float_targets else t)


@pytest.mark.parametrize("dtype", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("float_targets", [False, True])
def test_fused_bce_epilogue_equals_the_loss_kernel_on_the_sheet_model(dtype, float_targets):
    """A sheet model with dropout active, ragged batch (the narrow bf16 ring kernel / the tile epilogue)."""
    from .util import SheetConfig
    cfg = SheetConfig(max_length=24, sheet_h=16, sheet_w=40)
    B = 37
    x = torch.from_numpy(synth.encode_strings(synth.dataset_strings(B), 24))
    t = torch.from_numpy(synth.synth_sheet_targets(B, 16, 40, tensor_id=970))
    _fused_equals_unfused(cfg, dtype, B, x, None, t.float() / 255.0 if float_targets else t)


# ----------------------------------------------------------------------------- the fused small-net step
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("cfgkw,B", [
    (dict(hidden=(256,), out_h=16, out_w=16), 95),                          # C1 / C2's net: one ragged row block at the end
    (dict(hidden=(64,), out_h=8, out_w=8, n_fonts=2), 300),                 # smallest shapes the fused kernel takes, with fonts
    (dict(hidden=(192,), out_h=8, out_w=16, n_fonts=1, embed_dim=64), 130),  # wider embedding, widths that are not powers of 2
])
def test_fused_small_net_bce_step_equals_the_per_layer_kernels(cfgkw, B, dtype):
    """The BCE twin of test_fused_small_net_step_equals_the_per_layer_kernels: f32 (C1) against the per-layer kernels
    (AFR_CFG_NO_FUSED_GLYPH1), bf16 (C2) against the oracle rounded at the fused kernel's points."""
    cfg = GlyphConfig(**cfgkw)
    assert fused1_eligible(cfg)
    x, font, tu8 = glyph_inputs(cfg, B)
    xt, ft, tt = torch.from_numpy(x), torch.from_numpy(font) if cfg.n_fonts else None, torch.from_numpy(tu8)
    a = _engine(cfg, dtype=dtype, max_batch=B)
    a.train_step(xt, tt, font=ft, do_step=False)
    la = a.read_loss()
    if dtype == "f32":
        b = _engine(cfg, dtype=dtype, max_batch=B, flags=4)
        b.train_step(xt, tt, font=ft, do_step=False)
        lb = b.read_loss()
        assert abs(la - lb) <= 2e-6 * lb
        for k in a.grads:
            assert _rel(a.grads[k].cpu().numpy(), b.grads[k].cpu().numpy()) < 2e-5, k
        for _ in range(3):
            a.train_step(xt, tt, font=ft)
            b.train_step(xt, tt, font=ft)
        assert abs(a.read_loss() - b.read_loss()) < 1e-5 * 3
        for k in a.params:
            assert float((a.params[k] - b.params[k]).abs().max()) < 2e-5, k
    else:
        rnd = engine_rounding(cfg, dtype, train_step=True)
        P = tparams(cfg)
        _, cache = oracle.glyph_forward(P, xt, torch.from_numpy(font), cfg, rnd=rnd)
        lref, du = bce_ref.bce_logits_loss_grad(rnd(cache["u"]), torch.from_numpy(tu8.astype(np.float32) / 255.0))
        Gref = oracle.glyph_backward(P, cache, rnd_du(rnd, du), cfg, rnd=rnd)
        assert abs(la - float(lref)) < 3e-2 * float(lref)
        for k in a.grads:
            assert _rel(a.grads[k].cpu().numpy(), Gref[k].numpy()) < 3e-2, k
    assert a.error_flags() == 0
    a.train_step(xt, tt, font=ft, do_step=False)
    g1 = a.flat_grads.clone()
    a.train_step(xt, tt, font=ft, do_step=False)
    assert torch.equal(g1, a.flat_grads)                                   # run-to-run bitwise


def test_glyph_twin_fixture_with_bce_through_the_engine():
    """The torch.nn glyph twin with BCE-with-logits (two hidden layers with fonts; C1 through the fused step): sigmoid bitmaps,
    step-1 gradients, three AdamW steps -- held as test_golden_glyph_fixtures_through_the_engine holds the MSE twin."""
    from ai_font_renderer_amd.config import WORKLOADS
    fx = load("sheet_mini_bce.npz")
    for tag, cfg, B in (("small", GlyphConfig(hidden=(48, 40), out_h=4, out_w=6, n_fonts=2), 300), ("c1", WORKLOADS["c1"]["cfg"], 95)):
        x, font, tu8 = glyph_inputs(cfg, B)
        xt, ft, tt = torch.from_numpy(x), torch.from_numpy(font) if cfg.n_fonts else None, torch.from_numpy(tu8)
        eng = _engine(cfg, max_batch=B)
        assert maxabs(eng.forward(xt, ft).cpu().numpy(), fx[f"glyph/{tag}/eval_y"]) < 2e-5
        eng.train_step(xt, tt, font=ft, do_step=False)
        eng.read_loss()
        _check_vs_fixture(fx, f"glyph/{tag}/grad/", _grads(eng), 1e-4)
        for i in range(3):
            eng.train_step(xt, tt, font=ft)
            ref = float(fx[f"glyph/{tag}/losses"][i])
            assert abs(eng.read_loss() - ref) <= 1e-5 * ref, (tag, i)
        for k, v in eng.state_dict().items():
            got = v.cpu().numpy()
            if f"glyph/{tag}/param3/{k}" in fx.files:
                assert maxabs(got, fx[f"glyph/{tag}/param3/{k}"]) < 2e-5, (tag, k)
            else:
                assert maxabs(got.reshape(-1)[fx[f"glyph/{tag}/param3/{k}/idx"]], fx[f"glyph/{tag}/param3/{k}/samples"]) < 2e-5, (tag, k)
        assert eng.error_flags() == 0


# ----------------------------------------------------------------------------- by rows == dense on the gathered rows
def test_bce_by_rows_equals_gather_bitwise():
    """Sheet with dropout (f32 tile epilogue + loss kernel), C3 bf16 at the benchmark batch (ring epilogue, early uint8 targets
    through the row map), C1 through the fused small-net step: every call by rows against its dense twin, bitwise."""
    from ai_font_renderer_amd.config import WORKLOADS
    from .test_gpu_rows import _check_rows_equal_gather, _glyph_dataset, _rows_with_duplicates, _sheet_dataset
    _check_rows_equal_gather(MINI, "f32", _sheet_dataset(200, 10, 8, 24, 946), _rows_with_duplicates(200, 24, 1), 32, step=7, loss="bce")
    c3 = WORKLOADS["c3"]["cfg"]
    _check_rows_equal_gather(c3, "bf16", _glyph_dataset(c3, 380, 947), _rows_with_duplicates(380, 8192, 5), 8192, loss="bce")
    c1 = WORKLOADS["c1"]["cfg"]
    _check_rows_equal_gather(c1, "f32", _glyph_dataset(c1, 300, 948), _rows_with_duplicates(300, 95, 3), 95, loss="bce")


# ----------------------------------------------------------------------------- C3 at the benchmark batch, bf16
def test_c3_bench_batch_bf16_bce_step_vs_the_rounded_oracle():
    """BASELINE configs[2] as bench.py runs it, with the BCE loss: one afr_train_step (gradients materialised) against the oracle
    rounded at the engine's points, u and du in bf16.  The oracle takes the engine's ReLU masks (afr_debug_copy), which are
    verified separately; the sigmoid head has no discontinuity, so no pixel is excluded at the head."""
    from ai_font_renderer_amd.config import WORKLOADS
    cfg, B = WORKLOADS["c3"]["cfg"], WORKLOADS["c3"]["batch"]
    x, font, tu8 = glyph_inputs(cfg, B)
    xt, ft, tt = torch.from_numpy(x), torch.from_numpy(font), torch.from_numpy(tu8)
    eng = _engine(cfg, dtype="bf16", max_batch=B)
    rnd = engine_rounding(cfg, "bf16")
    eng.forward(xt, ft, want_output=False)
    u_eng = eng.debug_read("u").view(B, -1).cpu()
    rmasks = [eng.debug_read("act", i + 1).view(B, -1).cpu() > 0 for i in range(len(cfg.hidden))]
    P = tparams(cfg)
    _, own = oracle.glyph_forward(P, xt, ft, cfg, rnd=rnd)
    for i, m in enumerate(rmasks):                                       # masks differ only where the pre-activation is ~0
        bad = m != (own["pres"][i] > 0)
        assert bad.float().mean() < 1e-3 and (own["pres"][i][bad].abs() < 2e-2).all(), i
    _, cache = oracle.glyph_forward(P, xt, ft, cfg, rnd=rnd, relu_masks=rmasks)
    assert maxabs(u_eng.numpy(), cache["u"].numpy()) < 3e-2
    lref, du = bce_ref.bce_logits_loss_grad(rnd(cache["u"]), torch.from_numpy(tu8.astype(np.float32) / 255.0))
    Gref = oracle.glyph_backward(P, cache, rnd_du(rnd, du), cfg, rnd=rnd)
    eng.read_loss()
    eng.train_step(xt, tt, font=ft, do_step=False)
    assert abs(eng.read_loss() - float(lref)) < 3e-2 * float(lref)
    for k, g in eng.grads.items():
        assert _rel(g.cpu().numpy(), Gref[k].numpy()) < 3e-2, k
    y = eng.forward(xt[:64], ft[:64]).view(64, -1).cpu()
    assert maxabs(y.numpy(), bce_ref.sigmoid_stable(u_eng[:64]).numpy()) < 1e-6     # the eval output is sigmoid(stored u)
    assert eng.error_flags() == 0


# ----------------------------------------------------------------------------- the pixel transformer's head
def test_c5_mini_f32_bce_loss_and_every_gradient_vs_the_oracle():
    """AFR_KIND_PIXEL: sigmoid head output, loss and EVERY gradient against the fp64 oracle.pixel_backward fed the BCE du, at the
    bars of the f32 pixel test: bitmaps 2e-5, loss 1e-5 relative, every gradient within 1e-5 of the tensor's largest entry.
    The gradient is discontinuous where an MLP pre-activation is within rounding of zero, and -- unlike the clamp head, which
    gates most pixels' du to zero -- the sigmoid head sends a gradient through every token, so every such gate shows (f32
    against fp64 on the CPU oracle: 2 of this batch's 16.8 M gates differ, 9.2e-4 of the largest entry on
    positional_encoding; 9.4e-7 with the gates forced equal).  So, as for the large glyph shapes, the checker takes the
    ENGINE's gates (the sign of each block's stored ReLU output, afr_debug_copy) and verifies them separately: they may differ
    from the fp64 oracle's own only where its pre-activation is within 2e-5 of zero."""
    from ai_font_renderer_amd.config import C5_MINI as cfg
    fx = load("pixel_twin.npz")
    x, font, tgt = torch.from_numpy(fx["x"]), torch.from_numpy(fx["font"]), torch.from_numpy(fx["target_u8"])
    B = x.shape[0]
    eng = _engine(cfg, dtype="f32", max_batch=B)
    P64 = {k: v.double() for k, v in tparams(cfg).items()}
    _, c64 = oracle.pixel_forward(P64, x, font, cfg)
    y = eng.forward(x, font).cpu().numpy()
    assert maxabs(y.reshape(B, -1), bce_ref.sigmoid_stable(c64["u"]).reshape(B, -1).numpy()) < 2e-5
    eng.forward(x, font, training=True, want_output=False)
    flipped = 0
    for l in range(cfg.layers):
        gate = eng.debug_read("act", l).view(B, cfg.tokens, cfg.ff_dim).cpu() > 0
        pre = c64["saved"][l]["pre"]
        bad = gate != (pre > 0)
        assert bad.float().mean() < 1e-3 and (pre[bad].abs() < 2e-5).all(), l
        flipped += int(bad.sum())
        # the oracle's backward reads the gate as pre > 0 and the gated value as f: give it the engine's gates
        c64["saved"][l]["pre"] = torch.where(gate, pre.abs() + 1e-300, -pre.abs())
        c64["saved"][l]["f"] = torch.where(gate, pre.clamp(min=0.0), torch.zeros_like(pre))
    l64, du64 = bce_ref.bce_logits_loss_grad(c64["u"], tgt.double() / 255.0)
    G64 = oracle.pixel_backward(P64, c64, du64, cfg)
    eng.loss_grad(tgt)
    eng.backward()
    assert abs(eng.read_loss() - float(l64)) <= 1e-5 * float(l64)
    G = {n: eng.grads[n].cpu().numpy().copy() for n, _ in cfg.param_shapes()}
    worst = max((_rel(G[n], G64[n].numpy()), n) for n, _ in cfg.param_shapes())
    print(f"c5-mini bce: {flipped} engine gates differ from the fp64 oracle's; worst gradient {worst[1]} at {worst[0]:.2e} of its largest entry")
    for n, _ in cfg.param_shapes():
        assert _rel(G[n], G64[n].numpy()) <= 1e-5, n
    eng.train_step(x, tgt, font=font, do_step=False)                       # the one-call step: same kernels, same order
    assert abs(eng.read_loss() - float(l64)) <= 1e-5 * float(l64)
    for n, _ in cfg.param_shapes():
        assert np.array_equal(eng.grads[n].cpu().numpy(), G[n]), n
    assert eng.error_flags() == 0


# ----------------------------------------------------------------------------- caller-side loss on a sigmoid head
def test_set_output_grad_on_a_bce_model_equals_the_fused_bce_gradients(monkeypatch):
    """AttentionFontRenderer(loss="bce"): F.binary_cross_entropy(model(x), t) back-propagated by torch through
    afr_set_output_grad (du = dy * y * (1 - y)) equals the in-engine fused BCE gradients to 1e-4 relative on the MINI inputs
    (u in [-0.74, 0.82] there: no saturated pixel)."""
    from ai_font_renderer_amd import model as M
    from ai_font_renderer_amd.engine import Engine
    from .test_gpu_host import KEYS
    monkeypatch.setattr(M, "SHEET_HEIGHT", 8)
    monkeypatch.setattr(M, "SHEET_WIDTH", 24)
    base, fx = load("sheet_mini.npz"), load("sheet_mini_bce.npz")
    with pytest.raises(ValueError):
        M.AttentionFontRenderer(max_length=10, init=False, loss="focal")
    m = M.AttentionFontRenderer(max_length=10, init=False, loss="bce")
    assert m.loss == "bce" and m.engine.loss == "bce" and list(m.state_dict().keys()) == KEYS
    m.engine = Engine(replace(m.config, p_embed=0.0, p_attn=0.0, p_fc=0.0), dtype="f32", max_batch=8, device=M.device, loss="bce")
    m.engine.load_params(synth.make_params(MINI))
    P = {k: torch.nn.Parameter(v) for k, v in m.engine.params.items()}
    for name in KEYS:
        mod_, _, attr = name.rpartition(".")
        (m.get_submodule(mod_) if mod_ else m)._parameters[attr] = P[name]
    x, tu8 = torch.from_numpy(base["x10"]), torch.from_numpy(base["target_u8"])
    t = (tu8.float() / 255.0).to(M.device)
    m.eval()
    with torch.no_grad():
        assert maxabs(m(x).cpu().numpy(), fx["sheet/eval_y10"]) < 2e-5      # forward returns sigmoid(u)
    m.train()
    out = m(x)
    assert out.requires_grad
    loss = F.binary_cross_entropy(out, t.view(out.shape))
    loss.backward()
    assert abs(float(loss.detach()) - float(fx["sheet/nodrop_loss"])) <= 1e-5 * float(fx["sheet/nodrop_loss"])
    auto = {k: p.grad.detach().cpu().numpy().copy() for k, p in m.named_parameters()}
    m.engine.train_step(x, tu8, do_step=False)
    assert abs(m.engine.read_loss() - float(fx["sheet/nodrop_loss"])) <= 1e-5 * float(fx["sheet/nodrop_loss"])
    for k, g in _grads(m.engine).items():
        assert _rel(auto[k], g) < 1e-4, k
        assert _rel(auto[k], fx["sheet/nodrop_grad/" + k]) < 1e-4, k
    # a re-grown plan keeps the loss kind
    m.engine.ensure_batch(16)
    assert m.engine._c.loss == 1
    with torch.no_grad():
        m.eval()
        assert maxabs(m(x).cpu().numpy(), fx["sheet/eval_y10"]) < 2e-5


# ----------------------------------------------------------------------------- data parallel
@pytest.mark.parametrize("schedule", ["one-allreduce", "overlapped"])
def test_data_parallel_stepper_on_bce_engines_over_rccl_world1(schedule, monkeypatch):
    """DataParallelStepper is unchanged: world-1 RCCL through the multi-rank code path on a C3-shaped bf16 net and the sheet MINI
    model in f32 equals the single-GPU BCE step of the same arithmetic exactly (as test_data_parallel_stepper_over_rccl_world1
    holds the MSE step); and
    a shard that carries mean_elems of a four times larger global batch scales loss and gradients by exactly 1/4."""
    from ai_font_renderer_amd.config import WORKLOADS
    from ai_font_renderer_amd.parallel import DataParallelStepper
    with OP.rccl_world_one(schedule, monkeypatch) as dist:
        c3 = WORKLOADS["c3"]["cfg"]
        xg, fg, tg = glyph_inputs(c3, 1024)
        cases = [(c3, "bf16", 1024, torch.from_numpy(xg).cuda(), torch.from_numpy(fg).cuda(), torch.from_numpy(tg).cuda()),
                 (MINI, "f32", 24, torch.from_numpy(synth.encode_strings(synth.dataset_strings(24), 10)).cuda(), None,
                  torch.from_numpy(synth.synth_sheet_targets(24, 8, 24, tensor_id=971)).cuda())]
        for cfg, dtype, B, x, font, t in cases:
            me = B * cfg.pixels
            eng = _engine(cfg, dtype, B)
            st = DataParallelStepper(eng, dist, world=2)          # force the multi-rank code path
            for i in range(3):
                st.step(x, t, font, mean_elems=me, step=i + 1)
            l_dp, p_dp = st.global_loss(), eng.flat_params.clone()
            # The single-GPU step it must equal exactly is the one that does the same arithmetic: backward, then the stand-alone
            # AdamW kernel.  For the glyph net that is the default step.  The sheet model's default single-GPU step instead
            # applies AdamW to fc_output.weight inside its weight-gradient product -- whatever the loss kind -- which agrees with
            # the stand-alone kernel to the last bit only (test_fused_optimizer_step_equals_unfused_step), so the sheet model's
            # exact twin is the step with AFR_CFG_UNFUSED_OPTIMIZER, and the default step is held at that test's bars.
            sheet = cfg.kind == "sheet"
            eng2 = _engine(cfg, dtype, B, flags=1 if sheet else 0)
            st2 = DataParallelStepper(eng2, None, 1)
            for i in range(3):
                st2.step(x, t, font, mean_elems=me, step=i + 1)
            assert st2.global_loss() == l_dp, (cfg.kind, dtype)
            assert torch.equal(eng2.flat_params, p_dp), (cfg.kind, dtype)
            if sheet:
                eng3 = _engine(cfg, dtype, B)
                st3 = DataParallelStepper(eng3, None, 1)
                for i in range(3):
                    st3.step(x, t, font, mean_elems=me, step=i + 1)
                assert abs(st3.global_loss() - l_dp) <= 1e-6 * l_dp + 1e-7
                E = cfg.embed_dim
                for k in eng3.params:
                    d = (eng3.params[k] - eng.params[k]).abs()
                    if k == "attention.in_proj_bias":      # k-bias: analytically zero gradient, Adam amplifies rounding noise
                        d = torch.cat([d[:E], d[2 * E:]])
                    assert float(d.max()) <= 3e-6 * max(1.0, float(eng.params[k].abs().max())), k
            if dtype == "f32":      # (f32 gradients: a power-of-two scale is exact; bf16 du would round differently near its subnormals)
                a, b = _engine(cfg, dtype, B), _engine(cfg, dtype, B)
                a.train_step(x, t, font=font, step=5, mean_elems=me, do_step=False)
                b.train_step(x, t, font=font, step=5, mean_elems=4 * me, do_step=False)
                assert a.read_loss() == 4.0 * b.read_loss()
                assert torch.equal(a.flat_grads, 4.0 * b.flat_grads)


# ----------------------------------------------------------------------------- the training CLI and a real target
def test_train_string_renderer_end_to_end_with_bce(tmp_path, monkeypatch, capsys):
    """`AFR_LOSS=bce python model.py --train` in miniature (the form of test_train_string_renderer_end_to_end: 96 generated sheets,
    7 epochs): config.txt names the loss, every artefact of the default run is written, the validation BCE falls; render-only
    mode with the same selection loads the checkpoint and writes sigmoid bitmaps.  A default-loss run writes no `loss` line."""
    from PIL import Image
    from ai_font_renderer_amd import datagen, model as M
    from .test_gpu_host import KEYS
    monkeypatch.chdir(tmp_path)
    datagen.generate("train_input", 96)
    monkeypatch.setattr(M, "NUM_SAMPLES", 96)
    monkeypatch.setattr(M, "NUM_EPOCHS", 7)
    monkeypatch.setattr(M, "OUTPUT_DIR", "train_output_bce")
    monkeypatch.setattr(M, "COMPUTE_LOSS", "bce")                          # what AFR_LOSS=bce sets at import
    torch.manual_seed(42)
    M.main(["model.py", "--train"])
    out = tmp_path / "train_output_bce"
    cfg = (out / "config.txt").read_text().splitlines()
    assert cfg[0] == "# Training configuration" and "batch_size = 1024" in cfg and "data_size = 96" in cfg
    assert cfg[-1] == "loss = bce"
    res = dict(l.split(" = ") for l in (out / "training_results.txt").read_text().splitlines()[1:])
    assert res["final_epoch"] == "7" and res["early_stopped"] == "False" and res["training_duration_epochs"] == "7"
    for ep in (0, 5):
        assert sorted(os.listdir(out / f"epoch_{ep}")) == sorted(f"string_{i}.bmp" for i in range(15))
    assert (out / "string_14.bmp").exists() and (tmp_path / "font_renderer.pth").exists()
    sd = torch.load(tmp_path / "font_renderer.pth", weights_only=True)
    assert list(sd.keys()) == KEYS
    printed = capsys.readouterr().out
    val0 = float([l for l in printed.splitlines() if l.startswith("Epoch 0,")][0].split("Val Loss:")[1].split(",")[0])
    best = float(res["best_validation_loss"])
    assert np.isfinite(best) and best < val0, (best, val0)
    # render-only mode, same selection: the checkpoint through a sigmoid head
    monkeypatch.setattr(M, "OUTPUT_DIR", "render_only_bce")
    M.main(["model.py"])
    m = M.load_model(M.AttentionFontRenderer, M.MAX_CHARS_PER_SHEET, device=M.device)
    assert m.loss == "bce"
    x = torch.from_numpy(synth.encode_strings([M.test_strings[0]], M.MAX_CHARS_PER_SHEET))
    with torch.no_grad():
        y = m(x)[0].cpu().numpy()
    u = m.engine.debug_read("u").view(-1).cpu()                             # the logits of that forward
    assert maxabs(y.reshape(-1), bce_ref.sigmoid_stable(u).numpy()) < 1e-6 and 0.0 < y.min() and y.max() <= 1.0
    got = np.array(Image.open(tmp_path / "render_only_bce" / "string_0.bmp"))
    assert np.abs(got.astype(int) - oracle.sheet_to_u8(y).astype(int)).max() <= 1
    # a default-loss run: no `loss` line
    monkeypatch.setattr(M, "COMPUTE_LOSS", "mse")
    monkeypatch.setattr(M, "NUM_EPOCHS", 1)
    monkeypatch.setattr(M, "OUTPUT_DIR", "train_output_mse")
    M.main(["model.py", "--train"])
    cfg = (tmp_path / "train_output_mse" / "config.txt").read_text().splitlines()
    assert cfg[-1] == "sheet_width = 240" and not any(l.startswith("loss") for l in cfg)


def test_c1_trains_on_the_firacode_glyphs_with_bce():
    """BASELINE configs[0] on its real targets (FiraCode-Retina 16x16), 30 fused BCE steps: the loss falls, no error bit."""
    from ai_font_renderer_amd.config import WORKLOADS
    cfg = WORKLOADS["c1"]["cfg"]
    x = np.arange(32, 127, dtype=np.int64)
    t = synth.glyph_bitmap_targets(16, x)
    assert t is not None and t.shape == (95, 16, 16)
    eng = _engine(cfg, dtype="f32", max_batch=95)
    xt, tt = torch.from_numpy(x), torch.from_numpy(t)
    losses = []
    for _ in range(30):
        eng.train_step(xt, tt, lr=3e-3)
        losses.append(eng.read_loss())
    print("c1 on FiraCode with BCE:", losses[0], "->", losses[-1])
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert eng.error_flags() == 0
