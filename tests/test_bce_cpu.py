"""CPU: the BCE loss kind (AFR_LOSS_BCE, sigmoid head + binary cross-entropy on the logits).  The checker formula
(tests/bce_ref.py) against torch, the oracle + that formula against the reference-derived fixture
(tests/golden/sheet_mini_bce.npz, made by tests/golden/make_golden_bce.py), and the host side of the ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from . import bce_ref
from .util import MINI, ROOT, load, maxabs, oracle, synth, tmasks, tparams


def _t(a):
    return torch.from_numpy(np.asarray(a))


# ------------------------------------------------------------------------------------------ the formula
def _logits(n, dtype):
    g = torch.Generator().manual_seed(11)
    u = (torch.rand(n, 64, generator=g, dtype=torch.float64) * 60.0 - 30.0)
    u[0, :] = torch.linspace(-104.0, 104.0, 64, dtype=torch.float64)          # far tails: nothing may overflow
    u[1, :8] = torch.tensor([0.0, -0.0, 1e-8, -1e-8, 88.0, -88.0, 17.0, -17.0], dtype=torch.float64)
    t = torch.randint(0, 256, (n, 64), generator=g).to(torch.float64) / 255.0
    return u.to(dtype), t.to(dtype)


def test_bce_ref_equals_torch_bce_with_logits_and_autograd():
    u, t = _logits(300, torch.float64)
    ua = u.clone().requires_grad_(True)
    want = F.binary_cross_entropy_with_logits(ua, t)
    want.backward()
    loss, du = bce_ref.bce_logits_loss_grad(u, t)
    assert abs(float(loss) - float(want)) <= 1e-12 * abs(float(want))
    assert maxabs(du.numpy(), ua.grad.numpy()) <= 1e-12 * float(ua.grad.abs().max())
    assert maxabs(bce_ref.sigmoid_stable(u).numpy(), torch.sigmoid(u).numpy()) <= 1e-15
    # f32 on both sides: the project's f32 bars (loss 1e-5 relative, gradients 1e-4 relative)
    u32, t32 = u.float(), t.float()
    ua = u32.clone().requires_grad_(True)
    want = F.binary_cross_entropy_with_logits(ua, t32)
    want.backward()
    loss, du = bce_ref.bce_logits_loss_grad(u32, t32)
    assert abs(float(loss) - float(want)) <= 1e-5 * abs(float(want))
    assert maxabs(du.numpy(), ua.grad.numpy()) <= 1e-4 * float(ua.grad.abs().max())
    assert torch.isfinite(du).all() and np.isfinite(float(loss))


def test_bce_ref_total_elems_scales_loss_and_gradient_exactly():
    u, t = _logits(8, torch.float64)
    loss, du = bce_ref.bce_logits_loss_grad(u, t)
    loss4, du4 = bce_ref.bce_logits_loss_grad(u, t, total_elems=4 * u.numel())      # a power of two: exact in floating point
    assert float(loss4) * 4.0 == float(loss)
    assert torch.equal(du4 * 4.0, du)


# ------------------------------------------------------------------------------------------ oracle + formula vs the fixture
def _check_grads(fx, prefix, G, tol):
    """test_oracle_golden._check_grads, also for tensors the fixture stores as row sums, column sums and samples."""
    for k, g in G.items():
        got = g.numpy()
        if prefix + k in fx.files:
            ref = fx[prefix + k]
            scale = max(1e-6, float(np.abs(ref).max()))
            assert maxabs(got, ref) / scale < tol, (k, maxabs(got, ref), scale)
        else:
            g2 = got.reshape(got.shape[0], -1)
            for part, val in (("rowsum", g2.sum(1)), ("colsum", g2.sum(0)), ("samples", got.reshape(-1)[fx[f"{prefix}{k}/idx"]])):
                ref = fx[f"{prefix}{k}/{part}"]
                assert maxabs(val, ref) / max(1e-6, float(np.abs(ref).max())) < tol, (k, part)


def _check_param_summary(fx, prefix, k, got, bar=5e-6):
    """A parameter the fixture stores as sums and samples, held to what the per-entry bar of the full tensors (`bar`, absolute)
    implies: each sample within it, a sum of n entries within n times it."""
    g2 = got.reshape(got.shape[0], -1)
    assert maxabs(got.reshape(-1)[fx[f"{prefix}{k}/idx"]], fx[f"{prefix}{k}/samples"]) < bar, k
    assert maxabs(g2.sum(1), fx[f"{prefix}{k}/rowsum"]) < bar * g2.shape[1], k
    assert maxabs(g2.sum(0), fx[f"{prefix}{k}/colsum"]) < bar * g2.shape[0], k


def test_oracle_bce_matches_the_reference_graph_on_sheet_mini():
    """The reference's AttentionFontRenderer with BCE-with-logits on its hooked fc_output: sigmoid output on the three length
    branches, loss and the 12 gradients without and with injected dropout -- the bars of test_oracle_golden's MSE twins."""
    fx, base = load("sheet_mini_bce.npz"), load("sheet_mini.npz")
    P = tparams(MINI)
    tgt = _t(base["target_u8"].astype(np.float32) / 255.0)
    for key in ("10", "6", "14"):
        _, cache = oracle.sheet_forward(P, _t(base["x" + key]), MINI)
        y = bce_ref.sigmoid_stable(cache["u"]).reshape(-1, 8, 24)
        assert maxabs(y.numpy(), fx["sheet/eval_y" + key]) < 2e-6, key
    for key, pre in (("x10", "nodrop"), ("x6", "nodrop6")):
        _, cache = oracle.sheet_forward(P, _t(base[key]), MINI)
        loss, du = bce_ref.bce_logits_loss_grad(cache["u"], tgt)
        assert abs(float(loss) - float(fx[f"sheet/{pre}_loss"])) < 1e-6
        _check_grads(fx, f"sheet/{pre}_grad/", oracle.sheet_backward(P, cache, du, MINI), 2e-5)
    masks = tmasks(synth.sheet_dropout_masks(MINI, 5, 10, seed=42, step=7))
    _, cache = oracle.sheet_forward(P, _t(base["x10"]), MINI, masks)
    assert maxabs(bce_ref.sigmoid_stable(cache["u"]).reshape(-1, 8, 24).numpy(), fx["sheet/drop_y"]) < 2e-6
    loss, du = bce_ref.bce_logits_loss_grad(cache["u"], tgt)
    assert abs(float(loss) - float(fx["sheet/drop_loss"])) < 1e-6
    _check_grads(fx, "sheet/drop_grad/", oracle.sheet_backward(P, cache, du, MINI), 2e-5)


def test_oracle_bce_three_adamw_steps_on_sheet_mini():
    fx, base = load("sheet_mini_bce.npz"), load("sheet_mini.npz")
    P = tparams(MINI)
    M = {k: torch.zeros_like(v) for k, v in P.items()}
    V = {k: torch.zeros_like(v) for k, v in P.items()}
    tgt = _t(base["target_u8"].astype(np.float32) / 255.0)
    x = _t(base["x10"])
    for t in (1, 2, 3):
        loss, _, P, M, V = bce_ref.train_step(P, M, V, t, x, tgt, MINI)
        assert abs(float(loss) - float(fx["sheet/adamw_losses"][t - 1])) < 2e-6
    E = MINI.embed_dim
    for k in P:
        got = P[k].numpy()
        if "sheet/adamw_param/" + k not in fx.files:                   # fc_output.weight: sums and samples
            _check_param_summary(fx, "sheet/adamw_param/", k, got)
            continue
        ref = fx["sheet/adamw_param/" + k]
        if k == "attention.in_proj_bias":      # the k-bias gradient is analytically 0: Adam turns rounding noise into +-lr steps
            assert maxabs(got[E:2 * E], ref[E:2 * E]) < 3 * 1e-3 * 1.01
            got, ref = np.delete(got, np.s_[E:2 * E]), np.delete(ref, np.s_[E:2 * E])
        assert maxabs(got, ref) < 5e-6, k


def test_oracle_bce_matches_the_torch_nn_glyph_twin():
    from .test_oracle_golden import _twin_case
    fx = load("sheet_mini_bce.npz")
    for tag in ("small", "c1"):
        cfg, x, font, tgt = _twin_case(tag)
        P = tparams(cfg)
        _, cache = oracle.glyph_forward(P, x, font, cfg)
        y = bce_ref.sigmoid_stable(cache["u"]).reshape(-1, cfg.out_h, cfg.out_w)
        assert maxabs(y.numpy(), fx[f"glyph/{tag}/eval_y"]) < 2e-6, tag
        loss, du = bce_ref.bce_logits_loss_grad(cache["u"], tgt)
        assert abs(float(loss) - float(fx[f"glyph/{tag}/losses"][0])) < 1e-6
        _check_grads(fx, f"glyph/{tag}/grad/", oracle.glyph_backward(P, cache, du, cfg), 2e-5)
        M = {k: torch.zeros_like(v) for k, v in P.items()}
        V = {k: torch.zeros_like(v) for k, v in P.items()}
        for t in (1, 2, 3):
            loss, _, P, M, V = bce_ref.train_step(P, M, V, t, x, tgt, cfg, font=font)
            assert abs(float(loss) - float(fx[f"glyph/{tag}/losses"][t - 1])) < 2e-6, (tag, t)
        for k in P:
            if f"glyph/{tag}/param3/{k}" in fx.files:
                assert maxabs(P[k].numpy(), fx[f"glyph/{tag}/param3/{k}"]) < 5e-6, (tag, k)
            else:
                _check_param_summary(fx, f"glyph/{tag}/param3/", k, P[k].numpy())


# ------------------------------------------------------------------------------------------ the ABI, host side only
def test_config_carries_the_loss_kind_and_plan_create_validates_it():
    from ai_font_renderer_amd import _lib, config
    from ai_font_renderer_amd.engine import make_afr_config
    lib = _lib.lib()
    cfg = config.SheetConfig(max_length=10, sheet_h=8, sheet_w=24)
    assert make_afr_config(cfg, "f32", 8).loss == _lib.AFR_LOSS_MSE == 0
    assert make_afr_config(cfg, "f32", 8, loss="mse").loss == 0
    c = make_afr_config(cfg, "f32", 8, loss="bce")
    assert c.loss == _lib.AFR_LOSS_BCE == 1
    with pytest.raises(ValueError):
        make_afr_config(cfg, "f32", 8, loss="focal")
    # `loss` is the last field of the struct, after `reserved`, and grew it by 8 bytes (4 + tail padding)
    assert _lib.AfrConfig._fields_[-1][0] == "loss" and _lib.AfrConfig._fields_[-2][0] == "reserved"
    assert _lib.AfrConfig.loss.offset == _lib.AfrConfig.reserved.offset + 4 and C.sizeof(_lib.AfrConfig) == 120
    plan = C.c_void_p()
    for kind in (0, 1):
        c.loss = kind
        assert lib.afr_plan_create(C.byref(c), C.byref(plan)) == 0
        lib.afr_plan_destroy(plan)
    c.loss = 2
    assert lib.afr_plan_create(C.byref(c), C.byref(plan)) == -1           # AFR_EINVAL
    assert b"loss" in lib.afr_last_error()
    assert lib.afr_version() == 1


def test_bce_plan_has_the_layout_and_workspace_of_the_mse_plan():
    """The loss adds no buffer and no parameter."""
    from ai_font_renderer_amd import _lib, config
    from ai_font_renderer_amd.engine import make_afr_config
    lib = _lib.lib()
    for cfg, dt in ((config.SheetConfig(max_length=10, sheet_h=8, sheet_w=24), "f32"), (config.WORKLOADS["c1"]["cfg"], "bf16"),
                    (config.WORKLOADS["c3"]["cfg"], "bf16"), (config.WORKLOADS["c3"]["cfg"], "bf16x3"), (config.C5_MINI, "f32")):
        seen = []
        for loss in ("mse", "bce"):
            c = make_afr_config(cfg, dt, 64, loss=loss)
            plan = C.c_void_p()
            _lib.check(lib.afr_plan_create(C.byref(c), C.byref(plan)))
            name = C.create_string_buffer(128)
            off, numel, ndim = C.c_int64(), C.c_int64(), C.c_int32()
            shape = (C.c_int64 * 4)()
            table = []
            for i in range(lib.afr_param_count(plan)):
                _lib.check(lib.afr_param_info(plan, i, name, 128, C.byref(off), C.byref(numel), C.byref(ndim), shape))
                table.append((name.value, off.value, numel.value, tuple(shape[k] for k in range(ndim.value))))
            seen.append((lib.afr_param_elems(plan), lib.afr_workspace_bytes(plan), table))
            lib.afr_plan_destroy(plan)
        assert seen[0] == seen[1], (cfg, dt)


def test_op_bce_grad_is_declared_exported_and_bound():
    from ai_font_renderer_amd import _lib
    src = open(os.path.join(ROOT, "include", "afr.h")).read()
    assert re.search(r"\bint\s+afr_op_bce_grad\s*\(", src)
    assert re.search(r"AFR_LOSS_MSE\s*=\s*0", src) and re.search(r"AFR_LOSS_BCE\s*=\s*1", src)
    assert hasattr(C.CDLL(_lib.LIB_PATH), "afr_op_bce_grad")
    assert _lib.SIGNATURES["afr_op_bce_grad"] == _lib.SIGNATURES["afr_op_mse_grad"]
    # argument validation only: nothing is launched
    assert _lib.lib().afr_op_bce_grad(_lib.AFR_F32, None, None, 0, None, 8, 8, 64, None, None, None) == -1
