"""GPU: the bf16x3 mode (AFR_BF16X3).  f32 activations and kernels everywhere except the Linear products, which run as
three bf16 MFMAs on operands split x = hi + lo at staging (csrc/gemm.hip gemm_bf16x3).  Held to the north star's 1e-4
bars -- bitmaps max-abs, gradients relative -- against the reference's own goldens and the unrounded f32 oracle, and at
op level to the split's error bound against fp64."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest
import torch

from ai_font_renderer_amd import _lib
from .gpu_util import dev, gemm, ptr, stream
from .util import MINI, R0, glyph_inputs, load, maxabs, oracle, rand, synth, tparams

pytestmark = pytest.mark.gpu


def _engine(cfg, dtype="bf16x3", max_batch=64, **kw):
    from ai_font_renderer_amd.engine import Engine
    eng = Engine(cfg, dtype=dtype, max_batch=max_batch, **kw)
    eng.load_params(synth.make_params(cfg))
    return eng


def _rel(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return maxabs(got, ref) / max(1e-7, float(np.abs(ref).max()))


def _grads(eng):
    return {k: v.detach().cpu().numpy() for k, v in eng.grads.items()}


def _gemm_x3(A_log, B_log, a_kstrided=False, b_kstrided=False, bias=None, relu=False, aux=None, splitk=1):
    """afr_op_gemm with dtype AFR_BF16X3 (gpu_util.gemm maps every non-f32 dtype to bf16): f32 operands, f32 C."""
    lib = _lib.lib()
    M, K = A_log.shape
    N = B_log.shape[0]
    A = dev(A_log.t().contiguous() if a_kstrided else A_log, torch.float32)
    B = dev(B_log.t().contiguous() if b_kstrided else B_log, torch.float32)
    flags = (_lib.GEMM_A_KSTRIDED if a_kstrided else 0) | (_lib.GEMM_B_KSTRIDED if b_kstrided else 0)
    bias_d = aux_d = None
    if bias is not None:
        flags |= _lib.GEMM_BIAS
        bias_d = dev(bias, torch.float32)
    if relu:
        flags |= _lib.GEMM_RELU
    if aux is not None:
        flags |= _lib.GEMM_RELU_MASK
        aux_d = dev(aux, torch.float32)
    Cd = torch.full((splitk, M, N), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(lib.afr_op_gemm(_lib.AFR_BF16X3, flags, ptr(A), ptr(B), ptr(Cd), ptr(bias_d), ptr(aux_d), M, N, K,
                               M if a_kstrided else K, N if b_kstrided else K, N, N, splitk, stream()))
    if splitk > 1:
        out = torch.empty(M, N, dtype=torch.float32, device="cuda")
        _lib.check(lib.afr_op_reduce(ptr(out), ptr(Cd), splitk, M * N, M * N, 1.0, 0, stream()))
        torch.cuda.synchronize()
        return out.cpu()
    torch.cuda.synchronize()
    return Cd[0].cpu()


def _bound(A, B, K, C64, bias=None):
    """|C - C64| <= (3 2^-16 + K 2^-24) sum_k |a_k b_k| per element (+ one f32 rounding of the bias add)."""
    s = A.double().abs() @ B.double().abs().t()
    b = (3 * 2.0 ** -16 + K * 2.0 ** -24) * s
    if bias is not None:
        b = b + 2.0 ** -24 * (C64.abs() + bias.double().abs())
    return b


# ----------------------------------------------------------------------------- op level
@pytest.mark.parametrize("ak,bk", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_op_gemm_all_orientations_ragged_vs_fp64(ak, bk):
    M, N, K = 200, 136, 264                                   # no extent a tile multiple (128 x 128 x 32)
    A, B = rand(701, (M, K)), rand(702, (N, K))
    C64 = A.double() @ B.double().t()
    got = _gemm_x3(A, B, bool(ak), bool(bk))
    err = (got.double() - C64).abs()
    assert bool((err <= _bound(A, B, K, C64)).all()), float((err / _bound(A, B, K, C64)).max())
    e16 = float((gemm("bf16", A, B, bool(ak), bool(bk)).double() - C64).abs().max())
    print(f"bf16x3 <{ak},{bk}> max err {float(err.max()):.3e}, bf16 {e16:.3e} (ratio 1/{e16 / max(float(err.max()), 1e-30):.0f})")
    assert float(err.max()) <= e16 / 64                       # not plain bf16


def test_op_gemm_epilogues_and_splitk_vs_fp64():
    M, N, K = 160, 200, 200
    A, B = rand(711, (M, K)), rand(712, (N, K))
    bias, aux = rand(713, (N,)), rand(714, (M, N))
    C64 = A.double() @ B.double().t()
    b = _bound(A, B, K, C64, bias)
    pre = C64 + bias.double()
    got = _gemm_x3(A, B, bias=bias, relu=True)
    assert bool(((got.double() - pre.clamp(min=0)).abs() <= b).all())
    got = _gemm_x3(A, B, bias=bias, aux=aux)                  # ReLU mask read from an f32 activation
    assert bool(((got.double() - pre * (aux > 0).double()).abs() <= b).all())
    # split-K partial slabs, at the depth of R0's fc_output products (K = 6400), k-strided operands as in a weight gradient
    M, N, K = 136, 264, 6400
    A, B = rand(715, (M, K)), rand(716, (N, K))
    C64 = A.double() @ B.double().t()
    for sk, (ak, bk) in ((1, (0, 0)), (4, (1, 1)), (5, (0, 1))):
        got = _gemm_x3(A, B, ak, bk, splitk=sk)
        err = (got.double() - C64).abs()
        assert bool((err <= _bound(A, B, K, C64)).all()), (sk, float((err / _bound(A, B, K, C64)).max()))


# ----------------------------------------------------------------------------- sheet model vs reference goldens
def test_mini_eval_matches_reference_all_length_branches():
    fx = load("sheet_mini.npz")
    eng = _engine(MINI)
    for key in ("10", "6", "14"):
        d = maxabs(eng.forward(torch.from_numpy(fx["x" + key])).cpu().numpy(), fx["eval_y" + key])
        print(f"mini eval x{key}: bf16x3 max-abs {d:.3e}")
        assert d < 1e-4, key
    assert eng.error_flags() == 0


def test_mini_train_grads_without_and_with_dropout_and_three_adamw_steps():
    fx = load("sheet_mini.npz")
    nodrop = replace(MINI, p_embed=0.0, p_attn=0.0, p_fc=0.0)
    eng = _engine(nodrop)
    for key, pre in (("x10", "nodrop"), ("x6", "nodrop6")):
        eng.train_step(torch.from_numpy(fx[key]), torch.from_numpy(fx["target_u8"]), do_step=False)
        ref = float(fx[pre + "_loss"])
        assert abs(eng.read_loss() - ref) <= 1e-5 * ref
        for k, g in _grads(eng).items():
            assert _rel(g, fx[pre + "_grad/" + k]) < 1e-4, (pre, k)
    eng = _engine(MINI, seed=42)
    eng.train_step(torch.from_numpy(fx["x10"]), torch.from_numpy(fx["target_u8"]), step=7, do_step=False)
    assert abs(eng.read_loss() - float(fx["drop_loss"])) <= 1e-5 * float(fx["drop_loss"])
    for k, g in _grads(eng).items():
        assert _rel(g, fx["drop_grad/" + k]) < 1e-4, k
    eng = _engine(nodrop)
    x, t = torch.from_numpy(fx["x10"]), torch.from_numpy(fx["target_u8"])
    for i in range(3):
        eng.train_step(x, t)
        ref = float(fx["adamw_losses"][i])
        assert abs(eng.read_loss() - ref) <= 1e-5 * ref, i
    E = MINI.embed_dim
    for k, v in eng.state_dict().items():
        got, ref = v.cpu().numpy(), fx["adamw_param/" + k]
        if k == "attention.in_proj_bias":     # k-bias gradient is analytically 0: Adam amplifies rounding noise
            got, ref = np.delete(got, np.s_[E:2 * E]), np.delete(ref, np.s_[E:2 * E])
        assert maxabs(got, ref) < 1e-4, k


def test_r0_test_strings_and_train_step_grads():
    fx = load("sheet_r0.npz")
    eng = _engine(R0, max_batch=16, with_optimizer=False)
    y = eng.forward(torch.from_numpy(fx["test_x"])).cpu().numpy()
    d = maxabs(y, fx["test_eval_y"])
    print(f"R0 test_strings: bf16x3 max-abs bitmap diff {d:.3e}")
    assert d < 1e-4
    a, b = oracle.sheet_to_u8(y), oracle.sheet_to_u8(fx["test_eval_y"])
    assert np.abs(a.astype(int) - b.astype(int)).max() <= 1
    assert (a != b).mean() < 1e-3
    eng = _engine(replace(R0, p_embed=0.0, p_attn=0.0, p_fc=0.0), max_batch=8, with_optimizer=False)
    tu8 = synth.synth_sheet_targets(8, 80, 240, tensor_id=902)
    eng.forward(torch.from_numpy(fx["train_x"]), training=True, want_output=False)
    eng.loss_grad(torch.from_numpy(tu8))
    eng.backward()
    assert abs(eng.read_loss() - float(fx["train_loss"])) <= 1e-5 * float(fx["train_loss"])
    G = _grads(eng)
    gw = G.pop("fc_output.weight")
    for k, g in G.items():
        assert _rel(g, fx["train_grad/" + k]) < 1e-4, k
    assert _rel(gw.sum(1), fx["train_gradW_rowsum"]) < 1e-4
    assert _rel(gw.sum(0), fx["train_gradW_colsum"]) < 1e-4
    assert _rel(gw.reshape(-1)[fx["train_gradW_idx"]], fx["train_gradW_samples"]) < 1e-4


# ----------------------------------------------------------------------------- C3 at the benchmarked batch
def test_c3_bench_batch_grads_vs_unrounded_oracle_and_trained_bitmaps():
    from ai_font_renderer_amd.config import WORKLOADS
    cfg, B = WORKLOADS["c3"]["cfg"], WORKLOADS["c3"]["batch"]
    x, font, tu8 = glyph_inputs(cfg, B)
    xt, ft, tt = torch.from_numpy(x), torch.from_numpy(font), torch.from_numpy(tu8)
    eng = _engine(cfg, max_batch=B)
    # the oracle on the ENGINE's ReLU / clamp masks (gradients are discontinuous where a pre-activation sits within rounding
    # of a threshold); those masks may differ from the oracle's own only there
    eng.forward(xt, ft, want_output=False)
    u_eng = eng.debug_read("u").view(B, -1).cpu()
    rmasks = [eng.debug_read("act", i + 1).view(B, -1).cpu() > 0 for i in range(len(cfg.hidden))]
    cmask = (u_eng >= 0) & (u_eng <= 1)
    P = tparams(cfg)
    _, own = oracle.glyph_forward(P, xt, ft, cfg)
    for i, m in enumerate(rmasks):
        bad = m != (own["pres"][i] > 0)
        assert bad.float().mean() < 1e-3 and (own["pres"][i][bad].abs() < 1e-4).all(), i
    _, cache = oracle.glyph_forward(P, xt, ft, cfg, relu_masks=rmasks)
    du_ = maxabs(u_eng.numpy(), cache["u"].numpy())
    print(f"C3 forward u: bf16x3 max-abs {du_:.3e}")
    assert du_ < 1e-4
    lref, du = oracle.mse_loss_grad(cache["u"], torch.from_numpy(tu8.astype(np.float32) / 255.0), clamp_mask=cmask)
    Gref = oracle.glyph_backward(P, cache, du, cfg)
    eng.read_loss()
    eng.train_step(xt, tt, font=ft, do_step=False)           # fused loss epilogue, split-K dW + fused db, grouped reduce
    assert abs(eng.read_loss() - float(lref)) <= 1e-5 * float(lref)
    worst = 0.0
    for k, g in eng.grads.items():
        r = _rel(g.cpu().numpy(), Gref[k].numpy())
        worst = max(worst, r)
        assert r < 1e-4, k
    print(f"C3 gradients: bf16x3 worst relative error {worst:.3e}")
    for _ in range(30):                                       # the bench's step: AdamW inside the grouped reduce
        eng.train_step(xt, tt, font=ft)
    eng.read_loss()
    y = eng.forward(xt[:190], ft[:190]).cpu()
    Pe = {k: v.cpu() for k, v in eng.state_dict().items()}
    yref, _ = oracle.glyph_forward(Pe, xt[:190], ft[:190], cfg)
    d = float((y - yref).abs().max())
    print(f"C3 trained 30 steps, 190 glyphs: bf16x3 max-abs bitmap diff {d:.3e}")
    assert d < 1e-4


# ----------------------------------------------------------------------------- C5
def test_c5_mini_forward_and_grads_vs_the_torch_nn_twin():
    from ai_font_renderer_amd.config import C5_MINI as cfg
    from .test_gpu_pixel import _check_against_twin
    fx = load("pixel_twin.npz")
    x, font, tgt = torch.from_numpy(fx["x"]), torch.from_numpy(fx["font"]), torch.from_numpy(fx["target_u8"])
    eng = _engine(cfg, max_batch=32)
    d = maxabs(eng.forward(x, font).cpu().numpy(), fx["eval_y"])
    print(f"C5-mini forward: bf16x3 max-abs {d:.3e}")
    assert d < 1e-4
    eng.forward(x, font, training=True, want_output=False)
    eng.loss_grad(tgt)
    eng.backward()
    assert abs(eng.read_loss() - float(fx["losses"][0])) <= 1e-5 * float(fx["losses"][0])
    G = {n: eng.grads[n].cpu().numpy().copy() for n, _ in cfg.param_shapes()}
    assert _check_against_twin(fx, cfg, "grad/", G, 4e-3) == len(cfg.param_shapes())      # the f32-mode twin test's bound
    P64 = {k: v.double() for k, v in tparams(cfg).items()}
    _, c64 = oracle.pixel_forward(P64, x, font, cfg)
    _, du64 = oracle.mse_loss_grad(c64["u"], tgt.double() / 255.0)
    G64 = oracle.pixel_backward(P64, c64, du64, cfg)
    # against the fp64 oracle the f32 mode sits at 1.6e-6; bf16x3 measured 3.3e-3 of the largest entry, the size of the f32
    # twin's own distance to fp64 (2.3e-3: ReLU gates within rounding of zero flip), so it is held to the twin's 4e-3
    worst = max(_rel(G[n], G64[n].numpy()) for n, _ in cfg.param_shapes())
    print(f"C5-mini gradients vs fp64: bf16x3 worst relative error {worst:.3e}")
    assert worst < 4e-3
    assert eng.error_flags() == 0


# ----------------------------------------------------------------------------- the mode is engaged
def _profiled_kernels(eng, step):
    eng.profile(1)
    step()
    torch.cuda.synchronize()
    rows = eng.profile_table()
    eng.profile(0)
    return [r["kernel"] for r in rows]


def test_steps_run_bf16x3_products_and_no_f32_ones():
    from ai_font_renderer_amd.config import WORKLOADS
    cfg = WORKLOADS["c3"]["cfg"]
    x, font, tu8 = glyph_inputs(cfg, 1024)
    eng = _engine(cfg, max_batch=1024)
    ks = _profiled_kernels(eng, lambda: eng.train_step(torch.from_numpy(x), torch.from_numpy(tu8), font=torch.from_numpy(font)))
    assert any(k.startswith("gemm_bf16x3<") for k in ks) and not any("gemm_f32<" in k for k in ks), ks
    fx = load("sheet_r0.npz")
    eng = _engine(R0, max_batch=8)
    tu8 = synth.synth_sheet_targets(8, 80, 240, tensor_id=902)
    ks = _profiled_kernels(eng, lambda: eng.train_step(torch.from_numpy(fx["train_x"]), torch.from_numpy(tu8)))
    assert any(k.startswith("gemm_bf16x3<") for k in ks) and not any("gemm_f32<" in k for k in ks), ks


def test_c1_keeps_the_fused_f32_kernel_bitwise():
    from ai_font_renderer_amd.config import WORKLOADS
    cfg, B = WORKLOADS["c1"]["cfg"], WORKLOADS["c1"]["batch"]
    x, font, tu8 = glyph_inputs(cfg, B)
    out = {}
    for dt in ("f32", "bf16x3"):
        eng = _engine(cfg, dtype=dt, max_batch=B)
        eng.train_step(torch.from_numpy(x), torch.from_numpy(tu8), do_step=False)
        out[dt] = (eng.read_loss(), eng.flat_grads.clone())
    assert out["f32"][0] == out["bf16x3"][0]
    assert torch.equal(out["f32"][1], out["bf16x3"][1])


def test_steps_are_bitwise_reproducible():
    from ai_font_renderer_amd.config import WORKLOADS
    fx = load("sheet_r0.npz")
    tu8 = synth.synth_sheet_targets(8, 80, 240, tensor_id=902)
    cfg = WORKLOADS["c3"]["cfg"]
    gx, gf, gt = glyph_inputs(cfg, 2048)
    for eng, step in ((_engine(R0, max_batch=8), lambda e: e.train_step(torch.from_numpy(fx["train_x"]), torch.from_numpy(tu8), step=3, do_step=False)),
                      (_engine(cfg, max_batch=2048), lambda e: e.train_step(torch.from_numpy(gx), torch.from_numpy(gt), font=torch.from_numpy(gf), do_step=False))):
        outs = []
        for _ in range(2):
            step(eng)
            outs.append((eng.read_loss(), eng.flat_grads.clone()))
        assert outs[0][0] == outs[1][0]
        assert torch.equal(outs[0][1], outs[1][1])


def test_facade_draws_r0_test_strings():
    from ai_font_renderer_amd import model as M
    fx = load("sheet_r0.npz")
    m = M.AttentionFontRenderer(dtype="bf16x3", max_batch=16, init=False)
    assert m.engine.dtype == "bf16x3"
    m.engine.load_params(synth.make_params(m.config))
    m.eval()
    with torch.no_grad():
        y = m(torch.from_numpy(fx["test_x"]))
    assert maxabs(y.cpu().numpy(), fx["test_eval_y"]) < 1e-4
