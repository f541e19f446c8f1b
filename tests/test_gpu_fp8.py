"""GPU: the fp8 (OCP e4m3fn) building blocks of BASELINE configs[4] through the C ABI -- afr_op_f32_to_fp8 against torch's
float8_e4m3fn cast (round to nearest even, saturating) and afr_op_gemm_fp8 (v_mfma_scale_f32_16x16x128_f8f6f4, unit block
scales, per-tensor scale in the epilogue) against fp64 on the e4m3-rounded operands.  The reference has no fp8 path (SURVEY
8 f5): parity here is pinned to the OCP format definition (torch's CPU cast) and to exact arithmetic, not to the reference."""
import ctypes as C

import numpy as np
import pytest
import torch

from ai_font_renderer_amd import _lib
from .gpu_util import dev, ptr, stream
from .util import rand

pytestmark = pytest.mark.gpu


def _to_fp8(x, scale):
    """float32 CPU tensor -> (uint8 device tensor of e4m3 bytes via the library, the values those bytes stand for)."""
    lib = _lib.lib()
    src = dev(x, torch.float32)
    dst = torch.empty(x.shape, dtype=torch.uint8, device="cuda")
    _lib.check(lib.afr_op_f32_to_fp8(ptr(src), ptr(dst), x.numel(), float(scale), stream()))
    torch.cuda.synchronize()
    vals = dst.cpu().view(torch.float8_e4m3fn).to(torch.float32) * scale
    return dst, vals


def test_f32_to_fp8_is_the_ocp_e4m3_cast():
    x = torch.cat([rand(301, (4099,), 600.0), rand(302, (2048,), 2.0), rand(303, (2048,), 0.02),
                   torch.tensor([0.0, -0.0, 448.0, -448.0, 449.0, 1e6, -1e6, 2.0 ** -9, 2.0 ** -10, 0.0009765625 * 1.5, 17.0, 18.0, 19.0, 20.0])])
    for scale in (1.0, 0.37):
        got, _ = _to_fp8(x, scale)
        want = (x / scale).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
        g = got.cpu()
        same = g == want
        # (+0 / -0 of values that underflow may differ in sign bit only)
        assert bool((same | ((g & 0x7F) == 0) & ((want & 0x7F) == 0)).all()), (x[~same][:8], g[~same][:8], want[~same][:8])


@pytest.mark.parametrize("M,N,K", [(8192, 1024, 1024), (4000, 2040, 528), (256, 128, 128), (300, 72, 4096)])
def test_fp8_gemm_vs_fp64(M, N, K):
    lib = _lib.lib()
    sa, sb = 0.011, 0.0042
    A8, Av = _to_fp8(rand(311, (M, K), 3.0), sa)
    B8, Bv = _to_fp8(rand(312, (N, K), 1.5), sb)
    bias = rand(313, (N,))
    ref = Av.double() @ Bv.double().t()
    scale = float(ref.abs().max())
    for flags, post in ((0, lambda r: r), (_lib.GEMM_BIAS | _lib.GEMM_RELU, lambda r: torch.relu(r + bias.double()))):
        Cd = torch.full((M, N), float("nan"), dtype=torch.float32, device="cuda")
        _lib.check(lib.afr_op_gemm_fp8(flags, ptr(A8), ptr(B8), ptr(Cd), ptr(dev(bias)) if flags else C.c_void_p(0), M, N, K, K, K, N,
                                       sa * sb, stream()))
        torch.cuda.synchronize()
        # (the products of two e4m3 numbers are exact in f32; the 128-deep scaled MFMA sums them with somewhat less than a full
        # f32 fma chain's accuracy: measured 2e-5 of the largest output at K = 1024, against 1e-5 held by the bf16 kernels)
        err = float((Cd.cpu().double() - post(ref)).abs().max()) / scale
        print(f"fp8 gemm {M}x{N}x{K} flags {flags}: max err / max|C| = {err:.2e}")
        assert err < 5e-5, (M, N, K, flags)
    Cb = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device="cuda")
    _lib.check(lib.afr_op_gemm_fp8(_lib.GEMM_OUT_BF16, ptr(A8), ptr(B8), ptr(Cb), C.c_void_p(0), M, N, K, K, K, N, sa * sb, stream()))
    torch.cuda.synchronize()
    assert float((Cb.float().cpu().double() - ref).abs().max()) < 1e-2 * scale
    # unsupported forms are refused, not mis-computed
    assert lib.afr_op_gemm_fp8(_lib.GEMM_A_KSTRIDED, ptr(A8), ptr(B8), ptr(Cb), C.c_void_p(0), M, N, K, K, K, N, 1.0, stream()) == -4


def test_fp8_gemm_rate_against_the_5pf_roof():
    """Throughput of the fp8 product at a chip-filling shape (8192^3, random e4m3 operands), printed as a fraction of the 5 PF
    dense fp8 peak; asserted only to beat the bf16 ring kernel's best (1.3 PF): the MX-scaled instruction is in use."""
    lib = _lib.lib()
    M = N = K = 8192
    A8, _ = _to_fp8(rand(321, (M, K), 3.0), 0.01)
    B8, _ = _to_fp8(rand(322, (N, K), 3.0), 0.01)
    Cb = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    run = lambda: _lib.check(lib.afr_op_gemm_fp8(_lib.GEMM_OUT_BF16, ptr(A8), ptr(B8), ptr(Cb), C.c_void_p(0), M, N, K, K, K, N, 1e-4, stream()))
    for _ in range(5):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 20
    pf = 2.0 * M * N * K / (ms * 1e-3) / 1e15
    print(f"fp8 gemm 8192^3: {ms * 1e3:.1f} us, {pf:.2f} PF = {pf / 5.0:.2f} of the 5 PF dense fp8 peak")
    assert pf > 1.3


def test_fp8_linear_on_the_c5_mini_layer_shapes():
    """BASELINE configs[4] in miniature: the first block's MLP up-projection of the C5-mini fixture model (pixel_twin.npz's
    net: 32 glyphs x 64 pixel tokens = 2048 rows, d_model 512 -> ff 2048) with fp8 weights AND activations through
    afr_op_gemm_fp8 (bias + ReLU epilogue, bf16 out).  Against the exact product of the e4m3 operands (kernel correctness)
    and against the f32 oracle's relu(fc1(LN2(h))) (what e4m3 costs on this layer: a few percent of the largest activation)."""
    from ai_font_renderer_amd.config import C5_MINI as cfg
    from .util import load, oracle, tparams
    lib = _lib.lib()
    fx = load("pixel_twin.npz")
    P = tparams(cfg)
    _, cache = oracle.pixel_forward(P, torch.from_numpy(fx["x"]), torch.from_numpy(fx["font"]), cfg)
    n2 = cache["saved"][0]["n2"].reshape(-1, cfg.d_model)             # [2048, 512]
    W, b = P["layers.0.fc1.weight"], P["layers.0.fc1.bias"]
    f_ref = cache["saved"][0]["f"].reshape(-1, cfg.ff_dim)
    sa, sw = float(n2.abs().max()) / 448.0, float(W.abs().max()) / 448.0
    A8, Av = _to_fp8(n2, sa)
    W8, Wv = _to_fp8(W, sw)
    M, K, N = n2.shape[0], cfg.d_model, cfg.ff_dim
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device="cuda")
    _lib.check(lib.afr_op_gemm_fp8(_lib.GEMM_BIAS | _lib.GEMM_RELU | _lib.GEMM_OUT_BF16, ptr(A8), ptr(W8), ptr(out), ptr(dev(b)), M, N, K, K, K, N,
                                   sa * sw, stream()))
    torch.cuda.synchronize()
    got = out.float().cpu().double()
    exact = torch.relu(Av.double() @ Wv.double().t() + b.double())
    top = float(f_ref.abs().max())
    assert float((got - exact).abs().max()) < 1e-2 * top                       # bf16 output rounding
    err = float((got - f_ref.double()).abs().max()) / top
    print(f"C5-mini fc1 in e4m3 (per-tensor scales): max |err| = {err:.3f} of the largest activation")
    assert err < 8e-2
