"""CPU: the checker of the Linear products' tails (tests/linear_ref.py) is itself checked against torch's own ops at the shapes
tests/test_gpu_linear_ops.py uses; the planner answers that file relies on are held true; and afr_op_linear refuses, before it
launches anything, what it must refuse (host-only calls on made-up pointers)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from . import linear_ref as R

F64 = torch.float64
TILE_SHAPES = [(200, 136, 96), (264, 192, 128)]
RING_FWD = (7384, 1024, 256)
PAIR_256 = [(2048, 256, 3712), (2048, 256, 3704)]
PAIR_128 = (7176, 256, 1016)


# ------------------------------------------------------------------------------------------- bits, slices, gathers
@pytest.mark.parametrize("M,N", [(200, 136), (264, 192), (5, 8)])
def test_pack_bits_is_numpy_packbits_little(M, N):
    m = R.rnd(11, (M, N)) > 0
    got = R.pack_bits(m)
    assert got.dtype == torch.uint8 and got.shape == (M, N // 8)
    assert np.array_equal(got.numpy(), np.packbits(m.numpy(), axis=1, bitorder="little"))
    assert torch.equal(R.unpack_bits(got, N), m)
    one = torch.zeros(1, 16, dtype=torch.bool)
    one[0, 11] = True                                     # bit 11 & 7 = 3 of byte 11 / 8 = 1
    assert R.pack_bits(one).tolist() == [[0, 8]]


def test_k_slices_follow_k_range():
    assert R.k_slices(320, 4, 64) == [(0, 128), (128, 256), (256, 320), (320, 320)]          # the issue's example: the last slice is empty
    assert R.k_slices(320, 4, 32) == [(0, 96), (96, 192), (192, 288), (288, 320)]
    assert R.k_slices(200, 3, 64) == [(0, 128), (128, 200), (200, 200)]
    assert R.k_slices(200, 3, 32) == [(0, 96), (96, 192), (192, 200)]
    assert R.k_slices(200, 5, 32) == [(0, 64), (64, 128), (128, 192), (192, 200), (200, 200)]
    assert R.k_slices(200, 1, 64) == [(0, 200)]
    s = R.k_slices(14848, 58, 64)
    assert all(e - a == 256 for a, e in s)
    s = R.k_slices(15000, 58, 64)                        # slices of 320: 46 whole, one of 280, eleven empty
    assert [e - a for a, e in s] == [320] * 46 + [280] + [0] * 11
    for Rr, sk, bk in [(200, 3, 32), (200, 3, 64), (320, 4, 64), (15000, 58, 64), (7176, 15, 64)]:
        s = R.k_slices(Rr, sk, bk)
        assert len(s) == sk and s[0][0] == 0 and max(e for _, e in s) == Rr
        assert all(a % bk == 0 or a == Rr for a, _ in s)
        assert all(s[i][1] == s[i + 1][0] or s[i + 1][0] == s[i + 1][1] for i in range(sk - 1))


@pytest.mark.parametrize("B,sk,bk", [(200, 1, 32), (200, 3, 32), (200, 3, 64), (200, 5, 32), (320, 4, 64), (320, 4, 32)])
def test_slices_add_up_to_the_whole(B, sk, bk):
    N, K = 136, 96
    dy, x = R.rnd(21, (B, N)), R.rnd(22, (B, K))
    cs, ws = R.colsum_slices(dy, sk, bk), R.dw_slices(dy, x, sk, bk)
    assert cs.shape == (sk, N) and ws.shape == (sk, N, K)
    assert torch.allclose(cs.sum(0), dy.double().sum(0), rtol=0, atol=1e-12)
    assert torch.allclose(ws.sum(0), torch.einsum("bn,bk->nk", dy.double(), x.double()), rtol=0, atol=1e-11)
    for z, (a, e) in enumerate(R.k_slices(B, sk, bk)):
        if a == e:
            assert not cs[z].any() and not ws[z].any()


@pytest.mark.parametrize("B,N,K", TILE_SHAPES)
def test_products_are_torchs(B, N, K):
    i = R.linear_inputs("f32", B, N, K)
    x, W, b, dy = (i[k].double() for k in ("x", "W", "b", "dy"))
    assert torch.allclose(R.fwd(i["x"], i["W"], i["b"]), F.linear(x, W, b), rtol=0, atol=1e-12)
    xa, Wa = x.clone().requires_grad_(), W.clone().requires_grad_()
    F.linear(xa, Wa, b).backward(dy)
    assert torch.allclose(R.dx(i["dy"], i["W"]), xa.grad, rtol=0, atol=1e-12)
    assert torch.allclose(R.dw(i["dy"], i["x"]), Wa.grad, rtol=0, atol=1e-11)
    assert torch.allclose(R.colsum_slices(i["dy"], 1, 32)[0], dy.sum(0), rtol=0, atol=1e-12)


def test_rounded_operands_and_gathers():
    t = R.rnd(31, (77, 40))
    assert torch.equal(R.rounded("bf16", t), t.bfloat16().float()) and torch.equal(R.rounded("bf16x3", t), t) and torch.equal(R.rounded("f32", t), t)
    for n, h in [(200, 77), (7384, 250), (2048, 1001)]:
        assert h % 8
        r = R.row_map(n, h)
        assert r.dtype == torch.int32 and int(r.min()) == 0 and int(r.max()) == h - 1
        d = np.diff(r.numpy().astype(np.int64))
        assert (d > 0).any() and (d < 0).any()                              # not monotone
        assert len(np.unique(r.numpy())) < n                                # repeats
    r = R.row_map(200, 77)
    assert torch.equal(R.gather(t, r), torch.index_select(t, 0, r.long()))


# ------------------------------------------------------------------------------------------------------- loss
@pytest.mark.parametrize("kind", ["mse", "bce"])
def test_loss_du_is_torchs_loss_and_gradient(kind):
    B, N = 200, 136
    i = R.linear_inputs("f32", B, N, 96)
    u = R.fwd(i["x"], i["W"], i["b"]).requires_grad_()
    t = R.target_f32(R.targets_u8(41, B, N)).double()
    n = B * N * 3
    if kind == "mse":
        want = F.mse_loss(u.clamp(0.0, 1.0), t, reduction="sum") / n
    else:
        want = F.binary_cross_entropy_with_logits(u, t, reduction="sum") / n
    want.backward()
    loss, du = R.loss_du(kind, u.detach(), t, n)
    assert abs(float(loss) - float(want.detach())) <= 1e-12 * float(want.detach())
    assert torch.allclose(du, u.grad, rtol=0, atol=1e-15)
    assert R.target_f32(torch.tensor([[0, 51, 255]], dtype=torch.uint8)).tolist() == [[0.0, float(np.float32(51) / np.float32(255)), 1.0]]


@pytest.mark.parametrize("B,N,K", TILE_SHAPES + [RING_FWD])
def test_a_third_to_a_half_of_the_pre_activations_lie_inside_the_clamp(B, N, K):
    for dtype in ("f32", "bf16"):
        i = R.linear_inputs(dtype, B, N, K)
        u = R.fwd(i["x"], i["W"], i["b"])
        inside = float(((u > 0) & (u < 1)).double().mean())
        assert 0.3 <= inside <= 0.55, (dtype, inside)                                          # "about a third to a half"
        assert float((u <= 0).double().mean()) > 0.1 and float((u >= 1).double().mean()) > 0.1      # both ends of the clamp are met


# -------------------------------------------------------------------------------------------------- optimizer
def test_adamw_is_torch_optim_adamw():
    """From random m, positive v and t = 3 (the state the GPU tests start from), against torch.optim.AdamW in fp64; the float32
    folding of the step's scalars moves a result by a few 2^-24 relative."""
    n = 136 * 96
    p0, g = R.rnd(51, (n,), 0.2).double(), R.rnd(52, (n,), 30.0).double()
    m0, v0 = R.rnd(53, (n,), 3.0).double(), (R.rnd(54, (n,), 50.0).double().abs() + 1e-3)
    lr, b1, b2, eps, wd = 1e-3, 0.9, 0.99, 1e-8, 5e-4
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    opt.state[p] = {"step": torch.tensor(2.0), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    p.grad = g.clone()
    opt.step()
    gp, gm, gv = R.adamw(p0, g, m0, v0, 3, lr, b1, b2, eps, wd)
    st = opt.state[p]
    assert float(st["step"]) == 3.0
    for got, want in ((gp, p.detach()), (gm, st["exp_avg"]), (gv, st["exp_avg_sq"])):
        assert float((got - want).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max()))
    assert float((gp - p0).abs().max()) > 1e-4                                                  # the step moved the weights


# ---------------------------------------------------------------------------------------------------- bounds
def test_bounds_are_the_suites():
    ref = torch.tensor([[0.5, -3.0]], dtype=F64)
    assert R.f32_bound(96, ref) == (2e-6 * 96 ** 0.5 + 1e-6) * 3.0
    assert R.f32_bound(96, ref * 0.1) == 2e-6 * 96 ** 0.5 + 1e-6
    b = R.product_bound("bf16", 96, ref, out_bf16=True)
    assert torch.equal(b, R.f32_bound(96, ref) + 2.0 ** -8 * ref.abs())
    ap = torch.tensor([[2.0, 4.0]], dtype=F64)
    assert torch.equal(R.product_bound("bf16x3", 96, ref, ap), (3 * 2.0 ** -16 + 96 * 2.0 ** -24) * ap)


# --------------------------------------------------------------------------------- the library's host side
def _plan(B, N, K):
    from ai_font_renderer_amd import _lib
    t, s, c, w = C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
    rc = _lib.lib().afr_op_linear_pair_plan(B, N, K, C.byref(t), C.byref(s), C.byref(c), C.byref(w))
    return (rc, t.value, s.value, c.value, w.value)


def test_pair_planner_answers_the_gpu_tests_rely_on():
    from ai_font_renderer_amd import _lib
    for B, N, K in PAIR_256:                              # cooperative 256x256, 8 slices: afr_op_gemm_pair_plan's answer
        rc, t256, sk, coop, ws = _plan(B, N, K)
        assert (rc, t256, sk, coop) == (0, 1, 8, 1)
        sk2, ws2 = C.c_int(), C.c_size_t()
        assert _lib.lib().afr_op_gemm_pair_plan(B, N, K, C.byref(sk2), C.byref(ws2)) == 0 and (sk2.value, ws2.value) == (sk, ws)
    # the smallest batch (a multiple of 8) whose pair at N = 256 and eight 128-column tiles of the input gradient (K = 1016, ragged)
    # leaves as ONE grouped launch: 29 x 8 = 232 tiles.  Not cooperative, 256x128 tiles, 15 slabs.
    B, N, K = PAIR_128
    assert _plan(B, N, K) == (0, 0, 15, 0, 0)
    assert _plan(B - 8, N, K)[0] == _lib.AFR_EUNSUPPORTED and b"grouped" in _lib.lib().afr_last_error()
    assert _plan(200, 136, 96)[0] == _lib.AFR_EUNSUPPORTED


def test_entry_refuses_before_it_launches():
    from ai_font_renderer_amd import _lib
    lib, EI, EU = _lib.lib(), _lib.AFR_EINVAL, _lib.AFR_EUNSUPPORTED
    fk = C.c_void_p(0x1000)

    def call(dtype=_lib.AFR_BF16, which=_lib.LIN_FWD, B=7384, N=1024, K=256, x=fk, W=fk, bias=fk, dy=fk, out=fk, out2=fk, ws=None, wsb=0, **tail):
        t = _lib.AfrLinearTail()
        for k, v in tail.items():
            setattr(t, k, v)
        return lib.afr_op_linear(dtype, which, x, W, bias, dy, out, out2, B, N, K, C.byref(t), ws, wsb, None, 0, None)

    FWD, DX, DW, PAIR = _lib.LIN_FWD, _lib.LIN_DX, _lib.LIN_DW, _lib.LIN_PAIR
    loss = dict(target=0x1000, loss_accum=0x1000, loss_scratch=0x1000, mean_elems=100)
    assert call(dtype=7) == EI and call(which=4) == EI and call(B=0) == EI and call(out=None) == EI
    assert call(x=None) == EI and call(bias=None) == EI and call(which=DX, dy=None) == EI and call(which=DW, x=None) == EI
    assert call(which=PAIR, out2=None, B=2048, N=256, K=3712) == EI
    assert call(N=1020) == EU and b"multiples of 8" in lib.afr_last_error()
    assert call(ld_out=1000) == EI and call(ld_out=1028) == EU
    # a tail the product does not have
    assert call(which=DX, **loss) == EI and call(which=DW, mask_out=0x1000) == EI and call(aux=0x1000) == EI
    assert call(db=0x1000) == EI and call(which=DX, splitk=2) == EI and call(which=DX, p=0x1000) == EI and call(which=DX, x_rows=0x1000) == EI
    assert call(which=DW, x_rows=0x1000) == EU and b"cooperative" in lib.afr_last_error()
    # the loss
    assert call(target=0x1000, loss_scratch=0x1000, mean_elems=100) == EI               # no loss_accum
    assert call(**loss, target_dtype=2) == EI and call(**dict(loss, mean_elems=0)) == EI and call(**loss, loss_kind=2) == EI
    assert call(**dict(loss, loss_scratch=None)) == EI and call(target_rows=0x1000) == EI and call(**loss, mask_out=0x1000, ldmask=128) == EI
    # bits
    assert call(dtype=_lib.AFR_F32, mask_out=0x1000, ldmask=128) == EI and call(mask_out=0x1000, ldmask=127) == EI
    assert call(which=DX, mask_in=0x1000, ldmask=31) == EI and call(which=DX, dtype=_lib.AFR_BF16X3, mask_in=0x1000, ldmask=32) == EI
    assert call(which=DX, aux_rows=0x1000) == EI and call(which=DX, aux=0x1000, ldaux=248) == EI
    # the optimizer
    opt = dict(p=0x1000, m=0x1000, v=0x1000, t=3, grad_scale=1.0, lr=1e-3, beta1=0.9, beta2=0.99, eps=1e-8)
    assert call(which=DW, **dict(opt, t=0)) == EI and call(which=DW, **dict(opt, v=None)) == EI and call(which=DW, **dict(opt, opt_kind=2)) == EI
    assert call(which=DW, **opt, splitk=2) == EI and b"splitk must be 1" in lib.afr_last_error()
    assert call(which=DW, **dict(opt, grad_scale=0.5)) == EU and b"unscaled" in lib.afr_last_error()
    assert call(which=DW, dtype=_lib.AFR_F32, **opt, shadow=0x1000) == EI
    # what the launchers refuse comes back as a refusal with a message, never as another kernel
    for tail in (dict(loss, loss_kind=_lib.AFR_LOSS_BCE, x_rows=0x1000), dict(loss, target_rows=0x1000, x_rows=0x1000),
                 dict(x_rows=0x1000, B=200, N=136, K=96)):              # BCE / row-mapped targets on gathered rows; a row map off the ring
        assert call(**tail) == EU and b"launcher refuses" in lib.afr_last_error(), tail
    assert call(which=DX, dtype=_lib.AFR_F32, aux=0x1000, aux_rows=0x1000) == EU and b"launcher refuses" in lib.afr_last_error()
    # pairs
    assert call(which=PAIR, dtype=_lib.AFR_F32, B=2048, N=256, K=3712, db=0x1000) == EU
    assert call(which=PAIR, B=200, N=136, K=96, db=0x1000) == EU and b"grouped" in lib.afr_last_error()
    assert call(which=PAIR, B=2048, N=256, K=3712) == EI                                 # db is required
    assert call(which=PAIR, B=2048, N=256, K=3712, db=0x1000) == EI and b"workspace" in lib.afr_last_error()
    assert call(which=PAIR, B=7176, N=256, K=1016, db=0x1000, x_rows=0x1000) == EU and call(which=PAIR, B=7176, N=256, K=1016, db=0x1000, **opt) == EU
