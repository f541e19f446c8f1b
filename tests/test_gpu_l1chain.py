"""GPU: the folded first layer's fused backward as the FIFTH role of the chained gradient launch (csrc/gemm.hip GemmGroup::l1): its
workgroups follow the four products' in the grid and are handed d1 = dx_lo inside the launch.  Every result must be bit for bit what
the chained launch followed by afr_op_glyph_l1_bwd_fused on its dx_lo gives: same pieces, images, products and orders.
Op level: afr_op_linear_chain_l1 against afr_op_linear_chain + afr_op_glyph_l1_bwd_fused at the two shapes of tests/test_l1chain_cpu.py
(the one first-layer width that chains, ragged and whole blocks).  Engine level: C3 with config.reserved 0 against 512
(AFR_CFG_NO_L1_CHAIN) and 256 (AFR_CFG_NO_PAIR_CHAIN)."""
import ctypes as C

import numpy as np
import pytest
import torch

from .gpu_util import ptr, stream
from .op_harness import Outs, same, twice
from .test_gpu_chain import _engine, _inputs, _tail_struct, _tails
from .test_l1chain_cpu import FONTS, RAGGED, TWO_RANGES, VOCAB
from .util import glyph_inputs, rand

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
SHAPES = [pytest.param(RAGGED, id="7944x1000x1000x1024"), pytest.param(TWO_RANGES, id="8192x1024x1024x1024")]
LOSS_N, LOSS_BD = 700, 512            # deferred loss partials of a made-up producer launch: some threads add two of them, some one


def _ws_bytes(shape):
    from ai_font_renderer_amd import _lib
    nb, ws = C.c_int(), C.c_size_t()
    _lib.check(_lib.lib().afr_op_linear_chain_l1_plan(*shape, VOCAB, FONTS, 0, 0, C.byref(nb), C.byref(ws)))
    return ws.value


_GLYPH = {}


def _glyph(shape):
    """The first layer's own operands, made once: h0 dense [B][32] and as a 190-row table behind the chain inputs' row map, W1^T
    [32][N1], the codes and font ids, and loss partials."""
    if shape not in _GLYPH:
        B, _, _, N1 = shape
        g = {}
        g["h0"] = rand(4101, (B, 32)).to(BF).cuda()
        g["h0_table"] = rand(4102, (190, 32)).to(BF).cuda()
        g["W1T"] = (rand(4103, (32, N1)) * 0.05).to(BF).cuda()
        g["x"] = ((torch.arange(B) * 31 + 5) % VOCAB).to(torch.int64).cuda()
        g["font"] = ((torch.arange(B) * 13 + 3) % FONTS).to(torch.int64).cuda()
        g["partial"] = rand(4104, (LOSS_N,)).abs().cuda()
        _GLYPH[shape] = g
    return _GLYPH[shape]


def _launch(shape, variant, one_launch, dy_index=0, repeats=(0,), rowmap=False, loss=False):
    """The four products and the first-layer slabs on fresh guarded outputs: ONE afr_op_linear_chain_l1 launch, or afr_op_linear_chain
    followed by afr_op_glyph_l1_bwd_fused on its dx_lo.  repeats: the dy of each launch on the same buffers (no host synchronisation
    between them); -> the outputs (loss: the accumulator of the one launch as well)."""
    from ai_font_renderer_amd import _lib
    lib = _lib.lib()
    B, N_up, K_up, N1 = shape
    d, g = _inputs(shape), _glyph(shape)
    o = Outs()
    fused = variant in ("adamw", "lion")
    out_up, out_lo = o.new("dW_up", (N_up, K_up), F32), o.new("dW_lo", (K_up, N1), F32)
    mid, dx_lo = o.new("mid", (B, K_up), BF, guard=K_up), o.new("dx_lo", (B, N1), BF, guard=N1)
    nb, fl = lib.afr_glyph_l1_bwd_fused_blocks(B, N1), lib.afr_glyph_l1_bwd_fused_slab_floats(B, N1, VOCAB, FONTS)
    slabs = o.new("slabs", (nb, fl), F32, guard=fl)
    tu, tl, x_lo = _tails(shape, variant, o, d)
    ws = torch.full((_ws_bytes(shape),), 0x5A, dtype=torch.uint8, device="cuda")        # dirty on purpose: the op owns its state
    h0, rm = (g["h0_table"], d["rows"]) if rowmap else (g["h0"], None)
    accum = torch.zeros(1, dtype=F32, device="cuda")
    assert not loss or one_launch
    for r in repeats:
        dy = d["dy"][(dy_index + r) % 3]
        su_, sl_ = _tail_struct(tu), _tail_struct(tl)
        name = C.create_string_buffer(64)
        if one_launch:
            _lib.check(lib.afr_op_linear_chain_l1(ptr(dy), ptr(d["x_up"]), ptr(d["W_up"]), out_up, mid, C.byref(su_), ptr(x_lo), ptr(d["W_lo"]),
                                                  out_lo, dx_lo, C.byref(sl_), B, N_up, K_up, N1, ptr(ws), ws.numel(),
                                                  dx_lo, ptr(h0), 32, ptr(rm), ptr(g["W1T"]), ptr(g["x"]), ptr(g["font"]), VOCAB, FONTS, slabs,
                                                  ptr(g["partial"]) if loss else None, LOSS_N, LOSS_BD, 0.125, ptr(accum) if loss else None,
                                                  name, 64, stream()))
        else:
            _lib.check(lib.afr_op_linear_chain(ptr(dy), ptr(d["x_up"]), ptr(d["W_up"]), out_up, mid, C.byref(su_), ptr(x_lo), ptr(d["W_lo"]),
                                               out_lo, dx_lo, C.byref(sl_), B, N_up, K_up, N1, ptr(ws), ws.numel(), name, 64, stream()))
            _lib.check(lib.afr_op_glyph_l1_bwd_fused(dx_lo, ptr(h0), 32, ptr(rm), ptr(g["W1T"]), ptr(g["x"]), ptr(g["font"]), B, N1, VOCAB, FONTS,
                                                     slabs, stream()))
        assert name.value.decode() == ("gemm_bf16_group256_lion" if variant == "lion" else "gemm_bf16_group256")
    out = o.finish(may_keep_fill=("dW_up", "dW_lo") if fused else ())
    if loss:
        out["accum"] = accum.cpu()
    return out


@pytest.mark.parametrize("variant,rowmap", [("plain", False), ("adamw", True), ("lion", False)])
@pytest.mark.parametrize("shape", SHAPES)
def test_one_launch_with_the_first_layer_role_equals_chain_then_first_layer_kernel(shape, variant, rowmap):
    """dW_up, db_up, mid, dW_lo, db_lo, dx_lo, p / m / v, both shadows and every first-layer slab [dW1 | db1 | dTab], between guard
    bands: bit for bit the two launches'; each launch form repeated on fresh buffers repeats its bytes.  (adamw: h0 as gathered rows of
    a table, as a combination-table step passes it.)"""
    got = twice(lambda: _launch(shape, variant, True, rowmap=rowmap))
    ref = twice(lambda: _launch(shape, variant, False, rowmap=rowmap))
    same(got, ref, f"one launch against chain + first-layer kernel ({variant})")
    assert float(got["dx_lo"].float().abs().max()) > 0 and float(got["slabs"].abs().max()) > 0


def test_no_stale_hand_off_across_launches_on_the_same_buffers():
    """Three launches on the same buffers, each with another dy, the last two without a host synchronisation in between: every word
    of the third launch's results, the slabs included, is the separate-launch twin's for ITS dy.  A stale line of dx_lo in a first-layer
    workgroup, or an arrival counted against the previous launch's target, would show as the previous dy's rows in the slabs."""
    got = _launch(RAGGED, "plain", True, repeats=(0, 1, 2))
    ref = _launch(RAGGED, "plain", False, dy_index=2)
    prev = _launch(RAGGED, "plain", False, dy_index=1)
    first = _launch(RAGGED, "plain", False, dy_index=0)
    same(got, ref, "third launch against its separate-launch twin")
    same(_launch(RAGGED, "plain", True, repeats=(0, 1)), prev, "second launch against its twin")
    same(_launch(RAGGED, "plain", True), first, "first launch against its twin")
    assert not torch.equal(prev["slabs"], ref["slabs"]) and not torch.equal(first["slabs"], prev["slabs"])      # (the dys do differ)


def _deferred_sum(partial, n, bd, inv_n):
    """loss_sum_deferred term for term in float32: thread t adds partial[t], partial[t + bd], ... from 0; the LDS tree; sum * inv_n added
    to an accumulator that holds 0 (so a fused multiply-add rounds as the product does)"""
    p = partial.astype(np.float32)
    sh = np.zeros(bd, dtype=np.float32)
    for i in range(n):
        sh[i % bd] = np.float32(sh[i % bd] + p[i])
    o = bd // 2
    while o > 0:
        sh[:o] = sh[:o] + sh[o:2 * o]
        o //= 2
    return np.float32(sh[0] * np.float32(inv_n))


def test_deferred_loss_sum_rides_the_launch():
    """With deferred loss partials attached the grid has one more workgroup, which adds their sum to the accumulator exactly as the
    stand-alone kernel's appended workgroup does (the same device function, re-stated here in float32); every other output is the
    launch's without it.  (The separate launch's accumulator itself is compared through the engine below: a C3 step defers its loss.)"""
    got = _launch(RAGGED, "plain", True, loss=True)
    ref = _launch(RAGGED, "plain", True)
    want = _deferred_sum(_glyph(RAGGED)["partial"].cpu().numpy(), LOSS_N, LOSS_BD, 0.125)
    assert got.pop("accum").numpy()[0] == want
    same(got, ref, "with the loss-sum workgroup against without")


@pytest.mark.parametrize("B", [8192, 8008])
def test_c3_step_with_the_first_layer_role_equals_the_separate_launches(B):
    """C3 at the bench's batch and at a ragged one, three optimizer steps, config.reserved 0 against 512 (the first-layer backward a
    launch of its own) and 256 (no chain at all): every loss, the parameters and both moments agree bit for bit; no error flag; the
    profile table shows one gemm_bf16_group256[ launch and no glyph_l1_bwd_fused row at 0, one of each at 512."""
    from ai_font_renderer_amd.config import WORKLOADS
    cfg = WORKLOADS["c3"]["cfg"]
    x, font, tu8 = glyph_inputs(cfg, B)
    xt, ft, tt = torch.from_numpy(x), torch.from_numpy(font), torch.from_numpy(tu8)
    engs = {fl: _engine(cfg, B, fl) for fl in (0, 512, 256)}
    losses, rows = {}, {}
    for fl, e in engs.items():
        losses[fl] = []
        for st in range(3):
            if st == 2:
                e.profile(1)
            e.train_step(xt, tt, font=ft)
            losses[fl].append(e.read_loss())
        tab = e.profile_table()
        e.profile(0)
        rows[fl] = (sum(r["launches"] for r in tab if r["kernel"].startswith("gemm_bf16_group256[")),
                    sum(r["launches"] for r in tab if r["kernel"].startswith("glyph_l1_bwd_fused")))
    for fl in (512, 256):
        assert losses[0] == losses[fl], (fl, losses)
        assert torch.equal(engs[0].flat_params, engs[fl].flat_params), fl
        assert torch.equal(engs[0].exp_avg, engs[fl].exp_avg) and torch.equal(engs[0].exp_avg_sq, engs[fl].exp_avg_sq), fl
    assert rows == {0: (1, 0), 512: (1, 1), 256: (2, 1)}, rows
    for e in engs.values():
        assert e.error_flags() == 0
