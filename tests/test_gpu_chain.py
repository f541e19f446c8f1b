"""GPU: the chained gradient launch (csrc/gemm.hip GemmGroup::chain) -- the output layer's and the last hidden layer's gradient pairs
as ONE launch, in which the upper pair's workgroups hand the output layer's input gradient to the lower pair's inside the launch.  Every
result must be bit for bit what the two grouped launches give: same kernels, tiles, slices, K order and epilogues.
Op level: afr_op_linear_chain against two afr_op_linear(AFR_LIN_PAIR) launches on the same descriptors, at the smallest layer triple
the planner chains (tests/test_chain_cpu.py SMALLEST).  Engine level: C3 with config.reserved 0 against 256 (AFR_CFG_NO_PAIR_CHAIN)."""
import ctypes as C

import pytest
import torch

from .gpu_util import linear_pair_plan, ptr, stream
from .op_harness import Outs, same
from .test_chain_cpu import SMALLEST
from .util import glyph_inputs, rand, synth

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
OPT = dict(lr=1e-3, beta1=0.9, beta2=0.99, eps=1e-8, weight_decay=0.01, t=3, grad_scale=1.0)
VARIANTS = ("plain", "adamw", "lion", "gather", "bits")


def _plan(shape):
    from ai_font_renderer_amd import _lib
    su, sl, nb, ws = C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
    _lib.check(_lib.lib().afr_op_linear_chain_plan(*shape, 0, C.byref(su), C.byref(sl), C.byref(nb), C.byref(ws)))
    return su.value, sl.value, nb.value, ws.value


_INPUTS = {}


def _inputs(shape):
    """The operands of the two layers, made once: dy [3][B][N_up] (three different output gradients), the activations x_up [B][K_up]
    and x_lo [B][K_lo] (about half of each <= 0, so that the ReLU gates matter), the weights, a 190-row table + row map whose gathered
    rows stand for x_lo, the gates as bits, and the optimizer state."""
    if shape in _INPUTS:
        return _INPUTS[shape]
    B, N_up, K_up, K_lo = shape
    d = {}
    d["dy"] = (rand(4001, (3, B, N_up)) * 0.05).to(BF).cuda()
    d["x_up"] = rand(4002, (B, K_up)).to(BF).cuda()
    d["x_lo"] = rand(4003, (B, K_lo)).to(BF).cuda()
    d["W_up"] = (rand(4004, (N_up, K_up)) * 0.05).to(BF).cuda()
    d["W_lo"] = (rand(4005, (K_up, K_lo)) * 0.05).to(BF).cuda()
    d["table"] = rand(4006, (190, K_lo)).to(BF).cuda()
    d["rows"] = ((torch.arange(B) * 37 + 11) % 190).to(torch.int32).cuda()

    def as_bits(a):                        # bit k & 7 of byte [b][k / 8] = [a(b, k) > 0]
        g = (a.float() > 0).to(torch.uint8).reshape(a.shape[0], -1, 8)
        return (g << torch.arange(8, device=a.device, dtype=torch.uint8)).sum(-1).to(torch.uint8).contiguous()
    d["bits_up"], d["bits_lo"] = as_bits(d["x_up"]), as_bits(d["x_lo"])
    for nm, (n, k) in (("up", (N_up, K_up)), ("lo", (K_up, K_lo))):
        d["p_" + nm] = rand(4010 + len(nm), (n, k)).cuda() * 0.05
        d["m_" + nm] = rand(4020 + len(nm), (n, k)).cuda() * 0.01
        d["v_" + nm] = (rand(4030 + len(nm), (n, k)).cuda() * 0.01) ** 2
    _INPUTS[shape] = d
    return d


def _tails(shape, variant, o, d):
    """(tail_up, tail_lo, x_lo operand): the tails of both pairs for the variant, outputs allocated in `o`"""
    B, N_up, K_up, K_lo = shape
    su, sl, _, _ = _plan(shape)
    tu = dict(db=o.new("db_up", (su, N_up), F32), aux=d["x_up"])
    tl = dict(db=o.new("db_lo", (sl, K_up), F32), aux=d["x_lo"])
    x_lo = d["x_lo"]
    if variant in ("adamw", "lion"):
        for t, nm, (n, k) in ((tu, "up", (N_up, K_up)), (tl, "lo", (K_up, K_lo))):
            t.update(OPT, opt_kind=1 if variant == "lion" else 0, p=o.new("p_" + nm, (n, k), F32, init=d["p_" + nm]),
                     m=o.new("m_" + nm, (n, k), F32, init=d["m_" + nm]), shadow=o.new("shadow_" + nm, (n, k), BF))
            if variant == "adamw":
                t["v"] = o.new("v_" + nm, (n, k), F32, init=d["v_" + nm])
    if variant == "gather":                # the lower layer's input as rows of a table: the dW member and the ReLU gate gather
        x_lo = d["table"]
        tl.update(x_rows=d["rows"], aux=d["table"], aux_rows=d["rows"])
    if variant == "bits":
        tu.update(mask_in=d["bits_up"], ldmask=K_up // 8)
        tl.update(mask_in=d["bits_lo"], ldmask=K_lo // 8)
    return tu, tl, x_lo


def _tail_struct(t):
    from ai_font_renderer_amd import _lib
    s = _lib.AfrLinearTail()
    for k, v in t.items():
        setattr(s, k, v.data_ptr() if isinstance(v, torch.Tensor) else v.value if isinstance(v, C.c_void_p) else v)
    return s


def _launch(shape, variant, chained, dy_index=0, repeats=(0,)):
    """The four products on fresh guarded outputs: ONE afr_op_linear_chain launch, or the same two pairs as two afr_op_linear
    launches.  repeats: the dy used by each launch on the same buffers (no host synchronisation between them); -> the outputs."""
    from ai_font_renderer_amd import _lib
    B, N_up, K_up, K_lo = shape
    d = _inputs(shape)
    o = Outs()
    fused = variant in ("adamw", "lion")
    out_up, out_lo = o.new("dW_up", (N_up, K_up), F32), o.new("dW_lo", (K_up, K_lo), F32)
    mid, dx_lo = o.new("mid", (B, K_up), BF, guard=K_up), o.new("dx_lo", (B, K_lo), BF, guard=K_lo)
    tu, tl, x_lo = _tails(shape, variant, o, d)
    ws = torch.full((_plan(shape)[3],), 0x5A, dtype=torch.uint8, device="cuda")        # dirty on purpose: the op owns its state
    pu = _pair_ws(B, N_up, K_up)                 # the chain's workspace starts with the upper pair's, then the lower pair's
    for r in repeats:
        dy = d["dy"][(dy_index + r) % 3]
        if chained:
            su_, sl_ = _tail_struct(tu), _tail_struct(tl)
            name = C.create_string_buffer(64)
            _lib.check(_lib.lib().afr_op_linear_chain(ptr(dy), ptr(d["x_up"]), ptr(d["W_up"]), out_up, mid, C.byref(su_), ptr(x_lo), ptr(d["W_lo"]),
                                                      out_lo, dx_lo, C.byref(sl_), B, N_up, K_up, K_lo, ptr(ws), ws.numel(), name, 64, stream()))
            assert name.value.decode() == ("gemm_bf16_group256_lion" if variant == "lion" else "gemm_bf16_group256")
        else:
            su_, sl_ = _tail_struct(tu), _tail_struct(tl)
            lib = _lib.lib()
            _lib.check(lib.afr_op_linear(_lib.AFR_BF16, _lib.LIN_PAIR, ptr(d["x_up"]), ptr(d["W_up"]), None, ptr(dy), out_up, mid, B, N_up, K_up,
                                         C.byref(su_), ptr(ws), pu, None, 0, stream()))
            _lib.check(lib.afr_op_linear(_lib.AFR_BF16, _lib.LIN_PAIR, ptr(x_lo), ptr(d["W_lo"]), None, mid, out_lo, dx_lo, B, K_up, K_lo,
                                         C.byref(sl_), C.c_void_p(ws.data_ptr() + pu), ws.numel() - pu, None, 0, stream()))
    return o.finish(may_keep_fill=("dW_up", "dW_lo") if fused else ())


def _pair_ws(B, N, K):
    return linear_pair_plan(B, N, K)[3]


@pytest.mark.parametrize("variant", VARIANTS)
def test_one_chained_launch_equals_the_two_grouped_launches(variant):
    """dW_up, db_up, mid (= dh of the hidden layer), dW_lo, db_lo, dx_lo, p / m / v and both shadows, between guard bands: bit for bit
    the two launches'."""
    got = _launch(SMALLEST, variant, True)
    ref = _launch(SMALLEST, variant, False)
    same(got, ref, f"chained against two launches ({variant})")
    assert float(got["mid"].float().abs().max()) > 0 and float(got["dx_lo"].float().abs().max()) > 0


def test_no_stale_hand_off_across_launches_on_the_same_buffers():
    """Three launches on the same buffers, each with another dy, the last two without a host synchronisation in between: every word
    of the third launch's results is the two-launch reference's for ITS dy.  A stale L1 or L2 line of `mid` in a lower-pair
    workgroup would show as the previous dy's rows in dW_lo / dx_lo."""
    got = _launch(SMALLEST, "plain", True, repeats=(0, 1, 2))
    ref = _launch(SMALLEST, "plain", False, dy_index=2)
    prev = _launch(SMALLEST, "plain", False, dy_index=1)
    same(got, ref, "third chained launch against the two launches on its dy")
    assert not torch.equal(prev["mid"], ref["mid"]) and not torch.equal(prev["dx_lo"], ref["dx_lo"])      # (the dys do differ)


def _engine(cfg, B, flags):
    from ai_font_renderer_amd.engine import Engine
    eng = Engine(cfg, dtype="bf16", max_batch=B, flags=flags)
    eng.load_params(synth.make_params(cfg))
    return eng


def _group256_launches(eng, step):
    eng.profile(1)
    step()
    eng.read_loss()
    n = sum(r["launches"] for r in eng.profile_table() if r["kernel"].startswith("gemm_bf16_group256["))
    eng.profile(0)
    return n


@pytest.mark.parametrize("B", [8192, 8008])
def test_c3_chained_step_equals_the_two_launch_step(B):
    """C3 at the bench's batch and at a ragged one, config.reserved 0 (chained) against 256: the loss, every gradient of a
    do_step=False step, and the parameters and both moments after three optimizer steps agree bit for bit; no error flag; the
    profile table shows one gemm_bf16_group256[ launch per step chained and two unchained."""
    from ai_font_renderer_amd.config import WORKLOADS
    cfg = WORKLOADS["c3"]["cfg"]
    x, font, tu8 = glyph_inputs(cfg, B)
    xt, ft, tt = torch.from_numpy(x), torch.from_numpy(font), torch.from_numpy(tu8)
    engs = {fl: _engine(cfg, B, fl) for fl in (0, 256)}
    loss = {}
    for fl, e in engs.items():
        e.train_step(xt, tt, font=ft, do_step=False)
        loss[fl] = e.read_loss()
    assert loss[0] == loss[256]
    for k in engs[0].grads:
        assert torch.equal(engs[0].grads[k], engs[256].grads[k]), k
    count = {}
    for fl, e in engs.items():
        for _ in range(2):
            e.train_step(xt, tt, font=ft)
        count[fl] = _group256_launches(e, lambda: e.train_step(xt, tt, font=ft))
    assert engs[0].read_loss() == engs[256].read_loss()
    assert torch.equal(engs[0].flat_params, engs[256].flat_params)
    assert torch.equal(engs[0].exp_avg, engs[256].exp_avg) and torch.equal(engs[0].exp_avg_sq, engs[256].exp_avg_sq)
    assert count == {0: 1, 256: 2}, count
    for e in engs.values():
        assert e.error_flags() == 0
