"""CPU: the checker of the pixel transformer's token kernels (tests/pixel_ref.py) is itself checked, on exactly the inputs
tests/test_gpu_pixel_ops.py feeds the kernels: (a) the fp64 restatements ARE the model (composed in the plan's order they reproduce
oracle.pixel_forward / pixel_backward; every backward restatement agrees with autograd of its forward); (b) the float32 restatement
stays within a quarter of every bound; (c) planted subtle faults exceed the bounds at least ten times.  Plus the host-only argument
checks of the afr_op_pixel_* entries."""
import ctypes as C

import pytest
import torch

from . import pixel_ref as R
from .util import oracle, tparams

F64, F32 = torch.float64, torch.float32


# --------------------------------------------------------------------------------------------------------- (a)
def _compose(P, x, font, cfg, du_of):
    """forward and backward of the model as the plan orders its launches: token kernels from pixel_ref, Linear layers as matmuls"""
    d, T, B, L = cfg.d_model, cfg.tokens, x.shape[0], cfg.layers
    rows = B * T
    lin = lambda a, n: a @ P[n + ".weight"].t() + P[n + ".bias"]                                   # noqa: E731
    ctx = R.ctx(P["embedding.weight"], P["font_embedding.weight"] if cfg.n_fonts else None, x, font)
    Cn = ctx.shape[1]
    sv, h, a = [], None, None
    for l in range(L):
        p = f"layers.{l}."
        Win, bin_ = P[p + "attn.in_proj_weight"], P[p + "attn.in_proj_bias"]
        hin, n1 = R.add_ln(h, P["positional_encoding"] if l == 0 else None, a, P[p + "ln1.weight"], P[p + "ln1.bias"], T, rows, cfg.ln_eps)
        q = n1 @ Win[:d].t() + bin_[:d]
        kv = ctx @ Win[d:].t() + bin_[d:]                                                         # [B][C][2 d] = [k | v]
        o = R.attn(q, kv, T)
        h1, n2 = R.add_ln(hin, None, lin(o, p + "attn.out_proj"), P[p + "ln2.weight"], P[p + "ln2.bias"], T, rows, cfg.ln_eps)
        pre = lin(n2, p + "fc1")
        f = torch.relu(pre)
        a, h = lin(f, p + "fc2"), h1
        sv.append(dict(hin=hin, n1=n1, q=q, kv=kv, o=o, h1=h1, n2=n2, pre=pre, f=f))
    hf, u, y = R.head(h, a, P["ln_f.weight"], P["ln_f.bias"], P["fc_output.weight"].reshape(d), P["fc_output.bias"], cfg.ln_eps)
    du = du_of(u.reshape(B, T)).reshape(rows)
    G = {}
    dh, part = R.head_bwd(du, hf, P["ln_f.weight"], P["ln_f.bias"], P["fc_output.weight"].reshape(d), cfg.ln_eps)
    G["ln_f.weight"], G["ln_f.bias"], G["fc_output.weight"], G["fc_output.bias"] = part[0], part[1], part[2].reshape(1, d), part[3, :1]
    dctx = torch.zeros(B, Cn, d, dtype=dh.dtype)
    for l in reversed(range(L)):
        p = f"layers.{l}."
        s = sv[l]
        Win = P[p + "attn.in_proj_weight"]
        G[p + "fc2.weight"], G[p + "fc2.bias"] = dh.t() @ s["f"], dh.sum(0)
        df = (dh @ P[p + "fc2.weight"]) * (s["pre"] > 0)
        G[p + "fc1.weight"], G[p + "fc1.bias"] = df.t() @ s["n2"], df.sum(0)
        dh, lp = R.ln_bwd(df @ P[p + "fc1.weight"], s["h1"], P[p + "ln2.weight"], dh, cfg.ln_eps)
        G[p + "ln2.weight"], G[p + "ln2.bias"] = lp[0], lp[1]
        G[p + "attn.out_proj.weight"], G[p + "attn.out_proj.bias"] = dh.t() @ s["o"], dh.sum(0)
        dq, dkv = R.attn_bwd(dh @ P[p + "attn.out_proj.weight"], s["q"], s["kv"], T)
        dkvT = dkv.reshape(B, 2, 2 * d)[:, :Cn].reshape(B * Cn, 2 * d)                             # row c of sample b = [dk_c | dv_c]
        G[p + "attn.in_proj_weight"] = torch.cat([dq.t() @ s["n1"], dkvT.t() @ ctx.reshape(B * Cn, d)], 0)
        G[p + "attn.in_proj_bias"] = torch.cat([dq.sum(0), dkvT.sum(0)])
        dctx = dctx + (dkvT @ Win[d:]).reshape(B, Cn, d)
        dh, lp = R.ln_bwd(dq @ Win[:d], s["hin"], P[p + "ln1.weight"], dh, cfg.ln_eps)
        G[p + "ln1.weight"], G[p + "ln1.bias"] = lp[0], lp[1]
    G["positional_encoding"] = dh.reshape(B, T, d).sum(0)
    G["embedding.weight"], dfont = R.ctx_bwd(dctx, x, font, cfg.vocab, cfg.n_fonts)
    if cfg.n_fonts:
        G["font_embedding.weight"] = dfont
    return y.reshape(B, cfg.out_h, cfg.out_w), u.reshape(B, T), G


@pytest.mark.parametrize("n_fonts", [2, 0])
def test_a_fp64_restatements_composed_in_model_order_are_the_oracle(n_fonts):
    from ai_font_renderer_amd.config import PixelConfig
    cfg = PixelConfig(out_h=3, out_w=4, d_model=128, heads=2, layers=2, ff_dim=24, n_fonts=n_fonts)
    B = 3
    P = tparams(cfg, F64)
    x = torch.tensor([40, 77, 40])
    font = torch.tensor([1, 0, 1]) if n_fonts else None
    tgt = torch.from_numpy(R.synth.hash_u8(941, (B, cfg.tokens))).double() / 255.0
    yo, cache = oracle.pixel_forward(P, x, font, cfg)
    _, duo = oracle.mse_loss_grad(cache["u"], tgt)
    Go = oracle.pixel_backward(P, cache, duo, cfg)
    y, u, G = _compose(P, x, font, cfg, lambda uu: oracle.mse_loss_grad(uu, tgt)[1])
    rel = lambda a, b: float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)              # noqa: E731
    assert rel(y, yo) <= 1e-12 and rel(u, cache["u"]) <= 1e-12
    assert set(G) == {k for k, _ in cfg.param_shapes()}
    for k, _ in cfg.param_shapes():
        assert rel(G[k].reshape(Go[k].shape), Go[k]) <= 1e-12, k


def test_a_every_backward_restatement_agrees_with_autograd_of_its_forward():
    gen = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=F64)                                      # noqa: E731
    rel = lambda a, b: float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)              # noqa: E731
    for d in (64, 192):
        rows = 11
        # head: u(h, g, b, w, bo) with upstream du
        h, g, b, w, bo, du = (t.requires_grad_() for t in (rn(rows, d), 1 + 0.3 * rn(d), rn(d), rn(d), rn(1), rn(rows)))
        _, u, _ = R.head(h, torch.zeros_like(h), g, b, w, bo)
        gh, gg, gb, gw, gbo = torch.autograd.grad(u, (h, g, b, w, bo), du.detach())
        dh, part = R.head_bwd(du.detach(), h.detach(), g.detach(), b.detach(), w.detach())
        for got, want in ((dh, gh), (part[0], gg), (part[1], gb), (part[2], gw), (part[3, :1], gbo)):
            assert rel(got, want) <= 1e-10
        assert float(part[3, 1:].abs().max()) == 0.0
        # LayerNorm with the residual
        x, dy, res = rn(rows, d).requires_grad_(), rn(rows, d), rn(rows, d)
        _, n = R.add_ln(x, None, None, g, b, rows, rows)
        gx, gg, gb = torch.autograd.grad(n, (x, g, b), dy)
        dh, part = R.ln_bwd(dy, x.detach(), g.detach(), res)
        for got, want in ((dh, res + gx), (part[0], gg), (part[1], gb)):
            assert rel(got, want) <= 1e-10
        # attention, two keys and one
        for Cn in (2, 1):
            B, T = 2, 5
            q, kv, dO = rn(B * T, d).requires_grad_(), rn(B, Cn, 2 * d).requires_grad_(), rn(B * T, d)
            gq, gkv = torch.autograd.grad(R.attn(q, kv, T), (q, kv), dO)
            dq, dkv = R.attn_bwd(dO, q.detach(), kv.detach(), T)
            assert rel(dq, gq) <= 1e-10 or (Cn == 1 and float(dq.abs().max()) == 0.0 and float(gq.abs().max()) < 1e-15)
            assert rel(dkv.reshape(B, 2, 2 * d)[:, :Cn], gkv) <= 1e-10
            assert Cn == 2 or float(dkv[:, 2 * d:].abs().max()) == 0.0
    # context gather
    I = R.ctx_inputs(7, 64)
    emb, femb = I["emb"].double().requires_grad_(), I["femb"].double().requires_grad_()
    ge, gf = torch.autograd.grad(R.ctx(emb, femb, I["x"], I["font"]), (emb, femb), I["dctx"].double())
    demb, dfont = R.ctx_bwd(I["dctx"].double(), I["x"], I["font"], I["vocab"], I["n_fonts"])
    assert torch.equal(demb, ge) and torch.equal(dfont, gf)
    assert float(demb[65].abs().max()) > 0 and float(demb[0].abs().max()) == 0 and float(dfont[2].abs().max()) == 0


# --------------------------------------------------------------------------------------------------------- (b), (c)
LN_FAULTS = ("unbiased", "no_eps")


def _yardstick(name, ref, bnd, got, limit=0.25):
    worst = 0.0
    for k in ref:
        r = R.ratio(got[k], ref[k], bnd[k])
        worst = max(worst, r)
        assert r <= limit, (name, k, r)
    return worst


def _fault(name, ref, bnd, got, keys=None):
    r = max(R.ratio(got[k], ref[k], bnd[k]) for k in (keys or ref))
    assert r >= 10.0, (name, r)
    return r


def _stale_target(c):
    """a row of the last trip that lies in no planted group (the groups repeat: a stale copy of one is its twin)"""
    r = c["rows"] - R.GROUP - 3
    return r if r >= c["stride"] else None


@pytest.mark.parametrize("B,tokens,d", R.fwd_cases())
def test_bc_forward_kernels_f32_within_a_quarter_and_faults_ten_times_over(B, tokens, d):
    worst = 0.0
    for is_bf16 in (False, True):
        cases = [("add_ln/" + m, R.add_ln_case(B, tokens, d, m, is_bf16), R.add_ln_run, R.add_ln_bounds) for m in ("pos", "add", "no_n")]
        cases += [("head/" + ls, R.head_case(B, tokens, d, ls, is_bf16), R.head_run, R.head_bounds) for ls in ("mse", "bce")]
        cases += [(f"attn/C{Cn}", R.attn_case(B, tokens, d, Cn, is_bf16), R.attn_run, R.attn_bounds) for Cn in (2, 1)]
        for name, c, run, bounds in cases:
            name = f"{name} {B}x{tokens}x{d} bf16={is_bf16}"
            ref = run(c, F64)
            bnd = bounds(c, ref)
            worst = max(worst, _yardstick(name, ref, bnd, run(c, F32)))
            if is_bf16:
                continue
            main = "n" if "n" in ref else "u" if "u" in ref else "o"
            if name.startswith(("add_ln/pos", "add_ln/add", "head")):
                for f in LN_FAULTS + (("dead_mean",) if d == 192 else ()):
                    _fault(name + " " + f, ref, bnd, run(c, F64, fault=f), [main])
            r = _stale_target(c)
            if r is not None and not name.startswith("add_ln/no_n") and not name.startswith("attn/C1"):
                _fault(name + " stale", ref, bnd, {main: R.stale_row(ref[main], r, c["stride"])}, [main])
    print(f"forward {B}x{tokens}x{d}: float32 restatement at most {worst:.3f} of a bound")


@pytest.mark.parametrize("B,tokens,d", R.bwd_cases())
def test_bc_backward_kernels_f32_within_a_quarter_and_faults_ten_times_over(B, tokens, d):
    worst = 0.0
    for is_bf16 in (False, True):
        for name, c, run, bounds in (("head_bwd", R.head_bwd_case(B, tokens, d, is_bf16), R.head_bwd_run, R.head_bwd_bounds),
                                     ("ln_bwd", R.ln_bwd_case(B, tokens, d, is_bf16), R.ln_bwd_run, R.ln_bwd_bounds)):
            name = f"{name} {B}x{tokens}x{d} bf16={is_bf16}"
            ref = run(c, F64)
            bnd = bounds(c, ref)
            worst = max(worst, _yardstick(name, ref, bnd, run(c, F32)))
            if is_bf16:
                continue
            for f in LN_FAULTS + (("dead_mean",) if d == 192 else ()):
                _fault(name + " " + f, ref, bnd, run(c, F64, fault=f), ["dh"])
            r = _stale_target(c)
            if r is not None:
                _fault(name + " stale", ref, bnd, {"dh": R.stale_row(ref["dh"], r, c["stride"])}, ["dh"])
            if c["rows"] >= R.BWD_WAVES:
                _fault(name + " wave", ref, bnd, run(c, F64, row_weight=R.wave_rows(c["rows"])), ["part"])
    print(f"backward {B}x{tokens}x{d}: float32 restatement at most {worst:.3f} of a bound")


@pytest.mark.parametrize("B,tokens,d,Cn", R.attn_bwd_cases())
def test_bc_attention_backward_f32_within_a_quarter_and_faults_ten_times_over(B, tokens, d, Cn):
    for is_bf16 in (False, True):
        c = R.attn_bwd_case(B, tokens, d, Cn, is_bf16)
        name = f"attn_bwd {B}x{tokens}x{d} C{Cn} bf16={is_bf16}"
        ref = R.attn_bwd_run(c, F64)
        bnd = R.attn_bwd_bounds(c, ref)
        worst = _yardstick(name, ref, bnd, R.attn_bwd_run(c, F32))
        if is_bf16:
            continue
        if Cn == 2:
            _fault(name + " dq_scale", ref, bnd, R.attn_bwd_run(c, F64, fault="dq_scale"), ["dq"])
            _fault(name + " swap_dv", ref, bnd, R.attn_bwd_run(c, F64, fault="swap_dv"), ["dkv"])
        if tokens >= R.BWD_WAVES:
            w = torch.ones(B * tokens, dtype=F64)
            w[R.BWD_WAVES - 1:R.attn_chunk(tokens):R.BWD_WAVES] = 0.0                               # sample 0, chunk 0, wave 15
            _fault(name + " wave", ref, bnd, R.attn_bwd_run(c, F64, row_weight=w), ["dkv"])
    print(f"{name}: float32 restatement at most {worst:.3f} of a bound")


def test_bc_context_gradient_bound():
    I = R.ctx_inputs(13, 192)
    ref = R.ctx_bwd(I["dctx"].double(), I["x"], I["font"], I["vocab"], I["n_fonts"])
    got = R.ctx_bwd(I["dctx"], I["x"], I["font"], I["vocab"], I["n_fonts"])
    bnd = R.bound_ctx_bwd(I["dctx"].double(), I["x"], I["font"], I["vocab"], I["n_fonts"])
    for g_, r_, b_ in zip(got, ref, bnd):
        assert R.ratio(g_, r_, b_) <= 0.25
    assert R.ratio(ref[0] * (1 + 1e-4), ref[0], bnd[0]) >= 10.0


def test_inputs_hold_the_planted_rows_where_the_trips_begin_and_end():
    assert R.anchors(3, R.FWD_STRIDE) == [0]
    assert R.anchors(21, R.FWD_STRIDE) == [0, 16]
    assert R.anchors(36936, R.FWD_STRIDE) == [0, 32768, 36931]                                    # 36936 / (8192 * 4) = 1.13: the second trip is rows 32768 ..
    assert R.anchors(69768, R.FWD_STRIDE) == [0, 32768, 65531, 65536, 69763]                      # 2.13 trips
    assert R.anchors(28728, R.BWD_STRIDE) == [0, 8192, 16379, 16384, 24571, 24576, 28723]         # 28728 / (512 * 16) = 3.5 trips
    I = R.ln_inputs(36936, 64, R.FWD_STRIDE, 4104)
    x = I["hin"] + I["add"]
    for a in I["anchors"]:
        assert torch.equal(x[a:a + 5], x[0:5]) and torch.equal(I["dy"][a:a + 5], I["dy"][0:5])
        assert torch.equal(I["pos"][torch.arange(a, a + 5) % 4104], I["pos"][0:5])
    assert I["pos_anchors"] == I["anchors"]
    assert float(x[1].std()) == 0.0 and abs(float(x[2].mean()) - 1000) < 1 and float(x[3].abs().max()) <= 1e-4
    assert float(x[4].abs().max()) >= 5e3 and float(x[4].abs().median()) < 1
    assert not torch.equal(x[7], x[7 + R.FWD_STRIDE])                                               # the fill does not repeat one stride on
    c = R.attn_case(9, 4104, 128, 2, False)
    s = torch.einsum("the,che->tch", c["q"][:5].double().reshape(5, 2, 64) * 0.125, c["kv"][0, :, :128].double().reshape(2, 2, 64))
    gaps = (s[:, 0] - s[:, 1])
    want = torch.tensor([[R.GAPS[(i + h) % 8] for h in range(2)] for i in range(5)], dtype=F64)
    assert float(gaps[0, 0]) == 0.0 and float((gaps - want).abs().max()) < 1e-4
    assert torch.equal(c["kv"][1, 0, :64], c["kv"][1, 1, :64]) and not torch.equal(c["kv"][0, 0, :64], c["kv"][0, 1, :64])


# --------------------------------------------------------------------------------------------------------- the entry points
def test_pixel_op_entries_refuse_bad_arguments_before_touching_a_pointer():
    from ai_font_renderer_amd import _lib
    lib = _lib.lib()
    fk = C.c_void_p(0x10000)                      # never dereferenced
    for rows in (1, 15, 16, 17, 8191, 8192, 8193, 10 ** 7):
        assert lib.afr_pixel_bwd_blocks(rows) == R.bwd_blocks(rows)
    for t in (1, 8, 255, 256, 257, 4096):
        assert lib.afr_pixel_attn_chunk(t) == R.attn_chunk(t)
    EI, EU = _lib.AFR_EINVAL, _lib.AFR_EUNSUPPORTED
    calls = {
        "add_ln": lambda dt=0, rows=8, d=64, h=fk: lib.afr_op_pixel_add_ln(dt, fk, h, None, fk, fk, fk, fk, rows, 8, d, 1e-5, None),
        "attn": lambda dt=0, rows=8, d=64, h=fk, heads=1, Cn=2: lib.afr_op_pixel_attn(dt, fk, fk, h, rows, 8, d, heads, Cn, None),
        "attn_bwd": lambda dt=0, rows=1, d=64, h=fk, heads=1, Cn=2: lib.afr_op_pixel_attn_bwd(dt, fk, fk, fk, h, fk, rows, 8, d, heads, Cn, None),
        "head": lambda dt=0, rows=8, d=64, h=fk, loss=0: lib.afr_op_pixel_head(dt, loss, fk, h, fk, fk, fk, fk, fk, fk, fk, rows, d, 1e-5, None),
        "head_bwd": lambda dt=0, rows=8, d=64, h=fk: lib.afr_op_pixel_head_bwd(dt, fk, fk, fk, fk, fk, h, None, fk, rows, d, 1e-5, None),
        "ln_bwd": lambda dt=0, rows=8, d=64, h=fk: lib.afr_op_pixel_ln_bwd(dt, fk, fk, fk, h, None, fk, rows, d, 1e-5, None),
        "ctx": lambda dt=0, rows=2, d=64, h=fk: lib.afr_op_pixel_ctx(dt, fk, fk, fk, fk, rows, d, 128, 2, h, fk, None),
        "ctx_bwd": lambda dt=0, rows=2, d=64, h=fk: lib.afr_op_pixel_ctx_bwd(fk, fk, fk, rows, d, 128, 2, h, fk, None),
    }
    for name, call in calls.items():
        if name != "ctx_bwd":
            assert call(dt=_lib.AFR_BF16X3) == EI and b"act_dtype" in lib.afr_last_error(), name
        assert call(rows=0) == EI and b">= 1" in lib.afr_last_error(), name
        for d in (0, 32, 100, 576, 1024):
            assert call(d=d) == EU and b"64 * heads" in lib.afr_last_error(), (name, d)
        assert call(h=None) == EI and (b"null" in lib.afr_last_error().lower() or b"required" in lib.afr_last_error()), name
    for name in ("attn", "attn_bwd"):
        assert calls[name](d=128, heads=1) == EU and b"64 * heads" in lib.afr_last_error()
        for Cn in (0, 3):
            assert calls[name](Cn=Cn) == EI and b"context tokens" in lib.afr_last_error()
    assert calls["head"](loss=2) == EI and b"loss kind" in lib.afr_last_error()
    assert lib.afr_op_pixel_add_ln(0, fk, fk, fk, None, fk, fk, fk, 8, 8, 64, 1e-5, None) == EI and b"exactly one" in lib.afr_last_error()
    assert lib.afr_op_pixel_add_ln(0, None, fk, None, None, fk, fk, fk, 8, 8, 64, 1e-5, None) == EI
