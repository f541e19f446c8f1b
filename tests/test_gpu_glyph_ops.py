"""GPU: the glyph nets' first-layer kernels (csrc/elementwise.hip glyph_embed / glyph_combo / glyph_l1_bwd / glyph_embed_bwd,
csrc/gemm.hip glyph_l1_bwd_fused), ONE launch each through the afr_op_glyph_* entries, every output element against the fp64
restatement of tests/glyph_ref.py under its derived bound, or bit for bit where the kernel's arithmetic is one rounding or a stated
float32 order.  (The table + gather pair of the folded forward, glyph_table / glyph_l1_fwd, and the fused step are tested in
tests/test_gpu_glyph_step_ops.py.)  The shapes are the smallest at which each mechanism can fail
(tests/glyph_ref.py *_CASES): combination counts that end a group of four early (101, 111) or fill it, fc1 widths that end a 256-row
chunk early, E at the combination kernel's staging limit (40) and at 8, K0 from 48 to the post-pass's limit of 512 (8, 3 and 1 lane
groups), row blocks of the fused backward that are ragged (1, 63, 65, 200 glyphs) and full (64) in both h0 forms, its unsplit
(N1 = 384) and split (256: 2, 1024: 4 column ranges) grids, embedding-backward blocks of 1, 32 + 1 and many rows, tables up to 82 KB
of LDS; codes spread over the whole vocabulary with repeats, codes 0 and vocab - 1, one-code batches, font = NULL.  Besides the
error, every case checks: output buffers pre-filled with NaN (a sentinel for int32) hold none afterwards and their guard bands of
256 bytes on both sides keep their bits (tests/op_harness.py); columns of h1c between N1 and ld1 keep their fill; a second launch
repeats the first bit for bit; in-range indices leave the error word 0; out-of-range ones set bit 0 in the forward kernels, and in
every kernel give the outputs of the clamped indices; table rows no glyph of a block used are +0 in its slab.

Every case prints its largest error as a fraction of the bound (pytest -s).  Measured on MI355X, the largest per output over all
cases:
    embed          bit for bit (float32 and bf16), as are h0c, cidx and w1t of the combination kernel
    combo          h1c 0.990 (the rounding to bf16 is the 2^-8 |ref| term of the bound itself); no ReLU gate differs from fp64's
    l1_bwd         dw1 0.512, dtab_part 0.256
    l1_bwd_fused   per block dW1 0.021, db1 0.003, dTab at most 0.17 (0.054 against the bound widened by one bf16 ulp for every
                   partial that glyph_ref.fused_ref counts as near a rounding boundary; at most a third of that bound is the
                   widening); the fp64 sum of all slabs against the unsplit, unrounded dTab 0.892
    embed_bwd      bit for bit the float32 row-order sum; against fp64 0.077"""
import ctypes as C
import functools

import pytest
import torch

from ai_font_renderer_amd import _lib
from . import glyph_ref as R
from .glyph_harness import Tables, check_h1 as _check_h1, ids_dev as _ids
from .gpu_util import dev, ptr, stream
from .op_harness import Outs, bits, dt, judge, same, tt, twice

pytestmark = pytest.mark.gpu
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


# ------------------------------------------------------------------------------------------------------------------ launches
def run_embed(T, x, font, is_bf16):
    B = x.shape[0]
    xd, fd = _ids(x, font)
    o = Outs()
    po = o.new("out", (B, T.E), tt(is_bf16))
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().afr_op_glyph_embed(dt(is_bf16), T.p("emb"), T.p("femb"), ptr(xd), ptr(fd), B, T.E, T.vocab, T.n_fonts, po, ptr(err), stream()))
    return dict(o.finish(), err=int(err.cpu()))


def run_combo(T, x, font, ld1, with_w1t=True):
    B, nco = x.shape[0], T.vocab * max(T.n_fonts, 1)
    xd, fd = _ids(x, font)
    o = Outs()
    p1, p0, pc = o.new("h1c", (nco, ld1), BF16), o.new("h0c", (nco, T.E), BF16), o.new("cidx", B, torch.int32)
    pw = o.new("w1t", (T.E, T.N1), BF16) if with_w1t else C.c_void_p(0)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().afr_op_glyph_combo(T.p("emb"), T.p("femb"), T.p("W1"), T.p("b1"), ptr(xd), ptr(fd), B, T.E, T.N1, T.vocab, T.n_fonts, p1, ld1,
                                             p0, pc, pw, ptr(err), stream()))
    # h1c keeps its fill between N1 and ld1 (test_combo asserts that, and that no NaN is left below N1)
    return dict(o.finish(may_keep_fill=("h1c",) if ld1 > T.N1 else ()), err=int(err.cpu()))


def run_l1_bwd(slabs_d, nslabs, stride, W1d, N1, E, vocab, n_fonts):
    nb, R_ = (N1 + 7) // 8, vocab + n_fonts
    o = Outs()
    pd, pp = o.new("dw1", (N1, E), F32), o.new("part", (nb, R_, E), F32)
    _lib.check(_lib.lib().afr_op_glyph_l1_bwd(ptr(slabs_d), nslabs, stride, ptr(W1d), N1, E, vocab, n_fonts, pd, pp, stream()))
    return o.finish()


def run_fused(I, B, N1, vocab, n_fonts, x=None, font="same"):
    lib = _lib.lib()
    nb, fl = lib.afr_glyph_l1_bwd_fused_blocks(B, N1), lib.afr_glyph_l1_bwd_fused_slab_floats(B, N1, vocab, n_fonts)
    xd, fd = _ids(I["x"] if x is None else x, I["font"] if isinstance(font, str) else font)
    d1, h0, w1t = dev(I["d1"], BF16), dev(I["h0"], BF16), dev(I["W1"].t().contiguous(), BF16)
    rm = dev(I["rowmap"]) if I["rowmap"] is not None else None
    o = Outs()
    ps = o.new("slabs", (nb, fl), F32)
    _lib.check(lib.afr_op_glyph_l1_bwd_fused(ptr(d1), ptr(h0), I["ldh"], ptr(rm), ptr(w1t), ptr(xd), ptr(fd), B, N1, vocab, n_fonts, ps, stream()))
    return o.finish()["slabs"]


def run_embed_bwd(d, x, font, vocab, n_fonts, is_bf16):
    B, E = d.shape
    nb = _lib.lib().afr_embed_bwd_blocks(B)
    xd, fd = _ids(x, font)
    dd = dev(d, tt(is_bf16))
    o = Outs()
    ps = o.new("slabs", (nb, vocab + n_fonts, E), F32)
    _lib.check(_lib.lib().afr_op_glyph_embed_bwd(dt(is_bf16), ptr(dd), ptr(xd), ptr(fd), B, E, vocab, n_fonts, ps, stream()))
    return o.finish()["slabs"]


# ------------------------------------------------------------------------------------------------------------------ embed
def _embed_bits(T, xc, fc, is_bf16):
    v = R.embed_ref(T.t["emb"], T.t["femb"], xc, fc, T.n_fonts, F32)            # one float32 add: the same bits in torch
    return v.to(BF16) if is_bf16 else v


def _bf(cases):
    return [pytest.param(*c, bf, id="-".join(str(v) for v in c) + ("-bf16" if bf else "-f32")) for c in cases for bf in (False, True)]


@pytest.mark.parametrize("B,E,vocab,n_fonts,kind,is_bf16", _bf(R.EMBED_CASES))
def test_embed(B, E, vocab, n_fonts, kind, is_bf16):
    T = Tables(E, 8, vocab, n_fonts, 100)
    x, font = R.ids_for(B, vocab, n_fonts, 110, kind)
    xc, fc, _ = R.clamp_ids(x, font, vocab, n_fonts)
    a = twice(lambda: run_embed(T, x, font, is_bf16))
    assert a["err"] == 0
    assert torch.equal(bits(a["out"]), bits(_embed_bits(T, xc, fc, is_bf16))), "embed is not emb[x] + femb[f] bit for bit"
    print(f"embed {B}x{E} vocab {vocab} fonts {n_fonts} {kind}: bit for bit")
    if B >= 3:                                                    # out-of-range indices: flagged, and the outputs of the clamped ones
        xb, fb = R.bad_ids(B, vocab, n_fonts, x, font)
        xbc, fbc, flag = R.clamp_ids(xb, fb, vocab, n_fonts)
        bad = run_embed(T, xb, fb, is_bf16)
        assert flag and bad["err"] & 1
        assert torch.equal(bits(bad["out"]), bits(_embed_bits(T, xbc, fbc, is_bf16)))


# ------------------------------------------------------------------------------------------------------------------ h1 reference
@functools.lru_cache(maxsize=4)
def _fwd_reference(E, N1, vocab, n_fonts):
    T = Tables(E, N1, vocab, n_fonts, 100)
    Tr, Tb = R.table_ref(T.t["emb"], T.t["femb"], T.t["W1"], n_fonts)
    return T, Tr, Tb


# ------------------------------------------------------------------------------------------------------------------ combination table
@pytest.mark.parametrize("B,E,N1,vocab,n_fonts,kind,pad", R.COMBO_CASES, ids=lambda v: str(v))
def test_combo(B, E, N1, vocab, n_fonts, kind, pad):
    name = f"combo {B}x{E}->{N1} vocab {vocab} fonts {n_fonts} {kind} ld1 {N1 + pad}"
    T, Tr, Tb = _fwd_reference(E, N1, vocab, n_fonts)
    x, font = R.ids_for(B, vocab, n_fonts, 110, kind)
    xc, fc, _ = R.clamp_ids(x, font, vocab, n_fonts)
    ld1, nf = N1 + pad, max(n_fonts, 1)
    a = twice(lambda: run_combo(T, x, font, ld1))
    assert a["err"] == 0
    assert torch.equal(a["cidx"].long(), xc * nf + fc), "cidx is not x max(n_fonts, 1) + f"
    cx, cf = R.combo_ids(vocab, n_fonts)
    assert torch.equal(bits(a["h0c"]), bits(_embed_bits(T, cx, cf, True))), "h0c is not bf16(emb + femb)"
    assert torch.equal(bits(a["w1t"]), bits(T.t["W1"].to(BF16).t().contiguous())), "w1t is not bf16(W1) transposed"
    if pad:
        fill = bits(torch.full((1,), float("nan"), dtype=BF16))
        assert bool((bits(a["h1c"][:, N1:]) == fill).all()), "h1c: bytes between N1 and ld1 were written"
    h1c = a["h1c"][:, :N1].contiguous()
    assert not bool(torch.isnan(h1c.float()).any())
    h1r, flips = _check_h1(name, h1c, Tr, Tb, T.t["b1"], cx, cf, vocab, n_fonts, True)
    same(dict(a, w1t=0), dict(run_combo(T, x, font, ld1, with_w1t=False), w1t=0), "without w1t")
    judge(name, dict(h1c=h1r))
    print(f"    gates that differ from fp64's: {flips} of {h1c.numel()}")
    if B >= 3:
        xb, fb = R.bad_ids(B, vocab, n_fonts, x, font)
        xbc, fbc, flag = R.clamp_ids(xb, fb, vocab, n_fonts)
        bad = run_combo(T, xb, fb, ld1)
        assert flag and bad["err"] & 1
        assert torch.equal(bad["cidx"].long(), xbc * nf + fbc)
        same(dict(bad, err=0, cidx=0), dict(a, cidx=0), "out-of-range indices")


# ------------------------------------------------------------------------------------------------------------------ post-pass
@pytest.mark.parametrize("nslabs,N1,E,vocab,n_fonts,gap", R.L1_BWD_CASES, ids=lambda v: str(v))
def test_l1_bwd_post_pass(nslabs, N1, E, vocab, n_fonts, gap):
    K0 = R.k0_of(E, vocab, n_fonts)
    stride = N1 * K0 + gap
    W1 = R.make_tables(E, N1, vocab, n_fonts, 400)["W1"]
    sl = torch.full((nslabs, stride), float("nan"), dtype=F32)            # the space between two slabs is never read
    sl[:, :N1 * K0] = R.make_d((nslabs, N1 * K0), 410)
    sd, Wd = dev(sl), dev(W1)
    a = twice(lambda: run_l1_bwd(sd, nslabs, stride, Wd, N1, E, vocab, n_fonts))
    dw1, bw, part, bp = R.l1_bwd_ref(sl[:, :N1 * K0].reshape(nslabs, N1, K0), W1, E, vocab, n_fonts)
    judge(f"l1_bwd {nslabs} slabs {N1}x{K0} (E {E}) stride +{gap}", dict(dw1=R.ratio(a["dw1"], dw1, bw), dtab_part=R.ratio(a["part"], part, bp)))


# ------------------------------------------------------------------------------------------------------------------ fused backward
def _check_fused(name, slabs, I, B, N1, vocab, n_fonts):
    lib = _lib.lib()
    split = lib.afr_glyph_l1_bwd_fused_split(B, N1)
    nc, R_ = N1 // split, vocab + n_fonts
    dW, db, dT = R.split_fused_slabs(slabs, nc, R_)
    blocks = R.fused_ref(I["d1"], I["h0g"], I["W1"], I["xc"], I["fc"], vocab, n_fonts, split)
    assert len(blocks) == slabs.shape[0]
    worst = dict(dW1=0.0, db1=0.0, dTab=0.0)
    totT, boundT = torch.zeros(R_, 32, dtype=F64), torch.zeros(R_, 32, dtype=F64)
    for i, blk in enumerate(blocks):
        worst["dW1"] = max(worst["dW1"], R.ratio(dW[i], blk["dW1"], blk["bW"]))
        worst["db1"] = max(worst["db1"], R.ratio(db[i], blk["db1"], blk["bb"]))
        worst["dTab"] = max(worst["dTab"], R.ratio(dT[i], blk["dTab"], blk["bT"]))
        assert not bool(bits(dT[i])[~blk["used"]].any()), f"{name}: block {i}: a table row no glyph of the block used is not +0"
        totT += dT[i].double()
        boundT += blk["bT"]
    # the fp64 sum of all slabs against the unsplit, unrounded gradient, under the sum of the block bounds
    whole = R.fused_ref(I["d1"], I["h0g"], I["W1"], I["xc"], I["fc"], vocab, n_fonts, 1, rnd=None)
    worst["dTab total"] = R.ratio(totT, sum(w["dTab"] for w in whole), boundT)
    judge(name, worst)
    print(f"    split {split}, blocks {len(blocks)}, partials near a bf16 rounding boundary: {sum(b['near'] for b in blocks)}")
    return split


@pytest.mark.parametrize("B,N1,vocab,n_fonts,form,kind", R.FUSED_CASES, ids=lambda v: str(v))
def test_l1_bwd_fused(B, N1, vocab, n_fonts, form, kind):
    I = R.fused_inputs(B, N1, vocab, n_fonts, form, kind)
    a = twice(lambda: run_fused(I, B, N1, vocab, n_fonts))
    split = _check_fused(f"l1_bwd_fused {B}x{N1} vocab {vocab} fonts {n_fonts} {form} {kind}", a, I, B, N1, vocab, n_fonts)
    assert split == {256: 2, 384: 1, 1024: 4}[N1]


def test_l1_bwd_fused_cases_cover_both_grids_and_forms():
    lib = _lib.lib()
    splits = {lib.afr_glyph_l1_bwd_fused_split(B, N1) for B, N1, *_ in R.FUSED_CASES}
    assert 1 in splits and max(splits) > 1
    for form in ("dense", "combo"):
        assert any(c[4] == form and c[0] % 64 == 0 for c in R.FUSED_CASES) and any(c[4] == form and c[0] % 64 for c in R.FUSED_CASES)
    assert {c[0] for c in R.FUSED_CASES} == {1, 63, 64, 65, 200} and {c[1] for c in R.FUSED_CASES} == {256, 384, 1024}
    assert {c[2:4] for c in R.FUSED_CASES} == {(142, 2), (16, 1), (128, 2), (100, 0)}


@pytest.mark.parametrize("form", ["dense", "combo"])
def test_l1_bwd_fused_clamps_without_flagging(form):
    B, N1, vocab, n_fonts = 65, 256, 128, 2
    I = R.fused_inputs(B, N1, vocab, n_fonts, form, "spread")
    xb, fb = R.bad_ids(B, vocab, n_fonts, I["xc"], I["fc"])
    xbc, fbc, flag = R.clamp_ids(xb, fb, vocab, n_fonts)
    assert flag
    # the h0 rows stay those of the forward's (clamped) indices; only the one-hot rows move
    got = run_fused(I, B, N1, vocab, n_fonts, x=xb, font=fb)
    want = run_fused(I, B, N1, vocab, n_fonts, x=xbc, font=fbc)
    assert torch.equal(bits(got), bits(want))
    _check_fused(f"l1_bwd_fused {form} clamped", got, dict(I, xc=xbc, fc=fbc), B, N1, vocab, n_fonts)


# ------------------------------------------------------------------------------------------------------------------ embedding backward
@pytest.mark.parametrize("B,E,vocab,n_fonts,kind,is_bf16", _bf(R.EMBED_BWD_CASES))
def test_embed_bwd(B, E, vocab, n_fonts, kind, is_bf16):
    x, font = R.ids_for(B, vocab, n_fonts, 300, kind)
    xc, fc, _ = R.clamp_ids(x, font, vocab, n_fonts)
    d = R.make_d((B, E), 310, round_bf16=is_bf16)
    a = twice(lambda: run_embed_bwd(d, x, font, vocab, n_fonts, is_bf16))
    assert torch.equal(bits(a), bits(R.embed_bwd_f32(d, xc, fc, vocab, n_fonts))), "a slab is not the float32 sum of its rows in order"
    ref, bnd, used = R.embed_bwd_ref(d, xc, fc, vocab, n_fonts)
    assert not bool(bits(a)[~used].any()), "a table row no glyph of the block used is not +0"
    judge(f"embed_bwd {B}x{E} vocab {vocab} fonts {n_fonts} {kind} {'bf16' if is_bf16 else 'f32'}", dict(slabs=R.ratio(a, ref, bnd)))
    if B >= 3:                                                    # clamped, not flagged (there is no error word)
        xb, fb = R.bad_ids(B, vocab, n_fonts, x, font)
        xbc, fbc, _ = R.clamp_ids(xb, fb, vocab, n_fonts)
        assert torch.equal(bits(run_embed_bwd(d, xb, fb, vocab, n_fonts, is_bf16)), bits(R.embed_bwd_f32(d, xbc, fbc, vocab, n_fonts)))
