"""CPU: the checker of the glyph nets' first-layer kernels (tests/glyph_ref.py) is itself checked, and so is everything about the
afr_op_glyph_* entries that needs no device: (a) the fp64 restatements ARE torch's nn.Embedding / nn.Linear forward and autograd
backward -- summed over blocks and slabs, every route to dW1, db1, dEmb, dFont (widened slabs + post-pass, the fused backward's block
slabs without its rounding, the plain embedding backward) equals autograd's to 1e-12 relative; (b) the float32 orders the GPU tests
replay bit for bit stay inside their fp64 bounds; (c) at the case shapes at most 0.1 % of the ReLU gates sit closer to zero than the
bound of their pre-activation, from the reference inputs alone; (d) the getters answer what the checker's mirrors say; (e) every
refusal returns its code and message -- none of them launches anything (the pointers are not memory, so every call made here must
be one that is refused)."""
import ctypes as C

import pytest
import torch

from . import glyph_ref as R

F64 = torch.float64


def rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


# --------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("B,N1,vocab,n_fonts", [(200, 256, 142, 2), (65, 384, 100, 0), (1, 256, 16, 1), (130, 1024, 37, 3)])
def test_a_restatements_are_autograd(B, N1, vocab, n_fonts):
    E = 32
    t = R.make_tables(E, N1, vocab, n_fonts, 40)
    x, font = R.make_ids(B, vocab, n_fonts, 50)
    f = font if n_fonts > 0 else torch.zeros_like(x)
    emb = torch.nn.Embedding(vocab, E).double()
    fc1 = torch.nn.Linear(E, N1).double()
    with torch.no_grad():
        emb.weight.copy_(t["emb"]); fc1.weight.copy_(t["W1"]); fc1.bias.copy_(t["b1"])
    mods = [emb, fc1]
    h0 = emb(x)
    if n_fonts > 0:
        femb = torch.nn.Embedding(n_fonts, E).double()
        with torch.no_grad():
            femb.weight.copy_(t["femb"])
        mods.append(femb)
        h0 = h0 + femb(f)
    pre = fc1(h0)
    h1 = torch.relu(pre)
    g = R.make_d((B, N1), 60).double()
    (h1 * g).sum().backward()
    d1 = g * (pre.detach() > 0)
    # forward
    T, Tb = R.table_ref(t["emb"], t["femb"], t["W1"], n_fonts)
    pre_r, _, ref, _ = R.h1_ref(T, Tb, t["b1"], x, f, vocab, n_fonts)
    assert rel(pre_r, pre.detach()) <= 1e-12 and rel(ref, h1.detach()) <= 1e-12
    assert rel(R.embed_ref(t["emb"], t["femb"], x, f, n_fonts), h0.detach()) <= 1e-12
    want_tab = torch.cat([emb.weight.grad] + ([femb.weight.grad] if n_fonts > 0 else []))
    # route 1: the weight gradient against the widened operand in nslabs slabs of the batch, then the post-pass
    h0p = R.h0p_ref(t["emb"], t["femb"], x, f, vocab, n_fonts)
    assert torch.equal(h0p[:, E:].sum(1), torch.full((B,), 2.0 if n_fonts > 0 else 1.0, dtype=F64))
    cuts = [0, B // 3, B // 2, B]
    slabs = torch.stack([d1[a:b].t() @ h0p[a:b] for a, b in zip(cuts[:-1], cuts[1:])])
    dw1, _, part, _ = R.l1_bwd_ref(slabs, t["W1"], E, vocab, n_fonts)
    assert rel(dw1, fc1.weight.grad) <= 1e-12 and rel(part.sum(0), want_tab) <= 1e-12
    # route 2: the fused backward's block slabs, its rounding point switched off, at the kernel's own split
    split = R.fused_split(B, N1)
    blocks = R.fused_ref(d1, h0.detach(), t["W1"], x, f, vocab, n_fonts, split, rnd=None)
    nc = N1 // split
    dW = torch.zeros(N1, E, dtype=F64)
    db = torch.zeros(N1, dtype=F64)
    for i, b in enumerate(blocks):
        cs = i % split
        dW[cs * nc:(cs + 1) * nc] += b["dW1"]
        db[cs * nc:(cs + 1) * nc] += b["db1"]
    assert rel(dW, fc1.weight.grad) <= 1e-12 and rel(db, fc1.bias.grad) <= 1e-12
    assert rel(sum(b["dTab"] for b in blocks), want_tab) <= 1e-12
    # route 3: the plain embedding backward of dh0 = d1 . W1
    dh0 = d1 @ t["W1"].double()
    sl, _, _ = R.embed_bwd_ref(dh0, x, f, vocab, n_fonts)
    assert rel(sl.sum(0), want_tab) <= 1e-12


# --------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("B,E,vocab,n_fonts,kind", R.EMBED_BWD_CASES)
def test_b_embed_bwd_float32_order_is_inside_the_fp64_bound(B, E, vocab, n_fonts, kind):
    x, font = R.ids_for(B, vocab, n_fonts, 300, kind)
    xc, fc, _ = R.clamp_ids(x, font, vocab, n_fonts)
    d = R.make_d((B, E), 310)
    ref, bnd, used = R.embed_bwd_ref(d, xc, fc, vocab, n_fonts)
    got = R.embed_bwd_f32(d, xc, fc, vocab, n_fonts)
    assert R.ratio(got, ref, bnd) <= 1.0
    assert not bool(R.bits(got)[~used].any())
    assert used.sum(1).max() <= 2 * R.EMB_ROWS and ref.shape[0] == (B + 31) // 32


def test_b_fused_rounding_point_matters():
    """the block's own columns are what is rounded: rounding the unsplit dh0 instead misses the dTab bound of a split case"""
    B, N1, vocab, n_fonts = 65, 1024, 142, 2
    I = R.fused_inputs(B, N1, vocab, n_fonts, "dense", "spread")
    split = R.fused_split(B, N1)
    assert split == 4
    blocks = R.fused_ref(I["d1"], I["h0g"], I["W1"], I["xc"], I["fc"], vocab, n_fonts, split)
    print(f"partials within their float32 error of a bf16 rounding boundary: {sum(b['near'] for b in blocks)} of {B * 32 * split}")
    # a kernel that rounded a quarter of the UNSPLIT partial: wrong rounding point
    whole = R.fused_ref(I["d1"], I["h0g"], I["W1"], I["xc"], I["fc"], vocab, n_fonts, 1)
    worst = 0.0
    for rb in range(2):
        got = whole[rb]["dTab"] / 4
        for cs in range(split):
            worst = max(worst, R.ratio(got, blocks[rb * split + cs]["dTab"], blocks[rb * split + cs]["bT"]))
    assert worst > 10.0


# --------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("case", [c[:6] for c in R.COMBO_CASES], ids=str)
def test_c_relu_gates_near_zero_stay_under_the_cap(case):
    B, E, N1, vocab, n_fonts, kind = case
    t = R.make_tables(E, N1, vocab, n_fonts, 100)
    x, font = R.ids_for(B, vocab, n_fonts, 110, kind)
    xc, fc, _ = R.clamp_ids(x, font, vocab, n_fonts)
    T, Tb = R.table_ref(t["emb"], t["femb"], t["W1"], n_fonts)
    for xs, fs in ((xc, fc), R.combo_ids(vocab, n_fonts)):
        pre, bp, ref, _ = R.h1_ref(T, Tb, t["b1"], xs, fs, vocab, n_fonts)
        near = int((pre.abs() <= bp).sum())
        assert near <= 1e-3 * pre.numel(), (near, pre.numel())
        assert float(bp.max()) <= 1e-4 * float(pre.abs().max())              # the bound is not hollow: four digits of the largest output


# --------------------------------------------------------------------------------------------------------- (d)
def test_d_getters_answer_the_mirrors():
    from ai_font_renderer_amd import _lib
    lib = _lib.lib()
    for _, N1, E, vocab, n_fonts, _ in R.L1_BWD_CASES:
        assert lib.afr_glyph_k0(E, vocab, n_fonts) == R.k0_of(E, vocab, n_fonts)
        assert lib.afr_glyph_l1_bwd_blocks(N1) == (N1 + 7) // 8
    assert lib.afr_glyph_k0(32, 478, 2) == 512 and lib.afr_glyph_k0(32, 10, 2) == 48 and lib.afr_glyph_k0(32, 128, 2) == 168
    for B in (1, 32, 33, 257, 700):
        assert lib.afr_embed_bwd_blocks(B) == (B + 31) // 32
    splits = set()
    for B, N1, vocab, n_fonts, _, _ in R.FUSED_CASES:
        assert lib.afr_glyph_l1_bwd_fused_eligible(_lib.AFR_BF16, 32, N1, vocab, n_fonts) == 1
        s = lib.afr_glyph_l1_bwd_fused_split(B, N1)
        assert s == R.fused_split(B, N1) and s == {256: 2, 384: 1, 1024: 4}[N1]
        assert lib.afr_glyph_l1_bwd_fused_blocks(B, N1) == (B + 63) // 64 * s
        assert lib.afr_glyph_l1_bwd_fused_slab_floats(B, N1, vocab, n_fonts) == R.fused_slab_floats(B, N1, vocab, n_fonts)
        splits.add(s)
    assert splits == {1, 2, 4}
    assert lib.afr_glyph_l1_bwd_fused_split(8192, 1024) == 2 and lib.afr_glyph_l1_bwd_fused_split(64 * 200, 1024) == 1
    for args in ((_lib.AFR_F32, 32, 256, 128, 2), (_lib.AFR_BF16, 64, 256, 128, 2), (_lib.AFR_BF16, 32, 320, 128, 2), (_lib.AFR_BF16, 32, 128, 128, 2),
                 (_lib.AFR_BF16, 32, 1152, 128, 2), (_lib.AFR_BF16, 32, 256, 143, 2)):
        assert lib.afr_glyph_l1_bwd_fused_eligible(*args) == 0 and R.fused_eligible(*args[1:]) == (args[0] == _lib.AFR_F32)


# --------------------------------------------------------------------------------------------------------- (e)
def test_e_refusals_come_with_a_message_and_without_a_launch():
    from ai_font_renderer_amd import _lib
    lib = _lib.lib()
    EI, EU = _lib.AFR_EINVAL, _lib.AFR_EUNSUPPORTED
    fk = C.c_void_p(0x1000)                                   # not memory: a launch on it could not succeed
    err = lib.afr_last_error

    def embed(dt=0, emb=fk, femb=fk, x=fk, font=fk, B=4, E=32, vocab=128, nf=2, out=fk, er=fk):
        return lib.afr_op_glyph_embed(dt, emb, femb, x, font, B, E, vocab, nf, out, er, None)

    def combo(emb=fk, femb=fk, W1=fk, b1=fk, x=fk, font=fk, B=4, E=32, N1=256, vocab=128, nf=2, h1c=fk, ld1=256, h0c=fk, cidx=fk, w1t=None, er=fk):
        return lib.afr_op_glyph_combo(emb, femb, W1, b1, x, font, B, E, N1, vocab, nf, h1c, ld1, h0c, cidx, w1t, er, None)

    def post(slabs=fk, ns=2, stride=64 * 168, W1=fk, N1=64, E=32, vocab=128, nf=2, dw1=fk, part=fk):
        return lib.afr_op_glyph_l1_bwd(slabs, ns, stride, W1, N1, E, vocab, nf, dw1, part, None)

    def fused(d1=fk, h0=fk, ldh=168, rowmap=None, W1T=fk, x=fk, font=fk, B=64, N1=256, vocab=128, nf=2, slabs=fk):
        return lib.afr_op_glyph_l1_bwd_fused(d1, h0, ldh, rowmap, W1T, x, font, B, N1, vocab, nf, slabs, None)

    def ebwd(dt=0, d=fk, x=fk, font=fk, B=4, E=32, vocab=128, nf=2, slabs=fk):
        return lib.afr_op_glyph_embed_bwd(dt, d, x, font, B, E, vocab, nf, slabs, None)

    for call in (embed, combo, fused, ebwd):
        assert call(B=0) == EI and b"B = 0" in err()
        assert call(B=-3) == EI
        assert call(vocab=0) == EI and b"vocab" in err()
        assert call(nf=-1) == EI
    for call in (embed, ebwd):
        assert call(dt=2) == EI and b"act_dtype" in err()                  # AFR_BF16X3 is a plan mode, not an activation type
    for call in (embed, combo, post, ebwd):
        assert call(E=20) == EU and b"multiple of 8" in err()
        assert call(E=0) == EU
    for call in (combo, post, fused):
        assert call(N1=60) == EU and b"multiple of 8" in err()
    # the fold's post-pass: K0 <= 512, E <= 128
    assert post(vocab=479) == EU and b"K0 = 520" in err()
    assert post(E=136, vocab=16) == EU and b"E = 136" in err()
    # the combination kernel's 48 KiB of staging
    assert combo(E=48) == EU and b"48 KiB" in err()
    assert combo(ld1=248) == EI and b"ld1" in err()
    # the fused backward: only where eligible
    for kw in (dict(N1=128), dict(N1=320), dict(N1=1152), dict(vocab=143), dict(vocab=144, nf=1)):
        assert fused(**kw) == EU and b"fused backward" in err()
    assert fused(ldh=24) == EI and b"ldh" in err() and fused(ldh=36) == EI
    # the plain embedding backward: the table's accumulator must fit 160 KiB of LDS
    assert ebwd(E=128, vocab=600) == EU and b"160 KiB" in err()
    assert ebwd(E=32, vocab=1300, nf=0) == EU and b"160 KiB" in err()
    # the post-pass: slabs
    assert post(ns=0) == EI and b"nslabs" in err()
    assert post(stride=64 * 168 + 2) == EI and post(stride=64 * 168 - 4) == EI and b"slab_stride" in err()
    assert post(slabs=C.c_void_p(0x1004)) == EI and b"16-byte" in err()
    # null required pointers (font, w1t and the row map are optional; femb only without fonts)
    for call, names in ((embed, ("emb", "femb", "x", "out", "er")),
                        (combo, ("emb", "femb", "W1", "b1", "x", "h1c", "h0c", "cidx", "er")), (post, ("slabs", "W1", "dw1", "part")),
                        (fused, ("d1", "h0", "W1T", "x", "slabs")), (ebwd, ("d", "x", "slabs"))):
        for n in names:
            assert call(**{n: None}) == EI and b"null" in err(), (call.__name__, n)
    assert fused(d1=C.c_void_p(0x1008)) == EI and b"16-byte" in err()


def test_e_a_plan_whose_embedding_backward_cannot_fit_is_refused_at_creation():
    """vocab x embed_dim beyond what glyph_embed_bwd_kernel keeps in LDS used to surface as a launch error in the middle of a step"""
    from ai_font_renderer_amd import _lib, config
    from ai_font_renderer_amd.engine import make_afr_config
    lib = _lib.lib()
    plan = C.c_void_p()
    for cfg in (config.GlyphConfig(vocab=1300, hidden=(64,)), config.GlyphConfig(vocab=600, embed_dim=136, hidden=(64,)),
                config.GlyphConfig(vocab=1300, hidden=())):
        c = make_afr_config(cfg, "f32", 8)
        assert lib.afr_plan_create(C.byref(c), C.byref(plan)) == _lib.AFR_EUNSUPPORTED
        assert b"160 KiB" in lib.afr_last_error()
    for cfg in (config.GlyphConfig(vocab=1200, hidden=(64,)), config.GlyphConfig(vocab=478, hidden=(64,)), config.GlyphConfig(vocab=4000, embed_dim=8, hidden=())):
        c = make_afr_config(cfg, "f32", 8)
        assert lib.afr_plan_create(C.byref(c), C.byref(plan)) == 0, lib.afr_last_error()
        lib.afr_plan_destroy(plan)
