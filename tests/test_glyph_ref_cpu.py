"""CPU: the checker of the glyph nets' first-layer kernels (tests/glyph_ref.py) is itself checked, and so is everything about the
afr_op_glyph_* entries that needs no device: (a) the fp64 restatements ARE torch's nn.Embedding / nn.Linear forward and autograd
backward -- summed over blocks and slabs, every route to dW1, db1, dEmb, dFont (widened slabs + post-pass, the fused backward's block
slabs without its rounding, the plain embedding backward) equals autograd's to 1e-12 relative; (b) the float32 orders the GPU tests
replay bit for bit stay inside their fp64 bounds; (c) at the case shapes at most 0.1 % of the ReLU gates sit closer to zero than the
bound of their pre-activation, from the reference inputs alone; (d) the getters answer what the checker's mirrors say; (e) every
refusal returns its code and message -- none of them launches anything (the pointers are not memory, so every call made here must
be one that is refused).  For the fused step (step_ref, afr_op_glyph1_step) and the entries beside it: (f) the unrounded block
references of the kernel's own split sum to autograd's gradients and loss of the whole net to 1e-12; (g) on every case's final inputs no
ReLU or clamp gate is within 8 x / 4 x its bound of its threshold, and the planted columns sit on the clamp's edges exactly; (h) six
planted faults each break a bound, in float32 and in bf16; (i) getters and mirrors agree; (j) the refusals of the three entries; (k) step_model, the a-priori distance
of the kernel's arithmetic from the unrounded model: the rounded references' sum lies within it, planted faults' sums do not."""
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
@pytest.mark.parametrize("case", [c[:6] for c in R.COMBO_CASES] + R.L1_FWD_CASES, ids=str)
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


# --------------------------------------------------------------------------------------------------------- the fused step's checker
def _step(case, is_bf16, loss, **kw):
    B, E, N1, P, vocab, n_fonts = case
    I = R.step_inputs(case, is_bf16)
    k, rows, table = R.step_target_forms(B, P)
    cs = R.g1_colsplit(is_bf16, B, P)
    return I, k, rows, table, cs, R.step_ref(I, case, is_bf16, loss, cs, R.target_values(k), B * P + 7, **kw)


@pytest.mark.parametrize("case,loss", [((130, 64, 192, 128, 100, 3), "mse"), ((65, 32, 64, 192, 262, 2), "bce")])
def test_f_step_ref_unrounded_is_autograd(case, loss):
    """Embedding (+ font) -> Linear -> ReLU -> Linear -> clamp + MSE / BCE with logits, mean_elems != B P: the block references of the
    kernel's own split, summed, are autograd's gradients"""
    B, E, N1, P, vocab, n_fonts = case
    for is_bf16 in (False, True):
        I, k, _, _, cs, ref = _step(case, is_bf16, loss, rnd=None)
        assert cs > 1
        want, L = R.step_autograd(I, case, loss, R.target_values(k), B * P + 7)
        got = R.step_total(ref, case)
        for name in want:
            assert rel(got[name], want[name]) <= 1e-12, name
        assert abs(ref["loss"] - L) <= 1e-12 * abs(L)


@pytest.mark.parametrize("case", R.STEP_CASES, ids=str)
def test_g_no_gate_of_the_fused_step_is_left_to_rounding(case):
    B, E, N1, P, vocab, n_fonts = case
    for is_bf16 in (False, True):
        I, _, _, _, _, ref = _step(case, is_bf16, "mse")
        assert I["steps"][0] <= 2 and I["steps"][1] <= 15, I["steps"]
        assert bool((ref["pre"].abs() > 8 * ref["bpre"]).all())
        p0, p1 = I["planted"]
        keep = torch.ones(P, dtype=torch.bool)
        keep[[p0, p1]] = False
        u, bu = ref["u"][:, keep], ref["bu"][:, keep]
        for edge in (0.0, 1.0 + (R.UB if is_bf16 else 0.0)):
            assert bool(((u - edge).abs() > 4 * bu).all()), edge
        # the planted columns sit on the inclusive clamp's edges, exactly, and their gates are open
        assert bool((ref["u"][:, p0] == 1.0).all()) and bool((ref["u"][:, p1] == 0.0).all())
        assert 0.4 <= float((ref["pre"] > 0).double().mean()) <= 0.6
        inside = float(((ref["u"] >= 0) & (ref["u"] <= 1)).double().mean())
        assert 0.7 <= inside <= 0.97, inside
        print(f"{case} {'bf16' if is_bf16 else 'f32'}: b1 / b2 steps {I['steps']}, u inside [0, 1] {inside:.3f}, near " +
              ", ".join(f"{k} {v:.4f}" for k, v in ref["near"].items()))
        assert ref["near"].get("h1", 0.0) <= 0.02


STEP_FAULTS = [("dead_rows", (95, 32, 256, 256, 128, 0), "bce"), ("all_cols", (95, 32, 256, 256, 128, 0), "mse"), ("exclusive", (130, 64, 192, 128, 100, 3), "mse"),
               ("font_row", (200, 32, 128, 256, 37, 3), "mse"), ("row_map", (95, 32, 256, 256, 128, 0), "bce"), ("unsplit_round", (200, 32, 128, 256, 37, 3), "mse")]


@pytest.mark.parametrize("fault,case,loss", STEP_FAULTS, ids=lambda v: str(v))
def test_h_a_planted_fault_of_the_fused_step_breaks_a_bound(fault, case, loss):
    """one fault at a time in what a kernel could leave: some output exceeds its bound, in float32 and in bf16 (the rounding point: bf16)"""
    B, E, N1, P, vocab, n_fonts = case
    for is_bf16 in ((True,) if fault == "unsplit_round" else (False, True)):
        I, k, rows, table, cs, ref = _step(case, is_bf16, loss)
        if fault == "row_map":            # the targets of row b of the table instead of row rows[b]
            got = R.step_ref(I, case, is_bf16, loss, cs, R.target_values(table[:B]), B * P + 7)
        else:
            got = R.step_ref(I, case, is_bf16, loss, cs, R.target_values(k), B * P + 7, fault=fault)
        ratios = {n: R.ratio(got[n], ref[n], ref["b" + n]) for n in ("dW2", "db2", "dW1", "db1", "dTab")}
        ratios["loss"] = abs(got["loss"] - ref["loss"]) / ref["bloss"]
        print(f"{fault} {case} {'bf16' if is_bf16 else 'f32'}: " + ", ".join(f"{n} {v:.3g}" for n, v in ratios.items()))
        assert max(ratios.values()) > 1.0
        if fault == "exclusive":          # seen at the planted columns: db2 of the column whose u is exactly 1
            bad = ((got["db2"] - ref["db2"]).abs() > ref["bdb2"]).reshape(-1, P)            # [row block][column]
            assert all(bool(bad[:, p].any()) for p in I["planted"])                        # u exactly 1, and u exactly 0


def test_i_fused_step_getters_answer_the_mirrors():
    from ai_font_renderer_amd import _lib
    lib = _lib.lib()
    for bf, dtype in ((False, _lib.AFR_F32), (True, _lib.AFR_BF16)):
        assert lib.afr_glyph1_rows(dtype) == R.G1_ROWS[bf]
        for B in (1, 16, 17, 64, 65, 95, 1024, 1025, 2048, 4096, 4097, 8256, 16385):
            for P in (64, 128, 192, 256):
                assert lib.afr_glyph1_colsplit(dtype, B, P) == R.g1_colsplit(bf, B, P), (bf, B, P)
                assert lib.afr_glyph1_blocks(dtype, B, P) == R.g1_blocks(bf, B, P)
    assert [lib.afr_glyph1_colsplit(_lib.AFR_F32, B, 256) for B in (95, 1024, 1025, 2048, 2049)] == [4, 4, 2, 2, 1]
    assert [lib.afr_glyph1_colsplit(_lib.AFR_BF16, B, 64) for B in (1, 8192, 8256)] == [2, 2, 1]
    for case in R.STEP_CASES:
        assert lib.afr_glyph1_eligible(*case[1:]) == 1 and R.g1_eligible(*case[1:])
    for args in ((16, 64, 64, 5, 0), (96, 64, 64, 5, 0), (32, 96, 64, 5, 0), (32, 320, 64, 5, 0), (32, 64, 32, 5, 0), (32, 64, 320, 5, 0), (32, 64, 64, 263, 2),
                 (32, 64, 64, 265, 0)):
        assert lib.afr_glyph1_eligible(*args) == 0 and not R.g1_eligible(*args), args
    assert lib.afr_glyph1_eligible(64, 256, 256, 262, 2) == 1


def test_j_refusals_of_the_step_forward_and_transpose_entries():
    from ai_font_renderer_amd import _lib
    lib = _lib.lib()
    EI, EU = _lib.AFR_EINVAL, _lib.AFR_EUNSUPPORTED
    fk = C.c_void_p(0x1000)                                   # not memory: a launch on it could not succeed
    err = lib.afr_last_error

    def fwd(dt=0, emb=fk, femb=fk, W1=fk, b1=fk, x=fk, font=fk, B=4, E=32, N1=64, vocab=128, nf=2, table=fk, h0p=fk, h1=fk, w1t=None, er=fk):
        return lib.afr_op_glyph_l1_fwd(dt, emb, femb, W1, b1, x, font, B, E, N1, vocab, nf, table, h0p, h1, w1t, er, None)

    lay0 = dict(emb=0, font=4096, w1=4160, b1=6208, w2=6272, b2=10368, total=10432)      # vocab 128, 2 fonts, 32 -> 64 -> 64

    def step(dt=1, loss=0, emb=fk, femb=fk, W1=fk, b1=fk, W2=fk, b2=fk, W1T=fk, W2T=fk, x=fk, font=fk, target=fk, tdt=0, rows=None, B=4, E=32, N1=64,
             P=64, vocab=128, nf=2, mean=256, slabs=fk, lay=lay0, accum=fk, scratch=fk, er=fk):
        la = _lib.AfrGlyph1Layout(*[lay[n] for n in ("emb", "font", "w1", "b1", "w2", "b2", "total")]) if lay is not None else None
        return lib.afr_op_glyph1_step(dt, loss, emb, femb, W1, b1, W2, b2, W1T, W2T, x, font, target, tdt, rows, B, E, N1, P, vocab, nf, mean, slabs,
                                      C.byref(la) if la is not None else None, accum, scratch, er, None)

    def tr(W=fk, WT=fk, N=8, K=8):
        return lib.afr_op_transpose_bf16(W, WT, N, K, None)

    for call in (fwd, step):
        assert call(B=0) == EI and b"B = 0" in err()
        assert call(vocab=0) == EI and b"vocab" in err()
        assert call(nf=-1) == EI
    # the folded forward: the plan's fold condition
    assert fwd(dt=2) == EI and b"act_dtype" in err()
    assert fwd(E=20) == EU and b"multiple of 8" in err() and fwd(N1=60) == EU and b"multiple of 8" in err()
    assert fwd(vocab=479) == EU and b"K0 = 520" in err()
    assert fwd(E=136, vocab=16) == EU and b"E = 136" in err()
    for n in ("emb", "femb", "W1", "b1", "x", "table", "h0p", "h1", "er"):
        assert fwd(**{n: None}) == EI and b"null" in err(), n
    assert fwd(table=C.c_void_p(0x1008)) == EI and b"16-byte" in err()
    # the fused step
    assert step(dt=2) == EI and b"dtype" in err() and step(dt=-1) == EI
    assert step(loss=2) == EI and b"loss kind" in err()
    assert step(tdt=2) == EI and b"target_dtype" in err()
    assert step(mean=0) == EI and b"mean_elems" in err()
    for kw in (dict(E=16), dict(E=96), dict(N1=96), dict(N1=320), dict(P=32), dict(P=320), dict(vocab=263)):
        assert step(**kw) == EU and b"fused step" in err(), kw
    assert step(E=0) == EI and step(N1=0) == EI and step(P=-64) == EI
    for n in ("emb", "femb", "W1", "b1", "W2", "b2", "W1T", "W2T", "x", "target", "slabs", "lay", "accum", "scratch", "er"):
        assert step(**{n: None}) == EI and b"null" in err(), n
    for n in ("W1", "W2", "W1T", "W2T", "slabs"):
        assert step(**{n: C.c_void_p(0x1008)}) == EI and b"16-byte" in err(), n
    for bad, word in ((dict(total=10434), b"multiple of 4"), (dict(total=10428), b"inside"), (dict(font=4092), b"overlap"), (dict(b1=-64), b"inside"),
                      (dict(w1=4162), b"multiple of 4"), (dict(b2=6272), b"overlap")):
        assert step(lay=dict(lay0, **bad)) == EI and word in err(), bad
    assert step(vocab=129) == EI and b"overlap" in err()                                  # the layout was made for 128 rows
    # the transpose
    assert tr(N=0) == EI and tr(K=-1) == EI and b"N = " in err()
    assert tr(W=None) == EI and tr(WT=None) == EI and b"null" in err()


@pytest.mark.parametrize("i", range(len(R.STEP_CASES)), ids=lambda i: str(R.STEP_CASES[i]))
def test_k_model_bound_is_a_priori_holds_the_reference_and_is_not_hollow(i):
    """step_model: its gradient is the unrounded block references' sum; the ROUNDED references' sum -- what a correct kernel leaves, up to
    the block bounds -- lies within its a-priori term M of it; and sums with a planted fault leave M + the summed block bounds"""
    case, loss = R.STEP_CASES[i], R.STEP_VARIANTS[i][0]
    B, E, N1, P, vocab, n_fonts = case
    for is_bf16 in (False, True):
        I, k, _, _, cs, ref = _step(case, is_bf16, loss)
        t, n = R.target_values(k), B * P + 7
        whole, M = R.step_model(I, case, is_bf16, loss, cs, t, n)
        plain = R.step_total(R.step_ref(I, case, is_bf16, loss, cs, t, n, rnd=None), case)
        mine = R.step_total(ref, case)
        bsum = R.step_total({name: ref["b" + name] for name in ("dW2", "db2", "dW1", "db1", "dTab")}, case)
        for name in whole:
            assert rel(whole[name], plain[name]) <= 1e-12, name
        ratios = {name: R.ratio(mine[name], whole[name], M[name]) for name in whole}
        size = {name: float((bsum[name] + M[name]).max() / whole[name].abs().max()) for name in whole}
        print(f"{case} {'bf16' if is_bf16 else 'f32'}: rounded reference / M " + ", ".join(f"{a} {v:.3f}" for a, v in ratios.items())
              + "; largest bound / largest |gradient| " + ", ".join(f"{a} {v:.2g}" for a, v in size.items()))
        assert max(ratios.values()) <= 1.0
        if not is_bf16:
            assert max(size.values()) <= 0.05              # float32: the whole bound stays far below the gradient's own size
        assert size["w2"] <= 0.6 and size["b2"] <= 0.6      # bf16: dW2 / db2 stay below the gradient's own size at every case
        faults = {(95, 32, 256, 256, 128, 0): ("dead_rows", "all_cols"), (200, 32, 128, 256, 37, 3): ("font_row", "all_cols"),
                  (130, 64, 192, 128, 100, 3): ("exclusive", "dead_rows"), (65, 32, 64, 192, 262, 2): ("font_row", "dead_rows")}.get(case, ())
        for fault in faults:
            bad = R.step_total(R.step_ref(I, case, is_bf16, loss, cs, t, n, fault=fault), case)
            worst = max(R.ratio(bad[name], whole[name], bsum[name] + M[name]) for name in whole)
            print(f"    {fault}: {worst:.3g}")
            assert worst > 1.0, fault
