"""GPU: the glyph nets' fused step (csrc/glyph_fused.hip glyph1_step_kernel), the folded forward's table + gather pair
(csrc/elementwise.hip glyph_table + glyph_l1_fwd) and the operand transpose (transpose_bf16), ONE call each through afr_op_glyph1_step,
afr_op_glyph_l1_fwd and afr_op_transpose_bf16, every output element against the fp64 restatement of tests/glyph_ref.py under its derived
bound, or bit for bit where the kernel's arithmetic is one rounding.  The method is tests/op_harness.py's: outputs pre-filled with NaN
between guard bands of 256 bytes, the launch repeated bit for bit, the largest error printed as a fraction of the bound (pytest -s).

    l1_fwd           glyph_ref.L1_FWD_CASES in float32 and bf16: table under E u sum |tab| |W1|, h1 under the h1 bound with the gate rule of
                     the combination kernel's test, h0' (embedding, two one-hots, +0 pad up to K0) and w1t bit for bit, the other outputs
                     the same bits without w1t; out-of-range ids set bit 0 and give the clamped ids' outputs
    glyph1_step      glyph_ref.STEP_CASES in float32 and bf16, each judged in one instantiation (loss kind x target type x row-mapped
                     targets rotate, glyph_ref.STEP_VARIANTS) and repeated bit for bit with the other target type and the other target
                     addressing: per block its rows of dW2 / db2 and its partial dW1, db1, dTab under step_ref's bounds; the fp64 sum of
                     all slabs against the unsplit, unrounded model (glyph_ref.step_model); the loss, and twice the loss after a second launch into the same
                     accumulator; everything a block does not own keeps the fill; table rows none of its glyphs used are +0; the error
                     word; out-of-range ids.  The inputs leave no gate of the kernel to its rounding (glyph_ref.step_inputs), and two
                     planted columns hold u exactly on the inclusive clamp's two edges.
    transpose_bf16   bit for bit W.to(bf16).t()

Measured on MI355X against the fp64 reference, the largest error / bound per output over all cases:
    l1_fwd           table 0.102; h1 0.092 in float32 and 0.988 in bf16 (the rounding to bf16 is the 2^-8 |ref| term of the bound itself);
                     no ReLU gate differs from fp64's; h0', w1t bit for bit
    glyph1_step f32  per block dW2 0.034, db2 0.044, dW1 0.007, db1 0.006, dTab 0.002; loss 0.002; the fp64 sum of all slabs against the
                     unrounded model: w2 0.032, b2 0.019, w1 0.001, b1 0.001, tab 0.001 (its bound is at most 0.019 of the largest element)
    glyph1_step bf16 per block dW2 0.908, db2 0.676, dW1 0.248, db1 0.099, dTab 0.463; loss 0.003.  Shares of elements near a bf16 rounding
                     boundary (their bound is one bf16 ulp wider, and the widening compounds down the chain), the largest over the cases:
                     h1 0.020, u 0.252, du 0.281, dpre1 0.355, dh0 0.951.  The fp64 sum of all slabs against the unrounded model under
                     the summed block bounds plus glyph_ref.step_model's a-priori bf16 term: w2 0.715, b2 0.653, w1 0.372, b1 0.187,
                     tab 0.279.  That bound is 0.04 .. 0.5 of the largest element for w2 / b2; for w1, b1 and tab the ReLU gates it
                     must take as undecided make it 0.2 .. 31 times the largest element, so there the sum check only catches gross
                     faults and the per-block checks carry the weight (every case prints the figure).
    transpose_bf16   bit for bit"""
import ctypes as C

import pytest
import torch

from ai_font_renderer_amd import _lib
from . import glyph_ref as R
from .glyph_harness import Tables, check_h1, ids_dev
from .gpu_util import dev, ptr, stream
from .op_harness import Outs, bits, dt, judge, same, tt, twice

pytestmark = pytest.mark.gpu
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
LOSS = {"mse": _lib.AFR_LOSS_MSE, "bce": _lib.AFR_LOSS_BCE}


def _bf(cases):
    return [pytest.param(c, bf, id="-".join(str(v) for v in c) + ("-bf16" if bf else "-f32")) for c in cases for bf in (False, True)]


# ------------------------------------------------------------------------------------------------------------------ transpose
@pytest.mark.parametrize("N,K", [(256, 32), (8, 8), (200, 72)])
def test_transpose_bf16(N, K):
    W = R.make_d((N, K), 950)
    Wd = dev(W)

    def run():
        o = Outs()
        p = o.new("wt", (K, N), BF16)
        _lib.check(_lib.lib().afr_op_transpose_bf16(ptr(Wd), p, N, K, stream()))
        return o.finish()["wt"]

    assert torch.equal(bits(twice(run)), bits(W.to(BF16).t().contiguous())), "WT is not bf16(W) transposed"


# ------------------------------------------------------------------------------------------------------------------ folded forward
def run_l1_fwd(T, x, font, is_bf16, with_w1t=True):
    B, K0 = x.shape[0], R.k0_of(T.E, T.vocab, T.n_fonts)
    xd, fd = ids_dev(x, font)
    o = Outs()
    pt, p0, p1 = o.new("table", (T.vocab + T.n_fonts, T.N1), F32), o.new("h0p", (B, K0), tt(is_bf16)), o.new("h1", (B, T.N1), tt(is_bf16))
    pw = o.new("w1t", (T.E, T.N1), BF16) if with_w1t else C.c_void_p(0)
    pe = o.new("err", 1, torch.int32, init=torch.zeros(1, dtype=torch.int32))
    _lib.check(_lib.lib().afr_op_glyph_l1_fwd(dt(is_bf16), T.p("emb"), T.p("femb"), T.p("W1"), T.p("b1"), ptr(xd), ptr(fd), B, T.E, T.N1, T.vocab,
                                              T.n_fonts, pt, p0, p1, pw, pe, stream()))
    out = o.finish()
    return dict(out, err=int(out["err"]))


@pytest.mark.parametrize("case,is_bf16", _bf(R.L1_FWD_CASES))
def test_l1_fwd(case, is_bf16):
    B, E, N1, vocab, n_fonts, kind = case
    name = f"l1_fwd {B}x{E}->{N1} vocab {vocab} fonts {n_fonts} {kind} {'bf16' if is_bf16 else 'f32'}"
    T = Tables(E, N1, vocab, n_fonts, 100)
    x, font = R.ids_for(B, vocab, n_fonts, 110, kind)
    xc, fc, _ = R.clamp_ids(x, font, vocab, n_fonts)
    a = twice(lambda: run_l1_fwd(T, x, font, is_bf16))
    assert a["err"] == 0
    ref = R.l1_fwd_ref(T.t, xc, fc, vocab, n_fonts, is_bf16)
    assert torch.equal(bits(a["h0p"]), bits(ref["h0p"])), "h0' is not [emb + femb | one-hot of x | one-hot of vocab + f | +0 pad] bit for bit"
    assert torch.equal(bits(a["w1t"]), bits(ref["w1t"])), "w1t is not bf16(W1) transposed"
    h1r, flips = check_h1(name, a["h1"], ref["table"], ref["bT"], T.t["b1"], xc, fc, vocab, n_fonts, is_bf16)
    same(dict(a, w1t=0), dict(run_l1_fwd(T, x, font, is_bf16, with_w1t=False), w1t=0), "without w1t")
    judge(name, dict(table=R.ratio(a["table"], ref["table"], ref["bT"]), h1=h1r))
    print(f"    gates that differ from fp64's: {flips} of {a['h1'].numel()}")
    if B >= 3:
        xb, fb = R.bad_ids(B, vocab, n_fonts, x, font)
        xbc, fbc, flag = R.clamp_ids(xb, fb, vocab, n_fonts)
        bad = run_l1_fwd(T, xb, fb, is_bf16)
        assert flag and bad["err"] & 1
        same(dict(bad, err=0), dict(run_l1_fwd(T, xbc, fbc, is_bf16), err=0), "out-of-range indices")


# ------------------------------------------------------------------------------------------------------------------ fused step
class StepCase:
    """a fused-step case's inputs on the device, in one dtype"""

    def __init__(self, case, is_bf16):
        self.case, self.is_bf16 = case, is_bf16
        B, E, N1, P, vocab, n_fonts = case
        self.I = I = R.step_inputs(case, is_bf16)
        wt = tt(is_bf16)
        self.d = dict(emb=dev(I["emb"]), femb=dev(I["femb"]) if n_fonts > 0 else None, b1=dev(I["b1"]), b2=dev(I["b2"]),
                      W1=dev(I["W1"], wt), W2=dev(I["W2"], wt))
        if is_bf16:
            self.d.update(W1T=dev(I["W1"].t().contiguous(), BF16), W2T=dev(I["W2"].t().contiguous(), BF16))
        else:
            self.d.update(W1T=None, W2T=None)           # float32: not read
        self.lay, self.total = R.g1_layout(E, N1, P, vocab, n_fonts)
        self.k, self.rows, self.table = R.step_target_forms(B, P)     # u8 pixel values: dense [B][P]; row map and the table it indexes
        self.mean_elems = B * P + 7

    def targets(self, tgt, rowmapped):
        """-> (device targets, device row map or None): the same targets per glyph in all four forms"""
        k = self.table if rowmapped else self.k
        t = dev(k.to(torch.uint8)) if tgt == "u8" else dev(R.target_values(k))
        return t, (dev(self.rows.to(torch.int32)) if rowmapped else None)


def run_step(S, loss, tgt, rowmapped, x=None, font=None):
    """one launch into fresh slabs, then a second one into the same buffers: -> slabs [blocks][total], err, loss (after the first launch),
    loss2 (after the second)"""
    lib = _lib.lib()
    B, E, N1, P, vocab, n_fonts = S.case
    d, dtype = S.d, dt(S.is_bf16)
    nb = lib.afr_glyph1_blocks(dtype, B, P)
    xd, fd = ids_dev(S.I["x"] if x is None else x, S.I["font"] if x is None else font)
    td, rd = S.targets(tgt, rowmapped)
    lay = _lib.AfrGlyph1Layout(*[S.lay[n] for n in ("emb", "font", "w1", "b1", "w2", "b2")], S.total)
    o = Outs()
    ps = o.new("slabs", (nb, S.total), F32)
    pa = o.new("loss", 1, F32, init=torch.zeros(1))                        # accumulator, scratch (zero before the first call) and the error
    pc = o.new("scratch", 1040 + nb, F32, init=torch.zeros(1040 + nb))     # word are written too: between guard bands like the slabs
    pe = o.new("err", 1, torch.int32, init=torch.zeros(1, dtype=torch.int32))
    accum, band, _, _ = o.bufs["loss"]
    losses = []
    for _ in range(2):
        _lib.check(lib.afr_op_glyph1_step(dtype, LOSS[loss], ptr(d["emb"]), ptr(d["femb"]), ptr(d["W1"]), ptr(d["b1"]), ptr(d["W2"]), ptr(d["b2"]),
                                          ptr(d["W1T"]), ptr(d["W2T"]), ptr(xd), ptr(fd), ptr(td), _lib.AFR_TARGET_U8 if tgt == "u8" else _lib.AFR_TARGET_F32,
                                          ptr(rd), B, E, N1, P, vocab, n_fonts, S.mean_elems, ps, C.byref(lay), pa, pc, pe, stream()))
        losses.append(accum[band:band + 1].cpu())
    out = o.finish(may_keep_fill=("slabs",))                    # a block writes only what it owns (test_glyph1_step asserts exactly that)
    assert not bool(bits(out["scratch"][1032:1040]).any()), "the arrival counter was not re-armed"
    return dict(slabs=out["slabs"], err=int(out["err"]), loss=losses[0], loss2=losses[1])


@pytest.mark.parametrize("case,is_bf16", _bf(R.STEP_CASES))
def test_glyph1_step(case, is_bf16):
    lib = _lib.lib()
    B, E, N1, P, vocab, n_fonts = case
    loss, tgt, rowmapped = R.STEP_VARIANTS[R.STEP_CASES.index(case)]
    name = f"glyph1_step {B}x{E}->{N1}->{P} vocab {vocab} fonts {n_fonts} {'bf16' if is_bf16 else 'f32'} {loss} {tgt} {'rows' if rowmapped else 'dense'}"
    S = StepCase(case, is_bf16)
    cs = lib.afr_glyph1_colsplit(dt(is_bf16), B, P)
    assert cs == R.g1_colsplit(is_bf16, B, P)
    a = twice(lambda: run_step(S, loss, tgt, rowmapped))
    assert a["err"] == 0
    assert torch.equal(bits(a["loss2"]), bits(a["loss"] + a["loss"])), "a second launch did not add the same loss again"
    t = R.target_values(S.k)
    ref = R.step_ref(S.I, case, is_bf16, loss, cs, t, S.mean_elems)
    got = R.slab_views(a["slabs"], S.lay, case, cs)
    worst = {k: R.ratio(got[k], ref[k], ref["b" + k]) for k in ("dW2", "db2", "dW1", "db1", "dTab")}
    worst["loss"] = R.ratio(a["loss"], torch.tensor([ref["loss"]], dtype=F64), ref["bloss"])
    # what a block does not own keeps the fill; what it owns holds no NaN; table rows that none of its glyphs used are +0
    own = R.slab_owned(S.lay, S.total, case, cs).repeat(a["slabs"].shape[0] // cs, 1)
    fill = bits(torch.full((1,), float("nan"), dtype=F32))
    assert bool((bits(a["slabs"])[~own] == fill).all()), f"{name}: a block wrote outside what it owns"
    assert not bool(torch.isnan(a["slabs"][own]).any()), f"{name}: an element a block owns was not written"
    unused = ~ref["used"][:, None, :, None].expand_as(got["dTab"])
    assert not bool(bits(got["dTab"])[unused].any()), f"{name}: a table row no glyph of the block used is not +0"
    # the fp64 sum of all slabs against the unsplit, UNROUNDED model under the summed block bounds plus step_model's a-priori term: what
    # separates the kernel's arithmetic from the model (float32: the one add of h0; bf16: half an ulp at each rounding point, carried on)
    whole, M = R.step_model(S.I, case, is_bf16, loss, cs, t, S.mean_elems)
    sums = R.step_total({k: v.double() for k, v in got.items()}, case)
    bsum = R.step_total({k: ref["b" + k] for k in ("dW2", "db2", "dW1", "db1", "dTab")}, case)
    for k in whole:
        worst["sum " + k] = R.ratio(sums[k], whole[k], bsum[k] + M[k])
    judge(name, worst)
    print(f"    split {cs}, blocks {a['slabs'].shape[0]}, b1 / b2 steps {S.I['steps']}, near a bf16 rounding boundary: "
          + ", ".join(f"{k} {v:.4f}" for k, v in ref["near"].items()))
    print("    the sums' largest bound / largest |model gradient|: " + ", ".join(f"{k} {float((bsum[k] + M[k]).max() / whole[k].abs().max()):.2g}" for k in whole))
    # the same bits with the other target type and the other target addressing
    for v_tgt, v_rows in (("f32" if tgt == "u8" else "u8", rowmapped), (tgt, not rowmapped)):
        same(run_step(S, loss, v_tgt, v_rows), a, f"{name}: targets {v_tgt} {'rows' if v_rows else 'dense'}")
    if B >= 3:
        xb, fb = R.bad_ids(B, vocab, n_fonts, S.I["x"], S.I["font"])
        xbc, fbc, flag = R.clamp_ids(xb, fb, vocab, n_fonts)
        bad = run_step(S, loss, tgt, rowmapped, x=xb, font=fb)
        assert flag and bad["err"] & 1
        same(dict(bad, err=0), dict(run_step(S, loss, tgt, rowmapped, x=xbc, font=fbc if n_fonts > 0 else None), err=0), "out-of-range indices")


def test_glyph1_step_cases_cover_every_instantiation_and_split():
    lib = _lib.lib()
    seen, splits = set(), {False: set(), True: set()}
    for i, (B, E, N1, P, vocab, n_fonts) in enumerate(R.STEP_CASES):
        assert lib.afr_glyph1_eligible(E, N1, P, vocab, n_fonts) == 1
        for bf in (False, True):
            seen |= {(bf,) + v for v in R.step_instantiations(i)}
            splits[bf].add(lib.afr_glyph1_colsplit(dt(bf), B, P))
    assert seen == {(bf, loss, tgt, rows) for bf in (False, True) for loss in ("mse", "bce") for tgt in ("u8", "f32") for rows in (False, True)}
    assert splits[False] == {1, 4} and splits[True] == {1, 2, 4}
