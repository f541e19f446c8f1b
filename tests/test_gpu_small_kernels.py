"""GPU: the glyph step's three small kernels -- glyph_combo_kernel after its re-cut (16 combinations x 64 fc1 rows per block, the W1
row in registers, wave-uniform table rows), and reduce_group_kernel's deep path and glyph_l1_bwd_fused_kernel as they were (held
here so that a later change of either has its shapes and its digests) -- ONE launch each through the afr_op_* entries, by the method of tests/op_harness.py with the checkers
tests/reduce_ref.py and tests/glyph_ref.py: outputs between guard bands, every launch twice with the same bytes.

REDUCE (afr_op_reduce_group, afr_op_reduce_group_step).  One table of deep segments: 32 slabs (quarters of 8: one full round of
loads), 33 (9 / 9 / 9 / 6: a round and a tail), 128 (C3's column ranges: quarters of 32) and 130 (33 / 33 / 33 / 31), each at n = 4
(one float4), 4 * 65 (a 64-column group is crossed) and 4 * 129; plus W1 [64][32] of
128 slabs with its transposed copy.  Plain: torch.equal on the bits to reduce_ref.ordered_sum.  Fused AdamW and Lion, with and
without the bf16 shadow, with and without optimizer groups: against the flat optimizer entries on that gradient
(test_gpu_reduce_ops.fused_case).  The inputs' condition is asserted here: in every segment of 260 columns or more the documented
order differs in bits from the plain ascending one in at least a third of the columns.

COMBO (afr_op_glyph_combo).  37 x 3 = 111 combinations (6 groups of 16 and 15) and 5 x 1; N1 = 8 and 264 (no multiple of the 64-row
chunk); E = 8, 32, 40; n_fonts = 0; ld1 > N1.  cidx, h0c and W1^T bit for bit glyph_ref's; h1c bit for bit the table + gather pair's
bf16 h1 at the combinations' (x, f) (afr_op_glyph_l1_fwd: the arithmetic the combination rows restate) and under glyph_ref's bound;
the error word is 0 for in-range codes and has bit 0 set for out-of-range ones, which give the clamped codes' outputs.

L1 BACKWARD (afr_op_glyph_l1_bwd_fused).  B = 1, 64, 65; N1 = 256 (split in two: ONE 128-column sub-tile per block -- the entry takes
no N1 below 256), 384 (three sub-tiles, unsplit), 1024; dense and combo: glyph_ref.fused_ref under test_l1_bwd_fused's bounds.

PARENT DIGESTS.  SHA-256 of the output bytes of the same launches on the parent commit's build (one MI355X): the reduce table plain
and with AdamW, one combination launch, every l1-backward case.  The arithmetic of none of the three was reordered."""
import ctypes as C
import functools
import hashlib

import pytest
import torch

from ai_font_renderer_amd import _lib
from . import glyph_ref as G
from . import reduce_ref as R
from . import test_gpu_reduce_ops as RO
from .glyph_harness import Tables, check_h1
from .op_harness import Outs, bits, judge, same, twice
from .test_gpu_glyph_ops import _check_fused, run_combo, run_fused
from .test_gpu_glyph_step_ops import run_l1_fwd

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


# what the parent commit's build leaves (module docstring); filled in from its run
PARENT = {
    "combo": "988a1becbc1f42cb",
    "l1 1 1024 combo": "07dd25f58af35a07",
    "l1 1 1024 dense": "07dd25f58af35a07",
    "l1 1 256 combo": "a1657ebc0435bb21",
    "l1 1 256 dense": "a1657ebc0435bb21",
    "l1 1 384 combo": "e7df72194c55fcbf",
    "l1 1 384 dense": "e7df72194c55fcbf",
    "l1 64 1024 combo": "07c34a5b897443b7",
    "l1 64 1024 dense": "07c34a5b897443b7",
    "l1 64 256 combo": "315ab28f8385bde0",
    "l1 64 256 dense": "315ab28f8385bde0",
    "l1 64 384 combo": "06965a66b855c44e",
    "l1 64 384 dense": "06965a66b855c44e",
    "l1 65 1024 combo": "0e57158b6b3c801b",
    "l1 65 1024 dense": "0e57158b6b3c801b",
    "l1 65 256 combo": "38022c73e95619e7",
    "l1 65 256 dense": "38022c73e95619e7",
    "l1 65 384 combo": "bc57abe74e415389",
    "l1 65 384 dense": "bc57abe74e415389",
    "reduce adamw": "c474f269f2fc6a3b",
    "reduce plain": "04d3725c7b95f9fe",
}


def held(key, got):
    print("digest %s %s" % (key, got))
    assert PARENT.get(key) == got, "%s: not the parent build's bytes" % key


# ------------------------------------------------------------------------------------------------------------------ reduce
DEEP_SLABS, DEEP_N = (32, 33, 128, 130), (4, 4 * 65, 4 * 129)
NAME = "smallk"


@functools.lru_cache(maxsize=1)
def smallk_case():
    segs = [R.Seg(s, n, R.ND if (i + j) % 2 else (1.0, 1.0)) for i, s in enumerate(DEEP_SLABS) for j, n in enumerate(DEEP_N)]
    segs.append(R.Seg(128, 64 * 32, tr=(64, 64, 32)))                      # W1 [64][32] and its transposed copy at pitch 64
    return R.Case(NAME, segs, 7600, 64 + 2048 + 64)


@pytest.fixture(autouse=True)
def _own_case(monkeypatch):
    """reduce_ref.case (and with it state, and test_gpu_reduce_ops' launches) knows this file's table by its name"""
    known = R.case
    monkeypatch.setattr(R, "case", lambda name: smallk_case() if name == NAME else known(name))


def test_reduce_inputs_show_the_order():
    for sg in smallk_case().segs:
        assert sg.nslabs >= R.DEEP
        if sg.n >= 260:
            plain = R.sum_groups(sg.slabs, R.slab_groups(sg.nslabs, deep=False), sg.n)
            assert R.differing_share(sg.own, plain) >= 1 / 3, sg.label


def test_reduce_deep_plain_is_the_ordered_sum():
    """afr_op_reduce_group_step without a step (check_plain: the bits of ordered_sum, the gaps, fp64) and afr_op_reduce_group"""
    from .gpu_util import stream
    c = smallk_case()
    grads = RO.own_plain(NAME)
    sl, k = RO.dev_slabs(NAME), len(c.segs)

    def run():
        o = Outs()
        dst = o.new("dst", c.total, torch.float32, guard=RO.GUARD)
        _lib.check(_lib.lib().afr_op_reduce_group(
            k, (C.c_void_p * k)(*[dst.value + 4 * sg.off for sg in c.segs]), (C.c_void_p * k)(*[t.data_ptr() for t in sl]),
            (C.c_int * k)(*[sg.nslabs for sg in c.segs]), (C.c_int64 * k)(*[sg.stride for sg in c.segs]), (C.c_int64 * k)(*[sg.n for sg in c.segs]),
            stream()))
        return o.finish(may_keep_fill=("dst",))["dst"]
    dst = twice(run)
    judge("plain smallk (afr_op_reduce_group)", R.check_plain(c, dst))
    for sg, g in zip(c.segs, grads):
        assert torch.equal(bits(dst[sg.off:sg.off + sg.n]), bits(torch.from_numpy(R.ordered_sum(sg.slabs, sg.nslabs, sg.n)))) and torch.equal(bits(g), bits(dst[sg.off:sg.off + sg.n]))
    held("reduce plain", sha(dst))


@pytest.mark.parametrize("shadow", [False, True], ids=["noshadow", "shadow"])
@pytest.mark.parametrize("groups", [False, True], ids=["plain", "groups"])
@pytest.mark.parametrize("kind", ["adamw", "lion"])
def test_reduce_deep_fused_step(kind, groups, shadow):
    RO.fused_case(NAME, kind, groups, shadow)


def test_reduce_deep_fused_step_parent_bytes():
    """the fused AdamW launch of the table once more, for its bytes: p, m, v, the shadow and the transposed copy"""
    c, h, sl = smallk_case(), RO.HYPER["adamw"], RO.dev_slabs(NAME)
    P0, M0, V0 = R.state(NAME)
    k = len(c.segs)
    o = Outs()
    dst = o.new("dst", c.total, torch.float32, guard=RO.GUARD)
    ptrs = {n: o.new(n, c.total, torch.float32, guard=RO.GUARD, init=c.scatter(v)) for n, v in (("p", P0), ("m", M0), ("v", V0))}
    st = _lib.AfrReduceStep(opt_kind=_lib.OPT_KINDS["adamw"], lr=h["lr"], beta1=h["beta1"], beta2=h["beta2"], eps=h["eps"], weight_decay=h["weight_decay"],
                            t=h["t"], gbase=dst.value, p=ptrs["p"].value, m=ptrs["m"].value, v=ptrs["v"].value)
    st.shadow = o.new("shadow", c.total, BF16, guard=RO.GUARD).value
    base = o.new("shT", c.tr_total, BF16, guard=RO.GUARD).value
    st.shT = (C.c_void_p * k)(*[base + 2 * sg.tr[0] if sg.tr else None for sg in c.segs])
    st.tN, st.tK = (C.c_int32 * k)(*[sg.tr[1] if sg.tr else 0 for sg in c.segs]), (C.c_int32 * k)(*[sg.tr[2] if sg.tr else 0 for sg in c.segs])
    assert RO.group_launch(c, sl, dst, st) == "reduce_group<0,0>"
    out = o.finish(may_keep_fill=("dst", "p", "m", "v", "shadow", "shT"))
    held("reduce adamw", sha(torch.cat([bits(out[n]).view(torch.uint8).reshape(-1) for n in ("p", "m", "v", "shadow", "shT")])))


# ------------------------------------------------------------------------------------------------------------------ combo
# (B, E, N1, vocab, n_fonts, kind, ld1 - N1)
COMBO = [(300, 32, 264, 37, 3, "spread", 8), (10, 8, 8, 5, 1, "spread", 0), (64, 40, 264, 37, 0, "spread", 8), (33, 32, 8, 37, 3, "nofont", 0),
         (5, 40, 72, 5, 1, "one", 0)]


@pytest.mark.parametrize("B,E,N1,vocab,n_fonts,kind,pad", COMBO, ids=lambda v: str(v))
def test_combo_rows_are_the_dense_pair_bit_for_bit(B, E, N1, vocab, n_fonts, kind, pad):
    name = f"combo {B}x{E}->{N1} vocab {vocab} fonts {n_fonts} {kind} ld1 {N1 + pad}"
    T = Tables(E, N1, vocab, n_fonts, 100)
    x, font = G.ids_for(B, vocab, n_fonts, 110, kind)
    xc, fc, _ = G.clamp_ids(x, font, vocab, n_fonts)
    ld1, nf = N1 + pad, max(n_fonts, 1)
    a = twice(lambda: run_combo(T, x, font, ld1))
    assert a["err"] == 0
    assert torch.equal(a["cidx"].long(), xc * nf + fc)
    cx, cf = G.combo_ids(vocab, n_fonts)
    assert torch.equal(bits(a["h0c"]), bits(G.embed_ref(T.t["emb"], T.t["femb"], cx, cf, n_fonts, torch.float32).to(BF16)))
    assert torch.equal(bits(a["w1t"]), bits(T.t["W1"].to(BF16).t().contiguous()))
    if pad:
        fill = bits(torch.full((1,), float("nan"), dtype=BF16))
        assert bool((bits(a["h1c"][:, N1:]) == fill).all()), "h1c: bytes between N1 and ld1 were written"
    h1c = a["h1c"][:, :N1].contiguous()
    dense = run_l1_fwd(T, cx, cf if n_fonts > 0 else None, True)
    assert dense["err"] == 0
    assert torch.equal(bits(h1c), bits(dense["h1"])), "h1c is not the table + gather pair's h1 of the combinations"
    Tr, Tb = G.table_ref(T.t["emb"], T.t["femb"], T.t["W1"], n_fonts)
    h1r, _ = check_h1(name, h1c, Tr, Tb, T.t["b1"], cx, cf, vocab, n_fonts, True)
    judge(name, dict(h1c=h1r))
    same(dict(a, w1t=0), dict(run_combo(T, x, font, ld1, with_w1t=False), w1t=0), "without w1t")
    if B >= 3:
        xb, fb = G.bad_ids(B, vocab, n_fonts, x, font)
        xbc, fbc, flag = G.clamp_ids(xb, fb, vocab, n_fonts)
        bad = run_combo(T, xb, fb, ld1)
        assert flag and bad["err"] == 1
        assert torch.equal(bad["cidx"].long(), xbc * nf + fbc)
        same(dict(bad, err=0, cidx=0), dict(a, cidx=0), "out-of-range indices")
    if (B, E, N1) == (300, 32, 264):
        held("combo", sha(torch.cat([bits(a[n]).view(torch.uint8).reshape(-1) for n in ("h1c", "h0c", "cidx", "w1t")])))


# ------------------------------------------------------------------------------------------------------------------ l1 backward
L1 = [(B, N1, 142, 2, form) for B in (1, 64, 65) for N1 in (256, 384, 1024) for form in ("dense", "combo")]


@pytest.mark.parametrize("B,N1,vocab,n_fonts,form", L1, ids=lambda v: str(v))
def test_l1_bwd_fused_bounds_and_parent_bytes(B, N1, vocab, n_fonts, form):
    I = G.fused_inputs(B, N1, vocab, n_fonts, form, "spread")
    a = twice(lambda: run_fused(I, B, N1, vocab, n_fonts))
    split = _check_fused(f"l1_bwd_fused {B}x{N1} {form}", a, I, B, N1, vocab, n_fonts)
    assert N1 // split == {256: 128, 384: 384, 1024: 256}[N1]              # columns of a block: 1, 3 and 2 sub-tiles
    held("l1 %d %d %s" % (B, N1, form), sha(a))


def test_digest_table_is_complete():
    assert len(PARENT) == 3 + len(L1) and all(isinstance(v, str) and len(v) == 16 for v in PARENT.values())
    # (the dense and the combo form of one l1-backward shape read the same h0 values: one digest)
    assert len(set(PARENT.values())) == 3 + len(L1) // 2
