"""Checker for the glyph nets' first-layer kernels (csrc/elementwise.hip glyph_* and csrc/gemm.hip glyph_l1_bwd_fused_kernel, through
the afr_op_glyph_* entries): every kernel restated in plain fp64 torch, no device code, with the bound each output element is held to.
A restatement takes the kernel's rounding points as arguments (rnd: None = none, the model in fp64) and states them once.
u = 2^-24 and ub = 2^-8 are the unit roundoffs of float32 and bfloat16.

    embed          emb[x] + femb[f]: one correctly rounded float32 add, bit for bit torch's (then its .to(bfloat16))
    table          T = [emb; femb] . W1^T, an fma chain of E terms in float32:  |T - ref| <= E u sum_k |tab| |W1|
    h1             pre = (T[x] + b1) + T[vocab + f]: B_pre = the table bounds of the rows used + 3 u (|T_c| + |b1| + |T_f|);
                   |h1 - relu(pre)| <= B_pre (+ ub |ref| in bf16); the ReLU gate may differ from fp64's only where |pre| <= B_pre
    h0'            [embed | one-hot of x | one-hot of vocab + f | +0 pad]: the fused backward's dense operand, and the widened
                   operand behind the post-pass's slabs
    combo          cidx = x max(n_fonts, 1) + f exact, h0c = bf16(embed) exact, h1c under the h1 bound in bf16
    l1_bwd         S = sum_z slab_z:  |dw1 - S[:, :E]| <= nslabs u sum_z |slab|;  per block of 8 fc1 rows
                   |dtab_part - sum_q S[q][E + r] W1[q][k]| <= (nslabs + 8) u sum_q sum_z |slab_z[q][E + r]| |W1[q][k]|
    l1_bwd_fused   per block (64 glyphs, its ncols columns), operands exact bf16, float32 accumulation on the matrix cores:
                   dW1, db1 <= 64 u sum_b |d1| |h0| (h0 = 1 for db1);  dTab: the block forms dh0 over ITS columns, rounds that partial
                   to bf16 and sums it by table row:  sum_{b in row} (ub |dh0| + (1 + ub) ncols u sum_n |d1| |W1|) + 64 u sum_b |dh0|
                   (the reference's own rounding is not in this bound: where the kernel's float32 partial and the fp64 one fall on
                   different sides of a bf16 rounding boundary the two roundings are one bf16 ulp apart, not ub |dh0|.  fused_ref
                   counts the partials that lie within their float32 error bound of such a boundary (`near`); float32 accumulation
                   of exact bf16 products is far more accurate than that bound, and none of them has been seen to straddle)
    embed_bwd      per block of 32 rows, per table row the float32 sum in row order, bit for bit (embed_bwd_f32); against fp64
                   under 32 u sum |d|
"""
import numpy as np
import torch

from ai_font_renderer_amd import synth

from .op_harness import bits  # noqa: F401
from .util import bf16, ratio  # noqa: F401

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
U, UB = 2.0 ** -24, 2.0 ** -8
L1_R, EMB_ROWS, GL1_ROWS, MAX_SPLIT = 64, 32, 8, 4      # glyphs per fused block, rows per embed_bwd block, fc1 rows per post-pass block


# ---------------------------------------------------------------------------------------------------------------- shapes
def k0_of(E, vocab, n_fonts):
    return E + (vocab + n_fonts + 7) // 8 * 8


def fused_eligible(E, N1, vocab, n_fonts):
    return E == 32 and N1 % 128 == 0 and 256 <= N1 <= 1024 and vocab + n_fonts <= 144


def fused_split(B, N1):
    nrb, cs = (B + L1_R - 1) // L1_R, 1
    while cs * 2 <= MAX_SPLIT and cs * 2 * nrb <= 256 and N1 % (cs * 2 * 128) == 0:
        cs *= 2
    return cs


def fused_slab_floats(B, N1, vocab, n_fonts):
    nc = N1 // fused_split(B, N1)
    return nc * 32 + nc + (vocab + n_fonts) * 32


# ---------------------------------------------------------------------------------------------------------------- inputs
def make_ids(B, vocab, n_fonts, tid, kind="spread"):
    """codes over the whole vocabulary with repeats, 0 and vocab - 1 among them (kind "one": one code for every glyph); font ids"""
    x = np.floor(synth.hash_u01(tid, B) * vocab).astype(np.int64).clip(0, vocab - 1)
    if kind == "one":
        x[:] = (2 * vocab) // 3
    else:
        x[-1] = vocab - 1
        if B >= 2:
            x[0] = 0
        if B >= 4:
            x[B // 2] = x[1]
    font = np.floor(synth.hash_u01(tid + 1, B) * max(n_fonts, 1)).astype(np.int64).clip(0, max(n_fonts, 1) - 1)
    return torch.from_numpy(x), (torch.from_numpy(font) if n_fonts > 0 else None)


def make_tables(E, N1, vocab, n_fonts, tid):
    t = lambda i, shape, b: torch.from_numpy(synth.hash_uniform(tid + i, shape, b))      # noqa: E731
    return dict(emb=t(0, (vocab, E), 1.0), femb=t(1, (n_fonts, E), 0.5) if n_fonts > 0 else None,
                W1=t(2, (N1, E), 0.2), b1=t(3, (N1,), 0.1))


def make_d(shape, tid, zeros=0.0, round_bf16=False):
    d = torch.from_numpy(synth.hash_uniform(tid, shape, 1.0))
    if zeros > 0:
        d = torch.where(torch.from_numpy(synth.hash_u01(tid + 1, int(np.prod(shape))).reshape(shape)) < zeros, torch.zeros_like(d), d)
    return bf16(d) if round_bf16 else d


def bad_ids(B, vocab, n_fonts, x, font):
    """out-of-range indices planted: x in {-1, vocab, 2^40}, font in {-3, n_fonts}"""
    x, font = x.clone(), (font.clone() if font is not None else None)
    for i, v in zip((0, B // 2, B - 1), (-1, vocab, 2 ** 40)):
        x[i] = v
    if font is not None:
        for i, v in zip((1 % B, B - 1), (-3, n_fonts)):
            font[i] = v
    return x, font


def clamp_ids(x, font, vocab, n_fonts):
    """-> clamped x, clamped font (zeros where there is none), whether any index was out of range"""
    xc = x.clamp(0, vocab - 1)
    f = torch.zeros_like(x) if font is None else font
    fc = f.clamp(0, max(n_fonts, 1) - 1)
    flag = bool((xc != x).any()) or (n_fonts > 0 and bool((fc != f).any()))
    return xc, fc, flag


# ---------------------------------------------------------------------------------------------------------------- forward
def embed_ref(emb, femb, x, f, n_fonts, dtype=F64):
    e = emb.to(dtype)[x]
    return e + femb.to(dtype)[f] if n_fonts > 0 else e


def table_ref(emb, femb, W1, n_fonts):
    """-> T fp64 [vocab + n_fonts][N1] and its bound"""
    tab = torch.cat([emb, femb]) if n_fonts > 0 else emb
    E = tab.shape[1]
    return tab.double() @ W1.double().t(), E * U * (tab.double().abs() @ W1.double().abs().t())


def h1_ref(T, Tb, b1, x, f, vocab, n_fonts, is_bf16=False):
    """-> pre fp64 [B][N1], B_pre, relu(pre), the bound of h1 (out rounding: bf16 adds ub |ref|)"""
    b1 = b1.double()
    pre, mag, bp = T[x] + b1, T[x].abs() + b1.abs(), Tb[x]
    if n_fonts > 0:
        pre, mag, bp = pre + T[vocab + f], mag + T[vocab + f].abs(), bp + Tb[vocab + f]
    bp = bp + 3 * U * mag
    ref = pre.clamp_min(0)
    return pre, bp, ref, bp + (UB * ref if is_bf16 else 0)


def h0p_ref(emb, femb, x, f, vocab, n_fonts, dtype=F64):
    """h0' [B][K0] = [embed | one-hot of x | one-hot of vocab + f | zero pad]"""
    E, B = emb.shape[1], x.shape[0]
    out = torch.zeros(B, k0_of(E, vocab, n_fonts), dtype=dtype)
    out[:, :E] = embed_ref(emb, femb, x, f, n_fonts, dtype)
    r = torch.arange(B)
    out[r, E + x] = 1
    if n_fonts > 0:
        out[r, E + vocab + f] = 1
    return out


def combo_ids(vocab, n_fonts):
    """the (x, f) of every combination c = x max(n_fonts, 1) + f, in c order"""
    nf = max(n_fonts, 1)
    c = torch.arange(vocab * nf)
    return c // nf, c % nf


# ---------------------------------------------------------------------------------------------------------------- backward
def l1_bwd_ref(slabs, W1, E, vocab, n_fonts):
    """slabs fp32/fp64 [nslabs][N1][K0] -> dw1 [N1][E], its bound, dtab_part [blocks][R][E], its bound"""
    ns, N1, K0 = slabs.shape
    R = vocab + n_fonts
    s64, W = slabs.double(), W1.double()
    S, Sa = s64.sum(0), s64.abs().sum(0)
    nb = (N1 + GL1_ROWS - 1) // GL1_ROWS
    oh, oha = S[:, E:E + R].reshape(nb, GL1_ROWS, R), Sa[:, E:E + R].reshape(nb, GL1_ROWS, R)
    Wb = W.reshape(nb, GL1_ROWS, E)
    part = torch.einsum("bqr,bqk->brk", oh, Wb)
    pb = (ns + 8) * U * torch.einsum("bqr,bqk->brk", oha, Wb.abs())
    return S[:, :E], ns * U * Sa[:, :E], part, pb


def bf16_ulp(q):
    """the spacing of bfloat16 at |q| (q a bfloat16 value, fp64): 2^(exponent - 7); the smallest normal's for q == 0"""
    e = torch.floor(torch.log2(q.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=F64), e - 7)


def fused_ref(d1, h0, W1, x, f, vocab, n_fonts, split, rnd=bf16):
    """d1 [B][N1], h0 [B][32] (glyph order), W1 [N1][32], all exact bf16 values -> per block (row block rb, range cs) in the kernel's
    block order rb * split + cs: dict(dW1 [nc][32], db1 [nc], dTab [R][32], their bounds bW, bb, bT, used [R] bool, near: glyphs
    x columns whose partial may round to the neighbouring bf16).  rnd: the rounding of the block's dh0 partial (None: none)."""
    B, N1 = d1.shape
    R, nc = vocab + n_fonts, N1 // split
    d1, h0, W1 = d1.double(), h0.double(), W1.double()
    out = []
    for rb in range((B + L1_R - 1) // L1_R):
        rows = slice(rb * L1_R, min(B, (rb + 1) * L1_R))
        nbk = rows.stop - rows.start
        oh = torch.zeros(nbk, R, dtype=F64)
        oh[torch.arange(nbk), x[rows]] = 1
        if n_fonts > 0:
            oh[torch.arange(nbk), vocab + f[rows]] = 1
        for cs in range(split):
            cols = slice(cs * nc, (cs + 1) * nc)
            d, w = d1[rows, cols], W1[cols]
            dh0 = d @ w
            delta = (1 + UB) * nc * U * (d.abs() @ w.abs())
            q = dh0 if rnd is None else rnd(dh0)
            per = UB * dh0.abs() + delta
            near = torch.zeros_like(dh0, dtype=torch.bool)
            if rnd is not None:
                ulp = bf16_ulp(q)
                # the boundaries of the cell that rounds to q, in magnitude: |q| + ulp/2 and |q| - ulp/2 (at a power of two the cell
                # below is half as wide: |q| - ulp/4)
                a, qa = dh0.abs(), q.abs()
                lower = torch.where(qa == ulp * 128, ulp / 4, ulp / 2)
                dist = torch.minimum((a - (qa + ulp / 2)).abs(), (a - (qa - lower)).abs())
                near = dist <= delta
            out.append(dict(dW1=d.t() @ h0[rows], bW=L1_R * U * (d.abs().t() @ h0[rows].abs()), db1=d.sum(0), bb=L1_R * U * d.abs().sum(0),
                            dTab=oh.t() @ q, bT=oh.t() @ per + L1_R * U * (oh.t() @ dh0.abs()), used=oh.sum(0) > 0, near=int(near.sum())))
    return out


def split_fused_slabs(slabs, nc, R):
    """slabs [blocks][nc*32 + nc + R*32] -> dW1 [blocks][nc][32], db1 [blocks][nc], dTab [blocks][R][32]"""
    nb = slabs.shape[0]
    return slabs[:, :nc * 32].reshape(nb, nc, 32), slabs[:, nc * 32:nc * 33], slabs[:, nc * 33:].reshape(nb, R, 32)


def embed_bwd_f32(d, x, f, vocab, n_fonts):
    """the kernel's order: per block of 32 rows, one float32 accumulator per table element, rows added in order -> [blocks][R][E]"""
    B, E = d.shape
    R, d = vocab + n_fonts, d.to(F32)
    nb = (B + EMB_ROWS - 1) // EMB_ROWS
    out = torch.zeros(nb, R, E, dtype=F32)
    for b in range(B):
        acc = out[b // EMB_ROWS]
        acc[x[b]] = acc[x[b]] + d[b]
        if n_fonts > 0:
            acc[vocab + f[b]] = acc[vocab + f[b]] + d[b]
    return out


def embed_bwd_ref(d, x, f, vocab, n_fonts):
    """-> fp64 slabs [blocks][R][E], their bound 32 u sum |d|, used [blocks][R] bool"""
    B, E = d.shape
    R, d = vocab + n_fonts, d.double()
    nb = (B + EMB_ROWS - 1) // EMB_ROWS
    blk = torch.arange(B) // EMB_ROWS
    oh = torch.zeros(nb, B, R, dtype=F64)
    oh[blk, torch.arange(B), x] = 1
    if n_fonts > 0:
        oh[blk, torch.arange(B), vocab + f] = 1
    ref = torch.einsum("nbr,be->nre", oh, d)
    return ref, EMB_ROWS * U * torch.einsum("nbr,be->nre", oh, d.abs()), oh.sum(1) > 0


# ---------------------------------------------------------------------------------------------------------------- cases
EMBED_CASES = [(1, 32, 128, 2, "spread"), (300, 32, 128, 0, "spread"), (257, 64, 100, 3, "spread"), (40, 128, 128, 1, "nofont"),
               (77, 24, 50, 2, "spread"), (700, 32, 600, 2, "spread"), (64, 32, 128, 2, "one")]
EMBED_BWD_CASES = [(1, 32, 128, 2, "spread"), (33, 32, 128, 2, "spread")] + EMBED_CASES[1:]
# (B, E, N1, vocab, n_fonts, kind, ld1 - N1)
COMBO_CASES = [(8, 32, 256, 128, 2, "spread", 0), (300, 32, 384, 101, 1, "spread", 8), (513, 32, 640, 37, 3, "spread", 8),
               (65, 32, 1024, 128, 0, "nofont", 0), (100, 40, 264, 50, 2, "spread", 0), (10, 8, 8, 5, 1, "spread", 0),
               (64, 32, 256, 37, 3, "one", 8)]
# (nslabs, N1, E, vocab, n_fonts, slab_stride - N1 K0)
L1_BWD_CASES = [(1, 8, 32, 10, 2, 0), (2, 264, 32, 128, 2, 64), (9, 64, 32, 128, 2, 0), (58, 1024, 32, 128, 2, 0), (5, 40, 32, 478, 2, 4),
                (3, 24, 128, 128, 1, 0)]
# (B, N1, vocab, n_fonts, form, kind): every B, N1 and table of the issue appears; both forms at a ragged (1, 63, 65, 200) and at a full
# (64) last block; N1 = 384 is the unsplit kernel (CS = 1), 256 splits in 2, 1024 in 4
FUSED_CASES = [(1, 256, 142, 2, "dense", "spread"), (1, 384, 16, 1, "combo", "spread"), (63, 1024, 128, 2, "combo", "spread"),
               (63, 384, 100, 0, "dense", "spread"), (64, 384, 142, 2, "dense", "spread"), (64, 256, 128, 2, "combo", "spread"),
               (64, 1024, 16, 1, "dense", "one"), (65, 256, 100, 0, "combo", "spread"), (65, 1024, 142, 2, "dense", "spread"),
               (200, 384, 128, 2, "combo", "spread"), (200, 1024, 16, 1, "dense", "spread"), (200, 256, 142, 2, "combo", "nofont")]


def ids_for(B, vocab, n_fonts, tid, kind):
    """kind "nofont": font = NULL although n_fonts > 0 (font 0 everywhere)"""
    x, f = make_ids(B, vocab, n_fonts, tid, "one" if kind == "one" else "spread")
    if kind == "nofont":
        f = None
    return x, f


def fused_inputs(B, N1, vocab, n_fonts, form, kind, tid=700):
    """-> dict: d1 [B][N1], W1 [N1][32] (exact bf16 values, float32), x, font (or None), h0g [B][32] in glyph order, and the operand the
    kernel reads: "dense" h0 [B][K0] = h0' with ldh = K0, no row map; "combo" h0 = the combination table [ncombo][32], rowmap cidx"""
    x, font = ids_for(B, vocab, n_fonts, tid, kind)
    t = make_tables(32, N1, vocab, n_fonts, tid + 10)
    xc, fc, _ = clamp_ids(x, font, vocab, n_fonts)
    W1 = bf16(t["W1"])
    d1 = make_d((B, N1), tid + 20, zeros=0.3, round_bf16=True)
    h0g = bf16(embed_ref(t["emb"], t["femb"], xc, fc, n_fonts, F32))
    if form == "dense":
        h0 = bf16(h0p_ref(t["emb"], t["femb"], xc, fc, vocab, n_fonts, F32))
        ldh, rowmap = h0.shape[1], None
    else:
        cx, cf = combo_ids(vocab, n_fonts)
        h0 = bf16(embed_ref(t["emb"], t["femb"], cx, cf, n_fonts, F32))
        ldh, rowmap = 32, (xc * max(n_fonts, 1) + fc).to(torch.int32)
    return dict(d1=d1, W1=W1, x=x, font=font, xc=xc, fc=fc, h0g=h0g, h0=h0, ldh=ldh, rowmap=rowmap)
