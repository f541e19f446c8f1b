"""Checker for the sheet model's front end (csrc/sheet.hip through afr_op_sheet_fwd / afr_op_sheet_bwd): the two fused kernels
restated against their own interfaces (parameters, codes, dropout description and dz in; z, the save area and the ten parameter
gradients out), evaluated in fp64 (the reference) or in float32 (a yardstick for the bounds only -- the restatements compute in the
dtype they are handed), the error bounds the GPU tests hold the kernels to, faults that can be planted by name (tests of the
tests), and the deterministic inputs both test files share.

THE BOUNDS.  U = 2^-24 is one float32 rounding to nearest, relative.  A worst-case analysis (every rounding at its limit and all
of one sign) overstates float32 here by three to four orders of magnitude: a z element sits behind nine stages (embedding, in-proj,
scores, softmax, attention output, out-proj, LayerNorm, affine, fc1), each a sum of 8 .. 120 terms, and a gradient element behind
those, their reverses and a sum over B L positions -- such a bound would be wider than the faults it has to catch.  So the model is
the standard probabilistic one (Higham & Mary, SIAM J. Sci. Comput. 2019): the roundings of distinct operations are independent
errors of zero mean, each at most U times the magnitude it rounds.  Everything is first order in U and built from magnitudes of the
fp64 run; every quantity t of the chain carries a SQUARED bound vt per element, and

  * a linear step y = sum_k c_k x_k passes them on with squared coefficients, vy = sum_k c_k^2 vx_k; products and the nonlinear steps
    (exp, 1/x, 1/sqrt) are linearised around the fp64 values;
  * a sum of n terms adds n U^2 (sum |terms|)^2: n roundings of partial sums, each of which is at most the sum of the magnitudes.
    A K-term product run as a k-ordered fma chain (the MFMA tiles, dot8) has n = K + 1 (K fused steps and the bias).  The attention
    rows split their keys even / odd over two lanes: L / 2 fused steps in the lane, the add across the pair, the scaling by
    1 / sum, rounded up to n = L / 2 + 3; the by-column pass splits the queries alike; dq, formed as (T1 - delta T2) / sum from
    two such sums, has n = L / 2 + 7 on the magnitudes of T1 and delta T2;
  * __expf(g), g = s - max <= 0, is exp2(g log2 e) on the hardware exponential: the product rounds (U |g| log2 e on the exponent,
    that much relative on the result), the subtraction rounds (U |g|), the instruction is good to 1 ulp (2 U): (4 + 3 |g|) U
    relative -- entered as if it were random, which only widens -- on top of the errors of s and of the row maximum that shift g.
    A value below 2^-126 may be flushed to zero;
  * the row statistics: |max_j (s_j + e_j) - max_j s_j| <= max_j |e_j|; 1/sum carries the p-weighted errors of the exponentials;
  * LayerNorm: the mean is 2 add levels in a lane and 3 shuffle levels, the variance 4 fused steps and 3 levels.  A row of equal
    values is a case the kernel must handle and the one where roundings of a sum are NOT of zero mean (every addend is the same), so
    these two sums are taken at their worst: 5 U mean|x| and 7 U var.  The centred values carry the mean's error, rstd =
    1 / sqrt(var + eps) half the variance's relative error and 3 roundings; the backward's two row means have n = 8;
  * the dropout scales are the kernel's own float32 values in the reference; the float32 constant sqrt(1/8) is one more U on q;
  * the ten parameter gradients: (a) each (string, position) term with its squared bound; (b) each block's accumulator -- MFMA
    tile, aPos register, bias partials, the slab read-modify-write of an embedding row -- a chain of n_c = trips (L + 3) additions
    for the block (trips for a positional row), each rounding at most U times the block's sum of magnitudes S_blk:
    n_c U^2 S_blk^2 per block; (c) when the slabs are summed in float32 (afr_op_reduce, the grouped reduce) each addition rounds a
    partial total of the fp64 block gradients: U^2 sum_k (G_0 + .. + G_k)^2; summed in fp64 on the host, nothing.
The bound is LAM = 8 times the root of the squared bound: each piece above is already several standard deviations of what it
models (a rounding's standard deviation is U / sqrt 3, partial sums of mixed signs stay far below the sum of magnitudes), so LAM
covers both the maximum over 10^5 .. 10^6 elements and errors that are shared between paths (the same e feeds q, k, v and the
residual) and therefore not independent.  What is systematic (rounded constants) is covered by SYS U |out| with SYS = 4.
A bf16 z is the float32 value rounded once more to nearest even: (1 + 2^-8) bound + 2^-8 |ref| (8 significand bits: half an ulp is 2^-8 relative).  A bf16 dz is an exact input."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from ai_font_renderer_amd import synth

from .util import bf16, ratio  # noqa: F401

U = 2.0 ** -24
TINY = 2.0 ** -126
E, H, D, F, QKV = 32, 4, 8, 64, 96
LMAX, MAXBLK, SAVE_PER_POS = 120, 256, 56
EPS = 1e-5                                   # config.SheetConfig.ln_eps
RATES = (0.2, 0.2, 0.25)                     # config.SheetConfig p_embed, p_attn, p_fc: the reference's rates
LAM, SYS = 6.0, 4.0
SCALE = math.sqrt(1.0 / 8.0)
NAMES = ("pos", "emb", "w_in", "b_in", "w_o", "b_o", "ln_g", "ln_b", "w1", "b1")
STATE = dict(pos="positional_encoding", emb="embedding.weight", w_in="attention.in_proj_weight", b_in="attention.in_proj_bias",
             w_o="attention.out_proj.weight", b_o="attention.out_proj.bias", ln_g="layer_norm.weight", ln_b="layer_norm.bias",
             w1="fc1.weight", b1="fc1.bias")
F64, F32 = torch.float64, torch.float32


def blocks(B):
    return min(B, MAXBLK)


def trips(B):
    return -(-B // MAXBLK)


def kscale(p):
    """1 / (1 - p) as the kernels hold it: float32 arithmetic on the float32 rate"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def masks_for(B, L, drop):
    """the three keep masks of synth.sheet_dropout_masks for a dropout description (None: eval), as torch uint8"""
    if drop is None:
        return None
    cfg = SimpleNamespace(embed_dim=E, heads=H, fc_dim=F, p_embed=drop["p"][0], p_attn=drop["p"][1], p_fc=drop["p"][2])
    m = synth.sheet_dropout_masks(cfg, B, L, drop["seed"], drop["step"], drop["rank"])
    return {k: torch.from_numpy(v) for k, v in m.items()}


def scales_for(drop):
    return None if drop is None else tuple(kscale(p) for p in drop["p"])


def pack_bits(keep):
    """attention keep mask [B][H][L][L] (0/1) -> the save area's words, int64 [B][H][L][4] holding uint32 values: row (h, i), key j is
    bit (j>>1)&31 of word (j&1)*2 + (j>>6)"""
    B, Hh, L, _ = keep.shape
    out = torch.zeros(B, Hh, L, 4, dtype=torch.int64)
    for j in range(L):
        out[..., (j & 1) * 2 + (j >> 6)] |= keep[..., j].to(torch.int64) << ((j >> 1) & 31)
    return out


# ================================================================================================ restatements
FAULTS = ("keepword", "dk_scale", "demb_nomask", "chain8", "var31", "dpos_tail", "trip2_codes", "recompute_eval")


def _heads(t):
    B, L, _ = t.shape
    return t.reshape(B, L, H, D).permute(0, 2, 1, 3)


def _merge(t):
    B, _, L, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, L, E)


def front_fwd(P, x, L, max_length, masks=None, scales=None, eps=EPS, fault=None, relu_gate=None):
    """sheet_fwd_kernel.  P: name -> tensor (NAMES) in the dtype to compute in; x int64 [B][>= L]; masks / scales: None (eval) or the
    keep masks and their three scales.  -> z [B][max_length*64]; the save area's o [B][L][32], smax and sinv [B][4][L] (the row
    maximum of the scaled scores and 1 / sum_j exp(s_j - max)), bits [B][4][L][4] (training); cache: what front_bwd and the bounds need.
    relu_gate: bool [B][L][64] used instead of pre > 0.  fault: 'var31' divides the variance by 31; 'trip2_codes' gives string
    b of the second trip (256 <= b < 512) the codes of string b - 256; 'recompute_eval' ignores the attention mask."""
    dt = P["emb"].dtype
    B, vocab = x.shape[0], P["emb"].shape[0]
    tok = x[:, :L].clamp(0, vocab - 1)
    if fault == "trip2_codes" and B > MAXBLK:
        n2 = min(B, 2 * MAXBLK) - MAXBLK
        tok = tok.clone()
        tok[MAXBLK:MAXBLK + n2] = tok[:n2]
    se, sa, sf = scales if masks is not None else (1.0, 1.0, 1.0)
    one = torch.ones((), dtype=dt)
    me = masks["embed"].to(dt) * se if masks is not None else one
    ma = masks["attn"].to(dt) * sa if masks is not None and fault != "recompute_eval" else one
    mf = masks["fc"].to(dt) * sf if masks is not None else one
    e1 = P["emb"][tok] * me
    e = e1 + P["pos"][:L]
    qkv = e @ P["w_in"].t() + P["b_in"]
    q, k, v = (_heads(t) for t in qkv.split(E, dim=-1))
    qs = q * SCALE
    s = qs @ k.transpose(-1, -2)
    smax = s.amax(-1)
    pt = torch.exp(s - smax.unsqueeze(-1))
    sinv = 1.0 / pt.sum(-1)
    A = pt * sinv.unsqueeze(-1)
    o = _merge((A * ma) @ v)
    r = e + o @ P["w_o"].t() + P["b_o"]
    mu = r.mean(-1, keepdim=True)
    xc = r - mu
    var = (xc * xc).sum(-1, keepdim=True) / (31.0 if fault == "var31" else 32.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = xc * rstd
    n = xh * P["ln_g"] + P["ln_b"]
    pre = n @ P["w1"].t() + P["b1"]
    gate = (pre > 0) if relu_gate is None else relu_gate
    f = pre * gate.to(dt) * mf
    z = torch.zeros(B, max_length * F, dtype=dt)
    z[:, :L * F] = f.reshape(B, L * F)
    bits = pack_bits(masks["attn"]) if masks is not None else None
    cache = dict(tok=tok, L=L, max_length=max_length, me=me, ma=ma, mf=mf, e1=e1, e=e, q=q, k=k, v=v, qs=qs, s=s, A=A, o=o, r=r, xc=xc,
                 var=var, rstd=rstd, xh=xh, n=n, pre=pre, gate=gate, eps=eps, training=masks is not None)
    return dict(z=z, o=o, smax=smax, sinv=sinv, bits=bits, cache=cache)


def occurrence_rank(tok):
    """[B][L]: how many earlier positions of the string hold the same code"""
    L = tok.shape[1]
    same = (tok.unsqueeze(2) == tok.unsqueeze(1)) & torch.ones(L, L, dtype=torch.bool).tril(-1)
    return same.sum(-1)


def front_bwd(P, fw, dz, fault=None):
    """sheet_bwd_kernel on the forward state fw (front_fwd in the same dtype; the kernel reloads or recomputes exactly that state).
    dz [B][max_length*64].  -> G: the ten gradients (pos [max_length][32], emb [vocab][32]); Gs: per string, [B] in front; cache.
    fault: 'keepword' (the by-column pass reads key j >= 64's keep bit from the word of key j - 64), 'dk_scale' (dk without
    sqrt(1/8)), 'demb_nomask' (dEmb without the embedding-dropout mask), 'chain8' (a code's occurrences after the 8th left out),
    'dpos_tail' (rows of dP at or beyond L hold row L - 1)."""
    c = fw["cache"]
    dt = P["emb"].dtype
    L, tok = c["L"], c["tok"]
    B, vocab = tok.shape[0], P["emb"].shape[0]
    A, ma, xh = c["A"], c["ma"], c["xh"]
    df = dz[:, :L * F].reshape(B, L, F).to(dt) * c["mf"] * c["gate"].to(dt)
    Gs = {}
    Gs["w1"] = torch.einsum("blf,blc->bfc", df, c["n"])
    Gs["b1"] = df.sum(1)
    dn = df @ P["w1"]
    Gs["ln_g"], Gs["ln_b"] = (dn * xh).sum(1), dn.sum(1)
    g = dn * P["ln_g"]
    m1, m2 = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    dr = (g - m1 - xh * m2) * c["rstd"]
    Gs["w_o"] = torch.einsum("ble,blc->bec", dr, c["o"])
    Gs["b_o"] = dr.sum(1)
    dO = _heads(dr @ P["w_o"])
    dPv = dO @ c["v"].transpose(-1, -2)                           # [B][H][L][L]: dO_i . v_j
    dPm = dPv * ma
    delta = (A * dPm).sum(-1, keepdim=True)
    dS = A * (dPm - delta)
    dq = (dS @ c["k"]) * SCALE
    mac = ma
    if fault == "keepword" and L > 64 and c["training"]:
        mac = ma.clone()
        mac[..., 64:] = ma[..., :L - 64]
    dSc = A * (dPv * mac - delta)
    dk = dSc.transpose(-1, -2) @ (c["q"] if fault == "dk_scale" else c["qs"])
    dv = (A * mac).transpose(-1, -2) @ dO
    dqkv = torch.cat([_merge(dq), _merge(dk), _merge(dv)], -1)
    Gs["w_in"] = torch.einsum("blj,blc->bjc", dqkv, c["e"])
    Gs["b_in"] = dqkv.sum(1)
    de = dr + dqkv @ P["w_in"]
    Gs["pos"] = torch.zeros(B, c["max_length"], E, dtype=dt)
    Gs["pos"][:, :L] = de
    if fault == "dpos_tail":
        Gs["pos"][:, L:] = de[:, L - 1:L]
    de0 = de * (1.0 if fault == "demb_nomask" else c["me"])
    if fault == "chain8":
        de0 = de0 * (occurrence_rank(tok) < 8).to(dt).unsqueeze(-1)
    idx = (torch.arange(B).unsqueeze(1) * vocab + tok).reshape(-1)
    Gs["emb"] = torch.zeros(B * vocab, E, dtype=dt).index_add_(0, idx, de0.reshape(-1, E)).reshape(B, vocab, E)
    G = {k: t.sum(0) for k, t in Gs.items()}
    cache = dict(df=df, dn=dn, g=g, m1=m1, m2=m2, dr=dr, dO=dO, dPv=dPv, dPm=dPm, delta=delta, dS=dS, dq=dq, dk=dk, dv=dv, dqkv=dqkv,
                 de=de, de0=de0)
    return dict(G=G, Gs=Gs, cache=cache)


# ================================================================================================ bounds (fp64 tensors in)
U2 = U * U


def _mm2(x, vx, W, b=None):
    """squared bound of x . W^T (+ b), a K-term k-ordered fma chain: vx W^2 + (K + 1) U^2 (|x| |W|^T + |b|)^2"""
    mag = x.abs() @ W.abs().t()
    if b is not None:
        mag = mag + b.abs()
    return vx @ (W * W).t() + (W.shape[1] + 1.0) * U2 * mag * mag


def _T(t):
    return t.transpose(-1, -2)


def _fin(v, ref):
    return LAM * torch.sqrt(v) + SYS * U * ref.abs()


def fwd_bounds(P, fw, is_bf16=False):
    """-> bounds z [B][max_length*64] (zero beyond L*64: exact zeros are demanded), o [B][L][32], smax, sinv [B][4][L]; pre: the
    bound of the fc1 pre-activation (a ReLU gate may differ from fp64's only where |pre| is below it); var: the squared bounds
    of the intermediates, for bwd_bounds."""
    c = fw["cache"]
    L = c["L"]
    ne = L / 2.0 + 3.0
    ve = U2 * (c["e1"] ** 2 + c["e"] ** 2)
    vqkv = _mm2(c["e"], ve, P["w_in"], P["b_in"])
    vq, vk, vv = (_heads(t) for t in vqkv.split(E, dim=-1))
    q, k, v, qs, A, ma = c["q"], c["k"], c["v"], c["qs"], c["A"], c["ma"]
    vqs = (vq + 2.0 * U2 * q * q) * SCALE ** 2
    vs = vqs @ _T(k * k) + (qs * qs) @ _T(vk) + 9.0 * U2 * (qs.abs() @ _T(k.abs())) ** 2
    vmx = vs.amax(-1, keepdim=True)
    gap = (c["s"] - c["s"].amax(-1, keepdim=True)).abs()
    vrelp = vs + vmx + ((4.0 + 3.0 * gap) * U) ** 2
    pt = torch.exp(-gap)
    psum = pt.sum(-1, keepdim=True)
    vrelsum = (pt * pt * vrelp).sum(-1, keepdim=True) / psum ** 2 + ne * U2 + (L * TINY / psum) ** 2
    vsinv = ((vrelsum + 2.0 * U2) / psum ** 2).squeeze(-1)
    # A_j = p_j / sum_i p_i does not move with the maximum (the shift is common to both): d log A_j = ds_j - sum_i A_i ds_i
    vex = ((4.0 + 3.0 * gap) * U) ** 2
    vsx = vs + vex
    vA = A * A * ((1.0 - 2.0 * A) * vsx + (A * A * vsx).sum(-1, keepdim=True) + ne * U2) + (TINY / psum) ** 2
    Am = A * ma
    # the errors of v_j are NOT taken as independent over the keys j: one code at several positions gives (nearly) the same row and
    # the same roundings, so they are added linearly
    vo = _merge((vA * ma * ma) @ (v * v) + (Am @ torch.sqrt(vv)) ** 2 + ne * U2 * (Am @ v.abs()) ** 2)
    r, xc, var, rstd, xh = c["r"], c["xc"], c["var"], c["rstd"], c["xh"]
    vr = ve + _mm2(c["o"], vo, P["w_o"], P["b_o"]) + 2.0 * U2 * r * r
    vmu = vr.mean(-1, keepdim=True) / E + (5.0 * U * r.abs().mean(-1, keepdim=True)) ** 2
    # the errors of the mean and of rstd are common to a row's 32 channels: they reach pre as ONE error times a sum over the channels
    # (coherent), not as 32 independent ones, and the mean's drops out of the variance (the centred values sum to zero)
    vxc = vr + U2 * xc * xc
    vvar = (4.0 * xc * xc * vxc).mean(-1, keepdim=True) / E + (7.0 * U * var) ** 2
    vrelrs = 0.25 * vvar / (var + c["eps"]) ** 2 + 3.0 * U2
    vxh_own = vxc * rstd ** 2 + U2 * xh * xh
    vxh = vxh_own + vmu * rstd ** 2 + xh * xh * vrelrs
    vn = vxh * P["ln_g"] ** 2 + U2 * c["n"] ** 2
    vpre = _mm2(c["n"], vxh_own * P["ln_g"] ** 2 + U2 * c["n"] ** 2, P["w1"], P["b1"]) \
        + vmu * rstd ** 2 * (P["ln_g"] @ P["w1"].t()) ** 2 + vrelrs * ((xh * P["ln_g"]) @ P["w1"].t()) ** 2
    B = r.shape[0]
    zl = c["pre"] * c["gate"] * c["mf"]
    zb = torch.zeros(B, c["max_length"] * F, dtype=F64)
    zb[:, :L * F] = _fin(vpre * c["mf"] ** 2 + U2 * zl * zl, zl).reshape(B, L * F)
    if is_bf16:
        zb = zb * (1.0 + 2.0 ** -8) + 2.0 ** -8 * fw["z"].abs()
    var_ = dict(ve=ve, vk=vk, vv=vv, vqs=vqs, vA=vA, vo=vo, vxh=vxh, vrelrs=vrelrs, vn=vn)
    return dict(z=zb, o=_fin(vo, c["o"]), smax=_fin(vmx.squeeze(-1), fw["smax"]), sinv=_fin(vsinv, fw["sinv"]), pre=_fin(vpre, c["pre"]),
                var=var_)


def _blk(t, B):
    """per-string values [B][...] -> per-block sums [blocks][...]: block k owns strings k, k + 256, ..."""
    nb = blocks(B)
    return torch.zeros((nb,) + tuple(t.shape[1:]), dtype=t.dtype).index_add_(0, torch.arange(B) % nb, t)


def _trip_slices(B):
    nb = blocks(B)
    return [slice(t * nb, min(B, (t + 1) * nb)) for t in range(trips(B))]


def _chain_prod(a, b, B):
    """an MFMA accumulator tile: acc[f][c] += a[l][f] b[l][c] over the positions l of the block's strings in order.  Every addition
    rounds a partial sum that is at most the sum of the magnitudes so far -> sum over blocks and additions of that sum squared"""
    a, b = a.abs(), b.abs()
    run = torch.zeros(blocks(B), a.shape[-1], b.shape[-1], dtype=F64)
    acc = torch.zeros(a.shape[-1], b.shape[-1], dtype=F64)
    for sl in _trip_slices(B):
        n = sl.stop - sl.start
        for l in range(a.shape[1]):
            run[:n] += a[sl, l, :, None] * b[sl, l, None, :]
            acc += (run[:n] ** 2).sum(0)
    return acc


def _chain_cols(m, B, parts):
    """a column sum held in `parts` partials per string (rows p, p + parts, ... in order), the partials added in order, the string's
    total added to the block's register: the same count for m [B][L][C] magnitudes"""
    m = m.abs()
    run = torch.zeros(blocks(B), m.shape[-1], dtype=F64)
    acc = torch.zeros(m.shape[-1], dtype=F64)
    for sl in _trip_slices(B):
        n = sl.stop - sl.start
        tot = torch.zeros(n, m.shape[-1], dtype=F64)
        for p in range(parts):
            cs = m[sl, p::parts].cumsum(1)
            if cs.shape[1]:
                acc += (cs ** 2).sum((0, 1))
                tot = tot + cs[:, -1]
                acc += (tot ** 2).sum(0)
        run[:n] += tot
        acc += (run[:n] ** 2).sum(0)
    return acc


def _chain_emb(m, tok, B, vocab):
    """an embedding row: a code's occurrences in a string are added in position order, the string's sum to the block's slab row"""
    m = m.abs()
    run = torch.zeros(blocks(B), vocab, E, dtype=F64)
    acc = torch.zeros(vocab, E, dtype=F64)
    for sl in _trip_slices(B):
        n = sl.stop - sl.start
        rows = torch.arange(n)
        here = torch.zeros(n, vocab, E, dtype=F64)
        for l in range(m.shape[1]):
            here[rows, tok[sl, l]] += m[sl, l]
            acc.index_add_(0, tok[sl, l], here[rows, tok[sl, l]] ** 2)
        run[:n] += here
        touched = (here != 0).any(-1)
        acc += ((run[:n] ** 2) * touched.unsqueeze(-1)).sum(0)
    return acc


def _sum_bound(G, rows2, chain2, Gs, B, reduced):
    """a parameter gradient: rows2 = sum over the (string, position) terms of their squared bounds; chain2 = sum over the additions
    into the blocks' accumulators of the squared magnitude each rounds; Gs [B][...] the per-string fp64 gradients (for the
    float32 slab sum)"""
    b2 = rows2 + U2 * chain2
    if reduced:
        b2 = b2 + U2 * (_blk(Gs, B).cumsum(0) ** 2).sum(0)
    return _fin(b2, G)


def _prod_bound(a, va, b, vb, G, Gs, B, reduced):
    """G[f][c] = sum over (string, position) of a[.., f] b[.., c]: a term's squared bound is va b^2 + a^2 vb + U^2 (a b)^2"""
    va = va + U2 * a * a
    rows2 = torch.einsum("blf,blc->fc", va, b * b) + torch.einsum("blf,blc->fc", a * a, vb)
    return _sum_bound(G, rows2, _chain_prod(a, b, B), Gs, B, reduced)


def _col_bound(a, va, G, Gs, B, parts, reduced):
    return _sum_bound(G, va.sum((0, 1)), _chain_cols(a, B, parts), Gs, B, reduced)


def bwd_bounds(P, fw, fb, bw, reduced=False):
    """-> name -> bound of the summed slabs, per element, for the ten gradients.  fb = fwd_bounds(P, fw); bw = front_bwd(P, fw, dz).
    Rows of dP at or beyond L and embedding rows of codes no string holds get a zero bound (exact zeros are demanded)."""
    c, w, e = fw["cache"], bw["cache"], fb["var"]
    G, Gs = bw["G"], bw["Gs"]
    L, tok = c["L"], c["tok"]
    B, vocab = tok.shape[0], P["emb"].shape[0]
    ne = L / 2.0 + 3.0
    A, ma, xh, rstd = c["A"], c["ma"], c["xh"], c["rstd"]
    out = {}
    df = w["df"]
    vdf = 2.0 * U2 * df * df
    out["w1"] = _prod_bound(df, vdf, c["n"], e["vn"], G["w1"], Gs["w1"], B, reduced)
    out["b1"] = _col_bound(df, vdf, G["b1"], Gs["b1"], B, 4, reduced)
    dn = w["dn"]
    vdn = _mm2(df, vdf, P["w1"].t())
    out["ln_g"] = _col_bound(dn * xh, vdn * xh * xh + dn * dn * e["vxh"] + U2 * (dn * xh) ** 2, G["ln_g"], Gs["ln_g"], B, 4, reduced)
    out["ln_b"] = _col_bound(dn, vdn, G["ln_b"], Gs["ln_b"], B, 4, reduced)
    g, m1, m2, dr = w["g"], w["m1"], w["m2"], w["dr"]
    vg = vdn * P["ln_g"] ** 2 + U2 * g * g
    vm1 = vg.mean(-1, keepdim=True) / E + 8.0 * U2 * g.abs().mean(-1, keepdim=True) ** 2
    vm2 = (vg * xh * xh + g * g * e["vxh"]).mean(-1, keepdim=True) / E + 8.0 * U2 * (g * xh).abs().mean(-1, keepdim=True) ** 2
    vdr = (vg + vm1 + e["vxh"] * m2 * m2 + xh * xh * vm2 + 3.0 * U2 * (g.abs() + m1.abs() + (xh * m2).abs()) ** 2) * rstd ** 2 \
        + dr * dr * (e["vrelrs"] + U2)
    out["w_o"] = _prod_bound(dr, vdr, c["o"], e["vo"], G["w_o"], Gs["w_o"], B, reduced)
    out["b_o"] = _col_bound(dr, vdr, G["b_o"], Gs["b_o"], B, 4, reduced)
    dO = w["dO"]
    vdO = _heads(_mm2(dr, vdr, P["w_o"].t()))
    v, k, qs = c["v"], c["k"], c["qs"]
    dPm, delta, dS = w["dPm"], w["delta"], w["dS"]
    vdP = (vdO @ _T(v * v) + (dO * dO) @ _T(e["vv"]) + 10.0 * U2 * (dO.abs() @ _T(v.abs())) ** 2) * ma * ma
    AdP = A * dPm.abs()
    vdelta = (e["vA"] * dPm * dPm + A * A * vdP).sum(-1, keepdim=True) + ne * U2 * AdP.sum(-1, keepdim=True) ** 2
    # dS_ij = A_ij (dP_ij - sum_j' A_ij' dP_ij'): dP_ij's own error enters with 1 - A_ij (both passes form the same dP bit for bit)
    vdS = e["vA"] * (dPm - delta) ** 2 + A * A * (vdP * (1.0 - 2.0 * A) + vdelta) + 2.0 * U2 * dS * dS
    # dq as the kernel forms it: scale (T1 - delta T2) / sum, T1 = sum p dP k, T2 = sum p k
    vdq = SCALE ** 2 * (vdS @ (k * k) + (dS * dS) @ e["vk"] + (ne + 4.0) * U2 * (AdP @ k.abs() + delta.abs() * (A @ k.abs())) ** 2)
    vdk = _T(vdS) @ (qs * qs) + _T(dS * dS) @ e["vqs"] + ne * U2 * (_T(dS.abs()) @ qs.abs()) ** 2
    Am = A * ma
    vdv = _T(e["vA"] * ma * ma) @ (dO * dO) + _T(Am * Am) @ vdO + ne * U2 * (_T(Am) @ dO.abs()) ** 2
    dqkv = w["dqkv"]
    vdqkv = torch.cat([_merge(vdq), _merge(vdk), _merge(vdv)], -1)
    out["w_in"] = _prod_bound(dqkv, vdqkv, c["e"], e["ve"], G["w_in"], Gs["w_in"], B, reduced)
    out["b_in"] = _col_bound(dqkv, vdqkv, G["b_in"], Gs["b_in"], B, 2, reduced)
    de = w["de"]
    vde = vdr + _mm2(dqkv, vdqkv, P["w_in"].t()) + 2.0 * U2 * de * de
    pad = lambda t: torch.cat([t, torch.zeros(B, c["max_length"] - L, E, dtype=F64)], 1)                  # noqa: E731
    out["pos"] = _sum_bound(G["pos"], pad(vde).sum(0), _chain_cols(pad(de).reshape(B, 1, -1), B, 1).reshape(-1, E), Gs["pos"], B, reduced)
    out["pos"][L:] = 0.0
    de0 = w["de0"]
    vde0 = vde * c["me"] ** 2 + U2 * de0 * de0
    rows2 = torch.zeros(vocab, E, dtype=F64).index_add_(0, tok.reshape(-1), vde0.reshape(-1, E))
    out["emb"] = _sum_bound(G["emb"], rows2, _chain_emb(de0, tok, B, vocab), Gs["emb"], B, reduced)
    used = torch.zeros(vocab, dtype=torch.bool)
    used[tok.reshape(-1)] = True
    out["emb"][~used] = 0.0
    return out


# ================================================================================================ inputs
def slab_layout(max_length, vocab, align=64):
    """offsets (floats) of the ten tensors in a slab, each on a multiple of `align` as in the flat parameter buffer, and the total"""
    sizes = dict(pos=max_length * E, emb=vocab * E, w_in=QKV * E, b_in=QKV, w_o=E * E, b_o=E, ln_g=E, ln_b=E, w1=F * E, b1=F)
    off, o = {}, 0
    for n in NAMES:
        off[n] = o
        o = (o + sizes[n] + align - 1) // align * align
    return off, sizes, o


def params(max_length, vocab=128, kind="generic", seed=synth.SEED):
    """name -> float32 tensor.  generic: synth.make_params.  The special sets:
    scores     W_in's q and k rows x 8: score gaps reach 0 .. +-100 (one-hot rows; the all-one-code string keeps uniform rows)
    ln         W_o = b_o = 0 and pos[l] = l / 1024 in every channel, so a LayerNorm row is an embedding row plus a constant (position 0:
               the row itself; the constant keeps the rows of one code at several positions, and their roundings, apart), and q = 0,
               so the scores stay 0: code v % 4 = 0 constant 0.7, 1 mean 1e3, 2 magnitude
               1e-4, 3 one channel x 1e4
    gate_all / gate_none   fc1.bias + 10 / - 10: every gate open / closed (generic has about half open)"""
    from ai_font_renderer_amd.config import SheetConfig
    cfg = SheetConfig(max_length=max_length, vocab=vocab, sheet_h=1, sheet_w=1)
    raw = synth.make_params(cfg, seed)
    P = {n: torch.from_numpy(raw[STATE[n]]).clone() for n in NAMES}
    if kind == "scores":
        P["w_in"][:2 * E] *= 8.0
    elif kind == "ln":
        P["w_o"].zero_(); P["b_o"].zero_()
        P["pos"][:] = torch.arange(max_length, dtype=torch.float32).unsqueeze(1) * 2.0 ** -10   # constant over a row's channels
        P["w_in"][:E] = 0.0; P["b_in"][:E] = 0.0                # q = 0: the planted magnitudes stay out of the scores (uniform attention)
        v = torch.arange(vocab)
        emb = P["emb"]
        emb[v % 4 == 0] = 0.7
        emb[v % 4 == 1] += 1e3
        emb[v % 4 == 2] *= 1e-4
        emb[v % 4 == 3, 5] *= 1e4
    elif kind == "gate_all":
        P["b1"] += 10.0
    elif kind == "gate_none":
        P["b1"] -= 10.0
    else:
        assert kind == "generic", kind
    return P


RARE = 5                                                          # a code no generated string holds


def strings(B, L, ldx, vocab=128):
    """int64 [B][ldx].  String b is of family b % 5: 0 a dataset string (zero padded, so code 0 occurs); 1 all one code (an occurrence
    chain of length L); 2 one code at positions 0, 7, 15, 24, 41 (distances 7, 8, 9, 17) among distinct codes; 3 all distinct codes
    (L <= vocab); 4 codes 0 and vocab - 1 alternating.  The rare code RARE is planted at position b % L of strings 10, 10 + 256,
    10 + 512 (those that exist), and nowhere else."""
    x = synth.encode_strings(synth.dataset_strings(B), ldx)
    l = np.arange(ldx)
    for b in range(B):
        fam = b % 5
        if fam == 1:
            x[b] = 33 + b % 90
        elif fam == 2:
            x[b] = 6 + (l + 3 * b) % (vocab - 6)
            x[b, [p for p in (0, 7, 15, 24, 41) if p < ldx]] = x[b, 0]
        elif fam == 3:
            x[b] = 6 + (l * 7 + b) % (vocab - 6)
        elif fam == 4:
            x[b] = np.where(l % 2 == 0, 0, vocab - 1)
    assert not (x == RARE).any()
    for b in range(10, B, MAXBLK):
        x[b, b % L] = RARE
    return torch.from_numpy(x)


def make_case(B, L, max_length, mode="train", is_bf16=False, kind="generic", ldx=None, vocab=128, step=3):
    """One launch's inputs.  mode: 'eval' (no dropout description), 'train' (the reference's rates), 'train0' (all rates 0).
    dz is uniform +-1e-3 (rounded to bf16 for a bf16 launch: an exact input)."""
    ldx = L if ldx is None else ldx
    drop = None if mode == "eval" else dict(seed=synth.SEED, step=step, rank=0, p=RATES if mode == "train" else (0.0, 0.0, 0.0))
    dz = torch.from_numpy(synth.hash_uniform(960, (B, max_length * F), 1e-3, seed=synth.SEED + B + L))
    if is_bf16:
        dz = dz.bfloat16().float()
    return dict(B=B, L=L, max_length=max_length, vocab=vocab, ldx=ldx, mode=mode, is_bf16=is_bf16, kind=kind, drop=drop,
                P=params(max_length, vocab, kind), x=strings(B, L, ldx, vocab), dz=dz)


def run(c, dt, fault=None, relu_gate=None, x=None):
    """forward and backward of a case in dtype dt -> (fw, bw)"""
    P = {n: t.to(dt) for n, t in c["P"].items()}
    x = c["x"] if x is None else x
    masks, scales = masks_for(c["B"], c["L"], c["drop"]), scales_for(c["drop"])
    fw = front_fwd(P, x, c["L"], c["max_length"], masks, scales, fault=fault if fault in ("var31", "trip2_codes") else None,
                   relu_gate=relu_gate)
    fwb = fw
    if fault == "recompute_eval":
        fwb = front_fwd(P, x, c["L"], c["max_length"], masks, scales, fault=fault, relu_gate=fw["cache"]["gate"])
    return fw, front_bwd(P, fwb, c["dz"].to(dt), fault)


def bounds(c, fw, bw, reduced=False):
    P = {n: t.double() for n, t in c["P"].items()}
    fb = fwd_bounds(P, fw, c["is_bf16"])
    return fb, bwd_bounds(P, fw, fb, bw, reduced)


L_SWEEP = (1, 2, 3, 15, 16, 17, 63, 64, 65, 100, 119, 120)       # B = 3, max_length 120
TRIPS = ((1, 24), (255, 17), (256, 17), (257, 17), (300, 24), (600, 24))   # max_length 24
SPECIAL = ("scores", "ln", "gate_all", "gate_none")             # at (B, L) = (5, 65), max_length 120
MODES = ("eval", "train", "train0")
