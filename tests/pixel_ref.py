"""Checker for the token kernels of the pixel transformer (csrc/pixel.hip through the afr_op_pixel_* entries): every kernel restated
with its own interface (row-major buffers in, the same outputs out; parameter partials as the total over rows), evaluated in fp64
(the reference) or in float32 (a yardstick for the bounds only -- the restatements compute in the dtype they are handed), the
per-row / per-element error bounds the GPU tests hold the kernels to, and the deterministic inputs both test files share.

Notation of the bounds: U = 2^-24, one float32 rounding to nearest, relative.  A sum of d terms held 8 per lane is 7 adds in the
lane, 6 shuffle levels and a division: 14 roundings, each at most U times a partial sum, which is at most the sum of the
magnitudes.  KD(d) = log2 d + 10 (16 .. 19) is used for that count, so an error of such a MEAN is at most KD U mean|terms|."""
import math

import numpy as np
import torch

from ai_font_renderer_amd import synth

from .util import bf16, ratio  # noqa: F401

U = 2.0 ** -24
EPS = 1e-5                               # config.PixelConfig.ln_eps
FWD_STRIDE = 8192 * 4                    # rows per trip of the forward kernels: pix_grid caps at 8192 blocks of 4 waves
BWD_BLOCKS, BWD_WAVES = 512, 16          # the backward kernels: 512 blocks of 16 waves
BWD_STRIDE = BWD_BLOCKS * BWD_WAVES
ATTN_CHUNK = 256
TINY = 2.0 ** -126                       # an exponential below the smallest normal float may be flushed to zero
KS = 16.0                                # a 64-term dot product: 8 fma in the lane + 3 shuffle levels = 11 roundings, held to 16


def KD(d):
    return math.log2(d) + 10.0


def bwd_blocks(rows):
    return max(1, min(BWD_BLOCKS, (rows + BWD_WAVES - 1) // BWD_WAVES))


def attn_chunk(tokens):
    return min(tokens, ATTN_CHUNK)


# ================================================================================================ restatements
def layernorm(x, g, b, eps=EPS, fault=None):
    """Two-pass LayerNorm over the last axis, biased variance.  -> (out, xhat, rstd).
    fault (tests of the tests): 'unbiased' divides the variance by d - 1; 'no_eps' drops eps; 'dead_mean' takes the mean over the
    next power of two of channels (the lanes that hold no channel counted in)."""
    d = x.shape[-1]
    mu = x.sum(-1, keepdim=True) / ((1 << (d - 1).bit_length()) if fault == "dead_mean" else d)
    xc = x - mu
    var = (xc * xc).sum(-1, keepdim=True) / (d - 1 if fault == "unbiased" else d)
    rstd = torch.rsqrt(var + (0.0 if fault == "no_eps" else eps))
    xhat = xc * rstd
    return xhat * g + b, xhat, rstd


def f32_round(t):
    """the float32 value of t, in t's dtype: what a float32 buffer hands to the next operation"""
    return t.float().to(t.dtype)


def add_ln(hin, pos, add, g, b, tokens, rows, eps=EPS, fault=None, h_f32=False):
    """pixel_add_ln: h = (pos ? pos[r % tokens] : hin[r]) + (add ? add[r] : 0); n = LayerNorm(h) g + b (None without g).  h_f32: h is
    rounded to float32, as the kernel stores it, before the LayerNorm reads it (the checks; off, the function is the plain model)."""
    if pos is not None:
        h = pos[torch.arange(rows) % tokens]
    else:
        h = hin
    if add is not None:
        h = f32_round(h + add) if h_f32 else h + add
    n = None if g is None else layernorm(h, g, b, eps, fault)[0]
    return h, n


def head(hin, add, g, b, w, bo, eps=EPS, loss="mse", fault=None, h_f32=False):
    """pixel_head: h = hin + add (h_f32: rounded to float32 as stored); u = LayerNorm(h) g + b . w + bo; y = clamp(u, 0, 1) | sigmoid(u)."""
    h = f32_round(hin + add) if h_f32 else hin + add
    u = (layernorm(h, g, b, eps, fault)[0] * w).sum(-1) + bo
    return h, u, (torch.sigmoid(u) if loss == "bce" else u.clamp(0.0, 1.0))


def _ln_bwd_row(x, dy, g, eps, fault):
    d = x.shape[-1]
    _, xh, rstd = layernorm(x, g, torch.zeros_like(g), eps, fault)
    gg = dy * g
    m1 = gg.sum(-1, keepdim=True) / d
    m2 = (gg * xh).sum(-1, keepdim=True) / d
    return (gg - m1 - xh * m2) * rstd, xh


def head_bwd(du, hf, g, b, w, eps=EPS, fault=None, row_weight=None):
    """pixel_head_bwd: dh = LayerNorm-backward(du w; x = hf); partial totals [4][d] = dgamma, dbeta, dw_out, (db_out, 0, ...).
    row_weight [rows]: factor on every row's contribution to the totals (1; a fault plants zeros)."""
    dy = du.unsqueeze(-1) * w
    dx, xh = _ln_bwd_row(hf, dy, g, eps, fault)
    rw = torch.ones_like(du) if row_weight is None else row_weight.to(du.dtype)
    dyw = dy * rw.unsqueeze(-1)
    part = torch.zeros(4, hf.shape[-1], dtype=hf.dtype)
    part[0], part[1] = (dyw * xh).sum(0), dyw.sum(0)
    part[2] = ((du * rw).unsqueeze(-1) * (xh * g + b)).sum(0)
    part[3, 0] = (du * rw).sum()
    return dx, part


def ln_bwd(dy, hin, g, dh, eps=EPS, fault=None, row_weight=None):
    """pixel_ln_bwd: dh + LayerNorm-backward(dy; x = hin); partial totals [2][d] = dgamma, dbeta."""
    dx, xh = _ln_bwd_row(hin, dy, g, eps, fault)
    dyw = dy if row_weight is None else dy * row_weight.to(dy.dtype).unsqueeze(-1)
    return dh + dx, torch.stack([(dyw * xh).sum(0), dyw.sum(0)])


def _heads(t, B, tokens):
    return t.reshape(B, tokens, -1, 64)


def _kv(kv):
    B, C, d2 = kv.shape
    d = d2 // 2
    return kv[:, :, :d].reshape(B, C, -1, 64), kv[:, :, d:].reshape(B, C, -1, 64)


def softmax2(s):
    """max-subtracted softmax over axis 2 of s [B, tokens, C, H]"""
    e = torch.exp(s - s.amax(2, keepdim=True))
    return e / e.sum(2, keepdim=True)


def attn(q, kv, tokens):
    """pixel_attn: o[r] per head = softmax_c((q / 8) . k_c) . v_c;  q [rows][d], kv [B][C][2 d] = [k | v]."""
    B = kv.shape[0]
    k, v = _kv(kv)
    s = torch.einsum("bthe,bche->btch", _heads(q * 0.125, B, tokens), k)
    return torch.einsum("btch,bche->bthe", softmax2(s), v).reshape(q.shape)


def attn_bwd(dO, q, kv, tokens, fault=None, row_weight=None):
    """pixel_attn_bwd: -> dq [rows][d], dkv [B][4 d] = [dk_0 | dv_0 | dk_1 | dv_1] summed over the sample's tokens (C == 1: the
    second half zero).  fault: 'dq_scale' leaves the 1/8 out of dq; 'swap_dv' weighs dv_0 with p_1 and dv_1 with p_0."""
    B, C = kv.shape[:2]
    d = q.shape[-1]
    k, v = _kv(kv)
    qs, do = _heads(q * 0.125, B, tokens), _heads(dO, B, tokens)
    p = softmax2(torch.einsum("bthe,bche->btch", qs, k))
    dp = torch.einsum("bthe,bche->btch", do, v)
    ds = p * (dp - (p * dp).sum(2, keepdim=True))
    dq = torch.einsum("btch,bche->bthe", ds, k) * (1.0 if fault == "dq_scale" else 0.125)
    if row_weight is not None:
        rw = row_weight.to(q.dtype).reshape(B, tokens, 1, 1)
        qs, do = qs * rw, do * rw
    dk = torch.einsum("btch,bthe->bche", ds, qs).reshape(B, C, d)
    dv = torch.einsum("btch,bthe->bche", p.flip(2) if fault == "swap_dv" else p, do).reshape(B, C, d)
    dkv = torch.zeros(B, 2, 2 * d, dtype=q.dtype)
    dkv[:, :C, :d], dkv[:, :C, d:] = dk, dv
    return dq.reshape(q.shape), dkv.reshape(B, 4 * d)


def ctx(emb, femb, x, font):
    """pixel_ctx: [B][C][d] = Emb[x] (, Font[font])"""
    rows = [emb[x]] + ([femb[font]] if femb is not None else [])
    return torch.stack(rows, 1)


def ctx_bwd(dctx, x, font, vocab, n_fonts):
    """pixel_ctx_bwd: the scatter-add of dctx [B][C][d] into the table rows; rows no glyph uses are zero"""
    demb = torch.zeros(vocab, dctx.shape[-1], dtype=dctx.dtype).index_add_(0, x, dctx[:, 0])
    dfont = torch.zeros(n_fonts, dctx.shape[-1], dtype=dctx.dtype).index_add_(0, font, dctx[:, 1]) if n_fonts > 0 else None
    return demb, dfont


def stale_row(out, r, stride):
    """fault: row r of an output computed from the inputs one stride earlier (a prefetch register handed over late)"""
    out = out.clone()
    out[r] = out[r - stride]
    return out


def wave_rows(rows, wave=BWD_WAVES - 1):
    """row_weight of the fault 'the last wave's partial left out of block 0's slab': zero on the rows that wave walks"""
    w = torch.ones(rows, dtype=torch.float64)
    w[wave::bwd_blocks(rows) * BWD_WAVES] = 0.0
    return w


# ================================================================================================ bounds (fp64 tensors in)
def _ln_err(x, eps):
    """-> xhat, rstd, em, rr.  em [rows,1]: error of the mean, KD U mean|x|.  rr: relative error of rstd -- the variance is a
    mean of squares of values that each carry 2 roundings ((KD + 4) U relative, not halved by the root: slack for rsqrt's own
    ulp), and every centred value is shifted by the mean's error, which adds em^2 to the variance: (em rstd)^2 relative."""
    d = x.shape[-1]
    mu = x.mean(-1, keepdim=True)
    xc = x - mu
    rstd = torch.rsqrt((xc * xc).mean(-1, keepdim=True) + eps)
    em = KD(d) * U * x.abs().mean(-1, keepdim=True)
    return xc * rstd, rstd, em, (KD(d) + 4.0) * U + (em * rstd) ** 2


def bound_ln(x, g, b, eps=EPS):
    """[rows, 1] bound on n = xhat g + b.  xhat = (x - mu) rstd: the mean's error em moves every xhat by em rstd (times max|g|);
    rstd's relative error rr and the 3 roundings of (x - mu), * rstd and the fma act on max|xhat g|; the fma's result rounds
    once more on the output: 4 U (max|xhat g| + max|b|) covers the final roundings (2^-22 scale)."""
    xh, rstd, em, rr = _ln_err(x, eps)
    amp = (xh * g).abs().amax(-1, keepdim=True)
    return em * rstd * g.abs().max() + rr * amp + 4.0 * U * (amp + b.abs().max())


def bound_head_u(x, g, b, w, bo, eps=EPS):
    """[rows] bound on u = sum_j n_j w_j + bo.  The mean's error is ONE number per row, so it moves u by em rstd |sum g w|; rstd's
    error scales sum|xhat g w|; the per-channel roundings (3 in n, the product) and the d-term sum ((KD + 6) U together) act on
    sum|n_j w_j| <= sum|xhat g w| + sum|b w|; adding bo rounds once."""
    xh, rstd, em, rr = _ln_err(x, eps)
    s2 = (xh * g * w).abs().sum(-1)
    bu = (em * rstd).squeeze(-1) * (g * w).sum().abs() + rr.squeeze(-1) * s2 + (KD(x.shape[-1]) + 6.0) * U * (s2 + (b * w).abs().sum())
    return bu + 2.0 * U * (abs(float(bo)) + bu)


def bound_y(bu, loss):
    """clamp is 1-Lipschitz: the bound of u.  sigmoid is 1/4-Lipschitz; the fast exponential, the reciprocal and the argument
    scaling add 3 roundings of a value <= 1: 2^-21 absolute with slack."""
    return 0.25 * bu + 2.0 ** -21 if loss == "bce" else bu


def bound_ln_bwd(x, dy, g, eps=EPS, cdy=1.0):
    """-> (bdx [rows, d], exh [rows, d]) for dx = (gg - m1 - xhat m2) rstd, gg = dy g, m1 = mean gg, m2 = mean gg xhat.
    exh: error of xhat = em rstd + (rr + 2 U)|xhat|.  gg carries cdy roundings (1; 2 when dy = du w is formed in the kernel).
    e1 = (KD + cdy) U mean|gg|;  e2 = (KD + 2 + cdy) U mean|gg xhat| + mean(|gg| exh).  The bracket adds exh |m2| + |xhat| e2
    and 3 roundings of its own terms; the factor rstd and the
    final rounding contribute (rr + 4 U)|dx|."""
    d = x.shape[-1]
    xh, rstd, em, rr = _ln_err(x, eps)
    exh = em * rstd + (rr + 2.0 * U) * xh.abs()
    gg = dy * g
    m1, m2 = gg.mean(-1, keepdim=True), (gg * xh).mean(-1, keepdim=True)
    e1 = (KD(d) + cdy) * U * gg.abs().mean(-1, keepdim=True)
    e2 = (KD(d) + 2.0 + cdy) * U * (gg * xh).abs().mean(-1, keepdim=True) + (gg.abs() * exh).mean(-1, keepdim=True)
    dx = (gg - m1 - xh * m2) * rstd
    br = (cdy + 1.0) * U * gg.abs() + e1 + exh * m2.abs() + xh.abs() * e2 + 3.0 * U * (gg.abs() + m1.abs() + (xh * m2).abs())
    return br * rstd + (rr + 4.0 * U) * dx.abs(), exh


def bwd_nsum(rows, reduced):
    """the longest chain of float32 additions behind one element of a slab total: a wave's rows in sequence, the 16 waves in
    sequence, and (reduced: the slabs summed on the device, taken as sequential) the slabs; on the host the slabs add in fp64."""
    nb = bwd_blocks(rows)
    return -(-rows // (nb * BWD_WAVES)) + BWD_WAVES + (nb if reduced else 0)


def bound_head_bwd_part(du, hf, g, b, w, nsum, eps=EPS):
    """[4][d]: dgamma_j = sum_r dy_j xhat_j: sum_r |dy_j| exh_j + (nsum + 3) U sum_r |dy_j xhat_j| (the products carry dy's rounding,
    their own and the fma's); dbeta_j = sum_r dy_j: (nsum + 1) U sum|dy_j|; dw_out_j = sum_r du n_j with n the LayerNorm output:
    sum_r |du| bound_ln + (nsum + 2) U sum|du n_j|; db_out = sum du: nsum U sum|du|."""
    dy = du.unsqueeze(-1) * w
    xh, _, _, _ = _ln_err(hf, eps)
    _, exh = bound_ln_bwd(hf, dy, g, eps, 2.0)
    out = torch.zeros(4, hf.shape[-1], dtype=torch.float64)
    out[0] = (dy.abs() * exh).sum(0) + (nsum + 3.0) * U * (dy * xh).abs().sum(0)
    out[1] = (nsum + 1.0) * U * dy.abs().sum(0)
    out[2] = (du.abs().unsqueeze(-1) * bound_ln(hf, g, b, eps)).sum(0) + (nsum + 2.0) * U * (du.unsqueeze(-1) * (xh * g + b)).abs().sum(0)
    out[3, 0] = nsum * U * du.abs().sum()
    return out


def bound_ln_bwd_part(dy, hin, g, nsum, eps=EPS):
    """[2][d]: as the first two rows of bound_head_bwd_part with dy an input (no rounding of its own)."""
    xh, _, _, _ = _ln_err(hin, eps)
    _, exh = bound_ln_bwd(hin, dy, g, eps, 1.0)
    return torch.stack([(dy.abs() * exh).sum(0) + (nsum + 2.0) * U * (dy * xh).abs().sum(0), nsum * U * dy.abs().sum(0)])


def _attn_err(q, kv, tokens):
    """-> p, dpr [B, tokens, C, H]: the probabilities and their error.  A score s_c = (q/8) . k_c carries KS U sum|q k_c|/8.  The
    larger score's exponential is exp(0) = 1 exactly; the other is exp(-D), D = |s_0 - s_1|, evaluated as exp2(D log2 e): the
    subtraction and the argument scaling round D (2 U D), the instruction rounds once: relative (2 D + 4) U with slack, or TINY
    absolute where the result is flushed.  p = e / (e_0 + e_1) moves by p (1 - p) times the relative error of e_0 / e_1, plus 3
    roundings (sum, reciprocal, product) of p itself."""
    B, C = kv.shape[:2]
    k, _ = _kv(kv)
    qs = _heads(q * 0.125, B, tokens)
    s = torch.einsum("bthe,bche->btch", qs, k)
    p = softmax2(s)
    if C == 1:
        return p, torch.zeros_like(p)
    es = (KS * U * torch.einsum("bthe,bche->btch", qs.abs(), k.abs())).sum(2, keepdim=True)
    D = (s[:, :, :1] - s[:, :, 1:]).abs()
    return p, p * (1.0 - p) * (es + (2.0 * D + 4.0) * U) + 3.0 * U * p + TINY


def bound_attn(q, kv, tokens):
    """[rows][d] bound on o_j = p_0 v_0j + p_1 v_1j: sum_c dpr_c |v_cj| + 4 U sum_c p_c |v_cj| (product, fma, output).  C == 1: o is
    a copy of v -- the bound is 0."""
    B, C = kv.shape[:2]
    _, v = _kv(kv)
    p, dpr = _attn_err(q, kv, tokens)
    if C == 1:
        return torch.zeros(q.shape, dtype=torch.float64)
    return (torch.einsum("btch,bche->bthe", dpr, v.abs()) + 4.0 * U * torch.einsum("btch,bche->bthe", p, v.abs())).reshape(q.shape)


def attn_nsum(tokens, reduced):
    """a wave's tokens of one chunk in sequence, the 16 waves in sequence, and (reduced) the chunk slabs"""
    ch = attn_chunk(tokens)
    return -(-ch // BWD_WAVES) + BWD_WAVES + (-(-tokens // ch) if reduced else 0)


def bound_attn_bwd(dO, q, kv, tokens, nsum):
    """-> (bdq [rows][d], bdkv [B][4 d]).  dp_c = dO . v_c carries edp_c = KS U sum|dO v_c|.  dot = p_0 dp_0 + p_1 dp_1:
    ddot = sum_c (p_c edp_c + dpr_c |dp_c|) + 3 U sum_c p_c |dp_c|.  ds_c = p_c (dp_c - dot): p_c (edp_c + ddot + 2 U (|dp_c| + |dot|))
    + dpr_c |dp_c - dot| + U |ds_c|.  dq_j = (ds_0 k_0j + ds_1 k_1j) / 8: sum_c (dds_c |k_cj| + 4 U |ds_c k_cj|) / 8.
    dk_cj = sum_t ds_c q_j / 8: sum_t dds_c |q_j| / 8 + (nsum + 1) U sum_t |ds_c q_j| / 8;  dv_cj = sum_t p_c dO_j likewise with dpr_c.
    C == 1: ds is an exact zero (dq = dk = 0 exactly) and dv = sum_t dO_j: nsum U sum|dO_j|."""
    B, C = kv.shape[:2]
    d = q.shape[-1]
    k, v = _kv(kv)
    qs, do = _heads(q * 0.125, B, tokens), _heads(dO, B, tokens)
    bdkv = torch.zeros(B, 2, 2 * d, dtype=torch.float64)
    if C == 1:
        bdkv[:, 0, d:] = nsum * U * do.abs().sum(1).reshape(B, d)
        return torch.zeros(q.shape, dtype=torch.float64), bdkv.reshape(B, 4 * d)
    p, dpr = _attn_err(q, kv, tokens)
    dp = torch.einsum("bthe,bche->btch", do, v)
    edp = KS * U * torch.einsum("bthe,bche->btch", do.abs(), v.abs())
    dot = (p * dp).sum(2, keepdim=True)
    ddot = (p * edp + dpr * dp.abs()).sum(2, keepdim=True) + 3.0 * U * (p * dp.abs()).sum(2, keepdim=True)
    ds = p * (dp - dot)
    dds = p * (edp + ddot + 2.0 * U * (dp.abs() + dot.abs())) + dpr * (dp - dot).abs() + U * ds.abs()
    bdq = 0.125 * (torch.einsum("btch,bche->bthe", dds, k.abs()) + 4.0 * U * torch.einsum("btch,bche->bthe", ds.abs(), k.abs()))
    bdkv[:, :, :d] = (torch.einsum("btch,bthe->bche", dds, qs.abs()) + (nsum + 1.0) * U * torch.einsum("btch,bthe->bche", ds.abs(), qs.abs())).reshape(B, C, d)
    bdkv[:, :, d:] = (torch.einsum("btch,bthe->bche", dpr, do.abs()) + (nsum + 1.0) * U * torch.einsum("btch,bthe->bche", p, do.abs())).reshape(B, C, d)
    return bdq.reshape(q.shape), bdkv.reshape(B, 4 * d)


def bound_T(bound, ref, is_bf16):
    """an output stored in T: bf16 adds 2^-8 |ref| -- one rounding to nearest is 2^-9, the float32 error may carry it across a tie"""
    return bound + 2.0 ** -8 * ref.abs() if is_bf16 else bound


# ================================================================================================ inputs
GROUP = 5                                                        # rows of a planted group: probe, constant, mean 1e3, 1e-4, one channel x 1e4
_BASE_ROWS = 1021


def fill(tid, rows, d, amp=1.0):
    """[rows][d] float32 at unit scale (times amp): a hashed block of 1021 rows (synth.hash_uniform), gathered through a row walk
    that does not repeat within any two trips of a kernel, each row scaled by its own factor in [0.5, 1.5) -- a row taken from
    one stride earlier or later is a different row.  Costs a gather, not a hash, per element: the largest cases have 2e7 of them."""
    base = synth.hash_uniform(tid, (_BASE_ROWS, d), 1.0)
    r = np.arange(rows, dtype=np.int64)
    idx = (r * 389 + (r // _BASE_ROWS) * 17) % _BASE_ROWS
    sc = (0.5 + ((r * 2654435761 >> 11) & 63) / 64.0).astype(np.float32)
    return torch.from_numpy(base[idx] * sc[:, None] * np.float32(amp))


def anchors(rows, stride):
    """first rows of the planted groups: row 0, the last GROUP rows, and the first and last GROUP rows of every later trip"""
    cand = [0, rows - GROUP]
    for t in range(stride, rows, stride):
        cand += [t, min(t + stride, rows) - GROUP]
    out = []
    for a in cand:
        if a >= 0 and all(abs(a - o) >= GROUP for o in out):
            out.append(a)
    return sorted(out) if out else [0]


def edge_group(tid, d):
    """[GROUP][d]: a unit-scale probe row, a constant row (variance 0), mean 1e3 with unit spread, 1e-4 magnitude, one channel 1e4
    times the rest"""
    gq = torch.from_numpy(synth.hash_uniform(tid, (GROUP, d), 1.0)).clone()
    gq[1] = 0.37
    gq[2] += 1000.0
    gq[3] *= 1e-4
    gq[4, 5] = 1e4 * (0.5 + gq[4, 5].abs())
    return gq


def plant(x, group, anc):
    """write the group at every anchor (cut where the buffer ends)"""
    for a in anc:
        n = min(GROUP, x.shape[0] - a)
        x[a:a + n] = group[:n]
    return x


def affine(tid, d):
    """LayerNorm weight 1 + 0.5 u, bias 0.3 u, an output weight 0.2 u and bias (u uniform in [-1, 1])"""
    g = 1.0 + torch.from_numpy(synth.hash_uniform(tid, (d,), 0.5))
    b = torch.from_numpy(synth.hash_uniform(tid + 1, (d,), 0.3))
    w = torch.from_numpy(synth.hash_uniform(tid + 2, (d,), 0.2))
    return g, b, w, torch.tensor([0.25])


def ln_inputs(rows, d, stride, tokens=None, tid=700):
    """hin, add, dy [rows][d] float32, a residual dh, du [rows], pos [tokens][d] and the anchors.  hin carries the edge group at every
    anchor and add is zero there except on the probe row, so hin + add IS the planted row; dy, dh, du repeat one group of their
    own at the anchors (the bitwise row-locality check needs equal inputs).  pos (given tokens) holds the edge group at the anchors'
    token positions; pos_anchors are the anchors whose positions no earlier anchor claimed for another row of the group."""
    anc = anchors(rows, stride)
    hin = plant(fill(tid, rows, d), edge_group(tid + 10, d), anc)
    addg = torch.zeros(GROUP, d)
    addg[0] = torch.from_numpy(synth.hash_uniform(tid + 11, (d,), 1.0))
    add = plant(fill(tid + 1, rows, d, 0.5), addg, anc)
    dy = plant(fill(tid + 2, rows, d), torch.from_numpy(synth.hash_uniform(tid + 12, (GROUP, d), 1.0)), anc)
    dh = plant(fill(tid + 3, rows, d), torch.from_numpy(synth.hash_uniform(tid + 13, (GROUP, d), 1.0)), anc)
    du = plant(fill(tid + 4, rows, 1), torch.from_numpy(synth.hash_uniform(tid + 14, (GROUP, 1), 1.0)), anc).reshape(rows)
    pos, pos_anc = None, []
    if tokens is not None:
        pos = torch.from_numpy(synth.hash_uniform(tid + 5, (tokens, d), 1.0)).clone()
        eg, owner = edge_group(tid + 10, d), {}
        for a in anc:
            span = [((a + i) % tokens, i) for i in range(min(GROUP, rows - a))]
            if all(owner.get(t, i) == i for t, i in span):
                pos_anc.append(a)
                for t, i in span:
                    owner[t] = i
                    pos[t] = eg[i]
    return dict(hin=hin, add=add, dy=dy, dh=dh, du=du, pos=pos, anchors=anc, pos_anchors=pos_anc)


GAPS = (0.0, 0.5, 30.0, -100.0, -3.0, -30.0, 100.0, 1e-30)


def attn_inputs(B, tokens, d, C, stride, is_bf16=False, tid=760):
    """q, dO [B * tokens][d], kv [B][C][2 d] (float32 values, already rounded to bf16 when is_bf16) and the anchors.  Every sample
    that holds an anchor shares one kv (equal inputs for the row-locality check); where a sample holds none, its head 0 has
    k_1 = k_0: exactly equal scores under any q.  With two keys, head h of group row i has q = 8 gap (k_0 - k_1) / |k_0 - k_1|^2 for
    gap = GAPS[(i + h) % 8]: scores that differ by exactly 0 (q = 0), by about 1e-30, moderately, and by +-30 and +-100, where
    one probability rounds to zero or underflows."""
    rows = B * tokens
    anc = anchors(rows, stride)
    rnd = bf16 if is_bf16 else (lambda t: t)
    kv = torch.from_numpy(synth.hash_uniform(tid, (B, C, 2 * d), 1.0)).clone()
    held = sorted({(a + i) // tokens for a in anc for i in range(min(GROUP, rows - a))})
    kv[held] = kv[held[0]].clone()
    if C == 2:
        for b in range(B):
            if b not in held:
                kv[b, 1, :64] = kv[b, 0, :64]
    kv = rnd(kv)
    q = fill(tid + 1, rows, d)
    dO = plant(fill(tid + 2, rows, d), torch.from_numpy(synth.hash_uniform(tid + 12, (GROUP, d), 1.0)), anc)
    qg = torch.from_numpy(synth.hash_uniform(tid + 11, (GROUP, d), 1.0)).clone()
    if C == 2:
        k = kv[held[0], :, :d].double().reshape(2, -1, 64)
        dk = k[0] - k[1]
        for i in range(GROUP):
            for h in range(d // 64):
                gap = GAPS[(i + h) % 8]
                qg[i, 64 * h:64 * h + 64] = (8.0 * gap * dk[h] / (dk[h] * dk[h]).sum()).float()
    q = plant(q, qg, anc)
    return dict(q=rnd(q), dO=rnd(dO), kv=kv, anchors=anc)


def ctx_inputs(B, d, vocab=128, n_fonts=3, tid=790):
    """tables, repeated codes (code 65 in every third glyph), codes and fonts nobody uses, dctx [B][C][d]"""
    emb = torch.from_numpy(synth.hash_uniform(tid, (vocab, d), 1.0))
    femb = torch.from_numpy(synth.hash_uniform(tid + 1, (n_fonts, d), 1.0)) if n_fonts else None
    i = np.arange(B)
    x = torch.from_numpy(np.where(i % 3 == 0, 65, 32 + (i * 7) % 90).astype(np.int64))
    font = torch.from_numpy((i % max(n_fonts - 1, 1)).astype(np.int64)) if n_fonts else None       # the last font is never used
    dctx = torch.from_numpy(synth.hash_uniform(tid + 2, (B, 2 if n_fonts else 1, d), 1.0))
    return dict(emb=emb, femb=femb, x=x, font=font, dctx=dctx, vocab=vocab, n_fonts=n_fonts)


# the cases both test files walk: (rows as B x tokens, widths, ...).  Arithmetic of the trips is stated where the GPU tests list them.
WIDTHS = (64, 192, 320, 512)
FWD_SMALL = ((1, 3), (3, 7), (5, 24))                            # 3 rows (idle waves), 21 rows (not a multiple of 4), 120 rows (30 blocks)
FWD_TRIPS = ((8, 4096), (9, 4104), (17, 4104))                   # 32768 = exactly one trip; 36936 = 1.13 trips; 69768 = 2.13 trips
BWD_SMALL = ((1, 3), (3, 7), (5, 24), (3, 1000))                 # 3, 21, 120 rows (8 slabs), 3000 rows (188 slabs < 512)
BWD_TRIPS = ((2, 4096), (3, 4104), (7, 4104))                    # 8192 = exactly one trip; 12312 = 1.5 trips; 28728 = 3.5 trips
ATTN_BWD_TOKENS = (8, 200, 256, 264, 520)


# ================================================================================================ one case = inputs + run + bounds
def _c(t, dt):
    return None if t is None else t.to(dt)


def _T(t, is_bf16):
    """a buffer of the activation type T: its values rounded to bf16 in bf16 mode (kept as float32 numbers here)"""
    return bf16(t) if is_bf16 and t is not None else t


def add_ln_case(B, tokens, d, mode, is_bf16):
    """mode 'pos': the first block (h = pos[r % tokens], no add); 'add': h = hin + add with n; 'no_n': h = hin + add only"""
    rows = B * tokens
    I = ln_inputs(rows, d, FWD_STRIDE, tokens if mode == "pos" else None)
    g, b, _, _ = affine(720, d)
    pos = mode == "pos"
    return dict(rows=rows, tokens=tokens, d=d, is_bf16=is_bf16, mode=mode, stride=FWD_STRIDE, hin=None if pos else I["hin"], pos=I["pos"],
                add=None if pos else _T(I["add"], is_bf16), g=None if mode == "no_n" else g, b=None if mode == "no_n" else b,
                anchors=I["pos_anchors"] if pos else I["anchors"])


def add_ln_run(c, dt, fault=None):
    h, n = add_ln(_c(c["hin"], dt), _c(c["pos"], dt), _c(c["add"], dt), _c(c["g"], dt), _c(c["b"], dt), c["tokens"], c["rows"], fault=fault, h_f32=True)
    return dict(h=h) if n is None else dict(h=h, n=n)


def add_ln_bounds(c, ref):
    """h: a copy (bound 0) or one float32 addition, held to 4 U |h| like every final rounding (a correctly rounded result may use
    all of U |h|; the quarter rule of the float32 yardstick needs the 4); n: bound_ln on the stored h"""
    out = dict(h=torch.zeros(1, dtype=torch.float64) if c["add"] is None else 4.0 * U * ref["h"].abs())
    if "n" in ref:
        out["n"] = bound_T(bound_ln(ref["h"], c["g"].double(), c["b"].double()), ref["n"], c["is_bf16"])
    return out


def head_case(B, tokens, d, loss, is_bf16):
    rows = B * tokens
    I = ln_inputs(rows, d, FWD_STRIDE)
    g, b, w, bo = affine(730, d)
    # the output weight leans on the probe row: w += 0.1 (probe - mean) / max|probe - mean|.  With a purely random w the
    # LayerNorm part of the probe row's u is a sum of d signed terms near zero, and a wrong rstd (its only effect on u) hides
    # below the bound of the d-term sum -- at d = 512 the 3-row case, whose one ordinary row is the probe, did not see the
    # unbiased-variance fault.  Leaning w makes that part of u about 0.1 d std: every case sees the row's scale in u.
    pc = I["hin"][0] + I["add"][0]
    pc = pc - pc.mean()
    w = w + 0.1 * pc / pc.abs().max()
    return dict(rows=rows, tokens=tokens, d=d, is_bf16=is_bf16, loss=loss, stride=FWD_STRIDE, hin=I["hin"], add=_T(I["add"], is_bf16), g=g, b=b, w=w,
                bo=bo, anchors=I["anchors"])


def head_run(c, dt, fault=None):
    h, u, y = head(_c(c["hin"], dt), _c(c["add"], dt), _c(c["g"], dt), _c(c["b"], dt), _c(c["w"], dt), _c(c["bo"], dt), loss=c["loss"], fault=fault, h_f32=True)
    return dict(h=h, u=u, y=y)


def head_bounds(c, ref):
    bu = bound_head_u(ref["h"], c["g"].double(), c["b"].double(), c["w"].double(), c["bo"].double())
    return dict(h=4.0 * U * ref["h"].abs(), u=bu, y=bound_y(bu, c["loss"]))


def head_bwd_case(B, tokens, d, is_bf16):
    rows = B * tokens
    I = ln_inputs(rows, d, BWD_STRIDE)
    g, b, w, _ = affine(740, d)
    return dict(rows=rows, tokens=tokens, d=d, is_bf16=is_bf16, stride=BWD_STRIDE, du=I["du"], hf=I["hin"], g=g, b=b, w=w, anchors=I["anchors"])


def head_bwd_run(c, dt, fault=None, row_weight=None):
    dh, part = head_bwd(_c(c["du"], dt), _c(c["hf"], dt), _c(c["g"], dt), _c(c["b"], dt), _c(c["w"], dt), fault=fault, row_weight=row_weight)
    return dict(dh=dh, part=part)


def head_bwd_bounds(c, ref, reduced=False):
    du, hf, g, b, w = (c[k].double() for k in ("du", "hf", "g", "b", "w"))
    return dict(dh=bound_ln_bwd(hf, du.unsqueeze(-1) * w, g, cdy=2.0)[0], part=bound_head_bwd_part(du, hf, g, b, w, bwd_nsum(c["rows"], reduced)))


def ln_bwd_case(B, tokens, d, is_bf16):
    rows = B * tokens
    I = ln_inputs(rows, d, BWD_STRIDE, tid=750)
    g, _, _, _ = affine(755, d)
    return dict(rows=rows, tokens=tokens, d=d, is_bf16=is_bf16, stride=BWD_STRIDE, dy=_T(I["dy"], is_bf16), hin=I["hin"], g=g, dh=I["dh"], anchors=I["anchors"])


def ln_bwd_run(c, dt, fault=None, row_weight=None):
    dh, part = ln_bwd(_c(c["dy"], dt), _c(c["hin"], dt), _c(c["g"], dt), _c(c["dh"], dt), fault=fault, row_weight=row_weight)
    return dict(dh=dh, part=part)


def ln_bwd_bounds(c, ref, reduced=False):
    dy, hin, g = c["dy"].double(), c["hin"].double(), c["g"].double()
    return dict(dh=bound_ln_bwd(hin, dy, g)[0] + 4.0 * U * ref["dh"].abs(), part=bound_ln_bwd_part(dy, hin, g, bwd_nsum(c["rows"], reduced)))


def attn_case(B, tokens, d, C, is_bf16, stride=FWD_STRIDE):
    I = attn_inputs(B, tokens, d, C, stride, is_bf16)
    return dict(rows=B * tokens, B=B, tokens=tokens, d=d, C=C, is_bf16=is_bf16, stride=stride, **I)


def attn_run(c, dt, fault=None):
    return dict(o=attn(_c(c["q"], dt), _c(c["kv"], dt), c["tokens"]))


def attn_bounds(c, ref):
    return dict(o=bound_T(bound_attn(c["q"].double(), c["kv"].double(), c["tokens"]), ref["o"], c["is_bf16"]))


def attn_bwd_case(B, tokens, d, C, is_bf16):
    return attn_case(B, tokens, d, C, is_bf16, stride=2 * tokens)


def attn_bwd_run(c, dt, fault=None, row_weight=None):
    dq, dkv = attn_bwd(_c(c["dO"], dt), _c(c["q"], dt), _c(c["kv"], dt), c["tokens"], fault=fault, row_weight=row_weight)
    return dict(dq=dq, dkv=dkv)


def attn_bwd_bounds(c, ref, reduced=False):
    bdq, bdkv = bound_attn_bwd(c["dO"].double(), c["q"].double(), c["kv"].double(), c["tokens"], attn_nsum(c["tokens"], reduced))
    return dict(dq=bound_T(bdq, ref["dq"], c["is_bf16"]), dkv=bdkv)


def bound_ctx_bwd(dctx, x, font, vocab, n_fonts):
    """a table row is a sequential float32 sum over the B glyphs: B U sum|terms|"""
    demb, dfont = ctx_bwd(dctx.abs(), x, font, vocab, n_fonts)
    B = dctx.shape[0]
    return B * U * demb, None if dfont is None else B * U * dfont


def fwd_cases():
    """(B, tokens, d) of the forward kernels: the small sizes at every width; one, 1.13 and 2.13 trips at d = 64; one and 1.13 trips
    at d = 512 (three trips at d = 512 would be 143 MB per float32 buffer and ten times that for its fp64 reference)"""
    out = [(B, t, d) for d in WIDTHS for B, t in FWD_SMALL]
    return out + [(B, t, 64) for B, t in FWD_TRIPS] + [(B, t, 512) for B, t in FWD_TRIPS[:2]]


def bwd_cases():
    """the small sizes at every width; one, 1.5 and 3.5 trips at d = 64; 1.5 and 3.5 trips at d = 512"""
    out = [(B, t, d) for d in WIDTHS for B, t in BWD_SMALL]
    return out + [(B, t, 64) for B, t in BWD_TRIPS] + [(B, t, 512) for B, t in BWD_TRIPS[1:]]


def attn_bwd_cases():
    """(B, tokens, d, C): every token count with B = 1 and 3 at d = 64 and 192, C = 2; one of each at C = 1 and at the widest"""
    out = [(B, t, d, 2) for t in ATTN_BWD_TOKENS for B, d in ((1, 64), (3, 192))]
    return out + [(3, 520, 64, 1), (1, 8, 320, 1), (3, 264, 512, 2), (1, 520, 320, 2)]
