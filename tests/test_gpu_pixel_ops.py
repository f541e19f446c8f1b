"""GPU: the token kernels of the pixel transformer (csrc/pixel.hip), ONE launch each through the afr_op_pixel_* entries, every
output element against the fp64 restatement of tests/pixel_ref.py under its derived per-row / per-element bound.  The row counts
drive the grid-stride loops through none, part of, exactly one and several extra trips, with the planted rows (constant, mean 1e3,
1e-4, one channel x 1e4; score gaps 0 .. +-100) at the first and last rows of every trip.  Besides the error, each case checks:
outputs pre-filled with NaN hold none afterwards (every slab included); guard bands of one row (256 bytes at the least) in front of
and behind every output keep their bits (tests/op_harness.py); the planted groups, equal in content, give bit-identical output rows wherever they sit (row locality); a second launch
repeats the first bit for bit; dhT is bf16(dh) exactly; h is the float32 sum exactly.

Every case prints its largest error as a fraction of the bound (pytest -s).  Measured on MI355X, the largest per kernel:
    add_ln    n 0.995 (a bf16 output), h exact
    attn      o 0.996 (a bf16 output)
    head      u 0.054, y 0.054, h exact
    head_bwd  dh 0.119, slab totals 0.059 (summed in fp64) / 0.059 (afr_op_reduce)
    ln_bwd    dh 0.244, slab totals 0.122 / 0.128
    attn_bwd  dq 0.991 (a bf16 output), dk | dv 0.104 / 0.099
    ctx_bwd   0.187
The values near 1 belong to bf16 outputs: one rounding to bf16 at the bottom of a binade is the 2^-8 |ref| term of the bound itself."""
import ctypes as C

import pytest
import torch

from ai_font_renderer_amd import _lib
from . import pixel_ref as R
from .gpu_util import dev, ptr, stream
from .op_harness import Outs, bits, dt, judge, tt, twice

pytestmark = pytest.mark.gpu
F64 = torch.float64


def _locality(c, got, keys):
    """the planted groups hold the same rows at every anchor: their output rows are bit-identical"""
    for k in keys:
        for a in c["anchors"]:
            n = min(R.GROUP, c["rows"] - a)
            assert torch.equal(bits(got[k][a:a + n]), bits(got[k][0:n])), f"{k}: rows {a}..{a + n - 1} differ from rows 0..{n - 1} on equal inputs"


def _reduce(slabs, nslabs, n):
    """the slab totals as the plan forms them: afr_op_reduce over nslabs slabs of n floats"""
    dst = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    sl = slabs.cuda()
    _lib.check(_lib.lib().afr_op_reduce(ptr(dst), ptr(sl), nslabs, n, n, 1.0, 0, stream()))
    torch.cuda.synchronize()
    return dst.cpu()


# row counts of the forward kernels (one wave per row, at most 8192 blocks of 4 waves = 32768 rows per trip):
#   1 x 3     =     3 rows: 3 / (8192*4) < 1 trip, ONE block with an idle wave
#   3 x 7     =    21 rows: not a multiple of 4 (the last block has 3 idle waves), r % tokens and r / tokens at work
#   5 x 24    =   120 rows: 30 blocks
#   8 x 4096  = 32768 rows: 32768 / (8192*4) = 1.00 -- exactly one trip, no wave prefetches a second row
#   9 x 4104  = 36936 rows: 36936 / (8192*4) = 1.13 -- the first 4168 waves make a second trip, the others find no next row
#   17 x 4104 = 69768 rows: 69768 / (8192*4) = 2.13 -- three trips for 4232 waves, two for the rest
def _fwd_params():
    out = []
    for B, t, d in R.fwd_cases():
        for is_bf16 in (False, True):
            out.append(pytest.param(B, t, d, is_bf16, id=f"{B}x{t}-d{d}-{'bf16' if is_bf16 else 'f32'}"))
    return out


@pytest.mark.parametrize("mode", ["pos", "add", "no_n"])
@pytest.mark.parametrize("B,tokens,d,is_bf16", _fwd_params())
def test_add_ln(B, tokens, d, is_bf16, mode):
    lib = _lib.lib()
    c = R.add_ln_case(B, tokens, d, mode, is_bf16)
    rows, T = c["rows"], tt(is_bf16)
    hin, pos, add = (None if c[k] is None else dev(c[k], torch.float32 if k != "add" else T) for k in ("hin", "pos", "add"))
    g, b = (None if c[k] is None else dev(c[k]) for k in ("g", "b"))

    def launch():
        o = Outs()
        ph = o.new("h", (rows, d), torch.float32, guard=d)
        pn = o.new("n", (rows, d), T, guard=d) if mode != "no_n" else C.c_void_p(0)
        _lib.check(lib.afr_op_pixel_add_ln(dt(is_bf16), ptr(hin), ph, ptr(pos), ptr(add), ptr(g), ptr(b), pn, rows, tokens, d, R.EPS, stream()))
        return o.finish()
    got = twice(launch)
    ref = R.add_ln_run(c, F64)
    want_h = ref["h"].float() if mode == "pos" else c["hin"] + c["add"]          # a copy, or ONE float32 addition: exact
    assert torch.equal(bits(got["h"]), bits(want_h))
    _locality(c, got, list(got))
    judge(f"add_ln/{mode} {rows}x{d}", got, ref, R.add_ln_bounds(c, ref), list(got))


@pytest.mark.parametrize("variant", ["mse", "bce-y-only", "mse-u-only"])
@pytest.mark.parametrize("B,tokens,d,is_bf16", _fwd_params())
def test_head(B, tokens, d, is_bf16, variant):
    lib = _lib.lib()
    loss = variant[:3]
    c = R.head_case(B, tokens, d, loss, is_bf16)
    rows = c["rows"]
    hin, add = dev(c["hin"]), dev(c["add"], tt(is_bf16))
    g, b, w, bo = (dev(c[k]) for k in ("g", "b", "w", "bo"))

    def launch():
        o = Outs()
        ph = o.new("h", (rows, d), torch.float32, guard=d)
        pu = o.new("u", (rows,), torch.float32, guard=64) if variant != "bce-y-only" else C.c_void_p(0)
        py = o.new("y", (rows,), torch.float32, guard=64) if variant != "mse-u-only" else C.c_void_p(0)
        _lib.check(lib.afr_op_pixel_head(dt(is_bf16), _lib.LOSS_KINDS[loss], ptr(hin), ph, ptr(add), ptr(g), ptr(b), ptr(w), ptr(bo), pu, py,
                                         rows, d, R.EPS, stream()))
        return o.finish()
    got = twice(launch)
    ref = R.head_run(c, F64)
    assert torch.equal(bits(got["h"]), bits(c["hin"] + c["add"]))              # ONE float32 addition: exact
    _locality(c, got, list(got))
    judge(f"head/{variant} {rows}x{d}", got, ref, R.head_bounds(c, ref), list(got))


@pytest.mark.parametrize("Cn", [2, 1])
@pytest.mark.parametrize("B,tokens,d,is_bf16", _fwd_params())
def test_attn(B, tokens, d, is_bf16, Cn):
    lib = _lib.lib()
    c = R.attn_case(B, tokens, d, Cn, is_bf16)
    rows, T = c["rows"], tt(is_bf16)
    q, kv = dev(c["q"], T), dev(c["kv"], T)

    def launch():
        o = Outs()
        po = o.new("o", (rows, d), T, guard=d)
        _lib.check(lib.afr_op_pixel_attn(dt(is_bf16), ptr(q), ptr(kv), po, rows, tokens, d, d // 64, Cn, stream()))
        return o.finish()
    got = twice(launch)
    ref = R.attn_run(c, F64)
    _locality(c, got, ["o"])
    judge(f"attn/C{Cn} {rows}x{d}", got, ref, R.attn_bounds(c, ref), ["o"])


# row counts of the head / LayerNorm backward (512 blocks of 16 waves = 8192 rows per trip, one partial slab per block):
#   1 x 3     =     3 rows: fewer than 16 -- one block, 13 idle waves
#   3 x 7     =    21 rows, 5 x 24 = 120 rows (8 slabs), 3 x 1000 = 3000 rows: 188 slabs, fewer than 512
#   2 x 4096  =  8192 rows:  8192 / (512*16) = 1.00 -- exactly one trip
#   3 x 4104  = 12312 rows: 12312 / (512*16) = 1.50 -- half the waves make a second trip
#   7 x 4104  = 28728 rows: 28728 / (512*16) = 3.51 -- four trips for half the waves, three for the rest
def _bwd_params():
    out = []
    for B, t, d in R.bwd_cases():
        for is_bf16 in (False, True):
            out.append(pytest.param(B, t, d, is_bf16, id=f"{B}x{t}-d{d}-{'bf16' if is_bf16 else 'f32'}"))
    return out


def _slab_checks(name, c, bounds, got, ref, K):
    """dh (and dhT) per element; the slab totals summed on the host in fp64 and through afr_op_reduce"""
    rows, d = c["rows"], c["d"]
    nblk = _lib.lib().afr_pixel_bwd_blocks(rows)
    assert nblk == R.bwd_blocks(rows)
    if "dhT" in got:
        assert torch.equal(bits(got["dhT"]), bits(got["dh"].bfloat16())), "dhT is not bf16(dh)"
    _locality(c, got, ["dh"])
    slabs = got["part"].reshape(nblk, K, d)
    host = dict(dh=got["dh"], part=slabs.double().sum(0))
    judge(name + " (slabs summed in fp64)", host, ref, bounds(c, ref, reduced=False), ["dh", "part"])
    devsum = dict(part=_reduce(got["part"], nblk, K * d).reshape(K, d))
    judge(name + " (afr_op_reduce)", devsum, ref, bounds(c, ref, reduced=True), ["part"])
    return slabs


@pytest.mark.parametrize("B,tokens,d,is_bf16", _bwd_params())
def test_head_bwd(B, tokens, d, is_bf16):
    lib = _lib.lib()
    c = R.head_bwd_case(B, tokens, d, is_bf16)
    rows = c["rows"]
    du, hf, g, b, w = (dev(c[k]) for k in ("du", "hf", "g", "b", "w"))
    nblk = R.bwd_blocks(rows)

    def launch():
        o = Outs()
        pdh = o.new("dh", (rows, d), torch.float32, guard=d)
        pT = o.new("dhT", (rows, d), torch.bfloat16, guard=d) if is_bf16 else C.c_void_p(0)
        pp = o.new("part", (nblk, 4, d), torch.float32, guard=4 * d)
        _lib.check(lib.afr_op_pixel_head_bwd(dt(is_bf16), ptr(du), ptr(hf), ptr(g), ptr(b), ptr(w), pdh, pT, pp, rows, d, R.EPS, stream()))
        return o.finish()
    got = twice(launch)
    ref = R.head_bwd_run(c, F64)
    slabs = _slab_checks(f"head_bwd {rows}x{d}", c, R.head_bwd_bounds, got, ref, 4)
    assert float(slabs[:, 3, 1:].abs().max()) == 0.0                             # only element 0 of the fourth row carries db_out


@pytest.mark.parametrize("B,tokens,d,is_bf16", _bwd_params())
def test_ln_bwd_in_place(B, tokens, d, is_bf16):
    lib = _lib.lib()
    c = R.ln_bwd_case(B, tokens, d, is_bf16)
    rows = c["rows"]
    dy, hin, g = dev(c["dy"], tt(is_bf16)), dev(c["hin"]), dev(c["g"])
    nblk = R.bwd_blocks(rows)

    def launch():
        o = Outs()
        pdh = o.new("dh", (rows, d), torch.float32, guard=d, init=c["dh"])              # in place on dh, as the plan runs it
        pT = o.new("dhT", (rows, d), torch.bfloat16, guard=d) if is_bf16 else C.c_void_p(0)
        pp = o.new("part", (nblk, 2, d), torch.float32, guard=2 * d)
        _lib.check(lib.afr_op_pixel_ln_bwd(dt(is_bf16), ptr(dy), ptr(hin), ptr(g), pdh, pT, pp, rows, d, R.EPS, stream()))
        return o.finish()
    got = twice(launch)
    ref = R.ln_bwd_run(c, F64)
    _slab_checks(f"ln_bwd {rows}x{d}", c, R.ln_bwd_bounds, got, ref, 2)


# attention backward: one block per (sample, chunk of 256 tokens), 16 waves walking the chunk's tokens 16 apart.
#   tokens 8: half the waves idle;  200: one chunk, 12.5 tokens per wave;  256: one full chunk;  264: a second chunk of 8 tokens;
#   520: three chunks, the last of 8 tokens (fewer than the block's 16 waves).  B = 1 and 3.
@pytest.mark.parametrize("is_bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,tokens,d,Cn", R.attn_bwd_cases())
def test_attn_bwd(B, tokens, d, Cn, is_bf16):
    lib = _lib.lib()
    c = R.attn_bwd_case(B, tokens, d, Cn, is_bf16)
    rows, T = c["rows"], tt(is_bf16)
    dO, q, kv = dev(c["dO"], T), dev(c["q"], T), dev(c["kv"], T)
    chunk = lib.afr_pixel_attn_chunk(tokens)
    assert chunk == R.attn_chunk(tokens)
    chunks = -(-tokens // chunk)

    def launch():
        o = Outs()
        pdq = o.new("dq", (rows, d), T, guard=d)
        pp = o.new("part", (chunks, B, 4 * d), torch.float32, guard=4 * d)
        _lib.check(lib.afr_op_pixel_attn_bwd(dt(is_bf16), ptr(dO), ptr(q), ptr(kv), pdq, pp, B, tokens, d, d // 64, Cn, stream()))
        return o.finish()
    got = twice(launch)
    ref = R.attn_bwd_run(c, F64)
    _locality(c, got, ["dq"])
    if Cn == 1:
        assert float(got["part"][:, :, 2 * d:].abs().max()) == 0.0 and float(got["dq"].float().abs().max()) == 0.0
    name = f"attn_bwd {B}x{tokens}x{d} C{Cn}"
    judge(name + " (slabs summed in fp64)", dict(dq=got["dq"], dkv=got["part"].double().sum(0)), ref, R.attn_bwd_bounds(c, ref, reduced=False), ["dq", "dkv"])
    judge(name + " (afr_op_reduce)", dict(dkv=_reduce(got["part"], chunks, B * 4 * d).reshape(B, 4 * d)), ref, R.attn_bwd_bounds(c, ref, reduced=True), ["dkv"])


@pytest.mark.parametrize("B,d,n_fonts", [(1, 64, 3), (13, 192, 3), (40, 512, 3), (7, 320, 0)])
def test_ctx_and_ctx_bwd(B, d, n_fonts):
    """the gather is a copy (bf16: one rounding) -- exact; the scatter-add sums repeated codes (code 65 in every third glyph) in glyph
    order and writes ZERO rows for codes and fonts nobody uses, whatever the buffer held"""
    lib = _lib.lib()
    I = R.ctx_inputs(B, d, n_fonts=n_fonts)
    Cn = 2 if n_fonts else 1
    emb, femb, x, font, dctx = (None if I[k] is None else dev(I[k]) for k in ("emb", "femb", "x", "font", "dctx"))
    want = R.ctx(I["emb"], I["femb"], I["x"], I["font"])
    for is_bf16 in (False, True):
        err = torch.zeros(1, dtype=torch.int32, device="cuda")

        def launch():
            o = Outs()
            pc = o.new("ctx", (B, Cn, d), tt(is_bf16), guard=d)
            _lib.check(lib.afr_op_pixel_ctx(dt(is_bf16), ptr(emb), ptr(femb), ptr(x), ptr(font), B, d, I["vocab"], n_fonts, pc, ptr(err), stream()))
            return o.finish()
        got = twice(launch)
        assert torch.equal(bits(got["ctx"]), bits(want.to(tt(is_bf16)))) and int(err.item()) == 0

    def launch_bwd():
        o = Outs()
        pe = o.new("demb", (I["vocab"], d), torch.float32, guard=d)
        pf = o.new("dfont", (n_fonts, d), torch.float32, guard=d) if n_fonts else C.c_void_p(0)
        _lib.check(lib.afr_op_pixel_ctx_bwd(ptr(dctx), ptr(x), ptr(font), B, d, I["vocab"], n_fonts, pe, pf, stream()))
        return o.finish()
    got = twice(launch_bwd)
    ref = R.ctx_bwd(I["dctx"].double(), I["x"], I["font"], I["vocab"], n_fonts)
    bnd = R.bound_ctx_bwd(I["dctx"].double(), I["x"], I["font"], I["vocab"], n_fonts)
    keys = ["demb"] + (["dfont"] if n_fonts else [])
    judge(f"ctx_bwd {B}x{d}", got, dict(demb=ref[0], dfont=ref[1]), dict(demb=bnd[0], dfont=bnd[1]), keys)
    used = set(I["x"].tolist())
    for v in range(I["vocab"]):
        if v not in used:
            assert float(got["demb"][v].abs().max()) == 0.0, v
    assert float(got["demb"][65].abs().max()) > 0.0
    if n_fonts:
        assert float(got["dfont"][n_fonts - 1].abs().max()) == 0.0
