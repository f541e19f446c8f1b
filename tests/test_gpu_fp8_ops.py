"""GPU: the two fp8 building blocks one launch at a time -- afr_op_gemm_fp8 (fp8k::gemm_fp8, csrc/gemm.hip) and afr_op_f32_to_fp8
(f32_to_fp8_kernel, csrc/elementwise.hip) -- against tests/fp8_ref.py, by the method of tests/op_harness.py: every output between two
guard bands, every launch repeated bit for bit.

GEMM.  The case table holds the smallest shapes at which each branch of the kernel exists (tile 256 x 128, K-tile 128, three ring
stages): one interior block with nt = ceil(K / 128) = 1, 2, 3, 4, 5, 7 K-tiles (the prologue's three waits, no refill / first refill,
odd and even ends of the loop unrolled by two, the slot's wrap), each dense and with lda = K + 16, ldb = K + 48, ldc = N + 8; edge
blocks (the per-piece addressing) down to 8 x 8 x 16, with a K tail of 16, with four and nine blocks; and one launch with an interior
and three edge blocks.  Operands are e4m3 bytes made on the CPU (fp8_ref.encode); the padding columns [K, ld) and three rows behind the
last hold the NaN byte, the bias has NaN behind it: whatever is read there and used turns the output NaN.  C has ldc - N columns and
three rows that must keep their fill, and guard bands around all of it.  Data kinds: `position` (one operand one-hot per row at
k = (5 row + 3) mod K with value 1 or -2, the other ((7 row + 3 k) mod 31) - 15: C[m][n] names the k that met the one-hot k; both ways
round; bit for bit), `integer` (hashed {-2 .. 2}, K <= 512, every partial sum below 2^11: bit for bit), `random` (hashed operands with
per-tensor scales 0.011 and 0.0042; flags 0, BIAS, BIAS | RELU, each also with OUT_BF16; f32 results against fp64 within 5e-5 of the
largest |product|, the ReLU launch = max(own BIAS launch, +0) and every bf16 launch = its own f32 launch rounded to nearest even, bit
for bit).  The checks take the product as a function: tests/test_fp8_ref_cpu.py hands them fp8_ref.fault_model on the CPU.

CAST.  Byte-equal to fp8_ref.encode (x / scale in float32, round to nearest even, saturating, NaN stays NaN) on every finite code
point, every midpoint of adjacent code points with three float32 neighbours on either side, the subnormal boundary, the saturation
edge, infinities and NaNs, at five scales and at sizes that are tail only, one quad, quad + tail and several blocks of quads.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from ai_font_renderer_amd import synth
from . import fp8_ref as R
from .op_harness import Outs, bits, judge, twice
from .util import ratio

EXTRA = 3                                                    # rows behind the last row of A, B and C
FLAG_BIAS, FLAG_RELU, FLAG_BF16 = 1, 2, 8                    # AFR_GEMM_BIAS, AFR_GEMM_RELU, AFR_GEMM_OUT_BF16 (include/afr.h)
SA, SB = 0.011, 0.0042                                       # the random kind's per-tensor scales (those of tests/test_gpu_fp8.py)

# (M, N, K, dense)
GEMM_CASES = ([(256, 128, K, dense) for K in (128, 256, 384, 512, 640, 896) for dense in (True, False)] +
              [(8, 8, 16, False), (200, 72, 400, False), (264, 136, 144, False), (520, 264, 1040, False), (264, 136, 384, False)])
KINDS = ("position", "integer", "random")


def case_id(case):
    M, N, K, dense = case
    return "%dx%dx%d-%s" % (M, N, K, "dense" if dense else "padded")


def leading(case):
    M, N, K, dense = case
    return (K, K, N) if dense else (K + 16, K + 48, N + 8)


def applies(kind, case):
    """the integer kind is defined for K <= 512: beyond, 4 K could pass the 2^11 its exactness is argued from"""
    return kind != "integer" or case[2] <= 512


def padded_bytes(values, scale, rows, K, ld):
    """flat uint8 [(rows + EXTRA) ld]: the e4m3 bytes of values / scale in the [rows][K] corner, the NaN byte everywhere else"""
    buf = np.full((rows + EXTRA, ld), R.NAN_BYTE, dtype=np.uint8)
    buf[:rows, :K] = R.encode(values, scale)
    return buf.reshape(-1)


def one_hot(rows, K, value):
    v = np.zeros((rows, K), dtype=np.float32)
    v[np.arange(rows), (5 * np.arange(rows) + 3) % K] = value
    return v


def coded(rows, K):
    """((7 row + 3 k) mod 31) - 15: integers of [-15, 15], every one an e4m3 value"""
    return (((7 * np.arange(rows)[:, None] + 3 * np.arange(K)[None, :]) % 31) - 15).astype(np.float32)


@functools.lru_cache(maxsize=None)
def operands(kind, case):
    """-> dict(A8, B8: flat padded bytes; scale: scale_ab; bias: float32 [N] or None) of one data kind on one case"""
    M, N, K, _ = case
    lda, ldb, _ = leading(case)
    sa = sb = 1.0
    bias = None
    if kind in ("position +1", "position -2"):
        a, b = one_hot(M, K, 1.0 if kind == "position +1" else -2.0), coded(N, K)
    elif kind == "position mirror":
        a, b = coded(M, K), one_hot(N, K, 1.0)
    elif kind == "integer":
        a = synth.hash_u8(341, (M, K)).astype(np.float32) % 5 - 2
        b = synth.hash_u8(342, (N, K)).astype(np.float32) % 5 - 2
        assert float((np.abs(a) @ np.abs(b).T).max()) < 2.0 ** 11
    else:
        assert kind == "random"
        sa, sb = SA, SB
        a, b = synth.hash_uniform(343, (M, K), 3.0), synth.hash_uniform(344, (N, K), 1.5)
        bias = synth.hash_uniform(345, (N,), 1.5 * K ** 0.5)               # the standard deviation of a product element
    return dict(A8=padded_bytes(a, sa, M, K, lda), B8=padded_bytes(b, sb, N, K, ldb), scale=float(np.float32(sa) * np.float32(sb)), bias=bias)


def reference(ops, case, flags=0):
    M, N, K, _ = case
    lda, ldb, _ = leading(case)
    return R.gemm_ref(ops["A8"], ops["B8"], lda, ldb, M, N, K, ops["scale"], ops["bias"] if flags & FLAG_BIAS else None, bool(flags & FLAG_RELU))


def gpu_product(flags, A8, B8, cview, bias, M, N, K, lda, ldb, ldc, scale):
    """the launch under test: afr_op_gemm_fp8 into cview, a [M + EXTRA][ldc] view of a guarded device buffer"""
    from ai_font_renderer_amd import _lib
    from .gpu_util import dev, ptr, stream
    a, b = dev(A8), dev(B8)
    bd = None
    if bias is not None:
        bd = torch.full((bias.size + 8,), float("nan"), dtype=torch.float32, device="cuda")
        bd[:bias.size] = torch.from_numpy(bias)
    _lib.check(_lib.lib().afr_op_gemm_fp8(flags, ptr(a), ptr(b), C.c_void_p(cview.data_ptr()), ptr(bd), M, N, K, lda, ldb, ldc, scale, stream()))
    torch.cuda.synchronize()


def launch(product, device, ops, case, flags):
    """One launch, twice: -> the [M][N] corner of C on the CPU (float32 or bfloat16), after checking that the guard bands, the columns
    [N, ldc) and the rows behind M kept their fill and that no NaN came out."""
    M, N, K, _ = case
    lda, ldb, ldc = leading(case)
    dtype = torch.bfloat16 if flags & FLAG_BF16 else torch.float32
    what = "%s flags %d" % (case_id(case), flags)

    def once():
        o = Outs(device)
        o.new("C", (M + EXTRA, ldc), dtype, guard=ldc)
        t, band, n, shape = o.bufs["C"]
        product(flags, ops["A8"], ops["B8"], t[band:band + n].view(shape), ops["bias"] if flags & FLAG_BIAS else None, M, N, K, lda, ldb, ldc,
                ops["scale"])
        full = o.finish(may_keep_fill=("C",))["C"]
        corner = full[:M, :N].clone()
        full[:M, :N] = float("nan")
        fill = bits(torch.full((1,), float("nan"), dtype=dtype))
        assert bool((bits(full) == fill).all()), what + ": written outside [M][N]: columns [N, ldc) or rows behind M"
        bad = torch.isnan(corner.float())
        assert not bool(bad.any()), what + ": %d NaN outputs, the first at (m, n) = %s: an element not written, or padding read and used" % (
            int(bad.sum()), tuple(bad.nonzero()[0].tolist()))
        return corner
    return twice(once)


def check_position(case, product, device="cuda"):
    """scale_ab = 1, no flags: C[m][n] is the coded operand's entry at the one-hot operand's k, times the one-hot value; exact"""
    M, N, K, _ = case
    for kind in ("position +1", "position -2", "position mirror"):
        ops = operands(kind, case)
        want = torch.from_numpy(reference(ops, case)[1])
        got = launch(product, device, ops, case, 0)
        wrong = (got.double() != want.double()).nonzero()
        if len(wrong):
            m, n = wrong[0].tolist()
            row, other = (n, m) if kind == "position mirror" else (m, n)             # row: of the one-hot operand; other: of the coded one
            value = -2.0 if kind == "position -2" else 1.0
            met = [k for k in range(K) if value * ((7 * other + 3 * k) % 31 - 15) == float(got[m, n])]
            raise AssertionError("%s %s: %d elements differ; C[%d][%d] = %g, not %g: the one-hot k = %d met k in %s" % (
                case_id(case), kind, len(wrong), m, n, float(got[m, n]), float(want[m, n]), (5 * row + 3) % K, met[:8]))
        assert torch.equal(bits(got), bits(want.float())), "%s %s: the sign of a zero" % (case_id(case), kind)


def check_integer(case, product, device="cuda"):
    """hashed {-2 .. 2}: every product and partial sum is an integer below 2^11, exact in any order of summation; bound 0"""
    ops = operands("integer", case)
    want = torch.from_numpy(reference(ops, case)[1]).double()
    got = launch(product, device, ops, case, 0)
    judge("fp8 gemm %s integer" % case_id(case), dict(C=got), dict(C=want), dict(C=0.0), ["C"])


def check_random(case, product, device="cuda"):
    ops = operands("random", case)
    top = torch.from_numpy(reference(ops, case)[0]).abs().max()                      # the largest |product|, as test_fp8_gemm_vs_fp64 takes it
    f32 = {}
    ratios = {}
    for flags, name in ((0, "plain"), (FLAG_BIAS, "bias"), (FLAG_BIAS | FLAG_RELU, "bias+relu")):
        ref = torch.from_numpy(reference(ops, case, flags)[0])
        f32[flags] = got = launch(product, device, ops, case, flags)
        b16 = launch(product, device, ops, case, flags | FLAG_BF16)
        assert torch.equal(bits(b16), bits(got.to(torch.bfloat16))), "%s %s: the bf16 launch is not the f32 launch rounded to nearest even" % (
            case_id(case), name)
        ratios[name] = ratio(got, ref, R.F32_REL * top)
        ratios[name + " bf16"] = ratio(b16.float(), ref, R.F32_REL * top + R.BF16_ULP * ref.abs())
    judge("fp8 gemm %s random" % case_id(case), ratios)
    fb = f32[FLAG_BIAS]
    assert bool((fb < 0).any()) and bool((fb > 0).any())                              # the ReLU has something to clip and something to keep
    assert torch.equal(bits(f32[FLAG_BIAS | FLAG_RELU]), bits(torch.where(fb > 0, fb, torch.zeros_like(fb)))), \
        "%s: the bias + ReLU launch is not max(own bias launch, +0)" % case_id(case)


CHECKS = {"position": check_position, "integer": check_integer, "random": check_random}


@pytest.mark.gpu
@pytest.mark.parametrize("case,kind", [(c, k) for c in GEMM_CASES for k in KINDS if applies(k, c)], ids=lambda v: v if isinstance(v, str) else case_id(v))
def test_gemm_fp8(case, kind):
    CHECKS[kind](case, gpu_product)


# ================================================================================================================== the cast
SCALES = (1.0, 0.25, 0.37, 0.011, 3.0)
SIZES = (1, 2, 3, 4, 5, 1027, 4 * 256 * 3 + 3)
FLT_MAX = float(np.finfo(np.float32).max)
NANS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFABCDEF], dtype=np.uint32).view(np.float32)     # both signs, two payloads each
BEYOND = np.array([464.0, -464.0, 1e6, -1e6, FLT_MAX, -FLT_MAX, np.inf, -np.inf], dtype=np.float32)      # times any scale: beyond +-448


def neighbours(x, n=3):
    """x (float32) with its n float32 neighbours on either side"""
    out, lo, hi = [x], x, x
    for _ in range(n):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return np.stack(out, axis=-1).reshape(-1)


@functools.lru_cache(maxsize=None)
def cast_pool(scale):
    """-> (float32 inputs at this scale, the directed ones in front; how many of them are code points times the scale)"""
    s = np.float32(scale)
    finite = np.array([b for b in range(256) if b & 0x7F != R.NAN_BYTE], dtype=np.uint8)
    codes = R.TABLE[finite].astype(np.float32) * s
    mags = R.MAGNITUDES[1:]                                                          # midpoints of adjacent pairs: 126 per sign (0 | 2^-9 included)
    mid = (0.5 * (R.MAGNITUDES[:-1] + mags)).astype(np.float32)                      # (4 significant bits: exact in float32)
    with np.errstate(over="ignore"):
        mids = neighbours(np.concatenate([mid, -mid]) * s)
        edge = np.array([2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -10, 448.0, -448.0, np.nextafter(np.float32(448.0), np.float32(np.inf))], dtype=np.float32)
        head = np.concatenate([NANS[:2], BEYOND[6:], edge, edge * s, BEYOND, BEYOND * s, NANS[2:]])
    fill = synth.hash_uniform(351, (SIZES[-1],), 600.0) * s
    return np.concatenate([head, codes, mids, fill]).astype(np.float32), len(head), finite


def cast_input(n, scale):
    """n inputs: the pool's first n - 3 and a tail of a NaN, an infinity and the saturation tie, so that non-finite values sit in quads
    (the pool's head) and in the scalar tail; n <= 5: NaN, -inf, the tie, +inf, NaN -- tail only up to 3, then a quad, then quad + tail"""
    pool, _, _ = cast_pool(scale)
    tie = np.float32(464.0) * np.float32(scale)
    if n <= 5:
        return np.array([NANS[3], -np.inf, tie, np.inf, NANS[0]], dtype=np.float32)[:n]
    return np.concatenate([pool[:n - 3], np.array([NANS[1], -np.inf, -tie], dtype=np.float32)])


def same_bytes(got, want):
    """byte-equal; a NaN byte of either sign where a NaN is due; +0 and -0 both taken where a zero is due (as tests/test_gpu_fp8.py does)"""
    nan = (want & 0x7F) == R.NAN_BYTE
    zero = (want & 0x7F) == 0
    return np.where(nan, (got & 0x7F) == R.NAN_BYTE, np.where(zero, (got & 0x7F) == 0, got == want))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("scale", SCALES)
def test_f32_to_fp8_is_fp8_ref_encode(scale, n):
    from ai_font_renderer_amd import _lib
    from .gpu_util import dev, stream
    lib = _lib.lib()
    pool, n_head, finite = cast_pool(scale)
    assert len(pool) >= SIZES[-1] - 3
    x = cast_input(n, scale)
    src = dev(x)

    def once():
        o = Outs("cuda")
        p = o.new("dst", n, torch.uint8)
        _lib.check(lib.afr_op_f32_to_fp8(C.c_void_p(src.data_ptr()), p, n, float(scale), stream()))
        return o.finish()["dst"]
    got = twice(once).numpy()
    want = R.encode(x, scale)
    ok = same_bytes(got, want)
    nan = np.isnan(x)
    show = lambda idx: [(float(x[i]), float(R.scaled(x[i], scale)), hex(got[i]), hex(want[i])) for i in idx[:4]]
    assert bool(ok.all()), "n %d scale %g (x, x / scale, got, want): %d NaN inputs left as another byte %s; %d other inputs rounded to another byte %s" % (
        n, scale, int((~ok & nan).sum()), show(np.flatnonzero(~ok & nan)), int((~ok & ~nan).sum()), show(np.flatnonzero(~ok & ~nan)))
    # what the reference itself says about the directed inputs, so that the comparison above means what it claims
    assert bool(((want & 0x7F) == R.NAN_BYTE)[nan].all()) and not bool(((want & 0x7F) == R.NAN_BYTE)[~nan].any())
    with np.errstate(invalid="ignore"):
        far = np.abs(R.scaled(x, scale).astype(np.float64)) > R.MAX_FINITE
    assert bool((want[far] == np.where(np.signbit(x[far]), 0xFE, 0x7E)).all())
    if n == SIZES[-1]:
        assert int(nan.sum()) == 5 and int(np.isinf(x).sum()) >= 5
        if scale in (1.0, 0.25):                                                      # a power of two: every code point comes back as itself
            assert bool(same_bytes(got[n_head:n_head + len(finite)], finite).all())
