"""The fp8 building blocks' reference, from the format definition only (numpy, fp64; no torch cast, no GPU): the 256 values of OCP
e4m3fn, the cast the header promises for afr_op_f32_to_fp8, the product afr_op_gemm_fp8 computes read through its leading dimensions,
its bounds, and a restatement of the product with ONE planted fault at a time (fault_model) that tests/test_fp8_ref_cpu.py puts in the
kernel's place to show that the case table of tests/test_gpu_fp8_ops.py sees each of them.

BOUNDS (the project's own for this kernel; none taken from what the kernel returns): an f32 output 5e-5 of the largest |reference|
(tests/test_gpu_fp8.py::test_fp8_gemm_vs_fp64: the products of two e4m3 numbers are exact in f32, the 128-deep scaled MFMA sums them
with somewhat less than an f32 fma chain's accuracy); a bf16 output one bf16 ulp, 2^-8 |reference| per element, on top; integer-valued
operands whose partial sums stay below 2^11: 0."""
import numpy as np

NAN_BYTE = 0x7F
MAX_FINITE = 448.0
BM, BN, BK = 256, 128, 128             # the kernel's tile and K-tile: what the block- and tile-shaped faults are cut along
F32_REL = 5e-5
BF16_ULP = 2.0 ** -8

FAULTS = ("lda_is_k", "ldb_is_k", "ragged_last_ktile_dropped", "even_last_ktile_dropped", "a_halves_swapped", "block_rows_shifted",
          "bias_before_scale", "relu_before_bias", "bf16_truncated")


def decode_table():
    """float64[256]: the value of every e4m3fn byte -- sign, 4 exponent bits (bias 7), 3 mantissa bits; exponent 0: m 2^-9; 0x7F and
    0xFF: NaN; no infinities (exponent 15 with m < 7 is finite: the largest is 1.75 2^8 = 448)"""
    t = np.empty(256, dtype=np.float64)
    for b in range(256):
        e, m = (b >> 3) & 15, b & 7
        if e == 15 and m == 7:
            v = float("nan")
        elif e == 0:
            v = m * 2.0 ** -9
        else:
            v = (1.0 + m / 8.0) * 2.0 ** (e - 7)
        t[b] = -v if b & 0x80 else v
    return t


TABLE = decode_table()
MAGNITUDES = TABLE[:NAN_BYTE]          # codes 0x00 .. 0x7E: the finite magnitudes, ascending; the code of a magnitude is its index


def scaled(x, scale, mode="div"):
    """the float32 value the cast rounds: x / scale ("div", the contract of include/afr.h) or x * (1 / scale) ("recip", the rule the
    contract excludes: test_fp8_ref_cpu.py counts where the two part), either computed in float32 as a kernel does"""
    x, s = np.asarray(x, dtype=np.float32), np.float32(scale)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return x / s if mode == "div" else x * (np.float32(1.0) / s)


def encode(x, scale=1.0, mode="div"):
    """uint8 e4m3fn bytes of scaled(x, scale, mode): round to nearest, ties to the even code, by search in the table of finite values;
    beyond +-448 (the infinities included) the largest finite value of that sign; NaN -> 0x7F"""
    y = scaled(x, scale, mode).astype(np.float64)
    nan = np.isnan(y)
    a = np.minimum(np.abs(np.where(nan, 0.0, y)), MAX_FINITE)
    hi = np.clip(np.searchsorted(MAGNITUDES, a, side="left"), 1, NAN_BYTE - 1)          # MAGNITUDES[hi - 1] <= a <= MAGNITUDES[hi]
    lo = hi - 1
    dl, dh = a - MAGNITUDES[lo], MAGNITUDES[hi] - a
    code = np.where(dl < dh, lo, np.where(dh < dl, hi, np.where(lo % 2 == 0, lo, hi)))
    code = np.where(a == 0.0, 0, code)
    out = (code | np.where(np.signbit(y), 0x80, 0)).astype(np.uint8)
    return np.where(nan, np.uint8(NAN_BYTE), out)


def _rows(buf, ld, rows, K):
    """[rows][K] bytes of a flat operand read through its leading dimension: k >= K and rows behind the last are never touched"""
    flat = np.asarray(buf, dtype=np.uint8).reshape(-1)
    return flat[np.arange(rows, dtype=np.int64)[:, None] * ld + np.arange(K, dtype=np.int64)[None, :]]


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


def gemm_ref(A8, B8, lda, ldb, M, N, K, scale_ab=1.0, bias=None, relu=False):
    """-> (float64 [M][N]: scale_ab sum_k A[m lda + k] B[n ldb + k] (+ bias[n]) (relu), with scale_ab the float32 the entry receives;
    int64 [M][N]: the bare sum, where every operand value read is an integer, else None)"""
    a, b = TABLE[_rows(A8, lda, M, K)], TABLE[_rows(B8, ldb, N, K)]
    acc = a @ b.T
    c = acc * float(np.float32(scale_ab))
    if bias is not None:
        c = c + np.asarray(bias, dtype=np.float64)[None, :N]
    if relu:
        c = np.maximum(c, 0.0)
    whole = bool(np.all(a == np.rint(a)) and np.all(b == np.rint(b)))
    return c, (np.rint(a).astype(np.int64) @ np.rint(b).astype(np.int64).T if whole else None)


def f32_bound(ref):
    """the f32 output's bound: one number for the launch"""
    return F32_REL * float(np.max(np.abs(ref)))


def bf16_bound(ref, scale_ref=None):
    """the bf16 output's bound per element: the f32 bound (of scale_ref, default ref) and one bf16 ulp of the element"""
    return f32_bound(ref if scale_ref is None else scale_ref) + BF16_ULP * np.abs(ref)


def bf16_bits(c32, truncate=False):
    """uint16 bfloat16 bits of a float32 array: round to nearest even (or the upper half as it is)"""
    u = np.ascontiguousarray(c32, dtype=np.float32).view(np.uint32)
    if not truncate:
        u = u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))
    return (u >> np.uint32(16)).astype(np.uint16)


def fault_model(A8, B8, lda, ldb, M, N, K, scale_ab, bias=None, relu=False, out_bf16=False, fault=None):
    """The product restated in numpy with the float32 steps of the kernel's epilogue (scale the sum, add the bias, ReLU, round the
    output), and ONE planted fault (FAULTS; None: none).  -> float32 [M][N], or uint16 bfloat16 bits with out_bf16.  For the CPU test
    of the case table only: never compared with the GPU."""
    assert fault is None or fault in FAULTS, fault
    if fault == "lda_is_k":
        lda = K
    if fault == "ldb_is_k":
        ldb = K
    a, b = TABLE[_rows(A8, lda, M, K)], TABLE[_rows(B8, ldb, N, K)]
    nt = -(-K // BK)
    if (fault == "ragged_last_ktile_dropped" and K % BK) or (fault == "even_last_ktile_dropped" and nt % 2 == 0):
        a, b = a[:, :(nt - 1) * BK], b[:, :(nt - 1) * BK]
    if fault == "a_halves_swapped":                          # A's k ^ 16 meets B's k; what lies beyond K is the zero the staging gives
        K32 = -(-K // 32) * 32
        a = np.pad(a, ((0, 0), (0, K32 - K)))[:, np.arange(K32) ^ 16]
        b = np.pad(b, ((0, 0), (0, K32 - K)))
    acc = a @ b.T
    if fault == "block_rows_shifted":                        # block (0, 0) computes its rows from the other 128-row half of its A tile
        rows = np.pad(a, ((0, max(0, BM - M)), (0, 0)))[(np.arange(BM) + 128) % BM]
        acc[:min(M, BM), :min(N, BN)] = (rows @ b[:min(N, BN)].T)[:min(M, BM)]
    s = np.float32(scale_ab)
    bia = None if bias is None else np.asarray(bias, dtype=np.float32)[None, :N]
    with np.errstate(invalid="ignore", over="ignore"):
        if fault == "bias_before_scale" and bia is not None:
            c = _f32(_f32(acc) + bia) * s
        else:
            c = _f32(acc * float(s))
            if fault == "relu_before_bias" and relu:
                c = np.where(c > 0, c, np.float32(0.0))
            if bia is not None:
                c = c + bia
        if relu and fault != "relu_before_bias":
            c = np.where(c > 0, c, np.float32(0.0))
    c = c.astype(np.float32)
    return bf16_bits(c, truncate=fault == "bf16_truncated") if out_bf16 else c
