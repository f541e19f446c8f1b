"""Yardstick of the per-tensor statistics (include/afr.h afr_tensor_stat): the fp64 restatement, the error bound of the two float32
sums derived from the documented summation order, and a float32 replay of that order in numpy.  Nothing here knows the kernels."""
import numpy as np

EPS32 = 2.0 ** -24            # unit roundoff of float32
FLT_MAX = float(np.finfo(np.float32).max)
FIELDS = ("sumsq", "sum", "min", "max", "n_nan", "n_inf", "n_zero", "numel")


def classify(x):
    """(finite, nan, inf, zero) masks of a float32 array, by bit pattern: exponent field all ones is an infinity (mantissa 0) or a
    NaN; no bit below the sign is a zero.  A denormal is finite and non-zero whatever the arithmetic would make of it."""
    mag = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    return mag < 0x7F800000, mag > 0x7F800000, mag == 0x7F800000, mag == 0


def difference(a, minus):
    """x = a - minus in float32 (inf - inf is a NaN), the values the difference mode describes."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(a, dtype=np.float32) - np.asarray(minus, dtype=np.float32)).astype(np.float32)


def stats64(x):
    """The record of one tensor: the sums in fp64 over the finite elements; min / max the float32 values themselves (+inf / -inf
    when there is no finite element); the counts."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    fin, nan, inf, zero = classify(x)
    f = x[fin].astype(np.float64)
    return {"sumsq": float((f * f).sum()), "sum": float(f.sum()),
            "min": np.float32(x[fin].min()) if f.size else np.float32(np.inf), "max": np.float32(x[fin].max()) if f.size else np.float32(-np.inf),
            "n_nan": int(nan.sum()), "n_inf": int(inf.sum()), "n_zero": int(zero.sum()), "numel": int(x.size),
            "abs_sum": float(np.abs(f).sum())}


def chunks_of(numel, chunk):
    return max(1, -(-int(numel) // int(chunk)))


def chain_depth(numel, chunk):
    """D: the longest chain of float32 roundings between one term and the result, from the documented order.  A chunk of `chunk`
    elements is summed by 256 lanes; a lane keeps one accumulator per position in a group of 4 elements and takes the groups lane,
    lane + 256, ...: at most ceil(groups in the chunk / 256) terms per accumulator (the fused multiply-add of the squares rounds
    once per term), one more for a tail element behind the last whole group; (a0 + a1) + (a2 + a3): 2; the wave butterfly: 6; the
    four waves (w0 + w1) + (w2 + w3): 2; the finish: ceil(chunks / 64) partials per lane and 6 butterfly steps."""
    numel, chunk = int(numel), int(chunk)
    groups = min(numel // 4, chunk // 4)
    return -(-groups // 256) + (1 if numel % 4 else 0) + 2 + 6 + 2 + -(-chunks_of(numel, chunk) // 64) + 6


def bounds(x, chunk):
    """(bound of sum, bound of sumsq) against fp64 for one tensor's values: |err| <= (D + 1) 2^-24 sum |term|.  The squares add what
    the format itself loses below its normal range: a term x^2 under 2^-126 is rounded with an absolute error of up to 2^-150
    instead of a relative one (the sum of x is not affected: an addition whose result is subnormal is exact)."""
    r = stats64(x)
    d = chain_depth(r["numel"], chunk)
    return (d + 1) * EPS32 * r["abs_sum"], (d + 1) * EPS32 * r["sumsq"] + r["numel"] * 2.0 ** -150


def sumsq_overflows(x, chunk):
    """True when the float32 sum of squares must be +inf: one square alone, or the fp64 sum less its bound, lies beyond FLT_MAX."""
    r = stats64(x)
    return r["sumsq"] - bounds(x, chunk)[1] > FLT_MAX


# ------------------------------------------------------------------------------------------- float32 replay of the order
def _fma32(x, q):
    """fl32(x * x + q) for float32 arrays: the product is exact in float64, so only the final rounding differs from a true fused
    multiply-add, and only by a second rounding at 2^-53."""
    return (x.astype(np.float64) * x.astype(np.float64) + q.astype(np.float64)).astype(np.float32)


def _butterfly(v):
    """v [waves, 64] float32 -> lane 0 of every wave after the steps 32, 16, 8, 4, 2, 1 of v += v[lane ^ step]."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, lane ^ o]).astype(np.float32)
    return v[:, 0]


def _chunk32(groups, tail):
    """One chunk: groups float32 [m, 4] (m <= chunk / 4 whole groups, finite values or 0), tail <= 3 values of the tensor's last chunk
    (else empty).  Returns (sumsq, sum) float32."""
    m = len(groups)
    trips = max(1, -(-m // 256))
    g = np.zeros((trips * 256, 4), dtype=np.float32)
    g[:m] = groups
    g = g.reshape(trips, 256, 4)
    q, s = np.zeros((256, 4), dtype=np.float32), np.zeros((256, 4), dtype=np.float32)
    for t in range(trips):
        q, s = _fma32(g[t], q), (s + g[t]).astype(np.float32)
    for l, x in enumerate(tail):
        xv = np.float32(x)
        q[l, 0], s[l, 0] = _fma32(np.array([xv]), q[l, :1])[0], np.float32(s[l, 0] + xv)
    out = []
    for a in (q, s):
        lane = ((a[:, 0] + a[:, 1]).astype(np.float32) + (a[:, 2] + a[:, 3]).astype(np.float32)).astype(np.float32)
        w = _butterfly(lane.reshape(4, 64))
        out.append(np.float32(np.float32(w[0] + w[1]) + np.float32(w[2] + w[3])))
    return out


def replay32(x, chunk):
    """(sumsq, sum) of one tensor in float32, in the documented order (chunks, lanes, groups, pairing, butterfly, waves, finish)."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    x = np.where(classify(x)[0], x, np.float32(0)).astype(np.float32)
    n, n4 = x.size, x.size // 4
    nc = chunks_of(n, chunk)
    part = np.zeros((2, -(-nc // 64) * 64), dtype=np.float32)
    with np.errstate(over="ignore"):
        for c in range(nc):
            g0, g1 = c * (chunk // 4), min(n4, (c + 1) * (chunk // 4))
            groups = x[4 * g0:4 * max(g0, g1)].reshape(-1, 4)
            part[0, c], part[1, c] = _chunk32(groups, x[4 * n4:] if c == nc - 1 else x[:0])
        res = []
        for p in part:
            lanes = np.zeros(64, dtype=np.float32)
            for r in p.reshape(-1, 64):                      # lane l: chunks l, l + 64, ... in ascending order
                lanes = (lanes + r).astype(np.float32)
            res.append(_butterfly(lanes.reshape(1, 64))[0])
    return np.float32(res[0]), np.float32(res[1])


# ------------------------------------------------------------------------------------------- decoding and comparing records
def decode(raw):
    """raw: int32 [n, 8] as the library writes it -> dict of field -> array (float32 / uint32)."""
    raw = np.ascontiguousarray(raw, dtype=np.int32).reshape(-1, 8)
    f, u = raw.view(np.float32), raw.view(np.uint32)
    out = {k: f[:, i] for i, k in enumerate(FIELDS[:4])}
    out.update({k: u[:, 4 + i] for i, k in enumerate(FIELDS[4:])})
    return out


def check_record(got, x, chunk, what=""):
    """One tensor: got = dict field -> scalar, x = the float32 values it describes.  The exact fields exactly, the sums within the
    bound (a sum of squares beyond FLT_MAX must be +inf).  Returns the worst fraction of the bound the two sums used."""
    want = stats64(x)
    for k in ("n_nan", "n_inf", "n_zero", "numel"):
        assert int(got[k]) == want[k], (what, k, int(got[k]), want[k])
    for k in ("min", "max"):
        assert np.float32(got[k]) == want[k], (what, k, float(got[k]), float(want[k]))
    bs, bq = bounds(x, chunk)
    es = abs(float(got["sum"]) - want["sum"])
    assert es <= bs, (what, "sum", float(got["sum"]), want["sum"], es, bs)
    worst = es / bs if bs > 0 else 0.0
    if sumsq_overflows(x, chunk):
        assert np.isposinf(got["sumsq"]), (what, "sumsq beyond FLT_MAX", float(got["sumsq"]))
    else:
        eq = abs(float(got["sumsq"]) - want["sumsq"])
        assert eq <= bq, (what, "sumsq", float(got["sumsq"]), want["sumsq"], eq, bq)
        worst = max(worst, eq / bq if bq > 0 else 0.0)
    return worst
