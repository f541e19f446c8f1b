"""CPU: the yardstick of the per-tensor statistics (tests/tstats_ref.py) against numpy / torch on planted data, its bound against a
float32 replay of the documented summation order, TensorStats decoding, the AFR_TENSOR_REPORT setting and the report's lines."""
import types

import numpy as np
import pytest
import torch

from . import tstats_ref as R
from .util import ROOT  # noqa: F401  (puts the repository on sys.path)

CHUNK = 32768          # include/afr.h: the library's compile-time chunk (the GPU tests read it from afr_tensor_stats_chunk())


def _bits(*words):
    return np.array(words, dtype=np.uint32).view(np.float32)


def test_reference_classifies_by_bit_pattern_and_sums_the_finite_elements():
    x = np.concatenate([_bits(0x00000000, 0x80000000, 0x00000001, 0x80011171, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC01234, 0x7F800001),
                        np.array([1.5, -2.25, 1e18, -1e18, 3.0], dtype=np.float32)])
    fin, nan, inf, zero = R.classify(x)
    assert fin.tolist() == [True] * 4 + [False] * 5 + [True] * 5
    assert nan.tolist() == [False] * 6 + [True] * 3 + [False] * 5
    assert inf.tolist() == [False] * 4 + [True] * 2 + [False] * 8
    assert zero.tolist() == [True, True] + [False] * 12
    r = R.stats64(x)
    t = torch.from_numpy(x)
    assert (r["n_nan"], r["n_inf"], r["n_zero"], r["numel"]) == (int(torch.isnan(t).sum()), int(torch.isinf(t).sum()), int((t == 0).sum()), 14)
    assert r["n_nan"] == int(np.isnan(x).sum()) == 3 and r["n_inf"] == int(np.isinf(x).sum()) == 2 and r["n_zero"] == 2
    f = x[np.isfinite(x)].astype(np.float64)
    assert r["sum"] == float(f.sum()) and r["sumsq"] == float((f * f).sum())
    assert r["min"] == np.float32(-1e18) and r["max"] == np.float32(1e18)
    # denormals are finite and non-zero, and they are the extremes of a tensor that holds nothing else
    d = R.stats64(_bits(0x00000001, 0x80011171))
    assert d["n_zero"] == 0 and d["min"] == _bits(0x80011171)[0] and d["max"] == _bits(0x00000001)[0] and d["min"] < 0 < d["max"]
    # no finite element: min +inf, max -inf, sums 0
    e = R.stats64(_bits(0x7F800000, 0xFFC00000, 0xFF800000))
    assert np.isposinf(e["min"]) and np.isneginf(e["max"]) and e["sum"] == 0.0 and e["sumsq"] == 0.0 and e["n_nan"] == 1 and e["n_inf"] == 2
    z = R.stats64(np.zeros(0, dtype=np.float32))
    assert z["numel"] == 0 and np.isposinf(z["min"]) and np.isneginf(z["max"])
    # the difference mode: inf - inf is a NaN
    a, b = np.array([np.inf, 1.0, -np.inf, 2.0], dtype=np.float32), np.array([np.inf, 1.0, np.inf, 0.5], dtype=np.float32)
    dd = R.stats64(R.difference(a, b))
    assert (dd["n_nan"], dd["n_inf"], dd["n_zero"], dd["sum"]) == (1, 1, 1, 1.5)


def test_chain_depth_follows_the_documented_order():
    C = CHUNK
    assert R.chunks_of(0, C) == 1 and R.chunks_of(C, C) == 1 and R.chunks_of(C + 1, C) == 2
    # lane terms + tail + pairing + butterfly + waves + finish lane + finish butterfly
    assert R.chain_depth(1, C) == 0 + 1 + 2 + 6 + 2 + 1 + 6
    assert R.chain_depth(4, C) == 1 + 0 + 2 + 6 + 2 + 1 + 6
    assert R.chain_depth(1025, C) == 1 + 1 + 2 + 6 + 2 + 1 + 6            # 256 groups: one per lane
    assert R.chain_depth(1029, C) == 2 + 1 + 2 + 6 + 2 + 1 + 6
    assert R.chain_depth(C, C) == 32 + 0 + 2 + 6 + 2 + 1 + 6
    assert R.chain_depth(5 * C + 1029, C) == 32 + 1 + 2 + 6 + 2 + 1 + 6
    assert R.chain_depth(64 * C + 1, C) == 32 + 1 + 2 + 6 + 2 + 2 + 6       # 65 chunks: lane 0 of the finish adds two


@pytest.mark.parametrize("numel", [1, 3, 5, 257, 1023, 1029, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3, 5 * CHUNK + 1029, 65 * CHUNK + 7])
def test_float32_replay_of_the_order_stays_inside_the_bound(numel):
    """The bound is a statement about the ORDER: a numpy float32 replay of it, on signed and on all-positive data (where every
    rounding can pull the same way), errs by less than the bound and uses a visible part of it."""
    g = np.random.default_rng(numel)
    for name, x in (("uniform", g.uniform(-4, 4, numel)), ("positive", g.uniform(1, 2, numel))):
        x = x.astype(np.float32)
        q, s = R.replay32(x, CHUNK)
        want = R.stats64(x)
        bs, bq = R.bounds(x, CHUNK)
        es, eq = abs(float(s) - want["sum"]), abs(float(q) - want["sumsq"])
        assert es <= bs and eq <= bq, (name, es / bs, eq / bq)
        assert bq <= (R.chain_depth(numel, CHUNK) + 1) * R.EPS32 * want["sumsq"] * (1 + 1e-9) + numel * 2.0 ** -150
    # exactly representable data: the replay is exact, whatever the order
    k = np.arange(numel, dtype=np.float32) % 7 - 3
    q, s = R.replay32(k, CHUNK)
    assert float(q) == float((k.astype(np.float64) ** 2).sum()) and float(s) == float(k.astype(np.float64).sum())


def test_replay_skips_non_finite_elements_and_check_record_applies_the_rules():
    x = np.concatenate([np.arange(1, 9, dtype=np.float32), _bits(0x7FC00000, 0xFF800000), np.array([-0.0], dtype=np.float32)])
    q, s = R.replay32(x, CHUNK)
    assert float(q) == 204.0 and float(s) == 36.0
    good = {"sumsq": q, "sum": s, "min": np.float32(-0.0), "max": np.float32(8), "n_nan": 1, "n_inf": 1, "n_zero": 1, "numel": 11}
    assert R.check_record(good, x, CHUNK) == 0.0
    for k, v in (("n_zero", 0), ("min", np.float32(1)), ("sum", np.float32(36.01)), ("sumsq", np.float32(204.1)), ("numel", 12)):
        with pytest.raises(AssertionError):
            R.check_record({**good, k: v}, x, CHUNK)
    big = np.array([R.FLT_MAX, 1.0], dtype=np.float32)
    assert R.sumsq_overflows(big, CHUNK)
    rec = {"sumsq": np.float32(np.inf), "sum": np.float32(R.FLT_MAX), "min": np.float32(1), "max": np.float32(R.FLT_MAX), "n_nan": 0, "n_inf": 0,
           "n_zero": 0, "numel": 2}
    R.check_record(rec, big, CHUNK)
    with pytest.raises(AssertionError):
        R.check_record({**rec, "sumsq": np.float32(1e38)}, big, CHUNK)


def _hand_made():
    raw = np.zeros((3, 8), dtype=np.int32)
    f, u = raw.view(np.float32), raw.view(np.uint32)
    f[0, :4] = (25.0, 7.0, -3.0, 4.0)
    u[0, 4:] = (0, 0, 2, 10)
    f[1, :4] = (0.0, 0.0, np.inf, -np.inf)
    u[1, 4:] = (3, 1, 0, 4)
    f[2, :4] = (1e-6, -1e-3, -1e-3, 0.0)
    u[2, 4:] = (0, 0, 4_000_000_000, 4_000_000_001)
    return raw


def test_tensor_stats_object_decodes_a_hand_made_array():
    from ai_font_renderer_amd.engine import TensorStats
    raw = _hand_made()
    for src in (raw, torch.from_numpy(raw)):
        st = TensorStats(src, ["a", "b", "c"])
        assert st.cpu() is st and st.names == ["a", "b", "c"]
        assert st.sumsq.dtype == np.float32 and st.numel.dtype == np.uint32
        assert st.sumsq.tolist() == [25.0, 0.0, np.float32(1e-6)] and st.sum[0] == 7.0 and st.min[0] == -3.0 and st.max[0] == 4.0
        assert np.isposinf(st.min[1]) and np.isneginf(st.max[1])
        assert st.n_nan.tolist() == [0, 3, 0] and st.n_inf.tolist() == [0, 1, 0] and st.n_zero.tolist() == [2, 0, 4_000_000_000]
        assert st.numel.tolist() == [10, 4, 4_000_000_001]                     # unsigned: beyond 2^31
        assert st.norm().dtype == np.float64 and st.norm()[0] == 5.0
        assert st.nonfinite() == ["b"]
        d = R.decode(raw)
        assert all(np.array_equal(d[k], getattr(st, k)) for k in R.FIELDS)
    with pytest.raises(ValueError):
        TensorStats(raw[:, :7].copy(), ["a", "b", "c"]).cpu()
    with pytest.raises(ValueError):
        TensorStats(raw.astype(np.int64), ["a", "b", "c"]).cpu()


def test_tensor_report_setting_is_parsed_strictly(monkeypatch):
    from ai_font_renderer_amd import model as M
    for spec, want in (("1", True), (" 1 ", True), ("", False)):
        monkeypatch.setenv("AFR_TENSOR_REPORT", spec)
        assert M._tensor_report_from_env() is want
    monkeypatch.delenv("AFR_TENSOR_REPORT")
    assert M._tensor_report_from_env() is False
    for spec in ("yes", "0", "2", "true", "on"):
        monkeypatch.setenv("AFR_TENSOR_REPORT", spec)
        with pytest.raises(ValueError, match="AFR_TENSOR_REPORT"):
            M._tensor_report_from_env()


def _stats(names, sumsq, n_zero, numel, n_nan=None, n_inf=None):
    z = [0] * len(names)
    return types.SimpleNamespace(names=list(names), sumsq=np.array(sumsq, dtype=np.float32), n_zero=np.array(n_zero, dtype=np.uint32),
                                 numel=np.array(numel, dtype=np.uint32), n_nan=np.array(n_nan or z, dtype=np.uint32),
                                 n_inf=np.array(n_inf or z, dtype=np.uint32))


def test_tensor_report_lines():
    from ai_font_renderer_amd import model as M
    names = ["fc1.bias", "fc_output.weight"]
    p = _stats(names, [4.0, 100.0], [0, 0], [64, 1000])
    g = _stats(names, [1.0, 0.25], [16, 250], [64, 1000])
    d = _stats(names, [0.0004, 0.01], [0, 0], [64, 1000])
    lines = M._tensor_report_lines(p, g, d)
    assert lines[0] == "Tensor report:" and len(lines) == 3
    assert lines[1] == "  fc1.bias          |p| 2.0000e+00  |g| 1.0000e+00  |g|/|p| 5.000e-01  g zero 0.2500  |dp|/|p| 1.000e-02"
    assert lines[2] == "  fc_output.weight  |p| 1.0000e+01  |g| 5.0000e-01  |g|/|p| 5.000e-02  g zero 0.2500  |dp|/|p| 1.000e-02"
    # non-finite counts only when there are any; a dead head (every gradient of fc_output.weight zero) gets its own line
    g2 = _stats(names, [1.0, 0.0], [16, 1000], [64, 1000], n_nan=[2, 0], n_inf=[0, 0])
    p2 = _stats(names, [4.0, 100.0], [0, 0], [64, 1000], n_inf=[1, 0])
    lines = M._tensor_report_lines(p2, g2, d)
    assert len(lines) == 4 and lines[1].endswith("  NON-FINITE: p 0 nan 1 inf, g 2 nan 0 inf") and "NON-FINITE" not in lines[2]
    assert "g zero 1.0000" in lines[2]
    assert lines[3] == "Tensor report: DEAD OUTPUT HEAD (every gradient of fc_output.weight is zero)"
    # a tensor of zero norm: the ratios have no value
    lines = M._tensor_report_lines(_stats(["w"], [0.0], [4], [4]), _stats(["w"], [1.0], [0], [4]), _stats(["w"], [0.0], [4], [4]))
    assert "|g|/|p| nan" in lines[1] and len(lines) == 2
