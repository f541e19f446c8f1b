"""CPU: the test of the test helper -- tests/op_harness.py must see every fault a single launch can leave behind.  A fake "launch" is a
Python function that writes into the tensors behind the pointers Outs.new returned; one fault at a time is planted, and each must raise
an AssertionError that names the buffer."""
import pytest
import torch

from . import op_harness as H

DTYPES = [torch.float32, torch.bfloat16, torch.int32, torch.uint8]
CHECKED = DTYPES[:3]                              # a uint8 buffer has no value that no kernel writes: its owned part is not searched
SHAPE = (3, 5)


def _value(dtype):
    return torch.arange(15).reshape(SHAPE).to(dtype)


def _outs(dtype, **kw):
    """(Outs on the CPU with buffers "a" and "b" of the dtype, the whole tensor behind "b", its band in elements, b's pointer)"""
    o = H.Outs("cpu")
    o.new("a", 7, torch.float32)
    p = o.new("b", SHAPE, dtype, **kw)
    t, band, n, _ = o.bufs["b"]
    assert n == 15
    return o, t, band, p


def _launch(o, skip=()):
    """a clean launch: every owned element of every buffer is written"""
    for name, (t, band, n, _) in o.bufs.items():
        if name not in skip:
            t[band:band + n] = torch.arange(n).to(t.dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("kw", [{}, dict(guard=5), dict(guard=200), dict(guard=256)], ids=str)
def test_pointers_are_aligned_and_bands_are_whole_multiples_of_256_bytes(dtype, kw):
    o, t, band, p = _outs(dtype, **kw)
    size = t.element_size()
    assert (p.value - t.data_ptr()) == band * size and (band * size) % 256 == 0 and band * size >= 256
    assert band >= kw.get("guard", 0) and t.numel() == 15 + 2 * band                # never narrower than asked for, the same on both sides
    _launch(o)
    got = o.finish()
    assert got["b"].dtype == dtype and tuple(got["b"].shape) == SHAPE and tuple(got["a"].shape) == (7,)
    assert torch.equal(got["b"], _value(dtype))


def test_guarded_bytes_are_the_same_bands():
    buf, view = H.guarded_bytes(40, "cpu")
    assert buf.dtype == torch.uint8 and view.numel() == 40 and view.data_ptr() - buf.data_ptr() == 256 and buf.numel() == 40 + 512
    assert bool((buf == 0xFF).all()) and H.bands_kept(buf) == (True, True)
    view.zero_()
    assert H.bands_kept(buf) == (True, True)
    buf[255] = 0
    assert H.bands_kept(buf) == (False, True)
    buf[255], buf[40 + 256] = 0xFF, 0xFE
    assert H.bands_kept(buf) == (True, False)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_init_preloads_the_owned_part_and_a_launch_in_place_passes(dtype):
    o, t, band, _ = _outs(dtype, init=_value(torch.float32))
    assert torch.equal(t[band:band + 15].reshape(SHAPE), _value(dtype))
    _launch(o, skip=("b",))                                                          # b is left as init made it
    assert torch.equal(o.finish()["b"], _value(dtype))


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("side", ["front", "behind"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_one_element_written_in_a_band_raises(dtype, side, where):
    o, t, band, _ = _outs(dtype, guard=100)
    _launch(o)
    lo = 0 if side == "front" else band + 15
    t[lo if where == "first" else lo + band - 1] = 1
    with pytest.raises(AssertionError, match="^b: the guard band " + ("in front of" if side == "front" else "behind")):
        o.finish()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_another_nan_in_a_band_raises(dtype):
    """the bands are compared by bits: a NaN with another payload or sign is a write"""
    o, t, band, _ = _outs(dtype)
    _launch(o)
    H.bits(t)[band - 1] ^= 1
    with pytest.raises(AssertionError, match="^b: the guard band in front"):
        o.finish()


@pytest.mark.parametrize("at", [0, 7, 14])
@pytest.mark.parametrize("dtype", CHECKED, ids=str)
def test_one_owned_element_left_unwritten_raises_unless_the_buffer_may_keep_its_fill(dtype, at):
    o, t, band, _ = _outs(dtype)
    _launch(o)
    t[band + at] = H._fill(1, dtype, "cpu")[0]
    with pytest.raises(AssertionError, match="^b: 1 elements the kernel owns were not written"):
        o.finish()
    with pytest.raises(AssertionError, match="^b: "):
        o.finish(may_keep_fill=("a",))
    got = o.finish(may_keep_fill=("b",))
    assert torch.equal(H.bits(got["b"].reshape(-1)[at:at + 1]), H.bits(H._fill(1, dtype, "cpu")))


def test_a_uint8_buffer_may_hold_0xff():
    o, t, band, _ = _outs(torch.uint8)
    _launch(o)
    t[band + 3] = 0xFF
    assert int(o.finish()["b"].reshape(-1)[3]) == 0xFF


def test_nothing_written_at_all_raises_for_the_first_buffer():
    o, *_ = _outs(torch.float32)
    with pytest.raises(AssertionError, match="^a: 7 elements"):
        o.finish()


# ------------------------------------------------------------------------------------------------------------------ twice
def _launcher(results):
    it = iter(results)
    return lambda: next(it)


def _result(dtype=torch.float32):
    return "gemm_f32<0,0>", dict(y=torch.tensor([0.0, 1.5, float("nan")]).to(dtype), n=3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_twice_passes_equal_results_a_nan_included_and_returns_the_first(dtype):
    a, b = _result(dtype), _result(dtype)
    assert H.twice(_launcher([a, b])) is a
    t = torch.tensor([1, 2], dtype=torch.uint8)
    assert H.twice(_launcher([t, t.clone()])) is t


@pytest.mark.parametrize("fault", ["low bit", "sign of a zero", "name", "value", "keys", "dtype"])
def test_twice_sees_one_difference(fault):
    a, b = _result(), _result()
    if fault == "low bit":
        H.bits(b[1]["y"])[1] ^= 1
    elif fault == "sign of a zero":
        b[1]["y"][0] = -0.0
        assert bool(a[1]["y"][0] == b[1]["y"][0])                                   # equal as numbers: only the bits differ
    elif fault == "name":
        b = ("gemm_f32<0,1>", b[1])
    elif fault == "value":
        b[1]["n"] = 4
    elif fault == "keys":
        b[1]["z"] = 0
    else:
        b[1]["y"] = b[1]["y"].bfloat16()
    for first, second in ((a, b), (b, a)):
        with pytest.raises(AssertionError, match="a second launch"):
            H.twice(_launcher([first, second]))


# ------------------------------------------------------------------------------------------------------------------ judge
REF = dict(u=torch.zeros(4, dtype=torch.float64), v=torch.ones(2, 2, dtype=torch.float64))
BOUND = dict(u=torch.full((4,), 0.5, dtype=torch.float64), v=torch.tensor(0.25, dtype=torch.float64))


def _got(**change):
    got = dict(u=torch.zeros(4), v=torch.ones(4))                                    # v comes flat: judge gives it the reference's shape
    for k, (i, x) in change.items():
        got[k] = got[k].double()
        got[k][i] = x
    return got


def test_judge_prints_the_line_and_passes_at_exactly_the_bound(capsys):
    H.judge("case 3x5", _got(u=(2, 0.5), v=(1, 1.125)), REF, BOUND, ["u", "v"])
    assert capsys.readouterr().out == "case 3x5: max error / bound u 1.000, v 0.500\n"
    H.judge("case 3x5", dict(dW1=0.25, db1=1.0))
    assert capsys.readouterr().out == "case 3x5: max error / bound dW1 0.250, db1 1.000\n"


@pytest.mark.parametrize("change", [dict(u=(2, 0.5 * 1.0001)), dict(v=(3, 1.0 - 0.25 * 1.0001)), dict(u=(0, float("nan"))), dict(v=(0, float("inf")))],
                         ids=["1.0001 x bound", "1.0001 x bound below", "nan", "inf"])
def test_judge_fails_beyond_the_bound_and_on_a_nan(change):
    with pytest.raises(AssertionError, match="case"):
        H.judge("case", _got(**change), REF, BOUND, ["u", "v"])
    other = "v" if "u" in change else "u"
    H.judge("case", _got(**change), REF, BOUND, [other])                             # the key that is not asked for is not judged


def test_judge_demands_exactness_where_the_bound_is_zero():
    bound = dict(BOUND, u=torch.tensor([0.5, 0.0, 0.5, 0.5], dtype=torch.float64))
    H.judge("case", _got(u=(0, 0.4)), REF, bound, ["u"])
    with pytest.raises(AssertionError):
        H.judge("case", _got(u=(1, 1e-30)), REF, bound, ["u"])
    with pytest.raises(AssertionError):
        H.judge("case", dict(u=1.0001))
    with pytest.raises(AssertionError):
        H.judge("case", dict(u=float("nan")))


def test_bits_of_one_two_and_four_byte_tensors():
    for dtype, view in ((torch.uint8, torch.uint8), (torch.bfloat16, torch.int16), (torch.float16, torch.int16), (torch.float32, torch.int32),
                        (torch.int32, torch.int32)):
        t = torch.tensor([1, 0, 3]).to(dtype)
        assert H.bits(t).dtype == view and H.bits(t).data_ptr() == t.data_ptr()
    assert H.bits(torch.tensor([-0.0])).item() == -2 ** 31 and H.tt(True) == torch.bfloat16 and H.tt(False) == torch.float32
    with pytest.raises(KeyError):
        H.bits(torch.zeros(2, dtype=torch.float64))
