"""CPU: the test of the test helpers -- opt_paths.assert_same_state must see every difference two engines can end a path with.  Two
fake engines with a two-tensor layout (5 and 64 elements, padded to 64-element boundaries), f32 flats, the two bf16 shadows of a glyph
plan, an EMA and t; one fault at a time on one side."""
import copy
from types import SimpleNamespace

import pytest
import torch

from . import opt_paths as OP

LAYOUT = [("a.bias", (5,), 0, 5), ("b.weight", (8, 8), 64, 64)]
N = 128
FLATS = ("flat_params", "exp_avg", "exp_avg_sq", "flat_ema")
BUFFERS = FLATS + ("shadow0", "shadow1")
LIVE, PAD = 66, 17                              # an element of b.weight; an element of the padding behind a.bias


def _fake():
    gen = torch.Generator().manual_seed(3)
    eng = SimpleNamespace(layout=LAYOUT, n_flat=N, dtype="bf16", cfg=SimpleNamespace(kind="glyph"), t=7)
    for nm in FLATS:
        setattr(eng, nm, torch.randn(N, generator=gen))
    eng.workspace = torch.zeros(2 * (2 * N) + 64, dtype=torch.uint8)
    for sh in OP.shadows(eng):
        sh.copy_(torch.randn(N, generator=gen))
    return eng


def _buffer(eng, name):
    return OP.shadows(eng)[int(name[-1])] if name.startswith("shadow") else getattr(eng, name)


def _flip_bit(t, i):
    OP.bits(t)[i] ^= 1                          # the lowest bit of the significand


def test_shadows_of_the_fake_are_two_disjoint_aligned_views():
    a, b = OP.shadows(_fake())
    assert a.numel() == b.numel() == N and (b.data_ptr() - a.data_ptr()) % 256 == 0 and b.data_ptr() - a.data_ptr() >= 2 * N


@pytest.mark.parametrize("padding", [False, True])
def test_equal_engines_pass(padding):
    a = _fake()
    OP.assert_same_state(a, copy.deepcopy(a), "equal", padding=padding)
    OP.assert_tensor_same(a, copy.deepcopy(a), "b.weight", "equal")


@pytest.mark.parametrize("fault", ["bit", "minus-zero", "nan"])
@pytest.mark.parametrize("name", BUFFERS)
def test_one_difference_in_each_compared_buffer_raises(name, fault):
    a = _fake()
    _buffer(a, name)[LIVE] = 0.0
    b = copy.deepcopy(a)
    if fault == "bit":
        _flip_bit(_buffer(b, name), LIVE)
    elif fault == "minus-zero":
        _buffer(b, name)[LIVE] = -0.0
        assert bool(_buffer(a, name)[LIVE] == _buffer(b, name)[LIVE])       # equal as numbers: only the bit patterns differ
    else:
        _buffer(b, name)[LIVE] = float("nan")
    for x, y in ((a, b), (b, a)):
        with pytest.raises(AssertionError):
            OP.assert_same_state(x, y, (name, fault))
    if name != "flat_ema":
        with pytest.raises(AssertionError):
            OP.assert_tensor_same(a, b, "b.weight", (name, fault))
        OP.assert_tensor_same(a, b, "a.bias", (name, fault))                # the other tensor is untouched
    # the switches leave out exactly what they name
    if name == "flat_ema":
        OP.assert_same_state(a, b, (name, fault), ema=False)
    elif name.startswith("shadow"):
        OP.assert_same_state(a, b, (name, fault), shadows=False)
    else:
        with pytest.raises(AssertionError):
            OP.assert_same_state(a, b, (name, fault), ema=False, shadows=False)


def test_nan_on_both_sides_is_the_same_state():
    a = _fake()
    a.exp_avg[LIVE] = float("nan")
    OP.assert_same_state(a, copy.deepcopy(a), "the same NaN")


def test_step_counter_off_by_one_raises():
    a = _fake()
    b = copy.deepcopy(a)
    b.t += 1
    with pytest.raises(AssertionError):
        OP.assert_same_state(a, b, "t")


@pytest.mark.parametrize("name", BUFFERS)
def test_a_flip_in_the_padding_counts_only_with_padding(name):
    a = _fake()
    b = copy.deepcopy(a)
    _flip_bit(_buffer(b, name), PAD)
    OP.assert_same_state(a, b, name)
    with pytest.raises(AssertionError):
        OP.assert_same_state(a, b, name, padding=True)


def test_engines_without_an_ema_or_a_second_moment_or_shadows():
    a = _fake()
    a.flat_ema, a.exp_avg_sq, a.dtype = None, None, "f32"
    b = copy.deepcopy(a)
    OP.assert_same_state(a, b, "lean")
    with pytest.raises(Exception):
        OP.assert_same_state(a, b, "lean", ema=True)                       # asked for, and neither keeps one
    c = _fake()
    c.flat_ema = None
    with pytest.raises(AssertionError):
        OP.assert_same_state(c, b, "one keeps exp_avg_sq, the other does not")
    b.exp_avg[LIVE] += 1.0
    with pytest.raises(AssertionError):
        OP.assert_same_state(a, b, "lean")
