"""CPU: the Python twins of the weighted text source (synth.lcg_text_weighted, synth.text_weights, synth.alphabet_members) -- the twin
against synth.lcg_text where the two must agree, the letter table against hand-computed tables (tests/text_cases.py), the alphabet
parser, the letter statistics of steered texts, and what the two library entries and the two CLI switches refuse.  Integers only."""
import ctypes as C

import numpy as np
import pytest

from . import text_cases as TC
from .util import synth


def test_uniform_upper_case_equals_lcg_text():
    """Equal weights f on A-Z: ((state * 26 f) >> 32) / f == (state * 26) >> 32, so the texts are lcg_text's from the same draws."""
    up = synth.alphabet_members("upper")
    for f in (1, 4096):
        cum, w = synth.text_weights(None, up, f, 0)
        assert cum[-1] == 26 * f and w[65 - 33] == f and w[64 - 33] == 0 and w[91 - 33] == 0
        for seed in range(42, 3042):
            assert synth.lcg_text_weighted(seed, cum) == synth.lcg_text(seed), (f, seed)
    cum, _ = synth.text_weights(None, up, 7, 0)
    assert synth.lcg_text_weighted(7, cum, 3, 20) == synth.lcg_text(7, 3, 20)
    assert synth.lcg_text_weighted(42 - 2 ** 32, cum) == synth.lcg_text(42)          # the seed is taken mod 2^32
    with pytest.raises(ValueError):
        synth.lcg_text_weighted(42, [0] * 94)


@pytest.mark.parametrize("case", TC.TABLE_CASES, ids=[c[0] for c in TC.TABLE_CASES])
def test_text_weights_hand_computed(case):
    _, counters, alphabet, floor_w, gain, want = case
    members = synth.alphabet_members(alphabet)
    assert sorted(want) == [33 + i for i in range(94) if members[i]]
    cum, w = synth.text_weights(TC.by_code_array(counters), members, floor_w, gain)
    want_cum, want_w = TC.expected(want)
    assert w == want_w and cum == want_cum
    assert all(isinstance(v, int) for v in cum + w) and max(w) <= 65535 * 17 and cum[-1] < 2 ** 27


def test_text_weights_refuses_bad_arguments():
    up = synth.alphabet_members("upper")
    for members, floor_w, gain in (([0] * 94, 1, 0), (up[:93], 1, 0), (up, 0, 0), (up, 65536, 0), (up, 1, 65536), (up, 1, -1)):
        with pytest.raises(ValueError):
            synth.text_weights(None, members, floor_w, gain)


def test_alphabet_members():
    def codes(spec):
        return [33 + i for i, m in enumerate(synth.alphabet_members(spec)) if m]

    assert codes("upper") == list(range(65, 91)) and codes("lower") == list(range(97, 123))
    assert codes("letters") == list(range(65, 91)) + list(range(97, 123))
    assert codes("alnum") == list(range(48, 58)) + list(range(65, 91)) + list(range(97, 123))
    assert codes("ascii") == list(range(33, 127))
    assert codes("AZaz09,.") == sorted(map(ord, "AZaz09,."))
    assert codes("ABBA") == [65, 66] and codes("!~") == [33, 126]
    assert codes("Upper") == sorted(set(map(ord, "Upper")))                     # not a name: a literal
    assert codes("uper") == sorted(set(map(ord, "uper")))
    for bad in ("A B", " ", "", "café", "A\tB", "A\x7f", "\x00", None, 65, ["A"]):
        with pytest.raises(ValueError):
            synth.alphabet_members(bad)
    assert synth.members_words(synth.alphabet_members("!@A`a~")) == [1 | 1 << 31, 1 | 1 << 31, 1 | 1 << 29]
    assert synth.members_words(synth.alphabet_members("ascii")) == [0xFFFFFFFF, 0xFFFFFFFF, 0x3FFFFFFF]


def test_extreme_tables_draw_only_what_has_weight():
    """Zero-width entries in front, inside and at the end; a total of 2^32 - 1; a single member."""
    w = [0] * 94
    w[1], w[4], w[6] = 1, 5, 1                                                  # the [1, 0, 0, 5, 0, 1] pattern behind a leading zero
    cum = np.cumsum(w).tolist()
    seen = set("".join(synth.lcg_text_weighted(s, cum) for s in range(300))) - {" "}
    assert seen == {chr(34), chr(37), chr(39)}
    w = [0] * 94
    w[0], w[50], w[93] = 1, 2 ** 32 - 3, 1
    cum = np.cumsum(np.array(w, dtype=np.uint64)).tolist()
    assert cum[-1] == 2 ** 32 - 1
    assert set("".join(synth.lcg_text_weighted(s, cum) for s in range(300))) - {" "} == {chr(83)}
    one = [0] * 60 + [3] * 34
    assert set("".join(synth.lcg_text_weighted(s, one) for s in range(50))) - {" "} == {chr(93)}


def test_steered_letter_statistics():
    """4096 texts drawn with share 0.5 from the committed table: every member's count lies within 5 standard deviations (sqrt of the
    expected count, the Poisson bound of a multinomial cell) of total letters * w / sum(w); non-members are never drawn.  Measured on
    the twin: the largest deviation is printed (1.748 over 198 842 letters, 56 453 of them W)."""
    members = synth.alphabet_members("upper")
    cum, w = synth.text_weights(TC.steer_table(), members, 2048, 2048)
    assert max(w) == w[ord("W") - 33] and max(w) > 8 * sorted(x for x in w if x)[13]        # W is steered hard
    count = np.zeros(128, dtype=np.int64)
    for seed in range(1000, 1000 + 4096):
        count += np.bincount(np.frombuffer(synth.lcg_text_weighted(seed, cum).encode(), dtype=np.uint8), minlength=128)
    letters = int(count.sum() - count[32])
    got = count[33:127]
    want = np.array(w, dtype=np.float64) * letters / cum[-1]
    assert count[:32].sum() == 0 and count[127] == 0 and (got[want == 0] == 0).all()
    z = np.abs(got - want)[want > 0] / np.sqrt(want[want > 0])
    print(f"steered texts: {letters} letters, W {got[ord('W') - 33]} of them, max |count - expected| / sqrt(expected) = {z.max():.3f}")
    assert z.max() < 5.0


def test_the_two_entries_refuse_bad_arguments_before_any_launch():
    from ai_font_renderer_amd import _lib
    lib = _lib.lib()
    EI, EU = _lib.AFR_EINVAL, _lib.AFR_EUNSUPPORTED
    fk = C.c_void_p(0x1000)

    def text(seed_rows=None, out_rows=None, n=4, lo=10, hi=100, cum=fk, codes=fk, ldx=100, ln=None, err=None):
        return lib.afr_op_dataset_text_w(42, seed_rows, out_rows, n, lo, hi, cum, codes, ldx, ln, err, None)

    assert text(codes=None) == EI and b"null" in lib.afr_last_error()
    assert text(cum=None) == EI and b"null" in lib.afr_last_error()
    assert text(n=0) == EI and b"n = 0" in lib.afr_last_error()
    assert text(lo=0) == EI and text(lo=11, hi=10) == EI and text(hi=101) == EI and b"min_len" in lib.afr_last_error()
    assert text(ldx=0) == EI
    assert text(ldx=257) == EU and b"256" in lib.afr_last_error()
    for kw in (dict(codes=C.c_void_p(0x1004)), dict(ln=C.c_void_p(0x1002)), dict(cum=C.c_void_p(0x1002)), dict(err=C.c_void_p(0x1001)),
               dict(seed_rows=C.c_void_p(0x1004)), dict(out_rows=C.c_void_p(0x1004))):
        assert text(**kw) == EI and b"aligned" in lib.afr_last_error(), kw

    def weights(by=fk, n_codes=127, members=(0, 0x3FFFFFF, 0), floor_w=4096, gain=0, cum=fk, w=None):
        return lib.afr_op_text_weights(by, n_codes, (C.c_uint32 * 3)(*members) if members is not None else None, floor_w, gain, cum, w, None)

    assert weights(cum=None) == EI and weights(members=None) == EI and b"null" in lib.afr_last_error()
    assert weights(n_codes=126) == EI and b"n_codes" in lib.afr_last_error()
    assert weights(members=(0, 0, 0)) == EI and b"empty" in lib.afr_last_error()
    assert weights(members=(0, 0, 1 << 30)) == EI and weights(members=(1, 0, 1 << 31)) == EI and b"bit 93" in lib.afr_last_error()
    assert weights(floor_w=0) == EI and weights(floor_w=65536) == EI and weights(gain=65536) == EI and b"floor_w" in lib.afr_last_error()
    for kw in (dict(by=C.c_void_p(0x1004)), dict(cum=C.c_void_p(0x1002)), dict(w=C.c_void_p(0x1001))):
        assert weights(**kw) == EI and b"aligned" in lib.afr_last_error(), kw


def test_cli_switches_are_parsed(monkeypatch):
    from ai_font_renderer_amd import model as M
    names = ("AFR_DEVICE_DATA", "AFR_FRESH_DATA", "AFR_ALPHABET", "AFR_STEER")

    def parse(**env):
        for k in names:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        return M._alphabet_from_env(), M._steer_from_env()

    assert parse() == (None, 0.0)
    assert parse(AFR_DEVICE_DATA="default", AFR_ALPHABET="alnum") == ("alnum", 0.0)
    assert parse(AFR_DEVICE_DATA="default", AFR_ALPHABET="AZaz,") == ("AZaz,", 0.0)
    assert parse(AFR_DEVICE_DATA="default", AFR_FRESH_DATA="1", AFR_STEER="0.5") == (None, 0.5)
    assert parse(AFR_DEVICE_DATA="default", AFR_FRESH_DATA="1", AFR_STEER="0") == (None, 0.0)
    for env in (dict(AFR_ALPHABET="alnum"), dict(AFR_DEVICE_DATA="default", AFR_ALPHABET="café"), dict(AFR_DEVICE_DATA="default", AFR_STEER="0.5"),
                dict(AFR_DEVICE_DATA="default", AFR_FRESH_DATA="1", AFR_STEER="1"), dict(AFR_DEVICE_DATA="default", AFR_FRESH_DATA="1", AFR_STEER="-0.1"),
                dict(AFR_DEVICE_DATA="default", AFR_FRESH_DATA="1", AFR_STEER="half"), dict(AFR_DEVICE_DATA="default", AFR_FRESH_DATA="1", AFR_STEER="nan")):
        with pytest.raises(ValueError):
            parse(**env)
    assert M._steer_weights(0.5) == (2048, 2048) and M._steer_weights(0.0) == (4096, 0) and M._steer_weights(0.9999) == (1, 4096)
    up = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"
    assert M._extra_test_strings("upper") == [] and M._extra_test_strings(None) == []
    assert M._extra_test_strings("ascii") == list(M.EXTRA_TEST_STRINGS)
    assert M._extra_test_strings("lower") == [M.EXTRA_TEST_STRINGS[0]]
    assert M._extra_test_strings(up + "0,") == ["0", ","]
