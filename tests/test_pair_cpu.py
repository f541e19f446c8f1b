"""CPU: the Python twins of the pair tables and the Markov text source (synth.lcg_text_markov, synth.pair_weights, synth.pair_table;
tests/pair_ref.py) -- the Markov twin against synth.lcg_text and synth.lcg_text_weighted where the three must agree, a deterministic
chain literally, the pair weights against hand-computed tables (tests/pair_cases.py), the planted faults of tests/pair_ref.py on the
inputs tests/test_gpu_pair.py launches, the pair statistics and run lengths of steered texts, and what the three library entries and the
two CLI switches refuse.  Integers only."""
import ctypes as C

import numpy as np
import pytest

from . import pair_cases as PC
from . import pair_ref as R
from .util import synth

UPPER = synth.alphabet_members("upper")
PAIR_ERROR_SHAPES = [(1, 1), (1, 5), (3, 5), (3, 100), (64, 1), (64, 5), (64, 100), (3, 256)]      # (n, ldx) of the synthetic per_pos cases


def test_rank_one_table_equals_the_weighted_and_the_plain_source():
    """Every row of cum2 the same cum: the context never matters, the draws are afr_op_dataset_text_w's -- and with equal weights on A-Z
    afr_op_dataset_text's and the reference's."""
    for f in (1, 4096):
        cum, w = synth.text_weights(None, UPPER, f, 0)
        cum2 = R.pair_table(R.rank_one(w))
        assert all(row == cum for row in cum2)
        for seed in range(42, 3042):
            text = R.lcg_text_markov(seed, cum2)
            assert text == synth.lcg_text(seed) == synth.lcg_text_weighted(seed, cum), (f, seed)
    cum, w = synth.text_weights(_steer_table(), UPPER, 2048, 2048)
    cum2 = R.pair_table(R.rank_one(w))
    for seed in (7, 42 - 2 ** 32, 99999):
        assert R.lcg_text_markov(seed, cum2, 3, 20) == synth.lcg_text_weighted(seed, cum, 3, 20)
    assert synth.pair_weights(None, UPPER, 4096, 0, 0)[0] == R.pair_table(R.run_table(1))      # equal weights: the live pairs of A-Z


def _steer_table():
    from . import text_cases
    return text_cases.steer_table()


def test_deterministic_chain():
    """Words start with A, after A always B, after B always A: the lengths and spaces of lcg_text, ABAB... in every word."""
    cum2 = R.pair_table(R.chain_table())
    assert R.lcg_text_markov(42, cum2) == "A ABA AB ABABABABA ABABAB ABABAB"
    assert R.lcg_text_markov(43, cum2) == "AB A ABABABABA ABA ABA A ABABABA"
    for seed in range(42, 342):
        assert R.lcg_text_markov(seed, cum2) == R.chain_text(synth.lcg_text(seed)), seed
    assert R.lcg_text_markov(5, cum2, 1, 1) == "A"
    # the planted fault: a context that is carried over the space makes the word after "A" start with B
    assert any(R.markov_no_reset(seed, cum2) != R.lcg_text_markov(seed, cum2) for seed in range(42, 46))
    assert R.markov_no_reset(42, cum2).startswith("A BAB")


def test_a_reached_zero_row_is_an_error_and_an_unreached_one_is_not():
    w2 = R.chain_table()
    w2[1 + ord("B") - 33] = [0] * 94                                     # after B: nothing.  "AB" is fine, "ABA" is not
    cum2 = R.pair_table(w2)
    seeds = range(42, 142)
    short = [s for s in seeds if max(map(len, synth.lcg_text(s, 1, 8).split(" "))) <= 2]
    assert 10 < len(short) < 90
    for s in seeds:
        if s in short:
            assert R.lcg_text_markov(s, cum2, 1, 8) == R.chain_text(synth.lcg_text(s, 1, 8))
        else:
            with pytest.raises(ValueError):
                R.lcg_text_markov(s, cum2, 1, 8)
    zero0 = R.chain_table()
    zero0[0] = [0] * 94
    with pytest.raises(ValueError):
        R.lcg_text_markov(42, R.pair_table(zero0))
    for bad in ([[0] * 94] * 94, [[0] * 93] * 95):
        with pytest.raises(ValueError):
            R.lcg_text_markov(42, bad)


def test_pair_table():
    w2 = [[0] * 94 for _ in range(95)]
    w2[3][0], w2[3][50], w2[3][93] = 1, 2 ** 32 - 3, 1
    cum2 = R.pair_table(w2)
    assert cum2[3][-1] == 2 ** 32 - 1 and cum2[3][0] == 1 and cum2[3][49] == 1 and cum2[3][50] == 2 ** 32 - 2 and cum2[2] == [0] * 94
    assert R.pair_table(np.array(w2, dtype=np.uint64)) == cum2
    w2[3][1] = 1
    with pytest.raises(ValueError):
        R.pair_table(w2)
    w2[3][1] = -1
    with pytest.raises(ValueError):
        R.pair_table(w2)
    for bad in ([[1] * 94] * 94, [[1] * 95] * 95):
        with pytest.raises(ValueError):
            R.pair_table(bad)


@pytest.mark.parametrize("case", PC.TABLE_CASES, ids=[c[0] for c in PC.TABLE_CASES])
def test_pair_weights_hand_computed(case):
    _, counters, alphabet, floor_w, gain, min_chars, want = case
    members = synth.alphabet_members(alphabet)
    cum2, w2 = R.pair_weights(PC.by_pair_array(counters), members, floor_w, gain, min_chars)
    want_cum2, want_w2 = PC.expected(want, [33 + i for i in range(94) if members[i]])
    assert w2 == want_w2 and cum2 == want_cum2
    assert all(isinstance(v, int) for row in cum2 + w2 for v in row) and max(map(max, w2)) <= 65535 * 17 and max(row[-1] for row in cum2) < 2 ** 27
    dead = [p for p in range(1, 95) if not members[p - 1]]
    assert all(cum2[p] == [0] * 94 for p in dead)                       # the rows of non-member contexts are zero


def test_pair_weights_refuses_bad_arguments():
    for members, floor_w, gain, min_chars in (([0] * 94, 1, 0, 0), (UPPER[:93], 1, 0, 0), (UPPER, 0, 0, 0), (UPPER, 65536, 0, 0),
                                              (UPPER, 1, 65536, 0), (UPPER, 1, -1, 0), (UPPER, 1, 1, -1)):
        with pytest.raises(ValueError):
            R.pair_weights(None, members, floor_w, gain, min_chars)


def test_planted_faults_show_on_the_gpu_tests_inputs():
    """Each misreading of afr_op_pair_errors' contract gives another table on the synthetic cases the GPU test launches."""
    shown = {f: 0 for f in R.FAULTS}
    for n, ldx in PAIR_ERROR_SHAPES:
        codes, per_pos = R.synthetic_case(n, ldx)
        want = R.pair_errors(codes, per_pos)
        assert int(want[:, :, 0].sum()) > 0 or ldx == 1
        for fault in R.FAULTS:
            differs = not np.array_equal(R.pair_errors(codes, per_pos, fault=fault), want)
            shown[fault] += differs
            if n >= 3 and ldx >= 5:
                assert differs, (fault, n, ldx)
    assert all(shown.values())
    # the totals do not depend on the context: the sum over contexts is the sum by code of the contributing records
    codes, per_pos = R.synthetic_case(64, 100)
    want = R.pair_errors(codes, per_pos)
    for c in (65, 87, 126):
        at = (codes == c) & (per_pos[:, :100, 0] > 0)
        assert int(want[:, c - 33, 0].sum()) == int(at.sum()) and int(want[:, c - 33, 1].sum()) == int(per_pos[:, :100, 0][at].sum())
    assert int(want[0, :, 0].sum()) > 0 and int(want[1:, :, 0].sum()) > 0      # the word start and the letter contexts are both used


@pytest.mark.parametrize("factor, z_measured, e_min, run", [(8, 3.65, 180, 8), (64, 3.46, 67, 10)])
def test_run_tables_pair_statistics(factor, z_measured, e_min, run):
    """A-Z, every live pair at 4096, the diagonal times `factor`, over the texts of seeds 42..4137: no zero-weight pair is drawn, and
    every pair's count lies within 5 sqrt(e) of e = visits of its row x w / the row's total (the Poisson bound of a multinomial cell;
    the smallest e is 180 and 67, so the normal bound applies to every cell).  Measured on the twin: the largest deviation is 3.65 and
    3.46 standard deviations; the longest run of one letter is 8 and 10, against 4 for lcg_text.  All deterministic."""
    w2 = R.run_table(factor)
    cum2 = R.pair_table(w2)
    count = np.zeros((95, 94), dtype=np.int64)
    longest = 0
    for seed in range(42, 4138):
        text = R.lcg_text_markov(seed, cum2)
        longest = max(longest, R.longest_run(text))
        for word in text.split(" "):
            p = 0
            for ch in word:
                count[p, ord(ch) - 33] += 1
                p = 1 + ord(ch) - 33
    w = np.array(w2, dtype=np.float64)
    total = w.sum(1, keepdims=True)
    e = count.sum(1, keepdims=True) * w / np.where(total > 0, total, 1)
    assert (count[e == 0] == 0).all()
    z = np.abs(count - e)[e > 0] / np.sqrt(e[e > 0])
    print(f"diagonal x{factor}: {int(count.sum())} letters, smallest expected count {e[e > 0].min():.1f}, "
          f"max |count - expected| / sqrt(expected) = {z.max():.3f}, longest run {longest}")
    assert int(e[e > 0].min()) == e_min and round(float(z.max()), 2) == z_measured and z.max() < 5.0
    assert longest == run
    if factor == 64:
        assert max(R.longest_run(synth.lcg_text(seed)) for seed in range(42, 4138)) == 4


def test_the_three_entries_refuse_bad_arguments_before_any_launch():
    from ai_font_renderer_amd import _lib
    lib = _lib.lib()
    EI, EU = _lib.AFR_EINVAL, _lib.AFR_EUNSUPPORTED
    fk = C.c_void_p(0x1000)

    def text(seed_rows=None, out_rows=None, n=4, lo=10, hi=100, cum2=fk, codes=fk, ldx=100, ln=None, err=None):
        return lib.afr_op_dataset_text_m(42, seed_rows, out_rows, n, lo, hi, cum2, codes, ldx, ln, err, None)

    assert text(codes=None) == EI and b"null" in lib.afr_last_error()
    assert text(cum2=None) == EI and b"null" in lib.afr_last_error()
    assert text(n=0) == EI and b"n = 0" in lib.afr_last_error()
    assert text(lo=0) == EI and text(lo=11, hi=10) == EI and text(hi=101) == EI and b"min_len" in lib.afr_last_error()
    assert text(ldx=0) == EI
    assert text(ldx=257) == EU and b"256" in lib.afr_last_error()
    for kw in (dict(codes=C.c_void_p(0x1004)), dict(ln=C.c_void_p(0x1002)), dict(cum2=C.c_void_p(0x1002)), dict(err=C.c_void_p(0x1001)),
               dict(seed_rows=C.c_void_p(0x1004)), dict(out_rows=C.c_void_p(0x1004))):
        assert text(**kw) == EI and b"aligned" in lib.afr_last_error(), kw

    def errors(codes=fk, ldx=100, code_rows=None, n=4, per_pos=fk, by_pair=fk):
        return lib.afr_op_pair_errors(codes, ldx, code_rows, n, per_pos, by_pair, None)

    for kw in (dict(codes=None), dict(per_pos=None), dict(by_pair=None)):
        assert errors(**kw) == EI and b"null" in lib.afr_last_error(), kw
    assert errors(n=0) == EI and b"n = 0" in lib.afr_last_error()
    assert errors(ldx=0) == EI and b"ldx" in lib.afr_last_error()
    assert errors(ldx=257) == EU and b"256" in lib.afr_last_error()
    for kw in (dict(codes=C.c_void_p(0x1004)), dict(code_rows=C.c_void_p(0x1004)), dict(by_pair=C.c_void_p(0x1004)),
               dict(per_pos=C.c_void_p(0x1008))):
        assert errors(**kw) == EI and b"aligned" in lib.afr_last_error(), kw

    def weights(by=fk, members=(0, 0x3FFFFFF, 0), floor_w=4096, gain=0, min_chars=0, cum2=fk, w2=None):
        return lib.afr_op_pair_weights(by, (C.c_uint32 * 3)(*members) if members is not None else None, floor_w, gain, min_chars, cum2, w2, None)

    assert weights(cum2=None) == EI and weights(members=None) == EI and b"null" in lib.afr_last_error()
    assert weights(members=(0, 0, 0)) == EI and b"empty" in lib.afr_last_error()
    assert weights(members=(0, 0, 1 << 30)) == EI and weights(members=(1, 0, 1 << 31)) == EI and b"bit 93" in lib.afr_last_error()
    assert weights(floor_w=0) == EI and weights(floor_w=65536) == EI and weights(gain=65536) == EI and b"floor_w" in lib.afr_last_error()
    for kw in (dict(by=C.c_void_p(0x1004)), dict(cum2=C.c_void_p(0x1002)), dict(w2=C.c_void_p(0x1001))):
        assert weights(**kw) == EI and b"aligned" in lib.afr_last_error(), kw


def test_cli_switches_are_parsed(monkeypatch):
    from ai_font_renderer_amd import model as M
    names = ("AFR_DEVICE_DATA", "AFR_FRESH_DATA", "AFR_STEER", "AFR_PAIR_REPORT", "AFR_STEER_PAIRS")

    def parse(**env):
        for k in names:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        return M._pair_report_from_env(), M._steer_pairs_from_env()

    dd, fd = dict(AFR_DEVICE_DATA="default"), dict(AFR_DEVICE_DATA="default", AFR_FRESH_DATA="1")
    assert parse() == (None, 0.0)
    assert parse(**dd, AFR_PAIR_REPORT="5") == (5, 0.0)
    assert parse(**fd, AFR_STEER_PAIRS="0.5") == (None, 0.5)
    assert parse(**fd, AFR_STEER_PAIRS="0") == (None, 0.0)
    assert parse(**fd, AFR_STEER_PAIRS="0", AFR_STEER="0.5") == (None, 0.0)
    assert parse(**fd, AFR_STEER_PAIRS="0.25", AFR_STEER="0", AFR_PAIR_REPORT="1") == (1, 0.25)
    for env in (dict(AFR_PAIR_REPORT="5"), dict(**dd, AFR_PAIR_REPORT="0"), dict(**dd, AFR_PAIR_REPORT="many"), dict(**dd, AFR_PAIR_REPORT="-1"),
                dict(**dd, AFR_STEER_PAIRS="0.5"), dict(**fd, AFR_STEER_PAIRS="1"), dict(**fd, AFR_STEER_PAIRS="-0.1"),
                dict(**fd, AFR_STEER_PAIRS="half"), dict(**fd, AFR_STEER_PAIRS="nan"), dict(**fd, AFR_STEER_PAIRS="0.5", AFR_STEER="0.5")):
        with pytest.raises(ValueError):
            parse(**env)
    assert M.PAIR_MIN_CHARS == 8
    assert M._PairReport.name(0, 54) == "'W' after word start" and M._PairReport.name(55, 54) == "'W' after 'W'"
