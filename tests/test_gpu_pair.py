"""GPU: the pair tables and the Markov text source (csrc/dataset.hip) -- afr_op_dataset_text_m against synth.lcg_text_markov and, with a
rank-one table, against afr_op_dataset_text_w and afr_op_dataset_text themselves; afr_op_pair_errors against its numpy twin
(tests/pair_ref.py) on synthetic records and on the records of a real afr_op_sheet_char_errors launch; afr_op_pair_weights against
synth.pair_weights on the hand-computed tables (tests/pair_cases.py) and on a table afr_op_pair_errors left on the device; devdata's
surface; AFR_PAIR_REPORT and AFR_STEER_PAIRS in miniature.  Integers only: every comparison is exact.  The op tests launch into guarded
buffers (tests/op_harness.py), twice."""
import ctypes as C

import numpy as np
import pytest
import torch

from ai_font_renderer_amd import _lib
from . import pair_cases as PC
from . import pair_ref as R
from .gpu_util import dev, ptr, stream
from .op_harness import SENTINEL, Outs, bands_kept, guarded_bytes, twice
from .test_pair_cpu import PAIR_ERROR_SHAPES
from .util import load, synth

pytestmark = pytest.mark.gpu

CODE_FILL = int(np.array([SENTINEL, SENTINEL], dtype=np.int32).view(np.int64)[0])     # an int64 of the codes buffer nothing wrote
UPPER = synth.alphabet_members("upper")


def u32(t):
    return t.numpy().view(np.uint32).astype(np.int64)


def u64(t, shape):
    """the int32 words the harness hands back as the unsigned 64-bit counters they are"""
    words = t.numpy().view(np.uint32).astype(np.uint64).reshape(*shape, 2)
    return words[..., 0] | words[..., 1] << np.uint64(32)


def table_dev(cum2):
    return dev(np.ascontiguousarray(np.array(cum2, dtype=np.uint64).astype(np.uint32)).view(np.int32))


def text_m(n, cum2, first_seed=42, seed_rows=None, rows=None, n_rows=None, ldx=100, lo=10, hi=100, want_len=True, want_err=True):
    """afr_op_dataset_text_m twice into guarded buffers -> (int64 [n_rows][ldx] codes, int32 [n_rows] lengths or None, err word or None)"""
    n_rows = n if n_rows is None else n_rows
    sd = None if seed_rows is None else dev(np.asarray(seed_rows, dtype=np.int64))
    rd = None if rows is None else dev(np.asarray(rows, dtype=np.int64))
    cd = table_dev(cum2)
    assert cd.numel() == 95 * 94

    def launch():
        o = Outs()
        codes = o.new("codes", (n_rows, 2 * ldx), torch.int32)
        ln = o.new("len", n_rows, torch.int32) if want_len else None
        err = o.new("err", 1, torch.int32, init=torch.zeros(1, dtype=torch.int32)) if want_err else None
        _lib.check(_lib.lib().afr_op_dataset_text_m(first_seed, ptr(sd), ptr(rd), n, lo, hi, ptr(cd), codes, ldx, ln, err, stream()))
        return o.finish(may_keep_fill=("len", "codes") if rows is not None else ())

    res = twice(launch)
    return res["codes"].numpy().view(np.int64), res["len"].numpy() if want_len else None, int(res["err"][0]) if want_err else None


def text_w(n, cum):
    cd = dev(np.asarray(cum, dtype=np.uint32).view(np.int32))
    o = Outs()
    codes, ln = o.new("codes", (n, 200), torch.int32), o.new("len", n, torch.int32)
    _lib.check(_lib.lib().afr_op_dataset_text_w(42, None, None, n, 10, 100, ptr(cd), codes, 100, ln, None, stream()))
    res = o.finish()
    return res["codes"].numpy().view(np.int64), res["len"].numpy()


def text_plain(n):
    o = Outs()
    codes, ln = o.new("codes", (n, 200), torch.int32), o.new("len", n, torch.int32)
    _lib.check(_lib.lib().afr_op_dataset_text(42, None, None, n, 10, 100, codes, 100, ln, stream()))
    res = o.finish()
    return res["codes"].numpy().view(np.int64), res["len"].numpy()


def twin_texts(seeds, cum2, lo=10, hi=100):
    return [R.lcg_text_markov(int(s), cum2, lo, hi) for s in seeds]


def pair_errors(codes, per_pos, rows=None, by_init=None):
    """afr_op_pair_errors twice into a guarded table -> uint64 [95][94][4]; by_init: what the table holds before (default zeros)"""
    codes, per_pos = np.ascontiguousarray(codes, dtype=np.int64), np.ascontiguousarray(per_pos, dtype=np.uint32)
    n, ldx = per_pos.shape[0], codes.shape[1]
    cd, pd, rd = dev(codes), dev(per_pos.view(np.int32)), None if rows is None else dev(np.asarray(rows, dtype=np.int64))
    init = np.zeros((95, 94, 4), dtype=np.uint64) if by_init is None else by_init
    init = torch.from_numpy(np.ascontiguousarray(init).view(np.int32))

    def launch():
        o = Outs()
        by = o.new("by_pair", (95, 94, 8), torch.int32, init=init)
        _lib.check(_lib.lib().afr_op_pair_errors(ptr(cd), ldx, ptr(rd), n, ptr(pd), by, stream()))
        return o.finish()

    return u64(twice(launch)["by_pair"], (95, 94, 4))


def pair_weights(by, members, floor_w, gain, min_chars, want_w2=True, by_dev=None):
    """afr_op_pair_weights twice into guarded buffers -> (cum2, w2 or None) as lists of lists"""
    if by_dev is None and by is not None:
        by_dev = dev(np.ascontiguousarray(by).view(np.int64))
    words = (C.c_uint32 * 3)(*synth.members_words(members))

    def launch():
        o = Outs()
        cum2 = o.new("cum2", (95, 94), torch.int32)
        w2 = o.new("w2", (95, 94), torch.int32) if want_w2 else None
        _lib.check(_lib.lib().afr_op_pair_weights(ptr(by_dev), words, floor_w, gain, min_chars, cum2, w2, stream()))
        return o.finish()

    res = twice(launch)
    return u32(res["cum2"]).tolist(), u32(res["w2"]).tolist() if want_w2 else None


# ---------------------------------------------------------------------------------------------- text kernel
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_rank_one_table_is_dataset_text_w_and_dataset_text(n):
    want, want_len = text_plain(n)
    assert np.array_equal(want, synth.encode_strings([synth.lcg_text(42 + i) for i in range(n)], 100))
    for f in (1, 4096):
        cum, w = synth.text_weights(None, UPPER, f, 0)
        got_w, len_w = text_w(n, cum)
        codes, lens, err = text_m(n, R.pair_table(R.rank_one(w)))
        assert err == 0 and np.array_equal(codes, want) and np.array_equal(lens, want_len), f
        assert np.array_equal(codes, got_w) and np.array_equal(lens, len_w), f
    from . import text_cases
    cum, w = synth.text_weights(text_cases.steer_table(), synth.alphabet_members("alnum"), 1024, 3072)      # a steered table, not A-Z alone
    got_w, len_w = text_w(n, cum)
    codes, lens, err = text_m(n, R.pair_table(R.rank_one(w)))
    assert err == 0 and np.array_equal(codes, got_w) and np.array_equal(lens, len_w)


def _check_table(w2, n=300, **kw):
    cum2 = R.pair_table(w2)
    codes, lens, err = text_m(n, cum2, **kw)
    first = kw.get("first_seed", 42)
    strings = twin_texts(range(first, first + n), cum2, kw.get("lo", 10), kw.get("hi", 100))
    assert err == 0 and np.array_equal(codes, synth.encode_strings(strings, kw.get("ldx", 100))) and lens.tolist() == [len(s) for s in strings]
    return strings


def test_chain_and_run_tables():
    strings = _check_table(R.chain_table())
    assert strings[0] == "A ABA AB ABABABABA ABABAB ABABAB" and strings == [R.chain_text(synth.lcg_text(42 + i)) for i in range(300)]
    assert strings[0] != R.markov_no_reset(42, R.pair_table(R.chain_table()))              # the planted fault: no reset at a word's start
    for factor in (8, 64):
        strings = _check_table(R.run_table(factor), n=1000)
        assert max(map(R.longest_run, strings)) >= 5


def test_rows_with_zero_width_entries_and_a_full_total():
    """Rows with zero-width entries in front, inside and at the end, and two rows whose total is 2^32 - 1.  The letters that can be
    drawn (indices 0 '!', 3 '$', 5 '&', 50 'S', 88 'y', 91 '|', 93 '~') lead to non-zero rows only."""
    w2 = [[0] * 94 for _ in range(95)]
    w2[0] = [1, 0, 0, 5, 0, 1] + [0] * 88                               # a word's start: zeros inside and to the end
    w2[1 + 0] = [0] * 3 + [4] + [0] * 90                                # after '!': zeros in front, always '$'
    w2[1 + 3] = [0] * 88 + [1, 0, 0, 5, 0, 1]                           # after '$': the pattern at the end of the row
    w2[1 + 5] = [2 ** 31] + [0] * 49 + [1] + [0] * 42 + [2 ** 31 - 2]   # after '&': total 2^32 - 1, split between both ends
    w2[1 + 88] = [1] + [0] * 49 + [2 ** 32 - 3] + [0] * 42 + [1]        # after 'y': total 2^32 - 1, nearly all on 'S'
    w2[1 + 91] = [0] * 93 + [7]                                         # after '|': always '~'
    w2[1 + 93] = [0] * 3 + [4] + [0] * 90                               # after '~': always '$'
    w2[1 + 50] = [0] * 50 + [1] + [0] * 43                              # after 'S': always 'S'
    cum2 = R.pair_table(w2)
    assert cum2[1 + 5][-1] == cum2[1 + 88][-1] == 2 ** 32 - 1
    strings = _check_table(w2, n=600)
    assert set("".join(strings)) - {" "} == {"!", "$", "&", "y", "|", "~", "S"}


def test_a_reached_zero_row_zero_fills_and_flags():
    w2 = R.chain_table()
    w2[1 + ord("B") - 33] = [0] * 94                                    # after B: nothing.  A word of three letters reaches it
    cum2 = R.pair_table(w2)
    for n in (1, 300):
        codes, lens, err = text_m(n, cum2, lo=1, hi=8, ldx=9)
        plain = [synth.lcg_text(42 + i, 1, 8) for i in range(n)]
        ok = [max(map(len, s.split(" "))) <= 2 for s in plain]
        want = synth.encode_strings([R.chain_text(s) if good else "" for s, good in zip(plain, ok)], 9)
        assert np.array_equal(codes, want) and lens.tolist() == [len(s) if good else 0 for s, good in zip(plain, ok)]
        assert err == (0 if all(ok) else 1) and (n == 1 or (any(ok) and not all(ok)))
    codes, lens, err = text_m(300, cum2, lo=1, hi=8, ldx=9, want_len=False, want_err=False)        # no flag word to set, no lengths
    assert err is None and lens is None and np.array_equal(codes, want)
    # a zero row that no sample reaches sets nothing: words of at most two letters (max_len 2), and the chain itself (rows C.. are zero)
    codes, lens, err = text_m(300, cum2, lo=1, hi=2, ldx=2)
    assert err == 0 and lens.min() >= 1 and set(np.unique(codes).tolist()) <= {0, 32, 65, 66}
    # row 0 zero: every sample stops at its first letter
    w2 = R.chain_table()
    w2[0] = [0] * 94
    for n in (1, 257):
        codes, lens, err = text_m(n, R.pair_table(w2))
        assert err == 1 and not codes.any() and not lens.any() and codes.shape == (n, 100)
    codes, lens, err = text_m(5, [[0] * 94] * 95)
    assert err == 1 and not codes.any() and not lens.any()


def test_shapes():
    w2 = R.run_table(8)
    cum2 = R.pair_table(w2)
    for kw in (dict(lo=1, hi=1, ldx=1), dict(lo=1, hi=1, ldx=5), dict(lo=100, hi=100, ldx=100), dict(lo=3, hi=20, ldx=20), dict(lo=10, hi=100, ldx=104),
               dict(lo=10, hi=256, ldx=256)):
        n = 257
        codes, lens, err = text_m(n, cum2, **kw)
        strings = twin_texts(range(42, 42 + n), cum2, kw["lo"], kw["hi"])
        assert err == 0 and np.array_equal(codes, synth.encode_strings(strings, kw["ldx"])), kw
        assert lens.tolist() == [len(s) for s in strings] and lens.min() >= kw["lo"] and lens.max() <= kw["hi"], kw
        assert not codes[:, kw["hi"]:].any()                                                # the tail behind max_len is zero-filled
    codes, lens, err = text_m(64, cum2, first_seed=43, seed_rows=[7919 * s for s in range(64)], want_len=False, want_err=False)
    assert lens is None and err is None
    assert np.array_equal(codes, synth.encode_strings(twin_texts([43 + 7919 * s for s in range(64)], cum2), 100))
    codes, _, _ = text_m(3, cum2, first_seed=-5)                                            # the seed is taken mod 2^32
    assert np.array_equal(codes, synth.encode_strings(twin_texts([2 ** 32 - 5, 2 ** 32 - 4, 2 ** 32 - 3], cum2), 100))


@pytest.mark.parametrize("n", [1, 257])
def test_row_maps(n):
    """A permuted and gapped out_rows with seed_rows of its own: sample j lands in row rows[j] with seed 42 + seed_rows[j]; the rows in
    between keep the buffer's fill."""
    cum2 = R.pair_table(R.run_table(64))
    n_rows = 2 * n + 3
    perm = np.random.default_rng(n).permutation(n)
    rows, seeds = 2 * perm + 1, 1000 * n_rows + 3 * np.arange(n)
    codes, lens, err = text_m(n, cum2, seed_rows=seeds, rows=rows, n_rows=n_rows)
    want, want_len = np.full((n_rows, 100), CODE_FILL, dtype=np.int64), np.full(n_rows, SENTINEL, dtype=np.int32)
    strings = twin_texts(42 + seeds, cum2)
    want[rows] = synth.encode_strings(strings, 100)
    want_len[rows] = [len(s) for s in strings]
    assert err == 0 and np.array_equal(codes, want) and np.array_equal(lens, want_len)
    codes, _, _ = text_m(n, cum2, rows=rows, n_rows=n_rows)                                 # out_rows alone: seed = 42 + j
    want[rows] = synth.encode_strings(twin_texts(range(42, 42 + n), cum2), 100)
    assert np.array_equal(codes, want)


# ---------------------------------------------------------------------------------------------- pair errors
@pytest.mark.parametrize("n, ldx", PAIR_ERROR_SHAPES)
def test_pair_errors_synthetic(n, ldx):
    """Letters, spaces, codes 0..31 and above 126 as character and as predecessor, records without pixels, dirty codes behind the text."""
    codes, per_pos = R.synthetic_case(n, ldx)
    want = R.pair_errors(codes, per_pos)
    got = pair_errors(codes, per_pos)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    if n >= 3 and ldx >= 5:
        for fault in R.FAULTS:
            assert not np.array_equal(got, R.pair_errors(codes, per_pos, fault=fault)), fault


def test_pair_errors_sums_pass_32_bits_and_add_to_the_table():
    codes = np.full((3, 5), 32, dtype=np.int64)
    codes[:, 1:3] = 87                                                  # " WW  " three times: (word start, W) and (W, W)
    per_pos = np.zeros((3, 6, 4), dtype=np.uint32)
    per_pos[:, 1:3] = 2 ** 32 - 1
    per_pos[:, 5] = 2 ** 32 - 1                                         # the background slot is not read
    want = np.zeros((95, 94, 4), dtype=np.uint64)
    want[0, 54] = want[55, 54] = [3, 3 * (2 ** 32 - 1), 3 * (2 ** 32 - 1), 3 * (2 ** 32 - 1)]
    got = pair_errors(codes, per_pos)
    assert np.array_equal(got, want) and np.array_equal(got, R.pair_errors(codes, per_pos))
    before = np.zeros((95, 94, 4), dtype=np.uint64)
    before[:, :, :] = (np.arange(95 * 94 * 4, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15 >> 4)).reshape(95, 94, 4) >> np.uint64(2)
    got = pair_errors(codes, per_pos, by_init=before)
    assert np.array_equal(got, before + want) and np.array_equal(got, R.pair_errors(codes, per_pos, by_pair=before))


@pytest.mark.parametrize("n", [3, 64])
def test_pair_errors_code_rows_permuted_and_gapped(n):
    n_rows = 2 * n + 3
    codes, per_pos = R.synthetic_case(n, 100, seed=5, n_rows=n_rows)
    rows = 2 * np.random.default_rng(n).permutation(n) + 1
    want = R.pair_errors(codes, per_pos, rows=rows)
    got = pair_errors(codes, per_pos, rows=rows)
    assert np.array_equal(got, want) and not np.array_equal(got, R.pair_errors(codes, per_pos))
    assert not np.array_equal(got, R.pair_errors(codes, per_pos, rows=rows, fault="pos0_reads_previous_row"))


def test_pair_errors_of_a_real_char_errors_launch():
    """afr_op_sheet_char_errors on the fixture atlas leaves per_pos and by_code; afr_op_pair_errors scatters per_pos.  The table is the
    twin's, and summed over the contexts each code's {pixels, sumsq, wrong} are by_code's columns for that code."""
    from . import compose_ref
    from .test_gpu_charerr import launch as char_errors
    from .test_gpu_compose import _atlas
    fx = dict(load("atlas_sheets.npz"))
    A, codes, sheets = _atlas(fx, "mont"), fx["mont/codes"], fx["mont/sheets"]
    geo = compose_ref.geometry(int(A["origin_y"]))
    pred = np.ascontiguousarray(np.roll(sheets, -1, axis=0))            # every sheet measured against its neighbour's
    per_pos, by_code, err = char_errors(A, geo, codes, pred)
    assert err == 0 and per_pos.max() < 2 ** 32
    got = pair_errors(codes, per_pos.astype(np.uint32))
    assert np.array_equal(got, R.pair_errors(codes, per_pos))
    assert int(got[:, :, 0].sum()) > 500 and int(got[0, :, 0].sum()) > 50 and int(got[1:, :, 0].sum()) > 300
    by_context = got.sum(0)
    assert np.array_equal(by_context[:, 1:], by_code[33:127][:, [1, 2, 4]])
    assert (by_context[:, 0] <= by_code[33:127, 0]).all()               # by_code's chars also counts characters that own no pixel


# ---------------------------------------------------------------------------------------------- pair weights
@pytest.mark.parametrize("case", PC.TABLE_CASES, ids=[c[0] for c in PC.TABLE_CASES])
def test_pair_weights_hand_computed(case):
    _, counters, alphabet, floor_w, gain, min_chars, want = case
    members = synth.alphabet_members(alphabet)
    by = PC.by_pair_array(counters)
    cum2, w2 = pair_weights(by, members, floor_w, gain, min_chars)
    assert (cum2, w2) == R.pair_weights(by, members, floor_w, gain, min_chars) == PC.expected(want, [33 + i for i in range(94) if members[i]])
    again, none = pair_weights(by, members, floor_w, gain, min_chars, want_w2=False)
    assert none is None and again == cum2


def test_pair_weights_of_a_table_on_the_device_and_the_texts_drawn_from_it():
    """afr_op_pair_errors leaves a table and afr_op_pair_weights reads it where it lies; devdata's three calls give the same tables and
    the texts drawn from the result are the twin's."""
    from ai_font_renderer_amd import devdata
    atlas = devdata.GlyphAtlas.from_font(None).to("cuda")
    alphabet = "alnum"
    ds = devdata.reference_dataset(64, atlas, alphabet=alphabet)
    codes, sheets = ds.tensors
    pred = sheets.roll(-1, 0).contiguous()
    errors = devdata.char_errors(atlas, codes, pred)
    table = devdata.pair_errors(codes, errors.per_pos)
    assert table.dtype == torch.int64 and tuple(table.shape) == (95, 94, 4) and table.is_cuda
    by = table.cpu().numpy().astype(np.uint64)
    assert np.array_equal(by, R.pair_errors(codes.cpu().numpy(), errors.per_pos.cpu().numpy()))
    assert np.array_equal(by.sum(0)[:, 1:], errors.by_code.cpu().numpy().astype(np.uint64)[33:127][:, [1, 2, 4]])
    rows = torch.arange(63, -1, -1, device="cuda")
    twice_over = devdata.pair_errors(codes, devdata.char_errors(atlas, codes, pred.flip(0).contiguous(), rows=rows).per_pos, rows=rows, by_pair=table.clone())
    assert torch.equal(twice_over, 2 * table)
    members = synth.alphabet_members(alphabet)
    for min_chars in (0, 8):
        cum2, w2 = pair_weights(None, members, 1024, 3072, min_chars, by_dev=table)
        want_cum2, want_w2 = R.pair_weights(by, members, 1024, 3072, min_chars)
        assert cum2 == want_cum2 and w2 == want_w2, min_chars
        assert len({v for row in w2 for v in row}) > (20 if min_chars == 0 else 4), min_chars      # few pairs are seen 8 times in 64 sheets
    dcum2, dw2 = devdata.pair_weights(alphabet, table, 1024, 3072, min_chars=8)
    assert dcum2.dtype == torch.int32 and dcum2.is_cuda and dcum2.tolist() == want_cum2 and dw2.tolist() == want_w2
    got, lens = devdata.generate_codes(200, 1000, device="cuda", cum2=dcum2)
    strings = twin_texts(range(1000, 1200), want_cum2)
    assert np.array_equal(got.cpu().numpy(), synth.encode_strings(strings, 100)) and lens.tolist() == [len(s) for s in strings]
    flat, _ = devdata.pair_weights("upper", device="cuda")
    got, _ = devdata.generate_codes(100, device="cuda", cum2=flat)
    assert np.array_equal(got.cpu().numpy(), synth.encode_strings([synth.lcg_text(42 + i) for i in range(100)], 100))
    with pytest.raises(ValueError):
        devdata.generate_codes(4, device="cuda", cum=devdata.text_weights("upper", device="cuda")[0], cum2=flat)
    with pytest.raises(ValueError):
        devdata.generate_codes(4, device="cuda", cum2=torch.zeros((95, 94), dtype=torch.int32, device="cuda"))


def test_refusals_launch_nothing():
    """What the three entries refuse (the cases of tests/test_pair_cpu.py, here with real buffers): the error comes back and the outputs
    keep their fill."""
    lib, EI, EU = _lib.lib(), _lib.AFR_EINVAL, _lib.AFR_EUNSUPPORTED
    table_bytes, cum_bytes = 95 * 94 * 4 * 8, 95 * 94 * 4
    whole, own = guarded_bytes(table_bytes + 2 * cum_bytes + 2048 + 16)
    base = own.data_ptr()
    by, cum2, w2, codes = (C.c_void_p(base + off) for off in (0, table_bytes, table_bytes + cum_bytes, table_bytes + 2 * cum_bytes))
    good = table_dev(R.pair_table(R.run_table(8)))
    src = dev(np.full((2, 100), 87, dtype=np.int64))
    per_pos = dev(np.ones((2, 101, 4), dtype=np.int32))
    up = (C.c_uint32 * 3)(*synth.members_words(UPPER))
    off = lambda p, k: C.c_void_p(p.value + k)
    calls = [
        (EI, lambda: lib.afr_op_dataset_text_m(42, None, None, 1, 10, 100, None, codes, 100, None, None, stream())),
        (EI, lambda: lib.afr_op_dataset_text_m(42, None, None, 1, 10, 100, C.c_void_p(good.data_ptr() + 2), codes, 100, None, None, stream())),
        (EI, lambda: lib.afr_op_dataset_text_m(42, None, None, 1, 10, 101, ptr(good), codes, 100, None, None, stream())),
        (EI, lambda: lib.afr_op_dataset_text_m(42, None, None, 0, 10, 100, ptr(good), codes, 100, None, None, stream())),
        (EI, lambda: lib.afr_op_dataset_text_m(42, None, None, 1, 10, 100, ptr(good), off(codes, 4), 100, None, None, stream())),
        (EU, lambda: lib.afr_op_dataset_text_m(42, None, None, 1, 10, 100, ptr(good), codes, 257, None, None, stream())),
        (EI, lambda: lib.afr_op_pair_errors(None, 100, None, 2, ptr(per_pos), by, stream())),
        (EI, lambda: lib.afr_op_pair_errors(ptr(src), 100, None, 2, None, by, stream())),
        (EI, lambda: lib.afr_op_pair_errors(ptr(src), 100, None, 2, ptr(per_pos), None, stream())),
        (EI, lambda: lib.afr_op_pair_errors(ptr(src), 100, None, 0, ptr(per_pos), by, stream())),
        (EI, lambda: lib.afr_op_pair_errors(ptr(src), 0, None, 2, ptr(per_pos), by, stream())),
        (EU, lambda: lib.afr_op_pair_errors(ptr(src), 257, None, 2, ptr(per_pos), by, stream())),
        (EI, lambda: lib.afr_op_pair_errors(ptr(src), 100, None, 2, ptr(per_pos), off(by, 4), stream())),
        (EI, lambda: lib.afr_op_pair_errors(ptr(src), 100, None, 2, C.c_void_p(per_pos.data_ptr() + 8), by, stream())),
        (EI, lambda: lib.afr_op_pair_errors(C.c_void_p(src.data_ptr() + 4), 100, None, 2, ptr(per_pos), by, stream())),
        (EI, lambda: lib.afr_op_pair_errors(ptr(src), 100, C.c_void_p(src.data_ptr() + 4), 2, ptr(per_pos), by, stream())),
        (EI, lambda: lib.afr_op_pair_weights(None, (C.c_uint32 * 3)(0, 0, 0), 4096, 0, 0, cum2, w2, stream())),
        (EI, lambda: lib.afr_op_pair_weights(None, (C.c_uint32 * 3)(0, 0, 1 << 30), 4096, 0, 0, cum2, w2, stream())),
        (EI, lambda: lib.afr_op_pair_weights(None, up, 0, 0, 0, cum2, w2, stream())),
        (EI, lambda: lib.afr_op_pair_weights(None, up, 65536, 0, 0, cum2, w2, stream())),
        (EI, lambda: lib.afr_op_pair_weights(None, up, 4096, 65536, 0, cum2, w2, stream())),
        (EI, lambda: lib.afr_op_pair_weights(off(by, 4), up, 4096, 1, 0, cum2, w2, stream())),
        (EI, lambda: lib.afr_op_pair_weights(None, up, 4096, 0, 0, off(cum2, 2), w2, stream())),
        (EI, lambda: lib.afr_op_pair_weights(None, up, 4096, 0, 0, cum2, off(w2, 1), stream())),
        (EI, lambda: lib.afr_op_pair_weights(None, up, 4096, 0, 0, None, w2, stream())),
        (EI, lambda: lib.afr_op_pair_weights(None, None, 4096, 0, 0, cum2, w2, stream())),
    ]
    for i, (want, call) in enumerate(calls):
        assert call() == want, i
    torch.cuda.synchronize()
    assert all(bands_kept(whole)) and bool((own == 0xFF).all())


# ---------------------------------------------------------------------------------------------- CLI
def _run_cli(M, monkeypatch, name, report=None, share=0.0, epochs=2, fresh=True):
    monkeypatch.setattr(M, "NUM_SAMPLES", 96)
    monkeypatch.setattr(M, "NUM_EPOCHS", epochs)
    monkeypatch.setattr(M, "OUTPUT_DIR", name)
    monkeypatch.setattr(M, "DEVICE_DATA", "default")
    monkeypatch.setattr(M, "FRESH_DATA", fresh)
    monkeypatch.setattr(M, "ALPHABET", None)
    monkeypatch.setattr(M, "STEER", 0.0)
    monkeypatch.setattr(M, "PAIR_REPORT", report)
    monkeypatch.setattr(M, "STEER_PAIRS", share)
    torch.manual_seed(42)


def test_cli_pair_report_changes_nothing_else(tmp_path, monkeypatch, capsys):
    """AFR_PAIR_REPORT=3 under fresh data, two epochs: the same font_renderer.pth and, but for the report's block, the same lines as the
    run without it; one more line of config.txt; pair_errors.tsv holds the table's non-zero records."""
    from ai_font_renderer_amd import model as M
    monkeypatch.chdir(tmp_path)
    out, pth = {}, {}
    for name, report in (("out_plain", None), ("out_pairs", 3)):
        _run_cli(M, monkeypatch, name, report=report)
        M.main(["model.py", "--train"])
        out[name] = [l.replace(name, "DIR") for l in capsys.readouterr().out.splitlines()]
        pth[name] = torch.load(tmp_path / "font_renderer.pth", weights_only=True)
    at = out["out_pairs"].index(next(l for l in out["out_pairs"] if l.startswith("Pair report:")))
    seen = int(out["out_pairs"][at].split()[2])
    assert out["out_pairs"][at] == f"Pair report: {seen} pairs seen 8 times or more" and seen >= 1
    block = out["out_pairs"][at:at + 1 + min(3, seen)]
    assert out["out_pairs"][:at] + out["out_pairs"][at + len(block):] == out["out_plain"] and out["out_pairs"][at - 1].startswith("Epoch 0,")
    assert all(l.startswith("  '") and " after " in l and ": rms level error " in l and ", wrong ink " in l and ", chars " in l for l in block[1:])
    assert list(pth["out_plain"]) == list(pth["out_pairs"])
    for key in pth["out_plain"]:
        assert torch.equal(pth["out_plain"][key].view(torch.int32), pth["out_pairs"][key].view(torch.int32)), key
    cfg = [(tmp_path / d / "config.txt").read_text().splitlines() for d in ("out_plain", "out_pairs")]
    assert cfg[1] == cfg[0] + ["pair_report = 3"]
    assert not (tmp_path / "out_plain" / "epoch_0" / "pair_errors.tsv").exists()
    tsv = [l.split("\t") for l in (tmp_path / "out_pairs" / "epoch_0" / "pair_errors.tsv").read_text().splitlines()]
    assert tsv[0] == ["prev", "prev_char", "code", "char", "chars", "pixels", "sumsq", "wrong"] and len(tsv) > 100
    assert all(65 <= int(r[2]) <= 90 and int(r[4]) > 0 and int(r[5]) > 0 for r in tsv[1:]) and any(r[0] == "" for r in tsv[1:])
    chars = {(r[1], r[3]): int(r[4]) for r in tsv[1:]}
    for l in block[1:]:                                                 # the listed pairs: seen 8 times or more, as the table says
        c, p = l.split("'")[1], l.split(" after ")[1].split(":")[0]
        assert chars[("" if p == "word start" else p.strip("'"), c)] == int(l.rsplit("chars ", 1)[1]) >= 8


def test_cli_steer_pairs_in_miniature(tmp_path, monkeypatch, capsys):
    """AFR_STEER_PAIRS under fresh data, six epochs of 96 sheets.  Share 0: the rewritten rows are lcg_text's and no line is added.  Share
    0.5: epoch 0 is the same; the training rows after the last rewrite are the twin's texts for the table the twin builds from the pair
    table the validation pass before it left; the validation rows never change; the status line names the heaviest pairs."""
    from ai_font_renderer_amd import devdata, model as M
    monkeypatch.chdir(tmp_path)
    made = []
    fresh_rows = M._fresh_rows
    monkeypatch.setattr(M, "_fresh_rows", lambda *a: made.append(fresh_rows(*a)) or made[-1])
    N, E = 96, 6
    order = M._EpochOrder(N)
    tr, va = order.train_idx, order.val_idx
    atlas = devdata.GlyphAtlas.from_font(None).to("cuda")
    first = devdata.reference_dataset(N, atlas)
    lines, rows = {}, {}
    for name, share in (("out_zero", 0.0), ("out_half", 0.5)):
        _run_cli(M, monkeypatch, name, share=share, epochs=E)
        model = M.train_string_renderer()
        lines[name] = [l.replace(name, "DIR") for l in capsys.readouterr().out.splitlines()]
        x, _, t = model.engine._ds[:3]
        rows[name] = (x.cpu(), t.view(N, 80, 240).cpu())
        assert torch.equal(rows[name][0][va], first.tensors[0][va].cpu()) and torch.equal(rows[name][1][va], first.tensors[1][va].cpu())
    L = first.tensors[0].shape[1]
    zero, half = made
    assert zero.w2 is None and not any(l.startswith("Steer pairs:") for l in lines["out_zero"])
    assert torch.equal(rows["out_zero"][0][tr], torch.from_numpy(synth.encode_strings([synth.lcg_text(42 + (E - 1) * N + int(r), 10, L) for r in tr], L)))
    assert "steer" not in (tmp_path / "out_zero" / "config.txt").read_text()
    assert (tmp_path / "out_half" / "config.txt").read_text().splitlines()[-2:] == ["fresh_data = 1", "steer_pairs = 0.5"]
    e0 = [[l for l in lines[k] if l.startswith("Epoch 0,")] for k in ("out_zero", "out_half")]
    assert len(e0[0]) == 1 and e0[0] == e0[1]
    # the last rewrite, before epoch 5: the pair table of epoch 4's validation pass -> weights -> texts
    table = half.by_pair.cpu().numpy().astype(np.uint64)
    assert len(va) == 19 and int(table[:, 32:58, 0].sum()) == int(table[:, :, 0].sum()) > 300 and int(table[:, :, 2].sum()) > 0
    cum2, w2 = R.pair_weights(table, UPPER, 2048, 2048, 8)
    assert half.w2.tolist() == w2
    assert len({v for row in w2 for v in row}) >= 3                     # 0, the average, and what 19 sheets show 8 times or more
    strings = [R.lcg_text_markov(42 + (E - 1) * N + int(r), cum2, 10, L) for r in tr]
    want_x = torch.from_numpy(synth.encode_strings(strings, L))
    assert torch.equal(rows["out_half"][0][tr], want_x) and not torch.equal(want_x, rows["out_zero"][0][tr])
    assert torch.equal(rows["out_half"][1][tr], devdata.compose_sheets(atlas, want_x).cpu())
    steer = [l for l in lines["out_half"] if l.startswith("Steer pairs:")]
    top = sorted(((p, c) for p in range(95) for c in range(94) if w2[p][c]), key=lambda e: (-w2[e[0]][e[1]], e))[:5]
    assert len(steer) == 1 and steer[0].startswith("Steer pairs: share 0.5, heaviest 5 pairs "
                                                   + f"{M._PairReport.name(*top[0])} x{w2[top[0][0]][top[0][1]] / 4096:.2f}")
    assert lines["out_half"][lines["out_half"].index(steer[0]) - 1].startswith("Epoch 5,")
