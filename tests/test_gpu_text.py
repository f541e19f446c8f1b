"""GPU: the weighted text source (csrc/dataset.hip) -- afr_op_dataset_text_w against synth.lcg_text_weighted and, with equal weights on
A-Z, against afr_op_dataset_text itself; afr_op_text_weights against synth.text_weights on the hand-computed tables
(tests/text_cases.py) and on a table afr_op_sheet_char_errors left on the device; devdata's surface; AFR_ALPHABET and AFR_STEER in
miniature.  Integers only: every comparison is exact.  The op tests launch into guarded buffers (tests/op_harness.py), twice."""
import ctypes as C

import numpy as np
import pytest
import torch

from ai_font_renderer_amd import _lib
from . import text_cases as TC
from .gpu_util import dev, ptr, stream
from .op_harness import SENTINEL, Outs, bands_kept, guarded_bytes, twice
from .util import synth

pytestmark = pytest.mark.gpu

CODE_FILL = int(np.array([SENTINEL, SENTINEL], dtype=np.int32).view(np.int64)[0])     # an int64 of the codes buffer nothing wrote
UPPER = synth.alphabet_members("upper")


def u32(t):
    return t.numpy().view(np.uint32).astype(np.int64)


def cum_of(w):
    assert len(w) == 94
    return np.cumsum(np.array(w, dtype=np.uint64)).astype(np.uint32)


def text_w(n, cum, first_seed=42, seed_rows=None, rows=None, n_rows=None, ldx=100, lo=10, hi=100, want_len=True, want_err=True):
    """afr_op_dataset_text_w twice into guarded buffers -> (int64 [n_rows][ldx] codes, int32 [n_rows] lengths or None, err word or None)"""
    n_rows = n if n_rows is None else n_rows
    sd = None if seed_rows is None else dev(np.asarray(seed_rows, dtype=np.int64))
    rd = None if rows is None else dev(np.asarray(rows, dtype=np.int64))
    cd = dev(np.asarray(cum, dtype=np.uint32).view(np.int32))

    def launch():
        o = Outs()
        codes = o.new("codes", (n_rows, 2 * ldx), torch.int32)
        ln = o.new("len", n_rows, torch.int32) if want_len else None
        err = o.new("err", 1, torch.int32, init=torch.zeros(1, dtype=torch.int32)) if want_err else None
        _lib.check(_lib.lib().afr_op_dataset_text_w(first_seed, ptr(sd), ptr(rd), n, lo, hi, ptr(cd), codes, ldx, ln, err, stream()))
        return o.finish(may_keep_fill=("len", "codes") if rows is not None else ())

    res = twice(launch)
    return res["codes"].numpy().view(np.int64), res["len"].numpy() if want_len else None, int(res["err"][0]) if want_err else None


def text_plain(n, ldx=100, lo=10, hi=100):
    """afr_op_dataset_text into guarded buffers -> (codes, lengths)"""
    o = Outs()
    codes, ln = o.new("codes", (n, 2 * ldx), torch.int32), o.new("len", n, torch.int32)
    _lib.check(_lib.lib().afr_op_dataset_text(42, None, None, n, lo, hi, codes, ldx, ln, stream()))
    res = o.finish()
    return res["codes"].numpy().view(np.int64), res["len"].numpy()


def twin_texts(seeds, cum, lo=10, hi=100):
    return [synth.lcg_text_weighted(int(s), [int(c) for c in cum], lo, hi) for s in seeds]


def weights(counters, members, floor_w, gain, want_w=True, by_dev=None, n_codes=TC.N_CODES):
    """afr_op_text_weights twice into guarded buffers -> (cum [94], w [94] or None) as integers; counters: uint64 [n_codes + 1][5] on
    the host or None, or by_dev: the table where it lies on the device"""
    if by_dev is None and counters is not None:
        by_dev = dev(np.ascontiguousarray(counters).view(np.int64))
    words = (C.c_uint32 * 3)(*synth.members_words(members))

    def launch():
        o = Outs()
        cum = o.new("cum", 94, torch.int32)
        w = o.new("w", 94, torch.int32) if want_w else None
        _lib.check(_lib.lib().afr_op_text_weights(ptr(by_dev), n_codes, words, floor_w, gain, cum, w, stream()))
        return o.finish()

    res = twice(launch)
    return u32(res["cum"]).tolist(), u32(res["w"]).tolist() if want_w else None


# ---------------------------------------------------------------------------------------------- text kernel
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_uniform_upper_case_is_dataset_text(n):
    """Equal weights on A-Z, 1 and 4096 each: the bytes and lengths of afr_op_dataset_text, which are lcg_text's."""
    want, want_len = text_plain(n)
    assert np.array_equal(want, synth.encode_strings([synth.lcg_text(42 + i) for i in range(n)], 100))
    for f in (1, 4096):
        codes, lens, err = text_w(n, cum_of([f * m for m in UPPER]))
        assert err == 0 and np.array_equal(codes, want) and np.array_equal(lens, want_len), f


def _check_table(w, n=300, **kw):
    cum = cum_of(w)
    codes, lens, err = text_w(n, cum, **kw)
    strings = twin_texts(range(kw.get("first_seed", 42), kw.get("first_seed", 42) + n), cum, kw.get("lo", 10), kw.get("hi", 100))
    assert err == 0 and np.array_equal(codes, synth.encode_strings(strings, kw.get("ldx", 100))) and lens.tolist() == [len(s) for s in strings]
    drawn = set(np.unique(codes).tolist()) - {0, 32}
    assert drawn <= {33 + i for i in range(94) if w[i]}
    return drawn


def test_tables():
    one = [0] * 94
    one[57] = 7
    assert _check_table(one) == {90}                                                        # a single member
    w = [0] * 94
    w[1], w[4], w[6] = 1, 5, 1                                                              # [1, 0, 0, 5, 0, 1] behind a leading zero, zeros to the end
    assert _check_table(w) == {34, 37, 39}
    w = [1, 0, 0, 5, 0, 1] + [0] * 82 + [1, 0, 0, 5, 0, 1]                                  # the pattern at both ends of the table
    assert _check_table(w) == {33, 36, 38, 121, 124, 126}
    edges = [0] * 94
    for c in (33, 64, 65, 96, 97, 126):                                                     # the word edges of the member mask
        edges[c - 33] = 3
    assert _check_table(edges) == {33, 64, 65, 96, 97, 126}
    assert _check_table(synth.alphabet_members("ascii"), n=400) == set(range(33, 127))
    big = [0] * 94
    big[0], big[50], big[93] = 1, 2 ** 32 - 3, 1                                            # total = 2^32 - 1
    assert int(cum_of(big)[-1]) == 2 ** 32 - 1 and _check_table(big) == {83}
    big[0], big[50], big[93] = 2 ** 31, 1, 2 ** 31 - 2                                      # ... split between the first and the last code
    assert int(cum_of(big)[-1]) == 2 ** 32 - 1 and _check_table(big) >= {33, 126}


def test_zero_total_sets_the_flag_and_zero_fills():
    for n in (1, 300):
        codes, lens, err = text_w(n, np.zeros(94, dtype=np.uint32))
        assert err == 1 and not codes.any() and not lens.any() and codes.shape == (n, 100)
    codes, lens, err = text_w(5, np.zeros(94, dtype=np.uint32), want_err=False, want_len=False)      # no flag word to set, no lengths
    assert err is None and lens is None and not codes.any()


def test_shapes():
    cum = cum_of([3 * m for m in synth.alphabet_members("alnum")])
    for kw in (dict(lo=1, hi=1, ldx=1), dict(lo=1, hi=1, ldx=5), dict(lo=100, hi=100, ldx=100), dict(lo=3, hi=20, ldx=20), dict(lo=10, hi=100, ldx=104),
               dict(lo=10, hi=256, ldx=256)):
        n = 257
        codes, lens, err = text_w(n, cum, **kw)
        strings = twin_texts(range(42, 42 + n), cum, kw["lo"], kw["hi"])
        assert err == 0 and np.array_equal(codes, synth.encode_strings(strings, kw["ldx"])), kw
        assert lens.tolist() == [len(s) for s in strings] and lens.min() >= kw["lo"] and lens.max() <= kw["hi"], kw
        assert not codes[:, kw["hi"]:].any()                                                # the tail behind max_len is zero-filled
    codes, lens, err = text_w(64, cum, first_seed=43, seed_rows=[7919 * s for s in range(64)], want_len=False, want_err=False)
    assert lens is None and err is None
    assert np.array_equal(codes, synth.encode_strings(twin_texts([43 + 7919 * s for s in range(64)], cum), 100))
    codes, _, _ = text_w(3, cum, first_seed=-5)                                             # the seed is taken mod 2^32
    assert np.array_equal(codes, synth.encode_strings(twin_texts([2 ** 32 - 5, 2 ** 32 - 4, 2 ** 32 - 3], cum), 100))


@pytest.mark.parametrize("n", [1, 257])
def test_row_maps(n):
    """A permuted and gapped out_rows with seed_rows of its own: sample j lands in row rows[j] with seed 42 + seed_rows[j]; the rows in
    between keep the buffer's fill."""
    cum = cum_of([1 + (i % 5) for i in range(94)])
    n_rows = 2 * n + 3
    perm = np.random.default_rng(n).permutation(n)
    rows, seeds = 2 * perm + 1, 1000 * n_rows + 3 * np.arange(n)
    codes, lens, err = text_w(n, cum, seed_rows=seeds, rows=rows, n_rows=n_rows)
    want, want_len = np.full((n_rows, 100), CODE_FILL, dtype=np.int64), np.full(n_rows, SENTINEL, dtype=np.int32)
    strings = twin_texts(42 + seeds, cum)
    want[rows] = synth.encode_strings(strings, 100)
    want_len[rows] = [len(s) for s in strings]
    assert err == 0 and np.array_equal(codes, want) and np.array_equal(lens, want_len)
    codes, _, _ = text_w(n, cum, rows=rows, n_rows=n_rows)                                  # out_rows alone: seed = 42 + j
    want[rows] = synth.encode_strings(twin_texts(range(42, 42 + n), cum), 100)
    assert np.array_equal(codes, want)


# ---------------------------------------------------------------------------------------------- weights kernel
@pytest.mark.parametrize("case", TC.TABLE_CASES, ids=[c[0] for c in TC.TABLE_CASES])
def test_text_weights_hand_computed(case):
    _, counters, alphabet, floor_w, gain, want = case
    members = synth.alphabet_members(alphabet)
    by = TC.by_code_array(counters)
    cum, w = weights(by, members, floor_w, gain)
    assert (cum, w) == synth.text_weights(by, members, floor_w, gain) == TC.expected(want)
    cum2, none = weights(by, members, floor_w, gain, want_w=False)
    assert none is None and cum2 == cum


def test_text_weights_of_the_steering_table_and_a_wider_one():
    by = TC.steer_table()
    for alphabet, floor_w, gain in (("upper", 2048, 2048), ("ascii", 1, 65535), ("W", 4000, 96), ("letters", 65535, 65535)):
        members = synth.alphabet_members(alphabet)
        assert weights(by, members, floor_w, gain) == synth.text_weights(by, members, floor_w, gain), alphabet
    wide = np.zeros((301, 5), dtype=np.uint64)                                              # a table of 300 codes: rows are still indexed by code
    wide[:128] = by
    members = synth.alphabet_members("upper")
    assert weights(wide, members, 2048, 2048, n_codes=300) == synth.text_weights(by, members, 2048, 2048)


def test_text_weights_from_char_errors_on_the_device():
    """afr_op_sheet_char_errors fills a by-code table and afr_op_text_weights reads it where it lies; the texts drawn from the result are
    the twin's."""
    from ai_font_renderer_amd import devdata
    atlas = devdata.GlyphAtlas.from_font(None).to("cuda")
    alphabet = "alnum"
    ds = devdata.reference_dataset(64, atlas, alphabet=alphabet)
    codes, sheets = ds.tensors
    pred = sheets.roll(-1, 0).contiguous()                                                  # every sheet measured against its neighbour's
    table = devdata.char_errors(atlas, codes, pred).by_code
    members = synth.alphabet_members(alphabet)
    cum, w = weights(None, members, 1024, 3072, by_dev=table)
    by = table.cpu().numpy().astype(np.uint64)
    want_cum, want_w = synth.text_weights(by, members, 1024, 3072)
    assert (cum, w) == (want_cum, want_w) and len(set(w)) > 20 and int(by[:127, 2].sum()) > 0
    dcum, dw = devdata.text_weights(alphabet, table, 1024, 3072)
    assert dcum.dtype == torch.int32 and dcum.is_cuda and dcum.tolist() == want_cum and dw.tolist() == want_w
    got, lens = devdata.generate_codes(200, 1000, device="cuda", cum=dcum)
    strings = twin_texts(range(1000, 1200), want_cum)
    assert np.array_equal(got.cpu().numpy(), synth.encode_strings(strings, 100)) and lens.tolist() == [len(s) for s in strings]


def test_refusals_launch_nothing():
    """What the two entries refuse (the cases of tests/test_text_cpu.py, here with real buffers): the error comes back and the outputs keep
    their fill."""
    lib, EI = _lib.lib(), _lib.AFR_EINVAL
    whole, own = guarded_bytes(94 * 4 + 800 + 8)
    cum, codes = C.c_void_p(own.data_ptr()), C.c_void_p(own.data_ptr() + 376)
    table = dev(np.ascontiguousarray(TC.steer_table()).view(np.int64))
    up = (C.c_uint32 * 3)(*synth.members_words(UPPER))
    calls = [
        lambda: lib.afr_op_dataset_text_w(42, None, None, 1, 10, 100, None, codes, 100, None, None, stream()),
        lambda: lib.afr_op_dataset_text_w(42, None, None, 1, 10, 100, C.c_void_p(cum.value + 2), codes, 100, None, None, stream()),
        lambda: lib.afr_op_dataset_text_w(42, None, None, 1, 10, 101, cum, codes, 100, None, None, stream()),
        lambda: lib.afr_op_dataset_text_w(42, None, None, 0, 10, 100, cum, codes, 100, None, None, stream()),
        lambda: lib.afr_op_text_weights(ptr(table), 126, up, 4096, 0, cum, None, stream()),
        lambda: lib.afr_op_text_weights(ptr(table), 127, (C.c_uint32 * 3)(0, 0, 0), 4096, 0, cum, None, stream()),
        lambda: lib.afr_op_text_weights(ptr(table), 127, (C.c_uint32 * 3)(0, 0, 1 << 30), 4096, 0, cum, None, stream()),
        lambda: lib.afr_op_text_weights(ptr(table), 127, up, 0, 0, cum, None, stream()),
        lambda: lib.afr_op_text_weights(ptr(table), 127, up, 65536, 0, cum, None, stream()),
        lambda: lib.afr_op_text_weights(ptr(table), 127, up, 4096, 65536, cum, None, stream()),
        lambda: lib.afr_op_text_weights(C.c_void_p(table.data_ptr() + 4), 127, up, 4096, 0, cum, None, stream()),
        lambda: lib.afr_op_text_weights(ptr(table), 127, up, 4096, 0, C.c_void_p(cum.value + 2), None, stream()),
        lambda: lib.afr_op_text_weights(ptr(table), 127, up, 4096, 0, cum, C.c_void_p(cum.value + 1), stream()),
        lambda: lib.afr_op_text_weights(ptr(table), 127, up, 4096, 0, None, None, stream()),
    ]
    for i, call in enumerate(calls):
        assert call() == EI, i
    torch.cuda.synchronize()
    assert all(bands_kept(whole)) and bool((own == 0xFF).all())
    with pytest.raises(ValueError):
        from ai_font_renderer_amd import devdata
        devdata.generate_codes(4, device="cuda", cum=torch.zeros(94, dtype=torch.int32, device="cuda"))


# ---------------------------------------------------------------------------------------------- CLI
def _run_cli(M, monkeypatch, name, alphabet=None, fresh=False, steer=0.0, epochs=2):
    monkeypatch.setattr(M, "NUM_SAMPLES", 96)
    monkeypatch.setattr(M, "NUM_EPOCHS", epochs)
    monkeypatch.setattr(M, "OUTPUT_DIR", name)
    monkeypatch.setattr(M, "DEVICE_DATA", "default")
    monkeypatch.setattr(M, "FRESH_DATA", fresh)
    monkeypatch.setattr(M, "ALPHABET", alphabet)
    monkeypatch.setattr(M, "STEER", steer)
    torch.manual_seed(42)


def test_cli_alphabet_upper_is_the_run_without_it(tmp_path, monkeypatch, capsys):
    """AFR_ALPHABET=upper with fresh data, two epochs: the same font_renderer.pth and the same lines as the run without the variable -- the
    data set and the rewrite come from the weighted source -- and one more line of config.txt."""
    from ai_font_renderer_amd import model as M
    monkeypatch.chdir(tmp_path)
    out, pth = {}, {}
    for name, alphabet in (("out_plain", None), ("out_upper", "upper")):
        _run_cli(M, monkeypatch, name, alphabet, fresh=True)
        M.main(["model.py", "--train"])
        out[name] = [l.replace(name, "DIR") for l in capsys.readouterr().out.splitlines()]
        pth[name] = torch.load(tmp_path / "font_renderer.pth", weights_only=True)
    assert out["out_plain"] == out["out_upper"] and any(l.startswith("Epoch 0,") for l in out["out_plain"])
    assert list(pth["out_plain"]) == list(pth["out_upper"])
    for key in pth["out_plain"]:
        assert torch.equal(pth["out_plain"][key].view(torch.int32), pth["out_upper"][key].view(torch.int32)), key
    cfg = [(tmp_path / d / "config.txt").read_text().splitlines() for d in ("out_plain", "out_upper")]
    assert cfg[1] == cfg[0] + ["alphabet = upper"]
    assert not (tmp_path / "out_upper" / "string_15.bmp").exists() and (tmp_path / "out_upper" / "string_14.bmp").exists()


def test_cli_alphabet_alnum_trains_and_renders_lower_case(tmp_path, monkeypatch, capsys):
    from ai_font_renderer_amd import model as M
    monkeypatch.chdir(tmp_path)
    _run_cli(M, monkeypatch, "out_alnum", "alnum", epochs=1)
    M.main(["model.py", "--train"])
    lines = capsys.readouterr().out.splitlines()
    assert any(l.startswith("Epoch 0, Train Loss: ") for l in lines) and "Saved 17 rendered strings to out_alnum/" in lines
    assert (tmp_path / "out_alnum" / "config.txt").read_text().splitlines()[-2:] == ["device_data = default", "alphabet = alnum"]
    assert M._extra_test_strings("alnum") == ["the quick brown fox jumps over the lazy dog", "0123456789"]
    for d in ("out_alnum", "out_alnum/epoch_0"):
        assert (tmp_path / d / "string_16.bmp").exists() and not (tmp_path / d / "string_17.bmp").exists()
    # the data set it trained on: the twin's texts over the 62 characters
    from ai_font_renderer_amd import devdata
    atlas = devdata.GlyphAtlas.from_font(None).to("cuda")
    x = devdata.reference_dataset(96, atlas, alphabet="alnum").tensors[0].cpu().numpy()
    cum, _ = synth.text_weights(None, synth.alphabet_members("alnum"), 4096, 0)
    assert np.array_equal(x, synth.encode_strings([synth.lcg_text_weighted(42 + i, cum) for i in range(96)], x.shape[1]))
    assert set(np.unique(x).tolist()) - {0, 32} == set(map(ord, "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"))


def test_cli_steer_in_miniature(tmp_path, monkeypatch, capsys):
    """AFR_STEER under fresh data, six epochs of 96 sheets.  Share 0: the rewritten rows are lcg_text's, as without it, and no line is
    added.  Share 0.5: epoch 0 is the same; the training rows after the last rewrite are the twin's texts for the weights the twin builds
    from the table the validation pass before it left; the validation rows never change; the status line names the heaviest codes."""
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
        _run_cli(M, monkeypatch, name, None, fresh=True, steer=share, epochs=E)
        model = M.train_string_renderer()
        lines[name] = [l.replace(name, "DIR") for l in capsys.readouterr().out.splitlines()]
        x, _, t = model.engine._ds[:3]
        rows[name] = (x.cpu(), t.view(N, 80, 240).cpu())
        assert torch.equal(rows[name][0][va], first.tensors[0][va].cpu()) and torch.equal(rows[name][1][va], first.tensors[1][va].cpu())
    L = first.tensors[0].shape[1]
    zero, half = made
    assert zero.w is None and not any(l.startswith("Steer:") for l in lines["out_zero"])
    assert torch.equal(rows["out_zero"][0][tr], torch.from_numpy(synth.encode_strings([synth.lcg_text(42 + (E - 1) * N + int(r), 10, L) for r in tr], L)))
    assert "steer" not in (tmp_path / "out_zero" / "config.txt").read_text()
    assert (tmp_path / "out_half" / "config.txt").read_text().splitlines()[-2:] == ["fresh_data = 1", "steer = 0.5"]
    e0 = [[l for l in lines[k] if l.startswith("Epoch 0,")] for k in ("out_zero", "out_half")]
    assert len(e0[0]) == 1 and e0[0] == e0[1]
    # the last rewrite, before epoch 5: the table of epoch 4's validation pass -> weights -> texts
    table = half.by_code.cpu().numpy().astype(np.uint64)
    assert int(table[-1, 0]) == len(va) == 19 and int(table[65:91, 2].sum()) > 0
    cum, w = synth.text_weights(table, UPPER, 2048, 2048)
    assert half.w.tolist() == w and len(set(w)) > 10
    strings = [synth.lcg_text_weighted(42 + (E - 1) * N + int(r), cum, 10, L) for r in tr]
    want_x = torch.from_numpy(synth.encode_strings(strings, L))
    assert torch.equal(rows["out_half"][0][tr], want_x) and not torch.equal(want_x, rows["out_zero"][0][tr])
    assert torch.equal(rows["out_half"][1][tr], devdata.compose_sheets(atlas, want_x).cpu())
    steer = [l for l in lines["out_half"] if l.startswith("Steer:")]
    top = sorted((i for i in range(94) if w[i]), key=lambda i: (-w[i], i))[:5]
    assert len(steer) == 1 and steer[0].startswith("Steer: share 0.5, heaviest 5 codes " + f"{33 + top[0]} {chr(33 + top[0])!r} x{w[top[0]] / 4096:.2f}")
    assert lines["out_half"][lines["out_half"].index(steer[0]) - 1].startswith("Epoch 5,")
