"""GPU: afr_op_sheet_read_back (csrc/dataset.hip) against its numpy twin (tests/readback_ref.py), devdata.read_back on a composed batch,
and AFR_READ_REPORT in miniature.  Everything is integers: every comparison is exact.  The op tests launch into guarded buffers
(tests/op_harness.py), twice, and compare the two launches bit for bit; read and score start as the harness's fill, of which nothing
may be left, confusion as zeros (or as what it is to be added to)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from ai_font_renderer_amd import _lib
from . import charerr_ref as E
from . import compose_ref as R
from . import readback_ref as B
from .gpu_util import dev, ptr, stream
from .op_harness import Outs, twice
from .test_gpu_compose import DevAtlas, _atlas, _geo_struct
from .test_readback_cpu import check_refusals
from .util import load, synth

pytestmark = pytest.mark.gpu
UPPER = synth.alphabet_members("upper")


@pytest.fixture(scope="module")
def fx():
    return dict(load("atlas_sheets.npz"))


def u64(t):
    """the int32 words the harness hands back, as the unsigned counters they are"""
    return t.numpy().view(np.uint32).astype(np.uint64)


def launch(A, geo, codes, pred, members=B.ALL, rows=None, atlas=None, conf_init=None, read=True, score=True, confusion=True):
    """afr_op_sheet_read_back twice into guarded buffers -> (uint8 [n][ldx] or None, uint64 [n][ldx][2] or None, uint64 [n_codes][n_codes]
    or None, err word).  Sample j reads row rows[j] (default j) of codes and sheet j of pred; conf_init: what confusion holds before the
    launch (default zeros)."""
    atlas = atlas or DevAtlas(A)
    codes = np.ascontiguousarray(codes, dtype=np.int64)
    ldx, n, n_codes = codes.shape[1], len(pred), A["cells"].shape[0]
    assert pred.dtype == np.uint8 and pred.shape[1:] == (geo.height, geo.width)
    cd, pd, rd, g = dev(codes), dev(pred), None if rows is None else dev(np.asarray(rows, dtype=np.int64)), _geo_struct(geo)
    words = (C.c_uint32 * 3)(*synth.members_words(members))
    init = np.zeros((n_codes, n_codes), dtype=np.uint64) if conf_init is None else conf_init
    init = torch.from_numpy(np.ascontiguousarray(init).view(np.int32))

    def once():
        o = Outs()
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        rp = o.new("read", (n, ldx), torch.uint8) if read else None
        sp = o.new("score", (n, ldx, 2), torch.int32) if score else None
        cp = o.new("confusion", (n_codes, 2 * n_codes), torch.int32, init=init) if confusion else None
        _lib.check(_lib.lib().afr_op_sheet_read_back(C.byref(atlas.struct), C.byref(g), ptr(cd), ldx, ptr(rd), n, ptr(pd), words, rp, sp, cp,
                                                     ptr(err), stream()))
        return dict(o.finish(), err=int(err.cpu()))

    res = twice(once)
    got_read = got_conf = None
    if read:
        got_read = res["read"].numpy()
        assert (got_read != 0xFF).all()                                    # the harness's uint8 fill is no code of the atlas
    if confusion:
        w = u64(res["confusion"]).reshape(n_codes, n_codes, 2)
        got_conf = w[:, :, 0] | w[:, :, 1] << np.uint64(32)
    return got_read, u64(res["score"]) if score else None, got_conf, res["err"]


def check(got, want, what=None):
    """(read, score, confusion) of a launch against the twin's (read, score, confusion per batch)"""
    for name, g, w in zip(("read", "score", "confusion"), got, want):
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5])


@functools.lru_cache(maxsize=None)
def _reference(key):
    """the twin on every fixture text of one atlas with charerr_ref's three predictions, computed once: name -> (read [24][208], score
    [24][208][2], confusion per sheet [24][127][127]); and the predictions"""
    fx = dict(load("atlas_sheets.npz"))
    A, codes, sheets = _atlas(fx, key), fx[f"{key}/codes"], fx[f"{key}/sheets"]
    geo = R.geometry(int(A["origin_y"]))
    preds = E.predictions(sheets, synth)
    wins = [B.windows(A, geo, row) for row in codes]
    ref = {}
    for name, pred in preds.items():
        res = [B.read_back(A, geo, row, pred[j], B.ALL, win=wins[j]) for j, row in enumerate(codes)]
        assert not any(r[3] for r in res)
        ref[name] = tuple(np.stack([r[k] for r in res]) for k in range(3))
    return ref, preds


@pytest.mark.parametrize("key", ["fira", "mont"])
def test_fixture_texts_three_predictions(fx, key):
    """Every fixture text (rows of 208 codes), in one batch and one launch per text, read back from the target itself (every character
    read right, the true code's score 0), hashed noise, and the next text's sheet."""
    A, codes = _atlas(fx, key), fx[f"{key}/codes"]
    geo, atlas = R.geometry(int(A["origin_y"])), DevAtlas(A)
    ref, preds = _reference(key)
    assert codes.shape[1] == 208
    for name, pred in preds.items():
        want_read, want_score, want_conf = ref[name]
        read, score, conf, err = launch(A, geo, codes, pred, atlas=atlas)
        assert err == 0
        check((read, score, conf), (want_read, want_score, want_conf.sum(0)), name)
        scored, right, blank = B.rate(conf)
        print(f"{key} {name}: {scored} scored, {right} read right, {blank} read blank")
        if name == "target":
            assert right == scored > 900 and not score[..., 1].any() and np.array_equal(read[read > 0], codes[read > 0])
        else:
            assert right < scored // 10 and score[..., 0].any()
        for j in range(len(codes)):                                        # one launch per text
            got = launch(A, geo, codes[j:j + 1], pred[j:j + 1], atlas=atlas)
            assert got[3] == 0
            check((got[0][0], got[1][0], got[2]), (want_read[j], want_score[j], want_conf[j]), (name, j))


@pytest.mark.parametrize("key", ["fira", "mont"])
def test_miniature_sheets(fx, key):
    """8 x 24 sheets, lines 6 pixels apart: windows cut by all four edges and contexts of several lines; read back from the target, a
    white sheet (tied scores: the true code keeps them, which the twin's "tie_small" fault does not) and noise, with every code as a
    candidate and with A-Z alone ('y' and '.' of " Ty." are then candidates only because they are the true codes)."""
    A = _atlas(fx, key)
    geo, codes = E.mini_case(A, synth)
    atlas = DevAtlas(A)
    preds = B.mini_predictions(R.compose_batch(A, geo, codes)[0], synth)
    wins = [B.windows(A, geo, row) for row in codes]
    for members in (B.ALL, UPPER):
        for name, pred in preds.items():
            want = B.read_back_batch(A, geo, codes, pred, members, wins=wins)
            read, score, conf, err = launch(A, geo, codes, pred, members, atlas=atlas)
            assert err == 0
            check((read, score, conf), want[:3], (name, len(members)))
            if name == "white":
                small = B.read_back_batch(A, geo, codes, pred, members, "tie_small", wins=wins)
                assert not np.array_equal(read, small[0]) and B.rate(conf)[1] > 0
    j = E.MINI_TEXTS.index(" Ty.")
    assert read[j, 2] > 0 and read[j, 3] > 0 and score[j, 2, 1] > 0


def test_bad_codes_are_flagged_and_outputs_stay_at_their_positions(fx):
    A = _atlas(fx, "mont")
    geo = R.geometry(int(A["origin_y"]))
    dirty = E.dirty_rows(synth)
    pred = synth.hash_u8(7312, (len(dirty), geo.height, geo.width))
    want = B.read_back_batch(A, geo, dirty, pred, B.ALL)
    assert want[3].any()
    read, score, conf, err = launch(A, geo, dirty, pred)
    assert err & 1
    check((read, score, conf), want[:3])
    packed = B.read_back_batch(A, geo, dirty, pred, B.ALL, "packed_pos")
    assert not np.array_equal(read, packed[0]) and not np.array_equal(score, packed[1])
    assert read[0, 3] == 0 and read[0, 4] > 0 and read[3, 3] > 0 and read[3, 2] == 0
    read, _, _, err = launch(A, geo, dirty[2:3], pred[2:3], score=False, confusion=False)      # the clean row alone raises no flag
    assert err == 0 and np.array_equal(read[0], want[0][2])


@pytest.mark.parametrize("ldx", [100, 104])
def test_code_rows_permuted_and_gapped(fx, ldx):
    """The 23 texts that fit 100 codes lie in every other row of a wider buffer, in a shuffled order; the predictions are dense."""
    A, all_codes = _atlas(fx, "mont"), fx["mont/codes"]
    geo = R.geometry(int(A["origin_y"]))
    ref, preds = _reference("mont")
    fit = np.nonzero((all_codes[:, 100:] == 0).all(1))[0]
    assert len(fit) == 23
    rows = 2 * ((np.arange(len(fit)) * 7 + 3) % len(fit)) + 1
    assert len(set(rows.tolist())) == len(fit)
    buf = np.full((2 * len(fit) + 2, ldx), ord("W"), dtype=np.int64)        # the rows in between would read something else
    buf[rows] = all_codes[fit, :ldx]
    pred = np.ascontiguousarray(preds["noise"][fit])
    read, score, conf, err = launch(A, geo, buf, pred, rows=rows)
    want_read, want_score, want_conf = ref["noise"]
    assert err == 0
    check((read[:, :100], score[:, :100], conf), (want_read[fit, :100], want_score[fit, :100], want_conf[fit].sum(0)))
    assert not read[:, 100:].any() and not score[:, 100:].any()


def test_more_sheets_than_workgroups_accumulation_and_each_output_alone(fx):
    """2048 + 61 sheets: the grid is capped at 2048 workgroups, so 61 of them read a second sheet from the same LDS and count it into
    the same table.  Then 300 of them again, added onto the table the first launch left; and each output alone, the others NULL."""
    A, codes = _atlas(fx, "mont"), fx["mont/codes"]
    geo, atlas = R.geometry(int(A["origin_y"])), DevAtlas(A)
    ref, preds = _reference("mont")
    names = list(preds)
    i = np.arange(2048 + 61)
    pick, which = (i * 7) % len(codes), i % 3
    pred = np.stack([preds[names[w]][p] for p, w in zip(pick, which)])
    want = [np.stack([ref[names[w]][k][p] for p, w in zip(pick, which)]) for k in range(2)]
    want_conf = sum(ref[names[w]][2][p] for p, w in zip(pick, which))
    read, score, conf, err = launch(A, geo, codes[pick], pred, atlas=atlas)
    assert err == 0
    check((read, score, conf), (want[0], want[1], want_conf))
    first = sum(ref[names[w]][2][p] for p, w in zip(pick[:300], which[:300]))
    read2, score2, conf2, _ = launch(A, geo, codes[pick[:300]], pred[:300], atlas=atlas, conf_init=conf)
    check((read2, score2, conf2), (want[0][:300], want[1][:300], want_conf + first))
    only = launch(A, geo, codes[pick[:300]], pred[:300], atlas=atlas, score=False, confusion=False)
    assert only[1] is None and only[2] is None and np.array_equal(only[0], want[0][:300])
    only = launch(A, geo, codes[pick[:300]], pred[:300], atlas=atlas, read=False, confusion=False)
    assert only[0] is None and only[2] is None and np.array_equal(only[1], want[1][:300])
    only = launch(A, geo, codes[pick[:300]], pred[:300], atlas=atlas, read=False, score=False)
    assert only[0] is None and only[1] is None and np.array_equal(only[2], first)


def test_a_workgroup_empties_its_16_bit_counters_before_they_can_overflow(fx):
    """The confusion counters in LDS are 16 bits wide and a sheet may add ldx to one, so with rows of 256 codes a workgroup adds its table
    to global memory before its 256th sheet.  2048 * 256 miniature sheets, read through code_rows from 25 rows of codes: every workgroup
    empties its table once on the way and once at the end, and the sum is 2048 * 256 / 25 times the 25 sheets', none lost, none twice."""
    A = _atlas(fx, "fira")
    geo, codes = E.mini_case(A, synth)
    wide = np.zeros((len(codes), 256), dtype=np.int64)
    wide[:, :codes.shape[1]] = codes
    sheets = B.mini_predictions(R.compose_batch(A, geo, codes)[0], synth)["noise"]
    per_sheet = [B.read_back(A, geo, row, sheets[j], B.ALL)[2] for j, row in enumerate(wide)]
    n = 2048 * 256
    rows = np.arange(n) % len(codes)
    times = np.bincount(rows, minlength=len(codes))
    want = sum(c * np.uint64(t) for c, t in zip(per_sheet, times))
    _, _, conf, err = launch(A, geo, wide, sheets[rows], rows=rows, read=False, score=False)
    assert err == 0 and np.array_equal(conf, want) and int(conf.sum()) > 2 ** 21


def test_the_entry_refuses_bad_arguments_before_any_launch():
    check_refusals()


# ---------------------------------------------------------------------------------------------- Python surface, CLI
def test_devdata_read_back_on_a_composed_batch():
    """96 sheets composed over the whole alphabet: read back from themselves every character is read right; read back from the sheets
    shifted by one text the outputs are the twin's; rows and an accumulating table; texts() and rate()."""
    from ai_font_renderer_amd import devdata
    atlas = devdata.GlyphAtlas.from_font(None).to("cuda")
    ds = devdata.reference_dataset(96, atlas, alphabet="ascii")
    x, t = ds.tensors
    got = devdata.read_back(atlas, x, t, "ascii")
    assert got.read.dtype == torch.uint8 and tuple(got.read.shape) == tuple(x.shape) and tuple(got.score.shape) == (*x.shape, 2)
    assert got.confusion.dtype == torch.int64 and tuple(got.confusion.shape) == (127, 127)
    scored, right, blank = got.rate()
    assert scored == right > 96 * 10 and blank == 0 and not bool(got.score[..., 1].any())
    texts = got.texts()
    assert texts == ["".join(chr(c) for c in row if c) for row in x.cpu().tolist()]      # texts of 100 characters at the most fit six lines
    assert sum(len(s.replace(" ", "")) for s in texts) == scored
    A, geo = atlas.arrays(), R.geometry(atlas.origin_y)
    shifted = torch.roll(t, -1, 0).contiguous()
    want = B.read_back_batch(A, geo, x.cpu().numpy(), shifted.cpu().numpy(), synth.alphabet_members("alnum"))
    assert not want[3].any()
    got = devdata.read_back(atlas, x, shifted, "alnum")
    assert np.array_equal(got.read.cpu().numpy(), want[0]) and np.array_equal(got.score.cpu().numpy().astype(np.uint64), want[1])
    assert np.array_equal(got.confusion.cpu().numpy().astype(np.uint64), want[2])
    assert got.rate() == B.rate(want[2]) and got.rate()[1] < got.rate()[0] // 4
    # rows and an accumulating table: the second half through rows, added to the first half's table
    half = devdata.read_back(atlas, x[:48], shifted[:48], "alnum")
    both = devdata.read_back(atlas, x, shifted[48:].contiguous(), "alnum", rows=torch.arange(48, 96), confusion=half.confusion)
    assert both.confusion is half.confusion and torch.equal(both.confusion, got.confusion) and torch.equal(both.read, got.read[48:])
    assert both.texts() == got.texts()[48:]
    bad_codes = x[:2].clone()
    bad_codes[1, 0] = 300
    with pytest.raises(IndexError):
        devdata.read_back(atlas, bad_codes, t[:2].contiguous())


def _run_cli(M, monkeypatch, name, read_report, epochs):
    monkeypatch.setattr(M, "NUM_SAMPLES", 96)
    monkeypatch.setattr(M, "NUM_EPOCHS", epochs)
    monkeypatch.setattr(M, "OUTPUT_DIR", name)
    monkeypatch.setattr(M, "DEVICE_DATA", "default")
    monkeypatch.setattr(M, "FRESH_DATA", False)
    monkeypatch.setattr(M, "CHAR_REPORT", None)
    monkeypatch.setattr(M, "READ_REPORT", read_report)
    torch.manual_seed(42)


def test_cli_read_report_in_miniature(tmp_path, monkeypatch, capsys):
    """`AFR_DEVICE_DATA=default AFR_READ_REPORT=3 python model.py --train` in miniature (96 sheets, two epochs): one line is printed after
    epoch 0's status line, epoch_0/confusion.tsv and epoch_0/read_back.txt are written, font_renderer.pth and every other line of the
    output are those of the run without the variable.  A one-epoch run with the report writes the same files, and its table is
    devdata.read_back's over the validation rows with the model it returns."""
    from ai_font_renderer_amd import devdata, model as M
    monkeypatch.chdir(tmp_path)
    out, pth = {}, {}
    for name, k in (("out_plain", None), ("out_read", 3)):
        _run_cli(M, monkeypatch, name, k, 2)
        M.main(["model.py", "--train"])
        out[name] = [l.replace(name, "DIR") for l in capsys.readouterr().out.splitlines()]
        pth[name] = torch.load(tmp_path / "font_renderer.pth", weights_only=True)
    assert list(pth["out_plain"]) == list(pth["out_read"])
    for key in pth["out_plain"]:
        assert torch.equal(pth["out_plain"][key].view(torch.int32), pth["out_read"][key].view(torch.int32)), key
    at = [i for i, l in enumerate(out["out_read"]) if l.startswith("Read report: ")]
    assert len(at) == 1 and out["out_read"][at[0] - 1].startswith("Epoch 0,")
    assert out["out_read"][:at[0]] + out["out_read"][at[0] + 1:] == out["out_plain"]
    for f in ("confusion.tsv", "read_back.txt"):
        assert not (tmp_path / "out_plain" / "epoch_0" / f).exists() and (tmp_path / "out_read" / "epoch_0" / f).exists()
    cfg = (tmp_path / "out_read" / "config.txt").read_text().splitlines()
    assert cfg[-2:] == ["device_data = default", "read_report = 3"] and "read_report" not in (tmp_path / "out_plain" / "config.txt").read_text()
    # one epoch: the same epoch-0 files, and the model that was read
    _run_cli(M, monkeypatch, "out_one", 3, 1)
    model = M.train_string_renderer()
    capsys.readouterr()
    for f in ("confusion.tsv", "read_back.txt"):
        assert (tmp_path / "out_one" / "epoch_0" / f).read_bytes() == (tmp_path / "out_read" / "epoch_0" / f).read_bytes()
    lines = (tmp_path / "out_one" / "epoch_0" / "confusion.tsv").read_text().split("\n")
    assert lines[0].split("\t") == ["code", "char", "read", "read_char", "count"] and lines[-1] == ""
    table = {(int(f[0]), int(f[2])): int(f[4]) for f in (l.split("\t") for l in lines[1:-1])}
    x = model.engine._ds[0]
    va = M._EpochOrder(96).val_idx.cuda()
    assert len(va) == 19
    atlas = devdata.GlyphAtlas.from_font(None).to("cuda")
    model.eval()
    want = model.read_back(atlas, x[va].contiguous())
    conf = want.confusion.cpu()
    assert table == {(c, r): int(conf[c, r]) for c, r in torch.nonzero(conf).tolist()} and len(table) > 0
    scored, right, blank = want.rate()
    line = out["out_read"][at[0]]
    assert line.startswith(f"Read report: {scored} characters, read right {right / scored:.6f}, read blank {blank / scored:.6f}, confusions: ")
    pairs = sorted(((v, c, r) for (c, r), v in table.items() if c != r), key=lambda e: (-e[0], e[1], e[2]))[:3]
    assert line.split("confusions: ")[1] == ", ".join(f"{chr(c)}->{'blank' if r == 32 else chr(r)} {v}" for v, c, r in pairs)
    # read_back.txt: every test string, what was read below it, a blank line
    txt = (tmp_path / "out_one" / "epoch_0" / "read_back.txt").read_text().split("\n")
    assert txt[0::3][:len(M.test_strings)] == [s[:100] for s in M.test_strings] and len(txt) == 3 * len(M.test_strings) + 1
    codes = torch.from_numpy(synth.encode_strings(M.test_strings, 100)).cuda()
    assert txt[1::3] == model.read_back(atlas, codes).texts()
