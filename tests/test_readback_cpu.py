"""CPU: the numpy twin of afr_op_sheet_read_back (tests/readback_ref.py) against the facts counted when the definition was chosen, the
confusion table against the histogram of (true code, code read), each planted fault against the inputs tests/test_gpu_readback.py uses,
AFR_READ_REPORT's parsing, and every argument refusal of the entry (nothing launched)."""
import ctypes as C

import numpy as np
import pytest

from . import charerr_ref as E
from . import compose_ref as R
from . import readback_ref as B
from .util import load, synth

# (scored characters, read right) of the fixture texts with the target, hashed noise and the next text's sheet; on the miniature sheets
# (scored, read right from the target, read blank from a white sheet).  Candidates: every code 33..126.
FULL = {"fira": (960, 960, 35, 58), "mont": (913, 913, 6, 36)}
MINI = {"fira": (205, 205, 139), "mont": (185, 185, 118)}


def _atlas(fx, key):
    return {k: fx[f"{key}/{k}"] for k in ("cells", "adv64", "kern64", "origin_x", "origin_y")}


@pytest.fixture(scope="module")
def fx():
    return dict(load("atlas_sheets.npz"))


def _histogram(codes, read, n_codes):
    """confusion from read alone: a scored position holds a code read, never 0"""
    want = np.zeros((n_codes, n_codes), dtype=np.uint64)
    np.add.at(want, (codes[read > 0], read[read > 0].astype(np.int64)), np.uint64(1))
    return want


@pytest.mark.parametrize("key", ["fira", "mont"])
def test_fixture_texts_are_read_as_counted(fx, key):
    A, codes, sheets = _atlas(fx, key), fx[f"{key}/codes"], fx[f"{key}/sheets"]
    geo = R.geometry(int(A["origin_y"]))
    cells = A["cells"].reshape(len(A["cells"]), -1)
    assert len(np.unique(cells[33:127], axis=0)) == 94                             # no two cells are identical
    wins = [B.windows(A, geo, row) for row in codes]
    scored, right, noise_right, next_right = FULL[key]
    for name, pred in E.predictions(sheets, synth).items():
        read, score, confusion, bad = B.read_back_batch(A, geo, codes, pred, B.ALL, wins=wins)
        assert not bad.any()
        assert np.array_equal(confusion, _histogram(codes, read, len(cells))), name
        assert B.rate(confusion)[:2] == (scored, {"target": right, "noise": noise_right, "next": next_right}[name]), name
        assert (score[..., 0] <= score[..., 1]).all()
        if name == "target":
            assert not score[..., 1].any() and np.array_equal(read > 0, (codes > 32) & (read > 0)) and B.rate(confusion)[2] == 0
            assert np.array_equal(read[read > 0], codes[read > 0])
        else:
            assert score[..., 0].any()


@pytest.mark.parametrize("key", ["fira", "mont"])
def test_miniature_sheets_are_read_as_counted(fx, key):
    """windows clipped at all four edges; on a white sheet the blank wins unless the window holds no ink of any candidate's that tells
    them apart -- there the hypotheses tie and the true code keeps the tie, which the "tie_small" fault gives to the blank"""
    A = _atlas(fx, key)
    geo, codes = E.mini_case(A, synth)
    preds = B.mini_predictions(R.compose_batch(A, geo, codes)[0], synth)
    scored, right, blank = MINI[key]
    read, score, confusion, _ = B.read_back_batch(A, geo, codes, preds["target"], B.ALL)
    assert B.rate(confusion) == (scored, right, 0)
    # lines 6 pixels apart under cells 14 high: the true glyph goes on last where compose folded it in between, and the fold's rounding
    # depends on the order, so the true code's score is small here, not 0 as it is at the default geometry
    assert score[..., 1].any() and int(score[..., 1].max()) < 64
    read, score, confusion, _ = B.read_back_batch(A, geo, codes, preds["white"], B.ALL)
    assert B.rate(confusion) == (scored, scored - blank, blank)
    assert np.array_equal(confusion, _histogram(codes, read, len(A["cells"])))
    small = B.read_back_batch(A, geo, codes, preds["white"], B.ALL, "tie_small")[2]
    assert B.rate(small) == (scored, 0, scored)


def test_planted_substitutions_are_read_as_the_substitute(fx):
    """Fira Code has one advance and no kerning, so a substituted character moves nothing: the sheet composed from the changed text,
    read back against the original text, shows the substitute where it stands on a drawn line and every other character as itself."""
    A, codes = _atlas(fx, "fira"), fx["fira/codes"]
    assert len(set(A["adv64"][32:127].tolist())) == 1 and not A["kern64"].any()
    geo = R.geometry(int(A["origin_y"]))
    changed, subs = B.substitutions(codes)
    sheets = R.compose_batch(A, geo, changed)[0]
    read, _, confusion, _ = B.read_back_batch(A, geo, codes, sheets, B.ALL)
    landed = [(j, pos, sub) for j, pos, sub in subs if read[j, pos]]
    print(f"{len(landed)} of {len(subs)} substitutions stand on a drawn line")
    assert len(landed) >= 12
    want = np.where(read > 0, codes, 0)
    for j, pos, sub in landed:
        want[j, pos] = sub
    assert np.array_equal(read, want)
    assert B.rate(confusion)[1] == FULL["fira"][0] - len(landed)


def test_each_planted_fault_changes_an_output_of_the_gpu_inputs(fx):
    """"tie_small" needs tied scores -- the white miniature sheets; "no_ctx" and "ctx_self" show wherever cells overlap or hold ink;
    "packed_pos" needs a dropped code in front of a scored character: the dirty rows."""
    for key in ("fira", "mont"):
        A, codes = _atlas(fx, key), fx[f"{key}/codes"]
        geo = R.geometry(int(A["origin_y"]))
        preds = E.predictions(fx[f"{key}/sheets"], synth)
        good = B.read_back_batch(A, geo, codes, preds["target"], B.ALL)
        for fault in ("no_ctx", "ctx_self"):
            bad = B.read_back_batch(A, geo, codes, preds["target"], B.ALL, fault)
            assert not np.array_equal(bad[1], good[1]), (key, fault)
        mgeo, mcodes = E.mini_case(A, synth)
        mpreds = B.mini_predictions(R.compose_batch(A, mgeo, mcodes)[0], synth)
        for members in (B.ALL, synth.alphabet_members("upper")):
            good = B.read_back_batch(A, mgeo, mcodes, mpreds["white"], members)
            bad = B.read_back_batch(A, mgeo, mcodes, mpreds["white"], members, "tie_small")
            assert not np.array_equal(bad[0], good[0]) and not np.array_equal(bad[2], good[2]), key
        for fault in ("no_ctx", "ctx_self"):
            assert not np.array_equal(B.read_back_batch(A, mgeo, mcodes, mpreds["noise"], B.ALL, fault)[1],
                                      B.read_back_batch(A, mgeo, mcodes, mpreds["noise"], B.ALL)[1]), (key, fault)
        dirty = E.dirty_rows(synth)
        dnoise = synth.hash_u8(7312, (len(dirty), geo.height, geo.width))
        good = B.read_back_batch(A, geo, dirty, dnoise, B.ALL)
        assert good[3].tolist() == [True, True, False, True]
        bad = B.read_back_batch(A, geo, dirty, dnoise, B.ALL, "packed_pos")
        assert not np.array_equal(bad[0], good[0]) and not np.array_equal(bad[1], good[1]) and np.array_equal(bad[2], good[2])
        assert good[0][0, 3] == 0 and good[0][0, 4] > 0 and good[0][3, 3] > 0 and good[0][3, 2] == 0


def test_a_true_code_outside_the_members_is_still_a_candidate(fx):
    """'y' and '.' of " Ty." with A-Z as the members: read from the target they are themselves, score 0"""
    A = _atlas(fx, "mont")
    geo, codes = E.mini_case(A, synth)
    j = E.MINI_TEXTS.index(" Ty.")
    sheet = R.compose(A, geo, codes[j])[0]
    read, score, confusion, _ = B.read_back(A, geo, codes[j], sheet, synth.alphabet_members("upper"))
    assert "".join(chr(c) for c in read[:4]) == "\0Ty." and not score[:, 1].any() and confusion[ord("y"), ord("y")] == 1
    assert B.candidates(synth.alphabet_members("upper"), ord("y")) == [32, *range(65, 91), ord("y")]


def test_read_report_is_parsed_strictly(monkeypatch):
    from ai_font_renderer_amd import model as M
    monkeypatch.delenv("AFR_READ_REPORT", raising=False)
    monkeypatch.delenv("AFR_DEVICE_DATA", raising=False)
    assert M._read_report_from_env() is None
    monkeypatch.setenv("AFR_READ_REPORT", "")
    assert M._read_report_from_env() is None
    monkeypatch.setenv("AFR_DEVICE_DATA", "default")
    for bad in ("0", "x", "-2", "1.5"):
        monkeypatch.setenv("AFR_READ_REPORT", bad)
        with pytest.raises(ValueError, match="AFR_READ_REPORT"):
            M._read_report_from_env()
    monkeypatch.setenv("AFR_READ_REPORT", "5")
    assert M._read_report_from_env() == 5
    monkeypatch.delenv("AFR_DEVICE_DATA")
    with pytest.raises(ValueError, match="AFR_DEVICE_DATA"):
        M._read_report_from_env()


def test_read_report_line_and_table():
    """the printed line and confusion.tsv from a table, without a device"""
    import torch
    from types import SimpleNamespace
    from ai_font_renderer_amd import model as M
    rep = M._ReadReport(2, SimpleNamespace(n_codes=127, device="cpu"), None, None)
    for c, r, v in ((81, 81, 5), (81, 79, 312), (79, 48, 7), (73, 32, 7), (65, 65, 669)):
        rep.table[c, r] = v
    assert rep.line() == "Read report: 1000 characters, read right 0.674000, read blank 0.007000, confusions: Q->O 312, I->blank 7"
    assert M._ReadReport(2, SimpleNamespace(n_codes=127, device="cpu"), None, "ascii").line().endswith("confusions: none")


def check_refusals():
    """every refusal of afr_op_sheet_read_back, with pointers nothing is read from: nothing is launched"""
    from ai_font_renderer_amd import _lib
    lib = _lib.lib()
    EI, EU = _lib.AFR_EINVAL, _lib.AFR_EUNSUPPORTED
    fk = C.c_void_p(0x1000)
    all_members = (C.c_uint32 * 3)(0xFFFFFFFF, 0xFFFFFFFF, 0x3FFFFFFF)

    def call(cells=fk, adv=fk, kern=None, n_codes=127, ch=14, cw=8, ox=0, oy=11, H=80, W=240, wrap=15360, nl=6, codes=fk, ldx=100, rows=None,
             n=4, pred=fk, members=all_members, read=fk, score=fk, confusion=fk, err=None, atlas=True, geo=True):
        a = _lib.AfrGlyphAtlas(cells, adv, kern, n_codes, ch, cw, ox, oy)
        g = _lib.AfrSheetGeometry(H, W, wrap, nl)
        return lib.afr_op_sheet_read_back(C.byref(a) if atlas else None, C.byref(g) if geo else None, codes, ldx, rows, n, pred, members, read,
                                          score, confusion, err, None)

    def said(*words):
        msg = lib.afr_last_error()
        return msg.startswith(b"afr_op_sheet_read_back") and all(w in msg for w in words)

    # what compose and char_errors refuse
    for kw in (dict(atlas=False), dict(geo=False), dict(codes=None), dict(pred=None), dict(cells=None), dict(adv=None)):
        assert call(**kw) == EI and said(b"null"), kw
    assert call(n=0) == EI and said(b"n = 0")
    assert call(nl=0) == EI and call(nl=17) == EI and said(b"n_lines")
    for kw in (dict(n_codes=0), dict(ch=0), dict(cw=-1), dict(H=0), dict(W=0), dict(ldx=0), dict(wrap=-1)):
        assert call(**kw) == EI and said(b"positive"), kw
    for kw in (dict(ox=-1), dict(ox=8), dict(oy=-1), dict(oy=14)):
        assert call(**kw) == EI and said(b"origin"), kw
    for kw in (dict(pred=C.c_void_p(0x1004)), dict(cells=C.c_void_p(0x1002)), dict(codes=C.c_void_p(0x1004)), dict(rows=C.c_void_p(0x1004)),
               dict(err=C.c_void_p(0x1002)), dict(kern=C.c_void_p(0x1001)), dict(adv=C.c_void_p(0x1002))):
        assert call(**kw) == EI and said(b"aligned"), kw
    assert call(ldx=257) == EU and said(b"256")
    assert call(W=244) == EU and said(b"multiple of 8")
    assert call(ch=64, cw=16, oy=11) == EU and said(b"LDS")                        # 127 * 64 * 16 = 130048 bytes of cells
    # its own
    assert call(members=None) == EI and said(b"members is null")
    assert call(members=(C.c_uint32 * 3)(0, 0, 0x40000000)) == EI and said(b"bit 93")
    assert call(n_codes=126) == EI and said(b"126")
    assert call(n_codes=257, ch=2, cw=2, oy=1) == EU and said(b"byte")
    assert call(read=None, score=None, confusion=None) == EI and said(b"all NULL")
    assert call(confusion=C.c_void_p(0x1004)) == EI and said(b"8-byte")
    assert call(score=C.c_void_p(0x1004)) == EI and said(b"8-byte")
    assert call(read=C.c_void_p(0x1001), score=None, confusion=None, members=None) == EI      # read may lie anywhere: members is what is refused
    # 65025 * pixels must fit 32 bits: a cell of 66051 pixels at the most (such a cell passes the LDS budget as well: asked first)
    assert 65025 * 66051 < 2 ** 32 <= 65025 * 66052
    assert call(ch=8257, cw=8, oy=11) == EU and said(b"66051")
    assert call(ch=8256, cw=8, oy=11) == EU and said(b"LDS")
    # the LDS budget with this kernel's arrays counted: 127 cells of 20 x 15 with their ranges and the layout are 38100 + 720 + 5380
    # bytes, which compose and char_errors take; the records (5128), four windows (2400) and the confusion counters (18048) pass 64 KiB
    assert call(ch=20, cw=15, oy=11) == EU and said(b"LDS", b"confusion")
    g = _lib.AfrSheetGeometry(80, 240, 15360, 6)
    a = _lib.AfrGlyphAtlas(fk, fk, None, 127, 20, 15, 0, 11)
    assert lib.afr_op_sheet_char_errors(C.byref(a), C.byref(g), fk, 100, None, 4, fk, None, None, None, None) == EI      # its own refusal, not the budget's


def test_the_entry_refuses_bad_arguments_before_any_launch():
    check_refusals()
