"""CPU: the numpy twin of afr_op_sheet_char_errors (tests/charerr_ref.py) against numpy's whole-sheet sums, each planted fault against
the inputs tests/test_gpu_charerr.py uses, AFR_CHAR_REPORT's parsing, and every argument refusal of the entry (nothing launched)."""
import ctypes as C

import numpy as np
import pytest

from . import charerr_ref as E
from . import compose_ref as R
from .util import load, synth


def _atlas(fx, key):
    return {k: fx[f"{key}/{k}"] for k in ("cells", "adv64", "kern64", "origin_x", "origin_y")}


@pytest.fixture(scope="module")
def fx():
    return dict(load("atlas_sheets.npz"))


@pytest.mark.parametrize("key", ["fira", "mont"])
def test_twin_sums_to_the_whole_sheet(fx, key):
    """On the 48 fixture texts (24 per atlas): the records' pixels add up to the sheet, their three error sums to numpy's over the whole
    sheet against compose_ref.compose, a pixel has an owner exactly where the composed sheet is below 255, and by_code is per_pos
    summed by code."""
    A, codes = _atlas(fx, key), fx[f"{key}/codes"]
    geo = R.geometry(int(A["origin_y"]))
    assert len(codes) == 24                                                        # 48 with the other atlas
    sheets = np.stack([R.compose(A, geo, row)[0] for row in codes])
    assert np.array_equal(sheets, fx[f"{key}/sheets"])
    preds = E.predictions(sheets, synth)
    for j, row in enumerate(codes):
        own = E.owners(A, geo, row)
        assert np.array_equal(255 - own[0], sheets[j].astype(np.int64)), j
        assert np.array_equal(own[1] >= 0, sheets[j] < 255), j                     # background == (m == 0)
        for name, pred in preds.items():
            per_pos, by_code, bad = E.char_errors(A, geo, row, pred[j], own=own)
            assert not bad
            t, p = sheets[j].astype(np.int64), pred[j].astype(np.int64)
            d = np.abs(p - t)
            want = [geo.height * geo.width, int((d * d).sum()), int((d >= 2).sum()), int(((p >= 128) != (t >= 128)).sum())]
            assert per_pos.sum(0).tolist() == want, (j, name)
            assert by_code[:, 1:].sum(0).tolist() == want and int(by_code[-1, 0]) == 1, (j, name)
            assert by_code[-1, 1:].tolist() == per_pos[-1].tolist()
            if name == "target":
                assert not per_pos[:, 1:].any()
            text = [int(c) for c in row]
            for c in set(text) - {0}:
                at = [i for i, v in enumerate(text) if v == c]
                assert by_code[c, 1:].tolist() == per_pos[at].sum(0).tolist(), (j, name, c)


def _records(A, geo, codes, preds, fault=None):
    return E.char_errors_batch(A, geo, codes, preds, fault)[0]


def test_each_planted_fault_changes_the_records_of_the_gpu_inputs(fx):
    """"last" needs contested pixels -- the full-size fixture texts have them; "tie_late" needs tied ones, which only the miniature sheets
    hold; "packed_pos" needs a dropped code in front of an inked character: the dirty rows; "bg_any_cell" shows everywhere.  That the
    inputs hold such pixels is asserted, not assumed."""
    for key in ("fira", "mont"):
        A, codes = _atlas(fx, key), fx[f"{key}/codes"]
        geo = R.geometry(int(A["origin_y"]))
        own = [E.owners(A, geo, row) for row in codes]
        contested, tied = sum(int((o[5] >= 2).sum()) for o in own), sum(int(o[6].sum()) for o in own)
        print(f"{key}: full size, {contested} contested pixels, {tied} tied")
        assert contested > 0
        noise = E.predictions(fx[f"{key}/sheets"], synth)["noise"]
        good = _records(A, geo, codes, noise)
        for fault in ("last", "bg_any_cell"):
            assert not np.array_equal(_records(A, geo, codes, noise, fault), good), (key, fault)
        # the miniature sheets: ties
        mgeo, mcodes = E.mini_case(A, synth)
        mown = [E.owners(A, mgeo, row) for row in mcodes]
        mcontested, mtied = sum(int((o[5] >= 2).sum()) for o in mown), sum(int(o[6].sum()) for o in mown)
        print(f"{key}: miniature, {mcontested} contested pixels, {mtied} tied")
        assert mcontested > 0 and mtied > 0
        mnoise = synth.hash_u8(7301, (len(mcodes), mgeo.height, mgeo.width))
        mgood = _records(A, mgeo, mcodes, mnoise)
        for fault in ("last", "tie_late", "bg_any_cell"):
            assert not np.array_equal(_records(A, mgeo, mcodes, mnoise, fault), mgood), (key, fault)
        # the dirty rows: packed and original positions part
        dirty = E.dirty_rows(synth)
        dnoise = synth.hash_u8(7302, (len(dirty), geo.height, geo.width))
        dgood, _, bad = E.char_errors_batch(A, geo, dirty, dnoise)
        assert bad.tolist() == [True, True, False, True]
        assert not np.array_equal(_records(A, geo, dirty, dnoise, "packed_pos"), dgood), key
        assert not dgood[0, 3].any() and dgood[0, 4, 0] > 0 and not dgood[1, 0].any() and dgood[3, 3, 0] > 0 and not dgood[3, 2].any()


def test_wrapped_lines_find_their_positions_again(fx):
    """placed(): leading, doubled and trailing spaces, a separator dropped at a wrap, lines beyond the sheet"""
    A = _atlas(fx, "mont")
    geo = R.geometry(int(A["origin_y"]))
    for text in ["", " ", " A", "A  B", "A B ", " ".join(["W" * 25] * 8), "WWWW " * 19, "  AB   CD  "]:
        codes = synth.encode_strings([text], 208)[0]
        lines, bad = E.placed(codes, A, geo)
        assert not bad and len(lines) <= geo.n_lines
        for line in lines:
            assert [chr(c) for _, c, _, _ in line] == [text[pos] for pos, _, _, _ in line]
            assert [pos for pos, _, _, _ in line] == list(range(line[0][0], line[0][0] + len(line)))
    assert len(E.placed(synth.encode_strings([" ".join(["W" * 25] * 8)], 208)[0], A, geo)[0]) == geo.n_lines


def test_char_report_is_parsed_strictly(monkeypatch):
    from ai_font_renderer_amd import model as M
    monkeypatch.delenv("AFR_CHAR_REPORT", raising=False)
    monkeypatch.delenv("AFR_DEVICE_DATA", raising=False)
    assert M._char_report_from_env() is None
    monkeypatch.setenv("AFR_CHAR_REPORT", "")
    assert M._char_report_from_env() is None
    monkeypatch.setenv("AFR_DEVICE_DATA", "default")
    for bad in ("0", "x", "-2", "1.5"):
        monkeypatch.setenv("AFR_CHAR_REPORT", bad)
        with pytest.raises(ValueError, match="AFR_CHAR_REPORT"):
            M._char_report_from_env()
    monkeypatch.setenv("AFR_CHAR_REPORT", "5")
    assert M._char_report_from_env() == 5
    monkeypatch.delenv("AFR_DEVICE_DATA")
    with pytest.raises(ValueError, match="AFR_DEVICE_DATA"):
        M._char_report_from_env()
    assert M._device_data_from_env() == (None, False)                              # its signature and result are what they were


def test_the_entry_refuses_bad_arguments_before_any_launch():
    from ai_font_renderer_amd import _lib
    lib = _lib.lib()
    EI, EU = _lib.AFR_EINVAL, _lib.AFR_EUNSUPPORTED
    fk = C.c_void_p(0x1000)

    def call(cells=fk, adv=fk, kern=None, n_codes=127, ch=14, cw=8, ox=0, oy=11, H=80, W=240, wrap=15360, nl=6, codes=fk, ldx=100, rows=None,
             n=4, pred=fk, per_pos=fk, by_code=fk, err=None, atlas=True, geo=True):
        a = _lib.AfrGlyphAtlas(cells, adv, kern, n_codes, ch, cw, ox, oy)
        g = _lib.AfrSheetGeometry(H, W, wrap, nl)
        return lib.afr_op_sheet_char_errors(C.byref(a) if atlas else None, C.byref(g) if geo else None, codes, ldx, rows, n, pred, per_pos,
                                            by_code, err, None)

    def said(*words):
        msg = lib.afr_last_error()
        return msg.startswith(b"afr_op_sheet_char_errors") and all(w in msg for w in words)

    # what compose refuses
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
    assert call(per_pos=None, by_code=None) == EI and said(b"both NULL")
    assert call(by_code=C.c_void_p(0x1004)) == EI and said(b"aligned")
    assert call(per_pos=C.c_void_p(0x1008)) == EI and said(b"16-byte")
    assert call(per_pos=C.c_void_p(0x1008), by_code=None) == EI and call(per_pos=None, by_code=C.c_void_p(0x1004)) == EI
    # the LDS budget with the position records and the code counters counted: 127 cells of 28 x 15 with their ranges and the layout are
    # 53340 + 720 + 5376 = 59436 bytes, which compose takes; the records and the counters (5152 + 5120) pass 64 KiB
    assert call(ch=28, cw=15, oy=11) == EU and said(b"LDS", b"counters")
    # 65025 * pixels must fit 32 bits: 66051 pixels at the most.  8256 x 8 = 66048 is taken (the call then fails on its outputs), 8257 x 8 is not
    assert 65025 * 66051 < 2 ** 32 <= 65025 * 66052
    assert call(H=8256, W=8, nl=1, per_pos=None, by_code=None) == EI and said(b"both NULL")
    assert call(H=8257, W=8, nl=1, per_pos=None, by_code=None) == EU and said(b"66051")
    assert call(H=8257, W=8, nl=1) == EU and said(b"66051")
