"""numpy twin of afr_op_sheet_char_errors (csrc/dataset.hip): a prediction's error against the composed sheet, charged pixel by pixel to
the character that owns the pixel.  Written from compose_ref's text_of, wrap, pens and geometry (imported, not edited) and the
entry's contract in include/afr.h, not from the kernel.  tests/test_charerr_cpu.py holds it against numpy's whole-sheet sums and shows
that each planted fault changes the records of the GPU tests' inputs; tests/test_gpu_charerr.py holds the kernel against it.

fault= plants one mistake an implementation can make: "last" (the last glyph with ink owns the pixel), "tie_late" (equal coverage
goes to the later glyph), "packed_pos" (records indexed by the character's place in the packed text, not in its row of codes) and
"bg_any_cell" (a pixel under any cell, inked or not, is not counted as background: it goes to the first glyph whose cell covers it)."""
import numpy as np

from .compose_ref import geometry, pens, text_of, wrap  # noqa: F401  (geometry: for the callers)

FAULTS = (None, "last", "tie_late", "packed_pos", "bg_any_cell")
FIELDS = ("pixels", "sumsq", "off2", "wrong")


def placed(codes, atlas, geo):
    """-> (the drawn lines as lists of (position in `codes`, code, pen pixel, place in the kept text), whether a code was dropped).
    wrap() returns every line as codes; a line is a contiguous piece of the kept text that never starts with a space (a line that would is started by the word
    behind it), and only spaces are dropped between lines and in front of the first, so walking the kept text and skipping spaces at
    every line's start finds each character's place again."""
    n_codes = np.asarray(atlas["cells"]).shape[0]
    row = [int(c) for c in codes]
    if 0 in row:
        row = row[:row.index(0)]
    where = [i for i, c in enumerate(row) if 0 <= c < n_codes]
    text, bad = text_of(codes, n_codes)
    assert [row[i] for i in where] == text
    lines, at = [], 0
    for line in wrap(text, atlas, geo.wrap_width64):
        assert line and line[0] != 32
        while text[at] == 32:
            at += 1
        assert text[at:at + len(line)] == line
        lines.append([(where[at + k], c, px, at + k) for k, (c, px) in enumerate(zip(line, pens(line, atlas)))])
        at += len(line)
    assert all(c == 32 for c in text[at:])
    return lines[:geo.n_lines], bad


def owners(atlas, geo, codes, fault=None):
    """-> (int64 [height][width] composed coverage m, int [height][width] owner: the glyph's place in (line, character) order or -1,
    the drawn glyphs in that order as (position, code, place in the kept text), whether a code was dropped, bool [height][width]
    under any cell, int [height][width] how many glyphs have b > 0, bool [height][width] whether the largest b is reached twice)"""
    assert fault in FAULTS
    cells = np.asarray(atlas["cells"])
    _, ch, cw = cells.shape
    ox, oy = int(atlas["origin_x"]), int(atlas["origin_y"])
    lines, bad = placed(codes, atlas, geo)
    H, W = geo.height, geo.width
    m, top = np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=np.int64)
    owner, inked = np.full((H, W), -1, dtype=np.int64), np.zeros((H, W), dtype=np.int64)
    tied, under = np.zeros((H, W), dtype=bool), np.zeros((H, W), dtype=bool)
    glyphs = []
    for i, line in enumerate(lines):
        y_top = geo.baseline[i] - oy
        for pos, c, px, packed in line:
            g = len(glyphs)
            glyphs.append((pos, c, packed))
            left = px - ox
            y0, y1, x0, x1 = max(y_top, 0), min(y_top + ch, H), max(left, 0), min(left + cw, W)
            if y0 >= y1 or x0 >= x1:
                continue
            b = cells[c, y0 - y_top:y1 - y_top, x0 - left:x1 - left].astype(np.int64)
            win = (slice(y0, y1), slice(x0, x1))
            m[win] = m[win] + b - (m[win] * b + 127) // 255
            if fault == "bg_any_cell":
                take = (b > top[win]) | ((owner[win] < 0) & ~under[win])       # an empty pixel of the first cell over it is taken too
            elif fault == "last":
                take = b > 0
            elif fault == "tie_late":
                take = (b >= top[win]) & (b > 0)
            else:
                take = b > top[win]
            tied[win] = np.where(b > top[win], False, tied[win] | ((b == top[win]) & (b > 0)))
            owner[win] = np.where(take, g, owner[win])
            top[win] = np.maximum(top[win], b)
            inked[win] += b > 0
            under[win] = True
    return m, owner, glyphs, bad, under, inked, tied


def measures(m, pred):
    """the four per-pixel measures [4][height][width] of a prediction against the target 255 - m"""
    t, p = 255 - m, np.asarray(pred, dtype=np.int64)
    d = np.abs(p - t)
    return np.stack([np.ones_like(d), d * d, (d >= 2).astype(np.int64), ((p >= 128) != (t >= 128)).astype(np.int64)])


def char_errors(atlas, geo, codes, pred, fault=None, own=None):
    """one sheet -> (uint64 [ldx + 1][4] per_pos, uint64 [n_codes + 1][5] by_code, whether a code was dropped); own: what
    owners(atlas, geo, codes, fault) returned, for a caller that measures several predictions of one sheet"""
    n_codes, ldx = np.asarray(atlas["cells"]).shape[0], len(codes)
    m, owner, glyphs, bad, _, _, _ = own if own is not None else owners(atlas, geo, codes, fault)
    e = measures(m, pred)
    per_pos, by_code = np.zeros((ldx + 1, 4), dtype=np.uint64), np.zeros((n_codes + 1, 5), dtype=np.uint64)
    by_glyph = np.stack([np.bincount(owner.ravel() + 1, weights=None if f == 0 else e[f].ravel(), minlength=len(glyphs) + 1) for f in range(4)], 1)
    by_glyph = np.rint(by_glyph).astype(np.uint64)                      # bincount's float64 weights: every sum here is below 2^53
    per_pos[ldx] = by_glyph[0]
    by_code[n_codes, 0], by_code[n_codes, 1:] = 1, by_glyph[0]
    for g, (pos, c, packed) in enumerate(glyphs):
        per_pos[packed if fault == "packed_pos" else pos] += by_glyph[g + 1]
        by_code[c, 0] += np.uint64(1)
        by_code[c, 1:] += by_glyph[g + 1]
    return per_pos, by_code, bad


def char_errors_batch(atlas, geo, codes, preds, fault=None):
    """-> (uint64 [n][ldx + 1][4], uint64 [n_codes + 1][5] summed over the batch, bool [n])"""
    res = [char_errors(atlas, geo, row, p, fault) for row, p in zip(codes, preds)]
    return np.stack([r[0] for r in res]), sum(r[1] for r in res), np.array([r[2] for r in res])


# ---------------------------------------------------------------------------------------------- the cases both test files use
MINI_TEXTS = ["AV TO", "WWWWWW", "", "J", "A B C D E F G", "IIII IIII IIII", "Q  Q", " Ty.", "MMMM MM M"]      # + 16 LCG texts: test_compose_miniature_sheet's


def mini_case(atlas, synth):
    """the 8 x 24 sheets under cells that reach over all four edges -> (geometry, int64 [25][100] codes)"""
    geo = geometry(int(atlas["origin_y"]), height=8, width=24, line_height=6.0)
    return geo, synth.encode_strings(MINI_TEXTS + [synth.lcg_text(42 + i) for i in range(16)], 100)


def dirty_rows(synth):
    """test_compose_bad_codes_are_flagged_and_skipped's rows: codes outside the atlas inside a kerning run, first, at a space, and
    behind the text -- which then goes on"""
    dirty = synth.encode_strings(["AVAVAV TO TY", "HELLO WORLD", "P JAL WZ", "TO"], 100)
    dirty[0, 3], dirty[1, 0], dirty[1, 5], dirty[3, 2] = 200, -1, 127, 1 << 40
    dirty[3, 3] = ord("Y")
    return dirty


def predictions(sheets, synth, tensor_id=7300):
    """the three predictions every sheet is measured with -> name -> uint8 like sheets: the target itself, hashed noise, and the sheet
    of the next text"""
    return {"target": sheets, "noise": synth.hash_u8(tensor_id, sheets.shape), "next": np.roll(sheets, -1, axis=0)}
