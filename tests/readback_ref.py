"""numpy twin of afr_op_sheet_read_back (csrc/dataset.hip): for every drawn character, which glyph of the atlas -- put at this
character's pen among its neighbours -- explains a prediction's pixels best.  Written from the entry's contract in include/afr.h and from
compose_ref's geometry and fold and charerr_ref.placed (imported, not edited), not from the kernel.  tests/test_readback_cpu.py holds it
to the facts counted when the definition was chosen and shows that each planted fault changes an output of the GPU tests' inputs;
tests/test_gpu_readback.py holds the kernel against it.

fault= plants one mistake an implementation can make: "tie_small" (equal scores go to the smallest code, the true one or not), "no_ctx"
(the hypotheses ignore the neighbours: ctx = 0), "ctx_self" (the context includes the scored glyph itself) and "packed_pos" (outputs
indexed by the character's place in the packed text, not in its row of codes)."""
import numpy as np

from .charerr_ref import placed
from .compose_ref import geometry  # noqa: F401  (for the callers)

FAULTS = (None, "tie_small", "no_ctx", "ctx_self", "packed_pos")
BLANK, FIRST, CODES = 32, 33, 94


def candidates(members, c):
    """the member codes (94 flags, flag i = code 33 + i), the blank, and the character's own code, ascending"""
    assert len(members) == CODES
    return sorted({FIRST + i for i, m in enumerate(members) if m} | {BLANK, int(c)})


def _box(top, left, ch, cw, H, W):
    return max(top, 0), min(top + ch, H), max(left, 0), min(left + cw, W)


def windows(atlas, geo, codes, fault=None):
    """-> (the scored characters of one sheet in (line, character) order, whether a code was dropped).  A scored character is
    (position in `codes`, code, place in the kept text, (y0, y1, x0, x1) its window on the sheet, (cy0, cx0) the window's first pixel
    in the cell, int64 [y1 - y0][x1 - x0] ctx).  ctx does not depend on the prediction: a caller with several predictions of one sheet
    passes this on."""
    assert fault in FAULTS
    cells = np.asarray(atlas["cells"])
    _, ch, cw = cells.shape
    ox, oy = int(atlas["origin_x"]), int(atlas["origin_y"])
    H, W = geo.height, geo.width
    lines, bad = placed(codes, atlas, geo)
    glyphs = [(pos, c, packed, geo.baseline[i] - oy, px - ox) for i, line in enumerate(lines) for pos, c, px, packed in line]
    out = []
    for g, (pos, c, packed, top, left) in enumerate(glyphs):
        y0, y1, x0, x1 = _box(top, left, ch, cw, H, W)
        if c == BLANK or y0 >= y1 or x0 >= x1:
            continue
        ctx = np.zeros((y1 - y0, x1 - x0), dtype=np.int64)
        if fault != "no_ctx":
            for o, (_, oc, _, otop, oleft) in enumerate(glyphs):
                if o == g and fault != "ctx_self":
                    continue
                # the part of the other glyph's cell that lies in this window
                v0, v1, u0, u1 = max(y0, otop), min(y1, otop + ch), max(x0, oleft), min(x1, oleft + cw)
                if v0 >= v1 or u0 >= u1:
                    continue
                b = cells[oc, v0 - otop:v1 - otop, u0 - oleft:u1 - oleft].astype(np.int64)
                m = ctx[v0 - y0:v1 - y0, u0 - x0:u1 - x0]
                ctx[v0 - y0:v1 - y0, u0 - x0:u1 - x0] = m + b - (m * b + 127) // 255
        out.append((pos, c, packed, (y0, y1, x0, x1), (y0 - top, x0 - left), ctx))
    return out, bad


def read_back(atlas, geo, codes, pred, members, fault=None, win=None):
    """one sheet -> (uint8 [ldx] read, uint64 [ldx][2] score, uint64 [n_codes][n_codes] confusion, whether a code was dropped);
    win: what windows(atlas, geo, codes, fault) returned"""
    cells = np.asarray(atlas["cells"])
    n_codes, ldx = cells.shape[0], len(codes)
    scored, bad = win if win is not None else windows(atlas, geo, codes, fault)
    read, score = np.zeros(ldx, dtype=np.uint8), np.zeros((ldx, 2), dtype=np.uint64)
    confusion = np.zeros((n_codes, n_codes), dtype=np.uint64)
    for pos, c, packed, (y0, y1, x0, x1), (cy0, cx0), ctx in scored:
        a = 255 - np.asarray(pred[y0:y1, x0:x1], dtype=np.int64)
        cand = candidates(members, c)
        b = cells[cand, cy0:cy0 + y1 - y0, cx0:cx0 + x1 - x0].astype(np.int64)
        hyp = ctx + b - (ctx * b + 127) // 255
        s = ((a - hyp) ** 2).sum((1, 2))
        least = int(s.min())
        tied = [k for k, v in zip(cand, s) if int(v) == least]
        won = c if c in tied and fault != "tie_small" else tied[0]
        at = packed if fault == "packed_pos" else pos
        read[at], score[at] = won, (least, int(s[cand.index(c)]))
        confusion[c, won] += np.uint64(1)
    return read, score, confusion, bad


def read_back_batch(atlas, geo, codes, preds, members, fault=None, wins=None):
    """-> (uint8 [n][ldx], uint64 [n][ldx][2], uint64 [n_codes][n_codes] summed over the batch, bool [n])"""
    res = [read_back(atlas, geo, row, p, members, fault, None if wins is None else wins[j]) for j, (row, p) in enumerate(zip(codes, preds))]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), sum(r[2] for r in res), np.array([r[3] for r in res])


def rate(confusion):
    """(scored characters, read right, read blank) of a confusion table"""
    confusion = np.asarray(confusion)
    return int(confusion.sum()), int(np.trace(confusion)), int(confusion[:, BLANK].sum())


ALL = [1] * CODES                                                       # every code 33..126 a candidate


# ---------------------------------------------------------------------------------------------- the cases both test files use
def mini_predictions(sheets, synth, tensor_id=7311):
    """what the miniature sheets are read back from -> name -> uint8 like sheets: the target itself, a white sheet and hashed noise"""
    return {"target": sheets, "white": np.full_like(sheets, 255), "noise": synth.hash_u8(tensor_id, sheets.shape)}


def substitutions(codes, seed=20261):
    """one non-space character of every text that has one replaced by another code of 33..126 -> (the rows, [(row, position, substitute)])"""
    rng = np.random.default_rng(seed)
    out, subs = np.array(codes, copy=True), []
    for j, row in enumerate(codes):
        row = [int(c) for c in row]
        end = row.index(0) if 0 in row else len(row)
        at = [i for i in range(end) if row[i] != BLANK]
        if not at:                                                      # an empty text, or spaces alone
            continue
        pos = at[int(rng.integers(len(at)))]
        sub = int(rng.integers(FIRST, FIRST + CODES - 1))
        sub += sub >= row[pos]                                          # any code of 33..126 but the one that stands there
        out[j, pos] = sub
        subs.append((j, pos, sub))
    return out, subs
