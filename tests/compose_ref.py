"""numpy twin of the device data set (csrc/dataset.hip): the integer LCG text source and the integer sheet composer over a glyph atlas,
written from datagen.wrap_text / render_sheet and synth.lcg_text, not from the kernels.  tests/test_compose_cpu.py holds it against
PIL's own sheets; tests/test_gpu_compose.py holds the kernels against it.

An atlas here is a mapping with cells uint8 [n_codes][cell_h][cell_w] (coverage, 255 - pixel), adv64 int32 [n_codes], kern64 int16
[n_codes][n_codes] or None, origin_x, origin_y.  fault= plants one mistake a composer can make, for the tests that show each is seen:
"max" (the darker of two overlapping glyphs instead of compositing one over the other), "floor_pen" (the pen cut to a pixel instead of
rounded) and "no_kern" (kerning dropped from the pens and from the measured widths)."""
from types import SimpleNamespace

import numpy as np

FAULTS = (None, "max", "floor_pen", "no_kern")


def lcg_codes(seed, min_len=10, max_len=100):
    """synth.lcg_text in integers: int(rnd() * k) == (state * k) >> 32, since state / 2^32 * k is exact in a double."""
    state = int(seed) & 0xFFFFFFFF

    def draw(k):
        nonlocal state
        state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
        return (state * k) >> 32

    remaining = draw(max_len - min_len + 1) + min_len
    out = []
    while remaining > 0:
        wl = min(draw(10) + 1, remaining)
        out += [65 + draw(26) for _ in range(wl)]
        remaining -= wl
        if remaining > 0:
            out.append(32)
            remaining -= 1
    return out


def encode(seeds, ldx, min_len=10, max_len=100):
    """(int64 [n][ldx] zero-padded codes, int32 [n] lengths) of lcg_codes(seed) for every seed"""
    codes, lens = np.zeros((len(seeds), ldx), dtype=np.int64), np.zeros(len(seeds), dtype=np.int32)
    for j, s in enumerate(seeds):
        c = lcg_codes(s, min_len, max_len)
        codes[j, :len(c)], lens[j] = c, len(c)
    return codes, lens


def geometry(origin_y, height=80, width=240, line_height=14.4):
    """baseline of line i at floor((i + 1) * line_height + 0.5); the lines whose cell (top row baseline - origin_y) starts above the
    sheet's bottom edge, 16 at the most"""
    base = []
    while len(base) < 16:
        b = int(np.floor((len(base) + 1) * line_height + 0.5))
        if b - origin_y >= height:
            break
        base.append(b)
    return SimpleNamespace(height=height, width=width, wrap_width64=width * 64, n_lines=len(base), baseline=base)


def text_of(codes, n_codes):
    """the codes up to the first 0, without those outside [0, n_codes); and whether any was dropped"""
    codes = [int(c) for c in codes]
    if 0 in codes:
        codes = codes[:codes.index(0)]
    kept = [c for c in codes if 0 <= c < n_codes]
    return kept, len(kept) != len(codes)


def _kern(atlas, fault):
    k = atlas["kern64"]
    return None if k is None or fault == "no_kern" else np.asarray(k, dtype=np.int64)


def width64(s, atlas, fault=None):
    adv, k = np.asarray(atlas["adv64"], dtype=np.int64), _kern(atlas, fault)
    return int(sum(adv[c] for c in s) + (sum(k[a][b] for a, b in zip(s, s[1:])) if k is not None else 0))


def wrap(text, atlas, wrap_width64, fault=None):
    """datagen.wrap_text over lists of codes: split at every 32, empty words included"""
    words, cur = [[]], []
    for c in text:
        if c == 32:
            words.append([])
        else:
            words[-1].append(c)
    lines = []
    for word in words:
        cand = cur + [32] + word if cur else list(word)
        if width64(cand, atlas, fault) > wrap_width64 and cur:
            lines.append(cur)
            cur = list(word)
        else:
            cur = cand
    if cur:
        lines.append(cur)
    return lines


def pens(line, atlas, fault=None):
    """pixel pen of every character of one line"""
    adv, k = np.asarray(atlas["adv64"], dtype=np.int64), _kern(atlas, fault)
    out, pen = [], 0
    for j, c in enumerate(line):
        if j and k is not None:
            pen += int(k[line[j - 1]][c])
        out.append(pen >> 6 if fault == "floor_pen" else (pen + 32) >> 6)
        pen += int(adv[c])
    return out


def compose(atlas, geo, codes, fault=None):
    """-> (uint8 [height][width] sheet, whether a code was out of range)"""
    assert fault in FAULTS
    cells = np.asarray(atlas["cells"])
    n_codes, ch, cw = cells.shape
    ox, oy = int(atlas["origin_x"]), int(atlas["origin_y"])
    text, bad = text_of(codes, n_codes)
    m = np.zeros((geo.height, geo.width), dtype=np.int64)
    for i, line in enumerate(wrap(text, atlas, geo.wrap_width64, fault)[:geo.n_lines]):
        top = geo.baseline[i] - oy
        for c, px in zip(line, pens(line, atlas, fault)):
            left = px - ox
            y0, y1, x0, x1 = max(top, 0), min(top + ch, geo.height), max(left, 0), min(left + cw, geo.width)
            if y0 >= y1 or x0 >= x1:
                continue
            b = cells[c, y0 - top:y1 - top, x0 - left:x1 - left].astype(np.int64)
            old = m[y0:y1, x0:x1]
            m[y0:y1, x0:x1] = np.maximum(old, b) if fault == "max" else old + b - (old * b + 127) // 255
    return (255 - m).astype(np.uint8), bad


def compose_batch(atlas, geo, codes, fault=None):
    """-> (uint8 [n][height][width], bool [n] out-of-range flags) of the rows of codes"""
    res = [compose(atlas, geo, row, fault) for row in codes]
    return np.stack([r[0] for r in res]), np.array([r[1] for r in res])
