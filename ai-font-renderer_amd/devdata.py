"""The sheet data set composed on the device (csrc/dataset.hip): what datagen.generate writes as BMP files and
helpers.load_string_dataset_u8 reads back, produced directly in HBM by two kernels -- afr_op_dataset_text (the seeded LCG text
source of generate_font.ts:164-206, one lane per sample) and afr_op_compose_sheets (wrap, pens and blit of generate_font.ts:64-142
over a per-glyph atlas, one workgroup per sheet).

A sheet is a handful of glyph bitmaps blitted at integer pen positions, so the only thing PIL is still needed for is the atlas:
GlyphAtlas.from_font draws each printable ASCII glyph once and measures advances and pair kerning; the kernels reproduce
datagen.render_sheet's bytes from it exactly (tests/test_compose_cpu.py, tests/test_gpu_compose.py).

    atlas = GlyphAtlas.from_font("FiraCode-Retina.ttf").to("cuda")
    ds = reference_dataset(150000, atlas)            # TensorDataset(int64 codes [N, L], uint8 sheets [N, 80, 240]) in HBM

char_errors(atlas, codes, pred) runs the same layout once more (afr_op_sheet_char_errors) to charge a prediction's error to the characters
that own the pixels: the table AttentionFontRenderer.char_errors and AFR_CHAR_REPORT read.

The texts' alphabet is the caller's.  afr_op_dataset_text restates the reference's generator (words of A-Z); afr_op_dataset_text_w draws
each letter from a table of integer weights over the codes 33..126 instead -- text_weights(alphabet, by_code, floor_w, gain) builds the
table on the device, with equal weights or steered by char_errors' by-code counters where they lie -- and generate_codes(..., cum=...)
and reference_dataset(..., alphabet=...) draw from it.  With equal weights on A-Z the texts are the reference's byte for byte.

The letters can also depend on the letter before them: pair_errors(codes, per_pos) scatters char_errors' per-position records into a
table by (preceding character, character), pair_weights(alphabet, by_pair, floor_w, gain, min_chars) builds a first-order Markov table
from it (afr_op_pair_weights) and generate_codes(..., cum2=...) draws from that (afr_op_dataset_text_m) -- so a pair the model draws
badly, "WW" say, can be made frequent, which no table of single letters can do.

Two things the atlas cannot reproduce:
  * glyph substitution.  A font that replaces a run of characters by another glyph -- Fira Code's ligatures, "fi", "<>", "->" -- draws
    that glyph under raqm layout; the atlas knows single characters and pairs' kerning only.  With an alphabet that holds such pairs
    (lower, letters, alnum, ascii) a Fira Code atlas composes what the atlas says, not what a shaping engine would draw; the data set
    is self-consistent either way -- targets, char_errors and the steering all read the same layout -- and A-Z holds no such pair;
  * the .notdef box.  Codes outside 32..126 have a blank cell and no advance here, where PIL draws the font's missing-glyph box.  No
    alphabet reaches them: the text sources draw 32..126 only.
"""
import collections
import ctypes as C
import math

import numpy as np
import torch
import torch.utils.data as data

from . import _lib

FIRST_CODE, N_CODES = 32, 127            # one cell per code 0..126; 0..31 stay blank with advance 0
MIN_TEXT_LENGTH = 10                     # generate_font.ts:205
MAX_LINES = 16                           # afr_sheet_geometry.baseline
MAX_LDX = 256


class GlyphAtlas:
    """cells uint8 [n_codes, cell_h, cell_w] (coverage 0..255 = 255 - pixel, every cell cropped to the same box around the origin),
    adv64 int32 [n_codes] (advance in 1/64 px), kern64 int16 [n_codes, n_codes] (pair adjustment in 1/64 px), origin_x / origin_y
    (the cell's column / row that the pen and the baseline fall on).  Tensors; .to(device) moves them."""

    def __init__(self, cells, adv64, kern64, origin_x, origin_y):
        self.cells = torch.as_tensor(cells, dtype=torch.uint8).contiguous()
        self.adv64 = torch.as_tensor(adv64, dtype=torch.int32).contiguous()
        self.kern64 = None if kern64 is None else torch.as_tensor(kern64, dtype=torch.int16).contiguous()
        self.origin_x, self.origin_y = int(origin_x), int(origin_y)
        n = self.cells.shape[0]
        if self.cells.dim() != 3 or tuple(self.adv64.shape) != (n,) or (self.kern64 is not None and tuple(self.kern64.shape) != (n, n)):
            raise ValueError("atlas: cells [n, h, w], adv64 [n] and kern64 [n, n] do not match")

    n_codes = property(lambda self: self.cells.shape[0])
    cell_h = property(lambda self: self.cells.shape[1])
    cell_w = property(lambda self: self.cells.shape[2])
    device = property(lambda self: self.cells.device)

    @classmethod
    def from_font(cls, font_or_path=None, size=12):
        """font_or_path: a TTF path, a PIL FreeTypeFont, or None for Pillow's built-in scalable font at `size` (what datagen.generate
        uses without a font).  Every code 32..126 is drawn alone with anchor="ls" at an integer origin; the cells are the common
        bounding box of all the ink (and of the origin)."""
        from PIL import Image, ImageDraw, ImageFont
        if font_or_path is None:
            font = ImageFont.load_default(size)
        elif isinstance(font_or_path, (str, bytes)) or hasattr(font_or_path, "__fspath__"):
            font = ImageFont.truetype(font_or_path, size)
        else:
            font = font_or_path
        span = 4 * max(int(getattr(font, "size", size)), 8)
        ox = oy = span
        cov = np.zeros((N_CODES, 2 * span, 2 * span), dtype=np.uint8)
        for code in range(FIRST_CODE, N_CODES):
            img = Image.new("L", (2 * span, 2 * span), 255)
            ImageDraw.Draw(img).text((ox, oy), chr(code), fill=0, font=font, anchor="ls")
            cov[code] = 255 - np.asarray(img, dtype=np.uint8)
        ink = cov.max(0) > 0
        ink[oy, ox] = True
        ys, xs = np.nonzero(ink.any(1))[0], np.nonzero(ink.any(0))[0]
        if ys[0] == 0 or xs[0] == 0 or ys[-1] == 2 * span - 1 or xs[-1] == 2 * span - 1:
            raise ValueError("atlas: a glyph reaches the edge of the drawing canvas")
        cells = cov[:, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
        adv = np.zeros(N_CODES, dtype=np.int64)
        for code in range(FIRST_CODE, N_CODES):
            adv[code] = round(font.getlength(chr(code)) * 64)
        kern = np.zeros((N_CODES, N_CODES), dtype=np.int64)
        for a in range(FIRST_CODE, N_CODES):
            for b in range(FIRST_CODE, N_CODES):
                kern[a, b] = round(font.getlength(chr(a) + chr(b)) * 64) - adv[a] - adv[b]
        if np.abs(kern).max() > 32767:
            raise ValueError("atlas: a kerning pair does not fit 16 bits")
        return cls(cells, adv.astype(np.int32), kern.astype(np.int16), ox - xs[0], oy - ys[0])

    def to(self, device):
        return GlyphAtlas(self.cells.to(device), self.adv64.to(device), None if self.kern64 is None else self.kern64.to(device),
                          self.origin_x, self.origin_y)

    def arrays(self):
        """The atlas as numpy arrays by field name (what save writes)."""
        out = dict(cells=self.cells.cpu().numpy(), adv64=self.adv64.cpu().numpy(), origin_x=np.int32(self.origin_x),
                   origin_y=np.int32(self.origin_y))
        if self.kern64 is not None:
            out["kern64"] = self.kern64.cpu().numpy()
        return out

    def save(self, path):
        np.savez_compressed(path, **self.arrays())

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(z["cells"], z["adv64"], z["kern64"] if "kern64" in z.files else None, int(z["origin_x"]), int(z["origin_y"]))

    def _struct(self):
        return _lib.AfrGlyphAtlas(self.cells.data_ptr(), self.adv64.data_ptr(), None if self.kern64 is None else self.kern64.data_ptr(),
                                  self.n_codes, self.cell_h, self.cell_w, self.origin_x, self.origin_y)


def sheet_geometry(height=80, width=240, line_height=14.4, atlas=None):
    """afr_sheet_geometry of a sheet: wrap at the sheet's width, baseline of line i at floor((i + 1) * line_height + 0.5)
    (generate_font.ts:125-130, rounded the way the rasteriser places a fractional baseline), and every line whose cell still touches
    the sheet -- its top row, baseline - origin_y, lies above the bottom edge.  Without an atlas two line heights stand in for
    origin_y, which may add a line nothing is drawn from."""
    reach = atlas.origin_y if atlas is not None else int(math.ceil(2 * line_height))
    base = []
    while len(base) < MAX_LINES:
        b = int(math.floor((len(base) + 1) * line_height + 0.5))
        if b - reach >= height:
            break
        base.append(b)
    if not base:
        raise ValueError(f"sheet of height {height}: no line touches it")
    g = _lib.AfrSheetGeometry(int(height), int(width), int(width) * 64, len(base))
    for i, b in enumerate(base):
        g.baseline[i] = b
    return g


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _rows(t, n, device, what):
    if t is None:
        return None
    t = torch.as_tensor(t).to(device=device, dtype=torch.int64).contiguous().reshape(-1)
    if n is not None and t.numel() != n:
        raise ValueError(f"{what}: {t.numel()} entries for {n} samples")
    return t


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _codes_rows(codes, rows, device, shape="[N, L]"):
    """The codes as a contiguous int64 [N, L] tensor on the device and the rows of them that are read -> (codes, rows, n, L): sample j of n
    reads row rows[j], or row j of all N without rows."""
    codes = codes.to(device=device, dtype=torch.int64).contiguous()
    if codes.dim() != 2:
        raise ValueError(f"codes must be int64 {shape}")
    rows = _rows(rows, None, device, "rows")
    n = codes.shape[0] if rows is None else rows.numel()
    if rows is not None and n and (int(rows.min()) < 0 or int(rows.max()) >= codes.shape[0]):
        raise IndexError("rows outside codes")
    return codes, rows, n, codes.shape[1]


def _out_rows(rows, n, out, device):
    """The rows of out that n samples are written to: one per sample and inside out, or None for the first n, which out must have."""
    rows = _rows(rows, n, device, "rows")
    if rows is None and n > out.shape[0]:
        raise ValueError(f"{n} samples do not fit the {out.shape[0]} rows of out")
    if rows is not None and n and (int(rows.min()) < 0 or int(rows.max()) >= out.shape[0]):
        raise IndexError("rows outside out")
    return rows


def _table(table, name, shape, device):
    """A table of counters that a launch adds to: the caller's, or a new one of zeros."""
    if table is None:
        table = torch.zeros(shape, dtype=torch.int64, device=device)
    if table.dtype != torch.int64 or table.device != device or not table.is_contiguous() or tuple(table.shape) != tuple(shape):
        raise ValueError(f"{name} must be a contiguous int64 {list(shape)} tensor on {device}")
    return table


def _check_pred(pred, n, height, width, device):
    if pred.dtype != torch.uint8 or pred.device != device or not pred.is_contiguous() or pred.numel() != n * height * width:
        raise ValueError(f"pred must be a contiguous uint8 [{n}, {height}, {width}] tensor on {device}")


def _outside(atlas):
    """what the three sheet launches' flag means"""
    return IndexError(f"a code outside the atlas's 0..{atlas.n_codes - 1}")


def _member_words(alphabet):
    """An alphabet -- a name or literal string (synth.alphabet_members) or the 94 flags themselves -- as the three words the entries take."""
    from . import synth
    members = synth.alphabet_members(alphabet) if isinstance(alphabet, str) else [int(bool(m)) for m in alphabet]
    return (C.c_uint32 * 3)(*synth.members_words(members))


_ERR = object()                          # stands in a launch's arguments for the pointer to its err word


def _launch(device, entry, *args, flagged=None):
    """entry(*args, stream) on the device's current stream, _ERR among the arguments replaced by a fresh, zero err word.  flagged: the
    exception to raise when the launch set bit 0 of that word -- reading it waits for the launch; None leaves it unread.  The only place
    that reads the flag."""
    with torch.cuda.device(device):
        err = torch.zeros(1, dtype=torch.int32, device=device) if any(a is _ERR for a in args) else None
        _lib.check(entry(*[_ptr(err) if a is _ERR else a for a in args], _stream(device)))
        if flagged is not None and int(err) & 1:
            raise flagged


def text_weights(alphabet, by_code=None, floor_w=4096, gain=0, device=None):
    """afr_op_text_weights: the letter table of the weighted text source, built on the device -> (cum, w), two int32 [94] tensors holding
    uint32 words (the total stays below 2^27).  alphabet: a name or literal string (synth.alphabet_members) or the 94 flags themselves;
    by_code: char_errors' int64 [n_codes + 1, 5] table where it lies on the device, or None for equal weights floor_w.  Every member
    weighs floor_w + gain * min(its mean squared error / the alphabet's, 16): synth.text_weights in integers.  Nothing is read back."""
    from . import synth
    words = _member_words(alphabet)
    if by_code is not None:
        if by_code.dtype != torch.int64 or by_code.dim() != 2 or by_code.shape[1] != 5 or not by_code.is_contiguous() or not by_code.is_cuda:
            raise ValueError("by_code must be a contiguous int64 [n_codes + 1, 5] tensor on the device")
        device = by_code.device
    if device is None:
        raise ValueError("text_weights needs a device or a by_code table")
    device = torch.device(device)
    cum, w = torch.empty(synth.TEXT_CODES, dtype=torch.int32, device=device), torch.empty(synth.TEXT_CODES, dtype=torch.int32, device=device)
    _launch(device, _lib.lib().afr_op_text_weights, _ptr(by_code), 0 if by_code is None else by_code.shape[0] - 1, words, int(floor_w), int(gain),
            _ptr(cum), _ptr(w))
    return cum, w


PAIR_SHAPE = (95, 94)                    # [context][letter]: context 0 = word start, context 1 + i = after code 33 + i


def pair_errors(codes, per_pos, rows=None, by_pair=None):
    """afr_op_pair_errors: char_errors' per-position records (per_pos [n, L + 1, 4], as CharErrors holds them) scattered into the table
    by (preceding character, character) -> int64 [95, 94, 4] = {chars, pixels, sumsq, wrong} on the device; context 0 is "no letter
    before" (position 0, after a space or any code outside 33..126), context 1 + i "after code 33 + i".  Sample j reads row rows[j]
    (default j) of the int64 [N, L] codes, as char_errors did.  by_pair (default new and zero) is added to.  Nothing is read back."""
    device = per_pos.device
    if codes.dim() != 2 or not per_pos.is_cuda:
        raise ValueError("codes must be int64 [N, L], per_pos a tensor on the device")
    codes, rows, n, L = _codes_rows(codes, rows, device)
    if per_pos.dtype not in (torch.int32, torch.int64) or tuple(per_pos.shape) != (n, L + 1, 4):
        raise ValueError(f"per_pos must be an int32 or int64 [{n}, {L + 1}, 4] tensor (char_errors' records)")
    per_pos = per_pos.to(torch.int32).contiguous()                    # the uint32 words afr_op_sheet_char_errors stored
    by_pair = _table(by_pair, "by_pair", PAIR_SHAPE + (4,), device)
    if n:
        _launch(device, _lib.lib().afr_op_pair_errors, _ptr(codes), L, _ptr(rows), n, _ptr(per_pos), _ptr(by_pair))
    return by_pair


def pair_weights(alphabet, by_pair=None, floor_w=4096, gain=0, min_chars=0, device=None):
    """afr_op_pair_weights: the table of the Markov text source, built on the device -> (cum2, w2), two int32 [95, 94] tensors holding
    uint32 words.  alphabet as text_weights'; by_pair: pair_errors' int64 [95, 94, 4] table where it lies on the device, or None for
    equal weights floor_w on every pair of members.  A pair weighs floor_w + gain * min(its mean squared error / the table's, 16), a
    pair seen fewer than min_chars times as the average: synth.pair_weights in integers.  Nothing is read back."""
    words = _member_words(alphabet)
    if by_pair is not None:
        if by_pair.dtype != torch.int64 or tuple(by_pair.shape) != PAIR_SHAPE + (4,) or not by_pair.is_contiguous() or not by_pair.is_cuda:
            raise ValueError("by_pair must be a contiguous int64 [95, 94, 4] tensor on the device")
        device = by_pair.device
    if device is None:
        raise ValueError("pair_weights needs a device or a by_pair table")
    if not 0 <= int(min_chars) <= 0xFFFFFFFF:
        raise ValueError(f"min_chars {min_chars} must lie in 0..2^32 - 1")
    device = torch.device(device)
    cum2, w2 = torch.empty(PAIR_SHAPE, dtype=torch.int32, device=device), torch.empty(PAIR_SHAPE, dtype=torch.int32, device=device)
    _launch(device, _lib.lib().afr_op_pair_weights, _ptr(by_pair), words, int(floor_w), int(gain), int(min_chars), _ptr(cum2), _ptr(w2))
    return cum2, w2


def generate_codes(n, first_seed=42, max_length=100, device=None, out=None, rows=None, seed_rows=None, lens=None, cum=None, check_total=True,
                   cum2=None):
    """afr_op_dataset_text: the texts of synth.lcg_text(first_seed + seed, 10, max_length) as zero-padded int64 codes.  Sample j of n
    takes seed seed_rows[j] (default j) and goes to row rows[j] (default j) of out -- int64 [N, L >= max_length], default a new
    [n, max_length] -- and of lens (int32 [N], optional with out).  Returns (out, lens).  cum (text_weights' int32 [94] table on the
    device): afr_op_dataset_text_w instead, the texts of synth.lcg_text_weighted; a table whose total is 0 is a ValueError (the rows are
    zero-filled and flagged on the device; reading the flag waits for the launch, check_total=False leaves it unread -- for a table from
    text_weights, whose total cannot be 0).  cum2 (pair_weights' int32 [95, 94] table on the device): afr_op_dataset_text_m, the texts of
    synth.lcg_text_markov; a sample that reaches a context whose total is 0 is a ValueError in the same way.  cum and cum2 together is a
    ValueError."""
    if cum is not None and cum2 is not None:
        raise ValueError("cum and cum2 together: a text is drawn from one table")
    if out is None:
        if rows is not None:
            raise ValueError("rows needs the buffer they are rows of (out)")
        if device is None:
            raise ValueError("generate_codes needs a device or an out tensor")
        out = torch.empty((n, max_length), dtype=torch.int64, device=device)
        lens = torch.empty(n, dtype=torch.int32, device=device)
    device = out.device
    if out.dtype != torch.int64 or out.dim() != 2 or not out.is_contiguous():
        raise ValueError("out must be a contiguous int64 [N, L] tensor")
    if lens is not None and (lens.dtype != torch.int32 or lens.device != device or lens.numel() != out.shape[0] or not lens.is_contiguous()):
        raise ValueError("lens must be a contiguous int32 [N] tensor beside out")
    rows, seed_rows = _out_rows(rows, n, out, device), _rows(seed_rows, n, device, "seed_rows")
    if cum is not None and (cum.dtype != torch.int32 or cum.device != device or cum.numel() != 94 or not cum.is_contiguous()):
        raise ValueError(f"cum must be a contiguous int32 [94] tensor on {device} (text_weights' table)")
    if cum2 is not None and (cum2.dtype != torch.int32 or cum2.device != device or tuple(cum2.shape) != PAIR_SHAPE or not cum2.is_contiguous()):
        raise ValueError(f"cum2 must be a contiguous int32 [95, 94] tensor on {device} (pair_weights' table)")
    # the entry, its table before out, its err word at the end, and what a set flag means: chosen once, launched once
    if cum2 is not None:
        entry, table, err = _lib.lib().afr_op_dataset_text_m, [_ptr(cum2)], [_ERR]
        zero_total = "a text reached a context of the pair table whose total weight is 0"
    elif cum is not None:
        entry, table, err = _lib.lib().afr_op_dataset_text_w, [_ptr(cum)], [_ERR]
        zero_total = "the letter table's total weight is 0: no text can be drawn from it"
    else:
        entry, table, err = _lib.lib().afr_op_dataset_text, [], []
    _launch(device, entry, int(first_seed), _ptr(seed_rows), _ptr(rows), n, MIN_TEXT_LENGTH, int(max_length), *table, _ptr(out), out.shape[1],
            _ptr(lens), *err, flagged=ValueError(zero_total) if err and check_total else None)
    return out, lens


def compose_sheets(atlas, codes, height=80, width=240, out=None, rows=None, line_height=14.4):
    """afr_op_compose_sheets: uint8 [n, height, width] sheets of the int64 [n, L] codes, bit for bit datagen.render_sheet's for text the
    font does not substitute glyphs in.  Sample j goes to row rows[j] (default j) of out (uint8 [N, height, width], default new).  A
    code outside the atlas is an IndexError (it is skipped on the device and flagged; reading the flag waits for the launch)."""
    device = atlas.device
    codes, _, n, L = _codes_rows(codes, None, device, "[n, L]")
    if out is None:
        if rows is not None:
            raise ValueError("rows needs the buffer they are rows of (out)")
        out = torch.empty((n, height, width), dtype=torch.uint8, device=device)
    if out.dtype != torch.uint8 or out.device != device or not out.is_contiguous() or tuple(out.shape[1:]) != (height, width):
        raise ValueError(f"out must be a contiguous uint8 [N, {height}, {width}] tensor on {device}")
    rows = _out_rows(rows, n, out, device)
    a, g = atlas._struct(), sheet_geometry(height, width, line_height, atlas)
    _launch(device, _lib.lib().afr_op_compose_sheets, C.byref(a), C.byref(g), _ptr(codes), L, _ptr(rows), n, _ptr(out), _ERR,
            flagged=_outside(atlas))
    return out


class CharErrors(collections.namedtuple("CharErrors", "per_pos by_code")):
    """afr_op_sheet_char_errors' two tables as int64 tensors (the counters are below 2^63): per_pos [n, L + 1, 4] = {pixels, sumsq, off2,
    wrong} of the character at each position of its row of codes, slot L the background; by_code [n_codes + 1, 5] = {chars, pixels,
    sumsq, off2, wrong} summed by code, row n_codes the background with chars = sheets."""


def char_errors(atlas, codes, pred, height=80, width=240, rows=None, by_code=None, line_height=14.4):
    """afr_op_sheet_char_errors: how far the uint8 [n, height, width] prediction `pred` (AttentionFontRenderer.render_u8, evaluate's q) is
    from the sheets compose_sheets draws, charged to the character that owns each pixel -- the glyph with the largest coverage there,
    the earlier one on a tie; pixels no glyph inks are the background.  Sample j reads row rows[j] (default j) of the int64 [N, L]
    codes, so a batch can read a bound data set's codes where they lie.  by_code (int64 [n_codes + 1, 5], default new and zero) is
    added to.  A code outside the atlas is an IndexError, as in compose_sheets."""
    device = atlas.device
    codes, rows, n, L = _codes_rows(codes, rows, device)
    _check_pred(pred, n, height, width, device)
    by_code = _table(by_code, "by_code", (atlas.n_codes + 1, 5), device)
    per_pos = torch.empty((n, L + 1, 4), dtype=torch.int32, device=device)
    a, g = atlas._struct(), sheet_geometry(height, width, line_height, atlas)
    _launch(device, _lib.lib().afr_op_sheet_char_errors, C.byref(a), C.byref(g), _ptr(codes), L, _ptr(rows), n, _ptr(pred), _ptr(per_pos),
            _ptr(by_code), _ERR, flagged=_outside(atlas))
    return CharErrors(per_pos.to(torch.int64) & 0xFFFFFFFF, by_code)


class ReadBack(collections.namedtuple("ReadBack", "read score confusion codes")):
    """afr_op_sheet_read_back's three outputs: read uint8 [n, L] (the code read at each position of its row of codes, 0 where no
    character was scored), score int64 [n, L, 2] = {the winner's score, the true code's}, confusion int64 [n_codes, n_codes]
    (confusion[c, r] = characters of code c read as r; the counters are below 2^63) -- and codes, the int64 [n, L] rows that were read."""

    def texts(self):
        """what was read, one string per sheet: the character read at every scored position, the row's own space where the row holds
        one, nothing at any other position (behind the text, skipped codes, characters on no drawn line)"""
        out = []
        for rr, cr in zip(self.read.cpu().tolist(), self.codes.cpu().tolist()):
            end = cr.index(0) if 0 in cr else len(cr)
            out.append("".join(chr(r) if r else " " if c == 32 else "" for r, c in zip(rr[:end], cr[:end])))
        return out

    def rate(self):
        """(scored characters, how many were read right, how many were read blank), from the confusion table"""
        return confusion_rate(self.confusion)


def confusion_rate(confusion):
    """(scored characters, read right, read blank) of a confusion table; one transfer"""
    scored, right, blank = torch.stack([confusion.sum(), confusion.diagonal().sum(), confusion[:, 32].sum()]).cpu().tolist()
    return scored, right, blank


def read_back(atlas, codes, pred, alphabet="upper", height=80, width=240, rows=None, confusion=None, line_height=14.4):
    """afr_op_sheet_read_back: which glyph of the atlas each drawn character of the uint8 [n, height, width] prediction `pred`
    (AttentionFontRenderer.render_u8, evaluate's q) looks like.  For every character on a drawn line but the space, every candidate --
    the codes of `alphabet` (a name or literal string, synth.alphabet_members, or the 94 flags), the blank and the true code -- is put at
    the character's pen over the neighbours compose_sheets draws there, and the candidate with the least squared distance to the
    prediction over the character's cell box is what was read: the true code among equals, then the smallest.  Sample j reads row
    rows[j] (default j) of the int64 [N, L] codes.  confusion (int64 [n_codes, n_codes], default new and zero) is added to.  A code
    outside the atlas is an IndexError, as in compose_sheets.  -> ReadBack."""
    device = atlas.device
    words = _member_words(alphabet)
    codes, rows, n, L = _codes_rows(codes, rows, device)
    _check_pred(pred, n, height, width, device)
    confusion = _table(confusion, "confusion", (atlas.n_codes, atlas.n_codes), device)
    read = torch.empty((n, L), dtype=torch.uint8, device=device)
    score = torch.empty((n, L, 2), dtype=torch.int32, device=device)
    a, g = atlas._struct(), sheet_geometry(height, width, line_height, atlas)
    _launch(device, _lib.lib().afr_op_sheet_read_back, C.byref(a), C.byref(g), _ptr(codes), L, _ptr(rows), n, _ptr(pred), words, _ptr(read),
            _ptr(score), _ptr(confusion), _ERR, flagged=_outside(atlas))
    return ReadBack(read, score.to(torch.int64) & 0xFFFFFFFF, confusion, codes if rows is None else codes[rows])


def reference_dataset(n, atlas, first_seed=42, max_length=100, height=80, width=240, alphabet=None):
    """TensorDataset(int64 [n, L] codes, uint8 [n, height, width] sheets) on the atlas's device: the tensors
    helpers.load_string_dataset_u8 returns for the folder datagen.generate(out_dir, n, font, first_seed) writes -- L is the longest
    text's length, as there.  alphabet (a name or literal, synth.alphabet_members): the texts come from the weighted source with equal
    weights over that alphabet instead; "upper" gives the same bytes as None."""
    cum = None if alphabet is None else text_weights(alphabet, device=atlas.device)[0]
    codes, lens = generate_codes(n, first_seed, max_length, device=atlas.device, cum=cum)
    codes = codes[:, :int(lens.max())].contiguous()
    return data.TensorDataset(codes, compose_sheets(atlas, codes, height, width))
