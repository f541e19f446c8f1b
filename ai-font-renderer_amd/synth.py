"""Portable synthetic data: the same integers on every box, no torch RNG involved.

* text generator  -- integer-exact restatement of the reference's seeded LCG text source
                     (reference generate_font.ts:164-199, sample i uses seed i+42, :204)
* weights/targets -- counter-based splitmix64 hash of (tensor_id << 40) + flat_index
                     (SURVEY.md App. D); weights are never stored in fixtures
* dropout masks   -- 32-bit counter hash shared bit-for-bit with the HIP kernels
                     (csrc/afr_common.h: afr_hash32 / afr_keep); replaces the reference's
                     torch `bernoulli_` stream (model.py:137,144,149), which no GPU can replay
"""
import numpy as np

SEED = 42
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def splitmix64(x):
    """splitmix64 finaliser on a uint64 array (wrap-around arithmetic)."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def _counter(tensor_id, n, seed, lane=0):
    base = (np.uint64(tensor_id) << np.uint64(40)) ^ (np.uint64(seed) << np.uint64(24)) ^ (np.uint64(lane) << np.uint64(60))
    with np.errstate(over="ignore"):
        return splitmix64(base + np.arange(n, dtype=np.uint64))


def hash_u01(tensor_id, n, seed=SEED, lane=0):
    """n doubles in [0,1): top 53 bits of the hash."""
    return (_counter(tensor_id, n, seed, lane) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def hash_uniform(tensor_id, shape, bound, seed=SEED):
    n = int(np.prod(shape))
    return ((2.0 * hash_u01(tensor_id, n, seed) - 1.0) * bound).astype(np.float32).reshape(shape)


def hash_normal(tensor_id, shape, std, seed=SEED):
    n = int(np.prod(shape))
    u1 = hash_u01(tensor_id, n, seed, lane=0)
    u2 = hash_u01(tensor_id, n, seed, lane=1)
    z = np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)
    return (z * std).astype(np.float32).reshape(shape)


def hash_u8(tensor_id, shape, seed=SEED):
    n = int(np.prod(shape))
    return (_counter(tensor_id, n, seed) >> np.uint64(56)).astype(np.uint8).reshape(shape)


# ---------------------------------------------------------------- text (generate_font.ts:164-199)
def _lcg_walk(seed, min_length, max_length, letter):
    """The walk the three text sources share (and csrc/dataset.hip's text_walk restates): the LCG state from the seed, the length, then
    words of 1..10 letters with a space between them until the length is used up.  draw(k) is (state * k) >> 32 after one LCG update --
    int(rnd() * k) of generate_font.ts, exact in integers; letter(draw, prev) -> the code of a word's next letter, prev the code before
    it in the word (None at its start)."""
    state = int(seed) % 4294967296

    def draw(k):
        nonlocal state
        state = (state * 1664525 + 1013904223) % 4294967296
        return (state * k) >> 32

    remaining = draw(max_length - min_length + 1) + min_length
    out = []
    while remaining > 0:
        wl = min(draw(10) + 1, remaining)
        prev = None
        for _ in range(wl):
            prev = letter(draw, prev)
            out.append(chr(prev))
        remaining -= wl
        if remaining > 0:
            out.append(" ")
            remaining -= 1
    return "".join(out)


def lcg_text(seed, min_length=10, max_length=100):
    return _lcg_walk(seed, min_length, max_length, lambda draw, prev: 65 + draw(26))


# ---------------------------------------------------------------- weighted text (afr_op_dataset_text_w, afr_op_text_weights)
TEXT_FIRST, TEXT_CODES = 33, 94          # the drawable codes 33..126: every printable ASCII character but the space
REL_ONE, REL_CAP = 1 << 16, 16 << 16     # a character's error relative to the mean in 16.16 fixed point, and its cap
_ALPHABETS = {
    "upper": range(65, 91),
    "lower": range(97, 123),
    "letters": (*range(65, 91), *range(97, 123)),
    "alnum": (*range(48, 58), *range(65, 91), *range(97, 123)),
    "ascii": range(TEXT_FIRST, TEXT_FIRST + TEXT_CODES),
}


def alphabet_members(spec):
    """The 94 flags (0 / 1, flag i = code 33 + i) of an alphabet: one of the names upper, lower, letters, alnum, ascii, or -- any other
    string -- the literal set of its characters.  A literal that is empty or holds a space or a code outside 33..126 is a ValueError."""
    if not isinstance(spec, str):
        raise ValueError(f"an alphabet is a name ({', '.join(_ALPHABETS)}) or a string of characters, got {spec!r}")
    codes = _ALPHABETS.get(spec)
    if codes is None:
        codes = [ord(c) for c in spec]
        bad = sorted({c for c in codes if not TEXT_FIRST <= c < TEXT_FIRST + TEXT_CODES})
        if bad or not codes:
            raise ValueError(f"alphabet {spec!r}: " + ("empty" if not codes else
                             f"codes {bad} lie outside {TEXT_FIRST}..{TEXT_FIRST + TEXT_CODES - 1} (the space separates words and is never drawn as a letter)"))
    flags = [0] * TEXT_CODES
    for c in codes:
        flags[c - TEXT_FIRST] = 1
    return flags


def members_words(members):
    """The 94 flags as the three 32-bit words afr_op_text_weights takes: bit i of the mask = code 33 + i."""
    if len(members) != TEXT_CODES:
        raise ValueError(f"{len(members)} member flags, expected {TEXT_CODES}")
    mask = sum(1 << i for i, m in enumerate(members) if m)
    return [(mask >> (32 * k)) & 0xFFFFFFFF for k in range(3)]


def text_weights(by_code, members, floor_w, gain):
    """Twin of afr_op_text_weights in Python integers -> (cum, w), two lists of 94.  by_code: rows [code] = {chars, pixels, sumsq, ...}
    (afr_op_sheet_char_errors' table; only columns 1 and 2 of the member codes are read) or None; members: the 94 flags."""
    if len(members) != TEXT_CODES or not any(members):
        raise ValueError("members: 94 flags, at least one set")
    if not 1 <= floor_w <= 65535 or not 0 <= gain <= 65535:
        raise ValueError(f"floor_w {floor_w} must lie in 1..65535, gain {gain} in 0..65535")
    A = [TEXT_FIRST + i for i in range(TEXT_CODES) if members[i]]
    P = S = 0
    if by_code is not None:
        P, S = sum(int(by_code[c][1]) for c in A), sum(int(by_code[c][2]) for c in A)
    w = [0] * TEXT_CODES
    if by_code is None or gain == 0 or S == 0:
        for c in A:
            w[c - TEXT_FIRST] = floor_w
    else:
        k = max(0, S.bit_length() - 47)
        m_ref = max(1, ((S >> k) << 16) // max(1, P >> k))
        for c in A:
            pixels, sumsq = int(by_code[c][1]) >> k, int(by_code[c][2]) >> k
            rel = REL_ONE if pixels == 0 else min((((sumsq << 16) // pixels) << 16) // m_ref, REL_CAP)
            w[c - TEXT_FIRST] = floor_w + ((gain * rel) >> 16)
    cum, total = [], 0
    for x in w:
        total += x
        cum.append(total)
    return cum, w


def lcg_text_weighted(seed, cum, min_length=10, max_length=100):
    """Twin of afr_op_dataset_text_w: lcg_text with the letter drawn from the 94 inclusive cumulative weights `cum` -- r = (state *
    cum[93]) >> 32 after the same LCG update, the letter 33 + (the smallest i with cum[i] > r).  A zero total is a ValueError."""
    import bisect
    cum = [int(c) for c in cum]
    total = cum[-1]
    if len(cum) != TEXT_CODES or total == 0:
        raise ValueError("cum: 94 inclusive cumulative weights with a positive total")
    return _lcg_walk(seed, min_length, max_length, lambda draw, prev: TEXT_FIRST + bisect.bisect_right(cum, draw(total)))


# ---------------------------------------------------------------- Markov text (afr_op_dataset_text_m, afr_op_pair_weights)
TEXT_CONTEXTS = TEXT_CODES + 1           # row 0: the start of a word; row 1 + i: after code 33 + i


def pair_table(w2):
    """Any 95 x 94 table of non-negative integer weights (w2[context][letter]) -> cum2, the 95 lists of inclusive cumulative weights
    afr_op_dataset_text_m draws from.  A negative weight, another shape, or a row total above 2^32 - 1 is a ValueError."""
    rows = [[int(x) for x in row] for row in w2]
    if len(rows) != TEXT_CONTEXTS or any(len(row) != TEXT_CODES for row in rows):
        raise ValueError(f"w2: {TEXT_CONTEXTS} rows of {TEXT_CODES} weights")
    cum2 = []
    for r, row in enumerate(rows):
        total, cum = 0, []
        for x in row:
            if x < 0:
                raise ValueError(f"w2: a negative weight in row {r}")
            total += x
            cum.append(total)
        if total > 0xFFFFFFFF:
            raise ValueError(f"w2: row {r} sums to {total}, above 2^32 - 1")
        cum2.append(cum)
    return cum2


def pair_weights(by_pair, members, floor_w, gain, min_chars):
    """Twin of afr_op_pair_weights in Python integers -> (cum2, w2), two lists of 95 lists of 94.  by_pair: [context][letter] =
    {chars, pixels, sumsq, wrong} (afr_op_pair_errors' table; only the records of live pairs are read) or None; members: the 94 flags."""
    if len(members) != TEXT_CODES or not any(members):
        raise ValueError("members: 94 flags, at least one set")
    if not 1 <= floor_w <= 65535 or not 0 <= gain <= 65535:
        raise ValueError(f"floor_w {floor_w} must lie in 1..65535, gain {gain} in 0..65535")
    if min_chars < 0:
        raise ValueError(f"min_chars {min_chars} must not be negative")
    letters = [i for i in range(TEXT_CODES) if members[i]]
    live = [(p, c) for p in [0] + [1 + i for i in letters] for c in letters]
    P = S = 0
    if by_pair is not None and gain:
        P, S = sum(int(by_pair[p][c][1]) for p, c in live), sum(int(by_pair[p][c][2]) for p, c in live)
    w2 = [[0] * TEXT_CODES for _ in range(TEXT_CONTEXTS)]
    if S == 0:
        for p, c in live:
            w2[p][c] = floor_w
    else:
        k = max(0, S.bit_length() - 47)
        m_ref = max(1, ((S >> k) << 16) // max(1, P >> k))
        for p, c in live:
            chars, pixels, sumsq = int(by_pair[p][c][0]), int(by_pair[p][c][1]) >> k, int(by_pair[p][c][2]) >> k
            rel = REL_ONE if pixels == 0 or chars < min_chars else min((((sumsq << 16) // pixels) << 16) // m_ref, REL_CAP)
            w2[p][c] = floor_w + ((gain * rel) >> 16)
    return pair_table(w2), w2


def lcg_text_markov(seed, cum2, min_length=10, max_length=100):
    """Twin of afr_op_dataset_text_m: lcg_text_weighted with one row of cumulative weights per context -- cum2[0] at the start of every
    word, cum2[1 + i] after letter i.  Reaching a row whose total is 0 is a ValueError (the device zero-fills the sample and flags it)."""
    import bisect
    cum2 = [[int(c) for c in row] for row in cum2]
    if len(cum2) != TEXT_CONTEXTS or any(len(row) != TEXT_CODES for row in cum2):
        raise ValueError(f"cum2: {TEXT_CONTEXTS} rows of {TEXT_CODES} inclusive cumulative weights")

    def letter(draw, prev):
        ctx = 0 if prev is None else 1 + prev - TEXT_FIRST
        row = cum2[ctx]
        if row[-1] == 0:
            raise ValueError(f"cum2: the text of seed {seed} reaches context {ctx}, whose total weight is 0")
        return TEXT_FIRST + bisect.bisect_right(row, draw(row[-1]))

    return _lcg_walk(seed, min_length, max_length, letter)


def dataset_strings(n, first_seed=42):
    """Sample i (0-based) of the reference dataset uses seed i+42 (generate_font.ts:204)."""
    return [lcg_text(first_seed + i) for i in range(n)]


def encode_strings(strings, max_length):
    """ord() codes, truncated to max_length and zero padded (helpers.py:52-59,164-173)."""
    x = np.zeros((len(strings), max_length), dtype=np.int64)
    for i, s in enumerate(strings):
        codes = [ord(c) for c in s[:max_length]]
        x[i, :len(codes)] = codes
    return x


def synth_sheet_targets(n, height, width, tensor_id=900, seed=SEED, dark_fraction=0.12):
    """uint8 [n,h,w]: white (255) background, ~12 % hashed anti-aliased dark pixels."""
    cnt = n * height * width
    u = hash_u01(tensor_id, cnt, seed, lane=0)
    shade = hash_u8(tensor_id, (cnt,), seed ^ 0x5A5A)
    t = np.where(u < dark_fraction, shade, np.uint8(255)).astype(np.uint8)
    return t.reshape(n, height, width)


# ---------------------------------------------------------------- dropout counter hash (device twin)
STREAM_EMBED, STREAM_ATTN, STREAM_FC = 1, 2, 3


def dropout_key(seed, step, stream, rank=0):
    """32-bit key for one (seed, step, tensor stream, rank); host side of afr_keep()."""
    v = (int(seed) & 0xFFFFFFFFFFFFFFFF) ^ ((int(step) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)
    v ^= (int(stream) * 0xC2B2AE3D27D4EB4F) & 0xFFFFFFFFFFFFFFFF
    v ^= (int(rank) * 0x165667B19E3779F9) & 0xFFFFFFFFFFFFFFFF
    return int(splitmix64(np.array([v], dtype=np.uint64))[0]) & 0xFFFFFFFF


def keep_threshold(keep_prob):
    return int(float(keep_prob) * 16777216.0)


def dropout_keep_mask(key, n, keep_prob, offset=0):
    """Boolean keep mask for flat element indices offset..offset+n-1 (bit-exact twin of afr_keep)."""
    idx = np.arange(offset, offset + n, dtype=np.uint64)
    lo = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    hi = (idx >> np.uint64(32)).astype(np.uint32)
    with np.errstate(over="ignore"):
        k = np.uint32(key) + hi * np.uint32(0x85EBCA6B)
        h = lo * np.uint32(0x9E3779B1) + k
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x21F0AAAD)
        h ^= h >> np.uint32(15)
        h *= np.uint32(0x735A2D97)
        h ^= h >> np.uint32(15)
    return (h >> np.uint32(8)) < np.uint32(keep_threshold(keep_prob))


# ---------------------------------------------------------------- formula-generated parameters
def make_params(cfg, seed=SEED):
    """dict name -> float32 array for every tensor of cfg.param_shapes(), from the counter hash.
    Ranges follow the reference's default initialisers but biases / LayerNorm
    affine are made non-trivial so that parity tests exercise them."""
    out = {}
    for tid, (name, shape) in enumerate(cfg.param_shapes()):
        if name == "positional_encoding":
            a = hash_normal(tid, shape, 0.02, seed)                 # model.py:141
        elif name in ("embedding.weight", "font_embedding.weight"):
            a = hash_normal(tid, shape, 1.0, seed)                  # nn.Embedding default N(0,1)
        elif name.endswith("in_proj_weight"):
            a = hash_uniform(tid, shape, float(np.sqrt(6.0 / (shape[0] + shape[1]))), seed)
        elif name == "layer_norm.weight" or (len(shape) == 1 and name.split(".")[-2][:2] == "ln" and name.endswith(".weight")):
            a = 1.0 + hash_uniform(tid, shape, 0.1, seed)
        elif name == "layer_norm.bias" or (len(shape) == 1 and name.split(".")[-2][:2] == "ln" and name.endswith(".bias")):
            a = hash_uniform(tid, shape, 0.1, seed)
        elif name.endswith(".weight"):
            a = hash_uniform(tid, shape, float(1.0 / np.sqrt(shape[1])), seed)   # kaiming_uniform(a=sqrt5)
        elif name.endswith("in_proj_bias") or name.endswith("out_proj.bias"):
            a = hash_uniform(tid, shape, 0.05, seed)
        else:  # Linear biases: U(+-1/sqrt(fan_in)); fan_in is the matching weight's 2nd dim
            wshape = dict(cfg.param_shapes())[name[:-4] + "weight"]
            a = hash_uniform(tid, shape, float(1.0 / np.sqrt(wshape[1])), seed)
        out[name] = a.astype(np.float32)
    return out


def sheet_dropout_masks(cfg, B, L, seed, step, rank=0):
    """The three keep masks (uint8 0/1) exactly as the HIP kernels derive them."""
    E, H, F = cfg.embed_dim, cfg.heads, cfg.fc_dim

    def keep(p):
        # the keep probability as the kernels form it, in float32 from the float32 rate (afr_api.hip sheet_drop): for p = 0.2 that is
        # 13421773 / 2^24, one threshold step above the double 0.8 -- the element whose hash is 13421772 is KEPT
        return float(np.float32(1.0) - np.float32(p))
    me = dropout_keep_mask(dropout_key(seed, step, STREAM_EMBED, rank), B * L * E, keep(cfg.p_embed))
    ma = dropout_keep_mask(dropout_key(seed, step, STREAM_ATTN, rank), B * H * L * L, keep(cfg.p_attn))
    mf = dropout_keep_mask(dropout_key(seed, step, STREAM_FC, rank), B * L * F, keep(cfg.p_fc))
    return dict(embed=me.reshape(B, L, E).astype(np.uint8), attn=ma.reshape(B, H, L, L).astype(np.uint8),
                fc=mf.reshape(B, L, F).astype(np.uint8))


# ---------------------------------------------------------------- rasterised glyph targets (BASELINE C1-C4)
_GLYPH_FIXTURE = None


def glyph_bitmap_targets(size, x, font=None):
    """uint8 [B, size, size] targets for codes x (32..126) and font ids: the FreeType rasterisations of FiraCode-Retina
    (16x16; font 0 of 32x32) and Montserrat-Regular (font 1 of 32x32) that tests/golden/make_golden.py drew with
    datagen.render_glyphs from the reference's two TTFs.  None when the fixture file is not there or holds no such size."""
    global _GLYPH_FIXTURE
    import os
    if _GLYPH_FIXTURE is None:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "glyph_bitmaps.npz")
        _GLYPH_FIXTURE = dict(np.load(path)) if os.path.exists(path) else {}
    x = np.asarray(x, dtype=np.int64)
    if size == 16 and "fira16" in _GLYPH_FIXTURE:
        return _GLYPH_FIXTURE["fira16"][x - 32]
    if size == 32 and "fira_mont32" in _GLYPH_FIXTURE:
        f = np.zeros_like(x) if font is None else np.asarray(font, dtype=np.int64)
        return _GLYPH_FIXTURE["fira_mont32"][f, x - 32]
    return None
