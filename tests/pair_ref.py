"""The twins of the pair tables (include/afr.h: afr_op_pair_errors, afr_op_dataset_text_m, afr_op_pair_weights): a numpy pair_errors
written from the contract, synth's two twins by name, the tables the CPU and GPU tests share, and planted faults -- one reading of the
contract gone wrong each -- that tests/test_pair_cpu.py shows to differ on the very inputs tests/test_gpu_pair.py launches.  Integers
only.  Nothing here needs a GPU."""
import numpy as np

from .util import synth

FIRST, CODES, CONTEXTS = 33, 94, 95
lcg_text_markov, pair_weights, pair_table = synth.lcg_text_markov, synth.pair_weights, synth.pair_table

FAULTS = ("context_from_next", "pos0_reads_previous_row", "chars_without_pixels")
TEXT_FAULTS = ("no_reset_at_word_start",)


def _letter(c):
    return FIRST <= c < FIRST + CODES


def pair_errors(codes, per_pos, rows=None, by_pair=None, fault=None):
    """codes int64 [N][ldx], per_pos [n][ldx + 1][4] = {pixels, sumsq, off2, wrong}, rows (or None) the row of codes each sample reads
    -> uint64 [95][94][4] = {chars, pixels, sumsq, wrong}, added to by_pair when one is given (Python integers underneath: no sum
    wraps unseen).  fault: one of FAULTS."""
    codes, per_pos = np.asarray(codes, dtype=np.int64), np.asarray(per_pos).astype(np.uint64)
    n, ldx = per_pos.shape[0], codes.shape[1]
    assert per_pos.shape == (n, ldx + 1, 4)
    flat = codes.reshape(-1)
    table = [[[0, 0, 0, 0] for _ in range(CODES)] for _ in range(CONTEXTS)]
    for j in range(n):
        r = j if rows is None else int(rows[j])
        for i in range(ldx):
            c, (pixels, sumsq, _, wrong) = int(codes[r, i]), (int(v) for v in per_pos[j, i])
            if not _letter(c) or (pixels == 0 and fault != "chars_without_pixels"):
                continue
            if fault == "context_from_next":
                p = int(codes[r, i + 1]) if i + 1 < ldx else 0
            elif i == 0:
                p = int(flat[r * ldx - 1]) if fault == "pos0_reads_previous_row" and r > 0 else 0
            else:
                p = int(codes[r, i - 1])
            rec = table[1 + p - FIRST if _letter(p) else 0][c - FIRST]
            for f, v in enumerate((1, pixels, sumsq, wrong)):
                rec[f] += v
    out = np.zeros((CONTEXTS, CODES, 4), dtype=np.uint64) if by_pair is None else np.array(by_pair, dtype=np.uint64)
    for p in range(CONTEXTS):
        for c in range(CODES):
            for f in range(4):
                total = int(out[p, c, f]) + table[p][c][f]
                assert total < 1 << 64
                out[p, c, f] = total
    return out


def markov_no_reset(seed, cum2, min_length=10, max_length=100):
    """lcg_text_markov with the planted fault of TEXT_FAULTS: the context is carried over the space instead of starting at row 0"""
    import bisect
    state = int(seed) % 4294967296

    def draw(k):
        nonlocal state
        state = (state * 1664525 + 1013904223) % 4294967296
        return (state * k) >> 32

    remaining = draw(max_length - min_length + 1) + min_length
    out, ctx = [], 0
    while remaining > 0:
        wl = min(draw(10) + 1, remaining)
        for _ in range(wl):
            row = [int(c) for c in cum2[ctx]]
            i = bisect.bisect_right(row, draw(row[-1]))
            out.append(chr(FIRST + i))
            ctx = 1 + i
        remaining -= wl
        if remaining > 0:
            out.append(" ")
            remaining -= 1
    return "".join(out)


# ---------------------------------------------------------------- tables
def rank_one(w):
    """the 95 x 94 weights whose every row is w: the Markov source then draws what the weighted source draws from cumsum(w)"""
    return [list(w) for _ in range(CONTEXTS)]


def chain_table():
    """words start with A, after A always B, after B always A; every other row is zero and never reached"""
    w2 = [[0] * CODES for _ in range(CONTEXTS)]
    a, b = ord("A") - FIRST, ord("B") - FIRST
    w2[0][a], w2[1 + a][b], w2[1 + b][a] = 3, 1, 2
    return w2


def chain_text(s):
    """what the chain table makes of the text s of any other source: the same lengths and spaces, ABAB... in every word"""
    return " ".join(("AB" * len(word))[:len(word)] for word in s.split(" "))


def run_table(factor):
    """A-Z, every live pair at weight 4096, the diagonal (after a letter, the same letter again) multiplied by factor"""
    members = synth.alphabet_members("upper")
    w2 = [[0] * CODES for _ in range(CONTEXTS)]
    for p in [0] + [1 + i for i in range(CODES) if members[i]]:
        for c in range(CODES):
            if members[c]:
                w2[p][c] = 4096 * (factor if p == c + 1 else 1)
    return w2


def longest_run(s):
    best = run = 0
    prev = None
    for ch in s:
        run = run + 1 if ch == prev and ch != " " else 1
        prev = ch
        if ch != " ":
            best = max(best, run)
    return best


# ---------------------------------------------------------------- the inputs of the pair_errors tests (CPU faults, GPU launches)
def synthetic_case(n, ldx, seed=0, n_rows=None, dirty=True):
    """(codes int64 [n_rows][ldx], per_pos uint32 [n][ldx + 1][4]): texts of letters, spaces, codes 0..31 and 127..140 as characters and
    predecessors, a 0 that ends the text with (dirty) further codes behind it whose records are zero as afr_op_sheet_char_errors
    leaves them, records with pixels == 0 inside the text, and a letter at the end of every row and at position 0 of the next."""
    rng = np.random.default_rng(1000 * n + ldx + seed)
    n_rows = n if n_rows is None else n_rows
    pool = np.array([32, 32, 65, 65, 66, 87, 87, 87, 33, 126, 0, 5, 31, 127, 140, 90], dtype=np.int64)
    codes = pool[rng.integers(0, len(pool), size=(n_rows, ldx))]
    codes[:, -1] = 87                                                   # a letter where the next row's position 0 would look back
    codes[:, 0] = np.where(rng.integers(0, 2, n_rows) == 1, 87, codes[:, 0])
    per_pos = rng.integers(0, 5000, size=(n, ldx + 1, 4)).astype(np.uint32)
    per_pos[:, :, 0] = np.where(rng.integers(0, 4, size=(n, ldx + 1)) == 0, 0, per_pos[:, :, 0])      # a quarter own no pixel
    per_pos[per_pos[:, :, 0] == 0] = 0
    if dirty and ldx > 1:
        for j, end in enumerate(rng.integers(ldx // 2, ldx + 1, size=n)):   # behind the text: the codes stay dirty, the records are zero
            per_pos[j, end:ldx] = 0
    return codes, per_pos
