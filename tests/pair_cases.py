"""The hand-computed pair tables that tests/test_pair_cpu.py checks synth.pair_weights against and tests/test_gpu_pair.py runs through
afr_op_pair_weights, in the manner of tests/text_cases.py.  A case: (name, {(context, code): (chars, pixels, sumsq)}, the alphabet,
floor_w, gain, min_chars, {(context, code): expected weight}).  A context is None (the start of a word, row 0) or the code before; pairs
not named have zero counters, live pairs not named in the expectation weigh `rest` (the entry under the key "rest")."""
import numpy as np

HUGE = (1 << 63) - 1

TABLE_CASES = [
    # one live pair: the alphabet is A and the only context is the word start.  (A, A) is live too: zero counters, rel = 1 << 16.
    # P = 100, S = 5000: m_ref = 50 << 16, rel = 1 << 16, w = 10 + 100 for both
    ("one letter", {(None, 65): (9, 100, 5000)}, "A", 10, 100, 0, {"rest": 110}),
    # a live pair with pixels == 0 counts as average: P = 100, S = 1000, m_ref = 10 << 16; (None, A) is the whole mean
    ("pixels == 0", {(None, 65): (3, 100, 1000), (65, 66): (7, 0, 0)}, "AB", 5, 3, 0, {"rest": 8}),
    # chars just below and exactly at min_chars = 8: P = 20, S = 4000, m_ref = 200 << 16.  (A, B) has mean 300 = 3/2 of it, but 7
    # chars: average, 1000 + 2000.  (B, A) has mean 100 = 1/2 with exactly 8 chars: 1000 + 1000.
    ("chars below and at min_chars", {(65, 66): (7, 10, 3000), (66, 65): (8, 10, 1000)}, "AB", 1000, 2000, 8,
     {(66, 65): 2000, "rest": 3000}),
    # ... the same counters with min_chars = 7: both count.  rel(A, B) = 3/2: 1000 + 3000
    ("chars at min_chars on both", {(65, 66): (7, 10, 3000), (66, 65): (8, 10, 1000)}, "AB", 1000, 2000, 7,
     {(65, 66): 4000, (66, 65): 2000, "rest": 3000}),
    # S == 0: every live pair weighs floor_w whatever gain is
    ("S == 0", {(None, 65): (50, 50, 0), (65, 66): (70, 70, 0)}, "AB", 7, 65535, 0, {"rest": 7}),
    # records of pairs that are not live are never read: a non-member letter, a non-member context, both
    ("non-live records with huge counters", {(65, 66): (9, 10, 1000), (66, 65): (9, 10, 3000), (65, 67): (HUGE, HUGE, HUGE),
                                             (67, 65): (HUGE, HUGE, HUGE), (None, 33): (HUGE, HUGE, HUGE), (126, 126): (HUGE, HUGE, HUGE),
                                             (97, 66): (1, 1, HUGE)}, "AB", 1000, 2000, 0,
     {(65, 66): 2000, (66, 65): 4000, "rest": 3000}),
    # S = 2^52: k = 6.  Shifted: pixels 2^34 (the low 63 of the first are dropped), sumsq 2^44 and 3 * 2^44, P = 2^35, S = 2^46,
    # m_ref = 2^27, rel = ((2^60 / 2^34) << 16) / 2^27 = 2^15 and 3 * 2^15; chars is NOT shifted: 8 >= min_chars = 8
    ("counters that force k > 0", {(None, 65): (8, (1 << 40) + 63, 1 << 50), (65, 66): (8, 1 << 40, 3 << 50)}, "AB", 4096, 4096, 8,
     {(None, 65): 6144, (65, 66): 10240, "rest": 8192}),
    # ... a pair whose pixels shift to 0 (63 >> 6) counts as average although it was seen; P = 2^41 + 63 and S = 2^52 + 63 shift as above
    ("pixels that shift to 0", {(None, 65): (8, 1 << 40, 1 << 50), (65, 66): (8, 1 << 40, 3 << 50), (66, 66): (99, 63, 63)}, "AB",
     4096, 4096, 8, {(None, 65): 6144, (65, 66): 10240, "rest": 8192}),
    # P = 1000, S = 2000: m_ref = 2 << 16; rel = 1/2; the other pair's mean is 101, 50.5 times the table's: capped at 16
    ("the 16x cap", {(None, 65): (1, 990, 990), (65, 65): (1, 10, 1010)}, "A", 100, 1000, 0, {(None, 65): 600, (65, 65): 16100}),
    # exactly 16 times the mean is the cap's own value: P = 31, S = 62 (mean 2), the other pair's mean 32
    ("exactly 16 times the mean", {(None, 65): (1, 30, 30), (65, 65): (1, 1, 32)}, "A", 1, 10, 0, {(None, 65): 6, (65, 65): 161}),
    # q << 16 passes 64 bits: P = 2, S = 2^46 + 12345, m_ref = 2^61 + 12345 * 2^15; q = 2^61 -> rel = floor(2^77 / m_ref) = 65535,
    # q' = 2^61 + 12345 * 2^16 -> rel = 65536; w = 1 + (65535 * 65535 >> 16) = 65535 and 1 + 65535
    ("a quotient whose << 16 passes 64 bits", {(None, 65): (1, 1, 1 << 45), (65, 65): (1, 1, (1 << 45) + 12345)}, "A", 1, 65535, 0,
     {(None, 65): 65535, (65, 65): 65536}),
    # gain == 0 and a NULL table: floor_w over a scattered alphabet that touches every word edge of the mask
    ("gain == 0", {(None, 33): (5, 5, 500), (126, 126): (5, 5, 5)}, "!@A`a~", 9, 0, 0, {"rest": 9}),
    ("no table", None, "!@A`a~", 65535, 65535, 3, {"rest": 65535}),
]


def _row(ctx):
    return 0 if ctx is None else 1 + ctx - 33


def by_pair_array(counters):
    """{(context, code): (chars, pixels, sumsq)} -> uint64 [95][94][4] as afr_op_pair_errors lays it out; the column that is not
    read (wrong) holds a large value"""
    if counters is None:
        return None
    by = np.zeros((95, 94, 4), dtype=np.uint64)
    by[:, :, 3] = HUGE
    for (ctx, code), (chars, pixels, sumsq) in counters.items():
        by[_row(ctx), code - 33, :3] = chars, pixels, sumsq
    return by


def expected(want, alphabet_codes):
    """{(context, code): weight, "rest": weight} over the alphabet's codes -> (cum2, w2), two lists of 95 lists of 94"""
    w2 = [[0] * 94 for _ in range(95)]
    for ctx in [None] + list(alphabet_codes):
        for code in alphabet_codes:
            w2[_row(ctx)][code - 33] = want[(ctx, code)] if (ctx, code) in want else want["rest"]
    return [np.cumsum(np.array(row, dtype=np.int64)).tolist() for row in w2], w2
