"""The hand-computed letter tables that tests/test_text_cpu.py checks synth.text_weights against and tests/test_gpu_text.py runs through
afr_op_text_weights, and the committed steering table of the statistical check.  A case: (name, {code: (pixels, sumsq)}, the alphabet,
floor_w, gain, {code: expected weight}); codes not named have zero counters, members not named in the expectation are a fault."""
import numpy as np

N_CODES = 127
HUGE = (1 << 63) - 1

TABLE_CASES = [
    # P = 100, S = 5000: m_ref = 50 << 16, rel = 1 << 16, w = 10 + 100
    ("one member", {65: (100, 5000)}, "A", 10, 100, {65: 110}),
    # B was never seen: rel_B = 1 << 16; A is the whole mean, rel_A = 1 << 16
    ("a member with pixels == 0", {65: (100, 1000)}, "AB", 5, 3, {65: 8, 66: 8}),
    # S == 0: every member weighs floor_w whatever gain is
    ("S == 0", {65: (50, 0), 66: (70, 0)}, "AB", 7, 65535, {65: 7, 66: 7}),
    # by-code counters of non-members are never read: P = 20, S = 4000, m_ref = 200 << 16, rel_A = 1/2, rel_B = 3/2
    ("non-members with huge counters", {65: (10, 1000), 66: (10, 3000), 67: (1 << 62, HUGE), 33: (HUGE, HUGE), 126: (HUGE, 1), 97: (1, HUGE)}, "AB",
     1000, 2000, {65: 2000, 66: 4000}),
    # S = 2^52: k = 6.  Shifted: pixels 2^34 (the low 63 of A's are dropped), sumsq 2^44 and 3 * 2^44, P = 2^35, S = 2^46, m_ref = 2^27,
    # rel_A = ((2^60 / 2^34) << 16) / 2^27 = 2^15, rel_B = 3 * 2^15
    ("counters that force k > 0", {65: ((1 << 40) + 63, 1 << 50), 66: (1 << 40, 3 << 50)}, "AB", 4096, 4096, {65: 6144, 66: 10240}),
    # P = 1000, S = 2000: m_ref = 2 << 16; rel_A = 1/2; B's mean is 101, 50.5 times the alphabet's: capped at 16
    ("the 16x cap", {65: (990, 990), 66: (10, 1010)}, "AB", 100, 1000, {65: 600, 66: 16100}),
    # exactly 16 times the mean is the cap's own value: P = 31, S = 62 (mean 2), B's mean 32
    ("exactly 16 times the mean", {65: (30, 30), 66: (1, 32)}, "AB", 1, 10, {65: 6, 66: 161}),
    # q << 16 passes 64 bits: P = 2, S = 2^46 + 12345, m_ref = 2^61 + 12345 * 2^15; q_A = 2^61 -> rel_A = floor(2^77 / m_ref) = 65535,
    # q_B = 2^61 + 12345 * 2^16 -> rel_B = 65536; w_A = 1 + (65535 * 65535 >> 16) = 65535, w_B = 1 + 65535
    ("a quotient whose << 16 passes 64 bits", {65: (1, 1 << 45), 66: (1, (1 << 45) + 12345)}, "AB", 1, 65535, {65: 65535, 66: 65536}),
    # gain == 0 and a NULL table: floor_w over a scattered alphabet that touches every word edge of the mask
    ("gain == 0", {33: (5, 500), 126: (5, 5)}, "!@A`a~", 9, 0, {33: 9, 64: 9, 65: 9, 96: 9, 97: 9, 126: 9}),
    ("no table", None, "!@A`a~", 65535, 65535, {33: 65535, 64: 65535, 65: 65535, 96: 65535, 97: 65535, 126: 65535}),
]


def by_code_array(counters, n_codes=N_CODES):
    """{code: (pixels, sumsq)} -> uint64 [n_codes + 1][5] as afr_op_sheet_char_errors lays it out; the columns that are not read (chars,
    off2, wrong) and the background row hold large values"""
    if counters is None:
        return None
    by = np.zeros((n_codes + 1, 5), dtype=np.uint64)
    by[:, 0] = by[:, 3] = by[:, 4] = HUGE
    by[n_codes, 1:3] = HUGE
    for code, (pixels, sumsq) in counters.items():
        by[code, 1], by[code, 2] = pixels, sumsq
    return by


def expected(want):
    """{code: weight} -> (cum, w), two lists of 94"""
    w = [want.get(33 + i, 0) for i in range(94)]
    return list(np.cumsum(np.array(w, dtype=np.int64)).tolist()), w


def steer_table():
    """The committed table of the statistical check: A-Z with pixel counts of 2 000..12 000 and mean squared errors of 40..430, W at
    6 000 -- some fifteen times the rest.  uint64 [128][5]."""
    counters = {}
    for c in range(65, 91):
        pixels = 2000 + 397 * ((c * c) % 26)
        mean = 6000 if c == ord("W") else 40 + (c * 7919) % 391
        counters[c] = (pixels, pixels * mean)
    return by_code_array(counters)
