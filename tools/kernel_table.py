#!/usr/bin/env python3
"""Per-kernel resource and instruction table of libafr's device code, and the comparison of two such tables.

    python tools/kernel_table.py make [CSRC_DIR] > table.tsv     # device-only compile of every .hip (gfx950), no GPU needed
    python tools/kernel_table.py diff parent.tsv branch.tsv      # symbols, resources, instruction sequences

Columns: file, kernel symbol, VGPRs, AGPRs, scratch bytes/lane, LDS bytes/block, occupancy, instruction count, and three
digests: of the instruction text (opcode and operands, in order), of the opcode sequence, of the opcode histogram, and of the
histogram without the scalar unit's instructions (s_*, and v_readlane / v_writelane: SGPR spills).
"""
import collections, concurrent.futures, hashlib, os, re, subprocess, sys, tempfile

FILES = ["gemm", "elementwise", "glyph_fused", "pixel", "sheet", "dataset"]      # a tree that lacks one of them (an older commit) is tabled without it
FLAGS = "--offload-arch=gfx950 -O3 -fPIC -std=c++17 --cuda-device-only -S -Rpass-analysis=kernel-resource-usage".split()
SCALAR = ("s_", "v_readlane_b32", "v_writelane_b32")       # scalar unit, and SGPR spills to lanes
REMARKS = {"VGPRs": "vgpr", "AGPRs": "agpr", "ScratchSize [bytes/lane]": "scratch", "LDS Size [bytes/block]": "lds",
           "Occupancy [waves/SIMD]": "occ"}


def digest(items):
    return hashlib.sha1("\n".join(items).encode()).hexdigest()[:12]


def one_file(csrc, name, tmp):
    asm = os.path.join(tmp, name + ".s")
    r = subprocess.run(["hipcc", *FLAGS, os.path.join(csrc, name + ".hip"), "-o", asm], capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr)
    res, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s*([A-Za-z /\[\]]+?): (\d+)) \[-Rpass", line)
        if m and m.group(1):
            cur = res.setdefault(m.group(1), {})
        elif m and cur is not None and m.group(2).strip() in REMARKS:
            cur[REMARKS[m.group(2).strip()]] = m.group(3)
    body, cur = {}, None
    for line in open(asm):
        m = re.match(r"(\w+):", line)
        if m and m.group(1) in res:
            cur = body.setdefault(m.group(1), [])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and line.startswith("\t") and not line.lstrip().startswith((".", ";")):
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(line.split(";")[0].split())))      # labels without the function's number
    rows = []
    for sym in res:
        ins = body[sym]
        ops = [i.split()[0] for i in ins]
        hist = ["%s %d" % kv for kv in sorted(collections.Counter(ops).items())]
        vhist = [h for h in hist if not h.startswith(SCALAR)]
        rows.append([name, sym] + [res[sym].get(k, "?") for k in REMARKS.values()] +
                    [str(len(ins)), digest(ins), digest(ops), digest(hist), digest(vhist)])
    return rows


def make(csrc):
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(len(FILES)) as ex:
        print("\t".join(["file", "kernel", *REMARKS.values(), "insts", "text", "opseq", "ophist", "vhist"]))
        for rows in ex.map(lambda f: one_file(csrc, f, tmp), [f for f in FILES if os.path.exists(os.path.join(csrc, f + ".hip"))]):
            for r in sorted(rows):
                print("\t".join(r))


def load(path):
    rows = [l.rstrip("\n").split("\t") for l in open(path)][1:]
    return {(r[0], r[1]): r[2:] for r in rows}


def diff(a, b):
    A, B = load(a), load(b)
    bad = 0
    for f in FILES:
        na, nb = [k for k in A if k[0] == f], [k for k in B if k[0] == f]
        print("%-12s %3d kernels in each" % (f, len(na)) if set(na) == set(nb) else
              "%-12s SYMBOLS DIFFER: %s" % (f, sorted(set(na) ^ set(nb))))
        bad += set(na) != set(nb)
    same = 0
    for k in sorted(set(A) & set(B)):
        x, y = A[k], B[k]
        if x[:5] != y[:5]:
            print("RESOURCES DIFFER %s %s: %s -> %s" % (*k, x[:5], y[:5])); bad += 1
        if x[6] == y[6]:
            same += 1
        elif x[8] != y[8]:
            print("OPCODE HISTOGRAM DIFFERS %s %s: %s -> %s instructions%s" %
                  (*k, x[5], y[5], " (scalar-unit instructions only)" if x[9] == y[9] else "")); bad += 1
        else:
            print("differs  %s %s: %s" % (*k, "operands (registers, labels) only" if x[7] == y[7] else "instruction order"))
    print("%d of %d kernels instruction for instruction identical; %d failures" % (same, len(set(A) & set(B)), bad))
    return bad


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "make":
        make(sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(__file__), "..", "ai-font-renderer_amd", "csrc"))
    elif len(sys.argv) == 4 and sys.argv[1] == "diff":
        sys.exit(1 if diff(sys.argv[2], sys.argv[3]) else 0)
    else:
        sys.exit(__doc__)
