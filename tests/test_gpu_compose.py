"""GPU: the device data set (csrc/dataset.hip) -- afr_op_dataset_text against synth.lcg_text, afr_op_compose_sheets against the sheets PIL
drew (tests/golden/atlas_sheets.npz) and against the numpy composer (tests/compose_ref.py), devdata.reference_dataset against the folder
datagen.generate writes, and the two CLI switches in miniature.  Everything is integers: every comparison is exact.  The op tests launch
into guarded buffers (tests/op_harness.py), twice, and compare the two launches bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from ai_font_renderer_amd import _lib
from . import compose_ref as R
from .gpu_util import dev, ptr, stream
from .op_harness import SENTINEL, Outs, twice
from .util import load, synth

pytestmark = pytest.mark.gpu

INK = 0x37                      # pre-load of sheet buffers: no byte the composer left out passes for paper (0xFF, the harness's fill)
CODE_FILL = int(np.array([SENTINEL, SENTINEL], dtype=np.int32).view(np.int64)[0])   # an int64 of the codes buffer nothing wrote: the harness
#                                 fills 32-bit words, so the codes are handed to it as pairs of them


@pytest.fixture(scope="module")
def fx():
    return dict(load("atlas_sheets.npz"))


def _atlas(fx, key):
    return {k: fx[f"{key}/{k}"] for k in ("cells", "adv64", "kern64", "origin_x", "origin_y")}


class DevAtlas:
    """an atlas's arrays on the device and the afr_glyph_atlas that points at them"""

    def __init__(self, A, kern=True):
        self.cells, self.adv = dev(A["cells"]), dev(A["adv64"])
        self.kern = dev(A["kern64"]) if kern and A.get("kern64") is not None else None
        n, h, w = A["cells"].shape
        self.struct = _lib.AfrGlyphAtlas(self.cells.data_ptr(), self.adv.data_ptr(), None if self.kern is None else self.kern.data_ptr(), n, h, w,
                                         int(A["origin_x"]), int(A["origin_y"]))


def _geo_struct(geo):
    g = _lib.AfrSheetGeometry(geo.height, geo.width, geo.wrap_width64, geo.n_lines)
    for i, b in enumerate(geo.baseline):
        g.baseline[i] = b
    return g


def compose(A, geo, codes, rows=None, n_rows=None, atlas=None):
    """afr_op_compose_sheets twice into a guarded, pre-inked buffer of n_rows sheets -> (uint8 [n_rows][H][W], the err word)"""
    atlas = atlas or DevAtlas(A)
    codes = np.ascontiguousarray(codes, dtype=np.int64)
    n, ldx = codes.shape
    n_rows = n if n_rows is None else n_rows
    cd, rd, g = dev(codes), None if rows is None else dev(np.asarray(rows, dtype=np.int64)), _geo_struct(geo)

    def launch():
        o = Outs()
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        out = o.new("sheets", (n_rows, geo.height, geo.width), torch.uint8, init=torch.full((n_rows * geo.height * geo.width,), INK, dtype=torch.uint8))
        _lib.check(_lib.lib().afr_op_compose_sheets(C.byref(atlas.struct), C.byref(g), ptr(cd), ldx, ptr(rd), n, out, ptr(err), stream()))
        return dict(o.finish(), err=int(err.cpu()))

    res = twice(launch)
    return res["sheets"].numpy(), res["err"]


def text(n, first_seed=42, seed_rows=None, rows=None, n_rows=None, ldx=100, lo=10, hi=100, want_len=True):
    """afr_op_dataset_text twice into guarded buffers -> (int64 [n_rows][ldx] codes, int32 [n_rows] lengths or None)"""
    n_rows = n if n_rows is None else n_rows
    sd = None if seed_rows is None else dev(np.asarray(seed_rows, dtype=np.int64))
    rd = None if rows is None else dev(np.asarray(rows, dtype=np.int64))

    def launch():
        o = Outs()
        codes = o.new("codes", (n_rows, 2 * ldx), torch.int32)
        ln = o.new("len", n_rows, torch.int32) if want_len else None
        _lib.check(_lib.lib().afr_op_dataset_text(first_seed, ptr(sd), ptr(rd), n, lo, hi, codes, ldx, ln, stream()))
        return o.finish(may_keep_fill=("len", "codes") if rows is not None else ())

    res = twice(launch)
    return res["codes"].numpy().view(np.int64), res["len"].numpy() if want_len else None


# ---------------------------------------------------------------------------------------------- text kernel
@pytest.mark.parametrize("n", [1, 64, 257])
def test_text_kernel_equals_lcg_text(n):
    strings = [synth.lcg_text(42 + i) for i in range(n)]
    codes, lens = text(n)
    assert np.array_equal(codes, synth.encode_strings(strings, 100))
    assert lens.tolist() == [len(s) for s in strings]
    # spread seeds through seed_rows and another first_seed, a wider row, no length output
    seeds = [7919 * s for s in range(n)]
    codes, lens = text(n, first_seed=43, seed_rows=seeds, ldx=104, want_len=False)
    assert lens is None and np.array_equal(codes, synth.encode_strings([synth.lcg_text(43 + s) for s in seeds], 104))
    # other length bounds
    codes, lens = text(n, lo=3, hi=20, ldx=20)
    assert np.array_equal(codes, synth.encode_strings([synth.lcg_text(42 + i, 3, 20) for i in range(n)], 20))
    assert lens.min() >= 3 and lens.max() <= 20


@pytest.mark.parametrize("n", [1, 64, 257])
def test_text_kernel_row_maps(n):
    """A permuted and gapped out_rows with seed_rows of its own: sample j lands in row rows[j] with seed 42 + seed_rows[j]; the rows in
    between keep the buffer's fill."""
    n_rows = 2 * n + 3
    perm = np.random.default_rng(n).permutation(n)
    rows, seeds = 2 * perm + 1, 1000 * n_rows + 3 * np.arange(n)
    codes, lens = text(n, seed_rows=seeds, rows=rows, n_rows=n_rows)
    want = np.full((n_rows, 100), CODE_FILL, dtype=np.int64)
    want_len = np.full(n_rows, SENTINEL, dtype=np.int32)
    strings = [synth.lcg_text(42 + int(s)) for s in seeds]
    want[rows] = synth.encode_strings(strings, 100)
    want_len[rows] = [len(s) for s in strings]
    assert np.array_equal(codes, want) and np.array_equal(lens, want_len)
    # out_rows alone (seed = 42 + j) and seed_rows alone (row = j)
    codes, _ = text(n, rows=rows, n_rows=n_rows)
    want[rows] = synth.encode_strings([synth.lcg_text(42 + j) for j in range(n)], 100)
    assert np.array_equal(codes, want)
    codes, _ = text(n, seed_rows=seeds)
    assert np.array_equal(codes, synth.encode_strings(strings, 100))


# ---------------------------------------------------------------------------------------------- composer
@pytest.mark.parametrize("key", ["fira", "mont"])
def test_compose_fixture_texts(fx, key):
    """Every fixture text, alone and in one batch, equals the sheet PIL drew.  The codes are 208 wide because the eight-line text has 207
    characters; the 23 texts that fit 100 are also composed from rows of 100 and of 104 codes through a reversed, gapped out_rows."""
    A, sheets, codes = _atlas(fx, key), fx[f"{key}/sheets"], fx[f"{key}/codes"]
    geo, atlas = R.geometry(int(A["origin_y"])), DevAtlas(A)
    got, err = compose(A, geo, codes, atlas=atlas)
    assert err == 0
    differ = [j for j in range(len(codes)) if not np.array_equal(got[j], sheets[j])]
    assert not differ, differ
    for j in range(len(codes)):                                            # one launch per text
        one, err = compose(A, geo, codes[j:j + 1], atlas=atlas)
        assert err == 0 and np.array_equal(one[0], sheets[j]), j
    fit = np.nonzero((codes[:, 100:] == 0).all(1))[0]
    assert len(fit) == 23
    rows = 2 * np.arange(len(fit))[::-1] + 1
    for ldx in (100, 104):
        got, err = compose(A, geo, codes[fit, :ldx], rows=rows, n_rows=2 * len(fit) + 2, atlas=atlas)
        assert err == 0 and np.array_equal(got[rows], sheets[fit]), ldx
        untouched = np.setdiff1d(np.arange(2 * len(fit) + 2), rows)
        assert (got[untouched] == INK).all(), ldx


def test_compose_more_sheets_than_workgroups(fx):
    """2048 + 61 sheets: the grid is capped at 2048 workgroups, so 61 of them compose a second sheet from the same LDS."""
    A, sheets, codes = _atlas(fx, "mont"), fx["mont/sheets"], fx["mont/codes"]
    pick = (np.arange(2048 + 61) * 7) % len(codes)
    got, err = compose(A, R.geometry(int(A["origin_y"])), codes[pick])
    assert err == 0 and np.array_equal(got, sheets[pick])


def test_compose_without_kerning_table(fx):
    """kern64 NULL is a table of zeros: Fira Code's sheets stay what they are, Montserrat's equal the reference without kerning."""
    for key in ("fira", "mont"):
        A, codes = _atlas(fx, key), fx[f"{key}/codes"]
        geo = R.geometry(int(A["origin_y"]))
        got, err = compose(A, geo, codes, atlas=DevAtlas(A, kern=False))
        want = R.compose_batch(dict(A, kern64=None), geo, codes)[0]
        assert err == 0 and np.array_equal(got, want), key
        assert np.array_equal(got, fx[f"{key}/sheets"]) == (key == "fira")


def test_compose_miniature_sheet(fx):
    """An 8 x 24 sheet under a 14 x 15 cell: with lines 6 pixels apart the first line's cells start above the sheet and the last one's end
    below it, the first glyph's cell starts left of it (origin_x = 2) and long lines run off its right edge."""
    A = _atlas(fx, "mont")
    geo = R.geometry(int(A["origin_y"]), height=8, width=24, line_height=6.0)
    assert geo.n_lines == 3 and geo.baseline[0] - int(A["origin_y"]) < 0 and int(A["origin_x"]) > 0
    texts = ["AV TO", "WWWWWW", "", "J", "A B C D E F G", "IIII IIII IIII", "Q  Q", " Ty.", "MMMM MM M"] + [synth.lcg_text(42 + i) for i in range(16)]
    codes = synth.encode_strings(texts, 100)
    want, _ = R.compose_batch(A, geo, codes)
    ink = want < 255
    assert len({w.tobytes() for w in want}) > 20 and ink[:, 0].any() and ink[:, -1].any() and ink[:, :, 0].any() and ink[:, :, -1].any()
    got, err = compose(A, geo, codes)
    assert err == 0 and np.array_equal(got, want)


def test_compose_bad_codes_are_flagged_and_skipped(fx):
    A = _atlas(fx, "mont")
    geo = R.geometry(int(A["origin_y"]))
    codes = synth.encode_strings(["AVAVAV TO TY", "HELLO WORLD", "P JAL WZ", "TO"], 100)
    clean, err = compose(A, geo, codes)
    assert err == 0
    dirty = codes.copy()
    dirty[0, 3], dirty[1, 0], dirty[1, 5], dirty[3, 2] = 200, -1, 127, 1 << 40     # inside a kerning run, first, at a space, after the text
    dirty[3, 3] = ord("Y")                                                          # ... which then goes on: "TO" + bad + "Y"
    want, bad = R.compose_batch(A, geo, dirty)
    assert bad.tolist() == [True, True, False, True]
    got, err = compose(A, geo, dirty)
    assert err & 1 and np.array_equal(got, want)
    assert np.array_equal(got[2], clean[2]) and not np.array_equal(got[0], clean[0])
    assert np.array_equal(got[1], R.compose(A, geo, [ord(c) for c in "ELLOWORLD"])[0])


def test_compose_addresses_rows_beyond_2_gib(fx):
    """One sheet into row 111 849 of a 111 851-row buffer (row * 19200 > 2^31): that row equals the reference, its two neighbours and the
    first row keep the marker bytes written into them before."""
    A = _atlas(fx, "fira")
    geo, atlas = R.geometry(int(A["origin_y"])), DevAtlas(A)
    n_rows, row = 111851, 111849
    assert row * 19200 > 2 ** 31
    big = torch.empty((n_rows, 80, 240), dtype=torch.uint8, device="cuda")
    marked = [0, row - 1, row + 1]
    for r in marked:
        big[r] = INK
    codes = fx["fira/codes"][3:4]
    cd, rd, g = dev(codes), dev(np.array([row], dtype=np.int64)), _geo_struct(geo)
    for _ in range(2):
        big[row] = INK
        _lib.check(_lib.lib().afr_op_compose_sheets(C.byref(atlas.struct), C.byref(g), ptr(cd), codes.shape[1], ptr(rd), 1, ptr(big), None, stream()))
        torch.cuda.synchronize()
        assert np.array_equal(big[row].cpu().numpy(), fx["fira/sheets"][3])
        for r in marked:
            assert bool((big[r] == INK).all()), r
    del big
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------- Python surface, CLI
def test_reference_dataset_equals_the_generated_folder(tmp_path):
    """reference_dataset(96, atlas of the built-in font) == datagen.generate + helpers.load_string_dataset_u8, codes and sheets, with this
    machine's PIL on both sides."""
    from ai_font_renderer_amd import datagen, devdata, helpers
    datagen.generate(str(tmp_path / "train_input"), 96)
    want = helpers.load_string_dataset_u8(str(tmp_path / "train_input"), num_samples=96)
    atlas = devdata.GlyphAtlas.from_font(None).to("cuda")
    got = devdata.reference_dataset(96, atlas)
    assert got.tensors[0].is_cuda and got.tensors[0].dtype == torch.int64 and got.tensors[1].dtype == torch.uint8
    assert torch.equal(got.tensors[0].cpu(), want.tensors[0]) and torch.equal(got.tensors[1].cpu(), want.tensors[1])
    # rows and out: the same sheets into a caller's buffer, in another order; a code outside the atlas is an IndexError
    buf = torch.full((100, 80, 240), INK, dtype=torch.uint8, device="cuda")
    rows = torch.arange(95, -1, -1)
    assert devdata.compose_sheets(atlas, got.tensors[0], out=buf, rows=rows) is buf
    assert torch.equal(buf[rows].cpu(), want.tensors[1]) and bool((buf[96:] == INK).all())
    bad = got.tensors[0][:2].clone()
    bad[1, 0] = 300
    with pytest.raises(IndexError):
        devdata.compose_sheets(atlas, bad)


def _run_cli(M, monkeypatch, tmp_path, name, device_data=None, fresh=False, epochs=7):
    monkeypatch.setattr(M, "NUM_SAMPLES", 96)
    monkeypatch.setattr(M, "NUM_EPOCHS", epochs)
    monkeypatch.setattr(M, "OUTPUT_DIR", name)
    monkeypatch.setattr(M, "DEVICE_DATA", device_data)
    monkeypatch.setattr(M, "FRESH_DATA", fresh)
    torch.manual_seed(42)


def test_cli_with_device_data_writes_the_same_model(tmp_path, monkeypatch):
    """`AFR_DEVICE_DATA=default python model.py --train` in miniature (96 sheets, 7 epochs, as test_train_string_renderer_end_to_end): the
    same font_renderer.pth bit for bit, and the same config.txt but for the added line, as the run that reads train_input/."""
    from ai_font_renderer_amd import datagen, model as M
    monkeypatch.chdir(tmp_path)
    datagen.generate("train_input", 96)
    _run_cli(M, monkeypatch, tmp_path, "out_folder")
    M.main(["model.py", "--train"])
    folder = torch.load(tmp_path / "font_renderer.pth", weights_only=True)
    os.rename(tmp_path / "train_input", tmp_path / "train_input_gone")      # the second run has no folder to read
    _run_cli(M, monkeypatch, tmp_path, "out_device", device_data="default")
    M.main(["model.py", "--train"])
    device = torch.load(tmp_path / "font_renderer.pth", weights_only=True)
    assert list(folder) == list(device)
    for k in folder:
        assert torch.equal(folder[k].view(torch.int32), device[k].view(torch.int32)), k
    cfg_f = (tmp_path / "out_folder" / "config.txt").read_text().splitlines()
    cfg_d = (tmp_path / "out_device" / "config.txt").read_text().splitlines()
    assert cfg_d == cfg_f + ["device_data = default"]
    res = [(tmp_path / d / "training_results.txt").read_text().splitlines()[:6] for d in ("out_folder", "out_device")]
    assert res[0] == res[1] and res[0][1] == "final_epoch = 7"


def test_cli_with_fresh_data_rewrites_the_training_rows(tmp_path, monkeypatch, capsys):
    """AFR_FRESH_DATA in miniature, two epochs: epoch 0 prints the losses of the run without it; after epoch 1 the bound training rows are
    reference_dataset's for the seeds 42 + 1 * N + row (texts as long as the bound rows are wide) and the validation rows are untouched."""
    from ai_font_renderer_amd import devdata, model as M
    monkeypatch.chdir(tmp_path)
    lines = {}
    for name, fresh in (("plain", False), ("fresh", True)):
        _run_cli(M, monkeypatch, tmp_path, name, device_data="default", fresh=fresh, epochs=2)
        model = M.train_string_renderer()
        lines[name] = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Epoch 0,")]
    assert len(lines["plain"]) == 1 and lines["plain"] == lines["fresh"]
    cfg = (tmp_path / "fresh" / "config.txt").read_text().splitlines()
    assert cfg[-2:] == ["device_data = default", "fresh_data = 1"]
    assert "fresh_data = 1" not in (tmp_path / "plain" / "config.txt").read_text()
    x, _, t = model.engine._ds[:3]
    N, L = 96, x.shape[1]
    atlas = devdata.GlyphAtlas.from_font(None).to("cuda")
    first = devdata.reference_dataset(N, atlas)
    assert first.tensors[0].shape[1] == L
    order = M._EpochOrder(N)
    tr, va = order.train_idx, order.val_idx
    assert len(tr) == 77 and len(va) == 19
    assert torch.equal(x[va].cpu(), first.tensors[0][va].cpu()) and torch.equal(t.view(N, 80, 240)[va].cpu(), first.tensors[1][va].cpu())
    strings = [synth.lcg_text(42 + N + int(r), 10, L) for r in tr]
    want_x = torch.from_numpy(synth.encode_strings(strings, L))
    assert torch.equal(x[tr].cpu(), want_x)
    assert not torch.equal(x[tr].cpu(), first.tensors[0][tr].cpu())
    want_t = devdata.compose_sheets(atlas, want_x)
    assert torch.equal(t.view(N, 80, 240)[tr].cpu(), want_t.cpu())
    for j in (0, 40, 76):                                                  # and against PIL itself
        from PIL import ImageFont
        from ai_font_renderer_amd import datagen
        assert np.array_equal(want_t[j].cpu().numpy(), datagen.render_sheet(strings[j], ImageFont.load_default(datagen.FONT_SIZE)))
