"""GPU: the training loop's reports together -- the one character-error launch per validation batch that the by-code and the pair table
share (model._CharErrorPass), and every report of the CLI switched on at once in miniature.  Integers only: every comparison is exact."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_by_code_and_pair_tables_share_one_launch_per_batch(monkeypatch):
    """96 sheets of the default font's data set against themselves with seeded noise, fed in two batches of 48 rows: both tables are
    those of one launch over all the rows, and devdata.char_errors is entered once per batch."""
    from ai_font_renderer_amd import devdata, model as M
    atlas = devdata.GlyphAtlas.from_font(None).to("cuda")
    codes, sheets = devdata.reference_dataset(96, atlas).tensors
    noise = torch.randint(-40, 41, sheets.shape, generator=torch.Generator().manual_seed(5), dtype=torch.int16).cuda()
    pred = (sheets.to(torch.int16) + noise).clamp(0, 255).to(torch.uint8)
    want = devdata.char_errors(atlas, codes, pred)
    want_pairs = devdata.pair_errors(codes, want.per_pos)
    assert int(want.by_code[:-1, 2].sum()) > 0 and int(want_pairs[..., 0].sum()) > 1000
    entered, char_errors = [], devdata.char_errors
    monkeypatch.setattr(devdata, "char_errors", lambda *a, **k: entered.append(1) or char_errors(*a, **k))
    errors = M._CharErrorPass(atlas, codes, pairs=True)
    rows = torch.randperm(96, generator=torch.Generator().manual_seed(6)).cuda()
    for batch in (rows[:48], rows[48:]):
        errors.add(SimpleNamespace(u8=pred[batch]), batch)
    assert len(entered) == 2
    assert torch.equal(errors.by_code, want.by_code)
    assert torch.equal(errors.by_pair, want_pairs)
    assert [t.data_ptr() for t in errors.reduced] == [errors.by_code.data_ptr(), errors.by_pair.data_ptr()]


HEADS = ("Val report:", "Tensor report:", "Char report:", "Pair report:", "Read report:")
CONTINUES = {"Val report:": (), "Tensor report:": ("  ", "Tensor report: DEAD OUTPUT HEAD"), "Char report:": ("  code ",), "Pair report:": ("  '",),
             "Read report:": ()}


def _run_cli(M, monkeypatch, name, on):
    for k, v in dict(NUM_SAMPLES=96, NUM_EPOCHS=1, OUTPUT_DIR=name, DEVICE_DATA="default", FRESH_DATA=True, ALPHABET=None, STEER=0.0, STEER_PAIRS=0.0,
                     VAL_REPORT=2 if on else None, TENSOR_REPORT=on, CHAR_REPORT=3 if on else None, PAIR_REPORT=3 if on else None,
                     READ_REPORT=3 if on else None).items():
        monkeypatch.setattr(M, k, v)
    torch.manual_seed(42)


def _tsv(path, header):
    lines = path.read_text().split("\n")
    assert lines[0].split("\t") == header and lines[-1] == ""
    return [l.split("\t") for l in lines[1:-1]]


def test_cli_all_reports_together_change_nothing_else(tmp_path, monkeypatch, capsys):
    """Every report on at once under fresh data, one epoch of 96 sheets, beside the run with every report off: the five blocks follow
    epoch 0's status line once each in their fixed order, every other line and font_renderer.pth are the plain run's, config.txt has the
    five lines in order, the artefacts are there, and the pair table summed over its contexts is the by-code table -- the two come from
    one launch."""
    from ai_font_renderer_amd import model as M
    monkeypatch.chdir(tmp_path)
    out, pth = {}, {}
    for name, on in (("out_plain", False), ("out_all", True)):
        _run_cli(M, monkeypatch, name, on)
        M.main(["model.py", "--train"])
        out[name] = [l.replace(name, "DIR") for l in capsys.readouterr().out.splitlines()]
        pth[name] = torch.load(tmp_path / "font_renderer.pth", weights_only=True)
    lines = out["out_all"]
    assert not any(l.startswith(HEADS) for l in out["out_plain"])
    at = [next(i for i, l in enumerate(lines) if l.startswith(h)) for h in HEADS]
    assert lines[at[0] - 1].startswith("Epoch 0,") and at == sorted(at)
    end = at[0]
    for h, start in zip(HEADS, at):                                      # each block: its head where the block before it ended, then its own lines
        assert start == end and [l for l in lines if l.startswith(h) and not l.startswith("Tensor report: DEAD")] == [lines[start]], h
        end = start + 1
        while CONTINUES[h] and lines[end].startswith(CONTINUES[h]):
            end += 1
    assert lines[at[1]] == "Tensor report:" and at[2] - at[1] == 13 + lines[at[2] - 1].startswith("Tensor report: DEAD")
    assert at[3] - at[2] == 4 and 2 <= at[4] - at[3] <= 4 and end == at[4] + 1
    assert lines[:at[0]] + lines[end:] == out["out_plain"]
    assert list(pth["out_plain"]) == list(pth["out_all"])
    for key in pth["out_plain"]:
        assert torch.equal(pth["out_plain"][key].view(torch.int32), pth["out_all"][key].view(torch.int32)), key
    cfg = [(tmp_path / d / "config.txt").read_text().splitlines() for d in ("out_plain", "out_all")]
    assert cfg[0][-2:] == ["device_data = default", "fresh_data = 1"]
    assert cfg[1] == cfg[0][:-2] + ["val_report = 2", "tensor_report = 1"] + cfg[0][-2:] + ["char_report = 3", "read_report = 3", "pair_report = 3"]
    epoch = tmp_path / "out_all" / "epoch_0"
    made = ("val_worst_0.bmp", "val_worst_1.bmp", "char_errors.tsv", "pair_errors.tsv", "confusion.tsv", "read_back.txt")
    assert all((epoch / f).is_file() for f in made)
    assert not any((tmp_path / "out_plain" / "epoch_0" / f).exists() for f in made)
    assert {p.name for p in epoch.iterdir()} - set(made) == {p.name for p in (tmp_path / "out_plain" / "epoch_0").iterdir()}
    by_code = {r[0]: [int(v) for v in (r[2], r[3], r[4], r[6])]
               for r in _tsv(epoch / "char_errors.tsv", ["code", "char", "chars", "pixels", "sumsq", "off2", "wrong"]) if r[0] != "background"}
    summed = {}
    for r in _tsv(epoch / "pair_errors.tsv", ["prev", "prev_char", "code", "char", "chars", "pixels", "sumsq", "wrong"]):
        summed[r[2]] = [a + int(v) for a, v in zip(summed.get(r[2], [0, 0, 0, 0]), r[4:])]
    assert summed == by_code and len(by_code) > 20
