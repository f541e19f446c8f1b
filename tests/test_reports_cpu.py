"""The training loop's tables of optional config.txt lines and of the switches' preconditions, read with the module's switches set."""
from types import SimpleNamespace

import pytest

SWITCHES = dict(VAL_REPORT=2, TENSOR_REPORT=True, DEVICE_DATA="default", CHAR_REPORT=3, ALPHABET="alnum", STEER=0.0, READ_REPORT=4,
                PAIR_REPORT=5, STEER_PAIRS=0.0)
PLAIN = SimpleNamespace(loss="mse", optimizer="adamw", max_grad_norm=None, ema_decay=None, ema_every=1)


def _set(monkeypatch, **switches):
    from ai_font_renderer_amd import model as M
    for k, v in {**SWITCHES, **switches}.items():
        monkeypatch.setattr(M, k, v)
    return M


def test_config_lines_come_in_the_fixed_order_and_formats(monkeypatch):
    from ai_font_renderer_amd import model as M
    for k, v in dict(VAL_REPORT=None, TENSOR_REPORT=False, DEVICE_DATA=None, CHAR_REPORT=None, ALPHABET=None, STEER=0.0, READ_REPORT=None,
                     PAIR_REPORT=None, STEER_PAIRS=0.0).items():
        monkeypatch.setattr(M, k, v)
    assert M._optional_config_lines(PLAIN, False) == []                  # a default run's config.txt is the reference's
    eng = SimpleNamespace(loss="bce", optimizer="lion", max_grad_norm=0.5, ema_decay=0.999, ema_every=8)
    head = ["loss = bce", "optimizer = lion", "max_grad_norm = 0.5", "ema_decay = 0.999", "ema_every = 8"]
    assert M._optional_config_lines(eng, False) == head
    assert M._optional_config_lines(SimpleNamespace(loss="mse", optimizer="adamw", max_grad_norm=0, ema_decay=0.0, ema_every=1), False) == [
        "ema_decay = 0", "ema_every = 1"]                               # a decay of 0 is still an average that is kept
    # every switch set; the two steering shares exclude each other, so two calls cover both
    M = _set(monkeypatch, STEER=0.25)
    assert M._optional_config_lines(eng, True) == head + [
        "val_report = 2", "tensor_report = 1", "device_data = default", "fresh_data = 1", "char_report = 3", "alphabet = alnum", "steer = 0.25",
        "read_report = 4", "pair_report = 5"]
    M = _set(monkeypatch, STEER_PAIRS=0.5)
    assert M._optional_config_lines(PLAIN, True) == [
        "val_report = 2", "tensor_report = 1", "device_data = default", "fresh_data = 1", "char_report = 3", "alphabet = alnum",
        "read_report = 4", "pair_report = 5", "steer_pairs = 0.5"]
    M = _set(monkeypatch, STEER=1e-05, STEER_PAIRS=0.123456789)         # :g, as max_grad_norm
    assert [l for l in M._optional_config_lines(PLAIN, False) if l.startswith("steer")] == ["steer = 1e-05", "steer_pairs = 0.123457"]


def test_switches_are_refused_without_what_they_need(monkeypatch):
    from ai_font_renderer_amd import model as M
    off = dict(CHAR_REPORT=None, READ_REPORT=None, PAIR_REPORT=None, STEER=0.0, STEER_PAIRS=0.0)
    atlas, refresh = object(), object()
    _set(monkeypatch, **off)
    M._check_switches(None, None)
    _set(monkeypatch)
    M._check_switches(atlas, None)                                       # the three reports need the atlas alone
    _set(monkeypatch, STEER=0.5)
    M._check_switches(atlas, refresh)
    _set(monkeypatch, STEER_PAIRS=0.5)
    M._check_switches(atlas, refresh)
    for switch, value, have, message in (
            ("CHAR_REPORT", 3, (None, refresh), "the character report needs the glyph atlas the data set was composed from (AFR_DEVICE_DATA)"),
            ("READ_REPORT", 3, (None, refresh), "the read-back report needs the glyph atlas the data set was composed from (AFR_DEVICE_DATA)"),
            ("PAIR_REPORT", 3, (None, refresh), "the pair report needs the glyph atlas the data set was composed from (AFR_DEVICE_DATA)"),
            ("STEER", 0.5, (atlas, None), "steering needs the glyph atlas and the fresh-data rewrite (AFR_DEVICE_DATA, AFR_FRESH_DATA)"),
            ("STEER", 0.5, (None, refresh), "steering needs the glyph atlas and the fresh-data rewrite (AFR_DEVICE_DATA, AFR_FRESH_DATA)"),
            ("STEER_PAIRS", 0.5, (atlas, None), "pair steering needs the glyph atlas and the fresh-data rewrite (AFR_DEVICE_DATA, AFR_FRESH_DATA)"),
            ("STEER_PAIRS", 0.5, (None, refresh), "pair steering needs the glyph atlas and the fresh-data rewrite (AFR_DEVICE_DATA, AFR_FRESH_DATA)")):
        _set(monkeypatch, **{**off, switch: value})
        with pytest.raises(ValueError) as e:
            M._check_switches(*have)
        assert str(e.value) == message
    _set(monkeypatch, **{**off, "STEER": 0.5, "STEER_PAIRS": 0.5})
    with pytest.raises(ValueError) as e:
        M._check_switches(atlas, refresh)
    assert str(e.value) == "AFR_STEER_PAIRS and AFR_STEER together: the fresh texts are drawn from one table"


def test_env_parsers_keep_their_messages(monkeypatch):
    """the six bound names of the two generic parsers: each switch's own words in its refusals"""
    from ai_font_renderer_amd import model as M
    for k in ("AFR_DEVICE_DATA", "AFR_FRESH_DATA", "AFR_STEER", "AFR_STEER_PAIRS"):
        monkeypatch.delenv(k, raising=False)
    for parse, name, what, atlas_for in (
            (M._val_report_from_env, "AFR_VAL_REPORT", "worst validation sheets", None),
            (M._char_report_from_env, "AFR_CHAR_REPORT", "worst characters", "defines which character owns a pixel"),
            (M._read_report_from_env, "AFR_READ_REPORT", "confusions", "holds the candidates' cells"),
            (M._pair_report_from_env, "AFR_PAIR_REPORT", "worst pairs", "defines which character owns a pixel")):
        monkeypatch.setenv(name, "0")
        with pytest.raises(ValueError) as e:
            parse()
        assert str(e.value) == f"{name} must be an integer >= 1 (the number of {what} to list), got '0'"
        monkeypatch.setenv(name, "3")
        if atlas_for is None:
            assert parse() == 3
        else:
            with pytest.raises(ValueError) as e:
                parse()
            assert str(e.value) == f"{name} needs AFR_DEVICE_DATA: the glyph atlas the sheets are composed from {atlas_for}"
            monkeypatch.setenv("AFR_DEVICE_DATA", "default")
            assert parse() == 3
            monkeypatch.delenv("AFR_DEVICE_DATA")
        monkeypatch.delenv(name)
        assert parse() is None
    for parse, name in ((M._steer_from_env, "AFR_STEER"), (M._steer_pairs_from_env, "AFR_STEER_PAIRS")):
        monkeypatch.setenv(name, "1")
        with pytest.raises(ValueError) as e:
            parse()
        assert str(e.value) == f"{name} must be a share in [0, 1), e.g. 0.5, got '1'"
        monkeypatch.setenv(name, "0.5")
        with pytest.raises(ValueError) as e:
            parse()
        assert str(e.value) == f"{name} needs AFR_FRESH_DATA=1: only texts that are redrawn every epoch can be steered"
        monkeypatch.delenv(name)
        assert parse() == 0.0
    monkeypatch.setenv("AFR_FRESH_DATA", "1")
    monkeypatch.setenv("AFR_STEER", "0.5")
    monkeypatch.setenv("AFR_STEER_PAIRS", "0.25")
    assert M._steer_from_env() == 0.5                                    # the exclusion is AFR_STEER_PAIRS' to state
    with pytest.raises(ValueError) as e:
        M._steer_pairs_from_env()
    assert str(e.value) == "AFR_STEER_PAIRS and AFR_STEER together: the fresh texts are drawn from one table, by character or by pair"
    monkeypatch.setenv("AFR_STEER", "0")
    assert M._steer_pairs_from_env() == 0.25
