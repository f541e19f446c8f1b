"""Drop-in for the reference's model module on MI355X: same constants, class, training entry points, artefacts
and CLI (reference model.py:64-127, 129-204, 209-384, 389-454), with the hot path -- forward, MSE, backward,
AdamW -- running in libafr.so (hand-written HIP, see csrc/) instead of torch ops.

    python model.py --train        train, save font_renderer.pth, render the test strings
    python model.py                load (or train if missing) and render
    anything else                  two usage lines, exit status 1

What is deliberately different from the reference, and why:
  * device selection: the reference pins CUDA_VISIBLE_DEVICES="3" (model.py:95); here each process uses the GPU
    given by LOCAL_RANK (one process per GPU), and there is no CPU/MPS fallback -- the product IS the HIP path;
  * the dataset lives in HBM as uint8 sheets and batches are gathered on the device by index; the 2x32 DataLoader
    worker processes and the per-step 78 MB host->device copy (model.py:249-266,295-296) are gone.  Split and
    shuffle order reproduce random_split / DataLoader(shuffle=True, generator=g) draw for draw (_EpochOrder);
  * loss.item() per step (model.py:311) becomes one device->host read per epoch (the loss accumulates on device);
  * dropout uses a counter-hash stream instead of torch's bernoulli_ stream (same rates, same placement);
  * AFR_DTYPE=bf16 selects the throughput mode (bf16 MFMA operands); the default f32 mode is the parity mode, and
    AFR_DTYPE=bf16x3 the fast parity mode (f32 except that every Linear product runs as three split-bf16 MFMAs);
  * AFR_LOSS=bce selects a sigmoid output head trained with binary cross-entropy on the logits (the loss the reference's
    clamp head replaced, model.py:155) through the same fused step; the default, mse, is the reference's clamp + MSE.  A
    checkpoint does not record the head: the caller says which one it wants, as with the dtype;
  * AFR_CLIP_NORM=<max_norm> clips the gradients by their global L2 norm inside the optimizer step
    (torch.nn.utils.clip_grad_norm_'s formula; Engine.set_grad_clip).  Unset or 0: no clipping, the reference's loop;
  * AFR_OPTIMIZER=lion trains with Lion (one moment, sign update; include/afr.h afr_set_optimizer) instead of AdamW.  The loop then
    steps with LEARNING_RATE / 10 and WEIGHT_DECAY * 10 -- the Lion paper's rule of thumb, which keeps lr * weight_decay what it
    was; the plateau scheduler still works on the LEARNING_RATE scale.  Unset or adamw: the reference's optimizer;
  * AFR_EMA=<decay> or AFR_EMA=<decay>:<every> (0.999, 0.999:8) keeps an exponential moving average of the weights, updated on the
    device after every <every>-th optimizer step (Engine.set_ema).  The validation loss that picks the best epoch and drives the
    plateau scheduler, the 5-epoch test-string dumps and the saved model are then taken from the average.  Unset: the reference's
    loop, nothing changes;
  * AFR_NO_DECAY=1 takes the tensors of config.no_decay_names -- every bias and LayerNorm tensor, the positional table and the
    embedding -- out of weight decay (optimizer groups, Engine.set_param_groups).  Unset: one group, the reference's optimizer;
  * AFR_VAL_REPORT=<k> (k >= 1) adds a validation report, counted on the device (Engine.evaluate_last): on the epochs that print a
    status line, one more line with the rates of pixels whose 8-bit level is off by >= 1 and by >= 2 and of wrong-ink pixels, the
    largest level difference and the k validation sheets with the largest loss, whose predicted bitmaps are written as
    epoch_<e>/val_worst_<j>.bmp.  Unset: nothing changes;
  * AFR_TENSOR_REPORT=1 adds a per-tensor report, computed on the device (Engine.tensor_stats): on the epochs that print a status
    line, rank 0 prints a block headed "Tensor report:" with one line per parameter tensor -- the weight norm |p|, the gradient norm
    |g|, |g|/|p|, the fraction of gradient elements that are exactly zero, the relative size |dp|/|p| of the epoch's last optimizer
    step and the non-finite counts when there are any -- and one more line when the output head is dead (every gradient of
    fc_output.weight zero).  The gradients are those of a probe: one forward + backward on rank 0's shard of the epoch's first
    training batch after the validation pass, with a dropout step of its own, no optimizer step, and its loss discarded; the step
    size comes from a snapshot of the weights taken before the epoch's last training batch.  Neither changes the run: every artefact
    and every other line is what it is without the variable.  Unset: nothing changes;
  * AFR_DEVICE_DATA=<font file> or AFR_DEVICE_DATA=default takes the data set from devdata.reference_dataset instead of train_input/:
    the NUM_SAMPLES texts and their sheets are produced on the device from a glyph atlas of that font (default: Pillow's built-in
    font, as datagen.generate without one), byte for byte the tensors the folder datagen.generate writes would load as.  Every rank
    composes the same bytes; nothing is read from disk and nothing is broadcast.  Unset: the reference's folder;
  * AFR_FRESH_DATA=1 (needs AFR_DEVICE_DATA) rewrites the training rows in place before every epoch e >= 1: row r gets the text of seed
    42 + e * N + r (texts as long as the bound rows are wide, MAX_CHARS_PER_SHEET for the full data set) and its sheet.  The validation
    rows never change and epoch 0 is the run without the variable.  Unset: the data set is fixed, as the reference's;
  * AFR_CHAR_REPORT=<k> (k >= 1, needs AFR_DEVICE_DATA: the atlas is what says which character a pixel belongs to) adds a report of
    the rendering error by character, counted on the device (devdata.char_errors after Engine.evaluate_last's bitmaps): on the
    epochs that print a status line, a block headed "Char report:" with the background's rms level error and wrong-ink rate and the
    k codes with the largest mean squared level error over the validation sheets, and epoch_<e>/char_errors.tsv with every code's
    counters.  Nothing steps: every other line and artefact is what it is without the variable.  Unset: nothing changes;
  * AFR_ALPHABET=<name or characters> (needs AFR_DEVICE_DATA) draws the NUM_SAMPLES texts, and AFR_FRESH_DATA's, from the weighted text
    source (devdata.text_weights, afr_op_dataset_text_w) with equal weights over that alphabet: upper, lower, letters, alnum, ascii, or
    the literal set of the characters given (codes 33..126; the space separates words and is no letter).  With an alphabet other than
    upper the test-string renders add a lower-case pangram, the digits and a line of punctuation, each filtered to the alphabet.  Unset,
    or upper: byte for byte the run it is without the variable;
  * AFR_STEER=<share> (0 <= share < 1, needs AFR_FRESH_DATA) steers the fresh texts by the characters' errors: every validation pass keeps
    afr_op_sheet_char_errors' by-code table (AFR_CHAR_REPORT's mechanism, all-reduced, so every rank holds the same table), and the
    rewrite before the next epoch draws its letters with weight floor_w + gain * min(the character's mean squared error / the
    alphabet's, 16), floor_w = round((1 - share) * 4096), gain = round(share * 4096) -- built on the device from the table where it
    lies (afr_op_text_weights).  The validation rows are never rewritten, so validation losses stay comparable.  On the epochs that
    print a status line one more line names the five heaviest codes of the last rewrite.  Unset or 0: the run without it;
  * AFR_READ_REPORT=<k> (k >= 1, needs AFR_DEVICE_DATA; the candidates are AFR_ALPHABET's codes, A-Z without one) reads the validation
    sheets back on the device (devdata.read_back after Engine.evaluate_last's bitmaps): for every drawn character, which glyph of the
    atlas at this pen explains the predicted pixels best.  On the epochs that print a status line, one line headed "Read report:" with
    the share of characters read right, the share read blank and the k most frequent confusions as Q->O 312; epoch_<e>/confusion.tsv
    with every non-zero counter; and epoch_<e>/read_back.txt, each rendered test string beside what was read from it.  Nothing steps:
    every other line and artefact is what it is without the variable.  Unset: nothing changes;
  * AFR_PAIR_REPORT=<k> (k >= 1, needs AFR_DEVICE_DATA) adds a report of the rendering error by (preceding character, character),
    counted on the device (devdata.char_errors' per-position records scattered by devdata.pair_errors): on the epochs that print a
    status line, a block headed "Pair report:" with the k pairs of the alphabet seen at least 8 times that have the largest mean squared
    level error, as 'W' after 'W' (or: after word start), and epoch_<e>/pair_errors.tsv with every non-zero record.  Nothing steps:
    every other line and artefact is what it is without the variable.  Unset: nothing changes;
  * AFR_STEER_PAIRS=<share> (0 <= share < 1, needs AFR_FRESH_DATA, not together with a non-zero AFR_STEER) steers the fresh texts by the
    pairs' errors: every validation pass keeps the pair table, and the rewrite before the next epoch draws every letter given the letter
    before it (afr_op_dataset_text_m) with weight floor_w + gain * min(the pair's mean squared error / the table's, 16), a pair seen
    fewer than 8 times counting as average -- AFR_STEER's floor_w and gain, built on the device from the table where it lies
    (afr_op_pair_weights).  The validation rows are never rewritten.  On the epochs that print a status line one more line names the
    five heaviest pairs of the last rewrite.  Unset or 0: the run without it.
"""
import contextlib
import datetime
import os
import random
import sys
from functools import partial

import numpy as np
import torch
import torch.nn as nn

from . import helpers
from .config import SheetConfig, no_decay_names
from .helpers import MODEL_FILENAME, load_model, load_string_dataset, render_strings, save_model  # noqa: F401

# ---------------------------------------------------------------- constants (reference model.py:64-87)
SHEET_HEIGHT = 80
SHEET_WIDTH = 240
MAX_CHARS_PER_SHEET = 100
NUM_SAMPLES = 150000
OUTPUT_DIR = "train_output_" + datetime.datetime.now().strftime("%m_%d_%H_%M_%S")
NUM_EPOCHS = 10000
LEARNING_RATE = 0.001
EARLY_STOPPING_PATIENCE = 70
VALIDATION_SPLIT = 0.2
WEIGHT_DECAY = 0.0005
EMBEDDING_DIM = 32
DROPOUT_RATE = 0.2
NUM_ATTENTION_HEADS = 4
SCHEDULER_PATIENCE = 20
SCHEDULER_FACTOR = 0.7
MIN_LEARNING_RATE = 1e-6
SEED = 42
ADAM_BETAS = (0.9, 0.99)                      # model.py:273
COMPUTE_DTYPE = os.environ.get("AFR_DTYPE", "f32")
COMPUTE_LOSS = os.environ.get("AFR_LOSS", "mse")     # "mse" | "bce"
COMPUTE_OPTIMIZER = os.environ.get("AFR_OPTIMIZER", "adamw")     # "adamw" | "lion"
CLIP_NORM = float(os.environ.get("AFR_CLIP_NORM", "0") or 0) or None     # global gradient-norm clip; None = off


def _ema_from_env():
    """AFR_EMA = "<decay>" | "<decay>:<every>" -> (decay, every); unset or empty -> (None, 1).  Read when a model is constructed; a
    value that does not parse, or lies outside what Engine.set_ema takes, is a ValueError."""
    spec = os.environ.get("AFR_EMA", "").strip()
    if not spec:
        return None, 1
    decay, _, every = spec.partition(":")
    try:
        return float(decay), int(every) if every else 1
    except ValueError:
        raise ValueError(f"AFR_EMA must be <decay> or <decay>:<every>, e.g. 0.999 or 0.999:8, got {spec!r}") from None


def _count_from_env(name, what, atlas_for=None):
    """<name> = "<k>", k >= 1: a report that lists k of `what`; unset or empty -> None (off).  Anything else is a ValueError, and so is --
    with atlas_for, what the glyph atlas does for the report -- the report without AFR_DEVICE_DATA (no atlas)."""
    spec = os.environ.get(name, "").strip()
    if not spec:
        return None
    try:
        k = int(spec)
    except ValueError:
        k = 0
    if k < 1:
        raise ValueError(f"{name} must be an integer >= 1 (the number of {what} to list), got {spec!r}")
    if atlas_for and not os.environ.get("AFR_DEVICE_DATA", "").strip():
        raise ValueError(f"{name} needs AFR_DEVICE_DATA: the glyph atlas the sheets are composed from {atlas_for}")
    return k


def _share_from_env(name, instead_of=None):
    """<name> = "<share>", a float in [0, 1): how much of a fresh letter's weight follows the errors; unset, empty or 0 -> 0.0 (off).
    Anything else, a share without AFR_FRESH_DATA (nothing is redrawn), or -- with instead_of -- a share together with a non-zero share of
    that switch (a text is drawn from one table) is a ValueError."""
    spec = os.environ.get(name, "").strip()
    if not spec:
        return 0.0
    try:
        share = float(spec)
    except ValueError:
        share = -1.0
    if not 0.0 <= share < 1.0:
        raise ValueError(f"{name} must be a share in [0, 1), e.g. 0.5, got {spec!r}")
    if os.environ.get("AFR_FRESH_DATA", "").strip() != "1":
        raise ValueError(f"{name} needs AFR_FRESH_DATA=1: only texts that are redrawn every epoch can be steered")
    if share and instead_of and _share_from_env(instead_of):
        raise ValueError(f"{name} and {instead_of} together: the fresh texts are drawn from one table, by character or by pair")
    return share


_OWNERS = "defines which character owns a pixel"
# the validation report with the k worst sheets; the per-character and per-pair error reports with the k worst codes and pairs; the
# read-back report with the k most frequent confusions; the shares of a fresh letter's weight that follow its error and its pair's
_val_report_from_env = partial(_count_from_env, "AFR_VAL_REPORT", "worst validation sheets")
_char_report_from_env = partial(_count_from_env, "AFR_CHAR_REPORT", "worst characters", _OWNERS)
_read_report_from_env = partial(_count_from_env, "AFR_READ_REPORT", "confusions", "holds the candidates' cells")
_pair_report_from_env = partial(_count_from_env, "AFR_PAIR_REPORT", "worst pairs", _OWNERS)
_steer_from_env = partial(_share_from_env, "AFR_STEER")
_steer_pairs_from_env = partial(_share_from_env, "AFR_STEER_PAIRS", "AFR_STEER")


def _tensor_report_from_env():
    """AFR_TENSOR_REPORT = "1": the per-tensor report; unset or empty -> False (off).  Anything else is a ValueError."""
    spec = os.environ.get("AFR_TENSOR_REPORT", "").strip()
    if spec not in ("", "1"):
        raise ValueError(f"AFR_TENSOR_REPORT must be 1 (print the per-tensor report) or unset, got {spec!r}")
    return spec == "1"


def _device_data_from_env():
    """(AFR_DEVICE_DATA, AFR_FRESH_DATA) -> (None | "default" | the path of a font file, bool).  A font file that is not there, a
    fresh-data value other than 1, or fresh data without device data is a ValueError."""
    spec, fresh = os.environ.get("AFR_DEVICE_DATA", "").strip(), os.environ.get("AFR_FRESH_DATA", "").strip()
    if spec and spec != "default" and not os.path.isfile(spec):
        raise ValueError(f"AFR_DEVICE_DATA must be a font file or 'default' (Pillow's built-in font), got {spec!r}")
    if fresh not in ("", "1"):
        raise ValueError(f"AFR_FRESH_DATA must be 1 (new training rows every epoch) or unset, got {fresh!r}")
    if fresh and not spec:
        raise ValueError("AFR_FRESH_DATA=1 needs AFR_DEVICE_DATA: only a data set composed on the device can be rewritten")
    return spec or None, fresh == "1"


def _alphabet_from_env():
    """AFR_ALPHABET = one of synth's alphabet names or a literal string of characters -> the string; unset or empty -> None.  A literal
    with a space or a code outside 33..126, or an alphabet without AFR_DEVICE_DATA, is a ValueError."""
    spec = os.environ.get("AFR_ALPHABET", "")
    if not spec:
        return None
    from . import synth
    synth.alphabet_members(spec)
    if not os.environ.get("AFR_DEVICE_DATA", "").strip():
        raise ValueError("AFR_ALPHABET needs AFR_DEVICE_DATA: the folder data set's texts are what they are")
    return spec


# read at import, like the settings above: a bad value stops the run before it starts
VAL_REPORT, TENSOR_REPORT = _val_report_from_env(), _tensor_report_from_env()
DEVICE_DATA, FRESH_DATA = _device_data_from_env()
CHAR_REPORT, READ_REPORT = _char_report_from_env(), _read_report_from_env()
ALPHABET, STEER = _alphabet_from_env(), _steer_from_env()
PAIR_REPORT, STEER_PAIRS = _pair_report_from_env(), _steer_pairs_from_env()
PAIR_MIN_CHARS = 8                                            # a pair seen fewer times is not listed, and is steered as the average
STEER_UNIT = 4096                                             # floor_w + gain of the steered letter table: the weight of an average character


def _steer_weights(share):
    """(floor_w, gain) of devdata.text_weights for a steering share."""
    return max(1, round((1.0 - share) * STEER_UNIT)), round(share * STEER_UNIT)


DATA_FIRST_SEED = 42                                  # sample i of the data set is the text of seed i + 42 (generate_font.ts:204)


def _tensor_report_lines(p, g, d):
    """The block AFR_TENSOR_REPORT prints, as a list of lines.  p, g, d: the statistics of the weights, of the probe's gradients and of
    the last step's weight difference (TensorStats after cpu(), or anything with names, sumsq, n_nan, n_inf, n_zero, numel)."""
    def norm(st, i):
        return float(np.sqrt(np.float64(st.sumsq[i])))

    def ratio(a, b):
        return a / b if b > 0 else float("nan")

    width = max(len(nm) for nm in p.names)
    lines = ["Tensor report:"]
    for i, nm in enumerate(p.names):
        pn, gn, dn = norm(p, i), norm(g, i), norm(d, i)
        line = (f"  {nm:<{width}}  |p| {pn:.4e}  |g| {gn:.4e}  |g|/|p| {ratio(gn, pn):.3e}  "
                f"g zero {int(g.n_zero[i]) / max(1, int(g.numel[i])):.4f}  |dp|/|p| {ratio(dn, pn):.3e}")
        bad = [f"{tag} {int(st.n_nan[i])} nan {int(st.n_inf[i])} inf" for tag, st in (("p", p), ("g", g), ("dp", d))
               if int(st.n_nan[i]) + int(st.n_inf[i]) > 0]
        lines.append(line + ("  NON-FINITE: " + ", ".join(bad) if bad else ""))
    if "fc_output.weight" in g.names:
        i = g.names.index("fc_output.weight")
        if int(g.n_zero[i]) == int(g.numel[i]):
            lines.append("Tensor report: DEAD OUTPUT HEAD (every gradient of fc_output.weight is zero)")
    return lines


class _Report:
    """What _run_epoch asks of a report: hooks at the moments of an epoch, each a no-op unless a report overrides it."""
    takes_batches = False     # add() is fed every validation batch's evaluation (one Engine.evaluate_last, shared by all that take it) ...
    needs_u8 = False          # ... and reads its bitmaps, res.u8
    reduced = ()              # the tensors end_validation sums over the ranks

    def before_step(self, b, nb, rows, mean_elems):
        """before training batch b of nb; rows: this rank's rows of it"""

    def after_step(self, b, nb, rows, mean_elems):
        """after that batch's optimizer step"""

    def add(self, res, rows):
        """one validation batch: its evaluation and this rank's rows"""

    def end_validation(self, dist, rank, evaluate):
        """after the last validation batch, under the weights it was run with.  dist: torch.distributed when there are ranks to reduce
        over, else None -- every rank issues the same collectives; evaluate(rows) evaluates data-set rows once more, with bitmaps."""
        for t in self.reduced if dist is not None else ():
            dist.all_reduce(t, op=dist.ReduceOp.SUM)

    def end_epoch(self, inputs=None, targets=None):
        """once the validation loss has been read; the dense tensors when the epoch runs on them and not by rows"""


class _TensorReport(_Report):
    """What AFR_TENSOR_REPORT gathers during one epoch, on rank 0 alone and with no collective: the statistics of the last training
    step's weight difference (against a snapshot of the weights, allocated once per model) and those of the weights and of a probe's
    gradients.  Nothing here steps, advances a counter the run reads, or leaves a loss behind."""

    def __init__(self, model):
        self.model, self.eng = model, model.engine
        self.first = None                         # (this rank's rows of the epoch's first training batch, its mean_elems)
        self.p = self.g = self.d = None

    def before_step(self, b, nb, rows, mean_elems):
        if b == 0:
            self.first = (rows, mean_elems)
        if b == nb - 1:                           # the snapshot the last step is measured against
            if getattr(self.model, "_tensor_snapshot", None) is None:
                self.model._tensor_snapshot = torch.empty_like(self.eng.flat_params)
            self.model._tensor_snapshot.copy_(self.eng.flat_params)

    def after_step(self, b, nb, rows, mean_elems):
        if b == nb - 1:
            self.d = self.eng.tensor_stats("params", minus=self.model._tensor_snapshot)

    def end_epoch(self, inputs=None, targets=None):
        """The probe: forward + loss + backward of the first training batch's rows (by data-set rows, or dense when inputs are given); the
        dropout step is the next one the model WOULD draw, passed explicitly: model._next_step() does not move."""
        eng, (rows, me) = self.eng, self.first
        _batch_calls(eng, None, inputs, targets, rows).forward_loss(step=self.model._steps + 1, mean_elems=me)
        eng.backward()
        eng.read_loss(reset=True)                 # the probe's loss is nobody's
        self.g = eng.tensor_stats("grads").cpu()
        self.p = eng.tensor_stats("params").cpu()
        self.d = self.d.cpu()

    def lines(self):
        return _tensor_report_lines(self.p, self.g, self.d)


class _ValReport(_Report):
    """What AFR_VAL_REPORT keeps on the device during one validation pass: the column sums of the evaluation kernel's counts, their
    maximum, and the k largest per-sample losses with their data-set indices (merged batch by batch with torch.topk)."""
    takes_batches = True

    def __init__(self, k, dev, bitmaps=False):
        self.k, self.bitmaps = int(k), bool(bitmaps)
        self.sums = torch.zeros(4, dtype=torch.int64, device=dev)         # pixels off by >= 1, by >= 2, wrong ink; sheets
        self.max = torch.zeros(1, dtype=torch.int64, device=dev)
        self.loss = torch.empty(0, dtype=torch.float32, device=dev)
        self.idx = torch.empty(0, dtype=torch.int64, device=dev)
        self.u8 = None                                                    # [k, H, W] of the worst sheets (bitmaps, rank 0)

    def add(self, res, idx):
        st = res.stats
        self.sums[:3] += st[:, [0, 1, 3]].sum(0)
        self.sums[3] += st.shape[0]
        self.max = torch.maximum(self.max, st[:, 2].max().reshape(1))
        loss, ids = torch.cat([self.loss, res.loss_rows]), torch.cat([self.idx, idx.to(self.idx.device).reshape(-1)])
        top = torch.topk(loss, min(self.k, loss.numel()))
        self.loss, self.idx = top.values, ids[top.indices]

    def end_validation(self, dist, rank, evaluate):
        """Every rank issues both collectives (the setting is rank-invariant); the worst list stays this rank's."""
        if dist is not None:
            dist.all_reduce(self.sums, op=dist.ReduceOp.SUM)
            dist.all_reduce(self.max, op=dist.ReduceOp.MAX)
        if self.bitmaps and rank == 0 and self.idx.numel():               # the worst sheets once more, for their bitmaps (no collective)
            self.u8 = evaluate(self.idx).u8

    def line(self, pixels, world=1):
        s, n = self.sums.tolist(), max(1, int(self.sums[3]) * pixels)
        worst = ", ".join(f"{i}({v:.6f})" for i, v in zip(self.idx.tolist(), self.loss.tolist()))
        return (f"Val report: off by >= 1 level {s[0] / n:.6f}, off by >= 2 levels {s[1] / n:.6f}, wrong ink {s[2] / n:.6f}, "
                f"max level diff {int(self.max)}, worst {len(self.idx)}{' of rank 0 shard' if world > 1 else ''}: {worst}")


def _write_tsv(path, header, rows):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        for row in (header, *rows):
            f.write("\t".join(str(v) for v in row) + "\n")


class _CharErrorPass(_Report):
    """What the character-error pass of the validation batches leaves on the device: afr_op_sheet_char_errors' by-code table, which every
    batch's launch adds to (the batch's rows of the bound codes, the evaluation's bitmaps), and -- with pairs -- afr_op_pair_errors' table
    by (preceding character, character), scattered from the same launch's per-position records on the same rows.  AFR_CHAR_REPORT and
    AFR_STEER read by_code, AFR_PAIR_REPORT and AFR_STEER_PAIRS by_pair; only a table somebody reads is summed over the ranks."""
    takes_batches = needs_u8 = True

    def __init__(self, atlas, codes, by_code=True, pairs=False):
        from . import devdata
        self.atlas, self.codes = atlas, codes
        self.by_code = torch.zeros((atlas.n_codes + 1, 5), dtype=torch.int64, device=atlas.device)
        self.by_pair = torch.zeros(devdata.PAIR_SHAPE + (4,), dtype=torch.int64, device=atlas.device) if pairs else None
        self.reduced = ((self.by_code,) if by_code else ()) + ((self.by_pair,) if pairs else ())

    def add(self, res, rows):
        from . import devdata
        if rows.numel():
            per_pos = devdata.char_errors(self.atlas, self.codes, res.u8.contiguous(), res.u8.shape[1], res.u8.shape[2], rows=rows,
                                          by_code=self.by_code).per_pos
            if self.by_pair is not None:
                devdata.pair_errors(self.codes, per_pos, rows=rows, by_pair=self.by_pair)


class _CharReport:
    """AFR_CHAR_REPORT's block and char_errors.tsv, from the by-code table of a _CharErrorPass."""

    def __init__(self, k, errors):
        self.k, self.errors = int(k), errors

    table = property(lambda self: self.errors.by_code)

    @staticmethod
    def _rates(row):
        chars, pixels, sumsq, off2, wrong = row
        return float(np.sqrt(sumsq / pixels)) if pixels else 0.0, wrong / pixels if pixels else 0.0

    def lines(self):
        t = self.table.tolist()
        bg = t[-1]
        rms, wrong = self._rates(bg)
        out = [f"Char report: {bg[0]} sheets, background rms level error {rms:.4f}, wrong ink {wrong:.6f}"]
        inked = [c for c in range(len(t) - 1) if t[c][1] > 0]
        for c in sorted(inked, key=lambda c: (-(t[c][2] / t[c][1]), c))[:self.k]:
            rms, wrong = self._rates(t[c])
            out.append(f"  code {c} {chr(c)!r}: rms level error {rms:.4f}, wrong ink {wrong:.6f}, chars {t[c][0]}")
        return out

    def write_tsv(self, path):
        t = self.table.tolist()
        _write_tsv(path, ["code", "char", "chars", "pixels", "sumsq", "off2", "wrong"],
                   [[c, chr(c) if 32 < c < 127 else ""] + row for c, row in enumerate(t[:-1]) if row[1] > 0] + [["background", ""] + t[-1]])


class _PairReport:
    """AFR_PAIR_REPORT's block and pair_errors.tsv, from the pair table of a _CharErrorPass."""

    def __init__(self, k, errors, alphabet):
        from . import synth
        self.k, self.errors = int(k), errors
        self.members = synth.alphabet_members(alphabet or "upper")

    table = property(lambda self: self.errors.by_pair)

    @staticmethod
    def name(p, c):
        return f"{chr(33 + c)!r} after " + (f"{chr(32 + p)!r}" if p else "word start")

    def lines(self):
        t = self.table.tolist()
        letters = [i for i, m in enumerate(self.members) if m]
        seen = [(p, c) for p in [0] + [1 + i for i in letters] for c in letters if t[p][c][0] >= PAIR_MIN_CHARS and t[p][c][1] > 0]
        out = [f"Pair report: {len(seen)} pairs seen {PAIR_MIN_CHARS} times or more"]
        for p, c in sorted(seen, key=lambda e: (-(t[e[0]][e[1]][2] / t[e[0]][e[1]][1]), e))[:self.k]:
            chars, pixels, sumsq, wrong = t[p][c]
            out.append(f"  {self.name(p, c)}: rms level error {float(np.sqrt(sumsq / pixels)):.4f}, wrong ink {wrong / pixels:.6f}, chars {chars}")
        return out

    def write_tsv(self, path):
        _write_tsv(path, ["prev", "prev_char", "code", "char", "chars", "pixels", "sumsq", "wrong"],
                   [["" if p == 0 else 32 + p, "" if p == 0 else chr(32 + p), 33 + c, chr(33 + c)] + rec
                    for p, row in enumerate(self.table.tolist()) for c, rec in enumerate(row) if any(rec)])


class _ReadReport(_Report):
    """What AFR_READ_REPORT keeps on the device during one validation pass: afr_op_sheet_read_back's confusion table, which every
    validation batch's launch adds to (the batch's rows of the bound codes, the evaluation's bitmaps)."""
    takes_batches = needs_u8 = True

    def __init__(self, k, atlas, codes, alphabet):
        self.k, self.atlas, self.codes, self.alphabet = int(k), atlas, codes, alphabet or "upper"
        self.table = torch.zeros((atlas.n_codes, atlas.n_codes), dtype=torch.int64, device=atlas.device)
        self.reduced = (self.table,)

    def add(self, res, rows):
        from . import devdata
        if rows.numel():
            devdata.read_back(self.atlas, self.codes, res.u8.contiguous(), self.alphabet, res.u8.shape[1], res.u8.shape[2], rows=rows,
                              confusion=self.table)

    @staticmethod
    def _name(c):
        return chr(c) if 32 < c < 127 else "blank" if c == 32 else f"#{c}"

    def _confusions(self):
        """the non-zero counters off the diagonal as (count, true code, code read), the most frequent first, then by code"""
        t = self.table.cpu()
        at = torch.nonzero(t).tolist()
        return sorted(((int(t[c, r]), c, r) for c, r in at if c != r), key=lambda e: (-e[0], e[1], e[2])), t

    def line(self):
        pairs, t = self._confusions()
        scored, right, blank = int(t.sum()), int(t.diagonal().sum()), int(t[:, 32].sum())
        n = max(1, scored)
        worst = ", ".join(f"{self._name(c)}->{self._name(r)} {v}" for v, c, r in pairs[:self.k]) or "none"
        return f"Read report: {scored} characters, read right {right / n:.6f}, read blank {blank / n:.6f}, confusions: {worst}"

    def write_tsv(self, path):
        t = self.table.cpu()
        _write_tsv(path, ["code", "char", "read", "read_char", "count"],
                   [[c, chr(c) if 32 < c < 127 else "", r, chr(r) if 32 < r < 127 else "", int(t[c, r])] for c, r in torch.nonzero(t).tolist()])

    def write_strings(self, model, strings, path):
        """path: every test string, rendered by the model as render_strings renders it, beside what is read from the bitmap"""
        codes = torch.from_numpy(helpers.encode_for_model(strings, model.max_length, warn=False)).to(self.atlas.device)
        was_training = model.training
        model.eval()
        read = model.read_back(self.atlas, codes, self.alphabet).texts()
        if was_training:
            model.train()
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            for s, r in zip(strings, read):
                f.write(f"{s[:model.max_length]}\n{r}\n\n")


def _eval_weights(eng):
    """The weights evaluation is taken from: the engine's EMA when it keeps one, the weights themselves otherwise."""
    return eng.ema_weights() if eng.ema_decay is not None else contextlib.nullcontext()

random.seed(SEED)
np.random.seed(SEED)
torch.manual_seed(SEED)

_LOCAL_RANK = int(os.environ.get("LOCAL_RANK", "0"))
if torch.cuda.is_available():
    device = torch.device("cuda", _LOCAL_RANK)
    torch.cuda.set_device(device)              # one process per GPU: torch ops AND libafr launches of this process go to it
else:                                          # importable for inspection; constructing a model will raise
    device = torch.device("cpu")


def _init_distributed():
    """torchrun --nproc-per-node N model.py --train: one rank per GPU, gradients all-reduced over RCCL (parallel.py).
    Without WORLD_SIZE > 1 in the environment this is a no-op (single GPU, as the reference)."""
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 and dist.is_available() and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29512")
        dist.init_process_group("nccl", device_id=device)      # "nccl" is RCCL on ROCm

# the reference's 15 evaluation inputs (model.py:111-127): rendered every 5 epochs and at the end
test_strings = [
    "HELLO LEANN I LOVE YOU SO MUCH I HOPE YOU HAVE A GREAT DAY",
    "TWO WORLDS ONE FAMILY TRUST YOUR HEART LET FATE DECIDE TO GUIDE THESE LIVES WE SEE",
    "A PARADISE UNTOUCHED BY MAN WITHIN THIS WORLD BLESSED WITH LOVE A SIMPLE LIFE THEY LIVE IN PEACE",
    "SOFTLY TREAD THE SAND BELOW YOUR FEET NOW TWO WORLDS ONE FAMILY TRUST YOUR HEART LET FATE",
    "BENEATH THE SHELTER OF THE TREES ONLY LOVE CAN ENTER HERE A SIMPLE LIFE THEY LIVE IN PEACE",
    "THE QUICK BROWN FOX JUMPS OVER THE LAZY DOG",
    "ABCDEFGHIJKLMNOPQRSTUVWXYZ",
    "W" * 20,
    "I" * 20,
    "ALTERNATING CASE TEST   SPACES",
    "CLAUDE IS RENDERING FONTS",
    "ZYXWVUTSRQPONMLKJIHGFEDCBA",
    "AEIOU BCDFGHJKLMNPQRSTVWXYZ",
    "EXACTLY TWENTY CHARS",
    " " * 20,
]


# what an alphabet other than A-Z adds to them: a lower-case pangram, the digits, the punctuation
EXTRA_TEST_STRINGS = (
    "the quick brown fox jumps over the lazy dog",
    "0123456789",
    "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~",
)


def _extra_test_strings(alphabet):
    """EXTRA_TEST_STRINGS filtered to the alphabet's members and the space; strings nothing is left of are dropped.  None or upper: none."""
    if alphabet is None or alphabet == "upper":
        return []
    from . import synth
    members = synth.alphabet_members(alphabet)
    keep = {" "} | {chr(synth.TEXT_FIRST + i) for i, m in enumerate(members) if m}
    out = ["".join(c for c in s if c in keep).strip() for s in EXTRA_TEST_STRINGS]
    return [s for s in out if s]


# ---------------------------------------------------------------- model
class _Bag(nn.Module):
    """Names a group of parameters so that state_dict() keys match the reference's module tree."""

    def __init__(self, **tensors):
        super().__init__()
        for k, v in tensors.items():
            if isinstance(v, nn.Module):
                self.add_module(k, v)
            else:
                self.register_parameter(k, v)


def _reference_style_init(cfg):
    """Default initial values exactly as torch constructs the reference's layers, in the reference's creation order
    (model.py:136-152), so the same torch seed gives the same starting point."""
    E, F = cfg.embed_dim, cfg.fc_dim
    emb = nn.Embedding(cfg.vocab, E)
    pos = torch.zeros(cfg.max_length, E)
    nn.init.normal_(pos, mean=0, std=0.02)
    attn = nn.MultiheadAttention(embed_dim=E, num_heads=cfg.heads, dropout=cfg.p_attn)
    ln = nn.LayerNorm(E)
    fc1 = nn.Linear(E, F)
    fco = nn.Linear(F * cfg.max_length, cfg.sheet_h * cfg.sheet_w)
    return {
        "positional_encoding": pos, "embedding.weight": emb.weight.detach(),
        "attention.in_proj_weight": attn.in_proj_weight.detach(), "attention.in_proj_bias": attn.in_proj_bias.detach(),
        "attention.out_proj.weight": attn.out_proj.weight.detach(), "attention.out_proj.bias": attn.out_proj.bias.detach(),
        "layer_norm.weight": ln.weight.detach(), "layer_norm.bias": ln.bias.detach(),
        "fc1.weight": fc1.weight.detach(), "fc1.bias": fc1.bias.detach(),
        "fc_output.weight": fco.weight.detach(), "fc_output.bias": fco.bias.detach(),
    }


class _EngineForward(torch.autograd.Function):
    """forward(x) through libafr; backward routes d(loss)/d(sheet) into afr_backward and exposes the gradients as
    .grad views of the engine's flat gradient buffer (overwrite semantics == the reference's zero_grad + backward)."""

    @staticmethod
    def forward(ctx, anchor, module, x):
        step = module._next_step() if module.training else 0
        ctx.module = module
        return module.engine.forward(x, training=module.training, step=step)

    @staticmethod
    def backward(ctx, grad_out):
        m = ctx.module
        eng = m.engine
        eng.set_output_grad(grad_out.reshape(grad_out.shape[0], -1))
        eng.backward()
        for name, p in m.named_parameters():
            p.grad = eng.grads[name]
        return None, None, None


class AttentionFontRenderer(nn.Module):
    """Reference model.py:129-204.  forward(x: int64 [B,L]) -> float32 [B, SHEET_HEIGHT, SHEET_WIDTH] in [0,1];
    L > max_length is truncated, L < max_length zero-pads the flattened features; an index >= 128 raises
    IndexError (checked when `strict_indices`, default, at the cost of a device sync in eval mode only).
    loss: "mse" (clamp head, the reference's) or "bce" (sigmoid head: forward returns sigmoid(u), the fused steps train with
    binary cross-entropy on u); None takes AFR_LOSS from the environment.  state_dict() is the same for both.
    max_grad_norm: clip the gradients by their global L2 norm inside the engine's optimizer step (Engine.set_grad_clip); None
    takes AFR_CLIP_NORM from the environment (unset: off).  A torch optimizer on the autograd path clips with torch's own call.
    optimizer: "adamw" (the reference's) or "lion"; None takes AFR_OPTIMIZER from the environment.  train_attention_model steps a Lion
    model with LEARNING_RATE / 10 and WEIGHT_DECAY * 10 (the Lion paper's rule of thumb: lr * weight_decay stays what it was).
    ema_decay, ema_every: keep an exponential moving average of the weights (Engine.set_ema); ema_decay None takes AFR_EMA from the
    environment (unset: off).  train_attention_model then validates, renders and saves from the average.
    no_decay: True steps the tensors of config.no_decay_names with weight decay 0 (Engine.set_param_groups); None takes AFR_NO_DECAY=1
    from the environment (unset: off, the reference's single group)."""

    def __init__(self, max_length=MAX_CHARS_PER_SHEET, dtype=None, max_batch=1024, seed=SEED, rank=None, init=True, loss=None,
                 max_grad_norm=None, optimizer=None, ema_decay=None, ema_every=1, no_decay=None):
        super().__init__()
        from .engine import Engine
        self.max_length = max_length
        self.embedding_dim = EMBEDDING_DIM
        self.config = SheetConfig(max_length=max_length, embed_dim=EMBEDDING_DIM, heads=NUM_ATTENTION_HEADS, fc_dim=64,
                                  sheet_h=SHEET_HEIGHT, sheet_w=SHEET_WIDTH, p_embed=DROPOUT_RATE, p_attn=DROPOUT_RATE,
                                  p_fc=DROPOUT_RATE + 0.05)
        rank = int(os.environ.get("RANK", "0")) if rank is None else rank
        if ema_decay is None:
            ema_decay, ema_every = _ema_from_env()
        self.engine = Engine(self.config, dtype=dtype or COMPUTE_DTYPE, max_batch=max_batch, device=device, seed=seed, rank=rank,
                             loss=loss or COMPUTE_LOSS, max_grad_norm=CLIP_NORM if max_grad_norm is None else max_grad_norm,
                             optimizer=optimizer or COMPUTE_OPTIMIZER, ema_decay=ema_decay, ema_every=ema_every)
        self.no_decay = os.environ.get("AFR_NO_DECAY") == "1" if no_decay is None else bool(no_decay)
        if self.no_decay:
            self.engine.set_param_groups(wd_mult={name: 0.0 for name in no_decay_names(self.config)})
        self.loss = self.engine.loss
        self.optimizer = self.engine.optimizer
        self.max_grad_norm = self.engine.max_grad_norm
        P = {k: nn.Parameter(v) for k, v in self.engine.params.items()}
        self.positional_encoding = P["positional_encoding"]
        self.embedding = _Bag(weight=P["embedding.weight"])
        self.attention = _Bag(in_proj_weight=P["attention.in_proj_weight"], in_proj_bias=P["attention.in_proj_bias"],
                              out_proj=_Bag(weight=P["attention.out_proj.weight"], bias=P["attention.out_proj.bias"]))
        self.layer_norm = _Bag(weight=P["layer_norm.weight"], bias=P["layer_norm.bias"])
        self.fc1 = _Bag(weight=P["fc1.weight"], bias=P["fc1.bias"])
        self.fc_output = _Bag(weight=P["fc_output.weight"], bias=P["fc_output.bias"])
        self.strict_indices = True
        self._steps = 0
        self._seen_versions = None
        if init:
            self.engine.load_params(_reference_style_init(self.config))

    def _param_versions(self):
        return tuple(p._version for p in self.parameters())

    def _refresh_shadow_if_params_changed(self):
        """bf16 mode: the GEMMs read a bf16 shadow of the f32 masters that only libafr's own AdamW keeps current.  A stock
        torch optimizer (or any in-place edit of a Parameter) bumps the tensor's version counter; when the counters moved
        since the last forward the shadow is re-derived first, so the next forward sees the new weights."""
        if self.engine.dtype not in ("bf16", "bfloat16"):
            return
        v = self._param_versions()
        if v != self._seen_versions:
            self.engine.sync_params()
            self._seen_versions = v

    def _next_step(self):
        self._steps += 1
        return self._steps

    def tensor_stats(self, which="grads", minus=None):
        """Per-tensor statistics of the engine's flat buffer `which` (or of its difference to `minus`), computed on the device:
        Engine.tensor_stats.  The record buffer is allocated once and reused."""
        return self.engine.tensor_stats(which, minus)

    def render_u8(self, codes):
        """uint8 [B, SHEET_HEIGHT, SHEET_WIDTH] on the device: binary_array_to_image's levels of the eval-mode forward(codes), quantised
        by the library (Engine.render_u8) instead of on the host.  The same shape, shadow-refresh and index checks as forward."""
        if codes.dim() != 2:
            raise ValueError(f"expected [batch, seq_len] codes, got shape {tuple(codes.shape)}")
        self._refresh_shadow_if_params_changed()
        q = self.engine.render_u8(codes)
        if self.strict_indices and self.engine.error_flags():
            raise IndexError("index out of range in self")          # what nn.Embedding raises in the reference
        return q

    def char_errors(self, atlas, codes):
        """devdata.char_errors of render_u8(codes) against the sheets the atlas composes for the same codes: the rendering error charged
        to the character that owns each pixel.  Returns a devdata.CharErrors."""
        from . import devdata
        q = self.render_u8(codes)
        return devdata.char_errors(atlas, codes, q, q.shape[1], q.shape[2])

    def read_back(self, atlas, codes, alphabet="upper"):
        """devdata.read_back of render_u8(codes): for every character the atlas draws for the same codes, which candidate glyph of
        `alphabet` (or the blank, or the character itself) explains the rendered pixels best.  Returns a devdata.ReadBack."""
        from . import devdata
        q = self.render_u8(codes)
        return devdata.read_back(atlas, codes, q, alphabet, q.shape[1], q.shape[2])

    def forward(self, x):
        if x.dim() != 2:
            raise ValueError(f"expected [batch, seq_len] codes, got shape {tuple(x.shape)}")
        self._refresh_shadow_if_params_changed()
        if torch.is_grad_enabled() and self.training:
            y = _EngineForward.apply(self.positional_encoding, self, x)
        else:
            y = self.engine.forward(x, training=self.training, step=self._next_step() if self.training else 0)
        if self.strict_indices and not self.training and self.engine.error_flags():
            raise IndexError("index out of range in self")          # what nn.Embedding raises in the reference
        return y

    # the parameters live in HBM inside the engine: moving the module is a no-op
    def to(self, *args, **kwargs):
        return self

    def cuda(self, device=None):
        return self

    def cpu(self):
        return self

    def load_state_dict(self, state_dict, strict=True, assign=False):
        out = super().load_state_dict(state_dict, strict=strict, assign=False)
        self.engine.sync_params()                                  # refresh bf16 shadows
        if self.engine.flat_ema is not None:
            self.engine.reset_ema()                                # the average restarts from the loaded weights
        return out


# ---------------------------------------------------------------- data order (random_split + DataLoader, on device)
class _EpochOrder:
    """Reproduces which samples the reference trains/validates on and in which order (model.py:232-266):
    random_split(generator=manual_seed(42)) is one randperm; per epoch, from the generator the two loaders share,
    each DataLoader iterator draws one base-seed integer and RandomSampler draws two randperms (the second is its
    empty remainder).  Checked against the real loaders in tests/test_host_cpu.py (torch 2.10 sampler internals)."""

    def __init__(self, n, val_fraction=VALIDATION_SPLIT, seed=SEED):
        self.val_size = int(val_fraction * n)
        self.train_size = n - self.val_size
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
        self.train_idx, self.val_idx = perm[:self.train_size], perm[self.train_size:]
        self.g = torch.Generator()
        self.g.manual_seed(seed)

    def _iterator_seed(self):
        torch.empty((), dtype=torch.int64).random_(generator=self.g)

    def train_epoch(self):
        self._iterator_seed()
        perm = torch.randperm(self.train_size, generator=self.g)
        torch.randperm(self.train_size, generator=self.g)      # RandomSampler's remainder draw (sliced to length 0)
        return self.train_idx[perm]

    def val_epoch(self):
        self._iterator_seed()
        return self.val_idx


def _num_batches(n, bs):
    return (n + bs - 1) // bs


def _dist():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return dist, dist.get_world_size(), dist.get_rank()
    return None, 1, 0


def _step_hyper(eng, lr):
    """(lr, weight_decay) of one optimizer step at the schedule's learning rate: AdamW takes them as they are, Lion a tenth of the
    learning rate and ten times the decay (Chen et al. 2023, section 5: its sign update has a larger norm than AdamW's)."""
    if eng.optimizer == "lion":
        return lr / 10, WEIGHT_DECAY * 10
    return lr, WEIGHT_DECAY


def _batch_calls(eng, stepper, inputs, targets, rows):
    """The calls of one batch, bound to what they run on: the data-set rows `rows` themselves when inputs is None (the engine has the
    data set bound), else the dense tensors gathered from inputs and targets with index_select (targets None: the codes alone).  The one
    place an epoch chooses between the two forms.  step(mean_elems, **hyper) is the stepper's, the others are the engine's."""
    from functools import partial
    from types import SimpleNamespace
    if inputs is None:
        return SimpleNamespace(step=partial(stepper.step_rows, rows) if stepper else None, forward=partial(eng.forward_rows, rows),
                               evaluate_last=partial(eng.evaluate_last, rows=rows), loss_grad=partial(eng.loss_grad_rows, rows),
                               evaluate=partial(eng.evaluate_rows, rows), forward_loss=partial(eng.forward_loss_rows, rows))
    x, t = inputs.index_select(0, rows), None if targets is None else targets.index_select(0, rows)
    return SimpleNamespace(step=partial(stepper.step, x, t, None) if stepper else None, forward=partial(eng.forward, x),
                           evaluate_last=partial(eng.evaluate_last, target=t), loss_grad=partial(eng.loss_grad, t),
                           evaluate=partial(eng.evaluate, x), forward_loss=partial(eng.forward_loss, x, t))


def _run_epoch(model, stepper, order, inputs, targets, batch_size, lr, rank, world, by_rows=True, reports=()):
    """One epoch of the reference loop (model.py:288-333): the training pass over order.train_epoch(), then the validation
    pass; returns the two means of per-batch mean losses.  An engine that keeps a weight EMA validates from it.  by_rows: the engine has the data set bound (Engine.bind_dataset)
    and every step is driven by this rank's slice of the epoch's index vector -- the kernels read the rows where they lie.
    by_rows=False gathers each batch with index_select and hands the step dense tensors (the form tools/epoch_bench.py
    measures the other against).  reports: _Report objects, whose hooks are called in list order at their moments of the epoch; every
    rank passes the same list but for reports that issue no collective.  Those that take batches share one evaluation per validation
    batch, between its forward and its loss, with bitmaps if one of them reads bitmaps.  Without reports: the pass as it always was."""
    from .parallel import shard_rows
    eng = model.engine
    pixels = targets[0].numel()
    dense = (None, None) if by_rows else (inputs, targets)
    model.train()
    idx = order.train_epoch().to(inputs.device)
    nb = _num_batches(order.train_size, batch_size)
    for b in range(nb):
        rows = idx[b * batch_size:(b + 1) * batch_size]
        mine = rows[shard_rows(rows.numel(), rank, world)]
        step_lr, step_wd = _step_hyper(eng, lr)
        hyper = dict(step=model._next_step(), lr=step_lr, betas=ADAM_BETAS, weight_decay=step_wd)
        for r in reports:
            r.before_step(b, nb, mine, rows.numel() * pixels)
        _batch_calls(eng, stepper, *dense, mine).step(rows.numel() * pixels, **hyper)
        for r in reports:
            r.after_step(b, nb, mine, rows.numel() * pixels)
    avg_train_loss = stepper.global_loss() / nb                 # mean of per-batch means (model.py:311,333)

    model.eval()
    vidx = order.val_epoch().to(inputs.device)
    nvb = _num_batches(order.val_size, batch_size)
    takers = [r for r in reports if r.takes_batches]
    want_u8 = any(r.needs_u8 for r in takers)
    with _eval_weights(eng):
        for b in range(nvb):
            rows = vidx[b * batch_size:(b + 1) * batch_size]
            mine = rows[shard_rows(rows.numel(), rank, world)]
            calls = _batch_calls(eng, None, *dense, mine)
            calls.forward(training=False, want_output=False)
            if takers:
                res = calls.evaluate_last(want_u8=want_u8)
                for r in takers:
                    r.add(res, mine)
            calls.loss_grad(mean_elems=rows.numel() * pixels)
        for r in reports:
            r.end_validation(_dist()[0] if world > 1 else None, rank,
                             lambda rows: _batch_calls(eng, None, dense[0], None, rows).evaluate(want_u8=True))
    avg_val_loss = stepper.global_loss() / max(nvb, 1)
    for r in reports:
        r.end_epoch(*dense)
    return avg_train_loss, avg_val_loss


def _fresh_rows(atlas, n, alphabet=None, steer=0.0, steer_pairs=0.0):
    """AFR_FRESH_DATA: refresh(epoch, rows, inputs, targets, by_code=None, by_pair=None) rewrites rows `rows` of the bound codes and sheets in place, on
    the current stream: row r becomes the text of seed DATA_FIRST_SEED + epoch * n + r, as long as a row of inputs is wide at the most, and
    its sheet.  alphabet (AFR_ALPHABET) or steer (AFR_STEER) take the texts from the weighted source: equal weights over the alphabet
    (A-Z without one), or -- given by_code, the by-code table of the last validation pass -- _steer_weights(steer) of it.  The table, the
    letter weights and the texts follow one another on the stream: nothing is read back.  refresh.w and refresh.by_code hold the last
    rewrite's weights and the table they were built from.  steer_pairs (AFR_STEER_PAIRS) with by_pair, the pair table of the last
    validation pass: the texts come from the Markov source instead, _steer_weights(steer_pairs) of the pairs' errors with
    PAIR_MIN_CHARS; refresh.w2 and refresh.by_pair then hold the last rewrite's pair weights and their table."""
    from . import devdata, synth
    members = synth.alphabet_members(alphabet or "upper") if alphabet or steer or steer_pairs else None

    def refresh(epoch, rows, inputs, targets, by_code=None, by_pair=None):
        rows = rows.to(device)
        cum = cum2 = None
        if steer_pairs and by_pair is not None:
            cum2, refresh.w2 = devdata.pair_weights(members, by_pair, *_steer_weights(steer_pairs), min_chars=PAIR_MIN_CHARS, device=device)
            refresh.by_pair = by_pair
        elif members is not None:
            floor_w, gain = _steer_weights(steer) if by_code is not None else (STEER_UNIT, 0)
            cum, refresh.w = devdata.text_weights(members, by_code, floor_w, gain, device=device)
            refresh.by_code = by_code
        devdata.generate_codes(rows.numel(), DATA_FIRST_SEED, max_length=inputs.shape[1], out=inputs, rows=rows, seed_rows=epoch * n + rows, cum=cum,
                               cum2=cum2, check_total=False)
        devdata.compose_sheets(atlas, inputs.index_select(0, rows), targets.shape[1], targets.shape[2], out=targets, rows=rows)
    refresh.w = refresh.by_code = refresh.w2 = refresh.by_pair = None
    return refresh


def _steer_line(share, w, k=5):
    """The status line of AFR_STEER, read from the weights of the last rewrite (int32 [94] on the device): the one host read steering adds."""
    w = w.tolist()
    top = sorted((i for i in range(len(w)) if w[i]), key=lambda i: (-w[i], i))[:k]
    return f"Steer: share {share:g}, heaviest {len(top)} codes " + ", ".join(f"{33 + i} {chr(33 + i)!r} x{w[i] / STEER_UNIT:.2f}" for i in top)


def _steer_pairs_line(share, w2, k=5):
    """The status line of AFR_STEER_PAIRS, read from the pair weights of the last rewrite (int32 [95, 94] on the device): the one host
    read pair steering adds."""
    w2 = w2.tolist()
    top = sorted(((p, c) for p in range(len(w2)) for c in range(len(w2[p])) if w2[p][c]), key=lambda e: (-w2[e[0]][e[1]], e))[:k]
    return f"Steer pairs: share {share:g}, heaviest {len(top)} pairs " + ", ".join(f"{_PairReport.name(p, c)} x{w2[p][c] / STEER_UNIT:.2f}" for p, c in top)


def _optional_config_lines(eng, fresh):
    """The lines of config.txt that only a run with a non-default setting has, in their fixed order, from one table of (key, value or
    None, format): a default run's artefacts stay as they were.  The switches are read as they stand when this runs."""
    ema = eng.ema_decay is not None
    table = (("loss", eng.loss if eng.loss != "mse" else None, ""), ("optimizer", eng.optimizer if eng.optimizer != "adamw" else None, ""),
             ("max_grad_norm", eng.max_grad_norm or None, "g"), ("ema_decay", eng.ema_decay, "g"), ("ema_every", eng.ema_every if ema else None, ""),
             ("val_report", VAL_REPORT or None, ""), ("tensor_report", 1 if TENSOR_REPORT else None, ""), ("device_data", DEVICE_DATA or None, ""),
             ("fresh_data", 1 if fresh else None, ""), ("char_report", CHAR_REPORT or None, ""), ("alphabet", ALPHABET or None, ""),
             ("steer", STEER or None, "g"), ("read_report", READ_REPORT or None, ""), ("pair_report", PAIR_REPORT or None, ""),
             ("steer_pairs", STEER_PAIRS or None, "g"))
    return [f"{key} = {value:{fmt}}" for key, value, fmt in table if value is not None]


def _check_switches(atlas, refresh):
    """What the reports and the steering need of a training run, from one table of (switch, what is missing, message); the first that is
    on without it is a ValueError.  The switches are read as they stand when this runs."""
    no_atlas, no_rewrite = atlas is None, atlas is None or refresh is None
    for on, missing, message in (
            (CHAR_REPORT, no_atlas, "the character report needs the glyph atlas the data set was composed from (AFR_DEVICE_DATA)"),
            (READ_REPORT, no_atlas, "the read-back report needs the glyph atlas the data set was composed from (AFR_DEVICE_DATA)"),
            (STEER, no_rewrite, "steering needs the glyph atlas and the fresh-data rewrite (AFR_DEVICE_DATA, AFR_FRESH_DATA)"),
            (PAIR_REPORT, no_atlas, "the pair report needs the glyph atlas the data set was composed from (AFR_DEVICE_DATA)"),
            (STEER_PAIRS, no_rewrite, "pair steering needs the glyph atlas and the fresh-data rewrite (AFR_DEVICE_DATA, AFR_FRESH_DATA)"),
            (STEER_PAIRS, bool(STEER), "AFR_STEER_PAIRS and AFR_STEER together: the fresh texts are drawn from one table")):
        if on and missing:
            raise ValueError(message)


def _epoch_reports(model, atlas, inputs, targets, refresh, strings, epoch, rank, world):
    """The reports of one epoch, from the switches as they stand when this runs -> (reports, blocks, errors): the list _run_epoch drives;
    what rank 0 prints after a status line, in its fixed order, as pairs (lines() -> the lines to print, artefacts(folder) -> the files
    of the epoch's output folder, or None); and the _CharErrorPass among the reports (or None), whose tables the steering of the next
    epoch reads.  The reports that only print are built on the epochs that print a status line; the validation report and the tables of
    the steering are kept every epoch."""
    status, eng = epoch % 5 == 0, model.engine
    reports, blocks = [], []
    if VAL_REPORT:
        val = _ValReport(VAL_REPORT, device, bitmaps=status)
        reports.append(val)

        def worst_bitmaps(out):
            for j in range(0 if val.u8 is None else val.u8.shape[0]):
                helpers.u8_array_to_image(val.u8[j].cpu().numpy(), f"{out}/val_worst_{j}.bmp")
        blocks.append((lambda: [val.line(targets[0].numel(), world)], worst_bitmaps))
    if TENSOR_REPORT and rank == 0 and status:
        reports.append(_TensorReport(model))
        blocks.append((reports[-1].lines, None))
    char_lines, pair_lines = bool(CHAR_REPORT) and status, bool(PAIR_REPORT) and status
    errors = None
    if char_lines or STEER or pair_lines or STEER_PAIRS:
        errors = _CharErrorPass(atlas, inputs, by_code=char_lines or bool(STEER), pairs=pair_lines or bool(STEER_PAIRS))
        reports.append(errors)
    if char_lines:
        chars = _CharReport(CHAR_REPORT, errors)
        blocks.append((chars.lines, lambda out: chars.write_tsv(f"{out}/char_errors.tsv")))
    if STEER:
        blocks.append((lambda: [_steer_line(STEER, refresh.w)] if refresh.w is not None else [], None))
    if pair_lines:
        pairs = _PairReport(PAIR_REPORT, errors, ALPHABET)
        blocks.append((pairs.lines, lambda out: pairs.write_tsv(f"{out}/pair_errors.tsv")))
    if STEER_PAIRS:
        blocks.append((lambda: [_steer_pairs_line(STEER_PAIRS, refresh.w2)] if refresh.w2 is not None else [], None))
    if READ_REPORT and status:
        read = _ReadReport(READ_REPORT, atlas, inputs, ALPHABET)
        reports.append(read)

        def read_files(out):
            read.write_tsv(f"{out}/confusion.tsv")
            with _eval_weights(eng):
                read.write_strings(model, strings, f"{out}/read_back.txt")
        blocks.append((lambda: [read.line()], read_files))
    return reports, blocks, errors


def train_attention_model(model, dataset, batch_size, refresh=None, atlas=None):
    """Reference model.py:209-384: config.txt, 80/20 split, AdamW + ReduceLROnPlateau + early stopping, progress
    prints and test-string dumps every 5 epochs, training_results.txt.  Returns the model.  refresh (AFR_FRESH_DATA, _fresh_rows): called
    before every epoch >= 1 with the training rows of the split and the bound tensors, which it rewrites in place.  atlas: the glyph
    atlas the data set was composed from (AFR_CHAR_REPORT needs it)."""
    from .parallel import DataParallelStepper
    dist, world, rank = _dist()
    eng = model.engine
    os.makedirs(OUTPUT_DIR, exist_ok=True)
    if rank == 0:
        with open(f"{OUTPUT_DIR}/config.txt", "w") as f:
            f.write("# Training configuration\n")
            for k, v in (("num_epochs", NUM_EPOCHS), ("learning_rate", LEARNING_RATE), ("batch_size", batch_size),
                         ("early_stopping_patience", EARLY_STOPPING_PATIENCE), ("validation_split", VALIDATION_SPLIT),
                         ("weight_decay", WEIGHT_DECAY), ("embedding_dim", EMBEDDING_DIM), ("dropout_rate", DROPOUT_RATE),
                         ("num_attention_heads", NUM_ATTENTION_HEADS), ("max_length", model.max_length),
                         ("max_chars_per_sheet", MAX_CHARS_PER_SHEET), ("num_samples", NUM_SAMPLES), ("data_size", len(dataset)),
                         ("random_seed", SEED), ("sheet_height", SHEET_HEIGHT), ("sheet_width", SHEET_WIDTH)):
                f.write(f"{k} = {v}\n")
            f.write("".join(line + "\n" for line in _optional_config_lines(eng, refresh is not None)))
    _check_switches(atlas, refresh)
    strings = test_strings + _extra_test_strings(ALPHABET)
    pair_table = None                           # AFR_STEER_PAIRS: the pair table the last validation pass left on the device
    steer_table = None                          # AFR_STEER: the by-code table the last validation pass left on the device

    order = _EpochOrder(len(dataset))
    print(f"Dataset split: {order.train_size} training samples, {order.val_size} validation samples")

    # the whole dataset becomes HBM resident: codes int64 [N, L], sheets uint8 [N, H, W] when they are 8-bit exact
    inputs, targets = dataset.tensors
    inputs = inputs.to(device)
    t8 = helpers.targets_as_uint8(targets)
    targets = (t8 if t8 is not None else targets.to(torch.float32)).to(device)
    eng.bind_dataset(inputs, targets)       # a batch is a vector of row indices from here on: nothing is gathered per step

    # ReduceLROnPlateau is host logic on one float; torch's own class drives it through a one-parameter stand-in
    lr_holder = torch.optim.SGD([nn.Parameter(torch.zeros(1))], lr=LEARNING_RATE)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(lr_holder, mode="min", factor=SCHEDULER_FACTOR,
                                                           patience=SCHEDULER_PATIENCE, min_lr=MIN_LEARNING_RATE)
    stepper = DataParallelStepper(eng, dist, world)
    best_val_loss = float("inf")
    patience_counter = 0
    best_model_state = None

    # what the model holds when training ends: the (aliased, see below) best state, or -- with a weight EMA -- the average, which the
    # final render and font_renderer.pth are then taken from (the checkpoint layout is the same)
    def final_state():
        return eng.ema_state_dict() if eng.ema_decay is not None else best_model_state

    epoch = -1
    for epoch in range(NUM_EPOCHS):
        lr = lr_holder.param_groups[0]["lr"]
        reports, blocks, errors = _epoch_reports(model, atlas, inputs, targets, refresh, strings, epoch, rank, world)
        if refresh is not None and epoch >= 1:
            refresh(epoch, order.train_idx, inputs, targets, by_code=steer_table, by_pair=pair_table)
        avg_train_loss, avg_val_loss = _run_epoch(model, stepper, order, inputs, targets, batch_size, lr, rank, world, by_rows=True, reports=reports)

        if STEER:
            steer_table = errors.by_code
        if STEER_PAIRS:
            pair_table = errors.by_pair
        scheduler.step(avg_val_loss)
        is_best = avg_val_loss < best_val_loss
        if is_best:
            best_val_loss = avg_val_loss
            patience_counter = 0
            # The reference keeps `model.state_dict().copy()` (model.py:344): a shallow copy whose tensors alias the
            # live parameters, so "restoring the best state" later is a no-op.  Reproduced: keep aliases, not clones.
            best_model_state = dict(model.state_dict())
        else:
            patience_counter += 1

        if rank == 0:
            if epoch % 5 == 0:
                status = (f"Epoch {epoch}, Train Loss: {avg_train_loss:.6f}, Val Loss: {avg_val_loss:.6f}, "
                          f"LR: {lr_holder.param_groups[0]['lr']:.6f}")
                if is_best:
                    status += " (New Best)"
                print(status)
                for lines, artefacts in blocks:
                    text = lines()
                    if text:
                        print("\n".join(text))
                    if artefacts is not None:
                        artefacts(f"{OUTPUT_DIR}/epoch_{epoch}")
                with _eval_weights(eng):
                    render_strings(model, strings, output_dir=f"{OUTPUT_DIR}/epoch_{epoch}", sheet_height=SHEET_HEIGHT,
                                   sheet_width=SHEET_WIDTH, device=device)
            elif is_best:
                print(f"Epoch {epoch}, New best validation loss: {avg_val_loss:.6f}")
        if patience_counter >= EARLY_STOPPING_PATIENCE:
            if rank == 0:
                print(f"Early stopping at epoch {epoch}, Best Val Loss: {best_val_loss:.6f}")
            model.load_state_dict(final_state())
            break

    if best_model_state is not None and patience_counter < EARLY_STOPPING_PATIENCE:
        model.load_state_dict(final_state())
        if rank == 0:
            print(f"Training completed, Best Val Loss: {best_val_loss:.6f}")

    if rank == 0:
        final_epoch = epoch + 1 if patience_counter < EARLY_STOPPING_PATIENCE else epoch
        with open(f"{OUTPUT_DIR}/training_results.txt", "w") as f:
            f.write("# Training Results\n")
            f.write(f"final_epoch = {final_epoch}\n")
            f.write(f"best_validation_loss = {best_val_loss:.6f}\n")
            f.write(f"final_learning_rate = {lr_holder.param_groups[0]['lr']:.6f}\n")
            f.write(f"early_stopped = {patience_counter >= EARLY_STOPPING_PATIENCE}\n")
            f.write(f"training_duration_epochs = {final_epoch}\n")
            f.write(f"training_completed = {datetime.datetime.now().strftime('%Y-%m-%d %H:%M:%S')}\n")
    return model


def train_string_renderer():
    """Reference model.py:389-421."""
    print("Creating sheet dataset...")
    refresh = atlas = None
    if DEVICE_DATA:
        from . import datagen, devdata
        atlas = devdata.GlyphAtlas.from_font(None if DEVICE_DATA == "default" else DEVICE_DATA, datagen.FONT_SIZE).to(device)
        print(f"Composing {NUM_SAMPLES} samples on {device} from a glyph atlas of {DEVICE_DATA}...")
        dataset = devdata.reference_dataset(NUM_SAMPLES, atlas, DATA_FIRST_SEED, MAX_CHARS_PER_SHEET, SHEET_HEIGHT, SHEET_WIDTH, alphabet=ALPHABET)
        if FRESH_DATA:
            refresh = _fresh_rows(atlas, NUM_SAMPLES, ALPHABET, STEER, STEER_PAIRS)
    else:
        dataset = load_string_dataset(data_dir="train_input", num_samples=NUM_SAMPLES, sheet_height=SHEET_HEIGHT,
                                      sheet_width=SHEET_WIDTH)
    print("Training attention-based sheet renderer with reduced embedding dimensions (32) and learned positional encoding...")
    batch_size = 1024                                              # the reference's GPU batch size (model.py:408-409)
    model = AttentionFontRenderer(max_length=MAX_CHARS_PER_SHEET, max_batch=batch_size)
    model = model.to(device)
    print(f"Using batch size {batch_size}")
    return train_attention_model(model, dataset, batch_size, refresh, atlas)


def main(argv=None):
    """The reference's __main__ block (model.py:425-454)."""
    argv = sys.argv if argv is None else argv
    _init_distributed()
    print(f"Using HIP device: {torch.cuda.get_device_name(device) if torch.cuda.is_available() else 'none'}")
    print(f"Device: {device}")
    os.makedirs(OUTPUT_DIR, exist_ok=True)
    if len(argv) > 1:
        if argv[1] == "--train":
            model = train_string_renderer()
            save_model(model)
            render_strings(model, test_strings + _extra_test_strings(ALPHABET), output_dir=OUTPUT_DIR, sheet_height=SHEET_HEIGHT, sheet_width=SHEET_WIDTH,
                           device=device)
        else:
            print(f"Unknown option: {argv[1]}")
            print("Available options: --train")
            sys.exit(1)
    else:
        if os.path.exists(MODEL_FILENAME):
            model = load_model(AttentionFontRenderer, MAX_CHARS_PER_SHEET, device=device)
        else:
            print("No saved model found. Training a new model...")
            model = train_string_renderer()
            save_model(model)
        render_strings(model, test_strings + _extra_test_strings(ALPHABET), output_dir=OUTPUT_DIR, sheet_height=SHEET_HEIGHT, sheet_width=SHEET_WIDTH,
                       device=device)
