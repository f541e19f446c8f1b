"""Host-side driver of libafr.so: owns the device buffers (as PyTorch-ROCm tensors -- torch is only
the allocator and the stream provider here) and mirrors one training iteration of the reference
loop body (model.py:292-310) as forward -> loss_grad -> backward -> [all-reduce] -> adamw.

Needs a GPU and the built extension; raises otherwise (no CPU path).
"""
import contextlib
import ctypes as C

import numpy as np
import torch

from . import _lib
from .config import GlyphConfig, PixelConfig, SheetConfig

_DT = {"f32": _lib.AFR_F32, "fp32": _lib.AFR_F32, "float32": _lib.AFR_F32, "bf16": _lib.AFR_BF16, "bfloat16": _lib.AFR_BF16,
       "bf16x3": _lib.AFR_BF16X3}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream(device=None):
    """The caller's current stream ON `device` (torch.cuda.current_stream() alone is the stream of the process's current
    device, which is GPU 0 unless somebody called set_device)."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def make_afr_config(cfg, dtype, max_batch, seed=42, rank=0, flags=0, loss="mse"):
    """loss: "mse" (clamp head + MSE, the reference's) or "bce" (sigmoid head + binary cross-entropy on the logits)."""
    c = _lib.AfrConfig()
    c.loss = _lib.loss_kind(loss)
    c.reserved = int(flags)          # include/afr.h: bit 0 un-fused optimizer, bit 1 no grouped GEMM launches, bit 2 no fused small-net step
    c.dtype = _DT[dtype]
    c.max_batch = int(max_batch)
    c.vocab = cfg.vocab
    c.embed_dim = getattr(cfg, "embed_dim", 0)      # (PixelConfig: d_model, set below)
    c.seed = int(seed)
    c.rank = int(rank)
    if isinstance(cfg, SheetConfig):
        c.kind = _lib.AFR_KIND_SHEET
        c.out_h, c.out_w = cfg.sheet_h, cfg.sheet_w
        c.max_length, c.heads, c.fc_dim = cfg.max_length, cfg.heads, cfg.fc_dim
        c.p_embed, c.p_attn, c.p_fc, c.ln_eps = cfg.p_embed, cfg.p_attn, cfg.p_fc, cfg.ln_eps
    elif isinstance(cfg, GlyphConfig):
        c.kind = _lib.AFR_KIND_GLYPH
        c.out_h, c.out_w = cfg.out_h, cfg.out_w
        c.n_hidden = len(cfg.hidden)
        for i, h in enumerate(cfg.hidden):
            c.hidden[i] = h
        c.n_fonts = cfg.n_fonts
    elif isinstance(cfg, PixelConfig):
        c.kind = _lib.AFR_KIND_PIXEL                 # BASELINE configs[4] (include/afr.h)
        c.embed_dim = cfg.d_model
        c.out_h, c.out_w = cfg.out_h, cfg.out_w
        c.heads, c.fc_dim, c.n_hidden, c.n_fonts, c.ln_eps = cfg.heads, cfg.ff_dim, cfg.layers, cfg.n_fonts, cfg.ln_eps
    else:
        raise TypeError(f"unknown config {type(cfg)}")
    return c


class EvalResult:
    """What Engine.evaluate* returns, device tensors: loss_rows float32 [B] (per-sample mean loss), stats int64 [B, 4] (pixels off by
    >= 1 level, by >= 2 levels, the largest level difference, wrong-ink pixels: include/afr.h afr_eval) -- both None without a target --
    and u8 uint8 [B, H, W], the levels a BMP dump would hold, or None when not asked for."""
    __slots__ = ("loss_rows", "stats", "u8")

    def __init__(self, loss_rows, stats, u8):
        self.loss_rows, self.stats, self.u8 = loss_rows, stats, u8

    @staticmethod
    def cat(parts):
        def j(ts):
            return None if ts[0] is None else torch.cat(ts)
        return EvalResult(j([r.loss_rows for r in parts]), j([r.stats for r in parts]), j([r.u8 for r in parts]))


class TensorStats:
    """What Engine.tensor_stats returns: one record per parameter tensor (include/afr.h afr_tensor_stat).  raw is the [n, 8] int32
    tensor the library wrote, on the device (the engine keeps one per kind of request and writes the next request of that kind into
    it again: read it before asking once more); names the tensor names in the same order.  cpu() makes the one synchronising copy and
    returns self; after it sumsq, sum, min, max (float32) and n_nan, n_inf, n_zero, numel (uint32) are numpy views of that copy."""
    FLOATS, COUNTS = ("sumsq", "sum", "min", "max"), ("n_nan", "n_inf", "n_zero", "numel")

    def __init__(self, raw, names):
        self.raw, self.names, self._host = raw, list(names), None

    def cpu(self):
        if self._host is None:
            a = self.raw.cpu().numpy() if isinstance(self.raw, torch.Tensor) else np.asarray(self.raw)
            if a.dtype != np.int32 or a.ndim != 2 or a.shape != (len(self.names), 8):
                raise ValueError(f"expected an int32 array of shape ({len(self.names)}, 8), got {a.dtype} {a.shape}")
            self._host = np.ascontiguousarray(a)
            f, u = self._host.view(np.float32), self._host.view(np.uint32)
            for i, k in enumerate(self.FLOATS):
                setattr(self, k, f[:, i])
            for i, k in enumerate(self.COUNTS):
                setattr(self, k, u[:, 4 + i])
        return self

    def norm(self):
        """sqrt(sumsq) per tensor, float64."""
        return np.sqrt(self.cpu().sumsq.astype(np.float64))

    def nonfinite(self):
        """The names of the tensors that hold a NaN or an infinity."""
        h = self.cpu()
        return [nm for nm, a, b in zip(self.names, h.n_nan, h.n_inf) if int(a) + int(b) > 0]


class Engine:
    """One plan + its device buffers.  `params[name]` are views into the flat float32 buffer in
    state_dict order, so checkpoints interchange with the reference (helpers.py:76-105)."""

    def __init__(self, cfg, dtype="f32", max_batch=1024, device=None, seed=42, rank=0, with_optimizer=True, flags=0, micro_batch=None,
                 loss="mse", max_grad_norm=None, optimizer="adamw", ema_decay=None, ema_every=1, lr_mult=None, wd_mult=None):
        """lr_mult, wd_mult: optimizer groups (set_param_groups): dicts of tensor name -> multiplier of the step's lr / weight decay;
        None = the reference's single group.
        ema_decay: keep an exponential moving average of the weights (set_ema); None = off.  ema_every: update it every that many
        optimizer steps.
        optimizer: "adamw" (torch.optim.AdamW, the reference's) or "lion" (one moment, sign update: include/afr.h afr_set_optimizer);
        every optimizer step of the engine follows it, and a Lion engine allocates no exp_avg_sq.
        max_grad_norm: clip the gradients by their global L2 norm inside every optimizer step (set_grad_clip); None or 0 = off.
        micro_batch: train_step / forward_loss + backward of a batch larger than this many samples run as micro-steps of at
        most that many, their gradients summed (gradient accumulation: the saved activations of BASELINE configs[4]'s 2048
        glyphs per GPU would be 800 GB; 32 at a time they are 12.6 GB).  The plan is then sized for micro_batch, not max_batch."""
        if not torch.cuda.is_available():
            raise RuntimeError("ai_font_renderer_amd.Engine needs an MI355X: the hot path has no CPU fallback")
        _lib.loss_kind(loss)          # ValueError for anything but "mse" | "bce"
        self.loss = loss
        _lib.opt_kind(optimizer)      # ValueError for anything but "adamw" | "lion"
        self.optimizer = optimizer
        self.lib = _lib.lib()
        self.micro_batch = int(micro_batch) if micro_batch else None
        if self.micro_batch:
            max_batch = min(int(max_batch), self.micro_batch)
        self._grad_acc = None
        self.cfg, self.dtype, self.max_batch = cfg, dtype, int(max_batch)
        self.seed, self.rank, self.flags = int(seed), int(rank), int(flags)
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self._plan = None
        self.max_grad_norm = self._check_clip(max_grad_norm)
        self._clip_stats = None     # device float[2] the library writes (total_norm, coef) into on a clipping plan
        self._ds = None       # the bound data set: (x, font, target, target dtype code, rows, L), see bind_dataset
        # the weight EMA (set_ema): flat_ema in the parameter layout, ema_params its views; _ema_on inside ema_weights()
        self.ema_decay, self.ema_every = self._check_ema(ema_decay, ema_every)
        self.flat_ema, self.ema_params, self._ema_on = None, {}, False
        self.lr_mult, self.wd_mult, self._ranges = None, None, None      # optimizer groups (set_param_groups); _ranges: the plan's merged table
        self.layout = None          # read from the plan below, once it is bound
        self._make_plan(self.max_batch)
        n = self.lib.afr_param_elems(self._plan)
        self.n_flat = int(n)
        with torch.cuda.device(self.device):
            self.flat_params = torch.zeros(n, dtype=torch.float32, device=self.device)
            self.flat_grads = torch.zeros(n, dtype=torch.float32, device=self.device)
            self.exp_avg = torch.zeros(n, dtype=torch.float32, device=self.device) if with_optimizer else None
            self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=self.device) if with_optimizer and optimizer == "adamw" else None
            self.loss_accum = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._bind()
        self.layout = []
        name = C.create_string_buffer(128)
        off, numel, ndim = C.c_int64(), C.c_int64(), C.c_int32()
        shape = (C.c_int64 * 4)()
        for i in range(self.lib.afr_param_count(self._plan)):
            _lib.check(self.lib.afr_param_info(self._plan, i, name, 128, C.byref(off), C.byref(numel), C.byref(ndim), shape))
            self.layout.append((name.value.decode(), tuple(shape[k] for k in range(ndim.value)), off.value, numel.value))
        self.names = [nm for nm, _, _, _ in self.layout]
        self.params, self.grads = self._views(self.flat_params), self._views(self.flat_grads)
        self.pixels = cfg.pixels
        self._hw = (self._c.out_h, self._c.out_w)     # of one output: sheet_h x sheet_w, or the glyph's out_h x out_w
        self.t = 0            # AdamW step counter (model.py:310)
        # the tensors of an enqueued call, by slot, each until the next call that fills its slot: "in" (rows, x, font: until backward
        # has consumed them), "target", "eval", "sumsq", "minus"
        self._held = {}
        self._last_B = 0      # batch rows of the last forward / forward_rows (evaluate_last)
        self._tstats = {}     # tensor_stats: the record buffers, allocated once per kind of request
        if self.ema_decay is not None:
            self.set_ema(self.ema_decay, self.ema_every)
        if lr_mult is not None or wd_mult is not None:
            self.set_param_groups(lr_mult, wd_mult)

    def _call(self, fn, *args):
        """One libafr call that enqueues work: on THIS engine's device and on the caller's current stream of that device
        (the engine may live on cuda:k while the process's current device is another GPU)."""
        with torch.cuda.device(self.device):
            _lib.check(fn(*args, _stream(self.device)))

    def _views(self, flat):
        """The per-tensor views of a flat buffer in the parameter layout, by name."""
        return {nm: flat[o:o + k].view(shp) for nm, shp, o, k in self.layout}

    def _make_plan(self, max_batch):
        if self._plan:
            self.lib.afr_plan_destroy(self._plan)
        self.max_batch = int(max_batch)
        self._c = make_afr_config(self.cfg, self.dtype, self.max_batch, self.seed, self.rank, self.flags, self.loss)
        self._plan = C.c_void_p()
        _lib.check(self.lib.afr_plan_create(C.byref(self._c), C.byref(self._plan)))

    def _bind(self):
        with torch.cuda.device(self.device):
            self.ws_bytes = int(self.lib.afr_workspace_bytes(self._plan))
            self.workspace = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.afr_bind(self._plan, _ptr(self.flat_params), _ptr(self.flat_grads), _ptr(self.exp_avg),
                                     _ptr(self.exp_avg_sq), _ptr(self.workspace), self.ws_bytes))
        self._bind_ds()
        self._apply_clip()
        _lib.check(self.lib.afr_set_optimizer(self._plan, _lib.opt_kind(self.optimizer)))      # host-only; ensure_batch's new plan gets it again
        self._apply_ema()
        self._apply_groups()
        if self._ema_on:          # a re-plan inside ema_weights(): the new plan reads the EMA too
            self._call(self.lib.afr_use_ema, self._plan, 1)

    # ---------------------------------------------------------------- optimizer groups
    def _mult_array(self, mult):
        """dict name -> multiplier as the float array afr_set_param_groups takes, in layout order (missing names: 1.0); None stays None."""
        if mult is None:
            return None
        for nm in mult:
            if nm not in self.names:
                raise KeyError(f"{nm!r} is no parameter tensor of this model")
        return (C.c_float * len(self.names))(*[float(mult.get(nm, 1.0)) for nm in self.names])

    def _apply_groups(self):
        """Hand the plan its groups (host-only call; ensure_batch's new plan gets them again) and read the merged table back."""
        if self.layout is None:               # the constructor's first bind: the layout is not read yet, and there are no groups
            return
        lm, wm = self._mult_array(self.lr_mult), self._mult_array(self.wd_mult)
        _lib.check(self.lib.afr_set_param_groups(self._plan, lm, wm, len(self.layout)))
        n = int(self.lib.afr_param_group_ranges(self._plan, None, 0))
        self._ranges = (_lib.AfrOptRange * n)() if n else None
        if n:
            self.lib.afr_param_group_ranges(self._plan, self._ranges, n)

    def set_param_groups(self, lr_mult=None, wd_mult=None):
        """Optimizer groups from the next optimizer step on: tensor `name` is stepped with fl32(lr * lr_mult[name]) and
        fl32(weight_decay * wd_mult[name]) (include/afr.h afr_set_param_groups) through every path of a step -- fused or not, clipped or
        not, by rows, accumulated, and the slices of adamw_range.  Each argument is a dict of tensor name -> float; names that are
        missing take 1.0, an unknown name is a KeyError, a negative or non-finite value an AfrError.  Both None: groups off, the
        reference's single group.  state_dict() and the saved file know nothing of it."""
        self._not_in_ema("set_param_groups")
        old = self.lr_mult, self.wd_mult
        self.lr_mult = None if lr_mult is None else dict(lr_mult)
        self.wd_mult = None if wd_mult is None else dict(wd_mult)
        try:
            self._apply_groups()
        except Exception:
            self.lr_mult, self.wd_mult = old
            raise

    def param_group_ranges(self):
        """The plan's merged table: [(end offset, lr_mult, wd_mult)], [] when groups are off."""
        return [(int(r.end), float(r.lr_mult), float(r.wd_mult)) for r in (self._ranges or [])]

    # ---------------------------------------------------------------- weight EMA
    @staticmethod
    def _check_ema(decay, every):
        if decay is None:
            return None, 1
        decay = float(decay)
        if not (0.0 < decay < 1.0):
            raise ValueError(f"ema_decay must lie inside (0, 1) (None: off), got {decay!r}")
        if isinstance(every, bool) or int(every) != every or int(every) < 1:
            raise ValueError(f"ema_every must be an integer >= 1, got {every!r}")
        return decay, int(every)

    def _apply_ema(self):
        """Hand the plan its EMA setting (host-only call; ensure_batch's new plan gets it again, its count of steps starting anew)."""
        on = self.flat_ema is not None
        _lib.check(self.lib.afr_set_ema(self._plan, _ptr(self.flat_ema), float(self.ema_decay) if on else 0.0, int(self.ema_every) if on else 1))

    def _not_in_ema(self, what):
        """Inside ema_weights() nothing trains or steps (the library refuses with AFR_ESTATE; checked here before the step counter moves)."""
        if self._ema_on:
            raise _lib.AfrError(f"libafr error {_lib.AFR_ESTATE}: {what} while the engine reads its EMA weights (inside ema_weights())", _lib.AFR_ESTATE)

    def set_ema(self, decay, every=1):
        """Keep an exponential moving average of the weights from now on: after every `every`-th optimizer step of the engine
        (train_step*, adamw_step, the data-parallel schedules) e += (p - e) * (1 - decay), one pass over the flat buffer on the
        device (include/afr.h afr_set_ema).  flat_ema / ema_params / ema_state_dict() expose it, ema_weights() evaluates from it.
        The EMA starts as a copy of the parameters, and the count of steps at 0.  decay None switches it off."""
        self._not_in_ema("set_ema")
        self.ema_decay, self.ema_every = self._check_ema(decay, every)
        if self.ema_decay is None:
            self.flat_ema, self.ema_params = None, {}
            self._apply_ema()
            return
        if self.flat_ema is None:
            with torch.cuda.device(self.device):
                self.flat_ema = torch.zeros(self.n_flat, dtype=torch.float32, device=self.device)
            self.ema_params = self._views(self.flat_ema)
        self._apply_ema()
        self.reset_ema()

    def reset_ema(self):
        """EMA := the current parameters (load_params does it; reset_optimizer does not)."""
        self._not_in_ema("reset_ema")
        if self.flat_ema is None:
            raise _lib.AfrError("no EMA set (Engine(ema_decay=...) / set_ema)")
        self.flat_ema.copy_(self.flat_params)

    def ema_state_dict(self):
        if self.flat_ema is None:
            raise _lib.AfrError("no EMA set (Engine(ema_decay=...) / set_ema)")
        return {nm: self.ema_params[nm].detach().clone() for nm in self.names}

    def ema_update(self, sumsq=None):
        """Count one optimizer step that the engine did not perform itself (adamw_range on slices: parallel.py) and update the EMA
        when the interval says so.  sumsq: the 1-element device tensor the clipped slice update read; a non-finite value (a skipped
        step) leaves the EMA untouched."""
        self._not_in_ema("ema_update")
        self._call(self.lib.afr_ema_update, self._plan, _ptr(sumsq))
        self._held["sumsq"] = sumsq

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block forward / forward_rows (+ loss_grad*) and debug_read see the EMA weights (afr_use_ema: the bf16 shadow is
        re-derived on entry and on exit, one pass each); train_step*, forward_loss*, backward*, adamw_step and ema_update raise."""
        self._not_in_ema("ema_weights")
        self._call(self.lib.afr_use_ema, self._plan, 1)
        self._ema_on = True
        try:
            yield self
        finally:
            self._ema_on = False
            self._call(self.lib.afr_use_ema, self._plan, 0)

    @staticmethod
    def _check_clip(v):
        v = 0.0 if v is None else float(v)
        if not (np.isfinite(v) and v >= 0.0):
            raise ValueError(f"max_grad_norm must be a finite number >= 0 (0 or None: off), got {v!r}")
        return v or None

    def _apply_clip(self):
        """Hand the plan its clip setting (host-only call; ensure_batch's new plan gets it again)."""
        if self.max_grad_norm and self._clip_stats is None:
            with torch.cuda.device(self.device):
                self._clip_stats = torch.zeros(2, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.afr_set_grad_clip(self._plan, float(self.max_grad_norm or 0.0), _ptr(self._clip_stats if self.max_grad_norm else None)))

    def set_grad_clip(self, max_grad_norm):
        """Clip by global gradient norm from the next optimizer step on: g_eff = g * min(1, max_norm / (|grad_scale| * ||g|| + 1e-6)),
        the norm over every parameter tensor's elements (torch.nn.utils.clip_grad_norm_'s formula).  The coefficient lives inside
        the update: flat_grads is NOT rescaled (the one difference from torch).  A step whose gradients are not finite is skipped
        and sets bit 3 of error_flags().  None or 0 switches clipping off."""
        self.max_grad_norm = self._check_clip(max_grad_norm)
        self._apply_clip()

    def grad_sumsq(self, offset=0, n=None):
        """Sum of squares of the gradient buffer over the tensor elements (padding excluded) inside [offset, offset + n) of the flat
        layout, as a 1-element device tensor; works with clipping on or off.  offset and n are multiples of 4."""
        n = self.n_flat - int(offset) if n is None else int(n)
        with torch.cuda.device(self.device):
            out = torch.empty(1, dtype=torch.float32, device=self.device)
        self._call(self.lib.afr_grad_sumsq, self._plan, int(offset), n, _ptr(out))
        return out

    def tensor_stats(self, which="grads", minus=None):
        """Per-tensor statistics of a flat buffer, computed on the device in two launches (include/afr.h afr_tensor_stats): sum of
        squares, sum, minimum and maximum over the finite elements and the counts of NaN, infinite and zero elements of every
        parameter tensor, the padding between tensors never read.  which: "params" | "grads" | "exp_avg" | "exp_avg_sq" | "ema".
        minus: a float32 device tensor of n_flat elements in the flat layout; the statistics are then those of buffer - minus.  The
        update norm of a step: snap = eng.flat_params.clone(); the step; eng.tensor_stats("params", minus=snap).norm().
        Nothing is copied or synchronised until the result's cpu().  Which gradients the buffer holds after a fused optimizer step
        is described in the header."""
        if which not in _lib.STAT_KINDS:
            raise ValueError(f"which must be one of {sorted(_lib.STAT_KINDS)}, got {which!r}")
        if minus is not None and (not isinstance(minus, torch.Tensor) or minus.dtype != torch.float32 or minus.device != self.device or
                                  minus.numel() != self.n_flat or not minus.is_contiguous()):
            raise ValueError(f"minus must be a contiguous float32 tensor of {self.n_flat} elements on {self.device}")
        key = (which, minus is not None)
        if key not in self._tstats:
            with torch.cuda.device(self.device):
                self._tstats[key] = torch.empty((len(self.layout), 8), dtype=torch.int32, device=self.device)
        self._call(self.lib.afr_tensor_stats, self._plan, _lib.STAT_KINDS[which], _ptr(minus), _ptr(self._tstats[key]))
        self._held["minus"] = minus
        return TensorStats(self._tstats[key], self.names)

    def _read_clip_stats(self):
        if self._clip_stats is None or not self.max_grad_norm:
            raise _lib.AfrError("no clip statistics: clipping is off (Engine(max_grad_norm=...) / set_grad_clip)")
        return self._clip_stats.cpu()        # one synchronising copy

    def grad_norm(self):
        """|grad_scale| * global L2 norm of the gradients the last clipped optimizer step saw (before clipping)."""
        return float(self._read_clip_stats()[0])

    def clip_coef(self):
        """The coefficient min(1, max_norm / (norm + 1e-6)) the last clipped optimizer step applied."""
        return float(self._read_clip_stats()[1])

    def _bind_ds(self):
        if self._ds is not None:
            x, font, t, td, n, L = self._ds
            _lib.check(self.lib.afr_bind_dataset(self._plan, _ptr(x), _ptr(font), _ptr(t), td, n, L))

    def bind_dataset(self, x, target, font=None):
        """Make a data set resident and bind it: codes int64 [N, L] (sheet) or [N] (glyph / pixel, with font ids [N] when the
        model has fonts), targets uint8 or float32 [N, pixels] / [N, H, W].  forward_rows / loss_grad_rows / forward_loss_rows /
        train_step_rows then take a vector of row indices; the kernels read the targets where they lie.  The engine holds
        references to the tensors, and binds them again when ensure_batch re-creates the plan."""
        (_, x, font), (_, t), td, n, L, _ = self._batch(x, font, target)
        t = t.view(t.shape[0], -1)
        if t.shape != (n, self.pixels) or (font is not None and font.reshape(-1).shape[0] != n):
            raise ValueError(f"data set of {n} rows: targets {tuple(t.shape)} (expected {(n, self.pixels)}) / font ids do not match")
        self._ds = (x, None if font is None else font.reshape(-1), t, td, n, L)
        self._bind_ds()

    def ensure_batch(self, B):
        """Grow the plan's workspace for a larger batch; parameters, gradients and moments stay where they are."""
        if B > self.max_batch:
            torch.cuda.synchronize(self.device)
            self._make_plan(B)
            self._bind()
            self.sync_params()

    def __del__(self):
        try:
            if getattr(self, "_plan", None):
                self.lib.afr_plan_destroy(self._plan)
                self._plan = None
        except Exception:
            pass

    # ---------------------------------------------------------------- parameters
    def load_params(self, tensors):
        """tensors: dict name -> numpy array / torch tensor (any device), state_dict keys.  An EMA restarts from them."""
        self._not_in_ema("load_params")
        for nm, shp, _, _ in self.layout:
            src = tensors[nm]
            src = torch.from_numpy(np.ascontiguousarray(src)) if isinstance(src, np.ndarray) else src.detach()
            if tuple(src.shape) != tuple(shp):
                raise ValueError(f"{nm}: shape {tuple(src.shape)} != {tuple(shp)}")
            self.params[nm].copy_(src.to(torch.float32))
        self.sync_params()
        if self.flat_ema is not None:
            self.reset_ema()

    def sync_params(self):
        self._call(self.lib.afr_sync_params, self._plan)

    def state_dict(self):
        return {nm: self.params[nm].detach().clone() for nm in self.names}

    def reset_optimizer(self):
        for moment in (self.exp_avg, self.exp_avg_sq):
            if moment is not None:
                moment.zero_()
        self.t = 0

    # ---------------------------------------------------------------- the batch a call runs on
    def _batch(self, x=None, font=None, target=None, rows=None, mean_elems=None):
        """What every call below runs on: dense tensors (codes x, font ids, a target; each may be missing) or a vector of rows of the
        bound data set.  Returns ((rows, x, font), (rows, t), td, B, L, me): the tensors on the engine's device in the types the
        library reads (rows, x, font int64; t uint8 or float32, td its code), None where there is none; the sample count B; the codes
        per sample L (sheet model: x is [B, L]; glyph and pixel models: x is flattened, L = 1); and me, the element count the loss is
        the mean over, B * pixels unless mean_elems says otherwise.  With no tensor at all, B is that of the last forward
        (evaluate_last).  The first two members are what an enqueued call keeps alive (self._held) when it reads the inputs and when
        it reads the targets."""
        dev, t, td, L = self.device, None, 0, 1
        if rows is not None:
            if self._ds is None:
                raise _lib.AfrError("no data set bound: call bind_dataset before stepping by rows")
            rows = rows.to(dev, dtype=torch.int64, non_blocking=True).contiguous().reshape(-1)
            x, font, B = None, None, rows.shape[0]
        else:
            if x is not None:
                x = x.to(dev, dtype=torch.int64, non_blocking=True).contiguous()
                if font is not None:
                    font = font.to(dev, dtype=torch.int64, non_blocking=True).contiguous()
                if isinstance(self.cfg, SheetConfig):
                    if x.dim() != 2:
                        raise ValueError("sheet model takes int64 [B, L] codes")
                    L = x.shape[1]
                else:
                    x = x.reshape(-1)
            if target is not None and target.dtype == torch.uint8:
                t, td = target.to(dev, non_blocking=True).contiguous(), _lib.AFR_TARGET_U8
            elif target is not None:
                t, td = target.to(dev, dtype=torch.float32, non_blocking=True).contiguous(), _lib.AFR_TARGET_F32
            B = x.shape[0] if x is not None else t.shape[0] if t is not None else self._last_B
        return (rows, x, font), (rows, t), td, B, L, (B * self.pixels if mean_elems is None else int(mean_elems))

    def _prep_x(self, x, font):
        """The codes and font ids as the library reads them (the batch's; a glyph or pixel model's codes come back flattened)."""
        return self._batch(x, font)[0][1:]

    def _target(self, target):
        """The target as the library reads it, and its type code."""
        b = self._batch(target=target)
        return b[1][1], b[2]

    def _split(self, b):
        """The micro-batches of a batch in order: samples [lo, hi) of every tensor, at most micro_batch of them; me stays the whole
        batch's, so that the micro-steps' losses and gradients add up to the batch's."""
        (rows, x, font), (_, t), td, B, L, me = b
        for lo in range(0, B, self.micro_batch):
            hi = min(B, lo + self.micro_batch)
            rows_, x_, font_, t_ = (None if v is None else v[lo:hi] for v in (rows, x, font, t))
            yield (rows_, x_, font_), (rows_, t_), td, hi - lo, L, me

    # ---------------------------------------------------------------- the hot path: one body per operation, on a batch
    def _forward(self, b, training, step, want_output):
        (rows, x, font), _, _, B, L, _ = b
        if self.micro_batch and B > self.micro_batch:        # an inference forward of a large batch, micro_batch rows at a time
            outs = [self._forward(m, training, step, want_output) for m in self._split(b)]
            return torch.cat(outs) if want_output else None
        if B > self.max_batch:
            self.ensure_batch(B)
        y = torch.empty(B, self.pixels, dtype=torch.float32, device=self.device) if want_output else None
        if rows is not None:
            self._call(self.lib.afr_forward_rows, self._plan, _ptr(rows), B, _ptr(y), int(bool(training)), int(step))
        else:
            self._call(self.lib.afr_forward, self._plan, _ptr(x), _ptr(font), B, L, _ptr(y), int(bool(training)), int(step))
        self._held["in"] = b[0]
        self._last_B = B
        return None if y is None else y.view(B, *self._hw)

    def _loss_grad(self, b):
        _, (rows, t), td, B, _, me = b
        if rows is not None:
            self._call(self.lib.afr_loss_grad_rows, self._plan, _ptr(rows), B, me, _ptr(self.loss_accum))
        else:
            self._call(self.lib.afr_loss_grad, self._plan, _ptr(t), td, B, me, _ptr(self.loss_accum))
        self._held["target"] = b[1]

    def _forward_loss(self, b, step):
        (rows, x, font), (_, t), td, B, L, me = b
        if self.micro_batch and B > self.micro_batch:
            raise ValueError(f"forward_loss / backward work on one micro-batch (<= {self.micro_batch} samples); a batch of {B} "
                             f"accumulates through train_step{'' if rows is None else '_rows'}")
        if B > self.max_batch:
            self.ensure_batch(B)
        st = int(step if step is not None else self.t + 1)
        if rows is not None:
            self._call(self.lib.afr_forward_loss_rows, self._plan, _ptr(rows), B, me, _ptr(self.loss_accum), st)
        else:
            self._call(self.lib.afr_forward_loss, self._plan, _ptr(x), _ptr(font), _ptr(t), td, B, L, me, _ptr(self.loss_accum), st)
        self._held["in"], self._held["target"] = b[0], b[1]

    def _train_step(self, b, step=None, lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=5e-4, do_step=True):
        (rows, x, font), (_, t), td, B, L, me = b
        if self.micro_batch and B > self.micro_batch:
            return self._train_step_accumulated(b, step, lr, betas, eps, weight_decay, do_step)
        if B > self.max_batch:
            self.ensure_batch(B)
        if do_step:
            self.t += 1
        st = int(step if step is not None else self.t)
        if rows is not None:
            self._call(self.lib.afr_train_step_rows, self._plan, _ptr(rows), B, me, _ptr(self.loss_accum), st,
                       int(bool(do_step)), lr, betas[0], betas[1], eps, weight_decay, max(self.t, 1))
        else:
            self._call(self.lib.afr_train_step, self._plan, _ptr(x), _ptr(font), _ptr(t), td, B, L, me, _ptr(self.loss_accum), st,
                       int(bool(do_step)), lr, betas[0], betas[1], eps, weight_decay, max(self.t, 1))
        self._held["in"], self._held["target"] = b[0], b[1]

    def _train_step_accumulated(self, b, step, lr, betas, eps, weight_decay, do_step):
        """Gradient accumulation: the batch in micro-steps of self.micro_batch samples (forward + loss + backward each, the loss
        and its gradient scaled for the WHOLE batch through the batch's me), gradients summed in micro-step order, one AdamW step."""
        if self._grad_acc is None:
            self._grad_acc = torch.empty_like(self.flat_grads)
        st = int(step if step is not None else self.t + (1 if do_step else 0))
        for i, m in enumerate(self._split(b)):
            # (models with dropout: micro-step i draws its masks from stream st * 65536 + i.  A micro-step does not step: its
            # hyper-parameters are not read and stay the defaults)
            self._train_step(m, step=st * 65536 + i if step is None else st, do_step=False)
            # acc (+)= this micro-step's gradient, by the library's own slab-sum kernel (fixed order: micro-step by micro-step)
            self._call(self.lib.afr_op_reduce, _ptr(self._grad_acc), _ptr(self.flat_grads), 1, self.n_flat, self.n_flat, 1.0, int(i > 0))
        self._call(self.lib.afr_op_reduce, _ptr(self.flat_grads), _ptr(self._grad_acc), 1, self.n_flat, self.n_flat, 1.0, 0)
        if do_step:
            self.adamw_step(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)

    def _evaluate_last(self, b, want_u8):
        _, (rows, t), td, B, _, _ = b
        need_t = rows is not None or t is not None
        with torch.cuda.device(self.device):
            loss_rows = torch.empty(B, dtype=torch.float32, device=self.device) if need_t else None
            stats = torch.empty(B, 4, dtype=torch.int32, device=self.device) if need_t else None      # the library's uint32 words (<= pixels)
            q = torch.empty(B, self.pixels, dtype=torch.uint8, device=self.device) if want_u8 or not need_t else None
        if rows is not None:
            self._call(self.lib.afr_eval_rows, self._plan, _ptr(rows), B, _ptr(loss_rows), _ptr(stats), _ptr(q))
        else:
            self._call(self.lib.afr_eval, self._plan, _ptr(t), td, B, _ptr(loss_rows), _ptr(stats), _ptr(q))
        self._held["eval"] = b[1]
        return EvalResult(loss_rows, None if stats is None else stats.to(torch.int64), None if q is None else q.view(B, *self._hw))

    def _evaluate(self, b, want_u8):
        t, B = b[1][1], b[3]
        if t is not None and t.shape[0] != B:
            raise ValueError(f"{t.shape[0]} targets for a batch of {B}")
        if self.micro_batch and B > self.micro_batch:
            return EvalResult.cat([self._evaluate(m, want_u8) for m in self._split(b)])
        self._forward(b, False, 0, False)
        return self._evaluate_last(b, want_u8)

    # ---------------------------------------------------------------- the hot path: the public calls, dense and by rows
    def forward(self, x, font=None, training=False, step=0, want_output=True):
        return self._forward(self._batch(x, font), training, step, want_output)

    def forward_rows(self, rows, training=False, step=0, want_output=True):
        """forward() on the rows `rows` (int64 indices, duplicates allowed) of the bound data set."""
        return self._forward(self._batch(rows=rows), training, step, want_output)

    def evaluate_last(self, target=None, rows=None, want_u8=False):
        """The evaluation kernel alone (afr_eval / afr_eval_rows: one launch, nothing allocated by the library) on the pre-activation
        the last forward / forward_rows left in the workspace; the buffer is only read, so loss_grad* / set_output_grad / backward may
        follow as if nothing had happened.  target: uint8 or float32 [B, pixels] / [B, H, W]; or rows: the data-set rows of the
        forward_rows before it; neither: the bitmaps alone (want_u8 is then implied).  Returns an EvalResult."""
        if target is not None and rows is not None:
            raise ValueError("evaluate_last takes a target or rows, not both")
        return self._evaluate_last(self._batch(target=target, rows=rows), want_u8)

    def evaluate(self, x, target=None, font=None, want_u8=False):
        """An eval forward (no float32 output is materialised) followed by the evaluation kernel: per-sample loss and the 8-bit error
        counts against `target`, and with want_u8 (or without a target) the uint8 bitmaps.  A batch larger than micro_batch is split
        as forward() splits it."""
        return self._evaluate(self._batch(x, font, target), want_u8)

    def evaluate_rows(self, rows, want_u8=False):
        """evaluate() on rows of the bound data set (duplicates allowed), against their targets where they lie."""
        return self._evaluate(self._batch(rows=rows), want_u8)

    def render_u8(self, x, font=None):
        """uint8 [B, H, W]: the levels binary_array_to_image would write for forward(x), quantised on the device."""
        return self.evaluate(x, font=font, want_u8=True).u8

    def loss_grad(self, target, mean_elems=None):
        self._loss_grad(self._batch(target=target, mean_elems=mean_elems))

    def loss_grad_rows(self, rows, mean_elems=None):
        """loss_grad() against the targets of data-set rows `rows` (the rows of the forward before it)."""
        self._loss_grad(self._batch(rows=rows, mean_elems=mean_elems))

    def forward_loss(self, x, target, font=None, step=None, mean_elems=None):
        """Training forward with the loss/grad fused into the last layer's epilogue (no optimizer step)."""
        self._forward_loss(self._batch(x, font, target, mean_elems=mean_elems), step)

    def forward_loss_rows(self, rows, step=None, mean_elems=None):
        """forward_loss() on rows of the bound data set."""
        self._forward_loss(self._batch(rows=rows, mean_elems=mean_elems), step)

    def train_step(self, x, target, font=None, step=None, lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=5e-4,
                   mean_elems=None, do_step=True):
        """zero_grad -> forward -> loss -> backward -> AdamW, one C call (model.py:292-310)."""
        self._not_in_ema("train_step")
        self._train_step(self._batch(x, font, target, mean_elems=mean_elems), step, lr, betas, eps, weight_decay, do_step)

    def train_step_rows(self, rows, step=None, lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=5e-4, mean_elems=None, do_step=True):
        """train_step() on rows of the bound data set: one C call, no gather in front of it."""
        self._not_in_ema("train_step_rows")
        self._train_step(self._batch(rows=rows, mean_elems=mean_elems), step, lr, betas, eps, weight_decay, do_step)

    def set_output_grad(self, dy):
        """dy = d(loss)/d(output) from a caller-side loss (autograd); float32 [B, pixels].  The output is the clamped one, or the
        sigmoid of a loss="bce" engine."""
        dy = dy.to(self.device, dtype=torch.float32).contiguous()
        self._call(self.lib.afr_set_output_grad, self._plan, _ptr(dy), dy.shape[0])
        self._held["target"] = dy

    def backward(self):
        self._call(self.lib.afr_backward, self._plan)

    @property
    def backward_stages(self):
        return int(self.lib.afr_backward_stages(self._plan))

    def backward_stage(self, stage):
        """Run one backward stage; returns the view of flat_grads that is final after it."""
        off, n = C.c_int64(), C.c_int64()
        self._call(self.lib.afr_backward_stage, self._plan, int(stage), C.byref(off), C.byref(n))
        return self.flat_grads[off.value:off.value + n.value]

    def adamw_step(self, lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=5e-4, grad_scale=1.0):
        """One optimizer step of the engine's kind (the name is the AdamW engine's; a Lion engine ignores eps)."""
        self._not_in_ema("adamw_step")
        self.t += 1
        self._call(self.lib.afr_adamw_step, self._plan, lr, betas[0], betas[1], eps, weight_decay, self.t, grad_scale)

    def adamw_range(self, offset, n, lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=5e-4, grad_scale=1.0, sumsq=None):
        """One optimizer step (AdamW, or Lion on a Lion engine) on the flat-buffer slice [offset, offset + n) only (sharded optimizer under data parallelism:
        parallel.py).  Advances the step counter; the bf16 shadow is NOT refreshed (the caller syncs after its all-gather).
        sumsq: a 1-element device tensor holding the GLOBAL sum of squared gradients (grad_sumsq of every rank's range,
        all-reduced): the slice is then updated with the clip coefficient of self.max_grad_norm, as adamw_step would.
        The EMA is not touched: the caller counts the step with ema_update once every slice is in place."""
        self._not_in_ema("adamw_range")
        self.t += 1
        o, n, lion, null = int(offset), int(n), self.optimizer == "lion", C.c_void_p(0)
        p, g, m = (_ptr(flat[o:o + n]) for flat in (self.flat_params, self.flat_grads, self.exp_avg))
        v = null if lion else _ptr(self.exp_avg_sq[o:o + n])
        clip = (_ptr(sumsq), float(self.max_grad_norm or 0.0))
        if self._ranges is not None:      # optimizer groups: the slice in one launch of the range-aware kernel, with the plan's table
            fn, args = self.lib.afr_op_opt_groups, (_lib.opt_kind(self.optimizer), p, g, m, v, null, n, o, self._ranges, len(self._ranges),
                                                    lr, betas[0], betas[1], eps, weight_decay, self.t, grad_scale, *clip)
        elif lion:                        # the same slice step by afr_op_lion, clipped when sumsq is given
            fn, args = self.lib.afr_op_lion, (p, g, m, null, n, lr, betas[0], betas[1], weight_decay, grad_scale, *clip)
        else:
            fn, args = self.lib.afr_op_adamw, (p, g, m, v, null, n, lr, betas[0], betas[1], eps, weight_decay, self.t, grad_scale)
            if sumsq is not None:
                fn, args = self.lib.afr_op_adamw_clip, args + clip
        self._call(fn, *args)
        self._held["sumsq"] = sumsq

    def read_loss(self, reset=True):
        v = float(self.loss_accum.item())
        if reset:
            self.loss_accum.zero_()
        return v

    def error_flags(self):
        out = C.c_uint32(0)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.afr_error_flags(self._plan, _stream(self.device), C.byref(out)))
        return out.value

    def debug_read(self, which, index=0):
        """Copy an internal activation buffer of the last call (u/du, z, dz, glyph activation i, pixel block i's ReLU output)
        as float32."""
        code = {"u": _lib.BUF_U, "z": _lib.BUF_Z, "dz": _lib.BUF_DZ, "act": _lib.BUF_ACT + int(index), "w1t": _lib.BUF_W1T, "w2t": _lib.BUF_W2T}[which]
        dt = torch.bfloat16 if (self.dtype in ("bf16", "bfloat16") or which in ("w1t", "w2t")) else torch.float32
        es = 2 if dt == torch.bfloat16 else 4
        widest = max(self.pixels, getattr(self.cfg, "flat_dim", 0), *(getattr(self.cfg, "hidden", (0,))), getattr(self.cfg, "embed_dim", 0),
                     getattr(self.cfg, "tokens", 0) * getattr(self.cfg, "ff_dim", 0))     # (pixel model: a block's ReLU output)
        cap = max(self.max_batch * widest * es, 1 << 20)
        buf = torch.empty(cap, dtype=torch.uint8, device=self.device)
        n = C.c_size_t()
        self._call(self.lib.afr_debug_copy, self._plan, code, _ptr(buf), cap, C.byref(n))
        torch.cuda.synchronize(self.device)
        return buf[:n.value].view(dt).float()

    def debug_sheet_gather(self, x):
        """The rows the sheet front end's in-kernel embedding gather fetched for x [B, L]: float32 [B, min(L, max_length), E]."""
        x, _ = self._prep_x(x, None)
        self.ensure_batch(x.shape[0])
        B, L = x.shape
        e0 = torch.full((B, min(L, self.cfg.max_length), self.cfg.embed_dim), float("nan"), dtype=torch.float32, device=self.device)
        self._call(self.lib.afr_debug_sheet_gather, self._plan, _ptr(x), B, L, _ptr(e0))
        torch.cuda.synchronize(self.device)
        return e0

    # ---------------------------------------------------------------- measurement
    def profile(self, mode=1):
        """0 off, 1 time every launch, 2 time only the kernel that dominated the mode-1 recording."""
        _lib.check(self.lib.afr_profile_dominant(self._plan, int(mode)))

    def profile_table(self):
        buf = C.create_string_buffer(8192)
        _lib.check(self.lib.afr_profile_dump(self._plan, buf, 8192))
        rows = []
        for line in buf.value.decode().strip().split("\n"):
            if line:
                k, n, tot, avg, fl, by = line.split("\t")
                rows.append(dict(kernel=k, launches=int(n), total_ms=float(tot), avg_ms=float(avg), algo_flops=float(fl), algo_bytes=float(by)))
        return sorted(rows, key=lambda r: -r["total_ms"])

    def profile_read(self):
        name = C.create_string_buffer(128)
        ms, fl, by = C.c_double(), C.c_double(), C.c_double()
        n = C.c_int64()
        _lib.check(self.lib.afr_profile_read(self._plan, name, 128, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)))
        return dict(kernel=name.value.decode(), avg_ms=ms.value, launches=n.value, algo_flops=fl.value, algo_bytes=by.value)
