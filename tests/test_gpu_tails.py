"""GPU: the tails of the C3 step's launches.

* The deferred loss sum.  A monolithic fused training step (forward, whole backward and optimizer in one afr_train_step, fused
  first-layer backward) lets the forward's last GEMM store its per-workgroup loss partials without the arrival ticket; one
  workgroup appended to the first-layer backward's grid adds them.  The loss must equal the ticket form's bit for bit.
* The cooperative split-K tail keeps the strip a slice reduces itself in registers.  afr_op_gemm_pair must give the bytes the
  parent commit gave (tests/golden/tails_gemm_pair_sha256.json: digests of the parent build's outputs on one MI355X).
"""
import hashlib
import json
import os

import pytest
import torch

from .util import GlyphConfig, glyph_inputs, synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tails_gemm_pair_sha256.json")


def _engine(cfg, max_batch, flags=0):
    from ai_font_renderer_amd.engine import Engine
    eng = Engine(cfg, dtype="bf16", max_batch=max_batch, flags=flags)
    eng.load_params(synth.make_params(cfg))
    return eng


def _bits(v):
    return torch.tensor([v], dtype=torch.float32).view(torch.int32).item()


def _c3():
    from ai_font_renderer_amd.config import WORKLOADS
    return WORKLOADS["c3"]["cfg"]


# The forward's last GEMM runs 128x128 tiles of 256 threads below the chip-filling grids (6 loss workgroups for 300 glyphs of 16x16)
# and 256x128 tiles of 512 threads from there on (C3: 256 loss workgroups): both block sizes the deferred sum reproduces.
@pytest.mark.parametrize("name,B", [("h256x256_16x16", 300), ("c3", 8192)])
def test_deferred_loss_equals_ticket_loss_bitwise(name, B):
    """train_step x3, forward_loss, train_step on ONE engine, from a non-zero loss_accum and without resetting it: every loss
    read equals, bit for bit, that of an engine with AFR_CFG_UNFUSED_OPTIMIZER (config.reserved bit 0), whose steps run the
    unfused path and so take the ticket on the same partials.  lr = 0 keeps the parameters of both engines equal.  The
    forward_loss in between is a ticket-form call on the plan whose counter the deferred steps never touched."""
    cfg = _c3() if name == "c3" else GlyphConfig(hidden=(256, 256), out_h=16, out_w=16)
    x, font, tu8 = glyph_inputs(cfg, B)
    xt, tt = torch.from_numpy(x), torch.from_numpy(tu8)
    ft = torch.from_numpy(font) if cfg.n_fonts else None
    got = {}
    for flags in (0, 1):
        e = _engine(cfg, B, flags)
        p0 = e.flat_params.clone()
        e.loss_accum.fill_(0.37109375)
        reads = []
        for call in ("train", "train", "train", "fwd", "train"):
            if call == "train":
                e.train_step(xt, tt, font=ft, lr=0.0)
            else:
                e.forward_loss(xt, tt, font=ft)
            reads.append(e.read_loss(reset=False))
        assert e.error_flags() == 0
        assert torch.equal(e.flat_params, p0)           # lr = 0: both engines computed every loss from the same parameters
        got[flags] = reads
        del e
    print(name, "losses (deferred):", got[0])
    assert [_bits(v) for v in got[0]] == [_bits(v) for v in got[1]], (got[0], got[1])
    # the accumulator moved with every call (the sum really ran) and by the same loss each time: a read is a rounded sum (error
    # <= 2^-24 |accumulator|), a step is the difference of two reads, two steps differ by at most four such errors
    d = [b - a for a, b in zip([0.37109375] + got[0][:-1], got[0])]
    assert all(v > 0 for v in d) and max(d) - min(d) <= 4 * 2.0 ** -24 * got[0][-1], d


def _sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def pair_case(B, N, K):
    """One afr_op_gemm_pair launch (twice on one workspace) on hashed bf16 operands -> digests of dW, db and dX."""
    from .gpu_util import gemm_pair

    def rnd(tid, shape, bound):
        return torch.from_numpy(synth.hash_uniform(tid, shape, bound)).to(torch.bfloat16).to(torch.float32)
    dy, x = rnd(771, (B, N), 0.05), rnd(772, (B, K), 1.0)
    W, aux = rnd(773, (N, K), 0.2), rnd(774, (B, K), 1.0)
    outs, sk = gemm_pair(dy, x, W, aux, repeats=2)
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    dW, db, dX = outs[0]
    return {"splitk": sk, "dW": _sha(dW), "db": _sha(db), "dX": _sha(dX.to(torch.bfloat16))}


# The smallest products afr_op_gemm_pair_plan accepts at each split it knows: 8 slices own one 16-row strip of every wave's
# accumulators (C3's case), 4 slices two, 2 slices four.  (120 input-gradient tiles + 120 weight-gradient slices each.)
PAIR_CASES = [(2048, 256, 3712, 8), (2048, 512, 3712, 4), (2048, 1024, 3712, 2)]


@pytest.mark.parametrize("B,N,K,sk", PAIR_CASES)
def test_cooperative_pair_equals_parent_bitwise(B, N, K, sk):
    """The slice-order sum takes its own term from registers instead of the workspace: same terms, same order, same bytes as
    the parent commit's launch, whose digests are the fixture."""
    want = json.load(open(GOLDEN))["%dx%dx%d" % (B, N, K)]
    got = pair_case(B, N, K)
    assert got["splitk"] == sk == want["splitk"]
    assert got == want
