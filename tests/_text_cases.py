"""Inputs, references and bounds of the text-encoder tests (test_text_encoder_host.py / _gpu.py).

The core under test is the causal attention of the CLIP towers,
    out[b,i] = merge_heads( softmax_{j<=i}(scale q_i k_j^T) v ),        q, k, v [B,N,H*d]
Inputs come from `_attn_cases.make_case` (N = Nk, Bk = B) for its families, and from two families of this file that are built
with the same orthogonal-offset construction (logit[i][j] = scale q_perp[i].k_perp[j] + offset_j):
    diag_ramp    key j carries 3*j: every masked future key would outweigh all visible ones, each row is dominated by its diagonal
    first_only   key 0 carries +100: every row puts all its weight on the one key that is visible to all rows
The references materialise the masked softmax in fp64 and fp32; the metric is `_attn_cases.assert_attn_close`:
    err <= M * err_fp32ref + 1e-7   against the fp64 reference.

Two pairings are exact in every precision, so their err_fp32ref is 0 and their bound is the absolute 1e-7 alone (tighter than
any multiple of an fp32 error; both stay, they are the cases they are for):
    N = 1          a row with a single key has the weight 1 exactly and out = v: the row that must not divide by zero;
    first_only     exp(-100) is below half an ulp of 1 in fp64 too: out = v[0] to the last bit in the fp32 and the fp64 reference.
Every other (family, shape) has a finite, non-zero err_fp32ref (test_text_encoder_host.py checks all of them).
"""
from __future__ import annotations

import functools
import math

import torch

import _attn_cases as A

FAMILIES = ("randn", "spike_first", "spike_last", "all_high", "all_low", "odd_scale", "tiny_scale", "diag_ramp", "first_only")
SIZES = (1, 2, 15, 16, 17, 31, 32, 33, 64, 77, 128)          # every 32-key tile edge, the wave edges, 77, the limit
HEAD_DIMS = (32, 64)
BATCH_HEADS = ((1, 1), (2, 3))
DIAG_STEP = 3.0
FIRST = 100.0

# err_kernel <= M * err_fp32ref + 1e-7: twice the largest ratio measured on the MI355X over all cases (792, then 1 188 with the padded layout), rounded up, never above 8
# (profiles/text_encoder.md: largest ratio 2.84, `all_high` at N = 2, d = 32 -> 6).
M = 6
# the same kind of bound for a whole tower on the GPU against the fp64 CPU run of the same tree: M_TREE x the fp32 CPU tree's error
# (largest of the six measured ratios 1.25 -> 3)
M_TREE = 3


def make_text_case(family, B, H, N, d, seed=7):
    """-> q, k, v [B,N,H*d] (fp32), scale (a float fp32 holds exactly)."""
    if family in A.FAMILIES:
        q, k, v, _, scale = A.make_case(family, B, B, H, N, N, d, seed)
        return q, k, v, scale
    assert family in ("diag_ramp", "first_only")
    q, k, v, _, scale = A.make_case("randn", B, B, H, N, N, d, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    u = torch.randn(H, d, generator=g, dtype=torch.float64)
    u = u / u.norm(dim=-1, keepdim=True)
    off = DIAG_STEP * torch.arange(N, dtype=torch.float64) if family == "diag_ramp" else torch.zeros(N, dtype=torch.float64)
    if family == "first_only":
        off[0] = FIRST
    top = off.abs().max().item()
    C = H * d
    if top > 0:                                       # (diag_ramp over one key is flat: nothing to add)
        a = math.sqrt(top / scale)                    # the offset split evenly between q and k, as in _attn_cases.make_case
        c = off / (a * scale)
        q = (A._heads(A._along(q.double(), u, H), H) + a * u).reshape(B, N, C).float()
        k = (A._heads(A._along(k.double(), u, H), H) + c[None, :, None, None] * u).reshape(B, N, C).float()
    return q, k, v, scale


def causal_reference(q, k, v, scale, H, dtype):
    """Materialised masked softmax attention in `dtype` -> {"out": [B,N,C]}."""
    qh, kh, vh = (A._split(t, H, dtype) for t in (q, k, v))
    S = (qh @ kh.transpose(-1, -2)) * scale
    n = S.shape[-1]
    S = S.masked_fill(torch.ones(n, n, dtype=torch.bool).triu(1), float("-inf"))
    lse = torch.logsumexp(S, dim=-1)
    return {"out": A._merge(torch.exp(S - lse[..., None]) @ vh)}


def causal_logits(q, k, scale, H):
    """fp64 logits [B,H,N,N], future keys NOT masked (what a missing mask would see)."""
    return A.logits(q, k, scale, H)


class TextCase:
    """Inputs of one family at one shape with the fp64 and the fp32 causal reference (computed once, never modified); carries what
    `_attn_cases.assert_attn_close` reads."""

    def __init__(self, family, B, H, N, d, seed=7):
        self.family, self.shape, self.H, self.shared = family, (B, B, H, N, N, d), H, False
        self.q, self.k, self.v, self.scale = make_text_case(family, B, H, N, d, seed)
        self.ref64 = causal_reference(self.q, self.k, self.v, self.scale, H, torch.float64)
        self.ref32 = causal_reference(self.q, self.k, self.v, self.scale, H, torch.float32)
        self.err32 = A.errors(self.ref32, self.ref64, False)


@functools.lru_cache(maxsize=None)
def case(family, B, H, N, d, seed=7) -> TextCase:
    return TextCase(family, B, H, N, d, seed)


# ---------------------------------------------------------------------------------------------------------------------
# towers
# ---------------------------------------------------------------------------------------------------------------------
def tower(width, heads, act="quick_gelu", projection_dim=None, seed=11, vocab=514):
    """A seeded 2-layer CLIPTextModel (frozen, eval) on the CPU."""
    from stablekeypoints_amd.ldm.clip import CLIPTextModel
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)                           # (the global generator is left where it was)
    try:
        m = CLIPTextModel(vocab_size=vocab, hidden_size=width, num_hidden_layers=2, num_attention_heads=heads,
                          intermediate_size=4 * width, hidden_act=act, projection_dim=projection_dim, eos_token_id=vocab - 1)
    finally:
        torch.random.set_rng_state(state)
    return m.eval().requires_grad_(False)


def prompt_ids(n=3, L=77, vocab=514, seed=5):
    """n rows of L ids: BOS, random symbols, EOS at a different place per row, EOS padding behind it."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, vocab - 2, (n, L), generator=g)
    ids[:, 0] = vocab - 2
    for r in range(n):
        ids[r, min(L - 1, 5 + 9 * r):] = vocab - 1
    return ids
