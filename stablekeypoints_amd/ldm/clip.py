"""CLIP text towers of Stable Diffusion: the `model.text_encoder` of the reference's sampling entry (ptp_utils.py:436-439).

`CLIPTextModel` carries the transformers parameter names, so the `text_encoder/` of a diffusers checkpoint loads key for key:

    text_model.embeddings.{token_embedding,position_embedding}.weight
    text_model.encoder.layers.N.{layer_norm1, self_attn.{q,k,v,out}_proj, layer_norm2, mlp.{fc1,fc2}}
    text_model.final_layer_norm
    text_projection.weight                      (towers with a projection: SDXL's second one)

Pre-LN blocks, `quick_gelu` (x sigmoid(1.702 x)) or erf `gelu`, a causal mask and NO padding mask (how the Stable Diffusion
pipelines call the towers).  The towers are frozen: the forward runs without gradients.

    out = model(input_ids)                      # tuple; out[0] = final_layer_norm(last layer)  [n, L, width]  (the reference's call)
    out = model(input_ids, penultimate=True)    # out[0] = input of the last layer, WITHOUT the final norm (what SDXL conditions on)
    out[1]                                      # pooled: final_layer_norm(last)[first EOS position], through text_projection if any

On the GPU a block is one stacked q | k | v GEMM, `ops.text_attention` on its three column bands (csrc/skp_text_attn.hip),
`out_proj`, and `ops.add_layer_norm` for the two residual-plus-norm joints; host tensors run plain torch (route `host`).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import routes

# published towers (parameter counts: profiles/text_encoder.md, tests/test_text_encoder_host.py)
CONFIGS = {
    "sd15": dict(vocab_size=49408, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                 hidden_act="quick_gelu"),
    "sd21": dict(vocab_size=49408, hidden_size=1024, num_hidden_layers=23, num_attention_heads=16, intermediate_size=4096,
                 hidden_act="gelu"),
    # SDXL's second tower (OpenCLIP bigG); its first is the sd15 tree
    "sdxl_2": dict(vocab_size=49408, hidden_size=1280, num_hidden_layers=32, num_attention_heads=20, intermediate_size=5120,
                   hidden_act="gelu", projection_dim=1280),
}
_KEYS = ("vocab_size", "hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "hidden_act",
         "max_position_embeddings", "layer_norm_eps", "projection_dim", "eos_token_id")


def kwargs_from_config(c: dict, with_projection: bool) -> dict:
    """transformers `text_encoder/config.json` -> CLIPTextModel kwargs (only the keys this tree understands); `projection_dim` counts
    only for a tower that has the projection (`CLIPTextModelWithProjection`)."""
    kw = {k: c[k] for k in _KEYS if c.get(k) is not None}
    if not with_projection:
        kw.pop("projection_dim", None)
    return kw


def canonical_keys(state: dict) -> dict:
    """State dict with the checkpoint key names above.  Newer transformers versions keep the same tensors without the
    `text_model.` prefix in memory (`embeddings.*`, `encoder.*`, `final_layer_norm.*`); such keys get it back, nothing else moves."""
    bare = ("embeddings.", "encoder.", "final_layer_norm.")
    return {("text_model." + k if k.startswith(bare) else k): v for k, v in state.items()}


def _act(name):
    if name == "quick_gelu":
        return lambda x: x * torch.sigmoid(1.702 * x)
    if name == "gelu":
        return F.gelu
    raise ValueError(f"CLIP activation {name!r} is not built (quick_gelu, gelu)")


class CLIPAttention(nn.Module):
    def __init__(self, width, heads):
        super().__init__()
        if width % heads:
            raise ValueError(f"width {width} is no multiple of {heads} heads")
        self.heads, self.scale = heads, (width // heads) ** -0.5
        self.k_proj = nn.Linear(width, width)
        self.v_proj = nn.Linear(width, width)
        self.q_proj = nn.Linear(width, width)
        self.out_proj = nn.Linear(width, width)

    def _stacked(self):
        from .. import ops
        ws = [self.q_proj.weight, self.k_proj.weight, self.v_proj.weight]
        bs = [self.q_proj.bias, self.k_proj.bias, self.v_proj.bias]
        return (ops.cached(ws[0], ("text_qkv_w", *map(id, ws)), ws, lambda: torch.cat([w.detach() for w in ws]).contiguous()),
                ops.cached(bs[0], ("text_qkv_b", *map(id, bs)), bs, lambda: torch.cat([b.detach() for b in bs]).contiguous()))

    def forward(self, x):
        if x.is_cuda:
            from .. import ops
            w, b = self._stacked()
            return self.out_proj(ops.text_attention(F.linear(x, w, b), None, None, self.heads, self.scale))
        routes.note("text.attention", "host")
        n, L, C = x.shape
        q, k, v = (p(x).view(n, L, self.heads, C // self.heads).transpose(1, 2) for p in (self.q_proj, self.k_proj, self.v_proj))
        s = (q @ k.transpose(-1, -2)) * self.scale
        s = s.masked_fill(torch.ones(L, L, dtype=torch.bool, device=x.device).triu(1), float("-inf"))
        return self.out_proj((torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(n, L, C))


class CLIPMLP(nn.Module):
    def __init__(self, width, inner, act):
        super().__init__()
        self.fc1 = nn.Linear(width, inner)
        self.fc2 = nn.Linear(inner, width)
        self._act = _act(act)

    def forward(self, x):
        return self.fc2(self._act(self.fc1(x)))


class CLIPEncoderLayer(nn.Module):
    def __init__(self, width, heads, inner, act, eps):
        super().__init__()
        self.self_attn = CLIPAttention(width, heads)
        self.layer_norm1 = nn.LayerNorm(width, eps=eps)
        self.mlp = CLIPMLP(width, inner, act)
        self.layer_norm2 = nn.LayerNorm(width, eps=eps)


class CLIPEncoder(nn.Module):
    def __init__(self, n_layers, *a):
        super().__init__()
        self.layers = nn.ModuleList([CLIPEncoderLayer(*a) for _ in range(n_layers)])


class CLIPTextEmbeddings(nn.Module):
    def __init__(self, vocab, width, positions):
        super().__init__()
        self.token_embedding = nn.Embedding(vocab, width)
        self.position_embedding = nn.Embedding(positions, width)

    def forward(self, input_ids):
        L = input_ids.shape[1]
        if L > self.position_embedding.num_embeddings:
            raise ValueError(f"{L} tokens, the tower has {self.position_embedding.num_embeddings} positions")
        return self.token_embedding(input_ids) + self.position_embedding.weight[:L]


class CLIPTextTransformer(nn.Module):
    def __init__(self, vocab, width, n_layers, heads, inner, act, positions, eps):
        super().__init__()
        self.embeddings = CLIPTextEmbeddings(vocab, width, positions)
        self.encoder = CLIPEncoder(n_layers, width, heads, inner, act, eps)
        self.final_layer_norm = nn.LayerNorm(width, eps=eps)

    def forward(self, input_ids):
        """-> (final_layer_norm(last), input of the last layer, last before the final norm)"""
        x = self.embeddings(input_ids)
        layers = self.encoder.layers
        if x.is_cuda:
            from .. import ops
            norms = [self.final_layer_norm] + [l.layer_norm1 for l in layers] + [l.layer_norm2 for l in layers]
            if any(p.requires_grad for nm in norms for p in nm.parameters()):
                raise RuntimeError("CLIP text tower: its LayerNorm weights take gradients; the towers are frozen on the GPU route -- "
                                   "call requires_grad_(False) on the model (load_ldm(..., text_encoder=True) does)")
            if not all(ops.add_layer_norm_supported(x, nm) for nm in norms):
                raise RuntimeError(f"CLIP text tower of width {x.shape[-1]}: no residual + LayerNorm kernel for this width "
                                   "(include/skp.h: skp_add_layer_norm_ok)")
            x = x.contiguous()
            x, n = ops.add_layer_norm(None, x, layers[0].layer_norm1)
            before_last = x
            for i, l in enumerate(layers):
                before_last = x
                x, n = ops.add_layer_norm(x, l.self_attn(n), l.layer_norm2)
                nxt = layers[i + 1].layer_norm1 if i + 1 < len(layers) else self.final_layer_norm
                x, n = ops.add_layer_norm(x, l.mlp(n), nxt)
            return n, before_last, x
        before_last = x
        for l in layers:
            before_last = x
            x = x + l.self_attn(l.layer_norm1(x))
            x = x + l.mlp(l.layer_norm2(x))
        return self.final_layer_norm(x), before_last, x


class CLIPTextModel(nn.Module):
    """`projection_dim` None: transformers' CLIPTextModel; an int: CLIPTextModelWithProjection (bias-free `text_projection`).
    `eos_token_id`: the pooled row is the first position holding it (49407 in every published vocabulary; the built-in byte
    vocabulary's is 513)."""

    def __init__(self, vocab_size=49408, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                 hidden_act="quick_gelu", max_position_embeddings=77, layer_norm_eps=1e-5, projection_dim=None, eos_token_id=None):
        super().__init__()
        self.text_model = CLIPTextTransformer(vocab_size, hidden_size, num_hidden_layers, num_attention_heads, intermediate_size,
                                              hidden_act, max_position_embeddings, layer_norm_eps)
        if projection_dim is not None:
            self.text_projection = nn.Linear(hidden_size, projection_dim, bias=False)
        self.eos_token_id = vocab_size - 1 if eos_token_id is None else int(eos_token_id)
        if self.eos_token_id == 2:               # old configs carry 2 while the vocabulary's EOS is its last id
            self.eos_token_id = vocab_size - 1
        self.config = dict(vocab_size=vocab_size, hidden_size=hidden_size, num_hidden_layers=num_hidden_layers,
                           num_attention_heads=num_attention_heads, intermediate_size=intermediate_size, hidden_act=hidden_act,
                           max_position_embeddings=max_position_embeddings, layer_norm_eps=layer_norm_eps,
                           projection_dim=projection_dim, eos_token_id=self.eos_token_id)

    @property
    def width(self):
        return self.config["hidden_size"]

    @torch.no_grad()
    def forward(self, input_ids, penultimate=False):
        """input_ids: int64 [n, L] -> (hidden [n, L, width], pooled [n, width or projection_dim]).  `hidden` is
        final_layer_norm(last layer), or with `penultimate` the input of the last layer without the final norm."""
        if input_ids.dim() != 2:
            raise ValueError(f"input_ids must be [n, L], got {tuple(input_ids.shape)}")
        input_ids = input_ids.to(self.text_model.embeddings.token_embedding.weight.device)
        last, before_last, _ = self.text_model(input_ids)
        eos = (input_ids == self.eos_token_id).int().argmax(dim=-1)        # first EOS (no EOS in a row: position 0)
        pooled = last[torch.arange(last.shape[0], device=last.device), eos]
        if hasattr(self, "text_projection"):
            pooled = self.text_projection(pooled)
        return (before_last if penultimate else last), pooled


def n_params(model) -> int:
    return sum(p.numel() for p in model.parameters())
