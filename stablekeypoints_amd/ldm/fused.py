"""Fused execution of the frozen UNet/VAE blocks on the HIP kernels (GroupNorm+offset+SiLU).

`fuse_norms(module)` swaps the `forward` of every `ResnetBlock2D` / `Transformer2DModel` /
`AttentionBlock` / final-norm site for a version that is mathematically the module's own forward
(same weights, same order of operations per element) but runs
    conv1(no bias) -> [bias + time embedding folded into the norm's per-(n,c) offset] -> GN+SiLU
as ONE fused kernel pair instead of bias-add, temb-add, GroupNorm statistics, GroupNorm apply and SiLU
passes.  CUDA fp32 only; anything else falls through to the module's original forward.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import ops
from .. import routes
from .attention import AttentionBlock, BasicTransformerBlock, Transformer2DModel
from .unet import Downsample2D, ResnetBlock2D, UNet2DConditionModel, Upsample2D
from .vae import Decoder


def _resnet_forward(m: ResnetBlock2D):
    orig = m.forward

    def forward(x, temb=None):
        if not ops.group_norm_supported(x, m.norm1.num_groups):
            routes.note("resnet", "eager")
            return orig(x, temb)
        routes.note("resnet", "fused")
        # where the convolution runs with one output-channel group and no autograd (the VAE's first level: 128 -> 128 at the
        # image resolution, 1 GB activations) the norm is applied inside the convolution's patch load: no apply pass
        if ops.conv3x3_gn_fold_ok(x, m.norm1, m.conv1.weight):
            h = ops.conv3x3_gn_silu(x, m.norm1, m.conv1.weight, want_stats=True)
        else:
            # (statistics from x's producer when it left them); x' = x for the residual path below: its gradient is added
            # inside norm1's input-gradient kernel
            h, x = ops.group_norm_silu_fork(x, m.norm1)
            h = ops.conv3x3_auto(h, m.conv1.weight, want_stats=True)     # bias folded into norm2's offset
        off = _norm2_offset(m, x.shape[0], temb)
        bias = m.conv2.bias
        res = x
        if m.conv_shortcut is not None:
            # 1x1 shortcut = one batched GEMM on the NCHW planes (no layout transposes); its bias joins conv2's
            res, bias = ops.conv1x1_nobias(x, m.conv_shortcut.weight), _summed_bias(m)
        if ops.conv3x3_gn_fold_ok(h, m.norm2, m.conv2.weight, off, bias, res):
            return ops.conv3x3_gn_silu(h, m.norm2, m.conv2.weight, off=off, bias=bias, residual=res, want_stats=True)
        h = ops.group_norm_silu(h, m.norm2, off=off)
        # bias + shortcut in the conv epilogue; its block sums serve the next block's first norm
        return ops.conv3x3_auto(h, m.conv2.weight, bias, residual=res, want_stats=True)
    return forward


def _norm2_offset(m: ResnetBlock2D, rows: int, temb):
    """Per-(row, channel) offset in front of norm2: conv1.bias + time_emb_proj(silu(temb)), contiguous [rows, C].  With the
    time path kept by `_time_path` below the SAME `temb` tensor arrives every step, and the offset of a frozen block is kept
    with it, one per row count (4 small launches per block and step otherwise)."""
    def build():
        off = m.conv1.bias[None, :].expand(rows, -1)
        if m.time_emb_proj is not None and temb is not None:
            off = off + m.time_emb_proj(F.silu(temb))
        return off.contiguous()
    proj = m.time_emb_proj.parameters() if m.time_emb_proj is not None else ()
    return ops.cached(m, ("norm2_offset", rows), (m.conv1.bias, *proj, temb), build)


def _time_path(m: UNet2DConditionModel):
    """The time embedding of a frozen UNet depends on (timestep values, rows) only, and on this path the timestep is a host
    value (`scheduler.timesteps[noise_level]`, ptp_utils.py:219-221) that never changes during an optimisation: keep the
    embedding per key, so every step hands the resnets the same tensor."""
    orig = m.time_path

    def time_path(sample, timestep, added_cond_kwargs=None):
        host = not torch.is_tensor(timestep) or (timestep.device.type == "cpu" and timestep.numel() <= 64)
        tag = ops.frozen_tag([*m.time_embedding.parameters(), *(m.add_embedding.parameters() if m.add_embedding is not None else ())])
        if not host or tag is None or added_cond_kwargs is not None:
            routes.note("time_embedding", "eager")
            return orig(sample, timestep, added_cond_kwargs)
        vals = tuple(float(v) for v in (timestep.reshape(-1).tolist() if torch.is_tensor(timestep) else [timestep]))
        key = (vals, int(sample.shape[0]), tuple(sample.shape[-2:]), sample.device, sample.dtype, tag)
        memo = m.__dict__.setdefault("_skp_temb", {})
        hit = memo.get(key)
        if hit is None:
            if len(memo) >= 8:
                memo.clear()
            with torch.no_grad():
                hit = orig(sample, timestep, added_cond_kwargs)
            memo[key] = hit
        return ops.handed_out(hit)              # (a captured step holds it: the memo may drop it)
    return time_path


def _summed_bias(m: ResnetBlock2D):
    """conv2.bias + conv_shortcut.bias of a frozen block, cached against the parameters' versions."""
    b2, bs = m.conv2.bias, m.conv_shortcut.bias
    if bs is None:
        return b2
    return ops.cached(m, "bias_sum", (b2, bs), lambda: b2 + bs)


def _transformer_forward(m: Transformer2DModel):
    orig = m.forward

    def forward(x, context=None):
        if not ops.group_norm_supported(x, m.norm.num_groups):
            routes.note("transformer2d", "eager")
            return orig(x, context)
        if not ops.layout_supported(x):
            routes.note("transformer2d", "eager")
            return orig(x, context)                  # the module's own forward knows both projection layouts
        routes.note("transformer2d", "fused")
        h, x = ops.group_norm_silu_fork(x, m.norm, silu=False)          # x' = x for the residual add at the end
        # token layout throughout: the 1x1 convolutions are nn.Linear over tokens (bias fused in the GEMM), the two
        # permutes are tiled transposes and the residual add rides on the way back
        t = ops.nchw_to_tokens(h)
        t = F.linear(t, m.proj_in.weight.flatten(1), m.proj_in.bias)
        for blk in m.transformer_blocks:
            t = blk(t, context=context)
        t = F.linear(t, m.proj_out.weight.flatten(1), m.proj_out.bias)
        return ops.tokens_to_nchw_add(t, x)
    return forward


def _block_forward(m: BasicTransformerBlock):
    """`attn(norm(h)) + h` three times over: every residual add rides in the NEXT norm's kernel (ops.add_layer_norm), and the
    gradient that reaches the residual stream from its later uses is added inside that norm's input-gradient kernel."""
    orig = m.forward

    def forward(h, context=None):
        if not (ops.add_layer_norm_supported(h, m.norm1) and ops.add_layer_norm_supported(h, m.norm2)
                and ops.add_layer_norm_supported(h, m.norm3)):
            routes.note("transformer_block", "eager")
            return orig(h, context=context)
        routes.note("transformer_block", "fused")
        h, n = ops.add_layer_norm(None, h, m.norm1)
        h, n = ops.add_layer_norm(m.attn1(n), h, m.norm2)
        h, n = ops.add_layer_norm(m.attn2(n, context=context), h, m.norm3)
        return m.ff(n) + h
    return forward


def _vae_attention_forward(m: AttentionBlock):
    """VAE mid-block attention: GroupNorm on the fused kernel, tiled NCHW -> token transpose instead of a strided copy, the
    way back fused with the residual add.  The d = 512 single-head core: the wide flash kernel or the library GEMMs + softmax,
    as `ops.vae_attn_route` says (the kernel has no backward)."""
    orig = m.forward

    def forward(x):
        if not (ops.group_norm_supported(x, m.group_norm.num_groups) and ops.layout_supported(x)):
            routes.note("vae.attention", "eager")
            return orig(x)
        b, c, hh, ww = x.shape
        nh = m.num_heads
        d = c // nh
        needs_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in m.parameters()))
        route = ops.vae_attn_route(b, nh, hh * ww, d, needs_grad)
        routes.note("vae.attention", route)
        t = ops.nchw_to_tokens(ops.group_norm_silu(x, m.group_norm, silu=False))        # [b, hh*ww, c]
        q, k, v = m.query(t), m.key(t), m.value(t)
        if route == "flash_wide":
            return ops.tokens_to_nchw_add(m.proj_attn(ops.flash_attn_wide(q, k, v, nh, 1.0 / (d ** 0.5))), x)

        def split(u):
            return u.reshape(b, -1, nh, d).permute(0, 2, 1, 3).reshape(b * nh, -1, d)
        q, k, v = split(q), split(k), split(v)
        attn = torch.baddbmm(torch.empty(q.shape[0], q.shape[1], k.shape[1], dtype=q.dtype, device=q.device),
                             q, k.transpose(1, 2), beta=0, alpha=1.0 / (d ** 0.5)).softmax(dim=-1)
        o = torch.bmm(attn, v).reshape(b, nh, -1, d).permute(0, 2, 1, 3).reshape(b, -1, c)
        return ops.tokens_to_nchw_add(m.proj_attn(o), x)
    return forward


def _conv_forward(m: torch.nn.Conv2d):
    def forward(x):
        # (<= 4 input channels = a conv_in: its consumer is a ResnetBlock2D's first GroupNorm, which takes block statistics)
        return ops.conv3x3_auto(x, m.weight, m.bias, want_stats=m.weight.shape[1] <= 4)
    return forward


def _downsample_forward(m):
    """Downsample2D: the stride-2 convolution, its zero padding and its bias are one kernel (csrc/skp_conv_s2.hip); where the
    input needs a gradient (UNet) only the input gradient stays on the library.  Unsupported shapes: the module's own forward."""
    orig = m.forward

    def forward(x):
        frozen = not (m.conv.weight.requires_grad or (m.conv.bias is not None and m.conv.bias.requires_grad))
        if frozen and m.conv.stride == (2, 2) and ops.conv3x3_s2_supported(x, m.conv.weight):
            routes.note("downsample", "s2_direct")
            return ops.conv3x3_s2(x, m.conv.weight, m.conv.bias, pad=0 if m.padding == 0 else 1, want_stats=True)
        # (a layer the kernel refuses for its 16 x 32 pixel tile ALONE is a site of its own, a documented route; any other refusal --
        # unfrozen weights, stride, channels, CONV3X3_MODE -- is `downsample` / eager whatever the input's size)
        tile_only = frozen and m.conv.stride == (2, 2) and ops.conv3x3_s2_tile_only(x, m.conv.weight)
        routes.note("downsample.untiled" if tile_only else "downsample", "eager")
        return orig(x)
    return forward


def _upsample_forward(m: Upsample2D, always: bool):
    """Upsample2D: nearest 2x + 3x3 convolution as one kernel on the low-resolution input (ops.conv3x3_up2, which notes its route
    at the `upsample_conv` site).  `always`: the VAE decoder's up-samplers, which only ever run while sampling; the UNet's take it
    inside `ops.up2_in_unet()` alone -- everywhere else they run their own forward (interpolate + the patched convolution), route
    for route what the optimisation path has always noted."""
    def forward(x):
        frozen = not (m.conv.weight.requires_grad or (m.conv.bias is not None and m.conv.bias.requires_grad))
        if ((always or ops.up2_in_unet_enabled()) and frozen and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
                and not (torch.is_grad_enabled() and x.requires_grad)):
            return ops.conv3x3_up2(x, m.conv.weight, m.conv.bias)
        return m.conv(F.interpolate(x, scale_factor=2.0, mode="nearest"))    # the module's own forward: its convolution notes the route
    return forward


def _decoder_forward(m: Decoder):
    """VAE decoder: its resnets, mid-block attention, conv_in (4 -> C: the small-input kernel through the patched Conv2d) and
    up-samplers are patched module by module; this forward adds the tail -- GroupNorm + SiLU on the fused kernel and `conv_out`
    (C -> 3) on the small-output kernel, whose epilogue also makes the [0, 1] image when asked."""
    orig = m.forward

    def forward(z, to_image=False):
        if not (z.is_cuda and z.dtype == torch.float32 and not torch.is_grad_enabled()):
            routes.note("vae.decoder", "eager")
            return orig(z, to_image=to_image)
        routes.note("vae.decoder", "fused")
        with ops.conv3x3_own_kernels():              # (few-tile launches of a reduced-width tree stay on the HIP kernels)
            h = m.mid_block(m.conv_in(z))
            for blk in m.up_blocks:
                h = blk(h)
        h = (ops.group_norm_silu(h, m.conv_norm_out) if ops.group_norm_supported(h, m.conv_norm_out.num_groups)
             else F.silu(m.conv_norm_out(h)))
        co = m.conv_out
        if ops.conv3x3_small_out_ok(h, co.weight) and co.padding == (1, 1) and co.stride == (1, 1):
            return ops.conv3x3_small_out(h, co.weight, co.bias, image=to_image)
        y = co(h)                                    # (the patched Conv2d notes conv_out / lib)
        return (y / 2 + 0.5).clamp(0, 1) if to_image else y
    return forward


def _vae_encode(m):
    """`AutoencoderKL.encode` with the encoder's tail as ONE Winograd launch: `quant_conv` (1 x 1, 8 -> 8) after `conv_out` (3 x 3,
    512 -> 8) is a single 3 x 3 convolution with the composed filter `Wq . Wout` and bias `Wq . b_out + b_q` (exact algebra; the
    composition is built once per frozen weights), zero-padded to 32 output channels so that the F(4x4,3x3) kernels take it (8 channels
    are below their channel blocks: the library ran it as an NHWC implicit GEMM between two layout transposes, 0.33 ms per step for
    2.4 GF); GroupNorm + SiLU in front of it on the fused kernel."""
    orig = m.encode
    from .vae import DiagonalGaussianDistribution

    def compose():
        enc, q = m.encoder, m.quant_conv
        with torch.no_grad():
            wq = q.weight.flatten(1).double()                                   # [8, 8]
            w = (wq @ enc.conv_out.weight.double().flatten(1)).reshape(q.weight.shape[0], *enc.conv_out.weight.shape[1:])
            b = wq @ enc.conv_out.bias.double() + q.bias.double()
            co = w.shape[0]
            wp = torch.zeros(32, *w.shape[1:], device=w.device, dtype=torch.float32)
            bp = torch.zeros(32, device=w.device, dtype=torch.float32)
            wp[:co], bp[:co] = w.float(), b.float()
        return wp, bp

    def tail_params():
        return (m.encoder.conv_out.weight, m.encoder.conv_out.bias, m.quant_conv.weight, m.quant_conv.bias)

    def encode(x):
        enc, q = m.encoder, m.quant_conv
        ok = (x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled() and q.kernel_size == (1, 1)
              and q.weight.shape[0] <= 32 and enc.conv_out.kernel_size == (3, 3) and enc.conv_out.padding == (1, 1)
              and q.bias is not None and enc.conv_out.bias is not None and not any(p.requires_grad for p in tail_params()))
        if not ok:
            routes.note("vae.tail", "eager")
            return orig(x)
        h = enc.conv_in(x)
        for blk in enc.down_blocks:
            h = blk(h)
        h = enc.mid_block(h)
        if not (ops.group_norm_supported(h, enc.conv_norm_out.num_groups) and ops.conv3x3_wanted(h.shape, (32, h.shape[1], 3, 3))):
            routes.note("vae.tail", "eager")
            return {"latent_dist": DiagonalGaussianDistribution(q(enc.conv_out(F.silu(enc.conv_norm_out(h)))))}
        routes.note("vae.tail", "composed")
        wp, bp = ops.cached(m, "vae_tail", tail_params(), compose)
        h = ops.group_norm_silu(h, enc.conv_norm_out)
        y = ops.conv3x3_auto(h, wp, bp)
        return {"latent_dist": DiagonalGaussianDistribution(y[:, :q.weight.shape[0]])}
    return encode


def fuse_norms(module: torch.nn.Module) -> int:
    n = 0
    decoder_ups = {id(u) for d in module.modules() if isinstance(d, Decoder) for u in d.modules() if isinstance(u, Upsample2D)}
    for mod in module.modules():
        if isinstance(mod, Decoder) and "forward" not in mod.__dict__:
            mod.forward = _decoder_forward(mod); n += 1
            continue
        if isinstance(mod, Upsample2D) and "forward" not in mod.__dict__:
            mod.forward = _upsample_forward(mod, id(mod) in decoder_ups)    # (its .conv is patched below like any 3 x 3 Conv2d)
            continue
        if mod.__class__.__name__ == "AutoencoderKL" and hasattr(mod, "quant_conv") and "encode" not in mod.__dict__:
            mod.encode = _vae_encode(mod); n += 1
            continue
        if isinstance(mod, UNet2DConditionModel) and "time_path" not in mod.__dict__:
            mod.time_path = _time_path(mod)
            continue
        if isinstance(mod, Downsample2D) and "forward" not in mod.__dict__:
            mod.forward = _downsample_forward(mod); n += 1
            continue
        if (isinstance(mod, torch.nn.Conv2d) and mod.kernel_size == (3, 3) and mod.stride == (1, 1)
                and mod.padding == (1, 1) and mod.dilation == (1, 1) and mod.groups == 1
                and mod.padding_mode == "zeros" and "forward" not in mod.__dict__):
            mod.forward = _conv_forward(mod)        # Upsample2D.conv and friends (resnet convs are called below)
            continue
        if isinstance(mod, AttentionBlock) and "forward" not in mod.__dict__:
            mod.forward = _vae_attention_forward(mod); n += 1
            continue
        if isinstance(mod, BasicTransformerBlock) and "forward" not in mod.__dict__:
            mod.forward = _block_forward(mod); n += 1
            continue
        if isinstance(mod, ResnetBlock2D) and "forward" not in mod.__dict__:
            mod.forward = _resnet_forward(mod); n += 1
        elif isinstance(mod, Transformer2DModel) and "forward" not in mod.__dict__:
            mod.forward = _transformer_forward(mod); n += 1
    return n
