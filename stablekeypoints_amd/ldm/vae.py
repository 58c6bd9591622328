"""Build-owned SD `AutoencoderKL` with the diffusers==0.8.0 module tree [3P].

`encode(x)["latent_dist"].mean` is on the reference's optimisation path (ptp_utils.py:289-304) and is always built.  The DECODER half
(`decoder.*`, `post_quant_conv`) serves image sampling only (ptp_utils.py `latent2image` / `text2image_ldm_stable`) and is built
on request -- `AutoencoderKL.add_decoder(seed)` -- after everything else and from a generator of its own, so the encoder's
seeded synthetic weights and the `state_dict()` keys of a model without a decoder do not depend on it.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .attention import AttentionBlock
from .unet import ResnetBlock2D, Downsample2D, Upsample2D


class DownEncoderBlock2D(nn.Module):
    def __init__(self, in_ch, out_ch, num_layers=2, add_downsample=True):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(in_ch if i == 0 else out_ch, out_ch, temb_ch=None, eps=1e-6)
                                      for i in range(num_layers)])
        self.downsamplers = nn.ModuleList([Downsample2D(out_ch, padding=0)]) if add_downsample else None

    def forward(self, h):
        for r in self.resnets:
            h = r(h)
        if self.downsamplers is not None:
            h = self.downsamplers[0](h)
        return h


class UNetMidBlock2D(nn.Module):
    def __init__(self, ch):
        super().__init__()
        self.attentions = nn.ModuleList([AttentionBlock(ch, None, groups=32, eps=1e-6)])
        self.resnets = nn.ModuleList([ResnetBlock2D(ch, ch, temb_ch=None, eps=1e-6), ResnetBlock2D(ch, ch, temb_ch=None, eps=1e-6)])

    def forward(self, h):
        h = self.resnets[0](h)
        h = self.attentions[0](h)
        return self.resnets[1](h)


class Encoder(nn.Module):
    def __init__(self, in_channels=3, latent_channels=4, block_out_channels=(128, 256, 512, 512), layers_per_block=2):
        super().__init__()
        boc = list(block_out_channels)
        self.conv_in = nn.Conv2d(in_channels, boc[0], 3, padding=1)
        blocks, ch = [], boc[0]
        for i, oc in enumerate(boc):
            blocks.append(DownEncoderBlock2D(ch, oc, layers_per_block, add_downsample=i != len(boc) - 1))
            ch = oc
        self.down_blocks = nn.ModuleList(blocks)
        self.mid_block = UNetMidBlock2D(boc[-1])
        self.conv_norm_out = nn.GroupNorm(32, boc[-1], eps=1e-6)
        self.conv_out = nn.Conv2d(boc[-1], 2 * latent_channels, 3, padding=1)

    def forward(self, x):
        h = self.conv_in(x)
        for b in self.down_blocks:
            h = b(h)
        h = self.mid_block(h)
        return self.conv_out(F.silu(self.conv_norm_out(h)))


class UpDecoderBlock2D(nn.Module):
    def __init__(self, in_ch, out_ch, num_layers=3, add_upsample=True):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(in_ch if i == 0 else out_ch, out_ch, temb_ch=None, eps=1e-6)
                                      for i in range(num_layers)])
        self.upsamplers = nn.ModuleList([Upsample2D(out_ch)]) if add_upsample else None

    def forward(self, h):
        for r in self.resnets:
            h = r(h)
        if self.upsamplers is not None:
            h = self.upsamplers[0](h)
        return h


class Decoder(nn.Module):
    def __init__(self, latent_channels=4, out_channels=3, block_out_channels=(128, 256, 512, 512), layers_per_block=2):
        super().__init__()
        rev = list(reversed(block_out_channels))
        self.conv_in = nn.Conv2d(latent_channels, rev[0], 3, padding=1)
        self.mid_block = UNetMidBlock2D(rev[0])
        blocks, ch = [], rev[0]
        for i, oc in enumerate(rev):
            blocks.append(UpDecoderBlock2D(ch, oc, layers_per_block + 1, add_upsample=i != len(rev) - 1))
            ch = oc
        self.up_blocks = nn.ModuleList(blocks)
        self.conv_norm_out = nn.GroupNorm(32, rev[-1], eps=1e-6)
        self.conv_out = nn.Conv2d(rev[-1], out_channels, 3, padding=1)

    def forward(self, z, to_image=False):
        """`to_image`: return clamp(sample / 2 + 0.5, 0, 1), the [0, 1] image of `ptp_utils.latent2image`, instead of the sample."""
        h = self.mid_block(self.conv_in(z))
        for b in self.up_blocks:
            h = b(h)
        h = self.conv_out(F.silu(self.conv_norm_out(h)))
        return (h / 2 + 0.5).clamp(0, 1) if to_image else h


class DiagonalGaussianDistribution:
    def __init__(self, parameters: torch.Tensor):
        self.mean, self.logvar = torch.chunk(parameters, 2, dim=1)


class AutoencoderKL(nn.Module):
    def __init__(self, latent_channels=4, block_out_channels=(128, 256, 512, 512)):
        super().__init__()
        self.encoder = Encoder(3, latent_channels, block_out_channels)
        self.quant_conv = nn.Conv2d(2 * latent_channels, 2 * latent_channels, 1)
        self._decoder_cfg = (latent_channels, tuple(block_out_channels))

    def encode(self, x):
        return {"latent_dist": DiagonalGaussianDistribution(self.quant_conv(self.encoder(x)))}

    @property
    def has_decoder(self) -> bool:
        return "decoder" in self._modules

    def add_decoder(self, seed=0):
        """Build `decoder` and `post_quant_conv` (PyTorch default inits) from a generator of their own, seeded with `seed`: the
        global generator is left where it was, so nothing drawn before or after changes.  Parameters are drawn on the CPU and then
        moved to the encoder's device and dtype.  Returns self."""
        if self.has_decoder:
            return self
        latent_channels, boc = self._decoder_cfg
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            with torch.device("cpu"):
                decoder = Decoder(latent_channels, 3, boc)
                post_quant_conv = nn.Conv2d(latent_channels, latent_channels, 1)
        ref = self.quant_conv.weight
        self.decoder = decoder.to(device=ref.device, dtype=ref.dtype)
        self.post_quant_conv = post_quant_conv.to(device=ref.device, dtype=ref.dtype)
        self.decoder.train(self.training)
        self.post_quant_conv.train(self.training)
        return self

    def decode(self, z, to_image=False):
        if not self.has_decoder:
            raise RuntimeError("this AutoencoderKL was built without its decoder half: load the model with decoder=True "
                               "(optimize_token.load_ldm(..., decoder=True) / from_pretrained(..., with_decoder=True)), or call "
                               "vae.add_decoder(seed)")
        return {"sample": self.decoder(self.post_quant_conv(z), to_image=to_image)}
