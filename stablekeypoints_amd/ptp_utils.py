"""Attention plumbing with the reference's API (ptp_utils.py) on the MI355X kernels.

Kept names/signatures: `AttentionControl`, `AttentionStore`,
`register_attention_control`, `find_pred_noise`, `run_and_find_attn`, `image2latent`,
`find_top_k_gaussian`, `furthest_point_sampling`, `init_random_noise`, and the image-sampling entries `diffusion_step`,
`latent2image`, `init_latent`, `latent_step`, `text2image_ldm_stable` (ptp_utils.py:307-349,420-461); `init_latents` and
`guided_latent_step` are this port's batched / classifier-free-guidance companions of the last two, `sampler_latent_step` the step
of the named samplers (ldm/samplers.py), `keypoint_energy_grad` the energy and latent gradient of keypoint guidance
(`text2image_ldm_stable(keypoints=...)`), `pose_targets` / `gaussian_target_maps` the target maps of pose transfer
(`text2image_ldm_stable(target_maps=...)`).

What changes under the hood
  * the hooked cross-attention does NOT up-sample the layer input, re-project it and materialise a
    (B*h, R^2, T) tensor per layer (ptp_utils.py:513-538).  It records a light `FusedAttn` handle
    (q = to_q(x) which the ordinary attention needs anyway, k = to_k(context)); `collect_maps`
    turns all handles into the reduced [T,R,R] map with ONE fused HIP kernel
    (csrc/skp_attn_map.hip).  `AttentionStore.step_store["attn"]` still is a list whose length is
    the gate the patcher reads (ptp_utils.py:511); `FusedAttn.materialize()` yields the reference's
    tensor on demand (compat / tests);
  * token selection never leaves the device (no `.item()`), see csrc/skp_select_loss.hip.
"""
from __future__ import annotations

import abc
import contextlib
from typing import NamedTuple, Optional

import numpy as np

import torch

from . import ops
from . import routes
from .ldm.samplers import SamplerPlan, step_formula
from .ldm.unet import StopForward
from ._maps import FusedAttn, _materialize_host, collect_maps, stack_of


# ---------------------------------------------------------------------------------------------
# controllers                                                       reference ptp_utils.py:32-83
# ---------------------------------------------------------------------------------------------
class AttentionControl(abc.ABC):
    def step_callback(self, x_t):
        return x_t

    def between_steps(self):
        return

    @property
    def num_uncond_att_layers(self):
        return 0

    @abc.abstractmethod
    def forward(self, dict, is_cross: bool, place_in_unet: str):
        raise NotImplementedError

    def __call__(self, dict, is_cross: bool, place_in_unet: str):
        dict = self.forward(dict, is_cross, place_in_unet)
        return dict["attn"]

    def reset(self):
        self.cur_step = 0
        self.cur_att_layer = 0

    def __init__(self):
        self.cur_step = 0
        self.num_att_layers = -1
        self.cur_att_layer = 0


class AttentionStore(AttentionControl):
    """`step_store["attn"]` holds one entry per hooked layer: a `FusedAttn` handle (default) or, with
    `materialize=True`, the reference-layout tensor (B*h, R^2, T)."""

    @staticmethod
    def get_empty_store():
        return {"attn": []}

    def forward(self, dict, is_cross: bool, place_in_unet: str):
        self.step_store["attn"].append(dict["attn"])
        return dict

    def reset(self):
        super(AttentionStore, self).reset()
        self.step_store = self.get_empty_store()

    def __init__(self, materialize: bool = False):
        super(AttentionStore, self).__init__()
        self.step_store = self.get_empty_store()
        self.materialize = materialize
        self.stop_after: Optional[int] = None      # early exit once this many maps are stored


MAX_STORED_LAYERS = 4          # ptp_utils.py:511
MAX_STORED_SEQ = 32 ** 2       # ptp_utils.py:510


# ---------------------------------------------------------------------------------------------
# context projections of one forward                          reference ptp_utils.py:513-520
# ---------------------------------------------------------------------------------------------
CTX_KV_BATCHED = True        # False (tests): every layer projects the context for itself
_CTX_KV = {}                 # id(CrossAttention module) -> (k, v) [1,T,C] of the forward in flight


def _ctx_layer_ok(m, width):
    return (m.to_k.bias is None and m.to_v.bias is None and not m.to_k.weight.requires_grad and not m.to_v.weight.requires_grad
            and m.to_k.weight.shape[1] == width and "forward" not in m.to_k.__dict__ and "forward" not in m.to_v.__dict__)


def _context_kv_begin(unet, context, early_exit=False):
    """k = to_k(context), v = to_v(context) of the cross-attention layers for the ONE shared context row, before the UNet
    runs: the reference expands the learned embedding to the batch and projects it inside every layer (B x 77 rows through
    2 x 16 small GEMMs, as many again backward plus their accumulation adds).  The rows are identical, the weights frozen
    and bias-free: one batched GEMM per layer width (stacked weights, broadcast A operand) gives every layer its [1,T,C]
    pair, the attention kernels take a shared k / v (Bk = 1) and autograd sums the layers' gradients in one stack + one
    batched GEMM per width.  Layers that did not consume their pair in an earlier forward (beyond the early exit) are left
    out from the second forward on; a layer without a pair projects for itself, as before."""
    _CTX_KV.clear()
    if not (CTX_KV_BATCHED and context.is_cuda and context.dim() == 3 and context.shape[0] == 1):
        return
    plan = getattr(unet, "_skp_ctx_plan", None)
    # the plan holds only layers whose projections are frozen, bias-free and unpatched -- re-checked on every forward (32
    # modules): a layer that was unfrozen or re-patched since must project for itself again, or its weights would silently
    # get no gradient
    if plan is None or not all(_ctx_layer_ok(m, context.shape[-1]) for m in plan["mods"]):
        mods = [m.attn2 for m in unet.modules() if m.__class__.__name__ == "BasicTransformerBlock" and hasattr(m, "attn2")]
        mods = [m for m in mods if _ctx_layer_ok(m, context.shape[-1])]
        plan = {"mods": mods, "used": {}, "ids": {id(m) for m in mods}}
        unet._skp_ctx_plan = plan
    # which layers consume their pair depends on where the forward ends: one record per mode (early exit / full forward)
    used = plan["used"].get(bool(early_exit))
    mods = plan["mods"] if used is None else [m for m in plan["mods"] if id(m) in used]
    if used is None:
        used = plan["used"][bool(early_exit)] = set()
    _CTX_KV["plan"] = {"ids": plan["ids"], "used": used}
    groups = {}
    for m in mods:
        groups.setdefault(m.to_k.weight.shape[0], []).append(m)
    ctx2 = context[0]
    for c, ms in groups.items():
        w = ops.weight_stack([t for m in ms for t in (m.to_k.weight, m.to_v.weight)])        # [2n, C, Dctx], made once
        kv = torch.bmm(ctx2.unsqueeze(0).expand(w.shape[0], -1, -1), w.transpose(1, 2)).unbind(0)
        for i, m in enumerate(ms):
            _CTX_KV[id(m)] = (kv[2 * i].unsqueeze(0), kv[2 * i + 1].unsqueeze(0), used)


def _context_kv_end():
    _CTX_KV.clear()


def _context_kv(module):
    """(k, v) of `module` for the forward in flight, or None (no shared-context forward, or the layer was left out: it
    projects for itself this time and is part of the batch from the next forward on)."""
    hit = _CTX_KV.get(id(module))
    if hit is None:
        plan = _CTX_KV.get("plan")
        if plan is not None and id(module) in plan["ids"]:
            plan["used"].add(id(module))
        return None
    hit[2].add(id(module))
    return hit[0], hit[1]


def _attention_core(module, q, k, v, is_cross=False):
    """softmax(scale q k^T) v per head (ptp_utils.py:493-506) on [B,N,C]/[B,T,C] tensors.  Cross layers with
    a short key axis run on the fused fp32-MFMA kernel (csrc/skp_cross_attn.hip); self-attention runs on the
    flash-style kernels (csrc/skp_flash_attn.hip, csrc/skp_self_attn.hip).  On the GPU there is NO other route: a head
    size without a kernel raises.  Host tensors (the module tree on CPU is what oracle/ drives) take the plain
    baddbmm / softmax / bmm formulation of the reference."""
    if q.is_cuda:
        if is_cross and ops.cross_attn_supported(q.shape[-1], module.heads, k.shape[1]):
            return ops.cross_attention(q, k, v, module.heads, module.scale)
        if ops.self_attn_supported(q.shape[-1], module.heads):
            return ops.self_attention(q, k, v, module.heads, module.scale)
        raise RuntimeError(f"attention with {module.heads} heads of {q.shape[-1] // module.heads} channels has no HIP kernel "
                           f"(built head sizes: {ops.CROSS_ATTN_HEAD_DIMS}); there is no eager fallback on the GPU")
    routes.note("attn.cross" if is_cross else "attn.self", "host")
    qh = module.reshape_heads_to_batch_dim(q)
    kh = module.reshape_heads_to_batch_dim(k)
    vh = module.reshape_heads_to_batch_dim(v)
    attn = torch.baddbmm(torch.empty(qh.shape[0], qh.shape[1], kh.shape[1], dtype=q.dtype, device=q.device),
                         qh, kh.transpose(1, 2), beta=0, alpha=module.scale).softmax(dim=-1)
    return module.reshape_batch_dim_to_heads(torch.bmm(attn, vh))


def register_attention_control(model, controller, feature_upsample_res=256):
    """Same contract as ptp_utils.py:472-573: patches `.forward` of every module whose class is named
    `CrossAttention` under top-level children whose name contains "up", sets
    `controller.num_att_layers`, asserts that at least one layer was found."""

    def ca_forward(self, place_in_unet):
        to_out = self.to_out[0] if isinstance(self.to_out, torch.nn.ModuleList) else self.to_out

        def forward(x, context=None, mask=None):
            if mask is not None:
                raise NotImplementedError("attention masks are never used on this path (ptp_utils.py:496)")
            batch_size, sequence_length, dim = x.shape
            is_cross = context is not None
            ctx = context if is_cross else x
            stop = getattr(controller, "stop_after", None)
            if (is_cross and stop is not None and sequence_length <= MAX_STORED_SEQ
                    and len(controller.step_store["attn"]) + 1 >= min(stop, MAX_STORED_LAYERS)
                    and len(controller.step_store["attn"]) < MAX_STORED_LAYERS):
                # early exit: this is the LAST map the gate will store and the forward ends here (the caller discards the
                # prediction, ptp_utils.py:246) -- the layer's value projection and attention output have no consumer
                pre = _context_kv(self)
                rec = FusedAttn(self.to_q(x), pre[0] if pre is not None else self.to_k(ctx), self.heads, self.scale,
                                feature_upsample_res)
                if getattr(controller, "materialize", False):
                    rec = rec.materialize()
                controller({"attn": rec}, is_cross, place_in_unet)
                raise StopForward()
            if (not is_cross) and self.to_q.bias is None and self.to_k.bias is None and self.to_v.bias is None \
                    and "forward" not in self.to_q.__dict__:
                if x.is_cuda and ops.self_attn_supported(dim, self.heads):
                    return to_out(ops.self_attention_block(x, self.to_q.weight, self.to_k.weight, self.to_v.weight,
                                                           self.heads, self.scale))
                q, k, v = ops.qkv_proj(x, self.to_q.weight, self.to_k.weight, self.to_v.weight)
            else:
                q = self.to_q(x)
                pre = _context_kv(self) if is_cross else None
                k, v = pre if pre is not None else (self.to_k(ctx), self.to_v(ctx))
            out = _attention_core(self, q, k, v, is_cross)
            if (is_cross and sequence_length <= MAX_STORED_SEQ
                    and len(controller.step_store["attn"]) < MAX_STORED_LAYERS):
                rec = FusedAttn(q, k, self.heads, self.scale, feature_upsample_res)
                if getattr(controller, "materialize", False):
                    rec = rec.materialize()
                controller({"attn": rec}, is_cross, place_in_unet)
                stop = getattr(controller, "stop_after", None)
                if stop is not None and len(controller.step_store["attn"]) >= stop:
                    raise StopForward()
            elif (is_cross and sequence_length > MAX_STORED_SEQ and controller.step_store["attn"]
                  and getattr(controller, "stop_after", None) is not None):
                # only `up` blocks are hooked and their resolution never decreases: once a cross layer is past the
                # 32^2 gate no later layer can store (SD-2.x at 768^2 stores 3 layers, not 4) => nothing left to record
                raise StopForward()
            return to_out(out)

        return forward

    class DummyController:
        def __call__(self, *args):
            return args[0]

        def __init__(self):
            self.num_att_layers = 0
            self.step_store = {"attn": []}

    if controller is None:
        controller = DummyController()

    def register_recr(net_, count, place_in_unet):
        if net_.__class__.__name__ == "CrossAttention":
            net_.forward = ca_forward(net_, place_in_unet)
            return count + 1
        elif hasattr(net_, "children"):
            for net__ in net_.children():
                count = register_recr(net__, count, place_in_unet)
        return count

    cross_att_count = 0
    for name, child in model.named_children():
        if "up" in name:
            cross_att_count += register_recr(child, 0, "up")
    controller.num_att_layers = cross_att_count
    model.__dict__["_skp_hook_controller"] = controller        # (the sampling loop empties the hooked store after every forward)
    model.__dict__["_skp_hook_res"] = int(feature_upsample_res)     # R of the stored maps (pose transfer resamples its targets to it)
    assert cross_att_count != 0, ("No cross attention layers found in the model. The module tree must use the "
                                  "diffusers==0.8.0 `CrossAttention` layout.")


def accelerate_cross_attention(net):
    """Route the UNPATCHED (down/mid) cross-attention layers through the same fused kernel; they never store
    maps (the reference only hooks `up` blocks, ptp_utils.py:565-568) so only their `forward` core changes."""
    for mod in net.modules():
        if mod.__class__.__name__ == "CrossAttention" and "forward" not in mod.__dict__:
            def make(m):
                to_out = m.to_out[0] if isinstance(m.to_out, torch.nn.ModuleList) else m.to_out

                def forward(x, context=None, mask=None):
                    is_cross = context is not None
                    ctx = context if is_cross else x
                    if (not is_cross) and m.to_q.bias is None and m.to_k.bias is None and m.to_v.bias is None:
                        if x.is_cuda and ops.self_attn_supported(x.shape[-1], m.heads):
                            return to_out(ops.self_attention_block(x, m.to_q.weight, m.to_k.weight, m.to_v.weight, m.heads,
                                                                   m.scale))
                        q, k, v = ops.qkv_proj(x, m.to_q.weight, m.to_k.weight, m.to_v.weight)
                        return to_out(_attention_core(m, q, k, v, False))
                    pre = _context_kv(m) if is_cross else None
                    k, v = pre if pre is not None else (m.to_k(ctx), m.to_v(ctx))
                    return to_out(_attention_core(m, m.to_q(x), k, v, is_cross))
                return forward
            mod.forward = make(mod)


# ---------------------------------------------------------------------------------------------
# noised forward driver                                    reference ptp_utils.py:205-304
# ---------------------------------------------------------------------------------------------
def image2latent(model, image, device):
    """ptp_utils.py:289-304: [0,1] image -> *2-1 -> VAE posterior mean * 0.18215.  Accepts the reference's
    numpy NHWC array or a [B,3,H,W] tensor (no CPU round trip for tensors)."""
    with torch.no_grad():
        if isinstance(image, np.ndarray):
            image = torch.from_numpy(image).float().permute(0, 3, 1, 2)
        image = image.to(device=device, dtype=torch.float32) * 2 - 1
        vae = model.vae.module if isinstance(model.vae, torch.nn.DataParallel) else model.vae
        latents = vae.encode(image)["latent_dist"].mean
        return latents * 0.18215


def find_pred_noise(ldm, image, context, noise_level=-1, device="cuda", noise=None, early_exit=False,
                    controllers=None, latents=None):
    """ptp_utils.py:205-231.  `noise` lets a caller inject the gaussian (the reference draws it from the
    device RNG, :219).  `early_exit` stops the UNet after the last stored map -- result-identical for
    `run_and_find_attn`, which discards the prediction (ptp_utils.py:246).  `latents` [B,4,h,w]: already encoded
    rows (image2latent's output, e.g. kept from an earlier epoch) -- `image` is then ignored."""
    if latents is not None:
        latent = latents.to(device=device, dtype=torch.float32)
    else:
        if isinstance(image, torch.Tensor) and image.dim() == 3:
            image = image[None]
        latent = image2latent(ldm, image, device)
    if noise is None:
        noise = torch.randn_like(latent)
    t = ldm.scheduler.timesteps[noise_level]
    noisy_image = ldm.scheduler.add_noise(latent, noise, t)
    b = noisy_image.shape[0]
    if early_exit and controllers is not None:
        for c in controllers.values():
            c.stop_after = MAX_STORED_LAYERS
    try:
        _context_kv_begin(ldm.unet, context, early_exit=bool(early_exit and controllers is not None))
        pred_noise = ldm.unet(noisy_image, t.repeat(b), context.expand(b, -1, -1) if context.shape[0] == 1 else context)["sample"]
    except StopForward:
        pred_noise = None
    finally:
        _context_kv_end()
        if early_exit and controllers is not None:
            for c in controllers.values():
                c.stop_after = None
    return noise, pred_noise


def run_and_find_attn(ldm, image, context, noise_level=-1, device="cuda",
                      from_where=["down_cross", "mid_cross", "up_cross"], layers=[0, 1, 2, 3, 4, 5],
                      upsample_res=32, indices=None, controllers=None, noise=None, early_exit=True):
    """ptp_utils.py:234-272: one noised UNet forward, then `collect_maps` per controller."""
    find_pred_noise(ldm, image, context, noise_level=noise_level, device=device, noise=noise,
                    early_exit=early_exit, controllers=controllers)
    attention_maps = []
    for controller in controllers:
        attention_maps.append(collect_maps(controllers[controller], from_where=from_where,
                                           upsample_res=upsample_res, layers=layers, indices=indices))
        controllers[controller].reset()
    return attention_maps


# ---------------------------------------------------------------------------------------------
# image sampling from a learned embedding                reference ptp_utils.py:307-349,420-461
# ---------------------------------------------------------------------------------------------
def _unet_forward_shared_context(model, latents, t, context, records=None):
    """One full UNet forward with the learned embedding as the context of every row (k / v projected once per layer width for
    the shared row, as in `find_pred_noise`).  `records` (a list): receives what the hooks stored during this forward, before the
    store is emptied."""
    b = latents.shape[0]
    try:
        _context_kv_begin(model.unet, context, early_exit=False)
        return model.unet(latents, t, context.expand(b, -1, -1) if context.shape[0] == 1 else context)["sample"]
    finally:
        _context_kv_end()
        hooked = model.unet.__dict__.get("_skp_hook_controller")
        if hooked is not None and hasattr(hooked, "reset"):
            if records is not None:
                records.extend(hooked.step_store["attn"])
            hooked.reset()                           # maps the hooks recorded during this forward belong to no optimisation step


def diffusion_step(model, latents, context, t):
    """ptp_utils.py:307-313: the noise prediction of `model.unet` for `latents` at timestep `t`, every row conditioned on `context`
    ([1, T, D])."""
    t = torch.as_tensor(t)
    return _unet_forward_shared_context(model, latents, t.reshape(-1)[:1].repeat(latents.shape[0]), context)


def latent2image(vae, latents):
    """ptp_utils.py:316-322: latents / 0.18215 -> decode -> (x / 2 + 0.5).clamp(0, 1) -> uint8 numpy [B, H, W, 3].  (On the GPU the
    [0, 1] map is the epilogue of the decoder's last convolution.)"""
    with torch.no_grad():
        image = _latent2float(vae, latents)
    return _image2uint8(image)


def _image2uint8(image):
    """float [B, 3, H, W] in [0, 1] -> uint8 numpy [B, H, W, 3], truncating.  A float32 device image is permuted and converted by
    one kernel (csrc/skp_conv_out.hip), so the copy to the host is bytes; the result is the host expression's, bit for bit."""
    if image.is_cuda and image.dtype == torch.float32:
        routes.note("image.u8", "nhwc_u8")
        return ops.image_u8_nhwc(image).cpu().numpy()
    routes.note("image.u8", "host")
    image = image.cpu().permute(0, 2, 3, 1).numpy()
    return (image * 255).astype(np.uint8)


def _latent2float(vae, latents):
    vae = vae.module if isinstance(vae, torch.nn.DataParallel) else vae
    return vae.decode(1 / 0.18215 * latents, to_image=True)["sample"]


def _in_channels(unet):
    return int(getattr(unet, "in_channels", None) or unet.config["in_channels"])


def init_latent(latent, model, height, width, generator):
    """ptp_utils.py:325-334 -> (latent, latents): `latent` [1, C, height/8, width/8] drawn on the CPU from `generator` when None (the
    draw is the reference's, whatever device the model is on), `latents` = the same on `model.device`."""
    shape = (1, _in_channels(model.unet), height // 8, width // 8)
    if latent is None:
        latent = torch.randn(shape, generator=generator)
    latents = latent.expand(*shape).to(model.device)
    return latent, latents


def init_latents(latent, model, height, width, generators):
    """`init_latent` for n images -> (latent [n, C, height/8, width/8] on the CPU, the same on `model.device`).  `generators` is a list:
    image i is drawn as torch.randn((1, C, h, w), generator=generators[i]) on the CPU -- the reference's draw, so image i of a batch
    starts from the noise the single-image call with that generator starts from.  A given `latent` [n, C, h, w] is used as it is
    (`generators` is then not read)."""
    shape = (1, _in_channels(model.unet), height // 8, width // 8)
    if latent is None:
        if not generators:
            raise ValueError("init_latents: a list of generators (one per image) or a latent [n, C, h, w]")
        latent = torch.cat([torch.randn(shape, generator=g) for g in generators])
    if latent.dim() != 4 or tuple(latent.shape[1:]) != shape[1:]:
        raise ValueError(f"init_latents: latent {tuple(latent.shape)} is not [n, {shape[1]}, {shape[2]}, {shape[3]}]")
    return latent, latent.to(model.device)


def _predict(model, latents, context, t, doubled, records=None):
    """The UNet forward(s) of one sampling step -> (latents [n, C, h, w], pred_c, pred_u).  `context = [uncond, cond]`: `uncond`
    None -- the conditional prediction alone (pred_u None); contexts of equal length -- ONE forward of 2n rows, the unconditional
    rows first (`doubled`: `latents` already holds the n rows twice); otherwise two forwards of n rows.  `records` (a list):
    receives the hooked records of the forward that holds the conditional rows (its last n rows, in the one-forward case); the
    unconditional forward of the two-forward case then runs without autograd."""
    uncond, cond = context
    if uncond is None:
        return latents, _unet_forward_shared_context(model, latents, t, cond, records), None
    if uncond.shape[1] != cond.shape[1]:
        with torch.no_grad() if records is not None else contextlib.nullcontext():
            pred_u = _unet_forward_shared_context(model, latents.detach() if records is not None else latents, t, uncond)
        return latents, _unet_forward_shared_context(model, latents, t, cond, records), pred_u
    n = latents.shape[0] // 2 if doubled else latents.shape[0]
    rows = latents if doubled else torch.cat([latents, latents])
    ctx = torch.cat([uncond.expand(n, -1, -1), cond.expand(n, -1, -1)])
    pred = _unet_forward_shared_context(model, rows, t, ctx, records)
    return rows[:n], pred[n:], pred[:n]


class KeypointTargets(NamedTuple):
    """The checked arguments of keypoint guidance on the device, made once per call (`_keypoint_targets`)."""
    pos: torch.Tensor                        # [n, K, 2] float32 (row, col) in image fractions, on the latents' device
    ids: list                                # the K token ids, host ints
    sel: torch.Tensor                        # the same, int64 [K] on the device
    tokrow: torch.Tensor                     # int32 [T] on the device: the map row of a token, -1 for the others


def _keypoint_ids(keypoints, keypoint_indices, T):
    """Everything about the pair that does not depend on the number of images -> (pos [K, 2] or [m, K, 2] float32 on the host,
    ids: K host ints).  Reads `keypoint_indices` to the host once; ValueError for one without the other, positions that are not K
    (row, col) pairs, an index outside the T tokens or listed twice."""
    if (keypoints is None) != (keypoint_indices is None):
        raise ValueError("keypoints and keypoint_indices go together: K positions for K token ids")
    ids = [int(v) for v in torch.as_tensor(keypoint_indices).reshape(-1).tolist()]
    pos = torch.as_tensor(keypoints).detach().to("cpu", torch.float32)
    if pos.dim() not in (2, 3) or not ids or tuple(pos.shape[-2:]) != (len(ids), 2):
        raise ValueError(f"keypoints {tuple(pos.shape)} must be [K, 2] or [n, K, 2] with K = {len(ids)} token ids")
    if min(ids) < 0 or max(ids) >= T:
        raise ValueError(f"keypoint_indices {ids} reach outside the embedding's {T} tokens")
    if len(set(ids)) != len(ids):
        raise ValueError(f"keypoint_indices {ids} must be distinct")
    return pos, ids


def _keypoint_targets(pos, ids, n, T, device):
    """(pos, ids) of `_keypoint_ids` for n images -> KeypointTargets; ValueError when [m, K, 2] positions are not n rows."""
    if pos.dim() == 2:
        pos = pos[None].expand(n, -1, -1)
    if pos.shape[0] != n:
        raise ValueError(f"keypoints {tuple(pos.shape)}: {pos.shape[0]} rows of targets for {n} images")
    tokrow = torch.full((T,), -1, dtype=torch.int32)
    tokrow[ids] = torch.arange(len(ids), dtype=torch.int32)
    return KeypointTargets(pos.to(device).contiguous(), ids, torch.tensor(ids, dtype=torch.int64).to(device), tokrow.to(device))


TARGET_ENERGIES = ("cosine", "mse")


class MapTargets(NamedTuple):
    """The checked arguments of pose transfer -- keypoint guidance toward target maps -- on the device, made once per call
    (`_map_targets`); the counterpart of `KeypointTargets`."""
    maps: torch.Tensor                       # [n, K, R, R] or [1, K, R, R] (one target for every image), in the latents' dtype
    mode: str                                # "cosine" or "mse"
    ids: list                                # the K token ids, host ints
    sel: torch.Tensor                        # the same, int64 [K] on the device
    tokrow: torch.Tensor                     # int32 [T] on the device: the map row of a token, -1 for the others


def _target_map_ids(target_maps, target_energy, keypoint_indices, T):
    """Everything about target maps that does not depend on the number of images -> (maps [m, K, R', R'] where they are, ids: K
    host ints).  ValueError for maps without token ids, an unknown energy, maps that are not [K, R', R'] or [m, K, R', R'] with
    square R' and K = the number of ids, an index outside the T tokens or listed twice."""
    if target_maps is None or keypoint_indices is None:
        raise ValueError("target_maps and keypoint_indices go together: K target maps for K token ids")
    if target_energy not in TARGET_ENERGIES:
        raise ValueError(f"target_energy must be one of {TARGET_ENERGIES}, got {target_energy!r}")
    ids = [int(v) for v in torch.as_tensor(keypoint_indices).reshape(-1).tolist()]
    maps = torch.as_tensor(target_maps).detach()
    if maps.dim() == 3:
        maps = maps[None]
    if maps.dim() != 4 or not ids or maps.shape[1] != len(ids) or maps.shape[2] != maps.shape[3] or not maps.is_floating_point() \
            or 0 in maps.shape:
        raise ValueError(f"target_maps {tuple(maps.shape)} must be floating [K, R, R] or [n, K, R, R] with K = {len(ids)} token ids")
    if min(ids) < 0 or max(ids) >= T:
        raise ValueError(f"keypoint_indices {ids} reach outside the embedding's {T} tokens")
    if len(set(ids)) != len(ids):
        raise ValueError(f"keypoint_indices {ids} must be distinct")
    return maps, ids


def resample_target_maps(maps, R):
    """Target maps [m, K, R', R'] at the resolution R of the model's stored maps: as they are for R' == R, otherwise ONE library
    call, torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=True) -- plumbing of the sampling call
    (once per call), not a route."""
    if maps.shape[-1] == R and maps.shape[-2] == R:
        return maps
    import torch.nn.functional as F
    return F.interpolate(maps, size=(R, R), mode="bilinear", align_corners=False, antialias=True)


def _map_targets(maps, ids, mode, n, T, R, device, dtype):
    """(maps, ids) of `_target_map_ids` for n images of a model whose maps are R x R -> MapTargets; ValueError when the maps are
    neither one row nor n."""
    if maps.shape[0] not in (1, n):
        raise ValueError(f"target_maps {tuple(maps.shape)}: {maps.shape[0]} rows of targets for {n} images")
    maps = resample_target_maps(maps.to(device=device, dtype=dtype), int(R)).contiguous()
    tokrow = torch.full((T,), -1, dtype=torch.int32)
    tokrow[ids] = torch.arange(len(ids), dtype=torch.int32)
    return MapTargets(maps, mode, ids, torch.tensor(ids, dtype=torch.int64).to(device), tokrow.to(device))


def map_target_energy(M, target, mode):
    """The two energies of include/skp_targets.h in torch ops, in the dtype of M and differentiable by it: M [n, K, R, R], target
    [n, K, R, R] or [1, K, R, R] -> E [n].  "mse": mean_{k,r,c} (M - T)^2.  "cosine": (1/K) sum_k 1/2 sum (M / |M| - T / |T|)^2 =
    (1/K) sum_k (1 - cos(M_k, T_k)), formed from the squared differences; a map or target of zeros counts E_k = 1 and takes no
    gradient."""
    T = target.to(M.dtype).expand_as(M)
    if mode == "mse":
        return ((M - T) ** 2).mean(dim=(1, 2, 3))
    if mode != "cosine":
        raise ValueError(f"target_energy must be one of {TARGET_ENERGIES}, got {mode!r}")
    a, c = (M * M).sum(dim=(2, 3), keepdim=True), (T * T).sum(dim=(2, 3), keepdim=True)
    ok = (a > 0) & (c > 0)
    one = torch.ones_like(a)
    diff = M * torch.where(ok, a, one).rsqrt() - T * torch.where(ok, c, one).rsqrt()
    Ek = torch.where(ok, 0.5 * (diff ** 2).sum(dim=(2, 3), keepdim=True), one)
    return Ek.mean(dim=(1, 2, 3))


def gaussian_target_maps(points, R, sigma, reduce="max"):
    """Target maps from several points per token: points [K, P, 2] ((row, col) in image fractions) -> [K, R, R], every point a
    gaussian of width `sigma` map pixels by `optimize_token.gaussian_circle`'s formula, the P of a token combined by `reduce`
    ("max", "sum" or "mean").  With target_energy="mse" this is keypoint guidance with several points per token; with P = 1 it is
    the point form's target."""
    from .optimize_token import gaussian_circle
    points = torch.as_tensor(points)
    if points.dim() != 3 or points.shape[-1] != 2 or 0 in points.shape or not points.is_floating_point():
        raise ValueError(f"gaussian_target_maps: points {tuple(points.shape)} must be floating [K, P, 2]")
    if reduce not in ("max", "sum", "mean"):
        raise ValueError(f"gaussian_target_maps: reduce must be 'max', 'sum' or 'mean', got {reduce!r}")
    each = torch.stack([gaussian_circle(points[k], size=int(R), sigma=sigma) for k in range(points.shape[0])])      # [K, P, R, R]
    return each.amax(dim=1) if reduce == "max" else each.sum(dim=1) if reduce == "sum" else each.mean(dim=1)


@torch.no_grad()
def pose_targets(model, image, embedding, keypoint_indices, *, noise_level=-1, noise=None, layers=(0, 1, 2, 3)):
    """The target maps of one or several example images -> [m, K, R, R] on the model's device: exactly the quantity the energy of
    `keypoint_energy_grad` reads, the mean over the stored up-block cross layers `layers` and their heads of the up-res softmax
    maps of the K tokens `keypoint_indices` -- of `image` ([3, H, W] or [m, 3, H, W] in [0, 1], or a numpy [m, H, W, 3]) noised to
    `model.scheduler.timesteps[noise_level]` (`noise` [m, C, h, w]: the gaussian, drawn on the device when None) under the
    learned `embedding` [1, T, D].  One noised forward through `find_pred_noise`, `collect_maps_batched(controller, indices=)` on
    the device; no autograd; the hooked store is empty afterwards.  What the reference's generation script loads as
    "example_attn_maps_indices.pt"."""
    hooked = model.unet.__dict__.get("_skp_hook_controller")
    if hooked is None or not hasattr(hooked, "step_store"):
        raise RuntimeError("pose_targets: the UNet carries no attention store (register_attention_control / load_ldm)")
    T = embedding.shape[1]
    ids = [int(v) for v in torch.as_tensor(keypoint_indices).reshape(-1).tolist()]
    if not ids or min(ids) < 0 or max(ids) >= T or len(set(ids)) != len(ids):
        raise ValueError(f"keypoint_indices {ids} must be distinct ids of the embedding's {T} tokens")
    dtype = next(model.unet.parameters()).dtype
    hooked.reset()
    try:
        find_pred_noise(model, image, embedding.to(device=model.device, dtype=dtype), noise_level=noise_level, device=model.device,
                        noise=noise)
        chosen = [r for i, r in enumerate(hooked.step_store["attn"]) if i in layers]
        if not chosen or not all(isinstance(r, FusedAttn) for r in chosen):
            raise RuntimeError("pose_targets: no stored attention layer matches `layers` (or the store materialises its entries)")
        if chosen[0].q.is_cuda and chosen[0].q.dtype == torch.float32:
            from ._maps import collect_maps_batched
            return collect_maps_batched(hooked, layers=layers, indices=torch.tensor(ids))
        n, R, heads = chosen[0].q.shape[0], chosen[0].R, chosen[0].heads
        M = sum(_materialize_host(r.q, r.k, heads, r.scale, R).reshape(n, heads, R * R, -1)[..., ids].mean(dim=1) for r in chosen)
        return (M / len(chosen)).permute(0, 2, 1).reshape(n, len(ids), R, R).contiguous()
    finally:
        hooked.reset()


def keypoint_energy_grad(model, latents, context, t, keypoints, indices, sigma, layers=(0, 1, 2, 3), doubled=False, *,
                         target_maps=None, target_energy="cosine"):
    """Energy of keypoint guidance and its gradient by the latents at one timestep -> (pred_c, pred_u, E [n], g [n, C, h, w]).
    Runs the UNet forward(s) of `_predict` (`context = [uncond or None, cond]`, `doubled` as in `sampler_latent_step`) with autograd
    on, on a detached copy of `latents`; the maps M_i [K, R, R] of image i are the mean over the stored up-block cross layers
    `layers` and their heads of the up-res softmax maps of its CONDITIONAL row, for the tokens `indices` (K ids; what
    `collect_maps_batched(controller, indices=)` returns); E_i = mean (M_i - t_i)^2 against the gaussians of width `sigma` (in map
    pixels) at `keypoints` [K, 2] or [n, K, 2] ((row, col) in image fractions: `optimize_token.gaussian_circle`), the reference's
    `find_gaussian_loss_at_point` with one point per token; g_i = dE_i / dx_i.  The unconditional rows carry no loss; contexts of
    unequal length run the unconditional forward without autograd.  The predictions come back detached, the hooked store empty.
    float32 device tensors take one node, `ops.MapPointLossFn` (fused maps for K rows, the point-loss kernel, the sparse map
    backward), and the HIP backward of the frozen UNet; host tensors and other dtypes the same formulas in torch ops, so the call
    runs on an fp64 copy of the modules on the host.  The model must be hooked (`register_attention_control`, as `load_ldm`
    does).
    Pose transfer (keyword-only): `target_maps` [K, R', R'], [1, K, R', R'] or [n, K, R', R'] with `target_energy` "cosine" or "mse"
    in place of `keypoints` (pass None; `sigma` is unused) -- the energy of the K maps against target MAPS,
    `map_target_energy` / include/skp_targets.h: E_i = mean (M_i - T_i)^2, or (1/K) sum_k (1 - cos(M_ik, T_ik)), which does not
    see the scale of either map.  Targets of another resolution are resampled to R (`resample_target_maps`).  The device node is
    `ops.MapTargetLossFn`, the ledger site `sample.pose`."""
    n = latents.shape[0] // 2 if doubled else latents.shape[0]
    T = context[1].shape[1]
    if target_maps is not None:
        if keypoints is not None:
            raise ValueError("keypoints and target_maps are mutually exclusive")
        R = model.unet.__dict__.get("_skp_hook_res")
        if R is None:
            raise RuntimeError("keypoint_energy_grad: the UNet carries no attention store (register_attention_control / load_ldm)")
        maps, ids = _target_map_ids(target_maps, target_energy, indices, T)
        targets = _map_targets(maps, ids, target_energy, n, T, R, latents.device, latents.dtype)
    else:
        targets = _keypoint_targets(*_keypoint_ids(keypoints, indices, T), n, T, latents.device)
    return _energy_grad(model, latents, context, t, targets, sigma, layers, doubled)


def _energy_grad(model, latents, context, t, targets, sigma, layers=(0, 1, 2, 3), doubled=False):
    """`keypoint_energy_grad` for prepared `KeypointTargets` or `MapTargets` (the sampling loop makes them once, before its first
    step)."""
    hooked = model.unet.__dict__.get("_skp_hook_controller")
    if hooked is None or not hasattr(hooked, "step_store"):
        raise RuntimeError("keypoint_energy_grad: the UNet carries no attention store (register_attention_control / load_ldm)")
    uncond, cond = context
    n = latents.shape[0] // 2 if doubled else latents.shape[0]
    to_maps = isinstance(targets, MapTargets)
    site = "sample.pose" if to_maps else "sample.keypoints"
    ids, sel, tokrow = targets.ids, targets.sel, targets.tokrow
    hooked.reset()
    records = []
    with torch.enable_grad():
        x = latents.detach().requires_grad_()
        _, pred_c, pred_u = _predict(model, x, context, t, doubled, records)
        chosen = [r for i, r in enumerate(records) if i in layers]
        if not chosen or not all(isinstance(r, FusedAttn) for r in chosen):
            raise RuntimeError("keypoint_energy_grad: no stored attention layer matches `layers` (or the store materialises its "
                               "entries: AttentionStore(materialize=True) keeps no autograd history)")
        if x.is_cuda and x.dtype == torch.float32:
            routes.note(site, "map_target_loss" if to_maps else "map_point_loss")
            st = stack_of(chosen, "keypoint_energy_grad", rows=slice(-n, None))   # the conditional rows: the last n of the forward
            if to_maps:
                meta = dict(R=st.R, heads=st.heads, scales=st.scales, target=targets.maps, mode=targets.mode, sel=sel, tokrow=tokrow)
                E = ops.MapTargetLossFn.apply(meta, *st.flat())
            else:
                meta = dict(R=st.R, heads=st.heads, scales=st.scales, sigma=float(sigma), pos=targets.pos, sel=sel, tokrow=tokrow)
                E = ops.MapPointLossFn.apply(meta, *st.flat())
        else:
            routes.note(site, "host")
            R, heads = chosen[0].R, chosen[0].heads
            M = 0
            for r in chosen:
                k = r.k if r.k.shape[0] == 1 else r.k[-n:]
                probs = _materialize_host(r.q[-n:], k, heads, r.scale, R)     # (n * heads, R^2, T)
                M = M + probs.reshape(n, heads, R * R, -1)[..., ids].mean(dim=1)
            M = (M / len(chosen)).permute(0, 2, 1).reshape(n, len(ids), R, R)
            if to_maps:
                if tuple(targets.maps.shape[1:]) != (len(ids), R, R):
                    raise RuntimeError(f"keypoint_energy_grad: target maps {tuple(targets.maps.shape)} for maps {tuple(M.shape)}")
                E = map_target_energy(M, targets.maps, targets.mode)
            else:
                p = targets.pos.to(M.dtype) * R
                ar = torch.arange(R, device=M.device, dtype=M.dtype) + 0.5
                d2 = (ar.view(1, 1, 1, R) - p[..., 1, None, None]) ** 2 + (ar.view(1, 1, R, 1) - p[..., 0, None, None]) ** 2
                E = ((M - torch.exp(-d2 / (2.0 * float(sigma) ** 2))) ** 2).mean(dim=(1, 2, 3))
        g, = torch.autograd.grad(E.sum(), x)
    if doubled:
        g = g[n:]
    return pred_c.detach(), None if pred_u is None else pred_u.detach(), E.detach(), g


def _finish(controller, out, doubled):
    """`controller.step_callback` on the step's result -- on its first copy when `doubled`, duplicated again only if the callback
    returned another tensor."""
    if controller is not None:
        first = out[:out.shape[0] // 2] if doubled else out
        called = controller.step_callback(first)
        if called is not first:
            out = torch.cat([called, called]) if doubled else called
    return out


def guided_latent_step(model, controller, latents, context, t, guidance_scale, *, doubled=False):
    """One sampling step with classifier-free guidance: the branch of ptp_utils.py:337-349 that the reference's `low_resource=False`
    names, as an entry of its own (`latent_step` stays the conditional prediction alone).  `context = [uncond, cond]`, each [1, T, D];
    `latents` [n, C, h, w].
      * equal T: ONE UNet forward of 2n rows, the unconditional rows first, context [2n, T, D] (every layer projects it per row, as
        for any per-row context); the two halves of the output are the unconditional and the conditional prediction;
      * different T (a 77-token unconditional embedding against a 500-token learned one): two forwards of n rows, each with its
        shared context row.
    Both end in one `scheduler.step(cond, t, latents, uncond_output=uncond, guidance_scale=...)` -- on the GPU one kernel that mixes
    the two predictions and applies the update -- followed by `controller.step_callback`, as in `latent_step`.
    `doubled` (equal T only): `latents` is [2n, C, h, w] holding the n rows twice, and so is the result: the step writes its output
    twice, so the loop of `text2image_ldm_stable` concatenates once before its first step and never after (GPU, equal T; the
    host route and contexts of different length concatenate or run two forwards per step).  Works in whatever dtype the module tree and its inputs have."""
    uncond, cond = context
    if doubled and uncond.shape[1] != cond.shape[1]:
        raise ValueError("guided_latent_step: doubled latents need contexts of equal length")
    latents, pred_c, pred_u = _predict(model, latents, context, t, doubled)
    out = model.scheduler.step(pred_c, t, latents, uncond_output=pred_u, guidance_scale=guidance_scale,
                               copies=2 if doubled else 1)["prev_sample"]
    return _finish(controller, out, doubled)


def latent_step(model, controller, latents, context, t, guidance_scale, low_resource=True):
    """ptp_utils.py:337-349: one sampling step.  As in the reference's `low_resource` branch the prediction is the conditional
    one alone -- `context[1]`, the learned embedding; `context[0]` and `guidance_scale` are unused (the reference has the
    guidance line commented out).  The batched two-context branch is not built (classifier-free guidance is out of scope)."""
    if not low_resource:
        raise NotImplementedError("latent_step: only the low_resource branch (conditional prediction alone) is built")
    noise_pred = _unet_forward_shared_context(model, latents, t, context[1])
    return _finish(controller, model.scheduler.step(noise_pred, t, latents)["prev_sample"], False)


def sampler_latent_step(model, controller, latents, context, t, guidance_scale, *, plan, coef, x0_hist, noise=None, doubled=False,
                        preds=None, grad=None, grad_scale=None):
    """One step of a sampler of ldm/samplers.py: the UNet forward(s) of `latent_step` (`context[0]` None: the conditional prediction
    alone) or of `guided_latent_step` (one forward of 2n rows for contexts of equal length, two forwards otherwise; `doubled` as
    there), then the sampler's linear update with the host numbers `coef` (a `samplers.StepCoef` of `plan`, whose prediction type
    and clipping apply) and `controller.step_callback`.  `x0_hist` [n, C, h, w]: the previous step's clamped x0, read when
    `coef.c1 != 0` and overwritten in place with this step's (the multistep solvers only; None for "ddim").  `noise` [n, C, h, w]:
    this step's gaussian, read when `coef.cn != 0`.  float32 device tensors take one kernel, `ops.sampler_step`, that also
    writes the second copy of a doubled result; host tensors and other dtypes evaluate the same formula in torch, in the input
    dtype.  `preds` = (pred_c, pred_u): this step's predictions, already made (`keypoint_energy_grad`) -- no forward runs here;
    `grad` [n, C, h, w] with `grad_scale` [n] (on the latents' device, never read back): the gradient term of keypoint guidance,
    eps += s g and x0 -= (sb / sa) s g before the clamp (`samplers.step_formula`)."""
    uncond, cond = context
    guided = uncond is not None
    if doubled and not (guided and uncond.shape[1] == cond.shape[1]):
        raise ValueError("sampler_latent_step: doubled latents need guidance with contexts of equal length")
    if preds is None:
        latents, pred_c, pred_u = _predict(model, latents, context, t, doubled)
    else:
        latents, (pred_c, pred_u) = latents[:latents.shape[0] // 2] if doubled else latents, preds
    prev = x0_hist if coef.c1 != 0 else None
    nz = noise if coef.cn != 0 else None
    if latents.is_cuda and all(v is None or v.dtype == torch.float32 for v in (latents, pred_c, pred_u, prev, nz, x0_hist, grad,
                                                                               grad_scale)):
        routes.note("sample.step", "sampler_step")
        out = ops.sampler_step(latents, pred_c, pred_u, x0_prev=prev, noise=nz, coef=coef, guidance=float(guidance_scale),
                               prediction=plan.prediction_type, clip=plan.clip_sample, copies=2 if doubled else 1, x0_out=x0_hist,
                               grad=grad, grad_scale=grad_scale)
    else:
        routes.note("sample.step", "host")
        out, x0 = step_formula(latents, pred_c, pred_u, coef, guidance_scale, plan.prediction_type, plan.clip_sample, prev, nz,
                               grad, grad_scale)
        if x0_hist is not None:
            x0_hist.copy_(x0)
        out = torch.cat([out, out]) if doubled else out
    return _finish(controller, out, doubled)


def _step_noise(plan, steps, latent, generator):
    """The gaussians of a stochastic sampler, [steps, n, C, h, w] on the CPU: image i's row of step s is the s-th
    torch.randn((1, C, h, w), generator=generators[i]) after that image's initial latent -- the rule of `init_latents`, so image i
    of a batch sees the noise of the single-image call with its generator."""
    gens = list(generator) if isinstance(generator, (list, tuple)) else [generator]
    if any(g is None for g in gens) or len(gens) != latent.shape[0]:
        raise ValueError(f"sampler {plan.kind!r}" + (f" with eta = {plan.eta}" if plan.kind == "ddim" else "") + " draws noise at "
                         "every step: it needs a generator (one per image), also when `latent` is given")
    shape = (1,) + tuple(latent.shape[1:])
    return torch.stack([torch.cat([torch.randn(shape, generator=g) for g in gens]) for _ in range(steps)])


def _needs_text_encoder(model, what):
    if getattr(model, "tokenizer", None) is None:
        raise RuntimeError(f"{what}: this model was loaded without its text encoder; load it with "
                           "optimize_token.load_ldm(..., text_encoder=True)")


@torch.no_grad()
def encode_prompt(model, prompts):
    """ptp_utils.py:436-439: prompts (a string or a list of n strings) -> the context [n, 77, D] the UNet's cross-attention layers
    take, on the model's device.
      * SD-1.x / SD-2.x: `model.text_encoder(model.tokenizer(prompts, padding="max_length", max_length=77,
        return_tensors="pt").input_ids)[0]`, the reference's call;
      * SDXL: -> (context, pooled): the penultimate hidden states of the two towers side by side (768 + 1280 = 2048 channels) and the
        second tower's pooled projection [n, 1280].  Feeding that pooled vector into sampling as `text_embeds` is OUT OF SCOPE:
        `text2image_ldm_stable` keeps `default_added_cond`'s zeros, as it does for a learned embedding.
    Padding is the tokenizer's pad id and there is no padding mask (how the Stable Diffusion pipelines call the towers).  The
    model must have been loaded with `load_ldm(..., text_encoder=True)`."""
    _needs_text_encoder(model, "encode_prompt")
    prompts = [prompts] if isinstance(prompts, str) else list(prompts)

    def ids(tok):
        return tok(prompts, padding="max_length", max_length=tok.model_max_length, return_tensors="pt").input_ids.to(model.device)
    if getattr(model, "text_encoder_2", None) is None:
        return model.text_encoder(ids(model.tokenizer))[0]
    first = model.text_encoder(ids(model.tokenizer), penultimate=True)[0]
    second, pooled = model.text_encoder_2(ids(model.tokenizer_2), penultimate=True)
    return torch.cat([first, second], dim=-1), pooled


@contextlib.contextmanager
def _reproducible_library_convolutions():
    """Inside the block the library convolutions that the sampling path still reaches (few-tile layers, `conv3x3` / `lib`) may
    only use solvers that sum in a fixed order: a single-row 8^2 / 1^2 layer is otherwise split over its input channels with
    atomic adds, and two calls with the same latent differ in the last bits.  The project's own kernels have no atomics on this
    path.  This is a change of the existing default call too: its library convolutions may run on other solvers than before, so
    its image can differ from earlier versions' in the last bits (and is the same from call to call).  The flag is process-wide
    and the caller's again afterwards; like the scheduler's timestep table, which this call also borrows, it is not safe against
    another thread running library convolutions or sampling on the same process at the same time."""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = prev


# ---------------------------------------------------------------------------------------------
# the captured sampling loop: one recorded step, replayed            text2image_ldm_stable(capture=True)
# ---------------------------------------------------------------------------------------------
GRAPH_WARMUP_STEPS = 2         # steps of a captured call that run on eager launches first
GRAPH_MIN_ROWS = 64            # per-step buffers (table, sinusoids, noise, trace) hold at least this many steps


def sample_graph_key(*, rows, doubled, two_forward, tokens, latent_shape, prediction, clip, kind, history, noise, keypoints,
                     layers, extra=(), tag=()):
    """Everything shape-like or compiled into a recorded sampling step, as one hashable value: image rows, whether the UNet input
    is kept doubled, whether guidance takes two forwards, the token counts (conditional, unconditional or None), the latent
    shape [C, h, w], the prediction type, the clamp, the kind of plan ("axpby" / "ddim_step": the call without a sampler;
    otherwise the sampler's name), whether an x0 history and per-step noise exist, K of the keypoints (0: none), the stored
    layers the energy reads, `extra` (the energy's sigma and normalisation, which are arguments of recorded launches; with
    target maps ("maps", the energy mode, R, the rows of targets -- 1 or n --, the normalisation) instead) and, last, `tag`: `ops.frozen_tag` over the UNet's parameters, so a weight changed in place is another key."""
    return (int(rows), bool(doubled), bool(two_forward), tuple(None if t is None else int(t) for t in tokens),
            tuple(int(v) for v in latent_shape), str(prediction), bool(clip), str(kind), bool(history), bool(noise), int(keypoints),
            tuple(int(v) for v in layers), tuple(extra), tuple(tag))


class SampleGraphs:
    """The recorded sampling steps of one model, kept on it (`sample_graphs(model)`): `sample_graph_key` -> the recorded step with
    its static buffers, or "eager" for a key whose recording failed.  A key that differs from a new one in its tag alone (the
    weights changed) or whose buffers are too short for the call's steps is dropped when the new one is recorded.  `hits` /
    `misses` count the calls that found / had to record their step; `last` is "hit", "miss" or "eager" for the latest captured
    call and `last_key` its key.  `clear()` frees the graphs with their private memory pools and buffers."""

    def __init__(self):
        self.entries, self.hits, self.misses, self.last, self.last_key = {}, 0, 0, None, None

    def clear(self):
        self.entries.clear()
        self.last = self.last_key = None

    def keys(self):
        return list(self.entries)


def sample_graphs(model) -> SampleGraphs:
    return model.__dict__.setdefault("_skp_sample_graphs", SampleGraphs())


class _RecordedStep:
    """Static buffers of one key and the graphs recorded over them: "plain" (the forward(s) of `_predict`, the device-row step
    kernel, the counter's increment) and, with keypoints, "kp" (`_energy_grad`'s forward and backward in front of the same)."""

    def __init__(self, model, key, latents, context, x0_hist, noise, targets, steps, kind, prediction, clip, sigma, normalize,
                 layers):
        dev, n = latents.device, key[0]
        self.model, self.rows, self.doubled = model, n, key[1]
        self.kind, self.prediction, self.clip, self.sigma, self.normalize, self.layers = kind, prediction, clip, sigma, normalize, layers
        self.cap = cap = max(int(steps), GRAPH_MIN_ROWS)
        f32 = dict(device=dev, dtype=torch.float32)
        self.lat = torch.empty_like(latents)
        self.uncond = None if context[0] is None else torch.empty_like(context[0])
        self.cond = torch.empty_like(context[1])
        self.table = torch.zeros(cap, ops.STEP_ROW, **f32)
        self.tsin = torch.zeros(cap, int(model.unet._t_dim), **f32)
        self.counter = torch.zeros(1, device=dev, dtype=torch.int32)
        first = latents[:n]
        self.hist = None if x0_hist is None else torch.empty_like(first)
        self.noise = None if noise is None else torch.zeros((cap,) + tuple(first.shape), **f32)
        self.targets = self.kscale = self.trace = None
        if targets is not None:
            if isinstance(targets, MapTargets):
                self.targets = MapTargets(torch.empty_like(targets.maps), targets.mode, list(targets.ids),
                                          torch.empty_like(targets.sel), torch.empty_like(targets.tokrow))
            else:
                self.targets = KeypointTargets(torch.empty_like(targets.pos), list(targets.ids), torch.empty_like(targets.sel),
                                               torch.empty_like(targets.tokrow))
            self.kscale = torch.zeros(cap, **f32)
            self.trace = torch.zeros(cap, n, **f32)
        self.graphs = {}                                         # "plain" / "kp" -> (graph, held values, route notes of one replay)

    def stage(self, latents, context, table, timesteps, noise, x0_hist, targets, kscale, at):
        """This call's values into the static buffers, and the counter to step `at`.  Everything a replay reads is here afterwards."""
        steps = table.shape[0]
        self.lat.copy_(latents)
        if self.uncond is not None:
            self.uncond.copy_(context[0])
        self.cond.copy_(context[1])
        self.table[:steps].copy_(table)
        # timestep_embedding is elementwise: row i has the bits of the eager call at step i
        from .ldm.unet import timestep_embedding
        self.tsin[:steps].copy_(timestep_embedding(timesteps.reshape(-1).to(self.lat.device), self.tsin.shape[1]))
        self.counter.fill_(int(at))
        if self.noise is not None:
            self.noise[:steps].copy_(noise)
        if self.hist is not None:
            self.hist.copy_(x0_hist)
        if self.targets is not None:
            if isinstance(targets, MapTargets):
                self.targets.maps.copy_(targets.maps)
            else:
                self.targets.pos.copy_(targets.pos)
            self.targets.sel.copy_(targets.sel)
            self.targets.tokrow.copy_(targets.tokrow)
            self.targets.ids[:] = targets.ids
            self.kscale[:steps].copy_(kscale)

    @contextlib.contextmanager
    def _time_rows(self):
        """Inside the block the UNet's time path is the recorded one: the sinusoid row of the step the device counter names, from
        the per-call table, through the `time_embedding` MLP (and SDXL's micro-conditioning) as `UNet2DConditionModel.time_path`
        runs them -- `timestep` is not looked at.  The two Linear layers are plumbing, not a route."""
        unet = self.model.unet
        had = "time_path" in unet.__dict__
        prev = unet.__dict__.get("time_path")

        def time_path(sample, timestep, added_cond_kwargs=None):
            row = self.tsin.index_select(0, self.counter)
            temb = unet.time_embedding(row.expand(sample.shape[0], -1).contiguous().to(sample.dtype))
            if unet.add_embedding is not None:
                from .ldm.unet import timestep_embedding
                cond = added_cond_kwargs if added_cond_kwargs is not None else unet.default_added_cond(sample)
                ids = cond["time_ids"]
                tids = timestep_embedding(ids.reshape(-1), unet._add_t_dim).reshape(ids.shape[0], -1)
                temb = temb + unet.add_embedding(torch.cat([cond["text_embeds"], tids.to(sample.dtype)], dim=-1))
            return temb
        unet.__dict__["time_path"] = time_path
        try:
            yield
        finally:
            if had:
                unet.__dict__["time_path"] = prev
            else:
                del unet.__dict__["time_path"]

    def _step(self, latents, pred_c, pred_u, **kp):
        """The device-row step kernel of this key's plan, writing the next UNet input (both copies of a doubled one) in place."""
        row = dict(table=self.table, step=self.counter, steps=self.cap)
        copies = 2 if self.doubled else 1
        if self.kind == "axpby":
            return ops.axpby_dev(latents, pred_c, out=self.lat, **row)
        if self.kind == "ddim_step":
            return ops.ddim_step_dev(latents, pred_c, pred_u, prediction=self.prediction, clip=self.clip, copies=copies,
                                     out=self.lat, **row)
        routes.note("sample.step", "sampler_step")
        return ops.sampler_step_dev(latents, pred_c, pred_u, x0_prev=self.hist, noise=self.noise, prediction=self.prediction,
                                    clip=self.clip, copies=copies, out=self.lat, x0_out=self.hist, **row, **kp)

    def body(self, which):
        """One step on the static buffers, nothing from the host: what is recorded, and what runs once on eager launches before."""
        context = [self.uncond, self.cond]
        with self._time_rows():
            if which == "kp":
                pred_c, pred_u, energy, g = _energy_grad(self.model, self.lat, context, None, self.targets, self.sigma, self.layers,
                                                         doubled=self.doubled)
                s = self.kscale.index_select(0, self.counter).expand(self.rows)
                if self.normalize:
                    s = s / g.pow(2).mean(dim=(1, 2, 3)).sqrt().clamp_min(1e-12)
                self.trace.index_copy_(0, self.counter.to(torch.int64), energy[None])
                self._step(self.lat[:self.rows] if self.doubled else self.lat, pred_c, pred_u, grad=g, grad_scale=s)
            else:
                latents, pred_c, pred_u = _predict(self.model, self.lat, context, None, self.doubled)
                self._step(latents, pred_c, pred_u)
        ops.step_advance(self.counter)

    def record(self, which):
        """Run the step once on eager launches (the caches of the frozen weights and the library's choices are then those of
        exactly this body) with the buffers put back afterwards, then record it.  Neither run's route notes stay in the ledger:
        they come back once per replay."""
        kept = [(t, t.clone()) for t in (self.lat, self.hist, self.trace, self.counter) if t is not None]
        before = routes.snapshot()
        try:
            self.body(which)
        finally:
            routes.merge(routes.delta(before), -1)
        for t, saved in kept:
            t.copy_(saved)
        graph = torch.cuda.CUDAGraph()
        before = routes.snapshot()
        try:
            with ops.recording() as held, torch.cuda.graph(graph):
                self.body(which)
        finally:
            noted = routes.delta(before)
            routes.merge(noted, -1)
        self.graphs[which] = (graph, held, noted)

    def replay(self, which):
        graph, _, noted = self.graphs[which]
        graph.replay()
        routes.merge(noted)


def _overrides_step_callback(controller) -> bool:
    return controller is not None and getattr(type(controller), "step_callback", None) is not AttentionControl.step_callback


def _default_rows(sched, ts, kind):
    """The rows of the call without a sampler, from `DDIMScheduler._coefficients` (the timestep table of the call must be set):
    "axpby" -- cx = pa / sa and ce = pb - pa sb / sa, the two numbers `DDIMScheduler.step` hands `ops.axpby`, formed the same way;
    "ddim_step" -- c0 = pa and ce = pb."""
    from .ldm.samplers import StepCoef
    rows = []
    for t in ts:
        sa, sb, pa, pb = sched._coefficients(t)
        rows.append(StepCoef(sa, sb, pa / sa, pa, pb - pa * sb / sa, 0.0, 0.0) if kind == "axpby" else
                    StepCoef(sa, sb, 0.0, pa, pb, 0.0, 0.0))
    return rows


def _captured_steps(model, controller, latents, context, ts, at, guidance_scale, plan, coefs, x0_hist, noise, targets, kp, doubled):
    """Steps `at` .. of the loop of `text2image_ldm_stable(capture=True)` as replays of a recorded step -> the latents after the
    last step (laid out like `latents`), or None where the call has to go on with eager launches: a controller with its own
    `step_callback`, the clamped default step (torch ops on host numbers), weights that take gradients, a key marked eager, or a
    recording that failed just now (one warning, the key marked eager, never retried).  Notes `sample.loop` / `graph` per replay."""
    import warnings
    from .ldm.samplers import pack_step_table
    cache, sched, steps = sample_graphs(model), model.scheduler, len(ts)
    guided = context[0] is not None
    n = latents.shape[0] // 2 if doubled else latents.shape[0]
    if _overrides_step_callback(controller):
        warnings.warn("text2image_ldm_stable(capture=True): the controller overrides step_callback, which runs on the host after "
                      "every step; the call stays on eager launches")
        return None
    if plan is None:
        prediction, clip = sched.prediction_type, bool(sched.clip_sample)
        kind = "axpby" if prediction == "epsilon" and not guided else "ddim_step"
        if kind == "axpby" and clip:
            warnings.warn("text2image_ldm_stable(capture=True): the clamped default step is torch arithmetic on host numbers; the "
                          "call stays on eager launches")
            return None
        coefs = _default_rows(sched, ts, kind)
    else:
        prediction, clip, kind = plan.prediction_type, bool(plan.clip_sample), plan.kind
    tag = ops.frozen_tag(list(model.unet.parameters()))
    if tag is None:
        warnings.warn("text2image_ldm_stable(capture=True): the UNet has parameters that take gradients; the call stays on eager "
                      "launches")
        return None
    layers, extra, needs = (0, 1, 2, 3), (), ["plain"] * steps
    if targets is not None:
        lo, hi, kscale, sigma, normalize, trace = kp
        if isinstance(targets, MapTargets):                      # the kind of target, the energy's kernels, the static buffer's shape
            sigma, extra = 0.0, ("maps", targets.mode, int(targets.maps.shape[-1]), int(targets.maps.shape[0]), bool(normalize))
        else:
            extra = (float(sigma), bool(normalize))
        needs = ["kp" if lo <= i / steps < hi else "plain" for i in range(steps)]
    key = sample_graph_key(rows=n, doubled=doubled, two_forward=guided and not doubled,
                           tokens=(context[1].shape[1], context[0].shape[1] if guided else None), latent_shape=latents.shape[1:],
                           prediction=prediction, clip=clip, kind=kind, history=x0_hist is not None, noise=noise is not None,
                           keypoints=0 if targets is None else len(targets.ids), layers=layers, extra=extra, tag=tag)
    hit, cache.last_key = cache.entries.get(key), key
    if hit == "eager":
        cache.last = "eager"
        return None
    if hit is None or hit.cap < steps:
        for k in [k for k in cache.entries if k[:-1] == key[:-1]]:
            del cache.entries[k]                                 # changed weights or a longer table: the graph and what it holds retire
        hit = None
    try:
        step = hit if hit is not None else _RecordedStep(model, key, latents, context, x0_hist, noise, targets, steps, kind,
                                                            prediction, clip, float(sigma) if extra else 0.0,
                                                            bool(normalize) if extra else False, layers)
        ks = None if targets is None else torch.tensor([float(kscale) * c.sb for c in coefs], dtype=torch.float64).to(torch.float32)
        step.stage(latents, context, pack_step_table(coefs, guidance_scale), torch.as_tensor(ts), noise, x0_hist, targets, ks, at)
        missing = [w for w in sorted(set(needs[at:])) if w not in step.graphs]
        for which in missing:
            step.record(which)
    except Exception as e:                                       # noqa: BLE001 -- capture is an optimisation of the host side only
        warnings.warn(f"text2image_ldm_stable(capture=True): the call stays on eager launches (recording the step failed: {e})")
        hooked = model.unet.__dict__.get("_skp_hook_controller")
        if hooked is not None and hasattr(hooked, "reset"):
            hooked.reset()
        cache.entries[key], cache.last = "eager", "eager"
        return None
    cache.entries[key] = step
    if missing:
        cache.misses, cache.last = cache.misses + 1, "miss"
    else:
        cache.hits, cache.last = cache.hits + 1, "hit"
    for i in range(at, steps):                                   # back to back: no copy, no read-back, no synchronisation
        step.replay(needs[i])
        routes.note("sample.loop", "graph")
        if controller is not None:
            controller.reset()
    if targets is not None and trace is not None:
        rows = step.trace[:steps].clone()
        trace.extend(rows[i] for i in range(at, steps) if needs[i] == "kp")
    return step.lat.clone()


@torch.no_grad()
def text2image_ldm_stable(model, embedding, controller, num_inference_steps: int = 50, guidance_scale: float = 7.5,
                          generator: Optional[torch.Generator] = None, latent: Optional[torch.Tensor] = None, *,
                          height: int = 512, width: int = 512, output_type: str = "uint8",
                          uncond_embedding: Optional[torch.Tensor] = None, uncond_prompt: Optional[str] = None,
                          sampler: Optional[str] = None, eta: float = 0.0, keypoints=None, keypoint_indices=None,
                          keypoint_scale: float = 2.0, keypoint_sigma: float = 2.0, keypoint_steps=(0.0, 1.0),
                          keypoint_normalize: bool = True, keypoint_trace: Optional[list] = None, capture: bool = False,
                          target_maps=None, target_energy: str = "cosine"):
    """ptp_utils.py:420-461: sample an image from the learned `embedding` [1, T, D] by `num_inference_steps` steps of `sampler`
    (deterministic DDIM by default) and decode it -> (image, latent).  `image`: uint8 numpy [1, height, width, 3] (`output_type="uint8"`) or the float32
    tensor [1, 3, height, width] in [0, 1] on the model's device before the 8-bit rounding (`"float"`); `latent`: the initial
    noise [1, C, height/8, width/8] on the CPU (given, or drawn from `generator` on the CPU as the reference draws it).

    Batches: `generator` may be a list of n generators and `latent` may be [n, C, h, w]; all n images then go through every UNet
    forward and the decoder together, `image` and `latent` have n rows, and image i starts from the noise the single-image call
    with `generator[i]` starts from (`init_latents`).

    `uncond_embedding` None (the default): like the reference's `low_resource=True` branch only the learned embedding conditions
    the UNet -- no unconditional pass, no text encoder, `guidance_scale` unused.  `uncond_embedding` [1, T', D] (keyword-only
    extension): classifier-free guidance of strength `guidance_scale` against it, `guided_latent_step`; T' may differ from T.
    `uncond_prompt` (keyword-only extension, a string; "" is CLIP("")): the same with `encode_prompt(model, [uncond_prompt])` as the
    unconditional embedding -- the reference's own unconditional input, and a negative prompt.  Not together with
    `uncond_embedding`; the model must have been loaded with its text encoder (`load_ldm(..., text_encoder=True)`).
    What the UNet predicts (epsilon, v, sample) is the scheduler's `prediction_type` (`load_ldm(..., prediction_type=)`).
    `sampler` (keyword-only extension; ldm/samplers.py): None -- the deterministic DDIM step of `model.scheduler`, the call as it
    always was; "ddim" with `eta` in [0, 1] (eta = 0 is routed to that same step: the same bits as None); "dpm++2m"
    (DPM-Solver++ 2M, second-order multistep: the usual choice at about 20 steps); "dpm++2m-sde".  All walk the timestep table
    of `set_timesteps`; `eta` belongs to "ddim": a nonzero `eta` without a sampler or with another one raises ValueError.  A named sampler runs the same loop -- guided, doubled, batched or not
    -- on one fused kernel per step (`sampler_latent_step`, ledger site `sample.step`), its fp64 host coefficients taken from a
    plan that reads `model.scheduler` and leaves it as it is; the multistep solvers keep the previous step's x0 in one
    [n, C, h, w] buffer, updated in place.  The stochastic ones ("ddim" with eta > 0, "dpm++2m-sde") draw their noise on the CPU
    before the loop, image i's from `generator[i]` after its initial latent, one torch.randn((1, C, h, w)) per step -- image i
    of a batch sees the noise of the single-image call with that generator -- and upload it once as [steps, n, C, h, w]; they
    need a generator also when `latent` is given (ValueError otherwise).
    Keypoint guidance (keyword-only extension): `keypoints` [K, 2] (the same targets for every image) or [n, K, 2], (row, col) in
    image fractions (positions outside [0, 1] are legal), with `keypoint_indices`, K distinct token ids of the embedding -- the
    tensor `find_best_indices` returns, the reference's "outputs/indices.pt" -- samples an image whose learned keypoints sit where the
    caller puts them: what the reference's generation script was meant to do with the two files it loads
    ("example_attn_maps_indices.pt", "outputs/indices.pt") and then never uses.  At every step i of N with lo <= i / N < hi
    (`keypoint_steps` = (lo, hi)) `keypoint_energy_grad` gives E_i = mean (M_i - t_i)^2 -- M_i the K up-res cross-attention maps of
    image i's conditional row at this step, t_i gaussians of width `keypoint_sigma` map pixels at the targets -- and
    g_i = dE_i / dx_i by one backward through the frozen UNet; the step then shifts eps by s_i g_i and x0 by -(sb / sa) s_i g_i
    before the clamp and the sampler's update, with s_i = keypoint_scale sb_t / max(rms(g_i), 1e-12) (`keypoint_normalize`, the rms over
    C h w) or keypoint_scale sb_t.  The scales stay on the device; nothing in the loop is read back.  `keypoint_trace`: a list
    that receives each guided step's E [n] (a device tensor).  With keypoints the loop always runs `sampler_latent_step`
    (`sampler=None` takes the "ddim" eta = 0 plan there) -- guided, doubled, batched or not, for every sampler and prediction type;
    a guided step costs about one optimisation step's forward and backward for n rows on top.  The default scale of 2 was only
    tried on the seeded reduced-width tree of the tests, never on trained weights.  ValueError: one of the two without the other,
    a shape mismatch, an index outside the embedding (or twice).  Without `keypoints` nothing changes: the same routes, the same
    bits.
    Pose transfer (keyword-only extension): `target_maps` [K, R', R'], [1, K, R', R'] (the same targets for every image) or
    [n, K, R', R'] with `keypoint_indices`, in place of `keypoints` (ValueError if both are given), guides toward target MAPS --
    those of an example image from `pose_targets`, "sample an image in the pose of this photo", or several points per token
    from `gaussian_target_maps` -- instead of one gaussian per token: the other file the reference's script loads and never
    uses.  `target_energy`: "cosine" (the default) -- E_i = (1/K) sum_k (1 - cos(M_ik, T_ik)), blind to the scale of either map,
    which the example's maps and the sample's, taken at different noise levels, need not share; a map of zeros counts 1 -- or
    "mse" -- E_i = mean (M_i - T_i)^2, the reference's `find_gaussian_loss_at_point` with the target handed in
    (include/skp_targets.h, `map_target_energy`).  Targets of another resolution are resampled to the model's R once per call
    (`resample_target_maps`: one library call, plumbing).  `keypoint_scale`, `keypoint_steps`, `keypoint_normalize`,
    `keypoint_trace` and the step-kernel term mean what they mean above; `keypoint_sigma` is unused.  Like it, the default scale
    was only tried on the seeded reduced-width tree of the tests, for either energy.  ValueError, before anything is drawn from a
    generator: maps without indices, a wrong K, rows that are neither 1 nor n, maps that are not square, an unknown energy.
    Ledger site `sample.pose`.  Without `target_maps` nothing changes.
    `capture=True` (keyword-only extension; off by default, and then every route, bit and ledger note is what it was): on a float32
    GPU model the first two steps run as always, then ONE step is recorded as a graph over static buffers and replayed for every
    remaining step with no host work in between -- the per-step scalars, the timestep's sinusoid row, the noise row and the
    keypoint scale are read from device tables by a device counter (include/skp_sampler_graph.h, `ops.sampler_step_dev`), so the
    replays compute what the eager launches compute, bit for bit.  With keypoints the guided step is a second graph over the same
    buffers and the host picks one per step; target maps ride in a static buffer like the positions, and their kind, energy,
    R and row count are part of the key (other target VALUES replay the same graph).  Graphs and buffers are kept on the model (`sample_graphs(model)`, with `clear()`),
    keyed by `sample_graph_key` and the frozen tag of the UNet's weights; a later call with the same key refreshes the buffers and
    replays.  Calls of fewer than three steps, a controller with its own `step_callback` (one warning), the clamped default step
    and a key whose recording failed (one warning, never retried) stay on eager launches; host tensors take the host route.
    The ledger site `sample.loop` says per step which it was: "graph", "eager" or "host".  NOT reproduced: `register_attention_control_generation`, which re-installs the
    attention math the module tree already computes.  `height`,
    `width` and `output_type` are keyword-only extensions (the reference fixes 512 x 512).  The scheduler's timestep table is
    restored afterwards, so a sampling call between optimisation steps does not move their noise level.  The model must have
    been loaded with its VAE decoder (`load_ldm(..., decoder=True)`)."""
    if output_type not in ("uint8", "float"):
        raise ValueError(f"output_type must be 'uint8' or 'float', got {output_type!r}")
    vae = model.vae.module if isinstance(model.vae, torch.nn.DataParallel) else model.vae
    if not getattr(vae, "has_decoder", False):
        raise RuntimeError("text2image_ldm_stable: this model was loaded without the VAE decoder; load it with "
                           "optimize_token.load_ldm(..., decoder=True)")
    if height % 8 or width % 8:
        raise ValueError("height and width must be multiples of 8")
    plan = None
    if sampler is None and eta != 0:
        raise ValueError(f"eta = {eta!r} needs sampler=\"ddim\": without a sampler the call is the deterministic DDIM step")
    if sampler is not None:
        plan = SamplerPlan(model.scheduler, sampler, eta)          # an unknown name or eta outside [0, 1]: ValueError
        if plan.kind == "ddim" and plan.eta == 0:
            plan = None                                            # the step the call always had
    if plan is not None and plan.stochastic and generator is None:
        raise ValueError(f"sampler {sampler!r}" + (f" with eta = {eta}" if sampler == "ddim" else "") + " draws noise at every "
                         "step: it needs a generator (one per image), also when `latent` is given")
    if uncond_prompt is not None:
        if uncond_embedding is not None:
            raise ValueError("text2image_ldm_stable: uncond_prompt and uncond_embedding are mutually exclusive")
        if not isinstance(uncond_prompt, str):
            raise ValueError("uncond_prompt must be one string")
        _needs_text_encoder(model, "text2image_ldm_stable(uncond_prompt=...)")
        uncond_embedding = encode_prompt(model, [uncond_prompt])
        if isinstance(uncond_embedding, tuple):                    # SDXL: (context, pooled); the pooled vector is not fed to sampling
            uncond_embedding = uncond_embedding[0]
    targets = None
    if target_maps is not None:                                         # (checked before anything is drawn from a generator)
        if keypoints is not None:
            raise ValueError("text2image_ldm_stable: keypoints and target_maps are mutually exclusive")
        targets = _target_map_ids(target_maps, target_energy, keypoint_indices, embedding.shape[1])
        rows = len(generator) if isinstance(generator, (list, tuple)) else \
            latent.shape[0] if latent is not None and latent.dim() == 4 else 1
        if targets[0].shape[0] not in (1, rows):
            raise ValueError(f"target_maps {tuple(targets[0].shape)}: {targets[0].shape[0]} rows of targets for {rows} images")
        map_res = model.unet.__dict__.get("_skp_hook_res")
        if map_res is None:
            raise RuntimeError("text2image_ldm_stable(target_maps=...): the UNet carries no attention store "
                               "(register_attention_control / load_ldm)")
        lo, hi = (float(v) for v in keypoint_steps)
    elif keypoints is not None or keypoint_indices is not None:
        targets = _keypoint_ids(keypoints, keypoint_indices, embedding.shape[1])
        lo, hi = (float(v) for v in keypoint_steps)
    if isinstance(generator, (list, tuple)) or (latent is not None and latent.dim() == 4 and latent.shape[0] != 1):
        if isinstance(generator, (list, tuple)) and latent is not None and len(generator) != latent.shape[0]:
            raise ValueError(f"{len(generator)} generators for a latent of {latent.shape[0]} rows (a given latent is used as it is; "
                             "pass generator=None with it, or one generator per row)")
        latent, latents = init_latents(latent, model, height, width, generator)
    else:
        latent, latents = init_latent(latent, model, height, width, generator)
    latents = latents.to(torch.float32).contiguous()
    n = latents.shape[0]
    embedding = embedding.to(device=model.device, dtype=torch.float32)
    guided = uncond_embedding is not None
    if guided:
        uncond = uncond_embedding.to(device=model.device, dtype=torch.float32)
        uncond = uncond[None] if uncond.dim() == 2 else uncond
        if uncond.dim() != 3 or uncond.shape[0] != 1 or uncond.shape[-1] != embedding.shape[-1]:
            raise ValueError(f"uncond_embedding {tuple(uncond_embedding.shape)} must be [1, T, {embedding.shape[-1]}]")
    context = [uncond if guided else None, embedding]
    if targets is not None:
        if target_maps is not None:
            targets = _map_targets(*targets, target_energy, n, embedding.shape[1], map_res, latents.device, latents.dtype)
        else:
            targets = _keypoint_targets(*targets, n, embedding.shape[1], latents.device)
        if plan is None:
            plan = SamplerPlan(model.scheduler, "ddim", 0.0)       # the guided step is a term of the sampler kernel
    # on the GPU a guided step with contexts of equal length keeps the 2n-row UNet input between steps (written by the step kernel)
    doubled = guided and latents.is_cuda and uncond.shape[1] == embedding.shape[1]
    if doubled:
        latents = torch.cat([latents, latents])
    sched = model.scheduler
    kept = (sched.timesteps, sched.num_inference_steps)
    if plan is not None:
        timesteps, coefs = plan.plan(num_inference_steps)
        first = latents[:n]
        x0_hist = None if plan.kind == "ddim" else torch.empty_like(first)
        noise = _step_noise(plan, len(coefs), first, generator).to(first) if plan.stochastic else None     # one upload

    def eager_step(i, t, latents):
        """Step i on eager launches (or host tensors): the loop body the call always had."""
        if plan is not None:
            kp = {}
            if targets is not None and lo <= i / len(coefs) < hi:
                pred_c, pred_u, energy, g = _energy_grad(model, latents, context, t, targets, keypoint_sigma, doubled=doubled)
                s = torch.full_like(energy, float(keypoint_scale) * coefs[i].sb)
                if keypoint_normalize:
                    s = s / g.pow(2).mean(dim=(1, 2, 3)).sqrt().clamp_min(1e-12)
                if keypoint_trace is not None:
                    keypoint_trace.append(energy)
                kp = dict(preds=(pred_c, pred_u), grad=g, grad_scale=s)
            latents = sampler_latent_step(model, controller, latents, context, t, guidance_scale, plan=plan, coef=coefs[i],
                                          x0_hist=x0_hist, noise=None if noise is None else noise[i], doubled=doubled, **kp)
        elif guided:
            latents = guided_latent_step(model, controller, latents, context, t, guidance_scale, doubled=doubled)
        else:
            latents = latent_step(model, controller, latents, context, t, guidance_scale, low_resource=True)
        if controller is not None:
            controller.reset()
        return latents

    with _reproducible_library_convolutions():                 # the loop and the decode: one call, one result, bit for bit
        try:
            if plan is None:
                sched.set_timesteps(num_inference_steps)         # (a plan has its own table and leaves the scheduler alone)
            ts = sched.timesteps if plan is None else timesteps
            # capture: None (the call as it always was: nothing noted at `sample.loop`), or the route of every step that is not a replay
            loop_route = None
            if capture:
                on_gpu = latents.is_cuda and all(p.is_cuda and p.dtype == torch.float32 for p in model.unet.parameters())
                loop_route = "eager" if on_gpu else "host"
            with ops.up2_in_unet(latents.is_cuda):
                wants_graph = loop_route == "eager" and len(ts) > GRAPH_WARMUP_STEPS
                for i, t in enumerate(ts):
                    if wants_graph and i == GRAPH_WARMUP_STEPS:
                        done = _captured_steps(model, controller, latents, context, ts, i, guidance_scale, plan,
                                               None if plan is None else coefs, x0_hist if plan is not None else None,
                                               noise if plan is not None else None, targets,
                                               (lo, hi, keypoint_scale, keypoint_sigma, keypoint_normalize, keypoint_trace)
                                               if targets is not None else None, doubled)
                        if done is not None:
                            latents = done
                            break
                        wants_graph = False
                    latents = eager_step(i, t, latents)
                    if loop_route is not None:
                        routes.note("sample.loop", loop_route)
        finally:
            sched.timesteps, sched.num_inference_steps = kept
        if doubled:
            latents = latents[:n]
        if output_type == "float":
            return _latent2float(vae, latents), latent
        return latent2image(vae, latents), latent


# ---------------------------------------------------------------------------------------------
# token selection                                              reference ptp_utils.py:86-159
# ---------------------------------------------------------------------------------------------
def _ranked(score, argmax, R, top_k):
    """First `top_k` token ids by ascending score (ties by index, NaN last -- torch.argsort's order): the selection
    kernel's ranking stage; candidate lists longer than the kernel's 64 slots are a stable device sort."""
    n = score.shape[0]
    top_k = min(int(top_k), n)
    if 2 <= top_k <= ops.SELECT_MAX_CANDIDATES and n <= ops.SELECT_MAX_TOKENS:
        routes.note("select.rank", "select_kernel")
        cand, _ = ops.select_tokens(score, argmax, R, top_k, 2)
        return cand
    routes.note("select.rank", "sort")
    return torch.sort(score, stable=True).indices[:top_k]


def find_top_k_gaussian(attention_maps, top_k, sigma=3, epsilon=1e-5, num_subjects=1):
    """ptp_utils.py:86-112 -> int64[top_k] (device)."""
    am, kl = ops.token_stats(attention_maps, num_subjects=num_subjects, sigma=sigma, eps=epsilon)
    return _ranked(kl, am[0], attention_maps.shape[-1], top_k)


def furthest_point_sampling(attention_maps, top_k, top_initial_candidates):
    """ptp_utils.py:115-159 -> int64[min(top_k, candidates)] (device); greedy max-min over the candidates' arg-max
    pixels (the reference's loop stops adding once every candidate is chosen, :142-157)."""
    am, _ = ops.token_stats(attention_maps, num_subjects=1, want_kl=False)
    n = attention_maps.shape[0]
    cand = torch.as_tensor(top_initial_candidates, device=attention_maps.device).long()
    order = torch.full((n,), float("inf"), device=attention_maps.device)
    order[cand] = torch.arange(cand.numel(), device=attention_maps.device, dtype=torch.float32)
    _, sel = ops.select_tokens(order, am[0], attention_maps.shape[-1], int(cand.numel()),
                               min(int(top_k), int(cand.numel())))
    return sel


def entropy_sort(attention_maps, top_k, min_dist=0.05):
    """ptp_utils.py:165-187 -> int64[top_k] (device): tokens by ascending entropy of softmax_{R*R}(map)."""
    am, _, ent = ops.token_stats(attention_maps, num_subjects=1, want_kl=False, want_entropy=True)
    return _ranked(ent, am[0], attention_maps.shape[-1], top_k)


def init_random_noise(device, num_words=77, dim=768):
    """ptp_utils.py:649-650 (`dim` = the UNet's cross_attention_dim: 768 SD-1.x, 1024 SD-2.x, 2048 SDXL)."""
    return torch.randn(1, num_words, dim).to(device)
