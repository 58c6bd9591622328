"""Route ledger: which implementation every gated call site took, and how often.

Half of a step reaches the HIP kernels through gates (`ops.conv3x3_auto`, the forwards of `ldm/fused.py`, the flash and
cross-attention dispatch, the map kernels' shape rules) that hand a call to another kernel family, to the library, or back to the
module's own forward when a shape test says no.  The parity tests compare values, so a gate that regresses stays green and shows
up only as a slower step.  Every gate therefore notes its choice here:

    routes.note(site, route)        what the gates call (plain dict arithmetic)
    routes.snapshot() / reset() / table()
    with routes.expect(allow=routes.DOCUMENTED_LIBRARY_ROUTES): ...     raises UnexpectedRoute on exit
    with routes.strict(allow=...): ...                                  raises inside note(), at the offending gate

Every (site, route) pair is registered below with a KIND:
    "hip"      a kernel of libskp_hip.so
    "library"  hipBLASLt / rocBLAS / MIOpen through ATen on the GPU in place of an own kernel
    "eager"    the module's original forward
    "host"     the CPU-tensor branches (the module tree on the host is what the oracle drives)
`note()` with a pair that is not registered raises KeyError: a typo in a gate must not open a silent new column.  Plain nn.Linear
GEMMs are the design's stated plumbing and are not routes.

Sites are named by role, not by module path.  Where the C library picks the kernel form by a launch plan of its own, the gate names
the route from the library's own `*_ok` queries or from the plan's stated shape rule (`wino4_form`, `cross_attn_form` below).
A convolution whose batch is launched in chunks, or a map launch that runs token groups, is ONE decision and one note.
"""
from __future__ import annotations

import contextlib
import threading
from typing import Dict, Iterable, Optional, Tuple

KINDS = ("hip", "library", "eager", "host")

_WINO = {"wino4_c128": "hip", "wino4_c64": "hip", "wino4_raw": "hip", "wino2": "hip", "lib": "library"}
_FLASH = {"flash_split": "hip", "flash_f32": "hip", "self_attn_gen1": "hip"}
_BLOCK = {"fused": "hip", "eager": "eager"}

# site -> route -> kind
ROUTES: Dict[str, Dict[str, str]] = {
    # 3x3 / stride 1 / pad 1 convolutions of the frozen blocks (named by ops.conv3x3_plan, noted by ops._conv3x3_run / conv3x3_auto)
    "conv3x3": dict(_WINO),
    # their input gradient (ops.Conv3x3Fn.backward); the zero-stuffed stride-2 gradient runs on the same kernels and counts here too
    "conv3x3.bwd_data": dict(_WINO),
    "conv_in": {"small": "hip"},                          # <= 4 input channels (ops.conv3x3_small)
    # its input gradient when the latent takes one (keypoint guidance; ops.ConvInFn): the small-output kernel on the flipped filter
    "conv_in.bwd_data": {"small_out": "hip"},
    # <= 8 output channels: below the Winograd kernels' channel blocks; the VAE decoder's <= 4 on its own VALU kernel
    "conv_out": {"lib": "library", "small_out": "hip"},
    # Upsample2D of the VAE decoder, and of the UNet inside the sampling loop (ops.conv3x3_up2): polyphase kernel on the
    # low-resolution input / interpolate + the stride-1 convolution (which notes its own `conv3x3` route as well)
    "upsample_conv": {"up2_poly": "hip", "interp_wino": "hip"},
    "conv3x3_s2": {"s2_direct": "hip", "s2_wino": "hip"},  # ops._conv3x3_s2_raw: direct / polyphase Winograd F(4x4,2x2)
    "conv3x3_s2.bwd_data": {"zero_stuffed": "hip", "lib": "library"},
    "downsample": {"s2_direct": "hip", "eager": "eager"},
    "downsample.untiled": {"eager": "eager"},             # input no multiple of the stride-2 kernel's 16 x 32 pixel tile
    "resnet": dict(_BLOCK),
    "transformer2d": dict(_BLOCK),
    "transformer_block": dict(_BLOCK),
    "time_embedding": {"eager": "eager"},                 # (the kept embedding launches nothing and has no route)
    "group_norm": {"gn_fold": "hip", "gn_apply": "hip"},  # folded into the consuming convolution's patch load / own apply pass
    "group_norm.stats": {"producer_blocks": "hip", "own_pass": "hip"},
    "add_layer_norm": {"add_ln": "hip"},
    # VAE mid-block attention, one head of d = 512 (ops.vae_attn_route): the wide flash forward / library GEMMs + softmax
    "vae.attention": {"flash_wide": "hip", "lib_core": "library", "eager": "eager"},
    # causal attention core of the CLIP text towers (ops.text_attention, ldm/clip.py): the short-sequence causal kernel (N <= 128,
    # heads of 32 / 64 channels: every product tower) / library GEMMs + a masked softmax (another head size or length, and
    # ops.TEXT_ATTN_MODE = "lib"; NOT a documented library route: no supported tower takes it) / the module tree on host tensors
    "text.attention": {"causal_fused": "hip", "lib_core": "library", "host": "host"},
    "vae.tail": {"composed": "hip", "eager": "eager"},
    "vae.decoder": dict(_BLOCK),                          # Decoder.forward: fused tail (GroupNorm + SiLU, small-output conv_out) / its own
    # ptp_utils.latent2image: float NCHW image -> uint8 NHWC on the device (bytes cross to the host) / numpy on the host
    "image.u8": {"nhwc_u8": "hip", "host": "host"},
    # the step of a named sampler (ptp_utils.sampler_latent_step; text2image_ldm_stable(sampler=) other than the eta = 0 DDIM
    # step it always had, which has no gate and notes nothing): the fused step kernel / the formula in torch on host tensors
    "sample.step": {"sampler_step": "hip", "host": "host"},
    # text2image_ldm_stable(capture=True), once per step: a replay of the recorded step (its gates' own notes are merged per replay)
    # / the step on eager launches (the warm-up steps, and calls that cannot be recorded) / host tensors.  A call without
    # `capture` notes nothing here.
    "sample.loop": {"graph": "hip", "eager": "eager", "host": "host"},
    # energy and latent gradient of keypoint guidance (ptp_utils.keypoint_energy_grad): the fused maps + point-loss node
    # (ops.MapPointLossFn; its map kernels note `map.fwd` / `map.bwd` as well) / torch ops on host tensors and other dtypes
    "sample.keypoints": {"map_point_loss": "hip", "host": "host"},
    # the same with target MAPS (pose transfer: keypoint_energy_grad with `MapTargets`, text2image_ldm_stable(target_maps=)): the fused
    # maps + target-loss node (ops.MapTargetLossFn) / the two formulas of include/skp_targets.h in torch ops on host tensors
    "sample.pose": {"map_target_loss": "hip", "host": "host"},
    # visualize.overlay: (min, max) of every heat map, and images + maps + points -> bytes in a canvas: the range and overlay
    # kernels (ops.map_range, ops.overlay_u8) / visualize.range_formula, visualize.overlay_formula in torch on host tensors
    "visualize.range": {"map_range": "hip", "host": "host"},
    "visualize.overlay": {"overlay_u8": "hip", "host": "host"},
    # eval.locate_keypoints: the maps of a whole group of images -> peak locations (arg-max or the weighted mean around it): the
    # locator kernel (ops.locate) / eval.locate_formula in torch on host tensors and other dtypes
    "eval.locate": {"locate": "hip", "host": "host"},
    "attn.cross": {"ca_token_split": "hip", "ca_plain": "hip", "flash": "hip", "host": "host"},
    "attn.self": {"fused_qkv": "hip", "plain": "hip", "host": "host"},
    "flash.fwd": dict(_FLASH),
    "flash.bwd": dict(_FLASH),
    "map.fwd": {"map_fused": "hip", "map_wide": "hip", "map_groups": "hip", "host": "host"},
    "map.bwd": {"map_dense": "hip", "map_dense_groups": "hip", "map_col": "hip", "map_tok": "hip"},
    "map.select": {"batched": "hip", "per_image": "hip"},
    "map.collect": {"reference_ops": "library", "host": "host"},      # materialised entries: the reference's op sequence
    "select.rank": {"select_kernel": "hip", "sort": "library"},
}

# The non-HIP routes the supported configurations are MEANT to take on the GPU today: (site, route) -> reason.
DOCUMENTED_LIBRARY_ROUTES: Dict[Tuple[str, str], str] = {
    ("vae.attention", "lib_core"): "VAE mid-block attention, one head of d = 512, below ops.VAE_FLASH_MIN_KEYS keys (32 769; the 512^2 encode / decode has 4 096, SDXL at 1024^2 16 384) or with an "
                                    "input that needs a gradient: baddbmm + softmax + bmm (the wide flash kernel is forward only)",
    ("conv_out", "lib"): "UNet conv_out 320 -> 4 (full forward only) and a VAE conv_out 512 -> 8 whose tail is not composed: "
                         "output channels below the Winograd kernels' 32-channel blocks",
    ("downsample.untiled", "eager"): "Downsample2D whose input is no multiple of the stride-2 kernel's 16 x 32 pixel tile (SD-1.5 at 512^2: "
                                     "1280 -> 1280 at 16^2 -> 8^2): the module's own stride-2 convolution on MIOpen, forward and backward",
}


class UnexpectedRoute(RuntimeError):
    """A route outside the expected kinds ran.  `.found`: [(site, route, count)]."""

    def __init__(self, found):
        self.found = list(found)
        super().__init__("unexpected kernel routes: " + ", ".join(
            f"{s}/{r} x{n} ({ROUTES[s][r]})" for s, r, n in self.found))


# One table per noting thread (thread id -> site -> route -> count), summed on read: a thread only ever writes its own table, so
# the launch thread and the GroupLoader's assembler thread can note at once without a lock on the hot path.
_lock = threading.Lock()                     # guards the set of tables, not the counts
_tables: Dict[int, Dict[str, Dict[str, int]]] = {}
_ident = threading.get_ident
_denied: Optional[frozenset] = None          # strict mode: the pairs note() refuses


def _own_table() -> Dict[str, Dict[str, int]]:
    with _lock:
        return _tables.setdefault(_ident(), {s: dict.fromkeys(rs, 0) for s, rs in ROUTES.items()})


def kind(site: str, route: str) -> str:
    return ROUTES[site][route]


def note(site: str, route: str, n: int = 1) -> None:
    """Count one decision.  Host-side dict arithmetic on the calling thread's own table and nothing else: no tensor is read, no device
    call is made, nothing synchronises, so it is legal -- and free of side effects -- while a stream is being captured into a
    graph (keep it so).  An unregistered pair raises KeyError."""
    try:
        table = _tables[_ident()]
    except KeyError:
        table = _own_table()
    table[site][route] += n
    if _denied is not None and (site, route) in _denied:
        raise UnexpectedRoute([(site, route, n)])


def snapshot() -> Dict[Tuple[str, str], int]:
    """(site, route) -> count, pairs that ran only."""
    with _lock:
        tables = list(_tables.values())
    total: Dict[Tuple[str, str], int] = {}
    for t in tables:
        for s, rs in t.items():
            for r, c in rs.items():
                if c:
                    total[(s, r)] = total.get((s, r), 0) + c
    return {k: c for k, c in total.items() if c}


def reset() -> None:
    """Empty the ledger (call it between runs, not while another thread is inside a gate: that thread's note may survive)."""
    with _lock:
        for t in _tables.values():
            for rs in t.values():
                for r in rs:
                    rs[r] = 0


def delta(before: Dict[Tuple[str, str], int], after: Optional[Dict[Tuple[str, str], int]] = None) -> Dict[Tuple[str, str], int]:
    """Counts added between two snapshots (`after` None: now)."""
    after = snapshot() if after is None else after
    return {k: after.get(k, 0) - before.get(k, 0) for k in set(before) | set(after) if after.get(k, 0) != before.get(k, 0)}


def merge(counts: Dict[Tuple[str, str], int], times: int = 1) -> None:
    """Add `times` x `counts` to the ledger in one pass (a replayed graph adds what its capture noted; times = -1 takes it out)."""
    table = _own_table()
    for (s, r), c in counts.items():
        table[s][r] += times * c


def _outside(counts, allow, kinds):
    allow = set(allow or ())
    return sorted((s, r, c) for (s, r), c in counts.items() if c > 0 and ROUTES[s][r] not in kinds and (s, r) not in allow)


@contextlib.contextmanager
def expect(allow: Iterable[Tuple[str, str]] = (), kinds: Iterable[str] = ("hip",)):
    """On exit: raises UnexpectedRoute naming every (site, route, count) noted inside the block whose kind is outside `kinds` and which
    is not in `allow`."""
    kinds = tuple(kinds)
    before = snapshot()
    yield
    found = _outside(delta(before), allow, kinds)
    if found:
        raise UnexpectedRoute(found)


@contextlib.contextmanager
def strict(allow: Iterable[Tuple[str, str]] = (), kinds: Iterable[str] = ("hip",)):
    """The rule of `expect`, process-wide and at once: inside the block `note()` raises at the offending call, so the traceback
    points at the gate."""
    global _denied
    kinds, allow = tuple(kinds), set(allow or ())
    prev = _denied
    _denied = frozenset((s, r) for s, rs in ROUTES.items() for r, k in rs.items() if k not in kinds and (s, r) not in allow)
    try:
        yield
    finally:
        _denied = prev


MODES = ("off", "report", "strict")


def guard(mode: str = "off"):
    """The `routes=` keyword of `optimize_embedding` / `precompute_all_keypoints` / `run_image_with_context_augmented` as a context
    manager: "off" does nothing; "report" resets the ledger, so that `table()` afterwards describes this run; "strict" also
    runs the block under `strict(allow=DOCUMENTED_LIBRARY_ROUTES)`."""
    if mode not in MODES:
        raise ValueError(f"routes must be one of {MODES}, got {mode!r}")
    if mode == "off":
        return contextlib.nullcontext()
    reset()
    return strict(allow=DOCUMENTED_LIBRARY_ROUTES) if mode == "strict" else contextlib.nullcontext()


def table(counts: Optional[Dict[Tuple[str, str], int]] = None) -> str:
    """Sites as rows, routes as columns; routes that are not HIP kernels carry their kind: `lib[library]=2`."""
    counts = snapshot() if counts is None else counts
    sites = [s for s in ROUTES if any(k[0] == s for k in counts)]
    cols = []
    for s in sites:
        for r in ROUTES[s]:
            if (s, r) in counts and r not in cols:
                cols.append(r)
    if not sites:
        return "(no routes noted)"
    w0 = max(len("site"), *(len(s) for s in sites))

    def head(r):
        ks = {ROUTES[s][r] for s in sites if (s, r) in counts} - {"hip"}
        return r + ("[" + "/".join(sorted(ks)) + "]" if ks else "")
    heads = [head(r) for r in cols]
    lines = ["  ".join(["site".ljust(w0)] + [h.rjust(max(len(h), 6)) for h in heads])]
    for s in sites:
        lines.append("  ".join([s.ljust(w0)] + [(str(counts[(s, r)]) if (s, r) in counts else ".").rjust(max(len(h), 6))
                                                for r, h in zip(cols, heads)]))
    return "\n".join(lines)


def non_hip(counts: Optional[Dict[Tuple[str, str], int]] = None):
    """[(site, route, count, kind, documented reason or None)] of the routes that ran outside the HIP kernels."""
    counts = snapshot() if counts is None else counts
    return [(s, r, c, ROUTES[s][r], DOCUMENTED_LIBRARY_ROUTES.get((s, r)))
            for (s, r), c in sorted(counts.items()) if ROUTES[s][r] != "hip"]


# ---------------------------------------------------------------------------------------------
# names of the kernel forms the C library picks by a launch plan of its own (pure functions of the shapes)
# ---------------------------------------------------------------------------------------------
def wino4_form(cout: int, rows: int, h: int, w: int) -> str:
    """F(4x4,3x3) transformed-filter launch: the 128-channel workgroup form from 128 tiles on where the output channels fill its
    groups (a ragged last group of >= 64), the 64-channel form otherwise.  A RESTATEMENT of csrc/skp_conv_wino4.hip's
    wino4_use_c128 (the C ABI has no query for it; tests/test_routes.py checks it against skp_conv3x3_f4_gn_ok where that query
    decides the same thing).  A batch launched in chunks is named by its full chunks; a shorter last chunk may take the other form."""
    tiles = rows * (h // 4) * (w // 4)
    return "wino4_c128" if tiles >= 128 and (cout % 128 == 0 or (cout > 128 and cout % 128 >= 64)) else "wino4_c64"


def cross_attn_form(B: int, H: int, N: int, T: int, d: int, ts_off: bool = False) -> str:
    """Short-key cross-attention launch: the token-split form where the 128-query grid leaves the chip under one wave per SIMD
    (d = 80 / 160, >= 2 token tiles), the 128-query form otherwise (`ts_off`: the `cross_attn_ts` developer override is set to 1).
    A RESTATEMENT of csrc/skp_cross_attn.hip's ca_use_ts: no query of the C ABI answers differently for the two forms (their
    workspace is the same), so a change to that plan must be repeated here."""
    if ts_off or (T + 31) // 32 < 2 or d not in (80, 160):
        return "ca_plain"
    return "ca_token_split" if ((N + 127) // 128) * H * B * 4 < 1024 else "ca_plain"
