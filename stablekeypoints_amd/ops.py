"""Torch-facing wrappers of the HIP kernels (libskp_hip.so via ctypes).

PyTorch is used here only for device memory, streams and autograd bookkeeping; every op below
launches hand-written gfx950 kernels through the C ABI of include/skp.h on torch's CURRENT
stream.  No op has an eager/CPU fallback: a non-CUDA tensor raises.
"""
from __future__ import annotations

import contextlib
import weakref
from collections import namedtuple
from typing import List, Sequence, Tuple

import torch

from . import _native as N
from . import routes


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dev(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{name}: the StableKeypoints hot path runs on the HIP kernels only "
                           f"(got a {t.device} tensor; there is no CPU fallback)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: expected float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _ptr(t):
    return t.data_ptr() if t is not None else None


_ANY, _INT, _HOST = "any dtype", "an int", "a host value"      # what a slot of a launch plan takes, besides a torch dtype
_plans = {}


def _plan(name: str):
    """(the entry, what each of its arguments before the stream takes) from the table of `_native`; made once per entry."""
    slots = tuple((t.dtype or _ANY) if issubclass(t, N.DevicePointer) else _INT if t in (N._i, N._i64) else _HOST
                  for t in N.signature(name)[:-1])
    _plans[name] = plan = (getattr(N.lib(), name), slots)
    return plan


def _refused(name: str, i: int, want, a):
    if not isinstance(a, torch.Tensor):
        return TypeError(f"{name}: argument {i} takes an int, got {type(a).__name__} {a!r}")
    if want in (_INT, _HOST):
        return TypeError(f"{name}: argument {i} is no device pointer, got a tensor ({a.dtype}, {a.device})")
    if not a.is_cuda:
        return RuntimeError(f"{name}: argument {i}: the StableKeypoints hot path runs on the HIP kernels only "
                            f"(got a {a.device} tensor; there is no CPU fallback)")
    if a.get_device() != torch.cuda.current_device():
        return RuntimeError(f"{name}: argument {i}: expected a tensor on the current device cuda:{torch.cuda.current_device()} "
                            f"(the launch goes to its current stream), got one on {a.device}")
    return RuntimeError(f"{name}: argument {i}: expected {want}, got {a.dtype}")


def _launch(name: str, *args):
    """The one way this module starts a kernel: entry `name` of include/skp.h with `args` and torch's current stream, its return
    code checked.  A tensor stands for its address and is held to its slot first -- a device-pointer slot, on the current device,
    of the element type the header declares (`void*` takes any) -- so a wrong tensor is an exception here, not a fault on the
    device.  None is a null pointer; an int at a pointer slot is an address the caller has offset itself.  Nothing is copied,
    cast or made contiguous (`_dev` does that), and strides are not looked at: column bands and batch slices pass as they are."""
    fn, slots = _plans.get(name) or _plan(name)
    if len(args) != len(slots):
        raise TypeError(f"{name}: takes {len(slots)} arguments and the stream, got {len(args)}")
    call, device = [], None
    for a, want in zip(args, slots):
        if isinstance(a, torch.Tensor):
            if device is None and a.is_cuda:
                device = torch.cuda.current_device()
            if want is _INT or want is _HOST or a.get_device() != device or (want is not _ANY and a.dtype is not want):
                raise _refused(name, len(call), want, a)
            a = a.data_ptr()
        elif want is _INT and isinstance(a, float):
            raise _refused(name, len(call), want, a)
        call.append(a)
    N.check(fn(*call, _stream()), name)


def _workspace(query: str, *args, device):
    """Scratch for the launch that follows: `query(*args)` bytes as ceil(bytes / 4) floats, None (a null pointer) for 0 bytes;
    a negative answer raises."""
    nbytes = int(getattr(N.lib(), query)(*args))
    if nbytes < 0:
        N.check(nbytes, query)
    return torch.empty((nbytes + 3) // 4, device=device, dtype=torch.float32) if nbytes else None


def _gn_scratch(n: int, groups: int, device):
    """Statistics scratch of the GroupNorm entries (include/skp.h, skp_group_norm_fwd_f32: "workspace: N*G*64*3 floats")."""
    return torch.empty(n * groups * 64 * 3, device=device, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------
# values derived from frozen tensors (transformed filters, stacked weights, folded offsets / biases)
# ---------------------------------------------------------------------------------------------
# Built once and kept on an owner object (a Parameter or a module), so an entry dies with its owner.  An entry is reused while
# every input it was built from is the same object with the same storage, version, device and dtype; a changed input replaces
# the entry under its key; an input that takes gradients keeps nothing.  While a step is captured (optimize.GraphedStep) every
# value handed out is also held by the recording, for as long as the graph that reads it lives.
_recording = None


def frozen_tag(inputs):
    """(storage, version, device, dtype) of every input that is not None, or None when one of them takes gradients (nothing
    derived from it may be kept)."""
    tag = []
    for t in inputs:
        if t is not None:
            if t.requires_grad:
                return None
            tag.append((t.data_ptr(), t._version, t.device, t.dtype))
    return tuple(tag)


def handed_out(value):
    if _recording is not None:
        _recording.append(value)
    return value


@contextlib.contextmanager
def recording():
    """-> a list that receives every kept value handed out inside the block."""
    global _recording
    prev, _recording = _recording, []
    try:
        yield _recording
    finally:
        _recording = prev


def cached(owner, key, inputs, build):
    """`build()` -- a tensor or tuple of tensors that depends on `inputs` (None entries are skipped) and on what `key` names --
    kept on `owner`."""
    tag = frozen_tag(inputs)
    if tag is None:
        return build()
    store = owner.__dict__.setdefault("_skp_cache", {})
    hit = store.get(key)
    if hit is None or hit[0] != tag or not all(r() is t for r, t in zip(hit[1], (t for t in inputs if t is not None))):
        hit = store[key] = (tag, [weakref.ref(t) for t in inputs if t is not None], build())
    return handed_out(hit[2])


# ---------------------------------------------------------------------------------------------
# low-res logits (fp32 MFMA)                                            ptp_utils.py:483-493
# ---------------------------------------------------------------------------------------------
def qk_logits(q: torch.Tensor, k: torch.Tensor, heads: int, scale: float) -> torch.Tensor:
    """S[b,h,p,t] = scale*log2(e) * <q[b,p,h,:], k[bk,t,h,:]>;  q [B,s2,C], k [Bk,T,C] -> [B,H,s2,NT]
    (token-contiguous, NT = 16*ceil(T/16), pad columns zero)."""
    q, k = _dev(q, "q"), _dev(k, "k")
    B, s2, C = q.shape
    Bk, T, Ck = k.shape
    if Ck != C or C % heads:
        raise RuntimeError("qk_logits: channel mismatch")
    S = torch.empty(B, heads, s2, (T + 15) // 16 * 16, device=q.device, dtype=torch.float32)
    _launch("skp_qk_logits_f32", q, k, S, B, Bk, heads, T, s2, C // heads, float(scale))
    return S


def _gemm_nt(A, B, Cout, M, Nn, K, Z0, Z1, sa, sb, sc, alpha):
    _launch("skp_gemm_nt_f32", A, B, Cout, M, Nn, K, Z0, Z1, *sa, *sb, *sc, alpha)


TOKEN_GROUP = 128          # most tokens one fused-map launch can hold (one softmax row per lane, in registers)
GROUP_STEP = 96            # group width when T > TOKEN_GROUP (NT=96 instantiation: no register spills)


def _groups(T: int):
    return [(t0, min(T, t0 + GROUP_STEP)) for t0 in range(0, T, GROUP_STEP)]


def _log2sumexp2(xs: List[torch.Tensor]) -> torch.Tensor:
    st = torch.stack(xs, 0)
    m = st.max(dim=0).values
    return m + torch.log2(torch.exp2(st - m).sum(dim=0))


MAP_WIDE = True          # False (tests): token groups x two passes for T > 128
MAP_WIDE_MAX_T = 1024


def map_wide_supported(T: int, R: int, sides: Sequence[int] = (16,)) -> bool:
    """The one-pass wide kernel serves T in (128, 1024] where its launch plan fits (the library's own gate: layer side
    <= 64, R % 32 == 0, tile count, LDS); everything else takes the two-pass token-group route."""
    if not (MAP_WIDE and TOKEN_GROUP < T <= MAP_WIDE_MAX_T and R % 32 == 0):
        return False
    si, _keep = N.int_array([int(v) for v in sides])
    return bool(N.lib().skp_attn_map_fwd_wide_ok(si, len(sides), int(T), int(R)))


def _map_fwd(S: Sequence[torch.Tensor], sides: Sequence[int], B: int, H: int, T: int, R: int, tokrow=None, n_rows: int = 0):
    """-> (M [B,T,R,R], lse [B,L*H,R*R] log2-sum-exp over all tokens).  T <= 128: all tokens of a pixel in one lane;
    more tokens: ONE pass with the token axis in 64-token slices across lanes (csrc/skp_attn_map_wide.hip); shapes that
    kernel does not take run token groups in two passes (group statistics -> combine -> apply).
    `tokrow` (int32 [T] on the device: output row of a token or -1) restricts the written maps to `n_rows` rows -- wide
    kernel only."""
    dev = S[0].device
    L, ldt = len(S), S[0].shape[-1]
    si, _k2 = N.int_array(sides)
    if map_wide_supported(T, R, sides):
        routes.note("map.fwd", "map_wide")
        M = torch.empty(B, n_rows if tokrow is not None else T, R, R, device=dev, dtype=torch.float32)
        lse = torch.empty(B, L * H, R * R, device=dev, dtype=torch.float32)
        sp, _k1 = N.ptr_array([t.data_ptr() for t in S])
        _launch("skp_attn_map_fwd_wide_f32", sp, si, L, B, H, T, R, M, lse, tokrow, n_rows, ldt)
        return M, lse
    if tokrow is not None:
        raise RuntimeError("_map_fwd: row selection is served by the wide-token kernel only")
    M = torch.empty(B, T, R, R, device=dev, dtype=torch.float32)

    def launch(t0, t1, mode, lse_out, lse_in):
        sp, _k1 = N.ptr_array([t.data_ptr() + 4 * t0 for t in S])
        _launch("skp_attn_map_fwd_ex_f32", sp, si, L, B, H, t1 - t0, R, M.data_ptr() + 4 * t0 * R * R, lse_out, lse_in,
                ldt, T * R * R, mode)

    if T <= TOKEN_GROUP:
        routes.note("map.fwd", "map_fused")
        lse = torch.empty(B, L * H, R * R, device=dev, dtype=torch.float32)
        launch(0, T, 0, lse, None)
        return M, lse
    routes.note("map.fwd", "map_groups")
    parts = []
    for t0, t1 in _groups(T):
        parts.append(torch.empty(B, L * H, R * R, device=dev, dtype=torch.float32))
        launch(t0, t1, 1, parts[-1], None)
    lse = _log2sumexp2(parts)
    for t0, t1 in _groups(T):
        launch(t0, t1, 2, None, lse)
    return M, lse


def _map_bwd(S, dS, sides, B, H, T, R, dM, lse):
    dev = dM.device
    L, ldt = len(S), S[0].shape[-1]
    si, _k3 = N.int_array(sides)
    ws = _workspace("skp_attn_map_bwd_workspace", si, L, B, H, T if T <= TOKEN_GROUP else GROUP_STEP, R, device=dev)

    def launch(t0, t1, mode, dot):
        sp, _k1 = N.ptr_array([t.data_ptr() + 4 * t0 for t in S])
        dp, _k2 = N.ptr_array([t.data_ptr() + 4 * t0 for t in dS])
        _launch("skp_attn_map_bwd_ex_f32", sp, dp, si, L, B, H, t1 - t0, R, dM.data_ptr() + 4 * t0 * R * R, lse, ws, dot,
                ldt, T * R * R, mode)

    if T <= TOKEN_GROUP:
        routes.note("map.bwd", "map_dense")
        launch(0, T, 0, None)
        return
    routes.note("map.bwd", "map_dense_groups")
    dots = []
    for t0, t1 in _groups(T):
        dots.append(torch.empty(B, L * H, R * R, device=dev, dtype=torch.float32))
        launch(t0, t1, 1, dots[-1])
    dot = torch.stack(dots, 0).sum(dim=0)
    for t0, t1 in _groups(T):
        launch(t0, t1, 2, dot)


# Which map backward the fused step takes.  The losses give the map gradient as K selected rows per batch row; "auto" hands
# it over in that form (one map+losses node, ops.MapLossesFn) wherever a sparse kernel is the faster route:
#   the column sweep (csrc/skp_attn_map_col.hip, round 4: vertical adjoint in a register window, horizontal adjoint on complete
#   low-res rows, no dV staging) wherever it serves the shapes (R in {128, 256}, R / s in {4, 8}, K <= 16, any T <= 1024):
#   377 us against 541 us for the dense kernels at T = 77, 1.56 ms against 2.47 ms for the token-major sweep at T = 500;
#   other shapes: T <= 128 the dense-gradient kernels (the token-major sweep is slower there: 636 us), T > 128 the
#   token-major sweep (2.4 vs 7.9 ms at T = 500, B = 8, for token groups x two passes of the dense kernels).
# "col" / "sweep" force one sparse kernel where it serves the shapes, "sparse" = either, "dense" forces the dense route.
MAP_BWD_MODE = "auto"
MAP_SPARSE_MAX_SIDE, MAP_SPARSE_MAX_K, MAP_SPARSE_MAX_R = 32, 32, 1024     # limits of csrc/skp_attn_map_tok.hip
COL_MAX_T = 1024                                                             # token counts the column sweep is taken for


def map_bwd_col_supported(sides, K: int, R: int, T: int, heads: int = 8) -> bool:
    si, _keep = N.int_array([int(v) for v in sides])
    return bool(N.lib().skp_attn_map_bwd_col_ok(si, len(sides), int(heads), int(T), int(R), int(K)))


def map_bwd_sparse_supported(sides, K: int, R: int, T: int = 10 ** 9, heads: int = 8) -> bool:
    if MAP_BWD_MODE == "dense":
        return False
    col = MAP_BWD_MODE != "sweep" and T <= COL_MAX_T and map_bwd_col_supported(sides, K, R, T, heads)
    sweep = (MAP_BWD_MODE != "col" and max(sides) <= MAP_SPARSE_MAX_SIDE and 1 <= K <= MAP_SPARSE_MAX_K
             and R <= MAP_SPARSE_MAX_R)
    if MAP_BWD_MODE == "auto":
        return col or (sweep and T > TOKEN_GROUP)     # at T <= 128 the token-major sweep is slower than the dense route
    return col or sweep


def _map_bwd_sparse(S, sides, B, H, T, R, sel, G, lse):
    """dS[l] for a map gradient that is non-zero on the rows sel[b,:] of batch row b only (G [B,K,R,R] = those rows):
    token-major sweep, any T, no token groups, no dV staging (csrc/skp_attn_map_tok.hip)."""
    L, ldt, K = len(S), S[0].shape[-1], sel.shape[1]
    sel = sel.to(torch.int64).contiguous()
    G = _dev(G, "G")
    dS = [torch.empty_like(s_) for s_ in S]
    si, _k0 = N.int_array(sides)
    if MAP_BWD_MODE != "sweep" and T <= COL_MAX_T and map_bwd_col_supported(sides, K, R, T, H):
        query, name = "skp_attn_map_bwd_col_workspace", "skp_attn_map_bwd_col_f32"              # column sweep
        routes.note("map.bwd", "map_col")
    else:
        query, name = "skp_attn_map_bwd_sparse_workspace", "skp_attn_map_bwd_sparse_f32"        # token-major sweep
        routes.note("map.bwd", "map_tok")
    ws = _workspace(query, si, L, B, H, T, R, K, device=G.device)
    sp, _k1 = N.ptr_array([t.data_ptr() for t in S])
    dp, _k2 = N.ptr_array([t.data_ptr() for t in dS])
    _launch(name, sp, dp, si, L, B, H, T, R, sel, G, K, lse, ws, ldt)
    if ldt > (T + 15) // 16 * 16:                              # gap columns of a wider logits buffer: never read, keep finite
        for d_ in dS:
            d_[..., (T + 15) // 16 * 16:] = 0
    return dS


def _dqk_from_dS(qs, ks, dS, scales, H: int, T: int, needs) -> List[torch.Tensor]:
    """dq_l = scale * dS_l k_l, dk_l = scale * dS_l^T q_l on the fp32-MFMA GEMM (deterministic; a shared k sums over the
    batch rows).  `needs[2l]`, `needs[2l+1]`: which gradients autograd asked for."""
    grads: List[torch.Tensor] = []
    for l in range(len(qs)):
        q, k, ds, sc = qs[l], ks[l], dS[l], scales[l]
        B, s2, C = q.shape
        d = C // H
        Bk = k.shape[0]
        NT = ds.shape[-1]
        dq = dk = None
        if needs[2 * l]:
            dq = torch.empty_like(q)       # dq[b,p,h*d+c] = sc * sum_t dS[b,h,p,t] k[bk,t,h*d+c]
            _gemm_nt(ds, k, dq, s2, d, T, B, H,
                     (H * s2 * NT, s2 * NT, NT, 1), (0 if Bk == 1 else T * C, d, 1, C),
                     (s2 * C, d, C), sc)
        if needs[2 * l + 1]:
            dkb = torch.empty(B, T, C, device=q.device, dtype=torch.float32)
            _gemm_nt(ds, q, dkb, T, d, s2, B, H,    # dk[b,t,h*d+c] = sc * sum_p dS[b,h,p,t] q[b,p,h*d+c]
                     (H * s2 * NT, s2 * NT, 1, NT), (s2 * C, d, 1, C), (T * C, d, C), sc)
            dk = dkb.sum(dim=0, keepdim=True) if (Bk == 1 and B > 1) else dkb
        grads += [dq, dk]
    return grads


class MapStack(namedtuple("MapStack", "qs ks heads scales R sides B Bk T L")):
    """The hooked cross-attention layers behind one reduced map: q_l [B,s_l^2,C_l], k_l [Bk,T,C_l] with Bk in {1, B}, one head
    count and up-res side R for all, one logit scale per layer; `sides` = (s_l), `Bk` = the context rows of layer 0.  Checked
    here and nowhere else, before a kernel takes the geometry of layer 0 for every layer: shapes first (host tensors get that
    far), then `_dev` on every tensor.  `who` names the caller in the errors."""
    __slots__ = ()

    def __new__(cls, who: str, qs, ks, heads: int, scales, R: int):
        qs, ks, heads, scales = tuple(qs), tuple(ks), int(heads), tuple(float(v) for v in scales)
        L = len(qs)
        if L == 0 or len(ks) != L:
            raise RuntimeError(f"{who}: empty layer stack: one q and one k per hooked layer, got {L} and {len(ks)}")
        if len(scales) != L:
            raise RuntimeError(f"{who}: one scale per layer: {len(scales)} scales for {L} layers")
        B, Bk, T = qs[0].shape[0], ks[0].shape[0], ks[0].shape[1]
        sides = []
        for l, (q, k) in enumerate(zip(qs, ks)):
            s = int(round(q.shape[1] ** 0.5))
            bad = (f"query length {q.shape[1]} is not a square" if s * s != q.shape[1] else
                   f"q has {q.shape[0]} batch rows, layer 0 has {B}" if q.shape[0] != B else
                   f"k has {k.shape[0]} batch rows, neither 1 nor {B}" if k.shape[0] not in (1, B) else
                   f"k has a token count of {k.shape[1]}, layer 0 has {T}" if k.shape[1] != T else
                   f"{q.shape[2]} q channels do not split into {heads} heads" if q.shape[2] % heads else
                   f"k has {k.shape[2]} channels, q has {q.shape[2]}" if k.shape[2] != q.shape[2] else None)
            if bad:
                raise RuntimeError(f"{who}: layer {l}: {bad}")
            sides.append(s)
        return super().__new__(cls, tuple(_dev(q, "q") for q in qs), tuple(_dev(k, "k") for k in ks), heads, scales, int(R),
                               tuple(sides), B, Bk, T, L)

    @classmethod
    def of_flat(cls, who: str, qk, heads: int, scales, R: int):
        """The stack of `flat()`'s (q_0, k_0, q_1, k_1, ...), as `Function.apply` hands it to a node's forward."""
        return cls(who, qk[0::2], qk[1::2], heads, scales, R)

    def flat(self):
        return tuple(t for qk in zip(self.qs, self.ks) for t in qk)

    def logits(self) -> List[torch.Tensor]:
        return [qk_logits(q, k, self.heads, sc) for q, k, sc in zip(self.qs, self.ks, self.scales)]

    def maps(self, tokrow=None, n_rows: int = 0):
        """-> (S, M, lse): the layers' logits and `_map_fwd` of them."""
        S = self.logits()
        return (S, *_map_fwd(S, self.sides, self.B, self.heads, self.T, self.R, tokrow=tokrow, n_rows=n_rows))


def _save_stack(ctx, st: MapStack, S, lse, *own):
    """Keeps what a map node's backward needs: the tensors in autograd's saved-tensor slots, the geometry on `ctx`."""
    ctx.save_for_backward(lse, *st.qs, *st.ks, *S, *own)
    ctx.stack = st._replace(qs=(), ks=())


def _saved_stack(ctx):
    """-> (the stack, S, lse, own) that `_save_stack` kept."""
    t, L = ctx.saved_tensors, ctx.stack.L
    return ctx.stack._replace(qs=t[1:1 + L], ks=t[1 + L:1 + 2 * L]), t[1 + 2 * L:1 + 3 * L], t[0], t[1 + 3 * L:]


def _stack_grads(st: MapStack, S, lse, needs, dM=None, rows=None, sparse=None):
    """(dq_0, dk_0, dq_1, dk_1, ...) from the map gradient, given dense (`dM` [B,T,R,R]) or as its non-zero rows (`rows` =
    (sel [B,K], G [B,K,R,R])).  Rows go to the sparse kernels where `sparse` says so -- None asks `map_bwd_sparse_supported` --
    and are scattered into a dense gradient otherwise."""
    B, H, T, R = st.B, st.heads, st.T, st.R
    if rows is not None and sparse is None:
        sparse = map_bwd_sparse_supported(st.sides, rows[0].shape[1], R, T, H)
    if rows is not None and sparse:
        dS = _map_bwd_sparse(S, st.sides, B, H, T, R, *rows, lse)
    else:
        if rows is not None:
            sel, G = rows
            dM = torch.zeros(B, T, R, R, device=G.device, dtype=torch.float32).scatter_(1, sel[:, :, None, None].expand_as(G), G)
        # pad columns (t >= T) of a LAST partial group are written as 0 by the kernels; zero-fill covers the
        # (never read) gap columns when T > 128 is not a multiple of 16
        dS = [torch.empty_like(s_) if T <= TOKEN_GROUP else torch.zeros_like(s_) for s_ in S]
        _map_bwd(S, dS, st.sides, B, H, T, R, _dev(dM, "dM"), lse)
    return _dqk_from_dS(st.qs, st.ks, dS, st.scales, H, T, needs)


class AttnMapFn(torch.autograd.Function):
    """M[b,t,:,:] = mean over (layer, head) of softmax_t(bicubic_R(scale * q_l k_l^T)).

    Replaces ptp_utils.py:513-538 + optimize.py:27-79 (see csrc/skp_attn_map.hip).
    apply(R, heads, scales(tuple), q_0, k_0, q_1, k_1, ...) with q_l [B,s_l^2,C_l], k_l [Bk,T,C_l].
    """

    @staticmethod
    def forward(ctx, R: int, heads: int, scales: Tuple[float, ...], *qk: torch.Tensor):
        st = MapStack.of_flat("AttnMapFn", qk, heads, scales, R)
        S, M, lse = st.maps()
        _save_stack(ctx, st, S, lse)
        return M

    @staticmethod
    def backward(ctx, dM: torch.Tensor):
        st, S, lse, _ = _saved_stack(ctx)
        return (None, None, None, *_stack_grads(st, S, lse, ctx.needs_input_grad[3:], dM=dM))


def attn_map(qs: Sequence[torch.Tensor], ks: Sequence[torch.Tensor], heads: int, scales: Sequence[float],
             R: int) -> torch.Tensor:
    st = MapStack("attn_map", qs, ks, heads, scales, R)
    return AttnMapFn.apply(st.R, st.heads, st.scales, *st.flat())


@torch.no_grad()
def attn_map_rows(qs: Sequence[torch.Tensor], ks: Sequence[torch.Tensor], heads: int, scales: Sequence[float], R: int,
                  indices: torch.Tensor) -> torch.Tensor:
    """[B,len(indices),R,R]: the maps of the tokens `indices` only (optimize.py:58-59 `data[:, :, :, indices]`; inference
    keeps K of the T maps).  With a wide token axis (T > 128) the kernel writes just those rows -- the softmax still runs
    over all T tokens; otherwise all T maps are written and gathered.  No autograd (inference path)."""
    st = MapStack("attn_map_rows", qs, ks, heads, scales, R)
    idx = torch.as_tensor(indices, device=st.qs[0].device).long().reshape(-1)
    if map_wide_supported(st.T, st.R, st.sides):
        uniq, inv = torch.unique(idx, return_inverse=True)      # a token asked for twice is written once
        tokrow = torch.full((st.T,), -1, device=idx.device, dtype=torch.int32)
        tokrow[uniq] = torch.arange(uniq.numel(), device=idx.device, dtype=torch.int32)
        _, M, _ = st.maps(tokrow=tokrow, n_rows=int(uniq.numel()))
        return M if uniq.numel() == idx.numel() and bool((inv == torch.arange(idx.numel(), device=idx.device)).all()) else M[:, inv]
    return st.maps()[1][:, idx]


def materialize_probs(q: torch.Tensor, k: torch.Tensor, heads: int, scale: float, R: int) -> torch.Tensor:
    """Reference-layout tensor (B*h, R*R, T) of one hooked layer (ptp_utils.py:535-538), produced by
    the SAME fused kernel run one head at a time (L=1, H=1).  Compatibility/testing path only."""
    st = MapStack("materialize_probs", [q], [k], heads, [scale], R)
    S, = st.logits()
    outs = []
    for h in range(heads):
        Sh = S[:, h:h + 1].contiguous()
        Mh, _ = _map_fwd([Sh], st.sides, st.B, 1, st.T, R)      # [B,T,R,R]
        outs.append(Mh.reshape(st.B, st.T, R * R).permute(0, 2, 1))
    return torch.stack(outs, dim=1).reshape(st.B * heads, R * R, st.T)


# ---------------------------------------------------------------------------------------------
# token statistics / selection                      eval.py:39-111, ptp_utils.py:86-159
# ---------------------------------------------------------------------------------------------
def token_stats(M: torch.Tensor, num_subjects: int = 1, sigma: float = 2.0, eps: float = 1e-5,
                want_kl: bool = True, want_entropy: bool = False):
    """-> (argmax int32 [num_subjects, T] flat indices, kl float32 [T] or None[, entropy float32 [T]])."""
    M = _dev(M.detach(), "M")
    T, R, R2 = M.shape
    if R != R2:
        raise RuntimeError("token_stats: map must be square")
    am = torch.empty(num_subjects, T, device=M.device, dtype=torch.int32)
    kl = torch.empty(T, device=M.device, dtype=torch.float32) if want_kl else None
    ent = torch.empty(T, device=M.device, dtype=torch.float32) if want_entropy else None
    _launch("skp_token_stats_f32", M, T, R, num_subjects, float(sigma), float(eps), am, kl, ent)
    return (am, kl, ent) if want_entropy else (am, kl)


SELECT_MAX_CANDIDATES = 64     # SKP_SEL_MAXC / SKP_SEL_MAXT of csrc/skp_select_loss.hip
SELECT_MAX_TOKENS = 1024


def select_tokens(kl: torch.Tensor, argmax_t: torch.Tensor, R: int, n_cand: int, top_k: int):
    """-> (cand int64 [n_cand], sel int64 [top_k]); argmax_t = first-subject arg-max of the TRANSFORMED map."""
    T = kl.shape[0]
    cand = torch.empty(n_cand, device=kl.device, dtype=torch.int64)
    sel = torch.empty(top_k, device=kl.device, dtype=torch.int64)
    am = argmax_t.reshape(-1)[:T].contiguous()
    _launch("skp_select_tokens", kl, am, T, R, n_cand, top_k, cand, sel)
    return cand, sel


# ---------------------------------------------------------------------------------------------
# losses                                             optimize.py:157-206
# ---------------------------------------------------------------------------------------------
def invert_affine(theta) -> List[float]:
    """Inverse of the 2x3 affine [[a,b,tx],[c,d,ty]] (invertable_transform.py:77-84), closed form in fp64."""
    a, b, tx, c, d, ty = [float(v) for v in theta]
    det = a * d - b * c
    ia, ib, ic, id_ = d / det, -b / det, -c / det, a / det
    return [ia, ib, -(ia * tx + ib * ty), ic, id_, -(ic * tx + id_ * ty)]


class LossesFn(torch.autograd.Function):
    """(sharpening_loss, equivariance_loss) of optimize.py:157-206 for the selected tokens, fused with
    their gradients.  apply(M, Mt, sel, argmax, theta_inv(6 floats), sigma, num_subjects)."""

    @staticmethod
    def forward(ctx, M, Mt, sel, argmax, theta_inv, sigma, num_subjects):
        M, Mt = _dev(M, "M"), _dev(Mt, "Mt")
        T, R, _ = M.shape
        K = sel.shape[0]
        nchunk = (R * R + 1023) // 1024
        partial = torch.empty(2, K, nchunk, device=M.device, dtype=torch.float32)
        g_sharp = torch.empty(K, R, R, device=M.device, dtype=torch.float32)
        g_eq_a = torch.empty_like(g_sharp)
        g_eq_b = torch.empty_like(g_sharp)
        th, _keep = N.float_array(theta_inv)
        _launch("skp_losses_fwd_f32", M, Mt, sel, K, T, R, argmax, int(num_subjects), float(sigma), th, partial, g_sharp, g_eq_a,
                g_eq_b)
        sums = partial.sum(dim=(1, 2)) / float(K * R * R)
        ctx.save_for_backward(sel, g_sharp, g_eq_a, g_eq_b)
        ctx.shape = (T, R)
        return sums[0], sums[1]

    @staticmethod
    def backward(ctx, go_sharp, go_equiv):
        sel, g_sharp, g_eq_a, g_eq_b = ctx.saved_tensors
        T, R = ctx.shape
        dev = g_sharp.device
        z = torch.zeros((), device=dev, dtype=torch.float32)
        gs = z if go_sharp is None else go_sharp.reshape(()).float().contiguous()
        ge = z if go_equiv is None else go_equiv.reshape(()).float().contiguous()
        dM = torch.zeros(T, R, R, device=dev, dtype=torch.float32)
        dMt = torch.zeros(T, R, R, device=dev, dtype=torch.float32)
        K, n = sel.shape[0], R * R
        _launch("skp_rows_axpy_f32", dM, sel, K, n, g_sharp, gs, g_eq_a, ge)
        _launch("skp_rows_axpy_f32", dMt, sel, K, n, g_eq_b, ge, None, None)
        return dM, dMt, None, None, None, None, None


def fused_losses(M, Mt, sel, argmax, theta, sigma: float, num_subjects: int = 1):
    """theta: the FORWARD 2x3 affine of this image (6 floats, row-major). -> (sharp, equiv)."""
    return LossesFn.apply(M, Mt, sel, argmax, invert_affine(theta), float(sigma), int(num_subjects))


MAP_LOSSES_BATCHED = True     # False (tests): statistics / selection per image, through meta["score_fn"]


class MapLossesFn(torch.autograd.Function):
    """One node for `maps -> selection -> losses` of a group of images (optimize.py:347-414 for n images x 2 views), so that
    the map backward sees the gradient as it is -- K selected rows per batch row -- instead of a dense [B,T,R,R] tensor:
        forward : logits -> fused maps (+ lse) -> per image: token scores, selection, both losses and their unit gradients
        backward: G = go_sharp * g_sharp + go_equiv * g_eq (K rows per batch row) -> sparse token-major map backward
                  (csrc/skp_attn_map_tok.hip) -> dq_l, dk_l on the fp32-MFMA GEMM.
    apply(meta, q_0, k_0, q_1, k_1, ...) with rows 0..n-1 = the images, n..2n-1 = their affine copies;
    meta = dict(R, heads, scales, thetas [n][6] (host) or theta_inv_dev [n,6] (device), sigma, num_subjects, strategy, n_cand,
    top_k, score_fn).
    Returns (sum_i sharp_i, sum_i equiv_i, sel [n,K] int64)."""

    @staticmethod
    def forward(ctx, meta, *qk: torch.Tensor):
        st = MapStack.of_flat("MapLossesFn", qk, meta["heads"], meta["scales"], meta["R"])
        R, B, T = st.R, st.B, st.T
        n = B // 2
        th_dev = meta.get("theta_inv_dev")          # [n, 6] float32 on the device, instead of meta["thetas"] (host numbers)
        if th_dev is not None and (not th_dev.is_cuda or th_dev.dtype != torch.float32 or tuple(th_dev.shape) != (n, 6) or not th_dev.is_contiguous()):
            raise RuntimeError("MapLossesFn: theta_inv_dev must be a contiguous float32 [n, 6] device tensor")
        if B != 2 * n or (th_dev is None and len(meta["thetas"]) != n):
            raise RuntimeError("MapLossesFn: rows must be n images followed by their n affine copies, one affine per image")
        S, M, lse = st.maps()
        sigma, ns = float(meta["sigma"]), int(meta["num_subjects"])
        n_cand = min(int(meta["n_cand"]), T)
        K = min(int(meta["top_k"]), n_cand)
        dev = M.device
        sel_all = torch.empty(n, K, device=dev, dtype=torch.int64)
        g_sharp = torch.empty(n, K, R, R, device=dev, dtype=torch.float32)
        g_eq_a, g_eq_b = torch.empty_like(g_sharp), torch.empty_like(g_sharp)
        nchunk = (R * R + 1023) // 1024
        partial = torch.empty(n, 2, K, nchunk, device=dev, dtype=torch.float32)
        # token statistics and the selection of ALL images in three launches (one workgroup per (image, token) / per image: the
        # per-image launches were 77 workgroups of 40 us each, twelve of them per step); per-token results are what the
        # per-image calls give, bit for bit
        strategy = meta["strategy"]
        # (a caller-supplied score function is honoured: only the stock order of optimize.token_order is batched)
        batched = (strategy in ("gaussian", "entropy", "consistent") and T <= SELECT_MAX_TOKENS and n_cand <= SELECT_MAX_CANDIDATES
                   and K >= 2 and MAP_LOSSES_BATCHED and getattr(meta.get("score_fn"), "_skp_stock_order", False))
        routes.note("map.select", "batched" if batched else "per_image")
        if batched:
            flat = M.reshape(B * T, R, R)
            st_all = token_stats(flat[:n * T], num_subjects=ns, sigma=sigma, want_kl=strategy == "gaussian",
                                 want_entropy=strategy == "entropy")
            am_all = st_all[0].reshape(ns, n, T).permute(1, 0, 2).contiguous()                  # [n, ns, T]
            if strategy == "gaussian":
                score_all = st_all[1].reshape(n, T)
            elif strategy == "entropy":
                score_all = st_all[2].reshape(n, T)
            else:
                score_all = torch.arange(T, device=dev, dtype=torch.float32).repeat(n, 1)
            amt_all, _ = token_stats(flat[n * T:], num_subjects=1, sigma=sigma, want_kl=False)  # [1, n*T]
            cand_all = torch.empty(n, n_cand, device=dev, dtype=torch.int64)
            _launch("skp_select_tokens_batched", score_all.contiguous(), amt_all, n, T, R, n_cand, K, cand_all, sel_all)
        for i in range(n):
            if batched:
                am = am_all[i]
            else:
                am, score = meta["score_fn"](M[i], strategy, ns, sigma)
                am_t, _ = token_stats(M[n + i], num_subjects=1, sigma=sigma, want_kl=False)
                _, sel_i = select_tokens(score, am_t[0], R, n_cand, K)
                sel_all[i].copy_(sel_i)
            if th_dev is not None:                   # inverse affines in device memory (a captured step: new numbers per replay)
                _launch("skp_losses_fwd_dev_f32", M[i], M[n + i], sel_all[i], K, T, R, am, ns, sigma, th_dev[i], partial[i],
                        g_sharp[i], g_eq_a[i], g_eq_b[i])
                continue
            th, _keep = N.float_array(invert_affine(meta["thetas"][i]))
            _launch("skp_losses_fwd_f32", M[i], M[n + i], sel_all[i], K, T, R, am, ns, sigma, th, partial[i], g_sharp[i],
                    g_eq_a[i], g_eq_b[i])
        sums = partial.sum(dim=(0, 2, 3)) / float(K * R * R)
        _save_stack(ctx, st, S, lse, sel_all, g_sharp, g_eq_a, g_eq_b)
        ctx.mark_non_differentiable(sel_all)
        return sums[0], sums[1], sel_all

    @staticmethod
    def backward(ctx, go_sharp, go_equiv, _go_sel):
        st, S, lse, (sel_all, g_sharp, g_eq_a, g_eq_b) = _saved_stack(ctx)
        z = torch.zeros((), device=lse.device)
        gs = z if go_sharp is None else go_sharp.reshape(()).float()
        ge = z if go_equiv is None else go_equiv.reshape(()).float()
        G = torch.cat([gs * g_sharp + ge * g_eq_a, ge * g_eq_b], dim=0)            # [B,K,R,R]
        rows = (torch.cat([sel_all, sel_all], dim=0), G)        # (the caller took this node because the sparse kernels serve it)
        return (None, *_stack_grads(st, S, lse, ctx.needs_input_grad[1:], rows=rows, sparse=True))


def point_loss(M, pos, sigma: float):
    """Energy of K maps per image against gaussian targets at given positions (csrc/skp_point_loss.hip, formula in
    include/skp_keypoints.h): M [B,K,R,R], pos [B,K,2] (row, col) in image fractions, on the device -> (E [B] = mean_{k,r,c} (M - t)^2,
    G [B,K,R,R] = dE[b] / dM[b]).  No autograd; one kernel and one fixed-order sum of its chunk sums: the same bits from call to call."""
    M, pos = _dev(M.detach(), "M"), _dev(pos.detach(), "pos")
    if M.dim() != 4 or M.shape[2] != M.shape[3] or tuple(pos.shape) != (M.shape[0], M.shape[1], 2):
        raise RuntimeError(f"point_loss: maps {tuple(M.shape)} must be [B,K,R,R] and positions {tuple(pos.shape)} [B,K,2]")
    B, K, R, _ = M.shape
    partial = torch.empty(B, K, (R * R + 1023) // 1024, device=M.device, dtype=torch.float32)
    G = torch.empty_like(M)
    _launch("skp_point_loss_f32", M, pos, B, K, R, float(sigma), partial, G)
    return partial.sum(dim=(1, 2)) / float(K * R * R), G


TARGET_MODES = {"mse": 0, "cosine": 1}      # the `mode` of include/skp_targets.h by the name `text2image_ldm_stable(target_energy=)` takes


def map_target_loss(M, target, mode):
    """Energy of K maps per image against K target maps (csrc/skp_target_loss.hip, formulas in include/skp_targets.h): M [B,K,R,R],
    target [B,K,R,R] or [1,K,R,R] (one target for every image, read in place), on the device; `mode` "mse" -- E[b] = mean_{k,r,c}
    (M - T)^2 -- or "cosine" -- E[b] = (1/K) sum_k (1 - cos(M_k, T_k)), a map of zeros counting 1 -> (E [B], G [B,K,R,R] = dE[b] /
    dM[b]).  No autograd; one or two kernels and one fixed-order sum of their chunk sums: the same bits from call to call."""
    if mode not in TARGET_MODES:
        raise ValueError(f"map_target_loss: mode must be one of {sorted(TARGET_MODES)}, got {mode!r}")
    M, target = _dev(M.detach(), "M"), _dev(target.detach(), "target")
    if M.dim() != 4 or M.shape[2] != M.shape[3] or target.dim() != 4 or target.shape[0] not in (1, M.shape[0]) \
            or tuple(target.shape[1:]) != tuple(M.shape[1:]):
        raise RuntimeError(f"map_target_loss: maps {tuple(M.shape)} must be [B,K,R,R] and targets {tuple(target.shape)} [B,K,R,R] "
                           "or [1,K,R,R]")
    B, K, R, _ = M.shape
    code = TARGET_MODES[mode]
    partial = torch.empty(B, K, (R * R + 1023) // 1024, device=M.device, dtype=torch.float32)
    G = torch.empty_like(M)
    ws = _workspace("skp_map_target_loss_workspace", B, K, R, code, device=M.device)
    _launch("skp_map_target_loss_f32", M, target, B, target.shape[0], K, R, code, partial, G, ws)
    return partial.sum(dim=(1, 2)) / (float(K * R * R) if code == 0 else float(2 * K)), G


def _k_row_maps(st, sel, tokrow):
    """(S, M [B,K,R,R], lse) of a stack for the K tokens `sel`: the K rows alone where the wide kernel serves the shape, else all
    rows and a gather."""
    if map_wide_supported(st.T, st.R, st.sides):
        return st.maps(tokrow=tokrow, n_rows=sel.shape[0])
    S, M, lse = st.maps()
    return S, M.index_select(1, sel), lse


def _k_row_backward(ctx, go):
    """The backward of an energy of K rows per batch row whose forward saved (sel, G): G scaled by the incoming gradient, through
    `_stack_grads(rows=...)`."""
    st, S, lse, (sel, G) = _saved_stack(ctx)
    rows = (sel.expand(st.B, sel.shape[0]), go.reshape(st.B, 1, 1, 1).float() * G)
    return (None, *_stack_grads(st, S, lse, ctx.needs_input_grad[1:], rows=rows))


class MapPointLossFn(torch.autograd.Function):
    """One node for `maps of K tokens -> energy against caller-given positions` (keypoint guidance of image sampling,
    ptp_utils.keypoint_energy_grad), the sibling of MapLossesFn: the map backward sees K rows per batch row, not a dense [B,T,R,R].
        forward : logits -> fused maps (+ lse): the K rows alone where the wide kernel serves the shape, else all rows and a gather
                  -> point-loss kernel (energy and unit gradient)
        backward: G = go[b] * g[b] -> the sparse map backward where `map_bwd_sparse_supported`, else the rows scattered into a dense
                  gradient for the dense kernels -> dq_l (dk_l only if asked for: the context usually needs no gradient).
    apply(meta, q_0, k_0, q_1, k_1, ...); meta = dict(R, heads, scales, sigma, pos [B,K,2] float32 on the device, sel int64 [K]
    on the device: K distinct token ids, tokrow int32 [T] on the device: the output row of a token or -1).  Returns E [B]."""

    @staticmethod
    def forward(ctx, meta, *qk: torch.Tensor):
        st = MapStack.of_flat("MapPointLossFn", qk, meta["heads"], meta["scales"], meta["R"])
        sel, pos, tokrow = meta["sel"], meta["pos"], meta["tokrow"]
        K = sel.shape[0]
        if tuple(pos.shape) != (st.B, K, 2) or tuple(tokrow.shape) != (st.T,):
            raise RuntimeError("MapPointLossFn: positions [B,K,2] and a row table of T tokens")
        S, M, lse = _k_row_maps(st, sel, tokrow)
        E, G = point_loss(M, pos, float(meta["sigma"]))
        _save_stack(ctx, st, S, lse, sel, G)
        return E

    backward = staticmethod(_k_row_backward)


class MapTargetLossFn(torch.autograd.Function):
    """MapPointLossFn against target MAPS (pose transfer, ptp_utils.keypoint_energy_grad with `MapTargets`): the same forward up to
    the K rows' maps, `map_target_loss` for the energy and its unit gradient, the same backward.
    apply(meta, q_0, k_0, q_1, k_1, ...); meta = dict(R, heads, scales, target [B,K,R,R] or [1,K,R,R] float32 on the device, mode
    "mse" / "cosine", sel, tokrow as there).  Returns E [B]."""

    @staticmethod
    def forward(ctx, meta, *qk: torch.Tensor):
        st = MapStack.of_flat("MapTargetLossFn", qk, meta["heads"], meta["scales"], meta["R"])
        sel, target, tokrow = meta["sel"], meta["target"], meta["tokrow"]
        K = sel.shape[0]
        if target.dim() != 4 or target.shape[0] not in (1, st.B) or tuple(target.shape[1:]) != (K, st.R, st.R) \
                or tuple(tokrow.shape) != (st.T,):
            raise RuntimeError("MapTargetLossFn: targets [B,K,R,R] or [1,K,R,R] and a row table of T tokens")
        S, M, lse = _k_row_maps(st, sel, tokrow)
        E, G = map_target_loss(M, target, meta["mode"])
        _save_stack(ctx, st, S, lse, sel, G)
        return E

    backward = staticmethod(_k_row_backward)


UNWARP_MAX_K = 32


@torch.no_grad()
def unwarp_accumulate(maps: torch.Tensor, theta_inv: torch.Tensor, size: int, finish: bool = True):
    """Tail of the augmented inference (eval.py:239-353): maps [n,K,R,R] of n views, theta_inv [n,2,3] their inverse
    affines -> (sum_v unwarp(bilinear_{R->size}(maps[v])) [K,size,size], coverage count [size,size]); with `finish` the
    first is already sum / count with 0/0 -> 0.  One kernel (csrc/skp_unwarp.hip); K > 32 runs in chunks of 32 tokens."""
    maps = _dev(maps, "maps")
    n, K, R, _ = maps.shape
    th = theta_inv.to(device=maps.device, dtype=torch.float32).reshape(n, 6).contiguous()
    tot = torch.empty(K, size, size, device=maps.device, dtype=torch.float32)
    num = torch.empty(size, size, device=maps.device, dtype=torch.float32)
    for k0 in range(0, K, UNWARP_MAX_K):
        k1 = min(K, k0 + UNWARP_MAX_K)
        chunk = maps if (k0 == 0 and k1 == K) else maps[:, k0:k1].contiguous()
        _launch("skp_unwarp_accumulate_f32", chunk, th, n, k1 - k0, R, size, tot[k0:k1], num, 1 if finish else 0)
    return tot, num


# ---------------------------------------------------------------------------------------------
# ordinary cross-attention core (short key axis)                 ptp_utils.py:493-506,540
# ---------------------------------------------------------------------------------------------
CROSS_ATTN_HEAD_DIMS = (8, 16, 32, 40, 64, 80, 160)
CROSS_ATTN_MAX_T = 128


def cross_attn_supported(C: int, heads: int, T: int) -> bool:
    """Every key count is served: T <= 128 by the in-register softmax kernel, more tokens (the reference default is
    --num_tokens 500, main.py:77-79) by the key-tiled online-softmax (flash) kernels."""
    return C % heads == 0 and (C // heads) in CROSS_ATTN_HEAD_DIMS


class CrossAttnFn(torch.autograd.Function):
    """out[b,n,:] = merge_heads(softmax(scale q k^T) v); q [B,N,C], k,v [Bk,T,C] (Bk in {1,B}) -> [B,N,C]."""

    @staticmethod
    def forward(ctx, q, k, v, heads: int, scale: float):
        q, k, v = _dev(q, "q"), _dev(k, "k"), _dev(v, "v")
        B, Nq, C = q.shape
        Bk, T, _ = k.shape
        out = torch.empty_like(q)
        lse = torch.empty(B, heads, Nq, device=q.device, dtype=torch.float32)
        routes.note("attn.cross", routes.cross_attn_form(B, heads, Nq, T, C // heads, N.lib().skp_tune_get(b"cross_attn_ts") == 1))
        _launch("skp_cross_attn_fwd_f32", q, k, v, out, lse, B, Bk, heads, Nq, T, C // heads, float(scale))
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.meta = (heads, float(scale))
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        heads, scale = ctx.meta
        dout = _dev(dout, "dout")
        B, Nq, C = q.shape
        Bk, T, _ = k.shape
        dq = torch.empty_like(q)
        dk = torch.empty(B, T, C, device=q.device, dtype=torch.float32)
        dv = torch.empty_like(dk)
        ws = _workspace("skp_cross_attn_bwd_workspace", B, heads, Nq, T, C // heads, device=q.device)
        _launch("skp_cross_attn_bwd_f32", q, k, v, out, dout, lse, dq, dk, dv, ws, B, Bk, heads, Nq, T, C // heads, scale)
        if Bk == 1 and B > 1:
            dk, dv = dk.sum(dim=0, keepdim=True), dv.sum(dim=0, keepdim=True)
        return dq, dk, dv, None, None


def cross_attention(q, k, v, heads: int, scale: float):
    if k.shape[1] > CROSS_ATTN_MAX_T:
        routes.note("attn.cross", "flash")
        return FlashAttnFn.apply(q, k, v, int(heads), float(scale))
    return CrossAttnFn.apply(q, k, v, int(heads), float(scale))


# ---------------------------------------------------------------------------------------------
# causal self-attention of the CLIP text towers (csrc/skp_text_attn.hip)      ptp_utils.py:436-439
# ---------------------------------------------------------------------------------------------
# "auto": the causal kernel wherever it serves the shape (N <= 128, heads of 32 / 64 channels: all three product towers), library
# GEMMs + a masked softmax elsewhere; "lib" (tests): the library everywhere.
TEXT_ATTN_MODE = "auto"
TEXT_ATTN_MODES = ("auto", "lib")


def text_attn_supported(width: int, heads: int, n_tokens: int) -> bool:
    return (width % heads == 0
            and N.lib().skp_text_attn_fwd_ok(1, int(heads), int(n_tokens), int(width) // int(heads), int(width)) == 1)


def _text_attn_lib(q, k, v, heads: int, scale: float):
    """Library route of the same core: batched GEMMs and a softmax over the logits with -inf above the diagonal."""
    B, Nn, C = q.shape
    qh, kh, vh = (t.reshape(B, Nn, heads, C // heads).permute(0, 2, 1, 3) for t in (q, k, v))
    S = torch.matmul(qh, kh.transpose(-1, -2)) * scale
    S = S.masked_fill(torch.ones(Nn, Nn, device=q.device, dtype=torch.bool).triu(1), float("-inf"))
    return torch.matmul(torch.softmax(S, dim=-1), vh).permute(0, 2, 1, 3).reshape(B, Nn, C)


def text_attention(qkv_or_q, k, v, heads: int, scale: float):
    """out[b,i] = merge_heads(softmax_{j<=i}(scale q_i k_j^T) v); no gradient.  Either q, k, v [B,N,C] each (dense, or views with one
    common row stride such as the column bands of a stacked projection), or `qkv_or_q` [B,N,3C] holding q | k | v side by side and
    k = v = None: the kernel reads the three bands in place.  -> dense [B,N,C].  Notes `text.attention`: `causal_fused`, or
    `lib_core` for a head size or length the kernel does not serve and under TEXT_ATTN_MODE = "lib"."""
    if TEXT_ATTN_MODE not in TEXT_ATTN_MODES:
        raise ValueError(f"ops.TEXT_ATTN_MODE must be one of {TEXT_ATTN_MODES}, got {TEXT_ATTN_MODE!r}")
    if (k is None) != (v is None):
        raise RuntimeError("text_attention: pass q, k and v, or one packed q | k | v tensor with k = v = None")
    if k is None:
        qkv = _dev(qkv_or_q, "qkv")
        if qkv.dim() != 3 or qkv.shape[-1] % 3:
            raise RuntimeError(f"text_attention: packed q | k | v must be [B, N, 3C], got {tuple(qkv.shape)}")
        C = qkv.shape[-1] // 3
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    else:
        q, k, v = qkv_or_q, k, v
        for name, t in (("q", q), ("k", k), ("v", v)):
            if not t.is_cuda or t.dtype != torch.float32:
                _dev(t, name)                                    # raises: host tensor or another dtype
        if q.dim() != 3 or k.shape != q.shape or v.shape != q.shape:
            raise RuntimeError(f"text_attention: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} must be equal [B, N, C]")
        strides = {t.stride() for t in (q, k, v)}
        B_, N_, C_ = q.shape
        ld = q.stride(1)
        if not (len(strides) == 1 and q.stride(2) == 1 and ld >= C_ and ld % 4 == 0 and (B_ == 1 or q.stride(0) == N_ * ld)
                and all(t.data_ptr() % 16 == 0 for t in (q, k, v))):
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    B, Nn, C = q.shape
    if C % heads:
        raise RuntimeError(f"text_attention: width {C} is no multiple of {heads} heads")
    d, ld = C // heads, q.stride(1)
    if TEXT_ATTN_MODE == "lib" or N.lib().skp_text_attn_fwd_ok(B, heads, Nn, d, ld) != 1 or any(t.data_ptr() % 16 for t in (q, k, v)):
        routes.note("text.attention", "lib_core")
        return _text_attn_lib(q, k, v, int(heads), float(scale))
    routes.note("text.attention", "causal_fused")
    out = torch.empty(B, Nn, C, device=q.device, dtype=torch.float32)
    _launch("skp_text_attn_fwd_f32", q, k, v, out, B, heads, Nn, d, ld, float(scale))
    return out


# ---------------------------------------------------------------------------------------------
# fused GroupNorm (+offset) (+SiLU) of the frozen network's blocks
# ---------------------------------------------------------------------------------------------
def group_norm_supported(x: torch.Tensor, groups: int) -> bool:
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] % groups == 0
            and (x.shape[2] * x.shape[3]) % 4 == 0 and x.shape[0] * groups <= 65535)


class GroupNormSiLUFn(torch.autograd.Function):
    """y = act(GroupNorm(x + off[:, :, None, None])) with act = SiLU or identity; gamma/beta/off frozen."""

    @staticmethod
    def forward(ctx, x, off, gamma, beta, groups: int, eps: float, silu: bool, blocks=None):
        x = _dev(x, "x")
        Nn, C, Hh, Ww = x.shape
        off_c = _dev(off.reshape(Nn, C), "off") if off is not None else None
        y = torch.empty_like(x)
        mean = torch.empty(Nn, groups, device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        routes.note("group_norm", "gn_apply")
        if blocks is not None:                       # statistics from the producing convolution's epilogue
            routes.note("group_norm.stats", "producer_blocks")
            bs, nblk, pix = blocks
            _launch("skp_group_norm_fwd_blocks_f32", x, off_c, gamma, beta, y, mean, rstd, bs, nblk, pix, Nn, C, groups, Hh * Ww,
                    float(eps), silu)
        else:
            routes.note("group_norm.stats", "own_pass")
            ws = _gn_scratch(Nn, groups, x.device)
            _launch("skp_group_norm_fwd_f32", x, off_c, gamma, beta, y, mean, rstd, ws, Nn, C, groups, Hh * Ww, float(eps), silu)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(x, off_c if off_c is not None else x.new_empty(0), gamma, beta, mean, rstd)
        ctx.meta = (groups, float(eps), bool(silu), off_c is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, off_c, gamma, beta, mean, rstd = ctx.saved_tensors
        groups, eps, silu, has_off = ctx.meta
        dy = _dev(dy, "dy")
        Nn, C, Hh, Ww = x.shape
        dx = torch.empty_like(x)
        ws = _gn_scratch(Nn, groups, x.device)
        _launch("skp_group_norm_bwd_f32", x, off_c if has_off else None, gamma, beta, dy, mean, rstd, dx, ws, Nn, C, groups,
                Hh * Ww, eps, silu)
        return dx, None, None, None, None, None, None, None


class GroupNormSiLUForkFn(torch.autograd.Function):
    """(y, x') = (act(GroupNorm(x + off)), x): the norm of a block whose input ALSO feeds the block's residual path
    (ResnetBlock2D: conv2(...) + x; Transformer2DModel: proj_out(...) + x).  x' is x itself; routing the residual path through
    it hands BOTH gradients of x to this backward, where the residual path's gradient is added inside the norm's
    input-gradient kernel (skp_group_norm_bwd_add_f32) instead of by an accumulation pass of autograd's."""

    @staticmethod
    def forward(ctx, x, off, gamma, beta, groups: int, eps: float, silu: bool, blocks=None):
        y = GroupNormSiLUFn.forward(ctx, x, off, gamma, beta, groups, eps, silu, blocks)
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dxp):
        if dxp is None:
            return GroupNormSiLUFn.backward(ctx, dy)
        x, off_c, gamma, beta, mean, rstd = ctx.saved_tensors
        groups, eps, silu, has_off = ctx.meta
        Nn, C, Hh, Ww = x.shape
        if dy is None:
            return dxp, None, None, None, None, None, None, None
        dy, dxp = _dev(dy, "dy"), _dev(dxp, "dx'")
        dx = torch.empty_like(x)
        ws = _gn_scratch(Nn, groups, x.device)
        _launch("skp_group_norm_bwd_add_f32", x, off_c if has_off else None, gamma, beta, dy, mean, rstd, dx, dxp, ws, Nn, C,
                groups, Hh * Ww, eps, silu)
        return dx, None, None, None, None, None, None, None


def _blocks(x):
    """(block sums, blocks per image, pixels per block) that x's producing convolution left behind (`x._skp_blocks`, written by
    `_leave_blocks` alone), or None when there are none or they do not describe x."""
    blocks = getattr(x, "_skp_blocks", None)
    if blocks is not None and (blocks[0].shape[0] != x.shape[0] or blocks[0].shape[1] != x.shape[1]
                               or blocks[1] * blocks[2] != x.shape[2] * x.shape[3]):
        return None
    return blocks


def group_norm_silu(x, norm: torch.nn.GroupNorm, off=None, silu: bool = True):
    """GroupNorm(+offset)(+SiLU).  If `x` is the output of one of this library's convolutions that left block sums
    behind (`_blocks`), the statistics pass over `x` is skipped."""
    return GroupNormSiLUFn.apply(x, off, norm.weight, norm.bias, norm.num_groups, norm.eps, silu, _blocks(x))


def group_norm_silu_fork(x, norm: torch.nn.GroupNorm, off=None, silu: bool = True):
    """(group_norm_silu(x), x') with x' = x for the block's residual path: see GroupNormSiLUForkFn.  Without a gradient to
    carry x' is x itself and nothing changes."""
    if not (torch.is_grad_enabled() and x.requires_grad):
        return group_norm_silu(x, norm, off=off, silu=silu), x
    return GroupNormSiLUForkFn.apply(x, off, norm.weight, norm.bias, norm.num_groups, norm.eps, silu, _blocks(x))


# ---------------------------------------------------------------------------------------------
# flash-style self-attention (long image-token sequences)          ptp_utils.py:493-506,540
# ---------------------------------------------------------------------------------------------
def self_attn_supported(C: int, heads: int) -> bool:
    return C % heads == 0 and (C // heads) in CROSS_ATTN_HEAD_DIMS


# Flash attention of the big self-attention layers (>= 1024 keys, d = 40 / 80: the 64^2 and 32^2 levels) runs on the BF16 matrix
# cores with THREE-TERM OPERAND SPLITS (csrc/skp_flash_attn_s.hip): fp32 in / out, fp32 softmax and accumulation, every operand of the
# tile products the exact sum of three bf16 terms, six products per fp32 product.  Error against fp64 0.16-0.87x the
# fp32-instruction kernels' on the shapes it serves (tests/test_round5_gpu.py), forward 1.43-1.87x their speed, backward (d = 40)
# 1.10x (profiles/r05_flash_split.md).  Round 6 made it the route of record; FLASH_SPLIT = False restores the fp32-instruction
# kernels everywhere (bench.py times that step beside the line as `f32_instr`).
FLASH_SPLIT = True
FLASH_SPLIT_MIN_KEYS = 1024


def flash_split_ok(B, Bk, heads, Nq, Nk, d, backward=False) -> bool:
    """The split-bf16 kernels take this flash launch (the fp32-instruction kernels every other one)."""
    ok = N.lib().skp_flash_attn_bwd_split_ok if backward else N.lib().skp_flash_attn_fwd_split_ok
    return FLASH_SPLIT and Nk >= FLASH_SPLIT_MIN_KEYS and bool(ok(B, Bk, heads, Nq, Nk, d))


def _flash_fwd(q, k, v, out, lse, heads, scale, split=None):
    """out, lse (natural log) of softmax(scale q k^T) v; `split` forces the kernels, None: `flash_split_ok`."""
    B, Nq, C = q.shape
    Bk, Nk, _ = k.shape
    shape = (B, Bk, heads, Nq, Nk, C // heads)
    if split is None:
        split = flash_split_ok(*shape)
    if split:
        routes.note("flash.fwd", "flash_split")
        ws = _workspace("skp_flash_attn_fwd_split_workspace", *shape, device=q.device)
        _launch("skp_flash_attn_fwd_split_f32", q, k, v, out, lse, ws, *shape, float(scale))
    else:
        routes.note("flash.fwd", "flash_f32" if shape[5] in FA2_HEAD_DIMS else "self_attn_gen1")
        _launch("skp_flash_attn_fwd_f32", q, k, v, out, lse, *shape, float(scale))


def _flash_bwd(q, k, v, out, dout, lse, heads, scale, dq, dk, dv, ld, split=None):
    """dq, dk, dv of `_flash_fwd` into dq / dk / dv -- tensors, or the device addresses of column bands -- rows `ld` floats apart
    (H*d: dense tensors; dk / dv hold B rows even for a shared k / v); `split` as in `_flash_fwd`."""
    B, Nq, C = q.shape
    Bk, Nk, _ = k.shape
    shape = (B, Bk, heads, Nq, Nk, C // heads)
    if split is None:
        split = flash_split_ok(*shape, backward=True)
    if split:
        query, name = "skp_flash_attn_bwd_split_workspace", "skp_flash_attn_bwd_split_ld_f32"
        routes.note("flash.bwd", "flash_split")
    else:
        query, name = "skp_flash_attn_bwd_workspace", "skp_flash_attn_bwd_ld_f32"
        routes.note("flash.bwd", "flash_f32" if shape[5] in FA2_HEAD_DIMS else "self_attn_gen1")
    ws = _workspace(query, *shape, device=q.device)
    _launch(name, q, k, v, out, dout, lse, dq, dk, dv, ws, *shape, float(scale), ld)


def flash_attn_bwd_split(q, k, v, out, dout, lse, heads: int, scale: float):
    """Direct entry (tests / tools): (dq, dk, dv) of the split backward (self-attention shapes)."""
    q, k, v, out, dout, lse = (_dev(t_, "t") for t_ in (q, k, v, out, dout, lse))
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    _flash_bwd(q, k, v, out, dout, lse, heads, scale, dq, dk, dv, q.shape[2], split=True)
    return dq, dk, dv


def flash_attn_fwd_split(q, k, v, heads: int, scale: float):
    """Direct entry (tests / tools): (out, lse) of the split forward."""
    q, k, v = _dev(q, "q"), _dev(k, "k"), _dev(v, "v")
    out = torch.empty_like(q)
    lse = torch.empty(q.shape[0], heads, q.shape[1], device=q.device, dtype=torch.float32)
    _flash_fwd(q, k, v, out, lse, heads, scale, split=True)
    return out, lse


class FlashAttnFn(torch.autograd.Function):
    """out = merge_heads(softmax(scale q k^T) v); q [B,N,C], k, v [Bk,Nk,C] with Bk in {1,B}; key-tiled online
    softmax, scores never materialised.  Self-attention is the Bk == B, Nk == N case."""

    @staticmethod
    def forward(ctx, q, k, v, heads: int, scale: float):
        q, k, v = _dev(q, "q"), _dev(k, "k"), _dev(v, "v")
        B, Nq, C = q.shape
        out = torch.empty_like(q)
        lse = torch.empty(B, heads, Nq, device=q.device, dtype=torch.float32)
        _flash_fwd(q, k, v, out, lse, heads, scale)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.meta = (heads, float(scale))
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        heads, scale = ctx.meta
        dout = _dev(dout, "dout")
        B, Nq, C = q.shape
        Bk, Nk, _ = k.shape
        dq = torch.empty_like(q)
        dk = torch.empty(B, Nk, C, device=q.device, dtype=torch.float32)
        dv = torch.empty_like(dk)
        _flash_bwd(q, k, v, out, dout, lse, heads, scale, dq, dk, dv, C)
        if Bk == 1 and B > 1:
            dk, dv = dk.sum(dim=0, keepdim=True), dv.sum(dim=0, keepdim=True)
        return dq, dk, dv, None, None


SelfAttnFn = FlashAttnFn


def self_attention(q, k, v, heads: int, scale: float):
    routes.note("attn.self", "plain")
    return FlashAttnFn.apply(q, k, v, int(heads), float(scale))


# ---------------------------------------------------------------------------------------------
# VAE mid-block attention: one head of d = 512 (csrc/skp_flash_attn_wide.hip, forward only)
# ---------------------------------------------------------------------------------------------
# "auto": the flash kernel from VAE_FLASH_MIN_KEYS keys on, the library GEMMs + softmax below it; "flash": the kernel wherever it
# can run; "lib": the library everywhere.  Measured (profiles/vae_attention.md), the kernel is 1.16-2.07x SLOWER than the library
# at 9 216 and 16 384 keys, so in "auto" the route exists for memory, not speed: it opens where the library's two fp32 score
# matrices of ONE row (8 keys^2 bytes) exceed 8 GiB, i.e. above 32 768 keys.  The 512^2 encode / decode (4 096 keys) and SD-2.1 /
# SDXL (9 216 / 16 384) stay on the library.
VAE_ATTN_MODE = "auto"
VAE_FLASH_MIN_KEYS = 32 * 1024 + 1
VAE_ATTN_MODES = ("auto", "flash", "lib")


def vae_attn_route(B: int, heads: int, n_keys: int, d: int, needs_grad: bool) -> str:
    """Route of the `vae.attention` core for self-attention over n_keys tokens, `heads` heads of d channels: "flash_wide" or
    "lib_core".  A pure function of its arguments and the two module attributes; the kernel has no backward, so an input that
    needs a gradient always takes the library."""
    if VAE_ATTN_MODE not in VAE_ATTN_MODES:
        raise ValueError(f"ops.VAE_ATTN_MODE must be one of {VAE_ATTN_MODES}, got {VAE_ATTN_MODE!r}")
    if VAE_ATTN_MODE == "lib" or needs_grad:
        return "lib_core"
    if VAE_ATTN_MODE == "auto" and n_keys < VAE_FLASH_MIN_KEYS:
        return "lib_core"
    return "flash_wide" if N.lib().skp_flash_attn_fwd_wide_ok(B, B, heads, n_keys, n_keys, d) == 1 else "lib_core"


def flash_attn_wide(q, k, v, heads: int, scale: float):
    """Direct entry (tests / tools, and the flash route of the VAE attention): out = softmax(scale q k^T) v per head of 512
    channels, q [B,N,heads*512], k / v [B,Nk,heads*512]; no gradient."""
    q, k, v = _dev(q, "q"), _dev(k, "k"), _dev(v, "v")
    B, Nq, C = q.shape
    Bk, Nk, Ck = k.shape
    if C % heads or Ck != C or v.shape != k.shape:
        raise RuntimeError(f"flash_attn_wide: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}, {heads} heads")
    shape = (B, Bk, heads, Nq, Nk, C // heads)
    out = torch.empty_like(q)
    ws = _workspace("skp_flash_attn_fwd_wide_workspace", *shape, device=q.device)
    _launch("skp_flash_attn_fwd_wide_f32", q, k, v, out, ws, *shape, float(scale))
    return out


class AddBiasResidualFn(torch.autograd.Function):
    """out = a + b + bias[None,:,None,None] in one pass (bias frozen); gradients pass straight through."""

    @staticmethod
    def forward(ctx, a, b, bias):
        a, b = _dev(a, "a"), _dev(b, "b")
        Nn, C, Hh, Ww = a.shape
        out = torch.empty_like(a)
        _launch("skp_add_bias_residual_f32", a, b, bias, out, Nn, C, Hh * Ww)
        return out

    @staticmethod
    def backward(ctx, dy):
        return dy, dy, None


def add_bias_residual(a, b, bias):
    return AddBiasResidualFn.apply(a, b, bias)


# ---------------------------------------------------------------------------------------------------------
# residual add + LayerNorm of the transformer blocks, one pass per direction (csrc/skp_layer_norm.hip)
# ---------------------------------------------------------------------------------------------------------
def add_layer_norm_supported(h, norm: torch.nn.LayerNorm) -> bool:
    return bool(h.is_cuda and h.dtype == torch.float32 and len(norm.normalized_shape) == 1
                and norm.elementwise_affine and norm.bias is not None and h.shape[-1] == norm.normalized_shape[0]
                and not (norm.weight.requires_grad or norm.bias.requires_grad)
                and N.lib().skp_add_layer_norm_ok(int(h.shape[-1])))


class AddLayerNormFn(torch.autograd.Function):
    """(x, n) = (d + h, LayerNorm(d + h)); with d None: (h, LayerNorm(h)).  The first output carries the residual stream on,
    so the gradient that reaches it from its later uses is added inside the norm's input-gradient kernel instead of a
    separate accumulation pass; d and h both receive that sum."""

    @staticmethod
    def forward(ctx, d, h, weight, bias, eps):
        h = _dev(h, "h")
        C = h.shape[-1]
        rows = h.numel() // C
        n = torch.empty_like(h)
        stat = torch.empty(rows, 2, device=h.device, dtype=torch.float32)
        if d is not None:
            d = _dev(d, "d")
            x = torch.empty_like(h)
        else:
            x = h
        _launch("skp_add_layer_norm_fwd_f32", d, h, weight, bias, x if d is not None else None, n, stat, rows, C, float(eps))
        ctx.save_for_backward(x, stat, weight)
        ctx.has_d = d is not None
        return x, n                                  # d None: x is the input itself (autograd hands back an alias)

    @staticmethod
    def backward(ctx, gx, gn):
        x, stat, weight = ctx.saved_tensors
        C = x.shape[-1]
        if gn is None:
            dx = gx
        else:
            gn = _dev(gn, "gn")
            gx = _dev(gx, "gx") if gx is not None else None
            dx = torch.empty_like(x)
            _launch("skp_add_layer_norm_bwd_f32", gn, gx, x, stat, weight, dx, x.numel() // C, C)
        return (dx if ctx.has_d else None), dx, None, None, None


def add_layer_norm(d, h, norm: torch.nn.LayerNorm):
    """Returns (d + h, norm(d + h)); d may be None -> (h, norm(h))."""
    routes.note("add_layer_norm", "add_ln")
    return AddLayerNormFn.apply(d, h, norm.weight, norm.bias, norm.eps)


# ---------------------------------------------------------------------------------------------------------
# 3x3 / stride 1 / pad 1 convolutions of the frozen blocks: Winograd F(2x2,3x3) on the fp32 matrix cores.
# ---------------------------------------------------------------------------------------------------------
def conv3x3_supported(x_shape, w_shape, need_grad=True):
    """Shapes the kernel takes (everything else stays on the library convolution)."""
    if len(w_shape) != 4 or tuple(w_shape[2:]) != (3, 3) or len(x_shape) != 4:
        return False
    co, ci = int(w_shape[0]), int(w_shape[1])
    if co % 32 or ci % 32:
        return False
    _, _, h, w = (int(v) for v in x_shape)
    # the kernels address each tensor with 32-bit byte offsets (< 2 GiB per launch); larger batches are launched in
    # batch chunks (_conv3x3_run), so the limit applies to one image
    return max(ci * h * w, co * h * w, 16 * ci * co) * 4 < 2 ** 31


# transformed-filter forms of a 3x3 weight: (C entry, floats per channel pair)
_FILTER_FORMS = {"f2": ("skp_conv3x3_filter_f32", 16),          # Winograd F(2x2,3x3)
                 "f4": ("skp_conv3x3_f4_filter_f32", 36),       # Winograd F(4x4,3x3)
                 "f4r": ("skp_conv3x3_f4r_filter_f32", 9),      # raw-filter form: the 9 taps in MFMA operand order
                 "s2": ("skp_conv3x3_s2_filter_f32", 9),        # stride-2 direct kernel
                 "s2w": ("skp_conv3x3_s2w_filter_f32", 81),     # stride-2 polyphase Winograd F(4x4,2x2), pad 0
                 "up2": ("skp_conv3x3_up2_filter_f32", 16)}     # up-sampling convolution: four 2x2 phase filters


def _filters(weight, form, backward=False):
    """Filter of a frozen weight in the layout of one kernel form (`_FILTER_FORMS`), channel roles swapped for the
    backward-data launch; built once per weight version and kept on the weight."""
    def build():
        w = _dev(weight.detach(), "weight")
        co, ci = w.shape[:2]
        name, per_pair = _FILTER_FORMS[form]
        U = torch.empty(per_pair * co * ci, device=w.device, dtype=torch.float32)
        if form in ("s2", "up2"):
            _launch(name, w, U, co, ci)
        elif form == "s2w":
            _launch(name, w, U, co, ci, 0)
        else:
            _launch(name, w, U, *((ci, co, 1) if backward else (co, ci, 0)))
        return U
    return cached(weight, ("filters", form, bool(backward)), (weight,), build)


# entries of bench.py, the tools and the kernel tests
def _wino_filters(weight, backward):
    return _filters(weight, "f2", backward)


def _wino4_filters(weight, backward):
    return _filters(weight, "f4", backward)


def _wino4r_filters(weight, backward):
    return _filters(weight, "f4r", backward)


def _conv3x3_raw(x, U, bias, cout, variant=0, split=True, residual=None, out=None):
    B, ci, H, W = x.shape
    y = out if out is not None else torch.empty(B, cout, H, W, device=x.device, dtype=torch.float32)
    ws = _workspace("skp_conv3x3_workspace", B, ci, cout, H, W, int(variant), device=x.device) if split else None
    _launch("skp_conv3x3_f32", x, U, bias, residual, y, ws, B, ci, cout, H, W, int(variant))
    return y


def _conv3x3_f4_raw(x, U, bias, cout, split=True, residual=None, out=None, stats=None):
    B, ci, H, W = x.shape
    y = out if out is not None else torch.empty(B, cout, H, W, device=x.device, dtype=torch.float32)
    if stats is not None:                            # unsplit launch that also leaves the output's block sums behind
        _launch("skp_conv3x3_f4_stats_f32", x, U, bias, residual, y, stats, B, ci, cout, H, W)
        return y
    ws = _workspace("skp_conv3x3_f4_workspace", B, ci, cout, H, W, device=x.device) if split else None
    _launch("skp_conv3x3_f4_f32", x, U, bias, residual, y, ws, B, ci, cout, H, W)
    return y


def _conv3x3_f4r_raw(x, R, bias, cout, residual=None, out=None):
    """Small-spatial form (csrc/skp_conv_wino4.hip, skp_wino4r_*): raw taps + in-lane filter transform, input transform in the workspace."""
    B, ci, H, W = x.shape
    y = out if out is not None else torch.empty(B, cout, H, W, device=x.device, dtype=torch.float32)
    ws = _workspace("skp_conv3x3_f4r_workspace", B, ci, cout, H, W, device=x.device)
    _launch("skp_conv3x3_f4r_f32", x, R, bias, residual, y, ws, B, ci, cout, H, W)
    return y


def conv3x3_f4r_ok(x_shape, cout) -> bool:
    """The raw-filter gate (the one statement `conv3x3_plan` consults, at most once per plan)."""
    b, ci, h, w = (int(v) for v in x_shape)
    return CONV3X3_MODE == "f4" and bool(N.lib().skp_conv3x3_f4r_ok(b, ci, int(cout), h, w))


# "f4": Winograd F(4x4,3x3) where the shape allows (H, W % 4 == 0), F(2x2,3x3) otherwise; "f2": F(2x2,3x3) only;
# "lib": library convolution everywhere (A/B runs and the consistency test).  Default f4.
CONV3X3_MODE = "f4"
GN_ONEPASS = True        # False (tests): producers leave block statistics behind even where the norm would not want them
_CONV3X3_OWN_ONLY = False


@contextlib.contextmanager
def conv3x3_own_kernels():
    """Inside the block `conv3x3_plan` drops its tile-count rule: every shape the Winograd kernels can run takes them.  The VAE
    decoder runs in it (ldm/fused.py): a one-image latency path, whose full-width launches pass the tile rule anyway (one 64^2
    latent is 256 tiles) -- only reduced-width trees at 8^2 differ, and those then stay on the HIP kernels instead of the library."""
    global _CONV3X3_OWN_ONLY
    prev, _CONV3X3_OWN_ONLY = _CONV3X3_OWN_ONLY, True
    try:
        yield
    finally:
        _CONV3X3_OWN_ONLY = prev


def _rows_per_launch(ci, co, H, W) -> int:
    """Batch rows one convolution launch takes under the kernels' 32-bit byte offsets (< 2 GiB per tensor)."""
    return max(1, (2 ** 31 - 1) // (max(ci, co) * H * W * 4))


# One stride-1 3x3 launch, decided: `site` / `route` = the ledger entry ("lib": the kernels are not wanted), `form` = the filter
# layout (a key of _FILTER_FORMS) and with it the kernel family, `rows` = batch rows per launch, `nblk` / `pixels` = statistics
# blocks per image the launch leaves behind (0: none) and pixels per block, `fold` = a GroupNorm fold was asked for and the
# folded kernel serves every chunk, the tail included.
ConvPlan = namedtuple("ConvPlan", "site route form rows nblk pixels fold")


def conv3x3_plan(x_shape, w_shape, *, backward=False, want_stats=False, gn_fold=None, forced=False) -> ConvPlan:
    """Every decision about the 3x3 / stride 1 / pad 1 convolution of x [B,Cin,H,W] with a filter of shape `w_shape` [Cout,Cin,3,3]
    (backward-data: x = dy, channel roles already swapped), from the shapes and the module switches alone: pure host code, each
    library query asked at most once and only where its answer can matter, nothing kept between calls (skp_tune_set and the
    switches change the answers).  `want_stats`: True = for the GroupNorm that follows, "always" = whatever follows (callers that
    read the blocks themselves); `gn_fold`: the groups of a GroupNorm(+SiLU) to apply in the patch load; `forced`: ops.conv3x3."""
    site = "conv3x3.bwd_data" if backward else "conv3x3"
    if len(x_shape) != 4 or len(w_shape) != 4:
        return ConvPlan(site, "lib", None, 0, 0, 256, False)
    (b, xci, h, w), co, ci, lib = (int(v) for v in x_shape), int(w_shape[0]), int(w_shape[1]), N.lib()
    rows = min(b, _rows_per_launch(xci, co, h, w))
    # F(4x4) serves: >= 32 tiles (one tile block of the transformed-filter kernels), or fewer on the raw-filter form where the
    # library routes it (>= 1280 channels on both sides: the 8^2 layers of a 1- or 2-row step -- config 3's per-rank shape -- ran on
    # the library at 120 us per call incl. its layout transposes; the raw-filter kernel takes the same 55 us as at 8 rows)
    f4 = CONV3X3_MODE == "f4" and h % 4 == 0 and w % 4 == 0 and co % 16 == 0 and ci % 16 == 0 and 36 * co * ci * 4 < 2 ** 31
    raw = None
    if f4 and b * (h // 4) * (w // 4) < 32:
        f4 = raw = conv3x3_f4r_ok(x_shape, co)
    # wanted: supported AND enough tiles to fill the MFMA column blocks (layers with few workgroups are split over input channels
    # inside the library call, so the channel counts do not matter here); own kernels only / forced: no tile rule
    supported = conv3x3_supported(x_shape, w_shape)
    wanted = supported and (forced or (CONV3X3_MODE != "lib" and (_CONV3X3_OWN_ONLY or f4 or b * ((h + 1) // 2) * ((w + 1) // 2) >= 128)))
    nblk, fold = 0, False
    if f4 and supported and not backward:
        if gn_fold is not None:      # the norm's kernels take x, and the folded kernel takes the full chunks and the tail chunk
            fold = (xci % gn_fold == 0 and (h * w) % 4 == 0 and b * gn_fold <= 65535 and bool(lib.skp_conv3x3_f4_gn_ok(rows, xci, co, h, w))
                    and (b % rows == 0 or bool(lib.skp_conv3x3_f4_gn_ok(b % rows, xci, co, h, w))))
        # statistics: one launch for the whole batch, and only where the GroupNorm that follows does not hold its rows in registers
        # anyway (the one-pass form computes exact statistics from the row it has loaded; the library says which)
        if want_stats and rows == b and (want_stats == "always" or not (
                GN_ONEPASS and co % 32 == 0 and lib.skp_group_norm_onepass_ok(1, co, 32, h * w))):
            nblk = int(lib.skp_conv3x3_f4_stats_blocks(b, xci, co, h, w))
    # the raw-filter form leaves no statistics and folds no norm; asked (if not above) only of a plain launch that will run: a plan
    # made with `gn_fold` is about the folded launch alone, and no caller runs it without its `fold`
    raw = f4 and not (nblk or fold) and (raw if raw is not None else wanted and gn_fold is None and conv3x3_f4r_ok(x_shape, co))
    form = "f4r" if raw else "f4" if f4 else "f2"
    # (a batch launched in chunks is named by its full chunks)
    route = "lib" if not wanted else "wino4_raw" if form == "f4r" else routes.wino4_form(co, rows, h, w) if f4 else "wino2"
    return ConvPlan(site, route, form, rows, nblk, 256, fold)


# the earlier predicates, as views of the plan (bench.py, tools/, ldm/fused.py and the tests ask them)
def conv3x3_f4_ok(x_shape, w_shape):
    return conv3x3_plan(x_shape, w_shape).form in ("f4", "f4r")


def conv3x3_wanted(x_shape, w_shape):
    return conv3x3_plan(x_shape, w_shape).route != "lib"


def conv3x3_stats_blocks(x_shape, w_shape) -> int:
    """256-pixel blocks per image if the forward convolution of this shape can leave output statistics behind, else 0."""
    return conv3x3_plan(x_shape, w_shape, want_stats="always").nblk


def _leave_blocks(y, stats, nblk, pixels):
    """The one writer of `y._skp_blocks` = (block sums [B,C,nblk,2], blocks per image, pixels per block), which `_blocks` reads for
    the norm that consumes y (the same tensor object only).  -> y"""
    if stats is not None:
        y._skp_blocks = (stats, nblk, pixels)
    return y


def _rows(t, b0, b1):
    """Rows b0..b1 of t; t itself where that is all of it (the one-launch path makes no views)."""
    return t if t is None or (b0 == 0 and b1 == t.shape[0]) else t[b0:b1]


def _conv3x3_run(who, x, weight, bias, residual, plan: ConvPlan, stats=None, fold=None):
    """Executes `plan` (of `conv3x3_plan` for these operands): one ledger note, one filter, one loop over the batch chunks.
    `stats` [B,Cout,plan.nblk,2]: the launch leaves its block sums there; `fold` = (GroupNorm, offset or None): the folded kernel.
    What the plan does not serve is refused here, before anything is launched."""
    backward = plan.site == "conv3x3.bwd_data"
    B, ci, H, W = x.shape
    cout = int(weight.shape[1] if backward else weight.shape[0])
    bad = (f"the Winograd kernels are not planned for x {tuple(x.shape)}, weight {tuple(weight.shape)}" if plan.route == "lib" else
           f"block statistics on a plan of form {plan.form} that leaves none" if stats is not None and not (plan.form == "f4" and plan.nblk) else
           f"statistics of shape {tuple(stats.shape)}, the plan leaves {(B, cout, plan.nblk, 2)}"
           if stats is not None and tuple(stats.shape) != (B, cout, plan.nblk, 2) else
           f"residual of shape {tuple(residual.shape)}, the output has {(B, cout, H, W)}"
           if residual is not None and tuple(residual.shape) != (B, cout, H, W) else
           "the folded kernel does not serve this launch (ask conv3x3_gn_fold_ok first)" if fold is not None and not plan.fold else None)
    if bad:
        raise RuntimeError(f"{who}: {bad}")
    routes.note(plan.site, plan.route)
    coef = _gn_fold_coef(x, *fold) if fold is not None else None
    U = _filters(weight, plan.form, backward)
    y = torch.empty(B, cout, H, W, device=x.device, dtype=torch.float32)
    for b0 in range(0, B, plan.rows):
        b1 = min(B, b0 + plan.rows)
        xs, rs, ys = _rows(x, b0, b1), _rows(residual, b0, b1), _rows(y, b0, b1)
        if coef is not None:
            _launch("skp_conv3x3_f4_gn_f32", xs, U, bias, rs, ys, _rows(stats, b0, b1), coef[b0:b1], b1 - b0, ci, cout, H, W)
        elif plan.form == "f4r":                         # small spatial size, many channels: raw-filter form
            _conv3x3_f4r_raw(xs, U, bias, cout, residual=rs, out=ys)
        elif plan.form == "f4":
            _conv3x3_f4_raw(xs, U, bias, cout, residual=rs, out=ys, stats=stats)
        else:
            _conv3x3_raw(xs, U, bias, cout, residual=rs, out=ys)
    return y


class Conv3x3Fn(torch.autograd.Function):
    """y = conv2d(x, weight, bias, stride 1, padding 1) (+ residual) with frozen weight/bias, as `plan` says; dx is the same
    kernel run with the rotated, transposed filter; the residual's gradient is dy."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, stats, plan):
        ctx.weight = weight
        return _conv3x3_run("conv3x3", _dev(x, "x"), weight, bias, _dev(residual, "residual") if residual is not None else None, plan, stats)

    @staticmethod
    def backward(ctx, dy):
        dx = None
        if ctx.needs_input_grad[0]:
            w = ctx.weight
            co, ci = w.shape[:2]
            plan = conv3x3_plan(dy.shape, (ci, co, 3, 3), backward=True)
            if plan.route != "lib":
                dx = _conv3x3_run("conv3x3 backward", _dev(dy, "dy"), w, None, None, plan)
            else:       # too few tiles for these kernels: library backward-data
                routes.note("conv3x3.bwd_data", "lib")
                dx = torch.nn.grad.conv2d_input((dy.shape[0], ci, dy.shape[2], dy.shape[3]), w, dy, padding=1)
        return dx, None, None, (dy if ctx.needs_input_grad[3] else None), None, None


def conv3x3(x, weight, bias=None, residual=None):
    plan = conv3x3_plan(x.shape, weight.shape, forced=True)
    if plan.route == "lib":
        raise ValueError(f"conv3x3: unsupported shape x {tuple(x.shape)} w {tuple(weight.shape)}")
    if weight.requires_grad or (bias is not None and bias.requires_grad):
        raise ValueError("conv3x3: the Winograd kernels serve FROZEN weights only (no weight/bias gradient)")
    return Conv3x3Fn.apply(x, weight, bias, residual, None, plan)


def conv3x3_auto(x, weight, bias=None, residual=None, want_stats=False):
    """The frozen blocks' 3x3 convolution (+ bias + residual): Winograd kernel where it is wanted, library
    convolution (and the fused bias+residual pass) otherwise."""
    frozen = not (weight.requires_grad or (bias is not None and bias.requires_grad))     # the kernels give no dW / db
    own = frozen and x.is_cuda and x.dtype == torch.float32
    plan = conv3x3_plan(x.shape, weight.shape, want_stats=want_stats) if own else None
    if own and plan.route != "lib":
        stats = torch.empty(x.shape[0], weight.shape[0], plan.nblk, 2, device=x.device, dtype=torch.float32) if plan.nblk else None
        return _leave_blocks(Conv3x3Fn.apply(x, weight, bias, residual, stats, plan), stats, plan.nblk, plan.pixels)
    if own and residual is None and CONV3X3_MODE != "lib" and weight.shape[1] <= 4 and x.shape[3] % 2 == 0:
        if not (torch.is_grad_enabled() and x.requires_grad):
            return conv3x3_small(x, weight, bias, want_stats=want_stats)   # conv_in layers: output-bandwidth bound, own VALU kernel
        if conv_in_grad_ok(x, weight):           # the latent takes a gradient (keypoint guidance): its adjoint is a small-output conv
            return ConvInFn.apply(x, weight, bias)       # (no block statistics: the norm that follows makes its own)
    routes.note("conv_out" if weight.shape[0] <= 8 else "conv3x3", "lib")     # (<= 8 output channels = a conv_out, by the rule above)
    if residual is None:
        return torch.nn.functional.conv2d(x, weight, bias, padding=1)
    y = torch.nn.functional.conv2d(x, weight, None, padding=1)
    if bias is not None and y.is_cuda and y.dtype == torch.float32 and (y.shape[2] * y.shape[3]) % 4 == 0:
        return add_bias_residual(residual, y, bias)
    return (y + bias[None, :, None, None] if bias is not None else y) + residual


# GroupNorm(+offset)+SiLU folded into the consuming Winograd convolution (forward only, single output-channel group):
# saves the norm's apply pass (one read + one write of the activation).
def conv3x3_gn_fold_ok(x, norm: torch.nn.GroupNorm, weight, *others) -> bool:
    """`others`: every further tensor the folded call will read (offset, bias, residual).  The folded kernel is forward
    only: with autograd on, ANY operand that requires a gradient (input, norm affine, weight, offset, bias, residual) sends
    the block down the differentiable route.  The shape verdict is that of the plan `conv3x3_gn_silu` will execute."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4) or weight.requires_grad:
        return False
    if torch.is_grad_enabled() and any(t_ is not None and t_.requires_grad
                                       for t_ in (x, weight, norm.weight, norm.bias, *others)):
        return False
    return conv3x3_plan(x.shape, weight.shape, gn_fold=norm.num_groups).fold


def _gn_fold_coef(x, norm: torch.nn.GroupNorm, off):
    """-> [B,C,2], the per-(row, channel) scale and shift of GroupNorm(x + off) that the folded convolution applies in its patch
    load.  Statistics come from x's producer when it left block sums behind."""
    B, C, H, W = x.shape
    G = norm.num_groups
    off_c = _dev(off.reshape(B, C), "off") if off is not None else None
    mean = torch.empty(B, G, device=x.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    coef = torch.empty(B, C, 2, device=x.device, dtype=torch.float32)
    blocks = _blocks(x)
    routes.note("group_norm", "gn_fold")
    routes.note("group_norm.stats", "producer_blocks" if blocks is not None else "own_pass")
    own = blocks is None                             # the kernel reads x and a scratch buffer, or the producer's blocks
    bs, nblk, pix = (None, 0, 0) if own else blocks
    _launch("skp_group_norm_coef_f32", x if own else None, off_c, norm.weight, norm.bias, mean, rstd, coef, bs, nblk, pix,
            _gn_scratch(B, G, x.device) if own else None, B, C, G, H * W, float(norm.eps))
    return coef


@torch.no_grad()
def conv3x3_gn_silu(x, norm: torch.nn.GroupNorm, weight, off=None, bias=None, residual=None, want_stats=False):
    """conv3x3(silu(GroupNorm(x + off))) (+ bias) (+ residual) with the normalisation applied in the convolution's patch load
    (csrc/skp_conv_wino4.hip, GNF kernels): the plan's folded form, on the executor of every stride-1 route."""
    x = _dev(x, "x")
    bias = _dev(bias, "bias") if bias is not None else None
    residual = _dev(residual, "residual") if residual is not None else None
    plan = conv3x3_plan(x.shape, weight.shape, want_stats=want_stats, gn_fold=norm.num_groups)
    stats = torch.empty(x.shape[0], weight.shape[0], plan.nblk, 2, device=x.device, dtype=torch.float32) if plan.nblk else None
    y = _conv3x3_run("conv3x3_gn_silu", x, weight, bias, residual, plan, stats, fold=(norm, off))
    return _leave_blocks(y, stats, plan.nblk, plan.pixels)


def conv3x3_small(x, weight, bias=None, want_stats=False):
    """3x3 / stride 1 / padding 1 convolution with <= 4 input channels (the conv_in layers), forward only.  `want_stats`: where the
    kernel serves it (the VAE's 3 -> 128 at image resolution) the output carries its block statistics for the GroupNorm that
    follows (`y._skp_blocks`, consumed by group_norm_silu / conv3x3_gn_silu): no separate pass over the 1 GB activation."""
    x, w = _dev(x.detach(), "x"), _dev(weight.detach(), "weight")
    routes.note("conv_in", "small")
    B, ci, H, W = x.shape
    y = torch.empty(B, w.shape[0], H, W, device=x.device, dtype=torch.float32)
    bb = _dev(bias.detach(), "bias") if bias is not None else None
    nblk = int(N.lib().skp_conv3x3_small_stats_blocks(B, ci, w.shape[0], H, W)) if want_stats else 0
    if nblk:
        stats = torch.empty(B, w.shape[0], nblk, 2, device=x.device, dtype=torch.float32)
        _launch("skp_conv3x3_small_stats_f32", x, w, bb, y, stats, B, ci, w.shape[0], H, W)
        return _leave_blocks(y, stats, nblk, 512)
    _launch("skp_conv3x3_small_f32", x, w, bb, y, B, ci, w.shape[0], H, W)
    return y


def conv3x3_small_out(x, weight, bias=None, image=False):
    """3x3 / stride 1 / padding 1 convolution to <= 4 output channels (the VAE decoder's conv_out), forward only; `image`: the
    epilogue writes clamp(y / 2 + 0.5, 0, 1), the [-1, 1] -> [0, 1] map of `ptp_utils.latent2image`, instead of y."""
    x, w = _dev(x.detach(), "x"), _dev(weight.detach(), "weight")
    routes.note("conv_out", "small_out")
    B, ci, H, W = x.shape
    y = torch.empty(B, w.shape[0], H, W, device=x.device, dtype=torch.float32)
    bb = _dev(bias.detach(), "bias") if bias is not None else None
    _launch("skp_conv3x3_small_out_f32", x, w, bb, y, B, ci, w.shape[0], H, W, bool(image))
    return y


def conv3x3_small_out_ok(x, weight) -> bool:
    """Shapes `conv3x3_small_out` takes: Cin % 16 == 0, Cout <= 4, even width, 3x3 taps."""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and int(weight.shape[1]) == x.shape[1]
            and _small_out_shape_ok(x.shape[0], x.shape[1], weight.shape[0], x.shape[3], weight.shape[2:]))


def _small_out_shape_ok(B, ci, co, W, taps) -> bool:
    return tuple(taps) == (3, 3) and CONV3X3_MODE != "lib" and ci % 16 == 0 and co <= 4 and W % 2 == 0 and B <= 65535


def conv_in_grad_ok(x, weight) -> bool:
    """Whether the input gradient of `conv3x3_small(x, weight)` -- a 3x3 convolution of dy [B,Cout,H,W] to <= 4 channels with the
    flipped, transposed filter [Cin,Cout,3,3] -- is a shape `conv3x3_small_out` takes."""
    return x.dim() == 4 and _small_out_shape_ok(x.shape[0], weight.shape[0], weight.shape[1], x.shape[3], weight.shape[2:])


class ConvInFn(torch.autograd.Function):
    """`conv3x3_small` for an input that takes a gradient (the latent under keypoint guidance): the forward is that kernel, the
    backward the small-output kernel on dy with the flipped, transposed filter, made once per frozen weight.  No weight or bias
    gradient (frozen blocks only)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.weight = weight
        return conv3x3_small(x, weight, bias)

    @staticmethod
    def backward(ctx, dy):
        w = ctx.weight
        wt = cached(w, "conv_in_bwd", [w], lambda: w.detach().flip(2, 3).transpose(0, 1).contiguous())
        dy = _dev(dy, "dy")
        B, co, H, W = dy.shape
        routes.note("conv_in.bwd_data", "small_out")
        dx = torch.empty(B, wt.shape[0], H, W, device=dy.device, dtype=torch.float32)
        _launch("skp_conv3x3_small_out_f32", dy, wt, None, dx, B, co, wt.shape[0], H, W, False)
        return dx, None, None


# ---------------------------------------------------------------------------------------------------------
# nearest 2x up-sampling + 3x3 convolution (Upsample2D) without the up-sampled tensor; forward only (sampling runs under no_grad)
# ---------------------------------------------------------------------------------------------------------
def up2_fold_filter(weight):
    """The four 2x2 phase filters of `conv2d(interpolate(x, 2x, nearest), weight, padding=1)`: F [2, 2, Co, Ci, 2, 2] with
    y[:, :, 2i+a, 2j+c] = sum_{ci,dr,dc} F[a, c, :, ci, dr, dc] * x[:, ci, i+a-1+dr, j+c-1+dc]   (out of range = 0).
    Row phase 0 sees rows {i-1: w0, i: w1+w2}, phase 1 {i: w0+w1, i+1: w2}; columns fold the same way.  Plain torch in the
    weight's own dtype and device: the restatement of csrc/skp_conv_up2.hip's filter fold that the tests compare against."""
    m = torch.tensor([[[1, 0, 0], [0, 1, 1]], [[1, 1, 0], [0, 0, 1]]], dtype=weight.dtype, device=weight.device)   # [phase][tap][r]
    return torch.einsum("adr,oirs,ces->acoide", m, weight, m)


_UP2_IN_UNET = False


@contextlib.contextmanager
def up2_in_unet(on: bool = True):
    """Inside the block the UNet's Upsample2D layers may take `conv3x3_up2` (the sampling loop of
    ptp_utils.text2image_ldm_stable); outside -- the default -- they run interpolate + their own convolution, as the optimisation
    path always has."""
    global _UP2_IN_UNET
    prev, _UP2_IN_UNET = _UP2_IN_UNET, bool(on)
    try:
        yield
    finally:
        _UP2_IN_UNET = prev


def up2_in_unet_enabled() -> bool:
    return _UP2_IN_UNET


def conv3x3_up2(x, weight, bias=None):
    """y = conv2d(interpolate(x, scale 2, nearest), weight, bias, padding=1) for a frozen weight, forward only: the polyphase
    kernel on the low-resolution input where the library's gate (`skp_conv3x3_up2_ok`) takes the shape, else interpolate + the
    Winograd route of `conv3x3_auto`.  Either way the choice is noted at the `upsample_conv` site."""
    if weight.requires_grad or (bias is not None and bias.requires_grad):
        raise RuntimeError("conv3x3_up2: frozen weights only")
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError("conv3x3_up2: forward only (no input gradient); run it under torch.no_grad()")
    x = _dev(x.detach(), "x")
    B, ci, H, W = x.shape
    co = int(weight.shape[0])
    if tuple(weight.shape[1:]) != (ci, 3, 3):
        raise RuntimeError(f"conv3x3_up2: weight {tuple(weight.shape)} does not fit x {tuple(x.shape)}")
    if CONV3X3_MODE != "lib" and N.lib().skp_conv3x3_up2_ok(B, ci, co, H, W):
        routes.note("upsample_conv", "up2_poly")
        U = _filters(weight, "up2")
        y = torch.empty(B, co, 2 * H, 2 * W, device=x.device, dtype=torch.float32)
        bb = _dev(bias.detach(), "bias") if bias is not None else None
        _launch("skp_conv3x3_up2_f32", x, U, bb, y, B, ci, co, H, W)
        return y
    routes.note("upsample_conv", "interp_wino")
    return conv3x3_auto(torch.nn.functional.interpolate(x, scale_factor=2.0, mode="nearest"), weight, bias)


def axpby(x, z, a: float, b: float):
    """a * x + b * z in one pass (the DDIM update with host-computed coefficients; csrc/skp_sampler_step.hip)."""
    x, z = _dev(x, "x"), _dev(z, "z")
    if x.shape != z.shape:
        raise RuntimeError("axpby: shapes differ")
    y = torch.empty_like(x)
    _launch("skp_axpby_f32", x, z, y, x.numel(), float(a), float(b))
    return y


DDIM_PREDICTION = {"epsilon": 0, "v_prediction": 1, "sample": 2}


def _step_args(who, x, m_c, m_u, x0_prev, noise, prediction, copies, out):
    """What `ddim_step` and `sampler_step` share -> (x, m_c, m_u, noise, prediction as 0 | 1 | 2, x.numel(), out): the inputs as
    contiguous float32 device tensors of one shape, and `out` allocated or validated."""
    x, m_c = _dev(x, "x"), _dev(m_c, "m_c")
    m_u = _dev(m_u, "m_u") if m_u is not None else None
    noise = _dev(noise, "noise") if noise is not None else None
    if x0_prev is not None and not (x0_prev.is_cuda and x0_prev.dtype == torch.float32 and x0_prev.is_contiguous()):
        raise RuntimeError(f"{who}: `x0_prev` must be a contiguous float32 device tensor")
    if any(t is not None and t.shape != x.shape for t in (m_c, m_u, x0_prev, noise)):
        raise RuntimeError(f"{who}: shapes differ")
    pred = DDIM_PREDICTION.get(prediction, prediction)
    if pred not in (0, 1, 2) or copies not in (1, 2):
        raise ValueError(f"{who}: prediction {prediction!r} / copies {copies!r}")
    n = x.numel()
    if out is None:
        out = torch.empty((copies * x.shape[0],) + tuple(x.shape[1:]) if x.dim() else (copies,), device=x.device, dtype=torch.float32)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == copies * n):
        raise RuntimeError(f"{who}: `out` must be a contiguous float32 device tensor of copies * x.numel() elements")
    return x, m_c, m_u, noise, int(pred), n, out


def ddim_step(x, m_c, m_u=None, *, sa: float, sb: float, pa: float, pb: float, guidance: float = 1.0, prediction="epsilon",
              clip: bool = False, copies: int = 1, out=None):
    """The guided DDIM update in one pass (csrc/skp_sampler_step.hip, formula in include/skp.h): m = m_u + guidance (m_c - m_u) when
    `m_u` is given, else m_c; (x0, eps) from (x, m) by `prediction` ("epsilon" | "v_prediction" | "sample" or 0 | 1 | 2); x0
    clamped to [-1, 1] when `clip`; y = pa x0 + pb eps.  -> y shaped like x, or with `copies=2` like torch.cat([x, x]): the result
    twice along dim 0.  `out`: a contiguous float32 tensor of copies * x.numel() elements to write into; it may be x itself, or
    (copies = 2) a buffer whose first half x is."""
    x, m_c, m_u, _, pred, n, out = _step_args("ddim_step", x, m_c, m_u, None, None, prediction, copies, out)
    _launch("skp_ddim_step_f32", x, m_c, m_u, out, n, copies, float(guidance), pred, float(sa), float(sb), float(pa), float(pb),
            bool(clip))
    return out


def sampler_step(x, m_c, m_u=None, *, x0_prev=None, noise=None, coef, guidance: float = 1.0, prediction="epsilon",
                 clip: bool = False, copies: int = 1, out=None, x0_out=None, grad=None, grad_scale=None):
    """One step of a sampler of ldm/samplers.py in one pass (csrc/skp_sampler_step.hip, formula in include/skp.h): the guidance mix,
    (x0, eps) by `prediction` and the clamp as in `ddim_step`, then y = cx x + c0 x0 + ce eps + c1 x0_prev + cn noise with
    `coef` = (sa, sb, cx, c0, ce, c1, cn) (a `samplers.StepCoef`).  -> y shaped like x, or with `copies=2` like torch.cat([x, x]).
    `x0_prev` / `noise`: shaped like x; each may be None when its coefficient is 0.  `out`: as in `ddim_step` (it may be x, or
    a doubled buffer whose first half x is).  `x0_out`: a contiguous float32 tensor shaped like x that receives the clamped x0; it
    may be `x0_prev` itself (the history updated in place).
    `grad` (shaped like x) with `grad_scale` (float32 [rows] on the device, rows = x.shape[0]): the gradient term of keypoint
    guidance, eps += s g and x0 -= (sb / sa) s g before the clamp (skp_sampler_step_kp_f32, include/skp_keypoints.h); the scales
    are read by the kernel, never by the host."""
    x, m_c, m_u, noise, pred, n, out = _step_args("sampler_step", x, m_c, m_u, x0_prev, noise, prediction, copies, out)
    sa, sb, cx, c0, ce, c1, cn = (float(v) for v in coef)
    if (c1 != 0.0 and x0_prev is None) or (cn != 0.0 and noise is None):
        raise ValueError("sampler_step: a nonzero c1 needs `x0_prev`, a nonzero cn needs `noise`")
    if x0_out is not None and not (x0_out.is_cuda and x0_out.dtype == torch.float32 and x0_out.is_contiguous()
                                   and x0_out.numel() == n):
        raise RuntimeError("sampler_step: `x0_out` must be a contiguous float32 device tensor of x.numel() elements")
    if (grad is None) != (grad_scale is None):
        raise ValueError("sampler_step: `grad` and `grad_scale` go together")
    if grad is not None:
        grad, grad_scale = _dev(grad, "grad"), _dev(grad_scale, "grad_scale")
        rows = x.shape[0] if x.dim() else 1
        if grad.shape != x.shape or tuple(grad_scale.shape) != (rows,):
            raise RuntimeError(f"sampler_step: `grad` must be shaped like x and `grad_scale` be [{rows}]")
        _launch("skp_sampler_step_kp_f32", x, m_c, m_u, x0_prev, noise, out, x0_out, n, copies, float(guidance), pred, sa, sb, cx, c0,
                ce, c1, cn, bool(clip), grad, grad_scale, rows)
        return out
    _launch("skp_sampler_step_f32", x, m_c, m_u, x0_prev, noise, out, x0_out, n, copies, float(guidance), pred, sa, sb, cx, c0, ce,
            c1, cn, bool(clip))
    return out


STEP_ROW = 8                   # SKP_STEP_ROW of include/skp_sampler_graph.h: sa sb cx c0 ce c1 cn guidance


def _step_row(who, table, step, steps):
    """The device row of the `*_dev` steps, checked on the host as far as the host can: `table` float32 [rows, STEP_ROW] and
    contiguous, `step` ONE int32, both on the device, and at least `steps` rows -- the count of the plan the counter walks, which
    is also what the kernel holds the counter to.  -> int(steps)."""
    steps = int(steps)
    if not (isinstance(table, torch.Tensor) and table.is_cuda and table.dtype == torch.float32 and table.is_contiguous()
            and table.dim() == 2 and table.shape[1] == STEP_ROW):
        raise RuntimeError(f"{who}: `table` must be a contiguous float32 device tensor [steps, {STEP_ROW}]")
    if not (isinstance(step, torch.Tensor) and step.is_cuda and step.dtype == torch.int32 and step.numel() == 1):
        raise RuntimeError(f"{who}: `step` must be one int32 on the device")
    if steps < 1 or table.shape[0] < steps:
        raise ValueError(f"{who}: a table of {table.shape[0]} rows for a plan of {steps} steps")
    return steps


def step_advance(step):
    """*step += 1 on the device (skp_step_advance): the last launch of a recorded sampling step."""
    if not (isinstance(step, torch.Tensor) and step.is_cuda and step.dtype == torch.int32 and step.numel() == 1):
        raise RuntimeError("step_advance: `step` must be one int32 on the device")
    _launch("skp_step_advance", step)
    return step


def axpby_dev(x, z, *, table, step, steps, out=None):
    """`axpby` with a = cx and b = ce of row *step of `table` (skp_axpby_dev_f32).  `out`: may be x or z."""
    x, z = _dev(x, "x"), _dev(z, "z")
    if x.shape != z.shape:
        raise RuntimeError("axpby_dev: shapes differ")
    steps = _step_row("axpby_dev", table, step, steps)
    if out is None:
        out = torch.empty_like(x)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == x.numel()):
        raise RuntimeError("axpby_dev: `out` must be a contiguous float32 device tensor of x.numel() elements")
    _launch("skp_axpby_dev_f32", x, z, out, x.numel(), table, step, steps)
    return out


def ddim_step_dev(x, m_c, m_u=None, *, table, step, steps, prediction="epsilon", clip: bool = False, copies: int = 1, out=None):
    """`ddim_step` with (sa, sb, pa, pb, guidance) = columns (0, 1, 3, 4, 7) of row *step of `table` (skp_ddim_step_dev_f32): for
    equal floats, the bits of `ddim_step`."""
    x, m_c, m_u, _, pred, n, out = _step_args("ddim_step_dev", x, m_c, m_u, None, None, prediction, copies, out)
    steps = _step_row("ddim_step_dev", table, step, steps)
    _launch("skp_ddim_step_dev_f32", x, m_c, m_u, out, n, copies, pred, bool(clip), table, step, steps)
    return out


def sampler_step_dev(x, m_c, m_u=None, *, x0_prev=None, noise=None, table, step, steps, prediction="epsilon", clip: bool = False,
                     copies: int = 1, out=None, x0_out=None, grad=None, grad_scale=None):
    """`sampler_step` with its row (sa, sb, cx, c0, ce, c1, cn, guidance) read by the kernel from row *step of `table`
    (skp_sampler_step_dev_f32 / skp_sampler_step_kp_dev_f32, include/skp_sampler_graph.h): for equal floats, the bits of
    `sampler_step`.  `noise`: ALL steps' gaussians, [>= steps, *x.shape]; the kernel takes row *step.  `x0_prev` / `noise` are read
    only on steps whose c1 / cn is not 0, whatever they hold on the others; None says that no row has a nonzero coefficient.
    Everything else as for `sampler_step`."""
    x, m_c, m_u, _, pred, n, out = _step_args("sampler_step_dev", x, m_c, m_u, x0_prev, None, prediction, copies, out)
    steps = _step_row("sampler_step_dev", table, step, steps)
    if noise is not None:
        if not (noise.is_cuda and noise.dtype == torch.float32 and noise.is_contiguous()):
            raise RuntimeError("sampler_step_dev: `noise` must be a contiguous float32 device tensor")
        if noise.dim() != x.dim() + 1 or noise.shape[1:] != x.shape or noise.shape[0] < steps:
            raise ValueError(f"sampler_step_dev: noise {tuple(noise.shape)} is not [>= {steps}, {', '.join(map(str, x.shape))}]")
    if x0_out is not None and not (x0_out.is_cuda and x0_out.dtype == torch.float32 and x0_out.is_contiguous()
                                   and x0_out.numel() == n):
        raise RuntimeError("sampler_step_dev: `x0_out` must be a contiguous float32 device tensor of x.numel() elements")
    if (grad is None) != (grad_scale is None):
        raise ValueError("sampler_step_dev: `grad` and `grad_scale` go together")
    if grad is not None:
        grad, grad_scale = _dev(grad, "grad"), _dev(grad_scale, "grad_scale")
        rows = x.shape[0] if x.dim() else 1
        if grad.shape != x.shape or tuple(grad_scale.shape) != (rows,):
            raise RuntimeError(f"sampler_step_dev: `grad` must be shaped like x and `grad_scale` be [{rows}]")
        _launch("skp_sampler_step_kp_dev_f32", x, m_c, m_u, x0_prev, noise, out, x0_out, n, copies, pred, bool(clip), table, step,
                steps, grad, grad_scale, rows)
        return out
    _launch("skp_sampler_step_dev_f32", x, m_c, m_u, x0_prev, noise, out, x0_out, n, copies, pred, bool(clip), table, step, steps)
    return out


def image_u8_nhwc(x):
    """float [B,3,H,W] in [0, 1] -> uint8 [B,H,W,3] = (x.permute(0, 2, 3, 1) * 255) truncated, on the device
    (csrc/skp_conv_out.hip; `ptp_utils.latent2image`)."""
    x = _dev(x.detach(), "x")
    if x.dim() != 4 or x.shape[1] != 3:
        raise RuntimeError(f"image_u8_nhwc: expected [B,3,H,W], got {tuple(x.shape)}")
    B, _, H, W = x.shape
    y = torch.empty(B, H, W, 3, device=x.device, dtype=torch.uint8)
    _launch("skp_image_u8_nhwc_f32", x, y, B, H, W)
    return y


def map_range(maps):
    """float [..., h, w] -> [N, 2] = (min, max) of each of the N = prod(leading dims) maps, NaN ignored, (0, 0) for a map of only
    NaN; exact, whatever the split over workgroups (csrc/skp_overlay.hip, include/skp_overlay.h)."""
    maps = _dev(maps.detach(), "maps")
    if maps.dim() < 2 or maps.numel() == 0:
        raise RuntimeError(f"map_range: expected [..., h, w] with elements, got {tuple(maps.shape)}")
    plane = maps.shape[-2] * maps.shape[-1]
    n = maps.numel() // plane
    out = torch.empty(n, 2, device=maps.device, dtype=torch.float32)
    ws = _workspace("skp_map_range_workspace", n, plane, device=maps.device)
    _launch("skp_map_range_f32", maps, out, ws, n, plane)
    return out


def locate(maps, mode: int = 0, distance: float = 5.0):
    """float [..., h, w] -> (loc float32 [N,2] = (row, col) in pixels, flat int32 [N]) of each of the N = prod(leading dims) maps:
    the first maximal element, and the location `mode` makes of it -- 0: its centre; 1: the intensity-weighted mean over the
    pixels within `distance` of it (-1: the whole map).  One pass, `maps` is only read; the same bits on every call
    (csrc/skp_locate.hip; the definition is in include/skp_locate.h and, in torch, `eval.locate_formula`)."""
    maps = _dev(maps.detach(), "maps")
    if maps.dim() < 2 or maps.numel() == 0:
        raise RuntimeError(f"locate: expected [..., h, w] with elements, got {tuple(maps.shape)}")
    h, w = maps.shape[-2:]
    n = maps.numel() // (h * w)
    loc = torch.empty(n, 2, device=maps.device, dtype=torch.float32)
    flat = torch.empty(n, device=maps.device, dtype=torch.int32)
    ws = _workspace("skp_locate_workspace", n, h, w, device=maps.device)
    _launch("skp_locate_f32", maps, n, h, w, int(mode), float(distance), loc, flat, ws, 0 if ws is None else 4 * ws.numel())
    return loc, flat


def overlay_u8(img, maps=None, rng=None, lut=None, alpha: float = 0.7, pts=None, colors=None, glyphs=None, radius: float = 9.0,
               ring: float = 1.5, labels: bool = True, out=None, origin=(0, 0), cols: int = 1, gap: int = 0):
    """Images under an optional colour-mapped heat map and numbered markers, as bytes in a canvas (csrc/skp_overlay.hip; the
    per-pixel formula is in include/skp_overlay.h and, in torch, `visualize.overlay_formula`).  img [B,3,H,W]; maps [B,S,S] with
    rng [B,2] (`map_range`) and lut [L,3]; pts [B,K,2] (row, col) in image fractions with colors [K,3] and glyphs uint8 [10,7].
    `out`: a uint8 canvas [h, w, 3] on the device that image b is written into at origin + (b // cols, b % cols) * (H + gap, W + gap);
    None allocates [B,H,W,3], one image per tile (cols = 1, gap = 0).  Returns the canvas."""
    img = _dev(img.detach(), "img")
    if img.dim() != 4 or img.shape[1] != 3:
        raise RuntimeError(f"overlay_u8: expected [B,3,H,W], got {tuple(img.shape)}")
    B, _, H, W = img.shape
    S = L = K = 0
    if maps is not None:
        maps, rng, lut = _dev(maps.detach(), "maps"), _dev(rng.detach(), "rng"), _dev(lut.detach(), "lut")
        if maps.dim() != 3 or maps.shape[0] != B or maps.shape[1] != maps.shape[2] or tuple(rng.shape) != (B, 2) or lut.dim() != 2 \
                or lut.shape[1] != 3:
            raise RuntimeError(f"overlay_u8: maps {tuple(maps.shape)} must be [{B},S,S], rng {tuple(rng.shape)} [{B},2], "
                               f"lut {tuple(lut.shape)} [L,3]")
        S, L = maps.shape[1], lut.shape[0]
    else:
        rng = lut = None
    if pts is not None and pts.shape[1] > 0:
        pts, colors = _dev(pts.detach(), "pts"), _dev(colors.detach(), "colors")
        K = pts.shape[1]
        if tuple(pts.shape) != (B, K, 2) or tuple(colors.shape) != (K, 3):
            raise RuntimeError(f"overlay_u8: pts {tuple(pts.shape)} must be [{B},K,2] and colors {tuple(colors.shape)} [K,3]")
        if labels:
            if glyphs is None or not glyphs.is_cuda or glyphs.dtype != torch.uint8 or tuple(glyphs.shape) != (10, 7):
                raise RuntimeError("overlay_u8: labels need glyphs, uint8 [10,7] on the device (there is no CPU fallback)")
            glyphs = glyphs.contiguous()
        else:
            glyphs = None
    else:
        pts = colors = glyphs = None
    if out is None:
        out, origin, cols, gap = torch.empty(B, H, W, 3, device=img.device, dtype=torch.uint8), (0, 0), 1, 0
        ch, ld = B * H, W
    else:
        if not out.is_cuda or out.dtype != torch.uint8 or out.dim() != 3 or out.shape[2] != 3 or not out.is_contiguous():
            raise RuntimeError("overlay_u8: out must be a contiguous uint8 canvas [h, w, 3] on the device (there is no CPU fallback)")
        ch, ld = out.shape[0], out.shape[1]
    _launch("skp_overlay_u8_f32", img, maps, rng, lut, pts, colors, glyphs, out, B, H, W, S, L, K, float(alpha), float(radius),
            float(ring), int(bool(labels)), ld, ch, int(origin[0]), int(origin[1]), int(cols), int(gap))
    return out


def mfma_issue_rate(waves_per_simd: int = 1, iters: int = 20000, device=None) -> float:
    """Measurement aid: TFLOP/s of back-to-back independent fp32 MFMAs with `waves_per_simd` waves on every SIMD."""
    import ctypes
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    scratch = torch.empty(256 * 4 * 256, device=dev, dtype=torch.float32)
    out = ctypes.c_float(0.0)
    with torch.cuda.device(dev):
        N.check(N.lab().skp_probe_mfma_f32(int(waves_per_simd), int(iters), scratch.data_ptr(), ctypes.byref(out), _stream()),
                "skp_probe_mfma_f32")
    return float(out.value)


def _qkv_stack(wq, wk, wv):
    """[3, C, C] stack of the three frozen projection weights of a self-attention block (made once per block)."""
    return weight_stack([wq, wk, wv])


def weight_stack(ws):
    """[len(ws), N, K] stack of frozen [N, K] weights (~200 MB over SD-1.5's attention projections), kept on the first one per
    list of members and re-made whenever a member's storage or version has moved (`.to()`, dtype change, `load_state_dict`)."""
    return cached(ws[0], ("stack", *map(id, ws)), ws, lambda: torch.stack([w.detach() for w in ws]).contiguous())


def _qkv_forward(x, wq, wk, wv):
    """q, k, v as ONE strided-batched GEMM: A = x with batch stride 0, B_i = W_i^T, C = [3, M, C] -- three times the
    workgroups of a single projection in one launch and three contiguous outputs (no strided views for the attention
    kernels).  Bit-equal to three F.linear calls per library kernel choice; 8 rows: 220 -> 180 us at 64^2, 186 -> 165 us
    at 16^2, 2 rows: 79 -> 49 us (tools/qkv_probe.py)."""
    F = torch.nn.functional
    if not (x.is_cuda and wq.shape == wk.shape == wv.shape):
        return F.linear(x, wq), F.linear(x, wk), F.linear(x, wv)
    c_in, c_out = wq.shape[1], wq.shape[0]
    x2 = x.reshape(-1, c_in)
    m = x2.shape[0]
    out = torch.bmm(x2.unsqueeze(0).expand(3, m, c_in), _qkv_stack(wq, wk, wv).transpose(1, 2))
    shp = (*x.shape[:-1], c_out)
    return out[0].view(shp), out[1].view(shp), out[2].view(shp)


class QKVProjFn(torch.autograd.Function):
    """q, k, v = x.Wq^T, x.Wk^T, x.Wv^T of a frozen self-attention block (bias-free projections, ptp_utils.py:513-520).
    Forward: one batched GEMM (_qkv_forward).  The input gradient accumulates inside the GEMMs (dx = dq.Wq, then two
    beta = 1 GEMMs) instead of three GEMMs and two add passes over [B, N, C]."""

    @staticmethod
    def forward(ctx, x, wq, wk, wv):
        ctx.save_for_backward(wq, wk, wv)
        return _qkv_forward(x, wq, wk, wv)

    @staticmethod
    def backward(ctx, dq, dk, dv):
        wq, wk, wv = ctx.saved_tensors
        shp = dq.shape
        dx = torch.mm(dq.reshape(-1, shp[-1]), wq)
        dx.addmm_(dk.reshape(-1, shp[-1]), wk)
        dx.addmm_(dv.reshape(-1, shp[-1]), wv)
        return dx.reshape(*shp[:-1], wq.shape[1]), None, None, None


def qkv_proj(x, wq, wk, wv):
    """Self-attention projections; frozen bias-free weights take the accumulate-in-GEMM backward."""
    frozen = not (wq.requires_grad or wk.requires_grad or wv.requires_grad)
    if x.is_cuda and x.requires_grad and torch.is_grad_enabled() and frozen:
        return QKVProjFn.apply(x, wq, wk, wv)
    if frozen and not (x.requires_grad and torch.is_grad_enabled()):
        return _qkv_forward(x, wq, wk, wv)
    F = torch.nn.functional
    return F.linear(x, wq), F.linear(x, wk), F.linear(x, wv)


class SelfAttnQKVFn(torch.autograd.Function):
    """One self-attention block core with frozen bias-free projections (ptp_utils.py:513-520, 493-506, 540):
    out = merge_heads(softmax(scale q k^T) v), q | k | v = x.W^T as one batched GEMM.  Backward: the flash backward writes
    dq, dk, dv as column bands of ONE [B*N, 3C] buffer (skp_flash_attn_bwd_ld_f32), so dx is a single GEMM against the
    stacked weights [3C, C] instead of three accumulating ones (8 rows: 224 -> 174 us at 64^2, tools/qkv_probe.py)."""

    @staticmethod
    def forward(ctx, x, wq, wk, wv, heads, scale):
        q, k, v = _qkv_forward(x, wq, wk, wv)
        B, Nq, C = q.shape
        out = torch.empty_like(q)
        lse = torch.empty(B, heads, Nq, device=q.device, dtype=torch.float32)
        _flash_fwd(q, k, v, out, lse, heads, scale)
        ctx.save_for_backward(q, k, v, out, lse, wq, wk, wv)
        ctx.meta = (int(heads), float(scale), tuple(x.shape))
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse, wq, wk, wv = ctx.saved_tensors
        heads, scale, xshape = ctx.meta
        dout = _dev(dout, "dout")
        B, Nq, C = q.shape
        d3 = torch.empty(B * Nq, 3 * C, device=q.device, dtype=torch.float32)
        p = d3.data_ptr()
        _flash_bwd(q, k, v, out, dout, lse, heads, scale, p, p + 4 * C, p + 8 * C, 3 * C)
        dx = torch.mm(d3, _qkv_stack(wq, wk, wv).view(3 * C, wq.shape[1]))
        return dx.view(xshape), None, None, None, None, None


FA2_HEAD_DIMS = (40, 64, 80, 160)          # head sizes of the second-generation flash kernels (the *_ld entry serves these)


def self_attention_block(x, wq, wk, wv, heads: int, scale: float):
    """Self-attention core of a block whose q / k / v projections are frozen and bias-free: projections + attention, with
    the fused input gradient where the kernels serve the head size; the composition of `qkv_proj` and `self_attention`
    otherwise (no gradient wanted, other head sizes)."""
    frozen = not (wq.requires_grad or wk.requires_grad or wv.requires_grad)
    if (x.is_cuda and x.dim() == 3 and frozen and x.requires_grad
            and torch.is_grad_enabled() and wq.shape == wk.shape == wv.shape and wq.shape[0] % heads == 0
            and (wq.shape[0] // heads) in FA2_HEAD_DIMS):
        routes.note("attn.self", "fused_qkv")
        return SelfAttnQKVFn.apply(_dev(x, "x"), wq, wk, wv, int(heads), float(scale))
    q, k, v = qkv_proj(x, wq, wk, wv)
    return self_attention(q, k, v, heads, scale)


def conv1x1_nobias(x, weight):
    """1x1 convolution without its bias as one batched GEMM over the NCHW planes: y[b] = W [Co,Ci] . x[b] [Ci, H*W]
    (the library convolution wraps the same product in NCHW<->NHWC transposes).  Autograd: dx[b] = W^T . dy[b]."""
    b, ci, h, w = x.shape
    w2 = weight.reshape(weight.shape[0], ci)
    return torch.matmul(w2, x.reshape(b, ci, h * w)).reshape(b, weight.shape[0], h, w)


# ---------------------------------------------------------------------------------------------------------
# 3x3 / stride 2 down-sampling convolutions of the frozen VAE encoder (forward only: they run under no_grad).
# ---------------------------------------------------------------------------------------------------------
def conv3x3_s2_supported(x, weight) -> bool:
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and tuple(weight.shape[2:]) == (3, 3)):
        return False
    b, ci, h, w = (int(v) for v in x.shape)
    co = int(weight.shape[0])
    return (CONV3X3_MODE != "lib" and int(weight.shape[1]) == ci and ci % 16 == 0 and co % 32 == 0 and h % 16 == 0
            and w % 32 == 0 and max(b * ci * h * w, b * co * (h // 2) * (w // 2), 9 * ci * co) * 4 < 2 ** 31)


def conv3x3_s2_tile_only(x, weight) -> bool:
    """The stride-2 kernel refuses this input for its 16 x 32 pixel tile alone: the same tensor grown to the next tile multiple
    would pass `conv3x3_s2_supported` (asked of a stride-0 view of that size: the gate reads shape, device and dtype only)."""
    if x.dim() != 4 or 0 in x.shape:
        return False
    h, w = -(-x.shape[2] // 16) * 16, -(-x.shape[3] // 32) * 32
    return (h, w) != tuple(x.shape[2:]) and conv3x3_s2_supported(x[:, :, :1, :1].expand(-1, -1, h, w), weight)


class ConvS2Fn(torch.autograd.Function):
    """Stride-2 3x3 convolution of a frozen UNet Downsample2D whose INPUT needs a gradient: forward on the direct MFMA
    kernel.  Input gradient: the transposed stride-2 convolution is the stride-1 convolution of the ZERO-STUFFED output
    gradient (dy_up[2i, 2j] = dy[i, j]) with the rotated, transposed filter -- i.e. the Winograd backward-data kernel of
    the stride-1 layers on a dy_up of the input's size (three quarters of its taps multiply zeros, which costs what the
    direct form's 4x multiplies would; no library call, no NCHW <-> NHWC transposes).  pad = 1 (UNet): out[i] reads
    x[2i - 1 + k] => dx[y] = sum_k w[k] dy_up[y + 1 - k]; pad = 0 (asymmetric (0,1,0,1) extension): x[2i + k] =>
    dy_up is shifted by one: dy_up[2i + 1, 2j + 1] = dy[i, j]."""

    @staticmethod
    def forward(ctx, x, weight, bias, pad):
        ctx.weight = weight
        ctx.xshape, ctx.pad = tuple(x.shape), int(pad)
        return _conv3x3_s2_raw(x, weight, bias, pad, False)

    @staticmethod
    def backward(ctx, dy):
        w = ctx.weight
        b, c, h, wd = ctx.xshape
        co = w.shape[0]
        plan = conv3x3_plan((b, co, h, wd), (c, co, 3, 3), backward=True) if (h % 2 == 0 and wd % 2 == 0) else None
        if plan is not None and plan.route != "lib":
            dy = _dev(dy, "dy")
            routes.note("conv3x3_s2.bwd_data", "zero_stuffed")
            up = torch.zeros(b, co, h, wd, device=dy.device, dtype=torch.float32)
            o = 0 if ctx.pad == 1 else 1
            up[:, :, o::2, o::2] = dy
            return _conv3x3_run("conv3x3_s2 backward", up, w, None, None, plan), None, None, None
        routes.note("conv3x3_s2.bwd_data", "lib")
        if ctx.pad == 1:
            return torch.nn.grad.conv2d_input(ctx.xshape, w, dy.contiguous(), stride=2, padding=1), None, None, None
        dxp = torch.nn.grad.conv2d_input((b, c, h + 1, wd + 1), w, dy.contiguous(), stride=2, padding=0)   # pad 0 = (0,1,0,1) extension
        return dxp[:, :, :h, :wd], None, None, None


def conv3x3_s2(x, weight, bias=None, pad: int = 0, want_stats: bool = False):
    """y = conv2d(zero-extended x, weight, bias, stride 2): pad = 0 is F.pad(x, (0,1,0,1)) + padding 0 (the VAE's
    Downsample2D), pad = 1 is padding 1.  Frozen weights; an input that needs a gradient goes through ConvS2Fn."""
    if weight.requires_grad or (bias is not None and bias.requires_grad):
        raise RuntimeError("conv3x3_s2: frozen weights only")
    if torch.is_grad_enabled() and x.requires_grad:
        return ConvS2Fn.apply(x, weight, bias, int(pad))
    return _conv3x3_s2_raw(x, weight, bias, pad, want_stats)


def _conv3x3_s2_raw(x, weight, bias, pad, want_stats):
    x = _dev(x.detach(), "x")
    B, ci, H, W = x.shape
    dims = (B, ci, int(weight.shape[0]), H, W, int(pad))
    # decided here, once: the kernel family (polyphase Winograd F(4x4,2x2) where it was measured faster, else the direct kernel),
    # its ledger name and filter form, the statistics blocks per image (16 whole 4x4-output tiles / one 8 x 16 output tile each)
    # and the pixels per block
    if N.lib().skp_conv3x3_s2w_ok(*dims):
        tiles = (H // 8) * (W // 8)
        route, form, pixels, nblk = "s2_wino", "s2w", 256, (tiles // 16 if want_stats and tiles % 16 == 0 else 0)
        entry = "skp_conv3x3_s2w_stats_f32" if nblk else "skp_conv3x3_s2w_f32"
    else:
        route, form, pixels, nblk = "s2_direct", "s2", 128, ((H // 16) * (W // 32) if want_stats else 0)
        entry = "skp_conv3x3_s2_stats_f32" if nblk else "skp_conv3x3_s2_ws_f32"
    routes.note("conv3x3_s2", route)
    U = _filters(weight, form)
    y = torch.empty(B, dims[2], H // 2, W // 2, device=x.device, dtype=torch.float32)
    if nblk:
        extra = (torch.empty(B, dims[2], nblk, 2, device=x.device, dtype=torch.float32),)
    elif form == "s2":                                   # small grid: K split over the input channels
        extra = (_workspace("skp_conv3x3_s2_workspace", *dims[:5], device=x.device),)
    else:
        extra = ()
    _launch(entry, x, U, bias, y, *extra, *dims)
    return _leave_blocks(y, extra[0] if nblk else None, nblk, pixels)


class GEGLUFn(torch.autograd.Function):
    """h * gelu(gate) on the feed-forward projection [.., 2*inner] (h = first half, gate = second half)."""

    @staticmethod
    def forward(ctx, proj):
        proj = _dev(proj, "proj")
        inner = proj.shape[-1] // 2
        rows = proj.numel() // (2 * inner)
        y = torch.empty(*proj.shape[:-1], inner, device=proj.device, dtype=torch.float32)
        _launch("skp_geglu_fwd_f32", proj, y, rows, inner)
        ctx.save_for_backward(proj)
        return y

    @staticmethod
    def backward(ctx, dy):
        (proj,) = ctx.saved_tensors
        dy = _dev(dy, "dy")
        inner = proj.shape[-1] // 2
        dp = torch.empty_like(proj)
        _launch("skp_geglu_bwd_f32", proj, dy, dp, proj.numel() // (2 * inner), inner)
        return dp


def geglu(proj):
    return GEGLUFn.apply(proj)


def _to_tokens_raw(x):
    B, C, H, W = x.shape
    y = torch.empty(B, H * W, C, device=x.device, dtype=torch.float32)
    _launch("skp_nchw_to_tokens_f32", x, y, B, C, H * W)
    return y


def _to_nchw_raw(t, res, H, W):
    B, HW, C = t.shape
    y = torch.empty(B, C, H, W, device=t.device, dtype=torch.float32)
    _launch("skp_tokens_to_nchw_f32", t, res, y, B, C, HW)
    return y


class NchwToTokensFn(torch.autograd.Function):
    """[B,C,H,W] -> [B,H*W,C] (the permute(0,2,3,1).reshape of Transformer2DModel) as one tiled transpose."""

    @staticmethod
    def forward(ctx, x):
        ctx.hw = (x.shape[2], x.shape[3])
        return _to_tokens_raw(_dev(x, "x"))

    @staticmethod
    def backward(ctx, dy):
        return _to_nchw_raw(_dev(dy, "dy"), None, *ctx.hw)


class TokensToNchwAddFn(torch.autograd.Function):
    """[B,H*W,C] -> [B,C,H,W] plus the block residual in the same pass."""

    @staticmethod
    def forward(ctx, t, res):
        return _to_nchw_raw(_dev(t, "t"), _dev(res, "res"), res.shape[2], res.shape[3])

    @staticmethod
    def backward(ctx, dy):
        dy = _dev(dy, "dy")
        return (_to_tokens_raw(dy) if ctx.needs_input_grad[0] else None), (dy if ctx.needs_input_grad[1] else None)


def layout_supported(x):
    return x.is_cuda and x.dtype == torch.float32 and x.shape[1] % 4 == 0 and (x.shape[2] * x.shape[3]) % 4 == 0


def nchw_to_tokens(x):
    return NchwToTokensFn.apply(x)


def tokens_to_nchw_add(t, res):
    return TokensToNchwAddFn.apply(t, res)
