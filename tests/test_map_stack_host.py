"""CPU tests of `ops.MapStack`: every attention-map entry point holds its hooked layers to the same shape rules, and does so before
it looks at the device -- so a malformed stack is named on host tensors, and no kernel is ever launched with the geometry of
layer 0 on a layer of another shape."""
from types import SimpleNamespace

import pytest
import torch

from stablekeypoints_amd import _maps, ops

HEADS, C, SIDES, B, T, R = 2, 16, (4, 8), 2, 5, 16


def _stack(q1=(B, SIDES[1] ** 2, C), k1=(B, T, C)):
    """Two layers of host tensors, layer 1 with the given q / k shapes."""
    return [torch.zeros(B, SIDES[0] ** 2, C), torch.zeros(*q1)], [torch.zeros(B, T, C), torch.zeros(*k1)]


# case -> (keyword arguments of `_stack`, number of scales, what the message must say)
MALFORMED = {
    "query length not a square": (dict(q1=(B, 60, C)), 2, "layer 1: query length 60 is not a square"),
    "q batch rows": (dict(q1=(B + 1, 64, C)), 2, "layer 1: q has 3 batch rows"),
    "k batch rows": (dict(k1=(B + 1, T, C)), 2, "layer 1: k has 3 batch rows"),
    "k token count": (dict(k1=(B, T + 2, C)), 2, "layer 1: k has a token count of 7"),
    "head split": (dict(q1=(B, 64, 15), k1=(B, T, 15)), 2, "layer 1: 15 q channels do not split into 2 heads"),
    "k channels": (dict(k1=(B, T, 8)), 2, "layer 1: k has 8 channels, q has 16"),
    "scales": (dict(), 3, "one scale per layer: 3 scales for 2 layers"),
    "empty": (None, 0, "empty layer stack"),
}


def _flat(qs, ks):
    return [t for qk in zip(qs, ks) for t in qk]


def _meta(scales):
    return dict(R=R, heads=HEADS, scales=scales, thetas=[[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]], sigma=1.0, num_subjects=1,
                strategy="gaussian", n_cand=4, top_k=2, score_fn=None, pos=torch.zeros(B, 2, 2), sel=torch.tensor([0, 2]),
                tokrow=torch.full((T,), -1, dtype=torch.int32))


ENTRIES = {
    "attn_map": lambda qs, ks, sc: ops.attn_map(qs, ks, HEADS, sc, R),
    "attn_map_rows": lambda qs, ks, sc: ops.attn_map_rows(qs, ks, HEADS, sc, R, torch.tensor([0, 2])),
    "MapLossesFn": lambda qs, ks, sc: ops.MapLossesFn.apply(_meta(sc), *_flat(qs, ks)),
    "MapPointLossFn": lambda qs, ks, sc: ops.MapPointLossFn.apply(_meta(sc), *_flat(qs, ks)),
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_malformed_stack_is_named_before_the_device_check(entry, case):
    kw, n_scales, says = MALFORMED[case]
    qs, ks = ([], []) if kw is None else _stack(**kw)
    with pytest.raises(RuntimeError) as e:
        ENTRIES[entry](qs, ks, [0.25] * n_scales)
    msg = str(e.value)
    assert msg.startswith(entry + ": ") and says in msg, msg
    assert "no CPU fallback" not in msg, msg


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_well_formed_host_stack_still_meets_the_device_check(entry):
    qs, ks = _stack()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ENTRIES[entry](qs, ks, [0.25, 0.25])


def test_a_shared_context_row_is_well_formed():
    qs, ks = _stack(k1=(1, T, C))                                  # Bk = 1: one context for all batch rows
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.attn_map(qs, ks, HEADS, [0.25, 0.25], R)


def _records(R1=R, heads1=HEADS):
    qs, ks = _stack()
    return [_maps.FusedAttn(qs[0], ks[0], HEADS, 0.25, R), _maps.FusedAttn(qs[1], ks[1], heads1, 0.25, R1)]


@pytest.mark.parametrize("kw", [dict(R1=2 * R), dict(heads1=2 * HEADS)], ids=["R", "heads"])
def test_records_that_disagree_are_named_by_their_collector(kw):
    with pytest.raises(RuntimeError, match="^fused_maps: hooked layers disagree on feature_upsample_res / head count"):
        _maps.fused_maps(_records(**kw))
    controller = SimpleNamespace(step_store={"attn": _records(**kw)}, reset=lambda: None)
    with torch.no_grad(), pytest.raises(RuntimeError, match="^collect_maps_batched: hooked layers disagree on"):
        _maps.collect_maps_batched(controller, layers=(0, 1), indices=[0, 2])
    with pytest.raises(RuntimeError, match="^fused_maps: hooked layers disagree on"):
        _maps.collect_maps_batched(controller, layers=(0, 1))     # all rows: the differentiable route through fused_maps
