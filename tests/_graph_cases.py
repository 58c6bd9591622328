"""What tests/test_sample_graph_host.py and tests/test_sample_graph_gpu.py share: the rows the device-row step kernels are held to
(the samplers' coefficient rows restated in tests/_sampler_cases.py, placed in longer tables between NaN rows), the whole-call cases
of the captured loop, and the configurations the graph key has to tell apart.  Nothing here touches a device."""
from __future__ import annotations

import struct

import torch

import _sampler_cases as S

ROW = 8                                                   # SKP_STEP_ROW: sa sb cx c0 ce c1 cn guidance
TABLE_ROWS = 7                                            # the tables of the kernel tests: rows 0, 3 and 6 are read, the others are NaN
AT = (0, TABLE_ROWS // 2, TABLE_ROWS - 1)                  # *step at the first, a middle and the last row
SIZES = (1, 5, 768, 1023, 16387)                          # the sibling test's sizes (tests/test_samplers_gpu.py)
GUIDANCE = 7.5


def f32(v: float) -> float:
    """A host double rounded to float32 once, as a C `float` argument is."""
    return struct.unpack("f", struct.pack("f", float(v)))[0]


def sampler_rows():
    """[(label, position 0 | 1 | 2, (sa, sb, cx, c0, ce, c1, cn) in fp64)]: every sampler's row at the first, a middle and the last
    step of its 4- and 20-step tables, and the solvers' last row into final_alpha_cumprod == 1 (cx = 0, c0 = 1)."""
    out = []
    _, acp, final = S.schedule(False)
    for kind, eta in S.SAMPLERS:
        for n in (4, 20):
            rows = S.restated_rows(kind, eta, acp, final, n)
            out += [(f"{kind} eta={eta} {n} steps step {i}", pos, rows[i]) for pos, i in enumerate((0, n // 2, n - 1))]
    _, acp1, final1 = S.schedule(True)
    out += [(f"{kind} 4 steps last step into a' = 1", 2, S.restated_rows(kind, 0.0, acp1, final1, 4)[-1]) for kind in ("dpm++2m", "dpm++2m-sde")]
    assert any(r[5] != 0 and r[6] != 0 for _, _, r in out) and any(r[5] == 0 for _, _, r in out) and any(r[6] == 0 for _, _, r in out)
    return out


def table_with(row, at, guidance=GUIDANCE):
    """float32 [TABLE_ROWS, ROW] full of NaN except row `at` = (row, guidance), each number rounded once."""
    t = torch.full((TABLE_ROWS, ROW), float("nan"), dtype=torch.float32)
    t[at] = torch.tensor([f32(v) for v in tuple(row) + (guidance,)], dtype=torch.float32)
    return t


# ---------------------------------------------------------------------------------------------------------------------------
# the captured loop: the reduced-width tree at the sizes of tests/test_samplers_gpu.py (64^2) and, with keypoints, of
# tests/test_keypoint_guidance_gpu.py (128^2)
# ---------------------------------------------------------------------------------------------------------------------------
STEPS = 6
# name -> (sampler, eta, unconditional embedding None | "u16" (doubled) | "u24" (two forwards), seeds, prediction type)
LOOP_CASES = {
    "default": (None, 0.0, None, (50,), "epsilon"),                         # the axpby step
    "default-guided": (None, 0.0, "u16", (50,), "epsilon"),                 # the guided DDIM step, doubled
    "default-guided-t24": (None, 0.0, "u24", (50,), "epsilon"),             # two forwards
    "ddim-eta0": ("ddim", 0.0, None, (50,), "epsilon"),                     # routed to the default step
    "ddim-eta0.5": ("ddim", 0.5, None, (50,), "epsilon"),
    "ddim-eta0.5-guided": ("ddim", 0.5, "u16", (50,), "epsilon"),
    "dpm++2m": ("dpm++2m", 0.0, None, (50,), "epsilon"),
    "dpm++2m-guided": ("dpm++2m", 0.0, "u16", (50,), "epsilon"),
    "dpm++2m-guided-t24": ("dpm++2m", 0.0, "u24", (50,), "epsilon"),
    "dpm++2m-sde": ("dpm++2m-sde", 0.0, None, (50,), "epsilon"),
    "dpm++2m-sde-guided": ("dpm++2m-sde", 0.0, "u16", (50,), "epsilon"),
    "batch-of-3": ("dpm++2m-sde", 0.0, "u16", (50, 62, 54), "epsilon"),
    "v-default": (None, 0.0, None, (57,), "v_prediction"),                  # the DDIM step kernel without guidance
    "v-dpm++2m-guided": ("dpm++2m", 0.0, "u16", (43,), "v_prediction"),
}

# the three calls of the stale-state test, on ONE key: (steps, eta of "ddim", seed of the generator, seed of the embeddings, guidance)
STALE_CALLS = ((6, 0.5, 50, 23, 7.5), (4, 1.0, 62, 24, 3.0), (8, 0.25, 54, 25, 5.0))


def key_configurations():
    """A base configuration of `ptp_utils.sample_graph_key` and, per field, one that differs in that field alone."""
    base = dict(rows=1, doubled=False, two_forward=False, tokens=(16, None), latent_shape=(4, 8, 8), prediction="epsilon", clip=False,
                kind="ddim", history=False, noise=False, keypoints=0, layers=(0, 1, 2, 3), extra=(), tag=(("w", 0),))
    other = dict(rows=3, doubled=True, two_forward=True, tokens=(16, 24), latent_shape=(4, 16, 16), prediction="v_prediction",
                 clip=True, kind="dpm++2m", history=True, noise=True, keypoints=3, layers=(0, 1), extra=(2.0, True),
                 tag=(("w", 1),))
    return base, [dict(base, **{k: v}) for k, v in other.items()] + [dict(base, tokens=(24, None)), dict(base, kind="axpby"),
                                                                      dict(base, kind="ddim_step"), dict(base, extra=(2.0, False))]
