"""csrc/skp_select_loss.hip against the fp64 oracle over sizes, ties and affines.

Token statistics, candidate ranking + furthest-point sampling, the fused sharpening / equivariance losses with their three
gradients, the gather form of d equiv / d Mt and the row update, each in isolation.  The reference side is oracle/ref_path.py
on double tensors; integer outputs (arg-maxima, candidates, selections) are compared exactly, float outputs as
max |kernel - fp64| / max |fp64| against the bounds below.

`SKP_TEST_FP32_ORACLE=1` also prints the same ratio for the oracle run in fp32 on the CPU beside every kernel figure (`-s`).
"""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_path as R

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_ORACLE = os.environ.get("SKP_TEST_FP32_ORACLE") == "1"

# Bounds on max |kernel - fp64| / max |fp64|: 4x the larger of the two figures observed over every case of this file, rounded
# up to one significant digit.  Observed on the MI355X (`SKP_TEST_FP32_ORACLE=1 pytest -m gpu -s`, lines "err check"), worst case:
#                        kernel                               fp32 CPU oracle
TOL_KL = 5e-6          # 1.15e-6 (T 77, R 128)                5.7e-7 (T 77, R 128)
TOL_ENTROPY = 1e-6     # 2.4e-7 (T 1024, R 24); x10: 1.8e-7   2.2e-7; x10: 2.1e-7
TOL_SHARP = 5e-7       # 1.2e-7 (R 33, K 1, ns 3)             9.1e-8 (R 24, K 64, ns 3)
TOL_EQUIV = 3e-6       # 4.9e-7 (R 33, K 64, rot90)           6.9e-7 (R 33, K 1, rot90)
TOL_D_SHARP = 6e-7     # 1.3e-7 (R 24, K 64, ns 3)            1.3e-7 (R 33, K 64, ns 3)
TOL_D_EQUIV_M = 7e-5   # 1.5e-5 (R 128, K 64, scale0.3_out)   1.7e-5 (R 128, K 5, scale0.3_out)
TOL_D_EQUIV_MT = 2e-4  # 3.8e-5 (R 128, K 64, scale0.3_out)   4.2e-5 (R 128, K 1, scale0.3_out)
# (both equivariance gradients are worst where the inverse affine magnifies 3.3x at R = 128: an fp32 sampling position there
# is 1e-5 px off, in the kernel and in the fp32 oracle alike; at R <= 40 both stay below 1.2e-5.  The gather test, M = 1 at
# R = 33, observes at most 9.9e-6 anywhere.)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from stablekeypoints_amd import ops as o
    o.N.lib()                     # raises if libskp_hip.so is missing: no fallback
    return o


def _max_subjects() -> int:
    """SKP_MAX_SUBJECTS as the kernels see it: csrc/skp_common.h, which takes it from include/skp.h."""
    for rel in ("stablekeypoints_amd/csrc/skp_common.h", "include/skp.h"):
        m = re.search(r"^#define\s+SKP_MAX_SUBJECTS\s+(\d+)", open(os.path.join(_ROOT, rel)).read(), re.M)
        if m:
            return int(m.group(1))
    raise AssertionError("SKP_MAX_SUBJECTS not found")


MAX_SUBJECTS = _max_subjects()

# (T, R, n_cand, top_k, num_subjects)
SIZES = [
    (300, 40, 64, 64, 1),             # R^2 = 1600: two chunks, ragged second one, R^2 % 256 != 0; T > 256; 64 lanes; top_k = n_cand
    (1024, 24, 64, 10, 2),            # T at SKP_SEL_MAXT; R^2 = 576 < one chunk; two subjects
    (130, 33, 32, 2, 3),              # odd R, R^2 = 1089 = one chunk + 65; top_k = 2; three subjects
    (77, 128, 25, 10, 1),             # the workload's own shape, 16 chunks
    (16, 8, 16, 16, MAX_SUBJECTS),    # n_cand = T; 0.05 R < 1 pixel: the mask removes nothing
]
SIGMA = 2.0


def make_maps(T: int, R_: int, seed: int) -> torch.Tensor:
    """Non-negative maps [T,R,R] with sum_t == 1: noise plus one gaussian bump (sigma 2 px, height U[0,6]) per token, softmax
    over the tokens.  Some tokens are peaky, the KL values are spread."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(T, R_, R_, generator=g) * 1.5
    cy = torch.rand(T, generator=g) * R_
    cx = torch.rand(T, generator=g) * R_
    h = torch.rand(T, generator=g) * 6.0
    ar = torch.arange(R_, dtype=torch.float32) + 0.5
    d2 = (ar.view(1, R_, 1) - cy.view(T, 1, 1)) ** 2 + (ar.view(1, 1, R_) - cx.view(T, 1, 1)) ** 2
    z = z + h.view(T, 1, 1) * torch.exp(-d2 / (2.0 * 2.0 ** 2))
    return torch.softmax(z, dim=0).contiguous()


def _ratio(got: torch.Tensor, ref: torch.Tensor) -> float:
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    scale = ref.abs().max().item()
    return (got - ref).abs().max().item() / scale if scale > 0 else (got - ref).abs().max().item()


def _check(what: str, got, ref64, bound: float, ref32=None):
    """Print max |got - fp64| / max |fp64| (and the fp32 CPU oracle's, when given), then assert the kernel's against `bound`."""
    err = _ratio(torch.as_tensor(got), torch.as_tensor(ref64))
    side = f", fp32 oracle {_ratio(torch.as_tensor(ref32), torch.as_tensor(ref64)):.2e}" if ref32 is not None else ""
    print(f"err check [{what}]: kernel {err:.2e}{side} (bound {bound:.0e})")
    assert err <= bound, f"{what}: off by {err:.3e} of the fp64 maximum (bound {bound:.0e})"


def _positions(maps: torch.Tensor, ns: int) -> torch.Tensor:
    """R.find_k_max_pixels / R in the maps' dtype.  (The oracle's positions are fp32 whatever the maps are, so that its
    gaussian targets would stay fp32 under double maps.)"""
    return R.find_k_max_pixels(maps, ns).to(maps.dtype) / maps.shape[-1]


def _gaussian_kl(maps: torch.Tensor, ns: int, eps: float = 1e-5) -> torch.Tensor:
    """R.gaussian_kl with the target in the maps' dtype; the same values as the oracle's for fp32 maps."""
    n, h, w = maps.shape
    sm = torch.softmax(maps.reshape(n, h * w) + eps, dim=-1)
    tgt = R.gaussian_circles(_positions(maps, ns), size=h, sigma=SIGMA).reshape(n, h * w) + eps
    tgt = tgt / tgt.sum(dim=-1, keepdim=True)
    return torch.sum(tgt * (torch.log(tgt) - torch.log(sm)), dim=-1)


def _sharpening(maps: torch.Tensor, ns: int) -> torch.Tensor:
    """R.sharpening_loss with the target in the maps' dtype; the same value as the oracle's for fp32 maps."""
    return F.mse_loss(maps, R.gaussian_circles(_positions(maps, ns), size=maps.shape[1], sigma=SIGMA))


def _flat(pts: torch.Tensor, R_: int) -> torch.Tensor:
    """find_k_max_pixels' (row + 0.5, col + 0.5) -> flat pixel indices."""
    return ((pts[..., 0] - 0.5) * R_ + (pts[..., 1] - 0.5)).round().long()


# ----------------------------------------------------------------------------------------------------------------------------
# 1  token statistics
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,R_,n_cand,top_k,ns", SIZES)
def test_token_stats_vs_fp64(ops, T, R_, n_cand, top_k, ns):
    M = make_maps(T, R_, seed=11)
    am, kl, ent = ops.token_stats(M.cuda(), ns, sigma=SIGMA, want_entropy=True)
    ref_am = _flat(R.find_k_max_pixels(M, ns), R_)
    assert torch.equal(_flat(R.find_k_max_pixels(M.double(), ns), R_), ref_am), "near-tie in the input maps: pick another seed"
    assert torch.equal(am.cpu().long(), ref_am)
    tag = f"T{T} R{R_} ns{ns}"
    _check(f"kl {tag}", kl, _gaussian_kl(M.double(), ns), TOL_KL, R.gaussian_kl(M, SIGMA, 1e-5, ns) if FP32_ORACLE else None)
    _check(f"entropy {tag}", ent, R.token_entropy(M.double()), TOL_ENTROPY, R.token_entropy(M) if FP32_ORACLE else None)
    # as above these maps are nearly flat in space, every entropy within 1e-3 of log R^2: sharper ones spread them
    Ms = M * ENTROPY_GAIN
    _, _, ent = ops.token_stats(Ms.cuda(), 1, sigma=SIGMA, want_kl=False, want_entropy=True)
    _check(f"entropy x{ENTROPY_GAIN:.0f} {tag}", ent, R.token_entropy(Ms.double()), TOL_ENTROPY,
           R.token_entropy(Ms) if FP32_ORACLE else None)


def test_token_stats_exact_tie_and_masked_second_maximum(ops):
    """A planted two-way tie of the maximum: the first index wins.  A second maximum inside the first one's mask radius
    (0.05 * 40 = 2 px around the first centre) is skipped for the next one outside it."""
    T, R_ = 6, 40
    M = make_maps(T, R_, seed=3)
    top = M.max().item()
    # token 1: equal maxima at (30, 7) and (12, 25) -- the second one comes first in row-major order; both in different waves' share
    M[1, 30, 7] = top * 2; M[1, 12, 25] = top * 2
    # token 2: maximum at (20, 20), runner-up one pixel away (inside the mask), third value far away
    M[2, 20, 20] = top * 4; M[2, 21, 20] = top * 3; M[2, 5, 33] = top * 2
    # token 3: the tie is between the second maxima, after masking
    M[3, 8, 8] = top * 4; M[3, 33, 2] = top * 2; M[3, 15, 30] = top * 2
    # token 4: runner-up just OUTSIDE the radius ((1.5)^2 + (1.5)^2 = 4.5 > 4 from the centre (10.5, 10.5)): it is taken
    M[4, 10, 10] = top * 4; M[4, 12, 12] = top * 3
    am, _ = ops.token_stats(M.cuda(), 2, sigma=SIGMA, want_kl=False)
    am = am.cpu().long()
    assert torch.equal(am, _flat(R.find_k_max_pixels(M.double(), 2), R_))
    assert am[0, 1].item() == 12 * R_ + 25
    assert am[:, 2].tolist() == [20 * R_ + 20, 5 * R_ + 33]
    assert am[:, 3].tolist() == [8 * R_ + 8, 15 * R_ + 30]
    assert am[:, 4].tolist() == [10 * R_ + 10, 12 * R_ + 12]


# ----------------------------------------------------------------------------------------------------------------------------
# 2  candidate ranking + furthest-point sampling on synthetic scores and locations
# ----------------------------------------------------------------------------------------------------------------------------
SELECT_SIZES = [s[:4] for s in SIZES] + [(40, 12, 2, 2)]
SELECT_KINDS = ["distinct", "tie_blocks", "lattice", "one_pixel", "corners_cluster", "nan"]


def _select_input(kind: str, T: int, R_: int, n_cand: int, seed: int):
    """-> (kl float32 [T], argmax_t int32 [T] flat pixel indices)."""
    g = torch.Generator().manual_seed(seed)
    kl = torch.randperm(T, generator=g).float() * 0.25 + 1.0                   # distinct, exactly representable
    loc = torch.randint(0, R_ * R_, (T,), generator=g)
    if kind == "tie_blocks":                                                    # blocks of 7 equal scores: 7 divides no n_cand
        kl = (torch.randperm(T, generator=g) // 7).float() * 0.125
    elif kind == "lattice":                                                     # 4 x 4 lattice: many exactly equal distances
        step = max(R_ // 4, 1)
        loc = (torch.randint(0, 4, (T,), generator=g) * step) * R_ + torch.randint(0, 4, (T,), generator=g) * step
    elif kind == "one_pixel":
        loc = torch.full((T,), (R_ // 3) * R_ + R_ // 2)
    elif kind == "corners_cluster":                                             # the two far corners among the candidates + a 3 x 3 cluster
        c = R_ // 2
        loc = (c - 1 + torch.randint(0, 3, (T,), generator=g)) * R_ + c - 1 + torch.randint(0, 3, (T,), generator=g)
        first = torch.argsort(kl, stable=True)[:n_cand]
        pick = first[torch.randperm(n_cand, generator=g)[:2]]
        loc[pick[0]] = 0
        loc[pick[1]] = R_ * R_ - 1
    elif kind == "nan":                                                         # NaN (and +-inf) scores: NaN ranks last, index ascending
        n_nan = [T - min(n_cand, T) // 2, T // 3, T - n_cand][seed % 3]         # first variant: NaN reach the candidates
        idx = torch.randperm(T, generator=g)
        kl[idx[:n_nan]] = float("nan")
        if T - n_nan >= 4:
            kl[idx[n_nan]] = float("inf"); kl[idx[n_nan + 1]] = float("-inf"); kl[idx[n_nan + 2]] = float("inf")
    return kl.contiguous(), loc.to(torch.int32).contiguous()


def _furthest_points(loc, R_, cand, top_k):
    """The loops of R.furthest_point_sampling (ptp_utils.py:115-159) on arg-max locations, in float32 with IEEE operations
    (numpy): the kernel's contract is bit-equal distances, so that ties fall as in the reference.  The oracle itself cannot
    serve here: the fp32 torch.sqrt of the CPU build is not correctly rounded (1 ulp off for about 0.5 % of the arguments,
    depending on the host), and on locations drawn freely on the grid, where many distances are equal but for the rounding
    of (row + 0.5) / R, that decides late picks."""
    f = np.float32
    flat = loc.numpy().astype(np.int64)[cand.numpy()]
    ly, lx = ((flat // R_).astype(f) + f(0.5)) / f(R_), ((flat % R_).astype(f) + f(0.5)) / f(R_)      # find_max_pixel / h
    dy, dx = ly[:, None] - ly[None, :], lx[:, None] - lx[None, :]
    D = np.sqrt(dy * dy + dx * dx)
    assert D.dtype == f
    n = len(flat)
    best, pair = -1.0, None
    for i in range(n):                                                          # :132-137, strict '>': the first maximum wins
        for j in range(i + 1, n):
            if D[i, j] > best:
                best, pair = D[i, j], (i, j)
    chosen = list(pair)
    for _ in range(top_k - 2):                                                  # :142-157
        far, far_id = -1.0, None
        for c in range(n):
            if c in chosen:
                continue
            dmin = D[c, chosen].min()
            if dmin > far:
                far, far_id = dmin, c
        if far_id is not None:
            chosen.append(far_id)
    return cand[chosen]


def _select_reference(kl, loc, R_, n_cand, top_k):
    cand = torch.argsort(kl, stable=True)[:n_cand]
    return cand, _furthest_points(loc, R_, cand, top_k)


@pytest.mark.parametrize("T,R_,n_cand,top_k", SELECT_SIZES)
@pytest.mark.parametrize("kind", SELECT_KINDS)
def test_rank_and_furthest_point_sampling_exact(ops, kind, T, R_, n_cand, top_k):
    """Three images of different content: every single-image call equals the reference, and every row of the batched call
    equals its single-image call."""
    n = 3
    inputs = [_select_input(kind, T, R_, n_cand, seed) for seed in range(n)]
    kl_all = torch.stack([i[0] for i in inputs]).cuda()
    loc_all = torch.stack([i[1] for i in inputs]).cuda()
    cand_b = torch.full((n, n_cand), -1, device="cuda", dtype=torch.int64)
    sel_b = torch.full((n, top_k), -1, device="cuda", dtype=torch.int64)
    ops.N.check(ops.N.lib().skp_select_tokens_batched(kl_all.data_ptr(), loc_all.data_ptr(), n, T, R_, n_cand, top_k,
                                                      cand_b.data_ptr(), sel_b.data_ptr(), ops._stream()), "batched")
    for i, (kl, loc) in enumerate(inputs):
        cand, sel = ops.select_tokens(kl_all[i], loc_all[i], R_, n_cand, top_k)
        ref_cand, ref_sel = _select_reference(kl, loc, R_, n_cand, top_k)
        assert torch.equal(cand.cpu(), ref_cand), f"image {i}: candidates"
        assert torch.equal(sel.cpu(), ref_sel), f"image {i}: selection"
        assert torch.equal(cand_b[i], cand) and torch.equal(sel_b[i], sel), f"image {i}: batched row differs"


# ----------------------------------------------------------------------------------------------------------------------------
# 3  selection end to end on maps
# ----------------------------------------------------------------------------------------------------------------------------
MIN_SCORE_GAP = 1e-5
# The entropy strategy runs on the generator's maps times ENTROPY_GAIN.  As generated the maps are nearly flat in space (values
# around 1 / T), every entropy lies within 1e-3 of log R^2, and over seeds 1..39 the closest pair among the first n_cand + 1 is
# 2e-8 ... 4e-6 apart at the four larger sizes: below what fp32 resolves (fp32 vs fp64 oracle: 1.3e-6), so no seed defines an
# order.  Times 10 the entropies span 0.5 ... log R^2 and no probability reaches the FLT_EPSILON clamp of Categorical.
ENTROPY_GAIN = 10.0
# seed per (T, R, strategy), chosen on the CPU from the fp64 oracle scores alone as the best of seeds 1..24 (entropy) / 1..39
# (gaussian); value: (seed, smallest gap between adjacent sorted scores among the first n_cand + 1, fp32-vs-fp64 oracle score)
E2E_SEEDS = {
    (300, 40, "gaussian"): (20, 5.4e-5, 8.4e-7), (300, 40, "entropy"): (7, 7.8e-4, 1.3e-6),
    (1024, 24, "gaussian"): (18, 3.3e-5, 5.7e-7), (1024, 24, "entropy"): (22, 2.6e-4, 1.4e-6),
    (130, 33, "gaussian"): (30, 5.6e-4, 4.2e-7), (130, 33, "entropy"): (12, 1.5e-2, 1.2e-6),
    (77, 128, "gaussian"): (17, 6.9e-4, 9.1e-7), (77, 128, "entropy"): (6, 1.1e-2, 1.4e-6),
    (16, 8, "gaussian"): (14, 9.6e-3, 1.3e-7), (16, 8, "entropy"): (1, 6.4e-2, 2.5e-7),
}


@pytest.mark.parametrize("strategy", ["gaussian", "entropy"])
@pytest.mark.parametrize("T,R_,n_cand,top_k,ns", SIZES)
def test_selection_end_to_end_vs_fp64(ops, T, R_, n_cand, top_k, ns, strategy):
    seed = E2E_SEEDS[(T, R_, strategy)][0]
    gain = ENTROPY_GAIN if strategy == "entropy" else 1.0
    M, Mt = make_maps(T, R_, seed) * gain, make_maps(T, R_, seed + 1000) * gain
    score = R.gaussian_kl(M.double(), SIGMA, 1e-5, ns) if strategy == "gaussian" else R.token_entropy(M.double())
    gap = torch.sort(score).values[:n_cand + 1].diff().min().item()
    assert gap >= MIN_SCORE_GAP, f"fp64 scores {gap:.2e} apart: exact order is not defined in fp32, pick another seed"
    ref_cand = torch.argsort(score)[:n_cand]
    # R.select_tokens from here on (furthest-point sampling of these candidates on the arg-maxima of Mt), with the IEEE
    # square root of _furthest_points: with torch.sqrt the oracle's late picks depend on the host (see there)
    loc_t = _flat(R.find_max_pixel(Mt.double()), R_).to(torch.int32)
    ref_sel = _furthest_points(loc_t, R_, ref_cand, top_k)
    am, kl, ent = ops.token_stats(M.cuda(), ns, sigma=SIGMA, want_entropy=True)
    am_t, _ = ops.token_stats(Mt.cuda(), 1, sigma=SIGMA, want_kl=False)
    cand, sel = ops.select_tokens(kl if strategy == "gaussian" else ent, am_t[0], R_, n_cand, top_k)
    assert torch.equal(cand.cpu(), ref_cand)
    assert torch.equal(sel.cpu(), ref_sel)


# ----------------------------------------------------------------------------------------------------------------------------
# 4  losses and all three gradients over affines
# ----------------------------------------------------------------------------------------------------------------------------
def _reflection():
    th = R.affine_matrix(20.0, 0.8, (0.1, -0.15))
    th[0, 0] = -th[0, 0]                                                        # first row negated: det < 0
    return th


# (angle deg, scale, translate) of R.affine_matrix
AFFINES = {
    "identity": (0.0, 1.0, (0.0, 0.0)),
    "mild": (15.0, 0.9, (0.2, -0.25)),
    "rot45_half": (45.0, 0.5, (0.1, 0.1)),
    "rot-170": (-170.0, 1.3, (0.3, 0.3)),
    "scale2": (30.0, 2.0, (-0.25, 0.25)),                                       # inverse scale 0.5: pre-image box 4 x 4
    "rot90": (90.0, 1.0, (0.0, 0.0)),
    "scale0.3_out": (10.0, 0.3, (0.9, 0.0)),                                    # most of the footprint outside the map (clamped x0 / y0)
    "reflection": _reflection,
    "scale3.3": (-35.0, 3.3, (0.1, -0.2)),                                      # inverse scale 0.3: pre-image box about 7 x 7
}


def _theta(name: str) -> torch.Tensor:
    spec = AFFINES[name]
    return spec() if callable(spec) else R.affine_matrix(*spec)


def _loss_inputs(R_: int, K: int, seed: int):
    T = 70 if K == 64 else 12
    M, Mt = make_maps(T, R_, seed), make_maps(T, R_, seed + 1)
    sel = torch.randperm(T, generator=torch.Generator().manual_seed(seed + 2))[:K]      # distinct, unsorted
    return M, Mt, sel


def _ref_sharp(M, sel, ns, dtype):
    a = M.detach().to(dtype, copy=True).requires_grad_(True)
    sharp = R.sharpening_loss(a[sel], SIGMA, ns) if dtype == torch.float32 else _sharpening(a[sel], ns)
    return sharp.detach(), torch.autograd.grad(sharp, a)[0]


def _ref_equiv(M, Mt, sel, theta, dtype, direct_inverse=False):
    """-> (equiv, d/dM, d/dMt).  `direct_inverse`: theta IS the sampling affine (no inversion), for singular ones."""
    a, b = M.detach().to(dtype, copy=True).requires_grad_(True), Mt.detach().to(dtype, copy=True).requires_grad_(True)
    if direct_inverse:
        equiv = F.mse_loss(a[sel], R.affine_warp(b[sel][None], theta.to(dtype))[0])
    else:
        equiv = R.equivariance_loss(a[sel], b[sel], theta.to(dtype), 0)
    ga, gb = torch.autograd.grad(equiv, (a, b))
    return equiv.detach(), ga, gb


def _check_losses(ops, tag, M, Mt, sel, ns, theta, sharp_ref, direct_inverse=False):
    (s64, gs64), (s32, gs32) = sharp_ref
    a, b = M.cuda().requires_grad_(True), Mt.cuda().requires_grad_(True)
    seld = sel.cuda()
    am, _ = ops.token_stats(a, ns, sigma=SIGMA, want_kl=False)
    if direct_inverse:
        sharp, equiv = ops.LossesFn.apply(a, b, seld, am, theta.reshape(-1).tolist(), SIGMA, ns)
    else:
        sharp, equiv = ops.fused_losses(a, b, seld, am, theta.reshape(-1).tolist(), SIGMA, ns)
    gs, = torch.autograd.grad(sharp, a, retain_graph=True)
    ga, gb = torch.autograd.grad(equiv, (a, b), retain_graph=True)
    (3.0 * sharp + 7.0 * equiv).backward()
    e64, ga64, gb64 = _ref_equiv(M, Mt, sel, theta, torch.float64, direct_inverse)
    e32, ga32, gb32 = _ref_equiv(M, Mt, sel, theta, torch.float32, direct_inverse) if FP32_ORACLE else (None, None, None)
    _check(f"sharp {tag}", sharp, s64, TOL_SHARP, s32)
    _check(f"equiv {tag}", equiv, e64, TOL_EQUIV, e32)
    _check(f"d sharp/dM {tag}", gs, gs64, TOL_D_SHARP, gs32)
    _check(f"d equiv/dM {tag}", ga, ga64, TOL_D_EQUIV_M, ga32)
    _check(f"d equiv/dMt {tag}", gb, gb64, TOL_D_EQUIV_MT, gb32)
    # the weighted backward is the same three gradients combined, with fp32 products and adds (a few 2^-24) on top
    ms, me = 3.0 * gs64.abs().max().item(), 7.0 * ga64.abs().max().item()
    diff = (a.grad.cpu().double() - (3.0 * gs64 + 7.0 * ga64)).abs().max().item()
    assert diff <= (TOL_D_SHARP + 2.0 ** -22) * ms + (TOL_D_EQUIV_M + 2.0 ** -22) * me, f"{tag}: d(3 sharp + 7 equiv)/dM"
    assert _ratio(b.grad, 7.0 * gb64) <= TOL_D_EQUIV_MT + 2.0 ** -22, f"{tag}: d(3 sharp + 7 equiv)/dMt"
    rest = torch.ones(M.shape[0], dtype=torch.bool)
    rest[sel] = False
    for g_ in (gs, ga, gb, a.grad, b.grad):
        assert g_.cpu()[rest].abs().max().item() == 0.0, f"{tag}: an unselected row has a gradient"


def _sharp_refs(M, sel, ns):
    return _ref_sharp(M, sel, ns, torch.float64), (_ref_sharp(M, sel, ns, torch.float32) if FP32_ORACLE else (None, None))


@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("K", [1, 5, 64])
@pytest.mark.parametrize("R_", [24, 33, 40, 128])
def test_losses_and_gradients_vs_fp64_over_affines(ops, R_, K, ns):
    M, Mt, sel = _loss_inputs(R_, K, seed=100 + R_ + K)
    sharp_ref = _sharp_refs(M, sel, ns)
    for name in AFFINES:
        _check_losses(ops, f"R{R_} K{K} ns{ns} {name}", M, Mt, sel, ns, _theta(name), sharp_ref)


@pytest.mark.parametrize("R_,K", [(33, 5), (40, 1)])
def test_losses_singular_inverse_scans_everything(ops, R_, K):
    """An inverse affine with a zero second row (det == 0 <= 1e-12): every output pixel samples the same fractional row, the
    gather cannot bound its pre-image and scans the whole map.  Reference: grid_sample with that affine used directly."""
    M, Mt, sel = _loss_inputs(R_, K, seed=7)
    theta_inv = torch.tensor([[[0.9, 0.3, 0.05], [0.0, 0.0, 0.21]]])
    _check_losses(ops, f"R{R_} K{K} singular", M, Mt, sel, 1, theta_inv, _sharp_refs(M, sel, 1), direct_inverse=True)


def _raw_losses(ops, entry, M, Mt, sel, am, ns, theta_arg):
    T, R_, _ = M.shape
    K = sel.shape[0]
    nchunk = (R_ * R_ + 1023) // 1024
    out = [torch.full(s, float("nan"), device="cuda") for s in ((2, K, nchunk), (K, R_, R_), (K, R_, R_), (K, R_, R_))]
    rc = getattr(ops.N.lib(), entry)(M.data_ptr(), Mt.data_ptr(), sel.data_ptr(), K, T, R_, am.data_ptr(), ns, SIGMA, theta_arg,
                                     *[o.data_ptr() for o in out], ops._stream())
    assert rc == 0, f"{entry}: {rc}"
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("R_,K,ns,name", [(40, 5, 3, "mild"), (33, 64, 1, "rot45_half"), (128, 5, 1, "scale0.3_out")])
def test_device_theta_entry_is_bit_equal_to_host_theta_entry(ops, R_, K, ns, name):
    """skp_losses_fwd_dev_f32 (the entry of captured steps: six inverse numbers read from device memory) writes the same four
    buffers as skp_losses_fwd_f32, bit for bit."""
    M, Mt, sel = _loss_inputs(R_, K, seed=31)
    M, Mt, sel = M.cuda(), Mt.cuda(), sel.cuda()
    am, _ = ops.token_stats(M, ns, sigma=SIGMA, want_kl=False)
    inv = ops.invert_affine(_theta(name).reshape(-1).tolist())
    th_host, _keep = ops.N.float_array(inv)
    th_dev = torch.tensor(inv, dtype=torch.float32).cuda()
    host = _raw_losses(ops, "skp_losses_fwd_f32", M, Mt, sel, am, ns, th_host)
    dev = _raw_losses(ops, "skp_losses_fwd_dev_f32", M, Mt, sel, am, ns, th_dev.data_ptr())
    for what, h, d in zip(("partial", "g_sharp", "g_eq_a", "g_eq_b"), host, dev):
        assert not torch.isnan(h).any(), f"{what}: not every element was written"
        assert torch.equal(h, d), f"{what}: device-theta entry differs from the host-theta entry"


# ----------------------------------------------------------------------------------------------------------------------------
# 5  the gather of d equiv / d Mt collects every contribution
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(AFFINES))
def test_equiv_gather_is_complete_at_every_source_pixel(ops, name):
    """M = 1 and Mt = one-hot at a source pixel, one token per swept pixel (corners, edge midpoints, centre, 50 random ones at
    R = 33): every output pixel then carries a residual of order 1, so a contribution that the scanned bounding box misses is
    an O(1) relative error at that source pixel.  Compared per pixel, at the swept pixel and at every other one."""
    R_, e, c = 33, 32, 16
    g = torch.Generator().manual_seed(5)
    pix = [(0, 0), (0, e), (e, 0), (e, e), (0, c), (c, 0), (e, c), (c, e), (c, c)]
    pix += [tuple(p) for p in torch.randint(0, R_, (50, 2), generator=g).tolist()]
    T = len(pix)
    rows, cols = torch.tensor(pix).t()
    M = torch.ones(T, R_, R_)
    Mt = torch.zeros(T, R_, R_)
    Mt[torch.arange(T), rows, cols] = 1.0
    sel = torch.arange(T)
    theta = _theta(name)
    _, _, ref = _ref_equiv(M, Mt, sel, theta, torch.float64)
    a, b = M.cuda().requires_grad_(True), Mt.cuda().requires_grad_(True)
    am, _ = ops.token_stats(a, 1, sigma=SIGMA, want_kl=False)
    _, equiv = ops.fused_losses(a, b, sel.cuda(), am, theta.reshape(-1).tolist(), SIGMA, 1)
    got = torch.autograd.grad(equiv, b)[0].cpu().double()
    scale = ref.abs().max().item()
    assert scale > 0
    err = (got - ref).abs() / scale
    at = err[torch.arange(T), rows, cols]
    print(f"err check [gather {name}]: at the swept pixels {at.max().item():.2e}, anywhere {err.max().item():.2e} "
          f"(bound {TOL_D_EQUIV_MT:.0e})")
    worst = at.argmax().item()
    assert at.max().item() <= TOL_D_EQUIV_MT, f"{name}: d equiv/dMt at source pixel {pix[worst]} off by {at.max().item():.3e}"
    assert err.max().item() <= TOL_D_EQUIV_MT, f"{name}: d equiv/dMt off by {err.max().item():.3e} of its maximum"


# ----------------------------------------------------------------------------------------------------------------------------
# 6  row update
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_y", [True, False])
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1600])
def test_rows_axpy_vs_fp64(ops, n, K, with_y):
    """dst[sel[k]] += a * x[k] + b * y[k] (y may be null).  The rows of `sel` are distinct: that is the kernel's contract (two
    workgroups would otherwise update one row without ordering), and the selection never produces duplicates."""
    g = torch.Generator().manual_seed(n * 10 + K)
    rows = 9
    dst0 = torch.randn(rows, n, generator=g)
    x, y = torch.randn(K, n, generator=g), torch.randn(K, n, generator=g)
    a, b = torch.tensor(1.7), torch.tensor(-0.6)
    sel = torch.randperm(rows, generator=g)[:K]
    dst, xd, yd, ad, bd, seld = dst0.cuda(), x.cuda(), y.cuda(), a.cuda(), b.cuda(), sel.cuda()
    rc = ops.N.lib().skp_rows_axpy_f32(dst.data_ptr(), seld.data_ptr(), K, n, xd.data_ptr(), ad.data_ptr(),
                                       yd.data_ptr() if with_y else None, bd.data_ptr() if with_y else None, ops._stream())
    assert rc == 0
    ref = dst0.double()
    ref[sel] += a.double() * x.double() + (b.double() * y.double() if with_y else 0.0)
    # atol, for sums that cancel: three fp32 roundings (a x, + b y, dst +), each 2^-24 of at most (|a| + |b| + 1) * 5
    assert max(dst0.abs().max(), x.abs().max(), y.abs().max()).item() <= 5.0
    torch.testing.assert_close(dst.cpu().double(), ref, rtol=1e-6, atol=3 * 2.0 ** -24 * (1.7 + 0.6 + 1.0) * 5.0)
    rest = torch.ones(rows, dtype=torch.bool)
    rest[sel] = False
    assert torch.equal(dst.cpu()[rest], dst0[rest]), "a row outside `sel` changed"


# ----------------------------------------------------------------------------------------------------------------------------
# 7  argument checks of the C ABI (return codes only: a rejected call launches nothing)
# ----------------------------------------------------------------------------------------------------------------------------
def test_c_abi_rejects_bad_arguments(ops):
    lib, st = ops.N.lib(), ops._stream()
    T, R_, K = 8, 8, 4
    buf = torch.zeros(4096, device="cuda")                                      # large enough for every accepted call below
    ibuf = torch.arange(64, device="cuda", dtype=torch.int64)                   # distinct rows < T
    obuf = torch.zeros(64, device="cuda", dtype=torch.int64)                    # candidates / selections of the accepted calls
    p, ip, op = buf.data_ptr(), ibuf.data_ptr(), obuf.data_ptr()
    th, _keep = ops.N.float_array([1, 0, 0, 0, 1, 0])

    def select(T=T, n_cand=4, top_k=2, kl=p, am=ip, cand=op, sel=op):
        one = lib.skp_select_tokens(kl, am, T, R_, n_cand, top_k, cand, sel, st)
        many = lib.skp_select_tokens_batched(kl, am, 2, T, R_, n_cand, top_k, cand, sel, st)
        assert one == many
        return one

    assert select() == 0
    assert select(T=1025, n_cand=64) != 0
    assert select(T=100, n_cand=65) != 0
    assert select(T=8, n_cand=9) != 0
    assert select(top_k=1) != 0
    assert select(n_cand=4, top_k=5) != 0
    for null in ("kl", "am", "cand", "sel"):
        assert select(**{null: None}) != 0, null
    assert lib.skp_select_tokens_batched(p, ip, 0, T, R_, 4, 2, op, op, st) != 0

    def stats(ns=1, M=p, am=ip):
        return lib.skp_token_stats_f32(M, T, R_, ns, 2.0, 1e-5, am, p, None, st)

    assert stats() == 0
    assert stats(ns=0) != 0 and stats(ns=MAX_SUBJECTS + 1) != 0
    assert stats(M=None) != 0 and stats(am=None) != 0

    def losses(entry="skp_losses_fwd_f32", ns=1, theta=th, ptrs=None):
        a = dict(M=p, Mt=p, sel=ip, am=ip, partial=p, g_sharp=p, g_eq_a=p, g_eq_b=p)
        a.update(ptrs or {})
        return getattr(lib, entry)(a["M"], a["Mt"], a["sel"], K, T, R_, a["am"], ns, 2.0, theta, a["partial"], a["g_sharp"],
                                   a["g_eq_a"], a["g_eq_b"], st)

    assert losses() == 0
    assert losses("skp_losses_fwd_dev_f32", theta=p) == 0
    assert losses(theta=None) != 0
    assert losses("skp_losses_fwd_dev_f32", theta=None) != 0
    for entry, theta in (("skp_losses_fwd_f32", th), ("skp_losses_fwd_dev_f32", p)):
        assert losses(entry, ns=0, theta=theta) != 0 and losses(entry, ns=MAX_SUBJECTS + 1, theta=theta) != 0
        for null in ("M", "Mt", "sel", "am", "partial", "g_sharp", "g_eq_a", "g_eq_b"):
            assert losses(entry, theta=theta, ptrs={null: None}) != 0, (entry, null)

    def axpy(dst=p, sel=ip, x=p, a=p, y=p, b=p, K=2, n=16):
        return lib.skp_rows_axpy_f32(dst, sel, K, n, x, a, y, b, st)

    assert axpy() == 0 and axpy(y=None, b=None) == 0
    for null in ("dst", "sel", "x", "a"):
        assert axpy(**{null: None}) != 0, null
    assert axpy(b=None) != 0                                                    # y without its factor
    assert axpy(K=0) != 0 and axpy(n=0) != 0
    torch.cuda.synchronize()
