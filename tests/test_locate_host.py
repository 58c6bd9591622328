"""CPU tests of the keypoint locator (include/skp_locate.h, `eval.locate_keypoints`): the header against its table, refusals before any
launch, the launch plan's branches, the torch formula against the numpy fp64 restatement of tests/_locate_cases.py and against the
oracle on the reference's own maps, and the measurement the GPU test's tolerance comes from."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import _locate_cases as C
from oracle import ref_path as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["skp_locate_f32", "skp_locate_workspace"]


def _host_logic():
    spec = importlib.util.spec_from_file_location("_host_logic", os.path.join(ROOT, "tests", "test_host_logic.py"))
    H = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(H)
    return H


def test_locate_header_agrees_with_its_table():
    """include/skp_locate.h against `_native.LOCATE_SIGNATURES` with the comparison tests/test_host_logic.py applies to skp.h; the
    library exports the entries, the table is disjoint from the other three, the launching entry ends in the stream, the ABI moved."""
    from stablekeypoints_amd import _native as N
    from stablekeypoints_amd import ops
    H = _host_logic()
    hdr = open(os.path.join(ROOT, "include", "skp_locate.h")).read()
    abi = H._header_abi(hdr)
    assert sorted(abi) == sorted(N.LOCATE_SIGNATURES) == ENTRIES
    assert H._abi_mismatches(hdr, N.LOCATE_SIGNATURES) == []
    assert not set(N.LOCATE_SIGNATURES) & (set(N.SIGNATURES) | set(N.KEYPOINT_SIGNATURES) | set(N.OVERLAY_SIGNATURES))
    assert abi["skp_locate_f32"][1][-1] == "dev:void" and N.signature("skp_locate_f32") is N.LOCATE_SIGNATURES["skp_locate_f32"]
    assert N.signature("skp_map_range_f32") is N.OVERLAY_SIGNATURES["skp_map_range_f32"]
    lib = N.lib()
    assert lib.skp_abi_version() == N.ABI_VERSION >= 47
    for name, argtypes in N.LOCATE_SIGNATURES.items():
        assert getattr(lib, name).argtypes == argtypes
    assert len(ops._plan("skp_locate_f32")[1]) == len(N.LOCATE_SIGNATURES["skp_locate_f32"]) - 1
    mk = open(os.path.join(ROOT, "stablekeypoints_amd", "csrc", "Makefile")).read()
    assert "skp_locate.hip" in mk and "skp_locate.h" in mk


def _locate_args(**over):
    """A legal argument list of skp_locate_f32 (any non-null address: arguments are refused before a launch), edited by name."""
    one = 16
    a = dict(M=one, N=2, H=8, W=8, mode=1, distance=5.0, loc=one, flat=one, ws=one, ws_bytes=1 << 20)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values()) + [None]


def test_entries_refuse_bad_arguments_before_launching():
    from stablekeypoints_amd import _native as N
    lib = N.lib()
    BAD, RANGE = -1, -2
    q, f = lib.skp_locate_workspace, lib.skp_locate_f32
    assert q(0, 8, 8) == BAD and q(1, 0, 8) == BAD and q(1, 8, -1) == BAD
    assert q(1, 4097, 8) == RANGE and q(1, 8, 4097) == RANGE and q(2 ** 31 - 1, 4096, 4096) == 0
    for name in ("M", "loc", "flat"):
        assert f(*_locate_args(**{name: None})) == BAD, name
    for name in ("N", "H", "W"):
        for v in (0, -1):
            assert f(*_locate_args(**{name: v})) == BAD, name
    assert f(*_locate_args(mode=2)) == BAD and f(*_locate_args(mode=-1)) == BAD
    assert f(*_locate_args(distance=-2.0)) == BAD and f(*_locate_args(distance=-0.5)) == BAD
    assert f(*_locate_args(distance=float("nan"))) == BAD
    assert f(*_locate_args(H=4097)) == RANGE and f(*_locate_args(W=5000)) == RANGE
    need = q(3, 512, 512)
    assert need > 0
    assert f(*_locate_args(N=3, H=512, W=512, ws=None)) == BAD                       # the query asks for scratch here
    assert f(*_locate_args(N=3, H=512, W=512, ws_bytes=need - 1)) == BAD


def test_the_cases_cover_every_branch_of_the_plan():
    """What `skp_locate_workspace` tells apart -- no scratch (a wave or a workgroup per map; told apart by the 1024 elements the header
    states) and scratch of 32 bytes per segment -- and that the cases hold each: several maps per workgroup, one, several workgroups per map."""
    from stablekeypoints_amd import _native as N
    q = N.lib().skp_locate_workspace
    branch = {}
    for name, n, h, w, _ in C.CASES:
        ws = q(n, h, w)
        assert ws >= 0 and ws % (32 * n) == 0
        branch[name] = "split" if ws else ("wave" if h * w <= 1024 else "workgroup")
        if ws:
            segments = ws // (32 * n)
            assert 2 <= segments <= 256 and h * w >= 8192 and h * w / segments >= 4096 - 4
    assert {b: sum(v == b for v in branch.values()) >= 3 for b in ("wave", "workgroup", "split")} == dict(wave=True, workgroup=True, split=True)
    assert branch["n3 5x7"] == "wave" and branch["n70 64x64"] == "workgroup" and branch["n3 91x91"] == "split"
    assert q(1, 512, 512) == 64 * 32 and q(40, 512, 512) == 40 * 52 * 32 and q(5000, 128, 128) == 0
    assert {n for _, n, _, _, _ in C.CASES} == {1, 3, 70, 300}
    assert {(h, w) for _, _, h, w, _ in C.CASES} >= {(8, 8), (16, 16), (33, 33), (64, 64), (24, 40), (512, 512)}


def test_the_cases_hold_what_they_name():
    for name in ("n70 16x16", "n70 64x64"):
        maps, ks = C.build(name), C.kinds(name)
        assert set(ks) == set(C.KINDS)
        n, h, w = maps.shape
        for d in C.DISTANCES:
            loc, flat = C.want(name, 1, d)
            assert np.isfinite(loc).all() and ((0 <= flat) & (flat < h * w)).all()
        _, flat = C.want(name, 0)
        for i, k in enumerate(ks):
            m = maps[i]
            if k == "last":
                assert flat[i] == h * w - 1
            elif k == "corner00":
                assert flat[i] == 0
            elif k == "ties":
                hits = np.flatnonzero(m.reshape(-1) == m.max())
                assert len(hits) == 3 and flat[i] == hits[0]
            elif k == "zero":
                assert not m.any() and flat[i] == 0
                assert all((C.want(name, 1, d)[0][i] == 0.5).all() for d in C.DISTANCES)
            elif k == "constant":
                assert flat[i] == 0 and len(np.unique(m)) == 1
            elif k == "negative":
                assert (m < 0).all()
            elif k == "mixed":
                assert (m < 0).any() and (m > 0).any()
            elif k == "huge":
                assert m.max() == np.float32(1e30) and np.sort(m.reshape(-1))[-2] < 1e-6


@pytest.mark.parametrize("name", C.NAMES)
def test_formula_fp64_is_the_restatement(name):
    """`eval.locate_keypoints` on host fp64 tensors (the definition in torch) against the numpy restatement: the arg-max exact, the
    locations to 1e-12 of the map's side; the input untouched; leading dimensions kept."""
    from stablekeypoints_amd import eval as E
    from stablekeypoints_amd import routes
    maps = torch.from_numpy(C.build(name).astype(np.float64))
    keep = maps.clone()
    side = max(maps.shape[-2:])
    loc, flat = E.locate_formula(maps, "argmax")
    assert np.array_equal(flat.numpy(), C.want(name, 0)[1]) and np.array_equal(loc.numpy(), C.want(name, 0)[0])
    before = routes.snapshot()
    for d in C.DISTANCES:
        got = E.locate_keypoints(maps, "weighted_avg", d)
        assert got.dtype == torch.float64 and tuple(got.shape) == (maps.shape[0], 2)
        err = np.abs(got.numpy() - C.want(name, 1, d)[0]).max()
        assert err <= 1e-12 * side, (d, err)
    assert routes.delta(before) == {("eval.locate", "host"): len(C.DISTANCES)}
    assert torch.equal(maps, keep)
    if maps.shape[0] % 3 == 0 and maps.shape[0] <= 70:
        again = E.locate_keypoints(maps.reshape(3, -1, *maps.shape[1:]), "weighted_avg", 3)
        assert tuple(again.shape) == (3, maps.shape[0] // 3, 2)
        assert torch.equal(again.reshape(-1, 2), E.locate_keypoints(maps, "weighted_avg", 3))


def test_formula_fp32_on_the_reference_maps(golden):
    """The host route in fp32 on the reference's own augmented-inference maps, against the oracle (`pixel_from_weighted_avg`, which
    tests/test_oracle_golden.py pins to the reference's outputs) and against those outputs, at that test's tolerances."""
    from stablekeypoints_amd import eval as E
    g = golden("g9_reference_augmented_tiny.npz")
    maps = torch.from_numpy(g["maps"])
    keep, size = maps.clone(), float(maps.shape[-1])
    t = lambda a: torch.from_numpy(np.asarray(a))
    for d, key, tol, scale in ((5, "keypoints_weighted", dict(rtol=1e-6, atol=1e-6), size), (3, "weighted_d3", dict(rtol=1e-6, atol=1e-5), 1.0),
                               (-1, "weighted_all", dict(rtol=1e-6, atol=1e-5), 1.0)):
        got = E.locate_keypoints(maps, "weighted_avg", d)
        assert got.dtype == torch.float32
        torch.testing.assert_close(got / scale, R.pixel_from_weighted_avg(maps.clone(), distance=d) / scale, **tol)
        torch.testing.assert_close(got / scale, t(g[key]), **tol)
    assert torch.equal(E.locate_keypoints(maps), R.find_max_pixel(maps)) and torch.equal(E.locate_keypoints(maps) / size, t(g["keypoints"]))
    assert torch.equal(maps, keep)


def test_reference_order_fp32_error_is_what_is_recorded():
    """The measurement behind the GPU test's tolerance: the largest error, in pixels, of the reference-order fp32 computation
    (`oracle.ref_path.pixel_from_weighted_avg` on clones, on the CPU) against the fp64 restatement, over all cases -- windows and
    whole-map means apart.  Not zero (cases on which fp32 is exact would measure nothing); and what tests/_locate_cases.py records,
    to within a factor of 2 either way (the CPU's summation order may differ between torch builds)."""
    worst = {"window": 0.0, "whole": 0.0}
    for name in C.NAMES:
        maps = torch.from_numpy(C.build(name).copy())
        for d in C.DISTANCES:
            got = R.pixel_from_weighted_avg(maps.clone(), distance=d).numpy().astype(np.float64)
            err = float(np.abs(got - C.want(name, 1, d)[0]).max())
            key = "whole" if d == -1 else "window"
            if err > worst[key]:
                worst[key] = err
                print(f"{name}, distance {d}: {err:.3e} px")
    print(f"reference-order fp32: windows {worst['window']:.6e} px, whole map {worst['whole']:.6e} px")
    assert worst["window"] > 0 and worst["whole"] > 0
    assert C.REF_FP32_ERR_WINDOW / 2 <= worst["window"] <= 2 * C.REF_FP32_ERR_WINDOW
    assert C.REF_FP32_ERR_WHOLE / 2 <= worst["whole"] <= 2 * C.REF_FP32_ERR_WHOLE
    assert C.tolerance(3) == 4 * C.REF_FP32_ERR_WINDOW and C.tolerance(-1) == 4 * C.REF_FP32_ERR_WHOLE


def test_no_cpu_fallback_route_registered_arguments_checked():
    from stablekeypoints_amd import eval as E
    from stablekeypoints_amd import ops, routes
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.locate(torch.zeros(2, 4, 4))
    assert routes.ROUTES["eval.locate"] == {"locate": "hip", "host": "host"}
    with pytest.raises(ValueError):
        E.locate_keypoints(torch.zeros(2, 4, 4), "centroid")
    with pytest.raises(ValueError):
        E.locate_keypoints(torch.zeros(2, 4, 4), "weighted_avg", -3)
    with pytest.raises(ValueError):
        E.locate_keypoints(torch.zeros(4))
    with routes.strict():
        with pytest.raises(routes.UnexpectedRoute):
            E.locate_keypoints(torch.zeros(2, 4, 4))


def test_find_corresponding_points_on_host_tensors():
    """eval.py:159-195 against the oracle's entropy and arg-max: the tokens of lowest summed entropy, their locations as fractions."""
    from stablekeypoints_amd import eval as E
    g = torch.Generator().manual_seed(7)
    maps = torch.randn(3, 9, 12, 10, generator=g) * torch.linspace(0.2, 4, 9).view(1, 9, 1, 1)
    pts, tokens = E.find_corresponding_points(maps, num_points=4)
    ent = torch.stack([R.token_entropy(maps[i]) for i in range(3)]).sum(0)
    assert torch.equal(tokens, torch.argsort(ent)[:4])
    want = torch.stack([R.find_max_pixel(maps[i, tokens]) for i in range(3)]) / torch.tensor([12.0, 10.0])
    assert tuple(pts.shape) == (3, 4, 2) and torch.equal(pts, want) and float(pts.min()) > 0 and float(pts.max()) < 1
