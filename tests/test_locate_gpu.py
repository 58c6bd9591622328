"""GPU tests of the keypoint locator kernel (csrc/skp_locate.hip, include/skp_locate.h) against the numpy fp64 restatement of
tests/_locate_cases.py and against `eval.find_max_pixel`, on every branch of its launch plan."""
import numpy as np
import pytest
import torch

import _locate_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", C.NAMES)
def test_locate_against_the_restatement(name):
    """Per case: `flat` exact (mode 0, and what mode 1 reports); mode 0 = the pixel centre, bit for bit what `eval.find_max_pixel`
    gives on the same maps; mode 1 within `C.tolerance(distance)` pixels for every distance (4 x the measured error of the
    reference-order fp32 computation); the input unchanged; a second call gives the same bits."""
    from stablekeypoints_amd import eval as E
    from stablekeypoints_amd import ops
    host = torch.from_numpy(C.build(name).copy())
    maps = host.cuda()
    n, h, w = maps.shape
    loc, flat = ops.locate(maps, 0)
    want_loc, want_flat = C.want(name, 0)
    assert flat.dtype == torch.int32 and tuple(loc.shape) == (n, 2)
    assert np.array_equal(flat.cpu().numpy(), want_flat) and np.array_equal(loc.cpu().numpy().astype(np.float64), want_loc)
    if h == w:                                                      # (the token-statistics kernel takes square maps)
        assert torch.equal(loc, E.find_max_pixel(maps))
    for d in C.DISTANCES:
        loc, flat1 = ops.locate(maps, 1, d)
        again, flat2 = ops.locate(maps, 1, d)
        assert torch.equal(flat1, flat) and torch.equal(flat2, flat)
        assert torch.equal(loc.view(torch.int32), again.view(torch.int32)), d
        err = float(np.abs(loc.cpu().numpy().astype(np.float64) - C.want(name, 1, d)[0]).max())
        print(f"{name}, distance {d}: {err:.3e} px (tolerance {C.tolerance(d):.3e})")
        assert err <= C.tolerance(d), (d, err)
    assert torch.equal(maps.cpu(), host)


def test_locate_keypoints_shapes_ledger_and_alignment():
    """A [2,3,5,h,w] input equals the flattened call; one ledger note per call; a map that starts off a 16-byte boundary (the
    scalar-load kernels) gives the same bits as its aligned copy; non-contiguous input is read as its values."""
    from stablekeypoints_amd import eval as E
    from stablekeypoints_amd import ops, routes
    maps = torch.from_numpy(C.build("n70 16x16")[:30].copy()).cuda()
    for strategy, d in (("argmax", 5), ("weighted_avg", 5), ("weighted_avg", -1)):
        flat = E.locate_keypoints(maps, strategy, d)
        before = routes.snapshot()
        got = E.locate_keypoints(maps.view(2, 3, 5, 16, 16), strategy, d)
        assert routes.delta(before) == {("eval.locate", "locate"): 1}
        assert tuple(got.shape) == (2, 3, 5, 2) and got.dtype == torch.float32
        assert torch.equal(got.reshape(-1, 2).view(torch.int32), flat.view(torch.int32))
    for name in ("n3 64x64", "n1 128x128"):
        m = torch.from_numpy(C.build(name).copy()).cuda()
        buf = torch.empty(m.numel() + 1, device="cuda")
        off = buf[1:].view(m.shape)
        off.copy_(m)
        assert off.data_ptr() % 16 == 4
        for mode, d in ((0, 0), (1, 5), (1, -1)):
            a, fa = ops.locate(m, mode, d)
            b, fb = ops.locate(off, mode, d)
            assert torch.equal(fa, fb) and torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, mode, d)
    t = maps.transpose(1, 2)
    assert torch.equal(E.locate_keypoints(t, "weighted_avg"), E.locate_keypoints(t.contiguous(), "weighted_avg"))
    with routes.strict(allow=routes.DOCUMENTED_LIBRARY_ROUTES):
        E.locate_keypoints(maps, "weighted_avg")


def test_refused_arguments_launch_nothing():
    """Bad arguments come back as codes (through `ops.locate`: exceptions) and the outputs keep their contents."""
    from stablekeypoints_amd import _native as N
    from stablekeypoints_amd import ops
    lib = N.lib()
    maps = torch.rand(2, 8, 8, device="cuda")
    loc = torch.full((2, 2), -7.0, device="cuda")
    flat = torch.full((2,), -7, device="cuda", dtype=torch.int32)
    st = torch.cuda.current_stream().cuda_stream
    args = lambda **o: list({**dict(M=maps.data_ptr(), N=2, H=8, W=8, mode=1, distance=5.0, loc=loc.data_ptr(), flat=flat.data_ptr(),
                                    ws=None, ws_bytes=0), **o}.values()) + [st]
    assert lib.skp_locate_f32(*args(mode=3)) == -1 and lib.skp_locate_f32(*args(distance=-4.0)) == -1
    assert lib.skp_locate_f32(*args(N=0)) == -1 and lib.skp_locate_f32(*args(H=5000)) == -2
    assert lib.skp_locate_f32(*args(M=None)) == -1 and lib.skp_locate_f32(*args(flat=None)) == -1
    big = torch.rand(1, 128, 128, device="cuda")
    assert lib.skp_locate_f32(*args(M=big.data_ptr(), N=1, H=128, W=128)) == -1           # split, and no scratch given
    torch.cuda.synchronize()
    assert (loc == -7).all() and (flat == -7).all()
    assert lib.skp_locate_f32(*args()) == 0
    torch.cuda.synchronize()
    assert (flat >= 0).all() and (loc > 0).all()
    with pytest.raises(RuntimeError, match="SKP_E_BADARG"):
        ops.locate(maps, 2)
    with pytest.raises(RuntimeError, match="float32"):
        ops.locate(maps.double())


@pytest.mark.parametrize("shape", [(3, 16, 16), (2, 64, 64), (2, 128, 128)])
def test_a_map_with_nan_stays_inside_the_map(shape):
    """Unspecified values, but the call returns and every index is inside its map: one map that is only NaN, one with NaN
    scattered (its maximum among them), on each branch of the plan."""
    from stablekeypoints_amd import ops
    n, h, w = shape
    g = torch.Generator().manual_seed(h)
    m = torch.rand(n, h, w, generator=g)
    m[0] = float("nan")
    m[1].view(-1)[::3] = float("nan")
    for mode, d in ((0, 0), (1, 5), (1, -1)):
        loc, flat = ops.locate(m.cuda(), mode, d)
        torch.cuda.synchronize()
        assert ((flat >= 0) & (flat < h * w)).all()
        assert int(flat[0]) == 0
        if n > 2:
            assert torch.isfinite(loc[2:]).all()
