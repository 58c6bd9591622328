"""Algebra of the polyphase Winograd F(4x4,2x2) form of the 3x3 / stride-2 convolution (skp_conv_s2w.hip), in numpy fp64,
independent of the kernel: the phase split, the transform matrices and the structural zeros of the transformed phase filters."""
import numpy as np
import pytest

# interpolation points 0, 1, -1, 2, inf
BT = np.array([[2, -1, -2, 1, 0],
               [0, -2, -1, 1, 0],
               [0, 2, -3, 1, 0],
               [0, -1, 0, 1, 0],
               [0, 2, -1, -2, 1]], dtype=np.float64)
G = np.array([[1 / 2, 0],
              [-1 / 2, -1 / 2],
              [-1 / 6, 1 / 6],
              [1 / 6, 1 / 3],
              [0, 1]], dtype=np.float64)
AT = np.array([[1, 1, 1, 1, 0],
               [0, 1, -1, 2, 0],
               [0, 1, 1, 4, 0],
               [0, 1, -1, 8, 1]], dtype=np.float64)

# 1-D taps of the two phases: the two-tap phase sees (w0, w2), the one-tap phase (w1, 0).  With base = 2 i - pad the two-tap
# phase is x[base + 2 k] and the one-tap phase x[base + 2 k + 1], for both paddings (pad 0: even / odd, pad 1: shifted odd / even).
TAPS = ((0, 2), (1, None))


def phase_filter(w, rp, cp):
    """2x2 filter that phase (rp, cp) of the input sees; w is one 3x3 filter."""
    g = np.zeros((2, 2))
    for a, ra in enumerate(TAPS[rp]):
        for b, cb in enumerate(TAPS[cp]):
            if ra is not None and cb is not None:
                g[a, b] = w[ra, cb]
    return g


def conv_s2_ref(x, w, pad):
    """x [C, H, W], w [C, 3, 3] -> [H/2, W/2]; pad 0 = zero extension by (0,1,0,1), pad 1 = symmetric."""
    C, H, W = x.shape
    xp = np.zeros((C, H + 2, W + 2))
    if pad:
        xp[:, 1:H + 1, 1:W + 1] = x
    else:
        xp[:, :H, :W] = x
    y = np.zeros((H // 2, W // 2))
    for oy in range(H // 2):
        for ox in range(W // 2):
            y[oy, ox] = np.sum(xp[:, 2 * oy:2 * oy + 3, 2 * ox:2 * ox + 3] * w)
    return y


def conv_s2_polyphase(x, w, pad):
    C, H, W = x.shape
    OH, OW = H // 2, W // 2
    ext = np.zeros((C, H + 12, W + 12))                    # zero extension; image origin at (2, 2)
    ext[:, 2:H + 2, 2:W + 2] = x
    y = np.zeros((OH, OW))
    for ty in range(OH // 4):
        for tx in range(OW // 4):
            M = np.zeros((5, 5))
            for c in range(C):
                for rp in range(2):
                    for cp in range(2):
                        r0, c0 = 8 * ty - pad + rp + 2, 8 * tx - pad + cp + 2
                        d = ext[c, r0:r0 + 10:2, c0:c0 + 10:2]
                        M += (G @ phase_filter(w[c], rp, cp) @ G.T) * (BT @ d @ BT.T)
            y[4 * ty:4 * ty + 4, 4 * tx:4 * tx + 4] = AT @ M @ AT.T
    return y


@pytest.mark.parametrize("pad", [0, 1])
def test_polyphase_winograd_reproduces_stride2_conv(pad):
    rng = np.random.default_rng(7 + pad)
    x = rng.standard_normal((2, 12, 12))
    # 12 x 12 input -> 6 x 6 output; the tiling wants multiples of 4 outputs, so the image is embedded into 16 x 16 zeros
    # (which is what the zero extension is anyway): the 6 x 6 corner of that result is the small image's convolution
    x16 = np.zeros((2, 16, 16))
    x16[:, :12, :12] = x
    w = rng.standard_normal((2, 3, 3))
    got = conv_s2_polyphase(x16, w, pad)
    ref = conv_s2_ref(x16, w, pad)
    assert np.max(np.abs(got - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))
    small = conv_s2_ref(x, w, pad)
    assert np.max(np.abs(got[:6, :6] - small)) <= 1e-12 * max(1.0, np.max(np.abs(small)))


def test_transformed_phase_filters_have_19_structural_zero_blocks():
    rng = np.random.default_rng(11)
    zeros = 0
    for rp in range(2):
        for cp in range(2):
            acc = np.zeros((5, 5), dtype=bool)
            for _ in range(8):
                U = G @ phase_filter(rng.standard_normal((3, 3)), rp, cp) @ G.T
                acc |= U != 0.0
            expect = np.ones((5, 5), dtype=bool)
            if rp:
                expect[4, :] = False                       # the inf row picks the (zero) last vertical tap
            if cp:
                expect[:, 4] = False
            assert np.array_equal(acc, expect), (rp, cp)
            zeros += int((~acc).sum())
    assert zeros == 19                                     # 0 + 5 + 5 + 9: 81 of the 100 (position, phase) blocks remain
