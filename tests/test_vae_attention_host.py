"""The VAE mid-block attention route (one head of d = 512) without a GPU: the truth table of `ops.vae_attn_route`, the route
ledger's registration, and the C entry points of csrc/skp_flash_attn_wide.hip answering shapes and bad arguments on the host."""
import ctypes as C
import itertools
import os
import re

import pytest

from stablekeypoints_amd import _native as N
from stablekeypoints_amd import ops, routes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("skp_flash_attn_fwd_wide_ok", "skp_flash_attn_fwd_wide_workspace", "skp_flash_attn_fwd_wide_f32")
KEYS = (576, 4096, 8192, 16384)


def test_defaults():
    assert ops.VAE_ATTN_MODE == "auto" and ops.VAE_FLASH_MIN_KEYS >= 8192


@pytest.mark.parametrize("mode", ["auto", "flash", "lib"])
def test_route_truth_table(monkeypatch, mode):
    monkeypatch.setattr(ops, "VAE_ATTN_MODE", mode)
    monkeypatch.setattr(ops, "VAE_FLASH_MIN_KEYS", 8192)
    for keys, d, needs_grad in itertools.product(KEYS, (512, 256), (False, True)):
        want = "lib_core"
        if d == 512 and not needs_grad and (mode == "flash" or (mode == "auto" and keys >= 8192)):
            want = "flash_wide"
        for B, heads in ((1, 1), (8, 1), (2, 2)):
            assert ops.vae_attn_route(B, heads, keys, d, needs_grad) == want, (mode, B, heads, keys, d, needs_grad)


def test_auto_keeps_the_512sq_shapes_on_the_library(monkeypatch):
    monkeypatch.setattr(ops, "VAE_ATTN_MODE", "auto")
    assert ops.vae_attn_route(8, 1, 4096, 512, False) == "lib_core"        # the step's encode (tests/test_routes_gpu.py pins it)
    assert ops.vae_attn_route(1, 1, 4096, 512, False) == "lib_core"        # the 512^2 decode (tests/test_generate_gpu.py)
    monkeypatch.setattr(ops, "VAE_FLASH_MIN_KEYS", 1 << 20)
    assert ops.vae_attn_route(1, 1, 16384, 512, False) == "lib_core"       # the threshold is read at call time
    monkeypatch.setattr(ops, "VAE_ATTN_MODE", "flash")
    assert ops.vae_attn_route(1, 1, 576, 512, False) == "flash_wide"


def test_unknown_mode_raises(monkeypatch):
    monkeypatch.setattr(ops, "VAE_ATTN_MODE", "fast")
    with pytest.raises(ValueError):
        ops.vae_attn_route(1, 1, 16384, 512, False)


def test_cpu_tensors_raise():
    import torch
    x = torch.zeros(1, 16, 512)
    with pytest.raises(RuntimeError):
        ops.flash_attn_wide(x, x, x, 1, 0.1)


def test_routes_registration():
    assert routes.kind("vae.attention", "flash_wide") == "hip"
    assert routes.kind("vae.attention", "lib_core") == "library"
    assert ("vae.attention", "lib_core") in routes.DOCUMENTED_LIBRARY_ROUTES
    assert ("vae.attention", "flash_wide") not in routes.DOCUMENTED_LIBRARY_ROUTES
    before = routes.snapshot()
    routes.note("vae.attention", "flash_wide")
    assert routes.delta(before) == {("vae.attention", "flash_wide"): 1}
    routes.merge({("vae.attention", "flash_wide"): 1}, times=-1)


def test_symbols_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "skp.h")).read()
    lib = N.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/skp.h"
        assert hasattr(lib, name) and name in N.SIGNATURES
    assert lib.skp_flash_attn_fwd_wide_workspace.restype is C.c_int64
    assert lib.skp_abi_version() == N.ABI_VERSION >= 42


def test_ok_answers_shapes():
    ok = N.lib().skp_flash_attn_fwd_wide_ok
    for B, H, n in ((1, 1, 1), (1, 1, 17), (2, 1, 200), (1, 2, 77), (8, 1, 4096), (1, 1, 65536)):
        assert ok(B, B, H, n, n, 512) == 1
    assert ok(2, 2, 1, 100, 300, 512) == 1                                  # the key count is its own argument
    for d in (40, 64, 80, 160, 256):
        assert ok(2, 2, 1, 200, 200, d) == 0
    assert ok(2, 1, 1, 200, 200, 512) == 0 and ok(2, 3, 1, 200, 200, 512) == 0      # Bk != B
    for bad in ((0, 0, 1, 8, 8), (1, 1, 0, 8, 8), (1, 1, 1, 0, 8), (1, 1, 1, 8, 0), (-1, -1, 1, 8, 8), (1, 1, 1, -8, 8)):
        assert ok(*bad, 512) == 0, bad


REFUSED = [(2, 2, 1, 200, 200, d) for d in (40, 64, 80, 160, 256)] + [
    (2, 1, 1, 200, 200, 512), (0, 0, 1, 8, 8, 512), (1, 1, 0, 8, 8, 512), (1, 1, 1, 0, 8, 512), (1, 1, 1, 8, 0, 512),
    (1, 1, 1, 8, 8, 0), (1, 1, 1, 8, 8, -512)]


def test_launch_entry_refuses_before_launching():
    """No GPU here: an entry that reached a launch (or any other runtime call) could not answer with an SKP_E_* code."""
    lib = N.lib()
    room = (C.c_float * 16)()
    base = (C.addressof(room) + 15) & ~15                                   # a 16-byte aligned host address (never dereferenced)
    p = C.c_void_p(base)
    good = (1, 1, 1, 8, 8, 512)
    for i in range(4):                                                      # q, k, v, out null in turn (workspace may be null)
        ptrs = [p, p, p, p]
        ptrs[i] = None
        assert lib.skp_flash_attn_fwd_wide_f32(*ptrs, None, *good, 0.1, None) == -1
    for shape in REFUSED:
        assert lib.skp_flash_attn_fwd_wide_ok(*shape) == 0
        assert lib.skp_flash_attn_fwd_wide_f32(p, p, p, p, None, *shape, 0.1, None) in (-1, -2), shape
        assert lib.skp_flash_attn_fwd_wide_workspace(*shape) < 0, shape
    misaligned = C.c_void_p(base + 4)
    assert lib.skp_flash_attn_fwd_wide_f32(misaligned, p, p, p, None, *good, 0.1, None) == -1


def test_workspace_is_small():
    ws = N.lib().skp_flash_attn_fwd_wide_workspace
    for B, H, n in ((1, 1, 17), (2, 1, 200), (1, 2, 77), (8, 1, 4096), (1, 1, 4096), (2, 1, 9216), (1, 1, 16384), (1, 1, 65536)):
        nbytes = ws(B, B, H, n, n, 512)
        out_bytes = B * n * H * 512 * 4
        assert 0 <= nbytes <= 4 * out_bytes + 64 * B * H * n, (B, H, n, nbytes)
