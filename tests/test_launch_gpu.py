"""ops._launch, the one checked way ops.py starts a kernel: it launches exactly what the raw ctypes call launches, and it refuses a
wrong tensor BEFORE anything is launched (every refusal below is a Python exception; no kernel sees a bad pointer)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from stablekeypoints_amd import ops
    return ops


def _raw(ops, name, *args):
    ops.N.check(getattr(ops.N.lib(), name)(*args, ops._stream()), name)


def _rand(*shape, seed=0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def test_launch_equals_the_raw_call_bit_for_bit(ops):
    """One entry per argument kind, each against the same entry called through N.lib() with .data_ptr() on the same inputs."""
    # f32 pointers, an int64 count, floats
    n = 1000
    x, z = _rand(n, seed=1), _rand(n, seed=2)
    got, want = torch.full((n,), -7.0, device="cuda"), torch.full((n,), -7.0, device="cuda")
    ops._launch("skp_axpby_f32", x, z, got, n, 0.75, -1.25)
    _raw(ops, "skp_axpby_f32", x.data_ptr(), z.data_ptr(), want.data_ptr(), n, 0.75, -1.25)
    assert torch.equal(got, want) and not bool((got == -7.0).any())
    # a u8 output
    img = _rand(1, 3, 5, 7, seed=3)
    got, want = (torch.zeros(1, 5, 7, 3, device="cuda", dtype=torch.uint8) for _ in range(2))
    ops._launch("skp_image_u8_nhwc_f32", img, got, 1, 5, 7)
    _raw(ops, "skp_image_u8_nhwc_f32", img.data_ptr(), want.data_ptr(), 1, 5, 7)
    assert torch.equal(got, want) and int(got.max()) > 0
    # i32 and i64 pointers: T = 16 tokens on a 24 x 24 grid, 4 candidates, 2 selected
    T, R = 16, 24
    kl = _rand(T, seed=4)
    loc = torch.randint(0, R * R, (T,), generator=torch.Generator().manual_seed(5), dtype=torch.int32).cuda()
    got = [torch.full((k,), -1, device="cuda", dtype=torch.int64) for k in (4, 2)]
    want = [torch.full((k,), -1, device="cuda", dtype=torch.int64) for k in (4, 2)]
    ops._launch("skp_select_tokens", kl, loc, T, R, 4, 2, *got)
    _raw(ops, "skp_select_tokens", kl.data_ptr(), loc.data_ptr(), T, R, 4, 2, want[0].data_ptr(), want[1].data_ptr())
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and int(got[0].min()) >= 0 and int(got[1].min()) >= 0
    # a null pointer: no unconditional output
    m = _rand(n, seed=6)
    got, want = torch.full((n,), -7.0, device="cuda"), torch.full((n,), -7.0, device="cuda")
    ops._launch("skp_ddim_step_f32", x, m, None, got, n, 1, 1.0, 0, 0.8, 0.6, 0.9, 0.4, 0)
    _raw(ops, "skp_ddim_step_f32", x.data_ptr(), m.data_ptr(), None, want.data_ptr(), n, 1, 1.0, 0, 0.8, 0.6, 0.9, 0.4, 0)
    assert torch.equal(got, want) and not bool((got == -7.0).any())
    # a pre-offset integer address: the second half of each buffer, the first half stays as it was
    h = n // 2
    got, want = torch.full((n,), -7.0, device="cuda"), torch.full((n,), -7.0, device="cuda")
    ops._launch("skp_axpby_f32", x.data_ptr() + 4 * h, z[h:], got.data_ptr() + 4 * h, h, 2.0, 3.0)
    _raw(ops, "skp_axpby_f32", x.data_ptr() + 4 * h, z.data_ptr() + 4 * h, want.data_ptr() + 4 * h, h, 2.0, 3.0)
    assert torch.equal(got, want) and bool((got[:h] == -7.0).all()) and torch.equal(got[h:], 2.0 * x[h:] + 3.0 * z[h:])


def test_a_wrong_dtype_is_refused_before_launching(ops):
    """skp_axpby_f32 declares `void*` operands (include/skp.h), so its slots are untyped and the table cannot hold a dtype against them;
    the same refusal is shown on the float* slots of skp_ddim_step_f32, and for axpby at its public wrapper.  The output keeps its
    sentinel: nothing ran."""
    n = 1000
    x, m = _rand(n, seed=1), _rand(n, seed=2)
    bad = torch.ones(n, device="cuda", dtype=torch.int32)
    out = torch.full((n,), -7.0, device="cuda")
    for args in ((bad, m, None, out), (x, bad, None, out), (x, m, bad, out)):
        with pytest.raises(RuntimeError, match=r"skp_ddim_step_f32: argument \d: expected torch.float32, got torch.int32"):
            ops._launch("skp_ddim_step_f32", *args, n, 1, 1.0, 0, 0.8, 0.6, 0.9, 0.4, 0)
    with pytest.raises(RuntimeError, match="skp_ddim_step_f32: argument 3: expected torch.float32, got torch.int32"):
        ops._launch("skp_ddim_step_f32", x, m, None, bad, n, 1, 1.0, 0, 0.8, 0.6, 0.9, 0.4, 0)
    with pytest.raises(RuntimeError, match="expected float32"):
        ops.axpby(bad, x, 1.0, 1.0)
    with pytest.raises(TypeError, match="skp_axpby_f32: takes 6 arguments and the stream, got 7"):
        ops._launch("skp_axpby_f32", x, m, out, n, 1.0, 1.0, 0)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((bad == 1).all())


def test_index_tensors_of_the_wrong_width_are_refused(ops):
    """The kernels read `sel` as int64 and the arg-max locations as int32; the other width raises instead of being read as such."""
    T, R, K = 16, 24, 2
    M, Mt = _rand(T, R, R, seed=1), _rand(T, R, R, seed=2)
    am, kl = ops.token_stats(M, 1, want_kl=True)
    sel = torch.tensor([3, 9], device="cuda")
    theta = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    sharp, equiv = ops.fused_losses(M, Mt, sel, am, theta, 2.0, 1)                      # what the kernel asks for passes
    assert bool(torch.isfinite(sharp)) and bool(torch.isfinite(equiv))
    with pytest.raises(RuntimeError, match="skp_losses_fwd_f32: argument 2: expected torch.int64, got torch.int32"):
        ops.fused_losses(M, Mt, sel.int(), am, theta, 2.0, 1)
    with pytest.raises(RuntimeError, match="skp_losses_fwd_f32: argument 6: expected torch.int32, got torch.int64"):
        ops.LossesFn.apply(M, Mt, sel, am.long(), theta, 2.0, 1)
    cand, picked = ops.select_tokens(kl, am[0], R, 4, K)
    assert cand.shape == (4,) and picked.shape == (K,)
    with pytest.raises(RuntimeError, match="skp_select_tokens: argument 1: expected torch.int32, got torch.int64"):
        ops.select_tokens(kl, am[0].long(), R, 4, K)
    with pytest.raises(RuntimeError, match="skp_select_tokens: argument 0: expected torch.float32, got torch.float64"):
        ops.select_tokens(kl.double(), am[0], R, 4, K)
    torch.cuda.synchronize()


def test_lab_probe_takes_its_host_pointer(ops):
    """The one raw call ops.py keeps: tools/csrc/skp_lab.h's probe writes its result through a [host] float*."""
    rate = ops.mfma_issue_rate(1, iters=2000)
    assert 1.0 < rate < 1000.0, rate                # TFLOP/s of fp32 MFMA issue: tens, on any healthy device


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible devices")
def test_a_tensor_on_another_device_is_refused(ops):
    n = 1000
    torch.cuda.set_device(0)
    x, z = _rand(n, seed=1), _rand(n, seed=2)
    out = torch.full((n,), -7.0, device="cuda:0")
    with pytest.raises(RuntimeError, match="skp_axpby_f32: argument 1: expected a tensor on the current device cuda:0"):
        ops._launch("skp_axpby_f32", x, z.to("cuda:1"), out, n, 1.0, 1.0)
    far = torch.full((n,), -7.0, device="cuda:1")
    with pytest.raises(RuntimeError, match="skp_axpby_f32: argument 2: expected a tensor on the current device cuda:0"):
        ops._launch("skp_axpby_f32", x, z, far, n, 1.0, 1.0)
    torch.cuda.synchronize(0)
    torch.cuda.synchronize(1)
    assert bool((out == -7.0).all()) and bool((far == -7.0).all())
