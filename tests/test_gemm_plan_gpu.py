"""KERNEL_TIMER books the LinearD8 launches under the names the library's plans give them (octic_linear_d8_plan,
octic_linear_d8_wgrad_plan) - also under OCTIC_ROUTE_LINEAR_RING, where the hand-kept copy in ops.py used to book the
W-stationary kernel while the ring kernel ran.  Smallest shapes that reach each branch; the numerics of these paths are held
by test_wreg_gpu.py, test_kernels_gpu.py and test_fullsize_gpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
bf, f32 = torch.bfloat16, torch.float32


def _linear_fwd(M, cin, cout, dtype):
    from octic_vits_amd import ops
    g = torch.Generator(device=DEV).manual_seed(M + cin + cout)
    x = torch.randn(M, 8 * cin, generator=g, device=DEV).to(dtype)
    w = [torch.randn(cout, cin, generator=g, device=DEV).to(dtype) for _ in range(4)]
    w.append(torch.randn(2 * cout, 2 * cin, generator=g, device=DEV).to(dtype))
    y = torch.empty((M, 8 * cout), device=DEV, dtype=dtype)
    ops.linear_fwd(ops.pview(x, cin), w, None, ops.pview(y, cout), M, cin, cout, dtype, dtype, x)


def _linear_wgrad(M, cin, cout, dtype):
    from octic_vits_amd import ops
    g = torch.Generator(device=DEV).manual_seed(M + cin + cout)
    x = torch.randn(M, 8 * cin, generator=g, device=DEV).to(dtype)
    dy = torch.randn(M, 8 * cout, generator=g, device=DEV).to(dtype)
    ops.linear_wgrad(ops.pview(x, cin), ops.pview(dy, cout), M, cin, cout, dtype, x)


def _wgrad_tiled_name(M, cin, cout):
    from octic_vits_amd import _lib
    kernel, tile, _, colsum = _lib.plan("octic_linear_d8_wgrad_plan", M, cin, cout, _lib.BF16)
    assert (kernel, colsum) == (_lib.WGRAD_TILED, 0)
    return "wgrad_kernel<bf16,%d>" % (tile // 32)


@pytest.mark.parametrize("call,dtype,shape,ring_knob,want", [
    (_linear_fwd, bf, (96, 32, 32), 0, "linear_d8_wreg_kernel<bf16,0>"),
    (_linear_fwd, bf, (96, 32, 32), 1, "linear_d8_ring_kernel<bf16,bf16,0>"),
    (_linear_fwd, f32, (64, 24, 24), 0, "linear_d8_kernel<f32,f32>"),
    (_linear_fwd, f32, (64, 32, 24), 0, "linear_d8_ring_kernel<f32,f32,0>"),
    (_linear_wgrad, bf, (257, 160, 160), 0, "wgrad_ring_kernel<bf16>"),
    (_linear_wgrad, bf, (96, 32, 32), 0, _wgrad_tiled_name),
])
def test_kernel_timer_names_what_the_gemm_plans_say(call, dtype, shape, ring_knob, want):
    from octic_vits_amd import _lib, ops
    if callable(want):
        want = want(*shape)
    try:
        _lib.route_override(_lib.ROUTE_LINEAR_RING, ring_knob)
        ops.KERNEL_TIMER.enable()
        call(*shape, dtype)
        torch.cuda.synchronize()
        names = [r[0] for r in ops.KERNEL_TIMER.records]
    finally:
        ops.KERNEL_TIMER.disable()
        _lib.route_override(_lib.ROUTE_LINEAR_RING, 0)
    assert names == [want]
