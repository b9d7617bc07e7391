"""The Winograd weight gradient's owner store (csrc/conv3d.hip: WgOut.store,
wg_settle).  The Winograd-domain gradient dW_hat lives in the caller's
workspace and is never zero-filled by the entry itself: a point GEMM that
settles on one m-split of a plain grid stores each tile from its single owner,
every accumulating form (stream-K, m-splits with atomics, deterministic
partials) fills dW_hat first.  So with the workspace poisoned with NaN

* every single-owner kernel must write every (point, k, n), ragged edge tiles
  included, in both modes, and the two modes run the same reduction in the
  same workgroup: bit-equal results;
* an accumulating launch must still see zeros;
* the public C += A^T B entry must keep adding into the caller's C.

The reference is tests/convref.py's float64 weight gradient; the bound is the
one test_gpu_conv.py::test_wino_weight_gradient_accuracy holds the Winograd
weight gradient to, 2e-5 of the gradient's scale (measured on an MI355X: at
most 5.8e-6 over the single-owner cases, 9.7e-6 / 9.4e-6 for the stream-K /
partials launch)."""
import numpy as np
import pytest
import torch

import convref as R

pytestmark = pytest.mark.gpu

WINO_WGRAD_RTOL = 2e-5          # test_wino_weight_gradient_accuracy's bound


@pytest.fixture
def det(cuda):
    from m3d import _lib
    yield _lib
    _lib.set_deterministic(False)


# (Cin, Cout) -> the point-GEMM kernel of bwd_weight_wino
PAIRS = [(64, 64),       # x3_wgrad64_kernel
         (128, 128),     # x3_wgrad_kernel
         (128, 64),      # conv_wgrad_kernel<128, 64>, batched over the points
         (192, 192),     # x3_wgrad_tr_kernel, one partial 256 x 256 tile
         (256, 512)]     # x3_wgrad_tr_kernel, two full tiles
# (B, H, W, D) -> T tiles of F(4x2x4): 4 (less than one k-step), 18 (ragged on
# every axis), 32, and a batch of two (T = 8)
VOLUMES = [(1, 4, 4, 8), (1, 6, 6, 10), (1, 8, 8, 16), (2, 4, 4, 8)]
CASES = [(ci, co, v) for ci, co in PAIRS for v in VOLUMES[:3]] + [(192, 192, VOLUMES[3]), (64, 64, VOLUMES[3])]


def _inputs(cin, cout, vol, cuda):
    B, H, W, D = vol
    g = torch.Generator().manual_seed(1000 * cin + cout + 7 * H * W * D + B)
    x = torch.randn((B, H, W, D, cin), generator=g)
    dz = torch.randn((B, H, W, D, cout), generator=g)
    dw0 = torch.randn((3, 3, 3, cin, cout), generator=g)
    grad = R.conv_bwd_weight(x.numpy(), dz.numpy(), (3, 3, 3), (1, 1, 1), (1, 1, 1), (H, W, D),
                             np.zeros(dw0.shape))
    return x.to(cuda), dz.to(cuda), dw0.to(cuda), grad


def _poisoned_ws(L, vol, cin, cout, cuda):
    B, H, W, D = vol
    nb = int(L.m3d_conv3d_wino_workspace_bytes(B, H, W, D, D, cin, cout))
    return torch.full((nb // 4 + 1,), float("nan"), device=cuda), nb


def _wgrad(L, _lib, x, dz, dw0, cuda):
    """dw0 + the gradient through m3d_conv3d_bwd_weight_wino, workspace all NaN"""
    B, H, W, D, cin = x.shape
    cout = dz.shape[4]
    ws, nb = _poisoned_ws(L, (B, H, W, D), cin, cout, cuda)
    dw = dw0.clone()
    _lib.check(L.m3d_conv3d_bwd_weight_wino(x.data_ptr(), dz.data_ptr(), B, H, W, D, cin, cout, D, 1,
                                            dw.data_ptr(), ws.data_ptr(), nb, _lib.stream()), "wino wgrad")
    torch.cuda.synchronize()
    return dw


def _wgrad_u(L, _lib, x, dz, dw0, cuda):
    """the same through m3d_conv3d_bwd_weight_wino_u on the U that
    m3d_conv3d_fwd_wino_keep kept (None where the build keeps no U); the
    workspace is poisoned again after the forward"""
    B, H, W, D, cin = x.shape
    cout = dz.shape[4]
    ub = int(L.m3d_conv3d_wino_u_bytes(B, H, W, D, cin))
    if ub == 0:
        return None
    ws, nb = _poisoned_ws(L, (B, H, W, D), cin, cout, cuda)
    u = torch.empty(ub // 4, device=cuda)
    w = torch.zeros((3, 3, 3, cin, cout), device=cuda)
    y = torch.empty((B, H, W, D, cout), device=cuda)
    _lib.check(L.m3d_conv3d_fwd_wino_keep(x.data_ptr(), B, H, W, D, cin, w.data_ptr(), cout, D, 1, None, None,
                                          None, None, 0, None, y.data_ptr(), u.data_ptr(), ws.data_ptr(), nb,
                                          _lib.stream()), "fwd keep")
    ws.fill_(float("nan"))
    dw = dw0.clone()
    _lib.check(L.m3d_conv3d_bwd_weight_wino_u(u.data_ptr(), dz.data_ptr(), B, H, W, D, cin, cout, D, 1,
                                              dw.data_ptr(), ws.data_ptr(), nb, _lib.stream()), "wino wgrad u")
    torch.cuda.synchronize()
    return dw


def _check(dw, dw0, grad, what):
    """finite, and within the Winograd bound of dw0 + the float64 gradient
    (the scale is the gradient's own, not that of the preloaded dw0)"""
    assert bool(torch.isfinite(dw).all()), f"{what}: non-finite weight gradient"
    got = dw.double().cpu().numpy()
    want = dw0.double().cpu().numpy() + grad
    scale = float(np.abs(grad).max())
    err = float(np.abs(got - want).max())
    print(f"{what}: max err {err:.3e}, scale {scale:.3e} (rel {err / scale:.2e})")
    assert err <= WINO_WGRAD_RTOL * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


@pytest.mark.parametrize("cin,cout,vol", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_single_owner_store(det, cuda, cin, cout, vol):
    _lib = det
    L = _lib.load()
    x, dz, dw0, grad = _inputs(cin, cout, vol, cuda)
    for name, run in (("wino", _wgrad), ("wino_u", _wgrad_u)):
        _lib.set_deterministic(False)
        plain = run(L, _lib, x, dz, dw0, cuda)
        if plain is None:                   # the build keeps no U (forward and wgrad tiles differ)
            continue
        _lib.set_deterministic(True)
        fixed = run(L, _lib, x, dz, dw0, cuda)
        what = f"{name} {cin}->{cout} {vol}"
        _check(plain, dw0, grad, what)
        _check(fixed, dw0, grad, what + " deterministic")
        # one split in both modes: the same workgroup reduces the same rows in the same order
        assert torch.equal(plain, fixed), what


def test_accumulating_launch_still_zero_fills(det, cuda):
    """192 -> 192 on 16 x 16 x 64: T = 512 rows, the stream-K form outside
    deterministic mode and two m-splits through the partials inside it.  Both
    add into dW_hat, so the launcher's fill must have run."""
    _lib = det
    L = _lib.load()
    vol = (1, 16, 16, 64)
    x, dz, dw0, grad = _inputs(192, 192, vol, cuda)
    _lib.set_deterministic(False)
    _check(_wgrad(L, _lib, x, dz, dw0, cuda), dw0, grad, "stream-K 192->192")
    _lib.set_deterministic(True)
    _check(_wgrad(L, _lib, x, dz, dw0, cuda), dw0, grad, "partials 192->192")


def test_public_wgrad_gemm_keeps_accumulating(cuda):
    """m3d_gemm_wgrad_f32 is C += A^T B whatever the split: at M = 64 its one
    m-split is a single-owner launch, and it must add to the caller's C (never
    the store).  1e-5 of the scale, as test_wgrad_gemm_stream_k_shapes."""
    from m3d import _lib
    L = _lib.load()
    nb, M, K, N = 3, 64, 256, 256
    g = torch.Generator(device=cuda).manual_seed(17)
    A = torch.randn((nb, M, K), device=cuda, generator=g)
    Bm = torch.randn((nb, M, N), device=cuda, generator=g)
    C = torch.randn((nb, K, N), device=cuda, generator=g) * 8 + 3
    ref = torch.baddbmm(C.double(), A.double().transpose(1, 2), Bm.double())
    _lib.check(L.m3d_gemm_wgrad_f32(A.data_ptr(), Bm.data_ptr(), C.data_ptr(), nb, M, K, N, _lib.stream()),
               "gemm_wgrad")
    err = float((C.double() - ref).abs().max()) / float(ref.abs().max())
    assert err < 1e-5, err
