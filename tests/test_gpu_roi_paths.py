"""Every CropAndResize3D / PyramidROIAlign kernel path of csrc/roi_align.hip at
small shapes, against the CPU oracle (forward and deterministic backward:
bit-exact) and tests/roiref.py (atomic backward: the derived bound
(cnt + 4) * 2^-24 * abs64 and the touched-voxel set).

Which test reaches which path (dispatch of m3d_crop_and_resize3d_*,
pyramid_fwd_impl, m3d_pyramid_roi_align3d_bwd{,_det}, launch_det_bwd):

* line_fwd_sl_kernel<8>, no wave sort (C == 256, pd < 14, lines < 16384):
  test_pyramid_forward_bit_exact[256-pool0] (7,7,7) and [256-pool4] (1,5,1,
  140 lines: not a multiple of 8 slices x 4 waves)
* line_fwd_sl_kernel<8> + wave_key / excl_scan / line_scatter:
  test_pyramid_forward_bit_exact[256-pool1] (3,2,14) and [256-pool2]
  (14,14,14) by pd >= 14, [256-pool3] (25,25,1) by lines = 17500 >= 16384
* the same without a workspace (m3d_pyramid_roi_align3d_fwd):
  test_pyramid_forward_without_workspace[pool0] / [pool1]
* line_fwd_kernel<true> (C % 4 == 0, C != 256):
  test_pyramid_forward_bit_exact[64-pool5], [512-pool6] (two lane passes),
  [320-pool7] (a partial second pass)
* pyramid_fwd_kernel (C % 4 != 0): test_pyramid_forward_bit_exact[6-pool8],
  [70-pool9]
* line_fwd_kernel<false> with more than 64 float4 per voxel:
  test_crop_forward_trilinear_bit_exact[320-*], [512-*] ([256-*]: exactly 64)
* crop_fwd_kernel, trilinear scalar branch:
  test_crop_forward_trilinear_bit_exact[6-*], [70-*]
* gather_bwd_kernel<CQ,true>, CQ = 1, 2, 4, 8:
  test_pyramid_backward_within_bound[64-pool0], [128-pool1], [256-pool2],
  [512-pool3]
* gather_bwd_kernel<8,false>: test_crop_grad_image_c512
* pyramid_bwd_kernel (atomic scatter): test_pyramid_backward_within_bound
  [8-pool4], [6-pool5], [70-pool6], [256-pool7] (pool 33 > 32 at C = 256),
  [8-pool8] and test_pyramid_backward_deterministic[8-pool8] (pool 65: the
  deterministic mode falls back to it)
* m3d_pyramid_roi_align3d_bwd_det: test_pyramid_backward_deterministic, every
  case but [8-pool8]
* crop_bwd_det_kernel<4> / <1> (N > DET_CAP boxes):
  test_crop_grad_image_det_many_boxes[4] / [3]

All inputs are seeded and generated at run time.  Every pyramid case uses two
images, so a batch offset error (n / N) cannot hide, and every level holds at
least two ROIs of each image (asserted).
"""
import functools

import numpy as np
import pytest
import torch

import roiref
from oracle import ops_ref as R
from test_gpu_roi_nms import _det_case

pytestmark = pytest.mark.gpu

B, N = 2, 14
SHAPES = [(16, 16, 8), (8, 8, 8), (4, 4, 8), (2, 2, 8)]          # P2..P5 (H, W, D)
SIDES = (0.08, 0.12, 0.25, 0.3, 0.5, 0.6, 0.85, 0.95)
META_COLS = 12


def T(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)         # a copy: the cached inputs are read-only


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _pyr_input():
    """boxes [B,N,6], meta [B,12], and roi_prepare's boxes_adj / levels."""
    rng = np.random.default_rng(1405)
    boxes = np.zeros((B, N, 6), np.float32)
    for b in range(B):
        for i, s in enumerate(SIDES):                      # cubes at random offsets
            lo = rng.uniform(0, 1 - s, 3)
            boxes[b, i] = np.concatenate([lo, lo + s])
        boxes[b, 8] = [0, 0, 0, 1, 1, 1]                   # last samples round past S-1: extrapolated zeros
        c = rng.uniform(0.2, 0.8, 3)
        boxes[b, 9] = np.concatenate([c, c])               # zero extent
        boxes[b, 10] = 0                                   # ProposalLayer padding row
        boxes[b, 11] = np.array([-0.2, -0.1, -0.3, 0.5, 0.6, 0.4]) + rng.uniform(0, 0.05, 6)   # outside [0,1]
        lo = rng.uniform(0.2, 0.4, 3)
        boxes[b, 12] = np.concatenate([lo + 0.4, lo])      # flipped
        lo = rng.uniform(0.1, 0.8, 3)
        boxes[b, 13] = np.concatenate([lo, lo + [1 / 15, 1 / 15, 1 / 7]])   # about one P2 voxel
    meta = np.zeros((B, META_COLS), np.float32)
    meta[:, 5:8] = (512, 512, 256)
    prep = [R.roi_prepare(boxes[b], meta[b, 5:8]) for b in range(B)]
    adj = np.stack([p[0] for p in prep])
    lev = np.stack([p[1] for p in prep])
    # every level populated in every image, or the cases below compare nothing there
    for b in range(B):
        per_level = [int((lev[b] == l).sum()) for l in (2, 3, 4, 5)]
        assert min(per_level) >= 2, per_level
    return _ro(boxes), _ro(meta), _ro(adj), _ro(lev)


@functools.lru_cache(maxsize=4)
def _maps(C, nonfinite):
    rng = np.random.default_rng([C, 77])
    maps = [rng.normal(size=(B, *s, C)).astype(np.float32) for s in SHAPES]
    if nonfinite:                                          # the scrub path: the oracle zeroes such outputs
        for m in maps:
            flat = m.reshape(-1)
            pos = rng.choice(flat.size, 12, replace=False)
            flat[pos] = np.tile(np.array([np.inf, -np.inf, np.nan], np.float32), 4)
    return tuple(_ro(m) for m in maps)


@functools.lru_cache(maxsize=2)
def _fwd_want(C, pool):
    boxes, meta, _, _ = _pyr_input()
    maps = _maps(C, True)
    want = R.pyramid_roi_align(boxes, meta, list(maps), pool)
    clean = R.pyramid_roi_align(boxes, meta, [np.nan_to_num(m, nan=0.0, posinf=0.0, neginf=0.0) for m in maps], pool)
    assert np.isfinite(want).all()
    assert (want != clean).any(), "no output sample reads a non-finite voxel: the scrub path is not driven"
    return _ro(want)


def _fptrs(tensors):
    from m3d import _lib
    ptrs = (_lib.c_p * 4)(*[t.data_ptr() for t in tensors])
    shape = ((_lib.c_i64 * 3) * 4)(*[(_lib.c_i64 * 3)(*t.shape[1:4]) for t in tensors])
    return ptrs, shape


FWD_CASES = [(256, (7, 7, 7)), (256, (3, 2, 14)), (256, (14, 14, 14)), (256, (25, 25, 1)), (256, (1, 5, 1)),
             (64, (7, 7, 7)), (512, (3, 3, 3)), (320, (2, 3, 4)), (6, (3, 3, 3)), (70, (2, 2, 5))]


@pytest.mark.parametrize("C,pool", FWD_CASES)
def test_pyramid_forward_bit_exact(cuda, C, pool):
    from m3d import ops
    boxes, meta, adj, lev = _pyr_input()
    want = _fwd_want(C, pool)
    out, badj, blev = ops.pyramid_roi_align(T(boxes, cuda), T(meta, cuda), [T(m, cuda) for m in _maps(C, True)],
                                            pool, return_levels=True)
    np.testing.assert_array_equal(blev.cpu().numpy(), lev)
    np.testing.assert_array_equal(badj.cpu().numpy(), adj)
    np.testing.assert_array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("pool", [(7, 7, 7), (3, 2, 14)])
def test_pyramid_forward_without_workspace(cuda, pool):
    """The C entry without a workspace (launch order instead of the wave sort)."""
    from m3d import _lib, ops
    C = 256
    boxes, meta, adj, lev = _pyr_input()
    tb, tm, maps = T(boxes, cuda), T(meta, cuda), [T(m, cuda) for m in _maps(C, True)]
    out_ws, adj_ws, lev_ws = ops.pyramid_roi_align(tb, tm, maps, pool, return_levels=True)
    out = torch.full((B, N, *pool, C), float("nan"), device=cuda)
    badj = torch.full((B, N, 6), float("nan"), device=cuda)
    blev = torch.full((B, N), -1, dtype=torch.int32, device=cuda)
    fptrs, fshape = _fptrs(maps)
    _lib.check(_lib.load().m3d_pyramid_roi_align3d_fwd(fptrs, fshape, C, _lib.ptr(tb), _lib.ptr(tm), META_COLS, B, N,
                                                       *pool, _lib.ptr(out), _lib.ptr(badj), _lib.ptr(blev),
                                                       _lib.stream()), "pyramid_roi_align3d_fwd")
    assert torch.equal(blev, lev_ws) and torch.equal(badj, adj_ws)
    np.testing.assert_array_equal(blev.cpu().numpy(), lev)
    np.testing.assert_array_equal(badj.cpu().numpy(), adj)
    np.testing.assert_array_equal(out.cpu().numpy(), out_ws.cpu().numpy())
    np.testing.assert_array_equal(out.cpu().numpy(), _fwd_want(C, pool))


# ---------------------------------------------------------------------------
# PyramidROIAlign backward
# ---------------------------------------------------------------------------
BWD_CASES = [(64, (7, 7, 7)), (128, (3, 2, 14)), (256, (14, 14, 14)), (512, (2, 3, 4)),      # gather, CQ 1 2 4 8
             (8, (7, 7, 7)), (6, (3, 3, 3)), (70, (2, 2, 5)), (256, (33, 2, 2)), (8, (65, 1, 1))]   # atomic scatter


@functools.lru_cache(maxsize=2)
def _bwd_grad(C, pool):
    return _ro(np.random.default_rng([C, *pool]).normal(size=(B, N, *pool, C)).astype(np.float32))


@functools.lru_cache(maxsize=2)
def _bwd_ref(C, pool):
    _, _, adj, lev = _pyr_input()
    return roiref.pyramid_grad_ref(_bwd_grad(C, pool), adj, lev, SHAPES)


def _pyr_backward(cuda, C, pool):
    from m3d import ops
    boxes, meta, adj, lev = _pyr_input()
    maps = [T(m, cuda).requires_grad_(True) for m in _maps(C, False)]
    out, badj, blev = ops.pyramid_roi_align(T(boxes, cuda), T(meta, cuda), maps, pool, return_levels=True)
    np.testing.assert_array_equal(blev.cpu().numpy(), lev)
    np.testing.assert_array_equal(badj.cpu().numpy(), adj)
    out.backward(T(_bwd_grad(C, pool), cuda))
    return [m.grad.cpu().numpy() for m in maps]


def _check_bound(got, C, pool, what):
    ref = _bwd_ref(C, pool)
    for li in range(4):
        for b in range(B):          # per image: a gradient landing in the other image is a touched-set error
            r = roiref.check(got[li][b], tuple(x[b] for x in ref[li]), f"{what} C={C} pool={pool} P{li + 2} image {b}")
            assert r < 1.0


@pytest.mark.parametrize("C,pool", BWD_CASES)
def test_pyramid_backward_within_bound(cuda, C, pool):
    """Default mode (fp32 atomics, gather or scatter form)."""
    from m3d import _lib
    assert not _lib.deterministic()
    _check_bound(_pyr_backward(cuda, C, pool), C, pool, "pyramid bwd")


@pytest.mark.parametrize("C,pool", BWD_CASES)
def test_pyramid_backward_deterministic(cuda, C, pool):
    """Deterministic mode: bit-exact with the oracle's per-level sequential
    scatter over the level's ROIs in ascending index order.  A pool above 64
    falls back to the atomic scatter (m3d.ops): only the bound applies."""
    from m3d import _lib
    _lib.set_deterministic(True, scratch_bytes=4096)
    try:
        got = _pyr_backward(cuda, C, pool)
    finally:
        _lib.set_deterministic(False)
    if max(pool) > 64:
        _check_bound(got, C, pool, "pyramid bwd (deterministic mode, atomic fallback)")
        return
    _, _, adj, lev = _pyr_input()
    g = _bwd_grad(C, pool).reshape(B * N, *pool, C)
    for li, (H, W, D) in enumerate(SHAPES):
        sel = np.nonzero(lev.reshape(-1) == li + 2)[0]
        want = R.crop_and_resize_3d_grad_image(g[sel], adj.reshape(-1, 6)[sel], (sel // N).astype(np.int32),
                                               (B, H, W, D, C))
        assert np.abs(want).sum() > 0
        np.testing.assert_array_equal(got[li], want, err_msg=f"P{li + 2}")


# ---------------------------------------------------------------------------
# CropAndResize3D family
# ---------------------------------------------------------------------------
KINDS = ("random", "flipped", "aligned", "tiny")


def _crop_boxes(seed, n_per_kind):
    """The four box kinds of test_gpu_roi_nms._det_case, concatenated; B = 2 on a (9,7,11) image."""
    rng = np.random.default_rng(seed)
    parts = [_det_case(rng, kind, N=n_per_kind) for kind in KINDS]
    shape = parts[0][2]
    assert shape == (2, 9, 7, 11)
    boxes = np.concatenate([p[0] for p in parts])
    bi = np.concatenate([p[1] for p in parts])
    assert set(bi.tolist()) == {0, 1}
    return boxes, bi, shape


@pytest.mark.parametrize("crop", [(5, 4, 3), (1, 4, 1)])
@pytest.mark.parametrize("C", [6, 70, 256, 320, 512])
def test_crop_forward_trilinear_bit_exact(cuda, C, crop):
    from m3d import ops
    boxes, bi, (Bc, H, W, D) = _crop_boxes([C, *crop], 23)
    img = np.random.default_rng([C, 3]).normal(size=(Bc, H, W, D, C)).astype(np.float32)
    want = R.crop_and_resize_3d(img, boxes, bi, crop, "trilinear", -1.5)
    assert (want == -1.5).any() and (want != -1.5).any()
    got = ops.crop_and_resize_3d(T(img, cuda), T(boxes, cuda), T(bi, cuda), crop, "trilinear", -1.5)
    np.testing.assert_array_equal(got.cpu().numpy(), want)


def test_crop_grad_image_c512(cuda):
    """C = 512: gather_bwd_kernel<8,false> in fast mode, within the bound; deterministic = 1 bit-exact."""
    from m3d import ops
    C, crop = 512, (7, 7, 7)
    boxes, bi, (Bc, H, W, D) = _crop_boxes(512, 6)
    g = np.random.default_rng(5120).normal(size=(len(boxes), *crop, C)).astype(np.float32)
    shape = (Bc, H, W, D, C)
    args = (T(g, cuda), T(boxes, cuda), T(bi, cuda), shape)
    fast = ops.crop_and_resize_3d_grad_image(*args).cpu().numpy()
    det = ops.crop_and_resize_3d_grad_image(*args, deterministic=1).cpu().numpy()
    ref = roiref.grad_image_ref(g, boxes, bi, shape)
    for b in range(Bc):
        assert roiref.check(fast[b], tuple(x[b] for x in ref), f"crop grad_image C=512 image {b}") < 1.0
    np.testing.assert_array_equal(det, R.crop_and_resize_3d_grad_image(g, boxes, bi, shape))


@pytest.mark.parametrize("C", [4, 3])
def test_crop_grad_image_det_many_boxes(cuda, C):
    """520 boxes > DET_CAP (512): deterministic = 1 takes the block-strided crop_bwd_det_kernel<4> / <1>."""
    from m3d import ops
    crop = (2, 1, 3)
    boxes, bi, (Bc, H, W, D) = _crop_boxes([520, C], 130)
    assert len(boxes) == 520
    g = np.random.default_rng([520, C, 1]).normal(size=(520, *crop, C)).astype(np.float32)
    shape = (Bc, H, W, D, C)
    args = (T(g, cuda), T(boxes, cuda), T(bi, cuda), shape)
    par = ops.crop_and_resize_3d_grad_image(*args, deterministic=1).cpu().numpy()
    ser = ops.crop_and_resize_3d_grad_image(*args, deterministic=2).cpu().numpy()
    want = R.crop_and_resize_3d_grad_image(g, boxes, bi, shape)
    assert np.abs(want).sum() > 0
    np.testing.assert_array_equal(ser, want)
    np.testing.assert_array_equal(par, want)


# ---------------------------------------------------------------------------
# Host-side rejections: each returns before any launch (valid buffers all the same)
# ---------------------------------------------------------------------------
def _reject_setup(cuda, C=8, pool=(2, 2, 2)):
    boxes, meta, adj, lev = _pyr_input()
    maps = [torch.zeros((B, *s, C), device=cuda) for s in SHAPES]
    return T(boxes, cuda), T(meta, cuda), T(adj, cuda), T(lev, cuda), maps


def test_pyramid_bwd_det_rejects_pool_above_64(cuda):
    from m3d import _lib
    C, pool = 8, (65, 1, 1)
    _, _, adj, lev, gmaps = _reject_setup(cuda, C)
    grad = torch.zeros((B, N, *pool, C), device=cuda)
    bi = torch.zeros(4 * B * N, dtype=torch.int32, device=cuda)
    gptrs, fshape = _fptrs(gmaps)
    with pytest.raises(ValueError, match="crop sizes up to 64"):
        _lib.check(_lib.load().m3d_pyramid_roi_align3d_bwd_det(_lib.ptr(grad), _lib.ptr(adj), _lib.ptr(lev), B, N,
                                                               *pool, gptrs, fshape, C, _lib.ptr(bi), _lib.stream()))


def _fwd_ws_call(cuda, tb, tm, maps, fshape_override=None, meta_stride=META_COLS, C=8, pool=(2, 2, 2)):
    from m3d import _lib
    out = torch.zeros((B, N, *pool, C), device=cuda)
    badj = torch.zeros((B, N, 6), device=cuda)
    blev = torch.zeros((B, N), dtype=torch.int32, device=cuda)
    fptrs, fshape = _fptrs(maps)
    if fshape_override is not None:
        fshape = fshape_override
    L = _lib.load()
    wsb = int(L.m3d_pyramid_roi_align3d_fwd_workspace_bytes(_fptrs(maps)[1], B, N, pool[0], pool[1]))
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    _lib.check(L.m3d_pyramid_roi_align3d_fwd_ws(fptrs, fshape, C, _lib.ptr(tb), _lib.ptr(tm), meta_stride, B, N,
                                                *pool, _lib.ptr(out), _lib.ptr(badj), _lib.ptr(blev), _lib.ptr(ws),
                                                wsb, _lib.stream()))


def test_pyramid_fwd_rejects_meta_stride_7(cuda):
    tb, tm, _, _, maps = _reject_setup(cuda)
    with pytest.raises(ValueError, match="image_meta must have at least 8 columns"):
        _fwd_ws_call(cuda, tb, tm, maps, meta_stride=7)


def test_pyramid_fwd_rejects_zero_map_dimension(cuda):
    from m3d import _lib
    tb, tm, _, _, maps = _reject_setup(cuda)
    dims = [list(s) for s in SHAPES]
    dims[2][1] = 0
    bad = ((_lib.c_i64 * 3) * 4)(*[(_lib.c_i64 * 3)(*d) for d in dims])
    with pytest.raises(ValueError, match="feature map dimensions must be positive"):
        _fwd_ws_call(cuda, tb, tm, maps, fshape_override=bad)
