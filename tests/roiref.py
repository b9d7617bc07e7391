"""float64 reference of CropAndResize3DGradImage (trilinear) with a derived
error bound -- test infrastructure, plain numpy, no GPU.

Which voxels a sample touches and with which weights is decided in float32,
op for op as ``oracle/oracle.c`` and the kernels do:
``scale = ((b2-b1)*(S-1))/(n-1)``, ``in = b1*(S-1) + i*scale`` (or the double
midpoint for a single-sample axis), a sample outside ``[0, S-1]`` on any axis
contributes nothing, corners are floor / ceil and the corner weight is
``(wy*wx)*wz``.  The reference therefore touches exactly the voxels the
kernels touch.  Only the products ``g*w`` (exact in float64: 24 + 24
significand bits) and their sums are carried in float64, scattered with
``np.add.at``.

``grad_image_ref`` returns, per voxel and channel,

* ``sum64`` -- the gradient,
* ``abs64`` -- the same scatter applied to ``|g*w|``,

and per voxel ``cnt``, the number of contributions (corner hits) it received.

The bound.  A float32 implementation rounds each of the n = cnt products once
(relative error <= u = 2^-24) and adds them in some order with n - 1 rounded
additions.  To first order in u every term then carries at most n roundings,
so for any summation order -- sequential replay, per-wave partial sums plus
one atomic, atomics in arrival order --

    |fl(sum) - sum64| <= n * u * abs64 + O(u^2)

``bound`` returns ``(cnt + 4) * 2^-24 * abs64``; the + 4 absorbs the second
order terms (n^2 u^2 / 2 <= 4 u needs n <= 11585, far above any count here)
and the float64 error of the reference itself.  The bound is derived, not
measured: the tests that use it must not tune it.
"""
import numpy as np

F = np.float32
U = 2.0 ** -24


def _axis(b1, b2, S, n):
    """float32 sample coordinates of one axis: (kept sample indices, [2,k]
    corner voxels (floor, ceil), [2,k] float32 corner weights (1-l, l))."""
    b1, b2 = F(b1), F(b2)
    if n > 1:
        sc = ((b2 - b1) * F(S - 1)) / F(n - 1)
        x = b1 * F(S - 1) + np.arange(n, dtype=F) * sc
    else:
        x = np.array([0.5 * float(b1 + b2) * float(S - 1)], np.float64).astype(F)
    assert x.dtype == F
    keep = ~((x < 0) | (x > F(S - 1)))          # the oracle's test: NaN would be kept
    idx = np.nonzero(keep)[0]
    x = x[idx]
    if not np.isfinite(x).all():
        raise ValueError("roiref: non-finite sample coordinate (NaN box)")
    lo, hi = np.floor(x), np.ceil(x)
    lerp = x - lo
    assert lerp.dtype == F
    return idx, np.stack([lo, hi]).astype(np.int64), np.stack([F(1.0) - lerp, lerp])


def grad_image_ref(grads, boxes, box_ind, image_size):
    """grads [N,ch,cw,cd,C], boxes [N,6], box_ind [N], image_size (B,H,W,D,C)
    -> (sum64 [B,H,W,D,C], abs64 [B,H,W,D,C], cnt [B,H,W,D])."""
    grads = np.asarray(grads, F)
    boxes = np.asarray(boxes, F).reshape(-1, 6)
    box_ind = np.asarray(box_ind).reshape(-1)
    B, H, W, D, C = (int(v) for v in image_size)
    N, ch, cw, cd, Cg = grads.shape
    assert Cg == C and boxes.shape[0] == N and box_ind.shape[0] == N
    if N and (box_ind.min() < 0 or box_ind.max() >= B):
        raise ValueError("box_index has values outside [0, batch_size)")
    V = B * H * W * D
    sum64 = np.zeros((V, C), np.float64)
    abs64 = np.zeros((V, C), np.float64)
    cnt = np.zeros(V, np.int64)
    for n in range(N):
        ys, iy, wy = _axis(boxes[n, 0], boxes[n, 3], H, ch)
        xs, ix, wx = _axis(boxes[n, 1], boxes[n, 4], W, cw)
        zs, iz, wz = _axis(boxes[n, 2], boxes[n, 5], D, cd)
        if ys.size == 0 or xs.size == 0 or zs.size == 0:
            continue
        # axes (corner a, b, c, sample y, x, z)
        w = (wy[:, None, None, :, None, None] * wx[None, :, None, None, :, None]) * \
            wz[None, None, :, None, None, :]
        assert w.dtype == F
        vox = ((int(box_ind[n]) * H + iy[:, None, None, :, None, None]) * W +
               ix[None, :, None, None, :, None]) * D + iz[None, None, :, None, None, :]
        g = grads[n][np.ix_(ys, xs, zs)].astype(np.float64)               # [ky,kx,kz,C]
        term = w.astype(np.float64)[..., None] * g[None, None, None]      # exact products
        vox = np.ascontiguousarray(np.broadcast_to(vox, w.shape)).reshape(-1)
        flat = (vox[:, None] * C + np.arange(C)).reshape(-1)
        term = term.reshape(-1)
        np.add.at(sum64.reshape(-1), flat, term)
        np.add.at(abs64.reshape(-1), flat, np.abs(term))
        np.add.at(cnt, vox, 1)
    shape = (B, H, W, D)
    return sum64.reshape(shape + (C,)), abs64.reshape(shape + (C,)), cnt.reshape(shape)


def pyramid_grad_ref(grads, boxes_adj, levels, map_shapes):
    """Gradient of PyramidROIAlign w.r.t. P2..P5: grads [B,N,ph,pw,pd,C],
    boxes_adj [B,N,6] and levels [B,N] as ``oracle.ops_ref.roi_prepare`` gives
    them, map_shapes four (H,W,D).  The scatter runs per level, per image;
    returns four (sum64, abs64, cnt) with shapes [B,H,W,D,C] / [B,H,W,D]."""
    grads = np.asarray(grads, F)
    boxes_adj = np.asarray(boxes_adj, F)
    levels = np.asarray(levels)
    B, N = levels.shape
    C = grads.shape[-1]
    out = []
    for li, (H, W, D) in enumerate(map_shapes):
        s = np.zeros((B, H, W, D, C), np.float64)
        a = np.zeros((B, H, W, D, C), np.float64)
        c = np.zeros((B, H, W, D), np.int64)
        for b in range(B):
            sel = np.nonzero(levels[b] == li + 2)[0]
            if sel.size == 0:
                continue
            sb, ab, cb = grad_image_ref(grads[b, sel], boxes_adj[b, sel], np.zeros(sel.size, np.int32),
                                        (1, H, W, D, C))
            s[b], a[b], c[b] = sb[0], ab[0], cb[0]
        out.append((s, a, c))
    return out


def bound(abs64, cnt):
    """Elementwise bound on |float32 result - sum64| for any summation order."""
    return (cnt[..., None] + 4) * U * abs64


def check(got, ref, what=""):
    """Assert ``got`` (float32, any summation order) against ref = (sum64,
    abs64, cnt): within the bound everywhere, and non-zero exactly where
    cnt > 0.  Returns max(err / bound) over the touched voxels."""
    sum64, abs64, cnt = ref
    got = np.asarray(got)
    assert got.shape == sum64.shape, (what, got.shape, sum64.shape)
    assert np.isfinite(got).all(), what
    touched = np.broadcast_to((cnt > 0)[..., None], got.shape)
    assert touched.any(), f"{what}: no voxel touched"
    assert np.array_equal(got != 0, touched), f"{what}: touched voxel set differs"
    err = np.abs(got.astype(np.float64) - sum64)
    bnd = bound(abs64, cnt)
    assert (bnd[touched] > 0).all(), what
    ratio = float((err[touched] / bnd[touched]).max())
    print(f"{what}: max err / bound = {ratio:.3f} (max cnt {int(cnt.max())})")
    assert (err <= bnd).all(), f"{what}: max err / bound = {ratio:.3f}"
    return ratio
