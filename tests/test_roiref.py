"""tests/roiref.py (the float64 reference of the trilinear image gradient and
its derived bound) against the oracle's float32 sequential scatter -- no GPU.

The oracle adds its float32 terms one after the other, which is one of the
summation orders the bound covers: it must lie within (cnt + 4) * 2^-24 *
abs64 of sum64 and touch exactly the voxels with cnt > 0."""
import numpy as np
import pytest

import roiref
from oracle import ops_ref as R

H, W, D = 9, 7, 11


def _boxes(kind, rng):
    if kind == "random":         # partly outside the image on every side
        lo = rng.uniform(-0.2, 0.9, (12, 3))
        b = np.concatenate([lo, lo + rng.uniform(0.02, 0.6, (12, 3))], 1)
    elif kind == "flipped":      # y2 < y1 etc.: negative sample spacing
        lo = rng.uniform(-0.1, 0.6, (9, 3))
        b = np.concatenate([lo, lo + rng.uniform(0.1, 0.5, (9, 3))], 1)
        b[::2] = b[::2][:, [3, 4, 5, 0, 1, 2]]
        b[1, [0, 3]] = b[1, [3, 0]]          # one axis only
    elif kind == "aligned":      # integer coordinates: floor == ceil, two corners on one voxel
        q = rng.integers(0, 4, (10, 6)).astype(np.float32)
        b = q / np.array([H - 1, W - 1, D - 1] * 2, np.float32)
        b[:, 3:] = np.maximum(b[:, 3:], b[:, :3] + np.float32(2.0 / (H - 1)))
    elif kind == "whole":        # the whole image, a zero-extent box and a box past every edge
        b = np.array([[0, 0, 0, 1, 1, 1], [0.5, 0.5, 0.5, 0.5, 0.5, 0.5], [-0.5, -0.5, -0.5, 1.5, 1.5, 1.5],
                      [0, 0, 0, 1, 1, 1]], np.float64)
    else:
        raise AssertionError(kind)
    return b.astype(np.float32)


@pytest.mark.parametrize("kind,C,crop", [
    ("random", 5, (5, 4, 3)), ("random", 3, (14, 14, 14)), ("random", 4, (3, 2, 14)),
    ("random", 2, (1, 4, 1)), ("random", 2, (1, 1, 1)), ("random", 2, (4, 1, 5)),
    ("flipped", 3, (7, 7, 7)), ("flipped", 2, (1, 5, 1)),
    ("aligned", 4, (7, 5, 9)), ("aligned", 2, (3, 3, 3)),
    ("whole", 3, (7, 7, 7)), ("whole", 2, (9, 7, 11)), ("whole", 2, (2, 3, 4)), ("whole", 2, (1, 1, 1))])
def test_roiref_vs_oracle(kind, C, crop):
    rng = np.random.default_rng([ord(ch) for ch in kind] + [C, *crop])
    boxes = _boxes(kind, rng)
    N = len(boxes)
    bi = rng.integers(0, 2, N).astype(np.int32)
    bi[:2] = [0, 1]
    g = rng.normal(size=(N, *crop, C)).astype(np.float32)
    shape = (2, H, W, D, C)
    want = R.crop_and_resize_3d_grad_image(g, boxes, bi, shape)
    ref = roiref.grad_image_ref(g, boxes, bi, shape)
    ratio = roiref.check(want, ref, f"oracle {kind} C={C} crop={crop}")
    assert ratio < 1.0
    # every corner hit of every in-image sample is counted once
    sum64, abs64, cnt = ref
    assert cnt.sum() % 8 == 0
    assert (abs64 >= np.abs(sum64)).all()


def test_roiref_known_answer():
    """One box on a 3x3x3 image, 2x2x2 samples at (0.5, 1.5) per axis: every
    sample spreads g/8 over its 8 corners, the centre voxel gets all 8."""
    g = np.arange(1, 9, dtype=np.float32).reshape(1, 2, 2, 2, 1)
    boxes = np.array([[0.25, 0.25, 0.25, 0.75, 0.75, 0.75]], np.float32)
    s, a, cnt = roiref.grad_image_ref(g, boxes, [0], (1, 3, 3, 3, 1))
    assert cnt.sum() == 64 and cnt[0, 1, 1, 1] == 8 and cnt[0, 0, 0, 0] == 1 and cnt[0, 0, 1, 0] == 2
    assert s[0, 1, 1, 1, 0] == 36 / 8 and s[0, 0, 0, 0, 0] == 1 / 8 and s[0, 2, 2, 2, 0] == 8 / 8
    assert s[0, 0, 0, 1, 0] == (1 + 2) / 8
    np.testing.assert_array_equal(s, a)
    assert s.sum() == 36.0
    # integer-aligned single sample: floor == ceil on every axis, the second corner weighs 0
    s, a, cnt = roiref.grad_image_ref(-g[:, :1, :1, :1], np.array([[1, 1, 1, 0, 0, 0]], np.float32), [0],
                                      (1, 3, 3, 3, 1))
    assert cnt[0, 1, 1, 1] == 8 and cnt.sum() == 8
    assert s[0, 1, 1, 1, 0] == -1.0 and a[0, 1, 1, 1, 0] == 1.0
    assert np.array_equal(roiref.bound(a, cnt)[0, 1, 1, 1], [12 * 2.0 ** -24])


def test_roiref_pyramid_wrapper():
    """The pyramid wrapper is the per-level, per-image scatter: equal to the
    plain reference over the level's ROIs with box_ind = image."""
    rng = np.random.default_rng(5)
    B, N, C, pool = 2, 9, 3, (3, 2, 4)
    shapes = [(8, 8, 4), (4, 4, 4), (2, 2, 4), (1, 1, 4)]
    lo = rng.uniform(0, 0.5, (B, N, 3))
    boxes = np.concatenate([lo, lo + rng.choice([0.05, 0.2, 0.4, 0.5], (B, N, 1))], 2).astype(np.float32)
    prep = [R.roi_prepare(boxes[b], (1024, 1024, 256)) for b in range(B)]
    adj = np.stack([p[0] for p in prep])
    lev = np.stack([p[1] for p in prep])
    assert len(np.unique(lev)) == 4
    g = rng.normal(size=(B, N, *pool, C)).astype(np.float32)
    got = roiref.pyramid_grad_ref(g, adj, lev, shapes)
    for li, (Hl, Wl, Dl) in enumerate(shapes):
        sel = np.nonzero(lev.reshape(-1) == li + 2)[0]
        want = roiref.grad_image_ref(g.reshape(B * N, *pool, C)[sel], adj.reshape(-1, 6)[sel], sel // N,
                                     (B, Hl, Wl, Dl, C))
        for x, y in zip(got[li], want):
            np.testing.assert_array_equal(x, y)


def test_roiref_rejects_bad_input():
    g = np.zeros((1, 2, 2, 2, 1), np.float32)
    with pytest.raises(ValueError, match="box_index"):
        roiref.grad_image_ref(g, np.zeros((1, 6), np.float32), [1], (1, 3, 3, 3, 1))
    with pytest.raises(ValueError, match="non-finite"):
        roiref.grad_image_ref(g, np.full((1, 6), np.nan, np.float32), [0], (1, 3, 3, 3, 1))
