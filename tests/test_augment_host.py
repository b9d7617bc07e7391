"""The host side of m3d.augment (no GPU): jitter_boxes_3d, the flip decisions
and the box flips of apply_minimal_augs_3d (core/data_generators.py:13-167)."""
import numpy as np
import pytest

from m3d.augment import FLIP_X, FLIP_Y, FLIP_Z, draw_flips, flip_boxes, jitter_boxes_3d
from m3d.config import Config

BOXES = np.array([[10, 12, 2, 30, 40, 8], [40, 5, 0, 60, 25, 6]], np.float32)
SHAPE = (64, 64, 12)


def test_jitter_count_zero_returns_the_input():
    rng = np.random.RandomState(0)
    out = jitter_boxes_3d(BOXES, count=0, rng=rng)
    assert out.dtype == np.float32 and np.array_equal(out, BOXES)
    assert jitter_boxes_3d(None, rng=rng) is None
    assert jitter_boxes_3d(np.zeros((0, 6), np.float32), count=3, rng=rng).shape == (0, 6)
    assert rng.rand() == np.random.RandomState(0).rand()                 # nothing was drawn


@pytest.mark.parametrize("max_keep,added", [(None, 3), (2, 2), (1, 1), (5, 3)])
def test_jitter_without_noise_appends_exact_copies(max_keep, added):
    out = jitter_boxes_3d(BOXES, count=3, scale_sigma=0.0, trans=(0, 0, 0), img_shape=SHAPE, iou_thr=0.7,
                          max_keep=max_keep, rng=np.random.RandomState(1))
    assert out.dtype == np.float32 and out.shape == (2 + 2 * added, 6)
    assert np.array_equal(out[:2], BOXES)
    assert np.array_equal(out[2:2 + added], np.tile(BOXES[0], (added, 1)))   # box by box
    assert np.array_equal(out[2 + added:], np.tile(BOXES[1], (added, 1)))


def _iou(b, c):
    lo, hi = np.maximum(b[:3], c[:3]), np.minimum(b[3:], c[3:])
    inter = np.prod(np.maximum(hi - lo, 0).astype(np.float32))
    ab = max(np.prod((b[3:] - b[:3]).astype(np.float32)), 1e-6)
    ac = max(np.prod((c[3:] - c[:3]).astype(np.float32)), 1e-6)
    return np.float32(inter) / np.float32(max(np.float32(ab) + np.float32(ac) - np.float32(inter), 1e-6))


def test_jitter_seeded_case_recomputed_from_the_same_draws():
    """Per candidate three randn (scales of h, w, d), then three randint
    (shifts of y, x, z); the kept ones follow their box in descending IoU."""
    count, sigma, trans, thr, keep = 4, 0.1, (2, 2, 1), 0.4, 2
    out = jitter_boxes_3d(BOXES, count=count, scale_sigma=sigma, trans=trans, img_shape=SHAPE, iou_thr=thr,
                          max_keep=keep, rng=np.random.RandomState(42))
    rng = np.random.RandomState(42)
    want = [BOXES]
    for b in BOXES.astype(np.float64):
        ext = np.maximum(1.0, b[3:] - b[:3])
        ctr = (b[:3] + b[3:]) / 2.0
        cands = []
        for _ in range(count):
            s = np.array([1.0 + rng.randn() * sigma, 1.0 + rng.randn() * sigma, 1.0 + rng.randn() * sigma])
            t = np.array([rng.randint(-trans[0], trans[0] + 1), rng.randint(-trans[1], trans[1] + 1),
                          rng.randint(-trans[2], trans[2] + 1)], np.float64)
            half = np.maximum(1.0, ext * s) / 2.0
            lo = np.clip(ctr + t - half, 0, np.array(SHAPE) - 1)
            hi = np.clip(ctr + t + half, 1, np.array(SHAPE))
            if (hi > lo).all():
                cands.append(np.concatenate([lo, hi]).astype(np.float32))
        ious = np.array([_iou(b.astype(np.float32), c) for c in cands], np.float32)
        ok = [i for i in range(len(cands)) if ious[i] >= np.float32(thr)]
        order = np.argsort(ious[ok])[::-1][:keep] if len(ok) > keep else np.arange(len(ok))
        want.append(np.array([cands[ok[i]] for i in order], np.float32).reshape(-1, 6))
    want = np.concatenate(want)
    assert len(want) > 2 and np.array_equal(out, want)


class ScriptedRng:
    """No scaling; every shift is the largest (or, with low=True, the smallest) allowed."""

    def __init__(self, low=False):
        self.low = low

    def randn(self):
        return 0.0

    def randint(self, lo, hi):
        return lo if self.low else hi - 1


def test_jitter_clips_to_the_image_and_drops_what_is_left_empty():
    """Starts clip to [0, size - 1] and ends to [1, size], so a candidate pushed
    over a border keeps its last voxel there.  Nothing is left (end <= start
    after the clip) only where size - 1 == size in floating point: the drop is
    exercised at an extent of 2^54."""
    corner = np.array([[5, 60, 3, 9, 64, 6]], np.float32)
    out = jitter_boxes_3d(corner, count=2, scale_sigma=0.1, trans=(0, 40, 0), img_shape=SHAPE, iou_thr=0.0,
                          max_keep=None, rng=ScriptedRng())
    # x: centre 62 + 40 -> start clip(100, 0, 63) = 63, end clip(104, 1, 64) = 64
    assert np.array_equal(out, [[5, 60, 3, 9, 64, 6], [5, 63, 3, 9, 64, 6], [5, 63, 3, 9, 64, 6]])
    edge = np.array([[5, 0, 3, 9, 1, 6]], np.float32)
    out = jitter_boxes_3d(edge, count=1, scale_sigma=0.1, trans=(0, 40, 0), img_shape=SHAPE, iou_thr=0.0,
                          rng=ScriptedRng(low=True))
    # x: centre 0.5 - 40 -> start clip(-40, 0, 63) = 0, end clip(-39, 1, 64) = 1
    assert np.array_equal(out, [[5, 0, 3, 9, 1, 6], [5, 0, 3, 9, 1, 6]])
    # with iou_thr > 0 the shifted copies no longer overlap their box: filtered, the input comes back
    out = jitter_boxes_3d(corner, count=2, scale_sigma=0.1, trans=(0, 40, 0), img_shape=SHAPE, iou_thr=0.5,
                          rng=ScriptedRng())
    assert np.array_equal(out, corner)
    big = float(2 ** 54)                                                 # big - 1 == big in float64
    far = np.array([[big, 2, 2, big, 6, 6], [3, 2, 2, 9, 6, 6]], np.float32)
    out = jitter_boxes_3d(far, count=2, scale_sigma=0.0, trans=(0, 0, 0), img_shape=(big, 64, 12), iou_thr=0.0,
                          rng=ScriptedRng())
    # box 0: start clip(2^54 - 0.5 = 2^54, 0, 2^54) = end clip(2^54, 1, 2^54): dropped, both candidates;
    # box 1 keeps its two copies
    assert np.array_equal(out, np.concatenate([far, far[1:], far[1:]]))


def _cfg(**kw):
    return Config(IMAGE_SIZE=64, IMAGE_DEPTH=12, **kw)


class CountingRng(np.random.RandomState):
    calls = 0

    def rand(self, *a):
        self.calls += 1
        return super().rand(*a)


@pytest.mark.parametrize("axes,draws", [((True, True, False), 2), ((False, False, False), 0),
                                        ((True, True, True), 3), ((False, True, False), 1)])
def test_flip_decisions_draw_only_for_enabled_axes(axes, draws):
    cfg = _cfg(AUG_FLIP_Y=axes[0], AUG_FLIP_X=axes[1], AUG_FLIP_Z=axes[2], AUG_PROB=0.5)
    rng = CountingRng(7)
    mask = draw_flips(cfg, rng)
    assert rng.calls == draws
    ref = np.random.RandomState(7)
    want = 0
    for on, bit in zip(axes, (FLIP_Y, FLIP_X, FLIP_Z)):                  # Y, then X, then Z
        if on and ref.rand() < 0.5:
            want |= bit
    assert mask == want
    assert draw_flips(_cfg(AUG_FLIP_Z=True, AUG_PROB=1.0), np.random.RandomState(0)) == 7
    assert draw_flips(_cfg(AUG_FLIP_Z=True, AUG_PROB=0.0), np.random.RandomState(0)) == 0


def test_box_flips_against_hand_values():
    b = np.array([[10, 12, 2, 30, 40, 8]], np.float32)                   # in 64 x 48 x 12, exclusive ends
    shape = (64, 48, 12)
    assert np.array_equal(flip_boxes(b, shape, 0), b)
    assert np.array_equal(flip_boxes(b, shape, FLIP_Y), [[34, 12, 2, 54, 40, 8]])
    assert np.array_equal(flip_boxes(b, shape, FLIP_X), [[10, 8, 2, 30, 36, 8]])
    assert np.array_equal(flip_boxes(b, shape, FLIP_Z), [[10, 12, 4, 30, 40, 10]])
    assert np.array_equal(flip_boxes(b, shape, 7), [[34, 8, 4, 54, 36, 10]])
    assert np.array_equal(flip_boxes(flip_boxes(b, shape, 7), shape, 7), b)
    assert flip_boxes(np.zeros((0, 6)), shape, 7).shape == (0, 6) and flip_boxes(b, shape, 7).dtype == np.float32
    assert b[0, 0] == 10                                                 # the input is not modified


def test_generator_refuses_more_than_one_image_per_item():
    from m3d.generator import RPNGenerator
    with pytest.raises(ValueError, match="IMAGES_PER_GPU"):
        RPNGenerator(_cfg(IMAGES_PER_GPU=2), None, np.zeros((4, 6), np.float32), "cpu")
