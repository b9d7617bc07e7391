"""tests/normref.py (the restatement the GPU input-pipeline tests compare
against) pinned four ways: against np.percentile, against
m3d.dataset.normalize_image, on hand-derived cases, and on Philox4x32-10 known
answers."""
import numpy as np
import pytest

import normref as N


VOLUMES = N.VOLUMES


@pytest.mark.parametrize("name", list(VOLUMES))
def test_percentiles_equal_numpy(name):
    x = VOLUMES[name].astype(np.float64)
    want = np.percentile(x, [1, 99])
    p1, p99 = N.stats(x)[:2]
    scale = max(abs(want[0]), abs(want[1]), 1e-300)
    assert abs(p1 - want[0]) <= 1e-12 * scale and abs(p99 - want[1]) <= 1e-12 * scale


@pytest.mark.parametrize("name", list(VOLUMES))
def test_rounded_restatement_is_the_host_normalisation(name):
    """float32(restatement) against m3d.dataset.normalize_image: at most one float32 ulp apart."""
    from m3d.dataset import normalize_image
    raw = VOLUMES[name]
    host = normalize_image(raw)[..., 0]
    ref = N.normalize(raw)[0].astype(np.float32)
    assert host.shape == ref.shape == (raw.shape[1], raw.shape[2], raw.shape[0])
    ulp = np.spacing(np.maximum(np.abs(host), np.abs(ref)))
    assert (np.abs(host.astype(np.float64) - ref.astype(np.float64)) <= ulp).all()
    print(name, "bit-equal share", float((host == ref).mean()))


def test_transpose_flag():
    raw = VOLUMES["odd"]
    a, sa = N.normalize(raw, transpose=True)
    b, sb = N.normalize(np.transpose(raw, (1, 2, 0)), transpose=False)
    assert sa[:2] == sb[:2] and np.allclose(a, b, rtol=0, atol=1e-15)
    assert a.shape == (5, 7, 3)


def test_hand_derived_cases():
    # a constant image: p1 = p99 = mean = the value, std = 0 -> x - mean = 0 everywhere
    out, (p1, p99, mean, std) = N.normalize(np.full((2, 3, 4), 7, np.uint8))
    assert (p1, p99, mean, std) == (7.0, 7.0, 7.0, 0.0) and not out.any() and out.shape == (3, 4, 2)
    # n = 1
    out, st = N.normalize(np.array([[[513]]], np.uint16))
    assert st == (513.0, 513.0, 513.0, 0.0) and out.item() == 0.0
    # n = 101: v = 1 and 99 exactly, g = 0 -> the order statistics themselves
    x = np.arange(101, dtype=np.float32)[::-1].copy() * 2.5
    out, (p1, p99, mean, std) = N.normalize(x.reshape(1, 1, 101))
    assert (p1, p99) == (2.5, 247.5)
    c = np.clip(x.astype(np.float64), 2.5, 247.5)
    assert mean == c.mean() == 125.0 and std == c.std()
    assert out[0, 50, 0] == np.tanh(0.5 * (x[50] - 125.0) / std) and out[0, 0, 0] == np.tanh(0.5 * 122.5 / std)
    # three values: v = 0.02 -> a + (b - a) 0.02; v = 1.98 -> b - (b - a) 0.02
    p1, p99 = N.stats(np.array([10.0, 20.0, 40.0]))[:2]
    assert p1 == 10.0 + 10.0 * 0.02 and p99 == 40.0 - 20.0 * (1.0 - (1.98 - 1))


def test_float32_evaluation_errs_more_than_the_rounding_floor():
    for name in ("u16_full_range", "f32_signed", "u8_six_levels"):
        ref = N.normalize(VOLUMES[name])[0]
        floor = np.abs(ref.astype(np.float32).astype(np.float64) - ref).max()
        f32 = np.abs(N.normalize_f32(VOLUMES[name]).astype(np.float64) - ref).max()
        print(name, "floor", floor, "float32 evaluation", f32)
        assert floor <= 2.0 ** -25 and floor < f32


KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def test_philox_known_answers():
    for ctr, key, want in KAT:
        got = N.philox4x32_10(np.array(ctr, np.uint32), np.array(key, np.uint32))
        assert " ".join(f"{int(v):08x}" for v in got) == want
    # vectorised over counters, and independent of what else is in the batch
    ctrs = np.array([k[0] for k in KAT[::2]], np.uint32)
    one = N.philox4x32_10(ctrs[:1], np.array(KAT[0][1], np.uint32))
    assert " ".join(f"{int(v):08x}" for v in one[0]) == KAT[0][2]


def test_uniform_and_augment_restatement():
    assert N.uniform53(np.uint32(0), np.uint32(0)) == 0.0
    assert N.uniform53(np.uint32(0xFFFFFFFF), np.uint32(0xFFFFFFFF)) == 1.0 - 2.0 ** -53
    rng = np.random.default_rng(3)
    img = rng.normal(size=(7, 5, 9)).astype(np.float32)
    v, g = N.augment(img, 5, 0.0, 0.0)
    assert g is None and np.array_equal(v, img[::-1, :, ::-1])
    v, g = N.augment(img, 0, 0.5, 0.25, seed=(1, 2))
    assert v.min() >= img.min() and v.max() <= img.max() and (v == img.min()).any() and (v == img.max()).any()
    assert abs(g.mean()) < 6 * 0.25 / np.sqrt(g.size) and 0.2 < g.std() < 0.3
    # the value of a voxel depends on (seed, linear index) only
    v2, g2 = N.augment(np.zeros((2, 5, 9), np.float32), 0, 0.0, 0.25, seed=(1, 2))
    assert np.array_equal(g2.ravel(), g.ravel()[:90])
    assert np.array_equal(N.flip_boxes([[1, 2, 3, 4, 6, 8]], (10, 20, 30), 7), [[6, 14, 22, 9, 18, 27]])
