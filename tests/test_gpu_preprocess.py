"""The input pipeline on the GPU (m3d_normalize_image, m3d_augment_image,
m3d_flip_masks_u8, m3d_flip_boxes; m3d.preprocess, m3d.augment) against the
numpy float64 restatement tests/normref.py (pinned by tests/test_normref.py).

Bars.  Statistics: p1 / p99 within 1e-10 max(|p1|, |p99|), mean within 1e-10
max(|mean|, std), std within 1e-10 std (the bar of the unmold statistics; the
integer inputs' sums are exact).  Image: the GPU's maximum error against the
unrounded restatement is no larger than that of the same formula evaluated in
float32 numpy (float32 clip bounds, mean, std, tanh) on the same input -- a
kernel that evaluates in fp64 and rounds once sits at the float32 rounding
floor, one that takes tanhf or float32 statistics does not.  Flips and the
brightness leg: bit for bit.  Gaussian leg: 2 float32 ulp of max(|image|,
|noise|) (one for the noise's rounding after a device log / cos that may
differ from libm in the last fp64 bits, one for the sum's rounding).

Shapes (Z,Y,X): the ones of tests/test_normref.py -- (1,1,1); (1,1,101), g = 0
for both percentiles; (1,3,3); (5,7,67) uint16 spanning 0 and 65535; (33,9,70)
uint8 with six levels (every order statistic inside a run of ties); (12,40,40)
float32 with negatives and +-0; (3,5,7); (64,96,128), 786,432 voxels: above the
2048 x 256 threads of the flat kernels' grid cap, so their grid-stride loops
run (the 16-byte-load loops of the histogram and sum kernels run from 4096
bytes on); and (40,260,130), 2600 tiles of 64 x 64 against the transposing
kernel's cap of 2048 workgroups."""
import functools

import numpy as np
import pytest
import torch

import normref as N

VOLUMES = N.VOLUMES

pytestmark = pytest.mark.gpu

TILE_CAP = (40, 260, 130)


@functools.lru_cache(maxsize=None)
def _volume(name):
    if name == "tile_cap":
        return np.random.default_rng(5).integers(0, 3000, TILE_CAP).astype(np.uint16)
    return VOLUMES[name]


@functools.lru_cache(maxsize=None)
def _ref(name, transpose=True):
    raw = _volume(name)
    out, st = N.normalize(raw, transpose)
    f32 = N.normalize_f32(raw, transpose)
    return out, st, float(np.abs(f32.astype(np.float64) - out).max())


def _np(t):
    return t.cpu().numpy()


def _check_stats(got, want, name):
    p1, p99, mean, std = want
    g = [float(v) for v in got]
    tol_p = 1e-10 * max(abs(p1), abs(p99))
    print(name, "stats", g[:4], "want", want)
    assert abs(g[0] - p1) <= tol_p and abs(g[1] - p99) <= tol_p
    assert abs(g[2] - mean) <= 1e-10 * max(abs(mean), std)
    assert abs(g[3] - std) <= 1e-10 * std
    assert g[4] == 0.0 and g[5] == 0.0


def _check_image(got, ref64, bar, name):
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    floor = float(np.abs(ref64.astype(np.float32).astype(np.float64) - ref64).max())
    print(name, "gpu max error", err, "float32 evaluation", bar, "rounding floor", floor)
    assert got.dtype == np.float32 and err <= bar
    return err


NAMES = list(VOLUMES) + ["tile_cap"]


@pytest.mark.parametrize("name", NAMES)
def test_normalize_file_order(cuda, name):
    from m3d.dataset import normalize_image as host_normalize
    from m3d.preprocess import normalize_image
    raw = _volume(name)
    ref, st, bar = _ref(name)
    out, stats = normalize_image(torch.from_numpy(raw).to(cuda), return_stats=True)
    Z, Y, X = raw.shape
    assert tuple(out.shape) == (Y, X, Z, 1) and out.dtype == torch.float32 and stats.dtype == torch.float64
    _check_stats(_np(stats), st, name)
    got = _np(out)[..., 0]
    _check_image(got, ref, bar, name)
    print(name, "bit-equal to the host normalize_image:", float((got == host_normalize(raw)[..., 0]).mean()))


@pytest.mark.parametrize("name", NAMES)
def test_normalize_in_place_order_and_twice(cuda, name):
    """transpose = 0 on the raw dtype, and repeat = 2: the second pass is the
    float32 path on the first pass's own float32 output."""
    from m3d.preprocess import normalize_image
    raw = _volume(name)
    ref, st, bar = _ref(name, False)
    dev = torch.from_numpy(raw).to(cuda)
    out, stats = normalize_image(dev, transpose=False, return_stats=True)
    assert tuple(out.shape) == raw.shape + (1,)
    _check_stats(_np(stats), st, name)
    _check_image(_np(out)[..., 0], ref, bar, name)
    first = _np(normalize_image(dev))[..., 0]
    twice, stats2 = normalize_image(dev, repeat=2, return_stats=True)
    ref2, st2 = N.normalize(first, transpose=False)
    bar2 = float(np.abs(N.normalize_f32(first, transpose=False).astype(np.float64) - ref2).max())
    assert tuple(twice.shape) == first.shape + (1,)
    _check_stats(_np(stats2), st2, name + " (second pass)")
    _check_image(_np(twice)[..., 0], ref2, bar2, name + " (second pass)")


def test_other_dtypes_are_cast_on_the_device(cuda):
    from m3d.preprocess import normalize_image
    raw = _volume("odd").astype(np.int32) - 300
    ref, st = N.normalize(raw)
    out, stats = normalize_image(torch.from_numpy(raw).to(cuda), return_stats=True)
    _check_stats(_np(stats), st, "int32")
    assert np.abs(_np(out)[..., 0].astype(np.float64) - ref).max() <= 2.0 ** -24
    with pytest.raises(ValueError, match="3-D"):
        normalize_image(torch.zeros(4, 4, device=cuda))


def test_non_finite_inputs_are_counted(cuda):
    from m3d.preprocess import normalize_image
    raw = _volume("f32_signed").copy()
    raw[1, 2, 3], raw[4, 5, 6], raw[7, 8, 9] = np.nan, np.inf, -np.inf
    _, stats = normalize_image(torch.from_numpy(raw).to(cuda), return_stats=True)
    assert float(stats[4]) == 3.0


# ---- augmentation -------------------------------------------------------------

ODD = (7, 5, 9)


@functools.lru_cache(maxsize=None)
def _image(shape=ODD, seed=1):
    return np.random.default_rng(seed).normal(size=shape).astype(np.float32)


@pytest.mark.parametrize("mask", range(1, 8))
def test_image_flips_equal_numpy(cuda, mask):
    from m3d.augment import augment_image
    img = _image()
    got = augment_image(torch.from_numpy(img).to(cuda), mask)
    assert np.array_equal(_np(got), N.flip(img, mask))
    got = augment_image(torch.from_numpy(img[..., None]).to(cuda), mask)          # [H,W,D,1]
    assert tuple(got.shape) == ODD + (1,) and np.array_equal(_np(got)[..., 0], N.flip(img, mask))


@pytest.mark.parametrize("G", [1, 3, 16])
@pytest.mark.parametrize("mask", range(1, 8))
def test_mask_flips_equal_numpy(cuda, mask, G):
    """G = 1 and 3: byte and (without a z flip) wider line moves; G = 16 with
    aligned buffers: 16-byte vectors also under a z flip."""
    from m3d.augment import flip_masks
    m = np.random.default_rng(G).integers(0, 256, ODD + (G,)).astype(np.uint8)
    got = flip_masks(torch.from_numpy(m).to(cuda), mask)
    assert got.dtype == torch.uint8 and np.array_equal(_np(got), N.flip(m, mask))
    b = m > 127
    got = flip_masks(torch.from_numpy(b).to(cuda), mask)
    assert got.dtype == torch.bool and np.array_equal(_np(got), N.flip(b, mask))


def test_mask_flips_every_vector_width(cuda):
    """Unaligned views of one buffer: the widest vector that the pointers and
    the group (z flip) or line length allow, from 16 bytes down to 1."""
    import m3d._lib as lib
    L, p, s = lib.load(), lib.ptr, lib.stream()
    H, W, D, G = 3, 5, 4, 16
    m = np.random.default_rng(0).integers(0, 256, (H, W, D, G)).astype(np.uint8)
    n = m.size
    for off in (0, 8, 4, 2, 1):
        src = torch.zeros(n + 16, dtype=torch.uint8, device=cuda)
        dst = torch.full((n + 32,), 0x5A, dtype=torch.uint8, device=cuda)
        src[off:off + n] = torch.from_numpy(m.ravel()).to(cuda)
        for mask in (4, 3, 7):
            lib.check(L.m3d_flip_masks_u8(p(src[off:off + n]), H, W, D, G, mask, p(dst[16 + off:16 + off + n]), s))
            got = _np(dst)
            assert np.array_equal(got[16 + off:16 + off + n].reshape(m.shape), N.flip(m, mask)), (off, mask)
            assert (got[:16 + off] == 0x5A).all() and (got[16 + off + n:] == 0x5A).all()


def test_box_flips_equal_the_host_form(cuda):
    from m3d.augment import flip_boxes
    rng = np.random.default_rng(2)
    lo = rng.uniform(0, 40, (70, 3))
    boxes = np.concatenate([lo, lo + rng.uniform(1, 20, (70, 3))], 1).astype(np.float32)
    for mask in range(8):
        got = flip_boxes(torch.from_numpy(boxes).to(cuda), (64, 48, 60), mask)
        assert np.array_equal(_np(got), flip_boxes(boxes, (64, 48, 60), mask))
        assert np.array_equal(_np(got), N.flip_boxes(boxes, (64, 48, 60), mask))
    assert tuple(flip_boxes(torch.zeros((0, 6), device=cuda), (4, 4, 4), 7).shape) == (0, 6)


@pytest.mark.parametrize("mask,bd", [(0, 0.03), (7, 0.5), (2, 4.0)])
def test_brightness_leg_is_bit_equal(cuda, mask, bd):
    """bd = 0.5 and 4.0: the noise spans half and four times the image's range,
    so the clip binds at both ends."""
    from m3d.augment import augment_image
    img = _image((9, 11, 13), seed=4)
    want, _ = N.augment(img, mask, bd, 0.0, seed=(123, 0xFEDCBA98))
    got = _np(augment_image(torch.from_numpy(img).to(cuda), mask, bd, 0.0, seed=(123, 0xFEDCBA98)))
    assert np.array_equal(got, want)
    if bd >= 0.5:
        assert (want == img.min()).sum() > 5 and (want == img.max()).sum() > 5
    other = _np(augment_image(torch.from_numpy(img).to(cuda), mask, bd, 0.0, seed=(124, 0xFEDCBA98)))
    assert not np.array_equal(other, want)


@pytest.mark.parametrize("bd", [0.0, 0.1])
def test_gaussian_leg(cuda, bd):
    from m3d.augment import augment_image
    img = _image((16, 24, 20), seed=6)
    std = 0.05
    base, gauss = N.augment(img, 5, bd, std, seed=(7, 9))
    got = _np(augment_image(torch.from_numpy(img).to(cuda), 5, bd, std, seed=(7, 9)))
    want = base.astype(np.float64) + gauss
    ulp = np.spacing(np.maximum(np.abs(base), np.abs(gauss).astype(np.float32)))
    assert (np.abs(got.astype(np.float64) - want) <= 2.0 * ulp).all()
    exact = got == (base + gauss.astype(np.float32))
    print("voxels equal to the restatement rounded the same way:", float(exact.mean()))
    noise = got.astype(np.float64) - base
    assert abs(noise.mean()) <= 6 * std / np.sqrt(noise.size)
    assert 0.9 * std < noise.std() < 1.1 * std


def test_values_depend_on_seed_and_index_only(cuda):
    """Two extents that share a prefix of linear indices, and 600,000 voxels
    (more than 2048 x 256 threads: the grid-stride loop) against 5,000."""
    from m3d.augment import augment_image
    zeros = lambda *s: torch.zeros(s, device=cuda)                                # noqa: E731
    a = _np(augment_image(zeros(7, 5, 9), 0, 0.0, 0.3, seed=(1, 2))).ravel()
    b = _np(augment_image(zeros(2, 5, 9), 0, 0.0, 0.3, seed=(1, 2))).ravel()
    assert np.array_equal(a[:90], b) and a.std() > 0.2
    big = _np(augment_image(zeros(100, 100, 60), 0, 0.0, 0.3, seed=(1, 2))).ravel()
    small = _np(augment_image(zeros(10, 10, 50), 0, 0.0, 0.3, seed=(1, 2))).ravel()
    assert np.array_equal(big[:5000], small) and np.array_equal(big[:315], a)
    _, g = N.augment(np.zeros((100, 100, 60), np.float32), 0, 0.0, 0.3, seed=(1, 2))
    assert (np.abs(big - g.ravel()) <= 2 * np.spacing(np.abs(g.ravel()).astype(np.float32))).all()


@pytest.mark.parametrize("mask", [0, 3, 7])
def test_legs_off_leave_the_flipped_image(cuda, mask):
    from m3d.augment import augment_image
    img = _image()
    got = augment_image(torch.from_numpy(img).to(cuda), mask, 0.0, 0.0, seed=(5, 6))
    assert np.array_equal(_np(got), N.flip(img, mask))


def test_apply_minimal_augs(cuda):
    """AUG_PROB = 1 with all axes on: image, boxes and masks flip together; the
    noise key is drawn from rng after the flip decisions, only when a leg is on."""
    from m3d.augment import apply_minimal_augs_3d
    from m3d.config import Config
    img = _image((8, 6, 10))
    boxes = np.array([[1, 1, 2, 5, 4, 9]], np.float32)
    masks = np.random.default_rng(0).integers(0, 2, (8, 6, 10, 2)).astype(np.uint8)
    cfg = Config(IMAGE_SIZE=64, AUG_PROB=1.0, AUG_FLIP_Z=True, AUG_BRIGHTNESS_DELTA=0.0)
    rng = np.random.RandomState(3)
    dev_img = torch.from_numpy(img[..., None]).to(cuda)
    out, b, m = apply_minimal_augs_3d(dev_img, boxes, torch.from_numpy(masks).to(cuda), cfg, rng)
    assert tuple(out.shape) == (8, 6, 10, 1) and np.array_equal(_np(out)[..., 0], N.flip(img, 7))
    assert np.array_equal(b, N.flip_boxes(boxes, (8, 6, 10), 7)) and np.array_equal(_np(m), N.flip(masks, 7))
    ref = np.random.RandomState(3)
    ref.rand(3)
    assert rng.rand() == ref.rand()                                               # three draws, no key
    cfg = Config(IMAGE_SIZE=64, AUG_PROB=0.0, AUG_BRIGHTNESS_DELTA=0.2, AUG_GAUSS_NOISE_STD=0.0)
    rng, ref = np.random.RandomState(4), np.random.RandomState(4)
    out, b, m = apply_minimal_augs_3d(dev_img, boxes, None, cfg, rng)
    ref.rand(2)                                                                   # Y and X (Z is off)
    seed = (int(ref.randint(0, 2 ** 32, dtype=np.uint64)), int(ref.randint(0, 2 ** 32, dtype=np.uint64)))
    assert np.array_equal(_np(out)[..., 0], N.augment(img, 0, 0.2, 0.0, seed)[0])
    assert np.array_equal(b, boxes) and m is None and rng.rand() == ref.rand()


# ---- hygiene ------------------------------------------------------------------

PAD = 7


def _guarded(cuda, count, dtype, fill=0x5A):
    buf = torch.empty(count + 2 * PAD, dtype=dtype, device=cuda)
    buf.view(torch.uint8).fill_(fill)
    return buf, buf[PAD:PAD + count]


def _intact(buf, count):
    b = _np(buf.view(torch.uint8))
    w = buf.element_size()
    return (b[:PAD * w] == 0x5A).all() and (b[(PAD + count) * w:] == 0x5A).all()


@pytest.mark.parametrize("name,transpose", [("u16_full_range", 1), ("u8_six_levels", 1), ("f32_signed", 1),
                                            ("odd", 0), ("f32_signed", 0)])
def test_normalize_guard_bands(cuda, name, transpose):
    """raw, out, stats and the workspace as interior slices of sentinel-filled
    buffers (raw 7 elements in: not 16-byte aligned, so the scalar head and tail
    of the 16-byte-load loops run); every byte around them survives."""
    import m3d._lib as lib
    from m3d.preprocess import _CODES
    L, p, s = lib.load(), lib.ptr, lib.stream()
    raw = _volume(name)
    Z, Y, X = raw.shape
    n = raw.size
    tdt = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16,
           np.dtype(np.float32): torch.float32}[raw.dtype]
    raw_buf, raw_in = _guarded(cuda, n, tdt)
    raw_in.copy_(torch.from_numpy(raw.ravel()).to(cuda))
    out_buf, out = _guarded(cuda, n, torch.float32)
    st_buf, stats = _guarded(cuda, 6, torch.float64)
    wsb = int(L.m3d_normalize_image_workspace_bytes(Z, Y, X, _CODES[tdt]))
    ws_buf = torch.full((wsb + 32,), 0x5A, dtype=torch.uint8, device=cuda)
    lib.check(L.m3d_normalize_image(p(raw_in), _CODES[tdt], Z, Y, X, transpose, p(out), p(stats),
                                    p(ws_buf[16:16 + wsb]), wsb, s))
    torch.cuda.synchronize()
    ref, st, bar = _ref(name, bool(transpose))
    _check_stats(_np(stats), st, name)
    _check_image(_np(out).reshape(ref.shape), ref, bar, name)
    assert _intact(raw_buf, n) and _intact(out_buf, n) and _intact(st_buf, 6)
    assert np.array_equal(_np(raw_in), raw.ravel())
    w = _np(ws_buf)
    assert (w[:16] == 0x5A).all() and (w[16 + wsb:] == 0x5A).all()


def test_augment_guard_bands(cuda):
    import m3d._lib as lib
    L, p, s = lib.load(), lib.ptr, lib.stream()
    img = _image((9, 11, 13), seed=4)
    n = img.size
    in_buf, inp = _guarded(cuda, n, torch.float32)
    inp.copy_(torch.from_numpy(img.ravel()).to(cuda))
    out_buf, out = _guarded(cuda, n, torch.float32)
    wsb = int(L.m3d_augment_image_workspace_bytes(9, 11, 13))
    ws_buf = torch.full((wsb + 32,), 0x5A, dtype=torch.uint8, device=cuda)
    lib.check(L.m3d_augment_image(p(inp), 9, 11, 13, 7, 0.5, 0.0, 123, 0xFEDCBA98, p(out), p(ws_buf[16:16 + wsb]),
                                  wsb, s))
    torch.cuda.synchronize()
    assert np.array_equal(_np(out).reshape(img.shape), N.augment(img, 7, 0.5, 0.0, seed=(123, 0xFEDCBA98))[0])
    assert _intact(in_buf, n) and _intact(out_buf, n) and np.array_equal(_np(inp), img.ravel())
    w = _np(ws_buf)
    assert (w[:16] == 0x5A).all() and (w[16 + wsb:] == 0x5A).all()
    bx_buf, bx = _guarded(cuda, 30, torch.float32)
    src = torch.arange(30, dtype=torch.float32, device=cuda)
    lib.check(L.m3d_flip_boxes(p(src), 5, 64, 64, 64, 7, p(bx), s))
    assert _intact(bx_buf, 30) and np.array_equal(_np(bx).reshape(5, 6), N.flip_boxes(_np(src), (64, 64, 64), 7))


def _chain(cuda, raw, img, masks):
    from m3d.augment import augment_image, flip_masks
    from m3d.preprocess import normalize_image
    a, stats = normalize_image(raw, repeat=2, return_stats=True)
    b = augment_image(img, 5, 0.2, 0.05, seed=(3, 4))
    return a, stats, b, flip_masks(masks, 6)


def _chain_inputs(cuda):
    masks = np.random.default_rng(1).integers(0, 2, ODD + (3,)).astype(np.uint8)
    return (torch.from_numpy(_volume("u16_full_range")).to(cuda), torch.from_numpy(_image((9, 11, 13))).to(cuda),
            torch.from_numpy(masks).to(cuda))


def test_two_runs_are_bit_identical(cuda):
    args = _chain_inputs(cuda)
    f32 = torch.from_numpy(_volume("grid_cap").astype(np.float32)).to(cuda)
    from m3d.preprocess import normalize_image
    r1, r2 = _chain(cuda, *args), _chain(cuda, *args)
    g1, g2 = (normalize_image(f32, return_stats=True) for _ in range(2))
    torch.cuda.synchronize()
    for x, y in zip(r1 + g1, r2 + g2):
        assert torch.equal(x, y)
    assert r1[0].abs().max() > 0 and float(g1[1][3]) > 0


def test_graph_capture_and_replay(cuda):
    args = _chain_inputs(cuda)
    eager = _chain(cuda, *args)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _chain(cuda, *args)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _chain(cuda, *args)
    for t in out:
        t.view(torch.uint8).fill_(0xFF)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(out, eager):
        assert torch.equal(x, y)
