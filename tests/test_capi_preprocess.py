"""The input-pipeline entry points of include/m3d.h (m3d_normalize_image,
m3d_augment_image, m3d_flip_masks_u8, m3d_flip_boxes and the two workspace
functions) through the C-ABI without a GPU: exported, declared, documented,
and every rejection path returns M3D_EINVAL before any launch."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m3d_normalize_image", "m3d_augment_image", "m3d_flip_masks_u8", "m3d_flip_boxes")
SIZES = ("m3d_normalize_image_workspace_bytes", "m3d_augment_image_workspace_bytes")
FAKE = 0x1000           # a non-NULL, 16-byte aligned pointer that must never be dereferenced
OTHER = 0x2000
BIG = 1 << 30           # a workspace size that always suffices


def _lib():
    import m3d._lib as lib
    return lib, lib.load()


def _norm(L, raw=FAKE, dtype=1, Z=8, Y=8, X=8, transpose=1, out=OTHER, stats=FAKE, ws=FAKE, wsb=BIG):
    return L.m3d_normalize_image(raw, dtype, Z, Y, X, transpose, out, stats, ws, wsb, None)


def _aug(L, inp=FAKE, H=8, W=8, D=8, flip=7, bd=0.1, ns=0.1, out=OTHER, ws=FAKE, wsb=BIG):
    return L.m3d_augment_image(inp, H, W, D, flip, bd, ns, 1, 2, out, ws, wsb, None)


def _masks(L, inp=FAKE, H=8, W=8, D=8, G=3, flip=7, out=OTHER):
    return L.m3d_flip_masks_u8(inp, H, W, D, G, flip, out, None)


def _boxes(L, inp=FAKE, N=4, H=8, W=8, D=8, flip=7, out=OTHER):
    return L.m3d_flip_boxes(inp, N, H, W, D, flip, out, None)


def test_symbols_exported_declared_and_documented():
    lib, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "m3d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert hasattr(L, name) and name in lib.EXPORTED, name
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    for name in SIZES:
        assert hasattr(L, name) and name in lib.EXPORTED, name
        assert re.search(r"\bsize_t " + name + r"\s*\(", code), name
        assert getattr(L, name).restype is lib.c_sz
    comment = hdr[:hdr.index("size_t m3d_normalize_image_workspace_bytes(")].rsplit("/* The input pipeline", 1)[1]
    for cite in ("core/data_generators.py:1603-1630", "1227-1242", "13-86", "974-986"):
        assert cite in comment, cite
    for word in ("non-finite", "unspecified", "Philox4x32-10", "unseeded"):
        assert word in comment, word
    assert hdr.index("int m3d_labels_stack(") < hdr.index("int m3d_normalize_image(")
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW + SIZES:
        assert name in integ, name
    mk = open(os.path.join(ROOT, "3d-mask-r-cnn_amd", "Makefile")).read()
    assert "csrc/preprocess.hip" in mk


def test_workspace_sizes():
    lib, L = _lib()
    for dtype in (0, 1, 2):
        n = L.m3d_normalize_image_workspace_bytes(128, 128, 128, dtype)
        assert 0 < n < (1 << 20)                                         # state, histograms, partials, one level table
    assert L.m3d_normalize_image_workspace_bytes(128, 128, 128, 3) == 0
    assert L.m3d_normalize_image_workspace_bytes(0, 128, 128, 1) == 0
    assert 0 < L.m3d_augment_image_workspace_bytes(128, 128, 128) < (1 << 16)
    assert L.m3d_augment_image_workspace_bytes(128, -1, 128) == 0


def test_null_pointers_are_rejected():
    lib, L = _lib()
    for k in ("raw", "out", "stats"):
        assert _norm(L, **{k: None}) == -1 and b"NULL" in L.m3d_last_error(), k
    for k in ("inp", "out"):
        for call in (_aug, _masks, _boxes):
            assert call(L, **{k: None}) == -1 and b"NULL" in L.m3d_last_error(), (call, k)
    # no boxes: nothing to read or write, pointers unused
    assert _boxes(L, N=0, inp=None, out=None) == 0


def test_extents_must_be_positive_and_fit_31_bits():
    lib, L = _lib()
    for call, names in ((_norm, ("Z", "Y", "X")), (_aug, ("H", "W", "D")), (_masks, ("H", "W", "D")),
                        (_boxes, ("H", "W", "D"))):
        for k in names:
            for v in (0, -2):
                assert call(L, **{k: v}) == -1 and b"must be positive" in L.m3d_last_error(), (call, k, v)
    for call, names in ((_norm, ("Z", "Y", "X")), (_aug, ("H", "W", "D")), (_masks, ("H", "W", "D"))):
        a, b, c = names
        assert call(L, **{a: 1 << 20, b: 1 << 20, c: 4}) == -1 and b"31 bits" in L.m3d_last_error()
        assert call(L, **{a: 1 << 11, b: 1 << 10, c: 1 << 10}) == -1 and b"31 bits" in L.m3d_last_error()  # 2^31
        # 2^31 - 2^21 voxels pass this check (and stop at the next one)
        assert call(L, **{a: (1 << 10) - 1, b: 1 << 10, c: 1 << 11, "out": None}) == -1
        assert b"NULL" in L.m3d_last_error()
    for v in (0, -1, 1 << 31):
        assert _masks(L, G=v) == -1 and b"G must be" in L.m3d_last_error(), v
    for v in (-1, 1 << 40):
        assert _boxes(L, N=v) == -1 and b"N must be" in L.m3d_last_error(), v


def test_unknown_dtype_transpose_and_flip_mask():
    lib, L = _lib()
    for v in (-1, 3, 7):
        assert _norm(L, dtype=v) == -1 and b"dtype" in L.m3d_last_error(), v
    for v in (-1, 2):
        assert _norm(L, transpose=v) == -1 and b"transpose" in L.m3d_last_error(), v
    for call in (_aug, _masks, _boxes):
        for v in (-1, 8):
            assert call(L, flip=v) == -1 and b"flip_mask" in L.m3d_last_error(), (call, v)


def test_short_or_missing_workspace():
    lib, L = _lib()
    for dtype in (0, 1, 2):
        need = L.m3d_normalize_image_workspace_bytes(8, 8, 8, dtype)
        assert _norm(L, dtype=dtype, wsb=need - 1) == -1 and b"workspace too small" in L.m3d_last_error()
        assert _norm(L, dtype=dtype, ws=None) == -1 and b"workspace too small" in L.m3d_last_error()
        assert _norm(L, dtype=dtype, ws=FAKE + 4) == -1 and b"misaligned workspace" in L.m3d_last_error()
    need = L.m3d_augment_image_workspace_bytes(8, 8, 8)
    assert _aug(L, wsb=need - 1) == -1 and b"workspace too small" in L.m3d_last_error()
    assert _aug(L, ws=None, wsb=0) == -1 and b"workspace too small" in L.m3d_last_error()


def test_misaligned_pointers():
    lib, L = _lib()
    assert _norm(L, dtype=1, raw=FAKE + 1) == -1 and b"misaligned pointer" in L.m3d_last_error()
    assert _norm(L, dtype=2, raw=FAKE + 2) == -1 and b"misaligned pointer" in L.m3d_last_error()
    assert _norm(L, out=OTHER + 2) == -1 and b"misaligned pointer" in L.m3d_last_error()
    assert _norm(L, stats=FAKE + 4) == -1 and b"misaligned pointer" in L.m3d_last_error()


def test_in_place_is_rejected():
    lib, L = _lib()
    assert _norm(L, raw=FAKE, out=FAKE) == -1 and b"same buffer" in L.m3d_last_error()
    for call in (_aug, _masks, _boxes):
        assert call(L, inp=FAKE, out=FAKE) == -1 and b"same buffer" in L.m3d_last_error(), call


def test_python_wrappers_refuse_cpu_tensors():
    import numpy as np
    import torch
    from m3d import augment as A
    from m3d.config import Config
    from m3d.preprocess import normalize_image
    with pytest.raises(ValueError, match="GPU"):
        normalize_image(torch.zeros(4, 4, 4, dtype=torch.uint8))
    with pytest.raises(TypeError):
        normalize_image(np.zeros((4, 4, 4), np.uint8))
    with pytest.raises(ValueError, match="GPU"):
        A.augment_image(torch.zeros(4, 4, 4), 1)
    with pytest.raises(ValueError, match="GPU"):
        A.flip_masks(torch.zeros(4, 4, 4, 2, dtype=torch.uint8), 1)
    with pytest.raises(ValueError, match="GPU"):
        A.flip_boxes(torch.zeros(2, 6), (4, 4, 4), 1)
    with pytest.raises(ValueError, match="GPU"):
        A.apply_minimal_augs_3d(torch.zeros(4, 4, 4, 1), np.zeros((1, 6), np.float32), None,
                                Config(IMAGE_SIZE=64), np.random.RandomState(0))


def test_load_image_default_is_the_host_path(tmp_path):
    """ToyDataset.load_image without a device: numpy, equal to normalize_image of the stack."""
    import numpy as np
    from m3d.dataset import ToyDataset, normalize_image
    from m3d.tiff import imwrite
    raw = np.random.default_rng(0).integers(0, 4000, (4, 6, 5)).astype(np.uint16)
    path = os.path.join(str(tmp_path), "v.tiff")
    imwrite(path, raw)
    ds = ToyDataset()
    ds.add_image("dataset", image_id=0, path=path)
    got = ds.load_image(0)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (6, 5, 4, 1)
    assert np.array_equal(got, normalize_image(raw))
