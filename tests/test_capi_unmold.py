"""The unmolding / mask-IoU entry points of include/m3d.h (m3d_unmold_prepare,
m3d_unmold_overlaps, m3d_unmold_finalize, m3d_unmold_paste, m3d_mask_areas)
through the C-ABI without a GPU: exported, declared, and every rejection path
returns M3D_EINVAL before any launch."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m3d_unmold_prepare", "m3d_unmold_overlaps", "m3d_unmold_finalize", "m3d_unmold_paste", "m3d_mask_areas")
FAKE = 0x1000           # a non-NULL pointer that must never be dereferenced


def _lib():
    import m3d._lib as lib
    return lib, lib.load()


def test_symbols_exported_declared_and_documented():
    lib, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "m3d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in lib.EXPORTED, name
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    comment = hdr[:hdr.index("int m3d_unmold_prepare(")].rsplit("/* Detection unmolding", 1)[1]
    assert "core/models.py:7198-7419" in comment and "core/utils.py:312-334" in comment
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in integ, name
    # the status codes of the header, the package and the restatement agree
    from m3d import evaluate as E
    for i, n in enumerate(E.STATUS_NAMES):
        assert int(re.search(r"#define\s+M3D_UNMOLD_" + n + r"\s+(\d+)", hdr).group(1)) == i
    assert E.MAX_GRID == 32768


def _prepare(L, det=FAKE, mask=FAKE, n=4, m=28, C=2, H=64, W=64, D=64, small=FAKE, box=FAKE, status=FAKE,
             stats=FAKE):
    return L.m3d_unmold_prepare(det, mask, n, m, C, H, W, D, small, box, status, stats, None)


def _overlaps(L, small=FAKE, box=FAKE, status=FAKE, stats=FAKE, n=4, m=28, H=64, W=64, D=64, gt=FAKE, G=3,
              area=FAKE, inter=FAKE):
    return L.m3d_unmold_overlaps(small, box, status, stats, n, m, H, W, D, gt, G, area, inter, None)


def _paste(L, small=FAKE, box=FAKE, status=FAKE, stats=FAKE, n=4, m=28, H=64, W=64, D=64, dense=FAKE, union=FAKE):
    return L.m3d_unmold_paste(small, box, status, stats, n, m, H, W, D, dense, union, None)


def test_null_pointers_are_rejected():
    lib, L = _lib()
    for k in ("det", "mask", "small", "box", "status", "stats"):
        assert _prepare(L, **{k: None}) == -1 and b"NULL" in L.m3d_last_error(), k
    for k in ("small", "box", "status", "stats", "area"):
        assert _overlaps(L, **{k: None}) == -1 and b"NULL" in L.m3d_last_error(), k
    for k in ("gt", "inter"):
        assert _overlaps(L, **{k: None}) == -1 and b"must not be NULL when G > 0" in L.m3d_last_error(), k
    for k in ("small", "box", "status", "stats"):
        assert _paste(L, **{k: None}) == -1 and b"NULL" in L.m3d_last_error(), k
    assert L.m3d_unmold_finalize(None, FAKE, 4, 3, FAKE, FAKE, FAKE, FAKE, None) == -1
    assert L.m3d_unmold_finalize(FAKE, None, 4, 3, FAKE, FAKE, FAKE, FAKE, None) == -1
    assert L.m3d_unmold_finalize(FAKE, FAKE, 4, 3, None, FAKE, FAKE, FAKE, None) == -1
    assert L.m3d_unmold_finalize(FAKE, FAKE, 4, 3, FAKE, None, FAKE, FAKE, None) == -1
    assert L.m3d_unmold_finalize(FAKE, FAKE, 4, 3, FAKE, FAKE, None, FAKE, None) == -1
    assert b"iou needs area_gt" in L.m3d_last_error()
    assert L.m3d_mask_areas(None, 8, 8, 8, 3, FAKE, None) == -1 and b"NULL" in L.m3d_last_error()
    assert L.m3d_mask_areas(FAKE, 8, 8, 8, 3, None, None) == -1 and b"NULL" in L.m3d_last_error()


def test_grid_size_limit():
    """m^3 <= 32768: m = 32 passes this check (and reaches the NULL check), m = 33 does not."""
    lib, L = _lib()
    for call in (_prepare, _overlaps, _paste):
        assert call(L, m=33) == -1 and b"32768" in L.m3d_last_error()
        assert call(L, m=1 << 40) == -1 and b"32768" in L.m3d_last_error()
        assert call(L, m=32, small=None) == -1 and b"NULL" in L.m3d_last_error()


def test_shapes_must_be_positive():
    lib, L = _lib()
    for call in (_prepare, _overlaps, _paste):
        for k in ("m", "H", "W", "D"):
            for v in (0, -2):
                assert call(L, **{k: v}) == -1 and b"must be positive" in L.m3d_last_error(), (k, v)
        assert call(L, n=-1) == -1 and b"max_inst" in L.m3d_last_error()
        assert call(L, H=1 << 20, W=1 << 20, D=4) == -1 and b"31 bits" in L.m3d_last_error()
    for v in (0, -1):
        assert _prepare(L, C=v) == -1 and b"C must be positive" in L.m3d_last_error()
    for k in range(3):
        dims = [8, 8, 8]
        dims[k] = 0
        assert L.m3d_mask_areas(FAKE, *dims, 3, FAKE, None) == -1 and b"must be positive" in L.m3d_last_error()
    assert L.m3d_unmold_finalize(FAKE, FAKE, -1, 3, FAKE, FAKE, FAKE, FAKE, None) == -1


def test_negative_g_is_rejected():
    lib, L = _lib()
    assert _overlaps(L, G=-1) == -1 and b"G must be" in L.m3d_last_error()
    assert L.m3d_unmold_finalize(FAKE, FAKE, 4, -1, FAKE, FAKE, FAKE, FAKE, None) == -1
    assert b"G must be" in L.m3d_last_error()
    assert L.m3d_mask_areas(FAKE, 8, 8, 8, -1, FAKE, None) == -1 and b"G must be" in L.m3d_last_error()


def test_empty_calls_enqueue_nothing():
    """max_inst = 0 (and G = 0 for the areas) is a no-op that touches no pointer."""
    lib, L = _lib()
    assert _prepare(L, n=0) == 0 and _overlaps(L, n=0) == 0 and _paste(L, n=0) == 0
    assert L.m3d_unmold_finalize(FAKE, FAKE, 0, 3, FAKE, FAKE, FAKE, FAKE, None) == 0
    assert L.m3d_mask_areas(FAKE, 8, 8, 8, 0, FAKE, None) == 0
    assert _paste(L, dense=None, union=None) == 0


def test_python_ops_refuse_cpu_tensors():
    import torch
    from m3d import evaluate as E
    from m3d.heads import MaskRCNN
    det, mask = torch.zeros(4, 8), torch.zeros(4, 8, 8, 8, 2)
    with pytest.raises(ValueError, match="GPU"):
        E.unmold_detections(det, mask, (16, 16, 16))
    with pytest.raises(ValueError, match="GPU"):
        E.mask_areas(torch.zeros(4, 4, 4, 2, dtype=torch.uint8))
    u = E.Unmolded(det, (16, 16, 16), 8, None, None, torch.zeros(4, dtype=torch.int32), None, None, None, None)
    with pytest.raises(ValueError, match="GPU"):
        E.mask_overlaps(u, torch.zeros(16, 16, 16, 2, dtype=torch.uint8))
    with pytest.raises(ValueError, match="GPU"):
        E.evaluate_detections(det, mask, (16, 16, 16), [1], torch.zeros(16, 16, 16, 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="GPU"):
        MaskRCNN.evaluate(None, torch.zeros(1, 16, 16, 16, 1), torch.zeros(1, 18), [1], None,
                          torch.zeros(16, 16, 16, 1, dtype=torch.uint8))
