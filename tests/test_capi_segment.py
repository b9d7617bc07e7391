"""The label-volume entry points of include/m3d.h (m3d_unmold_labels,
m3d_label_pixelwise, m3d_labels_stack) through the C-ABI without a GPU:
exported, declared, documented, and every rejection path returns M3D_EINVAL
before any launch."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m3d_unmold_labels", "m3d_label_pixelwise", "m3d_labels_stack")
FAKE = 0x1000           # a non-NULL pointer that must never be dereferenced


def _lib():
    import m3d._lib as lib
    return lib, lib.load()


def _labels(L, small=FAKE, box=FAKE, status=FAKE, stats=FAKE, keep=FAKE, n=4, m=28, H=64, W=64, D=64,
            label_of=FAKE, labels=FAKE):
    return L.m3d_unmold_labels(small, box, status, stats, keep, n, m, H, W, D, label_of, labels, None)


def _pixelwise(L, labels=FAKE, gt=FAKE, H=64, W=64, D=64, G=3, counts=FAKE):
    return L.m3d_label_pixelwise(labels, gt, H, W, D, G, counts, None)


def _stack(L, labels=FAKE, H=64, W=64, D=64, bps=1, stack=FAKE):
    return L.m3d_labels_stack(labels, H, W, D, bps, stack, None)


def test_symbols_exported_declared_and_documented():
    lib, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "m3d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in lib.EXPORTED, name
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    comment = hdr[:hdr.index("int m3d_unmold_labels(")].rsplit("/* The segmentation volume", 1)[1]
    assert "core/models.py:7023-7087" in comment and "6153-6164" in comment
    assert hdr.index("int m3d_mask_areas(") < hdr.index("int m3d_unmold_labels(")       # next to the unmold block
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in integ, name


def test_null_pointers_are_rejected():
    lib, L = _lib()
    for k in ("small", "box", "status", "stats", "label_of", "labels"):
        assert _labels(L, **{k: None}) == -1 and b"NULL" in L.m3d_last_error(), k
    for k in ("labels", "counts"):
        assert _pixelwise(L, **{k: None}) == -1 and b"NULL" in L.m3d_last_error(), k
    assert _pixelwise(L, gt=None) == -1 and b"must not be NULL when G > 0" in L.m3d_last_error()
    for k in ("labels", "stack"):
        assert _stack(L, **{k: None}) == -1 and b"NULL" in L.m3d_last_error(), k


def test_shapes_must_be_positive_and_fit_31_bits():
    lib, L = _lib()
    for call in (_labels, _pixelwise, _stack):
        for k in ("H", "W", "D"):
            for v in (0, -2):
                assert call(L, **{k: v}) == -1 and b"must be positive" in L.m3d_last_error(), (call, k, v)
        assert call(L, H=1 << 20, W=1 << 20, D=4) == -1 and b"31 bits" in L.m3d_last_error()
        assert call(L, H=1 << 11, W=1 << 10, D=1 << 10) == -1 and b"31 bits" in L.m3d_last_error()   # 2^31 exactly
    for v in (0, -2):
        assert _labels(L, m=v) == -1 and b"must be positive" in L.m3d_last_error()


def test_grid_size_limit():
    """m^3 <= 32768: m = 32 passes this check (and reaches the NULL check), m = 33 does not."""
    lib, L = _lib()
    assert _labels(L, m=33) == -1 and b"32768" in L.m3d_last_error()
    assert _labels(L, m=1 << 40) == -1 and b"32768" in L.m3d_last_error()
    assert _labels(L, m=32, small=None) == -1 and b"NULL" in L.m3d_last_error()


def test_max_inst_limits():
    """A label fits 16 bits: 65535 rows pass this check (and reach the NULL check), 65536 do not."""
    lib, L = _lib()
    assert _labels(L, n=-1) == -1 and b"max_inst" in L.m3d_last_error()
    assert _labels(L, n=65536) == -1 and b"65535" in L.m3d_last_error()
    assert _labels(L, n=1 << 40) == -1 and b"max_inst" in L.m3d_last_error()
    assert _labels(L, n=65535, labels=None) == -1 and b"NULL" in L.m3d_last_error()


def test_negative_g_is_rejected():
    lib, L = _lib()
    assert _pixelwise(L, G=-1) == -1 and b"G must be" in L.m3d_last_error()
    assert _pixelwise(L, G=1 << 31) == -1 and b"G must be" in L.m3d_last_error()
    # G = 0 needs no gt_masks: the call gets past that check (and stops at the next one)
    assert _pixelwise(L, G=0, gt=None, counts=None) == -1 and b"NULL" in L.m3d_last_error()


def test_sample_width_must_be_one_or_two_bytes():
    lib, L = _lib()
    for v in (0, 3, 4, -1, 8):
        assert _stack(L, bps=v) == -1 and b"bytes_per_sample" in L.m3d_last_error(), v
    for v in (1, 2):
        assert _stack(L, bps=v, stack=None) == -1 and b"NULL" in L.m3d_last_error()


def test_python_ops_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from m3d import evaluate as E
    det, mask = torch.zeros(4, 8), torch.zeros(4, 8, 8, 8, 2)
    with pytest.raises(ValueError, match="GPU"):
        E.unmold_detections(det, mask, (16, 16, 16), labels=True, keep=torch.ones(4, dtype=torch.bool))
    with pytest.raises(ValueError, match="GPU"):
        E.pixelwise_counts(torch.zeros(4, 4, 4, dtype=torch.int32), torch.zeros(4, 4, 4, 2, dtype=torch.uint8))
    with pytest.raises(ValueError, match="GPU"):
        E.evaluate_detections(det, mask, (16, 16, 16), [1], torch.zeros(16, 16, 16, 1, dtype=torch.uint8),
                              labels=True)
    u = E.Unmolded(det, (16, 16, 16), 8, None, None, torch.zeros(4, dtype=torch.int32), None, None, None, None)
    assert u.labels is None and u.label_of is None
    with pytest.raises(ValueError, match="labels=True"):
        u.label_stack()
