"""m3d_rpn_eval_proposals (include/m3d.h) through the C-ABI without a GPU:
exported, declared, documented, named in INTEGRATION.md, and every rejection
returns M3D_EINVAL with its message before any launch."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "m3d_rpn_eval_proposals"
FAKE = 0x1000           # a non-NULL pointer that must never be dereferenced


def _lib():
    import m3d._lib as lib
    return lib, lib.load()


def _call(L, rois=FAKE, R=100, gt=FAKE, G=3, H=64, W=64, D=16, topk=50, thr=0.5, grid=FAKE, T=3, assoc=FAKE,
          matched=FAKE, first_hit=FAKE, counts=FAKE, iou=None):
    return L.m3d_rpn_eval_proposals(rois, R, gt, G, H, W, D, topk, thr, grid, T, assoc, matched, first_hit, counts,
                                    iou, None)


def test_symbol_exported_declared_and_documented():
    lib, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "m3d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert hasattr(L, NAME) and NAME in lib.EXPORTED
    assert re.search(r"\bint " + NAME + r"\s*\(", code)
    comment = hdr[:hdr.index("int " + NAME + "(")].rsplit("/* RPN evaluation", 1)[1]
    assert "*/" not in comment.rstrip()[:-2]                 # the comment directly above the declaration
    for ref in ("core/utils.py:1289-1392", "78-144", "1562-1574"):
        assert ref in comment, ref
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "csrc/rpn_eval.hip" in open(os.path.join(ROOT, "3d-mask-r-cnn_amd", "Makefile")).read()
    assert L.m3d_abi_version() == 3                          # an addition only


def test_null_pointers_are_rejected():
    lib, L = _lib()
    for k in ("gt", "assoc", "matched", "counts"):
        assert _call(L, **{k: None}) == -1 and b"NULL" in L.m3d_last_error(), k
    assert _call(L, rois=None) == -1 and b"rois must not be NULL when R > 0" in L.m3d_last_error()
    for k in ("grid", "first_hit"):
        assert _call(L, **{k: None}) == -1 and b"must not be NULL when T > 0" in L.m3d_last_error(), k
    # with T = 0 neither is needed: the call gets past that check and stops at another NULL
    assert _call(L, T=0, grid=None, first_hit=None, counts=None) == -1
    assert b"rpn_eval_proposals: NULL pointer" in L.m3d_last_error()


def test_shape_must_be_positive():
    lib, L = _lib()
    for k in ("H", "W", "D"):
        for v in (0, -2):
            assert _call(L, **{k: v}) == -1 and b"must be positive" in L.m3d_last_error(), (k, v)


def test_negative_counts_are_rejected():
    lib, L = _lib()
    assert _call(L, R=-1) == -1 and b"R must not be negative" in L.m3d_last_error()
    assert _call(L, topk=-1) == -1 and b"topk must not be negative" in L.m3d_last_error()
    assert _call(L, T=-1) == -1 and b"T must be in [0, 8]" in L.m3d_last_error()
    # R = 0 and topk = 0 are fine: the call reaches the NULL check
    assert _call(L, R=0, topk=0, rois=None, counts=None) == -1 and b"NULL pointer" in L.m3d_last_error()


def test_gt_count_limits_from_both_sides():
    lib, L = _lib()
    for v in (0, -1, 513, 1 << 40):
        assert _call(L, G=v) == -1 and b"G must be in [1, 512]" in L.m3d_last_error(), v
    for v in (1, 512):                                       # passes to the next check
        assert _call(L, G=v, counts=None) == -1 and b"NULL pointer" in L.m3d_last_error(), v


def test_grid_length_limits_from_both_sides():
    lib, L = _lib()
    for v in (9, 1 << 40):
        assert _call(L, T=v) == -1 and b"T must be in [0, 8]" in L.m3d_last_error(), v
    for v in (0, 8):
        assert _call(L, T=v, counts=None) == -1 and b"NULL pointer" in L.m3d_last_error(), v


def test_iou_matrix_must_fit_31_bits():
    lib, L = _lib()
    assert _call(L, R=1 << 22, G=512) == -1 and b"31 bits" in L.m3d_last_error()         # 2^31 exactly
    assert _call(L, R=1 << 40, G=1) == -1 and b"31 bits" in L.m3d_last_error()
    assert _call(L, R=(1 << 22) - 1, G=512, counts=None) == -1 and b"NULL pointer" in L.m3d_last_error()


def test_score_proposals_refuses_cpu_tensors_and_bad_arguments():
    import torch
    from m3d import rpn_eval
    rois, gt = torch.zeros(10, 6), torch.zeros(2, 6)
    with pytest.raises(ValueError, match="GPU"):
        rpn_eval.score_proposals(rois, gt, (64, 64, 16), 5, 0.5, [0.3, 0.5])
    with pytest.raises(ValueError, match="GPU"):
        rpn_eval.score_proposals(rois, gt, (64, 64, 16), 5, 0.5, [0.3], out=torch.zeros(64, dtype=torch.int32))
    assert rpn_eval.record_len(50, 3) == 502


def test_rpn_has_the_evaluate_method():
    from m3d.model import RPN
    assert callable(getattr(RPN, "evaluate", None))
    for word in ('generator.last["boxes"]', "Telemetry", "IMAGES_PER_GPU"):
        assert word in RPN.evaluate.__doc__, word
