"""Pins tests/headloss_ref.py (the torch restatement of the reference's three
head-loss graphs, the checker of the fused kernels) with hand-derived values,
and the argument checks of m3d_head_loss_fwd / _bwd (no GPU: every rejection
happens before any launch)."""
import math

import pytest
import torch

import headloss_ref as HL

F64 = torch.float64


def _cls(ids, logits, active=None):
    ids = torch.tensor(ids, dtype=torch.int32)
    logits = torch.tensor(logits, dtype=F64)
    B, T, C = logits.shape
    active = torch.ones(B, C, dtype=F64) if active is None else torch.tensor(active, dtype=F64)
    return float(HL.class_loss(ids, logits, active))


def test_class_background_row_at_exactly_one_half_has_no_penalty():
    # p = (0.5, 0.5): (1 - 0.5)^3 ln 2; max fg prob is not > 0.5; the weight cancels
    assert _cls([[0]], [[[0.0, 0.0]]]) == pytest.approx(0.125 * math.log(2), abs=1e-7)
    assert 0.125 * math.log(2) == pytest.approx(0.0866434, abs=1e-7)


def test_class_confident_false_positive_is_doubled():
    # p = (0.25, 0.75), target bg: 2 * 0.75^3 * ln 4
    assert _cls([[0]], [[[0.0, math.log(3)]]]) == pytest.approx(2 * 0.75 ** 3 * math.log(4), abs=1e-7)
    assert 2 * 0.75 ** 3 * math.log(4) == pytest.approx(1.169686, abs=1e-6)


def test_class_two_rows_share_the_weight_sum():
    got = _cls([[0, 0]], [[[0.0, 0.0], [0.0, math.log(3)]]])
    assert got == pytest.approx(0.628165, abs=1e-6)


def test_class_inactive_target_contributes_nothing():
    # C = 3, class 2 inactive: the row with target 2 leaves numerator and denominator
    logits = [[[0.3, -1.0, 2.0], [1.0, 0.5, -0.5]]]
    both = _cls([[2, 1]], logits, [[1, 1, 0]])
    alone = _cls([[1]], [[[1.0, 0.5, -0.5]]], [[1, 1, 0]])
    assert both == pytest.approx(alone, rel=1e-12)
    assert both != pytest.approx(_cls([[2, 1]], logits, [[1, 1, 1]]), rel=1e-3)
    # background is always allowed, whatever column 0 says
    assert _cls([[0]], [[[0.0, 0.0]]], [[0, 1]]) == pytest.approx(0.125 * math.log(2), abs=1e-7)


def test_class_active_row_is_r_mod_B_not_the_image():
    # B = 2, T = 2: flat rows 0..3 belong to images 0,0,1,1 but read active rows 0,1,0,1.
    # Only image 1 has class 1 inactive; all four targets are class 1.
    logits = torch.tensor([[[0.0, 1.0], [2.0, -1.0]], [[-1.0, 0.5], [0.3, 0.1]]], dtype=F64)
    ids = torch.ones(2, 2, dtype=torch.int32)
    active = torch.tensor([[1.0, 1.0], [1.0, 0.0]], dtype=F64)
    got = float(HL.class_loss(ids, logits, active))

    def rows(keep):
        flat = logits.reshape(4, 2)[keep][None]
        return float(HL.class_loss(torch.ones(1, len(keep), dtype=torch.int32), flat, torch.ones(1, 2, dtype=F64)))

    assert got == pytest.approx(rows([0, 2]), rel=1e-12)          # r mod B == 0
    assert got != pytest.approx(rows([0, 1]), rel=1e-3)           # r // T == 0 would keep these


def _box(target, pred=0.0, ids=((1,),)):
    ids = torch.tensor(ids, dtype=torch.int32)
    B, T = ids.shape
    tb = torch.full((B, T, 6), float(target), dtype=F64)
    pb = torch.full((B, T, 2, 6), float(pred), dtype=F64)
    return float(HL.bbox_loss(tb, ids, pb))


def test_bbox_values():
    assert _box(0.5) == pytest.approx(0.125, abs=1e-12)           # quadratic side
    assert _box(2.0) == pytest.approx(1.5, abs=1e-12)             # linear side
    assert _box(2.0, ids=((0,),)) == 0.0                          # no positives


def test_mask_values():
    ids = torch.tensor([[1]], dtype=torch.int32)
    tm = torch.tensor([1.0, 1.0, 0.0, 0.0], dtype=F64).reshape(1, 1, 2, 2, 1)
    pm = torch.full((1, 1, 2, 2, 1, 2), 0.5, dtype=F64)
    # bce = ln 2, dice = (2 + 1) / (2 + 2 + 1)
    assert float(HL.mask_loss(tm, ids, pm)) == pytest.approx(0.3 * math.log(2) + 0.7 * 0.4, abs=1e-6)
    assert 0.3 * math.log(2) + 0.7 * 0.4 == pytest.approx(0.487944, abs=1e-6)
    assert float(HL.mask_loss(torch.zeros_like(tm), ids, pm)) == 0.0      # the only positive is empty
    assert float(HL.mask_loss(tm, torch.zeros_like(ids), pm)) == 0.0      # no positives


def test_restatement_is_dtype_generic():
    g = torch.Generator().manual_seed(0)
    ids = torch.tensor([[0, 1, 2, 0]], dtype=torch.int32)
    args64 = (ids, torch.randn(1, 4, 6, generator=g, dtype=F64), torch.rand(1, 4, 2, 2, 2, generator=g, dtype=F64).round(),
              torch.randn(1, 4, 3, generator=g, dtype=F64), torch.randn(1, 4, 3, 6, generator=g, dtype=F64),
              torch.rand(1, 4, 2, 2, 2, 3, generator=g, dtype=F64), torch.ones(1, 3, dtype=F64))
    args32 = tuple(a.float() if a.is_floating_point() else a for a in args64)
    for a, b in zip(HL.losses(*args64), HL.losses(*args32)):
        assert b.dtype == torch.float32
        assert float(b) == pytest.approx(float(a), rel=1e-5)


def test_head_loss_invalid_arguments_are_rejected_without_touching_the_gpu():
    import m3d._lib as lib
    L = lib.load()
    N = None

    def fwd(B=1, T=4, C=2, V=8, gamma=3.0, ws=0x1000, ws_bytes=1 << 20):
        return L.m3d_head_loss_fwd(N, N, N, N, N, N, N, B, T, C, V, 0.85, gamma, 1.0, 1.0, 1.0, N, N, N, N, N,
                                   ws, ws_bytes, N)

    def bwd(B=1, T=4, C=2, V=8, gamma=3.0):
        return L.m3d_head_loss_bwd(N, N, N, N, N, N, N, B, T, C, V, 0.85, gamma, N, N, N, N, N, N)

    for call in (fwd, bwd):
        for kw in (dict(B=-1), dict(T=-1), dict(V=-1)):
            assert call(**kw) == -1 and b"negative" in L.m3d_last_error()
        assert call(C=1) == -1 and b"C must be >= 2" in L.m3d_last_error()
        assert call(gamma=0.5) == -1 and b"gamma must be >= 1" in L.m3d_last_error()
        assert call(B=1 << 20, T=1 << 10) == -1 and b"too many rows" in L.m3d_last_error()
        assert call(V=1 << 31) == -1 and b"mask volume too large" in L.m3d_last_error()
    need = L.m3d_head_loss_workspace_bytes(4, 8)
    assert need > 0
    assert L.m3d_head_loss_workspace_bytes(512, 28 ** 3) > L.m3d_head_loss_workspace_bytes(512, 64)
    assert fwd(ws_bytes=need - 1) == -1 and b"workspace too small" in L.m3d_last_error()
    assert L.m3d_head_loss_workspace_bytes(1 << 30, 8) == 0 and L.m3d_head_loss_workspace_bytes(4, 1 << 31) == 0
    # sizes in range, every pointer NULL: still refused before a launch
    assert fwd(ws_bytes=need) == -1 and b"NULL" in L.m3d_last_error()
    assert bwd() == -1 and b"NULL" in L.m3d_last_error()
