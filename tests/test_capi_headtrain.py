"""The head-training entry points of include/m3d.h (m3d_bn_train_*,
m3d_head_outputs_bwd, m3d_max_norm) through the C-ABI without a GPU: exported,
declared, and every rejection path returns M3D_EINVAL before any launch."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m3d_bn_train_few_rows_max", "m3d_bn_train_workspace_bytes", "m3d_bn_train_fwd", "m3d_bn_train_bwd",
       "m3d_head_outputs_bwd", "m3d_max_norm")
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
        assert re.search(r"\b" + name + r"\s*\(", code), name
    # each new group's comment names the reference lines it restates
    for name in ("m3d_bn_train_fwd", "m3d_head_outputs_bwd", "m3d_max_norm"):
        comment = hdr[:hdr.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "core/models.py:" in comment, name


def test_regime_constant_is_readable_and_matches_the_header():
    lib, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "m3d.h")).read()
    want = int(re.search(r"#define\s+M3D_BN_TRAIN_FEW_ROWS_MAX\s+(\d+)", hdr).group(1))
    assert L.m3d_bn_train_few_rows_max() == want
    from m3d import heads
    assert heads.bn_train_few_rows_max() == want
    # no workspace in the few-rows regime, partial rows above it
    assert L.m3d_bn_train_workspace_bytes(want, 32) == 0
    assert L.m3d_bn_train_workspace_bytes(want + 1, 32) > 0
    assert L.m3d_bn_train_workspace_bytes(1, 32) == 0 and L.m3d_bn_train_workspace_bytes(64, 6) == 0


def _fwd(L, M, C, ws=None, wsb=0, mm=FAKE, mv=FAKE, eps=1e-3):
    return L.m3d_bn_train_fwd(FAKE, M, C, FAKE, FAKE, eps, 0.9, 1, FAKE, FAKE, FAKE, mm, mv, ws, wsb, None)


def _bwd(L, M, C, ws=None, wsb=0, relu=1, y=FAKE):
    return L.m3d_bn_train_bwd(FAKE, y, FAKE, M, C, FAKE, FAKE, FAKE, relu, FAKE, FAKE, FAKE, ws, wsb, None)


def test_bn_train_rejections():
    lib, L = _lib()
    many = L.m3d_bn_train_few_rows_max() + 1
    for call in (_fwd, _bwd):
        assert call(L, 64, 6) == -1 and b"multiple of 4" in L.m3d_last_error()
        for M in (0, 1):
            assert call(L, M, 8) == -1 and b"M >= 2" in L.m3d_last_error()
        assert call(L, -3, 8) == -1 and b"positive" in L.m3d_last_error()
        assert call(L, 64, -8) == -1 and b"positive" in L.m3d_last_error()
        assert call(L, 64, 0) == -1 and b"positive" in L.m3d_last_error()
        need = L.m3d_bn_train_workspace_bytes(many, 32)
        assert call(L, many, 32, FAKE, need - 4) == -1 and b"workspace too small" in L.m3d_last_error()
        assert call(L, many, 32, None, need) == -1 and b"workspace too small" in L.m3d_last_error()
    assert _fwd(L, 64, 8, mm=FAKE, mv=None) == -1 and b"together" in L.m3d_last_error()
    assert _fwd(L, 64, 8, mm=None, mv=FAKE) == -1 and b"together" in L.m3d_last_error()
    assert _fwd(L, 64, 8, eps=0.0) == -1 and b"eps" in L.m3d_last_error()
    assert _bwd(L, 64, 8, relu=1, y=None) == -1 and b"relu needs y" in L.m3d_last_error()


def test_head_outputs_bwd_rejections():
    lib, L = _lib()
    for C in (2, 5):
        rc = L.m3d_head_outputs_bwd(FAKE, FAKE, FAKE, 10, 7 * C - 1, C, FAKE, None)
        assert rc == -1 and b"head_outputs_bwd" in L.m3d_last_error()
    assert L.m3d_head_outputs_bwd(FAKE, FAKE, FAKE, -1, 16, 2, FAKE, None) == -1
    assert L.m3d_head_outputs_bwd(FAKE, FAKE, FAKE, 10, 16, 0, FAKE, None) == -1
    assert L.m3d_head_outputs_bwd(FAKE, FAKE, FAKE, 10, 16, -2, FAKE, None) == -1
    assert L.m3d_head_outputs_bwd(FAKE, FAKE, FAKE, 0, 16, 2, FAKE, None) == 0          # nothing to do, no launch


def test_max_norm_rejections():
    lib, L = _lib()
    for rows, cols in ((0, 4), (4, 0), (-1, 4), (4, -1)):
        assert L.m3d_max_norm(FAKE, rows, cols, 1.0, None) == -1 and b"max_norm" in L.m3d_last_error()
    assert L.m3d_max_norm(FAKE, 4, 4, -1.0, None) == -1 and b"max_value" in L.m3d_last_error()
    assert L.m3d_max_norm(FAKE, 4, 4, float("nan"), None) == -1


def test_host_layer_surface():
    """BNLayer.momentum, the head's constraints and chunk range, and the
    optimizer's chunk-range validation (no GPU: the store stays on the CPU)."""
    import pytest
    import torch
    from m3d.heads import ClassifierHead
    from m3d.optim import KerasOptimizer, apply_max_norm  # noqa: F401
    from m3d.params import CHUNK, BNLayer, ConvLayer, ParamStore
    store = ParamStore()
    ConvLayer(store, "before", (1, 1, 1), 4, 4)
    other = BNLayer(store, "bn_other", 4)
    head = ClassifierHead(store, 3, 2, 32, 8)
    ConvLayer(store, "after", (1, 1, 1), 4, 4)
    store.finalize(torch.device("cpu"))
    assert other.momentum == 0.99 and head.bn1.momentum == 0.9 and head.bn2.momentum == 0.9
    assert head.max_norm_constraints == {"mrcnn_class_logits/kernel:0": 2.0, "mrcnn_bbox_fc/kernel:0": 1.0}
    lo, hi = head.chunk_range()
    ps = head.params()
    assert len(ps) == 12 and lo == ps[0].offset // CHUNK
    assert hi - lo == sum(-(-p.numel // CHUNK) for p in ps)
    assert store.by_name["after/kernel:0"].offset == hi * CHUNK
    with pytest.raises(ValueError, match="chunks"):
        KerasOptimizer({"name": "SGD"}).step(store, chunks=(hi, lo))
    with pytest.raises(ValueError, match="chunks"):
        KerasOptimizer({"name": "SGD"}).step(store, chunks=(0, store.n_chunks + 1))
