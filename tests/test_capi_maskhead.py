"""The mask-head training entry points of include/m3d.h (m3d_conv3d_bwd_data_dil,
m3d_conv3d_bwd_weight_dil, m3d_deconv3d_k2s2_bwd_data / _bwd_weight,
m3d_mask_out_bwd and its workspace query, m3d_add_f32) through the C-ABI without
a GPU: exported, declared, documented, and every rejection path returns
M3D_EINVAL before any launch."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m3d_conv3d_bwd_data_dil", "m3d_conv3d_bwd_weight_dil", "m3d_deconv3d_k2s2_bwd_data",
       "m3d_deconv3d_k2s2_bwd_weight", "m3d_mask_out_bwd_workspace_bytes", "m3d_mask_out_bwd", "m3d_add_f32")
FAKE = 0x1000           # a non-NULL pointer that must never be dereferenced
EINVAL = -1


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
    for name in ("m3d_conv3d_bwd_data_dil", "m3d_conv3d_bwd_weight_dil", "m3d_deconv3d_k2s2_bwd_data",
                 "m3d_mask_out_bwd", "m3d_add_f32"):
        comment = hdr[:hdr.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "core/models.py:" in comment, name
    assert L.m3d_abi_version() == 3
    for name in ("m3d_conv3d_bwd_weight_dil", "m3d_deconv3d_k2s2_bwd_weight"):
        assert name in lib.DET_ENTRY_POINTS           # they take the process's deterministic target


def _dgrad(L, cin=8, cout=32, k=(3, 3, 3), stride=(1, 1, 1), pad=(2, 2, 2), dil=(2, 2, 2), acc=0, sp=(5, 4, 3)):
    return L.m3d_conv3d_bwd_data_dil(FAKE, FAKE, 2, *sp, cin, *k, cout, *sp, *stride, *pad, *dil, FAKE, acc, None)


def test_bwd_data_dil_rejections():
    lib, L = _lib()
    for dil in ((0, 2, 2), (2, -1, 2), (2, 2, 0)):
        assert _dgrad(L, dil=dil) == EINVAL and b"dilation must be positive" in L.m3d_last_error()
    for stride in ((2, 1, 1), (1, 1, 2)):
        assert _dgrad(L, stride=stride) == EINVAL and b"stride must be 1" in L.m3d_last_error()
    assert _dgrad(L, stride=(2, 2, 2), k=(1, 1, 1), pad=(0, 0, 0)) == EINVAL       # strided even for 1^3 here
    for acc in (-1, 2):
        assert _dgrad(L, acc=acc) == EINVAL and b"accumulate must be 0 or 1" in L.m3d_last_error()
    assert _dgrad(L, cout=36) == EINVAL and b"Cout must be a multiple of 32" in L.m3d_last_error()
    assert _dgrad(L, cin=6) == EINVAL and b"Cin must be a multiple of 4" in L.m3d_last_error()
    assert _dgrad(L, sp=(0, 4, 3)) == EINVAL and b"positive" in L.m3d_last_error()
    assert _dgrad(L, k=(0, 3, 3)) == EINVAL and b"positive" in L.m3d_last_error()


def _wgrad(L, cin=8, cout=32, k=(3, 3, 3), dil=(2, 2, 2), sp=(5, 4, 3), det=None):
    return L.m3d_conv3d_bwd_weight_dil(FAKE, FAKE, 2, *sp, cin, *k, cout, *sp, 1, 1, 1, 2, 2, 2, *dil, FAKE, det, None)


def test_bwd_weight_dil_rejections():
    import ctypes
    lib, L = _lib()
    for dil in ((0, 2, 2), (2, -1, 2), (2, 2, 0)):
        assert _wgrad(L, dil=dil) == EINVAL and b"dilation must be positive" in L.m3d_last_error()
    assert _wgrad(L, cout=30) == EINVAL and b"Cout must be a multiple of 4" in L.m3d_last_error()
    assert _wgrad(L, sp=(5, 0, 3)) == EINVAL and b"positive" in L.m3d_last_error()
    assert _wgrad(L, k=(3, 3, -3)) == EINVAL and b"positive" in L.m3d_last_error()
    bad = lib.Det(1, None, 1 << 20)                   # deterministic mode without a scratch
    assert _wgrad(L, det=ctypes.addressof(bad)) == EINVAL and b"det->scratch" in L.m3d_last_error()


def test_deconv_bwd_rejections():
    import ctypes
    lib, L = _lib()
    for dims in ((0, 3, 3, 3, 32, 32), (2, 3, -3, 3, 32, 32), (2, 3, 3, 3, 0, 32), (2, 3, 3, 3, 32, 0)):
        assert L.m3d_deconv3d_k2s2_bwd_data(FAKE, FAKE, *dims, FAKE, None) == EINVAL
        assert b"positive" in L.m3d_last_error()
        assert L.m3d_deconv3d_k2s2_bwd_weight(FAKE, FAKE, *dims, FAKE, None, None) == EINVAL
        assert b"positive" in L.m3d_last_error()
    for cin, cout in ((30, 32), (32, 30)):
        assert L.m3d_deconv3d_k2s2_bwd_data(FAKE, FAKE, 2, 3, 3, 3, cin, cout, FAKE, None) == EINVAL
        assert b"Cin % 4 == 0 and Cout % 4 == 0" in L.m3d_last_error()
        assert L.m3d_deconv3d_k2s2_bwd_weight(FAKE, FAKE, 2, 3, 3, 3, cin, cout, FAKE, None, None) == EINVAL
        assert b"Cin % 4 == 0 and Cout % 4 == 0" in L.m3d_last_error()
    bad = lib.Det(1, None, 1 << 20)
    assert L.m3d_deconv3d_k2s2_bwd_weight(FAKE, FAKE, 2, 3, 3, 3, 32, 32, FAKE, ctypes.addressof(bad), None) == EINVAL


def _mob(L, V=1000, ch=64, C=2, ws=FAKE, wsb=None, ptrs=None):
    wsb = L.m3d_mask_out_bwd_workspace_bytes(V, ch, C) if wsb is None else wsb
    p = [FAKE] * 8 if ptrs is None else ptrs
    return L.m3d_mask_out_bwd(p[0], p[1], p[2], p[3], V, ch, C, p[4], p[5], p[6], p[7], ws, wsb, None)


def test_mask_out_bwd_rejections_and_workspace():
    lib, L = _lib()
    for V, ch, C in ((0, 64, 2), (-5, 64, 2), (100, 0, 2), (100, 64, 0), (100, 64, -1)):
        assert _mob(L, V, ch, C, wsb=1 << 20) == EINVAL and b"positive" in L.m3d_last_error()
        assert L.m3d_mask_out_bwd_workspace_bytes(V, ch, C) == 0
    assert _mob(L, C=9, wsb=1 << 20) == EINVAL and b"at most 8 classes" in L.m3d_last_error()
    for ch in (30, 1028):
        assert _mob(L, ch=ch, wsb=1 << 20) == EINVAL and b"multiple of 4, at most 1024" in L.m3d_last_error()
    need = L.m3d_mask_out_bwd_workspace_bytes(1000, 64, 2)
    assert _mob(L, wsb=need - 4) == EINVAL and b"workspace too small" in L.m3d_last_error()
    assert _mob(L, ws=None) == EINVAL and b"workspace too small" in L.m3d_last_error()
    for i in range(8):
        ptrs = [FAKE] * 8
        ptrs[i] = None
        assert _mob(L, ptrs=ptrs) == EINVAL and b"null tensor" in L.m3d_last_error()
    # one row of ch*C + ch + C partial sums per workgroup of 256 rows (1024 from 2^18 rows on)
    per = 4 * (64 * 2 + 64 + 2)
    assert need == 4 * per and L.m3d_mask_out_bwd_workspace_bytes(1024, 64, 2) == 4 * per
    assert L.m3d_mask_out_bwd_workspace_bytes(1025, 64, 2) == 5 * per
    assert L.m3d_mask_out_bwd_workspace_bytes((1 << 18) - 1, 64, 2) == 1024 * per
    assert L.m3d_mask_out_bwd_workspace_bytes(1 << 18, 64, 2) == 256 * per
    assert L.m3d_mask_out_bwd_workspace_bytes(100, 32, 5) == 4 * (32 * 5 + 32 + 5)


def test_add_f32_rejections():
    lib, L = _lib()
    assert L.m3d_add_f32(FAKE, FAKE, FAKE, 6, None) == EINVAL and b"multiple of 4" in L.m3d_last_error()
    assert L.m3d_add_f32(FAKE, FAKE, FAKE, -4, None) == EINVAL
    for i in range(3):
        ptrs = [FAKE] * 3
        ptrs[i] = None
        assert L.m3d_add_f32(*ptrs, 8, None) == EINVAL and b"null tensor" in L.m3d_last_error()
    assert L.m3d_add_f32(FAKE, FAKE, FAKE, 0, None) == 0                     # nothing to do, no launch


def test_host_layer_surface():
    """MaskHead.params / chunk_range and the train_heads argument check (no GPU:
    the store stays on the CPU)."""
    import pytest
    import torch
    from m3d.heads import ClassifierHead, MaskHead, MaskRCNN
    from m3d.params import CHUNK, ConvLayer, ParamStore
    store = ParamStore()
    ConvLayer(store, "before", (1, 1, 1), 4, 4)
    cls = ClassifierHead(store, 3, 2, 32, 8)
    head = MaskHead(store, 2, 32, 8)
    ConvLayer(store, "after", (1, 1, 1), 4, 4)
    store.finalize(torch.device("cpu"))
    ps = head.params()
    assert len(ps) == 24 and len(set(p.name for p in ps)) == 24
    lo, hi = head.chunk_range()
    assert lo == ps[0].offset // CHUNK and hi - lo == sum(-(-p.numel // CHUNK) for p in ps)
    assert cls.chunk_range()[1] == lo                       # the two heads are adjacent, as in MaskRCNN
    assert store.by_name["after/kernel:0"].offset == hi * CHUNK
    assert all(bn.momentum == 0.99 for _, bn in head.convs.values())
    assert MaskHead.ACTIVATIONS == ("bn1", "bn2", "bn3", "bn3b", "bn4", "deconv")
    with pytest.raises(ValueError, match="return_activations"):
        head(torch.zeros(1, 1, 3, 3, 3, 8), return_activations=True)
    for bad in ((), ("mask", "mask"), ("rpn",)):
        with pytest.raises(ValueError, match="heads"):
            MaskRCNN.train_heads(None, None, None, None, None, None, None, heads=bad)
