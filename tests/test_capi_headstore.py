"""The stored-head-target entry points of include/m3d.h (m3d_pack_bits_f32,
m3d_f32_to_f16, m3d_bits_row_counts, m3d_unpack_gather_bits,
m3d_unpack_gather_f16) through the C-ABI without a GPU: exported, declared,
documented, built from csrc/headstore.hip, and every rejection path returns
M3D_EINVAL before any launch."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m3d_pack_bits_f32", "m3d_f32_to_f16", "m3d_bits_row_counts", "m3d_unpack_gather_bits",
       "m3d_unpack_gather_f16")
FAKE = 0x1000           # a non-NULL, 16-byte aligned pointer that must never be dereferenced
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
    # each group's comment names the reference lines it restates
    for name, where in (("m3d_pack_bits_f32", "core/models.py:"), ("m3d_f32_to_f16", "core/models.py:"),
                        ("m3d_bits_row_counts", "core/data_generators.py:"),
                        ("m3d_unpack_gather_bits", "core/data_generators.py:")):
        comment = hdr[:hdr.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert where in comment, name
    assert L.m3d_abi_version() == 3                      # additions only
    mk = open(os.path.join(ROOT, "3d-mask-r-cnn_amd", "Makefile")).read()
    assert "csrc/headstore.hip" in mk


def test_pack_bits_rejections():
    lib, L = _lib()
    assert L.m3d_pack_bits_f32(FAKE, -1, FAKE, None) == EINVAL and b"negative" in L.m3d_last_error()
    assert L.m3d_pack_bits_f32(None, 8, FAKE, None) == EINVAL and b"NULL" in L.m3d_last_error()
    assert L.m3d_pack_bits_f32(FAKE, 8, None, None) == EINVAL and b"NULL" in L.m3d_last_error()
    for off in (4, 8, 12):                               # 16-byte loads: the input must be aligned for them
        assert L.m3d_pack_bits_f32(FAKE + off, 8, FAKE, None) == EINVAL and b"aligned" in L.m3d_last_error()
    assert L.m3d_pack_bits_f32(None, 0, None, None) == 0                 # nothing to do, no launch


def test_f32_to_f16_rejections():
    lib, L = _lib()
    assert L.m3d_f32_to_f16(FAKE, -4, FAKE, None) == EINVAL and b"negative" in L.m3d_last_error()
    assert L.m3d_f32_to_f16(None, 4, FAKE, None) == EINVAL and b"NULL" in L.m3d_last_error()
    assert L.m3d_f32_to_f16(FAKE, 4, None, None) == EINVAL and b"NULL" in L.m3d_last_error()
    assert L.m3d_f32_to_f16(FAKE + 8, 4, FAKE, None) == EINVAL and b"aligned" in L.m3d_last_error()
    for off in (2, 4, 6):                                # 8-byte stores
        assert L.m3d_f32_to_f16(FAKE, 4, FAKE + off, None) == EINVAL and b"aligned" in L.m3d_last_error()
    assert L.m3d_f32_to_f16(None, 0, None, None) == 0


def test_bits_row_counts_rejections():
    lib, L = _lib()
    assert L.m3d_bits_row_counts(FAKE, -1, 8, FAKE, None) == EINVAL and b"rows" in L.m3d_last_error()
    assert L.m3d_bits_row_counts(FAKE, 1 << 31, 8, FAKE, None) == EINVAL and b"rows" in L.m3d_last_error()
    for rb in (0, -3, 1 << 31):
        assert L.m3d_bits_row_counts(FAKE, 5, rb, FAKE, None) == EINVAL and b"row_bits" in L.m3d_last_error()
    assert L.m3d_bits_row_counts(None, 5, 27, FAKE, None) == EINVAL and b"NULL" in L.m3d_last_error()
    assert L.m3d_bits_row_counts(FAKE, 5, 27, None, None) == EINVAL and b"NULL" in L.m3d_last_error()
    assert L.m3d_bits_row_counts(FAKE + 1, 5, 27, FAKE, None) == EINVAL and b"aligned" in L.m3d_last_error()
    assert L.m3d_bits_row_counts(FAKE, 5, 27, FAKE + 2, None) == EINVAL and b"aligned" in L.m3d_last_error()
    assert L.m3d_bits_row_counts(None, 0, 27, None, None) == 0


def _ug(fn, R=5, S=(4, 3, 2), C=8, T=3, M=(3, 3, 2), ptrs=None):
    p = [FAKE] * 6 if ptrs is None else ptrs             # src, sel, i0, i1, i2, out
    return fn(p[0], R, *S, C, p[1], T, p[2], p[3], p[4], *M, p[5], None)


def test_unpack_gather_rejections():
    lib, L = _lib()
    for fn, nm in ((L.m3d_unpack_gather_bits, b"unpack_gather_bits"), (L.m3d_unpack_gather_f16, b"unpack_gather_f16")):
        assert _ug(fn, R=0) == EINVAL and nm in L.m3d_last_error() and b"positive" in L.m3d_last_error()
        for S in ((0, 3, 2), (4, -1, 2), (4, 3, 0)):
            assert _ug(fn, S=S) == EINVAL and b"positive" in L.m3d_last_error()
        assert _ug(fn, C=0) == EINVAL and b"positive" in L.m3d_last_error()
        assert _ug(fn, T=0) == EINVAL and b"positive" in L.m3d_last_error()
        for M in ((0, 3, 2), (3, 0, 2), (3, 3, -2)):
            assert _ug(fn, M=M) == EINVAL and b"positive" in L.m3d_last_error()
        assert _ug(fn, S=(1 << 31, 3, 2)) == EINVAL and b"2^31" in L.m3d_last_error()
        assert _ug(fn, T=1 << 20, M=(1 << 12, 3, 2)) == EINVAL and b"2^31" in L.m3d_last_error()
        assert _ug(fn, M=(3, 3, 1 << 29)) == EINVAL and b"2^31" in L.m3d_last_error()
        assert _ug(fn, R=1 << 40, S=((1 << 31) - 1,) * 3) == EINVAL and b"too many" in L.m3d_last_error()
        for i in range(6):
            ptrs = [FAKE] * 6
            ptrs[i] = None
            assert _ug(fn, ptrs=ptrs) == EINVAL and b"NULL" in L.m3d_last_error()
        ptrs = [FAKE] * 5 + [FAKE + 4]                   # float4 stores when C % 4 == 0
        assert _ug(fn, ptrs=ptrs) == EINVAL and b"out must be 16-byte aligned" in L.m3d_last_error()
        ptrs = [FAKE] * 5 + [FAKE + 2]
        assert _ug(fn, C=1, ptrs=ptrs) == EINVAL and b"aligned" in L.m3d_last_error()
    ptrs = [FAKE + 4] + [FAKE] * 5                       # 8-byte loads of four halves
    assert _ug(L.m3d_unpack_gather_f16, ptrs=ptrs) == EINVAL and b"float16 source" in L.m3d_last_error()
    ptrs = [FAKE + 1] + [FAKE] * 5
    assert _ug(L.m3d_unpack_gather_f16, C=3, ptrs=ptrs) == EINVAL and b"float16 source" in L.m3d_last_error()


def test_host_wrappers_refuse_cpu_tensors_and_bad_rows():
    import pytest
    import torch
    from m3d import headstore
    with pytest.raises(ValueError, match="GPU"):
        headstore.pack_bits(torch.zeros(8))
    with pytest.raises(ValueError, match="GPU"):
        headstore.to_half(torch.zeros(8))
    with pytest.raises(ValueError, match="GPU"):
        headstore.bits_row_counts(torch.zeros(8, dtype=torch.uint8), 2, 32)
    with pytest.raises(ValueError, match="GPU"):
        headstore.unpack_gather(torch.zeros(8, dtype=torch.uint8), (1, 2, 2, 2, 8), [0])
    with pytest.raises(ValueError, match="train_heads_on_features"):
        from m3d.heads import MaskRCNN
        MaskRCNN.train_heads_on_features(None, None, None, None, None, None, None, None, heads=("rpn",))
