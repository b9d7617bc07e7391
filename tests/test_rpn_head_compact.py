"""The compact RPN head backward without a GPU: the float64 restatement the GPU
tests compare against (tests/headref.py) pinned by hand-derived cases, and the
C-ABI of m3d_rpn_head_compact_* (exported, declared, documented; every invalid
argument is M3D_EINVAL before any launch)."""
import ctypes
import os
import re

import numpy as np

import headref as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("m3d_rpn_head_compact_workspace_bytes", "m3d_rpn_head_compact_bwd_data", "m3d_rpn_head_compact_bwd_weight")
FAKE = 0x1000           # a non-NULL pointer that must never be dereferenced


# --------------------------------------------------------------------------- the restatement
def _one_voxel(s1, s2):
    """one level of one voxel, one channel everywhere, apl = 1"""
    w1 = np.zeros((3, 3, 3, 1, 1))
    w1[1, 1, 1] = 3.0
    w1[0, 1, 1] = 100.0                                  # reaches no voxel of a 1 x 1 x 1 level
    dl, db = np.array([[1.0, 0.0]]), np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 2.0]])
    w24 = np.arange(1.0, 9.0).reshape(1, 8)
    return HR.head_backward(dl, db, [np.full((1, 1, 1, 1), s1)], [np.full((1, 1, 1, 1), s2)],
                            [np.full((1, 1, 1, 1), 2.0)], w1, np.array([[0.5]]), w24)


def test_restatement_one_voxel_by_hand():
    """P = 2, w1 = 3 -> s1 = 6, w2 = 0.5 -> s2 = 3; dz3 = (1, 0, ..., 0, 2), w24 = (1..8):
    dz2 = 1 * 1 + 2 * 8 = 17, dz1 = 17 * 0.5 = 8.5, dP = 8.5 * 3 = 25.5"""
    g = _one_voxel(6.0, 3.0)
    assert g["db24"].tolist() == [1, 0, 0, 0, 0, 0, 0, 2]
    assert g["dw24"].tolist() == [[3, 0, 0, 0, 0, 0, 0, 6]]
    assert g["db2"].tolist() == [17] and g["dw2"].tolist() == [[6 * 17]]
    assert g["db1"].tolist() == [8.5]
    want = np.zeros((3, 3, 3, 1, 1))
    want[1, 1, 1] = 2 * 8.5
    assert np.array_equal(g["dw1"], want)
    assert g["dP"][0].tolist() == [[[[25.5]]]]


def test_restatement_relu_masks_by_hand():
    """s2 = 0 exactly stops everything below the class/bbox pair (ReLU'(0) = 0); s1 <= 0 with
    s2 > 0 stops rpn_conv_shared1 only, and dw2 = s1 * dz2 keeps the sign of s1"""
    g = _one_voxel(6.0, 0.0)
    assert g["db24"].tolist() == [1, 0, 0, 0, 0, 0, 0, 2] and not g["dw24"].any()
    assert not g["db2"].any() and not g["dw2"].any() and not g["db1"].any() and not g["dw1"].any()
    assert not g["dP"][0].any()
    g = _one_voxel(-1.0, 3.0)
    assert g["db2"].tolist() == [17] and g["dw2"].tolist() == [[-17]]
    assert not g["db1"].any() and not g["dw1"].any() and not g["dP"][0].any()


def test_restatement_taps_and_levels_by_hand():
    """Level 0 is 1 x 1 x 2 (x = (5, 7)), level 1 is 1 x 1 x 1 (x = 11); channels 1, w2 = w24-row = 1
    so dz1 = dz3's first column where the masks pass.  Only the z taps w1[1, 1, kz] = (2, 3, 4) reach a
    voxel.  Active: row 0 (d = 1) and row 2, level 1's only row (d = 10); row 1 holds zeros.
    y[z] = sum_kz x[z + kz - 1] w[kz], so y[0] = x[0] w[1] + x[1] w[2]:  dP0[0] = d w[1] = 3,
    dP0[1] = d w[2] = 4, dP1[0] = 10 * 3;  dw1[1,1,1] = 5 * 1 + 11 * 10, dw1[1,1,2] = 7 * 1,
    dw1[1,1,0] = 0 (no voxel lies below z = 0)."""
    w1 = np.zeros((3, 3, 3, 1, 1))
    w1[1, 1, :, 0, 0] = (2.0, 3.0, 4.0)
    dl = np.array([[1.0, 0.0], [0.0, 0.0], [10.0, 0.0]])
    db = np.zeros((3, 6))
    w24 = np.zeros((1, 8))
    w24[0, 0] = 1.0
    P = [np.array([5.0, 7.0]).reshape(1, 1, 2, 1), np.array([11.0]).reshape(1, 1, 1, 1)]
    ones = [np.ones((1, 1, 2, 1)), np.ones((1, 1, 1, 1))]
    g = HR.head_backward(dl, db, ones, ones, P, w1, np.array([[1.0]]), w24)
    assert g["dP"][0].reshape(-1).tolist() == [3.0, 4.0]
    assert g["dP"][1].reshape(-1).tolist() == [30.0]
    assert g["dw1"][1, 1, :, 0, 0].tolist() == [0.0, 5.0 + 110.0, 7.0]
    assert g["db1"].tolist() == [11.0] and g["dw2"].tolist() == [[11.0]]
    # accumulate: dP0 is added, voxel for voxel
    g2 = HR.head_backward(dl, db, ones, ones, P, w1, np.array([[1.0]]), w24, dP0=[np.full((1, 1, 2, 1), 0.5),
                                                                                np.full((1, 1, 1, 1), -1.0)])
    assert g2["dP"][0].reshape(-1).tolist() == [3.5, 4.5] and g2["dP"][1].reshape(-1).tolist() == [29.0]


def test_scan_restatement_by_hand():
    dl, db = np.zeros((7, 2), np.float32), np.zeros((7, 6), np.float32)
    dl[1, 1] = 2.0
    db[3, 5] = -1.0                    # active through dbbox only
    dl[4] = -0.0                       # only negative zeros: inactive
    db[4] = -0.0
    db[6, 0] = np.nan                  # a NaN is active
    n, idx, slot, first = HR.scan(dl, db, 256, [0, 2, 4, 7])
    assert n == 3 and idx.tolist() == [1, 3, 6]
    assert slot.tolist() == [-1, 0, -1, 1, -1, -1, 2]
    assert first == [0, 1, 2, 3]
    n, idx, slot, first = HR.scan(dl, db, 2, [0, 2, 4, 7])             # cut at cap
    assert n == 3 and idx.tolist() == [1, 3] and slot.tolist() == [-1, 0, -1, 1, -1, -1, -1]
    assert first == [0, 1, 2, 2]


# --------------------------------------------------------------------------- the C-ABI
def _lib():
    import m3d._lib as lib
    return lib, lib.load()


def _args(lib, **over):
    """a valid argument block on fake pointers (levels 2 x 2 x 8 and 1 x 1 x 8, head channels)"""
    a = lib.RpnHeadBwd()
    a.nlevels, a.apl, a.cap, a.C0, a.C1, a.C2 = 2, 3, 256, 256, 512, 256
    for l, hw in enumerate((2, 1)):
        lv = a.levels[l]
        lv.p = lv.s1 = lv.s2 = lv.dp = FAKE
        lv.H, lv.W, lv.D, lv.accumulate = hw, hw, 8, 0
    for k in ("dlogits", "dbbox", "w1", "w2", "w24", "dw1", "db1", "dw2", "db2", "dw24", "db24", "workspace"):
        setattr(a, k, FAKE)
    a.ws_bytes = 1 << 40
    for k, v in over.items():
        if k.startswith("level_"):
            setattr(a.levels[0], k[6:], v)
        else:
            setattr(a, k, v)
    return a


def _both(lib, L, a):
    rc = (L.m3d_rpn_head_compact_bwd_data(ctypes.addressof(a), None),
          L.m3d_rpn_head_compact_bwd_weight(ctypes.addressof(a), None, None))
    return rc, L.m3d_last_error()


def test_symbols_exported_declared_and_documented():
    lib, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "m3d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert hasattr(L, name) and name in lib.EXPORTED
        assert re.search(r"\b(?:int|size_t) " + name + r"\s*\(", code), name
    comment = hdr[:hdr.index("#define M3D_RPN_HEAD_MAX_LEVELS")].rsplit("/* RPN head backward", 1)[1]
    assert "*/" not in comment.rstrip()[:-2]                 # the comment directly above the declarations
    for word in NAMES + ("core/models.py:512-557", "sticky", "NaN", "graph-replay", "!= 0.0f", "det"):
        assert word in comment, word
    for t in ("m3d_rpn_head_level_t", "m3d_rpn_head_bwd_t"):
        assert t in code
    assert L.m3d_abi_version() == 3                          # an addition only
    assert "m3d_rpn_head_compact_bwd_weight" in lib.DET_ENTRY_POINTS
    # the ctypes mirror has the header's layout: 4 + 3 * 2 ... words, levels of 4 pointers and 4 ints
    assert ctypes.sizeof(lib.RpnHeadLevel) == 4 * 8 + 4 * 4
    assert ctypes.sizeof(lib.RpnHeadBwd) == 16 + 24 + 8 * 48 + 12 * 8 + 8
    assert lib.RPN_HEAD_MAX_LEVELS == int(re.search(r"#define M3D_RPN_HEAD_MAX_LEVELS (\d+)", hdr).group(1))


def test_workspace_bytes():
    lib, L = _lib()
    f = L.m3d_rpn_head_compact_workspace_bytes
    nb = f(272, 256, 3, 256, 512, 256)
    assert nb > 0 and nb % 256 == 0
    # at least the matrices the header comment lists
    assert nb >= 4 * 256 * (32 + 2 * 256 + 2 * 512 + 2 * 27 * 256) + 6 * 27 * 256 * 512 + 8 * (256 // 64) * 512 * 256
    assert f(272, 512, 3, 256, 512, 256) > nb and f(100000, 256, 3, 256, 512, 256) > nb
    for bad in ((0, 256, 3, 256, 512, 256), (272, 0, 3, 256, 512, 256), (272, 300, 3, 256, 512, 256),
                (272, 4352, 3, 256, 512, 256), (272, 256, 0, 256, 512, 256), (272, 256, 9, 256, 512, 256),
                (272, 256, 3, 0, 512, 256)):
        assert f(*bad) == 0, bad


def test_invalid_arguments_are_rejected_before_any_launch():
    lib, L = _lib()
    assert L.m3d_rpn_head_compact_bwd_data(None, None) == -1 and b"NULL argument block" in L.m3d_last_error()
    assert L.m3d_rpn_head_compact_bwd_weight(None, None, None) == -1
    for over, msg in (({"cap": 300}, b"multiple of 256"), ({"cap": 4352}, b"multiple of 256"), ({"cap": 0}, b"multiple of 256"),
                      ({"nlevels": 0}, b"nlevels"), ({"nlevels": 9}, b"nlevels"), ({"apl": 0}, b"apl"), ({"apl": 9}, b"apl"),
                      ({"C1": 500}, b"channel counts"), ({"C0": 0}, b"channel counts"),
                      ({"level_H": 0}, b"extents"), ({"level_D": -1}, b"extents"),
                      ({"level_s1": None}, b"NULL level pointer"), ({"level_p": None}, b"NULL level pointer"),
                      ({"workspace": None}, b"workspace"), ({"ws_bytes": 1 << 20}, b"workspace")):
        rc, err = _both(lib, L, _args(lib, **over))
        assert rc == (-1, -1) and msg in err, (over, rc, err)
    need = L.m3d_rpn_head_compact_workspace_bytes(2 * 2 * 8 + 8, 256, 3, 256, 512, 256)
    rc, err = _both(lib, L, _args(lib, ws_bytes=need - 1))
    assert rc == (-1, -1) and b"too small" in err
    # what only one of the two calls needs
    for k in ("dlogits", "dbbox", "w1", "w2", "w24", "db1", "db2", "db24"):
        a = _args(lib, **{k: None})
        assert L.m3d_rpn_head_compact_bwd_data(ctypes.addressof(a), None) == -1 and b"NULL pointer" in L.m3d_last_error(), k
    for k in ("dw1", "dw2", "dw24"):
        a = _args(lib, **{k: None})
        assert L.m3d_rpn_head_compact_bwd_weight(ctypes.addressof(a), None, None) == -1
        assert b"NULL weight gradient" in L.m3d_last_error(), k
    a = _args(lib, level_dp=None)
    assert L.m3d_rpn_head_compact_bwd_data(ctypes.addressof(a), None) == -1 and b"NULL level pointer" in L.m3d_last_error()
    a = _args(lib, w2=FAKE + 4)
    assert L.m3d_rpn_head_compact_bwd_data(ctypes.addressof(a), None) == -1 and b"16-byte aligned" in L.m3d_last_error()
    a = _args(lib, level_accumulate=2)
    assert L.m3d_rpn_head_compact_bwd_data(ctypes.addressof(a), None) == -1 and b"accumulate" in L.m3d_last_error()
    d = lib.Det(1, None, 1 << 20)                           # a bad det is refused like everywhere else
    a = _args(lib)
    assert L.m3d_rpn_head_compact_bwd_weight(ctypes.addressof(a), ctypes.addressof(d), None) == -1
    assert b"det->scratch" in L.m3d_last_error()


def test_host_surface():
    """the route's switches and the bound's path from the targets to the head"""
    import inspect

    import torch
    from m3d import backbone, model, nn, targets
    assert nn.RPN_HEAD_COMPACT is True and nn.RPN_HEAD_COMPACT_MIN_ROWS > 5456      # the pinned launch plan's rows
    assert hasattr(backbone.RPNHead, "check_compact") and hasattr(backbone.RPNHead, "forward_levels")
    match = np.zeros((1, 40, 1), np.int32)
    match[0, [1, 5, 9]] = 1
    match[0, [2, 30]] = -1
    t = model.RPNTargets(match, np.zeros((1, 8, 6), np.float32), torch.device("cpu"))
    assert t.active_rows_bound == 5 == t.n_cls
    two = model.RPNTargets(np.concatenate([match, match]), np.zeros((2, 8, 6), np.float32), torch.device("cpu"))
    assert two.active_rows_bound is None                                         # B = 1 only
    d = model.DeviceRPNTargets(torch.zeros(40, dtype=torch.int8), torch.zeros(8, 6))
    assert d.active_rows_bound is None                                           # hand-made: stays dense
    assert model.DeviceRPNTargets(d.match, d.bbox, active_rows_bound=7).active_rows_bound == 7
    assert "active_rows_bound=self.total" in inspect.getsource(targets.RPNTargetBuilder.__call__)
    assert "active_rows_bound" in inspect.getsource(model.RPN.forward_backward)
