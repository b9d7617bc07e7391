"""m3d_rpn_head_compact_bwd_data / _bwd_weight (csrc/rpn_head_bwd.hip, "the RPN head's
backward on the sampled anchors' rows") against the float64 restatement of
tests/headref.py, and the route through backbone.RPNHead against the dense one.

Entry-point level: the head's channels (256 / 512 / 256, apl = 3) on levels
6x4x8, 3x2x8, 2x1x8, 1x1x8, 1x1x8 (R = 272: no level is a multiple of the 64-row
scan block, level boundaries fall inside blocks), cap = 256.  Bars, each
against the float64 result's largest magnitude: 1e-4 for the data gradients and
2e-5 for rpn_conv_shared1's weight gradient (the bars tests/test_gpu_rowsparse.py
sets for the same GEMMs), 1e-4 for the 1x1x1 tensors; and the compact result's
error may not exceed that of the dense entry points on the same inputs
scattered to dense form.  Model level: tests/test_gpu_rowsparse.py's 64x64x16
RPN with 256 sampled anchors."""
import ctypes

import numpy as np
import pytest
import torch

import headref as HR

pytestmark = pytest.mark.gpu

LEVELS = ((6, 4, 8), (3, 2, 8), (2, 1, 8), (1, 1, 8), (1, 1, 8))
ROWS = [h * w * d for h, w, d in LEVELS]
ROW0 = np.concatenate([[0], np.cumsum(ROWS)]).tolist()
R = ROW0[-1]
C0, C1, C2, APL, CAP, NPAD = 256, 512, 256, 3, 256, 32
N8 = 8 * APL
SETS = ("none", "row0", "level_firsts_and_last", "level1_empty", "all_of_level2", "bbox_only", "negative_zero",
        "n256", "n257")


@pytest.fixture(autouse=True)
def _mode_reset():
    from m3d import _lib
    yield
    _lib.set_deterministic(False)


def _active(which):
    """(active rows, rows written with -0.0 only)"""
    rng = np.random.default_rng(len(which))
    if which == "none":
        return [], []
    if which == "row0":
        return [0], []
    if which == "level_firsts_and_last":
        return ROW0[:-1] + [R - 1], []
    if which == "level1_empty":
        return [r for r in (3, 64, 100, 191, 245, 250, 257, 270)], []
    if which == "all_of_level2":
        return list(range(ROW0[2], ROW0[3])), []
    if which == "bbox_only":
        return [5, 200], []
    if which == "negative_zero":
        return [7, 63, 128], [8, 64]
    n = {"n256": 256, "n257": 257}[which]
    return sorted(rng.choice(R, n, replace=False).tolist()), []


def _gradient(which):
    rng = np.random.default_rng(11 + len(which))
    act, negz = _active(which)
    dl, db = np.zeros((R, 2 * APL), np.float32), np.zeros((R, 6 * APL), np.float32)
    dl[act] = rng.normal(size=(len(act), 2 * APL)).astype(np.float32)
    db[act] = rng.normal(size=(len(act), 6 * APL)).astype(np.float32)
    if which == "bbox_only":
        dl[5] = 0.0                             # row 5: a single bbox element only
        db[5] = 0.0
        db[5, 17] = 0.25
    dl[negz] = -0.0
    db[negz] = -0.0
    return dl, db


@pytest.fixture(scope="module")
def operands():
    """s1 / s2: about half the entries <= 0, some exactly 0 (they are ReLU outputs in the model; the
    entry points only read their signs and values)"""
    rng = np.random.default_rng(3)
    P = [rng.normal(size=(*sp, C0)).astype(np.float32) for sp in LEVELS]
    s1 = [rng.normal(size=(*sp, C1)).astype(np.float32) for sp in LEVELS]
    s2 = [rng.normal(size=(*sp, C2)).astype(np.float32) for sp in LEVELS]
    for a in s1 + s2:
        a[rng.random(a.shape) < 0.05] = 0.0
    w1 = rng.normal(0, 1.0 / np.sqrt(27 * C1), (3, 3, 3, C0, C1)).astype(np.float32)
    w2 = rng.normal(0, 1.0 / np.sqrt(C2), (C1, C2)).astype(np.float32)
    w24 = rng.normal(0, 1.0 / np.sqrt(N8), (C2, N8)).astype(np.float32)
    dP0 = [rng.normal(0, 0.5, (*sp, C0)).astype(np.float32) for sp in LEVELS]
    return {"P": P, "s1": s1, "s2": s2, "w1": w1, "w2": w2, "w24": w24, "dP0": dP0}


_REF = {}


def _ref(which, op):
    """the float64 result of a set, computed once and shared (read-only)"""
    if which not in _REF:
        dl, db = _gradient(which)
        _REF[which] = HR.head_backward(dl, db, op["s1"], op["s2"], op["P"], op["w1"], op["w2"], op["w24"])
    return _REF[which]


class _Dev:
    """the operands on the device, and one compact call"""

    def __init__(self, op, cuda):
        from m3d import _lib as lib
        self.lib, self.L, self.cuda = lib, lib.load(), cuda
        t = lambda a: torch.from_numpy(a).to(cuda)      # noqa: E731
        self.P, self.s1, self.s2 = ([t(a) for a in op[k]] for k in ("P", "s1", "s2"))
        self.w1, self.w2, self.w24 = t(op["w1"]), t(op["w2"]), t(op["w24"])
        self.dP0 = [t(a) for a in op["dP0"]]
        self.wsb = int(self.L.m3d_rpn_head_compact_workspace_bytes(R, CAP, APL, C0, C1, C2))
        assert self.wsb > 0

    def buffers(self, acc):
        g = {"dw1": torch.zeros_like(self.w1), "db1": torch.zeros(C1, device=self.cuda),
             "dw2": torch.zeros_like(self.w2), "db2": torch.zeros(C2, device=self.cuda),
             "dw24": torch.zeros((C2, NPAD), device=self.cuda), "db24": torch.zeros(NPAD, device=self.cuda)}
        g["dP"] = [a.clone() if acc else torch.full_like(a, 7.0) for a in self.dP0]
        return g

    def block(self, dl, db, g, ws, acc):
        a = self.lib.RpnHeadBwd()
        a.nlevels, a.apl, a.cap, a.C0, a.C1, a.C2 = len(LEVELS), APL, CAP, C0, C1, C2
        for l, sp in enumerate(LEVELS):
            lv = a.levels[l]
            lv.p, lv.s1, lv.s2, lv.dp = (x.data_ptr() for x in (self.P[l], self.s1[l], self.s2[l], g["dP"][l]))
            lv.H, lv.W, lv.D = sp
            lv.accumulate = acc
        a.dlogits, a.dbbox = dl.data_ptr(), db.data_ptr()
        a.w1, a.w2, a.w24 = self.w1.data_ptr(), self.w2.data_ptr(), self.w24.data_ptr()
        for k in ("dw1", "db1", "dw2", "db2", "dw24", "db24"):
            setattr(a, k, g[k].data_ptr())
        a.workspace, a.ws_bytes = ws.data_ptr(), self.wsb
        return a

    def launch(self, a):
        self.lib.check(self.L.m3d_rpn_head_compact_bwd_data(ctypes.addressof(a), self.lib.stream()), "bwd_data")
        self.lib.check(self.L.m3d_rpn_head_compact_bwd_weight(ctypes.addressof(a), self.lib.stream()), "bwd_weight")

    def run(self, dl, db, acc, ws=None):
        dl, db = torch.from_numpy(dl).to(self.cuda), torch.from_numpy(db).to(self.cuda)
        ws = torch.zeros(self.wsb // 4 + 1, device=self.cuda) if ws is None else ws
        g = self.buffers(acc)
        self.launch(self.block(dl, db, g, ws, acc))
        torch.cuda.synchronize()
        return g, ws

    def header(self, ws):
        """(n raw, n clamped, overflow word, level firsts, idx, slot) of a workspace"""
        h = ws.view(torch.int32).cpu().numpy()
        al = lambda n: (n + 63) // 64 * 64      # noqa: E731  (256 bytes, in ints)
        o_slot = al(64 + 4096) + al((R + 63) // 64)
        return (int(h[8]), int(h[3]), int(h[16]), h[32:32 + len(LEVELS) + 1].tolist(), h[64:64 + 4096],
                h[o_slot:o_slot + R])

    def dense(self, dl, db):
        """the same backward through today's dense entry points, level by level (nn._RPNOut's and the
        conv units' calls; the ReLU masks in between by torch)"""
        from m3d import nn as mnn
        lib, L, cuda = self.lib, self.L, self.cuda
        g = self.buffers(0)
        dz3 = torch.zeros((R, NPAD), device=cuda)
        dz3[:, :2 * APL] = torch.from_numpy(dl).to(cuda)
        dz3[:, 2 * APL:N8] = torch.from_numpy(db).to(cuda)
        w_pad = torch.nn.functional.pad(self.w24, (0, NPAD - N8)).contiguous()
        mnn.bias_grad(dz3, R, NPAD, g["db24"])
        w2p = mnn.X3_PLANES.get(self.w2, C1, C2, False)
        for l, (H, W, D) in enumerate(LEVELS):
            r0, r1 = ROW0[l], ROW0[l + 1]
            d3 = dz3[r0:r1].contiguous()
            one = (1, 1, 1, 0, 0, 0)                     # strides, pads
            dz2 = torch.empty((r1 - r0, C2), device=cuda)
            lib.check(L.m3d_conv3d_bwd_data(d3.data_ptr(), w_pad.data_ptr(), 1, H, W, D, C2, 1, 1, 1, NPAD, H, W, D, *one,
                                            dz2.data_ptr(), 0, lib.stream()), "dense dz2")
            lib.check(L.m3d_conv3d_bwd_weight(self.s2[l].data_ptr(), d3.data_ptr(), 1, H, W, D, C2, 1, 1, 1, NPAD, H, W,
                                              D, *one, g["dw24"].data_ptr(), lib.stream()), "dense dw24")
            dz2 = dz2 * (self.s2[l].reshape(-1, C2) > 0)
            mnn.bias_grad(dz2, r1 - r0, C2, g["db2"])
            # rpn_conv_shared2's data gradient through m3d_conv3d_bwd_data_x3, the entry point it runs on at
            # the sizes where the compact route is taken (nn._conv1_x3: P2 / P3 of a 64^3 volume and up)
            dz1 = torch.empty((r1 - r0, C1), device=cuda)
            lib.check(L.m3d_conv3d_bwd_data_x3(dz2.data_ptr(), w2p.data_ptr(), 1, H, W, D, C1, C2, dz1.data_ptr(),
                                               lib.stream()), "dense dz1")
            lib.check(L.m3d_conv3d_bwd_weight(self.s1[l].data_ptr(), dz2.data_ptr(), 1, H, W, D, C1, 1, 1, 1, C2, H, W, D,
                                              *one, g["dw2"].data_ptr(), lib.stream()), "dense dw2")
            dz1 = dz1 * (self.s1[l].reshape(-1, C1) > 0)
            mnn.bias_grad(dz1, r1 - r0, C1, g["db1"])
            nb = int(L.m3d_conv3d_wino_workspace_bytes(1, H, W, D, D, C0, C1))
            ws = torch.zeros(nb // 4 + 1, device=cuda)
            lib.check(L.m3d_conv3d_bwd_data_wino_rs(dz1.data_ptr(), self.w1.data_ptr(), 1, H, W, D, C0, C1, D, 1,
                                                    g["dP"][l].data_ptr(), 0, ws.data_ptr(), nb, 0, 0, None, 1,
                                                    lib.stream()), "dense dP")
            lib.check(L.m3d_conv3d_bwd_weight_wino_ux(None, self.P[l].data_ptr(), dz1.data_ptr(), 1, H, W, D, C0, C1, D, 1,
                                                      g["dw1"].data_ptr(), ws.data_ptr(), nb, 1, lib.stream()), "dense dw1")
        torch.cuda.synchronize()
        return g


@pytest.fixture(scope="module")
def dev(operands, cuda):
    return _Dev(operands, cuda)


def _err(got, ref):
    return float(np.abs(got.double().cpu().numpy() - ref).max())


def _flat(g):
    """name -> tensor of one result; dw24 / db24 without their padding columns"""
    out = {k: g[k] for k in ("dw1", "db1", "dw2", "db2")}
    out["dw24"], out["db24"] = g["dw24"][:, :N8], g["db24"][:N8]
    for l, a in enumerate(g["dP"]):
        out[f"dP{l}"] = a
    return out


@pytest.mark.parametrize("which", SETS[:-1])
def test_compact_backward(dev, operands, which):
    """scan outputs exactly; every gradient against float64, with accumulate 0 and 1; untouched voxels.

    The compact chain keeps double running sums in its 1x1x1 products and sums, so those tensors are
    rounded once where the dense entry points round along the way: that is what `es <= ed` rests on
    for them (with both forms on the same split GEMM the order of the last roundings decided it, and
    four sets missed by 15-30 %); for rpn_conv_shared1 it rests on the dense form being Winograd."""
    dl, db = _gradient(which)
    n, idx, slot, first = HR.scan(dl, db, CAP, ROW0)
    assert n == len(_active(which)[0])
    ref = _ref(which, operands)
    dense = _flat(dev.dense(dl, db))
    for acc in (0, 1):
        g, ws = dev.run(dl, db, acc)
        hn, hc, over, hfirst, hidx, hslot = dev.header(ws)
        assert (hn, hc, over) == (n, n, 0)
        assert hidx[:n].tolist() == idx.tolist() and np.array_equal(hslot, slot) and hfirst == first
        assert not g["dw24"][:, N8:].any() and not g["db24"][N8:].any()           # the padding columns
        got = _flat(g)
        for k, t in got.items():
            want = ref[k] if not k.startswith("dP") else ref["dP"][int(k[2:])] + (operands["dP0"][int(k[2:])] if acc else 0)
            scale = float(np.abs(want).max())
            bar = 2e-5 if k == "dw1" else 1e-4
            es = _err(t, want)
            line = f"{which} acc {acc} {k}: compact err {es:.3e}, bar {bar * scale:.3e}"
            if not acc:
                ed = _err(dense[k], want)
                line += f", dense err {ed:.3e}"
            print(line)
            assert es <= bar * scale + 1e-12, line
            if not acc:
                assert es <= ed, line
        # a voxel without an active row among its 27 neighbours: exactly zero, or unchanged under accumulate
        for l, (H, W, D) in enumerate(LEVELS):
            a = np.zeros((H + 2, W + 2, D + 2), bool)
            a[1:-1, 1:-1, 1:-1] = (slot[ROW0[l]:ROW0[l + 1]] >= 0).reshape(H, W, D)
            near = np.zeros((H, W, D), bool)
            for dy in range(3):
                for dx in range(3):
                    for dz in range(3):
                        near |= a[dy:dy + H, dx:dx + W, dz:dz + D]
            far = torch.from_numpy(~near).to(g["dP"][l].device)
            want = dev.dP0[l][far] if acc else torch.zeros_like(g["dP"][l][far])
            assert torch.equal(g["dP"][l][far], want), (which, acc, l)
        if which == "none":
            assert not any(t.any() for k, t in got.items() if not k.startswith("dP"))


def test_overflow_is_loud(dev, operands, cuda):
    """n = 257 > cap: the sticky word counts it, check_compact raises, the compact gradient is NaN"""
    from m3d.backbone import RPNHead
    dl, db = _gradient("n257")
    g, ws = dev.run(dl, db, 0)
    hn, hc, over, _, _, _ = dev.header(ws)
    assert (hn, hc, over) == (257, CAP, 1)
    dz3c = ws[dev.L.m3d_conv3d_rowsparse_scan_bytes(R) // 4:][:CAP * NPAD]
    assert not torch.isfinite(dz3c).any()
    assert not torch.isfinite(g["dw24"]).all() and not torch.isfinite(g["dw1"]).all()
    assert not all(torch.isfinite(a).all() for a in g["dP"])
    g, ws = dev.run(dl, db, 0, ws)                       # sticky: a second pass counts on
    assert dev.header(ws)[2] == 2
    g, ws = dev.run(*_gradient("row0"), 0, ws)           # ... and a good pass does not clear it
    assert dev.header(ws)[:3] == (1, 1, 2)
    head = RPNHead.__new__(RPNHead)
    head._compact_ws = {(R, CAP, cuda): (ws, dev.wsb)}
    with pytest.raises(RuntimeError, match="more active voxel rows"):
        head.check_compact()
    head.check_compact()                                 # cleared by the raise


def test_deterministic_runs_are_bit_equal(dev):
    dev.lib.set_deterministic(True, scratch_bytes=64 << 20)
    dl, db = _gradient("n256")
    a, _ = dev.run(dl, db, 0)
    b, _ = dev.run(dl, db, 0)
    for (k, x), y in zip(_flat(a).items(), _flat(b).values()):
        assert torch.equal(x, y), k


def test_graph_replay_follows_the_data(dev, cuda):
    """captured once, replayed with two active sets: each replay bit-equal to that set's eager run"""
    dev.lib.set_deterministic(True, scratch_bytes=64 << 20)
    sets = ("level1_empty", "n256", "none")
    eager = {k: _flat(dev.run(*_gradient(k), 0)[0]) for k in sets}
    dl, db = (torch.from_numpy(a).to(cuda) for a in _gradient(sets[0]))
    ws = torch.zeros(dev.wsb // 4 + 1, device=cuda)
    g = dev.buffers(0)
    a = dev.block(dl, db, g, ws, 0)
    dev.launch(a)                                        # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dev.launch(a)
    for k in sets[1:] + sets[:1]:
        nl, nb = _gradient(k)
        dl.copy_(torch.from_numpy(nl))
        db.copy_(torch.from_numpy(nb))
        for key in ("dw1", "db1", "dw2", "db2", "dw24", "db24"):
            g[key].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert dev.header(ws)[0] == len(_active(k)[0])
        for name, t in _flat(g).items():
            assert torch.equal(t, eager[k][name]), (k, name)


# --------------------------------------------------------------------------- model
N_TARGETS = 256


def _rpn(cuda, monkeypatch, compact, steps=0, min_rows=0, graphed=False, spy=None):
    """tests/test_gpu_rowsparse.py::_rpn's 64 x 64 x 16 model with 256 sampled anchors"""
    from m3d import nn as mnn
    from m3d.config import synthetic_rpn_config
    from m3d.model import RPN, RPNTargets, synthetic_rpn_targets, synthetic_volume
    monkeypatch.setattr(mnn, "RPN_HEAD_COMPACT", compact)
    if min_rows is not None:
        monkeypatch.setattr(mnn, "RPN_HEAD_COMPACT_MIN_ROWS", min_rows)
    if spy is not None:
        orig = mnn._RPNHeadCompact.apply
        monkeypatch.setattr(mnn._RPNHeadCompact, "apply", lambda *a: (spy.append(a[1]), orig(*a))[1])
    cfg = synthetic_rpn_config(64, depth=16, PRE_NMS_LIMIT=2000, POST_NMS_ROIS_TRAINING=200)
    image = synthetic_volume(64, 16, seed=3).to(cuda)
    model = RPN(cfg, device=cuda, seed=7)
    match, bbox = synthetic_rpn_targets(model.anchors.shape[1], N_TARGETS, seed=2)
    targets = RPNTargets(match, bbox, cuda)
    if graphed:
        step = model.graphed_train_step(image, targets, proposals=False, warmup=1)
        step()
        torch.cuda.synchronize()
        model.rpn.check_compact()
        return [p.data.clone() for p in model.store.params]
    if steps:
        for _ in range(steps):
            model.train_step(image, targets, proposals=False)
        torch.cuda.synchronize()
        model.rpn.check_compact()
        return [p.data.clone() for p in model.store.params]
    r = model.forward_backward(image, targets, proposals=False)
    torch.cuda.synchronize()
    model.rpn.check_compact()
    return r["loss"].clone(), {p.name: p.grad.clone() for p in model.store.params}


def test_model_step_compact_vs_off(cuda, monkeypatch):
    """the same loss bit for bit; every parameter gradient within 1e-4 of the tensor's largest
    magnitude (the bar of test_gpu_rowsparse.py::test_model_step_sparse_vs_off)"""
    from m3d import _lib as lib
    lib.set_deterministic(True)
    took = []
    with monkeypatch.context() as mp:
        l2, g2 = _rpn(cuda, mp, True, spy=took)
    assert took == [256]                                         # the route ran, cap = the bound rounded up
    with monkeypatch.context() as mp:
        l1, g1 = _rpn(cuda, mp, False, spy=took)
    assert took == [256]
    assert torch.equal(l2, l1)
    worst = 0.0
    for k, a in g1.items():
        scale = float(a.abs().max())
        err = float((g2[k] - a).abs().max())
        worst = max(worst, err / (scale + 1e-30))
        assert err <= 1e-4 * scale + 1e-30, (k, err, scale)
    print("largest gradient difference / scale over the parameters: %.3e" % worst)


def test_model_steps_deterministic(cuda, monkeypatch):
    from m3d import _lib as lib
    lib.set_deterministic(True)
    a = _rpn(cuda, monkeypatch, True, steps=4)
    b = _rpn(cuda, monkeypatch, True, steps=4)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_graphed_step_equals_eager(cuda, monkeypatch):
    """warm-up step + captured step replayed once == two eager steps"""
    from m3d import _lib as lib
    lib.set_deterministic(True)
    took = []
    a = _rpn(cuda, monkeypatch, True, graphed=True, spy=took)
    assert took and set(took) == {256}
    b = _rpn(cuda, monkeypatch, True, steps=2)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_default_threshold_keeps_todays_route(cuda, monkeypatch):
    """5456 rows are below RPN_HEAD_COMPACT_MIN_ROWS: the same configuration stays on the per-unit path"""
    took = []
    _rpn(cuda, monkeypatch, True, min_rows=None, spy=took)
    assert took == []
