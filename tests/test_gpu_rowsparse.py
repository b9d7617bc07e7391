"""The row-sparse path of the Winograd backward entry points (csrc/conv3d.hip, csrc/conv_rowsparse.hip,
"row-sparse output gradients"): the device-side scan of dz, the sparse data and
weight gradients against the float64 references of tests/convref.py, the
fallbacks, graph replay and the RPN step.

Bars: the ones tests/test_gpu_conv.py sets for the same entry points, max
|got - ref| against the reference's largest magnitude: 1e-4 of it for the data
gradient (test_winograd_z_halo_geometry), 2e-5 for the weight gradient
(test_wino_weight_gradient_accuracy); and the sparse result's error may not
exceed the dense path's own error on the same inputs.  Shapes: an 8 x 8 x 16 volume (1024 rows,
cap = min(4096, rows / 32) = 32) reached through rs_mode 2 of
m3d_conv3d_bwd_data_wino_rs / m3d_conv3d_bwd_weight_wino_ux (1: the path off)."""
import numpy as np
import pytest
import torch

import convref as R

pytestmark = pytest.mark.gpu

H, W, D = 8, 8, 16
SP = (H, W, D)
PAD = (1, 1, 1)
DENSE, SPARSE = 1, 2
HDR_INTS, CAP_MAX = 64, 4096


@pytest.fixture(autouse=True)
def _mode_reset():
    from m3d import _lib
    yield
    _lib.set_deterministic(False)


def _err(got, ref):
    return float(np.abs(got.double().cpu().numpy() - ref).max())


def _rows(B, which):
    """active dz rows (flat [B, H, W, D] indices) of a named case"""
    rows = B * H * W * D
    cap = rows // 32
    flat = lambda b, y, x, z: ((b * H + y) * W + x) * D + z   # noqa: E731
    rng = np.random.default_rng(len(which) + B)
    if which == "none":
        return []
    if which == "corners_faces":
        c = [flat(B - 1, y, x, z) for y in (0, H - 1) for x in (0, W - 1) for z in (0, D - 1)]
        return c + [flat(0, 0, 3, 5), flat(0, H - 1, 4, 9), flat(0, 2, 0, 7), flat(0, 5, W - 1, 8), flat(0, 3, 3, 0),
                    flat(0, 4, 4, D - 1)]
    if which == "adjacent":
        return [flat(0, 3, 4, 6), flat(0, 3, 4, 7), flat(B - 1, 4, 4, 7)]
    if which == "first_last":
        return [0, rows - 1]
    if which == "at_cap":
        return sorted(rng.choice(rows, cap, replace=False).tolist())
    if which == "over_cap":
        return sorted(rng.choice(rows, cap + 1, replace=False).tolist())
    if which == "dense":
        return list(range(rows))
    raise KeyError(which)


def _dz(B, cout, which, seed=0):
    rng = np.random.default_rng(seed)
    dz = np.zeros((B * H * W * D, cout), np.float32)
    r = _rows(B, which)
    dz[r] = rng.normal(size=(len(r), cout)).astype(np.float32)
    return dz.reshape(B, H, W, D, cout)


def _operands(B, cin, cout):
    rng = np.random.default_rng(5)
    x = rng.normal(size=(B, H, W, D, cin)).astype(np.float32)
    w = rng.normal(0, 1.0 / np.sqrt(27 * cout), (3, 3, 3, cin, cout)).astype(np.float32)
    return x, w


def _state(L, ws, B, cin, cout, pas):
    off = int(L.m3d_conv3d_rowsparse_header_offset(B, H, W, D, D, 1, cin, cout, pas, 0))
    assert off % 4 == 0 and off < ws.numel() * 4
    h = ws[off // 4: off // 4 + 4].view(torch.int32).cpu().tolist()
    return h[0], h[3]


def _dgrad(L, lib, mode, dz, w, dx0, acc, cuda):
    B, cin, cout = dz.shape[0], w.shape[3], w.shape[4]
    nb = int(L.m3d_conv3d_wino_workspace_bytes(B, H, W, D, D, cin, cout))
    ws = torch.zeros(nb // 4 + 1, device=cuda)
    dx = dx0.clone() if acc else torch.full_like(dx0, 7.0)
    lib.check(L.m3d_conv3d_bwd_data_wino_rs(dz.data_ptr(), w.data_ptr(), B, H, W, D, cin, cout, D, 1, dx.data_ptr(),
                                            acc, ws.data_ptr(), nb, 0, 0, None, mode, lib.stream()), "bwd_data_wino_rs")
    torch.cuda.synchronize()
    return dx, _state(L, ws, B, cin, cout, 0)


def _wgrad(L, lib, mode, form, x, w, dz, dw0, cuda):
    B, cin, cout = dz.shape[0], x.shape[4], dz.shape[4]
    nb = int(L.m3d_conv3d_wino_workspace_bytes(B, H, W, D, D, cin, cout))
    ws = torch.zeros(nb // 4 + 1, device=cuda)
    dw = dw0.clone()
    u = None
    if form == "ux":
        ub = int(L.m3d_conv3d_wino_u_bytes(B, H, W, D, cin))
        assert ub > 0
        u = torch.empty(ub // 4, device=cuda)
        y = torch.empty((B, H, W, D, cout), device=cuda)
        lib.check(L.m3d_conv3d_fwd_wino_keep(x.data_ptr(), B, H, W, D, cin, w.data_ptr(), cout, D, 1, None, None, None,
                                             None, 0, None, y.data_ptr(), u.data_ptr(), ws.data_ptr(), nb,
                                             lib.stream()), "fwd_wino_keep")
    lib.check(L.m3d_conv3d_bwd_weight_wino_ux(lib.ptr(u), x.data_ptr(), dz.data_ptr(), B, H, W, D, cin, cout, D, 1,
                                              dw.data_ptr(), ws.data_ptr(), nb, mode, lib.stream()), "wgrad ux")
    torch.cuda.synchronize()
    return dw, _state(L, ws, B, cin, cout, 1)


# --------------------------------------------------------------------------- 1. scan
def _scan(L, lib, dz, cap, cuda):
    rows, C = dz.shape
    nb = int(L.m3d_conv3d_rowsparse_scan_bytes(rows))
    ws = torch.zeros(nb // 4, device=cuda, dtype=torch.int32)
    d = torch.from_numpy(dz).to(cuda)
    lib.check(L.m3d_conv3d_rowsparse_scan(d.data_ptr(), rows, C, cap, ws.data_ptr(), nb, lib.stream()), "scan")
    torch.cuda.synchronize()
    h = ws.cpu().numpy()
    al = lambda n: (n + 63) // 64 * 64      # noqa: E731  (256 bytes, in ints)
    o_slot = al(HDR_INTS + CAP_MAX) + al((rows + 63) // 64)
    return h[:4], h[HDR_INTS:HDR_INTS + CAP_MAX], h[o_slot:o_slot + rows]


def test_scan(cuda):
    from m3d import _lib as lib
    L = lib.load()
    rows, C = 1000, 96                       # a ragged last block of 40 rows
    dz = np.zeros((rows, C), np.float32)
    dz[0, 3] = 1.0                           # first row
    dz[17, C - 1] = -2.0                     # only the last channel
    dz[18] = -0.0                            # all negative zeros: inactive
    dz[63, 0] = np.nan                       # a NaN row is active
    dz[999, 1] = 3.0                         # last row
    dz[64, 5] = 1.0                          # first row of the second block
    want = [0, 17, 63, 64, 999]
    h, idx, slot = _scan(L, lib, dz, 31, cuda)
    assert h.tolist() == [SPARSE, 1, 0, len(want)]
    assert idx[:len(want)].tolist() == want                     # ascending
    exp = np.full(rows, -1)
    exp[want] = np.arange(len(want))
    assert np.array_equal(slot, exp)                            # consistent with the index list
    # no active row at all
    h, _, slot = _scan(L, lib, np.zeros((rows, C), np.float32), 31, cuda)
    assert h.tolist() == [SPARSE, 1, 0, 0] and (slot == -1).all()
    # exactly cap active rows is sparse, one more is dense; so is a dense tensor (by the probe)
    rng = np.random.default_rng(1)
    for n, state in ((31, SPARSE), (32, DENSE)):
        dz = np.zeros((rows, C), np.float32)
        pick = np.sort(rng.choice(rows, n, replace=False))
        dz[pick, rng.integers(0, C, n)] = 1.0
        h, idx, _ = _scan(L, lib, dz, 31, cuda)
        assert h[0] == state and h[1] == (state == SPARSE) and h[2] == (state == DENSE)
        if state == SPARSE:
            assert h[3] == n and np.array_equal(idx[:n], pick)
    h, _, _ = _scan(L, lib, rng.normal(size=(rows, C)).astype(np.float32), 31, cuda)
    assert h[:3].tolist() == [DENSE, 0, 1]


# --------------------------------------------------------------------------- 2. data gradient
@pytest.mark.parametrize("B,cin,cout,which,acc", [
    (1, 64, 128, "none", 0), (1, 64, 128, "none", 1), (1, 64, 128, "corners_faces", 0),
    (1, 64, 128, "adjacent", 0), (1, 64, 128, "adjacent", 1), (1, 64, 128, "at_cap", 0),
    (2, 128, 64, "corners_faces", 1), (1, 128, 256, "first_last", 0)])
def test_dgrad_sparse(cuda, B, cin, cout, which, acc):
    from m3d import _lib as lib
    L = lib.load()
    _, w = _operands(B, cin, cout)
    dz = _dz(B, cout, which)
    dx0 = np.random.default_rng(3).normal(0, 0.5, (B, H, W, D, cin)).astype(np.float32)
    ref = R.conv_bwd_data(dz, w, dx0.shape, R.K3, R.S1, PAD, SP) + (dx0 if acc else 0.0)
    t = lambda a: torch.from_numpy(a).to(cuda)      # noqa: E731
    got, (state, n) = _dgrad(L, lib, 2, t(dz), t(w), t(dx0), acc, cuda)
    dense, _ = _dgrad(L, lib, 1, t(dz), t(w), t(dx0), acc, cuda)
    assert (state, n) == (SPARSE, len(_rows(B, which)))
    es, ed, scale = _err(got, ref), _err(dense, ref), float(np.abs(ref).max())
    print(f"dgrad {which} acc {acc}: sparse err {es:.3e}, dense err {ed:.3e}, 1e-4 of scale {1e-4 * scale:.3e}")
    assert es <= 1e-4 * scale + 1e-12
    assert es <= ed
    if which == "none":
        assert torch.equal(got, t(dx0) if acc else torch.zeros_like(got))


@pytest.mark.parametrize("which", ["over_cap", "dense"])
def test_dgrad_fallback_is_the_dense_path(cuda, which):
    from m3d import _lib as lib
    L = lib.load()
    _, w = _operands(1, 64, 128)
    t = lambda a: torch.from_numpy(a).to(cuda)      # noqa: E731
    dz, dx0 = t(_dz(1, 128, which)), torch.zeros((1, H, W, D, 64), device=cuda)
    got, (state, _) = _dgrad(L, lib, 2, dz, t(w), dx0, 0, cuda)
    off, _ = _dgrad(L, lib, 1, dz, t(w), dx0, 0, cuda)
    assert state == DENSE
    assert torch.equal(got, off)


@pytest.fixture
def big_volume(monkeypatch):
    """16 x 32 x 32: 16384 rows, cap 512 -- the smallest at which the sparse GEMMs take the 256-row tiles
    the step runs (x3_gemm256_af_kernel from 256 compact rows, stream-K x3_wgrad_tr_kernel from 512)"""
    import sys
    me = sys.modules[__name__]
    for k, v in (("H", 16), ("W", 32), ("D", 32), ("SP", (16, 32, 32))):
        monkeypatch.setattr(me, k, v)


def test_dgrad_sparse_256_row_tiles(cuda, big_volume):
    """Cin 256: N = 27 * 256 fills whole 256-column tiles; 300 active rows leave the second row tile
    ragged and make the third and fourth (rows 512.. of the padded cap) exit on the device-side count"""
    from m3d import _lib as lib
    L = lib.load()
    B, cin, cout = 1, 256, 32
    _, w = _operands(B, cin, cout)
    rng = np.random.default_rng(9)
    pick = np.sort(rng.choice(H * W * D, 300, replace=False))
    dz = np.zeros((H * W * D, cout), np.float32)
    dz[pick] = rng.normal(size=(300, cout)).astype(np.float32)
    dz = dz.reshape(B, H, W, D, cout)
    ref = R.conv_bwd_data(dz, w, (B, H, W, D, cin), R.K3, R.S1, PAD, SP)
    t = lambda a: torch.from_numpy(a).to(cuda)      # noqa: E731
    dx0 = torch.zeros((B, H, W, D, cin), device=cuda)
    got, (state, n) = _dgrad(L, lib, 2, t(dz), t(w), dx0, 0, cuda)
    dense, _ = _dgrad(L, lib, 1, t(dz), t(w), dx0, 0, cuda)
    assert (state, n) == (SPARSE, 300)
    es, ed, scale = _err(got, ref), _err(dense, ref), float(np.abs(ref).max())
    print(f"dgrad 256-row tiles: sparse err {es:.3e}, dense err {ed:.3e}, 1e-4 of scale {1e-4 * scale:.3e}")
    assert es <= 1e-4 * scale and es <= ed


def test_wgrad_sparse_stream_k(cuda, big_volume):
    """Cin = Cout = 192, cap 512: the atomic mode's stream-K x3_wgrad_tr_kernel behind the gate"""
    from m3d import _lib as lib
    L = lib.load()
    B, cin, cout = 1, 192, 192
    x, w = _operands(B, cin, cout)
    rng = np.random.default_rng(9)
    pick = np.sort(rng.choice(H * W * D, 300, replace=False))
    dz = np.zeros((H * W * D, cout), np.float32)
    dz[pick] = rng.normal(size=(300, cout)).astype(np.float32)
    dz = dz.reshape(B, H, W, D, cout)
    dw0 = rng.normal(0, 0.5, w.shape).astype(np.float32)
    ref = R.conv_bwd_weight(x, dz, R.K3, R.S1, PAD, SP, dw0)
    t = lambda a: torch.from_numpy(a).to(cuda)      # noqa: E731
    got, (state, n) = _wgrad(L, lib, 2, "plain", t(x), t(w), t(dz), t(dw0), cuda)
    dense, _ = _wgrad(L, lib, 1, "plain", t(x), t(w), t(dz), t(dw0), cuda)
    assert (state, n) == (SPARSE, 300)
    es, ed, scale = _err(got, ref), _err(dense, ref), float(np.abs(ref).max())
    print(f"wgrad stream-K: sparse err {es:.3e}, dense err {ed:.3e}, 2e-5 of scale {2e-5 * scale:.3e}")
    assert es <= 2e-5 * scale and es <= ed


# --------------------------------------------------------------------------- 3. weight gradient
@pytest.mark.parametrize("form", ["plain", "ux"])
@pytest.mark.parametrize("B,cin,cout,which", [
    (1, 64, 128, "none"), (1, 64, 128, "corners_faces"), (1, 64, 128, "adjacent"), (1, 64, 128, "at_cap"),
    (2, 128, 128, "corners_faces"), (1, 256, 256, "first_last")])
def test_wgrad_sparse(cuda, form, B, cin, cout, which):
    """(256, 256: x3_wgrad_tr_kernel; 64 / 128 channels: x3_wgrad64_kernel / x3_wgrad_kernel); always
    accumulating onto a non-zero dw, as the step does over levels"""
    from m3d import _lib as lib
    L = lib.load()
    x, w = _operands(B, cin, cout)
    dz = _dz(B, cout, which)
    dw0 = np.random.default_rng(4).normal(0, 0.5, w.shape).astype(np.float32)
    ref = R.conv_bwd_weight(x, dz, R.K3, R.S1, PAD, SP, dw0)
    t = lambda a: torch.from_numpy(a).to(cuda)      # noqa: E731
    got, (state, n) = _wgrad(L, lib, 2, form, t(x), t(w), t(dz), t(dw0), cuda)
    dense, _ = _wgrad(L, lib, 1, form, t(x), t(w), t(dz), t(dw0), cuda)
    assert (state, n) == (SPARSE, len(_rows(B, which)))
    es, ed, scale = _err(got, ref), _err(dense, ref), float(np.abs(ref).max())
    print(f"wgrad {form} {which}: sparse err {es:.3e}, dense err {ed:.3e}, 2e-5 of scale {2e-5 * scale:.3e}")
    assert es <= 2e-5 * scale
    assert es <= ed
    if which == "none":
        assert torch.equal(got, t(dw0))


@pytest.mark.parametrize("form", ["plain", "ux"])
def test_wgrad_fallback_and_determinism(cuda, form):
    from m3d import _lib as lib
    L = lib.load()
    x, w = _operands(1, 64, 128)
    t = lambda a: torch.from_numpy(a).to(cuda)      # noqa: E731
    dw0 = torch.zeros((3, 3, 3, 64, 128), device=cuda)
    lib.set_deterministic(True, scratch_bytes=16 << 20)
    for which in ("over_cap", "dense"):
        got, (state, _) = _wgrad(L, lib, 2, form, t(x), t(w), t(_dz(1, 128, which)), dw0, cuda)
        off, _ = _wgrad(L, lib, 1, form, t(x), t(w), t(_dz(1, 128, which)), dw0, cuda)
        assert state == DENSE
        assert torch.equal(got, off)
    runs = [_wgrad(L, lib, 2, form, t(x), t(w), t(_dz(1, 128, "at_cap")), dw0, cuda) for _ in range(3)]
    assert all(r[1][0] == SPARSE for r in runs)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][0], runs[2][0])


# --------------------------------------------------------------------------- 4. graph replay
def test_graph_replay_decides_on_the_device(cuda):
    from m3d import _lib as lib
    L = lib.load()
    B, cin, cout = 1, 64, 128
    x, w = _operands(B, cin, cout)
    t = lambda a: torch.from_numpy(a).to(cuda)      # noqa: E731
    xd, wd = t(x), t(w)
    contents = {"sparse": t(_dz(B, cout, "corners_faces")), "dense": t(_dz(B, cout, "dense")),
                "sparse2": t(_dz(B, cout, "adjacent"))}
    zero_dx, zero_dw = torch.zeros((B, H, W, D, cin), device=cuda), torch.zeros(w.shape, device=cuda)
    lib.set_deterministic(True, scratch_bytes=16 << 20)
    eager = {k: (_dgrad(L, lib, 2, v, wd, zero_dx, 0, cuda)[0], _wgrad(L, lib, 2, "plain", xd, wd, v, zero_dw, cuda)[0])
             for k, v in contents.items()}
    nb = int(L.m3d_conv3d_wino_workspace_bytes(B, H, W, D, D, cin, cout))
    ws1, ws2 = torch.zeros(nb // 4 + 1, device=cuda), torch.zeros(nb // 4 + 1, device=cuda)
    dz = contents["sparse"].clone()
    dx, dw = torch.empty_like(zero_dx), torch.zeros_like(zero_dw)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lib.check(L.m3d_conv3d_bwd_data_wino_rs(dz.data_ptr(), wd.data_ptr(), B, H, W, D, cin, cout, D, 1,
                                                dx.data_ptr(), 0, ws1.data_ptr(), nb, 0, 0, None, 2, lib.stream()),
                  "bwd_data_wino_rs")
        lib.check(L.m3d_conv3d_bwd_weight_wino_ux(None, xd.data_ptr(), dz.data_ptr(), B, H, W, D, cin, cout, D, 1,
                                                  dw.data_ptr(), ws2.data_ptr(), nb, 2, lib.stream()), "wgrad ux")
    for k, want_state in (("sparse", SPARSE), ("dense", DENSE), ("sparse2", SPARSE)):
        dz.copy_(contents[k])
        dw.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _state(L, ws1, B, cin, cout, 0)[0] == want_state and _state(L, ws2, B, cin, cout, 1)[0] == want_state
        assert torch.equal(dx, eager[k][0]), k
        assert torch.equal(dw, eager[k][1]), k


# --------------------------------------------------------------------------- 5. model
N_TARGETS = 64      # sampled anchors: about 45 rows of P2's 4096 (cap 128), 12 of P3's 1024 (cap 32), under both caps


def _rpn(cuda, mode, steps, monkeypatch, states=None):
    """The RPN of tests/test_gpu_launch_plan.py's 64 x 64 x 16 config with N_TARGETS sampled anchors.
    states: a list that receives (pass, H, Cin, Cout, state, n) of every call of the two rs_mode entry
    points, read from the call's header right after it (this run then synchronises after those calls)."""
    from m3d import _lib as lib
    from m3d import nn as mnn
    from m3d.config import synthetic_rpn_config
    from m3d.model import RPN, RPNTargets, synthetic_rpn_targets, synthetic_volume
    monkeypatch.setattr(mnn, "ROWSPARSE", mode)
    if states is not None:
        L = lib.load()
        held = {}                       # data_ptr -> workspace tensor, kept alive so nothing reuses it

        def keep(fn, pick):
            def f(*a, **k):
                r = fn(*a, **k)
                held[pick(r).data_ptr()] = pick(r)
                return r
            return f
        monkeypatch.setattr(mnn, "_wino_ws", keep(mnn._wino_ws, lambda r: r[0]))
        monkeypatch.setattr(mnn, "_shared_wino_ws", keep(mnn._shared_wino_ws, lambda r: r[0]))

        def spy(name, pas):
            orig = getattr(L, name)

            def f(*a):
                rc = orig(*a)
                torch.cuda.synchronize()
                if pas == 0:
                    B, Hh, Ww, Dd, cin, cout, OD, pz, ws, ty = *a[2:10], a[12], a[15]
                else:
                    B, Hh, Ww, Dd, cin, cout, OD, pz, ws, ty = *a[3:11], a[12], 0
                off = int(L.m3d_conv3d_rowsparse_header_offset(B, Hh, Ww, Dd, OD, pz, cin, cout, pas, ty))
                h = held[ws][off // 4: off // 4 + 4].view(torch.int32).cpu().tolist()
                states.append((pas, Hh, cin, cout, h[0], h[3]))
                return rc
            monkeypatch.setattr(L, name, f)
        spy("m3d_conv3d_bwd_data_wino_rs", 0)
        spy("m3d_conv3d_bwd_weight_wino_ux", 1)
    cfg = synthetic_rpn_config(64, depth=16, PRE_NMS_LIMIT=2000, POST_NMS_ROIS_TRAINING=200)
    image = synthetic_volume(64, 16, seed=3).to(cuda)
    model = RPN(cfg, device=cuda, seed=7)
    match, bbox = synthetic_rpn_targets(model.anchors.shape[1], N_TARGETS, seed=2)
    targets = RPNTargets(match, bbox, cuda)
    if steps:
        for _ in range(steps):
            model.train_step(image, targets, proposals=False)
        torch.cuda.synchronize()
        return [p.data.clone() for p in model.store.params]
    r = model.forward_backward(image, targets, proposals=False)
    torch.cuda.synchronize()
    return r["loss"].clone(), {p.name: p.grad.clone() for p in model.store.params}


def test_model_step_sparse_vs_off(cuda, monkeypatch):
    """One RPN forward_backward in rs_mode 2 and with the path off: the same loss;
    rpn_conv_shared1's own gradients and every gradient downstream of the one
    entering the FPN (all FPN and backbone parameters) within the conv bar, 1e-4
    of each tensor's largest magnitude.  rpn_conv_shared1 (256 -> 512) must have
    run SPARSE on P2 (16 x 16 x 16) and P3 (8 x 8 x 16) in both passes -- through
    nn.py's calls: the kept U beside x, the shared workspace with the header at
    each level's own offset, the side stream."""
    from m3d import _lib as lib
    lib.set_deterministic(True)
    states = []
    with monkeypatch.context() as mp:
        l2, g2 = _rpn(cuda, 2, 0, mp, states)
    for s in states:
        print("pass %d H %d %d->%d state %d n %d" % s)
    for pas in (0, 1):
        for Hh in (16, 8):
            got = [(s[4], s[5]) for s in states if s[:4] == (pas, Hh, 256, 512)]
            assert got and all(st == SPARSE and n > 0 for st, n in got), (pas, Hh, got, states)
    l1, g1 = _rpn(cuda, 1, 0, monkeypatch)
    assert torch.equal(l2, l1)
    assert any("rpn_conv_shared1" in k for k in g1)
    worst = 0.0
    for k, a in g1.items():
        scale = float(a.abs().max())
        err = float((g2[k] - a).abs().max())
        worst = max(worst, err / (scale + 1e-30))
        assert err <= 1e-4 * scale + 1e-30, (k, err, scale)
    print("largest gradient difference / scale over the parameters: %.3e" % worst)


def test_model_steps_deterministic(cuda, monkeypatch):
    """four deterministic steps in rs_mode 2 (sparse on P2 / P3, see above), run twice: the same weights"""
    from m3d import _lib as lib
    lib.set_deterministic(True)
    a = _rpn(cuda, 2, 4, monkeypatch)
    b = _rpn(cuda, 2, 4, monkeypatch)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
