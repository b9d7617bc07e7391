#!/usr/bin/env python
"""Per-call time of the Winograd backward with the row-sparse attempt off (rs_mode 1), as the library
decides (0) and forced (2), on dense and sparse dz at the 128^3 step's shapes: the measurement behind
RS_MIN_FLOP (csrc/conv_rowsparse.hip) and DESIGN.md 5, kept as profiles/rowsparse_overhead.txt.  HIP-event time
of 20 back-to-back calls after 5 warm-ups, median (min, max) of 5 such batches.  state: what the data
gradient's scan decided, [state (1 dense, 2 sparse), skip_dense, skip_sparse, n]; "-": no scan ran.

  python scripts/rowsparse_overhead.py > profiles/rowsparse_overhead.txt"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "3d-mask-r-cnn_amd")):
    sys.path.insert(0, p)
import numpy as np
import torch
from m3d import _lib as lib
L = lib.load()
dev = torch.device("cuda:0")


def timeit(fn, reps=20, batches=5):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(batches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps * 1e3)
    return float(np.median(out)), float(min(out)), float(max(out))


def case(name, H, W, D, cin, cout, nact):
    B = 1
    g = torch.Generator().manual_seed(1)
    x = torch.randn((B, H, W, D, cin), generator=g).to(dev)
    w = (torch.randn((3, 3, 3, cin, cout), generator=g) * 0.02).to(dev)
    rows = H * W * D
    if nact is None:
        dz = torch.randn((B, H, W, D, cout), generator=g).to(dev)
    else:
        dz = torch.zeros((rows, cout))
        pick = torch.randperm(rows, generator=g)[:nact]
        dz[pick] = torch.randn((nact, cout), generator=g)
        dz = dz.reshape(B, H, W, D, cout).to(dev)
    nb = int(L.m3d_conv3d_wino_workspace_bytes(B, H, W, D, D, cin, cout))
    ws = torch.zeros(nb // 4 + 1, device=dev)
    ws2 = torch.empty(nb // 4 + 1, device=dev)
    dx = torch.empty_like(x)
    dw = torch.zeros_like(w)
    ub = int(L.m3d_conv3d_wino_u_bytes(B, H, W, D, cin))
    u = torch.empty(ub // 4, device=dev)
    y = torch.empty((B, H, W, D, cout), device=dev)
    lib.check(L.m3d_conv3d_fwd_wino_keep(x.data_ptr(), B, H, W, D, cin, w.data_ptr(), cout, D, 1, None, None, None, None,
                                         0, None, y.data_ptr(), u.data_ptr(), ws.data_ptr(), nb, lib.stream()))
    del y
    st = lib.stream()
    off = int(L.m3d_conv3d_rowsparse_header_offset(B, H, W, D, D, 1, cin, cout, 0, 0))
    for mode in (1, 0, 2):
        ws[off // 4: off // 4 + 4] = 0
        # v_ready = 1 after the first call: the weight transform is shared by the levels in the step
        lib.check(L.m3d_conv3d_bwd_data_wino_rs(dz.data_ptr(), w.data_ptr(), B, H, W, D, cin, cout, D, 1, dx.data_ptr(), 0,
                                                ws.data_ptr(), nb, 0, 0, None, mode, st))
        td = timeit(lambda: lib.check(L.m3d_conv3d_bwd_data_wino_rs(
            dz.data_ptr(), w.data_ptr(), B, H, W, D, cin, cout, D, 1, dx.data_ptr(), 0, ws.data_ptr(), nb, 1, 0, None,
            mode, st)))
        tw = timeit(lambda: lib.check(L.m3d_conv3d_bwd_weight_wino_ux(
            u.data_ptr(), x.data_ptr(), dz.data_ptr(), B, H, W, D, cin, cout, D, 1, dw.data_ptr(), ws2.data_ptr(), nb,
            mode, st)))
        state = ws[off // 4: off // 4 + 4].view(torch.int32).cpu().tolist()
        state = state if state[0] else "-"
        print(f"{name:28s} rs_mode {mode} state {str(state):18s}: dgrad {td[0]:8.1f} us (min {td[1]:.1f} max {td[2]:.1f})   "
              f"wgrad {tw[0]:8.1f} us (min {tw[1]:.1f} max {tw[2]:.1f})", flush=True)


case("fpn_p2 dense 256->256", 32, 32, 128, 256, 256, None)
case("rpn_shared1 P2 dense", 32, 32, 128, 256, 512, None)
case("rpn_shared1 P2 1150 rows", 32, 32, 128, 256, 512, 1150)
case("rpn_shared1 P3 dense", 16, 16, 128, 256, 512, None)
case("rpn_shared1 P3 290 rows", 16, 16, 128, 256, 512, 290)
case("rpn_shared1 P4 72 rows", 8, 8, 128, 256, 512, 72)
