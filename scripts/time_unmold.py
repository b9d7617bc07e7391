"""Time of detection unmolding + mask overlaps (csrc/unmold.hip) at the
configs[3] shape: a 256^3 volume, DETECTION_MAX_INSTANCES detections with boxes
of 32-64 voxels per side, MASK_SHAPE 28^3, G = 50 ground-truth masks
([H,W,D,G] uint8).

Forms, alternating in one process, HIP events, median of --runs after --warmup:
  (i)   m3d_unmold_prepare + m3d_unmold_overlaps + m3d_mask_areas +
        m3d_unmold_finalize (IoU included)
  (ii)  m3d_unmold_overlaps alone
  (a)   the same counts in framework ops on the same GPU, starting from the
        kernels' own thresholded 28^3 grids (so without the statistics, the
        threshold and the cleaning): per detection F.interpolate (trilinear)
        into its box of an [N,H,W,D] float32 tensor, the GT masks cast to
        float32, one [N,V] x [V,G] matmul, column sums, the IoU expression
  (copy) a uint8 device copy of as many bytes as the overlaps kernel's
        algorithmic traffic, for its achievable rate in this run
  (b)   tests/unmoldref.py (numpy) on this host's CPU at 64^3 with the boxes
        scaled by 1/4, multiplied by 64 (the voxel ratio): an extrapolation,
        labelled as such

    python scripts/time_unmold.py [--size 256] [--gt 50] [--runs 30] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "3d-mask-r-cnn_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def workload(S, N, m, C, G, seed=0):
    """detections [N,8], mrcnn_mask [N,m,m,m,C] (a noisy ball per detection), GT boxes [G,6]."""
    rng = np.random.default_rng(seed)
    lo_side, hi_side = S // 8, S // 4                            # 32-64 voxels at 256
    det = np.zeros((N, 8), np.float32)
    g = np.indices((m, m, m)).astype(np.float32)
    mask = rng.uniform(0.0, 0.08, (N, m, m, m, C)).astype(np.float32)
    for i in range(N):
        side = rng.integers(lo_side, hi_side + 1, 3)
        lo = np.array([rng.integers(0, S - s + 1) for s in side])
        det[i, :6] = np.concatenate([lo, lo + side]) / S
        det[i, 6], det[i, 7] = 1, 0.99 - 0.01 * i
        c = rng.uniform(0.4 * m, 0.6 * m, 3)
        ball = sum((g[a] - c[a]) ** 2 for a in range(3)) <= (0.36 * m) ** 2
        mask[i, ..., 1] = np.where(ball, rng.uniform(0.6, 0.95, (m, m, m)), mask[i, ..., 1])
    gt_boxes = np.zeros((G, 6), np.int64)
    for k in range(G):
        side = rng.integers(lo_side, hi_side + 1, 3)
        lo = np.array([rng.integers(0, S - s + 1) for s in side])
        gt_boxes[k] = np.concatenate([lo, lo + side])
    return det, mask, gt_boxes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--gt", type=int, default=50)
    ap.add_argument("--mask", type=int, default=28)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_unmold: no GPU (timings are taken on the device only)")
    import torch.nn.functional as F
    import unmoldref as U
    import m3d._lib as lib
    from m3d.config import synthetic_mrcnn_config
    dev = torch.device("cuda:0")
    S, G, m, C = a.size, a.gt, a.mask, 2
    N = int(synthetic_mrcnn_config(S).DETECTION_MAX_INSTANCES)
    det_h, mask_h, gt_boxes = workload(S, N, m, C, G)
    det, mask = torch.from_numpy(det_h).to(dev), torch.from_numpy(mask_h).to(dev)
    gt = torch.zeros((S, S, S, G), dtype=torch.uint8, device=dev)
    for k, (y1, x1, z1, y2, x2, z2) in enumerate(gt_boxes.tolist()):
        gt[y1:y2, x1:x2, z1:z2, k] = 1
    L, p = lib.load(), lib.ptr
    small = torch.empty((N, m ** 3), dtype=torch.uint8, device=dev)
    box_i = torch.empty((N, 6), dtype=torch.int32, device=dev)
    status = torch.empty(N, dtype=torch.int32, device=dev)
    stats = torch.empty((N, 8), dtype=torch.float64, device=dev)
    area = torch.empty(N, dtype=torch.int32, device=dev)
    inter = torch.empty((N, G), dtype=torch.int32, device=dev)
    area_gt = torch.empty(G, dtype=torch.int32, device=dev)
    iou = torch.empty((N, G), dtype=torch.float32, device=dev)

    def overlaps():
        lib.check(L.m3d_unmold_overlaps(p(small), p(box_i), p(status), p(stats), N, m, S, S, S, p(gt), G, p(area),
                                        p(inter), lib.stream()))

    def prepare():
        lib.check(L.m3d_unmold_prepare(p(det), p(mask), N, m, C, S, S, S, p(small), p(box_i), p(status), p(stats),
                                       lib.stream()))

    def areas():
        lib.check(L.m3d_mask_areas(p(gt), S, S, S, G, p(area_gt), lib.stream()))

    def full():
        s = lib.stream()
        prepare()
        overlaps()
        areas()
        lib.check(L.m3d_unmold_finalize(p(box_i), p(status), N, G, p(area), p(inter), p(area_gt), p(iou), s))

    full()
    torch.cuda.synchronize()
    boxes, st_h = box_i.cpu().tolist(), stats.cpu().numpy()
    ok = (status == 0).cpu().numpy()
    grids = small.view(N, 1, 1, m, m, m).float()
    dense = torch.zeros((N, S, S, S), dtype=torch.float32, device=dev)

    def framework():
        dense.zero_()
        for i in range(N):
            if not ok[i]:
                continue
            y1, x1, z1, y2, x2, z2 = boxes[i]
            v = F.interpolate(grids[i], size=(y2 - y1, x2 - x1, z2 - z1), mode="trilinear", align_corners=False)
            dense[i, y1:y2, x1:x2, z1:z2] = (v[0, 0] >= float(st_h[i, 7])).float()
        gf = gt.view(-1, G).float()
        it = dense.view(N, -1) @ gf
        ap_, ag = dense.view(N, -1).sum(1), gf.sum(0)
        return it, it / (ap_[:, None] + ag[None, :] - it)

    vox = sum((b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2]) for b, k in zip(boxes, ok) if k)
    # csrc/unmold.hip: UM_MAX_SLABS = 64, UM_SLAB_VOX = 2048, UM_BLOCK = 256 voxels per chunk
    slabs = min(64, max(1, -(-S ** 3 // 2048)))
    wgs = sum(min(slabs, -(-((b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2])) // 256)) for b, k in zip(boxes, ok) if k)
    alg = vox * G + wgs * m ** 3
    src = torch.zeros(alg, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def copy():
        dst.copy_(src)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    forms = {"full": full, "overlaps": overlaps, "prepare": prepare, "areas": areas, "framework": framework,
             "copy": copy}
    for _ in range(a.warmup):
        for fn in forms.values():
            timed(fn)
    ms = {k: [] for k in forms}
    for _ in range(a.runs):                                     # alternating, same process
        for k, fn in forms.items():
            ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    it_f, iou_f = framework()
    full()
    torch.cuda.synchronize()
    set_bytes = int(area.sum()) * G

    # (b) numpy at 64^3, boxes scaled by 1/4
    s4 = 64
    d4, m4, gb4 = workload(s4, N, m, C, G)
    gt4 = np.zeros((s4, s4, s4, G), np.uint8)
    for k, (y1, x1, z1, y2, x2, z2) in enumerate(gb4.tolist()):
        gt4[y1:y2, x1:x2, z1:z2, k] = 1
    t0 = time.perf_counter()
    r4 = U.unmold(d4, m4, (s4, s4, s4))
    i4, ag4 = U.overlaps(r4["dense"], gt4)
    U.iou_matrix(i4, r4["area_pred"], ag4)
    t_np = (time.perf_counter() - t0) * 1e3

    lines = [
        f"unmold + mask overlaps, {S}^3 volume, N={N} detections ({int(ok.sum())} with a mask) of {S // 8}-{S // 4} "
        f"voxels per side, m={m}, C={C}, G={G}; median of {a.runs} after {a.warmup} warm-up (HIP events, ms)",
        f"device: {torch.cuda.get_device_name(0)}",
    ]
    names = {"full": "(i)  prepare + overlaps + areas + finalize", "overlaps": "(ii) m3d_unmold_overlaps alone",
             "prepare": "     m3d_unmold_prepare alone", "areas": "     m3d_mask_areas alone",
             "framework": "(a)  framework ops from the thresholded grids", "copy": "     uint8 copy of the algorithmic bytes"}
    for k in forms:
        lines.append(f"{names[k]:46s} median {med[k]:9.4f}  min {min(ms[k]):9.4f}  max {max(ms[k]):9.4f}")
    lines.append(f"(a) / (i) = {med['framework'] / med['full']:.1f}x")
    lines.append(f"(b) numpy on the host CPU at 64^3 (boxes / 4): {t_np:.1f} ms measured; x 64 voxels = "
                 f"{t_np * 64 / 1e3:.1f} s extrapolated to {S}^3 (not measured at that size)")
    lines.append(f"overlaps kernel, algorithmic bytes: {vox} box voxels x {G} GT bytes + {wgs} workgroups x {m}^3 = "
                 f"{alg / 1e6:.1f} MB -> {alg / (med['overlaps'] * 1e-3) / 1e12:.3f} TB/s")
    lines.append(f"  uint8 copy of {alg / 1e6:.1f} MB in this run: {alg / (med['copy'] * 1e-3) / 1e12:.3f} TB/s of payload "
                 f"(read + write: twice that on the bus); the kernel's algorithmic rate is "
                 f"{med['copy'] / med['overlaps']:.2f} of it")
    lines.append(f"  GT bytes of set voxels only (what the kernel requests): {set_bytes / 1e6:.1f} MB "
                 f"({100.0 * set_bytes / max(vox * G, 1):.0f} % of the box bytes)")
    lines.append(f"mask_areas reads {S ** 3 * G / 1e6:.1f} MB once: {S ** 3 * G / (med['areas'] * 1e-3) / 1e12:.3f} TB/s")
    same = int((it_f.round().int() == inter).sum())
    lines.append(f"framework vs kernels: {same} of {N * G} intersection counts equal (the framework resize clamps at "
                 f"the grid's edge, the kernels blend with zeros; ties at the threshold differ in float32), "
                 f"max |IoU difference| {float(torch.nan_to_num(iou_f - iou).abs().max()):.3g}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
