"""Time of the segmentation-volume kernels (csrc/unmold.hip: m3d_unmold_labels,
m3d_label_pixelwise, m3d_labels_stack) at the workload of scripts/time_unmold.py
(a 256^3 volume, DETECTION_MAX_INSTANCES detections with boxes of 32-64 voxels
per side, MASK_SHAPE 28^3, C = 2, G = 50), each beside its yardstick in the
same process: HIP events, median of --runs after --warmup, forms alternating.

  labels     m3d_unmold_labels            against  m3d_unmold_paste(seg_union) on a zeroed volume
                                                   (the same traversal with plain stores) and a memset
                                                   of the label volume alone
  pixelwise  m3d_label_pixelwise          against  m3d_mask_areas: V (G + 4) bytes read where that
                                                   kernel reads V G
  stack      m3d_labels_stack (1 and 2 B) against  a device copy of as many bytes as it reads + writes

    python scripts/time_segment.py [--size 256] [--gt 50] [--runs 30] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "3d-mask-r-cnn_amd"), ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)


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
        sys.exit("time_segment: no GPU (timings are taken on the device only)")
    import m3d._lib as lib
    from m3d.config import synthetic_mrcnn_config
    from time_unmold import workload
    dev = torch.device("cuda:0")
    S, G, m, C = a.size, a.gt, a.mask, 2
    V = S ** 3
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
    area_gt = torch.empty(G, dtype=torch.int32, device=dev)
    label_of = torch.empty(N, dtype=torch.int32, device=dev)
    labels = torch.empty((S, S, S), dtype=torch.int32, device=dev)
    union = torch.empty((S, S, S), dtype=torch.uint8, device=dev)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    stack8 = torch.empty((S, S, S), dtype=torch.uint8, device=dev)
    stack16 = torch.empty((S, S, S), dtype=torch.uint16, device=dev)
    s = lib.stream()
    lib.check(L.m3d_unmold_prepare(p(det), p(mask), N, m, C, S, S, S, p(small), p(box_i), p(status), p(stats), s))
    lib.check(L.m3d_unmold_overlaps(p(small), p(box_i), p(status), p(stats), N, m, S, S, S, None, 0, p(area), None,
                                    s))
    lib.check(L.m3d_unmold_finalize(p(box_i), p(status), N, 0, p(area), None, None, None, s))

    def f_labels():
        lib.check(L.m3d_unmold_labels(p(small), p(box_i), p(status), p(stats), None, N, m, S, S, S, p(label_of),
                                      p(labels), lib.stream()))

    def f_paste():
        union.zero_()
        lib.check(L.m3d_unmold_paste(p(small), p(box_i), p(status), p(stats), N, m, S, S, S, None, p(union),
                                     lib.stream()))

    def f_memset():
        labels.zero_()

    def f_pixelwise():
        lib.check(L.m3d_label_pixelwise(p(labels), p(gt), S, S, S, G, p(counts), lib.stream()))

    def f_areas():
        lib.check(L.m3d_mask_areas(p(gt), S, S, S, G, p(area_gt), lib.stream()))

    def f_stack8():
        lib.check(L.m3d_labels_stack(p(labels), S, S, S, 1, p(stack8), lib.stream()))

    def f_stack16():
        lib.check(L.m3d_labels_stack(p(labels), S, S, S, 2, p(stack16), lib.stream()))

    src8 = torch.zeros(V * 5 // 2, dtype=torch.uint8, device=dev)      # a copy moves its bytes twice: (4 + 1) V / 2
    dst8 = torch.empty_like(src8)
    src16 = torch.zeros(V * 6 // 2, dtype=torch.uint8, device=dev)
    dst16 = torch.empty_like(src16)

    def f_copy8():
        dst8.copy_(src8)

    def f_copy16():
        dst16.copy_(src16)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    f_labels()                                                  # the label volume the later forms read
    torch.cuda.synchronize()
    forms = {"labels": f_labels, "paste": f_paste, "memset": f_memset, "pixelwise": f_pixelwise, "areas": f_areas,
             "stack8": f_stack8, "copy8": f_copy8, "stack16": f_stack16, "copy16": f_copy16}
    for _ in range(a.warmup):
        for k, fn in forms.items():
            timed(fn)
            if k == "memset":
                f_labels()
    ms = {k: [] for k in forms}
    for _ in range(a.runs):                                     # alternating, same process
        for k, fn in forms.items():
            ms[k].append(timed(fn))
            if k == "memset":
                f_labels()                                      # (untimed) the volume back for the readers
    med = {k: statistics.median(v) for k, v in ms.items()}
    torch.cuda.synchronize()
    set_vox = int(area.sum())
    painted = int((labels > 0).sum())
    ok = (status == 0).cpu().numpy()
    boxes = box_i.cpu().tolist()
    vox = sum((b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2]) for b, k in zip(boxes, ok) if k)
    tp, fp, fn = counts.cpu().tolist()

    def tbs(nbytes, t):
        return nbytes / (t * 1e-3) / 1e12

    names = {"labels": "m3d_unmold_labels (memset + scan + paint)", "paste": "  memset + m3d_unmold_paste(seg_union)",
             "memset": "  memset of the int32 label volume alone", "pixelwise": "m3d_label_pixelwise",
             "areas": "  m3d_mask_areas", "stack8": "m3d_labels_stack, 1-byte samples",
             "copy8": "  device copy of (4 + 1) V / 2 bytes", "stack16": "m3d_labels_stack, 2-byte samples",
             "copy16": "  device copy of (4 + 2) V / 2 bytes"}
    lines = [
        f"segmentation volume kernels, {S}^3 volume (V = {V}), N={N} detections ({int(ok.sum())} with a mask) of "
        f"{S // 8}-{S // 4} voxels per side, m={m}, C={C}, G={G}; median of {a.runs} after {a.warmup} warm-up "
        f"(HIP events, ms)",
        f"device: {torch.cuda.get_device_name(0)}",
    ]
    for k in forms:
        lines.append(f"{names[k]:46s} median {med[k]:9.4f}  min {min(ms[k]):9.4f}  max {max(ms[k]):9.4f}")
    lines.append(f"labels: {vox} box voxels evaluated, {set_vox} set ({painted} voxels labelled): {4 * set_vox / 1e6:.1f} MB "
                 f"of 32-bit atomic max on top of the {4 * V / 1e6:.1f} MB zero-fill; algorithmic bytes 4 V + set voxels "
                 f"x 4 = {(4 * V + 4 * set_vox) / 1e6:.1f} MB -> {tbs(4 * V + 4 * set_vox, med['labels']):.3f} TB/s; "
                 f"labels / (memset + paste) = {med['labels'] / med['paste']:.2f} "
                 f"(the paste zero-fills V bytes, the labels 4 V); labels - memset = "
                 f"{med['labels'] - med['memset']:.4f} ms for the scan and the paint")
    px_bytes, ar_bytes = V * (G + 4), V * G
    spread = max(ms["areas"]) - min(ms["areas"])
    lines.append(f"pixelwise: reads V (G + 4) = {px_bytes / 1e6:.1f} MB -> {tbs(px_bytes, med['pixelwise']):.3f} TB/s; "
                 f"mask_areas reads V G = {ar_bytes / 1e6:.1f} MB -> {tbs(ar_bytes, med['areas']):.3f} TB/s; "
                 f"pixelwise / areas = {med['pixelwise'] / med['areas']:.3f} against (G + 4) / G = {(G + 4) / G:.3f}; "
                 f"areas min-max spread {spread:.4f} ms, bound (G + 4) / G x areas + spread = "
                 f"{(G + 4) / G * med['areas'] + spread:.4f} ms; counts tp {tp} fp {fp} fn {fn}")
    for w, k, c in ((1, "stack8", "copy8"), (2, "stack16", "copy16")):
        nb = V * (4 + w)
        lines.append(f"stack, {w}-byte samples: reads 4 V + writes {w} V = {nb / 1e6:.1f} MB -> {tbs(nb, med[k]):.3f} TB/s; "
                     f"a device copy moving the same bytes (read + write) -> {tbs(nb, med[c]):.3f} TB/s; "
                     f"stack / copy = {med[k] / med[c]:.2f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
