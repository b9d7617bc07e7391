"""Time of the fused head losses (m3d.head_losses.mrcnn_losses, forward +
backward) against the framework-op form (tests/headloss_ref.py in float32 on
the GPU, forward + autograd backward) on the same inputs, at the reference's
defaults R = TRAIN_ROIS_PER_IMAGE = 512, MASK_SHAPE = 28^3, NUM_CLASSES = 2.

HIP events around each forward + backward, median of --runs after --warmup,
the two forms alternating in one process.  Also prints the algorithmic HBM
bytes of the mask pass (forward 4 R V (C + 1), backward the same read plus
4 R V C written; rows that are not positive are not read, so the bytes really
moved are fewer) and the share of the 8.0 TB/s HBM peak they imply.

    python scripts/time_head_loss.py [--rois 512] [--mask 28] [--classes 2] [--runs 30] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "3d-mask-r-cnn_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK = 8.0e12


def inputs(T, m, C, dev, pos_frac):
    g = torch.Generator().manual_seed(0)
    ids = torch.zeros((1, T), dtype=torch.int32)
    npos = int(T * pos_frac)
    ids[0, T - npos:] = torch.randint(1, C, (npos,), generator=g, dtype=torch.int32)
    t = dict(ids=ids, tbox=torch.randn((1, T, 6), generator=g) * 1.5,
             tmask=(torch.rand((1, T, m, m, m), generator=g) < 0.3).float(),
             logits=torch.randn((1, T, C), generator=g) * 6, bbox=torch.randn((1, T, C, 6), generator=g) * 2.5,
             mask=torch.rand((1, T, m, m, m, C), generator=g), active=torch.ones((1, C)))
    t = {k: v.to(dev) for k, v in t.items()}
    for k in ("logits", "bbox", "mask"):
        t[k].requires_grad_(True)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rois", type=int, default=512)
    ap.add_argument("--mask", type=int, default=28)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--pos-frac", type=float, default=0.33, help="share of positive rows (ROI_POSITIVE_RATIO)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_head_loss: no GPU (timings are taken on the device only)")
    import headloss_ref as HL
    from m3d.head_losses import mrcnn_losses
    dev = torch.device("cuda:0")
    t = inputs(a.rois, a.mask, a.classes, dev, a.pos_frac)
    keys = ("logits", "bbox", "mask")

    def fused():
        out = mrcnn_losses(t["ids"], t["tbox"], t["tmask"], t["logits"], t["bbox"], t["mask"], t["active"])
        out[0].backward()
        return out

    def framework():
        out = HL.losses(t["ids"], t["tbox"], t["tmask"], t["logits"], t["bbox"], t["mask"], t["active"])
        out[0].backward()
        return out

    def timed(fn):
        for k in keys:
            t[k].grad = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    for _ in range(a.warmup):
        timed(fused)
        timed(framework)
    ms = {"fused": [], "framework": []}
    for _ in range(a.runs):                                     # alternating, same process
        ms["fused"].append(timed(fused)[0])
        ms["framework"].append(timed(framework)[0])
    # the fused pair as one captured HIP graph: the same launches without the host enqueue between them
    for k in keys:
        t[k].grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fused()
    for _ in range(a.warmup):
        graph.replay()
    ms["fused_graph"] = [timed(graph.replay)[0] for _ in range(a.runs)]
    _, of = timed(fused)
    gf = [t[k].grad.clone() for k in keys]
    _, orf = timed(framework)
    gr = [t[k].grad.clone() for k in keys]
    R, V, C = a.rois, a.mask ** 3, a.classes
    fwd_b, bwd_b = 4 * R * V * (C + 1), 4 * R * V * (C + 1) + 4 * R * V * C
    med = {k: statistics.median(v) for k, v in ms.items()}
    lines = [
        f"head losses, forward + backward, R={R} V={a.mask}^3 C={C}, {int(R * a.pos_frac)} positive rows, "
        f"median of {a.runs} after {a.warmup} warm-up (HIP events, ms)",
        f"device: {torch.cuda.get_device_name(0)}",
    ]
    for k in ("fused", "fused_graph", "framework"):
        v = ms[k]
        lines.append(f"{k:11s} median {med[k]:.4f}  min {min(v):.4f}  max {max(v):.4f}")
    lines.append(f"framework / fused = {med['framework'] / med['fused']:.2f}x")
    lines.append(f"algorithmic mask bytes: forward {fwd_b / 1e6:.1f} MB + backward {bwd_b / 1e6:.1f} MB")
    lines.append(f"  = {(fwd_b + bwd_b) / (med['fused_graph'] * 1e-3) / 1e12:.3f} TB/s over the graph-replay median "
                 f"= {100 * (fwd_b + bwd_b) / (med['fused_graph'] * 1e-3) / HBM_PEAK:.1f} % of the 8.0 TB/s HBM peak "
                 f"(all launches of the pair, their boundaries and the allocator's included)")
    P = int((t["ids"] > 0).sum())
    moved = 2 * 4 * P * V * (C + 1) + 4 * R * V * C              # positive rows read twice, the gradient written whole
    lines.append(f"bytes moved (only the {P} positive rows are read): {moved / 1e6:.1f} MB "
                 f"= {moved / (med['fused_graph'] * 1e-3) / 1e12:.3f} TB/s "
                 f"= {100 * moved / (med['fused_graph'] * 1e-3) / HBM_PEAK:.1f} % of peak over the same time")
    lines.append("losses  fused     " + " ".join(f"{float(v.detach()):.7f}" for v in of))
    lines.append("losses  framework " + " ".join(f"{float(v.detach()):.7f}" for v in orf))
    for k, x, y in zip(keys, gf, gr):
        lines.append(f"grad {k:6s} max |fused - framework| = {float((x - y).abs().max()):.3g} "
                     f"of max entry {float(y.abs().max()):.3g}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
