"""Time of the classifier head's training forward + backward
(m3d.heads.ClassifierHead(training=True): batch-statistics BN, all twelve
parameter gradients and d_pooled) against the same graph written with
framework ops in float32 on the same GPU (tests/headtrain_ref.head_forward +
autograd), at the default config: M = 512 ROIs, pool 7, C 256, fc 1024,
num_classes 2.  Both forms get the same fixed upstream gradients of the logits
and the boxes, so the losses are not in the timed region.

HIP events around each forward + backward, median of --runs after --warmup,
the two forms alternating in one process; the libm3d form also as one captured
HIP graph.  Also prints the algorithmic HBM bytes -- conv1 dominates: its
forward reads x [M, K] and W1 [K, fc], its weight gradient reads x and writes
dW1, its data gradient reads W1 and writes d_pooled (K = pool^3 C) -- and the
share of the 8.0 TB/s HBM peak they imply over the graph-replay median.

    python scripts/time_head_train.py [--rois 512] [--pool 7] [--channels 256] [--fc 1024] [--runs 30] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rois", type=int, default=512)
    ap.add_argument("--pool", type=int, default=7)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--fc", type=int, default=1024)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_head_train: no GPU (timings are taken on the device only)")
    import headtrain_ref as HT
    from m3d.heads import ClassifierHead
    from m3d.params import ParamStore
    dev = torch.device("cuda:0")
    M, p, C, fc, nc = a.rois, a.pool, a.channels, a.fc, a.classes
    K = p ** 3 * C
    store = ParamStore()
    head = ClassifierHead(store, p, nc, fc, C)
    store.finalize(dev, seed=1)
    g = torch.Generator(device=dev).manual_seed(0)
    pooled = torch.randn((1, M, p, p, p, C), device=dev, generator=g).requires_grad_(True)
    g_logits = torch.randn((1, M, nc), device=dev, generator=g) * 1e-3
    g_bbox = torch.randn((1, M, nc, 6), device=dev, generator=g) * 1e-3
    names = HT.PARAM_NAMES
    q = {k: store.by_name[k].data.detach().clone().requires_grad_(True) for k in names}

    def ours():
        store.grad_flat.zero_()
        logits, _, bbox = head(pooled, training=True)
        torch.autograd.backward([logits, bbox], [g_logits, g_bbox])

    def framework():
        for t in q.values():
            t.grad = None
        logits, _, bbox, _ = HT.head_forward(q, pooled, nc, training=True)
        torch.autograd.backward([logits, bbox], [g_logits, g_bbox])

    def timed(fn):
        pooled.grad = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(a.warmup):
        timed(ours)
        timed(framework)
    ms = {"libm3d": [], "framework": []}
    for _ in range(a.runs):                                     # alternating, same process
        ms["libm3d"].append(timed(ours))
        ms["framework"].append(timed(framework))
    pooled.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ours()
    for _ in range(a.warmup):
        graph.replay()
    ms["libm3d_graph"] = [timed(graph.replay) for _ in range(a.runs)]
    # same results?  (one more run of each; the moving statistics are not compared)
    timed(ours)
    mine = {k: store.by_name[k].grad.clone() for k in names}
    dp = pooled.grad.clone()
    timed(framework)
    med = {k: statistics.median(v) for k, v in ms.items()}
    x_b, w_b = 4 * M * K, 4 * K * fc
    parts = {"conv1 forward (x + W1)": x_b + w_b, "conv1 weight gradient (x + dW1)": x_b + w_b,
             "conv1 data gradient (W1 + d_pooled)": w_b + x_b}
    total = sum(parts.values())
    lines = [f"classifier head training forward + backward, M={M} pool={p} C={C} fc={fc} classes={nc} (K={K}), "
             f"median of {a.runs} after {a.warmup} warm-up (HIP events, ms)",
             f"device: {torch.cuda.get_device_name(0)}"]
    for k in ("libm3d", "libm3d_graph", "framework"):
        v = ms[k]
        lines.append(f"{k:13s} median {med[k]:.4f}  min {min(v):.4f}  max {max(v):.4f}")
    lines.append(f"framework / libm3d = {med['framework'] / med['libm3d']:.2f}x (eager), "
                 f"{med['framework'] / med['libm3d_graph']:.2f}x (graph)")
    for k, v in parts.items():
        lines.append(f"algorithmic bytes, {k}: {v / 1e6:.1f} MB")
    lines.append(f"  total {total / 1e6:.1f} MB = {total / (med['libm3d_graph'] * 1e-3) / 1e12:.3f} TB/s over the "
                 f"graph-replay median = {100 * total / (med['libm3d_graph'] * 1e-3) / HBM_PEAK:.1f} % of the "
                 f"8.0 TB/s HBM peak (every launch of the pass and its boundaries included; the [M, fc] "
                 f"activations, BN passes and Dense layers add < 1 % of these bytes)")
    for k in names:
        ref = q[k].grad
        lines.append(f"grad {k:30s} max |libm3d - framework| = {float((mine[k] - ref).abs().max()):.3g} "
                     f"of max entry {float(ref.abs().max()):.3g}")
    lines.append(f"d_pooled max |libm3d - framework| = {float((dp - pooled.grad).abs().max()):.3g} "
                 f"of max entry {float(pooled.grad.abs().max()):.3g}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
