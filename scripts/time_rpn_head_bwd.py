"""Time the RPN head's backward alone, dense (today's per-unit path) against the
compact route (nn.RPN_HEAD_COMPACT), on the pyramid of an S^3 volume:

    python scripts/time_rpn_head_bwd.py 64 128 [--iters 10] [--depth D]

The pyramid comes from one no-grad forward of the backbone and FPN; each
iteration runs the head's forward and the fused RPN loss, then times
loss.backward() + RPNHead.finish_backward() (the side-stream join included)
with device events.  Prints one JSON line per size: rows, cap and the median /
min ms of both routes -- the numbers RPN_HEAD_COMPACT_MIN_ROWS is set from
(DESIGN.md 5)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-mask-r-cnn_amd")]


def time_head(S, depth, iters):
    import torch
    from m3d import nn as mnn
    from m3d.config import synthetic_rpn_config
    from m3d.model import RPN, RPNTargets, rpn_losses, synthetic_rpn_targets, synthetic_volume
    dev = torch.device("cuda:0")
    cfg = synthetic_rpn_config(S, depth=depth or None)
    model = RPN(cfg, device=dev, seed=1)
    image = synthetic_volume(S, depth or None, seed=100).to(dev)
    match, bbox = synthetic_rpn_targets(model.anchors.shape[1], cfg.RPN_TRAIN_ANCHORS_PER_IMAGE, seed=200)
    targets = RPNTargets(match, bbox, dev)
    with torch.no_grad():
        fmaps = [p.detach() for p in model.features(image)]
    rows = sum(p.shape[1] * p.shape[2] * p.shape[3] for p in fmaps)
    res = {"size": S, "depth": int(image.shape[3]), "rows": rows, "sampled_anchors": targets.n_cls}
    for name, on in (("dense", False), ("compact", True)):
        mnn.RPN_HEAD_COMPACT, mnn.RPN_HEAD_COMPACT_MIN_ROWS = on, 0
        ts = []
        for it in range(iters + 2):
            model.store.zero_grad()
            leaves = [p.clone().requires_grad_() for p in fmaps]
            model.rpn.active_rows_bound = targets.active_rows_bound
            logits, _, rb = model.rpn(leaves)
            total, _, _ = rpn_losses(targets, logits, rb, 1.0, 1.5)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            total.backward()
            model.rpn.finish_backward()
            e1.record()
            torch.cuda.synchronize()
            if it >= 2:
                ts.append(e0.elapsed_time(e1))
        model.rpn.check_compact()
        res[name + "_ms"] = {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", type=int, nargs="+")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--depth", type=int, default=0)
    a = ap.parse_args()
    for S in a.sizes:
        print(json.dumps(time_head(S, a.depth, a.iters)), flush=True)


if __name__ == "__main__":
    main()
