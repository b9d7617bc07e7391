"""Time of the RPN-evaluation scoring (csrc/rpn_eval.hip: m3d_rpn_eval_proposals,
three launches) for one image at R = 6000 proposals (POST_NMS_ROIS_TRAINING), G =
50 GT boxes and the T = 3 thresholds of EVAL_MATCH_IOU_GRID, beside two other
routes to the same record in the same process:

  kernel  m3d.rpn_eval.score_proposals into a preallocated record
  replay  the same calls replayed from one HIP-graph capture (no host enqueue)
  torch   the same scoring as a torch expression on the device (pixel boxes,
          the [G,R] IoU, arg-max over G, a scatter-min for the claims, a masked
          min over rows for the first hits)
  host    the reference's route: the proposals copied to the host
          (synchronising), then the NumPy restatement tests/rpnevalref.py

kernel and torch: HIP events around --inner back-to-back calls, median of --runs
after --warmup, forms alternating; both include the host's enqueue when that
is slower than the device.  host: a host clock from a synchronised start to the
end of the NumPy work, one call per sample.

    python scripts/time_rpneval.py [--rois 6000] [--gt 50] [--runs 30] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "3d-mask-r-cnn_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

NONE = 2 ** 31 - 1


def make_case(R, G, shape, seed=0):
    """GT boxes at non-integer coordinates; half the proposals are a GT box moved
    by sub-voxel or few-voxel offsets, a tenth zero rows, the rest uniform."""
    rng = np.random.default_rng(seed)
    dims = np.array(shape, np.float64)
    lo = rng.uniform(0.0, 0.65, (G, 3)) * dims
    gt = np.concatenate([lo, lo + rng.uniform(0.08, 0.3, (G, 3)) * dims], 1).astype(np.float32)
    kind = rng.uniform(size=R)
    scale = np.where(rng.uniform(size=(R, 1)) < 0.5, 0.4, 3.0)
    near = gt[rng.integers(0, G, R)].astype(np.float64) + rng.normal(size=(R, 6)) * scale
    a, b = rng.uniform(0.0, 1.0, (R, 3)) * dims, rng.uniform(0.0, 1.0, (R, 3)) * dims
    px = np.where((kind < 0.5)[:, None], near, np.concatenate([np.minimum(a, b), np.maximum(a, b)], 1))
    rois = (px / np.concatenate([dims, dims])).astype(np.float32)
    rois[kind > 0.9] = 0.0
    return rois, gt


def torch_score(rois, gt, scale, lo, hi, topk, thr, grid):
    """The record as torch ops on the device -> (assoc, matched, first_hit, counts)."""
    R, G = rois.shape[0], gt.shape[0]
    px = torch.minimum(torch.maximum(rois * scale, lo), hi)
    valid = (px[:, 3] > px[:, 0]) & (px[:, 4] > px[:, 1]) & (px[:, 5] > px[:, 2])
    a = torch.cat([torch.minimum(gt[:, :3], gt[:, 3:]), torch.maximum(gt[:, :3], gt[:, 3:])], 1)[:, None, :]
    b = px[None]
    ext = (torch.minimum(a[..., 3:], b[..., 3:]) - torch.maximum(a[..., :3], b[..., :3])).clamp_min(0.0)
    inter = (ext[..., 0] * ext[..., 1]) * ext[..., 2]
    sa, sb = a[..., 3:] - a[..., :3], b[..., 3:] - b[..., :3]
    union = (((sa[..., 0] * sa[..., 1]) * sa[..., 2] + (sb[..., 0] * sb[..., 1]) * sb[..., 2]) - inter).clamp_min(1e-10)
    iou = torch.where(valid[None], (inter / union).clamp(0.0, 1.0), torch.zeros((), device=rois.device))
    idx = torch.arange(R, device=rois.device, dtype=torch.int32)
    none = torch.full((), NONE, device=rois.device, dtype=torch.int32)
    first_hit = torch.where((iou[None] >= grid[:, None, None]) & valid[None, None], idx, none).amin(-1)
    k = min(topk, R)
    best, arg = iou[:, :k].max(0)
    claim = torch.where(valid[:k] & (best.double() > thr), idx[:k], none)
    assoc = torch.full((G,), NONE, device=rois.device, dtype=torch.int32).scatter_reduce(0, arg, claim, "amin")
    hit = assoc != NONE
    matched = px[assoc.clamp(0, max(R - 1, 0)).long()] * hit[:, None]
    counts = torch.stack([valid[:k].sum().to(torch.int32), torch.where(valid, idx, none).amin()])
    return torch.where(hit, assoc, torch.full_like(assoc, -1)), matched, first_hit, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rois", type=int, default=6000)
    ap.add_argument("--gt", type=int, default=50)
    ap.add_argument("--topk", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_rpneval: no GPU (timings are taken on the device only)")
    import rpnevalref as E
    from m3d import rpn_eval
    dev = torch.device("cuda:0")
    shape, thr, grid_vals = (256, 256, 64), 0.5, [0.30, 0.40, 0.50]
    R, G, T = a.rois, a.gt, len(grid_vals)
    rois_h, gt_h = make_case(R, G, shape)
    rois, gt = torch.from_numpy(rois_h).to(dev), torch.from_numpy(gt_h).to(dev)
    grid = torch.tensor(grid_vals, dtype=torch.float32, device=dev)
    H, W, D = shape
    scale = torch.tensor([H, W, D, H, W, D], dtype=torch.float32, device=dev)
    lo = torch.tensor([0, 0, 0, 1, 1, 1], dtype=torch.float32, device=dev)
    rec = torch.empty(rpn_eval.record_len(G, T), dtype=torch.int32, device=dev)

    def kernel():
        rpn_eval.score_proposals(rois, gt, shape, a.topk, thr, grid, out=rec)

    def expr():
        return torch_score(rois, gt, scale, lo, scale, a.topk, thr, grid)

    def host():
        return E.score(rois.cpu().numpy(), gt_h, shape, a.topk, thr, grid_vals)

    # the three routes agree before anything is timed
    kernel()
    want = host()
    got = rpn_eval.unpack_record(rec.cpu().numpy(), G, T)
    assert all(np.array_equal(got[k].view(np.int32), want[k].view(np.int32)) for k in got), "kernel != restatement"
    t_assoc, t_matched, t_hit, t_counts = (t.cpu().numpy() for t in expr())
    assert np.array_equal(t_hit, want["first_hit"]) and np.array_equal(t_counts, want["counts"]), "torch != restatement"
    same_assoc = bool(np.array_equal(t_assoc, want["assoc"]))   # torch's max() does not promise the first maximum

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner

    def timed_host(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    # the same --inner calls captured once into a HIP graph: the device's share of `kernel`
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(a.inner):
            kernel()

    def timed_graph(_):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner

    runs = {"kernel": (kernel, timed), "replay": (None, timed_graph), "torch": (expr, timed),
            "host": (host, timed_host)}
    for _ in range(a.warmup):
        for fn, clock in runs.values():
            clock(fn)
    ms = {k: [] for k in runs}
    for _ in range(a.runs):                                     # alternating, same process
        for k, (fn, clock) in runs.items():
            ms[k].append(clock(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    matched_n = int((want["assoc"] >= 0).sum())
    lines = [f"RPN-evaluation scoring of one image, R={R} proposals, G={G} GT boxes, T={T} thresholds, topk={a.topk}, "
             f"volume {shape}; {matched_n} of {G} GT boxes matched; median of {a.runs} after {a.warmup} warm-up "
             f"(kernel / torch: HIP events around {a.inner} calls, ms per call; replay: around one replay of a graph "
             f"of {a.inner} calls; host: host clock, one call)",
             f"device: {torch.cuda.get_device_name(0)}",
             f"{'route':8s} {'median ms':>10s} {'min ms':>10s} {'max ms':>10s} {'/ kernel':>9s}"]
    for k in runs:
        lines.append(f"{k:8s} {med[k]:10.4f} {min(ms[k]):10.4f} {max(ms[k]):10.4f} {med[k] / med['kernel']:9.2f}")
    lines.append(f"torch expression's assoc equals the restatement's: {same_assoc} (first_hit and counts: asserted)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
