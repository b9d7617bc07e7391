"""Time of the mask head's training forward + backward
(m3d.heads.MaskHead(training=True): batch-statistics BN, all 24 parameter
gradients and d_pooled) against the same graph written with framework ops in
float32 on the same GPU (tests/maskhead_ref.forward + autograd), at the default
config: T = 128 ROIs, p = 14, 256 channels, C = 2.  Both forms get the same
fixed upstream gradient of mrcnn_mask, so the loss is not in the timed region.

HIP events around each forward + backward, median of --runs after --warmup, the
two forms alternating in one process.

m3d_mask_out_bwd is then timed alone, alternating with (a) the same three
operations in framework ops (the sigmoid / ReLU-masked data gradient, the
mrcnn_mask kernel and bias gradients, the deconv bias gradient) and (b) a float4
copy of up's size (torch's device-to-device copy), all in the same run.  Its
algorithmic bytes are 8 V ch (up read once, g_up written once) plus 8 V C
(g_mask, out) and the small weight / partial terms; the share of the 8.0 TB/s
HBM peak is those bytes over the median time.

    python scripts/time_mask_head_train.py [--rois 128] [--pool 14] [--channels 256] [--runs 30] [--out FILE]
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


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(forms, warmup, runs):
    for _ in range(warmup):
        for fn in forms.values():
            timed(fn)
    ms = {k: [] for k in forms}
    for _ in range(runs):
        for k, fn in forms.items():
            ms[k].append(timed(fn))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rois", type=int, default=128)
    ap.add_argument("--pool", type=int, default=14)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_mask_head_train: no GPU (timings are taken on the device only)")
    import maskhead_ref as MR
    from m3d import _lib
    from m3d.heads import MaskHead
    from m3d.params import ParamStore
    dev = torch.device("cuda:0")
    T, p, ch, C = a.rois, a.pool, a.channels, a.classes
    store = ParamStore()
    head = MaskHead(store, C, ch, ch)
    store.finalize(dev, seed=1)
    g = torch.Generator(device=dev).manual_seed(0)
    pooled = torch.randn((1, T, p, p, p, ch), device=dev, generator=g).requires_grad_(True)
    g_out = torch.randn((1, T, 2 * p, 2 * p, 2 * p, C), device=dev, generator=g) * 1e-3
    names = MR.PARAM_NAMES
    q = {k: store.by_name[k].data.detach().clone().requires_grad_(True) for k in names}

    def ours():
        pooled.grad = None
        store.grad_flat.zero_()
        head(pooled, training=True).backward(g_out)

    def framework():
        pooled.grad = None
        for t in q.values():
            t.grad = None
        MR.forward(q, pooled)[0].backward(g_out)

    ms = alternate({"libm3d": ours, "framework": framework}, a.warmup, a.runs)
    timed(ours)
    mine = {k: store.by_name[k].grad.clone() for k in names}
    dp = pooled.grad.clone()
    timed(framework)
    diffs = [f"grad {k:30s} max |libm3d - framework| = {float((mine[k] - q[k].grad).abs().max()):.3g} "
             f"of max entry {float(q[k].grad.abs().max()):.3g}" for k in names]
    diffs.append(f"d_pooled max |libm3d - framework| = {float((dp - pooled.grad).abs().max()):.3g} "
                 f"of max entry {float(pooled.grad.abs().max()):.3g}")
    del mine, dp
    pooled.grad = None
    for t in q.values():
        t.grad = None
    torch.cuda.empty_cache()

    # ---- m3d_mask_out_bwd alone
    L = _lib.load()
    V = T * (2 * p) ** 3
    up = torch.randn((V, ch), device=dev, generator=g).clamp_(min=0)
    w = torch.randn((ch, C), device=dev, generator=g) / 16
    out = torch.sigmoid(torch.randn((V, C), device=dev, generator=g))
    gm = torch.randn((V, C), device=dev, generator=g)
    g_up = torch.empty_like(up)
    dW, db, dbd = (torch.zeros(s, device=dev) for s in ((ch, C), (C,), (ch,)))
    wsb = int(L.m3d_mask_out_bwd_workspace_bytes(V, ch, C))
    ws = torch.empty(wsb // 4, device=dev)
    copy_dst = torch.empty_like(up)

    def kernel():
        _lib.check(L.m3d_mask_out_bwd(gm.data_ptr(), out.data_ptr(), up.data_ptr(), w.data_ptr(), V, ch, C,
                                      g_up.data_ptr(), dW.data_ptr(), db.data_ptr(), dbd.data_ptr(), ws.data_ptr(),
                                      wsb, _lib.stream()), "mask_out_bwd")

    def ops():
        gl = gm * out * (1 - out)
        gu = (gl @ w.T) * (up > 0)
        return gu, up.T @ gl, gl.sum(0), gu.sum(0)

    km = alternate({"m3d_mask_out_bwd": kernel, "framework_ops": ops, "float4_copy": lambda: copy_dst.copy_(up)},
                   a.warmup, a.runs)
    med = {k: statistics.median(v) for k, v in {**ms, **km}.items()}
    kbytes = 8 * V * ch + 8 * V * C + 4 * ch * C + 2 * wsb
    lines = [f"mask head training forward + backward, T={T} p={p} channels={ch} classes={C}, median of {a.runs} after "
             f"{a.warmup} warm-up (HIP events, ms), the forms alternating in one process",
             f"device: {torch.cuda.get_device_name(0)}"]
    for k in ("libm3d", "framework"):
        lines.append(f"{k:17s} median {med[k]:.3f}  min {min(ms[k]):.3f}  max {max(ms[k]):.3f}")
    lines.append(f"framework / libm3d = {med['framework'] / med['libm3d']:.2f}x")
    lines.append(f"m3d_mask_out_bwd alone, V={V} rows x {ch} channels (up {4 * V * ch / 1e9:.2f} GB):")
    for k in ("m3d_mask_out_bwd", "framework_ops", "float4_copy"):
        lines.append(f"{k:17s} median {med[k]:.3f}  min {min(km[k]):.3f}  max {max(km[k]):.3f}")
    lines.append(f"framework_ops / m3d_mask_out_bwd = {med['framework_ops'] / med['m3d_mask_out_bwd']:.2f}x")
    lines.append(f"algorithmic bytes {kbytes / 1e9:.3f} GB (8 V ch + 8 V C + w + partials) = "
                 f"{kbytes / (med['m3d_mask_out_bwd'] * 1e-3) / 1e12:.2f} TB/s = "
                 f"{100 * kbytes / (med['m3d_mask_out_bwd'] * 1e-3) / HBM_PEAK:.1f} % of the 8.0 TB/s HBM peak; "
                 f"the float4 copy of up ({8 * V * ch / 1e9:.3f} GB read + written) runs at "
                 f"{8 * V * ch / (med['float4_copy'] * 1e-3) / 1e12:.2f} TB/s in the same run")
    lines += diffs
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
