"""Time of the stored-head-target kernels (csrc/headstore.hip: m3d_pack_bits_f32,
m3d_f32_to_f16, m3d_unpack_gather_bits, m3d_unpack_gather_f16, and
m3d_bits_row_counts) at one image of TRAIN_ROIS_PER_IMAGE = 128 ROIs (POOL_SIZE
7, MASK_POOL_SIZE 14, 256 channels, MASK_SHAPE 28^3), each beside two
yardsticks in the same process: a device copy of as many bytes as the kernel
reads + writes, and the torch expression of the same result.  HIP events
around --inner back-to-back launches, median of --runs after --warmup, forms
alternating.  The gathers also run beside a memset of their output.

  pack      mask_aligned [T,14,14,14,256] f32 -> bits      torch: (x > 0.5) bytes x (128 .. 1) summed over 8
  pack_tm   target_mask  [T,28,28,28]     f32 -> bits
  half      rois_aligned [T,7,7,7,256]    f32 -> f16       torch: x.half()
  gather    mask bits -> [T,14,14,14,256] f32 (T rows in a shuffled order)
                                                           torch: index_select, shift, & 1, .float()
  gather_tm target-mask bits -> [T,28,28,28,1] f32 (the one-channel path)
  widen     rois_aligned f16 -> [T,7,7,7,256] f32          torch: index_select + .float()
  counts    set bits of each target-mask row               torch: unpacked .sum(1)

    python scripts/time_headstore.py [--rois 128] [--runs 30] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "3d-mask-r-cnn_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rois", type=int, default=128)
    ap.add_argument("--pool", type=int, default=7)
    ap.add_argument("--mask-pool", type=int, default=14)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--mask", type=int, default=28)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_headstore: no GPU (timings are taken on the device only)")
    import m3d._lib as lib
    from m3d import headstore
    dev = torch.device("cuda:0")
    T, P, M, C, m = a.rois, a.pool, a.mask_pool, a.channels, a.mask
    g = torch.Generator(device=dev).manual_seed(0)
    ra = torch.randn((T, P, P, P, C), device=dev, generator=g)
    ma = torch.rand((T, M, M, M, C), device=dev, generator=g)
    tm = (torch.rand((T, m, m, m), device=dev, generator=g) > 0.7).float()
    n_ra, n_ma, n_tm = ra.numel(), ma.numel(), tm.numel()
    assert n_ma % 8 == 0 and n_tm % 8 == 0
    ra16, ma_bits, tm_bits = headstore.to_half(ra), headstore.pack_bits(ma), headstore.pack_bits(tm)
    sel_host = torch.randperm(T, generator=torch.Generator().manual_seed(1))
    sel = sel_host.to(dev)
    L, p = lib.load(), lib.ptr
    sel32 = sel.to(torch.int32)
    tabs = {k: torch.arange(k, dtype=torch.int32, device=dev) for k in (P, M, m)}
    out_ma, out_tm, out_ra = torch.empty_like(ma), torch.empty((T, m, m, m, 1), device=dev), torch.empty_like(ra)
    bits_ma, bits_tm = torch.empty_like(ma_bits), torch.empty_like(tm_bits)
    half_ra = torch.empty_like(ra16)
    counts = torch.empty(T, dtype=torch.int32, device=dev)
    weights = torch.tensor([128, 64, 32, 16, 8, 4, 2, 1], dtype=torch.uint8, device=dev)
    shifts = torch.tensor([7, 6, 5, 4, 3, 2, 1, 0], dtype=torch.uint8, device=dev)

    def gather(fn, src, S, Cc, out):
        t = tabs[S]
        lib.check(fn(p(src), T, S, S, S, Cc, p(sel32), T, p(t), p(t), p(t), S, S, S, p(out), lib.stream()))

    def t_pack(x):
        return ((x > 0.5).view(-1, 8).to(torch.uint8) * weights).sum(1, dtype=torch.int32).to(torch.uint8)

    def t_unpack(bits, shape):
        rows = bits.view(shape[0], -1).index_select(0, sel)
        return ((rows.unsqueeze(-1) >> shifts) & 1).float().view(shape)

    # name -> (kernel, torch expression, bytes read + written by the kernel)
    forms = {
        "pack": (lambda: lib.check(L.m3d_pack_bits_f32(p(ma), n_ma, p(bits_ma), lib.stream())),
                 lambda: t_pack(ma), 4 * n_ma + n_ma // 8),
        "pack_tm": (lambda: lib.check(L.m3d_pack_bits_f32(p(tm), n_tm, p(bits_tm), lib.stream())),
                    lambda: t_pack(tm), 4 * n_tm + n_tm // 8),
        "half": (lambda: lib.check(L.m3d_f32_to_f16(p(ra), n_ra, p(half_ra), lib.stream())),
                 lambda: ra.half(), 6 * n_ra),
        "gather": (lambda: gather(L.m3d_unpack_gather_bits, ma_bits, M, C, out_ma),
                   lambda: t_unpack(ma_bits, (T, M, M, M, C)), n_ma // 8 + 4 * n_ma),
        "gather_tm": (lambda: gather(L.m3d_unpack_gather_bits, tm_bits, m, 1, out_tm),
                      lambda: t_unpack(tm_bits, (T, m, m, m, 1)), n_tm // 8 + 4 * n_tm),
        "widen": (lambda: gather(L.m3d_unpack_gather_f16, ra16, P, C, out_ra),
                  lambda: ra16.index_select(0, sel).float(), 6 * n_ra),
        "counts": (lambda: lib.check(L.m3d_bits_row_counts(p(tm_bits), T, m ** 3, p(counts), lib.stream())),
                   lambda: ((tm_bits.view(T, -1).unsqueeze(-1) >> shifts) & 1).sum((1, 2), dtype=torch.int32),
                   n_tm // 8 + 4 * T),
    }
    copies = {}
    for k, (_, _, nbytes) in forms.items():                     # a copy moves its bytes twice
        src = torch.randint(0, 255, (max(nbytes // 2, 1),), dtype=torch.uint8, device=dev)
        copies[k] = (src, torch.empty_like(src))

    # the kernels and the torch expressions agree before anything is timed
    for k, (kern, _, _) in forms.items():
        kern()
    assert torch.equal(bits_ma, t_pack(ma)) and torch.equal(bits_tm, t_pack(tm)) and torch.equal(half_ra, ra.half())
    assert torch.equal(out_ma, t_unpack(ma_bits, (T, M, M, M, C))) and torch.equal(out_ra, ra16.index_select(0, sel).float())
    assert torch.equal(out_tm, t_unpack(tm_bits, (T, m, m, m, 1))) and torch.equal(counts, forms["counts"][1]())

    def timed(fn):
        # --inner launches back to back between the events: these kernels take 8-120 us, and a
        # single launch between two events is timed with the host's launch latency on top
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner

    def copy_of(k):
        return lambda: copies[k][1].copy_(copies[k][0])

    fills = {"gather": out_ma, "gather_tm": out_tm, "widen": out_ra}          # the write side alone: a memset of the output
    runs = {}
    for k, (kern, expr, _) in forms.items():
        runs[k], runs[k + ":copy"], runs[k + ":torch"] = kern, copy_of(k), expr
        if k in fills:
            runs[k + ":fill"] = fills[k].zero_
    for _ in range(a.warmup):
        for fn in runs.values():
            timed(fn)
    ms = {k: [] for k in runs}
    for _ in range(a.runs):                                     # alternating, same process
        for k, fn in runs.items():
            ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}

    def tbs(nbytes, t):
        return nbytes / (t * 1e-3) / 1e12

    lines = [f"stored-head-target kernels, T={T} ROIs, P={P}, M={M}, C={C}, m={m}; median of {a.runs} after "
             f"{a.warmup} warm-up (HIP events around {a.inner} launches, ms per launch); bytes = what the kernel reads + "
             f"writes",
             f"device: {torch.cuda.get_device_name(0)}",
             f"{'form':10s} {'MB':>8s} {'kernel':>9s} {'min':>9s} {'TB/s':>7s} {'copy':>9s} {'TB/s':>7s} {'k/copy':>7s} "
             f"{'torch':>9s} {'torch/k':>8s}"]
    for k, (_, _, nbytes) in forms.items():
        t, c, e = med[k], med[k + ":copy"], med[k + ":torch"]
        lines.append(f"{k:10s} {nbytes / 1e6:8.1f} {t:9.4f} {min(ms[k]):9.4f} {tbs(nbytes, t):7.3f} {c:9.4f} "
                     f"{tbs(nbytes, c):7.3f} {t / c:7.2f} {e:9.4f} {e / t:8.2f}")
    for k, t in fills.items():
        nb = 4 * t.numel()
        lines.append(f"{k}: a memset of its {nb / 1e6:.1f} MB output alone takes {med[k + ':fill']:.4f} ms "
                     f"({tbs(nb, med[k + ':fill']):.3f} TB/s written); kernel / memset = {med[k] / med[k + ':fill']:.2f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
