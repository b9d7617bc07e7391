"""Float32-vs-float64 error of the head-training restatement
(tests/headtrain_ref.py) on the CPU, at the shapes of tests/test_gpu_bn_train.py
and tests/test_gpu_head_train.py: the figures their tolerance tables quote (each
bar is 10x the worst figure of its quantity).  CPU only; prints one line per
case and the worst per quantity.

  python scripts/measure_headtrain_f32.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "3d-mask-r-cnn_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import headtrain_ref as HT  # noqa: E402
import test_gpu_bn_train as TB  # noqa: E402
import test_gpu_head_train as TH  # noqa: E402


def worst(acc, errs):
    for k, v in errs.items():
        acc[k] = max(acc.get(k, 0.0), v)


def main():
    bn = {}
    for M, C, relu in TB.CASES:
        c = TB.case(M, C, relu)
        r64, r32 = TB.reference(c, relu), TB.reference(c, relu, torch.float32)
        errs = {k: TB.rel(r32[k], r64[k]) for k in TB.QUANTITIES}
        worst(bn.setdefault((M, C), {}), errs)
    for shape, errs in bn.items():
        print(f"    {shape}: (" + ", ".join(f"{errs[k]:.2e}" for k in TB.QUANTITIES) + "),")
    head = {}
    for name in TH.CASES:
        r = TH.reference(name)
        c = TH.to64(TH.case(name), torch.float32)
        total, lc, lb, grads, d_pooled, outs, aux = HT.loss_and_grads(c["p"], c["pooled"], c["ids"], c["tbox"],
                                                                      c["active"], c["nc"])
        g, b = TH.grad_errors(grads, r)
        errs = {"loss": max(abs(float(a) - float(b_)) / max(1.0, abs(float(b_)))
                            for a, b_ in ((total, r["total"]), (lc, r["lc"]), (lb, r["lb"]))),
                "grad": g, "bias": b, "d_pooled": TH.rel(d_pooled, r["d_pooled"]),
                "fwd": max(TH.rel(a, b_) for a, b_ in zip(outs, r["outs"]))}
        print(f"head {name} margins={TH.margins(r['aux'])} " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
        worst(head, errs)
    for opt in TH.OPTIMIZERS:
        traj, q, moving = TH.steps_reference(opt)
        c = TH.to64(TH.case("small5", 10.0, TH.STEPS_SEED), torch.float32)
        t32, q32, m32 = HT.train_steps(c["p"], c["moving"], c["pooled"], c["ids"], c["tbox"], c["active"], c["nc"],
                                       TH.STEPS, TH.OPTIMIZERS[opt][1], weight_decay=TH.WEIGHT_DECAY)
        errs = {"s_loss": float((np.abs(t32[:, :3] - traj[:, :3]) / np.maximum(1.0, np.abs(traj[:, :3]))).max()),
                "s_param": max(TH.rel(q32[k], q[k]) for k in HT.PARAM_NAMES),
                "s_moving": max(max(TH.rel(m32[k][0], moving[k][0]), TH.rel(m32[k][1], moving[k][1])) for k in moving),
                "s_norm": max(TH.rel(q32[k].norm(dim=0), q[k].norm(dim=0)) for k in HT.MAX_NORM)}
        print(f"steps {opt} min margin={traj[:, 3].min():.2e} losses={traj[:, 0]} " +
              " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
        print(f"    \"{opt}\": {{" + ", ".join(f'"{k}": {v:.2e}' for k, v in errs.items()) + "},")
    print("head worst:", {k: f"{v:.2e}" for k, v in head.items()})


if __name__ == "__main__":
    main()
