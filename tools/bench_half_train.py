#!/usr/bin/env python3
"""tools/bench_half_train.py [--steps S] [--warmup W] [--train-steps T] [--no-train] -- what fp16 slabs gain in TRAINING.

Prints one JSON line:
  march: C2 (80 cameras, 512^2, K = 4096; bench.py's scene, seed 1112, rays made inside the march) forward and backward ms
         (HIP events around the C-ABI launches, averaged over S steps) with fp32 slabs (mvpraymarch_from_cameras) and with
         fp16 slabs (halfslab.mvpraymarch_half_from_cameras, the shadow made once outside the timing, as the training loop's
         decoder makes it alongside the fp32 slabs); plus the shadow's own cost (template_to_half at C2).
  train: the `train` leg of bench.py (C2 frames per GPU, eager Trainer, no background MLP) in iterations/s, with and without
         RaymarchTrainModel(half_slabs=True)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _events_ms(fn, steps, warmup):
    """Average ms per step of each timed C-ABI launch name (ava-256_amd/_hooks.timed)."""
    from ava256_amd import _hooks
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = []
    _hooks.set_event_sink(ev)
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    _hooks.set_event_sink(None)
    out = {}
    for name, a, b in ev:
        out[name] = out.get(name, 0.0) + a.elapsed_time(b) / steps
    return out


def march_leg(steps, warmup):
    import ava256_amd as ops
    from ava256_amd import halfslab
    from ava256_amd.scene import make_scene
    dev = "cuda"
    s = make_scene(80, 512, 512, 4096, device=dev, seed=1112)
    names = ("primpos", "primrot", "primscale", "template")
    for k in names:
        s[k].requires_grad_(True)
    gout = torch.randn(80, 512, 512, 4, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    cams = (s["campos"], s["camrot"], s["focal"], s["princpt"], s["pixelcoords"], s["volradius"], s["stepsize"])
    prim = (s["primpos"], s["primrot"], s["primscale"])
    th = halfslab.template_to_half(s["template"].detach())

    def fp32():
        for k in names:
            s[k].grad = None
        ops.mvpraymarch_from_cameras(*cams, prim, s["template"]).backward(gout)

    def fp16():
        for k in names:
            s[k].grad = None
        halfslab.mvpraymarch_half_from_cameras(*cams, prim, s["template"], th).backward(gout)

    a = _events_ms(fp32, steps, warmup)
    b = _events_ms(fp16, steps, warmup)
    c = _events_ms(lambda: halfslab.template_to_half(s["template"].detach()), steps, warmup)
    res = {"workload": "C2: 80 cameras, 512x512, K=4096 (bench.py scene, seed 1112)", "steps": steps,
           "fp32": {"forward_ms": a.get("march_forward", 0.0), "backward_ms": a.get("march_backward", 0.0)},
           "fp16": {"forward_ms": b.get("march_forward_half", 0.0), "backward_ms": b.get("march_backward_half", 0.0)},
           "shadow_template_to_half_ms": c.get("template_to_half", 0.0)}
    for r in (res["fp32"], res["fp16"]):
        r["ms_per_step"] = r["forward_ms"] + r["backward_ms"]
    del s, gout, th
    torch.cuda.empty_cache()
    return res


def train_leg(steps, warmup, half_slabs):
    import time
    from ava256_amd.trainloop import (CodeEncoderStandIn, ColorCalStandIn, RaymarchTrainModel, SlabDecoderStandIn, Trainer,
                                      make_training_batch)
    dev = "cuda"
    N, H, W, K, slab = 80, 512, 512, 4096, 8       # bench.py WORKLOADS["C2"]
    batch, volradius = make_training_batch(N, H, W, K, dev, seed=1112, ncams=80, nident=4,
                                           target_decoder=SlabDecoderStandIn(K, slab, seed=9))
    model = RaymarchTrainModel(SlabDecoderStandIn(K, slab, seed=1), volradius, colorcal=ColorCalStandIn(80, 4),
                               encoder=CodeEncoderStandIn(), half_slabs=half_slabs).to(dev)
    tr = Trainer(model)
    loss = None
    for _ in range(warmup):
        loss, _ = tr.step(batch)
    kms = _events_ms(lambda: tr.step(batch), 1, 0)   # one instrumented iteration: which C-ABI launches, ms each
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss, _ = tr.step(batch)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    out = {"iters_per_s": steps / el, "ms_per_iter": 1e3 * el / steps, "final_loss": float(loss), "steps": steps,
           "kernel_ms": {k: round(v, 4) for k, v in sorted(kms.items())}}
    del tr, model, batch
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--train-steps", type=int, default=10)
    ap.add_argument("--no-train", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    out = {"march": march_leg(args.steps, args.warmup)}
    m = out["march"]
    m["speedup"] = {k: m["fp32"][k] / m["fp16"][k] if m["fp16"][k] > 0 else None
                    for k in ("forward_ms", "backward_ms", "ms_per_step")}
    if not args.no_train:
        out["train"] = {"workload": "C2: 80 frames/GPU, 512x512, K=4096, eager Trainer, no background MLP",
                        "fp32_slabs": train_leg(args.train_steps, args.warmup, False),
                        "half_slabs": train_leg(args.train_steps, args.warmup, True)}
        t = out["train"]
        t["speedup"] = t["half_slabs"]["iters_per_s"] / t["fp32_slabs"]["iters_per_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
