#!/usr/bin/env python3
"""tools/bench_depth.py [--steps S] [--warmup W] [--rounds R] -- what the expected-depth channel costs.

Prints one JSON line: C2 (80 cameras, 512^2, K = 4096; bench.py's scene, seed 1112; rays made once by compute_raydirs, outside
the timing) forward and backward ms (HIP events around the C-ABI launches, averaged over S steps) of mvpraymarch and of
mvpraymarch_depth, with the same upstream gradient of rayrgba and, for the depth operator, an upstream gradient of raydepth.
The two operators are timed in R alternating rounds; each figure is the best round's average (drift between rounds shows in
`rounds`)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    import ava256_amd as ops
    from ava256_amd.scene import make_scene
    dev = "cuda"
    s = make_scene(80, 512, 512, 4096, device=dev, seed=1112)
    names = ("primpos", "primrot", "primscale", "template")
    for k in names:
        s[k].requires_grad_(True)
    rp, rd, tm = ops.compute_raydirs(s["campos"], s["camrot"], s["focal"], s["princpt"], s["pixelcoords"], s["volradius"])
    gen = torch.Generator(device=dev).manual_seed(5)
    g_rgba = torch.randn(80, 512, 512, 4, device=dev, generator=gen)
    g_d = torch.randn(80, 512, 512, device=dev, generator=gen)
    prim = (s["primpos"], s["primrot"], s["primscale"])

    def plain():
        for k in names:
            s[k].grad = None
        ops.mvpraymarch(rp, rd, s["stepsize"], tm, prim, s["template"], None).backward(g_rgba)

    def depth():
        for k in names:
            s[k].grad = None
        rgba, d = ops.mvpraymarch_depth(rp, rd, s["stepsize"], tm, prim, s["template"], None)
        torch.autograd.backward([rgba, d], [g_rgba, g_d])

    rounds = []
    for _ in range(args.rounds):
        a = _events_ms(plain, args.steps, args.warmup)
        b = _events_ms(depth, args.steps, args.warmup)
        rounds.append({"mvpraymarch": {"forward_ms": a.get("march_forward", 0.0), "backward_ms": a.get("march_backward", 0.0)},
                       "mvpraymarch_depth": {"forward_ms": b.get("march_forward", 0.0),
                                             "backward_ms": b.get("march_backward", 0.0)}})
    res = {"workload": "C2: 80 cameras, 512x512, K=4096 (bench.py scene, seed 1112)", "steps": args.steps,
           "rounds": rounds}
    for op in ("mvpraymarch", "mvpraymarch_depth"):
        res[op] = {k: min(r[op][k] for r in rounds) for k in ("forward_ms", "backward_ms")}
    res["depth_cost"] = {k: res["mvpraymarch_depth"][k] / res["mvpraymarch"][k] - 1.0 for k in ("forward_ms", "backward_ms")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
