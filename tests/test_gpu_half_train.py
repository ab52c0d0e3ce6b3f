"""GPU tests of training over fp16 slabs (ava-256_amd/halfslab.py: mvpraymarch_half*, assemble_template_frames_half;
trainloop.RaymarchTrainModel(half_slabs=True)).

The sharp test: widening fp16 -> fp32 is exact and every fp16 sampler sums in the fp32 sampler's corner order, so
mvpraymarch_half(template=T, template_half=th) must give what mvpraymarch(template=th.float()) gives -- rayrgba, raysat and
the slab gradient of the primitive-centric backward (integer fixed-point sums: order-free) bit for bit.  Gradients the fp32
path itself sums in a run-dependent order (the pose gradients' fp32 sums, and every gradient of the ray-centric kernel's
global fp32 atomics) are held to the round-off bound the fp32 path's own tests use between two runs."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import FragileRays, npf, scene_rays, to_dev
from test_gpu_parity import BACKWARD_MODES, FWD_TOL, _check_grads, ops  # noqa: F401  (ops is a fixture)

pytestmark = pytest.mark.gpu

DBG_LIB = os.path.join(ROOT, "build_variants", "libmvp_dbg.so")
ORDER_TOL = 1e-4   # fp32 sums in another order: of the largest gradient (test_gpu_hardening's bound between two sweeps)
NAMES = ("primpos", "primrot", "primscale", "template")


def _scene(N, H, W, K, again, seed):
    from ava256_amd.scene import make_scene
    return make_scene(N, H, W, K, device="cuda", seed=seed, alpha_gain=again)


def _run(ops_mod, s, th, gout, mode, half, cams=False, retain=False):
    """One forward + backward through the fp16 operator (half=True: template = the fp32 master, template_half = th) or the
    fp32 operator on th.float().  Returns (rgba, raysat, grads)."""
    from ava256_amd import _hooks, halfslab
    handoff = _hooks.patched_handoff(cap=4 if mode == "cap4" else None, ray_centric=(mode == "ray"))
    t = {k: s[k].detach().clone().requires_grad_(True) for k in NAMES[:3]}
    t["template"] = (s["template"] if half else th.float()).detach().clone().requires_grad_(True)
    prim = (t["primpos"], t["primrot"], t["primscale"])
    _hooks.keep_raysat = True
    try:
        with handoff:
            if cams:
                c = (s["campos"], s["camrot"], s["focal"], s["princpt"], s["pixelcoords"], s["volradius"], s["stepsize"])
                rgba = (halfslab.mvpraymarch_half_from_cameras(*c, prim, t["template"], th) if half else
                        ops_mod.mvpraymarch_from_cameras(*c, prim, t["template"]))
            else:
                rp, rd, tm = ops_mod.compute_raydirs(s["campos"], s["camrot"], s["focal"], s["princpt"], s["pixelcoords"],
                                                     s["volradius"])
                rgba = (halfslab.mvpraymarch_half(rp, rd, s["stepsize"], tm, prim, t["template"], th) if half else
                        ops_mod.mvpraymarch(rp, rd, s["stepsize"], tm, prim, t["template"], None))
        sat = _hooks.last_raysat
    finally:
        _hooks.keep_raysat = False
        _hooks.last_raysat = _hooks.last_pl_count = None
    rgba.backward(gout, retain_graph=retain)
    torch.cuda.synchronize()
    grads = {k: t[k].grad for k in NAMES}
    assert grads["template"].dtype == torch.float32
    if retain:
        return rgba, sat, grads, t
    return rgba, sat, grads


def _assert_same_grads(g16, g32, mode, what):
    # the primitive-centric slab gradient is an integer sum: bit for bit
    if mode == "prim":
        assert torch.equal(g16["template"], g32["template"]), what
    for k in NAMES:
        a, b = g16[k], g32[k]
        assert torch.equal(torch.isfinite(a), torch.isfinite(b)), (what, k)
        fin = torch.isfinite(b)
        scale = float(b[fin].abs().max()) if bool(fin.any()) else 0.0
        assert float((a[fin] - b[fin]).abs().max()) <= ORDER_TOL * scale, (what, k)


def _both_sweeps(fn, slot):
    """fn() with the product library (lane-independent sweep where it applies) or with the debug build forcing the
    slot-synchronous sweep (as test_gpu_hardening.py::test_lane_independent_sweep_equals_slot_synchronous_sweep)."""
    from ava256_amd import _lib
    if not slot:
        return fn()
    if not os.path.exists(DBG_LIB):
        pytest.skip("build_variants/libmvp_dbg.so not built (__graft_entry__.build())")
    os.environ["MVP_DEBUG_SLOT_SWEEP"] = "1"
    _lib.use_library(DBG_LIB)
    try:
        return fn()
    finally:
        del os.environ["MVP_DEBUG_SLOT_SWEEP"]
        _lib.use_library(None)


@pytest.mark.parametrize("slot", [False, True], ids=["lane_sweep", "slot_sweep"])
@pytest.mark.parametrize("again", [1.0, 40.0], ids=["a1", "saturated_a40"])
@pytest.mark.parametrize("mode", BACKWARD_MODES)
def test_half_operator_equals_fp32_operator_on_the_widened_slabs(ops, mode, again, slot):
    from ava256_amd import halfslab
    s = _scene(2, 96, 104, 512, again, seed=301)
    th = halfslab.template_to_half(s["template"])
    gout = torch.randn(2, 96, 104, 4, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))

    def both():
        return _run(ops, s, th, gout, mode, True), _run(ops, s, th, gout, mode, False)
    (r16, s16, g16), (r32, s32, g32) = _both_sweeps(both, slot)
    assert float(r32[..., 3].max()) > 0.05
    assert torch.equal(r16, r32)
    assert torch.equal(s16, s32)
    _assert_same_grads(g16, g32, mode, (mode, again, slot))


@pytest.mark.parametrize("again", [1.0, 40.0], ids=["a1", "saturated_a40"])
@pytest.mark.parametrize("mode", BACKWARD_MODES)
def test_camera_form_equals_fp32_operator_on_the_widened_slabs(ops, mode, again):
    from ava256_amd import halfslab
    s = _scene(2, 80, 72, 1024, again, seed=302)
    th = halfslab.template_to_half(s["template"])
    gout = torch.randn(2, 80, 72, 4, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))
    r16, s16, g16 = _run(ops, s, th, gout, mode, True, cams=True)
    r32, s32, g32 = _run(ops, s, th, gout, mode, False, cams=True)
    assert torch.equal(r16, r32) and torch.equal(s16, s32)
    _assert_same_grads(g16, g32, mode, (mode, again))
    # ... and the ray form over the same widened slabs: the camera form makes the same rays
    r16b, _, _ = _run(ops, s, th, gout, mode, True, cams=False)
    assert torch.equal(r16, r16b)


@pytest.mark.parametrize("mode", BACKWARD_MODES)
def test_half_operator_matches_the_oracle_on_the_rounded_slabs(ops, oracle64, mode):
    from ava256_amd import _hooks, halfslab
    from ava256_amd.scene import make_scene
    s = make_scene(2, 64, 56, 256, device="cpu", seed=263, alpha_gain=6.0)
    tr = s["template"].half().float()               # the rounded slabs the oracle marches
    rp, rd, tm = scene_rays(oracle64, s)
    a = (rp, rd, s["stepsize"], tm, s["primpos"].numpy(), s["primrot"].numpy(), s["primscale"].numpy(), tr.numpy())
    ref_rgba, ref_sat, st = oracle64.march_forward(*a, ray_diagnostics=True)
    assert st["rays_hit"] > 0
    gout = np.random.default_rng(4).normal(size=ref_rgba.shape)
    fragile = FragileRays(ref_sat, st["margin"], gout, nsamples=st["nsamples"])
    t = {k: to_dev(s[k].numpy()).requires_grad_(True) for k in NAMES}
    th = halfslab.template_to_half(t["template"].detach())
    assert torch.equal(th.float().cpu(), tr)
    _hooks.keep_raysat = True
    try:
        with _hooks.patched_handoff(cap=4 if mode == "cap4" else None, ray_centric=(mode == "ray")):
            rgba = halfslab.mvpraymarch_half(to_dev(rp), to_dev(rd), float(s["stepsize"]), to_dev(tm),
                                             (t["primpos"], t["primrot"], t["primscale"]), t["template"], th)
        g = fragile(npf(_hooks.last_raysat))
    finally:
        _hooks.keep_raysat = False
        _hooks.last_raysat = _hooks.last_pl_count = None
    rgba.backward(to_dev(g))
    torch.cuda.synchronize()
    fr = fragile.mask
    rgp, rgr, rgs, rgt = oracle64.march_backward(*a, ref_sat, fragile.masked())
    out = npf(rgba)
    err = np.abs(out - ref_rgba).max(-1)
    assert (err[~fr] > FWD_TOL * max(1.0, np.abs(ref_rgba).max())).sum() == 0, err[~fr].max()
    mine = {k: npf(t[k].grad) for k in NAMES}
    _check_grads(mine, dict(template=rgt, primpos=rgp, primrot=rgr, primscale=rgs), mode)


@pytest.mark.parametrize("case", ["overflow_inf", "nan_voxel"])
@pytest.mark.parametrize("mode", BACKWARD_MODES)
def test_non_finite_slabs_poison_what_the_fp32_path_poisons(ops, mode, case):
    """Slabs that overflow fp16 (|x| > 65504 -> +-Inf) or carry NaN: the fp16 operator gives what the fp32 operator gives on
    the widened slabs -- the same rgba bits (NaN where NaN), the same non-finite gradient entries, the rest within round-off."""
    from ava256_amd import halfslab
    s = _scene(1, 64, 64, 256, 4.0, seed=303)
    tpl = s["template"].clone()
    if case == "overflow_inf":
        tpl[0, 40:48, 3, 4, 4, 0] = 1e5
        tpl[0, 50, 2, 3, 4, 3] = -1e6
    else:
        tpl[0, 40:44, 4, 4, 4, 1] = float("nan")
        tpl[0, 60, 3, 3, 3, 3] = float("nan")
    s["template"] = tpl
    th = halfslab.template_to_half(tpl)
    assert not bool(torch.isfinite(th).all())
    gout = torch.randn(1, 64, 64, 4, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
    r16, s16, g16 = _run(ops, s, th, gout, mode, True)
    r32, s32, g32 = _run(ops, s, th, gout, mode, False)
    assert torch.equal(torch.isnan(r16), torch.isnan(r32))
    assert bool((r16 == r32)[~torch.isnan(r32)].all())
    for k in NAMES:
        a, b = g16[k], g32[k]
        assert torch.equal(torch.isnan(a), torch.isnan(b)), (k, case, mode)
        assert torch.equal(torch.isinf(a), torch.isinf(b)), (k, case, mode)
        fin = torch.isfinite(b)
        if bool(fin.any()):
            assert float((a[fin] - b[fin]).abs().max()) <= ORDER_TOL * float(b[fin].abs().max()), (k, case, mode)


def test_backward_twice_over_one_forward(ops):
    from ava256_amd import halfslab
    s = _scene(2, 64, 64, 256, 4.0, seed=304)
    th = halfslab.template_to_half(s["template"])
    gout = 1e-3 * torch.randn(2, 64, 64, 4, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    rgba, _, g1, t = _run(ops, s, th, gout, "prim", True, retain=True)
    first = {k: v.clone() for k, v in g1.items()}
    for v in t.values():
        v.grad = None
    rgba.backward(gout)
    torch.cuda.synchronize()
    assert torch.equal(t["template"].grad, first["template"])
    for k in NAMES[:3]:
        assert float((t[k].grad - first[k]).abs().max()) <= ORDER_TOL * float(first[k].abs().max()), k


def test_assemble_frames_half_equals_assemble_frames_then_round(ops):
    from ava256_amd.assemble import assemble_template_frames
    from ava256_amd.halfslab import assemble_template_frames_half
    g = torch.Generator(device="cuda").manual_seed(3)
    B, nh = 8, 16
    tex = 30.0 * torch.randn(1, 3 * B, nh * B, nh * B, device="cuda", generator=g)
    tex[0, 0, :4, :4] = 3000.0                      # relu(x * 25 + 100) beyond 65504: +inf in fp16, as the cast
    op = torch.randn(1, B, nh * B, nh * B, device="cuda", generator=g)
    gain = 1.0 + 0.1 * torch.randn(5, device="cuda", generator=g)
    with torch.no_grad():
        full = assemble_template_frames(tex, op, gain, nh * nh, B)
    half = assemble_template_frames_half(tex, op, gain, nh * nh, B)
    assert half.dtype == torch.float16 and half.shape == full.shape
    assert torch.equal(half, full.half())
    assert bool(torch.isinf(half).any())


def _train_setup(half, N=2, H=64, W=64, K=256):
    from ava256_amd.trainloop import (CodeEncoderStandIn, ColorCalStandIn, RaymarchTrainModel, SlabDecoderStandIn,
                                      make_training_batch)
    batch, volradius = make_training_batch(N, H, W, K, "cuda", seed=5, target_decoder=SlabDecoderStandIn(K, seed=9))
    torch.manual_seed(0)
    model = RaymarchTrainModel(SlabDecoderStandIn(K, seed=1), volradius, colorcal=ColorCalStandIn(80, 4),
                               encoder=CodeEncoderStandIn(), half_slabs=half).to("cuda")
    return model, batch


def test_one_training_iteration_with_half_slabs(ops):
    from ava256_amd import halfslab
    from ava256_amd.trainloop import Trainer
    from ava256_amd import _hooks
    model, batch = _train_setup(True)
    tr = Trainer(model, lr=1e-3)
    ev = []
    _hooks.set_event_sink(ev)
    try:
        loss, _ = tr.step(batch)
    finally:
        _hooks.set_event_sink(None)
    names = {e[0] for e in ev}
    assert {"march_forward_half", "march_backward_half", "assemble_frames_half"} <= names, names   # the fp16 path ran
    assert "march_forward" not in names and "template_to_half" not in names, names
    assert np.isfinite(float(loss))
    assert all(bool(torch.isfinite(p).all()) for p in tr.params)
    # the decoder's fp16 shadow is its fp32 slabs rounded, and the march's gradients through it are the fp32 path's on the
    # widened shadow
    dec = model.decoder
    with torch.no_grad():
        code = batch["code"] if "code" in batch else torch.randn(2, 16, device="cuda")
        out = dec(code)
    th = out["template_half"]
    assert torch.equal(th, out["template"].half())
    s = {"primpos": out["primpos"], "primrot": out["primrot"], "primscale": out["primscale"], "template": out["template"]}
    for k in ("campos", "camrot", "focal", "princpt"):
        s[k] = batch[k].contiguous()
    s["pixelcoords"] = batch["pixelcoords"]
    s["volradius"], s["stepsize"] = model.raymarcher.volume_radius, model.raymarcher.dt
    N, H, W = s["campos"].shape[0], 64, 64
    gout = torch.randn(N, H, W, 4, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    r16, _, g16 = _run(ops, s, th, gout, "prim", True, cams=True)
    r32, _, g32 = _run(ops, s, th, gout, "prim", False, cams=True)
    assert torch.equal(r16, r32)
    _assert_same_grads(g16, g32, "prim", "train")
    assert torch.equal(halfslab.template_to_half(out["template"]), th)


def test_graph_replay_with_half_slabs_trains_like_the_eager_loop(ops):
    """Trainer(graph=True) captures the half-slab iteration (no host synchronisation in the new operators) and replays it."""
    from ava256_amd.trainloop import Trainer

    def run(graph):
        model, batch = _train_setup(True)
        tr = Trainer(model, lr=1e-3, graph=graph, graph_warmup=2)
        return tr, [float(tr.step(batch)[0]) for _ in range(6)]
    te, le = run(False)
    tg, lg = run(True)
    assert tg.graph and tg.graph_replays == 4
    for a, b in zip(le, lg):
        assert np.isfinite(b) and abs(a - b) <= 1e-4 * abs(a), (le, lg)


def test_full_c2_batch_in_one_launch(ops):
    from ava256_amd import halfslab
    s = _scene(80, 512, 512, 4096, 1.0, seed=1112)
    th = halfslab.template_to_half(s["template"])
    t = {k: s[k].requires_grad_(True) for k in NAMES}
    rgba = halfslab.mvpraymarch_half_from_cameras(s["campos"], s["camrot"], s["focal"], s["princpt"], s["pixelcoords"],
                                                  s["volradius"], s["stepsize"], (t["primpos"], t["primrot"], t["primscale"]),
                                                  t["template"], th)
    assert bool(torch.isfinite(rgba).all()) and float(rgba[..., 3].max()) > 0.05
    rgba.backward(torch.randn_like(rgba))
    torch.cuda.synchronize()
    for k in NAMES:
        assert bool(torch.isfinite(t[k].grad).all()), k
    assert float(t["template"].grad.abs().max()) > 0
