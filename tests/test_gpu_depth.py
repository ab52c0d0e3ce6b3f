"""GPU tests of the expected-depth channel (ava-256_amd/mvpraymarch.py: mvpraymarch_depth; Raymarcher(with_pos_img=True)).

Ground truth comes from an exact construction, with the float64 oracle unchanged.  Trilinear interpolation reproduces a
linear field exactly and the fade scales opacity only, so in a scene S' made from S by writing into every RGB voxel its own
world position (plus a constant c, the inverse of the march's PrimTransfSRT map: x = pos + R (y / scale)), the oracle's colour
is sum_i contrib_i * (x_i + c) = pos_img(S) + c * alpha.  With opacity unchanged, S and S' composite with the same weights.

Gradients of the loss <g_rgba, rayrgba> + <g_d, raydepth>: depth = (d . (rgb' - (o + c) alpha)) / |d|^2 on S', so the depth
term is the oracle's backward on S' under the upstream (g_d d / |d|^2 in RGB, -g_d d.(o + c) / |d|^2 in alpha), plus -- for the
pose -- the chain through the construction of S' (linear in the voxel positions, written in torch float64).  The colour term
is the oracle's backward on S under g_rgba."""
import numpy as np
import pytest
import torch

from helpers import EDGE_JUMP, SAT_BAND, FragileRays, cosine, npf, scene_rays, to_dev
from test_gpu_half_train import ORDER_TOL, _both_sweeps
from test_gpu_parity import BACKWARD_MODES, FWD_TOL, GT_TOL, POSE_COS, POSE_TOL, ops  # noqa: F401  (ops is a fixture)

pytestmark = pytest.mark.gpu

NAMES = ("primpos", "primrot", "primscale", "template")
OFFSET = 4.0  # c: keeps every S' colour above -1, so that the oracle's raysat test (primaccum.h:93) sees every saturated ray


def _voxel_positions(primpos, primrot, primscale, shape):
    """World position of every voxel centre of every slab, [N,K,TD,TH,TW,3] (torch; differentiable in the pose)."""
    TD, TH, TW = shape
    dt_ = primpos.dtype
    lin = [torch.linspace(-1.0, 1.0, n, dtype=dt_) for n in (TD, TH, TW)]
    z, y, x = torch.meshgrid(*lin, indexing="ij")
    yv = torch.stack([x, y, z], -1)                                   # box coordinate (x, y, z) of voxel (z, y, x)
    q = yv[None, None] / primscale[:, :, None, None, None, :]         # R^T (x - pos) = y / scale (rows of R: primrot[i])
    rit = torch.linalg.inv(primrot.transpose(-1, -2))                 # (R^T)^-1: no orthonormality assumed
    return primpos[:, :, None, None, None, :] + torch.einsum("nkij,nkdhwj->nkdhwi", rit, q)


def _scene_prime(a):
    """S' of the arrays a = (raypos, raydir, stepsize, tminmax, primpos, primrot, primscale, template)."""
    pp, pr, ps, tpl = (torch.as_tensor(np.asarray(v, np.float64)) for v in a[4:8])
    X = _voxel_positions(pp, pr, ps, tpl.shape[2:5]).numpy()
    t2 = np.asarray(a[7], np.float64).copy()
    t2[..., :3] = X + OFFSET
    return a[:7] + (t2,)


def _chain_pose(a, g_rgb):
    """Pose gradient through S' construction: sum over voxels of g_rgb . dX/d(pose)."""
    pp, pr, ps = (torch.as_tensor(np.asarray(v, np.float64)).requires_grad_(True) for v in a[4:7])
    X = _voxel_positions(pp, pr, ps, np.asarray(a[7]).shape[2:5])
    gp, gr, gs = torch.autograd.grad(X, (pp, pr, ps), grad_outputs=torch.as_tensor(g_rgb))
    return gp.numpy(), gr.numpy(), gs.numpy()


def _run_depth(ops_mod, a, fadescale, fadeexp, gout=None, mode="prim", op="depth", grad_mode=None):
    """mvpraymarch_depth (op='depth') or mvpraymarch (op='plain') through the public operator.  gout: None (forward only),
    an array [N,H,W,5] (g_rgba | g_d) or a callable(raysat) -> that array.  grad_mode (default: gout given) runs the forward
    in grad mode, which writes raysat.  Returns dict(rgba, depth, raysat, grads, two_pass)."""
    from ava256_amd import _hooks
    grad_mode = gout is not None if grad_mode is None else grad_mode
    t = {k: to_dev(v) for k, v in zip(("raypos", "raydir", "tminmax"), (a[0], a[1], a[3]))}
    for k, v in zip(NAMES, (a[4], a[5], a[6], a[7])):
        t[k] = to_dev(v).requires_grad_(grad_mode)
    prim = (t["primpos"], t["primrot"], t["primscale"])
    _hooks.keep_raysat = True
    try:
        with torch.set_grad_enabled(grad_mode), \
                _hooks.patched_handoff(cap=4 if mode == "cap4" else None, ray_centric=(mode == "ray")):
            if op == "depth":
                rgba, depth = ops_mod.mvpraymarch_depth(t["raypos"], t["raydir"], float(a[2]), t["tminmax"], prim,
                                                        t["template"], None, fadescale=fadescale, fadeexp=fadeexp)
            else:
                rgba = ops_mod.mvpraymarch(t["raypos"], t["raydir"], float(a[2]), t["tminmax"], prim, t["template"], None,
                                           fadescale=fadescale, fadeexp=fadeexp)
                depth = None
        raysat = _hooks.last_raysat
        pl = _hooks.last_pl_count
        out = dict(rgba=rgba.detach(), depth=None if depth is None else depth.detach(),
                   raysat=None if raysat is None else raysat.clone())
        if gout is not None:
            g = gout(npf(raysat)) if callable(gout) else gout
            g = to_dev(g)
            if op == "depth":
                torch.autograd.backward([rgba, depth], [g[..., :4].contiguous(), g[..., 4].contiguous()])
            else:
                rgba.backward(g[..., :4].contiguous())
            torch.cuda.synchronize()
            out["grads"] = {k: t[k].grad.detach().clone() for k in NAMES}
            if pl is not None:
                NK = a[4].shape[0] * a[4].shape[1]
                out["two_pass"] = int((((pl[:NK].to(torch.int64) & 0xffffffff) >> 30) & 1).sum())
    finally:
        _hooks.keep_raysat = False
        _hooks.last_raysat = _hooks.last_pl_count = None
    return out


def _make(N, H, W, K, again, slab, seed, oracle64, shape=None, scale_mul=1.0):
    from ava256_amd.scene import make_scene
    s = make_scene(N, H, W, K, device="cpu", seed=seed, alpha_gain=again, slab=slab)
    s["primscale"] = s["primscale"] * scale_mul
    tpl = s["template"].numpy()
    if shape is not None:  # non-cubic slabs
        rng = np.random.default_rng(seed)
        TD, TH, TW = shape
        tpl = np.concatenate([np.maximum(100 + 25 * rng.normal(size=(N, K, TD, TH, TW, 3)), 0),
                              again * np.exp(0.1 * rng.normal(size=(N, K, TD, TH, TW, 1)))], axis=-1).astype(np.float32)
    rp, rd, tm = scene_rays(oracle64, s)
    return (rp, rd, s["stepsize"], tm, s["primpos"].numpy(), s["primrot"].numpy(), s["primscale"].numpy(), tpl)


def _not_borderline(st):
    """Rays the float64 oracle does not call borderline (helpers.FragileRays): saturation margin >= SAT_BAND and no inclusion
    decision within round-off of flipping with more than EDGE_JUMP of opacity at stake.  Only those must agree in the forward."""
    return (st["margin"] >= SAT_BAND) & (st["edge"] <= EDGE_JUMP)


def _pos_img(a, rgba, depth):
    """raypos * alpha + raydir * raydepth, [N,H,W,3] (numpy float64)."""
    return np.asarray(a[0], np.float64) * rgba[..., 3:4] + np.asarray(a[1], np.float64) * depth[..., None]


FWD_SCENES = [
    # id, (N, H, W, K, alpha_gain, slab, seed, shape, scale_mul, fadescale, fadeexp)
    ("random", (2, 48, 40, 256, 1.0, 8, 11, None, 1.0, 8.0, 8.0)),
    ("random_a6", (1, 56, 56, 512, 6.0, 8, 12, None, 1.0, 8.0, 8.0)),
    ("saturated_a40", (1, 50, 37, 512, 40.0, 8, 13, None, 1.0, 8.0, 8.0)),
    ("noncubic_fade", (2, 40, 48, 96, 3.0, 4, 31, (4, 6, 5), 0.7, 5.0, 6.0)),
    ("K37", (2, 40, 40, 37, 8.0, 8, 44, None, 0.5, 8.0, 8.0)),
]


@pytest.mark.parametrize("slot", [False, True], ids=["lane_sweep", "slot_sweep"])
@pytest.mark.parametrize("name,cfg", FWD_SCENES, ids=[n for n, _ in FWD_SCENES])
def test_forward_pos_img_matches_oracle(ops, oracle64, name, cfg, slot):
    N, H, W, K, again, slab, seed, shape, smul, fs, fe = cfg
    a = _make(N, H, W, K, again, slab, seed, oracle64, shape, smul)
    _, _, st = oracle64.march_forward(*a, fadescale=fs, fadeexp=fe, ray_diagnostics=True)
    assert st["rays_hit"] > 0 and st["list_overflow"] == 0
    ref2, _, _ = oracle64.march_forward(*_scene_prime(a), fadescale=fs, fadeexp=fe)
    ref_pos = ref2[..., :3] - OFFSET * ref2[..., 3:4]
    ok = _not_borderline(st)
    assert ok.mean() > 0.95, ok.mean()
    out = _both_sweeps(lambda: _run_depth(ops, a, fs, fe), slot)
    rgba, depth = npf(out["rgba"]), npf(out["depth"])
    pos = _pos_img(a, rgba, depth)
    scale = max(1.0, np.abs(ref2).max())
    err = np.abs(pos - ref_pos).max(-1)
    assert (err[ok] > FWD_TOL * scale).sum() == 0, (name, err[ok].max(), scale)
    assert np.all(depth[rgba[..., 3] == 0] == 0)                 # 0 where the ray hits nothing
    assert float(np.abs(depth).max()) > 0


@pytest.mark.parametrize("slot", [False, True], ids=["lane_sweep", "slot_sweep"])
@pytest.mark.parametrize("mode", BACKWARD_MODES)
def test_rgba_and_raysat_are_bit_identical_to_mvpraymarch(ops, oracle64, mode, slot):
    a = _make(2, 48, 40, 256, 20.0, 8, 21, oracle64)

    def both():
        return (_run_depth(ops, a, 8.0, 8.0, mode=mode, grad_mode=True),
                _run_depth(ops, a, 8.0, 8.0, mode=mode, op="plain", grad_mode=True))
    d, p = _both_sweeps(both, slot)
    assert torch.equal(d["rgba"], p["rgba"])
    assert torch.equal(d["raysat"], p["raysat"])


def _reference_grads(oracle64, a, fs, fe, ref_sat, ref_sat2, g):
    """The float64 gradients of <g[...,:4], rayrgba> + <g[...,4], raydepth> (module docstring)."""
    rgp, rgr, rgs, rgt = oracle64.march_backward(*a, ref_sat, g[..., :4], fadescale=fs, fadeexp=fe)
    a2 = _scene_prime(a)
    o, d = np.asarray(a[0], np.float64), np.asarray(a[1], np.float64)
    gd = g[..., 4:5] / (d * d).sum(-1, keepdims=True)
    up = np.concatenate([gd * d, -gd * (d * (o + OFFSET)).sum(-1, keepdims=True)], -1)
    dp, dr, ds, dtp = oracle64.march_backward(*a2, ref_sat2, up, fadescale=fs, fadeexp=fe)
    cp, cr, cs = _chain_pose(a, dtp[..., :3])
    tmpl = rgt.copy()
    tmpl[..., 3] += dtp[..., 3]
    return dict(template=tmpl, primpos=rgp + dp + cp, primrot=rgr + dr + cr, primscale=rgs + ds + cs)


def _check(mine, ref, what):
    for k in NAMES:
        m, r = npf(mine[k]), ref[k]
        e = np.abs(m - r).max()
        if k == "template":
            assert e <= GT_TOL * np.abs(r).max(), (what, k, e, np.abs(r).max())
        else:
            c = cosine(m, r)
            assert c >= POSE_COS, (what, k, c)
            assert e <= POSE_TOL * np.abs(r).max(), (what, k, e, np.abs(r).max())


GRAD_CASES = [
    # id, g_rgba multiplier, g_d multiplier, heavy-tailed g_d (drives the two-pass instantiation)
    ("both", 1.0, 1.0, False),
    ("depth_only", 0.0, 1.0, False),
    ("depth_large", 1.0, 300.0, False),
    ("two_pass", 1.0, 1.0, True),
]


@pytest.mark.parametrize("mode", BACKWARD_MODES)
@pytest.mark.parametrize("case,grgba,gdep,heavy", GRAD_CASES, ids=[c[0] for c in GRAD_CASES])
def test_gradients_match_oracle(ops, oracle64, mode, case, grgba, gdep, heavy):
    fs, fe = 8.0, 8.0
    a = _make(2, 48, 40, 256, 6.0, 8, 51, oracle64)
    ref_rgba, ref_sat, st = oracle64.march_forward(*a, fadescale=fs, fadeexp=fe, ray_diagnostics=True)
    _, ref_sat2, _ = oracle64.march_forward(*_scene_prime(a), fadescale=fs, fadeexp=fe)
    rng = np.random.default_rng(5)
    g = rng.normal(size=ref_rgba.shape[:3] + (5,))
    g[..., :4] *= grgba
    g[..., 4] *= gdep
    if heavy:  # a few outlier rays of depth gradient, 1e4 above the rest: the dynamic-range test marks their primitives
        idx = rng.choice(np.flatnonzero(st["nsamples"].ravel() > 0), 6, replace=False)
        gd = g[..., 4].reshape(-1)
        gd[idx] *= 1.0e4
        g[..., 4] = gd.reshape(g.shape[:3])
    fragile = FragileRays(ref_sat, st["margin"], g, nsamples=st["nsamples"])
    out = _run_depth(ops, a, fs, fe, gout=fragile, mode=mode)
    ref = _reference_grads(oracle64, a, fs, fe, ref_sat, ref_sat2, fragile.masked())
    _check(out["grads"], ref, (case, mode))
    if heavy and mode == "prim":
        assert out["two_pass"] > 0, "the heavy-tailed depth gradient did not reach the two-pass instantiation"


@pytest.mark.parametrize("mode", BACKWARD_MODES)
def test_zero_depth_gradient_reduces_to_mvpraymarch(ops, oracle64, mode):
    a = _make(2, 48, 40, 256, 20.0, 8, 61, oracle64)
    g = np.random.default_rng(6).normal(size=(2, 48, 40, 5))
    g[..., 4] = 0.0
    d = _run_depth(ops, a, 8.0, 8.0, gout=g, mode=mode)
    p = _run_depth(ops, a, 8.0, 8.0, gout=g, mode=mode, op="plain")
    if mode == "prim":  # integer fixed-point sums: bit for bit
        assert torch.equal(d["grads"]["template"], p["grads"]["template"])
    for k in NAMES:
        x, y = d["grads"][k], p["grads"][k]
        assert float((x - y).abs().max()) <= ORDER_TOL * float(y.abs().max()), (mode, k)


def test_primitive_centric_slab_gradient_is_deterministic(ops, oracle64):
    a = _make(2, 48, 40, 256, 6.0, 8, 71, oracle64)
    g = np.random.default_rng(7).normal(size=(2, 48, 40, 5))
    r1 = _run_depth(ops, a, 8.0, 8.0, gout=g)
    r2 = _run_depth(ops, a, 8.0, 8.0, gout=g)
    assert torch.equal(r1["grads"]["template"], r2["grads"]["template"])
    assert float(r1["grads"]["template"][..., 3].abs().max()) > 0


def test_raymarcher_with_pos_img(ops):
    from ava256_amd import Raymarcher, compute_raydirs
    from ava256_amd.scene import make_scene
    s = make_scene(2, 40, 48, 128, device="cuda", seed=81, alpha_gain=6.0)
    rp, rd, tm = compute_raydirs(s["campos"], s["camrot"], s["focal"], s["princpt"], s["pixelcoords"], s["volradius"])
    rm = Raymarcher(s["volradius"])
    dec = {k: s[k] for k in ("primpos", "primrot", "primscale", "template")}
    rgb0, alpha0, rgba0, pos0 = rm(rp, rd, tm, dec)
    assert pos0 is None
    assert rm(rp, rd, tm, dec, with_pos_img=False)[3] is None
    dec = {k: v.detach().clone().requires_grad_(True) for k, v in dec.items()}
    rgb, alpha, rgba, pos = rm(rp, rd, tm, dec, with_pos_img=True)
    assert torch.equal(rgb, rgb0) and torch.equal(alpha, alpha0) and torch.equal(rgba, rgba0)
    assert pos.shape == (2, 3, 40, 48)
    _, depth = ops.mvpraymarch_depth(rp, rd, rm.dt, tm, (dec["primpos"], dec["primrot"], dec["primscale"]),
                                     dec["template"], None)
    want = rp.movedim(3, 1) * alpha + rd.movedim(3, 1) * depth.unsqueeze(1)
    assert torch.equal(pos, want)
    pos.square().sum().backward()
    torch.cuda.synchronize()
    assert float(dec["template"].grad[..., 3].abs().max()) > 0
    assert float(dec["template"].grad[..., :3].abs().max()) == 0   # depth and alpha reach the opacity only
    assert bool(torch.isfinite(dec["primpos"].grad).all())


def test_forward_under_graph_capture_replays(ops):
    from ava256_amd import compute_raydirs
    from ava256_amd.scene import make_scene
    s = make_scene(1, 64, 64, 256, device="cuda", seed=91, alpha_gain=6.0)
    rp, rd, tm = compute_raydirs(s["campos"], s["camrot"], s["focal"], s["princpt"], s["pixelcoords"], s["volradius"])
    prim = (s["primpos"], s["primrot"], s["primscale"])
    with torch.no_grad():
        eager = ops.mvpraymarch_depth(rp, rd, s["stepsize"], tm, prim, s["template"], None)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            ops.mvpraymarch_depth(rp, rd, s["stepsize"], tm, prim, s["template"], None)   # warm-up outside capture
        torch.cuda.current_stream().wait_stream(st)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap = ops.mvpraymarch_depth(rp, rd, s["stepsize"], tm, prim, s["template"], None)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(cap[0], eager[0]) and torch.equal(cap[1], eager[1])


def test_full_c2_batch_against_oracle_on_sampled_rays(ops, oracle64):
    """One full-size C2 launch (80 cameras, 512^2, K = 4096, the bench workload), checked against the oracle on 3 images x
    32 x 32 sampled rays, forward (pos_img) and the backward's finiteness."""
    from ava256_amd import compute_raydirs
    from ava256_amd.scene import make_scene
    s = make_scene(80, 512, 512, 4096, device="cuda", seed=1112, alpha_gain=1.0)
    rp, rd, tm = compute_raydirs(s["campos"], s["camrot"], s["focal"], s["princpt"], s["pixelcoords"], s["volradius"])
    t = {k: s[k].detach().clone().requires_grad_(True) for k in NAMES}
    rgba, depth = ops.mvpraymarch_depth(rp, rd, s["stepsize"], tm, (t["primpos"], t["primrot"], t["primscale"]),
                                        t["template"], None)
    torch.autograd.backward([rgba, depth], [torch.randn_like(rgba), torch.randn_like(depth)])
    torch.cuda.synchronize()
    for k in NAMES:
        assert bool(torch.isfinite(t[k].grad).all()), k
    rng = np.random.default_rng(12)
    for n in (0, 37, 79):
        ys, xs = rng.integers(0, 512, 32 * 32), rng.integers(0, 512, 32 * 32)
        pick = lambda x: npf(x[n][ys, xs]).reshape((1, 32, 32) + tuple(x.shape[3:]))  # noqa: E731
        a = (pick(rp), pick(rd), float(s["stepsize"]), pick(tm), npf(s["primpos"][n:n + 1]), npf(s["primrot"][n:n + 1]),
             npf(s["primscale"][n:n + 1]), npf(s["template"][n:n + 1]))
        ref, _, st = oracle64.march_forward(*a, ray_diagnostics=True)
        assert st["rays_hit"] > 0
        ref2, _, _ = oracle64.march_forward(*_scene_prime(a))
        ok = _not_borderline(st)
        mine_rgba = pick(rgba.detach())
        pos = _pos_img(a, mine_rgba, pick(depth.detach()))
        err = np.abs(pos - (ref2[..., :3] - OFFSET * ref2[..., 3:4])).max(-1)
        assert (err[ok] > FWD_TOL * max(1.0, np.abs(ref2).max())).sum() == 0, (n, err[ok].max())
        err_rgba = np.abs(mine_rgba - ref).max(-1)
        assert (err_rgba[ok] > FWD_TOL * max(1.0, np.abs(ref).max())).sum() == 0, (n, err_rgba[ok].max())
