"""halfslab -- the opt-in render path over half-precision slabs (round 5).

The reference's kernels read fp32 RGBA slabs (extensions/mvpraymarch/primsampler.h:44-66, utils.h:408-502; the decoder
hand-off models/decoders/assembler.py:261 makes them).  BASELINE.json's configs[1] is labelled "bf16" and the forward's
sweep is bound by its gathers, so a caller that RENDERS (no gradients) may hand the march fp16 RGBA slabs instead:

    th = template_to_half(template)                        # or assemble_template_half(tex, opacity, nboxes)
    rgba = render_half(raypos, raydir, stepsize, tminmax, (primpos, primrot, primscale), th)
    rgba = render_half_from_cameras(campos, camrot, focal, princpt, pixelcoords, volradius, stepsize, primtransf, th)

Same sample set, weights, interpolation and compositing in fp32; only the slab VALUES carry the fp16 storage rounding
(2^-11 relative).  Never the headline number: `mvpraymarch(...)` keeps fp32 slabs, and these render functions refuse to run
with gradients enabled on their inputs.  8^3 slabs (the reference's size).

TRAINING over fp16 slabs is a separate, differentiable operator (opt-in; trainloop.RaymarchTrainModel(half_slabs=True)):

    rgba = mvpraymarch_half(raypos, raydir, stepsize, tminmax, (primpos, primrot, primscale), template, template_half=None)
    rgba = mvpraymarch_half_from_cameras(campos, camrot, focal, princpt, pixelcoords, volradius, stepsize, primtransf,
                                         template, template_half=None)

The fp16 rounding is a straight-through step: the rays march over template_half (the round-to-nearest-even copy of the fp32
`template`; made here with template_to_half when not given), and the gradients -- fp32, for template and the three pose
tensors -- are the march's gradients at the rounded slab values.  The differentiable slab input is the fp32 master: autograd
casts a gradient to its input's dtype, and fp16 slab gradients would underflow.  Bit for bit what mvpraymarch gives on
template_half.float() (tests/test_gpu_half_train.py).  No warp field, 8^3 slabs."""
import math

import torch

from . import _hooks, _lib
from ._tensors import aligned, ptr, require_device_f32, stream_ptr
from .mvpraymarch import (_DEFAULT_OPTIONS, _MVPRaymarchHalf, _MVPRaymarchHalfFromCameras, _camera_args,
                          _unpack_primtransf, build_accel)


def template_to_half(template):
    """[N,K,TD,TH,TW,4] float32 -> float16, round to nearest even (one pass: 16 B read + 8 B written per voxel)."""
    template = aligned(require_device_f32("template", template))
    assert template.dim() == 6 and template.size(-1) == 4
    out = torch.empty(template.shape, device=template.device, dtype=torch.float16)
    with torch.cuda.device(template.device), _hooks.timed("template_to_half", template.device):
        _lib.check(_lib.get_lib().mvp_template_to_half(template.numel() // 4, ptr(template), ptr(out),
                                                       stream_ptr(template.device)), "mvp_template_to_half")
    return out


def assemble_template_half(tex, opacity, nboxes, boxsize=8):
    """assemble_template(...) writing fp16 slabs directly: tex [N,3*B,nh*B,nh*B], opacity [N,B,nh*B,nh*B] ->
    [N,nboxes,B,B,B,4] float16 (the decoder hand-off of rgb.py:137-143 / geometry.py:183-185 / assembler.py:261)."""
    tex = require_device_f32("tex", tex)
    opacity = require_device_f32("opacity", opacity)
    nh = int(math.isqrt(nboxes))
    assert nh * nh == nboxes, "nboxes must be a square (rgb.py:130-131)"
    N, S = tex.size(0), nh * boxsize
    assert tex.shape == (N, 3 * boxsize, S, S) and opacity.shape == (N, boxsize, S, S)
    out = torch.empty((N, nboxes, boxsize, boxsize, boxsize, 4), device=tex.device, dtype=torch.float16)
    with torch.cuda.device(tex.device), _hooks.timed("assemble_half", tex.device):
        _lib.check(_lib.get_lib().mvp_template_assemble_forward_half(N, nh, boxsize, ptr(tex), ptr(opacity), ptr(out),
                                                                     stream_ptr(tex.device)),
                   "mvp_template_assemble_forward_half")
    return out


def _device_prims(primtransf):
    primpos, primrot, primscale = _unpack_primtransf(primtransf)
    return (require_device_f32("primpos", primpos), require_device_f32("primrot", primrot),
            require_device_f32("primscale", primscale))


def _check_half(template_half, N, K):
    if not torch.is_tensor(template_half) or template_half.dtype != torch.float16 or not template_half.is_cuda:
        raise RuntimeError("template_half must be a float16 device tensor (template_to_half / assemble_template_half)")
    if not template_half.is_contiguous():
        raise RuntimeError("template_half must be contiguous")
    assert template_half.dim() == 6 and template_half.size(-1) == 4 and template_half.shape[:2] == (N, K)
    if tuple(template_half.shape[2:5]) != (8, 8, 8):
        raise NotImplementedError("the half-precision render path takes 8^3 slabs")
    return aligned(template_half)


def _check_prims(primpos, primrot, primscale, N):
    """The shape contract of the fp32 operator (mvpraymarch.py: _forward_impl; reference mvpraymarch.py:112-127): one
    primitive set PER IMAGE.  build_accel sizes the node boxes from primpos.size(0), so a [1,K,..] avatar rendered from N > 1
    cameras would make the kernel read boxes and poses of images that do not exist."""
    K = primpos.size(1) if primpos.dim() == 3 else -1
    assert primpos.shape == (N, K, 3) and primrot.shape == (N, K, 3, 3) and primscale.shape == (N, K, 3), \
        "primpos / primrot / primscale must be [N,K,3] / [N,K,3,3] / [N,K,3] with N = %d images" % N
    return K


def _same_device(*tensors):
    devs = {t.device for t in tensors if torch.is_tensor(t)}
    if len(devs) > 1:
        raise RuntimeError("all inputs must live on one device, got %s" % sorted(str(d) for d in devs))


def _no_grad(*tensors):
    if torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in tensors):
        raise RuntimeError("the half-precision slab path renders only: call it under torch.no_grad() (training keeps fp32 "
                           "slabs: mvpraymarch)")


def render_half(raypos, raydir, stepsize, tminmax, primtransf, template_half, fadescale=8.0, fadeexp=8.0):
    """mvpraymarch(...) without gradients over fp16 slabs -> rayrgba [N,H,W,4] float32."""
    primpos, primrot, primscale = _device_prims(primtransf)
    _no_grad(raypos, raydir, tminmax, primpos, primrot, primscale, template_half)
    raypos = aligned(require_device_f32("raypos", raypos))
    raydir = aligned(require_device_f32("raydir", raydir))
    tminmax = aligned(require_device_f32("tminmax", tminmax))
    assert raypos.dim() == 4 and raypos.size(3) == 3
    N, H, W = raypos.size(0), raypos.size(1), raypos.size(2)
    assert raydir.shape == raypos.shape and tminmax.shape == raypos.shape[:3] + (2,)
    K = _check_prims(primpos, primrot, primscale, N)
    th = _check_half(template_half, N, K)
    _same_device(raypos, raydir, tminmax, primpos, primrot, primscale, th)
    dev = primpos.device
    with torch.no_grad():
        _, _, nodeaabb = build_accel((primpos, primrot, primscale), 0, fixedorder=True)
        rayrgba = torch.empty((N, H, W, 4), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev), _hooks.timed("march_render_half", dev):
            _lib.check(_lib.get_lib().mvp_march_render_half(
                N, H, W, K, ptr(raypos), ptr(raydir), ptr(tminmax), None, None, None, None, None, 1.0, float(stepsize),
                ptr(nodeaabb), ptr(primpos), ptr(primrot), ptr(primscale), 8, 8, 8, ptr(th), ptr(rayrgba),
                float(fadescale), float(fadeexp), ptr(_hooks.diag), stream_ptr(dev)), "mvp_march_render_half")
    return rayrgba


def render_half_from_cameras(campos, camrot, focal, princpt, pixelcoords, volradius, stepsize, primtransf, template_half,
                             fadescale=8.0, fadeexp=8.0):
    """mvpraymarch_from_cameras(...) without gradients over fp16 slabs (rays made inside the march)."""
    primpos, primrot, primscale = _device_prims(primtransf)
    _no_grad(campos, camrot, focal, princpt, primpos, primrot, primscale, template_half)
    campos, camrot, focal, princpt, pc, N, H, W = _camera_args(campos, camrot, focal, princpt, pixelcoords)
    K = _check_prims(primpos, primrot, primscale, N)
    th = _check_half(template_half, N, K)
    _same_device(campos, camrot, focal, princpt, pc, primpos, primrot, primscale, th)
    dev = primpos.device
    with torch.no_grad():
        _, _, nodeaabb = build_accel((primpos, primrot, primscale), 0, fixedorder=True)
        rayrgba = torch.empty((N, H, W, 4), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev), _hooks.timed("march_render_half", dev):
            _lib.check(_lib.get_lib().mvp_march_render_half(
                N, H, W, K, None, None, None, ptr(campos), ptr(camrot), ptr(focal), ptr(princpt), ptr(pc),
                float(volradius), float(stepsize), ptr(nodeaabb), ptr(primpos), ptr(primrot), ptr(primscale), 8, 8, 8,
                ptr(th), ptr(rayrgba), float(fadescale), float(fadeexp), ptr(_hooks.diag), stream_ptr(dev)),
                "mvp_march_render_half")
    return rayrgba


# ---- training over fp16 slabs ------------------------------------------------------------------------------------------

def assemble_template_frames_half(tex, opacity, gain, nboxes, boxsize=8):
    """The fp16 twin of assemble.assemble_template_frames, without gradients: tex [1,3*B,nh*B,nh*B], opacity [1,B,nh*B,nh*B],
    gain [F] -> [F,nboxes,B,B,B,4] float16 = (gain[f] * assemble(tex, opacity)) rounded to nearest even -- bit for bit
    assemble_template_frames(...).half(), without the fp32 slabs ever being read back."""
    tex = require_device_f32("tex", tex)
    opacity = require_device_f32("opacity", opacity)
    gain = require_device_f32("gain", gain)
    nh = int(math.isqrt(nboxes))
    if nh * nh != nboxes:
        raise ValueError("nboxes must be a square (rgb.py:130-131)")
    S, F = nh * boxsize, gain.numel()
    if tex.shape != (1, 3 * boxsize, S, S) or opacity.shape != (1, boxsize, S, S) or gain.dim() != 1:
        raise ValueError("tex / opacity / gain must be [1,%d,%d,%d] / [1,%d,%d,%d] / [F]" % (3 * boxsize, S, S, boxsize, S, S))
    _same_device(tex, opacity, gain)
    dev = tex.device
    with torch.no_grad():
        out = torch.empty((F, nboxes, boxsize, boxsize, boxsize, 4), device=dev, dtype=torch.float16)
        with torch.cuda.device(dev), _hooks.timed("assemble_frames_half", dev):
            _lib.check(_lib.get_lib().mvp_template_assemble_frames_forward_half(
                F, nh, boxsize, ptr(tex), ptr(opacity), ptr(gain), ptr(out), stream_ptr(dev)),
                "mvp_template_assemble_frames_forward_half")
    return out


def _check_train_half_args(N, primpos, primrot, primscale, template, template_half, warp, algo, others):
    """Everything the training operator refuses, decided from shapes, dtypes and devices alone (no device work)."""
    if warp is not None or algo != 0:
        raise NotImplementedError("mvpraymarch_half has no warp-field sampler (algo 0 only)")
    for name, t in (("primpos", primpos), ("primrot", primrot), ("primscale", primscale), ("template", template)):
        if not torch.is_tensor(t):
            raise TypeError("%s must be a tensor" % name)
    if template.dtype != torch.float32:
        raise RuntimeError("template must be the float32 master (its gradient is returned in its dtype), got %s; pass the "
                           "fp16 copy as template_half" % template.dtype)
    K = primpos.size(1) if primpos.dim() == 3 else -1
    if primpos.shape != (N, K, 3) or primrot.shape != (N, K, 3, 3) or primscale.shape != (N, K, 3):
        raise ValueError("primpos / primrot / primscale must be [N,K,3] / [N,K,3,3] / [N,K,3] with N = %d images" % N)
    if template.dim() != 6 or template.size(-1) != 4 or tuple(template.shape[:2]) != (N, K):
        raise ValueError("template must be [N,K,TD,TH,TW,4] with N = %d, K = %d, got %s" % (N, K, tuple(template.shape)))
    if tuple(template.shape[2:5]) != (8, 8, 8):
        raise NotImplementedError("the half-precision slab path takes 8^3 slabs, got %s" % (tuple(template.shape[2:5]),))
    if template_half is not None:
        if not torch.is_tensor(template_half) or template_half.dtype != torch.float16:
            raise RuntimeError("template_half must be a float16 tensor (template_to_half / assemble_template_frames_half)")
        if template_half.shape != template.shape:
            raise ValueError("template_half %s must have the shape of template %s" % (tuple(template_half.shape),
                                                                                     tuple(template.shape)))
    _same_device(primpos, primrot, primscale, template, template_half, *others)
    return K


def _half_of(template, template_half):
    """The slabs the march reads: the given rounding (not differentiable), or the one made here."""
    if template_half is None:
        return template_to_half(template)
    if not template_half.is_cuda:
        raise RuntimeError("template_half must be a CUDA/HIP tensor (there is no CPU path)")
    if not template_half.is_contiguous():
        raise RuntimeError("template_half must be contiguous")
    return aligned(template_half.detach())


def _fade_options(fadescale, fadeexp):
    """mvpraymarch's default options with the two this path takes."""
    return dict(_DEFAULT_OPTIONS, fadescale=fadescale, fadeexp=fadeexp)


def mvpraymarch_half(raypos, raydir, stepsize, tminmax, primtransf, template, template_half=None, fadescale=8.0,
                     fadeexp=8.0, warp=None, algo=0):
    """mvpraymarch(...) over fp16 slabs, with gradients: template is the fp32 master [N,K,8,8,8,4]; template_half its
    round-to-nearest-even copy (float16, same shape; made here when None).  Returns rayrgba [N,H,W,4] float32.  `warp` /
    `algo` exist only to be refused (no warp-field sampler on this path)."""
    primpos, primrot, primscale = _unpack_primtransf(primtransf)
    for name, t in (("raypos", raypos), ("raydir", raydir), ("tminmax", tminmax)):
        if not torch.is_tensor(t):
            raise TypeError("%s must be a tensor" % name)
    if raypos.dim() != 4 or raypos.size(3) != 3 or raydir.shape != raypos.shape or \
            tminmax.shape != raypos.shape[:3] + (2,):
        raise ValueError("raypos / raydir / tminmax must be [N,H,W,3] / [N,H,W,3] / [N,H,W,2]")
    _check_train_half_args(raypos.size(0), primpos, primrot, primscale, template, template_half, warp, algo,
                           (raypos, raydir, tminmax))
    return _MVPRaymarchHalf.apply(raypos, raydir, stepsize, tminmax, primpos, primrot, primscale, template, template_half,
                                  torch.is_grad_enabled(), _fade_options(fadescale, fadeexp))


def mvpraymarch_half_from_cameras(campos, camrot, focal, princpt, pixelcoords, volradius, stepsize, primtransf, template,
                                  template_half=None, fadescale=8.0, fadeexp=8.0, warp=None, algo=0):
    """mvpraymarch_from_cameras(...) over fp16 slabs, with gradients (see mvpraymarch_half).  pixelcoords: [N,H,W,2] tensor
    or a (W, H) tuple."""
    primpos, primrot, primscale = _unpack_primtransf(primtransf)
    for name, t in (("campos", campos), ("camrot", camrot), ("focal", focal), ("princpt", princpt)):
        if not torch.is_tensor(t):
            raise TypeError("%s must be a tensor" % name)
    N = campos.size(0)
    if campos.shape != (N, 3) or camrot.shape != (N, 3, 3) or focal.shape != (N, 2) or princpt.shape != (N, 2):
        raise ValueError("campos / camrot / focal / princpt must be [N,3] / [N,3,3] / [N,2] / [N,2]")
    if isinstance(pixelcoords, tuple):
        W, H = pixelcoords
        pixelcoords = (int(W), int(H))
    elif not torch.is_tensor(pixelcoords) or pixelcoords.dim() != 4 or pixelcoords.size(0) != N or pixelcoords.size(3) != 2:
        raise ValueError("pixelcoords must be [N,H,W,2] or a (W, H) tuple")
    _check_train_half_args(N, primpos, primrot, primscale, template, template_half, warp, algo,
                           (campos, camrot, focal, princpt, pixelcoords))
    for name, t in (("campos", campos), ("camrot", camrot), ("focal", focal), ("princpt", princpt)):
        require_device_f32(name, t)
    if torch.is_tensor(pixelcoords):
        require_device_f32("pixelcoords", pixelcoords)
    return _MVPRaymarchHalfFromCameras.apply(campos, camrot, focal, princpt, pixelcoords, float(volradius), stepsize,
                                             primpos, primrot, primscale, template, template_half,
                                             torch.is_grad_enabled(), _fade_options(fadescale, fadeexp))
