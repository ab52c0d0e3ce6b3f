"""Training-loop counterpart (ava-256_amd/trainloop.py): loop semantics on CPU with an injected pure-torch renderer
(no oracle, no kernels), the 2-rank gloo DDP path, and -- on the GPU -- a real optimisation through the kernels."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT


def fake_renderer(camrot, campos, focal, princpt, pixelcoords, decout):
    """Differentiable stand-in for rays+raymarch on CPU: every decout tensor influences the image."""
    B, H, W = pixelcoords.shape[:3]
    t = decout["template"]
    rgb = t[..., :3].mean(dim=(1, 2, 3, 4)) * (1.0 + decout["primpos"].mean(dim=(1, 2)))[:, None]      # [B,3]
    a = torch.sigmoid(t[..., 3].mean(dim=(1, 2, 3, 4)) + decout["primrot"].mean(dim=(1, 2, 3)))         # [B]
    img = rgb[:, :, None, None] * (pixelcoords[..., 0] / W + 1.0)[:, None]
    return img * a[:, None, None, None], a[:, None, None, None].expand(B, 1, H, W)


def _batch(N, H, W, seed, code_dim=16):
    from ava256_amd.trainloop import make_training_batch
    b, _ = make_training_batch(N, H, W, 8, "cpu", seed=seed, code_dim=code_dim)
    g = torch.Generator().manual_seed(seed)
    b["image"] = 50.0 + 10.0 * torch.randn(N, 3, H, W, generator=g)
    return b


def _golden_loss():
    return np.load(os.path.join(ROOT, "tests", "golden", "trainstep_loss.npz"))


def test_loss_formula_is_the_references_own():
    """Trainer.losses / Trainer.total_loss against tests/golden/trainstep_loss.npz: the reference's statements
    ddp-train.py:404-430 executed by tests/golden/gen_trainstep.py (float64) with the weights of configs/config.yaml:17-21
    -- every term (irgbl1, vertl1 with its de-normalisation, primvolsum, kldiv) and the weighted total."""
    import types
    from ava256_amd.trainloop import REFERENCE_LOSS_WEIGHTS, Trainer
    g = _golden_loss()
    weights = dict(zip(g["weight_names"].tolist(), g["weight_values"].tolist()))
    assert REFERENCE_LOSS_WEIGHTS == weights
    t = lambda a: torch.from_numpy(np.asarray(a))
    tr = Trainer.__new__(Trainer)
    tr.loss_weights = dict(REFERENCE_LOSS_WEIGHTS)
    tr.raw_model = types.SimpleNamespace(decoder=types.SimpleNamespace(vertstd=t(g["vertstd"]), vertmean=t(g["vertmean"])))
    output = {k[4:]: t(g[k]) for k in g.files if k.startswith("out/")}
    batch = {k[5:]: t(g[k]) for k in g.files if k.startswith("data/")}
    losses = tr.losses(output, batch)
    assert sorted(losses) == sorted(k[5:] for k in g.files if k.startswith("term/"))
    for k, v in losses.items():
        assert v.shape == g["term/" + k].shape and np.allclose(v.numpy(), g["term/" + k], rtol=1e-13, atol=0), k
    assert abs(float(tr.total_loss(losses)) - float(g["loss"])) <= 1e-12 * abs(float(g["loss"]))
    # a model without a geometry branch / VAE pair computes only the terms it has the inputs for
    output.update(verts=None, expr_mu=None, expr_logstd=None)
    assert sorted(tr.losses(output, batch)) == ["irgbl1", "primvolsum"]


def _f64(batch):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}


def test_loop_semantics_cpu():
    import copy
    from ava256_amd.trainloop import (CodeEncoderStandIn, RaymarchTrainModel, SlabDecoderStandIn, Trainer,
                                      forward_schedule, mean_ell_1)
    torch.manual_seed(0)
    model = RaymarchTrainModel(SlabDecoderStandIn(8, seed=1), renderer=fake_renderer, encoder=CodeEncoderStandIn())
    tr = Trainer(model, lr=2e-4, lr_scheduler_iter=2, gamma=1.4, clip=1.0)
    assert isinstance(tr.optim, torch.optim.Adam) and tr.optim.defaults["betas"] == (0.9, 0.999)
    assert tr.loss_weights == {"irgbl1": 1.0, "vertl1": 0.1, "kldiv": 1.0e-3, "primvolsum": 0.01}  # configs/config.yaml:17-21
    b = _batch(3, 8, 8, 0)
    # the loss of the step = the (reference-pinned, see above) formula on the model's outputs at iteration 0
    twin = copy.deepcopy(model)
    out = twin(b["camrot"], b["campos"], b["focal"], b["princpt"], b["pixelcoords"], b["code"],
               schedule=forward_schedule(0), gt_verts=b["verts"], noise=b["noise"])
    twin_tr = Trainer(twin)
    terms = twin_tr.losses(out, b)
    assert sorted(terms) == ["irgbl1", "kldiv", "primvolsum", "vertl1"]
    ref = twin_tr.total_loss(terms)
    loss, parts = tr.step(b)
    assert torch.allclose(loss, ref.detach(), rtol=1e-6)
    # StepLR(step_size=2, gamma=1.4): lr after 2 steps = 2e-4 * 1.4
    tr.step(b)
    assert abs(tr.optim.param_groups[0]["lr"] - 2e-4 * 1.4) < 1e-12
    # gradient clipping: total norm after the step's clip is <= clip (checked on a fresh backward)
    tr.optim.zero_grad()
    out = model(b["camrot"], b["campos"], b["focal"], b["princpt"], b["pixelcoords"], b["code"])
    (1000.0 * mean_ell_1(out["irgbrec"], b["image"])).backward()
    torch.nn.utils.clip_grad_norm_(tr.params, 1.0)
    tot = torch.sqrt(sum((p.grad ** 2).sum() for p in tr.params if p.grad is not None))
    assert tot <= 1.0 + 1e-4


def test_forward_schedule_of_the_first_iterations():
    """ddp-train.py:371-377: running_avg_scale / gt_geo / residuals_weight switch at iteration 100."""
    from ava256_amd.trainloop import RaymarchTrainModel, SlabDecoderStandIn, Trainer, forward_schedule
    assert forward_schedule(0) == {"running_avg_scale": True, "use_gt_geo": True, "residuals_weight": 0.0}
    assert forward_schedule(99) == forward_schedule(0)
    assert forward_schedule(100) == {"running_avg_scale": False, "use_gt_geo": False, "residuals_weight": 1.0}
    model = RaymarchTrainModel(SlabDecoderStandIn(8, seed=1), renderer=fake_renderer)
    tr = Trainer(model)
    b = _batch(2, 8, 8, 0)
    tr.step(b)
    assert model.last_schedule == forward_schedule(0)
    tr.iternum = 100
    tr.step(b)
    assert model.last_schedule == forward_schedule(100) and tr.iternum == 101


def test_decoder_consumes_the_schedule():
    """What the three switches do inside the decoder (assembler.py:105-109,183-199,241-253): ground-truth guide mesh,
    running average of adaptwarps (first value assigned, then 0.9 / 0.1), residual weight 0 = pose residuals off."""
    from ava256_amd.trainloop import SlabDecoderStandIn, forward_schedule
    torch.manual_seed(3)
    dec = SlabDecoderStandIn(16, seed=2)
    with torch.no_grad():
        dec.pos_delta.normal_(), dec.rotvec.normal_(), dec.logscale.normal_()
    code, gt = torch.randn(3, 16), 0.1 * torch.randn(3, 16, 3)
    warm, late = forward_schedule(0), forward_schedule(100)
    assert float(dec.adaptwarps.max()) == 0.0
    o1 = dec(code, schedule=warm, gt_geo=gt)
    # guide mesh = ground truth: placement does not depend on the predicted geometry, which is still returned
    guide = gt * dec.vertstd + dec.vertmean
    pm = (dec.tri_bar[None, :, :, None] * guide[:, dec.tri_idx]).sum(2) / dec.volradius
    assert torch.allclose(o1["primpos"], pm, atol=1e-7)                      # residuals_weight = 0: no position residual
    assert torch.allclose(o1["verts"], dec.geo_head(code).view(3, 16, 3) * dec.vertstd + dec.vertmean)
    n1, n2 = dec.tri_idx[:, 1], dec.tri_idx[:, 2]
    cs = torch.maximum((pm[:, n1] - pm).norm(dim=-1), (pm[:, n2] - pm).norm(dim=-1)).amax(0)
    aw1 = 2.0 / cs
    assert torch.allclose(dec.adaptwarps, aw1)                               # first time: assigned (assembler.py:195-196)
    assert torch.allclose(o1["primscale"], (aw1 * 0.8)[None, :, None].expand(3, 16, 3))  # scale residual -> 1 at rw = 0
    assert torch.allclose(o1["primrot"], dec.base_rot[None].expand(3, -1, -1, -1), atol=1e-5)
    gt2 = 0.1 * torch.randn(3, 16, 3)
    dec(code, schedule=warm, gt_geo=gt2)
    guide2 = gt2 * dec.vertstd + dec.vertmean
    pm2 = (dec.tri_bar[None, :, :, None] * guide2[:, dec.tri_idx]).sum(2) / dec.volradius
    cs2 = torch.maximum((pm2[:, n1] - pm2).norm(dim=-1), (pm2[:, n2] - pm2).norm(dim=-1)).amax(0)
    aw2 = 0.9 * aw1 + 0.1 * (2.0 / cs2)
    assert torch.allclose(dec.adaptwarps, aw2)                               # then the running average (:197-198)
    o3 = dec(code, schedule=late, gt_geo=gt)                                 # iteration >= 100
    assert torch.equal(dec.adaptwarps, aw2.to(dec.adaptwarps.dtype)) or torch.allclose(dec.adaptwarps, aw2)  # frozen
    geo = o3["verts"]
    pm3 = (dec.tri_bar[None, :, :, None] * geo[:, dec.tri_idx]).sum(2) / dec.volradius
    assert torch.allclose(o3["primpos"], pm3 + 0.01 * dec.pos_delta[None], atol=1e-7)    # predicted mesh + residual
    assert torch.allclose(o3["primscale"], (dec.adaptwarps * 0.8)[None, :, None] * torch.exp(0.1 * dec.logscale)[None])
    assert not torch.allclose(o3["primrot"], o1["primrot"], atol=1e-3)


def test_nan_and_inf_gradients_are_zeroed():
    """ddp-train.py:436-439: NaN/Inf gradient entries become 0 before clipping and the optimiser step."""
    from ava256_amd.trainloop import RaymarchTrainModel, SlabDecoderStandIn, Trainer
    model = RaymarchTrainModel(SlabDecoderStandIn(8, seed=1), renderer=fake_renderer)
    tr = Trainer(model)
    p = model.decoder.pos_delta
    before = p.detach().clone()
    h = p.register_hook(lambda g: torch.full_like(g, float("nan")))
    h2 = model.decoder.logscale.register_hook(lambda g: torch.full_like(g, float("inf")))
    tr.step(_batch(2, 8, 8, 1))
    h.remove(), h2.remove()
    for q in tr.params:
        assert torch.isfinite(q).all()
    assert torch.equal(p.detach(), before)          # zero gradient -> Adam leaves the parameter where it was
    assert any(not torch.equal(q.detach(), q0) for q, q0 in [(model.decoder.rgb, torch.zeros_like(model.decoder.rgb))])


def test_decode_tail_matches_the_reference_statements():
    """Colour calibration, background and matting (models/autoencoder.py:254-265, models/colorcals/colorcal.py:27-31,
    models/bg/mlp2d.py:58-72 for the network shape): irgbrec = (w * rayrgb + b) + (1 - rayalpha) * bg, and the gradient
    that reaches rayalpha through the matting term is -bg * dL/dirgbrec summed over colour."""
    from ava256_amd.trainloop import BackgroundMLPStandIn, ColorCalStandIn, RaymarchTrainModel, SlabDecoderStandIn
    torch.manual_seed(1)
    cc, bgm = ColorCalStandIn(5, 3), BackgroundMLPStandIn(5, 3)
    with torch.no_grad():
        cc.wcam.add_(0.1 * torch.randn_like(cc.wcam)), cc.bident.add_(torch.randn_like(cc.bident))
    model = RaymarchTrainModel(SlabDecoderStandIn(8, seed=1), renderer=fake_renderer, colorcal=cc, bgmodel=bgm)
    b = _batch(3, 6, 10, 0)
    camindex, idindex = torch.tensor([0, 4, 2]), torch.tensor([1, 0, 2])
    out = model(b["camrot"], b["campos"], b["focal"], b["princpt"], b["pixelcoords"], b["code"], camindex=camindex,
                idindex=idindex)
    decout = model.decoder(b["code"])
    rgb, alpha = fake_renderer(b["camrot"], b["campos"], b["focal"], b["princpt"], b["pixelcoords"], decout)
    w = (cc.wcam[camindex] + cc.wident[idindex])[:, :, None, None]
    bb = (cc.bcam[camindex] + cc.bident[idindex])[:, :, None, None]
    assert out["bg"].shape == (3, 3, 6, 10)
    # the background network is a per-pixel function of (camera, identity, normalised pixel position): mlp2d.py:62-70
    pc = b["pixelcoords"]
    sc = torch.cat([pc[..., :1] * 2 / (pc.shape[-2] - 1) - 1, pc[..., 1:] * 2 / (pc.shape[-3] - 1) - 1], dim=-1)
    assert float(sc.min()) == -1.0 and float(sc.max()) == 1.0
    assert torch.allclose(out["bg"], bgm(camindex, idindex, sc))
    assert torch.allclose(out["irgbrec"], (w * rgb + bb) + (1.0 - alpha) * out["bg"], rtol=1e-6, atol=1e-4)
    # 120 -> 256 x 5 -> 3 per pixel, 40 + 40 + 40 input channels (mlp2d.py:29-41)
    lin = [m for m in bgm.mlp if isinstance(m, torch.nn.Linear)]
    assert [(m.in_features, m.out_features) for m in lin] == [(120, 256)] + [(256, 256)] * 4 + [(256, 3)]
    # without indices the reference skips both stages and mattes over black (autoencoder.py:255,259,266-269)
    out0 = model(b["camrot"], b["campos"], b["focal"], b["princpt"], b["pixelcoords"], b["code"])
    assert out0["bg"] is None and torch.allclose(out0["irgbrec"], rgb)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ddp_worker(rank, world, port, outdir):
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ava256_amd.trainloop import CodeEncoderStandIn, RaymarchTrainModel, SlabDecoderStandIn, Trainer
    from test_trainloop import _batch, _f64, fake_renderer
    # float64: the fake renderer's gradients are sums of +-1/numel terms that cancel; in float32 their value depends on
    # the thread-level summation order by ~1e-3, which would mask what this test is about
    model = RaymarchTrainModel(SlabDecoderStandIn(8, seed=1), renderer=fake_renderer, encoder=CodeEncoderStandIn()).double()
    tr = Trainer(model, ddp=True)
    full = _f64(_batch(4, 8, 8, 7))
    shard = {k: v[rank * 2:(rank + 1) * 2] for k, v in full.items()}
    tr.step(shard)
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    aw1 = model.decoder.adaptwarps.detach().clone()
    for _ in range(2):
        tr.step(shard)
    torch.save({"state": {k: v.detach().clone() for k, v in model.state_dict().items()}, "grads": grads, "aw1": aw1},
               os.path.join(outdir, "r%d.pt" % rank))
    dist.destroy_process_group()


def test_ddp_two_ranks_match_single_process(tmp_path):
    """Only parameter gradients cross ranks; with equal shards the 2-rank result equals one process on the full batch
    (mean of shard gradients = gradient of the mean loss)."""
    from ava256_amd.trainloop import CodeEncoderStandIn, RaymarchTrainModel, SlabDecoderStandIn, Trainer
    port = _free_port()
    mp.spawn(_ddp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a = torch.load(os.path.join(str(tmp_path), "r0.pt"))
    b = torch.load(os.path.join(str(tmp_path), "r1.pt"))
    for k in a["state"]:
        assert torch.equal(a["state"][k], b["state"][k]), k       # ranks stay in lock-step (buffers included: no
                                                                  # buffer broadcast, adaptwarps by its own all-reduce)
    # first-step gradients (after all-reduce, NaN masking and clipping) equal the single-process ones.  Parameters
    # after several Adam steps are not compared: Adam turns round-off-sized gradients into +-lr updates.
    model = RaymarchTrainModel(SlabDecoderStandIn(8, seed=1), renderer=fake_renderer, encoder=CodeEncoderStandIn()).double()
    tr = Trainer(model)
    tr.step(_f64(_batch(4, 8, 8, 7)))
    # the running average that does not shard by camera (assembler.py:183-199): the batch maximum is taken
    # over both ranks' frames (a K-float MAX all-reduce), so each rank holds the single-process value -- bit for bit
    assert torch.equal(a["aw1"], model.decoder.adaptwarps) and torch.equal(b["aw1"], model.decoder.adaptwarps)
    assert float(a["aw1"].min()) > 0.0
    for n, p_ in model.named_parameters():
        g = a["grads"][n]
        err = float((p_.grad - g).abs().max()) / float(g.abs().max() + 1e-300)
        assert err <= 1e-9, (n, err)


@pytest.mark.gpu
def test_training_through_the_kernels_reduces_the_loss():
    from ava256_amd.trainloop import RaymarchTrainModel, SlabDecoderStandIn, Trainer, make_training_batch
    dev = "cuda"
    batch, volradius = make_training_batch(4, 64, 64, 256, dev, seed=3, target_decoder=SlabDecoderStandIn(256, seed=9))
    model = RaymarchTrainModel(SlabDecoderStandIn(256, seed=1), volradius).to(dev)
    tr = Trainer(model, lr=2e-2)          # larger step than the reference's 2e-4 so that 40 iterations show progress
    first = None
    for it in range(40):
        loss, parts = tr.step(batch)
        if first is None:
            first = float(loss)
    last = float(loss)
    assert np.isfinite(last) and last < 0.8 * first, (first, last)
    for p in tr.params:
        assert torch.isfinite(p).all()


def test_config_reader_takes_the_references_keys(tmp_path):
    """ava-256_amd/config.py reads the keys ddp-train.py reads from configs/config*.yaml (:78,82,321,404-430,441) into the
    Trainer's arguments; `--opts`-style overrides; unknown loss terms are rejected, other sections ignored.  The keys this
    reader takes from the reference's own three files, with their values, are stored in tests/golden/reference_interfaces.json
    (tests/golden/gen_reference_interfaces.py) and read back through the same reader."""
    import json
    import os
    import yaml
    from ava256_amd.config import load_train_config
    from ava256_amd.trainloop import Trainer
    y = tmp_path / "c.yaml"
    y.write_text("device: cuda\ntrain:\n  dataset_dir: /x\n  nids: 4\n  init_learning_rate: 3.0e-4\n  lr_scheduler_iter: 5_000\n"
                 "  gamma: 1.2\n  batchsize: 6\n  clip: 0.5\n  losses:\n    irgbl1: 1.0\n    primvolsum: 0.02\n"
                 "progress:\n  output_path: run/\n")
    c = load_train_config(str(y))
    assert c["trainer"] == {"lr": 3.0e-4, "lr_scheduler_iter": 5000, "gamma": 1.2, "clip": 0.5,
                            "loss_weights": {"irgbl1": 1.0, "primvolsum": 0.02}}
    assert c["batchsize"] == 6 and c["nids"] == 4 and c["other"]["dataset_dir"] == "/x" and "progress" in c["other"]
    c2 = load_train_config(str(y), ["train.clip", "2.0", "train.losses.kldiv", "1e-3"])
    assert c2["trainer"]["clip"] == 2.0 and c2["trainer"]["loss_weights"]["kldiv"] == 1e-3
    tr = Trainer.from_config(torch.nn.Linear(2, 2), c)
    assert tr.clip == 0.5 and tr.optim.param_groups[0]["lr"] == 3.0e-4 and tr.sched.step_size == 5000 and tr.sched.gamma == 1.2
    assert tr.loss_weights == {"irgbl1": 1.0, "primvolsum": 0.02}
    (tmp_path / "bad.yaml").write_text("train:\n  losses:\n    irgbl1: 1.0\n    vgg: 1.0\n")
    with pytest.raises(NotImplementedError):
        load_train_config(str(tmp_path / "bad.yaml"))
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_interfaces.json")) as f:
        ref_configs = json.load(f)["configs"]
    assert sorted(ref_configs) == ["config-256.yaml", "config-4.yaml", "config.yaml"]
    for name, doc in ref_configs.items():
        p = tmp_path / name
        p.write_text(yaml.safe_dump(doc))
        r = load_train_config(str(p))
        tr_ref = doc["train"]
        assert r["trainer"]["lr"] == 2.0e-4 and r["trainer"]["clip"] == 1.0 and r["batchsize"] >= 1
        assert set(r["trainer"]["loss_weights"]) <= {"irgbl1", "vertl1", "kldiv", "primvolsum"}
        assert r["trainer"] == {"lr": tr_ref["init_learning_rate"], "lr_scheduler_iter": tr_ref["lr_scheduler_iter"],
                                "gamma": tr_ref["gamma"], "clip": tr_ref["clip"], "loss_weights": tr_ref["losses"]}
        assert (r["batchsize"], r["nids"], r["maxiter"], r["num_epochs"]) == (
            tr_ref["batchsize"], tr_ref["nids"], tr_ref["maxiter"], tr_ref["num_epochs"])


def test_matrix_form_of_rodrigues_equals_the_per_element_form():
    """trainloop.rodrigues_matrix (whole-matrix operations: an order of magnitude fewer kernels per training iteration) gives
    the values of scene.rodrigues (the reference's per-element Rodrigues statements), at zero rotation too."""
    from ava256_amd.scene import rodrigues
    from ava256_amd.trainloop import rodrigues_matrix
    g = torch.Generator().manual_seed(4)
    v = torch.cat([0.7 * torch.randn(200, 3, generator=g, dtype=torch.float64), torch.zeros(3, 3, dtype=torch.float64)])
    assert (rodrigues(v) - rodrigues_matrix(v)).abs().max().item() <= 1e-14
    v32 = v.float().requires_grad_(True)
    R = rodrigues_matrix(v32)
    assert R.shape == (203, 3, 3) and torch.isfinite(R).all()
    R.sum().backward()
    assert torch.isfinite(v32.grad).all()


def test_gemm_free_small_products_equal_the_matrix_products():
    """trainloop._matmul3 (stacks of 3x3 products as a broadcast product + sum) and trainloop._WideLinear (the geometry head
    with its input gradient as a broadcast product + sum) give what torch.matmul / F.linear give, gradients included."""
    from ava256_amd.trainloop import _matmul3, _WideLinear
    g = torch.Generator().manual_seed(9)
    a = torch.randn(50, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(50, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(50, 3, 3, generator=g, dtype=torch.float64)
    ga, gb = torch.autograd.grad((_matmul3(a, b) * w).sum(), (a, b))
    ra, rb = torch.autograd.grad((torch.matmul(a, b) * w).sum(), (a, b))
    assert (_matmul3(a, b) - torch.matmul(a, b)).abs().max().item() <= 1e-14
    assert (ga - ra).abs().max().item() <= 1e-13 and (gb - rb).abs().max().item() <= 1e-13
    for M in (300, 3072):        # plain product, and the split-over-M form (M a multiple of 1024)
        x = torch.randn(4, 16, generator=g, dtype=torch.float64, requires_grad=True)
        W = torch.randn(M, 16, generator=g, dtype=torch.float64, requires_grad=True)
        bias = torch.randn(M, generator=g, dtype=torch.float64, requires_grad=True)
        u = torch.randn(4, M, generator=g, dtype=torch.float64)
        got = torch.autograd.grad((_WideLinear.apply(x, W, bias) * u).sum(), (x, W, bias))
        ref = torch.autograd.grad((torch.nn.functional.linear(x, W, bias) * u).sum(), (x, W, bias))
        assert (_WideLinear.apply(x, W, bias) - torch.nn.functional.linear(x, W, bias)).abs().max().item() <= 1e-13
        for p_, q_ in zip(got, ref):
            assert (p_ - q_).abs().max().item() <= 1e-11

@pytest.mark.gpu
def test_graph_replay_trains_like_the_eager_loop():
    """Trainer(graph=True): after the eager warm-up iterations of a forward schedule the iteration is one hipGraph replay.
    Same initialisation, same batch, 12 iterations across ... the losses and the parameters follow the eager loop's (the
    placement backward accumulates with fp32 atomics, so not bit for bit: 1e-4 relative on the loss, 1e-3 of the largest
    update on the parameters), the learning-rate scalar the captured Adam reads is the schedule's, and replays happened."""
    from ava256_amd.trainloop import (CodeEncoderStandIn, ColorCalStandIn, RaymarchTrainModel, SlabDecoderStandIn, Trainer,
                                      make_training_batch)
    dev = "cuda"
    batch, volradius = make_training_batch(2, 64, 64, 256, dev, seed=5, target_decoder=SlabDecoderStandIn(256, seed=9))

    def run(graph):
        torch.manual_seed(0)
        model = RaymarchTrainModel(SlabDecoderStandIn(256, seed=1), volradius, colorcal=ColorCalStandIn(80, 4),
                                   encoder=CodeEncoderStandIn()).to(dev)
        tr = Trainer(model, lr=1e-3, lr_scheduler_iter=5, gamma=0.5, graph=graph, graph_warmup=2)
        losses = []
        for _ in range(12):
            loss, parts = tr.step(batch)
            losses.append(float(loss))
        return tr, losses, [p.detach().clone() for p in tr.params]

    te, le, pe = run(False)
    tg, lg, pg = run(True)
    assert tg.graph and tg.graph_replays == 10 and te.graph_replays == 0
    assert abs(float(tg._lr_dev) - 1e-3 * 0.25) <= 1e-9 and abs(te.optim.param_groups[0]["lr"] - 1e-3 * 0.25) <= 1e-12
    for a, b in zip(le, lg):
        assert np.isfinite(b) and abs(a - b) <= 1e-4 * abs(a), (le, lg)
    for a, b in zip(pe, pg):
        assert (a - b).abs().max().item() <= 1e-3 * 12 * 1e-3 + 1e-6 * a.abs().max().item()
    assert torch.isfinite(tg.last_grad_norm).all()


@pytest.mark.gpu
def test_graph_is_recaptured_only_when_a_new_capture_would_get_larger_lists(monkeypatch):
    """The captured iteration freezes the primitive-list capacity.  A raised list-overflow flag drops the graph only when
    the capacity feedback would NOW choose a larger capacity than the captured one; a flag the capacity policy itself leaves
    raised for good (outlier clipping, memory budget, the cap of 2048) must not cost a re-capture every 64 replays -- the
    interval between looks doubles instead (advisor, round 5)."""
    import importlib
    mm = importlib.import_module("ava256_amd.mvpraymarch")   # (the package re-exports a FUNCTION of that name)
    from ava256_amd.trainloop import (CodeEncoderStandIn, ColorCalStandIn, RaymarchTrainModel, SlabDecoderStandIn, Trainer,
                                      make_training_batch)
    dev = "cuda"
    batch, volradius = make_training_batch(2, 64, 64, 256, dev, seed=5, target_decoder=SlabDecoderStandIn(256, seed=9))
    torch.manual_seed(0)
    model = RaymarchTrainModel(SlabDecoderStandIn(256, seed=1), volradius, colorcal=ColorCalStandIn(80, 4),
                               encoder=CodeEncoderStandIn()).to(dev)
    tr = Trainer(model, lr=1e-3, graph=True, graph_warmup=2)
    tr.graph_check_every = 2
    real_capacity, real_wanted = mm.primlist_capacity, mm.capacity_wanted_now
    monkeypatch.setattr(mm, "primlist_capacity", lambda H, W, K, device=None, N=None: 4)   # lists far below the demand
    for _ in range(3):                       # two eager iterations, then the capture (its first replay)
        tr.step(batch)
    (st,) = tr._graphs.values()
    pl_count, nk, shape = st["handoff"]
    assert shape == (2, 64, 64, 256, 4) and int(pl_count[nk].item()) & 1, "the scene must overflow lists of 4 entries"
    # (a) the policy would choose the same capacity again: no re-capture, and the looks thin out
    monkeypatch.setattr(mm, "capacity_wanted_now", lambda *a: 4)
    for _ in range(12):
        tr.step(batch)
    assert tr.graph_recaptures == 0 and len(tr._graphs) == 1 and st["check_every"] >= 8
    # (b) the policy would choose a larger capacity: the graph is dropped at the next look, the eager iterations size their
    # lists from the measurement that look has noted, and the new graph's forward no longer overflows
    monkeypatch.setattr(mm, "capacity_wanted_now", real_wanted)
    monkeypatch.setattr(mm, "primlist_capacity", real_capacity)
    for _ in range(st["check_every"] + 1):
        tr.step(batch)
    assert tr.graph_recaptures == 1
    for _ in range(4):
        tr.step(batch)
    (st2,) = tr._graphs.values()
    pl2, nk2, shape2 = st2["handoff"]
    assert shape2[4] > 4 and (int(pl2[nk2].item()) & 1) == 0
    assert np.isfinite(float(tr.step(batch)[0]))
