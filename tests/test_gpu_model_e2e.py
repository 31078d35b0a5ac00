"""The whole paper model (version 0.4.0) in the opt-in end-to-end mode, float32, B = 1 at 192x224
(a size at which every Swin layer runs on the kernels): by default no encoder parameter receives
a gradient (the reference detaches the Swin maps, custom_model.py:332-333, Q1); after
set_end_to_end(True) the encoder trains through the fused hot path -- the parameters the RGB
baseline (version 0.0.0, whose encoder is not detached) trains on the same RGB input -- the
colour-map gradients obey the closed form at scale 3, nothing about the state_dict changes, and
the step still captures into a graph of at most two concurrent branches."""
import re

import numpy as np
import pytest
import torch

import _rgbd_import  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
B, H, W = 1, 192, 224


def _model(version):
    from rgbd_amd import init as winit
    from rgbd_amd.config import standard_config
    from rgbd_amd.custom_model import CustomMask2FormerForUniversalSegmentation
    torch.manual_seed(0)
    m = CustomMask2FormerForUniversalSegmentation(standard_config(48), version=version)
    winit.init_deterministic(m)
    return m.to(DEV).eval()  # eval: with B = 1 an active DropPath zeroes a layer's whole branch


@pytest.fixture(scope="module")
def batch():
    from rgbd_amd import ops, synthetic
    scenes = [synthetic.make_scene(synthetic.scene_seed(4, i), H, W) for i in range(B)]
    depth = torch.from_numpy(np.stack([s["depth_u8"] for s in scenes])).to(DEV)
    rgb = torch.from_numpy(np.stack([s["rgb_u8"] for s in scenes])).contiguous().to(DEV)
    labels = dict(mask_labels=[torch.from_numpy(s["masks"].astype(np.float32)).to(DEV) for s in scenes],
                  class_labels=[torch.from_numpy(s["classes"]).to(DEV) for s in scenes])
    return ops.assemble_pixel_values(depth, rgb), labels


@pytest.fixture(scope="module")
def paper():
    return _model("0.4.0")


def _encoder(m):
    return m.model.pixel_level_module.encoder


def _step(m, pv, labels):
    m.zero_grad(set_to_none=True)
    out = m(pixel_values=pv, **labels)
    out.loss.backward()
    return out.loss.detach()


def test_default_gives_the_encoder_no_gradient(paper, batch):
    pv, labels = batch
    assert paper.model.pixel_level_module.end_to_end is False
    loss = _step(paper, pv, labels)
    assert torch.isfinite(loss)
    got = [n for n, p in _encoder(paper).named_parameters() if p.grad is not None]
    assert not got, f"encoder parameters with a gradient in the default mode: {got[:5]}"
    assert paper.model.pixel_level_module.dsam0.rgb_projection.weight.grad is not None


def test_end_to_end_trains_the_encoder(paper, batch):
    pv, labels = batch
    keys = list(paper.state_dict().keys())
    plm = paper.model.pixel_level_module
    seen = {}
    inner = plm.hot_path_features

    def spy(pixel_values, color_feature_map, **kw):
        for c in color_feature_map:
            c.retain_grad()
        feats = inner(pixel_values, color_feature_map, **kw)
        seen["colors"], seen["kw"], seen["G"] = list(color_feature_map), kw, [None] * 4
        for k, f in enumerate(feats):
            f.register_hook(lambda g, k=k: seen["G"].__setitem__(k, g.detach().clone()))
        return feats
    assert paper.set_end_to_end(True) is paper and plm.end_to_end is True
    plm.hot_path_features = spy
    try:
        loss = _step(paper, pv, labels)
    finally:
        del plm.hot_path_features
        paper.set_end_to_end(False)
    assert torch.isfinite(loss) and seen["kw"]["color_grads"] is True
    assert list(paper.state_dict().keys()) == keys
    # the colour-map gradients: d c_3 = 2 G_3 exactly, d c_k = G_k + d cp1_k
    G, dc = seen["G"], [c.grad for c in seen["colors"]]
    assert all(g is not None for g in G) and all(d is not None for d in dc)
    assert torch.equal(dc[3], 2 * G[3])
    for k in range(3):
        assert torch.isfinite(dc[k] - G[k]).all() and (dc[k] - G[k]).any()
    # the encoder's parameters: the RGB baseline says which ones a loss reaches
    base = _model("0.0.0")
    _step(base, pv[:, 0:3].contiguous(), labels)
    reached = [n for n, p in _encoder(base).named_parameters() if p.grad is not None]
    del base
    assert len(reached) > 100
    grads = dict((n, p.grad) for n, p in _encoder(paper).named_parameters())
    bad = [n for n in reached if grads[n] is None or not torch.isfinite(grads[n]).all()]
    assert not bad, f"encoder parameters without a finite gradient: {bad[:8]}"
    stages = {}
    for n in reached:
        mt = re.search(r"layers\.(\d+)\.", n)
        if mt:
            stages[int(mt.group(1))] = stages.get(int(mt.group(1)), False) or bool(grads[n].any())
    assert sorted(stages) == [0, 1, 2, 3] and all(stages.values()), stages


def test_version_0_0_0_ignores_the_flag(batch):
    pv, labels = batch
    m = _model("0.0.0")
    rgb = pv[:, 0:3].contiguous()
    _step(m, rgb, labels)
    want = [None if p.grad is None else p.grad.clone() for p in _encoder(m).parameters()]
    m.set_end_to_end(True)
    _step(m, rgb, labels)
    got = [p.grad for p in _encoder(m).parameters()]
    assert all((a is None) == (b is None) for a, b in zip(want, got))
    assert any(a is not None for a in want)


def test_end_to_end_step_captures(paper, batch, monkeypatch):
    from rgbd_amd.optim import HF_TRAINER_ADAMW, HipAdamW
    from rgbd_amd.train_graph import CapturedTrainStep
    pv, labels = batch
    # A Trainer test earlier in the same process leaves accelerate's PartialState initialised; the
    # loss then takes the library's get_num_masks (a host copy, its all-reduce branch), which no
    # capture admits.  This test is about a single process without accelerate: say so.
    try:
        from accelerate import PartialState
        monkeypatch.setattr(PartialState, "_shared_state", {})
    except ImportError:
        pass
    paper.zero_grad(set_to_none=True)
    paper.set_end_to_end(True).train()
    try:
        opt = HipAdamW([p for p in paper.parameters() if p.requires_grad], **HF_TRAINER_ADAMW)

        def fb():
            out = paper(pixel_values=pv, **labels)
            out.loss.backward()
            return out.loss.detach()
        step = CapturedTrainStep(fb, opt, warmup=1)
        assert step.width <= 2
        enc = {n: p.detach().clone() for n, p in _encoder(paper).named_parameters()}
        loss = step()
        torch.cuda.synchronize()
        paper.model.pixel_level_module.check_statuses()
        assert torch.isfinite(loss)
        moved = [n for n, p in _encoder(paper).named_parameters() if not torch.equal(p.detach(), enc[n])]
        assert len(moved) > 100, f"a replay moved {len(moved)} encoder parameters"
        assert {int(mt.group(1)) for n in moved for mt in [re.search(r"layers\.(\d+)\.", n)] if mt} == {0, 1, 2, 3}
        del step
    finally:
        paper.set_end_to_end(False).eval()
        paper.zero_grad(set_to_none=True)
