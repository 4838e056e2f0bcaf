"""The validation pass of source pre-training against the reference's own numbers (fixture G31, made by
tests/golden/make_golden_eval.py from the reference's evaluate_model): eval_UDA.evaluate_model on the composed route (CPU, runs
anywhere) and on the fused kernel (GPU), SegmentationTrainer.validate, train()'s log keys, Segmentation_db's `label_raw`, and the
`prototype=` route.  Every pixel of G31 has a top-2 margin of at least 1e-4, so the IoU vectors are compared for equality."""
import numpy as np
import pytest
import torch
from torch import nn

import eval_fp64 as V

DEV = "cuda:0"
gpu = pytest.mark.gpu


class StandIn(nn.Module):
    """Returns its input as the model's main output: a batch's "image" is the low-resolution logits."""

    def forward(self, x):
        return None, {"out": x, "feat": x}


def _loader(g):
    return [{"image": torch.from_numpy(g[f"x{i}"]), "label": torch.from_numpy(g[f"label{i}"]),
             "label_raw": torch.from_numpy(g[f"label_raw{i}"])} for i in range(3)]


def _against_g31(g, device):
    from onda_amd.config import Cfg
    from onda_amd.framework.domain_adaptation.eval_UDA import evaluate_model
    cfg = Cfg.from_dict({"device": device, "NUM_CLASSES": 19})
    loader = _loader(g)
    assert [b["image"].shape[0] for b in loader] == [2, 2, 1] and float(g["margin"]) >= 1e-4
    size, size_org = tuple(g["size"].tolist()), tuple(g["size_org"].tolist())
    model = StandIn().train()
    iou, entropy = evaluate_model(model, loader, nn.Upsample(size=size, mode="bilinear", align_corners=True), cfg, return_entropy=True)
    assert model.training and isinstance(iou, np.ndarray) and iou.shape == (19,)
    assert np.array_equal(iou, g["iou"])
    V.check_mean(entropy, float(g["entropy64"]), f"G31 on {device}, against float64")
    print(f"the reference's own float32 entropy: {float(g['entropy']):.12g}")
    iou2, iou_org = evaluate_model(model, loader, size, cfg, intrp_org=size_org)  # (H, W) pairs are taken as well
    assert np.array_equal(iou2, g["iou"]) and np.array_equal(iou_org, g["iou_org"])
    out = evaluate_model(model, loader, size, cfg)
    assert isinstance(out, tuple) and len(out) == 1 and np.array_equal(out[0], g["iou"])
    iou3, entropy3, iou_org3 = evaluate_model(model, loader, size, cfg, return_entropy=True, intrp_org=size_org)
    assert np.array_equal(iou3, g["iou"]) and np.array_equal(iou_org3, g["iou_org"]) and entropy3 == entropy
    # the mean over the batches is unweighted: a mean weighted by the frames is another number
    weighted = float(np.average([V.restate(b["image"], b["label"])[2] for b in loader], weights=[2, 2, 1]))
    assert V.flagged(V.check_mean, weighted, float(g["entropy64"]), "probe")
    # labels of another size, a loader without `label_raw`
    with pytest.raises(RuntimeError):
        evaluate_model(model, loader, (size[0] + 1, size[1]), cfg)
    with pytest.raises(KeyError):
        evaluate_model(model, [{k: v for k, v in loader[0].items() if k != "label_raw"}], size, cfg, intrp_org=size_org)


def test_evaluate_model_composed_against_the_reference(golden):
    _against_g31(golden("g31_evaluate_model"), "cpu")


@gpu
def test_evaluate_model_fused_against_the_reference(golden, monkeypatch):
    from onda_amd.ops import loss as oloss
    seen = []
    real = oloss.call

    def spy(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(oloss, "call", spy)
    _against_g31(golden("g31_evaluate_model"), DEV)
    assert "onda_upsample_eval" in seen and "onda_upsample_fwd" not in seen, sorted(set(seen))


# ------------------------------------------------------------------------------------------------ trainer, train(), loader
@pytest.fixture(scope="module")
def model():
    from onda_amd.config import hybrid_switch_cfg
    from onda_amd.framework.handlers import get_model
    from onda_amd.synthetic import fill_state_dict
    m = get_model(hybrid_switch_cfg(128, 64, DEV, "NONE", batch_size=2)[0], 19)
    fill_state_dict(m, 1, 3.0)
    return m


def _val_loader():
    """Two batches of 2 and 1 frames at 64x128 with `label_raw` at 128x256."""
    from onda_amd.synthetic import synth_batch
    out = []
    for i, b in enumerate((2, 1)):
        batch = synth_batch(b, 64, 128, seed=400 + i)
        raw = torch.randint(0, 21, (b, 128, 256), generator=torch.Generator().manual_seed(500 + i)).to(torch.uint8)
        raw[raw >= 19] = 255
        batch["label_raw"] = raw
        out.append(batch)
    return out


@gpu
def test_trainer_validate_against_the_composed_route(model, monkeypatch):
    """SegmentationTrainer.validate at 64x128 with ORIGINAL_RES = [256, 128] against the same evaluate_model with
    ops.upsample_eval on its composed route (UpsampleFn, torch.softmax, the expression, .mean()).  The model's evaluation
    forward is deterministic, so both see the same logits: the IoU vectors are equal (one kernel family counts both), and
    each entropy is within BOUND of the float64 value, the two of each other within twice that."""
    from onda_amd.config import hybrid_switch_cfg
    from onda_amd.framework.domain_adaptation.methods.segmentation import SegmentationTrainer
    from onda_amd.ops import loss as oloss
    cfg, spec = hybrid_switch_cfg(128, 64, DEV, "NONE", batch_size=2)
    loader = _val_loader()
    tr = SegmentationTrainer(model.train(), cfg, spec)
    iou_plain, entropy_plain = tr.validate(loader)  # ORIGINAL_RES unset
    cfg.SCHEME.ORIGINAL_RES = [256, 128]
    assert tr.original_size == (128, 256)
    iou, entropy, iou_full = tr.validate(loader)
    assert model.training and iou.shape == iou_full.shape == (19,) and np.isfinite(entropy) and 0.0 < entropy < 1.0 / 19 + 1e-6
    assert np.array_equal(iou, iou_plain) and entropy == entropy_plain
    assert np.array_equal(iou, tr.evaluate(loader))  # the existing entry point: the same matrix
    assert not np.array_equal(iou, iou_full)
    monkeypatch.setattr(oloss, "EVAL_FUSED", False)
    seen = []
    real = oloss.call

    def spy(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(oloss, "call", spy)
    iou_c, entropy_c, iou_full_c = tr.validate(loader)
    assert "onda_upsample_eval" not in seen and "onda_upsample_fwd" in seen
    assert np.array_equal(iou, iou_c) and np.array_equal(iou_full, iou_full_c)
    V.check_mean(entropy, entropy_c, "validate, fused against composed", factor=2.0)


@gpu
def test_train_logs_the_four_validation_keys(model, tmp_path):
    from onda_amd import logging as olog
    from onda_amd.config import hybrid_switch_cfg
    from onda_amd.framework.domain_adaptation.methods import segmentation
    from onda_amd.synthetic import synth_batch
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    logs = []
    olog.set_sink(logs.append)
    try:
        for res in (None, [256, 128]):
            cfg, spec = hybrid_switch_cfg(128, 64, DEV, str(tmp_path), batch_size=2)
            cfg.SCHEME.SOURCE = "synthetic"
            spec.EPOCHS = 1
            if res is not None:
                cfg.SCHEME.ORIGINAL_RES = res
            del logs[:]
            segmentation.train(model, [synth_batch(2, 64, 128, seed=7)], {"val": _val_loader()}, cfg, spec)
            report = [d for d in logs if "epoch" in d]
            assert len(report) == 1
            want = {"epoch", "Val mIoU of val", "Val std IoU of val", "val entropy of val"} | ({"Val mIoU full image of val"} if res else set())
            assert set(report[0]) == want, sorted(report[0])
            assert all(np.isfinite(report[0][k]) for k in want)
            print(report[0])
    finally:
        olog.set_sink(None)
        model.load_state_dict(state)


@gpu
def test_segmentation_db_original_label(tmp_path):
    """Three 90x160 PNGs (the recipe of the pipeline test): `label_raw` is the id map on the raw label; the other fields are
    what the default loader returns; frames of two native sizes in one batch raise."""
    import pandas as pd
    from PIL import Image
    from onda_amd.framework.dataset.segmentation_db import Segmentation_db
    rng = np.random.default_rng(3)
    rows, raw = [], []
    for i in range(3):
        img = rng.integers(0, 256, (90, 160, 3), dtype=np.uint8)
        lab = rng.integers(0, 34, (90, 160), dtype=np.uint8)
        Image.fromarray(img).save(tmp_path / f"i{i}.png")
        Image.fromarray(lab).save(tmp_path / f"l{i}.png")
        rows.append({"image_path": f"i{i}.png", "label_path": f"l{i}.png"})
        raw.append(lab)
    ids = {i: (i % 19 if i % 3 else 255) for i in range(34)}
    lut = np.zeros(256, np.int64)
    for s, t in ids.items():
        lut[s] = t
    ds = Segmentation_db(str(tmp_path), pd.DataFrame(rows), ids, (64, 32), original_label=True)
    plain = Segmentation_db(str(tmp_path), pd.DataFrame(rows), ids, (64, 32))
    samples = next(iter(torch.utils.data.DataLoader(ds, batch_size=3, num_workers=0, collate_fn=lambda s: s)))
    batch, default = ds.gpu_collate(samples), plain.gpu_collate(samples)
    assert set(batch) == set(default) | {"label_raw"} and "label_raw" not in default
    for k in ("image", "label", "label_res"):
        assert torch.equal(batch[k], default[k])
    got = batch["label_raw"]
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 90, 160) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), np.stack([lut[l].astype(np.uint8) for l in raw]))
    Image.fromarray(rng.integers(0, 34, (80, 160), dtype=np.uint8)).save(tmp_path / "l2.png")
    samples = next(iter(torch.utils.data.DataLoader(ds, batch_size=3, num_workers=0, collate_fn=lambda s: s)))
    with pytest.raises(RuntimeError, match="one native size"):
        ds.gpu_collate(samples)
    assert "label_raw" not in plain.gpu_collate(samples)


# ------------------------------------------------------------------------------------------------ the prototype route
@gpu
def test_prototype_route_against_the_composed_route(monkeypatch):
    """`prototype=` with a dict output: the map is prototype.pseudo_labels(feat, prior, soft=True), an [N,19] soft map whose rows
    go in with shape=(B, h, w); the entropy takes a softmax of the interpolated probabilities again, as the reference does.
    Fused against composed on the same map: equal IoU, entropies within twice BOUND."""
    from onda_amd.framework.domain_adaptation.eval_UDA import evaluate_model
    from onda_amd.config import Cfg
    from onda_amd.framework.domain_adaptation.methods import prototype_handler as PH
    from onda_amd.ops import loss as oloss
    from onda_amd.synthetic import synth_prototypes
    proto = PH.prototype_handler(0.9995, 1, 0.3, "mahalanobis")
    state = synth_prototypes(256, 19)
    proto.prototypes, proto.squared_mean, proto.counter = (t.clone().to(DEV) for t in state)
    g = torch.Generator().manual_seed(9)
    B, h, w, size = 2, 9, 17, (33, 65)

    class WithFeatures(nn.Module):
        def forward(self, x):
            return None, {"out": x[:, :19], "feat": x}
    loader = []
    for i in range(2):
        cls = torch.randint(0, 19, (B, h, w), generator=g)
        feat = state[0][cls].permute(0, 3, 1, 2) + 0.8 * torch.randn(B, 256, h, w, generator=g)
        lab = torch.randint(0, 21, (B,) + size, generator=g).to(torch.uint8)
        lab[lab >= 19] = 255
        batch = {"image": feat.contiguous(), "label": lab}
        if i == 1:
            batch["soft_predictions"] = torch.softmax(torch.randn(B, 19, h, w, generator=g), 1)
        loader.append(batch)
    cfg = Cfg.from_dict({"OTHERS": {"DEVICE": DEV}, "NUM_CLASSES": 19})
    seen = []
    real = oloss.call

    def spy(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(oloss, "call", spy)
    iou, entropy = evaluate_model(WithFeatures(), loader, size, cfg, return_entropy=True, prototype=proto)
    assert seen.count("onda_upsample_eval") == 2
    monkeypatch.setattr(oloss, "EVAL_FUSED", False)
    iou_c, entropy_c = evaluate_model(WithFeatures(), loader, size, cfg, return_entropy=True, prototype=proto)
    assert seen.count("onda_upsample_eval") == 2 and np.array_equal(iou, iou_c) and float(np.nanmean(iou)) > 0.0
    V.check_mean(entropy, entropy_c, "prototype route, fused against composed", factor=2.0)
    # the map is a probability map: the second softmax flattens it, the entropy is near its maximum 1 / K per element
    assert 0.9 / 19 < entropy <= 1.0 / 19 + 1e-6
