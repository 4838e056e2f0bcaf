"""Timing of the DeepLabv2-Resnet101-ProDA model (``framework/model/deeplabv2_proda.py``), all in this process on the same device:

  (a) one train-mode forward + backward (upsample -> cross-entropy loss) at 512 x 1024, batch 4, "f16x2", with the BatchNorm affine
      parameters TRAINABLE (``onda_bn_bwd_affine_l2`` / ``onda_bn_pair_bwd_affine_l2`` / ``onda_bn_bwd_affine``) against
      ``freeze_bn=True`` (the frozen entry points): device time between two events around 5 passes, the two models alternating,
      4 rounds each after 3 warm-up passes each; with the number of library entry-point calls of one pass of each.  The affine
      calls launch what the frozen ones launch and write 2 * C more floats each: no difference beyond the spread is expected, and
      a difference beyond it means a launch or a pass was added.
  (b) one ``hybrid_proDA`` step (+ ``update_ema``) of the trainable model at the same size: median of 10 after 3 warm-up steps.

    python tools/proda101_timing.py
"""
import os, sys, statistics, tempfile, time, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from onda_amd import _lib, ops
from onda_amd.config import hybrid_switch_cfg
from onda_amd.framework.domain_adaptation.methods.adaptation_model import switch_batch_statistics
from onda_amd.framework.handlers import get_adapt_method, get_model, model_handler
from onda_amd.framework.model.deeplabv2_proda import Deeplab
from onda_amd.synthetic import fill_state_dict, synth_batch

DEV = "cuda:0"
B, H, W = 4, 512, 1024
PASSES = 5


def count_calls():
    """Wrap `call` wherever an onda_amd module holds it; returns (names list, undo)."""
    names, real, held = [], _lib.call, []

    def spy(name, *args):
        names.append(name)
        return real(name, *args)
    for mod in list(sys.modules.values()):
        if getattr(mod, "__name__", "").startswith("onda_amd") and getattr(mod, "call", None) is real:
            mod.call = spy
            held.append(mod)

    def undo():
        for mod in held:
            mod.call = real
    return names, undo


def build(freeze_bn):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (no cached ImageNet file: synthetic weights below)
        m = Deeplab(torch.nn.BatchNorm2d, num_classes=19, freeze_bn=freeze_bn).to(DEV)
    fill_state_dict(m, 1, 3.0)
    return m.train()


def main():
    ops.CONV_MODE = "f16x2"
    batch = synth_batch(B, H, W)
    image, label = batch["image"].to(DEV), batch["label"].to(DEV)
    models = {"trainable affine": build(False), "freeze_bn=True": build(True)}

    def one_pass(m):
        for p in m.parameters():
            p.grad = None
        ops.upsample_ce(m(image)[1]["out"], label).backward()

    def passes(m, n=PASSES):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            one_pass(m)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n

    for name, m in models.items():
        for _ in range(3):
            one_pass(m)
        names, undo = count_calls()
        one_pass(m)
        undo()
        torch.cuda.synchronize()
        affine = sum("affine" in n for n in names)
        print(f"{name}: {len(names)} library calls a pass, {affine} of them affine BatchNorm backward calls, "
              f"{sum(n in ('onda_bn_bwd', 'onda_bn_bwd_l2', 'onda_bn_pair_bwd_l2') for n in names)} frozen ones", flush=True)
    times = {name: [] for name in models}
    for rnd in range(4):
        for name, m in models.items():
            ms = passes(m)
            times[name].append(ms)
            print(f"round {rnd}: forward + backward {H} x {W}, batch {B}, {name}: {ms:.2f} ms a pass (device, {PASSES} passes)", flush=True)
    for name, ts in times.items():
        print(f"{name}: median {statistics.median(ts):.2f} ms, min {min(ts):.2f}, max {max(ts):.2f}", flush=True)
    del models
    torch.cuda.empty_cache()

    # (b): a hybrid_proDA step of the trainable model
    model_handler.enable_resnet101_proda()
    with tempfile.TemporaryDirectory() as tmp:
        cfg, spec = hybrid_switch_cfg(W, H, DEV, tmp, batch_size=B)
        cfg.MODEL.NAME = "DeepLabv2-Resnet101-ProDA"
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model = get_model(cfg, 19)
        fill_state_dict(model, 1, 3.0)
        da = get_adapt_method(cfg)(model, cfg, spec)
        src = [synth_batch(B, H, W, seed=100 + i) for i in range(2)]
        trg = [synth_batch(B, H, W, seed=200 + i) for i in range(2)]
        torch.manual_seed(123)
        da.update_dynamic()
        switch_batch_statistics(da.model, False)
        da.calculate_prototypes(src[:1], save=False)
        switch_batch_statistics(da.model, True)
        da.optimizer.zero_grad()

        def step(i):
            da.adjust_learning_rate(i, 1000)
            da.step([src[i % 2]], trg[i % 2])
            da.update_ema()

        for i in range(3):
            step(i)
        ts = []
        for i in range(3, 13):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(i)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        names, undo = count_calls()
        step(13)
        undo()
        print(f"hybrid_proDA step {H} x {W}, batch {B}, DeepLabv2-Resnet101-ProDA: median {statistics.median(ts):.2f} ms (min {min(ts):.2f}, "
              f"max {max(ts):.2f}); {len(names)} library calls a step, {sum('affine' in n for n in names)} of them affine BatchNorm backward calls",
              flush=True)


if __name__ == "__main__":
    main()
