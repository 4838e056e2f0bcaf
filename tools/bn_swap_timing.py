"""Timing of ``batchnorm_stats.exchange()`` -- the two BatchNorm state sets of PROTO_ADVENT and BN_POLICY "double" changing places --
as one ``onda_swap_multi`` launch against the copying route (``deepcopy(state_dict())`` + ``load_state_dict`` per BatchNorm, kept
behind ``ONDA_BN_SWAP=0``), both in this process on the same device:

  (a) device time between two events around 20 ``exchange()`` calls on the ResNet-50 model (53 BatchNorms, 265 tensors),
  (b) host wall time of the same 20 calls (the host is what a step waits for: nothing else is queued around an exchange),
  (c) a PROTO_ADVENT step (``adv_proDA.step`` + ``update_ema``) at 512 x 1024, batch 4, "f16x2": median of 10 after 3 warm-up steps,
      with the number of library entry-point calls of one step (a spy on ``_lib.call`` as the ops modules hold it).

    python tools/bn_swap_timing.py

The routes alternate, three rounds each for (a) / (b); the step runs the launch route first, then the copying route, then the
launch route again."""
import os, sys, statistics, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from onda_amd import _lib, ops
from onda_amd.config import hybrid_switch_cfg
from onda_amd.framework.domain_adaptation.methods.adaptation_model import batchnorm_stats, switch_batch_statistics
from onda_amd.framework.domain_adaptation.methods.prototype_advent import adv_proDA
from onda_amd.framework.handlers import get_model
from onda_amd.synthetic import fill_state_dict, synth_batch

DEV = "cuda:0"
B, H, W = 4, 512, 1024
ROUTES = {"one launch": "1", "copies (ONDA_BN_SWAP=0)": "0"}


def exchanges(bn, n=20):
    """(device us, host us) of n exchange() calls."""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(n):
        bn.exchange()
    b.record()
    host = time.perf_counter() - t0
    b.synchronize()
    return a.elapsed_time(b) * 1e3, host * 1e6


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


def main():
    ops.CONV_MODE = "f16x2"
    with tempfile.TemporaryDirectory() as tmp:
        cfg, spec = hybrid_switch_cfg(W, H, DEV, tmp, batch_size=B)
        cfg.METHOD.ADAPTATION.NAME = "PROTO_ADVENT"
        spec.pop("GRAY_AREA", None)
        for k, v in dict(SWITCH_PRIOR_THRESH=0.86, SOFT_TRANS=True, LAMBDA_ADV_AUX=0.0002, LAMBDA_SEG_AUX=0.1, LAMBDA_ADV_MAIN=0.001,
                         LAMBDA_SEG_MAIN=1).items():
            spec[k] = v
        model = get_model(cfg, 19)
        fill_state_dict(model, 1, 3.0)
        # (a), (b): the exchange alone
        bn = batchnorm_stats(model)
        pairs = sum(len(v) for v in bn.memory.values())
        print(f"{len(bn.memory)} BatchNorms, {pairs} tensor pairs, "
              f"{sum(t.numel() * t.element_size() for v in bn.memory.values() for t in v.values()) / 1e3:.0f} kB a set", flush=True)
        for env in ROUTES.values():  # warm-up of both routes
            os.environ["ONDA_BN_SWAP"] = env
            exchanges(bn, 4)
        for rnd in range(3):
            for route, env in ROUTES.items():
                os.environ["ONDA_BN_SWAP"] = env
                dev_us, host_us = exchanges(bn)
                print(f"round {rnd}: 20 x exchange(), {route}: device {dev_us:.0f} us, host {host_us:.0f} us", flush=True)
        # (c): the step
        torch.manual_seed(77)
        da = adv_proDA(model, cfg, spec)
        src = [synth_batch(B, H, W, seed=100 + i) for i in range(2)]
        trg = [synth_batch(B, H, W, seed=200 + i) for i in range(2)]
        torch.manual_seed(123)
        da.proto_model.update_dynamic()
        switch_batch_statistics(model, False)
        da.proto_model.calculate_prototypes(src[:1], save=False)
        switch_batch_statistics(model, True)
        da.advent.optimizer.zero_grad()

        def step(i):
            da.advent.adjust_learning_rate(i, 1000)
            log = da.step(src[i % 2], trg[i % 2])
            da.proto_model.update_ema()
            return log

        def timed(i):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(i)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        i = 0
        for route, env in list(ROUTES.items()) + [("one launch", "1")]:
            os.environ["ONDA_BN_SWAP"] = env
            for _ in range(3):
                step(i)
                i += 1
            ts = []
            for _ in range(10):
                ts.append(timed(i))
                i += 1
            names, undo = count_calls()
            step(i)
            i += 1
            undo()
            print(f"PROTO_ADVENT step {H} x {W}, batch {B}, {route}: median {statistics.median(ts):.2f} ms (min {min(ts):.2f}, max "
                  f"{max(ts):.2f}); {len(names)} library calls a step, {names.count('onda_swap_multi')} of them onda_swap_multi", flush=True)
    os.environ.pop("ONDA_BN_SWAP", None)


if __name__ == "__main__":
    main()
