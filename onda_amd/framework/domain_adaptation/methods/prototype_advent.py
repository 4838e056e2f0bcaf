"""Drop-in for ``framework/domain_adaptation/methods/prototype_advent.py`` (``adv_proDA``, :14-198): ``PROTO_ADVENT``, the
confidence-switch prototype method and the ADVENT baseline on ONE segmentation network -- a supervised source pass, a target pass
whose loss is the prototype pseudo-label loss plus ADVENT's adversarial term, and a discriminator pass over both domains.

It is a composition: ``proto_model`` is an ``hswitch_proDA`` and ``advent`` an ``advent`` over the same model object, built in that
order (the three deep copies of the model come before anything else, and the discriminators draw their initial weights from the
torch RNG after them).  ``advent.optimizer`` is the one that steps.

BatchNorm state sets.  The method keeps two complete sets: the model holds the TARGET statistics, ``advent.bn.memory`` the SOURCE
ones, and ``advent.bn.exchange()`` swaps them around the source pass (:32, :44) -- on the GPU one ``onda_swap_multi`` launch each
(``adaptation_model.batchnorm_stats``).  Nothing freezes running statistics in the step: each set tracks its own domain.

What runs where is what ``advent_da`` and ``prototypes`` say: source loss ``ops.upsample_ce``, entropy maps ``ops.upsample_entropy``
(the target maps of the adversarial pass reused detached by the discriminator pass, the source maps computed once without a graph),
the low-resolution target loss on the fused kernels ``online_proDA._target_terms`` selects.  The reference adds no EWC term in this
step (:82-96), so none is added here.  Dropout2d masks are drawn where the passes run: source student, target student, teacher.

One GPU, one stream (``advent``'s constructor raises with ``onda_amd.dist`` active).  ``SOFT_LABELS`` (:24-29, :56-81) takes the
soft-label kernels through ``_target_terms``, as in the prototype methods.
"""
import torch

from onda_amd import logging as olog
from onda_amd.config import unset
from onda_amd.framework.domain_adaptation.methods.adaptation_model import switch_batch_statistics
from onda_amd.framework.domain_adaptation.methods.advent_da import _out, advent
from onda_amd.framework.domain_adaptation.methods.prototypes import _Cycle
from onda_amd.framework.domain_adaptation.methods.prototypes_hswitch import hswitch_proDA


def _detached(value):
    return value.detach() if torch.is_tensor(value) else value


class adv_proDA:
    def __init__(self, model, cfg, cfg_spec) -> None:
        self.proto_model = hswitch_proDA(model, cfg, cfg_spec)
        self.advent = advent(model, cfg, cfg_spec)

    def update_cfg_spec(self, cfg_spec):
        self.proto_model.update_cfg_spec(cfg_spec)
        self.advent.update_cfg_spec(cfg_spec)

    def step(self, batch_source, batch_target):
        """One learning step (:23-152), in the reference's order."""
        proto, adv = self.proto_model, self.advent
        spec = proto.cfg_spec
        proto._soft_labels()  # (SOFT_LABELS with JS_D > 0 raises here, before anything is launched)
        # supervised loss, on the source statistics
        adv.bn.exchange()
        adv.discriminator_grad(False)
        pred_src_aux, pred_src_main = adv.model(batch_source["image"].to(adv.device))
        out_src_aux, out_src_main = _out(pred_src_aux), _out(pred_src_main)
        loss_seg_src = adv.supervised_loss(out_src_aux, out_src_main, batch_source["label"])
        loss_seg_src.backward()
        adv.bn.exchange()

        image = proto._device_image(batch_target)  # (prototype_predictions reads the same upload)
        pred_trg_aux, pred_trg_main = adv.model(image)
        out_trg = _out(pred_trg_main)
        # prototypical pseudolabeling
        proto_pred = proto.prototype_predictions(batch_target)
        proto._img_cache = None
        proto.prototypes.ma(proto_pred["ema_model"]["feat"], proto_pred["ema_model"]["out"])
        batch_size, channels, w, h = out_trg.size()
        predictions = proto_pred["pseudolabels"].reshape(batch_size, w, h)
        total_loss, terms = proto._target_terms(out_trg, predictions, proto_pred["soft_predictions"])

        # adversarial training
        ent_trg_aux, ent_trg_main = adv.entropy_map(_out(pred_trg_aux)), adv.entropy_map(out_trg)
        loss_adv = adv.adversarial_loss(ent_trg_aux, ent_trg_main)
        (total_loss + loss_adv).backward()

        # train discriminators
        adv.discriminator_grad(True)
        with torch.no_grad():
            ent_src_aux = adv.entropy_map(None if out_src_aux is None else out_src_aux.detach())
            ent_src_main = adv.entropy_map(out_src_main.detach())
        loss_d_source, loss_d_target = adv.discriminator_loss(ent_src_aux, ent_src_main, ent_trg_aux, ent_trg_main)
        d_loss = loss_d_source + loss_d_target
        d_loss.backward()

        adv.optimizer.step()
        adv.optimizer.zero_grad()
        if ent_trg_aux is not None:
            adv.optimizer_d_aux.step()
            adv.optimizer_d_aux.zero_grad()
        adv.optimizer_d_main.step()
        adv.optimizer_d_main.zero_grad()

        flat = proto_pred["pseudolabels"].reshape(-1)
        current_losses = {
            "Discriminator loss": d_loss,
            "Segmentation loss": loss_seg_src,
            "Adversarial loss": loss_adv,
            "pseudolabel_pixel_num": ((flat >= 0) * (flat != 255)).float().sum(),
            "mean_prototype_intensity_values": (proto.prototypes.prototypes ** 2).mean(),
            "rce_loss": terms["rce_loss"],
            "sym_loss": total_loss,  # the reference aliases total_loss = sym_loss
            "regularization_loss": terms["regularization_loss"],
            "JS Divergance loss": terms["JS Divergance loss"],
            "Total target loss": total_loss,
        }
        # the backward passes are done: the entries leave without the step's autograd graph
        current_losses = {key: _detached(value) for key, value in current_losses.items()}
        for name, value in proto.intensity_ma.avg().items():
            current_losses[f"{name} confidence ma"] = value
        current_losses["dev avg prior static"] = proto.intensity_ma.dev_avg("prior static")
        batch_target["stored_predictions"] = proto_pred["soft_predictions"].reshape(batch_size, w, h, channels).permute(0, 3, 1, 2)
        return current_losses

    def train(self, trainloader, targetloader, validation_loaders, log_fn=None):
        """The per-domain loop (:154-198); log dictionaries go to `log_fn` or the logging sink, as advent.train."""
        emit = log_fn or olog.log
        proto, adv = self.proto_model, self.advent
        proto.update_dynamic()
        if not proto.cfg_spec.SKIP_CALC:
            if not proto.skip_proto:
                switch_batch_statistics(proto.model, False)
                if proto.cfg_spec.STARTING_PROTO == "target":
                    proto.calculate_prototypes(targetloader)
                elif proto.cfg_spec.STARTING_PROTO == "source":
                    proto.calculate_prototypes(trainloader)
                switch_batch_statistics(proto.model, True)
                proto.skip_proto = True
            emit(proto.evaluate_all(validation_loaders))
        steps = proto.cfg_spec.EPOCHS * len(targetloader)
        sources, targets = _Cycle(trainloader), _Cycle(targetloader)
        adv.optimizer.zero_grad()
        adv.optimizer_d_main.zero_grad()
        adv.optimizer_d_aux.zero_grad()
        for i_iter in range(steps):
            adv.adjust_learning_rate(i_iter, steps)
            log = self.step(next(sources), next(targets))
            proto.update_ema()
            if (i_iter + 1) % len(targetloader) == 0:  # epoch end
                log.update(proto.evaluate_all(validation_loaders))
                if not unset(adv.cfg.OTHERS.GENERATE_SAMPLES_EVERY):
                    log.update(proto.test_on_samples(validation_loaders))
            emit(log)
        adv.save_model()
        proto.save_model()
