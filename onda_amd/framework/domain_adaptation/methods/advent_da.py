"""Drop-in for ``framework/domain_adaptation/methods/advent_da.py`` (``advent``, :40-214): the ADVENT adversarial baseline --
a supervised source pass, an adversarial target pass that asks the two discriminators to call the target's entropy maps
"source", and a discriminator pass over both domains' maps.

What runs where.  The segmentation network is the HIP model.  ``loss_calc(interp(out), label)`` is ``ops.upsample_ce``.  Every
``d(prob_2_entropy(F.softmax(interp(out))))`` of the reference (:94-128) takes its map from ``ops.upsample_entropy``: the
upsampled logits and the softmax never exist in memory, in either direction.  (The reference's ``F.softmax(x)`` has no
``dim``; for a 4-D input torch's implicit choice is ``dim=1``, the class axis -- what the kernel computes.)  The discriminators'
five 4x4 / stride 2 convolutions have a HIP route of their own, ``ops.disc_conv`` (``framework/model/discriminator.py`` says when
``forward`` takes it and when the ``torch.nn`` module chain runs); Adam is torch's.

The reference evaluates the expression six times a step with two heads: the discriminator pass recomputes the maps of
``pred.detach()``, which changes no number.  Here the target maps of the adversarial pass are reused, detached, and the source
maps are computed once without a graph: four forward launches.

One GPU, one stream: the discriminators' gradients have no exchange, so with ``onda_amd.dist`` active the constructor raises.
"""
import torch
from torch import optim

from onda_amd import dist as odist
from onda_amd import logging as olog
from onda_amd import ops
from onda_amd.config import unset
from onda_amd.framework.domain_adaptation.methods.adaptation_model import da_model, switch_batch_statistics
from onda_amd.framework.domain_adaptation.methods.prototypes import _Cycle
from onda_amd.framework.model.discriminator import get_fc_discriminator
from onda_amd.framework.utils.func import bce_loss


def _out(pred):
    """The low-resolution logits of one head's prediction (a dict with "out", or the tensor), None for an absent head."""
    if pred is None:
        return None
    return pred["out"] if isinstance(pred, dict) else pred


class advent(da_model):
    source_label = 0
    target_label = 1

    def __init__(self, model, cfg, cfg_spec) -> None:
        if odist.is_on():
            raise NotImplementedError("onda_amd: ADVENT runs on one GPU -- the discriminators' gradients have no exchange "
                                      "across ranks, and a run without one would train them on one rank's batches only")
        super().__init__(model, cfg, cfg_spec)
        num_classes = cfg.NUM_CLASSES
        self.d_aux = get_fc_discriminator(num_classes=num_classes).train().to(self.device)
        self.d_main = get_fc_discriminator(num_classes=num_classes).train().to(self.device)  # seg maps, i.e. output, level
        self.optimizer_d_aux = optim.Adam(self.d_aux.parameters(), lr=cfg_spec.LEARNING_RATE_D, betas=(0.9, 0.99))
        self.optimizer_d_main = optim.Adam(self.d_main.parameters(), lr=cfg_spec.LEARNING_RATE_D, betas=(0.9, 0.99))

    def save_model(self):
        super().save_model(model_dict={"model": self.model, "d_main": self.d_main, "d_aux": self.d_aux}, prefix="current")

    def models_eval(self):
        self.model.eval()

    def models_default_config(self):
        self.model.train()

    def discriminator_grad(self, option):
        for d in (self.d_aux, self.d_main):
            for param in d.parameters():
                param.requires_grad = option

    def entropy_map(self, out):
        """prob_2_entropy(softmax(interp(out), 1)) at SCHEME.RESOLUTION, f32[B,K,H,W]; None for an absent head."""
        return None if out is None else ops.upsample_entropy(out, self.interp.size)

    def supervised_loss(self, out_src_aux, out_src_main, label):
        """LAMBDA_SEG_MAIN * loss_calc(interp(main), label) + LAMBDA_SEG_AUX * the same of the auxiliary head (:84-92); the
        arguments are the heads' low-resolution logits, the interpolation happens inside the fused kernel."""
        label = label.to(self.device)
        loss_seg_src_aux = 0
        if out_src_aux is not None:
            loss_seg_src_aux = ops.upsample_ce(out_src_aux, label)
        loss_seg_src_main = ops.upsample_ce(out_src_main, label)
        return self.cfg_spec.LAMBDA_SEG_MAIN * loss_seg_src_main + self.cfg_spec.LAMBDA_SEG_AUX * loss_seg_src_aux

    def adversarial_loss(self, ent_trg_aux, ent_trg_main):
        """The target's entropy maps against the SOURCE label (:94-104)."""
        loss_adv_trg_aux = 0
        if ent_trg_aux is not None:
            loss_adv_trg_aux = bce_loss(self.d_aux(ent_trg_aux), self.source_label)
        loss_adv_trg_main = bce_loss(self.d_main(ent_trg_main), self.source_label)
        return self.cfg_spec.LAMBDA_ADV_MAIN * loss_adv_trg_main + self.cfg_spec.LAMBDA_ADV_AUX * loss_adv_trg_aux

    def discriminator_loss(self, ent_src_aux, ent_src_main, ent_trg_aux, ent_trg_main):
        """(loss on the source maps, loss on the target maps), each halved, no gradient into the maps (:106-128)."""
        loss_d_src_aux = 0
        if ent_src_aux is not None:
            loss_d_src_aux = bce_loss(self.d_aux(ent_src_aux.detach()), self.source_label) / 2
        loss_d_src_main = bce_loss(self.d_main(ent_src_main.detach()), self.source_label) / 2
        loss_d_source = loss_d_src_main + loss_d_src_aux
        loss_d_trg_aux = 0
        if ent_trg_aux is not None:
            loss_d_trg_aux = bce_loss(self.d_aux(ent_trg_aux.detach()), self.target_label) / 2
        loss_d_trg_main = bce_loss(self.d_main(ent_trg_main.detach()), self.target_label) / 2
        loss_d_target = loss_d_trg_main + loss_d_trg_aux
        return loss_d_source, loss_d_target

    def step(self, batch_source, batch_target):
        """One learning step (:130-181): source sample(s) supervised with frozen running statistics, the target sample
        adversarially, then the discriminators on both."""
        self.discriminator_grad(False)
        switch_batch_statistics(self.model, False)
        # task training
        pred_src_aux, pred_src_main = self.model(batch_source["image"].to(self.device))
        out_src_aux, out_src_main = _out(pred_src_aux), _out(pred_src_main)
        loss_seg_src = self.supervised_loss(out_src_aux, out_src_main, batch_source["label"])
        loss_seg_src.backward()
        switch_batch_statistics(self.model, True)
        # adversarial training
        pred_trg_aux, pred_trg_main = self.model(batch_target["image"].to(self.device))
        ent_trg_aux, ent_trg_main = self.entropy_map(_out(pred_trg_aux)), self.entropy_map(_out(pred_trg_main))
        loss_adv = self.adversarial_loss(ent_trg_aux, ent_trg_main)
        loss_adv.backward()
        # train discriminators
        self.discriminator_grad(True)
        with torch.no_grad():
            ent_src_aux = self.entropy_map(None if out_src_aux is None else out_src_aux.detach())
            ent_src_main = self.entropy_map(out_src_main.detach())
        loss_d_source, loss_d_target = self.discriminator_loss(ent_src_aux, ent_src_main, ent_trg_aux, ent_trg_main)
        d_loss = loss_d_source + loss_d_target
        d_loss.backward()

        self.optimizer.step()
        self.optimizer.zero_grad()
        if ent_trg_aux is not None:
            self.optimizer_d_aux.step()
            self.optimizer_d_aux.zero_grad()
        self.optimizer_d_main.step()
        self.optimizer_d_main.zero_grad()
        return {"Discriminator loss": d_loss.detach(), "Segmentation loss": loss_seg_src.detach(),
                "Adversarial loss": loss_adv.detach()}

    def train(self, trainloader, targetloader, validation_loaders, log_fn=None):
        """The per-domain loop (:183-214); log dictionaries go to `log_fn` or the logging sink, as prototypes.train."""
        emit = log_fn or olog.log
        if not self.cfg_spec.SKIP_CALC:
            emit(self.evaluate_all(validation_loaders))
        steps = self.cfg_spec.EPOCHS * len(targetloader)
        sources, targets = _Cycle(trainloader), _Cycle(targetloader)
        self.optimizer.zero_grad()
        self.optimizer_d_main.zero_grad()
        self.optimizer_d_aux.zero_grad()
        for i_iter in range(steps):
            self.adjust_learning_rate(i_iter, steps)
            log = self.step(next(sources), next(targets))
            if (i_iter + 1) % len(targetloader) == 0:  # epoch end
                log.update(self.evaluate_all(validation_loaders))
                if not unset(self.cfg.OTHERS.GENERATE_SAMPLES_EVERY):
                    log.update(self.test_on_samples(validation_loaders))
                self.save_model()
            emit(log)
        self.save_model()
