"""Drop-in for ``framework/domain_adaptation/methods/prototypes.py``: ``online_proDA`` -- the online prototype
adaptation loop whose ``step()`` (:418-450) is the unit BASELINE.json measures -- plus ``regular_loss`` (:29-39).

Same classes, methods, arguments, state and log keys as the reference; a different machine underneath:

* every forward / backward is HIP kernels; the three target losses are one fused kernel; softmax / argmax / confidence
  means of a logits map come from one kernel; pseudo-labels + soft map + monitor means come from one pass over the
  features; optimizer and teacher EMA are single multi-tensor launches; the target batch is uploaded once;
* the step is ordered for the GPU, not for the host: teacher and static forward passes run FIRST, their two confidence
  scalars start travelling to the host (all-reduced over ranks on the way) while the student's target forward pass is
  launched, and the static / dynamic decision reads them only afterwards -- the one host decision of a step never
  leaves the GPU idle.  Dropout2d masks are still drawn in the reference's order (source student, target student,
  teacher);
* everything else the monitor sees (student / dynamic / prototype / posterior / prior confidences) is read back ONCE,
  after the target backward pass has been launched; with several ranks those scalars, the prototype statistics and the
  BatchNorm running statistics ride in the tail of the gradient buffer (onda_amd/dist.py): two collectives per step;
* ``step_sharded`` processes several micro-batches per optimizer step with exactly the arithmetic of that many ranks
  (rank-local batch statistics, averaged gradients, summed prototype statistics, one switch decision): the
  strong-scaling mode of bench.py and the sequential emulation the multi-rank tests compare against;
* ``MODEL_REGULARIZATION > 0`` (the EWC penalty towards the static model, reference :81-91, :334-336): the value is one
  multi-tensor launch per optimizer step and joins the target total detached (``"sym_loss"``, ``"Total target loss"`` and
  ``"model regularization"`` are the reference's); its gradient never visits ``.grad`` -- the optimizer's launch forms it from
  the anchors (``ReplaySGD.anchor_of``) with autograd's roundings.  One GPU only.
"""
from copy import deepcopy

import numpy as np
import torch
from torch import nn
from torch.functional import F

from onda_amd import dist as odist
from onda_amd import logging as olog
from onda_amd import ops
from onda_amd.config import unset
from onda_amd.framework.domain_adaptation.methods.adaptation_model import da_model, switch_batch_statistics
from onda_amd.framework.domain_adaptation.methods.prototype_handler import prototype_handler
from onda_amd.framework.model import deeplabv2
from onda_amd.framework.utils.monitoring import ECE, Monitor
from onda_amd.synthetic import feature_hw as synthetic_feature_hw


import os

# the student's source-replay pass and its target pass as ONE pass over both batches (ops.row_groups); 0 = one after the
# other, as the reference orders them.  PAIR_MAX_ROWS: feature-grid pixels of both batches together up to which the paired
# pass is used -- a sanity bound only since round 5: the kernels address an operand with 32-bit byte offsets RELATIVE to the
# images a tile (a weight-gradient pixel range) touches, so the widest activation (layer4's 2048 channels: 2.17 GB of limb
# rows for 4 + 4 images of 1024x2048, 265 224 rows) may pass 2 GiB.  4 + 4 images of 512x1024 (67 080 rows): 22 GB peak
# with both autograd graphs alive; of 1024x2048: ~90 GB
PAIR_STUDENT = os.environ.get("ONDA_PAIR_STUDENT", "1") != "0"
PAIR_MAX_ROWS = 1 << 21
# the no-grad passes of a step (teacher; static -> switch -> dynamic) on two side streams, beside the student's forward
# pass on the main stream: three independent chains of launches, so one chain's latency-bound kernels (statistics
# finalisation, stream-K fix-ups, 264-tiles-on-256-CUs tails) are covered by another chain's convolutions.  0 = one stream
SIDE_STREAMS = os.environ.get("ONDA_SIDE_STREAMS", "1") != "0"


def _flat_int_buffers(module):
    """Rebind the integer buffers of `module` (BatchNorm's 0-dim `num_batches_tracked`) as views of one flat tensor, values
    kept; returns the flat tensor (None: no such buffers).  state_dict / load_state_dict / deepcopy see ordinary buffers."""
    slots = [(m, name, b) for m in module.modules() for name, b in m._buffers.items()
             if b is not None and not b.is_floating_point() and b.dim() == 0]
    if not slots:
        return None
    owner = getattr(module, "_onda_int_flat", None)
    if owner is not None and owner.numel() == len(slots) and all(b.data_ptr() == owner.data_ptr() + i * owner.element_size()
                                                               for i, (_, _, b) in enumerate(slots)):
        return owner
    flat = torch.stack([b.detach().to(slots[0][2].dtype) for _, _, b in slots])
    for i, (m, name, _) in enumerate(slots):
        m._buffers[name] = flat[i]
    module.__dict__["_onda_int_flat"] = flat
    return flat


def regular_loss(regularizer, activation):
    """"MRKLD": -mean(log_softmax(activation)) over every element (reference :35-38); "MRENT": sum(p * log p) over every
    element / (B*h*w) (:32-34); any other name: 0."""
    if regularizer not in ("MRKLD", "MRENT"):
        return 0
    labels = torch.zeros(activation.shape[0], *activation.shape[2:], dtype=torch.int64, device=activation.device)
    if regularizer == "MRKLD":
        return ops.seg_losses(activation, labels, 0.0, 0.0, 1.0)[0]
    return ops.target_losses(activation, labels, 0.0, 0.0, 1.0, "MRENT", 0.0)[0]


def _positive(v):
    return v if v > 0 else 0.0


class _StepLog(dict):
    """A log dictionary whose monitor entries are computed on first access (any read of the mapping).  They describe
    the monitor as it is at that moment: read the log before the next step, as the reference's loop does, and they are
    the reference's values."""

    def __init__(self, eager, lazy):
        super().__init__(eager)
        self._lazy = lazy

    def _resolve(self):
        lazy, self._lazy = self._lazy, None
        if lazy is not None:
            for key, value in lazy().items():
                dict.__setitem__(self, key, value)

    def __getitem__(self, key):
        if not dict.__contains__(self, key):
            self._resolve()
        return dict.__getitem__(self, key)

    def get(self, key, default=None):
        if not dict.__contains__(self, key):
            self._resolve()
        return dict.get(self, key, default)

    def __contains__(self, key):
        if dict.__contains__(self, key):
            return True
        self._resolve()
        return dict.__contains__(self, key)

    def __iter__(self):
        self._resolve()
        return dict.__iter__(self)

    def __len__(self):
        self._resolve()
        return dict.__len__(self)

    def keys(self):
        self._resolve()
        return dict.keys(self)

    def values(self):
        self._resolve()
        return dict.values(self)

    def items(self):
        self._resolve()
        return dict.items(self)

    def __repr__(self):
        self._resolve()
        return dict.__repr__(self)

    def copy(self):
        self._resolve()
        return dict(self)


class _Scalars:
    """Device scalars waiting for ONE transfer to the host (optionally averaged over ranks first)."""

    def __init__(self):
        self.keys, self.values = [], []

    def put(self, key, value):
        self.keys.append(key)
        self.values.append(value.detach().reshape(()).float())

    def packed(self):
        return torch.stack(self.values) if self.values else None


class online_proDA(da_model):
    # ------------------------------------------------------------------------------------------------ construction
    def __init__(self, model, cfg, cfg_spec) -> None:
        super().__init__(model, cfg, cfg_spec)
        spec = cfg_spec
        self.ema_model, self.dynamic_model, self.static_model = (deepcopy(model) for _ in range(3))
        monitor_args = [spec.AVG_MONITOR_SIZE]
        for optional in (spec.EXP_MONITOR_CONST, spec.DEV_MONITOR_FUNC):
            if unset(optional):
                break
            monitor_args.append(optional)
        self.intensity_ma = Monitor(*monitor_args)
        for m in self.static_model.modules():  # the static model's own BN momentum (reference :55-57)
            if isinstance(m, nn.BatchNorm2d):
                m.momentum = spec.BN_MOMENTUM
        self.models_default_config()
        self.prototypes = prototype_handler(ma_lambda=spec.MA_LAMBDA, tau=spec.TAU, thresh=spec.PSEUDO_THRESH,
                                            distance_metric=spec.DISTANCE_MEASURE,
                                            confidence_regularization_threshold=spec.CONFIDENCE_REGULARIZATION_THRESHOLD)
        self.skip_proto = isinstance(spec.LOAD_PROTO, str)
        if self.skip_proto:
            self.prototypes.load(spec.LOAD_PROTO)
            self.prototypes.to(self.device)
        snap = cfg.OTHERS.SNAPSHOT_DIR
        self.proto_loc, self.proto_cur = f"{snap}/proto_{spec.set_}.pickle", f"{snap}/proto_current.pickle"
        fill = 0 if unset(cfg.TRAINING.PERC_FILL_PER_DOMAIN) else cfg.TRAINING.PERC_FILL_PER_DOMAIN
        self.probability_per_step = fill * 1.0 * cfg.TRAINING.REPLAY_BUFFER / cfg.TRAINING.BATCH_SIZE
        self.model_regularization = None
        self._step_penalty = None  # inside step_sharded: a list that holds the step's penalty once its first micro-batch has launched it
        if not unset(spec.MODEL_REGULARIZATION) and spec.MODEL_REGULARIZATION > 0:
            if odist.is_on():
                raise NotImplementedError(
                    "onda_amd: MODEL_REGULARIZATION > 0 with several ranks: the bucketed gradient exchange overlaps the last "
                    "backward pass, and how the anchored optimizer step interacts with grad_scale across ranks is untested")
            # the EWC penalty towards the static model (reference :81-91; utils/ewc.py:47-54 with unit Fisher weights): its
            # value is one multi-tensor launch per step (`model_regularization`), its gradient is formed inside the
            # optimizer's launch from these anchors -- .grad never holds it
            half_lambda = spec.MODEL_REGULARIZATION / 2
            pairs, cache = list(zip(self.static_model.parameters(), self.model.parameters())), {}
            self.model_regularization = lambda: ops.sqdiff_multi(pairs, half_lambda, cache)
            self.optimizer.anchor_of = {id(p): p0 for p0, p in pairs}
            self.optimizer.half_lambda = half_lambda
        self.ece_save = {}
        if isinstance(spec.BN_POLICY, dict):
            self.cfg_spec.BN_POLICY = "freeze"
        if not unset(spec.LOAD_MODEL) and spec.LOAD_MODEL:
            super().load_model(spec.LOAD_MODEL)
        self.dynamic_update_counter = 0
        self._img_cache = None
        # one exchange per model: a second adapter over the same model (per-domain construction, tests) first detaches the
        # previous one (its hooks, its 46 M-float buffer, its claim on ops.GRAD_READY)
        previous = model.__dict__.get("_onda_grad_sync")
        if previous is not None:
            previous.close()
            if ops.GRAD_READY == previous.grad_ready:
                ops.GRAD_READY = None
        self._grad_sync = odist.GradSync(self.model, tail_floats=self._tail_size(), skip=deeplabv2.unused_head_skip(self.model))
        model.__dict__["_onda_grad_sync"] = self._grad_sync
        if self._grad_sync.active:
            ops.GRAD_READY = self._grad_sync.grad_ready
            self.optimizer.flat_zero = self._grad_sync.zero

    # ------------------------------------------------------------------------------------------- model bookkeeping
    def update_dynamic(self):
        self.dynamic_model = deepcopy(self.model)
        self.models_default_config()

    def models_default_config(self):
        self.model.train()
        self.ema_model.train()
        self.dynamic_model.eval()
        self.static_model.eval()
        self.intensity_ma.train()

    def models_eval(self):
        for m in (self.model, self.ema_model, self.dynamic_model, self.static_model, self.intensity_ma):
            m.eval()

    def update_cfg_spec(self, new_cfg):
        super().update_cfg_spec(new_cfg)
        self.proto_loc = self.cfg.OTHERS.SNAPSHOT_DIR + f"/proto_{new_cfg.set_}.pickle"

    def save_model(self):
        super().save_model(prefix="current")
        self.prototypes.save(self.proto_loc)

    def calculate_prototypes(self, dataloader, save=True):
        """Initial prototypes as running class means over a loader (reference :128-155)."""
        buffered = isinstance(self.cfg.TRAINING.BUFFER_DYNAMIC, bool) and self.cfg.TRAINING.BUFFER_DYNAMIC
        with torch.no_grad():
            for batch in (dataloader.sequential() if buffered else dataloader):
                pred = self.model(batch["image"].to(self.device))[1]
                feat, out = pred["feat"], pred["out"]
                if self.cfg_spec.STARTING_PROTO == "source":
                    # classes from the nearest-resized ground truth; 255 matches no class, so the sums kernel drops
                    # those pixels (the reference masks them out, :144-153)
                    classes = F.interpolate(batch["label"].unsqueeze(1).float(), size=tuple(out.shape[2:])).view(-1)
                    flat, K, C = self.prototypes.class_statistics(feat, out.shape[1], classes=classes)
                else:
                    flat, K, C = self.prototypes.class_statistics(feat, out)
                # sharded loaders: the class sums / counts of all ranks make ONE running mean, so that every rank
                # starts from the same prototypes (each rank must see the same number of batches)
                odist.all_reduce_sum(flat)
                self.prototypes.append_from_statistics(flat, K, C)
        if save:
            import os
            os.makedirs(self.cfg.OTHERS.SNAPSHOT_DIR, exist_ok=True)
            self.prototypes.save(self.proto_cur)

    # ------------------------------------------------------------------------------------------------------ losses
    def supervised_loss(self, batch):
        """CE (and optionally RCE) of the student on a source-replay batch (reference :157-189)."""
        out = self.model(batch["image"].to(self.device))[1]["out"]
        label = batch["stored_predictions"] if "stored_predictions" in batch.keys() else batch["label_res"]
        w_ce, w_rce = _positive(self.cfg_spec.BUFF_CE), _positive(self.cfg_spec.BUFF_RCE)
        total, ce, rc, _ = ops.seg_losses(out, label.long().to(self.device), w_ce, w_rce, 0.0)
        return {"buff_ce_loss": ce if w_ce > 0 else 0, "buff_rce_loss": rc if w_rce > 0 else 0, "buff_loss": total}

    # ---- calibration of the priors (evaluation only) -------------------------------------------------------------------
    def record_ece(self, name, prediction, label, shape=None):
        """ECE of interp(prediction) against `label` under "ece <name>" (reference :191-200): recorded only while the
        monitor is frozen, i.e. under ``evaluate``.  `prediction`: low-resolution probabilities, NCHW or an [N,K] map
        with shape=(B, h, w); they are upsampled inside the kernel and no softmax follows."""
        if not self.ece_record or not self.intensity_ma.freeze:
            return
        name = "ece " + name
        if name not in self.ece_save:
            self.ece_save[name] = ECE(self.ece_bins())
        self.ece_save[name].record_lowres(prediction if shape is None else (prediction, shape), label, self.interp.size,
                                          probs=True)

    def register_ece(self):
        if self.ece_record:
            self.eval_metric_list.extend((name, ece().item()) for name, ece in self.ece_save.items())
            self.ece_save = {}

    # ---- pieces of the target side ---------------------------------------------------------------------------------
    def _device_image(self, batch):
        img = batch["image"]
        if self._img_cache is not None and self._img_cache[0] is img:
            return self._img_cache[1]
        dev = img.to(self.device, non_blocking=True)
        self._img_cache = (img, dev)
        return dev

    def _forward_prior(self, model, image, want_argmax=False, mask=None, ece=None):
        """One no-grad forward: (output dict, softmax map [N,K], mean max-probability (device scalar), argmax or None).
        `ece` = (name, labels): the prior's record point of an evaluation (reference :216, :226, :241)."""
        if mask is not None:
            deeplabv2.force_mask(mask)
        pred = model(image)[1]
        conf, probs, am = ops.softmax_stats(pred["out"], want_probs=True, want_argmax=want_argmax)
        if ece is not None and ece[1] is not None:
            b, _, h, w = pred["out"].shape
            self.record_ece(ece[0], probs, ece[1], shape=(b, h, w))
        return pred, probs, conf, am

    def _teacher_static(self, image, teacher_mask=None, ece_label=None):
        """Teacher pass (train mode) and, with STATIC_LAMBDA > 0, the static model's pass; their confidences are NOT
        read here.  `ece_label`: the labels of an evaluation batch (prototype_predictions only; the step passes none)."""
        t = {"ece_label": ece_label}
        t["pred"], prior_ema, t["conf_ema"], t["cls"] = self._forward_prior(self.ema_model, image, True, teacher_mask,
                                                                            ece=("ema", ece_label))
        t["prior"] = self.cfg_spec.EMA_LAMBDA * prior_ema
        t["conf_static"] = None
        if self.cfg_spec.STATIC_LAMBDA > 0:
            _, prior_static, t["conf_static"], _ = self._forward_prior(self.static_model, image, ece=("static", ece_label))
            t["prior"] += self.cfg_spec.STATIC_LAMBDA * prior_static
        return t

    def _switch_scalars(self, ts):
        """[conf_ema, conf_static] averaged over the given teacher/static results (micro-batches) and over ranks, on its
        way to the host: returns a zero-argument function that yields the two floats (blocking only if they have not
        arrived yet)."""
        rows = [torch.stack([t["conf_ema"], t["conf_static"] if t["conf_static"] is not None else t["conf_ema"]]) for t in ts]
        vals = rows[0] if len(rows) == 1 else torch.stack(rows).mean(0)
        if not self.intensity_ma.freeze:
            odist.all_reduce_mean(vals)
        if not vals.is_cuda:
            return vals.tolist
        host = torch.empty(2, dtype=torch.float32, pin_memory=True)
        host.copy_(vals, non_blocking=True)
        done = torch.cuda.Event()
        done.record()

        def fetch():
            done.synchronize()
            return host.tolist()
        return fetch

    def _record_switch_scalars(self, t, fetch):
        ema, static = fetch()
        self.intensity_ma.add({"prior EMA": ema})
        if t["conf_static"] is not None:
            self.intensity_ma.add({"prior static": static})

    def _prior_plan(self):
        """(weight of the teacher/static prior, weight of the dynamic prior) once "prior static" is in the monitor --
        ``online_proDA``: the SWITCH_PRIOR_THRESH rule (reference :232-255); sub-classes put their switch here."""
        thr = self.cfg_spec.SWITCH_PRIOR_THRESH
        thr = 0 if unset(thr) else thr
        lam = self.cfg_spec.DYNAMIC_LAMBDA
        if lam <= 0:
            return 1.0, 0.0
        if thr > 0:
            return (0.0, lam) if self.intensity_ma.avg("prior static") < thr else (1.0, 0.0)
        return 1.0, lam

    def _mixed_prior(self, t, image, deferred):
        keep, w_dyn = self._prior_plan()
        prior = t["prior"]
        if w_dyn > 0:
            _, prior_dynamic, conf_dyn, _ = self._forward_prior(self.dynamic_model, image, ece=("dynamic", t.get("ece_label")))
            deferred.put("prior dynamic", conf_dyn)
            if keep == 0:
                prior = w_dyn * prior_dynamic
            else:
                prior = (prior if keep == 1 else keep * prior) + w_dyn * prior_dynamic
        elif keep != 1:
            prior = keep * prior
        return prior

    def _labels(self, t, prior, deferred):
        """Pseudo-labels, soft map and the three monitor means of one pass over the teacher's features."""
        feat = t["pred"]["feat"]
        crt = self.prototypes.confidence_regularization_threshold
        if crt < 1 and not self.intensity_ma.freeze:
            # tau regularisation is ON (not in the shipped configs): the reference bumps tau between its two
            # pseudo_labels calls from the monitor's median -- that needs the numbers on the host right here
            labels, soft, s = self.prototypes.assign_stats(feat, prior, reduce=odist.all_reduce_mean)
            self.intensity_ma.add({"prior": s[2]})
            labels = self.prototypes.pseudo_labels(feat, prior, confidence_monitor=self.intensity_ma)
            soft = self.prototypes.pseudo_labels(feat, prior, soft=True)
            s = self.prototypes.assign_stats(feat, prior, reduce=odist.all_reduce_mean)[2]
            self.intensity_ma.add({"pseudolabel confidence": s[1]})
        else:
            labels, soft, stats = self.prototypes._assign(feat, prior)
            deferred.put("prior", stats[2])
            deferred.put("prototypes", stats[0])
            deferred.put("pseudolabel confidence", stats[1])
        return {"ema_model": t["pred"], "pseudolabels": labels, "soft_predictions": soft, "ema_classes": t["cls"]}

    def prototype_predictions(self, batch):
        """Teacher / static / dynamic priors and prototype pseudo-labels (reference :208-273), everything at once."""
        with torch.no_grad():
            image = self._device_image(batch)
            # (hybrid_proDA puts a 0 where a batch has no labels: nothing to record against)
            recording = self.ece_record and self.intensity_ma.freeze and torch.is_tensor(batch.get("label"))
            t = self._teacher_static(image, ece_label=batch["label"] if recording else None)
            if not self.intensity_ma.freeze:
                self._record_switch_scalars(t, self._switch_scalars([t]))
            deferred = _Scalars()
            out = self._labels(t, self._mixed_prior(t, image, deferred), deferred)
            if recording:
                b, _, h, w = t["pred"]["out"].shape
                self.record_ece("pure prototypes", out["soft_predictions"], batch["label"], shape=(b, h, w))
            packed = deferred.packed()
            if packed is not None and not self.intensity_ma.freeze:
                self.intensity_ma.add_device(deferred.keys, odist.all_reduce_mean(packed))
        return out

    # ---- the target loss, pipelined ----------------------------------------------------------------------------------
    def _soft_labels(self):
        """The reference's `soft_labels` (:277-281): SOFT_LABELS, with None / {} meaning hard labels.  Soft labels with
        JS_D > 0 fail in the reference inside js_divergance (a shape mismatch, or one_hot on a float tensor): the same
        exception type here, raised by the step before it launches anything."""
        soft = self.cfg_spec.SOFT_LABELS
        soft = False if unset(soft) else soft
        if soft and self.cfg_spec.JS_D > 0:
            raise RuntimeError("onda_amd: SOFT_LABELS with JS_D > 0: the reference's js_divergance (loss.py:62-85) takes "
                               "hard labels only and raises on the soft map; set JS_D to 0 or SOFT_LABELS to False")
        return soft

    def _target_terms(self, out, predictions, soft_predictions=None):
        """The low-resolution target loss on the fused kernels: (total, {log entries of its terms}) with total = CE * RCE_ALPHA
        + RCE * RCE_BETA + REGULARIZER_WEIGHT * regulariser + JS_D * JS (reference :300-333); a term whose weight is not
        positive is logged as 0.  With SOFT_LABELS the target is `soft_predictions`, the [N,K] soft map (reference :305-322):
        CE over the raw logits against the truncated map (loss_calc's `.long()`: NaN in the log over negative logits, a
        finite gradient), RCE against the real soft values -- one launch each way, whatever the regulariser."""
        spec = self.cfg_spec
        w_ce, w_rce, w_reg = _positive(spec.RCE_ALPHA), _positive(spec.RCE_BETA), _positive(spec.REGULARIZER_WEIGHT)
        w_js = _positive(spec.JS_D)
        js_loss = 0
        if self._soft_labels():
            total, ce_loss, rce_loss, reg_loss = ops.soft_target_losses(out, soft_predictions, w_ce, w_rce, w_reg,
                                                                        spec.REGULARIZER, ce_trunc=True)
            if spec.REGULARIZER not in ops.REGULARIZERS:
                reg_loss = 0
        elif w_js > 0 or (w_reg > 0 and spec.REGULARIZER != "MRKLD"):
            # MRENT / an unknown regulariser (0, as the reference's regular_loss) and the JS term (reference :323-333);
            # the shipped configs (MRKLD, JS_D 0) keep the CE + RCE + MRKLD kernel below
            total, ce_loss, rce_loss, reg_loss, js_loss = ops.target_losses(out, predictions, w_ce, w_rce, w_reg,
                                                                            spec.REGULARIZER, w_js)
            if spec.REGULARIZER not in ops.REGULARIZERS:
                reg_loss = 0
        else:
            total, ce_loss, rce_loss, reg_loss = ops.seg_losses(out, predictions, w_ce, w_rce, w_reg)
        return total, {"ce_loss": ce_loss if w_ce > 0 else 0, "rce_loss": rce_loss if w_rce > 0 else 0,
                       "regularization_loss": reg_loss if w_reg > 0 else 0, "JS Divergance loss": js_loss if w_js > 0 else 0}

    def _target_losses(self, out, proto_pred, cls_model):
        batch_size, channels, w, h = out.size()
        predictions = proto_pred["pseudolabels"].reshape(batch_size, w, h)
        total, terms = self._target_terms(out, predictions, proto_pred["soft_predictions"])
        penalty = 0
        if self.model_regularization is not None:
            # total_loss += ewc_loss(...) (reference :334-336).  The value joins the total detached: its gradient is the
            # optimizer launch's business (ReplaySGD.anchor_of), backward() has nothing to do for it.  ONE penalty per
            # optimizer step, however many micro-batches (the weights do not move before optimizer.step()): the first one
            # launches it here, on the main stream behind the student's forward pass, which has joined the side streams by
            # now -- 91 + 15 us with the device to itself; ahead of the forward pass it shared the device with the no-grad
            # passes and sat in the student's chain for 98-400 us, its one-workgroup sum for up to 460 (docs/experiments.md)
            slot = self._step_penalty if self._step_penalty is not None else []
            if not slot:
                slot.append(self.model_regularization())
            penalty = slot[0]
            total = total + penalty
        flat = proto_pred["pseudolabels"].reshape(-1)
        return {
            "ce_loss": terms["ce_loss"],
            "pseudolabel_pixel_num": ((flat >= 0) * (flat != 255)).float().sum(),
            "output & prototype agreement": (flat == cls_model.long()).float().mean(),
            "rce_loss": terms["rce_loss"],
            "sym_loss": total,  # the reference aliases total_loss = sym_loss
            "regularization_loss": terms["regularization_loss"],
            "JS Divergance loss": terms["JS Divergance loss"],
            "Total target loss": total,
            "model regularization": penalty,
        }

    def _monitor_log(self, losses):
        """The step's log entries.  The monitor's statistics need this step's device scalars on the host; they are filled
        in when the log is first LOOKED AT (_StepLog), so a loop that logs every n-th step -- or the benchmark, which reads
        the last one -- never stops the host behind the backward pass it has just launched."""
        losses["mean_prototype_intensity_values"] = (self.prototypes.prototypes ** 2).mean()
        monitor = self.intensity_ma

        def entries():
            out = {}
            for name, value in monitor.avg().items():
                out[f"{name} confidence ma"] = value
            for name, value in monitor.exp().items():
                out[f"{name} exp confidence ma"] = value
            out["dev avg prior static"] = monitor.dev_avg("prior static")
            return out
        return _StepLog(losses, entries)

    def _target_prepare(self, batch):
        """First half of the target side: Dropout2d masks (in the reference's order of draws: the student's target pass,
        then the teacher's), teacher and static forward passes.  Nothing is read back."""
        self._soft_labels()  # (SOFT_LABELS with JS_D > 0 raises here, before anything is launched)
        if not unset(self.cfg_spec.PREDICTION_SAVE):
            raise NotImplementedError("onda_amd: PREDICTION_SAVE is a logging feature outside the hot path")
        image = self._device_image(batch)
        student_mask = deeplabv2.draw_mask(self.model, image.shape[0], image.device)
        teacher_mask = deeplabv2.draw_mask(self.ema_model, image.shape[0], image.device)
        with torch.no_grad():
            t = self._teacher_static(image, teacher_mask)
        t["image"], t["student_mask"] = image, student_mask
        return t

    # ---- the no-grad passes beside the student's forward pass -------------------------------------------------------------
    def _concurrent_ok(self, n_shards):
        """Sub-classes whose switch decision never visits the host (hybrid_proDA with the device-side switch) say yes."""
        return False

    def _side_streams(self):
        st = self.__dict__.get("_side")
        if st is None or st[0] != str(self.device):
            st = self.__dict__["_side"] = (str(self.device), torch.cuda.Stream(device=self.device), torch.cuda.Stream(device=self.device))
        return st[1], st[2]

    def _target_prepare_concurrent(self, batch, deferred):
        """``_target_prepare`` + the switch + the dynamic pass + the prior, issued on two side streams: stream 1 runs the
        teacher, stream 2 the static model, then (behind the teacher's confidence) the switch step and the predicated dynamic
        pass.  Returns at once; the caller launches the student's forward pass on the main stream and then ``_join``s."""
        image = self._device_image(batch)
        student_mask = deeplabv2.draw_mask(self.model, image.shape[0], image.device)
        teacher_mask = deeplabv2.draw_mask(self.ema_model, image.shape[0], image.device)
        # everything the passes share is made on the main stream first: the stem's patch matrix (cached on the image tensor)
        # and enough zeroed max|x| slots for the whole step (a refill inside a side stream would race the other streams)
        ops.stem_prefetch(image)
        ops.reserve_amax_slots(image.device, 4096)  # (a step takes ~1 000: four forward passes, two backward passes, two repacks)
        main = torch.cuda.current_stream()
        s1, s2 = self._side_streams()
        s1.wait_stream(main)
        s2.wait_stream(main)
        if teacher_mask is not None:
            # made on the main stream, dropped by the host as soon as the teacher's head has been ENQUEUED on stream 1: the
            # main stream (busy with the student meanwhile) must not get its memory back before stream 1 has read it
            teacher_mask.record_stream(s1)
        t = {"image": image, "student_mask": student_mask}
        with torch.no_grad():
            with torch.cuda.stream(s1):
                t["pred"], prior_ema, t["conf_ema"], t["cls"] = self._forward_prior(self.ema_model, image, True, teacher_mask)
            with torch.cuda.stream(s2):
                t["conf_static"] = None
                prior_static = None
                if self.cfg_spec.STATIC_LAMBDA > 0:
                    _, prior_static, t["conf_static"], _ = self._forward_prior(self.static_model, image)
                s2.wait_stream(s1)  # the teacher's confidence and prior
                # allocated on stream 1, read on stream 2 from here on (the switch scalars, the prior mix): tell the caching
                # allocator, so that a later piece of stream-1 work in this step cannot be handed their blocks while stream 2
                # still reads them (round-4 advisor: until now only the step's shape guaranteed that)
                for v in (prior_ema, t["conf_ema"], t["cls"]):
                    if torch.is_tensor(v) and v.is_cuda:
                        v.record_stream(s2)
                t["prior"] = self.cfg_spec.EMA_LAMBDA * prior_ema
                if prior_static is not None:
                    t["prior"] += self.cfg_spec.STATIC_LAMBDA * prior_static
                t["fetch"] = self._switch_scalars([t])
                t["mixed_prior"] = self._mixed_prior(t, image, deferred)
        t["streams"] = (s1, s2)
        return t

    def _join(self, t, deferred, fetch):
        """The main stream waits for the side streams; what they produced is handed over to it (caching allocator)."""
        main = torch.cuda.current_stream()
        for s_ in t.pop("streams"):
            main.wait_stream(s_)
        keep = [t["pred"]["feat"], t["pred"]["out"], t["conf_ema"], t["cls"], t["prior"], t["mixed_prior"], t["conf_static"], fetch]
        for v in keep + list(deferred.values):
            if torch.is_tensor(v) and v.is_cuda:
                v.record_stream(main)

    def _target_finish(self, batch, t, deferred, fetch=None, out=None):
        """Second half: the student's forward pass (launched BEFORE the switch scalars are read: `fetch`, given for the
        first micro-batch of a step; `out`: its logits when the paired pass has already produced them), prior mixing,
        pseudo-labels, the losses.  The prototype EMA and the monitor entries stay pending (``_settle``)."""
        image = t["image"]
        if out is None:
            if t["student_mask"] is not None:
                deeplabv2.force_mask(t["student_mask"])
            out = self.model(image)[1]["out"]
        if "streams" in t:
            self._join(t, deferred, fetch)  # (the student's forward pass is in the main stream's queue by now)
        with torch.no_grad():
            conf_model, _, cls_model = ops.softmax_stats(out, want_argmax=True)
            deferred.put("model", conf_model)
            if fetch is not None:
                self._record_switch_scalars(t, fetch)
            prior = t["mixed_prior"] if "mixed_prior" in t else self._mixed_prior(t, image, deferred)
            proto_pred = self._labels(t, prior, deferred)
        losses = self._target_losses(out, proto_pred, cls_model)
        b, k, w, h = out.size()
        batch["stored_predictions"] = proto_pred["soft_predictions"].reshape(b, w, h, k).permute(0, 3, 1, 2)
        return losses

    def _settle(self, losses, teacher_results, deferred):
        """After the target backward pass has been launched: prototype EMA from the (rank-summed) class statistics, the
        deferred scalars into the monitor (rank-mean), running statistics averaged over ranks, the monitor's log entries."""
        sync = self._grad_sync
        stats = None
        for t in teacher_results:
            flat, K, C = self.prototypes.class_statistics(t["pred"]["feat"], t["pred"]["out"], t["cls"])
            stats = flat if stats is None else stats + flat
        keys, packed = deferred.keys, deferred.packed()
        if len(teacher_results) > 1:  # several micro-batches: the mean of each key over them
            keys = list(dict.fromkeys(deferred.keys))
            packed = torch.stack([torch.stack([v for k_, v in zip(deferred.keys, deferred.values) if k_ == key]).mean()
                                  for key in keys])
        if sync.active:
            tail, n1 = sync.tail, stats.numel()
            tail[:n1].copy_(stats)
            tail[n1:n1 + packed.numel()].copy_(packed)
            bufs = self._float_buffers()
            nb = sum(b.numel() for b in bufs)
            if bufs:
                torch.cat([b.reshape(-1) for b in bufs], out=tail[n1 + 16:n1 + 16 + nb])
            sync.finish(mean=False)  # the buffer holds rank sums: the optimizer divides on the way in
            world = odist.world_size()
            self.optimizer.grad_scale = 1.0 / world
            stats = tail[:n1]
            packed = tail[n1:n1 + packed.numel()] / world
            if bufs:
                mean = tail[n1 + 16:n1 + 16 + nb] / world
                torch._foreach_copy_(bufs, [v.view_as(b) for v, b in zip(mean.split([b.numel() for b in bufs]), bufs)])
                for b in bufs:
                    torch.autograd.graph.increment_version(b)
        self.prototypes.ma_from_statistics(stats, K, C)
        if packed is not None:
            self.intensity_ma.add_device(keys, packed)
        return self._monitor_log(losses)

    def _bn_modules(self):
        """The BatchNorm2d modules of the student, listed once per model object (the step flips their statistics switch
        twice; the walk over the module tree costs 0.4 ms each time, at the start of a step where the device waits)."""
        plan = self.__dict__.get("_bn_plan")
        if plan is None or plan[0] is not self.model:
            plan = self.__dict__["_bn_plan"] = (self.model, [m for m in self.model.modules() if isinstance(m, torch.nn.BatchNorm2d)])
        return plan[1]

    def _float_buffers(self):
        return [b for b in self.model.buffers() if b.dtype == torch.float32]

    def _tail_size(self):
        K, C = self.cfg.NUM_CLASSES, 256
        return 2 * K * C + K + 16 + sum(b.numel() for b in self.model.buffers() if b.dtype == torch.float32)

    def pseudolabel_loss(self, batch):
        """Target loss from prototype pseudo-labels (reference :275-372), complete with monitor entries (the step itself
        uses the pipelined pieces and settles after the backward pass)."""
        deferred = _Scalars()
        t = self._target_prepare(batch)
        losses = self._target_finish(batch, t, deferred, self._switch_scalars([t]))
        return self._settle(losses, [t], deferred)

    def evaluate(self, validation_loader):
        def proto_func(batch):
            proto_pred = self.prototype_predictions(batch)
            b, k, h, w = proto_pred["ema_model"]["out"].size()
            return proto_pred["soft_predictions"].reshape(b, h, w, k).permute(0, 3, 1, 2)

        if isinstance(self.cfg_spec.SKIP_PROTO_EVAL, bool) and self.cfg_spec.SKIP_PROTO_EVAL:
            evaluation = super().evaluate(validation_loader)
        else:
            evaluation = super().evaluate(validation_loader, {"proto": proto_func})
        self.register_ece()
        return evaluation

    def evaluate_update_dynamic(self):
        if unset(self.cfg_spec.AUTO_DYNAMIC) or not self.cfg_spec.AUTO_DYNAMIC:
            return
        self.dynamic_update_counter += 1
        if self.dynamic_update_counter > 500 and np.abs(self.intensity_ma.dev_avg("prior static")) > self.cfg_spec.DEV_THRESH:
            self.update_dynamic()
            self.dynamic_update_counter = 0

    @torch.no_grad()
    def update_ema(self):
        """teacher = keep*teacher + (1-keep)*student for all 217 parameters, buffers copied (reference :407-416), as one
        multi-tensor launch.  (With several ranks the student's running statistics were averaged in the step's exchange.)"""
        keep = self.cfg_spec.EMA_UPDATE
        plan = self.__dict__.get("_ema_plan")
        if plan is None or plan["of"][0] is not self.model or plan["of"][1] is not self.ema_model or plan["of"][2] != keep:
            # the walk over both module trees (~1 ms) and the table are kept between steps: this runs when the device has
            # nothing queued (right behind the optimizer launch), so its host time is idle device time
            pairs = [(k, q, keep, 1.0 - keep) for q, k in zip(self.model.parameters(), self.ema_model.parameters())]
            for bq, bk in zip(self.model.buffers(), self.ema_model.buffers()):
                if bq.dtype == torch.float32:
                    pairs.append((bk, bq, 0.0, 1.0))
            # the integer buffers (53 `num_batches_tracked` counters) of each model become views of ONE tensor, so that the
            # teacher's copy of them is one device copy per step instead of 53 (each a 4 us launch at the end of the step,
            # where nothing else is queued)
            plan = self.__dict__["_ema_plan"] = {"of": (self.model, self.ema_model, keep), "pairs": pairs,
                                                 "ints_q": _flat_int_buffers(self.model), "ints_k": _flat_int_buffers(self.ema_model),
                                                 "cache": {}}
        ops.ema_multi(plan["pairs"], plan["cache"])
        if plan["ints_k"] is not None and plan["ints_q"] is not None:
            plan["ints_k"].copy_(plan["ints_q"])

    # -------------------------------------------------------------------------------------------------------- step
    def _source_replay(self, batches_source, scale=1.0, masks=None):
        """Source replay with the BatchNorm policy of the config around it; returns the last batch's log entries.
        `masks`: the Dropout2d masks of these passes when they were drawn ahead of time (one per batch, in order)."""
        policy = self.cfg_spec.BN_POLICY
        if policy == "freeze":
            switch_batch_statistics(self.model, False, self._bn_modules())
        elif policy == "double":
            self.bn.exchange()
        log = {}
        for i, batch in enumerate(batches_source):
            if self.cfg.TRAINING.REPLAY_BUFFER > 0:
                if masks is not None and masks[i] is not None:
                    deeplabv2.force_mask(masks[i])
                log = self.supervised_loss(batch)
                (log["buff_loss"] if scale == 1.0 else log["buff_loss"] * scale).backward()
        if policy == "freeze":
            switch_batch_statistics(self.model, True, self._bn_modules())
        elif policy == "double":
            self.bn.exchange()
        return log

    # ---- the student's two passes as one ---------------------------------------------------------------------------------
    def _pairable(self, batches_source, batch_target):
        """Can the student's source-replay pass and its target pass run as ONE pass over both batches (row groups:
        ops.row_groups)?  The reference runs them one after the other through the same weights (:418-450), each with its
        own BatchNorm batch statistics, the source pass with frozen running statistics (BN_POLICY "freeze"): the kernels
        keep exactly that per group, so the result is the same arithmetic with every launch covering twice the rows."""
        if not (PAIR_STUDENT and ops.row_groups_supported() and self.cfg_spec.BN_POLICY == "freeze"
                and len(batches_source) == 1 and self.cfg.TRAINING.REPLAY_BUFFER > 0 and self.model.training
                and not self.model.multi_level):  # (the auxiliary head would draw its Dropout2d mask in another order)
            return False
        src, trg = batches_source[0]["image"], batch_target["image"]
        if tuple(src.shape[1:]) != tuple(trg.shape[1:]):
            return False
        h, w = synthetic_feature_hw(src.shape[2], src.shape[3])
        return (src.shape[0] + trg.shape[0]) * h * w <= PAIR_MAX_ROWS

    def _source_mask(self, batch):
        """The Dropout2d mask of the source pass, drawn where the reference's source forward draws it (first in a step)."""
        image = batch["image"]
        return deeplabv2.draw_mask(self.model, image.shape[0], self.device)

    def _student_pair(self, batch_source, src_mask, batch_target, t, deferred, fetch):
        """Both student passes as one: returns (source log entries, target loss entries); the caller sums the two totals
        and runs ONE backward pass."""
        src_image = batch_source["image"].to(self.device, non_blocking=True)
        n_src = src_image.shape[0]
        image = torch.cat([src_image, t["image"]], 0)
        masks = [m for m in (src_mask, t["student_mask"]) if m is not None]
        if masks:
            deeplabv2.force_mask(torch.cat(masks, 0))
        with ops.row_groups(n_src):
            out = self.model(image)[1]["out"]
        out_src, out_trg = out[:n_src], out[n_src:]
        label = batch_source["stored_predictions"] if "stored_predictions" in batch_source.keys() else batch_source["label_res"]
        w_ce, w_rce = _positive(self.cfg_spec.BUFF_CE), _positive(self.cfg_spec.BUFF_RCE)
        total, ce, rc, _ = ops.seg_losses(out_src, label.long().to(self.device), w_ce, w_rce, 0.0)
        src_log = {"buff_ce_loss": ce if w_ce > 0 else 0, "buff_rce_loss": rc if w_rce > 0 else 0, "buff_loss": total}
        return src_log, self._target_finish(batch_target, t, deferred, fetch, out=out_trg)

    def step(self, batches_source, batch_target):
        """One adaptation step: source replay fwd+bwd (BN statistics frozen), teacher / static fwd, target fwd, (dynamic
        fwd), pseudo-labels, target bwd, prototype EMA, optimizer step."""
        return self.step_sharded([(batches_source, batch_target)])

    def step_sharded(self, shards):
        """`shards`: [(batches_source, batch_target), ...] -- micro-batches of ONE optimizer step, processed with the
        arithmetic of len(shards) ranks (x the real ranks): every micro-batch normalises with its own batch
        statistics, gradients are averaged, class statistics summed, monitor scalars averaged, the BatchNorm running
        statistics averaged, one switch decision.  Returns the first micro-batch's log dict."""
        self._soft_labels()  # (SOFT_LABELS with JS_D > 0 raises here, before anything is launched)
        n = len(shards)
        scale = 1.0 / n
        deferred, src_log, prepared = _Scalars(), {}, []
        # the student's source and target passes of a micro-batch as ONE pass over both batches, where the method's settings
        # allow it (every micro-batch of a step the same way)
        paired = all(self._pairable(bs, bt) for bs, bt in shards)
        concurrent = SIDE_STREAMS and self._concurrent_ok(n) and torch.device(self.device).type == "cuda"
        src_masks = []
        # source replay (gradients accumulate) and the no-grad teacher / static passes of every micro-batch; per
        # micro-batch the Dropout2d masks are drawn in the reference's order: source student, target student, teacher
        for i, (batches_source, batch_target) in enumerate(shards):
            if paired:
                src_masks.append(self._source_mask(batches_source[0]))
            elif concurrent and self.cfg.TRAINING.REPLAY_BUFFER > 0 and not self.model.multi_level:
                # the no-grad passes go to their side streams FIRST and run beside the source-replay pass as well; the
                # source passes' masks are drawn before theirs, as the reference's order of draws has it
                masks = [self._source_mask(b) for b in batches_source]
                prepared.append(self._target_prepare_concurrent(batch_target, deferred))
                src_log = self._source_replay(batches_source, scale, masks)
                continue
            else:
                log = self._source_replay(batches_source, scale)
                if i == 0:
                    src_log = log
            prepared.append(self._target_prepare_concurrent(batch_target, deferred) if concurrent else self._target_prepare(batch_target))
        # ONE decision per step, from the mean over micro-batches and ranks
        fetch = prepared[0].pop("fetch") if concurrent else self._switch_scalars(prepared)
        run0 = None
        if n > 1:  # every micro-batch starts from the same running statistics; their results are averaged
            bufs = self._float_buffers()
            run0 = [b.clone() for b in bufs]
            run_sum = [torch.zeros_like(b) for b in bufs]
        first_log = None
        self._step_penalty = []  # (filled by the first micro-batch's _target_losses when MODEL_REGULARIZATION is on)
        for i, ((_, batch_target), t) in enumerate(zip(shards, prepared)):
            if run0 is not None:
                torch._foreach_copy_(bufs, run0)
            if paired:
                log, losses = self._student_pair(shards[i][0][0], src_masks[i], batch_target, t, deferred, fetch if i == 0 else None)
                if i == 0:
                    src_log = log
                both = log["buff_loss"] + losses["Total target loss"]  # the reference's two backward passes, summed
            else:
                losses = self._target_finish(batch_target, t, deferred, fetch if i == 0 else None)
                both = losses["Total target loss"]
            if i == n - 1:
                self._grad_sync.arm()  # buckets go out as the last backward pass completes them
            (both if n == 1 else both * scale).backward()
            if i == 0:
                first_log = losses
            if run0 is not None:
                torch._foreach_add_(run_sum, bufs)
        self._img_cache = None
        self._step_penalty = None
        if run0 is not None:
            torch._foreach_mul_(run_sum, scale)
            torch._foreach_copy_(bufs, run_sum)
            for b in bufs:
                torch.autograd.graph.increment_version(b)
        first_log = self._settle(first_log, prepared, deferred)
        first_log["encoder_lr"] = self.optimizer.param_groups[0]["lr"]
        first_log.update(src_log)
        # the backward passes are done: the entries leave as plain values -- a caller that keeps log dictionaries must not
        # keep the step's autograd graph (and the ~7 GB of limb planes its nodes reference) alive with them
        for key, value in dict.items(first_log):
            if torch.is_tensor(value) and value.requires_grad:
                dict.__setitem__(first_log, key, value.detach())
        self.optimizer.step()
        self.optimizer.zero_grad()
        return first_log

    def buffer_update(self, batch_target, probability, trainloader):
        """With probability `probability` per target sample, put it (with its pseudo-label map at image resolution) into
        the replay buffer (reference :452-464).  The reference upsamples inside its loop over the chosen samples, i.e.
        a second chosen sample of the same batch would upsample the already-argmaxed map; here the map is built once."""
        total_buffer_updates = 0
        if probability > 0:
            chosen = np.where(np.random.rand(len(batch_target["stored_predictions"])) < probability)[0]
            if len(chosen):
                stored = batch_target["stored_predictions"]
                if stored.dim() == 4:
                    batch_target["stored_predictions"] = ops.upsample_argmax(stored, self.interp.size).long()
                for index in chosen:
                    trainloader.add_from_batch(batch_target, index)
                    total_buffer_updates += 1
        return total_buffer_updates

    def train(self, trainloader, targetloader, validation_loaders, log_fn=None):
        """The per-domain loop (reference :466-520).  Log dictionaries go to ``wandb.log`` when wandb is importable and a
        run is active -- as in the reference -- or to `log_fn` / onda_amd.logging.set_sink."""
        emit = log_fn or olog.log
        spec = self.cfg_spec
        if unset(spec.AUTO_DYNAMIC) or spec.AUTO_DYNAMIC is False:
            self.update_dynamic()
        if not spec.SKIP_CALC:
            if not self.skip_proto:
                switch_batch_statistics(self.model, False)
                self.calculate_prototypes(targetloader if spec.STARTING_PROTO == "target" else trainloader)
                switch_batch_statistics(self.model, True)
                self.skip_proto = True
            if validation_loaders:
                emit(self.evaluate_all(validation_loaders))
        steps = spec.EPOCHS * len(targetloader)
        update_prob = self.probability_per_step / steps
        sources, targets = _Cycle(trainloader), _Cycle(targetloader)
        self.optimizer.zero_grad()
        for i_iter in range(steps):
            self.adjust_learning_rate(i_iter, steps)
            source_samples = [next(sources) for _ in range(spec.SOURCE_REPEAT)]
            target_sample = next(targets)
            log = self.step(source_samples, target_sample)
            self.evaluate_update_dynamic()
            self.update_ema()
            log["Total buffer updates"] = self.buffer_update(target_sample, update_prob, trainloader)
            if (i_iter + 1) % len(targetloader) == 0:  # epoch end (reference :512-518)
                if validation_loaders:
                    log.update(self.evaluate_all(validation_loaders))
                    if not unset(self.cfg.OTHERS.GENERATE_SAMPLES_EVERY):
                        log.update(self.test_on_samples(validation_loaders))
                self._save_on_rank0()
            emit(log)
        self._save_on_rank0()

    def _save_on_rank0(self):
        """Checkpoint + prototypes written once per job: the replicas are identical, and several ranks writing the same
        paths at the same time tear the files (the reference is single-process)."""
        if odist.rank() == 0:
            self.save_model()
        odist.barrier()


class _Cycle:
    """next() over a loader, restarted when it runs out (the reference's try / except StopIteration blocks)."""

    def __init__(self, loader):
        self.loader, self.it = loader, iter(loader)

    def __next__(self):
        try:
            return next(self.it)
        except StopIteration:
            self.it = iter(self.loader)
            return next(self.it)
