"""What tests/golden/make_golden_proda101.py (the reference's side) and the tests of the DeepLabv2-Resnet101-ProDA mirror and of
``get_deeplab_v2(norm_grad=True)`` share: the seed, the batch size, the step's settings and the list of BatchNorm parameters.
A plain module, like gn_site_fp64.py."""
import torch

SEED = 26
H, W = 65, 129            # synth_batch(2, H, W): a 9 x 17 feature grid, the labels of gn_site_fp64.labels()
DIGEST = 16               # strided values per tensor in the tree fixture's digests
MARGIN = 4.0              # a tolerance is MARGIN x the reference's own float32 distance from its float64 run ...
U = 2.0 ** -24            # ... or MARGIN x u where that distance is smaller
SGD_LR = 1e-2
PRODA_MODEL = "DeepLabv2-Resnet101-ProDA"
# online_proDA with the static prior alone (tests/golden/make_golden.py g8 "online_static"), the replay buffer on
STEP_SPEC = dict(SWITCH_PRIOR_THRESH=1, STATIC_LAMBDA=1, DYNAMIC_LAMBDA=0)
STEP_HEAD_SCALE = 40.0


def bn_param_names(model):
    """Names of the weight / bias of every BatchNorm2d of `model`, in module order."""
    return [f"{name}.{leaf}" for name, m in model.named_modules() if isinstance(m, torch.nn.BatchNorm2d) for leaf in ("weight", "bias")]


def tolerance(e_ref):
    return MARGIN * max(float(e_ref), U)
