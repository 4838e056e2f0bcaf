from .model_handler import enable_resnet101_proda, get_model  # noqa: F401
from .adaptation_method_handler import enable_proto_advent, get_adapt_method  # noqa: F401
