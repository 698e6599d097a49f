"""Attribute / contrastive (same - not-same) losses of the controllable generator step."""
from .loss_model import LossModelClass, CRITERIA, PREDICTORS, L1Expend, get_same_not_same_list  # noqa: F401
from .loss_model import RECON_LOSS_NAMES, RECON_SLICES, extract_futures_from_vec  # noqa: F401
from .arc_face import ArcFaceSkeleton, Backbone, embedding_loss_models  # noqa: F401
