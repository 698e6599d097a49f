"""Generation from trained directories (reference: inference/): ``Inference`` draws images from a generator, ``Controller`` sets attribute
groups of the w latent from attribute values through the trained controllers."""
from .controller import Controller          # noqa: F401
from .inference import Inference          # noqa: F401
