"""Text side of the open-vocabulary classifier: the CLIP text encoder and its tokenizer."""
from .text_encoder import CLIPTEXT, SimpleTokenizer, build_text_encoder  # noqa
