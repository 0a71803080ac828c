from .align import TextAudioAlignment
from .bottleneck import Bottleneck
from .predictor import CodePredictor
from .vqtts import VQTTS

__all__ = ["Bottleneck", "CodePredictor", "TextAudioAlignment", "VQTTS"]
