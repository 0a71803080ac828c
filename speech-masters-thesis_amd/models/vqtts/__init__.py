from .align import TextAudioAlignment
from .bottleneck import Bottleneck
from .predictor import CodePredictor

__all__ = ["Bottleneck", "CodePredictor", "TextAudioAlignment"]
