from .align import TextAudioAlignment
from .bottleneck import Bottleneck

__all__ = ["Bottleneck", "TextAudioAlignment"]
