from .bottleneck import Bottleneck

__all__ = ["Bottleneck"]
