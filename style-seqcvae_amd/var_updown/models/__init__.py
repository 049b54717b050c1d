from .ensemble import CaptionerEnsemble
from .updown_captioner import UpDownCaptioner

__all__ = ["CaptionerEnsemble", "UpDownCaptioner"]
