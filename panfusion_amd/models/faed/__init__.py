from .FAED import FrechetAutoEncoderDistance  # noqa: F401
from .modules import Encoder  # noqa: F401
