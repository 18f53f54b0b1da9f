from .VRNN import VRNN  # noqa: F401
