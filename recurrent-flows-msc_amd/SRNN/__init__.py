from .SRNN import SRNN  # noqa: F401
