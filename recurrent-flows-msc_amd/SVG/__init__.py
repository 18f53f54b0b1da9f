from .SVG import SVG  # noqa: F401
