from .averagemodel import SimpleLinearModel  # noqa: F401
