"""Mirror of the reference's `networks` package (networks/__init__.py:1-4) for the three model
files on the hot path (DeepLabv3, DeepLabv3+, `simple`)."""
from . import deeplabv3, deeplabv3p, simple  # noqa: F401
from . import backbone  # noqa: F401
