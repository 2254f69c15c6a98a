"""Mirror of the reference's `networks` package (networks/__init__.py:1-4): its four model
files (DeepLabv3, DeepLabv3+, PSPNet, `simple`)."""
from . import deeplabv3, deeplabv3p, psp, simple  # noqa: F401
from . import backbone  # noqa: F401
