"""Host-side mirrors of the ``parakeet.utils`` helpers the synthesis recipes import (``layer_tools``); checkpoint reading
lives in ``parakeet_amd.checkpoint`` (parakeet/utils/checkpoint.py's role).  ``error_rate`` is parakeet/utils/error_rate.py
with the distance taken on the engine."""
from . import error_rate, layer_tools  # noqa: F401
