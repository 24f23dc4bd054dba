"""``torch | hip | auto`` -> ``torch | hip``, shared by the ops that have both a torch and a HIP form."""
from __future__ import annotations

from typing import Callable

import torch

from ._ext import available


def resolve(backend: str, supported: Callable[[], bool], unserved: str) -> str:
    """``hip`` needs a GPU, the extension and a shape that ``supported()`` accepts, and the ``ValueError`` says which
    is missing (``unserved`` describes the shape); ``auto`` is ``hip`` exactly when all three hold."""
    if backend not in ("torch", "hip", "auto"):
        raise ValueError(f"backend is {backend!r}, expected 'torch', 'hip' or 'auto'")
    if backend == "torch":
        return backend
    cuda = torch.cuda.is_available()
    if backend == "auto":
        return "hip" if (cuda and supported()) else "torch"
    if not cuda:
        raise ValueError("the hip backend needs a GPU")
    if not available():
        raise ValueError("the hip backend needs the HIP extension (python build.py)")
    if not supported():
        raise ValueError(f"the hip backend does not serve {unserved}")
    return backend
