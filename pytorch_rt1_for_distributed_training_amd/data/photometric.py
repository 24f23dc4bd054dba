"""Photometric augmentation of decoded uint8 training frames (the RT-1 input path).

The behaviour-cloning stack already has ``data/augment.py::PhotometricDistortions`` (brightness, saturation, hue,
contrast; ``language_table/train/input_pipeline_rlds.py:390-457``) as float torch ops.  The RT-1 path keeps its frames
uint8 from the shard to the stem kernel, so here the same transform runs in place on the decoded planar bytes: one
HIP launch per batch (``csrc/kernels/photometric.hip``) on the stream the crop kernel ran on.

One window of T frames shares four numbers ``(db, fs, dh, fc)``.  Per pixel:

1. ``c = u8 / 255``
2. brightness ``c = clamp(c + db, 0, 1)``
3. ``(h, s, v) = rgb_to_hsv``; ``s = clamp(s * fs, 0, 1)``; ``h = h + dh``; ``rgb = hsv_to_rgb(h mod 1, s, v)``
4. contrast about the frame's own per-channel mean after step 3: ``c = clamp((c - m) * fc + m, 0, 1)``
5. ``u8 = round_half_even(c * 255)``

:func:`photometric_u8_` takes the HIP kernel for GPU tensors and :func:`photometric_u8_reference` (torch fp32, the
same five steps) for CPU tensors.  Steps 1-4 are fp32 in both.  Two places are exact in both, because flat frames
(padding, a black or white background) would otherwise sit on rounding ties for a whole frame at once: the mean is the
exact sum rounded once (so a flat frame's mean is its value), and step 5 rounds the exact product ``c * 255``.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .augment import PhotometricDistortions


def check_spec(spec: PhotometricDistortions) -> PhotometricDistortions:
    """Refuse ranges the transform has no meaning for (NaN fails every comparison)."""
    if not 0.0 <= spec.brightness_max_delta <= 1.0:
        raise ValueError(f"photometric brightness delta must be in [0, 1], got {spec.brightness_max_delta}")
    if not 0.0 <= spec.saturation_lower <= spec.saturation_upper < float("inf"):
        raise ValueError(f"photometric saturation range needs 0 <= lo <= hi, got "
                         f"[{spec.saturation_lower}, {spec.saturation_upper}]")
    if not 0.0 <= spec.hue_max_delta <= 0.5:
        raise ValueError(f"photometric hue delta must be in [0, 0.5] turns, got {spec.hue_max_delta}")
    if not 0.0 <= spec.contrast_lower <= spec.contrast_upper < float("inf"):
        raise ValueError(f"photometric contrast range needs 0 <= lo <= hi, got "
                         f"[{spec.contrast_lower}, {spec.contrast_upper}]")
    return spec


def photometric_params(rng: np.random.Generator, windows: int, spec: PhotometricDistortions) -> np.ndarray:
    """float32 [windows, 4] of (db, fs, dh, fc), uniform in the spec's ranges.  A stage whose range is the identity
    yields exactly 0 or 1 (and still consumes its draws, so the other stages' draws do not depend on it)."""
    check_spec(spec)
    u = rng.random((int(windows), 4))
    lo = np.asarray([-spec.brightness_max_delta, spec.saturation_lower, -spec.hue_max_delta, spec.contrast_lower])
    hi = np.asarray([spec.brightness_max_delta, spec.saturation_upper, spec.hue_max_delta, spec.contrast_upper])
    out = (lo + u * (hi - lo)).astype(np.float32)
    np.clip(out, lo.astype(np.float32), hi.astype(np.float32), out=out)      # the fp32 rounding may step outside
    for i in range(4):
        if lo[i] == hi[i]:
            out[:, i] = lo[i]
    return out


def photometric_generator(seed: int, epoch: int, rank: int) -> np.random.Generator:
    """The loaders' generator for the photometric draws: keyed like their crop generator on (seed, epoch, rank), plus
    a constant of its own, so crop boxes and the shuffle do not depend on whether the option is on."""
    return np.random.default_rng([0x9E3779B1, int(seed), int(epoch), int(rank)])


def _check(image: torch.Tensor, params: torch.Tensor, frames_per_window: int) -> int:
    if image.dtype != torch.uint8 or image.dim() not in (4, 5) or image.shape[-3] != 3 or not image.is_contiguous():
        raise ValueError(f"photometric_u8_: image must be contiguous uint8 [N, 3, H, W] or [B, T, 3, H, W], got "
                         f"{image.dtype} {tuple(image.shape)}")
    n = image.shape[0] if image.dim() == 4 else image.shape[0] * image.shape[1]
    T = int(frames_per_window)
    if T <= 0 or n % T != 0:
        raise ValueError(f"photometric_u8_: {n} frames are not a whole number of windows of {T}")
    if params.dtype != torch.float32 or tuple(params.shape) != (n // T, 4) or params.device != image.device:
        raise ValueError(f"photometric_u8_: params must be float32 [{n // T}, 4] on {image.device}, got "
                         f"{params.dtype} {tuple(params.shape)} on {params.device}")
    return n


def photometric_u8_reference(image: torch.Tensor, params: torch.Tensor, frames_per_window: int) -> torch.Tensor:
    """The five steps in torch fp32 (out of place): the CPU path of :func:`photometric_u8_`."""
    n = _check(image, params, frames_per_window)
    if n == 0:
        return image.clone()
    x = image.reshape((n,) + tuple(image.shape[-3:])).to(torch.float32) / 255.0
    p = params.repeat_interleave(int(frames_per_window), 0)                 # frame n -> window n // T
    db, fs, dh, fc = (p[:, i].view(n, 1, 1) for i in range(4))
    r, g, b = (x + db.unsqueeze(1)).clamp(0, 1).unbind(1)
    mx = torch.maximum(torch.maximum(r, g), b)
    mn = torch.minimum(torch.minimum(r, g), b)
    d = mx - mn
    one = torch.ones_like(d)
    s = torch.where(mx > 0, d / torch.where(mx > 0, mx, one), torch.zeros_like(d))
    s = (s * fs).clamp(0, 1)
    rd = 1.0 / torch.where(d > 0, d, one)
    h6 = torch.where(mx == r, (g - b) * rd, torch.where(mx == g, (b - r) * rd + 2, (r - g) * rd + 4))
    h = torch.where(d > 0, h6 / 6, torch.zeros_like(d)) + dh
    h6 = (h - torch.floor(h)) * 6
    vs = mx * s
    out = []
    for k0 in (5.0, 3.0, 1.0):
        k = h6 + k0
        k = torch.where(k >= 6, k - 6, k)
        out.append((mx - vs * torch.minimum(k, 4 - k).clamp(0, 1)).clamp(0, 1))
    x = torch.stack(out, 1)
    mean = x.mean(dim=(-2, -1), keepdim=True, dtype=torch.float64).to(torch.float32)   # exact sum, rounded once
    x = ((x - mean) * fc.unsqueeze(1) + mean).clamp(0, 1)
    return torch.round(x.to(torch.float64) * 255.0).to(torch.uint8).reshape(image.shape)  # exact product, half-even


def photometric_u8_(image: torch.Tensor, params: torch.Tensor, frames_per_window: int) -> torch.Tensor:
    """In place on ``image`` (uint8 [N, 3, H, W] or [B, T, 3, H, W]); ``params`` float32 [N / frames_per_window, 4]
    on the same device.  GPU tensors: one HIP launch on the current stream.  CPU tensors: the torch fp32 path."""
    if image.is_cuda:
        from ..ops import load
        load().photometric_u8_(image, params, int(frames_per_window))
        return image
    image.copy_(photometric_u8_reference(image, params, frames_per_window))
    return image


def apply_to_decoded(image: torch.Tensor, params: Optional[torch.Tensor]) -> torch.Tensor:
    """Decode hook of the loaders: ``image`` [B, T, 3, H, W] just decoded, ``params`` [B, 4] or None (option off:
    nothing runs)."""
    if params is None:
        return image
    return photometric_u8_(image, params.to(image.device, non_blocking=True).contiguous(), image.shape[1])
