"""fp64 oracle of the photometric transform of uint8 training frames (data/photometric.py, csrc/kernels/photometric.hip).

Plain torch fp64, explicit params, the five steps in the literal order of ``data/augment.py::PhotometricDistortions``
(brightness, then an HSV round trip for the saturation, a second one for the hue, then the per-frame per-channel
contrast), with that module's ``_rgb_to_hsv`` / ``_hsv_to_rgb`` conventions copied here so the oracle shares no code
with what it judges.  Also the comparison helper and the shared frame contents / parameter sets of the tests.
"""
import math

import numpy as np
import torch

# (B, T, H, W): word path with several windows; H*W odd (unaligned planes, byte path); fewer pixels than threads;
# a mid size; one full-size window
CASES = [(2, 3, 36, 52), (3, 2, 15, 21), (1, 1, 8, 8), (2, 2, 64, 80), (1, 2, 300, 300)]
CONTENTS = ("noise", "ramps", "grey", "primaries", "black", "white")

# default ranges of PhotometricDistortions: brightness 0.1, saturation [0.8, 1.2], hue 0.03, contrast [0.8, 1.2]
PARAM_SETS = {
    "corner_lo": (-0.1, 0.8, -0.03, 0.8),
    "corner_hi": (0.1, 1.2, 0.03, 1.2),
    "corner_lo_hi": (-0.1, 1.2, -0.03, 1.2),
    "corner_hi_lo": (0.1, 0.8, 0.03, 0.8),
    "identity": (0.0, 1.0, 0.0, 1.0),
    "brightness": (0.06817, 1.0, 0.0, 1.0),
    "saturation": (0.0, 1.13727, 0.0, 1.0),
    "hue": (0.0, 1.0, -0.02113, 1.0),
    "contrast": (0.0, 1.0, 0.0, 0.85391),
    "wide": (-0.5, 2.0, 0.5, 2.0),
}


def rgb_to_hsv(x):
    r, g, b = x.unbind(-3)
    mx, _ = x.max(-3)
    mn, _ = x.min(-3)
    d = mx - mn
    s = torch.where(mx > 0, d / mx.clamp_min(1e-12), torch.zeros_like(mx))
    dd = d.clamp_min(1e-12)
    h = torch.where(mx == r, ((g - b) / dd) % 6, torch.where(mx == g, (b - r) / dd + 2, (r - g) / dd + 4)) / 6
    h = torch.where(d > 0, h, torch.zeros_like(h))
    return h, s, mx


def hsv_to_rgb(h, s, v):
    h6 = (h % 1.0) * 6
    k = torch.stack([(5 + h6) % 6, (3 + h6) % 6, (1 + h6) % 6], dim=-3)
    return v.unsqueeze(-3) - v.unsqueeze(-3) * s.unsqueeze(-3) * (torch.minimum(k, 4 - k).clamp(0, 1))


def oracle_float(image_u8: torch.Tensor, params: torch.Tensor, frames_per_window: int) -> torch.Tensor:
    """uint8 [N, 3, H, W] (or [B, T, 3, H, W]) -> fp64 [N, 3, H, W] in [0, 1] after steps 1-4."""
    x = image_u8.reshape((-1,) + tuple(image_u8.shape[-3:])).to(torch.float64) / 255.0
    N = x.shape[0]
    assert N % frames_per_window == 0 and params.shape == (N // frames_per_window, 4)
    p = params.to(torch.float64).repeat_interleave(frames_per_window, 0)            # frame n -> window n // T
    db, fs, dh, fc = (p[:, i].view(N, 1, 1) for i in range(4))
    x = (x + db.unsqueeze(1)).clamp(0, 1)
    h, s, v = rgb_to_hsv(x)
    s = (s * fs).clamp(0, 1)
    x = hsv_to_rgb(h, s, v).clamp(0, 1)
    h, s, v = rgb_to_hsv(x)
    h = h + dh
    x = hsv_to_rgb(h, s, v).clamp(0, 1)
    mean = x.mean(dim=(-2, -1), keepdim=True)
    return ((x - mean) * fc.unsqueeze(1) + mean).clamp(0, 1)


def oracle_u8(image_u8: torch.Tensor, params: torch.Tensor, frames_per_window: int) -> torch.Tensor:
    out = torch.round(oracle_float(image_u8, params, frames_per_window) * 255.0)     # torch.round: half to even
    return out.to(torch.uint8).reshape(image_u8.shape)


def compare(got: torch.Tensor, ref: torch.Tensor):
    """(largest byte difference, bytes that differ, allowed count = ceil(1e-3 * bytes))."""
    d = (got.cpu().to(torch.int16) - ref.cpu().to(torch.int16)).abs()
    return int(d.max()) if d.numel() else 0, int((d > 0).sum()), int(math.ceil(1e-3 * d.numel()))


def within_tolerance(got, ref) -> bool:
    mx, cnt, cap = compare(got, ref)
    return mx <= 1 and cnt <= cap


def assert_close(got, ref, what=""):
    mx, cnt, cap = compare(got, ref)
    assert mx <= 1 and cnt <= cap, f"{what}: max byte difference {mx} (allowed 1), {cnt} bytes differ (allowed {cap})"


def content(kind: str, H: int, W: int, seed: int) -> np.ndarray:
    """One uint8 [3, H, W] frame."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    if kind == "ramps":
        x = np.linspace(0, 255, W)
        return np.stack([np.tile(x, (H, 1)), np.tile(x[::-1], (H, 1)), np.tile((2 * x) % 256, (H, 1))]).astype(np.uint8)
    if kind == "grey":
        return np.repeat(rng.integers(0, 256, (1, H, W), dtype=np.uint8), 3, 0)
    if kind == "primaries":
        idx = (3 * np.arange(H)[:, None] + 5 * np.arange(W)[None, :]) % 8          # the 8 corners of the RGB cube
        return np.stack([(idx >> c & 1) * 255 for c in range(3)]).astype(np.uint8)
    if kind == "black":
        return np.zeros((3, H, W), np.uint8)
    if kind == "white":
        return np.full((3, H, W), 255, np.uint8)
    raise ValueError(kind)


def case_image(case, rotation: int) -> torch.Tensor:
    """[B, T, 3, H, W] uint8: frame i holds CONTENTS[(i + rotation) % 6], so six rotations put every content in
    every frame slot (and under every window's params)."""
    B, T, H, W = case
    frames = [content(CONTENTS[(i + rotation) % len(CONTENTS)], H, W, seed=1000 * rotation + i) for i in range(B * T)]
    return torch.from_numpy(np.stack(frames)).view(B, T, 3, H, W)


def case_params(case, first: int) -> torch.Tensor:
    """[B, 4] fp32: window w takes PARAM_SETS entry (first + w) % 10."""
    names = list(PARAM_SETS)
    return torch.tensor([PARAM_SETS[names[(first + w) % len(names)]] for w in range(case[0])], dtype=torch.float32)


def case_runs(case):
    """Every (rotation, first) run of a case: each content meets each parameter set in every case."""
    for rot in range(len(CONTENTS)):
        for first in range(len(PARAM_SETS)):
            yield rot, first
