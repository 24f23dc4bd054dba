"""Closed-loop evaluation loop (reference ``language_table/eval/main_rt1.py:100-201``).

Per episode: zero the policy state, reset the env, feed the centrally cropped
frame + instruction embedding, step until the env reports success or
``max_episode_steps`` is exceeded (the reference breaks once ``episode_steps >
80``, i.e. after at most 81 policy steps), record rendered frames and count
successes.  Videos are written as animated GIF (PIL) instead of mp4 (imageio is
not a dependency).
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional

import numpy as np

from .envs import CentralCropResize, History

try:
    from PIL import Image
except ImportError:  # pragma: no cover
    Image = None


def save_gif(frames: List[np.ndarray], path: str, fps: int = 10):
    imgs = [Image.fromarray(np.asarray(f, dtype=np.uint8)) for f in frames]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    imgs[0].save(path, save_all=True, append_images=imgs[1:], duration=int(1000 / fps), loop=0)


def blend_saliency(frame: np.ndarray, sal: np.ndarray, alpha: float = 0.6) -> np.ndarray:
    """frame (H, W, 3) uint8 with the (h', w') saliency map upsampled (bilinear) to it, scaled to its own maximum and
    blended in as red: where the map peaks the pixel is ``alpha`` red, where it is 0 the frame is dimmed only."""
    frame = np.asarray(frame, dtype=np.uint8)
    H, W = frame.shape[:2]
    m = np.asarray(sal, dtype=np.float32)
    m = m / max(float(m.max()), 1e-12)
    m = np.asarray(Image.fromarray(m, mode="F").resize((W, H), Image.BILINEAR), dtype=np.float32)
    m = np.clip(m, 0.0, 1.0)[..., None] * alpha
    out = 0.7 * frame.astype(np.float32) * (1.0 - m) + np.array([255.0, 0.0, 0.0], dtype=np.float32) * m
    return np.clip(out + 0.5, 0, 255).astype(np.uint8)


def evaluate(policy, env, episodes: int = 10, max_episode_steps: int = 80, crop: Optional[CentralCropResize] = None,
             history_length: int = 6, video_dir: Optional[str] = None, name: str = "blocktoblock",
             saliency: bool = False) -> Dict[str, float]:
    """``saliency``: next to each episode's video, a second GIF (``..._saliency.gif``, same frame count) of the frames
    the policy was given, each blended with the saliency map of its own step (``RT1Policy.last_saliency``); the last
    frame, which no step has read, is shown with an empty map."""
    crop = crop or CentralCropResize()
    hist = History(history_length)
    if saliency and not hasattr(policy, "last_saliency"):
        raise ValueError("evaluate(saliency=True) needs a policy with last_saliency() (RT1Policy)")
    successes = 0
    lengths = []
    for ep in range(episodes):
        policy.reset()
        obs = env.reset()
        frames = [env.render()]
        h = hist.reset({"rgb": crop(obs["rgb"]), "emb": obs["instruction_embedding"]})
        steps = 0
        done = False
        sal_frames = []
        while not done:
            action = policy.action(h["rgb"], h["emb"])
            if saliency:
                sal_frames.append(blend_saliency(np.asarray(h["rgb"])[-1], policy.last_saliency(newest=True)))
            obs, _, done, _ = env.step(action)
            frames.append(env.render())
            h = hist.push({"rgb": crop(obs["rgb"]), "emb": obs["instruction_embedding"]})
            steps += 1
            if steps > max_episode_steps:
                break
        ok = bool(env.succeeded)
        successes += int(ok)
        lengths.append(steps)
        if video_dir:
            stem = os.path.join(video_dir, f"{name}_{ep}_{'success' if ok else 'failure'}")
            save_gif(frames, stem + ".gif")
            if saliency:
                last = np.asarray(h["rgb"])[-1]
                sal_frames.append(blend_saliency(last, np.zeros((1, 1), np.float32)))
                save_gif(sal_frames, stem + "_saliency.gif")
    return {name: successes, "episodes": episodes, "success_rate": successes / max(episodes, 1),
            "mean_steps": float(np.mean(lengths)) if lengths else 0.0}
