"""Attention scores and saliency through the public interface, on the CPU (tiny preset, torch backend): the config flag,
the TokenLearner maps, the engine's rolling map window, the saliency function, the rollout's second GIF."""
import os

import numpy as np
import pytest
import torch

import pytorch_rt1_for_distributed_training_amd as rt1
from pytorch_rt1_for_distributed_training_amd.config import RT1Config
from pytorch_rt1_for_distributed_training_amd.engine.infer import InferenceEngine, saliency
from pytorch_rt1_for_distributed_training_amd.models import build_rt1


def tiny(**kw):
    return rt1.preset("tiny").replace(crop_ratio=0.0, **kw)


def test_config_flag_reaches_the_model():
    assert RT1Config().return_attention_scores is False
    cfg = tiny(return_attention_scores=True)
    torch.manual_seed(0)
    on = build_rt1(cfg).eval()
    torch.manual_seed(0)
    off = build_rt1(tiny()).eval()
    img = torch.rand(2, cfg.seq_len, 3, cfg.height, cfg.width)
    ctx = torch.randn(2, cfg.seq_len, 512)
    act = {"terminate_episode": torch.zeros(2, cfg.seq_len, dtype=torch.long),
           "action": torch.zeros(2, cfg.seq_len, 2)}
    with torch.no_grad():
        l_on, _ = on.train_forward(img, ctx, act)
        l_off, _ = off.train_forward(img, ctx, act)
    S = cfg.seq_len * on.tokens_per_step
    assert len(on.attention_scores) == cfg.num_layers
    assert all(a.shape == (2, cfg.num_heads, S, S) for a in on.attention_scores)
    assert off.attention_scores == [] and off.token_maps is None
    assert torch.equal(l_on, l_off), "the flag changed the forward"
    # the maps: [b, t, 8, P] fp32, a softmax over the P positions of each frame
    P = on._image_tokenizer._feature_positions
    assert on.token_maps.shape == (2, cfg.seq_len, 8, P) and on.token_maps.dtype == torch.float32
    torch.testing.assert_close(on.token_maps.sum(-1), torch.ones(2, cfg.seq_len, 8), rtol=0, atol=P * 2.0 ** -23)
    assert float(on.token_maps.min()) >= 0.0


def test_saliency_against_a_loop():
    g = torch.Generator().manual_seed(3)
    b, H, T, K, A, P = 2, 3, 3, 4, 2, 5
    L = K + A
    S = T * L
    attn = torch.rand(b, H, S, S, generator=g)
    maps = torch.rand(b, T, K, P, generator=g)
    rows = torch.tensor([K - 1 + L, K + L])                     # the predicting rows of step 1
    got = saliency(attn, maps, rows, K, L)
    ref = torch.zeros(b, T, P, dtype=torch.float64)
    for bi in range(b):
        for t in range(T):
            for k in range(K):
                w = 0.0
                for h in range(H):
                    for r in rows.tolist():
                        w += float(attn[bi, h, r, t * L + k])
                w /= H * len(rows)
                for p in range(P):
                    ref[bi, t, p] += w * float(maps[bi, t, k, p])
    assert got.shape == (b, T, P)
    torch.testing.assert_close(got.double(), ref, rtol=1e-5, atol=1e-6)


def test_engine_maps_follow_the_image_window_through_the_roll():
    """state_maps is rolled and written with state_img's indices: at every step slot t of both belongs to the same
    frame, checked against a second model that re-tokenizes each stored frame (indexing of tests/test_infer.py)."""
    cfg = tiny(seq_len=3, return_attention_scores=True)
    torch.manual_seed(0)
    eng = InferenceEngine(build_rt1(cfg), cfg, device="cpu", backend="torch")
    torch.manual_seed(0)
    ref = build_rt1(cfg).eval()
    T, K, L, A = eng.T, eng.K, eng.L, eng.A
    g = torch.Generator().manual_seed(1)
    window = []                                                  # (tokens, maps) of the frames in the window, oldest first
    for step in range(8):
        img = torch.randint(0, 256, (1, 3, 64, 64), generator=g, dtype=torch.uint8)
        ctx = torch.randn(1, 512, generator=g)
        with torch.no_grad():
            tok = ref.tokenize_images(img[:, None].float() / 255.0, ctx[:, None])
        window = (window + [(tok[:, 0], ref.token_maps[:, 0].clone())])[-T:]
        eng.step(img, ctx)
        n = len(window)
        assert eng.state_maps.shape == (1, T, K, eng.fmap[0] * eng.fmap[1])
        for t, (tk, mp) in enumerate(window):
            torch.testing.assert_close(eng.state_img[:, t], tk.float(), rtol=1e-5, atol=1e-5)
            torch.testing.assert_close(eng.state_maps[:, t], mp, rtol=1e-5, atol=1e-6)
        assert not eng.state_maps[:, n:].any()
        # attention and saliency of the step
        assert len(eng.last_attention) == cfg.num_layers
        assert eng.last_attention[-1].shape == (1, cfg.num_heads, T * L, T * L)
        for a, live in zip(eng.last_attention, eng.model.attention_scores):
            assert torch.equal(a, live.float())
        ts = min(step, T - 1)
        rows = torch.arange(K - 1 + ts * L, K - 1 + ts * L + A)
        w = eng.last_attention[-1][:, :, rows].mean(dim=(1, 2)).view(1, T, L)[:, :, :K]
        assert eng.last_saliency.shape == (1, T, *eng.fmap)
        torch.testing.assert_close(eng.last_saliency.sum((1, 2, 3)), w.sum((1, 2)), rtol=0, atol=1e-5)
        assert not eng.last_saliency[:, ts + 1:].any(), "frames after the current step got attention"
        assert float(eng.last_saliency[:, ts].sum()) > 0
    eng.reset()
    assert not eng.state_maps.any()


def test_engine_without_the_flag_has_no_explanation_state():
    cfg = tiny()
    eng = InferenceEngine(build_rt1(cfg), cfg, device="cpu", backend="torch")
    assert eng.last_attention is None and eng.last_saliency is None and eng.state_maps is None
    eng.step(torch.zeros(1, 3, 64, 64, dtype=torch.uint8), torch.zeros(1, 512))
    assert eng.model.attention_scores == []


def test_saliency_without_token_learner_is_refused():
    cfg = tiny(use_token_learner=False, return_attention_scores=True)
    with pytest.raises(ValueError, match="use_token_learner"):
        InferenceEngine(build_rt1(cfg), cfg, device="cpu", backend="torch")
    import eval_rt1
    with pytest.raises(SystemExit):
        eval_rt1.main(["--ckpt", "none.ckpt", "--saliency", "--no_token_learner"])


def test_rollout_writes_a_saliency_gif_next_to_each_video(tmp_path):
    from PIL import Image

    from pytorch_rt1_for_distributed_training_amd.eval import CentralCropResize, RT1Policy, ToyPushEnv, evaluate
    cfg = tiny(return_attention_scores=True)
    torch.manual_seed(0)
    policy = RT1Policy(build_rt1(cfg), device="cpu", cfg=cfg, backend="torch")
    res = evaluate(policy, ToyPushEnv(seed=0), episodes=2, max_episode_steps=3, crop=CentralCropResize(64, 64),
                   history_length=cfg.seq_len, video_dir=str(tmp_path), name="toy", saliency=True)
    assert res["episodes"] == 2
    sal = policy.last_saliency()
    assert sal.shape == (1, cfg.seq_len, *policy.engine.fmap)
    assert policy.last_saliency(newest=True).shape == tuple(policy.engine.fmap)
    files = sorted(os.listdir(tmp_path))
    plain = [f for f in files if not f.endswith("_saliency.gif")]
    assert len(plain) == 2 and len(files) == 4
    for f in plain:
        s = f[:-len(".gif")] + "_saliency.gif"
        assert s in files
        a, b = Image.open(tmp_path / f), Image.open(tmp_path / s)
        assert a.n_frames == b.n_frames >= 2
        a.seek(1)
        b.seek(1)
        fa = np.asarray(a.convert("RGB").resize(b.size), dtype=np.int32)
        fb = np.asarray(b.convert("RGB"), dtype=np.int32)
        assert np.abs(fa - fb).max() > 0, "the saliency GIF shows the plain frames"
    # a policy built without the flag has nothing to show
    plain_policy = RT1Policy(build_rt1(tiny()), device="cpu", cfg=tiny(), backend="torch")
    with pytest.raises(ValueError, match="return_attention_scores"):
        plain_policy.last_saliency()
