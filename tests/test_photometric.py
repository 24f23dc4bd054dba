"""Photometric augmentation of uint8 training frames (data/photometric.py), CPU side: the fp32 torch path against the
fp64 oracle (tests/photometric_oracle.py) on the cases the GPU test uses, the oracle against the existing
``PhotometricDistortions``, planted faults, the draws, the loaders and the command line.

Tolerance (photometric_oracle.compare): no byte differs by more than 1 and at most ceil(1e-3 * bytes) bytes differ.
Frame contents and the stage-alone parameter values avoid points where the exact-arithmetic result is a rounding tie
k + 0.5 for a whole class of pixels (short decimal factors such as 1.15 put every pixel with max - min = 10, 30, ... on
one; a noise field of RGB-cube corners does whenever its count of set pixels hits the wrong residue): there the fp64
oracle's own rounding error decides the byte, and a comparison with it says nothing.  The issue's fixed parameter sets
(the corners +-0.1 / 0.8 / 1.2 / +-0.03, the identity, -0.5 / 2 / 0.5 / 2) are used as given.
"""
import os

import numpy as np
import pytest
import torch

import photometric_oracle as O
from pytorch_rt1_for_distributed_training_amd.data import episodes as E
from pytorch_rt1_for_distributed_training_amd.data import photometric as P
from pytorch_rt1_for_distributed_training_amd.data import resident as R
from pytorch_rt1_for_distributed_training_amd.data import shards as S
from pytorch_rt1_for_distributed_training_amd.data.augment import PhotometricDistortions


@pytest.mark.parametrize("case", O.CASES, ids=lambda c: "x".join(map(str, c)))
def test_fp32_path_within_tolerance_of_oracle(case):
    total = differ = 0
    for rot, first in O.case_runs(case):
        img, prm = O.case_image(case, rot), O.case_params(case, first)
        got = P.photometric_u8_reference(img, prm, case[1])
        ref = O.oracle_u8(img, prm, case[1])
        O.assert_close(got, ref, f"case {case} rotation {rot} first param set {first}")
        total += img.numel()
        differ += O.compare(got, ref)[1]
    print(f"case {case}: {differ} of {total} bytes differ from the oracle ({differ / total:.2e})")


def test_oracle_equals_photometric_distortions_fp64():
    """The oracle fed the draws PhotometricDistortions makes from a seeded generator equals that class in fp64."""
    B, T, H, W = 3, 2, 20, 28
    img = O.case_image((B, T, H, W), 0)
    spec = PhotometricDistortions()
    g = torch.Generator().manual_seed(7)
    want = spec(img.to(torch.float64) / 255.0, g)
    g = torch.Generator().manual_seed(7)
    u = lambda lo, hi: torch.rand(B, generator=g) * (hi - lo) + lo           # the class's draw order
    db = u(-spec.brightness_max_delta, spec.brightness_max_delta)
    fs = u(spec.saturation_lower, spec.saturation_upper)
    dh = u(-spec.hue_max_delta, spec.hue_max_delta)
    fc = u(spec.contrast_lower, spec.contrast_upper)
    got = O.oracle_float(img, torch.stack([db, fs, dh, fc], 1), T).view(B, T, 3, H, W)
    assert torch.allclose(got, want, rtol=0, atol=1e-12), float((got - want).abs().max())


@pytest.mark.parametrize("case", O.CASES[:4], ids=lambda c: "x".join(map(str, c)))
def test_identity_params_are_bitwise_identity(case):
    img = O.case_image(case, 0)
    prm = torch.tensor([[0.0, 1.0, 0.0, 1.0]]).repeat(case[0], 1)
    assert torch.equal(P.photometric_u8_reference(img, prm, case[1]), img)
    assert torch.equal(O.oracle_u8(img, prm, case[1]), img)
    out = img.clone()
    assert P.photometric_u8_(out, prm, case[1]) is out and torch.equal(out, img)      # the in-place entry


# ---- planted faults: each must be caught by the oracle comparison on at least one listed case

def _flat(img):
    return img.reshape((-1,) + tuple(img.shape[-3:]))


def _fault_window_mean(img, prm, T):
    """contrast mean over the window instead of the frame: finish the colour steps per frame, then apply the contrast
    about the window's mean"""
    ident = prm.clone()
    ident[:, 3] = 1.0
    x = _flat(P.photometric_u8_reference(img, ident, T)).float() / 255.0
    n = x.shape[0]
    m = x.view(n // T, T, 3, -1).mean(dim=(1, 3)).repeat_interleave(T, 0).view(n, 3, 1, 1)
    fc = prm[:, 3].repeat_interleave(T).view(n, 1, 1, 1)
    return torch.round(((x - m) * fc + m).clamp(0, 1) * 255).to(torch.uint8).view(img.shape)


def _fault_one_mean(img, prm, T):
    ident = prm.clone()
    ident[:, 3] = 1.0
    x = _flat(P.photometric_u8_reference(img, ident, T)).float() / 255.0
    n = x.shape[0]
    m = x.mean(dim=(1, 2, 3), keepdim=True)
    fc = prm[:, 3].repeat_interleave(T).view(n, 1, 1, 1)
    return torch.round(((x - m) * fc + m).clamp(0, 1) * 255).to(torch.uint8).view(img.shape)


def _fault_param_index(img, prm, T):
    """params indexed by n % T instead of n // T (rows past the table wrap)"""
    n = _flat(img).shape[0]
    rows = prm[torch.arange(n) % T % prm.shape[0]]
    return P.photometric_u8_reference(_flat(img), rows, 1).view(img.shape)


def _fault_hue_sign(img, prm, T):
    p = prm.clone()
    p[:, 2] = -p[:, 2]
    return P.photometric_u8_reference(img, p, T)


def _fault_no_brightness_clamp(img, prm, T):
    """c + db carried unclamped into the HSV steps (v > 1 or < 0); later clamps still apply"""
    x = _flat(img).float() / 255.0
    n = x.shape[0]
    p = prm.repeat_interleave(T, 0)
    x = x + p[:, 0].view(n, 1, 1, 1)
    h, s, v = O.rgb_to_hsv(x)
    s = (s * p[:, 1].view(n, 1, 1)).clamp(0, 1)
    x = O.hsv_to_rgb(h + p[:, 2].view(n, 1, 1), s, v).clamp(0, 1)
    m = x.mean(dim=(2, 3), keepdim=True)
    x = ((x - m) * p[:, 3].view(n, 1, 1, 1) + m).clamp(0, 1)
    return torch.round(x * 255).to(torch.uint8).view(img.shape)


def _fault_tail_untouched(img, prm, T):
    """the last partial 4-pixel group of every plane keeps its input bytes"""
    out = P.photometric_u8_reference(img, prm, T)
    hw = img.shape[-1] * img.shape[-2]
    if hw % 4:
        o, i = out.view(-1, hw), img.reshape(-1, hw)
        o[:, hw - hw % 4:] = i[:, hw - hw % 4:]
    return out


def _fault_truncate(img, prm, T):
    ident_free = O.oracle_float(img, prm, T)
    return torch.floor(ident_free * 255.0).to(torch.uint8).view(img.shape)


FAULTS = {"window_mean": _fault_window_mean, "one_mean_for_three_channels": _fault_one_mean,
          "param_index_n_mod_T": _fault_param_index, "hue_sign": _fault_hue_sign,
          "brightness_clamp_missing": _fault_no_brightness_clamp, "tail_group_untouched": _fault_tail_untouched,
          "truncation": _fault_truncate}


@pytest.mark.parametrize("name", list(FAULTS))
def test_planted_fault_is_caught(name):
    caught = 0
    for case in O.CASES[:4]:
        for rot, first in O.case_runs(case):
            img, prm = O.case_image(case, rot), O.case_params(case, first)
            caught += not O.within_tolerance(FAULTS[name](img, prm, case[1]), O.oracle_u8(img, prm, case[1]))
        if caught:
            break
    assert caught, f"planted fault {name} passes the oracle comparison on every case"


# ---- draws

def test_params_in_range_and_identity_stages_exact():
    rng = np.random.default_rng(3)
    spec = PhotometricDistortions()
    p = P.photometric_params(rng, 4096, spec)
    assert p.dtype == np.float32 and p.shape == (4096, 4)
    lo = np.float32([-0.1, 0.8, -0.03, 0.8])
    hi = np.float32([0.1, 1.2, 0.03, 1.2])
    assert (p >= lo).all() and (p <= hi).all()
    assert ((p.max(0) - p.min(0)) > 0.9 * (hi - lo)).all()                   # the draws fill the ranges
    ident = PhotometricDistortions(brightness_max_delta=0.0, hue_max_delta=0.0, saturation_lower=1.0,
                                   saturation_upper=1.0, contrast_lower=1.0, contrast_upper=1.0)
    assert np.array_equal(P.photometric_params(rng, 5, ident), np.tile(np.float32([0, 1, 0, 1]), (5, 1)))
    one = PhotometricDistortions(brightness_max_delta=0.0, contrast_lower=1.0, contrast_upper=1.0)
    q = P.photometric_params(rng, 64, one)
    assert (q[:, 0] == 0).all() and (q[:, 3] == 1).all() and q[:, 1].std() > 0 and q[:, 2].std() > 0


@pytest.mark.parametrize("bad", [dict(brightness_max_delta=-0.1), dict(brightness_max_delta=1.5),
                                 dict(saturation_lower=1.3), dict(saturation_lower=-0.1),
                                 dict(hue_max_delta=0.6), dict(hue_max_delta=float("nan")),
                                 dict(contrast_lower=2.0, contrast_upper=1.0)])
def test_bad_ranges_refused(bad):
    with pytest.raises(ValueError, match="photometric"):
        P.photometric_params(np.random.default_rng(0), 2, PhotometricDistortions(**bad))


def test_bad_arguments_refused():
    img = torch.zeros(4, 3, 5, 6, dtype=torch.uint8)
    prm = torch.tensor([[0.0, 1.0, 0.0, 1.0]]).repeat(2, 1)
    P.photometric_u8_(img, prm, 2)
    with pytest.raises(ValueError):
        P.photometric_u8_(img.float(), prm, 2)
    with pytest.raises(ValueError):
        P.photometric_u8_(img, prm[:1], 2)
    with pytest.raises(ValueError):
        P.photometric_u8_(img, prm, 3)
    empty = torch.zeros(0, 3, 5, 6, dtype=torch.uint8)
    assert P.photometric_u8_(empty, prm[:0], 2).shape == empty.shape


# ---- loaders

@pytest.fixture()
def shard(tmp_path):
    ids = E.make_fake_episodes(str(tmp_path / "npz"), 6, steps=6, height=40, width=56, seed=2)
    S.pack_shard(str(tmp_path / "npz"), ids, str(tmp_path / "shard"))
    return str(tmp_path / "shard")


def _host_batches(path, epoch, photometric):
    ld = S.ShardBatchLoader(path, 4, 3, 0.9, seed=5, pin=False, threads=2, photometric=photometric)
    ld.set_epoch(epoch)
    return [{k: v.clone() for k, v in b["train_observation"].items()} for b in ld]


def _plans(path, epoch, photometric):
    ld = R.ResidentBatchLoader(R.ResidentShard(path, "cpu"), 4, 3, 0.9, seed=5, pin=False, photometric=photometric)
    ld.set_epoch(epoch)
    return [{k: v.clone() for k, v in b.items()} for b in ld]


@pytest.mark.parametrize("batches,order", [(_host_batches, "raw_frames"), (_plans, "plan_rows")])
def test_loader_option_leaves_boxes_and_order_alone(shard, batches, order):
    spec = PhotometricDistortions()
    off, on, again, other = (batches(shard, 1, None), batches(shard, 1, spec), batches(shard, 1, spec),
                             batches(shard, 2, spec))
    assert len(off) == len(on) > 1
    for a, b, c, d in zip(off, on, again, other):
        assert "photometric" not in a
        assert torch.equal(a["crop_boxes"], b["crop_boxes"]) and torch.equal(a[order], b[order])
        p = b["photometric"]
        assert p.dtype == torch.float32 and tuple(p.shape) == (4, 4)
        assert torch.equal(p, c["photometric"]) and not torch.equal(p, d["photometric"])
    assert not torch.equal(on[0]["photometric"], on[1]["photometric"])


def test_decode_on_device_applies_and_drops_the_key(shard):
    ld = S.ShardBatchLoader(shard, 4, 3, 0.9, seed=5, pin=False, threads=2, photometric=PhotometricDistortions())
    batch = next(iter(ld))
    obs = batch["train_observation"]
    plain = dict(batch, train_observation={k: v for k, v in obs.items() if k != "photometric"})
    want = S.decode_on_device(plain, 32, 44)["train_observation"]["image"]
    again = S.decode_on_device(plain, 32, 44)["train_observation"]["image"]
    assert torch.equal(want, again)                                           # without the key: today's output
    got = S.decode_on_device(batch, 32, 44)["train_observation"]
    assert "photometric" not in got and got["image"].dtype == torch.uint8
    assert torch.equal(got["image"], P.photometric_u8_(want.clone(), obs["photometric"], 3))
    assert not torch.equal(got["image"], want)


def test_decode_resident_applies_and_drops_the_key(shard):
    res = R.ResidentShard(shard, "cpu")
    plan = next(iter(R.ResidentBatchLoader(res, 4, 3, 0.9, seed=5, pin=False, photometric=PhotometricDistortions())))
    plain = {k: v for k, v in plan.items() if k != "photometric"}
    want = R.decode_resident(res, plain, 32, 44)
    got = R.decode_resident(res, plan, 32, 44)
    assert set(got["train_observation"]) == set(want["train_observation"])
    assert torch.equal(got["train_observation"]["image"],
                       P.photometric_u8_(want["train_observation"]["image"].clone(), plan["photometric"], 3))
    assert torch.equal(got["action_label"]["action"], want["action_label"]["action"])
    # without the key the decode equals the host-gather decode of the same windows, as before
    assert not torch.equal(got["train_observation"]["image"], want["train_observation"]["image"])


# ---- command line

def test_parser_refusals():
    import distribute_train as dt
    p = dt.build_parser()
    ok = p.parse_args(["--photometric", "--photometric_brightness", "0.2", "--photometric_saturation", "0.5", "1.5",
                       "--photometric_hue", "0.1", "--photometric_contrast", "0.7", "1.3"])
    dt.check_args(p, ok)
    spec = dt.photometric_spec(ok)
    assert (spec.brightness_max_delta, spec.saturation_lower, spec.saturation_upper, spec.hue_max_delta,
            spec.contrast_lower, spec.contrast_upper) == (0.2, 0.5, 1.5, 0.1, 0.7, 1.3)
    assert dt.photometric_spec(p.parse_args(["--photometric"])) == PhotometricDistortions()
    assert dt.photometric_spec(p.parse_args([])) is None
    for argv in (["--photometric", "--synthetic"], ["--photometric", "--data_format", "npz"],
                 ["--photometric", "--photometric_hue", "0.7"], ["--photometric", "--photometric_brightness", "-1"],
                 ["--photometric", "--photometric_saturation", "1.2", "0.8"],
                 ["--photometric", "--photometric_contrast", "-0.1", "1"], ["--photometric_hue", "0.01"]):
        with pytest.raises(SystemExit):
            dt.check_args(p, p.parse_args(argv))


def test_npz_dataset_refused_with_the_shard_format_named(tmp_path, capsys):
    """.npz episodes decode on CPU workers: --photometric names the packed-shard tool instead of training without it."""
    import distribute_train as dt
    root = tmp_path / "ds"
    for split in ("train", "test", "val"):
        E.make_fake_episodes(str(root / split), 2, steps=3, height=32, width=40, seed=1)
    with pytest.raises(SystemExit, match="pack_shards"):
        dt.main(["--device", "cpu", "--dataset_dir", str(root), "--photometric", "--height", "32", "--width", "32",
                 "--seq_len", "2", "--num_layers", "1", "--batch_size", "2", "--num_workers", "0", "--train_episode",
                 "2", "--test_episode", "2", "--eval_episode", "2"])


@pytest.mark.parametrize("residency", ["hbm", "host"])
def test_distribute_train_photometric_cpu(shard, tmp_path, capsys, residency):
    """The training entrypoint with --photometric on a packed shard, on both input paths (CPU, tiny model)."""
    import distribute_train as dt
    root = tmp_path / "ds"
    root.mkdir()
    for split in ("train", "test", "val"):
        os.symlink(shard, root / split)
    rc = dt.main(["--device", "cpu", "--mode", "train", "--dataset_dir", str(root), "--height", "64", "--width", "64",
                  "--seq_len", "2", "--num_layers", "2", "--batch_size", "2", "--max_epochs", "1",
                  "--limit_train_batches", "2", "--limit_val_batches", "1", "--dtype", "fp32", "--num_workers", "2",
                  "--data_residency", residency, "--photometric", "--photometric_hue", "0.05", "--log_dir",
                  str(tmp_path / "logs"), "--ckpt_dir", str(tmp_path / "ck"), "--log_every_n_steps", "1"])
    assert rc == 0
    out = capsys.readouterr().out
    assert "[train] photometric brightness +-0.1, saturation [0.8, 1.2], hue +-0.05 turns, contrast [0.8, 1.2]" in out
