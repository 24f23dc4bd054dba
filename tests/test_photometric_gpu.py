"""The photometric HIP kernel (csrc/kernels/photometric.hip) against the fp64 oracle (tests/photometric_oracle.py):
every listed case, every frame content under every parameter set, on the word path and the byte path.

Tolerance (photometric_oracle.compare): no byte differs by more than 1 and at most ceil(1e-3 * bytes) bytes differ,
per launch.  tests/test_photometric.py holds the CPU side and says how contents and values were chosen.
"""
import functools

import pytest
import torch

import photometric_oracle as O
from pytorch_rt1_for_distributed_training_amd.data import photometric as P

pytestmark = pytest.mark.gpu

CASE_IDS = ["x".join(map(str, c)) for c in O.CASES]
IDENTITY = (0.0, 1.0, 0.0, 1.0)


@functools.lru_cache(maxsize=None)
def _inputs(case, rot, first):
    return O.case_image(case, rot), O.case_params(case, first)


def _gpu(img, prm, T):
    out = img.cuda()
    P.photometric_u8_(out, prm.cuda(), T)
    return out.cpu()


@pytest.mark.parametrize("case", O.CASES, ids=CASE_IDS)
def test_kernel_within_tolerance_of_oracle(case):
    total = differ = 0
    for rot, first in O.case_runs(case):
        img, prm = _inputs(case, rot, first)
        got = _gpu(img, prm, case[1])
        ref = O.oracle_u8(img, prm, case[1])
        mx, cnt, cap = O.compare(got, ref)
        total += img.numel()
        differ += cnt
        assert mx <= 1 and cnt <= cap, (f"case {case} rotation {rot}, window params {prm.tolist()}: max byte "
                                        f"difference {mx} (allowed 1), {cnt} bytes differ (allowed {cap})")
    print(f"case {case}: {differ} of {total} bytes differ from the oracle ({differ / total:.2e})")


@pytest.mark.parametrize("case", O.CASES, ids=CASE_IDS)
def test_identity_is_bitwise_and_runs_repeat(case):
    B, T = case[:2]
    img, prm = _inputs(case, 1, 0)
    assert torch.equal(_gpu(img, torch.tensor([IDENTITY]).repeat(B, 1), T), img)
    assert torch.equal(_gpu(img, prm, T), _gpu(img, prm, T))


@pytest.mark.parametrize("case", O.CASES[:4], ids=CASE_IDS[:4])
def test_frame_alone_equals_frame_in_batch(case):
    """A frame's bytes depend on its own bytes and its window's numbers only: not on the batch, the grid, or the
    alignment its planes happen to have (a misaligned copy takes the byte path)."""
    B, T, H, W = case
    for rot in (0, 3):
        img, prm = _inputs(case, rot, 1)
        batch = _gpu(img, prm, T).view(B * T, 3, H, W)
        flat = img.view(B * T, 3, H, W)
        for n in range(B * T):
            alone = _gpu(flat[n:n + 1].clone(), prm[n // T:n // T + 1], 1)
            assert torch.equal(alone[0], batch[n]), (case, rot, n)
        for off in (1, 2):                                     # tensor base off by 1 or 2 bytes
            buf = torch.zeros(img.numel() + 4, dtype=torch.uint8, device="cuda")
            view = buf[off:off + img.numel()].view(img.shape)
            view.copy_(img)
            assert view.is_contiguous() and view.data_ptr() % 4 == off
            P.photometric_u8_(view, prm.cuda(), T)
            assert torch.equal(view.cpu().view(B * T, 3, H, W), batch), (case, rot, off)
            assert int(buf[:off].sum()) == 0 and int(buf[off + img.numel():].sum()) == 0   # nothing outside the view


@pytest.mark.parametrize("case", O.CASES[:4], ids=CASE_IDS[:4])
def test_gpu_against_cpu_path(case):
    for rot, first in ((0, 0), (2, 3), (4, 7), (5, 9)):
        img, prm = _inputs(case, rot, first)
        d = (_gpu(img, prm, case[1]).int() - P.photometric_u8_reference(img, prm, case[1]).int()).abs()
        assert int(d.max()) <= 1, (case, rot, first, int(d.max()))


def test_decode_resident_with_plan_equals_decode_then_kernel(tmp_path):
    from pytorch_rt1_for_distributed_training_amd.data import episodes as E
    from pytorch_rt1_for_distributed_training_amd.data import resident as R
    from pytorch_rt1_for_distributed_training_amd.data import shards as S
    from pytorch_rt1_for_distributed_training_amd.data.augment import PhotometricDistortions
    ids = E.make_fake_episodes(str(tmp_path / "npz"), 4, steps=5, height=90, width=160, seed=5)
    S.pack_shard(str(tmp_path / "npz"), ids, str(tmp_path / "shard"))
    res = R.ResidentShard(str(tmp_path / "shard"), "cuda")
    plan = next(iter(R.ResidentBatchLoader(res, 4, 3, 0.9, seed=1, photometric=PhotometricDistortions())))
    plan = {k: v.cuda() for k, v in plan.items()}
    got = R.decode_resident(res, plan, 64, 96)["train_observation"]
    plain = R.decode_resident(res, {k: v for k, v in plan.items() if k != "photometric"}, 64, 96)
    want = plain["train_observation"]["image"].clone()
    assert "photometric" not in got and not torch.equal(got["image"], want)
    P.photometric_u8_(want, plan["photometric"], 3)
    assert torch.equal(got["image"], want)
    # the host-gather decode takes the same hook
    raw = res.frames.index_select(0, plan["plan_rows"].reshape(-1)).view(4, 3, 90, 160, 3)
    host = {"train_observation": {"raw_frames": raw, "crop_boxes": plan["crop_boxes"],
                                  "photometric": plan["photometric"]}, "action_label": {}}
    assert torch.equal(S.decode_on_device(host, 64, 96)["train_observation"]["image"], want)


def test_binding_refusals():
    from pytorch_rt1_for_distributed_training_amd.ops import load
    f = load().photometric_u8_
    img = torch.zeros(4, 3, 6, 6, dtype=torch.uint8, device="cuda")
    prm = torch.tensor([IDENTITY], device="cuda").repeat(2, 1)
    f(img, prm, 2)
    f(img.view(2, 2, 3, 6, 6), prm, 2)
    f(img[:0], prm[:0], 2)                                     # empty batch: a no-op
    for bad in (lambda: f(img.float(), prm, 2), lambda: f(img, prm[:1], 2), lambda: f(img, prm[:, :3].contiguous(), 2),
                lambda: f(img, prm, 3), lambda: f(img, prm.double(), 2), lambda: f(img, prm.cpu(), 2),
                lambda: f(img[:, :, :, ::2], prm, 2), lambda: f(img, prm, 0)):
        with pytest.raises(RuntimeError):
            bad()
    assert int(img.sum()) == 0
