"""The stem oracle can fail (CPU).  stem.hip's arithmetic is emulated in fp32 torch (the exact bf16 operands, fp32 sums of
27 products, one bf16 store, per-workgroup partial rows of the stored values, per-workgroup weight-gradient partials);
the clean emulation passes every check of tests/stem_oracle.py and every planted fault is caught.  For each fault OLD
records whether tests/test_backbone_gpu.py::test_stem_with_shift (relative Frobenius error < 1e-2 of out and of dW)
would have seen it on the same data, and the test asserts that record.  (On frames this small a whole wrong column or
tile is more than 1 % of the norm, so the old assertion sees it; the 1 / 256 scale and the dead pixels in the partial
rows it cannot see at any size: the first is 0.4 % everywhere, the second is not in anything it compares.)"""
import pytest
import torch
import torch.nn.functional as F

import glue_oracle as go
import stem_oracle as sto

BF = torch.bfloat16
OLD = 1e-2


def gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31)
    return torch.Generator(device="cpu").manual_seed(seed)


def data(N, H, W, u8=True):
    g = gen(N, H, W, u8)
    img = torch.randint(0, 256, (N, 3, H, W), generator=g, dtype=torch.uint8)
    Ho, Wo = sto.out_hw(H, W)
    return {"img": img if u8 else img.float() / 255.0, "w": torch.randn(40, 27, generator=g) * 0.3,
            "dy": torch.randn(N, Ho, Wo, 40, generator=g).to(BF)}


def test_multiply_and_divide_stage_the_same_bf16():
    """bf16(fp32(v) * fp32(1 / 255)) == bf16(fp32(v) / 255) for all 256 bytes: the uint8 and the float route of the same
    frames stage identical operands."""
    v = torch.arange(256, dtype=torch.float32)
    assert torch.equal(sto.table(), (v / 255.0).to(BF).double())
    assert sto.table()[255].item() == 1.0 and sto.table()[0].item() == 0.0


def emu(d, shift, mb, fault=None):
    img, w = d["img"], d["w"]
    N, _, H, W = img.shape
    Ho, Wo = sto.out_hw(H, W)
    dy, dx = (0, 0) if shift is None else shift
    if fault == "dy_sign":
        p = sto.operand(img, (-dy, dx))
    elif fault == "scale_256":
        p = sto.shifted((img.float() * (1.0 / 256.0)).to(BF).double(), shift)
    elif fault == "hi_dword":                      # the dword past the row end is loaded: the next row's first bytes
        flat = torch.cat([img.reshape(-1), torch.zeros(8, dtype=torch.uint8)])
        base = torch.arange(img.numel()).view_as(img)
        x = torch.arange(W).expand_as(img)
        src = flat[(base + dx).clamp(0, flat.numel() - 1)]
        ok = (x + dx >= 0) & (x + dx < W + 4)
        p = sto.table()[torch.where(ok, src, torch.zeros_like(src)).long()]
        p = sto.shifted(p, (dy, 0))
    else:
        p = sto.operand(img, shift)
    if fault == "left_col":                        # the first window column under dx < 0 takes its neighbour's pixel
        assert dx < 0
        p[..., -dx] = p[..., -dx + 1]
    pp = F.pad(p, (1, 1, 1, 1))
    if fault == "odd_w_pad":                       # the column past the frame is not zeroed
        assert W % 2 == 1
        pp[..., W + 1] = pp[..., W]
    P = F.unfold(pp, 3, stride=2).transpose(1, 2).reshape(-1, 27).float()
    wq = w.to(BF).float()
    out = (P @ wq.t()).to(BF)
    g = sto.grid(N, H, W, mb)
    owner = sto.tile_index(N, H, W, g)
    if fault == "tile_skipped":                    # the last tile of workgroup 0 is never visited
        th, tw = sto.tiles_hw(H, W)
        n = torch.arange(N)[:, None, None]
        t = ((n * th + torch.arange(Ho)[None, :, None] // sto.TOH) * tw + torch.arange(Wo)[None, None, :] // sto.TOW)
        last = max(k for k in range(N * th * tw) if k % g == 0)
        out[t.reshape(-1) == last] = 0
    o32 = out.float()
    ps = torch.zeros(g, 40).index_add_(0, owner, o32)
    pq = torch.zeros(g, 40).index_add_(0, owner, o32 * o32)
    if fault == "dead_pixels_pq":                  # the tile row below the map is summed too (even H: it sees row H - 1)
        assert H % 2 == 0
        pd = F.pad(p, (1, 1, 1, 3))
        dead = (F.unfold(pd, 3, stride=2).transpose(1, 2).reshape(N, Ho + 1, Wo, 27)[:, Ho].reshape(-1, 27).float()
                @ wq.t()).to(BF).float()
        ps[0] += dead.sum(0)
        pq[0] += (dead * dead).sum(0)
    dyf = d["dy"].reshape(-1, 40).float()
    dw = torch.zeros(40, 27)
    for k in range(g):
        dw = dw + dyf[owner == k].t() @ P[owner == k]
    return (out.view(N, Ho, Wo, 40), ps, pq), dw


def run_checks(d, shift, mb, outs, dw, name):
    st, P = sto.check_fwd(d["img"], shift, d["w"], mb, outs, name)
    N, _, H, W = d["img"].shape
    return st, sto.check_wgrad(dw, d["dy"], P, sto.grid(N, H, W, mb) + 4, name)


def old_sees(d, shift, outs, dw):
    ref, _, P = sto.ref_fwd(d["img"], shift, d["w"])
    rdw = d["dy"].reshape(-1, 40).double().t() @ P
    return go.frob(outs[0].reshape(-1, 40), ref) > OLD or go.frob(dw, rdw) > OLD


CLEAN = [(1, 1, 1, None, 64, True), (3, 23, 63, (-1, 1), 2, True), (3, 50, 132, (-7, 13), 3, True),
         (1, 24, 64, (0, 64), 64, True), (3, 25, 65, (3, -3), 1, False), (1, 2, 4, (-3, 3), 64, False),
         (1, 24, 64, (-24, 0), 64, False)]


@pytest.mark.parametrize("N,H,W,shift,mb,u8", CLEAN)
def test_clean_emulation_passes(N, H, W, shift, mb, u8):
    d = data(N, H, W, u8)
    outs, dw = emu(d, shift, mb)
    st, sw = run_checks(d, shift, mb, outs, dw, f"clean N{N} H{H} W{W} {shift}")
    assert st["worst"] <= 1.0 and sw["worst"] <= 1.0
    assert not old_sees(d, shift, outs, dw)
    if shift is not None and (abs(shift[0]) >= H or abs(shift[1]) >= W):
        assert not outs[0].any()


# fault -> ((N, H, W, shift, max_blocks), seen by the old rel_err < 1e-2 on this data?)
FAULTS = {"left_col": ((3, 24, 68, (-2, -3), 64), True), "odd_w_pad": ((3, 23, 65, (-2, -3), 64), True),
          "dy_sign": ((3, 24, 68, (-2, 3), 64), True), "scale_256": ((3, 24, 68, (-2, 3), 64), False),
          "tile_skipped": ((3, 50, 132, (-2, 3), 2), True), "dead_pixels_pq": ((3, 24, 68, (-2, 3), 2), False),
          "hi_dword": ((3, 24, 68, (-2, 3), 64), True)}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_fault_is_caught(fault):
    (N, H, W, shift, mb), OLDSEES = FAULTS[fault]
    d = data(N, H, W)
    outs, dw = emu(d, shift, mb, fault)
    with pytest.raises(AssertionError):
        run_checks(d, shift, mb, outs, dw, fault)
    assert old_sees(d, shift, outs, dw) == OLDSEES, \
        f"{fault}: the old assertion {'misses' if OLDSEES else 'sees'} it on this data"


def test_exact_integers_have_no_room():
    """Small-integer frames, weights and dy on the float route: out and dW are exact integers, so the emulation equals
    the reference exactly and one doubled pixel is an error of at least 1."""
    g = gen(7)
    N, H, W = 2, 25, 66
    img = torch.randint(0, 4, (N, 3, H, W), generator=g).float()
    w = torch.randint(-2, 3, (40, 27), generator=g).float()
    Ho, Wo = sto.out_hw(H, W)
    d = {"img": img, "w": w, "dy": torch.randint(-2, 3, (N, Ho, Wo, 40), generator=g).float().to(BF)}
    outs, dw = emu(d, (1, -2), 3)
    ref, _, P = sto.ref_fwd(img, (1, -2), w)
    assert torch.equal(outs[0].reshape(-1, 40).double(), ref)
    assert torch.equal(dw.double(), d["dy"].reshape(-1, 40).double().t() @ P)
