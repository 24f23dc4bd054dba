"""stem_fwd and stem_bwd_weight (csrc/kernels/stem.hip) against the element-wise fp64 oracle of tests/stem_oracle.py on
every staging route: float, uint8 byte by byte (a base that is not 4-byte aligned, or W % 4 != 0), uint8 by aligned
dword pairs with the funnel shift and the software-pipelined win_load / win_store (W % 4 == 0 on an aligned base).
Heights Ho in {1, 11, 12, 13, 25} from odd and even H around the 12-row tile, widths around the 32-column tile and
down to one pixel, shifts that put both frame edges into the window at every funnel amount 0-3 and past the whole
frame, grid caps 1 / 2 / 3 / 64 with even and uneven tile counts per workgroup, N in {1, 3}.  Every element of out,
every partial row of ps / pq (the STORED values of the tiles the workgroup owns, dead pixels excluded) and dW are
checked; every route repeats bitwise, the routes agree bitwise with each other (the operands are identical), and the
kernels agree bitwise with themselves on the pre-shifted frames with no shift.  Run with -s for one line per case and
one summary per entry point (profiles/se_stem_tl_oracle_gpu.log)."""
import pytest
import torch

import gemm_oracle as gm
import stem_oracle as sto

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DEV = "cuda"
TABLES = {}


@pytest.fixture(scope="module")
def ext():
    from pytorch_rt1_for_distributed_training_amd import ops
    yield ops.load()
    for t in TABLES.values():
        t.summary()
    print()


def table(entry):
    return TABLES.setdefault(entry, gm.Table(entry))


def gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31)
    return torch.Generator(device="cpu").manual_seed(seed)


def misaligned(img):
    raw = torch.empty(img.numel() + 1, device=img.device, dtype=torch.uint8)
    mis = raw[1:].view(img.shape)
    mis.copy_(img)
    assert mis.data_ptr() % 4 != 0 and img.data_ptr() % 4 == 0
    return mis


def dev_shift(shift):
    return None if shift is None else torch.tensor(list(shift), dtype=torch.int32, device=DEV)


def run(ext, img, shift, w, dy, mb):
    sh = dev_shift(shift)
    outs = ext.stem_fwd(img, sh, w, mb)
    dw = ext.stem_bwd_weight(img, sh, dy, mb)
    again = ext.stem_fwd(img, sh, w, mb)
    assert all(torch.equal(a, b) for a, b in zip(outs, again)) and torch.equal(dw, ext.stem_bwd_weight(img, sh, dy, mb)), \
        "does not repeat bitwise"
    return outs, dw


# (N, H, W, shift, max_blocks): Ho = (H - 1) / 2 + 1 in {1, 11, 12, 13, 25}; the first block has W % 4 == 0 (all three
# routes), the second runs byte by byte and as float only
CASES = [
    (3, 50, 132, (-7, 13), 3),      # Ho 25, Wo 66: 27 tiles, 9 per workgroup
    (1, 50, 132, (-4, -5), 2),      # 9 tiles: 5 and 4 per workgroup (the last prefetch of one is skipped)
    (3, 25, 132, (4, 5), 2),        # Ho 13
    (1, 49, 128, (1, 1), 64),       # Ho 25, Wo 64
    (3, 50, 64, (3, -3), 1),        # Wo 32: 9 tiles, all one workgroup's
    (3, 25, 68, (-1, -1), 2),       # Wo 34
    (3, 24, 68, (0, 0), 64),        # Ho 12
    (1, 22, 128, (-3, 3), 3),       # Ho 11
    (3, 21, 4, None, 64),           # Wo 2
    (1, 2, 4, (1, -1), 64),         # Ho 1
    (3, 23, 64, (-1, 1), 3),
    (1, 24, 64, (0, 64), 64),       # |dx| >= W: exact zeros
    (1, 24, 64, (-24, 0), 64),      # |dy| >= H: exact zeros
    (1, 24, 68, (5, -70), 2),
    (3, 49, 65, (1, -1), 3),        # odd W: the last tap column is outside the frame
    (1, 1, 1, (0, 0), 64),
    (3, 23, 63, (-3, 3), 2),
    (1, 26, 66, (3, -3), 64),
    (3, 22, 2, (-4, -1), 1),
    (3, 26, 1, (4, 0), 64),
    (1, 25, 63, (-7, 13), 64),
]


@pytest.mark.parametrize("N,H,W,shift,mb", CASES, ids=[f"N{c[0]}-H{c[1]}-W{c[2]}-{c[3]}-mb{c[4]}" for c in CASES])
def test_stem_every_route(ext, N, H, W, shift, mb):
    g = gen(N, H, W, mb)
    img = torch.randint(0, 256, (N, 3, H, W), generator=g, dtype=torch.uint8).to(DEV)
    w = (torch.randn(40, 27, generator=g) * 0.3).to(DEV)
    Ho, Wo = sto.out_hw(H, W)
    dy = torch.randn(N, Ho, Wo, 40, generator=g).to(BF).to(DEV)
    grid = sto.grid(N, H, W, mb)
    routes = {"float": img.float() / 255.0, "bytes": misaligned(img) if W % 4 == 0 else img}
    if W % 4 == 0:
        routes["vec"] = img
    first = None
    for r, im in routes.items():
        assert sto.route(im, W) == r, (r, sto.route(im, W))
        name = f"N{N} H{H} W{W} shift {shift} grid {grid} {r}"
        outs, dw = run(ext, im, shift, w, dy, mb)
        st, P = sto.check_fwd(im, shift, w, mb, outs, "stem_fwd " + name)
        table("stem_fwd").add(name, st)
        table("stem_wgrad").add(name, sto.check_wgrad(dw, dy, P, grid + 4, "stem_bwd_weight " + name))
        if shift is not None and (abs(shift[0]) >= H or abs(shift[1]) >= W):
            assert not outs[0].any() and not dw.any(), f"{name}: a frame shifted out entirely must give exact zeros"
        # the same kernels on the pre-shifted frames: identical operands, fixed summation order
        pre = sto.shifted(im, shift).contiguous()
        if r == "bytes" and W % 4 == 0:
            pre = misaligned(pre)
        o0, d0 = run(ext, pre, None, w, dy, mb)
        assert all(torch.equal(a, b) for a, b in zip(outs, o0)) and torch.equal(dw, d0), \
            f"{name}: the shift read from device memory is not the pre-shifted frame"
        if first is None:
            first = (outs, dw)
        else:
            assert all(torch.equal(a, b) for a, b in zip(outs, first[0])) and torch.equal(dw, first[1]), \
                f"{name}: the staging routes disagree"


@pytest.mark.parametrize("N,H,W,shift,mb", [(3, 25, 66, (1, -2), 3), (1, 50, 132, (-3, 3), 2), (3, 23, 63, None, 64)])
def test_exact_integers_float_route(ext, N, H, W, shift, mb):
    """Frames in {0..3}, weights and dy in {-2..2}: every product and sum is an exact integer (|out| <= 162 fits bf16,
    |dW| < 2^24), so out and dW equal the integer reference exactly; one dropped or doubled pixel cannot hide."""
    g = gen(N, H, W, 5)
    img = torch.randint(0, 4, (N, 3, H, W), generator=g).float().to(DEV)
    w = torch.randint(-2, 3, (40, 27), generator=g).float().to(DEV)
    Ho, Wo = sto.out_hw(H, W)
    dy = torch.randint(-2, 3, (N, Ho, Wo, 40), generator=g).float().to(BF).to(DEV)
    (out, ps, pq), dw = run(ext, img, shift, w, dy, mb)
    ref, _, P = sto.ref_fwd(img, shift, w)
    assert torch.equal(out.reshape(-1, 40).double(), ref)
    assert torch.equal(dw.double(), dy.reshape(-1, 40).double().t() @ P)
    idx = sto.tile_index(N, H, W, sto.grid(N, H, W, mb), DEV)
    rs, _, rq, _ = gm.ref_stats(out.reshape(-1, 40), tile_index=idx, tiles=ps.shape[0])
    assert torch.equal(ps.double(), rs) and torch.equal(pq.double(), rq), "integer partial sums are exact"


@pytest.mark.parametrize("u8,N,H,W,shift,mb", [(True, 3, 25, 132, (-7, 13), 2), (True, 1, 2, 4, (1, -1), 64),
                                               (False, 3, 23, 63, (3, -3), 3), (True, 3, 49, 65, (-1, 1), 1),
                                               (False, 1, 1, 1, None, 64)])
def test_bn_backward_prologue_at_the_edges(ext, u8, N, H, W, shift, mb):
    """The fused BN-backward prologue stays bitwise equal to bn_bwd_apply followed by the plain kernel at the edge
    shapes (bn_bwd_apply itself is under glue_oracle)."""
    g = gen(N, H, W, 9)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    u = lambda *s: torch.rand(*s, generator=g).to(DEV)
    img = torch.randint(0, 256, (N, 3, H, W), generator=g, dtype=torch.uint8).to(DEV)
    img = img if u8 else img.float() / 255.0
    Ho, Wo = sto.out_hw(H, W)
    gg, x = r(N, Ho, Wo, 40).to(BF), r(N, Ho, Wo, 40).to(BF)
    sc, sh, mu, rs, gam = u(40) + 0.5, r(40) * 0.2, r(40) * 0.1, u(40) + 0.5, u(40) + 0.5
    mdz, mdzx = r(40) * 0.05, r(40) * 0.05
    s = dev_shift(shift)
    dy = ext.bn_bwd_apply(gg.view(-1, 40), None, None, 0, x.view(-1, 40), sc, sh, mu, rs, gam, 1, mdz, mdzx)
    ref = ext.stem_bwd_weight(img, s, dy.view(N, Ho, Wo, 40).contiguous(), mb)
    fused = ext.stem_bwd_weight(img, s, gg, mb, x, sc, sh, mu, rs, gam, mdz, mdzx)
    assert torch.equal(fused, ref)
