"""Every route of the squeeze-excitation kernels (csrc/kernels/se.hip) against the element-wise fp64 oracle of
tests/se_oracle.py: the 16- and 32-frame se_rowmat tiles one frame either side of their switch, K tails and K splits of
se_rowdot from the `chunks` clamp down to one slice, frame and unit tails, the frame slices of se_wsum_part, the
grid-stride loop of se_wsum_fin, S in (96, 128] where se_rowmat asks for more than 64 KB of LDS, and the three
fallback kernels on both column layouts.  Each case asserts the route it means to walk against the extension's own
plan (se_plan) and the plan re-derived in se_oracle.plan, repeats bitwise, and holds rb of se_bwd to rb of
se_bwd_frame bitwise; the cases marked `scaled` run the backward again with red * 2^-12 and require every output to be
the first run's times 2^-12, bit for bit.  Run with -s for one line per case and one summary per entry point
(profiles/se_stem_tl_oracle_gpu.log)."""
import pytest
import torch

import gemm_oracle as gm
import se_oracle as so

pytestmark = pytest.mark.gpu

DEV = "cuda"
TABLES = {}
SCALE = 2.0 ** -12


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


def se_case(ext, N, C, S, HW, expect=(), scaled=False, red_scale=1.0):
    g = gen(N, C, S, HW)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    pool_sum = r(N, C) * HW * 0.3 + HW * 0.1
    w1, b1 = r(S, C) * C ** -0.5, r(S) * 0.1
    w2, b2 = r(C, S) * S ** -0.5, r(C) * 0.1
    red = r(5, N, C) * red_scale
    inv_hw, count = 1.0 / HW, float(N * HW)
    p = so.plan(N, C, S)
    assert list(ext.se_plan(N, C, S)) == p["as_list"], (list(ext.se_plan(N, C, S)), p["as_list"])
    for k, v in dict(expect).items():
        assert p[k] == v, f"N{N} C{C} S{S}: the case is meant for {k} = {v}, the plan has {p[k]}"
    name = (f"N{N} C{C} S{S} ks{p['slices']} ft{p['ft_fwd']}/{p['ft_bwd']} fs{p['fslices']}x{p['nslice']} "
            f"fin{p['fin_grid']}x{p['fin_trips']} lds{max(p['lds_fwd'], p['lds_bwd'])}")

    pool, h, gate = ext.se_fwd(pool_sum, inv_hw, w1, b1, w2, b2)
    assert pool.data_ptr() == pool_sum.data_ptr()
    _, h2, gate2 = ext.se_fwd(pool_sum, inv_hw, w1, b1, w2, b2)
    assert torch.equal(h, h2) and torch.equal(gate, gate2), f"{name}: se_fwd does not repeat bitwise"
    table("se_fwd").add(name, so.check_fwd(pool, inv_hw, w1, b1, w2, b2, h, gate, "se_fwd " + name))

    def bwd(rd):
        outs = dict(zip(so.BWD_NAMES, ext.se_bwd(rd, gate, h, pool, inv_hw, w1, w2, count)))
        outs["dh"], rb = ext.se_bwd_frame(rd[0], gate, h, inv_hw, w1, w2)
        assert torch.equal(rb, outs["rb"]), f"{name}: rb of se_bwd is not rb of se_bwd_frame"
        return outs

    o, again = bwd(red), bwd(red)
    for k in o:
        assert torch.equal(o[k], again[k]), f"{name}: {k} does not repeat bitwise"
    table("se_bwd_frame").add(name, so.check_frame(red[0], gate, h, w1, w2, inv_hw, o["dh"], o["rb"],
                                                   "se_bwd_frame " + name))
    table("se_bwd_wsum").add(name, so.check_wsum(red, gate, h, o["dh"], pool, o["rb"], inv_hw, count, o,
                                                 "se_bwd_wsum " + name))
    if scaled:
        # dz, dh, rb and the weight sums are linear in red[0]; sdz = sum gate red[1] + rb red[2] (sdzx: red[3], red[4])
        # is linear in (red[0], red[1], red[3]) together.  A power of two scales every product, fma and fp64 sum
        # exactly while nothing underflows (|red| ~ 1: the smallest products here are ~1e-20)
        rs = red.clone()
        rs[[0, 1, 3]] *= SCALE
        s = bwd(rs)
        for k in o:
            assert torch.equal(s[k], o[k] * SCALE), f"{name}: {k} of red * 2^-12 is not 2^-12 x {k} of red"
    return o


FT_FWD = [(352, 16, 198), (353, 32, 216)]
FT_BWD = [(512, 16), (513, 32)]


@pytest.mark.parametrize("N,ft,tiles", FT_FWD)
def test_rowmat_forward_tile_switch(ext, N, ft, tiles):
    """C = 2304 is 18 channel tiles: 11 x 18 = 198 32-frame tiles stay on 16 frames, 12 x 18 = 216 switch."""
    assert (N + 31) // 32 * 18 == tiles
    se_case(ext, N, 2304, 96, 100, {"ft_fwd": ft, "ft_bwd": 16, "fin_trips": 2, "raise_lds": 0}, scaled=True)


@pytest.mark.parametrize("N,ft", FT_BWD)
def test_rowmat_backward_tile_switch(ext, N, ft):
    """N = 513: also nslice = 65 of se_wsum_part (three 32-frame chunks, the last of one frame) and the grid-stride
    loop of se_wsum_fin."""
    exp = {"ft_fwd": 32, "ft_bwd": ft, "fin_grid": 1024, "fin_trips": 2}
    if N == 513:
        exp.update(nslice=65, fslices=8)
    se_case(ext, N, 2304, 96, 100, exp, scaled=True, red_scale=1e-4 if N == 512 else 1.0)


# (N, C, S, HW, expected plan entries): frame tails N in {1, 5, 15, 16, 17, 31, 33, 37}, unit tails S in {1, 5, 6, 10, 31,
# 32, 33, 34, 58, 96}, K tails C in {24, 40, 144, 816, 1392} and none at 64 / 128
TAILS = [
    (1, 24, 1, 9, {"slices": 1, "k_tail": True, "nslice": 1, "fslices": 1, "fin_grid": 1, "fin_trips": 1}),
    (5, 24, 6, 9, {"slices": 1, "nslice": 1, "fslices": 5}),
    (15, 40, 10, 22500, {"slices": 1, "k_tail": True}),
    (16, 144, 6, 5625, {"slices": 3, "k_tail": True}),                 # the `chunks` clamp: 512 wanted, 3 chunks
    (17, 64, 5, 100, {"slices": 1, "k_tail": False}),
    (31, 128, 31, 100, {"slices": 2, "k_tail": False}),
    (33, 40, 33, 100, {"slices": 1}),
    (64, 128, 32, 361, {"slices": 2, "k_tail": False}),
    (33, 816, 34, 361, {"slices": 13, "k_tail": True}),
    (37, 816, 34, 361, {"slices": 13}),
    (37, 1392, 58, 100, {"slices": 22, "k_tail": True}),
    (768, 1392, 58, 100, {"slices": 11, "ft_fwd": 32, "ft_bwd": 16}),  # the model's block 19-24 shape
    (5473, 144, 96, 9, {"slices": 1, "k_tail": True}),                 # enough frame x unit tiles: no K split
    (9, 2304, 96, 100, {"nslice": 2, "fslices": 5, "fin_trips": 2}),    # 8 slices asked for, 5 run
]


@pytest.mark.parametrize("N,C,S,HW,exp", TAILS, ids=[f"N{c[0]}-C{c[1]}-S{c[2]}" for c in TAILS])
def test_tails_and_splits(ext, N, C, S, HW, exp):
    se_case(ext, N, C, S, HW, exp, scaled=N in (5, 33, 37, 9), red_scale=1e-4 if N in (15, 16, 768) else 1.0)


WIDE_S = [(16, 128, 97, {"raise_lds": 0}), (16, 128, 112, {"raise_lds": 0}), (16, 128, 114, {"raise_lds": 1}),
          (16, 128, 128, {"raise_lds": 1, "lds_fwd": 74240}),
          (353, 2304, 102, {"raise_lds": 1, "ft_fwd": 32, "ft_bwd": 16}),
          (513, 2304, 128, {"raise_lds": 1, "ft_fwd": 32, "ft_bwd": 32, "lds_fwd": 82432, "lds_bwd": 81920})]


@pytest.mark.parametrize("N,C,S,exp", WIDE_S, ids=[f"N{c[0]}-C{c[1]}-S{c[2]}" for c in WIDE_S])
def test_units_above_96(ext, N, C, S, exp):
    """S in (96, 128]: se_rowmat's dynamic LDS passes 64 KB from S = 102 (32-frame forward tiles) / 114 (16-frame
    ones); the launch raises the kernel's limit first."""
    se_case(ext, N, C, S, 100, exp, scaled=S == 128)


def test_units_above_128_are_refused(ext):
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(RuntimeError, match="S <= 128"):
        ext.se_fwd(z(16, 128), 1.0, z(129, 128), z(129), z(128, 129), z(128))
    with pytest.raises(RuntimeError, match="S <= 128"):
        ext.se_bwd(z(5, 16, 128), z(16, 128), z(16, 129), z(16, 128), 1.0, z(129, 128), z(128, 129), 16.0)
    with pytest.raises(RuntimeError, match="S <= 128"):
        ext.se_bwd_frame(z(16, 128), z(16, 128), z(16, 129), 1.0, z(129, 128), z(128, 129))
    with pytest.raises(RuntimeError):
        ext.se_plan(16, 128, 129)


@pytest.mark.parametrize("N,C", [(1, 40), (63, 40), (64, 24), (65, 144), (65, 4100)])
def test_fallback_kernels(ext, N, C):
    """se_bwd_dz / se_bwd_dh / se_bwd_bnsum: 16 columns x 64 frame groups up to SE_NARROW_MAX channels (N one short of,
    at and past the 64 groups), 64 columns x 16 groups above it (C = 4100: a 4-column tail)."""
    assert (C > so.SE_NARROW_MAX) == (C == 4100)
    g = gen(N, C, 7)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    gate, dsum, red, rbraw, hh = torch.sigmoid(r(N, C)), r(N, C) * 1e-4, r(5, N, C) * 1e-4, r(N, C), r(N, C) * 2
    inv_hw, count = 1.0 / 361, float(N * 361)
    name = f"N{N} C{C} {'64' if C > so.SE_NARROW_MAX else '16'}-column"
    dz, db = ext.se_bwd_dz(dsum, gate)
    st = so.check_fallback_dz(dsum, gate, dz, db, "se_bwd_dz " + name)
    dh, db1 = ext.se_bwd_dh(dsum, hh)
    st = so.do.merge(st, so.check_fallback_dh(dsum, hh, dh, db1, "se_bwd_dh " + name))
    outs = ext.se_bwd_bnsum(red, gate, rbraw, inv_hw, count)
    st = so.do.merge(st, so.check_fallback_bnsum(red, gate, rbraw, inv_hw, count, *outs, "se_bwd_bnsum " + name))
    table("se_fallback").add(name, st)
    again = list(ext.se_bwd_dz(dsum, gate)) + list(ext.se_bwd_dh(dsum, hh)) + list(ext.se_bwd_bnsum(red, gate, rbraw,
                                                                                                     inv_hw, count))
    assert all(torch.equal(a, b) for a, b in zip(again, [dz, db, dh, db1, *outs])), f"{name}: does not repeat bitwise"
    s = list(ext.se_bwd_dz(dsum * SCALE, gate)) + list(ext.se_bwd_dh(dsum * SCALE, hh))
    assert all(torch.equal(a, b * SCALE) for a, b in zip(s, [dz, db, dh, db1])), f"{name}: not linear in dsum bitwise"
