"""The SE oracle can fail (CPU).  se.hip's arithmetic is emulated in fp32 torch with the kernels' structure (one partial
per K slice summed in slice order, one partial per frame slice summed in slice order, fp64 column sums, the same
stored intermediates); the clean emulation passes every check of tests/se_oracle.py and every planted fault is caught.
For each fault OLD records whether the assertions of tests/test_backbone_gpu.py::test_se_fused (h rtol = atol = 1e-4,
gate rtol = 1e-4 / atol = 1e-5, every backward output rtol = atol = 2e-4) would have seen it on the same data, and the
test asserts that record.  The backward data is at training scale (|red| ~ 1e-4): of the backward faults only the
missing inv_hw (dw1 361 times too large) is visible to an absolute tolerance of 2e-4 there."""
import pytest
import torch

import se_oracle as so

SHAPES = [(5, 24, 6, 9), (37, 144, 34, 361), (33, 816, 58, 100), (64, 128, 10, 5625), (353, 2304, 96, 100)]
FAULT_SHAPE = (37, 144, 34, 361)      # 3 K slices with a 16-channel tail, 16-frame tiles, 19 frame slices of 2
RED_SCALE = 1e-4


def gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31)
    return torch.Generator(device="cpu").manual_seed(seed)


def data(N, C, S, HW):
    g = gen(N, C, S, HW)
    r = lambda *s: torch.randn(*s, generator=g)
    return {"pool": r(N, C) * HW * 0.3 + HW * 0.1, "inv_hw": 1.0 / HW, "w1": r(S, C) * C ** -0.5, "b1": r(S) * 0.1,
            "w2": r(C, S) * S ** -0.5, "b2": r(C) * 0.1, "red": r(5, N, C) * RED_SCALE, "count": float(N * HW)}


def sig(x):
    return 1.0 / (1.0 + torch.exp(-x))


def emu_fwd(d, fault=None):
    pool, w1, w2 = d["pool"], d["w1"], d["w2"]
    N, C = pool.shape
    S = w1.shape[0]
    p = so.plan(N, C, S)
    ih = torch.tensor(d["inv_hw"], dtype=torch.float32)
    acc = torch.zeros(N, S)
    for k in range(p["slices"]):
        kb, ke = k * p["kslice"], min(C, (k + 1) * p["kslice"])
        if fault == "k_tail" and ke == C:
            ke = (C - 1) // so.RD_KC * so.RD_KC                 # the partly filled last chunk is never staged
        acc = acc + pool[:, kb:ke] @ w1[:, kb:ke].t()
    h = acc * ih + d["b1"]
    stored = h.clone()
    if fault == "h_stale":                                      # the rows of one frame tile are never written
        stored[16:32] = 0.0
    y = h * sig(h)
    if fault == "tile_last_frame":
        y[p["ft_fwd"] - 1] = 0.0
    b2 = d["b2"].roll(1) if fault == "b2_shift" else d["b2"]
    return stored, sig(y @ w2.t() + b2)


def emu_bwd(d, h, gate, fault=None):
    red, pool, w1, w2 = d["red"], d["pool"], d["w1"], d["w2"]
    N, C = pool.shape
    S = w1.shape[0]
    p = so.plan(N, C, S)
    ih = torch.tensor(d["inv_hw"], dtype=torch.float32)
    dz = red[0] * (gate * (1 - gate))
    acc = torch.zeros(N, S)
    for k in range(p["slices"]):
        kb, ke = k * p["kslice"], min(C, (k + 1) * p["kslice"])
        acc = acc + dz[:, kb:ke] @ w2[kb:ke]
    sg = sig(h)
    dh = acc * (sg * (1 + h * (1 - sg)))
    ys = dh.clone()
    if fault == "tile_last_frame":
        ys[p["ft_bwd"] - 1] = 0.0
    rb = (ys @ w1) * ih
    hs = h * sg
    dw2, dw1 = torch.zeros(C, S), torch.zeros(S, C)
    pc, pj = torch.zeros(3, C, dtype=torch.float64), torch.zeros(S, dtype=torch.float64)
    for sl in range(p["fslices"]):
        if fault == "slice_skipped" and sl == 3:
            continue
        f = slice(sl * p["nslice"], min(N, (sl + 1) * p["nslice"]))
        dw2 = dw2 + dz[f].t() @ hs[f]
        part = dh[f].t() @ pool[f]
        if fault == "dw1_lost_frame" and sl == 5:               # one frame's product lost for 16 lanes
            n = f.start
            part[7, 64:80] -= dh[n, 7] * pool[n, 64:80]
        dw1 = dw1 + part
        pc[0] += dz[f].double().sum(0)
        pc[1] += (gate[f] * red[1][f] + rb[f] * red[2][f]).double().sum(0)
        pc[2] += (gate[f] * red[3][f] + rb[f] * red[4][f]).double().sum(0)
        pj += dh[f].double().sum(0)
    out = {"dh": dh, "rb": rb, "dw2": dw2, "dw1": dw1 if fault == "no_inv_hw" else dw1 * ih, "db2": pc[0].float(),
           "db1": pj.float(), "sdz": pc[1].float(), "sdzx": pc[2].float(),
           "mdz": (pc[1] / (N if fault == "mdz_N" else d["count"])).float(), "mdzx": (pc[2] / d["count"]).float()}
    return out


def run_checks(d, h, gate, o, name):
    so.check_fwd(d["pool"], d["inv_hw"], d["w1"], d["b1"], d["w2"], d["b2"], h, gate, name)
    so.check_frame(d["red"][0], gate, h, d["w1"], d["w2"], d["inv_hw"], o["dh"], o["rb"], name)
    return so.check_wsum(d["red"], gate, h, o["dh"], d["pool"], o["rb"], d["inv_hw"], d["count"], o, name)


@pytest.mark.parametrize("N,C,S,HW", SHAPES)
def test_clean_emulation_passes(N, C, S, HW):
    d = data(N, C, S, HW)
    h, gate = emu_fwd(d)
    st = run_checks(d, h, gate, emu_bwd(d, h, gate), f"clean N{N} C{C} S{S}")
    assert st["worst"] <= 1.0, st     # (the cast of an exact fp64 sum, db1, may use all of its half ulp)


def old_sees(d, h, gate, o):
    """Would test_se_fused's assert_close calls fail on these outputs?  Its references, fp64 from the stored h / gate."""
    def far(out, ref, rtol, atol):
        return bool(((out.double() - ref).abs() > atol + rtol * ref.abs()).any())

    if far(h, so.ref_h(d["pool"], d["inv_hw"], d["w1"], d["b1"])[0], 1e-4, 1e-4):
        return True
    hr = so.ref_h(d["pool"], d["inv_hw"], d["w1"], d["b1"])[0]
    gr = torch.sigmoid((hr * torch.sigmoid(hr)) @ d["w2"].double().t() + d["b2"].double())
    if far(gate, gr, 1e-4, 1e-5):
        return True
    dhr = so.ref_dh(d["red"][0], gate, h, d["w2"], 1)[0]
    rbr = so.ref_rb(dhr, d["w1"], d["inv_hw"])[0]
    r = so.ref_wsums(d["red"], gate, h, dhr, d["pool"], rbr, d["inv_hw"], d["count"])
    return far(o["rb"], rbr, 2e-4, 2e-4) or any(far(o[k], r[k][0], 2e-4, 2e-4) for k in r)


# fault -> (forward fault?, seen by the old assertions on this data?)
FAULTS = {"dw1_lost_frame": (False, False), "k_tail": (True, True), "slice_skipped": (False, False),
          "tile_last_frame": (True, True), "no_inv_hw": (False, True), "b2_shift": (True, True),
          "mdz_N": (False, False), "h_stale": (True, True)}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_fault_is_caught(fault):
    fwd, OLD = FAULTS[fault]
    d = data(*FAULT_SHAPE)
    h, gate = emu_fwd(d, fault if fwd else None)
    if fault == "tile_last_frame":
        hc, gc = emu_fwd(d)
        o = emu_bwd(d, hc, gc, fault)                       # the same slip in the backward tile, on clean inputs
        with pytest.raises(AssertionError, match=" rb"):
            run_checks(d, hc, gc, o, fault)
    else:
        o = emu_bwd(d, h, gate, None if fwd else fault)
    with pytest.raises(AssertionError):
        run_checks(d, h, gate, o, fault)
    assert old_sees(d, h, gate, o) == OLD, f"{fault}: the old assertions {'miss' if OLD else 'see'} it on this data"


def test_lost_frame_term_exceeds_its_bound_in_all_16_elements():
    """The historical fault (dw1 = the exact sum minus one frame's term for 16 lanes): each affected element is outside
    its bound, every other element inside."""
    d = data(*FAULT_SHAPE)
    h, gate = emu_fwd(d)
    o = emu_bwd(d, h, gate, "dw1_lost_frame")
    N, C, S, _ = FAULT_SHAPE
    ref, sab = so.ref_wsums(d["red"], gate, h, o["dh"], d["pool"], o["rb"], d["inv_hw"], d["count"])["dw1"]
    bound = so.U32 * ref.abs() + so.slack(N + so.plan(N, C, S)["fslices"] + 1) * sab
    over = (o["dw1"].double() - ref).abs() > bound
    assert int(over.sum()) == 16 and bool(over[7, 64:80].all())


def test_plan_routes_of_the_issue():
    """The switches the GPU file walks, from the re-derived plan."""
    assert (so.plan(352, 2304, 96)["ft_fwd"], so.plan(353, 2304, 96)["ft_fwd"]) == (16, 32)
    assert (so.plan(512, 2304, 96)["ft_bwd"], so.plan(513, 2304, 96)["ft_bwd"]) == (16, 32)
    p = so.plan(9, 2304, 96)
    assert (p["nslice"], p["fslices"]) == (2, 5)
    p = so.plan(513, 2304, 96)
    assert (p["nslice"], p["fslices"], p["fin_grid"]) == (65, 8, 1024) and p["fin_trips"] == 2
    assert so.plan(5, 24, 6)["nslice"] == 1 and so.plan(5, 24, 6)["fin_trips"] == 1
    assert so.plan(5473, 144, 96)["slices"] == 1 and so.plan(16, 1392, 34)["slices"] == 22
    assert so.plan(768, 2304, 96)["lds_fwd"] == 61952 and not so.plan(768, 2304, 96)["raise_lds"]
    assert so.plan(16, 128, 128)["lds_fwd"] == 74240 and so.plan(353, 2304, 128)["lds_fwd"] == 82432
    assert [so.plan(16, 128, s)["raise_lds"] for s in (97, 112, 113, 114, 128)] == [0, 0, 0, 1, 1]
    assert [so.plan(353, 2304, s)["raise_lds"] for s in (96, 101, 102)] == [0, 0, 1]
