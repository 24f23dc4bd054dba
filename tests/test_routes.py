"""Block routing (ops/backbone.py plan_block) on the CPU: the extension's capability queries are host functions, so
which kernels each MBConv block runs is checked without a GPU.

The literal tables below were produced at the commit BEFORE plan_block existed, by evaluating that commit's routing
predicates (x_mode_preferred, gram_bn_preferred, project_fused, proj_bwd_fused, pw_bwd_z_preferred, dw_fused_preferred,
z_gemm_preferred, the GEMM_PROJ / GEMM_PROJ_DGRAD tables and the ext.*_supported queries) per block in the order
MBConvFn.forward / backward consulted them -- the non-default sets each in a fresh process under the matching RT1_AB.
They are the record of what the step ran; plan_block must reproduce them.
"""
import dataclasses
import itertools

import pytest

from pytorch_rt1_for_distributed_training_amd.models.efficientnet import block_specs, conv_out_size
from pytorch_rt1_for_distributed_training_amd.ops import _ext, switches
from pytorch_rt1_for_distributed_training_amd.ops.backbone import BlockRoute, RouteFlags, plan_block
from test_backbone_gpu import BLOCKS_NHW, ROUTE_FLAG_SETS

pytestmark = pytest.mark.skipif(not _ext.available(), reason="HIP extension not built (python build.py)")

DEFAULT = RouteFlags.from_switches(switches.DEFAULTS.__getitem__)     # whatever RT1_AB this process runs under
COLUMNS = [f.name for f in dataclasses.fields(BlockRoute)]


def table(text):
    """'blocks  <one value per BlockRoute field>' rows -> the 26 BlockRoutes."""
    out = []
    for first, *vals in (ln.split() for ln in text.strip().splitlines()):
        assert len(vals) == len(COLUMNS), first
        lo, _, hi = first.partition("-")
        assert int(lo) == len(out), first
        out += [BlockRoute(*(int(v) if v.isdigit() else v for v in vals))] * (int(hi or lo) - int(lo) + 1)
    assert len(out) == 26
    return out


# 768 frames, 150x150 into block 0 (the 300x300 bench), block 0 in input-BN mode as the step runs it.  Columns: blocks,
# then bn1 se proj_fwd proj_bwd proj_dgrad dw_bwd dw_variant dw_blocks expand_bwd pw_bwd_blocks residual
STEP_ROUTES = table("""
    0      input_bn  fused  pw_gemm   proj_bwd  pw_gemm_bnbwd  fused  1  2048  none      0     none
    1      none      fused  pw_gemm   proj_bwd  pw_gemm_bnbwd  fused  1  2048  none      0     dw_bwd
    2      xmode     fused  pw_gemm   proj_bwd  pw_gemm_bnbwd  xmode  1  4096  pw_bwd_z  4096  none
    3-4    gemm      fused  pw_gemm   proj_bwd  pw_gemm_bnbwd  fused  1  2048  pw_bwd_z  3072  expand_bwd
    5      gemm      fused  pw_gemm   proj_bwd  pw_gemm_bnbwd  fused  1  512   pw_bwd_z  3072  none
    6-7    gemm      fused  pw_gemm   proj_bwd  pw_gemm_bnbwd  fused  1  1024  pw_bwd_z  512   expand_bwd
    8      gemm      fused  library   stored_a  library        fused  1  512   pw_bwd_z  512   none
    9-12   gram      fused  library   stored_a  library        fused  1  256   z_wide    0     expand_bwd
    13     gram      fused  library   stored_a  library        fused  1  256   z_wide    0     none
    14-17  gram      fused  library   stored_a  library        fused  1  2048  z_wide    0     expand_bwd
    18     gram      fused  gemm_hip  stored_a  gemm_hip       fused  1  2048  z_wide    0     none
    19-23  gram      fused  gemm_hip  stored_a  gemm_hip       fused  1  2048  z_gemm    0     expand_bwd
    24     gram      fused  library   stored_a  library        fused  1  2048  z_gemm    0     none
    25     gemm      fused  library   stored_a  library        fused  1  2048  library   0     add_scaled
""")

# the per-block GPU test's shape (4 frames, 48x64 into block 0, no input-BN) under each of its flag sets
TEST_ROUTES = {
    "default": table("""
    0      none   fused  pw_gemm   proj_bwd  pw_gemm_bnbwd  fused  1  2048  none      0    none
    1      none   fused  pw_gemm   proj_bwd  pw_gemm_bnbwd  fused  1  2048  none      0    dw_bwd
    2      xmode  fused  pw_gemm   proj_bwd  pw_gemm_bnbwd  xmode  1  4096  pw_bwd_z  512  none
    3-4    gemm   fused  pw_gemm   proj_bwd  pw_gemm_bnbwd  fused  1  2048  pw_bwd_z  512  expand_bwd
    5      gemm   fused  pw_gemm   proj_bwd  pw_gemm_bnbwd  fused  1  2048  pw_bwd_z  512  none
    6-7    gemm   fused  pw_gemm   proj_bwd  pw_gemm_bnbwd  fused  1  2048  pw_bwd_z  512  expand_bwd
    8      gemm   fused  library   stored_a  library        fused  1  2048  pw_bwd_z  512  none
    9-12   gram   fused  library   stored_a  library        fused  1  2048  z_wide    0    expand_bwd
    13     gram   fused  library   stored_a  library        fused  1  2048  z_wide    0    none
    14-17  gram   fused  library   stored_a  library        fused  1  2048  z_wide    0    expand_bwd
    18     gram   fused  gemm_hip  stored_a  gemm_hip       fused  1  2048  z_wide    0    none
    19-23  gram   fused  gemm_hip  stored_a  gemm_hip       fused  1  2048  z_gemm    0    expand_bwd
    24     gram   fused  library   stored_a  library        fused  1  2048  z_gemm    0    none
    25     gemm   fused  library   stored_a  library        fused  1  2048  library   0    add_scaled
    """),
    "dw_fused=0": table("""
    0      none  fused  pw_gemm   proj_bwd  pw_gemm_bnbwd  unfused  1  2048  none     0    none
    1      none  fused  pw_gemm   proj_bwd  pw_gemm_bnbwd  unfused  1  2048  none     0    add_scaled
    2      gemm  fused  pw_gemm   proj_bwd  pw_gemm_bnbwd  unfused  1  2048  pw_bwd   512  none
    3-4    gemm  fused  pw_gemm   proj_bwd  pw_gemm_bnbwd  unfused  1  2048  pw_bwd   512  expand_bwd
    5      gemm  fused  pw_gemm   proj_bwd  pw_gemm_bnbwd  unfused  1  2048  pw_bwd   512  none
    6-7    gemm  fused  pw_gemm   proj_bwd  pw_gemm_bnbwd  unfused  1  2048  pw_bwd   512  expand_bwd
    8      gemm  fused  library   stored_a  library        unfused  1  2048  pw_bwd   512  none
    9-12   gram  fused  library   stored_a  library        unfused  1  2048  library  0    add_scaled
    13     gram  fused  library   stored_a  library        unfused  1  2048  library  0    none
    14-17  gram  fused  library   stored_a  library        unfused  1  2048  library  0    add_scaled
    18     gram  fused  gemm_hip  stored_a  gemm_hip       unfused  1  2048  library  0    none
    19-23  gram  fused  gemm_hip  stored_a  gemm_hip       unfused  1  2048  library  0    add_scaled
    24     gram  fused  library   stored_a  library        unfused  1  2048  library  0    none
    25     gemm  fused  library   stored_a  library        unfused  1  2048  library  0    add_scaled
    """),
    "dw_variant=0": table("""
    0      none   fused  pw_gemm   proj_bwd  pw_gemm_bnbwd  fused  0  2048  none      0    none
    1      none   fused  pw_gemm   proj_bwd  pw_gemm_bnbwd  fused  0  2048  none      0    add_scaled
    2      xmode  fused  pw_gemm   proj_bwd  pw_gemm_bnbwd  xmode  0  4096  pw_bwd_z  512  none
    3-4    gemm   fused  pw_gemm   proj_bwd  pw_gemm_bnbwd  fused  0  2048  pw_bwd    512  expand_bwd
    5      gemm   fused  pw_gemm   proj_bwd  pw_gemm_bnbwd  fused  0  2048  pw_bwd_z  512  none
    6-7    gemm   fused  pw_gemm   proj_bwd  pw_gemm_bnbwd  fused  0  2048  pw_bwd    512  expand_bwd
    8      gemm   fused  library   stored_a  library        fused  0  2048  pw_bwd_z  512  none
    9-12   gram   fused  library   stored_a  library        fused  0  2048  library   0    add_scaled
    13     gram   fused  library   stored_a  library        fused  0  2048  library   0    none
    14-17  gram   fused  library   stored_a  library        fused  0  2048  library   0    add_scaled
    18     gram   fused  gemm_hip  stored_a  gemm_hip       fused  0  2048  z_wide    0    none
    19-23  gram   fused  gemm_hip  stored_a  gemm_hip       fused  0  2048  library   0    add_scaled
    24     gram   fused  library   stored_a  library        fused  0  2048  library   0    none
    25     gemm   fused  library   stored_a  library        fused  0  2048  library   0    add_scaled
    """),
    "se_fused=0": table("""
    0      none   library  pw_gemm   proj_bwd  pw_gemm_bnbwd  fused  1  2048  none      0    none
    1      none   library  pw_gemm   proj_bwd  pw_gemm_bnbwd  fused  1  2048  none      0    dw_bwd
    2      xmode  library  pw_gemm   proj_bwd  pw_gemm_bnbwd  xmode  1  4096  pw_bwd_z  512  none
    3-4    gemm   library  pw_gemm   proj_bwd  pw_gemm_bnbwd  fused  1  2048  pw_bwd_z  512  expand_bwd
    5      gemm   library  pw_gemm   proj_bwd  pw_gemm_bnbwd  fused  1  2048  pw_bwd_z  512  none
    6-7    gemm   library  pw_gemm   proj_bwd  pw_gemm_bnbwd  fused  1  2048  pw_bwd_z  512  expand_bwd
    8      gemm   library  library   stored_a  library        fused  1  2048  pw_bwd_z  512  none
    9-12   gram   library  library   stored_a  library        fused  1  2048  z_wide    0    expand_bwd
    13     gram   library  library   stored_a  library        fused  1  2048  z_wide    0    none
    14-17  gram   library  library   stored_a  library        fused  1  2048  z_wide    0    expand_bwd
    18     gram   library  gemm_hip  stored_a  gemm_hip       fused  1  2048  z_wide    0    none
    19-23  gram   library  gemm_hip  stored_a  gemm_hip       fused  1  2048  z_gemm    0    expand_bwd
    24     gram   library  library   stored_a  library        fused  1  2048  z_gemm    0    none
    25     gemm   library  library   stored_a  library        fused  1  2048  library   0    add_scaled
    """),
    "pw_pro=0": table("""
    0      none   fused  library   stored_a  pw_gemm_bnbwd  fused  1  2048  none      0    none
    1      none   fused  library   stored_a  pw_gemm_bnbwd  fused  1  2048  none      0    dw_bwd
    2      xmode  fused  library   stored_a  pw_gemm_bnbwd  xmode  1  4096  pw_bwd_z  512  none
    3-4    gemm   fused  library   stored_a  pw_gemm_bnbwd  fused  1  2048  pw_bwd_z  512  expand_bwd
    5      gemm   fused  library   stored_a  pw_gemm_bnbwd  fused  1  2048  pw_bwd_z  512  none
    6-7    gemm   fused  library   stored_a  pw_gemm_bnbwd  fused  1  2048  pw_bwd_z  512  expand_bwd
    8      gemm   fused  library   stored_a  library        fused  1  2048  pw_bwd_z  512  none
    9-12   gram   fused  library   stored_a  library        fused  1  2048  z_wide    0    expand_bwd
    13     gram   fused  library   stored_a  library        fused  1  2048  z_wide    0    none
    14-17  gram   fused  library   stored_a  library        fused  1  2048  z_wide    0    expand_bwd
    18     gram   fused  gemm_hip  stored_a  gemm_hip       fused  1  2048  z_wide    0    none
    19-23  gram   fused  gemm_hip  stored_a  gemm_hip       fused  1  2048  z_gemm    0    expand_bwd
    24     gram   fused  library   stored_a  library        fused  1  2048  z_gemm    0    none
    25     gemm   fused  library   stored_a  library        fused  1  2048  library   0    add_scaled
    """),
}

CHOICES = {          # every value of every stage, as BlockRoute documents them
    "bn1": {"xmode", "gram", "gemm", "input_bn", "none"},
    "se": {"fused", "library"},
    "proj_fwd": {"pw_gemm", "gemm_hip", "library"},
    "proj_bwd": {"proj_bwd", "stored_a"},
    "proj_dgrad": {"pw_gemm_bnbwd", "gemm_hip", "library"},
    "dw_bwd": {"xmode", "fused", "unfused"},
    "dw_variant": {0, 1},
    "expand_bwd": {"pw_bwd_z", "z_wide", "z_gemm", "pw_bwd", "library", "none"},
    "residual": {"dw_bwd", "expand_bwd", "add_scaled", "none"},
}


def routes(N, H, W, flags, in_bn0=False):
    out = []
    for sp in block_specs():
        out.append(plan_block(sp, N, H, W, in_bn0 and sp.index == 0, flags))
        H, W = conv_out_size(H, sp.kernel, sp.stride), conv_out_size(W, sp.kernel, sp.stride)
    return out


def test_default_routes_of_the_step():
    for i, (got, want) in enumerate(zip(routes(768, 150, 150, DEFAULT, in_bn0=True), STEP_ROUTES, strict=True)):
        assert got == want, i


@pytest.mark.parametrize("flag_set", list(ROUTE_FLAG_SETS))
def test_routes_of_the_gpu_tests_flag_sets(flag_set):
    got = routes(*BLOCKS_NHW, dataclasses.replace(DEFAULT, **ROUTE_FLAG_SETS[flag_set]))
    for i, (g, want) in enumerate(zip(got, TEST_ROUTES[flag_set], strict=True)):
        assert g == want, i


def test_gpu_tests_flag_sets_reach_every_route_value():
    """Over the union of the GPU test's flag sets at its shape, every value of every stage occurs -- except BN1's
    "input_bn", which no flag selects: it is the caller's in_bn argument (block 0 behind StemPreFn), which that test
    does not use and the encoder tests do."""
    assert set(TEST_ROUTES) == set(ROUTE_FLAG_SETS)
    assert set(CHOICES) | {"dw_blocks", "pw_bwd_blocks"} == set(COLUMNS)
    seen = {name: set() for name in CHOICES}
    for over in ROUTE_FLAG_SETS.values():
        for r in routes(*BLOCKS_NHW, dataclasses.replace(DEFAULT, **over)):
            for name in CHOICES:
                seen[name].add(getattr(r, name))
    missing = {name: CHOICES[name] - seen[name] for name in CHOICES if CHOICES[name] - seen[name]}
    assert missing == {"bn1": {"input_bn"}}, missing
    assert routes(*BLOCKS_NHW, DEFAULT, in_bn0=True)[0].bn1 == "input_bn"


# The on/off switches plan_block reads (g256 and gram_sx belong to the leaf dispatchers, the two stem switches to
# encoder_forward).  ALONE each pick the value of one stage that no invariant below mentions (se, gram-or-gemm BN1,
# proj_dgrad) and feed nothing else, so they flip together as one bit; the rest go through all 2^11 combinations.
ON_OFF = ["pw_tall", "dw_fused", "dw_s2_fused", "dw_variant", "dw_res", "pw_pro", "proj_bwd", "pw_bwd_z", "pw_z_wide",
          "gemm_proj", "tall_res"]
ALONE = ["se_fused", "gram_bn", "wgrad_mfma", "gemm_proj_dgrad"]


def test_route_invariants_over_all_flag_combinations():
    """What MBConvFn's forward and backward have to agree on, for every on/off combination of the switches (with each
    value of the two multi-valued ones), on every distinct block shape of the step and of the GPU test."""
    assert set(ON_OFF + ALONE) | {"g256", "gram_sx", "stem_in_block0", "stem_bn_bwd", "z_gemm", "xmode"} == {
        f.name for f in dataclasses.fields(RouteFlags)}
    cases = set()
    for in_bn0, (N, H, W) in ((True, (768, 150, 150)), (False, BLOCKS_NHW)):
        for sp in block_specs():
            cases.add((dataclasses.replace(sp, index=0, drop_rate=0.0), N, H, W, in_bn0 and sp.index == 0))
            H, W = conv_out_size(H, sp.kernel, sp.stride), conv_out_size(W, sp.kernel, sp.stride)
    for zx, alone, bits in itertools.product((("1", "1"), ("0", "all"), ("2", "0")), (False, True),
                                             itertools.product((False, True), repeat=len(ON_OFF))):
        on = {**dict(zip(ON_OFF, bits)), **dict.fromkeys(ALONE, alone)}
        flags = dataclasses.replace(DEFAULT, z_gemm=zx[0], xmode=zx[1], **{**on, "dw_variant": int(on["dw_variant"])})
        for sp, N, H, W, in_bn in cases:
            r = plan_block.__wrapped__(sp, N, H, W, in_bn, flags)
            expand = sp.expand_ratio != 1
            assert (r.expand_bwd != "none") == expand and (r.bn1 in ("xmode", "gram", "gemm")) == expand, (flags, r)
            assert (r.bn1 == "input_bn") == in_bn, (flags, r)
            # a dz-reading expand backward needs a depthwise backward that stores dz; x-mode has no y1 for any other
            if r.zmode:
                assert r.dw_bwd in ("xmode", "fused") and (sp.stride == 2 or r.dw_variant == 1), (flags, r)
            assert (r.bn1 == "xmode") == (r.dw_bwd == "xmode"), (flags, r)
            if r.dw_bwd == "xmode":
                assert r.expand_bwd == "pw_bwd_z", (flags, r)
            assert (r.pw_bwd_blocks > 0) == (r.expand_bwd in ("pw_bwd_z", "pw_bwd")), (flags, r)
            # proj_bwd only behind the prologue GEMM, the one that can skip storing A
            if r.proj_bwd == "proj_bwd":
                assert r.proj_fwd == "pw_gemm", (flags, r)
            # the residual gradient: exactly one agent on a skip block, none elsewhere
            assert (r.residual == "none") == (not sp.has_skip), (flags, r)
            if r.dw_res:
                assert (r.dw_bwd == "fused" and r.dw_variant != 0 and sp.stride == 1 and sp.has_skip
                        and r.bn1 == "none"), (flags, r)
            if r.residual == "expand_bwd":
                assert r.expand_bwd in ("pw_bwd_z", "pw_bwd", "z_wide", "z_gemm"), (flags, r)
