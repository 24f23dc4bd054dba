"""Depthwise launch plans (csrc/kernels/dw/dw_plan.h) against the recorded decisions of the code before the plan
existed: every grid helper and rt1_dw_tile_info over the host-check sweep, the shapes of test_dw_oracle_gpu.py and the
26 depthwise layers of the backbone, printed by the stand-alone host-check program (``--dw-plans``, built with
ASan + UBSan on the host side, nothing preloaded) and compared line by line with tests/fixtures/dw_plans.txt.  The
fixture was produced at the commit before the refactor and is never regenerated from the code under test.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "fixtures", "dw_plans.txt")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not available")
def test_dw_plans_match_recorded_decisions():
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "host_asan", "build_and_run.sh"), "--dw-plans"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    got = r.stdout.splitlines()
    with open(FIXTURE) as f:
        want = f.read().splitlines()
    assert len(want) > 700
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"first differing case, line {i + 1}:\n  recorded: {w}\n  now:      {g}"
    assert len(got) == len(want), f"{len(got)} cases printed, {len(want)} recorded"
