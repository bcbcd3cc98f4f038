"""k_lk_iter's J - I to float by mantissa bias (lk_jd512, motion_detection_amd/csrc/mdx_plan.h) on a
CPU, no device.

The row body's dot products give x = S + 256 - 512*I on top of the bias word 0x4B400000 that the class
planes' C carries; masking the low 9 bits and subtracting 12582912.f gives 512 * (x >> 9) as a float.
tests/lk_jbias_check.cpp (its own main, mdx_plan.h only, plain g++, -ffp-contract=off) checks through
that function: the identity bit for bit for every x of [-4177919, 4178431] (and the rest of (-2^22,
2^22)), that the range's end points as derived from the weight and tap bounds lie inside (-2^22, 2^22),
and that for the largest and smallest jd and f = +-4080, +-2056, +-1 the products and 400-term running
sums (rounded product then add, and fused) are 512 times the unscaled float computation bit for bit.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("lk_jbias_check") / "lk_jbias_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "motion_detection_amd", "csrc"),
                    os.path.join(ROOT, "tests", "lk_jbias_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    return r.returncode, r.stdout, r.stderr


def test_identity_range_and_scaled_sums(run):
    rc, out, err = run
    assert rc == 0, err
    doc = json.loads(out)
    assert doc["failures"] == 0
    assert (doc["x_min"], doc["x_max"]) == (-4177919, 4178431)
    assert doc["x_checked"] == 4178431 + 4177919 + 1      # every x of the range went through the identity
    assert doc["sums"] == 12                              # 2 ends of jd x 6 values of f
