"""The host plan of the class-plane LK (motion_detection_amd/csrc/mdx_plan.h) on a CPU, no device.

The plan decides which memory the class-plane kernels may read: group shapes and union starts, the
plane rows [vlo, vhi) of a band, the pyramid rows a band builds, the scratch layout.  tests/plan_check.cpp
(its own main, mdx_plan.h only, plain g++) builds the plans of the configurations below, checks the
invariants of DESIGN.md §5.2 by brute force over every grid point and prints the plans; this file runs it
once and compares what it printed with tests/golden/class_plan_parent.json.

The configurations are the smallest shapes at which each rule is reached: one level (41x41, 72x72), 2x2
classes (100x100 ps 1), narrow and wide frames (164x244, 4864x164), level counts cut by max_level (320x240
with 0 and 7), sizes that are no multiple of the step (330x250, 640x480 ps 7), G 8 / UW 512 with 16x16
classes (1280x720 ps 33), the widest usable step (1920x1080 ps 64), a step no shape fits (ps 70: nch 0),
six levels (3840x2160); each with the group size free, forced to 4 and to 8 and for contexts of 1 and 32
pairs; two with MDX_LK_ASTRIP 1 and 64; 1080p's grid rows cut into 2, 3, 4, 8 and 108 bands; the single
grid row [3, 4) of 320x240.

The golden file was recorded from commit 62e10c4, the parent of the commit that introduced mdx_plan.h:
plan_check.cpp compiled against a stand-in header that wrapped that commit's lines of mdx_pair.cpp,
mdx_internal.h and mdx_ctx.h, unchanged, behind a stub context holding lk_g, lk_astrip and max_batch.  It
is never re-recorded from mdx_plan.h itself.
"""
import hashlib
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "class_plan_parent.json")


def digest(doc):
    """plan_check's document with every plan's table (hex of its int16 values, low byte first) replaced by
    their SHA-256: what the golden file holds."""
    out = {"plans": [], "scratch": doc["scratch"]}
    for p in doc["plans"]:
        q = {k: v for k, v in p.items() if k != "tab"}
        raw = bytes.fromhex(p["tab"])
        q["tab_len"] = len(raw) // 2
        q["tab_sha256"] = hashlib.sha256(raw).hexdigest()
        out["plans"].append(q)
    return out


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("plan_check") / "plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "motion_detection_amd", "csrc"), "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    return r.returncode, digest(json.loads(r.stdout)), r.stderr


def by_cfg(doc):
    return {tuple(p["cfg"]): p for p in doc["plans"]}


def test_invariants_hold(run):
    rc, doc, err = run
    assert rc == 0, err
    usable = [p for p in doc["plans"] if p["nch"]]
    bands = [p for p in usable if p["cfg"][5] >= 0]
    # every plan but 1920x1080 ps 70's six is usable, so all of them went through the checks
    assert len(doc["plans"]) == 243 and len(usable) == 237 and len(bands) == 143 and len(doc["scratch"]) == 120


def test_same_as_parent(run):
    _, doc, _ = run
    with open(GOLDEN) as f:
        gold = json.load(f)
    new, old = by_cfg(doc), by_cfg(gold)
    assert list(new) == list(old)
    for cfg in old:
        assert new[cfg] == old[cfg], cfg
    assert doc["scratch"] == gold["scratch"]


def test_known_plans(run):
    """Figures of the parent commit, full frame, group size free; cfg = (w, h, ps, max_level, gy0, gy1, lk_g,
    lk_astrip, max_batch)."""
    _, doc, _ = run
    plans = by_cfg(doc)

    def shapes(p):
        return [(lv["G"], lv["UW"]) for lv in p["lv"]]
    for mb, strips in ((32, [7, 7, 8, 8, 8]), (1, [27, 27, 28, 28, 32])):
        p = plans[(1920, 1080, 10, 5, 0, -1, 0, 0, mb)]
        assert p["bytes_per_pair"] == 57284608 and p["nch"] == 1
        assert shapes(p) == [(8, 112), (4, 56), (4, 56), (4, 56), (4, 56)]
        assert [lv["asp"] for lv in p["lv"]] == [10, 5, 5, 5, 5]
        assert [lv["nstrip"] for lv in p["lv"]] == strips
    p = plans[(320, 240, 10, 5, 0, -1, 0, 0, 32)]
    assert p["bytes_per_pair"] == 2443264 and shapes(p) == [(8, 112), (4, 56), (4, 56)]
    p = plans[(72, 72, 3, 5, 0, -1, 0, 0, 32)]
    assert p["bytes_per_pair"] == 212736 and shapes(p) == [(4, 56)] and p["lv"][0]["asp"] == 0
    assert plans[(41, 41, 1, 5, 0, -1, 0, 0, 32)]["nlev"] == 1
    p = plans[(100, 100, 1, 5, 0, -1, 0, 0, 32)]
    assert p["nlev"] == 2 and (p["lv"][1]["nrx"], p["lv"][1]["nry"]) == (2, 2)
    p = plans[(1280, 720, 33, 5, 0, -1, 0, 0, 32)]
    assert (8, 512) in shapes(p) and (p["lv"][-1]["nrx"], p["lv"][-1]["nry"]) == (16, 16)
    assert plans[(3840, 2160, 10, 5, 0, -1, 0, 0, 32)]["nlev"] == 6
    for lk_g in (0, 4, 8):   # no kernel shape holds a group 70 px apart at level 0: the single-kernel LK
        assert plans[(1920, 1080, 70, 5, 0, -1, lk_g, 0, 32)]["nch"] == 0
