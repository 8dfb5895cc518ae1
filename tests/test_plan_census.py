"""Every drillUp shape gets the plan it got before the planner became a unit of its own (olap_plan_drillup.hip) and the
regime decision one function (drillup_form, olap_kernels.hpp): tests/_plan_census_worker.py prints kernel name and
Plan.describe() for some 1 200 plans — the shapes of the dry-planning worker, every shape at which test_gpu_parity.py
asserts a kernel name, both sides of every threshold; plans of a shape that differ only in dtype, default or rule share
a line — and tests/golden/drillup_plan_census.txt holds what the commit before that change printed (its describe() had
no `form` key).  Later work on the regimes regenerates the golden and
its diff shows which shapes moved."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "drillup_plan_census.txt")
DEVICE_SECTION = "# ---- device section"

# what olap_plan_kernel_name says for every form of Plan.describe()
KERNELS = {
    "rows": {"drillup_rows_kernel"},
    "rows_ragged": {"drillup_rows_kernel"},
    "tile": {"drillup_tile_kernel"},
    "gtile": {"drillup_gtile_kernel"},
    # "drillup_tile_kernel": a shape of the tile regime that the 16-byte grid keeps out of it (see flat_with_the_tile_name)
    "flat": {"drillup_flat_kernel", "drillup_tile_kernel"},
    "segments": {"drillup_rows_kernel (segments)+segments_combine_kernel"},
    "reduce4": {"drillup_reduce4_kernel", "drillup_reduce4_kernel+drillup_merge_kernel"},
    "reduce": {"drillup_reduce_kernel+drillup_merge_kernel"},
    "split4": {"drillup_split4_kernel+drillup_merge_kernel"},
    "split": {"drillup_split_kernel+drillup_merge_kernel"},
    "generic": {"drillup_generic_kernel"},
}


def golden_sections():
    lines = open(GOLDEN).read().splitlines()
    at = lines.index(next(l for l in lines if l.startswith(DEVICE_SECTION)))
    return lines[:at], lines[at + 1:]


def run_worker(args, extra_env):
    env = dict(os.environ, **extra_env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_plan_census_worker.py")] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout.splitlines()


def flat_with_the_tile_name(line, fields):
    """A plan names the tile kernel for every shape of the tile regime; where no whole number of rows per tile (fewer than four
    fit) puts every tile on the 16-byte grid, the launch runs flat even over aligned buffers.  Only those may differ."""
    item = 8 if "| float64/" in line else 4
    row, budget, per16 = int(fields["K"]) * int(fields["inner"]), 16384 // item, 16 // item
    pitch = int(fields["perm_pitch"]) * int(fields["inner"]) if fields["contiguous"] == "0" and int(fields["perm_pitch"]) else row
    rows = budget // pitch
    if rows >= 4:
        rows &= ~3
    while rows > 0 and (rows * row) % per16:
        rows -= 1
    return int(fields["inner"]) < 128 and 0 < row <= budget and rows == 0


def compare(got, want):
    """line by line; the `form` key is checked against the kernel name, not against the golden, which has no `longest_group`
    either (an empty axis given as a NULL map has empty groups: 0)"""
    assert len(got) == len(want), (len(got), len(want))
    forms = set()
    for g, w in zip(got, want):
        m = re.search(r" form=(\w+)", g)
        if m is None:  # a comment or the closing line
            assert g == w, (g, w)
            continue
        longest = re.search(r" longest_group=(\d+)", g)
        assert g.replace(m.group(0), "", 1).replace(longest.group(0), "", 1) == w, "\n got: %s\nwant: %s" % (g, w)
        assert "NULL map" not in g or longest.group(1) == "0", g
        name = g.split(" -> ")[2].split(" | ")[0]
        form = m.group(1)
        assert name in KERNELS[form], g
        if form == "flat" and name != "drillup_flat_kernel":
            assert flat_with_the_tile_name(g, dict(kv.split("=") for kv in g.split(" | ")[-1].split())), g
        forms.add(form)
    return forms


def test_drillup_plans_are_the_recorded_ones():
    """dry planning on the CPU: every form but the segmented rows (which dry planning skips) and the generic one"""
    forms = compare(run_worker([], {"OLAP_PLAN_DRY": "1"}), golden_sections()[0])
    assert forms == set(KERNELS) - {"segments", "generic"}, forms


@pytest.mark.gpu
def test_drillup_plans_with_segmented_rows_are_the_recorded_ones():
    """the shapes that reach the segmented rows, planned on the device (plans only: no store, no launch)"""
    import torch

    want = golden_sections()[1]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if want[0] != "# cus=%d" % cus:
        pytest.skip("the segments are sized by the CU count: recorded with %s, this device has %d" % (want[0][2:], cus))
    forms = compare(run_worker(["--device"], {}), want)
    assert "segments" in forms, forms
