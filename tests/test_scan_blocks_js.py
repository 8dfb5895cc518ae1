"""Cube.scan / Cube.iterateOverDimension served from one device pass (tests/js/scan_blocks_test.js): hand-worked
literals on a 2 x 3 x 2 cube, and the per-combination loop on a seeded cube of four measures of mixed cell type and
default — the same getData, getNestedObject, getTotal, serialize() bytes and rules, also after drillUp and dice of a
handed-out cube."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NODE = shutil.which("node")

pytestmark = pytest.mark.gpu


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_scan_and_iterate_over_dimension_in_one_device_pass():
    r = subprocess.run([NODE, os.path.join(HERE, "js", "scan_blocks_test.js")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " 0 failed" in r.stdout
