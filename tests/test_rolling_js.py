"""Cube.rolling and Cube.shift on the GPU (tests/js/rolling_test.js): hand-worked literals on a monthly TimeDimension and a
seeded [4, 12, 5] cube of mixed types and defaults against the definition run as written (Cube._rollingPerItem), on one
device and with every measure split over two shards (where the measures take the per-item path)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NODE = shutil.which("node")

pytestmark = pytest.mark.gpu


def run_node(env=None):
    r = subprocess.run([NODE, os.path.join(HERE, "js", "rolling_test.js")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-6000:]
    return r.stdout


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_rolling_cube_methods():
    assert " 0 failed" in run_node()


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_rolling_cube_methods_sharded():
    assert " 0 failed" in run_node({"OLAP_DEVICES": "0,0"})
