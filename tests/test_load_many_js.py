"""Cubes of several stored measures through hydrateFromCube, compose and project / reorderDimensions where the two cubes
hold a measure in different cell types, against cubes of one measure each, a source re-declared on the host and
hand-worked literals (tests/js/load_many_test.js), on one device and with every measure split over two shards."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NODE = shutil.which("node")

pytestmark = pytest.mark.gpu


def run_node(env=None):
    r = subprocess.run([NODE, os.path.join(HERE, "js", "load_many_test.js")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-6000:]
    return r.stdout


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_load_many_cube_methods():
    assert " 0 failed" in run_node()


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_load_many_cube_methods_sharded():
    assert " 0 failed" in run_node({"OLAP_DEVICES": "0,0"})
