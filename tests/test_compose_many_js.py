"""Cube.compose with one device pass per source cube against the reference's order of calls (Cube._composePerMeasure):
the compose cases of tests/js/gpu_test.js with 1, 3 and 9 measures per cube, a tracked measure among sum measures,
computed measures on the composed cube and what follows a compose (tests/js/compose_many_test.js), on one device and
with every measure split over two shards."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NODE = shutil.which("node")

pytestmark = pytest.mark.gpu


def run_node(env=None):
    r = subprocess.run([NODE, os.path.join(HERE, "js", "compose_many_test.js")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-6000:]
    return r.stdout


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_compose_many_cube_methods():
    assert " 0 failed" in run_node()


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_compose_many_cube_methods_sharded():
    assert " 0 failed" in run_node({"OLAP_DEVICES": "0,0"})
