"""Cube.variance / Cube.stddev on the GPU (tests/js/variance_test.js): hand-worked literals — the spread of a month's days
on a daily TimeDimension, a GenericDimension whose region groups interleave — and a seeded cube of mixed types, defaults
and rules (`first` / `last` included) against the definition written out on the host (Cube._varianceHost), on one
device and with the measures split over two shards (where the untracked measures take the host path and
HipStore.lastVariancePath says 'host')."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NODE = shutil.which("node")

pytestmark = pytest.mark.gpu


def run_node(env=None):
    r = subprocess.run([NODE, os.path.join(HERE, "js", "variance_test.js")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-6000:]
    return r.stdout


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_variance_cube_methods():
    assert " 0 failed" in run_node()


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_variance_cube_methods_sharded():
    assert " 0 failed" in run_node({"OLAP_DEVICES": "0,0"})
