"""The selection module of the Node.js host (olap-in-memory_amd/js/selection.js) without a GPU: filters of
getTotalForDimensionItems / copyMeasureData as device levels, in the per-cell path's nesting order."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_selection_levels_without_gpu():
    r = subprocess.run([NODE, os.path.join(HERE, "js", "select_host_test.js")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " 0 failed" in r.stdout
