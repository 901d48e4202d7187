"""examples/lookahead_fork.py (env.fork / snapshot / restore in a look-ahead loop) runs end to end on the GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_lookahead_fork_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "lookahead_fork.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "lookahead_fork: 8 worlds x 11 siblings, H = 5, 20 decisions" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
