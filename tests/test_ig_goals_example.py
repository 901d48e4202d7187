"""GPU: examples/exploration_goals.py runs end to end and prints its three rows."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_goals_example_runs():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "exploration_goals.py"), "--worlds", "16", "--steps", "64"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    rows = {}
    for name in ("goals", "random", "ig_greedy"):
        m = re.search(r"^%s\s+episodes (\d+)  mean team return (-?[\d.]+)  last" % name, p.stdout, flags=re.M)
        assert m, (name, p.stdout)
        rows[name] = (int(m.group(1)), float(m.group(2)))
    assert all(n > 0 for n, _ in rows.values()), rows
    m = re.search(r"^goals      set (\d+)  robot-steps at a goal (\d+)", p.stdout, flags=re.M)
    assert m and int(m.group(1)) >= 16 * 2, p.stdout  # every robot was given a goal at least once
    assert p.stdout.rstrip().endswith("exploration goals done")
