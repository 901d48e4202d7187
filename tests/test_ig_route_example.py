"""GPU: examples/exploration_viewpoints.py --rank route runs end to end at 16 worlds - every robot that chooses is sent to
ig_route_gains' best proposal, with and without headings - and prints its table; both policies' episode logs join on the stream key."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("headings", [0, 8])
def test_the_viewpoints_example_runs_with_route_ranking(headings):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "exploration_viewpoints.py"), "--worlds", "16", "--steps", "64",
                        "--rank", "route", "--stride", "4", "--headings", str(headings)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    rows = {}
    for name in ("viewpoints", "ig_greedy"):
        m = re.search(r"^%s\s+episodes\s+(\d+)  return mean (-?[\d.]+) median" % name, p.stdout, flags=re.M)
        assert m, (name, p.stdout)
        rows[name] = (int(m.group(1)), float(m.group(2)))
    assert all(n > 0 for n, _ in rows.values()), rows
    m = re.search(r"^viewpoints targets set (\d+)  moved off a teammate's (\d+)", p.stdout, flags=re.M)
    assert m and int(m.group(1)) >= 16 * 2, p.stdout  # every robot was asked to choose at least once
    m = re.search(r"^viewpoints - ig_greedy on\s+(\d+) shared worlds: mean return difference ([-+][\d.]+)", p.stdout, flags=re.M)
    assert m and int(m.group(1)) > 0, p.stdout  # the two logs join on the stream key
    assert int(m.group(1)) <= min(n for n, _ in rows.values())
    assert p.stdout.rstrip().endswith("exploration viewpoints done")
