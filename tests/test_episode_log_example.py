"""examples/training_monitor.py at a tiny size: it streams, reads windows of the episode log and switches stages on them."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_training_monitor_example_runs():
    # a bound above 100 %: every settled window ends its stage, so the run must switch at least once
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "training_monitor.py"), "--worlds", "16", "--depth", "3",
                        "--steps", "384", "--check", "64", "--window", "16", "--bound", "101", "--max-agents", "4"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout
    switches = re.findall(r"^step +\d+: collision rate [\d.]+ % over 16 episodes \(\d+ since the last switch\) -> stage (\d+), (\d+) agents$",
                          out, flags=re.M)
    assert switches and switches[0] == ("1", "3"), out
    m = re.search(r"^monitor done: stage (\d+), (\d+) agents, (\d+) episodes logged, last collision rate [\d.]+ %, lapped 0$", out, flags=re.M)
    assert m, out
    assert int(m.group(1)) == len(switches) and int(m.group(2)) == 2 + len(switches) and int(m.group(3)) >= 16, out
