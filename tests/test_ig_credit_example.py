"""GPU: examples/exploration_marl.py runs end to end at its smallest size - a team on an exploration stream through
CagymRobotVecEnv, per-robot returns for the three kinds of credit next to the team's."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_marl_example_runs():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "exploration_marl.py"), "--worlds", "16", "--steps", "32"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert re.search(r"^marl\s+envs 48 = 16 worlds x 3 robots  obs \(48, 3, 24, 24\)  reward 'difference'", p.stdout, flags=re.M), p.stdout
    m = re.search(r"^team\s+episodes (\d+)  mean return (-?[\d.]+)", p.stdout, flags=re.M)
    assert m and int(m.group(1)) > 0 and float(m.group(2)) > 0, p.stdout
    team = float(m.group(2))
    rows = re.findall(r"^robot (\d)\s+mean return  own (-?[\d.]+)  exclusive (-?[\d.]+)  difference (-?[\d.]+)", p.stdout, flags=re.M)
    assert [int(r[0]) for r in rows] == [0, 1, 2], p.stdout
    own, excl = sum(float(r[1]) for r in rows), sum(float(r[2]) for r in rows)
    assert all(float(r[1]) > 0 for r in rows), rows
    assert excl <= team + 1e-3 and team <= own + 1e-3, (excl, team, own)  # sum exclusive <= gain <= sum own, at the printed precision
    assert p.stdout.rstrip().endswith("exploration marl done")
