"""examples/exploration_eval.py at a tiny size: three policies on one stream seed, each with the IG team's episode log, the
statistics per policy and the paired return differences by stream key."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_exploration_eval_example_runs():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "exploration_eval.py"), "--worlds", "16", "--steps", "48"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout
    rows = dict(re.findall(r"^(random|ig_greedy|ig_mcts) +episodes +(\d+)  return mean [\d.]+ median [\d.]+  found [\d.]+ of targets", out, flags=re.M))
    assert sorted(rows) == ["ig_greedy", "ig_mcts", "random"] and all(int(n) >= 8 for n in rows.values()), out
    pairs = re.findall(r"^(\w+) +- (\w+) +on +(\d+) shared worlds: mean return difference [+-][\d.]+, better on [\d.]+ of them$", out, flags=re.M)
    assert [(a, b) for a, b, _ in pairs] == [("ig_greedy", "random"), ("ig_mcts", "random"), ("ig_mcts", "ig_greedy")], out
    # every world both policies finished pairs up: at least the first episode of most of the 16 worlds
    assert all(8 <= int(n) <= min(int(rows[a]), int(rows[b])) for a, b, n in pairs), out
    assert out.rstrip().endswith("exploration eval done")
