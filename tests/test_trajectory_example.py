"""examples/trajectory_dataset.py at a tiny size: it streams, exports the episodes the log names out of the trajectory ring and
writes pickles in the reference's trajectory schema."""
import glob
import os
import pickle
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"time", "pedestrian_goal_position", "coop_coef", "other_agents_pos", "other_agents_vel", "pedestrian_state"}


@pytest.mark.gpu
def test_trajectory_dataset_example_runs(tmp_path):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "trajectory_dataset.py"), "--worlds", "16", "--agents", "4",
                        "--steps", "384", "--every", "128", "--margin", "256", "--out", str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = re.findall(r"^steps +(\d+)  episodes logged +(\d+)  agent trajectories written +(\d+)  -> (\S+)$", p.stdout, flags=re.M)
    assert [int(l[0]) for l in lines] == [128, 256, 384], p.stdout
    assert re.search(r"^stream: \{'generated': \d+, 'n_failed': 0, 'n_lapped': 0, 'depth': 4\}$", p.stdout, flags=re.M), p.stdout
    files = sorted(glob.glob(os.path.join(str(tmp_path), "trajectories_*.pkl")))
    assert len(files) == 3
    total = 0
    for f, line in zip(files, lines):
        with open(f, "rb") as fh:
            trajs = pickle.load(fh)
        assert len(trajs) == int(line[2])
        total += len(trajs)
        for tr in trajs:
            assert tr and all(set(r) == KEYS and set(r["pedestrian_state"]) == {"position", "velocity"} for r in tr)
            assert all(len(r["other_agents_pos"]) == len(r["other_agents_vel"]) for r in tr) and tr[0]["coop_coef"] in (0.5, 1.0)
    assert total > 0, p.stdout
