"""CPU twin of cagym_generate_exploration_scenarios (csrc/cagym_explore.h): sampler_twin.generate for the internal stage parameter
set, then the team edit - robots in slots 0..R-1, targets in slots R..R+T-1.  Also the Python restatement of the field refresh's
window rule (field_next), which tests/test_exploration_twin.py drives with random finish patterns."""
import importlib

import numpy as np

import sampler_twin as tw

scen = importlib.import_module("gym-exploration-2d_amd.scenarios")


def internal_params(n_robots, n_targets, n_obst=None, max_tries=1000):
    """generate_reference_scenarios' arguments of the stage scenario an exploration world starts from"""
    return dict(number_of_agents=n_robots + n_targets, fixed_count=True, ego_policy=scen.POLICY_IGMCTS, ego_dynamics=scen.DYN_FIRSTORDER,
                other_policies=scen.POLICY_STATIC, p_b=0.0, other_dynamics=scen.DYN_FIRSTORDER, n_obst=n_obst, max_tries=max_tries)


def generate(S, M, K, kinds, seed, n_robots, n_targets, n_obst=None, target_radius=0.2, robot_pref_speed=1.0, max_tries=1000):
    """The pool generate_exploration_worlds writes for these arguments (kinds as GEN_* ids), as sampler_twin.generate returns it."""
    kinds = [kinds] if np.isscalar(kinds) else list(kinds)
    assert set(kinds) <= {scen.GEN_STAGE_1, scen.GEN_STAGE_2} and kinds and n_robots >= 1 and n_targets >= 0
    assert 2 <= n_robots + n_targets <= M
    out = tw.generate(S, M, K, kinds, seed, **internal_params(n_robots, n_targets, n_obst, max_tries))
    R, T = n_robots, n_targets
    out["policy"][:, :R] = scen.POLICY_IGMCTS
    out["dynamics"][:, :R] = scen.DYN_FIRSTORDER
    out["agents6"][:, :R, 4] = robot_pref_speed
    out["policy"][:, R:R + T] = scen.POLICY_STATIC
    out["agents6"][:, R:R + T, 5] = target_radius
    return out


class FieldBook(object):
    """The bookkeeping of an exploration stream, one ring of depth k per world: which episode's scenario every slot holds
    (`held`) and which episode's field (`field`), as the refill (cagym_stream.h) and the field refresh (cagym_explore.h) move them.
    Slots are (world, episode % k) pairs: world w owns pool slots w, w + N, ..."""

    def __init__(self, N, k):
        self.N, self.k = N, k
        self.episode = np.zeros(N, np.int64)
        self.next_episode = np.full(N, k, np.int64)
        self.field_next = np.full(N, k, np.int64)
        self.held = np.tile(np.arange(k), (N, 1))   # held[w, j]: the episode whose scenario slot j of world w holds
        self.field = self.held.copy()               # field[w, j]: the episode whose raster that slot's field was built from
        self.generated, self.fields_built, self.n_lapped = N * k, 0, 0
        self.touched = []                           # (world, slot, current slot) of every field write of the last refill

    def finish(self, w, n=1):
        self.episode[w] += n

    def refill(self):
        N, k = self.N, self.k
        for w in range(N):
            ep, nx = self.episode[w], self.next_episode[w]
            self.n_lapped += int(nx <= ep)
            first, last = max(nx, ep + 1), ep + k - 1
            if first <= last:
                for e in range(first, last + 1):
                    self.held[w, e % k] = e
                    self.generated += 1
                self.next_episode[w] = ep + k
        self.touched = []
        for w in range(N):
            ep, nx, fn = self.episode[w], self.next_episode[w], self.field_next[w]
            lo, hi = max(fn, ep + 1), nx - 1
            for e in range(lo, hi + 1):
                self.field[w, e % k] = e
                self.fields_built += 1
                self.touched.append((w, e % k, ep % k))
            self.field_next[w] = max(fn, nx)
