"""step(auto_reset=True) through cagym_step_autoreset_keep (keep_terminal_observations / attach_trajectory_ring): the three-launch step
must equal the auto-resetting launch bit for bit, and the terminal rows it keeps must be the observation an un-reset twin holds
before its own reset.  Shapes and pools: tests/terminal_util.py.

One recorded run per configuration feeds the tests (four handles stepped side by side for 60 steps):
  A  plain step(auto_reset=True), episode records and episode log attached;
  B  keep_terminal_observations() and a trajectory ring, the same recorders attached; its terminal buffers are filled with a
     sentinel before every step;
  C  step() and reset(world_mask=game_over, advance_episode=True), read between the two;
  D  CagymVecEnv(terminal_observation=True)."""
import functools
import importlib

import numpy as np
import pytest

import terminal_util as tu

pytestmark = pytest.mark.gpu
SENTINEL = -7.0
# (M, game_over_mode, rectangles + LaserScan): both copy widths, both rules, the laser configuration at M = 4
CONFIGS = [(4, "agent0", False), (7, "all", False), (7, "agent0", False), (4, "all", True)]


def _keys(laser):
    return ["dist_to_goal", "rel_goal", "heading_ego_frame", "other_agents_states"] + (["laserscan"] if laser else [])


@functools.lru_cache(maxsize=None)
def _run(M, mode, laser):
    import torch
    vec = importlib.import_module("gym-exploration-2d_amd.vecenv")
    A, Bk, Cn, Dn = (tu.make_env(M, mode, laser) for _ in range(4))
    for e in (A, Bk):
        e.attach_episode_records("last")
        e.attach_episode_log(64)
    Bk.keep_terminal_observations()
    Bk.attach_trajectory_ring(16)
    V = vec.CagymVecEnv(Dn, _keys(laser), terminal_observation=True)
    flat_c = vec.FlatObservation(Cn, _keys(laser))
    rec = []
    for _ in range(tu.STEPS):
        A.step(auto_reset=True)
        for t in Bk._term.values():
            t.fill_(SENTINEL)
        _, _, _, info = Bk.step(auto_reset=True)
        assert info["terminal"]["valid"] is Bk.game_over
        Cn.step()
        c_out, c_flat = tu.outputs(Cn), flat_c().cpu().numpy()
        Cn.reset(world_mask=Cn.game_over.clone(), advance_episode=True)
        _, _, dones, infos = V.step(None)
        rec.append({"A": (tu.outputs(A), tu.state(A)), "B": (tu.outputs(Bk), tu.state(Bk)),
                    "term": {k: v.cpu().numpy().copy() for k, v in info["terminal"].items()}, "C": c_out, "C_flat": c_flat,
                    "D_done": dones.cpu().numpy().copy(), "D_term": infos["terminal_observation"].cpu().numpy().copy()})
    torch.cuda.synchronize()
    tables = {}
    for name, e in (("A", A), ("B", Bk)):
        tables[name] = ({k: v.cpu().numpy() for k, v in e.episode_records().items()},
                        {k: v.cpu().numpy() for k, v in e.episode_log_views().items()})
    for e in (A, Bk, Cn, Dn):
        e.close()
    tu.assert_restarts([r["C"]["game_over"] for r in rec])
    return rec, tables


@pytest.mark.parametrize("M,mode,laser", CONFIGS)
def test_keep_step_equals_autoreset_step_bitwise(M, mode, laser):
    rec, _ = _run(M, mode, laser)
    for t, r in enumerate(rec):
        (out_a, st_a), (out_b, st_b) = r["A"], r["B"]
        assert ("obs_laser" in out_a) == laser
        assert "episode" in st_a and "stat_return" in st_a and "stat_outcomes" in st_a
        tu.assert_same_dicts(out_a, out_b, "outputs, step %d" % t)
        tu.assert_same_dicts(st_a, st_b, "state, step %d" % t)


@pytest.mark.parametrize("M,mode,laser", CONFIGS)
def test_terminal_rows_equal_the_unreset_twin(M, mode, laser):
    rec, _ = _run(M, mode, laser)
    pairs = [("other_agents_states", "obs_oas"), ("ego", "obs_ego")] + ([("laserscan", "obs_laser")] if laser else [])
    checked = 0
    for t, r in enumerate(rec):
        go = r["C"]["game_over"].astype(bool)
        assert np.array_equal(r["term"]["valid"].astype(bool), go), t
        assert tu.same(r["B"][0]["game_over"], r["C"]["game_over"]), t
        for kt, kc in pairs:
            assert tu.same(r["term"][kt][go], r["C"][kc][go]), (t, kt)
            assert (r["term"][kt][~go] == np.float32(SENTINEL)).all(), (t, kt)  # rows of unfinished worlds are not touched
        checked += int(go.sum())
    assert checked >= tu.N_WORLDS


@pytest.mark.parametrize("M,mode,laser", CONFIGS)
def test_records_and_log_are_fed_identically(M, mode, laser):
    _, tables = _run(M, mode, laser)
    (rec_a, log_a), (rec_b, log_b) = tables["A"], tables["B"]
    assert int(rec_a["desync"][0]) == 0 and int(log_a["desync"][0]) == 0
    assert int(log_a["head"][0]) >= tu.N_WORLDS and rec_a["count"].sum() >= tu.N_WORLDS
    tu.assert_same_dicts(rec_a, rec_b, "episode records")
    tu.assert_same_dicts(log_a, log_b, "episode log")


@pytest.mark.parametrize("M,mode,laser", CONFIGS)
def test_vecenv_terminal_observation(M, mode, laser):
    rec, _ = _run(M, mode, laser)
    checked = 0
    for t, r in enumerate(rec):
        done = r["D_done"].astype(bool)
        assert np.array_equal(done, r["C"]["game_over"].astype(bool)), t
        assert r["D_term"].shape == r["C_flat"].shape and r["D_term"].dtype == np.float32
        assert tu.same(r["D_term"][done], r["C_flat"][done]), t
        checked += int(done.sum())
    assert checked >= tu.N_WORLDS


@pytest.mark.parametrize("M", [4, 7])
def test_terminal_rows_into_buffers_that_are_not_16_byte_aligned(M):
    """the capture kernel's 4-byte path: caller-owned terminal buffers that start 4 bytes past an aligned address, through the C
    entry, against the env-owned (aligned, 16-byte path) buffers of a twin"""
    import ctypes
    import torch
    lib = importlib.import_module("gym-exploration-2d_amd._lib")
    A, Bk = tu.make_env(M, "all"), tu.make_env(M, "all")
    A.keep_terminal_observations()
    N = A.N
    raw = {"other_agents_states": torch.empty(N * M * (M - 1) * 10 + 1, dtype=torch.float32, device=A.device),
           "ego": torch.empty(N * M * 12 + 1, dtype=torch.float32, device=A.device)}
    term = lib.CagymTerminalOutputs(raw["other_agents_states"].data_ptr() + 4, raw["ego"].data_ptr() + 4, None)
    assert term.obs_oas % 16 == 4 and term.obs_ego % 16 == 4
    G = []
    for t in range(tu.STEPS):
        for k in raw:
            raw[k].fill_(SENTINEL)
            A._term[k].fill_(SENTINEL)
        A.step(auto_reset=True)
        assert A.L.cagym_step_autoreset_keep(Bk.h, None, ctypes.byref(Bk._out), ctypes.byref(term), Bk._stream()) == 0
        for k in raw:
            assert torch.equal(raw[k][1:].view(torch.int32), A._term[k].reshape(-1).view(torch.int32)), (t, k)
            assert float(raw[k][0]) == SENTINEL
        G.append(tu.outputs(A)["game_over"])
        assert (A._term["ego"][~A.game_over.bool()] == SENTINEL).all() and (A._term["ego"][A.game_over.bool()] != SENTINEL).any() == bool(G[-1].any())
    tu.assert_restarts(G)
    tu.assert_same_dicts(tu.state(A), tu.state(Bk), "state")
    A.close()
    Bk.close()


def test_keep_step_replays_from_a_captured_graph():
    """no argument of cagym_step_autoreset_keep advances on the host: one captured step, replayed, keeps pace with an eager twin -
    outputs, state, terminal rows and the ring's slices (the log's update rides in the same graph)"""
    import torch
    A, Bk, Cn = (tu.make_env(4, "agent0") for _ in range(3))
    for e in (Bk, Cn):
        e.keep_terminal_observations()
        e.attach_trajectory_ring(64)
        e.attach_episode_log(64)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        Bk.step(auto_reset=True)  # warm-up on the side stream (step 0)
    torch.cuda.current_stream().wait_stream(s)
    A.step(auto_reset=True)
    Cn.step(auto_reset=True)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        Bk.step(auto_reset=True)
    G = []
    for t in range(1, 40):
        A.step(auto_reset=True)
        Cn.step(auto_reset=True)
        g.replay()
        tu.assert_same_dicts(tu.outputs(A), tu.outputs(Bk), "outputs, step %d" % t)
        tu.assert_same_dicts(tu.state(A), tu.state(Bk), "state, step %d" % t)
        G.append(tu.outputs(A)["game_over"])
    tu.assert_restarts(G)
    for k, v in Cn.trajectory_views().items():
        assert torch.equal(v, Bk.trajectory_views()[k]), k
    assert int(Bk.trajectory_views()["head"].item()) == 40
    for k, v in Cn.episode_log_views().items():
        assert torch.equal(v, Bk.episode_log_views()[k]), k
    for k, v in Cn._term.items():
        assert torch.equal(v, Bk._term[k]), k
    for e in (A, Bk, Cn):
        e.close()


@pytest.mark.parametrize("M", [4, 7])
def test_keep_step_with_ga3c_attached(M):
    """One GA3C agent per world (slot 0), driven inside step(): 20 steps of both paths are bitwise equal - and so are the 40 after
    them, which let every world reach agent 0's time limit (at most 38 steps) so that the restarts the comparison relies on happen."""
    the_pool = tu.pool(M, seed=5, ga3c=True)
    A, Bk = (tu.make_env(M, "agent0", False, the_pool) for _ in range(2))
    A.attach_ga3c()
    Bk.attach_ga3c()
    Bk.keep_terminal_observations()
    Bk.attach_trajectory_ring(8)
    G = []
    for t in range(tu.STEPS):
        A.step(auto_reset=True)
        Bk.step(auto_reset=True)
        tu.assert_same_dicts(tu.outputs(A), tu.outputs(Bk), "outputs, step %d" % t)
        tu.assert_same_dicts(tu.state(A), tu.state(Bk), "state, step %d" % t)
        G.append(tu.outputs(A)["game_over"])
    assert np.asarray(G[:20]).any()  # a restart inside the first 20 steps (the head-on scenarios)
    tu.assert_restarts(G)
    A.close()
    Bk.close()
