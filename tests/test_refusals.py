"""The refusal matrix of the step consumers (episode records, episode log, trajectory ring), of restore() / fork() and of the calls
that need an *_init first: which error wins when several compete, and every text byte for byte.  The expected texts are literals
(`%s` stands for the refused call's name); the library's are read back through cagym_last_error after a raw call whose arguments are
valid apart from the refused state, and after every raw refusal the handle still steps.
Two handles of 4 worlds x 4 agents and 8 scenarios: one without rectangles, one with max_obstacles=4 for the exploration stream."""
import ctypes as C
import importlib

import pytest

pytestmark = pytest.mark.gpu
_lib = importlib.import_module("gym-exploration-2d_amd._lib")
E_STATE, E_UNSUPPORTED = -5, -6
N, M, S = 4, 4, 8

CONTRACT = {
    "ring": "%s(auto_reset=False) with a trajectory ring attached: the ring is fed by cagym_step_autoreset_keep only, every step exactly "
            "once and in order (include/cagym.h); detach_trajectory_ring() first",
    "log": "%s(auto_reset=False) with an episode log attached: cagym_episode_log_update takes the outputs of auto-reset stepping only, "
           "every step exactly once and in order (include/cagym.h); detach_episode_log() first",
    "records": "%s(auto_reset=False) with episode records attached: cagym_episode_records_update takes the outputs of auto-reset "
               "stepping only, every step exactly once and in order (include/cagym.h); detach_episode_records() first"}
TIMELINE = {
    "planner": "%s() with ig_greedy attached: the planner's workspace, its published plans and the host-side call counter are not part "
               "of a snapshot; detach_ig_mcts() first",
    "log": "%s() with an episode log attached: its running rows would describe another timeline (the library refuses as long as the "
           "log is initialised)",
    "ring": "%s() with a trajectory ring attached: its running values would describe another timeline (the library refuses as long as "
            "the ring is initialised)"}
STREAMING = {
    "restore": "restore() on a streaming env: the ring of scenario slots is not part of a snapshot (a restored episode index would meet "
               "other scenarios); stop_streaming() first",
    "fork": "fork() on a streaming env: the ring of scenario slots is not part of a snapshot, and a refill would overwrite the forked "
            "slot; stop_streaming() first"}
SPLIT_KEEP = {
    "ring": "%s(auto_reset=True)() with a trajectory ring attached: the split step ends in the auto-resetting launch, which overwrites "
            "the terminal observation and the terminal state; use step(auto_reset=True)",
    "keep": "%s(auto_reset=True)() with keep_terminal_observations() on: the split step ends in the auto-resetting launch, which "
            "overwrites the terminal observation and the terminal state; use step(auto_reset=True)"}
PLANNER_KEEP = {
    "ring": "%s() with a trajectory ring attached: an attached IG planner's per-world restart reads the game_over of the auto-resetting "
            "launch; the three-launch step has not been taken through it",
    "keep": "%s() with keep_terminal_observations() on: an attached IG planner's per-world restart reads the game_over of the "
            "auto-resetting launch; the three-launch step has not been taken through it"}
LIBRARY = {  # of cagym_restore and cagym_fork
    "streaming": (E_UNSUPPORTED, "%s on a streaming handle: the ring of scenario slots is not part of a snapshot"),
    "records": (E_STATE, "%s with episode records initialised: their running rows would describe another timeline; detach the records first"),
    "log": (E_STATE, "%s with an episode log initialised: its running rows would describe another timeline"),
    "ring": (E_STATE, "%s with a trajectory ring initialised: its running values would describe another timeline")}
BEFORE_INIT = [
    "cagym_episode_records_update before cagym_episode_records_init", "cagym_episode_records_restart before cagym_episode_records_init",
    "cagym_episode_records_get before cagym_episode_records_init", "cagym_episode_log_update before cagym_episode_log_init",
    "cagym_episode_log_restart before cagym_episode_log_init", "cagym_episode_log_get before cagym_episode_log_init",
    "cagym_trajectory_restart before cagym_trajectory_init", "cagym_trajectory_get before cagym_trajectory_init",
    "cagym_ig_reset_belief before cagym_ig_init"]


def _env(**kw):
    B = importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv
    return B(N, M, n_scenarios=S, game_over_mode="agent0", **kw)


def _raises(text, fn, *args, **kw):
    with pytest.raises(RuntimeError) as ei:
        fn(*args, **kw)
    assert str(ei.value) == text


def _contract(env, who):
    """step, step_finish and rollout without auto-reset are refused with `who`'s text"""
    _raises(CONTRACT[who] % "step", env.step, auto_reset=False)
    _raises(CONTRACT[who] % "step_finish", env.step_finish, auto_reset=False)
    _raises(CONTRACT[who] % "rollout", env.rollout, 2, auto_reset=False)


def _new_timeline(env, snap, restore_text, fork_text):
    _raises(restore_text, env.restore, snap)
    _raises(fork_text, env.fork, [0], [1])


def _keep(env, who):
    """the split step with auto-reset and attaching an IG planner are refused with `who`'s text"""
    _raises(SPLIT_KEEP[who] % "step_finish", env.step_finish, auto_reset=True)
    _raises(SPLIT_KEEP[who] % "step_overlapped", env.step_overlapped, lambda a: None, None, auto_reset=True)
    _raises(PLANNER_KEEP[who] % "attach_ig_mcts", env.attach_ig_mcts)
    _raises(PLANNER_KEEP[who] % "attach_ig_greedy", env.attach_ig_greedy)


def _raw(env, rc, want_rc, want_text):
    """a raw call's code and cagym_last_error; then the handle still steps"""
    assert rc == want_rc and env.L.cagym_last_error(env.h).decode() == want_text
    env.step(auto_reset=True)


def _raw_new_timeline(env, snap, ids, who):
    """cagym_restore and cagym_fork, every argument valid, refused with `who`'s code and text"""
    code, text = LIBRARY[who]
    st = env._stream()
    _raw(env, env.L.cagym_restore(env.h, C.byref(snap.layout), snap.blob.data_ptr(), None, snap.n, st), code, text % "cagym_restore")
    _raw(env, env.L.cagym_fork(env.h, ids[:1].data_ptr(), ids[1:].data_ptr(), 1, st), code, text % "cagym_fork")


def test_consumers_on_a_fixed_pool():
    import torch
    env = _env()
    assert env.generate_scenarios(seed=1) == 0
    env.reset()
    L, h, st = env.L, env.h, env._stream()
    ids = torch.tensor([0, 1], dtype=torch.int32, device=env.device)
    out = (env.flags.data_ptr(), env.reward.data_ptr(), env.game_over.data_ptr(), 1, st)
    calls = [lambda: L.cagym_episode_records_update(h, *out), lambda: L.cagym_episode_records_restart(h, None, 0, st),
             lambda: L.cagym_episode_records_get(h, C.byref(_lib.CagymEpisodeRecordPtrs())),
             lambda: L.cagym_episode_log_update(h, *out), lambda: L.cagym_episode_log_restart(h, None, 0, st),
             lambda: L.cagym_episode_log_get(h, C.byref(_lib.CagymEpisodeLogPtrs())),
             lambda: L.cagym_trajectory_restart(h, None, 0, st), lambda: L.cagym_trajectory_get(h, C.byref(_lib.CagymTrajectoryPtrs())),
             lambda: L.cagym_ig_reset_belief(h, None, st)]
    for call, text in zip(calls, BEFORE_INIT):
        _raw(env, call(), E_STATE, text)
    snap = env.snapshot()
    # the ring alone (the library checks records, log, ring in that order, and keeps each once it is initialised: ring first)
    env.attach_trajectory_ring(4)
    _contract(env, "ring")
    _new_timeline(env, snap, TIMELINE["ring"] % "restore", TIMELINE["ring"] % "fork")
    _raw_new_timeline(env, snap, ids, "ring")
    _keep(env, "ring")
    # ring and log: the ring's contract text wins; restore / fork name the log first, on the host and in the library
    env.attach_episode_log(16)
    _contract(env, "ring")
    _new_timeline(env, snap, TIMELINE["log"] % "restore", TIMELINE["log"] % "fork")
    _raw_new_timeline(env, snap, ids, "log")
    # all three: ring, then log, then records
    env.attach_episode_records()
    _contract(env, "ring")
    _raw_new_timeline(env, snap, ids, "records")
    env.detach_trajectory_ring()
    _contract(env, "log")
    env.detach_episode_log()
    _contract(env, "records")
    # records alone: the host lets restore / fork through and the library refuses
    code, text = LIBRARY["records"]
    _new_timeline(env, snap, "cagym_restore failed (%d): %s" % (code, text % "cagym_restore"),
                  "cagym_fork failed (%d): %s" % (code, text % "cagym_fork"))
    # the log alone
    env.detach_episode_records()
    env.attach_episode_log(16)
    _contract(env, "log")
    _new_timeline(env, snap, TIMELINE["log"] % "restore", TIMELINE["log"] % "fork")
    env.detach_episode_log()
    # terminal observations
    env.keep_terminal_observations()
    _keep(env, "keep")
    env.keep_terminal_observations(False)
    env.step(auto_reset=False)  # nothing attached any more
    env.close()


def test_restore_and_fork_on_an_exploration_stream():
    import torch
    env = _env(max_obstacles=4)
    assert env.stream_exploration_worlds(kinds="train_stage_1", seed=21, n_robots=2, n_targets=2, n_obst=(1, 4), robot_pref_speed=30.0) == 0
    env.reset()
    snap = env.snapshot()
    ids = torch.tensor([0, 1], dtype=torch.int32, device=env.device)
    _raw_new_timeline(env, snap, ids, "streaming")
    _new_timeline(env, snap, STREAMING["restore"], STREAMING["fork"])
    env.attach_trajectory_ring(4)  # ring > streaming
    _new_timeline(env, snap, TIMELINE["ring"] % "restore", TIMELINE["ring"] % "fork")
    env.attach_episode_log(16)     # log > ring > streaming
    _new_timeline(env, snap, TIMELINE["log"] % "restore", TIMELINE["log"] % "fork")
    _raw_new_timeline(env, snap, ids, "streaming")  # the library names the stream first
    env.detach_trajectory_ring()
    env.attach_ig_greedy(episodic=True)  # planner > log > streaming
    _new_timeline(env, snap, TIMELINE["planner"] % "restore", TIMELINE["planner"] % "fork")
    env.detach_ig_mcts()
    _new_timeline(env, snap, TIMELINE["log"] % "restore", TIMELINE["log"] % "fork")
    env.detach_episode_log()
    _new_timeline(env, snap, STREAMING["restore"], STREAMING["fork"])
    env.close()
