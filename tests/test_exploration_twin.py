"""Exploration worlds without a GPU: the ABI's new entries, the CPU twin's team edit (tests/exploration_twin.py) and the window
rule of the field refresh behind an exploration stream's refill (include/cagym.h: cagym_stream_exploration_scenarios)."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import exploration_twin as xt
import sampler_twin as tw

scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"cagym_generate_exploration_scenarios": 4, "cagym_stream_exploration_scenarios": 4, "cagym_stream_set_exploration_params": 2,
           "cagym_explore_stream_get": 3}
FIELDS = ["seed", "kinds_mask", "n_robots", "n_targets", "n_obst_min", "n_obst_max", "max_tries", "target_radius", "robot_pref_speed"]


def test_header_and_prototype_table_carry_the_exploration_entries():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cagym.h")).read(), flags=re.S)
    declared = {n: (0 if p.strip() in ("", "void") else p.count(",") + 1)
                for n, p in re.findall(r"\b(cagym_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src)}
    lib = importlib.import_module("gym-exploration-2d_amd._lib")
    for name, n_params in ENTRIES.items():
        assert declared.get(name) == n_params, (name, declared.get(name))
        assert name in lib._ARGTYPES and len(lib._ARGTYPES[name]) == n_params, name
    body = re.search(r"struct\s+cagym_explore_params\s*\{([^}]*)\}", src).group(1)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == FIELDS, names
    assert [f[0] for f in lib.CagymExploreParams._fields_] == FIELDS
    # two 8-byte words, six 4-byte ones, two doubles: no padding on either side of the ABI
    assert C.sizeof(lib.CagymExploreParams) == 48 and lib.CagymExploreParams.target_radius.offset == 32
    # the existing stream words were not widened
    assert [f[0] for f in lib.CagymStreamPtrs._fields_] == ["next_episode", "generated", "n_failed", "n_lapped"]
    L = lib.load()
    for name in ENTRIES:
        assert hasattr(L, name), name


@pytest.mark.parametrize("kind", [scen.GEN_STAGE_1, scen.GEN_STAGE_2])
def test_twin_is_the_stage_scenario_plus_the_team_edit(kind):
    S, M, K, R, T = 256, 6, 10, 2, 3
    kw = dict(n_obst=(1, 4) if kind == scen.GEN_STAGE_1 else None)
    pool = xt.generate(S, M, K, kind, 7, R, T, target_radius=0.2, robot_pref_speed=30.0, **kw)
    base = tw.generate(S, M, K, [kind], 7, **xt.internal_params(R, T, **kw))
    assert pool["n_failed"] == base["n_failed"] == 0
    assert (pool["n_agents"] == R + T).all()
    # robots fill slots 0..R-1 and nothing else is one
    assert (pool["policy"][:, :R] == scen.POLICY_IGMCTS).all() and (pool["policy"][:, R:] == scen.POLICY_STATIC).all()
    assert (pool["dynamics"][:, :R + T] == scen.DYN_FIRSTORDER).all()
    assert (pool["agents6"][:, :R, 4] == 30.0).all() and (pool["agents6"][:, :R, 5] == 0.5).all()
    assert (pool["agents6"][:, R:R + T, 5] == 0.2).all() and (pool["agents6"][:, R:, 4] == 1.0).all()
    # nothing new is drawn: starts, goals, rectangles and counts are the stage sampler's
    assert np.array_equal(pool["agents6"][:, :, :4], base["agents6"][:, :, :4])
    for k in ("obstacles", "n_obst", "coop", "kind"):
        assert np.array_equal(pool[k], base[k]), k
    assert (pool["n_obst"] > 0).any()
    # every start and goal is 1 m clear of every rectangle, and starts are 1.5 m apart
    for s in range(S):
        rects = pool["obstacles"][s, :pool["n_obst"][s]]
        for i in range(R + T):
            x, y, gx, gy = pool["agents6"][s, i, :4]
            assert tw._clear(rects, x, y) and tw._clear(rects, gx, gy), (s, i)
        p = pool["agents6"][s, :R + T, :2]
        d = np.linalg.norm(p[:, None] - p[None], axis=-1) + 10.0 * np.eye(R + T)
        assert d.min() >= 1.5, s


def test_twin_mixes_both_stage_kinds():
    pool = xt.generate(256, 4, 10, [scen.GEN_STAGE_1, scen.GEN_STAGE_2], 3, 1, 3)
    assert set(np.unique(pool["kind"])) == {scen.GEN_STAGE_1, scen.GEN_STAGE_2}
    assert (pool["policy"][:, 0] == scen.POLICY_IGMCTS).all() and (pool["policy"][:, 1:] == scen.POLICY_STATIC).all()
    assert (pool["n_agents"] == 4).all()


@pytest.mark.parametrize("k", [2, 3, 5])
def test_field_window_rule_leaves_no_regenerated_slot_unbuilt(k):
    """Random finish patterns, lapping included (a world finishing k or more episodes between two refills): after every refill the
    field of every slot is the field of the scenario the slot holds, and the slot of a world's current episode was not written."""
    rng = np.random.default_rng(100 + k)
    N = 13
    book = xt.FieldBook(N, k)
    lapped_seen = False
    for _ in range(300):
        for w in range(N):
            r = rng.random()
            book.finish(w, 0 if r < 0.5 else 1 if r < 0.8 else int(rng.integers(2, 2 * k + 1)))
        before = book.field.copy()
        book.refill()
        assert np.array_equal(book.field, book.held)
        assert np.array_equal(book.field_next, book.next_episode) and np.array_equal(book.next_episode, book.episode + k)
        for w, slot, current in book.touched:
            assert slot != current, (w, slot)
        cur = book.episode % k
        assert np.array_equal(book.field[np.arange(N), cur], before[np.arange(N), cur])  # the current slot's field stays
        assert book.fields_built == book.generated - N * k
        lapped_seen |= book.n_lapped > 0
    assert lapped_seen and book.fields_built > 0


def test_field_window_rule_when_the_team_attaches_late():
    """cagym_ig_init in the middle of a stream: it builds every field and sets field_next = next_episode; refills before it built
    nothing, refills after it build exactly what they regenerate."""
    rng = np.random.default_rng(5)
    N, k = 7, 3
    book = xt.FieldBook(N, k)
    for t in range(60):
        for w in range(N):
            book.finish(w, int(rng.random() < 0.4))
        if t < 20:  # no IG state yet: the refill alone
            fn, fld, built = book.field_next.copy(), book.field.copy(), book.fields_built
            book.refill()
            book.field_next, book.field, book.fields_built = fn, fld, built
            continue
        if t == 20:  # cagym_ig_init
            book.field, book.field_next = book.held.copy(), book.next_episode.copy()
            mark = book.generated
        book.refill()
        assert np.array_equal(book.field, book.held)
    assert book.fields_built == book.generated - mark > 0
