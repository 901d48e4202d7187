"""Whole-handle checkpoint (include/cagym.h: cagym_checkpoint_*), the part that needs no device: the header declares the three
entries and _lib.load() gives them prototypes, a null env is refused, and EnvCheckpoint.from_state_dict rejects a dict the library
should never see."""
import ctypes
import importlib
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"cagym_checkpoint_sizes": 2, "cagym_checkpoint_save": 6, "cagym_checkpoint_load": 6}
E_INVALID = -1


def _lib():
    importlib.import_module("gym-exploration-2d_amd.build").build()
    return importlib.import_module("gym-exploration-2d_amd._lib")


def test_header_and_prototype_table_carry_the_checkpoint_entries():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cagym.h")).read(), flags=re.S)
    declared = {n: (0 if p.strip() in ("", "void") else p.count(",") + 1)
                for n, p in re.findall(r"\b(cagym_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src)}
    lib = _lib()
    L = lib.load()
    for name, n_params in ENTRIES.items():
        assert declared.get(name) == n_params, (name, declared.get(name))
        assert len(getattr(L, name).argtypes) == n_params and getattr(L, name).restype is ctypes.c_int, name
    sections = re.search(r"enum\s*\{\s*CAGYM_CKPT_HOST\s*=\s*0(.*?)\}", src, flags=re.S).group(0)
    assert re.findall(r"CAGYM_CKPT_([A-Z]+)\s*=", sections) == [s.upper() for s in lib.CKPT_SECTIONS] + ["SECTIONS"]
    assert "CAGYM_VERSION 112" in src and L.cagym_version() == 112


def test_null_env_is_invalid():
    L = _lib().load()
    sizes = (ctypes.c_uint64 * 6)()
    buf = (ctypes.c_uint8 * 512)()
    assert L.cagym_checkpoint_sizes(None, sizes) == E_INVALID
    assert L.cagym_checkpoint_save(None, buf, 512, buf, 512, None) == E_INVALID
    assert L.cagym_checkpoint_load(None, buf, 512, buf, 512, None) == E_INVALID
    assert b"null env" in L.cagym_last_error(None)


def _state_dict(N=3, M=2, sizes=(160, 64, 32, 0, 16, 0)):
    """A well-formed state dict (of no real env): the header's first words are what the library writes there."""
    header = torch.zeros((sizes[0],), dtype=torch.uint8)
    header[8:8 + 48] = torch.tensor(list(sizes), dtype=torch.int64).view(torch.uint8)
    outs = {"obs_oas": torch.zeros((N, M, M - 1, 10)), "obs_ego": torch.zeros((N, M, 12)), "reward": torch.zeros((N, M)),
            "flags": torch.zeros((N, M), dtype=torch.uint8), "game_over": torch.zeros((N,), dtype=torch.uint8)}
    host = {"n_worlds": N, "streaming": True, "pool_policies": [1, 5], "n_ig": None, "log": 64, "replay": {"capacity": 16, "p": 0.5, "mask": 1}}
    return {"header": header, "blob": torch.zeros((sum(sizes[1:]),), dtype=torch.uint8), "sizes": list(sizes), "outputs": outs, "host": host}


def test_from_state_dict_validates_before_the_library():
    _lib()
    EnvCheckpoint = importlib.import_module("gym-exploration-2d_amd.batched_env").EnvCheckpoint
    good = EnvCheckpoint.from_state_dict(_state_dict(), "cpu")  # (the target device is only a destination: nothing is launched)
    assert good.sizes == [160, 64, 32, 0, 16, 0] and good.blob.numel() == 112 and good.host["log"] == 64

    def broken(edit):
        d = _state_dict()
        edit(d)
        return d

    cases = {
        "missing blob": lambda d: d.pop("blob"),
        "missing host": lambda d: d.pop("host"),
        "missing outputs": lambda d: d.pop("outputs"),
        "missing an output": lambda d: d["outputs"].pop("reward"),
        "missing a host key": lambda d: d["host"].pop("replay"),
        "an unknown output": lambda d: d["outputs"].update(extra=torch.zeros(3)),
        "blob dtype": lambda d: d.update(blob=d["blob"].to(torch.int32)),
        "header dtype": lambda d: d.update(header=d["header"].to(torch.float32)),
        "flags dtype": lambda d: d["outputs"].update(flags=d["outputs"]["flags"].to(torch.float32)),
        "reward dtype": lambda d: d["outputs"].update(reward=d["outputs"]["reward"].to(torch.float64)),
        "output rows": lambda d: d["outputs"].update(game_over=torch.zeros((4,), dtype=torch.uint8)),
        "short blob": lambda d: d.update(blob=d["blob"][:-16]),
        "long blob": lambda d: d.update(blob=torch.zeros((128,), dtype=torch.uint8)),
        "short header": lambda d: d.update(header=d["header"][:-8]),
        "sizes count": lambda d: d.update(sizes=d["sizes"][:5]),
        "sizes against the header": lambda d: d.update(sizes=[160, 64, 16, 16, 16, 0]),
        "replay keys": lambda d: d["host"].update(replay={"capacity": 16}),
    }
    for name, edit in cases.items():
        with pytest.raises(ValueError, match="from_state_dict"):
            EnvCheckpoint.from_state_dict(broken(edit), "cpu")
            pytest.fail("accepted: " + name)
