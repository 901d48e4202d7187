"""Whole-env checkpoint and resume of BatchedCollisionAvoidanceEnv (include/cagym.h: cagym_checkpoint_sizes / _save / _load)."""
import ctypes as C

import torch

from . import _lib
from ._consumers import _REC, _RING
from ._snapshot import _SNAP_OUT

_OUT_DTYPES = {"obs_oas": torch.float32, "obs_ego": torch.float32, "obs_laser": torch.float32, "reward": torch.float32,
               "flags": torch.uint8, "game_over": torch.uint8}
_HOST_KEYS = ("n_worlds", "streaming", "pool_policies", "n_ig", "log", "replay")
_SIZES_AT = 8  # the host header starts {magic u32, version u32, sizes u64 [6]} (include/cagym.h)


class EnvCheckpoint(object):
    """What BatchedCollisionAvoidanceEnv.checkpoint() returns and load_checkpoint() takes: `header` (the library's host header, a CPU
    u8 tensor), `blob` (its device sections back to back, a u8 device tensor), `sizes` (cagym_checkpoint_sizes: bytes of the header
    and of the state / pool / stream / log / replay sections), `outputs` (clones of the env-owned output tensors: nothing recomputes
    an observation without stepping, and a policy needs the one the run stopped at) and `host`: what the Python object itself tracks
    - streaming or not, the pool's policy set and IG team size, the log's capacity, the replay's capacity / p / mask."""

    def __init__(self, header, blob, sizes, outputs, host):
        self.header, self.blob, self.sizes, self.outputs, self.host = header, blob, [int(s) for s in sizes], outputs, host

    def state_dict(self):
        """A plain dict of CPU tensors and scalars: torch.save / torch.load of it give checkpoint and resume across processes."""
        return {"header": self.header.clone(), "blob": self.blob.cpu(), "sizes": list(self.sizes),
                "outputs": {k: v.cpu() for k, v in self.outputs.items()}, "host": dict(self.host)}

    @classmethod
    def from_state_dict(cls, d, device):
        """The checkpoint of a state_dict() on `device`.  Everything the library does not check itself is checked here, before
        anything reaches it: the keys, the dtypes, the buffers' lengths against `sizes`, and `sizes` against the header's own."""
        what = "EnvCheckpoint.from_state_dict: "
        missing = [k for k in ("header", "blob", "sizes", "outputs", "host") if k not in d]
        if missing:
            raise ValueError(what + "missing %s" % ", ".join(missing))
        header, blob = d["header"], d["blob"]
        for name, t in (("header", header), ("blob", blob)):
            if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != 1:
                raise ValueError(what + "`%s` must be a one-dimensional uint8 tensor" % name)
        sizes = [int(s) for s in d["sizes"]]
        if len(sizes) != len(_lib.CKPT_SECTIONS) or min(sizes) < 0:
            raise ValueError(what + "`sizes` must hold %d byte counts" % len(_lib.CKPT_SECTIONS))
        if header.numel() != sizes[0] or sizes[0] < _SIZES_AT + 8 * len(sizes):
            raise ValueError(what + "`header` holds %d bytes, `sizes` says %d" % (header.numel(), sizes[0]))
        own = header.cpu()[_SIZES_AT:_SIZES_AT + 8 * len(sizes)].contiguous().view(torch.int64).tolist()
        if own != sizes:
            raise ValueError(what + "`sizes` %s disagrees with the header's own %s" % (sizes, own))
        if blob.numel() != sum(sizes[1:]):
            raise ValueError(what + "`blob` holds %d bytes, the sections add up to %d" % (blob.numel(), sum(sizes[1:])))
        host, outs = d["host"], d["outputs"]
        if not isinstance(host, dict) or [k for k in _HOST_KEYS if k not in host]:
            raise ValueError(what + "`host` must hold %s" % ", ".join(_HOST_KEYS))
        if host["replay"] is not None and sorted(host["replay"]) != ["capacity", "mask", "p"]:
            raise ValueError(what + "`host['replay']` must hold capacity, mask and p")
        if not isinstance(outs, dict) or [k for k in outs if k not in _SNAP_OUT] or [k for k in _SNAP_OUT if k not in outs and k != "obs_laser"]:
            raise ValueError(what + "`outputs` must hold %s" % ", ".join(_SNAP_OUT))
        for k, t in outs.items():
            if not torch.is_tensor(t) or t.dtype != _OUT_DTYPES[k] or t.dim() < 1 or t.shape[0] != int(host["n_worlds"]):
                raise ValueError(what + "`outputs['%s']` must be a %s tensor with one row per world" % (k, _OUT_DTYPES[k]))
        dev = torch.device(device)
        return cls(header.cpu().contiguous(), blob.to(dev).contiguous(), sizes, {k: t.to(dev).contiguous() for k, t in outs.items()}, dict(host))


class _CheckpointMixin(object):
    def checkpoint(self):
        """The whole env as an EnvCheckpoint: state, scenario pool, the stream's ring position and counters, the episode log and
        the replay buffer - the configuration restore() refuses (stream_reference_scenarios + set_stream_params +
        attach_episode_log + attach_replay), and any smaller one, a fixed pool included.  One cagym_checkpoint_save (three copy
        launches on the current stream) plus clones of the output tensors; does not disturb a pending step_begin.  The rasters
        are not stored (12 KB per slot): load_checkpoint() rasterizes the rectangles again.  Refused by the library on an
        exploration stream, with information-gain state, with a trajectory ring or with episode records."""
        sizes = (C.c_uint64 * len(_lib.CKPT_SECTIONS))()
        _lib.call(self.L, self.h, "cagym_checkpoint_sizes", sizes)
        header = torch.zeros((int(sizes[0]),), dtype=torch.uint8)
        blob = torch.empty((sum(int(s) for s in sizes[1:]),), dtype=torch.uint8, device=self.device)
        _lib.call(self.L, self.h, "cagym_checkpoint_save", header.data_ptr(), header.numel(), blob.data_ptr(), blob.numel(), self._stream())
        host = {"n_worlds": self.N, "streaming": bool(self._streaming), "pool_policies": sorted(self._pool_policies), "n_ig": self._n_ig,
                "log": self._log, "replay": None if self._replay is None else dict(self._replay)}
        return EnvCheckpoint(header, blob, list(sizes), {k: v.clone() for k, v in self._outs().items()}, host)

    def load_checkpoint(self, ckpt):
        """Put this env - a fresh one of the same configuration, or the one the checkpoint was taken from - back where
        checkpoint() left it, bit for bit: one cagym_checkpoint_load (the three copies and the raster launch, on the current
        stream), then the output tensors and the Python-side state.  The env streams, logs and replays afterwards exactly as the
        checkpoint's did (a log or replay buffer of another capacity is allocated again; one the checkpoint lacks is cleared
        and detached), and step() / rollout() run the same chain: step(s), log update, harvest, refill.  A pending step_begin is
        void.  The library validates the checkpoint against this env's configuration first and leaves the env untouched when it
        refuses.  Raises RuntimeError with an ig_mcts / ig_greedy planner, a trajectory ring or episode records attached.  An
        attached GA3C policy is stateless and not part of a checkpoint: attach_ga3c() again on a fresh env."""
        if self._igm is not None:
            raise RuntimeError("load_checkpoint() with %s attached: the planner's workspace is not part of a checkpoint; "
                               "detach_ig_mcts() first" % self._igm.kind)
        for c in (_RING, _REC):
            if getattr(self, c.attr) is not None:
                raise RuntimeError("load_checkpoint() with %s attached: it is not part of a checkpoint; %s() first" % (c.noun, c.detach))
        outs = self._outs()
        for k, t in outs.items():
            if k not in ckpt.outputs or ckpt.outputs[k].shape != t.shape or ckpt.outputs[k].dtype != t.dtype:
                raise ValueError("load_checkpoint: the checkpoint's `%s` is not this env's %s %s" % (k, tuple(t.shape), t.dtype))
        blob = ckpt.blob.to(self.device)
        _lib.call(self.L, self.h, "cagym_checkpoint_load", ckpt.header.data_ptr(), ckpt.header.numel(), blob.data_ptr(), blob.numel(),
                  self._stream())
        for k, t in outs.items():
            t.copy_(ckpt.outputs[k])
        host = ckpt.host
        self._streaming, self._pool_policies, self._n_ig = bool(host["streaming"]), set(host["pool_policies"]), host["n_ig"]
        self._log = None if host["log"] is None else int(host["log"])
        self._replay = None if host["replay"] is None else dict(host["replay"])
        self._state = self._stream_views = self._explore_views = self._replay_views = self._log_views = self._rec_views = None
        return self
