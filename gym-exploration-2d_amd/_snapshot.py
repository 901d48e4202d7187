"""Per-world snapshot, restore and fork of BatchedCollisionAvoidanceEnv (include/cagym.h: cagym_snapshot / _restore / _fork)."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._consumers import _LOG, _RING

_SNAP_OUT = ("obs_oas", "obs_ego", "obs_laser", "reward", "flags", "game_over")  # the env-owned output tensors a snapshot carries rows of


class EnvSnapshot(object):
    """What BatchedCollisionAvoidanceEnv.snapshot() returns and restore() takes: `layout` (cagym_snapshot_layout), `blob`
    [n, row_bytes] u8 on the device (cagym_snapshot's rows), `worlds` [n] i32 device tensor of the origin world ids, and
    `outputs`: clones of the same worlds' rows of the env's output tensors - nothing in the C ABI recomputes an observation
    without stepping, and a policy needs the restored state's observation.  The scenario pool is not part of it."""

    def __init__(self, layout, blob, worlds, outputs, all_worlds=False, trusted=True):
        self.layout, self.blob, self.worlds, self.outputs = layout, blob, worlds, outputs
        self.all_worlds = bool(all_worlds)  # rows 0..N-1 are worlds 0..N-1 (snapshot() without a list)
        self.trusted = bool(trusted)        # the world ids were validated on the host
        self.n = int(blob.shape[0])

    def state_dict(self):
        """A plain dict of CPU tensors and ints: torch.save / torch.load of it give checkpoint and resume."""
        return {"layout": {k: int(getattr(self.layout, k)) for k, _ in _lib.CagymSnapshotLayout._fields_},
                "blob": self.blob.cpu(), "worlds": self.worlds.cpu(), "all_worlds": self.all_worlds,
                "outputs": {k: v.cpu() for k, v in self.outputs.items()}}

    @classmethod
    def from_state_dict(cls, d, device):
        layout = _lib.CagymSnapshotLayout(**{k: int(v) for k, v in d["layout"].items()})
        worlds = torch.as_tensor(d["worlds"]).to(torch.int32).reshape(-1)
        ids = worlds.numpy()
        if ids.size != int(d["blob"].shape[0]) or (ids.size and (ids.min() < 0 or ids.max() >= layout.n_worlds)) or np.unique(ids).size != ids.size:
            raise ValueError("EnvSnapshot.from_state_dict: `worlds` must name one distinct world of [0, %d) per blob row" % layout.n_worlds)
        dev = torch.device(device)
        return cls(layout, torch.as_tensor(d["blob"]).to(torch.uint8).to(dev).contiguous(), worlds.to(dev),
                   {k: torch.as_tensor(v).to(dev).contiguous() for k, v in d["outputs"].items()}, d.get("all_worlds", False), True)


class _SnapshotMixin(object):
    def _id_list(self, ids, what, check, limit, distinct=True):
        """A world / row list (sequence, numpy array or tensor) as (contiguous i32 device tensor, host int64 array or None).
        Data that arrives on the host is validated there; a device tensor is read back (ONE synchronisation) unless
        check=False - then nothing is known on the host, and the kernel's bounds guard and _row_map's masks take over."""
        if torch.is_tensor(ids) and ids.is_cuda:
            t = ids.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
            if not check:
                return t, None
            host = t.cpu().numpy().astype(np.int64)
        else:
            host = np.asarray(ids.cpu() if torch.is_tensor(ids) else ids).astype(np.int64).reshape(-1)
            t = torch.as_tensor(host.astype(np.int32), device=self.device)
        if host.size and (host.min() < 0 or host.max() >= limit):
            raise ValueError("%s: ids must lie in [0, %d), got %d..%d" % (what, limit, host.min(), host.max()))
        if distinct and np.unique(host).size != host.size:
            raise ValueError("%s: the ids must be distinct" % what)
        return t, host

    def _outs(self):
        return {k: getattr(self, k) for k in _SNAP_OUT if getattr(self, k) is not None}

    def _row_map(self, dst, valid):
        """For lists the host could not validate (valid: bool [n] device mask of the usable entries, None: validated): world ->
        (row of the list that writes it, whether one does), through an inverse map with one spare slot for the skipped
        entries - no synchronisation, and an id out of range never indexes a tensor."""
        if valid is None or dst.shape[0] == 0:
            return None
        N = self.N
        inv = torch.full((N + 1,), -1, dtype=torch.long, device=self.device)
        inv.index_copy_(0, torch.where(valid, dst, torch.full_like(dst, N)), torch.arange(dst.shape[0], device=self.device))
        return inv[:N].clamp(min=0), inv[:N] >= 0

    @staticmethod
    def _put_rows(t, dst, vals, mapped):
        """t[dst[r]] = vals[r]; mapped: _row_map's pair for an unvalidated dst, else None."""
        if dst.shape[0] == 0:
            return
        if mapped is None:
            t.index_copy_(0, dst, vals)
            return
        row, has = mapped
        t.copy_(torch.where(has.view((-1,) + (1,) * (t.dim() - 1)), vals.index_select(0, row), t))

    def snapshot_layout(self):
        L = _lib.CagymSnapshotLayout()
        _lib.call(self.L, self.h, "cagym_snapshot_layout_of", C.byref(L))
        return L

    def snapshot(self, worlds=None, check=True):
        """The state of the listed worlds (default: all) as an EnvSnapshot: ONE cagym_snapshot launch on the current stream plus
        clones of those worlds' rows of the output tensors.  Everything a world carries from step to step is in it (after
        cagym_ig_init the belief too), except an attached planner's workspace and the scenario pool.  Does not disturb a
        pending step_begin.  worlds: distinct ids; a device tensor is validated with one synchronisation unless check=False."""
        L = self.snapshot_layout()
        if worlds is None:
            blob = torch.empty((self.N, int(L.row_bytes)), dtype=torch.uint8, device=self.device)
            _lib.call(self.L, self.h, "cagym_snapshot", None, self.N, blob.data_ptr(), self._stream())
            return EnvSnapshot(L, blob, torch.arange(self.N, dtype=torch.int32, device=self.device),
                               {k: v.clone() for k, v in self._outs().items()}, True, True)
        ids, host = self._id_list(worlds, "snapshot(worlds)", check, self.N)
        # rows of ids the kernel skips must not look like rows: zeros carry no magic
        blob = (torch.empty if host is not None else torch.zeros)((ids.numel(), int(L.row_bytes)), dtype=torch.uint8, device=self.device)
        _lib.call(self.L, self.h, "cagym_snapshot", ids.data_ptr(), ids.numel(), blob.data_ptr(), self._stream())
        pick = ids.long() if host is not None else ids.long().clamp(0, self.N - 1)
        return EnvSnapshot(L, blob, ids, {k: v.index_select(0, pick) for k, v in self._outs().items()}, False, host is not None)

    def _refuse_new_timeline(self, what, why_streaming):
        """restore() and fork() put worlds on another timeline: what cannot follow them there refuses, in this order."""
        if self._igm is not None:
            raise RuntimeError("%s() with %s attached: the planner's workspace, its published plans and the host-side call counter are "
                               "not part of a snapshot; detach_ig_mcts() first" % (what, self._igm.kind))
        for c in (_LOG, _RING):
            if getattr(self, c.attr) is not None:
                raise RuntimeError("%s() with %s attached: %s" % (what, c.noun, c.timeline))
        self._refuse_streaming(what, why_streaming)

    def restore(self, snap, rows=None, check=True):
        """Put the rows of an EnvSnapshot (default: all; else distinct row indices into it) back, each into its origin world:
        ONE cagym_restore launch, then the same worlds' output rows.  A pending step_begin is void afterwards.  The snapshot
        may come from another handle of the same shape (resume): install the same scenario pool first.  Refused while an
        ig_mcts / ig_greedy planner is attached, while the env streams scenarios, and by the library while episode records are
        initialised."""
        self._refuse_new_timeline("restore", "the ring of scenario slots is not part of a snapshot (a restored episode index would meet "
                                  "other scenarios)")
        valid = None
        if rows is None and snap.all_worlds:  # whole tensors, and nothing allocated: the form a graph capture takes
            _lib.call(self.L, self.h, "cagym_restore", C.byref(snap.layout), snap.blob.data_ptr(), None, snap.n, self._stream())
            for k, t in self._outs().items():
                t.copy_(snap.outputs[k])
            return
        if rows is None:
            r, n, dst, vals = None, snap.n, snap.worlds.long(), snap.outputs
        else:
            r, host = self._id_list(rows, "restore(rows)", check, snap.n)
            n = r.numel()
            if host is None:  # nothing known on the host: rows outside the blob become -1, which the kernel skips
                valid = (r >= 0) & (r < snap.n)
                r = torch.where(valid, r, torch.full_like(r, -1))
            pick = r.long().clamp(0, max(snap.n - 1, 0))
            dst = snap.worlds.long().index_select(0, pick) if snap.n else snap.worlds.long()
            vals = {k: v.index_select(0, pick) for k, v in snap.outputs.items()} if snap.n else snap.outputs
        if not snap.trusted:
            in_range = (dst >= 0) & (dst < self.N)
            valid = in_range if valid is None else valid & in_range
        _lib.call(self.L, self.h, "cagym_restore", C.byref(snap.layout), snap.blob.data_ptr(), _lib.ptr(r), n, self._stream())
        mapped = self._row_map(dst, valid)
        for k, t in self._outs().items():
            self._put_rows(t, dst, vals[k], mapped)

    def fork(self, src, dst, check=True):
        """World dst[r] continues as a copy of world src[r]: cagym_fork (state rows except dst's own episode index and stat_*, and
        the pool rows of src's current scenario slot over dst's), then the same copy of the output rows.  dst ids are distinct
        and none is also a src.  Needs n_scenarios % n_worlds == 0; refused while a planner is attached, while the env streams
        scenarios, on handles with information-gain state and while episode records are initialised.  A pending step_begin is void
        afterwards."""
        self._refuse_new_timeline("fork", "the ring of scenario slots is not part of a snapshot, and a refill would overwrite the forked slot")
        s, hs = self._id_list(src, "fork(src)", check, self.N, distinct=False)
        d, hd = self._id_list(dst, "fork(dst)", check, self.N)
        if s.numel() != d.numel():
            raise ValueError("fork: src and dst must have the same length (%d, %d)" % (s.numel(), d.numel()))
        if hs is not None and hd is not None and np.intersect1d(hs, hd).size:
            raise ValueError("fork: a world is both src and dst: %s" % np.intersect1d(hs, hd).tolist())
        _lib.call(self.L, self.h, "cagym_fork", s.data_ptr(), d.data_ptr(), s.numel(), self._stream())
        valid = None
        if hs is None or hd is None:
            valid = (s >= 0) & (s < self.N) & (d >= 0) & (d < self.N)
        pick, to = s.long().clamp(0, self.N - 1), d.long()
        mapped = self._row_map(to, valid)
        for t in self._outs().values():
            self._put_rows(t, to, t.index_select(0, pick), mapped)
