"""All ranks of a decomposition on ONE device, in one process: every rank gets its DeviceLevel(s) and its native halo plan(s)
(ludwig_halo_plan_create without a communicator, every peer wired to rank 0), and an exchange is: every rank packs
(ludwig_halo_plan_pack), rank r's send segment for peer p is copied device-to-device into p's receive segment for r, every rank unpacks
(ludwig_halo_plan_unpack). The planning is partition.py's, as tests/test_partition_plan.py::_run_partitioned uses it on the CPU; the
descriptors, kernels and buffers are the ones a real multi-GPU run uses. No torch.distributed, no RCCL.

Importing this module needs no device; the HIP runtime is looked up on first use."""
import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np

from open_ludwig_amd import _lib, partition
from open_ludwig_amd.blocks import adapt

GROUPS = partition.FIELD_GROUPS                        # ("f", "vel", "f_post", "rho"): group index of a LudwigHaloPlanDesc
GROUP_COMPONENTS = {"f": 27, "vel": 3, "f_post": 27, "rho": 1}
H2D, D2H, D2D = 1, 2, 3                                # hipMemcpyKind

_hip = None


def hip():
    """the HIP runtime libludwig_hip.so itself loaded (the plan's buffers are raw device pointers of that runtime)"""
    global _hip
    if _hip is not None:
        return _hip
    _lib.load()
    # (a PyTorch in the process brings a second, private copy of the runtime: not that one)
    names = [l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l and "/" in l and "/torch/" not in l][:1]
    names += ["libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6"]
    for name in names:
        try:
            h = C.CDLL(name)
            break
        except OSError:
            continue
    else:
        raise RuntimeError("HIP runtime not loadable through ctypes")
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipMemcpy.restype = C.c_int
    h.hipDeviceSynchronize.argtypes = []
    h.hipDeviceSynchronize.restype = C.c_int
    _hip = h
    return h


def device_sync() -> None:
    assert hip().hipDeviceSynchronize() == 0


def memcpy(dst: int, src: int, nbytes: int, kind: int) -> None:
    if nbytes:
        assert hip().hipMemcpy(C.c_void_p(dst), C.c_void_p(src), nbytes, kind) == 0


def create_plan(level, peer_ranks: Sequence[int], send: Dict[str, List[np.ndarray]], recv: Dict[str, List[np.ndarray]], comm=None,
                send_count: Optional[Dict[str, Sequence[int]]] = None, recv_count: Optional[Dict[str, Sequence[int]]] = None,
                null_index: Sequence[str] = ()):
    """ludwig_halo_plan_create from per-group, per-peer offset lists (a group that is missing is empty: NULL counts).
    send_count / recv_count override the counts handed over (error paths); null_index: groups whose send index pointer is NULL
    although counts are given. Returns (return code, handle) - the handle a ctypes.c_void_p that held a non-null value before the call."""
    lib = _lib.load()
    n = len(peer_ranks)
    peers = np.asarray(peer_ranks, dtype=np.int32)
    d = _lib.HaloPlanDesc()
    d.n_peers = n
    d.peer_ranks = peers.ctypes.data if n else None
    keep = [peers]
    for gi, name in enumerate(GROUPS):
        for side, lists, counts, c_arr, i_arr in (("send", send, send_count, d.send_count, d.send_index), ("recv", recv, recv_count, d.recv_count, d.recv_index)):
            if name not in lists and not (counts and name in counts):
                continue
            ls = [np.asarray(a, dtype=np.int64) for a in lists.get(name, [np.zeros(0, np.int64)] * n)]
            assert len(ls) == n
            cnt = np.asarray(counts[name] if counts and name in counts else [a.size for a in ls], dtype=np.int64)
            idx = np.ascontiguousarray(np.concatenate(ls) if ls else np.zeros(0, np.int64), dtype=np.int64)
            keep += [cnt, idx]
            c_arr[gi] = cnt.ctypes.data if n else None
            i_arr[gi] = None if (side == "send" and name in null_index) or idx.size == 0 else idx.ctypes.data
    h = C.c_void_p(0xDEAD0)                            # the library must overwrite it, with NULL when it fails
    rc = lib.ludwig_halo_plan_create(level.handle, comm, C.byref(d), C.byref(h))
    del keep
    return rc, h


class PlanHandle:
    """the pack / unpack halves and the message buffers of a LudwigHaloPlan (a handle from create_plan or of a partition.NativeHalo)"""

    def __init__(self, handle, level, owns: bool = True):
        self.h, self.level, self.owns = handle, level, owns
        self.lib = _lib.load()

    def pack(self, group: str, field: str) -> int:
        return self.lib.ludwig_halo_plan_pack(self.h, GROUPS.index(group), _lib.FIELD_NAMES[field], None)

    def unpack(self, group: str, field: str) -> int:
        return self.lib.ludwig_halo_plan_unpack(self.h, GROUPS.index(group), _lib.FIELD_NAMES[field], None)

    def buffers(self, group: str):
        """(send pointer, n_send, receive pointer, n_recv); a pointer is None where the side is empty"""
        s, r, ns, nr = C.c_void_p(), C.c_void_p(), C.c_int64(-1), C.c_int64(-1)
        _lib.check(self.lib.ludwig_halo_plan_buffers(self.h, GROUPS.index(group), C.byref(s), C.byref(ns), C.byref(r), C.byref(nr)))
        return s.value, int(ns.value), r.value, int(nr.value)

    def read_send(self, group: str) -> np.ndarray:
        """the send buffer's words, once everything queued on the level's stream has run"""
        s, ns, _, _ = self.buffers(group)
        out = np.empty(ns, dtype=np.uint32)
        self.level.synchronize()
        memcpy(out.ctypes.data, s, out.nbytes, D2H)
        return out

    def write_recv(self, group: str, words: np.ndarray) -> None:
        _, _, r, nr = self.buffers(group)
        words = np.ascontiguousarray(words, dtype=np.uint32)
        assert words.size == nr
        memcpy(r, words.ctypes.data, words.nbytes, H2D)

    def close(self) -> None:
        if self.h and self.owns:
            self.lib.ludwig_halo_plan_destroy(self.h)
        self.h = None


def segments(plan: partition.HaloPlan, group: str, side: str) -> Dict[int, tuple]:
    """peer -> (first element, count) of its part of the concatenated message buffer"""
    lists = plan.send if side == "send" else plan.recv
    out, at = {}, 0
    for p in plan.peers:
        n = int(len(lists[p][group]))
        out[p] = (at, n)
        at += n
    return out


class RankLevel:
    """one rank's copy of one level: the view, the plan, the device level and the native plan (None where the rank holds no block)"""

    def __init__(self, view: partition.LocalView, plan: partition.HaloPlan, upload_state: bool = True):
        self.view, self.plan = view, plan
        partition.name_post_collision_readers(view.level, plan)
        self.level = adapt(view.level, 0, upload_state) if view.level.n_blocks > 0 else None
        self.native = self.handle = None
        if self.level is not None:
            self.native = partition.NativeHalo(plan, self.level, None, {p: 0 for p in plan.peers})
            self.handle = PlanHandle(self.native.handle, self.level, owns=False)

    def close(self) -> None:
        if self.native is not None:
            self.native.close()
        if self.level is not None:
            self.level.close()
        self.native = self.handle = self.level = None


def _plans(views: List[partition.LocalView], n_global: int, needs: List[Optional[Dict[str, np.ndarray]]]) -> List[partition.HaloPlan]:
    world = len(views)
    reqs = [partition.make_requests(v, n_global, needs[r]) for r, v in enumerate(views)]
    return [partition.build_plan(v, n_global, reqs[r], {q: reqs[q][r] for q in range(world) if r in reqs[q]}) for r, v in enumerate(views)]


def exchange(ranks: List[RankLevel], fields: Dict[str, str]) -> None:
    """one exchange of the named groups (group -> field of the level) among the ranks' copies of ONE level"""
    live = [r for r in ranks if r.handle is not None]
    for r in live:
        for g, f in fields.items():
            _lib.check(r.handle.pack(g, f))
    device_sync()
    for g in fields:
        for r in live:
            send_seg = segments(r.plan, g, "send")
            s_ptr = r.handle.buffers(g)[0]
            for p in r.plan.peers:
                a, n = send_seg[p]
                if n == 0:
                    continue
                peer = ranks[p]
                b, m = segments(peer.plan, g, "recv")[r.view.rank]
                assert m == n, f"rank {r.view.rank} sends {n} elements of {g} to {p}, which expects {m}"
                memcpy(peer.handle.buffers(g)[2] + 4 * b, s_ptr + 4 * a, 4 * n, D2D)
    device_sync()
    for r in live:
        for g, f in fields.items():
            _lib.check(r.handle.unpack(g, f))
    device_sync()


class SingleLevelWorld:
    """a populated global level cut by an owner map: build_local_level / slice_level_fields for every rank, every rank's make_requests
    handed over in-process, build_plan, a DeviceLevel and a native plan each. extra_needs(view, needs) may add to a rank's needs."""

    def __init__(self, global_level, owner: np.ndarray, params, extra_needs=None):
        self.params, self.world, self.n_global = params, int(np.max(owner)) + 1, global_level.n_blocks
        views, needs = [], []
        for r in range(self.world):
            v = partition.build_local_level(global_level.level_id, global_level.active_block_coords, global_level.neighbor_table, owner, r,
                                            float(global_level.tau), temporal=global_level.f_old.size > 27)
            partition.slice_level_fields(v, global_level)
            n = partition.compute_needs(v)
            if extra_needs is not None:
                extra_needs(v, n)
            views.append(v)
            needs.append(n)
        self.ranks = [RankLevel(v, p) for v, p in zip(views, _plans(views, self.n_global, needs))]

    def exchange(self, fields: Dict[str, str]) -> None:
        exchange(self.ranks, fields)

    def step(self, t: int, u_curr=0.0) -> None:
        """the non-overlap schedule of partition.DistributedLevelRunner.step: stream-collide everywhere, f_post exchange, Bouzidi
        correction, f / vel exchange"""
        from open_ludwig_amd.physics import apply_bouzidi_correction, stream_collide
        for r in self.ranks:
            stream_collide(r.level, None, np.float32(0.5), u_curr, self.params, t, part=_lib.PART_ALL)
        if any(r.plan.has("f_post") for r in self.ranks):
            self.exchange({"f_post": "f_post_collision"})
        for r in self.ranks:
            if r.level.has_post_collision:
                apply_bouzidi_correction(r.level, t, self.params.q_min_threshold)
        self.exchange({"f": "f_temp", "vel": "vel_temp"} if t % 2 == 0 else {"f": "f", "vel": "vel"})

    def close(self) -> None:
        device_sync()
        for r in self.ranks:
            r.close()


class NestedWorld:
    """nested levels, every level with an owner map of its own: views, needs and plans as partition.MultiLevelRunner builds them - a
    level's ghosts include the parent blocks this rank's finer blocks interpolate from (required_parent_blocks), its needs are the
    same-level needs plus interpolation_needs. levels[i][r] is rank r's copy of level i; same_level[i][r] / parent_data[i][r] are the
    two kinds of needs (local offsets) the plan was built from."""

    def __init__(self, grids, owners: List[np.ndarray], params, world: int, upload_state: bool = True):
        dims = (params.domain_nx, params.domain_ny, params.domain_nz)
        self.world, self.grids = world, grids
        views = [[None] * world for _ in grids]
        for r in range(world):
            for i in range(len(grids) - 1, -1, -1):
                g = grids[i]
                extra = None
                if i + 1 < len(grids):
                    extra = partition.required_parent_blocks(grids[i + 1], np.flatnonzero(np.asarray(owners[i + 1]) == r), g)
                v = partition.build_local_level(g.level_id, g.active_block_coords, g.neighbor_table, owners[i], r, float(g.tau),
                                                temporal=g.f_old.size > 27, extra_ghosts=extra)
                partition.slice_level_fields(v, g, state=upload_state)
                views[i][r] = v
        empty = lambda: np.zeros(0, np.int64)
        self.same_level, self.parent_data, self.levels = [], [], []
        for i, g in enumerate(grids):
            same, parent, needs = [], [], []
            for r in range(world):
                v = views[i][r]
                s = partition.compute_needs(v) if v.n_owned > 0 else {}
                s = {name: s.get(name, empty()) for name in GROUPS}
                p = {name: empty() for name in GROUPS}
                if i + 1 < len(grids) and views[i + 1][r].n_owned > 0:
                    p.update(partition.interpolation_needs(views[i + 1][r], v, dims))
                same.append(s)
                parent.append(p)
                needs.append({name: np.unique(np.concatenate([s[name], p[name]])) for name in GROUPS})
            plans = _plans(views[i], g.n_blocks, needs)
            self.same_level.append(same)
            self.parent_data.append(parent)
            self.levels.append([RankLevel(v, pl, upload_state) for v, pl in zip(views[i], plans)])

    def close(self) -> None:
        device_sync()
        for ranks in self.levels:
            for r in ranks:
                r.close()
