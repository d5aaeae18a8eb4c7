"""The native halo plan - build_octets, k_pack_octets / k_unpack_octets, ludwig_halo_plan_create / _pack / _unpack / _buffers - on ONE
device against a plain numpy gather / scatter (tests/_halo_ref.py), bit for bit.

Part A: constructed index lists on one small level. How the library sees a list (ludwig_hip.hip build_octets, kernels.hpp): an element
of the reference layout becomes element (block' K + k) 512 + cell of the device array (block' = the library's own block order); 8
consecutive such elements - 8 x-neighbours of one row - are one 32-byte sector ("octet"); consecutive list entries that stay in one
sector with ascending members share a descriptor (sector, message position of the first member, member mask); a descriptor with 1 or
2 members is dissolved into a second list of single elements. The cases below are chosen from that: which masks occur, where a
descriptor has to end, what sits on both sides of a peer boundary, which side of a group is empty.

Part B: whole decompositions with all ranks in this process (tests/_inprocess_world.py): ragged cuts, Bouzidi links across a cut,
parent-data ghosts of nested levels, the rho group behind the lazy rho store.

Every comparison is of 32-bit words; there is no tolerance in this file. What it cannot see: WHICH of the two lists a 1- or 2-member
sector went to (the threshold between them changes the thread count, never a value), and the wire between two devices."""
import ctypes as C
import os

import numpy as np
import pytest

import _halo_ref as ref
import _inprocess_world as ipw
from open_ludwig_amd import _lib, cases, partition
from open_ludwig_amd.blocks import adapt

GROUPS = ipw.GROUPS
K_OF = ipw.GROUP_COMPONENTS
GROUP_FIELDS = {"f": ("f", "f_temp"), "vel": ("vel", "vel_temp"), "f_post": ("f_post_collision",), "rho": ("rho",)}
ORDER_SWITCH = "LUDWIG_REFERENCE_BLOCK_ORDER"


def same_bits(a, b) -> bool:
    return a.shape == b.shape and np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------
# Part A: the index lists
# ---------------------------------------------------------------------------------------------------------------------------
def _cell(x, y, z):
    return np.sort((np.asarray(x) + 8 * np.asarray(y) + 64 * np.asarray(z)).reshape(-1))


_Y, _Z = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
X_FACE_LO, X_FACE_HI = _cell(0, _Y, _Z), _cell(7, _Y, _Z)            # single cells 32 B apart: every sector has one member
Y_FACE_LO, Y_FACE_HI = _cell(_Y, 0, _Z), _cell(_Y, 7, _Z)            # rows of 8: full sectors
Z_FACE_LO, Z_FACE_HI = _cell(_Y, _Z, 0), _cell(_Y, _Z, 7)            # whole planes
# sector (row of a block) -> members: 1, 2, 3, 7 and 8 of them, with and without holes
SECTORS = {0: [4], 1: [1, 6], 2: [0, 3, 7], 3: [2, 3, 4], 4: [0, 1, 2, 3, 4, 6, 7], 5: list(range(8)), 6: [0, 7], 7: [7], 8: [0],
           9: [0, 1, 2, 3, 4, 5, 6], 10: [3, 4], 11: [1, 2, 3, 4, 5, 6, 7]}
SECTOR_CELLS = np.array([8 * s + m for s, ms in SECTORS.items() for m in ms])


def _lists(K, nb):
    """E(k, b, cells): offsets of component k (modulo K) of block b; cat: one list out of several"""
    E = lambda k, b, c: ref.offset(nb, np.asarray(k) % K, b, c).reshape(-1)
    return E, lambda *ls: np.concatenate(ls)


def case_x_face(K, nb, gi):
    E, cat = _lists(K, nb)
    comps = sorted({0, K - 1})
    return [cat(*[E(k, 1, X_FACE_LO) for k in comps])], [cat(*[E(k, nb - 2, X_FACE_HI) for k in comps])]


def case_y_face(K, nb, gi):
    E, cat = _lists(K, nb)
    comps = sorted({1 % K, K - 1})
    return [cat(*[E(k, 3, Y_FACE_LO) for k in comps])], [cat(*[E(k, 4, Y_FACE_HI) for k in comps])]


def case_z_face(K, nb, gi):
    E, cat = _lists(K, nb)
    return [cat(E(K // 2, 5, Z_FACE_HI), E(K - 1, nb - 1, Z_FACE_HI))], [cat(E(K // 2, 6, Z_FACE_LO), E(0, 0, Z_FACE_LO))]


def case_sector_members(K, nb, gi):
    E, _ = _lists(K, nb)
    return [E(K // 2, 2, SECTOR_CELLS)], [E(K // 2 + 1, 9, SECTOR_CELLS)]


def case_run_across_sectors(K, nb, gi):
    """5 .. 10 crosses 7|8; 14 .. 17 comes back to the sector 8 .. 15 after a gap (same descriptor goes on) and crosses 15|16"""
    E, cat = _lists(K, nb)
    run = np.concatenate([np.arange(5, 11), np.arange(14, 18)])
    return [E(1, 7, run)], [E(0, 3, run + 64)]


def case_run_across_blocks(K, nb, gi):
    """consecutive offsets over 511|0: into the next block of the reference order, and from the last block into the next component"""
    E, cat = _lists(K, nb)
    a = E(K - 1, 4, 509) + np.arange(6)
    b = E(0, nb - 1, 508) + np.arange(4 if K == 1 else 9)
    c = E(0, 8, 509) + np.arange(6)
    d = E(K - 2 if K > 1 else 0, nb - 1, 510) + np.arange(2 if K == 1 else 7)
    return [cat(b, a)], [cat(c, d)]


def case_descending(K, nb, gi):
    E, cat = _lists(K, nb)
    return [cat(E(0, 2, SECTOR_CELLS), E(2, 5, Z_FACE_HI))[::-1].copy()], [cat(E(0, 6, Y_FACE_LO), E(1, 9, SECTOR_CELLS))[::-1].copy()]


def case_shuffled(K, nb, gi):
    E, cat = _lists(K, nb)
    rng = np.random.default_rng(100 + gi)
    s = cat(E(0, 3, Y_FACE_LO), E(K - 1, 2, SECTOR_CELLS), E(1, 1, X_FACE_LO))
    r = cat(E(0, 4, Y_FACE_HI), E(K - 1, 9, SECTOR_CELLS), E(1, 10, X_FACE_HI))
    return [rng.permutation(s)], [rng.permutation(r)]


def case_one_inversion(K, nb, gi):
    """ascending but for members 3 and 4 of one sector: that sector needs two descriptors, its neighbours one each"""
    E, _ = _lists(K, nb)
    cells = np.array(list(range(24, 32)) + [32, 33, 34, 36, 35, 37, 38, 39] + list(range(40, 48)))
    return [E(0, 6, cells)], [E(K - 1, 7, cells + 128)]


def case_same_element_adjacent(K, nb, gi):
    """an element that ends one peer's list and starts the next one's: inside a sector of many members (11) and as a lone one (40)"""
    E, _ = _lists(K, nb)
    s = [E(1, 5, [8, 9, 10, 11]), E(1, 5, [11, 12, 13, 14]), E(0, 5, [40]), E(0, 5, [40, 41])]
    r = [E(1, 6, [8, 9, 10, 11]), E(1, 7, [11, 12, 13, 14]), E(0, 6, [40]), E(0, 7, [40, 41])]
    return s, r


def case_same_element_far(K, nb, gi):
    E, cat = _lists(K, nb)
    s = [cat(E(0, 4, np.arange(16, 24)), E(K - 1, 1, SECTOR_CELLS)), cat(E(0, 5, np.arange(8)), E(0, 4, [18, 19, 20]), E(K - 1, 1, [16]))]
    r = [cat(E(0, 8, np.arange(16, 24)), E(K - 1, 3, SECTOR_CELLS)), cat(E(0, 9, np.arange(8)), E(0, 10, [18, 19, 20]), E(K - 1, 11, [17]))]
    return s, r


def case_peers_some_empty(K, nb, gi):
    """four peers; in group gi peer p has both sides, nothing, a send side only, a receive side only - by (p + gi) % 4"""
    E, _ = _lists(K, nb)
    s, r = [], []
    for p in range(4):
        role = (p + gi) % 4
        s.append(E(p, p, SECTOR_CELLS[: 5 + 3 * p]) if role in (0, 2) else np.zeros(0, np.int64))
        r.append(E(p + 1, nb - 1 - p, Y_FACE_LO[: 4 + 5 * p]) if role in (0, 3) else np.zeros(0, np.int64))
    return s, r


def case_one_element(K, nb, gi):
    E, _ = _lists(K, nb)
    return [E(K // 2, 5, [77])], [E(0, 6, [300])]


def case_first_and_last_element(K, nb, gi):
    last = ref.n_elements(nb, K) - 1                     # last component, last block, cell 511
    return [np.array([0]), np.array([last])], [np.array([last]), np.array([0])]


def case_send_only(K, nb, gi):
    E, _ = _lists(K, nb)
    return [E(0, 3, Y_FACE_LO)], [np.zeros(0, np.int64)]


def case_recv_only(K, nb, gi):
    E, _ = _lists(K, nb)
    return [np.zeros(0, np.int64)], [E(K - 1, 4, SECTOR_CELLS)]


def case_all_groups_empty(K, nb, gi):
    return [np.zeros(0, np.int64)] * 2, [np.zeros(0, np.int64)] * 2


def case_no_peers(K, nb, gi):
    return [], []


def case_per_direction(K, nb, gi):
    """another cell set for every component, as the f_post list of Bouzidi links has (sorted within a component, as compute_needs makes it)"""
    E, cat = _lists(K, nb)
    rng = np.random.default_rng(7 + gi)
    s = cat(*[E(k, k % nb, np.sort(rng.choice(512, size=20 + k, replace=False))) for k in range(K)])
    r = cat(*[E(k, (k + 5) % nb, np.sort(rng.choice(512, size=9 + 2 * k, replace=False))) for k in range(K)])
    return [s], [r]


CASES = {f.__name__[5:]: f for f in (
    case_x_face, case_y_face, case_z_face, case_sector_members, case_run_across_sectors, case_run_across_blocks, case_descending,
    case_shuffled, case_one_inversion, case_same_element_adjacent, case_same_element_far, case_peers_some_empty, case_one_element,
    case_first_and_last_element, case_send_only, case_recv_only, case_all_groups_empty, case_no_peers, case_per_direction)}


@pytest.fixture(scope="module")
def levels(gpu):
    """one 3 x 2 x 2 tunnel level with a body (so that f_post_collision exists), once in the library's own block order and once
    created under LUDWIG_REFERENCE_BLOCK_ORDER (read when the level is created)"""
    grids, _ = cases.tunnel_with_sphere((3, 2, 2), levels=1, temporal=False)
    host = grids[0]
    assert host.n_blocks == 12 and host.n_boundary_cells > 0
    saved = os.environ.pop(ORDER_SWITCH, None)
    out = {}
    try:
        out["internal"] = adapt(host, 0)
        os.environ[ORDER_SWITCH] = "1"
        out["reference"] = adapt(host, 0)
    finally:
        os.environ.pop(ORDER_SWITCH, None)
        if saved is not None:
            os.environ[ORDER_SWITCH] = saved
    assert np.array_equal(out["reference"].block_order(), np.arange(12))
    assert not np.array_equal(out["internal"].block_order(), np.arange(12)), "the two levels share one block order"
    assert all(lv.has_post_collision for lv in out.values())
    yield out
    for lv in out.values():
        lv.close()


def gather_with_k_gather(lvl, field: str, index: np.ndarray) -> np.ndarray:
    """the same message through the other kernel family: ludwig_halo_pack (k_gather), which takes the index list as it is"""
    import torch
    idx = torch.as_tensor(np.ascontiguousarray(index, dtype=np.int64), device="cuda:0")
    out = torch.empty(idx.numel(), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    _lib.check(_lib.load().ludwig_halo_pack(lvl.handle, _lib.FIELD_NAMES[field], C.c_void_p(idx.data_ptr()), idx.numel(),
                                            C.c_void_p(out.data_ptr()), None))
    lvl.synchronize()
    return out.cpu().numpy().view(np.uint32)


def check_group(lvl, plan, group: str, field: str, send_index: np.ndarray, recv_index: np.ndarray, seed: int) -> None:
    """pack and unpack of one group with one field against the reference, with a random fill and with the offset fill"""
    K, nb = K_OF[group], lvl.n_blocks
    n = ref.n_elements(nb, K)
    s_ptr, n_send, r_ptr, n_recv = plan.buffers(group)
    assert (n_send, n_recv) == (send_index.size, recv_index.size)
    assert (s_ptr is None) == (n_send == 0) and (r_ptr is None) == (n_recv == 0)
    for fill, words in (("random", ref.random_words(n, seed)), ("offsets", ref.offset_words(n, 1 + GROUPS.index(group)))):
        what = f"{group} / {field}, {fill} fill"
        lvl.upload(field, ref.as_field(words, nb, K))
        _lib.check(plan.pack(group, field))
        sent = plan.read_send(group)
        want = ref.pack(words, send_index)
        assert np.array_equal(sent, want), f"send buffer, {what}: {ref.first_difference(sent, want)}"
        if n_send:
            other = gather_with_k_gather(lvl, field, send_index)
            assert np.array_equal(other, want), f"ludwig_halo_pack, {what}: {ref.first_difference(other, want)}"
        assert np.array_equal(ref.bits(lvl.download(field)), words), f"pack changed the field, {what}"
        message = ref.random_words(n_recv, seed + 1) if fill == "random" else ref.offset_words(n_recv, 15)
        plan.write_recv(group, message)
        _lib.check(plan.unpack(group, field))
        lvl.synchronize()
        got = ref.bits(lvl.download(field))
        want = ref.unpack(words, recv_index, message)
        # the whole field: the listed elements hold the message, every other element is unchanged bit for bit
        assert np.array_equal(got, want), f"field after unpack, {what}: {ref.first_difference(got, want)}"


def build_case(name: str, nb: int):
    send, recv = {}, {}
    for gi, g in enumerate(GROUPS):
        send[g], recv[g] = CASES[name](K_OF[g], nb, gi)
    return send, recv


_cat = lambda ls: np.concatenate(ls).astype(np.int64) if len(ls) else np.zeros(0, np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["internal", "reference"])
@pytest.mark.parametrize("case", list(CASES))
def test_plan_pack_and_unpack_equal_the_numpy_gather(levels, order, case):
    """ludwig_halo_plan_pack -> the send buffer equals flat[concatenated send index]; a known message in the receive buffer ->
    ludwig_halo_plan_unpack -> the downloaded field equals the reference scatter, every unlisted element untouched. All four groups,
    each with every field it serves; ludwig_halo_pack (k_gather) on the same offsets gives the same message."""
    lvl = levels[order]
    send, recv = build_case(case, lvl.n_blocks)
    n_peers = len(send["f"])
    rc, h = ipw.create_plan(lvl, [0] * n_peers, send, recv)
    _lib.check(rc)
    assert h.value
    plan = ipw.PlanHandle(h, lvl)
    try:
        for gi, g in enumerate(GROUPS):
            for fi, field in enumerate(GROUP_FIELDS[g]):
                check_group(lvl, plan, g, field, _cat(send[g]), _cat(recv[g]), seed=1000 * gi + 10 * fi + 1)
    finally:
        plan.close()


def test_the_constructed_lists_are_what_they_claim():
    """no device: the cases hold the sector shapes their names promise (counted in the reference order, where block' = block), stay
    inside the field, and no receive list names an element twice"""
    nb = 12
    for name in CASES:
        send, recv = build_case(name, nb)
        for g in GROUPS:
            n = ref.n_elements(nb, K_OF[g])
            for side in (send[g], recv[g]):
                for a in side:
                    assert a.dtype == np.int64 and ((a >= 0) & (a < n)).all(), (name, g)
            r = _cat(recv[g])
            assert np.unique(r).size == r.size, (name, g)

    def members(a):                                    # sector -> members, in list order, of one component's part of a list
        out = {}
        for o in a:
            out.setdefault(int(o) >> 3, []).append(int(o) & 7)
        return out

    per = lambda name, g="vel": members(build_case(name, nb)[0][g][0])
    assert all(len(m) == 1 for m in per("x_face").values()) and len(per("x_face")) == 2 * 64
    assert all(m == list(range(8)) for m in per("y_face").values()) and len(per("y_face")) == 2 * 8
    assert all(m == list(range(8)) for m in per("z_face").values()) and len(per("z_face")) == 2 * 8
    assert sorted(len(m) for m in per("sector_members").values()) == sorted(len(m) for m in SECTORS.values())
    assert {1, 2, 3, 7, 8} <= {len(m) for m in per("sector_members").values()} and [0, 3, 7] in per("sector_members").values()
    assert [5, 6, 7] in per("run_across_sectors").values() and [0, 1, 2, 6, 7] in per("run_across_sectors").values()
    a = build_case("run_across_blocks", nb)[0]["vel"][0]
    assert (np.diff(a[:9]) == 1).all() and a[3] % 512 == 511 and a[4] == 512 * nb      # last block of component 0 -> component 1
    assert (np.diff(_cat(build_case("descending", nb)[0]["f"])) < 0).all()
    assert [0, 1, 2, 4, 3, 5, 6, 7] in per("one_inversion").values()
    s = build_case("same_element_adjacent", nb)[0]["f"]
    assert s[0][-1] == s[1][0] and s[2][-1] == s[3][0]
    s = build_case("same_element_far", nb)[0]["f"]
    assert np.intersect1d(s[0], s[1]).size == 4
    s, r = build_case("peers_some_empty", nb)
    for g in GROUPS:
        assert sorted((a.size > 0, b.size > 0) for a, b in zip(s[g], r[g])) == [(False, False), (False, True), (True, False), (True, True)]
    words = ref.random_words(4096, 3)
    assert np.isin(ref.SPECIALS, words).all() and np.unique(ref.offset_words(4096, 2)).size == 4096


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["internal", "reference"])
def test_exchange_with_device_copies_uses_the_per_peer_offsets(levels, order):
    """ludwig_halo_exchange without a communicator (every peer this rank itself: device copies from the send to the receive segment
    of each peer) on lists that are NOT symmetric: peers of different sizes, an empty one in between, other elements on the two sides.
    All four groups in one call; the result is flat[recv] = flat[send] of the state before the call."""
    lvl = levels[order]
    nb = lvl.n_blocks
    send, recv = {}, {}
    for gi, g in enumerate(GROUPS):
        K = K_OF[g]
        E, cat = _lists(K, nb)
        send[g] = [E(0, 1, SECTOR_CELLS[:13]), np.zeros(0, np.int64), cat(E(K - 1, 2, Y_FACE_LO[:16]), E(0, 3, [5]))[::-1].copy(), E(1, 4, X_FACE_LO[:7])]
        recv[g] = [E(1, 7, Z_FACE_HI[:13]), np.zeros(0, np.int64), E(K - 1, 8, SECTOR_CELLS[:17]), E(0, 9, [0, 9, 18, 27, 36, 45, 54])]
    rc, h = ipw.create_plan(lvl, [0] * 4, send, recv)
    _lib.check(rc)
    plan = ipw.PlanHandle(h, lvl)
    try:
        fields = {"f": "f_temp", "vel": "vel", "f_post": "f_post_collision", "rho": "rho"}
        words = {g: ref.random_words(ref.n_elements(nb, K_OF[g]), 50 + gi) for gi, g in enumerate(GROUPS)}
        for g, f in fields.items():
            lvl.upload(f, ref.as_field(words[g], nb, K_OF[g]))
        groups = (C.c_int32 * 4)(*range(4))
        flds = (C.c_int32 * 4)(*[_lib.FIELD_NAMES[fields[g]] for g in GROUPS])
        _lib.check(_lib.load().ludwig_halo_exchange(plan.h, 4, groups, flds))
        _lib.check(_lib.load().ludwig_halo_wait(plan.h))
        lvl.synchronize()
        for g, f in fields.items():
            got = ref.bits(lvl.download(f))
            want = ref.unpack(words[g], _cat(recv[g]), ref.pack(words[g], _cat(send[g])))
            assert np.array_equal(got, want), f"{g}: {ref.first_difference(got, want)}"
    finally:
        plan.close()


@pytest.fixture(scope="module")
def plain_level(gpu):
    """a level without f_post_collision"""
    grids, _ = cases.periodic_box((2, 1, 1))
    lv = adapt(grids[0], 0)
    assert not lv.has_post_collision
    yield lv
    lv.close()


def _assert_still_usable(lvl) -> None:
    nb = lvl.n_blocks
    send, recv = ref.offset(nb, 1, 0, SECTOR_CELLS), ref.offset(nb, 2, nb - 1, SECTOR_CELLS)
    rc, h = ipw.create_plan(lvl, [0], {"vel": [send]}, {"vel": [recv]})
    _lib.check(rc)
    plan = ipw.PlanHandle(h, lvl)
    try:
        check_group(lvl, plan, "vel", "vel", send, recv, seed=77)
    finally:
        plan.close()


E0 = np.zeros(0, np.int64)
BAD_PLANS = {
    # name: (level, keyword arguments of create_plan, expected code)
    "offset_equal_to_the_field_size": ("body", dict(peer_ranks=[0], send={"vel": [np.array([5, 3 * 12 * 512])]}, recv={}), -1),
    "offset_equal_to_the_field_size_on_the_receive_side": ("body", dict(peer_ranks=[0], send={}, recv={"rho": [np.array([12 * 512])]}), -1),
    "negative_offset": ("body", dict(peer_ranks=[0], send={"f": [np.array([7, -1, 9])]}, recv={}), -1),
    "negative_count": ("body", dict(peer_ranks=[0, 0], send={"vel": [np.array([1, 2, 3]), E0]}, recv={}, send_count={"vel": [3, -1]}), -1),
    "negative_count_that_a_positive_one_makes_up_for": ("body", dict(peer_ranks=[0, 0], send={}, recv={"f": [np.array([1, 2, 3]), E0]}, recv_count={"f": [-2, 5]}), -1),
    "index_list_missing": ("body", dict(peer_ranks=[0], send={}, recv={}, send_count={"rho": [4]}, null_index=["rho"]), -1),
    "f_post_group_without_the_array": ("plain", dict(peer_ranks=[0], send={"f_post": [np.array([0, 1, 2])]}, recv={}), -5),
    "f_post_group_without_the_array_receive_side": ("plain", dict(peer_ranks=[0], send={}, recv={"f_post": [np.array([4])]}), -5),
    "peer_rank_without_a_communicator": ("body", dict(peer_ranks=[0, 1], send={"vel": [np.array([1]), np.array([2])]}, recv={}), -1),
    "negative_peer_rank_without_a_communicator": ("body", dict(peer_ranks=[-1], send={}, recv={}), -1),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BAD_PLANS))
def test_plan_create_refuses_with_the_documented_code(levels, plain_level, name):
    """LUDWIG_ERR_INVALID (-1) for a bad argument, LUDWIG_ERR_STATE (-5) for a group the level has no storage for; *out is NULL
    afterwards (it held a non-null value before the call), the error text is set, and the level goes on working"""
    which, kwargs, code = BAD_PLANS[name]
    lvl = levels["internal"] if which == "body" else plain_level
    rc, h = ipw.create_plan(lvl, **kwargs)
    assert rc == code, (rc, _lib.load().ludwig_last_error())
    assert not h.value, "*out is not NULL after a failed ludwig_halo_plan_create"
    assert _lib.load().ludwig_last_error()
    _assert_still_usable(lvl)


@pytest.mark.gpu
def test_pack_and_unpack_refuse_a_field_of_another_component_count(levels):
    """group `vel` (3 components) asked to move f, rho, f_post_collision; group `rho` asked to move vel; group f asked to move the
    obstacle flags (1 byte per cell): LUDWIG_ERR_INVALID, and neither the fields nor the message buffers change"""
    lvl = levels["internal"]
    nb = lvl.n_blocks
    send, recv = build_case("sector_members", nb)
    rc, h = ipw.create_plan(lvl, [0], send, recv)
    _lib.check(rc)
    plan = ipw.PlanHandle(h, lvl)
    try:
        words = {f: ref.random_words(ref.n_elements(nb, K), 900 + i) for i, (f, K) in enumerate((("f", 27), ("vel", 3), ("rho", 1), ("f_post_collision", 27)))}
        for f, w in words.items():
            lvl.upload(f, ref.as_field(w, nb, w.size // (512 * nb)))
        for g in GROUPS:
            _lib.check(plan.pack(g, GROUP_FIELDS[g][0]))
        before = {g: plan.read_send(g) for g in GROUPS}
        marks = {g: ref.offset_words(plan.buffers(g)[3], 14) for g in GROUPS}
        for g in GROUPS:
            plan.write_recv(g, marks[g])
        for g, f in (("vel", "f"), ("vel", "rho"), ("vel", "f_post_collision"), ("rho", "vel"), ("f", "vel"), ("f", "obstacle"), ("f_post", "rho")):
            assert plan.pack(g, f) == -1, (g, f)
            assert plan.unpack(g, f) == -1, (g, f)
        assert _lib.load().ludwig_halo_plan_pack(plan.h, 4, _lib.FIELD_NAMES["f"], None) == -1          # no such group
        assert _lib.load().ludwig_halo_plan_unpack(plan.h, -1, _lib.FIELD_NAMES["f"], None) == -1
        lvl.synchronize()
        for g in GROUPS:
            assert np.array_equal(plan.read_send(g), before[g]), g
        for f, w in words.items():
            assert np.array_equal(ref.bits(lvl.download(f)), w), f
    finally:
        plan.close()
    _assert_still_usable(lvl)


# ---------------------------------------------------------------------------------------------------------------------------
# Part B: whole decompositions in this process
# ---------------------------------------------------------------------------------------------------------------------------
def _tunnel_cut_through_the_body():
    grids, params = cases.tunnel_with_sphere((6, 4, 4), levels=1, wall_model=False, temporal=False)
    bx = np.asarray(grids[0].active_block_coords)[:, 0]
    return grids[0], (bx > bx.min() + 2).astype(np.int64), params, np.float32(0.05)      # the cut runs through the sphere's blocks


def _ragged_owner(coords) -> np.ndarray:
    """three parts of 12, 8 and 10 blocks of a 5 x 3 x 2 box; part 1 is an L with a notch, part 2 what is left: no brick grid"""
    c = np.asarray(coords) - 1
    return np.where(c[:, 0] < 2, 0, np.where((c[:, 1] < 1) | ((c[:, 0] == 2) & (c[:, 2] == 0)), 1, 2)).astype(np.int64)


def _periodic_box_cut_three_ways():
    grids, params = cases.periodic_box((5, 3, 2), init=False)
    cases.init_perturbed(grids[0], 11)
    return grids[0], _ragged_owner(grids[0].active_block_coords), params, np.float32(0.0)


SINGLE_LEVEL_CASES = {"tunnel": _tunnel_cut_through_the_body, "periodic_box": _periodic_box_cut_three_ways}
STEPS = (5, 6)


def _newest(t: int):
    return ("f_temp", "vel_temp", "rho") if t % 2 == 0 else ("f", "vel", "rho")


@pytest.fixture(scope="module")
def single_device_runs(gpu):
    """case -> (global level, owner, params, u, {steps: {field: array}}): the one-device run of each case, taken once"""
    from open_ludwig_amd.physics import perform_timestep_v2
    out = {}
    for name, make in SINGLE_LEVEL_CASES.items():
        g, owner, params, u = make()
        dev = adapt(g, 0)
        states = {}
        for t in range(1, max(STEPS) + 1):
            perform_timestep_v2(dev, None, np.float32(0.5), u, params, t)
            if t in STEPS:
                states[t] = {n: dev.download(n) for n in _newest(t)}
        dev.close()
        out[name] = (g, owner, params, u, states)
    return out


def test_the_ragged_owner_map_is_no_brick_grid():
    grids, _ = cases.periodic_box((5, 3, 2), init=False)
    c = np.asarray(grids[0].active_block_coords)
    owner = _ragged_owner(c)
    assert np.bincount(owner).tolist() == [12, 8, 10]
    boxes = [int(np.prod(c[owner == r].max(axis=0) - c[owner == r].min(axis=0) + 1)) for r in range(3)]
    assert boxes[1] > 8 and boxes[2] > 10, "parts 1 and 2 were meant not to be boxes"


@pytest.mark.gpu
@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("case", list(SINGLE_LEVEL_CASES))
def test_single_level_stepped_with_native_plans_equals_the_single_device_run(single_device_runs, case, steps):
    """every rank on this device, exchanges through the native plans' pack / buffers / unpack, the non-overlap schedule of
    DistributedLevelRunner.step: owned blocks of every rank equal the one-device run bit for bit after an odd and an even number of
    steps. tunnel: the cut runs through the body - Bouzidi links cross it, the f_post group travels, and the ranks store
    f_post_collision only where a peer reads it (ludwig_level_add_post_collision_readers)."""
    g, owner, params, u, states = single_device_runs[case]
    world = ipw.SingleLevelWorld(g, owner, params)
    try:
        if case == "tunnel":
            assert all(r.level.n_boundary_cells > 0 for r in world.ranks), "the cut was meant to pass through the Bouzidi cells"
            assert sum(len(r.plan.recv[p]["f_post"]) for r in world.ranks for p in r.plan.peers) > 0, "no link reaches across the cut"
            assert sum(r.view.level.post_collision_readers.size for r in world.ranks) > 0
        else:
            assert world.world == 3 and all(len(r.plan.peers) == 2 for r in world.ranks)
        for t in range(1, steps + 1):
            world.step(t, u)
        ipw.device_sync()
        fn, vn, _ = _newest(steps)
        for r in world.ranks:
            own = r.view.local_to_global[: r.view.n_owned]
            for n in (fn, vn, "rho"):
                got = r.level.download(n)[:, :, :, : r.view.n_owned]
                assert same_bits(got, states[steps][n][:, :, :, own]), f"rank {r.view.rank} {n} differs from the single-device run"
        assert not np.array_equal(states[steps][vn], getattr(g, "vel")), "the velocity field has not moved"
    finally:
        world.close()


@pytest.mark.gpu
def test_rho_group_after_a_step_that_elided_the_rho_store(gpu):
    """The K = 1 group. A whole-level stream-collide launch leaves rho unwritten by default (lazy rho); ludwig_halo_plan_pack of the
    rho group has to produce it first (ensure_rho). The ghosts every rank receives equal the owner's rho after the step - which
    differs from the rho before it, so a pack of the stale array would show."""
    from open_ludwig_amd.physics import stream_collide
    g, owner, params, u = _periodic_box_cut_three_ways()

    def face_cells_of_rho(view, needs):                  # the cells of the velocity stencil, read as density too (a probe would)
        needs["rho"] = needs["vel"][needs["vel"] < 512 * view.level.n_blocks]

    world = ipw.SingleLevelWorld(g, owner, params, extra_needs=face_cells_of_rho)
    try:
        assert all(sum(len(r.plan.recv[p]["rho"]) for p in r.plan.peers) > 0 for r in world.ranks)
        for r in world.ranks:
            stream_collide(r.level, None, np.float32(0.5), u, params, 1, part=_lib.PART_ALL)
        world.exchange({"rho": "rho"})
        rho_after = np.zeros(g.rho.shape, dtype=np.float32, order="F")
        local = [r.level.download("rho") for r in world.ranks]
        for r, a in zip(world.ranks, local):
            rho_after[:, :, :, r.view.local_to_global[: r.view.n_owned]] = a[:, :, :, : r.view.n_owned]
        before, after = ref.bits(g.rho), ref.bits(rho_after)
        for r, a in zip(world.ranks, local):
            got = ref.bits(a)
            idx = _cat([r.plan.recv[p]["rho"] for p in r.plan.peers])
            glob = r.view.local_to_global[idx // 512] * 512 + idx % 512
            assert np.array_equal(got[idx], after[glob]), f"rank {r.view.rank}: {ref.first_difference(got[idx], after[glob])}"
            assert (after[glob] != before[glob]).mean() > 0.9, "the step was meant to change rho"
            untouched = np.ones(got.size, bool)
            untouched[idx] = False
            untouched[: 512 * r.view.n_owned] = False
            start = ref.bits(r.view.level.rho)
            assert np.array_equal(got[untouched], start[untouched]), f"rank {r.view.rank}: a ghost nobody sent has changed"
    finally:
        world.close()


_nested_grids = {}


def _nested_case(levels: int):
    if levels not in _nested_grids:
        _nested_grids[levels] = cases.tunnel_with_sphere((6, 4, 4), levels=levels, wall_model=False, temporal=True)
    return _nested_grids[levels]


def _nested_owners(grids, world: int, per_level: bool):
    """the owner maps of tests/test_partition_dist.py: x slabs of level-1 blocks with whole hierarchies per rank
    (test_two_ranks_nested_levels_cut_through_the_refinement), or every level bisected on its own
    (test_nested_levels_every_level_cut_on_its_own)"""
    if per_level:
        return partition.level_owners(grids, world)
    bx = np.asarray(grids[0].active_block_coords)[:, 0]
    owner1 = ((bx - 1) * world // int(bx.max())).astype(np.int64)
    return [owner1] + [partition.ancestor_owner(g.level_id, g.active_block_coords, grids[0].active_block_coords, owner1) for g in grids[1:]]


def _global_offsets(view, K: int, n_global: int) -> np.ndarray:
    """for every element of a rank's local array (by local offset) the offset of the same element in the global array"""
    l2g = np.asarray(view.local_to_global, dtype=np.int64)
    return ((np.arange(K, dtype=np.int64)[:, None, None] * n_global + l2g[None, :, None]) * 512 + np.arange(512, dtype=np.int64)[None, None, :]).reshape(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("levels,world,per_level", [(2, 2, False), (3, 2, False), (3, 2, True), (3, 3, True), (3, 4, True)])
def test_nested_levels_one_exchange_of_every_group(gpu, levels, world, per_level):
    """Nested levels whose refined region is cut, plans from the needs partition.MultiLevelRunner uses (same-level needs plus
    interpolation_needs). Every element holds its own global offset, every ghost a sentinel; after one exchange of every group each
    ghost element some plan receives holds the owner's value, every other ghost still the sentinel, every owned element its own
    value. Parent-data ghosts - parent cells of interface stencils that reach across a cut - are among what is received."""
    grids, params = _nested_case(levels)
    owners = _nested_owners(grids, world, per_level)
    nw = ipw.NestedWorld(grids, owners, params, world, upload_state=False)
    try:
        parent_only = 0
        for i, (g, ranks) in enumerate(zip(grids, nw.levels)):
            has_post = any(r.plan.has("f_post") for r in ranks)
            fields = {"f": "f", "vel": "vel", "rho": "rho"}
            if has_post:
                fields["f_post"] = "f_post_collision"
            start, truth = {}, {}
            for r in ranks:
                if r.level is None:
                    continue
                nb, n_owned = r.view.level.n_blocks, r.view.n_owned
                for gi, (grp, f) in enumerate(fields.items()):
                    K = K_OF[grp]
                    vals = (_global_offsets(r.view, K, g.n_blocks) | (np.int64(1 + gi) << 28)).astype(np.uint32)
                    ghost = (np.arange(vals.size) // 512) % nb >= n_owned
                    words = np.where(ghost, ref.SENTINEL, vals).astype(np.uint32)
                    r.level.upload(f, ref.as_field(words, nb, K))
                    start[r.view.rank, grp], truth[r.view.rank, grp] = words, vals
            ipw.exchange(ranks, fields)
            for r in ranks:
                if r.level is None:
                    continue
                nb, n_owned = r.view.level.n_blocks, r.view.n_owned
                for grp, f in fields.items():
                    got = ref.bits(r.level.download(f))
                    idx = _cat([r.plan.recv[p][grp] for p in r.plan.peers])
                    ghost = (np.arange(got.size) // 512) % nb >= n_owned
                    received = np.zeros(got.size, bool)
                    received[idx] = True
                    assert not received[~ghost].any(), "a plan receives into an owned block"
                    who = f"level {i + 1} rank {r.view.rank} {grp}"
                    t = truth[r.view.rank, grp]
                    assert np.array_equal(got[received], t[received]), f"{who}, received ghosts: {ref.first_difference(got[received], t[received])}"
                    assert (got[ghost & ~received] == ref.SENTINEL).all(), f"{who}: a ghost element no plan receives has changed"
                    assert np.array_equal(got[~ghost], t[~ghost]), f"{who}: an owned element has changed"
                # parent data: what the rank's finer blocks interpolate from and no same-level stencil of its own asks for
                if i + 1 < len(grids):
                    idx_all = {grp: _cat([r.plan.recv[p][grp] for p in r.plan.peers]) for grp in ("f", "rho")}
                    for grp in ("f", "rho"):
                        only = np.setdiff1d(nw.parent_data[i][r.view.rank][grp], nw.same_level[i][r.view.rank][grp])
                        assert np.isin(only, idx_all[grp]).all()
                        parent_only += only.size
        assert parent_only > 0, "no parent-data ghost crosses a cut: the case does not exercise them"
    finally:
        nw.close()
