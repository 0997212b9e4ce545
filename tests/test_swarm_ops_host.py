"""tests/swarm_ops_model.py on its own (no GPU): the crafted swarms tests/test_gpu_swarm_ops.py uploads -- the same
meshes, sizes, layouts and salts, imported from the model -- do exercise the paths they are there for, each with a
stated minimum count, so that a change to the generator cannot silently empty a case; the vectorised compaction
and sort key agree with a loop that takes one photon at a time; pack followed by unpack returns every travelling
photon with its bytes."""
import math

import numpy as np
import pytest

import swarm_ops_model as som

BIG = som.full_grid_n()           # on an MI355X (256 compute units); the GPU file derives it from the device


@pytest.fixture(scope="module")
def views():
    return {name: som.host_view(case)[1] for name, case in som.MESHES.items()}


def test_constants_come_from_the_header():
    assert (som.ST_ACTIVE, som.ST_ABSORBED, som.ST_ESCAPED, som.ST_OUTGOING, som.ST_OUTGOING_ABSORBED) == (0, 1, 2, 3, 4)
    assert som.RECORD_WORDS == 13 and len(som.KEYS) == 16
    assert BIG == 8 * 256 * 256 + 257 and BIG % 64 != 0


def test_crafted_swarms_bind_every_attribute_to_the_id(views):
    g = views["3d"]
    n = 2049
    sw = som.crafted(g, n, som.SALT["sort"])
    again = som.crafted(g, n, som.SALT["sort"])
    assert som.differing(sw, again) == []                                    # deterministic
    assert len(np.unique(sw["id"])) == n and int(sw["id"].max()) < 2 ** 63
    # no two attributes of a photon hold the same bytes, and no attribute repeats down the swarm
    for a in som.F64 + som.U64:
        for b in som.F64 + som.U64:
            if a < b:
                same = sw[a].view(np.uint64) == sw[b].view(np.uint64)
                assert same.mean() < 0.05, (a, b)             # (-0.0 and all-ones are shared on purpose)
    for k in ("x", "y", "z", "id", "rng"):
        assert len(np.unique(sw[k].view(np.uint64))) > 0.85 * n, k
    # the odd bit patterns, each at least 100 times over vx vy vz t e w
    bits = np.concatenate([sw[k].view(np.uint64) for k in ("vx", "vy", "vz", "t", "e", "w")])
    expo, frac = (bits >> np.uint64(52)) & np.uint64(0x7FF), bits & np.uint64(0x000FFFFFFFFFFFFF)
    assert int((bits == np.uint64(1 << 63)).sum()) >= 100                    # -0.0
    assert int(((expo == 0) & (frac != 0)).sum()) >= 100                     # denormals
    assert int(((expo == 0x7FF) & (frac != 0)).sum()) >= 100                 # NaNs with payloads
    assert int(((expo == 0x7FF) & (frac != 0) & (frac < np.uint64(1 << 51))).sum()) >= 30     # ... signalling ones
    assert int((sw["rng"] == np.uint64(2 ** 64 - 1)).sum()) >= 100
    assert int((sw["ip"] < 0).sum()) >= 100 and int((sw["kp"] > 2 ** 24).sum()) >= 100
    for k in ("x", "y", "z"):
        assert np.all(np.isfinite(sw[k]))
    # all five statuses, and for slots that are not ACTIVE every kind of blk
    assert set(np.unique(sw["status"]).tolist()) == {0, 1, 2, 3, 4}
    blk = sw["blk"][sw["status"] != som.ST_ACTIVE]
    for v in (-1, g.nblocks, som.INT_MAX):
        assert int((blk == v).sum()) >= 50, v
    assert int(((blk >= 0) & (blk < g.nblocks_total)).sum()) >= 100
    bad_active = (sw["status"] == som.ST_ACTIVE) & ((sw["blk"] < 0) | (sw["blk"] >= g.nblocks))
    assert int(bad_active.sum()) >= 30
    assert np.all(som.sort_key(g, sw, n)[bad_active] == g.nkeys)


# ---- compaction ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", som.LAYOUTS)
def test_compaction_layouts_hold_what_they_are_for(views, layout):
    g = views["1d"]
    for n in som.SMALL_N + (BIG,):
        sw = som.crafted(g, n, som.SALT["compact"], status=som.status_layout(layout, n, som.SALT["compact"]))
        survivors, want, holes, movers = som.compact(sw, n)
        assert len(holes) == len(movers) and len(want["id"]) == survivors         # holes equal to movers
        assert som.compact_failures(sw, n, want) == []
        kinds = set(sw["status"][movers].tolist())
        if layout == "random" and n >= 255:
            assert len(movers) >= n // 8 and kinds == set(som.LIVE), (n, len(movers))
        if layout == "upper half live" and n >= 2:
            assert len(movers) == survivors == n // 2 and len(holes) == n // 2   # every live slot moves
            assert n < 255 or kinds == set(som.LIVE)
        if layout == "alternating waves" and n >= 255:
            assert len(movers) >= n // 8 - 64 and kinds == set(som.LIVE), (n, len(movers))
        if layout == "all live":
            assert survivors == n and len(movers) == 0
        if layout == "none live":
            assert survivors == 0 and len(movers) == 0
        if layout == "one live at 0":
            assert survivors == 1 and len(movers) == 0
        if layout == "one live at n-1":
            assert survivors == 1 and len(movers) == (1 if n > 1 else 0)
        # a swarm with a mover: swapping two movers' rng, or dropping a copied attribute, is seen
        if len(movers) >= 2:
            wrong = som.copy(want)
            wrong["rng"][holes[0]], wrong["rng"][holes[1]] = want["rng"][holes[1]], want["rng"][holes[0]]
            assert som.compact_failures(sw, n, wrong) == ["moved rng"]
            stale = som.copy(want)
            stale["rng"][holes] = sw["rng"][holes]
            assert som.compact_failures(sw, n, stale) == ["moved rng"]


def _compact_one_at_a_time(sw, n):
    alive = [int(s) in som.LIVE for s in sw["status"][:n]]
    survivors = sum(alive)
    out = {k: [sw[k][q] for q in range(survivors)] for k in som.KEYS}
    movers = [q for q in range(survivors, n) if alive[q]]
    for q in range(survivors):
        if not alive[q]:
            s = movers.pop(0)
            for k in som.KEYS:
                out[k][q] = sw[k][s]
    assert movers == []
    return survivors, {k: np.array(out[k], dtype=sw[k].dtype) for k in som.KEYS}


def _sort_key_one_at_a_time(g, sw, n):
    keys = []
    for q in range(n):
        b = int(sw["blk"][q])
        if int(sw["status"][q]) != som.ST_ACTIVE or b < 0 or b >= g.nblocks:
            keys.append(g.nkeys)
            continue
        idx = []
        for d, name in enumerate(("x", "y", "z")):
            if d < g.ndim:
                i = math.floor((float(sw[name][q]) - float(g.xmin[b, d])) * (1.0 / float(g.dx[b, d]))) + g.first[d]
            else:
                i = g.first[d]
            idx.append(min(max(i, 0), g.dims[d] - 1))
        keys.append(b * g.ntot + (idx[2] * g.dims[1] + idx[1]) * g.dims[0] + idx[0])
    return np.array(keys)


@pytest.mark.parametrize("name", list(som.MESHES))
def test_the_model_agrees_with_a_loop_over_single_photons(views, name):
    g = views[name]
    n = 389
    sw = som.crafted(g, n, som.SALT["sort"] + 1)
    survivors, want, _, _ = som.compact(sw, n)
    s2, w2 = _compact_one_at_a_time(sw, n)
    assert survivors == s2 and som.differing(want, w2) == []
    key = som.sort_key(g, sw, n)
    assert np.array_equal(key, _sort_key_one_at_a_time(g, sw, n))
    assert key.max() == g.nkeys and key.min() >= 0
    # ... and sorted_failures accepts a stable sort, rejects a swapped attribute, a misplaced group, a lost photon
    order = np.argsort(key, kind="stable")
    good = som.take(sw, order)
    assert som.sorted_failures(g, sw, good, n) == []
    assert som.sorted_failures(g, sw, som.take(sw, order[::-1]), n) != []
    bad = som.copy(good)
    bad["rng"][[0, 1]] = bad["rng"][[1, 0]]
    assert som.sorted_failures(g, sw, bad, n) == ["group rng"]
    dup = som.copy(good)
    for k in som.KEYS:
        dup[k][1] = dup[k][0]
    assert som.sorted_failures(g, sw, dup, n) != []


# ---- the sort's cases ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(som.MESHES))
def test_sort_swarms_hold_what_they_are_for(views, name):
    g = views[name]
    many_cells = g.nblocks * g.ncell >= 64
    if name == "smr":
        assert len(np.unique(g.dx[:, 0])) == 2                 # block widths differ between blocks
    for n, runs_min, distinct_min, clamp_min in ((2049, 15, 1, 20), (BIG, 5000, 900, 5000)):
        # runs: runs of equal keys that cross a wave boundary; waves of 64 distinct keys (where the mesh has 64 cells)
        sw = som.sort_swarm(g, "runs", n, som.SALT["sort"])
        key = som.sort_key(g, sw, n)
        crossing, distinct = som.wave_census(key)
        assert crossing >= runs_min, (n, crossing)
        assert distinct >= (distinct_min if many_cells else 0), (n, distinct)
        assert int((key == g.nkeys).sum()) >= n // 20                         # runs of slots that are not ACTIVE too
        starts = som.run_starts(key)
        assert set(som.RUN_LENGTHS) <= set(starts)
        if n == BIG:                                                          # every run length at every lane offset
            for m in som.RUN_LENGTHS:
                assert starts[m] == set(range(64)), m
        assert som.clamp_census(g, sw, n) == [(0, 0)] * g.ndim               # (this group: every position in its cell)
        # hashed: nothing clamped, every blk valid, the swarm far from sorted
        sw = som.sort_swarm(g, "hashed", n, som.SALT["sort"])
        key = som.sort_key(g, sw, n)
        assert som.clamp_census(g, sw, n) == [(0, 0)] * g.ndim
        act = sw["status"] == som.ST_ACTIVE
        assert np.all((sw["blk"][act] >= 0) & (sw["blk"][act] < g.nblocks)) and int((np.diff(key) < 0).sum()) >= n // 8
        # edges: clamped positions on both sides of every active axis; ghost-layer keys; blk outside the blocks
        sw = som.sort_swarm(g, "edges", n, som.SALT["sort"])
        key = som.sort_key(g, sw, n)
        for below, above in som.clamp_census(g, sw, n):
            assert below >= clamp_min and above >= clamp_min, (n, below, above)
        raw = som.raw_cell_index(g, sw, n)
        valid = act_valid = (sw["status"] == som.ST_ACTIVE) & (sw["blk"] >= 0) & (sw["blk"] < g.nblocks)
        for d in range(g.ndim):
            ghost = valid & (((raw[d] >= 0) & (raw[d] < g.first[d])) | ((raw[d] >= g.first[d] + g.nx[d]) & (raw[d] < g.dims[d])))
            assert int(ghost.sum()) >= clamp_min // 2, (n, d)                 # one ghost layer out: in the array, not clamped
            assert int((np.abs(raw[d]) > 10 ** 6).sum()) >= clamp_min // 2     # far out
        assert int(((sw["status"] == som.ST_ACTIVE) & ~act_valid).sum()) >= clamp_min // 2
    # the small sizes are what they say
    for n in som.SMALL_N:
        sw = som.sort_swarm(g, "edges", n, som.SALT["sort"])
        assert len(sw["id"]) == n and som.sorted_failures(g, sw, som.take(sw, np.argsort(som.sort_key(g, sw, n), kind="stable")), n) == []


@pytest.mark.parametrize("which", list(som.CARRY_MESHES))
def test_the_carry_swarm_reaches_both_sides_of_every_stretch(which):
    _, g = som.host_view(som.CARRY_MESHES[which])
    tiles, edge = som.carry_tiles(g)
    assert (g.nblocks, g.nkeys + 1, tiles) == {"two stretches": (3, 2100013, 1026), "three stretches": (3, 4200013, 2051)}[which]
    assert edge == {"two stretches": [0, 1023, 1024, 1025], "three stretches": [0, 1023, 1024, 2047, 2048, 2050]}[which]
    sw = som.carry_swarm(g, som.CARRY_N, som.SALT["carry"])
    key = som.sort_key(g, sw, som.CARRY_N)
    per_tile = np.bincount(key // som.SCAN_TILE, minlength=tiles)
    for t in edge:
        assert per_tile[t] >= 100, (t, per_tile[t])
    assert int((key == g.nkeys).sum()) >= 300                    # the bin behind all cells: the last bin
    assert int((key == g.nkeys - 1).sum()) >= 20                 # the last cell of the last block (clamped from above)
    assert int((key == 0).sum()) >= 20                           # the first (clamped from below)
    # a carry lost between two stretches would move everything behind it: there is something in front of each
    for s in range(som.SUMS_STRETCH, tiles, som.SUMS_STRETCH):
        assert per_tile[s - som.SUMS_STRETCH:s].sum() >= 200 and per_tile[s:].sum() >= 200


# ---- hand-off -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", som.RANKS)
def test_pack_swarms_hold_what_they_are_for(R):
    mesh, g = som.host_view(som.RANK_MESH, 0, R)
    assert mesh.nblocks == 64 and g.nx[0] == 4 and sorted(set(g.owner.tolist())) == list(range(R))
    for to_self in (True, False):
        for n in (2049, BIG):
            sw, quiet = som.pack_swarm(g, n, som.SALT["pack"], to_self=to_self)
            st = sw["status"]
            out = (st == som.ST_OUTGOING) | (st == som.ST_OUTGOING_ABSORBED)
            assert int((st == som.ST_OUTGOING).sum()) >= n // 8 and int((st == som.ST_OUTGOING_ABSORBED).sum()) >= n // 8
            assert np.all((sw["blk"][out] >= 0) & (sw["blk"][out] < 64))          # an owner to look up, always
            ranks = g.owner[sw["blk"][out]]
            assert set(ranks.tolist()) == set(range(R)) - (set() if to_self else {0})
            assert to_self or not np.any(ranks == 0)
            # negative ip / jp: the sign handling of (unsigned)ip | jp << 32
            assert int((out & (sw["ip"] < 0)).sum()) >= n // 16 and int((out & (sw["jp"] < 0)).sum()) >= n // 16
            for first, last in som.pack_ranges(n, quiet):
                none, distinct = som.destination_census(g.owner, sw, first, last)
                counts, segments, after = som.pack(g.owner, sw, first, last, R)
                if (first, last) in ((0, n), (1, n - 1)):
                    assert none >= 1                                             # a wave with no outgoing photon
                    if R == 64 and to_self:
                        assert distinct >= 1                                     # a wave whose lanes go to 64 ranks
                    assert np.all(counts[0 if to_self else 1:] >= 1)
                if (first, last) == (quiet[0] + 1, quiet[1] - 1):
                    assert counts.sum() == 0 and last - first >= 64
                if (first, last) == (65, 70):
                    assert 1 <= counts.sum() <= 5
                assert counts.sum() == sum(len(s) for s in segments) == int((after["status"] != st).sum())
                untouched = np.ones(n, dtype=bool)
                untouched[first:last] = False
                assert som.differing(som.take(after, untouched), som.take(sw, untouched)) == []
    # slots outside (1, n - 1) that ARE outgoing and stay so
    sw, quiet = som.pack_swarm(g, 2049, som.SALT["pack"])
    st = sw["status"].copy()
    st[[0, 2048]] = som.ST_OUTGOING
    sw2 = som.crafted(g, 2049, som.SALT["pack"], status=st, dest=np.where(np.arange(2049) % 2048 == 0, 63, sw["blk"]))
    _, _, after = som.pack(g.owner, sw2, 1, 2048, R)
    assert after["status"][0] == after["status"][2048] == som.ST_OUTGOING


def test_record_layout_word_by_word():
    _, g = som.host_view(som.RANK_MESH, 0, 2)
    sw = som.crafted(g, 4, 1, status=[3, 4, 3, 4], dest=[40, 41, 42, 63])
    sw["ip"][:] = [-1, 5, -2 ** 31, 7]
    sw["jp"][:] = [2, -1, 3, -7]
    sw["kp"][:] = [-1, 0, 9, 2 ** 31 - 1]
    rec = som.records(sw, np.arange(4))
    for q, k in enumerate(som.F64):
        assert np.array_equal(rec[:, q], sw[k].view(np.uint64))
    assert rec[:, 9].tolist() == [int(sw["id"][0]), int(sw["id"][1]) | 1 << 63, int(sw["id"][2]), int(sw["id"][3]) | 1 << 63]
    assert rec[:, 10].tolist() == [0xFFFFFFFF | 2 << 32, 5 | 0xFFFFFFFF << 32, 0x80000000 | 3 << 32, 7 | 0xFFFFFFF9 << 32]
    assert rec[:, 11].tolist() == [0xFFFFFFFF | 40 << 32, 41 << 32, 9 | 42 << 32, 0x7FFFFFFF | 63 << 32]
    assert np.array_equal(rec[:, 12], sw["rng"])


def test_pack_then_unpack_returns_every_traveller_with_its_bytes():
    views = [som.host_view(som.RANK_MESH, r, 2)[1] for r in range(2)]
    assert views[1].gids[0] == 32 and views[1].local_index[32] == 0 and views[1].local_index[31] == 32
    n = 2049
    for rank in (0, 1):
        src, dst = views[rank], views[1 - rank]
        sw, _ = som.pack_swarm(src, n, som.SALT["exchange"] + rank, rank=rank, to_self=False, arrivals=True)
        counts, segments, after = som.pack(src.owner, sw, 0, n, 2)
        assert counts[rank] == 0 and counts[1 - rank] >= n // 4
        base = som.edelta_base(dst, som.SALT["base"])
        there = som.crafted(dst, 7, som.SALT["resident"])
        whole, edelta = som.unpack(dst, there, 7, segments[1 - rank], base)
        assert som.differing(som.take(whole, np.arange(7)), there) == []
        got = som.take(whole, np.arange(7, 7 + len(segments[1 - rank])))
        went = np.flatnonzero(after["status"] != sw["status"])
        sent = som.take(sw, went[np.argsort(sw["id"][went])])                 # travellers in id order
        absorbed = sent["status"] == som.ST_OUTGOING_ABSORBED
        got = som.take(got, np.argsort(got["id"] & ~som.BIT63))
        assert int(absorbed.sum()) >= n // 16 and int((~absorbed).sum()) >= n // 16
        for k in som.F64 + ("ip", "jp", "kp", "rng"):
            assert np.array_equal(got[k].view(np.uint8), sent[k].view(np.uint8)), k
        assert np.array_equal(got["id"], sent["id"] | np.where(absorbed, som.BIT63, np.uint64(0)))
        assert np.array_equal(got["blk"], dst.local_index[sent["blk"]]) and np.all(got["blk"] >= 0)
        assert np.array_equal(got["status"], np.where(absorbed, som.ST_ABSORBED, som.ST_ACTIVE))
        # energy_delta: the absorbed arrivals' weights, exactly, in any order of addition
        diff = edelta - base
        assert math.fsum(diff.ravel().tolist()) == math.fsum(sent["w"][absorbed].tolist())
        order = np.flatnonzero(absorbed)[::-1]
        again = base.copy()
        for q in order.tolist():
            again[got["blk"][q], got["kp"][q], got["jp"][q], got["ip"][q]] += got["w"][q]
        assert np.array_equal(again.view(np.uint64), edelta.view(np.uint64))
        assert int((diff != 0).sum()) >= 16
