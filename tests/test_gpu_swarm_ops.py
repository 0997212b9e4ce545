"""The kernels that move whole photons from slot to slot, on the GPU, against tests/swarm_ops_model.py bit for bit:
compaction (k_count_active, k_list_holes_movers, k_fill_holes), the defrag sort in its default order (k_sort_count,
the three scan kernels, k_sort_pack, k_sort_unpack) and the hand-off (k_count_outgoing, k_pack_outgoing,
k_unpack_incoming, jb_exchange through a loopback transport that plays the other ranks in this process).  Crafted
swarms on the smallest shapes where these kernels can go wrong -- tests/test_swarm_ops_host.py shows that the swarms
hold the cases; expected values come from the numpy model, never from the library.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import swarm_ops_model as som
from helpers import load_deck

from test_gpu_comb import _upload

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A5A5A5A5A        # what a record buffer holds where nothing may be written
AMPLE = 1 << 40


def _sizes(device):
    import torch
    return som.SMALL_N + (som.full_grid_n(torch.cuda.get_device_properties(device).multi_processor_count),)


@pytest.fixture(scope="module")
def views(gpu_device):
    """(driver, Geom) per (mesh, rank, nranks), made once: the driver's view of the mesh is the one the host test
    counted the cases on"""
    from jaybenne_amd import mcblock
    made = {}

    def get(case, rank=0, nranks=1):
        key = (repr(case), rank, nranks)
        if key not in made:
            drv = mcblock.McblockDriver(load_deck(*case), rank=rank, nranks=nranks, comm=None, device=gpu_device)
            md = drv.md
            assert md.cell_order == "any" and md.deposition == "atomic"
            g = som.Geom(drv.mesh, md.resident_gids, md.field_owner, md.nowned)
            _, h = som.host_view(case, rank, nranks)
            assert np.array_equal(g.gids, h.gids) and np.array_equal(g.owner, h.owner) and g.nowned == h.nowned
            assert np.array_equal(g.xmin, h.xmin) and np.array_equal(g.dx, h.dx)
            made[key] = (drv, g)
        return made[key]

    yield get
    for drv, _ in made.values():
        drv.md.close()
    made.clear()


def _download(md, n, first=0):
    import torch
    torch.cuda.synchronize(md.device)
    out = {k: md.swarm[k][first:n].cpu().numpy() for k in som.KEYS}
    out["id"], out["rng"] = out["id"].view(np.uint64), out["rng"].view(np.uint64)
    return out


def _check(md, st):
    from jaybenne_amd import _lib
    assert st == _lib.JB_COMPLETE, (st, md.lib.jb_last_error())


# ---- compaction -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", som.LAYOUTS)
def test_compaction_equals_the_model(gpu_device, views, layout):
    drv, g = views(som.MESHES["1d"])
    md = drv.md
    salt = som.SALT["compact"]
    for n in _sizes(gpu_device):
        sw = som.crafted(g, n, salt, status=som.status_layout(layout, n, salt))
        survivors, _, holes, movers = som.compact(sw, n)
        _upload(md, sw, gpu_device)
        md._sync_stream()
        _check(md, md.lib.jb_remove_marked_particles(md.pkg.ctx, C.byref(md.sv)))
        assert md.n == survivors, (layout, n)
        got = _download(md, survivors)
        assert som.compact_failures(sw, n, got) == [], (layout, n)      # stayers' bytes; the moved records as a multiset
        if layout in ("random", "upper half live", "alternating waves") and n >= 255:
            moved = set(got["status"][holes].tolist())
            assert moved == set(som.LIVE) == set(sw["status"][movers].tolist()), (layout, n)


# ---- defrag sort, default cell order -------------------------------------------------------------------------
def _defrag(md):
    md._sync_stream()
    _check(md, md.lib.jb_defrag_particles(md.pkg.ctx, md.handle, C.byref(md.sv)))


def _sort_now(md):
    md._sync_stream()
    done = C.c_int32(0)
    _check(md, md.lib.jb_defrag_policy(md.pkg.ctx, md.handle, C.byref(md.sv), 0, som.DEFRAG_SORT_NOW, C.byref(done)))
    assert done.value == 1


@pytest.mark.parametrize("group", ["hashed", "runs", "edges"])
@pytest.mark.parametrize("name", list(som.MESHES))
def test_defrag_sort_equals_the_model(gpu_device, views, name, group):
    drv, g = views(som.MESHES[name])
    md = drv.md
    sizes = _sizes(gpu_device)
    for n in sizes:
        sw = som.sort_swarm(g, group, n, som.SALT["sort"])
        _upload(md, sw, gpu_device)
        _defrag(md)
        assert md.n == n
        got = _download(md, n)
        assert som.sorted_failures(g, sw, got, n) == [], (name, group, n)
        if n in (2049, sizes[-1]):
            _defrag(md)                                                  # a second call, on the sorted swarm
            again = _download(md, n)
            assert som.sorted_failures(g, sw, again, n) == [], (name, group, n)
            key = som.sort_key(g, again, n)
            assert np.array_equal(key, som.sort_key(g, got, n))
        if n == 2049:
            _upload(md, sw, gpu_device)                                  # jb_defrag_policy, SORT_NOW: the same grouping
            _sort_now(md)
            assert som.sorted_failures(g, sw, _download(md, n), n) == [], (name, group, n)


@pytest.mark.parametrize("which", list(som.CARRY_MESHES))
def test_defrag_sort_carries_the_offset_between_stretches_of_tile_sums(gpu_device, which):
    """More than 1024 x 2048 histogram bins: k_scan_sums hands a running offset from one stretch of 1024 tile sums to
    the next -- once on the mesh of 2.1 M cells, twice on the one of 4.2 M, where the second hand-over must hold the
    sum of both stretches before it."""
    from jaybenne_amd import mcblock
    case = som.CARRY_MESHES[which]
    drv = mcblock.McblockDriver(load_deck(*case), device=gpu_device)
    md = drv.md
    try:
        assert md.cell_order == "any"
        g = som.Geom(drv.mesh, md.resident_gids, md.field_owner, md.nowned)
        tiles, edge = som.carry_tiles(g)
        assert tiles > som.SUMS_STRETCH * (2 if which == "three stretches" else 1)
        n = som.CARRY_N
        sw = som.carry_swarm(g, n, som.SALT["carry"])
        per_tile = np.bincount(som.sort_key(g, sw, n) // som.SCAN_TILE, minlength=tiles)
        assert all(per_tile[t] >= 100 for t in edge)
        _upload(md, sw, gpu_device)
        _defrag(md)
        got = _download(md, n)
        assert som.sorted_failures(g, sw, got, n) == [], which
        _upload(md, sw, gpu_device)
        _sort_now(md)
        assert som.sorted_failures(g, sw, _download(md, n), n) == [], which
    finally:
        md.close()


# ---- pack ------------------------------------------------------------------------------------------------------
def _pack(md, first, last, R, rec, capacity):
    counts = np.full(R, -7, dtype=np.int64)
    md._sync_stream()
    st = md.lib.jb_pack_outgoing(md.pkg.ctx, md.handle, C.byref(md.sv), first, last, R,
                                 rec.data_ptr() if rec is not None else None, capacity, counts.ctypes.data)
    return st, counts


def _segments_equal(buf, counts, offsets, segments):
    """each rank's segment of a record buffer (host array [*, 13]) at its offset, as a set, word by word"""
    for r, want in enumerate(segments):
        got = som.record_set(buf[offsets[r]:offsets[r] + counts[r]])
        if got.shape != want.shape or not np.array_equal(got, want):
            return False
    return True


@pytest.mark.parametrize("R", som.RANKS)
def test_pack_equals_the_model(gpu_device, views, R):
    import torch
    from jaybenne_amd import _lib
    drv, g = views(som.RANK_MESH, 0, R)
    md = drv.md
    sizes = _sizes(gpu_device)
    for n in sizes:
        sw, quiet = som.pack_swarm(g, n, som.SALT["pack"])
        ranges = som.pack_ranges(n, quiet) if n in (257, 2049, sizes[-1]) else [(0, n)]
        for first, last in ranges:
            want_counts, segments, after = som.pack(g.owner, sw, first, last, R)
            total = int(want_counts.sum())
            _upload(md, sw, gpu_device)
            rec = torch.full((total + 3, som.RECORD_WORDS), FILL, dtype=torch.int64, device=gpu_device)
            st, counts = _pack(md, first, last, R, rec, total + 3)
            _check(md, st)
            assert np.array_equal(counts, want_counts), (R, n, first, last)
            buf = rec.cpu().numpy().view(np.uint64)
            offsets = np.concatenate(([0], np.cumsum(want_counts)[:-1]))
            assert _segments_equal(buf, want_counts, offsets, segments), (R, n, first, last)
            assert np.all(buf[total:] == np.uint64(FILL))
            assert som.differing(_download(md, n), after) == [], (R, n, first, last)     # the swarm, byte for byte
    # the capacity path: the counts filled in, the swarm as it was; then a call with room
    n = 2049
    sw, _ = som.pack_swarm(g, n, som.SALT["pack"])
    want_counts, segments, after = som.pack(g.owner, sw, 0, n, R)
    total = int(want_counts.sum())
    _upload(md, sw, gpu_device)
    rec = torch.full((total, som.RECORD_WORDS), FILL, dtype=torch.int64, device=gpu_device)
    for buf_arg, capacity in ((None, total), (rec, total - 1), (rec, 0)):
        st, counts = _pack(md, 0, n, R, buf_arg, capacity)
        assert st == _lib.JB_ERR_CAPACITY and np.array_equal(counts, want_counts), (R, capacity)
        assert som.differing(_download(md, n), sw) == []
        assert bool((rec == FILL).all())
    st, counts = _pack(md, 0, n, R, rec, total)
    _check(md, st)
    offsets = np.concatenate(([0], np.cumsum(want_counts)[:-1]))
    assert np.array_equal(counts, want_counts)
    assert _segments_equal(rec.cpu().numpy().view(np.uint64), want_counts, offsets, segments)
    assert som.differing(_download(md, n), after) == []
    # ... and nothing is sent twice: a second pack of the same range finds nothing
    st, counts = _pack(md, 0, n, R, rec, total)
    _check(md, st)
    assert not counts.any() and som.differing(_download(md, n), after) == []


# ---- unpack ----------------------------------------------------------------------------------------------------
def _arrivals(g, nrec, salt, gids):
    """nrec records for this rank: both kinds, addressed to the blocks `gids`, in a hashed order"""
    q = np.arange(nrec)
    status = np.where(som._mod(q, salt + 1, 3) == 0, som.ST_OUTGOING_ABSORBED, som.ST_OUTGOING)
    dest = np.asarray(gids)[som._mod(q, salt + 2, len(gids))]
    sw = som.crafted(g, nrec, salt, status=status, dest=dest, arrivals=True)
    return som.records(sw, q)


def _set_edelta(md, g, salt):
    base = som.edelta_base(g, salt)
    md.set_field("edelta", base, local=True)
    return base


def _edelta(md):
    import torch
    torch.cuda.synchronize(md.device)
    return md.fields["edelta"].cpu().numpy()


UNPACK_VIEWS = {"3d, one rank": (som.MESHES["3d"], 0, 1), "1d, rank 1 of 2": (som.RANK_MESH, 1, 2)}


@pytest.mark.parametrize("view", list(UNPACK_VIEWS))
def test_unpack_equals_the_model(gpu_device, views, view):
    import torch
    drv, g = views(*UNPACK_VIEWS[view])
    md = drv.md
    if view != "3d, one rank":        # local block indices differ from global ids: 32 .. 63 are 0 .. 31, 31 is 32
        assert g.local_index[32] == 0 and g.local_index[31] == 32
    n0 = 301
    resident = som.crafted(g, n0, som.SALT["resident"])
    sizes = _sizes(gpu_device)
    for nrec in (1, 64, 257, sizes[-1]):
        rec = _arrivals(g, nrec, som.SALT["arrivals"], g.gids)
        base = _set_edelta(md, g, som.SALT["base"])
        want, want_edelta = som.unpack(g, resident, n0, rec, base)
        if nrec >= 257:
            assert int((want["status"][n0:] == som.ST_ABSORBED).sum()) >= nrec // 8
            assert len(set(want["blk"][n0:].tolist())) == g.nblocks and int((want_edelta != base).sum()) >= 8
        _upload(md, resident, gpu_device)
        md.reserve(n0 + nrec)
        rec_d = torch.from_numpy(rec.view(np.int64)).to(gpu_device)
        md._sync_stream()
        _check(md, md.lib.jb_unpack_incoming(md.pkg.ctx, md.handle, C.byref(md.sv), rec_d.data_ptr(), nrec))
        assert md.n == n0 + nrec
        got = _download(md, n0 + nrec)
        assert som.differing(som.take(got, np.arange(n0)), resident) == [], (view, nrec)     # what was there: untouched
        assert som.differing(got, want) == [], (view, nrec)                                  # arrivals, in record order
        assert np.array_equal(_edelta(md).view(np.uint64), want_edelta.view(np.uint64)), (view, nrec)


# ---- jb_exchange through a loopback transport ---------------------------------------------------------------------
class Loopback:
    """A jb_exchange_transport that plays ranks 1 .. R - 1 in this process.  The all-gather copies this rank's row
    into place and fills the other rows: ``incoming[r]`` records towards rank 0, ample room (``rooms[r]`` = (send,
    receive, swarm) overrides that), zero in any further word of the row -- the row's length is the callback's
    ``count``.  The all-to-all keeps a copy of the send buffer with its counts and offsets and writes ``records[r]``
    at the receive offsets."""

    def __init__(self, device, R, incoming, records, rooms=None):
        from jaybenne_amd import _lib
        from jaybenne_amd.handoff import _alias
        self.R, self.row_words, self.sent, self.error, self.exchanges = R, None, None, None, 0
        self.rooms = rooms or {}

        def all_gather(_h, in_dev, out_dev, count, _stream):
            try:
                import torch
                self.row_words = int(count)
                rows = np.zeros((R, count), dtype=np.int64)
                for r in range(1, R):
                    rows[r, 0] = incoming[r]
                    rows[r, R:R + 3] = self.rooms.get(r, (AMPLE, AMPLE, AMPLE))
                out = _alias(out_dev, count * R, device)
                out.copy_(torch.from_numpy(rows.reshape(-1)).to(device))
                out[:count].copy_(_alias(in_dev, count, device))
                return 0
            except Exception as e:   # noqa: BLE001 -- nothing may propagate through the C frames
                self.error = e
                return 1

        def all_to_all_v(_h, send_dev, sc, so, recv_dev, rc, ro, words, _stream):
            try:
                import torch
                self.exchanges += 1
                arr = lambda p: np.ctypeslib.as_array(p, shape=(R,)).astype(np.int64)      # noqa: E731
                self.sc, self.so, self.rc, self.ro, self.words = arr(sc), arr(so), arr(rc), arr(ro), int(words)
                nsend = int(self.sc.sum())
                self.sent = (_alias(send_dev, nsend * words, device).cpu().numpy().reshape(nsend, words).view(np.uint64)
                             if nsend else np.zeros((0, words), dtype=np.uint64))
                for r in range(R):
                    if self.rc[r]:
                        assert self.rc[r] == len(records[r])
                        dst = _alias(recv_dev + int(self.ro[r]) * words * 8, int(self.rc[r]) * words, device)
                        dst.copy_(torch.from_numpy(records[r].view(np.int64).reshape(-1)).to(device))
                return 0
            except Exception as e:   # noqa: BLE001
                self.error = e
                return 1

        self._keep = (_lib.ALL_GATHER_FN(all_gather), _lib.ALL_TO_ALL_V_FN(all_to_all_v))
        self.tr = _lib.ExchangeTransport()
        self.tr.handle = None
        self.tr.all_gather_u64, self.tr.all_to_all_v = self._keep


def _exchange(md, lb, first, last, R, send, send_cap, recv, recv_cap):
    nsent, nrecv, moved = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    md._sync_stream()
    st = md.lib.jb_exchange(md.pkg.ctx, md.handle, C.byref(md.sv), first, last, 0, R, C.byref(lb.tr),
                            send.data_ptr(), send_cap, recv.data_ptr(), recv_cap,
                            C.byref(nsent), C.byref(nrecv), C.byref(moved))
    assert lb.error is None, repr(lb.error)
    return st, nsent.value, nrecv.value, moved.value


def _exchange_case(g, R, n, salt):
    """(swarm, records arriving from each rank, the same in rank order as one array)"""
    sw, _ = som.pack_swarm(g, n, salt, to_self=False)
    incoming = [0] + [1 + (37 * r) % 53 for r in range(1, R)]
    if R == 8:
        incoming[5] = 300                   # more than a workgroup from one rank
    rec = _arrivals(g, sum(incoming), salt + 50, g.gids[:g.nowned])
    cut = np.concatenate(([0], np.cumsum(incoming)))
    return sw, incoming, [rec[cut[r]:cut[r + 1]] for r in range(R)], rec


@pytest.mark.parametrize("R", som.RANKS)
def test_exchange_through_a_loopback_transport(gpu_device, views, R):
    import torch
    drv, g = views(som.RANK_MESH, 0, R)
    md = drv.md
    sizes = _sizes(gpu_device)
    for n in (2049,) + ((sizes[-1],) if R == 8 else ()):
        sw, incoming, per_rank, rec = _exchange_case(g, R, n, som.SALT["exchange"])
        nin = len(rec)
        want_counts, segments, after = som.pack(g.owner, sw, 0, n, R)
        nout = int(want_counts.sum())
        assert want_counts[0] == 0 and np.all(want_counts[1:] > 0)
        base = _set_edelta(md, g, som.SALT["base"])
        want, want_edelta = som.unpack(g, after, n, rec, base)        # the packed slots are holes, the arrivals behind
        _upload(md, sw, gpu_device)
        md.reserve(n + nin)
        send = torch.full((nout + 2, som.RECORD_WORDS), FILL, dtype=torch.int64, device=gpu_device)
        recv = torch.full((nin + 2, som.RECORD_WORDS), FILL, dtype=torch.int64, device=gpu_device)
        lb = Loopback(gpu_device, R, incoming, per_rank)
        st, nsent, nrecv, moved = _exchange(md, lb, 0, n, R, send, nout + 2, recv, nin + 2)
        _check(md, st)
        assert (nsent, nrecv, moved) == (nout, nin, nout + nin) and lb.exchanges == 1
        assert lb.row_words >= R + 3 and lb.words == som.RECORD_WORDS
        assert np.array_equal(lb.sc, want_counts) and np.array_equal(lb.rc, incoming)
        assert np.array_equal(lb.so, np.concatenate(([0], np.cumsum(want_counts)[:-1])))
        assert np.array_equal(lb.ro, np.concatenate(([0], np.cumsum(incoming)[:-1])))
        assert _segments_equal(lb.sent, lb.sc, lb.so, segments), (R, n)          # the captured segments
        assert md.n == n + nin
        got = _download(md, n + nin)
        assert som.differing(som.take(got, np.arange(n)), after) == [], (R, n)    # the packed slots are holes
        assert som.differing(got, want) == [], (R, n)                             # ... and the arrivals behind them
        assert np.array_equal(_edelta(md).view(np.uint64), want_edelta.view(np.uint64))
        assert bool((send[nout:] == FILL).all()) and bool((recv[nin:] == FILL).all())
        # nothing left to go: a second call over the whole swarm moves nothing on this side
        quiet = Loopback(gpu_device, R, [0] * R, [rec[:0]] * R)
        st, nsent, nrecv, moved = _exchange(md, quiet, 0, md.n, R, send, nout + 2, recv, nin + 2)
        _check(md, st)
        assert (nsent, nrecv, moved) == (0, 0, 0) and quiet.exchanges == 0


def test_exchange_verdicts_come_before_any_pack(gpu_device, views):
    """The three capacity verdicts and "hands particles to itself" return with the swarm byte-identical, the buffers
    unwritten and the record exchange not entered; the call with room then goes through."""
    import torch
    from jaybenne_amd import _lib
    R, n = 8, 2049
    drv, g = views(som.RANK_MESH, 0, R)
    md = drv.md
    sw, incoming, per_rank, rec = _exchange_case(g, R, n, som.SALT["exchange"] + 7)
    nin = len(rec)
    want_counts, segments, after = som.pack(g.owner, sw, 0, n, R)
    nout = int(want_counts.sum())
    base = _set_edelta(md, g, som.SALT["base"])
    _upload(md, sw, gpu_device)
    md.reserve(n + nin)
    send = torch.full((nout, som.RECORD_WORDS), FILL, dtype=torch.int64, device=gpu_device)
    recv = torch.full((nin, som.RECORD_WORDS), FILL, dtype=torch.int64, device=gpu_device)

    def untouched(lb, what):
        assert lb.exchanges == 0, what
        assert som.differing(_download(md, n), sw) == [] and md.n == n, what
        assert bool((send == FILL).all()) and bool((recv == FILL).all()), what
        assert np.array_equal(_edelta(md).view(np.uint64), base.view(np.uint64)), what

    capacity = md.sv.capacity
    cases = [("send room, by the argument", {}, nout - 1, nin, capacity, b"rank 0's send buffer"),
             ("send room, by rank 3's row", {3: (incoming[3] - 1, AMPLE, AMPLE)}, nout, nin, capacity, b"rank 3's send buffer"),
             ("receive room, by the argument", {}, nout, nin - 1, capacity, b"rank 0's receive buffer"),
             ("receive room, by rank 5's row", {5: (AMPLE, int(want_counts[5]) - 1, AMPLE)}, nout, nin, capacity,
              b"rank 5's receive buffer"),
             ("swarm room, by the argument", {}, nout, nin, n + nin - 1, b"rank 0's swarm"),
             ("swarm room, by rank 7's row", {7: (AMPLE, AMPLE, int(want_counts[7]) - 1)}, nout, nin, capacity, b"rank 7's swarm")]
    for what, rooms, send_cap, recv_cap, swarm_cap, names in cases:
        lb = Loopback(gpu_device, R, incoming, per_rank, rooms)
        md.sv.capacity = swarm_cap
        try:
            st, nsent, nrecv, moved = _exchange(md, lb, 0, n, R, send, send_cap, recv, recv_cap)
        finally:
            md.sv.capacity = capacity
        assert st == _lib.JB_ERR_CAPACITY and names in md.lib.jb_last_error(), (what, st, md.lib.jb_last_error())
        assert (nsent, nrecv, moved) == (nout, nin, nout + nin), what          # what THIS rank needs
        untouched(lb, what)
    # one outgoing photon whose block rank 0 owns
    own = som.copy(sw)
    slot = int(np.flatnonzero(sw["status"] == som.ST_OUTGOING)[5])
    own["blk"][slot] = int(g.gids[0])
    assert g.owner[own["blk"][slot]] == 0
    _upload(md, own, gpu_device)
    md.reserve(n + nin)
    lb = Loopback(gpu_device, R, incoming, per_rank)
    st, _, _, _ = _exchange(md, lb, 0, n, R, send, nout, recv, nin)
    assert st == _lib.JB_ERR_INVALID and b"rank 0 hands particles to itself" in md.lib.jb_last_error()
    assert lb.exchanges == 0 and som.differing(_download(md, n), own) == []
    assert bool((send == FILL).all()) and bool((recv == FILL).all())
    # with room, and without that photon: the exchange goes through
    _upload(md, sw, gpu_device)
    md.reserve(n + nin)
    lb = Loopback(gpu_device, R, incoming, per_rank)
    st, nsent, nrecv, moved = _exchange(md, lb, 0, n, R, send, nout, recv, nin)
    _check(md, st)
    want, want_edelta = som.unpack(g, after, n, rec, base)
    assert (nsent, nrecv, moved) == (nout, nin, nout + nin) and _segments_equal(lb.sent, lb.sc, lb.so, segments)
    assert md.n == n + nin and som.differing(_download(md, n + nin), want) == []
    assert np.array_equal(_edelta(md).view(np.uint64), want_edelta.view(np.uint64))
