"""Ragged ranges through every tracking kernel: a swarm transported in one call over [0, n) and an identical copy
transported in consecutive calls over ranges of 1, 7, 8, 9, 63, 65, 511, 513, 1025 slots and the rest -- the number
of queues, a wave, queues x wave and queues x the 128-slot chunk, each minus and plus one -- end in the same bits.
Every seventh slot is a hole (status absorbed) that no kernel may touch.  What is under test is the dealing of slots
(jb_scaffold.hpp: the queue cursor, the exact claim, the chunk refill, the window of k_ddmc_all) and the counting of
finished histories: every live photon is followed once, every hole never, whatever the range."""
import numpy as np
import pytest

from helpers import load_deck

pytestmark = pytest.mark.gpu

LENGTHS = (1, 7, 8, 9, 63, 65, 511, 513, 1025)
SWITCHES = ("JB_NO_IMC_CELL", "JB_DDMC_QUEUES", "JB_COOP_GATHER", "JB_NO_DDMC_ALL", "JB_PER_EVENT_OPACITY")
N = {"jaybenne/num_particles": 2500}
IMC_3D = dict(N, **{"parthenon/mesh/nx2": 8, "parthenon/mesh/nx3": 8, "parthenon/mesh/nx1": 16,
                    "parthenon/meshblock/nx1": 8, "parthenon/meshblock/nx2": 4, "parthenon/meshblock/nx3": 4})
ST_ABSORBED = 1

# id, deck, overrides, DDMC entry point, switches, what jb_last_transport_variant must hold, lean arithmetic
CASES = [
    ("k_transport", "stepdiff", N, False, {}, ("k_transport<1, true,", "false>"), False),
    ("k_transport-lean", "stepdiff", N, False, {"JB_NO_IMC_CELL": "1"}, ("k_transport<1, true,", "true>"), True),
    ("k_imc_cell", "stepdiff", N, False, {}, ("k_imc_cell<1, true,",), True),
    ("k_imc_cell-3d", "stepdiff", IMC_3D, False, {}, ("k_imc_cell<3, true,",), True),
    ("k_ddmc_q", "stepdiff_ddmc", N, True, {"JB_DDMC_QUEUES": "1"}, ("k_ddmc_all<1, true", "queues"), False),
    ("k_ddmc_all-window", "stepdiff_ddmc", N, True, {"JB_DDMC_QUEUES": "0"}, ("k_ddmc_all<1, true", "records in LDS"),
     False),
    ("k_ddmc_all-quad", "stepdiff_ddmc", N, True, {"JB_COOP_GATHER": "1"}, ("k_ddmc_all<1, true", "quad gather"), False),
    ("k_hybrid-all-ddmc", "stepdiff_ddmc", N, True, {"JB_NO_DDMC_ALL": "1"}, ("k_hybrid<1",), False),
    ("k_hybrid", "stepdiff_smr_hybrid", N, True, {}, ("k_hybrid<2, exact",), False),
    ("k_hybrid-lean", "stepdiff_smr_hybrid", N, True, {}, ("k_hybrid<2, lean",), True),
    ("k_transport-ddmc", "stepdiff_smr_hybrid", N, True, {"JB_PER_EVENT_OPACITY": "1"}, ("k_transport<2, true, 0,",),
     False),
]
PARAMS = [pytest.param(*c[1:], marks=[pytest.mark.lean] if c[6] else [], id=c[0]) for c in CASES]
COUNTS = ("n_census", "n_absorbed", "n_escaped", "n_outgoing")


def _problem(deck, ov, device):
    """A freshly sourced swarm with every seventh slot turned into a hole, ready for the transport task."""
    from jaybenne_amd import jaybenne as jb
    from jaybenne_amd import mcblock
    drv = mcblock.McblockDriver(load_deck(deck, ov), device=device)
    md = drv.md
    assert md.n > sum(LENGTHS) + 1, md.n
    md.swarm["status"][0:md.n:7] = ST_ABSORBED
    jb.UpdateDerivedTransportFields(md, drv.dt)
    md.fields["tally"].zero_()
    return drv


def _transport(drv, ddmc, ranges):
    """The transport task over each of `ranges`; returns how many histories the counters say have ended."""
    from jaybenne_amd import jaybenne as jb
    before = drv.md.stats()
    for first, last in ranges:
        (jb.TransportPhotons_DDMC if ddmc else jb.TransportPhotons)(drv.md, 0.0, drv.dt, first, last,
                                                                   fuse_census_tally=True)
    after = drv.md.stats()
    return sum(after[k] - before[k] for k in COUNTS)


@pytest.mark.parametrize("deck,ov,ddmc,env,expect,lean", PARAMS)
def test_ragged_ranges_are_dealt_out_completely_once_and_only_where_live(gpu_device, monkeypatch, deck, ov, ddmc, env,
                                                                         expect, lean):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    whole, parts = _problem(deck, ov, gpu_device), _problem(deck, ov, gpu_device)
    assert whole.pkg.arithmetic() == ("lean" if lean else "exact")
    n = whole.md.n
    start = whole.md.get_swarm()
    start_parts = parts.md.get_swarm()
    for k in start:
        assert np.array_equal(start[k], start_parts[k]), k        # identical copies
    holes = np.zeros(n, dtype=bool)
    holes[::7] = True
    assert np.array_equal(start["status"] != 0, holes)
    live = int(n - holes.sum())

    ranges, first = [], 0
    for length in LENGTHS:
        ranges.append((first, first + length))
        first += length
    ranges.append((first, n))

    assert _transport(whole, ddmc, [(0, n)]) == live
    assert _transport(parts, ddmc, ranges) == live
    for drv in (whole, parts):
        v = drv.md.lib.jb_last_transport_variant(drv.md.handle).decode()
        assert v.startswith(expect[0]) and all(e in v for e in expect[1:]), v

    a, b = whole.md.get_swarm(), parts.md.get_swarm()
    assert whole.md.n == parts.md.n == n
    for k in a:
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a[k][holes], start[k][holes]), k   # the holes are untouched
    assert not np.array_equal(a["rng"][~holes], start["rng"][~holes])   # ... and the live photons were followed
    ta, tb = whole.md.get_field("tally"), parts.md.get_field("tally")
    assert ta.sum() > 0.0
    np.testing.assert_allclose(tb, ta, rtol=1e-12, atol=0)
