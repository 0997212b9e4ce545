"""Three trims of k_imc_cell's pass against the forms they replace.

The release library forms the high word of the nudge with one `v_bitop3_b32`, carries the mask of running lanes from
the end of a pass to the top of the next, and finds the scatter's azimuth grid point by adding 2^44 + 2^43 instead of
converting to an integer and back (jaybenne_amd/csrc: jb_physics.hpp, jb_kernel_imc.hpp, jb_math.hpp).
`-DJB_IMC_PARENT_FORMS` (`make -C jaybenne_amd/csrc parent_forms`) switches all three back; that library is the
reference here.

* bit equality: the five cases of tests/test_gpu_imc_nudge.py, two cycles of lean arithmetic under either library,
  each in a fresh child process; by photon id every integer attribute and the stream state equal, every floating
  attribute equal as uint64, event and outcome counts equal, the tally (and edelta where the material absorbs) within
  1e-15 of its largest entry (atomics add in any order);
* the azimuth reduction on raw inputs: debug cases 16 / 17 (the new reduction) against 9 / 10 (the conversion form),
  sine and cosine equal as uint64 on the grid points and their neighbours, the ends of (0, 1), the generator's
  uniforms next to every tie, and 2^20 uniforms drawn as LcgRng draws them.  At a true tie (256 u = n + 1/2, which
  no generator uniform is) the two forms pick different grid points where n is even (1/512: 0 by ties-to-even, 1 by
  floor) and may return different bits; both stay within their stated error, and `scatter_dir` on the tape generator
  (`jb_debug_sample_call` 5: the one place a TapeRng reaches the trait) returns the conversion form's bits at every
  tie;
* the kernels that inherit the azimuth reduction through `scatter_dir` without being `k_imc_cell`: the 3-D case on
  the lean x-space kernel (`k_transport`, JB_NO_IMC_CELL=1) and a 2-D IMC / DDMC mesh (`k_hybrid`), release against
  parent forms in the same way;
* the 3-D case under the checked library: no invariant violation.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_imc_nudge import CASES, CYCLES, FLT_KEYS, INT_KEYS, _child
from test_gpu_invariants import CHECKED, RELEASE, ROOT, TESTS, _clean, checked_lib  # noqa: F401  (checked_lib: fixture)
from test_gpu_parity import _dev_math, ctx  # noqa: F401  (ctx: fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.lean, pytest.mark.timeout(900, method="thread")]

PARENT = os.path.join(ROOT, "jaybenne_amd", "libjaybenne_amd_parent_forms.so")
LCG_MUL, LCG_INC = 6364136223846793005, 1442695040888963407      # jb_rng.hpp
C_LIGHT = 2.99792458e10


@pytest.fixture(scope="module")
def parent_lib():
    """The three earlier forms in one library: built once (a no-op when it is up to date)."""
    res = subprocess.run(["make", "-C", os.path.join(ROOT, "jaybenne_amd", "csrc"), "parent_forms"],
                         capture_output=True, text=True, timeout=840)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    return PARENT


# ---- 1. release against the parent forms -----------------------------------------------------------------------
def _compare(cid, a, ia, b, ib, noabs):
    print(f"{cid}: {ia['n0']} photons, {ia['events']} events in {CYCLES} cycles, stats {ia['stats']}")
    assert ia["n0"] == ib["n0"] and ia["events"] == ib["events"]
    for k in ("n_census", "n_absorbed", "n_escaped", "n_outgoing", "n_events"):
        assert ia["stats"][k] == ib["stats"][k], k     # (wave passes and services depend on the scheduling)
    assert ia["events"] >= 10 * ia["n0"]               # >= 10 events per history: scatters and crossings
    if not noabs:
        assert ia["stats"]["n_absorbed"] > 1000
    for cyc in range(CYCLES):
        assert np.array_equal(a[f"c{cyc}_events"], b[f"c{cyc}_events"]), cyc
        # (by id: the slot order moves with DefragParticles, whose schedule depends on timing)
        oa, ob = np.argsort(a[f"c{cyc}_id"]), np.argsort(b[f"c{cyc}_id"])
        assert oa.shape == ob.shape
        for k in INT_KEYS:
            assert np.array_equal(a[f"c{cyc}_{k}"][oa], b[f"c{cyc}_{k}"][ob]), (cyc, k)
        for k in FLT_KEYS:      # bit for bit (NaN-proof: compared as integers)
            x, y = a[f"c{cyc}_{k}"][oa], b[f"c{cyc}_{k}"][ob]
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (cyc, k)
        for k in ("tally",) if noabs else ("tally", "edelta"):
            x, y = a[f"c{cyc}_{k}"], b[f"c{cyc}_{k}"]
            scale = np.abs(y).max()
            assert scale > 0.0, k
            err = np.abs(x - y).max()
            print(f"  cycle {cyc + 1} {k}: largest difference {err / scale:.2e} of the largest entry")
            assert err <= 1e-15 * scale, (k, cyc, err, scale)


@pytest.mark.parametrize("cid", list(CASES))
def test_release_equals_the_parent_forms_bit_for_bit(gpu_device, parent_lib, tmp_path, cid):
    outs = {}
    for name, lib in (("release", RELEASE), ("parent", parent_lib)):
        info = _child(lib, "cycles", cid, tmp_path / f"{name}.npz")
        outs[name] = (np.load(tmp_path / f"{name}.npz"), info)
    (a, ia), (b, ib) = outs["release"], outs["parent"]
    _compare(cid, a, ia, b, ib, CASES[cid][3])


# The other callers of scatter_dir: id -> (deck, overrides, environment of the child, what the variant's name starts
# and ends with, NOABS).  The x-space kernel runs the 3-D case; the hybrid deck as tests/test_gpu_lean.py runs it.
OTHER = {
    "k_transport-lean-3d": (CASES["3d"][0], CASES["3d"][1], {"JB_NO_IMC_CELL": "1"}, ("k_transport<3, true,", "true>"),
                            True),
    "k_hybrid-2d": ("stepdiff_smr_hybrid", {"jaybenne/num_particles": 30000}, {}, ("k_hybrid<2,", ">"), True),
}


def child_other(cid, out):
    """As child_cycles of tests/test_gpu_imc_nudge.py, for a case of OTHER."""
    import torch
    from helpers import load_deck
    from jaybenne_amd import mcblock
    deck, ov, _, (head, tail), _ = OTHER[cid]
    drv = mcblock.McblockDriver(load_deck(deck, ov), device=torch.device("cuda", 0))
    assert drv.pkg.arithmetic() == "lean"
    sl = drv.mesh.interior()
    n0 = drv.md.n
    save = {}
    for cyc in range(CYCLES):
        drv.Step()
        v = drv.md.lib.jb_last_transport_variant(drv.md.handle).decode()
        assert v.startswith(head) and v.endswith(tail), v
        g = drv.md.get_swarm()
        for k in INT_KEYS + FLT_KEYS:
            save[f"c{cyc}_{k}"] = g[k]
        save[f"c{cyc}_tally"] = drv.md.get_field("tally")[sl]
        save[f"c{cyc}_edelta"] = drv.md.get_field("edelta")[sl]
        save[f"c{cyc}_events"] = np.array([drv.md.events, drv.md.n])
    np.savez(out, **save)
    return {"n0": n0, "events": int(drv.md.events), "stats": drv.md.stats(), "variant": v}


@pytest.mark.parametrize("cid", list(OTHER))
def test_other_callers_of_scatter_dir_equal_the_parent_forms(gpu_device, parent_lib, tmp_path, cid):
    outs = {}
    for name, lib in (("release", RELEASE), ("parent", parent_lib)):
        env = dict(os.environ, JAYBENNE_AMD_LIB=lib, **OTHER[cid][2])
        out = tmp_path / f"{name}.npz"
        res = subprocess.run([sys.executable, os.path.abspath(__file__), cid, str(out)], capture_output=True, text=True,
                             env=env, timeout=280, cwd=ROOT)
        assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-6000:]
        outs[name] = (np.load(out), json.loads(res.stdout.strip().splitlines()[-1]))
    (a, ia), (b, ib) = outs["release"], outs["parent"]
    print(cid, ia["variant"])
    assert ia["variant"] == ib["variant"]
    _compare(cid, a, ia, b, ib, OTHER[cid][4])


# ---- 2. the azimuth reduction ----------------------------------------------------------------------------------
def _lcg_uniforms(states, steps):
    """`steps` draws of each of the streams starting at `states`, as LcgRng::drand forms them."""
    s = np.asarray(states, dtype=np.uint64).copy()
    out = np.empty((steps, s.size))
    with np.errstate(over="ignore"):
        for i in range(steps):
            s = s * np.uint64(LCG_MUL) + np.uint64(LCG_INC)
            out[i] = ((s >> np.uint64(12)).astype(np.float64) + 0.5) * 2.0 ** -52
    return out


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_replica_of_the_generator(ctx):
    """The host-side recurrence below really is the device's generator."""
    from jaybenne_amd import _lib
    state = 0x9e3779b97f4a7c15
    out = np.empty(257)
    fin = C.c_uint64(0)
    _lib.check(ctx.lib.jb_debug_draw_stream(ctx.ctx, state, out.size, out.ctypes.data, C.byref(fin)))
    assert _same_bits(out, _lcg_uniforms([state], 257)[:, 0])


def test_azimuth_reduction_equals_the_conversion_form(ctx):
    ulp = 2.0 ** -53
    grid = np.clip(np.arange(257) / 256.0, ulp, 1.0 - ulp)
    grid = np.concatenate([grid, np.nextafter(grid, 0.0), np.nextafter(grid, 1.0)])
    grid = grid[(grid > 0.0) & (grid < 1.0)]
    ends = np.array([ulp, 1.0 - ulp])
    # generator uniforms (k + 1/2) 2^-52 on either side of every tie 256 u = n + 1/2: k = (2 n + 1) 2^43 - 1 and
    # (2 n + 1) 2^43 put 256 u at n + 1/2 -+ 2^-45
    n = np.arange(256, dtype=np.int64)
    k = np.concatenate([(2 * n + 1) * 2 ** 43 - 1, (2 * n + 1) * 2 ** 43])
    ties = (k.astype(np.float64) + 0.5) * 2.0 ** -52
    assert np.all(np.abs(256.0 * ties - (np.floor(256.0 * ties) + 0.5)) <= 2.0 ** -44)
    assert not np.any(256.0 * ties == np.floor(256.0 * ties) + 0.5)
    seeds = np.random.default_rng(11).integers(0, 2 ** 63, 1024, dtype=np.int64).astype(np.uint64)
    drawn = _lcg_uniforms(seeds, 1024).ravel()
    assert drawn.size == 1 << 20 and drawn.min() > 0.0 and drawn.max() < 1.0
    for name, u in (("grid points and neighbours", grid), ("ends of (0, 1)", ends), ("next to a tie", ties),
                    ("2^20 generator uniforms", drawn)):
        assert _same_bits(_dev_math(ctx, 16, u), _dev_math(ctx, 9, u)), name
        assert _same_bits(_dev_math(ctx, 17, u), _dev_math(ctx, 10, u)), name


def test_a_true_tie_is_the_tape_generators_business(ctx):
    """u = (2 n + 1) / 512: 256 u is an integer plus one half.  The conversion form rounds it up, the magic constant to
    the even neighbour: the same grid point for odd n (3/512: 2 either way), so the same bits; grid points n + 1 and n
    for even n (1/512, 257/512), where the two reduce by -1/512 and +1/512 of a turn and may return different bits.
    No equality is asked there, only that each is the sine / cosine of 2 pi u: within its stated absolute error of
    1.7e-16 plus what the value it is compared with here may be off by, numpy's sin(fl(2 pi) u) -- an argument off by
    <= 2 pi (2^-53 + 3.9e-17) = 9.4e-16 and half a unit in the last place of the result, 1.1e-16: 1.3e-15 in all (a
    wrong grid point is off by 2 pi / 256 = 0.025).
    The tape generator can hold such a number, so scatter_dir on a tape (jb_debug_sample_call 5) must use the
    conversion form: its direction is (st cos, st sin, mu) with cases 10 / 9 of jb_debug_math at every tie -- and is
    not what cases 17 / 16 would give wherever those differ, 1/512 and 257/512 among them."""
    from jaybenne_amd import _lib
    n = np.arange(256)
    u = (2.0 * n + 1.0) / 512.0
    s9, c9 = _dev_math(ctx, 9, u), _dev_math(ctx, 10, u)
    s16, c16 = _dev_math(ctx, 16, u), _dev_math(ctx, 17, u)
    differ = (s9.view(np.uint64) != s16.view(np.uint64)) | (c9.view(np.uint64) != c16.view(np.uint64))
    print(f"true ties: the two reductions differ in {int(differ.sum())} of {u.size} inputs; at 1/512: {differ[0]}, "
          f"at 257/512: {differ[128]}")
    assert not differ[n % 2 == 1].any()          # the same grid point: the same bits
    assert differ[0] and differ[128]             # 1/512 and 257/512 tell the two forms apart
    for got, want in ((s9, np.sin), (s16, np.sin), (c9, np.cos), (c16, np.cos)):
        assert np.abs(got - want(2.0 * np.pi * u)).max() <= 1.3e-15
    # scatter_dir(TapeRng): (st cos, st sin, mu), mu = 2 xi1 - 1, st = the lean sqrt of 1 - mu^2 (jb_debug_math 14)
    xi1 = 0.3125
    mu = 2.0 * xi1 - 1.0
    st = _dev_math(ctx, 14, [1.0 - mu * mu])[0]
    a8 = np.zeros(8)
    i4 = np.zeros(4, dtype=np.int32)
    told_apart = 0
    for j in range(u.size):
        tape = np.array([xi1, u[j]])
        out = np.zeros(4); io = np.zeros(2, dtype=np.int32); nd = C.c_int(0)
        _lib.check(ctx.lib.jb_debug_sample_call(ctx.ctx, 5, a8.ctypes.data, i4.ctypes.data, tape.ctypes.data, tape.size,
                                                out.ctypes.data, io.ctypes.data, C.byref(nd)))
        assert nd.value == 2
        conversion = np.array([st * c9[j], st * s9[j], mu])
        magic = np.array([st * c16[j], st * s16[j], mu])
        assert _same_bits(out[:3], conversion), (u[j], out[:3], conversion)
        told_apart += not _same_bits(conversion, magic)
        if j in (0, 128):
            assert not _same_bits(out[:3], magic), (u[j], out[:3], magic)
    assert told_apart >= 2
    # ... and on a tape of generator-form uniforms the two agree, as in the kernels
    tape = np.array([xi1, (float(3 * 2 ** 43) + 0.5) * 2.0 ** -52])
    out = np.zeros(4); io = np.zeros(2, dtype=np.int32); nd = C.c_int(0)
    _lib.check(ctx.lib.jb_debug_sample_call(ctx.ctx, 5, a8.ctypes.data, i4.ctypes.data, tape.ctypes.data, tape.size,
                                            out.ctypes.data, io.ctypes.data, C.byref(nd)))
    cs, sn = _dev_math(ctx, 17, tape[1:])[0], _dev_math(ctx, 16, tape[1:])[0]
    assert _same_bits(out[:3], np.array([st * cs, st * sn, mu]))


# ---- 3. the checked library ------------------------------------------------------------------------------------
def test_checked_library_sees_no_violation(gpu_device, checked_lib, tmp_path):
    info = _child(CHECKED, "cycles", "3d", tmp_path / "checked.npz")
    rep = info["report"]
    _clean(rep)
    assert rep["passes"]["imc_cell"] > 0, rep


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, TESTS)
    print(json.dumps(child_other(sys.argv[1], sys.argv[2])))
