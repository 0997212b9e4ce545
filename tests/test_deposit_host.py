"""Exact deposition (include/jaybenne_amd.h: jb_set_deposition) without a GPU: the fixed-point arithmetic of
jaybenne_amd/csrc/jb_deposit_fixed.hpp on the host against vectors written by tests/deposit_model.py
(tests/deposit_test.cpp, once plainly and once under the address and undefined-behaviour sanitizers -- a
stand-alone program), the model against math.fsum, the deck key, the exports, and the conditions of the GPU cases
on the CPU oracle."""
import math
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import deposit_cases as dc
import deposit_model as dm
from helpers import ROOT, load_deck

HEADER = os.path.join(ROOT, "include", "jaybenne_amd.h")


def _dbl(sig, e):
    """the double with significand bits ``sig`` (52 bits) and biased exponent ``e``"""
    return dm.from_bits((e << 52) | sig)


def _words(a):
    return " ".join(f"{(a >> (64 * q)) & ((1 << 64) - 1):x}" for q in range(4))


def _vectors(path):
    rng = random.Random(20251)
    F, T, A, S, R = [], [], [], [], []
    E = 1023
    # ---- double -> words: every word boundary, the edge of exactness, the headroom, what adds nothing
    ws = [1.0, 1.5, _dbl((1 << 52) - 1, 1023), 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308,
          0.0, -0.0, -3.0, math.inf, -math.inf, math.nan]
    ws += [_dbl(rng.getrandbits(52) | 1, E - 170 + d) for d in (-60, -53, -52, -2, -1, 0, 1, 5, 6, 7)]
    ws += [_dbl(rng.getrandbits(52), E + d) for d in (-107, -106, -43, -42, 20, 21, 22, 32, 33, 34, 500)]
    for w in ws:
        for e in (E, 1, 2046, E + 3):
            F.append((w, e))
    for _ in range(300):
        F.append((_dbl(rng.getrandbits(52), rng.randrange(0, 2047)), rng.randrange(1, 2047)))
    # ---- words -> double: ties to even, carries, subnormal and overflowing results
    As = [1, (1 << 53) - 1, 1 << 53, (1 << 53) + 1, (1 << 53) + 2, (1 << 53) + 3,        # ties: down to even, up to even
          (1 << 54) + 2, (1 << 54) + 6, ((1 << 53) - 1) << 1 | 1,                        # the tie that carries into 2^54
          (1 << 117) + (1 << 64), (1 << 117) + (1 << 64) + 1, (1 << 117) + (1 << 64) - 1,  # guard bit alone / + sticky
          (1 << 192) - 1, (1 << 128) - 1, (1 << 255) - 1, 1 << 255, (1 << 256) - 1,        # all ones: rounds up a word
          ((1 << 53) | 1) << 139, (((1 << 53) | 1) << 139) | 1, (3 << 52 | 1) << 75]
    As += [rng.getrandbits(rng.randrange(1, 257)) for _ in range(300)]
    for a in As:
        for e in (E, 1, 30, 170, 171, 190, 2046, 1245, 2300 - 1075):      # (small E: subnormal results; large: overflow)
            if 1 <= e <= 2046:
                T.append((a, e))
    # ---- adds with carries through one, two and three words
    ones = (1 << 64) - 1
    A += [(ones, 1), (ones | ones << 64, 1), (ones | ones << 64 | ones << 128, 1), (dm.MASK, 1), (1 << 63, 1 << 63),
          (ones << 64, 1 << 64), (ones | ones << 128, 1)]
    A += [(rng.getrandbits(256), rng.getrandbits(256)) for _ in range(200)]
    # ---- 2^32 x the largest weight: the accumulator itself (2^32 adds are too many to write out), and 4096 of them
    # added one by one; then mixed magnitudes whose sum needs every word
    big = _dbl((1 << 52) - 1, E)
    big_acc = dm.from_double(big, E)[1] << 32
    assert big_acc >> 255 == 0 and dm.to_double(big_acc, E) == big * 2.0 ** 32
    T.append((big_acc, E))
    S.append((E, [big] * 4096))
    S.append((E, [_dbl(rng.getrandbits(52), E - rng.randrange(0, 171)) for _ in range(500)]))
    S.append((E, [_dbl(rng.getrandbits(52), E + 32)] * 2))                 # the headroom's last binary order
    S.append((40, [_dbl(rng.getrandbits(52), rng.randrange(0, 41)) for _ in range(300)]))   # subnormal addends and sums
    S.append((E, [1.0, _dbl(0, E - 53), _dbl(0, E - 170)]))               # a tie broken by a bit 117 orders below
    # ---- the accumulator moved to a raised scale: across every word boundary, with and without bits falling off
    for a in (1, 1 << 64, (1 << 222) | 1, dm.MASK, ((1 << 53) - 1) << 98, 1 << 255):
        for s_ in (1, 40, 63, 64, 65, 98, 99, 128, 191, 192, 255, 256, 300):
            R.append((a, s_))
    R += [(rng.getrandbits(256), rng.randrange(1, 260)) for _ in range(200)]
    with open(path, "w") as f:
        for a, s_ in R:
            r, dropped = dm.shift_right(a, s_)
            f.write(f"R {_words(a)} {s_:x} {_words(r)} {int(dropped):x}\n")
        for w, e in F:
            st, a = dm.from_double(w, e)
            f.write(f"F {dm.bits(w):x} {e:x} {st:x} {_words(a)}\n")
        for a, e in T:
            got = dm.to_double(a, e)
            assert dm.bits(got) == dm.bits(dm.to_double_explicit(a, e)), (hex(a), e)
            f.write(f"T {_words(a)} {e:x} {dm.bits(got):x}\n")
        for a, b in A:
            f.write(f"A {_words(a)} {_words(b)} {_words((a + b) & dm.MASK)}\n")
        for e, ws_ in S:
            acc, n_add, n_trunc, _ = dm.accumulate(ws_, [0] * len(ws_), 1, e)
            if n_trunc == 0 and not dm.top_bit(acc):
                assert dm.to_double(acc[0], e) == math.fsum(ws_)
            f.write(f"S {e:x} {len(ws_):x} " + " ".join(f"{dm.bits(w):x}" for w in ws_) + f" {dm.bits(dm.to_double(acc[0], e)):x}\n")
    return len(F) + len(T) + len(A) + len(S) + len(R)


@pytest.mark.parametrize("sanitize", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")],
                         ids=["plain", "sanitized"])
def test_fixed_point_arithmetic_on_the_host(tmp_path, sanitize):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe, vec = str(tmp_path / "deposit_test"), str(tmp_path / "vectors.txt")
    assert _vectors(vec) > 1000
    res = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *sanitize,
                          os.path.join(ROOT, "tests", "deposit_test.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe, vec], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.startswith("ok"), run.stdout[-3000:] + run.stderr[-3000:]


# ---- the model ------------------------------------------------------------------------------------
def test_the_layout_of_the_model():
    assert dm.from_double(1.0, 1023) == (dm.ADDED, 1 << 222)
    assert dm.from_double(2.0 ** 32, 1023) == (dm.ADDED, 1 << 254)
    assert dm.from_double(2.0 ** 33, 1023) == (dm.ADDED, 1 << 255)          # the top bit: the close turns it down
    assert dm.from_double(2.0 ** 34, 1023) == (dm.ADDED, 1 << 255)
    # 2^32 addends of the largest weight stay below the top bit
    st, big = dm.from_double(dm.from_bits((1023 << 52) | ((1 << 52) - 1)), 1023)
    assert st == dm.ADDED and (big << 32) >> 255 == 0
    # exact down to E - 170, truncated -- never rounded -- below
    w = dm.from_bits(((1023 - 170) << 52) | 1)
    assert dm.from_double(w, 1023) == (dm.ADDED, (1 << 52) | 1)
    assert dm.from_double(w / 2, 1023) == (dm.TRUNCATED, 1 << 51)
    assert dm.from_double(dm.from_bits(((1023 - 171) << 52) | 3), 1023) == (dm.TRUNCATED, (1 << 51) | 1)
    assert dm.from_double(2.0 ** -300, 1023) == (dm.TRUNCATED, 0)
    for bad in (0.0, -1.0, math.inf, math.nan):
        assert dm.from_double(bad, 1023) == (dm.REJECTED, 0)
    assert dm.scale([0.0, -5.0, math.nan]) == 1 and dm.scale([3.0, 1e-300, math.inf]) == 1024


@pytest.mark.parametrize("spread", [0, 60, 150])
def test_the_model_equals_fsum_while_nothing_is_truncated(spread):
    rng = np.random.default_rng(7 + spread)
    n, ncells = 4000, 13
    w = np.ldexp(rng.integers(1 << 52, 1 << 53, n).astype(np.float64), rng.integers(-60, spread - 59, n).astype(np.int32))
    cell = rng.integers(0, ncells, n)
    cell[:1500] = 5
    E = dm.scale(w)
    acc, n_add, n_trunc, n_rej = dm.accumulate(w, cell, ncells, E)
    assert (n_add, n_trunc, n_rej) == (n, 0, 0)
    want = np.array([math.fsum(w[cell == c]) for c in range(ncells)])
    assert np.array_equal(dm.field(acc, E), want)
    perm = rng.permutation(n)
    assert dm.accumulate(w[perm], cell[perm], ncells, E)[0] == acc
    # ... and any scale that truncates nothing gives the same doubles
    assert np.array_equal(dm.field(dm.accumulate(w, cell, ncells, E + 11)[0], E + 11), want)


def test_truncation_depends_on_the_addend_and_the_scale_alone():
    rng = np.random.default_rng(3)
    n = 3000
    w = np.ldexp(rng.integers(1 << 52, 1 << 53, n).astype(np.float64), rng.integers(-52, 149, n).astype(np.int32))
    cell = rng.integers(0, 4, n)
    E = dm.scale(w)
    acc, n_add, n_trunc, _ = dm.accumulate(w, cell, 4, E)
    assert n_add == n and 0 < n_trunc < n
    perm = rng.permutation(n)
    assert dm.accumulate(w[perm], cell[perm], 4, E) == (acc, n_add, n_trunc, 0)
    got, want = dm.field(acc, E), np.array([math.fsum(w[cell == c]) for c in range(4)])
    # (the exact sum loses less than one unit of bit 0 per addend: rounded once, it is fsum or the double below it)
    assert n * 2.0 ** (E - dm.BIAS) < np.spacing(want).min()
    assert np.all(got <= want) and np.all(want - got <= np.spacing(want))


# ---- the deck key, the exports ----------------------------------------------------------------------
@pytest.mark.parametrize("value, want", [("exact", "exact"), ("atomic", "atomic"), (None, None)])
def test_deck_key_sets_the_mode(value, want):
    from jaybenne_amd import jaybenne as jb, mcblock, _lib
    pin = load_deck("stepdiff", {} if value is None else {"jaybenne_amd/deposition": value})
    assert mcblock.deck_deposition(pin) == want
    assert jb.deposition_code("exact") == _lib.DEPOSIT_EXACT and jb.deposition_code("atomic") == _lib.DEPOSIT_ATOMIC


@pytest.mark.parametrize("value", ["EXACT", "on", "1", "fixed"])
def test_a_wrong_value_names_the_key(value):
    from jaybenne_amd import jaybenne as jb, mcblock
    with pytest.raises(ValueError, match="jaybenne_amd/deposition"):
        mcblock.deck_deposition(load_deck("stepdiff", {"jaybenne_amd/deposition": value}))
    with pytest.raises(ValueError, match="deposition"):
        jb.deposition_code(value)


def test_symbols_are_exported_and_declared():
    from jaybenne_amd import _lib
    lib = _lib.load()
    text = open(HEADER).read()
    for name in ("jb_set_deposition", "jb_get_deposition", "jb_deposit_accumulate", "jb_deposit_close", "jb_deposit_last",
                 "jb_deposit_memory", "jb_deposit_kernel_launches"):
        assert name in _lib.PROTOTYPES
        assert getattr(lib, name) is not None
        assert re.search(r"\b" + name + r"\(", text), name
    assert re.search(r"enum \{ JB_DEPOSIT_ATOMIC = 0, JB_DEPOSIT_EXACT = 1 \}", text)
    assert re.search(r"enum \{ JB_DEPOSIT_ABSORBED = 1, JB_DEPOSIT_ARRIVALS = 2 \}", text)
    assert (_lib.DEPOSIT_ATOMIC, _lib.DEPOSIT_EXACT, _lib.JB_DEPOSIT_ABSORBED, _lib.JB_DEPOSIT_ARRIVALS) == (0, 1, 1, 2)
    # the struct, field for field
    body = re.search(r"typedef struct jb_deposit_stats \{(.*?)\} jb_deposit_stats;", text, re.S).group(1)
    names = re.findall(r"int(?:64|32)_t (\w+);", body)
    assert names == [n for n, _ in _lib.DepositStats._fields_]
    # no context exists without a GPU: null pointers are turned down before anything is touched
    assert lib.jb_set_deposition(None, _lib.DEPOSIT_EXACT) == _lib.JB_ERR_INVALID
    assert b"jb_set_deposition" in lib.jb_last_error()
    assert lib.jb_get_deposition(None) == _lib.DEPOSIT_ATOMIC
    assert lib.jb_deposit_close(None, None, None) == _lib.JB_ERR_INVALID
    assert lib.jb_deposit_last(None, None) == _lib.JB_ERR_INVALID
    assert lib.jb_deposit_memory(None) == 0 and lib.jb_deposit_kernel_launches(None) == 0


def test_the_cpp_host_reads_the_same_key(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    src = r'''
#include <cstdio>
#include <cstring>
#include "jaybenne_amd.hpp"
int main() {
  int bad = 0;
  for (const char *v : {"EXACT", "on", "1", ""}) {
    try { (void)jaybenne_amd::DepositionOf(v); } catch (const std::invalid_argument &e) {
      bad += std::strstr(e.what(), "jaybenne_amd/deposition") != nullptr;
    }
  }
  std::printf("%d %d %d\n", jaybenne_amd::DepositionOf("atomic"), jaybenne_amd::DepositionOf("exact"), bad);
}
'''
    (tmp_path / "t.cpp").write_text(src)
    exe = str(tmp_path / "t")
    res = subprocess.run([cxx, "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.cpp"),
                          "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.split() == ["0", "1", "4"], run.stdout + run.stderr


# ---- the conditions of the GPU cases, on the oracle ---------------------------------------------------
# (case, cycles the GPU tests run it for)
@pytest.mark.parametrize("name, cycles", [("imc-1d", 3), ("ddmc-1d", 1), ("imc-3d-smr", 1), ("imc-3d", 1),
                                          ("hybrid-2d", 1)])
def test_every_gpu_case_absorbs_enough_and_truncates_nothing(name, cycles):
    """In every cycle: >= 100 absorbed photons, >= 10 cells that receive >= 2 addends, and n_truncated == 0 in the
    model at the scale of the swarm the transport call follows."""
    for c, rec in enumerate(dc.oracle_absorbed(name, cycles)):
        n_abs, cells2, n_trunc = dc.conditions(rec)
        spread = dm.scale(rec["w_all"]) - min(dm.exponent(float(x)) for x in rec["w_all"] if x > 0)
        print(f"{name} cycle {c + 1}: {n_abs} absorbed, {cells2} cells with >= 2 addends, {n_trunc} truncated, "
              f"weights over {spread} binary orders")
        assert n_abs >= 100 and cells2 >= 10 and n_trunc == 0
        assert spread < 170
