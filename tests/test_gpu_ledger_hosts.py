"""The command-line hosts with ``--ledger FILE``: ``python -m jaybenne_amd`` and the native ``examples/mcblock_amd`` on
the C++ mirror write the same JSON lines for the same deck (G1-imc under RO: 1-D, reflecting wall left, open face
right), and what they write is the CPU oracle's ledger."""
import json
import os
import subprocess
import sys

import pytest

import axis_cases as ax
import ledger_cases as lc
from helpers import ROOT, DECK_DIR, load_deck, make_oracle

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "examples", "mcblock_amd")
# Sums whose INPUT is not the same bits in two runs of one problem: the fields the tracking kernels accumulate with
# atomics, and every sum over a swarm that a compaction has been through -- RemoveMarkedParticles pairs holes with
# movers through an atomic cursor, so the slot order, and with it the order of a sweep's additions, differs from run
# to run.  In the first cycle that is the census alone (the sweeps before it walk the initial order); from the second
# cycle on it is every energy.  Such terms agree between two runs to the project's 1e-12, as tests/test_gpu_parity.py
# compares such fields; counts, and every other term of the first cycle, must be equal.
FIELD_SUMS = ("e_tally", "e_delta", "e_material", "e_census")


def _near(x, y):
    x, y = (x, y) if isinstance(x, list) else ([x], [y])
    return all(abs(p - q) <= 1e-12 * abs(q) for p, q in zip(x, y))


def _run(cmd, env):
    res = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=240, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    return res.stdout


def test_both_hosts_write_the_oracles_ledger(gpu_device, tmp_path):
    from oracle import orc
    case = ax.BY_ID["G1-imc"]
    ov = ax.overrides(case, "RO")
    pin = load_deck(case.deck, ov)
    dt = pin.GetReal("jaybenne", "dt")
    ov["parthenon/time/tlim"] = 1.5 * dt                    # two cycles on either host
    args = ["-i", os.path.join(DECK_DIR, case.deck + ".in")] + [f"{k}={v}" for k, v in ov.items()]
    env = dict(os.environ, JB_EXACT_ARITH="1")
    env.pop("JB_LEDGER", None)
    assert os.path.exists(EXE), "examples/mcblock_amd has not been built (__graft_entry__.build())"
    out_py = _run([sys.executable, "-m", "jaybenne_amd"] + args + ["--ledger", str(tmp_path / "py.jsonl")], env)
    out_cc = _run([EXE] + args + ["--ledger", str(tmp_path / "cc.jsonl")], env)
    py = [json.loads(line) for line in open(tmp_path / "py.jsonl")]
    cc = [json.loads(line) for line in open(tmp_path / "cc.jsonl")]
    assert len(py) == len(cc) == 2
    # the oracle on the deck's own state (the hosts' ProblemGenerator), task by task
    O, _, _ = make_oracle(load_deck(case.deck, ov), orc.MATH_PORTABLE)
    t = 0.0
    for c, (a, b) in enumerate(zip(py, cc)):
        want = lc.oracle_cycle(O, pin, t)
        t += dt
        assert a.keys() == b.keys()
        for k in a:
            if k in FIELD_SUMS or (c > 0 and k.startswith("e_")):
                assert _near(a[k], b[k]), (c, k, a[k], b[k])
            elif k != "residual":
                assert a[k] == b[k], (k, a[k], b[k])
        for got in (a, b):
            assert got["n_escaped"] == want["n_escaped"] and got["n_census"] == want["n_census"]
            assert got["n_escaped"][1] >= 50 and sum(got["n_escaped"]) == got["n_escaped"][1]      # ox1 alone is open
            for k in ("e_census", "e_start", "e_tally"):
                assert abs(got[k] - want[k]) <= 1e-12 * want[k], (k, got[k], want[k])
            assert abs(got["e_escaped"][1] - want["e_escaped"][1]) <= 1e-12 * want["e_escaped"][1]
            assert got["n_escaped_unclassified"] == 0 and got["residual"] <= 1e-12
    for out in (out_py, out_cc):
        lines = [line for line in out.splitlines() if line.startswith("cycle=")]
        assert len(lines) == 2 and all(" leak=[" in line and " residual=" in line for line in lines), out
        assert "leakage by face:" in out and "ox1=" in out
