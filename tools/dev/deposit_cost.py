"""The cost of exact deposition (include/jaybenne_amd.h: jb_set_deposition) against the default, atomic one, both in
one run: whole RadiationSteps alternately in JB_DEPOSIT_ATOMIC and JB_DEPOSIT_EXACT on the same driver, timed with
HIP events behind one warm-up step per mode, median of ``--runs`` with min and max; then the pieces of the exact
mode alone on the swarm the steps left -- one absorbed sweep over all slots and one close (its census sweep and two
passes over the cells) -- next to the bytes they have to move:

    sweep   4 B of status per slot, + 8 (w) + 16 (blk, ip, jp, kp) + 8 (id) per counted slot
    close   32 B read and 8 B written per cell, twice; 4 B per slot + 8 + 16 per ACTIVE slot for the census sweep

The reference point is the ATOMIC step of the same run.  One JSON line per workload.

    python tools/dev/deposit_cost.py --workload c2        # 64 blocks of 64^3 cells, pure IMC (the headline)
    python tools/dev/deposit_cost.py --workload c3        # 128^3 cells in 8 blocks of 64^3, every step DDMC
    python tools/dev/deposit_cost.py --workload c3-1d     # the 1-D deck: 128 cells, the LDS form of the sweep
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    import torch
    from bench import make_deck
    from jaybenne_amd import _lib, mcblock
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2", choices=["c2", "c3", "c3-1d"])
    ap.add_argument("--particles", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    pin = make_deck(1, args.particles, 64, args.workload)
    drv = mcblock.McblockDriver(pin, device=dev)
    md = drv.md

    def timed(fn):
        md._sync_stream()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b)

    def spread(ts):
        return dict(median=round(statistics.median(ts), 3), min=round(min(ts), 3), max=round(max(ts), 3))

    times = {"atomic": [], "exact": []}
    for r in range(args.runs + 1):              # (the first pair: warm-up, the accumulators' allocation included)
        for mode in ("atomic", "exact"):
            md.deposition = mode
            t = timed(drv.Step)
            if r > 0:
                times[mode].append(t)
    mesh = drv.mesh
    cells = mesh.nblocks * mesh.ncell
    out = dict(workload=args.workload, photons=md.n, cells=cells, runs=args.runs,
               variant=md.lib.jb_last_transport_variant(md.handle).decode(),
               step_ms_atomic=spread(times["atomic"]), step_ms_exact=spread(times["exact"]),
               deposit_last=md.deposit_history[-1])
    out["exact_over_atomic"] = round(out["step_ms_exact"]["median"] / out["step_ms_atomic"]["median"], 4)
    # the pieces alone, on the census swarm the steps left (every slot ACTIVE: the absorbed sweep reads the status only)
    md.deposition = "exact"
    n = md.n
    both = _lib.JB_DEPOSIT_ABSORBED | _lib.JB_DEPOSIT_ARRIVALS
    sweeps, closes = [], []
    for r in range(args.runs + 1):
        t_s = timed(lambda: _lib.check(md.lib.jb_deposit_accumulate(md.pkg.ctx, md.handle, C.byref(md.sv), 0, n, both)))
        t_c = timed(lambda: _lib.check(md.lib.jb_deposit_close(md.pkg.ctx, md.handle, C.byref(md.sv))))
        if r > 0:
            sweeps.append(t_s)
            closes.append(t_c)
    st = md.deposit_last()
    out["sweep_ms"] = spread(sweeps)              # (with the scale pass of a first accumulate: 8 B of w per slot)
    out["close_ms"] = spread(closes)
    out["sweep_bytes_model"] = 4 * n + 8 * n + 32 * st["n_absorbed_addends"]
    # (the close here: one pass over the cells -- nothing absorbed is open --, the census scale pass and sweep)
    out["close_bytes_model"] = 40 * cells + 2 * 4 * n + (8 + 8 + 16) * st["n_census_addends"]
    out["close_gb_per_s"] = round(out["close_bytes_model"] / (out["close_ms"]["median"] * 1e-3) / 1e9, 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
