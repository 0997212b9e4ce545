"""The cost of the count path of SourcePhotons under both source allocations (include/jaybenne_amd.h:
jb_set_source_allocation) on the headline mesh, 64 blocks of 64^3 cells: UNIFORM (k_source_count alone) and ENERGY
(k_salloc_energy, the total on the host, k_salloc_count) alternately in one process.  HIP events around the library
calls -- so the read-backs of the per-block results and the host's part are inside --, one warm-up, median of
``--runs`` with min and max; the thermal source.  Beside them the byte model at the 6.3 TB/s a streaming kernel
reaches on an MI355X:

    uniform count   8 B read (sie), 20 B written (src_num, src_ew, prefix) per cell
    energy pass     16-24 B read (sie; rho and fleck for the emission source), 8 B written (src_ew) per cell
    count pass      8 B read (src_ew), 20 B written per cell

One JSON line.

    python tools/dev/source_alloc_cost.py
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

STREAM_TB_PER_S = 6.3


def main():
    import torch
    from bench import make_deck
    from jaybenne_amd import _lib, jaybenne as jb, mcblock
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--source", default="thermal", choices=["thermal", "emission"])
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    drv = mcblock.McblockDriver(make_deck(1, args.particles, 64, "c2"), device=dev, capacity_factor=2.5)
    md, ctx = drv.md, drv.pkg.ctx
    st = int(jb.SourceType[args.source])
    dt = drv.dt if args.source == "emission" else 0.0
    jb.UpdateDerivedTransportFields(md, drv.dt)
    nper = np.zeros(md.nblocks, dtype=np.int32)
    e_blk = np.zeros(md.nblocks)

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
        return dict(median=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4))

    def uniform():
        _lib.check(md.lib.jb_source_photons_count(ctx, md.handle, st, dt, 1, 1, nper.ctypes.data, md.prefix.data_ptr()))

    def energy_pass():
        _lib.check(md.lib.jb_source_energy_sums(ctx, md.handle, st, dt, e_blk.ctypes.data))

    def count_pass():
        e_tot = float(md.lib.jb_source_energy_total(e_blk.ctypes.data, md.nblocks))
        _lib.check(md.lib.jb_source_photons_count_energy(ctx, md.handle, st, dt, 1, e_tot, nper.ctypes.data,
                                                         md.prefix.data_ptr()))

    times = {"uniform": [], "energy_pass": [], "count_pass": []}
    totals = {}
    for r in range(args.runs + 1):              # (the first round: warm-up)
        md.source_allocation = "uniform"
        t = timed(uniform)
        totals["uniform"] = int(nper.sum())
        md.source_allocation = "energy"
        t1 = timed(energy_pass)
        t2 = timed(count_pass)
        totals["energy"] = int(nper.sum())
        if r > 0:
            times["uniform"].append(t)
            times["energy_pass"].append(t1)
            times["count_pass"].append(t2)
    cells = md.nblocks * drv.mesh.ncell
    read_e = 8 if args.source == "thermal" else 24
    model = {"uniform": 28 * cells, "energy_pass": (read_e + 8) * cells, "count_pass": 28 * cells}
    res = dict(workload="c2", source=args.source, cells=cells, num_particles=args.particles, runs=args.runs,
               photons=totals)
    for k in times:
        res[k + "_ms"] = spread(times[k])
        res[k + "_model_ms"] = round(model[k] / (STREAM_TB_PER_S * 1e12) * 1e3, 4)
    res["energy_ms_median"] = round(res["energy_pass_ms"]["median"] + res["count_pass_ms"]["median"], 4)
    res["energy_over_uniform"] = round(res["energy_ms_median"] / res["uniform_ms"]["median"], 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
