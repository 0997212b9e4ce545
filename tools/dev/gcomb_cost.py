"""The cost of the global census comb (include/jaybenne_amd.h: jb_comb_census_weigh / _plan_global / _apply) at the bench
sizes, on a census swarm after one step and a DefragParticles -- in (block, cell) order already, so the sort is not
what is timed.  HIP events around the three calls (their read-backs included), one warm-up, median of ``--runs`` with
min and max; the swarm is put back before every run.  N = n / 2 (thinning) and N = 2 n (splitting).  Reference points
from the same run: jb_defrag_particles alone, the per-cell comb at K = 25 (T = 50), and the byte model.  The move is
timed on its own too, by a pair of events around jb_comb_census_apply (k_gcomb_pack or k_comb_pack, k_sort_unpack and
the energy sum behind them): ``apply_ms`` -- to set beside the whole of jb_defrag_particles, whose move is k_sort_pack
and k_sort_unpack behind a histogram and a scan.  The byte model:

    keys 40 B + segmented scan 40 B + decide 28 B + two 4-byte scans 32 B per photon,
    one record move: 104 B read + 128 B written (pack), 128 B read + 104 B written (unpack) per OUTPUT photon

at the 6.3 TB/s a streaming kernel reaches on an MI355X.  One JSON line per workload and N.

    python tools/dev/gcomb_cost.py --workload c2                        # 64 blocks of 64^3 cells, 1e7 photons
    python tools/dev/gcomb_cost.py --workload c3 --particles 100000000  # 128^3 cells in 8 blocks, 1e8 photons
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

STREAM_TB_PER_S = 6.3


def main():
    import numpy as np
    import torch
    from bench import make_deck
    from jaybenne_amd import _lib, jaybenne as jb, mcblock
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2", choices=["c2", "c3", "c3-1d"])
    ap.add_argument("--particles", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    drv = mcblock.McblockDriver(make_deck(1, args.particles, 64, args.workload), device=dev)
    md = drv.md
    drv.Step()                                  # a census swarm, as a host meets it between two cycles
    jb.DefragParticles(md)
    n = md.n
    md.reserve(3 * n)
    md._sync_stream()
    keep = {k: v[:n].clone() for k, v in md.swarm.items()}

    def restore():
        for k, v in keep.items():
            md.swarm[k][:n].copy_(v)
        md.sv.n = n
        torch.cuda.synchronize(dev)

    def timed(fn):
        restore()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b), out

    apply_ms = {}

    def timed_apply(name, call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize(dev)
        apply_ms.setdefault(name, []).append(a.elapsed_time(b))

    def spread(ts):
        return dict(median=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4))

    def defrag():
        _lib.check(md.lib.jb_defrag_particles(md.pkg.ctx, md.handle, C.byref(md.sv)))

    def per_cell():
        plan, rep = _lib.CombPlan(), _lib.CombReport()
        _lib.check(md.lib.jb_comb_census_plan(md.pkg.ctx, md.handle, C.byref(md.sv), 50, 25, 1, C.byref(plan)))
        if plan.cells_combed > 0:
            timed_apply("per_cell_K25", lambda: _lib.check(
                md.lib.jb_comb_census_apply(md.pkg.ctx, md.handle, C.byref(md.sv), 1 << 40, C.byref(rep))))
        return dict(n_after=int(plan.n_after), cells_combed=int(plan.cells_combed))

    def global_comb(N, name):
        def run():
            plan, rep = _lib.CombGlobalPlan(), _lib.CombReport()
            e = np.zeros(md.nblocks)
            n_room = min(n + N, 64 * n)
            _lib.check(md.lib.jb_comb_census_weigh(md.pkg.ctx, md.handle, C.byref(md.sv), n_room, e.ctypes.data, C.byref(plan)))
            w_total = float(md.lib.jb_source_energy_total(e.ctypes.data, md.nblocks))
            _lib.check(md.lib.jb_comb_census_plan_global(md.pkg.ctx, md.handle, C.byref(md.sv), w_total, N, 2.0, 64, 1,
                                                         C.byref(plan)))
            if plan.cells_thinned + plan.cells_split > 0:
                timed_apply(name, lambda: _lib.check(
                    md.lib.jb_comb_census_apply(md.pkg.ctx, md.handle, C.byref(md.sv), 1 << 40, C.byref(rep))))
            assert plan.sorted == 0, "the swarm was to be in order already"
            return dict(n_after=int(plan.n_after), cells_thinned=int(plan.cells_thinned), cells_split=int(plan.cells_split),
                        max_per_cell=int(plan.max_per_cell), max_target=int(plan.max_target))
        return run

    cases = [("defrag", defrag), ("per_cell_K25", per_cell), ("global_half", global_comb(n // 2, "global_half")),
             ("global_double", global_comb(2 * n, "global_double"))]
    times = {name: [] for name, _ in cases}
    outs = {}
    for r in range(args.runs + 1):              # (the first round: warm-up, the scratch allocation included)
        for name, fn in cases:
            t, outs[name] = timed(fn)
            if r > 0:
                times[name].append(t)
    cells = md.nblocks * drv.mesh.ncell
    for name, N in (("global_half", n // 2), ("global_double", 2 * n)):
        n_after = outs[name]["n_after"]
        model = 140 * n + 464 * n_after
        res = dict(workload=args.workload, photons=n, cells=cells, target_N=N, runs=args.runs, plan=outs[name],
                   global_comb_ms=spread(times[name]), defrag_ms=spread(times["defrag"]),
                   per_cell_comb_ms=spread(times["per_cell_K25"]), per_cell_plan=outs["per_cell_K25"],
                   model_bytes=model, model_ms=round(model / (STREAM_TB_PER_S * 1e12) * 1e3, 4))
        # (the first entry of each list is the warm-up round's)
        res["apply_ms"] = spread(apply_ms[name][1:]) if len(apply_ms.get(name, [])) > 1 else None
        res["per_cell_apply_ms"] = spread(apply_ms["per_cell_K25"][1:]) if len(apply_ms.get("per_cell_K25", [])) > 1 else None
        if res["apply_ms"]:
            res["apply_ns_per_record"] = round(res["apply_ms"]["median"] * 1e6 / n_after, 4)
        if res["per_cell_apply_ms"]:
            res["per_cell_apply_ns_per_record"] = round(res["per_cell_apply_ms"]["median"] * 1e6 / outs["per_cell_K25"]["n_after"], 4)
        res["defrag_ns_per_record"] = round(res["defrag_ms"]["median"] * 1e6 / n, 4)
        res["over_model"] = round(res["global_comb_ms"]["median"] / res["model_ms"], 2)
        res["over_defrag"] = round(res["global_comb_ms"]["median"] / res["defrag_ms"]["median"], 2)
        res["over_per_cell_comb"] = round(res["global_comb_ms"]["median"] / res["per_cell_comb_ms"]["median"], 2)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
