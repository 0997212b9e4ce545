"""The cost of the radiation spectrum (include/jaybenne_amd.h: jb_evaluate_radiation_spectrum) against
jb_evaluate_radiation_moments on the same swarm in the same process.  The swarm is in (block, cell) order already -- the
sort is not what is timed.  HIP events around single calls, the two calls alternating, ``--warmup`` rounds first, then
the median of ``--runs`` with min and max.  The traffic the two calls have to move:

    spectrum    24 B per photon (w, e, the key's write and read) + 8 (ngroups + 2) B per cell
    moments     40 B per photon (w, vx, vy, vz, the key's write and read) + 104 B per cell

at the 6.3 TB/s a streaming kernel reaches on an MI355X.  One JSON line per workload.

    python tools/dev/spectrum_cost.py --workload c2                          # 64 blocks of 64^3 cells, 1e7 photons
    python tools/dev/spectrum_cost.py --workload c3 --particles 100000000    # 128^3 cells in 8 blocks, all DDMC

``--edges quantiles`` (the default) puts the edges at quantiles of the photons' energies, so that every bin is occupied
in every wave: the dearest case.  ``--edges linear`` puts them at equal steps up to 3.3 times the median energy; the
bench decks' census spans decades, so nearly all photons then fall into the two outer bins: the cheapest case.
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
    ap.add_argument("--ngroups", type=int, default=16)
    ap.add_argument("--edges", default="quantiles", choices=["quantiles", "linear"])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    drv = mcblock.McblockDriver(make_deck(1, args.particles, 64, args.workload), device=dev)
    md = drv.md
    drv.Step()                                  # a census swarm, as a host meets it between two cycles
    jb.DefragParticles(md)

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

    cells = md.nblocks * drv.mesh.ncell
    ng = args.ngroups
    e = md.swarm["e"][:md.n]
    if args.edges == "quantiles":
        # every bin occupied in every wave: quantiles of a sample of the photons' energies
        q = (torch.arange(ng + 1, dtype=torch.float64, device=dev) + 1.0) / (ng + 2)
        edges = np.unique(torch.quantile(e[::max(1, md.n // 1_000_000)].double(), q).cpu().numpy())
    else:
        edges = float(e.median().item()) / 3.5 * 12.0 * (np.arange(ng + 1) + 0.5) / (ng + 1)
    assert len(edges) == ng + 1 and np.all(np.isfinite(edges)), "the photons' energies do not make ngroups + 1 edges"
    edges = np.ascontiguousarray(edges)
    mom_d = torch.empty(int(md.lib.jb_moments_words(md.handle)), dtype=torch.float64, device=dev)
    spec_d = torch.empty(int(md.lib.jb_spectrum_words(md.handle, ng)), dtype=torch.float64, device=dev)
    mrep, srep = _lib.MomentsReport(), _lib.SpectrumReport()

    def moments(report):
        _lib.check(md.lib.jb_evaluate_radiation_moments(md.pkg.ctx, md.handle, C.byref(md.sv), mom_d.data_ptr(),
                                                        C.byref(mrep) if report else None))

    def spectrum(report):
        _lib.check(md.lib.jb_evaluate_radiation_spectrum(md.pkg.ctx, md.handle, C.byref(md.sv), edges.ctypes.data, ng,
                                                         spec_d.data_ptr(), C.byref(srep) if report else None))

    calls = (("spectrum", lambda: spectrum(False)), ("moments", lambda: moments(False)),
             ("spectrum_report", lambda: spectrum(True)), ("moments_report", lambda: moments(True)))
    times = {name: [] for name, _ in calls}
    for r in range(args.warmup + args.runs):    # (the first rounds: warm-up, the scratch allocation included)
        for name, fn in calls:
            t = timed(fn)
            if r >= args.warmup:
                times[name].append(t)
    torch.cuda.synchronize(dev)
    assert mrep.sorted == 0 and srep.sorted == 0, "the swarm was to be in order already"
    n = md.n
    spec_bytes, mom_bytes = 24 * n + 8 * (ng + 2) * cells, 40 * n + 104 * cells
    # the spectrum's bin 1 .. ngroups + the two outer bins add up to the moments' E: the same photons were read
    total = spec_d.view(ng + 2, -1).sum(0)
    E = mom_d.view(_lib.JB_MOMENTS, -1)[1]
    rel = float(((total - E).abs().max() / E.abs().max()).item())
    res = dict(workload=args.workload, edges=args.edges, photons=n, cells=cells, photons_per_cell=round(n / cells, 3), ngroups=ng,
               runs=args.runs, warmup=args.warmup, report=srep.as_dict(), sum_of_bins_vs_moments_e=rel,
               device=torch.cuda.get_device_name(0))
    for name in times:
        res[name + "_ms"] = spread(times[name])
    ratio = [s / m for s, m in zip(times["spectrum"], times["moments"])]
    res["spectrum_over_moments"] = dict(median=round(statistics.median(ratio), 3), min=round(min(ratio), 3), max=round(max(ratio), 3))
    res["traffic_bytes"] = dict(spectrum=spec_bytes, moments=mom_bytes, ratio=round(spec_bytes / mom_bytes, 3))
    res["traffic_ms"] = dict(spectrum=round(spec_bytes / (STREAM_TB_PER_S * 1e12) * 1e3, 4),
                             moments=round(mom_bytes / (STREAM_TB_PER_S * 1e12) * 1e3, 4))
    res["spectrum_over_traffic"] = round(res["spectrum_ms"]["median"] / res["traffic_ms"]["spectrum"], 2)
    res["moments_over_traffic"] = round(res["moments_ms"]["median"] / res["traffic_ms"]["moments"], 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
