"""The cost of the radiation moments (include/jaybenne_amd.h: jb_evaluate_radiation_moments) at the bench sizes, on a
swarm that is in (block, cell) order already -- the sort is not what is timed.  HIP events, one warm-up, median of
``--runs`` with min and max.  Two reference points from the same run: jb_evaluate_radiation_energy on the same swarm
(the zeroth moment alone, by atomics), and the byte model

    36 B per photon (w, vx, vy, vz and the key's write) + 4 B per key read + 96 B per cell

at the 6.3 TB/s a streaming kernel reaches on an MI355X.  One JSON line per workload.

    python tools/dev/moments_cost.py --workload c2        # 64 blocks of 64^3 cells: 0.6 photons per cell
    python tools/dev/moments_cost.py --workload c3        # 128^3 cells in 8 blocks: about 5 per cell at 1e7 photons
    python tools/dev/moments_cost.py --workload c3-1d     # the 1-D deck: 128 cells, 7.8e4 per cell at 1e7 photons
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
    out_d = torch.empty(int(md.lib.jb_moments_words(md.handle)), dtype=torch.float64, device=dev)
    rep = _lib.MomentsReport()

    def moments(report):
        _lib.check(md.lib.jb_evaluate_radiation_moments(md.pkg.ctx, md.handle, C.byref(md.sv), out_d.data_ptr(),
                                                        C.byref(rep) if report else None))

    def energy():
        _lib.check(md.lib.jb_evaluate_radiation_energy(md.pkg.ctx, md.handle, C.byref(md.sv)))

    times = {"moments": [], "moments_report": [], "energy": []}
    for r in range(args.runs + 1):              # (the first round: warm-up, the scratch allocation included)
        for name, fn in (("moments", lambda: moments(False)), ("moments_report", lambda: moments(True)),
                         ("energy", energy)):
            t = timed(fn)
            if r > 0:
                times[name].append(t)
    moments(True)
    torch.cuda.synchronize(dev)
    n = md.n
    model = 36 * n + 4 * n + 96 * cells
    res = dict(workload=args.workload, photons=n, cells=cells, photons_per_cell=round(n / cells, 3), runs=args.runs,
               report=rep.as_dict(), moments_ms=spread(times["moments"]), moments_with_report_ms=spread(times["moments_report"]),
               energy_tally_ms=spread(times["energy"]), model_bytes=model,
               model_ms=round(model / (STREAM_TB_PER_S * 1e12) * 1e3, 4))
    res["moments_over_model"] = round(res["moments_ms"]["median"] / res["model_ms"], 2)
    res["moments_over_energy_tally"] = round(res["moments_ms"]["median"] / res["energy_tally_ms"]["median"], 2)
    res["gb_per_s"] = round(model / (res["moments_ms"]["median"] * 1e-3) / 1e9, 1)
    assert rep.sorted == 0, "the swarm was to be in order already"
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
