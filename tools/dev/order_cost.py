"""The cost of the canonical sort (include/jaybenne_amd.h: jb_set_cell_order) against the default one, both in one
run: ``jb_defrag_particles`` on the same scrambled swarm in JB_CELL_ORDER_ANY and in JB_CELL_ORDER_BY_ID, timed with
HIP events behind a warm-up, median of ``--runs``; and the canonical mode's call on a swarm that is in order already
(the check alone).  One JSON line per workload.

    python tools/dev/order_cost.py --workload c3 --particles 100000000     # 128^3 cells in 8 blocks of 64^3
    python tools/dev/order_cost.py --workload c3-1d --particles 100000000  # the 1-D deck: 7.8e5 photons per cell
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
    ap.add_argument("--workload", default="c3", choices=["c3", "c3-1d", "c1", "c2"])
    ap.add_argument("--particles", type=int, default=100_000_000)
    ap.add_argument("--cycles", type=int, default=2, help="transport cycles before the sorts (they scramble the order)")
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    pin = make_deck(1, args.particles, 64, args.workload)
    pin.load_string("<jaybenne>\ndefrag_interval = 0\n")
    drv = mcblock.McblockDriver(pin, device=dev)
    md = drv.md
    for _ in range(args.cycles):
        drv.Step()
    n = md.n
    keep = {k: v[:n].clone() for k, v in md.swarm.items()}

    def restore(src):
        for k, v in src.items():
            md.swarm[k][:n].copy_(v)
        md.sv.n = n

    def sort_ms():
        md._sync_stream()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        a.record()
        _lib.check(md.lib.jb_defrag_particles(md.pkg.ctx, md.handle, C.byref(md.sv)))
        b.record()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b)

    out = dict(workload=args.workload, photons=n, cycles=args.cycles, runs=args.runs)
    for mode in ("any", "id"):
        md.cell_order = mode
        times = []
        for r in range(args.runs + 1):          # (the first: warm-up, scratch allocation included)
            restore(keep)
            t = sort_ms()
            if r > 0:
                times.append(t)
        out[f"sort_ms_{mode}"] = round(statistics.median(times), 3)
        out[f"sort_ms_{mode}_all"] = [round(t, 3) for t in times]
    # in canonical order now: the call that only looks
    out["in_order_ms_id"] = round(statistics.median([sort_ms() for _ in range(args.runs)]), 3)
    ids = md.swarm["id"][:n]
    out["max_id"] = int(ids.max().item())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
