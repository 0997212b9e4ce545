"""The regression decks' error number -- the mean weighted fractional error against the analytic solution that
`python -m jaybenne_amd --tolerance` gates (stepdiff 0.05, stepdiff_smr 0.3) -- under both source allocations
(include/jaybenne_amd.h: jb_set_source_allocation), ``--seeds`` seeds each at the decks' own num_particles, in one
process.  One JSON line per deck with every run's number, mean and sample deviation per mode, and the census size.

    python tools/dev/source_alloc_error.py
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

DECKS = {
    "stepdiff": {"parthenon/mesh/nx1": 128, "parthenon/meshblock/nx1": 128},
    "stepdiff_smr": {"parthenon/mesh/nx1": 64, "parthenon/mesh/nx2": 32, "parthenon/meshblock/nx1": 16,
                     "parthenon/meshblock/nx2": 16},
}


def main():
    import torch
    from jaybenne_amd import analysis, mcblock
    from jaybenne_amd.deck import DECK_DIR, ParameterInput
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=8)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for deck, ov in DECKS.items():
        res = dict(deck=deck, seeds=args.seeds)
        for mode in ("uniform", "energy"):
            errs, census = [], []
            for s in range(args.seeds):
                pin = ParameterInput.from_file(os.path.join(DECK_DIR, deck + ".in"))
                pin.modify(dict(ov, **{"jaybenne/seed": 1000 + 17 * s, "jaybenne_amd/source_allocation": mode}))
                drv = mcblock.McblockDriver(pin, device=dev)
                drv.Execute()
                err = analysis.analytic_errors(drv.mesh, drv.md.get_field("tally"), drv.time, analysis.ur_solution)
                errs.append(round(float(err["mean_frac_error_weighted"]), 5))
                census.append(drv.md.n)
                drv.md.close()
            res[mode] = dict(errors=errs, mean=round(statistics.mean(errs), 5), sd=round(statistics.stdev(errs), 5),
                             census=census[0])
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
