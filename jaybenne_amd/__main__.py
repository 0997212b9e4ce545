"""Run an input deck the way the reference's regression harness drives `mcblock`:

    python -m jaybenne_amd -i jaybenne_amd/decks/stepdiff.in parthenon/mesh/nx1=128 \\
           parthenon/meshblock/nx1=128 [--tolerance 0.05] [--comparison weighted_mean]

Trailing ``block/key=value`` arguments override deck values (Parthenon's command-line syntax,
which tst/regression_test.py:85-145 emulates by rewriting the deck).  After the last cycle the
energy tally is compared with the analytic solution of tst/stepdiff.py and the same five numbers
as tst/regression_test.py:408-412 are printed; the exit code is 0 iff the chosen criterion is
within the tolerance.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np


def ledger_json(led: dict) -> str:
    """One cycle's energy ledger as a JSON line (``--ledger FILE``; examples/mcblock_amd writes the same keys and
    values): a float is written so that reading the line restores its bits."""
    import json
    keys = ("cycle", "t_start", "dt", "e_start", "e_sourced", "n_sourced", "e_escaped", "n_escaped",
            "e_escaped_unclassified", "n_escaped_unclassified", "e_absorbed", "n_absorbed", "e_census", "n_census",
            "e_tally", "e_delta", "e_material", "residual")
    out = {k: led[k] for k in keys}
    for k in ("e_sourced_face", "n_sourced_face"):     # (only with a boundary source face on)
        if k in led:
            out[k] = led[k]
    return json.dumps(out)


def moments_integrals(fields: np.ndarray, blk_dx: np.ndarray, c: float) -> dict:
    """The domain integrals of the twelve moment fields ``[12, nblocks, ...]`` (``--moments FILE``): n, e = sum E dv,
    w2, f = sum F dv, q = sum Q dv, each summed sequentially in (component, block, cell) order -- as
    include/jaybenne_amd.hpp: IntegrateMoments, so that both hosts print the same digits -- and
    eddington[d] = q_dd / (c^2 e)."""
    nb = fields.shape[1]
    dv = (blk_dx[:nb, 0] * blk_dx[:nb, 1]) * blk_dx[:nb, 2]
    s = []
    for comp in range(fields.shape[0]):
        v = fields[comp].reshape(nb, -1)
        if comp not in (0, 2):
            v = v * dv[:, None]
        s.append(float(np.add.accumulate(v.reshape(-1))[-1]) if v.size else 0.0)     # (accumulate: one by one, in order)
    c2e = (c * c) * s[1]
    return dict(n=s[0], e=s[1], w2=s[2], f=s[3:6], q=s[6:12],
                eddington=[s[6 + d] / c2e if c2e > 0.0 else 0.0 for d in (0, 3, 5)])


def moments_json(cycle: int, t: float, report: dict, integ: dict) -> str:
    """One cycle's line of ``--moments FILE`` (examples/mcblock_amd writes the same characters: %.17g restores a
    float's bits)."""
    g = lambda x: "%.17g" % x                           # noqa: E731
    lst = lambda xs: "[" + ", ".join(g(x) for x in xs) + "]"      # noqa: E731
    return ("{" + f'"cycle": {int(cycle)}, "time": {g(t)}, "n_counted": {report["n_counted"]}, '
            f'"n_skipped": {report["n_skipped"]}, "cells_nonempty": {report["cells_nonempty"]}, '
            f'"longest_run": {report["longest_run"]}, "sorted": {report["sorted"]}, "n": {g(integ["n"])}, '
            f'"e": {g(integ["e"])}, "w2": {g(integ["w2"])}, "f": {lst(integ["f"])}, "q": {lst(integ["q"])}, '
            f'"eddington": {lst(integ["eddington"])}' + "}")


_DECIMAL = None


def parse_spectrum_edges(text: str) -> list:
    """``spectrum_edges = e0, e1, ..`` of a deck or a command line: a comma-separated list of decimal numbers; blanks
    around a number and empty items are ignored.  A number is ``[+-] digits [. digits] | [+-] . digits``, then
    optionally ``e|E [+-] digits`` -- the grammar of include/jaybenne_amd.hpp: ParseSpectrumEdges, narrower than
    ``float`` (no ``1_0``, no ``inf`` or ``nan``) and than strtod (no hex floats), so that no text is a number to one
    host and an error to the other.  The value is ``float``'s, correctly rounded as strtod's.  Anything else, or fewer
    than 2 or more than 65 numbers, raises ValueError with the words examples/mcblock_amd uses."""
    global _DECIMAL
    if _DECIMAL is None:
        import re
        _DECIMAL = re.compile(r"[+-]?(?:[0-9]+(?:\.[0-9]*)?|\.[0-9]+)(?:[eE][+-]?[0-9]+)?", re.ASCII)
    edges = []
    for item in text.split(","):
        item = item.strip(" \t")
        if not item:
            continue
        if not _DECIMAL.fullmatch(item):
            raise ValueError(f"spectrum_edges: '{item}' is not a decimal number")
        edges.append(float(item))
    if not 2 <= len(edges) <= 65:
        raise ValueError("spectrum_edges: 2 .. 65 comma-separated edges are needed")
    return edges


def spectrum_integrals(spec: np.ndarray, blk_dx: np.ndarray) -> list:
    """The domain integrals of the spectrum ``[NB, nblocks, ...]`` (``--spectrum FILE``): sum over cells of out[bin] dv
    for every bin, summed sequentially in (block, cell) order -- as include/jaybenne_amd.hpp: IntegrateSpectrum."""
    nb = spec.shape[1]
    dv = (blk_dx[:nb, 0] * blk_dx[:nb, 1]) * blk_dx[:nb, 2]
    out = []
    for b in range(spec.shape[0]):
        v = (spec[b].reshape(nb, -1) * dv[:, None]).reshape(-1)
        out.append(float(np.add.accumulate(v)[-1]) if v.size else 0.0)        # (accumulate: one by one, in order)
    return out


def spectrum_json(cycle: int, t: float, report: dict, edges, integ) -> str:
    """One cycle's line of ``--spectrum FILE`` (examples/mcblock_amd writes the same characters)"""
    g = lambda x: "%.17g" % x                           # noqa: E731
    lst = lambda xs: "[" + ", ".join(g(x) for x in xs) + "]"      # noqa: E731
    return ("{" + f'"cycle": {int(cycle)}, "time": {g(t)}, "n_counted": {report["n_counted"]}, '
            f'"n_skipped": {report["n_skipped"]}, "cells_nonempty": {report["cells_nonempty"]}, '
            f'"longest_run": {report["longest_run"]}, "n_below": {report["n_below"]}, "n_above": {report["n_above"]}, '
            f'"sorted": {report["sorted"]}, "ngroups": {len(edges) - 1}, "edges": {lst(edges)}, "e": {lst(integ)}' + "}")


def comb_json(rec: dict) -> str:
    """One combed cycle's line of ``--comb-history FILE`` (examples/mcblock_amd writes the same characters: %.17g
    restores a float's bits); the global comb's keys only for its records."""
    g = lambda x: "%.17g" % x                           # noqa: E731
    s = (f'"cycle": {int(rec["cycle"])}, "n_before": {rec["n_before"]}, "n_after": {rec["n_after"]}, '
         f'"n_new_ids": {rec["n_new_ids"]}, "id_base": {rec["id_base"]}, "cells_combed": {rec["cells_combed"]}, '
         f'"max_per_cell": {rec["max_per_cell"]}, "e_before": {g(rec["e_before"])}, "e_after": {g(rec["e_after"])}')
    if rec.get("mode") == "global":
        s += (f', "mode": "global", "cells_thinned": {rec["cells_thinned"]}, "cells_split": {rec["cells_split"]}, '
              f'"max_target": {rec["max_target"]}, "w_total": {g(rec["w_total"])}, "scale": {g(rec["scale"])}')
    return "{" + s + "}"


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m jaybenne_amd", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-i", "--input", required=True, help="Parthenon-style input deck")
    ap.add_argument("--tolerance", type=float, default=None,
                    help="pass/fail bound on the chosen error (0.05 stepdiff, 0.3 SMR decks in the reference)")
    ap.add_argument("--comparison", default="weighted_mean", choices=["mean", "pointwise", "weighted_mean"])
    ap.add_argument("--transverse-average", action="store_true",
                    help="average the tally over cells of equal x before comparing (uniform meshes)")
    ap.add_argument("--match-total-energy", action="store_true",
                    help="with --transverse-average: scale the solution to the tally's total energy "
                         "(fewer than one source particle per cell under-samples the energy)")
    ap.add_argument("--output", default=None,
                    help="write the final state to this file: .phdf (Parthenon-style HDF5, needs "
                         "libhdf5) or .npz.  Without it a deck with a <parthenon/output0> block of "
                         "file_type = hdf5 writes <problem_id>.out0.final.phdf into --output-dir")
    ap.add_argument("--output-dir", default=None, help="directory for deck-driven dumps (default: none written)")
    ap.add_argument("--ledger", default=None, metavar="FILE",
                    help="switch the energy ledger on: one JSON line per cycle to FILE, leak by face and the "
                         "residual of the energy balance on the per-cycle line, totals by face at the end")
    ap.add_argument("--moments", default=None, metavar="FILE",
                    help="after every cycle one JSON line to FILE: the report of EvaluateRadiationMoments and the "
                         "domain integrals of count, energy, flux and second-moment tensor, with the Eddington "
                         "factors (the deck key <jaybenne_amd> moments = true: to moments.jsonl)")
    ap.add_argument("--spectrum", default=None, metavar="FILE",
                    help="after every cycle one JSON line to FILE: the report of EvaluateRadiationSpectrum, the edges "
                         "(deck key <jaybenne_amd> spectrum_edges = e0, e1, ..) and the domain integral of the census "
                         "energy in every bin (the deck key <jaybenne_amd> spectrum = true: to spectrum.jsonl)")
    ap.add_argument("--comb-history", default=None, metavar="FILE",
                    help="one JSON line to FILE per cycle whose census comb (census_per_cell_max or "
                         "census_total_target) changed the swarm")
    ap.add_argument("overrides", nargs="*", help="block/key=value")
    args = ap.parse_args(argv)

    import torch
    from . import analysis, mcblock
    from .deck import ParameterInput

    pin = ParameterInput.from_file(args.input)
    ov = {}
    for item in args.overrides:
        if "=" not in item:
            ap.error(f"override '{item}' is not of the form block/key=value")
        k, v = item.split("=", 1)
        ov[k] = v
    pin.modify(ov)
    if not torch.cuda.is_available():
        print("jaybenne_amd needs a GPU (the history loop runs only as HIP kernels)", file=sys.stderr)
        return 2
    drv = mcblock.McblockDriver(pin, device=torch.device("cuda", 0), ledger=True if args.ledger else None)
    ledger_file = open(args.ledger, "w") if args.ledger else None
    moments_path = args.moments or ("moments.jsonl" if pin.GetOrAddBoolean("jaybenne_amd", "moments", False) else None)
    moments_file = open(moments_path, "w") if moments_path else None
    spectrum_path = args.spectrum or ("spectrum.jsonl" if pin.GetOrAddBoolean("jaybenne_amd", "spectrum", False) else None)
    spectrum_file, spectrum_edges = None, []
    if spectrum_path:
        try:
            spectrum_edges = parse_spectrum_edges(pin.GetOrAddString("jaybenne_amd", "spectrum_edges", ""))
        except ValueError as e:                      # (examples/mcblock_amd: the same words, the same exit code)
            print(f"python -m jaybenne_amd: {e}", file=sys.stderr)
            return 2
        spectrum_file = open(spectrum_path, "w")
    comb_file = open(args.comb_history, "w") if args.comb_history else None
    print(f"problem {drv.mcb.problem_id}: {drv.mesh.ndim}-D, {drv.mesh.nblocks} meshblocks, "
          f"levels {sorted(set(drv.mesh.blk_level.tolist()))}, {drv.md.n} photons")
    t0 = time.perf_counter()
    from ._lib import JB_ERR_INVARIANT, JaybenneError
    checked = drv.md.invariants_enabled()   # the checked library (JAYBENNE_AMD_LIB): report at exit
    try:
        while drv.time < drv.tlim:
            n0, e0 = drv.md.n, drv.md.events
            c0 = time.perf_counter()
            drv.Step()
            torch.cuda.synchronize()
            dt = time.perf_counter() - c0
            line = (f"cycle={drv.ncycle} time={drv.time:.6e} dt={drv.dt:.6e} photons={drv.md.n} "
                    f"histories/s={n0 / dt:.3e} events/s={(drv.md.events - e0) / dt:.3e}")
            if ledger_file is not None:
                led = drv.md.ledger
                bsh = drv.md.boundary_source_history
                if bsh and bsh[-1]["cycle"] == drv.md.cycle:   # per-face sourced energy of the boundary source
                    led = dict(led, e_sourced_face=bsh[-1]["e_face"], n_sourced_face=bsh[-1]["n_face"])
                ledger_file.write(ledger_json(led) + "\n")
                line += " leak=[" + ", ".join(f"{e:.6e}" for e in led["e_escaped"]) + f"] residual={led['residual']:.3e}"
            if drv.md.comb_history and drv.md.comb_history[-1]["cycle"] == drv.md.cycle:
                line += f" combed={drv.md.comb_history[-1]['cells_combed']} new_ids={drv.md.comb_history[-1]['n_new_ids']}"
                if comb_file is not None:
                    comb_file.write(comb_json(drv.md.comb_history[-1]) + "\n")
            if moments_file is not None:
                fields, rep = drv.jb.EvaluateRadiationMoments(drv.md)
                integ = moments_integrals(fields.cpu().numpy(), np.asarray(drv.mesh.blk_dx)[drv.md.resident_gids],
                                          drv.pkg.Param("speed_of_light"))
                moments_file.write(moments_json(drv.md.cycle, drv.time, rep, integ) + "\n")
                line += " eddington=[" + ", ".join(f"{e:.4f}" for e in integ["eddington"]) + "]"
            if spectrum_file is not None:
                spec, rep = drv.jb.EvaluateRadiationSpectrum(drv.md, spectrum_edges)
                integ = spectrum_integrals(spec.cpu().numpy(), np.asarray(drv.mesh.blk_dx)[drv.md.resident_gids])
                spectrum_file.write(spectrum_json(drv.md.cycle, drv.time, rep, spectrum_edges, integ) + "\n")
            print(line)
    except JaybenneError as e:
        if not (checked and e.status == JB_ERR_INVARIANT):
            raise
        print(f"invariants: {drv.md.invariant_report()}")
        print(f"TEST FAILED: {e}", file=sys.stderr)
        return 3
    print(f"walltime used = {time.perf_counter() - t0:.2f} s")
    if moments_file is not None:
        moments_file.close()
    if spectrum_file is not None:
        spectrum_file.close()
    if comb_file is not None:
        comb_file.close()
    if ledger_file is not None:
        ledger_file.close()
        import math
        from ._lib import LEDGER_FACES
        hist = drv.md.ledger_history
        print("leakage by face: " + " ".join(
            f"{name}={math.fsum(h['e_escaped'][f] for h in hist):.6e} ({sum(h['n_escaped'][f] for h in hist)})"
            for f, name in enumerate(LEDGER_FACES)))
        print(f"sourced={math.fsum(h['e_sourced'] for h in hist):.6e} absorbed={math.fsum(h['e_absorbed'] for h in hist):.6e} "
              f"unclassified={math.fsum(h['e_escaped_unclassified'] for h in hist):.6e} "
              f"census={hist[-1]['e_census'] if hist else 0.0:.6e} largest residual={max((h['residual'] for h in hist), default=0.0):.3e}")
    if checked:
        print(f"invariants: {drv.md.invariant_report()}")
    tally = drv.md.get_field("tally")
    if drv.mcb.problem_id.startswith("inf"):
        from . import constants
        solution = analysis.equilibrium_solution(drv.mcb.initial_temperature,
                                                 constants.STEFAN_BOLTZMANN, constants.SPEED_OF_LIGHT)
        print(f"domain-mean energy tally / (a T0^4): "
              f"{float(np.mean(np.asarray(tally)[drv.mesh.interior()])) / float(solution(0.0, 0.0)):.4f}")
    else:
        solution = analysis.ur_solution
    err = analysis.analytic_errors(drv.mesh, tally, drv.time, solution,
                                   transverse_average=args.transverse_average,
                                   match_total_energy=args.match_total_energy)
    print(f"Mean error:                     {err['mean_error']:.2e}")
    print(f"Mean fractional error:          {err['mean_frac_error']:.2e}")
    print(f"Mean weighted fractional error: {err['mean_frac_error_weighted']:.2e}")
    print(f"Max error:                      {err['max_error']:.2e}")
    print(f"Max fractional error:           {err['max_frac_error']:.2e}")
    out_path = args.output
    if out_path is None and args.output_dir is not None and \
            pin.GetOrAddString("parthenon/output0", "file_type", "none") == "hdf5":
        out_path = os.path.join(args.output_dir, f"{drv.mcb.problem_id}.out0.final.phdf")
    if out_path:
        from . import phdf
        if out_path.endswith(".npz") or not phdf.available():
            if not out_path.endswith(".npz"):
                print("libhdf5 not found: writing .npz instead", file=sys.stderr)
                out_path = os.path.splitext(out_path)[0] + ".npz"
            np.savez(out_path, tally=tally, time=drv.time, blk_xmin=drv.mesh.blk_xmin,
                     blk_dx=drv.mesh.blk_dx, blk_level=drv.mesh.blk_level)
        else:
            # <parthenon/output0> variables / swarm_variables of the deck (inputs/stepdiff_smr.in:86-94)
            names = {"field.material.density": "rho", "field.material.sie": "sie",
                     "field.material.internal_energy": "u", "field.jaybenne.energy_tally": "tally",
                     "field.jaybenne.fleck_factor": "fleck"}
            want = [v.strip() for v in pin.GetOrAddString(
                "parthenon/output0", "variables", "field.jaybenne.energy_tally").replace("&", "").split(",") if v.strip()]
            variables = {v: drv.md.get_field(names[v]) for v in want if v in names}
            sw = drv.md.get_swarm()
            svars = [v.strip() for v in pin.GetOrAddString(
                "parthenon/output0", "swarm_variables", "swarm.x, swarm.y").replace("&", "").split(",") if v.strip()]
            key = {"swarm.x": "x", "swarm.y": "y", "swarm.z": "z", "weight": "w", "time": "t", "energy": "e"}
            swarm = {"blk": drv.md.gids[sw["blk"]], "id": sw["id"]}
            swarm.update({v: sw[key[v]] for v in svars if v in key})
            phdf.write_dump(out_path, drv.mesh, drv.time, drv.dt, drv.ncycle, variables,
                            {"photons": swarm}, input_text=open(args.input).read())
        print(f"wrote {out_path}")
    if args.tolerance is None:
        return 0
    crit = {"mean": err["mean_frac_error"], "pointwise": err["max_frac_error"],
            "weighted_mean": err["mean_frac_error_weighted"]}[args.comparison]
    ok = crit <= args.tolerance
    print("TEST PASSED" if ok else "TEST FAILED")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
