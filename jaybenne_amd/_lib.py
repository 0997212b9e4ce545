"""ctypes binding of the C ABI (include/jaybenne_amd.h) exported by ``libjaybenne_amd.so``.

There is no fallback: if the HIP library is missing or a symbol is absent, importing the product
API fails loudly (build it with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C jaybenne_amd/csrc``).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# JAYBENNE_AMD_LIB selects another build of the same library (kernel experiments)
LIB_PATH = os.environ.get("JAYBENNE_AMD_LIB") or os.path.join(_HERE, "libjaybenne_amd.so")

JB_COMPLETE, JB_ITERATE, JB_INCOMPLETE = 0, 1, 2
JB_ERR_INVALID, JB_ERR_HIP, JB_ERR_CAPACITY, JB_ERR_UNSUPPORTED, JB_ERR_INVARIANT = -1, -2, -3, -4, -5
JB_SOURCE_THERMAL, JB_SOURCE_EMISSION = 0, 1
JB_STRATEGY_UNIFORM, JB_STRATEGY_ENERGY = 0, 1
JB_ST_ACTIVE, JB_ST_ABSORBED, JB_ST_ESCAPED, JB_ST_OUTGOING, JB_ST_OUTGOING_ABSORBED = 0, 1, 2, 3, 4
JB_RECORD_WORDS = 13

_dpp = C.POINTER(C.c_void_p)


class Params(C.Structure):
    _fields_ = [("num_particles", C.c_int64), ("dt", C.c_double),
                ("min_swarm_occupancy", C.c_double), ("numin", C.c_double), ("numax", C.c_double),
                ("tau_ddmc", C.c_double), ("unique_rank_seeds", C.c_int32), ("seed", C.c_int32),
                ("max_transport_iterations", C.c_int32), ("use_ddmc", C.c_int32),
                ("source_strategy", C.c_int32), ("do_emission", C.c_int32),
                ("do_feedback", C.c_int32), ("rank", C.c_int32)]


class Eos(C.Structure):
    _fields_ = [("model", C.c_int32), ("pad", C.c_int32), ("gm1", C.c_double), ("cv", C.c_double)]


class Opacity(C.Structure):
    _fields_ = [("model", C.c_int32), ("pad", C.c_int32), ("kappa", C.c_double),
                ("c", C.c_double), ("sb", C.c_double), ("time_scale", C.c_double),
                ("mass_scale", C.c_double), ("length_scale", C.c_double),
                ("temperature_scale", C.c_double)]


class Scattering(C.Structure):
    _fields_ = [("model", C.c_int32), ("pad", C.c_int32), ("kappa_s", C.c_double),
                ("apm", C.c_double), ("time_scale", C.c_double), ("mass_scale", C.c_double),
                ("length_scale", C.c_double), ("temperature_scale", C.c_double)]


ARITH_EXACT, ARITH_LEAN = 0, 1   # enum of jb_set_arithmetic
CELL_ORDER_ANY, CELL_ORDER_BY_ID = 0, 1   # enum of jb_set_cell_order
DEPOSIT_ATOMIC, DEPOSIT_EXACT = 0, 1      # enum of jb_set_deposition
TILT_NONE, TILT_LINEAR = 0, 1             # enum of jb_set_source_tilt
ALLOC_UNIFORM, ALLOC_ENERGY = 0, 1        # enum of jb_set_source_allocation
JB_DEPOSIT_ABSORBED, JB_DEPOSIT_ARRIVALS = 1, 2   # what jb_deposit_accumulate sweeps for (a sum of them)

FIELD_IDS = {"rho": 0, "sie": 1, "u": 2, "fleck": 3, "tally": 4, "edelta": 5}   # enum jb_field
FIELD_NAMES = ("rho", "sie", "u", "fleck", "tally", "edelta", "src_ew", "src_num", "P1", "P2", "P3")


class MeshView(C.Structure):
    _fields_ = ([("ndim", C.c_int32), ("ng", C.c_int32), ("nblocks", C.c_int32),
                 ("nblocks_total", C.c_int32), ("nx", C.c_int32 * 3), ("nleaf", C.c_int32 * 3),
                 ("bc", C.c_int32 * 6), ("rank", C.c_int32), ("pad", C.c_int32),
                 ("gmin", C.c_double * 3), ("gmax", C.c_double * 3),
                 ("leaf_map", C.c_void_p), ("owner", C.c_void_p), ("local_index", C.c_void_p),
                 ("gid", C.c_void_p), ("owned", C.c_void_p), ("blk_xmin", C.c_void_p), ("blk_xmax", C.c_void_p),
                 ("blk_dx", C.c_void_p), ("blk_level", C.c_void_p), ("blk_nbr_lev", C.c_void_p)] +
                [(n, C.c_void_p) for n in FIELD_NAMES])


SWARM_F64 = ("x", "y", "z", "vx", "vy", "vz", "t", "w", "e")
SWARM_I32 = ("ip", "jp", "kp", "blk", "status")


class SwarmView(C.Structure):
    _fields_ = ([("n", C.c_int64), ("capacity", C.c_int64)] +
                [(n, C.c_void_p) for n in SWARM_F64 + SWARM_I32] +
                [("id", C.c_void_p), ("rng", C.c_void_p)])


class TransportStats(C.Structure):
    _fields_ = [("n_census", C.c_int64), ("n_absorbed", C.c_int64), ("n_escaped", C.c_int64),
                ("n_outgoing", C.c_int64), ("n_events", C.c_int64),
                ("n_wave_passes", C.c_int64), ("n_wave_services", C.c_int64)]


class DebugStep(C.Structure):
    _fields_ = ([(n, C.c_double) for n in ("t_start", "dt", "ff", "aa", "ss", "vv", "dx_push")] +
                [("multi_d", C.c_int32), ("three_d", C.c_int32)] +
                [(n, C.c_double) for n in ("xl", "yl", "zl", "xu", "yu", "zu", "Px_l", "Py_l",
                                           "Pz_l", "Px_u", "Py_u", "Pz_u", "t", "x", "y", "z",
                                           "vx", "vy", "vz")] +
                [(n, C.c_int32) for n in ("ip", "jp", "kp", "is_absorbed", "is_scattered",
                                          "is_rejected")])


# jb_exchange_transport (include/jaybenne_amd.h): the two collectives of the hand-off on device buffers
ALL_GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)
ALL_TO_ALL_V_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                              C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int, C.c_void_p)


class ExchangeTransport(C.Structure):
    _fields_ = [("handle", C.c_void_p), ("all_gather_u64", ALL_GATHER_FN), ("all_to_all_v", ALL_TO_ALL_V_FN)]


# jb_rank_comm / jb_step_report of jb_radiation_step_ranks (include/jaybenne_amd.h)
RESERVE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(SwarmView), C.c_int64)


class RankComm(C.Structure):
    _fields_ = [("rank", C.c_int32), ("nranks", C.c_int32), ("transport", C.POINTER(ExchangeTransport)),
                ("host", C.c_void_p), ("reserve", RESERVE_FN)]


class StepReport(C.Structure):
    _fields_ = [("transport_iterations", C.c_int32), ("capacity_rounds", C.c_int32),
                ("sent", C.c_int64), ("received", C.c_int64), ("events", C.c_int64)]


# jb_invariant_report (include/jaybenne_amd.h): the checked library's counts
INV_KINDS = ("POSITION", "INDEX", "EVENT_OFF_BLOCK", "FACE_SAMPLE", "DDMC_CLASS", "SWARM")
INV_FAMILIES = ("transport", "imc_cell", "ddmc_all", "ddmc_q", "hybrid", "block_face", "ddmc_class", "swarm")


class InvariantReport(C.Structure):
    _fields_ = [("evaluated", C.c_int64 * len(INV_KINDS)), ("violated", C.c_int64 * len(INV_KINDS)),
                ("passes", C.c_int64 * len(INV_FAMILIES)),
                ("has_first", C.c_int32), ("first_kind", C.c_int32), ("first_family", C.c_int32),
                ("first_block", C.c_int32), ("first_slot", C.c_int64), ("first_id", C.c_int64),
                ("first_ip", C.c_int32), ("first_jp", C.c_int32), ("first_kp", C.c_int32),
                ("first_axis", C.c_int32), ("first_x", C.c_double), ("first_y", C.c_double),
                ("first_z", C.c_double)]

    def as_dict(self) -> dict:
        d = {"evaluated": dict(zip(INV_KINDS, self.evaluated)), "violated": dict(zip(INV_KINDS, self.violated)),
             "passes": dict(zip(INV_FAMILIES, self.passes)), "first": None}
        if self.has_first:
            d["first"] = {"kind": INV_KINDS[self.first_kind], "family": INV_FAMILIES[self.first_family],
                          "block": self.first_block, "slot": self.first_slot, "id": self.first_id,
                          "ijk": (self.first_ip, self.first_jp, self.first_kp), "axis": self.first_axis,
                          "x": (self.first_x, self.first_y, self.first_z)}
        return d


# jb_energy_ledger (include/jaybenne_amd.h): where the energy of one radiation cycle went
LEDGER_FACES = ("ix1", "ox1", "ix2", "ox2", "ix3", "ox3")
JB_LEDGER_SOURCED, JB_LEDGER_TRANSPORTED = 0, 1


class EnergyLedger(C.Structure):
    _fields_ = [("e_sourced", C.c_double), ("n_sourced", C.c_int64),
                ("e_escaped", C.c_double * 6), ("n_escaped", C.c_int64 * 6),
                ("e_escaped_unclassified", C.c_double), ("n_escaped_unclassified", C.c_int64),
                ("e_absorbed", C.c_double), ("n_absorbed", C.c_int64),
                ("e_census", C.c_double), ("n_census", C.c_int64),
                ("e_tally", C.c_double), ("e_delta", C.c_double), ("e_material", C.c_double),
                ("t_start", C.c_double), ("dt", C.c_double), ("cycle", C.c_int64)]

    @classmethod
    def from_dict(cls, d: dict) -> "EnergyLedger":
        led = cls()
        for name, kind in cls._fields_:
            if name in ("e_escaped", "n_escaped"):
                setattr(led, name, kind(*d[name]))
            else:
                setattr(led, name, d[name])
        return led

    def as_dict(self) -> dict:
        d = {}
        for name, kind in self._fields_:
            v = getattr(self, name)
            if name in ("e_escaped", "n_escaped"):
                d[name] = [float(x) if kind._type_ is C.c_double else int(x) for x in v]
            else:
                d[name] = float(v) if kind is C.c_double else int(v)
        return d


def ledger_residual(led: dict, e_start: float) -> float:
    """The residual of ``E0 + e_sourced = e_census + e_absorbed + sum_f e_escaped[f] + e_escaped_unclassified``
    relative to its left-hand side (0.0 when that is zero): a fixed sequence of IEEE operations, the one
    include/jaybenne_amd.hpp: LedgerResidual performs, so that every host prints the same bits."""
    lhs = e_start + led["e_sourced"]
    res = lhs - led["e_census"]
    res -= led["e_absorbed"]
    for e in led["e_escaped"]:
        res -= e
    res -= led["e_escaped_unclassified"]
    return abs(res) / lhs if lhs > 0.0 else 0.0


# jb_comb_plan / jb_comb_report (include/jaybenne_amd.h): the census comb
class CombPlan(C.Structure):
    _fields_ = [("n_before", C.c_int64), ("n_after", C.c_int64), ("n_new_ids", C.c_int64),
                ("cells_combed", C.c_int64), ("max_per_cell", C.c_int64), ("e_before", C.c_double),
                ("sorted", C.c_int64)]


class CombReport(C.Structure):
    _fields_ = [("n_after", C.c_int64), ("n_new_ids", C.c_int64), ("e_after", C.c_double)]


# jb_comb_global_plan (include/jaybenne_amd.h): the global census comb
class CombGlobalPlan(C.Structure):
    _fields_ = [("n_before", C.c_int64), ("n_after", C.c_int64), ("n_new_ids", C.c_int64),
                ("cells_thinned", C.c_int64), ("cells_split", C.c_int64), ("max_per_cell", C.c_int64),
                ("max_target", C.c_int64), ("sorted", C.c_int64), ("e_before", C.c_double)]


# jb_moments_report (include/jaybenne_amd.h): radiation moments; MOMENT_NAMES in the order of the enum JB_MOM_*
JB_MOMENTS = 12
MOMENT_NAMES = ("n", "e", "w2", "fx", "fy", "fz", "qxx", "qxy", "qxz", "qyy", "qyz", "qzz")


class MomentsReport(C.Structure):
    _fields_ = [("n_counted", C.c_int64), ("n_skipped", C.c_int64), ("cells_nonempty", C.c_int64),
                ("longest_run", C.c_int64), ("sorted", C.c_int32), ("pad", C.c_int32)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "pad"}


# jb_spectrum_report (include/jaybenne_amd.h): radiation spectrum
JB_SPECTRUM_MAX_GROUPS = 64


class SpectrumReport(C.Structure):
    _fields_ = [("n_counted", C.c_int64), ("n_skipped", C.c_int64), ("cells_nonempty", C.c_int64),
                ("longest_run", C.c_int64), ("n_below", C.c_int64), ("n_above", C.c_int64), ("sorted", C.c_int32),
                ("pad", C.c_int32)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "pad"}


# jb_deposit_stats (include/jaybenne_amd.h): the counts of the last close of exact deposition
class DepositStats(C.Structure):
    _fields_ = [("n_absorbed_addends", C.c_int64), ("n_census_addends", C.c_int64), ("n_truncated", C.c_int64),
                ("n_rejected", C.c_int64), ("scale_absorbed", C.c_int32), ("scale_census", C.c_int32)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# jb_boundary_source_plan / jb_boundary_source_record (include/jaybenne_amd.h): the boundary source
class BoundarySourcePlan(C.Structure):
    _fields_ = [("nper_block", C.c_void_p), ("e_face", C.c_double * 6), ("n_face", C.c_int64 * 6)]


class BoundarySourceRecord(C.Structure):
    _fields_ = [("e_face", C.c_double * 6), ("n_face", C.c_int64 * 6), ("kernel_launches", C.c_int64)]


# every entry point include/jaybenne_amd.h declares: name -> (restype, argtypes)
_vp, _i64, _f64, _int = C.c_void_p, C.c_int64, C.c_double, C.c_int
PROTOTYPES = {
    "jb_last_error": (C.c_char_p, []),
    "jb_version": (C.c_char_p, []),
    "jb_initialize": (_int, [C.POINTER(Params), C.POINTER(Eos), C.POINTER(Opacity),
                             C.POINTER(Scattering), _int, C.POINTER(_vp)]),
    "jb_finalize": (_int, [_vp]),
    "jb_set_stream": (_int, [_vp, _vp]),
    "jb_synchronize": (_int, [_vp]),
    "jb_param_seed": (C.c_int32, [_vp]),
    "jb_mesh_create": (_int, [_vp, C.POINTER(MeshView), C.POINTER(_vp)]),
    "jb_mesh_destroy": (_int, [_vp]),
    "jb_update_derived_transport_fields": (_int, [_vp, _vp, _f64]),
    "jb_source_photons_count": (_int, [_vp, _vp, _int, _f64, _int, C.c_uint32, _vp, _vp]),
    "jb_source_photons_fill": (_int, [_vp, _vp, C.POINTER(SwarmView), _int, _f64, _f64, _vp, _vp,
                                      _vp, _vp]),
    "jb_source_photons_fill_range": (_int, [_vp, _vp, C.POINTER(SwarmView), _int, _f64, _f64, _vp, _vp,
                                            _vp, _vp, _vp, _int]),
    "jb_set_boundary_source": (_int, [_vp, _int, _f64]),
    "jb_get_boundary_source": (_int, [_vp, _int, C.POINTER(C.c_double)]),
    "jb_boundary_source_enabled": (_int, [_vp]),
    "jb_set_boundary_source_count": (_int, [_vp, _i64, _i64]),
    "jb_boundary_face_cells": (_i64, [_vp, _vp]),
    "jb_boundary_prefix_words": (_i64, [_vp]),
    "jb_source_boundary_count": (_int, [_vp, _vp, _f64, _i64, _i64, C.c_uint32, C.POINTER(BoundarySourcePlan), _vp]),
    "jb_source_boundary_fill": (_int, [_vp, _vp, C.POINTER(SwarmView), _f64, _f64, _vp, _vp, _vp, _vp]),
    "jb_boundary_source_last": (_int, [_vp, C.POINTER(BoundarySourceRecord)]),
    "jb_transport_photons": (_int, [_vp, _vp, C.POINTER(SwarmView), _f64, _f64, _i64, _i64, _int]),
    "jb_transport_photons_ddmc": (_int, [_vp, _vp, C.POINTER(SwarmView), _f64, _f64, _i64, _i64,
                                         _int]),
    "jb_last_transport_variant": (C.c_char_p, [_vp]),
    "jb_last_transport_grid": (_int, [_vp]),
    "jb_last_transport_unit_cell": (_int, [_vp]),
    "jb_mesh_exact_geometry": (_int, [_vp]),
    "jb_mesh_ddmc_classes": (_int, [_vp]),
    "jb_get_transport_stats": (_int, [_vp, C.POINTER(TransportStats), _int]),
    "jb_sample_ddmc_block_face": (_int, [_vp, _vp, C.POINTER(SwarmView), _i64, _i64]),
    "jb_check_completion": (_int, [_vp, C.POINTER(SwarmView), _f64, C.POINTER(_i64)]),
    "jb_zero_energy_tally": (_int, [_vp, _vp]),
    "jb_evaluate_radiation_energy": (_int, [_vp, _vp, C.POINTER(SwarmView)]),
    "jb_update_fluid": (_int, [_vp, _vp]),
    "jb_photon_reflect_bc": (_int, [_vp, _vp, C.POINTER(SwarmView), _int]),
    "jb_remove_marked_particles": (_int, [_vp, C.POINTER(SwarmView)]),
    "jb_defrag_particles": (_int, [_vp, _vp, C.POINTER(SwarmView)]),
    "jb_release_scratch": (_int, [_vp]),
    "jb_comb_census_plan": (_int, [_vp, _vp, C.POINTER(SwarmView), _i64, _i64, C.c_uint32, C.POINTER(CombPlan)]),
    "jb_comb_census_apply": (_int, [_vp, _vp, C.POINTER(SwarmView), C.c_uint64, C.POINTER(CombReport)]),
    "jb_comb_census_weigh": (_int, [_vp, _vp, C.POINTER(SwarmView), _i64, _vp, C.POINTER(CombGlobalPlan)]),
    "jb_gcomb_kernel_launches": (_i64, [_vp]),
    "jb_comb_census_plan_global": (_int, [_vp, _vp, C.POINTER(SwarmView), C.c_double, _i64, C.c_double, _i64,
                                          C.c_uint32, C.POINTER(CombGlobalPlan)]),
    "jb_moments_words": (_i64, [_vp]),
    "jb_evaluate_radiation_moments": (_int, [_vp, _vp, C.POINTER(SwarmView), _vp, C.POINTER(MomentsReport)]),
    "jb_evaluate_radiation_moments_host": (_int, [_vp, _vp, C.POINTER(SwarmView), _vp, C.POINTER(MomentsReport)]),
    "jb_spectrum_words": (_i64, [_vp, _int]),
    "jb_evaluate_radiation_spectrum": (_int, [_vp, _vp, C.POINTER(SwarmView), _vp, _int, _vp,
                                              C.POINTER(SpectrumReport)]),
    "jb_evaluate_radiation_spectrum_host": (_int, [_vp, _vp, C.POINTER(SwarmView), _vp, _int, _vp,
                                                   C.POINTER(SpectrumReport)]),
    "jb_defrag_policy": (_int, [_vp, _vp, C.POINTER(SwarmView), _i64, C.c_int32, C.POINTER(C.c_int32)]),
    "jb_pack_outgoing": (_int, [_vp, _vp, C.POINTER(SwarmView), _i64, _i64, _int, _vp, _i64, _vp]),
    "jb_unpack_incoming": (_int, [_vp, _vp, C.POINTER(SwarmView), _vp, _i64]),
    "jb_transport_rccl": (_int, [_vp, _int, _int, _vp]),
    "jb_transport_release": (_int, [_vp]),
    "jb_exchange": (_int, [_vp, _vp, C.POINTER(SwarmView), _i64, _i64, _int, _int, _vp, _vp, _i64, _vp, _i64,
                           C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    "jb_gather_cells": (_int, [_vp, _vp, _int, _i64, _vp, _vp, _vp]),
    "jb_fill_cells": (_int, [_vp, _vp, _int, _i64, _int, _vp, _vp, _vp, _vp, _vp]),
    "jb_estimate_timestep": (_f64, [_vp]),
    "jb_radiation_step": (_int, [_vp, _vp, C.POINTER(SwarmView), _f64, _f64,
                                 C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), _vp]),
    "jb_radiation_step_ranks": (_int, [_vp, _vp, C.POINTER(SwarmView), _f64, _f64, C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_uint32), _vp, C.POINTER(RankComm), C.POINTER(StepReport)]),
    "jb_ledger_enable": (_int, [_vp, _int]),
    "jb_ledger_enabled": (_int, [_vp]),
    "jb_ledger_accumulate": (_int, [_vp, _vp, C.POINTER(SwarmView), _i64, _i64, _int]),
    "jb_ledger_close": (_int, [_vp, _vp, C.POINTER(SwarmView), _f64, _f64, C.POINTER(EnergyLedger)]),
    "jb_ledger_reduce": (_int, [_vp, C.POINTER(ExchangeTransport), _int, _int, _int, C.POINTER(EnergyLedger)]),
    "jb_ledger_last": (_int, [_vp, C.POINTER(EnergyLedger)]),
    "jb_invariants_enabled": (_int, []),
    "jb_invariant_report_get": (_int, [_vp, C.POINTER(InvariantReport), _int]),
    "jb_verify_swarm": (_int, [_vp, _vp, C.POINTER(SwarmView), _f64, _f64, C.POINTER(InvariantReport)]),
    "jb_range_push": (_int, [C.c_char_p]),
    "jb_range_pop": (_int, []),
    "jb_ranges_enabled": (_int, []),
    "jb_debug_philox": (_int, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                               C.POINTER(C.c_uint32)]),
    "jb_debug_rocrand_philox": (_int, [_vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32)]),
    "jb_debug_seed_state": (_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]),
    "jb_debug_stream_start": (_int, [_vp, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]),
    "jb_debug_draw_stream": (_int, [_vp, C.c_uint64, _int, _vp, C.POINTER(C.c_uint64)]),
    "jb_set_arithmetic": (_int, [_vp, _int]),
    "jb_get_arithmetic": (_int, [_vp]),
    "jb_set_cell_order": (_int, [_vp, _int]),
    "jb_get_cell_order": (_int, [_vp]),
    "jb_set_deposition": (_int, [_vp, _int]),
    "jb_get_deposition": (_int, [_vp]),
    "jb_deposit_accumulate": (_int, [_vp, _vp, C.POINTER(SwarmView), _i64, _i64, _int]),
    "jb_deposit_close": (_int, [_vp, _vp, C.POINTER(SwarmView)]),
    "jb_deposit_last": (_int, [_vp, C.POINTER(DepositStats)]),
    "jb_deposit_memory": (_i64, [_vp]),
    "jb_deposit_kernel_launches": (_i64, [_vp]),
    "jb_set_source_tilt": (_int, [_vp, _int]),
    "jb_get_source_tilt": (_int, [_vp]),
    "jb_source_tilt_slopes": (_int, [_vp, _vp, _int, _vp]),
    "jb_set_source_allocation": (_int, [_vp, _int]),
    "jb_get_source_allocation": (_int, [_vp]),
    "jb_source_energy_sums": (_int, [_vp, _vp, _int, C.c_double, _vp]),
    "jb_source_energy_total": (C.c_double, [_vp, _int]),
    "jb_source_photons_count_energy": (_int, [_vp, _vp, _int, C.c_double, C.c_uint32, C.c_double, _vp, _vp]),
    "jb_debug_math": (_int, [_vp, _int, _vp, _int, _vp]),
    "jb_debug_model_coefficients": (_int, [_vp, C.POINTER(C.c_double * 4)]),
    "jb_debug_model_eval": (_int, [_vp, _int, _vp, _int, _vp]),
    "jb_debug_step_call": (_int, [_vp, _int, C.POINTER(DebugStep), _vp, _int, C.POINTER(_int)]),
    "jb_debug_sample_call": (_int, [_vp, _int, _vp, _vp, _vp, _int, _vp, _vp, C.POINTER(_int)]),
}

_lib = None


class JaybenneError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"jaybenne_amd status {status}: {message}")
        self.status = status


def load():
    """Load the shared library and bind every declared symbol (AttributeError if one is absent)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP extension has not been built "
                "(run __graft_entry__.build() or make -C jaybenne_amd/csrc). "
                "There is no CPU fallback for the product path.")
        # PyTorch-ROCm ships its own HIP runtime; it has to be in the process before this library
        # is, so that both resolve libamdhip64 to the same copy (two runtimes in one process do
        # not see each other's devices or allocations)
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(status: int) -> int:
    if status < 0:
        raise JaybenneError(status, load().jb_last_error().decode())
    return status
