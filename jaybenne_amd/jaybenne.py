"""Host-side mirror of the reference's package interface (reference src/jaybenne/jaybenne.hpp:48-78)
over the C ABI of ``libjaybenne_amd.so``.

Same task names, same argument meaning (``md, t_start, dt``), same return convention
(``TaskStatus``) and the same failure conditions as the reference (PARTHENON_REQUIRE /
PARTHENON_FAIL become exceptions).  PyTorch appears only as the owner of device memory, the
stream and ``torch.distributed``; every field / particle update runs in the HIP library.
"""
from __future__ import annotations

import ctypes as C
import os
import time
import enum
import sys
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from .deck import ParameterInput
from .mesh import Mesh

photons_swarm_name = "photons"           # jaybenne_variables.hpp:23


class TaskStatus(enum.IntEnum):
    complete = _lib.JB_COMPLETE
    iterate = _lib.JB_ITERATE
    incomplete = _lib.JB_INCOMPLETE


class SourceType(enum.IntEnum):           # jaybenne.hpp:56
    thermal = _lib.JB_SOURCE_THERMAL
    emission = _lib.JB_SOURCE_EMISSION


class SourceStrategy(enum.IntEnum):       # jaybenne.hpp:55
    uniform = _lib.JB_STRATEGY_UNIFORM
    energy = _lib.JB_STRATEGY_ENERGY


# ------------------------------------------------------------------------------------------------
class StateDescriptor:
    """What ``jaybenne::Initialize`` returns: the package's parameters (``Param``) plus, here,
    the library context that owns the device-side copies of them."""

    def __init__(self, params: Dict[str, object], ctx: C.c_void_p, device: torch.device):
        self._params = dict(params)
        self.ctx = ctx
        self.device = device
        self.lib = _lib.load()

    def Param(self, name: str):
        return self._params[name]

    # arithmetic of the gray IMC tracking step (include/jaybenne_amd.h): "lean" (default) or
    # "exact" (bit-identical to the CPU oracle's portable flavour)
    def set_arithmetic(self, mode: str) -> None:
        code = {"exact": _lib.ARITH_EXACT, "lean": _lib.ARITH_LEAN}[mode]
        _lib.check(self.lib.jb_set_arithmetic(self.ctx, code))

    def arithmetic(self) -> str:
        return "lean" if self.lib.jb_get_arithmetic(self.ctx) == _lib.ARITH_LEAN else "exact"

    def AllParams(self) -> Dict[str, object]:
        return dict(self._params)

    def close(self) -> None:
        if self.ctx is not None:
            self.lib.jb_finalize(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def Initialize(pin: ParameterInput, opacity, scattering, eos, device: Optional[torch.device] = None,
               my_rank: int = 0) -> StateDescriptor:
    """``jaybenne::Initialize(pin, opacity, scattering, eos)`` -- reference jaybenne.cpp:158-266:
    same keys, defaults and failure conditions."""
    lib = _lib.load()
    num_particles = pin.GetInteger("jaybenne", "num_particles")
    dt = pin.GetOrAddReal("jaybenne", "dt", sys.float_info.max)
    min_occ = pin.GetOrAddReal("jaybenne", "min_swarm_occupancy", 0.0)
    if not (0.0 <= min_occ < 1.0):
        raise ValueError("Minimum allowable swarm occupancy must be >= 0 and less than 1")
    numin = pin.GetOrAddReal("jaybenne", "numin", sys.float_info.min)
    numax = pin.GetOrAddReal("jaybenne", "numax", sys.float_info.max)
    units = opacity.GetRuntimePhysicalConstants()
    unique_rank_seeds = pin.GetOrAddBoolean("jaybenne", "unique_rank_seeds", True)
    seed = pin.GetOrAddInteger("jaybenne", "seed", 123)
    max_iter = pin.GetOrAddInteger("jaybenne", "max_transport_iterations", 10000)
    use_ddmc = pin.GetOrAddBoolean("jaybenne", "use_ddmc", False)
    tau_ddmc = pin.GetOrAddReal("jaybenne", "tau_ddmc", 5.0)
    strategy = pin.GetOrAddString("jaybenne", "source_strategy", "uniform")
    if strategy == "uniform":
        source_strategy = SourceStrategy.uniform
    elif strategy == "energy":
        source_strategy = SourceStrategy.energy
    else:
        raise ValueError("Only uniform or energy source strategies supported!")
    do_emission = pin.GetOrAddBoolean("jaybenne", "do_emission", True)
    do_feedback = pin.GetOrAddBoolean("jaybenne", "do_feedback", True)

    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    p = _lib.Params(num_particles=num_particles, dt=dt, min_swarm_occupancy=min_occ, numin=numin,
                    numax=numax, tau_ddmc=tau_ddmc, unique_rank_seeds=int(unique_rank_seeds),
                    seed=seed, max_transport_iterations=max_iter, use_ddmc=int(use_ddmc),
                    source_strategy=int(source_strategy), do_emission=int(do_emission),
                    do_feedback=int(do_feedback), rank=my_rank)
    e = _lib.Eos(model=eos.model, gm1=eos.gm1, cv=eos.cv)
    scales = {k: float(getattr(opacity, k, 1.0)) for k in
              ("time_scale", "mass_scale", "length_scale", "temperature_scale")}
    o = _lib.Opacity(model=opacity.model, kappa=opacity.kappa, c=units.c, sb=units.sb, **scales)
    scales_s = {k: float(getattr(scattering, k, 1.0)) for k in
                ("time_scale", "mass_scale", "length_scale", "temperature_scale")}
    s = _lib.Scattering(model=scattering.model, kappa_s=scattering.kappa_s, apm=scattering.apm,
                        **scales_s)
    ctx = C.c_void_p()
    _lib.check(lib.jb_initialize(C.byref(p), C.byref(e), C.byref(o), C.byref(s),
                                 device.index or 0, C.byref(ctx)))
    params = dict(num_particles=num_particles, dt=dt, min_swarm_occupancy=min_occ, numin=numin,
                  numax=numax, speed_of_light=units.c, stefan_boltzmann=units.sb,
                  unique_rank_seeds=unique_rank_seeds, seed=int(lib.jb_param_seed(ctx)),
                  max_transport_iterations=max_iter, use_ddmc=use_ddmc, tau_ddmc=tau_ddmc,
                  source_strategy=source_strategy, do_emission=do_emission,
                  do_feedback=do_feedback, eos_d=eos, opacity_d=opacity, scattering_d=scattering)
    return StateDescriptor(params, ctx, device)


# ------------------------------------------------------------------------------------------------
_F64 = _lib.SWARM_F64
_I32 = _lib.SWARM_I32


class MeshData:
    """The blocks of one rank with their fields and photon swarm in HBM (the role of
    Parthenon's ``MeshData<Real>`` + ``SwarmContainer`` for this package).

    Layout in HBM: each field is one ``[nblocks_local, nk, nj, ni]`` float64 tensor (ghosts
    included; the C ABI receives one device pointer per block); the swarm is a structure of
    arrays with ``capacity`` slots, particles ``0..n-1`` valid.
    """

    def __init__(self, pkg: StateDescriptor, mesh: Mesh, capacity: int, rank: int = 0,
                 nranks: int = 1, comm=None, halo_rings: int = 1, replicated: bool = False):
        self.pkg = pkg
        self.mesh = mesh
        self.rank, self.nranks = rank, nranks
        self.comm = comm
        self.lib = pkg.lib
        dev = pkg.device
        self.device = dev
        # Replicated mesh, split particles (the reference has no such mode, its blocks are
        # partitioned: jaybenne.cpp:92-95): every rank holds EVERY block and follows its share of each
        # block's photons -- dealt by stream id at the source (jb_source_photons_fill_range) -- from
        # source to census; nothing is ever handed over, and the ranks' energy_tally / energy_delta
        # are summed once per cycle (one all-reduce each).  For meshes whose fields fit every GPU
        # many times over (the SMR decks: 20 / 32 blocks of 32^2 cells) this balances whatever the
        # blocks cost -- a DDMC block of BASELINE configs[4] costs 1 % of an IMC block --, which a
        # partition of 32 blocks over 8 ranks cannot.
        self.replicated = bool(replicated) and nranks > 1
        if self.replicated:
            owner = np.full(mesh.nblocks, rank, dtype=np.int32)
        else:
            owner = np.ascontiguousarray(mesh.owner, dtype=np.int32)
        self.field_owner = owner           # who holds the authoritative copy of a block's fields (halo.py)
        if owner.max() >= nranks:
            raise ValueError("mesh.owner names a rank >= nranks")
        self.gids = np.nonzero(owner == rank)[0].astype(np.int32)       # the blocks this rank owns
        if len(self.gids) == 0:
            raise ValueError(f"rank {rank} owns no blocks")
        self.nowned = len(self.gids)
        # Halo copies: read-only mirrors of the neighbouring ranks' blocks that touch ours.  A
        # particle that wanders across the rank boundary keeps being tracked here and is handed
        # to its owner once, when its history ends, instead of at every crossing (in the
        # reference every crossing costs a transport iteration with a global sync,
        # jaybenne.cpp:113-131).  HBM is plentiful: one ring costs a few GB at most.
        halo = (mesh.neighbours(self.gids, halo_rings) if (nranks > 1 and halo_rings > 0 and not self.replicated)
                else np.zeros(0, dtype=np.int32))
        self.resident_gids = np.concatenate([self.gids, halo]).astype(np.int32)
        self.owned_flags = np.concatenate([np.ones(self.nowned, dtype=np.int32),
                                           np.zeros(len(halo), dtype=np.int32)])
        self.nblocks = len(self.resident_gids)
        local_index = np.full(mesh.nblocks, -1, dtype=np.int32)
        local_index[self.resident_gids] = np.arange(self.nblocks, dtype=np.int32)
        self.local_index = local_index
        shape = (self.nblocks,) + tuple(mesh.field_shape[1:])
        names = list(_lib.FIELD_NAMES)
        use_ddmc = bool(pkg.Param("use_ddmc"))
        self.fields: Dict[str, torch.Tensor] = {}
        for n in names:
            if n in ("P1", "P2", "P3") and not use_ddmc:
                continue
            self.fields[n] = torch.zeros(shape, dtype=torch.float64, device=dev)
        # swarm
        self.capacity = int(capacity)
        self.swarm: Dict[str, torch.Tensor] = {}
        for n in _F64:
            self.swarm[n] = torch.zeros(self.capacity, dtype=torch.float64, device=dev)
        for n in _I32:
            self.swarm[n] = torch.zeros(self.capacity, dtype=torch.int32, device=dev)
        self.swarm["id"] = torch.zeros(self.capacity, dtype=torch.int64, device=dev)   # uint64 bits
        self.swarm["rng"] = torch.zeros(self.capacity, dtype=torch.int64, device=dev)  # uint64 bits
        self.sv = _lib.SwarmView(n=0, capacity=self.capacity)
        for n in _F64 + _I32 + ("id", "rng"):
            setattr(self.sv, n, self.swarm[n].data_ptr())
        self.max_capacity: Optional[int] = None   # set to forbid growth beyond a slot count
        self.prefix = torch.zeros(self.nblocks * mesh.ncell, dtype=torch.int32, device=dev)
        self.records: Optional[torch.Tensor] = None
        self.next_id = 0     # first unused stream id (global, kept in step on every rank)
        self.cycle = 0       # RadiationStep counter (keys the per-cell rounding streams: source_epoch); 0 = initialisation
        self.events = 0
        self.kernel_events = None   # set to [] to time every transport launch with HIP events
        self._exchange = None       # halo.FieldExchange, built on first use
        self.phase_times = None     # set to {} to account wall time per phase of RadiationStep
        # hand-off accounting (bench.py): records this rank handed to others, wall time spent in
        # the exchange phase, transport iterations, since the caller last zeroed them
        self.handoff_records = 0
        self.exchange_seconds = 0.0        # hand-off proper: from the end of the transport launch on
        self.transport_wait_seconds = 0.0  # host time spent waiting for the transport launch
        self.collective_seconds = 0.0      # part of exchange_seconds inside the two collectives
        self.transport_iterations_total = 0
        self._stats_cache = None           # counters as of the end of the last RadiationStep
        # measurement aid (bench.py --force-exchange): run the hand-off phase of the iterate-sublist
        # also when this rank holds the whole mesh (nothing moves; its fixed cost becomes visible)
        self.force_exchange = False
        # How particles are handed to other ranks: "c" (default) = the library's jb_exchange in one call, over a
        # communicator of its own on an RCCL process group and over torch.distributed callbacks otherwise
        # ("c-rccl" / "c-torch" force one); "python" = the same protocol driven from here (comm.py: count
        # kernel, read-back, all-gather, all-to-all-v from Python), kept for A/B; "step" = the whole cycle, its
        # iterate-sublist included, as ONE library call (jb_radiation_step_ranks) whose hand-off is jb_exchange over
        # the transport "c" picks (a replicated mesh keeps its own path).  JB_HANDOFF overrides.
        self.handoff = os.environ.get("JB_HANDOFF", "c")
        if self.handoff not in ("c", "c-torch", "c-rccl", "python", "step"):
            raise ValueError(f"JB_HANDOFF = {self.handoff!r}: one of c, c-torch, c-rccl, python, step")
        self._chandoff = None
        self._rank_comm = None      # JB_HANDOFF=step: the jb_rank_comm of the library call (and its reserve callback)
        self.step_report = None     # ... and the jb_step_report of the last cycle
        # DefragParticles after every k-th RadiationStep (0: never; the reference schedules none)
        # DefragParticles: -1 (default) on the library's schedule (jb_defrag_policy: when a cycle costs
        # 10 % more per event than the best one since the last sort), k > 0 after every k-th cycle,
        # 0 never (the reference: slot order stays what the task list makes it)
        self.defrag_interval = -1
        self.defrags = 0
        self._steps_since_defrag = 0
        # energy ledger (include/jaybenne_amd.h: jb_energy_ledger; enable_ledger, or JB_LEDGER=1 in the environment):
        # the last cycle's ledger as a dict, reduced over the ranks, and every cycle's
        self.ledger: Optional[dict] = None
        self.ledger_history: list = []
        self._ledger_e0: Optional[float] = None     # e_census the next cycle starts from
        self._ledger_handoff = None                 # a transport for jb_ledger_reduce where the hand-off has none
        # census comb (CombCensus; include/jaybenne_amd.h: jb_comb_census_plan): a cell that ends a cycle with more
        # than comb_trigger photons comes out with comb_target; 0 = off (the reference: no population control)
        self.comb_target = 0
        self.comb_trigger = 0
        self.comb_history: list = []                # one dict per cycle whose comb changed the swarm
        self._comb_sorted = False                   # the last plan sorted the swarm
        # global census comb (CombCensusGlobal; include/jaybenne_amd.h: jb_comb_census_weigh): the whole mesh is held
        # near census_total_target photons of equal weight; 0 = off.  Not together with comb_target.
        self.census_total_target = 0
        self.census_total_band = 2.0
        self.census_split_max = 64
        # radiation moments (EvaluateRadiationMoments; include/jaybenne_amd.h: jb_evaluate_radiation_moments): the
        # last call's device tensor (12, nblocks, nx3, nx2, nx1) and report; None until a host asks
        self.moments: Optional[torch.Tensor] = None
        # source allocation (md.source_allocation; include/jaybenne_amd.h: jb_set_source_allocation): E_tot of the last
        # source call under "energy"
        self.source_e_total: Optional[float] = None
        self.moments_report: Optional[dict] = None
        # radiation spectrum (EvaluateRadiationSpectrum; include/jaybenne_amd.h: jb_evaluate_radiation_spectrum): the
        # last call's device tensor (ngroups + 2, nblocks, nx3, nx2, nx1) and report; None until a host asks
        self.spectrum: Optional[torch.Tensor] = None
        self.spectrum_report: Optional[dict] = None
        # exact deposition (md.deposition; include/jaybenne_amd.h: jb_set_deposition): one record per cycle, the
        # counts of its close on this rank (jb_deposit_stats) and the cycle
        self.deposit_history: list = []
        # boundary source (SetBoundarySource; include/jaybenne_amd.h: jb_source_boundary_count): Planckian inflow
        # through the domain faces that carry a temperature; every face off (the default) = the reference
        self.bsource_num_particles = 0              # N_b: photons per cycle over all source faces of the whole mesh
        self.boundary_source_history: list = []     # one record per cycle: e_face / n_face summed over the ranks
        self._bs_temp = [0.0] * 6
        self._bs_prefix: Optional[torch.Tensor] = None
        self._bs_plan = None                        # counted by SourcePhotons(emission), filled by SourceBoundaryPhotons
        self._make_mesh_handle(owner)

    def reserve(self, nslots: int) -> None:
        """Make room for ``nslots`` particles (the role of Parthenon's pool growth inside
        ``Swarm::AddEmptyParticles``, reference sourcing.cpp:123-131): the swarm arrays are
        reallocated at twice the need and the live prefix ``0..n-1`` is carried over."""
        if nslots <= self.capacity:
            return
        if self.max_capacity is not None and nslots > self.max_capacity:
            raise MemoryError(f"swarm capacity {self.max_capacity} too small for {nslots} particles")
        new_cap = 2 * int(nslots)
        if self.max_capacity is not None:
            new_cap = min(new_cap, int(self.max_capacity))
        self._sync_stream()
        n = int(self.sv.n)
        for name in _F64 + _I32 + ("id", "rng"):
            old = self.swarm[name]
            new = torch.zeros(new_cap, dtype=old.dtype, device=old.device)
            new[:n].copy_(old[:n])
            self.swarm[name] = new
            setattr(self.sv, name, new.data_ptr())
        torch.cuda.synchronize(self.device)
        self.capacity = new_cap
        self.sv.capacity = new_cap

    # ---- C views
    def _make_mesh_handle(self, owner: np.ndarray) -> None:
        m = self.mesh
        g = self.resident_gids
        keep = dict(owned=self.owned_flags,
            leaf_map=np.ascontiguousarray(m.leaf_map, dtype=np.int32), owner=owner,
            local_index=self.local_index, gid=np.ascontiguousarray(g, dtype=np.int32),
            blk_xmin=np.ascontiguousarray(m.blk_xmin[g]), blk_xmax=np.ascontiguousarray(m.blk_xmax[g]),
            blk_dx=np.ascontiguousarray(m.blk_dx[g]),
            blk_level=np.ascontiguousarray(m.blk_level[g], dtype=np.int32),
            blk_nbr_lev=np.ascontiguousarray(m.blk_nbr_lev[g], dtype=np.int32))
        v = _lib.MeshView(ndim=m.ndim, ng=m.ng, nblocks=self.nblocks, nblocks_total=m.nblocks,
                          rank=self.rank)
        v.nx = (C.c_int32 * 3)(*m.nx)
        v.nleaf = (C.c_int32 * 3)(*m.nleaf)
        v.bc = (C.c_int32 * 6)(*m.swarm_bc)
        v.gmin = (C.c_double * 3)(*m.gmin)
        v.gmax = (C.c_double * 3)(*m.gmax)
        for k, a in keep.items():
            setattr(v, k, a.ctypes.data)
        ptr_tables = {}
        for n, t in self.fields.items():
            stride = t.stride(0) * t.element_size()
            tab = np.array([t.data_ptr() + b * stride for b in range(self.nblocks)], dtype=np.uint64)
            ptr_tables[n] = tab
            setattr(v, n, tab.ctypes.data)
        handle = C.c_void_p()
        self._sync_stream()
        _lib.check(self.lib.jb_mesh_create(self.pkg.ctx, C.byref(v), C.byref(handle)))
        self.handle = handle

    @property
    def exchange(self):
        """Ghost-zone / halo refresh plan for the host fields (built once per mesh)."""
        if self._exchange is None:
            from .halo import FieldExchange
            self._exchange = FieldExchange(self)
        return self._exchange

    def _sync_stream(self) -> None:
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self.lib.jb_set_stream(self.pkg.ctx, C.c_void_p(stream))

    @property
    def n(self) -> int:
        return int(self.sv.n)

    def ensure_handoff(self) -> None:
        """Makes the C hand-off's transport now (collective over the ranks: jaybenne_amd/handoff.py) instead of
        inside the first exchange."""
        if self.handoff != "python" and self._chandoff is None and self.comm is not None:
            from .handoff import CHandoff
            self._chandoff = CHandoff.make(self, {"c": "auto", "c-torch": "torch", "c-rccl": "rccl",
                                                  "step": "auto"}[self.handoff])

    def handoff_path(self) -> str:
        """What the hand-off of this MeshData runs through (bench.py: ``handoff.path``)."""
        if self.handoff == "python":
            return "python: comm.py (count kernel, read-back, all-gather and all-to-all-v driven from Python)"
        if self.handoff == "step" and not self.replicated:
            inner = f"hand-off {self._chandoff.path}" if self._chandoff is not None else "one rank, no hand-off"
            return f"c: jb_radiation_step_ranks (one call per cycle; {inner})"
        return self._chandoff.path if self._chandoff is not None else "c: jb_exchange (no exchange has run yet)"

    def close(self) -> None:
        if getattr(self, "_chandoff", None) is not None:
            self._chandoff.close()
            self._chandoff = None
        if getattr(self, "_ledger_handoff", None) is not None:
            self._ledger_handoff.close()
            self._ledger_handoff = None
        if getattr(self, "handle", None) is not None:
            self.lib.jb_mesh_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- host <-> device helpers for the harness
    def set_field(self, name: str, host: np.ndarray, local: bool = False) -> None:
        """host: [nblocks_total, nk, nj, ni] (whole mesh; the resident blocks are picked out) or,
        with ``local=True``, [len(resident_gids), nk, nj, ni]."""
        src = host if local else host[self.resident_gids]
        self.fields[name].copy_(torch.from_numpy(np.ascontiguousarray(src)))

    def get_field(self, name: str) -> np.ndarray:
        """The owned blocks' part of a field, in the order of ``gids``."""
        return self.fields[name][:self.nowned].cpu().numpy()

    def get_swarm(self) -> Dict[str, np.ndarray]:
        n = self.n
        out = {k: v[:n].cpu().numpy() for k, v in self.swarm.items()}
        out["id"] = out["id"].view(np.uint64)
        out["rng"] = out["rng"].view(np.uint64)
        return out

    def stats(self, reset: bool = False) -> Dict[str, int]:
        st = _lib.TransportStats()
        _lib.check(self.lib.jb_get_transport_stats(self.pkg.ctx, C.byref(st), int(reset)))
        self._stats_cache = None
        return {k: int(getattr(st, k)) for k, _ in st._fields_}

    # ---- energy ledger
    def enable_ledger(self, on: bool = True) -> None:
        """Switches the energy ledger of the library context on or off (``jb_ledger_enable``).  On: every
        RadiationStep leaves ``md.ledger`` -- the terms of ``jb_energy_ledger`` summed over the ranks, plus
        ``e_start`` (the census energy the cycle started from) and ``residual`` (of
        ``e_start + e_sourced = e_census + e_absorbed + escaped``, relative to the left-hand side) -- and appends
        it to ``md.ledger_history``."""
        self._sync_stream()
        _lib.check(self.lib.jb_ledger_enable(self.pkg.ctx, int(bool(on))))
        self.ledger, self.ledger_history, self._ledger_e0 = None, [], None

    def ledger_enabled(self) -> bool:
        return self.lib.jb_ledger_enabled(self.pkg.ctx) == 1

    # ---- the order of the photons within a cell behind a sort
    @property
    def cell_order(self) -> str:
        """``"any"`` (the default) or ``"id"``: the canonical order -- DefragParticles, the library's schedule and
        the census comb's plan sort by (block, cell, creation id), so that what a comb keeps does not depend on
        the slots the photons came in (include/jaybenne_amd.h: ``jb_set_cell_order``)."""
        return CELL_ORDERS[self.lib.jb_get_cell_order(self.pkg.ctx)]

    @cell_order.setter
    def cell_order(self, mode: str) -> None:
        _lib.check(self.lib.jb_set_cell_order(self.pkg.ctx, cell_order_code(mode)))

    # ---- exact deposition
    @property
    def deposition(self) -> str:
        """``"atomic"`` (the default) or ``"exact"``: energy_delta and the census tally as one rounding of the exact
        sum of their addends -- the same bits whatever the order of the photons, the time of the last sort or the
        number of ranks (include/jaybenne_amd.h: ``jb_set_deposition``).  Every cycle then appends the counts of its
        close to ``md.deposit_history``."""
        return DEPOSITIONS[self.lib.jb_get_deposition(self.pkg.ctx)]

    @deposition.setter
    def deposition(self, mode: str) -> None:
        if mode == "exact" and self.replicated:
            raise ValueError("deposition = 'exact': a replicated mesh sums its fields over the ranks in floating point")
        _lib.check(self.lib.jb_set_deposition(self.pkg.ctx, deposition_code(mode)))

    # ---- source tilt
    @property
    def source_tilt(self) -> str:
        """``"none"`` (the default) or ``"linear"``: within a cell the emission probability of ``SourcePhotons``
        follows the gradient of T^4 taken from the neighbouring cells instead of being uniform
        (include/jaybenne_amd.h: ``jb_set_source_tilt``).  Ids and draws do not depend on it."""
        return SOURCE_TILTS[self.lib.jb_get_source_tilt(self.pkg.ctx)]

    @source_tilt.setter
    def source_tilt(self, mode: str) -> None:
        _lib.check(self.lib.jb_set_source_tilt(self.pkg.ctx, source_tilt_code(mode)))

    def source_tilt_slopes(self) -> np.ndarray:
        """The slopes of the last ``SourcePhotons`` count under ``linear``, ``[owned blocks, 3, nx3, nx2, nx1]``
        (``jb_source_tilt_slopes``; zeros on inactive axes)."""
        m = self.mesh
        out = np.zeros((self.nowned, 3, m.ncell), dtype=np.float64)
        self._sync_stream()
        for b in range(self.nowned):
            _lib.check(self.lib.jb_source_tilt_slopes(self.pkg.ctx, self.handle, b, out[b].ctypes.data))
        return out.reshape((self.nowned, 3) + tuple(int(n) for n in m.nx[::-1]))

    # ---- source allocation
    @property
    def source_allocation(self) -> str:
        """``"uniform"`` (the default: every cell the same number of new photons, sourcing.cpp:68-69) or ``"energy"``:
        ``SourcePhotons`` gives a cell photons in proportion to the energy it sources, ``num_particles`` over the whole
        mesh per call, so that the new photons carry nearly equal weights (include/jaybenne_amd.h:
        ``jb_set_source_allocation``)."""
        return SOURCE_ALLOCATIONS[self.lib.jb_get_source_allocation(self.pkg.ctx)]

    @source_allocation.setter
    def source_allocation(self, mode: str) -> None:
        _lib.check(self.lib.jb_set_source_allocation(self.pkg.ctx, source_allocation_code(mode)))

    def deposit_close(self) -> dict:
        """``jb_deposit_close`` on this rank's swarm, then the counts of that close (``jb_deposit_last``)."""
        self._sync_stream()
        _lib.check(self.lib.jb_deposit_close(self.pkg.ctx, self.handle, C.byref(self.sv)))
        return self.deposit_last()

    def deposit_last(self) -> dict:
        st = _lib.DepositStats()
        _lib.check(self.lib.jb_deposit_last(self.pkg.ctx, C.byref(st)))
        return st.as_dict()

    def _ledger_transport(self):
        """The jb_exchange_transport the ledgers of several ranks are gathered through."""
        if self.nranks == 1:
            return None
        if self.handoff != "python":
            self.ensure_handoff()
            return C.byref(self._chandoff.tr)
        if self._ledger_handoff is None:
            from .handoff import CHandoff
            self._ledger_handoff = CHandoff(self, "torch")
        return C.byref(self._ledger_handoff.tr)

    def _ledger_reduce(self, led: "_lib.EnergyLedger") -> None:
        if self.nranks > 1:
            self._sync_stream()
            _lib.check(self.lib.jb_ledger_reduce(self.pkg.ctx, self._ledger_transport(), self.rank, self.nranks,
                                                 int(self.replicated), C.byref(led)))

    def _ledger_begin(self, t_start: float) -> None:
        """Before the first cycle with the ledger on: the census energy it starts from (a close of its own)."""
        if self._ledger_e0 is None:
            led = _lib.EnergyLedger()
            self._sync_stream()
            _lib.check(self.lib.jb_ledger_close(self.pkg.ctx, self.handle, C.byref(self.sv), t_start, 0.0, C.byref(led)))
            self._ledger_reduce(led)
            self._ledger_e0 = float(led.e_census)

    def _ledger_record(self, led: "_lib.EnergyLedger") -> None:
        d = led.as_dict()
        d["e_start"] = self._ledger_e0
        d["residual"] = _lib.ledger_residual(d, self._ledger_e0)
        self._ledger_e0 = d["e_census"]
        self.ledger = d
        self.ledger_history.append(d)

    def invariants_enabled(self) -> bool:
        """True under the checked library (libjaybenne_amd_checked.so, selected by JAYBENNE_AMD_LIB)."""
        return self.lib.jb_invariants_enabled() == 1

    def invariant_report(self, reset: bool = False) -> Dict[str, object]:
        """The checked library's transport-invariant counts (jb_invariant_report_get): per kind evaluated and
        violated, per kernel family the lane-passes checked, and the first violation (None when there is
        none).  JaybenneError (JB_ERR_UNSUPPORTED) under the release library."""
        r = _lib.InvariantReport()
        _lib.check(self.lib.jb_invariant_report_get(self.pkg.ctx, C.byref(r), int(reset)))
        return r.as_dict()

    def verify_swarm(self, t_start: float, t_end: float) -> Dict[str, object]:
        """The SWARM sweep over the live photons now (jb_verify_swarm); the counts of this sweep alone.
        Does not raise on a violation: the caller reads the counts."""
        r = _lib.InvariantReport()
        st = self.lib.jb_verify_swarm(self.pkg.ctx, self.handle, C.byref(self.sv), float(t_start), float(t_end),
                                      C.byref(r))
        if st < 0 and st != _lib.JB_ERR_INVARIANT:
            _lib.check(st)
        return r.as_dict()


# ------------------------------------------------------------------------------------------------
# tasks (reference jaybenne.hpp:59-76)
def UpdateDerivedTransportFields(md: MeshData, dt: float) -> TaskStatus:
    md._sync_stream()
    _lib.check(md.lib.jb_update_derived_transport_fields(md.pkg.ctx, md.handle, dt))
    return TaskStatus.complete


def _global_block_counts(md: MeshData, nper_local: np.ndarray) -> np.ndarray:
    counts = np.zeros(md.mesh.nblocks, dtype=np.int64)
    counts[md.resident_gids] = nper_local        # halo copies source nothing (zeros)
    if md.comm is not None and md.nranks > 1 and not md.replicated:
        counts = md.comm.allreduce_sum_int64(counts)
    return counts     # (replicated mesh: every rank has counted every block itself)


def rank_share(nper: np.ndarray, rank: int, nranks: int):
    """Which of a block's ``nper[b]`` new photons (numbered in cell order, as their stream ids are)
    rank ``rank`` of a replicated-mesh run sources: a contiguous range per block, ``first[b]`` ..
    ``first[b] + count[b]`` -- contiguous cells, so a rank's photons start out as compact in space as
    the whole swarm's do."""
    n = nper.astype(np.int64)
    first = (n * rank) // nranks
    return first.astype(np.int32), ((n * (rank + 1)) // nranks - first).astype(np.int32)


def _sum_over_ranks(md: MeshData, names) -> None:
    """Replicated mesh: the ranks' partial cell fields -> their sum, on every rank."""
    if md.replicated:
        for n in names:
            md.comm.allreduce_sum_tensor(md.fields[n])


def gather_block_energies(md: MeshData, e_local: np.ndarray) -> np.ndarray:
    """The block sums of the whole mesh by global block id from this rank's (``jb_source_energy_sums``: one per
    resident block, 0 for a halo copy).  On a block partition they travel as bit patterns in a zero-filled int64
    array through the integer all-reduce: each block has one owner, so the integer sum is an exact gather.  On a
    replicated mesh every rank has summed every block itself."""
    bits = np.zeros(md.mesh.nblocks, dtype=np.int64)
    bits[md.gids] = np.ascontiguousarray(e_local[:md.nowned], dtype=np.float64).view(np.int64)
    if md.comm is not None and md.nranks > 1 and not md.replicated:
        bits = np.ascontiguousarray(md.comm.allreduce_sum_int64(bits), dtype=np.int64)
    return bits.view(np.float64)


def _count_by_energy(md: MeshData, source_type, dt: float, nper: np.ndarray) -> float:
    """The count of a source call under ``source_allocation = energy``: energy pass, the total over the global block
    ids in rising order (the library's host helper, so that every host adds alike), count pass.  Fills ``nper`` and
    ``md.prefix``; returns ``E_tot``."""
    pkg = md.pkg
    e_local = np.zeros(md.nblocks, dtype=np.float64)
    _lib.check(md.lib.jb_source_energy_sums(pkg.ctx, md.handle, int(source_type), dt, e_local.ctypes.data))
    e_gid = np.ascontiguousarray(gather_block_energies(md, e_local), dtype=np.float64)
    e_total = float(md.lib.jb_source_energy_total(e_gid.ctypes.data, int(md.mesh.nblocks)))
    _lib.check(md.lib.jb_source_photons_count_energy(pkg.ctx, md.handle, int(source_type), dt,
                                                     source_epoch(md.cycle, source_type), e_total,
                                                     nper.ctypes.data, md.prefix.data_ptr()))
    return e_total


def source_epoch(cycle: int, source_type) -> int:
    """Key of the per-cell rounding streams of a source call (include/jaybenne_amd.hpp: SourceEpoch,
    shared by every host): 0 for the initial thermal source, k for the emission source of cycle k."""
    if int(source_type) == int(SourceType.emission):
        return int(cycle)
    return 0 if cycle == 0 else (1 << 19) | int(cycle)


def SourcePhotons(md: MeshData, source_type: SourceType, t_start: float, dt: float,
                  per_block: bool = False) -> TaskStatus:
    """``SourcePhotons<T, ST>(md, t_start, dt)`` -- reference sourcing.cpp:25-208.
    ``per_block=True`` is the ``MeshBlockData`` instantiation used at initialisation (one call
    per block, so the ``nblocks`` of sourcing.cpp:68-69 is 1)."""
    pkg = md.pkg
    if pkg.Param("source_strategy") == SourceStrategy.energy:
        raise NotImplementedError("Energy source strategy not implemented!")
    if source_type == SourceType.emission and not pkg.Param("do_emission"):
        return TaskStatus.complete
    md._sync_stream()
    nper = np.zeros(md.nblocks, dtype=np.int32)
    blocks_in_call = 1 if per_block else md.nowned   # vmesh.GetNBlocks() of this rank's MeshData
    if md.source_allocation == "energy":
        # (num_particles over the whole mesh, dealt to the cells by the energy they source: the ranks' block sums are
        # gathered between the energy pass and the count pass -- include/jaybenne_amd.h: jb_set_source_allocation)
        md.source_e_total = _count_by_energy(md, source_type, dt, nper)
    else:
        _lib.check(md.lib.jb_source_photons_count(pkg.ctx, md.handle, int(source_type), dt,
                                                  blocks_in_call, source_epoch(md.cycle, source_type),
                                                  nper.ctypes.data, md.prefix.data_ptr()))
    if source_type == SourceType.emission and boundary_source_on(md):
        # the boundary photons of block b take the ids behind its emission photons: counted before the ids are dealt
        return _source_emission_and_count_boundary(md, nper, t_start, dt)
    counts = _global_block_counts(md, nper)
    excl = np.concatenate(([0], np.cumsum(counts)[:-1]))
    id_base = np.ascontiguousarray(md.next_id + excl[md.resident_gids], dtype=np.uint64)
    if md.replicated:    # this rank's share of every block (stream ids stay those of the whole block)
        first, nper = rank_share(nper, md.rank, md.nranks)
    local_excl = np.concatenate(([0], np.cumsum(nper.astype(np.int64))[:-1]))
    slot_base = np.ascontiguousarray(md.n + local_excl, dtype=np.int64)
    tot = int(nper.sum())
    md.reserve(md.n + tot)
    if md.replicated:
        _lib.check(md.lib.jb_source_photons_fill_range(pkg.ctx, md.handle, C.byref(md.sv), int(source_type),
                                                       t_start, dt, nper.ctypes.data, md.prefix.data_ptr(),
                                                       slot_base.ctypes.data, id_base.ctypes.data,
                                                       first.ctypes.data, int(md.rank == 0)))
    else:
        _lib.check(md.lib.jb_source_photons_fill(pkg.ctx, md.handle, C.byref(md.sv), int(source_type),
                                                 t_start, dt, nper.ctypes.data, md.prefix.data_ptr(),
                                                 slot_base.ctypes.data, id_base.ctypes.data))
    md.sv.n += tot
    md.next_id += int(counts.sum())
    return TaskStatus.complete


# ---- boundary source: Planckian inflow through chosen domain faces (include/jaybenne_amd.h) ----------------
FACE_NAMES = _lib.LEDGER_FACES      # ix1, ox1, ix2, ox2, ix3, ox3


def SetBoundarySource(md: MeshData, face: int, temperature: float) -> None:
    """A black wall of temperature ``temperature`` behind domain face ``face`` (0..5 = ix1 .. ox3); 0 = off.  The
    face must belong to an active axis and its swarm boundary must not be periodic (checked by the count call,
    where the mesh is known); a replicated mesh has no boundary source."""
    if md.replicated and temperature > 0:
        raise ValueError("the boundary source needs the blocks dealt to the ranks: not with a replicated mesh")
    _lib.check(md.lib.jb_set_boundary_source(md.pkg.ctx, int(face), float(temperature)))
    md._bs_temp[int(face)] = float(temperature)
    _set_boundary_source_count(md)


def boundary_source_on(md: MeshData) -> bool:
    return any(t > 0.0 for t in md._bs_temp)


def boundary_face_cells_total(md: MeshData) -> int:
    """Source face cells of the WHOLE mesh under the faces now set (the same on every rank: from the global mesh)."""
    m = md.mesh
    total = 0
    for f, t in enumerate(md._bs_temp):
        d = f >> 1
        if not t > 0.0 or d >= m.ndim:
            continue
        half = 0.5 * m.blk_dx[:, d]
        on = (m.blk_xmax[:, d] > m.gmax[d] - half) if f & 1 else (m.blk_xmin[:, d] < m.gmin[d] + half)
        total += int(on.sum()) * (m.ncell // int(m.nx[d]))
    return total


def _set_boundary_source_count(md: MeshData) -> None:
    # (what the library's own step calls -- JB_HANDOFF=step -- ask for)
    _lib.check(md.lib.jb_set_boundary_source_count(md.pkg.ctx, int(md.bsource_num_particles),
                                                   boundary_face_cells_total(md)))


def _count_boundary(md: MeshData, dt: float):
    """jb_source_boundary_count: (photons per resident block, the rank's record)."""
    if md.replicated:
        raise ValueError("the boundary source needs the blocks dealt to the ranks: not with a replicated mesh")
    words = int(md.lib.jb_boundary_prefix_words(md.handle))
    if md._bs_prefix is None or md._bs_prefix.numel() < words:
        md._bs_prefix = torch.zeros(words, dtype=torch.int32, device=md.device)
    nper = np.zeros(md.nblocks, dtype=np.int32)
    plan = _lib.BoundarySourcePlan(nper_block=nper.ctypes.data)
    md._sync_stream()
    _lib.check(md.lib.jb_source_boundary_count(md.pkg.ctx, md.handle, dt, boundary_face_cells_total(md),
                                               int(md.bsource_num_particles), source_epoch(md.cycle, SourceType.emission),
                                               C.byref(plan), md._bs_prefix.data_ptr()))
    return nper, dict(e_face=[float(v) for v in plan.e_face], n_face=[int(v) for v in plan.n_face])


def _source_emission_and_count_boundary(md: MeshData, nper_em: np.ndarray, t_start: float, dt: float) -> TaskStatus:
    """The emission source's fill with the boundary source on: block b takes ``n_em[b] + n_bs[b]`` consecutive ids,
    the emission photons first (include/jaybenne_amd.hpp: PlanSourceWithBoundary).  The boundary photons are counted
    here and filled by ``SourceBoundaryPhotons``."""
    pkg = md.pkg
    nper_bs, rec = _count_boundary(md, dt)
    counts = _global_block_counts(md, nper_em.astype(np.int64) + nper_bs)
    excl = np.concatenate(([0], np.cumsum(counts)[:-1]))
    id_base = np.ascontiguousarray(md.next_id + excl[md.resident_gids], dtype=np.uint64)
    local_excl = np.concatenate(([0], np.cumsum(nper_em.astype(np.int64))[:-1]))
    slot_base = np.ascontiguousarray(md.n + local_excl, dtype=np.int64)
    tot = int(nper_em.sum())
    md.reserve(md.n + tot + int(nper_bs.sum()))
    _lib.check(md.lib.jb_source_photons_fill(pkg.ctx, md.handle, C.byref(md.sv), int(SourceType.emission),
                                             t_start, dt, nper_em.ctypes.data, md.prefix.data_ptr(),
                                             slot_base.ctypes.data, id_base.ctypes.data))
    md.sv.n += tot
    md.next_id += int(counts.sum())
    md._bs_plan = dict(nper=nper_bs, id_base=np.ascontiguousarray(id_base + nper_em.astype(np.uint64), dtype=np.uint64),
                       rec=rec, cycle=md.cycle)
    return TaskStatus.complete


def SourceBoundaryPhotons(md: MeshData, t_start: float, dt: float) -> TaskStatus:
    """The boundary source of one cycle, right behind ``SourcePhotons(emission)``: every source face cell emits
    ``sb T_f^4 A dt`` in photons born ``eps_imc dx`` inside it with a cosine-law inward direction
    (include/jaybenne_amd.h).  Appends the cycle's record -- ``e_face`` / ``n_face``, summed over the ranks -- to
    ``md.boundary_source_history``.  With every face off: nothing, and no kernel."""
    if not boundary_source_on(md):
        return TaskStatus.complete
    pkg = md.pkg
    plan, md._bs_plan = md._bs_plan, None
    if plan is None or plan["cycle"] != md.cycle:      # (no emission source in front: the boundary photons alone)
        nper, rec = _count_boundary(md, dt)
        counts = _global_block_counts(md, nper)
        excl = np.concatenate(([0], np.cumsum(counts)[:-1]))
        plan = dict(nper=nper, id_base=np.ascontiguousarray(md.next_id + excl[md.resident_gids], dtype=np.uint64),
                    rec=rec)
        md.next_id += int(counts.sum())
    nper = plan["nper"]
    local_excl = np.concatenate(([0], np.cumsum(nper.astype(np.int64))[:-1]))
    slot_base = np.ascontiguousarray(md.n + local_excl, dtype=np.int64)
    tot = int(nper.sum())
    md.reserve(md.n + tot)
    md._sync_stream()
    _lib.check(md.lib.jb_source_boundary_fill(pkg.ctx, md.handle, C.byref(md.sv), t_start, dt, nper.ctypes.data,
                                              md._bs_prefix.data_ptr(), slot_base.ctypes.data,
                                              plan["id_base"].ctypes.data))
    md.sv.n += tot
    _record_boundary_source(md, plan["rec"])
    return TaskStatus.complete


def _record_boundary_source(md: MeshData, rec: dict) -> None:
    """One cycle's per-face sourced energy and photons, summed over the ranks (in rank order: the same bits on all)."""
    e, n = np.array(rec["e_face"]), np.array(rec["n_face"], dtype=np.int64)
    if md.comm is not None and md.nranks > 1:
        both = np.zeros((md.nranks, 12), dtype=np.int64)
        both[md.rank, :6] = e.view(np.int64)
        both[md.rank, 6:] = n
        both = md.comm.allreduce_sum_int64(both.reshape(-1)).reshape(md.nranks, 12)
        e = np.zeros(6)
        for r in range(md.nranks):
            e = e + both[r, :6].copy().view(np.float64)
        n = both[:, 6:].sum(axis=0)
    md.boundary_source_history.append(dict(cycle=md.cycle, e_face=[float(v) for v in e], n_face=[int(v) for v in n]))


def _transport(md: MeshData, t_start: float, dt: float, first: int, last: Optional[int],
               fuse_census_tally: bool, ddmc: bool) -> TaskStatus:
    md._sync_stream()
    md._stats_cache = None       # (a transport launch outside RadiationStep moves the counters)
    last = md.n if last is None else last
    fn = md.lib.jb_transport_photons_ddmc if ddmc else md.lib.jb_transport_photons
    timed = md.kernel_events is not None and last > first
    if timed:   # HIP events on the stream the kernel is launched on (bench.py roofline)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(torch.cuda.current_stream(md.device))
    _lib.check(fn(md.pkg.ctx, md.handle, C.byref(md.sv), t_start, dt, first, last,
                  int(fuse_census_tally)))
    if timed:
        ev1.record(torch.cuda.current_stream(md.device))
        md.kernel_events.append((ev0, ev1, last - first))
    return TaskStatus.complete


def TransportPhotons(md: MeshData, t_start: float, dt: float, first: int = 0,
                     last: Optional[int] = None, fuse_census_tally: bool = False) -> TaskStatus:
    """reference transport.cpp:28-181"""
    return _transport(md, t_start, dt, first, last, fuse_census_tally, False)


def TransportPhotons_DDMC(md: MeshData, t_start: float, dt: float, first: int = 0,
                          last: Optional[int] = None, fuse_census_tally: bool = False) -> TaskStatus:
    """reference transport_ddmc.cpp:28-237"""
    return _transport(md, t_start, dt, first, last, fuse_census_tally, True)


def SampleDDMCBlockFace(md: MeshData, first: int = 0, last: Optional[int] = None) -> TaskStatus:
    """reference sample_ddmc_bface.cpp:81-427"""
    md._sync_stream()
    last = md.n if last is None else last
    _lib.check(md.lib.jb_sample_ddmc_block_face(md.pkg.ctx, md.handle, C.byref(md.sv), first, last))
    return TaskStatus.complete


def CheckCompletion(md: MeshData, t_end: float) -> TaskStatus:
    """reference transport.cpp:187-216 (local part; the global_sync of jaybenne.cpp:130-131 is
    the all-reduce in RadiationStep)"""
    md._sync_stream()
    unfinished = C.c_int64(0)
    st = _lib.check(md.lib.jb_check_completion(md.pkg.ctx, C.byref(md.sv), t_end,
                                               C.byref(unfinished)))
    md.num_unfinished = int(unfinished.value)
    return TaskStatus(st)


def EvaluateRadiationEnergy(md: MeshData) -> TaskStatus:
    """reference jaybenne.cpp:514-564"""
    md._sync_stream()
    _lib.check(md.lib.jb_evaluate_radiation_energy(md.pkg.ctx, md.handle, C.byref(md.sv)))
    _sum_over_ranks(md, ("tally",))
    return TaskStatus.complete


def EvaluateRadiationMoments(md: MeshData):
    """Per-cell count, energy density, sum of squared weights, flux and second-moment tensor of the census (the
    reference has no such task; include/jaybenne_amd.h: ``jb_evaluate_radiation_moments``).  Returns ``(moments,
    report)``: a device tensor of shape ``(12, nblocks, nx3, nx2, nx1)`` in the order of ``_lib.MOMENT_NAMES`` over
    the resident blocks (zeros in halo copies), also kept as ``md.moments``, and the call's report as a dict.  The
    call sorts the swarm by (block, cell) when it is not in that order.  On a replicated mesh every rank holds a
    share of every cell's photons and every component is linear in the photons: the ranks' tensors are summed with
    the all-reduce the tally uses (and the counts of the report over the ranks).  On a block partition a cell's
    photons are on its owner and nothing is reduced."""
    md._sync_stream()
    nx = md.mesh.nx
    shape = (_lib.JB_MOMENTS, md.nblocks, int(nx[2]), int(nx[1]), int(nx[0]))
    if md.moments is None or tuple(md.moments.shape) != shape:
        md.moments = torch.empty(shape, dtype=torch.float64, device=md.device)
    assert md.moments.numel() == int(md.lib.jb_moments_words(md.handle))
    rep = _lib.MomentsReport()
    _lib.check(md.lib.jb_evaluate_radiation_moments(md.pkg.ctx, md.handle, C.byref(md.sv), md.moments.data_ptr(),
                                                    C.byref(rep)))
    report = rep.as_dict()
    if md.replicated:
        md.comm.allreduce_sum_tensor(md.moments)
        keys = ("n_counted", "n_skipped")
        total = md.comm.allreduce_sum_int64(np.array([report[k] for k in keys], dtype=np.int64))
        report.update({k: int(v) for k, v in zip(keys, total)})
        report["cells_nonempty"] = int((md.moments[0] > 0).sum().item())
        report["longest_run"] = int(md.moments[0].max().item()) if md.moments[0].numel() else 0
    md.moments_report = report
    return md.moments, report


def EvaluateRadiationSpectrum(md: MeshData, edges):
    """Per-cell energy density of the census in frequency groups (the reference has no such task;
    include/jaybenne_amd.h: ``jb_evaluate_radiation_spectrum``).  ``edges``: ``ngroups + 1`` finite, strictly
    increasing photon energies; a photon's bin is the number of edges ``<= e``, so bin 0 lies below the first edge and
    bin ``ngroups + 1`` at or above the last.  Returns ``(spectrum, report)``: a device tensor of shape
    ``(ngroups + 2, nblocks, nx3, nx2, nx1)`` over the resident blocks (zeros in halo copies), also kept as
    ``md.spectrum``, and the call's report as a dict.  Sorts the swarm and reduces over the ranks of a replicated mesh
    exactly as ``EvaluateRadiationMoments`` does; ``cells_nonempty`` and ``longest_run`` are then the largest of the
    ranks' own."""
    md._sync_stream()
    edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    ngroups = int(edges.size) - 1
    words = int(md.lib.jb_spectrum_words(md.handle, ngroups))
    if words == 0:
        raise ValueError(f"EvaluateRadiationSpectrum: {edges.size} edges; "
                         f"2 .. {_lib.JB_SPECTRUM_MAX_GROUPS + 1} are allowed")
    nx = md.mesh.nx
    shape = (ngroups + 2, md.nblocks, int(nx[2]), int(nx[1]), int(nx[0]))
    if md.spectrum is None or tuple(md.spectrum.shape) != shape:
        md.spectrum = torch.empty(shape, dtype=torch.float64, device=md.device)
    assert md.spectrum.numel() == words
    rep = _lib.SpectrumReport()
    _lib.check(md.lib.jb_evaluate_radiation_spectrum(md.pkg.ctx, md.handle, C.byref(md.sv), edges.ctypes.data, ngroups,
                                                     md.spectrum.data_ptr(), C.byref(rep)))
    report = rep.as_dict()
    if md.replicated:
        md.comm.allreduce_sum_tensor(md.spectrum)
        keys = ("n_counted", "n_skipped", "n_below", "n_above")
        total = md.comm.allreduce_sum_int64(np.array([report[k] for k in keys], dtype=np.int64))
        report.update({k: int(v) for k, v in zip(keys, total)})
        for k in ("cells_nonempty", "longest_run"):                # (below 2^53: exact as floats)
            report[k] = int(md.comm.allreduce_max_float(float(report[k])))
    md.spectrum_report = report
    return md.spectrum, report


def UpdateFluid(md: MeshData) -> TaskStatus:
    """reference jaybenne.cpp:583-615"""
    md._sync_stream()
    _lib.check(md.lib.jb_update_fluid(md.pkg.ctx, md.handle))
    return TaskStatus.complete


def PhotonReflectBC(md: MeshData, face: int) -> None:
    """reference boundaries.hpp:24-84; face 0..5 = inner_x1, outer_x1, inner_x2, ..."""
    md._sync_stream()
    _lib.check(md.lib.jb_photon_reflect_bc(md.pkg.ctx, md.handle, C.byref(md.sv), face))


def RemoveMarkedParticles(md: MeshData) -> int:
    md._sync_stream()
    _lib.check(md.lib.jb_remove_marked_particles(md.pkg.ctx, C.byref(md.sv)))
    return md.n


def DefragParticles(md: MeshData) -> TaskStatus:
    """reference jaybenne.cpp:499-509 (``Swarm::Defrag``; scheduled by no task list of the
    reference).  The swarm here is always compact after RemoveMarkedParticles; what this task
    restores is its *order*: the photons sorted by (block, cell), as they are sourced -- the order
    that keeps the cell data a wave gathers in the L2 of its XCD, and that diffusion loosens from
    cycle to cycle (include/jaybenne_amd.h: ``jb_defrag_particles``; in place).
    ``MeshData.defrag_interval = k`` makes RadiationStep schedule it after every k-th cycle."""
    if md.n == 0:
        return TaskStatus.complete
    md._sync_stream()
    _lib.check(md.lib.jb_defrag_particles(md.pkg.ctx, md.handle, C.byref(md.sv)))
    md.defrags += 1
    return TaskStatus.complete


CELL_ORDERS = ("any", "id")
DEPOSITIONS = ("atomic", "exact")
SOURCE_TILTS = ("none", "linear")
SOURCE_ALLOCATIONS = ("uniform", "energy")


def source_allocation_code(mode: str, key: str = "source_allocation") -> int:
    """``JB_ALLOC_UNIFORM`` / ``_ENERGY`` of ``uniform`` / ``energy`` (the values of the deck key
    ``<jaybenne_amd> source_allocation``); anything else is an error that names ``key``."""
    if mode not in SOURCE_ALLOCATIONS:
        raise ValueError(f"{key} = {mode!r}: one of uniform, energy")
    return SOURCE_ALLOCATIONS.index(mode)


def SetSourceAllocation(md: "MeshData", mode: str) -> None:
    """``md.source_allocation = mode``: ``"uniform"`` or ``"energy"`` (include/jaybenne_amd.h:
    ``jb_set_source_allocation``)."""
    md.source_allocation = mode


def source_tilt_code(mode: str, key: str = "source_tilt") -> int:
    """``JB_TILT_NONE`` / ``_LINEAR`` of ``none`` / ``linear`` (the values of the deck key
    ``<jaybenne_amd> source_tilt``); anything else is an error that names ``key``."""
    if mode not in SOURCE_TILTS:
        raise ValueError(f"{key} = {mode!r}: one of none, linear")
    return SOURCE_TILTS.index(mode)


def SetSourceTilt(md: "MeshData", mode: str) -> None:
    """``md.source_tilt = mode``: ``"none"`` or ``"linear"`` (include/jaybenne_amd.h: ``jb_set_source_tilt``)."""
    md.source_tilt = mode


def deposition_code(mode: str, key: str = "deposition") -> int:
    """``JB_DEPOSIT_ATOMIC`` / ``_EXACT`` of ``atomic`` / ``exact`` (the values of the deck key
    ``<jaybenne_amd> deposition``); anything else is an error that names ``key``."""
    if mode not in DEPOSITIONS:
        raise ValueError(f"{key} = {mode!r}: one of atomic, exact")
    return DEPOSITIONS.index(mode)


def cell_order_code(mode: str, key: str = "cell_order") -> int:
    """``JB_CELL_ORDER_ANY`` / ``_BY_ID`` of ``any`` / ``id`` (the values of the deck key ``<jaybenne_amd> cell_order``);
    anything else is an error that names ``key``."""
    if mode not in CELL_ORDERS:
        raise ValueError(f"{key} = {mode!r}: one of any, id")
    return CELL_ORDERS.index(mode)


def comb_trigger_of(target: int, trigger: float) -> int:
    """``T = ceil(trigger * K)`` of the deck keys ``census_per_cell_max = K`` and ``census_comb_trigger`` (every host
    forms it this way)."""
    if target < 0:
        raise ValueError("census_per_cell_max must be >= 0")
    if not trigger >= 1.0:
        raise ValueError("census_comb_trigger must be >= 1")
    return int(np.ceil(trigger * target))


def CombCensus(md: MeshData) -> Optional[dict]:
    """Census population control at the end of a cycle (the reference has none): every cell that holds more than
    ``md.comb_trigger`` ACTIVE photons comes out with exactly ``md.comb_target`` of equal weight, its energy kept
    (include/jaybenne_amd.h: ``jb_comb_census_plan`` / ``_apply``).  The plan sorts the swarm by (block, cell).
    Census photons live in owned blocks, so the comb is local to a rank; the new creation ids are dealt like the
    source's: the ranks gather their counts, ``id_base = next_id + the counts of the lower ranks``, and ``next_id``
    advances by the total on every rank.  Returns the cycle's record (also appended to ``md.comb_history``) when
    the comb changed a swarm anywhere, else None."""
    if md.comb_target <= 0:
        return None
    if md.replicated:
        raise ValueError("the census comb needs the photons of a cell on one rank: not with a replicated mesh")
    md._sync_stream()
    plan = _lib.CombPlan()
    _lib.check(md.lib.jb_comb_census_plan(md.pkg.ctx, md.handle, C.byref(md.sv), int(md.comb_trigger),
                                          int(md.comb_target), int(md.cycle), C.byref(plan)))
    md._comb_sorted = bool(plan.sorted)
    new_ids = np.zeros(md.nranks, dtype=np.int64)
    new_ids[md.rank] = int(plan.n_new_ids)
    combed = np.zeros(md.nranks, dtype=np.int64)
    combed[md.rank] = int(plan.cells_combed)
    if md.comm is not None and md.nranks > 1:
        both = md.comm.allreduce_sum_int64(np.concatenate([new_ids, combed]))
        new_ids, combed = both[:md.nranks], both[md.nranks:]
    rec = None
    if plan.cells_combed > 0:
        rep = _lib.CombReport()
        id_base = md.next_id + int(new_ids[:md.rank].sum())
        _lib.check(md.lib.jb_comb_census_apply(md.pkg.ctx, md.handle, C.byref(md.sv), id_base, C.byref(rep)))
        rec = dict(cycle=md.cycle, n_before=int(plan.n_before), n_after=int(rep.n_after),
                   n_new_ids=int(rep.n_new_ids), id_base=id_base, cells_combed=int(plan.cells_combed),
                   max_per_cell=int(plan.max_per_cell), e_before=float(plan.e_before), e_after=float(rep.e_after))
    elif int(combed.sum()) > 0:   # (another rank's swarm changed: the cycle is on record here too)
        rec = dict(cycle=md.cycle, n_before=int(plan.n_before), n_after=int(plan.n_after), n_new_ids=0,
                   id_base=md.next_id + int(new_ids[:md.rank].sum()), cells_combed=0,
                   max_per_cell=int(plan.max_per_cell), e_before=float(plan.e_before), e_after=float(plan.e_before))
    md.next_id += int(new_ids.sum())
    if rec is not None:
        md.comb_history.append(rec)
    return rec


def check_census_total(target: int, band: float, split_max: int, per_cell_max: int = 0) -> None:
    """The ranges of the deck keys ``census_total_target``, ``census_total_band`` and ``census_split_max`` (every host
    checks them this way), and that the global comb is not asked for together with the per-cell comb."""
    if not 0 <= target < (1 << 31):
        raise ValueError("census_total_target must be in [0, 2^31)")
    if not (band >= 1.0 and np.isfinite(band)):
        raise ValueError("census_total_band must be a finite number >= 1")
    if split_max < 1:
        raise ValueError("census_split_max must be >= 1")
    if target > 0 and per_cell_max > 0:
        raise ValueError("census_total_target and census_per_cell_max: one comb at a time -- the global comb deals the "
                         "cells their shares itself")


def CombCensusGlobal(md: MeshData) -> Optional[dict]:
    """Census population control for the whole mesh at the end of a cycle (the reference has none): the swarm is held
    near ``md.census_total_target = N`` photons of equal weight.  N is dealt to the cells in proportion to the census
    energy they hold; a cell whose count is off its share by more than the factor ``md.census_total_band`` is combed to
    its share -- thinned or split, at most to ``md.census_split_max`` times its count -- and keeps its energy
    (include/jaybenne_amd.h: ``jb_comb_census_weigh`` / ``_plan_global`` / ``_apply``).  The block sums of the census
    energy are gathered by global block id and added by ``jb_source_energy_total``, so every rank divides by the same
    total; ids are dealt as ``CombCensus`` deals them.  Returns the cycle's record (also appended to
    ``md.comb_history``, ``mode="global"``) when the comb changed a swarm anywhere, else None."""
    N = int(md.census_total_target)
    if N <= 0:
        return None
    if md.replicated:
        raise ValueError("the census comb needs the photons of a cell on one rank: not with a replicated mesh")
    band, S = float(md.census_total_band), int(md.census_split_max)
    check_census_total(N, band, S, int(md.comb_target))
    md._sync_stream()
    n = int(md.sv.n)
    n_room = min(n + N, S * n)          # (n_after <= n + N: every combed cell had a photon)
    md.reserve(n_room)
    plan = _lib.CombGlobalPlan()
    e_local = np.zeros(md.nblocks, dtype=np.float64)
    _lib.check(md.lib.jb_comb_census_weigh(md.pkg.ctx, md.handle, C.byref(md.sv), n_room, e_local.ctypes.data,
                                           C.byref(plan)))
    e_gid = np.ascontiguousarray(gather_block_energies(md, e_local), dtype=np.float64)
    w_total = float(md.lib.jb_source_energy_total(e_gid.ctypes.data, int(md.mesh.nblocks)))
    if w_total > 0.0 and np.isfinite(w_total):
        _lib.check(md.lib.jb_comb_census_plan_global(md.pkg.ctx, md.handle, C.byref(md.sv), w_total, N, band, S,
                                                     int(md.cycle), C.byref(plan)))
    md._comb_sorted = bool(plan.sorted)
    changed_here = int(plan.cells_thinned) + int(plan.cells_split)
    new_ids = np.zeros(md.nranks, dtype=np.int64)
    new_ids[md.rank] = int(plan.n_new_ids)
    changed = np.zeros(md.nranks, dtype=np.int64)
    changed[md.rank] = changed_here
    if md.comm is not None and md.nranks > 1:
        both = md.comm.allreduce_sum_int64(np.concatenate([new_ids, changed]))
        new_ids, changed = both[:md.nranks], both[md.nranks:]
    rec = None
    id_base = md.next_id + int(new_ids[:md.rank].sum())
    if changed_here > 0:
        rep = _lib.CombReport()
        _lib.check(md.lib.jb_comb_census_apply(md.pkg.ctx, md.handle, C.byref(md.sv), id_base, C.byref(rep)))
        rec = dict(n_after=int(rep.n_after), n_new_ids=int(rep.n_new_ids), e_after=float(rep.e_after))
    elif int(changed.sum()) > 0:   # (another rank's swarm changed: the cycle is on record here too)
        rec = dict(n_after=int(plan.n_after), n_new_ids=0, e_after=float(plan.e_before))
    md.next_id += int(new_ids.sum())
    if rec is not None:
        # (n_eff = (sum w)^2 / sum w^2 is left out: the plan forms no sum of squared weights)
        rec.update(mode="global", cycle=md.cycle, n_before=int(plan.n_before), id_base=id_base,
                   cells_combed=changed_here, cells_thinned=int(plan.cells_thinned), cells_split=int(plan.cells_split),
                   max_per_cell=int(plan.max_per_cell), max_target=int(plan.max_target),
                   e_before=float(plan.e_before), w_total=w_total, scale=float(N) / w_total)
        md.comb_history.append(rec)
    return rec


def EstimateTimestepMesh(md: MeshData) -> float:
    """reference jaybenne.cpp:271-275"""
    return float(md.lib.jb_estimate_timestep(md.pkg.ctx))


def InitializeRadiation(md: MeshData, is_thermal: bool) -> None:
    """reference jaybenne.cpp:570-578 (called per block by mcblock's ProblemGenerator)"""
    if is_thermal:
        SourcePhotons(md, SourceType.thermal, 0.0, 0.0, per_block=True)
    EvaluateRadiationEnergy(md)


# ------------------------------------------------------------------------------------------------
def _exchange(md: MeshData, first: int, last: int):
    """MeshResetCommunication -> MeshSend -> MeshReceive (reference jaybenne.cpp:26-61) for the
    particles among [first, last) whose destination block lives on another rank.  Returns
    (number received, number handed over anywhere on the node).

    Per call: one count kernel + read-back, one all-gather of the rank x rank count matrix (which
    also answers the completion question), and -- only if anything moved -- one pack kernel, one
    all-to-all-v of 104-byte records and one unpack kernel.  Departed particles stay behind as
    holes until the swarm is compacted."""
    lib, ctx = md.lib, md.pkg.ctx
    if md.handoff != "python":
        # the library's one C call (jb_exchange; jaybenne_amd/handoff.py): the default
        md.ensure_handoff()
        t_c = time.perf_counter()
        out = md._chandoff.exchange(first, last)
        md.collective_seconds += time.perf_counter() - t_c   # (the whole call: the collectives are inside it)
        return out
    md._sync_stream()
    counts = np.zeros(md.nranks, dtype=np.int64)
    if md.records is None:
        md.records = torch.empty((max(4096, (last - first) // 16), _lib.JB_RECORD_WORDS),
                                 dtype=torch.int64, device=md.device)
    st = lib.jb_pack_outgoing(ctx, md.handle, C.byref(md.sv), first, last, md.nranks,
                              md.records.data_ptr(), md.records.shape[0], counts.ctypes.data)
    if st == _lib.JB_ERR_CAPACITY:      # counts are filled in before the capacity check: grow once
        md.records = torch.empty((int(counts.sum() * 1.5) + 4096, _lib.JB_RECORD_WORDS),
                                 dtype=torch.int64, device=md.device)
        st = lib.jb_pack_outgoing(ctx, md.handle, C.byref(md.sv), first, last, md.nranks,
                                  md.records.data_ptr(), md.records.shape[0], counts.ctypes.data)
    _lib.check(st)
    t_c = time.perf_counter()
    matrix = md.comm.gather_count_matrix(counts)
    md.collective_seconds += time.perf_counter() - t_c
    total = int(matrix.sum())
    if total == 0:
        return 0, 0
    nsend = int(counts.sum())
    md.handoff_records += nsend
    t_c = time.perf_counter()
    recv = md.comm.exchange_records(md.records[:nsend] if nsend else None, counts, md.device,
                                    recv_counts=matrix[:, md.rank].copy())
    md.collective_seconds += time.perf_counter() - t_c
    nrecv = 0 if recv is None else int(recv.shape[0])
    if nrecv:
        if md.n + nrecv > md.capacity:
            RemoveMarkedParticles(md)          # close the holes left by earlier departures
        md.reserve(md.n + nrecv)
        md._sync_stream()
        _lib.check(lib.jb_unpack_incoming(ctx, md.handle, C.byref(md.sv), recv.data_ptr(), nrecv))
    return nrecv, total


class _Range:
    """A trace range around a part of the task list (``jb_range_push`` / ``jb_range_pop``: ROCTx, shown by
    ``rocprofv3 --marker-trace``) -- the reference's ``Kokkos::Profiling::pushRegion("Jaybenne::Timestep")``
    and ``("Jaybenne::TransportLoop")``, jaybenne.cpp:87,115,127,145.  Does nothing without the marker library."""

    def __init__(self, md, name: str):
        self.lib, self.name = md.lib, name.encode()

    def __enter__(self):
        self.lib.jb_range_push(self.name)

    def __exit__(self, *exc):
        self.lib.jb_range_pop()
        return False


class _Phase:
    """Optional wall-clock accounting of the phases of RadiationStep (``md.phase_times = {}`` to
    switch it on; each phase then ends with a device synchronisation, so leave it off when
    measuring throughput)."""

    def __init__(self, md, name):
        self.md, self.name = md, name

    def __enter__(self):
        if self.md.phase_times is not None:
            torch.cuda.synchronize(self.md.device)
            self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        if self.md.phase_times is not None:
            torch.cuda.synchronize(self.md.device)
            self.md.phase_times[self.name] = (self.md.phase_times.get(self.name, 0.0)
                                              + time.perf_counter() - self.t0)
        return False


def RadiationStep(md: MeshData, t_start: float, dt: float) -> TaskStatus:
    """One radiation cycle: the task list of ``jaybenne::RadiationStep`` (reference
    jaybenne.cpp:68-151) for this rank's blocks.

    Single rank: one transport launch resolves every block crossing in flight.  Several ranks:
    the iterate-sublist of jaybenne.cpp:113-131 -- transport, hand-off of the particles that left
    for another rank's blocks, SampleDDMCBlockFace on the arrivals, and the global completion
    test (one all-reduced integer) -- repeated until no particle is in flight anywhere.
    """
    if md.handoff == "step" and not md.replicated:
        return _radiation_step_ranks(md, t_start, dt)   # (the library opens the reference's trace ranges itself)
    with _Range(md, "Jaybenne::Timestep"):          # jaybenne.cpp:87 ... :145
        return _radiation_step(md, t_start, dt)


def _radiation_step_ranks(md: MeshData, t_start: float, dt: float) -> TaskStatus:
    """JB_HANDOFF=step: the cycle of ``_radiation_step`` + ``_transport_loop`` as one library call,
    ``jb_radiation_step_ranks`` (include/jaybenne_amd.h) -- the same photons.  The hand-off runs through the
    transport of ``CHandoff.make(md, "auto")``; the swarm grows through ``md.reserve``."""
    pkg = md.pkg
    if md._rank_comm is None:
        transport = None
        if md.nranks > 1:
            md.ensure_handoff()
            transport = C.pointer(md._chandoff.tr)

        def reserve(_host, _swarm, n_slots):
            # (the library passes md.sv itself, which md.reserve updates in place)
            try:
                md.reserve(int(n_slots))
                return 0
            except Exception as e:   # noqa: BLE001 -- nothing may propagate through the C frames
                md._reserve_error = e
                return 1

        cb = _lib.RESERVE_FN(reserve)
        md._rank_comm = (_lib.RankComm(rank=md.rank, nranks=md.nranks, transport=transport, host=None, reserve=cb), cb)
    md._reserve_error = None
    ledger = md.ledger_enabled()
    if ledger:
        md._ledger_begin(t_start)
    if boundary_source_on(md):
        _set_boundary_source_count(md)
    md._sync_stream()
    next_id, cycle, rep = C.c_uint64(md.next_id), C.c_uint32(md.cycle), _lib.StepReport()
    st = md.lib.jb_radiation_step_ranks(pkg.ctx, md.handle, C.byref(md.sv), t_start, dt, C.byref(next_id),
                                        C.byref(cycle), md.prefix.data_ptr(), C.byref(md._rank_comm[0]),
                                        C.byref(rep))
    md.next_id, md.cycle = int(next_id.value), int(cycle.value)
    md._stats_cache = None       # (the counters moved inside the call)
    md.step_report = rep
    md.transport_iterations = int(rep.transport_iterations)
    md.transport_iterations_total += int(rep.transport_iterations)
    md.handoff_records += int(rep.sent)
    if st < 0:
        err = getattr(md._chandoff, "error", None) if md._chandoff is not None else None
        if err is not None:
            raise RuntimeError(f"hand-off transport failed: {err!r}")
        if md._reserve_error is not None and st == _lib.JB_ERR_CAPACITY:
            raise MemoryError(f"{md.lib.jb_last_error().decode()} ({md._reserve_error})")
        _lib.check(st)
    if st == _lib.JB_ITERATE:
        return TaskStatus.iterate
    md.events += int(rep.events)
    if boundary_source_on(md):     # (sourced inside the call, behind the emission source)
        last = _lib.BoundarySourceRecord()
        _lib.check(md.lib.jb_boundary_source_last(pkg.ctx, C.byref(last)))
        _record_boundary_source(md, dict(e_face=list(last.e_face), n_face=list(last.n_face)))
    if md.deposition == "exact":   # (closed inside the call, before UpdateFluid)
        md.deposit_history.append(dict(md.deposit_last(), cycle=md.cycle))
    if ledger:     # (closed and reduced over the ranks inside the call)
        led = _lib.EnergyLedger()
        _lib.check(md.lib.jb_ledger_last(pkg.ctx, C.byref(led)))
        md._ledger_record(led)
    _comb_and_defrag_after_step(md, int(rep.events))
    return TaskStatus.complete


def _transport_loop(md: MeshData, transport, use_ddmc: bool, t_start: float, dt: float) -> bool:
    """The iterate-sublist of jaybenne.cpp:113-131; False when max_transport_iterations passes did
    not finish it (TaskStatus.iterate)."""
    pkg = md.pkg
    first = 0
    md.transport_iterations = 0
    ledger = md.ledger_enabled()
    for it in range(int(pkg.Param("max_transport_iterations"))):
        last = md.n
        with _Phase(md, f"transport[{min(it, 2)}]"):
            transport(md, t_start, dt, first, last, fuse_census_tally=True)
            if ledger:   # exactly the range this launch followed, before the hand-off packs any of it
                _lib.check(md.lib.jb_ledger_accumulate(pkg.ctx, md.handle, C.byref(md.sv), first, last,
                                                       _lib.JB_LEDGER_TRANSPORTED))
        md.transport_iterations += 1
        md.transport_iterations_total += 1
        if (md.nranks == 1 or md.replicated) and not (md.force_exchange and md.comm is not None):
            return True
        with _Phase(md, "exchange"), _Range(md, "Jaybenne::MeshSendReceive"):
            # the hand-off clock starts when the transport launch has finished (its first device
            # read-back would otherwise be charged with the whole kernel)
            t_w = time.perf_counter()
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(md.device))
            done.synchronize()
            t_x = time.perf_counter()
            md.transport_wait_seconds += t_x - t_w
            nrecv, moved = _exchange(md, first, last)
            md.exchange_seconds += time.perf_counter() - t_x
        if moved == 0:
            return True
        first = md.n - nrecv        # the arrivals, appended at the end of the swarm
        if use_ddmc and nrecv:
            with _Phase(md, "block_face"):
                SampleDDMCBlockFace(md, first, md.n)
    return False


def _radiation_step(md: MeshData, t_start: float, dt: float) -> TaskStatus:
    pkg = md.pkg
    use_ddmc = bool(pkg.Param("use_ddmc"))
    transport = TransportPhotons_DDMC if use_ddmc else TransportPhotons
    ledger = md.ledger_enabled()
    if ledger:
        md._ledger_begin(t_start)
    md.cycle += 1
    with _Phase(md, "derived+source"):
        UpdateDerivedTransportFields(md, dt)
        n_before = md.n
        SourcePhotons(md, SourceType.emission, t_start, dt)
        SourceBoundaryPhotons(md, t_start, dt)
        if ledger and md.n > n_before:
            _lib.check(md.lib.jb_ledger_accumulate(pkg.ctx, md.handle, C.byref(md.sv), n_before, md.n,
                                                   _lib.JB_LEDGER_SOURCED))
        if md.replicated and md.rank != 0 and not pkg.Param("do_emission"):
            # Replicated mesh without the emission source: nothing resets energy_delta (sourcing.cpp:41-43
            # returns before :165-166 -- SURVEY App. C quirk 5), so behind last cycle's all-reduce EVERY rank
            # holds the global sum of all cycles so far.  One rank keeps carrying it; the others start the
            # cycle at zero and contribute their increment only -- the sum over ranks is then "everything so
            # far + this cycle's absorptions" once, not nranks times.
            md.fields["edelta"].zero_()
        # (the ddmc_face_prob ghost exchange of jaybenne.cpp:108-110 has no consumer: every face
        # the transport and resampling kernels read belongs to the block itself)
        md._sync_stream()
        _lib.check(md.lib.jb_zero_energy_tally(pkg.ctx, md.handle))
        # (the counters are cumulative: the previous step's closing read is this step's opening one,
        # one device synchronisation per step instead of two)
        before = md._stats_cache if md._stats_cache is not None else md.stats()
    with _Range(md, "Jaybenne::TransportLoop"):     # jaybenne.cpp:115 ... :127
        if not _transport_loop(md, transport, use_ddmc, t_start, dt):
            return TaskStatus.iterate
    with _Phase(md, "compaction+fluid"):
        after = md.stats()
        md._stats_cache = after
        if (md.nranks == 1 or md.replicated) and after["n_outgoing"] != before["n_outgoing"]:
            raise RuntimeError("particles left for another rank in a step that holds the whole mesh")
        # replicated mesh: the one exchange of the cycle -- census tally and absorbed / emitted energy
        # of all ranks' photons, summed on every rank (UpdateFluid then does the same on all of them)
        _sum_over_ranks(md, ("tally", "edelta"))
        if any(after[k] != before[k] for k in ("n_absorbed", "n_escaped", "n_outgoing")):
            RemoveMarkedParticles(md)
        md.events += after["n_events"] - before["n_events"]
        if md.deposition == "exact":     # energy_delta and the tally, each rounded once, before UpdateFluid reads them
            md.deposit_history.append(dict(md.deposit_close(), cycle=md.cycle))
        UpdateFluid(md)
        if ledger:
            led = _lib.EnergyLedger()
            _lib.check(md.lib.jb_ledger_close(pkg.ctx, md.handle, C.byref(md.sv), t_start, dt, C.byref(led)))
            led.cycle = md.cycle
            md._ledger_reduce(led)
            md._ledger_record(led)
        _comb_and_defrag_after_step(md, int(after["n_events"] - before["n_events"]))
    return TaskStatus.complete


def _comb_and_defrag_after_step(md: MeshData, events: int) -> None:
    """The end of a cycle: the census comb where it is on, then DefragParticles' schedule.  With the comb off this
    is ``_defrag_after_step`` and nothing else."""
    if md.comb_target <= 0 and md.census_total_target <= 0:
        _defrag_after_step(md, events)
        return
    if md.census_total_target > 0:
        CombCensusGlobal(md)
    else:
        CombCensus(md)
    _defrag_after_step(md, events, sorted_by_comb=md._comb_sorted)


def _defrag_after_step(md: MeshData, events: int, sorted_by_comb: bool = False) -> None:
    """DefragParticles at the end of a cycle: on the library's schedule (jb_defrag_policy) or every k-th cycle.
    ``sorted_by_comb``: the comb's plan has sorted the swarm in this cycle -- the k-th-cycle counter starts over;
    the library's schedule has started over inside the plan (jb_comb_census_plan) and is still called: it reads
    the cycle's kernel times and, one cycle behind a sort, never sorts."""
    pkg = md.pkg
    md._steps_since_defrag += 1
    if sorted_by_comb and md.defrag_interval >= 0:
        md._steps_since_defrag = 0
        return
    if md.defrag_interval < 0:
        sorted_ = C.c_int32(0)
        if md.nranks == 1:
            _lib.check(md.lib.jb_defrag_policy(pkg.ctx, md.handle, C.byref(md.sv), events, 0, C.byref(sorted_)))
        else:
            # the ranks sort together: a cycle is as long as its slowest rank (jaybenne_amd.h)
            _lib.check(md.lib.jb_defrag_policy(pkg.ctx, md.handle, C.byref(md.sv), events, 1, C.byref(sorted_)))
            if md.comm.allreduce_max_float(float(sorted_.value)) > 0.0:
                _lib.check(md.lib.jb_defrag_policy(pkg.ctx, md.handle, C.byref(md.sv), events, 2, C.byref(sorted_)))
            else:
                sorted_.value = 0
        if sorted_.value:
            md.defrags += 1
            md._steps_since_defrag = 0
    elif md.defrag_interval > 0 and md._steps_since_defrag >= md.defrag_interval:
        DefragParticles(md)
        md._steps_since_defrag = 0
