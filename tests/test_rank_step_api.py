"""jb_radiation_step_ranks (include/jaybenne_amd.h) without a GPU: the library exports it, the Python binding
matches the header, it refuses null or inconsistent arguments before it touches a device or a collective,
and the C++ mirror's multi-rank RadiationStep compiles against the headers."""
import ctypes
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_multi_rank_step_and_the_binding_matches():
    from jaybenne_amd import _lib
    lib = _lib.load()
    fn = lib.jb_radiation_step_ranks
    res, args = _lib.PROTOTYPES["jb_radiation_step_ranks"]
    assert fn.restype is res and list(fn.argtypes) == list(args)
    assert len(args) == 10
    assert args[2] is ctypes.POINTER(_lib.SwarmView)
    assert args[8] is ctypes.POINTER(_lib.RankComm) and args[9] is ctypes.POINTER(_lib.StepReport)


def test_rank_comm_and_step_report_layouts_match_the_header():
    from jaybenne_amd import _lib
    src = r'''
#include <stddef.h>
#include <stdio.h>
#include "jaybenne_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(jb_rank_comm), offsetof(jb_rank_comm, nranks),
         offsetof(jb_rank_comm, transport), offsetof(jb_rank_comm, host), offsetof(jb_rank_comm, reserve),
         sizeof(jb_step_report), offsetof(jb_step_report, transport_iterations),
         offsetof(jb_step_report, capacity_rounds), offsetof(jb_step_report, sent),
         offsetof(jb_step_report, received), offsetof(jb_step_report, events), sizeof(jb_exchange_transport));
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    R, S = _lib.RankComm, _lib.StepReport
    assert got == [ctypes.sizeof(R), R.nranks.offset, R.transport.offset, R.host.offset, R.reserve.offset,
                   ctypes.sizeof(S), S.transport_iterations.offset, S.capacity_rounds.offset, S.sent.offset,
                   S.received.offset, S.events.offset, ctypes.sizeof(_lib.ExchangeTransport)]


def _call(comm, ctx=None, mesh=None, swarm=True, next_id=True, cycle=True, report=None):
    from jaybenne_amd import _lib
    lib = _lib.load()
    sv = _lib.SwarmView(n=0, capacity=0)
    nid, cyc = ctypes.c_uint64(7), ctypes.c_uint32(3)
    st = lib.jb_radiation_step_ranks(ctx, mesh, ctypes.byref(sv) if swarm else None, 0.0, 1.0,
                                     ctypes.byref(nid) if next_id else None, ctypes.byref(cyc) if cycle else None,
                                     None, ctypes.byref(comm) if comm is not None else None,
                                     ctypes.byref(report) if report is not None else None)
    return st, lib.jb_last_error().decode(), nid.value, cyc.value


def test_invalid_arguments_are_refused_before_any_device_work():
    """Every verdict below comes before the call looks at a context or a device: JB_ERR_INVALID, a message
    that names the problem, next_id / cycle / report untouched."""
    from jaybenne_amd import _lib
    rep = _lib.StepReport(transport_iterations=-5)
    st, msg, nid, cyc = _call(None, report=rep)
    assert st == _lib.JB_ERR_INVALID and "null comm" in msg and (nid, cyc) == (7, 3)
    assert rep.transport_iterations == -5
    for rank, nranks in ((0, 0), (2, 2), (-1, 3)):
        st, msg, nid, cyc = _call(_lib.RankComm(rank=rank, nranks=nranks))
        assert st == _lib.JB_ERR_INVALID and "outside [0, nranks" in msg, msg
        assert (nid, cyc) == (7, 3)
    # several ranks without a transport (or with half of one)
    st, msg, _, _ = _call(_lib.RankComm(rank=0, nranks=2))
    assert st == _lib.JB_ERR_INVALID and "transport" in msg
    half = _lib.ExchangeTransport()
    half.all_gather_u64 = _lib.ALL_GATHER_FN(lambda *a: 0)
    st, msg, _, _ = _call(_lib.RankComm(rank=1, nranks=2, transport=ctypes.pointer(half)))
    assert st == _lib.JB_ERR_INVALID and "transport" in msg
    # one rank, no transport: a valid comm -- then the missing context / mesh / swarm / counters
    one = _lib.RankComm(rank=0, nranks=1)
    for kw in ({}, {"swarm": False}, {"next_id": False}, {"cycle": False}):
        st, msg, nid, cyc = _call(one, **kw)
        assert st == _lib.JB_ERR_INVALID and "null argument" in msg and (nid, cyc) == (7, 3)


def test_cpp_mirror_multi_rank_step_compiles():
    src = r'''
#include "jaybenne_amd.h"
#include "jaybenne_amd.hpp"
static int gather(void *, const uint64_t *, uint64_t *, int, void *) { return 0; }
static int a2a(void *, const int64_t *, const int64_t *, const int64_t *, int64_t *, const int64_t *,
               const int64_t *, int, void *) { return 0; }
jaybenne_amd::TaskStatus cycle(jaybenne_amd::MeshData *md, double t, double dt, int rank, int nranks) {
  jb_exchange_transport tr{nullptr, gather, a2a};
  const jaybenne_amd::TaskStatus st = jaybenne_amd::RadiationStep(md, t, dt, &tr, rank, nranks);
  const jb_step_report &r = md->last_step;
  (void)r.transport_iterations; (void)r.capacity_rounds; (void)r.sent; (void)r.received; (void)r.events;
  if (nranks == 1) return jaybenne_amd::RadiationStep(md, t, dt, nullptr, 0, 1);
  return st;
}
'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.cpp")
        open(c, "w").write(src)
        run = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I",
                              os.path.join(ROOT, "include"), c], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
