"""The one place the package's modules meet ctypes: the prototype of every
function declared in include/*.h, applied when its library is loaded, and the
device plumbing the tools share.

  DEVICE / HOST  name -> (restype, argtypes) of libmpc.so / libmpc_ingest.so
                 (tests/test_abi.py checks both against the headers)
  load           CDLL + the caller's ABI check + the table (engine.lib,
                 ingest._native: they keep the path, the build and the
                 HIP-runtime rules)
  host           libmpc_ingest.so or the caller's error
  host_check     a host call's return code, or the tool's error with its last_error
  error_text     the text of a failed libmpc.so call (engine._check, Device.check)
  h2d            a numpy array's bytes as a uint8 tensor on a GPU (engine.Batch, Device.put)
  Device         the scope of a call into libmpc.so on one GPU: torch, dev, lib,
                 stream, the H2D copies (put, put_all) and the check of its
                 return code

libmpc_synth.so has no public header: synth.py binds it.
"""
import ctypes
import warnings

import numpy as np

P = ctypes.POINTER
vp, cp, dbl, sz = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_double, ctypes.c_size_t
i32, u32, i64 = ctypes.c_int32, ctypes.c_uint32, ctypes.c_int64  # (int is 32 bits: ctypes.c_int is c_int32)
_LAST_ERROR = (cp, [])


def device_prototypes():
    """libmpc.so: mpc.h and the device halves of the five tool headers."""
    from .engine import PHASES, PlanInfo, _Input
    table = {
        "mpc_version": (i32, []), "mpc_build_flags": (i32, []), "mpc_last_error": _LAST_ERROR,
        "mpc_plan_create": (i32, [P(_Input), i64, P(vp)]),
        "mpc_plan_destroy": (i32, [vp]),
        "mpc_plan_parse_tables": (i32, [vp, vp, vp]),
        "mpc_plan_workspace_bytes": (i32, [vp, P(sz)]),
        "mpc_plan_bind": (i32, [vp, vp, sz]),
        "mpc_plan_buffer": (i32, [vp, i32, P(sz), P(i64)]),
        "mpc_plan_get_info": (i32, [vp, P(PlanInfo)]),
        "mpc_input_layout": (sz, [P(sz), i32]),
        "mpc_plan_set_input": (i32, [vp, P(_Input)]),
        "mpc_consensus": (i32, [vp, dbl, dbl, vp]),
        "mpc_run": (i32, [vp, dbl, dbl, vp]),
        "mpc_profile_kernel": (i32, [vp, i32, vp]),
        "mpc_verify_scan": (i32, [vp, vp, i32, vp, vp]),
        "mpc_coverage_run": (i32, [vp, vp, vp, vp, i64, vp, vp, i32, u32, vp, vp, vp, vp]),
        "mpc_coverage_tile_bytes": (i32, []),
        "mpc_linkage_run": (i32, [vp, vp, vp, vp, i64, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp]),
        "mpc_linkage_pairs": (i32, [vp, i64, i32, vp, vp, vp]),
        "mpc_linkage_tile_bytes": (i32, []),
        "mpc_linkage_scratch_bytes": (i64, [i64, i32]),
        "mpc_align_revcomp": (i32, [vp, i64, vp, i32, vp]),
        "mpc_align_trace": (i32, [vp, i64, vp, i32, vp, i64, vp, vp, i64, vp]),
        "mpc_align_cs_sizes": (i32, [vp, i32, i64, vp, vp, i64, vp, vp]),
        "mpc_align_cs_write": (i32, [vp, i64, vp, i32, vp, vp, i64, vp, vp, vp, i64, vp, i64, vp, i64, vp, vp]),
        "mpc_draft_vote": (i32, [vp, i64, vp, i32, vp, vp, i64, vp, i64, vp, vp]),
        "mpc_draft_call": (i32, [vp, vp, i64, vp, i64, vp, vp, vp]),
    }
    table.update(("mpc_" + phase, (i32, [vp, vp])) for phase in PHASES)
    return table


def host_prototypes():
    """libmpc_ingest.so: mpc_ingest.h and the host halves of the five tool headers."""
    from .coverage import _Paf
    from .ingest import _IngestOut
    from .pseudopair_reads import _Stats
    return {
        "mpc_ingest_version": (i32, []),
        "mpc_write_calls": (i32, [vp, i64, cp, cp, cp, i32, cp, i32]),
        "mpc_py_float_repr": (i32, [dbl, cp, i32]),
        "mpc_pseudopair": (i32, [cp, i64, i32, cp, i32, P(_Stats)]),
        "mpc_ingest": (i32, [cp, cp, cp, i32, P(_IngestOut)]),
        "mpc_ingest_multi": (i32, [i32, P(cp), P(cp), cp, i32, P(_IngestOut)]),
        "mpc_ingest_free": (None, [P(_IngestOut)]),
        "mpc_verify_scan_host": (i32, [vp, vp, i32, vp, i32]),
        "mpc_verify_script": (i32, [cp, i64, cp, i64, i32, i32, P(i32), P(i32), cp, sz]),
        "mpc_verify_last_error": _LAST_ERROR,
        "mpc_coverage_host": (i32, [vp, vp, vp, vp, i64, vp, vp, i32, u32, vp, vp, vp, i32, vp]),
        "mpc_coverage_ingest": (i32, [cp, i32, i32, P(_Paf)]),
        "mpc_coverage_ingest_free": (None, [P(_Paf)]),
        "mpc_coverage_last_error": _LAST_ERROR,
        "mpc_linkage_host": (i32, [vp, vp, vp, vp, i64, vp, i32, vp, vp, i32, vp, vp, vp, i32]),
        "mpc_linkage_pairs_host": (i32, [vp, i64, i32, vp, i32]),
        "mpc_linkage_last_error": _LAST_ERROR,
        "mpc_align_revcomp_host": (i32, [vp, i64, vp, i32, i32]),
        "mpc_align_plan": (i32, [vp, vp, i32, dbl, i64, vp, vp, P(i32)]),
        "mpc_align_trace_host": (i32, [vp, i64, vp, i32, vp, vp, i64, i32]),
        "mpc_align_render": (i32, [vp, i64, vp, i32, vp, vp, vp, i64, vp, vp, cp, vp, i64, vp, P(i64), i32]),
        "mpc_align_cs_sizes_host": (i32, [vp, i32, i64, vp, vp, i64, vp, i32]),
        "mpc_align_cs_write_host": (i32, [vp, i64, vp, i32, vp, vp, i64, vp, vp, vp, i64, vp, i64, vp, i64, i32]),
        "mpc_align_last_error": _LAST_ERROR,
        "mpc_draft_vote_host": (i32, [vp, i64, vp, i32, vp, vp, i64, vp, i64, vp, i32]),
        "mpc_draft_call_host": (i32, [vp, vp, i64, vp, i64, vp]),
        "mpc_draft_last_error": _LAST_ERROR,
    }


def load(path, prototypes, check):
    """CDLL(path) with prototypes() applied.  check(L) runs first (the caller's
    ABI test, on the default int restype): a stale library fails with its
    message, not on a symbol it lacks."""
    L = ctypes.CDLL(path)
    check(L)
    for name, (restype, argtypes) in prototypes().items():
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    return L


def host(err):
    """libmpc_ingest.so (built when stale); without it and without a compiler, err."""
    from . import ingest
    L = ingest._native()
    if L is None:
        raise err("libmpc_ingest.so is missing and cannot be built (no host compiler)")
    return L


def host_check(L, tool, err, rc, accept=()):
    """rc of a host call of ``tool`` when it is 0 or in ``accept``; else err with
    the text of mpc_<tool>_last_error."""
    if rc != 0 and rc not in accept:
        raise err(getattr(L, "mpc_{}_last_error".format(tool))().decode(errors="replace"))
    return rc


def error_text(L, rc):
    return f"libmpc error {rc}: {L.mpc_last_error().decode(errors='replace')}"


def h2d(torch, dev, a, pad=0, floor=0):
    """The bytes of a numpy array as a uint8 tensor on ``dev``, ``pad`` zeroed
    bytes behind them, at least ``floor`` bytes in all: one H2D copy."""
    a = np.ascontiguousarray(a)
    size = max(a.nbytes + pad, floor)
    d = torch.empty(size, dtype=torch.uint8, device=dev)
    if a.nbytes:
        # (read-only views of the ingest's buffers are only read here: the
        # host tensor is the source of one H2D copy, never written)
        with warnings.catch_warnings():
            warnings.filterwarnings("ignore", message="The given NumPy array is not writable")
            h = torch.from_numpy(a.reshape(-1).view(np.uint8))
        (d[: a.nbytes] if size > a.nbytes else d).copy_(h)
    if pad:
        d[a.nbytes:].zero_()
    return d


class Device:
    """A call into libmpc.so on GPU ``device``: torch, dev, lib and, once
    entered (torch.cuda.device(dev)), stream: the current stream as the C-ABI
    takes it.  libmpc.so is loaded before torch is imported: one HIP runtime in
    the process."""

    def __init__(self, device, cpu_path="host path"):
        from . import engine
        self.lib = engine.lib()
        import torch
        if not torch.cuda.is_available():
            raise engine.MpcError("no HIP device visible (use device='cpu' for the {})".format(cpu_path))
        self.torch, self.dev, self._error = torch, torch.device("cuda", int(device)), engine.MpcError

    def __enter__(self):
        self._guard = self.torch.cuda.device(self.dev)
        self._guard.__enter__()
        self.stream = vp(self.torch.cuda.current_stream(self.dev).cuda_stream)
        return self

    def __exit__(self, *exc):
        return self._guard.__exit__(*exc)

    def put(self, a):
        """The bytes of a numpy array as a uint8 tensor on the device."""
        return h2d(self.torch, self.dev, a)

    def put_all(self, parts):
        """Device pointers of the numpy arrays ``parts``, and the tensor that owns
        them: one blob, one H2D copy (int64 tables first keeps them 8-byte
        aligned), 8 spare bytes behind the last part."""
        parts = list(parts) + [np.zeros(8, np.uint8)]
        offs = np.cumsum([0] + [p.nbytes for p in parts])
        d_blob = self.put(np.concatenate([p.view(np.uint8).reshape(-1) for p in parts]))
        return [d_blob.data_ptr() + int(o) for o in offs[:-2]], d_blob

    def check(self, rc, accept=(), refused=None):
        """rc when it is 0 or in ``accept``.  -1 (MPC_E_ARG: the tables were
        refused before any launch) raises ``refused``, when given, with the text
        of mpc_last_error; every other code raises MpcError."""
        if rc == 0 or rc in accept:
            return rc
        if refused is not None and rc == -1:
            raise refused(self.lib.mpc_last_error().decode(errors="replace"))
        raise self._error(error_text(self.lib, rc))
