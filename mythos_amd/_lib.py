"""ctypes binding of libmythos_hip.so (the C ABI declared in include/mythos_hip.h).

There is no CPU fallback: if the shared library is missing, or a compute entry point is
called without a visible GPU, the call raises.  Building: ``python -c "import
__graft_entry__ as g; g.build()"`` or ``make -C mythos_amd/csrc``.
"""

from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import torch

_LIB_PATH = Path(__file__).resolve().parent / "lib" / "libmythos_hip.so"

c_int_p = C.POINTER(C.c_int32)
c_double_p = C.POINTER(C.c_double)
c_uint8_p = C.POINTER(C.c_uint8)


class MythosHipError(RuntimeError):
    """An error reported by libmythos_hip.so."""


_lib = None

V = C.c_void_p
# every prototype of include/mythos_hip.h: name -> (restype, argtypes)
_SIGS = {
    "mythos_version": (C.c_char_p, []),
    "mythos_last_error": (C.c_char_p, []),
    "mythos_device_count": (C.c_int, []),
    "mythos_debug_set": (C.c_int, [C.c_int, C.c_int64]),
    "mythos_debug_get": (C.c_int64, [C.c_int]),
    "mythos_oxdna_param_count": (C.c_int, []),
    "mythos_oxdna_param_name": (C.c_char_p, [C.c_int]),
    "mythos_oxdna_create": (V, [C.c_int, C.c_int, c_int_p, c_uint8_p, C.c_int, c_int_p, c_double_p, C.c_int, C.c_int]),
    "mythos_oxdna_destroy": (None, [V]),
    "mythos_oxdna_set_params": (C.c_int, [V, c_double_p, C.c_int]),
    "mythos_oxdna_set_pseq": (C.c_int, [V, c_double_p, c_int_p, C.c_int, c_double_p, C.c_int]),
    "mythos_oxdna_set_nucleotide_types": (C.c_int, [V, c_uint8_p]),
    "mythos_oxdna_set_neighbors": (C.c_int, [V, c_int_p, C.c_int]),
    "mythos_oxdna_build_neighbors": (C.c_int, [V, V, C.c_double, C.c_double, V]),
    "mythos_oxdna_neighbor_stats": (C.c_int, [V, C.POINTER(C.c_int), c_double_p]),
    "mythos_oxdna_get_rows": (C.c_int, [V, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int)]),
    "mythos_oxdna_energy": (C.c_int, [V, V, V, C.c_int, V, V, V, V, V]),
    "mythos_oxdna_energy_obs": (C.c_int, [V, V, V, C.c_int, V, V, V, V, V, V, V]),
    "mythos_oxdna_energy_dpseq": (C.c_int, [V, V, V, C.c_int, V, V, V, V, V, V, V]),
    "mythos_oxdna_debye_sweep": (C.c_int, [V, V, V, C.c_int, C.c_int, c_double_p, V, V, V]),
    "mythos_oxdna_order_params": (C.c_int, [V, V, V, C.c_int, C.c_int, c_int_p, c_int_p, c_int_p, C.c_int, C.c_double, V, V, V, V]),
    "mythos_observables_create": (V, [C.c_int, C.c_int, c_double_p, c_double_p, C.c_int, c_int_p, C.c_int, c_int_p, C.c_int, C.c_int, C.c_int]),
    "mythos_observables_destroy": (None, [V]),
    "mythos_observables_width": (C.c_int, [V]),
    "mythos_observables_eval": (C.c_int, [V, V, V, C.c_int, V, V]),
    "mythos_langevin_create": (V, [V, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, c_double_p, C.c_uint64]),
    "mythos_langevin_destroy": (None, [V]),
    "mythos_langevin_set_neighbor_policy": (C.c_int, [V, C.c_double, C.c_double, C.c_int]),
    "mythos_langevin_init_momenta": (C.c_int, [V, V, V, V]),
    "mythos_langevin_run": (C.c_int, [V, V, V, V, V, C.c_int, C.c_int, V, V, V, V]),
    "mythos_langevin_load": (C.c_int, [V, V, V, V, V, V]),
    "mythos_langevin_advance": (C.c_int, [V, C.c_int, C.c_int, V, V, V, V]),
    "mythos_langevin_store": (C.c_int, [V, V, V, V, V, V]),
    "mythos_langevin_get_step": (C.c_int64, [V]),
    "mythos_langevin_set_step": (C.c_int, [V, C.c_int64]),
    "mythos_langevin_set_seed": (C.c_int, [V, C.c_uint64]),
    "mythos_langevin_set_external_forces": (C.c_int, [V, C.c_int, c_int_p, c_double_p]),
    "mythos_langevin_set_restraints": (C.c_int, [V, C.c_int, c_int_p, c_double_p, c_double_p, c_int_p, C.c_int, c_int_p, c_int_p, c_int_p,
                                                 c_double_p, c_double_p, c_int_p]),
    "mythos_langevin_eval_external": (C.c_int, [V, V, V, V, V]),
    "mythos_langevin_set_point_forces": (C.c_int, [V, C.c_int, c_int_p, c_int_p, c_int_p, c_int_p, c_double_p]),
    "mythos_point_forces_check": (C.c_int, [C.c_int, C.c_int, C.c_int, c_int_p, c_int_p, c_int_p, c_int_p, c_double_p]),
    "mythos_langevin_eval_external_at": (C.c_int, [V, V, C.c_double, V, V, V]),
    "mythos_langevin_last_kernel_ms": (C.c_int, [V, c_double_p, c_double_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mythos_langevin_set_option": (C.c_int, [V, C.c_int, C.c_int64]),
    "mythos_langevin_set_timing": (C.c_int, [V, C.c_int]),
    "mythos_martini_langevin_set_timing": (C.c_int, [V, C.c_int]),
    "mythos_langevin_last_recoveries": (C.c_int, [V, C.POINTER(C.c_int)]),
    "mythos_langevin_last_rebuilds": (C.c_int, [V, C.POINTER(C.c_int)]),
    "mythos_umbrella_check": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, c_int_p, C.c_int, c_int_p, c_int_p, c_int_p, C.c_int, c_int_p,
                                        c_double_p, c_int_p, c_double_p, C.c_int]),
    "mythos_langevin_set_umbrella": (C.c_int, [V, C.c_int, C.c_int, c_int_p, c_int_p, c_int_p, C.c_int, c_int_p, c_double_p, c_int_p,
                                               c_double_p, C.c_double, C.c_int]),
    "mythos_langevin_advance_umbrella": (C.c_int, [V, C.c_int, C.c_int, V, V, V, V, V, V]),
    "mythos_langevin_umbrella_counts": (C.c_int, [V, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mythos_oxdna_read_trajectory": (C.c_int, [C.c_char_p, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p, C.POINTER(C.c_int)]),
    "mythos_oxdna_write_trajectory": (C.c_int, [C.c_char_p, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p, C.c_int]),
    "mythos_martini_create": (
        V,
        [C.c_int, c_int_p, C.c_int, c_double_p, c_double_p, C.c_int, c_int_p, c_double_p, c_double_p, C.c_int,
         c_int_p, c_double_p, c_double_p, C.c_int, C.c_double, C.c_int, C.c_int],
    ),
    "mythos_martini_destroy": (None, [V]),
    "mythos_martini_set_params": (C.c_int, [V, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    "mythos_martini_energy": (C.c_int, [V, V, V, C.c_int, V, V, V]),
    "mythos_martini_param_grads": (C.c_int, [V, V, V, C.c_int, V, V, V, V, V, V, V]),
    "mythos_martini_set_charges": (C.c_int, [V, c_double_p, C.c_double, C.c_double]),
    "mythos_martini_coulomb": (C.c_int, [V, V, V, C.c_int, V, V, V]),
    "mythos_martini_langevin_create": (V, [V, C.c_double, C.c_double, C.c_double, c_double_p, C.c_uint64]),
    "mythos_martini_langevin_destroy": (None, [V]),
    "mythos_martini_langevin_set_neighbor_policy": (C.c_int, [V, C.c_double, C.c_int]),
    "mythos_martini_langevin_set_inner_list": (C.c_int, [V, C.c_double, C.c_int]),
    "mythos_martini_langevin_init_velocities": (C.c_int, [V, V, V]),
    "mythos_martini_langevin_run": (C.c_int, [V, V, V, c_double_p, C.c_int, C.c_int, V, V, V]),
    "mythos_martini_langevin_load": (C.c_int, [V, V, V, c_double_p, V]),
    "mythos_martini_langevin_advance": (C.c_int, [V, C.c_int, C.c_int, V, V, V]),
    "mythos_martini_langevin_store": (C.c_int, [V, V, V, V]),
    "mythos_martini_langevin_get_step": (C.c_int64, [V]),
    "mythos_martini_langevin_last_rebuilds": (C.c_int, [V, C.POINTER(C.c_int)]),
    "mythos_martini_langevin_last_kernel_ms": (C.c_int, [V, c_double_p, c_double_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mythos_martini_langevin_last_recoveries": (C.c_int, [V, C.POINTER(C.c_int)]),
    "mythos_martini_langevin_neighbor_stats": (C.c_int, [V, C.POINTER(C.c_int), c_double_p]),
    "mythos_martini_langevin_get_rows": (C.c_int, [V, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int)]),
    "mythos_martini_langevin_set_barostat": (C.c_int, [V, C.c_int, C.c_int, c_double_p, c_double_p, C.c_double, C.c_int]),
    "mythos_martini_langevin_pressure": (C.c_int, [V, c_double_p, V]),
    "mythos_martini_langevin_get_box": (C.c_int, [V, c_double_p]),
    "mythos_martini_langevin_last_boxes": (C.c_int, [V, c_double_p, C.POINTER(C.c_int)]),
    "mythos_martini_langevin_create_ensemble": (V, [V, C.c_int, C.c_double, c_double_p, C.c_double, c_double_p, C.POINTER(C.c_uint64)]),
    "mythos_martini_ensemble_check": (C.c_int, [C.c_int, C.c_int, c_double_p, C.c_double, C.c_double, c_double_p]),
    "mythos_martini_langevin_n_replicas": (C.c_int, [V]),
    "mythos_martini_langevin_restart": (C.c_int, [V, C.POINTER(C.c_uint64), C.c_int64]),
    "mythos_martini_langevin_pressure_ensemble": (C.c_int, [V, c_double_p, V]),
    "mythos_martini_langevin_get_box_ensemble": (C.c_int, [V, c_double_p]),
    "mythos_martini_langevin_set_exchange": (C.c_int, [V, C.c_int, C.c_uint64]),
    "mythos_martini_langevin_set_ladder": (C.c_int, [V, C.POINTER(C.c_int32)]),
    "mythos_martini_langevin_get_ladder": (C.c_int, [V, C.POINTER(C.c_int32)]),
    "mythos_martini_langevin_last_ladder": (C.c_int, [V, C.POINTER(C.c_int32), C.POINTER(C.c_int)]),
    "mythos_martini_langevin_last_exchanges": (C.c_int, [V, c_double_p, C.POINTER(C.c_int)]),
    "mythos_martini_langevin_exchange_counts": (C.c_int, [V, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mythos_martini_exchange_check": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    "mythos_martini_window_exchange_check": (C.c_int, [C.c_int, C.c_int, c_double_p, C.c_int, C.c_int, C.c_int, c_double_p, C.POINTER(C.c_int32)]),
    "mythos_martini_langevin_set_window_exchange": (C.c_int, [V, C.c_int, C.c_uint64]),
    "mythos_martini_langevin_set_windows": (C.c_int, [V, C.POINTER(C.c_int32)]),
    "mythos_martini_langevin_get_windows": (C.c_int, [V, C.POINTER(C.c_int32)]),
    "mythos_martini_langevin_last_windows": (C.c_int, [V, C.POINTER(C.c_int32), C.POINTER(C.c_int)]),
    "mythos_martini_langevin_last_window_exchanges": (C.c_int, [V, c_double_p, C.POINTER(C.c_int)]),
    "mythos_martini_langevin_window_exchange_counts": (C.c_int, [V, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mythos_martini_restraints_check": (C.c_int, [C.c_int, C.c_int, C.c_int, c_int_p, c_double_p, c_double_p, C.c_int, c_int_p, c_int_p,
                                                  c_double_p, C.c_int, c_int_p, c_int_p, c_int_p, C.c_int, c_int_p, c_int_p, c_double_p,
                                                  c_double_p, C.c_int, C.c_int]),
    "mythos_martini_langevin_set_restraints": (C.c_int, [V, C.c_int, c_int_p, c_double_p, c_double_p, C.c_int, c_int_p, c_int_p, c_double_p,
                                                         C.c_int, c_int_p, c_int_p, c_int_p, C.c_int, c_int_p, c_int_p, c_double_p, c_double_p]),
    "mythos_martini_langevin_n_pull": (C.c_int, [V]),
    "mythos_martini_langevin_eval_external": (C.c_int, [V, V, C.c_double, V, V, V, V]),
    "mythos_martini_langevin_pull_values": (C.c_int, [V, V, C.c_int, V, V]),
    "mythos_martini_obs_create": (V, [C.c_int, C.c_int, c_int_p, c_int_p, c_int_p, C.c_int]),
    "mythos_martini_obs_destroy": (None, [V]),
    "mythos_martini_obs_count": (C.c_int64, [V]),
    "mythos_martini_obs_eval": (C.c_int, [V, V, V, C.c_int, C.c_int, V, V]),
    "mythos_w1_plan_create": (V, [C.c_int, c_int_p, c_int_p, V, C.POINTER(C.c_int64), V, V, c_uint8_p, V, C.c_int, V]),
    "mythos_w1_plan_destroy": (None, [V]),
    "mythos_w1_eval": (C.c_int, [V, V, V, V, V]),
    "mythos_membrane_create": (V, [C.c_int, C.c_int, c_int_p, c_int_p, C.c_int, c_int_p, c_int_p, C.c_int]),
    "mythos_membrane_destroy": (None, [V]),
    "mythos_membrane_n_lipids": (C.c_int, [V]),
    "mythos_membrane_eval": (C.c_int, [V, V, V, C.c_int, C.c_int, V, V, V]),
    "mythos_duplex_obs_create": (V, [C.c_int, C.c_int, c_double_p, c_double_p, C.c_int, c_int_p, C.c_int, c_int_p, c_int_p, c_double_p, C.c_int]),
    "mythos_duplex_obs_destroy": (None, [V]),
    "mythos_duplex_obs_eval": (C.c_int, [V, V, V, C.c_int, C.c_int, V, V]),
    "mythos_rdf_create": (V, [C.c_int, C.c_int, c_int_p, c_int_p, c_int_p, c_int_p, C.c_int, C.c_double, C.c_int, C.c_int]),
    "mythos_rdf_destroy": (None, [V]),
    "mythos_rdf_n_pairs": (C.c_int, [V, C.POINTER(C.c_int64)]),
    "mythos_rdf_eval": (C.c_int, [V, V, V, C.c_int, C.c_int, V, V, V]),
    "mythos_martini_bar_per_kj_mol_nm3": (C.c_double, []),
    "mythos_martini_stress_profile_check": (C.c_int, [C.c_int, C.c_double, C.c_int, c_double_p, C.c_int, c_int_p, C.c_int]),
    "mythos_martini_stress_profile": (C.c_int, [V, V, V, C.c_int, C.c_int, c_int_p, C.c_int, C.c_int, V, V]),
    "mythos_mbar_check": (C.c_int, [C.c_int, C.c_int64, C.c_int, c_double_p, c_double_p, C.POINTER(C.c_int64), c_double_p, C.c_int, c_double_p]),
    "mythos_mbar_create": (V, [C.c_int64, C.c_int, C.c_int]),
    "mythos_mbar_destroy": (None, [V]),
    "mythos_mbar_set_windows": (C.c_int, [V, C.c_int, c_double_p, c_double_p, C.POINTER(C.c_int64), V]),
    "mythos_mbar_set_matrix": (C.c_int, [V, V, C.POINTER(C.c_int64)]),
    "mythos_mbar_iterate": (C.c_int, [V, V, C.c_int, V, V]),
    "mythos_mbar_log_weights": (C.c_int, [V, V, V, V]),
    "mythos_mbar_binned_sum": (C.c_int, [V, C.c_int, V, V, V, V, C.c_double, V, V]),
    "mythos_mbar_gram": (C.c_int, [V, V, V, V, V]),
    "mythos_mbar_segment_moments": (C.c_int, [V, V, C.c_int, V, V, V, V, V]),
    "mythos_mbar_boot_colsums": (C.c_int, [V, V, C.c_int, V, V, V, V]),
    "mythos_mbar_boot_binned": (C.c_int, [V, V, C.c_int, V, V, C.c_int, V, V, C.c_int, V, C.c_double, V, V]),
    "mythos_timeseries_check": (C.c_int, [C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64), c_double_p]),
    "mythos_timeseries_moments": (C.c_int, [V, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64), V, V, V, C.c_int, V]),
    "mythos_timeseries_autocorr": (C.c_int, [V, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64), V, V, V, C.c_int64, C.c_int, V, C.c_int, V]),
}


def lib_path() -> Path:
    return Path(os.environ.get("MYTHOS_HIP_LIB", _LIB_PATH))


def load() -> C.CDLL:
    """Load the library once and declare every prototype of include/mythos_hip.h."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not path.exists():
        raise MythosHipError(
            f"{path} not found: the HIP extension is not built (run __graft_entry__.build()). "
            "mythos_amd has no CPU fallback."
        )
    lib = C.CDLL(str(path))
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)  # AttributeError here = header / library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


DECLARED_SYMBOLS = tuple(_SIGS)


MEMBRANE_ROW = 7  # MYTHOS_MEMBRANE_ROW of include/mythos_hip.h: doubles per frame of mythos_membrane_eval
STRESS_ROW, STRESS_ROW_BY_TERM = 4, 13  # MYTHOS_STRESS_ROW, MYTHOS_STRESS_ROW_BY_TERM: doubles per slab of mythos_martini_stress_profile
STRESS_MAX_BINS = 1024  # kStressMaxBins of csrc/stress_profile_checks.h


def last_error() -> str:
    return load().mythos_last_error().decode()


def check(rc: int, what: str = "") -> None:
    """Raise on a negative mythos_status (error conventions of SURVEY.md section 8b)."""
    if rc == 0:
        return
    msg = f"{what}: {last_error()} (status {rc})"
    if rc == -1:
        raise ValueError(msg)
    if rc == -6:
        raise FloatingPointError(msg)
    raise MythosHipError(msg)


# keys of mythos_debug_set (include/mythos_hip.h: enum mythos_debug_key) - test and diagnostic switches
DEBUG_KEYS = {"cell_bucket_cap": 0, "energy_list_cap": 1, "md_segment": 2, "md_overflow_at": 3, "md_dense": 4, "md_items_big": 5, "md_lanes": 6,
              "rows_filter": 7, "rows_cand_every": 8, "rows_cand_margin": 9}  # (rows_filter alone defaults to 1)


def debug_set(key: str, value: int) -> None:
    """Process-wide test / diagnostic switch of the library; 0 restores the default (rows_filter: 1 does)."""
    check(load().mythos_debug_set(DEBUG_KEYS[key], int(value)), f"debug_set({key})")


def debug_get(key: str) -> int:
    return int(load().mythos_debug_get(DEBUG_KEYS[key]))


_PARAM_NAMES: list[str] = []


def param_names() -> list[str]:
    """Names of the flat parameter vector, in its order (a property of the library: read once)."""
    if not _PARAM_NAMES:
        lib = load()
        _PARAM_NAMES.extend(lib.mythos_oxdna_param_name(i).decode() for i in range(lib.mythos_oxdna_param_count()))
    return list(_PARAM_NAMES)


def device_count() -> int:
    return int(load().mythos_device_count())


def ptr(t):
    """Device (or host) data pointer of a torch tensor / numpy array as c_void_p (None -> NULL)."""
    if t is None:
        return None
    if hasattr(t, "data_ptr"):
        return C.c_void_p(t.data_ptr())
    return C.c_void_p(t.ctypes.data)


def stream(device) -> C.c_void_p:
    """torch's current stream on ``device`` as the ABI's mythos_stream_t."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def dtype_code(dtype: torch.dtype) -> int:
    """MYTHOS_F32 / MYTHOS_F64 of include/mythos_hip.h."""
    if dtype == torch.float32:
        return 0
    if dtype == torch.float64:
        return 1
    raise ValueError(f"unsupported dtype {dtype}: use torch.float32 or torch.float64")


class Handle:
    """Owner of one handle of the C ABI: ``self._h`` from the named create function (NULL raises with the library's
    message), given back through the function the subclass names in ``_destroy`` by ``close()`` - any number of times -
    or when the object goes."""

    _destroy = ""
    _h = None

    def __init__(self, create: str, *args):
        self._lib = load()
        self._h = getattr(self._lib, create)(*args)
        if not self._h:
            raise MythosHipError(f"{create}: {last_error()}")

    def close(self) -> None:
        h, self._h = self._h, None
        if h:
            getattr(self._lib, self._destroy)(h)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


def per_device(owner, key, make):
    """``make()`` once per ``key`` - the device alone, or (n, dtype, device) where an object serves trajectories of several
    sizes - for ``owner`` (an observable object, frozen dataclasses included), kept in its ``_sets``."""
    sets = owner.__dict__.setdefault("_sets", {})
    key = str(key)
    if key not in sets:
        sets[key] = make()
    return sets[key]
