"""ctypes binding of libsitrk.so (include/sitrk.h).

The extension is built in-tree (sitrack_amd/csrc/Makefile -> sitrack_amd/libsitrk.so)
and loaded from there.  There is no CPU fallback: if the library is missing, or no
HIP device is usable, the product raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# the in-tree build; SITRK_LIB_PATH points A/B tooling at another build of the same sources
SO_PATH = os.environ.get("SITRK_LIB_PATH") or os.path.join(_HERE, "libsitrk.so")
CSRC = os.path.join(_HERE, "csrc")

SITRK_F32, SITRK_F64 = 0, 1
SAMPLE_AFTER, SAMPLE_ENTER = 0, 1            # SITRK_SAMPLE_*
SAMPLE_MAX_FIELDS = 8
_SAMPLE_MODES = {"after": SAMPLE_AFTER, "enter": SAMPLE_ENTER, SAMPLE_AFTER: SAMPLE_AFTER, SAMPLE_ENTER: SAMPLE_ENTER}
_SLOT_FIELDS = {"u": 0, "u_ice": 0, "v": 1, "v_ice": 1, "siconc": 2, "sic": 2, 0: 0, 1: 1, 2: 2}
FillValue = -9999.0
MESH_MAX = 8                                 # SITRK_MESH_MAX
MESH_NSTATS = 10                             # SITRK_MESH_NSTATS, in this order:
COARSE_MAXLEV = 16                           # SITRK_COARSE_MAXLEV
COARSE_NCOLS = 8                             # SITRK_COARSE_NCOLS, in this order:
COARSE_COLS = ("nboxes", "nfilled", "area", "area_div", "area_shr", "area_tot", "area_tot2", "area_tot3")
COARSE_VALUES = ("n", "A", "AUx", "AUy", "AVx", "AVy")     # the six values of a box
FEAT_NCOLS = 12                              # SITRK_FEAT_NCOLS, in this order:
FEAT_COLS = ("label", "npix", "jmin", "jmax", "imin", "imax", "sum_j", "sum_i", "sum_jj", "sum_ii", "sum_ji", "perimeter")
FEAT_WHAT = {"div": 0, "shr": 1, "vor": 2, "tot": 3}       # `what` of sitrk_mesh_features
LABEL_TILE = 64                              # SITRK_LABEL_TILE
KEEP_MAX = 16                                # SITRK_KEEP_MAX
MATCH_MAXREACH = 2                           # SITRK_MATCH_MAXREACH
MATCH_MAXSHIFT = 32768                       # |dj|, |di| of sitrk_features_match
SKEL_NCOLS = 7                               # SITRK_SKEL_NCOLS, in this order:
SKEL_COLS = ("label", "npix", "nskel", "nend", "njunc", "north", "ndiag")
SKEL_MAXSUB = 1 << 20                        # max_sub of the skeleton calls
PAIRS_MAXCLASS = 16                          # SITRK_PAIRS_MAXCLASS
PAIRS_NCOLS = 7                              # SITRK_PAIRS_NCOLS, in this order:
PAIRS_COLS = ("n", "sum_r0", "sum_e", "sum_abs_e", "sum_e2", "sum_abs_e3", "sum_d2")
DIST_MAXBINS = 1024                          # SITRK_DIST_MAXBINS
DIST_MAXQ = 16                               # SITRK_DIST_MAXQ
DIST_WHAT = {"div": 0, "shr": 1, "vor": 2, "tot": 3}       # `what` of sitrk_mesh_dist
MESH_STATS = ("n0", "n1", "n2", "area0", "area1", "area0_div", "area0_shr", "area0_tot", "area0_tot2", "area0_tot3")

_vp = C.c_void_p
_i64 = C.c_int64
_int = C.c_int
_dbl = C.c_double

# every symbol include/sitrk.h declares: (restype, argtypes)
_SIGNATURES = {
    "sitrk_version": (_int, []),
    "sitrk_create": (_int, [C.POINTER(_vp), _int]),
    "sitrk_destroy": (_int, [_vp]),
    "sitrk_last_error": (C.c_char_p, [_vp]),
    "sitrk_sync": (_int, [_vp]),
    "sitrk_set_stream": (_int, [_vp, _vp]),
    "sitrk_set_grid": (_int, [_vp, _int, _int] + [_vp] * 7),
    "sitrk_set_params": (_int, [_vp, _dbl, _int, _dbl]),
    "sitrk_set_substeps": (_int, [_vp, _int]),
    "sitrk_set_tuning": (_int, [_vp, C.c_char_p, _int]),
    "sitrk_alloc_records": (_int, [_vp, _int, _int]),
    "sitrk_push_record": (_int, [_vp, _int, _vp, _vp, _vp]),
    "sitrk_push_record_dev": (_int, [_vp, _int, _vp]),
    "sitrk_stage_acquire": (_int, [_vp, _int, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "sitrk_stage_submit": (_int, [_vp, _int, _int, _int]),
    "sitrk_stage_release": (_int, [_vp]),
    "sitrk_launch_stats": (_int, [_vp, _int, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    "sitrk_lane_stats": (_int, [_vp, _int, C.POINTER(_i64), C.POINTER(_i64)]),
    "sitrk_buoy_rows": (_int, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "sitrk_push_record_rows": (_int, [_vp, _int, _int, _int, _vp, _vp, _vp]),
    "sitrk_commit_record_rows": (_int, [_vp, _int, _int, _int]),
    "sitrk_buoy_box": (_int, [_vp] + [C.POINTER(C.c_int32)] * 4),
    "sitrk_push_record_box": (_int, [_vp, _int, _int, _int, _int, _int, _vp, _vp, _vp, _i64]),
    "sitrk_buoy_box_begin": (_int, [_vp]),
    "sitrk_buoy_box_end": (_int, [_vp] + [C.POINTER(C.c_int32)] * 5),
    "sitrk_stage_acquire_box": (_int, [_vp, _int, _int, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "sitrk_stage_submit_box": (_int, [_vp, _int, _int, _int, _int, _int]),
    "sitrk_commit_record_box": (_int, [_vp, _int, _int, _int, _int, _int]),
    "sitrk_commit_records_box": (_int, [_vp, _int, _int, _int, _int, _int, _int]),
    "sitrk_commit_records_box_async": (_int, [_vp, _int, _int, _int, _int, _int, _int]),
    "sitrk_record_ptr": (_vp, [_vp, _int]),
    "sitrk_commit_record": (_int, [_vp, _int]),
    "sitrk_set_buoys": (_int, [_vp, _i64, _vp, _vp, _vp, _vp]),
    "sitrk_restore_state": (_int, [_vp, _vp, _vp]),
    "sitrk_sort_buoys": (_int, [_vp]),
    "sitrk_set_resort": (_int, [_vp, _int]),
    "sitrk_step": (_int, [_vp, _int, _int]),
    "sitrk_run": (_int, [_vp, _int, _int, _int]),
    "sitrk_run_tlerp": (_int, [_vp, _int, _int, _int, _dbl, _int, _int]),
    "sitrk_fetch": (_int, [_vp, _vp, _vp, _vp, _vp]),
    "sitrk_fetch_record": (_int, [_vp, _int, _vp, _vp, _vp]),
    "sitrk_sample_slot": (_int, [_vp, _int, _int, _int, _int, _vp]),
    "sitrk_sample_fields": (_int, [_vp, _int, _int, _int, _int, _int, _int, _int, _int, C.POINTER(_vp), _i64, _vp]),
    "sitrk_deform_cells": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _int, _vp, _dbl, _vp, _vp, C.POINTER(_i64)]),
    "sitrk_deform_mark": (_int, [_vp, _int]),
    "sitrk_deform_since_mark": (_int, [_vp, _int, _i64, _int, _vp, _vp, _vp, C.POINTER(_i64)]),
    "sitrk_deform_kernel_ms": (_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sitrk_tri2quad": (_int, [_vp, _i64, _vp, _vp, _i64, _vp, _dbl, _dbl, _dbl, _dbl, _dbl, _i64, _vp, _vp, C.POINTER(_i64), C.POINTER(_int)]),
    "sitrk_tri2quad_buoys": (_int, [_vp, _i64, _vp, _dbl, _dbl, _dbl, _dbl, _dbl, _i64, _vp, _vp, C.POINTER(_i64), C.POINTER(_int)]),
    "sitrk_tri2quad_kernel_ms": (_int, [_vp] + [C.POINTER(C.c_float)] * 4),
    "sitrk_delaunay": (_int, [_vp, _i64, _vp, _vp, _dbl, _i64, _vp, C.POINTER(_i64), _vp]),
    "sitrk_delaunay_buoys": (_int, [_vp, _dbl, _i64, _vp, C.POINTER(_i64), _vp]),
    "sitrk_delaunay_kernel_ms": (_int, [_vp] + [C.POINTER(C.c_float)] * 3),
    "sitrk_delaunay_stats": (_int, [_vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "sitrk_mesh_build": (_int, [_vp, _int, _int, _dbl, _vp, _dbl, _dbl, _dbl, _dbl, _dbl, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_int)]),
    "sitrk_mesh_cells": (_int, [_vp, _int, _i64, _vp, C.POINTER(_i64)]),
    "sitrk_mesh_mark": (_int, [_vp, _int, _int]),
    "sitrk_mesh_deform": (_int, [_vp, _int, _int, _vp, _vp, _vp]),
    "sitrk_mesh_free": (_int, [_vp, _int]),
    "sitrk_mesh_kernel_ms": (_int, [_vp] + [C.POINTER(C.c_float)] * 4),
    "sitrk_raster_cells": (_int, [_vp, _i64, _vp, _i64, _int, _vp, _vp, _dbl, _dbl, _dbl, _int, _int, _vp, C.POINTER(_i64)]),
    "sitrk_mesh_raster": (_int, [_vp, _int, _int, _int, _dbl, _dbl, _dbl, _int, _int, _vp, _vp, C.POINTER(_i64)]),
    "sitrk_raster_kernel_ms": (_int, [_vp] + [C.POINTER(C.c_float)] * 2),
    "sitrk_raster_stats": (_int, [_vp, C.POINTER(_i64)]),
    "sitrk_coarse_cells": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _int, _vp, _vp, _dbl, _dbl, _dbl, _dbl, _int, _int, _int, _dbl,
                                  _vp, _vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "sitrk_mesh_coarse": (_int, [_vp, _int, _int, _dbl, _dbl, _dbl, _int, _int, _int, _dbl, _vp, _vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "sitrk_coarse_kernel_ms": (_int, [_vp] + [C.POINTER(C.c_float)] * 5),
    "sitrk_label_raster": (_int, [_vp, _int, _int, _vp, _int, _i64, _i64, _vp, _vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    "sitrk_mesh_features": (_int, [_vp, _int, _int, _int, _dbl, _dbl, _dbl, _int, _int, _int, _int, _dbl, _int, _i64, _i64, _vp, _vp,
                                   C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    "sitrk_features_kernel_ms": (_int, [_vp] + [C.POINTER(C.c_float)] * 3),
    "sitrk_mesh_features_keep": (_int, [_vp, _int, _int, _int, _int, _dbl, _dbl, _dbl, _int, _int, _int, _int, _dbl, _int, _i64, _i64, _vp, _vp,
                                        C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    "sitrk_keep_put": (_int, [_vp, _int, _int, _int, _vp, _int, _i64]),
    "sitrk_keep_get": (_int, [_vp, _int, C.POINTER(_int), C.POINTER(_int), C.POINTER(_int), C.POINTER(_i64), _vp]),
    "sitrk_keep_free": (_int, [_vp, _int]),
    "sitrk_mesh_features_advect": (_int, [_vp, _int, _int, _int, _int, _dbl, _dbl, _dbl, _int, _int, C.POINTER(_i64), C.POINTER(_i64)]),
    "sitrk_features_match": (_int, [_vp, _int, _int, _int, _int, _int, _i64, _vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "sitrk_match_kernel_ms": (_int, [_vp] + [C.POINTER(C.c_float)] * 3),
    "sitrk_advect_kernel_ms": (_int, [_vp, C.POINTER(C.c_float)]),
    "sitrk_skeleton_raster": (_int, [_vp, _int, _int, _vp, _int, _i64, _i64, _vp, _vp, _vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64),
                                     C.POINTER(_int), C.POINTER(_int)]),
    "sitrk_keep_skeleton": (_int, [_vp, _int, _int, _i64, _i64, _vp, _vp, _vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64),
                                   C.POINTER(_int), C.POINTER(_int)]),
    "sitrk_skeleton_kernel_ms": (_int, [_vp] + [C.POINTER(C.c_float)] * 3),
    "sitrk_pairs_points": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _int, _vp, _vp, C.POINTER(_i64)]),
    "sitrk_pairs_mark": (_int, [_vp, _int, _vp]),
    "sitrk_pairs_since_mark": (_int, [_vp, _int, _int, _vp, _vp, C.POINTER(_i64)]),
    "sitrk_pairs_free": (_int, [_vp]),
    "sitrk_pairs_kernel_ms": (_int, [_vp] + [C.POINTER(C.c_float)] * 3),
    "sitrk_pairs_stats": (_int, [_vp, C.POINTER(_i64)]),
    "sitrk_dist_values": (_int, [_vp, _i64, _vp, _vp, _int, _vp, _vp, _int, _vp, _vp, _vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "sitrk_mesh_dist": (_int, [_vp, _int, _int, _int, _int, _int, _vp, _vp, _int, _vp, _vp, _vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "sitrk_dist_kernel_ms": (_int, [_vp] + [C.POINTER(C.c_float)] * 3),
    "sitrk_dist_stats": (_int, [_vp, C.POINTER(_int), C.POINTER(C.c_float)]),
    "sitrk_coast_build": (_int, [_vp, _int, _int, _vp, _vp, _vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "sitrk_coast_segments": (_int, [_vp, _i64, _vp, _vp, C.POINTER(_i64)]),
    "sitrk_coast_dist": (_int, [_vp, _i64, _vp, _dbl, _vp, _vp]),
    "sitrk_coast_dist_buoys": (_int, [_vp, _dbl, _vp, _vp]),
    "sitrk_coast_kernel_ms": (_int, [_vp, C.POINTER(C.c_float)]),
    "sitrk_count_alive": (_int, [_vp, C.POINTER(_i64)]),
    "sitrk_find_cells": (_int, [_vp, _i64, _vp, _vp, _vp, _vp]),
    "sitrk_seed_init": (_int, [_vp, _i64] + [_vp] * 9),
    "sitrk_nemo_seed": (_int, [_vp, _int, _int, _int] + [_vp] * 7 + [_dbl, _dbl, _i64, _vp, _vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "sitrk_subsample_cloud": (_int, [_vp, _i64, _vp, _dbl, _vp, C.POINTER(_i64), C.POINTER(C.c_int32)]),
    "sitrk_cancel_too_close": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _dbl, _vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "sitrk_nearest_buoy": (_int, [_vp, _i64, _vp, _vp, _vp, _dbl, _vp, _vp]),
    "sitrk_nearest_point": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _dbl, _int, _vp, _vp]),
    "sitrk_eval_haversine": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "sitrk_eval_inside": (_int, [_vp, _i64, _vp, _vp, _vp]),
    "sitrk_eval_euler": (_int, [_vp, _i64, _vp, _vp, _dbl, _vp]),
    "sitrk_eval_intersect": (_int, [_vp, _i64, _vp, _vp, _vp]),
    "sitrk_eval_crossing": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "sitrk_survive_mask": (_int, [_vp, _vp, _vp]),
    "sitrk_cart2geo": (_int, [_vp, _i64, _vp, _dbl, _dbl, _vp]),
    "sitrk_geo2cart": (_int, [_vp, _i64, _vp, _dbl, _dbl, _vp]),
    "sitrk_timer_start": (_int, [_vp]),
    "sitrk_timer_stop": (_int, [_vp, C.POINTER(C.c_float)]),
}


class SitrkError(RuntimeError):
    pass


def build(force=False, verbose=False):
    """Compile libsitrk.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC] + (["-B"] if force else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or r.returncode:
        print(r.stdout + r.stderr)
    if r.returncode:
        raise SitrkError("building libsitrk.so failed (hipcc --offload-arch=gfx950)")
    return SO_PATH


_lib = None


def _one_hip_runtime():
    """A process must run on ONE HIP runtime.  PyTorch-ROCm wheels bundle their own (same soname as /opt/rocm's), and
    whichever copy is loaded first serves both libsitrk.so and torch: with the system's copy first, torch's bundled
    RCCL/HSA libraries come up next to it and the runtime that initialises second sees no device.  So if PyTorch is
    installed and not loaded yet, its copy is loaded before libsitrk.so (found without importing torch;
    SITRK_HIP_RUNTIME=system keeps the system's)."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("SITRK_HIP_RUNTIME", "") == "system":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    for loc in (spec.submodule_search_locations or []) if spec else []:
        p = os.path.join(loc, "lib", "libamdhip64.so")
        if os.path.exists(p):
            try:
                C.CDLL(p, mode=C.RTLD_GLOBAL)
            except OSError:
                pass
            return


def lib():
    """Load the in-tree extension; raise loudly if it is not there."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise SitrkError("%s not found: build it with `make -C %s` (or __graft_entry__.build()); "
                             "sitrack_amd has no CPU fallback" % (SO_PATH, CSRC))
        _one_hip_runtime()
        L = C.CDLL(SO_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_vp)


def as_c(a, dtype, shape=None, name="array"):
    """C-contiguous array of `dtype` (copy only when needed); validates the shape."""
    b = np.ascontiguousarray(a, dtype=dtype)
    if shape is not None and tuple(b.shape) != tuple(shape):
        raise ValueError("%s: expected shape %s, got %s" % (name, tuple(shape), tuple(b.shape)))
    return b


def reach(age, nsub=1):
    """The band/box rule of include/sitrk.h: `age` records after the buoys' host cells were evaluated, a buoy can start its
    step D = (age+1)*nsub - 1 cells away from them (a host cell moves at most one cell per sub-step; D = age for nsub = 1)."""
    return (int(age) + 1) * int(nsub) - 1


class Context:
    """Owns one sitrk_t handle (= one GPU)."""

    def __init__(self, device=0):
        self._L = lib()
        h = _vp()
        rc = self._L.sitrk_create(C.byref(h), int(device))
        if rc:
            raise SitrkError("sitrk_create: %s" % self._L.sitrk_last_error(None).decode())
        self._h = h
        self.device = int(device)
        self.Nj = self.Ni = 0
        self.nP = 0
        self.nslots = 0
        self.field_dtype = None
        self.nsub = 1

    # -- plumbing
    def _chk(self, rc):
        if rc:
            msg = self._L.sitrk_last_error(self._h).decode()
            if rc == -2:
                raise IndexError(msg)
            raise SitrkError(msg)

    def close(self):
        if getattr(self, "_h", None):
            self._L.sitrk_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def sync(self):
        self._chk(self._L.sitrk_sync(self._h))

    def set_stream(self, hip_stream):
        self._chk(self._L.sitrk_set_stream(self._h, hip_stream))

    # -- grid / params / records
    def set_grid(self, Yf, Xf, Yu, Xu, Yv, Xv, tmask):
        Yf = as_c(Yf, np.float64)
        Nj, Ni = Yf.shape
        arrs = [Yf] + [as_c(a, np.float64, (Nj, Ni), n) for a, n in
                       ((Xf, "Xf"), (Yu, "Yu"), (Xu, "Xu"), (Yv, "Yv"), (Xv, "Xv"))]
        tm = as_c(tmask, np.int8, (Nj, Ni), "tmask")
        self._chk(self._L.sitrk_set_grid(self._h, Nj, Ni, *[_ptr(a) for a in arrs], _ptr(tm)))
        self.Nj, self.Ni = Nj, Ni
        self.nP = 0
        self.nslots = 0

    def set_params(self, rdt=3600., uv_strategy=1, rmin_conc=0.1):
        self._chk(self._L.sitrk_set_params(self._h, float(rdt), int(uv_strategy), float(rmin_conc)))

    def set_substeps(self, nsub):
        """Advance every record in `nsub` Euler sub-steps of rdt/nsub (sitrk_set_substeps; 1 = the reference's one step)."""
        self._chk(self._L.sitrk_set_substeps(self._h, int(nsub)))
        self.nsub = int(nsub)

    def reach(self, age=0):
        """D: how many cells away from its host cell at the last buoy_rows()/buoy_box() evaluation a buoy can start the
        step of the record `age` records after it -- one cell per sub-step, (age+1)*nsub - 1 (= age without sub-steps)."""
        return reach(age, self.nsub)

    def set_tuning(self, **knobs):
        for k, v in knobs.items():
            self._chk(self._L.sitrk_set_tuning(self._h, k.encode(), int(v)))

    def alloc_records(self, nslots, dtype=np.float32):
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("records must be float32 or float64")
        self._chk(self._L.sitrk_alloc_records(self._h, int(nslots), SITRK_F64 if dt == np.float64 else SITRK_F32))
        self.nslots = int(nslots)
        self.field_dtype = dt

    def push_record(self, slot, u, v, sic):
        shp = (self.Nj, self.Ni)
        u = as_c(u, self.field_dtype, shp, "u")
        v = as_c(v, self.field_dtype, shp, "v")
        sic = as_c(sic, self.field_dtype, shp, "sic")
        # asynchronous: the library copies the fields into its pinned staging before returning (temporaries are fine)
        self._chk(self._L.sitrk_push_record(self._h, int(slot), _ptr(u), _ptr(v), _ptr(sic)))

    def stage(self, nrows=None, ncols=None):
        """The library's next pinned staging buffer as three (nrows, ncols) arrays of the records' dtype (ncols = Ni unless
        a box is staged): read the record straight into them, then submit(slot, j0[, i0]).  The arrays are VIEWS of pinned
        host memory the library owns: valid until submit() / stage_release(), and dangling after alloc_records(),
        set_grid() or close(), which free it.  Prefer stage_fill(), which also releases the buffer when the read fails."""
        nrows = self.Nj if nrows is None else int(nrows)
        ncols = self.Ni if ncols is None else int(ncols)
        pu, pv, ps = _vp(), _vp(), _vp()
        if ncols == self.Ni:
            self._chk(self._L.sitrk_stage_acquire(self._h, nrows, C.byref(pu), C.byref(pv), C.byref(ps)))
        else:
            self._chk(self._L.sitrk_stage_acquire_box(self._h, nrows, ncols, C.byref(pu), C.byref(pv), C.byref(ps)))
        nb = nrows * ncols * self.field_dtype.itemsize

        def view(p):
            return np.frombuffer((C.c_char * nb).from_address(p.value), dtype=self.field_dtype).reshape(nrows, ncols)
        self._staged_rows, self._staged_cols = nrows, ncols
        return view(pu), view(pv), view(ps)

    def stage_release(self):
        """Give the buffer handed out by stage() back without uploading it (the read into it failed): the views must not
        be used any more, the next stage() hands out the same buffer."""
        self._chk(self._L.sitrk_stage_release(self._h))

    def stage_fill(self, slot, j0, nrows, fill, i0=0, ncols=None):
        """stage() + fill(u, v, sic) + submit(slot, j0, i0), exception safe: if `fill` raises, the buffer is released, so the
        context stays usable (a later stage()/push_record is not refused with 'not submitted')."""
        bufs = self.stage(nrows, ncols)
        try:
            fill(*bufs)
        except BaseException:
            self.stage_release()
            raise
        finally:
            del bufs                                     # the views die with the hand-out
        self.submit(slot, j0, i0)

    def submit(self, slot, j0=0, i0=0):
        """Queue the staged box as rows [j0, j0+nrows) x columns [i0, i0+ncols) of `slot` (asynchronous, see
        sitrk_stage_submit / sitrk_stage_submit_box)."""
        j1, i1 = int(j0) + int(self._staged_rows), int(i0) + int(self._staged_cols)
        if int(i0) == 0 and i1 == self.Ni:
            self._chk(self._L.sitrk_stage_submit(self._h, int(slot), int(j0), j1))
        else:
            self._chk(self._L.sitrk_stage_submit_box(self._h, int(slot), int(j0), j1, int(i0), i1))

    def launch_stats(self, reset=False):
        a, b, c = _i64(0), _i64(0), _i64(0)
        self._chk(self._L.sitrk_launch_stats(self._h, int(bool(reset)), C.byref(a), C.byref(b), C.byref(c)))
        return {"fused_launches": a.value, "fused_records": b.value, "step_launches": c.value}

    def lane_stats(self, reset=False):
        """what of launch_stats() went on two lanes (knob "lanes"): segments between two joins, kernel launches of the lanes"""
        a, b = _i64(0), _i64(0)
        self._chk(self._L.sitrk_lane_stats(self._h, int(bool(reset)), C.byref(a), C.byref(b)))
        return {"lane_segments": a.value, "lane_launches": b.value}

    def buoy_rows(self):
        """(jmin, jmax) of the host rows of the buoys still alive; jmin > jmax when there is none."""
        a, b = C.c_int32(0), C.c_int32(0)
        self._chk(self._L.sitrk_buoy_rows(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def band(self, age=0):
        """Rows [j0,j1) of a record the next step(s) can touch: [jmin-2-D, jmax+3+D) clipped to the grid, where `age`
        = number of records stepped since buoy_rows() was evaluated and D = reach(age) (a host cell moves at most one row
        per sub-step)."""
        jmin, jmax = self.buoy_rows()
        if jmin > jmax:
            return 0, 0
        d = reach(age, self.nsub)
        return max(0, jmin - 2 - d), min(self.Nj, jmax + 3 + d)

    def buoy_box(self):
        """(jmin, jmax, imin, imax) of the host cells of the buoys still alive; jmin > jmax when there is none."""
        v = [C.c_int32(0) for _ in range(4)]
        self._chk(self._L.sitrk_buoy_box(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def box(self, age=0, align=4):
        """The box (j0, j1, i0, i1) of a record the next step(s) can touch: rows [jmin-2-D, jmax+3+D) x columns
        [imin-2-D, imax+3+D) clipped to the grid, the columns widened to multiples of `align` (16-byte lines of an fp32
        row).  `age` = records stepped since, D = reach(age) (a host cell moves at most one row and one column per
        sub-step)."""
        jmin, jmax, imin, imax = self.buoy_box()
        return self.box_of(jmin, jmax, imin, imax, age, align)

    def box_of(self, jmin, jmax, imin, imax, age=0, align=4):
        if jmin > jmax:
            return 0, 0, 0, 0
        d = reach(age, getattr(self, "nsub", 1))
        i0, i1 = max(0, imin - 2 - d), min(self.Ni, imax + 3 + d)
        i0 -= i0 % align
        i1 = min(self.Ni, -(-i1 // align) * align)
        return max(0, jmin - 2 - d), min(self.Nj, jmax + 3 + d), i0, i1

    def push_record_box(self, slot, j0, j1, i0, i1, u_box, v_box, sic_box):
        """The box rows [j0,j1) x columns [i0,i1) of a record from three (j1-j0, i1-i0) arrays.  Views into whole fields
        (`u[j0:j1, i0:i1]`: rows contiguous, one common row pitch) are handed over as they are -- the library gathers
        them into its pinned staging -- anything else is made contiguous first."""
        shp = (j1 - j0, i1 - i0)
        es = self.field_dtype.itemsize
        arrs = [np.asarray(x) for x in (u_box, v_box, sic_box)]
        for x, n in zip(arrs, ("u box", "v box", "sic box")):
            if tuple(x.shape) != shp:
                raise ValueError("%s: expected shape %s, got %s" % (n, shp, tuple(x.shape)))
        pitched = all(x.dtype == self.field_dtype and x.ndim == 2 and x.strides[1] == es and x.strides[0] % es == 0
                      and x.strides[0] >= shp[1] * es for x in arrs) and len({x.strides[0] for x in arrs}) == 1
        if pitched and shp[0] > 0 and shp[1] > 0:
            ld = arrs[0].strides[0] // es
        else:
            arrs = [as_c(x, self.field_dtype, shp) for x in arrs]
            ld = shp[1]
        self._chk(self._L.sitrk_push_record_box(self._h, int(slot), int(j0), int(j1), int(i0), int(i1), *[_ptr(x) for x in arrs], int(ld)))

    def buoy_box_begin(self):
        """queue the evaluation of buoy_box() on the compute stream without waiting for it (see sitrk_buoy_box_begin)"""
        self._chk(self._L.sitrk_buoy_box_begin(self._h))

    def buoy_box_end(self):
        """(jmin, jmax, imin, imax, age): the box as it was when buoy_box_begin() was queued, and the records stepped since"""
        v = [C.c_int32(0) for _ in range(5)]
        self._chk(self._L.sitrk_buoy_box_end(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def commit_record_box(self, slot, j0, j1, i0, i1):
        self._chk(self._L.sitrk_commit_record_box(self._h, int(slot), int(j0), int(j1), int(i0), int(i1)))

    def commit_records_box(self, slot0, nrec, j0, j1, i0, i1, on_ingest_stream=False):
        """commit_record_box for the nrec slots (slot0 + k) % nslots in one launch; on_ingest_stream: next to the stepping of other
        slots (sitrk_commit_records_box_async: the slabs must be complete in device memory)"""
        fn = self._L.sitrk_commit_records_box_async if on_ingest_stream else self._L.sitrk_commit_records_box
        self._chk(fn(self._h, int(slot0), int(nrec), int(j0), int(j1), int(i0), int(i1)))

    def push_record_rows(self, slot, j0, j1, u_rows, v_rows, sic_rows):
        shp = (j1 - j0, self.Ni)
        u = as_c(u_rows, self.field_dtype, shp, "u rows")
        v = as_c(v_rows, self.field_dtype, shp, "v rows")
        s = as_c(sic_rows, self.field_dtype, shp, "sic rows")
        self._chk(self._L.sitrk_push_record_rows(self._h, int(slot), int(j0), int(j1), _ptr(u), _ptr(v), _ptr(s)))

    def commit_record_rows(self, slot, j0, j1):
        self._chk(self._L.sitrk_commit_record_rows(self._h, int(slot), int(j0), int(j1)))

    def push_record_dev(self, slot, dev_ptr):
        self._chk(self._L.sitrk_push_record_dev(self._h, int(slot), _vp(dev_ptr)))

    def record_ptr(self, slot):
        p = self._L.sitrk_record_ptr(self._h, int(slot))
        if not p:
            raise SitrkError("sitrk_record_ptr: bad slot %d" % slot)
        return p

    def commit_record(self, slot):
        self._chk(self._L.sitrk_commit_record(self._h, int(slot)))

    @property
    def slab_elems(self):
        return 3 * self.Nj * self.Ni

    # -- buoys
    def set_buoys(self, yx, jiT, rec_first=None, rec_last=None, sort=True):
        yx = as_c(yx, np.float64)
        nP = yx.shape[0]
        yx = as_c(yx, np.float64, (nP, 2), "yx")
        ji = np.asarray(jiT)
        if ji.shape != (nP, 2):
            raise ValueError("jiT: expected shape %s, got %s" % ((nP, 2), ji.shape))
        ji32 = as_c(ji, np.int32)
        if not np.array_equal(ji32, ji):
            raise IndexError("jiT does not fit int32")
        f = None if rec_first is None else as_c(rec_first, np.int32, (nP,), "rec_first")
        l = None if rec_last is None else as_c(rec_last, np.int32, (nP,), "rec_last")
        self._chk(self._L.sitrk_set_buoys(self._h, nP, _ptr(yx), _ptr(ji32), _ptr(f), _ptr(l)))
        self.nP = nP
        if sort:
            self.sort_buoys()

    def restore_state(self, alive, kill_rec):
        """after set_buoys(sort=False): dead flags and kill records of buoys that were stepped elsewhere before"""
        al = as_c(alive, np.int8, (self.nP,), "alive")
        kr = as_c(kill_rec, np.int32, (self.nP,), "kill_rec")
        self._chk(self._L.sitrk_restore_state(self._h, _ptr(al), _ptr(kr)))

    def sort_buoys(self):
        self._chk(self._L.sitrk_sort_buoys(self._h))

    def set_resort(self, every):
        self._chk(self._L.sitrk_set_resort(self._h, int(every)))

    def step(self, slot, jrec):
        self._chk(self._L.sitrk_step(self._h, int(slot), int(jrec)))

    def run(self, slot0, jrec0, nsteps):
        self._chk(self._L.sitrk_run(self._h, int(slot0), int(jrec0), int(nsteps)))

    def run_tlerp(self, slot0, jrec0, nsteps, phase, have_prev=False, have_next=False):
        """sitrk_run with the velocities of every sub-step blended linearly in time between consecutive records
        (sitrk_run_tlerp): `phase` in [0,1] = where in its step interval a record is valid (0.5 time means, 0 snapshots at the
        start); have_prev / have_next: the slots in front of slot0 / behind the last one hold records jrec0-1 / jrec0+nsteps."""
        self._chk(self._L.sitrk_run_tlerp(self._h, int(slot0), int(jrec0), int(nsteps), float(phase), int(bool(have_prev)),
                                          int(bool(have_next))))

    def fetch(self, want=("yx", "jiT", "alive", "kill_rec")):
        nP = self.nP
        out = {}
        if "yx" in want:
            out["yx"] = np.empty((nP, 2), dtype=np.float64)
        if "jiT" in want:
            out["jiT"] = np.empty((nP, 2), dtype=np.int32)
        if "alive" in want:
            out["alive"] = np.empty(nP, dtype=np.int8)
        if "kill_rec" in want:
            out["kill_rec"] = np.empty(nP, dtype=np.int32)
        self._chk(self._L.sitrk_fetch(self._h, _ptr(out.get("yx")), _ptr(out.get("jiT")), _ptr(out.get("alive")),
                                      _ptr(out.get("kill_rec"))))
        return out

    def fetch_record(self, jrec, latlon=False):
        nP = self.nP
        yx = np.empty((nP, 2), dtype=np.float64)
        mask = np.empty(nP, dtype=np.int8)
        ll = np.empty((nP, 2), dtype=np.float64) if latlon else None
        self._chk(self._L.sitrk_fetch_record(self._h, int(jrec), _ptr(yx), _ptr(mask), _ptr(ll)))
        return (yx, mask, ll) if latlon else (yx, mask)

    # -- model fields along the trajectories (sitrk_sample_*)
    @staticmethod
    def _sample_mode(mode):
        try:
            return _SAMPLE_MODES[mode]
        except (KeyError, TypeError):
            return int(mode)                 # the library refuses it with its own message

    def sample_slot(self, slot, jrec, mode, field):
        """sitrk_sample_slot: field 0/'u', 1/'v' or 2/'siconc' of the resident record in `slot` at every buoy's host cell, (nP,)
        of the records' dtype; mode 'after' (the buoys that stepped at jrec) or 'enter' (those that start at jrec), -9999
        elsewhere."""
        out = np.empty(self.nP, dtype=self.field_dtype)
        f = _SLOT_FIELDS.get(field, field) if isinstance(field, (str, int)) else field
        self._chk(self._L.sitrk_sample_slot(self._h, int(slot), int(jrec), self._sample_mode(mode), int(f), _ptr(out)))
        return out

    def sample_fields(self, jrec, mode, fields, box=None):
        """sitrk_sample_fields: `fields` = a list of (Nj,Ni) arrays, or of (j1-j0, i1-i0) arrays with box = (j0,j1,i0,i1), all
        float32 or all float64 -> (nf, nP) of that dtype.  Views into whole fields (`X[j0:j1, i0:i1]`, rows contiguous, one
        common row pitch) are handed over as they are."""
        j0, j1, i0, i1 = (0, self.Nj, 0, self.Ni) if box is None else (int(x) for x in box)
        shp = (j1 - j0, i1 - i0)
        arrs = [np.asarray(x) for x in fields]
        if not arrs:
            raise ValueError("sample_fields: no field given")
        dt = np.dtype(np.float64) if any(x.dtype.newbyteorder('=') == np.float64 for x in arrs) else np.dtype(np.float32)
        for k, x in enumerate(arrs):
            if tuple(x.shape) != shp:
                raise ValueError("sample_fields: field %d has shape %s, expected %s" % (k, tuple(x.shape), shp))
            if x.dtype.newbyteorder('=') != dt:
                raise ValueError("sample_fields: the fields must all be float32 or all float64 (field %d is %s)" % (k, x.dtype))
        es = dt.itemsize
        pitched = all(x.dtype == dt and x.strides[1] == es and x.strides[0] % es == 0 and x.strides[0] >= shp[1] * es for x in arrs) \
            and len({x.strides[0] for x in arrs}) == 1
        if pitched and shp[0] > 0 and shp[1] > 0:
            ld = arrs[0].strides[0] // es
        else:
            arrs = [as_c(x, dt, shp) for x in arrs]
            ld = shp[1]
        nf = len(arrs)
        out = np.empty((nf, self.nP), dtype=dt)
        ptrs = (_vp * nf)(*[x.ctypes.data for x in arrs])
        self._chk(self._L.sitrk_sample_fields(self._h, int(jrec), self._sample_mode(mode), nf, SITRK_F64 if dt == np.float64 else SITRK_F32,
                                              j0, j1, i0, i1, ptrs, int(ld), _ptr(out)))
        return out

    # -- deformation rates of buoy cells (sitrk_deform_*)
    @staticmethod
    def _deform_cells_arg(cells, name):
        """(nC, 3|4) int32, C-contiguous; indices that do not fit int32 become -1 (the library reports them as out of range)"""
        c = np.asarray(cells)
        if c.ndim != 2 or c.shape[1] not in (3, 4):
            raise ValueError("%s: cells must be an (nC, 3) or (nC, 4) integer array, got shape %s" % (name, c.shape))
        if c.dtype.kind not in "iu":
            raise ValueError("%s: cells must hold integers, got %s" % (name, c.dtype))
        c32 = as_c(c, np.int32)
        if c32.dtype != c.dtype:
            c32[c32 != c] = -1
        return c32

    def deform_cells(self, yx0, yx1, cells, T, mask0=None, mask1=None):
        """sitrk_deform_cells: (out (5, nC) = div, shr, vor, area0, area1; valid (nC,) bool; nvalid) of the cells (nC, 3|4) of
        buoy indices, from the positions yx0, yx1 (nP,2) km that lie T seconds apart; mask0 / mask1: 0 = invalid vertex."""
        yx0 = as_c(yx0, np.float64)
        nP = yx0.shape[0]
        yx0 = as_c(yx0, np.float64, (nP, 2), "yx0")
        yx1 = as_c(yx1, np.float64, (nP, 2), "yx1")
        m0 = None if mask0 is None else as_c(np.asarray(mask0) != 0, np.int8, (nP,), "mask0")
        m1 = None if mask1 is None else as_c(np.asarray(mask1) != 0, np.int8, (nP,), "mask1")
        c = self._deform_cells_arg(cells, "deform_cells")
        nC, nv = c.shape
        out = np.empty((5, nC), dtype=np.float64)
        valid = np.empty(nC, dtype=np.int8)
        nvalid = _i64(0)
        self._chk(self._L.sitrk_deform_cells(self._h, nP, _ptr(yx0), _ptr(yx1), _ptr(m0), _ptr(m1), nC, nv, _ptr(c), float(T),
                                             _ptr(out), _ptr(valid), C.byref(nvalid)))
        return out, valid.astype(bool), nvalid.value

    def deform_mark(self, jrec0):
        """sitrk_deform_mark: snapshot every buoy's position on the device; jrec0 = the model record stepped next"""
        self._chk(self._L.sitrk_deform_mark(self._h, int(jrec0)))

    def deform_since_mark(self, jrec1, cells):
        """sitrk_deform_since_mark, right after the step of jrec1: like deform_cells() between the mark and now, no position
        leaving the device"""
        c = self._deform_cells_arg(cells, "deform_since_mark")
        nC, nv = c.shape
        out = np.empty((5, nC), dtype=np.float64)
        valid = np.empty(nC, dtype=np.int8)
        nvalid = _i64(0)
        self._chk(self._L.sitrk_deform_since_mark(self._h, int(jrec1), nC, nv, _ptr(c), _ptr(out), _ptr(valid), C.byref(nvalid)))
        return out, valid.astype(bool), nvalid.value

    def deform_kernel_ms(self):
        """(points_ms, cells_ms): GPU time of the two kernels of the last deform call (sitrk_deform_kernel_ms)"""
        a, b = C.c_float(0), C.c_float(0)
        self._chk(self._L.sitrk_deform_kernel_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # -- quadrangles from triangles (sitrk_tri2quad*)
    @staticmethod
    def _tris_arg(tris, name):
        """(nT, 3) int32, C-contiguous; indices that do not fit int32 become -1 (the library reports them as out of range)"""
        t = np.asarray(tris)
        if t.ndim != 2 or t.shape[1] != 3:
            raise ValueError("%s: tris must be an (nT, 3) integer array, got shape %s" % (name, t.shape))
        if t.dtype.kind not in "iu":
            raise ValueError("%s: tris must hold integers, got %s" % (name, t.dtype))
        t32 = as_c(t, np.int32)
        if t32.dtype != t.dtype:
            t32[t32 != t] = -1
        return t32

    def tri2quad(self, yx, tris, mask=None, cos_lo=0.5, cos_hi=-0.5, ratio_min=0.5, area_min=0., area_max=float("inf"), cap=None):
        """sitrk_tri2quad: (quads (nQ,4) int32, tri_quad (nT,) int32, rounds) of the triangles tris (nT,3) over the points yx
        (nP,2) km; mask: 0 = no valid vertex; cap: rows of room for quads (default nT // 2, the least the library takes)."""
        yx = as_c(yx, np.float64)
        nP = yx.shape[0]
        yx = as_c(yx, np.float64, (nP, 2), "yx")
        m = None if mask is None else as_c(np.asarray(mask) != 0, np.int8, (nP,), "mask")
        t = self._tris_arg(tris, "tri2quad")
        nT = t.shape[0]
        cap = nT // 2 if cap is None else int(cap)
        quads = np.empty((max(cap, 0), 4), dtype=np.int32)
        tri_quad = np.empty(nT, dtype=np.int32)
        nQ, rounds = _i64(0), _int(0)
        self._chk(self._L.sitrk_tri2quad(self._h, nP, _ptr(yx), _ptr(m), nT, _ptr(t), float(cos_lo), float(cos_hi), float(ratio_min),
                                         float(area_min), float(area_max), cap, _ptr(quads), _ptr(tri_quad), C.byref(nQ),
                                         C.byref(rounds)))
        return quads[:nQ.value].copy(), tri_quad, rounds.value

    def tri2quad_buoys(self, tris, cos_lo=0.5, cos_hi=-0.5, ratio_min=0.5, area_min=0., area_max=float("inf"), cap=None):
        """sitrk_tri2quad_buoys: the same on the buoys of set_buoys() at their current positions (alive = valid vertex), no
        position leaving the device"""
        t = self._tris_arg(tris, "tri2quad_buoys")
        nT = t.shape[0]
        cap = nT // 2 if cap is None else int(cap)
        quads = np.empty((max(cap, 0), 4), dtype=np.int32)
        tri_quad = np.empty(nT, dtype=np.int32)
        nQ, rounds = _i64(0), _int(0)
        self._chk(self._L.sitrk_tri2quad_buoys(self._h, nT, _ptr(t), float(cos_lo), float(cos_hi), float(ratio_min), float(area_min),
                                               float(area_max), cap, _ptr(quads), _ptr(tri_quad), C.byref(nQ), C.byref(rounds)))
        return quads[:nQ.value].copy(), tri_quad, rounds.value

    def tri2quad_kernel_ms(self):
        """(adjacency_ms, score_ms, rounds_ms, compact_ms): GPU time of the phases of the last tri2quad call (sitrk_tri2quad_kernel_ms)"""
        v = [C.c_float(0) for _ in range(4)]
        self._chk(self._L.sitrk_tri2quad_kernel_ms(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    # -- bounded Delaunay triangulation (sitrk_delaunay*)
    def _delaunay_call(self, call, nP, cap):
        """runs call(cap, tris, nT, vertex) with room for cap rows (default: the bound 2 nP, cut to what came back)"""
        rows = max(0, 2 * nP - 5) if cap is None else int(cap)
        tris = np.empty((max(rows, 0), 3), dtype=np.int32)
        vertex = np.zeros(nP, dtype=np.int8)
        nT = _i64(0)
        self._chk(call(rows, _ptr(tris), C.byref(nT), _ptr(vertex)))
        if nT.value > rows:
            return None, nT.value, vertex
        return tris[:nT.value].copy(), nT.value, vertex

    def delaunay(self, yx, rmax_km, mask=None, cap=None):
        """sitrk_delaunay: (tris (nT,3) int32, nT, vertex (nP,) int8) of the points yx (nP,2) km: every Delaunay triangle of
        circumradius <= rmax_km, rows (p,q,r) counter-clockwise, p lowest, in ascending (p,q); mask: 0 = no vertex; cap: rows of
        room (default 2 nP - 5, the most there can be); with cap < nT tris is None."""
        yx = as_c(yx, np.float64)
        nP = yx.shape[0]
        yx = as_c(yx, np.float64, (nP, 2), "yx")
        m = None if mask is None else as_c(np.asarray(mask) != 0, np.int8, (nP,), "mask")
        return self._delaunay_call(lambda cap_, t, n, v: self._L.sitrk_delaunay(self._h, nP, _ptr(yx), _ptr(m), float(rmax_km), cap_, t, n, v),
                                   nP, cap)

    def delaunay_buoys(self, rmax_km, cap=None):
        """sitrk_delaunay_buoys: the same on the buoys of set_buoys() at their current positions (alive = can be a vertex), no
        position leaving the device"""
        return self._delaunay_call(lambda cap_, t, n, v: self._L.sitrk_delaunay_buoys(self._h, float(rmax_km), cap_, t, n, v), self.nP, cap)

    def delaunay_kernel_ms(self):
        """(bin_ms, tri_ms, compact_ms): GPU time of the phases of the last delaunay call (sitrk_delaunay_kernel_ms)"""
        v = [C.c_float(0) for _ in range(3)]
        self._chk(self._L.sitrk_delaunay_kernel_ms(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def delaunay_stats(self):
        """(in-circle tests, those that took the 128-bit path) of the last delaunay call (sitrk_delaunay_stats)"""
        a, b = _i64(0), _i64(0)
        self._chk(self._L.sitrk_delaunay_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # -- device-resident quadrangle meshes (sitrk_mesh_*)
    def mesh_build(self, mesh, jrec0, rmax_km, mask=None, cos_lo=0.5, cos_hi=-0.5, ratio_min=0.5, area_min=0., area_max=float("inf")):
        """sitrk_mesh_build: (nT, nQ, rounds) of the mesh built in slot `mesh` from the buoys of set_buoys() at their current
        positions: the bounded Delaunay triangles of the buoys alive now whose mask (nP, caller's order) is not 0, paired into
        quadrangles; jrec0 = the model record stepped next.  No triangle, quadrangle or position leaves the device."""
        m = None if mask is None else as_c(np.asarray(mask) != 0, np.int8, (self.nP,), "mask")
        nT, nQ, rounds = _i64(0), _i64(0), _int(0)
        self._chk(self._L.sitrk_mesh_build(self._h, int(mesh), int(jrec0), float(rmax_km), _ptr(m), float(cos_lo), float(cos_hi),
                                           float(ratio_min), float(area_min), float(area_max), C.byref(nT), C.byref(nQ), C.byref(rounds)))
        return nT.value, nQ.value, rounds.value

    def mesh_cells(self, mesh):
        """sitrk_mesh_cells: the quadrangles (nQ,4) int32 of buoy indices of the mesh in slot `mesh`"""
        nQ = _i64(0)
        self._chk(self._L.sitrk_mesh_cells(self._h, int(mesh), 0, None, C.byref(nQ)))
        cells = np.empty((nQ.value, 4), dtype=np.int32)
        if nQ.value:
            self._chk(self._L.sitrk_mesh_cells(self._h, int(mesh), nQ.value, _ptr(cells), C.byref(nQ)))
        return cells

    def mesh_mark(self, mesh, jrec0):
        """sitrk_mesh_mark: the same cells' t0 positions taken again at the current positions; jrec0 = the record stepped next"""
        self._chk(self._L.sitrk_mesh_mark(self._h, int(mesh), int(jrec0)))

    def mesh_deform(self, mesh, jrec1, want=("out", "status", "stats")):
        """sitrk_mesh_deform, right after the step of jrec1: a dict with those of out (5, nQ) = div, shr, vor, area0, area1,
        status (nQ,) int8 (0 invalid, 1 valid and acceptable at t1, 2 valid, not acceptable) and stats (MESH_NSTATS,) that `want`
        names; only they come back from the device."""
        want = (want,) if isinstance(want, str) else tuple(want)
        bad = [w for w in want if w not in ("out", "status", "stats")]
        if bad or not want:
            raise ValueError("mesh_deform: want must name some of 'out', 'status', 'stats', got %r" % (want,))
        nQ = _i64(0)
        if "out" in want or "status" in want:
            self._chk(self._L.sitrk_mesh_cells(self._h, int(mesh), 0, None, C.byref(nQ)))
        res = {}
        if "out" in want:
            res["out"] = np.empty((5, nQ.value), dtype=np.float64)
        if "status" in want:
            res["status"] = np.empty(nQ.value, dtype=np.int8)
        if "stats" in want:
            res["stats"] = np.zeros(MESH_NSTATS, dtype=np.float64)
        self._chk(self._L.sitrk_mesh_deform(self._h, int(mesh), int(jrec1), _ptr(res.get("out")), _ptr(res.get("status")),
                                            _ptr(res.get("stats"))))
        return res

    def mesh_free(self, mesh):
        """sitrk_mesh_free: empties slot `mesh`"""
        self._chk(self._L.sitrk_mesh_free(self._h, int(mesh)))

    def mesh_kernel_ms(self, build=True, deform=True):
        """(build_ms, points_ms, cells_ms, stats_ms): GPU time of the last mesh_build (whole device chain) and of the kernels of
        the last mesh_deform (sitrk_mesh_kernel_ms); None for the part not asked for"""
        v = [C.c_float(0) for _ in range(4)]
        ask = [build, deform, deform, deform]
        self._chk(self._L.sitrk_mesh_kernel_ms(self._h, *[C.byref(x) if a else None for x, a in zip(v, ask)]))
        return tuple(x.value if a else None for x, a in zip(v, ask))

    # -- cells rasterised onto a regular grid (sitrk_raster_*)
    @staticmethod
    def _grid_arg(grid, name):
        """(y0, x0, d, ny, nx) as the C types; the library checks the values"""
        try:
            y0, x0, d, ny, nx = grid
            g = (float(y0), float(x0), float(d), int(ny), int(nx))
        except (TypeError, ValueError):
            raise ValueError("%s: grid must be (y0_km, x0_km, d_km, ny, nx), got %r" % (name, grid)) from None
        if g[3] != ny or g[4] != nx or not (-2 ** 31 <= g[3] < 2 ** 31 and -2 ** 31 <= g[4] < 2 ** 31):
            raise ValueError("%s: ny and nx must be integers that fit int32, got %r, %r" % (name, ny, nx))
        return g

    def raster_cells(self, yx, cells, grid, draw=None):
        """sitrk_raster_cells: (owner (ny,nx) int32, nowned) of the cells (nC, 3|4) of indices into the points yx (nP,2) km on the
        grid (y0_km, x0_km, d_km, ny, nx): per pixel the lowest-indexed drawn cell its centre lies in, -1 for none; draw (nC):
        0 = the cell is not drawn."""
        g = self._grid_arg(grid, "raster_cells")
        yx = as_c(yx, np.float64)
        nP = yx.shape[0]
        yx = as_c(yx, np.float64, (nP, 2), "yx")
        c = self._deform_cells_arg(cells, "raster_cells")
        nC, nv = c.shape
        dr = None if draw is None else as_c(np.asarray(draw) != 0, np.int8, (nC,), "draw")
        owner = np.empty((max(g[3], 0), max(g[4], 0)), dtype=np.int32)
        nowned = _i64(0)
        self._chk(self._L.sitrk_raster_cells(self._h, nP, _ptr(yx), nC, nv, _ptr(c), _ptr(dr), *g, _ptr(owner), C.byref(nowned)))
        return owner, nowned.value

    def mesh_raster(self, mesh, jrec1, grid, at_t1=False, want=("owner", "fields")):
        """sitrk_mesh_raster, right after the step of jrec1: a dict with those of owner (ny,nx) int32 and fields (5,ny,nx) fp64 =
        div, shr, vor, area0, area1 of the owner (FillValue where there is none) that `want` names, and nowned; the cells of the
        mesh in slot `mesh` drawn at their t0 positions (status 1 or 2) or, at_t1, at the current ones (status 1).  Only the
        raster comes back from the device."""
        want = (want,) if isinstance(want, str) else tuple(want)
        bad = [w for w in want if w not in ("owner", "fields")]
        if bad or not want:
            raise ValueError("mesh_raster: want must name some of 'owner', 'fields', got %r" % (want,))
        g = self._grid_arg(grid, "mesh_raster")
        ny, nx = max(g[3], 0), max(g[4], 0)
        res = {}
        if "owner" in want:
            res["owner"] = np.empty((ny, nx), dtype=np.int32)
        if "fields" in want:
            res["fields"] = np.empty((5, ny, nx), dtype=np.float64)
        nowned = _i64(0)
        self._chk(self._L.sitrk_mesh_raster(self._h, int(mesh), int(jrec1), 1 if at_t1 else 0, *g, _ptr(res.get("owner")),
                                            _ptr(res.get("fields")), C.byref(nowned)))
        res["nowned"] = nowned.value
        return res

    def raster_kernel_ms(self):
        """(cells_ms, gather_ms): GPU time of the fill with the cell kernel and of the gather kernel of the last raster call
        (sitrk_raster_kernel_ms)"""
        a, b = C.c_float(0), C.c_float(0)
        self._chk(self._L.sitrk_raster_kernel_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def raster_stats(self):
        """claims -- centres found inside a drawn cell, one atomic each -- of the last raster call that ran under
        set_tuning(raster_count=1) (sitrk_raster_stats)"""
        a = _i64(0)
        self._chk(self._L.sitrk_raster_stats(self._h, C.byref(a)))
        return a.value

    # -- coarse-grained deformation (sitrk_coarse_*)
    @staticmethod
    def coarse_level_shapes(ny, nx, nlev):
        """[(ny_l, nx_l)] of the levels 0 .. nlev-1 of the pyramid over an ny x nx grid"""
        return [((ny + (1 << l) - 1) >> l, (nx + (1 << l) - 1) >> l) for l in range(nlev)]

    def _coarse_out(self, g, nlev, boxes):
        nlev = int(nlev)
        shapes = self.coarse_level_shapes(max(g[3], 0), max(g[4], 0), min(max(nlev, 0), COARSE_MAXLEV))
        pyr = np.empty(6 * sum(a * b for a, b in shapes), dtype=np.float64) if boxes else None
        return nlev, shapes, pyr, np.zeros((len(shapes), COARSE_NCOLS), dtype=np.float64)

    @staticmethod
    def _coarse_result(shapes, pyr, table, nin, nout):
        levels = None
        if pyr is not None:
            levels, o = [], 0
            for a, b in shapes:
                levels.append(pyr[o:o + 6 * a * b].reshape(6, a, b))
                o += 6 * a * b
        return {"table": table, "nin": nin.value, "nout": nout.value, "levels": levels}

    def coarse_cells(self, yx0, yx1, cells, T, grid, nlev, fmin=0.5, mask0=None, mask1=None, use=None, boxes=False):
        """sitrk_coarse_cells: the cells (nC, 3|4) of indices into the points yx0, yx1 (nP,2) km, T seconds apart, coarse-grained
        on the pyramid of nlev levels over the grid (y0_km, x0_km, d_km, ny, nx).  A dict with table (nlev, 8) under the names
        COARSE_COLS, nin, nout and levels: None, or with boxes=True per level the (6, ny_l, nx_l) values COARSE_VALUES.  mask0 /
        mask1 (nP): 0 = invalid vertex; use (nC): 0 = the cell does not contribute."""
        g = self._grid_arg(grid, "coarse_cells")
        yx0 = as_c(yx0, np.float64)
        nP = yx0.shape[0]
        yx0 = as_c(yx0, np.float64, (nP, 2), "yx0")
        yx1 = as_c(yx1, np.float64, (nP, 2), "yx1")
        m0 = None if mask0 is None else as_c(np.asarray(mask0) != 0, np.int8, (nP,), "mask0")
        m1 = None if mask1 is None else as_c(np.asarray(mask1) != 0, np.int8, (nP,), "mask1")
        c = self._deform_cells_arg(cells, "coarse_cells")
        nC, nv = c.shape
        u = None if use is None else as_c(np.asarray(use) != 0, np.int8, (nC,), "use")
        nlev, shapes, pyr, table = self._coarse_out(g, nlev, boxes)
        nin, nout = _i64(0), _i64(0)
        self._chk(self._L.sitrk_coarse_cells(self._h, nP, _ptr(yx0), _ptr(yx1), _ptr(m0), _ptr(m1), nC, nv, _ptr(c), _ptr(u), float(T),
                                             *g, nlev, float(fmin), _ptr(pyr), _ptr(table), C.byref(nin), C.byref(nout)))
        return self._coarse_result(shapes, pyr, table, nin, nout)

    def mesh_coarse(self, mesh, jrec1, grid, nlev, fmin=0.5, boxes=False):
        """sitrk_mesh_coarse, right after the step of jrec1: the status-1 cells of the mesh in slot `mesh` coarse-grained like
        coarse_cells(), at their t0 positions; the same dict.  Only the table -- and with boxes=True the pyramid -- comes back
        from the device."""
        g = self._grid_arg(grid, "mesh_coarse")
        nlev, shapes, pyr, table = self._coarse_out(g, nlev, boxes)
        nin, nout = _i64(0), _i64(0)
        self._chk(self._L.sitrk_mesh_coarse(self._h, int(mesh), int(jrec1), *g, nlev, float(fmin), _ptr(pyr), _ptr(table),
                                            C.byref(nin), C.byref(nout)))
        return self._coarse_result(shapes, pyr, table, nin, nout)

    def coarse_kernel_ms(self):
        """(terms_ms, sort_ms, level0_ms, pyramid_ms, table_ms): GPU time of the phases of the last coarse-graining call
        (sitrk_coarse_kernel_ms)"""
        v = [C.c_float(0) for _ in range(5)]
        self._chk(self._L.sitrk_coarse_kernel_ms(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    # -- features of a map: connected components (sitrk_label_raster, sitrk_mesh_features)
    @staticmethod
    def _features_result(table, nfeat, ncomp, nactive, labels):
        rows = min(nfeat.value, table.shape[0])
        return {"table": table[:rows], "nfeat": nfeat.value, "ncomp": ncomp.value, "nactive": nactive.value, "labels": labels}

    def label_raster(self, active, conn=8, min_pix=1, maxfeat=65536, labels=True):
        """sitrk_label_raster: the connected components of the mask active (ny,nx) (a pixel is active iff its value is not 0) for
        conn = 4 or 8 neighbours.  A dict with table (rows, 12) int64 under the names FEAT_COLS -- one row per component of at
        least min_pix pixels, in ascending label, the first maxfeat of them --, nfeat (all such components: above maxfeat the
        table is truncated), ncomp, nactive and labels: (ny,nx) int32, -1 or the lowest linear index of the pixel's component;
        None with labels=False."""
        a = np.asarray(active)
        if a.ndim != 2:
            raise ValueError("label_raster: active must be (ny, nx), got shape %s" % (a.shape,))
        a = as_c(a != 0, np.int8)
        ny, nx = a.shape
        if not (ny < 2 ** 31 and nx < 2 ** 31):
            raise ValueError("label_raster: ny and nx must fit int32, got %d, %d" % (ny, nx))
        maxfeat = int(maxfeat)
        table = np.zeros((max(maxfeat, 0), FEAT_NCOLS), dtype=np.int64)
        lab = np.empty((ny, nx), dtype=np.int32) if labels else None
        nfeat, ncomp, nactive = _i64(0), _i64(0), _i64(0)
        self._chk(self._L.sitrk_label_raster(self._h, ny, nx, _ptr(a), int(conn), int(min_pix), maxfeat, _ptr(lab),
                                             _ptr(table) if maxfeat > 0 else None, C.byref(nfeat), C.byref(ncomp), C.byref(nactive)))
        return self._features_result(table, nfeat, ncomp, nactive, lab)

    def mesh_features(self, mesh, jrec1, grid, what, thr, sgn=1, conn=8, min_pix=1, maxfeat=65536, at_t1=False, labels=False):
        """sitrk_mesh_features, right after the step of jrec1: the mesh in slot `mesh` rasterised like mesh_raster(), the pixels
        with an owner whose rate `what` (0 div, 1 shr, 2 vor, 3 tot, or those names) passes sgn*f >= thr (tot: div^2 + shr^2 >=
        thr^2) labelled like label_raster(); the same dict.  Owner and rates stay on the device: only the table, the counts and,
        with labels=True, the labels come back."""
        g = self._grid_arg(grid, "mesh_features")
        what = FEAT_WHAT.get(what, what)
        maxfeat = int(maxfeat)
        table = np.zeros((max(maxfeat, 0), FEAT_NCOLS), dtype=np.int64)
        lab = np.empty((max(g[3], 0), max(g[4], 0)), dtype=np.int32) if labels else None
        nfeat, ncomp, nactive = _i64(0), _i64(0), _i64(0)
        self._chk(self._L.sitrk_mesh_features(self._h, int(mesh), int(jrec1), 1 if at_t1 else 0, *g, int(what), int(sgn), float(thr),
                                              int(conn), int(min_pix), maxfeat, _ptr(lab), _ptr(table) if maxfeat > 0 else None,
                                              C.byref(nfeat), C.byref(ncomp), C.byref(nactive)))
        return self._features_result(table, nfeat, ncomp, nactive, lab)

    def features_kernel_ms(self):
        """(mask_ms, label_ms, table_ms): GPU time of the phases of the last labelling call (sitrk_features_kernel_ms)"""
        v = [C.c_float(0) for _ in range(3)]
        self._chk(self._L.sitrk_features_kernel_ms(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    # -- features from window to window: kept maps, advection, matching (sitrk_keep_*, sitrk_mesh_features_advect, sitrk_features_match)
    def mesh_features_keep(self, keep, mesh, jrec1, grid, what, thr, sgn=1, conn=8, min_pix=1, maxfeat=65536, at_t1=False, labels=False):
        """sitrk_mesh_features_keep: mesh_features() with the same arguments and the same dict, and the labels of the features
        of at least min_pix pixels (-1 elsewhere) kept on the device in slot `keep` (0..KEEP_MAX-1)"""
        g = self._grid_arg(grid, "mesh_features_keep")
        what = FEAT_WHAT.get(what, what)
        maxfeat = int(maxfeat)
        table = np.zeros((max(maxfeat, 0), FEAT_NCOLS), dtype=np.int64)
        lab = np.empty((max(g[3], 0), max(g[4], 0)), dtype=np.int32) if labels else None
        nfeat, ncomp, nactive = _i64(0), _i64(0), _i64(0)
        self._chk(self._L.sitrk_mesh_features_keep(self._h, int(keep), int(mesh), int(jrec1), 1 if at_t1 else 0, *g, int(what), int(sgn),
                                                   float(thr), int(conn), int(min_pix), maxfeat, _ptr(lab),
                                                   _ptr(table) if maxfeat > 0 else None, C.byref(nfeat), C.byref(ncomp), C.byref(nactive)))
        return self._features_result(table, nfeat, ncomp, nactive, lab)

    def keep_put(self, keep, labels, conn=8, min_pix=1):
        """sitrk_keep_put: the host map labels (ny,nx), every value -1 or in [0, ny*nx), into slot `keep`"""
        a = np.asarray(labels)
        if a.ndim != 2 or a.dtype.kind not in "iu":
            raise ValueError("keep_put: labels must be an (ny, nx) array of integers, got %s %s" % (a.shape, a.dtype))
        ny, nx = a.shape
        if not (ny < 2 ** 31 and nx < 2 ** 31):
            raise ValueError("keep_put: ny and nx must fit int32, got %d, %d" % (ny, nx))
        if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise IndexError("keep_put: a value of the map does not fit int32")
        a = as_c(a, np.int32)
        self._chk(self._L.sitrk_keep_put(self._h, int(keep), ny, nx, _ptr(a), int(conn), int(min_pix)))

    def keep_get(self, keep, labels=True):
        """sitrk_keep_get: {"shape": (ny, nx), "conn", "min_pix", "labels": (ny,nx) int32 or None with labels=False} of slot `keep`"""
        ny, nx, conn, min_pix = _int(0), _int(0), _int(0), _i64(0)
        self._chk(self._L.sitrk_keep_get(self._h, int(keep), C.byref(ny), C.byref(nx), C.byref(conn), C.byref(min_pix), None))
        lab = None
        if labels:
            lab = np.empty((ny.value, nx.value), dtype=np.int32)
            self._chk(self._L.sitrk_keep_get(self._h, int(keep), None, None, None, None, _ptr(lab)))
        return {"shape": (ny.value, nx.value), "conn": conn.value, "min_pix": min_pix.value, "labels": lab}

    def keep_free(self, keep):
        self._chk(self._L.sitrk_keep_free(self._h, int(keep)))

    def mesh_features_advect(self, keep_from, keep_to, mesh, jrec1, grid):
        """sitrk_mesh_features_advect, right after the step of jrec1: the map of slot keep_from carried by the cells of the mesh
        in slot `mesh` from their t0 draw to their t1 draw on the grid, into slot keep_to.  (ncells, ncarried): the cells that
        carry a label, the pixels that received one."""
        g = self._grid_arg(grid, "mesh_features_advect")
        ncells, ncarried = _i64(0), _i64(0)
        self._chk(self._L.sitrk_mesh_features_advect(self._h, int(keep_from), int(keep_to), int(mesh), int(jrec1), *g, C.byref(ncells),
                                                     C.byref(ncarried)))
        return ncells.value, ncarried.value

    def features_match(self, keepA, keepB, reach=0, dj=0, di=0, maxpair=1 << 20):
        """sitrk_features_match: {"pairs": (rows, 3) int64 rows (a, b, count) in ascending (a, b), at most maxpair of them,
        "npair": all such rows, "nhit": the pixels of A that meet a feature of B} of the kept maps keepA and keepB, B read at
        the shift (dj, di) and within `reach` pixels"""
        maxpair = int(maxpair)
        pairs = np.zeros((max(maxpair, 0), 3), dtype=np.int64)
        npair, nhit = _i64(0), _i64(0)
        self._chk(self._L.sitrk_features_match(self._h, int(keepA), int(keepB), int(dj), int(di), int(reach), maxpair,
                                               _ptr(pairs) if maxpair > 0 else None, C.byref(npair), C.byref(nhit)))
        return {"pairs": pairs[:min(npair.value, pairs.shape[0])], "npair": npair.value, "nhit": nhit.value}

    def match_kernel_ms(self):
        """(emit_ms, sort_ms, rows_ms): GPU time of the phases of the last features_match (sitrk_match_kernel_ms)"""
        v = [C.c_float(0) for _ in range(3)]
        self._chk(self._L.sitrk_match_kernel_ms(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def advect_kernel_ms(self):
        """advect_ms: GPU time of the kernels of the last mesh_features_advect behind its two rasters (sitrk_advect_kernel_ms)"""
        v = C.c_float(0)
        self._chk(self._L.sitrk_advect_kernel_ms(self._h, C.byref(v)))
        return v.value

    # -- skeletons of a label map (sitrk_skeleton_raster, sitrk_keep_skeleton)
    def _skeleton_call(self, fn, head, shape, max_sub, maxfeat, maxnode, skel):
        maxfeat, maxnode = int(maxfeat), int(maxnode)
        table = np.zeros((max(maxfeat, 0), SKEL_NCOLS), dtype=np.int64)
        nodes = np.zeros((max(maxnode, 0), 3), dtype=np.int64)
        sk = np.empty(shape, dtype=np.int8) if skel else None
        nfeat, nnode, nskel, nsub, conv = _i64(0), _i64(0), _i64(0), _int(0), _int(0)
        self._chk(fn(self._h, *head, int(max_sub), maxfeat, maxnode, _ptr(sk), _ptr(table) if maxfeat > 0 else None,
                     _ptr(nodes) if maxnode > 0 else None, C.byref(nfeat), C.byref(nnode), C.byref(nskel), C.byref(nsub), C.byref(conv)))
        return {"table": table[:min(nfeat.value, table.shape[0])], "nodes": nodes[:min(nnode.value, nodes.shape[0])],
                "nfeat": nfeat.value, "nnode": nnode.value, "nskel": nskel.value, "nsub": nsub.value, "converged": conv.value,
                "skel": sk}

    def skeleton_raster(self, map, max_sub=4096, maxfeat=65536, maxnode=1 << 20, skel=True):
        """sitrk_skeleton_raster: the mask map >= 0 of the host label map (ny,nx), every value -1 or in [0, ny*nx), thinned by at
        most max_sub sub-iterations of Guo and Hall's algorithm.  A dict with table (rows, 7) int64 under the names SKEL_COLS --
        one row per distinct label in ascending order, the first maxfeat of them --, nodes (rows, 3) int64 rows (p, label, X) of
        the skeleton pixels with X != 2 in ascending p, the first maxnode of them, the counts nfeat, nnode, nskel, nsub,
        converged, and skel: (ny,nx) int8, None with skel=False."""
        a = np.asarray(map)
        if a.ndim != 2 or a.dtype.kind not in "iu":
            raise ValueError("skeleton_raster: map must be an (ny, nx) array of integers, got %s %s" % (a.shape, a.dtype))
        ny, nx = a.shape
        if not (ny < 2 ** 31 and nx < 2 ** 31):
            raise ValueError("skeleton_raster: ny and nx must fit int32, got %d, %d" % (ny, nx))
        if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise IndexError("skeleton_raster: a value of the map does not fit int32")
        a = as_c(a, np.int32)
        return self._skeleton_call(self._L.sitrk_skeleton_raster, (ny, nx, _ptr(a)), (ny, nx), max_sub, maxfeat, maxnode, skel)

    def keep_skeleton(self, keep, max_sub=4096, maxfeat=65536, maxnode=1 << 20, skel=False):
        """sitrk_keep_skeleton: skeleton_raster() of the kept map of slot `keep`, which stays on the device and as it was; the
        same dict"""
        shape = self.keep_get(keep, labels=False)["shape"] if skel else None
        return self._skeleton_call(self._L.sitrk_keep_skeleton, (int(keep),), shape, max_sub, maxfeat, maxnode, skel)

    def skeleton_kernel_ms(self):
        """(thin_ms, table_ms, nodes_ms): GPU time of the phases of the last skeleton call (sitrk_skeleton_kernel_ms)"""
        v = [C.c_float(0) for _ in range(3)]
        self._chk(self._L.sitrk_skeleton_kernel_ms(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    # -- distribution of values (sitrk_dist_*)
    @staticmethod
    def _dist_args(edges, q):
        e = None if edges is None else as_c(edges, np.float64)
        qq = None if q is None else as_c(q, np.float64)
        if e is not None and (e.ndim != 1 or e.shape[0] < 2):
            raise ValueError("edges must be the (nb + 1,) edges of nb >= 1 bins or None, got shape %s" % (e.shape,))
        if qq is not None and qq.ndim != 1:
            raise ValueError("q must be a (nq,) array or None, got shape %s" % (qq.shape,))
        nb = 0 if e is None else e.shape[0] - 1
        nq = 0 if qq is None else qq.shape[0]
        counts = np.zeros(nb + 2 if nb else 0, dtype=np.int64)
        qval, qrank = np.full(nq, np.nan, dtype=np.float64), np.full(nq, -1, dtype=np.int64)
        return e, qq, nb, nq, counts, qval, qrank

    @staticmethod
    def _dist_result(e, qq, nb, nq, counts, qval, qrank, m, nnan):
        return {"counts": counts if nb else None, "edges": e, "q": qq if nq else None, "values": qval, "ranks": qrank,
                "m": m.value, "nnan": nnan.value}

    def dist_values(self, x, edges=None, q=None, use=None):
        """sitrk_dist_values: the distribution of the values x (n,) fp64 whose `use` (n,) is not 0 (None: all), NaNs aside.  A
        dict with counts (nb + 2,) int64 -- counts[c] = the values with exactly c of the edges (nb + 1,) <= v; None without
        edges --, edges, q, values (nq,) -- the value at rank min(m - 1, floor(q*m)) of the ascending sample, one of its values
        bit for bit --, ranks (nq,) int64, m the sample's size and nnan the NaNs left out."""
        x = as_c(x, np.float64)
        if x.ndim != 1:
            raise ValueError("x must be a (n,) array, got shape %s" % (x.shape,))
        n = x.shape[0]
        u = None if use is None else as_c(np.asarray(use) != 0, np.int8, (n,), "use")
        a = self._dist_args(edges, q)
        e, qq, nb, nq, counts, qval, qrank = a
        m, nnan = _i64(0), _i64(0)
        self._chk(self._L.sitrk_dist_values(self._h, n, _ptr(x) if n else None, _ptr(u) if n else None, nb, _ptr(e),
                                            _ptr(counts) if nb else None, nq, _ptr(qq) if nq else None, _ptr(qval) if nq else None,
                                            _ptr(qrank) if nq else None, C.byref(m), C.byref(nnan)))
        return self._dist_result(*a, m, nnan)

    def mesh_dist(self, mesh, jrec1, what, sgn=1, edges=None, q=None):
        """sitrk_mesh_dist, right after the step of jrec1: like dist_values() on the status-1 cells of the mesh in slot `mesh`;
        what = 0 div, 1 shr, 2 vor (or those names) taken as f, -f, |f| for sgn = +1, -1, 0, or 3 / "tot" = div*div + shr*shr.
        No per-cell value leaves the device."""
        what = DIST_WHAT.get(what, what)
        a = self._dist_args(edges, q)
        e, qq, nb, nq, counts, qval, qrank = a
        m, nnan = _i64(0), _i64(0)
        self._chk(self._L.sitrk_mesh_dist(self._h, int(mesh), int(jrec1), int(what), int(sgn), nb, _ptr(e),
                                          _ptr(counts) if nb else None, nq, _ptr(qq) if nq else None, _ptr(qval) if nq else None,
                                          _ptr(qrank) if nq else None, C.byref(m), C.byref(nnan)))
        return self._dist_result(*a, m, nnan)

    def dist_kernel_ms(self):
        """(keys_ms, hist_ms, select_ms): GPU time of the phases of the last distribution call (sitrk_dist_kernel_ms)"""
        v = [C.c_float(0) for _ in range(3)]
        self._chk(self._L.sitrk_dist_kernel_ms(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def dist_stats(self):
        """(passes, top_pass_ms): the digit passes the selection of the last distribution call ran and the GPU time of the first
        of them (sitrk_dist_stats)"""
        n, t = _int(0), C.c_float(0)
        self._chk(self._L.sitrk_dist_stats(self._h, C.byref(n), C.byref(t)))
        return n.value, t.value

    # -- dispersion of buoy pairs (sitrk_pairs_*)
    @staticmethod
    def _edges_arg(edges_km):
        """(nc + 1,) float64, C-contiguous; the library checks the values"""
        e = as_c(edges_km, np.float64)
        if e.ndim != 1 or e.shape[0] < 2:
            raise ValueError("edges_km: expected a 1-D array of at least two values, got shape %s" % (e.shape,))
        return e

    def pairs_points(self, yx0, yx1, edges_km, mask0=None, mask1=None):
        """sitrk_pairs_points: every unordered pair of valid points of yx0, yx1 (nP,2) km whose t0 separation lies in a class
        [edges_km[c], edges_km[c+1]).  A dict with table (nc, 7) fp64 under the names PAIRS_COLS and npts, the valid points.
        mask0 / mask1 (nP): 0 = not valid."""
        yx0 = as_c(yx0, np.float64)
        nP = yx0.shape[0]
        yx0 = as_c(yx0, np.float64, (nP, 2), "yx0")
        yx1 = as_c(yx1, np.float64, (nP, 2), "yx1")
        m0 = None if mask0 is None else as_c(np.asarray(mask0) != 0, np.int8, (nP,), "mask0")
        m1 = None if mask1 is None else as_c(np.asarray(mask1) != 0, np.int8, (nP,), "mask1")
        e = self._edges_arg(edges_km)
        nc = e.shape[0] - 1
        table = np.zeros((nc, PAIRS_NCOLS), dtype=np.float64)
        npts = _i64(0)
        self._chk(self._L.sitrk_pairs_points(self._h, nP, _ptr(yx0), _ptr(yx1), _ptr(m0), _ptr(m1), nc, _ptr(e), _ptr(table),
                                             C.byref(npts)))
        return {"table": table, "npts": npts.value}

    def pairs_mark(self, jrec0, mask=None):
        """sitrk_pairs_mark: snapshot every buoy's position and validity (alive now, mask byte not 0) on the device; jrec0 = the
        model record stepped next"""
        m = None if mask is None else as_c(np.asarray(mask) != 0, np.int8, (self.nP,), "mask")
        self._chk(self._L.sitrk_pairs_mark(self._h, int(jrec0), _ptr(m)))

    def pairs_since_mark(self, jrec1, edges_km):
        """sitrk_pairs_since_mark, right after the step of jrec1: like pairs_points() between the mark and now, no position
        leaving the device"""
        e = self._edges_arg(edges_km)
        nc = e.shape[0] - 1
        table = np.zeros((nc, PAIRS_NCOLS), dtype=np.float64)
        npts = _i64(0)
        self._chk(self._L.sitrk_pairs_since_mark(self._h, int(jrec1), nc, _ptr(e), _ptr(table), C.byref(npts)))
        return {"table": table, "npts": npts.value}

    def pairs_free(self):
        """sitrk_pairs_free: drop the snapshot of pairs_mark()"""
        self._chk(self._L.sitrk_pairs_free(self._h))

    def pairs_kernel_ms(self):
        """(bin_ms, pairs_ms, table_ms): GPU time of the phases of the last pair-dispersion table (sitrk_pairs_kernel_ms)"""
        v = [C.c_float(0) for _ in range(3)]
        self._chk(self._L.sitrk_pairs_kernel_ms(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def pairs_stats(self):
        """the pairs whose t0 separation the last table's pairs kernel formed, all class passes together (sitrk_pairs_stats)"""
        a = _i64(0)
        self._chk(self._L.sitrk_pairs_stats(self._h, C.byref(a)))
        return a.value

    # -- distance to the model coastline (sitrk_coast_*)
    def coast_build(self, Yf=None, Xf=None, tmask=None):
        """sitrk_coast_build: (nseg, ndropped).  Yf, Xf (Nj,Ni) km and tmask (Nj,Ni), or none of them: the grid of set_grid().
        The bin side is the knob set_tuning(coast_bin=...) at this call."""
        given = [a is not None for a in (Yf, Xf, tmask)]
        nseg, ndrop = _i64(0), _i64(0)
        if not any(given):
            self._chk(self._L.sitrk_coast_build(self._h, 0, 0, None, None, None, C.byref(nseg), C.byref(ndrop)))
        else:
            if not all(given):
                raise ValueError("coast_build: Yf, Xf and tmask go together")
            Yf = as_c(Yf, np.float64)
            if Yf.ndim != 2:
                raise ValueError("coast_build: Yf must be (Nj,Ni)")
            Nj, Ni = Yf.shape
            Xf = as_c(Xf, np.float64, (Nj, Ni), "Xf")
            tm = as_c(tmask, np.int8, (Nj, Ni), "tmask")
            self._chk(self._L.sitrk_coast_build(self._h, Nj, Ni, _ptr(Yf), _ptr(Xf), _ptr(tm), C.byref(nseg), C.byref(ndrop)))
        return nseg.value, ndrop.value

    def coast_segments(self):
        """sitrk_coast_segments: (ids (n,) int32, ab (n,2,2) = [a|b][y,x] km) in id order"""
        n = _i64(0)
        self._chk(self._L.sitrk_coast_segments(self._h, 0, None, None, C.byref(n)))
        ids = np.empty(n.value, dtype=np.int32)
        ab = np.empty((n.value, 2, 2), dtype=np.float64)
        if n.value:
            self._chk(self._L.sitrk_coast_segments(self._h, n.value, _ptr(ids), _ptr(ab), C.byref(n)))
        return ids, ab

    @staticmethod
    def _coast_rmax(rmax_km):
        return 0.0 if rmax_km is None else float(rmax_km)

    def coast_dist(self, yx, rmax_km=None, want_seg=True):
        """sitrk_coast_dist: (dist (n,) km, seg (n,) int32 or None) of the points yx (n,2) [y,x] km; rmax_km None = unbounded"""
        yx = as_c(yx, np.float64)
        if yx.ndim != 2 or yx.shape[1] != 2:
            raise ValueError("coast_dist: yx must be (n,2)")
        n = yx.shape[0]
        dist = np.empty(n, dtype=np.float64)
        seg = np.empty(n, dtype=np.int32) if want_seg else None
        self._chk(self._L.sitrk_coast_dist(self._h, n, _ptr(yx), self._coast_rmax(rmax_km), _ptr(dist), _ptr(seg)))
        return dist, seg

    def coast_dist_buoys(self, rmax_km=None, want_seg=True):
        """sitrk_coast_dist_buoys: the same for every buoy of set_buoys() at its current position, in the caller's order"""
        dist = np.empty(self.nP, dtype=np.float64)
        seg = np.empty(self.nP, dtype=np.int32) if want_seg else None
        self._chk(self._L.sitrk_coast_dist_buoys(self._h, self._coast_rmax(rmax_km), _ptr(dist), _ptr(seg)))
        return dist, seg

    def coast_kernel_ms(self):
        """GPU time [ms] of the query kernel of the last coast_dist / coast_dist_buoys (sitrk_coast_kernel_ms)"""
        a = C.c_float(0)
        self._chk(self._L.sitrk_coast_kernel_ms(self._h, C.byref(a)))
        return a.value

    def count_alive(self):
        n = _i64(0)
        self._chk(self._L.sitrk_count_alive(self._h, C.byref(n)))
        return n.value

    # -- locate / projection
    def find_cells(self, yx, jiT_guess):
        yx = as_c(yx, np.float64)
        n = yx.shape[0]
        g = as_c(jiT_guess, np.int32, (n, 2), "jiT_guess")
        out = np.empty((n, 2), dtype=np.int32)
        found = np.empty(n, dtype=np.int8)
        self._chk(self._L.sitrk_find_cells(self._h, n, _ptr(yx), _ptr(g), _ptr(out), _ptr(found)))
        return found.astype(bool), out

    def seed_init(self, latlon, yx, latT, lonT, resolkm, sic):
        latlon = as_c(latlon, np.float64)
        nP = latlon.shape[0]
        yx = as_c(yx, np.float64, (nP, 2), "pSC")
        shp = (self.Nj, self.Ni)
        latT = as_c(latT, np.float64, shp, "latT")
        lonT = as_c(lonT, np.float64, shp, "lonT")
        res = None if resolkm is None else as_c(resolkm, np.float64, shp, "resolkm")
        sic = as_c(sic, np.float64, shp, "sic")
        jiT = np.zeros((nP, 2), dtype=np.int32)
        keep = np.zeros(nP, dtype=np.int8)
        why = np.zeros(nP, dtype=np.int8)
        self._chk(self._L.sitrk_seed_init(self._h, nP, _ptr(latlon), _ptr(yx), _ptr(latT), _ptr(lonT), _ptr(res), _ptr(sic),
                                          _ptr(jiT), _ptr(keep), _ptr(why)))
        return jiT, keep, why

    def nemo_seed(self, tmask, latT, lonT, sic, khss=1, rmask=None, latF=None, lonF=None, lat0=70., lon0=-45.):
        """sitrk_nemo_seed: (latlon (n,2), yx (n,2) km, nT, nF) -- T-seeds first, then F-seeds, each in C order."""
        tm = as_c(tmask, np.int8)
        Nj, Ni = tm.shape
        shp = (Nj, Ni)
        la, lo, ic = (as_c(x, np.float64, shp, n) for x, n in ((latT, "latT"), (lonT, "lonT"), (sic, "sic")))
        rm = None if rmask is None else as_c(rmask, np.int8, shp, "rmask")
        lf = None if latF is None else as_c(latF, np.float64, shp, "latF")
        of = None if lonF is None else as_c(lonF, np.float64, shp, "lonF")
        nT, nF = _i64(0), _i64(0)
        args = (self._h, Nj, Ni, int(khss), _ptr(tm), _ptr(rm), _ptr(la), _ptr(lo), _ptr(ic), _ptr(lf), _ptr(of), float(lat0), float(lon0))
        self._chk(self._L.sitrk_nemo_seed(*args, 0, None, None, C.byref(nT), C.byref(nF)))
        n = nT.value + nF.value
        ll = np.empty((n, 2), dtype=np.float64)
        yx = np.empty((n, 2), dtype=np.float64)
        if n:
            self._chk(self._L.sitrk_nemo_seed(*args, n, _ptr(ll), _ptr(yx), C.byref(nT), C.byref(nF)))
        return ll, yx, nT.value, nF.value

    def subsample_cloud(self, yx, rd_km):
        """sitrk_subsample_cloud: (keep (n,) bool, launches) -- point i kept iff no kept j < i lies closer than rd_km
        (squared distance < rd_km**2 in fp64, no FMA): gudhi's sparsify_point_set on yx (n,2) km in the given order."""
        yx = as_c(yx, np.float64)
        if yx.ndim != 2 or yx.shape[1] != 2:
            raise ValueError("subsample_cloud: yx must be (n,2)")
        n = yx.shape[0]
        keep = np.zeros(n, dtype=np.int8)
        nk, nl = _i64(0), C.c_int32(0)
        self._chk(self._L.sitrk_subsample_cloud(self._h, n, _ptr(yx), float(rd_km), _ptr(keep), C.byref(nk), C.byref(nl)))
        return keep.astype(bool), nl.value

    def _cloud_args(self, lat, lon, valid, name):
        lat = as_c(lat, np.float64)
        lon = as_c(lon, np.float64)
        if lat.ndim != 1 or lon.shape != lat.shape:
            raise ValueError("%s: lat and lon must be 1-D of one length" % name)
        if valid is not None:
            valid = as_c(np.asarray(valid) != 0, np.int8, lat.shape, name + ": valid")
        return lat, lon, valid

    def nearest_buoy(self, lat, lon, valid=None, rd_km=1.0):
        """sitrk_nearest_buoy: (nn (n,) int64, dmin (n,) km) -- the nearest other valid buoy by the reference Haversine
        (lowest index on ties) when it lies closer than rd_km, else -1 and +inf."""
        lat, lon, valid = self._cloud_args(lat, lon, valid, "nearest_buoy")
        n = lat.shape[0]
        nn = np.empty(n, dtype=np.int32)
        dmin = np.empty(n, dtype=np.float64)
        self._chk(self._L.sitrk_nearest_buoy(self._h, n, _ptr(lat), _ptr(lon), _ptr(valid), float(rd_km), _ptr(nn), _ptr(dmin)))
        return nn.astype(np.int64), dmin

    def cancel_too_close(self, lat, lon, valid, nrec_all, nrec_before, rd_km):
        """sitrk_cancel_too_close: (keep (n,) bool, nclose) -- the buoys CancelTooClose keeps at one record, given its
        positions, validity (None: all valid) and the per-buoy counts of valid records in all / before that record."""
        lat, lon, valid = self._cloud_args(lat, lon, valid, "cancel_too_close")
        n = lat.shape[0]
        nall = as_c(nrec_all, np.int32, (n,), "cancel_too_close: nrec_all")
        nbef = as_c(nrec_before, np.int32, (n,), "cancel_too_close: nrec_before")
        keep = np.zeros(n, dtype=np.int8)
        nk, nc = _i64(0), _i64(0)
        self._chk(self._L.sitrk_cancel_too_close(self._h, n, _ptr(lat), _ptr(lon), _ptr(valid), _ptr(nall), _ptr(nbef),
                                                 float(rd_km), _ptr(keep), C.byref(nk), C.byref(nc)))
        return keep.astype(bool), nc.value

    def nearest_point(self, latlon, latT, lonT, resolkm=None, rd_found_km=10., max_itr=5):
        """NearestPoint of the reference for an array of points: (ji (n,2) int32 with -1,-1 = not found, dmin km)."""
        latlon = as_c(latlon, np.float64)
        n = latlon.shape[0]
        latlon = as_c(latlon, np.float64, (n, 2), "latlon")
        latT = as_c(latT, np.float64, (self.Nj, self.Ni), "latT")
        lonT = as_c(lonT, np.float64, (self.Nj, self.Ni), "lonT")
        res = None if resolkm is None else as_c(resolkm, np.float64, (self.Nj, self.Ni), "resolkm")
        ji = np.empty((n, 2), dtype=np.int32)
        dmin = np.empty(n, dtype=np.float64)
        self._chk(self._L.sitrk_nearest_point(self._h, n, _ptr(latlon), _ptr(latT), _ptr(lonT), _ptr(res), float(rd_found_km),
                                              int(max_itr), _ptr(ji), _ptr(dmin)))
        return ji, dmin

    def eval_haversine(self, plat, plon, xlat, xlon):
        plat, plon, xlat, xlon = (np.ascontiguousarray(a, dtype=np.float64) for a in np.broadcast_arrays(plat, plon, xlat, xlon))
        out = np.empty(plat.shape, dtype=np.float64)
        self._chk(self._L.sitrk_eval_haversine(self._h, plat.size, _ptr(plat), _ptr(plon), _ptr(xlat), _ptr(xlon), _ptr(out)))
        return out

    # -- predicate probes (parity tests)
    def eval_inside(self, pts, quads):
        pts = as_c(pts, np.float64)
        n = pts.shape[0]
        quads = as_c(quads, np.float64, (n, 4, 2), "quads")
        out = np.empty(n, dtype=np.int8)
        self._chk(self._L.sitrk_eval_inside(self._h, n, _ptr(pts), _ptr(quads), _ptr(out)))
        if (out & 2).any():
            raise SitrkError("eval_inside: the division-free cell test and the plain one disagree for %d point(s), first at %d"
                             % (int((out & 2).astype(bool).sum()), int(np.flatnonzero(out & 2)[0])))
        return out.astype(bool)

    def eval_euler(self, r, vel, rdt=3600.):
        r = as_c(r, np.float64)
        vel = as_c(vel, np.float64, r.shape, "vel")
        out = np.empty_like(r)
        self._chk(self._L.sitrk_eval_euler(self._h, r.size, _ptr(r), _ptr(vel), float(rdt), _ptr(out)))
        return out

    def eval_intersect(self, segs):
        segs = as_c(segs, np.float64)
        n = segs.shape[0]
        segs = as_c(segs, np.float64, (n, 4, 2), "segs")
        inter = np.empty(n, dtype=np.int8)
        ccw = np.empty(n, dtype=np.int8)
        self._chk(self._L.sitrk_eval_intersect(self._h, n, _ptr(segs), _ptr(inter), _ptr(ccw)))
        return inter.astype(bool), ccw.astype(bool)

    def eval_crossing(self, P1, P2, jiT):
        P1 = as_c(P1, np.float64)
        n = P1.shape[0]
        P2 = as_c(P2, np.float64, (n, 2), "P2")
        ji = as_c(jiT, np.int32, (n, 2), "jiT")
        out = np.empty((n, 2), dtype=np.int32)
        codes = np.empty((n, 2), dtype=np.int32)
        self._chk(self._L.sitrk_eval_crossing(self._h, n, _ptr(P1), _ptr(P2), _ptr(ji), _ptr(out), _ptr(codes)))
        return out, codes[:, 0], codes[:, 1]

    def survive_mask(self, sic):
        sic = as_c(sic, np.float64, (self.Nj, self.Ni), "sic")
        out = np.empty((self.Nj, self.Ni), dtype=np.int8)
        self._chk(self._L.sitrk_survive_mask(self._h, _ptr(sic), _ptr(out)))
        return out

    def cart2geo(self, yx, lat0=70., lon0=-45.):
        yx = as_c(yx, np.float64)
        out = np.empty_like(yx)
        self._chk(self._L.sitrk_cart2geo(self._h, yx.shape[0], _ptr(yx), float(lat0), float(lon0), _ptr(out)))
        return out

    def geo2cart(self, latlon, lat0=70., lon0=-45.):
        g = as_c(latlon, np.float64)
        out = np.empty_like(g)
        self._chk(self._L.sitrk_geo2cart(self._h, g.shape[0], _ptr(g), float(lat0), float(lon0), _ptr(out)))
        return out

    # -- measurement
    def timer_start(self):
        self._chk(self._L.sitrk_timer_start(self._h))

    def timer_stop(self):
        ms = C.c_float(0)
        self._chk(self._L.sitrk_timer_stop(self._h, C.byref(ms)))
        return ms.value
