"""Snapshot files read by the library's own reader (bl_snapshot_open): Athena++ .athdf.

Mirrors what the reference's main() does with SimulationReader (src/blacklight.cpp:93, :181-186):
construct from the input parameters, Read(snapshot), hand the arrays to the radiation integrator.
"""
import ctypes as C

import numpy as np

from . import _capi
from .params import Params


class Snapshot:
    """One file of the run: `Snapshot(params, snapshot=0)`; pass it to Context.set_grid(). `file_number`: that file of a
    numbered series instead (bl_snapshot_open_number - what the slow-light window reads, simulation_reader.cpp:225-232)."""

    def __init__(self, params: Params, snapshot: int = 0, file_number: int = None, raw: bool = False):
        L = _capi.lib()
        self._lib = L
        self._params = params   # keeps simulation_kappa_name etc. alive
        self.raw = bool(raw)
        handle = C.c_void_p()
        err = C.create_string_buffer(1024)
        if raw:   # (simulation_format = iharm3d: the header and the file's prims as they lie - harm_header, harm_prims())
            if file_number is None:
                file_number = int(params.get("simulation_start")) + int(snapshot) if params.get("simulation_multiple") else -1
            rc = L.bl_snapshot_open_raw(params.ptr, int(file_number), C.byref(handle), err, len(err))
        elif file_number is None:
            rc = L.bl_snapshot_open(params.ptr, int(snapshot), C.byref(handle), err, len(err))
        else:
            rc = L.bl_snapshot_open_number(params.ptr, int(file_number), C.byref(handle), err, len(err))
        if rc != 0:
            raise _capi.BlacklightError(rc, err.value.decode())
        self._h = handle

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bl_snapshot_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def desc(self):
        """bl_grid_desc view of the arrays this object owns (valid until close())."""
        return self._lib.bl_snapshot_grid(self._h).contents

    @property
    def time(self):
        return self._lib.bl_snapshot_time(self._h)

    @property
    def warnings(self):
        return self._lib.bl_snapshot_warnings(self._h).decode()

    @property
    def file(self):
        return self._lib.bl_snapshot_file(self._h).decode()

    @property
    def blocks(self):
        """(levels [n_b], logical locations [n_b][3]) of the MeshBlocks."""
        levels = C.POINTER(C.c_int32)()
        locations = C.POINTER(C.c_int32)()
        n = self._lib.bl_snapshot_blocks(self._h, C.byref(levels), C.byref(locations))
        return (np.ctypeslib.as_array(levels, (n,)).copy(), np.ctypeslib.as_array(locations, (n, 3)).copy())

    @property
    def harm_header(self):
        """raw=True: the file's header as a _capi.HarmHeader (bl_harm_header) - what HarmGrid takes."""
        header = _capi.HarmHeader()
        rc = self._lib.bl_snapshot_harm_header(self._h, C.byref(header))
        if rc != 0:
            raise _capi.BlacklightError(rc, "Error: the snapshot was not opened with raw=True.")
        return header

    def harm_prims(self):
        """raw=True: a copy of the file's prims as they lie, float32 [n1][n2][n3][n_prim]."""
        h = self.harm_header
        ptr = self._lib.bl_snapshot_harm_prims(self._h)
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), (h.n1, h.n2, h.n3, h.n_prim)).copy()

    def arrays(self):
        """Copies of the arrays as numpy: prim [n_var][n_b][n_k][n_j][n_i] float32 and the six coordinate
        arrays [n_b][...] float64, plus the variable indices."""
        d = self.desc()
        shape = (d.n_var, d.n_blocks, d.n_k, d.n_j, d.n_i)
        out = {"prim": np.ctypeslib.as_array(C.cast(d.prim, C.POINTER(C.c_float)), shape).copy()}
        for name, n in (("x1f", d.n_i + 1), ("x2f", d.n_j + 1), ("x3f", d.n_k + 1), ("x1v", d.n_i), ("x2v", d.n_j),
                        ("x3v", d.n_k)):
            out[name] = np.ctypeslib.as_array(C.cast(getattr(d, name), C.POINTER(C.c_double)), (d.n_blocks, n)).copy()
        out["indices"] = {k: getattr(d, k) for k in ("ind_rho", "ind_pgas", "ind_kappa", "ind_uu1", "ind_uu2", "ind_uu3",
                                                      "ind_bb1", "ind_bb2", "ind_bb3")}
        return out


class HarmGrid:
    """The grid of an iharm3d-family header under `params` (bl_harm_grid): coordinates, for simulation_coord = fmks the bounds and the
    look-up table (built when desc() is first called), the variable and adiabatic indices, and the table of per-point factors of the
    primitive conversion. header: a _capi.HarmHeader (Snapshot(params, raw=True).harm_header, or filled in by the caller). Pass it to
    Context.set_grid_device_harm / harm_convert_device together with prims[n1][n2][n3][n_prim] in device memory, or convert on the
    host with convert_host()."""

    def __init__(self, params: Params, header):
        L = _capi.lib()
        self._lib = L
        self._params = params
        self.header = _capi.HarmHeader.from_buffer_copy(header)   # (a copy, as the library keeps one: the caller's struct may change)
        handle = C.c_void_p()
        err = C.create_string_buffer(1024)
        rc = L.bl_harm_grid_create(params.ptr, C.byref(self.header), C.byref(handle), err, len(err))
        if rc != 0:
            raise _capi.BlacklightError(rc, err.value.decode())
        self._h = handle

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bl_harm_grid_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @property
    def warnings(self):
        return self._lib.bl_harm_grid_warnings(self._h).decode()

    @property
    def planes(self):
        """Planes the conversion writes: 8, or 9 with plasma_model = code_kappa (the entropy last)."""
        return int(self._lib.bl_harm_grid_planes(self._h))

    @property
    def shape(self):
        h = self.header
        return (h.n1, h.n2, h.n3, h.n_prim)

    def desc(self, converted=False):
        """bl_grid_desc (valid until close()): converted=False - the header's variable indices, for set_grid_device_harm;
        converted=True - indices 0 ... 7 (8), for the planes convert_host / harm_convert_device write."""
        return self._lib.bl_harm_grid_desc(self._h, 1 if converted else 0).contents

    def convert_host(self, prims):
        """prims float32 [n1][n2][n3][n_prim] -> float32 [planes][n3][n2][n1]: rho, pgas, uu1..3, bb1..3 (, kappa) as the reader makes them."""
        prims = np.ascontiguousarray(prims, dtype=np.float32)
        if prims.shape != self.shape:
            raise ValueError(f"prims has shape {prims.shape}, the header says {self.shape}")
        h = self.header
        out = np.empty((self.planes, h.n3, h.n2, h.n1), dtype=np.float32)
        rc = self._lib.bl_harm_convert_host(self._h, prims.ctypes.data, out.ctypes.data)
        if rc != 0:
            raise _capi.BlacklightError(rc, "Error: bl_harm_convert_host refused its arguments.")
        return out
