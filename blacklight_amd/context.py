"""Host-side driver object over the C-ABI (bl_init / bl_set_grid / bl_render).

Mirrors how the reference's main() drives the hot path (src/blacklight.cpp:93-94, 178-233):
construct once from the input parameters, hand over the grid once per snapshot, render one adaptive
level per call. All computation happens in libblacklight_amd.so on the GPU.
"""
import ctypes as C
import math

import numpy as np

from . import _capi
from .params import Params


class Context:
    def __init__(self, params: Params, device: int = -1):
        L = _capi.lib()
        self._lib = L
        self.params = params
        handle = C.c_void_p()
        rc = L.bl_init(params.ptr, device, C.byref(handle))
        if rc != 0:
            raise _capi.BlacklightError(rc, L.bl_last_global_error().decode())
        self._ctx = handle
        self._grid_keepalive = None
        self.resolution = int(params.get("camera_resolution"))
        if getattr(params, "has_sweep", False):   # sweep_* keys of the .input grammar: the same call the command-line driver makes
            try:
                self.apply_sweep(params)
            except Exception:
                self.close()
                raise

    @classmethod
    def from_input(cls, path, device: int = -1):
        """A context from a .input file, its sweep keys applied (what bin/blacklight_amd sets up); .params.num_runs counts the snapshots."""
        return cls(Params.from_file(path), device=device)

    def apply_sweep(self, params=None):
        """bl_apply_sweep_all: the sweep_rat_low / sweep_rat_high / sweep_rho_cgs lists of `params` (default: this context's) as electron
        models and density units, or as polarized triples (with the electron lists: tuples), its sweep_cut_sigma_max list as sigma cuts
        its sweep_camera_th / sweep_camera_ph lists as cameras and its sweep_frequency list as frequencies - all of them or, where one
        is refused, none. An empty sweep changes nothing."""
        params = params or self.params
        if params.has_sweep:
            self._check(self._lib.bl_apply_sweep_all(self._ctx, C.byref(params.sweep_all)))

    @property
    def num_variants(self):
        """Images one render produces (bl_num_variants): electron mixes x models x units x sigma cuts, or polarized triples."""
        return self._lib.bl_num_variants(self._ctx)

    def _variants(self):
        """What the context renders (bl_variants_get), the one record of it: the columns rat_low, rat_high, rho_cgs, sigma_max over the
        images in row order - model-major, then unit, then cut, or the triples - and the flags (1: the triples carry their own cuts,
        2: their own electron mixes)."""
        n = self.num_variants
        columns, flags = np.zeros((4, n)), C.c_int(0)
        self._check(self._lib.bl_variants_get(self._ctx, n, *(column.ctypes.data_as(C.c_void_p) for column in columns), C.byref(flags)))
        return columns.tolist(), flags.value

    def variant_output_path(self, snapshot=0, variant=0, camera=0, frequency=None):
        """The file name write_output(variant=..., camera=...) uses without `path` (bl_camera_output_path): output_file, the file number
        of a series, and in front of the extension a tag .mMMuUU (.mMMuUUsSS with sigma cuts set, .eEE in front with electron mixes set) / .vVV when the context renders
        several variants, with .cCC in front of it when it renders several cameras (image.c01m00u02.npz). frequency = l: the name
        write_output(frequency=l, ...) uses (bl_frequency_output_path), with the tag fFF after the camera's (image.c01f02m00u02.npz)."""
        buf = C.create_string_buffer(4096)
        if frequency is not None:
            self._check(self._lib.bl_frequency_output_path(self._ctx, int(snapshot), int(frequency), int(camera), int(variant), buf, len(buf)))
            return buf.value.decode()
        self._check(self._lib.bl_camera_output_path(self._ctx, int(snapshot), int(camera), int(variant), buf, len(buf)))
        return buf.value.decode()

    # ------------------------------------------------------------------ frequencies
    def set_frequencies(self, hz):
        """Render an explicit list of observing frequencies (Hz) in one render (bl_set_frequencies): a scalar or a sequence, in any
        order, each with the meaning of image_frequency; an empty sequence restores the parameter block's own list. The list's length
        is the context's frequency count from then on: frequencies, n_freq, num_quantities and the row offsets are those of a block
        with image_num_frequencies = len(hz), and row l of a quantity is what a context with hz[l] as its one image_frequency
        renders. Geodesics stay resident."""
        values = np.ascontiguousarray(np.atleast_1d(np.asarray(hz, dtype=np.float64)).ravel())
        self._check(self._lib.bl_set_frequencies(self._ctx, int(values.size), values.ctypes.data_as(C.c_void_p)))

    @property
    def num_frequencies(self):
        """The length of the list set_frequencies() set (bl_num_frequencies); 0 when the parameter block's own list is rendered."""
        return self._lib.bl_num_frequencies(self._ctx)

    @property
    def n_freq(self):
        """Frequencies a render carries: the list's length, else the parameter block's image_num_frequencies."""
        return self.num_frequencies or int(self.params.get("image_num_frequencies"))

    # ------------------------------------------------------------------ cameras
    def set_cameras(self, th, ph=None):
        """Render several cameras (viewing angles camera_th, camera_ph in degrees, as the .input file writes them) in one render
        (bl_set_cameras). Scalars or sequences, broadcast against each other; ph=None: 0 for every camera; an empty sequence clears
        them (the parameter block's camera again). With C cameras a full root-level render has C * res^2 rays, camera c's outputs are
        the slice camera_slice(c) of every per-ray array, and the geodesics of all cameras are integrated as one set of rays."""
        th, ph = np.broadcast_arrays(np.atleast_1d(np.asarray(th, dtype=np.float64)), np.atleast_1d(np.asarray(0.0 if ph is None else ph, dtype=np.float64)))
        th, ph = np.ascontiguousarray(th.ravel()), np.ascontiguousarray(ph.ravel())
        self._check(self._lib.bl_set_cameras(self._ctx, int(th.size), th.ctypes.data_as(C.c_void_p), ph.ctypes.data_as(C.c_void_p)))

    @property
    def cameras(self):
        """The (th, ph) pairs in degrees of the camera list (bl_cameras_get); [] when the parameter block's camera is rendered."""
        n = self.num_cameras
        th, ph = np.zeros(max(n, 1)), np.zeros(max(n, 1))
        self._check(self._lib.bl_cameras_get(self._ctx, n, th.ctypes.data_as(C.c_void_p), ph.ctypes.data_as(C.c_void_p)))
        return [(float(th[c]), float(ph[c])) for c in range(n)]

    @property
    def num_cameras(self):
        return self._lib.bl_num_cameras(self._ctx)

    def camera_slice(self, camera):
        """Where camera `camera` of the list lies in every per-ray output of a full root-level render: slice(c res^2, (c + 1) res^2)."""
        n = max(1, self.num_cameras)
        if not 0 <= int(camera) < n:
            raise IndexError(f"camera_slice: camera {camera} outside 0 .. {n - 1}")
        pixels = self.resolution * self.resolution
        return slice(int(camera) * pixels, (int(camera) + 1) * pixels)

    def camera_frame_of(self, camera):
        """The frame of camera `camera` of the list (bl_camera_frame_get_camera); with no list, camera 0 is the parameter block's."""
        frame = _capi.CameraFrame()
        rc = self._lib.bl_camera_frame_get_camera(self._ctx, int(camera), C.byref(frame))
        if rc != 0:
            raise IndexError(f"camera_frame_of: camera {camera} outside the list")
        return frame

    def close(self):
        if self._ctx:
            for ptr in self.__dict__.pop("_pinned", []):   # (arrays from pinned_array() end here: copy what is to outlive the context)
                self._lib.bl_host_free(self._ctx, ptr)
            self._lib.bl_free(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise _capi.BlacklightError(rc, self._lib.bl_last_error(self._ctx).decode())

    # ------------------------------------------------------------------ queries
    @property
    def num_quantities(self):
        return self._lib.bl_image_num_quantities(self._ctx)

    @property
    def num_render_images(self):
        return self._lib.bl_render_num_images(self._ctx)

    @property
    def camera_frame(self):
        frame = _capi.CameraFrame()
        self._check(self._lib.bl_camera_frame_get(self._ctx, C.byref(frame)))
        return frame

    @property
    def frequencies(self):
        out = np.zeros(self.n_freq)
        self._check(self._lib.bl_frequencies(self._ctx, out.ctypes.data_as(C.POINTER(C.c_double)), self.n_freq))
        return out

    @property
    def warnings(self):
        return self._lib.bl_warnings(self._ctx).decode()

    @property
    def stats(self):
        st = _capi.Stats()
        self._check(self._lib.bl_get_stats(self._ctx, C.byref(st)))
        return st

    def set_scratch_limit(self, nbytes):
        self._check(self._lib.bl_set_scratch_limit(self._ctx, int(nbytes)))

    def debug_math(self, op, x, y=None):
        """Apply device math function `op` (see bl_debug_math in the header) element-wise; returns float64 array."""
        import numpy as np
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.empty_like(x)
        yp = None
        if y is not None:
            y = np.ascontiguousarray(y, dtype=np.float64)
            yp = y.ctypes.data
        self._check(self._lib.bl_debug_math(self._ctx, int(op), x.size, x.ctypes.data, yp, out.ctypes.data))
        return out

    def debug_locate_angles(self, points, spin, x2f, x2v, x3f, x3v):
        """The tolerant locate step's theta and phi of `points` ([m, 3] Cartesian Kerr-Schild) against an angular lattice (faces and centres
        of theta and of phi), relative to the centre of the guessed cell ("local") and by acos / atan2 ("global"): bl_debug_math ops 40
        (spin 0) and 41. Returns {"local": ..., "global": ...}, each a dict of arrays over the points: cell_th, cell_ph (the anchor cells),
        frac_th, frac_ph, margin (the smallest signed distance to anything compared), undecided, guess_th, guess_ph."""
        import numpy as np
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        m = points.shape[0]
        lattice = np.concatenate([np.asarray(v, dtype=np.float64).ravel() for v in (x2f, x2v, x3f, x3v)])
        n_th, n_ph = np.asarray(x2v).size, np.asarray(x3v).size
        if lattice.size != 2 * (n_th + n_ph) + 2:
            raise ValueError("faces must hold one value more than centres")
        n = max(16 * m, lattice.size)
        x = np.zeros(n)
        x[:4] = (m, float(spin), n_th, n_ph)
        x[4:4 + 3 * m] = points.T.ravel()
        y = np.zeros(n)
        y[:lattice.size] = lattice
        rows = self.debug_math(40 if float(spin) == 0.0 else 41, x, y)[:16 * m].reshape(16, m)
        names = ("cell_th", "cell_ph", "frac_th", "frac_ph", "margin", "undecided", "guess_th", "guess_ph")
        out = {}
        for half, key in enumerate(("local", "global")):
            out[key] = {name: (rows[8 * half + q] if name.startswith(("frac", "margin")) else rows[8 * half + q].astype(np.int64))
                        for q, name in enumerate(names)}
        return out

    def set_undefined_policy(self, policy):
        """"refuse" (default), "edge" (samples where the reference reads past its arrays), "kappa" (unpolarized kappa-distribution
        electrons, whose absorptivity the reference computes from an uninitialised constant), or "edge,kappa" (bl_set_undefined_policy)."""
        flags = 0
        for word in str(policy).replace("|", ",").split(","):
            flags |= {"refuse": 0, "edge": 1, "kappa": 2}[word.strip()]
        self._check(self._lib.bl_set_undefined_policy(self._ctx, flags))

    def set_arithmetic(self, mode):
        """"tolerant" (what a context starts in unless BLACKLIGHT_AMD_ARITHMETIC=exact) or "exact" (bit-identical to the reference):
        the arithmetic tier (bl_set_arithmetic)."""
        self._check(self._lib.bl_set_arithmetic(self._ctx, {"exact": 0, "tolerant": 1}[mode]))

    def set_reproducible(self, on=True):
        """Tolerant tier: bit-reproducible images (one transfer record per sample instead of composed maps; bl_set_reproducible)."""
        self._check(self._lib.bl_set_reproducible(self._ctx, 1 if on else 0))

    def set_tail_policy(self, policy):
        """"auto" (default), "wide", "quad" or "split": who steps the rays a chunk waits for longest (bl_set_tail_policy)."""
        self._check(self._lib.bl_set_tail_policy(self._ctx, {"auto": 0, "wide": 1, "quad": 2, "split": 3}[policy]))

    def set_geodesic_reuse(self, on=True):
        """Geodesics once per series (default on): a root-level render of an unchanged camera shades the sample records the last one
        left in HBM instead of integrating its rays again (bl_set_geodesic_reuse; stats.geodesics_reused says which way it went). A frame of
        more than one chunk is kept from the second render of its camera on, in a record store beside one chunk's shading arrays (the scratch
        the first render allocated, re-partitioned): the third and later frames reuse. Located samples of such frames, and anything under set_overlap(True), are
        not kept."""
        self._check(self._lib.bl_set_geodesic_reuse(self._ctx, 1 if on else 0))

    def set_electron_models(self, rat_high, rat_low=1.0):
        """Render several electron-temperature models (R_high / R_low pairs) in one render (bl_set_electron_models). Scalars or
        sequences, broadcast against each other; an empty sequence clears them (the parameter block's pair again). The image then
        holds the models one after another (render()["image_by_model"]: (n_models, n_q, n_rays)); geodesics stay resident."""
        high, low = np.broadcast_arrays(np.atleast_1d(np.asarray(rat_high, dtype=np.float64)),
                                        np.atleast_1d(np.asarray(rat_low, dtype=np.float64)))
        high = np.ascontiguousarray(high)
        low = np.ascontiguousarray(low)
        self._check(self._lib.bl_set_electron_models(self._ctx, int(high.size), low.ctypes.data_as(C.c_void_p),
                                                     high.ctypes.data_as(C.c_void_p)))

    @property
    def electron_models(self):
        """The (rat_high, rat_low) pairs set_electron_models() set; [] when the parameter block's pair is rendered."""
        (low, high, _, _), _ = self._variants()
        stride = max(1, self.num_density_units) * max(1, self.num_sigma_cuts)
        return [(high[m * stride], low[m * stride]) for m in range(self.num_electron_models)]

    @property
    def num_electron_models(self):
        return self._lib.bl_num_electron_models(self._ctx)

    def set_density_units(self, rho_cgs):
        """Render several density units (simulation_rho_cgs values, g / cm^3) in one render (bl_set_density_units). A scalar or a
        sequence; an empty sequence clears them (the parameter block's unit again). The image then holds, for every electron model,
        its units one after another (render()["image_by_unit"]: (n_models, n_units, n_q, n_rays)); geodesics stay resident."""
        units = np.ascontiguousarray(np.atleast_1d(np.asarray(rho_cgs, dtype=np.float64)).ravel())
        self._check(self._lib.bl_set_density_units(self._ctx, int(units.size), units.ctypes.data_as(C.c_void_p)))

    @property
    def density_units(self):
        """The simulation_rho_cgs values set_density_units() set; [] when the parameter block's unit is rendered."""
        (_, _, rho, _), _ = self._variants()
        return [rho[u * max(1, self.num_sigma_cuts)] for u in range(self.num_density_units)]

    @property
    def num_density_units(self):
        return self._lib.bl_num_density_units(self._ctx)

    def set_sigma_cuts(self, sigma_max):
        """Render several sigma cuts (cut_sigma_max values: cells with sigma = b.b / rho above the value are left out, a negative
        value switches the cut off) in one render (bl_set_sigma_cuts). A scalar or a sequence; an empty sequence clears them (the
        parameter block's cut_sigma_max again). The image then holds, for every electron model and density unit, its cuts one after
        another (render()["image_by_cut"]: (n_models, n_units, n_cuts, n_q, n_rays)); geodesics stay resident."""
        cuts = np.ascontiguousarray(np.atleast_1d(np.asarray(sigma_max, dtype=np.float64)).ravel())
        self._check(self._lib.bl_set_sigma_cuts(self._ctx, int(cuts.size), cuts.ctypes.data_as(C.c_void_p)))

    @property
    def sigma_cuts(self):
        """The cut_sigma_max values set_sigma_cuts() set; [] when the parameter block's cut is rendered."""
        return self._variants()[0][3][:self.num_sigma_cuts]

    @property
    def num_sigma_cuts(self):
        return self._lib.bl_num_sigma_cuts(self._ctx)

    def set_electron_mixes(self, mixes):
        """Render several electron distributions of an unpolarized run - thermal plus power-law mixes - in one render
        (bl_set_electron_mixes): one mapping or a sequence of them with the keys power_frac, p, gamma_min, gamma_max; a missing key
        takes the parameter block's value. An empty sequence clears them (the parameter block's mix again). The mixes are the
        outermost axis of the image rows (render()["image_by_mix"]: (n_mixes, rows of one mix, n_rays)); geodesics stay resident."""
        given = [mixes] if hasattr(mixes, "keys") else list(mixes)
        own = self._block_electrons()
        array = (_capi.ElectronMix * max(1, len(given)))()
        for e, mapping in enumerate(given):
            unknown = set(mapping) - set(_capi.ELECTRON_MIX_KEYS)
            if unknown:
                raise ValueError(f"set_electron_mixes: unknown electron key(s) {sorted(unknown)}; the keys are {list(_capi.ELECTRON_MIX_KEYS)}")
            for key in _capi.ELECTRON_MIX_KEYS:
                setattr(array[e], key, float(mapping.get(key, own[key])))
        self._check(self._lib.bl_set_electron_mixes(self._ctx, len(given), C.cast(array, C.c_void_p)))

    @property
    def electron_mixes(self):
        """The mixes set_electron_mixes() set (bl_electron_mix_get), one mapping each; [] when the parameter block's mix is rendered."""
        out = []
        for e in range(self.num_electron_mixes):
            mix = _capi.ElectronMix()
            self._check(self._lib.bl_electron_mix_get(self._ctx, e, C.byref(mix)))
            out.append({key: getattr(mix, key) for key in _capi.ELECTRON_MIX_KEYS})
        return out

    @property
    def num_electron_mixes(self):
        return self._lib.bl_num_electron_mixes(self._ctx)

    def fit_density_unit(self, target_jy, distance_pc, lo, hi, frequency=0, rtol=1.0e-3, per_render=16):
        """The density unit (simulation_rho_cgs) in [lo, hi] at which the root image's total flux (flux.total_flux_jy) at image
        frequency `frequency` is target_jy to within rtol. Each step renders `per_render` units log-spaced over the bracket in one
        render - geodesics stay resident, so every render after the first is a shading stage only - and keeps the adjacent pair whose
        fluxes straddle the target. With several electron models set, each model is fitted in turn. The context's models and units
        are restored on exit. Returns (rho_cgs, flux_jy, renders): floats, or lists by model with several models."""
        from . import flux as _flux
        if self.num_cameras >= 2:
            raise ValueError("fit_density_unit sums one camera's image: not with two or more cameras (set_cameras)")
        if not (0.0 < lo < hi) or not np.isfinite(hi):
            raise ValueError(f"fit_density_unit needs 0 < lo < hi, finite (got {lo}, {hi})")
        if not 2 <= per_render <= 16:
            raise ValueError("fit_density_unit: 2 <= per_render <= 16 (BL_MAX_DENSITY_UNITS)")
        if not (target_jy > 0.0 and rtol > 0.0):
            raise ValueError("fit_density_unit needs target_jy > 0 and rtol > 0")
        models, units = self.electron_models, self.density_units
        renders = 0

        def fit_one():
            nonlocal renders
            a, b = float(lo), float(hi)
            for _ in range(64):
                trial = np.geomspace(a, b, per_render)
                trial[0], trial[-1] = a, b   # (the bracket's own ends, not their rounded logarithms)
                self.set_density_units(trial)
                got = self.render()
                renders += 1
                fluxes = np.array([_flux.total_flux_jy(got["image_by_unit"][0, u], self.params, distance_pc, frequency)
                                   for u in range(per_render)])
                best = int(np.nanargmin(np.abs(fluxes - target_jy))) if np.isfinite(fluxes).any() else -1
                if best >= 0 and abs(fluxes[best] - target_jy) <= rtol * target_jy:
                    return float(trial[best]), float(fluxes[best])
                straddle = [k for k in range(per_render - 1) if (fluxes[k] - target_jy) * (fluxes[k + 1] - target_jy) <= 0.0]
                if not straddle:
                    raise ValueError(f"fit_density_unit: [{a:.6g}, {b:.6g}] g/cm^3 does not bracket {target_jy:.6g} Jy "
                                     f"(fluxes found: {np.nanmin(fluxes):.6g} .. {np.nanmax(fluxes):.6g} Jy)")
                a, b = float(trial[straddle[0]]), float(trial[straddle[0] + 1])
            raise RuntimeError(f"fit_density_unit: no unit within rtol = {rtol} of {target_jy} Jy after {renders} renders")

        try:
            if len(models) >= 2:
                found = []
                for high, low in models:
                    self.set_electron_models(high, rat_low=low)
                    found.append(fit_one())
                return [u for u, _ in found], [f for _, f in found], renders
            rho, flux = fit_one()
            return rho, flux, renders
        finally:
            self.set_density_units([])
            self.set_electron_models([h for h, _ in models], rat_low=[lo_ for _, lo_ in models])
            self.set_density_units(units)

    def set_polarized_variants(self, rat_high, rho_cgs, rat_low=1.0, sigma_max=None, electrons=None):
        """Render several (R_high, R_low, simulation_rho_cgs) triples of a polarized run in one render (bl_set_polarized_variants):
        a list of triples, not a product - scalars or sequences, broadcast against each other; empty sequences clear them (the
        parameter block's pair and unit again). The image then holds the variants one after another
        (render()["image_by_variant"]: (n_variants, n_q, n_rays)); geodesics stay resident.
        sigma_max: a sigma cut for every variant (bl_set_polarized_variants_sigma) - a scalar, or one cut_sigma_max value per
        variant (a negative value switches the cut off); None: the parameter block's own cut_sigma_max for all of them.
        electrons: an electron distribution for every variant (bl_set_polarized_variants_electrons) - one mapping, or one per variant,
        with the keys power_frac, p, gamma_min, gamma_max, kappa_frac, kappa, w (the plasma_* keys without their prefix); a missing
        key means the parameter block's value. None: the parameter block's own distribution for all of them."""
        high, unit, low = np.broadcast_arrays(np.atleast_1d(np.asarray(rat_high, dtype=np.float64)),
                                              np.atleast_1d(np.asarray(rho_cgs, dtype=np.float64)),
                                              np.atleast_1d(np.asarray(rat_low, dtype=np.float64)))
        high, unit, low = (np.ascontiguousarray(a.ravel()) for a in (high, unit, low))
        cuts = None
        if sigma_max is not None:
            cuts = np.atleast_1d(np.asarray(sigma_max, dtype=np.float64)).ravel()
            if cuts.size not in (1, high.size):
                raise ValueError(f"set_polarized_variants: sigma_max needs a scalar or one value per variant (got {cuts.size} for {high.size} variants)")
            cuts = np.ascontiguousarray(np.broadcast_to(cuts, high.shape))
        mixes = None
        if electrons is not None and high.size > 0:
            given = [electrons] * int(high.size) if hasattr(electrons, "keys") else list(electrons)
            if len(given) == 1:
                given = given * int(high.size)
            if len(given) != high.size:
                raise ValueError(f"set_polarized_variants: electrons needs one mapping or one per variant (got {len(given)} for {high.size} variants)")
            own = self._block_electrons()
            mixes = (_capi.ElectronMix * int(high.size))()
            for v, mapping in enumerate(given):
                unknown = set(mapping) - set(_capi.ELECTRON_MIX_KEYS)
                if unknown:
                    raise ValueError(f"set_polarized_variants: unknown electron key(s) {sorted(unknown)}; the keys are {list(_capi.ELECTRON_MIX_KEYS)}")
                for key in _capi.ELECTRON_MIX_KEYS:
                    setattr(mixes[v], key, float(mapping.get(key, own[key])))
        self._check(self._lib.bl_set_polarized_variants_electrons(self._ctx, int(high.size), low.ctypes.data_as(C.c_void_p),
                                                                  high.ctypes.data_as(C.c_void_p), unit.ctypes.data_as(C.c_void_p),
                                                                  cuts.ctypes.data_as(C.c_void_p) if cuts is not None else None,
                                                                  C.cast(mixes, C.c_void_p) if mixes is not None else None))

    @property
    def polarized_variants(self):
        """The (rat_high, rat_low, rho_cgs) triples set_polarized_variants() set; [] when the parameter block's are rendered."""
        (low, high, rho, _), _ = self._variants()
        return [(high[v], low[v], rho[v]) for v in range(self.num_polarized_variants)]

    @property
    def polarized_cuts(self):
        """The variants' sigma cuts set_polarized_variants(sigma_max=...) set, one per variant; None when every variant is rendered
        under the parameter block's own cut_sigma_max."""
        (_, _, _, sigma_max), flags = self._variants()
        return sigma_max if flags & 1 else None

    def _block_electrons(self):
        """The parameter block's own electron distribution, as a mapping with set_polarized_variants()'s keys."""
        values = {key: self.params.get("plasma_" + key) for key in _capi.ELECTRON_MIX_KEYS}
        return {key: float(value) if value is not None else 0.0 for key, value in values.items()}   # (a key the block does not set is not read)

    @property
    def polarized_electrons(self):
        """The electron distribution every variant renders with (bl_polarized_variant_electrons), one mapping per variant - the
        parameter block's own where set_polarized_variants(electrons=...) set none; one entry when no variants are set."""
        out = []
        for v in range(max(1, self.num_polarized_variants)):
            mix = _capi.ElectronMix()
            self._check(self._lib.bl_polarized_variant_electrons(self._ctx, v, C.byref(mix)))
            out.append({key: getattr(mix, key) for key in _capi.ELECTRON_MIX_KEYS})
        return out

    @property
    def polarized_electrons_set(self):
        """True when the variants carry distributions of their own (set_polarized_variants(electrons=...))."""
        return bool(self._variants()[1] & 2)

    @property
    def num_polarized_variants(self):
        return self._lib.bl_num_polarized_variants(self._ctx)

    def fit_density_units_polarized(self, pairs, target_jy, distance_pc, lo, hi, frequency=0, rtol=1.0e-3):
        """For every (rat_high, rat_low) pair of a polarized run, the density unit in [lo, hi] at which the root image's Stokes-I flux
        (flux.stokes_flux_jy) at image frequency `frequency` is target_jy to within rtol. All pairs advance together: every render
        carries each unfinished pair's current trial units as variants (up to 16 per render; more trials than that take another
        render of the same step) - the bracket's two ends first, then secant steps in log rho and log flux, falling back to
        bisection where a step leaves the bracket or shrinks it by less than half. The trials are rendered under the parameter
        block's own cut_sigma_max; the context's variants, and their sigma cuts if they had any, are restored on exit.
        Returns ([(rho_cgs, flux_jy, m_net, v_net) per pair], renders)."""
        from . import flux as _flux
        pairs = [(float(h), float(l)) for h, l in pairs]
        if self.num_cameras >= 2:
            raise ValueError("fit_density_units_polarized sums one camera's image: not with two or more cameras (set_cameras)")
        if not pairs:
            raise ValueError("fit_density_units_polarized needs at least one (rat_high, rat_low) pair")
        if not (0.0 < lo < hi) or not np.isfinite(hi):
            raise ValueError(f"fit_density_units_polarized needs 0 < lo < hi, finite (got {lo}, {hi})")
        if not (target_jy > 0.0 and rtol > 0.0):
            raise ValueError("fit_density_units_polarized needs target_jy > 0 and rtol > 0")
        saved, saved_cuts = self.polarized_variants, self.polarized_cuts
        saved_electrons = self.polarized_electrons if self.polarized_electrons_set else None
        renders = 0

        def evaluate(trials):   # [(pair index, rho)] -> [(I, Q, U, V) in Jy]
            nonlocal renders
            out = []
            for start in range(0, len(trials), 16):
                part = trials[start:start + 16]
                self.set_polarized_variants([pairs[k][0] for k, _ in part], [rho for _, rho in part], rat_low=[pairs[k][1] for k, _ in part])
                got = self.render()
                renders += 1
                out += [_flux.stokes_flux_jy(got["image_by_variant"][v], self.params, distance_pc, frequency) for v in range(len(part))]
            return out

        try:
            n = len(pairs)
            found = [None] * n
            # the bracket's ends: (log rho, log I) of both, for every pair
            ends = evaluate([(k, float(lo)) for k in range(n)] + [(k, float(hi)) for k in range(n)])
            a = [[math.log(lo), ends[k]] for k in range(n)]
            b = [[math.log(hi), ends[n + k]] for k in range(n)]
            bisect = [False] * n
            log_target = math.log(target_jy)

            def close(stokes):
                return abs(stokes[0] - target_jy) <= rtol * target_jy

            def result(rho, stokes):
                m_net, v_net, _ = _flux.net_polarization(stokes)
                return (float(rho), float(stokes[0]), m_net, v_net)

            for k in range(n):
                fa, fb = a[k][1][0], b[k][1][0]
                if close(a[k][1]):
                    found[k] = result(lo, a[k][1])
                elif close(b[k][1]):
                    found[k] = result(hi, b[k][1])
                elif not (fa - target_jy) * (fb - target_jy) < 0.0:
                    raise ValueError(f"fit_density_units_polarized: [{lo:.6g}, {hi:.6g}] g/cm^3 does not bracket {target_jy:.6g} Jy for the pair "
                                     f"{pairs[k]} (fluxes at the ends: {fa:.6g}, {fb:.6g} Jy)")
            for _ in range(64):
                todo = [k for k in range(n) if found[k] is None]
                if not todo:
                    break
                trials = []
                for k in todo:
                    xa, xb = a[k][0], b[k][0]
                    ia, ib = a[k][1][0], b[k][1][0]
                    x = 0.5 * (xa + xb)
                    if not bisect[k] and ia > 0.0 and ib > 0.0 and ia != ib:
                        la, lb = math.log(ia), math.log(ib)
                        secant = xa + (log_target - la) * (xb - xa) / (lb - la)
                        if min(xa, xb) < secant < max(xa, xb):
                            x = secant
                    trials.append((k, math.exp(x)))
                for (k, rho), stokes in zip(trials, evaluate(trials)):
                    if close(stokes):
                        found[k] = result(rho, stokes)
                        continue
                    x, width = math.log(rho), abs(b[k][0] - a[k][0])
                    if (stokes[0] - target_jy) * (a[k][1][0] - target_jy) > 0.0:
                        a[k] = [x, stokes]
                    else:
                        b[k] = [x, stokes]
                    bisect[k] = abs(b[k][0] - a[k][0]) > 0.5 * width   # (a secant step that hardly moved the bracket: halve it next)
            if any(f is None for f in found):
                raise RuntimeError(f"fit_density_units_polarized: no unit within rtol = {rtol} of {target_jy} Jy after {renders} renders")
            return found, renders
        finally:
            self.set_polarized_variants([h for h, _, _ in saved], [u for _, _, u in saved], rat_low=[l for _, l, _ in saved], sigma_max=saved_cuts,
                                        electrons=saved_electrons)

    def set_caller_stream(self, stream=None, enabled=True):
        """Every later render starts behind the work queued so far on `stream` (a raw hipStream_t handle, e.g.
        torch.cuda.current_stream().cuda_stream; None / 0: the NULL stream) - bl_set_caller_stream."""
        self._check(self._lib.bl_set_caller_stream(self._ctx, C.c_void_p(int(stream or 0)), 1 if enabled else 0))
        self._caller_stream = (int(stream or 0), bool(enabled))   # (what _render_level_device puts back)

    def follow_torch_stream(self, device=None):
        """set_caller_stream(torch's current stream on `device`): tensors torch filled, and collectives torch has waited for on
        that stream, are complete before a render touches the buffers."""
        import torch
        self.set_caller_stream(torch.cuda.current_stream(device).cuda_stream)

    def debug_set_switches(self, *names):
        """Measurement switches of this context by name (_capi.SWITCHES: "RECORD_EVERY_STEP", "NO_FUSED_LOCATE", ...); none: all off.
        They select another kernel or layout with the same results (bl_stats.switches echoes them)."""
        mask = 0
        for name in names:
            mask |= _capi.SWITCHES[name]
        self._check(self._lib.bl_debug_set_switches(self._ctx, mask))

    def debug_set_guard_band(self, relative_width):
        self._check(self._lib.bl_debug_set_guard_band(self._ctx, float(relative_width)))

    def set_overlap(self, on):
        """Overlap the geodesic kernel of the next chunk with the shading of the current one."""
        self._check(self._lib.bl_set_overlap(self._ctx, 1 if on else 0))

    # ------------------------------------------------------------------ grid
    def set_grid(self, grid):
        """grid: blacklight_amd.mock.Grid (or anything with .desc())."""
        desc = grid.desc()
        self._grid_keepalive = grid
        self._check(self._lib.bl_set_grid(self._ctx, C.byref(desc)))

    def _device_cells(self, grid, prim, stream, dims):
        """bl_device_cells for a torch tensor on this context's device; ValueError for anything the C call must not be handed."""
        import torch
        if dims not in ("vb", "bv"):
            raise ValueError('dims must be "vb" ([variable][block][k][j][i]) or "bv" ([block][variable][k][j][i])')
        if not isinstance(prim, torch.Tensor):
            raise ValueError("prim must be a torch.Tensor in device memory (host arrays go through set_grid)")
        if not prim.is_cuda:
            raise ValueError("prim lies in host memory: host arrays go through set_grid")
        device = self._lib.bl_context_device(self._ctx)
        if device >= 0 and prim.device.index != device:
            raise ValueError(f"prim lies on device {prim.device.index}, the context renders on device {device}")
        if prim.dtype not in (torch.float32, torch.float64):
            raise ValueError("prim must be float32 or float64")
        if prim.dim() != 5:
            raise ValueError("prim must have five dimensions: (variable, block) in the order `dims` says, then k, j, i")
        desc = grid.desc()
        n_k, n_j, n_i = desc.n_k, desc.n_j, desc.n_i
        if tuple(prim.shape[2:]) != (n_k, n_j, n_i):
            raise ValueError(f"prim's last three dimensions are {tuple(prim.shape[2:])}, the grid's blocks have {(n_k, n_j, n_i)} cells")
        if tuple(prim.stride()[2:]) != (n_j * n_i, n_i, 1):
            raise ValueError("the cells of one (variable, block) must be contiguous [k][j][i]")
        n_var, n_blocks = (prim.shape[0], prim.shape[1]) if dims == "vb" else (prim.shape[1], prim.shape[0])
        if n_blocks != desc.n_blocks:
            raise ValueError(f"prim holds {n_blocks} blocks, the grid {desc.n_blocks}")
        var_stride, block_stride = (prim.stride(0), prim.stride(1)) if dims == "vb" else (prim.stride(1), prim.stride(0))
        if (n_var > 1 and var_stride < 1) or (n_blocks > 1 and block_stride < 1):
            raise ValueError("prim's variable and block strides must be positive")
        desc.n_var = n_var
        cells = _capi.DeviceCells()
        cells.prim = prim.data_ptr()
        cells.dtype = _capi.BL_CELLS_F32 if prim.dtype == torch.float32 else _capi.BL_CELLS_F64
        cells.var_stride, cells.block_stride = max(int(var_stride), 1), max(int(block_stride), 1)
        cells.n_elements = prim.untyped_storage().nbytes() // prim.element_size() - prim.storage_offset()
        if stream == "torch":
            cells.wait, cells.stream = 1, torch.cuda.current_stream(prim.device).cuda_stream
        elif stream is not None:
            cells.wait, cells.stream = 1, int(stream)
        return desc, cells

    def set_grid_device(self, grid, prim, stream="torch", dims="vb"):
        """set_grid with the cells in device memory (bl_set_grid_device). grid: geometry and variable indices (a mock.Grid or anything
        with .desc(); its own prim may be None). prim: a torch tensor on this context's device, float32 or float64 (rounded to float32
        on the device), five dimensions: (variable, block) for dims="vb" or (block, variable) for dims="bv", then (n_k, n_j, n_i)
        contiguous; the first two strides may be anything positive. stream: "torch" - the staging waits for torch's current stream
        on that device; a raw hipStream_t handle - for that stream; None - for nothing (the caller has synchronised). The tensor may
        be overwritten as soon as the call returns."""
        desc, cells = self._device_cells(grid, prim, stream, dims)
        self._grid_keepalive = grid
        self._check(self._lib.bl_set_grid_device(self._ctx, C.byref(desc), C.byref(cells)))

    def _harm_cells(self, grid, prims, stream):
        """bl_harm_cells for a torch tensor on this context's device; ValueError for anything the C call must not be handed."""
        import torch
        if not isinstance(prims, torch.Tensor):
            raise ValueError("prims must be a torch.Tensor in device memory (host arrays go through HarmGrid.convert_host and set_grid)")
        if not prims.is_cuda:
            raise ValueError("prims lies in host memory: host arrays go through HarmGrid.convert_host and set_grid")
        device = self._lib.bl_context_device(self._ctx)
        if device >= 0 and prims.device.index != device:
            raise ValueError(f"prims lies on device {prims.device.index}, the context renders on device {device}")
        if prims.dtype not in (torch.float32, torch.float64):
            raise ValueError("prims must be float32 or float64")
        if tuple(prims.shape) != tuple(grid.shape):
            raise ValueError(f"prims has shape {tuple(prims.shape)}, the grid's header says {tuple(grid.shape)}: (n1, n2, n3, n_prim)")
        if not prims.is_contiguous():
            raise ValueError("prims must be contiguous [n1][n2][n3][n_prim]")
        cells = _capi.HarmCells()
        cells.prim = prims.data_ptr()
        cells.dtype = _capi.BL_CELLS_F32 if prims.dtype == torch.float32 else _capi.BL_CELLS_F64
        cells.n_elements = prims.untyped_storage().nbytes() // prims.element_size() - prims.storage_offset()
        if stream == "torch":
            cells.wait, cells.stream = 1, torch.cuda.current_stream(prims.device).cuda_stream
        elif stream is not None:
            cells.wait, cells.stream = 1, int(stream)
        return cells

    def set_grid_device_harm(self, grid, prims, stream="torch"):
        """set_grid_device for the array an iharm3d-family code holds (bl_set_grid_device_harm). grid: a snapshot.HarmGrid; prims: a torch
        tensor on this context's device, float32 or float64, contiguous (n1, n2, n3, n_prim). The staging kernel transposes and converts
        the cells as the file reader does: the render reads the bits set_grid(Snapshot) would have put there. stream: as set_grid_device."""
        cells = self._harm_cells(grid, prims, stream)
        self._grid_keepalive = grid
        self._check(self._lib.bl_set_grid_device_harm(self._ctx, grid.handle, C.byref(cells)))

    def set_grid_slice_device_harm(self, n, grid, prims, time, stream="torch"):
        """set_grid_slice with a harm-family array in device memory: set_grid_device_harm's arguments."""
        cells = self._harm_cells(grid, prims, stream)
        self._check(self._lib.bl_set_grid_slice_device_harm(self._ctx, int(n), grid.handle, C.byref(cells), float(time)))

    def harm_convert_device(self, grid, prims, out=None, stream="torch"):
        """The planes HarmGrid.convert_host makes, written on the device (bl_harm_convert_device): a float32 tensor
        (grid.planes, n3, n2, n1) - `out` if given (contiguous, on this context's device), else a new one. With grid.desc(converted=True)
        it is what set_grid_device takes. Returns when the planes are written."""
        import torch
        cells = self._harm_cells(grid, prims, stream)
        n1, n2, n3, _ = grid.shape
        shape = (grid.planes, n3, n2, n1)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=prims.device)
        elif (not isinstance(out, torch.Tensor) or out.device != prims.device or out.dtype != torch.float32 or tuple(out.shape) != shape
              or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous float32 tensor of shape {shape} on the device of prims")
        self._check(self._lib.bl_harm_convert_device(self._ctx, grid.handle, C.byref(cells), out.data_ptr()))
        return out

    @property
    def grid_host_bytes(self):
        """Bytes the last set_grid* call copied from host memory (after set_grid_device: the tables only)."""
        return int(self._lib.bl_grid_host_bytes(self._ctx))

    # ------------------------------------------------------------------ slow light
    def slow_light_read(self, snapshot):
        """SimulationReader::Read(snapshot) with slow_light_on: advance the window of files to the camera time of
        image `snapshot` (reads .athdf files itself) and select that image for the next render()."""
        self._check(self._lib.bl_slow_light_read(self._ctx, int(snapshot)))

    def set_grid_slice(self, n, grid, time):
        """Slice n of the slow-light window (n = 0: latest file) from a caller-side reader."""
        desc = grid.desc()
        self._check(self._lib.bl_set_grid_slice(self._ctx, int(n), C.byref(desc), float(time)))

    def set_grid_slice_device(self, n, grid, prim, time, stream="torch", dims="vb"):
        """set_grid_slice with the cells in device memory: set_grid_device's arguments."""
        desc, cells = self._device_cells(grid, prim, stream, dims)
        self._check(self._lib.bl_set_grid_slice_device(self._ctx, int(n), C.byref(desc), C.byref(cells), float(time)))

    def shift_grid_slices(self, count):
        self._check(self._lib.bl_shift_grid_slices(self._ctx, int(count)))

    def set_snapshot(self, snapshot):
        self._check(self._lib.bl_set_snapshot(self._ctx, int(snapshot)))

    def clear_warnings(self):
        self._lib.bl_warnings_clear(self._ctx)

    # ------------------------------------------------------------------ render
    def level_pixels(self, level=0, n_blocks=0):
        if level == 0:
            return max(1, self.num_cameras) * self.resolution * self.resolution   # (several cameras: "virtual pixels" c res^2 + m)
        bs = int(self.params.get("adaptive_block_size"))
        return n_blocks * bs * bs

    def pinned_array(self, shape, dtype=np.float64):
        """A numpy array over host memory the GPU downloads into at the link's rate (bl_host_alloc: pinned), owned by this context and
        freed with it (close(): the array must not be used afterwards) - what a frame loop hands to render(out=...) frame after frame.
        Falls back to an ordinary array where pinning is refused."""
        shape = tuple(int(n) for n in np.atleast_1d(shape))
        count = int(np.prod(shape))
        nbytes = count * np.dtype(dtype).itemsize
        ptr = self._lib.bl_host_alloc(self._ctx, nbytes) if nbytes > 0 else None
        if not ptr:
            return np.empty(shape, dtype=dtype)
        self.__dict__.setdefault("_pinned", []).append(ptr)
        raw = (C.c_char * nbytes).from_address(ptr)
        return np.frombuffer(raw, dtype=dtype, count=count).reshape(shape)

    def render(self, level=0, block_locs=None, pixel_map=None, want_camera=False, out=None):
        """Trace one adaptive level into host arrays. Returns a dict. out: a dict of arrays to receive "image" (n_q, n_rays) f64,
        "sample_num" (n_rays) i32 and "sample_flags" (n_rays) u8 instead of fresh ones - e.g. pinned_array()s a frame loop reuses:
        a download into touched, pinned pages takes a third of the time of one into new pageable memory."""
        d = _capi.RenderDesc()
        d.level = level
        keep = []
        n_blocks = 0
        if block_locs is not None:
            bl = np.ascontiguousarray(block_locs, dtype=np.int32).reshape(-1, 2)
            keep.append(bl)
            d.block_locs = bl.ctypes.data_as(C.c_void_p)
            n_blocks = bl.shape[0]
            d.n_blocks = n_blocks
        if pixel_map is not None:
            pm = np.ascontiguousarray(pixel_map, dtype=np.int32)
            keep.append(pm)
            d.pixel_map = pm.ctypes.data_as(C.c_void_p)
            n_rays = pm.size
        else:
            n_rays = self.level_pixels(level, n_blocks)
        d.n_rays = n_rays
        d.outputs_on_device = 0
        n_q = self.num_quantities
        out = out or {}
        image = out.get("image") if out.get("image") is not None else np.empty((n_q, n_rays), dtype=np.float64)
        sample_num = out.get("sample_num") if out.get("sample_num") is not None else np.empty(n_rays, dtype=np.int32)
        sample_flags = out.get("sample_flags") if out.get("sample_flags") is not None else np.empty(n_rays, dtype=np.uint8)
        if (image.shape != (n_q, n_rays) or image.dtype != np.float64 or not image.flags.c_contiguous or sample_num.shape != (n_rays,)
                or sample_num.dtype != np.int32 or sample_flags.shape != (n_rays,) or sample_flags.dtype != np.uint8):
            raise ValueError("render(out=...): image (n_q, n_rays) float64, sample_num (n_rays) int32, sample_flags (n_rays) uint8, C-contiguous")
        d.image = image.ctypes.data_as(C.c_void_p)
        d.sample_num = sample_num.ctypes.data_as(C.c_void_p)
        d.sample_flags = sample_flags.ctypes.data_as(C.c_void_p)
        camera_pos = camera_dir = None
        if want_camera:
            camera_pos = np.empty((n_rays, 4))
            camera_dir = np.empty((n_rays, 4))
            d.camera_pos = camera_pos.ctypes.data_as(C.c_void_p)
            d.camera_dir = camera_dir.ctypes.data_as(C.c_void_p)
        rendering = None
        n_render = self.num_render_images
        if n_render > 0:
            rendering = np.empty((n_render, 3, n_rays))
            d.render = rendering.ctypes.data_as(C.c_void_p)
        self._check(self._lib.bl_render(self._ctx, C.byref(d)))
        n_models, n_units = max(1, self.num_electron_models), max(1, self.num_density_units)
        n_variants = max(1, self.num_polarized_variants)
        n_cuts = max(1, self.num_sigma_cuts)
        # (electron mixes, the outermost axis: the three views below gain a leading axis of them while a list is set, and only then)
        n_mixes = max(1, self.num_electron_mixes)
        lead = (n_mixes,) if self.num_electron_mixes > 0 else ()
        rows = n_q // n_mixes
        return dict(image=image, image_by_model=image.reshape(lead + (n_models, rows // n_models, n_rays)),
                    image_by_variant=image.reshape(n_variants, n_q // n_variants, n_rays),
                    image_by_unit=image.reshape(lead + (n_models, n_units, rows // (n_models * n_units), n_rays)),
                    image_by_cut=image.reshape(lead + (n_models, n_units, n_cuts, rows // (n_models * n_units * n_cuts), n_rays)),
                    image_by_mix=image.reshape(n_mixes, rows, n_rays), sample_num=sample_num,
                    sample_flags=sample_flags, camera_pos=camera_pos, camera_dir=camera_dir, rendering=rendering, stats=self.stats)

    # ------------------------------------------------------------------ host steps of the reference loop
    def adaptive_refine(self, level, image, block_locs=None):
        """CheckAdaptiveRefinement for the level just rendered (reference radiation_adaptive.cpp:19-139)
        plus AugmentCamera's block list of the next level (camera.cpp:445-458).
        Returns (refine_flags, next_block_locs); an empty next list ends the adaptive loop."""
        image = np.ascontiguousarray(image, dtype=np.float64)
        if level == 0:
            bs = int(self.params.get("adaptive_block_size"))
            n_blocks = (self.resolution // bs) ** 2
            locs_ptr = None
        else:
            bl = np.ascontiguousarray(block_locs, dtype=np.int32).reshape(-1, 2)
            n_blocks = bl.shape[0]
            locs_ptr = bl.ctypes.data_as(C.c_void_p)
        flags = np.zeros(n_blocks, dtype=np.uint8)
        nxt = np.zeros((4 * n_blocks, 2), dtype=np.int32)
        count = C.c_int32(0)
        self._check(self._lib.bl_adaptive_refine(self._ctx, level, n_blocks, locs_ptr, image.ctypes.data_as(C.c_void_p),
                                                 flags.ctypes.data_as(C.c_void_p), C.byref(count),
                                                 nxt.ctypes.data_as(C.c_void_p)))
        return flags.astype(bool), nxt[: 4 * count.value].copy()

    def adaptive_refine_device(self, level, image, block_locs=None, rows=None, pixels=None):
        """adaptive_refine for a level whose image lies in device memory (bl_adaptive_refine_device): the same flags and the same
        next list, decided by one kernel over all blocks; only the flags come down. image: a torch tensor on this context's
        device, float64, contiguous, shape (rows, pixels) as render_device fills it - or a raw device pointer with `rows` and
        `pixels`. With set_caller_stream / follow_torch_stream enabled the kernel starts behind the work queued on that stream
        (what fills the tensor). ValueError for anything the C call must not be handed."""
        if isinstance(image, int) and not isinstance(image, bool):
            if rows is None or pixels is None or int(rows) < 1 or int(pixels) < 0 or image == 0:
                raise ValueError("a raw device pointer needs rows and pixels, the shape of the image it points at")
            pointer, rows, pixels = int(image), int(rows), int(pixels)
        else:
            import torch
            if not isinstance(image, torch.Tensor):
                raise ValueError("image must be a torch.Tensor in device memory or a raw device pointer (host arrays go through adaptive_refine)")
            if not image.is_cuda:
                raise ValueError("image lies in host memory: host arrays go through adaptive_refine")
            device = self._lib.bl_context_device(self._ctx)
            if device >= 0 and image.device.index != device:
                raise ValueError(f"image lies on device {image.device.index}, the context renders on device {device}")
            if image.dtype != torch.float64:
                raise ValueError("image must be float64")
            if image.dim() != 2 or not image.is_contiguous():
                raise ValueError("image must be contiguous with shape (rows, pixels)")
            pointer, (rows, pixels) = image.data_ptr(), image.shape
        if level == 0:
            bs = int(self.params.get("adaptive_block_size"))
            n_blocks = (self.resolution // bs) ** 2
            locs_ptr = None
        else:
            bl = np.ascontiguousarray(block_locs, dtype=np.int32).reshape(-1, 2)
            n_blocks = bl.shape[0]
            locs_ptr = bl.ctypes.data_as(C.c_void_p)
        if rows != self.num_quantities or pixels != self.level_pixels(level, n_blocks):
            raise ValueError(f"image has shape ({rows}, {pixels}), level {level} has ({self.num_quantities}, {self.level_pixels(level, n_blocks)})")
        flags = np.zeros(n_blocks, dtype=np.uint8)
        nxt = np.zeros((4 * n_blocks, 2), dtype=np.int32)
        count = C.c_int32(0)
        self._check(self._lib.bl_adaptive_refine_device(self._ctx, level, n_blocks, locs_ptr, C.c_void_p(pointer), flags.ctypes.data_as(C.c_void_p),
                                                        C.byref(count), nxt.ctypes.data_as(C.c_void_p)))
        return flags.astype(bool), nxt[: 4 * count.value].copy()

    def render_template(self, want_camera=False):
        """The per-pixel outputs of render() for zero rays: which rows a level has and their leading shapes
        (blacklight_amd.distributed uses it on a rank that holds no rays of a level)."""
        n_render = self.num_render_images
        return dict(image=np.empty((self.num_quantities, 0)), sample_num=np.empty(0, dtype=np.int32),
                    sample_flags=np.empty(0, dtype=np.uint8),
                    camera_pos=np.empty((0, 4)) if want_camera else None, camera_dir=np.empty((0, 4)) if want_camera else None,
                    rendering=np.empty((n_render, 3, 0)) if n_render > 0 else None)

    def render_adaptive(self, want_camera=False, distributed=False, comm=None):
        """The reference's do { Integrate; AddGeodesics } while (!done) loop (blacklight.cpp:196-233).
        Returns a list of per-level dicts (level 0 first), each with image / block_locs / ...
        distributed=True: every rank of torch.distributed's default group calls this; the camera is tiled over the
        ranks level by level (blacklight_amd.distributed.render_adaptive) and rank 0 gets the same list a single
        GPU returns (the other ranks get None); warnings with the levels' totals are in .distributed_warnings."""
        if distributed:
            from . import distributed as bd
            levels, self.distributed_warnings = bd.render_adaptive(self, comm, want_camera)
            return levels
        levels = [self.render(want_camera=want_camera)]
        levels[0]["block_locs"] = None
        if int(self.params.get("adaptive_max_level") or 0) <= 0:
            return levels
        level = 0
        while True:
            flags, nxt = self.adaptive_refine(level, levels[level]["image"], levels[level]["block_locs"])
            levels[level]["refinement_flags"] = flags
            if nxt.shape[0] == 0:
                return levels
            level += 1
            out = self.render(level=level, block_locs=nxt, want_camera=want_camera)
            out["block_locs"] = nxt
            levels.append(out)

    def _render_level_device(self, level=0, block_locs=None, want_camera=False):
        """One level of render_adaptive_device: render_device into fresh torch tensors on the context's device - image (n_q, n_rays)
        float64, sample_num int32, sample_flags uint8, camera_pos / camera_dir (n_rays, 4), rendering (n_images, 3, n_rays). The
        render is queued behind the tensors' creation on torch's current stream; the caller-stream setting the context had
        (set_caller_stream / follow_torch_stream, or none) is put back before the call returns."""
        import torch
        device = torch.device("cuda", self._lib.bl_context_device(self._ctx))
        n_blocks = 0 if block_locs is None else int(np.asarray(block_locs).reshape(-1, 2).shape[0])
        n_rays = self.level_pixels(level, n_blocks)
        n_render = self.num_render_images
        out = dict(image=torch.empty((self.num_quantities, n_rays), dtype=torch.float64, device=device),
                   sample_num=torch.empty(n_rays, dtype=torch.int32, device=device), sample_flags=torch.empty(n_rays, dtype=torch.uint8, device=device),
                   camera_pos=torch.empty((n_rays, 4), dtype=torch.float64, device=device) if want_camera else None,
                   camera_dir=torch.empty((n_rays, 4), dtype=torch.float64, device=device) if want_camera else None,
                   rendering=torch.empty((n_render, 3, n_rays), dtype=torch.float64, device=device) if n_render > 0 else None)
        before = self.__dict__.get("_caller_stream", (0, False))
        self.follow_torch_stream(device)
        try:
            pointer = {name: (0 if tensor is None else tensor.data_ptr()) for name, tensor in out.items()}
            out["stats"] = self.render_device(pointer["image"], n_rays, level=level, block_locs=block_locs, sample_num_ptr=pointer["sample_num"],
                                              sample_flags_ptr=pointer["sample_flags"], camera_pos_ptr=pointer["camera_pos"],
                                              camera_dir_ptr=pointer["camera_dir"], render_ptr=pointer["rendering"])
        finally:
            self.set_caller_stream(*before)
        return out

    def render_adaptive_device(self, want_camera=False):
        """render_adaptive with every level left in device memory: each level rendered by render_device into fresh torch tensors and
        refined by adaptive_refine_device, so that no image crosses to the host. A list of per-level dicts as render_adaptive's:
        image, sample_num, sample_flags, camera_pos, camera_dir and rendering as torch tensors on the device, block_locs and
        refinement_flags as numpy arrays, stats. The reshaped views of render()'s dicts (image_by_model, image_by_variant,
        image_by_unit, image_by_cut, image_by_mix) are not there: an adaptive run has one variant, and image.reshape gives them.
        The decision needs no caller stream: bl_render has returned when it is made, on the stream the level was rendered on.
        The context's caller-stream setting is left as it was."""
        levels = [self._render_level_device(want_camera=want_camera)]
        levels[0]["block_locs"] = None
        if int(self.params.get("adaptive_max_level") or 0) <= 0:
            return levels
        level = 0
        while True:
            flags, nxt = self.adaptive_refine_device(level, levels[level]["image"], levels[level]["block_locs"])
            levels[level]["refinement_flags"] = flags
            if nxt.shape[0] == 0:
                return levels
            level += 1
            out = self._render_level_device(level=level, block_locs=nxt, want_camera=want_camera)
            out["block_locs"] = nxt
            levels.append(out)

    def write_output(self, levels, path=None, snapshot=0, variant=None, camera=None, frequency=None):
        """OutputWriter::Write (reference output_writer.cpp:169-274); `levels` as from render_adaptive. variant = v: image v of a
        render of several variants ([render()]: the rows of all of them) as a file of its own (bl_write_output_variant) - what a
        context with that variant in its parameter block writes; without `path` the name is variant_output_path(snapshot, v).
        camera = c: camera c of a render of several cameras (bl_write_output_camera; with variant = v, that variant of it) - what a
        context with that camera's angles in its parameter block writes from the camera's slice of every row and record.
        frequency = l: the file of ONE frequency of the render (bl_write_output_frequency; with camera = c and variant = v, of that
        camera and variant) - what a context with image_num_frequencies = 1 and that image_frequency writes; without `path` the name
        is variant_output_path(snapshot, v, c, frequency=l)."""
        d = _capi.OutputDesc()
        d.adaptive_num_levels = len(levels) - 1
        d.snapshot = snapshot
        keep = []
        plane = int(self.params.get("camera_type")) == 0
        for index, lv in enumerate(levels):
            image = np.ascontiguousarray(lv["image"], dtype=np.float64)
            keep.append(image)
            d.level[index].image = image.ctypes.data_as(C.c_void_p)
            if index > 0:
                bl = np.ascontiguousarray(lv["block_locs"], dtype=np.int32)
                keep.append(bl)
                d.level[index].n_blocks = bl.shape[0]
                d.level[index].block_locs = bl.ctypes.data_as(C.c_void_p)
            if lv.get("rendering") is not None:
                rendering = np.ascontiguousarray(lv["rendering"], dtype=np.float64)
                keep.append(rendering)
                d.level[index].render = rendering.ctypes.data_as(C.c_void_p)
            records = lv.get("camera_pos") if plane else lv.get("camera_dir")
            if records is not None:
                records = np.ascontiguousarray(records, dtype=np.float64)
                keep.append(records)
                d.level[index].camera = records.ctypes.data_as(C.c_void_p)
        target = None if path is None else str(path).encode()
        if frequency is not None:
            self._check(self._lib.bl_write_output_frequency(self._ctx, target, C.byref(d), int(frequency), int(camera or 0), int(variant or 0)))
        elif camera is not None:
            self._check(self._lib.bl_write_output_camera(self._ctx, target, C.byref(d), int(camera), int(variant or 0)))
        elif variant is None:
            self._check(self._lib.bl_write_output(self._ctx, target, C.byref(d)))
        else:
            self._check(self._lib.bl_write_output_variant(self._ctx, target, C.byref(d), int(variant)))

    def render_device(self, image_ptr, n_rays, level=0, pixel_map=None, sample_num_ptr=0, sample_flags_ptr=0,
                      block_locs=None, camera_pos_ptr=0, camera_dir_ptr=0, render_ptr=0):
        """Trace into caller-owned HBM (raw device pointers, e.g. torch.Tensor.data_ptr()): image (n_q, n_rays), sample_num,
        sample_flags (n_rays), camera_pos / camera_dir (n_rays, 4), renderings (n_images, 3, n_rays) - the layouts of render()."""
        d = _capi.RenderDesc()
        d.level = level
        keep = []
        if block_locs is not None:
            bl = np.ascontiguousarray(block_locs, dtype=np.int32).reshape(-1, 2)
            keep.append(bl)
            d.block_locs = bl.ctypes.data_as(C.c_void_p)
            d.n_blocks = bl.shape[0]
        if pixel_map is not None:
            pm = np.ascontiguousarray(pixel_map, dtype=np.int32)
            keep.append(pm)
            d.pixel_map = pm.ctypes.data_as(C.c_void_p)
        d.n_rays = n_rays
        d.outputs_on_device = 1
        d.image = C.c_void_p(image_ptr)
        d.sample_num = C.c_void_p(sample_num_ptr) if sample_num_ptr else None
        d.sample_flags = C.c_void_p(sample_flags_ptr) if sample_flags_ptr else None
        d.camera_pos = C.c_void_p(camera_pos_ptr) if camera_pos_ptr else None
        d.camera_dir = C.c_void_p(camera_dir_ptr) if camera_dir_ptr else None
        d.render = C.c_void_p(render_ptr) if render_ptr else None
        self._check(self._lib.bl_render(self._ctx, C.byref(d)))
        return self.stats
