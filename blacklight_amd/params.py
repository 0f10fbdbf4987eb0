"""Parameter block of the drop-in boundary (mirror of the reference's InputReader).

The block itself lives in C (bl_params, include/blacklight_amd.h); Python only holds the bytes and
goes through the same `key = value` grammar as a line of a .input file, so there is exactly one
parser (blacklight_amd/csrc/bl_params.cpp).
"""
import ctypes as C

from . import _capi


def _format(value):
    if isinstance(value, bool):
        return "true" if value else "false"
    if isinstance(value, float):
        return repr(value)
    return str(value)


class Params:
    def __init__(self):
        L = _capi.lib()
        self._buf = C.create_string_buffer(L.bl_params_sizeof())
        L.bl_params_clear(self._buf)
        self._sweep = _capi.Sweep()   # the sweep_* keys: lists beside the block (bl_sweep), never in it
        self._sweep_cuts = _capi.SweepCuts()   # ... sweep_cut_sigma_max (bl_sweep_cuts)
        self._sweep_cameras = _capi.SweepCameras()   # ... sweep_camera_th, sweep_camera_ph (bl_sweep_cameras)
        self._sweep_electrons = _capi.SweepElectrons()   # ... sweep_power_frac ... sweep_w (bl_sweep_electrons)
        self._sweep_frequencies = _capi.SweepFrequencies()   # ... sweep_frequency (bl_sweep_frequencies)
        self.num_runs = 1

    @property
    def ptr(self):
        return C.cast(self._buf, C.c_void_p)

    @classmethod
    def from_file(cls, path):
        """InputReader::Read() (reference src/input_reader/input_reader.cpp:72)."""
        self = cls()
        err = C.create_string_buffer(1024)
        runs = C.c_int(1)
        rc = _capi.lib().bl_params_read_file_sweep_all(self._buf, C.byref(self.sweep_all), str(path).encode(), C.byref(runs), err, len(err))
        if rc != 0:
            raise _capi.BlacklightError(rc, err.value.decode())
        self.num_runs = runs.value
        return self

    @classmethod
    def from_text(cls, text):
        self = cls()
        for line in text.splitlines():
            self.set_line(line)
        return self

    @classmethod
    def from_dict(cls, mapping):
        self = cls()
        for key, value in mapping.items():
            self.set(key, value)
        return self

    def set_line(self, line):
        err = C.create_string_buffer(1024)
        rc = _capi.lib().bl_params_set_line_sweep_all(self._buf, C.byref(self.sweep_all), line.encode(), err, len(err))
        if rc != 0:
            raise _capi.BlacklightError(rc, err.value.decode())

    def set(self, key, value):
        self.set_line(f"{key} = {_format(value)}")

    def update(self, mapping):
        for key, value in mapping.items():
            self.set(key, value)
        return self

    def copy(self):
        other = Params()
        C.memmove(other._buf, self._buf, len(self._buf))
        C.memmove(C.byref(other._sweep), C.byref(self._sweep), C.sizeof(_capi.Sweep))
        C.memmove(C.byref(other._sweep_cuts), C.byref(self._sweep_cuts), C.sizeof(_capi.SweepCuts))
        C.memmove(C.byref(other._sweep_cameras), C.byref(self._sweep_cameras), C.sizeof(_capi.SweepCameras))
        C.memmove(C.byref(other._sweep_electrons), C.byref(self._sweep_electrons), C.sizeof(_capi.SweepElectrons))
        C.memmove(C.byref(other._sweep_frequencies), C.byref(self._sweep_frequencies), C.sizeof(_capi.SweepFrequencies))
        other.num_runs = self.num_runs
        return other

    # ------------------------------------------------------------------ sweeps (sweep_rat_low, sweep_rat_high, sweep_rho_cgs, sweep_cut_sigma_max)
    @property
    def sweep(self):
        """The bl_sweep filled by the sweep_* keys (what Context applies: bl_apply_sweep)."""
        return self._sweep

    @property
    def sweep_rat_low(self):
        return [float(x) for x in self._sweep.rat_low[:self._sweep.n_rat_low]]

    @property
    def sweep_rat_high(self):
        return [float(x) for x in self._sweep.rat_high[:self._sweep.n_rat_high]]

    @property
    def sweep_rho_cgs(self):
        return [float(x) for x in self._sweep.rho_cgs[:self._sweep.n_rho_cgs]]

    @property
    def sweep_cuts(self):
        """The bl_sweep_cuts filled by sweep_cut_sigma_max (what Context applies beside the sweep: bl_apply_sweeps)."""
        return self._sweep_cuts

    @property
    def sweep_cut_sigma_max(self):
        return [float(x) for x in self._sweep_cuts.sigma_max[:self._sweep_cuts.n_sigma_max]]

    @property
    def sweep_camera_lists(self):
        """The bl_sweep_cameras filled by sweep_camera_th / sweep_camera_ph (what Context applies beside the sweep: bl_apply_sweeps_cameras)."""
        return self._sweep_cameras

    @property
    def sweep_camera_th(self):
        return [float(x) for x in self._sweep_cameras.th[:self._sweep_cameras.n_th]]

    @property
    def sweep_camera_ph(self):
        return [float(x) for x in self._sweep_cameras.ph[:self._sweep_cameras.n_ph]]

    @property
    def sweep_cameras(self):
        """The cameras sweep_camera_th / sweep_camera_ph mean (bl_sweep_cameras_resolve): a list of (th, ph) in degrees, None for an
        angle that is the parameter block's own (a key that is absent); [] without the keys. Raises BlacklightError where the lists
        do not fit each other."""
        n, th_given, ph_given = C.c_int(0), C.c_int(0), C.c_int(0)
        th, ph = (C.c_double * _capi.BL_MAX_SWEEP)(), (C.c_double * _capi.BL_MAX_SWEEP)()
        err = C.create_string_buffer(1024)
        rc = _capi.lib().bl_sweep_cameras_resolve(C.byref(self._sweep_cameras), C.byref(n), th, ph, C.byref(th_given), C.byref(ph_given), err, len(err))
        if rc != 0:
            raise _capi.BlacklightError(rc, err.value.decode())
        return [(float(th[c]) if th_given.value else None, float(ph[c]) if ph_given.value else None) for c in range(n.value)]

    @property
    def sweep_lists(self):
        """A bl_sweep_lists that names this object's four structs (what the parser fills and Context applies: bl_apply_sweep_lists)."""
        return _capi.SweepLists(C.pointer(self._sweep), C.pointer(self._sweep_cuts), C.pointer(self._sweep_cameras), C.pointer(self._sweep_electrons))

    @property
    def sweep_all(self):
        """A bl_sweep_all that names this object's five structs (what the parser fills and Context applies: bl_apply_sweep_all)."""
        return _capi.SweepAll(C.pointer(self._sweep), C.pointer(self._sweep_cuts), C.pointer(self._sweep_cameras), C.pointer(self._sweep_electrons),
                              C.pointer(self._sweep_frequencies))

    @property
    def sweep_frequency_list(self):
        """The bl_sweep_frequencies filled by sweep_frequency."""
        return self._sweep_frequencies

    @property
    def sweep_frequency(self):
        """The observing frequencies of sweep_frequency as written (Hz); [] for an absent key."""
        return [float(x) for x in self._sweep_frequencies.hz[:self._sweep_frequencies.n]]

    @property
    def sweep_electron_lists(self):
        """The bl_sweep_electrons filled by sweep_power_frac ... sweep_w."""
        return self._sweep_electrons

    @property
    def sweep_electrons(self):
        """The seven electron lists as written, by the key without its sweep_ prefix: {"power_frac": [...], ...}; [] for an absent key."""
        e = self._sweep_electrons
        return {key: [float(x) for x in getattr(e, key)[:getattr(e, "n_" + key)]] for key in _capi.ELECTRON_MIX_KEYS}

    @property
    def has_sweep_electrons(self):
        return any(getattr(self._sweep_electrons, "n_" + key) > 0 for key in _capi.ELECTRON_MIX_KEYS)

    def resolved_electrons(self):
        """The tuples the electron lists and the three sweep lists mean together (bl_sweep_electrons_resolve): (rat_low, rat_high,
        rho_cgs, mixes) with one entry per variant, a mix being a mapping with Context.set_polarized_variants()'s keys; four empty lists
        when no key that makes polarized variants is written. Raises BlacklightError where the lists do not fit each other or the
        block is not polarized."""
        n = C.c_int(0)
        out = _capi.Sweep()
        mixes = (_capi.ElectronMix * _capi.BL_MAX_SWEEP)()
        err = C.create_string_buffer(1024)
        rc = _capi.lib().bl_sweep_electrons_resolve(C.byref(self._sweep_electrons), C.byref(self._sweep), self.ptr, C.byref(n), C.byref(out),
                                                    C.cast(mixes, C.c_void_p), err, len(err))
        if rc != 0:
            raise _capi.BlacklightError(rc, err.value.decode())
        count = n.value
        return ([float(x) for x in out.rat_low[:count]], [float(x) for x in out.rat_high[:count]], [float(x) for x in out.rho_cgs[:count]],
                [{key: getattr(mixes[v], key) for key in _capi.ELECTRON_MIX_KEYS} for v in range(count)])

    @property
    def has_sweep(self):
        return (self._sweep.n_rat_low > 0 or self._sweep.n_rat_high > 0 or self._sweep.n_rho_cgs > 0 or self._sweep_cuts.n_sigma_max > 0
                or self._sweep_cameras.n_th > 0 or self._sweep_cameras.n_ph > 0 or self.has_sweep_electrons or self._sweep_frequencies.n > 0)

    def resolved_sweep(self):
        """The lists as the setters receive them (bl_sweep_resolve): (polarized, rat_low, rat_high, rho_cgs). A polarized block's
        three lists have the number of triples; raises BlacklightError where the lists do not fit each other."""
        out = _capi.Sweep()
        polarized = C.c_int(0)
        err = C.create_string_buffer(1024)
        rc = _capi.lib().bl_sweep_resolve(C.byref(self._sweep), self.ptr, C.byref(out), C.byref(polarized), err, len(err))
        if rc != 0:
            raise _capi.BlacklightError(rc, err.value.decode())
        return (bool(polarized.value), [float(x) for x in out.rat_low[:out.n_rat_low]], [float(x) for x in out.rat_high[:out.n_rat_high]],
                [float(x) for x in out.rho_cgs[:out.n_rho_cgs]])

    def has(self, key):
        present = C.c_int(0)
        rc = _capi.lib().bl_params_get(self._buf, key.encode(), None, C.byref(present))
        if rc != 0:
            raise KeyError(key)
        return bool(present.value)

    def get(self, key):
        """Numeric value as stored (angles in radians, enums as their integer)."""
        value = C.c_double(0.0)
        present = C.c_int(0)
        rc = _capi.lib().bl_params_get(self._buf, key.encode(), C.byref(value), C.byref(present))
        if rc != 0:
            out = C.create_string_buffer(512)
            if _capi.lib().bl_params_get_string(self._buf, key.encode(), out, len(out)) != 0:
                raise KeyError(key)
            return out.value.decode()
        if not present.value:
            return None
        return value.value
