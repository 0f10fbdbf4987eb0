"""Total flux of a rendered image, as the reference's post-processing computes it.

The reference reads an image back from its output file and sums it in scripts/calculate_flux.py: the mean intensity over the
root image's pixels, NaN pixels left out (:157), times the solid angle of the square camera, whose side subtends
w = 2 atan(camera_width r_g / (2 D)) with r_g = G M / c^2 (:149), in Jy. This module does the same for a root-level image row
of bl_render - one variant's rows, e.g. render()["image_by_unit"][m, u] - without a file in between (Context.fit_density_unit).
"""
import math

import numpy as np

# the reference script's constants (cgs)
C_CGS = 2.99792458e10
GG_MSUN_CGS = 1.32712440018e26   # G M_sun
PC_CGS = 9.69394202136e18 / math.pi
JY_CGS = 1.0e-23


def camera_solid_angle(params, distance_pc):
    """w^2: the solid angle (sr) of a root-level camera of camera_width gravitational radii at distance_pc parsecs."""
    width_rg = float(params.get("camera_width"))
    mass_msun = params.get("simulation_m_msun")
    if mass_msun is None:
        raise ValueError("total flux: the parameter block has no simulation_m_msun")
    if not distance_pc > 0.0:
        raise ValueError("total flux: distance_pc must be > 0")
    r_g = GG_MSUN_CGS * float(mass_msun) / C_CGS ** 2
    width = 2.0 * math.atan(0.5 * width_rg * r_g / (float(distance_pc) * PC_CGS))
    return width * width


def total_flux_jy(image_rows, params, distance_pc, frequency=0):
    """Total flux (Jy) of row `frequency` (I_nu at the image's frequency number `frequency`) of one root-level image:
    image_rows is (n_q, n_pixels) - or (n_pixels,) for one row - in bl_render's units, erg / (s cm^2 sr Hz)."""
    rows = np.asarray(image_rows, dtype=np.float64)
    intensity = rows if rows.ndim == 1 else rows[frequency]
    if intensity.size == 0 or np.isnan(intensity).all():
        return math.nan
    return float(np.nanmean(intensity)) * camera_solid_angle(params, distance_pc) / JY_CGS


def stokes_flux_jy(image_rows, params, distance_pc, frequency=0):
    """(I, Q, U, V) in Jy of a polarized root-level image at the image's frequency number `frequency`: rows 4 f .. 4 f + 3 of
    image_rows (n_q, n_pixels), each summed as total_flux_jy sums a row - the mean over the pixels that are not NaN in that row."""
    rows = np.asarray(image_rows, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[0] < 4 * frequency + 4:
        raise ValueError(f"stokes flux: image rows {rows.shape} hold no Stokes rows of frequency {frequency}")
    return tuple(total_flux_jy(rows[4 * frequency + s], params, distance_pc) for s in range(4))


def net_polarization(stokes):
    """(m_net, v_net, evpa_rad) = (hypot(Q, U) / I, V / I, atan2(U, Q) / 2) of the fluxes (I, Q, U, V) stokes_flux_jy returns."""
    i, q, u, v = (float(x) for x in stokes)
    return math.hypot(q, u) / i, v / i, 0.5 * math.atan2(u, q)
