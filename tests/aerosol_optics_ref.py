"""The definition of ``ecckd_aerosol_optics`` (include/ecckd_hip.h, "Aerosol optics") restated in numpy: one numpy operation
per line of the header's text, in the dtype asked for, so that the results are those of a correctly rounded IEEE evaluation
in that precision and the GPU kernels can be held to them bit for bit.  Shared by the aerosol-optics tests; not a test."""
import numpy as np

RH_DEPENDENT = (2, 3, 4, 6)   # sea salt, sulfate, black carbon hydrophilic, organic carbon hydrophilic


def increment_eps(dt):
    """3 * tiny(1.0): the floor of ``ecckd_increment``'s denominators"""
    return dt(3) * dt(np.finfo(dt).tiny)


def floor_at(e, x):
    """max(e, x) as the header spells it: x where x > e, else e (a NaN gives e)"""
    return np.where(x > e, x, e)


def image_bytes(nband, nbin, nrh, two_stream, f32):
    """the header's image size formula"""
    entries = nbin * nrh + 3 * (nrh - 1) + 2
    return (3 if two_stream else 2) * nband * entries * 2 * (4 if f32 else 8)


def interval_and_weight(rh_levels, relhum):
    """0-based interval ``i`` and weight ``w`` of every cell; rh_levels and relhum already in the dtype of the call"""
    dt = relhum.dtype.type
    d = rh_levels[1:] - rh_levels[:-1]
    i = np.zeros(relhum.shape, dtype=np.int64)
    for j in range(1, len(rh_levels) - 1):
        i = i + (relhum >= rh_levels[j])
    with np.errstate(all="ignore"):
        w = (relhum - rh_levels[i]) / d[i]
    w = np.where(w > 0, w, dt(0))
    w = np.where(w < 1, w, dt(1))
    return i, w


def aerosol_optics(lut, aero_type, aero_size, aero_mass, relhum, two_stream, dtype=np.float64, op1=None):
    """``lut``: the dict of ``synthetic.aerosol_lut`` (the arguments of ``AerosolOptics.load``); species arrays
    ``(nspec, nlay, ncol)`` or ``(nlay, ncol)``; ``relhum`` ``(nlay, ncol)``.  Returns ``(tau, ssa, g)`` or ``(tau,)``,
    ``(nband, nlay, ncol)`` in ``dtype``.  ``op1``: the planes an ``accumulate`` call finds -- the result is then what it
    leaves, by ``ecckd_increment``'s formulas."""
    dt = np.dtype(dtype).type
    k3 = np.asarray(aero_type)
    if k3.ndim == 2:
        k3, aero_size, aero_mass = k3[None], np.asarray(aero_size)[None], np.asarray(aero_mass)[None]
    r3, m3 = np.asarray(aero_size).astype(dt), np.asarray(aero_mass).astype(dt)
    rh = np.asarray(relhum).astype(dt)
    lims = lut["merra_aero_bin_lims"].astype(dt)
    lev = lut["aero_rh"].astype(dt)
    dust, salt, sulf = (lut[n].astype(dt) for n in ("aero_dust_tbl", "aero_salt_tbl", "aero_sulf_tbl"))
    bcar, bcar_rh, ocar, ocar_rh = (lut[n].astype(dt) for n in ("aero_bcar_tbl", "aero_bcar_rh_tbl", "aero_ocar_tbl",
                                                                "aero_ocar_rh_tbl"))
    nband, nbin = dust.shape[0], dust.shape[1]
    i, w = interval_and_weight(lev, rh)
    shape = (nband,) + rh.shape
    T, TS, TSG, A = (np.zeros(shape, dtype=dt) for _ in range(4))
    with np.errstate(all="ignore"):
        for s in range(k3.shape[0]):
            k, m, r = k3[s], m3[s], r3[s]
            active = (k >= 1) & (k <= 7) & (m > 0)
            b = np.full(k.shape, -1, dtype=np.int64)
            for n in range(nbin - 1, -1, -1):
                b = np.where((lims[n, 0] <= r) & (r < lims[n, 1]), n, b)
            active = active & ~(((k == 1) | (k == 2)) & (b < 0))
            bc = np.maximum(b, 0)
            v = []
            for q in range(3):
                salt_v = salt[:, bc, i, q] + w * (salt[:, bc, i + 1, q] - salt[:, bc, i, q])
                sulf_v = sulf[:, i, q] + w * (sulf[:, i + 1, q] - sulf[:, i, q])
                bcrh_v = bcar_rh[:, i, q] + w * (bcar_rh[:, i + 1, q] - bcar_rh[:, i, q])
                ocrh_v = ocar_rh[:, i, q] + w * (ocar_rh[:, i + 1, q] - ocar_rh[:, i, q])
                fixed = [dust[:, bc, q], np.broadcast_to(bcar[:, q][:, None, None], shape),
                         np.broadcast_to(ocar[:, q][:, None, None], shape)]
                v.append(np.select([k == 1, k == 2, k == 3, k == 4, k == 5, k == 6, k == 7],
                                   [fixed[0], salt_v, sulf_v, bcrh_v, fixed[1], ocrh_v, fixed[2]], default=dt(0)).astype(dt))
            t = m * v[0]
            ts = t * v[1]
            tsg = ts * v[2]
            t, ts, tsg = (np.where(active, x, dt(0)) for x in (t, ts, tsg))
            T = T + t
            TS = TS + ts
            TSG = TSG + tsg
            A = A + (t - ts)
        e = dt(np.finfo(dt).eps)
        if two_stream:
            tau2 = T
            ssa2 = TS / floor_at(e, T)
            g2 = TSG / floor_at(e, TS)
            if op1 is None:
                return tau2, ssa2, g2
            tau1, ssa1, g1 = (np.asarray(x).astype(dt) for x in op1)
            e3 = increment_eps(dt)
            tau12 = tau1 + tau2
            tscat1 = tau1 * ssa1
            tscat2 = tau2 * ssa2
            tsg2 = tscat2 * g2
            tauscat12 = tscat1 + tscat2
            g12 = (tscat1 * g1 + tsg2) / floor_at(e3, tauscat12)
            ssa12 = tauscat12 / floor_at(e3, tau12)
            return tau12, ssa12, g12
        if op1 is None:
            return (A,)
        return (np.asarray(op1[0]).astype(dt) + A,)
