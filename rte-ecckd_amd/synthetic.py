"""Deterministic synthetic atmospheres for parity tests and bench.py.

No library RNG: ``u(c,f,j)`` = top 53 bits of one splitmix64 step of
``20221128 ^ (f << 56) ^ (c << 8) ^ j`` times 2**-53, so the same columns can be regenerated
bit for bit in C, Fortran or Python for any column range (column-range sharding across GPUs
needs no communication and no shared files).

Arrays follow the package convention: C order, reversed Fortran shape (``plev`` is
``(nlay+1, ncol)``).  Gas order is the RFMIP one (mo_rfmip_io.F90:204-259 / utils.f90:41-70):
co2, ch4, n2o, o2, cfc11, cfc12, h2o, o3, no2 -- no2 is unknown to the ecCKD tables and is
skipped by gas_optics (src/gas_optics_ecckd.f90:358-364).
"""
import numpy as np

SEED = 20221128
NLAY = 60
F_PS, F_TS, F_TLEV, F_TSFC, F_EMIS, F_H2O, F_O3, F_CO2, F_CH4, F_N2O, F_CFC11, F_CFC12, F_MU0, F_ALB = range(1, 15)
GAS_ORDER = ["co2", "ch4", "n2o", "o2", "cfc11", "cfc12", "h2o", "o3", "no2"]


def uniform(c, f, j):
    """u(c,f,j) in [0,1); c, j broadcastable integer arrays, f a field id."""
    with np.errstate(over="ignore"):
        x = (np.uint64(SEED) ^ (np.uint64(f) << np.uint64(56)) ^ (np.asarray(c, dtype=np.uint64) << np.uint64(8))
             ^ np.asarray(j, dtype=np.uint64))
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def columns(c0, ncol, press_min, nlay=NLAY, shortwave=False):
    """Columns ``c0 .. c0+ncol-1``.  ``press_min`` = ``ecckd%get_press_min()`` (the driver clamps
    the top level to it, ecckd_rfmip_lw.F90:90-94).  Returns a dict of float64 arrays."""
    c = np.arange(c0, c0 + ncol, dtype=np.uint64)[None, :]
    jl = np.arange(1, nlay + 2, dtype=np.uint64)[:, None]       # levels 1..nlay+1
    jm = np.arange(1, nlay + 1, dtype=np.uint64)[:, None]       # layers 1..nlay
    eta = ((np.arange(nlay + 1, dtype=np.float64)) / nlay) ** 2  # eta_j, j = 1..nlay+1
    eta = eta[:, None]
    ptop = press_min * (1 + 2.3e-16)
    ps = 95000.0 + 8000.0 * uniform(c, F_PS, 0)
    plev = ptop + (ps - ptop) * eta
    ts = 250.0 + 60.0 * uniform(c, F_TS, 0)
    tlev = ts - 70.0 * (1.0 - eta) ** 0.8 + 4.0 * (uniform(c, F_TLEV, jl) - 0.5)
    tlay = 0.5 * (tlev[1:] + tlev[:-1])
    tsfc = tlev[nlay] + 2.0 * (uniform(c, F_TSFC, 0)[0] - 0.5)
    sfc_emis = 0.95 + 0.05 * uniform(c, F_EMIS, 0)[0]
    eta_mid = 0.5 * (eta[1:] + eta[:-1])
    p_mid = 0.5 * (plev[1:] + plev[:-1])
    h2o = np.maximum(1e-7, 0.03 * uniform(c, F_H2O, jm) * eta_mid ** 3)
    o3 = 2e-8 + 8e-6 * np.exp(-((np.log(p_mid) - np.log(1000.0)) / 1.2) ** 2) * (0.5 + uniform(c, F_O3, jm))
    lin = lambda f, lo, hi: lo + (hi - lo) * uniform(c, f, 0)[0]
    out = dict(
        plev=np.ascontiguousarray(plev), tlev=np.ascontiguousarray(tlev), tlay=np.ascontiguousarray(tlay),
        tsfc=np.ascontiguousarray(tsfc), sfc_emis=np.ascontiguousarray(sfc_emis),
        h2o=np.ascontiguousarray(h2o), o3=np.ascontiguousarray(o3),
        co2=lin(F_CO2, 180e-6, 2240e-6), ch4=lin(F_CH4, 350e-9, 3500e-9), n2o=lin(F_N2O, 190e-9, 540e-9),
        cfc11=lin(F_CFC11, 0.0, 2000e-12), cfc12=lin(F_CFC12, 0.0, 550e-12), o2=0.209, no2=0.0)
    if shortwave:
        out["mu0"] = 0.05 + 0.95 * uniform(c, F_MU0, 0)[0]
        out["albedo"] = 0.05 + 0.3 * uniform(c, F_ALB, 0)[0]
        out["tsi"] = 1361.0
    return out


F_CLD_KIND, F_CLD_TAU, F_CLD_SSA, F_CLD_G = range(15, 19)


def clouds(c0, ncol, nlay, nband):
    """Particulate (cloud) optical properties on ``nband`` bands for columns ``c0 .. c0+ncol-1``, top layer first:
    a dict of float64 arrays ``tau``, ``ssa``, ``g`` of shape ``(nband, nlay, ncol)`` plus ``cloudy`` ``(ncol,)``.
    The column's ``uniform(c, F_CLD_KIND, 0)`` picks its kind -- below 0.3 a liquid-like low cloud (layers at
    0.75-0.9 of the grid, optically thick), 0.3-0.5 an ice-like high cloud (0.3-0.45 of the grid, thin), 0.5-0.6
    both, otherwise clear (``tau`` = 0 in every layer) -- so cloudy and clear columns alternate irregularly.
    ``tau`` lies in [0, 30], ``ssa`` in [0.6, 1) and falls with the band index, ``g`` in [0.7, 0.9).  ``ssa`` and
    ``g`` are defined in clear cells too (their values cannot matter where ``tau`` = 0)."""
    c = np.arange(c0, c0 + ncol, dtype=np.uint64)[None, None, :]
    jm = np.arange(1, nlay + 1, dtype=np.uint64)[None, :, None]
    band_pos = (np.arange(nband, dtype=np.float64)[:, None, None] + 1.0) / nband   # (0, 1]: the last band absorbs most
    kind = uniform(c, F_CLD_KIND, 0)
    lay = np.arange(nlay)[None, :, None]

    def slab(lo, hi):   # layers [lo*nlay, hi*nlay), at least one
        l0 = int(lo * nlay)
        return (lay >= l0) & (lay < max(l0 + 1, int(hi * nlay)))

    liquid = ((kind < 0.3) | ((kind >= 0.5) & (kind < 0.6))) & slab(0.75, 0.9)
    ice = (kind >= 0.3) & (kind < 0.6) & slab(0.3, 0.45) & ~liquid
    u_tau, u_ssa, u_g = uniform(c, F_CLD_TAU, jm), uniform(c, F_CLD_SSA, jm), uniform(c, F_CLD_G, jm)
    tau = np.where(liquid, 30.0 * u_tau ** 2, np.where(ice, 3.0 * u_tau, 0.0)) * (0.9 + 0.1 * band_pos)
    ssa = 1.0 - 0.4 * band_pos * (0.5 + 0.5 * u_ssa)
    g = np.where(liquid, 0.8, 0.7) + 0.1 * u_g + 0.0 * band_pos
    return dict(tau=np.ascontiguousarray(tau), ssa=np.ascontiguousarray(ssa), g=np.ascontiguousarray(g),
                cloudy=np.ascontiguousarray((kind < 0.6)[0, 0]))


F_CLD_FRAC = 19


def cloud_fraction(c0, ncol, nlay):
    """Layer cloud fractions ``(nlay, ncol)`` for columns ``c0 .. c0+ncol-1``, top layer first: in (0, 1] on exactly the
    layers where ``clouds`` has ``tau`` > 0, 0 elsewhere (input of ``sample_cloud_mask``)."""
    c = np.arange(c0, c0 + ncol, dtype=np.uint64)[None, :]
    jm = np.arange(1, nlay + 1, dtype=np.uint64)[:, None]
    has_cloud = clouds(c0, ncol, nlay, 1)["tau"][0] > 0.0
    return np.ascontiguousarray(np.where(has_cloud, 1.0 - uniform(c, F_CLD_FRAC, jm), 0.0))


F_CLD_LWP, F_CLD_IWP, F_CLD_RELIQ, F_CLD_REICE, F_CLD_MIXED = range(20, 25)
RADLIQ_LWR, RADLIQ_UPR, RADICE_LWR, RADICE_UPR = 2.5, 21.5, 10.0, 180.0   # microns (the ranges of RRTMGP's cloud tables)


def cloud_water(c0, ncol, nlay):
    """What a host model carries instead of ``clouds``: liquid and ice water paths ``clwp``, ``ciwp`` (g m-2) and
    effective radii ``reliq``, ``reice`` (microns), float64 ``(nlay, ncol)``, for columns ``c0 .. c0+ncol-1``, top layer
    first.  Water lies on exactly the layers where ``clouds`` has ``tau`` > 0: liquid (5-200 g m-2) in the lower part of
    the grid (from 0.6 of it down), ice (1-50 g m-2) above, and both in about a third of the liquid cells.  The radii are
    defined in every cell and lie inside the ranges of ``cloud_lut``."""
    c = np.arange(c0, c0 + ncol, dtype=np.uint64)[None, :]
    jm = np.arange(1, nlay + 1, dtype=np.uint64)[:, None]
    has_cloud = clouds(c0, ncol, nlay, 1)["tau"][0] > 0.0
    low = np.arange(nlay)[:, None] >= int(0.6 * nlay)
    mixed = uniform(c, F_CLD_MIXED, jm) < 1.0 / 3.0
    clwp = np.where(has_cloud & low, 5.0 + 195.0 * uniform(c, F_CLD_LWP, jm), 0.0)
    ciwp = np.where(has_cloud & (~low | mixed), 1.0 + 49.0 * uniform(c, F_CLD_IWP, jm), 0.0)
    reliq = RADLIQ_LWR + (RADLIQ_UPR - RADLIQ_LWR) * uniform(c, F_CLD_RELIQ, jm)
    reice = RADICE_LWR + (RADICE_UPR - RADICE_LWR) * uniform(c, F_CLD_REICE, jm)
    return tuple(np.ascontiguousarray(a) for a in (clwp, ciwp, reliq, reice))


def cloud_lut(nband, nsize_liq, nsize_ice, nrghice):
    """Smooth analytic cloud-optics tables in the layout of ``CloudOptics.load_lut``: a dict with the radius bounds
    ``radliq_lwr``, ``radliq_upr``, ``radice_lwr``, ``radice_upr`` (microns), the liquid tables ``lut_extliq``,
    ``lut_ssaliq``, ``lut_asyliq`` ``(nband, nsize_liq)`` and the ice tables ``lut_extice``, ``lut_ssaice``, ``lut_asyice``
    ``(nrghice, nband, nsize_ice)``, float64.  ``ext`` (m2 g-1) falls with the size like 1.5/r (liquid) or 1.6/r (ice)
    times a band factor, ``ssa`` lies in (0.5, 1) and falls with size and band, ``asy`` in (0.7, 0.95) and rises with size;
    rougher ice is a little less forward-scattering.  Every quantity is strictly monotonic in the size, so the slope is
    non-zero in every interval and a wrong index or a wrong weight shows."""
    band = (np.arange(nband, dtype=np.float64)[:, None] + 1.0) / nband   # (0, 1]

    def tables(r_lwr, r_upr, nsize, c_ext, rough):
        r = np.linspace(r_lwr, r_upr, nsize)[None, :]
        x = (r - r_lwr) / (r_upr - r_lwr)                                # [0, 1]
        ext = c_ext / r * (0.8 + 0.4 * band)
        ssa = 0.99 - 0.4 * band * (0.3 + 0.7 * x) - 0.02 * rough
        asy = 0.74 + 0.18 * x + 0.02 * band - 0.015 * rough
        return ext, ssa, asy

    liq = tables(RADLIQ_LWR, RADLIQ_UPR, nsize_liq, 1.5, 0.0)
    ice = [tables(RADICE_LWR, RADICE_UPR, nsize_ice, 1.6, float(k) / max(1, nrghice)) for k in range(nrghice)]
    out = dict(radliq_lwr=RADLIQ_LWR, radliq_upr=RADLIQ_UPR, radice_lwr=RADICE_LWR, radice_upr=RADICE_UPR)
    for i, q in enumerate(("ext", "ssa", "asy")):
        out["lut_" + q + "liq"] = np.ascontiguousarray(liq[i])
        out["lut_" + q + "ice"] = np.ascontiguousarray(np.stack([t[i] for t in ice]))
    return out


F_AER_COL, F_AER_CELL, F_AER_ODD, F_AER_KIND, F_AER_SIZE, F_AER_MASS, F_AER_RH = range(25, 32)
AERO_SIZE_LWR, AERO_SIZE_UPR = 0.1, 10.0   # microns: the span of the bins of ``aerosol_lut`` (MERRA's dust bins span it)


def aerosol_lut(nband, nbin, nrh):
    """Smooth analytic aerosol-optics tables in the layout (and with the argument names) of ``AerosolOptics.load``: a dict
    with ``merra_aero_bin_lims`` ``(nbin, 2)`` (microns; contiguous bins, geometric between 0.1 and 10), ``aero_rh``
    ``(nrh,)`` (unevenly spaced like MERRA's: the first half of the levels coarse from 0 up to 0.8, the rest fine from
    0.8 to 0.99), ``aero_dust_tbl`` ``(nband, nbin, 3)``, ``aero_salt_tbl`` ``(nband, nbin, nrh, 3)``, ``aero_sulf_tbl``,
    ``aero_bcar_rh_tbl``, ``aero_ocar_rh_tbl`` ``(nband, nrh, 3)`` and ``aero_bcar_tbl``, ``aero_ocar_tbl`` ``(nband, 3)``,
    float64; the last axis is mass extinction (m2 kg-1), ssa, asymmetry.  Every quantity rises strictly with the humidity
    (hygroscopic growth) and differs between bins, bands and types, so a wrong index, weight, bin or type shows."""
    edges = AERO_SIZE_LWR * (AERO_SIZE_UPR / AERO_SIZE_LWR) ** (np.arange(nbin + 1, dtype=np.float64) / nbin)
    lims = np.stack([edges[:-1], edges[1:]], axis=1)
    ncoarse = nrh // 2
    rh = np.concatenate([np.linspace(0.0, 0.8, ncoarse, endpoint=False), np.linspace(0.8, 0.99, nrh - ncoarse)])
    band = ((np.arange(nband, dtype=np.float64) + 1.0) / nband)[:, None, None]   # (0, 1]
    binpos = (np.arange(nbin, dtype=np.float64) / nbin)[None, :, None]           # [0, 1)
    hum = rh[None, None, :]

    def table(k, c_ext, growth, ssa0):   # (nband, nbin, nrh, 3) of type code k
        ext = c_ext * (0.6 + 0.4 * band) / (1.0 + 4.0 * binpos) * (1.0 + growth * hum / (1.05 - hum))
        ssa = ssa0 - 0.2 * band - 0.02 * binpos + 0.08 * hum
        asy = 0.6 + 0.03 * k + 0.02 * band + 0.05 * binpos + 0.1 * hum
        return np.ascontiguousarray(np.stack(np.broadcast_arrays(ext, ssa, asy), axis=-1))

    dust = table(1, 600.0, 0.0, 0.90)
    salt = table(2, 900.0, 1.0, 0.88)
    sulf = table(3, 3000.0, 0.8, 0.86)
    bcar_rh = table(4, 9000.0, 0.3, 0.35)
    bcar = table(5, 8000.0, 0.0, 0.30)
    ocar_rh = table(6, 4000.0, 0.5, 0.80)
    ocar = table(7, 3500.0, 0.0, 0.75)
    c = np.ascontiguousarray
    return dict(merra_aero_bin_lims=c(lims), aero_rh=c(rh), aero_dust_tbl=c(dust[:, :, 0, :]), aero_salt_tbl=salt,
                aero_sulf_tbl=c(sulf[:, 0, :, :]), aero_bcar_tbl=c(bcar[:, 0, 0, :]), aero_bcar_rh_tbl=c(bcar_rh[:, 0, :, :]),
                aero_ocar_tbl=c(ocar[:, 0, 0, :]), aero_ocar_rh_tbl=c(ocar_rh[:, 0, :, :]))


def aerosols(c0, ncol, nlay, nspec):
    """What a host model carries for its aerosol tracers, for columns ``c0 .. c0+ncol-1``, top layer first: ``aero_type``
    int32, ``aero_size`` (microns) and ``aero_mass`` (kg m-2), ``(nspec, nlay, ncol)``, and ``relhum`` ``(nlay, ncol)`` in
    [0, 1).  Plane ``s`` is mostly one type, ``1 + s % 7``: dust lies aloft (0.3-0.7 of the grid) in about 0.4 of the
    columns, sea salt and sulfate in the lowest third in about 0.6 of them, the carbons in the lower half in about 0.3;
    inside its slab a species fills four cells in five, and one such cell in ten holds a type drawn from all seven
    instead.  Every other cell holds none (type 0, mass 0): well over a third of all cells.  Masses are 1e-6 to 1e-4
    kg m-2; sizes are defined in every cell, log-uniform over the bins of ``aerosol_lut``."""
    s = np.arange(nspec, dtype=np.uint64)[:, None, None]
    c = np.arange(c0, c0 + ncol, dtype=np.uint64)[None, None, :]
    jm = np.arange(1, nlay + 1, dtype=np.uint64)[None, :, None]
    js = jm | (s << np.uint64(40))                         # one stream position per (species, layer): above the column's bits
    main = (1 + np.arange(nspec) % 7)[:, None, None]
    lay = np.arange(nlay)[None, :, None]

    def slab(lo, hi):   # layers [lo*nlay, hi*nlay), at least one
        l0 = min(int(lo * nlay), nlay - 1)
        return (lay >= l0) & (lay < max(l0 + 1, int(hi * nlay)))

    where = np.where(main == 1, slab(0.3, 0.7), np.where(main <= 3, slab(2.0 / 3.0, 1.0), slab(0.5, 1.0)))
    share = np.where(main == 1, 0.4, np.where(main <= 3, 0.6, 0.3))
    present = where & (uniform(c, F_AER_COL, s) < share) & (uniform(c, F_AER_CELL, js) < 0.8)
    odd = uniform(c, F_AER_ODD, js) < 0.1
    other = 1 + np.minimum(6, np.floor(7.0 * uniform(c, F_AER_KIND, js)).astype(np.int64))
    aero_type = np.where(present, np.where(odd, other, main), 0).astype(np.int32)
    aero_mass = np.where(present, 1e-6 * 100.0 ** uniform(c, F_AER_MASS, js), 0.0)
    aero_size = AERO_SIZE_LWR * (AERO_SIZE_UPR / AERO_SIZE_LWR) ** uniform(c, F_AER_SIZE, js)
    relhum = uniform(c[0], F_AER_RH, jm[0]) ** 0.7
    return tuple(np.ascontiguousarray(a) for a in (aero_type, aero_size, aero_mass, relhum))


def gas_items(cols):
    """[(name, array, col_stride, lay_stride)] in GAS_ORDER for oracle-style consumers: full
    arrays are (nlay,ncol) -> strides (1,ncol); per-column arrays (1,0); scalars (0,0)."""
    ncol = cols["plev"].shape[1]
    items = []
    for n in GAS_ORDER:
        v = cols[n]
        if np.isscalar(v):
            items.append((n, np.array([v], dtype=np.float64), 0, 0))
        elif v.ndim == 1:
            items.append((n, v, 1, 0))
        else:
            items.append((n, v, 1, ncol))
    return items
