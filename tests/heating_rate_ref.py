"""numpy restatement of ``ecckd_heating_rate`` (include/ecckd_hip.h, "Heating rates"): one numpy operation per line of the
definition, every operand and every result an array of the call's dtype, so that in ``float32`` no intermediate is ever a
``float64``.  numpy's elementwise subtract, multiply and divide are the correctly rounded IEEE operations; nothing is fused."""
import numpy as np

GRAV, CP_DRY = 9.80665, 1004.64


def heating_rate(flux_up, flux_dn, plev, cp=None, grav=GRAV, cp_dry=CP_DRY, dtype=None):
    """``flux_up``, ``flux_dn``: ``(nlay+1, ncol)`` or ``(nouter, nlay+1, ncol)``; ``plev``: ``(nlay+1, ncol)``; ``cp``:
    ``(nlay, ncol)`` or None.  Returns ``(nlay, ncol)`` / ``(nouter, nlay, ncol)`` of ``dtype`` (default: that of ``flux_up``).
    ``grav`` and ``cp_dry`` are rounded to ``dtype`` once."""
    dtype = np.dtype(flux_up.dtype if dtype is None else dtype)
    assert dtype in (np.dtype(np.float32), np.dtype(np.float64))
    fu, fd, p = (np.asarray(a).astype(dtype, copy=False) for a in (flux_up, flux_dn, plev))
    g = np.full((), grav, dtype=dtype)
    with np.errstate(all="ignore"):
        du = np.subtract(fu[..., 1:, :], fu[..., :-1, :], dtype=dtype)
        dd = np.subtract(fd[..., 1:, :], fd[..., :-1, :], dtype=dtype)
        dnet = np.subtract(du, dd, dtype=dtype)
        dp = np.subtract(p[1:, :], p[:-1, :], dtype=dtype)
        c = np.full(dp.shape, cp_dry, dtype=dtype) if cp is None else np.asarray(cp).astype(dtype, copy=False)
        num = np.multiply(dnet, g, dtype=dtype)
        den = np.multiply(c, dp, dtype=dtype)
        out = np.divide(num, den, dtype=dtype)
    assert out.dtype == dtype
    return out


def bits(a):
    """The array's bit patterns (uint64 / uint32), for bit-for-bit comparisons that tell -0 from +0 and compare NaNs."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def inputs(seed, ncol, nlay, nouter, dtype, with_cp):
    """Random fluxes of 0-500 W m-2, monotone pressures with layer thicknesses from 1 Pa to 5 kPa (log-uniform), and
    optionally a moist cp of 1004-1050 J kg-1 K-1.  ``nouter`` None: rank-2 fluxes."""
    rng = np.random.default_rng(seed)
    shape = ((nouter,) if nouter is not None else ()) + (nlay + 1, ncol)
    fu = rng.uniform(0.0, 500.0, shape).astype(dtype)
    fd = rng.uniform(0.0, 500.0, shape).astype(dtype)
    thick = np.exp(rng.uniform(np.log(1.0), np.log(5000.0), (nlay, ncol)))
    plev = (10.0 + np.concatenate([np.zeros((1, ncol)), np.cumsum(thick, axis=0)], axis=0)).astype(dtype)
    cp = rng.uniform(1004.0, 1050.0, (nlay, ncol)).astype(dtype) if with_cp else None
    return fu, fd, plev, cp
