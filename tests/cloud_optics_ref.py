"""numpy restatement of ``ecckd_cloud_optics`` (include/ecckd_hip.h, "Cloud optics"), written from the header's text.

Every line of the definition is one ufunc on arrays of the call's precision, so numpy evaluates it with one correctly
rounded IEEE operation per line, as the library does (its build has FMA contraction off): the results are compared BIT
FOR BIT, in float64 and in float32.  Arrays follow the package convention (C order, reversed Fortran shapes): inputs
``(nlay, ncol)``, liquid tables ``(nband, nsize)``, ice tables ``(nrghice, nband, nsize)``, planes ``(nband, nlay, ncol)``.
"""
import numpy as np


def _phase(wp, re, r_lwr, r_upr, ext, ssa, asy, dtype):
    """(t, ts, tsg), each (nband, nlay, ncol), of one phase; the tables (nband, nsize)."""
    real = dtype.type
    ext, ssa, asy = (np.asarray(t, dtype=np.float64).astype(dtype) for t in (ext, ssa, asy))   # rounded first
    nsize = ext.shape[1]
    r_lwr, r_upr = real(r_lwr), real(r_upr)
    step = (r_upr - r_lwr) / real(nsize - 1)
    cloudy = wp > real(0)                                        # NaN, 0, negative: not cloudy
    with np.errstate(all="ignore"):
        s = (re - r_lwr) / step
        f1 = np.floor(s) + real(1)
        index = np.where(f1 >= real(nsize - 1), nsize - 1, np.where(f1 >= real(1), f1, 1)).astype(np.int64)   # NaN: 1
        fint = s - (index - 1).astype(dtype)
        i0 = index - 1                                           # 0-based
        out = []
        factor = wp[None]
        for table in (ext, ssa, asy):
            slope = table[:, 1:] - table[:, :-1]
            value = table[:, i0] + fint[None] * slope[:, i0]     # (nband, nlay, ncol)
            factor = factor * value
            out.append(np.where(cloudy[None], factor, real(0)))  # a select, not a product
    return out


def cloud_optics(clwp, ciwp, reliq, reice, lut, icergh=1, two_stream=True, dtype=np.float64):
    """``lut``: the dict of ``synthetic.cloud_lut`` (bounds and float64 tables).  Returns ``(tau, ssa, g)`` or, with
    ``two_stream=False``, the absorption optical depth ``tau`` alone; arrays of ``dtype``."""
    dtype = np.dtype(dtype)
    real = dtype.type
    clwp, ciwp, reliq, reice = (np.asarray(a, dtype=dtype) for a in (clwp, ciwp, reliq, reice))
    lt, lts, ltsg = _phase(clwp, reliq, lut["radliq_lwr"], lut["radliq_upr"], lut["lut_extliq"], lut["lut_ssaliq"],
                           lut["lut_asyliq"], dtype)
    r = icergh - 1
    it, its, itsg = _phase(ciwp, reice, lut["radice_lwr"], lut["radice_upr"], lut["lut_extice"][r], lut["lut_ssaice"][r],
                           lut["lut_asyice"][r], dtype)
    if not two_stream:
        return (lt - lts) + (it - its)
    eps = real(np.finfo(dtype).eps)
    floor_eps = lambda x: np.where(x > eps, x, eps)              # max(eps, x); a NaN gives eps
    tau = lt + it
    tssa = lts + its
    with np.errstate(all="ignore"):
        g = (ltsg + itsg) / floor_eps(tssa)
        ssa = tssa / floor_eps(tau)
    return tau, ssa, g
