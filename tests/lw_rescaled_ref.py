"""The rescaled no-scattering longwave solver (ecckd_rte_lw_rescaled; RTE-RRTMGP's lw_solver_1rescl_GaussQuad, after Tang et
al. 2018, J. Atmos. Sci. 75, 2217) in numpy float64: the equations of include/ecckd_hip.h operation by operation, sharing
no code with the library.

Per (column, g-point, quadrature angle k), layers s = 0 .. nlay-1 counted from the top, level s the top of layer s:

    wb  = ssa*(1 - g)*0.5            sc = (1 - ssa) + wb          tl = (tau*sc)*D_k        t = exp(-tl)
    Cn  = 0.4*(wb/sc)                CA = Cn*(1 - t*t)
    sdn, sup: lw_source_noscat on tl (series below tau_thresh)
    SUA = sup - Cn*(sdn*t + sup)     SDA = sdn - Cn*(sup*t + sdn)
    sweep 1   dn0[s+1] = t*dn0[s] + sdn                      dn0[0] from inc_flux
    surface   up[nlay] = dn0[nlay]*(1 - emis) + emis*sfc_source
    sweep 2   up[s]    = t*up[s+1] + (SUA + CA*dn0[s])
    sweep 3   dn[s+1]  = t*dn[s]   + (SDA + CA*up[s+1])      dn[0] = dn0[0]
    flux = 2*pi*w_k * radiance, summed over the angles in order

Arrays follow the project's layout: tau / ssa / g / lay / inc / dec (ng, nlay, ncol), boundary values (ng, ncol), fluxes
(ng, nlay + 1, ncol), in the memory order that goes with `top_at_1`.  `inc` is the source at the level after the layer in
memory, `dec` at the level before it.  scale = False: no scaling at all -- the absorption-only fluxes when called on
tau*(1 - ssa).  `variant` names deliberately wrong forms for the test of what the method is for.
"""
import math

import numpy as np

GAUSS_DS = [[1.66], [1.18350343, 2.81649655], [1.09719858, 1.69338507, 4.70941630],
            [1.06056257, 1.38282560, 2.40148179, 7.15513024]]
GAUSS_WTS = [[0.5], [0.3180413817, 0.1819586183], [0.2009319137, 0.2292411064, 0.0698269799],
             [0.1355069134, 0.2034645680, 0.1298475476, 0.0311809710]]
TAU_THRESH = math.sqrt(2.220446049250313e-16)

_exp = np.vectorize(math.exp, otypes=[np.float64])   # the C library's exp: the same bits wherever numpy runs


def restate(tau, ssa, g, lay, inc, dec, sfc_emis, sfc_source, inc_flux=None, top_at_1=True, nmus=1, scale=True,
            tau_thresh=TAU_THRESH, series_terms=2, inc_isotropic=False, variant=None):
    """Spectral fluxes (up, dn), each (ng, nlay + 1, ncol) in memory order.  sfc_emis, sfc_source, inc_flux: (ng, ncol)."""
    tau, ssa, g, lay, inc, dec = (np.asarray(a, dtype=np.float64) for a in (tau, ssa, g, lay, inc, dec))
    emis, bsfc = np.asarray(sfc_emis, dtype=np.float64), np.asarray(sfc_source, dtype=np.float64)
    ng, nlay, ncol = tau.shape
    if top_at_1:
        bdn, bup = inc, dec          # the source at the level below / above the layer
    else:
        tau, ssa, g, lay = tau[:, ::-1], ssa[:, ::-1], g[:, ::-1], lay[:, ::-1]
        bdn, bup = dec[:, ::-1], inc[:, ::-1]
    pi = math.pi
    up, dn = np.zeros((ng, nlay + 1, ncol)), np.zeros((ng, nlay + 1, ncol))
    with np.errstate(all="ignore"):
        if scale:
            wb = ssa * (1.0 - g) * 0.5
            sc = (1.0 - ssa) + wb
            taus = tau * sc
            Cn = (1.0 if variant == "no_0.4" else 0.4) * (wb / sc)
            if variant == "wrong_sign":
                Cn = -Cn
        else:
            taus, Cn = tau, np.zeros_like(tau)
        for k in range(nmus):
            D, w = GAUSS_DS[nmus - 1][k], GAUSS_WTS[nmus - 1][k]
            tl = taus * D
            t = _exp(-tl)
            CA = Cn * (1.0 - t * t)
            omt = 1.0 - t
            if series_terms == 3:
                series = tl * (0.5 + tl * (-1.0 / 3.0 + tl * (1.0 / 8.0)))
            else:
                series = tl * (0.5 - 1.0 / 3.0 * tl)
            fact = np.where(tl > tau_thresh, omt / tl - t, series)
            sdn = omt * bdn + 2.0 * fact * (lay - bdn)
            sup = omt * bup + 2.0 * fact * (lay - bup)
            SUA = sup - Cn * (sdn * t + sup)
            SDA = sdn - Cn * (sup * t + sdn)
            dn0 = np.empty((ng, nlay + 1, ncol))
            if inc_flux is None:
                dn0[:, 0] = 0.0
            else:
                f = np.asarray(inc_flux, dtype=np.float64)
                dn0[:, 0] = f / pi if inc_isotropic else f / (2.0 * pi * w)
            for s in range(nlay):
                dn0[:, s + 1] = t[:, s] * dn0[:, s] + sdn[:, s]
            ru = np.empty((ng, nlay + 1, ncol))
            ru[:, nlay] = dn0[:, nlay] * (1.0 - emis) + emis * bsfc
            for s in range(nlay - 1, -1, -1):
                ru[:, s] = t[:, s] * ru[:, s + 1] + (SUA[:, s] + CA[:, s] * dn0[:, s])
            rd = np.empty((ng, nlay + 1, ncol))
            rd[:, 0] = dn0[:, 0]
            if variant == "no_third_sweep":
                rd = dn0
            else:
                for s in range(nlay):
                    rd[:, s + 1] = t[:, s] * rd[:, s] + (SDA[:, s] + CA[:, s] * ru[:, s + 1])
            wfac = 2.0 * pi * w
            up = wfac * ru if k == 0 else up + wfac * ru
            dn = wfac * rd if k == 0 else dn + wfac * rd
    if not top_at_1:
        up, dn = up[:, ::-1], dn[:, ::-1]
    return np.ascontiguousarray(up), np.ascontiguousarray(dn)


def flip_orientation(a):
    """lw_2stream_ref.flip_orientation, and lay_source (which the two-stream solver does not have) reversed with the layers."""
    import lw_2stream_ref
    out = lw_2stream_ref.flip_orientation(a)
    out["lay"] = np.flip(a["lay"], axis=1).copy(order="C")
    return out


def broadband(spectral):
    """Sum of (ng, nlev, ncol) over the g-points, in g-point order."""
    out = np.zeros(spectral.shape[1:])
    for k in range(spectral.shape[0]):
        out = out + spectral[k]
    return out
