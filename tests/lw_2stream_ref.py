"""The two-stream longwave solver (ecckd_rte_lw_2stream) twice over, sharing no expression:

* restate: the solver's own expressions (include/ecckd_hip.h) in numpy float64, in the order spelt there --
  two-stream reflectance / transmittance closed form, layer sources, adding upwards, fluxes downwards;
* truth: the two-stream equations with a source linear in optical depth as a boundary-value problem in multi-digit
  arithmetic (mpmath, imported inside the function: the GPU suite needs numpy only).  State y = [F_up, F_dn], tau
  increasing downwards, y' = M y + s inside a layer with

      M = [[g1, -g2],        g1 = D (1 - w (1 + g) / 2)      s = (g1 - g2) pi B [-1, +1]
           [g2, -g1]]        g2 = D w (1 - g) / 2            B linear in tau between the level values

  A layer is crossed with mpmath.expm(M tau) applied to the departure from the particular solution
  pi B +- pi B' / (g1 + g2); F_up(top) is found by linear shooting from F_dn(top) = inc_flux to
  F_up(sfc) = (1 - emis) F_dn(sfc) + pi emis B_sfc.  Shooting loses sum(k tau) / ln 10 digits (k^2 = g1^2 - g2^2), so the
  working precision is `dps` plus that many, as solver_truth.sw_truth does.  No Rdif / Tdif closed form, no adding
  recurrence, no floor on k^2 and no optical depth below which a layer stops emitting.

Arrays follow the project's layout: tau / ssa / g / inc / dec (ng, nlay, ncol), boundary values (ng, ncol), fluxes
(ng, nlay + 1, ncol), in the memory order that goes with `top_at_1`.  The level source at memory level j (0-based) is
dec[j] at j = 0, inc[nlay - 1] at j = nlay and sqrt(dec[j] inc[j - 1]) in between, whatever top_at_1 is.
"""
import math

import numpy as np

D = 1.66
K_FLOOR = 1e-12      # lower bound of k^2 in the solver
TAU_MIN = 1e-8       # a layer at or below this optical depth emits nothing in the solver

_exp = np.vectorize(math.exp, otypes=[np.float64])   # the C library's exp: the same bits wherever numpy runs


def level_sources(inc, dec):
    """(ng, nlay + 1, ncol) from the two (ng, nlay, ncol) arrays, by memory index."""
    inc, dec = np.asarray(inc, dtype=np.float64), np.asarray(dec, dtype=np.float64)
    ng, nlay, ncol = inc.shape
    lev = np.empty((ng, nlay + 1, ncol))
    lev[:, 0] = dec[:, 0]
    lev[:, nlay] = inc[:, nlay - 1]
    lev[:, 1:nlay] = np.sqrt(dec[:, 1:] * inc[:, :-1])
    return lev


def flip_orientation(a):
    """A dict of solver inputs stored the other way up: layers reversed, lev_source_inc and lev_source_dec exchanged
    (inc is the source at the level after the layer in memory)."""
    f = lambda x: np.flip(x, axis=1).copy(order="C")
    out = dict(a)
    out.update(tau=f(a["tau"]), ssa=f(a["ssa"]), g=f(a["g"]), inc=f(a["dec"]), dec=f(a["inc"]))
    return out


def restate(tau, ssa, g, inc, dec, sfc_emis, sfc_source, inc_flux=None, top_at_1=True):
    """Spectral fluxes (up, dn), each (ng, nlay + 1, ncol) in memory order.  sfc_emis, sfc_source, inc_flux: (ng, ncol)."""
    tau, ssa, g = (np.asarray(a, dtype=np.float64) for a in (tau, ssa, g))
    emis, bsfc = np.asarray(sfc_emis, dtype=np.float64), np.asarray(sfc_source, dtype=np.float64)
    ng, nlay, ncol = tau.shape
    lev = level_sources(inc, dec)
    if not top_at_1:
        tau, ssa, g, lev = tau[:, ::-1], ssa[:, ::-1], g[:, ::-1], lev[:, ::-1]
    pi = math.pi
    with np.errstate(all="ignore"):
        gamma1 = D * (1.0 - 0.5 * ssa * (1.0 + g))
        gamma2 = D * 0.5 * ssa * (1.0 - g)
        k = np.sqrt(np.maximum((gamma1 - gamma2) * (gamma1 + gamma2), K_FLOOR))
        e1 = _exp(-tau * k)
        e2 = e1 * e1
        RT = 1.0 / (k * (1.0 + e2) + gamma1 * (1.0 - e2))
        Rdif = RT * gamma2 * (1.0 - e2)
        Tdif = RT * 2.0 * k * e1
        Bt, Bb = lev[:, :-1], lev[:, 1:]
        Z = (Bb - Bt) / (tau * (gamma1 + gamma2))
        su = pi * ((Z + Bt) - Rdif * (-Z + Bt) - Tdif * (Z + Bb))
        sd = pi * ((-Z + Bb) - Rdif * (Z + Bb) - Tdif * (-Z + Bt))
        thick = tau > TAU_MIN
        su, sd = np.where(thick, su, 0.0), np.where(thick, sd, 0.0)
    albedo = np.empty((ng, nlay + 1, ncol))
    src = np.empty((ng, nlay + 1, ncol))
    den = np.empty((ng, nlay, ncol))
    albedo[:, nlay] = 1.0 - emis
    src[:, nlay] = pi * emis * bsfc
    for l in range(nlay - 1, -1, -1):
        den[:, l] = 1.0 / (1.0 - Rdif[:, l] * albedo[:, l + 1])
        albedo[:, l] = Rdif[:, l] + Tdif[:, l] * Tdif[:, l] * albedo[:, l + 1] * den[:, l]
        src[:, l] = su[:, l] + Tdif[:, l] * den[:, l] * (src[:, l + 1] + albedo[:, l + 1] * sd[:, l])
    up, dn = np.empty((ng, nlay + 1, ncol)), np.empty((ng, nlay + 1, ncol))
    dn[:, 0] = 0.0 if inc_flux is None else np.asarray(inc_flux, dtype=np.float64)
    up[:, 0] = dn[:, 0] * albedo[:, 0] + src[:, 0]
    for l in range(nlay):
        dn[:, l + 1] = (Tdif[:, l] * dn[:, l] + Rdif[:, l] * src[:, l + 1] + sd[:, l]) * den[:, l]
        up[:, l + 1] = dn[:, l + 1] * albedo[:, l + 1] + src[:, l + 1]
    if not top_at_1:
        up, dn = up[:, ::-1], dn[:, ::-1]
    return np.ascontiguousarray(up), np.ascontiguousarray(dn)


def broadband(spectral):
    """Sum of (ng, nlev, ncol) over the g-points, in g-point order."""
    out = np.zeros(spectral.shape[1:])
    for k in range(spectral.shape[0]):
        out = out + spectral[k]
    return out


def truth(tau, ssa, g, inc, dec, sfc_emis, sfc_source, inc_flux=None, top_at_1=True, dps=50):
    """Spectral fluxes (up, dn) of the boundary-value problem: object arrays (ng, nlay + 1, ncol) of mpf, memory order."""
    import mpmath as mp
    tau, ssa, g = (np.asarray(a, dtype=np.float64) for a in (tau, ssa, g))
    inc, dec = np.asarray(inc, dtype=np.float64), np.asarray(dec, dtype=np.float64)
    ng, nlay, ncol = tau.shape
    up, dn = np.empty((ng, nlay + 1, ncol), dtype=object), np.empty((ng, nlay + 1, ncol), dtype=object)
    order = range(nlay) if top_at_1 else range(nlay - 1, -1, -1)           # memory layer walked s-th from the top
    lorder = range(nlay + 1) if top_at_1 else range(nlay, -1, -1)           # memory level that is s-th from the top
    for kq in range(ng):
        for i in range(ncol):
            w64, g64, t64 = ssa[kq, :, i], g[kq, :, i], tau[kq, :, i]
            a1 = D * (1.0 - 0.5 * w64 * (1.0 + g64))
            a2 = D * 0.5 * w64 * (1.0 - g64)
            lost = float(np.sum(np.sqrt(np.maximum(a1 * a1 - a2 * a2, 0.0)) * t64)) / math.log(10.0)
            with mp.workdps(int(dps + lost) + 5):
                Dm = mp.mpf(166) / 100
                B = []                                                      # by memory level
                for j in range(nlay + 1):
                    if j == 0:
                        B.append(mp.mpf(float(dec[kq, 0, i])))
                    elif j == nlay:
                        B.append(mp.mpf(float(inc[kq, nlay - 1, i])))
                    else:
                        B.append(mp.sqrt(mp.mpf(float(dec[kq, j, i])) * mp.mpf(float(inc[kq, j - 1, i]))))
                B = [B[j] for j in lorder]                                  # from the top
                f0 = mp.mpf(0) if inc_flux is None else mp.mpf(float(inc_flux[kq][i]))
                part, homo = [mp.matrix([0, f0])], [mp.matrix([1, 0])]
                for s, l in enumerate(order):
                    t = mp.mpf(float(tau[kq, l, i]))
                    if t == 0:
                        part.append(part[-1].copy())
                        homo.append(homo[-1].copy())
                        continue
                    w, gg = mp.mpf(float(ssa[kq, l, i])), mp.mpf(float(g[kq, l, i]))
                    g1 = Dm * (1 - w * (1 + gg) / 2)
                    g2 = Dm * w * (1 - gg) / 2
                    E = mp.expm(mp.matrix([[g1, -g2], [g2, -g1]]) * t)
                    slope = mp.pi * (B[s + 1] - B[s]) / t / (g1 + g2)
                    p_top = mp.matrix([mp.pi * B[s] + slope, mp.pi * B[s] - slope])
                    p_bot = mp.matrix([mp.pi * B[s + 1] + slope, mp.pi * B[s + 1] - slope])
                    part.append(p_bot + E * (part[-1] - p_top))
                    homo.append(E * homo[-1])
                eps, bs = mp.mpf(float(sfc_emis[kq][i])), mp.mpf(float(sfc_source[kq][i]))
                p, h = part[-1], homo[-1]
                u = ((1 - eps) * p[1] + mp.pi * eps * bs - p[0]) / (h[0] - (1 - eps) * h[1])
                for s, j in enumerate(lorder):
                    v = part[s] + u * homo[s]
                    up[kq, j, i], dn[kq, j, i] = +v[0], +v[1]
    return up, dn


def to_f64(a):
    """Multi-digit values rounded once to float64."""
    return np.array([float(v) for v in np.asarray(a, dtype=object).ravel()], dtype=np.float64).reshape(np.shape(a))


def sum_gpts(a):
    """Sum of multi-digit spectral fluxes over the g-points, unrounded."""
    import mpmath as mp
    a = np.asarray(a, dtype=object)
    with mp.workdps(60):
        out = a[0].copy()
        for k in range(1, a.shape[0]):
            out = out + a[k]
    return out
