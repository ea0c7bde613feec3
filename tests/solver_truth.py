"""Independent solutions of the equations the flux solvers solve, in multi-digit arithmetic (mpmath).

Nothing here is shared with the oracle (oracle/ecckd_oracle.c), the product or helpers.lw_emulate, and none of
their expressions appears: no two-stream reflectance / transmittance closed form, no adding recurrence, no
lw_source_noscat expression, no table of secants.

* sw_truth: the two-stream equations with the Zdunkowski / PIFM coefficients as a boundary-value problem through the
  whole column.  State y = [F_up, F_dn_diffuse, F_dir] (F_dir on a horizontal surface), tau increasing downwards,
  y' = M y inside a layer with

      M = [[ g1, -g2, -w g3 / mu0 ],        g1 = (8 - w (5 + 3 g)) / 4     g3 = (2 - 3 mu0 g) / 4
           [ g2, -g1,  w g4 / mu0 ],        g2 = 3 w (1 - g) / 4           g4 = 1 - g3
           [  0,   0,     -1 / mu0 ]]

  F_dir(top) = mu0 toa, F_dn_diffuse(top) = inc_dif, F_up(sfc) = alb_dif F_dn_diffuse(sfc) + alb_dir F_dir(sfc).
  Each layer is crossed with mpmath.expm(M tau); F_up(top) is found by linear shooting.  Shooting loses
  sum(k tau) / ln(10) digits (k^2 = g1^2 - g2^2: the homogeneous solutions grow like exp(k tau)), so the working
  precision is `dps` plus that many digits: the result is good to about `dps` digits whatever the optical depth.
* lw_truth: dI/dt = -I + B along the slant path of each quadrature angle, B linear in tau between the level values.
* gauss_jacobi: the Gauss rule for the weight mu on [0, 1] from its moments 1 / (j + 2).

Arrays follow the project's layout: tau (ng, nlay, ncol), fluxes (ng, nlay + 1, ncol), boundary values (ng, ncol).
Layer 0 is the top layer; a caller with the other orientation flips its arrays.
"""
import math

import mpmath as mp
import numpy as np


def _obj(shape):
    return np.empty(shape, dtype=object)


def to_f64(a):
    """Multi-digit values rounded once to float64."""
    return np.array([float(v) for v in np.asarray(a, dtype=object).ravel()], dtype=np.float64).reshape(np.shape(a))


def sum_gpts(a, first=0, last=None):
    """Sum of multi-digit spectral fluxes (ng, ...) over g-points first..last-1, unrounded."""
    a = np.asarray(a, dtype=object)
    out = a[first].copy()
    for k in range(first + 1, a.shape[0] if last is None else last):
        out = out + a[k]
    return out


# ------------------------------------------------------------------------------------------------
# shortwave
# ------------------------------------------------------------------------------------------------
def sw_digits_lost(tau, ssa, g):
    """sum(k tau) / ln 10 of one (column, g-point): the digits linear shooting loses."""
    w, gg, t = (np.asarray(a, dtype=np.float64) for a in (ssa, g, tau))
    g1 = (8.0 - w * (5.0 + 3.0 * gg)) / 4.0
    g2 = 3.0 * w * (1.0 - gg) / 4.0
    return float(np.sum(np.sqrt(np.maximum(g1 * g1 - g2 * g2, 0.0)) * t)) / math.log(10.0)


def _sw_column(tau, ssa, g, mu0, toa, dif_top, alb_dir, alb_dif, dps):
    """One (column, g-point).  Returns (up, dn_diffuse, dir) at the nlay + 1 levels and the single-layer direct-beam
    reflectance, diffuse transmittance of the direct beam and direct transmittance of every layer (each layer alone
    over a black surface: a by-product of the same propagators)."""
    nlay = len(tau)
    with mp.workdps(int(dps + sw_digits_lost(tau, ssa, g)) + 5):
        m0 = mp.mpf(float(mu0))
        part = [mp.matrix([0, mp.mpf(float(dif_top)), m0 * mp.mpf(float(toa))])]
        homo = [mp.matrix([1, 0, 0])]
        rdir, tdir, tnos = [], [], []
        for l in range(nlay):
            w, gg, t = mp.mpf(float(ssa[l])), mp.mpf(float(g[l])), mp.mpf(float(tau[l]))
            g1 = (8 - w * (5 + 3 * gg)) / 4
            g2 = 3 * w * (1 - gg) / 4
            g3 = (2 - 3 * m0 * gg) / 4
            g4 = 1 - g3
            M = mp.matrix([[g1, -g2, -w * g3 / m0], [g2, -g1, w * g4 / m0], [0, 0, -1 / m0]])
            E = mp.expm(M * t)
            part.append(E * part[-1])
            homo.append(E * homo[-1])
            r = -E[0, 2] / E[0, 0]                 # F_up(top) that leaves F_up(bottom) = 0 for a unit direct beam
            rdir.append(r)
            tdir.append(E[1, 0] * r + E[1, 2])
            tnos.append(E[2, 2])
        ad, af = mp.mpf(float(alb_dir)), mp.mpf(float(alb_dif))
        p, h = part[-1], homo[-1]
        u = (af * p[1] + ad * p[2] - p[0]) / (h[0] - af * h[1])
        lev = [part[s] + u * homo[s] for s in range(nlay + 1)]
        return ([+v[0] for v in lev], [+v[1] for v in lev], [+v[2] for v in lev]), (rdir, tdir, tnos)


def sw_truth(tau, ssa, g, mu0, toa, alb_dir, alb_dif, inc_dif=None, dps=60):
    """Spectral fluxes of the two-stream boundary-value problem: dict of object arrays (ng, nlay + 1, ncol) of mpf
    `up`, `dn` (diffuse + direct) and `dir`, and (ng, nlay, ncol) `rdir`, `tdir`, `tnoscat` of the single layers.
    toa, alb_dir, alb_dif, inc_dif are (ng, ncol); the direct flux at the top is the unrounded product mu0 * toa."""
    tau, ssa, g = (np.asarray(a, dtype=np.float64) for a in (tau, ssa, g))
    ng, nlay, ncol = tau.shape
    out = {n: _obj((ng, nlay + 1, ncol)) for n in ("up", "dn", "dir")}
    out.update({n: _obj((ng, nlay, ncol)) for n in ("rdir", "tdir", "tnoscat")})
    for k in range(ng):
        for i in range(ncol):
            dif = 0.0 if inc_dif is None else inc_dif[k][i]
            (up, dn, dr), lay = _sw_column(tau[k, :, i], ssa[k, :, i], g[k, :, i], mu0[i], toa[k][i], dif, alb_dir[k][i],
                                           alb_dif[k][i], dps)
            for s in range(nlay + 1):
                out["up"][k, s, i], out["dn"][k, s, i], out["dir"][k, s, i] = up[s], dn[s] + dr[s], dr[s]
            for l in range(nlay):
                out["rdir"][k, l, i], out["tdir"][k, l, i], out["tnoscat"][k, l, i] = lay[0][l], lay[1][l], lay[2][l]
    return out


# ------------------------------------------------------------------------------------------------
# longwave
# ------------------------------------------------------------------------------------------------
def _lw_layer(I, x, b_in, b_out):
    """Radiance leaving a layer of slant optical depth x entered with I, the source running linearly (in optical
    depth) from b_in to b_out:  I e^-x + int_0^x (b_in + (b_out - b_in) s / x) e^-(x - s) ds."""
    if x == 0:
        return I
    T = mp.exp(-x)
    return I * T + b_out - b_in * T - (b_out - b_in) * (1 - T) / x


def lw_truth(tau, lev_source, sfc_emis, sfc_source, Ds, weights, inc_flux=None, isotropic=False, dps=60):
    """Spectral fluxes of the no-scattering longwave problem: (up, dn), object arrays (ng, nlay + 1, ncol) of mpf.
    lev_source (ng, nlay + 1, ncol) is the Planck source at the levels; sfc_emis, sfc_source, inc_flux are (ng, ncol).
    Angle k has secant Ds[k] and weight weights[k]: I_dn(top) = inc_flux / (2 pi w_k) (isotropic: inc_flux / pi),
    I_up(sfc) = emis sfc_source + (1 - emis) I_dn(sfc), flux = 2 pi sum_k w_k I_k."""
    tau = np.asarray(tau, dtype=np.float64)
    ng, nlay, ncol = tau.shape
    up, dn = _obj((ng, nlay + 1, ncol)), _obj((ng, nlay + 1, ncol))
    with mp.workdps(dps):
        Ds = [mp.mpf(d) for d in Ds]
        wts = [mp.mpf(w) for w in weights]
        two_pi = 2 * mp.pi
        for k in range(ng):
            for i in range(ncol):
                B = [mp.mpf(float(lev_source[k][s][i])) for s in range(nlay + 1)]
                t = [mp.mpf(float(tau[k, l, i])) for l in range(nlay)]
                eps, bs = mp.mpf(float(sfc_emis[k][i])), mp.mpf(float(sfc_source[k][i]))
                fu, fd = [mp.mpf(0)] * (nlay + 1), [mp.mpf(0)] * (nlay + 1)
                for D, w in zip(Ds, wts):
                    if inc_flux is None:
                        I = mp.mpf(0)
                    else:
                        f = mp.mpf(float(inc_flux[k][i]))
                        I = f / mp.pi if isotropic else f / (two_pi * w)
                    fd[0] = fd[0] + two_pi * w * I
                    for l in range(nlay):
                        I = _lw_layer(I, t[l] * D, B[l], B[l + 1])
                        fd[l + 1] = fd[l + 1] + two_pi * w * I
                    I = eps * bs + (1 - eps) * I
                    fu[nlay] = fu[nlay] + two_pi * w * I
                    for l in range(nlay - 1, -1, -1):
                        I = _lw_layer(I, t[l] * D, B[l + 1], B[l])
                        fu[l] = fu[l] + two_pi * w * I
                for s in range(nlay + 1):
                    up[k, s, i], dn[k, s, i] = fu[s], fd[s]
    return up, dn


# ------------------------------------------------------------------------------------------------
# quadrature
# ------------------------------------------------------------------------------------------------
def gauss_jacobi(n, dps=60):
    """(secants, weights) of the n-point Gauss rule for int_0^1 f(mu) mu dmu, secants ascending (D_k = 1 / mu_k), as
    lists of mpf.  From the moments m_j = 1 / (j + 2): the monic polynomial of degree n orthogonal to 1 .. mu^(n-1),
    its roots, and the weights that integrate 1 .. mu^(n-1) exactly."""
    with mp.workdps(dps + 20):
        m = lambda j: mp.mpf(1) / (j + 2)
        A = mp.matrix(n, n)
        b = mp.matrix(n, 1)
        for j in range(n):
            for i in range(n):
                A[j, i] = m(i + j)
            b[j] = -m(n + j)
        c = mp.lu_solve(A, b)                                       # p(mu) = mu^n + sum_i c_i mu^i
        roots = mp.polyroots([mp.mpf(1)] + [c[i] for i in range(n - 1, -1, -1)], maxsteps=500, extraprec=4 * dps)
        x = sorted((mp.re(r) for r in roots), reverse=True)
        V = mp.matrix(n, n)
        rhs = mp.matrix(n, 1)
        for j in range(n):
            for k in range(n):
                V[j, k] = x[k] ** j
            rhs[j] = m(j)
        w = mp.lu_solve(V, rhs)
        return [1 / xk for xk in x], [w[k] for k in range(n)]
