"""The single-precision two-stream longwave cell and column recurrences (ecckd_rte_lw_2stream_f32), restated in numpy
float32 with IEEE operations, in the order include/ecckd_hip.h spells ("Two-stream longwave, single precision").

It is the reference of the DEFINITION, not a bit-for-bit pin of the kernel: the kernel's reciprocal, exp and expm1 are the
device's fast forms.  The yardstick of both is tests/lw_2stream_ref.py (float64) -- test_lw_2stream_f32_host.py measures the
distance, cell by cell and on whole columns.

The float cell differs from the float64 one where float64's expressions cancel:

* gamma1 - gamma2 is formed as D*(1 - ssa), not as a difference of the two coefficients;
* 1 - e2 is formed as n1*(1 + e1) with n1 = -expm1(-k*tau): no digits are lost in a thin layer or under the k floor, so
  Rdif / Tdif need no series and the floor stays at 1e-12;
* the layer sources are written as pi*(Bt*A1 + dB*A2) and pi*(Bb*A1 - dB*A2) with the absorptance A1 = 1 - Rdif - Tdif and
  A2, both sums of positive terms: A1 = RT*(k*n1^2 + (gamma1-gamma2)*m), A2 = RT*(k*n1^2/(tau*(gamma1+gamma2)) + k*G),
  G = m/x - 2*e1 (x = k*tau).  G is the only difference that is left; below X_LIN it is the series
  e1*x^2/3*(1 + x^2/20*(1 + x^2/42)).  To first order in tau this is pi*(gamma1-gamma2)*tau*(Bt+Bb)/2, then -+ the dB terms.
* a layer emits where tau > 1e-30 (the quotients above need a normal number).

Arrays as in lw_2stream_ref: (ng, nlay, ncol), boundary values (ng, ncol), fluxes (ng, nlay + 1, ncol), memory order.
"""
import math

import numpy as np

F = np.float32
D = F(1.66)
PI = F(math.pi)
K_FLOOR = F(1e-12)
TAU_MIN = F(1e-30)
X_LIN = F(0.7)          # k*tau below which G is its series (the errors of the two forms cross here: DESIGN.md section 3)
ONE, TWO, HALF = F(1), F(2), F(0.5)
C3, C20, C42 = F(1.0 / 3.0), F(1.0 / 20.0), F(1.0 / 42.0)


def g_series(x, e1):
    x2 = x * x
    return e1 * (x2 * C3) * (ONE + (x2 * C20) * (ONE + x2 * C42))


def g_direct(x, e1, m):
    return m * (ONE / x) - TWO * e1


def cell(tau, ssa, g, Bt, Bb, x_lin=X_LIN, force=None):
    """(Rdif, Tdif, src_up, src_dn) of float32 arrays.  force: "series" / "direct" takes that form of G everywhere (the
    threshold study of the host test); None: the definition."""
    tau, ssa, g, Bt, Bb = (np.asarray(a, dtype=F) for a in (tau, ssa, g, Bt, Bb))
    with np.errstate(all="ignore"):
        gamma1 = D * (ONE - HALF * ssa * (ONE + g))
        gamma2 = D * HALF * ssa * (ONE - g)
        gm = D * (ONE - ssa)
        gp = gamma1 + gamma2
        kk0 = gm * gp
        k = np.sqrt(np.where(kk0 > K_FLOOR, kk0, K_FLOOR))
        x = tau * k
        e1 = np.exp(-x)
        n1 = -np.expm1(-x)
        m = n1 * (ONE + e1)
        RT = ONE / (k * (TWO - m) + gamma1 * m)
        Rdif = RT * gamma2 * m
        Tdif = RT * TWO * k * e1
        kn = k * n1 * n1
        A1 = RT * (kn + gm * m)
        gs, gd = g_series(x, e1), g_direct(x, e1, m)
        G = gs if force == "series" else gd if force == "direct" else np.where(x < x_lin, gs, gd)
        A2 = RT * (kn * (ONE / (tau * gp)) + k * G)
        dB = Bb - Bt
        su = PI * (Bt * A1 + dB * A2)
        sd = PI * (Bb * A1 - dB * A2)
        emits = tau > TAU_MIN
        su, sd = np.where(emits, su, F(0)), np.where(emits, sd, F(0))
    assert Rdif.dtype == F and su.dtype == F
    return Rdif, Tdif, su, sd


def level_sources(inc, dec):
    inc, dec = np.asarray(inc, dtype=F), np.asarray(dec, dtype=F)
    ng, nlay, ncol = inc.shape
    lev = np.empty((ng, nlay + 1, ncol), dtype=F)
    lev[:, 0] = dec[:, 0]
    lev[:, nlay] = inc[:, nlay - 1]
    with np.errstate(all="ignore"):
        lev[:, 1:nlay] = np.sqrt(dec[:, 1:] * inc[:, :-1])
    return lev


def restate(tau, ssa, g, inc, dec, sfc_emis, sfc_source, inc_flux=None, top_at_1=True):
    """Spectral fluxes (up, dn), float32 (ng, nlay + 1, ncol) in memory order; inputs are rounded to float32 first."""
    tau, ssa, g = (np.asarray(a, dtype=F) for a in (tau, ssa, g))
    emis, bsfc = np.asarray(sfc_emis, dtype=F), np.asarray(sfc_source, dtype=F)
    ng, nlay, ncol = tau.shape
    lev = level_sources(inc, dec)
    if not top_at_1:
        tau, ssa, g, lev = tau[:, ::-1], ssa[:, ::-1], g[:, ::-1], lev[:, ::-1]
    Rdif, Tdif, su, sd = cell(tau, ssa, g, lev[:, :-1], lev[:, 1:])
    albedo = np.empty((ng, nlay + 1, ncol), dtype=F)
    src = np.empty((ng, nlay + 1, ncol), dtype=F)
    den = np.empty((ng, nlay, ncol), dtype=F)
    with np.errstate(all="ignore"):
        albedo[:, nlay] = ONE - emis
        src[:, nlay] = PI * emis * bsfc
        for l in range(nlay - 1, -1, -1):
            den[:, l] = ONE / (ONE - Rdif[:, l] * albedo[:, l + 1])
            src[:, l] = su[:, l] + Tdif[:, l] * den[:, l] * (src[:, l + 1] + albedo[:, l + 1] * sd[:, l])
            albedo[:, l] = Rdif[:, l] + Tdif[:, l] * Tdif[:, l] * albedo[:, l + 1] * den[:, l]
        up, dn = np.empty((ng, nlay + 1, ncol), dtype=F), np.empty((ng, nlay + 1, ncol), dtype=F)
        dn[:, 0] = F(0) if inc_flux is None else np.asarray(inc_flux, dtype=F)
        up[:, 0] = dn[:, 0] * albedo[:, 0] + src[:, 0]
        for l in range(nlay):
            dn[:, l + 1] = (Tdif[:, l] * dn[:, l] + Rdif[:, l] * src[:, l + 1] + sd[:, l]) * den[:, l]
            up[:, l + 1] = dn[:, l + 1] * albedo[:, l + 1] + src[:, l + 1]
    if not top_at_1:
        up, dn = up[:, ::-1], dn[:, ::-1]
    return np.ascontiguousarray(up), np.ascontiguousarray(dn)


def broadband(spectral):
    """Sum over the g-points in float64 (the kernel's accumulators are double), rounded to float32 once."""
    return np.sum(np.asarray(spectral, dtype=np.float64), axis=0).astype(F)
