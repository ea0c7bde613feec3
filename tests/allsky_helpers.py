"""Numpy restatement of the element-wise operations on optical properties -- delta scaling and the four increments of
RTE-RRTMGP's optical-props kernels (delta_scale_2str_k / delta_scale_2str_f_k, increment_1scalar_by_1scalar,
increment_1scalar_by_2stream, increment_2stream_by_1scalar, increment_2stream_by_2stream and their inc_*_bybnd forms) --
written from the formulas, independent of the library, evaluated in the dtype of its inputs (float32, float64 or
np.longdouble).  Arrays follow the package convention: C order ``(n, nlay, ncol)``, n = g-points or bands.

Error bars of the GPU tests (relative, in units of the unit round-off u = eps/2 of the precision).  With tau >= 0,
0 <= ssa <= 1 and 0 <= g <= 0.9 every sum below has non-negative terms, so a relative error of its terms is not
amplified and every operation adds at most one rounding:

  1scl += 1scl   tau1 + tau2                                                      1 rounding
  1scl += 2str   1 - ssa2 | tau2 * (.) | tau1 + (.)                               3
  2str += 1scl   tau12 = tau1 + tau2 (1); ssa1 = tau1*ssa1 (1) / tau12 (+1) (1)   3 on ssa1, 1 on tau1
  2str += 2str   tau12 (1); tau1*ssa1 (1), tau2*ssa2 (1), their sum (1): tauscat12 carries 2 along a path;
                 ssa1 = tauscat12 (2) / tau12 (1), the division (1)               4
                 g1 = ((tau1*ssa1)*g1 (2) + (tau2*ssa2)*g2 (2), sum (1): 3) / tauscat12 (2), the division (1)   6

INCREMENT_ROUNDINGS = 6 is the largest count.  Each side of a comparison (the kernel, this restatement) sits at most
that many roundings from the exact value, so two sides differ by at most twice the count: INCREMENT_BAR_ULP = 12 u.
(1 - ssa2 in the second row subtracts two exact inputs: one rounding relative to its own result, however close ssa2
is to 1.)

Delta scaling (f = g*g or given, 0 <= f <= 0.81; wf = ssa*f <= 0.81):
  tau * (1 - wf)               f (1), wf (1), 1 - wf (1), product (1)                                  4
  (ssa - wf) / max(eps, 1-wf)  numerator: wf (2), difference (1); denominator 3; division (1)          7
  (g - f) / max(eps, 1 - f)    numerator: f (1), difference (1); denominator 2; division (1)           5
The differences 1 - wf, ssa - wf = ssa (1 - f), 1 - f divide the absolute error of the subtrahend by a result that is
at least 0.19 of the minuend: each inherited rounding is multiplied by at most 1/0.19 = 5.3.  g - g*g = g (1 - g) is the
exception: with g <= 0.9 the one rounding of f weighs g/(1 - g) <= 9 there; 9 + 1 + 5.3 * 2 + 1 = 21.6 u per side is
still inside DELTA_ROUNDINGS * 5.3 = 37 u.  DELTA_SCALE_BAR_ULP = 2 * 7 * 5.3 = 74.2 u.

tests/test_allsky_host.py confirms on synthetic.clouds that float64 against np.longdouble stays under half of each bar.
"""
import numpy as np

INCREMENT_ROUNDINGS = 6
DELTA_ROUNDINGS = 7
INCREMENT_BAR_ULP = 2 * INCREMENT_ROUNDINGS
DELTA_SCALE_BAR_ULP = 2 * DELTA_ROUNDINGS * 5.3


def unit_roundoff(dtype):
    return float(np.finfo(dtype).eps) / 2


def eps_floor(dtype):
    """3 * tiny(1._wp): the floor of the denominators."""
    return np.dtype(dtype).type(3) * np.finfo(dtype).tiny


def delta_scale(tau, ssa, g, forward=None):
    """(tau, ssa, g) delta-scaled with f = forward, or g*g.  Returns new arrays."""
    dt = tau.dtype.type
    f = g * g if forward is None else forward
    wf = ssa * f
    return (tau * (dt(1) - wf), (ssa - wf) / np.maximum(eps_floor(tau.dtype), dt(1) - wf),
            (g - f) / np.maximum(eps_floor(tau.dtype), dt(1) - f))


def spread(a, band2gpt, ngpt):
    """(nband, nlay, ncol) -> (ngpt, nlay, ncol): every band's plane repeated over its g-points (band2gpt 1-based,
    inclusive)."""
    out = np.empty((ngpt,) + a.shape[1:], dtype=a.dtype)
    for b, (lo, hi) in enumerate(np.asarray(band2gpt)):
        out[lo - 1:hi] = a[b]
    return out


def increment(op1, op2, band2gpt=None):
    """op1 += op2, each a tuple ``(tau,)`` (one-stream) or ``(tau, ssa, g)`` (two-stream); with band2gpt, op2 lives on
    bands.  Returns the new op1 as a tuple of new arrays."""
    ngpt = op1[0].shape[0]
    if band2gpt is not None:
        op2 = tuple(spread(a, band2gpt, ngpt) for a in op2)
    eps = eps_floor(op1[0].dtype)
    dt = op1[0].dtype.type
    if len(op1) == 1:
        if len(op2) == 1:
            return (op1[0] + op2[0],)
        return (op1[0] + op2[0] * (dt(1) - op2[1]),)
    tau1, ssa1, g1 = op1
    tau12 = tau1 + op2[0]
    if len(op2) == 1:
        return (tau12, tau1 * ssa1 / np.maximum(eps, tau12), g1.copy())
    tau2, ssa2, g2 = op2
    tauscat12 = tau1 * ssa1 + tau2 * ssa2
    return (tau12, tauscat12 / np.maximum(eps, tau12), (tau1 * ssa1 * g1 + tau2 * ssa2 * g2) / np.maximum(eps, tauscat12))


def worst_ulp(got, want):
    """Largest |got - want| / (u |want|) over the cells with want != 0, u of want's dtype; cells with want = 0 must hold
    got = 0 exactly (asserted)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    u = unit_roundoff(want.dtype if want.dtype != np.longdouble else got.dtype)
    d = np.abs(got.astype(np.longdouble) - want.astype(np.longdouble))
    w = np.abs(want.astype(np.longdouble))
    assert np.all(d[w == 0] == 0), "a cell whose expected value is 0 is not 0"
    return float(np.max(d[w > 0] / (u * w[w > 0]))) if np.any(w > 0) else 0.0


def band_tables():
    """band2gpt (nband, 2) of the three ecCKD files, by name."""
    import oracle
    from conftest import LW_FSCK, LW_RRTMGP, SW_WIDE
    return {n: (oracle.CkdModel(p).band2gpt.astype(np.int32), oracle.CkdModel(p).ng)
            for n, p in (("sw_wide", SW_WIDE), ("lw_fsck", LW_FSCK), ("lw_rrtmgp", LW_RRTMGP))}


# ------------------------------------------------------------------------------------------------
# all-sky oracle: the project's C oracle for gas optics and solvers, fed with numpy-incremented properties
# ------------------------------------------------------------------------------------------------
def oracle_sw_allsky(oracle_mod, m, cols, gas_items, cloud, delta=True, top_at_1=True, scale=None):
    """[up, dn, dir] of oracle.rte_sw on gas optics (oracle.gas_optics_ext) incremented in numpy by the band optics
    `cloud` (dict tau, ssa, g of (nband, nlay, ncol), or None: clear sky), delta-scaled first if `delta`."""
    otau, ossa, og, otoa, oerr = oracle_mod.gas_optics_ext(m, cols["plev"], cols["tlay"], gas_items)
    assert oerr == ""
    op = (otau, ossa, og)
    if cloud is not None:
        part = (cloud["tau"], cloud["ssa"], cloud["g"])
        if delta:
            part = delta_scale(*part)
        op = increment(op, part, m.band2gpt)
    if scale is not None:
        otoa = otoa * scale[None, :]
    g2b = m.gpt2band - 1
    return list(oracle_mod.rte_sw(op[0], op[1], op[2], cols["mu0"], otoa, np.ascontiguousarray(cols["alb_dir"][:, g2b].T),
                                  np.ascontiguousarray(cols["alb_dif"][:, g2b].T), top_at_1=top_at_1))


def oracle_lw_allsky(oracle_mod, m, cols, gas_items, cloud):
    """[up, dn] of oracle.rte_lw on gas optics (oracle.gas_optics_int) whose tau is incremented in numpy by the
    absorption optical depth of the band optics `cloud` (1scl += 2str by band), or clear sky (None)."""
    tau, lay, inc, dec, sfc, oerr = oracle_mod.gas_optics_int(m, cols["plev"], cols["tlay"], cols["tsfc"], gas_items, cols["tlev"])
    assert oerr == ""
    if cloud is not None:
        tau, = increment((tau,), (cloud["tau"], cloud["ssa"], cloud["g"]), m.band2gpt)
    emis = np.repeat(cols["sfc_emis"][None, :], m.ng, 0)
    return list(oracle_mod.rte_lw(tau, lay, inc, dec, emis, sfc))


def smallest_cloud_signal(allsky, clear, cloudy):
    """The smallest, over the cloudy columns, of the largest all-sky-minus-clear-sky flux change of the column (over
    levels and over the flux arrays): a flux bar must stay 20 times below it for a comparison to show the clouds."""
    change = np.max([np.abs(a - c).max(axis=0) for a, c in zip(allsky, clear)], axis=0)
    assert cloudy.any()
    return float(change[cloudy].min())
