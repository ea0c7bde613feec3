"""CPU tests of the single-precision two-stream longwave calls (include/ecckd_hip.h, "Two-stream longwave, single
precision"): the float cell and the float column recurrences as tests/lw_2stream_f32_ref.py restates them, against the
float64 restatement tests/lw_2stream_ref.py (never against the kernel); the refusals of ecckd_rte_lw_2stream_f32 and
ecckd_lw_fluxes_allsky_2stream_f32 on host-only models; the precision rules of the two new Python functions; the pinned
float64-only messages of the keyword routes.

Every bar below is TWICE a figure measured on the grid the test walks, with numpy 2.2 on x86-64 (the float32 restatement uses
IEEE operations and numpy's expf / expm1f, so the figures are properties of the definition, not of a GPU).  Measured:

  cell by cell (tau 1e-9 .. 1e2 on a log grid of 1057 points, ssa {0, 0.5, 0.999, 1}, g {0, 0.85}, Bb/Bt {1, 1.05, 0.8}),
  worst absolute error in units of pi*max(Bt, Bb) (Rdif / Tdif: absolute):
      Rdif %(RDIF).3e   Tdif %(TDIF).3e   src_up %(SU).3e   src_dn %(SD).3e
  The two source figures are NOT the float cell's error: they come from ssa = 1 at tau = 1.05e-8, the first grid point above
  RTE's tau > 1e-8 switch, where the float64 restatement sits on its k floor (k tau = 1e-14) and loses 1 - e2 to rounding --
  it emits 3.3e-3 pi B from a layer that conserves energy; the float cell gives 1e-21.  Without the rows ssa = 1 the figures
  are src_up %(SU_LT1).3e, src_dn %(SD_LT1).3e, which the test holds to a bar of its own, 8 float32 epsilons
  (9.54e-07): an output is a chain of about eight rounded float operations on quantities of order one.
  Across the threshold of G (k tau = 0.7) the error moves by at most %(JUMP).3e.

  columns (16 synthetic columns with synthetic.clouds on the 32-g longwave file, inputs rounded to float32), worst
  |float32 - float64| broadband flux: 60 layers %(COL60).3e W m-2, 137 layers %(COL137).3e W m-2.
"""
import ctypes as C
import inspect
import math

import numpy as np
import pytest

import __graft_entry__ as entry
import allsky_helpers as ah
import helpers
import lw_2stream_f32_ref as ref32
import lw_2stream_ref as ref64
from conftest import LW_FSCK, SW_WIDE
from rte_ecckd_amd import synthetic

MEASURED = dict(RDIF=2.530e-07, TDIF=2.210e-07, SU=1.054e-03, SD=1.054e-03, SU_LT1=2.682e-07, SD_LT1=2.821e-07, JUMP=6.484e-08,
                COL60=8.501e-05, COL137=1.187e-04)
__doc__ = __doc__ % MEASURED
EIGHT_EPS = 8 * float(np.finfo(np.float32).eps)
F4 = np.float32
TAUS = np.logspace(-9, 2, 12 * 11 * 8 + 1).astype(F4)
SSAS, GS, RATIOS = (0.0, 0.5, 0.999, 1.0), (0.0, 0.85), (1.0, 1.05, 0.8)
NLAY, NCOL = 5, 4


def cell64(tau, ssa, g, Bt, Bb):
    """(Rdif, Tdif, src_up, src_dn) of the float64 restatement, read off one-layer columns over a black, cold surface: with
    no incident flux flux_up(top) = src_up and flux_dn(bottom) = src_dn; a unit incident flux adds Rdif and Tdif."""
    n = np.size(tau)
    a = [np.asarray(v, dtype=np.float64).reshape(1, 1, n) for v in (tau, ssa, g)]
    inc, dec = (np.asarray(v, dtype=np.float64).reshape(1, 1, n) for v in (Bb, Bt))
    one, zero = np.ones((1, n)), np.zeros((1, n))
    u0, d0 = ref64.restate(*a, inc, dec, one, zero, zero)
    u1, d1 = ref64.restate(*a, inc, dec, one, zero, one)
    su, sd = u0[0, 0], d0[0, 1]
    return u1[0, 0] - su, d1[0, 1] - sd, su, sd


def cell_errors(tau, ssa, g, ratio, **kw):
    """float32 cell - float64 cell of the four outputs (signed), the sources in units of pi*max(Bt, Bb); inputs are float32 values."""
    n = tau.size
    s, gg = np.full(n, ssa, F4), np.full(n, g, F4)
    Bt, Bb = np.ones(n, F4), np.full(n, ratio, F4)
    got = ref32.cell(tau, s, gg, Bt, Bb, **kw)
    want = cell64(*(v.astype(np.float64) for v in (tau, s, gg, Bt, Bb)))
    unit = math.pi * max(1.0, float(F4(ratio)))
    return [(x.astype(np.float64) - w) / (1.0 if i < 2 else unit) for i, (x, w) in enumerate(zip(got, want))]


def test_float_cell_against_the_float64_restatement():
    names = ("RDIF", "TDIF", "SU", "SD")
    worst, below_one = np.zeros(4), np.zeros(4)
    for ssa in SSAS:
        for g in GS:
            for r in RATIOS:
                e = np.array([np.abs(x).max() for x in cell_errors(TAUS, ssa, g, r)])
                worst = np.maximum(worst, e)
                if ssa < 1.0:
                    below_one = np.maximum(below_one, e)
    for n, w, b in zip(names, worst, below_one):
        print("%s: worst %.3e (bar %.3e), without ssa = 1 %.3e (bar %.3e)" % (n, w, 2 * MEASURED[n], b, EIGHT_EPS))
        assert w <= 2 * MEASURED[n]
        assert b <= EIGHT_EPS
    # the rows ssa = 1: the float cell emits next to nothing (a conservative layer), whatever the float64 restatement says
    t = TAUS
    _, _, su, sd = ref32.cell(t, np.ones(t.size, F4), np.full(t.size, 0.85, F4), np.ones(t.size, F4), np.full(t.size, 0.8, F4))
    print("ssa = 1: largest |src| of the float cell %.3e pi B" % (max(np.abs(su).max(), np.abs(sd).max()) / math.pi))
    assert max(np.abs(su).max(), np.abs(sd).max()) <= 1e-6 * math.pi


def test_error_is_continuous_across_the_threshold():
    """Both sides of k tau = X_LIN: the last float32 tau whose cell takes the series and the first that takes the closed form."""
    worst = 0.0
    seen = 0
    for ssa in SSAS:
        for g in GS:
            gm, gp = ref32.D * (F4(1) - F4(ssa)), None
            gamma1 = ref32.D * (F4(1) - F4(0.5) * F4(ssa) * (F4(1) + F4(g)))
            gamma2 = ref32.D * F4(0.5) * F4(ssa) * (F4(1) - F4(g))
            gp = gamma1 + gamma2
            k = np.sqrt(max(gm * gp, ref32.K_FLOOR))
            tau = F4(ref32.X_LIN / k)
            if not tau < 100.0:
                continue   # (k on its floor: k tau never reaches the threshold on this grid)
            while tau * k >= ref32.X_LIN:
                tau = np.nextafter(tau, F4(0))
            while np.nextafter(tau, F4(np.inf)) * k < ref32.X_LIN:
                tau = np.nextafter(tau, F4(np.inf))
            pair = np.array([tau, np.nextafter(tau, F4(np.inf))], dtype=F4)
            assert pair[0] * k < ref32.X_LIN <= pair[1] * k
            seen += 1
            for r in RATIOS:
                e = cell_errors(pair, ssa, g, r)
                for i, n in enumerate(("RDIF", "TDIF", "SU", "SD")):
                    jump = abs(float(e[i][1] - e[i][0]))
                    worst = max(worst, jump)
                    assert jump <= 2 * MEASURED[n] and jump <= EIGHT_EPS, (ssa, g, r, n, jump)
    print("threshold pairs %d, largest jump of the error across the threshold %.3e" % (seen, worst))
    assert seen == 6


def test_conservative_thin_layer_against_the_truth():
    """Where the float cell and the float64 restatement part company -- ssa = 1 (k on its floor), tau just above RTE's 1e-8
    cutoff -- the 50-digit solution of the two-stream equations (lw_2stream_ref.truth: no closed form, no floor, no cutoff)
    sides with the float cell: one layer over a grey surface, the case test_gpu_lw_2stream_f32.py meets in its random columns."""
    tau, ssa, g = (np.full((1, 1, 1), v) for v in (float(F4(2.1364805e-08)), 1.0, float(F4(0.85))))
    inc, dec = np.full((1, 1, 1), 4.5), np.full((1, 1, 1), 3.5)
    emis, bsfc, top = np.full((1, 1), 0.9), np.full((1, 1), 5.0), np.full((1, 1), 12.0)
    tu, td = (ref64.to_f64(x) for x in ref64.truth(tau, ssa, g, inc, dec, emis, bsfc, top))
    u64, d64 = ref64.restate(tau, ssa, g, inc, dec, emis, bsfc, top)
    u32, d32 = ref32.restate(tau, ssa, g, inc, dec, emis, bsfc, top)
    e64 = max(np.abs(u64 - tu).max(), np.abs(d64 - td).max())
    e32 = max(np.abs(u32 - tu).max(), np.abs(d32 - td).max())
    ulp = float(np.spacing(F4(np.abs(tu).max())))
    print("conservative thin layer: float64 restatement %.3e W m-2 from the truth, float32 restatement %.3e (one float32 ulp of the flux: %.1e)"
          % (e64, e32, ulp))
    assert e32 <= 4 * ulp      # a handful of rounded operations on the boundary values: the layer itself does next to nothing
    assert e64 > 1e3 * e32     # (the figure that sets the bars against the fp64 calls is the fp64 expressions' own)


@pytest.fixture(scope="module")
def columns(pkg, oracle_mod):
    """Per layer count: float32-rounded solver inputs of 16 cloudy synthetic columns on the 32-g file, and the float64 fluxes."""
    m = oracle_mod.CkdModel(LW_FSCK)
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=-1) == ""
    out = {}
    for nlay in (60, 137):
        ncol, c0 = 16, 11
        cols = synthetic.columns(c0, ncol, k.get_press_min(), nlay=nlay)
        cloud = synthetic.clouds(c0, ncol, nlay, k.get_nband())
        assert cloud["cloudy"].any()
        tau, _, inc, dec, sfc, err = oracle_mod.gas_optics_int(m, cols["plev"], cols["tlay"], cols["tsfc"], helpers.oracle_gas_items(cols),
                                                               cols["tlev"])
        assert err == ""
        r = lambda a: np.asarray(a, dtype=F4)
        zero = np.zeros_like(r(tau))
        op = ah.increment((r(tau), zero, zero), (r(cloud["tau"]), r(cloud["ssa"]), r(cloud["g"])), m.band2gpt)
        assert all(a.dtype == F4 for a in op)
        emis = r(np.repeat(cols["sfc_emis"][None, :], m.ng, 0))
        a = dict(tau=op[0], ssa=op[1], g=op[2], inc=r(inc), dec=r(dec), emis=emis, sfc=r(sfc),
                 inc_flux=r(np.random.default_rng(nlay).uniform(0.0, 2.0, (m.ng, ncol))))
        d = {k: v.astype(np.float64) for k, v in a.items()}
        up, dn = ref64.restate(d["tau"], d["ssa"], d["g"], d["inc"], d["dec"], d["emis"], d["sfc"], d["inc_flux"])
        out[nlay] = (a, ref64.broadband(up), ref64.broadband(dn))
    return out


@pytest.mark.parametrize("nlay", [60, 137])
def test_float_columns_against_float64(columns, nlay):
    a, up64, dn64 = columns[nlay]
    worst = 0.0
    for top in (True, False):
        b = a if top else dict(ref64.flip_orientation(a), emis=a["emis"], sfc=a["sfc"], inc_flux=a["inc_flux"])
        up, dn = ref32.restate(b["tau"], b["ssa"], b["g"], b["inc"], b["dec"], b["emis"], b["sfc"], b["inc_flux"], top)
        assert up.dtype == F4
        bu, bd = ref32.broadband(up).astype(np.float64), ref32.broadband(dn).astype(np.float64)
        if not top:
            bu, bd = bu[::-1], bd[::-1]
        worst = max(worst, float(np.max(np.abs(bu - up64))), float(np.max(np.abs(bd - dn64))))
    key = "COL%d" % nlay
    print("%d layers: float32 restatement %.3e W m-2 from float64 (bar %.3e), flux_up(top) %.1f ... %.1f W m-2"
          % (nlay, worst, 2 * MEASURED[key], up64[0].min(), up64[0].max()))
    assert worst <= 2 * MEASURED[key]


# ---------------------------------------------------------------------------------------------------------------------
# refusals (host-only models: nothing computes, no device is asked for before the refusal)
# ---------------------------------------------------------------------------------------------------------------------
def P(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def test_symbols_and_bindings(pkg):
    L = pkg.lib()
    for s in ("ecckd_rte_lw_2stream_f32", "ecckd_lw_fluxes_allsky_2stream_f32", "ecckd_lw_fluxes_allsky_2stream_f32_scratch_bytes"):
        assert s in entry.exported_symbols() and hasattr(L, s) and getattr(L, s).argtypes is not None, s
    assert len(L.ecckd_rte_lw_2stream_f32.argtypes) == 20 and len(L.ecckd_lw_fluxes_allsky_2stream_f32.argtypes) == 25
    assert list(inspect.signature(pkg.rte_lw_2stream).parameters) == ["optical_props", "top_at_1", "sources", "sfc_emis", "fluxes",
                                                                     "inc_flux", "device"]
    assert list(inspect.signature(pkg.GasOpticsEcckd.lw_fluxes_allsky_2stream).parameters)[1:] == [
        "plev", "tlay", "tsfc", "tlev", "gas_desc", "top_at_1", "sfc_emis", "particles", "fluxes", "inc_flux", "cloud_mask"]
    # the work block: 4 cell arrays, the surface source and the float ring (half the fp64 solver's), each rounded to 256 bytes
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=-1) == ""
    r256 = lambda n: (n + 255) // 256 * 256
    for ncol, nlay in ((1, 1), (37, 60), (100000, 137)):
        ng = k.get_ngpt()
        want = 4 * r256(ncol * nlay * ng * 4) + r256(ncol * ng * 4) + r256(pkg.rte_lw_2stream_scratch_bytes(ncol, nlay, ng) // 2)
        assert k.lw_fluxes_allsky_2stream_f32_scratch_bytes(ncol, nlay) == want


def _solver_inputs(pkg, k, dtype):
    op = pkg.OpticalProps2str()
    op.alloc_2str(NCOL, NLAY, k, like=np.empty(0, dtype))
    src = pkg.SourceFuncLW()
    src.alloc(NCOL, NLAY, k, like=np.empty(0, dtype), separate_levels=True)
    for a in (op.tau, op.ssa, op.g, src.lay_source, src.lev_source_inc, src.lev_source_dec, src.sfc_source):
        a[:] = 0.5
    return op, src


def test_solver_refusals_before_any_device(pkg):
    """ecckd_rte_lw_2stream_f32 in the order of the fp64 call, under its own name, every later refusal armed (memspace 7)."""
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=-1) == ""
    ng, nb = k.get_ngpt(), k.get_nband()
    op, src = _solver_inputs(pkg, k, F4)
    emis = np.full((NCOL, nb), 0.98, F4)
    up, dn = outs = [np.full((NLAY + 1, NCOL), -7.0, F4) for _ in range(2)]
    L = pkg.lib()
    b2g = np.ascontiguousarray(op.band2gpt, dtype=np.int32)
    args = dict(tau=op.tau, ssa=op.ssa, g=op.g, lay=src.lay_source, inc=src.lev_source_inc, dec=src.lev_source_dec,
                sfc=src.sfc_source, emis=emis, incf=None, up=up, dn=dn)

    def raw(ncol=NCOL, nlay=NLAY, ngpt=ng, nband=nb, b2=b2g, memspace=pkg.HOST, dev=0, **kw):
        a = dict(args, **kw)
        return L.ecckd_rte_lw_2stream_f32(dev, ncol, nlay, ngpt, 1, P(a["tau"]), P(a["ssa"]), P(a["g"]), P(a["lay"]), P(a["inc"]),
                                          P(a["dec"]), P(a["sfc"]), nband, P(b2), P(a["emis"]), P(a["incf"]), P(a["up"]), P(a["dn"]),
                                          memspace, None)
    assert raw(ncol=-1, tau=None, memspace=7) == 1 and "bad ncol/nlay" in pkg.last_error()
    for name in ("tau", "ssa", "g", "inc", "dec", "sfc", "emis", "up", "dn"):
        assert raw(ngpt=300, memspace=7, **{name: None}) == 1 and "ecckd_rte_lw_2stream_f32: null argument" in pkg.last_error(), name
    assert raw(ngpt=300, memspace=7) == 1 and "ngpt must be in 1..256" in pkg.last_error()
    assert raw(nlay=700, memspace=7) == 1 and "too many layers" in pkg.last_error()
    pkg.set_arithmetic(pkg.REFERENCE_ORDER)
    try:
        assert raw(memspace=2) == 1 and "ecckd_rte_lw_2stream_f32: ECCKD_MIXED is not implemented" in pkg.last_error()
        assert raw(memspace=7) == 1 and pkg.last_error() == "ecckd: bad memspace"
        assert raw(dev=99) == 1 and "ecckd_rte_lw_2stream_f32: needs the fast arithmetic mode" in pkg.last_error()
    finally:
        pkg.set_arithmetic(pkg.FAST)
    assert raw(lay=None, dev=99) == 1 and ("bad device ordinal" in pkg.last_error() or "no HIP device" in pkg.last_error())
    assert all(np.all(a == -7.0) for a in outs)


def _wide_model(pkg, ng=65):
    lp = np.log([10., 100., 1000.])
    T = 200. + np.arange(6).reshape(2, 3)
    k = pkg.GasOpticsEcckd()
    err = k.init_from_tables(lp, T, [dict(name="x", code=1, coefficient=np.ones((2, 3, ng)))],
                             planck=(np.array([100., 200.]), np.ones((2, ng))), device=-1)
    assert err == "", err
    return k


def test_fused_refusals_in_order(pkg):
    """ecckd_lw_fluxes_allsky_2stream_f32 on host-only models, in the header's order, each under the call's name: a mask with more
    than 64 g-points; nband_p; tau_p, ssa_p or g_p NULL; reference-order arithmetic; no Planck table; tlev NULL; ECCKD_MIXED;
    the host-only model."""
    L = pkg.lib()
    who = "ecckd_lw_fluxes_allsky_2stream_f32"
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=-1) == ""
    ksw = pkg.GasOpticsEcckd()
    assert ksw.load(SW_WIDE, device=-1) == ""
    nb = k.get_nband()
    f = lambda shape, v: np.full(shape, v, F4)
    plev, tlay, tsfc, tlev = f((NLAY + 1, NCOL), 1e4), f((NLAY, NCOL), 250.), f(NCOL, 250.), f((NLAY + 1, NCOL), 250.)
    emis = f((NCOL, nb), 0.98)
    up, dn = outs = [f((NLAY + 1, NCOL), -7.0) for _ in range(2)]
    part = [f((nb, NLAY, NCOL), 0.5) for _ in range(3)]
    mask = np.full((NLAY, NCOL), 5, dtype=np.uint64)
    names = b"h2o".ljust(32, b" ")
    vmr = (C.c_void_p * 1)(None)
    z, sc = (C.c_longlong * 1)(0), (C.c_double * 1)(1e-3)

    def raw(model=k, nband_p=nb, tp=part[0], sp=part[1], gp=part[2], m_=None, tlev_=tlev, memspace=pkg.HOST):
        return L.ecckd_lw_fluxes_allsky_2stream_f32(None if model is None else model._need(), NCOL, NLAY, P(plev), P(tlay), P(tsfc),
                                                    P(tlev_), 1, names, vmr, z, z, sc, 1, P(emis), None, nband_p, P(tp), P(sp), P(gp),
                                                    P(m_), P(up), P(dn), memspace, None)
    assert raw(model=None) == 1 and "null model" in pkg.last_error()
    pkg.set_arithmetic(pkg.REFERENCE_ORDER)
    try:
        wide = _wide_model(pkg)
        assert wide.get_ngpt() == 65 and wide.get_nband() != nb + 7
        assert raw(model=wide, nband_p=nb + 7, tp=None, m_=mask, tlev_=None, memspace=2) == 1
        assert who + ":" in pkg.last_error() and "at most 64 g-points, not 65" in pkg.last_error()
        assert raw(model=wide, nband_p=nb + 7, tp=None, tlev_=None, memspace=2) == 1
        assert who + ": nband_p = %d" % (nb + 7) in pkg.last_error()
        assert raw(nband_p=nb + 1, tp=None, tlev_=None, memspace=2) == 1 and who + ": nband_p = %d" % (nb + 1) in pkg.last_error()
        for kw in (dict(tp=None), dict(sp=None), dict(gp=None)):
            assert raw(tlev_=None, memspace=2, **kw) == 1
            assert who + ": null argument (tau_p, ssa_p and g_p are required" in pkg.last_error(), kw
        assert raw(tlev_=None, memspace=2) == 1 and who + ": needs the fast arithmetic mode" in pkg.last_error()
    finally:
        pkg.set_arithmetic(pkg.FAST)
    nbs = ksw.get_nband()
    psw = f((nbs, NLAY, NCOL), 0.5)
    assert raw(model=ksw, nband_p=nbs, tp=psw, sp=psw, gp=psw, tlev_=None, memspace=2) == 1 and who + ": model has no Planck table" in pkg.last_error()
    assert raw(tlev_=None, memspace=2) == 1 and pkg.last_error() == "tlev is required for ecckd"
    assert raw(memspace=2) == 1 and who + ": ECCKD_MIXED is not implemented" in pkg.last_error()
    for m_ in (None, mask):
        assert raw(m_=m_, memspace=7) == 1 and "no CPU fallback" in pkg.last_error()
    assert all(np.all(a == -7.0) for a in outs) and all(np.all(a == 0.5) for a in part) and np.all(mask == 5)


def test_python_precisions_and_pinned_keyword_messages(pkg):
    """rte_lw_2stream and lw_fluxes_allsky_2stream: float64 or float32 arrays, a mixture is refused with a message that names
    two arrays; both precisions reach the library (a host-only model answers for it).  The keyword routes keep their
    float64-only messages."""
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=-1) == ""
    ng, nb = k.get_ngpt(), k.get_nband()
    for dtype, other in ((np.float64, F4), (F4, np.float64)):
        op, src = _solver_inputs(pkg, k, dtype)
        emis = np.full((NCOL, nb), 0.98, dtype)
        fl = pkg.FluxesBroadband(np.full((NLAY + 1, NCOL), -7.0, dtype), np.full((NLAY + 1, NCOL), -7.0, dtype))
        m = pkg.rte_lw_2stream(op, True, src, emis, fl, device=99)
        assert "bad device ordinal" in m or "no HIP device" in m, m
        m = pkg.rte_lw_2stream(op, True, src, emis, fl, inc_flux=np.zeros((ng, NCOL), other))
        assert m.startswith("rte_lw_2stream: mixing float32 and float64 arrays in one call") and "inc_flux" in m, m
        m = pkg.rte_lw_2stream(op, True, src, emis.astype(other), fl)
        assert "mixing float32 and float64" in m and "sfc_emis" in m
        assert "shape" in pkg.rte_lw_2stream(op, True, src, emis, fl, inc_flux=np.zeros((ng + 1, NCOL), dtype))
        one = pkg.OpticalProps1scl(); one.alloc_1scl(NCOL, NLAY, k, like=np.empty(0, dtype))
        assert "two-stream optical properties required" in pkg.rte_lw_2stream(one, True, src, emis, fl)
        bnd = [np.zeros((nb, NLAY + 1, NCOL), dtype) for _ in range(2)]
        assert "per-band fluxes" in pkg.rte_lw_2stream(op, True, src, emis, pkg.FluxesByband(bnd[0], bnd[1]))
        assert np.all(fl.flux_up == -7.0) and np.all(fl.flux_dn == -7.0)

        gc = pkg.GasConcs(["h2o"]); gc.set_vmr("h2o", 1e-3)
        f = lambda shape, v: np.full(shape, v, dtype)
        plev, tlay, tsfc, tlev = f((NLAY + 1, NCOL), 1e4), f((NLAY, NCOL), 250.), f(NCOL, 250.), f((NLAY + 1, NCOL), 250.)
        good = pkg.OpticalProps2str()
        assert good.alloc_2str_bands(NCOL, NLAY, k, like=np.empty(0, dtype)) == ""
        call = lambda p=good, e=emis, **kw: k.lw_fluxes_allsky_2stream(plev, tlay, tsfc, tlev, gc, True, e, p, fl, **kw)
        assert "no CPU fallback" in call()
        assert "no CPU fallback" in call(cloud_mask=np.full((NLAY, NCOL), 5, dtype=np.uint64))
        m = call(e=emis.astype(other))
        assert m.startswith("lw_fluxes_allsky_2stream: mixing float32 and float64 arrays in one call") and "sfc_emis" in m, m
        bad = pkg.OpticalProps2str(); bad.tau, bad.ssa, bad.g = good.tau, good.ssa, np.zeros(good.g.shape, other)
        assert "mixing float32 and float64" in call(bad) and "particles.g" in call(bad)
        nog = pkg.OpticalProps2str(); nog.tau, nog.ssa, nog.g = good.tau, good.ssa, None
        assert "with g" in call(nog)
        assert "uint64" in call(cloud_mask=np.zeros((NLAY, NCOL), dtype=np.int64))
        assert np.all(fl.flux_up == -7.0)

    # the keyword routes: float32 is still refused, with the messages tests/golden/fused_call_marshalling.json pins
    op32, src32 = _solver_inputs(pkg, k, F4)
    emis32 = np.full((NCOL, nb), 0.98, F4)
    fl32 = pkg.FluxesBroadband(np.zeros((NLAY + 1, NCOL), F4), np.zeros((NLAY + 1, NCOL), F4))
    assert pkg.rte_lw(op32, True, src32, emis32, fl32, use_2stream=True) == "rte_lw(use_2stream=True): implemented for float64 arrays"
    p32 = pkg.OpticalProps2str()
    assert p32.alloc_2str_bands(NCOL, NLAY, k, like=np.empty(0, F4)) == ""
    f = lambda shape, v: np.full(shape, v, F4)
    m = k.lw_fluxes_allsky(f((NLAY + 1, NCOL), 1e4), f((NLAY, NCOL), 250.), f(NCOL, 250.), f((NLAY + 1, NCOL), 250.),
                           pkg.GasConcs(["h2o"]), True, emis32, p32, fl32, use_2stream=True)
    assert m == "lw_fluxes_allsky: use_2stream=True is implemented for float64 arrays"


def test_marshalling_of_the_fused_call_argument_by_argument(pkg):
    """What lw_fluxes_allsky_2stream hands the library, recorded with the recorder of tests/golden/make_golden_fused_calls.py:
    on float64 arrays the arguments of lw_fluxes_allsky(use_2stream=True), which the golden recording pins; on float32 arrays
    the same arguments at the single-precision entry point (the binding forms its name as the fp64 name + "_f32", as lib() does
    for the prototypes, so the golden test's scan of the binding's literal names does not see it: this test stands in)."""
    import os
    import sys
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if golden not in sys.path:
        sys.path.insert(0, golden)
    import make_golden_fused_calls as gen
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=-1) == ""
    real = pkg.lib()

    def record(dtype, new, masked):
        a = gen.arrays(k, np.dtype(dtype), False)
        gc = pkg.GasConcs(["h2o", "co2"]); gc.set_vmr("h2o", a["vmr"]); gc.set_vmr("co2", 4e-4)
        part = pkg.OpticalProps2str()
        part.tau, part.ssa, part.g = a["particles.tau"], a["particles.ssa"], a["particles.g"]
        fl = pkg.FluxesBroadband(a["flux_up"], a["flux_dn"])
        head = (a["plev"], a["tlay"], a["tsfc"], a["tlev"], gc, True, a["sfc_emis"], part, fl)
        kw = dict(inc_flux=a["inc_flux"], cloud_mask=a["cloud_mask"] if masked else None)
        pkg._lib = rec = gen.Recorder(real)
        try:
            msg = k.lw_fluxes_allsky_2stream(*head, **kw) if new else k.lw_fluxes_allsky(*head, use_2stream=True, **kw)
        finally:
            pkg._lib = real
        assert msg == "" and len(rec.calls) == 1, (msg, rec.calls)
        return rec.calls[0][0], [gen.normalise(x, a, k) for x in rec.calls[0][1]]

    for masked in (False, True):
        name64, args64 = record(np.float64, True, masked)
        assert (name64, args64) == record(np.float64, False, masked) and name64 == "ecckd_lw_fluxes_allsky_2stream"
        name32, args32 = record(F4, True, masked)
        assert name32 == "ecckd_lw_fluxes_allsky_2stream_f32" and args32 == args64
        assert len(args64) == 25 and args64[0] == "handle" and args64[1:3] == [gen.NCOL, gen.NLAY]
        assert args64[3:7] == ["plev", "tlay", "tsfc", "tlev"] and args64[13:16] == [1, "sfc_emis", "inc_flux"]
        assert args64[16:23] == [k.get_nband(), "particles.tau", "particles.ssa", "particles.g", "cloud_mask" if masked else None,
                                 "flux_up", "flux_dn"]
        assert args64[23] == pkg.HOST and args64[24] is None
