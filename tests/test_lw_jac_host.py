"""CPU tests of the longwave surface-temperature Jacobian (include/ecckd_hip.h, "Longwave surface-temperature Jacobian"):
the three symbols and their bindings, the refusals in their documented order on a host-only model (nothing computes on the
CPU), the Python mirror's shape and dtype errors, the code objects of the new kernels next to their neighbours, and the
yardstick of the GPU tests itself: the oracle's rte_lw with zero layer and level sources and sfc_source = sfc_source_jac
is the difference of its upward fluxes at tsfc + 1 and at tsfc."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as entry
import helpers
from conftest import LW_FSCK, LW_RRTMGP, SW_WIDE
from helpers import FLUX_ATOL
from rte_ecckd_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NLAY, NCOL = 60, 4
SYMBOLS = ("ecckd_planck_sfc_source_jac", "ecckd_rte_lw_jac", "ecckd_lw_fluxes_jac")


def test_symbols_are_declared_exported_and_bound(pkg):
    L = pkg.lib()
    for s in SYMBOLS:
        assert s in entry.exported_symbols(), s
        assert hasattr(L, s) and getattr(L, s).argtypes is not None, s
    assert len(L.ecckd_planck_sfc_source_jac.argtypes) == 6
    # ecckd_rte_lw_inc_flux plus sfc_source_jac and flux_up_jac; ecckd_lw_fluxes_clear_allsky plus flux_up_jac
    assert len(L.ecckd_rte_lw_jac.argtypes) == 21
    assert len(L.ecckd_lw_fluxes_jac.argtypes) == len(L.ecckd_lw_fluxes_clear_allsky.argtypes) + 1 == 28
    for f in (pkg.rte_lw, pkg.GasOpticsEcckd.lw_fluxes, pkg.GasOpticsEcckd.lw_fluxes_allsky):
        p = inspect.signature(f).parameters
        assert list(p)[-1] == "flux_up_jac" and p["flux_up_jac"].default is None, f
    # both skies: a method of its own (tests/test_both_skies_host.py pins the argument list of lw_fluxes_clear_allsky)
    p = inspect.signature(pkg.GasOpticsEcckd.lw_fluxes_clear_allsky_jac).parameters
    assert list(p)[-6:] == ["fluxes", "fluxes_clear", "flux_up_jac", "n_gauss_angles", "inc_flux", "cloud_mask"]
    assert list(inspect.signature(pkg.GasOpticsEcckd.planck_sfc_source_jac).parameters) == ["self", "tsfc", "sources"]
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=-1) == ""
    src = pkg.SourceFuncLW()
    assert src.sfc_source_jac is None and src.alloc(NCOL, NLAY, k) == ""
    assert src.sfc_source_jac.shape == (k.get_ngpt(), NCOL) and src.sfc_source_jac.dtype == np.float64


def test_lw_jac_inline_option(pkg):
    assert pkg.get_solver_option("lw_jac_inline") in (0.0, 1.0)
    before = pkg.get_solver_option("lw_jac_inline")
    try:
        for v in (1, 0):
            pkg.set_solver_option("lw_jac_inline", v)
            assert pkg.get_solver_option("lw_jac_inline") == v
        with pytest.raises(Exception) as e:
            pkg.set_solver_option("lw_jac_inline", 2)
        assert "lw_jac_inline must be 0" in str(e.value)
    finally:
        pkg.set_solver_option("lw_jac_inline", before)


def _columns():
    return (np.full((NLAY + 1, NCOL), 1e4), np.full((NLAY, NCOL), 250.), np.full(NCOL, 250.), np.full((NLAY + 1, NCOL), 250.))


def _fluxes(n, value=-7.0):
    return [np.full((NLAY + 1, NCOL), value) for _ in range(n)]


def test_fused_refusals_in_order(pkg):
    """ecckd_lw_fluxes_jac on a host-only model: the existing call's list in its order (here: the all-sky list -- band
    count, tau_p, arithmetic mode, tlev -- and a NULL clear-sky output), then flux_up_jac equal to another output, then, with
    valid arguments, the host-only model fails loudly.  The list of ecckd_lw_fluxes begins with the host-only refusal, so the
    clear-sky form answers that whatever else is wrong (tests/test_gpu_lw_jac.py asks a device model for the rest of its
    order).  Outputs stay untouched throughout."""
    plev, tlay, tsfc, tlev = _columns()
    gc = pkg.GasConcs(["h2o"]); gc.set_vmr("h2o", 1e-3)
    up, dn, upc, dnc, jac = outs = _fluxes(5)
    fl, fc = pkg.FluxesBroadband(up, dn), pkg.FluxesBroadband(upc, dnc)
    untouched = lambda: all(np.all(a == -7.0) for a in outs)
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=-1) == ""
    nb = k.get_nband()
    emis = np.full((NCOL, nb), 0.98)
    wrong = pkg.OpticalProps1scl(); wrong.tau = np.full((nb + 1, NLAY, NCOL), 0.5)
    good = pkg.OpticalProps2str()
    assert good.alloc_2str_bands(NCOL, NLAY, k) == ""
    for a in (good.tau, good.ssa, good.g):
        a[:] = 0.5
    mask = np.full((NLAY, NCOL), 5, dtype=np.uint64)
    allsky = lambda p, tlev_, j, m_=None: k.lw_fluxes_allsky(plev, tlay, tsfc, tlev_, gc, True, emis, p, fl, cloud_mask=m_, flux_up_jac=j)
    both = lambda tlev_, fc_, j: k.lw_fluxes_clear_allsky_jac(plev, tlay, tsfc, tlev_, gc, True, emis, good, fl, fc_, j)
    clear = lambda tlev_, j: k.lw_fluxes(plev, tlay, tsfc, tlev_, gc, True, emis, fl, flux_up_jac=j)
    pkg.set_arithmetic(pkg.REFERENCE_ORDER)
    try:   # every later refusal is armed too (flux_up_jac is flux_up): the earlier one is the one named
        assert "nband_p = %d" % (nb + 1) in allsky(wrong, None, up) and untouched()
        assert "fast arithmetic mode" in allsky(good, None, up) and untouched()
        assert "no CPU fallback" in clear(None, up) and untouched()
    finally:
        pkg.set_arithmetic(pkg.FAST)
    assert allsky(good, None, up) == "tlev is required for ecckd" and untouched()
    m = both(tlev, pkg.FluxesBroadband(upc, None), up)
    assert "ecckd_lw_fluxes_clear_allsky: null argument" in m and untouched()
    assert "a clear-sky output must not be an all-sky output" in both(tlev, pkg.FluxesBroadband(dn, upc), upc) and untouched()
    for j in (up, dn):
        for m in (allsky(good, tlev, j), allsky(good, tlev, j, mask), both(tlev, fc, j)):
            assert "ecckd_lw_fluxes_jac: flux_up_jac must not be another output" in m and untouched()
    for j in (upc, dnc):
        assert "ecckd_lw_fluxes_jac: flux_up_jac must not be another output" in both(tlev, fc, j) and untouched()
    for m in (allsky(good, tlev, jac), allsky(good, tlev, jac, mask), both(tlev, fc, jac), clear(tlev, jac)):
        assert "no CPU fallback" in m and untouched()
    assert np.all(good.tau == 0.5) and np.all(good.ssa == 0.5) and np.all(mask == 5)

    # clear-sky outputs, a mask or a band count without tau_p select the clear-sky form: the host-only refusal, at the C ABI
    L = pkg.lib()
    P = lambda a: C.c_void_p(a.ctypes.data)
    names = b"h2o".ljust(32, b" ")
    vmr = (C.c_void_p * 1)(None)
    z, sc = (C.c_longlong * 1)(0), (C.c_double * 1)(1e-3)
    def raw(nband_p=0, mask_=None, upc_=None, dnc_=None, j=jac):
        return L.ecckd_lw_fluxes_jac(k._need(), NCOL, NLAY, P(plev), P(tlay), P(tsfc), P(tlev), 1, names, vmr, z, z, sc, 1, 1,
                                     P(emis), None, nband_p, None, None, None if mask_ is None else P(mask_), P(up), P(dn),
                                     None if upc_ is None else P(upc_), None if dnc_ is None else P(dnc_),
                                     None if j is None else P(j), pkg.HOST, None)
    for kw in (dict(upc_=upc, dnc_=dnc), dict(dnc_=dnc), dict(mask_=mask), dict(nband_p=nb), dict(upc_=upc, j=None),
               dict(upc_=upc, dnc_=dnc, j=up)):
        assert raw(**kw) == 1 and "no CPU fallback" in pkg.last_error() and untouched(), kw
    assert raw() == 1 and "no CPU fallback" in pkg.last_error() and untouched()
    assert raw(j=None) == 1 and "no CPU fallback" in pkg.last_error() and untouched()   # (forwards to ecckd_lw_fluxes)


def test_solver_and_planck_refusals(pkg):
    """ecckd_rte_lw_jac: the argument refusals of ecckd_rte_lw first, then a NULL sfc_source_jac or flux_up_jac, then an
    aliased flux_up_jac, each before any device is asked for; ecckd_planck_sfc_source_jac: the list of
    ecckd_planck_sources for its arguments."""
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=-1) == ""
    ng, nb = k.get_ngpt(), k.get_nband()
    op = pkg.OpticalProps1scl(); op.alloc_1scl(NCOL, NLAY, k)
    src = pkg.SourceFuncLW(); src.alloc(NCOL, NLAY, k)
    for a in (op.tau, src.lay_source, src.lev_source_inc, src.lev_source_dec, src.sfc_source, src.sfc_source_jac):
        a[:] = 1.0
    emis = np.full((NCOL, nb), 0.98)
    up, dn, jac = outs = _fluxes(3)
    untouched = lambda: all(np.all(a == -7.0) for a in outs)
    fl = pkg.FluxesBroadband(up, dn)
    assert "at least one quadrature point" in pkg.rte_lw(op, True, src, emis, fl, n_gauss_angles=5, flux_up_jac=up) and untouched()
    assert "flux_up_jac must not be one of the flux outputs" in pkg.rte_lw(op, True, src, emis, fl, flux_up_jac=up) and untouched()
    assert "flux_up_jac must not be one of the flux outputs" in pkg.rte_lw(op, True, src, emis, fl, flux_up_jac=dn) and untouched()
    # NULL pointers never leave the Python mirror, so at the C ABI
    L = pkg.lib()
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    b2g = np.ascontiguousarray(op.band2gpt, dtype=np.int32)
    def raw(sj, j, dev=0):
        return L.ecckd_rte_lw_jac(dev, NCOL, NLAY, ng, 1, 1, P(op.tau), P(src.lay_source), P(src.lev_source_inc),
                                  P(src.lev_source_dec), P(src.sfc_source), P(sj), nb, P(b2g), P(emis), None, P(up), P(dn), P(j),
                                  pkg.HOST, None)
    for sj, j in ((None, jac), (src.sfc_source_jac, None), (None, None)):
        assert raw(sj, j) == 1 and "ecckd_rte_lw_jac: null argument" in pkg.last_error() and untouched()
    assert raw(src.sfc_source_jac, jac, dev=99) == 1 and ("bad device ordinal" in pkg.last_error() or "no HIP device" in pkg.last_error())
    assert untouched()
    none = pkg.SourceFuncLW(); none.alloc(NCOL, NLAY, k); none.sfc_source_jac = None
    assert "sfc_source_jac" in pkg.rte_lw(op, True, none, emis, fl, flux_up_jac=jac)

    tsfc = np.full(NCOL, 280.0)
    assert "no CPU fallback" in k.planck_sfc_source_jac(tsfc, src) and np.all(src.sfc_source_jac == 1.0)
    ksw = pkg.GasOpticsEcckd()
    assert ksw.load(SW_WIDE, device=-1) == ""
    sw = pkg.SourceFuncLW(); sw.alloc(NCOL, NLAY, ksw)
    assert "no CPU fallback" in ksw.planck_sfc_source_jac(tsfc, sw)   # (the host-only refusal comes first, as in ecckd_planck_sources)
    assert L.ecckd_planck_sfc_source_jac(None, NCOL, P(tsfc), P(src.sfc_source_jac), pkg.HOST, None) == 1
    assert "null model" in pkg.last_error()


def test_python_mirror_shape_and_dtype_errors(pkg):
    """A Jacobian array or surface term of the wrong shape or type never reaches the library."""
    plev, tlay, tsfc, tlev = _columns()
    gc = pkg.GasConcs(["h2o"]); gc.set_vmr("h2o", 1e-3)
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=-1) == ""
    nb = k.get_nband()
    emis = np.full((NCOL, nb), 0.98)
    good = pkg.OpticalProps2str()
    assert good.alloc_2str_bands(NCOL, NLAY, k) == ""
    up, dn, upc, dnc, jac = _fluxes(5)
    fl, fc = pkg.FluxesBroadband(up, dn), pkg.FluxesBroadband(upc, dnc)
    calls = (lambda j: k.lw_fluxes(plev, tlay, tsfc, tlev, gc, True, emis, fl, flux_up_jac=j),
             lambda j: k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gc, True, emis, good, fl, flux_up_jac=j),
             lambda j: k.lw_fluxes_clear_allsky_jac(plev, tlay, tsfc, tlev, gc, True, emis, good, fl, fc, j))
    for call in calls:
        m = call(jac[1:])
        assert "flux_up_jac" in m and "shape" in m
        m = call(jac.astype(np.float32))
        assert "flux_up_jac" in m and "float64" in m
        assert "flux_up_jac" in call(np.asfortranarray(np.zeros((NLAY + 1, NCOL))))
    assert "flux_up_clear" in k.lw_fluxes_clear_allsky_jac(plev, tlay, tsfc, tlev, gc, True, emis, good, fl,
                                                           pkg.FluxesBroadband(upc[1:], dnc), jac)
    short = pkg.OpticalProps2str()
    short.tau, short.ssa, short.g = good.tau, good.ssa[:, 1:], good.g
    assert "particles.ssa" in k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gc, True, emis, short, fl, flux_up_jac=jac)
    assert "uint64" in k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gc, True, emis, good, fl,
                                          cloud_mask=np.zeros((NLAY, NCOL), dtype=np.int64), flux_up_jac=jac)

    op = pkg.OpticalProps1scl(); op.alloc_1scl(NCOL, NLAY, k)
    src = pkg.SourceFuncLW(); src.alloc(NCOL, NLAY, k)
    m = pkg.rte_lw(op, True, src, emis, fl, flux_up_jac=jac[:, 1:])
    assert "flux_up_jac" in m
    src.sfc_source_jac = src.sfc_source_jac[1:]
    assert "sfc_source_jac" in pkg.rte_lw(op, True, src, emis, fl, flux_up_jac=jac)
    src.sfc_source_jac = np.zeros((k.get_ngpt(), NCOL), dtype=np.float32)
    assert "sfc_source_jac" in pkg.rte_lw(op, True, src, emis, fl, flux_up_jac=jac)
    assert "sfc_source_jac" in k.planck_sfc_source_jac(tsfc, src)
    src.alloc(NCOL, NLAY, k)
    assert "tsfc" in k.planck_sfc_source_jac(tsfc[1:].astype(np.float32), src)
    f32 = pkg.OpticalProps1scl(); f32.alloc_1scl(NCOL, NLAY, k, like=np.empty(0, np.float32))
    assert "float64" in pkg.rte_lw(f32, True, src, emis, fl, flux_up_jac=jac)


def test_jacobian_code_objects(pkg):
    """The Jacobian kernels are in the library under their own names.  The stand-alone kernel -- surface term from the array or from the
    Planck table, times no particles, one- and two-stream particles, the latter two with and without mask -- one wave per
    block, no spilled VGPR, next to the surface-term kernel.  The flux kernels it stands next to keep their names and counts."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = kernel_resources.kernels(pkg.LIB_PATH)
    jac = {n: k for n, k in ks.items() if "rte_lw_jac_kernel<" in n}
    assert len(jac) == 10, list(jac)
    for n, k in jac.items():
        assert k["max_flat_wg"] == 64 and k["spill_vgpr"] == 0 and k["scratch_bytes"] == 0 and k["vgpr"] <= 168, (n, k)
    sfc = [k for n, k in ks.items() if "planck_sfc_jac_kernel" in n]
    assert len(sfc) == 1 and sfc[0]["spill_vgpr"] == 0 and sfc[0]["scratch_bytes"] == 0
    # the Jacobian form of the layer-split kernel: clear sky, one- and two-stream particles, the latter two with and without
    # mask, both series forms; one group of four waves per block (one wave per SIMD), no spilled VGPR
    inl = {n: k for n, k in ks.items() if "rte_lw_split_jac_kernel<" in n}
    assert len(inl) == 10, list(inl)
    for n, k in inl.items():
        assert "rte_lw_split_jac_kernel<15, 4, 32, " in n, n
        assert k["max_flat_wg"] == 256 and k["spill_vgpr"] == 0 and k["vgpr"] <= 512, (n, k)
    for name, count in (("rte_lw_split_both_kernel<", 8), ("rte_lw_split_allsky_kernel<", 4), ("rte_lw_split_mcica_kernel<", 4),
                        ("rte_lw_split_kernel<", 14)):
        assert len([n for n in ks if name in n]) == count, name


@pytest.mark.parametrize("which,nlay", [("fsck", 60), ("rrtmgp", 60), ("fsck", 37), ("rrtmgp", 37)])
def test_the_yardstick_is_the_flux_difference(oracle_mod, which, nlay):
    """The GPU tests pin flux_up_jac to the oracle's rte_lw run with lay_source = lev_source_inc = lev_source_dec = 0, no
    inc_flux and sfc_source = sfc_source(tsfc + 1) - sfc_source(tsfc).  The solver is linear in its sources, so that run must
    be the oracle's flux_up(tsfc + 1) - flux_up(tsfc), within 10 FLUX_ATOL (two flux computations of ~400 W m-2 each against
    one of ~5); its flux_dn is exactly 0, and flipping the orientation gives the same bits.  1 and 3 angles."""
    m = oracle_mod.CkdModel(LW_FSCK if which == "fsck" else LW_RRTMGP)
    ncol = 24
    cols = synthetic.columns(17, ncol, float(np.exp(m.log_pressure[0])), nlay=nlay)
    items = helpers.oracle_gas_items(cols)
    tau, lay, inc, dec, sfc0, err = oracle_mod.gas_optics_int(m, cols["plev"], cols["tlay"], cols["tsfc"], items, cols["tlev"])
    assert err == ""
    sfc1 = oracle_mod.gas_optics_int(m, cols["plev"], cols["tlay"], cols["tsfc"] + 1.0, items, cols["tlev"])[4]
    emis = np.repeat(cols["sfc_emis"][None, :], m.ng, 0)
    zero = np.zeros_like(tau)
    for nmus in (1, 3):
        jac, dn = oracle_mod.rte_lw(tau, zero, zero, zero, emis, sfc1 - sfc0, nmus=nmus)
        u0 = oracle_mod.rte_lw(tau, lay, inc, dec, emis, sfc0, nmus=nmus)[0]
        u1 = oracle_mod.rte_lw(tau, lay, inc, dec, emis, sfc1, nmus=nmus)[0]
        err = float(np.max(np.abs(jac - (u1 - u0))))
        print("yardstick %s %d layers %d angles: %.2e W m-2 K-1 (bar %.0e); surface %.2f ... %.2f, top %.2f ... %.2f" %
              (which, nlay, nmus, err, 10 * FLUX_ATOL, jac[-1].min(), jac[-1].max(), jac[0].min(), jac[0].max()))
        assert err < 10 * FLUX_ATOL and np.all(dn == 0.0) and np.all(jac > 0.0)
        flip = lambda a: np.ascontiguousarray(a[:, ::-1])
        jf = oracle_mod.rte_lw(flip(tau), zero, zero, zero, emis, sfc1 - sfc0, top_at_1=False, nmus=nmus)[0]
        assert np.array_equal(jf[::-1], jac)
        if nmus == 1:
            # the surface value is the sum over g-points of eps * pi * sfc_source_jac (2 pi w = pi), up to the order of the sum
            assert np.allclose(jac[-1], np.sum(emis * np.pi * (sfc1 - sfc0), axis=0), rtol=1e-14, atol=0)


def test_fortran_forms(pkg):
    """The modules bind the three C symbols behind ty_source_func_lw%sfc_source_Jac, ecckd%planck_sfc_source_jac and the
    optional flux_up_Jac of rte_lw, lw_fluxes and lw_fluxes_allsky; the driver takes jac.bin as its 14th argument and refuses
    it with the usage text in sw mode and with device-resident containers."""
    gas = open(os.path.join(pkg.FORTRAN_DIR, "gas_optics_ecckd.F90")).read()
    for sym in ("ecckd_planck_sfc_source_jac", "ecckd_lw_fluxes_jac"):
        assert 'name="%s"' % sym in gas, sym
    assert "procedure, public :: planck_sfc_source_jac" in gas and gas.count("optional :: flux_up_Jac") == 2
    assert 'name="ecckd_rte_lw_jac"' in open(os.path.join(pkg.FORTRAN_DIR, "mo_rte_solvers.F90")).read()
    assert "sfc_source_Jac" in open(os.path.join(pkg.FORTRAN_DIR, "mo_rte_min.F90")).read()
    assert "flux_up_Jac=jac_b" in open(os.path.join(pkg.FORTRAN_DIR, "ecckd_driver.F90")).read()
    drv = pkg.build_fortran()
    if drv is None:
        pytest.skip("no amdflang in this image")
    out = subprocess.run([drv], capture_output=True, text=True)
    assert out.returncode != 0 and "usage: ecckd_driver" in out.stderr and "[jac.bin" in out.stderr
    for mode, dev in (("sw", "0"), ("lw", "1")):
        out = subprocess.run([drv, mode, "none.nc", "none.bin", "none.out", "0", "1", dev, "1", "0", "1", "", "", "", "jac.bin"],
                             capture_output=True, text=True)
        assert out.returncode != 0 and "usage: ecckd_driver" in out.stderr
        assert "a Jacobian output file needs the longwave and device_resident = 0" in out.stderr, (mode, dev)
