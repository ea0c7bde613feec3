"""CPU tests of ecckd_lw_fluxes_clear_allsky / ecckd_sw_fluxes_clear_allsky: the symbols and their bindings, the refusals
in their documented order on host-only models (nothing computes on the CPU), the aliasing refusal, the Python mirror's
shape and dtype errors, the "lw_both_skies" option, the code objects of the dual-sky kernel and the Fortran sources."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as entry
from conftest import LW_FSCK, SW_WIDE
from test_mcica_host import _wide_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NLAY, NCOL = 60, 4


def test_symbols_are_declared_exported_and_bound(pkg):
    L = pkg.lib()
    for s in ("ecckd_lw_fluxes_clear_allsky", "ecckd_sw_fluxes_clear_allsky"):
        assert s in entry.exported_symbols(), s
        assert hasattr(L, s) and getattr(L, s).argtypes is not None, s
    # the McICA forms plus the clear-sky outputs
    assert len(L.ecckd_lw_fluxes_clear_allsky.argtypes) == len(L.ecckd_lw_fluxes_allsky_mcica.argtypes) + 2 == 27
    assert len(L.ecckd_sw_fluxes_clear_allsky.argtypes) == len(L.ecckd_sw_fluxes_allsky_mcica.argtypes) + 3 == 30
    sig = inspect.signature(pkg.GasOpticsEcckd.lw_fluxes_clear_allsky)
    assert list(sig.parameters)[-6:] == ["particles", "fluxes", "fluxes_clear", "n_gauss_angles", "inc_flux", "cloud_mask"]
    assert sig.parameters["n_gauss_angles"].default == 1 and sig.parameters["cloud_mask"].default is None
    sig = inspect.signature(pkg.GasOpticsEcckd.sw_fluxes_clear_allsky)
    assert list(sig.parameters)[-6:] == ["particles", "fluxes", "fluxes_clear", "delta_scale", "toa_scale", "cloud_mask"]
    assert sig.parameters["delta_scale"].default is True and sig.parameters["toa_scale"].default is None


def test_lw_both_skies_option(pkg):
    assert pkg.get_solver_option("lw_both_skies") in (0.0, 1.0)
    before = pkg.get_solver_option("lw_both_skies")
    try:
        for v in (1, 0):
            pkg.set_solver_option("lw_both_skies", v)
            assert pkg.get_solver_option("lw_both_skies") == v
        with pytest.raises(Exception) as e:
            pkg.set_solver_option("lw_both_skies", 2)
        assert "lw_both_skies must be 0" in str(e.value)
    finally:
        pkg.set_solver_option("lw_both_skies", before)


def _columns():
    gc_names = ["h2o"]
    return (np.full((NLAY + 1, NCOL), 1e4), np.full((NLAY, NCOL), 250.), np.full(NCOL, 250.), np.full((NLAY + 1, NCOL), 250.),
            gc_names)


def _fluxes(n, value=-7.0):
    return [np.full((NLAY + 1, NCOL), value) for _ in range(n)]


def test_longwave_refusals_in_order(pkg):
    """A mask with more than 64 g-points; the unmasked all-sky call's list in its order (band count, tau_p, arithmetic mode,
    Planck table, tlev); a NULL clear-sky output; a clear-sky output that is an all-sky output; then, with valid arguments, a
    host-only model fails loudly.  Outputs, particles and mask stay untouched throughout."""
    plev, tlay, tsfc, tlev, names = _columns()
    gc = pkg.GasConcs(names); gc.set_vmr("h2o", 1e-3)
    mask = np.full((NLAY, NCOL), 5, dtype=np.uint64)
    up, dn, upc, dnc = outs = _fluxes(4)
    fl, fc = pkg.FluxesBroadband(up, dn), pkg.FluxesBroadband(upc, dnc)
    untouched = lambda: all(np.all(a == -7.0) for a in outs) and np.all(mask == 5)

    wide = _wide_model(pkg)
    part = pkg.OpticalProps1scl()
    part.tau = np.full((wide.get_nband() + 1, NLAY, NCOL), 0.5)
    emis = np.full((NCOL, wide.get_nband()), 0.98)
    m = wide.lw_fluxes_clear_allsky(plev, tlay, tsfc, None, gc, True, emis, part, fl, pkg.FluxesBroadband(up, None), cloud_mask=mask)
    assert "at most 64 g-points, not 65" in m and untouched()
    assert "nband_p" in wide.lw_fluxes_clear_allsky(plev, tlay, tsfc, None, gc, True, emis, part, fl, pkg.FluxesBroadband(up, None))

    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=-1) == ""
    nb = k.get_nband()
    emis = np.full((NCOL, nb), 0.98)
    wrong = pkg.OpticalProps1scl(); wrong.tau = np.full((nb + 1, NLAY, NCOL), 0.5)
    none = pkg.OpticalProps1scl()
    good = pkg.OpticalProps2str()
    assert good.alloc_2str_bands(NCOL, NLAY, k) == ""
    for a in (good.tau, good.ssa, good.g):
        a[:] = 0.5
    alias = pkg.FluxesBroadband(dn, upc)   # (flux_up_clear is the all-sky flux_dn)
    null = pkg.FluxesBroadband(upc, None)
    call = lambda p, tlev_, fc_, m_=mask: k.lw_fluxes_clear_allsky(plev, tlay, tsfc, tlev_, gc, True, emis, p, fl, fc_, cloud_mask=m_)
    pkg.set_arithmetic(pkg.REFERENCE_ORDER)
    try:   # every later refusal is armed too: the earlier one is the one named
        assert "nband_p = %d" % (nb + 1) in call(wrong, None, null) and untouched()
        m = call(none, None, null)
        assert "nband_p = 0" in m and untouched()
        assert "fast arithmetic mode" in call(good, None, null) and untouched()
    finally:
        pkg.set_arithmetic(pkg.FAST)
    # a shortwave model has the band count of its own, so the Planck-table refusal is reached with matching particles
    ksw = pkg.GasOpticsEcckd()
    assert ksw.load(SW_WIDE, device=-1) == ""
    psw = pkg.OpticalProps1scl(); psw.tau = np.full((ksw.get_nband(), NLAY, NCOL), 0.5)
    m = ksw.lw_fluxes_clear_allsky(plev, tlay, tsfc, None, gc, True, np.full((NCOL, ksw.get_nband()), 0.98), psw, fl, null)
    assert "no Planck table" in m and untouched()
    assert call(good, None, null) == "tlev is required for ecckd" and untouched()
    for m_ in (mask, None):
        m = call(good, tlev, null, m_)
        assert "ecckd_lw_fluxes_clear_allsky: null argument" in m and "flux_dn_clear" in m and untouched()
        m = call(good, tlev, pkg.FluxesBroadband(None, dnc), m_)
        assert "ecckd_lw_fluxes_clear_allsky: null argument" in m and untouched()
        for fc_ in (alias, pkg.FluxesBroadband(upc, up), pkg.FluxesBroadband(up, dn)):
            m = call(good, tlev, fc_, m_)
            assert "ecckd_lw_fluxes_clear_allsky: a clear-sky output must not be an all-sky output" in m and untouched()
        assert "no CPU fallback" in call(good, tlev, fc, m_) and untouched()
    assert np.all(good.tau == 0.5) and np.all(good.ssa == 0.5)


def test_shortwave_refusals_in_order(pkg):
    plev, tlay, tsfc, tlev, names = _columns()
    gc = pkg.GasConcs(names); gc.set_vmr("h2o", 1e-3)
    mask = np.full((NLAY, NCOL), 5, dtype=np.uint64)
    outs = _fluxes(6)
    up, dn, dr, upc, dnc, drc = outs
    fl, fc = pkg.FluxesBroadband(up, dn, dr), pkg.FluxesBroadband(upc, dnc, drc)
    untouched = lambda: all(np.all(a == -7.0) for a in outs) and np.all(mask == 5)
    mu0 = np.full(NCOL, 0.5)

    wide = _wide_model(pkg)
    two = pkg.OpticalProps2str()
    two.tau, two.ssa, two.g = (np.full((wide.get_nband() + 1, NLAY, NCOL), 0.5) for _ in range(3))
    alb = np.full((NCOL, wide.get_nband()), 0.2)
    m = wide.sw_fluxes_clear_allsky(plev, tlay, gc, True, mu0, alb, alb, two, fl, pkg.FluxesBroadband(upc, None), cloud_mask=mask)
    assert "at most 64 g-points, not 65" in m and untouched()

    k = pkg.GasOpticsEcckd()
    assert k.load(SW_WIDE, device=-1) == ""
    nb = k.get_nband()
    alb = np.full((NCOL, nb), 0.2)
    good = pkg.OpticalProps2str()
    assert good.alloc_2str_bands(NCOL, NLAY, k) == ""
    for a in (good.tau, good.ssa, good.g):
        a[:] = 0.5
    bad = pkg.OpticalProps2str()
    bad.tau, bad.ssa, bad.g = (np.full((nb + 2, NLAY, NCOL), 0.5) for _ in range(3))
    nog = pkg.OpticalProps2str()
    nog.tau, nog.ssa, nog.g = good.tau, good.ssa, None
    null = pkg.FluxesBroadband(upc, None, drc)
    call = lambda p, fc_, m_=mask: k.sw_fluxes_clear_allsky(plev, tlay, gc, True, mu0, alb, alb, p, fl, fc_, cloud_mask=m_)
    pkg.set_arithmetic(pkg.REFERENCE_ORDER)
    try:
        assert "nband_p = %d" % (nb + 2) in call(bad, null) and untouched()
        assert "tau_p, ssa_p and g_p are all required" in call(nog, null) and untouched()
        assert "fast arithmetic mode" in call(good, null) and untouched()
    finally:
        pkg.set_arithmetic(pkg.FAST)
    for m_ in (mask, None):
        m = call(good, null, m_)
        assert "ecckd_sw_fluxes_clear_allsky: null argument" in m and "flux_dn_clear" in m and untouched()
        for fc_ in (pkg.FluxesBroadband(dn, dnc, drc), pkg.FluxesBroadband(upc, dnc, dr), pkg.FluxesBroadband(upc, dr, None),
                    pkg.FluxesBroadband(up, dn, dr)):
            m = call(good, fc_, m_)
            assert "ecckd_sw_fluxes_clear_allsky: a clear-sky output must not be an all-sky output" in m and untouched()
        # flux_dir may be absent on either side, independently: the call gets as far as the device
        for fl_, fc_ in ((fl, fc), (pkg.FluxesBroadband(up, dn), fc), (fl, pkg.FluxesBroadband(upc, dnc)),
                         (pkg.FluxesBroadband(up, dn), pkg.FluxesBroadband(upc, dnc))):
            m = k.sw_fluxes_clear_allsky(plev, tlay, gc, True, mu0, alb, alb, good, fl_, fc_, cloud_mask=m_)
            assert "no CPU fallback" in m and untouched()
    assert all(np.all(a == 0.5) for a in (good.tau, good.ssa, good.g))


def test_python_mirror_shape_and_dtype_errors(pkg):
    """Outputs, particles and masks of the wrong shape or type never reach the library."""
    plev, tlay, tsfc, tlev, names = _columns()
    gc = pkg.GasConcs(names); gc.set_vmr("h2o", 1e-3)
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=-1) == ""
    nb = k.get_nband()
    emis = np.full((NCOL, nb), 0.98)
    good = pkg.OpticalProps2str()
    assert good.alloc_2str_bands(NCOL, NLAY, k) == ""
    up, dn, upc, dnc = _fluxes(4)
    fl, fc = pkg.FluxesBroadband(up, dn), pkg.FluxesBroadband(upc, dnc)
    mask = np.zeros((NLAY, NCOL), dtype=np.uint64)
    call = lambda fl_=fl, fc_=fc, p=good, m_=None: k.lw_fluxes_clear_allsky(plev, tlay, tsfc, tlev, gc, True, emis, p, fl_, fc_,
                                                                            cloud_mask=m_)
    m = call(fc_=pkg.FluxesBroadband(upc[1:], dnc))
    assert "flux_up_clear" in m and "shape" in m
    m = call(fc_=pkg.FluxesBroadband(upc, dnc.astype(np.float32)))
    assert "flux_dn_clear" in m and "float64" in m
    assert "flux_dn_clear" in call(fc_=pkg.FluxesBroadband(upc, np.asfortranarray(np.zeros((NLAY + 1, NCOL)))))
    assert "flux_up" in call(fl_=pkg.FluxesBroadband(np.ascontiguousarray(up[:, 1:]), dn))
    short = pkg.OpticalProps2str()
    short.tau, short.ssa, short.g = good.tau, good.ssa[:, 1:], good.g
    assert "particles.ssa" in call(p=short)
    assert "uint64" in call(m_=mask.astype(np.int64))
    assert "shape" in call(m_=mask[1:])

    ksw = pkg.GasOpticsEcckd()
    assert ksw.load(SW_WIDE, device=-1) == ""
    nbs = ksw.get_nband()
    alb = np.full((NCOL, nbs), 0.2)
    sw = pkg.OpticalProps2str()
    assert sw.alloc_2str_bands(NCOL, NLAY, ksw) == ""
    dr, drc = _fluxes(2)
    swcall = lambda fl_, fc_, m_=None: ksw.sw_fluxes_clear_allsky(plev, tlay, gc, True, np.full(NCOL, 0.5), alb, alb, sw, fl_, fc_,
                                                                  cloud_mask=m_)
    m = swcall(pkg.FluxesBroadband(up, dn, dr), pkg.FluxesBroadband(upc, dnc, drc[1:]))
    assert "flux_dn_dir_clear" in m and "shape" in m
    m = swcall(pkg.FluxesBroadband(up, dn, dr.astype(np.float32)), pkg.FluxesBroadband(upc, dnc, drc))
    assert "flux_dn_dir" in m and "float64" in m
    assert "flux_up_clear" in swcall(pkg.FluxesBroadband(up, dn, dr), pkg.FluxesBroadband(upc[:, :2], dnc, drc))
    assert "uint64" in swcall(pkg.FluxesBroadband(up, dn), pkg.FluxesBroadband(upc, dnc), mask.astype(np.float64))


def test_dual_sky_code_objects(pkg):
    """rte_lw_split_both_kernel is in the library under its own name: one-stream, two-stream and mask variants for both
    series forms, one group of four waves per block (one wave per SIMD), no spilled VGPR.  The kernels it stands next to
    keep their names and counts."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = kernel_resources.kernels(pkg.LIB_PATH)
    both = {n: k for n, k in ks.items() if "rte_lw_split_both_kernel<" in n}
    assert len(both) == 8, list(both)
    for n, k in both.items():
        assert "rte_lw_split_both_kernel<15, 4, 32, " in n, n
        assert k["max_flat_wg"] == 256 and k["spill_vgpr"] == 0 and k["vgpr"] <= 512, (n, k)
    for name, count in (("rte_lw_split_allsky_kernel<", 4), ("rte_lw_split_mcica_kernel<", 4), ("rte_lw_split_kernel<", 14)):
        assert len([n for n in ks if name in n]) == count, name


def test_fortran_forms(pkg):
    """The module binds the two C symbols behind the optional clear-sky arguments of lw_fluxes_allsky / sw_fluxes_allsky, the
    driver takes the second output file, and a clear-sky file without a particle file is refused with the usage text."""
    text = open(os.path.join(pkg.FORTRAN_DIR, "gas_optics_ecckd.F90")).read()
    for sym in ("ecckd_lw_fluxes_clear_allsky", "ecckd_sw_fluxes_clear_allsky"):
        assert 'name="%s"' % sym in text, sym
    assert "optional :: flux_up_clear, flux_dn_clear, flux_dir_clear" in text and "optional :: flux_up_clear, flux_dn_clear\n" in text
    drv_text = open(os.path.join(pkg.FORTRAN_DIR, "ecckd_driver.F90")).read()
    assert "flux_up_clear=clear_up(c0:c1, :)" in drv_text
    drv = pkg.build_fortran()
    if drv is None:
        pytest.skip("no amdflang in this image")
    out = subprocess.run([drv], capture_output=True, text=True)
    assert out.returncode != 0 and "usage: ecckd_driver" in out.stderr and "[clear.bin" in out.stderr
    for fused, part in (("1", ""), ("0", "part.bin")):
        out = subprocess.run([drv, "lw", "none.nc", "none.bin", "none.out", "0", "1", "0", "1", "0", fused, part, "", "clear.bin"],
                             capture_output=True, text=True)
        assert out.returncode != 0 and "usage: ecckd_driver" in out.stderr
        assert "a clear-sky output file needs fused = 1 and a particle file (particles.bin)" in out.stderr, (fused, part)
