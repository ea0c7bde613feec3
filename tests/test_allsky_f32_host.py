"""CPU tests of the single-precision fused calls (ecckd_lw_fluxes_f32, ecckd_lw_fluxes_allsky[_mcica]_f32,
ecckd_lw_fluxes_clear_allsky_f32, ecckd_sw_fluxes_allsky[_mcica]_f32, ecckd_sw_fluxes_clear_allsky_f32 and the two size
functions): declared, exported and bound; on host-only models every call answers with the message of its fp64 namesake, in
its order, then "no CPU fallback", with the outputs untouched; the Python mirror's mixed-precision and float64-only
refusals; the size functions against the layout documented in include/ecckd_hip.h; the code objects of the new kernels."""
import ctypes as C
import os
import sys

import numpy as np

import __graft_entry__ as entry
from conftest import LW_FSCK, LW_RRTMGP, SW_WIDE
from test_mcica_host import _wide_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NLAY, NCOL = 60, 4
CALLS = ("ecckd_lw_fluxes_f32", "ecckd_lw_fluxes_allsky_f32", "ecckd_lw_fluxes_allsky_mcica_f32",
         "ecckd_lw_fluxes_clear_allsky_f32", "ecckd_sw_fluxes_allsky_f32", "ecckd_sw_fluxes_allsky_mcica_f32",
         "ecckd_sw_fluxes_clear_allsky_f32")
SIZES = ("ecckd_lw_fluxes_f32_scratch_bytes", "ecckd_sw_fluxes_allsky_f32_scratch_bytes")


def test_symbols_are_declared_exported_and_bound(pkg):
    L = pkg.lib()
    for s in CALLS + SIZES:
        assert s in entry.exported_symbols(), s
        assert hasattr(L, s) and getattr(L, s).argtypes is not None, s
    # the argument lists of the fp64 namesakes
    assert [len(getattr(L, s).argtypes) for s in CALLS] == [21, 24, 25, 27, 26, 27, 30]
    for s in ("ecckd_lw_fluxes_allsky_mcica", "ecckd_lw_fluxes_clear_allsky", "ecckd_sw_fluxes_allsky_mcica", "ecckd_sw_fluxes_clear_allsky"):
        assert len(getattr(L, s + "_f32").argtypes) == len(getattr(L, s).argtypes), s
    header = open(os.path.join(ROOT, "include", "ecckd_hip.h")).read()
    for s in CALLS + SIZES:
        assert s + "(" in header, s
    assert "Out of scope: the Fortran shim" in header


def _columns(dt):
    return (np.full((NLAY + 1, NCOL), 1e4, dt), np.full((NLAY, NCOL), 250., dt), np.full(NCOL, 250., dt),
            np.full((NLAY + 1, NCOL), 250., dt))


def _fluxes(n, dt, value=-7.0):
    return [np.full((NLAY + 1, NCOL), value, dt) for _ in range(n)]


def _bands(pkg, k, dt, cls=None, extra=0, value=0.5):
    p = (cls or pkg.OpticalProps2str)()
    shape = (k.get_nband() + extra, NLAY, NCOL)
    p.tau = np.full(shape, value, dt)
    if hasattr(p, "ssa"):
        p.ssa, p.g = np.full(shape, value, dt), np.full(shape, value, dt)
    return p


def _longwave_messages(pkg, dt):
    """The refusals of the longwave calls, in order, as (label, message) pairs, for arrays of dtype dt."""
    plev, tlay, tsfc, tlev = _columns(dt)
    gc = pkg.GasConcs(["h2o"]); gc.set_vmr("h2o", 1e-3)
    mask = np.full((NLAY, NCOL), 5, dtype=np.uint64)
    outs = _fluxes(4, dt)
    up, dn, upc, dnc = outs
    fl, fc = pkg.FluxesBroadband(up, dn), pkg.FluxesBroadband(upc, dnc)
    got = []

    def note(label, m):
        assert all(np.all(a == -7.0) for a in outs) and np.all(mask == 5), label
        got.append((label, m))

    wide = _wide_model(pkg)
    emis_w = np.full((NCOL, wide.get_nband()), 0.98, dt)
    pw = _bands(pkg, wide, dt, pkg.OpticalProps1scl, extra=1)
    note("mask too wide", wide.lw_fluxes_allsky(plev, tlay, tsfc, None, gc, True, emis_w, pw, fl, cloud_mask=mask))
    note("mask too wide, both", wide.lw_fluxes_clear_allsky(plev, tlay, tsfc, None, gc, True, emis_w, pw, fl,
                                                            pkg.FluxesBroadband(up, None), cloud_mask=mask))
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=-1) == ""
    emis = np.full((NCOL, k.get_nband()), 0.98, dt)
    good = _bands(pkg, k, dt)
    wrong = _bands(pkg, k, dt, pkg.OpticalProps1scl, extra=1)
    none = pkg.OpticalProps1scl()
    null = pkg.FluxesBroadband(upc, None)
    allsky = lambda p, tlev_, m_=None: k.lw_fluxes_allsky(plev, tlay, tsfc, tlev_, gc, True, emis, p, fl, cloud_mask=m_)
    both = lambda p, tlev_, fc_, m_=mask: k.lw_fluxes_clear_allsky(plev, tlay, tsfc, tlev_, gc, True, emis, p, fl, fc_, cloud_mask=m_)
    pkg.set_arithmetic(pkg.REFERENCE_ORDER)
    try:   # every later refusal is armed too: the earlier one is the one named
        for m_ in (None, mask):
            note("nband_p", allsky(wrong, None, m_))
            note("null planes", allsky(none, None, m_))
            note("arithmetic", allsky(good, None, m_))
        note("nband_p, both", both(wrong, None, null))
        note("arithmetic, both", both(good, None, null))
        # (the clear-sky call asks for the model's device first, as ecckd_lw_fluxes does: a host-only model answers that)
        note("no device, clear, reference order", k.lw_fluxes(plev, tlay, tsfc, tlev, gc, True, emis, fl))
    finally:
        pkg.set_arithmetic(pkg.FAST)
    ksw = pkg.GasOpticsEcckd()
    assert ksw.load(SW_WIDE, device=-1) == ""
    psw = _bands(pkg, ksw, dt, pkg.OpticalProps1scl)
    emis_s = np.full((NCOL, ksw.get_nband()), 0.98, dt)
    note("planck", ksw.lw_fluxes_allsky(plev, tlay, tsfc, None, gc, True, emis_s, psw, fl))
    note("no device, clear, shortwave model", ksw.lw_fluxes(plev, tlay, tsfc, tlev, gc, True, emis_s, fl))
    note("tlev", allsky(good, None))
    note("no device, clear, no tlev", k.lw_fluxes(plev, tlay, tsfc, None, gc, True, emis, fl))
    for m_ in (mask, None):
        note("null clear output", both(good, tlev, null, m_))
        for fc_ in (pkg.FluxesBroadband(dn, upc), pkg.FluxesBroadband(upc, up), pkg.FluxesBroadband(up, dn)):
            note("aliased", both(good, tlev, fc_, m_))
        note("no device, both", both(good, tlev, fc, m_))
        note("no device, allsky", allsky(good, tlev, m_))
    note("no device, clear", k.lw_fluxes(plev, tlay, tsfc, tlev, gc, True, emis, fl))
    assert np.all(good.tau == 0.5) and np.all(good.ssa == 0.5)
    return got


def test_longwave_refusals_are_those_of_the_fp64_calls(pkg):
    """Mask with more than 64 g-points; wrong nband_p; NULL planes; reference-order mode; no Planck table; tlev; a NULL or
    aliased clear-sky output; then a host-only model fails loudly.  float32 arrays give the messages float64 arrays give."""
    m64, m32 = _longwave_messages(pkg, np.float64), _longwave_messages(pkg, np.float32)
    assert m32 == m64
    want = {"mask too wide": "at most 64 g-points, not 65", "nband_p": "nband_p = ", "null planes": "nband_p = 0",
            "arithmetic": "fast arithmetic mode", "planck": "no Planck table", "tlev": "tlev is required for ecckd",
            "angles": "no more than 4", "null clear output": "ecckd_lw_fluxes_clear_allsky: null argument",
            "aliased": "a clear-sky output must not be an all-sky output", "no device": "no CPU fallback"}
    for label, m in m32:
        assert want[label.split(",")[0]] in m, (label, m)


def _shortwave_messages(pkg, dt):
    plev, tlay, _, _ = _columns(dt)
    gc = pkg.GasConcs(["h2o"]); gc.set_vmr("h2o", 1e-3)
    mask = np.full((NLAY, NCOL), 5, dtype=np.uint64)
    outs = _fluxes(6, dt)
    up, dn, dr, upc, dnc, drc = outs
    fl, fc = pkg.FluxesBroadband(up, dn, dr), pkg.FluxesBroadband(upc, dnc, drc)
    mu0 = np.full(NCOL, 0.5, dt)
    got = []

    def note(label, m):
        assert all(np.all(a == -7.0) for a in outs) and np.all(mask == 5), label
        got.append((label, m))

    wide = _wide_model(pkg)
    alb_w = np.full((NCOL, wide.get_nband()), 0.2, dt)
    note("mask too wide", wide.sw_fluxes_allsky(plev, tlay, gc, True, mu0, alb_w, alb_w, _bands(pkg, wide, dt, extra=1), fl,
                                                cloud_mask=mask))
    k = pkg.GasOpticsEcckd()
    assert k.load(SW_WIDE, device=-1) == ""
    alb = np.full((NCOL, k.get_nband()), 0.2, dt)
    good, bad = _bands(pkg, k, dt), _bands(pkg, k, dt, extra=2)
    nog = pkg.OpticalProps2str()
    nog.tau, nog.ssa, nog.g = good.tau, good.ssa, None
    null = pkg.FluxesBroadband(upc, None, drc)
    allsky = lambda p, m_=None: k.sw_fluxes_allsky(plev, tlay, gc, True, mu0, alb, alb, p, fl, cloud_mask=m_)
    both = lambda p, fc_, m_=mask: k.sw_fluxes_clear_allsky(plev, tlay, gc, True, mu0, alb, alb, p, fl, fc_, cloud_mask=m_)
    # delta_scale outside 0 / 1 cannot be said through the Python mirror (it passes a bool): the C call itself
    L = pkg.lib()
    f32 = dt == np.float32
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    names = b"h2o".ljust(pkg.NAME_LEN, b" ")
    one = (C.c_void_p * 1)(None)
    zero = (C.c_longlong * 1)(0)
    sc = (C.c_double * 1)(1e-3)

    def c_call(delta, nb=None, tau=good.tau):
        fn = L.ecckd_sw_fluxes_allsky_mcica_f32 if f32 else L.ecckd_sw_fluxes_allsky_mcica
        rc = fn(k._need(), NCOL, NLAY, P(plev), P(tlay), 1, names, one, zero, zero, sc, 1, P(mu0), None, P(alb), P(alb),
                k.get_nband() if nb is None else nb, None if tau is None else P(tau), P(good.ssa), P(good.g), delta, P(mask),
                P(up), P(dn), P(dr), pkg.HOST, None)
        return pkg.last_error() if rc else ""

    pkg.set_arithmetic(pkg.REFERENCE_ORDER)
    try:
        for m_ in (None, mask):
            note("nband_p", allsky(bad, m_))
            note("null planes", allsky(nog, m_))
            note("arithmetic", allsky(good, m_))
        note("nband_p, both", both(bad, null))
        note("null planes, both", both(nog, null))
        note("arithmetic, both", both(good, null))
        note("nband_p, C", c_call(2, nb=k.get_nband() + 1, tau=None))
        note("null planes, C", c_call(2, tau=None))
        note("delta_scale", c_call(2))
        note("delta_scale, negative", c_call(-1))
        note("arithmetic, C", c_call(1))
    finally:
        pkg.set_arithmetic(pkg.FAST)
    for m_ in (mask, None):
        note("null clear output", both(good, null, m_))
        for fc_ in (pkg.FluxesBroadband(dn, dnc, drc), pkg.FluxesBroadband(upc, dnc, dr), pkg.FluxesBroadband(upc, dr, None),
                    pkg.FluxesBroadband(up, dn, dr)):
            note("aliased", both(good, fc_, m_))
        note("no device, both", both(good, fc, m_))
        note("no device, allsky", allsky(good, m_))
    note("no device, C", c_call(1))
    klw = pkg.GasOpticsEcckd()
    assert klw.load(LW_FSCK, device=-1) == ""
    alb_l = np.full((NCOL, klw.get_nband()), 0.2, dt)
    note("no device, longwave model", klw.sw_fluxes_allsky(plev, tlay, gc, True, mu0, alb_l, alb_l, _bands(pkg, klw, dt), fl))
    assert all(np.all(a == 0.5) for a in (good.tau, good.ssa, good.g))
    return got


def test_shortwave_refusals_are_those_of_the_fp64_calls(pkg):
    """Mask with more than 64 g-points; wrong nband_p; NULL planes; delta_scale outside 0 / 1; reference-order mode; a NULL or
    aliased clear-sky output; then a host-only model fails loudly.  float32 arrays give the messages float64 arrays give."""
    m64, m32 = _shortwave_messages(pkg, np.float64), _shortwave_messages(pkg, np.float32)
    assert m32 == m64
    want = {"mask too wide": "at most 64 g-points, not 65", "nband_p": "nband_p = ", "null planes": "tau_p, ssa_p and g_p are all required",
            "delta_scale": "delta_scale must be 0 or 1", "arithmetic": "fast arithmetic mode",
            "null clear output": "ecckd_sw_fluxes_clear_allsky: null argument",
            "aliased": "a clear-sky output must not be an all-sky output", "no device": "no CPU fallback"}
    for label, m in m32:
        assert want[label.split(",")[0]] in m, (label, m)


def test_python_mixed_precision_and_float64_only_keywords(pkg):
    """A mix of float32 and float64 arrays is refused with the first array of the other precision named; float32 arrays with
    flux_up_jac, rescaled=True, use_2stream=True, lw_fluxes_rescaled, lw_fluxes_clear_allsky_jac or sw_fluxes_daylit are
    refused ("implemented for float64 arrays").  Nothing reaches the library: the outputs stay as they are."""
    f4 = np.float32
    plev, tlay, tsfc, tlev = _columns(f4)
    gc = pkg.GasConcs(["h2o"]); gc.set_vmr("h2o", 1e-3)
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=-1) == ""
    emis = np.full((NCOL, k.get_nband()), 0.98, f4)
    up, dn, upc, dnc, jac = outs = _fluxes(5, f4)
    fl, fc = pkg.FluxesBroadband(up, dn), pkg.FluxesBroadband(upc, dnc)
    good = _bands(pkg, k, f4)
    p64 = _bands(pkg, k, np.float64)
    d = lambda a: a.astype(np.float64)

    def mixed(m, name, kind):
        assert "mixing float32 and float64 arrays" in m and "%s is %s" % (name, kind) in m, m
        assert all(np.all(a == -7.0) for a in outs)

    mixed(k.lw_fluxes(plev, d(tlay), tsfc, tlev, gc, True, emis, fl), "tlay", "float64")
    mixed(k.lw_fluxes(d(plev), d(tlay), d(tsfc), d(tlev), gc, True, d(emis), pkg.FluxesBroadband(d(up), dn)), "flux_dn", "float32")
    mixed(k.lw_fluxes(plev, tlay, tsfc, tlev, gc, True, emis, fl, inc_flux=np.zeros((k.get_ngpt(), NCOL))), "inc_flux", "float64")
    mixed(k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gc, True, emis, p64, fl), "particles.tau", "float64")
    half = pkg.OpticalProps2str(); half.tau, half.ssa, half.g = good.tau, p64.ssa, good.g
    mixed(k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gc, True, emis, half, fl), "particles.ssa", "float64")
    mixed(k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gc, True, emis, good, fl, rescaled=True, flux_up_jac=d(jac)), "flux_up_jac", "float64")
    mixed(k.lw_fluxes_clear_allsky(plev, tlay, tsfc, tlev, gc, True, emis, good, fl, pkg.FluxesBroadband(upc, d(dnc))),
          "flux_dn_clear", "float64")
    for kw, what in ((dict(flux_up_jac=jac), "flux_up_jac"), (dict(rescaled=True), "rescaled=True"),
                     (dict(use_2stream=True), "use_2stream=True")):
        m = k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gc, True, emis, good, fl, **kw)
        assert what in m and "implemented for float64 arrays" in m, m
    m = k.lw_fluxes(plev, tlay, tsfc, tlev, gc, True, emis, fl, flux_up_jac=jac)
    assert "flux_up_jac" in m and "implemented for float64 arrays" in m
    assert "implemented for float64 arrays" in k.lw_fluxes_rescaled(plev, tlay, tsfc, tlev, gc, True, emis, good, fl)
    assert "implemented for float64 arrays" in k.lw_fluxes_clear_allsky_jac(plev, tlay, tsfc, tlev, gc, True, emis, good, fl, fc, jac)

    ksw = pkg.GasOpticsEcckd()
    assert ksw.load(SW_WIDE, device=-1) == ""
    alb = np.full((NCOL, ksw.get_nband()), 0.2, f4)
    mu0 = np.full(NCOL, 0.5, f4)
    sw = _bands(pkg, ksw, f4)
    dr, drc = _fluxes(2, f4)
    fls, fcs = pkg.FluxesBroadband(up, dn, dr), pkg.FluxesBroadband(upc, dnc, drc)
    mixed(ksw.sw_fluxes_allsky(plev, tlay, gc, True, d(mu0), alb, alb, sw, fls), "mu0", "float64")
    mixed(ksw.sw_fluxes_allsky(plev, tlay, gc, True, mu0, alb, alb, sw, pkg.FluxesBroadband(up, dn, d(dr))), "flux_dn_dir", "float64")
    mixed(ksw.sw_fluxes_allsky(plev, tlay, gc, True, mu0, alb, alb, sw, fls, toa_scale=np.ones(NCOL)), "toa_scale", "float64")
    mixed(ksw.sw_fluxes_clear_allsky(plev, tlay, gc, True, mu0, alb, alb, sw, fls, pkg.FluxesBroadband(upc, dnc, d(drc))),
          "flux_dn_dir_clear", "float64")
    swg = pkg.OpticalProps2str(); swg.tau, swg.ssa, swg.g = sw.tau, sw.ssa, d(sw.g)
    mixed(ksw.sw_fluxes_clear_allsky(plev, tlay, gc, True, mu0, alb, alb, swg, fls, fcs), "particles.g", "float64")
    assert "implemented for float64 arrays" in ksw.sw_fluxes_daylit(plev, tlay, gc, True, mu0, alb, alb, fls)
    assert all(np.all(a == -7.0) for a in outs + [dr, drc])
    # a float32 gas array in a float64 call, and the reverse, never reach the library either
    gcv = pkg.GasConcs(["h2o"]); gcv.set_vmr("h2o", np.full((NLAY, NCOL), 1e-3))
    try:
        m = k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gcv, True, emis, good, fl)
    except TypeError as e:
        m = str(e)
    assert "vmr of h2o" in m and "float32" in m


def test_scratch_size_functions(pkg):
    """ecckd_lw_fluxes_f32_scratch_bytes and ecckd_sw_fluxes_allsky_f32_scratch_bytes against the layout documented in
    include/ecckd_hip.h, at three shapes each (a host-only model has no tail split: its solver room is the ring alone)."""
    L = pkg.lib()
    a256 = lambda n: (n + 255) // 256 * 256
    for path in (LW_FSCK, LW_RRTMGP):
        k = pkg.GasOpticsEcckd()
        assert k.load(path, device=-1) == ""
        ng = k.get_ngpt()
        for ncol, nlay in ((1, 60), (130, 37), (33, 137)):
            want = 4 * a256(ncol * nlay * ng * 4) + a256(ncol * ng * 4) + a256(pkg.rte_lw_scratch_bytes(ncol, nlay, ng))
            assert L.ecckd_lw_fluxes_f32_scratch_bytes(k._need(), ncol, nlay) == want, (path, ncol, nlay)
            assert (nlay > 96) == (pkg.rte_lw_scratch_bytes(ncol, nlay, ng) > 0)
    assert L.ecckd_lw_fluxes_f32_scratch_bytes(None, 4, 60) == 0 and L.ecckd_lw_fluxes_f32_scratch_bytes(k._need(), 0, 60) == 0
    k = pkg.GasOpticsEcckd()
    assert k.load(SW_WIDE, device=-1) == ""
    ng, nb = k.get_ngpt(), k.get_nband()
    for ncol, nlay in ((1, 60), (130, 37), (65, 61), (130, 137)):
        room = 0 if nlay <= 60 else pkg.rte_sw_scratch_bytes(ncol, nlay, ng)   # (layer-systolic: partial sums only)
        for delta in (0, 1):
            want = a256(ncol * nlay * ng * 4) + room + 3 * delta * a256(ncol * nlay * nb * 4)
            assert L.ecckd_sw_fluxes_allsky_f32_scratch_bytes(k._need(), ncol, nlay, delta) == want, (ncol, nlay, delta)
    assert L.ecckd_sw_fluxes_allsky_f32_scratch_bytes(None, 4, 60, 1) == 0


def test_code_objects_of_the_new_kernels(pkg):
    """The new kernels are in the library under names of their own.  rte_lw_allsky_f32_kernel: one instantiation per variant
    the single-precision solver takes (exact 60 layers with 32- and 64-bit lane offsets, padded 32 / 48 / 64 / 80 / 96,
    overflow; both series forms), no spilled VGPR and no scratch, one wave per block.  The shortwave ones (two per solver and
    clamp form, the layer-systolic ones for full and ragged layer groups) are counted and their figures printed."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = kernel_resources.kernels(pkg.LIB_PATH)
    lw = {n: k for n, k in ks.items() if "rte_lw_allsky_f32_kernel<" in n}
    assert len(lw) == 16, sorted(lw)
    for n, k in lw.items():
        print("%-100s vgpr %3d sgpr %3d spill v%d/s%d scratch %d B" % (n[:100], k["vgpr"], k["sgpr"], k["spill_vgpr"], k["spill_sgpr"],
                                                                         k["scratch_bytes"]))
        assert k["spill_vgpr"] == 0 and k["scratch_bytes"] == 0 and k["vgpr"] + k["agpr"] <= 512, (n, k)
        assert k["max_flat_wg"] == 64, (n, k)
    for name, count in (("rte_sw_sys_allsky_f32_kernel<", 4), ("rte_sw_sys_mcica_f32_kernel<", 4), ("rte_sw_allsky_f32_kernel<", 2),
                        ("rte_sw_mcica_f32_kernel<", 2)):
        sw = {n: k for n, k in ks.items() if name in n}
        assert len(sw) == count, (name, sorted(sw))
        for n, k in sorted(sw.items()):
            print("%-100s vgpr %3d (+agpr %3d) sgpr %3d spill v%d/s%d scratch %d B" % (
                n[:100], k["vgpr"], k["agpr"], k["sgpr"], k["spill_vgpr"], k["spill_sgpr"], k["scratch_bytes"]))
    # the names the existing host tests count by are not among the new ones
    for n in ks:
        if "_f32_kernel<" in n:
            assert not any(s in n for s in ("rte_sw_allsky_kernel<", "rte_sw_sys_allsky_kernel<", "rte_sw_mcica_kernel<",
                                            "rte_sw_sys_mcica_kernel<", "rte_lw_kernel<", "rte_sw_kernel<", "rte_lw_split_",
                                            "increment_kernel<")), n
