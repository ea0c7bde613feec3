"""CPU tests of the daylit-column calls (ecckd_daylit_columns, ecckd_gather_columns, ecckd_scatter_columns,
ecckd_sw_fluxes_daylit): the symbols and their bindings, every refusal of ecckd_sw_fluxes_daylit with its message and in
its documented order on host-only models (nothing computes on the CPU), the ECCKD_HOST list checks, nday = 0, and the
scratch formula."""
import ctypes as C
import inspect

import numpy as np

import __graft_entry__ as entry
from conftest import SW_WIDE
from test_mcica_host import _wide_model

NLAY, NCOL = 60, 6


def test_symbols_are_declared_exported_and_bound(pkg):
    L = pkg.lib()
    for s in ("ecckd_daylit_columns", "ecckd_daylit_columns_f32", "ecckd_gather_columns", "ecckd_scatter_columns",
              "ecckd_sw_fluxes_daylit_scratch_bytes", "ecckd_sw_fluxes_daylit"):
        assert s in entry.exported_symbols(), s
        assert hasattr(L, s) and getattr(L, s).argtypes is not None, s
    # nday and day_index in front of the argument list of ecckd_sw_fluxes_clear_allsky
    assert len(L.ecckd_sw_fluxes_daylit.argtypes) == len(L.ecckd_sw_fluxes_clear_allsky.argtypes) + 2 == 32
    assert L.ecckd_sw_fluxes_daylit.argtypes[5:] == L.ecckd_sw_fluxes_clear_allsky.argtypes[3:]
    sig = inspect.signature(pkg.GasOpticsEcckd.sw_fluxes_daylit)
    assert list(sig.parameters)[1:] == ["plev", "tlay", "gas_desc", "top_at_1", "mu0", "sfc_alb_dir", "sfc_alb_dif", "fluxes",
                                        "particles", "fluxes_clear", "delta_scale", "toa_scale", "cloud_mask", "day_index",
                                        "mu0_min"]
    assert sig.parameters["delta_scale"].default is True and sig.parameters["mu0_min"].default == 0.0
    for n in ("particles", "fluxes_clear", "toa_scale", "cloud_mask", "day_index"):
        assert sig.parameters[n].default is None
    assert inspect.signature(pkg.daylit_columns).parameters["mu0_min"].default == 0.0
    assert callable(pkg.gather_columns) and callable(pkg.scatter_columns)


def _setup(pkg):
    k = pkg.GasOpticsEcckd()
    assert k.load(SW_WIDE, device=-1) == ""
    gc = pkg.GasConcs(["h2o"]); gc.set_vmr("h2o", 1e-3)
    plev, tlay = np.full((NLAY + 1, NCOL), 1e4), np.full((NLAY, NCOL), 250.)
    mu0 = np.array([0.5, -0.1, 0.3, 0.0, 0.9, -0.4])
    alb = np.full((NCOL, k.get_nband()), 0.2)
    good = pkg.OpticalProps2str()
    assert good.alloc_2str_bands(NCOL, NLAY, k) == ""
    for a in (good.tau, good.ssa, good.g):
        a[:] = 0.5
    return k, gc, plev, tlay, mu0, alb, good


def test_refusals_in_order(pkg):
    """A mask with more than 64 g-points; the all-sky call's list (band count, the particle triple, delta_scale is a bool in
    Python, arithmetic mode); clear sky with all-sky extras; the clear-sky outputs; then this call's own -- nday outside
    0..ncol, the ECCKD_HOST list checks -- and, with valid arguments, a host-only model fails loudly.  Every later refusal is
    armed when an earlier one is asked for.  Outputs, particles and mask stay untouched throughout."""
    k, gc, plev, tlay, mu0, alb, good = _setup(pkg)
    nb = k.get_nband()
    mask = np.full((NLAY, NCOL), 5, dtype=np.uint64)
    outs = [np.full((NLAY + 1, NCOL), -7.0) for _ in range(6)]
    up, dn, dr, upc, dnc, drc = outs
    fl, fc = pkg.FluxesBroadband(up, dn, dr), pkg.FluxesBroadband(upc, dnc, drc)
    untouched = lambda: all(np.all(a == -7.0) for a in outs) and np.all(mask == 5)
    idx = np.array([0, 2, 4], dtype=np.int32)
    too_many = np.arange(NCOL + 1, dtype=np.int32)          # nday = ncol + 1
    unsorted = np.array([2, 0, 4], dtype=np.int32)
    twice = np.array([0, 2, 2], dtype=np.int32)
    outside = np.array([0, 2, NCOL], dtype=np.int32)
    negative = np.array([-1, 2, 4], dtype=np.int32)

    wide = _wide_model(pkg)
    two = pkg.OpticalProps2str()
    two.tau, two.ssa, two.g = (np.full((wide.get_nband() + 1, NLAY, NCOL), 0.5) for _ in range(3))
    walb = np.full((NCOL, wide.get_nband()), 0.2)
    m = wide.sw_fluxes_daylit(plev, tlay, gc, True, mu0, walb, walb, fl, particles=two, fluxes_clear=pkg.FluxesBroadband(upc, None),
                              cloud_mask=mask, day_index=too_many)
    assert "ecckd_sw_fluxes_daylit" in m and "at most 64 g-points, not 65" in m and untouched()

    bad = pkg.OpticalProps2str()
    bad.tau, bad.ssa, bad.g = (np.full((nb + 2, NLAY, NCOL), 0.5) for _ in range(3))
    nog = pkg.OpticalProps2str()
    nog.tau, nog.ssa, nog.g = good.tau, good.ssa, None
    null = pkg.FluxesBroadband(upc, None, drc)
    call = lambda p, fc_, ix, m_=mask, fl_=fl: k.sw_fluxes_daylit(plev, tlay, gc, True, mu0, alb, alb, fl_, particles=p,
                                                                 fluxes_clear=fc_, cloud_mask=m_, day_index=ix)
    pkg.set_arithmetic(pkg.REFERENCE_ORDER)
    try:
        m = call(bad, null, too_many)
        assert "ecckd_sw_fluxes_daylit: nband_p = %d" % (nb + 2) in m and untouched()
        assert "tau_p, ssa_p and g_p are given together or not at all" in call(nog, null, too_many) and untouched()
        # clear sky (no particles) takes no mask and no clear-sky outputs
        for p, fc_, m_ in ((None, None, mask), (None, fc, None)):
            m = call(p, fc_, too_many, m_)
            assert "clear sky (tau_p NULL) takes no ssa_p, g_p, cloud_mask or clear-sky outputs" in m and untouched()
        assert "ecckd_sw_fluxes_daylit: needs the fast arithmetic mode" in call(good, null, too_many) and untouched()
        assert "ecckd_sw_fluxes_daylit: needs the fast arithmetic mode" in call(None, None, too_many, None) and untouched()
    finally:
        pkg.set_arithmetic(pkg.FAST)
    for m_ in (mask, None):
        m = call(good, null, too_many, m_)
        assert "ecckd_sw_fluxes_daylit: null argument" in m and "flux_dn_clear" in m and untouched()
        for fc_ in (pkg.FluxesBroadband(dn, dnc, drc), pkg.FluxesBroadband(upc, dnc, dr), pkg.FluxesBroadband(up, dn, dr)):
            m = call(good, fc_, too_many, m_)
            assert "ecckd_sw_fluxes_daylit: a clear-sky output must not be an all-sky output" in m and untouched()
    # this call's own refusals, for every configuration
    for p, fc_, m_ in ((None, None, None), (good, None, None), (good, None, mask), (good, fc, mask)):
        m = call(p, fc_, too_many, m_)
        assert "ecckd_sw_fluxes_daylit: nday = %d outside 0..%d" % (NCOL + 1, NCOL) in m and untouched()
        for ix in (unsorted, twice, outside, negative):
            m = call(p, fc_, ix, m_)
            assert "ecckd_sw_fluxes_daylit: day_index must be strictly ascending and inside [0,ncol)" in m and untouched()
        # valid arguments: the call gets as far as the device, with a list, with every column and with nday = 0
        for ix in (idx, np.arange(NCOL, dtype=np.int32), np.zeros(0, dtype=np.int32)):
            assert "no CPU fallback" in call(p, fc_, ix, m_) and untouched()
        assert "no CPU fallback" in call(p, fc_, idx, m_, pkg.FluxesBroadband(up, dn)) and untouched()
    assert all(np.all(a == 0.5) for a in (good.tau, good.ssa, good.g))
    # no list given: the selection needs a device of its own and says so
    m = k.sw_fluxes_daylit(plev, tlay, gc, True, mu0, alb, alb, fl)
    assert ("no HIP device" in m or "no CPU fallback" in m) and untouched()


def test_null_list_and_direct_calls(pkg):
    """The C calls directly: day_index NULL with nday > 0 (the Python mirror always has a list), and the refusals of the
    public selection / gather / scatter calls that need no device."""
    k, gc, plev, tlay, mu0, alb, good = _setup(pkg)
    L = pkg.lib()
    up, dn = np.full((NLAY + 1, NCOL), -7.0), np.full((NLAY + 1, NCOL), -7.0)
    P = lambda a: C.c_void_p(a.ctypes.data)
    n, names, ptrs, cs, ls, sc, keep = k._gas_args(gc, NCOL, NLAY, pkg.HOST)
    args = lambda nday, ip: (k._need(), NCOL, NLAY, nday, ip, P(plev), P(tlay), n, names, ptrs, cs, ls, sc, 1, P(mu0), None, P(alb),
                             P(alb), 0, None, None, None, 0, None, P(up), P(dn), None, None, None, None, pkg.HOST, None)
    assert L.ecckd_sw_fluxes_daylit(*args(3, None)) != 0
    assert "ecckd_sw_fluxes_daylit: day_index is NULL with nday > 0" in pkg.last_error()
    assert L.ecckd_sw_fluxes_daylit(*args(-1, None)) != 0
    assert "ecckd_sw_fluxes_daylit: nday = -1 outside 0..%d" % NCOL in pkg.last_error()
    assert L.ecckd_sw_fluxes_daylit(*args(0, None)) != 0        # nday = 0 needs no list: the model is what stops it
    assert "no CPU fallback" in pkg.last_error()
    assert np.all(up == -7.0) and np.all(dn == -7.0)

    idx = np.array([0, 2, 4], dtype=np.int32)
    src, dst = np.arange(NCOL * 3, dtype=np.float64).reshape(3, NCOL), np.full((3, 3), -7.0)
    g = lambda *a: L.ecckd_gather_columns(0, *a, pkg.HOST, None)
    s = lambda *a: L.ecckd_scatter_columns(0, *a, 0.0, pkg.HOST, None)
    for f, who in ((g, "ecckd_gather_columns"), (s, "ecckd_scatter_columns")):
        assert f(0, NCOL, 3, 8, 3, P(idx), P(src), P(dst)) != 0 and who + ": bad ninner / ncol / nouter" in pkg.last_error()
        assert f(1, NCOL, 3, 2, 3, P(idx), P(src), P(dst)) != 0 and who + ": elem_bytes must be 4 or 8" in pkg.last_error()
        assert f(1, NCOL, 3, 8, NCOL + 1, P(idx), P(src), P(dst)) != 0 and who + ": nday = 7 outside 0..6" in pkg.last_error()
        assert f(1, NCOL, 3, 8, 3, None, P(src), P(dst)) != 0 and who + ": day_index is NULL with nday > 0" in pkg.last_error()
        assert f(1, NCOL, 3, 8, 3, P(idx), P(src), None) != 0 and who + ": null argument" in pkg.last_error()
        for bad in ([2, 0, 4], [0, 2, 2], [0, 2, NCOL], [-1, 2, 4]):
            b = np.array(bad, dtype=np.int32)
            assert f(1, NCOL, 3, 8, 3, P(b), P(src), P(dst)) != 0
            assert who + ": day_index must be strictly ascending and inside [0,ncol)" in pkg.last_error()
    assert np.all(dst == -7.0)
    nday = C.c_int(-5)
    out = np.zeros(NCOL, dtype=np.int32)
    assert L.ecckd_daylit_columns(0, -1, P(mu0), 0.0, P(out), C.byref(nday), pkg.HOST, None) != 0
    assert "ecckd_daylit_columns: bad ncol" in pkg.last_error()
    assert L.ecckd_daylit_columns(0, NCOL, None, 0.0, P(out), C.byref(nday), pkg.HOST, None) != 0
    assert "ecckd_daylit_columns: null argument" in pkg.last_error()
    assert L.ecckd_daylit_columns(0, NCOL, P(mu0), 0.0, P(out), C.byref(nday), 7, None) != 0
    assert "bad memspace" in pkg.last_error()


def test_scratch_formula(pkg):
    """ecckd_sw_fluxes_daylit_scratch_bytes: 0 without daylit columns, the documented sum (for the two-pass solver, whose
    terms need no device), independent of ncol, and monotone in every argument."""
    k = pkg.GasOpticsEcckd()
    assert k.load(SW_WIDE, device=-1) == ""
    L = pkg.lib()
    ng, nb = k.get_ngpt(), k.get_nband()
    f = lambda ncol=1000, nday=400, nlay=61, ngas=2, part=1, delta=1, mask=1, clear=1: int(
        L.ecckd_sw_fluxes_daylit_scratch_bytes(k._need(), ncol, nday, nlay, ngas, part, delta, mask, clear))
    assert f(nday=0) == 0 and f(nlay=0) == 0
    assert int(L.ecckd_sw_fluxes_daylit_scratch_bytes(None, 1000, 400, 61, 2, 1, 1, 1, 1)) == 0
    a = lambda n: (n + 255) // 256 * 256
    nday, nlay = 400, 61
    inner = a(nday * nlay * ng * 8) + pkg.rte_sw_scratch_bytes(nday, nlay, ng) + 3 * a(nday * nlay * nb * 8)
    rooms = (a(nday * (nlay + 1) * 8) + a(nday * nlay * 8) + 2 * a(nday * 8) + 2 * a(nb * nday * 8) + 2 * a(nday * nlay * 8) +
             3 * a(nday * nlay * nb * 8) + a(nday * nlay * 8) + 6 * a(nday * (nlay + 1) * 8))
    assert f() == inner + rooms
    assert f(ncol=1000) == f(ncol=400) == f(ncol=10 ** 6)
    # without particles the mask, the scaled planes and the clear-sky outputs take no room
    assert f(part=0) == f(part=0, delta=0, mask=0, clear=0) < f(part=1, delta=0, mask=0, clear=0)
    base = dict(ncol=5000, nday=300, nlay=30, ngas=1, part=0, delta=0, mask=0, clear=0)
    steps = dict(ncol=(5000, 5001, 20000), nday=(300, 301, 1000, 5000), nlay=(30, 31, 60, 61, 62, 137), ngas=(1, 2, 9),
                 part=(0, 1), delta=(0, 1), mask=(0, 1), clear=(0, 1))
    for with_part in (0, 1):
        for name, values in steps.items():
            if name == "part" and with_part:
                continue
            got = [f(**{**base, "part": with_part, name: v}) for v in values]
            assert got == sorted(got), (name, with_part, got)
            if name in ("nday", "nlay", "ngas") or (with_part and name in ("delta", "mask", "clear")):
                assert len(set(got)) == len(got), (name, with_part, got)   # strictly
