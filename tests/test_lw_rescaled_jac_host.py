"""CPU tests of the rescaled longwave solver's clear-sky outputs and surface-temperature Jacobian (include/ecckd_hip.h,
"Rescaled longwave: clear sky and Jacobian"): the symbols and the Python surface, the scratch arithmetic, the refusals in
their documented order on host-only models (nothing computes on the CPU and no device is asked for before a refusal), and
the yardstick of the GPU tests -- the numpy restatement tests/lw_rescaled_ref.py run with every source zero -- against a
finite difference of the restatement in the surface source."""
import ctypes as C
import inspect

import numpy as np

import __graft_entry__ as entry
import lw_rescaled_ref as ref
from conftest import LW_FSCK, SW_WIDE
from test_lw_rescaled_host import _solver_inputs, _wide_model, random_case, run

NLAY, NCOL = 5, 4


def test_symbols_bindings_and_signatures(pkg):
    L = pkg.lib()
    counts = dict(ecckd_rte_lw_rescaled_jac=23, ecckd_lw_fluxes_rescaled_jac=29, ecckd_lw_fluxes_rescaled_jac_scratch_bytes=4)
    for s, n in counts.items():
        assert s in entry.exported_symbols() and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None and len(getattr(L, s).argtypes) == n, s
    # two / three more arguments than the calls they extend
    assert len(L.ecckd_rte_lw_rescaled.argtypes) == 21 and len(L.ecckd_lw_fluxes_allsky_rescaled.argtypes) == 26
    assert list(inspect.signature(pkg.rte_lw_rescaled_jac).parameters) == [
        "optical_props", "top_at_1", "sources", "sfc_emis", "fluxes", "flux_up_jac", "n_gauss_angles", "device", "inc_flux"]
    p = inspect.signature(pkg.GasOpticsEcckd.lw_fluxes_rescaled).parameters
    assert list(p) == ["self", "plev", "tlay", "tsfc", "tlev", "gas_desc", "top_at_1", "sfc_emis", "particles", "fluxes", "fluxes_clear",
                       "flux_up_jac", "n_gauss_angles", "inc_flux", "cloud_mask"]
    assert p["fluxes_clear"].default is None and p["flux_up_jac"].default is None and p["n_gauss_angles"].default == 1
    assert inspect.signature(pkg.rte_lw_rescaled_jac).parameters["n_gauss_angles"].default == 1
    # the existing entry points keep their argument lists
    for f in (pkg.rte_lw, pkg.GasOpticsEcckd.lw_fluxes_allsky):
        assert list(inspect.signature(f).parameters)[-3:] == ["rescaled", "use_2stream", "flux_up_jac"]


def test_scratch_arithmetic(pkg):
    """with_clear = 0 is the existing call's block; with_clear adds what the clear pass needs on its general route: nothing
    at 60 layers (the shipped model's table fits the clear-sky layer-split kernel), else the no-scattering solver's ring."""
    L = pkg.lib()
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=-1) == ""
    ng = k.get_ngpt()
    r32 = lambda n: (n + 31) // 32 * 32
    old = lambda ncol, nlay: int(L.ecckd_lw_fluxes_allsky_rescaled_scratch_bytes(k._need(), ncol, nlay))
    new = lambda ncol, nlay, c: int(L.ecckd_lw_fluxes_rescaled_jac_scratch_bytes(k._need(), ncol, nlay, c))
    for ncol, nlay in ((1, 1), (17, 61), (37, 137), (1000, 60), (16, 8), (10**5, 59), (300, 200)):
        assert new(ncol, nlay, 0) == old(ncol, nlay) > 0
        ring = pkg.rte_lw_scratch_bytes(ncol, nlay, ng)
        assert ring % 8 == 0
        assert new(ncol, nlay, 1) == old(ncol, nlay) + (0 if nlay == 60 else 8 * r32(ring // 8)), (ncol, nlay)
        assert new(ncol, nlay, 7) == new(ncol, nlay, 1) == k.lw_fluxes_rescaled_scratch_bytes(ncol, nlay, True)
        assert k.lw_fluxes_rescaled_scratch_bytes(ncol, nlay) == old(ncol, nlay)
    assert pkg.rte_lw_scratch_bytes(300, 200, ng) > 0          # (a ring exists among the cases)
    assert new(1000, 60, 0) == 8 * r32(1000 * 60 * ng)
    assert new(0, 60, 1) == 0 and new(5, 0, 1) == 0 and int(L.ecckd_lw_fluxes_rescaled_jac_scratch_bytes(None, 5, 5, 1)) == 0


def test_solver_refusals_in_order(pkg):
    """ecckd_rte_lw_rescaled_jac: the list of ecckd_rte_lw_rescaled in its order, then sfc_source_jac or flux_up_jac NULL, then
    flux_up_jac equal to a flux output -- each with every later refusal armed, the outputs untouched, no device asked for.
    Then the mirror."""
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=-1) == ""
    ng, nb = k.get_ngpt(), k.get_nband()
    op, src = _solver_inputs(pkg, k)
    emis = np.full((NCOL, nb), 0.98)
    sjac = np.full((ng, NCOL), 0.1)
    up, dn, jac = outs = [np.full((NLAY + 1, NCOL), -7.0) for _ in range(3)]
    untouched = lambda: all(np.all(a == -7.0) for a in outs)
    L = pkg.lib()
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    b2g = np.ascontiguousarray(op.band2gpt, dtype=np.int32)
    args = dict(tau=op.tau, ssa=op.ssa, g=op.g, lay=src.lay_source, inc=src.lev_source_inc, dec=src.lev_source_dec,
                sfc=src.sfc_source, sjac=sjac, emis=emis, incf=None, up=up, dn=dn, jac=jac)

    def raw(ncol=NCOL, nlay=NLAY, ngpt=ng, nmus=1, nband=nb, b2=b2g, memspace=pkg.HOST, dev=0, **kw):
        a = dict(args, **kw)
        return L.ecckd_rte_lw_rescaled_jac(dev, ncol, nlay, ngpt, 1, nmus, P(a["tau"]), P(a["ssa"]), P(a["g"]), P(a["lay"]), P(a["inc"]),
                                           P(a["dec"]), P(a["sfc"]), P(a["sjac"]), nband, P(b2), P(a["emis"]), P(a["incf"]), P(a["up"]),
                                           P(a["dn"]), P(a["jac"]), memspace, None)
    later = dict(sjac=None, jac=up)   # this call's own refusals, armed behind everything of the existing list
    assert raw(ncol=-1, nmus=0, tau=None, memspace=7, **later) == 1 and "bad ncol/nlay" in pkg.last_error()
    assert raw(nlay=0, nmus=0, tau=None, memspace=7, **later) == 1 and "bad ncol/nlay" in pkg.last_error()
    for nmus in (0, 5):
        assert raw(nmus=nmus, tau=None, memspace=7, **later) == 1 and "at least one quadrature point and no more than 4" in pkg.last_error()
    for name in ("tau", "ssa", "g", "lay", "inc", "dec", "sfc", "emis", "up", "dn"):
        kw = dict(later, **{name: None})
        assert raw(ngpt=300, memspace=7, **kw) == 1 and "ecckd_rte_lw_rescaled: null argument" in pkg.last_error(), name
    assert raw(ngpt=300, memspace=7, **later) == 1 and "ngpt must be in 1..256" in pkg.last_error()
    assert raw(b2=None, memspace=7, **later) == 1 and "bad band description" in pkg.last_error()
    bad = b2g.copy(); bad[0, 0] = 2
    assert raw(b2=bad, memspace=7, **later) == 1 and "band2gpt" in pkg.last_error()
    assert raw(memspace=2, **later) == 1 and "ecckd_rte_lw_rescaled: ECCKD_MIXED is not implemented" in pkg.last_error()
    assert raw(memspace=7, **later) == 1 and pkg.last_error() == "ecckd: bad memspace"
    for kw in (dict(sjac=None, jac=up), dict(jac=None)):
        assert raw(dev=99, **kw) == 1 and "ecckd_rte_lw_rescaled_jac: null argument (sfc_source_jac and flux_up_jac" in pkg.last_error(), kw
    for same in (up, dn):
        assert raw(dev=99, jac=same) == 1 and "flux_up_jac must not be one of the flux outputs" in pkg.last_error()
    # valid arguments: the device is asked for, and there is none or not this one
    assert raw(nmus=4, dev=99) == 1 and ("bad device ordinal" in pkg.last_error() or "no HIP device" in pkg.last_error())
    assert untouched()

    # the mirror
    fl = pkg.FluxesBroadband(up, dn)
    src.sfc_source_jac = sjac
    call = lambda o=op, f=fl, j=jac, s=src, **kw: pkg.rte_lw_rescaled_jac(o, True, s, emis, f, j, **kw)
    one = pkg.OpticalProps1scl(); one.alloc_1scl(NCOL, NLAY, k)
    assert "two-stream optical properties required" in call(one)
    op32, _ = _solver_inputs(pkg, k, np.float32)
    assert "float64" in call(op32)
    bnd = [np.zeros((nb, NLAY + 1, NCOL)) for _ in range(2)]
    assert "per-band fluxes" in call(f=pkg.FluxesByband(bnd[0], bnd[1]))
    assert "flux_up_jac is required" in call(j=None)
    bare = pkg.SourceFuncLW()
    bare.lay_source, bare.lev_source_inc, bare.lev_source_dec, bare.sfc_source = src.lay_source, src.lev_source_inc, src.lev_source_dec, src.sfc_source
    assert "sfc_source_jac" in call(s=bare)
    assert "flux_up_jac" in call(j=np.zeros((NLAY, NCOL)))                      # shape
    assert "flux_up_jac" in call(j=np.zeros((NLAY + 1, NCOL), np.float32))      # dtype
    assert "inc_flux" in call(inc_flux=np.zeros((ng + 1, NCOL)))
    assert "no more than 4" in call(n_gauss_angles=5)
    assert "must not be one of the flux outputs" in call(j=up)
    m = call(inc_flux=np.zeros((ng, NCOL)), n_gauss_angles=3, device=99)
    assert "bad device ordinal" in m or "no HIP device" in m
    assert untouched()
    # the keyword of rte_lw still refuses, and names where the Jacobian is
    m = pkg.rte_lw(op, True, src, emis, fl, rescaled=True, flux_up_jac=jac)
    assert "flux_up_jac" in m and "rte_lw_rescaled_jac" in m


def test_fused_refusals_in_order(pkg):
    """ecckd_lw_fluxes_rescaled_jac on host-only models: the list of ecckd_lw_fluxes_allsky_rescaled with its messages, then
    exactly one clear-sky output NULL, a clear-sky output that is an all-sky output, flux_up_jac that is another output,
    then the host-only model -- each with every later refusal armed.  Then the mirror and the keyword of lw_fluxes_allsky."""
    L = pkg.lib()
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=-1) == ""
    ksw = pkg.GasOpticsEcckd()
    assert ksw.load(SW_WIDE, device=-1) == ""
    nb = k.get_nband()
    plev, tlay, tsfc, tlev = (np.full((NLAY + 1, NCOL), 1e4), np.full((NLAY, NCOL), 250.), np.full(NCOL, 250.), np.full((NLAY + 1, NCOL), 250.))
    emis = np.full((NCOL, nb), 0.98)
    up, dn, upc, dnc, jac = outs = [np.full((NLAY + 1, NCOL), -7.0) for _ in range(5)]
    untouched = lambda: all(np.all(a == -7.0) for a in outs)
    part = [np.full((nb, NLAY, NCOL), 0.5) for _ in range(3)]
    mask = np.full((NLAY, NCOL), 5, dtype=np.uint64)
    names = b"h2o".ljust(32, b" ")
    vmr = (C.c_void_p * 1)(None)
    z, sc = (C.c_longlong * 1)(0), (C.c_double * 1)(1e-3)

    def raw(model=k, nband_p=nb, tp=part[0], sp=part[1], gp=part[2], m_=None, tlev_=tlev, nmus=1, memspace=pkg.HOST, uc=upc, dc=dnc, j=jac):
        return L.ecckd_lw_fluxes_rescaled_jac(None if model is None else model._need(), NCOL, NLAY, P(plev), P(tlay), P(tsfc),
                                              P(tlev_), 1, names, vmr, z, z, sc, 1, nmus, P(emis), None, nband_p, P(tp), P(sp),
                                              P(gp), P(m_), P(up), P(dn), P(uc), P(dc), P(j), memspace, None)
    later = dict(uc=None, dc=up, j=dn)   # the new refusals, armed behind the existing list
    assert raw(model=None, **later) == 1 and "null model" in pkg.last_error()
    pkg.set_arithmetic(pkg.REFERENCE_ORDER)
    try:
        wide = _wide_model(pkg)
        assert raw(model=wide, nband_p=nb + 7, tp=None, m_=mask, tlev_=None, nmus=0, **later) == 1
        assert "ecckd_lw_fluxes_allsky_rescaled" in pkg.last_error() and "at most 64 g-points, not 65" in pkg.last_error()
        assert raw(model=wide, nband_p=nb + 7, tp=None, tlev_=None, nmus=0, **later) == 1 and "nband_p = %d" % (nb + 7) in pkg.last_error()
        assert raw(nband_p=nb + 1, tp=None, tlev_=None, nmus=0, **later) == 1 and "nband_p = %d" % (nb + 1) in pkg.last_error()
        for kw in (dict(tp=None), dict(sp=None), dict(gp=None)):
            assert raw(tlev_=None, nmus=0, **later, **kw) == 1 and "tau_p, ssa_p and g_p are required" in pkg.last_error(), kw
        assert raw(tlev_=None, nmus=0, **later) == 1 and "ecckd_lw_fluxes_allsky_rescaled: needs the fast arithmetic mode" in pkg.last_error()
    finally:
        pkg.set_arithmetic(pkg.FAST)
    nbs = ksw.get_nband()
    psw = np.full((nbs, NLAY, NCOL), 0.5)
    assert raw(model=ksw, nband_p=nbs, tp=psw, sp=psw, gp=psw, tlev_=None, nmus=0, **later) == 1 and "no Planck table" in pkg.last_error()
    assert raw(tlev_=None, nmus=0, memspace=7, **later) == 1 and pkg.last_error() == "tlev is required for ecckd"
    for nmus in (0, 5):
        assert raw(nmus=nmus, memspace=7, **later) == 1 and "at least one quadrature point and no more than 4" in pkg.last_error()
    # this call's own, in order; the host-only model (and a bad memspace) stay armed behind them
    for kw in (dict(uc=None, dc=up, j=dn), dict(uc=up, dc=None, j=dn)):
        assert raw(memspace=7, **kw) == 1 and "flux_up_clear and flux_dn_clear are given together or not at all" in pkg.last_error(), kw
    for kw in (dict(uc=up), dict(uc=dn), dict(dc=up), dict(dc=dn)):
        assert raw(memspace=7, j=dn, **kw) == 1 and "a clear-sky output must not be an all-sky output" in pkg.last_error(), kw
    for j in (up, dn, upc, dnc):
        assert raw(memspace=7, j=j) == 1 and "ecckd_lw_fluxes_rescaled_jac: flux_up_jac must not be another output" in pkg.last_error()
    for j in (up, dn):   # ... also without clear-sky outputs
        assert raw(memspace=7, uc=None, dc=None, j=j) == 1 and "flux_up_jac must not be another output" in pkg.last_error()
    for kw in (dict(), dict(uc=None, dc=None), dict(j=None), dict(uc=None, dc=None, j=None, m_=mask)):
        assert raw(nmus=4, memspace=7, **kw) == 1 and "no CPU fallback" in pkg.last_error(), kw
    assert untouched() and all(np.all(a == 0.5) for a in part) and np.all(mask == 5)

    # the mirror
    gc = pkg.GasConcs(["h2o"]); gc.set_vmr("h2o", 1e-3)
    fl, flc = pkg.FluxesBroadband(up, dn), pkg.FluxesBroadband(upc, dnc)
    good = pkg.OpticalProps2str()
    assert good.alloc_2str_bands(NCOL, NLAY, k) == ""
    call = lambda p=good, f=fl, **kw: k.lw_fluxes_rescaled(plev, tlay, tsfc, tlev, gc, True, emis, p, f, **kw)
    one = pkg.OpticalProps1scl(); one.alloc_1scl_bands(NCOL, NLAY, k)
    assert "two-stream optical properties on the model's bands" in call(one)
    nog = pkg.OpticalProps2str(); nog.tau, nog.ssa, nog.g = good.tau, good.ssa, None
    assert "with g" in call(nog)
    bnd = [np.zeros((nb, NLAY + 1, NCOL)) for _ in range(2)]
    assert "per-band fluxes" in call(f=pkg.FluxesByband(bnd[0], bnd[1]))
    assert "per-band fluxes" in call(fluxes_clear=pkg.FluxesByband(bnd[0], bnd[1]))
    p32 = pkg.OpticalProps2str(); p32.tau, p32.ssa, p32.g = (np.zeros(good.tau.shape, np.float32) for _ in range(3))
    assert "float64" in call(p32)
    assert "uint64" in call(cloud_mask=np.zeros((NLAY, NCOL), dtype=np.int64))
    assert "flux_up_jac" in call(flux_up_jac=np.zeros((NLAY, NCOL)))
    assert "flux_up_jac" in call(flux_up_jac=np.zeros((NLAY + 1, NCOL), np.float32))
    assert "flux_up_clear" in call(fluxes_clear=pkg.FluxesBroadband(np.zeros((NLAY, NCOL)), dnc))
    assert "given together or not at all" in call(fluxes_clear=pkg.FluxesBroadband(upc, None))
    assert "must not be an all-sky output" in call(fluxes_clear=pkg.FluxesBroadband(up, dnc))
    assert "must not be another output" in call(fluxes_clear=flc, flux_up_jac=upc)
    assert "no more than 4" in call(n_gauss_angles=5)
    for kw in (dict(), dict(fluxes_clear=flc), dict(flux_up_jac=jac), dict(fluxes_clear=flc, flux_up_jac=jac, cloud_mask=mask, n_gauss_angles=3)):
        assert "no CPU fallback" in call(**kw), kw
    assert untouched()
    # the keyword of lw_fluxes_allsky still refuses, and names where the Jacobian is
    m = k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gc, True, emis, good, fl, rescaled=True, flux_up_jac=jac)
    assert "flux_up_jac" in m and "lw_fluxes_rescaled" in m


def jacobian_case(ncol, nlay, ng, seed):
    """Cloudy cells of test_lw_rescaled_host.random_case with optical depths scaled so that the surface is seen from the top."""
    a = random_case(ncol, nlay, ng, seed)
    a["tau"] = a["tau"] * 0.02
    a["ssa"][:, :, ::3] = 0.0          # columns without scattering
    rng = np.random.default_rng(seed + 1)
    a["sfc_source_jac"] = rng.uniform(0.01, 0.2, (ng, ncol))
    return a


def zero_source_run(a, top_at_1=True, nmus=1):
    zero = np.zeros_like(a["tau"])
    return ref.restate(a["tau"], a["ssa"], a["g"], zero, zero, zero, a["sfc_emis"], a["sfc_source_jac"], None, top_at_1, nmus)


def test_the_yardstick_is_the_derivative_of_the_restatement():
    """The equations are affine in the surface source, so restate(sfc_source + J) - restate(sfc_source) in flux_up equals the
    zero-source run's flux_up to rounding (fluxes up to 1e3 W m-2: 1e-11 is some tens of ulps), both orientations, 1 and 3 angles,
    with inc_flux in the perturbed pair and none in the zero-source run.  The zero-source flux_dn is NOT zero on scattering
    columns -- under rescaling the downward flux depends on the surface temperature too -- and is zero without scattering."""
    worst, dn_max = 0.0, 0.0
    for nlay in (1, 8, 60):
        a = jacobian_case(9, nlay, 5, nlay)
        scat = np.any(a["ssa"] > 0, axis=(0, 1))
        assert scat.any() and (~scat).any()
        for top in (True, False):
            b = a if top else dict(ref.flip_orientation(a), sfc_source_jac=a["sfc_source_jac"])
            for nmus in (1, 3):
                jup, jdn = zero_source_run(b, top, nmus)
                base = run(b, top, nmus)
                moved = run(dict(b, sfc_source=b["sfc_source"] + b["sfc_source_jac"]), top, nmus)
                d = float(np.max(np.abs((moved[0] - base[0]) - jup)))
                worst = max(worst, d)
                assert d <= 1e-11, (nlay, top, nmus, d)
                sfc = -1 if top else 0
                assert np.all(np.abs(jdn[:, sfc][:, scat]) > 0.0) and np.all(jdn[:, :, ~scat] == 0.0)
                assert np.all(jup > 0.0)
                dn_max = max(dn_max, float(np.max(ref.broadband(jdn))))
                # ... and the downward derivative is what the finite difference shows as well
                assert float(np.max(np.abs((moved[1] - base[1]) - jdn))) <= 1e-11
    print("zero-source flux_up against the finite difference of the restatement: %.2e W m-2 K-1; zero-source flux_dn up to %.3f" % (worst, dn_max))
    assert dn_max > 1e-3
