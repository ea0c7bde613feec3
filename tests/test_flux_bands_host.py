"""CPU tests of ecckd_lw_flux_bands / ecckd_sw_flux_bands (fused per-band fluxes): the four symbols and their bindings, the
refusals in the order include/ecckd_hip.h documents -- on host-only models of the three data files, called through ctypes so
that every argument can be armed on its own --, the scratch sizes against the documented formulas, and the answers of the
Python methods to a FluxesBroadband, float32 arrays and a mixed-precision call.  Nothing computes on the CPU."""
import ctypes as C
import inspect

import numpy as np
import pytest

import __graft_entry__ as entry
from conftest import LW_FSCK, LW_RRTMGP, SW_WIDE
from test_mcica_host import _wide_model

NLAY, NCOL = 60, 4
SYMBOLS = ("ecckd_lw_flux_bands", "ecckd_sw_flux_bands", "ecckd_lw_flux_bands_scratch_bytes", "ecckd_sw_flux_bands_scratch_bytes")


def test_symbols_are_declared_exported_and_bound(pkg):
    L = pkg.lib()
    for s in SYMBOLS:
        assert s in entry.exported_symbols(), s
        assert hasattr(L, s) and getattr(L, s).argtypes is not None, s
        assert "_fluxes" not in s   # (tests/test_fused_call_marshalling_host.py pins every symbol that has it)
    # the McICA forms plus the band planes
    assert len(L.ecckd_lw_flux_bands.argtypes) == len(L.ecckd_lw_fluxes_allsky_mcica.argtypes) + 2 == 27
    assert len(L.ecckd_sw_flux_bands.argtypes) == len(L.ecckd_sw_fluxes_allsky_mcica.argtypes) + 3 == 30
    assert L.ecckd_lw_flux_bands_scratch_bytes.restype is C.c_size_t and L.ecckd_sw_flux_bands_scratch_bytes.restype is C.c_size_t
    sig = inspect.signature(pkg.GasOpticsEcckd.lw_fluxes_byband)
    assert list(sig.parameters) == ["self", "plev", "tlay", "tsfc", "tlev", "gas_desc", "top_at_1", "sfc_emis", "fluxes",
                                    "n_gauss_angles", "inc_flux", "particles", "cloud_mask"]
    assert sig.parameters["n_gauss_angles"].default == 1
    assert all(sig.parameters[p].default is None for p in ("inc_flux", "particles", "cloud_mask"))
    sig = inspect.signature(pkg.GasOpticsEcckd.sw_fluxes_byband)
    assert list(sig.parameters) == ["self", "plev", "tlay", "gas_desc", "top_at_1", "mu0", "sfc_alb_dir", "sfc_alb_dif", "fluxes",
                                    "particles", "delta_scale", "toa_scale", "cloud_mask"]
    assert sig.parameters["delta_scale"].default is True
    assert all(sig.parameters[p].default is None for p in ("particles", "toa_scale", "cloud_mask"))
    assert list(inspect.signature(pkg.GasOpticsEcckd.lw_flux_bands_scratch_bytes).parameters) == ["self", "ncol", "nlay"]
    sig = inspect.signature(pkg.GasOpticsEcckd.sw_flux_bands_scratch_bytes)
    assert list(sig.parameters) == ["self", "ncol", "nlay", "delta_scale"] and sig.parameters["delta_scale"].default is True


def _host_model(pkg, path):
    k = pkg.GasOpticsEcckd()
    assert k.load(path, device=-1) == ""
    return k


class _Call:
    """One of the two entry points with valid host arguments for a model; ``run(name=value, ...)`` replaces arguments by
    name (an array, None or an int) and returns the message ('' = success).  Every array is checked untouched afterwards."""

    def __init__(self, pkg, k, longwave):
        self.pkg, self.k, self.longwave = pkg, k, longwave
        nb, ng = k.get_nband(), k.get_ngpt()
        f = lambda *shape, v=0.5: np.full(shape, v)
        a = dict(model=k._need(), ncol=NCOL, nlay=NLAY, plev=f(NLAY + 1, NCOL, v=1e4), tlay=f(NLAY, NCOL, v=250.))
        if longwave:
            a.update(tsfc=f(NCOL, v=250.), tlev=f(NLAY + 1, NCOL, v=250.))
        a.update(ngas=0, gas_names=None, vmr=None, col_stride=None, lay_stride=None, scalar=None, top_at_1=1)
        if longwave:
            a.update(n_gauss_angles=1, sfc_emis=f(NCOL, nb, v=0.98), inc_flux=None, nband_p=nb, tau_p=f(nb, NLAY, NCOL),
                     ssa_p=f(nb, NLAY, NCOL))
        else:
            a.update(mu0=f(NCOL), toa_scale=None, sfc_alb_dir=f(NCOL, nb, v=0.2), sfc_alb_dif=f(NCOL, nb, v=0.2), nband_p=nb,
                     tau_p=f(nb, NLAY, NCOL), ssa_p=f(nb, NLAY, NCOL), g_p=f(nb, NLAY, NCOL), delta_scale=1)
        a.update(cloud_mask=np.full((NLAY, NCOL), 5, dtype=np.uint64), bnd_flux_up=f(nb, NLAY + 1, NCOL, v=-7.),
                 bnd_flux_dn=f(nb, NLAY + 1, NCOL, v=-7.))
        if not longwave:
            a.update(bnd_flux_dir=f(nb, NLAY + 1, NCOL, v=-7.))
        a.update(flux_up=f(NLAY + 1, NCOL, v=-7.), flux_dn=f(NLAY + 1, NCOL, v=-7.))
        if not longwave:
            a.update(flux_dir=f(NLAY + 1, NCOL, v=-7.))
        a.update(memspace=pkg.HOST, stream=None)
        self.args = a
        self.copies = {n: v.copy() for n, v in a.items() if isinstance(v, np.ndarray)}
        self.fn = pkg.lib().ecckd_lw_flux_bands if longwave else pkg.lib().ecckd_sw_flux_bands
        assert len(a) == len(self.fn.argtypes)

    def run(self, **replace):
        a = dict(self.args)
        for n, v in replace.items():
            assert n in a, n
            a[n] = v
        rc = self.fn(*[C.c_void_p(v.ctypes.data) if isinstance(v, np.ndarray) else v for v in a.values()])
        for n, c in self.copies.items():
            assert np.array_equal(self.args[n], c), n + " was written"
        return self.pkg.last_error() if rc else ""


def _armed(call, **first):
    """The call with every later refusal of the documented list armed as well: the one named must be the earlier one."""
    late = dict(memspace=call.pkg.MIXED, bnd_flux_up=None, ncol=-1)
    late.update(first)
    return call.run(**late)


def test_longwave_refusals_in_documented_order(pkg):
    who = "ecckd_lw_flux_bands: "
    for path in (LW_RRTMGP, LW_FSCK):
        k = _host_model(pkg, path)
        c = _Call(pkg, k, True)
        nb = k.get_nband()
        m = c.run(model=None, nband_p=nb + 1)
        assert m == who + "null model"
        wide = _Call(pkg, _wide_model(pkg), True)
        m = _armed(wide, nband_p=7, tlev=None)
        assert m.startswith("ecckd_lw_flux_bands: a cloud mask is one 64-bit word") and m.endswith("not 65")
        pkg.set_arithmetic(pkg.REFERENCE_ORDER)
        try:   # (the arithmetic mode is armed as well up to its own place in the list)
            m = _armed(c, nband_p=nb + 1, tau_p=None)
            assert m.startswith(who + "nband_p = %d but the model has %d bands" % (nb + 1, nb))
            m = _armed(c, tau_p=None)
            assert m.startswith(who + "null argument (tau_p is required with nband_p > 0")
            for extra in (dict(), dict(tau_p=None, ssa_p=None), dict(tau_p=None, cloud_mask=None), dict(ssa_p=None, cloud_mask=None)):
                m = _armed(c, nband_p=0, **extra)
                assert m.startswith(who + "nband_p = 0 is the clear sky"), extra
            m = _armed(c, tlev=None, n_gauss_angles=0)
            assert m == who + "needs the fast arithmetic mode (ecckd_set_arithmetic(0))"
        finally:
            pkg.set_arithmetic(pkg.FAST)
        m = _armed(c, tlev=None, n_gauss_angles=0)
        assert m == who + "tlev is required for ecckd"
        for n in (0, 5):
            assert _armed(c, n_gauss_angles=n) == who + "have to ask for at least one quadrature point and no more than 4"
        a = c.args
        for gone in ("bnd_flux_up", "bnd_flux_dn"):
            m = c.run(memspace=pkg.MIXED, ncol=-1, flux_up=a["flux_dn"], **{gone: None})
            assert m.startswith(who + "null argument (bnd_flux_up and bnd_flux_dn are required)")
        for x, y in (("bnd_flux_dn", "bnd_flux_up"), ("flux_up", "bnd_flux_dn"), ("flux_dn", "flux_up")):
            m = c.run(memspace=pkg.MIXED, ncol=-1, **{x: a[y]})
            assert m.startswith(who + "two outputs are the same array"), (x, y)
        for space in (pkg.MIXED, 7, -1):
            assert c.run(memspace=space, ncol=-1).startswith(who + "bad memspace")
        # with valid arguments -- clear sky, one-stream and two-stream particles, masked, without the broadband members --
        # a host-only model fails loudly, and before it looks at the shape
        for extra in (dict(), dict(ncol=-1), dict(ssa_p=None), dict(cloud_mask=None), dict(flux_up=None, flux_dn=None),
                      dict(nband_p=0, tau_p=None, ssa_p=None, cloud_mask=None), dict(memspace=pkg.DEVICE)):
            m = c.run(**extra)
            assert m.startswith(who + "host-only model") and "no CPU fallback" in m, extra
    # a shortwave model is refused by name
    sw = _Call(pkg, _host_model(pkg, SW_WIDE), False)
    lw_on_sw = _Call(pkg, _host_model(pkg, SW_WIDE), True)
    assert _armed(lw_on_sw, tlev=None) == who + "model has no Planck table (shortwave model?)"
    assert sw.run().startswith("ecckd_sw_flux_bands: host-only model")


def test_shortwave_refusals_in_documented_order(pkg):
    who = "ecckd_sw_flux_bands: "
    k = _host_model(pkg, SW_WIDE)
    c = _Call(pkg, k, False)
    nb = k.get_nband()
    assert c.run(model=None, delta_scale=3) == who + "null model"
    # (the 65-g model has no solar table: the mask is named first)
    wide = _Call(pkg, _wide_model(pkg), False)
    m = _armed(wide, nband_p=7, delta_scale=3)
    assert m.startswith("ecckd_sw_flux_bands: a cloud mask is one 64-bit word") and m.endswith("not 65")
    pkg.set_arithmetic(pkg.REFERENCE_ORDER)
    try:
        m = _armed(c, nband_p=nb + 2, g_p=None, delta_scale=3)
        assert m.startswith(who + "nband_p = %d but the model has %d bands" % (nb + 2, nb))
        for gone in ("tau_p", "ssa_p", "g_p"):
            m = _armed(c, delta_scale=3, **{gone: None})
            assert m.startswith(who + "null argument (tau_p, ssa_p and g_p are all required with nband_p > 0)"), gone
        for extra in (dict(), dict(tau_p=None, ssa_p=None, g_p=None), dict(tau_p=None, ssa_p=None, cloud_mask=None)):
            m = _armed(c, nband_p=0, delta_scale=3, **extra)
            assert m.startswith(who + "nband_p = 0 is the clear sky"), extra
        for d in (2, -1):
            assert _armed(c, delta_scale=d) == who + "delta_scale must be 0 or 1"
        assert _armed(c) == who + "needs the fast arithmetic mode (ecckd_set_arithmetic(0))"
    finally:
        pkg.set_arithmetic(pkg.FAST)
    a = c.args
    for gone in ("bnd_flux_up", "bnd_flux_dn"):
        m = c.run(memspace=pkg.MIXED, ncol=-1, bnd_flux_dir=None, **{gone: None})
        assert m.startswith(who + "null argument (bnd_flux_up and bnd_flux_dn are required")
    assert c.run(memspace=pkg.MIXED, ncol=-1, bnd_flux_dir=None, flux_up=a["flux_dn"]) == who + "flux_dir needs bnd_flux_dir"
    for x, y in (("bnd_flux_dir", "bnd_flux_up"), ("flux_dir", "flux_dn"), ("flux_up", "bnd_flux_dir"), ("bnd_flux_dn", "bnd_flux_up")):
        m = c.run(memspace=pkg.MIXED, ncol=-1, **{x: a[y]})
        assert m.startswith(who + "two outputs are the same array"), (x, y)
    for space in (pkg.MIXED, 7):
        assert c.run(memspace=space, ncol=-1).startswith(who + "bad memspace")
    for extra in (dict(), dict(ncol=-1), dict(delta_scale=0), dict(cloud_mask=None), dict(bnd_flux_dir=None, flux_dir=None),
                  dict(flux_up=None, flux_dn=None, flux_dir=None), dict(nband_p=0, tau_p=None, ssa_p=None, g_p=None, cloud_mask=None),
                  dict(memspace=pkg.DEVICE)):
        m = c.run(**extra)
        assert m.startswith(who + "host-only model") and "no CPU fallback" in m, extra
    # a longwave model is refused by name
    for path in (LW_RRTMGP, LW_FSCK):
        sw_on_lw = _Call(pkg, _host_model(pkg, path), False)
        assert _armed(sw_on_lw) == who + "model has no solar table (longwave model?)"


def _align256(n):
    return (n + 255) // 256 * 256


def test_scratch_sizes_are_the_documented_ones(pkg):
    L = pkg.lib()
    for path in (LW_RRTMGP, LW_FSCK):
        k = _host_model(pkg, path)
        ng = k.get_ngpt()
        assert k.lw_flux_bands_scratch_bytes(0, 60) == 0 and k.lw_flux_bands_scratch_bytes(5, 0) == 0
        # 60 layers: what include/ecckd_hip.h documents for ecckd_lw_fluxes -- the optical depth alone
        assert k.lw_flux_bands_scratch_bytes(1000, 60) == (1000 * 60 * ng + 32) * 8
        # the general route: optical depth, three source arrays, surface source, the solver's ring
        for ncol, nlay in ((17, 61), (5, 137)):
            want = (4 * ncol * nlay * ng + ncol * ng + 64) * 8 + L.ecckd_rte_lw_scratch_bytes(ncol, nlay, ng)
            assert k.lw_flux_bands_scratch_bytes(ncol, nlay) == want, (ncol, nlay)
        assert L.ecckd_rte_lw_scratch_bytes(5, 137, ng) > 0
    assert L.ecckd_lw_flux_bands_scratch_bytes(None, 10, 60) == 0
    k = _host_model(pkg, SW_WIDE)
    ng, nb = k.get_ngpt(), k.get_nband()
    counts = [ng] + [int(hi - lo + 1) for lo, hi in k.get_band2gpt()]
    assert sum(counts[1:]) == ng
    dev = k.get_device()
    assert k.sw_flux_bands_scratch_bytes(0, 60) == 0 and L.ecckd_sw_flux_bands_scratch_bytes(None, 10, 60, 1) == 0

    def solver_term(ncol, nlay, n):   # the rule at ecckd_sw_fluxes
        tail = L.ecckd_rte_sw_tail_scratch_bytes(dev, ncol, nlay, n)
        return tail if nlay <= 60 else max(L.ecckd_rte_sw_scratch_bytes(ncol, nlay, n), tail)

    for ncol, nlay in ((1000, 60), (17, 61)):
        S = max(solver_term(ncol, nlay, n) for n in counts)
        for ds in (0, 1):
            want = _align256(ncol * nlay * ng * 8) + S + (3 * _align256(ncol * nlay * nb * 8) if ds else 0)
            assert k.sw_flux_bands_scratch_bytes(ncol, nlay, bool(ds)) == want, (ncol, nlay, ds)
    # at (1000, 60) that is the block of the broadband all-sky call: the term of the whole model is the largest
    assert solver_term(1000, 60, ng) == max(solver_term(1000, 60, n) for n in counts)
    assert solver_term(17, 61, ng) == max(solver_term(17, 61, n) for n in counts) > 0


def test_python_methods_answer_with_messages(pkg):
    """A FluxesBroadband, float32 arrays, a mixed-precision call and arrays of the wrong shape are answered with a message,
    not an exception, and never reach the library."""
    gc = pkg.GasConcs(["h2o"]); gc.set_vmr("h2o", 1e-3)
    plev, tlay, tsfc, tlev = (np.full((NLAY + 1, NCOL), 1e4), np.full((NLAY, NCOL), 250.), np.full(NCOL, 250.),
                              np.full((NLAY + 1, NCOL), 250.))
    k = _host_model(pkg, LW_RRTMGP)
    nb = k.get_nband()
    emis = np.full((NCOL, nb), 0.98)
    bnd = lambda dt=np.float64: np.full((nb, NLAY + 1, NCOL), -7., dtype=dt)
    bb = lambda dt=np.float64: np.full((NLAY + 1, NCOL), -7., dtype=dt)
    good = pkg.FluxesByband(bnd(), bnd(), flux_up=bb(), flux_dn=bb())
    call = lambda fl=good, tl=tlay, **kw: k.lw_fluxes_byband(plev, tl, tsfc, tlev, gc, True, emis, fl, **kw)
    m = call(pkg.FluxesBroadband(bb(), bb()))
    assert m.startswith("lw_fluxes_byband: fluxes must be a FluxesByband")
    f32 = [a.astype(np.float32) for a in (plev, tlay, tsfc, tlev, emis)]
    m = k.lw_fluxes_byband(f32[0], f32[1], f32[2], f32[3], gc, True, f32[4],
                           pkg.FluxesByband(bnd(np.float32), bnd(np.float32)))
    assert m == "lw_fluxes_byband: per-band output from the fused path is implemented for float64 arrays"
    m = call(pkg.FluxesByband(bnd(), bnd(np.float32)))
    assert m.startswith("lw_fluxes_byband: mixing float32 and float64 arrays in one call") and "bnd_flux_dn is float32" in m
    m = call(pkg.FluxesByband(bnd()[1:], bnd()))
    assert "bnd_flux_up" in m and "shape" in m
    m = call(pkg.FluxesByband(bnd(), bnd(), flux_up=bb()[1:]))
    assert "flux_up" in m and "shape" in m
    part = pkg.OpticalProps2str()
    assert part.alloc_2str_bands(NCOL, NLAY, k) == ""
    short = pkg.OpticalProps2str()
    short.tau, short.ssa, short.g = part.tau, part.ssa[:, 1:], part.g
    assert "particles.ssa" in call(particles=short)
    assert "uint64" in call(particles=part, cloud_mask=np.zeros((NLAY, NCOL), dtype=np.int64))
    # valid calls get as far as the library, which has no device to run them on
    for kw in (dict(), dict(particles=part), dict(particles=part, cloud_mask=np.zeros((NLAY, NCOL), dtype=np.uint64)),
               dict(n_gauss_angles=3, inc_flux=np.full((k.get_ngpt(), NCOL), 1.))):
        m = call(**kw)
        assert m.startswith("ecckd_lw_flux_bands: host-only model"), kw
    assert np.all(good.bnd_flux_up == -7.) and np.all(good.flux_dn == -7.)

    ks = _host_model(pkg, SW_WIDE)
    nbs = ks.get_nband()
    alb, mu0 = np.full((NCOL, nbs), 0.2), np.full(NCOL, 0.5)
    sbnd = lambda dt=np.float64: np.full((nbs, NLAY + 1, NCOL), -7., dtype=dt)
    sgood = pkg.FluxesByband(sbnd(), sbnd(), sbnd(), bb(), bb(), bb())
    scall = lambda fl=sgood, **kw: ks.sw_fluxes_byband(plev, tlay, gc, True, mu0, alb, alb, fl, **kw)
    assert scall(pkg.FluxesBroadband(bb(), bb(), bb())).startswith("sw_fluxes_byband: fluxes must be a FluxesByband")
    m = ks.sw_fluxes_byband(f32[0], f32[1], gc, True, mu0.astype(np.float32), alb.astype(np.float32), alb.astype(np.float32),
                            pkg.FluxesByband(sbnd(np.float32), sbnd(np.float32)))
    assert m == "sw_fluxes_byband: per-band output from the fused path is implemented for float64 arrays"
    m = scall(pkg.FluxesByband(sbnd(), sbnd(), sbnd(np.float32)))
    assert m.startswith("sw_fluxes_byband: mixing float32 and float64 arrays in one call") and "bnd_flux_dn_dir" in m
    assert "shape" in scall(pkg.FluxesByband(sbnd(), sbnd()[1:]))
    spart = pkg.OpticalProps2str()
    assert spart.alloc_2str_bands(NCOL, NLAY, ks) == ""
    assert scall(pkg.FluxesByband(sbnd(), sbnd(), None, bb(), bb(), bb())) == "ecckd_sw_flux_bands: flux_dir needs bnd_flux_dir"
    for kw in (dict(), dict(particles=spart), dict(particles=spart, delta_scale=False),
               dict(particles=spart, cloud_mask=np.zeros((NLAY, NCOL), dtype=np.uint64)), dict(toa_scale=np.full(NCOL, 1.))):
        assert scall(**kw).startswith("ecckd_sw_flux_bands: host-only model"), kw
    assert scall(pkg.FluxesByband(sbnd(), sbnd())).startswith("ecckd_sw_flux_bands: host-only model")


def test_band_window_kernels_are_in_the_code_object(pkg):
    """The band-window forms are kernels of their own; the kernels they stand next to keep their names and counts."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources
    ks = kernel_resources.kernels(pkg.LIB_PATH)
    bands = {n: k for n, k in ks.items() if "rte_lw_split_bands_kernel<" in n}
    assert len(bands) == 10, list(bands)   # (series form) x (clear, one- / two-stream particles, each masked or not)
    for n, k in bands.items():
        assert "rte_lw_split_bands_kernel<15, 4, 32, " in n and k["spill_vgpr"] == 0 and k["max_flat_wg"] == 512, (n, k)
    for name, count in (("rte_sw_sys_mcica_bands_kernel<", 4), ("rte_sw_mcica_bands_kernel<", 2), ("rte_lw_split_allsky_kernel<", 4),
                        ("rte_lw_split_mcica_kernel<", 4), ("rte_lw_split_kernel<", 14), ("rte_sw_sys_mcica_kernel<", 4)):
        assert len([n for n in ks if name in n]) == count, name
