"""GPU parity tests: the HIP path, called through the C ABI, against the CPU oracle on the same
seeded inputs.  Stated tolerances (north_star: fluxes within 1e-6 W m-2 in fp64):

  Planck sources (lay/lev/sfc)   bit-identical   (no transcendental on the path)
  tau, ssa                       relative 1e-12  (the only difference is device log() vs libm)
  broadband fluxes               absolute 1e-9 W m-2 (device exp(), g-point summation order)
"""
import numpy as np
import pytest

import helpers
from helpers import edge_columns, orography_ramp
from conftest import LW_FSCK, LW_RRTMGP, SW_WIDE
from rte_ecckd_amd import synthetic

pytestmark = pytest.mark.gpu
TAU_RTOL = 1e-12
FLUX_ATOL = 1e-9


@pytest.fixture(autouse=True, params=["fast", "reference_order"])
def arithmetic(request, pkg):
    """Every test runs in both arithmetic modes of the library (ecckd_set_arithmetic): the fused
    fast kernel (default) and the reference-expression-order kernels."""
    pkg.set_arithmetic(pkg.FAST if request.param == "fast" else pkg.REFERENCE_ORDER)
    yield request.param
    pkg.set_arithmetic(pkg.FAST)


@pytest.fixture(scope="module")
def lw(pkg, gpu, oracle_mod):
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=0) == ""
    return k, oracle_mod.CkdModel(LW_FSCK)


def check_lw(pkg, k, m, oracle_mod, cols, device, names=None, overrides=None):
    err, tau, lay, inc, dec, sfc = helpers.run_lw_gas_optics(pkg, k, cols, device, names, overrides)
    assert err == ""
    otau, olay, oinc, odec, osfc, oerr = oracle_mod.gas_optics_int(
        m, cols["plev"], cols["tlay"], cols["tsfc"], helpers.oracle_gas_items(cols, names, overrides), cols["tlev"])
    assert oerr == ""
    assert np.array_equal(lay, olay) and np.array_equal(inc, oinc) and np.array_equal(dec, odec)
    assert np.array_equal(sfc, osfc)
    assert helpers.max_rel(tau, otau) < TAU_RTOL
    assert np.array_equal(tau == 0, otau == 0)     # clamped cells are exactly zero on both sides
    return tau, lay, inc, dec, sfc, (otau, olay, oinc, odec, osfc)


@pytest.mark.parametrize("ncol", [1, 63, 64, 65, 513, 1500])
def test_lw_gas_optics_ragged_sizes(pkg, gpu, oracle_mod, lw, ncol):
    k, m = lw
    check_lw(pkg, k, m, oracle_mod, synthetic.columns(7, ncol, k.get_press_min()), gpu)


def test_lw_gas_optics_edge_branches(pkg, gpu, oracle_mod, lw):
    k, m = lw
    check_lw(pkg, k, m, oracle_mod, edge_columns(k.get_press_min()), gpu)


@pytest.mark.parametrize("ncol", [2048, 3000])
def test_lw_gas_optics_orography(pkg, gpu, oracle_mod, lw, ncol):
    k, m = lw
    check_lw(pkg, k, m, oracle_mod, orography_ramp(k.get_press_min(), ncol), gpu)
    rev = orography_ramp(k.get_press_min(), ncol)          # descending ramp, shuffled blocks of 64 columns
    perm = np.random.default_rng(ncol).permutation(ncol // 64 + 1)
    idx = np.concatenate([np.arange(b * 64, min((b + 1) * 64, ncol)) for b in perm])
    for key, v in rev.items():
        if isinstance(v, np.ndarray):
            rev[key] = np.ascontiguousarray(v[..., idx])
    check_lw(pkg, k, m, oracle_mod, rev, gpu)


def test_lw_gas_lists(pkg, gpu, oracle_mod, lw):
    """gas_desc order, unknown gases, composite-once, missing composite (src/gas_optics_ecckd.f90:348-374)."""
    k, m = lw
    cols = synthetic.columns(0, 70, k.get_press_min())
    base = check_lw(pkg, k, m, oracle_mod, cols, gpu)[0]
    rev = list(reversed(synthetic.GAS_ORDER))
    t_rev = check_lw(pkg, k, m, oracle_mod, cols, gpu, names=rev)[0]
    assert helpers.max_rel(t_rev, base) < 1e-13     # different summation order, same physics
    with_n2 = synthetic.GAS_ORDER + ["n2"]
    t_n2 = check_lw(pkg, k, m, oracle_mod, cols, gpu, names=with_n2, overrides={"n2": 0.78})[0]
    assert np.array_equal(t_n2, base)               # composite table counted once
    no_comp = [g for g in synthetic.GAS_ORDER if g != "o2"]
    t_nc = check_lw(pkg, k, m, oracle_mod, cols, gpu, names=no_comp)[0]
    assert np.all(t_nc <= base) and np.any(t_nc < base)
    only_unknown = check_lw(pkg, k, m, oracle_mod, cols, gpu, names=["no2", "xyz"], overrides={"xyz": 0.5})[0]
    assert np.all(only_unknown == 0)
    prof = {"co2": np.linspace(3e-4, 5e-4, 60)}     # a (nlay) profile, as ty_gas_concs allows
    check_lw(pkg, k, m, oracle_mod, cols, gpu, overrides=prof)


def test_host_and_device_memspace_agree(pkg, gpu, lw):
    k, _ = lw
    cols = synthetic.columns(3, 130, k.get_press_min())
    d = helpers.run_lw_gas_optics(pkg, k, cols, gpu)
    h = helpers.run_lw_gas_optics(pkg, k, cols, None)
    assert d[0] == h[0] == ""
    for a, b in zip(d[1:], h[1:]):
        assert np.array_equal(a, b)


def test_column_count_limit_is_an_error_not_a_fault(pkg, gpu, lw):
    """The gas-optics kernels address a g-plane pair with 32-bit byte offsets: a call whose
    ncol*(nlay+1) does not fit is refused before anything is read (no reference counterpart)."""
    import ctypes as C
    k, _ = lw
    d = np.zeros(8)
    p = d.ctypes.data_as(C.c_void_p)
    none = (C.c_void_p * 1)()
    z = (C.c_longlong * 1)(0)
    sc = (C.c_double * 1)(0.0)
    rc = pkg.lib().ecckd_gas_optics_lw(k._need(), 9_000_000, 60, p, p, p, p, 0, b"", none, z, z, sc, p, p, p, p, p,
                                       pkg.HOST, None)
    assert rc != 0 and "split the column range" in pkg.last_error()


def test_tlev_required_error_behaviour(pkg, gpu, oracle_mod, lw):
    """:414-417 -- tau, lay_source and sfc_source are produced, then the call fails."""
    k, m = lw
    cols = synthetic.columns(0, 40, k.get_press_min())
    err, tau, lay, inc, dec, sfc = helpers.run_lw_gas_optics(pkg, k, cols, gpu, tlev=False)
    assert err == "tlev is required for ecckd"
    ok = helpers.run_lw_gas_optics(pkg, k, cols, gpu)
    assert np.array_equal(tau, ok[1]) and np.array_equal(lay, ok[2]) and np.array_equal(sfc, ok[5])


def test_builder_route_equals_load_route(pkg, gpu, oracle_mod, lw):
    """ecckd_model_begin/_add_gas/_finalize (filling the type's members) == ecckd_model_load."""
    k, m = lw
    gases = [dict(name=n, code=t["code"], composite_only=int(t["composite_only"]), mole_fraction=t["mole_fraction"],
                  reference_mole_fraction=t["reference_mole_fraction"],
                  coefficient=t["coefficient"] if t["code"] == 2 else t["coefficient"][0])
             for n, t in zip(m.gas, m.tables)]
    k2 = pkg.GasOpticsEcckd()
    assert k2.init_from_tables(m.log_pressure, m.temperature, gases,
                               planck=(m.temperature_planck, m.planck_function)) == ""
    assert k2.get_gases() == k.get_gases() and k2.get_ngpt() == 32
    cols = synthetic.columns(11, 100, k.get_press_min())
    a = helpers.run_lw_gas_optics(pkg, k, cols, gpu)
    b = helpers.run_lw_gas_optics(pkg, k2, cols, gpu)
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)


def test_two_lut_gases_and_negative_tables(pkg, gpu, oracle_mod, lw):
    """A model with two look_up_table gases (second kernel pass, accumulate) and a table with
    negative coefficients (per-g clamp variant)."""
    k, m = lw
    rng = np.random.default_rng(5)
    tabs = []
    for n, t in zip(m.gas[:4], m.tables[:4]):
        tabs.append(dict(name=n, code=t["code"], composite_only=0, mole_fraction=t["mole_fraction"],
                         reference_mole_fraction=t["reference_mole_fraction"],
                         coefficient=t["coefficient"] if t["code"] == 2 else t["coefficient"][0]))
    h2o = m.tables[0]
    tabs.append(dict(name="h2o_b", code=2, composite_only=0, mole_fraction=h2o["mole_fraction"] * 0.5,
                     reference_mole_fraction=0.0, coefficient=h2o["coefficient"] * 0.25))
    neg = m.tables[2]["coefficient"][0] * rng.choice([1.0, -1.0], size=m.tables[2]["coefficient"][0].shape)
    tabs.append(dict(name="weird", code=1, composite_only=0, mole_fraction=None, reference_mole_fraction=0.0,
                     coefficient=neg))
    k2 = pkg.GasOpticsEcckd()
    assert k2.init_from_tables(m.log_pressure, m.temperature, tabs,
                               planck=(m.temperature_planck, m.planck_function)) == ""

    class M2:   # oracle-side twin of the same tables
        pass
    m2 = oracle_mod.CkdModel(LW_FSCK)
    m2.gas = [t["name"] for t in tabs]
    m2.tables = [dict(code=t["code"], composite_only=False, mole_fraction=None if t["mole_fraction"] is None else np.ascontiguousarray(t["mole_fraction"], dtype=np.float64),
                      reference_mole_fraction=t["reference_mole_fraction"],
                      coefficient=np.ascontiguousarray(t["coefficient"] if t["coefficient"].ndim == 4 else t["coefficient"][None]),
                      nv=t["coefficient"].shape[0] if t["coefficient"].ndim == 4 else 1) for t in tabs]
    m2.num_gases = len(tabs)
    cols = synthetic.columns(21, 200, k.get_press_min())
    names = ["co2", "h2o", "weird", "h2o_b", "o3", "ch4"]
    over = {"weird": 1e-4, "h2o_b": cols["h2o"] * 0.5}
    check_lw(pkg, k2, m2, oracle_mod, cols, gpu, names=names, overrides=over)
    # the second pass accumulates into tau: a segment walked once per slab position must not add twice
    wide = orography_ramp(k.get_press_min(), 1500, c0=21)
    check_lw(pkg, k2, m2, oracle_mod, wide, gpu, names=names, overrides={"weird": 1e-4, "h2o_b": wide["h2o"] * 0.5})


@pytest.mark.parametrize("nmus", [1, 2, 3, 4])
def test_rte_lw_vs_oracle(pkg, gpu, oracle_mod, lw, nmus):
    import torch
    k, m = lw
    cols = edge_columns(k.get_press_min(), 150)
    tau, lay, inc, dec, sfc, o = check_lw(pkg, k, m, oracle_mod, cols, gpu)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    op = pkg.OpticalProps1scl(); op.tau = t(tau); op.band2gpt = k.get_band2gpt()
    src = pkg.SourceFuncLW()
    src.lay_source, src.lev_source_inc, src.lev_source_dec, src.sfc_source = t(lay), t(inc), t(dec), t(sfc)
    ncol = tau.shape[2]
    fl = pkg.FluxesBroadband(torch.empty((61, ncol), dtype=torch.float64, device=gpu),
                             torch.empty((61, ncol), dtype=torch.float64, device=gpu))
    assert pkg.rte_lw(op, True, src, t(cols["sfc_emis"][:, None]), fl, n_gauss_angles=nmus) == ""
    fu, fd = oracle_mod.rte_lw(tau, lay, inc, dec, np.repeat(cols["sfc_emis"][None], 32, 0), sfc, nmus=nmus)
    ok = np.isfinite(fu)   # columns pushed outside the tables may overflow identically on both sides
    assert np.max(np.abs(fl.flux_up.cpu().numpy() - fu)[ok]) < FLUX_ATOL
    assert np.max(np.abs(fl.flux_dn.cpu().numpy() - fd)[ok]) < FLUX_ATOL
    assert np.all(fl.flux_dn.cpu().numpy()[0] == 0)
    assert pkg.rte_lw(op, True, src, t(cols["sfc_emis"][:, None]), fl, n_gauss_angles=5) != ""


@pytest.mark.parametrize("nlay,top_at_1", [(60, False), (5, True), (32, False), (33, True), (61, True), (64, False),
                                           (80, True), (91, False), (96, True), (97, True), (137, False), (200, True)])
def test_rte_lw_other_layer_counts_and_orientation(pkg, gpu, oracle_mod, nlay, top_at_1):
    """nlay != 60 takes the padded register-resident variants (<= 32, 48, 64, 80, 96 layers) or, beyond 96
    layers, the overflow variant (bottom 96 layers in registers, the rest through a scratch ring); top_at_1 = .false. walks the arrays backwards; 1-3 quadrature angles."""
    import torch
    rng = np.random.default_rng(nlay)
    nmus = 1 + nlay % 3
    ng, ncol = 7, 77
    tau = rng.uniform(0, 2, (ng, nlay, ncol)) * rng.choice([1e-9, 1e-3, 1.0], size=(ng, nlay, ncol))
    lay, inc, dec = (rng.uniform(1, 9, (ng, nlay, ncol)) for _ in range(3))
    sfc = rng.uniform(1, 9, (ng, ncol))
    emis = rng.uniform(0.7, 1.0, (ncol, 2))
    b2g = np.array([[1, 3], [4, 7]], dtype=np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    op = pkg.OpticalProps1scl(); op.tau = t(tau); op.band2gpt = b2g
    src = pkg.SourceFuncLW()
    src.lay_source, src.lev_source_inc, src.lev_source_dec, src.sfc_source = t(lay), t(inc), t(dec), t(sfc)
    fl = pkg.FluxesBroadband(torch.empty((nlay + 1, ncol), dtype=torch.float64, device=gpu),
                             torch.empty((nlay + 1, ncol), dtype=torch.float64, device=gpu))
    assert pkg.rte_lw(op, top_at_1, src, t(emis), fl, n_gauss_angles=nmus) == ""
    emis_gpt = np.stack([emis[:, 0]] * 3 + [emis[:, 1]] * 4)
    fu, fd = oracle_mod.rte_lw(tau, lay, inc, dec, emis_gpt, sfc, top_at_1=top_at_1, nmus=nmus)
    assert np.max(np.abs(fl.flux_up.cpu().numpy() - fu)) < FLUX_ATOL
    assert np.max(np.abs(fl.flux_dn.cpu().numpy() - fd)) < FLUX_ATOL
    # host memspace gives the same numbers
    fl2 = pkg.FluxesBroadband(np.empty((nlay + 1, ncol)), np.empty((nlay + 1, ncol)))
    op2 = pkg.OpticalProps1scl(); op2.tau = tau; op2.band2gpt = b2g
    s2 = pkg.SourceFuncLW(); s2.lay_source, s2.lev_source_inc, s2.lev_source_dec, s2.sfc_source = lay, inc, dec, sfc
    assert pkg.rte_lw(op2, top_at_1, s2, np.ascontiguousarray(emis), fl2, n_gauss_angles=nmus) == ""
    assert np.array_equal(fl2.flux_up, fl.flux_up.cpu().numpy())


@pytest.mark.parametrize("nlay,top_at_1,nmus", [(60, True, 1), (60, False, 3), (33, True, 2), (96, False, 1), (137, True, 1)])
def test_rte_lw_shared_levels_is_bit_identical(pkg, gpu, nlay, top_at_1, nmus):
    """ecckd_rte_lw_shared_levels (one value per level, read once) against ecckd_rte_lw on level sources that do
    hold one value per level -- lev_source_inc(:,l,:) == lev_source_dec(:,l+1,:), as ecckd's gas optics writes
    them (src/gas_optics_ecckd.f90:419-424): the same fluxes bit for bit, in every solver variant."""
    import torch
    rng = np.random.default_rng(1000 + nlay)
    ng, ncol = 6, 200
    tau = rng.uniform(0, 2, (ng, nlay, ncol)) * rng.choice([1e-9, 1e-3, 1.0], size=(ng, nlay, ncol))
    lay = rng.uniform(1, 9, (ng, nlay, ncol))
    lev = rng.uniform(1, 9, (ng, nlay + 1, ncol))
    inc, dec = np.ascontiguousarray(lev[:, 1:]), np.ascontiguousarray(lev[:, :-1])
    sfc = rng.uniform(1, 9, (ng, ncol))
    emis = rng.uniform(0.7, 1.0, (ncol, 1))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    op = pkg.OpticalProps1scl(); op.tau = t(tau); op.band2gpt = np.array([[1, ng]], dtype=np.int32)
    src = pkg.SourceFuncLW()
    src.lay_source, src.lev_source_inc, src.lev_source_dec, src.sfc_source = t(lay), t(inc), t(dec), t(sfc)
    out = []
    for shared in (False, True):
        fl = pkg.FluxesBroadband(torch.zeros((nlay + 1, ncol), dtype=torch.float64, device=gpu),
                                 torch.zeros((nlay + 1, ncol), dtype=torch.float64, device=gpu))
        assert pkg.rte_lw(op, top_at_1, src, t(emis), fl, n_gauss_angles=nmus, shared_levels=shared) == ""
        out.append((fl.flux_up.cpu().numpy(), fl.flux_dn.cpu().numpy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert np.all(out[0][0] > 0)


def test_gas_optics_marks_its_level_sources_as_shared(pkg, gpu, lw):
    import torch
    k, m = lw
    cols = synthetic.columns(9, 130, k.get_press_min())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    gc = helpers.product_gas_concs(pkg, cols, to=t)
    plev = t(cols["plev"])
    op = pkg.OpticalProps1scl(); op.alloc_1scl(130, 60, k, like=plev)
    src = pkg.SourceFuncLW(); src.alloc(130, 60, k, like=plev)
    assert not src.levels_shared
    assert k.gas_optics(None, plev, t(cols["tlay"]), t(cols["tsfc"]), gc, op, src, tlev=t(cols["tlev"])) == ""
    assert src.levels_shared
    assert torch.equal(src.lev_source_inc[:, :-1], src.lev_source_dec[:, 1:])       # the property itself
    fl = [pkg.FluxesBroadband(torch.zeros((61, 130), dtype=torch.float64, device=gpu),
                              torch.zeros((61, 130), dtype=torch.float64, device=gpu)) for _ in range(2)]
    emis = t(cols["sfc_emis"][:, None])
    assert pkg.rte_lw(op, True, src, emis, fl[0]) == ""
    assert pkg.rte_lw(op, True, src, emis, fl[1], shared_levels=src.levels_shared) == ""
    assert torch.equal(fl[0].flux_up, fl[1].flux_up) and torch.equal(fl[0].flux_dn, fl[1].flux_dn)


def test_fluxes_byband_lw_and_sw(pkg, gpu, oracle_mod):
    """ty_fluxes_byband (RTE-RRTMGP callers; the reference drivers use the broadband type): per-band fluxes
    equal the oracle run on each band's g-points alone, their sum equals the broadband call."""
    import torch
    rng = np.random.default_rng(77)
    ng, nlay, ncol = 11, 60, 150
    b2g = np.array([[1, 2], [3, 3], [4, 8], [9, 11]], dtype=np.int32)
    nband = b2g.shape[0]
    g2b = np.concatenate([[b] * (hi - lo + 1) for b, (lo, hi) in enumerate(b2g)])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=gpu)
    # ---- longwave ----
    tau = rng.uniform(0, 2, (ng, nlay, ncol))
    lay, inc, dec = (rng.uniform(1, 9, (ng, nlay, ncol)) for _ in range(3))
    sfc = rng.uniform(1, 9, (ng, ncol))
    emis = rng.uniform(0.7, 1.0, (ncol, nband))
    op = pkg.OpticalProps1scl(); op.tau = t(tau); op.band2gpt = b2g
    src = pkg.SourceFuncLW()
    src.lay_source, src.lev_source_inc, src.lev_source_dec, src.sfc_source = t(lay), t(inc), t(dec), t(sfc)
    bb = pkg.FluxesBroadband(z(nlay + 1, ncol), z(nlay + 1, ncol))
    assert pkg.rte_lw(op, True, src, t(emis), bb, n_gauss_angles=2) == ""
    fb = pkg.FluxesByband(z(nband, nlay + 1, ncol), z(nband, nlay + 1, ncol), flux_up=z(nlay + 1, ncol), flux_dn=z(nlay + 1, ncol))
    assert pkg.rte_lw(op, True, src, t(emis), fb, n_gauss_angles=2) == ""
    for b, (lo, hi) in enumerate(b2g):
        sl = slice(lo - 1, hi)
        fu, fd = oracle_mod.rte_lw(tau[sl], lay[sl], inc[sl], dec[sl], np.repeat(emis[None, :, b], hi - lo + 1, 0), sfc[sl], nmus=2)
        assert np.max(np.abs(fb.bnd_flux_up[b].cpu().numpy() - fu)) < FLUX_ATOL
        assert np.max(np.abs(fb.bnd_flux_dn[b].cpu().numpy() - fd)) < FLUX_ATOL
    assert torch.equal(fb.flux_up, fb.bnd_flux_up.sum(0)) or torch.allclose(fb.flux_up, fb.bnd_flux_up.sum(0), rtol=0, atol=1e-10)
    assert torch.allclose(fb.flux_up, bb.flux_up, rtol=0, atol=FLUX_ATOL) and torch.allclose(fb.flux_dn, bb.flux_dn, rtol=0, atol=FLUX_ATOL)
    # host arrays take the same route
    hb = pkg.FluxesByband(np.zeros((nband, nlay + 1, ncol)), np.zeros((nband, nlay + 1, ncol)), flux_up=np.zeros((nlay + 1, ncol)))
    oph = pkg.OpticalProps1scl(); oph.tau = tau; oph.band2gpt = b2g
    sh = pkg.SourceFuncLW(); sh.lay_source, sh.lev_source_inc, sh.lev_source_dec, sh.sfc_source = lay, inc, dec, sfc
    assert pkg.rte_lw(oph, True, sh, emis, hb, n_gauss_angles=2) == ""
    assert np.array_equal(hb.bnd_flux_up, fb.bnd_flux_up.cpu().numpy()) and np.allclose(hb.flux_up, fb.flux_up.cpu().numpy(), rtol=0, atol=1e-10)
    # ---- shortwave ----
    ssa = rng.uniform(0, 1, (ng, nlay, ncol)); gg = rng.uniform(-0.3, 0.8, (ng, nlay, ncol))
    mu0 = rng.uniform(0.1, 1.0, ncol); toa = rng.uniform(1, 50, (ng, ncol))
    adir = rng.uniform(0.05, 0.4, (ncol, nband)); adif = rng.uniform(0.05, 0.4, (ncol, nband))
    op2 = pkg.OpticalProps2str(); op2.tau, op2.ssa, op2.g, op2.band2gpt = t(tau), t(ssa), t(gg), b2g
    sb = pkg.FluxesBroadband(z(nlay + 1, ncol), z(nlay + 1, ncol), z(nlay + 1, ncol))
    assert pkg.rte_sw(op2, True, t(mu0), t(toa), t(adir), t(adif), sb) == ""
    fs = pkg.FluxesByband(z(nband, nlay + 1, ncol), z(nband, nlay + 1, ncol), z(nband, nlay + 1, ncol),
                          flux_up=z(nlay + 1, ncol), flux_dn=z(nlay + 1, ncol), flux_dn_dir=z(nlay + 1, ncol))
    assert pkg.rte_sw(op2, True, t(mu0), t(toa), t(adir), t(adif), fs) == ""
    for b, (lo, hi) in enumerate(b2g):
        sl = slice(lo - 1, hi)
        n = hi - lo + 1
        fu, fd, fdir = oracle_mod.rte_sw(tau[sl], ssa[sl], gg[sl], mu0, toa[sl], np.repeat(adir[None, :, b], n, 0),
                                         np.repeat(adif[None, :, b], n, 0))
        assert np.max(np.abs(fs.bnd_flux_up[b].cpu().numpy() - fu)) < FLUX_ATOL
        assert np.max(np.abs(fs.bnd_flux_dn[b].cpu().numpy() - fd)) < FLUX_ATOL
        assert np.max(np.abs(fs.bnd_flux_dn_dir[b].cpu().numpy() - fdir)) < FLUX_ATOL
    for got, want in ((fs.flux_up, sb.flux_up), (fs.flux_dn, sb.flux_dn), (fs.flux_dn_dir, sb.flux_dn_dir)):
        assert torch.allclose(got, want, rtol=0, atol=FLUX_ATOL)
    assert g2b.shape[0] == ng


def test_lw_36g_16band_model(pkg, gpu, oracle_mod):
    """The higher-g-point LW file present in the reference (rrtmgp-tol0.061: 36 g, 16 bands)."""
    import torch
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_RRTMGP, device=0) == ""
    m = oracle_mod.CkdModel(LW_RRTMGP)
    cols = synthetic.columns(5, 300, k.get_press_min())
    tau, lay, inc, dec, sfc, _ = check_lw(pkg, k, m, oracle_mod, cols, gpu)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    op = pkg.OpticalProps1scl(); op.tau = t(tau); op.band2gpt = k.get_band2gpt()
    src = pkg.SourceFuncLW()
    src.lay_source, src.lev_source_inc, src.lev_source_dec, src.sfc_source = t(lay), t(inc), t(dec), t(sfc)
    emis = np.random.default_rng(0).uniform(0.9, 1.0, (300, 16))
    fl = pkg.FluxesBroadband(torch.empty((61, 300), dtype=torch.float64, device=gpu),
                             torch.empty((61, 300), dtype=torch.float64, device=gpu))
    assert pkg.rte_lw(op, True, src, t(emis), fl) == ""
    emis_gpt = emis[:, m.gpt2band - 1].T
    fu, fd = oracle_mod.rte_lw(tau, lay, inc, dec, np.ascontiguousarray(emis_gpt), sfc)
    assert np.max(np.abs(fl.flux_up.cpu().numpy() - fu)) < FLUX_ATOL
    assert np.max(np.abs(fl.flux_dn.cpu().numpy() - fd)) < FLUX_ATOL


@pytest.mark.parametrize("window", ["16", "48"])
def test_planck_window_smaller_than_the_temperature_range(pkg, gpu, oracle_mod, lw, window, monkeypatch):
    """The fused kernel may stage only a window of the Planck table in LDS (it does for the 36-g file);
    ECCKD_PLANCK_WINDOW forces a small one on the 32-g model so that, with the 60 K + edge-case temperature
    spread of these columns, most waves take the out-of-window path.  Sources must stay bit-identical."""
    k, m = lw
    monkeypatch.setenv("ECCKD_PLANCK_WINDOW", window)
    check_lw(pkg, k, m, oracle_mod, synthetic.columns(11, 1500, k.get_press_min()), gpu)
    check_lw(pkg, k, m, oracle_mod, edge_columns(k.get_press_min()), gpu)
    cold_to_hot = synthetic.columns(3, 640, k.get_press_min())     # a ramp: every wave in a different window
    ramp = np.linspace(-60.0, 60.0, 640)[None, :]
    for f in ("tlev", "tlay"):
        cold_to_hot[f] = cold_to_hot[f] + ramp
    cold_to_hot["tsfc"] = cold_to_hot["tsfc"] + ramp[0]
    check_lw(pkg, k, m, oracle_mod, cold_to_hot, gpu)


def test_sw_gas_optics_and_rte_sw(pkg, gpu, oracle_mod):
    import torch
    k = pkg.GasOpticsEcckd()
    assert k.load(SW_WIDE, device=0) == ""
    m = oracle_mod.CkdModel(SW_WIDE)
    ncol, nlay, ng = 333, 60, 27
    cols = synthetic.columns(9, ncol, k.get_press_min(), shortwave=True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    names = ["co2", "ch4", "n2o", "o2", "h2o", "o3"]
    gc = helpers.product_gas_concs(pkg, cols, t, names)
    op = pkg.OpticalProps2str(); op.alloc_2str(ncol, nlay, k, like=t(np.zeros(1)))
    toa = torch.empty((ng, ncol), dtype=torch.float64, device=gpu)
    assert k.gas_optics(None, t(cols["plev"]), t(cols["tlay"]), gc, op, toa) == ""
    otau, ossa, og, otoa, oerr = oracle_mod.gas_optics_ext(m, cols["plev"], cols["tlay"],
                                                           helpers.oracle_gas_items(cols, names))
    assert oerr == ""
    assert helpers.max_rel(op.tau.cpu().numpy(), otau) < TAU_RTOL
    assert helpers.max_rel(op.ssa.cpu().numpy(), ossa) < TAU_RTOL
    assert np.all(op.g.cpu().numpy() == 0) and np.array_equal(toa.cpu().numpy(), otoa)
    # one-stream optical props -> the reference's error, after tau has been written (:457-464)
    op1 = pkg.OpticalProps1scl(); op1.alloc_1scl(ncol, nlay, k, like=t(np.zeros(1)))
    assert k.gas_optics(None, t(cols["plev"]), t(cols["tlay"]), gc, op1, toa) == "shortwave must use ty_optical_props_2str"
    assert np.array_equal(op1.tau.cpu().numpy(), op.tau.cpu().numpy())
    # solver on the oracle's optical properties (isolates the solver), 5 bands of albedo
    rng = np.random.default_rng(2)
    alb_dir = rng.uniform(0.05, 0.4, (ncol, 5)); alb_dif = rng.uniform(0.05, 0.4, (ncol, 5))
    op.tau, op.ssa, op.g = t(otau), t(ossa), t(og)
    fl = pkg.FluxesBroadband(*(torch.empty((nlay + 1, ncol), dtype=torch.float64, device=gpu) for _ in range(3)))
    assert pkg.rte_sw(op, True, t(cols["mu0"]), toa, t(alb_dir), t(alb_dif), fl) == ""
    g2b = m.gpt2band - 1
    fu, fd, fdir = oracle_mod.rte_sw(otau, ossa, og, cols["mu0"], otoa, np.ascontiguousarray(alb_dir[:, g2b].T),
                                     np.ascontiguousarray(alb_dif[:, g2b].T))
    assert np.max(np.abs(fl.flux_up.cpu().numpy() - fu)) < FLUX_ATOL
    assert np.max(np.abs(fl.flux_dn.cpu().numpy() - fd)) < FLUX_ATOL
    assert np.max(np.abs(fl.flux_dn_dir.cpu().numpy() - fdir)) < FLUX_ATOL
    # bottom-at-1 orientation
    f = lambda a: np.ascontiguousarray(a[:, ::-1, :])
    op.tau, op.ssa, op.g = t(f(otau)), t(f(ossa)), t(f(og))
    assert pkg.rte_sw(op, False, t(cols["mu0"]), toa, t(alb_dir), t(alb_dif), fl) == ""
    assert np.max(np.abs(fl.flux_up.cpu().numpy()[::-1] - fu)) < FLUX_ATOL


def test_sw_gas_optics_orography(pkg, gpu, oracle_mod):
    """Shortwave gas optics over columns whose surface pressure spans more pressure rows than the LDS slab
    holds (slab positions, masked stores of tau / ssa / g)."""
    import torch
    k = pkg.GasOpticsEcckd()
    assert k.load(SW_WIDE, device=0) == ""
    m = oracle_mod.CkdModel(SW_WIDE)
    ncol, nlay, ng = 1500, 60, 27
    cols = orography_ramp(k.get_press_min(), ncol, c0=3)
    cols["plev"][:, ::7] *= 0.8                      # every 7th column elsewhere: waves split between positions
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    names = ["co2", "ch4", "n2o", "o2", "h2o", "o3"]
    gc = helpers.product_gas_concs(pkg, cols, t, names)
    op = pkg.OpticalProps2str(); op.alloc_2str(ncol, nlay, k, like=t(np.zeros(1)))
    toa = torch.empty((ng, ncol), dtype=torch.float64, device=gpu)
    assert k.gas_optics(None, t(cols["plev"]), t(cols["tlay"]), gc, op, toa) == ""
    otau, ossa, og, otoa, oerr = oracle_mod.gas_optics_ext(m, cols["plev"], cols["tlay"],
                                                           helpers.oracle_gas_items(cols, names))
    assert oerr == ""
    assert helpers.max_rel(op.tau.cpu().numpy(), otau) < TAU_RTOL
    assert helpers.max_rel(op.ssa.cpu().numpy(), ossa) < TAU_RTOL
    assert np.all(op.g.cpu().numpy() == 0)


def test_modes_agree_to_a_few_ulp(pkg, gpu, lw):
    """fast vs reference-order arithmetic: same formula, re-associated."""
    k, _ = lw
    cols = edge_columns(k.get_press_min(), 256)
    pkg.set_arithmetic(pkg.REFERENCE_ORDER)
    r = helpers.run_lw_gas_optics(pkg, k, cols, gpu)
    pkg.set_arithmetic(pkg.FAST)
    f = helpers.run_lw_gas_optics(pkg, k, cols, gpu)
    assert helpers.max_rel(f[1], r[1]) < 5e-15
    for a, b in zip(f[2:], r[2:]):
        assert np.array_equal(a, b)          # Planck sources: identical in both modes


def test_single_precision_lw_path(pkg, gpu, oracle_mod, lw, arithmetic):
    """float32 arrays take ecckd_gas_optics_lw_f32 / ecckd_rte_lw_f32 (a host built with wp = real32).
    Checked against the fp64 oracle with single-precision tolerances (BASELINE configs[4]: fp32 vs fp64
    sweep): tau 2e-5 relative (where tau is not tiny), sources 2e-6 relative, fluxes 2e-3 W m-2."""
    import torch
    k, m = lw
    if arithmetic == "reference_order":
        pkg.set_arithmetic(pkg.FAST)          # the single-precision path exists in the fast mode only
    ncol, nlay, ng = 700, 60, 32
    cols = synthetic.columns(3, ncol, k.get_press_min())
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu)
    gc = pkg.GasConcs(synthetic.GAS_ORDER)
    for n in synthetic.GAS_ORDER:
        v = cols[n]
        if np.isscalar(v):
            gc.set_vmr(n, float(v))
        elif v.ndim == 1:
            gc.set_vmr_column(n, t32(v))
        else:
            gc.set_vmr(n, t32(v))
    plev, tlay, tlev, tsfc = t32(cols["plev"]), t32(cols["tlay"]), t32(cols["tlev"]), t32(cols["tsfc"])
    op = pkg.OpticalProps1scl(); op.alloc_1scl(ncol, nlay, k, like=plev)
    src = pkg.SourceFuncLW(); src.alloc(ncol, nlay, k, like=plev)
    assert op.tau.dtype == torch.float32
    assert k.gas_optics(None, plev, tlay, tsfc, gc, op, src, tlev=tlev) == ""
    fl = pkg.FluxesBroadband(torch.empty((nlay + 1, ncol), dtype=torch.float32, device=gpu),
                             torch.empty((nlay + 1, ncol), dtype=torch.float32, device=gpu))
    assert pkg.rte_lw(op, True, src, t32(cols["sfc_emis"][:, None]), fl) == ""
    # oracle on the float32-rounded inputs, in double
    r = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32), dtype=np.float64)
    c32 = {n: (r(v) if isinstance(v, np.ndarray) else v) for n, v in cols.items()}
    tau, lay, inc, dec, sfc, _ = oracle_mod.gas_optics_int(m, c32["plev"], c32["tlay"], c32["tsfc"],
                                                           helpers.oracle_gas_items(c32), c32["tlev"])
    fu, fd = oracle_mod.rte_lw(tau, lay, inc, dec, np.repeat(c32["sfc_emis"][None], ng, 0), sfc)
    gt = op.tau.cpu().numpy().astype(np.float64)
    big = tau > 1e-6 * tau.max()
    assert np.max(np.abs(gt - tau)[big] / tau[big]) < 2e-5
    assert helpers.max_rel(src.lay_source.cpu().numpy(), lay) < 2e-6
    assert helpers.max_rel(src.lev_source_inc.cpu().numpy(), inc) < 2e-6
    assert np.max(np.abs(fl.flux_up.cpu().numpy() - fu)) < 2e-3 and np.max(np.abs(fl.flux_dn.cpu().numpy() - fd)) < 2e-3
    # mixing precisions in one call is refused, not silently converted
    with pytest.raises(TypeError):
        k.gas_optics(None, plev, tlay.double(), tsfc, gc, op, src, tlev=tlev)


def test_calls_can_be_captured_in_a_hip_graph(pkg, gpu, lw, arithmetic):
    """ECCKD_DEVICE calls are plain asynchronous launches on the caller's stream (no allocation, no
    synchronisation after the first call of a shape), so a host model can capture gas_optics + rte_lw for a
    block of columns in a HIP graph, together with its own kernels, and replay it."""
    import torch
    k, m = lw
    ncol, nlay = 256, 60
    cols = synthetic.columns(90, ncol, k.get_press_min())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    gc = helpers.product_gas_concs(pkg, cols, to=t)
    plev, tlay, tlev, tsfc = t(cols["plev"]), t(cols["tlay"]), t(cols["tlev"]), t(cols["tsfc"])
    emis = t(cols["sfc_emis"][:, None])
    op = pkg.OpticalProps1scl(); op.alloc_1scl(ncol, nlay, k, like=plev)
    src = pkg.SourceFuncLW(); src.alloc(ncol, nlay, k, like=plev)
    fl = pkg.FluxesBroadband(torch.zeros((nlay + 1, ncol), dtype=torch.float64, device=gpu),
                             torch.zeros((nlay + 1, ncol), dtype=torch.float64, device=gpu))

    def step():
        assert k.gas_optics(None, plev, tlay, tsfc, gc, op, src, tlev=tlev) == ""
        assert pkg.rte_lw(op, True, src, emis, fl) == ""

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ref_up = fl.flux_up.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    # new inputs in the same buffers, results through a replay only
    cols2 = synthetic.columns(5000, ncol, k.get_press_min())
    plev.copy_(t(cols2["plev"])); tlay.copy_(t(cols2["tlay"])); tlev.copy_(t(cols2["tlev"])); tsfc.copy_(t(cols2["tsfc"]))
    fl.flux_up.zero_(); fl.flux_dn.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(fl.flux_up, ref_up)
    want_up = fl.flux_up.clone()
    fl.flux_up.zero_()
    step()                                      # the same inputs through direct calls
    torch.cuda.synchronize()
    assert torch.equal(fl.flux_up, want_up)


def test_golden_fixture_on_gpu(pkg, gpu, lw):
    """HIP path vs the committed golden vectors (tests/golden/lw_fsck_synth16.npz)."""
    import os
    import torch
    k, _ = lw
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "lw_fsck_synth16.npz"))
    cols = synthetic.columns(0, 16, k.get_press_min())
    err, tau, lay, inc, dec, sfc = helpers.run_lw_gas_optics(pkg, k, cols, gpu)
    assert err == ""
    assert np.array_equal(lay, z["lay_source"]) and np.array_equal(inc, z["lev_source_inc"])
    assert np.array_equal(sfc, z["sfc_source"])
    assert helpers.max_rel(tau, z["tau"]) < TAU_RTOL


def test_full_size_properties(pkg, gpu, oracle_mod, lw):
    """BASELINE config 2 size (1e5 columns x 60 x 32): oracle spot checks at both ends, column
    independence (a shuffled batch gives the shuffled answer, bit for bit), exact linearity of
    rte_lw in the sources, zero incident flux at the top, and determinism."""
    import torch
    k, m = lw
    ncol, nlay, ng = 100000, 60, 32
    cols = synthetic.columns(0, ncol, k.get_press_min())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    dcols = {n: (t(v) if isinstance(v, np.ndarray) else v) for n, v in cols.items()}

    def run(dc, scale=1.0):
        gc = pkg.GasConcs(synthetic.GAS_ORDER)
        for n in synthetic.GAS_ORDER:
            v = dc[n]
            if not torch.is_tensor(v):
                gc.set_vmr(n, float(v))
            elif v.ndim == 1:
                gc.set_vmr_column(n, v)
            else:
                gc.set_vmr(n, v)
        op = pkg.OpticalProps1scl(); op.alloc_1scl(ncol, nlay, k, like=dc["plev"])
        src = pkg.SourceFuncLW(); src.alloc(ncol, nlay, k, like=dc["plev"])
        assert k.gas_optics(None, dc["plev"], dc["tlay"], dc["tsfc"], gc, op, src, tlev=dc["tlev"]) == ""
        if scale != 1.0:
            for a in (src.lay_source, src.lev_source_inc, src.lev_source_dec, src.sfc_source):
                a.mul_(scale)
        fl = pkg.FluxesBroadband(torch.empty((nlay + 1, ncol), dtype=torch.float64, device=gpu),
                                 torch.empty((nlay + 1, ncol), dtype=torch.float64, device=gpu))
        assert pkg.rte_lw(op, True, src, dc["sfc_emis"].reshape(ncol, 1), fl) == ""
        torch.cuda.synchronize()
        return op, src, fl

    op, src, fl = run(dcols)
    for sl in (slice(0, 128), slice(ncol - 128, ncol)):
        sub = {n: (np.ascontiguousarray(v[..., sl]) if isinstance(v, np.ndarray) else v) for n, v in cols.items()}
        otau, olay, oinc, odec, osfc, _ = oracle_mod.gas_optics_int(m, sub["plev"], sub["tlay"], sub["tsfc"],
                                                                    synthetic.gas_items(sub), sub["tlev"])
        fu, fd = oracle_mod.rte_lw(otau, olay, oinc, odec, np.repeat(sub["sfc_emis"][None], ng, 0), osfc)
        assert helpers.max_rel(op.tau[..., sl].cpu().numpy(), otau) < TAU_RTOL
        assert np.array_equal(src.lev_source_inc[..., sl].cpu().numpy(), oinc)
        assert np.max(np.abs(fl.flux_up[:, sl].cpu().numpy() - fu)) < FLUX_ATOL
        assert np.max(np.abs(fl.flux_dn[:, sl].cpu().numpy() - fd)) < FLUX_ATOL
    assert bool(torch.all(fl.flux_dn[0] == 0))
    assert bool(torch.all(fl.flux_up > 0)) and bool(torch.all(torch.isfinite(fl.flux_up)))
    # determinism
    op2, src2, fl2 = run(dcols)
    assert torch.equal(fl2.flux_up, fl.flux_up) and torch.equal(op2.tau, op.tau)
    # column independence: permute the batch
    perm = torch.randperm(ncol, device=gpu, generator=torch.Generator(device=gpu).manual_seed(1))
    pc = {n: (v[..., perm].contiguous() if torch.is_tensor(v) else v) for n, v in dcols.items()}
    op3, src3, fl3 = run(pc)
    assert torch.equal(fl3.flux_up, fl.flux_up[:, perm]) and torch.equal(fl3.flux_dn, fl.flux_dn[:, perm])
    assert torch.equal(op3.tau, op.tau[..., perm])
    # linearity in the sources: x2 is exact in binary floating point
    _, _, fl4 = run(dcols, scale=2.0)
    assert torch.equal(fl4.flux_up, 2.0 * fl.flux_up) and torch.equal(fl4.flux_dn, 2.0 * fl.flux_dn)
