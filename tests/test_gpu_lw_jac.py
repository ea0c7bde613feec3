"""The longwave surface-temperature Jacobian on the GPU: ecckd_planck_sfc_source_jac, ecckd_rte_lw_jac and
ecckd_lw_fluxes_jac (include/ecckd_hip.h, "Longwave surface-temperature Jacobian").

The yardstick: the solver is linear in its sources, so flux_up_jac is the flux_up of the oracle's rte_lw with
lay_source = lev_source_inc = lev_source_dec = 0, no inc_flux and sfc_source = sfc_source_jac, on the optical depth the
flux pass saw (tests/test_lw_jac_host.py pins that run to the oracle's flux difference).  The bar is FLUX_ATOL = 1e-9
W m-2 K-1: the project's fp64 flux bar, applied to values a hundred times smaller than fluxes; the oracle's own two routes
differ by 5e-13 here.  Everything that the feature promises as an equality is checked as one: the surface term against the
oracle's sfc_source difference, the fluxes of every call against the call without the Jacobian, the Jacobian with against
without inc_flux, host arrays against device arrays, clear columns of a cloudy call against the clear-sky call, caller-owned
scratch and graph replay against the eager call.

Measured on an MI355X, next to the bars (which come from the issue, not from these figures): every equality held; rte_lw
Jacobian against the oracle 1.8e-15 ... 8.9e-15 W m-2 K-1 over the six shapes, fused calls 8.9e-16 ... 6.2e-15 over the 36
cases (bar 1e-9); the two "lw_jac_inline" routes at 60 layers differ by at most 8.0e-15 (same bar);
smallest cloud signal in the Jacobian 0.14 W m-2 K-1 (the bar times 20 is 2e-8); lw_fluxes(tsfc + 1) - lw_fluxes(tsfc) against
flux_up_jac 2.2e-13 ... 5.3e-13 (bar 1e-8)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import allsky_helpers as ah
import helpers
import mcica_helpers as mh
from helpers import FLUX_ATOL
from rte_ecckd_amd import synthetic
from test_gpu_lw_allsky import T, back, block_gas_concs, case, driver, particles, read_output, write_input, write_particles

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def default_options(pkg):
    pkg.reset_solver_options()
    pkg.set_arithmetic(pkg.FAST)
    inline = pkg.get_solver_option("lw_jac_inline")
    yield
    pkg.reset_solver_options()
    pkg.set_arithmetic(pkg.FAST)
    pkg.set_solver_option("lw_jac_inline", inline)


def inline_forms(nlay):
    """Values of "lw_jac_inline" that take different routes at this layer count: both at 60 layers."""
    return (0, 1) if nlay == 60 else (0,)


@pytest.fixture(scope="module")
def lw(pkg, gpu, oracle_mod):
    from conftest import LW_FSCK, LW_RRTMGP
    out = {}
    for name, path in (("fsck", LW_FSCK), ("rrtmgp", LW_RRTMGP)):
        k = pkg.GasOpticsEcckd()
        assert k.load(path, device=0) == ""
        out[name] = (k, oracle_mod.CkdModel(path), path)
    return out


def oracle_sfc_source(oracle_mod, m, tsfc):
    """sfc_source (ng, ncol) of the oracle's gas_optics_int: it depends on tsfc and the Planck table alone, so one dummy
    layer serves."""
    n = tsfc.shape[0]
    out = oracle_mod.gas_optics_int(m, np.repeat(np.array([[5e4], [6e4]]), n, 1), np.full((1, n), 250.0), tsfc,
                                    [("h2o", np.array([1e-3]), 0, 0)], np.full((2, n), 250.0))
    assert out[5] == ""
    return out[4]


def oracle_sfc_jac(oracle_mod, m, tsfc):
    return oracle_sfc_source(oracle_mod, m, tsfc + 1.0) - oracle_sfc_source(oracle_mod, m, tsfc)


def oracle_jac(oracle_mod, tau, emis_gpt, sfc_jac, top_at_1=True, nmus=1):
    zero = np.zeros_like(tau)
    up, dn = oracle_mod.rte_lw(tau, zero, zero, zero, emis_gpt, sfc_jac, top_at_1=top_at_1, nmus=nmus)
    assert np.all(dn == 0.0)
    return up


# ------------------------------------------------------------------------------------------------
# 1. the surface term
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["fsck", "rrtmgp"])
def test_sfc_source_jac_bit_for_bit(pkg, gpu, oracle_mod, lw, which):
    """sfc_source_jac = oracle sfc_source(tsfc + 1) - oracle sfc_source(tsfc), bit for bit, on the branch columns (tsfc
    below 120 K, at 120 K, at 350 K and above it among them): device and host arrays, and a single column."""
    k, m, _ = lw[which]
    tsfc = helpers.branch_columns(m)["tsfc"]
    assert tsfc.shape == (20,) and tsfc.min() < 120.0 and tsfc.max() > 350.0 and (tsfc == 120.0).any() and (tsfc == 350.0).any()
    want = oracle_sfc_jac(oracle_mod, m, tsfc)
    assert np.all(np.isfinite(want)) and np.all(want > 0.0)
    for to in (T(gpu), np.ascontiguousarray):
        src = pkg.SourceFuncLW()
        src.alloc(20, 60, k, like=to(np.zeros(1)))
        src.sfc_source_jac = to(np.full((k.get_ngpt(), 20), -1.0))
        assert k.planck_sfc_source_jac(to(tsfc), src) == ""
        assert np.array_equal(back(src.sfc_source_jac), want)
        for c in (0, 7, 9):
            one = pkg.SourceFuncLW()
            one.alloc(1, 60, k, like=to(np.zeros(1)))
            assert k.planck_sfc_source_jac(to(tsfc[c:c + 1]), one) == ""
            assert np.array_equal(back(one.sfc_source_jac), want[:, c:c + 1])


# ------------------------------------------------------------------------------------------------
# 2. rte_lw(flux_up_jac=)
# ------------------------------------------------------------------------------------------------
def solver_case(ncol, nlay, ng, seed):
    rng = np.random.default_rng(seed)
    nb = 3
    edges = [0, ng // 3, (2 * ng) // 3, ng]
    b2g = np.array([[edges[b] + 1, edges[b + 1]] for b in range(nb)], dtype=np.int32)
    g2b = np.repeat(np.arange(nb), np.diff(edges))
    c = dict(tau=10.0 ** rng.uniform(-4, 1, (ng, nlay, ncol)), lay=rng.uniform(10, 100, (ng, nlay, ncol)),
             inc=rng.uniform(10, 100, (ng, nlay, ncol)), dec=rng.uniform(10, 100, (ng, nlay, ncol)),
             sfc=rng.uniform(10, 100, (ng, ncol)), sfc_jac=rng.uniform(0.01, 0.2, (ng, ncol)),
             emis=rng.uniform(0.9, 1.0, (ncol, nb)), inc_flux=rng.uniform(0.0, 2.0, (ng, ncol)), b2g=b2g)
    c["emis_gpt"] = np.ascontiguousarray(c["emis"][:, g2b].T)
    return c


def run_rte_lw(pkg, c, to, top_at_1, nmus, inc, with_jac):
    ng, nlay, ncol = c["tau"].shape
    op = pkg.OpticalProps1scl()
    op.tau, op.band2gpt = to(c["tau"]), c["b2g"]
    src = pkg.SourceFuncLW()
    src.lay_source, src.lev_source_inc, src.lev_source_dec = to(c["lay"]), to(c["inc"]), to(c["dec"])
    src.sfc_source, src.sfc_source_jac = to(c["sfc"]), to(c["sfc_jac"])
    fl = pkg.FluxesBroadband(to(np.full((nlay + 1, ncol), -1.0)), to(np.full((nlay + 1, ncol), -1.0)))
    jac = to(np.full((nlay + 1, ncol), -1.0)) if with_jac else None
    assert pkg.rte_lw(op, top_at_1, src, to(c["emis"]), fl, n_gauss_angles=nmus, inc_flux=to(c["inc_flux"]) if inc else None,
                      flux_up_jac=jac) == ""
    return back(fl.flux_up), back(fl.flux_dn), None if jac is None else back(jac)


@pytest.mark.parametrize("ncol,nlay,ng", [(1, 60, 32), (33, 60, 33), (130, 60, 36), (333, 37, 33), (65, 137, 32), (33, 1, 33)])
def test_rte_lw_with_jacobian(pkg, gpu, oracle_mod, ncol, nlay, ng):
    """1 and 3 angles, both orientations, with and without inc_flux: the fluxes are those of the call without the Jacobian,
    the Jacobian is within FLUX_ATOL of the oracle's zero-source run on the same tau and does not change with inc_flux.
    (33 g-points: the last wave lane carries weight 0.)"""
    c = solver_case(ncol, nlay, ng, 100 * ncol + nlay)
    t = T(gpu)
    worst = 0.0
    for top_at_1 in (True, False):
        for nmus in (1, 3):
            want = oracle_jac(oracle_mod, c["tau"], c["emis_gpt"], c["sfc_jac"], top_at_1, nmus)
            jacs = []
            for inc in (False, True):
                up, dn, jac = run_rte_lw(pkg, c, t, top_at_1, nmus, inc, True)
                up0, dn0, _ = run_rte_lw(pkg, c, t, top_at_1, nmus, inc, False)
                assert np.array_equal(up, up0) and np.array_equal(dn, dn0), (top_at_1, nmus, inc)
                assert np.all(np.isfinite(jac))
                worst = max(worst, float(np.max(np.abs(jac - want))))
                jacs.append(jac)
            assert np.array_equal(jacs[0], jacs[1])
    print("rte_lw jacobian %d x %d x %d g: %.2e W m-2 K-1 from the oracle (bar %.0e)" % (ncol, nlay, ng, worst, FLUX_ATOL))
    assert worst < FLUX_ATOL


def test_rte_lw_jacobian_host_arrays_and_extremes(pkg, gpu, oracle_mod):
    """Host arrays give the bits of device arrays.  A layer of tau = inf in every g-point gives exactly 0 above it (and
    the untouched value below); tau = 0 everywhere gives the surface value at every level."""
    t = T(gpu)
    for ncol, nlay, top_at_1 in ((130, 60, True), (65, 137, False), (33, 37, True)):
        c = solver_case(ncol, nlay, 33, ncol)
        d = run_rte_lw(pkg, c, t, top_at_1, 3, True, True)
        h = run_rte_lw(pkg, c, np.ascontiguousarray, top_at_1, 3, True, True)
        for a, b in zip(d, h):
            assert np.array_equal(a, b), (ncol, nlay)
        lay = nlay // 2                                     # array index of the opaque layer
        opaque = dict(c, tau=c["tau"].copy())
        opaque["tau"][:, lay, :] = np.inf
        jac = run_rte_lw(pkg, opaque, t, top_at_1, 3, False, True)[2]
        above = slice(0, lay + 1) if top_at_1 else slice(lay + 1, None)   # levels on the far side of the layer from the surface
        below = slice(lay + 1, None) if top_at_1 else slice(0, lay + 1)
        assert np.all(jac[above] == 0.0) and np.array_equal(jac[below], d[2][below]) and np.all(jac[below] > 0.0)
        clear = dict(c, tau=np.zeros_like(c["tau"]))
        jac = run_rte_lw(pkg, clear, t, top_at_1, 1, False, True)[2]
        sfc = jac[-1] if top_at_1 else jac[0]
        assert np.all(jac == sfc[None, :]) and np.all(sfc > 0.0)


# ------------------------------------------------------------------------------------------------
# 3. the fused calls
# ------------------------------------------------------------------------------------------------
def fused_call(pkg, k, cols, to, top_at_1=True, nmus=1, inc=False, cloud=None, one_stream=False, mask=None, both=False,
               with_jac=True, tsfc=None):
    """lw_fluxes / lw_fluxes_allsky / lw_fluxes_clear_allsky with (or without) flux_up_jac.  Returns the flux arrays of the
    call (up, dn[, up_clear, dn_clear]) and the Jacobian (or None)."""
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to)
    new = lambda: to(np.full((nlay + 1, ncol), -1.0))
    fl = pkg.FluxesBroadband(new(), new())
    jac = new() if with_jac else None
    args = (to(cols["plev"]), to(cols["tlay"]), to(cols["tsfc"] if tsfc is None else tsfc), to(cols["tlev"]), gc, top_at_1,
            to(cols["emis"]))
    kw = dict(n_gauss_angles=nmus, inc_flux=to(cols["inc_flux"]) if inc else None, flux_up_jac=jac)
    outs = [fl]
    if cloud is None:
        assert k.lw_fluxes(*args, fl, **kw) == ""
    else:
        part = particles(pkg, cloud, to, one_stream)
        if mask is not None:
            import torch
            kw["cloud_mask"] = mask if to is np.ascontiguousarray else torch.from_numpy(mask.view(np.int64)).to(fl.flux_up.device)
        if both:
            fc = pkg.FluxesBroadband(new(), new())
            outs.append(fc)
            if with_jac:
                assert k.lw_fluxes_clear_allsky_jac(*args, part, fl, fc, kw.pop("flux_up_jac"), **kw) == ""
            else:
                assert k.lw_fluxes_clear_allsky(*args, part, fl, fc, **{n: v for n, v in kw.items() if n != "flux_up_jac"}) == ""
        else:
            assert k.lw_fluxes_allsky(*args, part, fl, **kw) == ""
    fluxes = [back(a) for f in outs for a in (f.flux_up, f.flux_dn)]
    return fluxes, None if jac is None else back(jac)


def incremented(tau, m, cloud, one_stream, mask):
    """The oracle's gas optical depth incremented in numpy by the (masked) particles, as the flux pass increments it."""
    if cloud is None:
        return tau
    ptau = cloud["tau"]
    if mask is None:
        op2 = (ptau,) if one_stream else (ptau, cloud["ssa"], cloud["g"])
        return ah.increment((tau,), op2, m.band2gpt)[0]
    mt = mh.masked_tau(ptau, mask, m.band2gpt, m.ng)
    op2 = (mt,) if one_stream else (mt, ah.spread(cloud["ssa"], m.band2gpt, m.ng), ah.spread(cloud["g"], m.band2gpt, m.ng))
    return ah.increment((tau,), op2)[0]


VARIANTS = (("clear", dict()), ("two-stream", dict(cloudy=True)), ("one-stream", dict(cloudy=True, one_stream=True)),
            ("two-stream mask", dict(cloudy=True, masked=True)), ("one-stream mask", dict(cloudy=True, one_stream=True, masked=True)),
            ("both skies", dict(cloudy=True, both=True)), ("both skies mask", dict(cloudy=True, both=True, masked=True)))


@pytest.mark.parametrize("ncol", [1, 33, 65, 130, 333, 777])
@pytest.mark.parametrize("nlay", [60, 37, 137])
@pytest.mark.parametrize("which", ["fsck", "rrtmgp"])
def test_fused_calls_with_jacobian(pkg, gpu, oracle_mod, lw, which, nlay, ncol):
    """lw_fluxes, lw_fluxes_allsky (one- and two-stream particles, with and without a McICA mask) and lw_fluxes_clear_allsky
    with flux_up_jac, 1 and 3 angles, both orientations at 60 and 137 layers, both values of "lw_jac_inline" at 60 layers:
    every flux array equals the existing call's, the Jacobian is within FLUX_ATOL of the oracle's zero-source run on the
    numpy-incremented optical depth, the two "lw_jac_inline" routes agree within FLUX_ATOL, the clear columns of a cloudy
    call hold the clear-sky call's Jacobian bit for bit, and the clouds show: the smallest Jacobian change over the cloudy
    columns is at least 20 bars."""
    k, m, _ = lw[which]
    t = T(gpu)
    cols, cloud = case(k, 7 * ncol + nlay, ncol, nlay)
    items = helpers.oracle_gas_items(cols)
    tau = oracle_mod.gas_optics_int(m, cols["plev"], cols["tlay"], cols["tsfc"], items, cols["tlev"])[0]
    sfc_jac = oracle_sfc_jac(oracle_mod, m, cols["tsfc"])
    emis_gpt = np.repeat(cols["sfc_emis"][None, :], m.ng, 0)
    mask = mh.sample(synthetic.cloud_fraction(7 * ncol + nlay, ncol, nlay), m.ng, mh.MAX_RAN, None, 5, 0)
    cloudy = cloud["cloudy"]
    worst, routes, signal = 0.0, 0.0, np.inf
    for top_at_1 in ((True, False) if nlay in (60, 137) else (True,)):
        for nmus in (1, 3):
            clear_jac, wants = {}, {}   # (both skies: the all-sky Jacobian, on the optical depth of the single all-sky call)
            for name, v in VARIANTS:
                kw = dict(top_at_1=top_at_1, nmus=nmus, inc=nmus == 3, cloud=cloud if v.get("cloudy") else None,
                          one_stream=v.get("one_stream", False), mask=mask if v.get("masked") else None, both=v.get("both", False))
                plain, _ = fused_call(pkg, k, cols, t, with_jac=False, **kw)
                sky = (v.get("cloudy", False), kw["one_stream"], v.get("masked", False))
                if sky not in wants:
                    wants[sky] = oracle_jac(oracle_mod, incremented(tau, m, kw["cloud"], kw["one_stream"], kw["mask"]), emis_gpt,
                                            sfc_jac, top_at_1, nmus)
                want = wants[sky]
                by_route = []
                for inline in inline_forms(nlay):
                    pkg.set_solver_option("lw_jac_inline", inline)
                    fluxes, jac = fused_call(pkg, k, cols, t, **kw)
                    what = (which, ncol, nlay, top_at_1, nmus, name, inline)
                    for a, b in zip(fluxes, plain):
                        assert np.array_equal(a, b), what
                    assert np.all(np.isfinite(jac)), what
                    worst = max(worst, float(np.max(np.abs(jac - want))))
                    if name == "clear":
                        clear_jac[inline] = jac
                    else:
                        assert np.array_equal(jac[:, ~cloudy], clear_jac[inline][:, ~cloudy]), what
                    by_route.append(jac)
                if len(by_route) == 2:
                    routes = max(routes, float(np.max(np.abs(by_route[0] - by_route[1]))))
                if name == "clear":
                    clear_want = want
                elif cloudy.any() and not v.get("masked"):
                    signal = min(signal, ah.smallest_cloud_signal([want], [clear_want], cloudy))
    print("fused jacobian %s %d x %d: %.2e W m-2 K-1 from the oracle, %.2e between the lw_jac_inline routes (bar %.0e); "
          "smallest cloud signal %.2e" % (which, ncol, nlay, worst, routes, FLUX_ATOL, signal))
    assert worst < FLUX_ATOL and routes < FLUX_ATOL
    assert signal >= 20 * FLUX_ATOL


# ------------------------------------------------------------------------------------------------
# 4. the product alone: the Jacobian is the flux difference of two calls
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,ncol,nlay", [("fsck", 130, 60), ("rrtmgp", 65, 60), ("fsck", 65, 37), ("rrtmgp", 130, 37)])
def test_jacobian_is_the_flux_difference(pkg, gpu, lw, which, ncol, nlay):
    """lw_fluxes at tsfc + 1 minus at tsfc equals flux_up_jac within 10 FLUX_ATOL (two fluxes of some 400 W m-2 against one
    value of some 5), and flux_dn is the same bits at both temperatures: clear and all-sky."""
    k = lw[which][0]
    t = T(gpu)
    cols, cloud = case(k, 3 * ncol + nlay, ncol, nlay)
    for inline in inline_forms(nlay):
        pkg.set_solver_option("lw_jac_inline", inline)
        for cl in (None, cloud):
            for nmus in (1, 3):
                f0, jac = fused_call(pkg, k, cols, t, nmus=nmus, cloud=cl)
                f1, _ = fused_call(pkg, k, cols, t, nmus=nmus, cloud=cl, with_jac=False, tsfc=cols["tsfc"] + 1.0)
                err = float(np.max(np.abs((f1[0] - f0[0]) - jac)))
                print("flux difference %s %d x %d %s %d angles, lw_jac_inline %d: %.2e W m-2 K-1 (bar %.0e)" %
                      (which, ncol, nlay, "clear" if cl is None else "all-sky", nmus, inline, err, 10 * FLUX_ATOL))
                assert err < 10 * FLUX_ATOL and np.array_equal(f0[1], f1[1])


# ------------------------------------------------------------------------------------------------
# 5./6. containment, host arrays
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,ncol,nlay", [("fsck", 130, 60), ("rrtmgp", 65, 37), ("fsck", 65, 137)])
def test_nan_tsfc_stays_in_its_column_and_host_equals_device(pkg, gpu, lw, which, ncol, nlay):
    k = lw[which][0]
    t = T(gpu)
    cols, cloud = case(k, 19, ncol, nlay)
    mask = mh.sample(synthetic.cloud_fraction(19, ncol, nlay), k.get_ngpt(), mh.MAX_RAN, None, 5, 0)
    for inline in inline_forms(nlay):
        pkg.set_solver_option("lw_jac_inline", inline)
        for kw in (dict(), dict(cloud=cloud), dict(cloud=cloud, one_stream=True, mask=mask),
                   dict(cloud=cloud, both=True, nmus=3, inc=True)):
            fd, jd = fused_call(pkg, k, cols, t, **kw)
            fh, jh = fused_call(pkg, k, cols, np.ascontiguousarray, **kw)
            assert np.array_equal(jd, jh) and all(np.array_equal(a, b) for a, b in zip(fd, fh)), (kw, inline)
            bad = cols["tsfc"].copy()
            hit = ncol // 2
            bad[hit] = np.nan
            _, jn = fused_call(pkg, k, cols, t, tsfc=bad, **kw)
            keep = np.arange(ncol) != hit
            assert np.all(np.isnan(jn[:, hit])) and np.array_equal(jn[:, keep], jd[:, keep]), (kw, inline)


# ------------------------------------------------------------------------------------------------
# the rest of the refusal order of the clear-sky form, which a host-only model cannot answer
# ------------------------------------------------------------------------------------------------
def test_clear_form_refusals_on_a_device_model(pkg, gpu, lw):
    k = lw["fsck"][0]
    ncol, nlay = 4, 60
    cols, _ = case(k, 1, ncol, nlay)
    names = b"".join(n.encode().ljust(32, b" ") for n in ("h2o",))
    outs = [np.full((nlay + 1, ncol), -7.0) for _ in range(5)]
    up, dn, upc, dnc, jac = outs
    cols = {n: np.ascontiguousarray(v) for n, v in cols.items() if isinstance(v, np.ndarray)}
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    vmr = (C.c_void_p * 1)(None)
    z, sc = (C.c_longlong * 1)(0), (C.c_double * 1)(1e-3)
    mask = np.zeros((nlay, ncol), dtype=np.uint64)

    def raw(tlev=cols["tlev"], nband_p=0, ssa=None, mask_=None, upc_=None, dnc_=None, j=jac):
        rc = pkg.lib().ecckd_lw_fluxes_jac(k._need(), ncol, nlay, P(cols["plev"]), P(cols["tlay"]), P(cols["tsfc"]), P(tlev), 1, names,
                                           vmr, z, z, sc, 1, 1, P(cols["emis"]), None, nband_p, None, P(ssa), P(mask_), P(up), P(dn),
                                           P(upc_), P(dnc_), P(j), pkg.HOST, None)
        return pkg.last_error() if rc else ""
    untouched = lambda: all(np.all(a == -7.0) for a in outs)
    assert raw(tlev=None, j=up, upc_=upc) == "tlev is required for ecckd" and untouched()           # the existing call's list first
    assert "must not be another output" in raw(j=up, upc_=upc) and untouched()                        # then the alias
    assert "must not be another output" in raw(j=dn, mask_=mask) and untouched()
    for kw in (dict(upc_=upc, dnc_=dnc), dict(dnc_=dnc), dict(mask_=mask), dict(nband_p=k.get_nband()), dict(ssa=np.zeros(4)),
               dict(upc_=upc, j=None)):
        assert "without tau_p" in raw(**kw) and untouched(), kw                                          # then particles' arguments alone
    assert raw() == "" and not untouched()


# ------------------------------------------------------------------------------------------------
# 7./8. caller-owned scratch, graph capture
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,ncol,nlay,inline", [("fsck", 1000, 60, 0), ("rrtmgp", 1000, 60, 1), ("rrtmgp", 333, 37, 0)])
def test_caller_owned_scratch_and_capture(pkg, gpu, lw, which, ncol, nlay, inline):
    """The call with flux_up_jac runs on a caller-owned block of exactly the size documented for the existing call -- 60
    layers: (ncol*nlay*ngpt + 32)*8 bytes; general route: (4*ncol*nlay*ngpt + ncol*ngpt + 64)*8 +
    ecckd_rte_lw_scratch_bytes -- filled with 0xFF bytes, and gives the eager bits; a capture on one stream after a warm-up
    call replays to the eager bits, twice."""
    import torch
    t = T(gpu)
    k = lw[which][0]
    ng = k.get_ngpt()
    pkg.set_solver_option("lw_jac_inline", inline)
    cols, cloud = case(k, 3, ncol, nlay)
    n3 = ncol * nlay * ng
    need = (n3 + 32) * 8 if nlay == 60 else (4 * n3 + ncol * ng + 64) * 8 + pkg.rte_lw_scratch_bytes(ncol, nlay, ng)
    for kw in (dict(), dict(cloud=cloud, nmus=3, inc=True), dict(cloud=cloud, both=True)):
        ref = fused_call(pkg, k, cols, t, **kw)
        stream = torch.cuda.Stream()
        buf = torch.full((need,), 0xFF, dtype=torch.uint8, device=gpu)   # (NaN patterns: stale data would show)
        torch.cuda.synchronize()
        pkg.set_stream_scratch(buf, stream=stream)
        try:
            with torch.cuda.stream(stream):
                out = fused_call(pkg, k, cols, t, **kw)
            torch.cuda.synchronize()
        finally:
            pkg.set_stream_scratch(None, stream=stream)
        assert np.array_equal(out[1], ref[1]) and all(np.array_equal(a, b) for a, b in zip(out[0], ref[0])), kw
        del buf
    # capture
    ref = fused_call(pkg, k, cols, t, cloud=cloud)
    gc = helpers.product_gas_concs(pkg, cols, t)
    part = particles(pkg, cloud, t, False)
    args = (t(cols["plev"]), t(cols["tlay"]), t(cols["tsfc"]), t(cols["tlev"]), gc, True, t(cols["emis"]), part)
    fl = pkg.FluxesBroadband(*(t(np.zeros((nlay + 1, ncol))) for _ in range(2)))
    jac = t(np.zeros((nlay + 1, ncol)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert k.lw_fluxes_allsky(*args, fl, flux_up_jac=jac) == ""   # warm-up: the stream's block exists now
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert k.lw_fluxes_allsky(*args, fl, flux_up_jac=jac) == ""
    for _ in range(2):
        for a in (fl.flux_up, fl.flux_dn, jac):
            a.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(back(fl.flux_up), ref[0][0]) and np.array_equal(back(fl.flux_dn), ref[0][1])
        assert np.array_equal(back(jac), ref[1])
    del graph
    pkg.release_scratch(0)


# ------------------------------------------------------------------------------------------------
# 9. Fortran: ecckd_driver with jac.bin
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused,with_particles", [(1, False), (1, True), (0, False)])
def test_fortran_driver_jacobian(pkg, gpu, lw, tmp_path, fused, with_particles):
    """ecckd_driver lw ... jac.bin, 250 columns in blocks of 100 (a ragged last block): fluxes and Jacobian are bit for bit
    those of the Python calls on host arrays with the same blocks -- fused = 1: lw_fluxes / lw_fluxes_allsky with
    flux_up_jac; fused = 0: gas_optics, planck_sfc_source_jac, rte_lw(flux_up_jac=)."""
    drv = driver(pkg)
    k, m, path = lw["rrtmgp"]
    nb = k.get_nband()
    ncol, nlay, block = 250, 60, 100
    cols = synthetic.columns(40, ncol, k.get_press_min(), nlay=nlay)
    cloud = synthetic.clouds(40, ncol, nlay, nb)
    names = synthetic.GAS_ORDER
    write_input(tmp_path / "in.bin", cols, names, False)
    part = ""
    if with_particles:
        write_particles(tmp_path / "part.bin", cloud, True, False)
        part = str(tmp_path / "part.bin")
    r = subprocess.run([drv, "lw", path, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(block), "1", "0", "1", "0",
                        str(fused), part, "", "", str(tmp_path / "jac.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    fu, fd = read_output(tmp_path / "out.bin", ncol, nlay)
    fj = np.fromfile(tmp_path / "jac.bin", dtype="<f8")
    assert fj.size == ncol * (nlay + 1)
    fj = fj.reshape(nlay + 1, ncol)
    pu, pd, pj = np.empty_like(fu), np.empty_like(fd), np.empty_like(fj)
    for c0 in range(0, ncol, block):
        c1 = min(ncol, c0 + block)
        nc = c1 - c0
        cut = lambda a: np.ascontiguousarray(a[..., c0:c1])
        gc = block_gas_concs(pkg, cols, names, c0, c1)
        fl = pkg.FluxesBroadband(np.empty((nlay + 1, nc)), np.empty((nlay + 1, nc)))
        jac = np.empty((nlay + 1, nc))
        emis = np.repeat(cut(cols["sfc_emis"])[:, None], nb, 1)
        args = (cut(cols["plev"]), cut(cols["tlay"]), cut(cols["tsfc"]), cut(cols["tlev"]), gc, True, emis)
        if with_particles:
            p2 = particles(pkg, {n: cut(cloud[n]) for n in ("tau", "ssa", "g")}, np.ascontiguousarray, False)
            assert k.lw_fluxes_allsky(*args, p2, fl, flux_up_jac=jac) == ""
        elif fused:
            assert k.lw_fluxes(*args, fl, flux_up_jac=jac) == ""
        else:
            op = pkg.OpticalProps1scl(); op.alloc_1scl(nc, nlay, k)
            src = pkg.SourceFuncLW(); src.alloc(nc, nlay, k)
            assert k.gas_optics(None, args[0], args[1], args[2], gc, op, src, tlev=args[3]) == ""
            assert k.planck_sfc_source_jac(args[2], src) == ""
            assert pkg.rte_lw(op, True, src, emis, fl, flux_up_jac=jac) == ""
        pu[:, c0:c1], pd[:, c0:c1], pj[:, c0:c1] = fl.flux_up, fl.flux_dn, jac
    assert np.array_equal(fu, pu) and np.array_equal(fd, pd) and np.array_equal(fj, pj)
    assert np.all(fj > 0.0)
