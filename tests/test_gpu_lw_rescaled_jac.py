"""The rescaled longwave solver's clear-sky outputs and surface-temperature Jacobian on the GPU: ecckd_rte_lw_rescaled_jac
(rte_lw_rescaled_jac) and the fused superset ecckd_lw_fluxes_rescaled_jac (GasOpticsEcckd.lw_fluxes_rescaled).

Yardstick of the Jacobian: the numpy restatement tests/lw_rescaled_ref.py run with every layer, level and incident source
zero and sfc_source_jac as the surface source (tied on the CPU to a finite difference of the restatement by
tests/test_lw_rescaled_jac_host.py), flux_up summed over the g-points, within helpers.FLUX_ATOL (1e-9, the project's fp64
flux bar, as in tests/test_gpu_lw_jac.py).  The zero-source run's flux_dn is not zero under rescaling and is not looked at.
Fluxes are compared bit for bit with the calls they must equal.  Every test prints the distances it asserts on.

Inputs: random_case of tests/test_gpu_lw_rescaled.py with tau x 0.02 at 8 layers and more, so that the Jacobian at the top of
the domain is not zero.

Measured on an MI355X: the Jacobian at most 7.2e-15 W m-2 K-1 from the yardstick (solver call) and 6.3e-15 (fused call), 5.4e-15
between the two "lw_jac_inline" routes, 0 from the no-scattering Jacobian where ssa = 0 and on clear columns; scattering moves
the Jacobian at the top of the domain by 1.7e-3 ... 0.29 on the scattering columns; the finite difference in tsfc is within
3.8e-13; every bit-for-bit case holds as an equality; Jacobians at the top of the domain reach 1.6 W m-2 K-1."""
import numpy as np
import pytest

import helpers
import lw_rescaled_ref as ref
from helpers import FLUX_ATOL
from test_gpu_lw_jac import oracle_sfc_jac, run_rte_lw
from test_gpu_lw_rescaled import T, back, band_particles, bands_of, fused, fused_case, per_gpt, random_case, solve, to_mask

pytestmark = pytest.mark.gpu
BAR = FLUX_ATOL
FD_BAR = 1e-8        # a finite difference in tsfc against the Jacobian: the bar of the same check in tests/test_gpu_lw_jac.py
host = lambda x: np.ascontiguousarray(x).copy()


@pytest.fixture(autouse=True)
def default_options(pkg):
    pkg.reset_solver_options()
    pkg.set_arithmetic(pkg.FAST)
    inline = pkg.get_solver_option("lw_jac_inline")
    yield
    pkg.reset_solver_options()
    pkg.set_arithmetic(pkg.FAST)
    pkg.set_solver_option("lw_jac_inline", inline)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------
# the solver call
# ---------------------------------------------------------------------------------------------------------------------
def jac_case(ncol, nlay, ng, nband, seed):
    a = random_case(ncol, nlay, ng, nband, seed)
    if nlay >= 8:
        a["tau"] = a["tau"] * 0.02
    a["sfc_source_jac"] = np.random.default_rng(seed + 1).uniform(0.01, 0.2, (ng, ncol))
    return a


def flipped(a):
    return dict(ref.flip_orientation(a), sfc_source_jac=a["sfc_source_jac"])


def solve_jac(pkg, a, band2gpt, to, top_at_1=True, nmus=1, inc=True):
    """rte_lw_rescaled_jac on the inputs dict `a`; outputs pre-filled with -1."""
    ng, nlay, ncol = a["tau"].shape
    op = pkg.OpticalProps2str()
    op.tau, op.ssa, op.g = to(a["tau"]), to(a["ssa"]), to(a["g"])
    op.band2gpt = np.asarray(band2gpt)
    src = pkg.SourceFuncLW()
    src.lay_source, src.lev_source_inc, src.lev_source_dec, src.sfc_source = to(a["lay"]), to(a["inc"]), to(a["dec"]), to(a["sfc_source"])
    src.sfc_source_jac = to(a["sfc_source_jac"])
    fl = pkg.FluxesBroadband(to(np.full((nlay + 1, ncol), -1.0)), to(np.full((nlay + 1, ncol), -1.0)))
    jac = to(np.full((nlay + 1, ncol), -1.0))
    assert pkg.rte_lw_rescaled_jac(op, top_at_1, src, to(a["sfc_emis"]), fl, jac, n_gauss_angles=nmus,
                                   inc_flux=to(a["inc_flux"]) if inc else None) == ""
    return back(fl.flux_up), back(fl.flux_dn), back(jac)


def yardstick(tau, ssa, g, emis_gpt, sfc_source_jac, top_at_1, nmus):
    zero = np.zeros_like(tau)
    return ref.broadband(ref.restate(tau, ssa, g, zero, zero, zero, emis_gpt, sfc_source_jac, None, top_at_1, nmus)[0])


def no_scattering_jac(pkg, a, tau, b2g, to, top_at_1=True, nmus=1):
    """rte_lw(flux_up_jac=) -- the absorption-only Jacobian -- on `tau` with the other inputs of `a`."""
    c = dict(tau=tau, lay=a["lay"], inc=a["inc"], dec=a["dec"], sfc=a["sfc_source"], sfc_jac=a["sfc_source_jac"], emis=a["sfc_emis"],
             inc_flux=a["inc_flux"], b2g=np.asarray(b2g, dtype=np.int32))
    return run_rte_lw(pkg, c, to, top_at_1, nmus, False, True)[2]


@pytest.mark.parametrize("ncol,nlay,ng", [(1, 60, 32), (33, 60, 33), (37, 8, 5), (33, 1, 3), (65, 137, 32)])
def test_solver_call(pkg, gpu, ncol, nlay, ng):
    """Both orientations, 1 and 3 angles, with and without inc_flux: the fluxes are those of rte_lw(rescaled=True) bit for bit,
    the Jacobian is within the bar of the yardstick and the same bits with and without inc_flux; host arrays give the bits of
    device arrays.  (33 g-points: the last wave lane carries weight 0.)"""
    b2g = bands_of(ng, "each")
    a = jac_case(ncol, nlay, ng, ng, 100 * ncol + nlay)
    t = T(gpu)
    worst, top_min, top_max = 0.0, np.inf, 0.0
    for top in (True, False):
        b = a if top else flipped(a)
        emis = per_gpt(b["sfc_emis"], b2g, ng)
        for nmus in (1, 3):
            want = yardstick(b["tau"], b["ssa"], b["g"], emis, b["sfc_source_jac"], top, nmus)
            jacs = []
            for inc in (True, False):
                up, dn, jac = solve_jac(pkg, b, b2g, t, top, nmus, inc)
                assert same((up, dn), solve(pkg, b, b2g, t, top, nmus, inc)), (top, nmus, inc)
                d = float(np.max(np.abs(jac - want)))
                worst = max(worst, d)
                assert d <= BAR, (top, nmus, inc, d)
                jacs.append(jac)
            assert np.array_equal(jacs[0], jacs[1])
            toa = jacs[0][0 if top else -1]
            top_min, top_max = min(top_min, float(toa.min())), max(top_max, float(toa.max()))
        assert same(solve_jac(pkg, b, b2g, host, top, 3, True), solve_jac(pkg, b, b2g, t, top, 3, True))
    print("ncol %d nlay %d ng %d: Jacobian %.3e W m-2 K-1 from the yardstick (bar %.0e); at the top of the domain %.3e ... %.3e"
          % (ncol, nlay, ng, worst, BAR, top_min, top_max))
    assert top_max > 1e3 * BAR


def test_solver_call_more_tiles_than_one_round(pkg, gpu):
    """More tiles of 32 columns than the Jacobian kernel's grid has blocks (16384): the first blocks walk a second tile with
    accumulators they have cleared."""
    ncol, nlay, ng = 16384 * 32 + 37, 1, 1
    b2g = bands_of(ng, "each")
    a = jac_case(ncol, nlay, ng, ng, 5)
    up, dn, jac = solve_jac(pkg, a, b2g, T(gpu))
    assert same((up, dn), solve(pkg, a, b2g, T(gpu)))
    d = float(np.max(np.abs(jac - yardstick(a["tau"], a["ssa"], a["g"], per_gpt(a["sfc_emis"], b2g, ng), a["sfc_source_jac"], True, 1))))
    print("%d columns x 1 layer x 1 g: Jacobian %.3e W m-2 K-1 from the yardstick (bar %.0e)" % (ncol, d, BAR))
    assert d <= BAR


@pytest.mark.parametrize("ncol,nlay,ng", [(37, 60, 5), (37, 8, 5), (33, 1, 3)])
def test_scattering_is_in_the_jacobian(pkg, gpu, ncol, nlay, ng):
    """On every column with ssa > 0 the Jacobian at the top of the domain differs from the absorption-only Jacobian --
    rte_lw(flux_up_jac=) on tau*(1 - ssa) -- by more than 20 x the bar; with ssa = 0 it is within the bar of
    rte_lw(flux_up_jac=) on tau."""
    b2g = bands_of(ng, "each")
    a = jac_case(ncol, nlay, ng, ng, 7 + nlay)
    t = T(gpu)
    scat = np.any(a["ssa"] > 0, axis=(0, 1))
    assert scat.any() and (~scat).any()
    for nmus in (1, 3):
        jac = solve_jac(pkg, a, b2g, t, True, nmus)[2]
        absorb = no_scattering_jac(pkg, a, a["tau"] * (1.0 - a["ssa"]), b2g, t, True, nmus)
        effect = np.abs(jac[0] - absorb[0])
        print("nlay %d, %d angles: scattering moves the Jacobian at the top by %.3e ... %.3e W m-2 K-1 on the scattering columns (20 x bar %.0e)"
              % (nlay, nmus, effect[scat].min(), effect[scat].max(), 20 * BAR))
        assert np.all(effect[scat] > 20 * BAR)
        b = dict(a, ssa=np.zeros_like(a["ssa"]))
        d = float(np.max(np.abs(solve_jac(pkg, b, b2g, t, True, nmus)[2] - no_scattering_jac(pkg, b, b["tau"], b2g, t, True, nmus))))
        print("nlay %d, %d angles, ssa = 0: %.3e W m-2 K-1 from rte_lw(flux_up_jac=) (bar %.0e)" % (nlay, nmus, d, BAR))
        assert d <= BAR


# ---------------------------------------------------------------------------------------------------------------------
# the fused call
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(pkg, gpu, oracle_mod):
    from conftest import LW_FSCK
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=0) == ""
    return k, oracle_mod.CkdModel(LW_FSCK)


def inline_forms(nlay):
    """Values of "lw_jac_inline" that take different routes at this layer count: both at 60 layers."""
    return (0, 1) if nlay == 60 else (0,)


def fused_new(pkg, k, cols, cloud, mask, to, device=True, top_at_1=True, inc=True, nmus=1, clear=False, jac=False, tsfc=None):
    """lw_fluxes_rescaled; returns (flux_up, flux_dn), (clear up, clear dn) or None, jac or None.  Outputs pre-filled with -1."""
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to)
    new = lambda: to(np.full((nlay + 1, ncol), -1.0))
    fl = pkg.FluxesBroadband(new(), new())
    flc = pkg.FluxesBroadband(new(), new()) if clear else None
    j = new() if jac else None
    assert k.lw_fluxes_rescaled(to(cols["plev"]), to(cols["tlay"]), to(cols["tsfc"] if tsfc is None else tsfc), to(cols["tlev"]), gc, top_at_1,
                                to(cols["emis"]), band_particles(pkg, cloud, to), fl, fluxes_clear=flc, flux_up_jac=j, n_gauss_angles=nmus,
                                inc_flux=to(cols["inc_flux"]) if inc else None, cloud_mask=to_mask(mask, to, device)) == ""
    return ((back(fl.flux_up), back(fl.flux_dn)), None if flc is None else (back(flc.flux_up), back(flc.flux_dn)),
            None if j is None else back(j))


def clear_sky(pkg, k, cols, to, top_at_1=True, inc=True, nmus=1, jac=False):
    """lw_fluxes on the same atmosphere."""
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to)
    fl = pkg.FluxesBroadband(to(np.full((nlay + 1, ncol), -2.0)), to(np.full((nlay + 1, ncol), -2.0)))
    j = to(np.full((nlay + 1, ncol), -2.0)) if jac else None
    assert k.lw_fluxes(to(cols["plev"]), to(cols["tlay"]), to(cols["tsfc"]), to(cols["tlev"]), gc, top_at_1, to(cols["emis"]), fl,
                       n_gauss_angles=nmus, inc_flux=to(cols["inc_flux"]) if inc else None, flux_up_jac=j) == ""
    return (back(fl.flux_up), back(fl.flux_dn)), None if j is None else back(j)


def composed_triple(pkg, k, cols, cloud, mask, to):
    """(tau, ssa, g) of the composed route: gas_optics_tau, then increment[_masked] by band on (tau, 0, 0)."""
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to)
    like = to(np.zeros(1))
    one = pkg.OpticalProps1scl(); one.alloc_1scl(ncol, nlay, k, like=like)
    assert k.gas_optics_tau(to(cols["plev"]), to(cols["tlay"]), gc, one) == ""
    op = pkg.OpticalProps2str(); op.alloc_2str(ncol, nlay, k, like=like)
    op.tau.copy_(one.tau); op.ssa.zero_(); op.g.zero_()
    assert op.increment(band_particles(pkg, cloud, to), band2gpt=k.get_band2gpt(), cloud_mask=to_mask(mask, to, True)) == ""
    return back(op.tau), back(op.ssa), back(op.g)


@pytest.mark.parametrize("nlay,ncol", [(60, 37), (61, 17), (8, 16)])
def test_fused_call(pkg, gpu, model, oracle_mod, nlay, ncol):
    """With and without a sampled mask, both orientations, one angle with inc_flux and three without, both values of
    "lw_jac_inline" at 60 layers: the all-sky fluxes are those of lw_fluxes_allsky(rescaled=True) bit for bit whatever else is
    asked for; the clear-sky fluxes are those of lw_fluxes bit for bit; the Jacobian is within the bar of the yardstick on the
    (tau, ssa, g) of the composed route and the oracle's sfc_source(tsfc + 1) - sfc_source(tsfc); the two inline routes agree
    within the bar; host arrays give the bits of device arrays."""
    (k, m), t = model, T(gpu)
    ng = k.get_ngpt()
    cols, cloud, mask = fused_case(pkg, k, 40 + nlay, ncol, nlay)
    assert cloud["cloudy"].any() and np.any(mask != 0) and np.any(mask != np.uint64(2 ** ng - 1))
    sjac = oracle_sfc_jac(oracle_mod, m, cols["tsfc"])
    emis = per_gpt(cols["emis"], k.get_band2gpt(), ng)
    worst, between, top_min, top_max = 0.0, 0.0, np.inf, 0.0
    for msk in (None, mask):
        triple = composed_triple(pkg, k, cols, cloud, msk, t)
        for top in (True, False):
            for inc, nmus in ((True, 1), (False, 3)):
                kw = dict(top_at_1=top, inc=inc, nmus=nmus)
                old = fused(pkg, k, cols, cloud, msk, t, True, top, inc, nmus)
                clr = clear_sky(pkg, k, cols, t, top, inc, nmus)[0]
                want = yardstick(*triple, emis, sjac, top, nmus)
                plain = fused_new(pkg, k, cols, cloud, msk, t, **kw)
                assert same(plain[0], old) and plain[1] is None and plain[2] is None, (msk is not None, kw)
                both = fused_new(pkg, k, cols, cloud, msk, t, clear=True, **kw)
                assert same(both[0], old) and same(both[1], clr), (msk is not None, kw)
                jacs = {}
                for inline in inline_forms(nlay):
                    pkg.set_solver_option("lw_jac_inline", inline)
                    only = fused_new(pkg, k, cols, cloud, msk, t, jac=True, **kw)
                    every = fused_new(pkg, k, cols, cloud, msk, t, clear=True, jac=True, **kw)
                    assert same(only[0], old) and same(every[0], old) and same(every[1], clr), (msk is not None, kw, inline)
                    assert np.array_equal(only[2], every[2])
                    d = float(np.max(np.abs(only[2] - want)))
                    worst = max(worst, d)
                    assert d <= BAR, (msk is not None, kw, inline, d)
                    jacs[inline] = only[2]
                if len(jacs) == 2:
                    d = float(np.max(np.abs(jacs[0] - jacs[1])))
                    between = max(between, d)
                    assert d <= BAR, (msk is not None, kw, d)
                toa = only[2][0 if top else -1]
                top_min, top_max = min(top_min, float(toa.min())), max(top_max, float(toa.max()))
        hst = fused_new(pkg, k, cols, cloud, msk, host, device=False, clear=True, jac=True)
        dev = fused_new(pkg, k, cols, cloud, msk, t, clear=True, jac=True)
        assert same(hst[0], dev[0]) and same(hst[1], dev[1]) and np.array_equal(hst[2], dev[2])
    print("nlay %d: Jacobian %.3e W m-2 K-1 from the yardstick, %.3e between the two lw_jac_inline routes (bar %.0e); at the top %.3e ... %.3e"
          % (nlay, worst, between, BAR, top_min, top_max))


@pytest.mark.parametrize("nlay,ncol", [(60, 37), (61, 17), (8, 16)])
def test_fused_jacobian_on_clear_columns_and_by_finite_difference(pkg, gpu, model, nlay, ncol):
    """On the clear columns of a cloudy call the Jacobian is within the bar of lw_fluxes(flux_up_jac=); and
    lw_fluxes_rescaled at tsfc + 1 minus at tsfc, in flux_up, is within 1e-8 of flux_up_jac on every column."""
    (k, _), t = model, T(gpu)
    cols, cloud, _ = fused_case(pkg, k, 40 + nlay, ncol, nlay)
    clear_cols = ~cloud["cloudy"]
    assert clear_cols.any() and cloud["cloudy"].any()
    for inline in inline_forms(nlay):
        pkg.set_solver_option("lw_jac_inline", inline)
        for nmus in (1, 3):
            base = fused_new(pkg, k, cols, cloud, None, t, nmus=nmus, jac=True)
            want = clear_sky(pkg, k, cols, t, nmus=nmus, jac=True)[1]
            d = float(np.max(np.abs(base[2][:, clear_cols] - want[:, clear_cols])))
            warm = fused_new(pkg, k, cols, cloud, None, t, nmus=nmus, tsfc=cols["tsfc"] + 1.0)
            fd = float(np.max(np.abs((warm[0][0] - base[0][0]) - base[2])))
            moved = float(np.max(np.abs(base[2][:, cloud["cloudy"]] - want[:, cloud["cloudy"]])))
            print("nlay %d inline %d, %d angles: clear columns %.3e from lw_fluxes(flux_up_jac=) (bar %.0e; cloudy columns differ by up to %.3e); "
                  "finite difference in tsfc %.3e (bar %.0e)" % (nlay, inline, nmus, d, BAR, moved, fd, FD_BAR))
            assert d <= BAR and fd <= FD_BAR


@pytest.mark.parametrize("nlay", [60, 61])
def test_caller_owned_scratch_and_graph_capture(pkg, gpu, model, nlay):
    """On a caller-owned block of exactly ecckd_lw_fluxes_rescaled_jac_scratch_bytes, filled with 0xFF bytes, the call gives
    the eager bits; and after one warm-up call on the stream a capture replays to the eager bits."""
    import torch
    (k, _), t = model, T(gpu)
    ncol = 17
    cols, cloud, mask = fused_case(pkg, k, 3, ncol, nlay)
    for clear in (False, True):
        want = fused_new(pkg, k, cols, cloud, mask, t, nmus=2, clear=clear, jac=True)
        need = k.lw_fluxes_rescaled_scratch_bytes(ncol, nlay, clear)
        stream = torch.cuda.Stream()
        buf = torch.full((need,), 0xFF, dtype=torch.uint8, device=gpu)   # (NaN patterns: stale data would show)
        torch.cuda.synchronize()
        pkg.set_stream_scratch(buf, stream=stream)
        try:
            with torch.cuda.stream(stream):
                got = fused_new(pkg, k, cols, cloud, mask, t, nmus=2, clear=clear, jac=True)
            torch.cuda.synchronize()
        finally:
            pkg.set_stream_scratch(None, stream=stream)
        assert same(got[0], want[0]) and np.array_equal(got[2], want[2]) and (not clear or same(got[1], want[1])), clear
        del buf
    # capture
    gc = helpers.product_gas_concs(pkg, cols, t)
    args = (t(cols["plev"]), t(cols["tlay"]), t(cols["tsfc"]), t(cols["tlev"]), gc, True, t(cols["emis"]), band_particles(pkg, cloud, t))
    new = lambda: t(np.zeros((nlay + 1, ncol)))
    fl, flc, jac = pkg.FluxesBroadband(new(), new()), pkg.FluxesBroadband(new(), new()), new()
    kw = dict(fluxes_clear=flc, flux_up_jac=jac, inc_flux=t(cols["inc_flux"]), cloud_mask=to_mask(mask, t, True), n_gauss_angles=2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert k.lw_fluxes_rescaled(*args, fl, **kw) == ""   # warm-up: the stream's block exists now
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert k.lw_fluxes_rescaled(*args, fl, **kw) == ""
    for a in (fl.flux_up, fl.flux_dn, flc.flux_up, flc.flux_dn, jac):
        a.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert same((back(fl.flux_up), back(fl.flux_dn)), want[0]) and same((back(flc.flux_up), back(flc.flux_dn)), want[1])
    assert np.array_equal(back(jac), want[2])
    del graph
    pkg.release_scratch(0)
