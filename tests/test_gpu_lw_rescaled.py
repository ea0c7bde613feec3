"""The rescaled no-scattering longwave solver on the GPU: ecckd_rte_lw_rescaled (rte_lw(rescaled=True)), the spectral
ecckd_lw_solver_1rescl_gpt and the fused ecckd_lw_fluxes_allsky_rescaled.

Yardsticks: the numpy restatement tests/lw_rescaled_ref.py (tied on the CPU to the oracle's no-scattering solver and to the
two-stream solution by tests/test_lw_rescaled_host.py) within BAR; the no-scattering calls in the two limits where the
solvers coincide, within BAR; and -- for the fused call -- bit equality with the composed route gas_optics_tau,
planck_sources, increment by band on (tau, 0, 0), rte_lw(rescaled=True).  Every test prints the figure it asserts on.

BAR: 4 x the largest distance measured on an MI355X over the cases of this file (fluxes up to 540 W m-2); it tolerates the
difference between the C library's exp and the solver's own on other machines, and is never looser than 1e-11 W m-2 --
beyond that a difference is not rounding.  Measured: from the restatement at most 5.7e-13 W m-2 at 60 layers and 2.3e-13
elsewhere (per g-point 7e-15); from the no-scattering solver with ssa = 0 or g = 1 at most 6.9e-13; the fused call with
g_p = 1 from ecckd_lw_fluxes_allsky 4.6e-13; every bit-for-bit case holds as an equality; the scattering effect at the top of
the cloudy columns is 0.9 ... 7.7 W m-2."""
import numpy as np
import pytest

import helpers
import lw_rescaled_ref as ref
from rte_ecckd_amd import synthetic

pytestmark = pytest.mark.gpu
MEASURED = 6.9e-13   # W m-2: the largest figure above
BAR = min(4 * MEASURED, 1e-11)
TILE = 32            # columns per tile of the 60-layer kernels


@pytest.fixture(autouse=True)
def default_options(pkg):
    pkg.reset_solver_options()
    pkg.set_arithmetic(pkg.FAST)
    yield
    pkg.reset_solver_options()
    pkg.set_arithmetic(pkg.FAST)


def T(gpu):
    import torch
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def back(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def random_case(ncol, nlay, ng, nband, seed):
    rng = np.random.default_rng(seed)
    shape = (ng, nlay, ncol)
    tau = 10.0 ** rng.uniform(-2.0, np.log10(30.0), shape)
    tau[rng.uniform(size=shape) < 0.05] = 0.0
    tau[rng.uniform(size=shape) < 0.05] *= 1e-9          # below the series threshold
    ssa, g = rng.uniform(0.0, 0.999, shape), rng.uniform(-0.2, 0.95, shape)
    ssa[:, :, ::5] = 0.0
    Tl = 215.0 + np.cumsum(rng.uniform(-0.3, 80.0 / (nlay + 1), (nlay + 1, ncol)), axis=0)
    lev = rng.uniform(3.0, 5.0, (ng, 1, 1)) * (Tl[None] / 250.0) ** 4
    inc, dec = np.ascontiguousarray(lev[:, 1:]), np.ascontiguousarray(lev[:, :-1])
    if nlay > 1:   # level sources that differ between the two layers of a level, in the odd columns
        inc[:, :-1, 1::2] *= 1.0 + rng.uniform(-0.02, 0.02, (ng, nlay - 1, ncol))[:, :, 1::2]
    lay = 0.5 * (inc + dec) * rng.uniform(0.99, 1.01, shape)
    return dict(tau=tau, ssa=ssa, g=g, lay=lay, inc=inc, dec=dec, sfc_emis=rng.uniform(0.8, 1.0, (ncol, nband)),
                sfc_source=rng.uniform(3.0, 6.0, (ng, ncol)), inc_flux=rng.uniform(0.0, 20.0, (ng, ncol)))


def bands_of(ng, kind):
    return np.array([[1, 3], [4, 5]]) if kind == "two" else np.array([[i, i] for i in range(1, ng + 1)])


def per_gpt(emis, band2gpt, ng):
    out = np.empty((ng, emis.shape[0]))
    for b, (lo, hi) in enumerate(band2gpt):
        out[lo - 1:hi] = emis[:, b][None]
    return out


def solve(pkg, a, band2gpt, to, top_at_1=True, nmus=1, inc=True, rescaled=True):
    """rte_lw(rescaled=True) on the inputs dict `a`; outputs pre-filled with -1.  rescaled=False: the no-scattering call on
    a["tau"] alone."""
    ng, nlay, ncol = a["tau"].shape
    op = pkg.OpticalProps2str() if rescaled else pkg.OpticalProps1scl()
    op.tau = to(a["tau"])
    if rescaled:
        op.ssa, op.g = to(a["ssa"]), to(a["g"])
    op.band2gpt = np.asarray(band2gpt)
    src = pkg.SourceFuncLW()
    src.lay_source, src.lev_source_inc, src.lev_source_dec, src.sfc_source = to(a["lay"]), to(a["inc"]), to(a["dec"]), to(a["sfc_source"])
    fl = pkg.FluxesBroadband(to(np.full((nlay + 1, ncol), -1.0)), to(np.full((nlay + 1, ncol), -1.0)))
    kw = dict(rescaled=True) if rescaled else {}
    assert pkg.rte_lw(op, top_at_1, src, to(a["sfc_emis"]), fl, n_gauss_angles=nmus, inc_flux=to(a["inc_flux"]) if inc else None, **kw) == ""
    return back(fl.flux_up), back(fl.flux_dn)


def restated(a, band2gpt, top_at_1=True, nmus=1, inc=True, **kw):
    ng = a["tau"].shape[0]
    up, dn = ref.restate(a["tau"], a["ssa"], a["g"], a["lay"], a["inc"], a["dec"], per_gpt(a["sfc_emis"], band2gpt, ng), a["sfc_source"],
                         a["inc_flux"] if inc else None, top_at_1, nmus, **kw)
    return ref.broadband(up), ref.broadband(dn)


def distance(got, want):
    return max(float(np.max(np.abs(got[0] - want[0]))), float(np.max(np.abs(got[1] - want[1]))))


@pytest.mark.parametrize("ncol,nlay,ng", [(1, 1, 3), (37, 8, 5), (300, 61, 3)])
def test_spectral_route(pkg, gpu, ncol, nlay, ng):
    """ecckd_lw_solver_1rescl_gpt equals the restatement per g-point, host and device arrays give the same bits, and its
    g-point sum is the broadband call's away from 60 layers bit for bit (the same kernel and sum)."""
    b2g = bands_of(ng, "each")
    a = random_case(ncol, nlay, ng, ng, 31 * ncol + nlay)
    emis = per_gpt(a["sfc_emis"], b2g, ng)
    t = T(gpu)
    for top in (True, False):
        b = a if top else ref.flip_orientation(a)
        for nmus in (1, 3):
            Ds, W = ref.GAUSS_DS[nmus - 1], ref.GAUSS_WTS[nmus - 1]
            want = ref.restate(b["tau"], b["ssa"], b["g"], b["lay"], b["inc"], b["dec"], emis, b["sfc_source"], b["inc_flux"], top, nmus)
            got = {}
            for space, to in (("device", t), ("host", lambda x: np.ascontiguousarray(x).copy())):
                up, dn = to(np.full((ng, nlay + 1, ncol), -1.0)), to(np.full((ng, nlay + 1, ncol), -1.0))
                assert pkg.lw_solver_1rescl_gpt(*(to(b[k]) for k in ("tau", "ssa", "g", "lay", "inc", "dec")), to(emis), to(b["sfc_source"]),
                                                up, dn, top_at_1=top, Ds=Ds, weights=W, inc_flux=to(b["inc_flux"])) == ""
                if space == "device":
                    import torch
                    torch.cuda.synchronize()
                got[space] = (back(up), back(dn))
            assert np.array_equal(got["device"][0], got["host"][0]) and np.array_equal(got["device"][1], got["host"][1])
            d = distance(got["device"], want)
            bb = solve(pkg, b, b2g, t, top, nmus)
            same = np.array_equal(ref.broadband(got["device"][0]), bb[0]) and np.array_equal(ref.broadband(got["device"][1]), bb[1])
            print("spectral ncol %d nlay %d ng %d top %d nmus %d: %.3e W m-2 from the restatement (bar %.1e)" % (ncol, nlay, ng, top, nmus, d, BAR))
            assert d <= BAR and same


# 60 layers (the layer-split kernel): one below, at and one above the tile width, several tiles with a partial last one;
# g-point groups of two lanes that end ragged (3, 5, 27) and full (32); both band tables.  Other layer counts (the
# compatibility kernel): 1, 8, 59, 61.
SHAPES = [(TILE - 1, 60, 3, "each"), (TILE, 60, 5, "two"), (TILE + 1, 60, 27, "each"), (37, 60, 32, "each"), (2 * TILE + 5, 60, 5, "each"),
          (37, 1, 5, "two"), (17, 8, 3, "each"), (TILE + 1, 59, 5, "two"), (16, 61, 27, "each")]


@pytest.mark.parametrize("ncol,nlay,ng,kind", SHAPES)
def test_against_the_restatement(pkg, gpu, ncol, nlay, ng, kind):
    """Both orientations, with and without inc_flux, one angle and three."""
    b2g = bands_of(ng, kind)
    a = random_case(ncol, nlay, ng, b2g.shape[0], 1000 * ncol + 10 * nlay + ng)
    worst = 0.0
    for top in (True, False):
        b = a if top else ref.flip_orientation(a)
        for nmus, inc in ((1, True), (1, False), (3, top)):
            d = distance(solve(pkg, b, b2g, T(gpu), top, nmus, inc), restated(b, b2g, top, nmus, inc))
            worst = max(worst, d)
    print("ncol %d nlay %d ng %d: %.3e W m-2 from the restatement (bar %.1e)" % (ncol, nlay, ng, worst, BAR))
    assert worst <= BAR


@pytest.mark.parametrize("nlay", [60, 8])
def test_every_angle_count(pkg, gpu, nlay):
    b2g = bands_of(5, "two")
    a = random_case(TILE + 1, nlay, 5, 2, 5 + nlay)
    for nmus in (1, 2, 3, 4):
        d = distance(solve(pkg, a, b2g, T(gpu), True, nmus), restated(a, b2g, True, nmus))
        print("nlay %d, %d angles: %.3e W m-2 from the restatement (bar %.1e)" % (nlay, nmus, d, BAR))
        assert d <= BAR


def test_more_tiles_than_one_round(pkg, gpu):
    """60 layers: more tiles than the persistent grid has blocks (2048 x 32 columns), so the first blocks walk a second tile
    with accumulators they have cleared.  One layer: more (column, g-point) pairs than the compatibility kernel's grid has
    threads (16384 x 256)."""
    for ncol, nlay, ng in ((2048 * TILE + 37, 60, 1), (16384 * 256 // 3 + 300, 1, 3)):
        b2g = bands_of(ng, "each")
        a = random_case(ncol, nlay, ng, ng, 77)
        d = distance(solve(pkg, a, b2g, T(gpu)), restated(a, b2g))
        print("%d columns x %d layers x %d g: %.3e W m-2 from the restatement (bar %.1e)" % (ncol, nlay, ng, d, BAR))
        assert d <= BAR


@pytest.mark.parametrize("nlay", [60, 8])
def test_without_scattering_it_is_the_no_scattering_solver(pkg, gpu, nlay):
    """ssa = 0 gives the fluxes of ecckd_rte_lw_inc_flux, g = 1 those of ecckd_rte_lw_inc_flux on tau*(1 - ssa): to the
    rounding bar, not bit for bit (the sweeps are composed and summed in another order)."""
    b2g = bands_of(27, "each")
    a = random_case(37, nlay, 27, 27, 3 + nlay)
    t = T(gpu)
    for what, b in (("ssa = 0", dict(a, ssa=np.zeros_like(a["ssa"]))), ("g = 1", dict(a, g=np.ones_like(a["g"])))):
        for nmus in (1, 3):
            got = solve(pkg, b, b2g, t, True, nmus)
            want = solve(pkg, dict(b, tau=b["tau"] * (1.0 - b["ssa"])), b2g, t, True, nmus, rescaled=False)
            d = distance(got, want)
            print("nlay %d, %s, %d angles: %.3e W m-2 from the no-scattering call (bar %.1e)" % (nlay, what, nmus, d, BAR))
            assert d <= BAR


@pytest.mark.parametrize("nlay", [60, 8])
def test_nan_and_conservative_forward_scattering_stay_in_their_columns(pkg, gpu, nlay):
    """A NaN in one column's tau, and ssa = g = 1 (0/0 in Cn, unguarded as in RTE) in another: every other column keeps its
    bits, and the two columns are NaN below the top."""
    a = random_case(37, nlay, 5, 2, 10 + nlay)
    b2g = bands_of(5, "two")
    bad = dict(a, tau=a["tau"].copy(), ssa=a["ssa"].copy(), g=a["g"].copy())
    bad["tau"][:, :, 18] = np.nan
    bad["ssa"][:, :, 6] = 1.0
    bad["g"][:, :, 6] = 1.0
    others = ~np.isin(np.arange(37), (6, 18))
    for top in (True, False):
        c, d = (a, bad) if top else (ref.flip_orientation(a), ref.flip_orientation(bad))
        clean, dirty = solve(pkg, c, b2g, T(gpu), top), solve(pkg, d, b2g, T(gpu), top)
        for x, y in zip(clean, dirty):
            assert np.array_equal(x[:, others], y[:, others])
        up = dirty[0] if top else dirty[0][::-1]
        assert np.all(np.isnan(up[:-1, 18])) and np.all(np.isnan(up[:-1, 6]))


@pytest.mark.parametrize("nlay", [60, 8])
def test_solver_options_act_as_on_the_no_scattering_solver(pkg, gpu, nlay):
    """lw_tau_thresh, lw_series_terms and lw_inc_flux_isotropic reach the kernels: with each set, the call follows the
    restatement under the same setting, and differs from the default call."""
    b2g = bands_of(5, "two")
    a = random_case(TILE + 1, nlay, 5, 2, 21 + nlay)
    a["tau"][:, ::2] *= 0.05          # optical depths between the default threshold and the one set below
    t = T(gpu)
    base = solve(pkg, a, b2g, t, True, 3)
    for opts, kw in ((dict(lw_tau_thresh=0.5), dict(tau_thresh=0.5)),
                     (dict(lw_tau_thresh=0.5, lw_series_terms=3), dict(tau_thresh=0.5, series_terms=3)),
                     (dict(lw_inc_flux_isotropic=1), dict(inc_isotropic=True))):
        pkg.reset_solver_options()
        for name, v in opts.items():
            pkg.set_solver_option(name, v)
        got = solve(pkg, a, b2g, t, True, 3)
        d, moved = distance(got, restated(a, b2g, True, 3, **kw)), distance(got, base)
        print("nlay %d %s: %.3e W m-2 from the restatement (bar %.1e), %.3e from the default call" % (nlay, opts, d, BAR, moved))
        assert d <= BAR and moved > 1e-6
    pkg.reset_solver_options()
    again = solve(pkg, a, b2g, t, True, 3)
    assert np.array_equal(again[0], base[0]) and np.array_equal(again[1], base[1])


def test_host_arrays_equal_device_arrays(pkg, gpu):
    for nlay in (60, 8):
        a = random_case(37, nlay, 5, 2, 9)
        b2g = bands_of(5, "two")
        dev = solve(pkg, a, b2g, T(gpu), True, 2)
        host = solve(pkg, a, b2g, lambda x: np.ascontiguousarray(x).copy(), True, 2)
        assert np.array_equal(dev[0], host[0]) and np.array_equal(dev[1], host[1])
        assert np.all(np.isfinite(dev[0])) and np.all(dev[1] >= 0)


# ---------------------------------------------------------------------------------------------------------------------
# the fused call
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(pkg, gpu):
    from conftest import LW_FSCK
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=0) == ""
    return k


def fused_case(pkg, k, c0, ncol, nlay):
    cols = synthetic.columns(c0, ncol, k.get_press_min(), nlay=nlay)
    cloud = synthetic.clouds(c0, ncol, nlay, k.get_nband())
    rng = np.random.default_rng(c0)
    cols["inc_flux"] = rng.uniform(0.0, 2.0, (k.get_ngpt(), ncol))
    cols["emis"] = np.repeat(cols["sfc_emis"][:, None], k.get_nband(), 1) * rng.uniform(0.95, 1.0, (ncol, k.get_nband()))
    cf = np.ascontiguousarray(synthetic.cloud_fraction(c0, ncol, nlay))
    mask = pkg.sample_cloud_mask(cf, k.get_ngpt(), seed=c0)
    return cols, cloud, mask


def band_particles(pkg, cloud, to):
    op = pkg.OpticalProps2str()
    op.tau, op.ssa, op.g = to(cloud["tau"].copy()), to(cloud["ssa"].copy()), to(cloud["g"].copy())
    return op


def to_mask(mask, to, device):
    if mask is None:
        return None
    return to(mask.view(np.int64)) if device else mask.copy()


def fused(pkg, k, cols, cloud, mask, to, device=True, top_at_1=True, inc=True, nmus=1, rescaled=True):
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to)
    fl = pkg.FluxesBroadband(to(np.full((nlay + 1, ncol), -1.0)), to(np.full((nlay + 1, ncol), -1.0)))
    kw = dict(rescaled=True) if rescaled else {}
    assert k.lw_fluxes_allsky(to(cols["plev"]), to(cols["tlay"]), to(cols["tsfc"]), to(cols["tlev"]), gc, top_at_1, to(cols["emis"]),
                              band_particles(pkg, cloud, to), fl, n_gauss_angles=nmus, inc_flux=to(cols["inc_flux"]) if inc else None,
                              cloud_mask=to_mask(mask, to, device), **kw) == ""
    return back(fl.flux_up), back(fl.flux_dn)


def composed(pkg, k, cols, cloud, mask, to, top_at_1=True, inc=True, nmus=1):
    """gas_optics_tau -> planck_sources -> increment[_masked] by band on (tau, 0, 0) -> rte_lw(rescaled=True)."""
    import torch
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to)
    like = to(np.zeros(1))
    one = pkg.OpticalProps1scl(); one.alloc_1scl(ncol, nlay, k, like=like)
    assert k.gas_optics_tau(to(cols["plev"]), to(cols["tlay"]), gc, one) == ""
    op = pkg.OpticalProps2str(); op.alloc_2str(ncol, nlay, k, like=like)
    op.tau.copy_(one.tau); op.ssa.zero_(); op.g.zero_()
    src = pkg.SourceFuncLW(); src.alloc(ncol, nlay, k, like=like)
    assert k.planck_sources(to(cols["tlay"]), to(cols["tsfc"]), src, tlev=to(cols["tlev"])) == ""
    assert op.increment(band_particles(pkg, cloud, to), band2gpt=k.get_band2gpt(), cloud_mask=to_mask(mask, to, True)) == ""
    fl = pkg.FluxesBroadband(to(np.full((nlay + 1, ncol), -2.0)), to(np.full((nlay + 1, ncol), -2.0)))
    assert pkg.rte_lw(op, top_at_1, src, to(cols["emis"]), fl, n_gauss_angles=nmus, rescaled=True,
                      inc_flux=to(cols["inc_flux"]) if inc else None) == ""
    torch.cuda.synchronize()
    return back(fl.flux_up), back(fl.flux_dn)


@pytest.mark.parametrize("nlay,ncol", [(60, 37), (61, 17), (8, 16)])
def test_fused_equals_the_composed_route(pkg, gpu, model, nlay, ncol):
    """Bit for bit: with and without a sampled mask, both orientations, both memory spaces, with and without inc_flux (one
    angle) and with three angles."""
    k, t = model, T(gpu)
    cols, cloud, mask = fused_case(pkg, k, 40 + nlay, ncol, nlay)
    assert cloud["cloudy"].any() and np.any(mask != 0) and np.any(mask != np.uint64(2 ** k.get_ngpt() - 1))
    for m in (None, mask):
        for top in (True, False):
            for inc, nmus in ((True, 1), (False, 1), (True, 3)):
                want = composed(pkg, k, cols, cloud, m, t, top, inc, nmus)
                dev = fused(pkg, k, cols, cloud, m, t, True, top, inc, nmus)
                host = fused(pkg, k, cols, cloud, m, lambda x: np.ascontiguousarray(x).copy(), False, top, inc, nmus)
                assert np.all(np.isfinite(want[0])) and np.all(want[0] > 0)
                for got in (dev, host):
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (m is not None, top, inc, nmus)


@pytest.mark.parametrize("nlay", [60, 61])
def test_fused_forward_scattering_only_and_the_scattering_effect(pkg, gpu, model, nlay):
    """g_p = 1: nothing is scattered backwards, the fluxes are those of ecckd_lw_fluxes_allsky (to the rounding bar).  With
    the clouds' own g the upward flux at the top of the cloudy columns moves by far more than that."""
    k, t = model, T(gpu)
    cols, cloud, _ = fused_case(pkg, k, 7, 37, nlay)
    forward = dict(cloud, g=np.ones_like(cloud["g"]))
    for nmus in (1, 3):
        d = distance(fused(pkg, k, cols, forward, None, t, nmus=nmus), fused(pkg, k, cols, forward, None, t, nmus=nmus, rescaled=False))
        print("nlay %d, g_p = 1, %d angles: %.3e W m-2 from lw_fluxes_allsky (bar %.1e)" % (nlay, nmus, d, BAR))
        assert d <= BAR
    half = dict(cloud, ssa=np.full_like(cloud["ssa"], 0.5))
    s, n = fused(pkg, k, cols, half, None, t, inc=False), fused(pkg, k, cols, half, None, t, inc=False, rescaled=False)
    effect = np.abs(s[0][0] - n[0][0])
    print("scattering effect on flux_up at the top, cloudy columns: %.3f ... %.3f W m-2" % (effect[cloud["cloudy"]].min(), effect[cloud["cloudy"]].max()))
    assert effect.max() > 1e3 * BAR


@pytest.mark.parametrize("nlay", [60, 61])
def test_fused_graph_capture(pkg, gpu, model, nlay):
    """After one warm-up call on the stream, a capture replays to the eager bits."""
    import torch
    k, t = model, T(gpu)
    ncol = 17
    cols, cloud, mask = fused_case(pkg, k, 3, ncol, nlay)
    want = fused(pkg, k, cols, cloud, mask, t, nmus=2)
    gc = helpers.product_gas_concs(pkg, cols, t)
    args = (t(cols["plev"]), t(cols["tlay"]), t(cols["tsfc"]), t(cols["tlev"]), gc, True, t(cols["emis"]), band_particles(pkg, cloud, t))
    kw = dict(inc_flux=t(cols["inc_flux"]), cloud_mask=to_mask(mask, t, True), rescaled=True, n_gauss_angles=2)
    fl = pkg.FluxesBroadband(*(t(np.zeros((nlay + 1, ncol))) for _ in range(2)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert k.lw_fluxes_allsky(*args, fl, **kw) == ""   # warm-up: the stream's block exists now
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert k.lw_fluxes_allsky(*args, fl, **kw) == ""
    for a in (fl.flux_up, fl.flux_dn):
        a.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(back(fl.flux_up), want[0]) and np.array_equal(back(fl.flux_dn), want[1])
    del graph
    pkg.release_scratch(0)
