"""The two-stream longwave solver on the GPU: ecckd_rte_lw_2stream (rte_lw(use_2stream=True)), the spectral
ecckd_lw_solver_2stream_gpt / lw_solver_2stream, and the fused ecckd_lw_fluxes_allsky_2stream.

Yardsticks: the multi-digit truth in tests/golden/lw_2stream_truth.npz within each set's recorded bar (4 x the numpy
restatement's own distance from it; tests/test_lw_2stream_host.py ties the restatement to the truth on the CPU), the
restatement itself at helpers.FLUX_ATOL on shapes beyond the fixture, and -- for the fused call -- bit equality with the
composed route gas_optics_tau, planck_sources, increment by band on (tau, 0, 0), rte_lw(use_2stream=True).
Every test prints the figure it asserts on.

Measured on an MI355X, next to the bars (which come from the fixture's metadata and from helpers.FLUX_ATOL, not from these
figures): cloudy sets 7e-15 ... 3.6e-14 W m-2 (bars 6.7e-14 ... 1.4e-13), thin 2.7e-10 (1.1e-9), near-conservative 2.8e-9
(1.1e-8), cutoff 1.4e-14 (1e-9) -- the same in both arithmetic modes and orientations to the digits shown; shapes beyond the
fixture at most 2.7e-13 from the restatement (27 g-points), per g-point at most 9e-15; every bit-for-bit case holds as an
equality; the scattering effect at the top of the cloudy columns is 1.2 ... 9.6 W m-2."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import helpers
import lw_2stream_ref as ref
import truth_fixture
from helpers import FLUX_ATOL
from rte_ecckd_amd import synthetic

pytestmark = pytest.mark.gpu
SETS = ("cloudy_n1", "cloudy_n2", "cloudy_n8", "cloudy_n61", "thin_n8", "near_conservative_n8", "cutoff_n8")


@pytest.fixture(autouse=True)
def default_options(pkg):
    pkg.reset_solver_options()
    pkg.set_arithmetic(pkg.FAST)
    yield
    pkg.reset_solver_options()
    pkg.set_arithmetic(pkg.FAST)


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(helpers.GOLDEN, "lw_2stream_truth.npz"))
    arrays = {k: z[k] for k in z.files}
    meta = json.loads(str(arrays.pop("meta")))
    for a in arrays.values():
        a.setflags(write=False)
    return arrays, meta["sets"]


def T(gpu):
    import torch
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def back(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def solve(pkg, a, band2gpt, to, top_at_1=True, lay="nan"):
    """rte_lw(use_2stream=True) on the inputs dict `a` (tau, ssa, g, inc, dec, sfc_emis (ncol, nband), sfc_source, inc_flux or
    None); outputs pre-filled with -1.  lay: "nan" (an array of NaNs: it is never read) or None (NULL)."""
    ng, nlay, ncol = a["tau"].shape
    op = pkg.OpticalProps2str()
    op.tau, op.ssa, op.g = to(a["tau"]), to(a["ssa"]), to(a["g"])
    op.band2gpt = np.asarray(band2gpt)
    src = pkg.SourceFuncLW()
    src.lay_source = None if lay is None else to(np.full((ng, nlay, ncol), np.nan))
    src.lev_source_inc, src.lev_source_dec, src.sfc_source = to(a["inc"]), to(a["dec"]), to(a["sfc_source"])
    fl = pkg.FluxesBroadband(to(np.full((nlay + 1, ncol), -1.0)), to(np.full((nlay + 1, ncol), -1.0)))
    inc = a.get("inc_flux")
    assert pkg.rte_lw(op, top_at_1, src, to(a["sfc_emis"]), fl, use_2stream=True, inc_flux=None if inc is None else to(inc)) == ""
    return back(fl.flux_up), back(fl.flux_dn)


def distance(got, want):
    return max(float(np.max(np.abs(got[0] - want[0]))), float(np.max(np.abs(got[1] - want[1]))))


@pytest.mark.parametrize("name", SETS)
def test_fixture_sets(pkg, gpu, fixture, name):
    """Every set, both orientations, both arithmetic modes, within the set's bar."""
    arrays, meta = fixture
    pre = name + "."
    a = {k[len(pre):]: v for k, v in arrays.items() if k.startswith(pre)}
    bar = meta[name]["bar"]
    worst = 0.0
    for mode in (pkg.FAST, pkg.REFERENCE_ORDER):
        pkg.set_arithmetic(mode)
        for top in (True, False):
            b = a if top else ref.flip_orientation(a)
            up, dn = solve(pkg, b, truth_fixture.BAND2GPT, T(gpu), top)
            if not top:
                up, dn = up[::-1], dn[::-1]
            d = distance((up, dn), (a["up"], a["dn"]))
            print("%s mode %d top_at_1 %d: %.3e W m-2 (bar %.3e)" % (name, mode, top, d, bar))
            worst = max(worst, d)
    assert worst <= bar


def random_case(ncol, nlay, ng, nband, seed):
    rng = np.random.default_rng(seed)
    shape = (ng, nlay, ncol)
    tau = 10.0 ** rng.uniform(-2.0, np.log10(30.0), shape)
    if nlay > 1:
        tau[rng.uniform(size=shape) < 0.05] = 0.0
    ssa, g = rng.uniform(0.0, 0.999, shape), rng.uniform(-0.2, 0.9, shape)
    ssa[:, :, ::5] = 0.0
    Tl = 215.0 + np.cumsum(rng.uniform(-0.3, 80.0 / (nlay + 1), (nlay + 1, ncol)), axis=0)
    lev = rng.uniform(3.0, 5.0, (ng, 1, 1)) * (Tl[None] / 250.0) ** 4
    inc, dec = np.ascontiguousarray(lev[:, 1:]), np.ascontiguousarray(lev[:, :-1])
    if nlay > 1:
        inc[:, :-1, 1::2] *= 1.0 + rng.uniform(-0.02, 0.02, (ng, nlay - 1, ncol))[:, :, 1::2]
    inc_flux = rng.uniform(0.0, 20.0, (ng, ncol))
    return dict(tau=tau, ssa=ssa, g=g, inc=inc, dec=dec, sfc_emis=rng.uniform(0.8, 1.0, (ncol, nband)),
                sfc_source=rng.uniform(3.0, 6.0, (ng, ncol)), inc_flux=inc_flux)


def bands_of(ng, kind):
    return np.array([[1, 3], [4, 5]]) if kind == "two" else np.array([[i, i] for i in range(1, ng + 1)])


def per_gpt(emis, band2gpt, ng):
    out = np.empty((ng, emis.shape[0]))
    for b, (lo, hi) in enumerate(band2gpt):
        out[lo - 1:hi] = emis[:, b][None]
    return out


# a partial tile (1, 15, 17, 37), a partial g-point group (3, 5, 27 of 4 lanes), fewer layers than the prefetch depth
# (1, 2), the partial last prefetch group (4, 61, 137), the ring at depth (137), inc_flux None and given
SHAPES = [(1, 1, 3, "each"), (15, 2, 5, "two"), (16, 3, 27, "each"), (17, 4, 5, "two"), (37, 60, 3, "each"), (37, 61, 27, "each"),
          (17, 137, 5, "two"), (1, 61, 5, "each"), (16, 137, 3, "each"), (15, 60, 27, "each"), (37, 3, 5, "two"), (17, 2, 27, "each")]


@pytest.mark.parametrize("ncol,nlay,ng,kind", SHAPES)
def test_shapes_beyond_the_fixture(pkg, gpu, ncol, nlay, ng, kind):
    """Against the numpy restatement, both orientations and arithmetic modes, bar FLUX_ATOL."""
    b2g = bands_of(ng, kind)
    a = random_case(ncol, nlay, ng, b2g.shape[0], 1000 * ncol + 10 * nlay + ng)
    if (ncol + nlay) % 2:
        a["inc_flux"] = None
    emis = per_gpt(a["sfc_emis"], b2g, ng)
    worst = 0.0
    for top in (True, False):
        b = a if top else ref.flip_orientation(a)
        ru, rd = ref.restate(b["tau"], b["ssa"], b["g"], b["inc"], b["dec"], emis, b["sfc_source"], b["inc_flux"], top)
        want = (ref.broadband(ru), ref.broadband(rd))
        for mode in (pkg.FAST, pkg.REFERENCE_ORDER):
            pkg.set_arithmetic(mode)
            worst = max(worst, distance(solve(pkg, b, b2g, T(gpu), top), want))
    print("ncol %d nlay %d ng %d: %.3e W m-2 from the restatement (bar %.1e)" % (ncol, nlay, ng, worst, FLUX_ATOL))
    assert worst <= FLUX_ATOL


def test_more_tiles_than_one_round(pkg, gpu):
    """More tiles than the persistent grid has waves (4096 x 16 columns): the first waves walk a second tile."""
    ncol, nlay, ng = 4096 * 16 + 37, 3, 3
    b2g = bands_of(ng, "each")
    a = random_case(ncol, nlay, ng, ng, 77)
    ru, rd = ref.restate(a["tau"], a["ssa"], a["g"], a["inc"], a["dec"], per_gpt(a["sfc_emis"], b2g, ng), a["sfc_source"], a["inc_flux"])
    d = distance(solve(pkg, a, b2g, T(gpu)), (ref.broadband(ru), ref.broadband(rd)))
    print("%d columns: %.3e W m-2 from the restatement" % (ncol, d))
    assert d <= FLUX_ATOL


def gpt_call(pkg, a, emis_gpt, space, to, top_at_1=True):
    ng, nlay, ncol = a["tau"].shape
    up, dn = to(np.full((ng, nlay + 1, ncol), -1.0)), to(np.full((ng, nlay + 1, ncol), -1.0))
    P = lambda x: None if x is None else (C.c_void_p(x.data_ptr()) if hasattr(x, "data_ptr") else C.c_void_p(x.ctypes.data))
    keep = [to(a[k]) for k in ("tau", "ssa", "g", "inc", "dec")] + [to(emis_gpt), to(a["sfc_source"]), to(a["inc_flux"])]
    stream = None
    if space == pkg.DEVICE:
        import torch
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = pkg.lib().ecckd_lw_solver_2stream_gpt(0, ncol, nlay, ng, int(top_at_1), P(keep[0]), P(keep[1]), P(keep[2]), None, P(keep[3]),
                                               P(keep[4]), P(keep[5]), P(keep[6]), P(keep[7]), P(up), P(dn), space, stream)
    assert rc == 0, pkg.last_error()
    if space == pkg.DEVICE:
        import torch
        torch.cuda.synchronize()
    return back(up), back(dn)


@pytest.mark.parametrize("ncol,nlay,ng", [(37, 8, 5), (300, 61, 3), (1, 1, 27)])
def test_spectral_route(pkg, gpu, ncol, nlay, ng):
    """ecckd_lw_solver_2stream_gpt equals the restatement per g-point (FLUX_ATOL), its g-point sum equals the broadband call
    (FLUX_ATOL), host and device arrays give the same bits, and lw_solver_2stream of librte_kernels_hip gives the bits of the
    _gpt call with the incident flux taken from flux_dn(:, top, :)."""
    b2g = bands_of(ng, "each")
    a = random_case(ncol, nlay, ng, ng, 31 * ncol + nlay)
    emis = per_gpt(a["sfc_emis"], b2g, ng)
    K = C.CDLL(pkg.RTE_KERNELS_LIB)
    for top in (True, False):
        b = a if top else ref.flip_orientation(a)
        want = ref.restate(b["tau"], b["ssa"], b["g"], b["inc"], b["dec"], emis, b["sfc_source"], b["inc_flux"], top)
        dev = gpt_call(pkg, b, emis, pkg.DEVICE, T(gpu), top)
        host = gpt_call(pkg, b, emis, pkg.HOST, lambda x: np.ascontiguousarray(x), top)
        assert np.array_equal(dev[0], host[0]) and np.array_equal(dev[1], host[1])
        d = distance(dev, want)
        pkg.set_arithmetic(pkg.REFERENCE_ORDER)
        bb = solve(pkg, b, b2g, T(gpu), top)
        pkg.set_arithmetic(pkg.FAST)
        d2 = distance((ref.broadband(dev[0]), ref.broadband(dev[1])), bb)
        print("spectral ncol %d nlay %d ng %d top %d: %.3e from the restatement, sum %.3e from the broadband call" % (ncol, nlay, ng, top, d, d2))
        assert d <= FLUX_ATOL and d2 <= FLUX_ATOL
        # RTE's bind(C) name: by reference, flux_dn(:, top, :) holds the incident flux on entry
        up, dn = np.full((ng, nlay + 1, ncol), -1.0), np.full((ng, nlay + 1, ncol), -1.0)
        dn[:, 0 if top else nlay] = b["inc_flux"]
        P = lambda x: C.c_void_p(x.ctypes.data)
        I = lambda v: C.byref(C.c_int(v))
        arrs = [np.ascontiguousarray(b[k]) for k in ("tau", "ssa", "g")] + [np.full(b["tau"].shape, np.nan)] + \
               [np.ascontiguousarray(b[k]) for k in ("inc", "dec")] + [emis, np.ascontiguousarray(b["sfc_source"])]
        K.lw_solver_2stream.restype = None
        K.lw_solver_2stream(I(ncol), I(nlay), I(ng), C.byref(C.c_bool(top)), *[P(x) for x in arrs], P(up), P(dn))
        assert np.array_equal(up, dev[0]) and np.array_equal(dn, dev[1])


def test_host_arrays_and_null_lay_source(pkg, gpu):
    a = random_case(37, 61, 5, 2, 9)
    b2g = bands_of(5, "two")
    for mode in (pkg.FAST, pkg.REFERENCE_ORDER):
        pkg.set_arithmetic(mode)
        dev = solve(pkg, a, b2g, T(gpu))
        host = solve(pkg, a, b2g, lambda x: np.ascontiguousarray(x).copy())
        null = solve(pkg, a, b2g, T(gpu), lay=None)
        assert np.array_equal(dev[0], host[0]) and np.array_equal(dev[1], host[1])
        assert np.array_equal(dev[0], null[0]) and np.array_equal(dev[1], null[1])
        assert np.all(np.isfinite(dev[0])) and np.all(dev[1] >= 0)


def test_nan_stays_in_its_column(pkg, gpu):
    a = random_case(37, 8, 5, 2, 10)
    b2g = bands_of(5, "two")
    bad = dict(a, tau=a["tau"].copy())
    bad["tau"][:, :, 18] = np.nan
    others = np.arange(37) != 18
    for mode in (pkg.FAST, pkg.REFERENCE_ORDER):
        pkg.set_arithmetic(mode)
        clean, dirty = solve(pkg, a, b2g, T(gpu)), solve(pkg, bad, b2g, T(gpu))
        for c, d in zip(clean, dirty):
            assert np.array_equal(c[:, others], d[:, others]) and np.all(np.isnan(d[1:, 18]))


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
    assert mask.dtype == np.uint64
    return cols, cloud, mask


def band_particles(pkg, cloud, to):
    op = pkg.OpticalProps2str()
    op.tau, op.ssa, op.g = to(cloud["tau"].copy()), to(cloud["ssa"].copy()), to(cloud["g"].copy())
    return op


def to_mask(mask, to, device):
    if mask is None:
        return None
    return to(mask.view(np.int64)) if device else mask.copy()


def fused(pkg, k, cols, cloud, mask, to, device=True, top_at_1=True, inc=True, two_stream=True):
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to)
    fl = pkg.FluxesBroadband(to(np.full((nlay + 1, ncol), -1.0)), to(np.full((nlay + 1, ncol), -1.0)))
    kw = dict(use_2stream=True) if two_stream else {}
    assert k.lw_fluxes_allsky(to(cols["plev"]), to(cols["tlay"]), to(cols["tsfc"]), to(cols["tlev"]), gc, top_at_1, to(cols["emis"]),
                              band_particles(pkg, cloud, to), fl, inc_flux=to(cols["inc_flux"]) if inc else None,
                              cloud_mask=to_mask(mask, to, device), **kw) == ""
    return back(fl.flux_up), back(fl.flux_dn)


def composed(pkg, k, cols, cloud, mask, to, top_at_1=True, inc=True):
    """gas_optics_tau -> planck_sources -> increment[_masked] by band on (tau, 0, 0) -> rte_lw(use_2stream=True)."""
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
    assert pkg.rte_lw(op, top_at_1, src, to(cols["emis"]), fl, use_2stream=True, inc_flux=to(cols["inc_flux"]) if inc else None) == ""
    torch.cuda.synchronize()
    return back(fl.flux_up), back(fl.flux_dn)


@pytest.mark.parametrize("nlay,ncol", [(60, 37), (61, 17), (8, 16)])
def test_fused_equals_the_composed_route(pkg, gpu, model, nlay, ncol):
    """Bit for bit: with and without a sampled mask, both orientations, both memory spaces, with and without inc_flux."""
    k, t = model, T(gpu)
    cols, cloud, mask = fused_case(pkg, k, 40 + nlay, ncol, nlay)
    assert cloud["cloudy"].any() and np.any(mask != 0) and np.any(mask != np.uint64(2 ** k.get_ngpt() - 1))
    for m in (None, mask):
        for top in (True, False):
            for inc in (True, False):
                want = composed(pkg, k, cols, cloud, m, t, top, inc)
                dev = fused(pkg, k, cols, cloud, m, t, True, top, inc)
                host = fused(pkg, k, cols, cloud, m, lambda x: np.ascontiguousarray(x).copy(), False, top, inc)
                assert np.all(np.isfinite(want[0])) and np.all(want[0] > 0)
                for got in (dev, host):
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (m is not None, top, inc)


def test_fused_g_without_scattering_and_the_scattering_effect(pkg, gpu, model):
    k, t = model, T(gpu)
    nlay, ncol = 60, 37
    cols, cloud, _ = fused_case(pkg, k, 7, ncol, nlay)
    ones = np.full((nlay, ncol), np.uint64(2 ** k.get_ngpt() - 1), dtype=np.uint64)
    # ssa_p = 0: nothing scatters, g_p cannot matter
    absorbing = dict(cloud, ssa=np.zeros_like(cloud["ssa"]))
    a = fused(pkg, k, cols, absorbing, ones, t)
    b = fused(pkg, k, cols, dict(absorbing, g=np.zeros_like(cloud["g"])), ones, t)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # ssa_p = 0.5: the upward flux at the top differs from the no-scattering all-sky call's
    half = dict(cloud, ssa=np.full_like(cloud["ssa"], 0.5))
    s = fused(pkg, k, cols, half, None, t, inc=False)
    n = fused(pkg, k, cols, half, None, t, inc=False, two_stream=False)
    effect = np.abs(s[0][0] - n[0][0])
    print("scattering effect on flux_up at the top, cloudy columns: %.3f ... %.3f W m-2" % (effect[cloud["cloudy"]].min(), effect[cloud["cloudy"]].max()))
    assert effect.max() > FLUX_ATOL


def test_fused_graph_capture(pkg, gpu, model):
    """After one warm-up call on the stream, a capture replays to the eager bits."""
    import torch
    k, t = model, T(gpu)
    nlay, ncol = 61, 17
    cols, cloud, mask = fused_case(pkg, k, 3, ncol, nlay)
    want = fused(pkg, k, cols, cloud, mask, t)
    gc = helpers.product_gas_concs(pkg, cols, t)
    args = (t(cols["plev"]), t(cols["tlay"]), t(cols["tsfc"]), t(cols["tlev"]), gc, True, t(cols["emis"]), band_particles(pkg, cloud, t))
    kw = dict(inc_flux=t(cols["inc_flux"]), cloud_mask=to_mask(mask, t, True), use_2stream=True)
    fl = pkg.FluxesBroadband(*(t(np.zeros((nlay + 1, ncol))) for _ in range(2)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert k.lw_fluxes_allsky(*args, fl, **kw) == ""   # warm-up: the stream's block exists now
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert k.lw_fluxes_allsky(*args, fl, **kw) == ""
    for _ in range(2):
        for a in (fl.flux_up, fl.flux_dn):
            a.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(back(fl.flux_up), want[0]) and np.array_equal(back(fl.flux_dn), want[1])
    del graph
    pkg.release_scratch(0)
