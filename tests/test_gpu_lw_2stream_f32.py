"""The single-precision two-stream longwave calls on the GPU: ecckd_rte_lw_2stream_f32 (rte_lw_2stream on float32 arrays) and
the fused ecckd_lw_fluxes_allsky_2stream_f32 (GasOpticsEcckd.lw_fluxes_allsky_2stream on float32 arrays).

Equalities, no tolerance: the fused call against its composed route gas_optics (float32) -> increment[_masked] by band on
(tau, 0, 0) -> rte_lw_2stream; columns past one round of the persistent grid against the same columns in two halves; a NaN
column against the clean call; a captured graph against the eager call; the new functions on float64 arrays against the
keyword routes.

Distances from the fp64 calls on the same float32-rounded inputs: the bar is TWICE the figure of the first run on an MI355X,
recorded here; every test prints the figure it asserts on.
  solver on arrays (tau log-uniform 1e-9 .. 50, a fifth of the columns ssa = 1 with g = 0.85, the rest ssa up to 0.999999;
  37 columns, 32 and 36 g-points, nlay 1, 2, 3, 5, 60, 61, 137, both orientations): worst |float32 - float64| %(SOLVER).3e W m-2
  over all columns, %(SOLVER_SSA_LT1).3e W m-2 over the columns with ssa < 1.  The first figure is the fp64 call's error, not the
  float call's: it comes from the conservative columns (ssa = 1: k on its floor of 1e-6) in layers of tau just above RTE's
  1e-8 cutoff, where fp64 forms 1 - e2 at k tau = 1e-14 and emits up to 3e-3 pi B from a layer that conserves energy; the
  50-digit solution sides with the float cell there (tests/test_lw_2stream_f32_host.py).
  fused call on 64 synthetic columns with synthetic.clouds: 60 layers %(FUSED60).3e, 137 layers %(FUSED137).3e W m-2
  yardstick, reported and not asserted: the no-scattering ecckd_lw_fluxes_allsky_f32 from its fp64 call on those columns:
  60 layers %(YARD60).3e, 137 layers %(YARD137).3e W m-2.
"""
import numpy as np
import pytest

import helpers
import lw_2stream_ref as ref64
from rte_ecckd_amd import synthetic

pytestmark = pytest.mark.gpu
F4 = np.float32
MEASURED = dict(SOLVER=4.425e-02, SOLVER_SSA_LT1=4.053e-04, FUSED60=1.048e-04, FUSED137=2.475e-04, YARD60=6.182e-04, YARD137=9.301e-04)
__doc__ = __doc__ % MEASURED
NLAYS = (1, 2, 3, 5, 60, 61, 137)   # 1-3: the partial groups of the prefetch ring at either depth; 61, 137: the ragged last group
NCOL = 37                           # two full tiles of 16 columns and a ragged one


@pytest.fixture(autouse=True)
def default_options(pkg):
    pkg.reset_solver_options()
    pkg.set_arithmetic(pkg.FAST)
    yield
    pkg.reset_solver_options()
    pkg.set_arithmetic(pkg.FAST)


@pytest.fixture(scope="module")
def models(pkg, gpu):
    from conftest import LW_FSCK, LW_RRTMGP
    out = {}
    for name, path in (("fsck", LW_FSCK), ("rrtmgp", LW_RRTMGP)):
        k = pkg.GasOpticsEcckd()
        assert k.load(path, device=0) == ""
        out[name] = k
    assert out["fsck"].get_ngpt() == 32 and out["rrtmgp"].get_ngpt() > 32   # (g-points in the second half of the mask word)
    return out


def T(gpu, dtype=F4):
    import torch
    return lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(gpu)


def H(dtype=F4):
    return lambda a: np.ascontiguousarray(a, dtype=dtype).copy()


def back(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def to_mask(mask, to):
    if mask is None:
        return None
    probe = to(np.zeros(1))
    if hasattr(probe, "cpu"):
        import torch
        return torch.from_numpy(np.ascontiguousarray(mask).view(np.int64)).to(probe.device)
    return np.ascontiguousarray(mask).copy()


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def distance(a, b):
    return max(float(np.max(np.abs(x.astype(np.float64) - y.astype(np.float64)))) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------
# the fused call and its composed route
# ---------------------------------------------------------------------------------------------------------------------
def fused_case(pkg, k, c0, ncol, nlay):
    cols = synthetic.columns(c0, ncol, k.get_press_min(), nlay=nlay)
    cloud = synthetic.clouds(c0, ncol, nlay, k.get_nband())
    rng = np.random.default_rng(c0)
    cols["inc_flux"] = rng.uniform(0.0, 2.0, (k.get_ngpt(), ncol))
    cols["emis"] = np.repeat(cols["sfc_emis"][:, None], k.get_nband(), 1) * rng.uniform(0.95, 1.0, (ncol, k.get_nband()))
    cf = np.ascontiguousarray(synthetic.cloud_fraction(c0, ncol, nlay))
    mask = pkg.sample_cloud_mask(cf, k.get_ngpt(), seed=c0)   # (ecckd_cloud_mask_sample)
    assert mask.dtype == np.uint64
    return cols, cloud, mask


def particles(pkg, cloud, to):
    op = pkg.OpticalProps2str()
    op.tau, op.ssa, op.g = to(cloud["tau"]), to(cloud["ssa"]), to(cloud["g"])
    return op


def fused(pkg, k, cols, cloud, mask, to, top_at_1=True, inc=True, dtype=F4):
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to)
    fl = pkg.FluxesBroadband(to(np.full((nlay + 1, ncol), -1.0)), to(np.full((nlay + 1, ncol), -1.0)))
    part = particles(pkg, cloud, to)
    assert k.lw_fluxes_allsky_2stream(to(cols["plev"]), to(cols["tlay"]), to(cols["tsfc"]), to(cols["tlev"]), gc, top_at_1,
                                      to(cols["emis"]), part, fl, inc_flux=to(cols["inc_flux"]) if inc else None,
                                      cloud_mask=to_mask(mask, to)) == ""
    out = [back(fl.flux_up), back(fl.flux_dn)]
    assert all(a.dtype == dtype for a in out)
    assert np.array_equal(back(part.tau), cloud["tau"].astype(dtype)) and np.array_equal(back(part.g), cloud["g"].astype(dtype))
    return out


def composed(pkg, k, cols, cloud, mask, to, top_at_1=True, inc=True):
    """gas_optics (float32) -> increment[_masked] by band on (tau, 0, 0) -> rte_lw_2stream (float32), device tensors."""
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to)
    like = to(np.zeros(1))
    one = pkg.OpticalProps1scl(); one.alloc_1scl(ncol, nlay, k, like=like)
    src = pkg.SourceFuncLW(); src.alloc(ncol, nlay, k, like=like, separate_levels=True)
    assert k.gas_optics(None, to(cols["plev"]), to(cols["tlay"]), to(cols["tsfc"]), gc, one, src, tlev=to(cols["tlev"])) == ""
    op = pkg.OpticalProps2str(); op.alloc_2str(ncol, nlay, k, like=like)
    op.tau.copy_(one.tau); op.ssa.zero_(); op.g.zero_()
    assert op.increment(particles(pkg, cloud, to), band2gpt=k.get_band2gpt(), cloud_mask=to_mask(mask, to)) == ""
    fl = pkg.FluxesBroadband(to(np.full((nlay + 1, ncol), -2.0)), to(np.full((nlay + 1, ncol), -2.0)))
    assert pkg.rte_lw_2stream(op, top_at_1, src, to(cols["emis"]), fl, inc_flux=to(cols["inc_flux"]) if inc else None) == ""
    out = [back(fl.flux_up), back(fl.flux_dn)]
    assert all(a.dtype == F4 for a in out)
    return out


@pytest.mark.parametrize("nlay", NLAYS)
@pytest.mark.parametrize("which", ["fsck", "rrtmgp"])
def test_fused_equals_the_composed_route(pkg, gpu, models, which, nlay):
    """Bit for bit in float32: with and without a sampled mask, both orientations, with and without inc_flux, host and device
    arrays."""
    k, t = models[which], T(gpu)
    cols, cloud, mask = fused_case(pkg, k, 40 + nlay, NCOL, nlay)
    full = np.uint64(2 ** k.get_ngpt() - 1)
    if nlay >= 5:
        assert cloud["cloudy"].any() and np.any(mask != 0) and np.any(mask != full)
    for m in (None, mask):
        for top in (True, False):
            for inc in (True, False):
                want = composed(pkg, k, cols, cloud, m, t, top, inc)
                dev = fused(pkg, k, cols, cloud, m, t, top, inc)
                host = fused(pkg, k, cols, cloud, m, H(), top, inc)
                assert np.all(np.isfinite(want[0])) and np.all(want[0] > 0)
                assert same(dev, want) and same(host, want), (which, nlay, m is not None, top, inc)
    if nlay >= 5:   # the mask and the scattering are seen
        a, b = fused(pkg, k, cols, cloud, None, t), fused(pkg, k, cols, cloud, mask, t)
        assert not same(a, b)


@pytest.mark.parametrize("nlay", [60, 137])
def test_fused_float_against_the_fused_fp64_call(pkg, gpu, models, nlay):
    """64 synthetic columns with clouds on the 32-g file, float32-rounded inputs to both calls; beside it the distance of the
    no-scattering lw_fluxes_allsky (float32) from its fp64 call on the same columns -- the yardstick, reported only."""
    k = models["fsck"]
    cols, cloud, mask = fused_case(pkg, k, 500 + nlay, 64, nlay)
    r = lambda d: {n: (helpers.r32(v) if isinstance(v, np.ndarray) and v.dtype == np.float64 else v) for n, v in d.items()}
    cols, cloud = r(cols), r({n: v for n, v in cloud.items() if n in ("tau", "ssa", "g")})
    worst = 0.0
    for m in (None, mask):
        f = fused(pkg, k, cols, cloud, m, T(gpu))
        d = fused(pkg, k, cols, cloud, m, T(gpu, np.float64), dtype=np.float64)
        worst = max(worst, distance(f, d))

    def noscat(to):
        nl, nc = cols["tlay"].shape
        fl = pkg.FluxesBroadband(to(np.zeros((nl + 1, nc))), to(np.zeros((nl + 1, nc))))
        assert k.lw_fluxes_allsky(to(cols["plev"]), to(cols["tlay"]), to(cols["tsfc"]), to(cols["tlev"]),
                                  helpers.product_gas_concs(pkg, cols, to), True, to(cols["emis"]), particles(pkg, cloud, to), fl,
                                  inc_flux=to(cols["inc_flux"])) == ""
        return [back(fl.flux_up), back(fl.flux_dn)]
    yard = distance(noscat(T(gpu)), noscat(T(gpu, np.float64)))
    key = "FUSED%d" % nlay
    print("%d layers: fused two-stream float32 %.3e W m-2 from the fp64 call (bar %.3e); yardstick lw_fluxes_allsky float32 %.3e W m-2"
          % (nlay, worst, 2 * MEASURED[key], yard))
    assert worst <= 2 * MEASURED[key]


# ---------------------------------------------------------------------------------------------------------------------
# the solver on arrays
# ---------------------------------------------------------------------------------------------------------------------
def bands_of(ng, nband=2):
    return np.array([[1, 3], [4, ng]]) if nband == 2 else np.array([[1, ng]])


def random_case(ncol, nlay, ng, seed, nband=2):
    """float32-representable inputs, held in float64: tau log-uniform 1e-9 .. 50; every fifth column ssa = 1 with g = 0.85, the
    others ssa up to 0.999999 and g in -0.2 .. 0.9; sources that fall with height, every second column with a kink."""
    rng = np.random.default_rng(seed)
    shape = (ng, nlay, ncol)
    tau = 10.0 ** rng.uniform(-9.0, np.log10(50.0), shape)
    ssa = 1.0 - 10.0 ** rng.uniform(-6.0, 0.0, shape)
    g = rng.uniform(-0.2, 0.9, shape)
    ssa[:, :, ::5], g[:, :, ::5] = 1.0, 0.85
    Tl = 215.0 + np.cumsum(rng.uniform(-0.3, 80.0 / (nlay + 1), (nlay + 1, ncol)), axis=0)
    lev = rng.uniform(3.0, 5.0, (ng, 1, 1)) * (Tl[None] / 250.0) ** 4
    inc, dec = np.ascontiguousarray(lev[:, 1:]), np.ascontiguousarray(lev[:, :-1])
    if nlay > 1:
        inc[:, :-1, 1::2] *= 1.0 + rng.uniform(-0.02, 0.02, (ng, nlay - 1, ncol))[:, :, 1::2]
    a = dict(tau=tau, ssa=ssa, g=g, inc=inc, dec=dec, sfc_emis=rng.uniform(0.8, 1.0, (ncol, nband)),
             sfc_source=rng.uniform(3.0, 6.0, (ng, ncol)), inc_flux=rng.uniform(0.0, 20.0, (ng, ncol)))
    return {n: helpers.r32(v) for n, v in a.items()}


def solve(pkg, a, to, top_at_1=True, keyword=False):
    """rte_lw_2stream in the precision of `to` (keyword: rte_lw(use_2stream=True), float64); outputs pre-filled with -1."""
    ng, nlay, ncol = a["tau"].shape
    op = pkg.OpticalProps2str()
    op.tau, op.ssa, op.g = to(a["tau"]), to(a["ssa"]), to(a["g"])
    op.band2gpt = bands_of(ng, a["sfc_emis"].shape[1])
    src = pkg.SourceFuncLW()
    src.lay_source = None
    src.lev_source_inc, src.lev_source_dec, src.sfc_source = to(a["inc"]), to(a["dec"]), to(a["sfc_source"])
    fl = pkg.FluxesBroadband(to(np.full((nlay + 1, ncol), -1.0)), to(np.full((nlay + 1, ncol), -1.0)))
    inc = None if a.get("inc_flux") is None else to(a["inc_flux"])
    if keyword:
        assert pkg.rte_lw(op, top_at_1, src, to(a["sfc_emis"]), fl, use_2stream=True, inc_flux=inc) == ""
    else:
        assert pkg.rte_lw_2stream(op, top_at_1, src, to(a["sfc_emis"]), fl, inc_flux=inc) == ""
    return [back(fl.flux_up), back(fl.flux_dn)]


@pytest.mark.parametrize("nlay", NLAYS)
@pytest.mark.parametrize("ng", [32, 36])
def test_solver_against_the_fp64_solver(pkg, gpu, ng, nlay):
    """ecckd_rte_lw_2stream_f32 against ecckd_rte_lw_2stream on the same float32-rounded inputs, both orientations, host and
    device arrays (the same bits).  Two figures, each with its bar: over all columns, and over the columns with ssa < 1 -- the
    first is set by the conservative columns (see the module's docstring)."""
    a = random_case(NCOL, nlay, ng, 100 * ng + nlay)
    assert a["tau"].min() < 1e-8 or nlay < 3
    below_one = np.arange(NCOL) % 5 != 0
    worst, worst_below_one = 0.0, 0.0
    for top in (True, False):
        b = a if top else dict(ref64.flip_orientation(a))
        if nlay % 2:
            b = dict(b, inc_flux=None)
        f = solve(pkg, b, T(gpu), top)
        assert all(x.dtype == F4 for x in f) and all(np.all(np.isfinite(x)) for x in f)
        assert same(f, solve(pkg, b, H(), top))
        d = solve(pkg, b, T(gpu, np.float64), top)
        worst = max(worst, distance(f, d))
        worst_below_one = max(worst_below_one, distance([x[:, below_one] for x in f], [x[:, below_one] for x in d]))
    print("ng %d nlay %d: float32 solver %.3e W m-2 from the fp64 solver (bar %.3e); columns with ssa < 1 %.3e (bar %.3e)"
          % (ng, nlay, worst, 2 * MEASURED["SOLVER"], worst_below_one, 2 * MEASURED["SOLVER_SSA_LT1"]))
    assert worst <= 2 * MEASURED["SOLVER"]
    assert worst_below_one <= 2 * MEASURED["SOLVER_SSA_LT1"]


def columns_of(d, lo, hi, ncol):
    """The columns lo .. hi-1 of every array of the dict: the last axis, or the first of a (ncol, nband) array."""
    out = {}
    for n, v in d.items():
        if not isinstance(v, np.ndarray) or v.ndim < 1:
            out[n] = v
        elif v.ndim == 2 and v.shape[0] == ncol and v.shape[1] != ncol:
            out[n] = np.ascontiguousarray(v[lo:hi])
        else:
            out[n] = np.ascontiguousarray(v[..., lo:hi]) if v.shape[-1] == ncol else v
    return out


def test_past_one_round_plain_form(pkg, gpu):
    """16*4096 + 37 columns, 3 layers, 4 g-points in one band: the first waves walk a second tile.  Bit for bit the same
    columns in two halves (cut inside a tile)."""
    ncol, cut = 16 * 4096 + 37, 33003
    a = random_case(ncol, 3, 4, 5, nband=1)
    whole = solve(pkg, a, T(gpu))
    halves = [solve(pkg, columns_of(a, lo, hi, ncol), T(gpu)) for lo, hi in ((0, cut), (cut, ncol))]
    joined = [np.concatenate([halves[0][i], halves[1][i]], axis=1) for i in range(2)]
    assert all(np.all(np.isfinite(x)) for x in whole) and same(whole, joined)


def test_past_one_round_masked_form(pkg, gpu, oracle_mod):
    """The same through the fused call with a cloud mask, on a model of the first 4 g-points of the 32-g file in one band."""
    from conftest import LW_FSCK
    m = oracle_mod.CkdModel(LW_FSCK)
    ng = 4
    gases = [dict(name=n, code=t["code"], composite_only=int(t["composite_only"]), mole_fraction=t["mole_fraction"],
                  reference_mole_fraction=t["reference_mole_fraction"],
                  coefficient=np.ascontiguousarray((t["coefficient"] if t["code"] == 2 else t["coefficient"][0])[..., :ng]))
             for n, t in zip(m.gas, m.tables)]
    k = pkg.GasOpticsEcckd()
    assert k.init_from_tables(m.log_pressure, m.temperature, gases,
                              planck=(m.temperature_planck, np.ascontiguousarray(m.planck_function[:, :ng])),
                              bands=(np.array([[10.0, 3000.0]]), np.array([[1, ng]])), device=0) == ""
    assert k.get_ngpt() == ng and k.get_nband() == 1
    ncol, nlay = 16 * 4096 + 37, 3
    cols, cloud, mask = fused_case(pkg, k, 9, ncol, nlay)
    cloud = {n: v for n, v in cloud.items() if n in ("tau", "ssa", "g")}
    assert np.any(mask != 0) and np.any(mask != np.uint64(2 ** ng - 1))
    t = T(gpu)
    whole = fused(pkg, k, cols, cloud, mask, t)
    cut = 33003
    parts = [fused(pkg, k, columns_of(cols, lo, hi, ncol), columns_of(cloud, lo, hi, ncol), np.ascontiguousarray(mask[:, lo:hi]), t)
             for lo, hi in ((0, cut), (cut, ncol))]
    joined = [np.concatenate([parts[0][i], parts[1][i]], axis=1) for i in range(2)]
    assert all(np.all(np.isfinite(x)) for x in whole) and same(whole, joined)
    assert not same(whole, fused(pkg, k, cols, cloud, None, t))


def test_nan_stays_in_its_column(pkg, gpu):
    a = random_case(NCOL, 8, 5, 10)
    bad = dict(a, tau=a["tau"].copy())
    bad["tau"][:, :, 18] = np.nan
    others = np.arange(NCOL) != 18
    clean, dirty = solve(pkg, a, T(gpu)), solve(pkg, bad, T(gpu))
    for c, d in zip(clean, dirty):
        assert np.array_equal(c[:, others], d[:, others]) and np.all(np.isnan(d[1:, 18]))


def test_fused_graph_capture(pkg, gpu, models):
    """After one warm-up call on the stream, a single-stream capture replays to the eager bits."""
    import torch
    k, t = models["fsck"], T(gpu)
    nlay, ncol = 61, 17
    cols, cloud, mask = fused_case(pkg, k, 3, ncol, nlay)
    want = fused(pkg, k, cols, cloud, mask, t)
    gc = helpers.product_gas_concs(pkg, cols, t)
    args = (t(cols["plev"]), t(cols["tlay"]), t(cols["tsfc"]), t(cols["tlev"]), gc, True, t(cols["emis"]), particles(pkg, cloud, t))
    kw = dict(inc_flux=t(cols["inc_flux"]), cloud_mask=to_mask(mask, t))
    fl = pkg.FluxesBroadband(*(t(np.zeros((nlay + 1, ncol))) for _ in range(2)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert k.lw_fluxes_allsky_2stream(*args, fl, **kw) == ""   # warm-up: the stream's block exists now
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert k.lw_fluxes_allsky_2stream(*args, fl, **kw) == ""
    for a in (fl.flux_up, fl.flux_dn):
        a.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert same([back(fl.flux_up), back(fl.flux_dn)], want)
    del graph
    pkg.release_scratch(0)


def test_float64_arrays_give_the_keyword_routes(pkg, gpu, models):
    """rte_lw_2stream and lw_fluxes_allsky_2stream on float64 arrays: the bits of rte_lw(use_2stream=True) and
    lw_fluxes_allsky(use_2stream=True)."""
    t = T(gpu, np.float64)
    a = random_case(NCOL, 61, 5, 3)
    for top in (True, False):
        assert same(solve(pkg, a, t, top), solve(pkg, a, t, top, keyword=True))
    k = models["rrtmgp"]
    cols, cloud, mask = fused_case(pkg, k, 77, NCOL, 60)
    for m in (None, mask):
        nlay, ncol = cols["tlay"].shape
        fl = pkg.FluxesBroadband(t(np.full((nlay + 1, ncol), -1.0)), t(np.full((nlay + 1, ncol), -1.0)))
        assert k.lw_fluxes_allsky(t(cols["plev"]), t(cols["tlay"]), t(cols["tsfc"]), t(cols["tlev"]),
                                  helpers.product_gas_concs(pkg, cols, t), True, t(cols["emis"]), particles(pkg, cloud, t), fl,
                                  inc_flux=t(cols["inc_flux"]), cloud_mask=to_mask(m, t), use_2stream=True) == ""
        assert same(fused(pkg, k, cols, cloud, m, t, dtype=np.float64), [back(fl.flux_up), back(fl.flux_dn)])
