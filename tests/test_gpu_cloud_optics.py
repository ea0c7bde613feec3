"""Cloud optics on the GPU: ``ecckd_cloud_optics`` / ``_f32`` against the numpy restatement of the header's definition
(tests/cloud_optics_ref.py), BIT FOR BIT -- no tolerance is involved: the build has FMA contraction off and every line
of the definition is one correctly rounded IEEE operation, in fp64 and in float.  Two-stream and one-scalar forms, both
table routes (LDS and through L2), every memory space, non-finite radii in clear cells, the all-sky chain from water
paths to fluxes, and a graph capture without a warm-up."""
import numpy as np
import pytest

import cloud_optics_ref as ref
import helpers
from rte_ecckd_amd import synthetic

pytestmark = pytest.mark.gpu
NRGH = 3
LDS_BYTES = 32768   # include/ecckd_hip.h: the tables are staged in LDS up to this size, else read through L2


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


def bits(a):
    a = back(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def load(pkg, lut, device=0):
    co = pkg.CloudOptics()
    assert co.load_lut(None, lut["radliq_lwr"], lut["radliq_upr"], 1.0, lut["radice_lwr"], lut["radice_upr"], 1.0,
                       lut["lut_extliq"], lut["lut_ssaliq"], lut["lut_asyliq"], lut["lut_extice"], lut["lut_ssaice"],
                       lut["lut_asyice"], device=device) == ""
    return co


def image_bytes(nband, nsl, nsi, two, dtype):
    return (3 if two else 2) * nband * ((nsl - 1) + (nsi - 1)) * 2 * np.dtype(dtype).itemsize


def inputs(ncol, nlay, dtype, seed=0):
    """Water paths and radii (nlay, ncol) of `dtype`.  In the order of the cells in memory (64 to a wave): the first wave
    holds both phases, the second ice only, the third liquid only, the fourth neither, then a sparse mixture.  Radii sit on
    both bounds of each table exactly in cloudy cells; one column is clear throughout; the thinnest paths (1e-300; in float
    1e-30) make tau and tssa smaller than eps, so that max(eps, .) is taken."""
    rng = np.random.default_rng(1000 * ncol + 10 * nlay + seed)
    n = ncol * nlay
    wave = np.arange(n) // 64
    u = rng.uniform(size=(4, n))
    liq = np.where(wave == 0, True, np.where((wave == 1) | (wave == 3), False, np.where(wave == 2, True, u[0] < 0.3)))
    ice = np.where(wave == 0, True, np.where((wave == 2) | (wave == 3), False, np.where(wave == 1, True, u[1] < 0.3)))
    if n == 1:
        liq[:], ice[:] = True, True
    clwp = np.where(liq, 5.0 + 195.0 * u[2], 0.0)
    ciwp = np.where(ice, 1.0 + 49.0 * u[3], 0.0)
    reliq = rng.uniform(synthetic.RADLIQ_LWR, synthetic.RADLIQ_UPR, n)
    reice = rng.uniform(synthetic.RADICE_LWR, synthetic.RADICE_UPR, n)
    arrs = [a.reshape(nlay, ncol).astype(dtype) for a in (clwp, ciwp, reliq, reice)]
    clwp, ciwp, reliq, reice = arrs
    if ncol > 2:   # a column whose cells are all clear
        clwp[:, 1] = 0
        ciwp[:, 1] = 0
    tiny = dtype(1e-300) if dtype is np.float64 else dtype(1e-30)
    lb = [dtype(v) for v in (synthetic.RADLIQ_LWR, synthetic.RADLIQ_UPR, synthetic.RADICE_LWR, synthetic.RADICE_UPR)]
    flat = [a.reshape(-1) for a in arrs]
    cl, ci = np.flatnonzero(flat[0] > 0), np.flatnonzero(flat[1] > 0)
    if cl.size:   # cloudy cells on the bounds, and a thinnest path
        flat[2][cl[0]], flat[2][cl[-1]] = lb[0], lb[1]
        flat[0][cl[cl.size // 2]] = tiny
    if ci.size:
        flat[3][ci[0]], flat[3][ci[-1]] = lb[3], lb[2]
        flat[1][ci[ci.size // 2]] = tiny
    if cl.size and ci.size and ncol * nlay > 64:   # a cell where both phases are thinnest
        flat[0][cl[1]] = tiny
        flat[1][cl[1]] = tiny
    return clwp, ciwp, reliq, reice


def run(pkg, co, arrs, nband, two, to_in, to_out, fill=-7.0):
    """The planes of one call: inputs moved by `to_in`, planes (prefilled) by `to_out`; the planes come back as numpy."""
    nlay, ncol = arrs[0].shape
    dt = arrs[0].dtype
    op = pkg.OpticalProps2str() if two else pkg.OpticalProps1scl()
    op.tau = to_out(np.full((nband, nlay, ncol), fill, dt))
    if two:
        op.ssa, op.g = to_out(np.full((nband, nlay, ncol), fill, dt)), to_out(np.full((nband, nlay, ncol), fill, dt))
    assert co.cloud_optics(*[to_in(a) for a in arrs], op) == ""
    if hasattr(op.tau, "cpu"):
        import torch
        torch.cuda.synchronize()
    return (back(op.tau), back(op.ssa), back(op.g)) if two else (back(op.tau),)


def want(arrs, lut, icergh, two, dt):
    out = ref.cloud_optics(*arrs, lut, icergh=icergh, two_stream=two, dtype=dt)
    return out if two else (out,)


# nband x nsize of the issue, plus one table set that takes the L2 route in every form and precision
TABLES = [(nband, nsize, nsize) for nband in (1, 5, 16) for nsize in (2, 20)] + [(16, 200, 150)]


@pytest.mark.parametrize("nband,nsl,nsi", TABLES)
def test_bit_equality_with_the_reference(pkg, gpu, nband, nsl, nsi):
    """Every shape, roughness, form and precision against the restatement; the inputs reach the bounds, clear columns,
    waves without one phase or without cloud, and paths thin enough for max(eps, .)."""
    t = T(gpu)
    lut = synthetic.cloud_lut(nband, nsl, nsi, NRGH)
    co = load(pkg, lut)
    routes = set()
    for dt in (np.float64, np.float32):
        for two in (True, False):
            routes.add(image_bytes(nband, nsl, nsi, two, dt) <= LDS_BYTES)
        for ncol in (1, 63, 65, 130):
            for nlay in (1, 3):
                arrs = inputs(ncol, nlay, dt)
                if ncol == 130 and nlay == 3:   # what the docstring of inputs() promises, for the largest shape
                    cl, ci = (arrs[0] > 0).reshape(-1), (arrs[1] > 0).reshape(-1)
                    w = lambda m, i: m[64 * i:64 * i + 64]
                    assert w(cl, 0).any() and w(ci, 0).any() and not w(cl, 1).any() and w(ci, 1).any()
                    assert w(cl, 2).any() and not w(ci, 2).any() and not w(cl, 3).any() and not w(ci, 3).any()
                    assert not cl.reshape(3, 130)[:, 1].any() and not ci.reshape(3, 130)[:, 1].any()
                for icergh in (1, NRGH):
                    assert co.set_ice_roughness(icergh) == ""
                    for two in (True, False):
                        got = run(pkg, co, arrs, nband, two, t, t)
                        exp = want(arrs, lut, icergh, two, dt)
                        for name, a, b in zip(("tau", "ssa", "g"), got, exp):
                            assert a.dtype == dt and same_bits(a, b), (name, dt.__name__, ncol, nlay, icergh, two,
                                                                         int((bits(a) != bits(b)).sum()))
                        if two and ncol == 130:   # max(eps, .) is taken somewhere, and the clear column is exact zeros
                            eps = np.finfo(dt).eps
                            assert ((got[0] > 0) & (got[0] < eps)).any()
                            assert all(not bits(p[:, :, 1]).any() for p in got)
    assert routes == ({False} if nsl >= 150 else {True})   # (the large set reads through L2 in every form, the others from LDS)


def test_roughness_and_route_change_the_answer(pkg, gpu):
    """The checks above would pass a kernel that ignored icergh or the table if the reference did too: the tables differ
    between roughness values, so the planes must."""
    t = T(gpu)
    lut = synthetic.cloud_lut(5, 20, 20, NRGH)
    co = load(pkg, lut)
    arrs = inputs(130, 3, np.float64)
    co.set_ice_roughness(1)
    a = run(pkg, co, arrs, 5, True, t, t)
    co.set_ice_roughness(NRGH)
    b = run(pkg, co, arrs, 5, True, t, t)
    ice_only = (arrs[1] > 0) & (arrs[0] == 0)
    assert (a[1][:, ice_only] != b[1][:, ice_only]).all() and same_bits(a[0][:, arrs[1] == 0], b[0][:, arrs[1] == 0])


@pytest.mark.parametrize("nsl,nsi", [(20, 20), (200, 150)])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_wild_radii_in_clear_cells(pkg, gpu, nsl, nsi, dt):
    """Device arrays whose CLEAR cells hold NaN, infinite or far out-of-range radii: exact zeros there, and every other
    cell keeps the bits it has without them.  (An out-of-range radius in a cloudy cell is not fed on the device: the
    clamp that makes it safe is read in the kernel, interval_of, not provoked.)"""
    t = T(gpu)
    nband = 16
    lut = synthetic.cloud_lut(nband, nsl, nsi, NRGH)
    co = load(pkg, lut)
    arrs = inputs(130, 3, dt)
    clean = run(pkg, co, arrs, nband, True, t, t)
    clwp, ciwp, reliq, reice = (a.copy() for a in arrs)
    wild = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, -4.0], dtype=dt)
    no_l, no_i = np.flatnonzero(~(clwp > 0).reshape(-1)), np.flatnonzero(~(ciwp > 0).reshape(-1))
    reliq.reshape(-1)[no_l] = wild[np.arange(no_l.size) % wild.size]
    reice.reshape(-1)[no_i] = wild[(np.arange(no_i.size) + 3) % wild.size]
    clwp.reshape(-1)[no_l[::5]] = np.nan      # NaN, negative and -0 water paths are clear too
    ciwp.reshape(-1)[no_i[::7]] = -3.0
    clwp.reshape(-1)[no_l[1::5]] = -0.0
    for two in (True, False):
        got = run(pkg, co, (clwp, ciwp, reliq, reice), nband, two, t, t)
        exp = want(arrs, lut, 1, two, dt)
        for a, b in zip(got, exp):
            assert same_bits(a, b)
        if two:
            assert all(same_bits(a, b) for a, b in zip(got, clean))
            clear = ~(arrs[0] > 0) & ~(arrs[1] > 0)
            assert clear.sum() > 64 and all(not bits(p[:, clear]).any() for p in got)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_memory_spaces_give_the_same_bits(pkg, gpu, dt):
    """Host arrays (staged), device arrays, and host inputs with device planes (ECCKD_MIXED)."""
    t, h = T(gpu), (lambda a: a.copy())
    for nband, nsl, nsi in ((5, 20, 18), (16, 200, 150)):
        lut = synthetic.cloud_lut(nband, nsl, nsi, NRGH)
        co = load(pkg, lut)
        co.set_ice_roughness(2)
        arrs = inputs(130, 3, dt, seed=5)
        for two in (True, False):
            dev, host, mixed = (run(pkg, co, arrs, nband, two, a, b) for a, b in ((t, t), (h, h), (h, t)))
            exp = want(arrs, lut, 2, two, dt)
            for d, ho, m, e in zip(dev, host, mixed, exp):
                assert same_bits(d, e) and same_bits(ho, e) and same_bits(m, e)
        op = pkg.OpticalProps1scl()
        op.tau = np.zeros((nband, 3, 130), dt)
        assert "mixing host and device" in co.cloud_optics(*[t(a) for a in arrs], op)   # device inputs, host planes: refused
        bad = arrs[2].copy()
        bad[arrs[0] > 0] = 30.0
        assert "liquid effective radius" in co.cloud_optics(arrs[0], arrs[1], bad, arrs[3], op)   # host values are checked


@pytest.fixture(scope="module")
def models(pkg, gpu):
    from conftest import LW_FSCK, LW_RRTMGP, SW_WIDE
    out = {}
    for name, path in (("fsck", LW_FSCK), ("rrtmgp", LW_RRTMGP), ("sw", SW_WIDE)):
        k = pkg.GasOpticsEcckd()
        assert k.load(path, device=0) == ""
        out[name] = k
    return out


def chain_planes(pkg, k, c0, ncol, nlay, t):
    """(device planes made by CloudOptics from synthetic.cloud_water, the reference's planes) on the bands of `k`."""
    nband = k.get_nband()
    lut = synthetic.cloud_lut(nband, 20, 18, NRGH)
    co = load(pkg, lut)
    water = synthetic.cloud_water(c0, ncol, nlay)
    assert (water[0] > 0).any() and (water[1] > 0).any()
    op = pkg.OpticalProps2str()
    assert op.alloc_2str_bands(ncol, nlay, k, like=t(np.zeros(1))) == ""
    assert co.cloud_optics(*[t(a) for a in water], op) == ""
    exp = ref.cloud_optics(*water, lut)
    assert all(same_bits(a, b) for a, b in zip((op.tau, op.ssa, op.g), exp))
    theirs = pkg.OpticalProps2str()
    theirs.tau, theirs.ssa, theirs.g = (t(a) for a in exp)
    return op, theirs


@pytest.mark.parametrize("which,nlay", [("fsck", 60), ("rrtmgp", 60), ("rrtmgp", 137)])
def test_chain_longwave(pkg, gpu, models, which, nlay):
    """cloud_optics -> lw_fluxes_allsky (no-scattering, rescaled, two-stream): fed the device planes, the fluxes equal bit
    for bit those of the same calls fed the reference's planes."""
    t = T(gpu)
    k, ncol = models[which], 70
    ours, theirs = chain_planes(pkg, k, 11, ncol, nlay, t)
    cols = synthetic.columns(11, ncol, k.get_press_min(), nlay=nlay)
    emis = t(np.repeat(cols["sfc_emis"][:, None], k.get_nband(), 1))
    for kw in (dict(), dict(rescaled=True), dict(use_2stream=True)):
        out = []
        for part in (ours, theirs):
            gc = helpers.product_gas_concs(pkg, cols, t)
            fl = pkg.FluxesBroadband(t(np.full((nlay + 1, ncol), -1.0)), t(np.full((nlay + 1, ncol), -1.0)))
            assert k.lw_fluxes_allsky(t(cols["plev"]), t(cols["tlay"]), t(cols["tsfc"]), t(cols["tlev"]), gc, True, emis, part, fl,
                                      **kw) == "", kw
            out.append((back(fl.flux_up), back(fl.flux_dn)))
        assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1]), kw
        assert np.isfinite(out[0][0]).all() and out[0][0].min() > 0
    gc = helpers.product_gas_concs(pkg, cols, t)   # the clouds are seen: the clear-sky fluxes differ
    fl = pkg.FluxesBroadband(t(np.zeros((nlay + 1, ncol))), t(np.zeros((nlay + 1, ncol))))
    assert k.lw_fluxes(t(cols["plev"]), t(cols["tlay"]), t(cols["tsfc"]), t(cols["tlev"]), gc, True, emis, fl) == ""
    assert np.abs(back(fl.flux_up)[0] - out[0][0][0]).max() > 1.0


@pytest.mark.parametrize("nlay", [60, 137])
def test_chain_shortwave(pkg, gpu, models, nlay):
    """cloud_optics -> sw_fluxes_allsky(delta_scale=1), as test_chain_longwave."""
    t = T(gpu)
    k, ncol = models["sw"], 70
    ours, theirs = chain_planes(pkg, k, 23, ncol, nlay, t)
    cols = synthetic.columns(23, ncol, k.get_press_min(), nlay=nlay, shortwave=True)
    alb = np.repeat(cols["albedo"][:, None], k.get_nband(), 1)
    out = []
    for part in (ours, theirs):
        gc = helpers.product_gas_concs(pkg, cols, t, helpers.SW_NAMES)
        fl = pkg.FluxesBroadband(*(t(np.full((nlay + 1, ncol), -1.0)) for _ in range(3)))
        assert k.sw_fluxes_allsky(t(cols["plev"]), t(cols["tlay"]), gc, True, t(cols["mu0"]), t(alb), t(alb.copy()), part, fl,
                                  delta_scale=True) == ""
        out.append([back(a) for a in (fl.flux_up, fl.flux_dn, fl.flux_dn_dir)])
    assert all(same_bits(a, b) for a, b in zip(*out))
    assert np.isfinite(out[0][1]).all() and out[0][1][-1].min() >= 0


def test_graph_capture_without_a_warm_up(pkg, gpu):
    """One call captured on a fresh stream, with a table shape no earlier call of this test has used, replays to the
    bits of the reference, twice (the call uses no scratch; the process keeps its default queue count)."""
    import torch
    t = T(gpu)
    nband, ncol, nlay = 7, 130, 3
    lut = synthetic.cloud_lut(nband, 9, 11, NRGH)
    co = load(pkg, lut)
    arrs = inputs(ncol, nlay, np.float64, seed=9)
    dev = [t(a) for a in arrs]
    op = pkg.OpticalProps2str()
    op.tau, op.ssa, op.g = (t(np.full((nband, nlay, ncol), -7.0)) for _ in range(3))
    exp = want(arrs, lut, 1, True, np.float64)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert co.cloud_optics(*dev, op) == ""
    for _ in range(2):
        for a in (op.tau, op.ssa, op.g):
            a.fill_(-7.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert all(same_bits(a, b) for a, b in zip((op.tau, op.ssa, op.g), exp))
    del graph
