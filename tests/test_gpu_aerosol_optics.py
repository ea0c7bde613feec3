"""Aerosol optics on the GPU: ``ecckd_aerosol_optics`` / ``_f32`` against the numpy restatement of the header's definition
(tests/aerosol_optics_ref.py), BIT FOR BIT -- no tolerance is involved: the build has FMA contraction off and every line of
the definition is one correctly rounded IEEE operation, in fp64 and in float.  Two-stream and one-scalar forms, plain and
accumulating, 1 to 8 species (and the instantiation beyond 16), both table routes (LDS and through L2), a shape larger
than the resident grid, every memory space, inputs only a device array may hold, the all-sky chain to fluxes, and a
graph capture without a warm-up."""
import numpy as np
import pytest

import aerosol_optics_ref as ref
import helpers
from rte_ecckd_amd import synthetic

pytestmark = pytest.mark.gpu
LDS_BYTES = 32768   # include/ecckd_hip.h: the image is staged in LDS up to this size, else read through L2
TABLE_NAMES = ("merra_aero_bin_lims", "aero_rh", "aero_dust_tbl", "aero_salt_tbl", "aero_sulf_tbl", "aero_bcar_tbl",
               "aero_bcar_rh_tbl", "aero_ocar_tbl", "aero_ocar_rh_tbl")
RH_TYPES = np.array(ref.RH_DEPENDENT)


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
    ao = pkg.AerosolOptics()
    assert ao.load(None, *[lut[n] for n in TABLE_NAMES], device=device) == ""
    return ao


def inputs(lut, ncol, nlay, nspec, dtype, seed=0, host_safe=False):
    """Type, size, mass (nspec, nlay, ncol) and relhum (nlay, ncol) of `dtype`.  In the order of the cells in memory (64 to
    a wave): wave 0 is all one humidity-dependent type per species plane, wave 1 all dust, wave 2 the eight codes mixed,
    wave 3 none, then a sparse mixture (half the cells none).  Dust and salt sizes sit exactly on both limits of each bin
    (the upper limit of the last bin: inactive), relhum exactly on every level, above the last, equal to 1 and -- unless
    `host_safe`, since a host array with it is refused -- below the first; cells whose masses are all tiny (1e-300; in
    float 1e-30) make T and TS smaller than eps; column 1 is clear throughout."""
    rng = np.random.default_rng(1000 * ncol + 10 * nlay + nspec + seed)
    n = ncol * nlay
    cell = np.arange(n)
    wave = cell // 64
    s = np.arange(nspec)[:, None]
    lims, lev = lut["merra_aero_bin_lims"], lut["aero_rh"]
    sparse = np.where(rng.uniform(size=(nspec, n)) < 0.5, 0, rng.integers(1, 8, size=(nspec, n)))
    kind = np.where(wave == 0, RH_TYPES[(s + 1) % 4], np.where(wave == 1, 1, np.where(wave == 2, (cell + 3 * s) % 8,
                    np.where(wave == 3, 0, sparse)))) + np.zeros((nspec, n), np.int64)
    if n == 1:
        kind[:] = 2
    mass = np.where(kind > 0, 1e-6 * 100.0 ** rng.uniform(size=(nspec, n)), 0.0)
    size = lims[0, 0] * (lims[-1, 1] / lims[0, 0]) ** rng.uniform(size=(nspec, n))
    rh = rng.uniform(size=n) ** 0.7
    edge = lims.reshape(-1)[:-1] if host_safe else lims.reshape(-1)   # (the last upper limit is in no bin: refused on the host)
    if n >= 128:
        size[:, 64:64 + edge.size] = edge                  # dust on both limits of each bin (wave 1)
        salt = np.flatnonzero(kind[0] == 2)
        take = salt[:edge.size]
        size[0, take] = edge[:take.size]                   # salt too, where the first plane holds it
        special = np.concatenate([lev, [1.0, 0.995] + ([] if host_safe else [-0.25])])[:61]
        rh[3:3 + special.size] = special                   # in the wave of humidity-dependent types (cell 1 is the clear column)
        mass[:, 2] = 1e-300 if dtype is np.float64 else 1e-30
    kind, size, mass = (a.reshape(nspec, nlay, ncol) for a in (kind, size, mass))
    rh = rh.reshape(nlay, ncol)
    kind, size, mass, rh = kind.astype(np.int32), size.astype(dtype), mass.astype(dtype), rh.astype(dtype)
    if ncol > 2:   # a column whose cells are all clear
        kind[:, :, 1] = 0
        mass[:, :, 1] = 0
    return kind, size, mass, rh


def assert_the_cases_are_there(lut, arrs, dtype, host_safe=False):
    """What the docstring of inputs() promises, for the largest shape: a regenerated input cannot make the tests vacuous."""
    kind, size, mass, rh = arrs
    nspec, nlay, ncol = kind.shape
    lims, lev = lut["merra_aero_bin_lims"].astype(dtype), lut["aero_rh"].astype(dtype)
    flat = lambda a: a.reshape(a.shape[0], -1) if a.ndim == 3 else a.reshape(-1)
    k, r, m, h = flat(kind), flat(size), flat(mass), flat(rh)
    w = lambda i: slice(64 * i, 64 * i + 64)
    col = np.arange(nlay * ncol) % ncol
    live = col != 1
    assert np.isin(k[:, w(0)][:, live[w(0)]], RH_TYPES).all() and (k[:, w(1)][:, live[w(1)]] == 1).all()
    assert set(np.unique(k[0, w(2)]).tolist()) == set(range(8)) and not k[:, w(3)].any()
    active = (k >= 1) & (k <= 7) & (m > 0)
    assert not active[:, col == 1].any() and active.any(axis=1).all()
    binned = active & (k <= 2)
    for b in range(len(lims)):
        assert (binned & (r == lims[b, 0])).any()
        assert (binned & (r == lims[b, 1])).any() or (host_safe and b == len(lims) - 1)
    rh_cell = (active & np.isin(k, RH_TYPES)).any(axis=0)
    for v in lev:
        assert (rh_cell & (h == v)).any()
    assert (rh_cell & (h > lev[-1]) & (h < 1)).any() and (rh_cell & (h == 1)).any()
    assert host_safe or (rh_cell & (h < lev[0])).any()
    tiny = dtype(1e-300 if dtype is np.float64 else 1e-30)
    assert (active.any(axis=0) & ((m == tiny) | ~active).all(axis=0)).any()


def cloud_planes(nband, nlay, ncol, two, dtype):
    cl = synthetic.clouds(17, ncol, nlay, nband)
    return tuple(cl[n].astype(dtype) for n in (("tau", "ssa", "g") if two else ("tau",)))


def run(pkg, ao, arrs, nband, two, to_in, to_out, accumulate=False, fill=-7.0):
    """The planes of one call: inputs moved by `to_in`, planes by `to_out` -- prefilled with `fill`, or holding the
    synthetic clouds when the call accumulates; the planes come back as numpy."""
    nspec, nlay, ncol = arrs[0].shape
    dt = arrs[1].dtype.type
    start = cloud_planes(nband, nlay, ncol, two, dt) if accumulate else tuple(np.full((nband, nlay, ncol), fill, dt)
                                                                            for _ in range(3 if two else 1))
    op = pkg.OpticalProps2str() if two else pkg.OpticalProps1scl()
    op.tau = to_out(start[0].copy())
    if two:
        op.ssa, op.g = to_out(start[1].copy()), to_out(start[2].copy())
    assert ao.aerosol_optics(*[to_in(a) for a in arrs], op, accumulate=accumulate) == ""
    if hasattr(op.tau, "is_cuda") and op.tau.is_cuda:
        import torch
        torch.cuda.synchronize()
    return (back(op.tau), back(op.ssa), back(op.g)) if two else (back(op.tau),)


def want(lut, arrs, nband, two, dt, accumulate=False):
    nspec, nlay, ncol = arrs[0].shape
    op1 = cloud_planes(nband, nlay, ncol, two, dt) if accumulate else None
    return ref.aerosol_optics(lut, *arrs, two, dt, op1=op1)


# nband x (nbin, nrh) of the issue; (1, 5, 36) stays in LDS and (16, 5, 36) reads through L2 in every form and precision
TABLES = [(nband, nbin, nrh) for nband in (1, 5, 16) for nbin, nrh in ((1, 2), (5, 36))]


@pytest.mark.parametrize("nband,nbin,nrh", TABLES)
def test_bit_equality_with_the_reference(pkg, gpu, nband, nbin, nrh):
    """Every shape, species count, form and precision, plain and accumulating, against the restatement."""
    t = T(gpu)
    lut = synthetic.aerosol_lut(nband, nbin, nrh)
    ao = load(pkg, lut)
    routes = set()
    for dt in (np.float64, np.float32):
        for two in (True, False):
            routes.add(ref.image_bytes(nband, nbin, nrh, two, dt is np.float32) <= LDS_BYTES)
        for ncol, nlay in ((1, 1), (63, 2), (70, 3), (257, 5)):
            for nspec in (1, 3, 8):
                arrs = inputs(lut, ncol, nlay, nspec, dt)
                if ncol == 257 and nrh == 36:
                    assert_the_cases_are_there(lut, arrs, dt)
                for two in (True, False):
                    for accumulate in ((False, True) if ncol >= 70 else (False,)):
                        got = run(pkg, ao, arrs, nband, two, t, t, accumulate)
                        exp = want(lut, arrs, nband, two, dt, accumulate)
                        for name, a, b in zip(("tau", "ssa", "g"), got, exp):
                            assert a.dtype == dt and same_bits(a, b), (name, dt.__name__, ncol, nlay, nspec, two, accumulate,
                                                                         int((bits(a) != bits(b)).sum()))
                        if two and not accumulate and ncol == 257 and nrh == 36:
                            eps = np.finfo(dt).eps   # max(eps, .) is taken somewhere; the clear column is exact zeros
                            assert ((got[0] > 0) & (got[0] < eps)).any()
                            assert all(not bits(p[:, :, 1]).any() for p in got)
    if (nband, nbin, nrh) == (1, 5, 36):
        assert routes == {True}
    if (nband, nbin, nrh) == (16, 5, 36):
        assert routes == {False}
    if nrh == 2:
        assert routes == {True}


@pytest.mark.parametrize("nband,nspec", [(1, 1), (2, 3)])
def test_more_cells_than_the_resident_grid(pkg, gpu, nband, nspec):
    """The launch rule of the header: at most CUs * 8 blocks of 256 cells (fewer with more species or a large LDS image),
    the rest by grid stride.  A shape with more cells than CUs * 8 * 256 therefore strides on every route."""
    import torch
    t = T(gpu)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nlay = 4
    ncol = cus * 8 * 256 // nlay + 37
    assert -(-ncol * nlay // 256) > cus * 8
    lut = synthetic.aerosol_lut(nband, 5, 36)
    assert ref.image_bytes(nband, 5, 36, True, False) <= LDS_BYTES and 163840 // ref.image_bytes(nband, 5, 36, True, False) >= 5
    ao = load(pkg, lut)
    kind, size, mass, rh = synthetic.aerosols(3, ncol, nlay, nspec)
    got = run(pkg, ao, (kind, size, mass, rh), nband, True, t, t)
    exp = want(lut, (kind, size, mass, rh), nband, True, np.float64)
    assert all(same_bits(a, b) for a, b in zip(got, exp))
    assert (got[0][:, :, -300:] > 0).any() and (got[0][:, :, :300] > 0).any()


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_more_than_sixteen_species(pkg, gpu, dt):
    """17 species take the instantiation that re-forms the table entry per band: the same bits."""
    t = T(gpu)
    for nband, nbin, nrh in ((5, 5, 36), (2, 3, 7)):
        lut = synthetic.aerosol_lut(nband, nbin, nrh)
        ao = load(pkg, lut)
        arrs = inputs(lut, 257, 5, 17, dt)
        for two in (True, False):
            for accumulate in (False, True):
                got = run(pkg, ao, arrs, nband, two, t, t, accumulate)
                assert all(same_bits(a, b) for a, b in zip(got, want(lut, arrs, nband, two, dt, accumulate)))
    arrs16 = inputs(lut, 257, 5, 16, dt)
    got = run(pkg, ao, arrs16, nband, True, t, t)
    assert all(same_bits(a, b) for a, b in zip(got, want(lut, arrs16, nband, True, dt)))


@pytest.mark.parametrize("nband", [1, 16])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_what_only_a_device_array_may_hold(pkg, gpu, nband, dt):
    """NaN sizes, NaN relhum, types 9 and -1, negative and NaN masses in device arrays: the definition gives each a stated
    result (an inactive species; a NaN humidity takes the first level's value), the output equals the restatement bit for
    bit, and cells the values cannot reach keep the bits they have without them.  Nothing can index outside a table: the
    interval is a count, the bin comes from comparisons, an inactive species is not computed."""
    t = T(gpu)
    lut = synthetic.aerosol_lut(nband, 5, 36)
    ao = load(pkg, lut)
    arrs = inputs(lut, 257, 5, 3, dt)
    clean = run(pkg, ao, arrs, nband, True, t, t)
    kind, size, mass, rh = (a.copy() for a in arrs)
    n = kind[0].size
    k, r, m, h = kind.reshape(3, n), size.reshape(3, n), mass.reshape(3, n), rh.reshape(n)
    none = ~((k >= 1) & (m > 0))
    r[none] = np.array([np.nan, np.inf, -1.0, 1e30], dtype=dt)[np.arange(none.sum()) % 4]      # sizes of inactive species
    r[(k >= 3) & ~none] = np.nan                                                               # sizes no table looks at
    no_rh = ~(((k == 2) | (k == 3) | (k == 4) | (k == 6)) & (m > 0)).any(axis=0)
    h[no_rh] = np.array([np.nan, 5.0, -3.0], dtype=dt)[np.arange(no_rh.sum()) % 3]             # humidity nobody depends on
    idle = np.flatnonzero(none[1])
    k[1, idle[0::4]], k[1, idle[1::4]] = 9, -1                                                 # codes outside 0..7: none
    m[1, idle[0::4]], m[1, idle[1::4]] = 1e-5, 1e-5
    m[1, idle[2::4]], k[1, idle[2::4]] = -1e-5, 3                                              # negative mass: inactive
    m[1, idle[3::4]], k[1, idle[3::4]] = np.nan, 3                                             # NaN mass: inactive
    for two in (True, False):
        for accumulate in (False, True):
            got = run(pkg, ao, (kind, size, mass, rh), nband, two, t, t, accumulate)
            assert all(same_bits(a, b) for a, b in zip(got, want(lut, (kind, size, mass, rh), nband, two, dt, accumulate)))
            if two and not accumulate:
                assert all(same_bits(a, b) for a, b in zip(got, clean))
    # values with a stated result: a NaN size in a dust cell makes it inactive, a NaN humidity takes the first level
    dust = np.flatnonzero((k[0] == 1) & (m[0] > 0))
    r[0, dust[::2]] = np.nan
    wet = np.flatnonzero((k[0] == 3) & (m[0] > 0))
    h[wet[::2]] = np.nan
    got = run(pkg, ao, (kind, size, mass, rh), nband, True, t, t)
    exp = want(lut, (kind, size, mass, rh), nband, True, dt)
    assert all(same_bits(a, b) for a, b in zip(got, exp)) and not all(same_bits(a, b) for a, b in zip(got, clean))
    assert np.isfinite(got[0]).all()


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("two", [True, False])
def test_accumulate_is_the_plain_call_and_increment(pkg, gpu, dt, two):
    """accumulate onto the synthetic clouds = the plain call into fresh planes, then the package's increment on the band
    grid, bit for bit -- and both equal the restatement."""
    import torch
    t = T(gpu)
    for nband, nspec in ((5, 3), (16, 8)):
        lut = synthetic.aerosol_lut(nband, 5, 36)
        ao = load(pkg, lut)
        arrs = inputs(lut, 257, 5, nspec, dt)
        fused = run(pkg, ao, arrs, nband, two, t, t, accumulate=True)
        plain = run(pkg, ao, arrs, nband, two, t, t)
        base, aer = (pkg.OpticalProps2str() if two else pkg.OpticalProps1scl() for _ in range(2))
        for op, planes in ((base, cloud_planes(nband, 5, 257, two, dt)), (aer, plain)):
            op.tau = t(planes[0])
            if two:
                op.ssa, op.g = t(planes[1]), t(planes[2])
        assert base.increment(aer) == ""
        torch.cuda.synchronize()
        chained = (base.tau, base.ssa, base.g) if two else (base.tau,)
        exp = want(lut, arrs, nband, two, dt, accumulate=True)
        for a, b, e in zip(fused, chained, exp):
            assert same_bits(a, b) and same_bits(a, e)
        assert not same_bits(fused[0], plain[0])


def test_species_sum_is_ordered_and_one_call(pkg, gpu):
    """One nspec = 3 call is the restatement's ordered sum.  Three accumulating single-species calls compute the same
    tau (the same additions in the same order) but form ssa and g from re-multiplied ratios, so those can differ from the
    one-call result, in rounding only: a few operations of relative error eps each per increment on values below 1
    (bound: 32 eps; on these inputs the two routes happen to agree in every bit)."""
    t = T(gpu)
    nband = 5
    lut = synthetic.aerosol_lut(nband, 5, 36)
    ao = load(pkg, lut)
    kind, size, mass, rh = synthetic.aerosols(40, 257, 6, 3)
    got = run(pkg, ao, (kind, size, mass, rh), nband, True, t, t)
    assert all(same_bits(a, b) for a, b in zip(got, want(lut, (kind, size, mass, rh), nband, True, np.float64)))
    op = pkg.OpticalProps2str()
    op.tau, op.ssa, op.g = (t(np.zeros((nband, 6, 257))) for _ in range(3))
    for s in range(3):
        assert ao.aerosol_optics(t(kind[s]), t(size[s]), t(mass[s]), t(rh), op, accumulate=True) == ""
    several = (kind > 0).sum(axis=0) > 1
    assert several.any()
    assert same_bits(op.tau, got[0])
    eps = np.finfo(np.float64).eps
    for a, b in ((back(op.ssa), got[1]), (back(op.g), got[2])):
        assert np.abs(a - b).max() <= 32 * eps


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_memory_spaces_give_the_same_bits(pkg, gpu, dt):
    """numpy arrays and torch host tensors (staged), device tensors, and host inputs with device planes (ECCKD_MIXED);
    the value checks fire on host arrays and not on device arrays."""
    import torch
    t, h, th = T(gpu), (lambda a: a.copy()), (lambda a: torch.from_numpy(a.copy()))
    for nband, nbin, nrh in ((5, 5, 36), (1, 1, 2)):
        lut = synthetic.aerosol_lut(nband, nbin, nrh)
        ao = load(pkg, lut)
        arrs = inputs(lut, 257, 5, 3, dt, seed=5, host_safe=True)
        for two in (True, False):
            for accumulate in (False, True):
                exp = want(lut, arrs, nband, two, dt, accumulate)
                for to_in, to_out in ((t, t), (h, h), (th, th), (h, t), (th, t)):
                    got = run(pkg, ao, arrs, nband, two, to_in, to_out, accumulate)
                    assert all(same_bits(a, b) for a, b in zip(got, exp)), (two, accumulate)
        op = pkg.OpticalProps1scl()
        op.tau = np.zeros((nband, 5, 257), dt)
        assert "mixing host and device" in ao.aerosol_optics(*[t(a) for a in arrs], op)   # device inputs, host planes
        kind, size, mass, rh = (a.copy() for a in arrs)
        kind[0, 0, 0] = 9
        assert "type outside 0..7" in ao.aerosol_optics(kind, size, mass, rh, op)
        dev_op = pkg.OpticalProps1scl()
        dev_op.tau = t(np.zeros((nband, 5, 257), dt))
        assert "type outside 0..7" in ao.aerosol_optics(kind, size, mass, rh, dev_op)     # MIXED: host inputs are checked
        assert ao.aerosol_optics(t(kind), t(size), t(mass), t(rh), dev_op) == ""          # device arrays are not
        torch.cuda.synchronize()
        assert same_bits(dev_op.tau, ref.aerosol_optics(lut, kind, size, mass, rh, False, dt)[0])


@pytest.fixture(scope="module")
def models(pkg, gpu):
    from conftest import LW_RRTMGP, SW_WIDE
    out = {}
    for name, path in (("rrtmgp", LW_RRTMGP), ("sw", SW_WIDE)):
        k = pkg.GasOpticsEcckd()
        assert k.load(path, device=0) == ""
        out[name] = k
    return out


def chain_planes(pkg, k, c0, ncol, nlay, t):
    """(clouds + aerosols made on the device by CloudOptics-style planes and AerosolOptics(accumulate), the same from the
    restatement) on the bands of `k`."""
    nband = k.get_nband()
    lut = synthetic.aerosol_lut(nband, 5, 36)
    ao = load(pkg, lut)
    aer = synthetic.aerosols(c0, ncol, nlay, 5)
    assert (aer[0] > 0).any()
    cl = synthetic.clouds(c0, ncol, nlay, nband)
    op = pkg.OpticalProps2str()
    op.tau, op.ssa, op.g = (t(cl[n]) for n in ("tau", "ssa", "g"))
    assert ao.aerosol_optics(*[t(a) for a in aer], op, accumulate=True) == ""
    exp = ref.aerosol_optics(lut, *aer, True, op1=(cl["tau"], cl["ssa"], cl["g"]))
    assert all(same_bits(a, b) for a, b in zip((op.tau, op.ssa, op.g), exp))
    theirs = pkg.OpticalProps2str()
    theirs.tau, theirs.ssa, theirs.g = (t(a) for a in exp)
    return op, theirs


def test_chain_longwave(pkg, gpu, models):
    """aerosol_optics -> lw_fluxes_allsky (plain and rescaled) on the 16-band longwave file: fed the device planes, the
    fluxes equal bit for bit those of the same calls fed the restatement's planes."""
    t = T(gpu)
    k, ncol, nlay = models["rrtmgp"], 70, 60
    assert k.get_nband() == 16
    ours, theirs = chain_planes(pkg, k, 11, ncol, nlay, t)
    cols = synthetic.columns(11, ncol, k.get_press_min(), nlay=nlay)
    emis = t(np.repeat(cols["sfc_emis"][:, None], k.get_nband(), 1))
    for kw in (dict(), dict(rescaled=True)):
        out = []
        for part in (ours, theirs):
            gc = helpers.product_gas_concs(pkg, cols, t)
            fl = pkg.FluxesBroadband(t(np.full((nlay + 1, ncol), -1.0)), t(np.full((nlay + 1, ncol), -1.0)))
            assert k.lw_fluxes_allsky(t(cols["plev"]), t(cols["tlay"]), t(cols["tsfc"]), t(cols["tlev"]), gc, True, emis, part, fl,
                                      **kw) == "", kw
            out.append((back(fl.flux_up), back(fl.flux_dn)))
        assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1]), kw
        assert np.isfinite(out[0][0]).all() and out[0][0].min() > 0


def test_chain_shortwave(pkg, gpu, models):
    """aerosol_optics -> sw_fluxes_allsky(delta_scale=1), as test_chain_longwave."""
    t = T(gpu)
    k, ncol, nlay = models["sw"], 70, 60
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
    """One call captured on a fresh stream, with a table shape and species count no earlier call of this test has used,
    replays to the bits of the reference, twice (the call uses no scratch; the process keeps its default queue count)."""
    import torch
    t = T(gpu)
    nband, ncol, nlay, nspec = 7, 257, 5, 4
    lut = synthetic.aerosol_lut(nband, 4, 9)
    ao = load(pkg, lut)
    arrs = inputs(lut, ncol, nlay, nspec, np.float64, seed=9)
    dev = [t(a) for a in arrs]
    op = pkg.OpticalProps2str()
    op.tau, op.ssa, op.g = (t(np.full((nband, nlay, ncol), -7.0)) for _ in range(3))
    exp = want(lut, arrs, nband, True, np.float64)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert ao.aerosol_optics(*dev, op) == ""
    for _ in range(2):
        for a in (op.tau, op.ssa, op.g):
            a.fill_(-7.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert all(same_bits(a, b) for a, b in zip((op.tau, op.ssa, op.g), exp))
    del graph
