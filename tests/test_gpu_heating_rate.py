"""Heating rates on the GPU: ``ecckd_heating_rate`` / ``_f32`` against the numpy restatement (tests/heating_rate_ref.py),
bit for bit, over the column counts around a wave and a block, shallow and deep grids, one and many outer planes, both
precisions, both cp forms, the three memory spaces and a side stream; zero thickness and NaN confined to their cells; an
array past 2^31 elements; the real chains (lw_fluxes, sw_fluxes_allsky, rte_lw by band) in both orientations; the class
conveniences; graph capture without a warm-up."""
import numpy as np
import pytest

import helpers
import heating_rate_ref as ref
from conftest import LW_RRTMGP, SW_WIDE
from rte_ecckd_amd import synthetic

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]


def T(gpu):
    import torch
    return lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def back(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def same_bits(got, want):
    got, want = back(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(ref.bits(got), ref.bits(want))


def same_bits_nan_aware(got, want):
    """A NaN where `want` has one, the bits of `want` everywhere else (IEEE 754 leaves the sign and payload of a NaN result
    to the implementation: the device's subtraction is an addition of the negated operand, which flips the sign of a NaN
    subtrahend; the host's does not)."""
    got, want = back(got), np.asarray(want)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and same_bits(got[~nan], want[~nan])


# every value of ncol {1, 63, 64, 65, 257}, nlay {1, 2, 60, 137} and nouter {1 (rank 2 and rank 3), 3, 16}; each case runs
# in both precisions and both cp forms
SHAPES = [(1, 1, 1), (63, 2, 3), (64, 60, 16), (65, 137, None), (257, 137, 3), (257, 60, 16), (64, 1, None), (1, 60, 3)]


@pytest.mark.parametrize("with_cp", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ncol,nlay,nouter", SHAPES)
def test_device_arrays_equal_the_restatement_bit_for_bit(pkg, gpu, ncol, nlay, nouter, dtype, with_cp):
    t = T(gpu)
    fu, fd, plev, cp = ref.inputs(ncol * 1000 + nlay, ncol, nlay, nouter, dtype, with_cp)
    want = ref.heating_rate(fu, fd, plev, cp)
    err, out = pkg.heating_rate(t(fu), t(fd), t(plev), cp=t(cp))
    assert err == ""
    assert out.is_cuda and same_bits(out, want)
    assert np.isfinite(want).all() and (want != 0).any()
    # other constants, into a given array
    given = t(np.full(want.shape, -7.0, dtype))
    err, out = pkg.heating_rate(t(fu), t(fd), t(plev), heating_rate=given, cp=t(cp), grav=3.71, cp_dry=735.0)
    assert err == "" and out is given
    assert same_bits(given, ref.heating_rate(fu, fd, plev, cp, grav=3.71, cp_dry=735.0))


@pytest.mark.parametrize("with_cp", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("space", ["host", "mixed"])
def test_host_and_mixed_arrays(pkg, gpu, space, dtype, with_cp):
    ncol, nlay, nouter = 65, 60, 3
    fu, fd, plev, cp = ref.inputs(77, ncol, nlay, nouter, dtype, with_cp)
    want = ref.heating_rate(fu, fd, plev, cp)
    if space == "host":
        err, out = pkg.heating_rate(fu, fd, plev, cp=cp)
        assert err == "" and isinstance(out, np.ndarray)
    else:
        given = T(gpu)(np.full(want.shape, -7.0, dtype))
        err, out = pkg.heating_rate(fu, fd, plev, heating_rate=given, cp=cp)
        assert err == "" and out is given
    assert same_bits(out, want)
    # device inputs with a host result are not a memory space of the library
    err, _ = pkg.heating_rate(T(gpu)(fu), T(gpu)(fd), T(gpu)(plev), heating_rate=np.zeros(want.shape, dtype))
    assert "mixing host and device arrays" in err


@pytest.mark.parametrize("dtype", DTYPES)
def test_side_stream(pkg, gpu, dtype):
    import torch
    t = T(gpu)
    fu, fd, plev, cp = ref.inputs(5, 257, 60, 3, dtype, True)
    want = ref.heating_rate(fu, fd, plev, cp)
    dev = [t(a) for a in (fu, fd, plev, cp)]
    out = t(np.full(want.shape, -7.0, dtype))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        err, _ = pkg.heating_rate(dev[0], dev[1], dev[2], heating_rate=out, cp=dev[3])
    assert err == ""
    side.synchronize()
    assert same_bits(out, want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_thickness_and_nan_stay_in_their_cell(pkg, gpu, dtype):
    t = T(gpu)
    fu, fd, plev, _ = ref.inputs(6, 130, 9, 3, dtype, False)
    clean = ref.heating_rate(fu, fd, plev)
    plev[4, 70] = plev[3, 70]    # dp = 0 in layer 3 of column 70 (every plane)
    fu[1, 6, 2] = np.nan         # a NaN level in plane 1: layers 5 and 6 of column 2
    want = ref.heating_rate(fu, fd, plev)
    err, out = pkg.heating_rate(t(fu), t(fd), t(plev))
    assert err == ""
    out = back(out)
    assert np.isnan(want).sum() == 2 and same_bits_nan_aware(out, want)   # (the infinities are compared by their bits)
    assert np.isinf(out[:, 3, 70]).all() and np.isnan(out[1, 5:7, 2]).all()
    touched = np.zeros(out.shape, bool)
    touched[:, 3:5, 70] = touched[1, 5:7, 2] = True
    assert np.isfinite(out[~touched]).all() and np.array_equal(ref.bits(out)[~touched], ref.bits(clean)[~touched])


def test_offsets_past_two_to_the_31(pkg, gpu):
    """ncol*(nlay+1)*nouter = 65537*129*260 = 2.2e9 elements: the planes whose offsets pass 2^31 hold the restatement's
    bits (float32; three planes are checked on the host, the first, the one that straddles 2^31 and the last)."""
    import torch
    ncol, nlay, nouter = 65537, 128, 260
    assert ncol * (nlay + 1) * nouter > 2 ** 31 and 254 * ncol * (nlay + 1) < 2 ** 31 < 255 * ncol * (nlay + 1)
    gen = torch.Generator(device=gpu).manual_seed(3)
    fu = torch.rand((nouter, nlay + 1, ncol), dtype=torch.float32, device=gpu, generator=gen) * 500.0
    fd = torch.rand((nouter, nlay + 1, ncol), dtype=torch.float32, device=gpu, generator=gen) * 500.0
    plev = ref.inputs(8, ncol, nlay, None, np.float32, False)[2]
    out = torch.full((nouter, nlay, ncol), -7.0, dtype=torch.float32, device=gpu)
    err, _ = pkg.heating_rate(fu, fd, T(gpu)(plev), heating_rate=out)
    assert err == ""
    for plane in (0, 254, nouter - 1):
        assert same_bits(out[plane], ref.heating_rate(back(fu[plane]), back(fd[plane]), plev)), plane
    assert bool((out != -7.0).all())


# ---- the real chains ----
@pytest.fixture(scope="module")
def models(pkg, gpu):
    out = {}
    for name, path in (("lw", LW_RRTMGP), ("sw", SW_WIDE)):
        k = pkg.GasOpticsEcckd()
        assert k.load(path, device=0) == ""
        out[name] = k
    return out


def oriented(cols, top_at_1, cloud=None):
    """The columns (and band planes) as they are, or with the vertical axis of every profile reversed."""
    cols = dict(cols)
    if not top_at_1:
        for n in ("plev", "tlay", "tlev", "h2o", "o3"):
            cols[n] = np.ascontiguousarray(cols[n][::-1])
        if cloud is not None:
            cloud = {n: np.ascontiguousarray(cloud[n][:, ::-1]) for n in ("tau", "ssa", "g")}
    return cols, cloud


def flip_bound(fluxes_a, fluxes_b, plev, hr_a, hr_b):
    """How far the heating rates of two runs may sit apart, given how far their fluxes do.  With w = grav / (cp_dry |dp|):
    the flux differences of the four levels a cell reads, carried through the expression, (sum |d flux|) w; and per side
    the roundings, with u the unit round-off: du and dd round by u |du| and u |dd| (absolute: dnet may cancel), which w
    carries, and dnet, dp, the two products and the quotient by 5 u of the result.  Nothing else enters."""
    u = np.finfo(np.float64).eps / 2
    w = ref.GRAV / (ref.CP_DRY * np.abs(np.diff(plev, axis=0)))
    moved = sum(np.abs(a - b) for a, b in zip(fluxes_a, fluxes_b))             # (.., nlay+1, ncol): |d flux_up| + |d flux_dn|
    steps = sum(np.abs(np.diff(a, axis=-2)) for a in tuple(fluxes_a) + tuple(fluxes_b))   # |du| + |dd| of either side
    return (moved[..., 1:, :] + moved[..., :-1, :]) * w + u * (steps * w + 5 * (np.abs(hr_a) + np.abs(hr_b)))


def check_both_orientations(pkg, t, run, plev):
    """run(top_at_1) -> (flux_up, flux_dn, heating_rate) as numpy arrays in the run's own orientation (the vertical axis
    second to last).  Each run's heating rate is the restatement of its own fluxes bit for bit.  Flipped onto each other
    the two agree within what their fluxes differ by (flip_bound) -- which is the flux call's own reproducibility under the
    flip and can be large: gas optics, like the reference's, takes plev(j+1) - plev(j) for the layer's mass, so a bottom-up
    call sees other, negative optical depths (the shortwave then returns NaN, which the heating rate carries: there only
    the NaN itself is compared and no bound exists).  And with the fluxes held fixed the orientation does not matter at
    all: the call on the top-down run's fluxes, flipped, gives that run's heating rate, flipped, bit for bit."""
    (ua, da, ha), (ub, db, hb) = run(True), run(False)
    pb = np.ascontiguousarray(plev[::-1])
    assert same_bits(ha, ref.heating_rate(ua, da, plev)) and same_bits_nan_aware(hb, ref.heating_rate(ub, db, pb))
    flip = lambda a: np.ascontiguousarray(a[..., ::-1, :])
    bound = flip_bound((ua, da), (flip(ub), flip(db)), plev, ha, flip(hb))
    diff = np.abs(flip(hb) - ha)
    ok = np.isfinite(bound)
    print("heating rates of the two orientations: worst |difference| / bound = %.3f over the %d of %d cells with a finite bound"
          % (float(np.max(diff[ok & (bound > 0)] / bound[ok & (bound > 0)], initial=0.0)), ok.sum(), ok.size))
    assert np.isfinite(ha).all() and (ha != 0).any() and (diff[ok] <= bound[ok]).all()
    err, flipped = pkg.heating_rate(t(flip(ua)), t(flip(da)), t(pb))
    assert err == "" and same_bits(flipped, flip(ha))


def test_chain_lw_fluxes_both_orientations(pkg, gpu, models):
    t = T(gpu)
    k, ncol, nlay = models["lw"], 70, 60
    base = synthetic.columns(31, ncol, k.get_press_min(), nlay=nlay)
    emis = t(np.repeat(base["sfc_emis"][:, None], k.get_nband(), 1))

    def run(top_at_1):
        cols, _ = oriented(base, top_at_1)
        fl = pkg.FluxesBroadband(t(np.zeros((nlay + 1, ncol))), t(np.zeros((nlay + 1, ncol))))
        assert k.lw_fluxes(t(cols["plev"]), t(cols["tlay"]), t(cols["tsfc"]), t(cols["tlev"]),
                           helpers.product_gas_concs(pkg, cols, t), top_at_1, emis, fl) == ""
        err, hr = pkg.heating_rate(fl.flux_up, fl.flux_dn, t(cols["plev"]))
        assert err == ""
        err, again = fl.heating_rate(t(cols["plev"]))          # the class convenience: the free function's bits
        assert err == "" and same_bits(again, back(hr))
        return back(fl.flux_up), back(fl.flux_dn), back(hr)

    check_both_orientations(pkg, t, run, base["plev"])


def test_chain_sw_fluxes_allsky_both_orientations(pkg, gpu, models):
    t = T(gpu)
    k, ncol, nlay = models["sw"], 70, 60
    nband = k.get_nband()
    base = synthetic.columns(47, ncol, k.get_press_min(), nlay=nlay, shortwave=True)
    base_cloud = synthetic.clouds(47, ncol, nlay, nband)
    alb = np.repeat(base["albedo"][:, None], nband, 1)

    def run(top_at_1):
        cols, cloud = oriented(base, top_at_1, base_cloud)
        part = pkg.OpticalProps2str()
        part.tau, part.ssa, part.g = (t(cloud[n]) for n in ("tau", "ssa", "g"))
        fl = pkg.FluxesBroadband(*(t(np.zeros((nlay + 1, ncol))) for _ in range(3)))
        assert k.sw_fluxes_allsky(t(cols["plev"]), t(cols["tlay"]), helpers.product_gas_concs(pkg, cols, t, helpers.SW_NAMES),
                                  top_at_1, t(cols["mu0"]), t(alb), t(alb.copy()), part, fl, delta_scale=True) == ""
        err, hr = fl.heating_rate(t(cols["plev"]))              # flux_dn is the total: direct beam included
        assert err == ""
        if top_at_1:
            assert float(fl.flux_dn_dir.max()) > 0 and bool((fl.flux_dn >= fl.flux_dn_dir).all())
        return back(fl.flux_up), back(fl.flux_dn), back(hr)

    check_both_orientations(pkg, t, run, base["plev"])


def test_chain_rte_lw_byband_both_orientations(pkg, gpu, models):
    t = T(gpu)
    k, ncol, nlay = models["lw"], 70, 60
    nband = k.get_nband()
    base = synthetic.columns(59, ncol, k.get_press_min(), nlay=nlay)
    emis = t(np.repeat(base["sfc_emis"][:, None], nband, 1))

    def run(top_at_1):
        cols, _ = oriented(base, top_at_1)
        like = t(np.zeros(1))
        op = pkg.OpticalProps1scl()
        op.alloc_1scl(ncol, nlay, k, like=like)
        src = pkg.SourceFuncLW()
        src.alloc(ncol, nlay, k, like=like)
        assert k.gas_optics(None, t(cols["plev"]), t(cols["tlay"]), t(cols["tsfc"]), helpers.product_gas_concs(pkg, cols, t),
                            op, src, tlev=t(cols["tlev"])) == ""
        z = lambda *s: t(np.zeros(s))
        fl = pkg.FluxesByband(z(nband, nlay + 1, ncol), z(nband, nlay + 1, ncol), flux_up=z(nlay + 1, ncol), flux_dn=z(nlay + 1, ncol))
        assert pkg.rte_lw(op, top_at_1, src, emis, fl) == ""
        err, hr = fl.bnd_heating_rate(t(cols["plev"]))          # nouter = nband
        assert err == "" and tuple(hr.shape) == (nband, nlay, ncol)
        err, again = pkg.heating_rate(fl.bnd_flux_up, fl.bnd_flux_dn, t(cols["plev"]))
        assert err == "" and same_bits(again, back(hr))
        err, broad = fl.heating_rate(t(cols["plev"]))           # the broadband members of the same container
        assert err == "" and same_bits(broad, ref.heating_rate(back(fl.flux_up), back(fl.flux_dn), cols["plev"]))
        return back(fl.bnd_flux_up), back(fl.bnd_flux_dn), back(hr)

    assert nband > 1
    check_both_orientations(pkg, t, run, base["plev"])


def test_graph_capture_without_a_warm_up(pkg, gpu):
    """One call captured on a fresh stream -- a single-branch graph, no call of this shape before it -- and replayed once
    gives the restatement's bits (the call uses no scratch)."""
    import torch
    t = T(gpu)
    fu, fd, plev, cp = ref.inputs(9, 131, 7, 5, np.float64, True)
    want = ref.heating_rate(fu, fd, plev, cp)
    dev = [t(a) for a in (fu, fd, plev, cp)]
    out = t(np.full(want.shape, -7.0))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        err, _ = pkg.heating_rate(dev[0], dev[1], dev[2], heating_rate=out, cp=dev[3])
    assert err == ""
    out.fill_(-7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out, want)
