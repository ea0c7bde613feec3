"""Fused per-band fluxes on the GPU (lw_fluxes_byband / sw_fluxes_byband: ecckd_lw_flux_bands / ecckd_sw_flux_bands) against
the composed routes the library already has, on the shapes that reach each solver family's band-window path.

Bars.  Longwave, every variant: np.array_equal per band plane and for the broadband members against gas_optics ->
[increment by band (masked)] -> rte_lw with a FluxesByband; with inc_flux (the by-band solver call has none) plain
rte_lw(inc_flux=) on each band's g-slice of the same arrays, the broadband members then being the planes added in band order
from +0, as sum_planes does.  Shortwave clear sky without toa_scale: array_equal against gas_optics -> rte_sw with a
FluxesByband.  Shortwave all-sky, masked or with toa_scale: 1e-9 * max(1, max|flux_dn|) of the composed by-band result, the
bar tests/test_gpu_allsky.py holds the broadband pair to (ssa is formed in a different order inside the solver).

Longwave at 60 layers: the fused kernels (the parent's lw_fluxes among them) are not bit-identical to rte_lw at its default
solver at any g-point count -- they fold four 15-layer segments where the register-resident solver walks the column -- so
against that route the 60-layer cases are held to helpers.FLUX_ATOL, and bit for bit against rte_lw on the layer-split solver
with the same segments ("lw_solver" = 1, "lw_split_seg" = 15).

Measured on an MI355X: 60-layer planes 1.7e-13 / 2.3e-13 / 2.8e-13 W m-2 from the default-solver route at 70 (top-down),
70 (bottom-up, three angles, inc_flux) and 20000 columns, every variant, and 0 from the layer-split route; lw_fluxes itself
1.7e-13 from gas_optics + rte_lw at 70 x 60 x 36 g and 0 with the layer-split solver; every other longwave case 0; shortwave
with particles / mask / toa_scale 0 to 4.4e-16 (1.1e-13 at 16454 columns) against a bar of 1.3e-6; the sum of the planes
1e-13 to 7e-13 from the broadband fused calls."""
import types

import numpy as np
import pytest

import helpers
from helpers import FLUX_ATOL
from rte_ecckd_amd import synthetic

pytestmark = pytest.mark.gpu
SW_NAMES = helpers.SW_NAMES


def _defaults(pkg):
    pkg.reset_solver_options()   # (leaves the implementation choices alone: they are set back here)
    for name, value in (("sw_solver", 0), ("sw_tail_split", 1), ("lw_solver", 0), ("lw_split_seg", 10)):
        pkg.set_solver_option(name, value)
    pkg.set_arithmetic(pkg.FAST)


@pytest.fixture(autouse=True)
def default_options(pkg):
    _defaults(pkg)
    yield
    _defaults(pkg)


@pytest.fixture(scope="module")
def models(pkg, gpu):
    from conftest import LW_FSCK, LW_RRTMGP, SW_WIDE
    out = {}
    for name, path in (("rrtmgp", LW_RRTMGP), ("fsck", LW_FSCK), ("sw", SW_WIDE)):
        out[name] = pkg.GasOpticsEcckd()
        assert out[name].load(path, device=0) == ""
    counts = lambda k: [int(hi - lo + 1) for lo, hi in k.get_band2gpt()]
    assert counts(out["rrtmgp"]) == [3, 4, 5, 5, 4, 1, 3, 1, 3, 1, 1, 1, 1, 1, 1, 1] and out["rrtmgp"].get_ngpt() == 36
    assert counts(out["fsck"]) == [32] and counts(out["sw"]) == [8, 7, 6, 2, 4]
    return out


def T(gpu):
    import torch

    def to(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(gpu)
    return to


def back(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def make_mask(seed, nlay, ncol, b2g):
    """Random 63-bit words; column 0 all ones, column 1 all zero (where the call has them); in every band of two or more
    g-points some word's bits differ inside the band."""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 2**63, (nlay, ncol), dtype=np.uint64)
    if ncol >= 2:
        m[:, 0] = np.uint64(2**64 - 1)
        m[:, 1] = np.uint64(0)
    if nlay * ncol >= 8:
        for lo, hi in b2g:
            if hi > lo:
                bits = (m >> np.uint64(lo - 1)) & np.uint64((1 << int(hi - lo + 1)) - 1)
                assert np.any((bits != 0) & (bits != np.uint64((1 << int(hi - lo + 1)) - 1))), (lo, hi)
    return m


def particles(pkg, cloud, to, kind):
    """kind '2str' (tau, ssa, g), '1scl' (tau alone) or None."""
    if kind is None:
        return None
    op = pkg.OpticalProps2str() if kind == "2str" else pkg.OpticalProps1scl()
    op.tau = to(cloud["tau"].copy())
    if kind == "2str":
        op.ssa, op.g = to(cloud["ssa"].copy()), to(cloud["g"].copy())
    return op


def band_fluxes(pkg, to, nb, nlay, ncol, dn_dir=None, broadband=True):
    """A FluxesByband filled with NaN: dn_dir None (longwave), True or False (shortwave with / without the direct planes)."""
    nan3 = lambda: to(np.full((nb, nlay + 1, ncol), np.nan))
    nan2 = lambda: to(np.full((nlay + 1, ncol), np.nan)) if broadband else None
    return pkg.FluxesByband(nan3(), nan3(), nan3() if dn_dir else None, nan2(), nan2(), nan2() if dn_dir else None)


def values(fl):
    return {n: back(getattr(fl, n)) for n in ("bnd_flux_up", "bnd_flux_dn", "bnd_flux_dn_dir", "flux_up", "flux_dn", "flux_dn_dir")
            if getattr(fl, n) is not None}


def same_bits(got, want, what=""):
    assert got.keys() == want.keys(), (got.keys(), want.keys())
    for n in got:
        assert np.array_equal(got[n], want[n], equal_nan=True), "%s %s: max |diff| %.3e" % (
            what, n, np.nanmax(np.abs(got[n] - want[n])))


# ------------------------------------------------------------------------------------------------
# longwave
# ------------------------------------------------------------------------------------------------
def lw_case(k, c0, ncol, nlay, top_at_1, seed):
    cols = synthetic.columns(c0, ncol, k.get_press_min(), nlay=nlay)
    cloud = synthetic.clouds(c0, ncol, nlay, k.get_nband())
    rng = np.random.default_rng(seed)
    cols["emis"] = rng.uniform(0.9, 1.0, (ncol, k.get_nband()))
    cols["inc_flux"] = rng.uniform(0.0, 2.0, (k.get_ngpt(), ncol))
    if not top_at_1:   # bottom-up arrays: the vertical axis of every profile reversed
        for n in ("plev", "tlay", "tlev", "h2o", "o3"):
            cols[n] = np.ascontiguousarray(cols[n][::-1])
        for n in ("tau", "ssa", "g"):
            cloud[n] = np.ascontiguousarray(cloud[n][:, ::-1])
    return cols, cloud


def lw_bands(pkg, k, cols, cloud, to, top_at_1, kind=None, mask=None, nmus=1, inc=False, broadband=True):
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to)
    fl = band_fluxes(pkg, to, k.get_nband(), nlay, ncol, None, broadband)
    part = particles(pkg, cloud, to, kind)
    ins = [to(cols[n]) for n in ("plev", "tlay", "tsfc", "tlev", "emis")] + [to(cols["inc_flux"]) if inc else None,
                                                                            None if mask is None else to(mask)]
    copies = [None if a is None else back(a).copy() for a in ins] + ([back(a).copy() for a in (part.tau,)] if part else [])
    assert k.lw_fluxes_byband(ins[0], ins[1], ins[2], ins[3], gc, top_at_1, ins[4], fl, n_gauss_angles=nmus, inc_flux=ins[5],
                              particles=part, cloud_mask=ins[6]) == ""
    for a, c in zip(ins + ([part.tau] if part else []), copies):   # inputs are never written
        assert a is None or np.array_equal(back(a), c, equal_nan=True)
    return values(fl)


def lw_composed(pkg, k, cols, cloud, to, top_at_1, kind=None, mask=None, nmus=1, inc=False, split15=False):
    """gas_optics -> [increment(particles, band2gpt[, cloud_mask])] -> rte_lw with a FluxesByband; with inc_flux plain rte_lw
    on each band's g-slice, the broadband members the planes added in band order.  split15: rte_lw takes the layer-split
    solver with 15 layers per wave ("lw_solver" = 1, "lw_split_seg" = 15), the segments of the fused 60-layer kernels."""
    if split15:
        pkg.set_solver_option("lw_solver", 1)
        pkg.set_solver_option("lw_split_seg", 15)
        try:
            return lw_composed(pkg, k, cols, cloud, to, top_at_1, kind, mask, nmus, inc)
        finally:
            pkg.set_solver_option("lw_solver", 0)
            pkg.set_solver_option("lw_split_seg", 10)
    nlay, ncol = cols["tlay"].shape
    nb, b2g = k.get_nband(), k.get_band2gpt()
    gc = helpers.product_gas_concs(pkg, cols, to)
    like = to(np.zeros(1))
    op = pkg.OpticalProps1scl(); op.alloc_1scl(ncol, nlay, k, like=like)
    src = pkg.SourceFuncLW(); src.alloc(ncol, nlay, k, like=like)
    assert k.gas_optics(None, to(cols["plev"]), to(cols["tlay"]), to(cols["tsfc"]), gc, op, src, tlev=to(cols["tlev"])) == ""
    if kind is not None:
        assert op.increment(particles(pkg, cloud, to, kind), band2gpt=b2g, cloud_mask=None if mask is None else to(mask)) == ""
    emis = to(cols["emis"])
    fl = band_fluxes(pkg, to, nb, nlay, ncol)
    if not inc:
        assert pkg.rte_lw(op, top_at_1, src, emis, fl, n_gauss_angles=nmus) == ""
        return values(fl)
    incf = to(cols["inc_flux"])
    lev_inc, lev_dec = src.level_views() if hasattr(src, "level_views") else (src.lev_source_inc, src.lev_source_dec)
    for b, (lo, hi) in enumerate(b2g):
        g = slice(int(lo) - 1, int(hi))
        op_b = types.SimpleNamespace(tau=op.tau[g], band2gpt=np.array([[1, int(hi - lo + 1)]], dtype=np.int32))
        src_b = types.SimpleNamespace(lay_source=src.lay_source[g], lev_source_inc=lev_inc[g], lev_source_dec=lev_dec[g],
                                      sfc_source=src.sfc_source[g], sfc_source_jac=None)
        one = pkg.FluxesBroadband(fl.bnd_flux_up[b], fl.bnd_flux_dn[b])
        assert pkg.rte_lw(op_b, top_at_1, src_b, emis[:, b:b + 1].contiguous(), one, n_gauss_angles=nmus, inc_flux=incf[g]) == ""
    out = values(fl)
    for n in ("up", "dn"):
        acc = np.zeros((nlay + 1, ncol))
        for b in range(nb):
            acc = acc + out["bnd_flux_" + n][b]
        out["flux_" + n] = acc
    return out


LW_CASES = [   # ncol, nlay, top_at_1, angles, inc_flux, variants
    (70, 60, True, 1, False, "all"),       # fused kernels, ragged last tile
    (70, 60, False, 3, True, "all"),
    (33, 61, True, 1, True, "all"),        # padded 64-layer variant
    (33, 61, False, 3, False, "all"),
    (5, 137, True, 3, False, "all"),       # ring beyond 96 layers
    (1, 1, True, 1, True, "all"),          # degenerate
    (20000, 60, True, 1, False, "few"),    # many tiles, where the broadband kernels would tail-split
]


@pytest.mark.parametrize("ncol,nlay,top_at_1,nmus,inc,variants", LW_CASES)
def test_longwave_planes_equal_the_composed_route(pkg, gpu, models, ncol, nlay, top_at_1, nmus, inc, variants):
    k, to = models["rrtmgp"], T(gpu)
    cols, cloud = lw_case(k, 11 * ncol, ncol, nlay, top_at_1, ncol + nlay)
    if ncol >= 20:
        assert cloud["cloudy"].any() and not cloud["cloudy"].all()
    mask = make_mask(ncol * nlay, nlay, ncol, k.get_band2gpt())
    kinds = [(None, None), ("2str", None), ("1scl", None), ("2str", mask), ("1scl", mask)]
    if variants == "few":
        kinds = [(None, None), ("2str", mask)]
    for kind, m in kinds:
        what = "%d x %d %s%s" % (ncol, nlay, kind, " masked" if m is not None else "")
        got = lw_bands(pkg, k, cols, cloud, to, top_at_1, kind, m, nmus, inc)
        want = lw_composed(pkg, k, cols, cloud, to, top_at_1, kind, m, nmus, inc)
        for n, a in got.items():   # every plane is written
            assert np.array_equal(np.isnan(a), np.isnan(want[n])), n
            assert not top_at_1 or not np.isnan(a).any(), n
        if nlay == 60:
            # The 60-layer fused kernels fold the composites of four 15-layer segments; rte_lw's default solver walks the
            # column from the top.  The two associate the same per-cell arithmetic differently (kernels_rte_lw_split.hip),
            # in the parent too -- measured below on lw_fluxes -- so against rte_lw at its default options these cases are
            # held to FLUX_ATOL, and to the bit against rte_lw on the layer-split solver with the same segments.
            worst = max(float(np.nanmax(np.abs(got[n] - want[n]))) for n in got)
            print("%s: planes - composed route at rte_lw's default solver %.2e W m-2 (bar %.0e)" % (what, worst, FLUX_ATOL))
            assert worst <= FLUX_ATOL
            want = lw_composed(pkg, k, cols, cloud, to, top_at_1, kind, m, nmus, inc, split15=True)
        same_bits(got, want, what)
        # the sum of the band planes against the broadband fused call
        if not inc and m is None and top_at_1:
            gc = helpers.product_gas_concs(pkg, cols, to)
            fl = pkg.FluxesBroadband(to(np.empty((nlay + 1, ncol))), to(np.empty((nlay + 1, ncol))))
            args = [to(cols[n]) for n in ("plev", "tlay", "tsfc", "tlev")] + [gc, top_at_1, to(cols["emis"])]
            if kind is None:
                assert k.lw_fluxes(*args, fl, n_gauss_angles=nmus) == ""
            else:
                assert k.lw_fluxes_allsky(*args, particles(pkg, cloud, to, kind), fl, n_gauss_angles=nmus) == ""
            for n in ("flux_up", "flux_dn"):
                d = float(np.max(np.abs(got["bnd_" + n].sum(axis=0) - back(getattr(fl, n)))))
                print("%d x %d %s: sum of planes - broadband %s %.2e" % (ncol, nlay, kind, n, d))
                assert d <= FLUX_ATOL


def test_broadband_fused_call_against_default_rte_lw_measured(pkg, gpu, models):
    """What the 60-layer bar above rests on, measured on the unchanged broadband call: lw_fluxes (Planck-recomputing
    layer-split kernel) against gas_optics -> rte_lw at its default solver, 36 g-points at once.  Printed; held to FLUX_ATOL."""
    k, to = models["rrtmgp"], T(gpu)
    ncol, nlay = 70, 60
    cols, _ = lw_case(k, 11 * ncol, ncol, nlay, True, ncol + nlay)
    gc, like = helpers.product_gas_concs(pkg, cols, to), to(np.zeros(1))
    ins = [to(cols[n]) for n in ("plev", "tlay", "tsfc", "tlev")]
    fused = pkg.FluxesBroadband(to(np.empty((nlay + 1, ncol))), to(np.empty((nlay + 1, ncol))))
    assert k.lw_fluxes(*ins, gc, True, to(cols["emis"]), fused) == ""
    op = pkg.OpticalProps1scl(); op.alloc_1scl(ncol, nlay, k, like=like)
    src = pkg.SourceFuncLW(); src.alloc(ncol, nlay, k, like=like)
    assert k.gas_optics(None, ins[0], ins[1], ins[2], gc, op, src, tlev=ins[3]) == ""
    for options in ((0, 10), (1, 15)):
        pkg.set_solver_option("lw_solver", options[0])
        pkg.set_solver_option("lw_split_seg", options[1])
        pair = pkg.FluxesBroadband(to(np.empty((nlay + 1, ncol))), to(np.empty((nlay + 1, ncol))))
        assert pkg.rte_lw(op, True, src, to(cols["emis"]), pair) == ""
        d = max(float(np.max(np.abs(back(getattr(fused, n)) - back(getattr(pair, n))))) for n in ("flux_up", "flux_dn"))
        print("lw_fluxes - (gas_optics + rte_lw, lw_solver %d, lw_split_seg %d): %.2e W m-2" % (options + (d,)))
        assert d <= FLUX_ATOL
        if options[0] == 1:
            assert d == 0.0   # the same segments: the same bits
    _defaults(pkg)


@pytest.mark.parametrize("ncol,nlay", [(70, 60), (33, 61)])
def test_one_band_is_the_existing_call(pkg, gpu, models, ncol, nlay):
    """LW_FSCK has one band: a window that spans the model is lw_fluxes / lw_fluxes_allsky / (cloud_mask=), bit for bit."""
    k, to = models["fsck"], T(gpu)
    cols, cloud = lw_case(k, 5, ncol, nlay, True, 3)
    mask = make_mask(7, nlay, ncol, k.get_band2gpt())
    args = lambda: [to(cols[n]) for n in ("plev", "tlay", "tsfc", "tlev")] + [helpers.product_gas_concs(pkg, cols, to), True,
                                                                              to(cols["emis"])]
    for kind, m in ((None, None), ("2str", None), ("1scl", None), ("2str", mask)):
        got = lw_bands(pkg, k, cols, cloud, to, True, kind, m)
        fl = pkg.FluxesBroadband(to(np.empty((nlay + 1, ncol))), to(np.empty((nlay + 1, ncol))))
        if kind is None:
            assert k.lw_fluxes(*args(), fl) == ""
        else:
            assert k.lw_fluxes_allsky(*args(), particles(pkg, cloud, to, kind), fl, cloud_mask=None if m is None else to(m)) == ""
        for n in ("flux_up", "flux_dn"):
            assert np.array_equal(got["bnd_" + n][0], back(getattr(fl, n))), (kind, n)
            assert np.array_equal(got[n], back(getattr(fl, n))), (kind, n)


def other_particles(cloud, keep, seed):
    """The particles of every band but `keep` replaced by other values."""
    rng = np.random.default_rng(seed)
    out = {n: v.copy() for n, v in cloud.items()}
    for n, lo, hi in (("tau", 0.0, 9.0), ("ssa", 0.5, 0.99), ("g", 0.5, 0.9)):
        new = rng.uniform(lo, hi, cloud[n].shape)
        new[keep] = cloud[n][keep]
        out[n] = new
    return out


def test_longwave_bands_are_independent_and_masks_act_per_bit(pkg, gpu, models):
    k, to = models["rrtmgp"], T(gpu)
    for ncol, nlay in ((70, 60), (33, 61)):
        cols, cloud = lw_case(k, 77, ncol, nlay, True, 1)
        mask = make_mask(3, nlay, ncol, k.get_band2gpt())
        ref = lw_bands(pkg, k, cols, cloud, to, True, "2str", mask)
        for b in (2, 5):   # a five-g-point band and a singleton band behind it
            got = lw_bands(pkg, k, cols, other_particles(cloud, b, b), to, True, "2str", mask)
            for n in ("bnd_flux_up", "bnd_flux_dn"):
                assert np.array_equal(got[n][b], ref[n][b]), (b, n)
                assert not np.array_equal(got[n][(b + 1) % 16], ref[n][(b + 1) % 16])
        unmasked = lw_bands(pkg, k, cols, cloud, to, True, "2str")
        ones = np.full((nlay, ncol), 2**64 - 1, dtype=np.uint64)
        same_bits(lw_bands(pkg, k, cols, cloud, to, True, "2str", ones), unmasked, "all-ones mask")
        clear = lw_bands(pkg, k, cols, cloud, to, True)
        for n in ref:   # column 1 of the mask is all zero: the clear-sky bits in every band; column 0 all ones: the unmasked bits
            assert np.array_equal(ref[n][..., 1], clear[n][..., 1]), n
            assert np.array_equal(ref[n][..., 0], unmasked[n][..., 0]), n
        # without the broadband members the planes are the same
        bare = lw_bands(pkg, k, cols, cloud, to, True, "2str", mask, broadband=False)
        assert set(bare) == {"bnd_flux_up", "bnd_flux_dn"}
        same_bits(bare, {n: ref[n] for n in bare})


# ------------------------------------------------------------------------------------------------
# shortwave
# ------------------------------------------------------------------------------------------------
def sw_case(k, c0, ncol, nlay, top_at_1, seed):
    cols = synthetic.columns(c0, ncol, k.get_press_min(), nlay=nlay, shortwave=True)
    rng = np.random.default_rng(seed)
    nb = k.get_nband()
    cols["alb_dir"], cols["alb_dif"] = rng.uniform(0.02, 0.6, (ncol, nb)), rng.uniform(0.02, 0.6, (ncol, nb))
    cols["scale"] = rng.uniform(0.97, 1.03, ncol)
    cloud = synthetic.clouds(c0, ncol, nlay, nb)
    if not top_at_1:
        for n in ("plev", "tlay", "tlev", "h2o", "o3"):
            cols[n] = np.ascontiguousarray(cols[n][::-1])
        for n in ("tau", "ssa", "g"):
            cloud[n] = np.ascontiguousarray(cloud[n][:, ::-1])
    return cols, cloud


def sw_bands(pkg, k, cols, cloud, to, top_at_1, part=False, delta=True, mask=None, scale=False, dn_dir=True, broadband=True):
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to, SW_NAMES)
    fl = band_fluxes(pkg, to, k.get_nband(), nlay, ncol, dn_dir, broadband)
    p = particles(pkg, cloud, to, "2str" if part else None)
    ins = [to(cols[n]) for n in ("plev", "tlay", "mu0", "alb_dir", "alb_dif")] + [to(cols["scale"]) if scale else None,
                                                                                 None if mask is None else to(mask)]
    ins += [p.tau, p.ssa, p.g] if part else []
    copies = [None if a is None else back(a).copy() for a in ins]
    assert k.sw_fluxes_byband(ins[0], ins[1], gc, top_at_1, ins[2], ins[3], ins[4], fl, particles=p, delta_scale=delta,
                              toa_scale=ins[5], cloud_mask=ins[6]) == ""
    for a, c in zip(ins, copies):   # inputs are never written
        assert a is None or np.array_equal(back(a), c, equal_nan=True)
    return values(fl)


def sw_composed(pkg, k, cols, cloud, to, top_at_1, part=False, delta=True, mask=None, scale=False):
    """gas_optics -> (delta_scale of a copy) -> increment by band (masked) -> rte_sw with a FluxesByband."""
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to, SW_NAMES)
    op = pkg.OpticalProps2str(); op.alloc_2str(ncol, nlay, k, like=to(np.zeros(1)))
    toa = to(np.empty((k.get_ngpt(), ncol)))
    assert k.gas_optics(None, to(cols["plev"]), to(cols["tlay"]), gc, op, toa) == ""
    if part:
        p = particles(pkg, cloud, to, "2str")
        if delta:
            assert p.delta_scale() == ""
        assert op.increment(p, band2gpt=k.get_band2gpt(), cloud_mask=None if mask is None else to(mask)) == ""
    if scale:
        toa = toa * to(cols["scale"])[None, :]
    fl = band_fluxes(pkg, to, k.get_nband(), nlay, ncol, True)
    assert pkg.rte_sw(op, top_at_1, to(cols["mu0"]), toa, to(cols["alb_dir"]), to(cols["alb_dif"]), fl) == ""
    return values(fl)


SW_CASES = [   # ncol, nlay, top_at_1, "sw_solver"
    (70, 60, True, 0),           # layer-systolic
    (70, 60, False, 0),
    (70, 60, True, 1),           # two-pass
    (70, 60, False, 1),
    (33, 61, True, 0),           # two-pass beyond 60 layers
    (1, 1, True, 0),             # degenerate
    (16384 + 70, 60, True, 0),   # a full round of whole tiles and a tail handed out one g-point per block
]


@pytest.mark.parametrize("ncol,nlay,top_at_1,solver", SW_CASES)
def test_shortwave_planes_against_the_composed_route(pkg, gpu, models, ncol, nlay, top_at_1, solver):
    k, to = models["sw"], T(gpu)
    pkg.set_solver_option("sw_solver", solver)
    cols, cloud = sw_case(k, 13 * ncol, ncol, nlay, top_at_1, ncol + nlay)
    if ncol >= 20:
        assert cloud["cloudy"].any() and not cloud["cloudy"].all()
    mask = make_mask(ncol + 1, nlay, ncol, k.get_band2gpt())
    big = ncol > 1000
    # clear sky without toa_scale: the bits of gas_optics -> rte_sw with a FluxesByband
    got = sw_bands(pkg, k, cols, cloud, to, top_at_1)
    want = sw_composed(pkg, k, cols, cloud, to, top_at_1)
    for n, a in got.items():
        assert not top_at_1 or not np.isnan(a).any(), n
    same_bits(got, want, "%d x %d clear" % (ncol, nlay))
    two = sw_bands(pkg, k, cols, cloud, to, top_at_1, dn_dir=False)
    assert "bnd_flux_dn_dir" not in two and "flux_dn_dir" not in two
    same_bits(two, {n: got[n] for n in two}, "without bnd_flux_dn_dir")
    variants = [dict(part=True, delta=True), dict(part=True, delta=False), dict(part=True, delta=True, mask=mask),
                dict(part=True, delta=False, mask=mask, scale=True), dict(scale=True)]
    if big:
        variants = [dict(part=True, delta=True, mask=mask, scale=True)]
    for v in variants:
        got = sw_bands(pkg, k, cols, cloud, to, top_at_1, **v)
        want = sw_composed(pkg, k, cols, cloud, to, top_at_1, **v)
        dn = want["flux_dn"]
        bar = 1e-9 * max(1.0, float(np.max(np.abs(dn)[~np.isnan(dn)], initial=0.0)))
        worst = 0.0
        for n, a in got.items():
            assert np.array_equal(np.isnan(a), np.isnan(want[n])), (n, v.keys())
            assert not top_at_1 or not np.isnan(a).any(), n
            worst = max(worst, float(np.max(np.abs(a - want[n])[~np.isnan(a)], initial=0.0)))
        print("%d x %d solver %d %s: fused - composed %.2e (bar %.1e)" % (ncol, nlay, solver, sorted(v), worst, bar))
        assert worst <= bar
        if v.get("part") and "mask" not in v and top_at_1:   # the sum of the planes against the broadband fused call
            gc = helpers.product_gas_concs(pkg, cols, to, SW_NAMES)
            fl = pkg.FluxesBroadband(*(to(np.empty((nlay + 1, ncol))) for _ in range(3)))
            assert k.sw_fluxes_allsky(to(cols["plev"]), to(cols["tlay"]), gc, True, to(cols["mu0"]), to(cols["alb_dir"]),
                                      to(cols["alb_dif"]), particles(pkg, cloud, to, "2str"), fl, delta_scale=v["delta"]) == ""
            for n in ("flux_up", "flux_dn", "flux_dn_dir"):
                d = float(np.max(np.abs(got["bnd_" + n].sum(axis=0) - back(getattr(fl, n)))))
                print("sum of planes - broadband %s %.2e" % (n, d))
                assert d <= FLUX_ATOL


def test_shortwave_bands_are_independent_and_masks_act_per_bit(pkg, gpu, models):
    k, to = models["sw"], T(gpu)
    for ncol, nlay, solver in ((70, 60, 0), (70, 60, 1), (33, 61, 0)):
        pkg.set_solver_option("sw_solver", solver)
        cols, cloud = sw_case(k, 99, ncol, nlay, True, 2)
        mask = make_mask(5, nlay, ncol, k.get_band2gpt())
        ref = sw_bands(pkg, k, cols, cloud, to, True, part=True, mask=mask)
        for b in (1, 3):   # seven g-points; two g-points (the narrowest band of the file)
            got = sw_bands(pkg, k, cols, other_particles(cloud, b, b), to, True, part=True, mask=mask)
            for n in ("bnd_flux_up", "bnd_flux_dn", "bnd_flux_dn_dir"):
                assert np.array_equal(got[n][b], ref[n][b]), (b, n)
                assert not np.array_equal(got[n][(b + 1) % 5], ref[n][(b + 1) % 5])
        unmasked = sw_bands(pkg, k, cols, cloud, to, True, part=True)
        ones = np.full((nlay, ncol), 2**64 - 1, dtype=np.uint64)
        same_bits(sw_bands(pkg, k, cols, cloud, to, True, part=True, mask=ones), unmasked, "all-ones mask")
        clear = sw_bands(pkg, k, cols, cloud, to, True)
        for n in ref:   # column 0: all ones, the unmasked bits; column 1: all zero, the clear sky at the bar of zero particles
            assert np.array_equal(ref[n][..., 0], unmasked[n][..., 0]), n
            assert float(np.max(np.abs(ref[n][..., 1] - clear[n][..., 1]))) <= 10 * FLUX_ATOL, n


# ------------------------------------------------------------------------------------------------
# memory spaces, caller-owned scratch, capture
# ------------------------------------------------------------------------------------------------
def test_host_arrays_scratch_block_and_capture(pkg, gpu, models):
    import torch
    to, host = T(gpu), np.ascontiguousarray
    ncol, nlay = 70, 60
    runs = []
    k = models["rrtmgp"]
    cols, cloud = lw_case(k, 21, ncol, nlay, True, 4)
    mask = make_mask(9, nlay, ncol, k.get_band2gpt())
    lw = lambda t_, c=cols, kk=k, m=mask: lw_bands(pkg, kk, c, cloud, t_, True, "2str", m, 3, True)
    runs.append((lw, k.lw_flux_bands_scratch_bytes(ncol, nlay)))
    assert runs[0][1] == (ncol * nlay * 36 + 32) * 8
    cols61, cloud61 = lw_case(k, 21, 33, 61, True, 4)
    mask61 = make_mask(9, 61, 33, k.get_band2gpt())
    runs.append((lambda t_: lw_bands(pkg, k, cols61, cloud61, t_, True, "2str", mask61, 1, False), k.lw_flux_bands_scratch_bytes(33, 61)))
    ks = models["sw"]
    scols, scloud = sw_case(ks, 23, ncol, nlay, True, 6)
    smask = make_mask(11, nlay, ncol, ks.get_band2gpt())
    runs.append((lambda t_: sw_bands(pkg, ks, scols, scloud, t_, True, part=True, delta=True, mask=smask, scale=True),
                 ks.sw_flux_bands_scratch_bytes(ncol, nlay, True)))
    align = lambda n: (n + 255) // 256 * 256
    tail = pkg.rte_sw_tail_scratch_bytes(ncol, nlay, 27)
    assert runs[2][1] >= align(ncol * nlay * 27 * 8) + tail + 3 * align(ncol * nlay * 5 * 8)
    for run, need in runs:
        ref = run(to)
        same_bits(run(host), ref, "host arrays")
        stream = torch.cuda.Stream()
        buf = torch.full((need,), 0xFF, dtype=torch.uint8, device=gpu)   # (NaN patterns: stale data would show)
        torch.cuda.synchronize()
        pkg.set_stream_scratch(buf, stream=stream)
        try:
            with torch.cuda.stream(stream):
                out = run(to)
            torch.cuda.synchronize()
            same_bits(out, ref, "caller-owned block")
        finally:
            pkg.set_stream_scratch(None, stream=stream)
        del buf
    # capture after one warm-up call on the stream: one linear sequence, replayed twice
    for longwave in (True, False):
        if longwave:
            gc = helpers.product_gas_concs(pkg, cols, to)
            fl = band_fluxes(pkg, to, 16, nlay, ncol)
            args = [to(cols[n]) for n in ("plev", "tlay", "tsfc", "tlev")] + [gc, True, to(cols["emis"]), fl]
            kw = dict(n_gauss_angles=3, inc_flux=to(cols["inc_flux"]), particles=particles(pkg, cloud, to, "2str"), cloud_mask=to(mask))
            call, ref = (lambda: k.lw_fluxes_byband(*args, **kw)), lw(to)
        else:
            gc = helpers.product_gas_concs(pkg, scols, to, SW_NAMES)
            fl = band_fluxes(pkg, to, 5, nlay, ncol, True)
            args = [to(scols["plev"]), to(scols["tlay"]), gc, True, to(scols["mu0"]), to(scols["alb_dir"]), to(scols["alb_dif"]), fl]
            kw = dict(particles=particles(pkg, scloud, to, "2str"), delta_scale=True, toa_scale=to(scols["scale"]), cloud_mask=to(smask))
            call, ref = (lambda: ks.sw_fluxes_byband(*args, **kw)), runs[2][0](to)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            assert call() == ""   # warm-up: the stream's block exists now
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            assert call() == ""
        for _ in range(2):
            for a in values(fl).keys():
                getattr(fl, a).fill_(float("nan"))
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            same_bits(values(fl), ref, "graph replay")
        del graph
    pkg.release_scratch(0)
