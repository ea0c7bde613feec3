"""GPU tests of McICA cloud sampling: the sampler against its numpy restatement bit for bit, the masked increment against
the numpy increment on masked optical depths, the masked fused calls against their building blocks and the C oracle, the
unbiasedness of the sampled fluxes against the exact independent-column answer, graph capture, and the Fortran driver.

Bars.  Sampler and fp64 increments: none (array_equal; there is no rounding in the definition, and the fp64 increment
spells the restatement's operations).  f32 increments: allsky_helpers.INCREMENT_BAR_ULP.  Longwave fused against its
building blocks: none (bit for bit); against the oracle: 10 FLUX_ATOL, test_gpu_lw_allsky's bar.  Shortwave: the two bars
tests/test_gpu_allsky.py holds the unmasked call to -- fused against composed 1e-9 max(1, max|flux|), either against the
oracle 10 FLUX_ATOL.  Unbiasedness: |mean - exact| <= 5 SE + 10 FLUX_ATOL per level and flux (the exact answer is a
probability-weighted sum of unmasked calls, so it does not depend on the sampler)."""
import struct
import subprocess

import numpy as np
import pytest

import allsky_helpers as ah
import helpers
import mcica_helpers as mh
import test_gpu_allsky as swt
import test_gpu_lw_allsky as lwt
from helpers import FLUX_ATOL
from rte_ecckd_amd import synthetic

pytestmark = pytest.mark.gpu
BAR = 10 * FLUX_ATOL
T, back = lwt.T, lwt.back


@pytest.fixture(autouse=True)
def default_options(pkg):
    def reset():
        pkg.reset_solver_options()
        pkg.set_solver_option("sw_solver", 0)
        pkg.set_solver_option("sw_tail_split", 1)
        pkg.set_arithmetic(pkg.FAST)
    reset()
    yield
    reset()


@pytest.fixture(scope="module")
def lw(pkg, gpu, oracle_mod):
    from conftest import LW_FSCK, LW_RRTMGP
    out = {}
    for name, path in (("fsck", LW_FSCK), ("rrtmgp", LW_RRTMGP)):
        k = pkg.GasOpticsEcckd()
        assert k.load(path, device=0) == ""
        out[name] = (k, oracle_mod.CkdModel(path), path)
    return out


@pytest.fixture(scope="module")
def sw(pkg, gpu, oracle_mod):
    from conftest import SW_WIDE
    k = pkg.GasOpticsEcckd()
    assert k.load(SW_WIDE, device=0) == ""
    return k, oracle_mod.CkdModel(SW_WIDE), SW_WIDE


def words(mask):
    """uint64 words of a mask returned by sample_cloud_mask (numpy uint64, or a torch int64 tensor with the same bits)."""
    return back(mask).view(np.uint64) if hasattr(mask, "cpu") else mask


def to_mask(mask, to):
    """A uint64 numpy mask as `to` wants it: numpy as it is, a device tensor as int64 with the same bits."""
    return mask if to is np.ascontiguousarray else to(mask.view(np.int64))


# ------------------------------------------------------------------------------------------------
# 6. the sampler
# ------------------------------------------------------------------------------------------------
def hand_profiles(nlay, ncol):
    out = {"clear": np.zeros((nlay, ncol)), "overcast": np.ones((nlay, ncol))}
    single = np.zeros((nlay, ncol)); single[nlay // 2] = 0.37
    alt = np.zeros((nlay, ncol)); alt[::2] = 0.55
    rng = np.random.default_rng(nlay + ncol)
    mixed = rng.uniform(0, 1, (nlay, ncol)) * (rng.uniform(0, 1, (nlay, ncol)) < 0.6)
    nan = mixed.copy(); nan[rng.uniform(0, 1, (nlay, ncol)) < 0.1] = np.nan
    out.update(single=single, alternating=alt, mixed=mixed, nan=nan)
    return out


@pytest.mark.parametrize("ncol,nlay", [(1, 1), (63, 137), (333, 60), (20000, 60)])
def test_sampler_equals_its_restatement(pkg, gpu, ncol, nlay):
    """ecckd_cloud_mask_sample equals mcica_helpers.sample bit for bit: both overlaps, synthetic and hand-made profiles,
    ngpt 27 / 32 / 36 / 64 / 1, col0 0 / 12345 / 2^33 + 5, device and host arrays, two column shards against the whole."""
    t = T(gpu)
    big = ncol >= 20000
    profiles = {"synthetic": synthetic.cloud_fraction(11, ncol, nlay)}
    if big:
        profiles["nan"] = hand_profiles(nlay, ncol)["nan"]
    else:
        profiles.update(hand_profiles(nlay, ncol))
    rng = np.random.default_rng(5)
    alpha = rng.uniform(0, 1, (max(nlay - 1, 0), ncol))
    alpha[rng.uniform(0, 1, alpha.shape) < 0.1] = 1.0
    alpha[rng.uniform(0, 1, alpha.shape) < 0.1] = 0.0
    ncase = 0
    for name, cf in profiles.items():
        for ng in ((27, 36, 64) if big else (27, 32, 36, 64, 1)):
            for col0 in ((12345, 2 ** 33 + 5) if big else (0, 12345, 2 ** 33 + 5)):
                for ov, al in (("max_ran", None), ("exp_ran", alpha)):
                    seed = 77 + ng
                    want = mh.sample(cf, ng, mh.MAX_RAN if ov == "max_ran" else mh.EXP_RAN, al, seed, col0)
                    got = words(pkg.sample_cloud_mask(t(cf), ng, ov, None if al is None else t(al), seed=seed, col0=col0))
                    assert got.shape == (nlay, ncol) and np.array_equal(got, want), (name, ng, col0, ov)
                    ncase += 1
                    if col0 == 12345 and ng in (27, 64):
                        host = pkg.sample_cloud_mask(cf, ng, ov, al, seed=seed, col0=col0)
                        assert host.dtype == np.uint64 and np.array_equal(host, want), (name, ng, ov, "host")
                        if ncol >= 63:   # two shards against the whole
                            cut = ncol // 3
                            a = words(pkg.sample_cloud_mask(t(cf[:, :cut]), ng, ov, None if al is None else t(al[:, :cut]),
                                                            seed=seed, col0=col0))
                            b = words(pkg.sample_cloud_mask(t(cf[:, cut:]), ng, ov, None if al is None else t(al[:, cut:]),
                                                            seed=seed, col0=col0 + cut))
                            assert np.array_equal(np.concatenate([a, b], axis=1), want), (name, ng, ov, "shards")
    print("%d x %d: %d sampler cases equal the restatement bit for bit" % (ncol, nlay, ncase))


# ------------------------------------------------------------------------------------------------
# 7. masked increment
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table,ncol,nlay", [
    ("sw_wide", 1, 1), ("lw_fsck", 63, 60), ("lw_rrtmgp", 64, 137), ("sw_wide", 333, 60), ("lw_rrtmgp", 333, 1),
    ("lw_fsck", 64, 1), ("sw_wide", 63, 137), ("sw_wide", 20000, 60)])
def test_increment_masked(pkg, gpu, table, ncol, nlay):
    """ecckd_increment_masked equals allsky_helpers.increment on op2 whose tau is zeroed where the bit is clear: the four
    combinations, on g-points and by band, fp64 array_equal and f32 at INCREMENT_BAR_ULP, device and host arrays (the case
    grid of test_increment_and_delta_scale); an all-ones mask equals ecckd_increment bit for bit."""
    b2g, ng = ah.band_tables()[table]
    nb = b2g.shape[0]
    cloud = synthetic.clouds(3 * ncol, ncol, nlay, nb)
    rng = np.random.default_rng(ncol + nlay)
    mask = rng.integers(0, 2 ** 63, (nlay, ncol), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (nlay, ncol), dtype=np.uint64)
    mask &= np.uint64(2 ** ng - 1)
    mask[rng.uniform(0, 1, (nlay, ncol)) < 0.2] = 0
    ones = np.full((nlay, ncol), 2 ** ng - 1, dtype=np.uint64)
    bits = np.moveaxis(mh.unpack(mask, ng), -1, 0)
    worst = 0.0
    spaces = [T(gpu)] + ([np.ascontiguousarray] if ncol <= 333 else [])
    for dt in (np.float64, np.float32):
        gas = tuple(a.astype(dt) for a in (
            rng.uniform(0, 2, (ng, nlay, ncol)) * rng.choice([0.0, 1e-6, 1.0], size=(ng, nlay, ncol)),
            rng.uniform(0, 1, (ng, nlay, ncol)), rng.uniform(0, 0.9, (ng, nlay, ncol))))
        part = tuple(cloud[n].astype(dt) for n in ("tau", "ssa", "g"))
        same = tuple(ah.spread(a, b2g, ng) for a in part)
        masked = (np.where(bits, same[0], dt(0)),) + same[1:]
        for to in spaces:
            for op1 in (gas[:1], gas):
                for op2, bands, ref2 in ((part[:1], b2g, masked[:1]), (part, b2g, masked), (same[:1], None, masked[:1]),
                                         (same, None, masked)):
                    a = swt.make(pkg, op1, to)
                    assert a.increment(swt.make(pkg, op2, to), band2gpt=bands, cloud_mask=to_mask(mask, to)) == ""
                    for got, want in zip(swt.values(a), ah.increment(op1, ref2)):
                        assert got.dtype == dt
                        if dt is np.float64:
                            assert np.array_equal(got, want)
                        worst = max(worst, ah.worst_ulp(got, want))
                    full, plain = swt.make(pkg, op1, to), swt.make(pkg, op1, to)
                    assert full.increment(swt.make(pkg, op2, to), band2gpt=bands, cloud_mask=to_mask(ones, to)) == ""
                    assert plain.increment(swt.make(pkg, op2, to), band2gpt=bands) == ""
                    for x, y in zip(swt.values(full), swt.values(plain)):
                        assert np.array_equal(x, y)
    print("%s %d x %d: masked increments %.2f u (bar %d)" % (table, ncol, nlay, worst, ah.INCREMENT_BAR_ULP))
    assert worst <= ah.INCREMENT_BAR_ULP


# ------------------------------------------------------------------------------------------------
# 8. fused longwave
# ------------------------------------------------------------------------------------------------
def lw_fused(pkg, k, cols, cloud, to, mask, one_stream=False, nmus=1, inc=False, top_at_1=True):
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to)
    part = lwt.particles(pkg, cloud, to, one_stream)
    fl = pkg.FluxesBroadband(to(np.full((nlay + 1, ncol), -1.0)), to(np.full((nlay + 1, ncol), -1.0)))
    assert k.lw_fluxes_allsky(to(cols["plev"]), to(cols["tlay"]), to(cols["tsfc"]), to(cols["tlev"]), gc, top_at_1,
                              to(cols["emis"]), part, fl, n_gauss_angles=nmus, inc_flux=to(cols["inc_flux"]) if inc else None,
                              cloud_mask=None if mask is None else to_mask(mask, to)) == ""
    assert np.array_equal(back(part.tau), cloud["tau"], equal_nan=True)
    return [back(fl.flux_up), back(fl.flux_dn)]


def lw_composed(pkg, k, cols, cloud, to, mask, one_stream=False, nmus=1, inc=False, top_at_1=True):
    """gas_optics_tau -> increment(particles, band2gpt, cloud_mask) -> rte_lw_fused, device tensors."""
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to)
    op = pkg.OpticalProps1scl(); op.alloc_1scl(ncol, nlay, k, like=to(np.zeros(1)))
    assert k.gas_optics_tau(to(cols["plev"]), to(cols["tlay"]), gc, op) == ""
    assert op.increment(lwt.particles(pkg, cloud, to, one_stream), band2gpt=k.get_band2gpt(), cloud_mask=to_mask(mask, to)) == ""
    fl = pkg.FluxesBroadband(to(np.full((nlay + 1, ncol), -2.0)), to(np.full((nlay + 1, ncol), -2.0)))
    assert k.rte_lw_fused(op, top_at_1, to(cols["tlay"]), to(cols["tlev"]), to(cols["tsfc"]), to(cols["emis"]), fl,
                          n_gauss_angles=nmus, inc_flux=to(cols["inc_flux"]) if inc else None) == ""
    return [back(fl.flux_up), back(fl.flux_dn)]


def layer_order(a, top_at_1):
    return a if top_at_1 else np.ascontiguousarray(a[::-1])


@pytest.mark.parametrize("ncol", [333, 777, 130, 1])
@pytest.mark.parametrize("nlay", [60, 37, 137])
@pytest.mark.parametrize("which", ["fsck", "rrtmgp"])
def test_longwave_fused_equals_its_building_blocks(pkg, gpu, lw, which, nlay, ncol):
    """lw_fluxes_allsky(cloud_mask=) equals gas_optics_tau + increment(cloud_mask=) + rte_lw_fused bit for bit on the grid
    of test_fused_equals_its_building_blocks (1 and 3 angles, inc_flux, one- and two-stream particles, both orientations
    at 60 and 137 layers); an all-ones mask equals the unmasked call and an all-zero mask the call with tau_p = 0, bit for
    bit.  The mask is sampled from synthetic.cloud_fraction (the cloudy layers of synthetic.clouds)."""
    k = lw[which][0]
    ng = k.get_ngpt()
    t = T(gpu)
    c0 = 7 * ncol + nlay
    cols, cloud = lwt.case(k, c0, ncol, nlay)
    cf = synthetic.cloud_fraction(c0, ncol, nlay)
    mask = mh.sample(cf, ng, mh.MAX_RAN, None, 99, c0)
    assert np.array_equal(words(pkg.sample_cloud_mask(t(cf), ng, seed=99, col0=c0)), mask)
    if cloud["cloudy"].any():
        part_bits = mh.unpack(mask[cf > 0], ng)
        assert part_bits.any() and (ncol < 100 or not part_bits.all())   # the mask does mask
    ones, zeros = np.full_like(mask, 2 ** ng - 1), np.zeros_like(mask)
    nothing = dict(cloud, tau=np.zeros_like(cloud["tau"]))
    for top_at_1 in ((True, False) if nlay in (60, 137) else (True,)):
        for one_stream in (False, True):
            for nmus in (1, 3):
                for inc in (False, True):
                    what = (which, nlay, ncol, top_at_1, one_stream, nmus, inc)
                    f = lw_fused(pkg, k, cols, cloud, t, mask, one_stream, nmus, inc, top_at_1)
                    c = lw_composed(pkg, k, cols, cloud, t, mask, one_stream, nmus, inc, top_at_1)
                    assert np.all(np.isfinite(f[0])) and np.all(np.isfinite(f[1])), what
                    assert np.array_equal(f[0], c[0]) and np.array_equal(f[1], c[1]), what
            plain = lw_fused(pkg, k, cols, cloud, t, None, one_stream, 1, True, top_at_1)
            full = lw_fused(pkg, k, cols, cloud, t, ones, one_stream, 1, True, top_at_1)
            assert np.array_equal(full[0], plain[0]) and np.array_equal(full[1], plain[1]), (which, nlay, ncol, "all ones")
            empty = lw_fused(pkg, k, cols, cloud, t, zeros, one_stream, 1, True, top_at_1)
            none = lw_fused(pkg, k, cols, nothing, t, None, one_stream, 1, True, top_at_1)
            assert np.array_equal(empty[0], none[0]) and np.array_equal(empty[1], none[1]), (which, nlay, ncol, "all zero")
            if cloud["cloudy"].any() and ncol >= 100:
                assert not np.array_equal(f[0], plain[0])
    # host arrays: the same bits
    h = lw_fused(pkg, k, cols, cloud, np.ascontiguousarray, mask, False, 1, False, True)
    d = lw_fused(pkg, k, cols, cloud, t, mask, False, 1, False, True)
    assert np.array_equal(h[0], d[0]) and np.array_equal(h[1], d[1])


@pytest.mark.parametrize("c0,ncol,nlay", [(9, 333, 60), (5, 130, 37)])
@pytest.mark.parametrize("which", ["fsck", "rrtmgp"])
def test_longwave_against_the_oracle(pkg, gpu, oracle_mod, lw, which, c0, ncol, nlay):
    """Against oracle.rte_lw on tau incremented in numpy by the numpy-masked cloud optical depth: 10 FLUX_ATOL, which stays
    20 times below the smallest cloud signal of a cloudy column."""
    k, m, _ = lw[which]
    ng = k.get_ngpt()
    cols = synthetic.columns(c0, ncol, k.get_press_min(), nlay=nlay)
    cloud = synthetic.clouds(c0, ncol, nlay, k.get_nband())
    cols["emis"] = np.repeat(cols["sfc_emis"][:, None], k.get_nband(), 1)
    cols["inc_flux"] = None
    items = helpers.oracle_gas_items(cols)
    mask = mh.sample(synthetic.cloud_fraction(c0, ncol, nlay), ng, mh.EXP_RAN, np.full((nlay - 1, ncol), 0.7), 3, c0)
    tau, lay, inc, dec, sfc, oerr = oracle_mod.gas_optics_int(m, cols["plev"], cols["tlay"], cols["tsfc"], items, cols["tlev"])
    assert oerr == ""
    emis = np.repeat(cols["sfc_emis"][None, :], m.ng, 0)
    clear = list(oracle_mod.rte_lw(tau, lay, inc, dec, emis, sfc))
    tm = mh.masked_tau(cloud["tau"], mask, m.band2gpt, ng)
    for one_stream in (False, True):
        op2 = (tm,) if one_stream else (tm, ah.spread(cloud["ssa"], m.band2gpt, ng), ah.spread(cloud["g"], m.band2gpt, ng))
        ref = list(oracle_mod.rte_lw(ah.increment((tau,), op2)[0], lay, inc, dec, emis, sfc))
        # (the existing guard, over the cloudy columns at least one g-point of which sees a cloud: a cloudy column whose
        # mask came out all clear equals its clear-sky column and has no signal to show)
        seen = mh.unpack(mask, ng).any(axis=-1).any(axis=0) & cloud["cloudy"]
        assert BAR <= ah.smallest_cloud_signal(ref, clear, seen) / 20
        out = lw_fused(pkg, k, cols, cloud, T(gpu), mask, one_stream)
        err = max(float(np.max(np.abs(a - b))) for a, b in zip(out, ref))
        print("longwave McICA %s %d x %d %s: %.2e W m-2 from the oracle (bar %.0e)" %
              (which, ncol, nlay, "one-stream" if one_stream else "two-stream", err, BAR))
        assert all(np.all(np.isfinite(a)) for a in out) and err < BAR


# ------------------------------------------------------------------------------------------------
# 9. fused shortwave
# ------------------------------------------------------------------------------------------------
def sw_fused(pkg, k, cols, cloud, to, delta, mask, with_dir=True):
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to, swt.SW_NAMES)
    part = swt.make(pkg, (cloud["tau"], cloud["ssa"], cloud["g"]), to)
    fl = pkg.FluxesBroadband(*(to(np.full((nlay + 1, ncol), -1.0)) for _ in range(3 if with_dir else 2)))
    assert k.sw_fluxes_allsky(to(cols["plev"]), to(cols["tlay"]), gc, True, to(cols["mu0"]), to(cols["alb_dir"]),
                              to(cols["alb_dif"]), part, fl, delta_scale=delta,
                              cloud_mask=None if mask is None else to_mask(mask, to)) == ""
    for a, b in zip(swt.values(part), (cloud["tau"], cloud["ssa"], cloud["g"])):
        assert np.array_equal(a, b, equal_nan=True)
    return [back(fl.flux_up), back(fl.flux_dn)] + ([back(fl.flux_dn_dir)] if with_dir else [])


def sw_composed(pkg, k, cols, cloud, to, delta, mask):
    """gas_optics_sw -> (delta_scale of a copy) -> increment by band with the mask -> rte_sw through the API objects."""
    nlay, ncol = cols["tlay"].shape
    ng = k.get_ngpt()
    gc = helpers.product_gas_concs(pkg, cols, to, swt.SW_NAMES)
    op = pkg.OpticalProps2str(); op.alloc_2str(ncol, nlay, k, like=to(np.zeros(1)))
    toa = to(np.empty((ng, ncol)))
    assert k.gas_optics(None, to(cols["plev"]), to(cols["tlay"]), gc, op, toa) == ""
    part = swt.make(pkg, (cloud["tau"], cloud["ssa"], cloud["g"]), to)
    if delta:
        assert part.delta_scale() == ""
    assert op.increment(part, band2gpt=k.get_band2gpt(), cloud_mask=to_mask(mask, to)) == ""
    fl = pkg.FluxesBroadband(*(to(np.empty((nlay + 1, ncol))) for _ in range(3)))
    assert pkg.rte_sw(op, True, to(cols["mu0"]), toa, to(cols["alb_dir"]), to(cols["alb_dif"]), fl) == ""
    return [back(fl.flux_up), back(fl.flux_dn), back(fl.flux_dn_dir)]


def oracle_sw_masked(oracle_mod, m, cols, items, cloud, delta, mask):
    """[up, dn, dir] of oracle.rte_sw on gas optics incremented in numpy by the (delta-scaled) band optics whose optical
    depth is zeroed where the g-point's bit is clear; mask None: clear sky."""
    otau, ossa, og, otoa, oerr = oracle_mod.gas_optics_ext(m, cols["plev"], cols["tlay"], items)
    assert oerr == ""
    op = (otau, ossa, og)
    if mask is not None:
        part = (cloud["tau"], cloud["ssa"], cloud["g"])
        if delta:
            part = ah.delta_scale(*part)
        op = ah.increment(op, (mh.masked_tau(part[0], mask, m.band2gpt, m.ng), ah.spread(part[1], m.band2gpt, m.ng),
                               ah.spread(part[2], m.band2gpt, m.ng)))
    g2b = m.gpt2band - 1
    return list(oracle_mod.rte_sw(op[0], op[1], op[2], cols["mu0"], otoa, np.ascontiguousarray(cols["alb_dir"][:, g2b].T),
                                  np.ascontiguousarray(cols["alb_dif"][:, g2b].T)))


@pytest.mark.parametrize("ncol,nlay", [(333, 60), (1500, 60), (333, 137), (700, 61)])
def test_shortwave_fused_composed_oracle(pkg, gpu, oracle_mod, sw, ncol, nlay):
    """sw_fluxes_allsky(cloud_mask=) -- the layer-systolic form at 60 layers, the two-pass form beyond -- against
    gas_optics + (delta_scale) + increment(cloud_mask=) + rte_sw at 1e-9 max(1, max|flux|), and either against the oracle
    on numpy-masked properties at 10 FLUX_ATOL, delta_scale 0 and 1: the bars of test_shortwave_compositions_and_fused.
    An all-ones mask equals the unmasked call bit for bit; host arrays stay inside the oracle bar."""
    k, m, _ = sw
    ng = k.get_ngpt()
    t = T(gpu)
    c0 = 7 * ncol
    cols, cloud = swt.sw_case(k, c0, ncol, nlay, ncol + nlay)
    items = helpers.oracle_gas_items(cols, swt.SW_NAMES)
    cf = synthetic.cloud_fraction(c0, ncol, nlay)
    mask = words(pkg.sample_cloud_mask(t(cf), ng, seed=5, col0=c0))
    assert np.array_equal(mask, mh.sample(cf, ng, mh.MAX_RAN, None, 5, c0))
    ones = np.full_like(mask, 2 ** ng - 1)
    clear = oracle_sw_masked(oracle_mod, m, cols, items, cloud, False, None)
    # (the guard below runs over the cloudy columns at least one g-point of which sees a cloud, as in the longwave test)
    seen = mh.unpack(mask, ng).any(axis=-1).any(axis=0) & cloud["cloudy"]
    for delta in (False, True):
        f = sw_fused(pkg, k, cols, cloud, t, delta, mask)
        c = sw_composed(pkg, k, cols, cloud, t, delta, mask)
        assert all(np.all(np.isfinite(a)) for a in f + c)
        pair_bar = 1e-9 * max(1.0, float(np.max(np.abs(c[1]))))
        pair_err = max(float(np.max(np.abs(a - b))) for a, b in zip(f, c))
        print("McICA %d x %d delta %d: fused - composed %.2e (bar %.1e)" % (ncol, nlay, delta, pair_err, pair_bar))
        assert pair_err <= pair_bar
        two = sw_fused(pkg, k, cols, cloud, t, delta, mask, with_dir=False)
        assert np.array_equal(two[0], f[0]) and np.array_equal(two[1], f[1])
        ref = oracle_sw_masked(oracle_mod, m, cols, items, cloud, delta, mask)
        assert BAR <= ah.smallest_cloud_signal(ref, clear, seen) / 20
        ef = max(float(np.max(np.abs(a - b))) for a, b in zip(f, ref))
        ec = max(float(np.max(np.abs(a - b))) for a, b in zip(c, ref))
        print("McICA %d x %d delta %d: fused %.2e, composed %.2e W m-2 from the oracle (bar %.0e)" % (ncol, nlay, delta, ef, ec, BAR))
        assert ef < BAR and ec < BAR
        plain = sw_fused(pkg, k, cols, cloud, t, delta, None)
        full = sw_fused(pkg, k, cols, cloud, t, delta, ones)
        assert all(np.array_equal(a, b) for a, b in zip(full, plain))
        assert not np.array_equal(f[0], plain[0])
        if ncol <= 333:
            h = sw_fused(pkg, k, cols, cloud, np.ascontiguousarray, delta, mask)
            assert max(float(np.max(np.abs(a - b))) for a, b in zip(h, ref)) < BAR


@pytest.mark.parametrize("ncol,nlay", [(333, 60), (200, 91)])
def test_shortwave_upper_half_of_the_word(pkg, gpu, sw, ncol, nlay):
    """A 54-g shortwave model (the tables of the 27-g file twice, ten bands, through init_from_tables) puts g-points into
    bits 32..53 of the word: the masked fused call -- layer-systolic and two-pass form -- against gas_optics +
    delta_scale + increment(cloud_mask=) + rte_sw at the bar of the 27-g test, with a mask whose lower and upper halves
    differ; clearing the upper half alone changes the fluxes, and gives those of the composition with the same mask."""
    k27, m, _ = sw
    twice = lambda a: np.concatenate([a, a], axis=-1)
    gases = [dict(name=n, code=tb["code"], composite_only=int(tb["composite_only"]), mole_fraction=tb["mole_fraction"],
                  reference_mole_fraction=tb["reference_mole_fraction"],
                  coefficient=twice(tb["coefficient"] if tb["code"] == 2 else tb["coefficient"][0]))
             for n, tb in zip(m.gas, m.tables)]
    b2g = np.concatenate([m.band2gpt, m.band2gpt + m.ng]).astype(np.int32)
    k = pkg.GasOpticsEcckd()
    assert k.init_from_tables(m.log_pressure, m.temperature, gases, solar=(0.5 * twice(m.solar_irradiance), twice(m.rayleigh)),
                              bands=(np.concatenate([m.band_lims_wvn, m.band_lims_wvn]), b2g)) == ""
    ng = k.get_ngpt()
    assert ng == 54 and k.get_nband() == 2 * k27.get_nband()
    t = T(gpu)
    cols, cloud = swt.sw_case(k, 13, ncol, nlay, ncol + nlay)
    mask = mh.sample(synthetic.cloud_fraction(13, ncol, nlay), ng, mh.MAX_RAN, None, 31, 13)
    cloudy = synthetic.cloud_fraction(13, ncol, nlay) > 0
    assert (mask[cloudy] >> np.uint64(32)).any() and ((mask[cloudy] >> np.uint64(32)) != (mask[cloudy] & np.uint64(2 ** 22 - 1))).any()
    lower = mask & np.uint64(2 ** 32 - 1)
    for delta in (False, True):
        f = sw_fused(pkg, k, cols, cloud, t, delta, mask)
        c = sw_composed(pkg, k, cols, cloud, t, delta, mask)
        assert all(np.all(np.isfinite(a)) for a in f + c)
        pair_bar = 1e-9 * max(1.0, float(np.max(np.abs(c[1]))))
        pair_err = max(float(np.max(np.abs(a - b))) for a, b in zip(f, c))
        fl_ = sw_fused(pkg, k, cols, cloud, t, delta, lower)
        cl_ = sw_composed(pkg, k, cols, cloud, t, delta, lower)
        low_err = max(float(np.max(np.abs(a - b))) for a, b in zip(fl_, cl_))
        moved = float(np.max(np.abs(f[0] - fl_[0])))
        print("54-g McICA %d x %d delta %d: fused - composed %.2e, upper half cleared %.2e (bar %.1e); clearing it moves flux_up by %.2e"
              % (ncol, nlay, delta, pair_err, low_err, pair_bar, moved))
        assert pair_err <= pair_bar and low_err <= pair_bar and moved > 1000 * pair_bar


# ------------------------------------------------------------------------------------------------
# 10. McICA is unbiased against the exact independent-column answer
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lw", "sw"])
def test_mcica_is_unbiased(pkg, gpu, lw, sw, kind):
    """4 096 copies of column 5 of synthetic.columns, 60 layers, cloud_frac 0.3 / 0.6 / 0.6 / 0.2 in layers 48-51 and 0.5 in
    layer 20, tau_p 8 and 1 there on every band, ssa_p 0.9, g_p 0.85, albedo 0.2, maximum-random overlap, seed 2024,
    col0 0.  The exact answer is the probability-weighted sum over the 4 x 2 cloud configurations (block A: none 0.4,
    {49, 50} 0.3, {48, 49, 50} 0.1, all 0.2; layer 20: 0.5) of overcast-or-clear unmasked calls.  Per level and flux:
    |mean over columns - exact| <= 5 SE + 10 FLUX_ATOL, SE = sample standard deviation / sqrt(4096).
    (The restatement alone, through the C oracle, sits at <= 1.98 SE longwave and <= 1.97 SE shortwave.)"""
    N, nlay = 4096, 60
    k = lw["fsck"][0] if kind == "lw" else sw[0]
    ng, nb = k.get_ngpt(), k.get_nband()
    t = T(gpu)
    one = synthetic.columns(5, 1, k.get_press_min(), nlay=nlay, shortwave=(kind == "sw"))

    def columns(n):
        cols = {name: (np.ascontiguousarray(np.repeat(v, n, axis=-1)) if isinstance(v, np.ndarray) else v) for name, v in one.items()}
        cols["emis"] = np.repeat(cols["sfc_emis"][:, None], nb, 1) if "sfc_emis" in cols else None
        cols["alb_dir"] = cols["alb_dif"] = np.full((n, nb), 0.2)
        cols["inc_flux"] = None
        return cols

    def cloud_of(n, on):
        tp = np.zeros((nb, nlay, n))
        tp[:, 48:52] = 8.0
        tp[:, 20] = 1.0
        tp *= on[None, :, None]
        return dict(tau=tp, ssa=np.full((nb, nlay, n), 0.9), g=np.full((nb, nlay, n), 0.85))

    def run(cols, cloud, mask):
        if kind == "lw":
            return lw_fused(pkg, k, cols, cloud, t, mask)
        return sw_fused(pkg, k, cols, cloud, t, True, mask, with_dir=False)

    cf = np.zeros((nlay, N))
    cf[48:52] = np.array([0.3, 0.6, 0.6, 0.2])[:, None]
    cf[20] = 0.5
    mask = words(pkg.sample_cloud_mask(t(cf), ng, "max_ran", seed=2024, col0=0))
    assert np.array_equal(mask, mh.sample(cf, ng, mh.MAX_RAN, None, 2024, 0))
    got = run(columns(N), cloud_of(N, np.ones(nlay)), mask)
    exact = [0.0, 0.0]
    c1 = columns(1)
    for layers_a, pa in (((), 0.4), ((49, 50), 0.3), ((48, 49, 50), 0.1), ((48, 49, 50, 51), 0.2)):
        for layers_b, pb in (((), 0.5), ((20,), 0.5)):
            on = np.zeros(nlay)
            on[list(layers_a + layers_b)] = 1.0
            f = run(c1, cloud_of(1, on), None)
            for i in range(2):
                exact[i] = exact[i] + pa * pb * f[i][:, 0]
    clear = run(c1, cloud_of(1, np.zeros(nlay)), None)
    for i, name in enumerate(("up", "dn")):
        mean = got[i].mean(axis=1)
        se = got[i].std(axis=1, ddof=1) / np.sqrt(N)
        dev = np.abs(mean - exact[i])
        z = dev / np.where(se > 0, se, np.inf)
        print("McICA %s flux_%s: max |mean - exact| %.3e W m-2, max z %.2f, SE up to %.3e, cloud signal %.2f W m-2" %
              (kind, name, dev.max(), z.max(), se.max(), np.abs(exact[i] - clear[i][:, 0]).max()))
        assert np.all(dev <= 5 * se + 10 * FLUX_ATOL), (kind, name, float(z.max()))
        assert np.abs(exact[i] - clear[i][:, 0]).max() > 20 * se.max()   # the clouds show far above the sampling noise


# ------------------------------------------------------------------------------------------------
# 11. capture
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lw", "sw"])
def test_sampler_and_masked_call_capture(pkg, gpu, lw, sw, kind):
    """The sampler and the masked fused call captured in one graph on one stream after a warm-up call, replayed twice, give
    the eager bits (the mask is made inside the graph; the stream's scratch block exists since the warm-up)."""
    import torch
    t = T(gpu)
    ncol, nlay = 1000, 60
    k = lw["rrtmgp"][0] if kind == "lw" else sw[0]
    ng = k.get_ngpt()
    if kind == "lw":
        cols, cloud = lwt.case(k, 3, ncol, nlay)
    else:
        cols, cloud = swt.sw_case(k, 3, ncol, nlay, 17)
    cf = synthetic.cloud_fraction(3, ncol, nlay)
    mask = mh.sample(cf, ng, mh.MAX_RAN, None, 8, 3)
    ref = lw_fused(pkg, k, cols, cloud, t, mask) if kind == "lw" else sw_fused(pkg, k, cols, cloud, t, True, mask, with_dir=False)
    gc = helpers.product_gas_concs(pkg, cols, t, swt.SW_NAMES if kind == "sw" else None)
    d_cf = t(cf)
    fl = pkg.FluxesBroadband(*(t(np.zeros((nlay + 1, ncol))) for _ in range(2)))
    if kind == "lw":
        part = lwt.particles(pkg, cloud, t, False)
        args = (t(cols["plev"]), t(cols["tlay"]), t(cols["tsfc"]), t(cols["tlev"]), gc, True, t(cols["emis"]), part, fl)
        call = lambda m_: k.lw_fluxes_allsky(*args, cloud_mask=m_)
    else:
        part = swt.make(pkg, (cloud["tau"], cloud["ssa"], cloud["g"]), t)
        args = (t(cols["plev"]), t(cols["tlay"]), gc, True, t(cols["mu0"]), t(cols["alb_dir"]), t(cols["alb_dif"]), part, fl)
        call = lambda m_: k.sw_fluxes_allsky(*args, delta_scale=True, cloud_mask=m_)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm = pkg.sample_cloud_mask(d_cf, ng, seed=8, col0=3)
        assert call(warm) == ""   # warm-up: the stream's block exists now
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    keep = {}
    with torch.cuda.graph(graph, stream=side):
        keep["mask"] = pkg.sample_cloud_mask(d_cf, ng, seed=8, col0=3)
        assert call(keep["mask"]) == ""
    for _ in range(2):
        for a in (fl.flux_up, fl.flux_dn, keep["mask"]):
            a.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(words(keep["mask"]), mask)
        assert np.array_equal(back(fl.flux_up), ref[0]) and np.array_equal(back(fl.flux_dn), ref[1])
    del graph
    pkg.release_scratch(0)


def _on_block(pkg, gpu, stream, size, body):
    """Runs body() on `stream` with a caller-owned scratch block of `size` bytes filled with 0xFF (stale data would show)."""
    import torch
    buf = torch.full((size,), 0xFF, dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    pkg.set_stream_scratch(buf, stream=stream)
    try:
        with torch.cuda.stream(stream):
            out = body()
        torch.cuda.synchronize()
    finally:
        pkg.set_stream_scratch(None, stream=stream)
    del buf
    return out


@pytest.mark.parametrize("nlay", [60, 37])
def test_longwave_masked_on_a_caller_owned_block(pkg, gpu, lw, nlay):
    """lw_fluxes_allsky(cloud_mask=) on a caller-owned block of exactly what the unmasked call documents for the shape (the
    mask is read in place) -- 60 layers: (ncol*nlay*ngpt + 32)*8 bytes; 37 layers (the general route, which runs the masked
    by-band increment on the scratch optical depth): (4*ncol*nlay*ngpt + ncol*ngpt + 64)*8 bytes plus the solver's ring,
    rte_lw_scratch_bytes -- filled with 0xFF bytes gives the eager bits; one byte less is refused ("too small") and
    launches nothing.  The unmasked call takes the same block: the sizes are equal."""
    import torch
    t = T(gpu)
    for which, ncol in (("fsck", 1000), ("rrtmgp", 1777)):
        k = lw[which][0]
        ng = k.get_ngpt()
        cols, cloud = lwt.case(k, 3, ncol, nlay)
        mask = mh.sample(synthetic.cloud_fraction(3, ncol, nlay), ng, mh.MAX_RAN, None, 8, 3)
        n3 = ncol * nlay * ng
        need = (n3 + 32) * 8 if nlay == 60 else (n3 + 32 + 3 * n3 + ncol * ng + 32) * 8 + pkg.rte_lw_scratch_bytes(ncol, nlay, ng)
        stream = torch.cuda.Stream()
        for one_stream in (False, True):
            ref = lw_fused(pkg, k, cols, cloud, t, mask, one_stream, 3, True)
            out = _on_block(pkg, gpu, stream, need, lambda: lw_fused(pkg, k, cols, cloud, t, mask, one_stream, 3, True))
            assert np.array_equal(out[0], ref[0]) and np.array_equal(out[1], ref[1]), (which, nlay, one_stream)
            plain = lw_fused(pkg, k, cols, cloud, t, None, one_stream, 3, True)
            out = _on_block(pkg, gpu, stream, need, lambda: lw_fused(pkg, k, cols, cloud, t, None, one_stream, 3, True))
            assert np.array_equal(out[0], plain[0]) and np.array_equal(out[1], plain[1])

            def too_small(with_mask):
                gc = helpers.product_gas_concs(pkg, cols, t)
                fl = pkg.FluxesBroadband(*(t(np.full((nlay + 1, ncol), -5.0)) for _ in range(2)))
                msg = k.lw_fluxes_allsky(t(cols["plev"]), t(cols["tlay"]), t(cols["tsfc"]), t(cols["tlev"]), gc, True,
                                         t(cols["emis"]), lwt.particles(pkg, cloud, t, one_stream), fl,
                                         cloud_mask=to_mask(mask, t) if with_mask else None)
                torch.cuda.synchronize()
                return msg, back(fl.flux_up), back(fl.flux_dn)
            for with_mask in (True, False):   # (the same byte is the limit with and without a mask)
                msg, up, dn = _on_block(pkg, gpu, stream, need - 1, lambda: too_small(with_mask))
                assert "too small" in msg and np.all(up == -5.0) and np.all(dn == -5.0), (which, nlay, one_stream, with_mask, msg)
        pkg.release_scratch(0)


@pytest.mark.parametrize("nlay", [60, 91])
def test_shortwave_masked_on_a_caller_owned_block(pkg, gpu, sw, nlay):
    """sw_fluxes_allsky(cloud_mask=) on a caller-owned block: the smallest block the UNMASKED call accepts for the shape
    (found by bisection on its "too small" refusal, which launches nothing) is the smallest the masked call accepts --
    the mask is read in place -- and on exactly that block, filled with 0xFF bytes, the masked call gives the eager bits;
    with delta_scale the block holds the three scaled band planes as well (include/ecckd_hip.h).  One byte less is refused
    with the outputs untouched."""
    import torch
    t = T(gpu)
    k = sw[0]
    ng, nb, ncol = k.get_ngpt(), k.get_nband(), 1000
    cols, cloud = swt.sw_case(k, 3, ncol, nlay, 17)
    mask = mh.sample(synthetic.cloud_fraction(3, ncol, nlay), ng, mh.MAX_RAN, None, 8, 3)
    stream = torch.cuda.Stream()
    align = lambda n: (n + 255) // 256 * 256

    def attempt(size, with_mask, delta):
        def body():
            gc = helpers.product_gas_concs(pkg, cols, t, swt.SW_NAMES)
            fl = pkg.FluxesBroadband(*(t(np.full((nlay + 1, ncol), -5.0)) for _ in range(3)))
            msg = k.sw_fluxes_allsky(t(cols["plev"]), t(cols["tlay"]), gc, True, t(cols["mu0"]), t(cols["alb_dir"]), t(cols["alb_dif"]),
                                     swt.make(pkg, (cloud["tau"], cloud["ssa"], cloud["g"]), t), fl, delta_scale=delta,
                                     cloud_mask=to_mask(mask, t) if with_mask else None)
            torch.cuda.synchronize()
            return msg, [back(fl.flux_up), back(fl.flux_dn), back(fl.flux_dn_dir)]
        return _on_block(pkg, gpu, stream, size, body)

    for delta in (False, True):
        planes = 3 * align(ncol * nlay * nb * 8) if delta else 0
        lo, hi = align(ncol * nlay * ng * 8) + planes - 1, 4 * align(ncol * nlay * ng * 8) + planes + (64 << 20)
        assert "too small" in attempt(lo, False, delta)[0] and attempt(hi, False, delta)[0] == ""
        while hi - lo > 1:   # smallest block the unmasked call accepts
            mid = (lo + hi) // 2
            if attempt(mid, False, delta)[0] == "":
                hi = mid
            else:
                lo = mid
        need = hi
        assert need >= align(ncol * nlay * ng * 8) + planes
        ref = sw_fused(pkg, k, cols, cloud, t, delta, mask)
        msg, out = attempt(need, True, delta)
        assert msg == "" and all(np.array_equal(a, b) for a, b in zip(out, ref)), (nlay, delta, msg)
        msg, out = attempt(need - 1, True, delta)
        assert "too small" in msg and all(np.all(a == -5.0) for a in out), (nlay, delta, msg)
        print("shortwave %d layers delta %d: caller-owned block of %d bytes serves the masked and the unmasked call" % (nlay, delta, need))
    pkg.release_scratch(0)


# ------------------------------------------------------------------------------------------------
# 12. Fortran driver with a cloud-fraction file
# ------------------------------------------------------------------------------------------------
def write_cloudfrac(path, overlap, seed, cf, alpha):
    with open(path, "wb") as f:
        f.write(struct.pack("<iq", overlap, seed))
        f.write(np.ascontiguousarray(cf, dtype="<f8").tobytes())
        if overlap == 1:
            f.write(np.ascontiguousarray(alpha, dtype="<f8").tobytes())


@pytest.mark.parametrize("mode,overlap", [("lw", 0), ("sw", 1), ("lw", 1), ("sw", 0)])
def test_fortran_driver_mcica(pkg, gpu, oracle_mod, lw, sw, tmp_path, mode, overlap):
    """ecckd_driver ... fused=1 particles.bin cloudfrac.bin, 250 columns in blocks of 64 (the last block partial: col0
    matters): output bit for bit the Python call -- with the mask sampled in ONE call over the whole column range -- on the
    whole column range, and on the driver's blocks."""
    drv = lwt.driver(pkg)
    shortwave = mode == "sw"
    ncol, nlay, block = 250, 60, 64
    k, m, path = sw if shortwave else lw["rrtmgp"]
    nb, ng = k.get_nband(), k.get_ngpt()
    cols = synthetic.columns(40, ncol, k.get_press_min(), nlay=nlay, shortwave=shortwave)
    cloud = synthetic.clouds(40, ncol, nlay, nb)
    cf = synthetic.cloud_fraction(40, ncol, nlay)
    alpha = np.random.default_rng(1).uniform(0, 1, (nlay - 1, ncol))
    seed = 2 ** 40 + 17
    names = synthetic.GAS_ORDER
    lwt.write_input(tmp_path / "in.bin", cols, names, shortwave)
    lwt.write_particles(tmp_path / "part.bin", cloud, True, True)
    write_cloudfrac(tmp_path / "frac.bin", overlap, seed, cf, alpha)
    base = [drv, mode, path, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(block), "1", "0", "1", "0", "1"]
    r = subprocess.run(base + [str(tmp_path / "part.bin"), str(tmp_path / "frac.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    fu, fd = lwt.read_output(tmp_path / "out.bin", ncol, nlay)
    mask = pkg.sample_cloud_mask(cf, ng, "exp_ran" if overlap else "max_ran", alpha if overlap else None, seed=seed, col0=0)
    assert np.array_equal(mask, mh.sample(cf, ng, overlap, alpha if overlap else None, seed, 0))

    def python_call(c0, c1):
        nc = c1 - c0
        cut = lambda a: np.ascontiguousarray(a[..., c0:c1])
        gc = lwt.block_gas_concs(pkg, cols, names, c0, c1)
        part = lwt.particles(pkg, {n: cut(cloud[n]) for n in ("tau", "ssa", "g")}, np.ascontiguousarray, False)
        fl = pkg.FluxesBroadband(np.empty((nlay + 1, nc)), np.empty((nlay + 1, nc)))
        if shortwave:
            alb = np.repeat(cut(cols["albedo"])[:, None], nb, 1)
            assert k.sw_fluxes_allsky(cut(cols["plev"]), cut(cols["tlay"]), gc, True, cut(cols["mu0"]), alb, alb.copy(), part, fl,
                                      delta_scale=True, cloud_mask=cut(mask)) == ""
        else:
            emis = np.repeat(cut(cols["sfc_emis"])[:, None], nb, 1)
            assert k.lw_fluxes_allsky(cut(cols["plev"]), cut(cols["tlay"]), cut(cols["tsfc"]), cut(cols["tlev"]), gc, True, emis,
                                      part, fl, cloud_mask=cut(mask)) == ""
        return fl.flux_up, fl.flux_dn

    pu, pd = np.empty_like(fu), np.empty_like(fd)
    for c0 in range(0, ncol, block):
        c1 = min(ncol, c0 + block)
        pu[:, c0:c1], pd[:, c0:c1] = python_call(c0, c1)
    assert np.array_equal(fu, pu) and np.array_equal(fd, pd), "driver against the Python call on the same blocks"
    wu, wd = python_call(0, ncol)
    assert np.array_equal(fu, wu) and np.array_equal(fd, wd), "driver against the Python call on the whole column range"
    # the mask changed something: the overcast call differs
    r = subprocess.run(base + [str(tmp_path / "part.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ou, _ = lwt.read_output(tmp_path / "out.bin", ncol, nlay)
    assert not np.array_equal(ou, fu)
