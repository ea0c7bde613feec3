"""CPU tests of McICA cloud sampling: the five C symbols and their Python bindings, the numpy restatement of the sampler
(tests/mcica_helpers.py: known answers of Philox4x32-10, statistics and structure of the masks), the refusals of the new
calls in their documented order where no GPU is (nothing computes on the CPU), the code objects of the masked kernels, and
the Fortran sources."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as entry
import mcica_helpers as mh
from conftest import LW_FSCK, SW_WIDE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ecckd_cloud_mask_sample", "ecckd_increment_masked", "ecckd_increment_masked_f32", "ecckd_sw_fluxes_allsky_mcica",
           "ecckd_lw_fluxes_allsky_mcica")


def test_symbols_are_declared_exported_and_bound(pkg):
    for s in SYMBOLS:
        assert s in entry.exported_symbols(), s
        assert hasattr(pkg.lib(), s) and getattr(pkg.lib(), s).argtypes is not None, s
    L = pkg.lib()
    assert len(L.ecckd_cloud_mask_sample.argtypes) == 12
    assert len(L.ecckd_increment_masked.argtypes) == 15
    assert len(L.ecckd_lw_fluxes_allsky_mcica.argtypes) == 25 and len(L.ecckd_sw_fluxes_allsky_mcica.argtypes) == 27
    assert len(L.ecckd_lw_fluxes_allsky.argtypes) == 24   # (the unmasked call keeps its argument list)
    header = open(os.path.join(ROOT, "include", "ecckd_hip.h")).read()
    assert "#define ECCKD_OVERLAP_MAX_RAN 0" in header and "#define ECCKD_OVERLAP_EXP_RAN 1" in header
    assert "PARITY WITH IT IS UNPINNED" in header
    for f in (pkg.OpticalProps1scl.increment, pkg.GasOpticsEcckd.lw_fluxes_allsky, pkg.GasOpticsEcckd.sw_fluxes_allsky):
        assert inspect.signature(f).parameters["cloud_mask"].default is None, f
    sig = inspect.signature(pkg.sample_cloud_mask)
    assert list(sig.parameters) == ["cloud_frac", "ngpt", "overlap", "overlap_param", "seed", "col0", "device"]
    assert sig.parameters["overlap"].default == "max_ran"
    assert "kernels_cloud_sampling.hip" in pkg._SOURCES


def test_philox_known_answers():
    for ctr, key, want in mh.KNOWN_ANSWERS:
        got = mh.philox4x32_10(*ctr, *key)
        assert tuple(int(x) for x in got) == want, (ctr, key, [hex(int(x)) for x in got])
    # vectorised over the counter: the same words
    c0 = np.array([0, 0xFFFFFFFF, 0x243F6A88], dtype=np.uint64)
    assert int(mh.philox4x32_10(c0, 0, 0, 0, 0, 0)[0][0]) == 0x6627E8D5


def _profile(nlay, ncol):
    cf = np.zeros((nlay, ncol))
    cf[3:7] = np.array([0.2, 0.5, 0.3, 0.8])[:, None]
    cf[10] = 0.4
    cf[12:14] = 0.6
    cf[15] = 1.0
    return cf


def test_sampler_restatement_properties():
    """What the definition promises, on 20 000 columns x 32 g-points: layer cover within 5 standard errors of cloud_frac;
    maximum overlap nests adjacent cloudy layers and a block's cover is its largest fraction; parameter 0 is random
    overlap; blocks behind a clear layer are independent; a column's mask depends on its global index only."""
    nlay, ncol, ng = 20, 20000, 32
    cf = _profile(nlay, ncol)
    cases = ((mh.MAX_RAN, None), (mh.EXP_RAN, np.full((nlay - 1, ncol), 0.5)), (mh.EXP_RAN, np.zeros((nlay - 1, ncol))),
             (mh.EXP_RAN, np.ones((nlay - 1, ncol))))
    for ov, al in cases:
        m = mh.sample(cf, ng, ov, al, seed=12345, col0=7)
        b = mh.unpack(m, ng)
        assert not np.any(m >> np.uint64(ng)), "bits ngpt..63 must be 0"
        frac = b.mean(axis=(1, 2))
        se = np.sqrt(cf[:, 0] * (1 - cf[:, 0]) / (ncol * ng))
        # (g-points of a column are independent draws within a layer: u is drawn per g-point or carried per g-point)
        assert np.all(np.abs(frac - cf[:, 0]) <= 5 * se), (ov, frac, cf[:, 0])
        assert b[15].all() and not m[cf[:, 0] == 0].any()
        cover = b[3:7].any(axis=0).mean()
        maximal = ov == mh.MAX_RAN or al[0, 0] == 1.0
        if maximal:
            assert np.all(b[3] <= b[4]) and np.all(b[5] <= b[4]) and np.all(b[5] <= b[6])
            assert abs(cover - 0.8) <= 5 * np.sqrt(0.8 * 0.2 / (ncol * ng)), cover
        if ov == mh.EXP_RAN and al[0, 0] == 0.0:
            want = 1 - 0.8 * 0.5 * 0.7 * 0.2
            assert abs(cover - want) <= 5 * np.sqrt(want * (1 - want) / (ncol * ng)), cover
        if ov == mh.EXP_RAN and al[0, 0] == 0.5:
            assert 0.8 < cover < 1 - 0.8 * 0.5 * 0.7 * 0.2
        # layers 10 and 12 are separated by a clear layer: independent
        both = (b[10] & b[12]).mean()
        assert abs(both - 0.24) <= 5 * np.sqrt(0.24 * 0.76 / (ncol * ng)), both
    # sharding: columns 100..199 of a call with col0 = 7 are a call of their own with col0 = 107
    m = mh.sample(cf, ng, mh.MAX_RAN, None, 12345, 7)
    assert np.array_equal(m[:, 100:200], mh.sample(cf[:, 100:200], ng, mh.MAX_RAN, None, 12345, 107))
    assert not np.array_equal(m[:, 100:200], mh.sample(cf[:, 100:200], ng, mh.MAX_RAN, None, 12345, 0))
    assert not np.array_equal(m, mh.sample(cf, ng, mh.MAX_RAN, None, 12346, 7))
    # 0 / 1 / NaN
    cf3 = np.array([[0.0, 1.0, np.nan, 1.0], [1.0, 1.0, 0.5, np.nan]])
    m3 = mh.sample(cf3, 27, mh.MAX_RAN, None, 1, 0)
    full = np.uint64(2 ** 27 - 1)
    assert m3[0, 0] == 0 and m3[0, 1] == full and m3[0, 2] == 0 and m3[0, 3] == full
    assert m3[1, 0] == full and m3[1, 1] == full and m3[1, 3] == 0 and 0 <= int(m3[1, 2]) <= int(full)
    # 64 g-points fill the word; 1 g-point uses bit 0 only
    assert mh.sample(np.ones((2, 3)), 64)[0, 0] == np.uint64(2 ** 64 - 1)
    assert np.all(mh.sample(np.full((5, 50), 0.5), 1) <= 1)


def test_synthetic_cloud_fraction(pkg):
    from rte_ecckd_amd import synthetic
    for c0, ncol, nlay in ((0, 333, 60), (17, 64, 137), (5, 1, 60)):
        cf = synthetic.cloud_fraction(c0, ncol, nlay)
        tau = synthetic.clouds(c0, ncol, nlay, 5)["tau"]
        assert cf.shape == (nlay, ncol) and cf.dtype == np.float64 and cf.flags.c_contiguous
        assert np.array_equal(cf > 0, tau[0] > 0) and np.all(cf <= 1.0) and np.all(cf[cf > 0] > 0)
    # columns are addressed globally, as every other synthetic field
    assert np.array_equal(synthetic.cloud_fraction(0, 100, 60)[:, 40:], synthetic.cloud_fraction(40, 60, 60))
    assert len(np.unique(synthetic.cloud_fraction(0, 333, 60))) > 100


def test_sampler_refusals_in_order_launch_nothing(pkg):
    """ngpt > 64; unknown overlap; EXP_RAN without overlap_param; host values outside [0, 1]; then, with valid arguments,
    no device: an error, never a mask made on the CPU."""
    import torch
    cf = np.full((6, 4), 2.0)   # (outside [0, 1]: every earlier refusal wins over it)
    al = np.full((5, 4), 0.5)

    def msg(*a, **k):
        with pytest.raises(ValueError) as e:
            pkg.sample_cloud_mask(*a, **k)
        return str(e.value)

    assert "at most 64 g-points, not 65" in msg(cf, 65, overlap=7)
    assert "ngpt must be at least 1" in msg(cf, 0, overlap=7)
    assert "unknown overlap 7" in msg(cf, 32, overlap=7)
    assert "unknown overlap" in msg(cf, 32, overlap="random")
    assert "needs overlap_param" in msg(cf, 32, overlap="exp_ran")
    assert "cloud fraction outside [0, 1]" in msg(cf, 32, overlap="exp_ran", overlap_param=al)
    assert "cloud fraction outside [0, 1]" in msg(-cf, 32)
    ok = np.full((6, 4), 0.5)
    ok[2, 1] = np.nan   # (a NaN is a clear layer, not an error)
    assert "overlap parameter outside [0, 1]" in msg(ok, 32, overlap="exp_ran", overlap_param=al + 1.0)
    if torch.cuda.is_available():   # (where there is a GPU the valid call computes: the words of the restatement)
        assert np.array_equal(pkg.sample_cloud_mask(ok, 32, overlap="exp_ran", overlap_param=al),
                              mh.sample(ok, 32, mh.EXP_RAN, al))
    else:
        assert "no CPU fallback" in msg(ok, 32, overlap="exp_ran", overlap_param=al)
        assert "no CPU fallback" in msg(ok, 32)


def _wide_model(pkg, ng=65):
    """A host-only model of `ng` g-points with a Planck table (the builder route of test_capi_host)."""
    lp = np.log([10., 100., 1000.])
    T = 200. + np.arange(6).reshape(2, 3)
    k = pkg.GasOpticsEcckd()
    err = k.init_from_tables(lp, T, [dict(name="x", code=1, coefficient=np.ones((2, 3, ng)))],
                             planck=(np.array([100., 200.]), np.ones((2, ng))), device=-1)
    assert err == "", err
    return k


def test_masked_call_refusals_in_order(pkg):
    """The masked fused calls and the masked increment: more than 64 g-points first -- it wins over everything in the
    unmasked call's own list -- then that list; with valid arguments a host-only model fails loudly.  Outputs untouched."""
    nlay, ncol = 60, 4
    gc = pkg.GasConcs(["h2o"]); gc.set_vmr("h2o", 1e-3)
    fl = pkg.FluxesBroadband(np.full((nlay + 1, ncol), -7.0), np.full((nlay + 1, ncol), -7.0))
    plev, tlay, tsfc, tlev = (np.full((nlay + 1, ncol), 1e4), np.full((nlay, ncol), 250.), np.full(ncol, 250.),
                              np.full((nlay + 1, ncol), 250.))
    mask = np.full((nlay, ncol), 5, dtype=np.uint64)
    untouched = lambda: np.all(fl.flux_up == -7.0) and np.all(fl.flux_dn == -7.0) and np.all(mask == 5)

    # longwave: a 65-g model with the wrong band count and no tlev -- the g-point count is named first
    wide = _wide_model(pkg)
    part = pkg.OpticalProps1scl()
    part.tau = np.full((wide.get_nband() + 1, nlay, ncol), 0.5)
    emis = np.full((ncol, wide.get_nband()), 0.98)
    m = wide.lw_fluxes_allsky(plev, tlay, tsfc, None, gc, True, emis, part, fl, cloud_mask=mask)
    assert "ecckd_lw_fluxes_allsky_mcica" in m and "at most 64 g-points, not 65" in m and untouched()
    # ... and without a mask the same call names the band count (the unmasked call's first refusal)
    assert "nband_p" in wide.lw_fluxes_allsky(plev, tlay, tsfc, None, gc, True, emis, part, fl)
    # shortwave entry point: the model's g-point count is checked before anything else as well
    two = pkg.OpticalProps2str()
    two.tau, two.ssa, two.g = (np.full((wide.get_nband() + 1, nlay, ncol), 0.5) for _ in range(3))
    m = wide.sw_fluxes_allsky(plev, tlay, gc, True, np.full(ncol, 0.5), emis, emis, two, fl, cloud_mask=mask)
    assert "ecckd_sw_fluxes_allsky_mcica" in m and "at most 64 g-points, not 65" in m and untouched()

    # the unmasked calls' own lists, in their order, with a mask
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=-1) == ""
    nb = k.get_nband()
    emis = np.full((ncol, nb), 0.98)
    wrong = pkg.OpticalProps1scl(); wrong.tau = np.full((nb + 1, nlay, ncol), 0.5)
    good = pkg.OpticalProps2str()
    assert good.alloc_2str_bands(ncol, nlay, k) == ""
    for a in (good.tau, good.ssa, good.g):
        a[:] = 0.5
    call = lambda p, tlev_=tlev: k.lw_fluxes_allsky(plev, tlay, tsfc, tlev_, gc, True, emis, p, fl, cloud_mask=mask)
    pkg.set_arithmetic(pkg.REFERENCE_ORDER)
    try:
        assert "nband_p = %d" % (nb + 1) in call(wrong, None) and untouched()
        assert "fast arithmetic mode" in call(good, None) and untouched()
    finally:
        pkg.set_arithmetic(pkg.FAST)
    assert call(good, None) == "tlev is required for ecckd" and untouched()
    assert "no CPU fallback" in call(good) and untouched()
    # a mask of the wrong type or shape never reaches the library
    assert "uint64" in k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gc, True, emis, good, fl, cloud_mask=mask.astype(np.int64))
    assert "shape" in k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gc, True, emis, good, fl, cloud_mask=mask[1:])

    ksw = pkg.GasOpticsEcckd()
    assert ksw.load(SW_WIDE, device=-1) == ""
    nbs = ksw.get_nband()
    alb = np.full((ncol, nbs), 0.2)
    sw = pkg.OpticalProps2str()
    assert sw.alloc_2str_bands(ncol, nlay, ksw) == ""
    for a in (sw.tau, sw.ssa, sw.g):
        a[:] = 0.5
    swcall = lambda p: ksw.sw_fluxes_allsky(plev, tlay, gc, True, np.full(ncol, 0.5), alb, alb, p, fl, cloud_mask=mask)
    bad = pkg.OpticalProps2str()
    bad.tau, bad.ssa, bad.g = (np.full((nbs + 2, nlay, ncol), 0.5) for _ in range(3))
    assert "nband_p = %d" % (nbs + 2) in swcall(bad) and untouched()
    pkg.set_arithmetic(pkg.REFERENCE_ORDER)
    try:
        assert "fast arithmetic mode" in swcall(sw) and untouched()
    finally:
        pkg.set_arithmetic(pkg.FAST)
    assert "no CPU fallback" in swcall(sw) and untouched()

    # masked increment: ngpt > 64 first (it wins over ssa without g), then ecckd_increment's list, then no device
    op1 = pkg.OpticalProps2str()
    op1.tau, op1.ssa = np.full((65, nlay, ncol), 1.0), np.full((65, nlay, ncol), 0.5)
    op1.g = np.full((65, nlay, ncol), 0.5)
    op2 = pkg.OpticalProps1scl(); op2.tau = np.full((65, nlay, ncol), 1.0)
    m = op1.increment(op2, cloud_mask=mask)
    assert "ecckd_increment_masked" in m and "at most 64 g-points, not 65" in m and np.all(op1.tau == 1.0)
    import torch
    if not torch.cuda.is_available():
        assert "no HIP device" in op1.increment(op2) and np.all(op1.tau == 1.0)   # (65 g-points are fine without a mask)
        op1.tau, op1.ssa, op1.g = (np.full((32, nlay, ncol), 0.5) for _ in range(3))
        op2.tau = np.full((32, nlay, ncol), 1.0)
        assert "no CPU fallback" in op1.increment(op2, cloud_mask=mask) and np.all(op1.tau == 0.5)
    b2g = np.array([[1, 10], [12, 32]], dtype=np.int32)
    op1.tau, op1.ssa, op1.g = (np.full((32, nlay, ncol), 0.5) for _ in range(3))
    op2.tau = np.full((2, nlay, ncol), 1.0)
    assert "does not tile" in op1.increment(op2, band2gpt=b2g, cloud_mask=mask) and np.all(op1.tau == 0.5)


def test_mcica_code_objects(pkg):
    """The masked kernels are in the library under their own names.  The masked forms of the Planck-recomputing layer-split
    solver keep what the all-sky forms they extend have -- no spilled VGPR, no scratch, two waves per SIMD; the masked
    shortwave forms keep three waves per SIMD (the systolic form spills outside its sweeps as the form it extends does,
    114 VGPRs there: reported, not capped)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = kernel_resources.kernels(pkg.LIB_PATH)
    lw = {n: k for n, k in ks.items() if "rte_lw_split_mcica_kernel<" in n}
    assert len(lw) == 4, list(lw)
    for n, k in lw.items():
        assert "rte_lw_split_mcica_kernel<15, 4, 32, " in n and n.split(">")[0].endswith(", 2"), n
        assert k["spill_vgpr"] == 0 and k["scratch_bytes"] == 0 and kernel_resources.waves_per_simd(k) == 2, (n, k)
        assert k["max_flat_wg"] == 512, (n, k)
    sys_ = {n: k for n, k in ks.items() if "rte_sw_sys_mcica_kernel<" in n}
    two = {n: k for n, k in ks.items() if "rte_sw_mcica_kernel<" in n}
    assert len(sys_) == 4 and len(two) == 2, (list(sys_), list(two))
    for n, k in list(sys_.items()) + list(two.items()):
        assert kernel_resources.waves_per_simd(k) == 3, (n, k)
        print(n, "spilled VGPRs", k["spill_vgpr"], "scratch", k["scratch_bytes"], "B")
    assert len([n for n in ks if "increment_masked_kernel<" in n]) == 16
    assert len([n for n in ks if "cloud_mask_sample_kernel<" in n]) == 6
    # the kernels they extend are still there under their names
    for name, count in (("rte_lw_split_allsky_kernel<", 4), ("rte_sw_sys_allsky_kernel<", 4), ("rte_sw_allsky_kernel<", 2),
                        ("increment_kernel<", 16)):
        assert len([n for n in ks if name in n]) == count, name


def test_fortran_mcica_forms(pkg):
    """The module declares sample_cloud_mask over the C symbol and the optional cloud_mask arguments, the driver takes the
    cloud-fraction file, and the sources still compile (skipped without amdflang)."""
    text = open(os.path.join(pkg.FORTRAN_DIR, "gas_optics_ecckd.F90")).read()
    assert "procedure, public :: sample_cloud_mask" in text
    for sym in ("ecckd_cloud_mask_sample", "ecckd_lw_fluxes_allsky_mcica", "ecckd_sw_fluxes_allsky_mcica"):
        assert 'name="%s"' % sym in text, sym
    assert text.count("integer(c_int64_t), dimension(:,:), intent(in), optional :: cloud_mask") == 2
    drv_text = open(os.path.join(pkg.FORTRAN_DIR, "ecckd_driver.F90")).read()
    assert "sample_cloud_mask" in drv_text and "cloud_mask=mask_b" in drv_text and "int(c0 - 1, int64)" in drv_text
    drv = pkg.build_fortran()
    if drv is None:
        pytest.skip("no amdflang in this image")
    out = subprocess.run([drv], capture_output=True, text=True)
    assert out.returncode != 0 and "usage: ecckd_driver" in out.stderr and "[cloudfrac.bin]" in out.stderr
    # a cloud-fraction file without a particle file is refused with the usage text, before any file is opened
    out = subprocess.run([drv, "lw", "none.nc", "none.bin", "none.out", "0", "1", "0", "1", "0", "1", "", "cloudfrac.bin"],
                         capture_output=True, text=True)
    assert out.returncode != 0 and "needs a particle file" in out.stderr and "usage: ecckd_driver" in out.stderr
