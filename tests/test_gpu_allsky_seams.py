"""The all-sky and McICA flux calls with clouds and cleared mask bits on the layers where the solvers change hands.

Every other GPU test of these calls takes its particles from synthetic.clouds, which leaves the first and the last layer of
every column -- and most prefetch, padding, ring and segment boundaries of the solvers -- free of particles.  Here the
particles and the hand-made mask words of tests/seam_helpers.py sit on exactly those layers (seam_helpers' docstring lists
them with the kernel lines they come from), and each call is held to the reference and the bar of its existing test:

  fp64 lw_fluxes_allsky (plain / cloud_mask, one- / two-stream particles), general route
      gas_optics_tau + increment + rte_lw_fused bit for bit; the C oracle on the numpy-incremented (masked) optical depth
      at 10 FLUX_ATOL = 1e-8 W m-2 (test_gpu_lw_allsky.py, test_gpu_mcica.py)
  fp64 at 60 layers (layer-split kernels): the same, lw_fluxes_clear_allsky with "lw_both_skies" 0 / 1 against the two
      calls bit for bit, flux_up_jac with "lw_jac_inline" 0 / 1 against the oracle's zero-source run at FLUX_ATOL
  fp64 flux_up_jac of the stand-alone kernel at 1, 2, 3, 4, 5, 7 and 61 layers: the oracle's zero-source run at FLUX_ATOL
  fp64 lw_fluxes_allsky(rescaled=True) / (use_2stream=True) at 60, 59, 61 and 5 layers: the composed route bit for bit; the
      composed solver against lw_rescaled_ref (test_gpu_lw_rescaled.BAR) / lw_2stream_ref (FLUX_ATOL)
  float32 lw_fluxes_allsky / lw_fluxes_clear_allsky: gas_optics + increment + rte_lw on float32 arrays bit for bit; one case
      per kernel form against the oracle on the float32-rounded inputs at helpers.lw_f32_bar
  fp64 sw_fluxes_allsky / sw_fluxes_clear_allsky / cloud_mask: the oracle at 10 FLUX_ATOL, fused against composed at
      1e-9 max(1, max|flux|), the clear-sky output bit for bit sw_fluxes
  float32 sw_fluxes_allsky: max and 99th percentile of e(F) <= 2 x those of e(C) against the fp64 call R, pooled per layer
      count over the "one"-pattern cases (test_gpu_allsky_f32.py), and 20 max e(F) <= the smallest cloud signal

Conditions asserted in the tests themselves: (1) removing the particles of any seam layer moves the case's reference by at
least 20 bars in every column that carries them (seam_helpers.layer_signals; shortwave cases with more than 8 seam layers
use one cloud per column, seam_helpers.signal_pattern); (2) test_every_seam_is_covered: over the module's cases every seam
layer of every form gets a cloudy cell, a cleared and a set mask bit; (3) where the existing tests promise it (longwave) the
clear columns equal the clear-sky call bit for bit, and the cloudy columns differ everywhere.
Condition 1 under a mask is narrower than "every column that carries a cloud": the 20-bar signal, the float32 shortwave
signal and "the cloudy columns differ" are taken over the columns in which at least half of the g-points see the cloud (the
mask words "ones" and "alternating").  A zero word makes the cell a clear one, and under a one-bit word one g-point of 27 to
36 carries the cloud, which moves the broadband flux by as little as 1e-8 W m-2; those words test the choice of the bit,
and a kernel that reads another bit, word half or layer for such a cell errs by the signal measured on the neighbouring
columns.  The case tables and both checks live in tests/seam_cases.py, which tests/test_allsky_seams_host.py runs on the CPU.

Layer counts and seam layers (array indices, top_at_1 = True; bottom-up they mirror):
  longwave register-resident solver, fp64 (LW_NLAY) and float32 (LW_NLAY and 60): 1 .. 5 every layer; 31 {0, 7, 8, 30};
      32 {0, 7, 8, 31}; 33 {0, 7, 8, 32}; 48, 49, 59, 60, 61, 64, 65, 80 {0, 7, 8, nlay-1}; 81, 96 {0, 3, 4, nlay-1};
      97 {0, 1, 3, 4, 5, 96}; 98 {0, 1, 2, 3, 4, 5, 6, 97}; 137 {0, 3, 4, 40, 41, 44, 45, 136}
  longwave layer-split kernels, fp64, 60 layers: {0, 1, 2, 14, 15, 16, 17, 29, 30, 31, 32, 44, 45, 46, 47, 59}, with the
      stand-alone Jacobian kernel's {0, 3, 55, 56, 59} ("lw_jac_inline" = 0)
  stand-alone Jacobian kernel: 1 .. 5 every layer; 7 {0, 2, 3, 6}; 61 {0, 56, 57, 60}, with the register solver's seams
  shortwave layer-systolic solver (SW_NLAY up to 60): the first and the last layer of every wave of 5 layers
  shortwave two-pass solver (61, 62, 137; "sw_solver" = 1 at 4, 10, 56 and 60): {0, 1, 2, 3, nlay-4 .. nlay-1} -- two
      layers in flight in the all-sky kernels, three in the composition's rte_sw, handed over at either end
  longwave two-stream solver (60, 59, 61, 5): the same {0, 1, 2, 3, nlay-4 .. nlay-1}, with the seams of the solver the
      rescaled call takes at that layer count (60: the layer-split kernels'; else the register-resident solver's)

Measured on an MI355X, the largest distance next to each bar (the bars come from the existing tests, not from these figures):
  fp64 longwave, general route: 2.3e-13 ... 1.1e-11 W m-2 from the oracle (bar 1e-8), smallest seam-layer signal 0.033;
      60 layers: 1.4e-13 ... 4.6e-13 (bar 1e-8), Jacobian 1.1e-15 ... 6.2e-15 W m-2 K-1 (bar 1e-9), signal 0.051
  stand-alone Jacobian kernel: 8.9e-16 ... 5.3e-15 W m-2 K-1 (bar 1e-9), smallest signal 3.6e-4
  rescaled: 5.7e-14 ... 8.8e-13 W m-2 from the restatement (bar 2.8e-12); two-stream: 2.8e-13 ... 5.8e-12 (bar 1e-9)
  float32 longwave: every equality holds; 2.9e-4 ... 1.1e-3 W m-2 from the oracle (bars 2.0e-3 ... 5.9e-3, signals 0.33 ... 8.2)
  fp64 shortwave: 8.5e-14 ... 2.0e-10 W m-2 from the oracle (bar 1e-8), fused - composed below 0.005 of its bar, signal 0.013
  float32 shortwave on seam clouds, max e(F) = max e(C) at every layer count (F and C hold the same bits), W m-2, with the
      smallest cloud signal: 1 layer 0.010 / 27; 2 0.0020 / 27; 4 0.0027 / 5.6; 5 0.00079 / 24; 6 0.0029 / 12; 9 0.033 / 15;
      10 0.0080 / 10; 11 0.0048 / 24; 55 0.026 / 25; 56 0.048 / 5.9; 59 0.20 / 8.2; 60 0.031 / 6.0; 61 0.0078 / 53;
      62 0.039 / 18; 137 0.13 / 7.2
Sensitivity (not committed): a library whose rte_lw_allsky_f32_kernel skips with_particles on the first walked layer passes
all of test_gpu_allsky_f32.py and fails all 56 cases of the two float32 longwave tests here."""
import json

import numpy as np
import pytest

import allsky_helpers as ah
import helpers
import lw_2stream_ref
import mcica_helpers as mh
import seam_helpers as sh
import test_gpu_allsky_f32 as f32t
import test_gpu_both_skies as bst
import test_gpu_lw_2stream as tst
import test_gpu_lw_jac as jact
import test_gpu_lw_rescaled as rst
from helpers import FLUX_ATOL, r32
from rte_ecckd_amd import synthetic
from seam_cases import (F32_ORACLE, JAC_KINDS, JAC_SHAPES, LW_WALK, SCAT_SHAPES, SCAT_WALK, SPLIT_KINDS, SW_NLAY, SW_SHAPES,
                        check_every_seam_is_covered, check_signal, differ_columns, f32_oracle_case, lw_general_cases, scat_kinds,
                        seam_case, seams_of, sw_cases, sw_ncol, sw_seam_case)
from test_gpu_allsky_f32 import models   # noqa: F401  (module-scoped fixture: name -> (GasOpticsEcckd, oracle CkdModel))

pytestmark = pytest.mark.gpu
BAR = 10 * FLUX_ATOL
F4 = np.float32


@pytest.fixture(autouse=True)
def default_options(pkg):
    def reset():
        pkg.reset_solver_options()
        for n, v in (("lw_tail_split", 1), ("sw_tail_split", 1), ("sw_solver", 0), ("lw_both_skies", 0)):
            pkg.set_solver_option(n, v)
        pkg.set_arithmetic(pkg.FAST)
    inline = pkg.get_solver_option("lw_jac_inline")
    reset()
    yield
    reset()
    pkg.set_solver_option("lw_jac_inline", inline)


def T(gpu, dtype=np.float64):
    """Arrays to device tensors: fp64 as they are (a mask's int64 view stays int64), float32 by one rounding."""
    return rst.T(gpu) if dtype == np.float64 else f32t.T(gpu, dtype)


def lw_columns(k, nlay, ncol):
    cols = synthetic.columns(3 + nlay, ncol, k.get_press_min(), nlay=nlay)
    rng = np.random.default_rng(ncol + nlay)
    cols["inc_flux"] = rng.uniform(0.0, 2.0, (k.get_ngpt(), ncol))
    cols["emis"] = np.repeat(cols["sfc_emis"][:, None], k.get_nband(), 1)
    return cols


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def distance(a, b):
    return max(float(np.max(np.abs(np.asarray(x, dtype=np.float64) - y))) for x, y in zip(a, b))


def lw_options(pkg, oracle_mod, series, iso, tail):
    pkg.set_solver_option("lw_series_terms", series)
    pkg.set_solver_option("lw_inc_flux_isotropic", iso)
    pkg.set_solver_option("lw_tail_split", tail)
    return oracle_mod.solver_options(lw_series_terms=series, lw_inc_flux_isotropic=iso)


# ------------------------------------------------------------------------------------------------
# longwave, fp64
# ------------------------------------------------------------------------------------------------
def lw_blocks(pkg, k, cols, cloud, to, mask, one_stream, nmus, inc, top_at_1):
    """gas_optics_tau -> increment(particles, band2gpt[, cloud_mask]) -> rte_lw_fused (test_gpu_mcica.lw_composed)."""
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to)
    op = pkg.OpticalProps1scl(); op.alloc_1scl(ncol, nlay, k, like=to(np.zeros(1)))
    assert k.gas_optics_tau(to(cols["plev"]), to(cols["tlay"]), gc, op) == ""
    assert op.increment(f32t.particles(pkg, cloud, to, one_stream), band2gpt=k.get_band2gpt(), cloud_mask=f32t.to_mask(mask, to)) == ""
    fl = pkg.FluxesBroadband(to(np.full((nlay + 1, ncol), -2.0)), to(np.full((nlay + 1, ncol), -2.0)))
    assert k.rte_lw_fused(op, top_at_1, to(cols["tlay"]), to(cols["tlev"]), to(cols["tsfc"]), to(cols["emis"]), fl,
                          n_gauss_angles=nmus, inc_flux=to(cols["inc_flux"]) if inc else None) == ""
    return [f32t.back(fl.flux_up), f32t.back(fl.flux_dn)]


def lw_fp64_variant(pkg, gpu, oracle_mod, k, m, which, kinds, nlay, ncol, v):
    """One walk entry of an fp64 longwave case: building blocks, clear columns, signal, oracle.  Returns (distance from the
    oracle, smallest seam-layer signal)."""
    top, one_stream, nmus, inc, masked, series, iso, tail = v
    what = (which, nlay, ncol) + tuple(v)
    t = T(gpu)
    cols = lw_columns(k, nlay, ncol)
    seams, cloud, mask = seam_case(which, kinds, nlay, ncol, top)
    mask = mask if masked else None
    opt = lw_options(pkg, oracle_mod, series, iso, tail)
    kw = dict(top_at_1=top, nmus=nmus, inc=inc)
    f, _ = jact.fused_call(pkg, k, cols, t, cloud=cloud, one_stream=one_stream, mask=mask, with_jac=False, **kw)
    assert all(np.all(np.isfinite(a)) for a in f), what
    assert same(f, lw_blocks(pkg, k, cols, cloud, t, mask, one_stream, nmus, inc, top)), what
    clear, _ = jact.fused_call(pkg, k, cols, t, with_jac=False, **kw)
    keep, differ = ~cloud["cloudy"], differ_columns(cloud, mask, m.ng)
    assert all(np.array_equal(a[:, keep], b[:, keep]) for a, b in zip(f, clear)), what          # condition 3
    assert differ.any() and np.all(np.abs(f[0] - clear[0]).max(axis=0)[differ] > 0), what
    run = sh.lw_reference(oracle_mod, m, cols, mask, one_stream, top, nmus, cols["inc_flux"] if inc else None, opt)
    ref = run(cloud)
    low = check_signal(run, ref, cloud, seams, mask, m.ng, BAR, what)
    err = distance(f, ref)
    assert err < BAR, (what, err)
    return err, low


@pytest.mark.parametrize("nlay,ncol", list(lw_general_cases(False)))
@pytest.mark.parametrize("which", ["fsck", "rrtmgp"])
def test_longwave_fp64_general_route(pkg, gpu, oracle_mod, models, which, nlay, ncol):
    """lw_fluxes_allsky away from 60 layers, the walk LW_WALK: building blocks bit for bit, the oracle at 10 FLUX_ATOL."""
    k, m = models[which]
    out = [lw_fp64_variant(pkg, gpu, oracle_mod, k, m, which, ("lw_register",), nlay, ncol, v) for v in LW_WALK]
    print("SEAM lw fp64 %s nlay %d ncol %d seams %s: %.2e W m-2 from the oracle (bar %.0e), smallest seam-layer signal %.3g"
          % (which, nlay, ncol, seams_of(("lw_register",), nlay, True), max(e for e, _ in out), BAR, min(s for _, s in out)))


@pytest.mark.parametrize("ncol", [1, 65])
@pytest.mark.parametrize("which", ["fsck", "rrtmgp"])
def test_longwave_fp64_sixty_layers(pkg, gpu, oracle_mod, models, which, ncol):
    """The layer-split kernels: plain, McICA, dual-sky and inline-Jacobian forms, and the stand-alone Jacobian kernel."""
    k, m = models[which]
    nlay, t = 60, T(gpu)
    out = [lw_fp64_variant(pkg, gpu, oracle_mod, k, m, which, SPLIT_KINDS, nlay, ncol, v) for v in LW_WALK]
    cols = lw_columns(k, nlay, ncol)
    sfc_jac = jact.oracle_sfc_jac(oracle_mod, m, cols["tsfc"])
    emis_gpt = np.repeat(cols["sfc_emis"][None, :], m.ng, 0)
    tau = sh.lw_reference(oracle_mod, m, cols).tau
    worst = 0.0
    for top, one_stream, nmus, inc, masked, series, iso, tail in LW_WALK:
        lw_options(pkg, oracle_mod, series, 0, tail)
        seams, cloud, mask = seam_case(which, SPLIT_KINDS, nlay, ncol, top)
        mask = mask if masked else None
        what = (which, ncol, top, one_stream, nmus, inc, masked, series)
        two = bst.lw_separate(pkg, k, cols, cloud, t, mask, one_stream, nmus, inc, top)
        for form in (0, 1):
            pkg.set_solver_option("lw_both_skies", form)
            assert same(bst.lw_both(pkg, k, cols, cloud, t, mask, one_stream, nmus, inc, top), two), (what, form)
        pkg.set_solver_option("lw_both_skies", 0)
        # the Jacobian: one cloud per column (seventeen cloudy layers leave 9e-9 W m-2 K-1 of the surface term at the top);
        # the single-column case then carries the first seam only -- the 65-column case has four columns on every seam
        seams, cloud, mask = seam_case(which, SPLIT_KINDS, nlay, ncol, top, sh.signal_pattern(seams))
        mask = mask if masked else None
        run = lambda c: [jact.oracle_jac(oracle_mod, jact.incremented(tau, m, c, one_stream, mask), emis_gpt, sfc_jac, top, nmus)]
        want = run(cloud)
        check_signal(run, want, cloud, seams, mask, m.ng, FLUX_ATOL, what)
        plain, _ = jact.fused_call(pkg, k, cols, t, top, nmus, inc, cloud, one_stream, mask, with_jac=False)
        for inline in (0, 1):
            pkg.set_solver_option("lw_jac_inline", inline)
            fluxes, jac = jact.fused_call(pkg, k, cols, t, top, nmus, inc, cloud, one_stream, mask)
            assert same(fluxes, plain), (what, inline)
            d = distance([jac], want)
            worst = max(worst, d)
            assert np.all(np.isfinite(jac)) and d < FLUX_ATOL, (what, inline, d)
    print("SEAM lw fp64 split %s ncol %d: %.2e W m-2 from the oracle (bar %.0e), Jacobian %.2e W m-2 K-1 (bar %.0e), smallest signal %.3g"
          % (which, ncol, max(e for e, _ in out), BAR, worst, FLUX_ATOL, min(s for _, s in out)))


@pytest.mark.parametrize("nlay,ncol", JAC_SHAPES)
@pytest.mark.parametrize("which", ["fsck", "rrtmgp"])
def test_longwave_jacobian_stand_alone_kernel(pkg, gpu, oracle_mod, models, which, nlay, ncol):
    """flux_up_jac of lw_fluxes, lw_fluxes_allsky and the masked call away from 60 layers, against the oracle's zero-source
    run on the numpy-incremented optical depth at FLUX_ATOL; the fluxes beside it are the plain call's bits."""
    k, m = models[which]
    kinds, t = JAC_KINDS, T(gpu)
    cols = lw_columns(k, nlay, ncol)
    sfc_jac = jact.oracle_sfc_jac(oracle_mod, m, cols["tsfc"])
    emis_gpt = np.repeat(cols["sfc_emis"][None, :], m.ng, 0)
    tau = sh.lw_reference(oracle_mod, m, cols).tau
    worst, low = 0.0, np.inf
    for top, one_stream, nmus, inc, masked, series, iso, tail in LW_WALK:
        lw_options(pkg, oracle_mod, series, 0, tail)
        seams, cloud, mask = seam_case(which, kinds, nlay, ncol, top)
        mask = mask if masked else None
        what = (which, nlay, ncol, top, one_stream, nmus, inc, masked, series)
        clear_jac = jact.fused_call(pkg, k, cols, t, top, nmus, inc)[1]
        worst = max(worst, distance([clear_jac], [jact.oracle_jac(oracle_mod, tau, emis_gpt, sfc_jac, top, nmus)]))
        run = lambda c: [jact.oracle_jac(oracle_mod, jact.incremented(tau, m, c, one_stream, mask), emis_gpt, sfc_jac, top, nmus)]
        want = run(cloud)
        low = min(low, check_signal(run, want, cloud, seams, mask, m.ng, FLUX_ATOL, what))
        plain, _ = jact.fused_call(pkg, k, cols, t, top, nmus, inc, cloud, one_stream, mask, with_jac=False)
        fluxes, jac = jact.fused_call(pkg, k, cols, t, top, nmus, inc, cloud, one_stream, mask)
        assert same(fluxes, plain) and np.all(np.isfinite(jac)), what
        keep = ~cloud["cloudy"]
        assert np.array_equal(jac[:, keep], clear_jac[:, keep]), what
        worst = max(worst, distance([jac], want))
    print("SEAM lw jacobian %s nlay %d ncol %d seams %s: %.2e W m-2 K-1 from the oracle (bar %.0e), smallest signal %.3g"
          % (which, nlay, ncol, seams_of(kinds, nlay, True), worst, FLUX_ATOL, low))
    assert worst < FLUX_ATOL


# ------------------------------------------------------------------------------------------------
# longwave with scattering, fp64: the rescaled and the two-stream solver
# ------------------------------------------------------------------------------------------------
def scattering_inputs(pkg, k, cols, to):
    """The gas optical depth and the Planck sources of the composed routes, as numpy arrays (with sfc_emis, inc_flux)."""
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to)
    like = to(np.zeros(1))
    one = pkg.OpticalProps1scl(); one.alloc_1scl(ncol, nlay, k, like=like)
    assert k.gas_optics_tau(to(cols["plev"]), to(cols["tlay"]), gc, one) == ""
    src = pkg.SourceFuncLW(); src.alloc(ncol, nlay, k, like=like)
    assert k.planck_sources(to(cols["tlay"]), to(cols["tsfc"]), src, tlev=to(cols["tlev"])) == ""
    b = f32t.back
    return dict(gas=b(one.tau), lay=b(src.lay_source), inc=b(src.lev_source_inc), dec=b(src.lev_source_dec),
                sfc_source=b(src.sfc_source), sfc_emis=cols["emis"], inc_flux=cols["inc_flux"])


def scattering_cell(a, cloud, mask, b2g, ng):
    """`a` with (tau, ssa, g) = (gas, 0, 0) incremented in numpy by the (masked) band triple."""
    tp = ah.spread(cloud["tau"], b2g, ng) if mask is None else mh.masked_tau(cloud["tau"], mask, b2g, ng)
    zero = np.zeros_like(a["gas"])
    tau, ssa, g = ah.increment((a["gas"], zero, zero), (tp, ah.spread(cloud["ssa"], b2g, ng), ah.spread(cloud["g"], b2g, ng)))
    return dict(a, tau=tau, ssa=ssa, g=g)


@pytest.mark.parametrize("nlay,ncol", SCAT_SHAPES)
def test_longwave_with_scattering(pkg, gpu, models, nlay, ncol):
    """lw_fluxes_allsky(rescaled=True) and (use_2stream=True): bit for bit the composed route (gas_optics_tau, planck_sources,
    increment by band on (tau, 0, 0), rte_lw); the composed solver on the numpy-incremented cell against the numpy
    restatement at the bar of its own test; the restatement's change when a seam layer loses its particles >= 20 bars."""
    k, m = models["fsck"]
    t = T(gpu)
    kinds = scat_kinds(nlay)
    cols = lw_columns(k, nlay, ncol)
    cols["emis"] = cols["emis"] * np.random.default_rng(nlay).uniform(0.95, 1.0, cols["emis"].shape)
    a0 = scattering_inputs(pkg, k, cols, t)
    b2g = k.get_band2gpt()
    worst_r = worst_2 = 0.0
    for top, masked, inc, nmus in SCAT_WALK:
        seams, cloud, mask = seam_case("fsck", kinds, nlay, ncol, top)
        mask = mask if masked else None
        what = (nlay, ncol, top, masked, inc, nmus)
        a = scattering_cell(a0, cloud, mask, b2g, m.ng)
        # rescaled
        fused = rst.fused(pkg, k, cols, cloud, mask, t, True, top, inc, nmus)
        assert same(fused, rst.composed(pkg, k, cols, cloud, mask, t, top, inc, nmus)), what
        assert same(fused, rst.solve(pkg, a, b2g, t, top, nmus, inc)), what
        run = lambda c: list(rst.restated(scattering_cell(a0, c, mask, b2g, m.ng), b2g, top, nmus, inc))
        want = run(cloud)
        check_signal(run, want, cloud, seams, mask, m.ng, rst.BAR, what)
        worst_r = max(worst_r, distance(fused, want))
        # two-stream (one angle by definition)
        if nmus == 1:
            a2 = dict(a, inc_flux=a["inc_flux"] if inc else None)
            fused = tst.fused(pkg, k, cols, cloud, mask, t, True, top, inc)
            assert same(fused, tst.composed(pkg, k, cols, cloud, mask, t, top, inc)), what
            assert same(fused, tst.solve(pkg, a2, b2g, t, top)), what
            emis = tst.per_gpt(a["sfc_emis"], b2g, m.ng)

            def run2(c):
                x = scattering_cell(a0, c, mask, b2g, m.ng)
                ru, rd = lw_2stream_ref.restate(x["tau"], x["ssa"], x["g"], x["inc"], x["dec"], emis, x["sfc_source"], a2["inc_flux"], top)
                return [lw_2stream_ref.broadband(ru), lw_2stream_ref.broadband(rd)]
            want = run2(cloud)
            check_signal(run2, want, cloud, seams, mask, m.ng, FLUX_ATOL, what)
            worst_2 = max(worst_2, distance(fused, want))
    print("SEAM lw scattering nlay %d ncol %d seams %s: rescaled %.2e W m-2 from the restatement (bar %.1e), two-stream %.2e (bar %.0e)"
          % (nlay, ncol, seams_of(kinds, nlay, True), worst_r, rst.BAR, worst_2, FLUX_ATOL))
    assert worst_r <= rst.BAR and worst_2 <= FLUX_ATOL


# ------------------------------------------------------------------------------------------------
# longwave, float32
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlay,ncol", list(lw_general_cases(True)))
@pytest.mark.parametrize("which", ["fsck", "rrtmgp"])
def test_longwave_f32_equals_the_composition(pkg, gpu, models, which, nlay, ncol):
    """float32 device tensors, every longwave layer count, both orientations: lw_fluxes_allsky (masked or not) equals
    gas_optics + increment + rte_lw bit for bit, lw_fluxes_clear_allsky gives that and lw_fluxes; the clear columns hold
    the clear-sky call's bits and every cloudy column differs."""
    k, m = models[which]
    t = T(gpu, F4)
    cols = lw_columns(k, nlay, ncol)
    for top, one_stream, nmus, inc, masked, series, iso, tail in LW_WALK:
        pkg.set_solver_option("lw_series_terms", series)
        pkg.set_solver_option("lw_inc_flux_isotropic", iso)
        pkg.set_solver_option("lw_tail_split", tail)
        seams, cloud, mask = seam_case(which, ("lw_register",), nlay, ncol, top)
        mask = mask if masked else None
        what = (which, nlay, ncol, top, one_stream, nmus, inc, masked, series, iso, tail)
        f = f32t.lw_fused(pkg, k, cols, cloud, t, one_stream, nmus, inc, top, mask)
        assert all(np.all(np.isfinite(a)) for a in f), what
        assert same(f, f32t.lw_composed(pkg, k, cols, cloud, t, one_stream, nmus, inc, top, mask)), what
        clear = f32t.lw_fused(pkg, k, cols, None, t, nmus=nmus, inc=inc, top_at_1=top)
        assert same(clear, f32t.lw_composed(pkg, k, cols, None, t, nmus=nmus, inc=inc, top_at_1=top)), what
        both = f32t.lw_fused(pkg, k, cols, cloud, t, one_stream, nmus, inc, top, mask, clear=True)
        assert same(both[:2], f) and same(both[2:], clear), what
        keep, differ = ~cloud["cloudy"], differ_columns(cloud, mask, m.ng)
        assert all(np.array_equal(a[:, keep], b[:, keep]) for a, b in zip(f, clear)), what
        assert differ.any() and np.all(np.abs(f[0].astype(np.float64) - clear[0]).max(axis=0)[differ] > 0), what



@pytest.mark.parametrize("which,nlay,top_at_1", F32_ORACLE)
def test_longwave_f32_against_the_oracle(pkg, gpu, oracle_mod, models, which, nlay, top_at_1):
    """So that two equal wrong answers cannot pass: the fused float32 call against ah.oracle_lw_allsky's reference on the
    float32-rounded inputs, at helpers.lw_f32_bar (4 x the float32 restatement's own distance from the oracle, at least
    1e-4 W m-2), which stays 20 times below every seam layer's signal."""
    k, m = models[which]
    cols, cloud, ref, bar, low = f32_oracle_case(oracle_mod, m, k.get_press_min(), which, nlay, top_at_1)
    out = f32t.lw_fused(pkg, k, cols, cloud, T(gpu, F4), top_at_1=top_at_1)
    err = distance(out, ref)
    print("SEAM lw f32 %s nlay %d top %d: %.3e W m-2 from the oracle (bar %.3e), smallest seam-layer signal %.3g"
          % (which, nlay, top_at_1, err, bar, low))
    assert err < bar


# ------------------------------------------------------------------------------------------------
# shortwave
# ------------------------------------------------------------------------------------------------
def sw_columns(k, nlay, ncol):
    cols = synthetic.columns(3 + nlay, ncol, k.get_press_min(), nlay=nlay, shortwave=True)
    rng = np.random.default_rng(ncol + nlay)
    nb = k.get_nband()
    cols["alb_dir"], cols["alb_dif"] = rng.uniform(0.02, 0.6, (ncol, nb)), rng.uniform(0.02, 0.6, (ncol, nb))
    cols["scale"] = rng.uniform(0.97, 1.03, ncol)
    return {n: (r32(v) if isinstance(v, np.ndarray) and v.dtype == np.float64 else v) for n, v in cols.items()}



@pytest.mark.parametrize("nlay,ncol", SW_SHAPES)
def test_shortwave_fp64(pkg, gpu, oracle_mod, models, nlay, ncol):
    """sw_fluxes_allsky, the masked call and sw_fluxes_clear_allsky against the oracle at 10 FLUX_ATOL, against the
    composition at 1e-9 max(1, max|flux|); the clear-sky output is sw_fluxes bit for bit and the all-sky output the single
    call's; every cloudy column differs from the clear sky."""
    k, m = models["sw_wide"]
    t = T(gpu)
    cols = sw_columns(k, nlay, ncol)
    worst_o = worst_p = 0.0
    low = np.inf
    for delta, scale, masked, split, solver, top in sw_cases(nlay):
        pkg.set_solver_option("sw_tail_split", split)
        pkg.set_solver_option("sw_solver", solver)
        seams, cloud, mask = sw_seam_case(nlay, ncol, solver, top)
        mask = mask if masked else None
        what = (nlay, ncol, delta, scale, masked, split, solver, top)
        f = f32t.sw_fused(pkg, k, cols, cloud, t, bool(delta), top, bool(scale), mask=mask)
        c = f32t.sw_composed(pkg, k, cols, cloud, t, bool(delta), top, bool(scale), mask=mask)
        assert all(np.all(np.isfinite(a)) for a in f + c), what
        pair_bar = 1e-9 * max(1.0, float(np.max(np.abs(c[1]))))
        worst_p = max(worst_p, distance(f, c) / pair_bar)
        assert distance(f, c) <= pair_bar, what
        clear = f32t.sw_fused(pkg, k, cols, None, t, top_at_1=top, scale=bool(scale))
        both = f32t.sw_fused(pkg, k, cols, cloud, t, bool(delta), top, bool(scale), mask=mask, clear=True)
        assert same(both[:3], f) and same(both[3:], clear), what
        assert same(f32t.sw_fused(pkg, k, cols, cloud, t, bool(delta), top, bool(scale), with_dir=False, mask=mask), f[:2]), what
        differ = differ_columns(cloud, mask, m.ng)
        assert differ.any() and np.all(np.abs(f[0] - clear[0]).max(axis=0)[differ] > 0), what
        run = sh.sw_reference(oracle_mod, m, cols, bool(delta), mask, top, cols["scale"] if scale else None)
        ref = run(cloud)
        low = min(low, check_signal(run, ref, cloud, seams, mask, m.ng, BAR, what))
        worst_o = max(worst_o, distance(f, ref), distance(c, ref))
        assert distance(f, ref) < BAR and distance(c, ref) < BAR, (what, distance(f, ref), distance(c, ref))
        assert distance(clear, run(None)) < BAR, what
    print("SEAM sw fp64 nlay %d ncol %d: %.2e W m-2 from the oracle (bar %.0e), fused - composed %.2f of its bar, smallest seam-layer signal %.3g"
          % (nlay, ncol, worst_o, BAR, worst_p, low))


@pytest.mark.parametrize("nlay", SW_NLAY)
def test_shortwave_f32_is_as_close_as_the_composition(pkg, gpu, oracle_mod, models, nlay):
    """F = the fused float32 call, C = the float32 composition, R = the fp64 fused call on the same float32-rounded inputs,
    e(X) = per-column max over levels and fluxes of |X - R|, one cloud per column (pattern "one"), pooled over the cases of
    the layer count: max e(F) <= 2 max e(C), the same for the 99th percentile, and 20 max e(F) <= the smallest
    all-sky-minus-clear-sky signal of the oracle over the columns at least half of whose g-points see their cloud."""
    k, m = models["sw_wide"]
    t32, t64 = T(gpu, F4), T(gpu)
    ncol = sw_ncol(nlay)
    cols = sw_columns(k, nlay, ncol)
    ef, ec, signal = [], [], np.inf
    for delta, scale, masked, split, solver, top in sw_cases(nlay):
        pkg.set_solver_option("sw_tail_split", split)
        pkg.set_solver_option("sw_solver", solver)
        seams, cloud, mask = sw_seam_case(nlay, ncol, solver, top, "one")
        mask = mask if masked else None
        args = (bool(delta), top, bool(scale))
        f = f32t.sw_fused(pkg, k, cols, cloud, t32, *args, mask=mask)
        c = f32t.sw_composed(pkg, k, cols, cloud, t32, *args, mask=mask)
        r = f32t.sw_fused(pkg, k, cols, cloud, t64, *args, mask=mask)
        assert all(a.dtype == F4 for a in f) and all(np.all(np.isfinite(a)) for a in f + c + r)
        assert same(f32t.sw_fused(pkg, k, cols, cloud, t32, *args, with_dir=False, mask=mask), f[:2])
        ef.append(f32t.column_error(f, r)); ec.append(f32t.column_error(c, r))
        run = sh.sw_reference(oracle_mod, m, cols, bool(delta), mask, top, cols["scale"] if scale else None)
        differ = differ_columns(cloud, mask, m.ng)
        if differ.any():
            signal = min(signal, ah.smallest_cloud_signal(run(cloud), run(None), differ))
    ef, ec = np.concatenate(ef), np.concatenate(ec)
    fig = dict(nlay=nlay, columns=int(ef.size), max_eF=float(ef.max()), max_eC=float(ec.max()), p99_eF=float(np.percentile(ef, 99)),
               p99_eC=float(np.percentile(ec, 99)), signal=signal)
    print("SEAM sw f32 pooled " + json.dumps(fig))
    assert fig["max_eF"] <= 2 * fig["max_eC"] and fig["p99_eF"] <= 2 * fig["p99_eC"], fig
    assert np.isfinite(signal) and 20 * fig["max_eF"] <= signal, fig


# ------------------------------------------------------------------------------------------------
# condition 2: every seam gets tested
# ------------------------------------------------------------------------------------------------
def test_every_seam_is_covered():
    """Condition 2, from the case tables alone (no GPU work): seam_cases.check_every_seam_is_covered."""
    check_every_seam_is_covered()
