"""Single-precision longwave solver (ecckd_rte_lw_f32, _inc_flux_f32, _byband_f32) at every layer-count form of
launch_real() (kernels_rte_lw.hip): the padded register forms (<= 32, 48, 64, 80, 96 layers), the exact 60-layer form,
the overflow form beyond 96 layers (scratch ring, four g-points per shuffle), their series-3 twins and the fp32 tail
split; and in both precisions the overflow form's grid stride (more than kOverWaves x kOverCW columns) and the deepest
grid its LDS accumulators admit.

Every case is checked against the fp64 oracle run on the float32-rounded inputs with the same solver options.  The flux
bar of a case is derived, not guessed: 4 x the largest distance of helpers.lw_emulate (the kernel's recurrence restated
in float32) from the oracle, at least 1e-4 W m-2 (helpers.lw_f32_bar).  Every case also asserts that its bar is at most
1/20 of the oracle's flux change when one seam layer of the form is made transparent or top_at_1 is flipped
(helpers.lw_flux_changes), so that a bar can never be wide enough to hide a misplaced layer or orientation."""
import numpy as np
import pytest

import helpers
from helpers import EPS32_THRESH, FLUX_ATOL, r32

pytestmark = pytest.mark.gpu

LDS_BUDGET = 160 * 1024       # kLdsBudget (kernels.hpp)
OVER_CW = 16                  # kOverCW: columns per wave of the overflow form
OVER_WAVES = 2048             # kOverWaves: its grid
REPORT = []                   # (case, largest error, bar): printed at the end of the module (pytest -s)


@pytest.fixture(autouse=True)
def default_options(pkg):
    pkg.reset_solver_options()
    pkg.set_solver_option("lw_tail_split", 1)
    yield
    pkg.reset_solver_options()
    pkg.set_solver_option("lw_tail_split", 1)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for line in REPORT:
        print("LWF32 %-60s err %.3e  bar %.3e" % line)


def solver_case(rng, ng, nlay, ncol, top_at_1, b2g):
    """Random inputs (already float32-rounded, held in float64) with tau ~ 1 on the seam layers of the form."""
    tau = rng.uniform(0, 2, (ng, nlay, ncol)) * rng.choice([1e-9, 1e-3, 1.0], size=(ng, nlay, ncol))
    seams = helpers.lw_seam_layers(nlay, top_at_1)
    tau[:, seams, :] = rng.uniform(0.8, 1.2, (ng, len(seams), ncol))
    lay, inc, dec = (rng.uniform(1, 9, (ng, nlay, ncol)) for _ in range(3))
    emis = rng.uniform(0.7, 1.0, (ncol, b2g.shape[0]))
    gpt2band = np.concatenate([np.full(hi - lo + 1, b) for b, (lo, hi) in enumerate(b2g)])
    c = dict(tau=tau, lay=lay, inc=inc, dec=dec, sfc=rng.uniform(1, 9, (ng, ncol)), emis=emis)
    c = {k: r32(v) for k, v in c.items()}
    c["emis_gpt"] = np.ascontiguousarray(c["emis"][:, gpt2band].T)
    c["b2g"], c["seams"] = b2g, seams
    return c


def two_bands(ng):
    return np.array([[1, 3], [4, ng]], dtype=np.int32) if ng > 3 else np.array([[1, ng]], dtype=np.int32)


def to_space(gpu, host, dtype=np.float32):
    import torch
    if host:
        return lambda a: np.ascontiguousarray(a, dtype=dtype)
    return lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(gpu)


def run_gpu(pkg, gpu, c, top_at_1, nmus, dtype=np.float32, host=False, inc_flux=None, tau=None, byband=False):
    """rte_lw through the public API on NaN-filled outputs; returns (err, up, dn) as float64 numpy arrays
    (byband: (err, bnd_up, bnd_dn, up, dn))."""
    import torch
    t = to_space(gpu, host, dtype)
    ng, nlay, ncol = c["tau"].shape
    op = pkg.OpticalProps1scl(); op.tau = t(c["tau"] if tau is None else tau); op.band2gpt = c["b2g"]
    src = pkg.SourceFuncLW()
    src.lay_source, src.lev_source_inc, src.lev_source_dec, src.sfc_source = t(c["lay"]), t(c["inc"]), t(c["dec"]), t(c["sfc"])
    nan = lambda *shape: t(np.full(shape, np.nan))
    back = (lambda a: np.asarray(a, dtype=np.float64)) if host else (lambda a: a.cpu().numpy().astype(np.float64))
    kw = dict(inc_flux=t(inc_flux)) if inc_flux is not None else {}
    if byband:
        nb = c["b2g"].shape[0]
        fl = pkg.FluxesByband(nan(nb, nlay + 1, ncol), nan(nb, nlay + 1, ncol), flux_up=nan(nlay + 1, ncol),
                              flux_dn=nan(nlay + 1, ncol))
    else:
        fl = pkg.FluxesBroadband(nan(nlay + 1, ncol), nan(nlay + 1, ncol))
    err = pkg.rte_lw(op, top_at_1, src, t(c["emis"]), fl, n_gauss_angles=nmus, **kw)
    if not host:
        torch.cuda.synchronize()
    if byband:
        return err, back(fl.bnd_flux_up), back(fl.bnd_flux_dn), back(fl.flux_up), back(fl.flux_dn)
    return err, back(fl.flux_up), back(fl.flux_dn)


def oracle_args(c, sl=slice(None)):
    return (c["tau"][sl], c["lay"][sl], c["inc"][sl], c["dec"][sl], c["emis_gpt"][sl], c["sfc"][sl])


def oracle_kw(oracle_mod, series3=False, thresh=None, iso=0):
    """The oracle's options for the solver options the device runs with (its fp32 default threshold included)."""
    return dict(lw_series_terms=3 if series3 else 2, lw_tau_thresh=EPS32_THRESH if thresh is None else thresh,
                lw_inc_flux_isotropic=iso)


def check_f32(oracle_mod, name, c, got, top_at_1, nmus, series3=False, thresh=None, iso=0, inc_flux=None,
              sl=slice(None), teeth=True):
    """got = (up, dn) of the device against the oracle on the g-points `sl`; the bar derived by helpers.lw_f32_bar and
    its teeth asserted.  Returns the bar."""
    okw = oracle_kw(oracle_mod, series3, thresh, iso)
    opt = oracle_mod.solver_options(**okw)
    inc = None if inc_flux is None else inc_flux[sl]
    ref = oracle_mod.rte_lw(*oracle_args(c, sl), top_at_1=top_at_1, nmus=nmus, inc_flux=inc, options=opt)
    case = dict(zip(("tau", "lay", "inc", "dec", "emis_gpt", "sfc"), oracle_args(c, sl)))
    bar = helpers.lw_f32_bar(case, top_at_1, nmus, ref, series3=series3,
                             tau_thresh=EPS32_THRESH if thresh is None else thresh, inc_flux=inc, inc_isotropic=bool(iso))
    if teeth:
        changes = helpers.lw_flux_changes(oracle_mod, case, top_at_1, nmus, ref, c["seams"], inc_flux=inc, options=opt)
        assert all(bar <= ch / 20 for ch in changes.values()), (bar, changes)
    err = 0.0
    for a, b in zip(got, ref):
        assert np.array_equal(np.isfinite(a), np.isfinite(b)), name
        ok = np.isfinite(b)
        err = max(err, float(np.max(np.abs(a - b)[ok], initial=0.0)))
    REPORT.append((name, err, bar))
    assert err < bar, (name, err, bar)
    return bar


# ---------------------------------------------------------------------------------------------------------------
# 2. the single-precision solver matrix
# ---------------------------------------------------------------------------------------------------------------
NLAYS = [1, 5, 32, 33, 48, 59, 60, 61, 64, 65, 80, 81, 91, 96, 97, 137, 200]


@pytest.mark.parametrize("series3", [False, True])
@pytest.mark.parametrize("i,nlay", list(enumerate(NLAYS)))
def test_f32_layer_counts(pkg, gpu, oracle_mod, i, nlay, series3):
    """Every layer-count form of launch_real() in float32, series 2 and series 3: ng = 7 over two unequal bands,
    alternating orientation, 1-4 angles, ragged column counts (one column in a few cases)."""
    top_at_1, nmus = i % 2 == 0, 1 + i % 4
    ncol = 1 if nlay in (5, 64, 137) and not series3 else 77
    rng = np.random.default_rng(100 * nlay + series3)
    c = solver_case(rng, 7, nlay, ncol, top_at_1, two_bands(7))
    if series3:
        pkg.set_solver_option("lw_series_terms", 3)
    err, up, dn = run_gpu(pkg, gpu, c, top_at_1, nmus)
    assert err == ""
    check_f32(oracle_mod, "nlay %d ser%d top %d nmus %d ncol %d" % (nlay, 3 if series3 else 2, top_at_1, nmus, ncol),
              c, (up, dn), top_at_1, nmus, series3=series3)


@pytest.mark.parametrize("nlay", [60, 137])
@pytest.mark.parametrize("ng", [1, 67])
def test_f32_g_point_counts(pkg, gpu, oracle_mod, nlay, ng):
    """One g-point (half of every group idle) and 67 over three bands (more g-points than one wave holds)."""
    b2g = np.array([[1, 1]], dtype=np.int32) if ng == 1 else np.array([[1, 20], [21, 50], [51, 67]], dtype=np.int32)
    top_at_1 = nlay == 60
    c = solver_case(np.random.default_rng(ng * nlay), ng, nlay, 77, top_at_1, b2g)
    err, up, dn = run_gpu(pkg, gpu, c, top_at_1, 2)
    assert err == ""
    check_f32(oracle_mod, "ng %d nlay %d" % (ng, nlay), c, (up, dn), top_at_1, 2)


@pytest.mark.parametrize("nlay,top_at_1,nmus", [(40, True, 2), (91, False, 3), (137, True, 1)])
def test_f32_incident_flux_and_byband(pkg, gpu, oracle_mod, nlay, top_at_1, nmus):
    """ecckd_rte_lw_inc_flux_f32 with both lw_inc_flux_isotropic values, and ecckd_rte_lw_byband_f32: each band against
    the oracle on its own g-points, the band sums against the broadband call."""
    ng = 11
    b2g = np.array([[1, 2], [3, 3], [4, 8], [9, 11]], dtype=np.int32)
    c = solver_case(np.random.default_rng(7 * nlay), ng, nlay, 130, top_at_1, b2g)
    incf = r32(np.random.default_rng(nlay).uniform(0, 30, (ng, 130)))
    for iso in (0, 1):
        pkg.set_solver_option("lw_inc_flux_isotropic", iso)
        err, up, dn = run_gpu(pkg, gpu, c, top_at_1, nmus, inc_flux=incf)
        assert err == ""
        check_f32(oracle_mod, "inc_flux iso %d nlay %d" % (iso, nlay), c, (up, dn), top_at_1, nmus, iso=iso, inc_flux=incf)
    pkg.set_solver_option("lw_inc_flux_isotropic", 0)
    err, bb_up, bb_dn = run_gpu(pkg, gpu, c, top_at_1, nmus)
    assert err == ""
    check_f32(oracle_mod, "broadband nlay %d" % nlay, c, (bb_up, bb_dn), top_at_1, nmus)
    err, bup, bdn, sup, sdn = run_gpu(pkg, gpu, c, top_at_1, nmus, byband=True)
    assert err == ""
    for b, (lo, hi) in enumerate(b2g):
        sl = slice(lo - 1, hi)
        check_f32(oracle_mod, "byband %d nlay %d" % (b, nlay), c, (bup[b], bdn[b]), top_at_1, nmus, sl=sl)
    # band sums against the broadband call: the two calls group and round the g-points differently, by as much as the
    # float32 restatement predicts for the same two calls (band fluxes rounded to float32 and summed in float32)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    emu = lambda sl: helpers.lw_emulate(*oracle_args(c, sl), top_at_1, nmus, np.float32, tau_thresh=EPS32_THRESH)
    e_bb = [f32(x) for x in emu(slice(None))]
    e_sum = [np.zeros_like(x) for x in e_bb]
    for lo, hi in b2g:
        for s_, x in zip(e_sum, emu(slice(lo - 1, hi))):
            s_ += f32(x)
    gap = max(float(np.max(np.abs(a.astype(np.float64) - b))) for a, b in zip(e_sum, e_bb))
    tol = max(4 * gap, 8 * np.finfo(np.float32).eps * np.max(np.abs(bb_up)))
    REPORT.append(("band sums - broadband nlay %d" % nlay, max(np.max(np.abs(sup - bb_up)), np.max(np.abs(sdn - bb_dn))), tol))
    assert np.max(np.abs(sup - bb_up)) < tol and np.max(np.abs(sdn - bb_dn)) < tol
    eps_sum = 4 * np.finfo(np.float32).eps * len(b2g)
    assert np.max(np.abs(sup - bup.sum(0))) < eps_sum * np.max(np.abs(sup))
    assert np.max(np.abs(sdn - bdn.sum(0))) < eps_sum * np.max(np.abs(sdn))


@pytest.mark.parametrize("nlay", [91, 137])
def test_f32_host_arrays_give_the_device_bits(pkg, gpu, oracle_mod, nlay):
    """numpy float32 arrays (the ECCKD_HOST arena sized with esz(); beyond 96 layers the overflow ring is taken on the
    null stream) give the same bits as device arrays."""
    c = solver_case(np.random.default_rng(nlay + 5), 7, nlay, 301, False, two_bands(7))
    err, up, dn = run_gpu(pkg, gpu, c, False, 2)
    herr, hup, hdn = run_gpu(pkg, gpu, c, False, 2, host=True)
    assert err == herr == ""
    assert np.array_equal(up, hup) and np.array_equal(dn, hdn)
    check_f32(oracle_mod, "host nlay %d" % nlay, c, (hup, hdn), False, 2)


@pytest.mark.parametrize("nlay,top_at_1", [(40, False), (137, True)])
def test_f32_solver_switches(pkg, gpu, oracle_mod, nlay, top_at_1):
    """lw_series_terms = 3 with a non-default lw_tau_thresh; the oracle runs with the same options."""
    thresh = 2e-3
    c = solver_case(np.random.default_rng(nlay + 11), 7, nlay, 77, top_at_1, two_bands(7))
    pkg.set_solver_option("lw_series_terms", 3)
    pkg.set_solver_option("lw_tau_thresh", thresh)
    err, up, dn = run_gpu(pkg, gpu, c, top_at_1, 3)
    assert err == ""
    check_f32(oracle_mod, "ser3 thresh %g nlay %d" % (thresh, nlay), c, (up, dn), top_at_1, 3, series3=True, thresh=thresh)


@pytest.mark.parametrize("nlay", [40, 137])
def test_f32_extreme_and_nan_columns(pkg, gpu, oracle_mod, nlay):
    """The fp32 counterpart of test_longwave_solver_extreme_and_nan_columns: the single-precision solver takes expf and
    `/`.  Whole columns of tau 0, a float32 subnormal, just below / above sqrt(eps32)/D, 1e30 and inf stay within the bar
    and finite; NaN and inf in single cells of two columns give NaN exactly where the oracle has it, and every other
    column keeps the bits of the clean run."""
    ng, ncol, top_at_1 = 7, 96, nlay == 40
    c = solver_case(np.random.default_rng(nlay + 78), ng, nlay, ncol, top_at_1, two_bands(ng))
    D = helpers.GAUSS_DS[0][0]
    tau = c["tau"]
    tau[:, :, 0] = 0.0
    tau[:, :, 1] = float(np.float32(1e-40))                  # subnormal in float32
    tau[:, :, 2] = r32(0.98 * EPS32_THRESH / D)
    tau[:, :, 3] = r32(1.02 * EPS32_THRESH / D)
    tau[:, :, 4] = 1e30
    tau[:, :, 5] = np.inf
    tau[:, nlay // 2, 6] = 1e30
    err, up, dn = run_gpu(pkg, gpu, c, top_at_1, 1)
    assert err == ""
    assert np.all(np.isfinite(up)) and np.all(np.isfinite(dn))
    check_f32(oracle_mod, "extreme columns nlay %d" % nlay, c, (up, dn), top_at_1, 1)
    bad = c["tau"].copy()
    bad[2, nlay // 3, 9] = np.nan
    bad[ng - 1, nlay - 1, 11] = np.inf
    bad[ng - 1, 0, 12] = np.nan                              # the last g-point: the idle lane of its group repeats it
    err, hu, hd = run_gpu(pkg, gpu, c, top_at_1, 1, tau=bad)
    assert err == ""
    opt = oracle_mod.solver_options(**oracle_kw(oracle_mod))
    fu, fd = oracle_mod.rte_lw(bad, c["lay"], c["inc"], c["dec"], c["emis_gpt"], c["sfc"], top_at_1=top_at_1, nmus=1, options=opt)
    keep = np.ones(ncol, bool); keep[[9, 11, 12]] = False
    assert np.array_equal(hu[:, keep], up[:, keep]) and np.array_equal(hd[:, keep], dn[:, keep])
    for a, b in ((hu, fu), (hd, fd)):
        assert np.array_equal(np.isnan(a), np.isnan(b))
        assert np.any(np.isnan(b))


# ---------------------------------------------------------------------------------------------------------------
# 3. tile loop and depth edges (both precisions)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("top_at_1", [True, False])
def test_overflow_grid_stride(pkg, gpu, oracle_mod, f32, top_at_1):
    """More columns than the overflow form's grid holds (kOverWaves waves of kOverCW columns): each wave solves a second
    tile on the same scratch ring and LDS accumulators.  Every column is written (NaN-filled outputs) and matches the
    oracle: fp64 to FLUX_ATOL, fp32 to its derived bar."""
    nlay, ng, nmus = 137, 4, 2
    ncol = OVER_WAVES * OVER_CW + 37
    c = solver_case(np.random.default_rng(ncol + top_at_1), ng, nlay, ncol, top_at_1, np.array([[1, 1], [2, 4]], np.int32))
    err, up, dn = run_gpu(pkg, gpu, c, top_at_1, nmus, dtype=np.float32 if f32 else np.float64)
    assert err == ""
    assert not np.any(np.isnan(up)) and not np.any(np.isnan(dn))
    if f32:
        check_f32(oracle_mod, "grid stride ncol %d top %d" % (ncol, top_at_1), c, (up, dn), top_at_1, nmus)
    else:
        fu, fd = oracle_mod.rte_lw(*oracle_args(c), top_at_1=top_at_1, nmus=nmus)
        assert np.max(np.abs(up - fu)) < FLUX_ATOL and np.max(np.abs(dn - fd)) < FLUX_ATOL


# Deepest grid: the overflow form (kOverCW = 16 columns per wave, padded: one dummy row) holds double accumulators
# [dn, up][nlay + 2][16] per wave -- 8 * 2 * (nlay + 2) * 16 = 256 * (nlay + 2) bytes -- and launch_ser refuses a call
# above kLdsBudget = 160 KiB: nlay + 2 <= 163840 / 256 = 640.
DEEPEST = LDS_BUDGET // (8 * 2 * OVER_CW) - 2


@pytest.mark.parametrize("f32", [False, True])
def test_deepest_accepted_grid_and_the_refusal_beyond(pkg, gpu, oracle_mod, f32):
    assert DEEPEST == 638
    ncol, ng, nmus, top_at_1 = 40, 3, 1, True
    c = solver_case(np.random.default_rng(DEEPEST + f32), ng, DEEPEST, ncol, top_at_1, np.array([[1, 3]], np.int32))
    dt = np.float32 if f32 else np.float64
    err, up, dn = run_gpu(pkg, gpu, c, top_at_1, nmus, dtype=dt)
    assert err == ""
    if f32:
        check_f32(oracle_mod, "deepest nlay %d" % DEEPEST, c, (up, dn), top_at_1, nmus)
    else:
        fu, fd = oracle_mod.rte_lw(*oracle_args(c), top_at_1=top_at_1, nmus=nmus)
        assert np.max(np.abs(up - fu)) < FLUX_ATOL and np.max(np.abs(dn - fd)) < FLUX_ATOL
    c1 = solver_case(np.random.default_rng(1), ng, DEEPEST + 1, ncol, top_at_1, np.array([[1, 3]], np.int32))
    err, up1, dn1 = run_gpu(pkg, gpu, c1, top_at_1, nmus, dtype=dt)
    assert err != ""
    assert np.all(np.isnan(up1)) and np.all(np.isnan(dn1))
    # the refusal leaves nothing behind: the next call at the deepest grid gives the same bits
    err, up2, dn2 = run_gpu(pkg, gpu, c, top_at_1, nmus, dtype=dt)
    assert err == "" and np.array_equal(up2, up) and np.array_equal(dn2, dn)


@pytest.mark.parametrize("ncol,nlay,ng,nmus,top_at_1", [
    (2000, 40, 27, 3, False),
    (33000, 91, 16, 2, True),
    (1013, 96, 7, 4, True),
    (3000, 64, 32, 1, False),
])
def test_f32_tail_split_is_bit_identical(pkg, gpu, oracle_mod, ncol, nlay, ng, nmus, top_at_1):
    """rte_lw_tail_plan / rte_lw_tail_reduce<float> at padded depths: the same bits as lw_tail_split = 0, and the split
    does happen (non-zero scratch; 2500 x 40 and 5000 x 64 would need more than the plan's 64 MiB of partials)."""
    assert pkg.rte_lw_tail_scratch_bytes(ncol, nlay, ng, n_gauss_angles=nmus, single_precision=True) > 0
    half = ng // 2
    c = solver_case(np.random.default_rng(ncol + nlay), ng, nlay, ncol, top_at_1,
                    np.array([[1, half], [half + 1, ng]], np.int32))
    out = {}
    for split in (1, 0):
        pkg.set_solver_option("lw_tail_split", split)
        out[split] = run_gpu(pkg, gpu, c, top_at_1, nmus)
        assert out[split][0] == ""
    pkg.set_solver_option("lw_tail_split", 1)
    assert np.array_equal(out[1][1], out[0][1]) and np.array_equal(out[1][2], out[0][2])
    assert not np.any(np.isnan(out[1][1])) and not np.any(np.isnan(out[1][2]))
    if ncol <= 2000:
        check_f32(oracle_mod, "tail split %dx%d ng %d" % (ncol, nlay, ng), c, out[1][1:], top_at_1, nmus)
