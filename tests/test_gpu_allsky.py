"""All-sky on the GPU: ecckd_increment / ecckd_delta_scale against the numpy restatement (tests/allsky_helpers.py) at the
derived round-off bars, the longwave and shortwave compositions and the fused ecckd_sw_fluxes_allsky against the C
oracle fed with numpy-incremented properties, and the fused call on caller-owned scratch and in a graph capture.

Measured on an MI355X, next to the bars (which are derived in allsky_helpers, not tuned):
  increments and delta scaling: 0 u in every case of test_increment_and_delta_scale, fp64 and f32, device and host arrays
  (bars 12 u and 74.2 u) -- the kernels reproduce numpy's IEEE evaluation bit for bit (the build has FMA contraction off and
  division is correctly rounded).  fp64 therefore asserts array_equal; f32 is held to the derived bars.
  longwave composition: 6.3e-13 / 4.6e-13 W m-2 from the oracle (bar 1e-8).
  shortwave, 60-137 layers: fused and composed 1.3e-10 ... 5.0e-9 W m-2 from the oracle (bar 1e-8; the distance is the
  solvers' own, the same in both); fused against composed <= 1.2e-13 W m-2 (bar 1.4e-6); extreme particles 2.2e-11."""
import numpy as np
import pytest

import allsky_helpers as ah
import helpers
from helpers import FLUX_ATOL
from rte_ecckd_amd import synthetic

pytestmark = pytest.mark.gpu
SW_NAMES = helpers.SW_NAMES


@pytest.fixture(autouse=True)
def default_options(pkg):
    pkg.reset_solver_options()
    pkg.set_solver_option("sw_solver", 0)
    pkg.set_solver_option("sw_tail_split", 1)
    pkg.set_arithmetic(pkg.FAST)
    yield
    pkg.reset_solver_options()
    pkg.set_solver_option("sw_solver", 0)
    pkg.set_solver_option("sw_tail_split", 1)
    pkg.set_arithmetic(pkg.FAST)


@pytest.fixture(scope="module")
def sw(pkg, gpu, oracle_mod):
    from conftest import SW_WIDE
    k = pkg.GasOpticsEcckd()
    assert k.load(SW_WIDE, device=0) == ""
    return k, oracle_mod.CkdModel(SW_WIDE)


def T(gpu):
    import torch
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def back(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def make(pkg, arrays, to):
    """OpticalProps1scl / 2str holding copies of `arrays` moved by `to`."""
    op = pkg.OpticalProps2str() if len(arrays) == 3 else pkg.OpticalProps1scl()
    op.tau = to(arrays[0].copy())
    if len(arrays) == 3:
        op.ssa, op.g = to(arrays[1].copy()), to(arrays[2].copy())
    return op


def values(op):
    return (back(op.tau),) + ((back(op.ssa), back(op.g)) if hasattr(op, "ssa") else ())


@pytest.mark.parametrize("table,ncol,nlay", [
    ("sw_wide", 1, 1), ("lw_fsck", 63, 60), ("lw_rrtmgp", 64, 137), ("sw_wide", 333, 60), ("lw_rrtmgp", 333, 1),
    ("lw_fsck", 64, 1), ("sw_wide", 63, 137), ("sw_wide", 20000, 60)])
def test_increment_and_delta_scale(pkg, gpu, table, ncol, nlay):
    """All four increments, on g-points and by band (band tables of the three ecCKD files: 5, 1 and 16 bands, bands of
    one g-point included), and delta scaling with and without `forward`; fp64 and f32; device and host arrays.  Bars:
    allsky_helpers (12 u, 74.2 u); cells whose expected value is 0 (tau = 0 under the eps floor) must be 0."""
    b2g, ng = ah.band_tables()[table]
    nb = b2g.shape[0]
    cloud = synthetic.clouds(3 * ncol, ncol, nlay, nb)
    rng = np.random.default_rng(ncol + nlay)
    worst_inc = worst_ds = 0.0
    spaces = [T(gpu)] + ([np.ascontiguousarray] if ncol <= 333 else [])
    for dt in (np.float64, np.float32):
        gas = tuple(a.astype(dt) for a in (
            rng.uniform(0, 2, (ng, nlay, ncol)) * rng.choice([0.0, 1e-6, 1.0], size=(ng, nlay, ncol)),
            rng.uniform(0, 1, (ng, nlay, ncol)), rng.uniform(0, 0.9, (ng, nlay, ncol))))
        part = tuple(cloud[n].astype(dt) for n in ("tau", "ssa", "g"))
        same = tuple(ah.spread(a, b2g, ng) for a in part)
        fwd = (dt(0.9) * part[2] * part[2]).astype(dt)
        for to in spaces:
            for op1 in (gas[:1], gas):
                for op2, bands in ((part[:1], b2g), (part, b2g), (same[:1], None), (same, None)):
                    a = make(pkg, op1, to)
                    assert a.increment(make(pkg, op2, to), band2gpt=bands) == ""
                    for got, want in zip(values(a), ah.increment(op1, op2, bands)):
                        assert got.dtype == dt
                        if dt is np.float64:
                            assert np.array_equal(got, want)     # (bit for bit: see the module docstring)
                        worst_inc = max(worst_inc, ah.worst_ulp(got, want))
            for f in (None, fwd):
                a = make(pkg, part, to)
                assert a.delta_scale(forward=None if f is None else to(f)) == ""
                for got, want in zip(values(a), ah.delta_scale(*part, forward=f)):
                    if dt is np.float64:
                        assert np.array_equal(got, want)
                    worst_ds = max(worst_ds, ah.worst_ulp(got, want))
    print("%s %d x %d: increments %.2f u (bar %d), delta scaling %.2f u (bar %.1f)" %
          (table, ncol, nlay, worst_inc, ah.INCREMENT_BAR_ULP, worst_ds, ah.DELTA_SCALE_BAR_ULP))
    assert worst_inc <= ah.INCREMENT_BAR_ULP and worst_ds <= ah.DELTA_SCALE_BAR_ULP


@pytest.mark.parametrize("which", ["fsck", "rrtmgp"])
def test_longwave_composition(pkg, gpu, oracle_mod, which):
    """gas_optics_lw -> increment (band two-stream cloud into the one-stream tau: absorption only) -> rte_lw against
    oracle.rte_lw on numpy-incremented tau, at 10 FLUX_ATOL (each side runs on its own optical properties)."""
    from conftest import LW_FSCK, LW_RRTMGP
    path = LW_FSCK if which == "fsck" else LW_RRTMGP
    k = pkg.GasOpticsEcckd()
    assert k.load(path, device=0) == ""
    m = oracle_mod.CkdModel(path)
    ncol, nlay, t = 333, 60, T(gpu)
    cols = synthetic.columns(9, ncol, k.get_press_min(), nlay=nlay)
    cloud = synthetic.clouds(9, ncol, nlay, k.get_nband())
    gc = helpers.product_gas_concs(pkg, cols, t)
    like = t(np.zeros(1))
    op = pkg.OpticalProps1scl(); op.alloc_1scl(ncol, nlay, k, like=like)
    src = pkg.SourceFuncLW(); src.alloc(ncol, nlay, k, like=like)
    assert k.gas_optics(None, t(cols["plev"]), t(cols["tlay"]), t(cols["tsfc"]), gc, op, src, tlev=t(cols["tlev"])) == ""
    part = make(pkg, (cloud["tau"], cloud["ssa"], cloud["g"]), t)
    assert op.increment(part, band2gpt=k.get_band2gpt()) == ""
    fl = pkg.FluxesBroadband(t(np.zeros((nlay + 1, ncol))), t(np.zeros((nlay + 1, ncol))))
    emis = t(np.repeat(cols["sfc_emis"][:, None], k.get_nband(), 1))
    assert pkg.rte_lw(op, True, src, emis, fl) == ""
    items = helpers.oracle_gas_items(cols)
    ref = ah.oracle_lw_allsky(oracle_mod, m, cols, items, cloud)
    clear = ah.oracle_lw_allsky(oracle_mod, m, cols, items, None)
    bar = 10 * FLUX_ATOL
    assert bar <= ah.smallest_cloud_signal(ref, clear, cloud["cloudy"]) / 20
    err = max(float(np.max(np.abs(back(a) - b))) for a, b in zip((fl.flux_up, fl.flux_dn), ref))
    print("longwave %s: %.2e W m-2 from the oracle (bar %.0e)" % (which, err, bar))
    assert err < bar


def sw_case(k, c0, ncol, nlay, seed, top_at_1=True):
    cols = synthetic.columns(c0, ncol, k.get_press_min(), nlay=nlay, shortwave=True)
    rng = np.random.default_rng(seed)
    nb = k.get_nband()
    cols["alb_dir"], cols["alb_dif"] = rng.uniform(0.02, 0.6, (ncol, nb)), rng.uniform(0.02, 0.6, (ncol, nb))
    cols["scale"] = rng.uniform(0.97, 1.03, ncol)
    cloud = synthetic.clouds(c0, ncol, nlay, nb)
    if not top_at_1:   # bottom-up arrays: the vertical axis of every profile reversed
        for n in ("plev", "tlay", "tlev", "h2o", "o3"):
            cols[n] = np.ascontiguousarray(cols[n][::-1])
        for n in ("tau", "ssa", "g"):
            cloud[n] = np.ascontiguousarray(cloud[n][:, ::-1])
    return cols, cloud


def fused(pkg, k, cols, cloud, to, delta, top_at_1=True, scale=False, with_dir=True):
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to, SW_NAMES)
    part = make(pkg, (cloud["tau"], cloud["ssa"], cloud["g"]), to)
    fl = pkg.FluxesBroadband(*(to(np.full((nlay + 1, ncol), -1.0)) for _ in range(3 if with_dir else 2)))
    assert k.sw_fluxes_allsky(to(cols["plev"]), to(cols["tlay"]), gc, top_at_1, to(cols["mu0"]), to(cols["alb_dir"]),
                              to(cols["alb_dif"]), part, fl, delta_scale=delta, toa_scale=to(cols["scale"]) if scale else None) == ""
    for a, b in zip(values(part), (cloud["tau"], cloud["ssa"], cloud["g"])):
        assert np.array_equal(a, b, equal_nan=True)                  # the caller's arrays are never written
    return [back(fl.flux_up), back(fl.flux_dn)] + ([back(fl.flux_dn_dir)] if with_dir else [])


def composed(pkg, k, cols, cloud, to, delta, top_at_1=True, scale=False):
    """gas_optics_sw -> (delta_scale of a copy) -> increment by band -> rte_sw through the API objects."""
    nlay, ncol = cols["tlay"].shape
    ng = k.get_ngpt()
    gc = helpers.product_gas_concs(pkg, cols, to, SW_NAMES)
    op = pkg.OpticalProps2str(); op.alloc_2str(ncol, nlay, k, like=to(np.zeros(1)))
    toa = to(np.empty((ng, ncol)))
    assert k.gas_optics(None, to(cols["plev"]), to(cols["tlay"]), gc, op, toa) == ""
    part = make(pkg, (cloud["tau"], cloud["ssa"], cloud["g"]), to)
    if delta:
        assert part.delta_scale() == ""
    assert op.increment(part, band2gpt=k.get_band2gpt()) == ""
    if scale:
        toa = toa * to(cols["scale"])[None, :]
    fl = pkg.FluxesBroadband(*(to(np.empty((nlay + 1, ncol))) for _ in range(3)))
    assert pkg.rte_sw(op, top_at_1, to(cols["mu0"]), toa, to(cols["alb_dir"]), to(cols["alb_dif"]), fl) == ""
    return [back(fl.flux_up), back(fl.flux_dn), back(fl.flux_dn_dir)]


@pytest.mark.parametrize("ncol,nlay,top_at_1,scale,solver", [
    (333, 60, True, False, 0), (1500, 61, True, True, 0), (333, 91, True, False, 0), (1500, 137, True, True, 0),
    (333, 60, True, True, 1), (700, 60, False, True, 0), (20000, 60, True, False, 0)])
def test_shortwave_compositions_and_fused(pkg, gpu, oracle_mod, sw, ncol, nlay, top_at_1, scale, solver):
    """gas_optics_sw -> increment -> rte_sw through the API, and the fused sw_fluxes_allsky, delta_scale 0 and 1: each
    against oracle.rte_sw on the numpy-incremented properties at 10 FLUX_ATOL (test_fused_sw_path's bar for the same
    comparison), fused against the API composition at 1e-9 max(1, max|flux|) (tests/test_gpu_sw_any_depth.py's bar
    between two solvers); without flux_dir; host arrays; a zero particulate array gives ecckd_sw_fluxes.  Bottom-up
    (profiles reversed: the gas optics takes negative layer masses, as in test_fused_sw_path) checks fused against
    composition only."""
    k, m = sw
    pkg.set_solver_option("sw_solver", solver)
    t = T(gpu)
    cols, cloud = sw_case(k, 7 * ncol, ncol, nlay, ncol + nlay, top_at_1)
    items = helpers.oracle_gas_items(cols, SW_NAMES)
    sc = cols["scale"] if scale else None
    clear = ah.oracle_sw_allsky(oracle_mod, m, cols, items, None, scale=sc) if top_at_1 and ncol <= 1500 else None
    for delta in (False, True):
        f = fused(pkg, k, cols, cloud, t, delta, top_at_1, scale)
        c = composed(pkg, k, cols, cloud, t, delta, top_at_1, scale)
        pair_bar = 1e-9 * max(1.0, float(np.max(np.abs(c[1])[~np.isnan(c[1])], initial=0.0)))
        for a, b in zip(f, c):   # (bottom-up: the negative layer masses make NaN fluxes, in the same places)
            assert np.array_equal(np.isnan(a), np.isnan(b)) and (top_at_1 is False or not np.isnan(a).any())
        pair_err = max(float(np.max(np.abs(a - b)[~np.isnan(b)], initial=0.0)) for a, b in zip(f, c))
        print("%d x %d delta %d: fused - composed %.2e (bar %.1e)" % (ncol, nlay, delta, pair_err, pair_bar))
        assert pair_err <= pair_bar
        two = fused(pkg, k, cols, cloud, t, delta, top_at_1, scale, with_dir=False)
        assert np.array_equal(two[0], f[0], equal_nan=True) and np.array_equal(two[1], f[1], equal_nan=True)
        if clear is not None:
            ref = ah.oracle_sw_allsky(oracle_mod, m, cols, items, cloud, delta=delta, scale=sc)
            bar = 10 * FLUX_ATOL
            assert bar <= ah.smallest_cloud_signal(ref, clear, cloud["cloudy"]) / 20
            ef = max(float(np.max(np.abs(a - b))) for a, b in zip(f, ref))
            ec = max(float(np.max(np.abs(a - b))) for a, b in zip(c, ref))
            print("%d x %d delta %d: fused %.2e, composed %.2e W m-2 from the oracle (bar %.0e)" % (ncol, nlay, delta, ef, ec, bar))
            assert ef < bar and ec < bar
            if ncol <= 333:
                h = fused(pkg, k, cols, cloud, np.ascontiguousarray, delta, top_at_1, scale)
                assert max(float(np.max(np.abs(a - b))) for a, b in zip(h, ref)) < bar
    if clear is not None:   # zero particulate optical depth: the fluxes of ecckd_sw_fluxes
        zero = dict(cloud, tau=np.zeros_like(cloud["tau"]))
        z = fused(pkg, k, cols, zero, t, True, top_at_1, scale)
        gc = helpers.product_gas_concs(pkg, cols, t, SW_NAMES)
        fl = pkg.FluxesBroadband(*(t(np.empty((nlay + 1, ncol))) for _ in range(3)))
        assert k.sw_fluxes(t(cols["plev"]), t(cols["tlay"]), gc, True, t(cols["mu0"]), t(cols["alb_dir"]), t(cols["alb_dif"]), fl,
                           toa_scale=t(cols["scale"]) if scale else None) == ""
        ez = max(float(np.max(np.abs(a - back(b)))) for a, b in zip(z, (fl.flux_up, fl.flux_dn, fl.flux_dn_dir)))
        print("zero particles against ecckd_sw_fluxes: %.2e" % ez)
        assert ez < 10 * FLUX_ATOL


def test_extreme_and_nan_particles(pkg, gpu, oracle_mod, sw):
    """Particulate tau of 0, 1e-12 and 1e4, ssa = 1, g = 0 stay within the flux bar of the oracle; a NaN in one column's
    cloud stays in that column."""
    k, m = sw
    ncol, nlay, t = 200, 60, T(gpu)
    cols, cloud = sw_case(k, 31, ncol, nlay, 5)
    cloud["tau"][:, :, 0] = 0.0
    cloud["tau"][:, :, 1] = 1e-12
    cloud["tau"][:, 40:44, 2] = 1e4
    cloud["tau"][:, 30:50, 3] = 5.0; cloud["ssa"][:, :, 3] = 1.0
    cloud["tau"][:, 30:50, 4] = 5.0; cloud["g"][:, :, 4] = 0.0
    cloud["tau"][:, 10:50, 5] = 20.0; cloud["ssa"][:, :, 5] = 1.0; cloud["g"][:, :, 5] = 0.0
    items = helpers.oracle_gas_items(cols, SW_NAMES)
    for delta in (False, True):
        ref = ah.oracle_sw_allsky(oracle_mod, m, cols, items, cloud, delta=delta)
        for out in (fused(pkg, k, cols, cloud, t, delta), composed(pkg, k, cols, cloud, t, delta)):
            err = max(float(np.max(np.abs(a - b))) for a, b in zip(out, ref))
            print("extreme particles, delta %d: %.2e W m-2 from the oracle" % (delta, err))
            assert all(np.all(np.isfinite(a)) for a in out) and err < 10 * FLUX_ATOL
    clean = fused(pkg, k, cols, cloud, t, True)
    bad = {n: v.copy() for n, v in cloud.items()}
    bad["tau"][2, 41, 17] = np.nan
    bad["ssa"][1, 35, 90] = np.nan
    out = fused(pkg, k, cols, bad, t, True)
    keep = np.ones(ncol, bool); keep[[17, 90]] = False
    for a, b in zip(out, clean):
        assert np.array_equal(a[:, keep], b[:, keep])
    assert np.all(np.isnan(out[0][:, 17])) and np.any(np.isnan(out[0][:, 90]))


def test_caller_owned_scratch_and_capture(pkg, gpu, sw):
    """sw_fluxes_allsky on a caller-owned block of exactly the size include/ecckd_hip.h documents -- what ecckd_sw_fluxes
    needs for the shape plus, with delta_scale, three band planes -- gives the eager bits
    (the scaled band planes, the solver's room and the optical depth do not overlap), one byte less is refused; a capture
    on one stream after a warm-up call replays to the eager bits."""
    import torch
    k, _ = sw
    ng, nb, t = k.get_ngpt(), k.get_nband(), T(gpu)
    align = lambda n: (n + 255) // 256 * 256
    for ncol, nlay, delta in ((1000, 137, True), (1000, 60, True), (70000, 60, False), (3000, 91, True)):
        cols, cloud = sw_case(k, 3, ncol, nlay, ncol)
        ref = fused(pkg, k, cols, cloud, t, delta, True, True)
        tail = pkg.rte_sw_tail_scratch_bytes(ncol, nlay, ng)
        solver = tail if nlay <= 60 else max(pkg.rte_sw_scratch_bytes(ncol, nlay, ng), tail)   # layer-systolic / two-pass
        need = align(ncol * nlay * ng * 8) + solver + (3 * align(ncol * nlay * nb * 8) if delta else 0)
        stream = torch.cuda.Stream()
        for size in (need, need - 1):
            buf = torch.full((size,), 0xFF, dtype=torch.uint8, device=gpu)   # (NaN patterns: stale data would show)
            torch.cuda.synchronize()
            pkg.set_stream_scratch(buf, stream=stream)
            try:
                with torch.cuda.stream(stream):
                    if size == need:
                        out = fused(pkg, k, cols, cloud, t, delta, True, True)
                        for a, b in zip(out, ref):
                            assert np.array_equal(a, b)
                    else:
                        gc = helpers.product_gas_concs(pkg, cols, t, SW_NAMES)
                        fl = pkg.FluxesBroadband(*(t(np.zeros((nlay + 1, ncol))) for _ in range(2)))
                        msg = k.sw_fluxes_allsky(t(cols["plev"]), t(cols["tlay"]), gc, True, t(cols["mu0"]), t(cols["alb_dir"]),
                                                 t(cols["alb_dif"]), make(pkg, (cloud["tau"], cloud["ssa"], cloud["g"]), t), fl,
                                                 delta_scale=delta)
                        assert "too small" in msg
                torch.cuda.synchronize()
            finally:
                pkg.set_stream_scratch(None, stream=stream)
        del buf
    ncol, nlay = 1000, 137
    cols, cloud = sw_case(k, 3, ncol, nlay, ncol)
    ref = fused(pkg, k, cols, cloud, t, True, True, True)
    gc = helpers.product_gas_concs(pkg, cols, t, SW_NAMES)
    part = make(pkg, (cloud["tau"], cloud["ssa"], cloud["g"]), t)
    args = (t(cols["plev"]), t(cols["tlay"]), gc, True, t(cols["mu0"]), t(cols["alb_dir"]), t(cols["alb_dif"]), part)
    scale = t(cols["scale"])
    fl = pkg.FluxesBroadband(*(t(np.zeros((nlay + 1, ncol))) for _ in range(3)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert k.sw_fluxes_allsky(*args, fl, delta_scale=True, toa_scale=scale) == ""   # warm-up: the stream's block exists now
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert k.sw_fluxes_allsky(*args, fl, delta_scale=True, toa_scale=scale) == ""
    for a in (fl.flux_up, fl.flux_dn, fl.flux_dn_dir):
        a.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip((fl.flux_up, fl.flux_dn, fl.flux_dn_dir), ref):
        assert np.array_equal(a.cpu().numpy(), b)
    del graph
    pkg.release_scratch(0)
