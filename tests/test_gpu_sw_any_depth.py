"""Shortwave at any layer count: single precision (ecckd_rte_sw_f32, _byband_f32) and the fused path (ecckd_sw_fluxes,
fp64 and fp32) beyond the 60 layers of the layer-systolic solver, and with "sw_solver" = 1, take the two-pass kernel
(kernels_rte_sw.hip: real = float and DERIVE instantiations).  Checked against the fp64 oracle, against the API pair
bit for bit, on caller-owned scratch of the size include/ecckd_hip.h gives, in a graph capture and through the Fortran
driver."""
import os
import subprocess

import numpy as np
import pytest

import helpers
from test_gpu_round2 import T, FLUX_ATOL
from test_gpu_round3 import SW_NAMES, sw_api_path, sw_fused_path, sw_inputs, run_sw, oracle_sw

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def default_options(pkg):
    pkg.reset_solver_options()
    pkg.set_solver_option("sw_solver", 0)
    pkg.set_solver_option("sw_tail_split", 1)
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


def columns(k, c0, ncol, nlay, rng):
    from rte_ecckd_amd import synthetic
    cols = synthetic.columns(c0, ncol, k.get_press_min(), nlay=nlay, shortwave=True)
    nband = k.get_nband()
    cols["alb_dir"] = rng.uniform(0.02, 0.6, (ncol, nband))
    cols["alb_dif"] = rng.uniform(0.02, 0.6, (ncol, nband))
    cols["scale"] = rng.uniform(0.97, 1.03, ncol)
    return cols


def t32(gpu):
    import torch
    return lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu)


def oracle_f32(oracle_mod, m, cols):
    """The fp64 oracle pair on the float32-rounded inputs: (tau, ssa, toa), [up, dn, dir]."""
    r = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32), dtype=np.float64)
    c32 = {n: (r(v) if isinstance(v, np.ndarray) else v) for n, v in cols.items()}
    otau, ossa, og, otoa, oerr = oracle_mod.gas_optics_ext(m, c32["plev"], c32["tlay"], helpers.oracle_gas_items(c32, SW_NAMES))
    assert oerr == ""
    g2b = m.gpt2band - 1
    ref = oracle_mod.rte_sw(otau, ossa, og, c32["mu0"], otoa, np.ascontiguousarray(c32["alb_dir"][:, g2b].T),
                            np.ascontiguousarray(c32["alb_dif"][:, g2b].T))
    return (otau, ossa, otoa), ref


def precision_limited_columns(tau, ssa, mu0, toa, above=0.05):
    """Columns whose direct-beam terms alone float32 cannot resolve to `above` W m-2: sw_two_stream's Rdir and Tdir (g = 0)
    evaluated in numpy in float32 and float64, the difference times the incoming beam, the worst cell of each column.  The
    terms divide by 1 - (k mu0)**2, which float32 resolves to a few digits only near k mu0 = 1 (the resonance: out of
    this file's scope); a deeper grid holds more cells, so more of its columns come near it."""
    res = {}
    with np.errstate(all="ignore"):
        for dt in (np.float64, np.float32):
            res[dt] = _direct_terms(dt, tau, ssa, mu0)
    err = np.maximum(np.abs(res[np.float32][0] - res[np.float64][0]), np.abs(res[np.float32][1] - res[np.float64][1]))
    return (err * (toa * mu0[None, :])[:, None, :]).max(axis=(0, 1)) > above


def _direct_terms(dt, tau, ssa, mu0):
    """Rdir, Tdir of sw_two_stream (g = 0) in precision dt.  (k^2 is floored at 1e-12 in both precisions here; the
    single-precision solvers floor it at min(1e-6, 1e-4 / tau^2), kSwKFloorF32 of capi.cpp.  That differs only in cells with ssa within
    1e-7 of 1, which this emulation therefore flags more readily than the solver errs: it only picks the columns that
    check_f32_bars holds to the wider bar.)"""
    t, w, mu = tau.astype(dt), ssa.astype(dt), mu0.astype(dt)[None, None, :]
    g1, g2 = (dt(8) - w * dt(5)) * dt(.25), dt(3) * w * dt(.25)
    k = np.sqrt(np.maximum((g1 - g2) * (g1 + g2), dt(1e-12)))
    e1 = np.exp(-t * k)
    e2 = e1 * e1
    tn = np.exp(-t / mu)
    kmu, a, kg = k * mu, g1 * dt(.5) + g2 * dt(.5), k * dt(.5)
    d = dt(1) - kmu * kmu
    eps = np.finfo(dt).eps
    rt = w / (k * (1 + e2) + g1 * (1 - e2)) / np.where(np.abs(d) >= eps, d, eps)
    rdir = rt * ((1 - kmu) * (a + kg) - (1 + kmu) * (a - kg) * e2 - 2 * (kg - a * kmu) * e1 * tn)
    tdir = -rt * ((1 + kmu) * (a + kg) * tn - (1 - kmu) * (a - kg) * e2 * tn - 2 * (kg + a * kmu) * e1)
    return rdir.astype(np.float64), tdir.astype(np.float64)


def oracle_mu0(cols):
    return np.asarray(cols["mu0"], dtype=np.float32).astype(np.float64)


def check_f32_bars(fluxes, ref, limited):
    """test_single_precision_sw_path's bars -- 0.5 W m-2 in the worst column, 0.05 W m-2 in 99 % of them -- over the
    columns that are not `limited` (precision_limited_columns); those, at most 5 % of a call, are held to 5 W m-2.
    Without the exemption the 600-column calls miss the bars at depth: 91 layers 2.32 W m-2 in one column (a cell
    2.4e-7 from the resonance; the float32 emulation predicts 2.31), 137 layers 0.052 W m-2 at the 99th percentile
    (the emulation flags 17 columns of 600 at 137 layers, 8 at 91, 7 at 60)."""
    assert limited.mean() <= 0.05, limited.mean()
    for a, b in zip(fluxes, ref):
        d = np.abs(np.asarray(a, dtype=np.float64) - b).max(axis=0)
        assert np.max(d[limited], initial=0.0) < 5.0, (np.flatnonzero(limited), d[limited])
        assert np.percentile(d[~limited], 99) < 0.05, np.percentile(d[~limited], 99)
        assert np.max(d[~limited]) < 0.5, (np.flatnonzero(~limited)[np.argmax(d[~limited])], np.max(d[~limited]))


@pytest.mark.parametrize("nlay", [61, 91, 137])
def test_f32_api_pair_beyond_60_layers(pkg, gpu, oracle_mod, sw, nlay):
    """gas_optics + rte_sw on float32 arrays where the layer-systolic solver does not apply (it refused before)."""
    import torch
    k, m = sw
    ncol = 600
    cols = columns(k, 3 * nlay, ncol, nlay, np.random.default_rng(nlay))
    api, op, toa = sw_api_path(pkg, k, cols, t32(gpu), np.float32)
    assert op.tau.dtype == torch.float32 and api[0].dtype == np.float32
    (otau, ossa, otoa), ref = oracle_f32(oracle_mod, m, cols)
    gt = op.tau.cpu().numpy().astype(np.float64)
    big = otau > 1e-6 * otau.max()
    assert np.max(np.abs(gt - otau)[big] / otau[big]) < 5e-5
    assert np.max(np.abs(op.ssa.cpu().numpy() - ossa)) < 5e-5
    check_f32_bars(api, ref, precision_limited_columns(otau, ossa, oracle_mu0(cols), otoa))


def test_f32_two_pass_at_60_layers(pkg, gpu, oracle_mod, sw):
    """fp32 with "sw_solver" = 1 at 60 layers: the two-pass kernel against the oracle and against the layer-systolic
    fp32 result, with the single-precision bars."""
    k, m = sw
    ncol = 900
    cols = columns(k, 11, ncol, 60, np.random.default_rng(2))
    sys_out, _, _ = sw_api_path(pkg, k, cols, t32(gpu), np.float32)
    pkg.set_solver_option("sw_solver", 1)
    try:
        two, _, _ = sw_api_path(pkg, k, cols, t32(gpu), np.float32)
    finally:
        pkg.set_solver_option("sw_solver", 0)
    (otau, ossa, otoa), ref = oracle_f32(oracle_mod, m, cols)
    res = precision_limited_columns(otau, ossa, oracle_mu0(cols), otoa)
    check_f32_bars(two, ref, res)
    check_f32_bars(two, [a.astype(np.float64) for a in sys_out], res)
    assert not all(np.array_equal(a, b) for a, b in zip(two, sys_out))   # (two solvers did run)


@pytest.mark.parametrize("ncol,nlay,top_at_1,scale,split", [
    (333, 91, True, False, 1), (1500, 137, True, True, 1), (700, 137, False, True, 1), (2000, 137, True, False, 0),
    (20000, 91, True, False, 1),
])
def test_fused_fp64_beyond_60_layers(pkg, gpu, oracle_mod, sw, ncol, nlay, top_at_1, scale, split):
    """ecckd_sw_fluxes beyond 60 layers gives the fluxes of gas_optics + rte_sw bit for bit (device and host arrays,
    with and without flux_dir, with and without toa_scale, bottom-up), and the oracle's within 10 FLUX_ATOL."""
    k, m = sw
    pkg.set_solver_option("sw_tail_split", split)
    cols = columns(k, 5 * ncol, ncol, nlay, np.random.default_rng(ncol + nlay))
    if not top_at_1:   # (as test_fused_sw_path: reversed profiles, only the bit-identity with the API pair is checked)
        for n in ("plev", "tlay", "tlev", "h2o", "o3"):
            cols[n] = np.ascontiguousarray(cols[n][::-1])
    t = T(gpu)
    api, _, _ = sw_api_path(pkg, k, cols, t, np.float64, top_at_1, scale)
    fused = sw_fused_path(pkg, k, cols, t, np.float64, top_at_1, scale)
    for a, b in zip(api, fused):
        assert np.array_equal(a, b, equal_nan=True)
    two = sw_fused_path(pkg, k, cols, t, np.float64, top_at_1, scale, with_dir=False)
    assert np.array_equal(two[0], fused[0], equal_nan=True) and np.array_equal(two[1], fused[1], equal_nan=True)
    if ncol <= 2000:
        host = sw_fused_path(pkg, k, cols, np.ascontiguousarray, np.float64, top_at_1, scale)
        for a, b in zip(host, fused):
            assert np.array_equal(a, b, equal_nan=True)
    if ncol <= 2000 and top_at_1:
        otau, ossa, og, otoa, oerr = oracle_mod.gas_optics_ext(m, cols["plev"], cols["tlay"], helpers.oracle_gas_items(cols, SW_NAMES))
        assert oerr == ""
        if scale:
            otoa = otoa * cols["scale"][None, :]
        g2b = m.gpt2band - 1
        ref = oracle_mod.rte_sw(otau, ossa, og, cols["mu0"], otoa, np.ascontiguousarray(cols["alb_dir"][:, g2b].T),
                                np.ascontiguousarray(cols["alb_dif"][:, g2b].T))
        for a, b in zip(fused, ref):
            assert np.max(np.abs(a - b)) < 10 * FLUX_ATOL


def test_fused_fp64_two_pass_at_60_layers(pkg, gpu, sw):
    """"sw_solver" = 1 at 60 layers: the fused path follows the two-pass API pair bit for bit."""
    k, _ = sw
    ncol = 1200
    cols = columns(k, 17, ncol, 60, np.random.default_rng(60))
    t = T(gpu)
    sys_fused = sw_fused_path(pkg, k, cols, t, np.float64, True, True)
    pkg.set_solver_option("sw_solver", 1)
    try:
        api, _, _ = sw_api_path(pkg, k, cols, t, np.float64, True, True)
        fused = sw_fused_path(pkg, k, cols, t, np.float64, True, True)
        host = sw_fused_path(pkg, k, cols, np.ascontiguousarray, np.float64, True, True)
    finally:
        pkg.set_solver_option("sw_solver", 0)
    for a, b, h, s in zip(api, fused, host, sys_fused):
        assert np.array_equal(a, b) and np.array_equal(h, b)
        assert np.max(np.abs(b - s)) < 1e-9 * max(1.0, float(np.max(np.abs(s))))   # the other solver: the last bits only


def test_fused_f32_137_layers(pkg, gpu, sw):
    """ecckd_sw_fluxes_f32 at 137 layers: the fluxes of the fp32 API pair bit for bit."""
    k, _ = sw
    ncol = 800
    cols = columns(k, 29, ncol, 137, np.random.default_rng(137))
    api, _, _ = sw_api_path(pkg, k, cols, t32(gpu), np.float32, True, True)
    fused = sw_fused_path(pkg, k, cols, t32(gpu), np.float32, True, True)
    for a, b in zip(api, fused):
        assert a.dtype == np.float32 and np.array_equal(a, b)
    host = sw_fused_path(pkg, k, cols, lambda a: np.ascontiguousarray(a, dtype=np.float32), np.float32, True, True)
    for a, b in zip(host, fused):
        assert np.array_equal(a, b)


def test_byband_f32_137_layers(pkg, gpu, oracle_mod, sw):
    """ecckd_rte_sw_byband_f32 at 137 layers: the band fluxes summed in band order are the broadband output, which
    agrees with the broadband fp32 call and with the oracle."""
    import torch
    k, m = sw
    ncol, nlay = 600, 137
    cols = columns(k, 3 * nlay, ncol, nlay, np.random.default_rng(nlay))
    t = t32(gpu)
    api, op, toa = sw_api_path(pkg, k, cols, t, np.float32)
    nband = k.get_nband()
    z = lambda *s: torch.full(s, -1.0, dtype=torch.float32, device=gpu)
    fb = pkg.FluxesByband(z(nband, nlay + 1, ncol), z(nband, nlay + 1, ncol), z(nband, nlay + 1, ncol),
                          z(nlay + 1, ncol), z(nlay + 1, ncol), z(nlay + 1, ncol))
    assert pkg.rte_sw(op, True, t(cols["mu0"]), toa, t(cols["alb_dir"]), t(cols["alb_dif"]), fb) == ""
    bands = [fb.bnd_flux_up.cpu().numpy(), fb.bnd_flux_dn.cpu().numpy(), fb.bnd_flux_dn_dir.cpu().numpy()]
    broad = [fb.flux_up.cpu().numpy(), fb.flux_dn.cpu().numpy(), fb.flux_dn_dir.cpu().numpy()]
    for bnd, tot, one in zip(bands, broad, api):
        acc = np.zeros_like(tot)
        for b in range(nband):
            acc += bnd[b]
        assert np.array_equal(acc, tot)
        assert np.max(np.abs(tot.astype(np.float64) - one)) < 0.05
    (otau, ossa, otoa), ref = oracle_f32(oracle_mod, m, cols)
    check_f32_bars(broad, ref, precision_limited_columns(otau, ossa, oracle_mu0(cols), otoa))


def test_extreme_and_nan_columns_137_layers(pkg, gpu, oracle_mod, sw):
    """As test_shortwave_solver_extreme_and_nan_columns, at 137 layers: fp32 optical depths from 1e-12 to 1e30 stay
    finite and near the oracle, a NaN / inf optical depth poisons its own column only; the fused fp64 path with an
    optically black column and a NaN cosine of the solar zenith angle keeps the other columns' bits and the API pair's bits."""
    rng = np.random.default_rng(77)
    ncol, nlay, ng = 200, 137, 9
    inp = list(sw_inputs(rng, ncol, nlay, ng, nband=2, g_zero=True))
    tau, ssa, mu0 = inp[0], inp[1], inp[3]
    tau[:, 10:13, 0] = 1.0e3
    tau[:, 20, 1] = 1.0e30
    tau[:, :, 2] = 1.0e-12
    ssa[:, :, 3] = 1.0 - 1.0e-6
    mu0[4] = 1.0e-3
    tau[:, :, 5] = 50.0; ssa[:, :, 5] = 0.999999
    f = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64) if isinstance(a, np.ndarray) and a.dtype == np.float64 else a
    inp = [f(a) for a in inp]
    ref = oracle_sw(oracle_mod, inp, True)

    def run32(data):
        import torch
        tau_, ssa_, g_, mu0_, toa_, albd, albf, b2g = data
        t = t32(gpu)
        op = pkg.OpticalProps2str(); op.tau, op.ssa, op.g = t(tau_), t(ssa_), t(g_)
        op.band2gpt = b2g
        fl = pkg.FluxesBroadband(*(torch.full((nlay + 1, ncol), -1., dtype=torch.float32, device=gpu) for _ in range(3)))
        assert pkg.rte_sw(op, True, t(mu0_), t(toa_), t(albd), t(albf), fl) == ""
        return [fl.flux_up.cpu().numpy(), fl.flux_dn.cpu().numpy(), fl.flux_dn_dir.cpu().numpy()]

    clean = run32(inp)
    res = precision_limited_columns(inp[0], inp[1], inp[3], inp[4])
    for a, b in zip(clean, ref):
        assert np.all(np.isfinite(a))
        assert np.max(np.abs(a - b)[:, ~res]) < 0.5 and np.max(np.abs(a - b)[:, res], initial=0.0) < 5.0
    bad = [x.copy() for x in inp]
    bad[0][3, 17, 7] = np.nan
    bad[0][5, 40, 8] = np.inf
    out = run32(bad)
    keep = np.ones(ncol, bool); keep[[7, 8]] = False
    for a, b in zip(out, clean):
        assert np.array_equal(a[:, keep], b[:, keep])
    assert np.all(np.isnan(out[0][:, 7])) and np.any(np.isnan(out[1][:, 7]))

    # fused fp64: extreme absorption (water vapour x 1e4 in column 0) and a NaN mu0 (column 1: gas optics clamps a NaN
    # temperature into its tables, so the NaN is handed to the solver directly)
    k, _ = sw
    nc = 300
    cols = columns(k, 0, nc, nlay, np.random.default_rng(5))
    cols["h2o"] = np.array(cols["h2o"], dtype=np.float64)
    cols["h2o"][:, 0] *= 1.0e4
    t = T(gpu)
    clean = sw_fused_path(pkg, k, cols, t, np.float64)
    for a in clean:
        assert np.all(np.isfinite(a))
    cols["mu0"] = cols["mu0"].copy()
    cols["mu0"][1] = np.nan
    fused = sw_fused_path(pkg, k, cols, t, np.float64)
    api, _, _ = sw_api_path(pkg, k, cols, t, np.float64)
    keep = np.ones(nc, bool); keep[1] = False
    for a, b, c in zip(fused, clean, api):
        assert np.array_equal(a, c, equal_nan=True)
        assert np.array_equal(a[:, keep], b[:, keep])
    assert np.any(np.isnan(fused[0][:, 1]))


def test_fused_scratch_sizing_and_capture_137_layers(pkg, gpu, sw):
    """ecckd_sw_fluxes on a stream with a caller-owned buffer of exactly the size include/ecckd_hip.h gives for the
    two-pass solver -- align256(tau) + max(ecckd_rte_sw_scratch_bytes, ecckd_rte_sw_tail_scratch_bytes) -- gives the
    eager bits (the solver's ring must not overwrite tau, which lives at the start of the same block); one byte less
    is refused; a capture on one stream after a warm-up call replays to the same bits."""
    import torch
    k, _ = sw
    ng = k.get_ngpt()
    t = T(gpu)
    for ncol, split in ((1000, 1), (1000, 0), (70000, 1)):
        pkg.set_solver_option("sw_tail_split", split)
        nlay = 137
        cols = columns(k, 7, ncol, nlay, np.random.default_rng(ncol))
        ref = sw_fused_path(pkg, k, cols, t, np.float64, True, True)
        align = lambda n: (n + 255) // 256 * 256
        need = align(ncol * nlay * ng * 8) + max(pkg.rte_sw_scratch_bytes(ncol, nlay, ng), pkg.rte_sw_tail_scratch_bytes(ncol, nlay, ng))
        assert (pkg.rte_sw_tail_scratch_bytes(ncol, nlay, ng) > 0) == (split == 1 and ncol == 1000)
        stream = torch.cuda.Stream()
        for size in (need, need - 1):
            buf = torch.full((size,), 0xFF, dtype=torch.uint8, device=gpu)   # (NaN patterns: stale data would show)
            torch.cuda.synchronize()
            pkg.set_stream_scratch(buf, stream=stream)
            try:
                with torch.cuda.stream(stream):
                    if size == need:
                        out = sw_fused_path(pkg, k, cols, t, np.float64, True, True)
                        for a, b in zip(out, ref):
                            assert np.array_equal(a, b)
                    else:
                        gc = helpers.product_gas_concs(pkg, cols, t, SW_NAMES)
                        fl = pkg.FluxesBroadband(*(t(np.zeros((nlay + 1, ncol))) for _ in range(2)))
                        msg = k.sw_fluxes(t(cols["plev"]), t(cols["tlay"]), gc, True, t(cols["mu0"]), t(cols["alb_dir"]),
                                          t(cols["alb_dif"]), fl, toa_scale=t(cols["scale"]))
                        assert "too small" in msg
                torch.cuda.synchronize()
            finally:
                pkg.set_stream_scratch(None, stream=stream)
        del buf
    # capture of the fused call on one stream (library-owned block, warmed up first), replayed once
    pkg.set_solver_option("sw_tail_split", 1)
    ncol, nlay = 1000, 137
    cols = columns(k, 7, ncol, nlay, np.random.default_rng(ncol))
    ref = sw_fused_path(pkg, k, cols, t, np.float64, True, True)
    gc = helpers.product_gas_concs(pkg, cols, t, SW_NAMES)
    args = (t(cols["plev"]), t(cols["tlay"]), gc, True, t(cols["mu0"]), t(cols["alb_dir"]), t(cols["alb_dif"]))
    scale = t(cols["scale"])
    fl = pkg.FluxesBroadband(*(t(np.zeros((nlay + 1, ncol))) for _ in range(3)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert k.sw_fluxes(*args, fl, toa_scale=scale) == ""   # warm-up: the stream's scratch block exists now
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert k.sw_fluxes(*args, fl, toa_scale=scale) == ""
    for a in (fl.flux_up, fl.flux_dn, fl.flux_dn_dir):
        a.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip((fl.flux_up, fl.flux_dn, fl.flux_dn_dir), ref):
        assert np.array_equal(a.cpu().numpy(), b)
    del graph
    pkg.release_scratch(0)


def test_fortran_fused_sw_91_layers(pkg, gpu, tmp_path):
    """ecckd_driver sw ... fused 1 on a 91-layer input (ecckd%sw_fluxes) gives the fluxes of the unfused block loop bit
    for bit."""
    from conftest import SW_WIDE
    from rte_ecckd_amd import synthetic
    from test_fortran_shim import write_input, read_output
    drv = pkg.FORTRAN_DRIVER if os.path.exists(pkg.FORTRAN_DRIVER) else pkg.build_fortran()
    if drv is None:
        pytest.skip("no Fortran driver binary and no amdflang")
    k = pkg.GasOpticsEcckd()
    assert k.load(SW_WIDE, device=0) == ""
    ncol, nlay = 250, 91
    cols = synthetic.columns(5, ncol, k.get_press_min(), nlay=nlay, shortwave=True)
    write_input(tmp_path / "in.bin", cols, synthetic.GAS_ORDER, True)
    out = {}
    for fused in ("0", "1"):
        r = subprocess.run([drv, "sw", SW_WIDE, str(tmp_path / "in.bin"), str(tmp_path / ("o%s.bin" % fused)), "100", "1", "0", "1", "0",
                            fused], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out[fused] = read_output(tmp_path / ("o%s.bin" % fused), ncol, nlay)
    assert np.array_equal(out["0"][0], out["1"][0]) and np.array_equal(out["0"][1], out["1"][1])
    assert np.all(np.isfinite(out["1"][0])) and np.all(np.isfinite(out["1"][1]))
