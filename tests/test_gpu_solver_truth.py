"""Every HIP solver route that takes optical properties directly, against independent multi-digit solutions of the
two-stream and Schwarzschild equations (tests/golden/solver_truth_{sw,lw}.npz; tests/solver_truth.py and
tests/golden/make_golden_solver_truth.py say how they are made, tests/test_solver_truth_host.py holds the oracle to
them).  The fixtures are read with numpy; nothing here needs mpmath or the oracle.

Bars: helpers.FLUX_ATOL for fp64; the bars recorded for `conservative` (4 x the oracle's distance) and `resonance`
(64 x 2^-53 / |1 - (k mu0)^2| of the incident flux); helpers.lw_f32_bar with the truth as reference for fp32 longwave;
the bars of tests/test_gpu_sw_any_depth.py for fp32 shortwave."""
import ctypes as C

import numpy as np
import pytest

import helpers
import truth_fixture as tf
from helpers import FLUX_ATOL
from test_solver_truth_host import (RESONANCE_FACTOR, drop_level, incident, lw_split_inputs, resonance_bar,
                                    sw_split_inputs)

pytestmark = pytest.mark.gpu

B2G = tf.BAND2GPT.astype(np.int32)
IMPLEMENTATION = ("lw_solver", "lw_split_seg", "lw_tail_split", "sw_solver", "sw_tail_split")
SW_F64 = [n for n, s in tf.sw_meta().items() if s["kind"] != "diffuse_in"]
SW_F32 = [n for n, s in tf.sw_meta().items() if s["f32"]]
LW_TAB = [(n, v) for n, s in tf.lw_meta().items() for v in s["variants"] if v.startswith("tab") and v.endswith("f64")]
LW_EXACT = [(n, v) for n, s in tf.lw_meta().items() for v in s["variants"] if v.startswith("exact")]
LW_F32 = [(n, v) for n, s in tf.lw_meta().items() for v in s["variants"] if v.endswith("f32")]


@pytest.fixture(autouse=True)
def default_options(pkg):
    """Every test starts from the defaults and leaves the implementation choices as it found them."""
    saved = {n: pkg.get_solver_option(n) for n in IMPLEMENTATION}
    pkg.reset_solver_options()
    pkg.set_arithmetic(pkg.FAST)
    yield
    pkg.reset_solver_options()
    pkg.set_arithmetic(pkg.FAST)
    for n, v in saved.items():
        pkg.set_solver_option(n, v)


def to_gpu(gpu, dtype=np.float64):
    import torch
    return lambda a: torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(gpu)   # (a copy: the fixtures are read-only)


def filled(gpu, dtype, *shape):
    import torch
    return torch.full(shape, -1.0, dtype=torch.float32 if dtype == np.float32 else torch.float64, device=gpu)


def back(a, top_at_1, axis):
    a = a.cpu().numpy().astype(np.float64)
    return a if top_at_1 else tf.flip(a, axis)


def run_sw(pkg, gpu, inp, top_at_1=True, dtype=np.float64, with_dir=True, byband=False):
    """ecckd_rte_sw / _f32 / _byband / _byband_f32 through the Python mirror; fluxes top first.  byband: (bnd_up, bnd_dn,
    bnd_dir, up, dn, dir)."""
    import torch
    t = to_gpu(gpu, dtype)
    a = [inp["tau"], inp["ssa"], inp["g"]]
    if not top_at_1:
        a = [tf.flip(x, 1) for x in a]
    ng, nlay, ncol = a[0].shape
    op = pkg.OpticalProps2str()
    op.tau, op.ssa, op.g = (t(x) for x in a)
    op.band2gpt = B2G
    bb = [filled(gpu, dtype, nlay + 1, ncol) for _ in range(3 if with_dir else 2)]
    if byband:
        bnd = [filled(gpu, dtype, 2, nlay + 1, ncol) for _ in range(3)]
        fl = pkg.FluxesByband(*bnd, *bb)
    else:
        fl = pkg.FluxesBroadband(*bb)
    err = pkg.rte_sw(op, top_at_1, t(inp["mu0"]), t(inp["toa"]), t(inp["alb_dir"]), t(inp["alb_dif"]), fl)
    assert err == "", err
    torch.cuda.synchronize()
    out = [back(x, top_at_1, 0) for x in bb]
    return ([back(x, top_at_1, 1) for x in bnd] + out) if byband else out


def sw_bar(name, inp):
    """Per-column bar of a shortwave set in fp64."""
    kind = tf.sw_meta()[name]["kind"]
    n = inp["mu0"].shape[0]
    if kind == "conservative":
        return np.full(n, tf.sw_meta()[name]["bar"])
    if kind == "resonance":
        return resonance_bar(inp)
    return np.full(n, FLUX_ATOL)


def col_distance(out, exp, names):
    return np.max([np.abs(o - exp[n]).reshape(-1, o.shape[-1]).max(axis=0) for o, n in zip(out, names)], axis=0)


# ------------------------------------------------------------------------------------------------
# shortwave, fp64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_at_1", [True, False])
@pytest.mark.parametrize("name", SW_F64)
def test_rte_sw(pkg, gpu, name, top_at_1):
    """ecckd_rte_sw: both solvers ("sw_solver" 0: layer-systolic up to 60 layers; 1 and every deeper call: two-pass), the
    tail split on and off, both arithmetic modes, flux_dir given and NULL, and on the `main` sets (where no layer
    leaves the clamp's range) "sw_dir_clamp" 1: every combination inside the set's bar."""
    inp, exp = tf.sw_set(name)
    bar = sw_bar(name, inp)
    worst = 0.0
    clamps = (0, 1) if tf.sw_meta()[name]["kind"] == "main" else (0,)
    for solver in (0, 1):
        for split in (1, 0):
            for mode in (pkg.FAST, pkg.REFERENCE_ORDER):
                for clamp in clamps:
                    for with_dir in (True, False):
                        pkg.set_solver_option("sw_solver", solver)
                        pkg.set_solver_option("sw_tail_split", split)
                        pkg.set_solver_option("sw_dir_clamp", clamp)
                        pkg.set_arithmetic(mode)
                        out = run_sw(pkg, gpu, inp, top_at_1, with_dir=with_dir)
                        d = col_distance(out, exp, ("up", "dn", "dir"))
                        worst = max(worst, float((d / bar).max()))
                        assert np.all(d < bar), (solver, split, mode, clamp, with_dir, float(d.max()), float(bar.min()))
    print("%s top_at_1=%d: largest distance %.3f of the bar (bar %.3e .. %.3e W m-2)" % (name, top_at_1, worst, bar.min(), bar.max()))
    if name == "resonance":
        d = col_distance(run_sw(pkg, gpu, inp, top_at_1), exp, ("up", "dn", "dir"))
        print("resonance: largest constant %.3f (bar %g)" % ((d * inp["d_min"] / (2.0 ** -53 * incident(inp))).max(), RESONANCE_FACTOR))


@pytest.mark.parametrize("name", [n for n, s in tf.sw_meta().items() if s["out"] == "bnd"])
def test_rte_sw_byband(pkg, gpu, name):
    """ecckd_rte_sw_byband: band fluxes against the truth's per-g-point fluxes summed by band (bands of two and of one
    g-point), the broadband outputs against the sum over all."""
    inp, exp = tf.sw_set(name)
    for top_at_1 in (True, False):
        for solver in (0, 1):
            pkg.set_solver_option("sw_solver", solver)
            out = run_sw(pkg, gpu, inp, top_at_1, byband=True)
            d = col_distance(out, exp, ("bnd_up", "bnd_dn", "bnd_dir", "up", "dn", "dir"))
            print("%s top_at_1=%d sw_solver=%d: %.3e W m-2" % (name, top_at_1, solver, d.max()))
            assert d.max() < FLUX_ATOL


@pytest.mark.parametrize("top_at_1", [True, False])
def test_sw_kernel_level_diffuse_in(pkg, gpu, top_at_1):
    """ecckd_sw_solver_2stream_gpt with a diffuse flux incident at the top: spectral fluxes against the truth, and
    ecckd_sum_broadband of them against its broadband sums."""
    import torch
    inp, exp = tf.sw_set("diffuse_in")
    t = to_gpu(gpu)
    a = [inp["tau"], inp["ssa"], inp["g"]]
    if not top_at_1:
        a = [tf.flip(x, 1) for x in a]
    ng, nlay, ncol = a[0].shape
    keep = [t(x) for x in a] + [t(inp["mu0"]), t(inp["toa"] * inp["mu0"][None, :]), t(inp["inc_dif"]),
                                t(tf.per_gpt(inp["alb_dir"])), t(tf.per_gpt(inp["alb_dif"]))]
    gpt = [filled(gpu, np.float64, ng, nlay + 1, ncol) for _ in range(3)]
    vp = lambda x: C.c_void_p(x.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = pkg.lib().ecckd_sw_solver_2stream_gpt(0, ncol, nlay, ng, int(top_at_1), *[vp(x) for x in keep], *[vp(x) for x in gpt],
                                               pkg.DEVICE, st)
    assert rc == 0, pkg.last_error()
    bb = [filled(gpu, np.float64, nlay + 1, ncol) for _ in range(3)]
    for s, b in zip(gpt, bb):
        rc = pkg.lib().ecckd_sum_broadband(0, ncol, nlay + 1, ng, vp(s), vp(b), pkg.DEVICE, st)
        assert rc == 0, pkg.last_error()
    torch.cuda.synchronize()
    d = col_distance([back(x, top_at_1, 1) for x in gpt] + [back(x, top_at_1, 0) for x in bb], exp,
                     ("gpt_up", "gpt_dn", "gpt_dir", "up", "dn", "dir"))
    print("diffuse_in top_at_1=%d: %.3e W m-2" % (top_at_1, d.max()))
    assert d.max() < FLUX_ATOL


# ------------------------------------------------------------------------------------------------
# longwave, fp64
# ------------------------------------------------------------------------------------------------
def run_lw(pkg, gpu, inp, variant, top_at_1=True, dtype=np.float64, entry="plain", byband=False):
    """ecckd_rte_lw (entry "plain"), _shared_levels ("shared"), _inc_flux ("inc": with the set's incident flux) and the
    _f32 / _byband forms through the Python mirror; fluxes top first."""
    import torch
    t = to_gpu(gpu, dtype)
    nmus = int(variant.split()[1])
    a = [inp["tau"], inp["lay"], inp["inc"], inp["dec"]]
    if not top_at_1:
        a = [tf.flip(inp["tau"], 1), tf.flip(inp["lay"], 1), tf.flip(inp["dec"], 1), tf.flip(inp["inc"], 1)]
    ng, nlay, ncol = a[0].shape
    op = pkg.OpticalProps1scl()
    op.tau, op.band2gpt = t(a[0]), B2G
    src = pkg.SourceFuncLW()
    src.lay_source, src.lev_source_inc, src.lev_source_dec, src.sfc_source = t(a[1]), t(a[2]), t(a[3]), t(inp["sfc_source"])
    bb = [filled(gpu, dtype, nlay + 1, ncol) for _ in range(2)]
    if byband:
        bnd = [filled(gpu, dtype, 2, nlay + 1, ncol) for _ in range(2)]
        fl = pkg.FluxesByband(*bnd, None, *bb)
    else:
        fl = pkg.FluxesBroadband(*bb)
    err = pkg.rte_lw(op, top_at_1, src, t(inp["sfc_emis"]), fl, n_gauss_angles=nmus, shared_levels=entry == "shared",
                     inc_flux=t(inp["inc_flux"]) if entry == "inc" else None)
    assert err == "", err
    torch.cuda.synchronize()
    out = [back(x, top_at_1, 0) for x in bb]
    return ([back(x, top_at_1, 1) for x in bnd] + out) if byband else out


def lw_routes(nlay):
    """(lw_solver, lw_split_seg, lw_tail_split) worth a launch at this depth: the layer-split solver serves 60 layers."""
    routes = [(0, 10, 1), (0, 10, 0)]
    if nlay == 60:
        routes += [(1, 10, 1), (1, 12, 1), (1, 15, 1), (1, 15, 0)]
    return routes


@pytest.mark.parametrize("name,variant", LW_TAB)
def test_rte_lw(pkg, gpu, name, variant):
    """ecckd_rte_lw and ecckd_rte_lw_shared_levels (no incident flux; the piecewise-linear source has one value per
    level) or ecckd_rte_lw_inc_flux (both "lw_inc_flux_isotropic" forms), both orientations, every solver route of the
    depth, both arithmetic modes; and the series switches (3 terms; 3 and 2 terms at the single-precision threshold),
    which change only rounding against the truth: all inside FLUX_ATOL."""
    inp, exp = tf.lw_set(name, variant)
    inc = variant.split()[2]
    entries = ("plain", "shared") if inc == "none" else ("inc",)
    worst = 0.0
    for top_at_1 in (True, False):
        for solver, seg, tail in lw_routes(inp["tau"].shape[1]):
            for mode, switches in ((pkg.FAST, {}), (pkg.REFERENCE_ORDER, {}), (pkg.FAST, dict(lw_series_terms=3)),
                                   (pkg.FAST, dict(lw_series_terms=3, lw_tau_thresh=helpers.EPS32_THRESH)),
                                   (pkg.FAST, dict(lw_tau_thresh=helpers.EPS32_THRESH))):
                pkg.reset_solver_options()
                for k, v in dict(switches, lw_solver=solver, lw_split_seg=seg, lw_tail_split=tail,
                                 lw_inc_flux_isotropic=int(inc == "isotropic")).items():
                    pkg.set_solver_option(k, v)
                pkg.set_arithmetic(mode)
                for entry in entries:
                    up, dn = run_lw(pkg, gpu, inp, variant, top_at_1, entry=entry)
                    d = max(np.abs(up - exp["up"]).max(), np.abs(dn - exp["dn"]).max())
                    worst = max(worst, d)
                    assert d < FLUX_ATOL, (top_at_1, solver, seg, tail, mode, switches, entry, d)
    print("%s %s: largest distance %.3e W m-2" % (name, variant, worst))


@pytest.mark.parametrize("name,variant", [c for c in LW_TAB if tf.lw_meta()[c[0]]["bnd"] and c[1].split()[2] == "none"])
def test_rte_lw_byband(pkg, gpu, name, variant):
    """ecckd_rte_lw_byband: band fluxes against the truth's per-g-point fluxes summed by band, and the broadband sums."""
    inp, exp = tf.lw_set(name, variant)
    for top_at_1 in (True, False):
        out = run_lw(pkg, gpu, inp, variant, top_at_1, byband=True)
        d = col_distance(out, exp, ("bnd_up", "bnd_dn", "up", "dn")).max()
        print("%s %s top_at_1=%d: %.3e W m-2" % (name, variant, top_at_1, d))
        assert d < FLUX_ATOL


@pytest.mark.parametrize("name,variant", LW_EXACT)
def test_lw_kernel_level_exact_nodes(pkg, gpu, name, variant):
    """ecckd_lw_solver_noscat_gpt handed the exact Gauss-Jacobi nodes (rounded to float64; one angle: secant 1.5, not
    the table's 1.66) and an incident flux: spectral fluxes against the truth for those nodes."""
    import torch
    inp, exp = tf.lw_set(name, variant)
    nmus = int(variant.split()[1])
    Ds, wts = tf.exact_quadrature(nmus)
    t = to_gpu(gpu)
    vp = lambda x: C.c_void_p(x.data_ptr())
    for top_at_1 in (True, False):
        a = [inp["tau"], inp["lay"], inp["inc"], inp["dec"]]
        if not top_at_1:
            a = [tf.flip(inp["tau"], 1), tf.flip(inp["lay"], 1), tf.flip(inp["dec"], 1), tf.flip(inp["inc"], 1)]
        ng, nlay, ncol = a[0].shape
        keep = [t(Ds), t(wts)] + [t(x) for x in a] + [t(inp["emis_gpt"]), t(inp["sfc_source"]), t(inp["inc_flux"])]
        gpt = [filled(gpu, np.float64, ng, nlay + 1, ncol) for _ in range(2)]
        rc = pkg.lib().ecckd_lw_solver_noscat_gpt(0, ncol, nlay, ng, int(top_at_1), nmus, *[vp(x) for x in keep], *[vp(x) for x in gpt],
                                                  pkg.DEVICE, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, pkg.last_error()
        torch.cuda.synchronize()
        d = col_distance([back(x, top_at_1, 1) for x in gpt], exp, ("gpt_up", "gpt_dn")).max()
        print("%s %s top_at_1=%d: %.3e W m-2" % (name, variant, top_at_1, d))
        assert d < FLUX_ATOL


# ------------------------------------------------------------------------------------------------
# single precision: the truth of the float32 image of the inputs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SW_F32)
def test_rte_sw_f32(pkg, gpu, name):
    """ecckd_rte_sw_f32 (and _byband_f32 where the set stores band fluxes), both solvers, both orientations, with the
    bars tests/test_gpu_sw_any_depth.py applies against the fp64 oracle -- 0.5 W m-2 in the worst column, 0.05 W m-2 in
    99 % of them -- and none of its exemptions: no column counts as precision-limited.
    `conservative` (ssa == 1 layers) was 11.6 W m-2 (8 layers) and 8.3 W m-2 (60 layers) off with k^2 floored at 1e-12:
    float keeps no digit of 1 - exp(-2 k tau) at k = 1e-6.  The single-precision solvers now floor k^2 at
    min(1e-6, 1e-4 / tau^2) per cell (capi.cpp, kSwKFloorF32; 1e-6 in every cell of these sets, tau <= 5).  Measured there
    against a constant floor: 1e-9 0.22 / 0.51, 1e-7 0.018 / 0.049, 1e-6 0.009 / 0.008,
    4e-6 0.014 / 0.009, 2.4e-5 0.009 / 0.030, 1e-4 0.036 / 0.12, 1.2e-3 0.42 / 1.46 W m-2; the other sets do not move.
    (4e-6 moved a 137-layer column of ssa = 1 - 1e-6, k^2 = 3e-6, by 1.3 W m-2: test_extreme_and_nan_columns_137_layers.)"""
    from test_gpu_sw_any_depth import check_f32_bars
    inp, exp = tf.sw_set(name, "f32")
    limited = np.zeros(inp["mu0"].shape[0], dtype=bool)
    byband = tf.sw_meta()[name]["out"] == "bnd"
    for top_at_1 in (True, False):
        for solver in (0, 1):
            pkg.set_solver_option("sw_solver", solver)
            out = run_sw(pkg, gpu, inp, top_at_1, np.float32, byband=byband)
            names = ("bnd_up", "bnd_dn", "bnd_dir", "up", "dn", "dir") if byband else ("up", "dn", "dir")
            ref = [exp[n].reshape(-1, exp[n].shape[-1]) for n in names]
            print("%s top_at_1=%d sw_solver=%d: %.3e W m-2 (%d columns limited)"
                  % (name, top_at_1, solver, col_distance(out, exp, names).max(), limited.sum()))
            check_f32_bars([o.reshape(-1, o.shape[-1]) for o in out], ref, limited)


@pytest.mark.parametrize("name,variant", LW_F32)
def test_rte_lw_f32(pkg, gpu, name, variant):
    """ecckd_rte_lw_f32, ecckd_rte_lw_inc_flux_f32 and ecckd_rte_lw_byband_f32 against the truth of the float32 image, bar
    helpers.lw_f32_bar with the truth in place of the oracle (4 x the float32 restatement's distance, at least
    1e-4 W m-2)."""
    inp, exp = tf.lw_set(name, variant)
    _, nmus, inc, _ = variant.split()
    case = dict(tau=inp["tau"], lay=inp["lay"], inc=inp["inc"], dec=inp["dec"], emis_gpt=inp["emis_gpt"], sfc=inp["sfc_source"])
    emu = {} if inc == "none" else dict(inc_flux=inp["inc_flux"])
    bar = helpers.lw_f32_bar(case, True, int(nmus), (exp["up"], exp["dn"]), **emu)
    for top_at_1 in (True, False):
        up, dn = run_lw(pkg, gpu, inp, variant, top_at_1, np.float32, entry="plain" if inc == "none" else "inc")
        d = max(np.abs(up - exp["up"]).max(), np.abs(dn - exp["dn"]).max())
        print("%s %s top_at_1=%d: %.3e W m-2, bar %.3e" % (name, variant, top_at_1, d, bar))
        assert d < bar
    if inc == "none" and "bnd_up" in exp:
        out = run_lw(pkg, gpu, inp, variant, True, np.float32, byband=True)
        d = col_distance(out, exp, ("bnd_up", "bnd_dn", "up", "dn")).max()
        print("%s %s byband: %.3e W m-2" % (name, variant, d))
        assert d < bar


# ------------------------------------------------------------------------------------------------
# layer splitting on the GPU
# ------------------------------------------------------------------------------------------------
def first_layers(inp, n):
    out = dict(inp)
    for k in ("tau", "ssa", "g"):
        if k in inp:
            out[k] = np.ascontiguousarray(inp[k][:, :n])
    return out


@pytest.mark.parametrize("nlay", [59, 60])
def test_rte_sw_layer_splitting(pkg, gpu, nlay):
    """A layer cut into two of half the optical depth: no flux at the original levels changes.  59 -> 60 layers stays in
    the layer-systolic solver, 60 -> 61 crosses to the two-pass kernel."""
    inp = first_layers(tf.sw_set("main_n60")[0], nlay)
    a = run_sw(pkg, gpu, inp)
    for l in (0, 2, nlay - 1):
        b = run_sw(pkg, gpu, sw_split_inputs(inp, l))
        d = max(np.abs(drop_level(y, l) - x).max() for x, y in zip(a, b))
        print("%d -> %d layers, layer %d: %.3e W m-2" % (nlay, nlay + 1, l, d))
        assert d < FLUX_ATOL


def test_rte_lw_layer_splitting(pkg, gpu):
    """96 -> 97 layers (register-resident to overflow form), the interpolated source at the new level."""
    full = tf.lw_set("n97")
    lev = np.ascontiguousarray(full["lev_source"][:, :97])
    inp = dict(full, tau=np.ascontiguousarray(full["tau"][:, :96]), lev_source=lev, inc=np.ascontiguousarray(lev[:, 1:]),
               dec=np.ascontiguousarray(lev[:, :-1]))
    inp["lay"] = 0.5 * (inp["inc"] + inp["dec"])
    v = "tab 3 none f64"
    a = run_lw(pkg, gpu, inp, v)
    for l in (0, 50, 95):
        b = run_lw(pkg, gpu, lw_split_inputs(inp, l), v)
        d = max(np.abs(drop_level(y, l) - x).max() for x, y in zip(a, b))
        print("96 -> 97 layers, layer %d: %.3e W m-2" % (l, d))
        assert d < FLUX_ATOL
