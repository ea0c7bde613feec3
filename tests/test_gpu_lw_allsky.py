"""The fused all-sky longwave call ecckd_lw_fluxes_allsky on the GPU, and the Fortran forms of both all-sky calls.

Bit-for-bit checks first (no tolerance: the fused call runs the same kernels and the same expressions as a composition
the library already offers): against gas_optics_tau + increment + rte_lw_fused, host arrays against device arrays, no
particles against the clear-sky call, both solver orientations.  Then the C oracle on numpy-incremented optical depth at
10 FLUX_ATOL = 1e-8 W m-2 (test_longwave_composition's bar for two sides that each run on their own optical properties),
every level of every column; NaN containment and extreme particles; caller-owned scratch and graph capture; the Fortran
driver with a particle file against the Python call (bit for bit) and the oracle.

Measured on an MI355X, next to the bars (which come from the issue and test_longwave_composition, not from these figures):
  every bit-for-bit case holds as an equality (192 combinations top-down, 128 bottom-up; host against device arrays; no
  particles against lw_fluxes; clear columns of a cloudy call; eager against caller-owned scratch and graph replay);
  against the oracle, all sixteen cases: 3.4e-13 ... 8.0e-13 W m-2 (32-g file 6.3e-13 ... 8.0e-13, 36-g file
  3.4e-13 ... 7.1e-13; one- and two-stream particles alike), bar 1e-8;
  extreme particles (tau_p = 0, 1e-12, 1e4; ssa_p = 0 and 1): 4.0e-13 (32-g) and 3.4e-13 (36-g) W m-2, bar 1e-8;
  Fortran driver: bit for bit the Python call; 3.4e-13 W m-2 (longwave) and 2.2e-11 W m-2 (shortwave) from the oracle."""
import os
import struct
import subprocess

import numpy as np
import pytest

import allsky_helpers as ah
import helpers
from helpers import FLUX_ATOL
from rte_ecckd_amd import synthetic

pytestmark = pytest.mark.gpu
BAR = 10 * FLUX_ATOL


@pytest.fixture(autouse=True)
def default_options(pkg):
    pkg.reset_solver_options()
    pkg.set_arithmetic(pkg.FAST)
    yield
    pkg.reset_solver_options()
    pkg.set_arithmetic(pkg.FAST)


@pytest.fixture(scope="module")
def lw(pkg, gpu, oracle_mod):
    from conftest import LW_FSCK, LW_RRTMGP
    out = {}
    for name, path in (("fsck", LW_FSCK), ("rrtmgp", LW_RRTMGP)):
        k = pkg.GasOpticsEcckd()
        assert k.load(path, device=0) == ""
        out[name] = (k, oracle_mod.CkdModel(path), path)
    return out


def T(gpu):
    import torch
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def back(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def particles(pkg, cloud, to, one_stream):
    """OpticalProps1scl (tau) or OpticalProps2str (tau, ssa, g) on bands holding copies of the cloud moved by `to`."""
    op = pkg.OpticalProps1scl() if one_stream else pkg.OpticalProps2str()
    op.tau = to(cloud["tau"].copy())
    if not one_stream:
        op.ssa, op.g = to(cloud["ssa"].copy()), to(cloud["g"].copy())
    return op


def case(k, c0, ncol, nlay, seed=None):
    cols = synthetic.columns(c0, ncol, k.get_press_min(), nlay=nlay)
    cloud = synthetic.clouds(c0, ncol, nlay, k.get_nband())
    rng = np.random.default_rng(ncol + nlay if seed is None else seed)
    cols["inc_flux"] = rng.uniform(0.0, 2.0, (k.get_ngpt(), ncol))
    cols["emis"] = np.repeat(cols["sfc_emis"][:, None], k.get_nband(), 1)
    return cols, cloud


def fused(pkg, k, cols, cloud, to, one_stream=False, nmus=1, inc=False, top_at_1=True):
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to)
    part = particles(pkg, cloud, to, one_stream)
    fl = pkg.FluxesBroadband(to(np.full((nlay + 1, ncol), -1.0)), to(np.full((nlay + 1, ncol), -1.0)))
    assert k.lw_fluxes_allsky(to(cols["plev"]), to(cols["tlay"]), to(cols["tsfc"]), to(cols["tlev"]), gc, top_at_1,
                              to(cols["emis"]), part, fl, n_gauss_angles=nmus,
                              inc_flux=to(cols["inc_flux"]) if inc else None) == ""
    assert np.array_equal(back(part.tau), cloud["tau"], equal_nan=True)          # the caller's arrays are never written
    if not one_stream:
        assert np.array_equal(back(part.ssa), cloud["ssa"], equal_nan=True)
    return [back(fl.flux_up), back(fl.flux_dn)]


def composed(pkg, k, cols, cloud, to, one_stream=False, nmus=1, inc=False, top_at_1=True):
    """gas_optics_tau -> OpticalProps1scl.increment(particles, band2gpt) -> rte_lw_fused, device tensors."""
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to)
    op = pkg.OpticalProps1scl(); op.alloc_1scl(ncol, nlay, k, like=to(np.zeros(1)))
    assert k.gas_optics_tau(to(cols["plev"]), to(cols["tlay"]), gc, op) == ""
    assert op.increment(particles(pkg, cloud, to, one_stream), band2gpt=k.get_band2gpt()) == ""
    fl = pkg.FluxesBroadband(to(np.full((nlay + 1, ncol), -2.0)), to(np.full((nlay + 1, ncol), -2.0)))
    assert k.rte_lw_fused(op, top_at_1, to(cols["tlay"]), to(cols["tlev"]), to(cols["tsfc"]), to(cols["emis"]), fl,
                          n_gauss_angles=nmus, inc_flux=to(cols["inc_flux"]) if inc else None) == ""
    return [back(fl.flux_up), back(fl.flux_dn)]


def clear_sky(pkg, k, cols, to, nmus=1, inc=False, top_at_1=True):
    nlay, ncol = cols["tlay"].shape
    gc = helpers.product_gas_concs(pkg, cols, to)
    fl = pkg.FluxesBroadband(to(np.full((nlay + 1, ncol), -3.0)), to(np.full((nlay + 1, ncol), -3.0)))
    assert k.lw_fluxes(to(cols["plev"]), to(cols["tlay"]), to(cols["tsfc"]), to(cols["tlev"]), gc, top_at_1, to(cols["emis"]),
                       fl, n_gauss_angles=nmus, inc_flux=to(cols["inc_flux"]) if inc else None) == ""
    return [back(fl.flux_up), back(fl.flux_dn)]


def oracle_lw(oracle_mod, m, cols, items, cloud, one_stream):
    """[up, dn] of the oracle: two-stream particles through ah.oracle_lw_allsky, one-stream particles the same with
    ah.increment((tau,), (cloud tau,), band2gpt); cloud None: clear sky."""
    if cloud is None or not one_stream:
        return ah.oracle_lw_allsky(oracle_mod, m, cols, items, cloud)
    tau, lay, inc, dec, sfc, oerr = oracle_mod.gas_optics_int(m, cols["plev"], cols["tlay"], cols["tsfc"], items, cols["tlev"])
    assert oerr == ""
    tau, = ah.increment((tau,), (cloud["tau"],), m.band2gpt)
    return list(oracle_mod.rte_lw(tau, lay, inc, dec, np.repeat(cols["sfc_emis"][None, :], m.ng, 0), sfc))


@pytest.mark.parametrize("ncol", [333, 777, 130, 1])
@pytest.mark.parametrize("nlay", [60, 37, 137])
@pytest.mark.parametrize("which", ["fsck", "rrtmgp"])
def test_fused_equals_its_building_blocks(pkg, gpu, lw, which, nlay, ncol):
    """lw_fluxes_allsky equals gas_optics_tau + increment (by band) + rte_lw_fused bit for bit: 1 and 3 angles, with and
    without inc_flux, two-stream and one-stream particles -- and, at 60 and 137 layers, the same with top_at_1 = False on
    both sides.  The gas optics takes plev(:,l+1) - plev(:,l) as the layer mass, so it assumes the top at index 1 itself;
    only the solver has another orientation, and the solver-only building block rte_lw_fused is tied to the oracle in both
    orientations by tests/test_gpu_round2.py::test_fused_lw_path_vs_oracle: bottom-up, the equality with the composition
    is the whole check and no oracle comparison is made."""
    k = lw[which][0]
    t = T(gpu)
    cols, cloud = case(k, 7 * ncol + nlay, ncol, nlay)
    for top_at_1 in ((True, False) if nlay in (60, 137) else (True,)):
        for one_stream in (False, True):
            for nmus in (1, 3):
                for inc in (False, True):
                    f = fused(pkg, k, cols, cloud, t, one_stream, nmus, inc, top_at_1)
                    c = composed(pkg, k, cols, cloud, t, one_stream, nmus, inc, top_at_1)
                    what = (which, nlay, ncol, top_at_1, one_stream, nmus, inc)
                    assert np.all(np.isfinite(f[0])) and np.all(np.isfinite(f[1])), what
                    assert np.array_equal(f[0], c[0]) and np.array_equal(f[1], c[1]), what


@pytest.mark.parametrize("which,ncol,nlay", [("fsck", 333, 60), ("rrtmgp", 130, 60), ("fsck", 130, 37), ("rrtmgp", 333, 37)])
def test_host_arrays_equal_device_arrays(pkg, gpu, lw, which, ncol, nlay):
    k = lw[which][0]
    cols, cloud = case(k, 11, ncol, nlay)
    for one_stream in (False, True):
        for nmus, inc in ((1, False), (3, True)):
            d = fused(pkg, k, cols, cloud, T(gpu), one_stream, nmus, inc)
            h = fused(pkg, k, cols, cloud, np.ascontiguousarray, one_stream, nmus, inc)
            assert np.array_equal(d[0], h[0]) and np.array_equal(d[1], h[1]), (one_stream, nmus, inc)


@pytest.mark.parametrize("which,ncol,nlay", [("fsck", 333, 60), ("rrtmgp", 777, 60), ("fsck", 130, 37), ("rrtmgp", 130, 137)])
def test_no_particles_no_change(pkg, gpu, lw, which, ncol, nlay):
    """tau_p = 0 everywhere gives lw_fluxes bit for bit (tau + 0*(1 - ssa) is tau); with synthetic.clouds the columns
    without a cloud equal the clear-sky call's columns bit for bit, and the cloudy ones do not."""
    k = lw[which][0]
    t = T(gpu)
    cols, cloud = case(k, 23, ncol, nlay)
    zero = dict(cloud, tau=np.zeros_like(cloud["tau"]))
    for nmus, inc in ((1, False), (3, True)):
        clear = clear_sky(pkg, k, cols, t, nmus, inc)
        for one_stream in (False, True):
            z = fused(pkg, k, cols, zero, t, one_stream, nmus, inc)
            assert np.array_equal(z[0], clear[0]) and np.array_equal(z[1], clear[1])
            f = fused(pkg, k, cols, cloud, t, one_stream, nmus, inc)
            keep = ~cloud["cloudy"]
            assert keep.any() and cloud["cloudy"].any()
            for a, b in zip(f, clear):
                assert np.array_equal(a[:, keep], b[:, keep])
            assert np.all(np.abs(f[0] - clear[0]).max(axis=0)[cloud["cloudy"]] > 0)


@pytest.mark.parametrize("c0,ncol,nlay", [(9, 333, 60), (21, 777, 60), (5, 130, 37), (5, 130, 137)])
@pytest.mark.parametrize("which", ["fsck", "rrtmgp"])
def test_against_the_oracle(pkg, gpu, oracle_mod, lw, which, c0, ncol, nlay):
    """Two-stream particles against ah.oracle_lw_allsky, one-stream particles against the same with
    ah.increment((tau,), (cloud tau,), band2gpt): every level of every column under 10 FLUX_ATOL = 1e-8 W m-2, which
    stays 20 times below the smallest all-sky-minus-clear signal of a cloudy column.
    Measured on an MI355X: 3.4e-13 ... 8.0e-13 W m-2 over the sixteen combinations (module docstring)."""
    k, m, _ = lw[which]
    cols = synthetic.columns(c0, ncol, k.get_press_min(), nlay=nlay)
    cloud = synthetic.clouds(c0, ncol, nlay, k.get_nband())
    cols["emis"] = np.repeat(cols["sfc_emis"][:, None], k.get_nband(), 1)
    items = helpers.oracle_gas_items(cols)
    clear = oracle_lw(oracle_mod, m, cols, items, None, False)
    for one_stream in (False, True):
        ref = oracle_lw(oracle_mod, m, cols, items, cloud, one_stream)
        assert all(np.all(np.isfinite(a)) for a in ref)
        assert BAR <= ah.smallest_cloud_signal(ref, clear, cloud["cloudy"]) / 20
        out = fused(pkg, k, cols, cloud, T(gpu), one_stream)
        err = max(float(np.max(np.abs(a - b))) for a, b in zip(out, ref))
        print("longwave all-sky %s %d x %d %s: %.2e W m-2 from the oracle (bar %.0e)" %
              (which, ncol, nlay, "one-stream" if one_stream else "two-stream", err, BAR))
        assert all(np.all(np.isfinite(a)) for a in out) and err < BAR


@pytest.mark.parametrize("which", ["fsck", "rrtmgp"])
def test_containment_and_extremes(pkg, gpu, oracle_mod, lw, which):
    """A NaN in one column's tau_p (or ssa_p) makes that column's fluxes NaN and leaves every other column bit-identical
    to the run without it; particulate optical depths of 0, 1e-12 and 1e4 stay within the bar of the oracle."""
    k, m, _ = lw[which]
    ncol, nlay, t = 200, 60, T(gpu)
    cols, cloud = case(k, 31, ncol, nlay)
    cloud["tau"][:, :, 0] = 0.0
    cloud["tau"][:, :, 1] = 1e-12
    cloud["tau"][:, 40:44, 2] = 1e4
    cloud["tau"][:, :, 3] = 1e4
    cloud["tau"][:, 10:50, 4] = 20.0; cloud["ssa"][:, :, 4] = 1.0
    cloud["tau"][:, 10:50, 5] = 20.0; cloud["ssa"][:, :, 5] = 0.0
    items = helpers.oracle_gas_items(cols)
    for one_stream in (False, True):
        ref = oracle_lw(oracle_mod, m, cols, items, cloud, one_stream)
        out = fused(pkg, k, cols, cloud, t, one_stream)
        err = max(float(np.max(np.abs(a - b))) for a, b in zip(out, ref))
        print("extreme particles %s %s: %.2e W m-2 from the oracle (bar %.0e)" %
              (which, "one-stream" if one_stream else "two-stream", err, BAR))
        assert all(np.all(np.isfinite(a)) for a in out) and err < BAR
        clean = out
        bad = {n: v.copy() for n, v in cloud.items()}
        bad["tau"][k.get_nband() - 1, 41, 17] = np.nan
        hit = [17]
        if not one_stream:
            bad["ssa"][0, 35, 90] = np.nan
            hit.append(90)
        got = fused(pkg, k, cols, bad, t, one_stream)
        keep = np.ones(ncol, bool); keep[hit] = False
        for a, b in zip(got, clean):
            assert np.array_equal(a[:, keep], b[:, keep])
        for c in hit:   # the upward flux passes the layer on its way from the surface: every level
            assert np.all(np.isnan(got[0][:, c])) and np.any(np.isnan(got[1][:, c])), c


def test_caller_owned_scratch_and_capture(pkg, gpu, lw):
    """lw_fluxes_allsky at 60 layers on a caller-owned block of exactly the size include/ecckd_hip.h documents --
    (ncol*nlay*ngpt + 32)*8 bytes, what ecckd_lw_fluxes asks its stream's block for on this route: the band planes are
    read in place -- filled with 0xFF bytes gives the eager bits; one byte less is refused ("too small") and launches
    nothing; a capture on one stream after a warm-up call (a single chain of kernels) replays to the eager bits, twice."""
    import torch
    t = T(gpu)
    for which, ncol in (("fsck", 1000), ("rrtmgp", 1777)):
        k = lw[which][0]
        nlay, ng = 60, k.get_ngpt()
        cols, cloud = case(k, 3, ncol, nlay)
        for one_stream in (False, True):
            ref = fused(pkg, k, cols, cloud, t, one_stream, 3, True)
            need = (ncol * nlay * ng + 32) * 8
            stream = torch.cuda.Stream()
            for size in (need, need - 1):
                buf = torch.full((size,), 0xFF, dtype=torch.uint8, device=gpu)   # (NaN patterns: stale data would show)
                torch.cuda.synchronize()
                pkg.set_stream_scratch(buf, stream=stream)
                try:
                    with torch.cuda.stream(stream):
                        if size == need:
                            out = fused(pkg, k, cols, cloud, t, one_stream, 3, True)
                            assert np.array_equal(out[0], ref[0]) and np.array_equal(out[1], ref[1])
                        else:
                            gc = helpers.product_gas_concs(pkg, cols, t)
                            fl = pkg.FluxesBroadband(*(t(np.full((nlay + 1, ncol), -5.0)) for _ in range(2)))
                            msg = k.lw_fluxes_allsky(t(cols["plev"]), t(cols["tlay"]), t(cols["tsfc"]), t(cols["tlev"]), gc, True,
                                                     t(cols["emis"]), particles(pkg, cloud, t, one_stream), fl)
                            assert "too small" in msg
                            torch.cuda.synchronize()
                            assert np.all(back(fl.flux_up) == -5.0) and np.all(back(fl.flux_dn) == -5.0)
                    torch.cuda.synchronize()
                finally:
                    pkg.set_stream_scratch(None, stream=stream)
            del buf
        # capture
        ref = fused(pkg, k, cols, cloud, t, False, 1, False)
        gc = helpers.product_gas_concs(pkg, cols, t)
        part = particles(pkg, cloud, t, False)
        args = (t(cols["plev"]), t(cols["tlay"]), t(cols["tsfc"]), t(cols["tlev"]), gc, True, t(cols["emis"]), part)
        fl = pkg.FluxesBroadband(*(t(np.zeros((nlay + 1, ncol))) for _ in range(2)))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            assert k.lw_fluxes_allsky(*args, fl) == ""   # warm-up: the stream's block exists now
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            assert k.lw_fluxes_allsky(*args, fl) == ""
        for _ in range(2):
            for a in (fl.flux_up, fl.flux_dn):
                a.zero_()
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(back(fl.flux_up), ref[0]) and np.array_equal(back(fl.flux_dn), ref[1])
        del graph
        pkg.release_scratch(0)


# ------------------------------------------------------------------------------------------------
# Fortran: ecckd_driver with a particle file
# ------------------------------------------------------------------------------------------------
def write_input(path, cols, names, shortwave):
    nlay, ncol = cols["tlay"].shape
    with open(path, "wb") as f:
        f.write(struct.pack("<iii", ncol, nlay, len(names)))
        for n in names:
            f.write(n.encode().ljust(32, b" "))
        f64 = lambda a: f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())
        f64(cols["plev"]); f64(cols["tlev"]); f64(cols["tlay"]); f64(cols["tsfc"])
        if shortwave:
            f64(cols["mu0"]); f64(cols["albedo"])
        else:
            f64(cols["sfc_emis"])
        for n in names:
            f64(full_field(cols, n))


def full_field(cols, n):
    nlay, ncol = cols["tlay"].shape
    v = cols[n]
    return np.ascontiguousarray(np.broadcast_to(np.float64(v) if np.isscalar(v) else np.asarray(v, dtype=np.float64), (nlay, ncol)))


def write_particles(path, cloud, with_ssa_g, delta):
    with open(path, "wb") as f:
        f.write(struct.pack("<iii", cloud["tau"].shape[0], int(with_ssa_g), int(delta)))
        for n in ("tau", "ssa", "g") if with_ssa_g else ("tau",):
            f.write(np.ascontiguousarray(cloud[n], dtype="<f8").tobytes())


def read_output(path, ncol, nlay):
    a = np.fromfile(path, dtype="<f8")
    assert a.size == 2 * ncol * (nlay + 1)
    return a[:ncol * (nlay + 1)].reshape(nlay + 1, ncol), a[ncol * (nlay + 1):].reshape(nlay + 1, ncol)


def block_gas_concs(pkg, cols, names, c0, c1):
    """The block's gases as the driver hands them over: a field that is uniform over the block is a scalar."""
    gc = pkg.GasConcs(list(names))
    for n in names:
        v = full_field(cols, n)[:, c0:c1]
        if np.all(v == v[0, 0]):
            assert gc.set_vmr(n, float(v[0, 0])) == ""
        else:
            assert gc.set_vmr(n, np.ascontiguousarray(v)) == ""
    return gc


def driver(pkg):
    drv = pkg.FORTRAN_DRIVER if os.path.exists(pkg.FORTRAN_DRIVER) else pkg.build_fortran()
    if drv is None:
        pytest.skip("no Fortran driver binary and no amdflang")
    return drv


@pytest.mark.parametrize("mode,with_ssa_g,delta", [("lw", True, False), ("lw", False, False), ("sw", True, True), ("sw", True, False)])
def test_fortran_driver_all_sky(pkg, gpu, oracle_mod, lw, tmp_path, mode, with_ssa_g, delta):
    """ecckd_driver lw|sw ... fused=1 particles.bin (type-bound lw_fluxes_allsky / sw_fluxes_allsky), 250 columns in blocks
    of 100 (a ragged last block): bit for bit the Python call on host arrays with the same blocks, and within 1e-8 W m-2
    of the all-sky oracle (a sanity bound: the equality with the Python call is the check).  The driver's shortwave input
    has one albedo per column: the (ncol, nband) albedo arrays repeat it.  With fused=0 and a particle file the driver
    exits non-zero with the usage text."""
    from conftest import SW_WIDE
    drv = driver(pkg)
    sw = mode == "sw"
    ncol, nlay, block = 250, 60, 100
    if sw:
        path = SW_WIDE
        k = pkg.GasOpticsEcckd()
        assert k.load(path, device=0) == ""
        m = oracle_mod.CkdModel(path)
    else:
        k, m, path = lw["rrtmgp"]
    nb = k.get_nband()
    cols = synthetic.columns(40, ncol, k.get_press_min(), nlay=nlay, shortwave=sw)
    cloud = synthetic.clouds(40, ncol, nlay, nb)
    names = synthetic.GAS_ORDER
    write_input(tmp_path / "in.bin", cols, names, sw)
    write_particles(tmp_path / "part.bin", cloud, with_ssa_g, delta)
    base = [drv, mode, path, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(block), "1", "0", "1", "0"]
    r = subprocess.run(base + ["0", str(tmp_path / "part.bin")], capture_output=True, text=True)
    assert r.returncode != 0 and "usage: ecckd_driver" in r.stderr
    r = subprocess.run(base + ["1", str(tmp_path / "part.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    fu, fd = read_output(tmp_path / "out.bin", ncol, nlay)
    # the Python call on host arrays, block by block
    pu, pd = np.empty_like(fu), np.empty_like(fd)
    for c0 in range(0, ncol, block):
        c1 = min(ncol, c0 + block)
        nc = c1 - c0
        cut = lambda a: np.ascontiguousarray(a[..., c0:c1])
        gc = block_gas_concs(pkg, cols, names, c0, c1)
        part = particles(pkg, {n: cut(cloud[n]) for n in ("tau", "ssa", "g")}, np.ascontiguousarray, not with_ssa_g)
        fl = pkg.FluxesBroadband(np.empty((nlay + 1, nc)), np.empty((nlay + 1, nc)))
        if sw:
            alb = np.repeat(cut(cols["albedo"])[:, None], nb, 1)
            assert k.sw_fluxes_allsky(cut(cols["plev"]), cut(cols["tlay"]), gc, True, cut(cols["mu0"]), alb, alb.copy(), part, fl,
                                      delta_scale=delta) == ""
        else:
            emis = np.repeat(cut(cols["sfc_emis"])[:, None], nb, 1)
            assert k.lw_fluxes_allsky(cut(cols["plev"]), cut(cols["tlay"]), cut(cols["tsfc"]), cut(cols["tlev"]), gc, True, emis,
                                      part, fl) == ""
        pu[:, c0:c1], pd[:, c0:c1] = fl.flux_up, fl.flux_dn
    assert np.array_equal(fu, pu) and np.array_equal(fd, pd)
    if sw:
        cols["alb_dir"] = cols["alb_dif"] = np.repeat(cols["albedo"][:, None], nb, 1)
        ref = ah.oracle_sw_allsky(oracle_mod, m, cols, helpers.oracle_gas_items(cols, names), cloud, delta=delta)[:2]
    else:
        ref = oracle_lw(oracle_mod, m, cols, helpers.oracle_gas_items(cols, names), cloud, not with_ssa_g)
    err = max(float(np.max(np.abs(a - b))) for a, b in zip((fu, fd), ref))
    print("fortran all-sky %s ssa/g %d delta %d: %.2e W m-2 from the oracle (bound 1e-8)" % (mode, with_ssa_g, delta, err))
    assert err < 1e-8
