"""ecckd_lw_fluxes_clear_allsky / ecckd_sw_fluxes_clear_allsky on the GPU: clear-sky and all-sky fluxes from one gas-optics
pass.

Every numerical check is an equality with a call the library already has, so there is no tolerance anywhere: the
clear-sky outputs are those of lw_fluxes / sw_fluxes and the all-sky outputs those of lw_fluxes_allsky / sw_fluxes_allsky
(with cloud_mask where one is given), bit for bit -- at 60 layers (the fused layer-split kernels, as two launches and as the
dual-sky kernel: "lw_both_skies" 0 and 1), at 37 and 137 layers (the general route), in both orientations, for either
"sw_solver".  The outputs are prefilled with distinct sentinels, every value must be finite (but for the bottom-up
shortwave columns, whose NaNs the existing calls produce as well and which are compared as they are), and the particle
arrays and the mask must come back untouched.  Then: a second call on the same stream with other particles (an increment left in
the scratch optical depth, or a clear pass run after it, would show in the clear-sky output), host arrays against device
arrays, a caller-owned scratch block of exactly the all-sky call's documented size with eager call, capture and replay,
and the Fortran driver's second output file."""
import subprocess

import numpy as np
import pytest

import helpers
import mcica_helpers as mh
import test_gpu_allsky as swt
import test_gpu_lw_allsky as lwt
from rte_ecckd_amd import synthetic

pytestmark = pytest.mark.gpu
T, back = lwt.T, lwt.back
SENTINELS = (-1.0, -2.0, -3.0, -4.0, -5.0, -6.0)
# A masked cloud layer must show in the fluxes where its optical depth is above this floor: the absorbing share of a
# two-stream layer is at least 0.2 / nband of it (synthetic.clouds: ssa <= 1 - 0.2 / nband), so above 1e-3 for the shipped
# band counts; against a gas optical depth of 1e3 in the same cell that still moves the source weights by parts in 1e9,
# seven orders above the last bit of a broadband flux.
SEEN_FLOOR = 0.1


@pytest.fixture(autouse=True)
def default_options(pkg):
    def reset():
        pkg.reset_solver_options()
        pkg.set_solver_option("sw_solver", 0)
        pkg.set_solver_option("sw_tail_split", 1)
        pkg.set_solver_option("lw_both_skies", 0)
        pkg.set_arithmetic(pkg.FAST)
    reset()
    yield
    reset()


@pytest.fixture(scope="module")
def lw(pkg, gpu):
    from conftest import LW_FSCK, LW_RRTMGP
    out = {}
    for name, path in (("fsck", LW_FSCK), ("rrtmgp", LW_RRTMGP)):
        k = pkg.GasOpticsEcckd()
        assert k.load(path, device=0) == ""
        out[name] = (k, path)
    return out


@pytest.fixture(scope="module")
def sw(pkg, gpu):
    from conftest import SW_WIDE
    k = pkg.GasOpticsEcckd()
    assert k.load(SW_WIDE, device=0) == ""
    return k, SW_WIDE


def to_mask(mask, to):
    if mask is None:
        return None
    return mask if to is np.ascontiguousarray else to(mask.view(np.int64))


def untouched(part, cloud, mask, dmask, one_stream=False):
    names = ("tau",) if one_stream else (("tau", "ssa", "g") if getattr(part, "g", None) is not None else ("tau", "ssa"))
    for n in names:
        assert np.array_equal(back(getattr(part, n)), cloud[n]), n
    if mask is not None:
        assert np.array_equal(back(dmask).view(np.uint64), mask)


# ------------------------------------------------------------------------------------------------
# longwave
# ------------------------------------------------------------------------------------------------
def lw_args(pkg, k, cols, to, top_at_1):
    gc = helpers.product_gas_concs(pkg, cols, to)
    return (to(cols["plev"]), to(cols["tlay"]), to(cols["tsfc"]), to(cols["tlev"]), gc, top_at_1, to(cols["emis"]))


def lw_both(pkg, k, cols, cloud, to, mask=None, one_stream=False, nmus=1, inc=False, top_at_1=True):
    """[up, dn, up_clear, dn_clear] of lw_fluxes_clear_allsky."""
    nlay, ncol = cols["tlay"].shape
    part = lwt.particles(pkg, cloud, to, one_stream)
    dmask = to_mask(mask, to)
    fl = pkg.FluxesBroadband(*(to(np.full((nlay + 1, ncol), s)) for s in SENTINELS[:2]))
    fc = pkg.FluxesBroadband(*(to(np.full((nlay + 1, ncol), s)) for s in SENTINELS[2:4]))
    assert k.lw_fluxes_clear_allsky(*lw_args(pkg, k, cols, to, top_at_1), part, fl, fc, n_gauss_angles=nmus,
                                    inc_flux=to(cols["inc_flux"]) if inc else None, cloud_mask=dmask) == ""
    untouched(part, cloud, mask, dmask, one_stream)
    out = [back(fl.flux_up), back(fl.flux_dn), back(fc.flux_up), back(fc.flux_dn)]
    assert all(np.all(np.isfinite(a)) for a in out)
    return out


def lw_separate(pkg, k, cols, cloud, to, mask=None, one_stream=False, nmus=1, inc=False, top_at_1=True):
    """[up, dn, up_clear, dn_clear] of lw_fluxes_allsky(cloud_mask=) and lw_fluxes."""
    nlay, ncol = cols["tlay"].shape
    part = lwt.particles(pkg, cloud, to, one_stream)
    fl = pkg.FluxesBroadband(*(to(np.full((nlay + 1, ncol), s)) for s in SENTINELS[:2]))
    fc = pkg.FluxesBroadband(*(to(np.full((nlay + 1, ncol), s)) for s in SENTINELS[2:4]))
    incf = to(cols["inc_flux"]) if inc else None
    assert k.lw_fluxes(*lw_args(pkg, k, cols, to, top_at_1), fc, n_gauss_angles=nmus, inc_flux=incf) == ""
    assert k.lw_fluxes_allsky(*lw_args(pkg, k, cols, to, top_at_1), part, fl, n_gauss_angles=nmus, inc_flux=incf,
                              cloud_mask=to_mask(mask, to)) == ""
    return [back(fl.flux_up), back(fl.flux_dn), back(fc.flux_up), back(fc.flux_dn)]


def forms(nlay):
    return (0, 1) if nlay == 60 else (0,)


@pytest.mark.parametrize("ncol", [1, 130, 333])
@pytest.mark.parametrize("nlay", [60, 37, 137])
@pytest.mark.parametrize("which", ["fsck", "rrtmgp"])
def test_longwave_equals_the_two_calls(pkg, gpu, lw, which, nlay, ncol):
    """1 column, a ragged 32-column tile (130) and an odd tile count (333: one group of a two-group block lies beyond the
    end); one- and two-stream particles; with and without a mask from sample_cloud_mask; 1 and 3 angles, with and without
    inc_flux; bottom-up as well at 60 and 137 layers; "lw_both_skies" 0 and 1 at 60 layers.  Cloudy columns differ between
    the two skies (with a mask: every column where a g-point sees a cloud layer), cloud-free columns agree bit for bit."""
    k = lw[which][0]
    t = T(gpu)
    c0 = 5 * ncol + nlay
    cols, cloud = lwt.case(k, c0, ncol, nlay)
    sampled = pkg.sample_cloud_mask(t(synthetic.cloud_fraction(c0, ncol, nlay)), k.get_ngpt(), seed=77, col0=c0)
    sampled = back(sampled).view(np.uint64)
    cloudy = cloud["cloudy"]
    # With a mask, the columns that have to differ are those where some g-point sees a layer of particle optical depth above
    # SEEN_FLOOR (a layer none of the g-points sees adds nothing, and a thinner one need not move the last bit).
    seen = ((sampled != 0) & (cloud["tau"].min(axis=0) > SEEN_FLOOR)).any(axis=0)
    assert not (seen & ~cloudy).any()
    if ncol > 1:
        assert cloudy.any() and (~cloudy).any() and seen.any()
    for top_at_1 in ((True, False) if nlay in (60, 137) else (True,)):
        for one_stream in (False, True):
            for mask in (None, sampled):
                for nmus in (1, 3):
                    for inc in (False, True):
                        ref = lw_separate(pkg, k, cols, cloud, t, mask, one_stream, nmus, inc, top_at_1)
                        for form in forms(nlay):
                            pkg.set_solver_option("lw_both_skies", form)
                            out = lw_both(pkg, k, cols, cloud, t, mask, one_stream, nmus, inc, top_at_1)
                            what = (which, nlay, ncol, top_at_1, one_stream, mask is not None, nmus, inc, form)
                            for a, b in zip(out, ref):
                                assert np.array_equal(a, b), what
                            for a, c in zip(out[:2], out[2:]):
                                assert np.array_equal(a[:, ~cloudy], c[:, ~cloudy]), what
                            differ = cloudy if mask is None else seen
                            assert np.all(np.abs(out[0] - out[2]).max(axis=0)[differ] > 0), what
                        pkg.set_solver_option("lw_both_skies", 0)


@pytest.mark.parametrize("nlay,form", [(60, 0), (60, 1), (37, 0)])
def test_longwave_repeated_call(pkg, gpu, lw, nlay, form):
    """Two calls on one stream with different particles: the second call's clear-sky output is the first's (and
    lw_fluxes'), its all-sky output is its own particles'."""
    k = lw["fsck"][0]
    t = T(gpu)
    ncol = 333
    cols, cloud = lwt.case(k, 19, ncol, nlay)
    other = synthetic.clouds(4000, ncol, nlay, k.get_nband())
    assert not np.array_equal(other["tau"], cloud["tau"])
    ref = lw_separate(pkg, k, cols, other, t)
    pkg.set_solver_option("lw_both_skies", form)
    first = lw_both(pkg, k, cols, cloud, t)
    second = lw_both(pkg, k, cols, other, t)
    assert np.array_equal(second[2], first[2]) and np.array_equal(second[3], first[3])
    for a, b in zip(second, ref):
        assert np.array_equal(a, b)
    assert not np.array_equal(second[0], first[0])


# ------------------------------------------------------------------------------------------------
# shortwave
# ------------------------------------------------------------------------------------------------
def sw_outputs(to, nlay, ncol, sentinels, with_dir):
    import rte_ecckd_amd as pkg
    return pkg.FluxesBroadband(*(to(np.full((nlay + 1, ncol), s)) for s in (sentinels if with_dir else sentinels[:2])))


def sw_args(pkg, cols, to, top_at_1):
    gc = helpers.product_gas_concs(pkg, cols, to, swt.SW_NAMES)
    return (to(cols["plev"]), to(cols["tlay"]), gc, top_at_1, to(cols["mu0"]), to(cols["alb_dir"]), to(cols["alb_dif"]))


def fluxes_of(fl):
    return [back(fl.flux_up), back(fl.flux_dn)] + ([back(fl.flux_dn_dir)] if fl.flux_dn_dir is not None else [])


def sw_both(pkg, k, cols, cloud, to, delta, mask=None, dirs=(True, True), scale=False, top_at_1=True):
    """(all-sky [up, dn(, dir)], clear-sky [up, dn(, dir)]) of sw_fluxes_clear_allsky."""
    nlay, ncol = cols["tlay"].shape
    part = swt.make(pkg, (cloud["tau"], cloud["ssa"], cloud["g"]), to)
    dmask = to_mask(mask, to)
    fl, fc = sw_outputs(to, nlay, ncol, SENTINELS[:3], dirs[0]), sw_outputs(to, nlay, ncol, SENTINELS[3:], dirs[1])
    assert k.sw_fluxes_clear_allsky(*sw_args(pkg, cols, to, top_at_1), part, fl, fc, delta_scale=delta,
                                    toa_scale=to(cols["scale"]) if scale else None, cloud_mask=dmask) == ""
    untouched(part, cloud, mask, dmask)
    out = fluxes_of(fl), fluxes_of(fc)
    if top_at_1:   # (bottom-up columns hand the gas optics negative layer masses: NaNs, the same in every call)
        assert all(np.all(np.isfinite(a)) for a in out[0] + out[1])
    assert not any(np.any(a == s) for side, ss in zip(out, (SENTINELS[:3], SENTINELS[3:])) for a, s in zip(side, ss))
    return out


def sw_separate(pkg, k, cols, cloud, to, delta, mask=None, scale=False, top_at_1=True):
    nlay, ncol = cols["tlay"].shape
    part = swt.make(pkg, (cloud["tau"], cloud["ssa"], cloud["g"]), to)
    fl, fc = sw_outputs(to, nlay, ncol, SENTINELS[:3], True), sw_outputs(to, nlay, ncol, SENTINELS[3:], True)
    sc = to(cols["scale"]) if scale else None
    assert k.sw_fluxes(*sw_args(pkg, cols, to, top_at_1), fc, toa_scale=sc) == ""
    assert k.sw_fluxes_allsky(*sw_args(pkg, cols, to, top_at_1), part, fl, delta_scale=delta, toa_scale=sc,
                              cloud_mask=to_mask(mask, to)) == ""
    return fluxes_of(fl), fluxes_of(fc)


@pytest.mark.parametrize("ncol", [1, 130, 333])
@pytest.mark.parametrize("nlay,solver", [(60, 0), (37, 0), (137, 0), (60, 1)])
def test_shortwave_equals_the_two_calls(pkg, gpu, sw, nlay, solver, ncol):
    """Layer-systolic solver at 60 and 37 layers, two-pass solver at 137 layers and ("sw_solver" = 1) at 60; delta_scale 0
    and 1; with and without a mask; with toa_scale; flux_dir / flux_dir_clear present or absent independently; bottom-up at
    60 layers (the gas optics takes plev(:,l+1) - plev(:,l) as the layer mass, so reversed columns give it negative masses and
    the existing calls NaNs: there the NaN patterns have to agree as well, as in test_gpu_allsky.py)."""
    k = sw[0]
    t = T(gpu)
    c0 = 3 * ncol + nlay
    pkg.set_solver_option("sw_solver", solver)
    for top_at_1 in ((True, False) if nlay == 60 and solver == 0 else (True,)):
        cols, cloud = swt.sw_case(k, c0, ncol, nlay, 17, top_at_1=top_at_1)
        cf = synthetic.cloud_fraction(c0, ncol, nlay)
        sampled = mh.sample(cf if top_at_1 else np.ascontiguousarray(cf[::-1]), k.get_ngpt(), mh.MAX_RAN, None, 5, c0)
        cloudy = cloud["cloudy"]
        for delta in (False, True):
            for mask in (None, sampled):
                for scale in (False, True):
                    ref = sw_separate(pkg, k, cols, cloud, t, delta, mask, scale, top_at_1)
                    for dirs in ((True, True), (False, True), (True, False), (False, False)) if not scale else ((True, True),):
                        out = sw_both(pkg, k, cols, cloud, t, delta, mask, dirs, scale, top_at_1)
                        what = (nlay, solver, ncol, top_at_1, delta, mask is not None, scale, dirs)
                        for side in (0, 1):
                            assert len(out[side]) == (3 if dirs[side] else 2)
                            for a, b in zip(out[side], ref[side]):
                                assert np.array_equal(a, b, equal_nan=not top_at_1), what
                        lit = cols["mu0"] > 0
                        if mask is None and top_at_1 and (cloudy & lit).any():
                            assert np.all(np.abs(out[0][1] - out[1][1]).max(axis=0)[cloudy & lit] > 0), what


def test_shortwave_repeated_call(pkg, gpu, sw):
    k = sw[0]
    t = T(gpu)
    ncol, nlay = 333, 60
    cols, cloud = swt.sw_case(k, 19, ncol, nlay, 3)
    other = synthetic.clouds(4000, ncol, nlay, k.get_nband())
    ref = sw_separate(pkg, k, cols, other, t, True)
    first = sw_both(pkg, k, cols, cloud, t, True)
    second = sw_both(pkg, k, cols, other, t, True)
    for a, b in zip(second[1], first[1]):
        assert np.array_equal(a, b)
    for side in (0, 1):
        for a, b in zip(second[side], ref[side]):
            assert np.array_equal(a, b)
    assert not np.array_equal(second[0][0], first[0][0])


# ------------------------------------------------------------------------------------------------
# host arrays
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlay", [60, 37])
def test_host_arrays_equal_device_arrays(pkg, gpu, lw, sw, nlay):
    t = T(gpu)
    ncol = 130
    for which in ("fsck", "rrtmgp"):
        k = lw[which][0]
        cols, cloud = lwt.case(k, 11, ncol, nlay)
        mask = mh.sample(synthetic.cloud_fraction(11, ncol, nlay), k.get_ngpt(), mh.MAX_RAN, None, 8, 11)
        for form in forms(nlay):
            pkg.set_solver_option("lw_both_skies", form)
            for one_stream, m, nmus, inc in ((False, None, 1, False), (True, mask, 3, True), (False, mask, 1, True)):
                d = lw_both(pkg, k, cols, cloud, t, m, one_stream, nmus, inc)
                h = lw_both(pkg, k, cols, cloud, np.ascontiguousarray, m, one_stream, nmus, inc)
                for a, b in zip(d, h):
                    assert np.array_equal(a, b), (which, form, one_stream, m is not None)
        pkg.set_solver_option("lw_both_skies", 0)
    k = sw[0]
    cols, cloud = swt.sw_case(k, 11, ncol, nlay, 5)
    mask = mh.sample(synthetic.cloud_fraction(11, ncol, nlay), k.get_ngpt(), mh.MAX_RAN, None, 8, 11)
    for delta, m, dirs, scale in ((True, None, (True, True), False), (False, mask, (False, True), True), (True, mask, (True, False), True)):
        d = sw_both(pkg, k, cols, cloud, t, delta, m, dirs, scale)
        h = sw_both(pkg, k, cols, cloud, np.ascontiguousarray, delta, m, dirs, scale)
        for side in (0, 1):
            assert len(d[side]) == len(h[side])
            for a, b in zip(d[side], h[side]):
                assert np.array_equal(a, b), (delta, m is not None, dirs)


# ------------------------------------------------------------------------------------------------
# caller-owned scratch and capture
# ------------------------------------------------------------------------------------------------
def on_block_then_captured(pkg, gpu, need, call, outputs, ref):
    """`call()` on a caller-owned block of `need` bytes filled with 0xFF: the eager call, a capture on that stream and two
    replays all give `ref`; one byte less is refused with the outputs untouched."""
    import torch
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())

    def read():
        torch.cuda.synchronize()
        return [back(a).copy() for a in outputs]

    def wipe():
        for a in outputs:
            a.fill_(-9.0)
        torch.cuda.synchronize()

    for size in (need - 1, need):
        buf = torch.full((size,), 0xFF, dtype=torch.uint8, device=gpu)
        torch.cuda.synchronize()
        pkg.set_stream_scratch(buf, stream=stream)
        try:
            wipe()
            with torch.cuda.stream(stream):
                msg = call()
            got = read()
            if size < need:
                assert "too small" in msg and all(np.all(a == -9.0) for a in got)
                continue
            assert msg == ""
            assert all(np.array_equal(a, b) for a, b in zip(got, ref)), "eager call on the caller-owned block"
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                assert call() == ""
            for _ in range(2):
                wipe()
                graph.replay()
                got = read()
                assert all(np.array_equal(a, b) for a, b in zip(got, ref)), "graph replay"
            del graph
        finally:
            torch.cuda.synchronize()
            pkg.set_stream_scratch(None, stream=stream)
        del buf


@pytest.mark.parametrize("nlay,form", [(60, 0), (60, 1), (37, 0)])
def test_longwave_caller_owned_scratch_and_capture(pkg, gpu, lw, nlay, form):
    """The block ecckd_lw_fluxes_allsky takes for the shape (include/ecckd_hip.h) serves the call: at 60 layers the gas
    optical depth alone, (ncol*nlay*ngpt + 32)*8 bytes; on the general route (37 layers) the optical depth, the three Planck
    source arrays, the surface source and the solver's ring, which the clear pass and the all-sky pass share."""
    t = T(gpu)
    k = lw["rrtmgp"][0]
    ncol, ng = 1000, k.get_ngpt()
    n3 = ncol * nlay * ng
    need = (n3 + 32) * 8 if nlay == 60 else (4 * n3 + ncol * ng + 64) * 8 + pkg.rte_lw_scratch_bytes(ncol, nlay, ng)
    cols, cloud = lwt.case(k, 3, ncol, nlay)
    mask = mh.sample(synthetic.cloud_fraction(3, ncol, nlay), ng, mh.MAX_RAN, None, 8, 3)
    for m in (None, mask):
        ref = lw_separate(pkg, k, cols, cloud, t, m, False, 3, True)
        pkg.set_solver_option("lw_both_skies", form)
        part = lwt.particles(pkg, cloud, t, False)
        args = lw_args(pkg, k, cols, t, True)
        incf, dmask = t(cols["inc_flux"]), to_mask(m, t)
        outs = [t(np.zeros((nlay + 1, ncol))) for _ in range(4)]
        fl, fc = pkg.FluxesBroadband(outs[0], outs[1]), pkg.FluxesBroadband(outs[2], outs[3])
        call = lambda: k.lw_fluxes_clear_allsky(*args, part, fl, fc, n_gauss_angles=3, inc_flux=incf, cloud_mask=dmask)
        on_block_then_captured(pkg, gpu, need, call, outs, ref)
        pkg.set_solver_option("lw_both_skies", 0)
    pkg.release_scratch(0)


@pytest.mark.parametrize("nlay", [60, 91])
def test_shortwave_caller_owned_scratch_and_capture(pkg, gpu, sw, nlay):
    """The block ecckd_sw_fluxes_allsky documents for the shape (include/ecckd_hip.h: optical depth, the solver's room --
    layer-systolic at 60 layers, two-pass at 91 -- and the three delta-scaled band planes) serves the call: both solver
    passes share the solver room."""
    t = T(gpu)
    k = sw[0]
    ng, nb, ncol = k.get_ngpt(), k.get_nband(), 1000
    cols, cloud = swt.sw_case(k, 3, ncol, nlay, 17)
    align = lambda n: (n + 255) // 256 * 256
    tail = pkg.rte_sw_tail_scratch_bytes(ncol, nlay, ng)
    solver = tail if nlay <= 60 else max(pkg.rte_sw_scratch_bytes(ncol, nlay, ng), tail)
    need = align(ncol * nlay * ng * 8) + solver + 3 * align(ncol * nlay * nb * 8)
    args = sw_args(pkg, cols, t, True)
    part = swt.make(pkg, (cloud["tau"], cloud["ssa"], cloud["g"]), t)
    outs = [t(np.zeros((nlay + 1, ncol))) for _ in range(6)]
    fl, fc = pkg.FluxesBroadband(*outs[:3]), pkg.FluxesBroadband(*outs[3:])
    ref = sw_separate(pkg, k, cols, cloud, t, True)
    call = lambda: k.sw_fluxes_clear_allsky(*args, part, fl, fc, delta_scale=True)
    on_block_then_captured(pkg, gpu, need, call, outs, ref[0] + ref[1])
    pkg.release_scratch(0)


# ------------------------------------------------------------------------------------------------
# Fortran: ecckd_driver with a second output file
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["lw", "sw"])
def test_fortran_driver_clear_sky_file(pkg, gpu, lw, sw, tmp_path, mode):
    """ecckd_driver ... fused=1 particles.bin "" clear.bin (the 13th argument), 250 columns in blocks of 100: output.bin and
    clear.bin equal the Python call on host arrays with the same blocks bit for bit."""
    drv = lwt.driver(pkg)
    shortwave = mode == "sw"
    ncol, nlay, block = 250, 60, 100
    k, path = sw if shortwave else lw["rrtmgp"]
    nb = k.get_nband()
    cols = synthetic.columns(40, ncol, k.get_press_min(), nlay=nlay, shortwave=shortwave)
    cloud = synthetic.clouds(40, ncol, nlay, nb)
    names = synthetic.GAS_ORDER
    lwt.write_input(tmp_path / "in.bin", cols, names, shortwave)
    lwt.write_particles(tmp_path / "part.bin", cloud, True, True)
    base = [drv, mode, path, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(block), "1", "0", "1", "0"]
    r = subprocess.run(base + ["1", str(tmp_path / "part.bin"), "", str(tmp_path / "clear.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    fu, fd = lwt.read_output(tmp_path / "out.bin", ncol, nlay)
    cu, cd = lwt.read_output(tmp_path / "clear.bin", ncol, nlay)
    want = [np.empty_like(fu) for _ in range(4)]
    for c0 in range(0, ncol, block):
        c1 = min(ncol, c0 + block)
        nc = c1 - c0
        cut = lambda a: np.ascontiguousarray(a[..., c0:c1])
        gc = lwt.block_gas_concs(pkg, cols, names, c0, c1)
        part = lwt.particles(pkg, {n: cut(cloud[n]) for n in ("tau", "ssa", "g")}, np.ascontiguousarray, False)
        fl = pkg.FluxesBroadband(np.empty((nlay + 1, nc)), np.empty((nlay + 1, nc)))
        fc = pkg.FluxesBroadband(np.empty((nlay + 1, nc)), np.empty((nlay + 1, nc)))
        if shortwave:
            alb = np.repeat(cut(cols["albedo"])[:, None], nb, 1)
            assert k.sw_fluxes_clear_allsky(cut(cols["plev"]), cut(cols["tlay"]), gc, True, cut(cols["mu0"]), alb, alb.copy(),
                                            part, fl, fc, delta_scale=True) == ""
        else:
            emis = np.repeat(cut(cols["sfc_emis"])[:, None], nb, 1)
            assert k.lw_fluxes_clear_allsky(cut(cols["plev"]), cut(cols["tlay"]), cut(cols["tsfc"]), cut(cols["tlev"]), gc, True,
                                            emis, part, fl, fc) == ""
        for w, a in zip(want, (fl.flux_up, fl.flux_dn, fc.flux_up, fc.flux_dn)):
            w[:, c0:c1] = a
    for got, w in zip((fu, fd, cu, cd), want):
        assert np.array_equal(got, w)
    assert not np.array_equal(fu, cu)
    # the second output file needs the fused path and a particle file
    r = subprocess.run(base + ["1", "", "", str(tmp_path / "clear.bin")], capture_output=True, text=True)
    assert r.returncode != 0 and "usage: ecckd_driver" in r.stderr
