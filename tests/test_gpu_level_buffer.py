"""The longwave level sources as one buffer (include/ecckd_hip.h, "Level buffer"): lev_source_inc == lev_source_dec + ncol
names the two views of one (ngpt, nlay+1, ncol) array, gas optics stores each level once and rte_lw reads it once.  Only
addresses change, never arithmetic, so every comparison here is bit for bit.

Shapes: 1 column, 63 / 65 (a ragged and a just-over wave), 1541 (more than one tile of 512, odd: paired 16-byte stores on
8-byte-aligned planes); 1 layer (first and last at once), 2 and 3 (the second store of a level comes and goes), 60 and 61
(the shipped shape and one beyond it); solver layer counts on both sides of every unrolled variant (32 | 33, 96 | 97), the
60-layer exact form and the scratch-ring form (137); 5 and 6 g-points (odd: the upper half-wave clamps to the last one)."""
import ctypes as C

import numpy as np
import pytest

import helpers
from conftest import LW_FSCK, LW_RRTMGP
from rte_ecckd_amd import synthetic

pytestmark = pytest.mark.gpu
OPTIONS = ("gas_input_ahead", "gas_slab_f32", "gas_tile_sync", "lw_solver", "lw_tail_split")
SENTINEL = -7.25


@pytest.fixture(autouse=True)
def options_back(pkg):
    saved = {n: pkg.get_solver_option(n) for n in OPTIONS}
    pkg.set_arithmetic(pkg.FAST)
    yield
    pkg.set_arithmetic(pkg.FAST)
    for n, v in saved.items():
        pkg.set_solver_option(n, v)


@pytest.fixture(scope="module")
def models(pkg, gpu):
    out = {}
    for name, path in (("fsck", LW_FSCK), ("rrtmgp", LW_RRTMGP)):
        k = pkg.GasOpticsEcckd()
        assert k.load(path, device=0) == ""
        out[name] = k
    return out


_columns = {}


def columns(k, c0, ncol, nlay):
    """synthetic.columns, computed once per shape and never written to."""
    key = (c0, ncol, nlay, k.get_press_min())
    if key not in _columns:
        _columns[key] = synthetic.columns(c0, ncol, k.get_press_min(), nlay=nlay)
    return _columns[key]


def same_bits(a, b):
    """Two float64 device tensors, bit for bit (NaN payloads and signed zeros included)."""
    import torch
    a, b = a.contiguous(), b.contiguous()
    return a.dtype == b.dtype == torch.float64 and a.shape == b.shape and bool((a.view(torch.int64) == b.view(torch.int64)).all())


class GasCall:
    """ecckd_gas_optics_lw called through the C ABI on device tensors; the level sources either as two separate arrays or as
    the two views of one buffer that stands between guard planes of a sentinel."""

    def __init__(self, pkg, k, cols, gpu):
        import torch
        self.pkg, self.k, self.torch = pkg, k, torch
        self.nlay, self.ncol = cols["tlay"].shape
        self.ng = k.get_ngpt()
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(gpu)
        self.gc = helpers.product_gas_concs(pkg, cols, to)
        self.plev, self.tlay, self.tsfc, self.tlev = (to(cols[n]) for n in ("plev", "tlay", "tsfc", "tlev"))
        self.gas = k._gas_args(self.gc, self.ncol, self.nlay, pkg.DEVICE)
        self.gpu = gpu

    def full(self, *shape):
        return self.torch.full(shape, SENTINEL, dtype=self.torch.float64, device=self.gpu)

    def call(self, tau, lay, inc_ptr, dec_ptr, sfc, tlev=True):
        n, names, ptrs, cs, ls, sc, _ = self.gas
        p = lambda t: C.c_void_p(t.data_ptr())
        stream = C.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        rc = self.pkg.lib().ecckd_gas_optics_lw(self.k._need(), self.ncol, self.nlay, p(self.plev), p(self.tlay), p(self.tsfc),
                                                p(self.tlev) if tlev else None, n, names, ptrs, cs, ls, sc, p(tau), p(lay),
                                                C.c_void_p(inc_ptr), C.c_void_p(dec_ptr), p(sfc), self.pkg.DEVICE, stream)
        self.torch.cuda.synchronize()
        return rc

    def separate(self):
        ng, nlay, ncol = self.ng, self.nlay, self.ncol
        tau, lay, inc, dec, sfc = self.full(ng, nlay, ncol), self.full(ng, nlay, ncol), self.full(ng, nlay, ncol), self.full(ng, nlay, ncol), self.full(ng, ncol)
        assert self.call(tau, lay, inc.data_ptr(), dec.data_ptr(), sfc) == 0, self.pkg.last_error()
        return tau, lay, inc, dec, sfc

    def buffer(self, tlev=True):
        """(tau, lay, inc view, dec view, sfc), after checking that nothing outside the region was written."""
        ng, nlay, ncol = self.ng, self.nlay, self.ncol
        guard = 2 * ncol + 1   # (odd: the region starts on an 8-byte, not a 16-byte, boundary)
        n = ng * (nlay + 1) * ncol
        raw = self.full(n + 2 * guard)
        tau, lay, sfc = self.full(ng, nlay, ncol), self.full(ng, nlay, ncol), self.full(ng, ncol)
        dec_ptr = raw.data_ptr() + 8 * guard
        rc = self.call(tau, lay, dec_ptr + 8 * ncol, dec_ptr, sfc, tlev=tlev)
        assert bool((raw[:guard] == SENTINEL).all()) and bool((raw[guard + n:] == SENTINEL).all())
        lev = raw[guard:guard + n].view(ng, nlay + 1, ncol)
        if not tlev:   # the call does its work and answers as the reference does; the level sources are not produced
            assert rc != 0 and self.pkg.last_error() == "tlev is required for ecckd"
            assert bool((lev == SENTINEL).all())
        else:
            assert rc == 0, self.pkg.last_error()
        return tau, lay, lev[:, 1:], lev[:, :-1], sfc


def buffer_equals_separate(pkg, call, fast_settings=True):
    """The buffer form against separate arrays, in the arithmetic mode that is set: all five outputs, bit for bit; in the
    fast mode the buffer form at every setting of the three gas-optics options."""
    ref = call.separate()
    settings = [(a, s, f) for a in (0, 1) for s in (0, 1) for f in (0, 1, 2)] if fast_settings else [None]
    for st in settings:
        if st is not None:
            for name, v in zip(("gas_input_ahead", "gas_tile_sync", "gas_slab_f32"), st):
                pkg.set_solver_option(name, v)
        got = call.buffer()
        for name, a, b in zip(("tau", "lay_source", "lev_source_inc", "lev_source_dec", "sfc_source"), got, ref):
            assert same_bits(a.contiguous(), b), (name, st)
    for name in ("gas_input_ahead", "gas_tile_sync", "gas_slab_f32"):
        pkg.set_solver_option(name, -1 if name != "gas_slab_f32" else 2)
    return ref


@pytest.mark.parametrize("table", ["fsck", "rrtmgp"])
@pytest.mark.parametrize("nlay", [1, 2, 3, 60, 61])
@pytest.mark.parametrize("ncol", [1, 63, 65, 1541])
def test_gas_optics_buffer_equals_separate(pkg, gpu, models, ncol, nlay, table):
    """32-g table and 36-g table (Planck window); fast arithmetic at every option setting, then reference order."""
    k = models[table]
    call = GasCall(pkg, k, columns(k, 7, ncol, nlay), gpu)
    ref = buffer_equals_separate(pkg, call)
    # what the separate arrays hold is one value per level: the buffer loses nothing
    assert same_bits(ref[2][:, :-1].contiguous(), ref[3][:, 1:].contiguous())
    pkg.set_arithmetic(pkg.REFERENCE_ORDER)
    buffer_equals_separate(pkg, call, fast_settings=False)


@pytest.mark.parametrize("arith", ["fast", "reference"])
def test_gas_optics_without_tlev_leaves_the_buffer_alone(pkg, gpu, models, arith):
    k = models["fsck"]
    pkg.set_arithmetic(pkg.FAST if arith == "fast" else pkg.REFERENCE_ORDER)
    call = GasCall(pkg, k, columns(k, 7, 65, 3), gpu)
    tau, lay, _, _, sfc = call.buffer(tlev=False)
    ref = call.separate()
    assert same_bits(tau, ref[0]) and same_bits(lay, ref[1]) and same_bits(sfc, ref[4])


def test_gas_optics_shuffled_surface_pressures(pkg, gpu, models):
    """Surface pressures of 50-103 kPa shuffled over the columns (the generator of tools/bench_gas_optics_spread.py): several
    slab positions per segment, waves split between positions, waves on the tables-from-global-memory path."""
    k = models["fsck"]
    ncol, nlay = 700, 60
    c = dict(columns(k, 0, ncol, nlay))
    eta = (np.arange(nlay + 1, dtype=np.float64) / nlay) ** 2
    ptop = c["plev"][0, 0]
    ps = 50000 + 53000 * np.random.default_rng(1).random(ncol)
    c["plev"] = np.ascontiguousarray(ptop + (ps[None, :] - ptop) * eta[:, None])
    buffer_equals_separate(pkg, GasCall(pkg, k, c, gpu))


def test_gas_optics_forced_planck_window(pkg, gpu, monkeypatch):
    """A window of 16 rows of the Planck table: most waves take the tables-from-global-memory path."""
    monkeypatch.setenv("ECCKD_PLANCK_WINDOW", "16")
    k = pkg.GasOpticsEcckd()
    assert k.load(LW_FSCK, device=0) == ""
    buffer_equals_separate(pkg, GasCall(pkg, k, columns(k, 11, 1541, 3), gpu))


# ---------------------------------------------------------------------------------------------------------------------
# rte_lw
# ---------------------------------------------------------------------------------------------------------------------
def solver_case(pkg, gpu, ng, nlay, ncol, seed):
    """Random tau / lay / lev as in test_rte_lw_shared_levels_is_bit_identical: optical props, a container on the views of one
    level buffer (assigned, so that nothing is copied) and one on contiguous copies of the same views."""
    import torch
    rng = np.random.default_rng(seed)
    tau = rng.uniform(0, 2, (ng, nlay, ncol)) * rng.choice([1e-9, 1e-3, 1.0], size=(ng, nlay, ncol))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    nband = 2 if ng >= 2 else 1
    b2g = np.array([[1, ng]] if nband == 1 else [[1, ng // 2], [ng // 2 + 1, ng]], dtype=np.int32)
    op = pkg.OpticalProps1scl(); op.tau = t(tau); op.band2gpt = b2g
    lev = t(rng.uniform(1, 9, (ng, nlay + 1, ncol)))
    buf = pkg.SourceFuncLW()
    buf.lay_source, buf.sfc_source = t(rng.uniform(1, 9, (ng, nlay, ncol))), t(rng.uniform(1, 9, (ng, ncol)))
    buf._lev = lev
    sep = pkg.SourceFuncLW()
    sep.lay_source, sep.sfc_source = buf.lay_source, buf.sfc_source
    sep.lev_source_inc, sep.lev_source_dec = lev[:, 1:].contiguous(), lev[:, :-1].contiguous()
    emis = t(rng.uniform(0.7, 1.0, (ncol, nband)))
    inc_flux = t(rng.uniform(0, 3, (ng, ncol)))
    return op, buf, sep, emis, inc_flux, nband


def fluxes(pkg, gpu, op, src, emis, top_at_1, nmus, nlay, ncol, **kw):
    import torch
    fl = pkg.FluxesBroadband(torch.zeros((nlay + 1, ncol), dtype=torch.float64, device=gpu),
                             torch.zeros((nlay + 1, ncol), dtype=torch.float64, device=gpu))
    assert pkg.rte_lw(op, top_at_1, src, emis, fl, n_gauss_angles=nmus, **kw) == ""
    torch.cuda.synchronize()
    return fl.flux_up, fl.flux_dn


@pytest.mark.parametrize("ncol", [1, 31, 33, 200])
@pytest.mark.parametrize("nlay", [1, 32, 33, 60, 96, 97, 137])
def test_rte_lw_buffer_equals_separate(pkg, gpu, monkeypatch, nlay, ncol):
    import torch
    for ng in (5, 6):
        op, buf, sep, emis, inc_flux, nband = solver_case(pkg, gpu, ng, nlay, ncol, 1000 + nlay + ncol + ng)
        assert buf.lev_source is not None
        for top_at_1 in (True, False):
            for nmus in (1, 2, 3):
                for tail in (0, 1):
                    pkg.set_solver_option("lw_tail_split", tail)
                    want = fluxes(pkg, gpu, op, sep, emis, top_at_1, nmus, nlay, ncol)
                    also = fluxes(pkg, gpu, op, sep, emis, top_at_1, nmus, nlay, ncol, shared_levels=True)
                    got = fluxes(pkg, gpu, op, buf, emis, top_at_1, nmus, nlay, ncol)
                    for a, b, c in zip(got, want, also):
                        assert same_bits(a, b) and same_bits(a, c), (ng, top_at_1, nmus, tail)
            # incident flux at the top
            want = fluxes(pkg, gpu, op, sep, emis, top_at_1, 2, nlay, ncol, inc_flux=inc_flux)
            got = fluxes(pkg, gpu, op, buf, emis, top_at_1, 2, nlay, ncol, inc_flux=inc_flux)
            assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
            # by-band outputs
            z = lambda *s: torch.zeros(s, dtype=torch.float64, device=gpu)
            out = []
            for src in (sep, buf):
                fb = pkg.FluxesByband(z(nband, nlay + 1, ncol), z(nband, nlay + 1, ncol), flux_up=z(nlay + 1, ncol), flux_dn=z(nlay + 1, ncol))
                assert pkg.rte_lw(op, top_at_1, src, emis, fb, n_gauss_angles=2) == ""
                out.append(fb)
            for n in ("bnd_flux_up", "bnd_flux_dn", "flux_up", "flux_dn"):
                assert same_bits(getattr(out[0], n), getattr(out[1], n)), n
        if nlay == 60:   # the layer-split solver, and the 64-bit offsets of the register-resident one
            pkg.set_solver_option("lw_solver", 1)
            for top_at_1 in (True, False):
                want = fluxes(pkg, gpu, op, sep, emis, top_at_1, 2, nlay, ncol)
                also = fluxes(pkg, gpu, op, sep, emis, top_at_1, 2, nlay, ncol, shared_levels=True)
                got = fluxes(pkg, gpu, op, buf, emis, top_at_1, 2, nlay, ncol)
                assert all(same_bits(a, b) and same_bits(a, c) for a, b, c in zip(got, want, also))
            pkg.set_solver_option("lw_solver", 0)
            monkeypatch.setenv("ECCKD_LW_NO_OFF32", "1")
            for top_at_1 in (True, False):
                want = fluxes(pkg, gpu, op, sep, emis, top_at_1, 2, nlay, ncol)
                got = fluxes(pkg, gpu, op, buf, emis, top_at_1, 2, nlay, ncol)
                assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
            monkeypatch.delenv("ECCKD_LW_NO_OFF32")
        assert buf.lev_source is not None   # nothing above copied the buffer out


# ---------------------------------------------------------------------------------------------------------------------
# containers
# ---------------------------------------------------------------------------------------------------------------------
def test_alloc_makes_one_buffer_on_float64_device_tensors(pkg, gpu, models):
    import torch
    k = models["fsck"]
    ng, nlay, ncol = k.get_ngpt(), 7, 33
    like = torch.zeros(1, dtype=torch.float64, device=gpu)
    assert pkg.lib().ecckd_has_level_buffer() == 1
    src = pkg.SourceFuncLW(); src.alloc(ncol, nlay, k, like=like)
    assert tuple(src.lev_source.shape) == (ng, nlay + 1, ncol) and not src.levels_shared
    inc, dec = src.level_views()
    assert tuple(inc.shape) == tuple(dec.shape) == (ng, nlay, ncol)
    assert inc.stride() == dec.stride() == ((nlay + 1) * ncol, ncol, 1)
    assert dec.data_ptr() == src.lev_source.data_ptr() and inc.data_ptr() == dec.data_ptr() + 8 * ncol
    # separate arrays everywhere else
    for other, kw in ((like, {"separate_levels": True}), (torch.zeros(1, dtype=torch.float32, device=gpu), {}),
                      (np.zeros(1), {}), (np.zeros(1, np.float32), {})):
        s = pkg.SourceFuncLW(); s.alloc(ncol, nlay, k, like=other, **kw)
        assert s.lev_source is None
        a, b = s.level_views()
        assert a is s.lev_source_inc and b is s.lev_source_dec and tuple(a.shape) == tuple(b.shape) == (ng, nlay, ncol)
        if isinstance(a, np.ndarray):
            assert a.flags.c_contiguous and b.flags.c_contiguous and not np.shares_memory(a, b)
        else:
            assert a.is_contiguous() and b.is_contiguous() and a.data_ptr() != b.data_ptr()
    # separate_levels() keeps the values; reading or assigning the attributes does the same
    src.lev_source.copy_(torch.rand(ng, nlay + 1, ncol, dtype=torch.float64, device=gpu))
    want_inc, want_dec = (v.clone() for v in src.level_views())
    src.separate_levels()
    assert src.lev_source is None and src.lev_source_inc.is_contiguous() and src.lev_source_dec.is_contiguous()
    assert torch.equal(src.lev_source_inc, want_inc) and torch.equal(src.lev_source_dec, want_dec)
    s2 = pkg.SourceFuncLW(); s2.alloc(ncol, nlay, k, like=like)
    s2.lev_source.copy_(torch.cat([want_dec[:, :1], want_inc], 1))
    assert torch.equal(s2.lev_source_dec, want_dec) and s2.lev_source is None and torch.equal(s2.lev_source_inc, want_inc)
    # two independent arrays again: scaling both scales every level once
    s2.lev_source_inc.mul_(2.0); s2.lev_source_dec.mul_(2.0)
    assert torch.equal(s2.lev_source_inc, 2.0 * want_inc) and torch.equal(s2.lev_source_dec, 2.0 * want_dec)


def test_other_solvers_on_an_allocated_container(pkg, gpu, models):
    """gas_optics, then the two-stream and the rescaled solver (which read two separate arrays: the container copies its
    buffer out, once) and planck_sources, against the same calls on a separate_levels=True container; then gas_optics and
    rte_lw again on the demoted container."""
    import torch
    k = models["fsck"]
    ng, nlay, ncol = k.get_ngpt(), 60, 130
    cols = columns(k, 9, ncol, nlay)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    gc = helpers.product_gas_concs(pkg, cols, t)
    plev, tlay, tsfc, tlev = (t(cols[n]) for n in ("plev", "tlay", "tsfc", "tlev"))
    emis = t(cols["sfc_emis"][:, None])
    rng = np.random.default_rng(5)
    ssa, g = t(rng.uniform(0, 0.9, (ng, nlay, ncol))), t(rng.uniform(-0.2, 0.8, (ng, nlay, ncol)))
    z = lambda: pkg.FluxesBroadband(torch.zeros((nlay + 1, ncol), dtype=torch.float64, device=gpu),
                                    torch.zeros((nlay + 1, ncol), dtype=torch.float64, device=gpu))
    out = {}
    for sepl in (True, False):
        op = pkg.OpticalProps2str(); op.alloc_2str(ncol, nlay, k, like=plev)
        op.ssa.copy_(ssa); op.g.copy_(g)
        src = pkg.SourceFuncLW(); src.alloc(ncol, nlay, k, like=plev, separate_levels=sepl)
        assert (src.lev_source is None) == sepl
        assert k.gas_optics(None, plev, tlay, tsfc, gc, op, src, tlev=tlev) == ""
        assert (src.lev_source is None) == sepl and src.levels_shared
        r = [z() for _ in range(5)]
        assert pkg.rte_lw(op, True, src, emis, r[0]) == ""
        assert (src.lev_source is None) == sepl
        assert pkg.rte_lw(op, True, src, emis, r[1], use_2stream=True) == ""
        assert src.lev_source is None
        assert pkg.rte_lw(op, True, src, emis, r[2], rescaled=True, n_gauss_angles=2) == ""
        assert k.planck_sources(tlay, tsfc, src, tlev=tlev) == ""
        planck = [a.clone() for a in (src.lay_source, src.lev_source_inc, src.lev_source_dec, src.sfc_source)]
        # the demoted container goes on working
        assert k.gas_optics(None, plev, tlay, tsfc, gc, op, src, tlev=tlev) == ""
        assert pkg.rte_lw(op, True, src, emis, r[3]) == ""
        torch.cuda.synchronize()
        out[sepl] = ([(f.flux_up, f.flux_dn) for f in r[:4]], planck, op.tau.clone())
    for (a_up, a_dn), (b_up, b_dn) in zip(out[True][0], out[False][0]):
        assert same_bits(a_up, b_up) and same_bits(a_dn, b_dn)
    for a, b in zip(out[True][1], out[False][1]):
        assert same_bits(a, b)
    assert same_bits(out[True][2], out[False][2])
    assert same_bits(out[False][0][0][0], out[False][0][3][0]) and same_bits(out[False][0][0][1], out[False][0][3][1])


def test_planck_sources_into_the_buffer(pkg, gpu, models):
    """ecckd_planck_sources takes the level buffer: fast and reference-order kernels, odd g-point... and layer counts."""
    import torch
    k = models["rrtmgp"]
    for ncol, nlay in ((1, 1), (65, 2), (1541, 3), (130, 61)):
        cols = columns(k, 11, ncol, nlay)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
        tlay, tsfc, tlev = (t(cols[n]) for n in ("tlay", "tsfc", "tlev"))
        for mode in (pkg.FAST, pkg.REFERENCE_ORDER):
            pkg.set_arithmetic(mode)
            res = []
            for sepl in (True, False):
                src = pkg.SourceFuncLW(); src.alloc(ncol, nlay, k, like=tlay, separate_levels=sepl)
                for a in (src.lay_source, src.sfc_source) + tuple(src.level_views() if sepl else (src.lev_source,)):
                    a.fill_(SENTINEL)
                assert k.planck_sources(tlay, tsfc, src, tlev=tlev) == ""
                assert (src.lev_source is None) == sepl
                torch.cuda.synchronize()
                res.append([a.contiguous() for a in (src.lay_source,) + tuple(src.level_views()) + (src.sfc_source,)])
            for a, b in zip(*res):
                assert same_bits(a, b), (ncol, nlay, mode)


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
LEAD = ": lev_source_inc == lev_source_dec + ncol names one level buffer (ncol,nlay+1,ngpt); "


def test_host_arrays_are_refused(pkg, gpu, models):
    k = models["fsck"]
    ng, nlay, ncol = k.get_ngpt(), 3, 17
    cols = columns(k, 7, ncol, nlay)
    to = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    gc = helpers.product_gas_concs(pkg, cols, to)
    n, names, ptrs, cs, ls, sc, _ = k._gas_args(gc, ncol, nlay, pkg.HOST)
    plev, tlay, tsfc, tlev = (to(cols[v]) for v in ("plev", "tlay", "tsfc", "tlev"))
    lev = np.full((ng, nlay + 1, ncol), SENTINEL)
    tau, lay, sfc = np.full((ng, nlay, ncol), SENTINEL), np.full((ng, nlay, ncol), SENTINEL), np.full((ng, ncol), SENTINEL)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = pkg.lib().ecckd_gas_optics_lw(k._need(), ncol, nlay, p(plev), p(tlay), p(tsfc), p(tlev), n, names, ptrs, cs, ls, sc, p(tau),
                                       p(lay), C.c_void_p(lev.ctypes.data + 8 * ncol), p(lev), p(sfc), pkg.HOST, None)
    assert rc != 0
    assert pkg.last_error() == "ecckd_gas_optics_lw" + LEAD + "host arrays (ECCKD_HOST) are not taken in that form: pass two separate arrays"
    assert all(np.all(a == SENTINEL) for a in (lev, tau, lay, sfc))
    # the solver
    b2g = np.array([1, ng], dtype=np.int32)
    emis, fu, fd = np.ones((ncol, 1)), np.full((nlay + 1, ncol), SENTINEL), np.full((nlay + 1, ncol), SENTINEL)
    tau[:] = 1.0
    rc = pkg.lib().ecckd_rte_lw(0, ncol, nlay, ng, 1, 1, p(tau), p(lay), C.c_void_p(lev.ctypes.data + 8 * ncol), p(lev), p(sfc), 1,
                                p(b2g), p(emis), p(fu), p(fd), pkg.HOST, None)
    assert rc != 0
    assert pkg.last_error() == "ecckd_rte_lw" + LEAD + "host arrays (ECCKD_HOST) are not taken in that form: pass two separate arrays"
    assert np.all(fu == SENTINEL) and np.all(fd == SENTINEL)


def test_single_precision_is_refused(pkg, gpu, models):
    import torch
    k = models["fsck"]
    ng, nlay, ncol = k.get_ngpt(), 3, 17
    cols = columns(k, 7, ncol, nlay)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu)
    gc = helpers.product_gas_concs(pkg, cols, to)
    n, names, ptrs, cs, ls, sc, _ = k._gas_args(gc, ncol, nlay, pkg.DEVICE, True)
    plev, tlay, tsfc, tlev = (to(cols[v]) for v in ("plev", "tlay", "tsfc", "tlev"))
    f = lambda *s: torch.full(s, SENTINEL, dtype=torch.float32, device=gpu)
    lev, tau, lay, sfc = f(ng, nlay + 1, ncol), f(ng, nlay, ncol), f(ng, nlay, ncol), f(ng, ncol)
    p = lambda a: C.c_void_p(a.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = pkg.lib().ecckd_gas_optics_lw_f32(k._need(), ncol, nlay, p(plev), p(tlay), p(tsfc), p(tlev), n, names, ptrs, cs, ls, sc,
                                           p(tau), p(lay), C.c_void_p(lev.data_ptr() + 4 * ncol), p(lev), p(sfc), pkg.DEVICE, stream)
    torch.cuda.synchronize()
    assert rc != 0
    assert pkg.last_error() == "ecckd_gas_optics_lw" + LEAD + "single precision does not take that form: pass two separate arrays"
    assert all(bool((a == SENTINEL).all()) for a in (lev, tau, lay, sfc))
    b2g = np.array([1, ng], dtype=np.int32)
    emis, fu, fd = torch.ones((ncol, 1), dtype=torch.float32, device=gpu), f(nlay + 1, ncol), f(nlay + 1, ncol)
    tau.fill_(1.0)
    rc = pkg.lib().ecckd_rte_lw_f32(0, ncol, nlay, ng, 1, 1, p(tau), p(lay), C.c_void_p(lev.data_ptr() + 4 * ncol), p(lev), p(sfc), 1,
                                    C.c_void_p(b2g.ctypes.data), p(emis), p(fu), p(fd), pkg.DEVICE, stream)
    torch.cuda.synchronize()
    assert rc != 0
    assert pkg.last_error() == "ecckd_rte_lw" + LEAD + "single precision does not take that form: pass two separate arrays"
    assert bool((fu == SENTINEL).all()) and bool((fd == SENTINEL).all())


def test_entry_points_without_the_form_refuse_it(pkg, gpu):
    """The two-stream solver through the C ABI (the Python wrapper copies a container's buffer out before it calls)."""
    import torch
    ng, nlay, ncol = 4, 5, 9
    f = lambda *s: torch.full(s, 0.5, dtype=torch.float64, device=gpu)
    lev, tau, sfc, emis = f(ng, nlay + 1, ncol), f(ng, nlay, ncol), f(ng, ncol), f(ncol, 1)
    fu, fd = torch.full((nlay + 1, ncol), SENTINEL, dtype=torch.float64, device=gpu), torch.full((nlay + 1, ncol), SENTINEL, dtype=torch.float64, device=gpu)
    b2g = np.array([1, ng], dtype=np.int32)
    p = lambda a: C.c_void_p(a.data_ptr())
    rc = pkg.lib().ecckd_rte_lw_2stream(0, ncol, nlay, ng, 1, p(tau), p(tau), p(tau), None, C.c_void_p(lev.data_ptr() + 8 * ncol), p(lev),
                                        p(sfc), 1, C.c_void_p(b2g.ctypes.data), p(emis), None, p(fu), p(fd), pkg.DEVICE,
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc != 0
    assert pkg.last_error() == "ecckd_rte_lw_2stream" + LEAD + "this entry point does not take that form: pass two separate arrays"
    assert bool((fu == SENTINEL).all()) and bool((fd == SENTINEL).all())
