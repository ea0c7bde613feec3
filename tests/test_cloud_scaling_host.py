"""CPU tests of the sampled optical-depth scaling (in-cloud water variability): the new symbols and their bindings, the
lognormal table builder against an mpmath evaluation of the same bin means, the numpy restatement of the sampler
(tests/cloud_scaling_ref.py) -- its seen cells are the bits of the mask sampler, its statistics those of the table, a
column depends on its global index only --, the refusals in their documented order where no GPU is, and the scratch sizes
against their formulas.  Nothing computes on the CPU."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import __graft_entry__ as entry
import cloud_scaling_ref as ref
import mcica_helpers as mh
from conftest import LW_FSCK, LW_RRTMGP, SW_WIDE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ecckd_cloud_scaling_create", "ecckd_cloud_scaling_destroy", "ecckd_cloud_scaling_get_nfsd", "ecckd_cloud_scaling_get_nq",
           "ecckd_cloud_scaling_get_fsd0", "ecckd_cloud_scaling_get_dfsd", "ecckd_cloud_scaling_get_values",
           "ecckd_cloud_scaling_lognormal", "ecckd_cloud_scaling_sample", "ecckd_increment_scaled", "ecckd_increment_scaled_f32",
           "ecckd_lw_flux_scaled", "ecckd_sw_flux_scaled", "ecckd_lw_flux_scaled_scratch_bytes", "ecckd_sw_flux_scaled_scratch_bytes")


def test_symbols_are_declared_exported_and_bound(pkg):
    L = pkg.lib()
    for s in SYMBOLS:
        assert s in entry.exported_symbols(), s
        assert hasattr(L, s) and getattr(L, s).argtypes is not None, s
        assert "_fluxes" not in s   # (tests/test_fused_call_marshalling_host.py pins every symbol that has it)
    # the argument lists of the McICA calls, the scaling in the mask's place
    assert len(L.ecckd_lw_flux_scaled.argtypes) == len(L.ecckd_lw_fluxes_allsky_mcica.argtypes) == 25
    assert len(L.ecckd_sw_flux_scaled.argtypes) == len(L.ecckd_sw_fluxes_allsky_mcica.argtypes) == 27
    assert len(L.ecckd_cloud_scaling_sample.argtypes) == 16
    assert len(L.ecckd_increment_scaled.argtypes) == len(L.ecckd_increment_masked.argtypes) == 15
    assert L.ecckd_lw_flux_scaled_scratch_bytes.restype is C.c_size_t and L.ecckd_sw_flux_scaled_scratch_bytes.restype is C.c_size_t
    header = open(os.path.join(ROOT, "include", "ecckd_hip.h")).read()
    assert "PARITY WITH ecRad AND RTE-RRTMGP IS UNPINNED" in header and "gamma distribution is not built by the library" in header
    sig = inspect.signature(pkg.sample_cloud_scaling)
    assert list(sig.parameters) == ["cloud_frac", "ngpt", "table", "fsd", "overlap", "overlap_param", "seed", "col0", "device",
                                    "return_mask"]
    assert sig.parameters["return_mask"].default is False
    for cls in (pkg.OpticalProps1scl, pkg.OpticalProps2str):
        assert list(inspect.signature(cls.increment_scaled).parameters) == ["self", "other", "cloud_scaling", "band2gpt"]
    for name in ("lw_flux_scaled", "sw_flux_scaled", "lw_flux_scaled_scratch_bytes", "sw_flux_scaled_scratch_bytes"):
        assert callable(getattr(pkg.GasOpticsEcckd, name)), name
    assert callable(pkg.CloudScaling.from_table) and callable(pkg.CloudScaling.lognormal)


# ---- the table builder ----

TABLES = ((5, 0.0, 0.5, 16), (3, 0.25, 0.75, 8), (4, 0.0, 1.0, 1), (2, 0.1, 3.0, 128), (3, 0.5, 0.5, 7))


def test_lognormal_table_against_mpmath(pkg):
    """Bar per row: 16 * nq * 2^-52 * max(1, largest value of the row).  A bin mean is nq times a difference of two Phi
    values of absolute error about 2^-52 each; a one-ulp residual of the quantile solve moves Phi(z - sigma) by that residual
    times the scaling at the bin edge; the factor 16 covers a few ulp of erfc."""
    for nfsd, fsd0, dfsd, nq in TABLES:
        got = pkg.CloudScaling.lognormal_values(nfsd, fsd0, dfsd, nq)
        want = ref.lognormal_mp(nfsd, fsd0, dfsd, nq)
        assert got.shape == want.shape == (nfsd, nq)
        for k in range(nfsd):
            bar = 16 * nq * 2.0 ** -52 * max(1.0, want[k].max())
            dist = np.abs(got[k] - want[k]).max()
            print("lognormal nq %d fsd %.3g: distance %.3e, bar %.3e" % (nq, fsd0 + k * dfsd, dist, bar))
            assert dist <= bar, (nfsd, fsd0, dfsd, nq, k, dist, bar)
            assert abs(got[k].mean() - 1.0) <= nq * 2.0 ** -50, (nq, k, got[k].mean())
            assert np.all(np.diff(got[k]) >= 0) and np.all(got[k] > 0)


def test_lognormal_rows(pkg):
    v = pkg.CloudScaling.lognormal_values(5, 0.0, 0.5, 16)
    assert np.array_equal(v[0], np.ones(16))   # f = 0: exactly ones
    # bin means under-disperse: the standard deviation of a row is below its FSD and approaches it as nq grows
    assert abs(v[2].std() - 0.908) < 1e-3
    sd = [pkg.CloudScaling.lognormal_values(2, 1.0, 1.0, nq)[0].std() for nq in (8, 16, 128, 4096)]
    assert sd == sorted(sd) and sd[0] < 0.87 and 0.98 < sd[-1] < 1.0, sd
    for bad, text in (((0, 0.0, 0.5, 16), "nfsd must be at least 1"), ((2, 0.0, 0.5, 0), "nq must be at least 1"),
                      ((2, -0.1, 0.5, 4), "fsd0 must not be negative"), ((2, 0.0, 0.0, 4), "dfsd must be greater than 0"),
                      ((2, 0.0, float("nan"), 4), "dfsd must be greater than 0")):
        with pytest.raises(ValueError) as e:
            pkg.CloudScaling.lognormal_values(*bad)
        assert text in str(e.value), bad
    assert pkg.lib().ecckd_cloud_scaling_lognormal(2, 0.0, 0.5, 4, None) == 1 and "null argument" in pkg.last_error()


def test_table_object_and_its_refusals(pkg):
    v = pkg.CloudScaling.lognormal_values(5, 0.0, 0.5, 16)
    t = pkg.CloudScaling.from_table(v, 0.0, 0.5, device=-1)
    assert (t.get_nfsd(), t.get_nq(), t.get_fsd0(), t.get_dfsd()) == (5, 16, 0.0, 0.5)
    assert np.array_equal(t.get_values(), v)
    t.finalize()
    with pytest.raises(RuntimeError):
        t.get_nq()
    L = pkg.lib()
    h = C.c_void_p()
    P = lambda a: C.c_void_p(a.ctypes.data)
    bad = v.copy(); bad[3, 2] = np.nan
    neg = v.copy(); neg[0, 0] = -1e-300
    # each refusal with every later one armed as well
    for args, text in (((-1, 1, 0.0, 0.0, 0, None, None), "null argument (the handle)"),
                       ((-1, 1, 0.0, 0.0, 0, None, C.byref(h)), "nfsd must be at least 2"),
                       ((-1, 2, 0.0, 0.0, 0, None, C.byref(h)), "nq must be at least 1"),
                       ((-1, 2, 0.0, 0.0, 3, None, C.byref(h)), "dfsd must be greater than 0"),
                       ((-1, 2, 0.0, -1.0, 3, None, C.byref(h)), "dfsd must be greater than 0"),
                       ((-1, 2, 0.0, float("nan"), 3, None, C.byref(h)), "dfsd must be greater than 0"),
                       ((-1, 5, 0.0, 0.5, 16, None, C.byref(h)), "null argument (values)"),
                       ((7, 5, 0.0, 0.5, 16, P(bad), C.byref(h)), "must be finite and not negative (entry 50)"),
                       ((7, 5, 0.0, 0.5, 16, P(neg), C.byref(h)), "must be finite and not negative (entry 0)")):
        assert L.ecckd_cloud_scaling_create(*args) == 1
        assert text in pkg.last_error(), (args, pkg.last_error())
        assert not h.value
    assert L.ecckd_cloud_scaling_get_nq(None) == 0 and L.ecckd_cloud_scaling_get_dfsd(None) == 0.0
    L.ecckd_cloud_scaling_destroy(None)
    with pytest.raises(ValueError):
        pkg.CloudScaling.from_table(np.ones(4), 0.0, 0.5, device=-1)


# ---- the restatement of the sampler ----

NLAY, NCOL, NG = 12, 4096, 32
FSD_NODES = dict(nfsd=5, fsd0=0.0, dfsd=0.5, nq=16)


def _inputs():
    rng = np.random.default_rng(20240607)
    cf = np.zeros((NLAY, NCOL))
    cf[1:4] = np.array([0.3, 0.7, 0.5])[:, None]
    cf[5] = 0.4
    cf[7:10] = rng.uniform(0.05, 1.0, (3, NCOL))
    cf[10] = 1.0
    fsd = rng.uniform(0.0, 2.0, (NLAY, NCOL))
    fsd[2] = np.nan    # -> row 0, weight 0: FSD 0
    fsd[5] = 0.0
    fsd[8] = 1.0       # exactly on a node
    fsd[0] = np.inf    # a clear layer: must not matter
    al = rng.uniform(0.0, 1.0, (NLAY - 1, NCOL))
    return cf, fsd, al


@pytest.fixture(scope="module")
def restated(pkg):
    v = pkg.CloudScaling.lognormal_values(FSD_NODES["nfsd"], FSD_NODES["fsd0"], FSD_NODES["dfsd"], FSD_NODES["nq"])
    cf, fsd, al = _inputs()
    out = {}
    for ov, a in ((mh.MAX_RAN, None), (mh.EXP_RAN, al)):
        out[ov] = ref.sample(cf, NG, v, 0.0, 0.5, fsd, ov, a, seed=99, col0=2 ** 33 + 5)
    return v, cf, fsd, al, out


def test_restatement_sees_what_the_mask_sampler_sees(restated):
    v, cf, fsd, al, out = restated
    for ov, a in ((mh.MAX_RAN, None), (mh.EXP_RAN, al)):
        s, m = out[ov]
        assert s.dtype == np.float32 and s.shape == (NG, NLAY, NCOL)
        want = mh.sample(cf, NG, ov, a, seed=99, col0=2 ** 33 + 5)
        assert np.array_equal(m, want)
        assert np.array_equal(s > 0, np.moveaxis(mh.unpack(want, NG), -1, 0))
        assert not np.any(np.signbit(s)) and np.all(np.isfinite(s))
        # FSD 0 and a NaN FSD: exactly 1 where seen
        for l in (2, 5):
            assert np.all(s[:, l][s[:, l] > 0] == 1.0)
        assert np.all(s[:, 10] > 0) and not np.any(s[:, [0, 4, 6, 11]])
        # on a node the values are the row's own, rounded to float
        assert set(np.unique(s[:, 8])) <= set(v[2].astype(np.float32)) | {np.float32(0)}
        # the mean over the seen cells of a layer: the row mean, 1 (0.9997 .. 1.0009 in the prototype of the definition)
        for l in (1, 3, 7, 8, 9, 10):
            seen = s[:, l][s[:, l] > 0].astype(np.float64)
            assert abs(seen.mean() - 1.0) <= 5 * 1.6 / np.sqrt(seen.size), (ov, l, seen.mean())
        # clear layers ignore fsd altogether
        fsd2 = fsd.copy(); fsd2[[0, 4, 6, 11]] = -7.0
        assert np.array_equal(ref.sample(cf[:, :64], NG, v, 0.0, 0.5, fsd2[:, :64], ov, None if a is None else a[:, :64], 99, 2 ** 33 + 5)[0],
                              s[:, :, :64])


def test_restatement_interpolates_and_clamps():
    v = np.array([[1.0, 1.0, 1.0, 1.0], [0.5, 0.75, 1.0, 1.75], [0.25, 0.5, 1.0, 2.25]])
    cf = np.ones((1, 2000))
    for fsd, row in ((-3.0, v[0]), (0.0, v[0]), (0.5, v[1]), (0.25, v[0] + 0.5 * (v[1] - v[0])), (1.0, v[1] + 1.0 * (v[2] - v[1])),
                     (9.0, v[1] + 1.0 * (v[2] - v[1])), (np.nan, v[0]), (np.inf, v[2])):
        s, m = ref.sample(cf, 8, v, 0.0, 0.5, fsd, seed=3)
        assert set(np.unique(s)) == set(row.astype(np.float32)), (fsd, np.unique(s))
        assert np.all(m == np.uint64(255))
    # overcast: p is the rank itself, so the bin of a g-point is int(u * nq)
    s, _ = ref.sample(cf, 8, v, 0.0, 0.5, 0.5, seed=3)
    u = mh.draws(3, np.arange(2000), 0, 8, 0)
    assert np.array_equal(s[:, 0, :].T, v[1][np.minimum((u * 4).astype(int), 3)].astype(np.float32))


def test_restatement_is_shard_independent(restated):
    v, cf, fsd, al, out = restated
    c0 = 2 ** 33 + 5
    for ov, a in ((mh.MAX_RAN, None), (mh.EXP_RAN, al)):
        s, m = out[ov]
        cut = 1000
        for lo, hi in ((0, cut), (cut, NCOL)):
            sh, mk = ref.sample(cf[:, lo:hi], NG, v, 0.0, 0.5, fsd[:, lo:hi], ov, None if a is None else a[:, lo:hi], 99, c0 + lo)
            assert np.array_equal(sh, s[:, :, lo:hi]) and np.array_equal(mk, m[:, lo:hi])
        other = ref.sample(cf[:, cut:], NG, v, 0.0, 0.5, fsd[:, cut:], ov, None if a is None else a[:, cut:], 99, c0)[0]
        assert not np.array_equal(other, s[:, :, cut:])


# ---- refusals where no GPU is ----

def test_sampler_refusals_in_documented_order(pkg):
    t = pkg.CloudScaling.lognormal(5, 0.0, 0.5, 16, device=-1)
    cf = np.full((6, 4), 2.0)   # (outside [0, 1]: every earlier refusal wins over it)
    al = np.full((5, 4), 0.5)

    def msg(*a, **k):
        with pytest.raises(ValueError) as e:
            pkg.sample_cloud_scaling(*a, **k)
        return str(e.value)

    assert "at most 64 g-points" in msg(cf, 65, t, 1.0, overlap=7) and "not 65" in msg(cf, 65, t, 1.0, overlap=7)
    assert "ngpt must be at least 1" in msg(cf, 0, t, 1.0, overlap=7)
    assert "unknown overlap 7" in msg(cf, 32, t, 1.0, overlap=7)
    assert "unknown overlap" in msg(cf, 32, t, 1.0, overlap="random")
    assert "needs overlap_param" in msg(cf, 32, t, 1.0, overlap="exp_ran")
    assert "cloud fraction outside [0, 1]" in msg(cf, 32, t, 1.0, overlap="exp_ran", overlap_param=al)
    ok = np.full((6, 4), 0.5)
    ok[2, 1] = np.nan
    assert "overlap parameter outside [0, 1]" in msg(ok, 32, t, 1.0, overlap="exp_ran", overlap_param=al + 1.0)
    # valid arguments: a host-only table, never a scaling made on the CPU
    for fsd in (1.0, np.full((6, 4), 1.0)):
        assert "host-only scaling table" in msg(ok, 32, t, fsd, return_mask=True)
    # through ctypes: null pointers come before the memory space, a null table before "no device"
    L = pkg.lib()
    P = lambda a: C.c_void_p(a.ctypes.data)
    out = np.zeros((32, 6, 4), dtype=np.float32)
    names = ("dev", "ncol", "nlay", "ng", "ov", "cf", "al", "fsd", "fc", "table", "seed", "col0", "out", "mask", "space", "stream")

    def call(**k):
        a = dict(dev=0, ncol=4, nlay=6, ng=32, ov=0, cf=P(ok), al=None, fsd=None, fc=1.0, table=t._need(), seed=1, col0=0,
                 out=P(out), mask=None, space=pkg.HOST, stream=None)
        assert set(k) <= set(a)
        a.update(k)
        return L.ecckd_cloud_scaling_sample(*[a[n] for n in names])

    assert call(nlay=0, cf=None) == 1 and "bad ncol/nlay" in pkg.last_error()
    for gone in ("cf", "out"):
        assert call(space=7, table=None, **{gone: None}) == 1 and "cloud_frac and scaling are required" in pkg.last_error()
    assert call(space=7, table=None) == 1 and "null argument (the scaling table)" in pkg.last_error()
    assert call(space=7) == 1 and "bad memspace" in pkg.last_error()
    assert call(dev=3) == 1 and "host-only scaling table" in pkg.last_error()
    assert not out.any()


def _host_model(pkg, path):
    k = pkg.GasOpticsEcckd()
    assert k.load(path, device=-1) == ""
    return k


def test_increment_scaled_refusals(pkg):
    """ecckd_increment's list; more than 64 g-points are no refusal; no device: an error."""
    ng, nlay, ncol = 70, 3, 5
    op1, op2 = pkg.OpticalProps1scl(), pkg.OpticalProps1scl()
    op1.tau, op2.tau = np.ones((ng, nlay, ncol)), np.ones((ng, nlay, ncol))
    sc = np.ones((ng, nlay, ncol), dtype=np.float32)
    assert "float32" in op1.increment_scaled(op2, sc.astype(np.float64))
    assert "shape" in op1.increment_scaled(op2, sc[1:])
    import torch
    if not torch.cuda.is_available():
        assert "no HIP device" in op1.increment_scaled(op2, sc)
        assert np.all(op1.tau == 1.0)
    op2s = pkg.OpticalProps2str()
    op2s.tau, op2s.ssa, op2s.g = np.ones((2, nlay, ncol)), np.ones((2, nlay, ncol)), None
    m = op1.increment_scaled(op2s, sc, band2gpt=np.array([[1, 30], [32, 70]]))
    assert m   # (ssa without g, or bands that do not tile: ecckd_increment's own answers)


def test_fused_scaled_calls_refuse_in_the_order_of_the_allsky_calls(pkg):
    nlay, ncol = 60, 4
    gc = pkg.GasConcs(["h2o"]); gc.set_vmr("h2o", 1e-3)
    plev, tlay, tsfc, tlev = (np.full((nlay + 1, ncol), 1e4), np.full((nlay, ncol), 250.), np.full(ncol, 250.),
                              np.full((nlay + 1, ncol), 250.))
    bb = lambda: np.full((nlay + 1, ncol), -7.)
    for path in (LW_RRTMGP, LW_FSCK):
        k = _host_model(pkg, path)
        ng, nb = k.get_ngpt(), k.get_nband()
        part = pkg.OpticalProps2str()
        assert part.alloc_2str_bands(ncol, nlay, k) == ""
        fl = pkg.FluxesBroadband(bb(), bb())
        sc = np.ones((ng, nlay, ncol), dtype=np.float32)
        emis = np.full((ncol, nb), 0.98)
        call = lambda s=sc, p=part, **kw: k.lw_flux_scaled(plev, tlay, tsfc, tlev, gc, True, emis, p, fl, s, **kw)
        assert "cloud_scaling" in call(sc.astype(np.float64)) and "float32" in call(sc.astype(np.float64))
        assert "cloud_scaling" in call(sc[1:]) and "shape" in call(sc[1:])
        pkg.set_arithmetic(pkg.REFERENCE_ORDER)
        try:
            assert call() == "ecckd_lw_fluxes_allsky: needs the fast arithmetic mode (ecckd_set_arithmetic(0))"
        finally:
            pkg.set_arithmetic(pkg.FAST)
        for s in (sc, None):   # (None: the unmasked call)
            assert call(s).startswith("ecckd: host-only model"), s
        assert call(n_gauss_angles=3, inc_flux=np.full((ng, ncol), 1.)).startswith("ecckd: host-only model")
        assert np.all(fl.flux_up == -7.)
        short = pkg.OpticalProps2str()
        short.tau, short.ssa, short.g = part.tau[1:], part.ssa[1:], part.g[1:]
        assert call(p=short).startswith("ecckd_lw_fluxes_allsky: nband_p = %d but the model has %d bands" % (nb - 1, nb))
    ks = _host_model(pkg, SW_WIDE)
    ng, nb = ks.get_ngpt(), ks.get_nband()
    part = pkg.OpticalProps2str()
    assert part.alloc_2str_bands(ncol, nlay, ks) == ""
    fl = pkg.FluxesBroadband(bb(), bb(), bb())
    sc = np.ones((ng, nlay, ncol), dtype=np.float32)
    alb, mu0 = np.full((ncol, nb), 0.2), np.full(ncol, 0.5)
    call = lambda s=sc, **kw: ks.sw_flux_scaled(plev, tlay, gc, True, mu0, alb, alb, part, fl, s, **kw)
    assert "float32" in call(sc.astype(np.float64))
    pkg.set_arithmetic(pkg.REFERENCE_ORDER)
    try:
        assert call() == "ecckd_sw_fluxes_allsky: needs the fast arithmetic mode (ecckd_set_arithmetic(0))"
    finally:
        pkg.set_arithmetic(pkg.FAST)
    for kw in (dict(), dict(delta_scale=False), dict(toa_scale=np.full(ncol, 1.)), dict(s=None)):
        assert call(**kw).startswith("ecckd: host-only model"), kw


def _align256(n):
    return (n + 255) // 256 * 256


def test_scratch_sizes_are_the_documented_ones(pkg):
    L = pkg.lib()
    for path in (LW_RRTMGP, LW_FSCK):
        k = _host_model(pkg, path)
        ng = k.get_ngpt()
        assert k.lw_flux_scaled_scratch_bytes(0, 60) == 0 and k.lw_flux_scaled_scratch_bytes(5, 0) == 0
        assert k.lw_flux_scaled_scratch_bytes(1000, 60) == (1000 * 60 * ng + 32) * 8   # the optical depth alone
        for ncol, nlay in ((17, 61), (5, 137)):   # ... plus three source arrays, the surface source, the solver's ring
            want = (4 * ncol * nlay * ng + ncol * ng + 64) * 8 + L.ecckd_rte_lw_scratch_bytes(ncol, nlay, ng)
            assert k.lw_flux_scaled_scratch_bytes(ncol, nlay) == want, (ncol, nlay)
    assert L.ecckd_lw_flux_scaled_scratch_bytes(None, 10, 60) == 0 and L.ecckd_sw_flux_scaled_scratch_bytes(None, 10, 60, 1) == 0
    k = _host_model(pkg, SW_WIDE)
    ng, nb = k.get_ngpt(), k.get_nband()
    for ncol, nlay in ((1000, 60), (17, 61), (100000, 60)):
        ring = L.ecckd_rte_sw_scratch_bytes(ncol, nlay, ng)   # the two-pass solver's term at every layer count
        assert ring > 0
        for ds in (0, 1):
            got = k.sw_flux_scaled_scratch_bytes(ncol, nlay, bool(ds))
            floor = _align256(ncol * nlay * ng * 8) + ring + (3 * _align256(ncol * nlay * nb * 8) if ds else 0)
            # (a host-only model has no device to plan a tail split for: the ring is the whole term)
            assert got == floor, (ncol, nlay, ds, got, floor)
