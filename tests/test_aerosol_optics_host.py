"""Aerosol optics without a GPU: the numpy restatement (tests/aerosol_optics_ref.py) against an independent scalar loop
written here, every refusal of ``ecckd_aerosol_optics_create_lut`` / ``ecckd_aerosol_optics`` with its message and its
place in the order the header states (a host-only object, device -1, serves: every refusal comes before a device is asked
for), the getters, the Python mirror's own messages, the exported symbols and the synthetic tables and inputs."""
import ctypes as C
import math

import numpy as np
import pytest

import aerosol_optics_ref as ref
from rte_ecckd_amd import synthetic

HOST, DEVICE, MIXED = 0, 1, 2
TABLE_NAMES = ("merra_aero_bin_lims", "aero_rh", "aero_dust_tbl", "aero_salt_tbl", "aero_sulf_tbl", "aero_bcar_tbl",
               "aero_bcar_rh_tbl", "aero_ocar_tbl", "aero_ocar_rh_tbl")


# ---- the restatement against a scalar double loop (Python floats are IEEE doubles; one operation per statement) ----
def scalar_cell(lut, kinds, sizes, masses, rh, band, two_stream, op1=None):
    lev, lims = lut["aero_rh"], lut["merra_aero_bin_lims"]
    nrh, nbin = len(lev), len(lims)
    i = 0
    for j in range(1, nrh - 1):
        if rh >= lev[j]:
            i += 1
    d = float(lev[i + 1]) - float(lev[i])
    w = (rh - float(lev[i])) / d
    w = w if w > 0 else 0.0
    w = w if w < 1 else 1.0
    T = TS = TSG = A = 0.0
    for k, r, m in zip(kinds, sizes, masses):
        if not (1 <= k <= 7 and m > 0):
            continue
        b = None
        if k in (1, 2):
            for n in range(nbin):
                if lims[n][0] <= r and r < lims[n][1]:
                    b = n
                    break
            if b is None:
                continue
        v = []
        for q in range(3):
            if k in ref.RH_DEPENDENT:
                tbl = {2: lambda x: lut["aero_salt_tbl"][band][b][x][q], 3: lambda x: lut["aero_sulf_tbl"][band][x][q],
                       4: lambda x: lut["aero_bcar_rh_tbl"][band][x][q], 6: lambda x: lut["aero_ocar_rh_tbl"][band][x][q]}[k]
                lo, hi = float(tbl(i)), float(tbl(i + 1))
                slope = hi - lo
                ws = w * slope
                v.append(lo + ws)
            else:
                v.append(float({1: lambda: lut["aero_dust_tbl"][band][b][q], 5: lambda: lut["aero_bcar_tbl"][band][q],
                                7: lambda: lut["aero_ocar_tbl"][band][q]}[k]()))
        t = m * v[0]
        ts = t * v[1]
        tsg = ts * v[2]
        T += t
        TS += ts
        TSG += tsg
        A += t - ts
    eps = 2.0 ** -52
    if not two_stream:
        return (A,) if op1 is None else (op1[0] + A,)
    tau2, ssa2, g2 = T, TS / (T if T > eps else eps), TSG / (TS if TS > eps else eps)
    if op1 is None:
        return tau2, ssa2, g2
    e3 = 3.0 * 2.2250738585072014e-308
    tau1, ssa1, g1 = op1
    tau12 = tau1 + tau2
    tscat1 = tau1 * ssa1
    tscat2 = tau2 * ssa2
    tsg2 = tscat2 * g2
    tauscat12 = tscat1 + tscat2
    num = tscat1 * g1
    num = num + tsg2
    return tau12, tauscat12 / (tau12 if tau12 > e3 else e3), num / (tauscat12 if tauscat12 > e3 else e3)


def small_case(nspec=3, nlay=3, ncol=40, nband=2, nbin=3, nrh=5):
    lut = synthetic.aerosol_lut(nband, nbin, nrh)
    rng = np.random.default_rng(7)
    kind = rng.integers(0, 8, size=(nspec, nlay, ncol)).astype(np.int32)
    size = 0.05 * 300.0 ** rng.uniform(size=kind.shape)          # some below the first and above the last bin
    mass = np.where(rng.uniform(size=kind.shape) < 0.8, 1e-5 * rng.uniform(size=kind.shape), 0.0)
    rh = rng.uniform(size=(nlay, ncol))
    lev, lims = lut["aero_rh"], lut["merra_aero_bin_lims"]
    rh.reshape(-1)[:len(lev)] = lev                               # exactly on every level
    rh.reshape(-1)[len(lev):len(lev) + 2] = (1.0, 0.995)
    size.reshape(-1)[:2 * nbin] = lims.reshape(-1)                # exactly on every bin limit
    mass.reshape(-1)[5] = 1e-300                                  # T and TS below eps
    kind[:, 2, 3], mass[:, 2, 3] = 3, 1e-300
    return lut, kind, size, mass, rh


@pytest.mark.parametrize("two_stream", [True, False])
@pytest.mark.parametrize("accumulate", [False, True])
def test_restatement_equals_the_scalar_loop_bit_for_bit(two_stream, accumulate):
    lut, kind, size, mass, rh = small_case()
    nspec, nlay, ncol = kind.shape
    nband = lut["aero_dust_tbl"].shape[0]
    op1 = None
    if accumulate:
        cl = synthetic.clouds(3, ncol, nlay, nband)
        op1 = (cl["tau"], cl["ssa"], cl["g"]) if two_stream else (cl["tau"],)
    got = ref.aerosol_optics(lut, kind, size, mass, rh, two_stream, np.float64, op1=op1)
    assert len(got) == (3 if two_stream else 1) and all(p.dtype == np.float64 and p.shape == (nband, nlay, ncol) for p in got)
    some_active = 0
    for b in range(nband):
        for l in range(nlay):
            for c in range(ncol):
                o1 = None if op1 is None else tuple(float(p[b, l, c]) for p in op1)
                exp = scalar_cell(lut, kind[:, l, c], [float(x) for x in size[:, l, c]], [float(x) for x in mass[:, l, c]],
                                  float(rh[l, c]), b, two_stream, o1)
                for p, e in zip(got, exp):
                    assert np.float64(p[b, l, c]).tobytes() == np.float64(e).tobytes(), (b, l, c, p[b, l, c], e)
                some_active += exp[0] > 0
    assert some_active > nband * nlay * ncol // 2


def test_restatement_single_species_is_the_two_dimensional_call():
    lut, kind, size, mass, rh = small_case(nspec=1)
    a = ref.aerosol_optics(lut, kind, size, mass, rh, True)
    b = ref.aerosol_optics(lut, kind[0], size[0], mass[0], rh, True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_inactive_cells_are_exact_zero(dtype):
    lut = synthetic.aerosol_lut(2, 3, 5)
    kind = np.array([[[0, 9, -1, 3, 3, 3, 1, 2, 1]]], dtype=np.int32)
    mass = np.array([[[1.0, 1.0, 1.0, 0.0, -1.0, np.nan, 1.0, 1.0, 1.0]]])
    size = np.array([[[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, np.nan, 10.0, 0.01]]])   # NaN, the last upper limit, below the bins
    rh = np.full((1, 9), np.nan)
    for two in (True, False):
        for p in ref.aerosol_optics(lut, kind, size, mass, rh, two, dtype):
            assert p.dtype == dtype and not p.view(np.uint64 if dtype is np.float64 else np.uint32).any()


def test_restatement_humidity_edges():
    lev = np.array([0.0, 0.5, 0.8, 0.9])
    i, w = ref.interval_and_weight(lev, np.array([-0.5, 0.0, 0.25, 0.5, 0.8, 0.85, 0.9, 0.95, 1.0, np.nan]))
    assert i.tolist() == [0, 0, 0, 1, 2, 2, 2, 2, 2, 0]
    assert w.tolist() == [0.0, 0.0, 0.5, 0.0, 0.0, (0.85 - 0.8) / (0.9 - 0.8), 1.0, 1.0, 1.0, 0.0]


def test_image_size_formula():
    # the 1-band longwave file with the real 36-level, 5-bin tables fits the LDS budget; 16 bands never do in fp64
    assert ref.image_bytes(1, 5, 36, True, False) == 3 * (180 + 105 + 2) * 16 <= 32768
    assert ref.image_bytes(16, 5, 36, True, False) == 220416 > 32768


# ---- the C ABI: construction, getters, refusals ----
@pytest.fixture(scope="module")
def L(pkg):
    return pkg.lib()


def create(L, lut=None, device=-1, **over):
    lut = synthetic.aerosol_lut(3, 4, 5) if lut is None else lut
    a = dict(nband=lut["aero_dust_tbl"].shape[0], nbin=lut["merra_aero_bin_lims"].shape[0], nrh=lut["aero_rh"].shape[0])
    tabs = {n: lut[n] for n in TABLE_NAMES}
    null_handle = over.pop("null_handle", False)
    for k, v in over.items():
        (tabs if k in tabs else a)[k] = v
    h = C.c_void_p(None)
    ptrs = [None if t is None else C.c_void_p(t.ctypes.data) for t in tabs.values()]
    rc = L.ecckd_aerosol_optics_create_lut(a["nband"], a["nbin"], a["nrh"], *ptrs, device, None if null_handle else C.byref(h))
    return rc, h, (L.ecckd_last_error().decode() if rc else "")


def test_create_lut_round_trips_the_getters(L):
    rc, h, msg = create(L, synthetic.aerosol_lut(7, 5, 36))
    assert rc == 0, msg
    try:
        assert L.ecckd_aerosol_optics_get_nband(h) == 7
        assert L.ecckd_aerosol_optics_get_nbin(h) == 5
        assert L.ecckd_aerosol_optics_get_nrh(h) == 36
    finally:
        L.ecckd_aerosol_optics_destroy(h)
    assert L.ecckd_aerosol_optics_get_nband(None) == 0 and L.ecckd_aerosol_optics_get_nrh(None) == 0
    L.ecckd_aerosol_optics_destroy(None)


def test_create_lut_refusals_in_the_stated_order(L):
    """Each case carries every later fault too, so the message shows which check came first."""
    lut = synthetic.aerosol_lut(3, 4, 5)
    bad_rh = lut["aero_rh"].copy()
    bad_rh[2] = bad_rh[1]
    nan_rh = lut["aero_rh"].copy()
    nan_rh[3] = np.nan
    empty_bin = lut["merra_aero_bin_lims"].copy()
    empty_bin[1, 1] = empty_bin[1, 0]
    overlap = lut["merra_aero_bin_lims"].copy()
    overlap[1, 1] = overlap[2, 0] * 1.01
    later = dict(aero_ocar_rh_tbl=None)
    cases = [
        (dict(null_handle=True, nband=0, nrh=1, aero_rh=bad_rh, merra_aero_bin_lims=empty_bin, **later), "null argument (the handle)"),
        (dict(nband=0, nrh=1, aero_rh=bad_rh, merra_aero_bin_lims=empty_bin, **later), "nband and nbin must be at least 1"),
        (dict(nbin=0, nrh=1, aero_rh=bad_rh, merra_aero_bin_lims=empty_bin, **later), "nband and nbin must be at least 1"),
        (dict(nrh=1, aero_rh=bad_rh, merra_aero_bin_lims=empty_bin, **later), "nrh must be at least 2"),
        (dict(aero_rh=bad_rh, merra_aero_bin_lims=empty_bin, **later), "not strictly increasing"),
        (dict(aero_rh=nan_rh, merra_aero_bin_lims=empty_bin, **later), "not strictly increasing"),
        (dict(aero_rh=None, merra_aero_bin_lims=empty_bin, **later), "rh_levels null"),
        (dict(merra_aero_bin_lims=empty_bin, **later), "a bin empty or reversed"),
        (dict(merra_aero_bin_lims=overlap, **later), "bins overlapping"),
        (dict(merra_aero_bin_lims=None, **later), "bin_lims null"),
    ] + [({n: None}, "null table") for n in TABLE_NAMES[2:]] + [
        (dict(device=12345), "device"),
    ]
    for over, needle in cases:
        over = dict(over)
        device = over.pop("device", -1)
        rc, h, msg = create(L, lut, device=device, **over)
        assert rc != 0 and needle in msg, (over.keys(), msg)
        assert not h.value
    # bins may touch (contiguous) or leave gaps
    gaps = lut["merra_aero_bin_lims"].copy()
    gaps[:, 1] *= 0.9
    rc, h, msg = create(L, lut, merra_aero_bin_lims=gaps)
    assert rc == 0, msg
    L.ecckd_aerosol_optics_destroy(h)


def compute(L, h, ncol=4, nlay=2, nspec=2, f32=False, memspace=HOST, accumulate=0, two=True, **over):
    dt = np.float32 if f32 else np.float64
    nband = max(1, L.ecckd_aerosol_optics_get_nband(h))
    n = max(1, ncol) * max(1, nlay)
    a = dict(aero_type=np.full(n * max(1, nspec), 3, np.int32), aero_size=np.full(n * max(1, nspec), 1.0, dt),
             aero_mass=np.full(n * max(1, nspec), 1e-5, dt), relhum=np.full(n, 0.5, dt), tau=np.zeros(n * nband, dt),
             ssa=np.zeros(n * nband, dt) if two else None, g=np.zeros(n * nband, dt) if two else None)
    a.update(over)
    p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
    f = L.ecckd_aerosol_optics_f32 if f32 else L.ecckd_aerosol_optics
    rc = f(h, ncol, nlay, nspec, p(a["aero_type"]), p(a["aero_size"]), p(a["aero_mass"]), p(a["relhum"]), accumulate,
           p(a["tau"]), p(a["ssa"]), p(a["g"]), memspace, None)
    return rc, (L.ecckd_last_error().decode() if rc else "")


@pytest.mark.parametrize("f32", [False, True])
def test_compute_refusals_in_the_stated_order(L, f32):
    """A host-only object: every refusal, the HOST value checks included, comes before "host-only object"."""
    lut = synthetic.aerosol_lut(3, 4, 5)
    rc, h, msg = create(L, lut)
    assert rc == 0, msg
    dt = np.float32 if f32 else np.float64
    n = 8
    kinds = np.full(2 * n, 3, np.int32)
    bad_type, bad_mass, bad_size, bad_rh = kinds.copy(), np.full(2 * n, 1e-5, dt), np.full(2 * n, 1.0, dt), np.full(n, 0.5, dt)
    bad_type[3] = 8
    bad_mass[4] = -1e-5
    kinds_salt = kinds.copy()
    kinds_salt[5] = 2
    bad_size[5] = 100.0
    bad_rh[6] = 1.5
    nan_rh = np.full(n, 0.5, dt)
    nan_rh[1] = np.nan
    try:
        steps = [
            (dict(nspec=0, g=None, ncol=-1, aero_mass=None, accumulate=2, memspace=7), "nspec must be at least 1"),
            (dict(g=None, ncol=-1, aero_mass=None, accumulate=2, memspace=7), "ssa without g or g without ssa"),
            (dict(ssa=None, ncol=-1, aero_mass=None, accumulate=2, memspace=7), "ssa without g or g without ssa"),
            (dict(ncol=-1, aero_mass=None, accumulate=2, memspace=7), "ncol"),
            (dict(aero_mass=None, accumulate=2, memspace=7), "null argument"),
            (dict(aero_type=None, accumulate=2, memspace=7), "null argument"),
            (dict(aero_size=None, accumulate=2, memspace=7), "null argument"),
            (dict(relhum=None, accumulate=2, memspace=7), "null argument"),
            (dict(tau=None, ssa=None, g=None, accumulate=2, memspace=7), "null argument"),
            (dict(accumulate=2, memspace=7), "accumulate must be 0 or 1"),
            (dict(accumulate=-1, memspace=7), "accumulate must be 0 or 1"),
            (dict(memspace=7, aero_type=bad_type), "bad memspace"),
            (dict(aero_type=bad_type, aero_mass=bad_mass, aero_size=bad_size, relhum=bad_rh), "type outside 0..7"),
            (dict(aero_type=kinds_salt, aero_mass=bad_mass, aero_size=bad_size, relhum=bad_rh), "negative aerosol mass"),
            (dict(aero_type=kinds_salt, aero_size=bad_size, relhum=bad_rh), "lies in no bin"),
            (dict(relhum=bad_rh), "relative humidity outside [0,1]"),
            (dict(relhum=nan_rh), "relative humidity outside [0,1]"),
            (dict(memspace=MIXED, relhum=bad_rh), "relative humidity outside [0,1]"),
            (dict(), "host-only object"),
            (dict(memspace=DEVICE, aero_type=bad_type, relhum=bad_rh), "host-only object"),   # device arrays: nothing is read
        ]
        for kw, needle in steps:
            rc, msg = compute(L, h, f32=f32, **kw)
            assert rc != 0 and needle in msg, (kw.keys(), msg)
        rc, msg = compute(L, None, nspec=0)
        assert rc != 0 and "null aerosol-optics object" in msg
        # what the value checks let through: none-cells with any size and humidity, an inactive salt cell off the bins,
        # humidity out of range where no active species depends on it
        ok_type = np.array([0, 1, 5, 7, 2, 3, 0, 0] * 2, np.int32)
        ok_mass = np.array([5.0, 1e-5, 1e-5, 1e-5, 0.0, 0.0, 0.0, 0.0] * 2, dt)
        ok_size = np.array([np.nan, 1.0, np.nan, -1.0, 500.0, 1.0, 1.0, 1.0] * 2, dt)
        ok_rh = np.array([np.nan, 2.0, -1.0, np.nan, 7.0, np.nan, 0.5, 0.5], dt)
        rc, msg = compute(L, h, f32=f32, aero_type=ok_type, aero_mass=ok_mass, aero_size=ok_size, relhum=ok_rh)
        assert rc != 0 and "host-only object" in msg, msg
    finally:
        L.ecckd_aerosol_optics_destroy(h)


# ---- the Python mirror ----
def load(pkg, lut, device=-1, **over):
    ao = pkg.AerosolOptics()
    a = dict(lut)
    a.update(over)
    return ao, ao.load(None, *[a[n] for n in TABLE_NAMES], device=device)


def test_python_mirror_getters_constants_and_messages(pkg):
    assert (pkg.AERO_NONE, pkg.AERO_DUST, pkg.AERO_SALT, pkg.AERO_SULF, pkg.AERO_BCAR_RH, pkg.AERO_BCAR, pkg.AERO_OCAR_RH,
            pkg.AERO_OCAR) == tuple(range(8))
    lut = synthetic.aerosol_lut(3, 4, 5)
    ao, msg = load(pkg, lut)
    assert msg == "" and (ao.get_nband(), ao.get_nbin(), ao.get_nrh()) == (3, 4, 5)
    op = pkg.OpticalProps2str()
    op.tau, op.ssa, op.g = (np.zeros((3, 2, 6)) for _ in range(3))
    kind = np.full((2, 2, 6), 3, np.int32)
    one = np.full((2, 2, 6), 1e-5)
    rh = np.full((2, 6), 0.5)
    assert "host-only object" in ao.aerosol_optics(kind, one, one, rh, op)
    assert "host-only object" in ao.aerosol_optics(kind[0], one[0], one[0], rh, op, accumulate=True)   # RTE's 2-D call
    assert "int32" in ao.aerosol_optics(kind.astype(np.int64), one, one, rh, op)
    assert "shape" in ao.aerosol_optics(kind, one[:1], one, rh, op)
    assert "float64" in ao.aerosol_optics(kind, one.astype(np.float32), one, rh, op)
    bad = one.copy()
    bad[1, 1, 1] = -1.0
    assert "negative aerosol mass" in ao.aerosol_optics(kind, one, bad, rh, op)
    op5 = pkg.OpticalProps1scl()
    op5.tau = np.zeros((5, 2, 6))
    assert "5 bands, the tables 3" in ao.aerosol_optics(kind, one, one, rh, op5)
    assert "not allocated" in ao.aerosol_optics(kind, one, one, rh, pkg.OpticalProps1scl())
    ao.finalize()
    assert ao.get_nband() == 0 and "have not been loaded" in ao.aerosol_optics(kind, one, one, rh, op)


def test_load_refuses_shapes_that_disagree(pkg):
    lut = synthetic.aerosol_lut(3, 4, 5)
    other = synthetic.aerosol_lut(2, 3, 6)
    for name in TABLE_NAMES:
        ao, msg = load(pkg, lut, **{name: other[name]})
        assert "sized inconsistently" in msg, (name, msg)
        assert ao.get_nband() == 0
    _, msg = load(pkg, lut, aero_sulf_tbl=lut["aero_sulf_tbl"].astype(np.float32))
    assert "float64" in msg
    _, msg = load(pkg, lut, aero_sulf_tbl=lut["aero_sulf_tbl"][:, :, :, None])
    assert "(nband, nrh, 3)" in msg
    ao = pkg.AerosolOptics()
    assert "sized inconsistently" in ao.load(np.zeros((4, 2)), *[lut[n] for n in TABLE_NAMES], device=-1)
    assert ao.load(np.zeros((3, 2)), *[lut[n] for n in TABLE_NAMES], device=-1) == ""


def test_symbols_are_exported(pkg):
    import __graft_entry__ as entry
    names = ["ecckd_aerosol_optics_create_lut", "ecckd_aerosol_optics_destroy", "ecckd_aerosol_optics_get_nband",
             "ecckd_aerosol_optics_get_nbin", "ecckd_aerosol_optics_get_nrh", "ecckd_aerosol_optics", "ecckd_aerosol_optics_f32"]
    declared = entry.exported_symbols()
    for n in names:
        assert n in declared and getattr(pkg.lib(), n) is not None


# ---- the synthetic tables and inputs ----
@pytest.mark.parametrize("nband,nbin,nrh", [(1, 1, 2), (5, 5, 36), (16, 3, 7)])
def test_aerosol_lut_properties(nband, nbin, nrh):
    lut = synthetic.aerosol_lut(nband, nbin, nrh)
    lims, rh = lut["merra_aero_bin_lims"], lut["aero_rh"]
    assert lims.shape == (nbin, 2) and rh.shape == (nrh,)
    assert (lims[:, 0] < lims[:, 1]).all() and np.array_equal(lims[1:, 0], lims[:-1, 1])          # contiguous bins
    assert lims[0, 0] == synthetic.AERO_SIZE_LWR and math.isclose(lims[-1, 1], synthetic.AERO_SIZE_UPR)
    assert (np.diff(rh) > 0).all() and rh[0] == 0.0 and rh[-1] <= 0.99 + 1e-15
    if nrh >= 6:   # coarse up to 0.8, fine above
        steps = np.diff(rh)
        assert steps[rh[:-1] < 0.8 - 1e-12].min() > 2 * steps[rh[:-1] >= 0.8 - 1e-12].max()
    assert lut["aero_dust_tbl"].shape == (nband, nbin, 3) and lut["aero_salt_tbl"].shape == (nband, nbin, nrh, 3)
    for n in ("aero_sulf_tbl", "aero_bcar_rh_tbl", "aero_ocar_rh_tbl"):
        assert lut[n].shape == (nband, nrh, 3) and (np.diff(lut[n], axis=1) > 0).all()            # strictly monotonic in RH
    assert (np.diff(lut["aero_salt_tbl"], axis=2) > 0).all()
    for n in ("aero_bcar_tbl", "aero_ocar_tbl"):
        assert lut[n].shape == (nband, 3)
    if nbin > 1:   # the bins differ in every quantity
        assert (np.diff(lut["aero_dust_tbl"], axis=1) != 0).all() and (np.diff(lut["aero_salt_tbl"], axis=1) != 0).all()
    # the types differ in every quantity at every band and level
    rows = [lut["aero_sulf_tbl"], lut["aero_bcar_rh_tbl"], lut["aero_ocar_rh_tbl"], lut["aero_salt_tbl"][:, 0],
            np.repeat(lut["aero_bcar_tbl"][:, None], nrh, 1), np.repeat(lut["aero_ocar_tbl"][:, None], nrh, 1),
            np.repeat(lut["aero_dust_tbl"][:, :1], nrh, 1)]
    for i in range(len(rows)):
        for j in range(i):
            assert (rows[i] != rows[j]).all()
    for n in TABLE_NAMES[2:]:
        t = lut[n]
        assert t.dtype == np.float64 and t.flags.c_contiguous and (t[..., 0] > 0).all()
        assert (t[..., 1] > 0).all() and (t[..., 1] < 1).all() and (t[..., 2] > 0).all() and (t[..., 2] < 1).all()


def test_aerosols_properties():
    ncol, nlay, nspec = 400, 30, 8
    kind, size, mass, rh = synthetic.aerosols(5, ncol, nlay, nspec)
    assert kind.dtype == np.int32 and kind.shape == size.shape == mass.shape == (nspec, nlay, ncol) and rh.shape == (nlay, ncol)
    assert all(a.flags.c_contiguous for a in (kind, size, mass, rh))
    assert set(np.unique(kind).tolist()) == set(range(8))                          # every type occurs
    assert (kind == 0).mean() >= 1.0 / 3.0                                          # at least a third hold none ...
    assert ((kind == 0).all(axis=0)).mean() >= 1.0 / 3.0                            # ... in every species at once
    assert ((kind > 0) == (mass > 0)).all() and (mass >= 0).all() and mass.max() <= 1e-4
    assert (rh >= 0).all() and (rh <= 1).all()
    lims = synthetic.aerosol_lut(1, 5, 2)["merra_aero_bin_lims"]
    active = kind > 0
    for b in range(5):                                                              # every bin occurs, in dust and in salt
        inside = (size >= lims[b, 0]) & (size < lims[b, 1])
        assert (inside & (kind == 1)).any() and (inside & (kind == 2)).any()
    assert ((size >= lims[0, 0]) & (size < lims[-1, 1])).all()
    for s in range(nspec):                                                          # plane s is mostly one type
        main = 1 + s % 7
        assert (kind[s][active[s]] == main).mean() > 0.8
    top, low = slice(0, nlay // 4), slice(2 * nlay // 3, nlay)
    assert (kind[0] == 1).any() and not (kind[0][low] == 1).all() and (kind[0][int(0.3 * nlay):int(0.7 * nlay)] > 0).any()
    assert not (kind[0][top] > 0).any() and not (kind[0][int(0.7 * nlay):] > 0).any()   # dust aloft only
    assert not (kind[1][:2 * nlay // 3] > 0).any() and not (kind[2][:2 * nlay // 3] > 0).any()   # salt, sulfate: lowest third
    dusty = (kind[0] > 0).any(axis=0)
    assert 0.2 < dusty.mean() < 0.6                                                 # dust in some columns only
    again = synthetic.aerosols(5 + 100, ncol - 100, nlay, nspec)                    # any column range regenerates the same
    assert np.array_equal(again[0], kind[:, :, 100:]) and np.array_equal(again[3], rh[:, 100:])
    one = synthetic.aerosols(5, ncol, nlay, 1)
    assert np.array_equal(one[0][0], kind[0]) and np.array_equal(one[2][0], mass[0])
