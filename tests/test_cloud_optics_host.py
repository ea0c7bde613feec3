"""Cloud optics without a GPU: the numpy restatement (tests/cloud_optics_ref.py) against hand-worked values, every refusal
of ``ecckd_cloud_optics_create_lut`` / ``ecckd_cloud_optics`` with its message and its place in the order the header
states (a host-only object, device -1, serves: every refusal comes before a device is asked for), the getters, the Python
mirror's own messages and the synthetic inputs."""
import ctypes as C

import numpy as np
import pytest

import cloud_optics_ref as ref
from rte_ecckd_amd import synthetic

HOST, DEVICE, MIXED = 0, 1, 2


# ---- the reference against hand-worked values: 2-entry tables, one band, one roughness ----
# liquid: radii [2, 6] (step 4), ext 0.5 -> 0.25, ssa 0.75 -> 0.5, asy 0.75 -> 0.875
# ice:    radii [10, 20] (step 10), ext 0.125 -> 0.0625, ssa 0.5 -> 0.25, asy 0.5 -> 1.0      (all exact in binary)
HAND = dict(radliq_lwr=2.0, radliq_upr=6.0, radice_lwr=10.0, radice_upr=20.0,
            lut_extliq=np.array([[0.5, 0.25]]), lut_ssaliq=np.array([[0.75, 0.5]]), lut_asyliq=np.array([[0.75, 0.875]]),
            lut_extice=np.array([[[0.125, 0.0625]]]), lut_ssaice=np.array([[[0.5, 0.25]]]), lut_asyice=np.array([[[0.5, 1.0]]]))


def one(lwp, iwp, rel, rei, lut=HAND, dtype=np.float64, **kw):
    a = lambda v: np.array([[v]], dtype=np.float64)
    out = ref.cloud_optics(a(lwp), a(iwp), a(rel), a(rei), lut, dtype=dtype, **kw)
    return tuple(float(x[0, 0, 0]) for x in out) if isinstance(out, tuple) else float(out[0, 0, 0])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_hand_values_liquid_only(dtype):
    # lower bound: s = 0, index 1, fint 0: t = 8*0.5 = 4, ts = 4*0.75 = 3, tsg = 3*0.75 = 2.25
    assert one(8.0, 0.0, 2.0, 15.0, dtype=dtype) == (4.0, 3.0 / 4.0, 2.25 / 3.0)
    # upper bound: s = 1, index = min(2, nsize-1) = 1, fint 1: t = 8*0.25 = 2, ts = 2*0.5 = 1, tsg = 0.875
    assert one(8.0, 0.0, 6.0, 15.0, dtype=dtype) == (2.0, 0.5, 0.875)
    # midway: fint 0.5: t = 8*0.375 = 3, ts = 3*0.625 = 1.875, tsg = 1.875*0.8125
    assert one(8.0, 0.0, 4.0, 15.0, dtype=dtype) == (3.0, 0.625, 0.8125)
    assert one(8.0, 0.0, 4.0, 15.0, dtype=dtype, two_stream=False) == 3.0 - 1.875


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_hand_values_interior_node(dtype):
    lut = dict(HAND, radliq_upr=10.0, lut_extliq=np.array([[0.5, 0.25, 0.125]]), lut_ssaliq=np.array([[0.75, 0.5, 0.25]]),
               lut_asyliq=np.array([[0.75, 0.875, 0.5]]))
    # re = 6 is the middle node: s = 1, index = min(2, 2) = 2, fint = 0: the node's own values
    assert one(8.0, 0.0, 6.0, 15.0, lut, dtype) == (2.0, 0.5, 0.875)
    # re = 10, the upper bound of a 3-entry table: s = 2, index = min(3, 2) = 2, fint = 1: the last entry
    assert one(8.0, 0.0, 10.0, 15.0, lut, dtype) == (1.0, 0.25, 0.5)
    # re = 7: index 2, fint 0.25: ext 0.25 - 0.25*0.125 = 0.21875, ssa 0.4375, asy 0.78125
    t = 8.0 * 0.21875
    assert one(8.0, 0.0, 7.0, 15.0, lut, dtype) == (t, 0.4375, 0.78125)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_hand_values_ice_only_and_both(dtype):
    # ice at 15: fint 0.5: t = 16*0.09375 = 1.5, ts = 1.5*0.375 = 0.5625, tsg = 0.5625*0.75 = 0.421875
    assert one(0.0, 16.0, 4.0, 15.0, dtype=dtype) == (1.5, 0.375, 0.75)
    assert one(0.0, 16.0, 4.0, 15.0, dtype=dtype, two_stream=False) == 1.5 - 0.5625
    # both: tau = 3 + 1.5, tssa = 1.875 + 0.5625 = 2.4375, tsg = 1.5234375 + 0.421875 = 1.9453125
    assert one(8.0, 16.0, 4.0, 15.0, dtype=dtype) == (4.5, dtype(2.4375) / dtype(4.5), dtype(1.9453125) / dtype(2.4375))
    assert one(8.0, 16.0, 4.0, 15.0, dtype=dtype, two_stream=False) == (3.0 - 1.875) + (1.5 - 0.5625)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("lwp,iwp", [(0.0, 0.0), (-1.0, 0.0), (np.nan, np.nan), (0.0, -0.0)])
def test_reference_clear_cell_with_nan_radius_is_exact_zero(dtype, lwp, iwp):
    out = ref.cloud_optics(np.array([[lwp]]), np.array([[iwp]]), np.array([[np.nan]]), np.array([[np.inf]]), HAND, dtype=dtype)
    for plane in out:   # tau, ssa, g: +0, bit for bit
        assert plane.dtype == dtype and plane.tobytes() == np.zeros((1, 1, 1), dtype).tobytes()
    tau = ref.cloud_optics(np.array([[lwp]]), np.array([[iwp]]), np.array([[np.nan]]), np.array([[-5.0]]), HAND, dtype=dtype,
                           two_stream=False)
    assert tau.tobytes() == np.zeros((1, 1, 1), dtype).tobytes()


def test_reference_clamps_and_tiny_paths():
    # below the table: index stays 1, fint = -0.25 (extrapolates); a NaN radius in a CLOUDY cell gives NaN, no exception
    assert one(8.0, 0.0, 1.0, 15.0)[0] == 8.0 * (0.5 + -0.25 * -0.25)
    assert np.isnan(one(8.0, 0.0, np.nan, 15.0)[0])
    # a path so thin that max(eps, .) is taken: ssa = tssa/eps, g = tsg/eps
    tau, ssa, g = one(1e-300, 0.0, 2.0, 15.0)
    eps = np.finfo(np.float64).eps
    assert tau == 1e-300 * 0.5 and ssa == (tau * 0.75) / eps and g == (tau * 0.75 * 0.75) / eps


# ---- the C ABI: construction, getters, refusals ----
@pytest.fixture(scope="module")
def L(pkg):
    return pkg.lib()


def tables(nband=3, nsl=4, nsi=5, nrgh=2):
    return synthetic.cloud_lut(nband, nsl, nsi, nrgh)


def create(L, lut=None, device=-1, **over):
    lut = tables() if lut is None else lut
    nband, nsl = lut["lut_extliq"].shape
    nrgh, _, nsi = lut["lut_extice"].shape
    a = dict(nband=nband, nsize_liq=nsl, nsize_ice=nsi, nrghice=nrgh, radliq_lwr=lut["radliq_lwr"], radliq_upr=lut["radliq_upr"],
             radice_lwr=lut["radice_lwr"], radice_upr=lut["radice_upr"])
    tabs = {n: lut[n] for n in ("lut_extliq", "lut_ssaliq", "lut_asyliq", "lut_extice", "lut_ssaice", "lut_asyice")}
    null_handle = over.pop("null_handle", False)
    for k, v in over.items():
        (tabs if k in tabs else a)[k] = v
    h = C.c_void_p(None)
    ptrs = [None if t is None else C.c_void_p(t.ctypes.data) for t in tabs.values()]
    rc = L.ecckd_cloud_optics_create_lut(a["nband"], a["nsize_liq"], a["nsize_ice"], a["nrghice"], a["radliq_lwr"], a["radliq_upr"],
                                         a["radice_lwr"], a["radice_upr"], *ptrs, device, None if null_handle else C.byref(h))
    return rc, h, (L.ecckd_last_error().decode() if rc else "")


def test_create_lut_round_trips_the_getters(L):
    lut = tables(nband=7, nsl=4, nsi=9, nrgh=3)
    rc, h, msg = create(L, lut)
    assert rc == 0, msg
    try:
        assert L.ecckd_cloud_optics_get_nband(h) == 7
        assert L.ecckd_cloud_optics_get_nrghice(h) == 3
        assert L.ecckd_cloud_optics_get_min_radius_liq(h) == lut["radliq_lwr"]
        assert L.ecckd_cloud_optics_get_max_radius_liq(h) == lut["radliq_upr"]
        assert L.ecckd_cloud_optics_get_min_radius_ice(h) == lut["radice_lwr"]
        assert L.ecckd_cloud_optics_get_max_radius_ice(h) == lut["radice_upr"]
    finally:
        L.ecckd_cloud_optics_destroy(h)
    L.ecckd_cloud_optics_destroy(None)   # (harmless)


# each entry breaks one argument; an entry also carries every LATER entry's fault, so its message shows its place in the order
CREATE_REFUSALS = [
    (dict(null_handle=True), "null argument (the handle)"),
    (dict(nband=0), "nband must be at least 1"),
    (dict(nsize_liq=1), "a table needs at least 2 sizes"),
    (dict(nsize_ice=1), "a table needs at least 2 sizes"),
    (dict(nrghice=0), "nrghice must be at least 1"),
    (dict(radliq_upr=2.5), "radliq_upr must exceed radliq_lwr"),
    (dict(radice_upr=float("nan")), "radice_upr must exceed radice_lwr"),
    (dict(lut_asyice=None), "null table"),
]


@pytest.mark.parametrize("i", range(len(CREATE_REFUSALS)))
def test_create_lut_refusals_in_order(L, i):
    over = {}
    for o, _ in CREATE_REFUSALS[i:]:
        over.update(o)
    rc, h, msg = create(L, **over)
    assert rc != 0 and not h
    assert msg.startswith("ecckd_cloud_optics_create_lut: ") and CREATE_REFUSALS[i][1] in msg, msg


FAULT_CELL = dict(reliq=0, reice=1, clwp=2, ciwp=3)


def call(L, h, ncol=2, nlay=2, nband=3, icergh=1, memspace=HOST, f32=False, null=(), two=True, cell=None, **cells):
    """One ecckd_cloud_optics call on host arrays; cells: a clwp / ciwp / reliq / reice value for that array's FAULT_CELL, or all for `cell`."""
    dt = np.float32 if f32 else np.float64
    arr = dict(clwp=np.full((nlay, ncol), 50.0, dt), ciwp=np.full((nlay, ncol), 20.0, dt), reliq=np.full((nlay, ncol), 10.0, dt),
               reice=np.full((nlay, ncol), 60.0, dt)) if ncol > 0 and nlay > 0 else {n: np.zeros((2, 2), dt) for n in ("clwp", "ciwp", "reliq", "reice")}
    for n, v in cells.items():   # (each array's fault in a cell of its own, so that one does not hide another)
        arr[n].flat[FAULT_CELL[n] if cell is None else cell] = v
    out = {n: np.zeros((nband, max(nlay, 1), max(ncol, 1)), dt) for n in ("tau", "ssa", "g")}
    if not two:
        out["ssa"] = out["g"] = None
    P = lambda n, a: None if (a is None or n in null) else C.c_void_p(a.ctypes.data)
    f = L.ecckd_cloud_optics_f32 if f32 else L.ecckd_cloud_optics
    rc = f(h, ncol, nlay, *[P(n, arr[n]) for n in ("clwp", "ciwp", "reliq", "reice")], icergh,
           *[P(n, out[n]) for n in ("tau", "ssa", "g")], memspace, None)
    return rc, (L.ecckd_last_error().decode() if rc else "")


# as CREATE_REFUSALS: in the header's order; each case also carries the faults of every later one
CALL_REFUSALS = [
    (dict(icergh=3), "ice roughness 3 outside 1..2"),
    (dict(null=("g",)), "ssa without g or g without ssa"),
    (dict(nlay=0), "bad ncol/nlay"),
    (dict(null=("reice",)), "null argument (clwp, ciwp, reliq, reice and tau are required)"),
    (dict(memspace=7), "bad memspace"),
    (dict(reliq=21.6), "liquid effective radius out of the table's range in a cloudy cell"),
    (dict(reice=float("nan")), "ice effective radius out of the table's range in a cloudy cell"),
    (dict(clwp=-1.0), "negative liquid water path"),
    (dict(ciwp=-1e-3), "negative ice water path"),
    (dict(), "host-only object (device -1)"),
]


@pytest.fixture(scope="module")
def host_only(L):
    rc, h, msg = create(L)
    assert rc == 0, msg
    yield h
    L.ecckd_cloud_optics_destroy(h)


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("i", range(len(CALL_REFUSALS)))
def test_call_refusals_in_order(L, host_only, i, f32):
    kw = {}
    for o, _ in CALL_REFUSALS[i:]:
        for k, v in o.items():
            kw[k] = tuple(kw.get(k, ())) + tuple(v) if k == "null" else v
    rc, msg = call(L, host_only, f32=f32, **kw)
    assert rc != 0 and CALL_REFUSALS[i][1] in msg, msg


def test_call_refusals_null_object_and_alone(L, host_only):
    rc, msg = call(L, None)
    assert rc != 0 and "null cloud-optics object" in msg
    for o, text in CALL_REFUSALS:   # each fault alone
        rc, msg = call(L, host_only, **o)
        assert rc != 0 and text in msg, msg
    rc, msg = call(L, host_only, null=("ssa",))
    assert rc != 0 and "ssa without g or g without ssa" in msg
    rc, msg = call(L, host_only, ncol=-1)
    assert rc != 0 and "bad ncol/nlay" in msg


def test_host_value_checks_look_at_cloudy_cells_only(L, host_only):
    """A clear cell may hold any radius; both bounds themselves are inside; MIXED checks its host inputs too."""
    for kw in (dict(clwp=0.0, reliq=float("nan")), dict(ciwp=0.0, reice=1e9), dict(clwp=float("nan"), reliq=-3.0),
               dict(reliq=synthetic.RADLIQ_LWR), dict(reliq=synthetic.RADLIQ_UPR), dict(reice=synthetic.RADICE_UPR)):
        for f32 in (False, True):
            rc, msg = call(L, host_only, f32=f32, cell=1, **kw)
            assert rc != 0 and "host-only object" in msg, (kw, msg)   # (past every value check)
    rc, msg = call(L, host_only, memspace=MIXED, reliq=1.0)
    assert rc != 0 and "liquid effective radius" in msg
    rc, msg = call(L, host_only, two=False)
    assert rc != 0 and "host-only object" in msg


# ---- the Python mirror and the synthetic inputs ----
def test_mirror_load_getters_and_messages(pkg):
    lut = tables()
    co = pkg.CloudOptics()
    assert co.get_num_ice_roughness_types() == 0
    assert "before initialization" in co.set_ice_roughness(1)
    args = lambda d: (None, d["radliq_lwr"], d["radliq_upr"], 1.0, d["radice_lwr"], d["radice_upr"], 1.0, d["lut_extliq"],
                      d["lut_ssaliq"], d["lut_asyliq"], d["lut_extice"], d["lut_ssaice"], d["lut_asyice"])
    assert co.load_lut(*args(lut), device=-1) == ""
    assert (co.get_nband(), co.get_num_ice_roughness_types()) == (3, 2)
    assert (co.get_min_radius_liq(), co.get_max_radius_liq(), co.get_min_radius_ice(), co.get_max_radius_ice()) == \
        (lut["radliq_lwr"], lut["radliq_upr"], lut["radice_lwr"], lut["radice_upr"])
    assert co.set_ice_roughness(2) == "" and "nrghice" in co.set_ice_roughness(3)
    assert "sized inconsistently" in co.load_lut(*args(dict(lut, lut_ssaliq=lut["lut_ssaliq"][:, :-1].copy())), device=-1)
    assert "radliq_upr must exceed" in co.load_lut(*args(dict(lut, radliq_upr=0.0)), device=-1)
    assert co.load_lut(*args(lut), device=-1) == ""

    class Desc:
        def get_band2gpt(self):
            return np.array([[1, 1], [2, 2], [3, 3]], dtype=np.int32)

        def get_nband(self):
            return 3

    clwp, ciwp, reliq, reice = synthetic.cloud_water(0, 8, 6)
    op = pkg.OpticalProps2str()
    op.alloc_2str_bands(8, 6, Desc())
    assert "host-only object" in co.cloud_optics(clwp, ciwp, reliq, reice, op)
    assert "expected (6, 8)" in co.cloud_optics(clwp[:-1], ciwp, reliq, reice, op)
    assert "float64" in co.cloud_optics(clwp.astype(np.float32), ciwp, reliq, reice, op)
    op1 = pkg.OpticalProps1scl()
    op1.tau = np.zeros((4, 6, 8))
    assert "4 bands" in co.cloud_optics(clwp, ciwp, reliq, reice, op1)
    co.finalize()
    assert "not been loaded" in co.cloud_optics(clwp, ciwp, reliq, reice, op)


def test_synthetic_cloud_water_and_lut():
    ncol, nlay = 200, 60
    clwp, ciwp, reliq, reice = synthetic.cloud_water(3, ncol, nlay)
    has = synthetic.clouds(3, ncol, nlay, 1)["tau"][0] > 0
    assert all(a.shape == (nlay, ncol) and a.dtype == np.float64 for a in (clwp, ciwp, reliq, reice))
    assert np.array_equal((clwp > 0) | (ciwp > 0), has)             # water exactly where clouds is cloudy
    assert ((clwp > 0) & (ciwp > 0)).any() and ((clwp > 0) & (ciwp == 0)).any() and ((clwp == 0) & (ciwp > 0)).any()
    assert clwp.min() == 0 and ciwp.min() == 0 and clwp.max() <= 200 and ciwp.max() <= 50
    assert reliq.min() >= synthetic.RADLIQ_LWR and reliq.max() <= synthetic.RADLIQ_UPR
    assert reice.min() >= synthetic.RADICE_LWR and reice.max() <= synthetic.RADICE_UPR
    again = synthetic.cloud_water(3 + 50, 20, nlay)                # a column range regenerates the same columns
    assert np.array_equal(again[0], clwp[:, 50:70]) and np.array_equal(again[3], reice[:, 50:70])
    for nband, nsl, nsi, nrgh in ((1, 2, 2, 1), (16, 20, 18, 3)):
        lut = synthetic.cloud_lut(nband, nsl, nsi, nrgh)
        assert lut["lut_extliq"].shape == (nband, nsl) and lut["lut_asyice"].shape == (nrgh, nband, nsi)
        for ph in ("liq", "ice"):
            ext, ssa, asy = (lut["lut_%s%s" % (q, ph)] for q in ("ext", "ssa", "asy"))
            assert (np.diff(ext, axis=-1) < 0).all() and (ext > 0).all()
            assert (ssa > 0.5).all() and (ssa < 1).all() and (np.diff(ssa, axis=-1) != 0).all()
            assert (asy > 0.7).all() and (asy < 0.95).all() and (np.diff(asy, axis=-1) != 0).all()
        if nrgh > 1:
            assert (lut["lut_asyice"][0] != lut["lut_asyice"][-1]).all()
