"""Heating rates without a GPU: the header's block and the exported entry points, every refusal of ``ecckd_heating_rate``
with its message and its place in the order the header states (reached through the raw ctypes call: every refusal comes
before a device is used), the Python mirror's own refusals, the numpy restatement (tests/heating_rate_ref.py) against
closed forms, and the Fortran sources."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import heating_rate_ref as ref

HOST, DEVICE, MIXED = 0, 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L(pkg):
    return pkg.lib()


# ---- the header and the library ----
def test_header_declares_and_defines():
    text = open(os.path.join(ROOT, "include", "ecckd_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+ecckd_heating_rate\s*\(\s*int device, int ncol, int nlay, int nouter, const double \*flux_up", code)
    assert re.search(r"\bint\s+ecckd_heating_rate_f32\s*\(\s*int device, int ncol, int nlay, int nouter, const float \*flux_up", code)
    for line in ("du   = flux_up[l+1] - flux_up[l]", "dd   = flux_dn[l+1] - flux_dn[l]", "dnet = du - dd",
                 "dp   = plev[l+1] - plev[l]", "c    = cp ? cp[l] : cp_dry", "heating_rate[l] = (dnet * grav) / (c * dp)"):
        assert line in text, line
    block = text[text.index("Heating rates:"):text.index("int ecckd_heating_rate(")]
    for word in ("PARITY WITH IT IS\n * UNPINNED", "no top_at_1", "must not alias", "9.80665", "1004.64", "capture-safe"):
        assert word in block, word
    # after the aerosol optics
    assert text.index("int ecckd_aerosol_optics_f32(") < text.index("int ecckd_heating_rate(")


def test_library_exports_both_entry_points(L):
    for f in ("ecckd_heating_rate", "ecckd_heating_rate_f32"):
        assert getattr(L, f).argtypes is not None and len(getattr(L, f).argtypes) == 13


# ---- the refusals, in the header's order ----
def call(L, ncol=3, nlay=2, nouter=2, f32=False, null=(), grav=9.80665, cp_dry=1004.64, with_cp=False, memspace=HOST, device=999):
    """One raw call on host arrays.  The default device ordinal does not exist, so a call that is not refused earlier ends
    at the device check (no GPU: "no HIP device"; with GPUs: "bad device ordinal") and never launches."""
    dt = np.float32 if f32 else np.float64
    n = lambda *s: np.ones(tuple(max(x, 1) for x in s), dt)
    arr = dict(flux_up=n(nouter, nlay + 1, ncol), flux_dn=n(nouter, nlay + 1, ncol), plev=n(nlay + 1, ncol),
               cp=n(nlay, ncol) if with_cp else None, heating_rate=n(nouter, nlay, ncol))
    P = lambda k: None if (arr[k] is None or k in null) else C.c_void_p(arr[k].ctypes.data)
    f = L.ecckd_heating_rate_f32 if f32 else L.ecckd_heating_rate
    rc = f(device, ncol, nlay, nouter, P("flux_up"), P("flux_dn"), P("plev"), grav, cp_dry, P("cp"), P("heating_rate"), memspace, None)
    return rc, (L.ecckd_last_error().decode() if rc else "")


# each case also carries the faults of every later one, so its message shows its place in the order
REFUSALS = [
    (dict(nouter=0), "ncol, nlay and nouter must be at least 1"),
    (dict(null=("plev",)), "null argument (flux_up, flux_dn, plev and heating_rate are required)"),
    (dict(grav=float("inf")), "grav must be finite and positive"),
    (dict(cp_dry=0.0), "cp_dry must be finite and positive"),
    (dict(memspace=7), "bad memspace"),
    (dict(), "device"),
]


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_refusals_in_order(L, i, f32):
    kw = {}
    for o, _ in REFUSALS[i:]:
        kw.update(o)
    rc, msg = call(L, f32=f32, **kw)
    assert rc != 0 and REFUSALS[i][1] in msg, msg
    if i < 4:
        assert msg.startswith("ecckd_heating_rate: "), msg


def test_refusals_alone_and_variants(L):
    for o, text in REFUSALS:
        rc, msg = call(L, **o)
        assert rc != 0 and text in msg, msg
    for o in (dict(ncol=0), dict(nlay=0), dict(ncol=-4), dict(nouter=-1)):
        assert "must be at least 1" in call(L, **o)[1]
    for name in ("flux_up", "flux_dn", "plev", "heating_rate"):
        assert "null argument" in call(L, null=(name,))[1]
    for g in (0.0, -9.8, float("nan"), float("-inf")):
        assert "grav must be finite and positive" in call(L, grav=g)[1]
    for c in (-1.0, float("nan"), float("inf")):
        assert "cp_dry must be finite and positive" in call(L, cp_dry=c)[1]
        # with cp per cell cp_dry is not looked at: the call goes on to the device check
        rc, msg = call(L, cp_dry=c, with_cp=True)
        assert rc != 0 and "device" in msg and "cp_dry" not in msg, msg
    for space in (DEVICE, MIXED):
        rc, msg = call(L, memspace=space)
        assert rc != 0 and "device" in msg and "memspace" not in msg, msg


# ---- the Python mirror ----
def test_mirror_refuses_mixed_precisions_and_wrong_shapes(pkg):
    fu, fd, plev, cp = ref.inputs(0, 5, 4, None, np.float64, True)
    f32 = lambda a: a.astype(np.float32)
    err, out = pkg.heating_rate(fu, f32(fd), plev)
    assert "mixing float32 and float64" in err and "flux_dn" in err and out is None
    assert "mixing float32 and float64" in pkg.heating_rate(fu, fd, plev, cp=f32(cp))[0]
    assert "mixing float32 and float64" in pkg.heating_rate(fu, fd, plev, heating_rate=np.zeros((4, 5), np.float32))[0]
    assert "mixing float32 and float64" in pkg.heating_rate(f32(fu), f32(fd), plev)[0]
    assert "flux_dn: shape (4, 5), expected (5, 5)" in pkg.heating_rate(fu, fd[:-1].copy(), plev)[0]
    assert "plev: shape" in pkg.heating_rate(fu, fd, plev[:, :-1].copy())[0]
    assert "cp: shape (5, 5), expected (4, 5)" in pkg.heating_rate(fu, fd, plev, cp=plev)[0]
    assert "heating_rate: shape" in pkg.heating_rate(fu, fd, plev, heating_rate=np.zeros((5, 5)))[0]
    assert "plev: shape" in pkg.heating_rate(np.stack([fu, fu]), np.stack([fd, fd]), np.stack([plev, plev]))[0]
    assert "heating_rate: shape (4, 5), expected (2, 4, 5)" in pkg.heating_rate(np.stack([fu, fu]), np.stack([fd, fd]), plev,
                                                                                heating_rate=np.zeros((4, 5)))[0]
    assert "must be (nlay+1, ncol) or (nouter, nlay+1, ncol)" in pkg.heating_rate(fu[0], fd[0], plev[0])[0]
    assert "at least two levels" in pkg.heating_rate(fu[:1], fd[:1], plev[:1])[0]
    assert "contiguous" in pkg.heating_rate(fu[:, ::2], fd[:, ::2], plev[:, ::2])[0]
    # a well-formed call reaches the library: its message, not the mirror's (a nonexistent device: nothing is launched)
    err, out = pkg.heating_rate(fu, fd, plev, cp=cp, device=999)
    assert "device" in err and out.shape == (4, 5) and out.dtype == np.float64
    err, out = pkg.heating_rate(f32(fu), f32(fd), f32(plev), grav=-1.0, device=999)
    assert "grav must be finite and positive" in err and out.dtype == np.float32
    assert (pkg.GRAV, pkg.CP_DRY) == (9.80665, 1004.64) == (ref.GRAV, ref.CP_DRY)


def test_mirror_class_conveniences_forward(pkg):
    fu, fd, plev, _ = ref.inputs(1, 5, 4, 3, np.float64, False)
    fl = pkg.FluxesByband(fu, fd, flux_up=fu[0], flux_dn=fd[0])
    assert "grav must be finite" in fl.heating_rate(plev, grav=0.0)[0]
    err, out = fl.heating_rate(plev, device=999)
    assert "device" in err and out.shape == (4, 5)
    err, out = fl.bnd_heating_rate(plev, device=999)
    assert "device" in err and out.shape == (3, 4, 5)
    assert "grav must be finite" in pkg.FluxesBroadband(fu[0], fd[0]).heating_rate(plev, grav=0.0)[0]


# ---- the restatement against closed forms ----
def ulp_distance(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    i = np.int64 if a.dtype == np.float64 else np.int32
    return np.abs(a.view(i).astype(np.int64) - b.view(i).astype(np.int64))   # (same sign, finite: the distance in ulp)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_linear_net_flux_gives_uniform_heating(dtype):
    """net = flux_up - flux_dn linear in pressure with slope s: every layer heats at s*grav/cp_dry.  Numbers chosen exact in
    both precisions (powers of two and small integers), so only the final multiply and divide round: a few ulp."""
    nlay, ncol = 12, 3
    slope = 2.0 ** -8   # W m-2 Pa-1
    plev = (1024.0 * np.arange(1, nlay + 2, dtype=np.float64)[:, None] * np.ones((1, ncol))).astype(dtype)
    fd = (3.0 * np.ones((nlay + 1, ncol))).astype(dtype)
    fu = (fd + slope * plev).astype(dtype)
    out = ref.heating_rate(fu, fd, plev)
    assert out.dtype == dtype and out.shape == (nlay, ncol)
    want = np.full(out.shape, np.float64(slope) * ref.GRAV / ref.CP_DRY).astype(dtype)
    assert ulp_distance(out, want).max() <= 3
    assert (out == out[0, 0]).all()   # the same bits in every layer


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("with_cp", [False, True])
def test_reference_reversal_is_bit_for_bit(dtype, with_cp):
    fu, fd, plev, cp = ref.inputs(2, 7, 9, 3, dtype, with_cp)
    a = ref.heating_rate(fu, fd, plev, cp)
    b = ref.heating_rate(fu[:, ::-1], fd[:, ::-1], plev[::-1], None if cp is None else cp[::-1])
    assert np.array_equal(ref.bits(a), ref.bits(b[:, ::-1]))
    assert np.isfinite(a).all() and (a != 0).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_cp_filled_with_cp_dry_gives_the_scalar_bits(dtype):
    fu, fd, plev, _ = ref.inputs(3, 7, 9, None, dtype, False)
    cp = np.full((9, 7), ref.CP_DRY, dtype=dtype)
    assert np.array_equal(ref.bits(ref.heating_rate(fu, fd, plev, cp)), ref.bits(ref.heating_rate(fu, fd, plev)))
    assert not np.array_equal(ref.heating_rate(fu, fd, plev, cp * dtype(1.03)), ref.heating_rate(fu, fd, plev))


def test_reference_float32_has_no_float64_intermediates():
    """Operands whose float64 evaluation, rounded once at the end, differs from the float32 chain."""
    fu, fd, plev, cp = ref.inputs(4, 64, 30, 2, np.float32, True)
    f32 = ref.heating_rate(fu, fd, plev, cp)
    f64 = ref.heating_rate(fu.astype(np.float64), fd.astype(np.float64), plev.astype(np.float64), cp.astype(np.float64),
                           grav=float(np.float32(ref.GRAV)))
    assert f32.dtype == np.float32 and (f32 != f64.astype(np.float32)).any()


def test_reference_zero_thickness_and_nan_stay_in_their_cell():
    fu, fd, plev, _ = ref.inputs(5, 6, 8, None, np.float64, False)
    clean = ref.heating_rate(fu, fd, plev)
    plev[4, 2] = plev[3, 2]      # dp = 0 in layer 3 of column 2 (layer 4 grows)
    fu[6, 1] = np.nan            # a NaN level: layers 5 and 6 of column 1
    out = ref.heating_rate(fu, fd, plev)
    assert np.isinf(out[3, 2]) and np.isnan(out[5, 1]) and np.isnan(out[6, 1])
    touched = np.zeros(out.shape, bool)
    touched[3:5, 2] = touched[5:7, 1] = True
    assert np.array_equal(ref.bits(out)[~touched], ref.bits(clean)[~touched]) and np.isfinite(out[~touched]).all()


# ---- Fortran ----
def test_fortran_heating_sources_compile(pkg):
    """The module and the program build with amdflang against the C ABI library (skipped without it); the program prints
    its usage."""
    if pkg.build_fortran() is None:
        pytest.skip("no amdflang in this image")
    assert os.path.exists(pkg.HEATING_DRIVER)   # (it uses the module: linked, so both compiled)
    out = subprocess.run([pkg.HEATING_DRIVER], capture_output=True, text=True)
    assert out.returncode != 0 and "usage: ecckd_heating_driver" in out.stderr
