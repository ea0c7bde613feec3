"""Writes tests/golden/fused_call_marshalling.json: what the Python mirror hands to every fused flux entry point
(``ecckd_*_fluxes*``) of the C ABI, and what it answers when it refuses a call, recorded without a GPU.

    python tests/golden/make_golden_fused_calls.py

The recording.  Host-only models are loaded (``load(..., device=-1)``) and ``pkg._lib`` is replaced by a proxy that
forwards every attribute to the real library, except a name that contains ``_fluxes`` and does not end in ``_bytes``:
for such a name the proxy notes ``(name, args)`` and returns 0.  One case is one line of the file: ``[id, "called", entry
point, arguments]``, or for a call that is refused ``[id, "returned", message]`` / ``[id, "raised", class name, text]``
(and then the proxy has noted nothing).  Each argument is written down as what it means:

  int                 the int                      None / a null pointer      null
  the gas names       "names:h2o,o3"               an array of numbers        [values]
  the model handle    "handle"                     the gas pointer array      "ptrs:10" (1: not null)
  a data pointer      the name of the array of the case it points into ("+bytes" where it points past its start)

A pointer that lies in no array of the case stops the recording (and fails the replaying test).

The cases.  ``(nlay, ncol) = (3, 2)``, numpy arrays (default allocation, nothing padded).  A *route* is a public method
with the keywords that pick its entry point (``ROUTES``).  Per route: the call without any optional argument and with all of them, in float64 and
in float32 -- a float64-only route refuses that -- and in float64 with each option that takes something away (no tlev, no
flux_dn_dir, one-stream particles, an empty column list).
Per method, on its widest route (``WRONG_ARRAYS``), float64, the call with every optional argument and: a gas the model
does not know (it goes through), a gas never set, then each array in turn with a wrong shape; an input, an output, the
mask, the gas array and the column list also with a wrong dtype, as a non-contiguous view, in the other precision
(``MUTATIONS``).  ``lw_fluxes`` and ``sw_fluxes`` get every way to pass a gas (``GASES``).  ``REFUSALS`` lists the
Python-level refusals (rescaled / use_2stream / FluxesByband / one-stream particles / a keyword that needs float64) by
hand.  ``sw_fluxes_daylit`` always gets its ``day_index``: selecting the columns is a call into the real library and
belongs to the GPU tests.

The file also holds ``git rev-parse HEAD`` of the tree that generated it ("recorded_at").  The point of the fixture is
to pin the mirror's behaviour ACROSS a change of ``rte-ecckd_amd/__init__.py``: generate it before such a change,
replay it (tests/test_fused_call_marshalling_host.py) after, and regenerate only where a change of behaviour is meant.
"""
import ctypes as C
import inspect
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PATH = os.path.join(HERE, "fused_call_marshalling.json")
DATA = os.path.join(ROOT, "data")
LW_FSCK = os.path.join(DATA, "ecckd-1.2_lw_ckd-definition_climate_fsck-tol0.0161.nc")   # (tests/conftest.py)
SW_WIDE = os.path.join(DATA, "ecckd-1.2_sw_ckd-definition_climate_wide-tol0.05.nc")
NLAY, NCOL = 3, 2
F64, F32 = "float64", "float32"

# route: (method, keywords that pick the entry point, optional arguments, serves float32)
ROUTES = {
    "lw_fluxes": ("lw_fluxes", {}, ("inc_flux", "no_tlev", "n_gauss_angles"), True),
    "lw_fluxes+jac": ("lw_fluxes", {"flux_up_jac": True}, ("inc_flux", "n_gauss_angles"), False),
    "lw_fluxes_allsky": ("lw_fluxes_allsky", {}, ("inc_flux", "cloud_mask", "n_gauss_angles", "one_stream"), True),
    "lw_fluxes_allsky+jac": ("lw_fluxes_allsky", {"flux_up_jac": True}, ("inc_flux", "cloud_mask", "one_stream"), False),
    "lw_fluxes_allsky+2stream": ("lw_fluxes_allsky", {"use_2stream": True}, ("inc_flux", "cloud_mask"), False),
    "lw_fluxes_allsky+rescaled": ("lw_fluxes_allsky", {"rescaled": True}, ("inc_flux", "cloud_mask", "n_gauss_angles"), False),
    "lw_fluxes_rescaled": ("lw_fluxes_rescaled", {}, ("inc_flux", "cloud_mask", "fluxes_clear", "flux_up_jac", "n_gauss_angles"),
                           False),
    "lw_fluxes_clear_allsky": ("lw_fluxes_clear_allsky", {}, ("inc_flux", "cloud_mask", "n_gauss_angles", "one_stream"), True),
    "lw_fluxes_clear_allsky_jac": ("lw_fluxes_clear_allsky_jac", {"flux_up_jac": True}, ("inc_flux", "cloud_mask", "one_stream"),
                                   False),
    "sw_fluxes": ("sw_fluxes", {}, ("toa_scale", "no_dn_dir"), True),
    "sw_fluxes_allsky": ("sw_fluxes_allsky", {}, ("toa_scale", "cloud_mask", "delta_scale_off", "no_dn_dir"), True),
    "sw_fluxes_clear_allsky": ("sw_fluxes_clear_allsky", {}, ("toa_scale", "cloud_mask", "delta_scale_off", "no_dn_dir",
                                                             "no_dn_dir_clear"), True),
    "sw_fluxes_daylit": ("sw_fluxes_daylit", {"day_index": True}, ("toa_scale",), False),
    "sw_fluxes_daylit+particles": ("sw_fluxes_daylit", {"day_index": True, "particles": True},
                                   ("toa_scale", "cloud_mask", "delta_scale_off", "one_stream"), False),
    "sw_fluxes_daylit+both": ("sw_fluxes_daylit", {"day_index": True, "particles": True, "fluxes_clear": True},
                              ("toa_scale", "cloud_mask", "delta_scale_off", "no_dn_dir", "no_dn_dir_clear", "empty_day_index"), False),
}
# (the one-stream longwave solvers take tau and ssa of two-stream particles: their g is never looked at, whatever it is)
IGNORES_G = ("lw_fluxes_allsky", "lw_fluxes_allsky+jac", "lw_fluxes_clear_allsky", "lw_fluxes_clear_allsky_jac")
# every method once (its widest route) for the wrong arrays: each array the call takes in turn, the others valid
WRONG_ARRAYS = ("lw_fluxes", "lw_fluxes_allsky", "lw_fluxes_allsky+2stream", "lw_fluxes_allsky+rescaled", "lw_fluxes_rescaled",
                "lw_fluxes_clear_allsky", "lw_fluxes_clear_allsky_jac", "sw_fluxes", "sw_fluxes_allsky", "sw_fluxes_clear_allsky",
                "sw_fluxes_daylit+both")
# every array gets a wrong shape; these get more (an input, an output, and what is not a float array)
MUTATIONS = {"plev": ("shape", "dtype", "strided", "other"), "flux_dn": ("shape", "dtype", "strided", "other"),
             "cloud_mask": ("shape", "dtype"), "day_index": ("shape", "dtype", "strided"), "vmr": ("shape", "other")}
GASES = ("scalars", "profile", "column", "unknown", "unset")   # (the base case: an (nlay, ncol) array and a scalar)
EVERY_GAS = ("lw_fluxes", "sw_fluxes")   # (the other WRONG_ARRAYS routes: the unknown and the unset gas)
# (id, route, precision, options): refusals of the Python mirror that no single wrong array reaches
REFUSALS = (
    ("rescaled and use_2stream", "lw_fluxes_allsky+rescaled", F64, {"use_2stream": True}),
    ("rescaled and flux_up_jac", "lw_fluxes_allsky+rescaled", F64, {"flux_up_jac": True}),
    ("rescaled and FluxesByband", "lw_fluxes_allsky+rescaled", F64, {"byband": True}),
    ("rescaled and one-stream particles", "lw_fluxes_allsky+rescaled", F64, {"one_stream": True}),
    ("rescaled and particles without g", "lw_fluxes_allsky+rescaled", F64, {"no_g": True}),
    ("rescaled, use_2stream and flux_up_jac, float32", "lw_fluxes_allsky+rescaled", F32, {"use_2stream": True, "flux_up_jac": True}),
    ("rescaled, float32 with a float64 flux_up_jac", "lw_fluxes_allsky+rescaled", F32, {"flux_up_jac": True, "other": "flux_up_jac"}),
    ("use_2stream and flux_up_jac", "lw_fluxes_allsky+2stream", F64, {"flux_up_jac": True}),
    ("use_2stream and two angles", "lw_fluxes_allsky+2stream", F64, {"n_gauss_angles": True}),
    ("use_2stream and one-stream particles", "lw_fluxes_allsky+2stream", F64, {"one_stream": True}),
    ("use_2stream and particles without g", "lw_fluxes_allsky+2stream", F64, {"no_g": True}),
    ("use_2stream and flux_up_jac, float32", "lw_fluxes_allsky+2stream", F32, {"flux_up_jac": True}),
    ("lw_fluxes_rescaled and one-stream particles", "lw_fluxes_rescaled", F64, {"one_stream": True}),
    ("lw_fluxes_rescaled and particles without g", "lw_fluxes_rescaled", F64, {"no_g": True}),
    ("lw_fluxes_rescaled and FluxesByband", "lw_fluxes_rescaled", F64, {"byband": True}),
    ("lw_fluxes_rescaled and FluxesByband for the clear sky", "lw_fluxes_rescaled", F64, {"fluxes_clear": True, "byband_clear": True}),
    ("lw_fluxes_clear_allsky_jac without flux_up_jac", "lw_fluxes_clear_allsky_jac", F64, {"null_jac": True}),
    ("lw_fluxes_clear_allsky_jac, float64 with a float32 flux_up_jac", "lw_fluxes_clear_allsky_jac", F64, {"other": "flux_up_jac"}),
    ("sw_fluxes_allsky and one-stream particles", "sw_fluxes_allsky", F64, {"one_stream": True}),
    ("sw_fluxes_clear_allsky and one-stream particles", "sw_fluxes_clear_allsky", F64, {"one_stream": True}),
)
# calls that go through although they look like refusals: (id, route, precision, options)
ACCEPTED = (
    ("sw_fluxes_allsky and particles without g", "sw_fluxes_allsky", F64, {"no_g": True}),
    ("lw_fluxes_allsky and particles without g", "lw_fluxes_allsky", F64, {"no_g": True}),
    ("lw_fluxes_allsky and FluxesByband", "lw_fluxes_allsky", F64, {"byband": True}),
)


class Recorder:
    """The library with every fused flux entry point replaced by a function that notes its arguments and returns 0."""

    def __init__(self, real):
        self._real = real
        self.calls = []

    def __getattr__(self, name):
        if "_fluxes" in name and not name.endswith("_bytes"):
            getattr(self._real, name)   # (a name the library does not export stays an AttributeError)
            return lambda *args: self.calls.append((name, args)) or 0
        return getattr(self._real, name)


def arrays(k, dt, shortwave):
    """The arrays of a case by name; every one a distinct allocation."""
    ng, nb = k.get_ngpt(), k.get_nband()
    lev, lay, col = (NLAY + 1, NCOL), (NLAY, NCOL), (NCOL,)
    f = lambda shape, v: np.full(shape, v, dt)
    a = {"plev": f(lev, 1e4), "tlay": f(lay, 250.0), "flux_up": f(lev, -7.0), "flux_dn": f(lev, -7.0),
         "flux_up_clear": f(lev, -7.0), "flux_dn_clear": f(lev, -7.0),
         "particles.tau": f((nb,) + lay, 0.5), "particles.ssa": f((nb,) + lay, 0.5), "particles.g": f((nb,) + lay, 0.5),
         "cloud_mask": np.full(lay, 5, np.uint64), "vmr": f(lay, 1e-3), "vmr_profile": f((NLAY,), 1e-3), "vmr_column": f(col, 1e-3)}
    if shortwave:
        a.update({"mu0": f(col, 0.5), "toa_scale": f(col, 1.0), "sfc_alb_dir": f((NCOL, nb), 0.2), "sfc_alb_dif": f((NCOL, nb), 0.3),
                  "flux_dn_dir": f(lev, -7.0), "flux_dn_dir_clear": f(lev, -7.0), "day_index": np.array([1], np.int32)})
    else:
        a.update({"tsfc": f(col, 250.0), "tlev": f(lev, 250.0), "sfc_emis": f((NCOL, nb), 0.98), "inc_flux": f((ng, NCOL), 1.0),
                  "flux_up_jac": f(lev, -7.0)})
    return a


def mutate(arr, how):
    ints = arr.dtype.kind in "ui"
    if how == "shape":   # (a list of columns has no expected length: it gets a second dimension)
        return arr.reshape(1, -1) if ints and arr.ndim == 1 else np.zeros(arr.shape[:-1] + (arr.shape[-1] + 1,), arr.dtype)
    if how == "dtype":
        return arr.astype(np.int64 if ints else np.int32)
    if how == "strided":   # (two entries at least: a view of one element counts as contiguous)
        last = max(arr.shape[-1], 2)
        return np.zeros(arr.shape[:-1] + (2 * last,), arr.dtype)[..., ::2]
    assert how == "other" and not ints
    return arr.astype(np.float32 if arr.dtype == np.float64 else np.float64)


def gases(pkg, k, a, how):
    first, second = k.get_gases()[:2]
    gc = pkg.GasConcs([first, second] + (["unobtainium"] if how == "unknown" else []))
    if how == "scalars":
        assert gc.set_vmr(first, 1e-3) == ""
    elif how == "column":
        assert gc.set_vmr_column(first, a["vmr_column"]) == ""
    else:
        assert gc.set_vmr(first, a["vmr_profile" if how == "profile" else "vmr"]) == ""
    if how != "unset":
        assert gc.set_vmr(second, 4e-4) == ""
    return gc


def keywords(pkg, k, method, a, o):
    """The keyword arguments of `method` from the arrays `a` and the options `o` (what is not named stays at its default)."""
    accepted = inspect.signature(getattr(k, method)).parameters
    shortwave = method.startswith("sw_")
    kw = {"plev": a["plev"], "tlay": a["tlay"], "gas_desc": gases(pkg, k, a, o.get("gas", "array")), "top_at_1": not o.get("full")}
    if shortwave:
        kw.update(mu0=a["mu0"], sfc_alb_dir=a["sfc_alb_dir"], sfc_alb_dif=a["sfc_alb_dif"])
    else:
        kw.update(tsfc=a["tsfc"], tlev=None if o.get("no_tlev") else a["tlev"], sfc_emis=a["sfc_emis"])

    def fluxes(suffix, byband, no_dir):
        args = [a["flux_up" + suffix], a["flux_dn" + suffix]] + ([None if no_dir else a["flux_dn_dir" + suffix]] if shortwave else [])
        return pkg.FluxesByband(None, None, None, *args) if byband else pkg.FluxesBroadband(*args)

    kw["fluxes"] = fluxes("", o.get("byband"), o.get("no_dn_dir"))
    if "fluxes_clear" in accepted and (o.get("fluxes_clear") or accepted["fluxes_clear"].default is inspect.Parameter.empty):
        kw["fluxes_clear"] = fluxes("_clear", o.get("byband_clear"), o.get("no_dn_dir_clear"))
    if "particles" in accepted and (o.get("particles") or accepted["particles"].default is inspect.Parameter.empty):
        p = pkg.OpticalProps1scl() if o.get("one_stream") else pkg.OpticalProps2str()
        p.tau = a["particles.tau"]
        if not o.get("one_stream"):
            p.ssa, p.g = a["particles.ssa"], None if o.get("no_g") else a["particles.g"]
        kw["particles"] = p
    for name in ("inc_flux", "cloud_mask", "flux_up_jac", "toa_scale", "day_index"):
        if o.get(name):
            kw[name] = a[name]
    if o.get("empty_day_index"):
        kw["day_index"] = np.zeros(0, np.int32)
    if o.get("null_jac"):
        kw["flux_up_jac"] = None
    for name in ("rescaled", "use_2stream"):
        if o.get(name):
            kw[name] = True
    if o.get("n_gauss_angles"):
        kw["n_gauss_angles"] = 2
    if o.get("delta_scale_off"):
        kw["delta_scale"] = False
    return kw


def leaves(kw):
    """Every array a call has been given, through its containers."""
    for v in kw.values():
        if isinstance(v, np.ndarray):
            yield v
        for attr in ("tau", "ssa", "g", "flux_up", "flux_dn", "flux_dn_dir"):
            if isinstance(getattr(v, attr, None), np.ndarray):
                yield getattr(v, attr)
        for w in getattr(v, "_conc", {}).values():
            w = w[1] if isinstance(w, tuple) else w
            if isinstance(w, np.ndarray):
                yield w


def cases(pkg, models):
    """[(id, route, precision, options, (array name, mutation) or None, expect a call)], in the order of the fixture."""
    out = []
    for route, (method, fixed, optional, serves_f32) in ROUTES.items():
        alone = [name for name in optional if name.startswith("no_") or name in ("one_stream", "empty_day_index")]
        full = dict(fixed, full=True, **{name: True for name in optional if name not in alone})
        for dt in (F64, F32):
            ok = dt == F64 or serves_f32
            out.append(("%s/%s/plain" % (route, dt), route, dt, dict(fixed), None, ok))
            out.append(("%s/%s/full" % (route, dt), route, dt, full, None, ok))
        for name in alone:   # (what takes something away cannot be part of `full`)
            out.append(("%s/%s/%s" % (route, F64, name), route, F64, dict(fixed, **{name: True}), None, True))
        for how in GASES if route in EVERY_GAS else GASES[-2:] if route in WRONG_ARRAYS else ():
            out.append(("%s/%s/gas %s" % (route, F64, how), route, F64, dict(fixed, gas=how), None, how != "unset"))
        if route in WRONG_ARRAYS:
            k = models[method.startswith("sw_")]
            a = arrays(k, np.dtype(F64), method.startswith("sw_"))
            used = list(leaves(keywords(pkg, k, method, a, full)))
            for name, arr in a.items():
                for how in MUTATIONS.get(name, ("shape",)) if any(arr is u for u in used) else ():
                    out.append(("%s/%s/%s %s" % (route, F64, name, how), route, F64, full, (name, how),
                                name == "particles.g" and route in IGNORES_G))
    for label, route, dt, o in REFUSALS:
        out.append(("refusal/" + label, route, dt, dict(ROUTES[route][1], **o), None, False))
    for label, route, dt, o in ACCEPTED:
        out.append(("accepted/" + label, route, dt, dict(ROUTES[route][1], **o), None, True))
    assert len({c[0] for c in out}) == len(out)
    return out


def normalise(x, a, k):
    if x is None or isinstance(x, int):
        return x
    if isinstance(x, bytes):   # the gas names, each padded to its 32 characters
        names = [x[i:i + 32].decode("ascii").rstrip(" ") for i in range(0, len(x), 32)]
        assert b"".join(n.encode().ljust(32, b" ") for n in names) == x
        return "names:" + ",".join(names)
    if isinstance(x, C.Array):
        return "ptrs:" + "".join(str(int(bool(p))) for p in x) if x._type_ is C.c_void_p else list(x)
    assert isinstance(x, C.c_void_p), "an argument of type %s" % type(x).__name__
    if not x.value:
        return None
    if x.value == k._h.value:
        return "handle"
    for name, arr in a.items():
        if arr.size and 0 <= x.value - arr.ctypes.data < arr.nbytes:
            return name + ("+%d" % (x.value - arr.ctypes.data) if x.value != arr.ctypes.data else "")
    raise AssertionError("a pointer into none of the arrays of the case")


def run(pkg, models, case):
    """Replay one case, as the fixture stores it: ``[id, "called", entry point, arguments]``, ``[id, "returned", message]``
    or ``[id, "raised", class name, text]``."""
    ident, route, dt, o, mutation, expect_call = case
    method = ROUTES[route][0]
    shortwave = method.startswith("sw_")
    k = models[shortwave]
    a = arrays(k, np.dtype(dt), shortwave)
    if mutation is not None:
        a[mutation[0]] = mutate(a[mutation[0]], mutation[1])
    if "other" in o:
        a[o["other"]] = mutate(a[o["other"]], "other")
    kw = keywords(pkg, k, method, a, o)
    real = pkg.lib()
    pkg._lib = rec = Recorder(real)
    try:
        outcome = ["returned", getattr(k, method)(**kw)]
    except Exception as e:
        outcome = ["raised", type(e).__name__, str(e)]
    finally:
        pkg._lib = real
    assert (len(rec.calls) == 1 and outcome == ["returned", ""]) if expect_call else not rec.calls, (ident, outcome, rec.calls)
    if rec.calls:
        outcome = ["called", rec.calls[0][0], [normalise(x, a, k) for x in rec.calls[0][1]]]
    return [ident] + outcome


def load_models(pkg):
    """Host-only models, by `shortwave`."""
    models = {}
    for shortwave, path in ((False, LW_FSCK), (True, SW_WIDE)):
        models[shortwave] = pkg.GasOpticsEcckd()
        err = models[shortwave].load(path, device=-1)
        assert err == "", err
    return models


def main():
    import rte_ecckd_amd as pkg
    pkg.build()
    models = load_models(pkg)
    head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    records = [run(pkg, models, c) for c in cases(pkg, models)]
    with open(PATH, "w") as f:   # one case per line: a change of behaviour shows as the lines it changes
        f.write('{"recorded_at": %s, "shape": %s, "cases": [\n' % (json.dumps(head), json.dumps({"nlay": NLAY, "ncol": NCOL})))
        f.write(",\n".join(json.dumps(r) for r in records))
        f.write("\n]}\n")
    called = sorted({r[2] for r in records if r[1] == "called"})
    print("wrote %s: %d cases (%d reach the library), %d bytes, recorded at %s" % (
        PATH, len(records), sum(r[1] == "called" for r in records), os.path.getsize(PATH), head))
    print("entry points:", " ".join(called))


if __name__ == "__main__":
    main()
