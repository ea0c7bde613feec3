"""Writes tests/golden/capi_refusals.json: what every fused flux entry point of the C ABI (``ecckd_*_fluxes*``,
``ecckd_*_flux_bands``, ``ecckd_*_flux_scaled``, fp64 and ``_f32``) answers to a call it refuses -- return value and
``ecckd_last_error()`` -- one fault at a time and two at a time, so that the ORDER of the refusals is on record too.

    python tests/golden/make_golden_capi_refusals.py            # the host section (no GPU)
    python tests/golden/make_golden_capi_refusals.py --device   # the device section as well (needs a GPU)

The calls go through ``ctypes`` straight to the library with the argument types of ``_fused_prototypes()``, not through
the methods of the Python mirror (which refuses much of this itself).  ``(ncol, nlay) = (2, 3)``.

The host section.  Host-only models (``device=-1``).  Per entry point one valid call (the host-only refusal) and every
fault of ``faults()`` that applies to its arguments, alone; then every pair of two faults that touch different arguments,
both at once.  Two more models of 65 g-points (one with a Planck table, one with a solar table) take the calls that name a
cloud mask.

The device section.  The refusals behind ``check_model`` need a model on a device: a null required array, a bad memory
space (``ECCKD_MIXED`` included), bad ``ncol`` / ``nlay``, ``ncol = 0`` (returns 0, with and without a mask), a mask on a
device model of 65 g-points; and, since the plain calls (``ecckd_lw_fluxes``, ``ecckd_sw_fluxes``, ``ecckd_lw_fluxes_jac``
without ``tau_p``) keep their whole list behind ``check_model``: the other spectrum's model, arithmetic mode 1,
``n_gauss_angles`` 0 and 5, a clear sky with something of the particles' left over or with an aliased ``flux_up_jac``.
Each alone and every pair; none of them launches a kernel.

The file.  ``outcomes`` is the table of distinct ``[return value, message]`` (the message is "" where the call
returned 0); per section and entry point ``singles`` is ``{case id: outcome}`` and ``pairs[i][j - i - 1]`` the outcome of
``"<single i>+<single j>"`` in the order of ``singles`` (-1: the two touch the same argument, no such case).
``expand()`` turns a section back into ``{(entry point, case id): [return value, message]}``.  The file also holds
``git rev-parse HEAD`` of the tree whose library answered ("recorded_at"): generate it before a change of
rte-ecckd_amd/csrc/capi.cpp, replay it after (tests/test_capi_refusals_host.py, tests/test_gpu_capi_refusals.py),
regenerate only where a change of behaviour is meant.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PATH = os.path.join(HERE, "capi_refusals.json")
DATA = os.path.join(ROOT, "data")
LW_FSCK = os.path.join(DATA, "ecckd-1.2_lw_ckd-definition_climate_fsck-tol0.0161.nc")   # (tests/conftest.py)
SW_WIDE = os.path.join(DATA, "ecckd-1.2_sw_ckd-definition_climate_wide-tol0.05.nc")
NCOL, NLAY = 2, 3
HOST, DEVICE, MIXED = 0, 1, 2

# the named pieces of the argument lists, as rte_ecckd_amd._fused_prototypes() has them: i = int, p = pointer, s = char *
_GAS = [("ngas", "i"), ("gas_names", "s"), ("vmr", "p"), ("col_stride", "p"), ("lay_stride", "p"), ("scalar", "p")]
_TAIL = [("space", "i"), ("stream", "p")]


def _p(*names):
    return [(n, "p") for n in names]


def _i(*names):
    return [(n, "i") for n in names]


_LW = _p("model") + _i("ncol", "nlay") + _p("plev", "tlay", "tsfc", "tlev") + _GAS
_SW = _p("model") + _i("ncol", "nlay") + _p("plev", "tlay") + _GAS
_SW_DAYLIT = _p("model") + _i("ncol", "nlay", "nday") + _p("day_index", "plev", "tlay") + _GAS
_LW_BOUND = _i("top_at_1", "n_gauss_angles") + _p("sfc_emis", "inc_flux")
_LW_BOUND_2STREAM = _i("top_at_1") + _p("sfc_emis", "inc_flux")
_SW_BOUND = _i("top_at_1") + _p("mu0", "toa_scale", "sfc_alb_dir", "sfc_alb_dif")
_LW_PART = _i("nband_p") + _p("tau_p", "ssa_p")
_LW_PART_G = _i("nband_p") + _p("tau_p", "ssa_p", "g_p")
_SW_PART = _i("nband_p") + _p("tau_p", "ssa_p", "g_p") + _i("delta_scale")
_MASK, _SCALING = _p("cloud_mask"), _p("cloud_scaling")
_LW_OUT, _LW_CLEAR, _JAC = _p("flux_up", "flux_dn"), _p("flux_up_clear", "flux_dn_clear"), _p("flux_up_jac")
_SW_OUT, _SW_CLEAR = _p("flux_up", "flux_dn", "flux_dn_dir"), _p("flux_up_clear", "flux_dn_clear", "flux_dn_dir_clear")
_LW_BANDS, _SW_BANDS = _p("bnd_flux_up", "bnd_flux_dn"), _p("bnd_flux_up", "bnd_flux_dn", "bnd_flux_dn_dir")

# entry point: (its arguments by name, an _f32 namesake exists)
SIGNATURES = {
    "ecckd_lw_flux_bands": (_LW + _LW_BOUND + _LW_PART + _MASK + _LW_BANDS + _LW_OUT + _TAIL, False),
    "ecckd_sw_flux_bands": (_SW + _SW_BOUND + _SW_PART + _MASK + _SW_BANDS + _SW_OUT + _TAIL, False),
    "ecckd_lw_flux_scaled": (_LW + _LW_BOUND + _LW_PART + _SCALING + _LW_OUT + _TAIL, False),
    "ecckd_sw_flux_scaled": (_SW + _SW_BOUND + _SW_PART + _SCALING + _SW_OUT + _TAIL, False),
    "ecckd_lw_fluxes": (_LW + _LW_BOUND + _LW_OUT + _TAIL, True),
    "ecckd_lw_fluxes_allsky": (_LW + _LW_BOUND + _LW_PART + _LW_OUT + _TAIL, True),
    "ecckd_lw_fluxes_allsky_mcica": (_LW + _LW_BOUND + _LW_PART + _MASK + _LW_OUT + _TAIL, True),
    "ecckd_lw_fluxes_clear_allsky": (_LW + _LW_BOUND + _LW_PART + _MASK + _LW_OUT + _LW_CLEAR + _TAIL, True),
    "ecckd_lw_fluxes_jac": (_LW + _LW_BOUND + _LW_PART + _MASK + _LW_OUT + _LW_CLEAR + _JAC + _TAIL, False),
    "ecckd_lw_fluxes_allsky_2stream": (_LW + _LW_BOUND_2STREAM + _LW_PART_G + _MASK + _LW_OUT + _TAIL, True),
    "ecckd_lw_fluxes_allsky_rescaled": (_LW + _LW_BOUND + _LW_PART_G + _MASK + _LW_OUT + _TAIL, False),
    "ecckd_lw_fluxes_rescaled_jac": (_LW + _LW_BOUND + _LW_PART_G + _MASK + _LW_OUT + _LW_CLEAR + _JAC + _TAIL, False),
    "ecckd_sw_fluxes": (_SW + _SW_BOUND + _SW_OUT + _TAIL, True),
    "ecckd_sw_fluxes_allsky": (_SW + _SW_BOUND + _SW_PART + _SW_OUT + _TAIL, True),
    "ecckd_sw_fluxes_allsky_mcica": (_SW + _SW_BOUND + _SW_PART + _MASK + _SW_OUT + _TAIL, True),
    "ecckd_sw_fluxes_clear_allsky": (_SW + _SW_BOUND + _SW_PART + _MASK + _SW_OUT + _SW_CLEAR + _TAIL, True),
    "ecckd_sw_fluxes_daylit": (_SW_DAYLIT + _SW_BOUND + _SW_PART + _MASK + _SW_OUT + _SW_CLEAR + _TAIL, False),
}
_CTYPE = {"i": C.c_int, "p": C.c_void_p, "s": C.c_char_p}

PLANES = ("tau_p", "ssa_p", "g_p")
CLEAR_OUT = ("flux_up_clear", "flux_dn_clear", "flux_dn_dir_clear")
OUTPUTS = ("bnd_flux_up", "bnd_flux_dn", "bnd_flux_dn_dir", "flux_up", "flux_dn", "flux_dn_dir") + CLEAR_OUT + ("flux_up_jac",)
# what belongs to the particles of a call: gone together in the "clear sky" cases
PARTICLE_SIDE = PLANES + ("cloud_mask", "cloud_scaling") + CLEAR_OUT
# the arrays a call cannot do without once the model is on a device (the band calls sum into flux_up / flux_dn only if given)
REQUIRED = ("plev", "tlay", "tsfc", "tlev", "gas_names", "sfc_emis", "mu0", "sfc_alb_dir", "sfc_alb_dif", "bnd_flux_up",
            "bnd_flux_dn", "flux_up", "flux_dn")


def entry_points():
    """[(entry point, its arguments by name, single precision)] in the order of the fixture."""
    out = []
    for name, (sig, has_f32) in SIGNATURES.items():
        out.append((name, sig, False))
        if has_f32:
            out.append((name + "_f32", sig, True))
    return out


def shortwave(name):
    return name.startswith("ecckd_sw_")


class Models:
    """The models of a section, by (shortwave, wide): the two files, and two 65-g models from tables."""

    def __init__(self, pkg, device):
        self.pkg, self.by = pkg, {}
        for sw, path in ((False, LW_FSCK), (True, SW_WIDE)):
            k = pkg.GasOpticsEcckd()
            err = k.load(path, device=device)
            assert err == "", err
            self.by[(sw, False)] = k
        lp, T, ng = np.log([10., 100., 1000.]), 200. + np.arange(6).reshape(2, 3), 65
        for sw in (False, True):
            k = pkg.GasOpticsEcckd()
            table = dict(solar=(np.ones(ng), np.zeros(ng))) if sw else dict(planck=(np.array([100., 200.]), np.ones((2, ng))))
            err = k.init_from_tables(lp, T, [dict(name="x", code=1, coefficient=np.ones((2, 3, ng)))], device=device, **table)
            assert err == "", err
            self.by[(sw, True)] = k

    def handle(self, sw, wide=False):
        return self.by[(sw, wide)]._h.value


def baseline(models, name, sig, f32):
    """The arguments of a valid call by name (every optional array given but inc_flux and toa_scale) and the arrays they
    point into, which the caller keeps alive."""
    sw = shortwave(name)
    k = models.by[(sw, False)]
    ng, nb = k.get_ngpt(), k.get_nband()
    dt = np.float32 if f32 else np.float64
    lev, lay = (NLAY + 1, NCOL), (NLAY, NCOL)
    full = lambda shape, v: np.full(shape, v, dt)
    arrays = {"plev": full(lev, 1e4), "tlay": full(lay, 250.0), "tsfc": full((NCOL,), 250.0), "tlev": full(lev, 250.0),
              "sfc_emis": full((NCOL, nb), 0.98), "mu0": full((NCOL,), 0.5), "sfc_alb_dir": full((NCOL, nb), 0.2),
              "sfc_alb_dif": full((NCOL, nb), 0.3), "tau_p": full((nb,) + lay, 0.5), "ssa_p": full((nb,) + lay, 0.5),
              "g_p": full((nb,) + lay, 0.5), "cloud_mask": np.full(lay, 5, np.uint64),
              "cloud_scaling": np.full((ng,) + lay, 1.0, np.float32), "day_index": np.array([1], np.int32),
              "vmr0": full(lay, 1e-3)}
    for o in OUTPUTS:
        arrays[o] = full((nb,) + lev if o.startswith("bnd_") else lev, -7.0)
    first, second = k.get_gases()[:2]
    arrays["gas_names"] = C.create_string_buffer(b"".join(g.encode().ljust(32, b" ") for g in (first, second)), 64)
    arrays["vmr"] = (C.c_void_p * 2)(arrays["vmr0"].ctypes.data, None)
    arrays["col_stride"], arrays["lay_stride"] = (C.c_longlong * 2)(1, 0), (C.c_longlong * 2)(NCOL, 0)
    arrays["scalar"] = (C.c_double * 2)(0.0, 4e-4)
    ints = {"ncol": NCOL, "nlay": NLAY, "nday": 1, "ngas": 2, "top_at_1": 1, "n_gauss_angles": 1, "nband_p": nb, "delta_scale": 1,
            "space": HOST}
    args = {}
    for arg, kind in sig:
        if kind == "i":
            args[arg] = ints[arg]
        elif arg == "model":
            args[arg] = models.handle(sw)
        elif arg in ("inc_flux", "toa_scale", "stream"):
            args[arg] = None
        elif arg == "gas_names":
            args[arg] = C.cast(arrays[arg], C.c_char_p)
        elif isinstance(arrays[arg], np.ndarray):
            args[arg] = arrays[arg].ctypes.data
        else:
            args[arg] = C.cast(arrays[arg], C.c_void_p).value
    return args, arrays


def faults(models, name, sig):
    """{case id: the arguments it replaces}, host section: every fault that applies to the arguments of `name`.  The key
    "arithmetic" is no argument: the call runs in that arithmetic mode."""
    has = {a for a, _ in sig}
    sw = shortwave(name)
    nb = models.by[(sw, False)].get_nband()
    f = {"null model": {"model": None}, "the other spectrum's model": {"model": models.handle(not sw)},
         "arithmetic mode 1": {"arithmetic": 1}}
    side = {a: None for a in PARTICLE_SIDE if a in has}
    if "nband_p" in has:
        f["nband_p wrong"] = {"nband_p": nb + 1}
        f["nband_p 0"] = {"nband_p": 0}
        f["clear sky"] = dict(side, nband_p=0)
        for a in side:   # a stray plane, mask, scaling or clear-sky output where the call then takes none
            f["clear sky but " + a] = {b: v for b, v in dict(side, nband_p=0).items() if b != a}
            f["clear sky (nband_p kept) but " + a] = {b: v for b, v in side.items() if b != a}
        f["clear sky (nband_p kept)"] = dict(side)
        for a in PLANES + ("cloud_mask", "cloud_scaling") + CLEAR_OUT:
            if a in has:
                f["null " + a] = {a: None}
    if "cloud_mask" in has:
        f["65-g model"] = {"model": models.handle(sw, True)}
    if "delta_scale" in has:
        f["delta_scale 2"] = {"delta_scale": 2}
    if "tlev" in has:
        f["null tlev"] = {"tlev": None}
    if "n_gauss_angles" in has:
        f["n_gauss_angles 0"], f["n_gauss_angles 5"] = {"n_gauss_angles": 0}, {"n_gauss_angles": 5}
    outs = [o for o in OUTPUTS if o in has]
    for i, a in enumerate(outs):
        for b in outs[i + 1:]:
            f["%s is %s" % (b, a)] = {b: ("same as", a)}
    if "nday" in has:
        f["nday -1"], f["nday ncol+1"] = {"nday": -1}, {"nday": NCOL + 1}
        f["day_index unsorted"] = {"nday": 2, "day_index": ("array", np.array([1, 0], np.int32))}
        f["day_index null"] = {"day_index": None}
        f["nday 0"] = {"nday": 0}
    return f


def device_faults(models, name, sig):
    """{case id: the arguments it replaces}, device section: what only a model on a device is asked.  No case launches."""
    has = {a for a, _ in sig}
    sw = shortwave(name)
    required = [a for a in REQUIRED if a in has and not ("_flux_bands" in name and a in ("flux_up", "flux_dn"))]
    f = {"null " + a: {a: None} for a in required}
    f.update({"memspace 7": {"space": 7}, "memspace ECCKD_MIXED": {"space": MIXED}, "ncol -1": {"ncol": -1}, "nlay 0": {"nlay": 0},
              "ncol 0": {"ncol": 0}, "ncol 0, device arrays": {"ncol": 0, "space": DEVICE}})
    if "nday" in has:
        f["ncol 0"], f["ncol 0, device arrays"] = {"ncol": 0, "nday": 0}, {"ncol": 0, "nday": 0, "space": DEVICE}
    if "cloud_mask" in has:
        f["65-g model"] = {"model": models.handle(sw, True)}
        f["65-g model, no mask, ncol 0"] = {"model": models.handle(sw, True), "cloud_mask": None, "ncol": 0, "nday": 0}
    # what a host-only model answers too, for the calls whose whole list stands behind check_model (and the others once more)
    f["the other spectrum's model"] = {"model": models.handle(not sw)}
    f["arithmetic mode 1"] = {"arithmetic": 1}
    if "n_gauss_angles" in has:
        f["n_gauss_angles 0"], f["n_gauss_angles 5"] = {"n_gauss_angles": 0}, {"n_gauss_angles": 5}
    if "nband_p" in has:   # (the clear sky itself would compute: only with something of the particles' left, or an aliased Jacobian)
        side = {a: None for a in PARTICLE_SIDE if a in has}
        for a in side:
            f["clear sky but " + a] = {b: v for b, v in dict(side, nband_p=0).items() if b != a}
        if "flux_up_jac" in has:
            f["clear sky, flux_up_jac is flux_up"] = dict(side, nband_p=0, flux_up_jac=("same as", "flux_up"))
    return f


def call(pkg, name, sig, args, arrays, *changes):
    """The outcome [return value, message] of `name` with `changes` applied to its valid arguments in turn."""
    a = dict(args)
    keep = []
    for change in changes:
        for arg, v in change.items():
            if isinstance(v, tuple) and v[0] == "same as":
                v = args[v[1]]
            elif isinstance(v, tuple) and v[0] == "array":
                keep.append(v[1])
                v = v[1].ctypes.data
            a[arg] = v
    L = pkg.lib()
    fn = getattr(L, name)
    assert fn.argtypes == [_CTYPE[kind] for _, kind in sig], name   # (set by lib(), from _fused_prototypes())
    mode = a.pop("arithmetic", 0)
    if mode:
        assert L.ecckd_set_arithmetic(mode) == 0
    try:
        ret = fn(*[a[arg] for arg, _ in sig])
    finally:
        if mode:
            L.ecckd_set_arithmetic(0)
    for arr in arrays.values():   # a refused call, and a call on no columns, leave every output as it was
        if isinstance(arr, np.ndarray) and arr.dtype.kind == "f" and arr.flat[0] == -7.0:
            assert np.all(arr == -7.0), name
    return [int(ret), pkg.last_error() if ret else ""]


def case_ids(models, device=False):
    """{entry point: (single ids in order, [(i, j)] of the pairs)} -- what the file must hold."""
    out = {}
    for name, sig, f32 in entry_points():
        f = device_faults(models, name, sig) if device else faults(models, name, sig)
        ids = ["valid"] + list(f) if not device else list(f)
        changes = [{}] * (0 if device else 1) + list(f.values())
        pairs = [(i, j) for i in range(0 if device else 1, len(ids)) for j in range(i + 1, len(ids))
                 if not set(changes[i]) & set(changes[j])]
        out[name] = (ids, changes, pairs)
    return out


def record(pkg, models, device=False):
    """{(entry point, case id): [return value, message]} of a section, from the library that `pkg` has loaded."""
    out = {}
    for name, sig, f32 in entry_points():
        ids, changes, pairs = case_ids(models, device)[name]
        args, arrays = baseline(models, name, sig, f32)
        for ident, change in zip(ids, changes):
            out[(name, ident)] = call(pkg, name, sig, args, arrays, change)
            assert not device or out[(name, ident)][0] or "ncol 0" in ident, (name, ident, "would have launched")
        for i, j in pairs:
            out[(name, ids[i] + "+" + ids[j])] = call(pkg, name, sig, args, arrays, changes[i], changes[j])
            assert not device or out[(name, ids[i] + "+" + ids[j])][0] or "ncol 0" in ids[i] + ids[j], (name, ids[i], ids[j], "would have launched")
    return out


def compact(models, recorded, outcomes, device=False):
    """A section in the form of the file (module docstring); `outcomes` grows by what is new."""
    def index(o):
        if o not in outcomes:
            outcomes.append(o)
        return outcomes.index(o)

    section = {}
    for name, (ids, changes, pairs) in case_ids(models, device).items():
        rows = [[-1] * (len(ids) - i - 1) for i in range(len(ids))] if pairs else []
        for i, j in pairs:
            rows[i][j - i - 1] = index(recorded[(name, ids[i] + "+" + ids[j])])
        section[name] = {"singles": {ident: index(recorded[(name, ident)]) for ident in ids}, "pairs": rows}
    return section


def expand(fixture, section):
    """{(entry point, case id): [return value, message]} of a section of the file."""
    out = {}
    for name, entry in fixture[section].items():
        ids = list(entry["singles"])
        for ident, o in entry["singles"].items():
            out[(name, ident)] = fixture["outcomes"][o]
        for i, row in enumerate(entry["pairs"]):
            for k, o in enumerate(row):
                if o >= 0:
                    out[(name, ids[i] + "+" + ids[i + 1 + k])] = fixture["outcomes"][o]
    return out


def main():
    import rte_ecckd_amd as pkg
    pkg.lib()
    head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    out = PATH
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    if "--recorded-at" in sys.argv:   # (where the tree is no git checkout)
        head = sys.argv[sys.argv.index("--recorded-at") + 1]
    fixture = {"recorded_at": head, "shape": {"ncol": NCOL, "nlay": NLAY}, "outcomes": [], "host": {}, "device": {}}
    if os.path.exists(PATH):   # a section that is not recorded now stays as it is
        with open(PATH) as f:
            old = json.load(f)
        fixture["outcomes"], fixture["host"], fixture["device"] = old["outcomes"], old["host"], old["device"]
        assert "--device" not in sys.argv or old["recorded_at"] == head, "the two sections come from one tree"
    if "--device" in sys.argv:
        models = Models(pkg, 0)
        fixture["device"] = compact(models, record(pkg, models, True), fixture["outcomes"], True)
    else:
        models = Models(pkg, -1)
        fixture["outcomes"] = []
        fixture["device"] = {}
        fixture["host"] = compact(models, record(pkg, models), fixture["outcomes"])
    with open(out, "w") as f:   # one entry point and section per line
        f.write('{"recorded_at": %s, "shape": %s,\n"outcomes": [\n' % (json.dumps(head), json.dumps(fixture["shape"])))
        f.write(",\n".join(json.dumps(o) for o in fixture["outcomes"]))
        for section in ("host", "device"):
            f.write('\n],\n"%s": {\n' % section if section == "host" else '\n},\n"%s": {\n' % section)
            f.write(",\n".join("%s: %s" % (json.dumps(n), json.dumps(e, separators=(",", ":"))) for n, e in fixture[section].items()))
        f.write("\n}}\n")
    n = {s: len(expand(fixture, s)) for s in ("host", "device")}
    print("wrote %s: %d host cases, %d device cases, %d outcomes, %d bytes, recorded at %s" % (
        out, n["host"], n["device"], len(fixture["outcomes"]), os.path.getsize(out), head))


if __name__ == "__main__":
    main()
