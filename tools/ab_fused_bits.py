#!/usr/bin/env python3
"""Bits of every fused flux entry point of the C ABI on this build against another build of the library (the parent
commit's): the same calls in two fresh child processes (ECCKD_LIB selects the library), every output array compared as
bytes, so that NaN equals NaN.  A recorded measurement, not a test: later kernel work may move last bits on purpose.

What a child calls, through ctypes with the argument lists of tests/golden/make_golden_capi_refusals.py: each of the 26
entry points (``ecckd_*_fluxes*``, ``ecckd_*_flux_bands``, ``ecckd_*_flux_scaled``) at 97 columns (a multiple of neither 16,
32 nor 64) and 60, 37 and 137 layers (the fused kernels, the general route, the overflow ring), on
``synthetic.columns`` / ``synthetic.clouds`` with a random 64-bit mask and a random float32 scaling, every optional array
given, with device arrays and with host arrays, and with each value of the solver option that routes the call
("lw_jac_inline", "lw_both_skies", "sw_solver": 0 and 1).  A call that the library refuses at a depth (the two-stream
longwave beyond its layer limit) is recorded by its message.

The run fails if a child fails (each has its own time limit), if any output differs, or if an entry point is not served
(return value 0) in each of the two memory spaces.

    python tools/ab_fused_bits.py --parent-lib lib.so [--out profiles/fused_call_refactor_bits.json]"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCOL, DEPTHS = 97, (60, 37, 137)
HOST, DEVICE = 0, 1
OPTIONS = {"lw_jac_inline": lambda n: "_jac" in n, "lw_both_skies": lambda n: n.startswith("ecckd_lw") and ("clear_allsky" in n or n.endswith("_jac")),
           "sw_solver": lambda n: n.startswith("ecckd_sw")}


def child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import torch
    import rte_ecckd_amd as pkg
    from rte_ecckd_amd import synthetic
    import make_golden_capi_refusals as gen

    L = pkg.lib()
    dev = torch.device("cuda:0")
    models = {}
    for sw, path in ((False, gen.LW_FSCK), (True, gen.SW_WIDE)):
        models[sw] = pkg.GasOpticsEcckd()
        msg = models[sw].load(path, device=0)
        if msg:
            raise SystemExit(msg)
    results = {}

    def inputs(sw, nlay, f32):
        """The arrays of a call by argument name (numpy, the precision of the call) and its integer arguments."""
        k = models[sw]
        ng, nb = k.get_ngpt(), k.get_nband()
        cols = synthetic.columns(0, NCOL, k.get_press_min(), nlay=nlay, shortwave=sw)
        cl = synthetic.clouds(0, NCOL, nlay, nb)
        rng = np.random.default_rng(nlay + 1000 * sw)
        dt = np.float32 if f32 else np.float64
        a = {name: cols[name].astype(dt) for name in ("plev", "tlay", "tlev", "tsfc")}
        a["tau_p"], a["ssa_p"], a["g_p"] = (cl[x].astype(dt) for x in ("tau", "ssa", "g"))
        a["cloud_mask"] = rng.integers(0, 2 ** 64, (nlay, NCOL), dtype=np.uint64)
        a["cloud_scaling"] = rng.uniform(0.0, 2.0, (ng, nlay, NCOL)).astype(np.float32)
        a["inc_flux"] = rng.uniform(0.0, 5.0, (ng, NCOL)).astype(dt)
        a["sfc_emis"] = np.ascontiguousarray(np.repeat(cols["sfc_emis"][:, None], nb, 1)).astype(dt)
        if sw:
            a["mu0"] = cols["mu0"].astype(dt)
            a["toa_scale"] = rng.uniform(0.9, 1.1, NCOL).astype(dt)
            a["sfc_alb_dir"] = np.ascontiguousarray(np.repeat(cols["albedo"][:, None], nb, 1)).astype(dt)
            a["sfc_alb_dif"] = (a["sfc_alb_dir"] * dt(0.9)).astype(dt)
        a["day_index"] = np.arange(0, NCOL, 2, dtype=np.int32)
        names = synthetic.GAS_ORDER
        arrays = [n for n in names if not np.isscalar(cols[n])]   # (ncol,) or (nlay, ncol); the others are scalars
        for n in arrays:
            a[n] = cols[n].astype(dt)
        for o in gen.OUTPUTS:
            a[o] = np.full((nb, nlay + 1, NCOL) if o.startswith("bnd_") else (nlay + 1, NCOL), -7.0, dt)
        scalars = (C.c_double * len(names))(*[0.0 if n in arrays else float(cols[n]) for n in names])
        ints = {"ncol": NCOL, "nlay": nlay, "nday": len(a["day_index"]), "ngas": len(names), "top_at_1": 1, "n_gauss_angles": 2,
                "nband_p": nb, "delta_scale": 1}
        return a, ints, names, arrays, scalars

    for name, sig, f32 in gen.entry_points():
        sw = gen.shortwave(name)
        fn = getattr(L, name)
        option_sets = [{}] + [{opt: v} for opt, applies in OPTIONS.items() if applies(name) for v in (0.0, 1.0)]
        for nlay in DEPTHS:
            a, ints, names, arrays, scalars = inputs(sw, nlay, f32)
            for space in (DEVICE, HOST):
                for opts in option_sets:
                    bits = lambda v: v.view(np.int64) if v.dtype == np.uint64 else v   # (torch has no uint64 arithmetic; same bytes)
                    held = {n: (torch.from_numpy(bits(v).copy()).to(dev) if space == DEVICE else v.copy()) for n, v in a.items()}
                    ptr = lambda n: held[n].data_ptr() if space == DEVICE else held[n].ctypes.data
                    vmr = (C.c_void_p * len(names))(*[ptr(n) if n in arrays else None for n in names])
                    cs = (C.c_longlong * len(names))(*[1 if n in arrays else 0 for n in names])
                    ls = (C.c_longlong * len(names))(*[NCOL if n in arrays and a[n].ndim == 2 else 0 for n in names])
                    gas_names = b"".join(n.encode().ljust(32, b" ") for n in names)
                    special = {"model": models[sw]._h.value, "gas_names": gas_names, "vmr": C.cast(vmr, C.c_void_p).value,
                               "col_stride": C.cast(cs, C.c_void_p).value, "lay_stride": C.cast(ls, C.c_void_p).value,
                               "scalar": C.cast(scalars, C.c_void_p).value, "space": space, "stream": None}
                    args = [special[n] if n in special else ints[n] if kind == "i" else ptr(n) for n, kind in sig]
                    pkg.reset_solver_options()
                    for opt, v in opts.items():
                        pkg.set_solver_option(opt, v)
                    ret = fn(*args)
                    pkg.reset_solver_options()
                    key = "%s nlay=%d %s %s" % (name, nlay, "device" if space == DEVICE else "host",
                                                ",".join("%s=%d" % kv for kv in opts.items()) or "default")
                    if ret:
                        results[key] = {"refused": pkg.last_error()}
                        continue
                    if space == DEVICE:
                        torch.cuda.synchronize()
                    outs = {}
                    for o in gen.OUTPUTS:
                        if o in dict(sig):
                            b = held[o].cpu().numpy() if space == DEVICE else held[o]
                            outs[o] = hashlib.sha256(np.ascontiguousarray(b).view(np.uint8).tobytes()).hexdigest()
                            if np.all(b == -7.0):
                                raise SystemExit("%s: %s was not written" % (key, o))
                    results[key] = outs
    print("BITS " + json.dumps(results), flush=True)


def run(lib, timeout):
    env = dict(os.environ)
    env.pop("ECCKD_LIB", None)
    if lib:
        env["ECCKD_LIB"] = os.path.abspath(lib)
    r = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(__file__), "--child"], env=env, cwd=ROOT,
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("the child on %s failed with %d (nothing more is started)\n%s\n%s" % (
            lib or "this build", r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    return json.loads([x for x in r.stdout.splitlines() if x.startswith("BITS ")][-1][5:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=False)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child()
    if not args.parent_lib:
        raise SystemExit("--parent-lib is required")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_capi_refusals as gen
    parent, branch = run(args.parent_lib, args.timeout), run(None, args.timeout)
    differ = sorted(k for k in set(parent) | set(branch) if parent.get(k) != branch.get(k))
    served = {(k.split()[0], k.split()[2]) for k, v in branch.items() if "refused" not in v}
    unserved = sorted((n, s) for n, _, _ in gen.entry_points() for s in ("device", "host") if (n, s) not in served)
    report = {"ncol": NCOL, "depths": list(DEPTHS), "calls": len(branch), "refused": sum("refused" in v for v in branch.values()),
              "output_arrays_compared": sum(len(v) for v in branch.values() if "refused" not in v),
              "differ": differ, "entry_points_not_served_in_a_memory_space": unserved, "identical": not differ and not unserved}
    print(json.dumps(report, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    if differ or unserved:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
