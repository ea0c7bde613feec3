#!/usr/bin/env python3
"""The longwave surface-temperature Jacobian next to the fluxes (ecckd_lw_fluxes_jac), fp64,
synthetic.columns / synthetic.clouds.  Per shape kind:ncol:nlay (kind = lw_fsck | lw_rrtmgp) and per configuration -- clear
sky and two-stream all sky -- on this build, interleaved in one process:
  (a) the existing call: lw_fluxes / lw_fluxes_allsky;
  (b) 60 layers: the call with flux_up_jac and "lw_jac_inline" = 1 (the Jacobian form of the layer-split kernel);
  (c) the call with flux_up_jac and "lw_jac_inline" = 0 (the flux kernel, then the stand-alone Jacobian kernel);
  (d) what a host does without the feature: the existing call twice (at tsfc and at tsfc + 1);
and, with --parent-lib,
  (e) the existing calls on this build and on another build of the library (the parent commit's), in fresh child processes
      that alternate: their min-max ranges must overlap.
The decision rule for the default of "lw_jac_inline": 1 only if the min-max range of (b) lies wholly below that of (c) for
every configuration at every 60-layer shape; otherwise 0.
HIP-event timing: 3 warm-up calls, then --repeats timed calls per variant, the variants interleaved round-robin; median
and min-max.  Usage: python tools/bench_lw_jac.py [--shapes lw_fsck:100000:60,...] [--parent-lib lib.so] [--out f.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_allsky import interleaved, stats  # noqa: E402
from bench_mcica import DATA, FILES  # noqa: E402

DEFAULT_SHAPES = "lw_fsck:100000:60,lw_fsck:1000000:60,lw_rrtmgp:100000:60,lw_fsck:100000:137"


def child(kind, ncol, nlay, repeats, existing_only):
    import torch
    sys.path.insert(0, ROOT)
    import rte_ecckd_amd as pkg
    from rte_ecckd_amd import synthetic
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def check(msg):
        if msg:
            raise SystemExit(msg)

    k = pkg.GasOpticsEcckd()
    check(k.load(os.path.join(DATA, FILES[kind]), device=0))
    ng, nb = k.get_ngpt(), k.get_nband()
    cols = synthetic.columns(0, ncol, k.get_press_min(), nlay=nlay)
    cloud = synthetic.clouds(0, ncol, nlay, nb)
    gc = pkg.GasConcs(synthetic.GAS_ORDER)
    for n in synthetic.GAS_ORDER:
        v = cols[n]
        if np.isscalar(v):
            gc.set_vmr(n, float(v))
        elif v.ndim == 1:
            gc.set_vmr_column(n, t(v))
        else:
            gc.set_vmr(n, t(v))
    plev, tlay, tlev = t(cols["plev"]), t(cols["tlay"]), t(cols["tlev"])
    tsfc, tsfc1 = t(cols["tsfc"]), t(cols["tsfc"] + 1.0)
    emis = t(np.repeat(cols["sfc_emis"][:, None], nb, 1))
    two = pkg.OpticalProps2str()
    two.tau, two.ssa, two.g = t(cloud["tau"]), t(cloud["ssa"]), t(cloud["g"])
    empty = lambda: torch.empty((nlay + 1, ncol), dtype=torch.float64, device=dev)
    fl, fl1, jac = pkg.FluxesBroadband(empty(), empty()), pkg.FluxesBroadband(empty(), empty()), empty()

    def clear(ts=tsfc, f=fl, **kw):
        check(k.lw_fluxes(plev, tlay, ts, tlev, gc, True, emis, f, **kw))

    def allsky(ts=tsfc, f=fl, **kw):
        check(k.lw_fluxes_allsky(plev, tlay, ts, tlev, gc, True, emis, two, f, **kw))

    variants = {}
    for name, call in (("clear", clear), ("allsky", allsky)):
        variants[name + ":a_existing_call"] = call
        if existing_only:
            continue

        def form(v, call=call):
            def run():
                pkg.set_solver_option("lw_jac_inline", v)
                call(flux_up_jac=jac)
            return run

        def twice(call=call):
            call()
            call(tsfc1, fl1)
        if nlay == 60:
            variants[name + ":b_jac_inline"] = form(1)
        variants[name + ":c_jac_stand_alone"] = form(0)
        variants[name + ":d_existing_call_twice"] = twice
    res = {n: stats(v) for n, v in interleaved(variants, repeats).items()}
    print(json.dumps({"kind": kind, "ncol": ncol, "nlay": nlay, "ngpt": ng, "nband": nb, "device": torch.cuda.get_device_name(0),
                      "build": pkg.lib().ecckd_build_info().decode(), "results": res}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2, help="fresh processes per build and shape, alternating")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lw_jac.json"))
    ap.add_argument("--child", default=None, help="(child mode) kind:ncol:nlay")
    ap.add_argument("--existing-only", action="store_true", help="(child mode) time the calls that exist on the parent alone")
    args = ap.parse_args()
    if args.child:
        kind, ncol, nlay = args.child.split(":")
        child(kind, int(ncol), int(nlay), args.repeats, args.existing_only)
        return

    def run(shape, lib, existing_only):
        env = dict(os.environ)
        env.pop("ECCKD_LIB", None)
        if lib:
            env["ECCKD_LIB"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--repeats", str(args.repeats)]
        print("bench_lw_jac: %s, %s" % (shape, "another build, existing calls" if lib else "this build"), file=sys.stderr, flush=True)
        r = subprocess.run(cmd + (["--existing-only"] if existing_only else []), env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:   # (a failed child ends the job: nothing more is started on the GPU)
            raise SystemExit("child failed (%s): %s" % (shape, r.stderr[-2000:]))
        return json.loads(r.stdout.strip().splitlines()[-1])

    out = {"timing": "HIP events, 3 warm-up calls, variants interleaved; builds in alternating fresh processes", "repeats": args.repeats,
           "shapes": []}
    below = []   # range of (b) wholly below range of (c), per configuration and 60-layer shape
    for shape in args.shapes.split(","):
        entry = {"shape": shape}
        if args.parent_lib:
            runs = {"parent": [], "branch": []}
            for _ in range(args.rounds):
                for name, lib in (("parent", args.parent_lib), ("branch", None)):
                    runs[name].append(run(shape, lib, True)["results"])
            overlap = {}
            for call in ("clear:a_existing_call", "allsky:a_existing_call"):
                lo = {b: min(c[call]["min_ms"] for c in runs[b]) for b in runs}
                hi = {b: max(c[call]["max_ms"] for c in runs[b]) for b in runs}
                med = {b: sorted(c[call]["median_ms"] for c in runs[b])[len(runs[b]) // 2] for b in runs}
                overlap[call] = {"parent_ms": [lo["parent"], hi["parent"]], "branch_ms": [lo["branch"], hi["branch"]],
                                 "parent_median_ms": med["parent"], "branch_median_ms": med["branch"],
                                 "ranges_overlap": lo["parent"] <= hi["branch"] and lo["branch"] <= hi["parent"]}
            entry["e_existing_calls_min_max"] = overlap
        new = run(shape, None, False)
        entry.update({n: new[n] for n in ("kind", "ncol", "nlay", "ngpt", "device", "build")})
        r = new["results"]
        entry["results"] = r
        ratios = {}
        for cfg in ("clear", "allsky"):
            a = r[cfg + ":a_existing_call"]
            ratios[cfg] = {}
            for key, label in (("b_jac_inline", "b_over_a"), ("c_jac_stand_alone", "c_over_a"), ("d_existing_call_twice", "d_over_a")):
                v = r.get(cfg + ":" + key)
                if v:
                    ratios[cfg][label] = v["median_ms"] / a["median_ms"]
                    ratios[cfg][label + "_range"] = [v["min_ms"] / a["max_ms"], v["max_ms"] / a["min_ms"]]
            b, c = r.get(cfg + ":b_jac_inline"), r[cfg + ":c_jac_stand_alone"]
            if b:
                ratios[cfg]["b_wholly_below_c"] = b["max_ms"] < c["min_ms"]
                below.append(b["max_ms"] < c["min_ms"])
        entry["ratios"] = ratios
        out["shapes"].append(entry)
        print(json.dumps({k: v for k, v in entry.items() if k != "results"}), flush=True)
    out["lw_jac_inline_default_by_rule"] = int(bool(below) and all(below))
    print(json.dumps({"lw_jac_inline_default_by_rule": out["lw_jac_inline_default_by_rule"]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
