#!/usr/bin/env python3
"""The rescaled no-scattering longwave solver next to its neighbours, fp64, fast arithmetic mode.
Per shape kind:ncol:nlay (kind = lw_fsck | lw_rrtmgp), on this build, interleaved in one process:
  solver   ecckd_rte_lw_rescaled beside ecckd_rte_lw (1 angle) and ecckd_rte_lw_2stream on arrays of the same size (random
           optical properties generated on the device);
  fused    ecckd_lw_fluxes_allsky_rescaled beside its composed route (gas_optics_tau into the two-stream container's tau,
           ssa and g zeroed, planck_sources, increment by band, rte_lw(rescaled=True)), beside the no-scattering
           ecckd_lw_fluxes_allsky and the two-stream ecckd_lw_fluxes_allsky_2stream, on synthetic.columns / synthetic.clouds;
and, with --parent-lib,
  existing ecckd_lw_fluxes, ecckd_lw_fluxes_allsky, ecckd_lw_fluxes_allsky_2stream and the two existing solvers on this build
           and on another build of the library (the parent commit's), in fresh child processes that alternate: their
           min-max ranges must overlap.
HIP-event timing: 3 warm-up calls, then --repeats timed calls per variant, the variants interleaved round-robin; median and
min-max.  Usage: python tools/bench_lw_rescaled.py [--shapes lw_fsck:100000:60,...] [--parent-lib lib.so] [--out f.json]"""
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

DEFAULT_SHAPES = "lw_fsck:100000:60,lw_fsck:1000000:60,lw_fsck:100000:137"
EXISTING = ("existing:lw_fluxes", "existing:lw_fluxes_allsky", "existing:lw_fluxes_allsky_2stream", "existing:rte_lw_1angle",
            "existing:rte_lw_2stream")


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
    plev, tlay, tlev, tsfc = t(cols["plev"]), t(cols["tlay"]), t(cols["tlev"]), t(cols["tsfc"])
    emis = t(np.repeat(cols["sfc_emis"][:, None], nb, 1))
    two = pkg.OpticalProps2str()
    two.tau, two.ssa, two.g = t(cloud["tau"]), t(cloud["ssa"]), t(cloud["g"])
    empty = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    fl = pkg.FluxesBroadband(empty(nlay + 1, ncol), empty(nlay + 1, ncol))

    # the solvers alone, on arrays of the same size
    op = pkg.OpticalProps2str()
    op.alloc_2str(ncol, nlay, k, like=plev)
    src = pkg.SourceFuncLW()
    src.alloc(ncol, nlay, k, like=plev)

    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    op.tau.copy_(10.0 ** (torch.rand(op.tau.shape, generator=gen, device=dev, dtype=torch.float64) * 3.0 - 2.0))
    op.ssa.copy_(torch.rand(op.tau.shape, generator=gen, device=dev, dtype=torch.float64) * 0.999)
    op.g.copy_(torch.rand(op.tau.shape, generator=gen, device=dev, dtype=torch.float64) * 0.9)
    src.lev_source_dec.copy_(3.0 + torch.rand(op.tau.shape, generator=gen, device=dev, dtype=torch.float64))
    src.lev_source_inc.copy_(src.lev_source_dec * 1.01)
    src.lay_source.copy_(src.lev_source_dec * 1.005)
    src.sfc_source.fill_(4.0)

    variants, solvers = {}, {}
    solvers["existing:rte_lw_1angle"] = lambda: check(pkg.rte_lw(op, True, src, emis, fl, n_gauss_angles=1))
    solvers["existing:rte_lw_2stream"] = lambda: check(pkg.rte_lw(op, True, src, emis, fl, use_2stream=True))
    variants["existing:lw_fluxes_allsky_2stream"] = lambda: check(k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gc, True, emis, two, fl,
                                                                                     use_2stream=True))
    variants["existing:lw_fluxes"] = lambda: check(k.lw_fluxes(plev, tlay, tsfc, tlev, gc, True, emis, fl))
    variants["existing:lw_fluxes_allsky"] = lambda: check(k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gc, True, emis, two, fl))
    if not existing_only:
        solvers["solver:rte_lw_rescaled"] = lambda: check(pkg.rte_lw(op, True, src, emis, fl, n_gauss_angles=1, rescaled=True))
        # the fused call and its composed route (gas optics writes into the two-stream container's tau)
        gas = pkg.OpticalProps1scl()
        gas.tau, gas.band2gpt = op.tau, op.band2gpt
        b2g = k.get_band2gpt()

        def composed():
            check(k.gas_optics_tau(plev, tlay, gc, gas))
            op.ssa.zero_()
            op.g.zero_()
            check(k.planck_sources(tlay, tsfc, src, tlev=tlev))
            check(op.increment(two, band2gpt=b2g))
            check(pkg.rte_lw(op, True, src, emis, fl, rescaled=True))
        variants["fused:lw_fluxes_allsky_rescaled"] = lambda: check(k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gc, True, emis, two, fl,
                                                                                       rescaled=True))
        variants["fused:composed_route"] = composed
    # (the solver group first, on its random arrays; the composed route then overwrites the container's tau, ssa and g)
    res = {n: stats(v) for n, v in interleaved(solvers, repeats).items()} if solvers else {}
    res.update({n: stats(v) for n, v in interleaved(variants, repeats).items()})
    print(json.dumps({"kind": kind, "ncol": ncol, "nlay": nlay, "ngpt": ng, "nband": nb, "device": torch.cuda.get_device_name(0),
                      "build": pkg.lib().ecckd_build_info().decode(), "results": res}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=2, help="fresh processes per build and shape, alternating")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-commit", default=None, help="recorded beside the parent's figures")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lw_rescaled.json"))
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
        print("bench_lw_rescaled: %s, %s" % (shape, "another build, existing calls" if lib else "this build"), file=sys.stderr, flush=True)
        r = subprocess.run(cmd + (["--existing-only"] if existing_only else []), env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:   # (a failed child ends the job: nothing more is started on the GPU)
            raise SystemExit("child failed (%s): %s" % (shape, r.stderr[-2000:]))
        return json.loads(r.stdout.strip().splitlines()[-1])

    out = {"timing": "HIP events, 3 warm-up calls, variants interleaved; builds in alternating fresh processes", "repeats": args.repeats,
           "parent_commit": args.parent_commit, "shapes": []}
    for shape in args.shapes.split(","):
        entry = {"shape": shape}
        if args.parent_lib:
            runs = {"parent": [], "branch": []}
            for _ in range(args.rounds):
                for name, lib in (("parent", args.parent_lib), ("branch", None)):
                    runs[name].append(run(shape, lib, True)["results"])
            overlap = {}
            for call in EXISTING:
                lo = {b: min(c[call]["min_ms"] for c in runs[b]) for b in runs}
                hi = {b: max(c[call]["max_ms"] for c in runs[b]) for b in runs}
                med = {b: sorted(c[call]["median_ms"] for c in runs[b])[len(runs[b]) // 2] for b in runs}
                overlap[call] = {"parent_ms": [lo["parent"], hi["parent"]], "branch_ms": [lo["branch"], hi["branch"]],
                                 "parent_median_ms": med["parent"], "branch_median_ms": med["branch"],
                                 "ranges_overlap": lo["parent"] <= hi["branch"] and lo["branch"] <= hi["parent"]}
            entry["existing_calls_min_max"] = overlap
        new = run(shape, None, False)
        entry.update({n: new[n] for n in ("kind", "ncol", "nlay", "ngpt", "device", "build")})
        r = new["results"]
        entry["results"] = r
        sr, fr = r["solver:rte_lw_rescaled"], r["fused:lw_fluxes_allsky_rescaled"]
        f2, fn = r["existing:lw_fluxes_allsky_2stream"], r["existing:lw_fluxes_allsky"]
        entry["ratios"] = {"fused_rescaled_over_noscat_allsky": fr["median_ms"] / fn["median_ms"],
                           "fused_rescaled_over_2stream_allsky": fr["median_ms"] / f2["median_ms"],
                           "fused_rescaled_wholly_below_2stream_allsky": fr["max_ms"] < f2["min_ms"],
                           "fused_over_composed": fr["median_ms"] / r["fused:composed_route"]["median_ms"],
                           "rte_lw_rescaled_over_rte_lw_1angle": sr["median_ms"] / r["existing:rte_lw_1angle"]["median_ms"],
                           "rte_lw_rescaled_over_rte_lw_2stream": sr["median_ms"] / r["existing:rte_lw_2stream"]["median_ms"]}
        out["shapes"].append(entry)
        print(json.dumps({k: v for k, v in entry.items() if k != "results"}), flush=True)
        if args.out:   # (rewritten after every shape: a job cut short keeps what it measured)
            with open(args.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
