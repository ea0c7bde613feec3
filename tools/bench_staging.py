#!/usr/bin/env python3
"""Host-side cost of the C ABI on this build and on another build of the library (the parent commit's), in fresh child
processes that alternate ("Three memory spaces, one code path"):
  bench       python bench.py --steps 10 --warmup 2: ms per step of the device route at the headline size;
  small       the direct-call lines of tools/bench_small_blocks.py: us per step of gas_optics + rte_lw on 1 .. 16384 columns,
              where the host side of a call is what is measured;
  host        one ECCKD_HOST call each of lw_fluxes and rte_sw at 100000 x 60 (numpy arrays in, fluxes out; wall clock,
              1 warm-up call, then --repeats timed calls): the PCIe-bound route;
  device      lw_fluxes and sw_fluxes_allsky on device arrays at 64 x 60: us per call over 200 calls back to back, where the
              host side of a fused call is what is measured.
Acceptance is the project's rule: the min-max ranges of the two builds overlap at every point.  A child that fails ends the
run.  Usage: python tools/bench_staging.py --parent-lib lib.so [--rounds 3] [--out profiles/staging_refactor.json]"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_child(repeats):
    sys.path.insert(0, ROOT)
    import rte_ecckd_amd as pkg
    from rte_ecckd_amd import synthetic
    ncol, nlay = 100000, 60

    def timed(call):
        out = []
        for i in range(repeats + 1):
            t0 = time.perf_counter()
            msg = call()
            if msg:
                raise SystemExit(msg)
            out.append((time.perf_counter() - t0) * 1e3)
        return out[1:]

    k = pkg.GasOpticsEcckd()
    msg = k.load(os.path.join(ROOT, "data", "ecckd-1.2_lw_ckd-definition_climate_fsck-tol0.0161.nc"), device=0)
    if msg:
        raise SystemExit(msg)
    cols = synthetic.columns(0, ncol, k.get_press_min(), nlay=nlay)
    gc = pkg.GasConcs(synthetic.GAS_ORDER)
    for name in synthetic.GAS_ORDER:
        v = cols[name]
        (gc.set_vmr_column if not np.isscalar(v) and v.ndim == 1 else gc.set_vmr)(name, float(v) if np.isscalar(v) else v)
    fl = pkg.FluxesBroadband(np.empty((nlay + 1, ncol)), np.empty((nlay + 1, ncol)), np.empty((nlay + 1, ncol)))
    emis = np.ascontiguousarray(cols["sfc_emis"][:, None])
    res = {"lw_fluxes": timed(lambda: k.lw_fluxes(cols["plev"], cols["tlay"], cols["tsfc"], cols["tlev"], gc, True, emis, fl))}
    rng = np.random.default_rng(0)
    ng = 32
    op = pkg.OpticalProps2str()
    op.band2gpt = np.array([[1, ng]], dtype=np.int32)
    op.tau, op.ssa, op.g = (rng.uniform(lo, hi, (ng, nlay, ncol)) for lo, hi in ((0, 2), (0, 1), (0, 0.8)))
    mu0, toa, alb = rng.uniform(0.1, 1, ncol), rng.uniform(1, 50, (ng, ncol)), rng.uniform(0.05, 0.4, (ncol, 1))
    res["rte_sw"] = timed(lambda: pkg.rte_sw(op, True, mu0, toa, alb, alb, fl))
    print("HOST_MS " + json.dumps(res), flush=True)
    print("FUSED_US " + json.dumps(fused_device_calls(pkg, synthetic, k, repeats)), flush=True)


def fused_device_calls(pkg, synthetic, k_lw, repeats, ncol=64, nlay=60, calls=200):
    """us per call of lw_fluxes and sw_fluxes_allsky on device arrays at 64 x 60, where the host side of the call shows:
    `calls` calls back to back and one synchronisation, `repeats` times after a warm-up."""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def gases(cols):
        gc = pkg.GasConcs(synthetic.GAS_ORDER)
        for name in synthetic.GAS_ORDER:
            v = cols[name]
            (gc.set_vmr_column if not np.isscalar(v) and v.ndim == 1 else gc.set_vmr)(name, float(v) if np.isscalar(v) else t(v))
        return gc

    def timed(call):
        out = []
        for i in range(repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                msg = call()
                if msg:
                    raise SystemExit(msg)
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e6 / calls)
        return out[1:]

    flux = lambda: torch.empty((nlay + 1, ncol), dtype=torch.float64, device=dev)
    cols = synthetic.columns(0, ncol, k_lw.get_press_min(), nlay=nlay)
    gc = gases(cols)
    plev, tlay, tsfc, tlev = (t(cols[n]) for n in ("plev", "tlay", "tsfc", "tlev"))
    emis = t(cols["sfc_emis"][:, None])
    fl = pkg.FluxesBroadband(flux(), flux())
    res = {"lw_fluxes": timed(lambda: k_lw.lw_fluxes(plev, tlay, tsfc, tlev, gc, True, emis, fl))}
    k = pkg.GasOpticsEcckd()
    msg = k.load(os.path.join(ROOT, "data", "ecckd-1.2_sw_ckd-definition_climate_wide-tol0.05.nc"), device=0)
    if msg:
        raise SystemExit(msg)
    nb = k.get_nband()
    cols = synthetic.columns(0, ncol, k.get_press_min(), nlay=nlay, shortwave=True)
    gc2 = gases(cols)
    cl = synthetic.clouds(0, ncol, nlay, nb)
    part = pkg.OpticalProps2str()
    part.tau, part.ssa, part.g = t(cl["tau"]), t(cl["ssa"]), t(cl["g"])
    plev2, tlay2, mu0 = t(cols["plev"]), t(cols["tlay"]), t(cols["mu0"])
    alb = t(np.repeat(cols["albedo"][:, None], nb, 1))
    fl2 = pkg.FluxesBroadband(flux(), flux(), flux())
    res["sw_fluxes_allsky"] = timed(lambda: k.sw_fluxes_allsky(plev2, tlay2, gc2, True, mu0, alb, alb, part, fl2))
    return res


def run(cmd, lib, timeout):
    env = dict(os.environ)
    env.pop("ECCKD_LIB", None)
    if lib:
        env["ECCKD_LIB"] = os.path.abspath(lib)
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit("%s failed with %d (nothing more is started)\n%s\n%s" % (" ".join(cmd), r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return host_child(args.repeats)
    py = sys.executable
    samples = {}   # point -> build -> list of numbers

    def add(point, build, values):
        samples.setdefault(point, {}).setdefault(build, []).extend(values)

    for _ in range(args.rounds):
        for build, lib in (("parent", args.parent_lib), ("branch", None)):
            if build == "parent" and not lib:
                continue
            out = run([py, "bench.py", "--steps", "10", "--warmup", "2"], lib, 600)
            line = [json.loads(x) for x in out.splitlines() if x.startswith("{")][-1]
            add("bench.py ms_per_step", build, [line["ms_per_step"]])
            for ncol, us in re.findall(r"ncol\s+(\d+): direct calls \(Python mirror\)\s+([0-9.]+) us/step", run([py, "tools/bench_small_blocks.py"], lib, 600)):
                add("small blocks ncol %s us_per_step" % ncol, build, [float(us)])
            out = run([py, os.path.abspath(__file__), "--child", "--repeats", str(args.repeats)], lib, 600)
            for name, ms in json.loads([x for x in out.splitlines() if x.startswith("HOST_MS ")][-1][8:]).items():
                add("host %s 100000x60 ms" % name, build, ms)
            for name, us in json.loads([x for x in out.splitlines() if x.startswith("FUSED_US ")][-1][9:]).items():
                add("device %s 64x60 us_per_call" % name, build, us)
    report = {"rounds": args.rounds, "host_repeats_per_round": args.repeats, "points": {}}
    for point, by in samples.items():
        e = {b: {"min": min(v), "max": max(v), "samples": v} for b, v in by.items()}
        if len(e) == 2:
            e["ranges_overlap"] = e["parent"]["min"] <= e["branch"]["max"] and e["branch"]["min"] <= e["parent"]["max"]
        report["points"][point] = e
        print(point, {b: (round(x["min"], 3), round(x["max"], 3)) if isinstance(x, dict) else x for b, x in e.items()}, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
