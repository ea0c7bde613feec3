#!/usr/bin/env python3
"""A/B/A of solver option "gas_tile_sync" ("Address translation") against the parent commit's build, in
fresh child processes that alternate: every round runs each point on the parent's library, on this build with the option
at 0, with the option at 1 and as shipped (the option at its default, -1: per mode).  Points:
  lw_f64_1e6   python bench.py --steps 10 --warmup 2                       (the headline)    kernel gas_lw_fused
  lw_f32_1e6   ... --dtype f32                                                                kernel gas_lw_fused_f32
  lw_f64_1e5   ... --ncol 100000                                                              kernel gas_lw_fused
  sw_f64_1e5   ... --mode sw --ncol 100000                                  (768 threads)     kernel tau
  lw_fluxes    ecckd_lw_fluxes on device arrays at 1e6 columns: the tau-only mode (768 threads) + the fused solver
Per point and variant: ms_per_step and the gas-optics kernel's HIP-event time, every sample, min, max and median.
The rule (decided per point): a setting wins when its whole ms_per_step range lies below the parent's range and its median
is lower by more than twice the parent's own min-max spread of this run; the option at 0 must overlap the parent.
The clocks the device reports (rocm-smi, read only) are sampled idle before the first child and while the first headline
child runs.
Usage: python tools/bench_gas_tile_sync.py (--parent-lib lib.so | --parent-ref HEAD~1) [--rounds 3] [--out profiles/gas_tile_sync.json]
--parent-ref builds the library of that commit from `git archive` in a temporary directory (needs the repository's .git)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = ["bench.py", "--steps", "10", "--warmup", "2"]
POINTS = (("lw_f64_1e6", BENCH, "gas_lw_fused"),
          ("lw_f32_1e6", BENCH + ["--dtype", "f32"], "gas_lw_fused_f32"),
          ("lw_f64_1e5", BENCH + ["--ncol", "100000"], "gas_lw_fused"),
          ("sw_f64_1e5", BENCH + ["--mode", "sw", "--ncol", "100000"], "tau"),
          ("lw_fluxes_f64_1e6", None, "tau"))


def fluxes_child(option, steps=10, warmup=2, ncol=1000000):
    """One JSON line like bench.py's: ms_per_step and per-kernel times of ecckd_lw_fluxes on resident device arrays."""
    sys.path.insert(0, ROOT)
    import torch
    import bench
    import rte_ecckd_amd as pkg
    if option is not None:
        pkg.set_solver_option("gas_tile_sync", option)
    L = pkg.lib()
    dev = torch.device("cuda:0")
    k = pkg.GasOpticsEcckd()
    msg = k.load(bench.LW_FILE, device=0)
    if msg:
        raise SystemExit(msg)
    case = bench.LwCase(pkg, k, ncol, 0, dev, torch.float64, k.get_press_min())
    tsfc, fl, emis = case.percol["tsfc"], case.fl, case.emis
    case.src = None          # (the fused path needs no source arrays)
    torch.cuda.empty_cache()

    def step():
        e = k.lw_fluxes(case.plev, case.tlay, tsfc, case.tlev, case.gc, True, emis, fl, n_gauss_angles=1)
        if e:
            raise SystemExit(e)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    L.ecckd_prof_enable(1)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    L.ecckd_prof_enable(0)
    kern = bench.prof_report(L)
    print(json.dumps({"ms_per_step": ms, "kernels": {n: {"avg_ms": v[0]} for n, v in kern.items()}}), flush=True)


def smi():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--showpower", "--json"], capture_output=True, text=True, timeout=20).stdout
        d = json.loads(out)
        c = d[sorted(d)[0]]
        return {kk: v for kk, v in c.items() if any(s in kk.lower() for s in ("sclk", "mclk", "fclk", "power"))}
    except Exception as e:  # noqa: BLE001
        return {"error": str(e)}


def run(cmd, lib, timeout, sample=None):
    env = dict(os.environ)
    env.pop("ECCKD_LIB", None)
    if lib:
        env["ECCKD_LIB"] = os.path.abspath(lib)
    p = subprocess.Popen(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    stop = []
    if sample is not None:
        def sampler():
            while not stop:
                sample.append(smi())
                time.sleep(1.0)
        th = threading.Thread(target=sampler)
        th.start()
    try:
        out, err = p.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        p.kill()
        p.communicate()
        stop.append(1)
        raise SystemExit("%s ran into its time limit of %d s (nothing more is started)" % (" ".join(cmd), timeout))
    stop.append(1)
    if sample is not None:
        th.join()
    if p.returncode != 0:
        raise SystemExit("%s failed with %d (nothing more is started)\n%s\n%s" % (" ".join(cmd), p.returncode, out[-2000:], err[-2000:]))
    return [json.loads(x) for x in out.splitlines() if x.startswith("{")][-1]


def build_parent(ref, tmp):
    subprocess.run("git archive %s | tar -x -C %s" % (ref, tmp), shell=True, check=True, cwd=ROOT)
    subprocess.run([sys.executable, "-c", "import rte_ecckd_amd as p; p.build()"], check=True, cwd=tmp)
    return os.path.join(tmp, "rte-ecckd_amd", "librte_ecckd_hip.so")


def stats(v):
    return {"min": min(v), "max": max(v), "median": statistics.median(v), "samples": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-ref", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--fluxes-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.fluxes_child is not None:
        return fluxes_child(None if args.fluxes_child == "none" else float(args.fluxes_child))
    tmp = None
    if not args.parent_lib:
        if not args.parent_ref:
            raise SystemExit("--parent-lib or --parent-ref is required")
        tmp = tempfile.TemporaryDirectory()
        args.parent_lib = build_parent(args.parent_ref, tmp.name)
    py = sys.executable
    variants = (("parent", args.parent_lib, None), ("option_0", None, 0), ("option_1", None, 1), ("default", None, None))
    ms, kms = {}, {}
    clocks = {"idle": smi(), "loaded": []}
    for r in range(max(args.rounds, 3)):
        for point, cmd, kernel in POINTS:
            for name, lib, opt in variants:
                if cmd is None:
                    c = [py, os.path.abspath(__file__), "--fluxes-child", "none" if opt is None else str(opt)]
                else:
                    c = [py] + cmd + ([] if opt is None else ["--solver-option", "gas_tile_sync=%d" % opt])
                first = r == 0 and point == POINTS[0][0] and name == "parent"
                line = run(c, lib, 600, clocks["loaded"] if first else None)
                ms.setdefault(point, {}).setdefault(name, []).append(line["ms_per_step"])
                kms.setdefault(point, {}).setdefault(name, []).append(line["kernels"][kernel]["avg_ms"])
                if args.out:   # (every sample so far: a run that is cut short still leaves its numbers)
                    with open(args.out + ".partial", "w") as f:
                        json.dump({"ms_per_step": ms, "kernel_ms": kms, "clocks": clocks}, f)
                print("round %d %-18s %-9s %8.3f ms/step  %s %7.3f ms" % (r, point, name, line["ms_per_step"], kernel, line["kernels"][kernel]["avg_ms"]), flush=True)
    clocks["loaded"] = clocks["loaded"][2:-1][:8]
    report = {"rounds": max(args.rounds, 3), "clocks": clocks, "points": {}}
    for point, _, kernel in POINTS:
        e = {n: {"ms_per_step": stats(ms[point][n]), kernel + "_ms": stats(kms[point][n])} for n in ms[point]}
        par = e["parent"]["ms_per_step"]
        spread = par["max"] - par["min"]
        e["parent_spread_ms"] = spread
        for n in ("option_0", "option_1", "default"):
            s = e[n]["ms_per_step"]
            e[n]["overlaps_parent"] = s["min"] <= par["max"] and par["min"] <= s["max"]
            e[n]["wins"] = s["max"] < par["min"] and par["median"] - s["median"] > 2 * spread
            e[n]["median_vs_parent"] = s["median"] / par["median"]
        report["points"][point] = e
        print(point, {n: (round(e[n]["ms_per_step"]["min"], 3), round(e[n]["ms_per_step"]["median"], 3), round(e[n]["ms_per_step"]["max"], 3))
                      for n in ms[point]}, "option_0 overlaps parent:", e["option_0"]["overlaps_parent"], "option_1 wins:", e["option_1"]["wins"],
              "default wins:", e["default"]["wins"], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
        os.remove(args.out + ".partial")
    if tmp:
        tmp.cleanup()


if __name__ == "__main__":
    main()
