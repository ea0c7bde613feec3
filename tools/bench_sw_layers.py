#!/usr/bin/env python3
"""The shortwave against the layer count (synthetic columns, 27 g-points of the shortwave file): rte_sw alone in fp64 and
fp32, the fused sw_fluxes in fp64 and fp32, and the gas_optics + rte_sw pair that sw_fluxes replaces -- which solver a
shape takes (layer-systolic up to 60 layers with "sw_solver" 0, the two-pass kernel otherwise) and what it costs.
Each point: two warm-up calls, then device-synchronised wall time over at least 0.5 s.
Usage: python tools/bench_sw_layers.py [ncol]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rte_ecckd_amd as pkg            # noqa: E402
from rte_ecckd_amd import synthetic    # noqa: E402

SW_FILE = os.path.join(ROOT, "data", "ecckd-1.2_sw_ckd-definition_climate_wide-tol0.05.nc")
NAMES = ["co2", "ch4", "n2o", "o2", "h2o", "o3"]
ncol = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
dev = torch.device("cuda:0")


def timed(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        if n >= 3:
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= 0.5:
                return dt / n


def check(msg):
    assert msg == "", msg


k = pkg.GasOpticsEcckd()
check(k.load(SW_FILE, device=0))
ng, nband = k.get_ngpt(), k.get_nband()
print("shortwave, %d columns x %d g-points, device %s" % (ncol, ng, torch.cuda.get_device_name(0)), flush=True)
for nlay, solver in ((60, 0), (60, 1), (91, 0), (137, 0)):
    cols = synthetic.columns(0, ncol, k.get_press_min(), nlay=nlay, shortwave=True)
    rng = np.random.default_rng(nlay)
    alb_dir, alb_dif = rng.uniform(0.02, 0.6, (ncol, nband)), rng.uniform(0.02, 0.6, (ncol, nband))
    pkg.set_solver_option("sw_solver", solver)
    cells = ncol * nlay * ng
    for dtype in (torch.float64, torch.float32):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype)
        gc = pkg.GasConcs(NAMES)
        for n in NAMES:
            v = cols[n]
            if np.isscalar(v):
                gc.set_vmr(n, float(v))
            elif v.ndim == 1:
                gc.set_vmr_column(n, t(v))
            else:
                gc.set_vmr(n, t(v))
        plev, tlay, mu0, ad, af = t(cols["plev"]), t(cols["tlay"]), t(cols["mu0"]), t(alb_dir), t(alb_dif)
        op = pkg.OpticalProps2str(); op.alloc_2str(ncol, nlay, k, like=torch.zeros(1, dtype=dtype, device=dev))
        toa = torch.empty((ng, ncol), dtype=dtype, device=dev)
        fl = pkg.FluxesBroadband(*(torch.empty((nlay + 1, ncol), dtype=dtype, device=dev) for _ in range(3)))
        prec = "f64" if dtype == torch.float64 else "f32"
        check(k.gas_optics(None, plev, tlay, gc, op, toa))
        rows = [
            ("rte_sw", lambda: check(pkg.rte_sw(op, True, mu0, toa, ad, af, fl))),
            ("sw_fluxes", lambda: check(k.sw_fluxes(plev, tlay, gc, True, mu0, ad, af, fl))),
            ("gas_optics+rte_sw", lambda: (check(k.gas_optics(None, plev, tlay, gc, op, toa)),
                                           check(pkg.rte_sw(op, True, mu0, toa, ad, af, fl)))),
        ]
        for name, fn in rows:
            dt = timed(fn)
            print("nlay %3d  sw_solver %d  %s  %-18s %8.3f ms  %7.0f Mcell/s" % (nlay, solver, prec, name, dt * 1e3, cells / dt / 1e6),
                  flush=True)
        del op, toa, fl, gc
        torch.cuda.empty_cache()
pkg.set_solver_option("sw_solver", 0)
