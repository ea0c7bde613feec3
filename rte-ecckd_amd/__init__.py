"""rte-ecckd hot path for MI355X -- Python host side.

This package is a thin mirror of the reference's Fortran interface on top of the C ABI in
``include/ecckd_hip.h`` (``librte_ecckd_hip.so``, hand-written HIP for gfx950):

* :class:`GasOpticsEcckd`  <-> ``type(ty_gas_optics_ecckd)`` (src/gas_optics_ecckd.f90:23-48)
  with ``load()`` (= ``load_and_init``, example/rfmip-rad-irf/mo_load_coefficients.F90:19) and
  the generic ``gas_optics()`` (LW: ``gas_optics_int`` :381, SW: ``gas_optics_ext`` :431);
* :class:`GasConcs`, :class:`OpticalProps1scl`, :class:`OpticalProps2str`,
  :class:`SourceFuncLW`, :class:`FluxesBroadband` <-> the RTE-RRTMGP types the reference
  passes around (only the members it touches);
* :class:`CloudOptics` <-> RTE-RRTMGP's ``ty_cloud_optics`` (look-up-table form): water paths and effective
  radii to the particulate properties on the bands, in front of the all-sky calls;
* :class:`AerosolOptics` <-> RTE-RRTMGP's ``ty_aerosol_optics_rrtmgp_merra``: aerosol species, sizes, masses and relative
  humidity to the particulate properties on the bands, several species per call, optionally added onto the clouds;
* :func:`rte_lw`, :func:`rte_sw` <-> RTE-RRTMGP's solvers as called at
  ecckd_rfmip_lw.F90:130-135 and ecckd_rfmip_sw.F90:148-154;
* :func:`heating_rate` <-> RTE-RRTMGP's ``compute_heating_rate``: fluxes and level pressures to the temperature tendency
  in K s-1, the last step of a radiation call.

Error behaviour follows the reference: the entry points return a message string, empty on
success.  Arrays are numpy (host: staged through the GPU by the library) or torch CUDA tensors
(device resident, asynchronous on the current stream); either way C-ordered with the REVERSE
of the Fortran shape, i.e. the reference's column-major memory: ``tau`` is
``(ngpt, nlay, ncol)``, ``plev`` is ``(nlay+1, ncol)``, fluxes are ``(nlay+1, ncol)``.

There is no CPU fallback anywhere in this package: without the HIP library and a GPU every
compute call raises / returns an error.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("ECCKD_LIB", os.path.join(_HERE, "librte_ecckd_hip.so"))   # override: kernel experiments
HOST, DEVICE = 0, 1
MIXED = 2   # host inputs, device-resident spectral arrays (ECCKD_MIXED)
NAME_LEN = 32

_SOURCES = ["kernels_gas_fused.hip", "kernels_gas_roles.hip", "kernels_tau.hip", "kernels_planck.hip", "kernels_rte_lw.hip", "kernels_rte_lw_split.hip",
            "kernels_rte_lw_jac.hip", "kernels_rte_lw_2str.hip",
            "kernels_rte_sw.hip", "kernels_rte_sw_sys.hip", "kernels_rte_gpt.hip", "kernels_optical_props.hip",
            "kernels_cloud_sampling.hip", "kernels_cloud_optics.hip", "kernels_aerosol_optics.hip", "kernels_columns.hip",
            "kernels_heating_rate.hip",
            "capi.cpp", "nc_capi.cpp", "model.cpp", "cdf1.cpp"]
_HEADERS = ["kernels.hpp", "wave_pair.hpp", "gas_fused_body.hpp", "sw_two_stream.hpp", "sw_two_stream_body.inc", "rte_lw_body.inc", "lw_two_stream.hpp", "lw_layer.hpp", "planck_at.hpp", "model.hpp", "cdf1.hpp", os.path.join("..", "..", "include", "ecckd_hip.h"),
            os.path.join("..", "..", "include", "ecckd_nc.h"), os.path.join("..", "..", "include", "rte_kernels_hip.h"),
            os.path.join("..", "..", "include", "rte_kernels_lw_2stream_hip.h")]
# second library: RTE-RRTMGP's kernel-level bind(C) names over the C ABI of the first (include/rte_kernels_hip.h)
RTE_KERNELS_LIB = os.path.join(_HERE, "librte_kernels_hip.so")
_RTE_KERNELS_SRC = "rte_kernels_capi.cpp"
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
               "-ffp-contract=off", "-Wall", "-Wno-unused-function"]


def build(force=False, verbose=False):
    """Compile the HIP library for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = [os.path.join(_CSRC, s) for s in _SOURCES]
    deps = srcs + [os.path.join(_CSRC, h) for h in _HEADERS] + [os.path.join(_CSRC, _RTE_KERNELS_SRC)]
    if not force and os.path.exists(LIB_PATH) and os.path.exists(RTE_KERNELS_LIB):
        t = min(os.path.getmtime(LIB_PATH), os.path.getmtime(RTE_KERNELS_LIB))
        if all(os.path.getmtime(d) <= t for d in deps):
            return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # one object per source (in parallel, recompiled only when the source or a header is newer), then the link
    objdir = os.path.join(_HERE, "build", "obj")
    os.makedirs(objdir, exist_ok=True)
    hdr_t = max(os.path.getmtime(os.path.join(_CSRC, h)) for h in _HEADERS)
    flags = [f for f in HIPCC_FLAGS if f != "-shared"]
    jobs, objs = [], []
    for s in srcs:
        o = os.path.join(objdir, os.path.basename(s).rsplit(".", 1)[0] + ".o")
        objs.append(o)
        if force or not os.path.exists(o) or os.path.getmtime(o) < max(os.path.getmtime(s), hdr_t):
            cmd = [hipcc] + flags + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd))
            jobs.append((cmd, subprocess.Popen(cmd)))
    for cmd, p in jobs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, cmd)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,-rpath,/opt/rocm/lib", "-o", LIB_PATH] + objs
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    cmd = [hipcc, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", RTE_KERNELS_LIB, os.path.join(_CSRC, _RTE_KERNELS_SRC),
           "-L" + _HERE, "-lrte_ecckd_hip", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,/opt/rocm/lib"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB_PATH


FORTRAN_DIR = os.path.join(_HERE, "fortran")
FORTRAN_BUILD = os.path.join(FORTRAN_DIR, "build")
FORTRAN_DRIVER = os.path.join(FORTRAN_BUILD, "ecckd_driver")
RFMIP_LW = os.path.join(FORTRAN_BUILD, "ecckd_rfmip_lw")
RFMIP_SW = os.path.join(FORTRAN_BUILD, "ecckd_rfmip_sw")
CLOUD_DRIVER = os.path.join(FORTRAN_BUILD, "ecckd_cloud_driver")
AEROSOL_DRIVER = os.path.join(FORTRAN_BUILD, "ecckd_aerosol_driver")
HEATING_DRIVER = os.path.join(FORTRAN_BUILD, "ecckd_heating_driver")
BANDS_DRIVER = os.path.join(FORTRAN_BUILD, "ecckd_bands_driver")
SCALING_DRIVER = os.path.join(FORTRAN_BUILD, "ecckd_scaling_driver")
_FORTRAN_MODULES = ["mo_rte_min.F90", "mo_ecckd_device.F90", "gas_optics_ecckd.F90", "mo_rte_solvers.F90", "rfmip_support.F90",
                    "mo_cloud_optics.F90", "mo_aerosol_optics.F90", "mo_heating_rates.F90"]
_FORTRAN_PROGRAMS = [("ecckd_driver", "ecckd_driver.F90", []), ("ecckd_rfmip_lw", "ecckd_rfmip.F90", []),
                     ("ecckd_rfmip_sw", "ecckd_rfmip.F90", ["-DSHORTWAVE"]), ("ecckd_cloud_driver", "ecckd_cloud_driver.F90", []),
                     ("ecckd_aerosol_driver", "ecckd_aerosol_driver.F90", []),
                     ("ecckd_heating_driver", "ecckd_heating_driver.F90", []),
                     ("ecckd_bands_driver", "ecckd_bands_driver.F90", []),
                     ("ecckd_scaling_driver", "ecckd_scaling_driver.F90", [])]


def build_fortran(force=False, verbose=False):
    """Compile the Fortran drop-in module, the solver shims, the RFMIP support modules and the host
    programs (ecckd_driver, ecckd_rfmip_lw, ecckd_rfmip_sw) with amdflang and link them against
    librte_ecckd_hip.so.  Returns the path of ecckd_driver, or None if no Fortran compiler is
    installed (the C ABI and the Python mirror do not need one)."""
    fc = os.environ.get("FC", "/opt/rocm/bin/amdflang")
    if not os.path.exists(fc):
        return None
    srcs = [os.path.join(FORTRAN_DIR, s) for s in _FORTRAN_MODULES + sorted({p[1] for p in _FORTRAN_PROGRAMS})]
    exes = [os.path.join(FORTRAN_BUILD, p[0]) for p in _FORTRAN_PROGRAMS]
    if not force and all(os.path.exists(e) for e in exes):
        t = min(os.path.getmtime(e) for e in exes)
        if all(os.path.getmtime(d) <= t for d in srcs + [LIB_PATH]):
            return FORTRAN_DRIVER
    os.makedirs(FORTRAN_BUILD, exist_ok=True)

    def run(cmd):
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)

    objs = []
    for s in _FORTRAN_MODULES:
        o = os.path.join(FORTRAN_BUILD, s[:-4] + ".o")
        run([fc, "-O2", "-module-dir", FORTRAN_BUILD, "-I" + FORTRAN_BUILD, "-c", os.path.join(FORTRAN_DIR, s), "-o", o])
        objs.append(o)
    for exe, src, flags in _FORTRAN_PROGRAMS:
        o = os.path.join(FORTRAN_BUILD, exe + ".o")
        run([fc, "-O2", "-cpp"] + flags + ["-module-dir", FORTRAN_BUILD, "-I" + FORTRAN_BUILD, "-c",
                                           os.path.join(FORTRAN_DIR, src), "-o", o])
        run([fc, "-o", os.path.join(FORTRAN_BUILD, exe), o] + objs +
            ["-L" + _HERE, "-lrte_ecckd_hip", "-Wl,-rpath,$ORIGIN/../..", "-Wl,-rpath,/opt/rocm/lib"])
    return FORTRAN_DRIVER


_lib = None
_dp = C.POINTER(C.c_double)


def _fused_prototypes():
    """``argtypes`` of the fused flux entry points (a ``_f32`` namesake shares its list), from the pieces every one of them is
    made of: each argument is named, so that the lengths follow from the declarations in include/ecckd_hip.h."""
    ints, ptrs = (lambda *names: [C.c_int] * len(names)), (lambda *names: [C.c_void_p] * len(names))
    gas = ints("ngas") + [C.c_char_p] + ptrs("vmr", "col_stride", "lay_stride", "scalar")
    tail = ints("space") + ptrs("stream")
    lw = ptrs("model") + ints("ncol", "nlay") + ptrs("plev", "tlay", "tsfc", "tlev") + gas
    sw = ptrs("model") + ints("ncol", "nlay") + ptrs("plev", "tlay") + gas
    sw_daylit = ptrs("model") + ints("ncol", "nlay", "nday") + ptrs("day_index", "plev", "tlay") + gas
    lw_bound = ints("top_at_1", "n_gauss_angles") + ptrs("sfc_emis", "inc_flux")
    lw_bound_2stream = ints("top_at_1") + ptrs("sfc_emis", "inc_flux")   # (no quadrature)
    sw_bound = ints("top_at_1") + ptrs("mu0", "toa_scale", "sfc_alb_dir", "sfc_alb_dif")
    lw_part = ints("nband_p") + ptrs("tau_p", "ssa_p")
    lw_part_g = ints("nband_p") + ptrs("tau_p", "ssa_p", "g_p")
    sw_part = ints("nband_p") + ptrs("tau_p", "ssa_p", "g_p") + ints("delta_scale")
    mask = ptrs("cloud_mask")
    lw_out, lw_clear, jac = ptrs("flux_up", "flux_dn"), ptrs("flux_up_clear", "flux_dn_clear"), ptrs("flux_up_jac")
    sw_out, sw_clear = ptrs("flux_up", "flux_dn", "flux_dn_dir"), ptrs("flux_up_clear", "flux_dn_clear", "flux_dn_dir_clear")
    lw_bands, sw_bands = ptrs("bnd_flux_up", "bnd_flux_dn"), ptrs("bnd_flux_up", "bnd_flux_dn", "bnd_flux_dn_dir")
    return {"ecckd_lw_flux_bands": lw + lw_bound + lw_part + mask + lw_bands + lw_out + tail,
            "ecckd_sw_flux_bands": sw + sw_bound + sw_part + mask + sw_bands + sw_out + tail,
            "ecckd_lw_flux_scaled": lw + lw_bound + lw_part + ptrs("cloud_scaling") + lw_out + tail,
            "ecckd_sw_flux_scaled": sw + sw_bound + sw_part + ptrs("cloud_scaling") + sw_out + tail,
            "ecckd_lw_fluxes": lw + lw_bound + lw_out + tail,
            "ecckd_lw_fluxes_allsky": lw + lw_bound + lw_part + lw_out + tail,
            "ecckd_lw_fluxes_allsky_mcica": lw + lw_bound + lw_part + mask + lw_out + tail,
            "ecckd_lw_fluxes_clear_allsky": lw + lw_bound + lw_part + mask + lw_out + lw_clear + tail,
            "ecckd_lw_fluxes_jac": lw + lw_bound + lw_part + mask + lw_out + lw_clear + jac + tail,
            "ecckd_lw_fluxes_allsky_2stream": lw + lw_bound_2stream + lw_part_g + mask + lw_out + tail,
            "ecckd_lw_fluxes_allsky_rescaled": lw + lw_bound + lw_part_g + mask + lw_out + tail,
            "ecckd_lw_fluxes_rescaled_jac": lw + lw_bound + lw_part_g + mask + lw_out + lw_clear + jac + tail,
            "ecckd_sw_fluxes": sw + sw_bound + sw_out + tail,
            "ecckd_sw_fluxes_allsky": sw + sw_bound + sw_part + sw_out + tail,
            "ecckd_sw_fluxes_allsky_mcica": sw + sw_bound + sw_part + mask + sw_out + tail,
            "ecckd_sw_fluxes_clear_allsky": sw + sw_bound + sw_part + mask + sw_out + sw_clear + tail,
            "ecckd_sw_fluxes_daylit": sw_daylit + sw_bound + sw_part + mask + sw_out + sw_clear + tail}


def lib():
    """Load librte_ecckd_hip.so (fails loudly if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("librte_ecckd_hip.so is missing: run `python -c 'import __graft_entry__ as g; "
                           "g.build()'` (there is no CPU fallback)")
    try:  # share torch's HIP runtime when torch is around (it must be loaded first)
        import torch  # noqa: F401
    except Exception:  # pragma: no cover
        pass
    L = C.CDLL(LIB_PATH)
    L.ecckd_last_error.restype = C.c_char_p
    L.ecckd_build_info.restype = C.c_char_p
    for f in ("press_min", "press_max", "temp_min", "temp_max", "total_solar_irradiance"):
        getattr(L, "ecckd_model_get_" + f).restype = C.c_double
        getattr(L, "ecckd_model_get_" + f).argtypes = [C.c_void_p]
    for f in ("ngpt", "nband", "ngas", "device"):
        getattr(L, "ecckd_model_get_" + f).argtypes = [C.c_void_p]
    L.ecckd_model_source_is_internal.argtypes = [C.c_void_p]
    L.ecckd_model_source_is_external.argtypes = [C.c_void_p]
    L.ecckd_model_destroy.argtypes = [C.c_void_p]
    L.ecckd_model_destroy.restype = None
    L.ecckd_model_add_gas.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                      C.c_double, C.c_void_p]
    L.ecckd_planck_sources.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_int, C.c_void_p]
    L.ecckd_gas_optics_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_void_p]
    L.ecckd_gas_optics_plan_ex.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_void_p, C.c_int,
                                           C.c_void_p]
    L.ecckd_set_solver_option.argtypes = [C.c_char_p, C.c_double]
    L.ecckd_get_solver_option.argtypes = [C.c_char_p, C.POINTER(C.c_double)]
    for f in ("ecckd_rte_lw_scratch_bytes", "ecckd_rte_sw_scratch_bytes"):
        getattr(L, f).restype = C.c_size_t
        getattr(L, f).argtypes = [C.c_int, C.c_int, C.c_int]
    L.ecckd_rte_sw_tail_scratch_bytes.restype = C.c_size_t
    L.ecckd_rte_sw_tail_scratch_bytes.argtypes = [C.c_int] * 4
    L.ecckd_rte_lw_tail_scratch_bytes.restype = C.c_size_t
    L.ecckd_rte_lw_tail_scratch_bytes.argtypes = [C.c_int] * 6
    L.ecckd_set_stream_scratch.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    L.ecckd_release_scratch.argtypes = [C.c_int]
    # the fused flux calls, from the named pieces of _fused_prototypes.  (hasattr: ECCKD_LIB may name an older build, which lacks
    # the later ones -- the --parent-lib mode of the tools/bench_*.py scripts; so for the other guards below)
    for name, argtypes in _fused_prototypes().items():
        for f in (name, name + "_f32"):
            if hasattr(L, f):
                getattr(L, f).argtypes = argtypes
    if hasattr(L, "ecckd_cloud_mask_sample"):   # (the McICA calls: 64-bit seed / col0 and the mask pointer need prototypes)
        L.ecckd_cloud_mask_sample.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_void_p, C.c_ulonglong, C.c_longlong, C.c_void_p,
                                                              C.c_int, C.c_void_p]
        for f in ("ecckd_increment_masked", "ecckd_increment_masked_f32"):
            getattr(L, f).argtypes = [C.c_int] * 4 + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
    if hasattr(L, "ecckd_cloud_scaling_sample"):   # (ECCKD_LIB may name an older build, which lacks them)
        L.ecckd_cloud_scaling_create.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
        L.ecckd_cloud_scaling_destroy.argtypes = [C.c_void_p]
        L.ecckd_cloud_scaling_destroy.restype = None
        for f in ("nfsd", "nq"):
            getattr(L, "ecckd_cloud_scaling_get_" + f).argtypes = [C.c_void_p]
        for f in ("fsd0", "dfsd"):
            getattr(L, "ecckd_cloud_scaling_get_" + f).restype = C.c_double
            getattr(L, "ecckd_cloud_scaling_get_" + f).argtypes = [C.c_void_p]
        L.ecckd_cloud_scaling_get_values.argtypes = [C.c_void_p, C.c_void_p]
        L.ecckd_cloud_scaling_lognormal.argtypes = [C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p]
        L.ecckd_cloud_scaling_sample.argtypes = ([C.c_int] * 5 + [C.c_void_p] * 3 + [C.c_double, C.c_void_p, C.c_ulonglong,
                                                                                  C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p])
        for f in ("ecckd_increment_scaled", "ecckd_increment_scaled_f32"):
            getattr(L, f).argtypes = [C.c_int] * 4 + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
        L.ecckd_lw_flux_scaled_scratch_bytes.restype = C.c_size_t
        L.ecckd_lw_flux_scaled_scratch_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.ecckd_sw_flux_scaled_scratch_bytes.restype = C.c_size_t
        L.ecckd_sw_flux_scaled_scratch_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    if hasattr(L, "ecckd_lw_fluxes_f32_scratch_bytes"):   # (an older build lacks them: tools/bench_allsky_f32.py --parent-lib)
        L.ecckd_lw_fluxes_f32_scratch_bytes.restype = C.c_size_t
        L.ecckd_lw_fluxes_f32_scratch_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.ecckd_sw_fluxes_allsky_f32_scratch_bytes.restype = C.c_size_t
        L.ecckd_sw_fluxes_allsky_f32_scratch_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    if hasattr(L, "ecckd_lw_flux_bands_scratch_bytes"):   # (an older build lacks them: tools/bench_flux_bands.py --parent-lib)
        L.ecckd_lw_flux_bands_scratch_bytes.restype = C.c_size_t
        L.ecckd_lw_flux_bands_scratch_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.ecckd_sw_flux_bands_scratch_bytes.restype = C.c_size_t
        L.ecckd_sw_flux_bands_scratch_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    if hasattr(L, "ecckd_daylit_columns"):   # (an older build lacks them: tools/bench_sw_daylit.py times the parent's library)
        for f in ("ecckd_daylit_columns", "ecckd_daylit_columns_f32"):
            getattr(L, f).argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_void_p]
        L.ecckd_gather_columns.argtypes = [C.c_int] * 6 + [C.c_void_p] * 3 + [C.c_int, C.c_void_p]
        L.ecckd_scatter_columns.argtypes = [C.c_int] * 6 + [C.c_void_p] * 3 + [C.c_double, C.c_int, C.c_void_p]
        L.ecckd_sw_fluxes_daylit_scratch_bytes.restype = C.c_size_t
        L.ecckd_sw_fluxes_daylit_scratch_bytes.argtypes = [C.c_void_p] + [C.c_int] * 8
    if hasattr(L, "ecckd_planck_sfc_source_jac"):   # (an older build lacks them: tools/bench_lw_jac.py --parent-lib)
        L.ecckd_planck_sfc_source_jac.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.ecckd_rte_lw_jac.argtypes = [C.c_int] * 6 + [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
    if hasattr(L, "ecckd_rte_lw_2stream"):   # (an older build lacks them: tools/bench_lw_2stream.py --parent-lib)
        L.ecckd_rte_lw_2stream.argtypes = [C.c_int] * 5 + [C.c_void_p] * 7 + [C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
        L.ecckd_lw_solver_2stream_gpt.argtypes = [C.c_int] * 5 + [C.c_void_p] * 11 + [C.c_int, C.c_void_p]
        L.ecckd_rte_lw_2stream_scratch_bytes.restype = C.c_size_t
        L.ecckd_rte_lw_2stream_scratch_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    if hasattr(L, "ecckd_rte_lw_2stream_f32"):   # (an older build lacks them: ECCKD_LIB)
        L.ecckd_rte_lw_2stream_f32.argtypes = L.ecckd_rte_lw_2stream.argtypes
        L.ecckd_lw_fluxes_allsky_2stream_f32_scratch_bytes.restype = C.c_size_t
        L.ecckd_lw_fluxes_allsky_2stream_f32_scratch_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int]
    if hasattr(L, "ecckd_rte_lw_rescaled"):   # (an older build lacks them: tools/bench_lw_rescaled.py --parent-lib)
        L.ecckd_rte_lw_rescaled.argtypes = [C.c_int] * 6 + [C.c_void_p] * 7 + [C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
        L.ecckd_lw_solver_1rescl_gpt.argtypes = [C.c_int] * 6 + [C.c_void_p] * 13 + [C.c_int, C.c_void_p]
        L.ecckd_rte_lw_rescaled_scratch_bytes.restype = C.c_size_t
        L.ecckd_rte_lw_rescaled_scratch_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        L.ecckd_lw_fluxes_allsky_rescaled_scratch_bytes.restype = C.c_size_t
        L.ecckd_lw_fluxes_allsky_rescaled_scratch_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int]
    if hasattr(L, "ecckd_rte_lw_rescaled_jac"):   # (an older build lacks them: tools/bench_lw_rescaled_jac.py --parent-lib)
        L.ecckd_rte_lw_rescaled_jac.argtypes = ([C.c_int] * 6 + [C.c_void_p] * 8 + [C.c_int] + [C.c_void_p] * 6 +
                                                [C.c_int, C.c_void_p])
        L.ecckd_lw_fluxes_rescaled_jac_scratch_bytes.restype = C.c_size_t
        L.ecckd_lw_fluxes_rescaled_jac_scratch_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    if hasattr(L, "ecckd_cloud_optics"):   # (ECCKD_LIB may name an older build, which lacks them)
        L.ecckd_cloud_optics_create_lut.argtypes = [C.c_int] * 4 + [C.c_double] * 4 + [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
        L.ecckd_cloud_optics_destroy.argtypes = [C.c_void_p]
        L.ecckd_cloud_optics_destroy.restype = None
        for f in ("nband", "nrghice"):
            getattr(L, "ecckd_cloud_optics_get_" + f).argtypes = [C.c_void_p]
        for f in ("min_radius_liq", "max_radius_liq", "min_radius_ice", "max_radius_ice"):
            getattr(L, "ecckd_cloud_optics_get_" + f).restype = C.c_double
            getattr(L, "ecckd_cloud_optics_get_" + f).argtypes = [C.c_void_p]
        for f in ("ecckd_cloud_optics", "ecckd_cloud_optics_f32"):
            getattr(L, f).argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p]
    if hasattr(L, "ecckd_aerosol_optics"):   # (ECCKD_LIB may name an older build, which lacks them)
        L.ecckd_aerosol_optics_create_lut.argtypes = [C.c_int] * 3 + [C.c_void_p] * 9 + [C.c_int, C.c_void_p]
        L.ecckd_aerosol_optics_destroy.argtypes = [C.c_void_p]
        L.ecckd_aerosol_optics_destroy.restype = None
        for f in ("nband", "nbin", "nrh"):
            getattr(L, "ecckd_aerosol_optics_get_" + f).argtypes = [C.c_void_p]
        for f in ("ecckd_aerosol_optics", "ecckd_aerosol_optics_f32"):
            getattr(L, f).argtypes = [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p]
    if hasattr(L, "ecckd_heating_rate"):   # (ECCKD_LIB may name an older build, which lacks them)
        for f in ("ecckd_heating_rate", "ecckd_heating_rate_f32"):
            getattr(L, f).argtypes = [C.c_int] * 4 + [C.c_void_p] * 3 + [C.c_double] * 2 + [C.c_void_p] * 2 + [C.c_int, C.c_void_p]
    _lib = L
    return L


def last_error():
    return lib().ecckd_last_error().decode()


FAST, REFERENCE_ORDER = 0, 1


def set_arithmetic(mode):
    """0 = fast (fused kernel, re-associated FMAs; default), 1 = reference expression order
    (bit-faithful kernels); see ecckd_set_arithmetic in include/ecckd_hip.h."""
    if lib().ecckd_set_arithmetic(int(mode)):
        raise ValueError(last_error())


def get_arithmetic():
    return lib().ecckd_get_arithmetic()


SOLVER_OPTIONS = ("lw_tau_thresh", "lw_series_terms", "lw_inc_flux_isotropic", "sw_k_floor", "sw_dir_clamp", "lw_solver",
                  "lw_split_seg", "gas_merge_scalars", "lw_tail_split", "sw_tail_split", "sw_solver", "gas_slab_f32",
                  "gas_tile_sync", "gas_input_ahead", "gas_wave_roles")


def set_solver_option(name, value):
    """Version switches of rte_lw / rte_sw (ecckd_set_solver_option in include/ecckd_hip.h); the defaults
    are the RTE-RRTMGP v1.5-era forms."""
    if lib().ecckd_set_solver_option(name.encode(), float(value)):
        raise ValueError(last_error())


def get_solver_option(name):
    v = C.c_double()
    if lib().ecckd_get_solver_option(name.encode(), C.byref(v)):
        raise ValueError(last_error())
    return v.value


def solver_options():
    """The active switches as a dict (bench.py prints it)."""
    out = {}
    for n in SOLVER_OPTIONS:
        try:
            out[n] = get_solver_option(n)
        except ValueError:   # (ECCKD_LIB names an older build that lacks the option: tools/bench_gas_tile_sync.py)
            if LIB_PATH == os.path.join(_HERE, "librte_ecckd_hip.so"):
                raise
    return out


def reset_solver_options():
    """The version switches back to their (v1.5-era) defaults; the implementation choices (lw_solver, lw_split_seg)
    are left alone."""
    for n, v in (("lw_tau_thresh", 0.0), ("lw_series_terms", 2), ("lw_inc_flux_isotropic", 0), ("sw_k_floor", 1e-12),
                 ("sw_dir_clamp", 0)):
        set_solver_option(n, v)


def rte_sw_scratch_bytes(ncol, nlay, ngpt):
    return int(lib().ecckd_rte_sw_scratch_bytes(int(ncol), int(nlay), int(ngpt)))


def rte_lw_scratch_bytes(ncol, nlay, ngpt):
    return int(lib().ecckd_rte_lw_scratch_bytes(int(ncol), int(nlay), int(ngpt)))


def rte_sw_tail_scratch_bytes(ncol, nlay, ngpt, device=0):
    return int(lib().ecckd_rte_sw_tail_scratch_bytes(int(device), int(ncol), int(nlay), int(ngpt)))


def rte_lw_2stream_scratch_bytes(ncol, nlay, ngpt):
    return int(lib().ecckd_rte_lw_2stream_scratch_bytes(int(ncol), int(nlay), int(ngpt)))


def rte_lw_rescaled_scratch_bytes(ncol, nlay, ngpt):
    return int(lib().ecckd_rte_lw_rescaled_scratch_bytes(int(ncol), int(nlay), int(ngpt)))


def rte_lw_tail_scratch_bytes(ncol, nlay, ngpt, n_gauss_angles=1, single_precision=False, device=0):
    return int(lib().ecckd_rte_lw_tail_scratch_bytes(int(device), int(ncol), int(nlay), int(ngpt), int(n_gauss_angles),
                                                     int(bool(single_precision))))


def set_stream_scratch(buffer, device=None, stream=None):
    """Hand a caller-owned device buffer (a torch CUDA uint8/any tensor, or None to take it back) to the solver
    calls on `stream` (default: torch's current stream) -- ecckd_set_stream_scratch."""
    import torch
    st = torch.cuda.current_stream() if stream is None else stream
    dev = (buffer.device.index if buffer is not None else torch.cuda.current_device()) if device is None else device
    ptr = C.c_void_p(buffer.data_ptr()) if buffer is not None else None
    n = buffer.numel() * buffer.element_size() if buffer is not None else 0
    if lib().ecckd_set_stream_scratch(int(dev or 0), C.c_void_p(st.cuda_stream), ptr, n):
        raise ValueError(last_error())


def release_scratch(device=0):
    if lib().ecckd_release_scratch(int(device)):
        raise RuntimeError(last_error())


# ------------------------------------------------------------------------------------------
# array plumbing: numpy (host) or torch.cuda tensors (device)
# ------------------------------------------------------------------------------------------
_F32, _F64 = np.dtype(np.float32), np.dtype(np.float64)   # (dtype objects: comparing against the scalar types converts them every time)


def _is_torch(a):
    return type(a).__module__.startswith("torch")


def _space_of(arrays):
    dev = host = False
    for a in arrays:
        if a is not None:
            if _is_torch(a) and a.is_cuda:
                dev = True
            else:
                host = True
    if dev and host:
        raise TypeError("mixing host and device arrays in one call")
    return DEVICE if dev else HOST


def _is_f32(a):
    """True for float32 arrays/tensors (the single-precision flavour of the entry points)."""
    if a is None:
        return False
    if _is_torch(a):
        import torch
        return a.dtype == torch.float32
    return isinstance(a, np.ndarray) and a.dtype == _F32


def _call_precision(who, named):
    """Precision of a fused call from its ``(name, array)`` pairs: ``(f32, "")`` with the precision of the first float32 /
    float64 array, or ``(f32, message)`` where a later one has the other precision (it is named).  Arrays of any other
    type are left to the pointer checks."""
    first = None
    for name, a in named:
        if _is_f32(a):
            p = True
        elif a is not None and ((isinstance(a, np.ndarray) and a.dtype == _F64) or str(getattr(a, "dtype", "")).endswith("float64")):
            p = False
        else:
            continue
        if first is None:
            first = (name, p)
        elif p != first[1]:
            kind = lambda x: "float32" if x else "float64"
            return first[1], "%s: mixing float32 and float64 arrays in one call (%s is %s, %s is %s)" % (
                who, first[0], kind(first[1]), name, kind(p))
    return (first[1] if first else False), ""


def _entry(name, f32):
    """The entry point ``name`` in the precision of a call: its ``_f32`` namesake for float32 arrays (``lib()`` gives the two one
    prototype)."""
    return getattr(lib(), name + "_f32" if f32 else name)


def _f64_only(who, what):
    return "%s: %s is implemented for float64 arrays" % (who, what)


def _ptr(a, shape=None, what="array", f32=False):
    """Data pointer of a C-contiguous float64 (or, with f32, float32) array (numpy or torch)."""
    if a is None:
        return None
    want = "float32" if f32 else "float64"
    if _is_torch(a):
        import torch
        if a.dtype != (torch.float32 if f32 else torch.float64) or not a.is_contiguous():
            raise TypeError(what + ": need a contiguous " + want + " tensor")
        if shape is not None and tuple(a.shape) != tuple(shape):
            raise ValueError("%s: shape %s, expected %s" % (what, tuple(a.shape), tuple(shape)))
        return C.c_void_p(a.data_ptr())
    if not isinstance(a, np.ndarray) or a.dtype != (_F32 if f32 else _F64) or not a.flags.c_contiguous:
        raise TypeError(what + ": need a C-contiguous " + want + " ndarray")
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError("%s: shape %s, expected %s" % (what, a.shape, tuple(shape)))
    return C.c_void_p(a.ctypes.data)


def _int32_ptr(a, shape, what):
    """Data pointer of a C-contiguous int32 array (numpy or torch) of the given shape."""
    if _is_torch(a):
        import torch
        if a.dtype != torch.int32 or not a.is_contiguous():
            raise TypeError(what + ": need a contiguous int32 tensor")
        if tuple(a.shape) != tuple(shape):
            raise ValueError("%s: shape %s, expected %s" % (what, tuple(a.shape), tuple(shape)))
        return C.c_void_p(a.data_ptr())
    if not isinstance(a, np.ndarray) or a.dtype != np.int32 or not a.flags.c_contiguous:
        raise TypeError(what + ": need a C-contiguous int32 ndarray")
    if tuple(a.shape) != tuple(shape):
        raise ValueError("%s: shape %s, expected %s" % (what, a.shape, tuple(shape)))
    return C.c_void_p(a.ctypes.data)


def _lev_ptrs(sources, shape, f32=False):
    """Data pointers ``(lev_source_inc, lev_source_dec)`` of a source container for an entry point that takes the level
    buffer (include/ecckd_hip.h): the pair is accepted when it is exactly the two views of one ``(ngpt, nlay+1, ncol)``
    float64 tensor -- the data pointers one plane of columns apart, strides ``((nlay+1)*ncol, ncol, 1)`` -- and anything
    else goes through ``_ptr`` (contiguous arrays only).  A container without ``level_views`` is read by attribute."""
    views = getattr(sources, "level_views", None)
    inc, dec = views() if views is not None else (sources.lev_source_inc, sources.lev_source_dec)
    if inc is not None and dec is not None and not f32 and _is_torch(inc) and _is_torch(dec):
        import torch
        ng, nlay, ncol = shape
        want = ((nlay + 1) * ncol, ncol, 1)
        if (inc.dtype == torch.float64 and dec.dtype == torch.float64 and tuple(inc.shape) == tuple(shape)
                and tuple(dec.shape) == tuple(shape) and tuple(inc.stride()) == want and tuple(dec.stride()) == want
                and inc.data_ptr() - dec.data_ptr() == ncol * 8):
            return C.c_void_p(inc.data_ptr()), C.c_void_p(dec.data_ptr())
    return _ptr(inc, shape, "lev_source_inc", f32), _ptr(dec, shape, "lev_source_dec", f32)


def _stream(space):
    if space == DEVICE:
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return None


def _empty_like_space(shape, like):
    """Uninitialised array in the memory space (and precision, if float32) of `like`."""
    if _is_torch(like):
        import torch
        return torch.empty(shape, dtype=torch.float32 if _is_f32(like) else torch.float64, device=like.device)
    return np.empty(shape, dtype=np.float32 if _is_f32(like) else np.float64)


def _mask_ptr(mask, nlay, ncol, space):
    """Data pointer of a cloud mask ``(nlay, ncol)``: numpy uint64 (host) or a torch int64 device tensor (same bits)."""
    if mask is None:
        return None
    if _is_torch(mask):
        import torch
        if space != DEVICE or not mask.is_cuda:
            raise TypeError("cloud_mask: mixing host and device arrays in one call")
        if mask.dtype != torch.int64 or not mask.is_contiguous():
            raise TypeError("cloud_mask: need a contiguous int64 tensor (the bits of the uint64 words)")
        if tuple(mask.shape) != (nlay, ncol):
            raise ValueError("cloud_mask: shape %s, expected %s" % (tuple(mask.shape), (nlay, ncol)))
        return C.c_void_p(mask.data_ptr())
    if space != HOST:
        raise TypeError("cloud_mask: mixing host and device arrays in one call")
    if not isinstance(mask, np.ndarray) or mask.dtype != np.uint64 or not mask.flags.c_contiguous:
        raise TypeError("cloud_mask: need a C-contiguous uint64 ndarray")
    if mask.shape != (nlay, ncol):
        raise ValueError("cloud_mask: shape %s, expected %s" % (mask.shape, (nlay, ncol)))
    return C.c_void_p(mask.ctypes.data)


_OVERLAP = {"max_ran": 0, "exp_ran": 1}


def sample_cloud_mask(cloud_frac, ngpt, overlap="max_ran", overlap_param=None, seed=0, col0=0, device=0):
    """McICA cloud mask (``ecckd_cloud_mask_sample``; the definition is in include/ecckd_hip.h): ``cloud_frac``
    ``(nlay, ncol)`` float64, ``overlap`` ``"max_ran"`` or ``"exp_ran"`` (then ``overlap_param`` ``(nlay-1, ncol)``),
    ``col0`` the global index of the first column.  numpy arrays give a ``uint64 (nlay, ncol)`` array; torch device tensors
    give an ``int64`` tensor with the same bits, asynchronously on the current stream (``device`` is then the tensor's).
    Bit g of a word set = g-point g sees the layer's cloud.  Raises ValueError with the library's message."""
    nlay, ncol = cloud_frac.shape
    code = _OVERLAP.get(overlap, overlap) if isinstance(overlap, str) else overlap
    if not isinstance(code, int):
        raise ValueError("sample_cloud_mask: unknown overlap %r (one of %s)" % (overlap, sorted(_OVERLAP)))
    try:
        space = _space_of([cloud_frac, overlap_param])
        cf = _ptr(cloud_frac, (nlay, ncol), "cloud_frac")
        al = _ptr(overlap_param, (max(nlay - 1, 0), ncol), "overlap_param")
    except TypeError as e:
        raise ValueError(str(e))
    if space == DEVICE:
        import torch
        mask = torch.empty((nlay, ncol), dtype=torch.int64, device=cloud_frac.device)
        mp, device = C.c_void_p(mask.data_ptr()), _device_of(cloud_frac)
    else:
        mask = np.zeros((nlay, ncol), dtype=np.uint64)
        mp = C.c_void_p(mask.ctypes.data)
    rc = lib().ecckd_cloud_mask_sample(int(device), ncol, nlay, int(ngpt), int(code), cf, al, int(seed) & (2**64 - 1), int(col0),
                                       mp, space, _stream(space))
    if rc:
        raise ValueError(last_error())
    return mask


class _Scaling:
    """A sampled optical-depth scaling in the mask slot of ``GasOpticsEcckd._fused``."""

    def __init__(self, array):
        self.array = array


def _scaling_ptr(scaling, ng, nlay, ncol, space):
    """Data pointer of an optical-depth scaling ``(ngpt, nlay, ncol)`` float32, numpy (host) or device tensor."""
    if scaling is None:
        return None
    if _space_of([scaling]) != space:
        raise TypeError("cloud_scaling: mixing host and device arrays in one call")
    return _ptr(scaling, (ng, nlay, ncol), "cloud_scaling", True)


class CloudScaling:
    """The table of in-cloud water variability (``ecckd_cloud_scaling_create``; include/ecckd_hip.h, "In-cloud water
    variability"): ``values`` ``(nfsd, nq)``, row k the scalings of the ``nq`` equal-probability bins of the in-cloud
    distribution at the fractional standard deviation ``fsd0 + k*dfsd``.  ``device`` -1: a host-only object."""

    def __init__(self):
        self._h = None

    def __del__(self):
        try:
            self.finalize()
        except Exception:
            pass

    def finalize(self):
        if self._h:
            lib().ecckd_cloud_scaling_destroy(self._h)
        self._h = None

    def _need(self):
        if not self._h:
            raise RuntimeError("CloudScaling: no table (from_table or lognormal first)")
        return self._h

    @classmethod
    def from_table(cls, values, fsd0, dfsd, device=0):
        """A table of the host's own (a gamma distribution, for instance).  Raises ValueError with the library's message."""
        v = np.ascontiguousarray(values, dtype=np.float64)
        if v.ndim != 2:
            raise ValueError("CloudScaling.from_table: values must be (nfsd, nq)")
        t = cls()
        h = C.c_void_p()
        rc = lib().ecckd_cloud_scaling_create(int(device), int(v.shape[0]), float(fsd0), float(dfsd), int(v.shape[1]),
                                              C.c_void_p(v.ctypes.data), C.byref(h))
        if rc:
            raise ValueError(last_error())
        t._h = h
        return t

    @staticmethod
    def lognormal_values(nfsd, fsd0, dfsd, nq):
        """``ecckd_cloud_scaling_lognormal``: the ``(nfsd, nq)`` bin means of the unit-mean lognormal distribution (host code)."""
        v = np.zeros((max(int(nfsd), 0), max(int(nq), 0)))
        if lib().ecckd_cloud_scaling_lognormal(int(nfsd), float(fsd0), float(dfsd), int(nq), C.c_void_p(v.ctypes.data)):
            raise ValueError(last_error())
        return v

    @classmethod
    def lognormal(cls, nfsd, fsd0, dfsd, nq, device=0):
        """The table of ``lognormal_values``."""
        return cls.from_table(cls.lognormal_values(nfsd, fsd0, dfsd, nq), fsd0, dfsd, device=device)

    def get_nfsd(self):
        return int(lib().ecckd_cloud_scaling_get_nfsd(self._need()))

    def get_nq(self):
        return int(lib().ecckd_cloud_scaling_get_nq(self._need()))

    def get_fsd0(self):
        return float(lib().ecckd_cloud_scaling_get_fsd0(self._need()))

    def get_dfsd(self):
        return float(lib().ecckd_cloud_scaling_get_dfsd(self._need()))

    def get_values(self):
        v = np.zeros((self.get_nfsd(), self.get_nq()))
        if lib().ecckd_cloud_scaling_get_values(self._need(), C.c_void_p(v.ctypes.data)):
            raise ValueError(last_error())
        return v


def sample_cloud_scaling(cloud_frac, ngpt, table, fsd, overlap="max_ran", overlap_param=None, seed=0, col0=0, device=0,
                         return_mask=False):
    """Sampled optical-depth scaling (``ecckd_cloud_scaling_sample``; the definition is in include/ecckd_hip.h):
    ``cloud_frac`` ``(nlay, ncol)`` float64, ``table`` a ``CloudScaling``, ``fsd`` a ``(nlay, ncol)`` float64 array or one
    number for every cell; ``overlap``, ``overlap_param``, ``seed``, ``col0`` as ``sample_cloud_mask``.  Returns the
    ``(ngpt, nlay, ncol)`` float32 scaling -- numpy for numpy arrays, a device tensor (asynchronously on the current stream)
    for device tensors --, 0 where the g-point does not see the layer's cloud; with ``return_mask`` the pair
    ``(scaling, mask)``, the mask that of ``sample_cloud_mask``.  Raises ValueError with the library's message."""
    nlay, ncol = cloud_frac.shape
    code = _OVERLAP.get(overlap, overlap) if isinstance(overlap, str) else overlap
    if not isinstance(code, int):
        raise ValueError("sample_cloud_scaling: unknown overlap %r (one of %s)" % (overlap, sorted(_OVERLAP)))
    fsd_array = None if np.isscalar(fsd) else fsd
    try:
        space = _space_of([cloud_frac, overlap_param, fsd_array])
        cf = _ptr(cloud_frac, (nlay, ncol), "cloud_frac")
        al = _ptr(overlap_param, (max(nlay - 1, 0), ncol), "overlap_param")
        fp = _ptr(fsd_array, (nlay, ncol), "fsd")
    except TypeError as e:
        raise ValueError(str(e))
    ngpt = int(ngpt)
    shape = (max(ngpt, 0), nlay, ncol)
    mask = None
    if space == DEVICE:
        import torch
        scaling = torch.empty(shape, dtype=torch.float32, device=cloud_frac.device)
        if return_mask:
            mask = torch.empty((nlay, ncol), dtype=torch.int64, device=cloud_frac.device)
        sp, mp, device = C.c_void_p(scaling.data_ptr()), (C.c_void_p(mask.data_ptr()) if return_mask else None), _device_of(cloud_frac)
    else:
        scaling = np.zeros(shape, dtype=np.float32)
        if return_mask:
            mask = np.zeros((nlay, ncol), dtype=np.uint64)
        sp, mp = C.c_void_p(scaling.ctypes.data), (C.c_void_p(mask.ctypes.data) if return_mask else None)
    rc = lib().ecckd_cloud_scaling_sample(int(device), ncol, nlay, ngpt, int(code), cf, al, fp,
                                          0.0 if fsd_array is not None else float(fsd), table._need(),
                                          int(seed) & (2**64 - 1), int(col0), sp, mp, space, _stream(space))
    if rc:
        raise ValueError(last_error())
    return (scaling, mask) if return_mask else scaling


# ------------------------------------------------------------------------------------------
# column compaction: the shortwave on the daylit columns (include/ecckd_hip.h, "The shortwave on the daylit columns only")
# ------------------------------------------------------------------------------------------
def daylit_columns(mu0, mu0_min=0.0, device=0):
    """``ecckd_daylit_columns`` (float32 ``mu0``: ``_f32``): the ascending, 0-based list of the columns with
    ``mu0 > mu0_min`` (compared in double; NaN is night) and their number, ``(index, nday)``.  ``index`` is an int32 array of
    ``nday`` entries where ``mu0`` lives: numpy for numpy, a device tensor for a device tensor (``device`` is then the
    tensor's).  The call synchronises -- ``nday`` is a Python int -- and cannot be captured into a graph; ``sw_fluxes_daylit``
    with the list can.  Raises ValueError with the library's message."""
    f32 = _is_f32(mu0)
    if mu0.ndim != 1:
        raise ValueError("daylit_columns: mu0 must have one dimension (ncol,)")
    ncol = int(mu0.shape[0])
    try:
        space = _space_of([mu0])
        mp = _ptr(mu0, (ncol,), "mu0", f32)
    except TypeError as e:
        raise ValueError(str(e))
    if space == DEVICE:
        import torch
        index = torch.empty((ncol,), dtype=torch.int32, device=mu0.device)
        ip, device = C.c_void_p(index.data_ptr()), _device_of(mu0)
    else:
        index = np.zeros((ncol,), dtype=np.int32)
        ip = C.c_void_p(index.ctypes.data)
    nday = C.c_int(0)
    rc = (lib().ecckd_daylit_columns_f32 if f32 else lib().ecckd_daylit_columns)(
        int(device), ncol, mp, float(mu0_min), ip, C.byref(nday), space, _stream(space))
    if rc:
        raise ValueError(last_error())
    return index[:nday.value], nday.value


def _raw(a, what):
    """(data pointer, element size) of a contiguous array of 4- or 8-byte elements (numpy or torch)."""
    if _is_torch(a):
        if not a.is_contiguous():
            raise TypeError(what + ": need a contiguous tensor")
        size = a.element_size()
        p = C.c_void_p(a.data_ptr())
    else:
        if not isinstance(a, np.ndarray) or not a.flags.c_contiguous:
            raise TypeError(what + ": need a C-contiguous ndarray")
        size = a.dtype.itemsize
        p = C.c_void_p(a.ctypes.data)
    if size not in (4, 8):
        raise TypeError(what + ": need 4- or 8-byte elements")
    return p, size


def _column_view(shape, axis):
    """(ninner, ncol, nouter) of a C-ordered array whose `axis` runs over the columns."""
    axis = axis % len(shape)
    return int(np.prod(shape[axis + 1:], dtype=np.int64)), int(shape[axis]), int(np.prod(shape[:axis], dtype=np.int64)), axis


def gather_columns(src, index, axis=-1, device=0):
    """``ecckd_gather_columns``: ``src`` with its column axis ``axis`` reduced to the columns of ``index`` (an int32 list as
    ``daylit_columns`` returns it), as a new array where ``src`` lives.  Any dtype of 4 or 8 bytes; ``axis = -1`` serves the
    ``(nlay, ncol)`` and ``(n, nlay, ncol)`` arrays, ``axis = 0`` the ``(ncol, nband)`` albedos.  Raises ValueError with the
    library's message."""
    ninner, ncol, nouter, axis = _column_view(src.shape, axis)
    nday = int(index.shape[0])
    try:
        space = _space_of([src, index])
        sp, size = _raw(src, "src")
        ip = _int32_ptr(index, (nday,), "index")
    except TypeError as e:
        raise ValueError(str(e))
    shape = tuple(src.shape[:axis]) + (nday,) + tuple(src.shape[axis + 1:])
    if space == DEVICE:
        import torch
        dst = torch.empty(shape, dtype=src.dtype, device=src.device)
        dp, device = C.c_void_p(dst.data_ptr()), _device_of(src)
    else:
        dst = np.empty(shape, dtype=src.dtype)
        dp = C.c_void_p(dst.ctypes.data)
    if lib().ecckd_gather_columns(int(device), ninner, ncol, nouter, size, nday, ip, sp, dp, space, _stream(space)):
        raise ValueError(last_error())
    return dst


def scatter_columns(src, index, dst, axis=-1, fill=0.0, device=0):
    """``ecckd_scatter_columns``: ``dst[.., index[k], ..] = src[.., k, ..]`` along the column axis ``axis`` and ``fill`` in every
    column of ``dst`` that ``index`` does not list; ``dst`` is written in full, in one pass.  ``index`` must ascend.  Raises
    ValueError with the library's message."""
    ninner, ncol, nouter, axis = _column_view(dst.shape, axis)
    nday = int(index.shape[0])
    want = tuple(dst.shape[:axis]) + (nday,) + tuple(dst.shape[axis + 1:])
    try:
        space = _space_of([src, index, dst])
        sp, size = _raw(src, "src")
        dp, dsize = _raw(dst, "dst")
        ip = _int32_ptr(index, (nday,), "index")
    except TypeError as e:
        raise ValueError(str(e))
    if tuple(src.shape) != want or src.dtype != dst.dtype or size != dsize:
        raise ValueError("scatter_columns: src is %s %s, expected %s %s" % (tuple(src.shape), src.dtype, want, dst.dtype))
    if space == DEVICE:
        device = _device_of(dst)
    if lib().ecckd_scatter_columns(int(device), ninner, ncol, nouter, size, nday, ip, sp, dp, float(fill), space, _stream(space)):
        raise ValueError(last_error())
    return dst


# ------------------------------------------------------------------------------------------
# RTE-RRTMGP data types, as far as the reference touches them
# ------------------------------------------------------------------------------------------
class GasConcs:
    """``ty_gas_concs``: init / set_vmr / get_vmr / get_gas_names / get_num_gases
    (used at src/gas_optics_ecckd.f90:340-351 and mo_rfmip_io.F90:202-259)."""

    def __init__(self, gas_names=()):
        self.init(gas_names)

    def init(self, gas_names):
        names = [n.strip().lower() for n in gas_names]
        if len(set(names)) != len(names):
            return "ty_gas_concs%init: duplicate gas names aren't allowed"
        if any(len(n) == 0 for n in names):
            return "ty_gas_concs%init: must provide non-empty gas names"
        self._names = names
        self._conc = {}
        return ""

    def set_vmr(self, gas, w):
        """w: scalar, profile ``(nlay,)``, or full ``(nlay, ncol)`` [Fortran (ncol,nlay)]."""
        gas = gas.strip().lower()
        if gas not in self._names:
            return "ty_gas_concs%set_vmr: trying to set " + gas + " but name not provided at initialization"
        if np.isscalar(w):
            if w < 0 or w > 1:
                return "ty_gas_concs%set_vmr: concentrations should be >= 0, <= 1"
            self._conc[gas] = float(w)
        else:
            if w.ndim not in (1, 2):
                return "ty_gas_concs%set_vmr: need a scalar, (nlay) or (ncol,nlay) array"
            self._conc[gas] = w
        return ""

    def set_vmr_column(self, gas, w):
        """Extension of the C ABI (per-column value, broadcast over layers)."""
        gas = gas.strip().lower()
        if gas not in self._names:
            return "ty_gas_concs%set_vmr: trying to set " + gas + " but name not provided at initialization"
        self._conc[gas] = ("column", w)
        return ""

    def get_num_gases(self):
        return len(self._names)

    def get_gas_names(self):
        return list(self._names)

    def entries(self, ncol, nlay, known=None):
        """[(name, array-or-None, col_stride, lay_stride, scalar)] in gas order; raises KeyError
        with the ty_gas_concs%get_vmr message for a gas that was never set.  `known`: gas names of the
        k-distribution -- like the reference (src/gas_optics_ecckd.f90:348-364), get_vmr is only
        consulted for gases the model holds a table for; the others cross the boundary as a name with
        a null pointer (nothing is staged for them, and an unset one is not an error)."""
        out = []
        for n in self._names:
            if known is not None and n not in known:
                out.append((n, None, 0, 0, 0.0))
                continue
            if n not in self._conc:
                raise KeyError("ty_gas_concs%get_vmr; gas " + n + " not found")
            w = self._conc[n]
            if isinstance(w, float):
                out.append((n, None, 0, 0, w))
            elif isinstance(w, tuple):
                if tuple(w[1].shape) != (ncol,):
                    raise KeyError("ty_gas_concs%get_vmr; gas " + n + " array is inconsistent with ncol")
                out.append((n, w[1], 1, 0, 0.0))
            elif w.ndim == 1:
                if w.shape[0] != nlay:
                    raise KeyError("ty_gas_concs%get_vmr; gas " + n + " array is inconsistent with nlay")
                out.append((n, w, 0, 1, 0.0))
            else:
                if tuple(w.shape) != (nlay, ncol):
                    raise KeyError("ty_gas_concs%get_vmr; gas " + n + " array is inconsistent with ncol/nlay")
                out.append((n, w, 1, ncol, 0.0))
        return out


class OpticalProps1scl:
    """``ty_optical_props_1scl``: tau(ncol,nlay,ngpt) (+ band structure of the parent)."""

    def __init__(self):
        self.tau = None
        self.band2gpt = None

    def alloc_1scl(self, ncol, nlay, spectral_desc, like=None):
        self.band2gpt = spectral_desc.get_band2gpt()
        ng = spectral_desc.get_ngpt()
        self.tau = _empty_like_space((ng, nlay, ncol), like if like is not None else np.empty(0))
        return ""

    def alloc_1scl_bands(self, ncol, nlay, spectral_desc, like=None):
        """One-stream properties on the BANDS of ``spectral_desc``: a ``(nband, nlay, ncol)`` array (longwave aerosol
        optics as a host model carries them)."""
        self.band2gpt = spectral_desc.get_band2gpt()
        nb = spectral_desc.get_nband()
        self.tau = _empty_like_space((nb, nlay, ncol), like if like is not None else np.empty(0))
        return ""

    def get_ngpt(self):
        return self.tau.shape[0]

    def increment(self, other, band2gpt=None, cloud_mask=None):
        """``self += other`` (RTE-RRTMGP's ``op%increment``; ``ecckd_increment`` / ``_f32``): ``other`` one- or
        two-stream, on the same g-points, or -- with ``band2gpt`` ``(nband, 2)``, 1-based inclusive -- on bands
        ``(nband, nlay, ncol)``.  ``cloud_mask`` ``(nlay, ncol)`` (``sample_cloud_mask``; ``ecckd_increment_masked``):
        where bit g of a word is clear, g-point g is incremented as if ``other.tau`` were 0 there.
        Returns the error message ('' = success)."""
        return _increment(self, other, band2gpt, cloud_mask)

    def increment_scaled(self, other, cloud_scaling, band2gpt=None):
        """``ecckd_increment_scaled`` (float32 containers: ``_f32``): ``increment`` by ``other`` with its optical depth
        multiplied, per g-point, by ``cloud_scaling`` ``(ngpt, nlay, ncol)`` float32 (``sample_cloud_scaling``, or the
        host's own); any number of g-points.  Returns the error message ('' = success)."""
        return _increment(self, other, band2gpt, cloud_scaling=cloud_scaling)


class OpticalProps2str(OpticalProps1scl):
    """``ty_optical_props_2str``: tau, ssa, g."""

    def __init__(self):
        super().__init__()
        self.ssa = None
        self.g = None

    def alloc_2str(self, ncol, nlay, spectral_desc, like=None):
        self.alloc_1scl(ncol, nlay, spectral_desc, like)
        self.ssa = _empty_like_space(tuple(self.tau.shape), self.tau)
        self.g = _empty_like_space(tuple(self.tau.shape), self.tau)
        return ""

    def alloc_2str_bands(self, ncol, nlay, spectral_desc, like=None):
        """Two-stream properties on the BANDS of ``spectral_desc``: ``(nband, nlay, ncol)`` arrays (cloud / aerosol
        optics as a host model carries them)."""
        self.band2gpt = spectral_desc.get_band2gpt()
        nb = spectral_desc.get_nband()
        self.tau = _empty_like_space((nb, nlay, ncol), like if like is not None else np.empty(0))
        self.ssa = _empty_like_space(tuple(self.tau.shape), self.tau)
        self.g = _empty_like_space(tuple(self.tau.shape), self.tau)
        return ""

    def delta_scale(self, forward=None):
        """In-place delta scaling (``ecckd_delta_scale`` / ``_f32``) with the forward-scattering fraction ``forward``
        (same shape), or ``g*g``.  Returns the error message ('' = success)."""
        n, nlay, ncol = self.tau.shape
        f32 = _is_f32(self.tau)
        try:
            space = _space_of([self.tau, self.ssa, self.g, forward])
            P = lambda a, what: _ptr(a, (n, nlay, ncol), what, f32)
            args = (P(self.tau, "tau"), P(self.ssa, "ssa"), P(self.g, "g"), P(forward, "forward"))
        except (TypeError, ValueError) as e:
            return str(e)
        rc = (lib().ecckd_delta_scale_f32 if f32 else lib().ecckd_delta_scale)(
            int(_device_of(self.tau)), ncol, nlay, n, *args, space, _stream(space))
        return last_error() if rc else ""


class CloudOptics:
    """``ty_cloud_optics`` (RTE-RRTMGP, extensions/cloud_optics/mo_cloud_optics.F90), look-up-table form, backed by a
    device-resident table handle: liquid / ice water paths (g m-2) and effective radii (microns) per (column, layer) to
    the particulate properties on the bands -- what the all-sky calls take as ``particles``.  The definition is in
    include/ecckd_hip.h (``ecckd_cloud_optics``); parity with RTE-RRTMGP is unpinned.  The Pade form is not provided."""

    def __init__(self):
        self._h = C.c_void_p(None)
        self._icergh = 1
        self._device = -1

    def __del__(self):
        try:
            self.finalize()
        except Exception:
            pass

    def finalize(self):
        if self._h:
            lib().ecckd_cloud_optics_destroy(self._h)
            self._h = C.c_void_p(None)

    def load_lut(self, band_lims_wvn, radliq_lwr, radliq_upr, radliq_fac, radice_lwr, radice_upr, radice_fac,
                 lut_extliq, lut_ssaliq, lut_asyliq, lut_extice, lut_ssaice, lut_asyice, device=0):
        """``load`` (LUT form) with RTE-RRTMGP's argument list.  Host tables, numpy float64: liquid ``(nband, nsize_liq)``,
        ice ``(nrghice, nband, nsize_ice)`` (the reversed Fortran shapes).  ``band_lims_wvn`` ``(nband, 2)`` or None gives
        nothing but the band count; ``radliq_fac`` / ``radice_fac`` are accepted and unused, as the LUT form of RTE-RRTMGP
        leaves them.  ``device`` -1 makes a host-only object.  Returns the error message ('' = success)."""
        self.finalize()
        tabs = (lut_extliq, lut_ssaliq, lut_asyliq, lut_extice, lut_ssaice, lut_asyice)
        for t in tabs:
            if not isinstance(t, np.ndarray) or t.dtype != np.float64 or not t.flags.c_contiguous:
                return "cloud_optics%init(): the tables are C-contiguous float64 ndarrays on the host"
        if lut_extliq.ndim != 2 or lut_extice.ndim != 3:
            return "cloud_optics%init(): liquid tables are (nband, nsize_liq), ice tables (nrghice, nband, nsize_ice)"
        if any(t.shape != lut_extliq.shape for t in tabs[:3]) or any(t.shape != lut_extice.shape for t in tabs[3:]):
            return "cloud_optics%init(): arrays sized inconsistently"
        nband, nsize_liq = lut_extliq.shape
        nrghice, nband_ice, nsize_ice = lut_extice.shape
        if nband_ice != nband or (band_lims_wvn is not None and np.shape(band_lims_wvn)[0] != nband):
            return "cloud_optics%init(): arrays sized inconsistently"
        h = C.c_void_p(None)
        if lib().ecckd_cloud_optics_create_lut(nband, nsize_liq, nsize_ice, nrghice, float(radliq_lwr), float(radliq_upr),
                                               float(radice_lwr), float(radice_upr),
                                               *[C.c_void_p(t.ctypes.data) for t in tabs], int(device), C.byref(h)):
            return last_error()
        self._h, self._icergh, self._device = h, 1, int(device)
        return ""

    def set_ice_roughness(self, icergh):
        """The roughness (1-based) the next calls pass to ``ecckd_cloud_optics``; it is state of this mirror only."""
        if not self._h:
            return "cloud_optics%set_ice_roughness(): can't set before initialization"
        if icergh < 1 or icergh > self.get_num_ice_roughness_types():
            return "cloud_optics%set_ice_roughness(): must be > 0 and <= nrghice"
        self._icergh = int(icergh)
        return ""

    def get_num_ice_roughness_types(self):
        return lib().ecckd_cloud_optics_get_nrghice(self._h) if self._h else 0

    def get_nband(self):
        return lib().ecckd_cloud_optics_get_nband(self._h) if self._h else 0

    def get_min_radius_liq(self):
        return lib().ecckd_cloud_optics_get_min_radius_liq(self._h)

    def get_max_radius_liq(self):
        return lib().ecckd_cloud_optics_get_max_radius_liq(self._h)

    def get_min_radius_ice(self):
        return lib().ecckd_cloud_optics_get_min_radius_ice(self._h)

    def get_max_radius_ice(self):
        return lib().ecckd_cloud_optics_get_max_radius_ice(self._h)

    def cloud_optics(self, clwp, ciwp, reliq, reice, optical_props):
        """``cloud_optics(clwp, ciwp, reliq, reice, optical_props)``: inputs ``(nlay, ncol)``; ``optical_props`` an
        :class:`OpticalProps2str` (tau, ssa, g) or :class:`OpticalProps1scl` (absorption optical depth) made by
        ``alloc_*_bands``, ``(nband, nlay, ncol)``.  numpy arrays (staged), torch device tensors (asynchronous on the
        current stream), or numpy inputs with device planes.  float32 planes take the ``_f32`` call.
        Returns the error message ('' = success)."""
        if not self._h:
            return "cloud_optics%cloud_optics(): the tables have not been loaded"
        op = optical_props
        two = isinstance(op, OpticalProps2str)
        if op.tau is None or op.tau.ndim != 3:
            return "cloud_optics%cloud_optics(): optical properties are not allocated (alloc_1scl_bands / alloc_2str_bands)"
        nband, nlay, ncol = op.tau.shape
        if nband != self.get_nband():
            return ("cloud_optics%cloud_optics(): optical properties have " + str(nband) + " bands, the tables " +
                    str(self.get_nband()))
        f32 = _is_f32(op.tau)
        planes = [op.tau] + ([op.ssa, op.g] if two else [])
        inputs = [clwp, ciwp, reliq, reice]
        try:
            space = _space_of(planes)
            if space == DEVICE and _space_of(inputs) == HOST:
                space = MIXED
            elif _space_of(inputs) != space:
                raise TypeError("mixing host and device arrays in one call")
            ins = [_ptr(a, (nlay, ncol), n, f32) for a, n in zip(inputs, ("clwp", "ciwp", "reliq", "reice"))]
            outs = [_ptr(a, (nband, nlay, ncol), n, f32) for a, n in zip(planes, ("tau", "ssa", "g"))] + [None] * (3 - len(planes))
        except (TypeError, ValueError) as e:
            return str(e)
        st = _stream(DEVICE) if space == DEVICE else None
        rc = (lib().ecckd_cloud_optics_f32 if f32 else lib().ecckd_cloud_optics)(
            self._h, ncol, nlay, *ins, self._icergh, *outs, space, st)
        return last_error() if rc else ""


# aerosol type codes (RTE-RRTMGP's merra_aero_* parameters; ECCKD_AERO_* in include/ecckd_hip.h)
AERO_NONE, AERO_DUST, AERO_SALT, AERO_SULF, AERO_BCAR_RH, AERO_BCAR, AERO_OCAR_RH, AERO_OCAR = range(8)


class AerosolOptics:
    """``ty_aerosol_optics_rrtmgp_merra`` (RTE-RRTMGP, extensions/aerosols/mo_aerosol_optics_rrtmgp_merra.F90), backed by
    a device-resident table handle: aerosol type, size (microns), mass (kg m-2) and relative humidity per (column, layer)
    to the particulate properties on the bands.  Beyond RTE-RRTMGP: several species per call and ``accumulate``.  The
    definition is in include/ecckd_hip.h (``ecckd_aerosol_optics``); parity with RTE-RRTMGP is unpinned."""

    def __init__(self):
        self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.finalize()
        except Exception:
            pass

    def finalize(self):
        if self._h:
            lib().ecckd_aerosol_optics_destroy(self._h)
            self._h = C.c_void_p(None)

    def load(self, band_lims_wvn, merra_aero_bin_lims, aero_rh, aero_dust_tbl, aero_salt_tbl, aero_sulf_tbl, aero_bcar_tbl,
             aero_bcar_rh_tbl, aero_ocar_tbl, aero_ocar_rh_tbl, device=0):
        """``load`` with RTE-RRTMGP's argument list.  Host tables, C-contiguous numpy float64 in the reversed Fortran
        shapes: ``merra_aero_bin_lims`` ``(nbin, 2)``, ``aero_rh`` ``(nrh,)``, dust ``(nband, nbin, 3)``, salt
        ``(nband, nbin, nrh, 3)``, sulf / bcar_rh / ocar_rh ``(nband, nrh, 3)``, bcar / ocar ``(nband, 3)``.
        ``band_lims_wvn`` ``(nband, 2)`` or None gives nothing but the band count.  ``device`` -1 makes a host-only
        object.  Returns the error message ('' = success)."""
        self.finalize()
        tabs = (merra_aero_bin_lims, aero_rh, aero_dust_tbl, aero_salt_tbl, aero_sulf_tbl, aero_bcar_tbl, aero_bcar_rh_tbl,
                aero_ocar_tbl, aero_ocar_rh_tbl)
        for t in tabs:
            if not isinstance(t, np.ndarray) or t.dtype != np.float64 or not t.flags.c_contiguous:
                return "aerosol_optics%load(): the tables are C-contiguous float64 ndarrays on the host"
        if (merra_aero_bin_lims.ndim != 2 or aero_rh.ndim != 1 or aero_dust_tbl.ndim != 3 or aero_salt_tbl.ndim != 4
                or aero_sulf_tbl.ndim != 3 or aero_bcar_tbl.ndim != 2):
            return ("aerosol_optics%load(): bin limits are (nbin, 2), levels (nrh,), dust (nband, nbin, 3), salt "
                    "(nband, nbin, nrh, 3), sulf / bcar_rh / ocar_rh (nband, nrh, 3), bcar / ocar (nband, 3)")
        nbin, nrh, nband = merra_aero_bin_lims.shape[0], aero_rh.shape[0], aero_dust_tbl.shape[0]
        if (merra_aero_bin_lims.shape != (nbin, 2) or aero_dust_tbl.shape != (nband, nbin, 3)
                or aero_salt_tbl.shape != (nband, nbin, nrh, 3)
                or any(t.shape != (nband, nrh, 3) for t in (aero_sulf_tbl, aero_bcar_rh_tbl, aero_ocar_rh_tbl))
                or any(t.shape != (nband, 3) for t in (aero_bcar_tbl, aero_ocar_tbl))
                or (band_lims_wvn is not None and np.shape(band_lims_wvn)[0] != nband)):
            return "aerosol_optics%load(): arrays sized inconsistently"
        h = C.c_void_p(None)
        if lib().ecckd_aerosol_optics_create_lut(nband, nbin, nrh, *[C.c_void_p(t.ctypes.data) for t in tabs], int(device),
                                                 C.byref(h)):
            return last_error()
        self._h = h
        return ""

    def get_nband(self):
        return lib().ecckd_aerosol_optics_get_nband(self._h) if self._h else 0

    def get_nbin(self):
        return lib().ecckd_aerosol_optics_get_nbin(self._h) if self._h else 0

    def get_nrh(self):
        return lib().ecckd_aerosol_optics_get_nrh(self._h) if self._h else 0

    def aerosol_optics(self, aero_type, aero_size, aero_mass, relhum, optical_props, accumulate=False):
        """``aerosol_optics(aero_type, aero_size, aero_mass, relhum, optical_props)``: the species arrays ``(nlay, ncol)``
        (RTE-RRTMGP's call) or ``(nspec, nlay, ncol)``, ``aero_type`` int32; ``relhum`` ``(nlay, ncol)``;
        ``optical_props`` an :class:`OpticalProps2str` (tau, ssa, g) or :class:`OpticalProps1scl` (absorption optical
        depth) on the bands, ``(nband, nlay, ncol)``.  ``accumulate``: add onto what the planes hold (``increment``'s
        arithmetic) instead of overwriting them.  numpy arrays or torch host tensors (staged), torch device tensors
        (asynchronous on the current stream), or host inputs with device planes.  float32 planes take the ``_f32``
        call.  Returns the error message ('' = success)."""
        if not self._h:
            return "aerosol_optics%aerosol_optics(): the tables have not been loaded"
        op = optical_props
        two = isinstance(op, OpticalProps2str)
        if op.tau is None or op.tau.ndim != 3:
            return "aerosol_optics%aerosol_optics(): optical properties are not allocated (alloc_1scl_bands / alloc_2str_bands)"
        nband, nlay, ncol = op.tau.shape
        if nband != self.get_nband():
            return ("aerosol_optics%aerosol_optics(): optical properties have " + str(nband) + " bands, the tables " +
                    str(self.get_nband()))
        if aero_type is None or getattr(aero_type, "ndim", 0) not in (2, 3):
            return "aerosol_optics%aerosol_optics(): aero_type is (nlay, ncol) or (nspec, nlay, ncol)"
        nspec = 1 if aero_type.ndim == 2 else int(aero_type.shape[0])
        shape = (nlay, ncol) if aero_type.ndim == 2 else (nspec, nlay, ncol)
        f32 = _is_f32(op.tau)
        planes = [op.tau] + ([op.ssa, op.g] if two else [])
        inputs = [aero_type, aero_size, aero_mass, relhum]
        try:
            space = _space_of(planes)
            if space == DEVICE and _space_of(inputs) == HOST:
                space = MIXED
            elif _space_of(inputs) != space:
                raise TypeError("mixing host and device arrays in one call")
            ins = [_int32_ptr(aero_type, shape, "aero_type"), _ptr(aero_size, shape, "aero_size", f32),
                   _ptr(aero_mass, shape, "aero_mass", f32), _ptr(relhum, (nlay, ncol), "relhum", f32)]
            outs = [_ptr(a, (nband, nlay, ncol), n, f32) for a, n in zip(planes, ("tau", "ssa", "g"))] + [None] * (3 - len(planes))
        except (TypeError, ValueError) as e:
            return str(e)
        st = _stream(DEVICE) if space == DEVICE else None
        rc = (lib().ecckd_aerosol_optics_f32 if f32 else lib().ecckd_aerosol_optics)(
            self._h, ncol, nlay, nspec, *ins, 1 if accumulate else 0, *outs, space, st)
        return last_error() if rc else ""


class SourceFuncLW:
    """``ty_source_func_lw``: lay_source, lev_source_inc, lev_source_dec, sfc_source, sfc_source_jac.

    An allocated float64 device container holds ONE value per level, as ecCKD produces them
    (src/gas_optics_ecckd.f90:419-424): ``alloc`` makes one tensor ``lev_source`` ``(ngpt, nlay+1, ncol)``, and the two
    level arrays are its views ``lev_source[:, :-1]`` (dec) and ``lev_source[:, 1:]`` (inc) -- the "level buffer" of
    include/ecckd_hip.h.  ``gas_optics`` / ``planck_sources`` then store each level once and ``rte_lw`` reads it once.
    ``level_views()`` returns the two views; the library's own calls go through it.

    Independent level sources (RRTMGP-style: two different values at a level) are assigned as the caller's own arrays,
    or allocated with ``separate_levels=True``.  So that code written for two independent arrays keeps its meaning --
    scaling both in place must not scale a level twice -- READING OR ASSIGNING ``lev_source_inc`` / ``lev_source_dec``
    AS ATTRIBUTES FIRST TURNS THE VIEWS INTO TWO CONTIGUOUS ARRAYS OF THEIR VALUES (``separate_levels()``: one copy, once
    per container, and the buffer is dropped); from then on the container behaves as one allocated with
    ``separate_levels=True``.  Entry points that do not take the level buffer (two-stream, rescaled) do the same."""

    def __init__(self):
        self.lay_source = self.sfc_source = self.sfc_source_jac = None
        self._lev = None                 # the level buffer (ngpt, nlay+1, ncol), or None: two separate arrays
        self._inc = self._dec = None     # the separate arrays (None while the buffer stands)
        self.levels_shared = False   # True after ecckd's gas_optics: one value per level (:419-424)

    def alloc(self, ncol, nlay, spectral_desc, like=None, separate_levels=False):
        ng = spectral_desc.get_ngpt()
        like = like if like is not None else np.empty(0)
        self.lay_source = _empty_like_space((ng, nlay, ncol), like)
        self._lev = self._inc = self._dec = None
        self.levels_shared = False
        # one level buffer: float64 device tensors, and a library that knows the form (ECCKD_LIB may name an older build)
        if (not separate_levels and _is_torch(like) and like.is_cuda and not _is_f32(like)
                and hasattr(lib(), "ecckd_has_level_buffer")):
            self._lev = _empty_like_space((ng, nlay + 1, ncol), like)
        else:
            self._inc = _empty_like_space((ng, nlay, ncol), like)
            self._dec = _empty_like_space((ng, nlay, ncol), like)
        self.sfc_source = _empty_like_space((ng, ncol), like)
        self.sfc_source_jac = _empty_like_space((ng, ncol), like)   # (planck_sfc_source_jac fills it; float64 only)
        return ""

    @property
    def lev_source(self):
        """The level buffer ``(ngpt, nlay+1, ncol)``, or None when the container holds two separate arrays."""
        return self._lev

    def level_views(self):
        """``(lev_source_inc, lev_source_dec)`` as they stand: the two views of the level buffer, or the two arrays."""
        if self._lev is not None:
            return self._lev[:, 1:], self._lev[:, :-1]
        return self._inc, self._dec

    def separate_levels(self):
        """Replace the two views by contiguous copies of their values and drop the buffer (no-op without one)."""
        if self._lev is not None:
            inc, dec = self.level_views()
            self._inc, self._dec = inc.contiguous(), dec.contiguous()
            self._lev = None
        return self

    @property
    def lev_source_inc(self):
        return self.separate_levels()._inc

    @lev_source_inc.setter
    def lev_source_inc(self, a):
        self.separate_levels()._inc = a

    @property
    def lev_source_dec(self):
        return self.separate_levels()._dec

    @lev_source_dec.setter
    def lev_source_dec(self, a):
        self.separate_levels()._dec = a


class FluxesBroadband:
    """``ty_fluxes_broadband``: flux_up, flux_dn (ncol,nlay+1) [+ flux_dn_dir]."""

    def __init__(self, flux_up=None, flux_dn=None, flux_dn_dir=None):
        self.flux_up, self.flux_dn, self.flux_dn_dir = flux_up, flux_dn, flux_dn_dir

    def heating_rate(self, plev, **kw):
        """:func:`heating_rate` of the broadband ``flux_up`` / ``flux_dn`` (the total downward flux): ``(nlay, ncol)``."""
        return heating_rate(self.flux_up, self.flux_dn, plev, **kw)


class FluxesByband(FluxesBroadband):
    """``ty_fluxes_byband``: bnd_flux_up, bnd_flux_dn (nband,nlay+1,ncol in numpy order) [+ bnd_flux_dn_dir],
    and optionally the broadband members of the parent."""

    def __init__(self, bnd_flux_up, bnd_flux_dn, bnd_flux_dn_dir=None, flux_up=None, flux_dn=None, flux_dn_dir=None):
        super().__init__(flux_up, flux_dn, flux_dn_dir)
        self.bnd_flux_up, self.bnd_flux_dn, self.bnd_flux_dn_dir = bnd_flux_up, bnd_flux_dn, bnd_flux_dn_dir

    def bnd_heating_rate(self, plev, **kw):
        """:func:`heating_rate` of the by-band ``bnd_flux_up`` / ``bnd_flux_dn``, one plane per band: ``(nband, nlay, ncol)``
        (``heating_rate`` of the parent serves the broadband members)."""
        return heating_rate(self.bnd_flux_up, self.bnd_flux_dn, plev, **kw)


# ------------------------------------------------------------------------------------------
# argument groups of the fused calls (GasOpticsEcckd._fused).  A group is a tuple of slots in the order of the C argument
# list: an int goes through as it is, ``(name, array, shape)`` becomes the array's data pointer, checked against the shape
# ------------------------------------------------------------------------------------------
_LEV, _LAY, _COL, _BAND, _GPT, _PART, _SPEC, _BANDLEV = range(8)   # (shape: an index into the tuple that _fused makes)


def _lw_groups(plev, tlay, tsfc, tlev, top_at_1, n_gauss_angles, sfc_emis, inc_flux):
    """``head`` and ``boundary`` of a longwave call (``n_gauss_angles`` None: the entry point has no quadrature)."""
    angles = () if n_gauss_angles is None else (int(n_gauss_angles),)
    return {"head": (("plev", plev, _LEV), ("tlay", tlay, _LAY), ("tsfc", tsfc, _COL), ("tlev", tlev, _LEV)),
            "boundary": (int(bool(top_at_1)),) + angles + (("sfc_emis", sfc_emis, _BAND), ("inc_flux", inc_flux, _GPT))}


def _sw_groups(plev, tlay, top_at_1, mu0, toa_scale, sfc_alb_dir, sfc_alb_dif):
    """``head`` and ``boundary`` of a shortwave call."""
    return {"head": (("plev", plev, _LEV), ("tlay", tlay, _LAY)),
            "boundary": (int(bool(top_at_1)), ("mu0", mu0, _COL), ("toa_scale", toa_scale, _COL),
                         ("sfc_alb_dir", sfc_alb_dir, _BAND), ("sfc_alb_dif", sfc_alb_dif, _BAND))}


def _particle_slots(tau, ssa, *g, tau_required=False):
    """``particles``: the band count and the planes of particulate properties on bands (``g`` where the call takes it)."""
    nbp = int(tau.shape[0]) if tau_required or tau is not None else 0
    return (nbp, ("particles.tau", tau, _PART), ("particles.ssa", ssa, _PART)) + tuple(("particles.g", a, _PART) for a in g)


def _flux_slots(fluxes, suffix="", dn_dir=False):
    """``outputs``: the arrays of a fluxes object, ``flux_dn_dir`` where the call takes it."""
    out = (("flux_up" + suffix, fluxes.flux_up, _LEV), ("flux_dn" + suffix, fluxes.flux_dn, _LEV))
    return out + ((("flux_dn_dir" + suffix, fluxes.flux_dn_dir, _LEV),) if dn_dir else ())


_NO_FLUXES = FluxesBroadband()   # (null pointers, where a call may go without its clear-sky fluxes)


def _jac_slot(flux_up_jac):
    return (("flux_up_jac", flux_up_jac, _LEV),)


def _named(*groups):
    """The ``(name, array)`` pairs of groups, for ``_call_precision``."""
    return [s[:2] for g in groups for s in g if type(s) is tuple]


_FUSED_CHECKS = ("gas", "head", "boundary", "particles", "mask", "outputs")


# ------------------------------------------------------------------------------------------
# ty_gas_optics_ecckd
# ------------------------------------------------------------------------------------------
class GasOpticsEcckd:
    """``type(ty_gas_optics_ecckd)`` backed by a device-resident model handle."""

    def __init__(self):
        self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.finalize()
        except Exception:
            pass

    def finalize(self):
        if self._h:
            lib().ecckd_model_destroy(self._h)
            self._h = C.c_void_p(None)

    # -- construction ---------------------------------------------------------------
    def load(self, filename, available_gases=None, device=0):
        """``load_and_init(ecckd, filename, available_gases)``; ``available_gases`` is accepted
        and ignored exactly as in the reference (mo_load_coefficients.F90:19,23)."""
        self.finalize()
        h = C.c_void_p(None)
        if lib().ecckd_model_load(os.fsencode(filename), int(device), C.byref(h)):
            return last_error()
        self._h = h
        return ""

    def init_from_tables(self, log_pressure, temperature, gases, planck=None, solar=None, bands=None,
                         device=0):
        """Fill the public members directly (src/gas_optics_ecckd.f90:24-36).  ``temperature`` is
        ``(nt,np)``, tables ``(nv,nt,np,ng)``; ``planck=(temperature_planck, planck_function(ntp,ng))``;
        ``solar=(solar_irradiance, rayleigh)``; ``bands=(band_lims_wvn(nband,2), band2gpt(nband,2))``;
        ``gases`` = list of dicts(name, code, composite_only, mole_fraction, reference_mole_fraction,
        coefficient)."""
        self.finalize()
        L = lib()
        f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        lp, T = f8(log_pressure), f8(temperature)
        ng = gases[0]["coefficient"].shape[-1]
        h = C.c_void_p(None)
        if L.ecckd_model_begin(ng, lp.shape[0], T.shape[0], _ptr(lp), _ptr(T), C.byref(h)):
            return last_error()
        try:
            if planck is not None:
                tp, pf = f8(planck[0]), f8(planck[1])
                if L.ecckd_model_set_planck(h, tp.shape[0], _ptr(tp), _ptr(pf)):
                    raise RuntimeError(last_error())
            if solar is not None:
                si, ray = f8(solar[0]), f8(solar[1])
                if L.ecckd_model_set_solar(h, _ptr(si), _ptr(ray)):
                    raise RuntimeError(last_error())
            if bands is not None:
                lims = f8(bands[0])
                b2g = np.ascontiguousarray(bands[1], dtype=np.int32)
                if L.ecckd_model_set_bands(h, b2g.shape[0], _ptr(lims), C.c_void_p(b2g.ctypes.data)):
                    raise RuntimeError(last_error())
            for g in gases:
                coef = f8(g["coefficient"])
                mf = g.get("mole_fraction")
                mf = None if mf is None else f8(mf)
                if L.ecckd_model_add_gas(h, g["name"].encode(), int(g["code"]), int(g.get("composite_only", 0)),
                                         coef.shape[0] if coef.ndim == 4 else 1, _ptr(mf),
                                         float(g.get("reference_mole_fraction", 0.0)), _ptr(coef)):
                    raise RuntimeError(last_error())
            if L.ecckd_model_finalize(h, int(device)):
                raise RuntimeError(last_error())
        except RuntimeError as e:
            L.ecckd_model_destroy(h)
            return str(e)
        self._h = h
        return ""

    # -- type-bound getters (src/gas_optics_ecckd.f90:477-553 + parent) -----------------
    def _need(self):
        if not self._h:
            raise RuntimeError("ty_gas_optics_ecckd: not loaded")
        return self._h

    def get_ngpt(self):
        return lib().ecckd_model_get_ngpt(self._need())

    def get_nband(self):
        return lib().ecckd_model_get_nband(self._need())

    def get_ngas(self):
        return lib().ecckd_model_get_ngas(self._need())

    def get_gases(self):
        out = []
        buf = C.create_string_buffer(NAME_LEN)
        for i in range(self.get_ngas()):
            lib().ecckd_model_get_gas_name(self._need(), i, buf)
            out.append(buf.value.decode())
        return out

    def source_is_internal(self):
        return bool(lib().ecckd_model_source_is_internal(self._need()))

    def source_is_external(self):
        return bool(lib().ecckd_model_source_is_external(self._need()))

    def plan(self, ncol, nlay, gas_names, single_precision=False, scalar_gases=()):
        """``ecckd_gas_optics_plan_ex``: how gas_optics would run for this model, gas list and size (works
        without a GPU on a ``device=-1`` model).  ``scalar_gases`` names the gases that would be passed as
        one number (they can share the merged slot).  Returns a dict, or raises RuntimeError with the
        library's message."""
        names = b"".join(n.strip().lower().encode().ljust(NAME_LEN, b" ") for n in gas_names)
        sc = {n.strip().lower() for n in scalar_gases}
        flags = (C.c_int * max(1, len(gas_names)))(*[int(n.strip().lower() in sc) for n in gas_names])
        out = (C.c_int * 10)()
        if lib().ecckd_gas_optics_plan_ex(self._need(), int(ncol), int(nlay), int(bool(single_precision)),
                                          len(gas_names), names, flags, 10, out):
            raise RuntimeError(last_error())
        keys = ("passes", "fused", "planck_fused", "slab_rows", "planck_rows", "col_chunks", "lds_bytes", "g_chunk",
                "slots", "merged")
        return dict(zip(keys, list(out)))

    def get_press_min(self):
        return lib().ecckd_model_get_press_min(self._need())

    def get_press_max(self):
        return lib().ecckd_model_get_press_max(self._need())

    def get_temp_min(self):
        return lib().ecckd_model_get_temp_min(self._need())

    def get_temp_max(self):
        return lib().ecckd_model_get_temp_max(self._need())

    def get_total_solar_irradiance(self):
        return lib().ecckd_model_get_total_solar_irradiance(self._need())

    def get_band2gpt(self):
        b = np.zeros((self.get_nband(), 2), dtype=np.int32)
        lib().ecckd_model_get_band2gpt(self._need(), C.c_void_p(b.ctypes.data))
        return b

    def get_band_lims_wavenumber(self):
        b = np.zeros((self.get_nband(), 2), dtype=np.float64)
        lib().ecckd_model_get_band_lims_wvn(self._need(), C.c_void_p(b.ctypes.data))
        return b

    def get_device(self):
        return lib().ecckd_model_get_device(self._need())

    # -- gas_optics ---------------------------------------------------------------------
    def _gas_args(self, gas_desc, ncol, nlay, space, f32=False):
        ent = gas_desc.entries(ncol, nlay, known=set(self.get_gases()))
        n = len(ent)
        names = b"".join(e[0].encode().ljust(NAME_LEN, b" ") for e in ent)
        keep = []
        ptrs = (C.c_void_p * max(n, 1))()
        for i, e in enumerate(ent):
            if e[1] is None:
                ptrs[i] = None
            else:
                if (_is_torch(e[1]) and e[1].is_cuda) != (space == DEVICE):
                    raise TypeError("gas " + e[0] + ": vmr array is not in the same memory space as the inputs")
                p = _ptr(e[1], what="vmr of " + e[0], f32=f32)
                keep.append(e[1])
                ptrs[i] = p.value
        cs = (C.c_longlong * max(n, 1))(*[e[2] for e in ent])
        ls = (C.c_longlong * max(n, 1))(*[e[3] for e in ent])
        sc = (C.c_double * max(n, 1))(*[e[4] for e in ent])
        return n, names, ptrs, cs, ls, sc, keep

    def gas_optics(self, play, plev, tlay, *args, **kw):
        """Generic ``gas_optics``: ``(play, plev, tlay, tsfc, gas_desc, optical_props, sources,
        col_dry=None, tlev=None)`` -> gas_optics_int; ``(play, plev, tlay, gas_desc, optical_props,
        toa_src, col_dry=None)`` -> gas_optics_ext.  Returns the error message ('' = success)."""
        if len(args) >= 1 and isinstance(args[0], GasConcs):
            return self.gas_optics_ext(play, plev, tlay, *args, **kw)
        return self.gas_optics_int(play, plev, tlay, *args, **kw)

    def gas_optics_int(self, play, plev, tlay, tsfc, gas_desc, optical_props, sources, col_dry=None,
                       tlev=None):
        """float64 arrays -> ecckd_gas_optics_lw; float32 arrays -> ecckd_gas_optics_lw_f32."""
        nlay, ncol = tlay.shape
        ng = self.get_ngpt()
        f32 = _is_f32(plev)
        try:
            space = _space_of([plev, tlay, tsfc, tlev, optical_props.tau, sources.lay_source])
            n, names, ptrs, cs, ls, sc, keep = self._gas_args(gas_desc, ncol, nlay, space, f32)
        except KeyError as e:
            return str(e.args[0])
        fn = lib().ecckd_gas_optics_lw_f32 if f32 else lib().ecckd_gas_optics_lw
        P = lambda a, shape, what: _ptr(a, shape, what, f32)
        rc = fn(self._need(), ncol, nlay, P(plev, (nlay + 1, ncol), "plev"), P(tlay, (nlay, ncol), "tlay"),
                P(tsfc, (ncol,), "tsfc"), P(tlev, (nlay + 1, ncol), "tlev"), n, names, ptrs, cs, ls, sc,
                P(optical_props.tau, (ng, nlay, ncol), "tau"), P(sources.lay_source, (ng, nlay, ncol), "lay_source"),
                *_lev_ptrs(sources, (ng, nlay, ncol), f32),
                P(sources.sfc_source, (ng, ncol), "sfc_source"), space, _stream(space))
        sources.levels_shared = rc == 0 and tlev is not None
        return last_error() if rc else ""

    def planck_sources(self, tlay, tsfc, sources, tlev=None):
        """``ecckd_planck_sources``: the four Planck source arrays alone (device tensors, fp64)."""
        nlay, ncol = tlay.shape
        ng = self.get_ngpt()
        space = _space_of([tlay, tsfc, sources.lay_source])
        rc = lib().ecckd_planck_sources(
            self._need(), ncol, nlay, _ptr(tlay, (nlay, ncol), "tlay"),
            None if tlev is None else _ptr(tlev, (nlay + 1, ncol), "tlev"), _ptr(tsfc, (ncol,), "tsfc"),
            _ptr(sources.lay_source, (ng, nlay, ncol), "lay_source"),
            *((None, None) if tlev is None else _lev_ptrs(sources, (ng, nlay, ncol))),
            _ptr(sources.sfc_source, (ng, ncol), "sfc_source"), space, _stream(space))
        return last_error() if rc else ""

    def planck_sfc_source_jac(self, tsfc, sources):
        """``ecckd_planck_sfc_source_jac``: ``sources.sfc_source_jac`` ``(ngpt, ncol)`` = B(tsfc + 1) - B(tsfc), the
        surface term of the longwave surface-temperature Jacobian (``rte_lw(..., flux_up_jac=)``).  float64; numpy or
        device tensors.  Returns the error message ('' = success)."""
        ncol = int(tsfc.shape[0]) if getattr(tsfc, "ndim", 0) == 1 else -1
        try:
            space = _space_of([tsfc, sources.sfc_source_jac])
            args = (_ptr(tsfc, (ncol,), "tsfc"), _ptr(sources.sfc_source_jac, (self.get_ngpt(), ncol), "sfc_source_jac"))
        except (TypeError, ValueError) as e:
            return str(e)
        if args[0] is None or args[1] is None:
            return "planck_sfc_source_jac: tsfc and sources.sfc_source_jac are required"
        rc = lib().ecckd_planck_sfc_source_jac(self._need(), ncol, *args, space, _stream(space))
        return last_error() if rc else ""

    def _fused(self, fn, f32, returns, gas_desc, head, boundary=(), particles=(), mask=(), outputs=(), columns=None):
        """One call of an entry point that takes ``(model, ncol, nlay[, nday, day_index], head, gases, boundary, particles, mask,
        outputs, space, stream)``.  ``head``, ``boundary``, ``particles`` and ``outputs`` are tuples of slots (``_lw_groups`` and
        its neighbours make them), ``mask`` is ``(cloud_mask,)`` where the entry point takes one, ``columns`` the list of daylit
        columns or a function that gives it.  The memory space comes from the arrays that are marshalled.  ``returns`` names the
        groups that are checked first, in its order, and whose ``TypeError`` / ``ValueError`` is answered with its message; the
        other groups follow in the order of ``_FUSED_CHECKS`` and raise.  A gas that was never set is answered with a message
        everywhere.  Returns the error message ('' = success)."""
        nlay, ncol = head[1][1].shape   # (tlay)
        ng = self.get_ngpt()
        shapes = ((nlay + 1, ncol), (nlay, ncol), (ncol,), (ncol, self.get_nband()), (ng, ncol),
                  (particles[0] if particles else 0, nlay, ncol), (ng, nlay, ncol), (self.get_nband(), nlay + 1, ncol))
        slots = {"head": head, "boundary": boundary, "particles": particles, "outputs": outputs}
        args = {}
        group = returns[0] if returns else _FUSED_CHECKS[0]
        try:
            # (without the mask: _mask_ptr holds it against the space of the others, with a message of its own)
            space = _space_of([s[1] for s in head + boundary + particles + outputs if type(s) is tuple] +
                              [None if callable(columns) else columns])
            for group in returns + _FUSED_CHECKS:
                if group in args:
                    continue
                if group == "gas":
                    args[group] = self._gas_args(gas_desc, ncol, nlay, space, f32)[:6]
                elif group == "mask":
                    args[group] = [_scaling_ptr(m.array, ng, nlay, ncol, space) if isinstance(m, _Scaling)
                                   else _mask_ptr(m, nlay, ncol, space) for m in mask]
                elif group == "columns":
                    index = columns() if callable(columns) else columns
                    nday = int(index.shape[0])
                    args[group] = (nday, _int32_ptr(index, (nday,), "day_index") if nday else None)
                else:
                    args[group] = [s if type(s) is int else _ptr(s[1], shapes[s[2]], s[0], f32) for s in slots[group]]
        except KeyError as e:
            return str(e.args[0])
        except (TypeError, ValueError) as e:
            if group not in returns:
                raise
            return str(e)
        rc = fn(self._need(), ncol, nlay, *args.get("columns", ()), *args["head"], *args["gas"], *args["boundary"],
                *args["particles"], *args["mask"], *args["outputs"], space, _stream(space))
        return last_error() if rc else ""

    def gas_optics_tau(self, plev, tlay, gas_desc, optical_props):
        """``ecckd_gas_optics_lw_tau``: gas_optical_depth alone (tau only), device tensors."""
        return self._fused(lib().ecckd_gas_optics_lw_tau, False, (), gas_desc, (("plev", plev, _LEV), ("tlay", tlay, _LAY)),
                           outputs=(("tau", optical_props.tau, _SPEC),))

    def rte_lw_fused(self, optical_props, top_at_1, tlay, tlev, tsfc, sfc_emis, fluxes, n_gauss_angles=1, inc_flux=None):
        """``ecckd_rte_lw_fused``: rte_lw that recomputes the Planck sources from the temperatures (device tensors)."""
        ng, nlay, ncol = optical_props.tau.shape
        space = _space_of([optical_props.tau, tlay, tlev, tsfc, sfc_emis, inc_flux, fluxes.flux_up, fluxes.flux_dn])
        rc = lib().ecckd_rte_lw_fused(self._need(), ncol, nlay, int(bool(top_at_1)), int(n_gauss_angles),
                                      _ptr(optical_props.tau), _ptr(tlay, (nlay, ncol), "tlay"),
                                      _ptr(tlev, (nlay + 1, ncol), "tlev"), _ptr(tsfc, (ncol,), "tsfc"),
                                      _ptr(sfc_emis, (ncol, self.get_nband()), "sfc_emis"),
                                      _ptr(inc_flux, (ng, ncol), "inc_flux"), _ptr(fluxes.flux_up, (nlay + 1, ncol), "flux_up"),
                                      _ptr(fluxes.flux_dn, (nlay + 1, ncol), "flux_dn"), space, _stream(space))
        return last_error() if rc else ""

    def _lw_fluxes_jac(self, plev, tlay, tsfc, tlev, gas_desc, top_at_1, sfc_emis, particles, fluxes, fluxes_clear,
                       n_gauss_angles, inc_flux, cloud_mask, flux_up_jac):
        """``ecckd_lw_fluxes_jac`` behind ``lw_fluxes`` / ``lw_fluxes_allsky`` / ``lw_fluxes_clear_allsky`` with
        ``flux_up_jac``: shape and dtype errors are answered here and never reach the library."""
        ptau = None if particles is None else particles.tau
        ssa = None if particles is None else getattr(particles, "ssa", None)
        return self._fused(lib().ecckd_lw_fluxes_jac, False, ("gas", "particles", "mask", "outputs", "head", "boundary"), gas_desc,
                           particles=_particle_slots(ptau, ssa), mask=(cloud_mask,),
                           outputs=_flux_slots(fluxes) + _flux_slots(fluxes_clear or _NO_FLUXES, "_clear") + _jac_slot(flux_up_jac),
                           **_lw_groups(plev, tlay, tsfc, tlev, top_at_1, n_gauss_angles, sfc_emis, inc_flux))

    def lw_fluxes(self, plev, tlay, tsfc, tlev, gas_desc, top_at_1, sfc_emis, fluxes, n_gauss_angles=1, inc_flux=None,
                  flux_up_jac=None):
        """``ecckd_lw_fluxes``: gas optics + rte_lw in one call for hosts that only need broadband fluxes (tau in
        library-owned scratch, sources recomputed in the solver); numpy or device tensors.  ``flux_up_jac``
        ``(nlay+1, ncol)`` float64 (``ecckd_lw_fluxes_jac``): receives the derivative of ``flux_up`` with respect to the
        surface temperature, W m-2 K-1; the fluxes are the same bits with and without it.  float32 arrays (all of them)
        take ``ecckd_lw_fluxes_f32``: the fluxes of ``gas_optics`` + ``rte_lw`` on float32 arrays, bit for bit; no
        ``flux_up_jac``."""
        lw, out = _lw_groups(plev, tlay, tsfc, tlev, top_at_1, n_gauss_angles, sfc_emis, inc_flux), _flux_slots(fluxes)
        f32, mixed = _call_precision("lw_fluxes", _named(lw["head"], lw["boundary"], out, _jac_slot(flux_up_jac)))
        if mixed:
            return mixed
        if flux_up_jac is not None:
            if f32:
                return _f64_only("lw_fluxes", "flux_up_jac")
            return self._lw_fluxes_jac(plev, tlay, tsfc, tlev, gas_desc, top_at_1, sfc_emis, None, fluxes, None, n_gauss_angles,
                                       inc_flux, None, flux_up_jac)
        # (returns nothing: a wrong array raises here, where the all-sky calls answer with a message)
        return self._fused(lib().ecckd_lw_fluxes_f32 if f32 else lib().ecckd_lw_fluxes, f32, (), gas_desc, outputs=out, **lw)

    def _lw_fluxes_allsky_2stream(self, plev, tlay, tsfc, tlev, gas_desc, top_at_1, sfc_emis, particles, fluxes, n_gauss_angles,
                                  inc_flux, cloud_mask, flux_up_jac):
        """``ecckd_lw_fluxes_allsky_2stream`` behind ``lw_fluxes_allsky(..., use_2stream=True)``."""
        who = "lw_fluxes_allsky(use_2stream=True): "
        if not isinstance(particles, OpticalProps2str) or particles.g is None:
            return who + "the particles must be two-stream optical properties on the model's bands, with g (alloc_2str_bands)"
        if flux_up_jac is not None:
            return who + "flux_up_jac is not implemented"
        if n_gauss_angles != 1:
            return who + "the two-stream solver has no quadrature (n_gauss_angles must be 1)"
        return self._fused(lib().ecckd_lw_fluxes_allsky_2stream, False, ("gas", "particles", "mask", "head", "boundary", "outputs"),
                           gas_desc, particles=_particle_slots(particles.tau, particles.ssa, particles.g),
                           mask=(cloud_mask,), outputs=_flux_slots(fluxes),
                           **_lw_groups(plev, tlay, tsfc, tlev, top_at_1, None, sfc_emis, inc_flux))

    def _lw_fluxes_allsky_rescaled(self, plev, tlay, tsfc, tlev, gas_desc, top_at_1, sfc_emis, particles, fluxes, n_gauss_angles,
                                   inc_flux, cloud_mask, use_2stream, flux_up_jac):
        """``ecckd_lw_fluxes_allsky_rescaled`` behind ``lw_fluxes_allsky(..., rescaled=True)``."""
        who = "lw_fluxes_allsky(rescaled=True): "
        if use_2stream:
            return who + "rescaled and use_2stream name two different solvers (pass one of them)"
        if not isinstance(particles, OpticalProps2str) or particles.g is None:
            return who + "the particles must be two-stream optical properties on the model's bands, with g (alloc_2str_bands)"
        if flux_up_jac is not None:
            return who + "flux_up_jac is not implemented for this keyword (lw_fluxes_rescaled returns it)"
        if isinstance(fluxes, FluxesByband):
            return who + "per-band fluxes are not implemented (broadband fluxes only)"
        if any(_is_f32(a) for a in (tlay, particles.tau)):
            return who + "implemented for float64 arrays"
        return self._fused(lib().ecckd_lw_fluxes_allsky_rescaled, False, ("gas", "particles", "mask", "head", "boundary", "outputs"),
                           gas_desc, particles=_particle_slots(particles.tau, particles.ssa, particles.g),
                           mask=(cloud_mask,), outputs=_flux_slots(fluxes),
                           **_lw_groups(plev, tlay, tsfc, tlev, top_at_1, n_gauss_angles, sfc_emis, inc_flux))

    def lw_fluxes_allsky(self, plev, tlay, tsfc, tlev, gas_desc, top_at_1, sfc_emis, particles, fluxes, n_gauss_angles=1,
                         inc_flux=None, cloud_mask=None, rescaled=False, use_2stream=False, flux_up_jac=None):
        """``ecckd_lw_fluxes_allsky``: ``lw_fluxes`` with the combined particulate optical properties ``particles`` on
        the model's bands added to the gas optical depth inside the solver: an ``OpticalProps2str``
        (``alloc_2str_bands``; absorption optical depth ``tau*(1 - ssa)``, its ``g`` is ignored) or an
        ``OpticalProps1scl`` (``alloc_1scl_bands``; ``tau`` as it is).  ``particles`` is never written.  float64, fast
        arithmetic mode; numpy or device tensors.  ``cloud_mask`` ``(nlay, ncol)`` (``sample_cloud_mask``;
        ``ecckd_lw_fluxes_allsky_mcica``): a g-point whose bit is clear sees no particles in that layer.
        ``flux_up_jac`` ``(nlay+1, ncol)`` (``ecckd_lw_fluxes_jac``): the surface-temperature Jacobian of the all-sky
        ``flux_up``.  ``use_2stream=True`` (``ecckd_lw_fluxes_allsky_2stream``): the particles scatter -- the two-stream
        longwave solver on (``tau``, ``ssa``, ``g``) of a two-stream ``particles`` object on the bands; no quadrature
        (``n_gauss_angles`` must be 1) and no ``flux_up_jac``; pass both by keyword (``flux_up_jac`` stays the last
        parameter).  ``rescaled=True`` (``ecckd_lw_fluxes_allsky_rescaled``; by keyword): the rescaled no-scattering solver --
        what RTE-RRTMGP's ``rte_lw`` runs on two-stream properties without ``use_2stream``: cloud scattering as an adjustment of
        the no-scattering sweeps, with the quadrature (``n_gauss_angles`` 1..4); a two-stream ``particles`` object with ``g``,
        float64; refused with ``use_2stream=True``, ``flux_up_jac`` (``lw_fluxes_rescaled`` returns it, and the clear sky),
        ``FluxesByband``.  float32 arrays (all of them) take ``ecckd_lw_fluxes_allsky_f32`` / ``_mcica_f32``: the fluxes of
        ``gas_optics`` + ``increment(particles, band2gpt[, cloud_mask])`` + ``rte_lw`` on float32 arrays, bit for bit;
        ``flux_up_jac``, ``rescaled`` and ``use_2stream`` are float64 only.  Returns the error message ('' = success)."""
        who = "lw_fluxes_allsky"
        lw = _lw_groups(plev, tlay, tsfc, tlev, top_at_1, n_gauss_angles, sfc_emis, inc_flux)
        part, out = _particle_slots(particles.tau, getattr(particles, "ssa", None)), _flux_slots(fluxes)
        f32, mixed = _call_precision(who, _named(lw["head"], lw["boundary"], part, out, _jac_slot(flux_up_jac)))
        if f32 or mixed:   # (float64 calls with these keywords keep the messages of their own routes)
            for on, what in ((rescaled, "rescaled=True"), (use_2stream, "use_2stream=True"), (flux_up_jac is not None, "flux_up_jac")):
                if on:
                    return mixed or _f64_only(who, what)
        if mixed:
            return mixed
        if rescaled:
            return self._lw_fluxes_allsky_rescaled(plev, tlay, tsfc, tlev, gas_desc, top_at_1, sfc_emis, particles, fluxes,
                                                   n_gauss_angles, inc_flux, cloud_mask, use_2stream, flux_up_jac)
        if use_2stream:
            return self._lw_fluxes_allsky_2stream(plev, tlay, tsfc, tlev, gas_desc, top_at_1, sfc_emis, particles, fluxes,
                                                  n_gauss_angles, inc_flux, cloud_mask, flux_up_jac)
        if flux_up_jac is not None:
            return self._lw_fluxes_jac(plev, tlay, tsfc, tlev, gas_desc, top_at_1, sfc_emis, particles, fluxes, None,
                                       n_gauss_angles, inc_flux, cloud_mask, flux_up_jac)
        L = lib()
        if f32:
            fn = L.ecckd_lw_fluxes_allsky_f32 if cloud_mask is None else L.ecckd_lw_fluxes_allsky_mcica_f32
        else:
            fn = L.ecckd_lw_fluxes_allsky if cloud_mask is None else L.ecckd_lw_fluxes_allsky_mcica
        # (the inputs and the outputs are not in `returns`: a wrong one raises, a wrong particle plane or mask is a message)
        return self._fused(fn, f32, ("gas", "particles", "mask"), gas_desc, particles=part,
                           mask=() if cloud_mask is None else (cloud_mask,), outputs=out, **lw)

    def lw_fluxes_rescaled(self, plev, tlay, tsfc, tlev, gas_desc, top_at_1, sfc_emis, particles, fluxes, fluxes_clear=None,
                           flux_up_jac=None, n_gauss_angles=1, inc_flux=None, cloud_mask=None):
        """``ecckd_lw_fluxes_rescaled_jac``: ``lw_fluxes_allsky(..., rescaled=True)`` with, from the same gas-optics pass,
        the clear sky -- ``fluxes_clear`` receives what ``lw_fluxes`` writes, bit for bit -- and ``flux_up_jac``
        ``(nlay+1, ncol)``, the surface-temperature Jacobian of the all-sky ``flux_up`` under the rescaled solver, W m-2 K-1
        (the derivative of ``flux_dn``, which is not zero under rescaling, is not returned).  ``fluxes`` holds the bits of
        ``lw_fluxes_allsky(..., rescaled=True)`` whatever else is asked for.  ``particles``: a two-stream object on the model's
        bands with ``g``; float64, fast arithmetic mode; numpy or device tensors.  Returns the error message ('' = success)."""
        who = "lw_fluxes_rescaled: "
        if not isinstance(particles, OpticalProps2str) or particles.g is None:
            return who + "the particles must be two-stream optical properties on the model's bands, with g (alloc_2str_bands)"
        if isinstance(fluxes, FluxesByband) or isinstance(fluxes_clear, FluxesByband):
            return who + "per-band fluxes are not implemented (broadband fluxes only)"
        if any(_is_f32(a) for a in (tlay, particles.tau)):
            return who + "implemented for float64 arrays"
        return self._fused(lib().ecckd_lw_fluxes_rescaled_jac, False, ("gas", "particles", "mask", "head", "boundary", "outputs"),
                           gas_desc, particles=_particle_slots(particles.tau, particles.ssa, particles.g),
                           mask=(cloud_mask,),
                           outputs=_flux_slots(fluxes) + _flux_slots(fluxes_clear or _NO_FLUXES, "_clear") + _jac_slot(flux_up_jac),
                           **_lw_groups(plev, tlay, tsfc, tlev, top_at_1, n_gauss_angles, sfc_emis, inc_flux))

    def lw_fluxes_allsky_2stream(self, plev, tlay, tsfc, tlev, gas_desc, top_at_1, sfc_emis, particles, fluxes, inc_flux=None,
                                 cloud_mask=None):
        """``ecckd_lw_fluxes_allsky_2stream`` or its ``_f32`` namesake: all-sky longwave fluxes with scattering particles, in the
        precision of the arrays.  float64 arrays give the bits of ``lw_fluxes_allsky(..., use_2stream=True)``;
        float32 arrays (all of them) take the single-precision call: the fluxes of ``gas_optics`` + ``increment(particles,
        band2gpt[, cloud_mask])`` on ``(tau, 0, 0)`` + ``rte_lw_2stream`` on float32 arrays, bit for bit.  ``particles``: a
        two-stream object on the model's bands with ``g``; never written.  ``cloud_mask`` ``(nlay, ncol)`` as in
        ``lw_fluxes_allsky``.  Fast arithmetic mode; numpy or device tensors.  Returns the error message ('' = success)."""
        who = "lw_fluxes_allsky_2stream"
        if not isinstance(particles, OpticalProps2str) or particles.g is None:
            return who + ": the particles must be two-stream optical properties on the model's bands, with g (alloc_2str_bands)"
        if isinstance(fluxes, FluxesByband):
            return who + ": per-band fluxes are not implemented (broadband fluxes only)"
        lw = _lw_groups(plev, tlay, tsfc, tlev, top_at_1, None, sfc_emis, inc_flux)
        part, out = _particle_slots(particles.tau, particles.ssa, particles.g), _flux_slots(fluxes)
        f32, mixed = _call_precision(who, _named(lw["head"], lw["boundary"], part, out))
        if mixed:
            return mixed
        return self._fused(_entry("ecckd_lw_fluxes_allsky_2stream", f32), f32, ("gas", "particles", "mask", "head", "boundary", "outputs"),
                           gas_desc, particles=part, mask=(cloud_mask,), outputs=out, **lw)

    def lw_fluxes_allsky_2stream_f32_scratch_bytes(self, ncol, nlay):
        """The stream scratch of ``lw_fluxes_allsky_2stream`` on float32 device tensors (the ``_scratch_bytes`` function of the
        single-precision entry point)."""
        return int(lib().ecckd_lw_fluxes_allsky_2stream_f32_scratch_bytes(self._need(), int(ncol), int(nlay)))

    def lw_fluxes_rescaled_scratch_bytes(self, ncol, nlay, with_clear=False):
        """``ecckd_lw_fluxes_rescaled_jac_scratch_bytes``: the stream scratch of ``lw_fluxes_rescaled`` on device tensors."""
        return int(lib().ecckd_lw_fluxes_rescaled_jac_scratch_bytes(self._need(), int(ncol), int(nlay), int(bool(with_clear))))

    def lw_fluxes_clear_allsky(self, plev, tlay, tsfc, tlev, gas_desc, top_at_1, sfc_emis, particles, fluxes, fluxes_clear,
                               n_gauss_angles=1, inc_flux=None, cloud_mask=None):
        """``ecckd_lw_fluxes_clear_allsky``: one gas-optics pass, then both skies -- ``fluxes_clear`` receives what
        ``lw_fluxes`` writes and ``fluxes`` what ``lw_fluxes_allsky(..., cloud_mask=cloud_mask)`` writes, bit for bit.
        ``particles`` and ``cloud_mask`` as for ``lw_fluxes_allsky``; neither is written.  float64, fast arithmetic mode;
        numpy or device tensors.  float32 arrays (all of them) take ``ecckd_lw_fluxes_clear_allsky_f32``.  Returns the
        error message ('' = success).  With the surface-temperature Jacobian: ``lw_fluxes_clear_allsky_jac`` (float64)."""
        lw = _lw_groups(plev, tlay, tsfc, tlev, top_at_1, n_gauss_angles, sfc_emis, inc_flux)
        part = _particle_slots(particles.tau, getattr(particles, "ssa", None))
        out = _flux_slots(fluxes) + _flux_slots(fluxes_clear, "_clear")
        f32, mixed = _call_precision("lw_fluxes_clear_allsky", _named(lw["head"], lw["boundary"], part, out))
        if mixed:
            return mixed
        # (the inputs are not in `returns`: a wrong one raises, every other wrong array is a message)
        return self._fused(lib().ecckd_lw_fluxes_clear_allsky_f32 if f32 else lib().ecckd_lw_fluxes_clear_allsky, f32,
                           ("gas", "particles", "mask", "outputs"), gas_desc, particles=part, mask=(cloud_mask,),
                           outputs=out, **lw)

    def lw_fluxes_clear_allsky_jac(self, plev, tlay, tsfc, tlev, gas_desc, top_at_1, sfc_emis, particles, fluxes, fluxes_clear,
                                   flux_up_jac, n_gauss_angles=1, inc_flux=None, cloud_mask=None):
        """``lw_fluxes_clear_allsky`` plus ``flux_up_jac`` ``(nlay+1, ncol)`` float64 (``ecckd_lw_fluxes_jac``): the
        surface-temperature Jacobian of the all-sky ``flux_up``.  (A method of its own: the argument list of
        ``lw_fluxes_clear_allsky`` is fixed.)  Every flux array holds the bits ``lw_fluxes_clear_allsky`` writes."""
        if flux_up_jac is None:
            return "lw_fluxes_clear_allsky_jac: flux_up_jac is required"
        if _is_f32(tlay) or _is_f32(flux_up_jac):
            return _f64_only("lw_fluxes_clear_allsky_jac", "flux_up_jac")
        return self._lw_fluxes_jac(plev, tlay, tsfc, tlev, gas_desc, top_at_1, sfc_emis, particles, fluxes, fluxes_clear,
                                   n_gauss_angles, inc_flux, cloud_mask, flux_up_jac)

    def sw_fluxes_clear_allsky(self, plev, tlay, gas_desc, top_at_1, mu0, sfc_alb_dir, sfc_alb_dif, particles, fluxes,
                               fluxes_clear, delta_scale=True, toa_scale=None, cloud_mask=None):
        """``ecckd_sw_fluxes_clear_allsky``: one gas-optics pass, then both skies -- ``fluxes_clear`` receives what
        ``sw_fluxes`` writes and ``fluxes`` what ``sw_fluxes_allsky(..., cloud_mask=cloud_mask)`` writes, bit for bit.
        ``flux_dn_dir`` of either may be None independently of the other.  float64, fast arithmetic mode; numpy or device
        tensors.  float32 arrays (all of them) take ``ecckd_sw_fluxes_clear_allsky_f32``.  Returns the error message
        ('' = success)."""
        sw = _sw_groups(plev, tlay, top_at_1, mu0, toa_scale, sfc_alb_dir, sfc_alb_dif)
        # (tau_required: particles without tau raise here, as they always have)
        part = _particle_slots(particles.tau, particles.ssa, particles.g, tau_required=True)
        out = _flux_slots(fluxes, dn_dir=True) + _flux_slots(fluxes_clear, "_clear", dn_dir=True)
        f32, mixed = _call_precision("sw_fluxes_clear_allsky", _named(sw["head"], sw["boundary"], part, out))
        if mixed:
            return mixed
        # (the inputs are not in `returns`: a wrong one raises, every other wrong array is a message)
        return self._fused(lib().ecckd_sw_fluxes_clear_allsky_f32 if f32 else lib().ecckd_sw_fluxes_clear_allsky, f32,
                           ("mask", "gas", "particles", "outputs"), gas_desc, particles=part + (int(bool(delta_scale)),),
                           mask=(cloud_mask,), outputs=out, **sw)

    def gas_optics_ext(self, play, plev, tlay, gas_desc, optical_props, toa_src, col_dry=None):
        """float64 arrays -> ecckd_gas_optics_sw; float32 arrays -> ecckd_gas_optics_sw_f32."""
        two = isinstance(optical_props, OpticalProps2str)
        f32 = _is_f32(plev)
        return self._fused(lib().ecckd_gas_optics_sw_f32 if f32 else lib().ecckd_gas_optics_sw, f32, (), gas_desc,
                           (("plev", plev, _LEV), ("tlay", tlay, _LAY)),
                           outputs=(("tau", optical_props.tau, _SPEC), ("ssa", optical_props.ssa if two else None, _SPEC),
                                    ("g", optical_props.g if two else None, _SPEC), ("toa_src", toa_src, _GPT)))

    def sw_fluxes_allsky(self, plev, tlay, gas_desc, top_at_1, mu0, sfc_alb_dir, sfc_alb_dif, particles, fluxes,
                         delta_scale=True, toa_scale=None, cloud_mask=None):
        """``ecckd_sw_fluxes_allsky``: ``sw_fluxes`` with the combined particulate optical properties ``particles``
        (an ``OpticalProps2str`` on the model's bands, ``alloc_2str_bands``) added to the gas optics inside the solver;
        ``delta_scale``: the library delta-scales a copy of them (f = g*g) first, ``particles`` is never written.
        float64, fast arithmetic mode.  ``cloud_mask`` ``(nlay, ncol)`` (``sample_cloud_mask``;
        ``ecckd_sw_fluxes_allsky_mcica``): a g-point whose bit is clear sees no particles in that layer.  float32 arrays
        (all of them) take ``ecckd_sw_fluxes_allsky_f32`` / ``_mcica_f32``: the same route in single precision, to rounding
        what ``gas_optics`` + ``delta_scale`` + ``increment`` + ``rte_sw`` give on float32 arrays."""
        sw = _sw_groups(plev, tlay, top_at_1, mu0, toa_scale, sfc_alb_dir, sfc_alb_dif)
        # (tau_required: particles without tau raise here, as they always have)
        part = _particle_slots(particles.tau, particles.ssa, particles.g, tau_required=True)
        out = _flux_slots(fluxes, dn_dir=True)
        f32, mixed = _call_precision("sw_fluxes_allsky", _named(sw["head"], sw["boundary"], part, out))
        if mixed:
            return mixed
        L = lib()
        if f32:
            fn = L.ecckd_sw_fluxes_allsky_f32 if cloud_mask is None else L.ecckd_sw_fluxes_allsky_mcica_f32
        else:
            fn = L.ecckd_sw_fluxes_allsky if cloud_mask is None else L.ecckd_sw_fluxes_allsky_mcica
        # (the inputs and the outputs are not in `returns`: a wrong one raises, a wrong particle plane or mask is a message)
        return self._fused(fn, f32, ("mask", "gas", "particles"), gas_desc, particles=part + (int(bool(delta_scale)),),
                           mask=() if cloud_mask is None else (cloud_mask,), outputs=out, **sw)

    def sw_fluxes(self, plev, tlay, gas_desc, top_at_1, mu0, sfc_alb_dir, sfc_alb_dif, fluxes, toa_scale=None):
        """``ecckd_sw_fluxes`` (float32 arrays: ``_f32``): gas optics + rte_sw in one call for hosts that only need
        broadband fluxes -- the total optical depth alone goes through (library-owned) memory, the solver derives
        ssa, g = 0 and the incoming beam from plev and the model's tables as gas_optics_ext does.  ``toa_scale``
        ``(ncol,)``: the drivers' rescaling of the incoming beam (total solar irradiance), or None.  Any layer count and
        either ``"sw_solver"``; the fast arithmetic mode only.  The solver is the one ``rte_sw`` takes for the same shape,
        so the fluxes equal those of ``gas_optics`` + ``rte_sw`` bit for bit."""
        f32 = _is_f32(plev)   # (from plev alone, where its siblings go through _call_precision)
        # (returns nothing: a wrong array raises here, where the all-sky calls answer with a message)
        return self._fused(lib().ecckd_sw_fluxes_f32 if f32 else lib().ecckd_sw_fluxes, f32, (), gas_desc,
                           outputs=_flux_slots(fluxes, dn_dir=True),
                           **_sw_groups(plev, tlay, top_at_1, mu0, toa_scale, sfc_alb_dir, sfc_alb_dif))

    def _flux_bands(self, who, fn, gas_desc, groups, part, cloud_mask, fluxes, dn_dir):
        """``ecckd_lw_flux_bands`` / ``ecckd_sw_flux_bands`` behind ``lw_fluxes_byband`` / ``sw_fluxes_byband``: every wrong
        array is answered with a message and never reaches the library."""
        if not isinstance(fluxes, FluxesByband):
            return who + ": fluxes must be a FluxesByband (bnd_flux_up and bnd_flux_dn; the broadband members are optional)"
        bands = (("bnd_flux_up", fluxes.bnd_flux_up, _BANDLEV), ("bnd_flux_dn", fluxes.bnd_flux_dn, _BANDLEV))
        if dn_dir:
            bands += (("bnd_flux_dn_dir", fluxes.bnd_flux_dn_dir, _BANDLEV),)
        out = bands + _flux_slots(fluxes, dn_dir=dn_dir)
        f32, mixed = _call_precision(who, _named(groups["head"], groups["boundary"], part, out))
        if mixed:
            return mixed
        if f32:
            return _f64_only(who, "per-band output from the fused path")
        return self._fused(fn, False, ("gas", "particles", "mask", "outputs", "head", "boundary"), gas_desc, particles=part,
                           mask=(cloud_mask,), outputs=out, **groups)

    def lw_fluxes_byband(self, plev, tlay, tsfc, tlev, gas_desc, top_at_1, sfc_emis, fluxes, n_gauss_angles=1, inc_flux=None,
                         particles=None, cloud_mask=None):
        """``ecckd_lw_flux_bands``: ``lw_fluxes`` / ``lw_fluxes_allsky`` with per-band output.  ``fluxes`` is a
        ``FluxesByband``: ``bnd_flux_up`` / ``bnd_flux_dn`` ``(nband, nlay+1, ncol)`` receive, per band of the model, the sum
        over the band's g-points -- bit for bit what ``gas_optics`` + [``increment(particles, band2gpt[, cloud_mask])``] +
        ``rte_lw`` with a ``FluxesByband`` give, without the host owning a per-g-point array; its ``flux_up`` / ``flux_dn``,
        where given, receive the sum of the planes in band order.  ``particles``: None (clear sky), an ``OpticalProps2str``
        (absorption optical depth) or an ``OpticalProps1scl`` on the model's bands; ``cloud_mask`` ``(nlay, ncol)`` with
        particles only.  float64, fast arithmetic mode; numpy or device tensors.  Returns the error message ('' = success)."""
        ptau = None if particles is None else particles.tau
        ssa = None if particles is None else getattr(particles, "ssa", None)
        return self._flux_bands("lw_fluxes_byband", lib().ecckd_lw_flux_bands, gas_desc,
                                _lw_groups(plev, tlay, tsfc, tlev, top_at_1, n_gauss_angles, sfc_emis, inc_flux),
                                _particle_slots(ptau, ssa), cloud_mask, fluxes, False)

    def sw_fluxes_byband(self, plev, tlay, gas_desc, top_at_1, mu0, sfc_alb_dir, sfc_alb_dif, fluxes, particles=None,
                         delta_scale=True, toa_scale=None, cloud_mask=None):
        """``ecckd_sw_flux_bands``: ``sw_fluxes`` / ``sw_fluxes_allsky`` with per-band output.  ``fluxes`` is a
        ``FluxesByband``: ``bnd_flux_up`` / ``bnd_flux_dn`` / ``bnd_flux_dn_dir`` (optional) ``(nband, nlay+1, ncol)``; its
        broadband members, where given, receive the sum of the planes in band order (``flux_dn_dir`` needs
        ``bnd_flux_dn_dir``).  Clear sky without ``toa_scale``: the bits of ``gas_optics`` + ``rte_sw`` with a
        ``FluxesByband``; with ``particles`` (an ``OpticalProps2str`` on the model's bands; ``delta_scale``: a library-owned
        copy is scaled), ``cloud_mask`` or ``toa_scale``: that composition to rounding, as ``sw_fluxes_allsky``.  float64, fast
        arithmetic mode; numpy or device tensors.  Returns the error message ('' = success)."""
        triple = (None, None, None) if particles is None else (particles.tau, getattr(particles, "ssa", None),
                                                                getattr(particles, "g", None))
        return self._flux_bands("sw_fluxes_byband", lib().ecckd_sw_flux_bands, gas_desc,
                                _sw_groups(plev, tlay, top_at_1, mu0, toa_scale, sfc_alb_dir, sfc_alb_dif),
                                _particle_slots(*triple) + (int(bool(delta_scale)),), cloud_mask, fluxes, True)

    def lw_flux_scaled(self, plev, tlay, tsfc, tlev, gas_desc, top_at_1, sfc_emis, particles, fluxes, cloud_scaling,
                       n_gauss_angles=1, inc_flux=None):
        """``ecckd_lw_flux_scaled``: ``lw_fluxes_allsky`` with the particulate optical depth of every (layer, g-point) cell
        multiplied by ``cloud_scaling`` ``(ngpt, nlay, ncol)`` float32 (``sample_cloud_scaling``, or the host's own; None: the
        unmasked call) -- bit for bit ``gas_optics_tau`` + ``increment_scaled(particles, cloud_scaling, band2gpt)`` +
        ``rte_lw_fused``, without the host owning a per-g-point float64 array.  float64, fast arithmetic mode; numpy or
        device tensors.  Returns the error message ('' = success)."""
        who = "lw_flux_scaled"
        lw = _lw_groups(plev, tlay, tsfc, tlev, top_at_1, n_gauss_angles, sfc_emis, inc_flux)
        part, out = _particle_slots(particles.tau, getattr(particles, "ssa", None)), _flux_slots(fluxes)
        f32, mixed = _call_precision(who, _named(lw["head"], lw["boundary"], part, out))
        if mixed or f32:
            return mixed or _f64_only(who, "the sampled optical-depth scaling in the fused path")
        return self._fused(lib().ecckd_lw_flux_scaled, False, ("gas", "particles", "mask"), gas_desc, particles=part,
                           mask=(_Scaling(cloud_scaling),), outputs=out, **lw)

    def sw_flux_scaled(self, plev, tlay, gas_desc, top_at_1, mu0, sfc_alb_dir, sfc_alb_dif, particles, fluxes, cloud_scaling,
                       delta_scale=True, toa_scale=None):
        """``ecckd_sw_flux_scaled``: ``sw_fluxes_allsky`` with the particulate optical depth of every (layer, g-point) cell --
        after the delta scaling -- multiplied by ``cloud_scaling`` ``(ngpt, nlay, ncol)`` float32 (None: the unmasked call), in
        the two-pass solver whatever ``"sw_solver"`` says: ``gas_optics`` + ``delta_scale`` + ``increment_scaled`` + ``rte_sw``
        to rounding.  float64, fast arithmetic mode; numpy or device tensors.  Returns the error message ('' = success)."""
        who = "sw_flux_scaled"
        sw = _sw_groups(plev, tlay, top_at_1, mu0, toa_scale, sfc_alb_dir, sfc_alb_dif)
        part = _particle_slots(particles.tau, particles.ssa, particles.g, tau_required=True)
        out = _flux_slots(fluxes, dn_dir=True)
        f32, mixed = _call_precision(who, _named(sw["head"], sw["boundary"], part, out))
        if mixed or f32:
            return mixed or _f64_only(who, "the sampled optical-depth scaling in the fused path")
        return self._fused(lib().ecckd_sw_flux_scaled, False, ("mask", "gas", "particles"), gas_desc,
                           particles=part + (int(bool(delta_scale)),), mask=(_Scaling(cloud_scaling),), outputs=out, **sw)

    def lw_flux_scaled_scratch_bytes(self, ncol, nlay):
        """``ecckd_lw_flux_scaled_scratch_bytes``: the stream scratch of ``lw_flux_scaled`` on device tensors."""
        return int(lib().ecckd_lw_flux_scaled_scratch_bytes(self._need(), int(ncol), int(nlay)))

    def sw_flux_scaled_scratch_bytes(self, ncol, nlay, delta_scale=True):
        """``ecckd_sw_flux_scaled_scratch_bytes``: the stream scratch of ``sw_flux_scaled`` on device tensors."""
        return int(lib().ecckd_sw_flux_scaled_scratch_bytes(self._need(), int(ncol), int(nlay), int(bool(delta_scale))))

    def lw_flux_bands_scratch_bytes(self, ncol, nlay):
        """``ecckd_lw_flux_bands_scratch_bytes``: the stream scratch of ``lw_fluxes_byband`` on device tensors."""
        return int(lib().ecckd_lw_flux_bands_scratch_bytes(self._need(), int(ncol), int(nlay)))

    def sw_flux_bands_scratch_bytes(self, ncol, nlay, delta_scale=True):
        """``ecckd_sw_flux_bands_scratch_bytes``: the stream scratch of ``sw_fluxes_byband`` on device tensors."""
        return int(lib().ecckd_sw_flux_bands_scratch_bytes(self._need(), int(ncol), int(nlay), int(bool(delta_scale))))

    def sw_fluxes_daylit(self, plev, tlay, gas_desc, top_at_1, mu0, sfc_alb_dir, sfc_alb_dif, fluxes, particles=None,
                         fluxes_clear=None, delta_scale=True, toa_scale=None, cloud_mask=None, day_index=None, mu0_min=0.0):
        """``ecckd_sw_fluxes_daylit``: the shortwave on the daylit columns only.  Every array has the full ``ncol``; the
        columns of ``day_index`` (an int32 list as ``daylit_columns`` returns it; None: the call selects ``mu0 > mu0_min``
        first, which synchronises) are gathered, computed by the pipeline of ``sw_fluxes`` (``particles`` None),
        ``sw_fluxes_allsky`` (``particles``, with ``cloud_mask`` the McICA form) or ``sw_fluxes_clear_allsky`` (``fluxes_clear``
        as well) -- bit for bit what that call gives on the gathered columns -- and scattered back; every other column of the
        requested outputs is 0 at every level.  float64, fast arithmetic mode; numpy or device tensors; with device tensors
        and a list made beforehand the call is asynchronous and can be captured.  Returns the error message ('' = success)."""
        if any(_is_f32(a) for a in (plev, tlay, mu0, fluxes.flux_up)):
            return "sw_fluxes_daylit: implemented for float64 arrays"
        # (the inputs are not in `returns`: a wrong one raises, every other wrong array is a message.  Without a list the columns
        # are selected once the memory space is known, and a failure of that call is a message as well)
        return self._fused(lib().ecckd_sw_fluxes_daylit, False, ("columns", "mask", "gas", "particles", "outputs"), gas_desc,
                           columns=day_index if day_index is not None else (lambda: daylit_columns(mu0, mu0_min)[0]),
                           particles=_particle_slots(*[getattr(particles, a, None) for a in ("tau", "ssa", "g")]) +
                           (int(bool(delta_scale)),), mask=(cloud_mask,),
                           outputs=_flux_slots(fluxes, dn_dir=True) + _flux_slots(fluxes_clear or _NO_FLUXES, "_clear", dn_dir=True),
                           **_sw_groups(plev, tlay, top_at_1, mu0, toa_scale, sfc_alb_dir, sfc_alb_dif))


# ------------------------------------------------------------------------------------------
# RTE solvers
# ------------------------------------------------------------------------------------------
def _device_of(a):
    if _is_torch(a) and a.is_cuda:
        return a.device.index if a.device.index is not None else 0
    return 0


def _increment(op1, op2, band2gpt, cloud_mask=None, cloud_scaling=None):
    """``ecckd_increment`` / ``_f32`` (with a mask: ``ecckd_increment_masked``; with a scaling: ``ecckd_increment_scaled``)
    on the Python containers."""
    ng, nlay, ncol = op1.tau.shape
    f32 = _is_f32(op1.tau)
    two1, two2 = isinstance(op1, OpticalProps2str), isinstance(op2, OpticalProps2str)
    try:
        space = _space_of([op1.tau, op2.tau] + ([op1.ssa, op1.g] if two1 else []) + ([op2.ssa, op2.g] if two2 else []))
        if band2gpt is None:
            nband, b2g, n2 = 0, None, ng
        else:
            b2g = np.ascontiguousarray(band2gpt, dtype=np.int32)
            nband = n2 = b2g.shape[0]
        P1 = lambda a, what: _ptr(a, (ng, nlay, ncol), what, f32)
        P2 = lambda a, what: _ptr(a, (n2, nlay, ncol), what, f32)
        a1 = (P1(op1.tau, "tau"), P1(op1.ssa, "ssa") if two1 else None, P1(op1.g, "g") if two1 else None)
        a2 = (P2(op2.tau, "other.tau"), P2(op2.ssa, "other.ssa") if two2 else None, P2(op2.g, "other.g") if two2 else None)
        mp = _mask_ptr(cloud_mask, nlay, ncol, space)
        sp = _scaling_ptr(cloud_scaling, ng, nlay, ncol, space)
    except (TypeError, ValueError) as e:
        return str(e)
    b2p = C.c_void_p(b2g.ctypes.data) if b2g is not None else None
    if cloud_scaling is not None:
        rc = (lib().ecckd_increment_scaled_f32 if f32 else lib().ecckd_increment_scaled)(
            int(_device_of(op1.tau)), ncol, nlay, ng, *a1, nband, b2p, *a2, sp, space, _stream(space))
    elif cloud_mask is not None:
        rc = (lib().ecckd_increment_masked_f32 if f32 else lib().ecckd_increment_masked)(
            int(_device_of(op1.tau)), ncol, nlay, ng, *a1, nband, b2p, *a2, mp, space, _stream(space))
    else:
        rc = (lib().ecckd_increment_f32 if f32 else lib().ecckd_increment)(
            int(_device_of(op1.tau)), ncol, nlay, ng, *a1, nband, b2p, *a2, space, _stream(space))
    return last_error() if rc else ""


def _rte_lw_2stream(optical_props, top_at_1, sources, sfc_emis, fluxes, n_gauss_angles, device, shared_levels, inc_flux,
                    flux_up_jac):
    """``ecckd_rte_lw_2stream`` behind ``rte_lw(..., use_2stream=True)``."""
    who = "rte_lw(use_2stream=True): "
    if not isinstance(optical_props, OpticalProps2str):
        return who + "two-stream optical properties required (OpticalProps2str)"
    if _is_f32(optical_props.tau):
        return who + "implemented for float64 arrays"
    if shared_levels:
        return who + "shared_levels belongs to the no-scattering solver"
    if isinstance(fluxes, FluxesByband):
        return who + "per-band fluxes are not implemented (broadband fluxes only)"
    if flux_up_jac is not None:
        return who + "flux_up_jac is not implemented"
    if n_gauss_angles != 1:
        return who + "the two-stream solver has no quadrature (n_gauss_angles must be 1)"
    ng, nlay, ncol = optical_props.tau.shape
    b2g = np.ascontiguousarray(optical_props.band2gpt, dtype=np.int32)
    nband = b2g.shape[0]
    if hasattr(sources, "separate_levels"):
        sources.separate_levels()   # this entry point reads two separate arrays: a level buffer is copied out, once
    try:
        space = _space_of([optical_props.tau, optical_props.ssa, optical_props.g, sources.lev_source_inc, sources.lev_source_dec,
                           sources.sfc_source, sfc_emis, inc_flux, fluxes.flux_up, fluxes.flux_dn])
        a3 = [_ptr(a, (ng, nlay, ncol), w) for a, w in ((optical_props.tau, "tau"), (optical_props.ssa, "ssa"), (optical_props.g, "g"),
                                                        (getattr(sources, "lay_source", None), "lay_source"),
                                                        (sources.lev_source_inc, "lev_source_inc"),
                                                        (sources.lev_source_dec, "lev_source_dec"))]
        sfc = _ptr(sources.sfc_source, (ng, ncol), "sfc_source")
        rest = [_ptr(sfc_emis, (ncol, nband), "sfc_emis"), _ptr(inc_flux, (ng, ncol), "inc_flux"),
                _ptr(fluxes.flux_up, (nlay + 1, ncol), "flux_up"), _ptr(fluxes.flux_dn, (nlay + 1, ncol), "flux_dn")]
    except (TypeError, ValueError) as e:
        return str(e)
    dev = _device_of(optical_props.tau) if device is None else device
    rc = lib().ecckd_rte_lw_2stream(int(dev), ncol, nlay, ng, int(bool(top_at_1)), *a3, sfc, nband, C.c_void_p(b2g.ctypes.data),
                                    *rest, space, _stream(space))
    return last_error() if rc else ""


def rte_lw_2stream(optical_props, top_at_1, sources, sfc_emis, fluxes, inc_flux=None, device=None):
    """``ecckd_rte_lw_2stream`` or its ``_f32`` namesake: the two-stream longwave solver, in which clouds scatter, in the
    precision of the arrays.  float64 arrays give the bits of ``rte_lw(..., use_2stream=True)``; float32 arrays (all of them)
    take the single-precision solver, whose cell is defined in include/ecckd_hip.h ("Two-stream longwave, single precision":
    fast arithmetic mode only) and whose distance from the float64 call is recorded in DESIGN.md section 3.  An
    ``OpticalProps2str``, broadband fluxes, ``inc_flux`` ``(ngpt, ncol)`` accepted, no quadrature; ``sources.lay_source`` is
    never read.  numpy or device tensors.  Returns the error message ('' = success)."""
    who = "rte_lw_2stream"
    if not isinstance(optical_props, OpticalProps2str):
        return who + ": two-stream optical properties required (OpticalProps2str)"
    if isinstance(fluxes, FluxesByband):
        return who + ": per-band fluxes are not implemented (broadband fluxes only)"
    if hasattr(sources, "separate_levels"):
        sources.separate_levels()   # this entry point reads two separate arrays: a level buffer is copied out, once
    lay = getattr(sources, "lay_source", None)
    named = [("tau", optical_props.tau), ("ssa", optical_props.ssa), ("g", optical_props.g), ("lay_source", lay),
             ("lev_source_inc", sources.lev_source_inc), ("lev_source_dec", sources.lev_source_dec),
             ("sfc_source", sources.sfc_source), ("sfc_emis", sfc_emis), ("inc_flux", inc_flux), ("flux_up", fluxes.flux_up),
             ("flux_dn", fluxes.flux_dn)]
    f32, mixed = _call_precision(who, named)
    if mixed:
        return mixed
    ng, nlay, ncol = optical_props.tau.shape
    b2g = np.ascontiguousarray(optical_props.band2gpt, dtype=np.int32)
    nband = b2g.shape[0]
    shapes = [(ng, nlay, ncol)] * 6 + [(ng, ncol), (ncol, nband), (ng, ncol), (nlay + 1, ncol), (nlay + 1, ncol)]
    try:
        space = _space_of([a for _, a in named])
        ptrs = [_ptr(a, shape, what, f32) for (what, a), shape in zip(named, shapes)]
    except (TypeError, ValueError) as e:
        return str(e)
    dev = _device_of(optical_props.tau) if device is None else device
    rc = _entry("ecckd_rte_lw_2stream", f32)(int(dev), ncol, nlay, ng, int(bool(top_at_1)), *ptrs[:7], nband, C.c_void_p(b2g.ctypes.data), *ptrs[7:], space,
            _stream(space))
    return last_error() if rc else ""


def _rte_lw_rescaled(optical_props, top_at_1, sources, sfc_emis, fluxes, n_gauss_angles, device, shared_levels, inc_flux,
                     use_2stream, flux_up_jac):
    """``ecckd_rte_lw_rescaled`` behind ``rte_lw(..., rescaled=True)``."""
    who = "rte_lw(rescaled=True): "
    if use_2stream:
        return who + "rescaled and use_2stream name two different solvers (pass one of them)"
    if not isinstance(optical_props, OpticalProps2str):
        return who + "two-stream optical properties required (OpticalProps2str; an OpticalProps1scl has nothing to rescale)"
    if _is_f32(optical_props.tau):
        return who + "implemented for float64 arrays"
    if shared_levels:
        return who + "shared_levels is not implemented"
    if isinstance(fluxes, FluxesByband):
        return who + "per-band fluxes are not implemented (broadband fluxes only)"
    if flux_up_jac is not None:
        return who + "flux_up_jac is not implemented for this keyword (rte_lw_rescaled_jac returns it)"
    ng, nlay, ncol = optical_props.tau.shape
    b2g = np.ascontiguousarray(optical_props.band2gpt, dtype=np.int32)
    nband = b2g.shape[0]
    if hasattr(sources, "separate_levels"):
        sources.separate_levels()   # this entry point reads two separate arrays: a level buffer is copied out, once
    try:
        space = _space_of([optical_props.tau, optical_props.ssa, optical_props.g, sources.lay_source, sources.lev_source_inc,
                           sources.lev_source_dec, sources.sfc_source, sfc_emis, inc_flux, fluxes.flux_up, fluxes.flux_dn])
        a3 = [_ptr(a, (ng, nlay, ncol), w) for a, w in ((optical_props.tau, "tau"), (optical_props.ssa, "ssa"), (optical_props.g, "g"),
                                                        (sources.lay_source, "lay_source"),
                                                        (sources.lev_source_inc, "lev_source_inc"),
                                                        (sources.lev_source_dec, "lev_source_dec"))]
        sfc = _ptr(sources.sfc_source, (ng, ncol), "sfc_source")
        rest = [_ptr(sfc_emis, (ncol, nband), "sfc_emis"), _ptr(inc_flux, (ng, ncol), "inc_flux"),
                _ptr(fluxes.flux_up, (nlay + 1, ncol), "flux_up"), _ptr(fluxes.flux_dn, (nlay + 1, ncol), "flux_dn")]
    except (TypeError, ValueError) as e:
        return str(e)
    dev = _device_of(optical_props.tau) if device is None else device
    rc = lib().ecckd_rte_lw_rescaled(int(dev), ncol, nlay, ng, int(bool(top_at_1)), int(n_gauss_angles), *a3, sfc, nband,
                                     C.c_void_p(b2g.ctypes.data), *rest, space, _stream(space))
    return last_error() if rc else ""


def rte_lw_rescaled_jac(optical_props, top_at_1, sources, sfc_emis, fluxes, flux_up_jac, n_gauss_angles=1, device=None, inc_flux=None):
    """``ecckd_rte_lw_rescaled_jac``: ``rte_lw(..., rescaled=True)`` plus ``flux_up_jac`` ``(nlay+1, ncol)`` float64, the
    derivative of ``flux_up`` with respect to the surface temperature under the rescaled solver (rte_lw's ``flux_up_Jac``), from
    ``sources.sfc_source_jac`` (``GasOpticsEcckd.planck_sfc_source_jac``).  The fluxes are those of ``rte_lw(..., rescaled=True)``
    bit for bit; the derivative of ``flux_dn`` (not zero under rescaling) is not returned.  An ``OpticalProps2str`` (float64),
    ``n_gauss_angles`` 1..4, broadband fluxes, ``inc_flux`` accepted (it does not enter the Jacobian); numpy or device tensors.
    Returns the error message ('' = success)."""
    who = "rte_lw_rescaled_jac: "
    if not isinstance(optical_props, OpticalProps2str):
        return who + "two-stream optical properties required (OpticalProps2str; an OpticalProps1scl has nothing to rescale)"
    if _is_f32(optical_props.tau):
        return who + "implemented for float64 arrays"
    if isinstance(fluxes, FluxesByband):
        return who + "per-band fluxes are not implemented (broadband fluxes only)"
    if flux_up_jac is None:
        return who + "flux_up_jac is required"
    if getattr(sources, "sfc_source_jac", None) is None:
        return who + "flux_up_jac needs sources.sfc_source_jac (planck_sfc_source_jac)"
    ng, nlay, ncol = optical_props.tau.shape
    b2g = np.ascontiguousarray(optical_props.band2gpt, dtype=np.int32)
    nband = b2g.shape[0]
    if hasattr(sources, "separate_levels"):
        sources.separate_levels()   # this entry point reads two separate arrays: a level buffer is copied out, once
    try:
        space = _space_of([optical_props.tau, optical_props.ssa, optical_props.g, sources.lay_source, sources.lev_source_inc,
                           sources.lev_source_dec, sources.sfc_source, sources.sfc_source_jac, sfc_emis, inc_flux, fluxes.flux_up,
                           fluxes.flux_dn, flux_up_jac])
        a3 = [_ptr(a, (ng, nlay, ncol), w) for a, w in ((optical_props.tau, "tau"), (optical_props.ssa, "ssa"), (optical_props.g, "g"),
                                                        (sources.lay_source, "lay_source"),
                                                        (sources.lev_source_inc, "lev_source_inc"),
                                                        (sources.lev_source_dec, "lev_source_dec"))]
        a2 = [_ptr(sources.sfc_source, (ng, ncol), "sfc_source"), _ptr(sources.sfc_source_jac, (ng, ncol), "sfc_source_jac")]
        rest = [_ptr(sfc_emis, (ncol, nband), "sfc_emis"), _ptr(inc_flux, (ng, ncol), "inc_flux"),
                _ptr(fluxes.flux_up, (nlay + 1, ncol), "flux_up"), _ptr(fluxes.flux_dn, (nlay + 1, ncol), "flux_dn"),
                _ptr(flux_up_jac, (nlay + 1, ncol), "flux_up_jac")]
    except (TypeError, ValueError) as e:
        return str(e)
    dev = _device_of(optical_props.tau) if device is None else device
    rc = lib().ecckd_rte_lw_rescaled_jac(int(dev), ncol, nlay, ng, int(bool(top_at_1)), int(n_gauss_angles), *a3, *a2, nband,
                                         C.c_void_p(b2g.ctypes.data), *rest, space, _stream(space))
    return last_error() if rc else ""


def lw_solver_1rescl_gpt(tau, ssa, g, lay_source, lev_source_inc, lev_source_dec, sfc_emis, sfc_src, gpt_flux_up, gpt_flux_dn,
                         top_at_1=True, Ds=(1.66,), weights=(0.5,), inc_flux=None, device=None):
    """``ecckd_lw_solver_1rescl_gpt``: RTE-RRTMGP's kernel-level ``lw_solver_1rescl_GaussQuad`` -- the rescaled
    no-scattering solver with spectral fluxes ``(ngpt, nlay+1, ncol)``; ``sfc_emis`` / ``sfc_src`` / ``inc_flux``
    ``(ngpt, ncol)``; ``Ds`` and ``weights`` of 1..4 quadrature angles.  float64, numpy or device tensors; the compatibility
    kernel (any layer count, slow).  Returns the error message ('' = success)."""
    ng, nlay, ncol = tau.shape
    D, W = np.ascontiguousarray(Ds, dtype=np.float64), np.ascontiguousarray(weights, dtype=np.float64)
    if D.shape != W.shape or D.ndim != 1:
        return "lw_solver_1rescl_gpt: Ds and weights must be two vectors of one length"
    try:
        space = _space_of([tau, ssa, g, lay_source, lev_source_inc, lev_source_dec, sfc_emis, sfc_src, inc_flux, gpt_flux_up,
                           gpt_flux_dn])
        a3 = [_ptr(a, (ng, nlay, ncol), w) for a, w in ((tau, "tau"), (ssa, "ssa"), (g, "g"), (lay_source, "lay_source"),
                                                        (lev_source_inc, "lev_source_inc"), (lev_source_dec, "lev_source_dec"))]
        a2 = [_ptr(a, (ng, ncol), w) for a, w in ((sfc_emis, "sfc_emis"), (sfc_src, "sfc_src"), (inc_flux, "inc_flux"))]
        out = [_ptr(a, (ng, nlay + 1, ncol), w) for a, w in ((gpt_flux_up, "gpt_flux_up"), (gpt_flux_dn, "gpt_flux_dn"))]
    except (TypeError, ValueError) as e:
        return str(e)
    dev = _device_of(tau) if device is None else device
    rc = lib().ecckd_lw_solver_1rescl_gpt(int(dev), ncol, nlay, ng, int(bool(top_at_1)), int(D.shape[0]), C.c_void_p(D.ctypes.data),
                                          C.c_void_p(W.ctypes.data), *a3, *a2, *out, space, _stream(space))
    return last_error() if rc else ""


def rte_lw(optical_props, top_at_1, sources, sfc_emis, fluxes, n_gauss_angles=1, device=None,
           shared_levels=False, inc_flux=None, rescaled=False, use_2stream=False, flux_up_jac=None):
    """``rte_lw(optical_props, top_at_1, sources, sfc_emis(nband,ncol), fluxes, n_gauss_angles=)``
    (ecckd_rfmip_lw.F90:130-135).  ``sfc_emis`` is ``(ncol, nband)`` in numpy order.  float32 arrays
    take the single-precision entry point.  ``shared_levels=True`` asserts that the level sources hold
    one value per level (``sources.levels_shared``, set by ecckd's gas_optics) and takes
    ``ecckd_rte_lw_shared_levels`` (fp64 only).  ``inc_flux`` ``(ngpt, ncol)``: incident diffuse flux at the
    top of the domain (rte_lw's optional argument; ``ecckd_rte_lw_inc_flux`` / ``_f32``, generic solver).
    ``flux_up_jac`` ``(nlay+1, ncol)`` float64 (rte_lw's optional ``flux_up_Jac``; ``ecckd_rte_lw_jac``): receives the
    derivative of ``flux_up`` with respect to the surface temperature from ``sources.sfc_source_jac``
    (``GasOpticsEcckd.planck_sfc_source_jac``); the fluxes are those of the call without it, bit for bit.
    ``use_2stream=True`` (rte_lw's ``use_2stream``; ``ecckd_rte_lw_2stream``): the two-stream solver, in which clouds
    scatter -- an ``OpticalProps2str`` (float64), broadband fluxes, ``inc_flux`` accepted; ``shared_levels``,
    ``FluxesByband``, ``flux_up_jac``, float32 and ``n_gauss_angles != 1`` are refused with a message.  Parity with
    RTE-RRTMGP's ``lw_solver_2stream`` is unpinned.  Pass ``use_2stream`` and ``flux_up_jac`` by
    keyword: ``flux_up_jac`` stays the last parameter (tests/test_lw_jac_host.py pins that), so ``use_2stream`` sits before it.
    ``rescaled=True`` (``ecckd_rte_lw_rescaled``; by keyword): the rescaled no-scattering solver, which RTE-RRTMGP's rte_lw runs
    on two-stream properties without ``use_2stream`` -- an ``OpticalProps2str`` (float64), ``n_gauss_angles`` 1..4, broadband
    fluxes, ``inc_flux`` accepted; ``use_2stream=True``, ``flux_up_jac`` (``rte_lw_rescaled_jac`` returns it), ``FluxesByband``,
    ``shared_levels``, float32 and an ``OpticalProps1scl`` are refused with a message.  Parity with RTE-RRTMGP is unpinned
    (DESIGN.md section 3)."""
    if rescaled:
        return _rte_lw_rescaled(optical_props, top_at_1, sources, sfc_emis, fluxes, n_gauss_angles, device, shared_levels,
                                inc_flux, use_2stream, flux_up_jac)
    if use_2stream:
        return _rte_lw_2stream(optical_props, top_at_1, sources, sfc_emis, fluxes, n_gauss_angles, device, shared_levels,
                               inc_flux, flux_up_jac)
    ng, nlay, ncol = optical_props.tau.shape
    b2g = np.ascontiguousarray(optical_props.band2gpt, dtype=np.int32)
    nband = b2g.shape[0]
    f32 = _is_f32(optical_props.tau)
    if flux_up_jac is not None:
        if f32 or shared_levels or isinstance(fluxes, FluxesByband):
            return "rte_lw: flux_up_jac is implemented for float64 broadband fluxes of the generic solver"
        if sources.sfc_source_jac is None:
            return "rte_lw: flux_up_jac needs sources.sfc_source_jac (planck_sfc_source_jac)"
        try:
            space = _space_of([optical_props.tau, sources.lay_source, sources.sfc_source_jac, sfc_emis, inc_flux, fluxes.flux_up,
                               fluxes.flux_dn, flux_up_jac])
            a3 = [_ptr(a, (ng, nlay, ncol), w) for a, w in ((optical_props.tau, "tau"), (sources.lay_source, "lay_source"))]
            a3 += _lev_ptrs(sources, (ng, nlay, ncol))
            a2 = [_ptr(sources.sfc_source, (ng, ncol), "sfc_source"), _ptr(sources.sfc_source_jac, (ng, ncol), "sfc_source_jac")]
            out = [_ptr(a, (nlay + 1, ncol), w) for a, w in ((fluxes.flux_up, "flux_up"), (fluxes.flux_dn, "flux_dn"),
                                                             (flux_up_jac, "flux_up_jac"))]
            emis = [_ptr(sfc_emis, (ncol, nband), "sfc_emis"), _ptr(inc_flux, (ng, ncol), "inc_flux")]
        except (TypeError, ValueError) as e:
            return str(e)
        dev = _device_of(optical_props.tau) if device is None else device
        rc = lib().ecckd_rte_lw_jac(int(dev), ncol, nlay, ng, int(bool(top_at_1)), int(n_gauss_angles), *a3, *a2, nband,
                                    C.c_void_p(b2g.ctypes.data), *emis, *out, space, _stream(space))
        return last_error() if rc else ""
    space = _space_of([optical_props.tau, sources.lay_source, sfc_emis, fluxes.flux_up, fluxes.flux_dn])
    dev = _device_of(optical_props.tau) if device is None else device
    if isinstance(fluxes, FluxesByband):
        if shared_levels:
            return "rte_lw: per-band fluxes are implemented for the generic solver"
        space = _space_of([optical_props.tau, sources.lay_source, sfc_emis, fluxes.bnd_flux_up, fluxes.bnd_flux_dn])
        Pb = lambda a, shape=None, what="array": _ptr(a, shape, what, f32)
        opt = lambda a, what: Pb(a, (nlay + 1, ncol), what) if a is not None else None
        rc = (lib().ecckd_rte_lw_byband_f32 if f32 else lib().ecckd_rte_lw_byband)(
            int(dev), ncol, nlay, ng, int(bool(top_at_1)), int(n_gauss_angles), Pb(optical_props.tau),
            Pb(sources.lay_source, (ng, nlay, ncol), "lay_source"),
            *_lev_ptrs(sources, (ng, nlay, ncol), f32),
            Pb(sources.sfc_source, (ng, ncol), "sfc_source"), nband, C.c_void_p(b2g.ctypes.data),
            Pb(sfc_emis, (ncol, nband), "sfc_emis"), Pb(fluxes.bnd_flux_up, (nband, nlay + 1, ncol), "bnd_flux_up"),
            Pb(fluxes.bnd_flux_dn, (nband, nlay + 1, ncol), "bnd_flux_dn"), opt(fluxes.flux_up, "flux_up"),
            opt(fluxes.flux_dn, "flux_dn"), space, _stream(space))
        return last_error() if rc else ""
    if shared_levels and f32:
        return "rte_lw: shared_levels is implemented for float64 arrays"
    if inc_flux is not None:
        if shared_levels:
            return "rte_lw: inc_flux is implemented for the generic solver"
        space = _space_of([optical_props.tau, sources.lay_source, sfc_emis, inc_flux, fluxes.flux_up, fluxes.flux_dn])
        Pi = lambda a, shape=None, what="array": _ptr(a, shape, what, f32)
        rc = (lib().ecckd_rte_lw_inc_flux_f32 if f32 else lib().ecckd_rte_lw_inc_flux)(
            int(dev), ncol, nlay, ng, int(bool(top_at_1)), int(n_gauss_angles), Pi(optical_props.tau),
            Pi(sources.lay_source, (ng, nlay, ncol), "lay_source"),
            *_lev_ptrs(sources, (ng, nlay, ncol), f32),
            Pi(sources.sfc_source, (ng, ncol), "sfc_source"), nband, C.c_void_p(b2g.ctypes.data),
            Pi(sfc_emis, (ncol, nband), "sfc_emis"), Pi(inc_flux, (ng, ncol), "inc_flux"),
            Pi(fluxes.flux_up, (nlay + 1, ncol), "flux_up"), Pi(fluxes.flux_dn, (nlay + 1, ncol), "flux_dn"),
            space, _stream(space))
        return last_error() if rc else ""
    fn = lib().ecckd_rte_lw_f32 if f32 else (lib().ecckd_rte_lw_shared_levels if shared_levels else lib().ecckd_rte_lw)
    P = lambda a, shape=None, what="array": _ptr(a, shape, what, f32)
    rc = fn(int(dev), ncol, nlay, ng, int(bool(top_at_1)), int(n_gauss_angles), P(optical_props.tau),
            P(sources.lay_source, (ng, nlay, ncol), "lay_source"),
            *_lev_ptrs(sources, (ng, nlay, ncol), f32),
            P(sources.sfc_source, (ng, ncol), "sfc_source"), nband, C.c_void_p(b2g.ctypes.data),
            P(sfc_emis, (ncol, nband), "sfc_emis"), P(fluxes.flux_up, (nlay + 1, ncol), "flux_up"),
            P(fluxes.flux_dn, (nlay + 1, ncol), "flux_dn"), space, _stream(space))
    return last_error() if rc else ""


def rte_sw(optical_props, top_at_1, mu0, toa_flux, sfc_alb_dir, sfc_alb_dif, fluxes, device=None):
    """``rte_sw(optical_props, top_at_1, mu0, toa_flux, sfc_alb_dir, sfc_alb_dif, fluxes)``
    (ecckd_rfmip_sw.F90:148-154).  Albedos are ``(ncol, nband)`` in numpy order.  float32 arrays take
    ``ecckd_rte_sw_f32`` (``_byband_f32`` for by-band fluxes).  Any layer count: up to 60 layers the layer-systolic
    solver (``"sw_solver"`` 0, the default), otherwise the two-pass kernel (include/ecckd_hip.h, ``"sw_solver"``)."""
    if not isinstance(optical_props, OpticalProps2str):
        return "rte_sw: two-stream optical properties required"
    ng, nlay, ncol = optical_props.tau.shape
    b2g = np.ascontiguousarray(optical_props.band2gpt, dtype=np.int32)
    nband = b2g.shape[0]
    space = _space_of([optical_props.tau, mu0, toa_flux, sfc_alb_dir, sfc_alb_dif, fluxes.flux_up])
    dev = _device_of(optical_props.tau) if device is None else device
    if isinstance(fluxes, FluxesByband):
        space = _space_of([optical_props.tau, mu0, toa_flux, sfc_alb_dir, sfc_alb_dif, fluxes.bnd_flux_up])
        fb = _is_f32(optical_props.tau)   # float32 arrays take ecckd_rte_sw_byband_f32
        Pb = lambda a, shape=None, what="array": _ptr(a, shape, what, fb)
        opt = lambda a, shape, what: Pb(a, shape, what) if a is not None else None
        rc = (lib().ecckd_rte_sw_byband_f32 if fb else lib().ecckd_rte_sw_byband)(
            int(dev), ncol, nlay, ng, int(bool(top_at_1)), Pb(optical_props.tau),
            Pb(optical_props.ssa, (ng, nlay, ncol), "ssa"), Pb(optical_props.g, (ng, nlay, ncol), "g"),
            Pb(mu0, (ncol,), "mu0"), Pb(toa_flux, (ng, ncol), "toa_flux"), nband,
            C.c_void_p(b2g.ctypes.data), Pb(sfc_alb_dir, (ncol, nband), "sfc_alb_dir"),
            Pb(sfc_alb_dif, (ncol, nband), "sfc_alb_dif"),
            Pb(fluxes.bnd_flux_up, (nband, nlay + 1, ncol), "bnd_flux_up"),
            Pb(fluxes.bnd_flux_dn, (nband, nlay + 1, ncol), "bnd_flux_dn"),
            opt(fluxes.bnd_flux_dn_dir, (nband, nlay + 1, ncol), "bnd_flux_dn_dir"),
            opt(fluxes.flux_up, (nlay + 1, ncol), "flux_up"), opt(fluxes.flux_dn, (nlay + 1, ncol), "flux_dn"),
            opt(fluxes.flux_dn_dir, (nlay + 1, ncol), "flux_dn_dir"), space, _stream(space))
        return last_error() if rc else ""
    f32 = _is_f32(optical_props.tau)   # float32 arrays take ecckd_rte_sw_f32
    P = lambda a, shape=None, what="array": _ptr(a, shape, what, f32)
    rc = (lib().ecckd_rte_sw_f32 if f32 else lib().ecckd_rte_sw)(
        int(dev), ncol, nlay, ng, int(bool(top_at_1)), P(optical_props.tau),
        P(optical_props.ssa, (ng, nlay, ncol), "ssa"), P(optical_props.g, (ng, nlay, ncol), "g"),
        P(mu0, (ncol,), "mu0"), P(toa_flux, (ng, ncol), "toa_flux"), nband,
        C.c_void_p(b2g.ctypes.data), P(sfc_alb_dir, (ncol, nband), "sfc_alb_dir"),
        P(sfc_alb_dif, (ncol, nband), "sfc_alb_dif"), P(fluxes.flux_up, (nlay + 1, ncol), "flux_up"),
        P(fluxes.flux_dn, (nlay + 1, ncol), "flux_dn"),
        P(fluxes.flux_dn_dir, (nlay + 1, ncol), "flux_dn_dir"), space, _stream(space))
    return last_error() if rc else ""


# ------------------------------------------------------------------------------------------
# heating rates (include/ecckd_hip.h, "Heating rates")
# ------------------------------------------------------------------------------------------
GRAV, CP_DRY = 9.80665, 1004.64   # m s-2, J kg-1 K-1: the customary constants; arguments of every call, not library state


def heating_rate(flux_up, flux_dn, plev, heating_rate=None, cp=None, grav=GRAV, cp_dry=CP_DRY, device=None):
    """``ecckd_heating_rate`` (RTE-RRTMGP's ``compute_heating_rate``): the divergence of the net flux across each layer as a
    temperature tendency in K s-1, ``(dnet * grav) / (c * dp)`` operation by operation as include/ecckd_hip.h spells it.
    ``flux_up``, ``flux_dn``: ``(nlay+1, ncol)`` or ``(nouter, nlay+1, ncol)`` -- the by-band fluxes, or any stack of flux
    sets; for shortwave ``flux_dn`` is the total, direct beam included.  ``plev``: ``(nlay+1, ncol)``, shared by the planes.
    ``cp``: ``(nlay, ncol)`` specific heat per cell, replacing ``cp_dry``.  ``heating_rate``: ``(nlay, ncol)`` or
    ``(nouter, nlay, ncol)``; allocated like ``flux_up`` when not given; it must not alias an input.  There is no
    ``top_at_1``: the expression does not depend on the orientation.  numpy arrays (staged), torch device tensors
    (asynchronous on the current stream, capturable), or numpy inputs with a device ``heating_rate``.  float32 arrays take
    the ``_f32`` call (``grav`` and ``cp_dry`` are rounded to float once); mixed precisions are refused.
    Returns ``(error_message, heating_rate)``, the message '' on success."""
    who = "heating_rate"
    if getattr(flux_up, "ndim", 0) not in (2, 3):
        return who + ": flux_up must be (nlay+1, ncol) or (nouter, nlay+1, ncol)", heating_rate
    nlev, ncol = (int(n) for n in flux_up.shape[-2:])
    outer = tuple(int(n) for n in flux_up.shape[:-2])
    nouter, nlay = (outer[0] if outer else 1), nlev - 1
    if nlay < 1 or ncol < 1 or nouter < 1:
        return who + ": flux_up has shape %s: at least two levels, one column and one plane are needed" % (tuple(flux_up.shape),), heating_rate
    named = (("flux_up", flux_up), ("flux_dn", flux_dn), ("plev", plev), ("cp", cp), ("heating_rate", heating_rate))
    f32, err = _call_precision(who, named)
    if err:
        return err, heating_rate
    try:
        inputs = [flux_up, flux_dn, plev, cp]
        space = _space_of(inputs)
        if heating_rate is None:
            heating_rate = _empty_like_space(outer + (nlay, ncol), flux_up)
        elif _space_of([heating_rate]) != space:
            if space != HOST:
                raise TypeError("mixing host and device arrays in one call")
            space = MIXED   # host inputs, a device result
        ptrs = [_ptr(flux_up, outer + (nlev, ncol), "flux_up", f32), _ptr(flux_dn, outer + (nlev, ncol), "flux_dn", f32),
                _ptr(plev, (nlev, ncol), "plev", f32)]
        cpp = _ptr(cp, (nlay, ncol), "cp", f32)
        out = _ptr(heating_rate, outer + (nlay, ncol), "heating_rate", f32)
    except (TypeError, ValueError) as e:
        return who + ": " + str(e), heating_rate
    if device is None:
        device = _device_of(heating_rate if space == MIXED else flux_up)
    rc = (lib().ecckd_heating_rate_f32 if f32 else lib().ecckd_heating_rate)(
        int(device), ncol, nlay, nouter, *ptrs, float(grav), float(cp_dry), cpp, out, space, _stream(space))
    return (last_error() if rc else ""), heating_rate
