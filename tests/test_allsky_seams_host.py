"""CPU checks of tests/seam_helpers.py: the seam layers of every solver form against values worked out by hand from the
kernels' constants, the cloud and mask generators against their description, and -- on the C oracle alone -- the conditions
the GPU seam tests assert (tests/test_gpu_allsky_seams.py): every seam layer's particles move the reference fluxes by at
least 20 fp64 bars in the columns that carry them, and the one-cloud-per-column pattern keeps the shortwave cloud signal
far above what single precision can blur.

Measured here with the oracle (24 columns from column 3, 48 in the shortwave; W m-2), the smallest change over the seam
layers: longwave at 1, 2, 5, 33, 60, 97 and 137 layers (the seam layers of the register-resident and the two-stream solver
at once, at 60 those of the layer-split and Jacobian kernels as well) 0.045 (fsck) and 1.35 (rrtmgp) with pattern "all",
0.71 and 3.41 with pattern "one", 0.15 and 0.52 under the mask; shortwave at 1, 4, 6, 59, 60 and 61 layers 0.017 plain and
0.17 masked; shortwave pattern "one", all-sky minus clear-sky, 25.1.
The float32 longwave bars are 2.0e-3 ... 5.9e-3 W m-2 under signals of 0.33 ... 8.2."""
import numpy as np
import pytest

import allsky_helpers as ah
import mcica_helpers as mh
import seam_cases as gpu_cases
import seam_helpers as sh
from helpers import FLUX_ATOL
from rte_ecckd_amd import synthetic

BAR = 10 * FLUX_ATOL


def test_seam_layers_by_hand():
    s = sh.seam_layers
    assert s("lw_register", 1, True) == [0] and s("lw_register", 2, False) == [0, 1]
    assert s("lw_register", 33, True) == [0, 7, 8, 32]                      # padded to 48, kPF = 8
    assert s("lw_register", 33, False) == [0, 24, 25, 32]
    assert s("lw_register", 81, True) == [0, 3, 4, 80]                      # padded to 96, kPF = 4
    assert s("lw_register", 137, True) == [0, 3, 4, 40, 41, 44, 45, 136]    # nover = 41
    assert s("lw_register", 137, False) == [0, 91, 92, 95, 96, 132, 133, 136]
    assert s("lw_register", 97, True) == [0, 1, 3, 4, 5, 96]                # nover = 1: the ring holds one layer
    assert s("lw_split60", 60, True) == [0, 1, 2, 14, 15, 16, 17, 29, 30, 31, 32, 44, 45, 46, 47, 59]
    assert s("lw_split60", 60, False) == [59 - l for l in reversed(s("lw_split60", 60, True))]
    assert s("sw_systolic", 4, True) == [0, 3] and s("sw_systolic", 5, True) == [0, 4]
    assert s("sw_systolic", 6, True) == [0, 4, 5] and s("sw_systolic", 11, False) == [0, 1, 5, 6, 10]
    assert s("sw_systolic", 56, True) == sorted(set(range(0, 56, 5)) | set(range(4, 56, 5)) | {55})
    # two passes, 2 (with particles) or 3 layers in flight: 0, 1 | 2, 2 | 3 from the top, the same from the surface
    assert s("sw_two_pass", 137, True) == [0, 1, 2, 3, 133, 134, 135, 136] == s("sw_two_pass", 137, False)
    assert s("sw_two_pass", 2, True) == [0, 1] and s("sw_two_pass", 4, False) == [0, 1, 2, 3]
    assert s("sw_two_pass", 10, True) == [0, 1, 2, 3, 6, 7, 8, 9] and s("sw_two_pass", 6, True) == [0, 1, 2, 3, 4, 5]
    assert s("lw_2stream", 59, False) == [0, 1, 2, 3, 55, 56, 57, 58] and s("lw_2stream", 5, True) == [0, 1, 2, 3, 4]
    assert s("lw_jac", 7, True) == [0, 2, 3, 6] and s("lw_jac", 61, True) == [0, 56, 57, 60]   # walked from the surface
    assert s("lw_jac", 61, False) == [0, 3, 4, 60]
    for kind in sh.KINDS:
        for nlay in (60,) if kind == "lw_split60" else (1, 2, 3, 4, 5, 6, 9, 10, 11, 31, 59, 60):
            for top in (True, False):
                got = s(kind, nlay, top)
                assert got == sorted(set(got)) and got[0] == 0 and got[-1] == nlay - 1, (kind, nlay, top)


@pytest.mark.parametrize("nlay,ncol", [(1, 1), (5, 33), (60, 65), (137, 130)])
def test_generators_do_what_they_say(nlay, ncol):
    seams = sh.seam_layers("lw_register", nlay, True)
    off = np.setdiff1d(np.arange(nlay), seams)
    for pattern in ("all", "one"):
        c = sh.seam_clouds(5, nlay, ncol, seams, pattern, 7)
        again = sh.seam_clouds(5, nlay, ncol, seams, pattern, 7)
        assert all(np.array_equal(c[n], again[n]) for n in c)
        assert c["tau"].shape == c["ssa"].shape == c["g"].shape == (5, nlay, ncol) and c["cloudy"].shape == (ncol,)
        assert np.all(c["tau"][:, off, :] == 0)
        on = c["tau"] > 0
        assert np.all((c["tau"][on] >= 0.5) & (c["tau"][on] < 3.0)) and np.all(on == on[:1])
        for n, lo, hi in (("ssa", 0.6, 1.0), ("g", 0.7, 0.9)):   # random in every cell: no two cells alike, none zero
            assert np.all((c[n] >= lo) & (c[n] < hi)) and np.unique(c[n]).size == c[n].size
        if pattern == "all":
            assert np.array_equal(c["cloudy"], (np.arange(ncol) % 2 == 1) | (ncol == 1))
            assert np.all(on[0][np.ix_(seams, c["cloudy"])]) and not on[0][:, ~c["cloudy"]].any()
        else:
            assert c["cloudy"].all() and np.all(on[0].sum(axis=0) == 1)
            assert np.array_equal(np.argmax(on[0], axis=0), np.asarray(seams)[np.arange(ncol) % len(seams)])
    for ngpt in (27, 32, 36):
        m = sh.seam_masks(nlay, ncol, ngpt, seams, 11)
        assert m.dtype == np.uint64 and m.shape == (nlay, ncol) and np.array_equal(m, sh.seam_masks(nlay, ncol, ngpt, seams, 11))
        assert not (m >> np.uint64(ngpt)).any()
        bits = mh.unpack(m, ngpt)
        for i, l in enumerate(seams):
            for c_ in range(ncol):
                b, p = bits[l, c_], sh.MASK_PATTERNS[sh.seam_pattern(i, c_)]
                want = {"ones": np.ones(ngpt, bool), "zero": np.zeros(ngpt, bool), "bit0": np.arange(ngpt) == 0,
                        "last_bit": np.arange(ngpt) == ngpt - 1, "upper_half": np.arange(ngpt) >= 32,
                        "alternating": np.arange(ngpt) % 2 == 0}[p]
                assert np.array_equal(b, want), (ngpt, l, c_, p)
        if ncol >= 33:   # the odd (cloudy) columns meet all six patterns on every seam layer; off the seams the words differ
            for i in range(len(seams)):
                assert {sh.seam_pattern(i, c_) for c_ in range(1, ncol, 2)} == set(range(6))
            if off.size:
                assert np.unique(m[off]).size > 0.9 * m[off].size
    # coverage as the GPU module's union check computes it
    c = sh.seam_clouds(5, nlay, ncol, seams, "all", 7)
    cell, cleared, kept = sh.coverage(c, sh.seam_masks(nlay, ncol, 36, seams, 11), 36)
    assert np.array_equal(np.nonzero(cell)[0], seams)
    if ncol >= 33:
        assert np.array_equal(np.nonzero(cleared)[0], seams) and np.array_equal(np.nonzero(kept)[0], seams)


def sw_columns(m, ncol, nlay, c0=3):
    cols = synthetic.columns(c0, ncol, float(np.exp(m.log_pressure[0])), nlay=nlay, shortwave=True)
    rng = np.random.default_rng(ncol + nlay)
    nb = m.band2gpt.shape[0]
    cols["alb_dir"], cols["alb_dif"] = rng.uniform(0.02, 0.6, (ncol, nb)), rng.uniform(0.02, 0.6, (ncol, nb))
    cols["scale"] = rng.uniform(0.97, 1.03, ncol)
    return cols


@pytest.mark.parametrize("which", ["fsck", "rrtmgp"])
def test_longwave_seam_signal_on_the_oracle(oracle_mod, which):
    """Condition 1 on the oracle alone: removing the particles of any one seam layer moves the reference by at least 20 bars
    (2e-7 W m-2) in every column that carries them -- pattern "all" (every other seam cloudy as well) and "one", both
    orientations, with the mask (over the cells where at least half of the g-points see the cloud, seam_helpers.layer_signals)."""
    from conftest import LW_FSCK, LW_RRTMGP
    m = oracle_mod.CkdModel(LW_FSCK if which == "fsck" else LW_RRTMGP)
    nb, ncol, low = m.band2gpt.shape[0], 24, {}
    for nlay in (1, 2, 5, 33, 60, 97, 137):
        cols = synthetic.columns(3, ncol, float(np.exp(m.log_pressure[0])), nlay=nlay)
        for top in (True, False):
            kinds = ["lw_register", "lw_2stream"] + (["lw_split60"] if nlay == 60 else []) + (["lw_jac"] if nlay <= 60 else [])
            seams = sorted(set().union(*[sh.seam_layers(k, nlay, top) for k in kinds]))
            mask = sh.seam_masks(nlay, ncol, m.ng, seams, nlay)
            for pattern, mk in (("all", None), ("one", None), ("all", mask)):
                cloud = sh.seam_clouds(nb, nlay, ncol, seams, pattern, nlay)
                sig = sh.layer_signals(sh.lw_reference(oracle_mod, m, cols, mk, top_at_1=top), cloud, seams, mk, m.ng)
                assert sorted(sig) == seams or (pattern == "one" and ncol < len(seams)) or mk is not None, (nlay, top, pattern)
                key = (pattern, mk is not None)
                low[key] = min(low.get(key, np.inf), min(sig.values()))
                assert min(sig.values()) >= 20 * BAR, (which, nlay, top, pattern, mk is not None, sig)
    print("longwave %s: smallest seam-layer signal, W m-2: %s" % (which, {k: "%.3g" % v for k, v in low.items()}))


def test_shortwave_seam_signal_on_the_oracle(oracle_mod):
    """Condition 1 for the shortwave: under sh.signal_pattern's choice every seam layer of either solver keeps 20 fp64 bars,
    masked or not; pattern "one" keeps the all-sky-minus-clear-sky signal of every column far above single precision's
    reach (the GPU test asserts 20 max e(F) <= the signal)."""
    from conftest import SW_WIDE
    m = oracle_mod.CkdModel(SW_WIDE)
    nb, ncol, low, one = m.band2gpt.shape[0], 48, {}, np.inf
    for nlay in (1, 4, 6, 59, 60, 61):
        cols = sw_columns(m, ncol, nlay)
        for kind in ["sw_two_pass"] + (["sw_systolic"] if nlay <= 60 else []):
            for top, delta in ((True, True), (False, False)):
                seams = sh.seam_layers(kind, nlay, top)
                pattern = sh.signal_pattern(seams)
                mask = sh.seam_masks(nlay, ncol, m.ng, seams, nlay)
                for mk in (None, mask):
                    cloud = sh.seam_clouds(nb, nlay, ncol, seams, pattern, nlay)
                    sig = sh.layer_signals(sh.sw_reference(oracle_mod, m, cols, delta, mk, top), cloud, seams, mk, m.ng)
                    assert mk is not None or sorted(sig) == seams
                    low[mk is not None] = min(low.get(mk is not None, np.inf), min(sig.values()))
                    assert min(sig.values()) >= 20 * BAR, (nlay, kind, top, delta, mk is not None, sig)
                cloud = sh.seam_clouds(nb, nlay, ncol, seams, "one", nlay)
                run = sh.sw_reference(oracle_mod, m, cols, delta, None, top)
                one = min(one, ah.smallest_cloud_signal(run(cloud), run(None), cloud["cloudy"]))
    print('shortwave: smallest seam-layer signal, pattern "all": %.3g (plain) %.3g (masked); pattern "one", all-sky minus clear-sky: %.3g W m-2'
          % (low[False], low[True], one))
    assert one >= 20 * 0.5     # 0.5 W m-2: the worst-column bar of the single-precision clear-sky shortwave


def test_every_seam_of_the_gpu_module_is_covered():
    """Condition 2 from the GPU module's case tables: every form it runs, at every layer count and orientation, puts a
    cloudy cell, a cleared mask bit and a set mask bit on every seam layer."""
    cov = gpu_cases.check_every_seam_is_covered()
    assert {(k[0], k[2]) for k in cov} >= {("lw fp64", n) for n in gpu_cases.LW_NLAY} | {("lw f32", 60), ("lw fp64 split", 60)} \
        | {("sw fp64", n) for n in gpu_cases.SW_NLAY} | {("sw f32", n) for n in gpu_cases.SW_NLAY} | {("lw jacobian", n) for n in gpu_cases.JAC_NLAY} \
        | {(f, n) for f in ("lw rescaled", "lw two-stream") for n in gpu_cases.SCAT_NLAY}


def test_float32_longwave_bars_stay_below_the_seam_signals(oracle_mod):
    """The single-precision longwave cases of the GPU module against the oracle: helpers.lw_f32_bar (from the float32
    restatement, no GPU involved) stays 20 times below every seam layer's signal (asserted inside f32_oracle_case)."""
    from conftest import LW_FSCK, LW_RRTMGP
    models = {"fsck": oracle_mod.CkdModel(LW_FSCK), "rrtmgp": oracle_mod.CkdModel(LW_RRTMGP)}
    for which, nlay, top in gpu_cases.F32_ORACLE:
        m = models[which]
        bar, low = gpu_cases.f32_oracle_case(oracle_mod, m, float(np.exp(m.log_pressure[0])), which, nlay, top)[3:]
        print("float32 longwave %s nlay %d top_at_1 %d: bar %.3g, smallest seam-layer signal %.3g W m-2" % (which, nlay, top, bar, low))
        assert 1e-4 <= bar and 20 * bar <= low
