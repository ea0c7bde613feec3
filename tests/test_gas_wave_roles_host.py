"""gas_roles_kernel (rte-ecckd_amd/csrc/kernels_gas_roles.hip) in the built gfx950 code object, read from its metadata through
tools/kernel_resources.py; no GPU needed.  Every instantiation runs three waves per SIMD: 768 threads per block, one block
per CU -- the point of the kernel is the third wave slot, which the source waves take.  The register figures are printed
(pytest -s shows them; profiles/gas_wave_roles_kernel_resources_this.txt holds the listing of the commit)."""
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def test_roles_kernels_run_three_waves_per_simd(pkg):
    import kernel_resources
    ks = {n: k for n, k in kernel_resources.kernels(pkg.LIB_PATH).items() if re.search(r"gas_roles_kernel<[^>]*>", n)}
    shapes = sorted(re.search(r"gas_roles_kernel<([^>]*)>", n).group(1).replace(" ", "") for n in ks)
    assert "8,7" in shapes and "4,7" in shapes, shapes      # the 32-g and the 36-g file
    for name, k in sorted(ks.items()):
        print("%s: vgpr %d, spilled vgpr %d, spilled sgpr %d, scratch %d B, waves/SIMD %d"
              % (re.search(r"gas_roles_kernel<[^>]*>", name).group(0), k["vgpr"], k["spill_vgpr"], k["spill_sgpr"],
                 k["scratch_bytes"], kernel_resources.waves_per_simd(k)))
        assert kernel_resources.waves_per_simd(k) == 3, name
        assert k["max_flat_wg"] == 768, name
