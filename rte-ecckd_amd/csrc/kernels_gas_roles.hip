// kernels_gas_roles.hip -- longwave gas optics with the work of a block split by kind between its waves ("gas_wave_roles").
//
// gas_fused_kernel (kernels_gas_fused.hip) keeps all the work of a cell in one wave: at 232-256 VGPRs two waves per SIMD
// alternate "compute a chunk" and "store a chunk", and a wave that waits for room in the CU's store path cannot issue its
// arithmetic.  Here a block of 768 threads walks the same 512-column tiles of one layer:
//   waves 0-7   tau waves: the tau-only work of their 64 columns (inputs, two logs, corner weights, look-up-table and
//               bilinear items) and the tau stores -- a third of the bytes; the register set of the tau-only shape, which
//               fits the 168-VGPR cap of three waves per SIMD;
//   waves 8-11  source waves: wave 8 + s computes and stores the Planck sources of the columns of tau waves 2s and 2s + 1
//               -- about ten fp64 operations and four LDS reads per cell, two thirds of the bytes.
// Each SIMD holds two tau waves and one source wave, and back-pressure from the store path parks mostly the wave that has
// no arithmetic to lose.  Grid, tile, segment logic, slab placement, Planck window and LDS image are gas_fused_kernel's:
// the body is the same function (gas_fused_body.hpp, ROLES = true), and so are the expressions -- the outputs hold the
// same bits.  planck_edge_kernel (kernels_planck.hip) keeps the surface source and the top level.
//
// Barriers: every block barrier of the body stands in code that all twelve waves run the same number of times (the LDS
// clear, the segment pre-pass, the slab positions), and the per-tile execution barrier of "gas_tile_sync" stands before
// the role branch of the one tile loop; see the comment there.
#include "gas_fused_body.hpp"

namespace ecckd {
namespace {

template <int GC, int NB>
__global__ void __launch_bounds__(kRolesThreads, 3) gas_roles_kernel(const FusedArgs a) {
  gas_fused_body<double, GC, NB, true, false, MODE_LW, double, kBlock, true>(a);
}

template <int GC, int NB>
hipError_t launch_roles(const FusedArgs &a, size_t lds_bytes, hipStream_t s) {
  auto k = gas_roles_kernel<GC, NB>;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k, dim3(a.tau.col_chunks, a.tau.nlay), dim3(kRolesThreads), lds_bytes, s, a);
  return hipGetLastError();
}

}  // namespace

// The shapes with an instantiation: seven bilinear slots (the 32-g file in chunks of 8 g-points, the 36-g file in chunks of
// 4) and the merged-slot shape of two.
bool gas_roles_applies(int GC, int NB) { return (GC == 8 || GC == 4) && (NB == 7 || NB == 2); }

// "gas_wave_roles" = -1: on for the shapes whose points won against the parent commit's build (DESIGN.md section 5.1,
// "Wave roles"; profiles/gas_wave_roles.json), off elsewhere.
bool gas_roles_default(int GC, int NB) { return NB == 7 && (GC == 8 || GC == 4); }

hipError_t launch_gas_roles(const FusedArgs &a, int GC, int NB, size_t lds_bytes, hipStream_t s) {
  if (!a.wave_roles || a.mode != MODE_LW || a.f32 || a.slab32 || a.tau.ng % GC != 0) return hipErrorInvalidValue;
  if (GC == 8 && NB == 7) return launch_roles<8, 7>(a, lds_bytes, s);
  if (GC == 4 && NB == 7) return launch_roles<4, 7>(a, lds_bytes, s);
  if (GC == 8 && NB == 2) return launch_roles<8, 2>(a, lds_bytes, s);
  if (GC == 4 && NB == 2) return launch_roles<4, 2>(a, lds_bytes, s);
  return hipErrorInvalidValue;   // (prepare_gas_fused asks gas_roles_applies first: a missing kernel is an error)
}

}  // namespace ecckd
