// kernels_cloud_optics.hip -- cloud optics: liquid and ice water paths and effective radii per (column, layer) to the
// particulate optical properties tau, ssa, g (or the absorption optical depth alone) on the model's bands -- what an
// all-sky host calls between gas_optics and increment / the fused all-sky flux calls.
//
// Restates the look-up-table form of RTE-RRTMGP's ty_cloud_optics%cloud_optics of the v1.5 era [RTE-ext:
// extensions/cloud_optics/mo_cloud_optics.F90, compute_all_from_table and the combination of the two phases; the library
// is not part of the reference tree].  The definition is spelt operation by operation in include/ecckd_hip.h
// (ecckd_cloud_optics); every expression here keeps that order, and the build has FMA contraction off, so the results are
// those of an IEEE evaluation of the formulas in the precision of the call.
//
// Mapping (gfx950): a streaming kernel judged by bytes moved over time (32 + 24*nband bytes per cell in fp64).  One lane
// owns a (column, layer) cell, the column fastest: it reads its four inputs once, forms the table index and the
// interpolation weight of each phase once, then walks the bands; every store of a wave is one full coalesced line of a
// band plane.  256 threads per block; the grid is what is resident at a time (8 blocks per CU, or as many as the LDS images
// allow), the rest of the cells by grid stride: a larger grid would leave a second, partly filled round of blocks.
// Tables: the object keeps, per precision, an image of (value, slope) pairs -- a 16-byte-aligned pair in fp64, so one
// 128-bit read serves an interpolation (8 bytes and one 64-bit read in single precision).  While both phases' images for
// the chosen roughness fit kCloudOpticsLdsBytes (32 KiB: five blocks, 20 waves, stay resident per CU beside the 160 KiB
// of LDS) a block copies them into LDS, and only once a cell of the block is cloudy; larger tables are read in place,
// through L2 (the image of a real table set is tens of KiB and stays there).
// Most cells are clear: a phase that no lane of a wave holds is skipped with a ballot, so a wave without cloud writes its
// zeros and reads no table.  Lanes of a wave that does read are safe whatever their radius holds: the index is clamped
// to the table on both sides (a NaN takes the first interval), and a clear cell selects +0, it does not multiply.
#include "kernels.hpp"

namespace ecckd {
namespace {

constexpr int kCoBlock = 256;
constexpr int kCoBlocksPerCu = 8;   // 32 waves per CU; fewer where the LDS image of the tables allows fewer (launch_t)

template <typename real> __host__ __device__ constexpr real co_eps() {   // epsilon(1._wp)
  return sizeof(real) == 4 ? real(1.1920928955078125e-07f) : real(2.220446049250313e-16);
}
// max(eps, x) as the Fortran intrinsic on finite arguments; a NaN gives eps (the numerators carry the NaN on)
template <typename real> __device__ __forceinline__ real floor_eps(real x) { return x > co_eps<real>() ? x : co_eps<real>(); }

// 0-based interval of the radius `re` in a table of npair = nsize-1 intervals, and the weight inside it:
//   s = (re - r_lwr)/step;  index = min(floor(s)+1, nsize-1), at least 1 (a NaN takes 1);  fint = s - (index-1)
template <typename real> __device__ __forceinline__ int interval_of(real re, real r_lwr, real step, int npair, real &fint) {
  const real s = (re - r_lwr) / step;
  const real f1 = floor(s) + real(1);
  const int index = f1 >= real(npair) ? npair : (f1 >= real(1) ? (int)f1 : 1);
  fint = s - real(index - 1);
  return index - 1;
}

// t, ts, tsg of one phase at one band: rows of the band at `row` (ext), row + qstride (ssa), row + 2*qstride (asy)
template <typename real, bool TWO_STREAM>
__device__ __forceinline__ void phase_band(const CloudLutPair<real> *row, size_t qstride, real wp, real fint, bool cloudy, real &t,
                                           real &ts, real &tsg) {
  const CloudLutPair<real> e = row[0], w = row[qstride];
  const real t_ = wp * (e.value + fint * e.slope);
  const real ts_ = t_ * (w.value + fint * w.slope);
  t = cloudy ? t_ : real(0);
  ts = cloudy ? ts_ : real(0);
  if constexpr (TWO_STREAM) {
    const CloudLutPair<real> a = row[2 * qstride];
    const real tsg_ = ts_ * (a.value + fint * a.slope);
    tsg = cloudy ? tsg_ : real(0);
  }
}

template <typename real, bool TWO_STREAM, bool LDS>
__global__ void __launch_bounds__(kCoBlock) cloud_optics_kernel(const CloudOpticsArgs a) {
  extern __shared__ __align__(16) unsigned char co_smem[];
  typedef CloudLutPair<real> Pair;
  const int npl = a.nsize_liq - 1, npi = a.nsize_ice - 1;
  const size_t ql = (size_t)a.nband * npl, qi = (size_t)a.nband * npi;   // pairs of one quantity
  constexpr int kQuantities = TWO_STREAM ? 3 : 2;                        // (the one-scalar form reads no asymmetry)
  const Pair *liq = static_cast<const Pair *>(a.lut_liq), *ice = static_cast<const Pair *>(a.lut_ice);
  if constexpr (LDS) {
    liq = reinterpret_cast<const Pair *>(co_smem);
    ice = liq + kQuantities * ql;
  }
  const real *clwp = reinterpret_cast<const real *>(a.clwp), *ciwp = reinterpret_cast<const real *>(a.ciwp),
             *reliq = reinterpret_cast<const real *>(a.reliq), *reice = reinterpret_cast<const real *>(a.reice);
  real *tau = reinterpret_cast<real *>(a.tau), *ssa = reinterpret_cast<real *>(a.ssa), *g = reinterpret_cast<real *>(a.g);
  const real rl_lwr = (real)a.radliq_lwr, rl_step = (real)a.radliq_step, ri_lwr = (real)a.radice_lwr, ri_step = (real)a.radice_step;
  const size_t ncell = (size_t)a.ncol * a.nlay;
  [[maybe_unused]] bool staged = false;   // (the same in every thread of the block)

  for (size_t base = (size_t)blockIdx.x * kCoBlock; base < ncell; base += (size_t)gridDim.x * kCoBlock) {
    const size_t cell = base + threadIdx.x;
    const bool live = cell < ncell;
    real lwp = real(0), iwp = real(0), rel = real(0), rei = real(0);
    if (live) { lwp = clwp[cell]; iwp = ciwp[cell]; rel = reliq[cell]; rei = reice[cell]; }
    const bool cl = lwp > real(0), ci = iwp > real(0);   // (NaN, 0, negative: not cloudy)
    if constexpr (LDS) {
      if (!staged && __syncthreads_or(cl || ci)) {
        Pair *sm = reinterpret_cast<Pair *>(co_smem);
        const Pair *gl = static_cast<const Pair *>(a.lut_liq), *gi = static_cast<const Pair *>(a.lut_ice);
        for (size_t i = threadIdx.x; i < kQuantities * ql; i += kCoBlock) sm[i] = gl[i];
        for (size_t i = threadIdx.x; i < kQuantities * qi; i += kCoBlock) sm[kQuantities * ql + i] = gi[i];
        __syncthreads();
        staged = true;
      }
    }
    const bool any_l = __ballot(cl) != 0ull, any_i = __ballot(ci) != 0ull;
    real fl = real(0), fi = real(0);
    const int il = interval_of(rel, rl_lwr, rl_step, npl, fl), ii = interval_of(rei, ri_lwr, ri_step, npi, fi);
    for (int b = 0; b < a.nband; ++b) {
      real lt = real(0), lts = real(0), ltsg = real(0), it = real(0), its = real(0), itsg = real(0);
      if (any_l) phase_band<real, TWO_STREAM>(liq + (size_t)b * npl + il, ql, lwp, fl, cl, lt, lts, ltsg);
      if (any_i) phase_band<real, TWO_STREAM>(ice + (size_t)b * npi + ii, qi, iwp, fi, ci, it, its, itsg);
      if (!live) continue;
      const size_t q = cell + ncell * b;
      if constexpr (TWO_STREAM) {
        const real t = lt + it;
        const real tssa = lts + its;
        g[q] = (ltsg + itsg) / floor_eps(tssa);
        ssa[q] = tssa / floor_eps(t);
        tau[q] = t;
      } else {
        tau[q] = (lt - lts) + (it - its);
      }
    }
  }
}

template <typename real>
hipError_t launch_t(const CloudOpticsArgs &a, hipStream_t s) {
  const bool two = a.ssa != nullptr;
  const size_t image = cloud_optics_image_bytes(a.nband, a.nsize_liq, a.nsize_ice, two, sizeof(real) == 4);
  const bool lds = image <= kCloudOpticsLdsBytes;
  const size_t ncell = (size_t)a.ncol * a.nlay, want = (ncell + kCoBlock - 1) / kCoBlock;
  const size_t by_lds = lds && image > 0 ? (size_t)kLdsBudget / image : (size_t)kCoBlocksPerCu;
  const size_t resident = (size_t)(a.cus > 0 ? a.cus : 256) * (by_lds < (size_t)kCoBlocksPerCu ? by_lds : (size_t)kCoBlocksPerCu);
  const unsigned blocks = (unsigned)(want > resident ? resident : want);
  typedef void (*K)(const CloudOpticsArgs);
  const K k = two ? (lds ? cloud_optics_kernel<real, true, true> : cloud_optics_kernel<real, true, false>)
                  : (lds ? cloud_optics_kernel<real, false, true> : cloud_optics_kernel<real, false, false>);
  hipLaunchKernelGGL(k, dim3(blocks), dim3(kCoBlock), lds ? image : 0, s, a);
  return hipGetLastError();
}

}  // namespace

size_t cloud_optics_image_bytes(int nband, int nsize_liq, int nsize_ice, bool two_stream, bool f32) {
  const size_t pairs = (size_t)(two_stream ? 3 : 2) * nband * ((size_t)(nsize_liq - 1) + (size_t)(nsize_ice - 1));
  return pairs * 2 * (f32 ? sizeof(float) : sizeof(double));
}

hipError_t launch_cloud_optics(const CloudOpticsArgs &a, hipStream_t s) {
  if (a.ncol <= 0 || a.nlay <= 0) return hipSuccess;
  if (a.nband < 1 || a.nsize_liq < 2 || a.nsize_ice < 2 || (a.ssa == nullptr) != (a.g == nullptr)) return hipErrorInvalidValue;
  return a.f32 ? launch_t<float>(a, s) : launch_t<double>(a, s);
}

}  // namespace ecckd
