// kernels_aerosol_optics.hip -- aerosol optics: species type, particle size, mass and relative humidity per (column,
// layer) to the particulate optical properties tau, ssa, g (or the absorption optical depth alone) on the model's bands,
// several species summed in one call and, with `accumulate`, added onto planes that already hold the clouds.
//
// The counterpart in RTE-RRTMGP is ty_aerosol_optics_rrtmgp_merra%aerosol_optics [RTE-ext:
// extensions/aerosols/mo_aerosol_optics_rrtmgp_merra.F90; the library is not part of the reference tree].  The definition
// is this project's own, spelt operation by operation in include/ecckd_hip.h (ecckd_aerosol_optics); every expression
// here keeps that order, and the build has FMA contraction off, so the results are those of an IEEE evaluation of the
// formulas in the precision of the call.
//
// Mapping (gfx950): a streaming kernel judged by bytes moved over time.  One lane owns a (column, layer) cell, the column
// fastest.  It reads its relative humidity and, per species, type, mass and size once, forms the
// humidity interval and weight once per cell and the table entry once per species, then walks the bands with the species
// as the inner loop: T, TS, TSG (or A) stay in registers and every store of a wave is one full coalesced line of a band
// plane.  The per-species state (an entry index and the mass) lives in registers: the kernel is instantiated for 1, 2, 4,
// 8 and 16 species (the next size up is taken, the slots beyond nspec are skipped uniformly); beyond 16 species a
// compatibility instantiation re-forms the entry inside the band loop (the inputs then come from L2 once per band).
// 256 threads per block, one wave per SIMD: the launch bounds ask the compiler for kAoBlocksPerCu(NS) waves per SIMD (8 up
// to two species, 4 up to eight and for the compatibility instantiation, 2 for sixteen, whose state alone is 48
// registers in fp64), and the grid is that many blocks per CU (or as many as the LDS image allows) -- what is resident at
// a time -- with the rest of the cells by grid stride.
// Tables: per precision one image of (value, slope) pairs, [quantity: ext, ssa, asy][band][entry], where the
// kAoEntries(nbin, nrh) entries of a (quantity, band) row are, in this order: dust[nbin], salt[nbin][nrh-1], sulfate[nrh-1],
// hydrophilic black carbon[nrh-1], hydrophilic organic carbon[nrh-1], hydrophobic black carbon, hydrophobic organic carbon
// (the humidity-independent entries carry a slope of 0 that is never read into the arithmetic: the value is selected).
// A species of a cell therefore needs one entry index, and the three quantities of a band are three reads one quantity
// stride apart -- a 128-bit read each in fp64, 64-bit in float.  While the image fits kAerosolOpticsLdsBytes a block copies
// it into LDS, and only once a cell of the block is active; larger images are read in place through L2.  The humidity
// levels, their differences and the bin limits (the "head", 3*nrh-1+2*nbin reals at most) are read with wave-uniform
// addresses from global memory on both routes.
// A wave ballot per species gives a mask of the species some lane of the wave holds: the others are skipped, so a clear
// wave reads no table and no level, and a species plane that is uniformly one type touches one group of entries.  Lanes
// are safe whatever their inputs hold: a type outside 1..7 is "none", the interval index is a count bounded by nrh-2,
// the bin comes from comparisons against the limits, and an inactive species is not computed at all.
#include "kernels.hpp"

namespace ecckd {
namespace {

constexpr int kAoBlock = 256;

template <typename real> __host__ __device__ constexpr real ao_eps() {   // epsilon(1._wp)
  return sizeof(real) == 4 ? real(1.1920928955078125e-07f) : real(2.220446049250313e-16);
}
// max(eps, x): x where x > eps, else eps (a NaN gives eps; the numerators carry the NaN on)
template <typename real> __device__ __forceinline__ real ao_floor(real x) { return x > ao_eps<real>() ? x : ao_eps<real>(); }
// the floor of ecckd_increment's denominators (kernels_optical_props.hip)
template <typename real> __device__ __forceinline__ real inc_floor(real x) { return x > op_eps<real>() ? x : op_eps<real>(); }

// The 0-based entry of a species in a (quantity, band) row, or -1 where the species is not active.  i0: the 0-based
// humidity interval of the cell.  lims: bin_lims(2,nbin).  The size r matters for dust and sea salt only.
template <typename real>
__device__ __forceinline__ int species_entry(int k, real m, real r, int i0, int nbin, int nrh, const real *__restrict__ lims) {
  if (!(k >= 1 && k <= 7 && m > real(0))) return -1;
  const int nint = nrh - 1, rh0 = nbin * nrh;
  if (k <= 2) {
    int bin = -1;
    for (int b = nbin - 1; b >= 0; --b)
      if (lims[2 * b] <= r && r < lims[2 * b + 1]) bin = b;   // (the first such bin wins; a NaN is in none)
    if (bin < 0) return -1;
    return k == 1 ? bin : nbin + bin * nint + i0;
  }
  switch (k) {
    case 3: return rh0 + i0;
    case 4: return rh0 + nint + i0;
    case 6: return rh0 + 2 * nint + i0;
    case 5: return rh0 + 3 * nint;
    default: return rh0 + 3 * nint + 1;
  }
}

// NS > 0: up to NS species, their state in registers.  NS == 0: any number, the state re-formed per band.
template <typename real, bool TWO_STREAM, bool LDS, int NS>
__global__ void __launch_bounds__(kAoBlock, kAoBlocksPerCu(NS)) aerosol_optics_kernel(const AerosolOpticsArgs a) {
  extern __shared__ __align__(16) unsigned char ao_smem[];
  typedef CloudLutPair<real> Pair;
  constexpr int kQuantities = TWO_STREAM ? 3 : 2;   // (the one-scalar form reads no asymmetry)
  constexpr int kSlots = NS > 0 ? NS : 1;
  const int nbin = a.nbin, nrh = a.nrh, nspec = a.nspec;
  const int nent = kAoEntries(nbin, nrh);
  const size_t qstride = (size_t)a.nband * nent;    // pairs of one quantity
  const Pair *img = static_cast<const Pair *>(a.image);
  if constexpr (LDS) img = reinterpret_cast<const Pair *>(ao_smem);
  const real *__restrict__ lev = static_cast<const real *>(a.head);   // levels[nrh], d[nrh-1], lims[2*nbin]
  const real *__restrict__ dlev = lev + nrh;
  const real *__restrict__ lims = dlev + (nrh - 1);
  const int *type = a.type;
  const real *size = reinterpret_cast<const real *>(a.size), *mass = reinterpret_cast<const real *>(a.mass),
             *relhum = reinterpret_cast<const real *>(a.relhum);
  real *tau = reinterpret_cast<real *>(a.tau), *ssa = reinterpret_cast<real *>(a.ssa), *g = reinterpret_cast<real *>(a.g);
  const size_t ncell = (size_t)a.ncol * a.nlay;
  const int rh_lo = nbin, rh_hi = nbin * nrh + 3 * (nrh - 1);   // entries [rh_lo, rh_hi) depend on the humidity
  [[maybe_unused]] bool staged = false;                         // (the same in every thread of the block)

  for (size_t base = (size_t)blockIdx.x * kAoBlock; base < ncell; base += (size_t)gridDim.x * kAoBlock) {
    const size_t cell = base + threadIdx.x;
    const bool live = cell < ncell;
    // which species could be active here (before the bin is known): decides staging and whether the levels are read
    // (the sizes are read here too, with the types and masses, so that all reads of a cell are in flight together: read
    // where the type is known to need them they are one dependent round trip to memory per species)
    int kk[kSlots];
    real ms[kSlots], rs[kSlots];
    bool maybe = false;
    if constexpr (NS > 0) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        kk[s] = 0; ms[s] = real(0); rs[s] = real(0);
        if (s < nspec && live) { kk[s] = type[cell + ncell * s]; ms[s] = mass[cell + ncell * s]; rs[s] = size[cell + ncell * s]; }
        maybe = maybe || (kk[s] >= 1 && kk[s] <= 7 && ms[s] > real(0));
      }
    } else {
      for (int s = 0; s < nspec && live; ++s) {
        const int k = type[cell + ncell * s];
        maybe = maybe || (k >= 1 && k <= 7 && mass[cell + ncell * s] > real(0));
      }
    }
    if constexpr (LDS) {
      if (!staged && __syncthreads_or(maybe)) {
        Pair *sm = reinterpret_cast<Pair *>(ao_smem);
        const Pair *gi = static_cast<const Pair *>(a.image);
        for (size_t i = threadIdx.x; i < kQuantities * qstride; i += kAoBlock) sm[i] = gi[i];
        __syncthreads();
        staged = true;
      }
    }
    const bool any = __ballot(maybe) != 0ull;   // false: a clear wave, which reads no level and no table
    // the humidity interval and weight, once per cell
    int i0 = 0;
    real w = real(0);
    if (any) {
      const real rh = live ? relhum[cell] : real(0);
      for (int j = 1; j < nrh - 1; ++j) i0 += rh >= lev[j] ? 1 : 0;   // (a NaN counts nothing)
      w = (rh - lev[i0]) / dlev[i0];
      w = w > real(0) ? w : real(0);
      w = w < real(1) ? w : real(1);
    }
    // the entry of each species, once per species, and the species some lane of the wave holds
    int ent[kSlots];
    [[maybe_unused]] unsigned held = 0u;
    if constexpr (NS > 0) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        ent[s] = -1;
        if (!any) continue;
        ent[s] = species_entry<real>(kk[s], ms[s], rs[s], i0, nbin, nrh, lims);
        if (__ballot(ent[s] >= 0) != 0ull) held |= 1u << s;
      }
    }
    for (int b = 0; b < a.nband; ++b) {
      // the band's rows of the three quantities: wave-uniform bases, so a lane's address is a base and a 32-bit entry
      const Pair *row_ext = img + (size_t)b * nent, *row_ssa = row_ext + qstride;
      [[maybe_unused]] const Pair *row_asy = row_ssa + qstride;
      real T = real(0), TS = real(0), TSG = real(0), A = real(0);
      auto add = [&](int e, real m) {
        if (e < 0) return;   // inactive: t = ts = tsg = +0, and x + (+0) leaves every sum as it is
        const bool rhdep = e >= rh_lo && e < rh_hi;
        const Pair pe = row_ext[(unsigned)e], ps = row_ssa[(unsigned)e];
        const real v_ext = rhdep ? pe.value + w * pe.slope : pe.value;
        const real v_ssa = rhdep ? ps.value + w * ps.slope : ps.value;
        const real t = m * v_ext;
        const real ts = t * v_ssa;
        if constexpr (TWO_STREAM) {
          const Pair pa = row_asy[(unsigned)e];
          const real v_asy = rhdep ? pa.value + w * pa.slope : pa.value;
          const real tsg = ts * v_asy;
          T += t; TS += ts; TSG += tsg;
        } else {
          A += (t - ts);
        }
      };
      if constexpr (NS > 0) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          if (held & (1u << s)) add(ent[s], ms[s]);
          // four species' table reads in flight at a time: without the fence the scheduler gathers the reads of all NS
          // species ahead of the arithmetic
          if constexpr (NS > 4) if (s % 4 == 3) __builtin_amdgcn_sched_barrier(0);
        }
      } else {
        for (int s = 0; s < nspec && live && any; ++s) {
          const size_t at = cell + ncell * s;
          const real m = mass[at];
          add(species_entry<real>(type[at], m, size[at], i0, nbin, nrh, lims), m);
        }
      }
      if (!live) continue;
      const size_t q = cell + ncell * b;
      if constexpr (TWO_STREAM) {
        const real t2 = T;
        const real s2 = TS / ao_floor(T);
        const real g2 = TSG / ao_floor(TS);
        if (!a.accumulate) {
          tau[q] = t2; ssa[q] = s2; g[q] = g2;
        } else {   // increment_2stream_by_2stream, operation for operation
          const real t1 = tau[q], s1 = ssa[q];
          const real tscat2 = t2 * s2;
          const real tsg2 = tscat2 * g2;
          const real tau12 = t1 + t2;
          const real tscat1 = t1 * s1;
          const real tauscat12 = tscat1 + tscat2;
          g[q] = (tscat1 * g[q] + tsg2) / inc_floor(tauscat12);
          ssa[q] = tauscat12 / inc_floor(tau12);
          tau[q] = tau12;
        }
      } else {
        tau[q] = a.accumulate ? tau[q] + A : A;   // increment_1scalar_by_1scalar
      }
    }
  }
}

template <typename real, bool TWO_STREAM, bool LDS>
hipError_t launch_ns(const AerosolOpticsArgs &a, unsigned blocks, size_t lds, hipStream_t s) {
  typedef void (*K)(const AerosolOpticsArgs);
  const int n = a.nspec;
  const K k = n <= 1 ? aerosol_optics_kernel<real, TWO_STREAM, LDS, 1>
            : n <= 2 ? aerosol_optics_kernel<real, TWO_STREAM, LDS, 2>
            : n <= 4 ? aerosol_optics_kernel<real, TWO_STREAM, LDS, 4>
            : n <= 8 ? aerosol_optics_kernel<real, TWO_STREAM, LDS, 8>
            : n <= kAoMaxRegisterSpecies ? aerosol_optics_kernel<real, TWO_STREAM, LDS, kAoMaxRegisterSpecies>
                                         : aerosol_optics_kernel<real, TWO_STREAM, LDS, 0>;
  hipLaunchKernelGGL(k, dim3(blocks), dim3(kAoBlock), lds, s, a);
  return hipGetLastError();
}

template <typename real>
hipError_t launch_t(const AerosolOpticsArgs &a, hipStream_t s) {
  const bool two = a.ssa != nullptr;
  const size_t image = aerosol_optics_image_bytes(a.nband, a.nbin, a.nrh, two, sizeof(real) == 4);
  const bool lds = image <= kAerosolOpticsLdsBytes;
  const unsigned blocks = aerosol_optics_grid(a.ncol, a.nlay, a.nspec, a.cus, lds ? image : 0);
  if (two) return lds ? launch_ns<real, true, true>(a, blocks, image, s) : launch_ns<real, true, false>(a, blocks, 0, s);
  return lds ? launch_ns<real, false, true>(a, blocks, image, s) : launch_ns<real, false, false>(a, blocks, 0, s);
}

}  // namespace

size_t aerosol_optics_image_bytes(int nband, int nbin, int nrh, bool two_stream, bool f32) {
  const size_t pairs = (size_t)(two_stream ? 3 : 2) * nband * (size_t)kAoEntries(nbin, nrh);
  return pairs * 2 * (f32 ? sizeof(float) : sizeof(double));
}

unsigned aerosol_optics_grid(int ncol, int nlay, int nspec, int cus, size_t lds_image_bytes) {
  const size_t ncell = (size_t)ncol * nlay, want = (ncell + kAoBlock - 1) / kAoBlock;
  const size_t by_regs = (size_t)kAoBlocksPerCu(nspec > kAoMaxRegisterSpecies ? 0 : nspec);
  const size_t by_lds = lds_image_bytes > 0 ? (size_t)kLdsBudget / lds_image_bytes : by_regs;
  const size_t resident = (size_t)(cus > 0 ? cus : 256) * (by_lds < by_regs ? by_lds : by_regs);
  return (unsigned)(want > resident ? resident : want);
}

hipError_t launch_aerosol_optics(const AerosolOpticsArgs &a, hipStream_t s) {
  if (a.ncol <= 0 || a.nlay <= 0) return hipSuccess;
  if (a.nband < 1 || a.nbin < 1 || a.nrh < 2 || a.nspec < 1 || (a.ssa == nullptr) != (a.g == nullptr)) return hipErrorInvalidValue;
  return a.f32 ? launch_t<float>(a, s) : launch_t<double>(a, s);
}

}  // namespace ecckd
