// kernels_gas_fused.hip -- gas optics in one pass: optical depth of all gases AND (longwave) the
// three Planck source arrays, or (shortwave) the Rayleigh/ssa/g epilogue.
//
// Replaces, for one call of gas_optics_int / gas_optics_ext (src/gas_optics_ecckd.f90:381-473):
// calculate_optical_depth x ngas + the tau accumulation (:64-241, :348-374),
// calculate_planck_function x 3 (:245-289, :407-424) or the Rayleigh epilogue (:293-319, :455-460).
//
// Why one kernel: the interpolation is bound by fp64 VALU issue (61 fp64 operations and 21 16-byte
// LDS reads per cell pair), the Planck sources by HBM stores (24 B/cell).  Run back to back they
// take the sum; fused, most of the arithmetic hides under the stores (32 B/cell written: tau,
// lay_source, lev_source_inc, lev_source_dec).  The kernel writes what belongs to a layer: a block of layer j stores
// lev_source_dec of layer j+1 -- as a second store of the level's value, or, when the two level arrays are the views of
// one level buffer (include/ecckd_hip.h, "Level buffer"; FusedArgs::lev_gstride), as the SAME store: 24 B/cell written.
// The two sources that belong to no layer -- sfc_source and lev_source_dec of the first layer
// -- are planck_edge_kernel's (kernels_planck.hip), which launch_gas_fused puts on the stream behind this kernel: as work
// of the blocks of the first layer they cost every block 32 VGPRs, 36 B of scratch and half the compile time.
//
// Arithmetic ("fast" mode, the default): the four (eight) interpolation weights of a cell are
// multiplied out once per (column,layer) and every coefficient costs one FMA,
//     od_gas(g) = w_gas * (a00*c00 + a10*c10 + a01*c01 + a11*c11),   a_pt = tw_t * pw_p,
// the look_up_table gas is summed first and the other gases in gas_desc order.  That is the
// reference's formula re-associated: tau agrees with the reference-order kernels
// (kernels_tau.hip, kept as the bit-faithful mode) to a few ulp; the stated test tolerance is
// 1e-12 relative.  Per-gas clamping of negative optical depths (:234-238) is kept exactly:
// tables without negative entries (all ecCKD files) clamp the weight instead, tables with
// negative entries take the ANYCLAMP instantiation.  Planck sources are computed in the
// reference's order and are bit-identical.
//
// Mapping: lane -> column, block = kBlock columns of ONE layer (grid.y), LDS = slab of R pressure
// rows of every active table + the Planck table (or a window of it), row strides == 2 (mod 4)
// doubles.  Per segment of kSeg tiles a pre-pass finds the pressure-row (and Planck-row) range and
// places the slab; segments spanning more rows than the slab holds are walked once per slab
// position; waves with a lane outside the staged rows read the tables from global memory.
//
// The device code is gas_fused_body.hpp, shared with gas_roles_kernel (kernels_gas_roles.hip), the form of the fp64
// longwave launch in which tau waves and source waves share a block ("gas_wave_roles"); this file keeps gas_fused_kernel,
// the spread probe and the host side of every fused launch.
#include "gas_fused_body.hpp"

namespace ecckd {
namespace {

template <typename real>
__global__ void __launch_bounds__(256) spread_probe_kernel(const real *plev, int ncol, int nlay, real lp0, UDiv dlp_h, int np, int *count) {
  // both ends of the arrays (blockIdx.y): the call does not say which one is the surface, and the top contributes nothing
  const real *plev0 = plev + (long)ncol * (blockIdx.y ? nlay - 1 : 0), *plev1 = plev0 + ncol;
  const UDivT<real> dlp = make_udiv_t<real>(dlp_h);
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  int ip = -1;
  if (c < ncol) ip = pressure_point<real>(plev0[c], plev1[c], lp0, dlp, np).ip0;
  int lo = ip < 0 ? 0x7fffffff : ip, hi = ip;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = min(lo, __shfl_xor(lo, o));
    hi = max(hi, __shfl_xor(hi, o));
  }
  if ((threadIdx.x & 63) == 0 && hi - lo >= 2) atomicAdd(count, 1);
}

// The kernel: gas_fused_body (gas_fused_body.hpp) with every wave doing all the work of its 64 columns.
template <typename real, int GC, int NB, bool FULL, bool ANYCLAMP, int MODE, typename sreal = real, int BLOCK = kBlock>
__global__ void __launch_bounds__(BLOCK, (BLOCK > 512 ? 3 : sizeof(real) == 4 ? ECCKD_F32_WAVES : ECCKD_F64_WAVES)) gas_fused_kernel(const FusedArgs a) {
  gas_fused_body<real, GC, NB, FULL, ANYCLAMP, MODE, sreal, BLOCK, false>(a);
}

template <typename real, int GC, int NB, bool FULL, bool ANYCLAMP, int MODE, typename sreal = real>
hipError_t launch_one(const FusedArgs &a, size_t lds_bytes, hipStream_t s) {
  constexpr int kBlock = fused_block(MODE);
  auto k = gas_fused_kernel<real, GC, NB, FULL, ANYCLAMP, MODE, sreal, kBlock>;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k, dim3(a.tau.col_chunks, a.tau.nlay), dim3(kBlock), lds_bytes, s, a);
  return hipGetLastError();
}

int pick_nb(int nbil) {
  if (nbil <= 2) return 2;
  if (nbil <= 5) return 5;
  if (nbil <= 7) return 7;
  return kTauPassGases;
}

template <typename real, int MODE>
hipError_t launch_mode(const FusedArgs &a, size_t lds, int NBsel, bool anyclamp, hipStream_t s) {
  const int ng = a.tau.ng;
  if (anyclamp && ng % 4 == 0) return launch_one<real, 4, kTauPassGases, true, true, MODE>(a, lds, s);
  if (anyclamp) return launch_one<real, 4, kTauPassGases, false, true, MODE>(a, lds, s);
  if (NBsel == 2 && ng % 8 == 0) return launch_one<real, 8, 2, true, false, MODE>(a, lds, s);
  if (NBsel == 2 && ng % 4 == 0) return launch_one<real, 4, 2, true, false, MODE>(a, lds, s);
  if (NBsel == 2) return launch_one<real, 4, 2, false, false, MODE>(a, lds, s);
  if (NBsel == 7 && ng % 8 == 0) return launch_one<real, 8, 7, true, false, MODE>(a, lds, s);
  if (NBsel == 7 && ng % 4 == 0) return launch_one<real, 4, 7, true, false, MODE>(a, lds, s);
  if (NBsel == 5 && ng % 4 == 0) return launch_one<real, 4, 5, true, false, MODE>(a, lds, s);
  if (NBsel == 5) return launch_one<real, 4, 5, false, false, MODE>(a, lds, s);
  if (ng % 4 == 0) return launch_one<real, 4, kTauPassGases, true, false, MODE>(a, lds, s);
  return launch_one<real, 4, kTauPassGases, false, false, MODE>(a, lds, s);
}

// (FULL = true instantiations -- g-point count a multiple of the chunk, true for both longwave tables -- carry no
// per-g-point bounds checks and keep everything in registers; the FULL = false ones spill 13-108 VGPRs and only
// serve tables whose g-point count is not a multiple of 4, e.g. the 27 g-points of the shortwave table with
// more than 7 gases.)
// (GC, NB) of the instantiation launch_mode() will pick
// float32 image of the tables under a double kernel: instantiated for the full-chunk longwave shape of the ecCKD files
bool slab32_applies(int mode, int ng, int nbil, bool anyclamp) {
  return mode == MODE_LW && !anyclamp && ng % 8 == 0 && pick_nb(nbil) == 7;
}

void pick_shape(int ng, int nbil, bool anyclamp, int *GC, int *NB) {
  const int nb = pick_nb(nbil);
  if (anyclamp) { *GC = 4; *NB = kTauPassGases; }
  else if (nb == 2) { *GC = ng % 8 == 0 ? 8 : 4; *NB = 2; }
  else if (nb == 7 && ng % 8 == 0) { *GC = 8; *NB = 7; }
  else if (nb == 7 && ng % 4 == 0) { *GC = 4; *NB = 7; }
  else if (nb == 5) { *GC = 4; *NB = 5; }
  else { *GC = 4; *NB = kTauPassGases; }
}

}  // namespace

// Rows of the LDS slab for a fused launch that keeps `pl_rows` rows of the Planck table in LDS, or 0
// if it does not fit with at least `min_rows`.
// f32: 0 double arithmetic and tables, 1 float arithmetic and tables, 2 double arithmetic over the float32 image of the
// tables (FusedArgs::slab32).
int fused_slab_rows(int ng, int np, int nt, int nbil, int nv_lut, int pl_rows, int min_rows, int anyclamp, int f32, int block) {
  if (block <= 0) block = kBlock;
  int GC, NB;
  pick_shape(ng, nbil, anyclamp != 0, &GC, &NB);
  const int ngp = (ng + GC - 1) / GC * GC;
  const size_t esz = f32 ? sizeof(float) : sizeof(double);
  int R = 0;
  for (int r = 2; r <= np; ++r) {
    if (esz * (size_t)f_layout(ngp, np, nt, nbil, NB, nv_lut, r, pl_rows, f32 == 2 ? 2 : 1, block / 64).total <= (size_t)kLdsBudget) R = r;
    else break;
  }
  return R >= min_rows ? R : 0;
}

// Planck rows to stage for a fused longwave launch: the whole table if it fits next to >= 3 slab
// rows, else the largest window of the list that does (a segment of 4096 columns of one layer
// rarely spans more than ~70 K = 70 rows of the 1 K table); 0 = does not fit at all.
// ECCKD_PLANCK_WINDOW=<rows> forces a window (tests of the out-of-window path).
int fused_planck_rows(int ng, int np, int nt, int nbil, int nv_lut, int ntp, int anyclamp, int f32) {
  if (ntp < 2) return 0;
  if (const char *e = getenv("ECCKD_PLANCK_WINDOW")) {
    const int w = atoi(e);
    if (w >= 2 && w < ntp && fused_slab_rows(ng, np, nt, nbil, nv_lut, w, 3, anyclamp, f32) > 0) return w;
  }
  if (fused_slab_rows(ng, np, nt, nbil, nv_lut, ntp, 3, anyclamp, f32) > 0) return ntp;
  for (int w : {128, 96, 64, 48, 32, 16})
    if (w < ntp && fused_slab_rows(ng, np, nt, nbil, nv_lut, w, 3, anyclamp, f32) > 0) return w;
  return 0;
}

UDiv make_udiv(double d, int f32) {
  UDiv u;
  if (f32) d = (double)(float)d;   // the kernel works with the rounded divisor
  u.d = d;
  u.r = f32 ? (double)(1.f / (float)d) : 1. / d;   // correctly rounded reciprocal in the working precision
  unsigned long long bits;
  static_assert(sizeof(bits) == sizeof(d), "");
  __builtin_memcpy(&bits, &d, 8);
  bool all_ones = (bits & 0xFFFFFFFFFFFFFULL) == 0xFFFFFFFFFFFFFULL;
  if (f32) {
    const float df = (float)d;
    unsigned int b32;
    __builtin_memcpy(&b32, &df, 4);
    all_ones = (b32 & 0x7FFFFFu) == 0x7FFFFFu;
  }
  u.exact = (d == d) && d != 0. && (d - d == 0.) && !all_ones && (u.r - u.r == 0.) ? 1 : 0;
  return u;
}

// The gases of a pass whose mole fraction is one number for the whole call: scalar entries of gas_desc (get_vmr
// broadcasts them, src/gas_optics_ecckd.f90:351) and the none_ composite (:213-221).  Their optical depths are
//     od_k = simple_weight * m_k * bilinear(coefficient_k),   m_k = vmr_k | vmr_k - reference_k | 1,
// so their sum is simple_weight * bilinear(sum_k m_k * coefficient_k): one table, one slab slot, four LDS reads and five
// FMAs per g-point pair instead of that per gas.  The per-gas clamp od_k < 0 -> 0 (:234-238) is kept exactly as long as
// every od_k of a cell has the sign of simple_weight, i.e. for tables without negative entries and m_k >= 0 -- a gas
// below its reference concentration, a table with negative entries or a non-finite value keeps its own slot.
int merge_scalar_gases(TauArgs &t, int f32) {
  t.merge_slot = -1;
  t.nmerge = 0;
  int cand[kMaxSeq], ncand = 0;
  double mult[kMaxSeq];
  for (int s = 0; s < t.nbil; ++s) {
    const SeqGas &e = t.seq[t.bil_seq[s]];
    if (e.clamp) continue;
    double m;
    if (e.code == 0) m = 1.;
    else if (e.vmr) continue;
    else if (e.code == 3) m = f32 ? (double)((float)e.scalar - (float)e.ref) : e.scalar - e.ref;
    else m = f32 ? (double)(float)e.scalar : e.scalar;
    if (!(m >= 0.) || !(m - m == 0.)) continue;
    cand[ncand] = t.bil_seq[s];
    mult[ncand++] = m;
  }
  if (ncand < 2) return 0;
  int keep[kMaxSeq], nkeep = 0;
  for (int s = 0; s < t.nbil; ++s) {
    bool merged = false;
    for (int k = 0; k < ncand; ++k) merged |= cand[k] == t.bil_seq[s];
    if (!merged) keep[nkeep++] = t.bil_seq[s];
  }
  for (int s = 0; s < nkeep; ++s) { t.bil_seq[s] = keep[s]; t.seq[keep[s]].slot = s; }
  t.merge_slot = nkeep;
  t.bil_seq[nkeep] = cand[0];   // (never read for the merged slot)
  t.nbil = nkeep + 1;
  t.nmerge = ncand;
  for (int k = 0; k < ncand; ++k) { t.merge_seq[k] = cand[k]; t.merge_mult[k] = mult[k]; t.seq[cand[k]].slot = nkeep; }
  return ncand;
}

// Host-side decisions of a fused launch (slots, slab rows, Planck window, grid): everything but the
// launch itself, so that ecckd_gas_optics_plan() can report them without a GPU.
hipError_t prepare_gas_fused(FusedArgs &a, FusedPlan &plan) {
  TauArgs &t = a.tau;
  plan = FusedPlan{};
  a.ud_dlp = make_udiv(t.dlp, a.f32);
  a.ud_dt = make_udiv(t.dt, a.f32);
  a.ud_dlv = make_udiv(t.lut >= 0 ? t.seq[t.lut].d_log_vmr : 1., a.f32);
  a.ud_pdt = make_udiv(a.mode == MODE_LW ? a.pdt : 1., a.f32);
  const size_t esz = a.f32 ? sizeof(float) : sizeof(double);
  // working-precision arithmetic for the constants folded on the host
  auto sub = [&](double x, double y) { return a.f32 ? (double)((float)x - (float)y) : x - y; };
  for (int s = 0; s <= kTauPassGases; ++s) {
    const int k = s < kTauPassGases ? (s < t.nbil ? t.bil_seq[s] : -1) : t.lut;
    SlotArgs &o = a.slot[s];
    o = SlotArgs{t.zero, 0, 0u, 0., 0.};   // unused slot or scalar gas: the load reads a zero word of the model
    if (s < kTauPassGases && s == t.merge_slot) {
      o.beta = 1.;                         // the multipliers are in the merged table: weight = simple_weight
    } else if (k >= 0) {
      const SeqGas &e = t.seq[k];
      const bool arr = e.vmr != nullptr;
      if (arr) {
        if (e.cs < 0 || (unsigned long long)e.cs * (unsigned long long)(t.ncol > 0 ? t.ncol : 1) * esz >= 0xFFFFFFF0ull)
          return hipErrorInvalidValue;   // column stride of a vmr array beyond 32-bit byte offsets
        o.vmr = e.vmr; o.ls = e.ls; o.cs_bytes = (unsigned)((unsigned long long)e.cs * esz);
      }
      switch (e.code) {
        case 0: o.alpha = 0.; o.beta = 1.; break;                                     // none_: weight = simple_weight (:213-221)
        case 3: o.alpha = arr ? 1. : 0.; o.beta = arr ? -e.ref : sub(e.scalar, e.ref); break;   // relative_linear (:146)
        default: o.alpha = arr ? 1. : 0.; o.beta = arr ? 0. : e.scalar; break;        // linear, look_up_table (:148)
      }
    }
  }
  if (t.ncol <= 0 || t.nlay <= 0) { plan.empty = 1; return hipSuccess; }
  if (t.nseq > kTauPassGases) return hipErrorInvalidValue;
  // separate level arrays unless the caller says otherwise (FusedArgs::lev_gstride); no single-precision level buffer
  const size_t plane = (size_t)t.ncol * (size_t)t.nlay;
  if (a.lev_gstride <= 0) a.lev_gstride = (long long)plane;
  if (a.f32 && (size_t)a.lev_gstride != plane) return hipErrorInvalidValue;
  // store_pair() addresses a plane pair with a 32-bit byte offset: the larger of the two strides counts
  const size_t widest = (size_t)a.lev_gstride > plane ? (size_t)a.lev_gstride : plane;
  if ((widest + (size_t)t.ncol) * (a.f32 ? sizeof(float) : sizeof(double)) >= (size_t)0xFFFFFFF0u)
    return hipErrorInvalidValue;
  const int nv_lut = t.lut >= 0 ? t.seq[t.lut].nv : 0;
  bool anyclamp = false;
  for (int k = 0; k < t.nseq; ++k) anyclamp |= t.seq[k].clamp != 0;
  if (a.mode == MODE_LW) {
    a.pw = fused_planck_rows(t.ng, t.np, t.nt, t.nbil, nv_lut, a.ntp, anyclamp, a.f32);
    if (a.pw < 2) return hipErrorInvalidValue;   // the caller checks fused_planck_rows() first
  } else {
    a.pw = 0;
  }
  int GC, NB;
  pick_shape(t.ng, t.nbil, anyclamp, &GC, &NB);
  const int ngp = (t.ng + GC - 1) / GC * GC;
  // float32 image of the tables under a double kernel: only the instantiations built for it (slab32_applies)
  if (a.slab32 && !(a.f32 == 0 && slab32_applies(a.mode, t.ng, t.nbil, anyclamp) && t.merge_slot < 0)) a.slab32 = 0;
  const int store = a.f32 ? 1 : (a.slab32 ? 2 : 0);
  if (a.mode == MODE_LW && store == 2) a.pw = fused_planck_rows(t.ng, t.np, t.nt, t.nbil, nv_lut, a.ntp, anyclamp, 2);
  const int block = fused_block(a.mode);   // columns of a tile (= threads of a block, but for the wave-roles form)
  int threads = block;
  t.R = fused_slab_rows(t.ng, t.np, t.nt, t.nbil, nv_lut, a.pw, 0, anyclamp, store, threads);
  // "gas_wave_roles": the fp64 longwave launch over the fp64 slab, full chunks, a shape gas_roles_kernel is instantiated for
  // -- and only while the four extra waves' words of reduction scratch leave the slab the rows it has without them
  if (a.wave_roles) {
    const bool can = a.mode == MODE_LW && store == 0 && !anyclamp && t.ng % GC == 0 && gas_roles_applies(GC, NB) &&
                     fused_slab_rows(t.ng, t.np, t.nt, t.nbil, nv_lut, a.pw, 0, anyclamp, store, kRolesThreads) == t.R;
    a.wave_roles = can && (a.wave_roles > 0 || gas_roles_default(GC, NB)) ? 1 : 0;
    if (a.wave_roles) threads = kRolesThreads;
  }
  const size_t lds = (store ? sizeof(float) : sizeof(double)) *
                     (size_t)f_layout(ngp, t.np, t.nt, t.nbil, NB, nv_lut, t.R, a.pw, store == 2 ? 2 : 1, threads / 64).total;
  if (lds > (size_t)kLdsBudget) return hipErrorInvalidValue;
  // one block per CU (LDS-bound): a block count that is a multiple of the 256 CUs keeps the last
  // round of blocks full
  const long ntiles = ((long)t.ncol + block - 1) / block;
  long chunks = 1;
  while ((chunks * t.nlay) % 256 != 0 && chunks < 256) ++chunks;
  while (chunks * 2 * kSeg <= ntiles && chunks * t.nlay < 2048) chunks *= 2;
  if (chunks * kSeg > ntiles) chunks = (ntiles + kSeg - 1) / kSeg;
  if (chunks < 1) chunks = 1;
  t.col_chunks = (int)chunks;
  {
    long per_block = (ntiles + chunks - 1) / chunks;
    t.seg = (int)(per_block < kSeg ? kSeg : (per_block > kSegMax ? kSegMax : per_block));
  }
  if (a.f32 && a.mode == MODE_TAU) return hipErrorNotSupported;   // single precision: the one-pass longwave and shortwave paths
  plan.lds_bytes = lds;
  plan.anyclamp = anyclamp ? 1 : 0;
  plan.GC = GC; plan.NB = NB; plan.merged = t.merge_slot >= 0 ? t.nmerge : 0;
  plan.slab_rows = t.R; plan.planck_rows = a.pw; plan.col_chunks = t.col_chunks;
  return hipSuccess;
}

namespace {
hipError_t launch_gas_fused_layers(FusedArgs &a, hipStream_t s);
}

// The longwave mode is two kernels on the stream: gas_fused_kernel for everything that belongs to a layer, then
// planck_edge_kernel for sfc_source and the top plane of lev_source_dec -- once per call, whichever of the fp64-slab and
// float32-image forms the spread probe picks.
hipError_t launch_gas_fused(FusedArgs &a, hipStream_t s) {
  const hipError_t e = launch_gas_fused_layers(a, s);
  if (e != hipSuccess || a.mode != MODE_LW) return e;
  return launch_planck_edge(a, s);   // (a.ud_pdt: filled by prepare_gas_fused)
}

namespace {
// the fp64 longwave launch over the fp64 slab: gas_roles_kernel where prepare_gas_fused chose it, else gas_fused_kernel
hipError_t launch_lw_f64(const FusedArgs &a, const FusedPlan &plan, hipStream_t s) {
  if (a.wave_roles) return launch_gas_roles(a, plan.GC, plan.NB, plan.lds_bytes, s);
  return launch_mode<double, MODE_LW>(a, plan.lds_bytes, pick_nb(a.tau.nbil), plan.anyclamp != 0, s);
}

hipError_t launch_gas_fused_layers(FusedArgs &a, hipStream_t s) {
  FusedPlan plan;
  if (a.slab32 == 2) {   // auto: spread probe, then both forms; the one the probe does not choose returns at once
    FusedArgs b = a;
    b.slab32 = 1;
    FusedPlan pb;
    hipError_t eb = prepare_gas_fused(b, pb);
    if (eb == hipSuccess && !pb.empty && b.slab32 == 1 && a.choose_buf) {
      a.slab32 = 0;
      eb = prepare_gas_fused(a, plan);
      if (eb != hipSuccess) return eb;
      const TauArgs &t = a.tau;
      eb = hipMemsetAsync(a.choose_buf, 0, sizeof(int), s);
      if (eb != hipSuccess) return eb;
      const long nw = ((long)t.ncol + 63) / 64;
      hipLaunchKernelGGL(spread_probe_kernel<double>, dim3((unsigned)((t.ncol + 255) / 256), t.nlay > 1 ? 2 : 1), dim3(256), 0, s,
                         t.plev, t.ncol, t.nlay, t.lp0, a.ud_dlp, t.np, a.choose_buf);
      eb = hipGetLastError();
      if (eb != hipSuccess) return eb;
      a.choose = b.choose = a.choose_buf;
      a.choose_total = b.choose_total = (int)(nw > 0x7fffffff ? 0x7fffffff : nw);
      eb = launch_lw_f64(a, plan, s);
      if (eb != hipSuccess) return eb;
      return launch_one<double, 8, 7, true, false, MODE_LW, float>(b, pb.lds_bytes, s);
    }
    a.slab32 = 0;   // no float32 form for this shape (or no room for the probe's counter): the fp64 slab
  }
  const hipError_t e = prepare_gas_fused(a, plan);
  if (e != hipSuccess || plan.empty) return e;
  const TauArgs &t = a.tau;
  const bool anyclamp = plan.anyclamp != 0;
  if (a.slab32 && !a.f32) return launch_one<double, 8, 7, true, false, MODE_LW, float>(a, plan.lds_bytes, s);
  if (a.f32 && a.mode == MODE_SW) return launch_mode<float, MODE_SW>(a, plan.lds_bytes, pick_nb(t.nbil), anyclamp, s);
  if (a.f32) return launch_mode<float, MODE_LW>(a, plan.lds_bytes, pick_nb(t.nbil), anyclamp, s);
  if (a.mode == MODE_LW) return launch_lw_f64(a, plan, s);
  if (a.mode == MODE_SW) return launch_mode<double, MODE_SW>(a, plan.lds_bytes, pick_nb(t.nbil), anyclamp, s);
  return launch_mode<double, MODE_TAU>(a, plan.lds_bytes, pick_nb(t.nbil), anyclamp, s);
}
}  // namespace

}  // namespace ecckd
