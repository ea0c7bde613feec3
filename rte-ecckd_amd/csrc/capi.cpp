// capi.cpp -- the C ABI of include/ecckd_hip.h: model construction, gas_optics (LW/SW) and the
// RTE solvers, in device-pointer and host-pointer flavours.  Host logic only; the arithmetic
// is in kernels_*.hip.  There is deliberately no CPU fallback: a missing/unusable GPU is an
// error returned to the caller.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ecckd_hip.h"
#include "kernels.hpp"
#include "model.hpp"

namespace {

thread_local std::string g_err;

int fail(const std::string &msg) {
  g_err = msg;
  return 1;
}
}  // namespace

namespace ecckd {
int set_last_error(const std::string &msg) { return fail(msg); }   // for nc_capi.cpp
}  // namespace ecckd

namespace {

#define HIPCHK(expr)                                                                     \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

// trim() of a blank- or NUL-padded character(len=32) record
std::string trim_name(const char *p) {
  size_t n = 0;
  while (n < ECCKD_NAME_LEN && p[n] != '\0') ++n;
  while (n > 0 && p[n - 1] == ' ') --n;
  return std::string(p, n);
}

// Grow-only device arena of the solver calls on host arrays, one per device (Stage; the model calls use the model's own).
struct Arena {
  std::mutex mu;
  void *p = nullptr;
  size_t bytes = 0;
};
Arena g_solver_arena[16];

// Scratch rings of the solvers (rte_sw always; rte_lw beyond 96 layers), stream-ordered: a launch takes the
// block that belongs to (device, stream).  Work on one stream is ordered, so consecutive calls on a stream
// reuse its block without any synchronisation, and calls on different streams never share one -- the call
// stays asynchronous and can be captured in a HIP graph.
// Lifetime rules:
//  * A call holds a ScratchLease from the moment it asks for a block until it has launched its kernels.  A block that
//    has become too small is freed at once only when nothing can still refer to it: no other call holds a lease on this
//    device (another host thread between "got the pointer" and "launched"), the stream has drained, and the block was
//    never handed to a captured call.  Otherwise it is retired and released by ecckd_release_scratch() or at exit.
//  * A block handed out while its stream was being captured belongs to that graph from then on: the next eager call on
//    the stream gets a fresh block (the graph may be replayed on any stream, concurrently with eager calls).
//  * A caller that wants no allocation inside the library at all hands its own buffer over with
//    ecckd_set_stream_scratch(); ecckd_release_scratch() leaves such entries alone.
struct ScratchPool {
  std::mutex mu;
  struct Block { void *p = nullptr; size_t bytes = 0; bool caller_owned = false; bool captured = false; };
  std::map<hipStream_t, Block> live;
  std::vector<void *> retired;
  int leases = 0;             // calls between acquiring a block and having launched on it
};
ScratchPool g_scratch_pool[16];
ScratchPool g_flag_pool[16];   // one small block per (device, stream): the counter of the gas-optics spread probe ("gas_slab_f32" = auto)

struct ScratchLease {
  ScratchPool *pool = nullptr;
  ScratchLease() = default;
  ScratchLease(const ScratchLease &) = delete;
  ScratchLease &operator=(const ScratchLease &) = delete;
  void take(ScratchPool &p) {   // (p.mu held by the caller)
    if (!pool) { pool = &p; ++p.leases; }
  }
  ~ScratchLease() {
    if (!pool) return;
    std::lock_guard<std::mutex> lock(pool->mu);
    --pool->leases;
  }
};

bool stream_is_capturing(hipStream_t stream) {
  hipStreamCaptureStatus c = hipStreamCaptureStatusNone;
  return stream && hipStreamIsCapturing(stream, &c) == hipSuccess && c != hipStreamCaptureStatusNone;
}

// Returns the scratch block of (device, stream) with at least `need` bytes in *out; `lease` keeps it safe from other
// host threads until the caller has launched (it must outlive the launches of the call).
int stream_scratch(int device, hipStream_t stream, size_t need, void **out, ScratchLease &lease, ScratchPool *pools = g_scratch_pool) {
  ScratchPool &pool = pools[device];
  std::lock_guard<std::mutex> lock(pool.mu);
  lease.take(pool);
  ScratchPool::Block &b = pool.live[stream];
  const bool capturing = stream_is_capturing(stream);
  if (b.captured && !capturing && !b.caller_owned) {   // the block belongs to a captured graph: eager calls move on
    pool.retired.push_back(b.p);
    b = ScratchPool::Block{};
  }
  if (b.bytes >= need) {
    if (capturing && !b.caller_owned) b.captured = true;
    *out = b.p;
    return 0;
  }
  if (b.caller_owned)
    return fail("ecckd: the scratch buffer set with ecckd_set_stream_scratch is too small for this call (" +
                std::to_string(need) + " bytes needed: ecckd_rte_lw_scratch_bytes / ecckd_rte_sw_scratch_bytes, or "
                "ecckd_rte_lw_tail_scratch_bytes / ecckd_rte_sw_tail_scratch_bytes with the tail splits)");
  if (capturing)
    return fail("ecckd: this call needs " + std::to_string(need) + " bytes of solver scratch on a stream that is being "
                "captured; run the call once on this stream before the capture, or hand a buffer over with "
                "ecckd_set_stream_scratch (no allocation happens inside a capture)");
  void *p = nullptr;
  size_t want = need + need / 4;   // head room: a slightly larger shape on the same stream does not reallocate
  if (hipMalloc(&p, want) != hipSuccess) {
    (void)hipGetLastError();       // the refused request must not surface as the next launch's error
    want = need;
    HIPCHK(hipMalloc(&p, want));
  }
  if (b.p) {   // the outgrown block: see the lifetime rules above
    if (!b.captured && pool.leases == 1 && hipStreamQuery(stream) == hipSuccess) (void)hipFree(b.p);
    else pool.retired.push_back(b.p);
    (void)hipGetLastError();       // hipStreamQuery's hipErrorNotReady is not an error of this call
  }
  b.p = p; b.bytes = want; b.caller_owned = false; b.captured = false;
  *out = p;
  return 0;
}

// Same block, for a use the call can do without (the tail split of rte_lw): nullptr instead of an error when the block
// cannot be provided (caller-owned block too small, stream being captured, allocation refused).
void *stream_scratch_optional(int device, hipStream_t stream, size_t need, ScratchLease &lease, ScratchPool *pools = g_scratch_pool) {
  {
    ScratchPool &pool = pools[device];
    std::lock_guard<std::mutex> lock(pool.mu);
    const auto it = pool.live.find(stream);
    const bool capturing = stream_is_capturing(stream);
    const bool have = it != pool.live.end() && it->second.bytes >= need;
    if (!have) {
      if (it != pool.live.end() && it->second.caller_owned) return nullptr;
      if (capturing) return nullptr;
    }
  }
  void *p = nullptr;
  if (stream_scratch(device, stream, need, &p, lease, pools)) {
    (void)hipGetLastError();
    return nullptr;
  }
  return p;
}

// SIMDs of the device = waves of the register-resident LW solver that run at a time (one wave owns a SIMD)
int simd_slots(int device) {
  static std::atomic<int> cached[16];
  int v = cached[device].load();
  if (v > 0) return v;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) return 0;
  cached[device].store(4 * cus);
  return 4 * cus;
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// Single precision: the *_f32 entry points cast their float pointers to `double *` (dp) and pass f32 = true down;
// Stage below takes that flag to size its rooms and copies and the kernels are launched with f32 = 1.  Data
// pointers keep their `double *` static type on the way through (they are only passed on, never indexed).
size_t esz(bool f32) { return f32 ? sizeof(float) : sizeof(double); }
inline const double *dp(const float *p) { return reinterpret_cast<const double *>(p); }
inline double *dp(float *p) { return reinterpret_cast<double *>(p); }
inline const double *const *dp(const float *const *p) { return reinterpret_cast<const double *const *>(p); }

// ecckd_sw_fluxes: the shortwave solver derives ssa / g / toa itself (RteSwArgs::derive) and works in `room` inside
// ecckd_sw_fluxes' own scratch block (sw_fluxes_solver_bytes): the partial sums of the layer-systolic solver, or the
// scratch ring of the two-pass solver with its partial sums behind it
// part_*: ecckd_sw_fluxes_allsky -- the particulate band optics the solver adds to the gas optics (RteSwArgs::allsky), or null
struct SwDerive {
  const double *plev, *rayleigh, *solar, *toa_scale; double gw; double *room;
  const double *part_tau = nullptr, *part_ssa = nullptr, *part_g = nullptr;
  const unsigned long long *part_mask = nullptr;   // ecckd_sw_fluxes_allsky_mcica (RteSwArgs::part_mask), or null
  int mask_first = -1;                             // ecckd_sw_flux_bands: >= 0, the model's g-point of the launch's first (RteSwArgs::mask_first)
  const float *part_scaling = nullptr;             // ecckd_sw_flux_scaled (RteSwArgs::part_scaling): the two-pass solver, whatever "sw_solver" says
};
// What a public entry point asks of the solver implementations besides its arguments.
struct Call {
  bool f32 = false;
  int band = -1;                      // the per-band solvers: band of every g-point of the sub-range (else band2gpt)
  bool shared_levels = false;         // ecckd_rte_lw_shared_levels
  const SwDerive *derive = nullptr;   // ecckd_sw_fluxes
};
// ecckd_gas_optics_plan(): gas_optical_depth_dev() given one records its decisions here and launches nothing
struct PlanRecord {
  const int *is_scalar = nullptr;   // per gas of the list: its mole fraction would be passed as one number
  int npass = 0, first_fused = 0, planck_fused = 0;
  ecckd::FusedPlan first;
};

// :107 / :314  1./(gravity*0.001*dry_air_molar_mass) with default-real literals (:51-52); with wp = float in single
// precision
double gw(bool f32) {
  return f32 ? (double)(1.f / (9.80665f * 0.001f * 28.970f)) : 1. / ((double)9.80665f * (double)0.001f * (double)28.970f);
}
// the model table at `off` (in elements), in the fp64 image or its float32 copy
const double *table(const ecckd_model *m, size_t off, bool f32) {
  return f32 ? reinterpret_cast<const double *>(m->dbuf32 + off) : m->dbuf + off;
}

// Arithmetic mode (ecckd_set_arithmetic): 0 = fast (fused kernel, re-associated FMAs),
// 1 = reference order (kernels_tau.hip + kernels_planck.hip, bit-faithful expression order).
std::atomic<int> g_arith{0};

// Version switches of the (un-pinned) RTE-RRTMGP solvers, ecckd_set_solver_option.  Process-wide, read once
// per call; the defaults are the v1.5-era forms the oracle restates.
struct SolverOptions {
  std::atomic<double> lw_tau_thresh{0.};        // <= 0: sqrt(epsilon) of the working precision
  std::atomic<int> lw_series_terms{2};
  std::atomic<int> lw_inc_flux_isotropic{0};
  std::atomic<double> sw_k_floor{1.e-12};
  std::atomic<int> sw_dir_clamp{0};
  // implementation choices (same results to ~1e-16 relative): which fp64 / 60-layer longwave solver runs
  std::atomic<int> lw_solver{0};   // 0 register-resident (kernels_rte_lw.hip), 1 layer-split
  std::atomic<int> lw_split_seg{10};
  // ... and whether the call-constant gases of a pass share one slab slot (merge_scalar_gases(); ~1e-16 relative on tau)
  std::atomic<int> gas_merge_scalars{1};
  std::atomic<int> lw_tail_split{1};
  std::atomic<int> sw_tail_split{1};
  std::atomic<int> gas_slab_f32{2};   // fp64 gas optics over the float32 image of the tables in LDS (2: auto)
  // fused gas-optics kernel: 1 = the waves of a block meet at an execution barrier before every tile (same bits), 0 = they
  // run free, -1 (default) = per mode as measured ("Address translation", profiles/gas_tile_sync.json):
  // on in the longwave mode (fp64 and fp32) and in the shortwave mode, off in the tau-only mode
  std::atomic<int> gas_tile_sync{-1};
  // fused gas-optics kernel, longwave mode (the 512-thread instantiations): 1 = a wave loads the per-column inputs of its next
  // tile before the chunk loops of the tile in hand (same bits), 0 = at the top of the tile, -1 (default) = per mode as
  // measured ("Layer-edge sources", profiles/gas_lean.json)
  std::atomic<int> gas_input_ahead{-1};
  // fp64 longwave gas optics: 1 = gas_roles_kernel (tau waves and source waves share a block of 768 threads; same bits)
  // wherever it is instantiated, 0 = never (gas_fused_kernel), -1 (default) = per shape as measured against the parent
  // commit's build ("Wave roles", profiles/gas_wave_roles.json; kernels_gas_roles.hip: gas_roles_default)
  std::atomic<int> gas_wave_roles{-1};
  std::atomic<int> sw_solver{0};   // 0 layer-systolic (kernels_rte_sw_sys.hip; up to 60 layers), 1 per-lane two-pass kernel
  // ecckd_lw_fluxes_clear_allsky at 60 layers: 0 the clear-sky and the all-sky kernel one after the other, 1 the dual-sky
  // kernel (rte_lw_split_both_kernel); same bits.  1: its min-max range lies below that of 0 at every 60-layer shape and
  // configuration measured (profiles/both_skies.json)
  std::atomic<int> lw_both_skies{1};
  std::atomic<int> lw_jac_inline{1};   // (the inline form lies wholly below the stand-alone route at every 60-layer shape)
};
SolverOptions g_opt;
// "gas_input_ahead" = -1: what the measurement chose in fp64 (on: the headline wins) and in fp32 (off: 3 % slower with it);
// the option only reaches the longwave mode ("Layer-edge sources")
constexpr int kGasInputAheadDefault[2] = {1, 0};

// lw_tau_thresh in effect: the option, or sqrt(epsilon(1._wp)) of the working precision
double lw_tau_thresh(bool f32) {
  const double t = g_opt.lw_tau_thresh.load();
  return t > 0. ? t : (f32 ? std::sqrt(1.1920928955078125e-07) : std::sqrt(2.220446049250313e-16));
}

// ---- optional per-kernel timing with HIP events on the launch stream (ecckd_prof_*) ----
struct ProfRec { const char *name; hipEvent_t start, stop; };
std::mutex g_prof_mu;
bool g_prof_on = false;
std::vector<ProfRec> g_prof;

struct ProfScope {
  hipStream_t s;
  ProfRec r{};
  bool on;
  ProfScope(const char *name, hipStream_t stream) : s(stream), on(g_prof_on) {
    if (!on) return;
    r.name = name;
    if (hipEventCreate(&r.start) != hipSuccess || hipEventCreate(&r.stop) != hipSuccess) { on = false; return; }
    (void)hipEventRecord(r.start, s);
  }
  ~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(r.stop, s);
    std::lock_guard<std::mutex> lock(g_prof_mu);
    g_prof.push_back(r);
  }
};

struct GasDesc {   // gas_desc as it crosses the ABI
  int ngas;
  const char *names;
  const double *const *vmr;
  const long long *cs, *ls;
  const double *scalar;
};

size_t vmr_extent(const GasDesc &gd, int j, int ncol, int nlay) {
  if (!gd.vmr || !gd.vmr[j]) return 0;
  const long long cs = gd.cs ? gd.cs[j] : 0, ls = gd.ls ? gd.ls[j] : 0;
  return (size_t)(1 + (long long)(ncol - 1) * cs + (long long)(nlay - 1) * ls);
}

// Planck side of a longwave call, for the fused kernel.
struct PlanckSide {
  const double *tlev, *tsfc;
  double *lay_source, *lev_inc, *lev_dec, *sfc_source;
  long long lev_gstride = 0;   // g-plane stride of lev_inc / lev_dec, elements (level_pair()); 0: separate arrays, nlay*ncol
};

// Planck kernel arguments (fp64) for the sources of `pl`
ecckd::PlanckArgs planck_args(const ecckd_model *m, int ncol, int nlay, const double *tlay, const PlanckSide &pl) {
  ecckd::PlanckArgs p{};
  p.ncol = ncol; p.nlay = nlay; p.ng = m->ng; p.ntp = m->ntp;
  p.planck = m->dbuf + m->off_planck;
  p.t0 = m->temperature_planck[0];                                  // :272
  p.dt = m->temperature_planck[1] - m->temperature_planck[0];      // :271
  p.tlay = tlay; p.tlev = pl.tlev; p.tsfc = pl.tsfc;
  p.lay_source = pl.lay_source; p.lev_source_inc = pl.lev_inc; p.lev_source_dec = pl.lev_dec;
  p.sfc_source = pl.sfc_source;
  p.lev_gstride = pl.lev_gstride;
  return p;
}

// :407-424 on device pointers; the fast arithmetic mode takes the kernel with paired 16-byte stores (same bits)
int planck_sources_dev(const ecckd_model *m, int ncol, int nlay, const double *tlay, const PlanckSide &pl,
                       hipStream_t stream) {
  ecckd::PlanckArgs p = planck_args(m, ncol, nlay, tlay, pl);
  ProfScope prof("planck", stream);
  if (g_arith.load() == 0) HIPCHK(ecckd::launch_planck_pair(p, 0, stream));
  else HIPCHK(ecckd::launch_planck(p, stream));
  return 0;
}

// gas_optical_depth (src/gas_optics_ecckd.f90:323-376) on device pointers.  `sw` selects the
// gas_optics_ext epilogue (:455-460).  When `pl` is given and the fast arithmetic mode is on, the
// Planck sources (:407-424) are produced by the same launch and *planck_done is set.  With `plan`
// given, the decisions are recorded there and nothing is launched.
int gas_optical_depth_dev(const ecckd_model *m, bool f32, PlanRecord *plan, int ncol, int nlay, const double *plev,
                          const double *tlay, const GasDesc &gd, double *tau, bool sw, double *ssa,
                          double *g, const PlanckSide *pl, bool *planck_done, hipStream_t stream) {
  using namespace ecckd;
  if (planck_done) *planck_done = false;
  std::vector<SeqGas> seq;
  bool first_calc = true;   // :347
  for (int j = 0; j < gd.ngas; ++j) {   // :348
    const std::string name = trim_name(gd.names + (size_t)j * ECCKD_NAME_LEN);
    size_t i = 0;
    for (; i < m->gas.size(); ++i)
      if (m->gas[i].name == name) break;   // :349-357
    if (i >= m->gas.size()) continue;      // :358-364 unknown gas: silently skipped
    const ecckd_model::Gas &t = m->gas[i];
    if (t.composite_only && !first_calc) continue;   // :365-367
    SeqGas e{};
    e.coef = table(m, t.dev_off, f32);
    e.vmr = gd.vmr ? gd.vmr[j] : nullptr;
    e.cs = gd.cs ? gd.cs[j] : 0;
    e.ls = gd.ls ? gd.ls[j] : 0;
    e.scalar = gd.scalar ? gd.scalar[j] : 0.;
    if (plan) {   // no data in a plan call: an array gas gets a (never dereferenced) non-null marker, a scalar one 1.0
      const bool sc = plan->is_scalar && plan->is_scalar[j];
      e.vmr = sc ? nullptr : reinterpret_cast<const double *>(sizeof(double));
      e.scalar = 1.;
    }
    e.ref = t.ref;
    e.code = t.code;
    e.nv = t.nv;
    e.clamp = t.has_negative ? 1 : 0;
    if (t.code == ECCKD_LOOK_UP_TABLE) {
      e.mf0 = t.mole_fraction[0];
      e.log_mf0 = std::log(t.mole_fraction[0]);                          // :156
      e.d_log_vmr = std::log(t.mole_fraction[1] / t.mole_fraction[0]);   // :154-155
    }
    seq.push_back(e);
    if (t.composite_only) first_calc = false;   // :371-373
  }

  // Split the sequence into passes holding at most one look_up_table gas and kTauPassGases
  // gases each; later passes start from the tau already stored, so the summation order of :370
  // is preserved exactly in the reference-order mode.
  const bool fast = g_arith.load() == 0;
  size_t pos = 0;
  bool first_pass = true;
  do {
    FusedArgs fa{};
    TauArgs &a = fa.tau;
    a.ncol = ncol; a.nlay = nlay; a.ng = m->ng; a.np = m->np; a.nt = m->nt;
    a.plev = plev; a.tlay = tlay;
    a.temperature = table(m, m->off_temperature, f32);
    a.zero = table(m, m->off_zero, f32);
    a.lp0 = m->log_pressure[0];                               // :104
    a.dlp = m->log_pressure[1] - m->log_pressure[0];          // :105
    a.dt = m->temperature[m->np] - m->temperature[0];         // :106 T(1,2)-T(1,1)
    a.gw = gw(f32);                                           // :107
    a.lut = -1;
    a.merge_slot = -1;
    a.nmerge = 0;
    a.nbil = 0;
    a.nseq = 0;
    while (pos < seq.size()) {
      SeqGas e = seq[pos];
      if (a.nseq >= kTauPassGases) break;
      if (e.code == ECCKD_LOOK_UP_TABLE) {
        if (a.lut >= 0) break;
        a.lut = a.nseq;
      } else {
        e.slot = a.nbil;
        a.bil_seq[a.nbil++] = a.nseq;
      }
      a.seq[a.nseq++] = e;
      ++pos;
    }
    a.accumulate = first_pass ? 0 : 1;
    a.tau = tau;
    const bool last = pos >= seq.size();
    if (sw && last) {
      a.rayleigh = table(m, m->off_rayleigh, f32);
      a.ssa = ssa;
      a.g = g;
    }
    if (fast) {
      fa.mode = (sw && last) ? 2 : 0;
      // (fp64 only: in single precision the two-slot instantiation measured 5 % slower than the seven-slot one it replaces)
      if (g_opt.gas_merge_scalars.load() && !f32) merge_scalar_gases(a, f32);
      const int nv_lut = a.lut >= 0 ? a.seq[a.lut].nv : 0;
      // Planck sources ride along with the first pass when the table, or a window of it, fits next
      // to >= 3 slab rows
      int pass_clamp = 0;
      for (int k = 0; k < a.nseq; ++k) pass_clamp |= a.seq[k].clamp;
      if (pl && first_pass && !sw &&
          fused_planck_rows(a.ng, a.np, a.nt, a.nbil, nv_lut, m->ntp, pass_clamp, f32) > 0) {
        fa.mode = 1;
        fa.ntp = m->ntp;
        fa.planck = table(m, m->off_planck, f32);
        fa.pt0 = m->temperature_planck[0];                                  // :272
        fa.pdt = m->temperature_planck[1] - m->temperature_planck[0];      // :271
        fa.tlev = pl->tlev; fa.tsfc = pl->tsfc;
        fa.lay_source = pl->lay_source; fa.lev_source_inc = pl->lev_inc;
        fa.lev_source_dec = pl->lev_dec; fa.sfc_source = pl->sfc_source;
        fa.lev_gstride = pl->lev_gstride;
        if (planck_done) *planck_done = true;
      }
      fa.f32 = f32;
      {
        const int sync = g_opt.gas_tile_sync.load();
        fa.tile_sync = sync >= 0 ? sync : (fa.mode != 0 ? 1 : 0);
        const int ahead = g_opt.gas_input_ahead.load();
        fa.input_ahead = ahead >= 0 ? ahead : kGasInputAheadDefault[f32 ? 1 : 0];
        fa.wave_roles = (fa.mode == 1 && !f32) ? g_opt.gas_wave_roles.load() : 0;   // (prepare_gas_fused resolves it per shape)
      }
      // fp64 over the float32 image of the tables in LDS ("gas_slab_f32": 0 never, 1 always, 2 where the probe finds the
      // columns spread over many pressure rows); the probe's counter is a word that belongs to this stream
      ScratchLease flag_lease;
      fa.slab32 = (!f32 && !plan && m->f32_exact && fa.mode == 1) ? g_opt.gas_slab_f32.load() : 0;
      if (fa.slab32 == 2) fa.choose_buf = static_cast<int *>(stream_scratch_optional(m->device, stream, 256, flag_lease, g_flag_pool));
      if (f32 && ((fa.mode != 1 && fa.mode != 2) || !last || !first_pass))
        return fail("ecckd: single precision is implemented for one-pass gas optics (fused longwave, shortwave); this "
                    "model / gas list needs the multi-pass or unfused path");
      if (plan) {
        FusedPlan fp;
        HIPCHK(prepare_gas_fused(fa, fp));
        if (plan->npass == 0) { plan->first_fused = 1; plan->planck_fused = fa.mode == 1; plan->first = fp; }
        ++plan->npass;
      } else {
        ProfScope prof(fa.mode == 1 ? (f32 ? "gas_lw_fused_f32" : "gas_lw_fused") : "tau", stream);
        HIPCHK(launch_gas_fused(fa, stream));
      }
    } else {
      if (f32) return fail("ecckd: single precision needs the fast arithmetic mode (ecckd_set_arithmetic(0))");
      if (plan) {
        ++plan->npass;
      } else {
        ProfScope prof("tau", stream);
        HIPCHK(launch_tau(a, stream));
      }
    }
    first_pass = false;
  } while (pos < seq.size());
  return 0;
}

int check_model(const ecckd_model *m) {
  if (!m) return fail("ecckd: null model");
  if (!m->finalized) return fail("ecckd: model is not finalized");
  if (m->device < 0) return fail("ecckd: host-only model (device -1): no GPU, no compute (there is no CPU fallback)");
  return 0;
}

int check_dims(int ncol, int nlay) {
  if (ncol < 0 || nlay < 1) return fail("ecckd: bad ncol/nlay");
  return 0;
}
int check_gas_optics_dims(int ncol, int nlay) {
  if (check_dims(ncol, nlay)) return 1;
  // the gas-optics kernels address one g-plane pair of a column-fastest array with 32-bit byte offsets
  if (((size_t)ncol * (size_t)nlay + (size_t)ncol) * sizeof(double) >= (size_t)0xFFFFFFF0u)
    return fail("ecckd: ncol*(nlay+1) too large for one call (limit 2^29 elements): split the column range");
  return 0;
}
// ... and with one level buffer the level planes are (nlay+1)*ncol apart
int check_level_buffer_dims(int ncol, int nlay) {
  if (((size_t)ncol * (size_t)(nlay + 1) + (size_t)ncol) * sizeof(double) >= (size_t)0xFFFFFFF0u)
    return fail("ecckd: ncol*(nlay+2) too large for one call on a level buffer (limit 2^29 elements): split the column range");
  return 0;
}

// Level buffer (include/ecckd_hip.h, "Level buffer"): lev_source_inc == lev_source_dec + ncol, in elements of the call's
// precision, names the two views of ONE array lev(ncol, nlay+1, ngpt) -- dec(:,l,:) = lev(:,l,:), inc(:,l,:) = lev(:,l+1,:),
// both with a g-plane stride of (nlay+1)*ncol.  Two contiguous (ncol,nlay,ngpt) arrays at those addresses would overlap, so
// nothing else can be meant.  Every entry point that takes the pair asks here: the g-plane stride of the two arrays, and
// whether the levels are physically shared.  `accepts`: the entry point's kernels take the stride; the others, host arrays
// (Stage copies nlay*ncol*ngpt contiguous elements per array) and single precision refuse the aliased pair.
struct LevelPair {
  long long gstride = 0;   // elements
  bool shared = false;     // one level buffer: a writer stores each level once, a reader may read it once
};
int level_pair(const char *who, const void *inc, const void *dec, int ncol, int nlay, bool f32, int memspace, bool accepts,
               LevelPair *out) {
  out->gstride = (long long)ncol * nlay;
  out->shared = false;
  if (!inc || !dec || ncol <= 0) return 0;
  if (static_cast<const char *>(inc) != static_cast<const char *>(dec) + (size_t)ncol * esz(f32)) return 0;
  const std::string lead = std::string(who) + ": lev_source_inc == lev_source_dec + ncol names one level buffer (ncol,nlay+1,ngpt)";
  if (memspace == ECCKD_HOST) return fail(lead + "; host arrays (ECCKD_HOST) are not taken in that form: pass two separate arrays");
  if (f32) return fail(lead + "; single precision does not take that form: pass two separate arrays");
  if (!accepts) return fail(lead + "; this entry point does not take that form: pass two separate arrays");
  out->gstride = (long long)ncol * (nlay + 1);
  out->shared = true;
  return 0;
}
// the entry points whose kernels read two separate arrays
int refuse_level_buffer(const char *who, const void *inc, const void *dec, int ncol, int nlay, int memspace) {
  LevelPair lp;
  return level_pair(who, inc, dec, ncol, nlay, false, memspace, false, &lp);
}

// Element counts of the arrays of a call: (ncol), (ncol,nlay), (ncol,nlay+1), and per g-point or band of each
struct Counts {
  size_t col, lay, lev, lay_g, col_g, lay_b, col_b;
  Counts(int ncol, int nlay, int ng, int nband)
      : col((size_t)ncol), lay(col * nlay), lev(col * (nlay + 1)), lay_g(lay * ng), col_g(col * ng), lay_b(lay * nband),
        col_b(col * nband) {}
};

// ---- staging: a call's arrays are declared once, wherever they live ----
// An entry point hands open() a function that declares every array of the call -- in / out / inout with its element
// count, kBig for the spectral arrays that ECCKD_MIXED leaves on the device -- and takes the pointers its kernels get.
// An array that lives on the device comes back as the caller's pointer, untouched.  A host array gets a 256-byte-aligned
// room of the arena and is copied in; close() copies the outputs back and synchronises once.  A null (optional) pointer
// stays null and takes no room.  With anything to stage, open() takes the arena's lock and runs the declarations twice:
// first to add the rooms up, then -- the arena grown to that size, which frees the old block, so before any copy -- to
// carve them and issue the copies: the statements that carve the arena are the ones that size it.  With ECCKD_DEVICE
// open() runs them once and close() does nothing: no lock, no allocation, no heap, no synchronisation, capturable.
// The declarations must do nothing but declare (they run twice); pointers derived from a room are formed after open().
constexpr bool kBig = true;

class Stage {
 public:
  const hipStream_t stream;   // where the call launches: the caller's stream (ECCKD_DEVICE), else the arena's

  // a solver call: the arena of the device and the null stream
  Stage(int device, int memspace, void *caller_stream, bool f32)
      : Stage(device, memspace, caller_stream, f32, g_solver_arena[device].mu, g_solver_arena[device].p,
              g_solver_arena[device].bytes, nullptr) {}
  // a call on a model: the model's arena and its host stream
  Stage(ecckd_model *m, int memspace, void *caller_stream, bool f32)
      : Stage(m->device, memspace, caller_stream, f32, m->mu, m->arena, m->arena_bytes, m->host_stream) {}

  const double *in(const double *p, size_t n, bool big = false) { return static_cast<double *>(place(p, n * es, big, true, false)); }
  // back = false: a room the kernels write and nobody reads back
  double *out(double *p, size_t n, bool big = false, bool back = true) { return static_cast<double *>(place(p, n * es, big, false, back)); }
  double *inout(double *p, size_t n, bool back = true) { return static_cast<double *>(place(p, n * es, false, true, back)); }
  // cloud masks: 8-byte words whatever the precision of the call
  const unsigned long long *in(const unsigned long long *p, size_t n) { return static_cast<unsigned long long *>(place(p, n * 8, false, true, false)); }
  unsigned long long *out(unsigned long long *p, size_t n) { return static_cast<unsigned long long *>(place(p, n * 8, false, false, true)); }
  // aerosol type codes: 4-byte integers whatever the precision of the call
  const int *in(const int *p, size_t n) { return static_cast<int *>(place(p, n * 4, false, true, false)); }
  // column lists (ecckd_daylit_columns) and arrays given by their size in bytes (ecckd_gather_columns / _scatter_columns)
  int *out(int *p, size_t n) { return static_cast<int *>(place(p, n * 4, false, false, true)); }
  const void *in_bytes(const void *p, size_t bytes) { return place(p, bytes, false, true, false); }
  void *out_bytes(void *p, size_t bytes) { return place(p, bytes, false, false, true); }
  // a spectral array the call reads and writes (ECCKD_MIXED leaves it on the device)
  double *inout_big(double *p, size_t n) { return static_cast<double *>(place(p, n * es, kBig, true, true)); }

  // The gas description with its concentration arrays staged (the strides and scalars stay as they are)
  GasDesc gases(const GasDesc &gd, int ncol, int nlay) {
    if (!host_any) return gd;
    vmr.assign(gd.ngas, nullptr);
    for (int j = 0; j < gd.ngas; ++j) vmr[j] = in(gd.vmr ? gd.vmr[j] : nullptr, vmr_extent(gd, j, ncol, nlay));
    GasDesc d = gd;
    d.vmr = vmr.data();
    return d;
  }

  // The work block of the call (optical depth between the kernels, sources, rings, scaled planes; the entry point lays it
  // out, the same way on every route): the scratch block of the caller's stream under the rules of ScratchPool -- the
  // lease lasts as long as the Stage, past the launches -- or, with host arrays, a room of the arena.  One per call.
  double *work(size_t bytes) {
    if (host_any) return static_cast<double *>(room(bytes));
    void *p = nullptr;
    if (stream_scratch(device, stream, bytes, &p, lease)) err = 1;
    return static_cast<double *>(p);
  }
  // ... with `extra` bytes behind it for a use the call can do without (a tail split): *got_extra tells whether they are
  // there -- always with host arrays; with the stream's block under the rules of stream_scratch_optional
  double *work(size_t bytes, size_t extra, bool *got_extra) {
    *got_extra = extra > 0;
    if (host_any) return static_cast<double *>(room(bytes + extra));
    if (extra)
      if (void *p = stream_scratch_optional(device, stream, bytes + extra, lease)) return static_cast<double *>(p);
    *got_extra = false;
    return work(bytes);
  }

  template <class F> int open(F &&declare) {
    if (!host_any) { declare(); return err; }
    lock = std::unique_lock<std::mutex>(mu);
    measuring = true;
    declare();
    if (err || grow(off)) return 1;
    measuring = false;
    off = 0;
    declare();
    return err;
  }

  int close() {
    if (!host_any) return 0;
    for (int i = 0; i < nback; ++i)
      HIPCHK(hipMemcpyAsync(backs[i].host, backs[i].dev, backs[i].bytes, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
  }

 private:
  Stage(int device_, int memspace, void *caller_stream, bool f32, std::mutex &mu_, void *&arena_, size_t &arena_bytes_,
        hipStream_t arena_stream)
      : stream(memspace == ECCKD_DEVICE ? static_cast<hipStream_t>(caller_stream) : arena_stream), device(device_),
        host_any(memspace != ECCKD_DEVICE), host_big(host_any && memspace != ECCKD_MIXED), es(esz(f32)), mu(mu_),
        arena(arena_), arena_bytes(arena_bytes_) {}

  // (the lock is held) the model's host stream may still read the old block; the solver arena's null stream needs no such care
  int grow(size_t need) {
    if (need <= arena_bytes) return 0;
    if (stream) HIPCHK(hipStreamSynchronize(stream));
    if (arena) { HIPCHK(hipFree(arena)); arena = nullptr; arena_bytes = 0; }
    HIPCHK(hipMalloc(&arena, need));
    arena_bytes = need;
    return 0;
  }

  void *room(size_t bytes) {
    const size_t at = off;
    off += align256(bytes);
    return measuring || !bytes ? nullptr : static_cast<char *>(arena) + at;
  }

  void *place(const void *p, size_t bytes, bool big, bool copy_in, bool copy_back) {
    void *const caller = const_cast<void *>(p);
    if (!p || !bytes || !(big ? host_big : host_any)) return caller;
    void *d = room(bytes);
    if (measuring || err) return caller;
    if (copy_in) {
      const hipError_t e = hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, stream);
      if (e != hipSuccess) err = fail(std::string("hipMemcpyAsync (host to device): ") + hipGetErrorString(e));
    }
    if (copy_back) {
      if (nback == kMaxBack) err = fail("ecckd: internal: too many outputs in one staged call");
      else backs[nback++] = Back{caller, d, bytes};
    }
    return d;
  }

  static constexpr int kMaxBack = 8;
  struct Back { void *host; const void *dev; size_t bytes; };
  const int device;
  const bool host_any, host_big;   // host arrays at all / the kBig arrays too
  const size_t es;                 // element size of the call: esz()
  std::mutex &mu;
  void *&arena;
  size_t &arena_bytes;
  std::unique_lock<std::mutex> lock;
  ScratchLease lease;
  std::vector<const double *> vmr;   // (host arrays only)
  Back backs[kMaxBack];
  int nback = 0, err = 0;
  size_t off = 0;
  bool measuring = false;
};

// out(:) = sum over planes of planes(:, b) on the host, in the precision of T
template <class T> void sum_planes_host(const T *planes, int nplanes, size_t n, T *out) {
  for (size_t i = 0; i < n; ++i) {
    T acc = 0;
    for (int b = 0; b < nplanes; ++b) acc += planes[(size_t)b * n + i];
    out[i] = acc;
  }
}

// out(:) = sum over planes of planes(:, b), on the device or on the host
int sum_planes(const double *planes, int nplanes, size_t n, double *out, bool f32, int memspace, void *stream) {
  if (memspace == ECCKD_DEVICE) {
    HIPCHK(ecckd::launch_sum_planes(planes, nplanes, n, out, f32, static_cast<hipStream_t>(stream)));
    return 0;
  }
  if (f32)   // (the single-precision flavours: float data behind the double pointers)
    sum_planes_host(reinterpret_cast<const float *>(planes), nplanes, n, reinterpret_cast<float *>(out));
  else
    sum_planes_host(planes, nplanes, n, out);
  return 0;
}
// p + n elements of the precision of the call (float data sits behind the double pointers of the _f32 flavours)
template <class T> T *el(T *p, size_t n, bool f32) { return reinterpret_cast<T *>(reinterpret_cast<uintptr_t>(p) + n * esz(f32)); }

int fill_band_map(int ngpt, int nband, const int *band2gpt, unsigned char *gpt2band) {
  if (ngpt < 1 || ngpt > 256) return fail("ecckd: ngpt must be in 1..256");
  if (nband < 1 || nband > 255 || !band2gpt) return fail("ecckd: bad band description");
  std::memset(gpt2band, 0, 256);
  std::vector<int> seen(ngpt, 0);
  for (int b = 0; b < nband; ++b) {
    const int lo = band2gpt[2 * b], hi = band2gpt[2 * b + 1];
    if (lo < 1 || hi > ngpt || lo > hi) return fail("ecckd: band2gpt out of range");
    for (int gpt = lo; gpt <= hi; ++gpt) { gpt2band[gpt - 1] = (unsigned char)b; seen[gpt - 1] = 1; }
  }
  for (int i = 0; i < ngpt; ++i)
    if (!seen[i]) return fail("ecckd: band2gpt does not cover every g-point");
  return 0;
}

}  // namespace

// ---- cloud optics: the object and its host-side helpers (the entry points are below, with kernels_cloud_optics.hip) ----
// The look-up tables of ty_cloud_optics.  On the device: one buffer of (value, slope) pair images, per precision the liquid
// image [quantity][band][nsize_liq-1] and, per roughness, the ice image [quantity][band][nsize_ice-1].
struct ecckd_cloud_lut {
  int nband = 0, nsize_liq = 0, nsize_ice = 0, nrghice = 0, device = -1;
  double radliq_lwr = 0., radliq_upr = 0., radice_lwr = 0., radice_upr = 0.;
  char *dbuf = nullptr;
  size_t off_liq[2] = {0, 0}, off_ice[2] = {0, 0}, ice_stride[2] = {0, 0};   // bytes; [0] fp64, [1] float
};

// ---- sampled optical-depth scaling: the table of in-cloud water variability (ecckd_cloud_scaling_create) ----
// values(nfsd,nq), q fastest, on the host and -- with a device -- on the device
struct ecckd_cloud_scaling {
  int nfsd = 0, nq = 0, device = -1;
  double fsd0 = 0., dfsd = 0.;
  std::vector<double> values;
  double *dvalues = nullptr;
};

namespace {

// (value, slope) pairs of the rows of `table` (nsize, nrow), size fastest, appended to `out`: the table is rounded to
// `real` first and the slope is the subtraction table[i+1] - table[i] in `real`
template <typename real>
void append_pairs(std::vector<ecckd::CloudLutPair<real>> &out, const double *table, int nsize, size_t nrow) {
  for (size_t r = 0; r < nrow; ++r)
    for (int i = 0; i + 1 < nsize; ++i) {
      const real lo = (real)table[r * nsize + i], hi = (real)table[r * nsize + i + 1];
      out.push_back(ecckd::CloudLutPair<real>{lo, hi - lo});
    }
}

template <typename real>
std::vector<ecckd::CloudLutPair<real>> cloud_lut_image(int nsize, int nband, int nrgh, const double *ext, const double *ssa,
                                                       const double *asy) {
  std::vector<ecckd::CloudLutPair<real>> out;
  out.reserve((size_t)3 * nrgh * nband * (nsize - 1));
  const size_t plane = (size_t)nsize * nband;
  for (int r = 0; r < nrgh; ++r) {
    append_pairs(out, ext + r * plane, nsize, nband);
    append_pairs(out, ssa + r * plane, nsize, nband);
    append_pairs(out, asy + r * plane, nsize, nband);
  }
  return out;
}

// RTE's check_values on host arrays: the first complaint, or null.  Bounds in the precision of the call.
template <typename real>
const char *cloud_optics_check_host(const ecckd_cloud_lut &co, size_t n, const real *clwp, const real *ciwp, const real *reliq,
                                    const real *reice) {
  const real ll = (real)co.radliq_lwr, lu = (real)co.radliq_upr, il = (real)co.radice_lwr, iu = (real)co.radice_upr;
  for (size_t i = 0; i < n; ++i)
    if (clwp[i] > real(0) && !(reliq[i] >= ll && reliq[i] <= lu))
      return "ecckd_cloud_optics: liquid effective radius out of the table's range in a cloudy cell";
  for (size_t i = 0; i < n; ++i)
    if (ciwp[i] > real(0) && !(reice[i] >= il && reice[i] <= iu))
      return "ecckd_cloud_optics: ice effective radius out of the table's range in a cloudy cell";
  for (size_t i = 0; i < n; ++i)
    if (clwp[i] < real(0)) return "ecckd_cloud_optics: negative liquid water path";
  for (size_t i = 0; i < n; ++i)
    if (ciwp[i] < real(0)) return "ecckd_cloud_optics: negative ice water path";
  return nullptr;
}

}  // namespace

// ---- aerosol optics: the object and its host-side helpers (the entry points are below, with kernels_aerosol_optics.hip) ----
// The tables of the MERRA-style aerosol optics.  On the device: one buffer holding, per precision, the head (rh_levels,
// their differences, bin_lims) and the image of (value, slope) pairs laid out as kernels.hpp describes.
struct ecckd_aerosol_lut {
  int nband = 0, nbin = 0, nrh = 0, device = -1;
  std::vector<double> bin_lims, rh_levels;   // host copies: the value checks of host arrays
  char *dbuf = nullptr;
  size_t off_head[2] = {0, 0}, off_image[2] = {0, 0};   // bytes; [0] fp64, [1] float
};

namespace {

struct AerosolTables {
  const double *dust, *salt, *sulf, *bcar, *bcar_rh, *ocar, *ocar_rh;
};

// rh_levels, d(i) = levels(i+1) - levels(i), bin_lims, rounded to `real` first
template <typename real>
std::vector<real> aerosol_head(int nbin, int nrh, const double *bin_lims, const double *rh_levels) {
  std::vector<real> out;
  out.reserve((size_t)2 * nrh - 1 + 2 * nbin);
  for (int i = 0; i < nrh; ++i) out.push_back((real)rh_levels[i]);
  for (int i = 0; i + 1 < nrh; ++i) out.push_back((real)rh_levels[i + 1] - (real)rh_levels[i]);
  for (int i = 0; i < 2 * nbin; ++i) out.push_back((real)bin_lims[i]);
  return out;
}

// the image [quantity][band][entry] (kernels.hpp): tables rounded to `real` first, slope = table(i+1) - table(i) in `real`
template <typename real>
std::vector<ecckd::CloudLutPair<real>> aerosol_image(int nband, int nbin, int nrh, const AerosolTables &t) {
  typedef ecckd::CloudLutPair<real> Pair;
  std::vector<Pair> out;
  out.reserve((size_t)3 * nband * ecckd::kAoEntries(nbin, nrh));
  auto rh_row = [&](const double *tbl, size_t at) {   // tbl(q, 1..nrh) at `at`, stride 3
    for (int i = 0; i + 1 < nrh; ++i) {
      const real lo = (real)tbl[at + (size_t)3 * i], hi = (real)tbl[at + (size_t)3 * (i + 1)];
      out.push_back(Pair{lo, hi - lo});
    }
  };
  for (int q = 0; q < 3; ++q)
    for (int b = 0; b < nband; ++b) {
      for (int n = 0; n < nbin; ++n) out.push_back(Pair{(real)t.dust[q + 3 * ((size_t)n + (size_t)nbin * b)], real(0)});
      for (int n = 0; n < nbin; ++n) rh_row(t.salt, q + (size_t)3 * nrh * ((size_t)n + (size_t)nbin * b));
      rh_row(t.sulf, q + (size_t)3 * nrh * b);
      rh_row(t.bcar_rh, q + (size_t)3 * nrh * b);
      rh_row(t.ocar_rh, q + (size_t)3 * nrh * b);
      out.push_back(Pair{(real)t.bcar[q + (size_t)3 * b], real(0)});
      out.push_back(Pair{(real)t.ocar[q + (size_t)3 * b], real(0)});
    }
  return out;
}

// the value checks of host arrays: the first complaint, or null.  Limits in the precision of the call.
template <typename real>
const char *aerosol_optics_check_host(const ecckd_aerosol_lut &ao, size_t n2, int nspec, const int *type, const real *size,
                                      const real *mass, const real *relhum) {
  const size_t n3 = n2 * nspec;
  auto active = [&](size_t i) { return type[i] >= 1 && type[i] <= 7 && mass[i] > real(0); };
  auto in_a_bin = [&](real r) {
    for (int b = 0; b < ao.nbin; ++b)
      if ((real)ao.bin_lims[2 * b] <= r && r < (real)ao.bin_lims[2 * b + 1]) return true;
    return false;
  };
  for (size_t i = 0; i < n3; ++i)
    if (type[i] < 0 || type[i] > 7) return "ecckd_aerosol_optics: aerosol type outside 0..7";
  for (size_t i = 0; i < n3; ++i)
    if (mass[i] < real(0)) return "ecckd_aerosol_optics: negative aerosol mass";
  for (size_t i = 0; i < n3; ++i)
    if (active(i) && type[i] <= 2 && !in_a_bin(size[i]))
      return "ecckd_aerosol_optics: the size of an active dust or sea-salt cell lies in no bin";
  for (size_t i = 0; i < n3; ++i) {
    const int k = type[i];
    if (active(i) && (k == 2 || k == 3 || k == 4 || k == 6)) {
      const real rh = relhum[i % n2];
      if (!(rh >= real(0) && rh <= real(1)))
        return "ecckd_aerosol_optics: relative humidity outside [0,1] in a cell with an active humidity-dependent species";
    }
  }
  return nullptr;
}

}  // namespace

extern "C" {

const char *ecckd_last_error(void) { return g_err.c_str(); }

const char *ecckd_build_info(void) {
  return "rte-ecckd hot path for MI355X: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off, fp64";
}

// ------------------------------- device memory for hosts without a HIP binding ---------------------

int ecckd_device_malloc(int device, size_t bytes, void **ptr) {
  if (!ptr) return fail("ecckd_device_malloc: null output");
  *ptr = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail("ecckd: no HIP device available (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail("ecckd_device_malloc: bad device ordinal");
  HIPCHK(hipSetDevice(device));
  if (bytes == 0) return 0;
  HIPCHK(hipMalloc(ptr, bytes));
  return 0;
}

int ecckd_device_free(int device, void *ptr) {
  if (!ptr) return 0;
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipFree(ptr));
  return 0;
}

int ecckd_device_memcpy(int device, void *dst, const void *src, size_t bytes, int to_device) {
  if (bytes == 0) return 0;
  if (!dst || !src) return fail("ecckd_device_memcpy: null pointer");
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipMemcpy(dst, src, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost));
  return 0;
}

// ------------------------------- kernel timing hooks -------------------------------------

int ecckd_set_arithmetic(int mode) {
  if (mode != 0 && mode != 1) return fail("ecckd_set_arithmetic: mode must be 0 (fast) or 1 (reference order)");
  g_arith.store(mode);
  return 0;
}

int ecckd_get_arithmetic(void) { return g_arith.load(); }

int ecckd_set_solver_option(const char *name, double value) {
  if (!name) return fail("ecckd_set_solver_option: null name");
  const std::string n(name);
  if (!(value - value == 0.)) return fail("ecckd_set_solver_option: value must be finite");
  if (n == "lw_tau_thresh") g_opt.lw_tau_thresh.store(value);                       // <= 0 restores the default
  else if (n == "lw_series_terms") {
    if (value != 2. && value != 3.) return fail("ecckd_set_solver_option: lw_series_terms must be 2 or 3");
    g_opt.lw_series_terms.store((int)value);
  } else if (n == "lw_inc_flux_isotropic") g_opt.lw_inc_flux_isotropic.store(value != 0. ? 1 : 0);
  else if (n == "sw_k_floor") {
    if (!(value > 0.)) return fail("ecckd_set_solver_option: sw_k_floor must be > 0");
    g_opt.sw_k_floor.store(value);
  } else if (n == "sw_dir_clamp") g_opt.sw_dir_clamp.store(value != 0. ? 1 : 0);
  else if (n == "lw_solver") {
    if (value != 0. && value != 1.) return fail("ecckd_set_solver_option: lw_solver must be 0 (register-resident) or 1 (layer-split)");
    g_opt.lw_solver.store((int)value);
  } else if (n == "lw_split_seg") {
    if (value != 10. && value != 12. && value != 15.) return fail("ecckd_set_solver_option: lw_split_seg must be 10, 12 or 15");
    g_opt.lw_split_seg.store((int)value);
  } else if (n == "gas_merge_scalars") g_opt.gas_merge_scalars.store(value != 0. ? 1 : 0);
  else if (n == "lw_tail_split") g_opt.lw_tail_split.store(value != 0. ? 1 : 0);
  else if (n == "sw_tail_split") g_opt.sw_tail_split.store(value != 0. ? 1 : 0);
  else if (n == "sw_solver") {
    if (value != 0. && value != 1.) return fail("ecckd_set_solver_option: sw_solver must be 0 (layer-systolic) or 1 (two-pass per lane)");
    g_opt.sw_solver.store((int)value);
  }
  else if (n == "lw_both_skies") {
    if (value != 0. && value != 1.) return fail("ecckd_set_solver_option: lw_both_skies must be 0 (two launches) or 1 (dual-sky kernel)");
    g_opt.lw_both_skies.store((int)value);
  }
  else if (n == "lw_jac_inline") {
    if (value != 0. && value != 1.) return fail("ecckd_set_solver_option: lw_jac_inline must be 0 (stand-alone Jacobian kernel) or 1 (inside the layer-split kernel)");
    g_opt.lw_jac_inline.store((int)value);
  }
  else if (n == "gas_slab_f32") {
    if (value != 0. && value != 1. && value != 2.) return fail("ecckd_set_solver_option: gas_slab_f32 must be 0 (never), 1 (always) or 2 (auto)");
    g_opt.gas_slab_f32.store((int)value);
  }
  else if (n == "gas_tile_sync") {
    if (value != 0. && value != 1. && value != -1.)
      return fail("ecckd_set_solver_option: gas_tile_sync must be 0 (off), 1 (a block barrier per tile) or -1 (the default of each mode)");
    g_opt.gas_tile_sync.store((int)value);
  }
  else if (n == "gas_input_ahead") {
    if (value != 0. && value != 1. && value != -1.)
      return fail("ecckd_set_solver_option: gas_input_ahead must be 0 (inputs loaded at the top of a tile), 1 (a tile ahead) or -1 (the default of each mode)");
    g_opt.gas_input_ahead.store((int)value);
  }
  else if (n == "gas_wave_roles") {
    if (value != 0. && value != 1. && value != -1.)
      return fail("ecckd_set_solver_option: gas_wave_roles must be 0 (never), 1 (wherever the wave-roles kernel exists) or -1 (the default of each shape)");
    g_opt.gas_wave_roles.store((int)value);
  }
  else return fail("ecckd_set_solver_option: unknown option '" + n + "' (lw_tau_thresh, lw_series_terms, "
                   "lw_inc_flux_isotropic, sw_k_floor, sw_dir_clamp, lw_solver, lw_split_seg, gas_merge_scalars, lw_tail_split, "
                   "sw_tail_split, sw_solver, gas_slab_f32, gas_tile_sync, gas_input_ahead, gas_wave_roles, lw_both_skies, lw_jac_inline)");
  return 0;
}

int ecckd_get_solver_option(const char *name, double *value) {
  if (!name || !value) return fail("ecckd_get_solver_option: null argument");
  const std::string n(name);
  if (n == "lw_tau_thresh") *value = lw_tau_thresh(false);
  else if (n == "lw_series_terms") *value = g_opt.lw_series_terms.load();
  else if (n == "lw_inc_flux_isotropic") *value = g_opt.lw_inc_flux_isotropic.load();
  else if (n == "sw_k_floor") *value = g_opt.sw_k_floor.load();
  else if (n == "sw_dir_clamp") *value = g_opt.sw_dir_clamp.load();
  else if (n == "lw_solver") *value = g_opt.lw_solver.load();
  else if (n == "lw_split_seg") *value = g_opt.lw_split_seg.load();
  else if (n == "gas_merge_scalars") *value = g_opt.gas_merge_scalars.load();
  else if (n == "lw_tail_split") *value = g_opt.lw_tail_split.load();
  else if (n == "sw_tail_split") *value = g_opt.sw_tail_split.load();
  else if (n == "sw_solver") *value = g_opt.sw_solver.load();
  else if (n == "gas_slab_f32") *value = g_opt.gas_slab_f32.load();
  else if (n == "gas_tile_sync") *value = g_opt.gas_tile_sync.load();
  else if (n == "gas_input_ahead") *value = g_opt.gas_input_ahead.load();
  else if (n == "gas_wave_roles") *value = g_opt.gas_wave_roles.load();
  else if (n == "lw_both_skies") *value = g_opt.lw_both_skies.load();
  else if (n == "lw_jac_inline") *value = g_opt.lw_jac_inline.load();
  else return fail("ecckd_get_solver_option: unknown option '" + n + "'");
  return 0;
}

size_t ecckd_rte_lw_scratch_bytes(int ncol, int nlay, int ngpt) {
  return ncol > 0 && nlay > 0 ? ecckd::rte_lw_scratch_bytes(ncol, nlay, ngpt) : 0;
}
size_t ecckd_rte_sw_scratch_bytes(int ncol, int nlay, int ngpt) {
  return ncol > 0 && nlay > 0 ? ecckd::rte_sw_scratch_bytes(ncol, nlay, ngpt) : 0;
}

size_t ecckd_rte_sw_tail_scratch_bytes(int device, int ncol, int nlay, int ngpt) {
  if (ncol <= 0 || nlay <= 0 || ngpt <= 0 || device < 0 || device >= 16 || !g_opt.sw_tail_split.load()) return 0;
  ecckd::RteSwArgs a{};
  a.ncol = ncol; a.nlay = nlay; a.ng = ngpt;
  if (g_opt.sw_solver.load() == 0 && ecckd::rte_sw_sys_applies(a)) return ecckd::rte_sw_sys_plan(a, simd_slots(device) / 4);
  long first = -1;
  size_t at = 0;
  return ecckd::rte_sw_tail_plan(a, &first, &at);
}
// What ecckd_sw_fluxes needs behind the optical depth in its scratch block for the solver it will take (the sizing
// rule of include/ecckd_hip.h): the layer-systolic solver's partial sums, or the two-pass solver's ring and partial sums.
// two_pass (ecckd_sw_flux_scaled): the two-pass solver whatever "sw_solver" says.
static size_t sw_fluxes_solver_bytes(int device, int ncol, int nlay, int ngpt, bool two_pass = false) {
  ecckd::RteSwArgs a{};
  a.ncol = ncol; a.nlay = nlay; a.ng = ngpt;
  if (two_pass) {
    long first = -1;
    size_t at = 0;
    const size_t tail2 = g_opt.sw_tail_split.load() && device >= 0 && device < 16 ? ecckd::rte_sw_tail_plan(a, &first, &at) : 0;
    const size_t ring2 = ecckd_rte_sw_scratch_bytes(ncol, nlay, ngpt);
    return tail2 > ring2 ? tail2 : ring2;
  }
  const size_t tail = ecckd_rte_sw_tail_scratch_bytes(device, ncol, nlay, ngpt);
  if (g_opt.sw_solver.load() == 0 && ecckd::rte_sw_sys_applies(a)) return tail;
  const size_t ring = ecckd_rte_sw_scratch_bytes(ncol, nlay, ngpt);
  return tail > ring ? tail : ring;
}
size_t ecckd_rte_lw_tail_scratch_bytes(int device, int ncol, int nlay, int ngpt, int n_gauss_angles, int single_precision) {
  if (ncol <= 0 || nlay <= 0 || ngpt <= 0 || device < 0 || device >= 16 || !g_opt.lw_tail_split.load()) return 0;
  if (n_gauss_angles < 1 || n_gauss_angles > 4) return 0;
  ecckd::RteLwArgs a{};
  a.ncol = ncol; a.nlay = nlay; a.ng = ngpt; a.nmus = n_gauss_angles; a.f32 = single_precision ? 1 : 0;
  a.use_split = g_opt.lw_solver.load();
  long first = -1;
  return ecckd::rte_lw_tail_plan(a, simd_slots(device), &first);
}

int ecckd_set_stream_scratch(int device, void *stream, void *buffer, size_t bytes) {
  if (device < 0 || device >= 16) return fail("ecckd_set_stream_scratch: bad device ordinal");
  if ((buffer == nullptr) != (bytes == 0)) return fail("ecckd_set_stream_scratch: buffer and size must both be given, or neither");
  ScratchPool &pool = g_scratch_pool[device];
  std::lock_guard<std::mutex> lock(pool.mu);
  ScratchPool::Block &b = pool.live[static_cast<hipStream_t>(stream)];
  if (b.p && !b.caller_owned) pool.retired.push_back(b.p);
  b.p = buffer; b.bytes = bytes; b.caller_owned = buffer != nullptr; b.captured = false;
  return 0;
}

static int release_pool(ScratchPool &pool, int device);
int ecckd_release_scratch(int device) {
  if (device < 0 || device >= 16) return fail("ecckd_release_scratch: bad device ordinal");
  if (release_pool(g_flag_pool[device], device)) return 1;
  return release_pool(g_scratch_pool[device], device);
}
static int release_pool(ScratchPool &pool, int device) {
  std::lock_guard<std::mutex> lock(pool.mu);
  if (pool.live.empty() && pool.retired.empty()) return 0;
  HIPCHK(hipSetDevice(device));
  if (pool.leases > 0) return fail("ecckd_release_scratch: another thread is inside a solver call on this device");
  HIPCHK(hipDeviceSynchronize());   // nothing in flight may still use a block
  // (graphs captured with library-owned scratch hold these addresses: destroy them before releasing -- see the header)
  for (auto it = pool.live.begin(); it != pool.live.end();) {
    if (it->second.caller_owned) { ++it; continue; }   // the caller's buffer stays registered
    if (it->second.p) (void)hipFree(it->second.p);
    it = pool.live.erase(it);
  }
  for (void *p : pool.retired) (void)hipFree(p);
  pool.retired.clear();
  return 0;
}

// Every launch sits in a ProfScope on the stream it goes to, whatever the memory space of the call: with host arrays the
// stand-alone solvers and element-wise calls are recorded too (on the arena's stream), as the fused calls always were.
int ecckd_prof_enable(int on) {
  std::lock_guard<std::mutex> lock(g_prof_mu);
  g_prof_on = on != 0;
  return 0;
}

int ecckd_prof_report(int max_kernels, char *names, double *total_ms, long long *launches) {
  std::lock_guard<std::mutex> lock(g_prof_mu);
  int n = 0;
  for (ProfRec &r : g_prof) {
    float ms = 0.f;
    if (hipEventSynchronize(r.stop) == hipSuccess) (void)hipEventElapsedTime(&ms, r.start, r.stop);
    (void)hipEventDestroy(r.start);
    (void)hipEventDestroy(r.stop);
    int k = 0;
    for (; k < n; ++k)
      if (std::strncmp(names + (size_t)k * ECCKD_NAME_LEN, r.name, ECCKD_NAME_LEN) == 0) break;
    if (k == n) {
      if (n >= max_kernels) continue;
      std::memset(names + (size_t)n * ECCKD_NAME_LEN, 0, ECCKD_NAME_LEN);
      std::strncpy(names + (size_t)n * ECCKD_NAME_LEN, r.name, ECCKD_NAME_LEN - 1);
      total_ms[n] = 0.;
      launches[n] = 0;
      ++n;
    }
    total_ms[k] += ms;
    launches[k] += 1;
  }
  g_prof.clear();
  return n;
}

// ------------------------------- model construction -------------------------------------

int ecckd_model_begin(int ng, int np, int nt, const double *log_pressure, const double *temperature,
                      ecckd_model_t **model) {
  if (!model) return fail("ecckd_model_begin: null output");
  *model = nullptr;
  if (ng < 1 || np < 2 || nt < 2 || !log_pressure || !temperature)
    return fail("ecckd_model_begin: bad dimensions or null tables");
  ecckd_model *m = new ecckd_model;
  m->ng = ng; m->np = np; m->nt = nt;
  m->log_pressure.assign(log_pressure, log_pressure + np);
  m->temperature.assign(temperature, temperature + (size_t)np * nt);
  // default band structure: a single band over all g-points
  m->nband = 1;
  m->band2gpt = {1, ng};
  m->band_lims_wvn = {0., 0.};
  *model = m;
  return 0;
}

int ecckd_model_set_planck(ecckd_model_t *m, int ntp, const double *temperature_planck,
                           const double *planck_function) {
  if (!m || m->finalized) return fail("ecckd_model_set_planck: model missing or frozen");
  if (ntp < 2 || !temperature_planck || !planck_function) return fail("ecckd_model_set_planck: bad table");
  m->ntp = ntp;
  m->temperature_planck.assign(temperature_planck, temperature_planck + ntp);
  m->planck_function.assign(planck_function, planck_function + (size_t)m->ng * ntp);
  m->has_planck = true;
  return 0;
}

int ecckd_model_set_solar(ecckd_model_t *m, const double *solar_irradiance, const double *rayleigh) {
  if (!m || m->finalized) return fail("ecckd_model_set_solar: model missing or frozen");
  if (!solar_irradiance || !rayleigh) return fail("ecckd_model_set_solar: null table");
  m->solar_irradiance.assign(solar_irradiance, solar_irradiance + m->ng);
  m->rayleigh.assign(rayleigh, rayleigh + m->ng);
  m->total_solar_irradiance = 0.;
  for (double s : m->solar_irradiance) m->total_solar_irradiance += s;   // mo_load_coefficients.F90:89
  m->has_solar = true;
  return 0;
}

int ecckd_model_set_bands(ecckd_model_t *m, int nband, const double *band_lims_wvn, const int *band2gpt) {
  if (!m || m->finalized) return fail("ecckd_model_set_bands: model missing or frozen");
  unsigned char tmp[256];
  if (fill_band_map(m->ng, nband, band2gpt, tmp)) return 1;
  m->nband = nband;
  m->band2gpt.assign(band2gpt, band2gpt + 2 * (size_t)nband);
  if (band_lims_wvn) m->band_lims_wvn.assign(band_lims_wvn, band_lims_wvn + 2 * (size_t)nband);
  else m->band_lims_wvn.assign(2 * (size_t)nband, 0.);
  return 0;
}

int ecckd_model_add_gas(ecckd_model_t *m, const char *name, int code, int composite_only, int nv,
                        const double *mole_fraction, double reference_mole_fraction,
                        const double *coefficient) {
  if (!m || m->finalized) return fail("ecckd_model_add_gas: model missing or frozen");
  if (!name || !coefficient) return fail("ecckd_model_add_gas: null argument");
  if (m->gas.size() >= ECCKD_MAX_GASES) return fail("ecckd_model_add_gas: more than 16 gases");
  if (code < 0 || code > 3) return fail(std::string("load_and_init_ecckd: bad concentration code for ") + name);
  ecckd_model::Gas g;
  g.name = trim_name(name);
  g.code = code;
  g.composite_only = composite_only ? 1 : 0;
  g.ref = reference_mole_fraction;
  if (code == ECCKD_LOOK_UP_TABLE) {
    if (nv < 2 || !mole_fraction) return fail("ecckd_model_add_gas: look_up_table gas needs mole_fraction(nv>=2)");
    g.nv = nv;
    g.mole_fraction.assign(mole_fraction, mole_fraction + nv);
  } else {
    g.nv = 1;
  }
  g.coef.assign(coefficient, coefficient + (size_t)m->ng * m->np * m->nt * g.nv);
  m->gas.push_back(std::move(g));
  return 0;
}

int ecckd_model_finalize(ecckd_model_t *m, int device) {
  if (!m) return fail("ecckd_model_finalize: null model");
  if (m->finalized) return fail("ecckd_model_finalize: already finalized");
  {
    const std::string bad = ecckd::validate_model(*m);
    if (!bad.empty()) return fail("ecckd_model_finalize: " + bad);
  }
  if (device == -1) {   // host-only model: getters work, every compute call fails
    m->device = -1;
    m->finalized = true;
    return 0;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail("ecckd: no HIP device available (this library has no CPU fallback)");
  if (device < 0 || device >= ndev || device >= 16) return fail("ecckd_model_finalize: bad device ordinal");
  HIPCHK(hipSetDevice(device));
  // layout of the single device buffer
  std::vector<double> host;
  auto put = [&](const std::vector<double> &v) {
    size_t off = host.size();
    host.insert(host.end(), v.begin(), v.end());
    while (host.size() % 32) host.push_back(0.);
    return off;
  };
  m->off_zero = put(std::vector<double>(32, 0.));
  m->off_temperature = put(m->temperature);
  if (m->has_planck) m->off_planck = put(m->planck_function);
  if (m->has_solar) { m->off_rayleigh = put(m->rayleigh); m->off_solar = put(m->solar_irradiance); }
  for (size_t i = 0; i < m->gas.size(); ++i) {
    ecckd_model::Gas &g = m->gas[i];
    g.has_negative = false;
    for (double c : g.coef)
      if (!(c >= 0.)) { g.has_negative = true; break; }   // negatives or NaN: keep the per-g clamp
    bool shared = false;
    for (size_t k = 0; k < i && !shared; ++k) {   // o2/n2 carry identical composite tables
      const ecckd_model::Gas &o = m->gas[k];
      if (o.coef.size() == g.coef.size() &&
          std::memcmp(o.coef.data(), g.coef.data(), g.coef.size() * sizeof(double)) == 0) {
        g.dev_off = o.dev_off;
        shared = true;
      }
    }
    if (!shared) g.dev_off = put(g.coef);
  }
  HIPCHK(hipMalloc(reinterpret_cast<void **>(&m->dbuf), host.size() * sizeof(double)));
  HIPCHK(hipMemcpy(m->dbuf, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice));
  {   // the same image rounded to float, for the single-precision entry points
    std::vector<float> hostf(host.begin(), host.end());
    // ... and whether that rounding changed anything: ecCKD's files hold float32 variables (widened exactly by the reader,
    // example/rfmip-rad-irf/mo_simple_netcdf.F90:44-142), so a fp64 kernel may stage them in LDS as float32 ("gas_slab_f32")
    m->f32_exact = true;
    for (size_t i = 0; i < host.size() && m->f32_exact; ++i) m->f32_exact = (double)hostf[i] == host[i];
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&m->dbuf32), hostf.size() * sizeof(float)));
    HIPCHK(hipMemcpy(m->dbuf32, hostf.data(), hostf.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  HIPCHK(hipStreamCreateWithFlags(&m->host_stream, hipStreamNonBlocking));
  m->device = device;
  m->finalized = true;
  return 0;
}

int ecckd_model_load(const char *filename, int device, ecckd_model_t **model) {
  if (!model || !filename) return fail("ecckd_model_load: null argument");
  *model = nullptr;
  ecckd_model *m = new ecckd_model;
  try {
    ecckd::load_and_init(*m, filename);
  } catch (const std::exception &e) {
    delete m;
    return fail(e.what());
  }
  if (ecckd_model_finalize(m, device)) {
    delete m;
    return 1;
  }
  *model = m;
  return 0;
}

void ecckd_model_destroy(ecckd_model_t *m) {
  if (!m) return;
  if (m->finalized && m->device >= 0) {
    (void)hipSetDevice(m->device);
    if (m->host_stream) (void)hipStreamDestroy(m->host_stream);
    if (m->arena) (void)hipFree(m->arena);
    if (m->dbuf) (void)hipFree(m->dbuf);
    if (m->dbuf32) (void)hipFree(m->dbuf32);
  }
  delete m;
}

// ------------------------------------- getters -------------------------------------------

int ecckd_model_get_ngpt(const ecckd_model_t *m) { return m ? m->ng : 0; }
int ecckd_model_get_nband(const ecckd_model_t *m) { return m ? m->nband : 0; }
int ecckd_model_get_ngas(const ecckd_model_t *m) { return m ? (int)m->gas.size() : 0; }
int ecckd_model_get_gas_name(const ecckd_model_t *m, int index, char *name) {
  if (!m || !name || index < 0 || index >= (int)m->gas.size()) return fail("ecckd_model_get_gas_name: bad index");
  std::memset(name, 0, ECCKD_NAME_LEN);
  std::strncpy(name, m->gas[index].name.c_str(), ECCKD_NAME_LEN - 1);
  return 0;
}
int ecckd_model_source_is_internal(const ecckd_model_t *m) { return m && m->has_planck; }
int ecckd_model_source_is_external(const ecckd_model_t *m) { return m && m->has_solar; }
double ecckd_model_get_press_min(const ecckd_model_t *m) { return m ? std::exp(m->log_pressure.front()) : 0.; }
double ecckd_model_get_press_max(const ecckd_model_t *m) { return m ? std::exp(m->log_pressure.back()) : 0.; }
double ecckd_model_get_temp_min(const ecckd_model_t *m) {
  if (!m) return 0.;
  double v = m->temperature[0];
  for (double t : m->temperature) v = t < v ? t : v;
  return v;
}
double ecckd_model_get_temp_max(const ecckd_model_t *m) {
  if (!m) return 0.;
  double v = m->temperature[0];
  for (double t : m->temperature) v = t > v ? t : v;
  return v;
}
double ecckd_model_get_total_solar_irradiance(const ecckd_model_t *m) { return m ? m->total_solar_irradiance : 0.; }
int ecckd_model_get_band2gpt(const ecckd_model_t *m, int *band2gpt) {
  if (!m || !band2gpt) return fail("ecckd_model_get_band2gpt: null argument");
  std::memcpy(band2gpt, m->band2gpt.data(), m->band2gpt.size() * sizeof(int));
  return 0;
}
int ecckd_model_get_band_lims_wvn(const ecckd_model_t *m, double *lims) {
  if (!m || !lims) return fail("ecckd_model_get_band_lims_wvn: null argument");
  std::memcpy(lims, m->band_lims_wvn.data(), m->band_lims_wvn.size() * sizeof(double));
  return 0;
}
int ecckd_model_get_device(const ecckd_model_t *m) { return m ? m->device : -1; }

// ------------------------------------ gas optics -----------------------------------------

static int gas_optics_lw_dev(const ecckd_model *m, bool f32, int ncol, int nlay, const double *plev,
                             const double *tlay, const GasDesc &gd, double *tau, const PlanckSide &pl, hipStream_t stream) {
  bool planck_done = false;
  if (gas_optical_depth_dev(m, f32, nullptr, ncol, nlay, plev, tlay, gd, tau, false, nullptr, nullptr, &pl, &planck_done,
                            stream))
    return 1;   // :401
  if (planck_done) return 0;
  if (f32) return fail("ecckd: single precision is implemented for the fused longwave gas optics only");
  return planck_sources_dev(m, ncol, nlay, tlay, pl, stream);
}

int ecckd_has_level_buffer(void) { return 1; }

int ecckd_planck_sources(const ecckd_model_t *m, int ncol, int nlay, const double *tlay, const double *tlev,
                         const double *tsfc, double *lay_source, double *lev_source_inc, double *lev_source_dec,
                         double *sfc_source, int memspace, void *stream) {
  if (check_model(m) || check_gas_optics_dims(ncol, nlay)) return 1;
  if (!m->has_planck) return fail("ecckd_planck_sources: model has no Planck table (shortwave model?)");
  if (memspace != ECCKD_DEVICE) return fail("ecckd_planck_sources: device arrays only (ECCKD_DEVICE)");
  if (!tlay || !tsfc || !lay_source || !sfc_source) return fail("ecckd_planck_sources: null argument");
  if (tlev && (!lev_source_inc || !lev_source_dec)) return fail("ecckd_planck_sources: null level sources");
  HIPCHK(hipSetDevice(m->device));
  if (ncol == 0) return 0;
  LevelPair lp;
  if (level_pair("ecckd_planck_sources", tlev ? lev_source_inc : nullptr, lev_source_dec, ncol, nlay, false, memspace, true, &lp)) return 1;
  if (lp.shared && check_level_buffer_dims(ncol, nlay)) return 1;
  const PlanckSide pl{tlev, tsfc, lay_source, lev_source_inc, lev_source_dec, sfc_source, lp.gstride};
  return planck_sources_dev(m, ncol, nlay, tlay, pl, static_cast<hipStream_t>(stream));
}

int ecckd_planck_sfc_source_jac(const ecckd_model_t *m, int ncol, const double *tsfc, double *sfc_source_jac, int memspace,
                                void *stream) {
  if (check_model(m) || check_gas_optics_dims(ncol, 1)) return 1;
  if (!m->has_planck) return fail("ecckd_planck_sfc_source_jac: model has no Planck table (shortwave model?)");
  if (memspace != ECCKD_DEVICE && memspace != ECCKD_HOST) return fail("ecckd_planck_sfc_source_jac: bad memspace (ECCKD_HOST or ECCKD_DEVICE)");
  if (!tsfc || !sfc_source_jac) return fail("ecckd_planck_sfc_source_jac: null argument");
  HIPCHK(hipSetDevice(m->device));
  if (ncol == 0) return 0;
  const double t0 = m->temperature_planck[0], dt = m->temperature_planck[1] - m->temperature_planck[0];
  Stage st(const_cast<ecckd_model *>(m), memspace, stream, false);
  const double *d_tsfc = nullptr;
  double *d_jac = nullptr;
  if (st.open([&] { d_tsfc = st.in(tsfc, ncol); d_jac = st.out(sfc_source_jac, (size_t)ncol * m->ng); })) return 1;
  {
    ProfScope prof("planck_sfc_jac", st.stream);
    HIPCHK(ecckd::launch_planck_sfc_jac(m->dbuf + m->off_planck, m->ng, m->ntp, t0, dt, ncol, d_tsfc, d_jac, st.stream));
  }
  return st.close();
}

int ecckd_gas_optics_plan(const ecckd_model_t *m, int ncol, int nlay, int single_precision, int ngas,
                          const char *gas_names, int *plan) {
  int p[ECCKD_PLAN_LEN];
  if (ecckd_gas_optics_plan_ex(m, ncol, nlay, single_precision, ngas, gas_names, nullptr, ECCKD_PLAN_LEN, p)) return 1;
  if (!plan) return fail("ecckd_gas_optics_plan: null argument");
  for (int i = 0; i < 8; ++i) plan[i] = p[i];
  return 0;
}

int ecckd_gas_optics_plan_ex(const ecckd_model_t *m, int ncol, int nlay, int single_precision, int ngas,
                             const char *gas_names, const int *vmr_is_scalar, int nplan, int *plan_out) {
  if (!m) return fail("ecckd: null model");
  if (!m->finalized) return fail("ecckd: model is not finalized");
  if (check_gas_optics_dims(ncol, nlay)) return 1;
  if (!plan_out || nplan < 1 || (ngas > 0 && !gas_names)) return fail("ecckd_gas_optics_plan: null argument");
  int plan[ECCKD_PLAN_LEN] = {0};
  PlanRecord rec;
  rec.is_scalar = vmr_is_scalar;
  const GasDesc gd{ngas, gas_names, nullptr, nullptr, nullptr, nullptr};
  const PlanckSide pl{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const bool lw = m->has_planck;
  bool planck_done = false;
  if (gas_optical_depth_dev(m, single_precision != 0, &rec, ncol, nlay, nullptr, nullptr, gd, nullptr, !lw, nullptr,
                            nullptr, lw ? &pl : nullptr, &planck_done, nullptr))
    return 1;
  plan[0] = rec.npass;
  plan[1] = rec.first_fused;
  plan[2] = rec.planck_fused;
  plan[3] = rec.first.slab_rows;
  plan[4] = rec.first.planck_rows;
  plan[5] = rec.first.col_chunks;
  plan[6] = (int)rec.first.lds_bytes;
  plan[7] = rec.first.GC;
  plan[8] = rec.first.NB;
  plan[9] = rec.first.merged;
  for (int i = 0; i < nplan && i < ECCKD_PLAN_LEN; ++i) plan_out[i] = plan[i];
  return 0;
}

static int gas_optics_lw_impl(bool f32, const ecckd_model_t *m, int ncol, int nlay, const double *plev, const double *tlay,
                              const double *tsfc, const double *tlev, int ngas, const char *gas_names,
                              const double *const *vmr, const long long *vmr_col_stride, const long long *vmr_lay_stride,
                              const double *vmr_scalar, double *tau, double *lay_source, double *lev_source_inc,
                              double *lev_source_dec, double *sfc_source, int memspace, void *stream) {
  if (check_model(m) || check_gas_optics_dims(ncol, nlay)) return 1;
  if (!m->has_planck) return fail("ecckd_gas_optics_lw: model has no Planck table (shortwave model?)");
  if (!plev || !tlay || !tsfc || !tau || !lay_source || !sfc_source || (ngas > 0 && !gas_names))
    return fail("ecckd_gas_optics_lw: null argument");
  if (tlev && (!lev_source_inc || !lev_source_dec)) return fail("ecckd_gas_optics_lw: null level sources");
  HIPCHK(hipSetDevice(m->device));
  const GasDesc gd{ngas, gas_names, vmr, vmr_col_stride, vmr_lay_stride, vmr_scalar};
  if (ncol == 0) return tlev ? 0 : fail("tlev is required for ecckd");
  if (memspace != ECCKD_DEVICE && memspace != ECCKD_HOST && memspace != ECCKD_MIXED) return fail("ecckd: bad memspace");
  LevelPair lp;
  if (level_pair("ecckd_gas_optics_lw", tlev ? lev_source_inc : nullptr, lev_source_dec, ncol, nlay, f32, memspace, true, &lp)) return 1;
  if (lp.shared && check_level_buffer_dims(ncol, nlay)) return 1;
  // ECCKD_MIXED: inputs are host arrays (staged here), the (ncol,nlay,ngpt) / (ncol,ngpt) outputs are the caller's
  // device buffers: nothing but ~4 KB per column crosses the bus
  const Counts n(ncol, nlay, m->ng, m->nband);
  Stage st(const_cast<ecckd_model *>(m), memspace, stream, f32);
  const double *d_plev = nullptr, *d_tlay = nullptr;
  PlanckSide pl{};
  GasDesc d_gd{};
  double *d_tau = nullptr;
  if (st.open([&] {
        d_plev = st.in(plev, n.lev); d_tlay = st.in(tlay, n.lay);
        pl.tsfc = st.in(tsfc, n.col); pl.tlev = st.in(tlev, n.lev);
        d_gd = st.gases(gd, ncol, nlay);
        d_tau = st.out(tau, n.lay_g, kBig);
        pl.lay_source = st.out(lay_source, n.lay_g, kBig); pl.sfc_source = st.out(sfc_source, n.col_g, kBig);
        // (without tlev the level sources are not produced: nothing to copy back)
        pl.lev_inc = st.out(lev_source_inc, n.lay_g, kBig, tlev != nullptr);
        pl.lev_dec = st.out(lev_source_dec, n.lay_g, kBig, tlev != nullptr);
      }))
    return 1;
  pl.lev_gstride = lp.gstride;
  if (gas_optics_lw_dev(m, f32, ncol, nlay, d_plev, d_tlay, d_gd, d_tau, pl, st.stream)) return 1;
  if (st.close()) return 1;   // (ECCKD_MIXED synchronises too: the solver call that follows runs on another stream)
  return tlev ? 0 : fail("tlev is required for ecckd");   // :414-417
}

int ecckd_gas_optics_lw(const ecckd_model_t *m, int ncol, int nlay, const double *plev,
                        const double *tlay, const double *tsfc, const double *tlev, int ngas,
                        const char *gas_names, const double *const *vmr,
                        const long long *vmr_col_stride, const long long *vmr_lay_stride,
                        const double *vmr_scalar, double *tau, double *lay_source,
                        double *lev_source_inc, double *lev_source_dec, double *sfc_source,
                        int memspace, void *stream) {
  return gas_optics_lw_impl(false, m, ncol, nlay, plev, tlay, tsfc, tlev, ngas, gas_names, vmr, vmr_col_stride,
                            vmr_lay_stride, vmr_scalar, tau, lay_source, lev_source_inc, lev_source_dec, sfc_source,
                            memspace, stream);
}

int ecckd_gas_optics_lw_f32(const ecckd_model_t *m, int ncol, int nlay, const float *plev, const float *tlay,
                            const float *tsfc, const float *tlev, int ngas, const char *gas_names,
                            const float *const *vmr, const long long *vmr_col_stride,
                            const long long *vmr_lay_stride, const double *vmr_scalar, float *tau,
                            float *lay_source, float *lev_source_inc, float *lev_source_dec,
                            float *sfc_source, int memspace, void *stream) {
  return gas_optics_lw_impl(true, m, ncol, nlay, dp(plev), dp(tlay), dp(tsfc), dp(tlev), ngas, gas_names,
                            reinterpret_cast<const double *const *>(vmr), vmr_col_stride, vmr_lay_stride, vmr_scalar,
                            dp(tau), dp(lay_source), dp(lev_source_inc), dp(lev_source_dec), dp(sfc_source), memspace,
                            stream);
}

static int gas_optics_sw_dev(const ecckd_model *m, bool f32, int ncol, int nlay, const double *plev,
                             const double *tlay, const GasDesc &gd, double *tau, double *ssa,
                             double *g, double *toa_src, hipStream_t stream) {
  const bool two_stream = ssa && g;
  if (gas_optical_depth_dev(m, f32, nullptr, ncol, nlay, plev, tlay, gd, tau, true, two_stream ? ssa : nullptr,
                            two_stream ? g : nullptr, nullptr, nullptr, stream))   // :449-460
    return 1;
  if (!two_stream) return 0;   // caller reports :461-463 after tau has been written
  HIPCHK(ecckd::launch_toa_src(table(m, m->off_solar, f32), ncol, m->ng, toa_src, f32, stream));   // :468-472
  return 0;
}

static int gas_optics_sw_impl(bool f32, const ecckd_model_t *m, int ncol, int nlay, const double *plev, const double *tlay,
                              int ngas, const char *gas_names, const double *const *vmr, const long long *vmr_col_stride,
                              const long long *vmr_lay_stride, const double *vmr_scalar, double *tau, double *ssa,
                              double *g, double *toa_src, int memspace, void *stream) {
  if (check_model(m) || check_gas_optics_dims(ncol, nlay)) return 1;
  if (!m->has_solar) return fail("ecckd_gas_optics_sw: model has no solar table (longwave model?)");
  if (!plev || !tlay || !tau || (ngas > 0 && !gas_names)) return fail("ecckd_gas_optics_sw: null argument");
  const bool two_stream = ssa && g;
  if (two_stream && !toa_src) return fail("ecckd_gas_optics_sw: null toa_src");
  HIPCHK(hipSetDevice(m->device));
  const GasDesc gd{ngas, gas_names, vmr, vmr_col_stride, vmr_lay_stride, vmr_scalar};
  static const char *kNot2str = "shortwave must use ty_optical_props_2str";   // :462
  if (ncol == 0) return two_stream ? 0 : fail(kNot2str);
  if (memspace != ECCKD_DEVICE && memspace != ECCKD_HOST && memspace != ECCKD_MIXED) return fail("ecckd: bad memspace");
  // ECCKD_MIXED: tau, ssa, g are the caller's device buffers; toa_src and the inputs are host arrays
  const Counts n(ncol, nlay, m->ng, m->nband);
  Stage st(const_cast<ecckd_model *>(m), memspace, stream, f32);
  const double *d_plev = nullptr, *d_tlay = nullptr;
  GasDesc d_gd{};
  double *d_tau = nullptr, *d_ssa = nullptr, *d_g = nullptr, *d_toa = nullptr;
  if (st.open([&] {
        d_plev = st.in(plev, n.lev); d_tlay = st.in(tlay, n.lay);
        d_gd = st.gases(gd, ncol, nlay);
        d_tau = st.out(tau, n.lay_g, kBig);
        d_ssa = st.out(ssa, n.lay_g, kBig, two_stream); d_g = st.out(g, n.lay_g, kBig, two_stream);
        d_toa = st.out(toa_src, n.col_g, false, two_stream);
      }))
    return 1;
  if (gas_optics_sw_dev(m, f32, ncol, nlay, d_plev, d_tlay, d_gd, d_tau, d_ssa, d_g, d_toa, st.stream)) return 1;
  if (st.close()) return 1;
  return two_stream ? 0 : fail(kNot2str);
}

int ecckd_gas_optics_sw(const ecckd_model_t *m, int ncol, int nlay, const double *plev,
                        const double *tlay, int ngas, const char *gas_names,
                        const double *const *vmr, const long long *vmr_col_stride,
                        const long long *vmr_lay_stride, const double *vmr_scalar, double *tau,
                        double *ssa, double *g, double *toa_src, int memspace, void *stream) {
  return gas_optics_sw_impl(false, m, ncol, nlay, plev, tlay, ngas, gas_names, vmr, vmr_col_stride, vmr_lay_stride,
                            vmr_scalar, tau, ssa, g, toa_src, memspace, stream);
}

int ecckd_gas_optics_sw_f32(const ecckd_model_t *m, int ncol, int nlay, const float *plev, const float *tlay, int ngas,
                            const char *gas_names, const float *const *vmr, const long long *vmr_col_stride,
                            const long long *vmr_lay_stride, const double *vmr_scalar, float *tau, float *ssa, float *g,
                            float *toa_src, int memspace, void *stream) {
  return gas_optics_sw_impl(true, m, ncol, nlay, dp(plev), dp(tlay), ngas, gas_names,
                            reinterpret_cast<const double *const *>(vmr), vmr_col_stride, vmr_lay_stride, vmr_scalar,
                            dp(tau), dp(ssa), dp(g), dp(toa_src), memspace, stream);
}

// -------------------------------------- solvers ------------------------------------------

// Gauss-Jacobi-5 quadrature of RTE-RRTMGP's mo_rte_lw (secants and weights for 1..4 angles;
// ecckd_rfmip_lw.F90:40-44 selects 1 or 3).
static const double kGaussDs[4][4] = {{1.66, 0., 0., 0.},
                                      {1.18350343, 2.81649655, 0., 0.},
                                      {1.09719858, 1.69338507, 4.70941630, 0.},
                                      {1.06056257, 1.38282560, 2.40148179, 7.15513024}};
static const double kGaussWts[4][4] = {{0.5, 0., 0., 0.},
                                       {0.3180413817, 0.1819586183, 0., 0.},
                                       {0.2009319137, 0.2292411064, 0.0698269799, 0.},
                                       {0.1355069134, 0.2034645680, 0.1298475476, 0.0311809710}};

// The longwave solver's switches (ecckd_set_solver_option) and its n_gauss_angles quadrature angles
static void fill_lw_options(ecckd::RteLwArgs &a, int n_gauss_angles, bool f32) {
  a.nmus = n_gauss_angles;
  a.tau_thresh = lw_tau_thresh(f32);
  a.series3 = g_opt.lw_series_terms.load() == 3;
  a.inc_isotropic = g_opt.lw_inc_flux_isotropic.load();
  a.use_split = g_opt.lw_solver.load();
  a.split_seg = g_opt.lw_split_seg.load();
  for (int k = 0; k < n_gauss_angles; ++k) {
    a.Ds[k] = kGaussDs[n_gauss_angles - 1][k];
    a.wts[k] = kGaussWts[n_gauss_angles - 1][k];
  }
}

static int check_device(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail("ecckd: no HIP device available (this library has no CPU fallback)");
  if (device < 0 || device >= ndev || device >= 16) return fail("ecckd: bad device ordinal");
  HIPCHK(hipSetDevice(device));
  return 0;
}

static int rte_lw_impl(const Call &c, int device, int ncol, int nlay, int ngpt, int top_at_1, int n_gauss_angles,
                       const double *tau, const double *lay_source, const double *lev_source_inc, const double *lev_source_dec,
                       const double *sfc_source, int nband, const int *band2gpt, const double *sfc_emis,
                       const double *inc_flux, double *flux_up, double *flux_dn, int memspace, void *stream) {
  if (check_dims(ncol, nlay)) return 1;
  if (n_gauss_angles < 1 || n_gauss_angles > 4) return fail("rte_lw: have to ask for at least one quadrature point and no more than 4");
  if (!tau || !lay_source || !lev_source_inc || !lev_source_dec || !sfc_source || !sfc_emis || !flux_up || !flux_dn)
    return fail("ecckd_rte_lw: null argument");
  ecckd::RteLwArgs a{};
  if (c.band >= 0) std::memset(a.gpt2band, c.band, sizeof a.gpt2band);
  else if (fill_band_map(ngpt, nband, band2gpt, a.gpt2band)) return 1;
  if (check_device(device)) return 1;
  if (ncol == 0) return 0;
  a.ncol = ncol; a.nlay = nlay; a.ng = ngpt; a.top_at_1 = top_at_1 ? 1 : 0;
  a.nband = nband;
  a.f32 = c.f32;
  // one level buffer behind the two arrays: its levels ARE shared, whichever entry point was called
  LevelPair lp;
  if (level_pair("ecckd_rte_lw", lev_source_inc, lev_source_dec, ncol, nlay, c.f32, memspace, true, &lp)) return 1;
  a.shared_levels = c.shared_levels || lp.shared;
  a.lev_gstride = lp.gstride;
  fill_lw_options(a, n_gauss_angles, c.f32);
  const size_t scratch = ecckd::rte_lw_scratch_bytes(ncol, nlay, ngpt);
  Stage st(device, memspace, stream, c.f32);
  ScratchLease lease;   // (held until the kernels of this call have been launched)
  if (scratch) {   // more than 96 layers: stream-ordered scratch ring, no synchronisation (see ScratchPool)
    void *sp = nullptr;
    if (stream_scratch(device, st.stream, scratch, &sp, lease)) return 1;
    a.scratch = static_cast<double *>(sp);
  } else if (g_opt.lw_tail_split.load()) {   // tail tiles one g-pair per wave (rte_lw_tail_plan); optional, same bits
    long first = -1;
    const size_t need = ecckd::rte_lw_tail_plan(a, simd_slots(device), &first);
    if (need) {
      if (void *sp = stream_scratch_optional(device, st.stream, need, lease)) {
        a.partials = static_cast<double *>(sp);
        a.tail_first = first;
      }
    }
  }
  if (memspace != ECCKD_DEVICE && memspace != ECCKD_HOST && memspace != ECCKD_MIXED) return fail("ecckd: bad memspace");
  // ECCKD_MIXED: tau, the three source arrays and sfc_source are device buffers (what gas_optics left there);
  // sfc_emis / inc_flux come from the host and the fluxes go back to it
  const Counts n(ncol, nlay, ngpt, nband);
  if (st.open([&] {
        a.tau = st.in(tau, n.lay_g, kBig); a.lay_source = st.in(lay_source, n.lay_g, kBig);
        a.lev_source_inc = st.in(lev_source_inc, n.lay_g, kBig); a.lev_source_dec = st.in(lev_source_dec, n.lay_g, kBig);
        a.sfc_source = st.in(sfc_source, n.col_g, kBig);
        a.sfc_emis = st.in(sfc_emis, n.col_b); a.inc_flux = st.in(inc_flux, n.col_g);
        a.flux_up = st.out(flux_up, n.lev); a.flux_dn = st.out(flux_dn, n.lev);
      }))
    return 1;
  {
    ProfScope prof("rte_lw", st.stream);
    HIPCHK(ecckd::launch_rte_lw(a, st.stream));
  }
  return st.close();
}

int ecckd_rte_lw(int device, int ncol, int nlay, int ngpt, int top_at_1, int n_gauss_angles,
                 const double *tau, const double *lay_source, const double *lev_source_inc,
                 const double *lev_source_dec, const double *sfc_source, int nband,
                 const int *band2gpt, const double *sfc_emis, double *flux_up, double *flux_dn,
                 int memspace, void *stream) {
  return rte_lw_impl(Call{}, device, ncol, nlay, ngpt, top_at_1, n_gauss_angles, tau, lay_source, lev_source_inc,
                     lev_source_dec, sfc_source, nband, band2gpt, sfc_emis, nullptr, flux_up, flux_dn, memspace, stream);
}

int ecckd_rte_lw_f32(int device, int ncol, int nlay, int ngpt, int top_at_1, int n_gauss_angles, const float *tau,
                     const float *lay_source, const float *lev_source_inc, const float *lev_source_dec,
                     const float *sfc_source, int nband, const int *band2gpt, const float *sfc_emis,
                     float *flux_up, float *flux_dn, int memspace, void *stream) {
  return rte_lw_impl(Call{true}, device, ncol, nlay, ngpt, top_at_1, n_gauss_angles, dp(tau), dp(lay_source),
                     dp(lev_source_inc), dp(lev_source_dec), dp(sfc_source), nband, band2gpt, dp(sfc_emis), nullptr,
                     dp(flux_up), dp(flux_dn), memspace, stream);
}

int ecckd_rte_lw_shared_levels(int device, int ncol, int nlay, int ngpt, int top_at_1, int n_gauss_angles,
                               const double *tau, const double *lay_source, const double *lev_source_inc,
                               const double *lev_source_dec, const double *sfc_source, int nband,
                               const int *band2gpt, const double *sfc_emis, double *flux_up, double *flux_dn,
                               int memspace, void *stream) {
  return rte_lw_impl(Call{false, -1, /*shared_levels*/ true}, device, ncol, nlay, ngpt, top_at_1, n_gauss_angles, tau,
                     lay_source, lev_source_inc, lev_source_dec, sfc_source, nband, band2gpt, sfc_emis, nullptr,
                     flux_up, flux_dn, memspace, stream);
}

int ecckd_rte_lw_inc_flux(int device, int ncol, int nlay, int ngpt, int top_at_1, int n_gauss_angles,
                          const double *tau, const double *lay_source, const double *lev_source_inc,
                          const double *lev_source_dec, const double *sfc_source, int nband,
                          const int *band2gpt, const double *sfc_emis, const double *inc_flux, double *flux_up,
                          double *flux_dn, int memspace, void *stream) {
  return rte_lw_impl(Call{}, device, ncol, nlay, ngpt, top_at_1, n_gauss_angles, tau, lay_source, lev_source_inc,
                     lev_source_dec, sfc_source, nband, band2gpt, sfc_emis, inc_flux, flux_up, flux_dn, memspace, stream);
}

int ecckd_rte_lw_inc_flux_f32(int device, int ncol, int nlay, int ngpt, int top_at_1, int n_gauss_angles, const float *tau,
                              const float *lay_source, const float *lev_source_inc, const float *lev_source_dec,
                              const float *sfc_source, int nband, const int *band2gpt, const float *sfc_emis,
                              const float *inc_flux, float *flux_up, float *flux_dn, int memspace, void *stream) {
  return rte_lw_impl(Call{true}, device, ncol, nlay, ngpt, top_at_1, n_gauss_angles, dp(tau), dp(lay_source),
                     dp(lev_source_inc), dp(lev_source_dec), dp(sfc_source), nband, band2gpt, dp(sfc_emis), dp(inc_flux),
                     dp(flux_up), dp(flux_dn), memspace, stream);
}

// The Jacobian kernel's arguments for a solver call: the quadrature of fill_lw_options, nothing of the version switches
static void fill_jac_args(ecckd::RteLwJacArgs &j, int ncol, int nlay, int ngpt, int top_at_1, int n_gauss_angles, int nband) {
  j.ncol = ncol; j.nlay = nlay; j.ng = ngpt; j.top_at_1 = top_at_1 ? 1 : 0; j.nmus = n_gauss_angles; j.nband = nband;
  for (int k = 0; k < n_gauss_angles; ++k) {
    j.Ds[k] = kGaussDs[n_gauss_angles - 1][k];
    j.wts[k] = kGaussWts[n_gauss_angles - 1][k];
  }
}

int ecckd_rte_lw_jac(int device, int ncol, int nlay, int ngpt, int top_at_1, int n_gauss_angles, const double *tau,
                     const double *lay_source, const double *lev_source_inc, const double *lev_source_dec,
                     const double *sfc_source, const double *sfc_source_jac, int nband, const int *band2gpt,
                     const double *sfc_emis, const double *inc_flux, double *flux_up, double *flux_dn, double *flux_up_jac,
                     int memspace, void *stream) {
  // the refusals of ecckd_rte_lw_inc_flux that need no device, then this call's own, all before the first launch
  if (check_dims(ncol, nlay)) return 1;
  if (n_gauss_angles < 1 || n_gauss_angles > 4) return fail("rte_lw: have to ask for at least one quadrature point and no more than 4");
  if (!tau || !lay_source || !lev_source_inc || !lev_source_dec || !sfc_source || !sfc_emis || !flux_up || !flux_dn)
    return fail("ecckd_rte_lw: null argument");
  if (!sfc_source_jac || !flux_up_jac) return fail("ecckd_rte_lw_jac: null argument (sfc_source_jac and flux_up_jac are required)");
  if (flux_up_jac == flux_up || flux_up_jac == flux_dn) return fail("ecckd_rte_lw_jac: flux_up_jac must not be one of the flux outputs");
  if (memspace != ECCKD_HOST && memspace != ECCKD_DEVICE) return fail("ecckd_rte_lw_jac: bad memspace (ECCKD_HOST or ECCKD_DEVICE)");
  ecckd::RteLwJacArgs j{};
  if (fill_band_map(ngpt, nband, band2gpt, j.gpt2band)) return 1;
  if (rte_lw_impl(Call{}, device, ncol, nlay, ngpt, top_at_1, n_gauss_angles, tau, lay_source, lev_source_inc, lev_source_dec,
                  sfc_source, nband, band2gpt, sfc_emis, inc_flux, flux_up, flux_dn, memspace, stream))
    return 1;
  if (ncol == 0) return 0;
  fill_jac_args(j, ncol, nlay, ngpt, top_at_1, n_gauss_angles, nband);
  // (host arrays: staged once more, behind the flux call, which has copied its fluxes back and let the arena go)
  const Counts n(ncol, nlay, ngpt, nband);
  Stage st(device, memspace, stream, false);
  if (st.open([&] {
        j.tau = st.in(tau, n.lay_g); j.sfc_source_jac = st.in(sfc_source_jac, n.col_g); j.sfc_emis = st.in(sfc_emis, n.col_b);
        j.flux_up_jac = st.out(flux_up_jac, n.lev);
      }))
    return 1;
  {
    ProfScope prof("rte_lw_jac", st.stream);
    HIPCHK(ecckd::launch_rte_lw_jac(j, nullptr, 0, 0., 1., st.stream));
  }
  return st.close();
}

static const double kSwKFloorF32 = 1.e-6;      // lower bound of "sw_k_floor" in the single-precision shortwave solvers ...
static const double kSwKFloorTauF32 = 1.e-4;   // ... which a cell of optical depth tau lowers to this / tau^2 (k tau = 1e-2)

static int rte_sw_impl(const Call &c, int device, int ncol, int nlay, int ngpt, int top_at_1, const double *tau,
                       const double *ssa, const double *g, const double *mu0, const double *toa_flux, int nband,
                       const int *band2gpt, const double *sfc_alb_dir, const double *sfc_alb_dif, double *flux_up,
                       double *flux_dn, double *flux_dir, int memspace, void *stream) {
  if (check_dims(ncol, nlay)) return 1;
  if (!tau || !mu0 || !sfc_alb_dir || !sfc_alb_dif || !flux_up || !flux_dn || (!c.derive && (!ssa || !g || !toa_flux)))
    return fail("ecckd_rte_sw: null argument");
  ecckd::RteSwArgs a{};
  if (c.band >= 0) std::memset(a.gpt2band, c.band, sizeof a.gpt2band);
  else if (fill_band_map(ngpt, nband, band2gpt, a.gpt2band)) return 1;
  if (check_device(device)) return 1;
  if (ncol == 0) return 0;
  a.ncol = ncol; a.nlay = nlay; a.ng = ngpt; a.top_at_1 = top_at_1 ? 1 : 0; a.nband = nband;
  a.exact_division = g_arith.load() != 0;
  a.k_floor = g_opt.sw_k_floor.load();
  // (fast arithmetic mode: sw_sqrt() of sw_two_stream.hpp takes normal numbers; a subnormal floor changes nothing a flux can show)
  if (!a.exact_division && a.k_floor < 2.2250738585072014e-308) a.k_floor = 2.2250738585072014e-308;
  // single precision: a conservative layer (ssa == 1, as float rounds anything above 1 - 3e-8) sits on the floor, and with
  // k = 1e-6 float keeps no digit of 1 - exp(-2 k tau): fluxes 8-12 W m-2 from the solution of the k = 0 equations.
  // Rounding costs about eps / (k tau) of a cell's reflectance, the floor (k tau)^2 / 12: what counts is k tau, and 5e-3 to
  // 1e-2 serves both (tests/test_gpu_solver_truth.py: 0.01 W m-2 for tau <= 5 with k^2 = 1e-6).  A constant 1e-6 would reach
  // too far in thick cells: (g1-g2)(g1+g2) = 2 (1-w) (2 - w/2 - 1.5 w g) is below it for 1 - w < 3.4e-7 at g = 0 but for
  // 1 - w < 2.2e-6 at g = 0.85, and raising k of three cloud layers of tau = 100, ssa = 1 - 1e-6, g = 0.85 from 6.7e-4 to 1e-3
  // moves the fluxes by 9.5 W m-2 (measured in fp64 with that floor).  So the bound of a cell is min(1e-6, 1e-4 / tau^2): 1e-6
  // up to tau = 10, k tau = 1e-2 beyond.  A "sw_k_floor" of 1e-6 or more holds in every cell as it is set.
  if (c.f32 && a.k_floor < kSwKFloorF32) { a.k_floor = kSwKFloorF32; a.k_floor_tau = kSwKFloorTauF32; }
  a.dir_clamp = g_opt.sw_dir_clamp.load();
  a.f32 = c.f32;
  const SwDerive *dv = c.derive;
  if (dv) {   // ecckd_sw_fluxes: ssa / g / toa derived inside the solver (RteSwArgs::derive)
    a.derive = 1;
    a.plev = dv->plev; a.rayleigh = dv->rayleigh; a.solar = dv->solar; a.gw = dv->gw;
    a.toa_scale = dv->toa_scale;
    if (dv->part_tau) { a.allsky = 1; a.part_tau = dv->part_tau; a.part_ssa = dv->part_ssa; a.part_g = dv->part_g; a.part_mask = dv->part_mask; }
    if (dv->part_mask && dv->mask_first >= 0) { a.mask_window = 1; a.mask_first = dv->mask_first; }
    if (dv->part_scaling) { a.part_scaling = dv->part_scaling; a.mask_window = 2; }
  }
  Stage st(device, memspace, stream, c.f32);
  ScratchLease lease;   // (held until the kernels of this call have been launched)
  const int cus = simd_slots(device) / 4;
  a.use_sys = g_opt.sw_solver.load() == 0 && ecckd::rte_sw_sys_applies(a) && cus > 0 && a.mask_window != 2;
  if (a.use_sys) {
    // layer-systolic solver: no scratch ring; the g-point chunks of the last part-empty round go through partial sums
    if (g_opt.sw_tail_split.load()) {
      const size_t need = ecckd::rte_sw_sys_plan(a, cus);
      if (need) {
        if (dv) a.partials = dv->room;   // (ecckd_sw_fluxes sized its block with sw_fluxes_solver_bytes)
        else if (void *sp = stream_scratch_optional(device, st.stream, need, lease)) a.partials = static_cast<double *>(sp);
        if (!a.partials) { a.sys_tail_first = -1; a.sys_gchunk = 0; }
      }
    }
  } else if (dv) {
    // two-pass solver inside ecckd_sw_fluxes: the stream's scratch block holds the optical depth, so the ring and the
    // partial sums come from the room behind it (sw_fluxes_solver_bytes), never from stream_scratch
    a.scratch = dv->room;
    if (!a.scratch) return fail("ecckd_rte_sw: the fused shortwave path has no room for the two-pass solver's scratch ring");
    if (g_opt.sw_tail_split.load()) {
      long first = -1;
      size_t partials_at = 0;
      if (ecckd::rte_sw_tail_plan(a, &first, &partials_at)) {
        a.partials = reinterpret_cast<double *>(reinterpret_cast<char *>(dv->room) + partials_at);
        a.tail_first = first;
      }
    }
  } else {
  const size_t scratch = ecckd::rte_sw_scratch_bytes(ncol, nlay, ngpt);
  if (g_opt.sw_tail_split.load()) {   // tail tiles one g-point group per wave (rte_sw_tail_plan); optional, same bits
    long first = -1;
    size_t partials_at = 0;
    const size_t need = ecckd::rte_sw_tail_plan(a, &first, &partials_at);
    if (need) {
      if (void *sp = stream_scratch_optional(device, st.stream, need > scratch ? need : scratch, lease)) {
        a.scratch = static_cast<double *>(sp);
        a.partials = reinterpret_cast<double *>(static_cast<char *>(sp) + partials_at);
        a.tail_first = first;
      }
    }
  }
  if (scratch && a.tail_first < 0) {   // stream-ordered scratch ring, no synchronisation (see ScratchPool)
    void *sp = nullptr;
    if (stream_scratch(device, st.stream, scratch, &sp, lease)) return 1;
    a.scratch = static_cast<double *>(sp);
  }
  }
  if (memspace != ECCKD_DEVICE && memspace != ECCKD_HOST && memspace != ECCKD_MIXED) return fail("ecckd: bad memspace");
  // ECCKD_MIXED: tau, ssa, g are device buffers; everything else is host
  const Counts n(ncol, nlay, ngpt, nband);
  if (st.open([&] {
        a.tau = st.in(tau, n.lay_g, kBig); a.ssa = st.in(ssa, n.lay_g, kBig); a.g = st.in(g, n.lay_g, kBig);
        a.mu0 = st.in(mu0, n.col); a.toa = st.in(toa_flux, n.col_g);
        a.alb_dir = st.in(sfc_alb_dir, n.col_b); a.alb_dif = st.in(sfc_alb_dif, n.col_b);
        a.flux_up = st.out(flux_up, n.lev); a.flux_dn = st.out(flux_dn, n.lev); a.flux_dir = st.out(flux_dir, n.lev);
      }))
    return 1;
  {
    ProfScope prof("rte_sw", st.stream);
    HIPCHK(a.use_sys ? ecckd::launch_rte_sw_sys(a, cus, st.stream) : ecckd::launch_rte_sw(a, st.stream));
  }
  return st.close();
}

int ecckd_rte_sw(int device, int ncol, int nlay, int ngpt, int top_at_1, const double *tau,
                 const double *ssa, const double *g, const double *mu0, const double *toa_flux,
                 int nband, const int *band2gpt, const double *sfc_alb_dir,
                 const double *sfc_alb_dif, double *flux_up, double *flux_dn, double *flux_dir,
                 int memspace, void *stream) {
  return rte_sw_impl(Call{}, device, ncol, nlay, ngpt, top_at_1, tau, ssa, g, mu0, toa_flux, nband, band2gpt,
                     sfc_alb_dir, sfc_alb_dif, flux_up, flux_dn, flux_dir, memspace, stream);
}

int ecckd_rte_sw_f32(int device, int ncol, int nlay, int ngpt, int top_at_1, const float *tau, const float *ssa, const float *g,
                     const float *mu0, const float *toa_flux, int nband, const int *band2gpt, const float *sfc_alb_dir,
                     const float *sfc_alb_dif, float *flux_up, float *flux_dn, float *flux_dir, int memspace, void *stream) {
  return rte_sw_impl(Call{true}, device, ncol, nlay, ngpt, top_at_1, dp(tau), dp(ssa), dp(g), dp(mu0), dp(toa_flux), nband,
                     band2gpt, dp(sfc_alb_dir), dp(sfc_alb_dif), dp(flux_up), dp(flux_dn), dp(flux_dir), memspace, stream);
}

// ---- RTE-RRTMGP's kernel-level interfaces: spectral fluxes (ncol,nlay+1,ngpt), sum_broadband ----

static void fill_gpt_options(ecckd::RteGptArgs &a) {
  a.tau_thresh = lw_tau_thresh(false);
  a.series3 = g_opt.lw_series_terms.load() == 3;
  a.inc_isotropic = g_opt.lw_inc_flux_isotropic.load();
  a.k_floor = g_opt.sw_k_floor.load();
  a.dir_clamp = g_opt.sw_dir_clamp.load();
}

int ecckd_lw_solver_noscat_gpt(int device, int ncol, int nlay, int ngpt, int top_at_1, int nmus, const double *Ds,
                               const double *weights, const double *tau, const double *lay_source,
                               const double *lev_source_inc, const double *lev_source_dec, const double *sfc_emis,
                               const double *sfc_src, const double *inc_flux, double *gpt_flux_up, double *gpt_flux_dn,
                               int memspace, void *stream) {
  if (check_dims(ncol, nlay)) return 1;
  if (ngpt < 1) return fail("ecckd_lw_solver_noscat_gpt: bad ngpt");
  if (nmus < 1 || nmus > 4 || !Ds || !weights) return fail("ecckd_lw_solver_noscat_gpt: 1..4 quadrature angles with Ds and weights");
  if (!tau || !lay_source || !lev_source_inc || !lev_source_dec || !sfc_emis || !sfc_src || !gpt_flux_up || !gpt_flux_dn)
    return fail("ecckd_lw_solver_noscat_gpt: null argument");
  if (refuse_level_buffer("ecckd_lw_solver_noscat_gpt", lev_source_inc, lev_source_dec, ncol, nlay, memspace)) return 1;
  if (check_device(device)) return 1;
  if (ncol == 0) return 0;
  ecckd::RteGptArgs a{};
  a.ncol = ncol; a.nlay = nlay; a.ng = ngpt; a.top_at_1 = top_at_1 ? 1 : 0; a.nmus = nmus;
  for (int k = 0; k < nmus; ++k) { a.Ds[k] = Ds[k]; a.wts[k] = weights[k]; }
  fill_gpt_options(a);
  if (memspace != ECCKD_DEVICE && memspace != ECCKD_HOST) return fail("ecckd: bad memspace");
  const Counts n(ncol, nlay, ngpt, 1);
  Stage st(device, memspace, stream, false);
  if (st.open([&] {
        a.tau = st.in(tau, n.lay_g); a.lay_source = st.in(lay_source, n.lay_g);
        a.lev_source_inc = st.in(lev_source_inc, n.lay_g); a.lev_source_dec = st.in(lev_source_dec, n.lay_g);
        a.sfc_emis = st.in(sfc_emis, n.col_g); a.sfc_src = st.in(sfc_src, n.col_g); a.inc_flux = st.in(inc_flux, n.col_g);
        a.flux_up = st.out(gpt_flux_up, n.lev * ngpt); a.flux_dn = st.out(gpt_flux_dn, n.lev * ngpt);
      }))
    return 1;
  {
    ProfScope prof("lw_gpt", st.stream);
    HIPCHK(ecckd::launch_lw_gpt(a, st.stream));
  }
  return st.close();
}

int ecckd_sw_solver_2stream_gpt(int device, int ncol, int nlay, int ngpt, int top_at_1, const double *tau, const double *ssa,
                                const double *g, const double *mu0, const double *flux_dir_top, const double *inc_flux_dif,
                                const double *sfc_alb_dir, const double *sfc_alb_dif, double *gpt_flux_up, double *gpt_flux_dn,
                                double *gpt_flux_dir, int memspace, void *stream) {
  if (check_dims(ncol, nlay)) return 1;
  if (ngpt < 1) return fail("ecckd_sw_solver_2stream_gpt: bad ngpt");
  if (!tau || !ssa || !g || !mu0 || !flux_dir_top || !sfc_alb_dir || !sfc_alb_dif || !gpt_flux_up || !gpt_flux_dn)
    return fail("ecckd_sw_solver_2stream_gpt: null argument");
  if (check_device(device)) return 1;
  if (ncol == 0) return 0;
  ecckd::RteGptArgs a{};
  a.ncol = ncol; a.nlay = nlay; a.ng = ngpt; a.top_at_1 = top_at_1 ? 1 : 0; a.nmus = 1;
  fill_gpt_options(a);
  if (memspace != ECCKD_DEVICE && memspace != ECCKD_HOST) return fail("ecckd: bad memspace");
  const Counts n(ncol, nlay, ngpt, 1);
  Stage st(device, memspace, stream, false);
  if (st.open([&] {
        a.tau = st.in(tau, n.lay_g); a.ssa = st.in(ssa, n.lay_g); a.g = st.in(g, n.lay_g); a.mu0 = st.in(mu0, n.col);
        a.fdir_top = st.in(flux_dir_top, n.col_g); a.inc_dif = st.in(inc_flux_dif, n.col_g);
        a.alb_dir = st.in(sfc_alb_dir, n.col_g); a.alb_dif = st.in(sfc_alb_dif, n.col_g);
        a.flux_up = st.out(gpt_flux_up, n.lev * ngpt); a.flux_dn = st.out(gpt_flux_dn, n.lev * ngpt);
        a.flux_dir = st.out(gpt_flux_dir, n.lev * ngpt);
      }))
    return 1;
  {
    ProfScope prof("sw_gpt", st.stream);
    HIPCHK(ecckd::launch_sw_gpt(a, st.stream));
  }
  return st.close();
}

// ---- two-stream longwave solver (kernels_rte_lw_2str.hip): clouds scatter ----

size_t ecckd_rte_lw_2stream_scratch_bytes(int ncol, int nlay, int ngpt) { return ecckd::rte_lw_2str_scratch_bytes(ncol, nlay, ngpt); }

static int lw_2stream_layers_fit(int nlay) {
  if (sizeof(double) * 2 * ((size_t)nlay + 1) * 16 > (size_t)ecckd::kLdsBudget)
    return fail("ecckd_rte_lw_2stream: too many layers for the level accumulators in LDS (nlay = " + std::to_string(nlay) + ")");
  return 0;
}

// (f32: float arrays behind the double pointers; the same list of refusals in the same order under the call's own name)
static int rte_lw_2stream_impl(bool f32, int device, int ncol, int nlay, int ngpt, int top_at_1, const double *tau, const double *ssa,
                               const double *g, const double *lay_source, const double *lev_source_inc, const double *lev_source_dec,
                               const double *sfc_source, int nband, const int *band2gpt, const double *sfc_emis,
                               const double *inc_flux, double *flux_up, double *flux_dn, int memspace, void *stream) {
  const std::string who = f32 ? "ecckd_rte_lw_2stream_f32" : "ecckd_rte_lw_2stream";
  (void)lay_source;   // an argument as in RTE-RRTMGP's lw_solver_2stream, which never reads it
  if (check_dims(ncol, nlay)) return 1;
  if (!tau || !ssa || !g || !lev_source_inc || !lev_source_dec || !sfc_source || !sfc_emis || !flux_up || !flux_dn)
    return fail(who + ": null argument (only lay_source and inc_flux may be null)");
  LevelPair lp;
  if (level_pair(who.c_str(), lev_source_inc, lev_source_dec, ncol, nlay, f32, memspace, false, &lp)) return 1;
  ecckd::RteLw2strArgs a{};
  if (fill_band_map(ngpt, nband, band2gpt, a.gpt2band)) return 1;
  if (lw_2stream_layers_fit(nlay)) return 1;
  if (memspace == ECCKD_MIXED) return fail(who + ": ECCKD_MIXED is not implemented (ECCKD_DEVICE or ECCKD_HOST)");
  if (memspace != ECCKD_DEVICE && memspace != ECCKD_HOST) return fail("ecckd: bad memspace");
  if (f32 && g_arith.load() != 0) return fail(who + ": needs the fast arithmetic mode (ecckd_set_arithmetic(0))");
  if (check_device(device)) return 1;
  if (ncol == 0) return 0;
  a.ncol = ncol; a.nlay = nlay; a.ng = ngpt; a.top_at_1 = top_at_1 ? 1 : 0; a.nband = nband;
  a.exact_division = g_arith.load() != 0;
  const Counts n(ncol, nlay, ngpt, nband);
  Stage st(device, memspace, stream, f32);
  ScratchLease lease;   // (held until the kernel of this call has been launched)
  void *sp = nullptr;
  // (single precision: the ring is in floats and takes the first half of the block)
  if (stream_scratch(device, st.stream, ecckd::rte_lw_2str_scratch_bytes(ncol, nlay, ngpt), &sp, lease)) return 1;
  a.scratch = static_cast<double *>(sp);
  if (st.open([&] {
        a.tau = st.in(tau, n.lay_g); a.ssa = st.in(ssa, n.lay_g); a.g = st.in(g, n.lay_g);
        a.lev_source_inc = st.in(lev_source_inc, n.lay_g); a.lev_source_dec = st.in(lev_source_dec, n.lay_g);
        a.sfc_source = st.in(sfc_source, n.col_g); a.sfc_emis = st.in(sfc_emis, n.col_b); a.inc_flux = st.in(inc_flux, n.col_g);
        a.flux_up = st.out(flux_up, n.lev); a.flux_dn = st.out(flux_dn, n.lev);
      }))
    return 1;
  {
    ProfScope prof(f32 ? "rte_lw_2stream_f32" : "rte_lw_2stream", st.stream);
    HIPCHK(f32 ? ecckd::launch_rte_lw_2str_f32(a, st.stream) : ecckd::launch_rte_lw_2str(a, st.stream));
  }
  return st.close();
}

int ecckd_rte_lw_2stream(int device, int ncol, int nlay, int ngpt, int top_at_1, const double *tau, const double *ssa,
                         const double *g, const double *lay_source, const double *lev_source_inc, const double *lev_source_dec,
                         const double *sfc_source, int nband, const int *band2gpt, const double *sfc_emis, const double *inc_flux,
                         double *flux_up, double *flux_dn, int memspace, void *stream) {
  return rte_lw_2stream_impl(false, device, ncol, nlay, ngpt, top_at_1, tau, ssa, g, lay_source, lev_source_inc, lev_source_dec,
                             sfc_source, nband, band2gpt, sfc_emis, inc_flux, flux_up, flux_dn, memspace, stream);
}

int ecckd_rte_lw_2stream_f32(int device, int ncol, int nlay, int ngpt, int top_at_1, const float *tau, const float *ssa,
                             const float *g, const float *lay_source, const float *lev_source_inc, const float *lev_source_dec,
                             const float *sfc_source, int nband, const int *band2gpt, const float *sfc_emis, const float *inc_flux,
                             float *flux_up, float *flux_dn, int memspace, void *stream) {
  return rte_lw_2stream_impl(true, device, ncol, nlay, ngpt, top_at_1, dp(tau), dp(ssa), dp(g), dp(lay_source), dp(lev_source_inc),
                             dp(lev_source_dec), dp(sfc_source), nband, band2gpt, dp(sfc_emis), dp(inc_flux), dp(flux_up),
                             dp(flux_dn), memspace, stream);
}

int ecckd_lw_solver_2stream_gpt(int device, int ncol, int nlay, int ngpt, int top_at_1, const double *tau, const double *ssa,
                                const double *g, const double *lay_source, const double *lev_source_inc,
                                const double *lev_source_dec, const double *sfc_emis, const double *sfc_src,
                                const double *inc_flux, double *gpt_flux_up, double *gpt_flux_dn, int memspace, void *stream) {
  (void)lay_source;   // never read, as in RTE-RRTMGP
  if (check_dims(ncol, nlay)) return 1;
  if (ngpt < 1) return fail("ecckd_lw_solver_2stream_gpt: bad ngpt");
  if (!tau || !ssa || !g || !lev_source_inc || !lev_source_dec || !sfc_emis || !sfc_src || !gpt_flux_up || !gpt_flux_dn)
    return fail("ecckd_lw_solver_2stream_gpt: null argument (only lay_source and inc_flux may be null)");
  if (refuse_level_buffer("ecckd_lw_solver_2stream_gpt", lev_source_inc, lev_source_dec, ncol, nlay, memspace)) return 1;
  if (memspace != ECCKD_DEVICE && memspace != ECCKD_HOST) return fail("ecckd: bad memspace");
  if (check_device(device)) return 1;
  if (ncol == 0) return 0;
  ecckd::RteGptArgs a{};
  a.ncol = ncol; a.nlay = nlay; a.ng = ngpt; a.top_at_1 = top_at_1 ? 1 : 0; a.nmus = 1;
  const Counts n(ncol, nlay, ngpt, 1);
  Stage st(device, memspace, stream, false);
  if (st.open([&] {
        a.tau = st.in(tau, n.lay_g); a.ssa = st.in(ssa, n.lay_g); a.g = st.in(g, n.lay_g);
        a.lev_source_inc = st.in(lev_source_inc, n.lay_g); a.lev_source_dec = st.in(lev_source_dec, n.lay_g);
        a.sfc_emis = st.in(sfc_emis, n.col_g); a.sfc_src = st.in(sfc_src, n.col_g); a.inc_flux = st.in(inc_flux, n.col_g);
        a.flux_up = st.out(gpt_flux_up, n.lev * ngpt); a.flux_dn = st.out(gpt_flux_dn, n.lev * ngpt);
      }))
    return 1;
  {
    ProfScope prof("lw_2str_gpt", st.stream);
    HIPCHK(ecckd::launch_lw_2str_gpt(a, st.stream));
  }
  return st.close();
}

int ecckd_sum_broadband(int device, int ncol, int nlev, int ngpt, const double *spectral_flux, double *broadband_flux,
                        int memspace, void *stream) {
  if (ncol < 0 || nlev < 1 || ngpt < 1) return fail("ecckd_sum_broadband: bad dimensions");
  if (!spectral_flux || !broadband_flux) return fail("ecckd_sum_broadband: null argument");
  const size_t n = (size_t)ncol * nlev;
  if (n == 0) return 0;
  if (memspace == ECCKD_HOST) {   // a sum over ngpt planes: not worth a round trip over the bus
    sum_planes_host(spectral_flux, ngpt, n, broadband_flux);
    return 0;
  }
  if (memspace != ECCKD_DEVICE) return fail("ecckd: bad memspace");
  if (check_device(device)) return 1;
  HIPCHK(ecckd::launch_sum_planes(spectral_flux, ngpt, n, broadband_flux, 0, static_cast<hipStream_t>(stream)));
  return 0;
}

// ---- fused longwave: tau-only gas optics + solver that recomputes the Planck sources ----

int ecckd_gas_optics_lw_tau(const ecckd_model_t *m, int ncol, int nlay, const double *plev, const double *tlay, int ngas,
                            const char *gas_names, const double *const *vmr, const long long *vmr_col_stride,
                            const long long *vmr_lay_stride, const double *vmr_scalar, double *tau, int memspace,
                            void *stream) {
  if (check_model(m) || check_gas_optics_dims(ncol, nlay)) return 1;
  if (memspace != ECCKD_DEVICE) return fail("ecckd_gas_optics_lw_tau: device arrays only (ECCKD_DEVICE); ecckd_lw_fluxes takes host arrays");
  if (!plev || !tlay || !tau || (ngas > 0 && !gas_names)) return fail("ecckd_gas_optics_lw_tau: null argument");
  HIPCHK(hipSetDevice(m->device));
  if (ncol == 0) return 0;
  const GasDesc gd{ngas, gas_names, vmr, vmr_col_stride, vmr_lay_stride, vmr_scalar};
  return gas_optical_depth_dev(m, false, nullptr, ncol, nlay, plev, tlay, gd, tau, false, nullptr, nullptr, nullptr, nullptr,
                               static_cast<hipStream_t>(stream));
}

static size_t r32(size_t n) { return (n + 31) & ~(size_t)31; }   // the next multiple of 32 doubles (256 bytes)

// Scratch (in doubles) the fused solver needs besides tau: none at 60 layers (the Planck sources are recomputed inside the
// layer-split solver); any other layer count takes the general route -- Planck kernel into scratch, then the
// register-resident solver with shared level sources -- and needs room for the sources and that solver's ring.
static bool fused_lw_kernels_apply(const ecckd_model *m, int nlay) {
  return nlay == 60 && ecckd::rte_lw_planck_fits(m->ng, m->ntp);   // (a 64-g Planck table does not fit: general route)
}
static size_t fused_scratch_doubles(const ecckd_model *m, int ncol, int nlay) {
  if (fused_lw_kernels_apply(m, nlay)) return 0;
  const size_t n3 = (size_t)ncol * nlay * m->ng;
  return 3 * n3 + (size_t)ncol * m->ng + 32 + ecckd::rte_lw_scratch_bytes(ncol, nlay, m->ng) / sizeof(double);
}

// ---- a fused flux call is Columns + Particles + outputs ----
// An entry point fills these structs from its own parameters, once (the _f32 ones through dp(): float data behind the double
// pointers), and everything below it takes the structs.  Each has one member that declares its arrays to a Stage and
// returns the image the kernels read: the only place those declarations stand, so their order is the same in every call.

// The atmosphere and the boundary conditions of a longwave call, in the memory space of the call
struct LwColumns {
  int ncol, nlay;
  const double *plev, *tlay, *tsfc, *tlev;
  GasDesc gas;
  int top_at_1, n_gauss_angles;
  const double *sfc_emis, *inc_flux;
  LwColumns staged(Stage &st, const Counts &n) const {
    LwColumns d = *this;
    d.plev = st.in(plev, n.lev); d.tlay = st.in(tlay, n.lay); d.tsfc = st.in(tsfc, n.col); d.tlev = st.in(tlev, n.lev);
    d.sfc_emis = st.in(sfc_emis, n.col_b); d.inc_flux = st.in(inc_flux, n.col_g);
    d.gas = st.gases(gas, ncol, nlay);
    return d;
  }
  bool null_array() const { return !plev || !tlay || !tsfc || !sfc_emis || (gas.ngas > 0 && !gas.names); }
};

// ... of a shortwave call
struct SwColumns {
  int ncol, nlay;
  const double *plev, *tlay;
  GasDesc gas;
  int top_at_1;
  const double *mu0, *toa_scale, *sfc_alb_dir, *sfc_alb_dif;
  SwColumns staged(Stage &st, const Counts &n) const {
    SwColumns d = *this;
    d.plev = st.in(plev, n.lev); d.tlay = st.in(tlay, n.lay); d.mu0 = st.in(mu0, n.col); d.toa_scale = st.in(toa_scale, n.col);
    d.sfc_alb_dir = st.in(sfc_alb_dir, n.col_b); d.sfc_alb_dif = st.in(sfc_alb_dif, n.col_b);
    d.gas = st.gases(gas, ncol, nlay);
    return d;
  }
  bool null_array() const { return !plev || !tlay || !mu0 || !sfc_alb_dir || !sfc_alb_dif || (gas.ngas > 0 && !gas.names); }
};

// The combined particulate optical properties on the model's bands, (ncol,nlay,nband) each, in the memory space of the call;
// tau == nullptr: no particles.  Longwave: ssa == nullptr: one-stream particles; g: the scattering solvers only.
// mask: the McICA cloud mask (ncol,nlay), or null.  scaling: ecckd_*_flux_scaled -- the sampled optical-depth scaling
// (ncol,nlay,ngpt), float32, or null; in the longwave the scaled by-band increment then runs on the scratch tau at every
// layer count and the solver sees no particles.
static const char kMaskTooWide[] = ": a cloud mask is one 64-bit word per (column, layer): at most 64 g-points, not ";
struct LwParticles {
  const double *tau = nullptr, *ssa = nullptr, *g = nullptr;
  const unsigned long long *mask = nullptr;
  const float *scaling = nullptr;
  LwParticles staged(Stage &st, const Counts &n) const {
    LwParticles d;
    d.tau = st.in(tau, n.lay_b); d.ssa = st.in(ssa, n.lay_b); d.g = st.in(g, n.lay_b);
    d.mask = st.in(mask, n.lay);
    d.scaling = static_cast<const float *>(st.in_bytes(scaling, n.lay_g * sizeof(float)));
    return d;
  }
};
// Shortwave: delta_scale: the library delta-scales a copy (f = g*g) first
struct SwParticles {
  const double *tau = nullptr, *ssa = nullptr, *g = nullptr;
  int delta_scale = 0;
  const unsigned long long *mask = nullptr;
  const float *scaling = nullptr;
  SwParticles staged(Stage &st, const Counts &n) const {
    SwParticles d;
    d.tau = st.in(tau, n.lay_b); d.ssa = st.in(ssa, n.lay_b); d.g = st.in(g, n.lay_b);
    d.delta_scale = delta_scale;
    d.mask = st.in(mask, n.lay);
    d.scaling = static_cast<const float *>(st.in_bytes(scaling, n.lay_g * sizeof(float)));
    return d;
  }
};

// One set of fluxes, (ncol,nlay+1) each -- (ncol,nlay+1,nband) for the band planes -- in the memory space of the call;
// dir: shortwave only, may be null
struct Fluxes {
  double *up = nullptr, *dn = nullptr, *dir = nullptr;
  Fluxes staged(Stage &st, size_t n) const { return Fluxes{st.out(up, n), st.out(dn, n), st.out(dir, n)}; }
};
// What a fused call delivers: the fluxes of the sky it computes, and -- each only where the call has it and the caller
// names it -- the clear-sky fluxes next to them, the band planes, flux_up_jac
struct FluxOutputs {
  Fluxes all, clear, bands;
  double *jac = nullptr;
};

// first[b] = first 0-based g-point of band b, first[nband] = ngpt; the bands must tile 1..ngpt in ascending order
static int band_windows(const ecckd_model *m, const char *who, unsigned short *first) {
  int next = 1;
  for (int b = 0; b < m->nband; ++b) {
    if (m->band2gpt[2 * b] != next || m->band2gpt[2 * b + 1] < next)
      return fail(std::string(who) + ": the model's band2gpt does not tile 1..ngpt in ascending order");
    first[b] = (unsigned short)(next - 1);
    next = m->band2gpt[2 * b + 1] + 1;
  }
  if (next != m->ng + 1) return fail(std::string(who) + ": the model's band2gpt does not tile 1..ngpt in ascending order");
  first[m->nband] = (unsigned short)m->ng;
  return 0;
}

static int outputs_alias(const char *who, std::initializer_list<const double *> outs) {
  for (auto p = outs.begin(); p != outs.end(); ++p)
    for (auto q = p + 1; q != outs.end(); ++q)
      if (*p && *p == *q) return fail(std::string(who) + ": two outputs are the same array (each needs an array of its own)");
  return 0;
}

// a clear-sky output that is an all-sky output as well
static bool clear_aliases_all(const Fluxes &clear, const Fluxes &all) {
  for (double *c : {clear.up, clear.dn, clear.dir})
    for (double *f : {all.up, all.dn, all.dir})
      if (c && c == f) return true;
  return false;
}

// ---- what a fused call refuses ----
// The words of a call in the refusals that the calls share: data only.  The shared lists below are short and linear; an
// implementation calls them in its order, with its own checks in between, and ends with one of the three tails
// (lw_plain_tail / sw_plain_tail, on_device, bands_tail).  What needs no device comes before check_model, so that a
// host-only model answers it too.
struct CallWords {
  const char *who = nullptr;             // the call's name in the messages of its list
  const char *who_mask = nullptr;        // ... where it refuses a mask on more than 64 g-points
  const char *planes_tail = nullptr;     // behind `who` where a required plane is missing; null: the call names no particles
  bool need_ssa_g = true;                // tau_p, ssa_p and g_p are required (longwave one-stream calls: tau_p alone)
  bool nband0_clear = false;             // nband_p = 0 is the clear sky: no plane and no mask then
  const char *no_particles_tail = nullptr;   // tau_p NULL is the clear sky: behind `who` where something of the particles' is named then
  const char *who_clear = nullptr, *clear_tail = nullptr;   // the name and the words where flux_up_clear or flux_dn_clear is missing
  bool clear_required = false;           // the clear-sky outputs are part of the call (else: named by giving one)
  const char *tlev_text = "tlev is required for ecckd";
};

static int refuse(const char *who, const char *tail) { return fail(std::string(who) + tail); }

// null model, a mask on more than 64 g-points, nband_p, the planes (`ssa` / `g`: as the call requires them)
static int particles_refusals(const CallWords &w, const ecckd_model *m, int nband_p, const double *tau, const double *ssa,
                              const double *g, const unsigned long long *mask) {
  if (!m) return fail("ecckd: null model");
  if (mask && m->ng > 64) return fail(w.who_mask + std::string(kMaskTooWide) + std::to_string(m->ng));
  const bool clear_sky = w.nband0_clear && nband_p == 0;
  if (nband_p != m->nband && !clear_sky)
    return fail(std::string(w.who) + ": nband_p = " + std::to_string(nband_p) + " but the model has " + std::to_string(m->nband) +
                " bands (particulate properties live on the model's bands" + (w.nband0_clear ? "; 0: clear sky)" : ")"));
  if (!clear_sky && (!tau || (w.need_ssa_g && (!ssa || !g)))) return refuse(w.who, w.planes_tail);
  if (clear_sky && (tau || ssa || g || mask))
    return refuse(w.who, ": nband_p = 0 is the clear sky: the particulate planes and cloud_mask must be null");
  return 0;
}

// the clear-sky outputs: both or (where the call allows that) neither, and none of them an all-sky output
static int clear_refusals(const CallWords &w, const FluxOutputs &o) {
  if (!w.clear_required && !o.clear.up && !o.clear.dn && !o.clear.dir) return 0;
  if (!o.clear.up || !o.clear.dn) return refuse(w.who_clear, w.clear_tail);
  if (clear_aliases_all(o.clear, o.all))
    return refuse(w.who_clear, ": a clear-sky output must not be an all-sky output (the two sets of fluxes need arrays of their own)");
  return 0;
}

static int jac_refusals(const char *who_jac, const FluxOutputs &o, bool with_clear = true) {
  if (o.jac && (o.jac == o.all.up || o.jac == o.all.dn || (with_clear && (o.jac == o.clear.up || o.jac == o.clear.dn))))
    return refuse(who_jac, ": flux_up_jac must not be another output (it needs an array of its own)");
  return 0;
}

static int gauss_refusals(const LwColumns &c, const char *lead = "rte_lw") {
  if (c.n_gauss_angles >= 1 && c.n_gauss_angles <= 4) return 0;
  return refuse(lead, ": have to ask for at least one quadrature point and no more than 4");
}

// The head of every longwave list that names particles: particles, arithmetic mode, Planck table, tlev
static int lw_head(const CallWords &w, const ecckd_model *m, const LwColumns &c, int nband_p, const LwParticles &pt) {
  if (particles_refusals(w, m, nband_p, pt.tau, pt.ssa, pt.g, pt.mask)) return 1;
  if (g_arith.load() != 0) return refuse(w.who, ": needs the fast arithmetic mode (ecckd_set_arithmetic(0))");
  if (!m->has_planck) return refuse(w.who, ": model has no Planck table (shortwave model?)");
  if (!c.tlev) return fail(w.tlev_text);
  return 0;
}

// ... of every shortwave list that names particles: particles (tau_p NULL: the clear sky, where the call has that),
// delta_scale, arithmetic mode
static int sw_head(const CallWords &w, const ecckd_model *m, int nband_p, const SwParticles &pt, const FluxOutputs &o) {
  if (w.no_particles_tail && !pt.tau) {
    if (!m) return fail("ecckd: null model");
    if (pt.mask && m->ng > 64) return fail(w.who_mask + std::string(kMaskTooWide) + std::to_string(m->ng));
    if (pt.ssa || pt.g || pt.mask || o.clear.up || o.clear.dn || o.clear.dir) return refuse(w.who, w.no_particles_tail);
  } else {
    if (particles_refusals(w, m, nband_p, pt.tau, pt.ssa, pt.g, pt.mask)) return 1;
    if (pt.delta_scale != 0 && pt.delta_scale != 1) return refuse(w.who, ": delta_scale must be 0 or 1");
  }
  if (g_arith.load() != 0) return refuse(w.who, ": needs the fast arithmetic mode (ecckd_set_arithmetic(0))");
  return 0;
}

// Tail: behind check_model, the dimensions and the call's null arrays -- memory space, device, and *done where the call
// has no columns and returns 0
static int on_device(const ecckd_model *m, int ncol, int memspace, bool *done) {
  if (memspace != ECCKD_DEVICE && memspace != ECCKD_HOST) return fail("ecckd: bad memspace");
  HIPCHK(hipSetDevice(m->device));
  *done = ncol == 0;
  return 0;
}

// Tail of ecckd_{lw,sw}_flux_bands, which put their name in front of every message: memory space, the model, the
// dimensions, null arrays, the band windows into `first`
static int bands_tail(const char *who, const ecckd_model *m, int ncol, int nlay, bool null_array, int memspace,
                      unsigned short *first, bool *done) {
  if (memspace != ECCKD_DEVICE && memspace != ECCKD_HOST) return refuse(who, ": bad memspace (ECCKD_DEVICE or ECCKD_HOST)");
  if (!m->finalized) return refuse(who, ": model is not finalized");
  if (m->device < 0) return refuse(who, ": host-only model (device -1): no GPU, no compute (there is no CPU fallback)");
  if (check_gas_optics_dims(ncol, nlay)) return 1;
  if (null_array) return refuse(who, ": null argument");
  if (band_windows(m, who, first)) return 1;
  HIPCHK(hipSetDevice(m->device));
  *done = ncol == 0;
  return 0;
}

// Tail: the list of ecckd_lw_fluxes, which the all-sky forms on its solver run through behind their own (a call without
// columns returns before the memory space is looked at).  Without tau_p nothing of the particles' may be named
// (ecckd_lw_fluxes_jac).
static int lw_plain_tail(const ecckd_model *m, const LwColumns &c, int nband_p, const LwParticles &pt, const FluxOutputs &o,
                         int memspace, bool *done) {
  if (check_model(m) || check_gas_optics_dims(c.ncol, c.nlay)) return 1;
  if (!m->has_planck) return fail("ecckd_lw_fluxes: model has no Planck table (shortwave model?)");
  if (gauss_refusals(c)) return 1;
  if (c.null_array() || !o.all.up || !o.all.dn) return fail("ecckd_lw_fluxes: null argument");
  if (!c.tlev) return fail("tlev is required for ecckd");
  if (g_arith.load() != 0) return fail("ecckd_lw_fluxes: needs the fast arithmetic mode (ecckd_set_arithmetic(0))");
  if (jac_refusals("ecckd_lw_fluxes_jac", o, false)) return 1;
  if (!pt.tau && (nband_p != 0 || pt.ssa || pt.mask || o.clear.up || o.clear.dn))
    return fail("ecckd_lw_fluxes_jac: nband_p, cloud_mask and the clear-sky outputs belong to particles: without tau_p they must be 0 / null");
  HIPCHK(hipSetDevice(m->device));
  *done = c.ncol == 0;
  if (!*done && memspace != ECCKD_DEVICE && memspace != ECCKD_HOST) return fail("ecckd: bad memspace");
  return 0;
}

// ... and that of ecckd_sw_fluxes
static int sw_plain_tail(const ecckd_model *m, const SwColumns &c, const FluxOutputs &o, int memspace, bool *done) {
  if (check_model(m) || check_gas_optics_dims(c.ncol, c.nlay)) return 1;
  if (!m->has_solar) return fail("ecckd_sw_fluxes: model has no solar table (longwave model?)");
  if (c.null_array() || !o.all.up || !o.all.dn) return fail("ecckd_sw_fluxes: null argument");
  if (g_arith.load() != 0) return fail("ecckd_sw_fluxes: needs the fast arithmetic mode (ecckd_set_arithmetic(0))");
  HIPCHK(hipSetDevice(m->device));
  *done = c.ncol == 0;
  if (!*done && memspace != ECCKD_DEVICE && memspace != ECCKD_HOST) return fail("ecckd: bad memspace");
  return 0;
}

// The kernel arguments every longwave solver launch of a model starts from (`c`: staged)
static int lw_solver_args(const ecckd_model *m, const LwColumns &c, bool f32, ecckd::RteLwArgs &a) {
  if (fill_band_map(m->ng, m->nband, m->band2gpt.data(), a.gpt2band)) return 1;
  a.ncol = c.ncol; a.nlay = c.nlay; a.ng = m->ng; a.top_at_1 = c.top_at_1 ? 1 : 0; a.nband = m->nband;
  a.f32 = f32 ? 1 : 0;
  fill_lw_options(a, c.n_gauss_angles, f32);
  a.sfc_emis = c.sfc_emis; a.inc_flux = c.inc_flux;
  return 0;
}

// `both` (60-layer route with `pt` only): the dual-sky kernel, clear-sky fluxes to *both and all-sky fluxes to `to`
// `pt` (60-layer route only): the band planes the solver adds to tau as it reads it; the general route gets a tau that
// launch_increment has incremented already
// `jac_inline` (60-layer route, without `both`): the Jacobian form of the kernel, which stores flux_up_jac there as well
// `sources` (general route only; ecckd_lw_fluxes_rescaled_jac): the Planck sources are there already, wherever the caller
// keeps them, and `scratch` is the solver's ring alone
static int rte_lw_fused_dev(const ecckd_model *m, const LwColumns &c, const double *tau, const Fluxes &to, double *scratch,
                            hipStream_t stream, const LwParticles *pt = nullptr, const Fluxes *both = nullptr,
                            bool sources_in_scratch = false, double *jac_inline = nullptr, const PlanckSide *sources = nullptr) {
  const int ncol = c.ncol, nlay = c.nlay;
  ecckd::RteLwArgs a{};
  if (lw_solver_args(m, c, false, a)) return 1;
  a.use_split = 1;
  a.tau = tau; a.flux_up = to.up; a.flux_dn = to.dn;
  if (fused_lw_kernels_apply(m, nlay)) {
    if (pt) { a.part_tau = pt->tau; a.part_ssa = pt->ssa; a.part_1scl = pt->ssa ? 0 : 1; a.part_mask = pt->mask; }
    ProfScope prof("rte_lw_fused", stream);
    HIPCHK(ecckd::launch_rte_lw_planck(a, m->dbuf + m->off_planck, m->ntp, m->temperature_planck[0],
                                       m->temperature_planck[1] - m->temperature_planck[0], c.tlay, c.tlev, c.tsfc, stream,
                                       both ? both->up : nullptr, both ? both->dn : nullptr, jac_inline));
    return 0;
  }
  if (both || jac_inline) return fail("ecckd: internal: the dual-sky and the Jacobian longwave kernels serve 60 layers only");
  // general route (any layer count): sources through scratch, one value per level
  if (!scratch && !(sources && !ecckd::rte_lw_scratch_bytes(ncol, nlay, m->ng)))
    return fail("ecckd: internal: the fused longwave solver needs scratch for this layer count");
  const size_t n3 = (size_t)ncol * nlay * m->ng;
  double *lay, *inc, *dec, *sfc, *ring;
  if (sources) {
    lay = sources->lay_source; inc = sources->lev_inc; dec = sources->lev_dec; sfc = sources->sfc_source; ring = scratch;
  } else {
    lay = scratch; inc = lay + n3; dec = inc + n3; sfc = dec + n3; ring = sfc + (((size_t)ncol * m->ng + 31) & ~(size_t)31);
  }
  if (!sources && !sources_in_scratch) {   // (the all-sky pass of ecckd_lw_fluxes_clear_allsky finds the clear pass's sources there)
    ecckd::PlanckArgs p = planck_args(m, ncol, nlay, c.tlay, PlanckSide{c.tlev, c.tsfc, lay, inc, dec, sfc});
    ProfScope prof("planck", stream);
    HIPCHK(ecckd::launch_planck(p, stream));
  }
  a.lay_source = lay; a.lev_source_inc = inc; a.lev_source_dec = dec; a.sfc_source = sfc;
  a.shared_levels = c.inc_flux ? 0 : 1;
  a.use_split = 0;
  a.scratch = ecckd::rte_lw_scratch_bytes(ncol, nlay, m->ng) ? ring : nullptr;
  ProfScope prof("rte_lw", stream);
  HIPCHK(ecckd::launch_rte_lw(a, stream));
  return 0;
}

int ecckd_rte_lw_fused(const ecckd_model_t *m, int ncol, int nlay, int top_at_1, int n_gauss_angles, const double *tau,
                       const double *tlay, const double *tlev, const double *tsfc, const double *sfc_emis,
                       const double *inc_flux, double *flux_up, double *flux_dn, int memspace, void *stream) {
  if (check_model(m) || check_dims(ncol, nlay)) return 1;
  if (!m->has_planck) return fail("ecckd_rte_lw_fused: model has no Planck table (shortwave model?)");
  if (memspace != ECCKD_DEVICE) return fail("ecckd_rte_lw_fused: device arrays only (ECCKD_DEVICE); ecckd_lw_fluxes takes host arrays");
  if (n_gauss_angles < 1 || n_gauss_angles > 4) return fail("rte_lw: have to ask for at least one quadrature point and no more than 4");
  if (!tau || !tlay || !tsfc || !sfc_emis || !flux_up || !flux_dn) return fail("ecckd_rte_lw_fused: null argument");
  if (!tlev) return fail("tlev is required for ecckd");
  HIPCHK(hipSetDevice(m->device));
  if (ncol == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  void *sp = nullptr;
  ScratchLease lease;
  const size_t extra = fused_scratch_doubles(m, ncol, nlay);
  if (extra && stream_scratch(m->device, st, extra * sizeof(double), &sp, lease)) return 1;
  const LwColumns c{ncol, nlay, nullptr, tlay, tsfc, tlev, GasDesc{}, top_at_1, n_gauss_angles, sfc_emis, inc_flux};
  return rte_lw_fused_dev(m, c, tau, Fluxes{flux_up, flux_dn}, static_cast<double *>(sp), st);
}

// General route of the all-sky call (any layer count): tau += the particles' (absorption) optical depth by band, the
// one-stream-op1 increment kernel of ecckd_increment on the scratch tau between gas optics and the solver
// (ssa1 / g1: ecckd_lw_fluxes_allsky_rescaled -- the two-stream increment on (tau, ssa1, g1) with the band triple)
static int lw_increment_dev(const ecckd_model *m, int ncol, int nlay, double *tau, const LwParticles &pt, hipStream_t stream,
                            double *ssa1 = nullptr, double *g1 = nullptr) {
  ecckd::OptPropsArgs o{};
  o.ncol = ncol; o.nlay = nlay; o.ng = m->ng; o.nband = m->nband; o.f32 = 0;
  // the increment kernel wants bands in ascending order that tile 1..ngpt, as ecckd_increment checks
  if (band_windows(m, "ecckd_lw_fluxes_allsky", o.band_first)) return 1;
  o.tau1 = tau; o.tau2 = pt.tau; o.ssa2 = pt.ssa; o.g2 = pt.ssa;   // (g2 marks op2 as two-stream; 1scl += 2str never reads it)
  if (ssa1) { o.ssa1 = ssa1; o.g1 = g1; o.g2 = pt.g; }
  o.mask = pt.mask;   // (McICA: the masked by-band increment)
  o.scaling = pt.scaling;
  ProfScope prof("increment", stream);
  HIPCHK(ecckd::launch_increment(o, stream));
  return 0;
}

// ecckd_lw_fluxes_clear_allsky behind the gas optics: both skies from the one scratch tau.  60 layers: the clear-sky and the
// all-sky kernel one after the other, or the dual-sky kernel ("lw_both_skies").  Any other layer count: Planck sources into
// scratch once, the clear pass, the by-band increment in place, the solver again -- the clear pass has to see tau before
// the increment.
static int lw_both_skies_dev(const ecckd_model *m, const LwColumns &c, double *tau, const LwParticles &pt, const FluxOutputs &o,
                             double *scratch, hipStream_t stream, double *jac_inline = nullptr) {
  const bool fused = fused_lw_kernels_apply(m, c.nlay);
  // (jac_inline: the dual-sky kernel has no Jacobian form -- two launches, the all-sky one the Jacobian kernel; same fluxes)
  if (fused && g_opt.lw_both_skies.load() == 1 && !jac_inline) return rte_lw_fused_dev(m, c, tau, o.all, scratch, stream, &pt, &o.clear);
  if (rte_lw_fused_dev(m, c, tau, o.clear, scratch, stream)) return 1;
  if (!fused && lw_increment_dev(m, c.ncol, c.nlay, tau, pt, stream)) return 1;
  return rte_lw_fused_dev(m, c, tau, o.all, scratch, stream, &pt, nullptr, !fused, jac_inline);
}

// flux_up_jac behind the flux pass(es) of a fused call, from the scratch tau: the stand-alone Jacobian kernel with the
// surface term formed from tsfc and the Planck table.  On the 60-layer route the flux kernel has added the particles as it
// read tau, so the Jacobian kernel does the same (`pt`); on the general route tau was incremented in place.
static int lw_jac_dev(const ecckd_model *m, const LwColumns &c, const double *tau, const LwParticles *pt, double *jac,
                      hipStream_t stream) {
  ecckd::RteLwJacArgs j{};
  if (fill_band_map(m->ng, m->nband, m->band2gpt.data(), j.gpt2band)) return 1;
  fill_jac_args(j, c.ncol, c.nlay, m->ng, c.top_at_1, c.n_gauss_angles, m->nband);
  j.tau = tau; j.tsfc = c.tsfc; j.sfc_emis = c.sfc_emis; j.flux_up_jac = jac;
  if (pt && fused_lw_kernels_apply(m, c.nlay)) { j.part_tau = pt->tau; j.part_ssa = pt->ssa; j.part_mask = pt->mask; }
  ProfScope prof("rte_lw_jac", stream);
  HIPCHK(ecckd::launch_rte_lw_jac(j, m->dbuf + m->off_planck, m->ntp, m->temperature_planck[0],
                                  m->temperature_planck[1] - m->temperature_planck[0], stream));
  return 0;
}

// The work block of the single-precision fused longwave calls (ecckd_lw_fluxes_f32_scratch_bytes,
// ecckd_lw_fluxes_allsky_2stream_f32_scratch_bytes), in this order: tau, lay_source, lev_source_inc, lev_source_dec (`cells`
// bytes each: what the single-precision gas optics writes), sfc_source (`sfc`), the solver's ring (`ring_bytes`: that of the
// overflow solver beyond 96 layers, else nothing; the two-stream solver's in floats); every part a multiple of 256 bytes.
// The partial sums of the tail split follow when the block has room for them.
struct LwWorkF32 {
  size_t cells, sfc, ring;
  LwWorkF32(const ecckd_model *m, int ncol, int nlay, size_t ring_bytes) {
    const Counts n(ncol, nlay, m->ng, m->nband);
    cells = align256(n.lay_g * sizeof(float));
    sfc = align256(n.col_g * sizeof(float));
    ring = align256(ring_bytes);
  }
  size_t bytes() const { return 4 * cells + sfc + ring; }
  double *at(double *work, size_t off) const { return reinterpret_cast<double *>(reinterpret_cast<char *>(work) + off); }
  double *tau(double *work) const { return work; }
  PlanckSide sources(double *work, const LwColumns &c) const {
    return PlanckSide{c.tlev, c.tsfc, at(work, cells), at(work, 2 * cells), at(work, 3 * cells), at(work, 4 * cells)};
  }
  double *ring_at(double *work) const { return at(work, 4 * cells + sfc); }
};
static LwWorkF32 lw_work_f32(const ecckd_model *m, int ncol, int nlay) {
  return LwWorkF32(m, ncol, nlay, ecckd::rte_lw_scratch_bytes(ncol, nlay, m->ng));
}
static LwWorkF32 lw_2stream_work_f32(const ecckd_model *m, int ncol, int nlay) {
  return LwWorkF32(m, ncol, nlay, ecckd::rte_lw_2str_scratch_bytes(ncol, nlay, m->ng) / 2);
}

// ecckd_lw_fluxes_f32 and its all-sky forms behind the refusal list: the single-precision gas optics writes tau and the
// Planck sources (two separate level arrays) into the work block, the single-precision register-resident solver follows on
// them at every layer count -- launch_rte_lw (clear sky), launch_rte_lw_allsky_f32 (particles: added where the solver
// consumes tau), or one after the other on the same arrays (clear-sky outputs).  What ecckd_gas_optics_lw_f32 [+
// ecckd_increment(_masked)_f32] + ecckd_rte_lw(_inc_flux)_f32 compute, bit for bit.
static int lw_fluxes_f32_run(const ecckd_model *m, const LwColumns &c, const LwParticles &pt, const FluxOutputs &o, int memspace,
                             void *stream) {
  const int ncol = c.ncol, nlay = c.nlay;
  const Counts n(ncol, nlay, m->ng, m->nband);
  const LwWorkF32 w = lw_work_f32(m, ncol, nlay);
  long tail_first = -1;
  size_t tail = 0;   // tail tiles one g-pair per wave (rte_lw_tail_plan); optional, same bits
  ecckd::RteLwArgs a{};
  if (lw_solver_args(m, c, true, a)) return 1;
  if (!w.ring && g_opt.lw_tail_split.load()) tail = ecckd::rte_lw_tail_plan(a, simd_slots(m->device), &tail_first);
  Stage st(const_cast<ecckd_model *>(m), memspace, stream, true);
  LwColumns d{};
  LwParticles d_pt{};
  FluxOutputs d_o{};
  double *d_work = nullptr;
  bool got_tail = false;
  if (st.open([&] {
        d = c.staged(st, n);
        d_pt = pt.staged(st, n);
        d_o.clear = o.clear.staged(st, n.lev);
        d_o.all = o.all.staged(st, n.lev);
        d_work = st.work(w.bytes(), tail, &got_tail);
      }))
    return 1;
  a.sfc_emis = d.sfc_emis; a.inc_flux = d.inc_flux;   // (the staged ones)
  const PlanckSide src = w.sources(d_work, d);
  const hipStream_t s = st.stream;
  if (gas_optics_lw_dev(m, true, ncol, nlay, d.plev, d.tlay, d.gas, w.tau(d_work), src, s)) return 1;
  a.tau = w.tau(d_work); a.lay_source = src.lay_source; a.lev_source_inc = src.lev_inc; a.lev_source_dec = src.lev_dec;
  a.sfc_source = src.sfc_source;
  if (w.ring) a.scratch = w.ring_at(d_work);
  if (tail && got_tail) { a.partials = w.at(d_work, w.bytes()); a.tail_first = tail_first; }
  if (d_o.clear.up) {
    a.flux_up = d_o.clear.up; a.flux_dn = d_o.clear.dn;
    ProfScope prof("rte_lw", s);
    HIPCHK(ecckd::launch_rte_lw(a, s));
  }
  a.flux_up = d_o.all.up; a.flux_dn = d_o.all.dn;
  if (d_pt.tau) {
    a.part_tau = d_pt.tau; a.part_ssa = d_pt.ssa; a.part_1scl = d_pt.ssa ? 0 : 1; a.part_mask = d_pt.mask;
    ProfScope prof("rte_lw_allsky_f32", s);
    HIPCHK(ecckd::launch_rte_lw_allsky_f32(a, s));
  } else {
    ProfScope prof("rte_lw", s);
    HIPCHK(ecckd::launch_rte_lw(a, s));
  }
  return st.close();
}

// The fused longwave calls on the no-scattering solver: gas optical depth into the work block, then the solver pass(es) the
// call's particles and outputs ask for
// (`w`: the words of an all-sky form, whose list goes first; null: ecckd_lw_fluxes, and ecckd_lw_fluxes_jac without tau_p)
static int lw_fluxes_impl(const CallWords *w, bool f32, const ecckd_model_t *m, const LwColumns &c, int nband_p, const LwParticles &pt,
                          const FluxOutputs &o, int memspace, void *stream) {
  bool done;
  if (w && (lw_head(*w, m, c, nband_p, pt) || clear_refusals(*w, o) || jac_refusals("ecckd_lw_fluxes_jac", o))) return 1;
  if (lw_plain_tail(m, c, nband_p, pt, o, memspace, &done)) return 1;
  if (done) return 0;
  if (f32) {   // (the _f32 entry points: no Jacobian form)
    if (o.jac) return fail("ecckd: internal: the single-precision fused longwave calls have no Jacobian form");
    return lw_fluxes_f32_run(m, c, pt, o, memspace, stream);
  }
  const int ncol = c.ncol, nlay = c.nlay;
  const Counts n(ncol, nlay, m->ng, m->nband);
  const bool part = pt.tau != nullptr, both = o.clear.up != nullptr;
  // the Jacobian inside the 60-layer flux kernel ("lw_jac_inline" = 1), or from the stand-alone kernel behind the flux pass
  const bool jac_in = o.jac && fused_lw_kernels_apply(m, nlay) && g_opt.lw_jac_inline.load() == 1;
  // tau lives in the work block between the kernels; behind it what the general route needs (fused_scratch_doubles)
  const size_t extra = fused_scratch_doubles(m, ncol, nlay);
  Stage st(const_cast<ecckd_model *>(m), memspace, stream, false);
  LwColumns d{};
  LwParticles d_pt{};
  FluxOutputs d_o{};
  double *d_tau = nullptr;
  if (st.open([&] {
        d = c.staged(st, n);
        d_pt = pt.staged(st, n);
        d_o.clear = o.clear.staged(st, n.lev);
        d_o.all = o.all.staged(st, n.lev);
        d_o.jac = st.out(o.jac, n.lev);
        d_tau = st.work((n.lay_g + 32 + extra) * sizeof(double));
      }))
    return 1;
  double *d_extra = extra ? d_tau + r32(n.lay_g) : nullptr;
  const hipStream_t s = st.stream;
  if (gas_optical_depth_dev(m, false, nullptr, ncol, nlay, d.plev, d.tlay, d.gas, d_tau, false, nullptr, nullptr, nullptr, nullptr, s)) return 1;
  if (pt.scaling) {   // ecckd_lw_flux_scaled: the scaled increment in place, then the solver without particles
    if (both || o.jac) return fail("ecckd: internal: the scaled longwave call has no both-skies or Jacobian form");
    if (lw_increment_dev(m, ncol, nlay, d_tau, d_pt, s)) return 1;
    if (rte_lw_fused_dev(m, d, d_tau, d_o.all, d_extra, s)) return 1;
  } else if (both) {
    if (lw_both_skies_dev(m, d, d_tau, d_pt, d_o, d_extra, s, jac_in ? d_o.jac : nullptr)) return 1;
  } else {
    if (part && !fused_lw_kernels_apply(m, nlay) && lw_increment_dev(m, ncol, nlay, d_tau, d_pt, s)) return 1;
    if (rte_lw_fused_dev(m, d, d_tau, d_o.all, d_extra, s, part ? &d_pt : nullptr, nullptr, false, jac_in ? d_o.jac : nullptr)) return 1;
  }
  // (both skies, general route: behind the second solver pass, on the tau that pass saw)
  if (o.jac && !jac_in && lw_jac_dev(m, d, d_tau, part ? &d_pt : nullptr, d_o.jac, s)) return 1;
  return st.close();
}

// the words of the all-sky forms on the no-scattering solver (clear_required: the clear-sky outputs are part of the call)
static CallWords lw_allsky_words(bool clear_required = false) {
  CallWords w;
  w.who = "ecckd_lw_fluxes_allsky";
  w.who_mask = "ecckd_lw_fluxes_allsky_mcica";
  w.planes_tail = ": null argument (tau_p is required; ssa_p may be null: one-stream particles)";
  w.need_ssa_g = false;
  w.who_clear = "ecckd_lw_fluxes_clear_allsky";
  w.clear_tail = ": null argument (flux_up_clear and flux_dn_clear are both required)";
  w.clear_required = clear_required;
  return w;
}
static const CallWords kLwAllsky = lw_allsky_words(), kLwClearAllsky = lw_allsky_words(true);

int ecckd_lw_fluxes(const ecckd_model_t *m, int ncol, int nlay, const double *plev, const double *tlay, const double *tsfc,
                    const double *tlev, int ngas, const char *gas_names, const double *const *vmr,
                    const long long *vmr_col_stride, const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1,
                    int n_gauss_angles, const double *sfc_emis, const double *inc_flux, double *flux_up, double *flux_dn,
                    int memspace, void *stream) {
  const LwColumns c{ncol, nlay, plev, tlay, tsfc, tlev, GasDesc{ngas, gas_names, vmr, vmr_col_stride, vmr_lay_stride, vmr_scalar},
                    top_at_1, n_gauss_angles, sfc_emis, inc_flux};
  const FluxOutputs o{Fluxes{flux_up, flux_dn}};
  return lw_fluxes_impl(nullptr, false, m, c, 0, LwParticles{}, o, memspace, stream);
}

int ecckd_lw_fluxes_clear_allsky(const ecckd_model_t *m, int ncol, int nlay, const double *plev, const double *tlay,
                                 const double *tsfc, const double *tlev, int ngas, const char *gas_names,
                                 const double *const *vmr, const long long *vmr_col_stride, const long long *vmr_lay_stride,
                                 const double *vmr_scalar, int top_at_1, int n_gauss_angles, const double *sfc_emis,
                                 const double *inc_flux, int nband_p, const double *tau_p, const double *ssa_p,
                                 const unsigned long long *cloud_mask, double *flux_up, double *flux_dn, double *flux_up_clear,
                                 double *flux_dn_clear, int memspace, void *stream) {
  const LwColumns c{ncol, nlay, plev, tlay, tsfc, tlev, GasDesc{ngas, gas_names, vmr, vmr_col_stride, vmr_lay_stride, vmr_scalar},
                    top_at_1, n_gauss_angles, sfc_emis, inc_flux};
  return lw_fluxes_impl(&kLwClearAllsky, false, m, c, nband_p, LwParticles{tau_p, ssa_p, nullptr, cloud_mask},
                        FluxOutputs{Fluxes{flux_up, flux_dn}, Fluxes{flux_up_clear, flux_dn_clear}}, memspace, stream);
}

int ecckd_lw_fluxes_allsky(const ecckd_model_t *m, int ncol, int nlay, const double *plev, const double *tlay, const double *tsfc,
                           const double *tlev, int ngas, const char *gas_names, const double *const *vmr,
                           const long long *vmr_col_stride, const long long *vmr_lay_stride, const double *vmr_scalar,
                           int top_at_1, int n_gauss_angles, const double *sfc_emis, const double *inc_flux, int nband_p,
                           const double *tau_p, const double *ssa_p, double *flux_up, double *flux_dn, int memspace,
                           void *stream) {
  const LwColumns c{ncol, nlay, plev, tlay, tsfc, tlev, GasDesc{ngas, gas_names, vmr, vmr_col_stride, vmr_lay_stride, vmr_scalar},
                    top_at_1, n_gauss_angles, sfc_emis, inc_flux};
  LwParticles pt;
  pt.tau = tau_p; pt.ssa = ssa_p;
  const FluxOutputs o{Fluxes{flux_up, flux_dn}};
  return lw_fluxes_impl(&kLwAllsky, false, m, c, nband_p, pt, o, memspace, stream);
}

int ecckd_lw_fluxes_allsky_mcica(const ecckd_model_t *m, int ncol, int nlay, const double *plev, const double *tlay,
                                 const double *tsfc, const double *tlev, int ngas, const char *gas_names,
                                 const double *const *vmr, const long long *vmr_col_stride, const long long *vmr_lay_stride,
                                 const double *vmr_scalar, int top_at_1, int n_gauss_angles, const double *sfc_emis,
                                 const double *inc_flux, int nband_p, const double *tau_p, const double *ssa_p,
                                 const unsigned long long *cloud_mask, double *flux_up, double *flux_dn, int memspace,
                                 void *stream) {
  const LwColumns c{ncol, nlay, plev, tlay, tsfc, tlev, GasDesc{ngas, gas_names, vmr, vmr_col_stride, vmr_lay_stride, vmr_scalar},
                    top_at_1, n_gauss_angles, sfc_emis, inc_flux};
  return lw_fluxes_impl(&kLwAllsky, false, m, c, nband_p, LwParticles{tau_p, ssa_p, nullptr, cloud_mask},
                        FluxOutputs{Fluxes{flux_up, flux_dn}}, memspace, stream);
}

// The superset of the four calls above, with flux_up_jac of the sky that flux_up holds (include/ecckd_hip.h)
int ecckd_lw_fluxes_jac(const ecckd_model_t *m, int ncol, int nlay, const double *plev, const double *tlay, const double *tsfc,
                        const double *tlev, int ngas, const char *gas_names, const double *const *vmr,
                        const long long *vmr_col_stride, const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1,
                        int n_gauss_angles, const double *sfc_emis, const double *inc_flux, int nband_p, const double *tau_p,
                        const double *ssa_p, const unsigned long long *cloud_mask, double *flux_up, double *flux_dn,
                        double *flux_up_clear, double *flux_dn_clear, double *flux_up_jac, int memspace, void *stream) {
  const LwColumns c{ncol, nlay, plev, tlay, tsfc, tlev, GasDesc{ngas, gas_names, vmr, vmr_col_stride, vmr_lay_stride, vmr_scalar},
                    top_at_1, n_gauss_angles, sfc_emis, inc_flux};
  const LwParticles pt{tau_p, ssa_p, nullptr, cloud_mask};
  const FluxOutputs o{Fluxes{flux_up, flux_dn}, Fluxes{flux_up_clear, flux_dn_clear}, Fluxes{}, flux_up_jac};
  // without tau_p: the clear sky of ecckd_lw_fluxes, whose list refuses whatever else of the particles' is named
  return lw_fluxes_impl(tau_p ? &kLwAllsky : nullptr, false, m, c, nband_p, pt, o, memspace, stream);
}

// ---- fused all-sky longwave with scattering clouds: gas optics -> Planck sources -> two-stream solver (PART / MASK) ----

// scratch of the device route, in doubles, in this order: optical depth, the three Planck arrays, the surface source (the
// two-stream solver's ring follows, ecckd_rte_lw_2stream_scratch_bytes)
static size_t allsky_2stream_doubles(const ecckd_model *m, int ncol, int nlay) {
  const size_t n3 = (size_t)ncol * nlay * m->ng;
  return r32(n3) + 3 * n3 + r32((size_t)ncol * m->ng);
}

static const char kScatteringPlanesTail[] =
    ": null argument (tau_p, ssa_p and g_p are required; one-stream particles: ecckd_lw_fluxes_allsky)";

// The two-stream solver's arguments on device pointers: the optical depth, the sources of `src` (the layer source is not
// read), the particles and where the fluxes go
static int lw_2stream_args(const ecckd_model *m, const LwColumns &c, const LwParticles &pt, const Fluxes &to, const double *tau,
                           const PlanckSide &src, double *ring, ecckd::RteLw2strArgs &a) {
  if (fill_band_map(m->ng, m->nband, m->band2gpt.data(), a.gpt2band)) return 1;
  a.ncol = c.ncol; a.nlay = c.nlay; a.ng = m->ng; a.top_at_1 = c.top_at_1 ? 1 : 0; a.nband = m->nband;
  a.exact_division = 0;
  a.tau = tau; a.lev_source_inc = src.lev_inc; a.lev_source_dec = src.lev_dec; a.sfc_source = src.sfc_source;
  a.sfc_emis = c.sfc_emis; a.inc_flux = c.inc_flux;
  a.part_tau = pt.tau; a.part_ssa = pt.ssa; a.part_g = pt.g; a.part_mask = pt.mask;
  a.flux_up = to.up; a.flux_dn = to.dn; a.scratch = ring;
  return 0;
}

// behind the gas optics, on device pointers: `work` holds tau at its start
static int lw_allsky_2stream_dev(const ecckd_model *m, const LwColumns &c, const LwParticles &pt, const Fluxes &to, double *work,
                                 hipStream_t stream) {
  const size_t n3 = (size_t)c.ncol * c.nlay * m->ng;
  double *tau = work, *lay = tau + r32(n3), *inc = lay + n3, *dec = inc + n3, *sfc = dec + n3, *ring = sfc + r32((size_t)c.ncol * m->ng);
  const PlanckSide src{c.tlev, c.tsfc, lay, inc, dec, sfc};
  if (planck_sources_dev(m, c.ncol, c.nlay, c.tlay, src, stream)) return 1;
  ecckd::RteLw2strArgs a{};
  if (lw_2stream_args(m, c, pt, to, tau, src, ring, a)) return 1;
  ProfScope prof("rte_lw_2stream_allsky", stream);
  HIPCHK(ecckd::launch_rte_lw_2str(a, stream));
  return 0;
}

size_t ecckd_lw_fluxes_allsky_2stream_f32_scratch_bytes(const ecckd_model_t *m, int ncol, int nlay) {
  if (!m || ncol <= 0 || nlay <= 0) return 0;
  return lw_2stream_work_f32(m, ncol, nlay).bytes();
}

// (f32: float arrays behind the double pointers -- the single-precision gas optics and Planck sources into the work block,
// then the float solver; the same list of refusals in the same order under the call's own name)
static int lw_fluxes_allsky_2stream_impl(bool f32, const ecckd_model_t *m, const LwColumns &c, int nband_p, const LwParticles &pt,
                                         const Fluxes &to, int memspace, void *stream) {
  CallWords words;
  words.who = words.who_mask = f32 ? "ecckd_lw_fluxes_allsky_2stream_f32" : "ecckd_lw_fluxes_allsky_2stream";
  words.planes_tail = kScatteringPlanesTail;
  bool done;
  if (lw_head(words, m, c, nband_p, pt)) return 1;
  // (the single-precision call names ECCKD_MIXED; the fp64 call has always answered it as a bad memspace, below)
  if (f32 && memspace == ECCKD_MIXED) return refuse(words.who, ": ECCKD_MIXED is not implemented (ECCKD_DEVICE or ECCKD_HOST)");
  if (check_model(m) || check_gas_optics_dims(c.ncol, c.nlay)) return 1;
  if (c.null_array() || !to.up || !to.dn) return refuse(words.who, ": null argument");
  if (lw_2stream_layers_fit(c.nlay) || on_device(m, c.ncol, memspace, &done)) return 1;
  if (done) return 0;
  const int ncol = c.ncol, nlay = c.nlay;
  const Counts n(ncol, nlay, m->ng, m->nband);
  const LwWorkF32 w = lw_2stream_work_f32(m, ncol, nlay);
  const size_t work_bytes = f32 ? w.bytes()
                                : allsky_2stream_doubles(m, ncol, nlay) * sizeof(double) + ecckd::rte_lw_2str_scratch_bytes(ncol, nlay, m->ng);
  Stage st(const_cast<ecckd_model *>(m), memspace, stream, f32);
  LwColumns d{};
  LwParticles d_pt{};
  Fluxes d_to{};
  double *work = nullptr;
  if (st.open([&] {
        d = c.staged(st, n);
        d_pt = pt.staged(st, n);
        d_to = to.staged(st, n.lev);
        work = st.work(work_bytes);
      }))
    return 1;
  if (f32) {
    const PlanckSide src = w.sources(work, d);
    if (gas_optics_lw_dev(m, true, ncol, nlay, d.plev, d.tlay, d.gas, w.tau(work), src, st.stream)) return 1;
    ecckd::RteLw2strArgs a{};
    if (lw_2stream_args(m, d, d_pt, d_to, w.tau(work), src, w.ring_at(work), a)) return 1;
    ProfScope prof("rte_lw_2stream_allsky_f32", st.stream);
    HIPCHK(ecckd::launch_rte_lw_2str_f32(a, st.stream));
    return st.close();
  }
  if (gas_optical_depth_dev(m, false, nullptr, ncol, nlay, d.plev, d.tlay, d.gas, work, false, nullptr, nullptr, nullptr, nullptr, st.stream))
    return 1;
  if (lw_allsky_2stream_dev(m, d, d_pt, d_to, work, st.stream)) return 1;
  return st.close();
}

int ecckd_lw_fluxes_allsky_2stream(const ecckd_model_t *m, int ncol, int nlay, const double *plev, const double *tlay,
                                   const double *tsfc, const double *tlev, int ngas, const char *gas_names,
                                   const double *const *vmr, const long long *vmr_col_stride, const long long *vmr_lay_stride,
                                   const double *vmr_scalar, int top_at_1, const double *sfc_emis, const double *inc_flux,
                                   int nband_p, const double *tau_p, const double *ssa_p, const double *g_p,
                                   const unsigned long long *cloud_mask, double *flux_up, double *flux_dn, int memspace,
                                   void *stream) {
  const LwColumns c{ncol, nlay, plev, tlay, tsfc, tlev, GasDesc{ngas, gas_names, vmr, vmr_col_stride, vmr_lay_stride, vmr_scalar},
                    top_at_1, 1, sfc_emis, inc_flux};
  const LwParticles pt{tau_p, ssa_p, g_p, cloud_mask};
  return lw_fluxes_allsky_2stream_impl(false, m, c, nband_p, pt, Fluxes{flux_up, flux_dn}, memspace, stream);
}

int ecckd_lw_fluxes_allsky_2stream_f32(const ecckd_model_t *m, int ncol, int nlay, const float *plev, const float *tlay,
                                       const float *tsfc, const float *tlev, int ngas, const char *gas_names,
                                       const float *const *vmr, const long long *vmr_col_stride, const long long *vmr_lay_stride,
                                       const double *vmr_scalar, int top_at_1, const float *sfc_emis, const float *inc_flux,
                                       int nband_p, const float *tau_p, const float *ssa_p, const float *g_p,
                                       const unsigned long long *cloud_mask, float *flux_up, float *flux_dn, int memspace,
                                       void *stream) {
  const LwColumns c{ncol, nlay, dp(plev), dp(tlay), dp(tsfc), dp(tlev),
                    GasDesc{ngas, gas_names, dp(vmr), vmr_col_stride, vmr_lay_stride, vmr_scalar}, top_at_1, 1, dp(sfc_emis),
                    dp(inc_flux)};
  LwParticles pt;
  pt.tau = dp(tau_p); pt.ssa = dp(ssa_p); pt.g = dp(g_p); pt.mask = cloud_mask;
  return lw_fluxes_allsky_2stream_impl(true, m, c, nband_p, pt, Fluxes{dp(flux_up), dp(flux_dn)}, memspace, stream);
}

// ---- rescaled no-scattering longwave solver (RTE-RRTMGP's lw_solver_1rescl_GaussQuad): cheap cloud scattering ----

// bytes of one spectral plane set (ncol,nlay+1,ngpt), rounded as the scratch layouts below place it
static size_t resc_plane_doubles(int ncol, int nlay, int ngpt) { return r32((size_t)ncol * (nlay + 1) * ngpt); }

size_t ecckd_rte_lw_rescaled_scratch_bytes(int ncol, int nlay, int ngpt) {
  if (ncol <= 0 || nlay < 1 || ngpt < 1 || nlay == 60) return 0;
  return sizeof(double) * 3 * resc_plane_doubles(ncol, nlay, ngpt);
}

static void fill_resc_gpt(ecckd::RteLwRescGptArgs &q, const ecckd::RteLwArgs &a) {
  q.ncol = a.ncol; q.nlay = a.nlay; q.ng = a.ng; q.top_at_1 = a.top_at_1; q.nmus = a.nmus;
  for (int k = 0; k < a.nmus; ++k) { q.Ds[k] = a.Ds[k]; q.wts[k] = a.wts[k]; }
  q.tau = a.tau; q.ssa = a.ssa; q.g = a.g; q.lay_source = a.lay_source; q.lev_source_inc = a.lev_source_inc;
  q.lev_source_dec = a.lev_source_dec; q.sfc_emis = a.sfc_emis; q.sfc_src = a.sfc_source; q.inc_flux = a.inc_flux;
  q.nband = a.nband;
  std::memcpy(q.gpt2band, a.gpt2band, sizeof q.gpt2band);
  q.tau_thresh = a.tau_thresh; q.series3 = a.series3; q.inc_isotropic = a.inc_isotropic;
}

// The rescaled solver on device arrays (a.tau / ssa / g, the sources, a.flux_*).  60 layers: the layer-split kernel.  Any
// other layer count: the compatibility kernel into `spec` (spectral up, spectral dn, work: ecckd_rte_lw_rescaled_scratch_bytes)
// and the g-point sum of sum_broadband.
static int lw_rescaled_dev(const ecckd::RteLwArgs &a, double *spec, hipStream_t stream) {
  if (a.nlay == 60) {
    ProfScope prof("rte_lw_rescaled", stream);
    HIPCHK(ecckd::launch_rte_lw_rescaled_split(a, stream));
    return 0;
  }
  if (!spec) return fail("ecckd: internal: the rescaled longwave solver needs scratch for this layer count");
  const size_t plane = resc_plane_doubles(a.ncol, a.nlay, a.ng), nlev = (size_t)a.ncol * (a.nlay + 1);
  ecckd::RteLwRescGptArgs q{};
  fill_resc_gpt(q, a);
  q.flux_up = spec; q.flux_dn = spec + plane; q.work = spec + 2 * plane;
  {
    ProfScope prof("lw_1rescl_gpt", stream);
    HIPCHK(ecckd::launch_lw_1rescl_gpt(q, stream));
  }
  ProfScope prof("sum_broadband", stream);
  HIPCHK(ecckd::launch_sum_planes(q.flux_up, a.ng, nlev, a.flux_up, 0, stream));
  HIPCHK(ecckd::launch_sum_planes(q.flux_dn, a.ng, nlev, a.flux_dn, 0, stream));
  return 0;
}

// ecckd_rte_lw_rescaled_jac: the surface term and where the Jacobian goes, in the memory space of the call
struct RescJac { const double *sfc_source_jac; double *flux_up_jac; };

// The rescaled Jacobian on the cell's (tau, ssa, g) on the device, behind the flux pass: the stand-alone kernel.  The surface
// term is sfc_source_jac(ncol,ng), or -- null -- formed from tsfc and the model's Planck table.
static int lw_rescaled_jac_dev(const ecckd::RteLwArgs &a, const double *sfc_source_jac, const ecckd_model *m, const double *tsfc,
                               double *jac, hipStream_t stream) {
  ecckd::RteLwRescJacArgs j{};
  std::memcpy(j.gpt2band, a.gpt2band, sizeof j.gpt2band);
  j.ncol = a.ncol; j.nlay = a.nlay; j.ng = a.ng; j.top_at_1 = a.top_at_1; j.nmus = a.nmus; j.nband = a.nband;
  for (int k = 0; k < a.nmus; ++k) { j.Ds[k] = a.Ds[k]; j.wts[k] = a.wts[k]; }
  j.tau = a.tau; j.ssa = a.ssa; j.g = a.g; j.part_tau = a.part_tau; j.part_ssa = a.part_ssa; j.part_g = a.part_g; j.part_mask = a.part_mask;
  j.sfc_source_jac = sfc_source_jac; j.tsfc = tsfc; j.sfc_emis = a.sfc_emis; j.flux_up_jac = jac;
  ProfScope prof("rte_lw_rescaled_jac", stream);
  if (m)
    HIPCHK(ecckd::launch_rte_lw_rescaled_jac(j, m->dbuf + m->off_planck, m->ntp, m->temperature_planck[0],
                                             m->temperature_planck[1] - m->temperature_planck[0], stream));
  else
    HIPCHK(ecckd::launch_rte_lw_rescaled_jac(j, nullptr, 0, 0., 1., stream));
  return 0;
}

static int rte_lw_rescaled_impl(int device, int ncol, int nlay, int ngpt, int top_at_1, int n_gauss_angles, const double *tau,
                                const double *ssa, const double *g, const double *lay_source, const double *lev_source_inc,
                                const double *lev_source_dec, const double *sfc_source, int nband, const int *band2gpt,
                                const double *sfc_emis, const double *inc_flux, double *flux_up, double *flux_dn, int memspace,
                                void *stream, const RescJac *jx = nullptr) {
  if (check_dims(ncol, nlay)) return 1;
  if (n_gauss_angles < 1 || n_gauss_angles > 4) return fail("rte_lw: have to ask for at least one quadrature point and no more than 4");
  if (!tau || !ssa || !g || !lay_source || !lev_source_inc || !lev_source_dec || !sfc_source || !sfc_emis || !flux_up || !flux_dn)
    return fail("ecckd_rte_lw_rescaled: null argument (only inc_flux may be null)");
  if (refuse_level_buffer("ecckd_rte_lw_rescaled", lev_source_inc, lev_source_dec, ncol, nlay, memspace)) return 1;
  ecckd::RteLwArgs a{};
  if (fill_band_map(ngpt, nband, band2gpt, a.gpt2band)) return 1;
  if (memspace == ECCKD_MIXED) return fail("ecckd_rte_lw_rescaled: ECCKD_MIXED is not implemented (ECCKD_DEVICE or ECCKD_HOST)");
  if (memspace != ECCKD_DEVICE && memspace != ECCKD_HOST) return fail("ecckd: bad memspace");
  if (jx) {   // this call's own refusals, behind those of ecckd_rte_lw_rescaled that need no device
    if (!jx->sfc_source_jac || !jx->flux_up_jac)
      return fail("ecckd_rte_lw_rescaled_jac: null argument (sfc_source_jac and flux_up_jac are required)");
    if (jx->flux_up_jac == flux_up || jx->flux_up_jac == flux_dn)
      return fail("ecckd_rte_lw_rescaled_jac: flux_up_jac must not be one of the flux outputs");
  }
  if (check_device(device)) return 1;
  if (ncol == 0) return 0;
  a.ncol = ncol; a.nlay = nlay; a.ng = ngpt; a.top_at_1 = top_at_1 ? 1 : 0; a.nband = nband;
  fill_lw_options(a, n_gauss_angles, false);
  const Counts n(ncol, nlay, ngpt, nband);
  Stage st(device, memspace, stream, false);
  ScratchLease lease;   // (held until the kernels of this call have been launched)
  void *sp = nullptr;
  const size_t scratch = ecckd_rte_lw_rescaled_scratch_bytes(ncol, nlay, ngpt);
  if (scratch && stream_scratch(device, st.stream, scratch, &sp, lease)) return 1;
  const double *d_sjac = nullptr;
  double *d_jac = nullptr;
  if (st.open([&] {
        a.tau = st.in(tau, n.lay_g); a.ssa = st.in(ssa, n.lay_g); a.g = st.in(g, n.lay_g);
        a.lay_source = st.in(lay_source, n.lay_g); a.lev_source_inc = st.in(lev_source_inc, n.lay_g);
        a.lev_source_dec = st.in(lev_source_dec, n.lay_g); a.sfc_source = st.in(sfc_source, n.col_g);
        a.sfc_emis = st.in(sfc_emis, n.col_b); a.inc_flux = st.in(inc_flux, n.col_g);
        a.flux_up = st.out(flux_up, n.lev); a.flux_dn = st.out(flux_dn, n.lev);
        if (jx) { d_sjac = st.in(jx->sfc_source_jac, n.col_g); d_jac = st.out(jx->flux_up_jac, n.lev); }
      }))
    return 1;
  if (lw_rescaled_dev(a, static_cast<double *>(sp), st.stream)) return 1;
  if (jx && lw_rescaled_jac_dev(a, d_sjac, nullptr, nullptr, d_jac, st.stream)) return 1;
  return st.close();
}

int ecckd_rte_lw_rescaled(int device, int ncol, int nlay, int ngpt, int top_at_1, int n_gauss_angles, const double *tau,
                          const double *ssa, const double *g, const double *lay_source, const double *lev_source_inc,
                          const double *lev_source_dec, const double *sfc_source, int nband, const int *band2gpt,
                          const double *sfc_emis, const double *inc_flux, double *flux_up, double *flux_dn, int memspace,
                          void *stream) {
  return rte_lw_rescaled_impl(device, ncol, nlay, ngpt, top_at_1, n_gauss_angles, tau, ssa, g, lay_source, lev_source_inc,
                              lev_source_dec, sfc_source, nband, band2gpt, sfc_emis, inc_flux, flux_up, flux_dn, memspace, stream);
}

int ecckd_rte_lw_rescaled_jac(int device, int ncol, int nlay, int ngpt, int top_at_1, int n_gauss_angles, const double *tau,
                              const double *ssa, const double *g, const double *lay_source, const double *lev_source_inc,
                              const double *lev_source_dec, const double *sfc_source, const double *sfc_source_jac, int nband,
                              const int *band2gpt, const double *sfc_emis, const double *inc_flux, double *flux_up,
                              double *flux_dn, double *flux_up_jac, int memspace, void *stream) {
  const RescJac jx{sfc_source_jac, flux_up_jac};
  return rte_lw_rescaled_impl(device, ncol, nlay, ngpt, top_at_1, n_gauss_angles, tau, ssa, g, lay_source, lev_source_inc,
                              lev_source_dec, sfc_source, nband, band2gpt, sfc_emis, inc_flux, flux_up, flux_dn, memspace, stream,
                              &jx);
}

int ecckd_lw_solver_1rescl_gpt(int device, int ncol, int nlay, int ngpt, int top_at_1, int nmus, const double *Ds,
                               const double *weights, const double *tau, const double *ssa, const double *g,
                               const double *lay_source, const double *lev_source_inc, const double *lev_source_dec,
                               const double *sfc_emis, const double *sfc_src, const double *inc_flux, double *gpt_flux_up,
                               double *gpt_flux_dn, int memspace, void *stream) {
  if (check_dims(ncol, nlay)) return 1;
  if (ngpt < 1) return fail("ecckd_lw_solver_1rescl_gpt: bad ngpt");
  if (nmus < 1 || nmus > 4 || !Ds || !weights) return fail("ecckd_lw_solver_1rescl_gpt: 1..4 quadrature angles with Ds and weights");
  if (!tau || !ssa || !g || !lay_source || !lev_source_inc || !lev_source_dec || !sfc_emis || !sfc_src || !gpt_flux_up || !gpt_flux_dn)
    return fail("ecckd_lw_solver_1rescl_gpt: null argument (only inc_flux may be null)");
  if (refuse_level_buffer("ecckd_lw_solver_1rescl_gpt", lev_source_inc, lev_source_dec, ncol, nlay, memspace)) return 1;
  if (memspace != ECCKD_DEVICE && memspace != ECCKD_HOST) return fail("ecckd: bad memspace");
  if (check_device(device)) return 1;
  if (ncol == 0) return 0;
  ecckd::RteLwRescGptArgs a{};
  a.ncol = ncol; a.nlay = nlay; a.ng = ngpt; a.top_at_1 = top_at_1 ? 1 : 0; a.nmus = nmus;
  for (int k = 0; k < nmus; ++k) { a.Ds[k] = Ds[k]; a.wts[k] = weights[k]; }
  a.tau_thresh = lw_tau_thresh(false);
  a.series3 = g_opt.lw_series_terms.load() == 3;
  a.inc_isotropic = g_opt.lw_inc_flux_isotropic.load();
  const Counts n(ncol, nlay, ngpt, 1);
  Stage st(device, memspace, stream, false);
  ScratchLease lease;
  void *sp = nullptr;   // the radiances between the sweeps, one (ncol,nlay+1,ngpt) plane set
  if (stream_scratch(device, st.stream, sizeof(double) * resc_plane_doubles(ncol, nlay, ngpt), &sp, lease)) return 1;
  a.work = static_cast<double *>(sp);
  if (st.open([&] {
        a.tau = st.in(tau, n.lay_g); a.ssa = st.in(ssa, n.lay_g); a.g = st.in(g, n.lay_g);
        a.lay_source = st.in(lay_source, n.lay_g); a.lev_source_inc = st.in(lev_source_inc, n.lay_g);
        a.lev_source_dec = st.in(lev_source_dec, n.lay_g);
        a.sfc_emis = st.in(sfc_emis, n.col_g); a.sfc_src = st.in(sfc_src, n.col_g); a.inc_flux = st.in(inc_flux, n.col_g);
        a.flux_up = st.out(gpt_flux_up, n.lev * ngpt); a.flux_dn = st.out(gpt_flux_dn, n.lev * ngpt);
      }))
    return 1;
  {
    ProfScope prof("lw_1rescl_gpt", st.stream);
    HIPCHK(ecckd::launch_lw_1rescl_gpt(a, st.stream));
  }
  return st.close();
}

// scratch of the fused call behind the gas optical depth, in doubles: nothing at 60 layers (the Planck-recomputing
// layer-split kernel); otherwise ssa and g of the cells, the three Planck arrays, the surface source and the solver's planes
static bool resc_fused_kernel_applies(const ecckd_model *m, int nlay) {
  return nlay == 60 && ecckd::rte_lw_rescaled_planck_fits(m->ng, m->ntp);
}
static size_t allsky_rescaled_doubles(const ecckd_model *m, int ncol, int nlay) {
  const size_t n3 = r32((size_t)ncol * nlay * m->ng);
  if (resc_fused_kernel_applies(m, nlay)) return n3;
  return 6 * n3 + r32((size_t)ncol * m->ng) + 3 * resc_plane_doubles(ncol, nlay, m->ng);
}

size_t ecckd_lw_fluxes_allsky_rescaled_scratch_bytes(const ecckd_model_t *m, int ncol, int nlay) {
  if (!m || ncol <= 0 || nlay < 1) return 0;
  return sizeof(double) * allsky_rescaled_doubles(m, ncol, nlay);
}

// The work block with clear-sky outputs: behind the block of ecckd_lw_fluxes_allsky_rescaled, what the clear pass needs on
// its general route -- at 60 layers its sources and ring (nothing where the clear-sky layer-split kernel serves the model),
// otherwise the ring alone (the sources are the rescaled route's)
static size_t allsky_rescaled_jac_doubles(const ecckd_model *m, int ncol, int nlay, bool with_clear) {
  const size_t n = allsky_rescaled_doubles(m, ncol, nlay);
  if (!with_clear) return n;
  if (resc_fused_kernel_applies(m, nlay)) return n + r32(fused_scratch_doubles(m, ncol, nlay));
  return n + r32(ecckd::rte_lw_scratch_bytes(ncol, nlay, m->ng) / sizeof(double));
}

size_t ecckd_lw_fluxes_rescaled_jac_scratch_bytes(const ecckd_model_t *m, int ncol, int nlay, int with_clear) {
  if (!m || ncol <= 0 || nlay < 1) return 0;
  return sizeof(double) * allsky_rescaled_jac_doubles(m, ncol, nlay, with_clear != 0);
}

// ecckd_lw_fluxes_allsky_rescaled and ecckd_lw_fluxes_rescaled_jac (`o.clear`, `o.jac`: each may be null)
static int lw_fluxes_allsky_rescaled_impl(const ecckd_model_t *m, const LwColumns &c, int nband_p, const LwParticles &pt,
                                          const FluxOutputs &o, int memspace, void *stream) {
  CallWords w;
  w.who = w.who_mask = "ecckd_lw_fluxes_allsky_rescaled";
  w.planes_tail = kScatteringPlanesTail;
  // ecckd_lw_fluxes_rescaled_jac's own, behind the refusals that a host-only model answers too and before the model is
  // asked for its device
  w.who_clear = "ecckd_lw_fluxes_rescaled_jac";
  w.clear_tail = ": null argument (flux_up_clear and flux_dn_clear are given together or not at all)";
  bool done;
  if (lw_head(w, m, c, nband_p, pt) || gauss_refusals(c) || clear_refusals(w, o) || jac_refusals(w.who_clear, o)) return 1;
  if (check_model(m) || check_gas_optics_dims(c.ncol, c.nlay)) return 1;
  if (c.null_array() || !o.all.up || !o.all.dn) return refuse(w.who, ": null argument");
  if (on_device(m, c.ncol, memspace, &done)) return 1;
  if (done) return 0;
  const int ncol = c.ncol, nlay = c.nlay;
  const Counts n(ncol, nlay, m->ng, m->nband);
  const bool with_clear = o.clear.up != nullptr;
  const bool resc_fused = resc_fused_kernel_applies(m, nlay);
  // the Jacobian inside the 60-layer flux kernel ("lw_jac_inline" = 1, and its third accumulator plane fits next to the
  // model's Planck table), or from the stand-alone kernel behind the flux pass
  const bool jac_in = o.jac && resc_fused && g_opt.lw_jac_inline.load() == 1 && ecckd::rte_lw_rescaled_planck_fits(m->ng, m->ntp, true);
  Stage st(const_cast<ecckd_model *>(m), memspace, stream, false);
  LwColumns d{};
  LwParticles d_pt{};
  FluxOutputs d_o{};
  double *work = nullptr;
  if (st.open([&] {
        d = c.staged(st, n);
        d_pt = LwParticles{pt.tau, pt.ssa, nullptr, pt.mask}.staged(st, n);
        d_pt.g = st.in(pt.g, n.lay_b);   // (this call has always declared g behind the mask: its rooms stay where they were)
        d_o.all = o.all.staged(st, n.lev);
        d_o.clear = o.clear.staged(st, n.lev);
        d_o.jac = st.out(o.jac, n.lev);
        work = st.work(allsky_rescaled_jac_doubles(m, ncol, nlay, with_clear) * sizeof(double));
      }))
    return 1;
  ecckd::RteLwArgs a{};
  if (lw_solver_args(m, d, false, a)) return 1;
  a.flux_up = d_o.all.up; a.flux_dn = d_o.all.dn;
  const hipStream_t s = st.stream;
  if (gas_optical_depth_dev(m, false, nullptr, ncol, nlay, d.plev, d.tlay, d.gas, work, false, nullptr, nullptr, nullptr, nullptr, s))
    return 1;
  a.tau = work;
  double *const clear_extra = work + allsky_rescaled_doubles(m, ncol, nlay);   // (with_clear: what the clear pass needs)
  if (resc_fused) {   // the band triple and the mask ride into the solver
    // the clear sky first, from the gas optical depth as it stands: the launch of ecckd_lw_fluxes
    if (with_clear && rte_lw_fused_dev(m, d, work, d_o.clear, fused_scratch_doubles(m, ncol, nlay) ? clear_extra : nullptr, s)) return 1;
    a.part_tau = d_pt.tau; a.part_ssa = d_pt.ssa; a.part_g = d_pt.g; a.part_mask = d_pt.mask;
    {
      ProfScope prof("rte_lw_rescaled_allsky", s);
      HIPCHK(ecckd::launch_rte_lw_rescaled_planck(a, m->dbuf + m->off_planck, m->ntp, m->temperature_planck[0],
                                                  m->temperature_planck[1] - m->temperature_planck[0], d.tlay, d.tlev, d.tsfc, s,
                                                  jac_in ? d_o.jac : nullptr));
    }
    // (scratch still holds the gas optical depth: the stand-alone kernel forms the cell's triple as the flux kernel did)
    if (o.jac && !jac_in && lw_rescaled_jac_dev(a, nullptr, m, d.tsfc, d_o.jac, s)) return 1;
    return st.close();
  }
  // any other layer count (slow): Planck sources and the by-band increment on (tau, 0, 0) through scratch, then the
  // compatibility route of ecckd_rte_lw_rescaled
  const size_t n3 = r32(n.lay_g);
  double *ssa = work + n3, *g = ssa + n3, *lay = g + n3, *inc = lay + n3, *dec = inc + n3, *sfc = dec + n3;
  double *spec = sfc + r32((size_t)ncol * m->ng);
  const PlanckSide src{d.tlev, d.tsfc, lay, inc, dec, sfc};
  if (planck_sources_dev(m, ncol, nlay, d.tlay, src, s)) return 1;
  // the clear sky before the by-band increment: the general route of ecckd_lw_fluxes on these sources
  if (with_clear && rte_lw_fused_dev(m, d, work, d_o.clear, ecckd::rte_lw_scratch_bytes(ncol, nlay, m->ng) ? clear_extra : nullptr, s,
                                     nullptr, nullptr, false, nullptr, &src))
    return 1;
  HIPCHK(hipMemsetAsync(ssa, 0, 2 * n3 * sizeof(double), s));
  if (lw_increment_dev(m, ncol, nlay, work, d_pt, s, ssa, g)) return 1;
  a.ssa = ssa; a.g = g; a.lay_source = lay; a.lev_source_inc = inc; a.lev_source_dec = dec; a.sfc_source = sfc;
  if (lw_rescaled_dev(a, spec, s)) return 1;
  // on the (tau, ssa, g) the increment left in scratch
  if (o.jac && lw_rescaled_jac_dev(a, nullptr, m, d.tsfc, d_o.jac, s)) return 1;
  return st.close();
}

int ecckd_lw_fluxes_allsky_rescaled(const ecckd_model_t *m, int ncol, int nlay, const double *plev, const double *tlay,
                                    const double *tsfc, const double *tlev, int ngas, const char *gas_names,
                                    const double *const *vmr, const long long *vmr_col_stride, const long long *vmr_lay_stride,
                                    const double *vmr_scalar, int top_at_1, int n_gauss_angles, const double *sfc_emis,
                                    const double *inc_flux, int nband_p, const double *tau_p, const double *ssa_p,
                                    const double *g_p, const unsigned long long *cloud_mask, double *flux_up, double *flux_dn,
                                    int memspace, void *stream) {
  const LwColumns c{ncol, nlay, plev, tlay, tsfc, tlev, GasDesc{ngas, gas_names, vmr, vmr_col_stride, vmr_lay_stride, vmr_scalar},
                    top_at_1, n_gauss_angles, sfc_emis, inc_flux};
  return lw_fluxes_allsky_rescaled_impl(m, c, nband_p, LwParticles{tau_p, ssa_p, g_p, cloud_mask},
                                        FluxOutputs{Fluxes{flux_up, flux_dn}}, memspace, stream);
}

int ecckd_lw_fluxes_rescaled_jac(const ecckd_model_t *m, int ncol, int nlay, const double *plev, const double *tlay,
                                 const double *tsfc, const double *tlev, int ngas, const char *gas_names,
                                 const double *const *vmr, const long long *vmr_col_stride, const long long *vmr_lay_stride,
                                 const double *vmr_scalar, int top_at_1, int n_gauss_angles, const double *sfc_emis,
                                 const double *inc_flux, int nband_p, const double *tau_p, const double *ssa_p,
                                 const double *g_p, const unsigned long long *cloud_mask, double *flux_up, double *flux_dn,
                                 double *flux_up_clear, double *flux_dn_clear, double *flux_up_jac, int memspace, void *stream) {
  const LwColumns c{ncol, nlay, plev, tlay, tsfc, tlev, GasDesc{ngas, gas_names, vmr, vmr_col_stride, vmr_lay_stride, vmr_scalar},
                    top_at_1, n_gauss_angles, sfc_emis, inc_flux};
  const LwParticles pt{tau_p, ssa_p, g_p, cloud_mask};
  const FluxOutputs o{Fluxes{flux_up, flux_dn}, Fluxes{flux_up_clear, flux_dn_clear}, Fluxes{}, flux_up_jac};
  return lw_fluxes_allsky_rescaled_impl(m, c, nband_p, pt, o, memspace, stream);
}

// ---- fused shortwave: total optical depth only between the kernels (SURVEY 8(f) rank 4 for the shortwave) ----

// The work block of sw_fluxes_run: the optical depth, the solver's room, the three scaled band planes (or none)
struct SwWork {
  size_t tau_bytes, solver, plane;
  SwWork(const ecckd_model *m, bool f32, int ncol, int nlay, bool scaled_planes, bool two_pass = false) {
    const Counts n(ncol, nlay, m->ng, m->nband);
    tau_bytes = align256(n.lay_g * esz(f32));
    solver = sw_fluxes_solver_bytes(m->device, ncol, nlay, m->ng, two_pass);
    plane = scaled_planes ? align256(n.lay_b * esz(f32)) : 0;
  }
  size_t bytes() const { return tau_bytes + solver + 3 * plane; }
};

// The delta-scaled copy of the band triple (f = g*g) in three planes of `plane` bytes at `room`: the caller's arrays are
// never written, `pt` points at the copy afterwards
static int delta_scaled_copy(SwParticles &pt, size_t count, char *room, size_t plane, bool f32, hipStream_t stream) {
  double *q_tau = reinterpret_cast<double *>(room), *q_ssa = reinterpret_cast<double *>(room + plane),
         *q_g = reinterpret_cast<double *>(room + 2 * plane);
  ProfScope prof("delta_scale", stream);
  HIPCHK(ecckd::launch_delta_scale(count, pt.tau, pt.ssa, pt.g, nullptr, q_tau, q_ssa, q_g, f32 ? 1 : 0, stream));
  pt.tau = q_tau; pt.ssa = q_ssa; pt.g = q_g;
  return 0;
}

// The fused shortwave calls behind their refusals: gas optical depth into the work block, then the solver -- once, or for
// the clear sky first where `o.clear` is named
static int sw_fluxes_run(bool f32, const ecckd_model *m, const SwColumns &c, const SwParticles &pt, const FluxOutputs &o,
                         int memspace, void *stream) {
  const int ncol = c.ncol, nlay = c.nlay;
  const Counts n(ncol, nlay, m->ng, m->nband);
  const bool part = pt.tau != nullptr, both = o.clear.up != nullptr;
  // The work block: tau between the two kernels, the solver's room behind it, and -- all-sky with delta scaling -- three
  // band planes for the scaled copy of the particles.  With device arrays it is the stream's scratch block, so the
  // capture rules of stream_scratch cover all of it.
  const SwWork work(m, f32, ncol, nlay, part && pt.delta_scale, part && pt.scaling);
  Stage st(const_cast<ecckd_model *>(m), memspace, stream, f32);
  SwColumns d{};
  SwParticles d_pt{};
  FluxOutputs d_o{};
  double *d_tau = nullptr;
  if (st.open([&] {
        d = c.staged(st, n);
        d_pt = pt.staged(st, n);
        d_o.clear = o.clear.staged(st, n.lev);
        d_o.all = o.all.staged(st, n.lev);
        d_tau = st.work(work.bytes());
      }))
    return 1;
  char *const room = reinterpret_cast<char *>(d_tau) + work.tau_bytes;
  if (work.plane && delta_scaled_copy(d_pt, n.lay_b, room + work.solver, work.plane, f32, st.stream)) return 1;
  // gas_optics_ext's tau (:449-456) without ssa / g: the total optical depth, gases + Rayleigh
  if (gas_optical_depth_dev(m, f32, nullptr, ncol, nlay, d.plev, d.tlay, d.gas, d_tau, true, nullptr, nullptr, nullptr, nullptr, st.stream))
    return 1;
  SwDerive dv{d.plev, table(m, m->off_rayleigh, f32), table(m, m->off_solar, f32), d.toa_scale, gw(f32),
              work.solver ? reinterpret_cast<double *>(room) : nullptr};
  auto solve = [&](const Fluxes &to) {   // (its arrays are on the device by now, whatever the call's memory space)
    return rte_sw_impl(Call{f32, -1, false, &dv}, m->device, ncol, nlay, m->ng, d.top_at_1, d_tau, nullptr, nullptr, d.mu0, nullptr,
                       m->nband, m->band2gpt.data(), d.sfc_alb_dir, d.sfc_alb_dif, to.up, to.dn, to.dir, ECCKD_DEVICE, st.stream);
  };
  // ecckd_sw_fluxes_clear_allsky: the clear-sky solver of ecckd_sw_fluxes first, on the same tau and in the same room
  if (both && solve(d_o.clear)) return 1;
  if (part) { dv.part_tau = d_pt.tau; dv.part_ssa = d_pt.ssa; dv.part_g = d_pt.g; dv.part_mask = d_pt.mask; dv.part_scaling = d_pt.scaling; }
  if (solve(d_o.all)) return 1;
  return st.close();
}

// (`w`: the words of an all-sky form, whose list goes first; null: ecckd_sw_fluxes)
static int sw_fluxes_impl(const CallWords *w, bool f32, const ecckd_model_t *m, const SwColumns &c, int nband_p, const SwParticles &pt,
                          const FluxOutputs &o, int memspace, void *stream) {
  bool done;
  if (w && (sw_head(*w, m, nband_p, pt, o) || clear_refusals(*w, o))) return 1;
  if (sw_plain_tail(m, c, o, memspace, &done)) return 1;
  return done ? 0 : sw_fluxes_run(f32, m, c, pt, o, memspace, stream);
}

// the words of the all-sky forms (clear_required: the clear-sky outputs are part of the call)
static CallWords sw_allsky_words(bool clear_required = false) {
  CallWords w;
  w.who = "ecckd_sw_fluxes_allsky";
  w.who_mask = "ecckd_sw_fluxes_allsky_mcica";
  w.planes_tail = ": null argument (tau_p, ssa_p and g_p are all required)";
  w.who_clear = "ecckd_sw_fluxes_clear_allsky";
  w.clear_tail = ": null argument (flux_up_clear and flux_dn_clear are both required; flux_dir_clear may be null)";
  w.clear_required = clear_required;
  return w;
}
static const CallWords kSwAllsky = sw_allsky_words(), kSwClearAllsky = sw_allsky_words(true);

int ecckd_sw_fluxes(const ecckd_model_t *m, int ncol, int nlay, const double *plev, const double *tlay, int ngas,
                    const char *gas_names, const double *const *vmr, const long long *vmr_col_stride,
                    const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1, const double *mu0,
                    const double *toa_scale, const double *sfc_alb_dir, const double *sfc_alb_dif, double *flux_up,
                    double *flux_dn, double *flux_dir, int memspace, void *stream) {
  const SwColumns c{ncol, nlay, plev, tlay, GasDesc{ngas, gas_names, vmr, vmr_col_stride, vmr_lay_stride, vmr_scalar}, top_at_1,
                    mu0, toa_scale, sfc_alb_dir, sfc_alb_dif};
  const FluxOutputs o{Fluxes{flux_up, flux_dn, flux_dir}};
  return sw_fluxes_impl(nullptr, false, m, c, 0, SwParticles{}, o, memspace, stream);
}

int ecckd_sw_fluxes_clear_allsky(const ecckd_model_t *m, int ncol, int nlay, const double *plev, const double *tlay, int ngas,
                                 const char *gas_names, const double *const *vmr, const long long *vmr_col_stride,
                                 const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1, const double *mu0,
                                 const double *toa_scale, const double *sfc_alb_dir, const double *sfc_alb_dif, int nband_p,
                                 const double *tau_p, const double *ssa_p, const double *g_p, int delta_scale,
                                 const unsigned long long *cloud_mask, double *flux_up, double *flux_dn, double *flux_dir,
                                 double *flux_up_clear, double *flux_dn_clear, double *flux_dir_clear, int memspace,
                                 void *stream) {
  const SwColumns c{ncol, nlay, plev, tlay, GasDesc{ngas, gas_names, vmr, vmr_col_stride, vmr_lay_stride, vmr_scalar}, top_at_1,
                    mu0, toa_scale, sfc_alb_dir, sfc_alb_dif};
  const SwParticles pt{tau_p, ssa_p, g_p, delta_scale, cloud_mask};
  const FluxOutputs o{Fluxes{flux_up, flux_dn, flux_dir}, Fluxes{flux_up_clear, flux_dn_clear, flux_dir_clear}};
  return sw_fluxes_impl(&kSwClearAllsky, false, m, c, nband_p, pt, o, memspace, stream);
}

int ecckd_sw_fluxes_allsky(const ecckd_model_t *m, int ncol, int nlay, const double *plev, const double *tlay, int ngas,
                           const char *gas_names, const double *const *vmr, const long long *vmr_col_stride,
                           const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1, const double *mu0,
                           const double *toa_scale, const double *sfc_alb_dir, const double *sfc_alb_dif, int nband_p,
                           const double *tau_p, const double *ssa_p, const double *g_p, int delta_scale, double *flux_up,
                           double *flux_dn, double *flux_dir, int memspace, void *stream) {
  const SwColumns c{ncol, nlay, plev, tlay, GasDesc{ngas, gas_names, vmr, vmr_col_stride, vmr_lay_stride, vmr_scalar}, top_at_1,
                    mu0, toa_scale, sfc_alb_dir, sfc_alb_dif};
  return sw_fluxes_impl(&kSwAllsky, false, m, c, nband_p, SwParticles{tau_p, ssa_p, g_p, delta_scale},
                        FluxOutputs{Fluxes{flux_up, flux_dn, flux_dir}}, memspace, stream);
}

int ecckd_sw_fluxes_allsky_mcica(const ecckd_model_t *m, int ncol, int nlay, const double *plev, const double *tlay, int ngas,
                                 const char *gas_names, const double *const *vmr, const long long *vmr_col_stride,
                                 const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1, const double *mu0,
                                 const double *toa_scale, const double *sfc_alb_dir, const double *sfc_alb_dif, int nband_p,
                                 const double *tau_p, const double *ssa_p, const double *g_p, int delta_scale,
                                 const unsigned long long *cloud_mask, double *flux_up, double *flux_dn, double *flux_dir,
                                 int memspace, void *stream) {
  const SwColumns c{ncol, nlay, plev, tlay, GasDesc{ngas, gas_names, vmr, vmr_col_stride, vmr_lay_stride, vmr_scalar}, top_at_1,
                    mu0, toa_scale, sfc_alb_dir, sfc_alb_dif};
  return sw_fluxes_impl(&kSwAllsky, false, m, c, nband_p, SwParticles{tau_p, ssa_p, g_p, delta_scale, cloud_mask},
                        FluxOutputs{Fluxes{flux_up, flux_dn, flux_dir}}, memspace, stream);
}

// ---- the shortwave on the daylit columns only (kernels_columns.hip): select, gather, solve, scatter ----

// A host list of columns as ecckd_daylit_columns delivers it: strictly ascending, inside [0,ncol)
static bool column_list_ok(const int *index, int nday, int ncol) {
  for (int k = 0; k < nday; ++k)
    if (index[k] < 0 || index[k] >= ncol || (k > 0 && index[k] <= index[k - 1])) return false;
  return true;
}

static int daylit_columns_impl(bool f32, int device, int ncol, const void *mu0, double mu0_min, int *day_index, int *nday,
                               int memspace, void *stream) {
  if (ncol < 0) return fail("ecckd_daylit_columns: bad ncol");
  if (!mu0 || !day_index || !nday) return fail("ecckd_daylit_columns: null argument");
  if (memspace != ECCKD_DEVICE && memspace != ECCKD_HOST) return fail("ecckd: bad memspace");
  if (check_device(device)) return 1;
  *nday = 0;
  if (ncol == 0) return 0;
  if (memspace == ECCKD_DEVICE && stream_is_capturing(static_cast<hipStream_t>(stream)))
    return fail("ecckd_daylit_columns: the call returns the count to the host and cannot be captured into a graph (select before "
                "the capture and capture ecckd_sw_fluxes_daylit with the list)");
  Stage st(device, memspace, stream, f32);
  const double *d_mu0 = nullptr;
  int *d_index = nullptr, *d_work = nullptr;
  if (st.open([&] {
        d_mu0 = st.in(static_cast<const double *>(mu0), (size_t)ncol);
        d_index = st.out(day_index, (size_t)ncol);
        d_work = reinterpret_cast<int *>(st.work(ecckd::daylit_work_bytes(ncol)));
      }))
    return 1;
  {
    ProfScope prof("daylit_columns", st.stream);
    HIPCHK(ecckd::launch_daylit_columns(d_mu0, f32, ncol, mu0_min, d_index, d_work, st.stream));
  }
  int count = 0;
  HIPCHK(hipMemcpyAsync(&count, d_work, sizeof(int), hipMemcpyDeviceToHost, st.stream));
  if (st.close()) return 1;
  HIPCHK(hipStreamSynchronize(st.stream));   // (host arrays: close() has synchronised already)
  *nday = count;
  return 0;
}

int ecckd_daylit_columns(int device, int ncol, const double *mu0, double mu0_min, int *day_index, int *nday, int memspace,
                         void *stream) {
  return daylit_columns_impl(false, device, ncol, mu0, mu0_min, day_index, nday, memspace, stream);
}
int ecckd_daylit_columns_f32(int device, int ncol, const float *mu0, double mu0_min, int *day_index, int *nday, int memspace,
                             void *stream) {
  return daylit_columns_impl(true, device, ncol, mu0, mu0_min, day_index, nday, memspace, stream);
}

// The refusals ecckd_gather_columns and ecckd_scatter_columns share
static int check_column_move(const char *who, int ninner, int ncol, int nouter, int elem_bytes, int nday, const int *day_index,
                             const void *src, const void *dst, int memspace) {
  const std::string w(who);
  if (ninner < 1 || ncol < 0 || nouter < 1) return fail(w + ": bad ninner / ncol / nouter");
  if (elem_bytes != 4 && elem_bytes != 8) return fail(w + ": elem_bytes must be 4 or 8");
  if (nday < 0 || nday > ncol) return fail(w + ": nday = " + std::to_string(nday) + " outside 0.." + std::to_string(ncol));
  if (nday > 0 && !day_index) return fail(w + ": day_index is NULL with nday > 0");
  if (nday > 0 && (!src || !dst)) return fail(w + ": null argument");
  if (memspace != ECCKD_DEVICE && memspace != ECCKD_HOST) return fail("ecckd: bad memspace");
  if (memspace == ECCKD_HOST && !column_list_ok(day_index, nday, ncol))
    return fail(w + ": day_index must be strictly ascending and inside [0,ncol)");
  return 0;
}

int ecckd_gather_columns(int device, int ninner, int ncol, int nouter, int elem_bytes, int nday, const int *day_index,
                         const void *src, void *dst, int memspace, void *stream) {
  if (check_column_move("ecckd_gather_columns", ninner, ncol, nouter, elem_bytes, nday, day_index, src, dst, memspace)) return 1;
  if (check_device(device)) return 1;
  if (nday == 0) return 0;
  Stage st(device, memspace, stream, false);
  const size_t full = (size_t)ninner * ncol * nouter * elem_bytes, part = (size_t)ninner * nday * nouter * elem_bytes;
  const int *d_index = nullptr;
  const void *d_src = nullptr;
  void *d_dst = nullptr;
  if (st.open([&] { d_index = st.in(day_index, (size_t)nday); d_src = st.in_bytes(src, full); d_dst = st.out_bytes(dst, part); }))
    return 1;
  {
    ProfScope prof("gather_columns", st.stream);
    HIPCHK(ecckd::launch_gather_columns(ninner, ncol, nouter, elem_bytes, nday, d_index, d_src, d_dst, st.stream));
  }
  return st.close();
}

int ecckd_scatter_columns(int device, int ninner, int ncol, int nouter, int elem_bytes, int nday, const int *day_index,
                          const void *src, void *dst, double fill, int memspace, void *stream) {
  if (check_column_move("ecckd_scatter_columns", ninner, ncol, nouter, elem_bytes, nday, day_index, src, dst, memspace)) return 1;
  if (!dst && ncol > 0) return fail("ecckd_scatter_columns: null argument");
  if (check_device(device)) return 1;
  if (ncol == 0) return 0;
  Stage st(device, memspace, stream, false);
  const size_t full = (size_t)ninner * ncol * nouter * elem_bytes, part = (size_t)ninner * nday * nouter * elem_bytes;
  const int *d_index = nullptr;
  const void *d_src = nullptr;
  void *d_dst = nullptr;
  if (st.open([&] { d_index = st.in(day_index, (size_t)nday); d_src = st.in_bytes(src, part); d_dst = st.out_bytes(dst, full); }))
    return 1;
  {
    ProfScope prof("scatter_columns", st.stream);
    HIPCHK(ecckd::launch_scatter_columns(ninner, ncol, nouter, elem_bytes, nday, d_index, d_src, d_dst, fill, st.stream));
  }
  return st.close();
}

// The rooms of ecckd_sw_fluxes_daylit behind the inner call's work block (SwWork): every array of the call on nday columns,
// each rounded up to 256 bytes, in the order of include/ecckd_hip.h.  toa_scale and the direct-beam outputs have their rooms
// whether or not they are given.
struct DaylitRooms {
  size_t lev, lay, col, col_b, lay_b;   // bytes of one room of each kind
  int ngas_arrays, nflux;
  bool particles, mask;
  DaylitRooms(const ecckd_model *m, int nday, int nlay, int ngas_arrays_, bool particles_, bool mask_, bool clear)
      : ngas_arrays(ngas_arrays_), nflux(clear ? 6 : 3), particles(particles_), mask(mask_) {
    const Counts n(nday, nlay, m->ng, m->nband);
    lev = align256(n.lev * 8); lay = align256(n.lay * 8); col = align256(n.col * 8); col_b = align256(n.col_b * 8);
    lay_b = align256(n.lay_b * 8);
  }
  size_t bytes() const {
    return lev + lay + 2 * col + 2 * col_b + (size_t)ngas_arrays * lay + (particles ? 3 * lay_b : 0) + (mask ? lay : 0) +
           (size_t)nflux * lev;
  }
};

size_t ecckd_sw_fluxes_daylit_scratch_bytes(const ecckd_model_t *m, int ncol, int nday, int nlay, int ngas_arrays,
                                            int with_particles, int delta_scale, int with_mask, int with_clear) {
  (void)ncol;   // (the scatter works in place on the caller's arrays: the full column count needs no room)
  if (!m || !m->finalized || nday <= 0 || nlay <= 0) return 0;
  if (ngas_arrays < 0) ngas_arrays = 0;
  const bool part = with_particles != 0;
  return SwWork(m, false, nday, nlay, part && delta_scale != 0).bytes() +
         DaylitRooms(m, nday, nlay, ngas_arrays, part, part && with_mask != 0, part && with_clear != 0).bytes();
}

int ecckd_sw_fluxes_daylit(const ecckd_model_t *m, int ncol, int nlay, int nday, const int *day_index, const double *plev,
                           const double *tlay, int ngas, const char *gas_names, const double *const *vmr,
                           const long long *vmr_col_stride, const long long *vmr_lay_stride, const double *vmr_scalar,
                           int top_at_1, const double *mu0, const double *toa_scale, const double *sfc_alb_dir,
                           const double *sfc_alb_dif, int nband_p, const double *tau_p, const double *ssa_p, const double *g_p,
                           int delta_scale, const unsigned long long *cloud_mask, double *flux_up, double *flux_dn,
                           double *flux_dir, double *flux_up_clear, double *flux_dn_clear, double *flux_dir_clear, int memspace,
                           void *stream) {
  const SwColumns c{ncol, nlay, plev, tlay, GasDesc{ngas, gas_names, vmr, vmr_col_stride, vmr_lay_stride, vmr_scalar}, top_at_1,
                    mu0, toa_scale, sfc_alb_dir, sfc_alb_dif};
  const SwParticles pt{tau_p, ssa_p, g_p, delta_scale, cloud_mask};
  const FluxOutputs o{Fluxes{flux_up, flux_dn, flux_dir}, Fluxes{flux_up_clear, flux_dn_clear, flux_dir_clear}};
  // the refusals of the all-sky calls in their order (those of the particles only with particles), then this call's own,
  // then those of ecckd_sw_fluxes, which sees nday columns only (and nothing at all with nday = 0)
  CallWords w;
  w.who = w.who_mask = w.who_clear = "ecckd_sw_fluxes_daylit";
  w.planes_tail = ": null argument (tau_p, ssa_p and g_p are given together or not at all)";
  w.no_particles_tail = ": clear sky (tau_p NULL) takes no ssa_p, g_p, cloud_mask or clear-sky outputs";
  w.clear_tail = ": null argument (flux_up_clear and flux_dn_clear are given together or not at all; flux_dir_clear may be null)";
  bool done;
  if (sw_head(w, m, nband_p, pt, o) || clear_refusals(w, o)) return 1;
  if (nday < 0 || nday > ncol)
    return fail("ecckd_sw_fluxes_daylit: nday = " + std::to_string(nday) + " outside 0.." + std::to_string(ncol));
  if (nday > 0 && !day_index) return fail("ecckd_sw_fluxes_daylit: day_index is NULL with nday > 0");
  if (memspace == ECCKD_HOST && !column_list_ok(day_index, nday, ncol))
    return fail("ecckd_sw_fluxes_daylit: day_index must be strictly ascending and inside [0,ncol)");
  if (check_model(m) || check_gas_optics_dims(ncol, nlay)) return 1;
  if (!m->has_solar) return fail("ecckd_sw_fluxes_daylit: model has no solar table (longwave model?)");
  if (c.null_array() || !flux_up || !flux_dn) return fail("ecckd_sw_fluxes_daylit: null argument");
  if (on_device(m, ncol, memspace, &done)) return 1;
  if (done) return 0;

  const bool cloudy = tau_p != nullptr, clear_out = o.clear.up != nullptr;
  int ngas_arrays = 0;   // the gas arrays that differ between columns: the others are read in place
  for (int j = 0; j < ngas && nday > 0; ++j)
    if (vmr && vmr[j] && vmr_col_stride && vmr_col_stride[j] != 0) ++ngas_arrays;
  const Counts n(ncol, nlay, m->ng, m->nband);
  const DaylitRooms rooms(m, nday, nlay, ngas_arrays, cloudy, cloud_mask != nullptr, clear_out);
  // With device arrays the work block is the stream's scratch block: the inner call asks for the same block and takes its
  // share from the front, the gathered arrays sit behind it.  With host arrays the gathered arrays are a room of the arena
  // and the inner call, which then runs on device arrays, takes the scratch block of the model's host stream.
  const size_t inner_bytes = nday > 0 && memspace == ECCKD_DEVICE ? SwWork(m, false, nday, nlay, cloudy && delta_scale).bytes() : 0;
  Stage st(const_cast<ecckd_model *>(m), memspace, stream, false);
  const int *d_index = nullptr;
  SwColumns d{};
  SwParticles d_pt{};
  FluxOutputs d_o{};
  double *d_work = nullptr;
  if (st.open([&] {
        if (nday > 0) {
          d_index = st.in(day_index, (size_t)nday);
          d = c.staged(st, n);
          if (cloudy) d_pt = pt.staged(st, n);
        }
        d_o.all = o.all.staged(st, n.lev);
        d_o.clear = o.clear.staged(st, n.lev);
        if (nday > 0) d_work = st.work(inner_bytes + rooms.bytes());
      }))
    return 1;
  const hipStream_t s = st.stream;
  double *const d_out[6] = {d_o.all.up, d_o.all.dn, d_o.all.dir, d_o.clear.up, d_o.clear.dn, d_o.clear.dir};
  double *g_out[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (nday > 0) {
    char *at = reinterpret_cast<char *>(d_work) + inner_bytes;
    auto take = [&at](size_t bytes) { double *p = reinterpret_cast<double *>(at); at += bytes; return p; };
    double *g_plev = take(rooms.lev), *g_tlay = take(rooms.lay), *g_mu0 = take(rooms.col), *g_scale = take(rooms.col);
    double *g_ad = take(rooms.col_b), *g_af = take(rooms.col_b);
    std::vector<const double *> g_vmr(ngas > 0 ? ngas : 1, nullptr);
    std::vector<long long> g_cs(ngas > 0 ? ngas : 1, 0), g_ls(ngas > 0 ? ngas : 1, 0);
    {
      ProfScope prof("daylit_gather", s);
      // (ninner, ncol, nouter) of each array: planes (1, ncol, n), albedos (nband, ncol, 1)
      auto gather = [&](int ninner, int nouter, const void *src, void *dst) {
        return ecckd::launch_gather_columns(ninner, ncol, nouter, 8, nday, d_index, src, dst, s);
      };
      HIPCHK(gather(1, nlay + 1, d.plev, g_plev));
      HIPCHK(gather(1, nlay, d.tlay, g_tlay));
      HIPCHK(gather(1, 1, d.mu0, g_mu0));
      if (d.toa_scale) HIPCHK(gather(1, 1, d.toa_scale, g_scale));
      HIPCHK(gather(m->nband, 1, d.sfc_alb_dir, g_ad));
      HIPCHK(gather(m->nband, 1, d.sfc_alb_dif, g_af));
      for (int j = 0; j < ngas; ++j) {
        g_vmr[j] = d.gas.vmr ? d.gas.vmr[j] : nullptr;
        g_cs[j] = vmr_col_stride ? vmr_col_stride[j] : 0;
        g_ls[j] = vmr_lay_stride ? vmr_lay_stride[j] : 0;
        if (!g_vmr[j] || g_cs[j] == 0) continue;
        double *room = take(rooms.lay);
        HIPCHK(ecckd::launch_gather_strided(ncol, nlay, 8, nday, d_index, g_cs[j], g_ls[j], g_vmr[j], room, s));
        g_vmr[j] = room; g_cs[j] = 1; g_ls[j] = nday;
      }
      if (cloudy) {
        double *g_tau = take(rooms.lay_b), *g_ssa = take(rooms.lay_b), *g_g = take(rooms.lay_b);
        HIPCHK(gather(1, nlay * m->nband, d_pt.tau, g_tau));
        HIPCHK(gather(1, nlay * m->nband, d_pt.ssa, g_ssa));
        HIPCHK(gather(1, nlay * m->nband, d_pt.g, g_g));
        d_pt.tau = g_tau; d_pt.ssa = g_ssa; d_pt.g = g_g;
        if (d_pt.mask) {
          double *g_mask = take(rooms.lay);
          HIPCHK(gather(1, nlay, d_pt.mask, g_mask));
          d_pt.mask = reinterpret_cast<const unsigned long long *>(g_mask);
        }
      }
    }
    for (int f = 0; f < 6; ++f)
      if (d_out[f]) g_out[f] = take(rooms.lev);
    // the pipeline of the plain calls, unchanged, on nday columns of device arrays
    const SwColumns g_c{nday, nlay, g_plev, g_tlay, GasDesc{ngas, gas_names, g_vmr.data(), g_cs.data(), g_ls.data(), vmr_scalar},
                        top_at_1, g_mu0, d.toa_scale ? g_scale : nullptr, g_ad, g_af};
    FluxOutputs g_o;
    g_o.all = Fluxes{g_out[0], g_out[1], g_out[2]};
    if (clear_out) g_o.clear = Fluxes{g_out[3], g_out[4], g_out[5]};
    if (sw_fluxes_run(false, m, g_c, cloudy ? d_pt : SwParticles{}, g_o, ECCKD_DEVICE, s)) return 1;
  }
  {
    ProfScope prof("daylit_scatter", s);
    for (int f = 0; f < 6; ++f)
      if (d_out[f]) HIPCHK(ecckd::launch_scatter_columns(1, ncol, nlay + 1, 8, nday, d_index, g_out[f], d_out[f], 0., s));
  }
  return st.close();
}

// ---- element-wise operations on optical properties (kernels_optical_props.hip) ----

static int delta_scale_impl(bool f32, int device, int ncol, int nlay, int n, double *tau, double *ssa, double *g,
                            const double *forward, int memspace, void *stream) {
  if (check_dims(ncol, nlay)) return 1;
  if (n < 1) return fail("ecckd_delta_scale: n must be at least 1");
  if (!tau || !ssa || !g) return fail("ecckd_delta_scale: null argument (two-stream properties: tau, ssa and g)");
  if (memspace != ECCKD_DEVICE && memspace != ECCKD_HOST) return fail("ecckd: bad memspace");
  const size_t n3 = (size_t)ncol * nlay * n;
  if (forward && memspace == ECCKD_HOST) {
    bool ok = true;
    if (f32) { const float *f = reinterpret_cast<const float *>(forward); for (size_t i = 0; i < n3 && ok; ++i) ok = f[i] >= 0.f && f[i] <= 1.f; }
    else for (size_t i = 0; i < n3 && ok; ++i) ok = forward[i] >= 0. && forward[i] <= 1.;
    if (!ok) return fail("ecckd_delta_scale: forward scattering fraction outside [0, 1]");
  }
  if (check_device(device)) return 1;
  if (ncol == 0) return 0;
  Stage st(device, memspace, stream, f32);
  double *d_tau = nullptr, *d_ssa = nullptr, *d_g = nullptr;
  const double *d_f = nullptr;
  if (st.open([&] { d_tau = st.inout(tau, n3); d_ssa = st.inout(ssa, n3); d_g = st.inout(g, n3); d_f = st.in(forward, n3); })) return 1;
  {
    ProfScope prof("delta_scale", st.stream);
    HIPCHK(ecckd::launch_delta_scale(n3, d_tau, d_ssa, d_g, d_f, d_tau, d_ssa, d_g, f32, st.stream));
  }
  return st.close();
}

int ecckd_delta_scale(int device, int ncol, int nlay, int n, double *tau, double *ssa, double *g, const double *forward,
                      int memspace, void *stream) {
  return delta_scale_impl(false, device, ncol, nlay, n, tau, ssa, g, forward, memspace, stream);
}
int ecckd_delta_scale_f32(int device, int ncol, int nlay, int n, float *tau, float *ssa, float *g, const float *forward,
                          int memspace, void *stream) {
  return delta_scale_impl(true, device, ncol, nlay, n, dp(tau), dp(ssa), dp(g), dp(forward), memspace, stream);
}

// mask: ecckd_increment_masked -- one word per (column, layer) in `memspace`, or null
static int increment_impl(bool f32, int device, int ncol, int nlay, int ngpt, double *tau1, double *ssa1, double *g1, int nband,
                          const int *band2gpt, const double *tau2, const double *ssa2, const double *g2, int memspace,
                          void *stream, const unsigned long long *mask = nullptr, const float *scaling = nullptr) {
  if (mask && ngpt > 64) return fail("ecckd_increment_masked" + std::string(kMaskTooWide) + std::to_string(ngpt));
  if (check_dims(ncol, nlay)) return 1;
  if (ngpt < 1) return fail("ecckd_increment: ngpt must be at least 1");
  if (!tau1 || !tau2) return fail("ecckd_increment: null argument (tau1 and tau2 are required)");
  if ((ssa1 == nullptr) != (g1 == nullptr))
    return fail("ecckd_increment: op1 has ssa without g or g without ssa (pass both: two-stream, or neither: one-stream)");
  if ((ssa2 == nullptr) != (g2 == nullptr))
    return fail("ecckd_increment: op2 has ssa without g or g without ssa (pass both: two-stream, or neither: one-stream)");
  ecckd::OptPropsArgs a{};
  if (nband < 0) return fail("ecckd_increment: nband must not be negative");
  if (nband > 0) {
    if (!band2gpt) return fail("ecckd_increment: band2gpt is required with nband > 0");
    if (nband > 256 || ngpt > 65535) return fail("ecckd_increment: at most 256 bands and 65535 g-points");
    int next = 1;   // bands in ascending order, each starting where the one before ended: they tile 1..ngpt
    for (int bnd = 0; bnd < nband; ++bnd) {
      const int lo = band2gpt[2 * bnd], hi = band2gpt[2 * bnd + 1];
      if (lo != next || hi < lo || hi > ngpt)
        return fail("ecckd_increment: band2gpt does not tile 1..ngpt (band " + std::to_string(bnd + 1) + " covers " +
                    std::to_string(lo) + ".." + std::to_string(hi) + ", expected to start at " + std::to_string(next) + ")");
      a.band_first[bnd] = (unsigned short)(lo - 1);
      next = hi + 1;
    }
    if (next != ngpt + 1) return fail("ecckd_increment: band2gpt does not tile 1..ngpt (the last band ends at " + std::to_string(next - 1) + ")");
    a.band_first[nband] = (unsigned short)ngpt;
  }
  if (memspace != ECCKD_DEVICE && memspace != ECCKD_HOST) return fail("ecckd: bad memspace");
  if (check_device(device)) return 1;
  if (ncol == 0) return 0;
  a.ncol = ncol; a.nlay = nlay; a.ng = ngpt; a.nband = nband; a.f32 = f32;
  const size_t n1 = (size_t)ncol * nlay * ngpt, n2 = (size_t)ncol * nlay * (nband > 0 ? nband : ngpt);
  Stage st(device, memspace, stream, f32);
  if (st.open([&] {
        a.mask = st.in(mask, (size_t)ncol * nlay);
        a.scaling = static_cast<const float *>(st.in_bytes(scaling, n1 * sizeof(float)));   // (float32 in either precision)
        a.tau1 = st.inout(tau1, n1); a.ssa1 = st.inout(ssa1, n1);
        a.g1 = st.inout(g1, n1, ssa2 != nullptr);   // (g1 changes only when op2 scatters)
        a.tau2 = st.in(tau2, n2); a.ssa2 = st.in(ssa2, n2); a.g2 = st.in(g2, n2);
      }))
    return 1;
  {
    ProfScope prof("increment", st.stream);
    HIPCHK(ecckd::launch_increment(a, st.stream));
  }
  return st.close();
}

int ecckd_increment(int device, int ncol, int nlay, int ngpt, double *tau1, double *ssa1, double *g1, int nband,
                    const int *band2gpt, const double *tau2, const double *ssa2, const double *g2, int memspace, void *stream) {
  return increment_impl(false, device, ncol, nlay, ngpt, tau1, ssa1, g1, nband, band2gpt, tau2, ssa2, g2, memspace, stream);
}
int ecckd_increment_f32(int device, int ncol, int nlay, int ngpt, float *tau1, float *ssa1, float *g1, int nband,
                        const int *band2gpt, const float *tau2, const float *ssa2, const float *g2, int memspace, void *stream) {
  return increment_impl(true, device, ncol, nlay, ngpt, dp(tau1), dp(ssa1), dp(g1), nband, band2gpt, dp(tau2), dp(ssa2), dp(g2),
                        memspace, stream);
}

int ecckd_increment_masked(int device, int ncol, int nlay, int ngpt, double *tau1, double *ssa1, double *g1, int nband,
                           const int *band2gpt, const double *tau2, const double *ssa2, const double *g2,
                           const unsigned long long *mask, int memspace, void *stream) {
  return increment_impl(false, device, ncol, nlay, ngpt, tau1, ssa1, g1, nband, band2gpt, tau2, ssa2, g2, memspace, stream, mask);
}
int ecckd_increment_masked_f32(int device, int ncol, int nlay, int ngpt, float *tau1, float *ssa1, float *g1, int nband,
                               const int *band2gpt, const float *tau2, const float *ssa2, const float *g2,
                               const unsigned long long *mask, int memspace, void *stream) {
  return increment_impl(true, device, ncol, nlay, ngpt, dp(tau1), dp(ssa1), dp(g1), nband, band2gpt, dp(tau2), dp(ssa2), dp(g2),
                        memspace, stream, mask);
}

int ecckd_increment_scaled(int device, int ncol, int nlay, int ngpt, double *tau1, double *ssa1, double *g1, int nband,
                           const int *band2gpt, const double *tau2, const double *ssa2, const double *g2, const float *scaling,
                           int memspace, void *stream) {
  return increment_impl(false, device, ncol, nlay, ngpt, tau1, ssa1, g1, nband, band2gpt, tau2, ssa2, g2, memspace, stream, nullptr,
                        scaling);
}
int ecckd_increment_scaled_f32(int device, int ncol, int nlay, int ngpt, float *tau1, float *ssa1, float *g1, int nband,
                               const int *band2gpt, const float *tau2, const float *ssa2, const float *g2, const float *scaling,
                               int memspace, void *stream) {
  return increment_impl(true, device, ncol, nlay, ngpt, dp(tau1), dp(ssa1), dp(g1), nband, band2gpt, dp(tau2), dp(ssa2), dp(g2),
                        memspace, stream, nullptr, scaling);
}

// ---- cloud optics (kernels_cloud_optics.hip): water paths and effective radii to band properties ----

int ecckd_cloud_optics_create_lut(int nband, int nsize_liq, int nsize_ice, int nrghice, double radliq_lwr, double radliq_upr,
                                  double radice_lwr, double radice_upr, const double *lut_extliq, const double *lut_ssaliq,
                                  const double *lut_asyliq, const double *lut_extice, const double *lut_ssaice,
                                  const double *lut_asyice, int device, ecckd_cloud_optics_t **cloud_optics) {
  if (!cloud_optics) return fail("ecckd_cloud_optics_create_lut: null argument (the handle)");
  *cloud_optics = nullptr;
  if (nband < 1) return fail("ecckd_cloud_optics_create_lut: nband must be at least 1");
  if (nsize_liq < 2 || nsize_ice < 2) return fail("ecckd_cloud_optics_create_lut: a table needs at least 2 sizes");
  if (nrghice < 1) return fail("ecckd_cloud_optics_create_lut: nrghice must be at least 1");
  if (!(radliq_upr > radliq_lwr)) return fail("ecckd_cloud_optics_create_lut: radliq_upr must exceed radliq_lwr");
  if (!(radice_upr > radice_lwr)) return fail("ecckd_cloud_optics_create_lut: radice_upr must exceed radice_lwr");
  if (!lut_extliq || !lut_ssaliq || !lut_asyliq || !lut_extice || !lut_ssaice || !lut_asyice)
    return fail("ecckd_cloud_optics_create_lut: null table (ext, ssa and asy of both phases are required)");
  ecckd_cloud_lut co;
  co.nband = nband; co.nsize_liq = nsize_liq; co.nsize_ice = nsize_ice; co.nrghice = nrghice;
  co.radliq_lwr = radliq_lwr; co.radliq_upr = radliq_upr; co.radice_lwr = radice_lwr; co.radice_upr = radice_upr;
  if (device != -1) {   // (-1: a host-only object: getters and refusals work, the compute call fails)
    if (check_device(device)) return 1;
    const auto liq64 = cloud_lut_image<double>(nsize_liq, nband, 1, lut_extliq, lut_ssaliq, lut_asyliq);
    const auto ice64 = cloud_lut_image<double>(nsize_ice, nband, nrghice, lut_extice, lut_ssaice, lut_asyice);
    const auto liq32 = cloud_lut_image<float>(nsize_liq, nband, 1, lut_extliq, lut_ssaliq, lut_asyliq);
    const auto ice32 = cloud_lut_image<float>(nsize_ice, nband, nrghice, lut_extice, lut_ssaice, lut_asyice);
    co.off_liq[0] = 0;
    co.off_ice[0] = align256(liq64.size() * 16);
    co.off_liq[1] = co.off_ice[0] + align256(ice64.size() * 16);
    co.off_ice[1] = co.off_liq[1] + align256(liq32.size() * 8);
    co.ice_stride[0] = ice64.size() / nrghice * 16;
    co.ice_stride[1] = ice32.size() / nrghice * 8;
    const size_t total = co.off_ice[1] + align256(ice32.size() * 8);
    std::vector<char> host(total, 0);
    std::memcpy(host.data() + co.off_liq[0], liq64.data(), liq64.size() * 16);
    std::memcpy(host.data() + co.off_ice[0], ice64.data(), ice64.size() * 16);
    std::memcpy(host.data() + co.off_liq[1], liq32.data(), liq32.size() * 8);
    std::memcpy(host.data() + co.off_ice[1], ice32.data(), ice32.size() * 8);
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&co.dbuf), total));
    if (hipMemcpy(co.dbuf, host.data(), total, hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(co.dbuf);
      return fail("ecckd_cloud_optics_create_lut: copying the tables to the device failed");
    }
    co.device = device;
  }
  *cloud_optics = new ecckd_cloud_lut(co);
  return 0;
}

void ecckd_cloud_optics_destroy(ecckd_cloud_optics_t *co) {
  if (!co) return;
  if (co->device >= 0 && co->dbuf) {
    (void)hipSetDevice(co->device);
    (void)hipFree(co->dbuf);
  }
  delete co;
}

int ecckd_cloud_optics_get_nband(const ecckd_cloud_optics_t *co) { return co ? co->nband : 0; }
int ecckd_cloud_optics_get_nrghice(const ecckd_cloud_optics_t *co) { return co ? co->nrghice : 0; }
double ecckd_cloud_optics_get_min_radius_liq(const ecckd_cloud_optics_t *co) { return co ? co->radliq_lwr : 0.; }
double ecckd_cloud_optics_get_max_radius_liq(const ecckd_cloud_optics_t *co) { return co ? co->radliq_upr : 0.; }
double ecckd_cloud_optics_get_min_radius_ice(const ecckd_cloud_optics_t *co) { return co ? co->radice_lwr : 0.; }
double ecckd_cloud_optics_get_max_radius_ice(const ecckd_cloud_optics_t *co) { return co ? co->radice_upr : 0.; }

static int cloud_optics_impl(bool f32, const ecckd_cloud_optics_t *co, int ncol, int nlay, const double *clwp, const double *ciwp,
                             const double *reliq, const double *reice, int icergh, double *tau, double *ssa, double *g,
                             int memspace, void *stream) {
  if (!co) return fail("ecckd_cloud_optics: null cloud-optics object");
  if (icergh < 1 || icergh > co->nrghice)
    return fail("ecckd_cloud_optics: ice roughness " + std::to_string(icergh) + " outside 1.." + std::to_string(co->nrghice));
  if ((ssa == nullptr) != (g == nullptr))
    return fail("ecckd_cloud_optics: ssa without g or g without ssa (pass both: two-stream, or neither: one-scalar)");
  if (check_dims(ncol, nlay)) return 1;
  if (!clwp || !ciwp || !reliq || !reice || !tau)
    return fail("ecckd_cloud_optics: null argument (clwp, ciwp, reliq, reice and tau are required)");
  if (memspace != ECCKD_DEVICE && memspace != ECCKD_HOST && memspace != ECCKD_MIXED) return fail("ecckd: bad memspace");
  const size_t n2 = (size_t)ncol * nlay, n3 = n2 * co->nband;
  if (memspace != ECCKD_DEVICE) {   // (host inputs; device inputs are not checked: the call stays asynchronous)
    const char *bad = f32 ? cloud_optics_check_host(*co, n2, reinterpret_cast<const float *>(clwp), reinterpret_cast<const float *>(ciwp),
                                                    reinterpret_cast<const float *>(reliq), reinterpret_cast<const float *>(reice))
                          : cloud_optics_check_host(*co, n2, clwp, ciwp, reliq, reice);
    if (bad) return fail(bad);
  }
  if (co->device < 0)
    return fail("ecckd_cloud_optics: host-only object (device -1): no GPU, no compute (there is no CPU fallback)");
  if (check_device(co->device)) return 1;
  if (ncol == 0) return 0;
  ecckd::CloudOpticsArgs a{};
  a.ncol = ncol; a.nlay = nlay; a.nband = co->nband; a.f32 = f32;
  a.nsize_liq = co->nsize_liq; a.nsize_ice = co->nsize_ice;
  a.cus = simd_slots(co->device) / 4;
  if (f32) {   // bounds rounded to float, the step formed in float
    const float ll = (float)co->radliq_lwr, il = (float)co->radice_lwr;
    a.radliq_lwr = ll; a.radliq_step = ((float)co->radliq_upr - ll) / (float)(co->nsize_liq - 1);
    a.radice_lwr = il; a.radice_step = ((float)co->radice_upr - il) / (float)(co->nsize_ice - 1);
  } else {
    a.radliq_lwr = co->radliq_lwr; a.radliq_step = (co->radliq_upr - co->radliq_lwr) / (double)(co->nsize_liq - 1);
    a.radice_lwr = co->radice_lwr; a.radice_step = (co->radice_upr - co->radice_lwr) / (double)(co->nsize_ice - 1);
  }
  a.lut_liq = co->dbuf + co->off_liq[f32];
  a.lut_ice = co->dbuf + co->off_ice[f32] + (size_t)(icergh - 1) * co->ice_stride[f32];
  Stage st(co->device, memspace, stream, f32);
  if (st.open([&] {
        a.clwp = st.in(clwp, n2); a.ciwp = st.in(ciwp, n2); a.reliq = st.in(reliq, n2); a.reice = st.in(reice, n2);
        a.tau = st.out(tau, n3, kBig); a.ssa = st.out(ssa, n3, kBig); a.g = st.out(g, n3, kBig);
      }))
    return 1;
  {
    ProfScope prof("cloud_optics", st.stream);
    HIPCHK(ecckd::launch_cloud_optics(a, st.stream));
  }
  return st.close();
}

int ecckd_cloud_optics(const ecckd_cloud_optics_t *co, int ncol, int nlay, const double *clwp, const double *ciwp,
                       const double *reliq, const double *reice, int icergh, double *tau, double *ssa, double *g, int memspace,
                       void *stream) {
  return cloud_optics_impl(false, co, ncol, nlay, clwp, ciwp, reliq, reice, icergh, tau, ssa, g, memspace, stream);
}
int ecckd_cloud_optics_f32(const ecckd_cloud_optics_t *co, int ncol, int nlay, const float *clwp, const float *ciwp,
                           const float *reliq, const float *reice, int icergh, float *tau, float *ssa, float *g, int memspace,
                           void *stream) {
  return cloud_optics_impl(true, co, ncol, nlay, dp(clwp), dp(ciwp), dp(reliq), dp(reice), icergh, dp(tau), dp(ssa), dp(g),
                           memspace, stream);
}

// ---- aerosol optics (kernels_aerosol_optics.hip): species, mass, size and humidity to band properties ----

int ecckd_aerosol_optics_create_lut(int nband, int nbin, int nrh, const double *bin_lims, const double *rh_levels,
                                    const double *dust_tbl, const double *salt_tbl, const double *sulf_tbl, const double *bcar_tbl,
                                    const double *bcar_rh_tbl, const double *ocar_tbl, const double *ocar_rh_tbl, int device,
                                    ecckd_aerosol_optics_t **aerosol_optics) {
  if (!aerosol_optics) return fail("ecckd_aerosol_optics_create_lut: null argument (the handle)");
  *aerosol_optics = nullptr;
  if (nband < 1 || nbin < 1) return fail("ecckd_aerosol_optics_create_lut: nband and nbin must be at least 1");
  if (nrh < 2) return fail("ecckd_aerosol_optics_create_lut: nrh must be at least 2");
  if (!rh_levels) return fail("ecckd_aerosol_optics_create_lut: rh_levels null, not strictly increasing, or NaN");
  for (int i = 0; i + 1 < nrh; ++i)
    if (!(rh_levels[i + 1] > rh_levels[i]))
      return fail("ecckd_aerosol_optics_create_lut: rh_levels null, not strictly increasing, or NaN");
  if (!bin_lims) return fail("ecckd_aerosol_optics_create_lut: bin_lims null, a bin empty or reversed, or bins overlapping");
  for (int b = 0; b < nbin; ++b)
    if (!(bin_lims[2 * b] < bin_lims[2 * b + 1]) || (b + 1 < nbin && !(bin_lims[2 * b + 1] <= bin_lims[2 * b + 2])))
      return fail("ecckd_aerosol_optics_create_lut: bin_lims null, a bin empty or reversed, or bins overlapping");
  if (!dust_tbl || !salt_tbl || !sulf_tbl || !bcar_tbl || !bcar_rh_tbl || !ocar_tbl || !ocar_rh_tbl)
    return fail("ecckd_aerosol_optics_create_lut: null table (dust, salt, sulf, bcar, bcar_rh, ocar and ocar_rh are required)");
  ecckd_aerosol_lut ao;
  ao.nband = nband; ao.nbin = nbin; ao.nrh = nrh;
  ao.bin_lims.assign(bin_lims, bin_lims + 2 * (size_t)nbin);
  ao.rh_levels.assign(rh_levels, rh_levels + nrh);
  if (device != -1) {   // (-1: a host-only object: getters and refusals work, the compute call fails)
    if (check_device(device)) return 1;
    const AerosolTables t{dust_tbl, salt_tbl, sulf_tbl, bcar_tbl, bcar_rh_tbl, ocar_tbl, ocar_rh_tbl};
    const auto head64 = aerosol_head<double>(nbin, nrh, bin_lims, rh_levels);
    const auto head32 = aerosol_head<float>(nbin, nrh, bin_lims, rh_levels);
    const auto img64 = aerosol_image<double>(nband, nbin, nrh, t);
    const auto img32 = aerosol_image<float>(nband, nbin, nrh, t);
    ao.off_head[0] = 0;
    ao.off_image[0] = align256(head64.size() * 8);
    ao.off_head[1] = ao.off_image[0] + align256(img64.size() * 16);
    ao.off_image[1] = ao.off_head[1] + align256(head32.size() * 4);
    const size_t total = ao.off_image[1] + align256(img32.size() * 8);
    std::vector<char> host(total, 0);
    std::memcpy(host.data() + ao.off_head[0], head64.data(), head64.size() * 8);
    std::memcpy(host.data() + ao.off_image[0], img64.data(), img64.size() * 16);
    std::memcpy(host.data() + ao.off_head[1], head32.data(), head32.size() * 4);
    std::memcpy(host.data() + ao.off_image[1], img32.data(), img32.size() * 8);
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&ao.dbuf), total));
    if (hipMemcpy(ao.dbuf, host.data(), total, hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(ao.dbuf);
      return fail("ecckd_aerosol_optics_create_lut: copying the tables to the device failed");
    }
    ao.device = device;
  }
  *aerosol_optics = new ecckd_aerosol_lut(ao);
  return 0;
}

void ecckd_aerosol_optics_destroy(ecckd_aerosol_optics_t *ao) {
  if (!ao) return;
  if (ao->device >= 0 && ao->dbuf) {
    (void)hipSetDevice(ao->device);
    (void)hipFree(ao->dbuf);
  }
  delete ao;
}

int ecckd_aerosol_optics_get_nband(const ecckd_aerosol_optics_t *ao) { return ao ? ao->nband : 0; }
int ecckd_aerosol_optics_get_nbin(const ecckd_aerosol_optics_t *ao) { return ao ? ao->nbin : 0; }
int ecckd_aerosol_optics_get_nrh(const ecckd_aerosol_optics_t *ao) { return ao ? ao->nrh : 0; }

static int aerosol_optics_impl(bool f32, const ecckd_aerosol_optics_t *ao, int ncol, int nlay, int nspec, const int *aero_type,
                               const double *aero_size, const double *aero_mass, const double *relhum, int accumulate, double *tau,
                               double *ssa, double *g, int memspace, void *stream) {
  if (!ao) return fail("ecckd_aerosol_optics: null aerosol-optics object");
  if (nspec < 1) return fail("ecckd_aerosol_optics: nspec must be at least 1");
  if ((ssa == nullptr) != (g == nullptr))
    return fail("ecckd_aerosol_optics: ssa without g or g without ssa (pass both: two-stream, or neither: one-scalar)");
  if (check_dims(ncol, nlay)) return 1;
  if (!aero_type || !aero_size || !aero_mass || !relhum || !tau)
    return fail("ecckd_aerosol_optics: null argument (aero_type, aero_size, aero_mass, relhum and tau are required)");
  if (accumulate != 0 && accumulate != 1) return fail("ecckd_aerosol_optics: accumulate must be 0 or 1");
  if (memspace != ECCKD_DEVICE && memspace != ECCKD_HOST && memspace != ECCKD_MIXED) return fail("ecckd: bad memspace");
  const size_t n2 = (size_t)ncol * nlay, ns = n2 * nspec, n3 = n2 * ao->nband;
  if (memspace != ECCKD_DEVICE) {   // (host inputs; device inputs are not checked: the call stays asynchronous)
    const char *bad = f32 ? aerosol_optics_check_host(*ao, n2, nspec, aero_type, reinterpret_cast<const float *>(aero_size),
                                                      reinterpret_cast<const float *>(aero_mass), reinterpret_cast<const float *>(relhum))
                          : aerosol_optics_check_host(*ao, n2, nspec, aero_type, aero_size, aero_mass, relhum);
    if (bad) return fail(bad);
  }
  if (ao->device < 0)
    return fail("ecckd_aerosol_optics: host-only object (device -1): no GPU, no compute (there is no CPU fallback)");
  if (check_device(ao->device)) return 1;
  if (ncol == 0) return 0;
  ecckd::AerosolOpticsArgs a{};
  a.ncol = ncol; a.nlay = nlay; a.nband = ao->nband; a.nspec = nspec; a.f32 = f32; a.accumulate = accumulate;
  a.cus = simd_slots(ao->device) / 4;
  a.nbin = ao->nbin; a.nrh = ao->nrh;
  a.head = ao->dbuf + ao->off_head[f32];
  a.image = ao->dbuf + ao->off_image[f32];
  Stage st(ao->device, memspace, stream, f32);
  if (st.open([&] {
        a.type = st.in(aero_type, ns); a.size = st.in(aero_size, ns); a.mass = st.in(aero_mass, ns); a.relhum = st.in(relhum, n2);
        if (accumulate) {
          a.tau = st.inout_big(tau, n3); a.ssa = st.inout_big(ssa, n3); a.g = st.inout_big(g, n3);
        } else {
          a.tau = st.out(tau, n3, kBig); a.ssa = st.out(ssa, n3, kBig); a.g = st.out(g, n3, kBig);
        }
      }))
    return 1;
  {
    ProfScope prof("aerosol_optics", st.stream);
    HIPCHK(ecckd::launch_aerosol_optics(a, st.stream));
  }
  return st.close();
}

int ecckd_aerosol_optics(const ecckd_aerosol_optics_t *ao, int ncol, int nlay, int nspec, const int *aero_type,
                         const double *aero_size, const double *aero_mass, const double *relhum, int accumulate, double *tau,
                         double *ssa, double *g, int memspace, void *stream) {
  return aerosol_optics_impl(false, ao, ncol, nlay, nspec, aero_type, aero_size, aero_mass, relhum, accumulate, tau, ssa, g,
                             memspace, stream);
}
int ecckd_aerosol_optics_f32(const ecckd_aerosol_optics_t *ao, int ncol, int nlay, int nspec, const int *aero_type,
                             const float *aero_size, const float *aero_mass, const float *relhum, int accumulate, float *tau,
                             float *ssa, float *g, int memspace, void *stream) {
  return aerosol_optics_impl(true, ao, ncol, nlay, nspec, aero_type, dp(aero_size), dp(aero_mass), dp(relhum), accumulate,
                             dp(tau), dp(ssa), dp(g), memspace, stream);
}

// ---- heating rates (kernels_heating_rate.hip): flux divergence to K s-1 ----

static int heating_rate_impl(bool f32, int device, int ncol, int nlay, int nouter, const double *flux_up, const double *flux_dn,
                             const double *plev, double grav, double cp_dry, const double *cp, double *heating_rate, int memspace,
                             void *stream) {
  if (ncol < 1 || nlay < 1 || nouter < 1) return fail("ecckd_heating_rate: ncol, nlay and nouter must be at least 1");
  if (!flux_up || !flux_dn || !plev || !heating_rate)
    return fail("ecckd_heating_rate: null argument (flux_up, flux_dn, plev and heating_rate are required)");
  if (!(std::isfinite(grav) && grav > 0.)) return fail("ecckd_heating_rate: grav must be finite and positive");
  if (!cp && !(std::isfinite(cp_dry) && cp_dry > 0.))
    return fail("ecckd_heating_rate: cp_dry must be finite and positive (or pass cp per cell)");
  if (memspace != ECCKD_DEVICE && memspace != ECCKD_HOST && memspace != ECCKD_MIXED) return fail("ecckd: bad memspace");
  if (check_device(device)) return 1;
  const size_t lev = (size_t)ncol * ((size_t)nlay + 1), lay = (size_t)ncol * nlay;
  ecckd::HeatingRateArgs a{};
  a.ncol = ncol; a.nlay = nlay; a.nouter = nouter; a.f32 = f32;
  a.cus = simd_slots(device) / 4;
  if (f32) {   // the constants rounded to float once
    a.grav = (float)grav; a.cp_dry = (float)cp_dry;
  } else {
    a.grav = grav; a.cp_dry = cp_dry;
  }
  Stage st(device, memspace, stream, f32);
  if (st.open([&] {
        a.flux_up = st.in(flux_up, lev * nouter); a.flux_dn = st.in(flux_dn, lev * nouter); a.plev = st.in(plev, lev);
        a.cp = st.in(cp, lay);
        a.heating_rate = st.out(heating_rate, lay * nouter, kBig);
      }))
    return 1;
  {
    ProfScope prof("heating_rate", st.stream);
    HIPCHK(ecckd::launch_heating_rate(a, st.stream));
  }
  return st.close();
}

int ecckd_heating_rate(int device, int ncol, int nlay, int nouter, const double *flux_up, const double *flux_dn,
                       const double *plev, double grav, double cp_dry, const double *cp, double *heating_rate, int memspace,
                       void *stream) {
  return heating_rate_impl(false, device, ncol, nlay, nouter, flux_up, flux_dn, plev, grav, cp_dry, cp, heating_rate, memspace,
                           stream);
}
int ecckd_heating_rate_f32(int device, int ncol, int nlay, int nouter, const float *flux_up, const float *flux_dn,
                           const float *plev, double grav, double cp_dry, const float *cp, float *heating_rate, int memspace,
                           void *stream) {
  return heating_rate_impl(true, device, ncol, nlay, nouter, dp(flux_up), dp(flux_dn), dp(plev), grav, cp_dry, dp(cp),
                           dp(heating_rate), memspace, stream);
}

// ---- McICA cloud sampling (kernels_cloud_sampling.hip) ----

int ecckd_cloud_mask_sample(int device, int ncol, int nlay, int ngpt, int overlap, const double *cloud_frac,
                            const double *overlap_param, unsigned long long seed, long long col0, unsigned long long *mask,
                            int memspace, void *stream) {
  if (ngpt > 64) return fail("ecckd_cloud_mask_sample" + std::string(kMaskTooWide) + std::to_string(ngpt));
  if (ngpt < 1) return fail("ecckd_cloud_mask_sample: ngpt must be at least 1");
  if (overlap != ECCKD_OVERLAP_MAX_RAN && overlap != ECCKD_OVERLAP_EXP_RAN)
    return fail("ecckd_cloud_mask_sample: unknown overlap " + std::to_string(overlap) +
                " (ECCKD_OVERLAP_MAX_RAN = 0, ECCKD_OVERLAP_EXP_RAN = 1)");
  const bool exp_ran = overlap == ECCKD_OVERLAP_EXP_RAN;
  if (exp_ran && !overlap_param && nlay > 1) return fail("ecckd_cloud_mask_sample: ECCKD_OVERLAP_EXP_RAN needs overlap_param");
  if (check_dims(ncol, nlay)) return 1;
  if (!cloud_frac || !mask) return fail("ecckd_cloud_mask_sample: null argument (cloud_frac and mask are required)");
  if (memspace != ECCKD_DEVICE && memspace != ECCKD_HOST) return fail("ecckd: bad memspace");
  const size_t n2 = (size_t)ncol * nlay, np = exp_ran && nlay > 1 ? (size_t)ncol * (nlay - 1) : 0;
  if (memspace == ECCKD_HOST) {   // (a NaN fraction is a clear layer, a NaN parameter no correlation: neither is refused)
    for (size_t i = 0; i < n2; ++i)
      if (cloud_frac[i] < 0. || cloud_frac[i] > 1.) return fail("ecckd_cloud_mask_sample: cloud fraction outside [0, 1]");
    for (size_t i = 0; i < np; ++i)
      if (overlap_param[i] < 0. || overlap_param[i] > 1.) return fail("ecckd_cloud_mask_sample: overlap parameter outside [0, 1]");
  }
  if (check_device(device)) return 1;
  if (ncol == 0) return 0;
  Stage st(device, memspace, stream, false);
  const double *d_cf = nullptr, *d_al = nullptr;
  unsigned long long *d_mask = nullptr;
  if (st.open([&] { d_cf = st.in(cloud_frac, n2); d_al = st.in(np ? overlap_param : nullptr, np); d_mask = st.out(mask, n2); })) return 1;
  {
    ProfScope prof("cloud_mask_sample", st.stream);
    HIPCHK(ecckd::launch_cloud_mask_sample(ncol, nlay, ngpt, exp_ran, d_cf, d_al, seed, col0, d_mask, st.stream));
  }
  return st.close();
}

// ---- sampled optical-depth scaling (kernels_cloud_sampling.hip; include/ecckd_hip.h, "In-cloud water variability") ----

int ecckd_cloud_scaling_create(int device, int nfsd, double fsd0, double dfsd, int nq, const double *values,
                               ecckd_cloud_scaling_t **table) {
  if (!table) return fail("ecckd_cloud_scaling_create: null argument (the handle)");
  *table = nullptr;
  if (nfsd < 2) return fail("ecckd_cloud_scaling_create: nfsd must be at least 2 (the rows are interpolated)");
  if (nq < 1) return fail("ecckd_cloud_scaling_create: nq must be at least 1");
  if (!(dfsd > 0.) || !std::isfinite(dfsd) || !std::isfinite(fsd0))
    return fail("ecckd_cloud_scaling_create: dfsd must be greater than 0 (and fsd0 and dfsd finite)");
  if ((long long)nfsd * nq > (1ll << 24)) return fail("ecckd_cloud_scaling_create: at most 2^24 table entries");
  if (!values) return fail("ecckd_cloud_scaling_create: null argument (values)");
  const size_t n = (size_t)nfsd * nq;
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(values[i]) || values[i] < 0.)
      return fail("ecckd_cloud_scaling_create: a scaling must be finite and not negative (entry " + std::to_string(i) + ")");
  ecckd_cloud_scaling t;
  t.nfsd = nfsd; t.nq = nq; t.fsd0 = fsd0; t.dfsd = dfsd;
  t.values.assign(values, values + n);
  if (device != -1) {   // (-1: a host-only object: getters and refusals work, the sampler fails)
    if (check_device(device)) return 1;
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&t.dvalues), n * sizeof(double)));
    if (hipMemcpy(t.dvalues, values, n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(t.dvalues);
      return fail("ecckd_cloud_scaling_create: copying the table to the device failed");
    }
    t.device = device;
  }
  *table = new ecckd_cloud_scaling(std::move(t));
  return 0;
}

void ecckd_cloud_scaling_destroy(ecckd_cloud_scaling_t *t) {
  if (!t) return;
  if (t->device >= 0 && t->dvalues) {
    (void)hipSetDevice(t->device);
    (void)hipFree(t->dvalues);
  }
  delete t;
}

int ecckd_cloud_scaling_get_nfsd(const ecckd_cloud_scaling_t *t) { return t ? t->nfsd : 0; }
int ecckd_cloud_scaling_get_nq(const ecckd_cloud_scaling_t *t) { return t ? t->nq : 0; }
double ecckd_cloud_scaling_get_fsd0(const ecckd_cloud_scaling_t *t) { return t ? t->fsd0 : 0.; }
double ecckd_cloud_scaling_get_dfsd(const ecckd_cloud_scaling_t *t) { return t ? t->dfsd : 0.; }
int ecckd_cloud_scaling_get_values(const ecckd_cloud_scaling_t *t, double *values) {
  if (!t || !values) return fail("ecckd_cloud_scaling_get_values: null argument");
  std::memcpy(values, t->values.data(), t->values.size() * sizeof(double));
  return 0;
}

// Phi(x) through erfc, and its inverse for 0 < p <= 1/2: Acklam's rational start (relative error 1.2e-9), then Halley
// steps on Phi(z) - p until the step is below an ulp of z
static double std_normal_cdf(double x) { return 0.5 * std::erfc(-x * 0.70710678118654752440); }
static double std_normal_quantile_lower(double p) {
  static const double a[6] = {-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02,
                              1.383577518672690e+02, -3.066479806614716e+01, 2.506628277459239e+00};
  static const double b[5] = {-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02,
                              6.680131188771972e+01, -1.328068155288572e+01};
  static const double c[6] = {-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00,
                              -2.549732539343734e+00, 4.374664141464968e+00, 2.938163982698783e+00};
  static const double d[4] = {7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00, 3.754408661907416e+00};
  double z;
  if (p < 0.02425) {
    const double q = std::sqrt(-2. * std::log(p));
    z = (((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) / ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1.);
  } else {
    const double q = p - 0.5, r = q * q;
    z = (((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * q /
        (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1.);
  }
  for (int it = 0; it < 4; ++it) {
    const double e = std_normal_cdf(z) - p;
    const double u = e * 2.50662827463100050242 * std::exp(0.5 * z * z);
    const double step = u / (1. + 0.5 * z * u);
    z -= step;
    if (std::fabs(step) <= 1e-16 * std::fabs(z)) break;
  }
  return z;
}

int ecckd_cloud_scaling_lognormal(int nfsd, double fsd0, double dfsd, int nq, double *values) {
  if (nfsd < 1) return fail("ecckd_cloud_scaling_lognormal: nfsd must be at least 1");
  if (nq < 1) return fail("ecckd_cloud_scaling_lognormal: nq must be at least 1");
  if (!(fsd0 >= 0.) || !(dfsd > 0.) || !std::isfinite(fsd0) || !std::isfinite(dfsd))
    return fail("ecckd_cloud_scaling_lognormal: fsd0 must not be negative and dfsd must be greater than 0 (both finite)");
  if (!values) return fail("ecckd_cloud_scaling_lognormal: null argument (values)");
  // the bin edges z_j = Phi^-1(j / nq), j = 1 .. nq-1: the lower half solved, the upper half its mirror image
  std::vector<double> z((size_t)nq + 1, 0.);
  for (int j = 1; j < nq; ++j) {
    if (2 * j < nq) z[j] = std_normal_quantile_lower((double)j / (double)nq);
    else if (2 * j == nq) z[j] = 0.;
    else z[j] = -std_normal_quantile_lower((double)(nq - j) / (double)nq);
  }
  for (int k = 0; k < nfsd; ++k) {
    const double f = fsd0 + k * dfsd;
    double *row = values + (size_t)k * nq;
    if (f == 0.) {
      for (int j = 0; j < nq; ++j) row[j] = 1.;
      continue;
    }
    const double sigma = std::sqrt(std::log(1. + f * f));
    double below = 0.;   // Phi(z_j - sigma); z_0 = -inf
    for (int j = 0; j < nq; ++j) {
      const double above = j + 1 < nq ? std_normal_cdf(z[j + 1] - sigma) : 1.;
      row[j] = (double)nq * (above - below);
      below = above;
    }
  }
  return 0;
}

int ecckd_cloud_scaling_sample(int device, int ncol, int nlay, int ngpt, int overlap, const double *cloud_frac,
                               const double *overlap_param, const double *fsd, double fsd_const,
                               const ecckd_cloud_scaling_t *table, unsigned long long seed, long long col0, float *scaling,
                               unsigned long long *mask, int memspace, void *stream) {
  const std::string who = "ecckd_cloud_scaling_sample";
  if (ngpt > 64) return fail(who + ": the ranks of at most 64 g-points are held at once, not " + std::to_string(ngpt));
  if (ngpt < 1) return fail(who + ": ngpt must be at least 1");
  if (overlap != ECCKD_OVERLAP_MAX_RAN && overlap != ECCKD_OVERLAP_EXP_RAN)
    return fail(who + ": unknown overlap " + std::to_string(overlap) + " (ECCKD_OVERLAP_MAX_RAN = 0, ECCKD_OVERLAP_EXP_RAN = 1)");
  const bool exp_ran = overlap == ECCKD_OVERLAP_EXP_RAN;
  if (exp_ran && !overlap_param && nlay > 1) return fail(who + ": ECCKD_OVERLAP_EXP_RAN needs overlap_param");
  if (check_dims(ncol, nlay)) return 1;
  if (!cloud_frac || !scaling) return fail(who + ": null argument (cloud_frac and scaling are required)");
  if (!table) return fail(who + ": null argument (the scaling table)");
  if (memspace != ECCKD_DEVICE && memspace != ECCKD_HOST) return fail("ecckd: bad memspace");
  const size_t n2 = (size_t)ncol * nlay, np = exp_ran && nlay > 1 ? (size_t)ncol * (nlay - 1) : 0;
  if (memspace == ECCKD_HOST) {   // (as ecckd_cloud_mask_sample; fsd is not checked: every value has a meaning)
    for (size_t i = 0; i < n2; ++i)
      if (cloud_frac[i] < 0. || cloud_frac[i] > 1.) return fail(who + ": cloud fraction outside [0, 1]");
    for (size_t i = 0; i < np; ++i)
      if (overlap_param[i] < 0. || overlap_param[i] > 1.) return fail(who + ": overlap parameter outside [0, 1]");
  }
  if (table->device < 0) return fail(who + ": host-only scaling table (device -1): no GPU, no compute (there is no CPU fallback)");
  if (table->device != device) return fail(who + ": the scaling table lives on device " + std::to_string(table->device) + ", not " + std::to_string(device));
  if (check_device(device)) return 1;
  if (ncol == 0) return 0;
  Stage st(device, memspace, stream, false);
  ecckd::CloudScalingArgs a{};
  a.ncol = ncol; a.nlay = nlay; a.ngpt = ngpt; a.exp_ran = exp_ran ? 1 : 0;
  a.fsd_const = fsd_const; a.nfsd = table->nfsd; a.nq = table->nq; a.fsd0 = table->fsd0; a.dfsd = table->dfsd;
  a.values = table->dvalues; a.seed = seed; a.col0 = col0;
  if (st.open([&] {
        a.cloud_frac = st.in(cloud_frac, n2); a.overlap_param = st.in(np ? overlap_param : nullptr, np); a.fsd = st.in(fsd, n2);
        a.scaling = static_cast<float *>(st.out_bytes(scaling, n2 * (size_t)ngpt * sizeof(float))); a.mask = st.out(mask, n2);
      }))
    return 1;
  {
    ProfScope prof("cloud_scaling_sample", st.stream);
    HIPCHK(ecckd::launch_cloud_scaling_sample(a, st.stream));
  }
  return st.close();
}

size_t ecckd_lw_flux_scaled_scratch_bytes(const ecckd_model_t *m, int ncol, int nlay) {
  if (!m || ncol <= 0 || nlay <= 0) return 0;
  return ((size_t)ncol * nlay * m->ng + 32 + fused_scratch_doubles(m, ncol, nlay)) * sizeof(double);
}

size_t ecckd_sw_flux_scaled_scratch_bytes(const ecckd_model_t *m, int ncol, int nlay, int delta_scale) {
  if (!m || ncol <= 0 || nlay <= 0) return 0;
  return SwWork(m, false, ncol, nlay, delta_scale != 0, true).bytes();
}

int ecckd_lw_flux_scaled(const ecckd_model_t *m, int ncol, int nlay, const double *plev, const double *tlay, const double *tsfc,
                         const double *tlev, int ngas, const char *gas_names, const double *const *vmr,
                         const long long *vmr_col_stride, const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1,
                         int n_gauss_angles, const double *sfc_emis, const double *inc_flux, int nband_p, const double *tau_p,
                         const double *ssa_p, const float *cloud_scaling, double *flux_up, double *flux_dn, int memspace,
                         void *stream) {
  // (the refusal list of the unmasked all-sky call, in its order; a null scaling is that call)
  const LwColumns c{ncol, nlay, plev, tlay, tsfc, tlev, GasDesc{ngas, gas_names, vmr, vmr_col_stride, vmr_lay_stride, vmr_scalar},
                    top_at_1, n_gauss_angles, sfc_emis, inc_flux};
  LwParticles pt;
  pt.tau = tau_p; pt.ssa = ssa_p; pt.scaling = cloud_scaling;
  const FluxOutputs o{Fluxes{flux_up, flux_dn}};
  return lw_fluxes_impl(&kLwAllsky, false, m, c, nband_p, pt, o, memspace, stream);
}

int ecckd_sw_flux_scaled(const ecckd_model_t *m, int ncol, int nlay, const double *plev, const double *tlay, int ngas,
                         const char *gas_names, const double *const *vmr, const long long *vmr_col_stride,
                         const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1, const double *mu0,
                         const double *toa_scale, const double *sfc_alb_dir, const double *sfc_alb_dif, int nband_p,
                         const double *tau_p, const double *ssa_p, const double *g_p, int delta_scale, const float *cloud_scaling,
                         double *flux_up, double *flux_dn, double *flux_dir, int memspace, void *stream) {
  const SwColumns c{ncol, nlay, plev, tlay, GasDesc{ngas, gas_names, vmr, vmr_col_stride, vmr_lay_stride, vmr_scalar}, top_at_1,
                    mu0, toa_scale, sfc_alb_dir, sfc_alb_dif};
  return sw_fluxes_impl(&kSwAllsky, false, m, c, nband_p, SwParticles{tau_p, ssa_p, g_p, delta_scale, nullptr, cloud_scaling},
                        FluxOutputs{Fluxes{flux_up, flux_dn, flux_dir}}, memspace, stream);
}

int ecckd_sw_fluxes_f32(const ecckd_model_t *m, int ncol, int nlay, const float *plev, const float *tlay, int ngas,
                        const char *gas_names, const float *const *vmr, const long long *vmr_col_stride,
                        const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1, const float *mu0,
                        const float *toa_scale, const float *sfc_alb_dir, const float *sfc_alb_dif, float *flux_up,
                        float *flux_dn, float *flux_dir, int memspace, void *stream) {
  const SwColumns c{ncol, nlay, dp(plev), dp(tlay), GasDesc{ngas, gas_names, dp(vmr), vmr_col_stride, vmr_lay_stride, vmr_scalar},
                    top_at_1, dp(mu0), dp(toa_scale), dp(sfc_alb_dir), dp(sfc_alb_dif)};
  const FluxOutputs o{Fluxes{dp(flux_up), dp(flux_dn), dp(flux_dir)}};
  return sw_fluxes_impl(nullptr, true, m, c, 0, SwParticles{}, o, memspace, stream);
}

// ---- single-precision fused fluxes: longwave, all-sky, McICA, both skies (the *_impl functions with f32 = true) ----

size_t ecckd_lw_fluxes_f32_scratch_bytes(const ecckd_model_t *m, int ncol, int nlay) {
  if (!m || ncol <= 0 || nlay <= 0) return 0;
  return lw_work_f32(m, ncol, nlay).bytes();
}

size_t ecckd_sw_fluxes_allsky_f32_scratch_bytes(const ecckd_model_t *m, int ncol, int nlay, int delta_scale) {
  if (!m || ncol <= 0 || nlay <= 0) return 0;
  return SwWork(m, true, ncol, nlay, delta_scale != 0).bytes();
}

int ecckd_lw_fluxes_f32(const ecckd_model_t *m, int ncol, int nlay, const float *plev, const float *tlay, const float *tsfc,
                        const float *tlev, int ngas, const char *gas_names, const float *const *vmr,
                        const long long *vmr_col_stride, const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1,
                        int n_gauss_angles, const float *sfc_emis, const float *inc_flux, float *flux_up, float *flux_dn,
                        int memspace, void *stream) {
  const LwColumns c{ncol, nlay, dp(plev), dp(tlay), dp(tsfc), dp(tlev),
                    GasDesc{ngas, gas_names, dp(vmr), vmr_col_stride, vmr_lay_stride, vmr_scalar}, top_at_1, n_gauss_angles,
                    dp(sfc_emis), dp(inc_flux)};
  const FluxOutputs o{Fluxes{dp(flux_up), dp(flux_dn)}};
  return lw_fluxes_impl(nullptr, true, m, c, 0, LwParticles{}, o, memspace, stream);
}

int ecckd_lw_fluxes_allsky_f32(const ecckd_model_t *m, int ncol, int nlay, const float *plev, const float *tlay, const float *tsfc,
                               const float *tlev, int ngas, const char *gas_names, const float *const *vmr,
                               const long long *vmr_col_stride, const long long *vmr_lay_stride, const double *vmr_scalar,
                               int top_at_1, int n_gauss_angles, const float *sfc_emis, const float *inc_flux, int nband_p,
                               const float *tau_p, const float *ssa_p, float *flux_up, float *flux_dn, int memspace, void *stream) {
  const LwColumns c{ncol, nlay, dp(plev), dp(tlay), dp(tsfc), dp(tlev),
                    GasDesc{ngas, gas_names, dp(vmr), vmr_col_stride, vmr_lay_stride, vmr_scalar}, top_at_1, n_gauss_angles,
                    dp(sfc_emis), dp(inc_flux)};
  LwParticles pt;
  pt.tau = dp(tau_p); pt.ssa = dp(ssa_p);
  const FluxOutputs o{Fluxes{dp(flux_up), dp(flux_dn)}};
  return lw_fluxes_impl(&kLwAllsky, true, m, c, nband_p, pt, o, memspace, stream);
}

int ecckd_lw_fluxes_allsky_mcica_f32(const ecckd_model_t *m, int ncol, int nlay, const float *plev, const float *tlay,
                                     const float *tsfc, const float *tlev, int ngas, const char *gas_names,
                                     const float *const *vmr, const long long *vmr_col_stride, const long long *vmr_lay_stride,
                                     const double *vmr_scalar, int top_at_1, int n_gauss_angles, const float *sfc_emis,
                                     const float *inc_flux, int nband_p, const float *tau_p, const float *ssa_p,
                                     const unsigned long long *cloud_mask, float *flux_up, float *flux_dn, int memspace,
                                     void *stream) {
  const LwColumns c{ncol, nlay, dp(plev), dp(tlay), dp(tsfc), dp(tlev),
                    GasDesc{ngas, gas_names, dp(vmr), vmr_col_stride, vmr_lay_stride, vmr_scalar}, top_at_1, n_gauss_angles,
                    dp(sfc_emis), dp(inc_flux)};
  return lw_fluxes_impl(&kLwAllsky, true, m, c, nband_p, LwParticles{dp(tau_p), dp(ssa_p), nullptr, cloud_mask},
                        FluxOutputs{Fluxes{dp(flux_up), dp(flux_dn)}}, memspace, stream);
}

int ecckd_lw_fluxes_clear_allsky_f32(const ecckd_model_t *m, int ncol, int nlay, const float *plev, const float *tlay,
                                     const float *tsfc, const float *tlev, int ngas, const char *gas_names,
                                     const float *const *vmr, const long long *vmr_col_stride, const long long *vmr_lay_stride,
                                     const double *vmr_scalar, int top_at_1, int n_gauss_angles, const float *sfc_emis,
                                     const float *inc_flux, int nband_p, const float *tau_p, const float *ssa_p,
                                     const unsigned long long *cloud_mask, float *flux_up, float *flux_dn, float *flux_up_clear,
                                     float *flux_dn_clear, int memspace, void *stream) {
  const LwColumns c{ncol, nlay, dp(plev), dp(tlay), dp(tsfc), dp(tlev),
                    GasDesc{ngas, gas_names, dp(vmr), vmr_col_stride, vmr_lay_stride, vmr_scalar}, top_at_1, n_gauss_angles,
                    dp(sfc_emis), dp(inc_flux)};
  const LwParticles pt{dp(tau_p), dp(ssa_p), nullptr, cloud_mask};
  const FluxOutputs o{Fluxes{dp(flux_up), dp(flux_dn)}, Fluxes{dp(flux_up_clear), dp(flux_dn_clear)}};
  return lw_fluxes_impl(&kLwClearAllsky, true, m, c, nband_p, pt, o, memspace, stream);
}

int ecckd_sw_fluxes_allsky_f32(const ecckd_model_t *m, int ncol, int nlay, const float *plev, const float *tlay, int ngas,
                               const char *gas_names, const float *const *vmr, const long long *vmr_col_stride,
                               const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1, const float *mu0,
                               const float *toa_scale, const float *sfc_alb_dir, const float *sfc_alb_dif, int nband_p,
                               const float *tau_p, const float *ssa_p, const float *g_p, int delta_scale, float *flux_up,
                               float *flux_dn, float *flux_dir, int memspace, void *stream) {
  const SwColumns c{ncol, nlay, dp(plev), dp(tlay), GasDesc{ngas, gas_names, dp(vmr), vmr_col_stride, vmr_lay_stride, vmr_scalar},
                    top_at_1, dp(mu0), dp(toa_scale), dp(sfc_alb_dir), dp(sfc_alb_dif)};
  return sw_fluxes_impl(&kSwAllsky, true, m, c, nband_p, SwParticles{dp(tau_p), dp(ssa_p), dp(g_p), delta_scale},
                        FluxOutputs{Fluxes{dp(flux_up), dp(flux_dn), dp(flux_dir)}}, memspace, stream);
}

int ecckd_sw_fluxes_allsky_mcica_f32(const ecckd_model_t *m, int ncol, int nlay, const float *plev, const float *tlay, int ngas,
                                     const char *gas_names, const float *const *vmr, const long long *vmr_col_stride,
                                     const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1, const float *mu0,
                                     const float *toa_scale, const float *sfc_alb_dir, const float *sfc_alb_dif, int nband_p,
                                     const float *tau_p, const float *ssa_p, const float *g_p, int delta_scale,
                                     const unsigned long long *cloud_mask, float *flux_up, float *flux_dn, float *flux_dir,
                                     int memspace, void *stream) {
  const SwColumns c{ncol, nlay, dp(plev), dp(tlay), GasDesc{ngas, gas_names, dp(vmr), vmr_col_stride, vmr_lay_stride, vmr_scalar},
                    top_at_1, dp(mu0), dp(toa_scale), dp(sfc_alb_dir), dp(sfc_alb_dif)};
  return sw_fluxes_impl(&kSwAllsky, true, m, c, nband_p, SwParticles{dp(tau_p), dp(ssa_p), dp(g_p), delta_scale, cloud_mask},
                        FluxOutputs{Fluxes{dp(flux_up), dp(flux_dn), dp(flux_dir)}}, memspace, stream);
}

int ecckd_sw_fluxes_clear_allsky_f32(const ecckd_model_t *m, int ncol, int nlay, const float *plev, const float *tlay, int ngas,
                                     const char *gas_names, const float *const *vmr, const long long *vmr_col_stride,
                                     const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1, const float *mu0,
                                     const float *toa_scale, const float *sfc_alb_dir, const float *sfc_alb_dif, int nband_p,
                                     const float *tau_p, const float *ssa_p, const float *g_p, int delta_scale,
                                     const unsigned long long *cloud_mask, float *flux_up, float *flux_dn, float *flux_dir,
                                     float *flux_up_clear, float *flux_dn_clear, float *flux_dir_clear, int memspace,
                                     void *stream) {
  const SwColumns c{ncol, nlay, dp(plev), dp(tlay), GasDesc{ngas, gas_names, dp(vmr), vmr_col_stride, vmr_lay_stride, vmr_scalar},
                    top_at_1, dp(mu0), dp(toa_scale), dp(sfc_alb_dir), dp(sfc_alb_dif)};
  const SwParticles pt{dp(tau_p), dp(ssa_p), dp(g_p), delta_scale, cloud_mask};
  const FluxOutputs o{Fluxes{dp(flux_up), dp(flux_dn), dp(flux_dir)}, Fluxes{dp(flux_up_clear), dp(flux_dn_clear), dp(flux_dir_clear)}};
  return sw_fluxes_impl(&kSwClearAllsky, true, m, c, nband_p, pt, o, memspace, stream);
}

// ---- spectral (per-band) fluxes: ty_fluxes_byband of RTE-RRTMGP ----

// One solver pass per band over its (contiguous) g-points, each told its band (Call::band) instead of a band2gpt map
static int rte_lw_byband_impl(bool f32, int device, int ncol, int nlay, int ngpt, int top_at_1, int n_gauss_angles,
                              const double *tau, const double *lay_source, const double *lev_source_inc,
                              const double *lev_source_dec, const double *sfc_source, int nband, const int *band2gpt,
                              const double *sfc_emis, double *bnd_flux_up, double *bnd_flux_dn, double *flux_up,
                              double *flux_dn, int memspace, void *stream) {
  if (check_dims(ncol, nlay)) return 1;
  unsigned char map[256];
  if (fill_band_map(ngpt, nband, band2gpt, map)) return 1;
  if (!bnd_flux_up || !bnd_flux_dn) return fail("ecckd_rte_lw_byband: null argument");
  const size_t n3 = (size_t)ncol * nlay, n2l = (size_t)ncol * (nlay + 1);
  // (one level buffer: a band's sub-range of the two views is still the pair of views, at the buffer's g-plane stride)
  LevelPair lp;
  if (level_pair("ecckd_rte_lw_byband", lev_source_inc, lev_source_dec, ncol, nlay, f32, memspace, true, &lp)) return 1;
  const size_t nl3 = (size_t)lp.gstride;
  for (int b = 0; b < nband; ++b) {
    const int g0 = band2gpt[2 * b] - 1, n = band2gpt[2 * b + 1] - g0;
    if (rte_lw_impl(Call{f32, b}, device, ncol, nlay, n, top_at_1, n_gauss_angles, el(tau, n3 * g0, f32),
                    el(lay_source, n3 * g0, f32), el(lev_source_inc, nl3 * g0, f32), el(lev_source_dec, nl3 * g0, f32),
                    el(sfc_source, (size_t)ncol * g0, f32), nband, nullptr, sfc_emis, nullptr,
                    el(bnd_flux_up, n2l * b, f32), el(bnd_flux_dn, n2l * b, f32), memspace, stream))
      return 1;
  }
  if (ncol == 0) return 0;
  if (flux_up && sum_planes(bnd_flux_up, nband, n2l, flux_up, f32, memspace, stream)) return 1;
  if (flux_dn && sum_planes(bnd_flux_dn, nband, n2l, flux_dn, f32, memspace, stream)) return 1;
  return 0;
}

static int rte_sw_byband_impl(bool f32, int device, int ncol, int nlay, int ngpt, int top_at_1, const double *tau,
                              const double *ssa, const double *g, const double *mu0, const double *toa_flux, int nband,
                              const int *band2gpt, const double *sfc_alb_dir, const double *sfc_alb_dif,
                              double *bnd_flux_up, double *bnd_flux_dn, double *bnd_flux_dir, double *flux_up,
                              double *flux_dn, double *flux_dir, int memspace, void *stream) {
  if (check_dims(ncol, nlay)) return 1;
  unsigned char map[256];
  if (fill_band_map(ngpt, nband, band2gpt, map)) return 1;
  if (!bnd_flux_up || !bnd_flux_dn) return fail("ecckd_rte_sw_byband: null argument");
  if (flux_dir && !bnd_flux_dir) return fail("ecckd_rte_sw_byband: flux_dir needs bnd_flux_dir");
  const size_t n3 = (size_t)ncol * nlay, n2l = (size_t)ncol * (nlay + 1);
  for (int b = 0; b < nband; ++b) {
    const int g0 = band2gpt[2 * b] - 1, n = band2gpt[2 * b + 1] - g0;
    if (rte_sw_impl(Call{f32, b}, device, ncol, nlay, n, top_at_1, el(tau, n3 * g0, f32), el(ssa, n3 * g0, f32),
                    el(g, n3 * g0, f32), mu0, el(toa_flux, (size_t)ncol * g0, f32), nband, nullptr, sfc_alb_dir,
                    sfc_alb_dif, el(bnd_flux_up, n2l * b, f32), el(bnd_flux_dn, n2l * b, f32),
                    bnd_flux_dir ? el(bnd_flux_dir, n2l * b, f32) : nullptr, memspace, stream))
      return 1;
  }
  if (ncol == 0) return 0;
  if (flux_up && sum_planes(bnd_flux_up, nband, n2l, flux_up, f32, memspace, stream)) return 1;
  if (flux_dn && sum_planes(bnd_flux_dn, nband, n2l, flux_dn, f32, memspace, stream)) return 1;
  if (flux_dir && sum_planes(bnd_flux_dir, nband, n2l, flux_dir, f32, memspace, stream)) return 1;
  return 0;
}

int ecckd_rte_lw_byband(int device, int ncol, int nlay, int ngpt, int top_at_1, int n_gauss_angles,
                        const double *tau, const double *lay_source, const double *lev_source_inc,
                        const double *lev_source_dec, const double *sfc_source, int nband, const int *band2gpt,
                        const double *sfc_emis, double *bnd_flux_up, double *bnd_flux_dn, double *flux_up,
                        double *flux_dn, int memspace, void *stream) {
  return rte_lw_byband_impl(false, device, ncol, nlay, ngpt, top_at_1, n_gauss_angles, tau, lay_source, lev_source_inc,
                            lev_source_dec, sfc_source, nband, band2gpt, sfc_emis, bnd_flux_up, bnd_flux_dn, flux_up,
                            flux_dn, memspace, stream);
}

int ecckd_rte_sw_byband(int device, int ncol, int nlay, int ngpt, int top_at_1, const double *tau,
                        const double *ssa, const double *g, const double *mu0, const double *toa_flux, int nband,
                        const int *band2gpt, const double *sfc_alb_dir, const double *sfc_alb_dif,
                        double *bnd_flux_up, double *bnd_flux_dn, double *bnd_flux_dir, double *flux_up,
                        double *flux_dn, double *flux_dir, int memspace, void *stream) {
  return rte_sw_byband_impl(false, device, ncol, nlay, ngpt, top_at_1, tau, ssa, g, mu0, toa_flux, nband, band2gpt,
                            sfc_alb_dir, sfc_alb_dif, bnd_flux_up, bnd_flux_dn, bnd_flux_dir, flux_up, flux_dn, flux_dir,
                            memspace, stream);
}

// Single-precision flavours of the per-band solvers (the reference is precision-generic through `wp`).
int ecckd_rte_lw_byband_f32(int device, int ncol, int nlay, int ngpt, int top_at_1, int n_gauss_angles, const float *tau,
                            const float *lay_source, const float *lev_source_inc, const float *lev_source_dec,
                            const float *sfc_source, int nband, const int *band2gpt, const float *sfc_emis,
                            float *bnd_flux_up, float *bnd_flux_dn, float *flux_up, float *flux_dn, int memspace, void *stream) {
  return rte_lw_byband_impl(true, device, ncol, nlay, ngpt, top_at_1, n_gauss_angles, dp(tau), dp(lay_source),
                            dp(lev_source_inc), dp(lev_source_dec), dp(sfc_source), nband, band2gpt, dp(sfc_emis),
                            dp(bnd_flux_up), dp(bnd_flux_dn), dp(flux_up), dp(flux_dn), memspace, stream);
}

int ecckd_rte_sw_byband_f32(int device, int ncol, int nlay, int ngpt, int top_at_1, const float *tau, const float *ssa,
                            const float *g, const float *mu0, const float *toa_flux, int nband, const int *band2gpt,
                            const float *sfc_alb_dir, const float *sfc_alb_dif, float *bnd_flux_up, float *bnd_flux_dn,
                            float *bnd_flux_dir, float *flux_up, float *flux_dn, float *flux_dir, int memspace, void *stream) {
  return rte_sw_byband_impl(true, device, ncol, nlay, ngpt, top_at_1, dp(tau), dp(ssa), dp(g), dp(mu0), dp(toa_flux), nband,
                            band2gpt, dp(sfc_alb_dir), dp(sfc_alb_dif), dp(bnd_flux_up), dp(bnd_flux_dn), dp(bnd_flux_dir),
                            dp(flux_up), dp(flux_dn), dp(flux_dir), memspace, stream);
}

// ---- per-band fluxes from the fused path (include/ecckd_hip.h, "Fused per-band fluxes") ----

size_t ecckd_lw_flux_bands_scratch_bytes(const ecckd_model_t *m, int ncol, int nlay) {
  if (!m || ncol <= 0 || nlay <= 0) return 0;
  return ((size_t)ncol * nlay * m->ng + 32 + fused_scratch_doubles(m, ncol, nlay)) * sizeof(double);
}

int ecckd_lw_flux_bands(const ecckd_model_t *m, int ncol, int nlay, const double *plev, const double *tlay, const double *tsfc,
                        const double *tlev, int ngas, const char *gas_names, const double *const *vmr,
                        const long long *vmr_col_stride, const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1,
                        int n_gauss_angles, const double *sfc_emis, const double *inc_flux, int nband_p, const double *tau_p,
                        const double *ssa_p, const unsigned long long *cloud_mask, double *bnd_flux_up, double *bnd_flux_dn,
                        double *flux_up, double *flux_dn, int memspace, void *stream) {
  const LwColumns c{ncol, nlay, plev, tlay, tsfc, tlev, GasDesc{ngas, gas_names, vmr, vmr_col_stride, vmr_lay_stride, vmr_scalar},
                    top_at_1, n_gauss_angles, sfc_emis, inc_flux};
  const LwParticles pt{tau_p, ssa_p, nullptr, cloud_mask};
  const FluxOutputs o{Fluxes{flux_up, flux_dn}, Fluxes{}, Fluxes{bnd_flux_up, bnd_flux_dn}};
  CallWords w;   // (the refusals in the order of the header; this call puts its name in front of every message)
  w.who = w.who_mask = "ecckd_lw_flux_bands";
  w.planes_tail = ": null argument (tau_p is required with nband_p > 0; ssa_p may be null: one-stream particles)";
  w.need_ssa_g = false;
  w.nband0_clear = true;
  w.tlev_text = "ecckd_lw_flux_bands: tlev is required for ecckd";
  unsigned short first[257];
  bool done;
  if (!m) return refuse(w.who, ": null model");
  if (lw_head(w, m, c, nband_p, pt) || gauss_refusals(c, w.who)) return 1;
  if (!bnd_flux_up || !bnd_flux_dn) return refuse(w.who, ": null argument (bnd_flux_up and bnd_flux_dn are required)");
  if (outputs_alias(w.who, {bnd_flux_up, bnd_flux_dn, flux_up, flux_dn})) return 1;
  if (bands_tail(w.who, m, ncol, nlay, c.null_array(), memspace, first, &done)) return 1;
  if (done) return 0;
  const Counts n(ncol, nlay, m->ng, m->nband);
  const bool fused = fused_lw_kernels_apply(m, nlay);
  const size_t extra = fused_scratch_doubles(m, ncol, nlay);
  Stage st(const_cast<ecckd_model *>(m), memspace, stream, false);
  LwColumns d{};
  LwParticles d_pt{};
  FluxOutputs d_o{};
  double *d_tau = nullptr;
  if (st.open([&] {
        d = c.staged(st, n);
        d_pt = pt.staged(st, n);
        d_o.bands = o.bands.staged(st, n.lev * m->nband);
        d_o.all = o.all.staged(st, n.lev);
        d_tau = st.work((n.lay_g + 32 + extra) * sizeof(double));
      }))
    return 1;
  double *const d_bup = d_o.bands.up, *const d_bdn = d_o.bands.dn;
  const hipStream_t s = st.stream;
  if (gas_optical_depth_dev(m, false, nullptr, ncol, nlay, d.plev, d.tlay, d.gas, d_tau, false, nullptr, nullptr, nullptr, nullptr, s)) return 1;
  ecckd::RteLwArgs a{};
  if (lw_solver_args(m, d, false, a)) return 1;
  a.tau = d_tau;
  if (fused) {
    // 60 layers: the Planck-recomputing layer-split solver in its band-window form, one launch for all bands
    a.use_split = 1;
    a.flux_up = d_bup; a.flux_dn = d_bdn;
    if (d_pt.tau) { a.part_tau = d_pt.tau; a.part_ssa = d_pt.ssa; a.part_1scl = d_pt.ssa ? 0 : 1; a.part_mask = d_pt.mask; }
    ProfScope prof("rte_lw_fused_bands", s);
    HIPCHK(ecckd::launch_rte_lw_planck_bands(a, m->dbuf + m->off_planck, m->ntp, m->temperature_planck[0],
                                             m->temperature_planck[1] - m->temperature_planck[0], d.tlay, d.tlev, d.tsfc, first, s));
  } else {
    // general route: Planck sources into scratch, the by-band (masked) increment in place on the scratch optical depth,
    // then the register-resident solver once per band on that band's planes of the same arrays (a launch of its own:
    // window = pointer + count, the band told to every g-point of the launch as ecckd_rte_lw_byband does)
    double *scratch = d_tau + r32(n.lay_g);
    double *lay = scratch, *inc = lay + n.lay_g, *dec = inc + n.lay_g, *sfc = dec + n.lay_g, *ring = sfc + r32(n.col_g);
    {
      ecckd::PlanckArgs p = planck_args(m, ncol, nlay, d.tlay, PlanckSide{d.tlev, d.tsfc, lay, inc, dec, sfc});
      ProfScope prof("planck", s);
      HIPCHK(ecckd::launch_planck(p, s));
    }
    if (d_pt.tau && lw_increment_dev(m, ncol, nlay, d_tau, d_pt, s)) return 1;
    a.use_split = 0;
    a.shared_levels = d.inc_flux ? 0 : 1;
    a.scratch = ecckd::rte_lw_scratch_bytes(ncol, nlay, m->ng) ? ring : nullptr;
    ProfScope prof("rte_lw_bands", s);
    for (int b = 0; b < m->nband; ++b) {
      const size_t g0 = first[b];
      ecckd::RteLwArgs w = a;
      std::memset(w.gpt2band, b, sizeof w.gpt2band);
      w.ng = first[b + 1] - first[b];
      w.tau = d_tau + n.lay * g0; w.lay_source = lay + n.lay * g0; w.lev_source_inc = inc + n.lay * g0;
      w.lev_source_dec = dec + n.lay * g0; w.sfc_source = sfc + n.col * g0;
      w.inc_flux = d.inc_flux ? d.inc_flux + n.col * g0 : nullptr;
      w.flux_up = d_bup + n.lev * b; w.flux_dn = d_bdn + n.lev * b;
      HIPCHK(ecckd::launch_rte_lw(w, s));
    }
  }
  if (d_o.all.up) HIPCHK(ecckd::launch_sum_planes(d_bup, m->nband, n.lev, d_o.all.up, 0, s));
  if (d_o.all.dn) HIPCHK(ecckd::launch_sum_planes(d_bdn, m->nband, n.lev, d_o.all.dn, 0, s));
  return st.close();
}

// The shortwave work block: that of ecckd_sw_fluxes_allsky for the shape, the solver's room sized for the widest need of a
// band's launch (the whole model's where that is larger: the solvers' plans are not monotonic in the g-point count)
struct SwBandsWork {
  size_t tau_bytes, solver, plane;
  SwBandsWork(const ecckd_model *m, int ncol, int nlay, bool scaled_planes) {
    const SwWork w(m, false, ncol, nlay, scaled_planes);
    tau_bytes = w.tau_bytes; solver = w.solver; plane = w.plane;
    for (int b = 0; b < m->nband; ++b) {
      const size_t need = sw_fluxes_solver_bytes(m->device, ncol, nlay, m->band2gpt[2 * b + 1] - m->band2gpt[2 * b] + 1);
      if (need > solver) solver = need;
    }
  }
  size_t bytes() const { return tau_bytes + solver + 3 * plane; }
};

size_t ecckd_sw_flux_bands_scratch_bytes(const ecckd_model_t *m, int ncol, int nlay, int delta_scale) {
  if (!m || ncol <= 0 || nlay <= 0) return 0;
  return SwBandsWork(m, ncol, nlay, delta_scale != 0).bytes();
}

int ecckd_sw_flux_bands(const ecckd_model_t *m, int ncol, int nlay, const double *plev, const double *tlay, int ngas,
                        const char *gas_names, const double *const *vmr, const long long *vmr_col_stride,
                        const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1, const double *mu0,
                        const double *toa_scale, const double *sfc_alb_dir, const double *sfc_alb_dif, int nband_p,
                        const double *tau_p, const double *ssa_p, const double *g_p, int delta_scale,
                        const unsigned long long *cloud_mask, double *bnd_flux_up, double *bnd_flux_dn, double *bnd_flux_dir,
                        double *flux_up, double *flux_dn, double *flux_dir, int memspace, void *stream) {
  const SwColumns c{ncol, nlay, plev, tlay, GasDesc{ngas, gas_names, vmr, vmr_col_stride, vmr_lay_stride, vmr_scalar}, top_at_1,
                    mu0, toa_scale, sfc_alb_dir, sfc_alb_dif};
  const SwParticles pt{tau_p, ssa_p, g_p, delta_scale, cloud_mask};
  const FluxOutputs o{Fluxes{flux_up, flux_dn, flux_dir}, Fluxes{}, Fluxes{bnd_flux_up, bnd_flux_dn, bnd_flux_dir}};
  CallWords w;   // (the refusals in the order of the header; this call puts its name in front of every message)
  w.who = w.who_mask = "ecckd_sw_flux_bands";
  w.planes_tail = ": null argument (tau_p, ssa_p and g_p are all required with nband_p > 0)";
  w.nband0_clear = true;
  unsigned short first[257];
  bool done;
  if (!m) return refuse(w.who, ": null model");
  if (sw_head(w, m, nband_p, pt, o)) return 1;
  if (!m->has_solar) return refuse(w.who, ": model has no solar table (longwave model?)");
  if (!bnd_flux_up || !bnd_flux_dn) return refuse(w.who, ": null argument (bnd_flux_up and bnd_flux_dn are required; bnd_flux_dir may be null)");
  if (flux_dir && !bnd_flux_dir) return refuse(w.who, ": flux_dir needs bnd_flux_dir");
  if (outputs_alias(w.who, {bnd_flux_up, bnd_flux_dn, bnd_flux_dir, flux_up, flux_dn, flux_dir})) return 1;
  if (bands_tail(w.who, m, ncol, nlay, c.null_array(), memspace, first, &done)) return 1;
  if (done) return 0;
  const Counts n(ncol, nlay, m->ng, m->nband);
  const bool part = nband_p != 0;
  const SwBandsWork work(m, ncol, nlay, part && delta_scale);
  Stage st(const_cast<ecckd_model *>(m), memspace, stream, false);
  SwColumns d{};
  SwParticles d_pt{};
  FluxOutputs d_o{};
  double *d_tau = nullptr;
  if (st.open([&] {
        d = c.staged(st, n);
        d_pt = pt.staged(st, n);
        d_o.bands = o.bands.staged(st, n.lev * m->nband);
        d_o.all = o.all.staged(st, n.lev);
        d_tau = st.work(work.bytes());
      }))
    return 1;
  const Fluxes &bnd = d_o.bands;
  const hipStream_t s = st.stream;
  char *const room = reinterpret_cast<char *>(d_tau) + work.tau_bytes;
  // the scaled copy of the band triple, as ecckd_sw_fluxes_allsky makes it
  if (work.plane && delta_scaled_copy(d_pt, n.lay_b, room + work.solver, work.plane, false, s)) return 1;
  if (gas_optical_depth_dev(m, false, nullptr, ncol, nlay, d.plev, d.tlay, d.gas, d_tau, true, nullptr, nullptr, nullptr, nullptr, s)) return 1;
  // One solver launch per band on that band's planes of the optical depth, with the band's entries of the Rayleigh and solar
  // tables: the solver ecckd_sw_fluxes_allsky takes for the shape, told its band as ecckd_rte_sw_byband tells it, and -- with
  // a mask -- in its band-window form, which reads the mask bit at the model's g-point (SwDerive::mask_first).
  for (int b = 0; b < m->nband; ++b) {
    const size_t g0 = first[b];
    const int count = first[b + 1] - first[b];
    SwDerive dv{d.plev, table(m, m->off_rayleigh, false) + g0, table(m, m->off_solar, false) + g0, d.toa_scale, gw(false),
                work.solver ? reinterpret_cast<double *>(room) : nullptr};
    if (part) { dv.part_tau = d_pt.tau; dv.part_ssa = d_pt.ssa; dv.part_g = d_pt.g; dv.part_mask = d_pt.mask; dv.mask_first = (int)g0; }
    if (rte_sw_impl(Call{false, b, false, &dv}, m->device, ncol, nlay, count, d.top_at_1, d_tau + n.lay * g0, nullptr, nullptr, d.mu0,
                    nullptr, m->nband, nullptr, d.sfc_alb_dir, d.sfc_alb_dif, bnd.up + n.lev * b, bnd.dn + n.lev * b,
                    bnd.dir ? bnd.dir + n.lev * b : nullptr, ECCKD_DEVICE, s))
      return 1;
  }
  if (d_o.all.up) HIPCHK(ecckd::launch_sum_planes(bnd.up, m->nband, n.lev, d_o.all.up, 0, s));
  if (d_o.all.dn) HIPCHK(ecckd::launch_sum_planes(bnd.dn, m->nband, n.lev, d_o.all.dn, 0, s));
  if (d_o.all.dir) HIPCHK(ecckd::launch_sum_planes(bnd.dir, m->nband, n.lev, d_o.all.dir, 0, s));
  return st.close();
}

}  // extern "C"
