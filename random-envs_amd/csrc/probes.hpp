// probes.hpp -- every profiling probe of the library: compile-time switches, storage, readers and the hooks the kernels and engines call.
//
// The product build defines none of the switches below and every hook is EMPTY there: a call site costs no instruction, no register and
// no #if in the code it sits in.  A probe build is the same sources with one or more of
//   -DREX_KTIME     cycles per phase of a forward evaluation, summed over the launch        (profiles/ktime_probe*.py)
//   -DREX_WAVETIME  cycles, event counts and placement of every WAVE of the last step launch (profiles/wavetime_probe*.py, waveplace_probe.py,
//                   slow_wave_phases.py); with the phase stamps of -DREX_PHASES unless -DREX_NOPHASES is given as well
//   -DREX_PHASES    cycles per phase of forward() and of the Newton iteration, per wave      (profiles/phase_probe.py)
//   -DREX_KSTATS    wave-level event counts of the planar solver, summed over the launch     (profiles/kstats_probe.py)
//   -DREX_MARKS     comment markers in the ISA of a -S build                                 (profiles/isa_regions.py)
//   -DREX_STATS     HOST builds of the planar engine: solver event counts of one lane        (profiles/wave_balance_host.cpp)
// loaded through REX_LIB.  The readers are extern "C" rex_debug_* functions that are not part of include/rex.h.
//
// Layout: slot names; for HIP translation units the storage with its readers -- defined by the ONE translation unit that sets
// REX_PROBES_STORAGE before its first include, declared everywhere else; the hook macros of the engine headers (host-clean: the engines are
// also compiled by a plain C++17 compiler); the hook macros of the step kernels.
#pragma once

#include "planar_spec.hpp"   // REX_WAVE_ANY

// ---- slot names -----------------------------------------------------------------------------------------------------------------------------
// humanoid, -DREX_KTIME: the per-lane accumulators Kin::tacc / PKin::tacc (HT_*: cycles, HC_*: counts); g_ktime[8 + slot]
enum { HT_SMOOTH = 0, HT_LIMITS, HT_BROAD, HT_NARROW_LOOP, HT_PAIR, HT_ROWS, HT_FACTOR, HT_BUILD_A, HT_SWEEPS, HT_QACC, HT_FORWARD,
       HC_EVALS, HC_PAIR_CALLS, HC_ROW_CALLS, HC_SWEEPS, HC_NEFC, HT_SLOTS };

namespace rex {

// planar solver event counts (REX_COUNT): g_kstats[slot] of -DREX_KSTATS, g_waveinfo[wave][slot] of -DREX_WAVETIME
// (slot 7: fastpath in g_kstats, selfpath in g_waveinfo)
enum { KS_solves = 0, KS_iters = 1, KS_pass1 = 2, KS_pass2 = 3, KS_ls_evals = 4, KS_nocon = 5, KS_slots_active = 6, KS_fastpath = 7, KS_selfpath = 7 };

// ---- storage (HIP translation units) ----------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#if defined(REX_PROBES_STORAGE)
#define REX_PROBE_VAR __device__
#else
#define REX_PROBE_VAR extern __device__
#endif
#if defined(REX_KTIME)
REX_PROBE_VAR unsigned long long g_ktime[24 + 72];   // 0..7 planar phases, 8..23 humanoid phases, [24 + lvl]: wave-evaluations per sweep level, [40 + lvl]: their sweep cycles, 72.. histogram of humanoid row counts
#endif
#if defined(REX_WAVETIME)
// cycles every wave of the last planar / humanoid step launch spent in its substeps (the kernel time at B = 32 768 is the SLOWEST wave's, not the average)
REX_PROBE_VAR unsigned long long g_wavetime[8192];
REX_PROBE_VAR unsigned long long g_waveinfo[8192][8];
REX_PROBE_VAR unsigned long long g_wavehum[1024][16];
REX_PROBE_VAR unsigned long long g_wavephase[8192][4];
REX_PROBE_VAR unsigned long long g_wavetail[8192][8];    // planar step kernel: what the tail of a wave (everything behind the substeps) spends where
REX_PROBE_VAR unsigned long long g_waveplace[8192][4];   // 100 MHz clock at entry and exit, HW_ID, XCC_ID: where and when each wave ran
#endif
#if defined(REX_WAVETIME) || defined(REX_PHASES)
REX_PROBE_VAR unsigned long long g_evalphase[8192][16];   // forward(): kinematics, mass+bias, detect, dispatch+self, rows+solve, pass 1, pass 2, H, ldl+solve, phi', update, correction
#endif
#if defined(REX_KSTATS)
REX_PROBE_VAR unsigned long long g_kstats[8];
#endif
#endif  // __HIPCC__

}  // namespace rex

// ---- readers: diagnostic builds only (not in rex.h) -------------------------------------------------------------------------------------------
#if defined(__HIPCC__) && defined(REX_PROBES_STORAGE)
#if defined(REX_KTIME)
extern "C" int rex_debug_ktime(unsigned long long* out) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(rex::g_ktime), sizeof(unsigned long long) * 96) != hipSuccess) return -1;
  unsigned long long z[96] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(rex::g_ktime), z, sizeof z); return 0; }
#endif
#if defined(REX_WAVETIME) || defined(REX_PHASES)
extern "C" int rex_debug_evalphase(unsigned long long* out, int n) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(rex::g_evalphase), sizeof(unsigned long long) * 16 * (n < 8192 ? n : 8192)) != hipSuccess) return -1;
  static unsigned long long z[8192][16]; return hipMemcpyToSymbol(HIP_SYMBOL(rex::g_evalphase), z, sizeof z) == hipSuccess ? 0 : -1; }
#endif
#if defined(REX_WAVETIME)
// g_wavephase: planar step kernel, cycles entry -> state loaded -> substeps done -> outputs stored -> fused reset done
extern "C" int rex_debug_wavephase(unsigned long long* out, int n) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(rex::g_wavephase), sizeof(unsigned long long) * 4 * (n < 8192 ? n : 8192)) == hipSuccess ? 0 : -1; }
// g_wavetail: cycles from the end of the substeps to [0] t and episode back from LDS, [1] reward / done / info stores issued; from there to [2] episode stored,
// [3] reset state and observation drawn, [4] xi draws done and stored, [5] end of the reset path (walker2d: the re-derive); the one set of
// state / obs stores follows.  [2..5] are maxima over the launches since the last read (zeroed here) and stay 0 for a wave that skipped the reset.
extern "C" int rex_debug_wavetail(unsigned long long* out, int n) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(rex::g_wavetail), sizeof(unsigned long long) * 8 * (n < 8192 ? n : 8192)) != hipSuccess) return -1;
  static unsigned long long z[8192][8]; return hipMemcpyToSymbol(HIP_SYMBOL(rex::g_wavetail), z, sizeof z) == hipSuccess ? 0 : -1; }
extern "C" int rex_debug_waveplace(unsigned long long* out, int n) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(rex::g_waveplace), sizeof(unsigned long long) * 4 * (n < 8192 ? n : 8192)) == hipSuccess ? 0 : -1; }
extern "C" int rex_debug_wavehum(unsigned long long* out) {   // humanoid: per-wave phase accumulators of the last launch (-DREX_KTIME -DREX_WAVETIME)
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(rex::g_wavehum), sizeof(unsigned long long) * 1024 * 16) == hipSuccess ? 0 : -1; }
extern "C" int rex_debug_waveinfo(unsigned long long* out, int n) {   // n waves x 8 counters, then zeroed
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(rex::g_waveinfo), sizeof(unsigned long long) * 8 * (n < 8192 ? n : 8192)) != hipSuccess) return -1;
  static unsigned long long z[8192][8]; return hipMemcpyToSymbol(HIP_SYMBOL(rex::g_waveinfo), z, sizeof z) == hipSuccess ? 0 : -1; }
extern "C" int rex_debug_wavetime(unsigned long long* out, int n) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(rex::g_wavetime), sizeof(unsigned long long) * (n < 8192 ? n : 8192)) == hipSuccess ? 0 : -1; }
#endif
#if defined(REX_KSTATS)
extern "C" int rex_debug_kstats(unsigned long long* out) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(rex::g_kstats), sizeof(unsigned long long) * 8) != hipSuccess) return -1;
  unsigned long long z[8] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(rex::g_kstats), z, sizeof z); return 0; }
#endif
#endif  // __HIPCC__ && REX_PROBES_STORAGE

// ---- hooks of the engine headers (host-clean) ---------------------------------------------------------------------------------------------------
// REX_MARK -- -DREX_MARKS: comment markers in the ISA (profiles/isa_regions.py counts the instructions between them)
#if defined(REX_MARKS) && defined(__HIP_DEVICE_COMPILE__)
#define REX_MARK(name) asm volatile("; REXMARK " name)
#else
#define REX_MARK(name) ((void)0)
#endif

// REX_PSTAMP / REX_PACC -- cycles per phase of forward(), summed per wave (lane 0) with fire-and-forget atomics.  The stamp
// takes a value the phase produced as an input, so that value is complete before the clock is read.
#if (defined(REX_WAVETIME) || defined(REX_PHASES)) && !defined(REX_NOPHASES) && defined(__HIP_DEVICE_COMPILE__)
#define REX_PSTAMP(var, dep) unsigned long long var; { float dep_ = (float)(dep); asm volatile("s_nop 0\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var) : "v"(dep_) : "memory"); }
#define REX_PACC(slot, t0, t1) do { if ((threadIdx.x & 63) == 0) atomicAdd(&g_evalphase[blockIdx.x & 8191][slot], (t1) - (t0)); } while (0)
#else
#define REX_PSTAMP(var, dep) ((void)0)
#define REX_PACC(slot, t0, t1) ((void)0)
#endif

// REX_COUNT -- planar solver event counts: one host lane (-DREX_STATS), wave-level over the launch (-DREX_KSTATS: lane 0 of each wave adds),
// or the same counts per WAVE (-DREX_WAVETIME: slot = workgroup index, next to the wave's cycle count)
#if defined(REX_STATS) && !defined(__HIP_DEVICE_COMPILE__)
namespace rex {
struct GlobalStats { long solves, iters, pass1, pass2, ls_evals, nocon, slots_active; long toggles[4][4]; int trace[64], ntrace; };   // trace: mode * 100 + Newton iterations of the last solves
inline GlobalStats& gstats() { static GlobalStats g{}; return g; }
}
#define REX_COUNT(field, n) (gstats().field += (n))
#elif defined(REX_KSTATS) && defined(__HIP_DEVICE_COMPILE__)
#define REX_COUNT(field, n) do { if ((threadIdx.x & 63) == 0) atomicAdd(&g_kstats[KS_##field], (unsigned long long)(n)); } while (0)
#define REX_KCOUNT(field, n) REX_COUNT(field, n)
#elif defined(REX_WAVETIME) && defined(__HIP_DEVICE_COMPILE__)
#define REX_COUNT(field, n) do { if ((threadIdx.x & 63) == 0) g_waveinfo[blockIdx.x & 8191][KS_##field] += (unsigned long long)(n); } while (0)
#define REX_WCOUNT(field, n) REX_COUNT(field, n)
#else
#define REX_COUNT(field, n) ((void)0)
#endif
#if !defined(REX_KCOUNT)
#define REX_KCOUNT(field, n) ((void)0)   // counted by -DREX_KSTATS only (fastpath: wave-solves on the feet-only path)
#endif
#if !defined(REX_WCOUNT)
#define REX_WCOUNT(field, n) ((void)0)   // counted by -DREX_WAVETIME only (selfpath: self-pair / general-path solves of the wave)
#endif
// one solve of forward(): -DREX_KSTATS counts the slots some lane of the WAVE has active, the other builds this lane's
#if defined(REX_KSTATS) && defined(__HIP_DEVICE_COMPILE__)
#define REX_COUNT_SOLVE(C, nslots) do { unsigned um = 0; for (int k = 0; k < (nslots); k++) if (REX_WAVE_ANY(((C).con_mask >> k) & 1u)) um |= 1u << k; \
    REX_COUNT(solves, 1); if (!REX_WAVE_ANY((C).any)) REX_COUNT(nocon, 1); REX_COUNT(slots_active, __popc(um)); } while (0)
#else
#define REX_COUNT_SOLVE(C, nslots) do { REX_COUNT(solves, 1); if (!(C).any) REX_COUNT(nocon, 1); REX_COUNT(slots_active, __builtin_popcount((C).con_mask)); } while (0)
#endif
// -DREX_STATS only: which groups toggled along a full Newton step ([limits][slots], 3 = three or more), corrections tried / accepted
// ([3][3] / [3][2]), and the (mode, iterations) trace of the last solves
#if defined(REX_STATS) && !defined(__HIP_DEVICE_COMPILE__)
#define REX_STAT_TOGGLES(lim_bits, slot_bits, full_step) do { const int nl = __builtin_popcount(lim_bits), ns = __builtin_popcount(slot_bits); \
    if (full_step) gstats().toggles[nl < 3 ? nl : 3][ns < 3 ? ns : 3]++; } while (0)
#define REX_STAT_CORRECTION(tried, accepted) do { if (tried) { gstats().toggles[3][3]++; if (accepted) gstats().toggles[3][2]++; } } while (0)
#define REX_STAT_TRACE(v) (gstats().trace[gstats().ntrace++ & 63] = (v))
#else
#define REX_STAT_TOGGLES(lim_bits, slot_bits, full_step) ((void)0)
#define REX_STAT_CORRECTION(tried, accepted) ((void)0)
#define REX_STAT_TRACE(v) ((void)0)
#endif

// REX_STAMP / REX_TACC / REX_TCNT -- -DREX_KTIME, planar: per-phase cycle stamps (s_memtime), summed per wave into g_ktime[]
#if defined(REX_KTIME) && defined(__HIP_DEVICE_COMPILE__)
#define REX_STAMP(var) unsigned long long var = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0)
#define REX_TACC(slot, t0, t1) do { if ((threadIdx.x & 63) == 0) atomicAdd(&g_ktime[slot], (t1) - (t0)); } while (0)
#define REX_TCNT(slot, n) do { if ((threadIdx.x & 63) == 0) atomicAdd(&g_ktime[slot], (unsigned long long)(n)); } while (0)
#else
#define REX_STAMP(var) ((void)0)
#define REX_TACC(slot, t0, t1) ((void)0)
#define REX_TCNT(slot, n) ((void)0)
#endif

// REX_HSTAMP / REX_HACC / REX_HCNT -- -DREX_KTIME, humanoid: s_memtime deltas summed in per-lane registers (Kin::tacc, declared by
// REX_HTACC_MEMBER) and flushed once per kernel by the caller (REX_HFLUSH: wave maximum per slot), so the probes do not perturb what they measure.
#if defined(REX_KTIME)
#define REX_HTACC_MEMBER unsigned long long tacc[HT_SLOTS];
#else
#define REX_HTACC_MEMBER
#endif
#if defined(REX_KTIME) && defined(__HIP_DEVICE_COMPILE__)
#define REX_HSTAMP(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#define REX_HACC(K, slot, t0, t1) ((K).tacc[slot] += (t1) - (t0))
#define REX_HCNT(K, slot, v) ((K).tacc[slot] += (unsigned long long)(v))
// the pair kernel's dual PGS by sweep level: g_ktime[24 + lvl] wave-evaluations, [40 + lvl] their sweep cycles, [56 + lvl] their build cycles,
// [72 + n]: wave-evaluations by their largest row count
#define REX_HSWEEP_LEVEL(lvl, n, p0, p1, p2) do { int nm = (n); for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(nm, off); nm = o > nm ? o : nm; } \
    if ((threadIdx.x & 63) == 0) { atomicAdd(&g_ktime[24 + (lvl)], 1ull); atomicAdd(&g_ktime[40 + (lvl)], (p2) - (p1)); atomicAdd(&g_ktime[56 + (lvl)], (p1) - (p0)); \
                                   atomicAdd(&g_ktime[72 + (nm < 23 ? nm : 23)], 1ull); } } while (0)
#else
#define REX_HSTAMP(var) ((void)0)
#define REX_HACC(K, slot, t0, t1) ((void)0)
#define REX_HCNT(K, slot, v) ((void)0)
#define REX_HSWEEP_LEVEL(lvl, n, p0, p1, p2) ((void)0)
#endif

// ---- hooks of the step kernels (HIP only) ---------------------------------------------------------------------------------------------------------
// Each macro names the stamps it declares or reads, so the flow of a stamp is visible at the call sites.
// planar_step_kernel: -DREX_WAVETIME fills g_wavetime / g_wavephase / g_wavetail / g_waveplace and slot 1 of g_waveinfo, -DREX_KTIME adds the
// substeps to g_ktime[5].  Humanoid step kernels: -DREX_WAVETIME the cycles of the wave's env_step (g_wavetime); -DREX_KTIME clears the lanes'
// accumulators (`K`: hum::Kin / hum::pr::PKin) and flushes them ONCE per wave and kernel -- the wave maximum of every accumulator, into
// g_ktime[8 + slot] and, with both switches, g_wavehum[wave][slot].
#if defined(REX_WAVETIME)
#define REX_WSTAMP(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#define REX_WCLOCK(var) const unsigned long long var = __builtin_amdgcn_s_memrealtime()
#define REX_WSTAMP_LDS(var) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); const unsigned long long var = __builtin_amdgcn_s_memtime()
#define REX_WSUBSTEPS(t0, t1) const unsigned long long t1 = __builtin_amdgcn_s_memtime(); if ((threadIdx.x & 63) == 0) g_wavetime[blockIdx.x & 8191] = t1 - (t0)
#define REX_WWAVE_DONE(t0) do { if ((threadIdx.x & 63) == 0) g_wavetime[blockIdx.x & 8191] = __builtin_amdgcn_s_memtime() - (t0); } while (0)
#define REX_WTAIL_MAX(slot, t0) atomicMax(&g_wavetail[blockIdx.x & 8191][slot], __builtin_amdgcn_s_memtime() - (t0))
#define REX_WSTEP_EXIT(tp0, tw0, tk0, tk1, tt0, tr0) do { \
  if ((threadIdx.x & 63) == 0) { g_waveinfo[blockIdx.x & 8191][1] += __builtin_amdgcn_s_memtime() - tr0; }   /* slot 1 ("iters", unused): cycles in the fused reset */ \
  if ((threadIdx.x & 63) == 0) { unsigned long long* ph = g_wavephase[blockIdx.x & 8191]; ph[0] = tk0 - tp0; ph[1] = tk1 - tk0; ph[2] = tr0 - tk1; ph[3] = __builtin_amdgcn_s_memtime() - tr0; } \
  if ((threadIdx.x & 63) == 0) { unsigned long long* tl = g_wavetail[blockIdx.x & 8191]; tl[0] = tt0 - tk1; tl[1] = tr0 - tk1; } \
  if ((threadIdx.x & 63) == 0) { unsigned long long* pl = g_waveplace[blockIdx.x & 8191]; pl[0] = tw0; pl[1] = __builtin_amdgcn_s_memrealtime(); \
    pl[2] = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4); pl[3] = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20); }   /* HW_REG_HW_ID, HW_REG_XCC_ID */ \
  } while (0)
#define REX_HFLUSH_WAVE(k, v) do { if ((threadIdx.x & 63) == 0 && k < 16) g_wavehum[blockIdx.x & 1023][k] = v; } while (0)
#else
#define REX_WSTAMP(var) ((void)0)
#define REX_WCLOCK(var) ((void)0)
#define REX_WSTAMP_LDS(var) ((void)0)
#define REX_WSUBSTEPS(t0, t1) ((void)0)
#define REX_WWAVE_DONE(t0) ((void)0)
#define REX_WTAIL_MAX(slot, t0) ((void)0)
#define REX_WSTEP_EXIT(tp0, tw0, tk0, tk1, tt0, tr0) ((void)0)
#define REX_HFLUSH_WAVE(k, v) ((void)0)
#endif
#if defined(REX_KTIME) || defined(REX_WAVETIME)
#define REX_KWSTAMP(var) unsigned long long var = __builtin_amdgcn_s_memtime()
#else
#define REX_KWSTAMP(var) ((void)0)
#endif
#if defined(REX_KTIME)
#define REX_KSUBSTEPS(t0) do { if ((threadIdx.x & 63) == 0) atomicAdd(&g_ktime[5], __builtin_amdgcn_s_memtime() - (t0)); } while (0)
#define REX_HCLEAR(K) for (int k = 0; k < HT_SLOTS; k++) (K).tacc[k] = 0
#define REX_HFLUSH(K) for (int k = 0; k < HT_SLOTS; k++) { \
    unsigned long long v = (K).tacc[k]; \
    for (int off = 32; off > 0; off >>= 1) { unsigned long long o = __shfl_xor(v, off); v = o > v ? o : v; } \
    if ((threadIdx.x & 63) == 0) atomicAdd(&g_ktime[8 + k], v); \
    REX_HFLUSH_WAVE(k, v); }
#else
#define REX_KSUBSTEPS(t0) ((void)0)
#define REX_HCLEAR(K) ((void)0)
#define REX_HFLUSH(K) ((void)0)
#endif
