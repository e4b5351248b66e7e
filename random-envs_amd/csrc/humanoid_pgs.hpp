// humanoid_pgs.hpp -- humanoid engine, layer 6: the constraint solvers -- the scratch-row PGS, the phase fence and register pins, the sweep
// families over the lane's LDS column (packed triangle, square) and the dual solver that builds A and picks the sweep size.
// Includes humanoid_collision.hpp.
#pragma once
#include "humanoid_collision.hpp"

namespace rex {
namespace hum {

// [3P] mj_solPGS on the dual, with qacc carried along: res_i = J_i qacc - aref_i + R_i f_i.  Rows stay in scratch: only
// used when an evaluation has more rows than the LDS column holds (pile-ups).
template <class T>
REX_HD int solve_pgs(const Model<T>& m, const MassFactor<T>& F, const Kin<T>& K, Scratch<T>& s, T* qacc) {
  for (int k = 0; k < NV; k++) qacc[k] = K.qacc_smooth[k];
  for (int i = 0; i < K.nefc; i++) {
    T x[NV], jr[NV];
    for (int k = 0; k < NV; k++) { jr[k] = s.J[i][k]; x[k] = jr[k]; }
    solve(F, x);
    T a = s.R[i];
    for (int k = 0; k < NV; k++) { s.MiJ[i][k] = x[k]; a += jr[k] * x[k]; }
    s.Adiag[i] = a; s.force[i] = 0;   // warmstart disabled (humanoid.xml:11)
  }
  const T scale = T(1) / (m.meaninertia * T(NV));
  int it = 0;
  const int n = K.nefc;
  // the rows live in scratch: row i + 1 (J, M^-1 J^T and its four scalars) is fetched while row i is updated -- unpipelined, every
  // row update was two dependent memory round trips, which is all this path (lying, crumpled bodies: 22 .. 108 rows) waits for
  T jn[NV], mn[NV], sn[4];
  auto fetch = [&](int i) { for (int k = 0; k < NV; k++) { jn[k] = s.J[i][k]; mn[k] = s.MiJ[i][k]; } sn[0] = s.R[i]; sn[1] = s.aref[i]; sn[2] = s.Adiag[i]; sn[3] = s.force[i]; };
  for (; it < m.iterations; it++) {
    T improvement = 0;
    fetch(0);
    for (int i = 0; i < n; i++) {
      T jr[NV], mr[NV];
      for (int k = 0; k < NV; k++) { jr[k] = jn[k]; mr[k] = mn[k]; }
      const T Ri = sn[0], arefi = sn[1], Ad = sn[2], old = sn[3];
      fetch(i + 1 < n ? i + 1 : i);   // (the force of row i + 1 is not written by row i)
      T res = Ri * old - arefi;
      for (int k = 0; k < NV; k++) res += jr[k] * qacc[k];
      const T nf = hmax(T(0), old - res / Ad), df = nf - old;
      s.force[i] = nf;
      if (df != T(0)) for (int k = 0; k < NV; k++) qacc[k] += mr[k] * df;
      improvement -= T(0.5) * df * df * Ad + df * res;
    }
    if (improvement * scale < m.tolerance) { it++; break; }
  }
  return it;
}

// phase boundary: keeps the machine scheduler from interleaving two phases of forward() (which only lengthens live
// ranges: 739 -> spilled VGPRs without it)
#if defined(__HIP_DEVICE_COMPILE__)
#define REX_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define REX_FENCE() ((void)0)
#endif

// keeps a batch of LDS reads together: all of them are issued, waited for once and held in registers from here on
#if defined(__HIP_DEVICE_COMPILE__) && !defined(REX_NOPIN)
#define REX_PIN4(a, b, c, d) asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d))
#define REX_PIN2(a, b) asm volatile("" : "+v"(a), "+v"(b))
#else
#define REX_PIN4(a, b, c, d) ((void)0)
#define REX_PIN2(a, b) ((void)0)
#endif

template <int Q, int NP, class T>
REX_HD void pin_all(T (&a)[NP]) { if constexpr (Q < NP) { REX_PIN4(a[Q], a[Q + 1], a[Q + 2], a[Q + 3]); pin_all<Q + 4>(a); } }

// Gauss-Seidel sweeps over rows / columns 0..NC-1 of the lane's packed A (NC a multiple of 4, or DUAL_NMAX).  The forces
// live in registers and every index is a compile-time constant: a row update is one batch of LDS reads at fixed offsets
// (no address arithmetic, no LDS write) followed by four short FMA chains.  Rows beyond the largest row count of the wave
// are skipped; padding inside the range is zero, which makes its update a no-op.
#ifndef REX_PGS_CHECK
#define REX_PGS_CHECK 10
#endif
constexpr int PGS_CHECK = REX_PGS_CHECK;   // the device sweeps evaluate the stopping criterion every PGS_CHECK-th sweep (pgs_sweeps_sq)

// How often a sweep evaluates the stopping criterion: every PGS_CHECK-th sweep in the fp32 device code (pgs_sweeps_sq has the argument), every
// sweep ([3P] mj_solPGS) in the host instantiations -- unless the harness is built with -DREX_PGS_CHECK_HOST, which gives the fp32 host code the
// DEVICE's schedule so a host test exercises exactly the sweep counts the GPU runs (tests/test_humanoid_host.py).  REX_PGS_CHECK itself is a
// compile-time define: it reaches the product only through the hipcc flags, which __graft_entry__ hashes into librex_hip.so.digest.
template <class T> constexpr int pgs_check_period() {
#if defined(__HIP_DEVICE_COMPILE__) || defined(REX_PGS_CHECK_HOST)
  return sizeof(T) == 4 ? PGS_CHECK : 1;
#else
  return 1;
#endif
}
// is the criterion evaluated after sweep `it` (0-based) of at most `iters`?  (groups of K - 1 unchecked sweeps + one checked, the last sweep always checked)
template <class T> REX_HD bool pgs_checked(int it, int iters) { constexpr int K = pgs_check_period<T>(); return K == 1 || (it + 1) % K == 0 || it + 1 == iters; }
template <int NC, int I, class T>
REX_HD void pgs_load_row(const T* col, T (&a)[(NC + 3) / 4 * 4 + 2]) {   // row I of the packed A, then b_I and 1 / A_II
  constexpr int NP = (NC + 3) / 4 * 4;
  static_for<0, NP>([&](auto JJ) { constexpr int j = JJ; a[j] = j < NC ? col[j <= I ? tri(I) + j : tri(j) + I] : T(0); });
  a[NP] = col[DUAL_B + I]; a[NP + 1] = col[DUAL_DI + I];
}
template <int Q, int N, class T>
REX_HD void pin_row(T (&a)[N]) {
  if constexpr (Q + 4 <= N) { REX_PIN4(a[Q], a[Q + 1], a[Q + 2], a[Q + 3]); pin_row<Q + 4>(a); }
  else if constexpr (Q + 2 <= N) { REX_PIN2(a[Q], a[Q + 1]); pin_row<Q + 2>(a); }
}

// The sweep schedule of every checked-every-K-th-sweep family (pgs_sweeps, pgs_sweeps_sq, and the two pair forms of
// humanoid_pair_pgs.hpp): groups of K - 1 unchecked sweeps and one checked, the last sweep always checked; stops after the first checked
// sweep whose cost decrease falls under the tolerance ([3P] mj_solPGS).  sweep(std::true_type) accumulates the decrease in `improvement`;
// REDUCE completes it where it is a partial sum (the pair: improvement += p.xchg(improvement)) and is empty otherwise.  `it` counts the
// sweeps run.  A macro, not a function: as pgs_schedule<K>(m, scale, sweep, improvement, reduce) it changed both step kernels' code
// (profiles/HISTORY.md).
#if defined(__HIP_DEVICE_COMPILE__)
#define REX_UNROLL_1 _Pragma("unroll 1")
#else
#define REX_UNROLL_1
#endif
#define REX_PGS_SCHEDULE(K, it, m, scale, sweep, improvement, REDUCE) \
  while (it < m.iterations) { \
    int nun = m.iterations - 1 - it; nun = nun < (K) - 1 ? nun : (K) - 1; \
    REX_UNROLL_1 \
    for (int u = 0; u < nun; u++) { sweep(std::false_type{}); it++; } \
    improvement = 0; \
    sweep(std::true_type{}); it++; \
    REDUCE; \
    if (improvement * scale < m.tolerance) break; \
  }

template <int NC, class T>
REX_HD int pgs_sweeps(const Model<T>& m, const T* col, int n, T (&f)[DUAL_NMAX]) {
  constexpr int NP = (NC + 3) / 4 * 4;
  const T scale = T(1) / (m.meaninertia * T(NV));
  // Software pipeline over the rows: the reads of row i + 1 (they do not depend on the forces) are issued before row i is
  // consumed, so the LDS latency hides behind the FMA chains and the projection of the previous row.  All NC rows run (no
  // branch between rows: the whole sweep is one basic block); rows >= n are zero padding and leave f unchanged.
  T buf[NP + 2];
  pgs_load_row<NC, 0>(col, buf);
  int it = 0;
  T improvement = 0;
  auto sweep = [&](auto CHECK) {
    static_for<0, NC>([&](auto II) {
      constexpr int i = II, nxt = (i + 1) % NC;
      T a[NP + 2];
      static_for<0, NP + 2>([&](auto KK) { a[KK] = buf[KK]; });
      pgs_load_row<NC, nxt>(col, buf);   // next row (row 0 of the next sweep after the last one): in flight while this one is used
      pin_row<0>(a);
      T res;
#if defined(__HIP_DEVICE_COMPILE__) && !defined(REX_NO_PK)
      if constexpr (sizeof(T) == 4) {   // two packed chains: v_pk_fma_f32 does two of the row's products per instruction
        typedef float v2f __attribute__((ext_vector_type(2)));
        v2f acc0 = {a[NP], 0.0f}, acc1 = {0.0f, 0.0f};
        static_for<0, NP / 4>([&](auto QQ) {
          constexpr int q = 4 * QQ;
          const v2f a01 = {a[q], a[q + 1]}, f01 = {f[q], q + 1 < NC ? f[q + 1 < DUAL_NMAX ? q + 1 : 0] : 0.0f};
          const v2f a23 = {a[q + 2], a[q + 3]}, f23 = {q + 2 < NC ? f[q + 2 < DUAL_NMAX ? q + 2 : 0] : 0.0f, q + 3 < NC ? f[q + 3 < DUAL_NMAX ? q + 3 : 0] : 0.0f};
          acc0 = __builtin_elementwise_fma(a01, f01, acc0); acc1 = __builtin_elementwise_fma(a23, f23, acc1);
        });
        const v2f t = acc0 + acc1;
        res = t.x + t.y;
      } else
#endif
      {
        T r0 = a[NP], r1 = 0, r2 = 0, r3 = 0;
        static_for<0, NP / 4>([&](auto QQ) {
          constexpr int q = 4 * QQ;
          r0 += a[q] * f[q]; if constexpr (q + 1 < NC) r1 += a[q + 1] * f[q + 1]; if constexpr (q + 2 < NC) r2 += a[q + 2] * f[q + 2]; if constexpr (q + 3 < NC) r3 += a[q + 3] * f[q + 3];
        });
        res = (r0 + r1) + (r2 + r3);
      }
      const T old = f[i], nf = hmax(T(0), old - res * a[NP + 1]), df = nf - old;
      f[i] = nf;
      if constexpr (decltype(CHECK)::value) improvement -= df * (T(0.5) * df * a[i] + res);   // cost decrease of this update ([3P] mj_solPGS), three instructions
    });
  };
  // the stopping criterion in every K-th sweep only on the device (pgs_sweeps_sq has the argument); every sweep on the host
  constexpr int K = pgs_check_period<T>();
  REX_PGS_SCHEDULE(K, it, m, scale, sweep, improvement, (void)0)
  return it;
}

// The same sweeps for NC <= 16 with A stored SQUARE, row-major with row stride NP = NC rounded up to a multiple of 4, then
// b[NP] and 1/A_ii[NP] (NP^2 + 2 NP <= 288 words).  A row is NP / 4 contiguous 16-byte LDS reads that land in aligned register
// pairs -- what v_pk_fma_f32 wants -- instead of NC scattered words of the packed triangle that have to be re-paired with
// moves.
constexpr int sq_stride(int nc) { return (nc + 3) / 4 * 4; }

// The sweeps of a dual solve run over the smallest of eight fixed sizes that holds every lane of the wave (the launch ends with its slowest
// wave and sweeps cost 50 x NC rows: sizes in steps of two above 8).  Sizes up to 16 keep A square (row stride sq_stride), the two largest a
// triangle (packed here, padded in humanoid_pair_pgs.hpp); the level is wave-uniform, so the layout is known before A is built.
constexpr int DUAL_LEVELS = 8, DUAL_SQ_LEVELS = 6;
constexpr int kDualRows[DUAL_LEVELS] = {4, 8, 10, 12, 14, 16, 18, DUAL_NMAX};
static_assert(kDualRows[DUAL_SQ_LEVELS - 1] == 16 && sq_stride(16) * (sq_stride(16) + 2) <= DUAL_WORDS, "the square sizes must fit the LDS column");
template <class Any>
REX_HD int dual_level(Any&& any, int n) {   // any(b): does some lane of the wave say b
  int lvl = 0;
  static_for<0, DUAL_LEVELS>([&](auto LL) { if (any(n > kDualRows[LL])) lvl = LL + 1; });
#if defined(__HIP_DEVICE_COMPILE__)
  lvl = __builtin_amdgcn_readfirstlane(lvl);
#endif
  return lvl;
}
constexpr bool dual_square(int lvl) { return lvl < DUAL_SQ_LEVELS; }
constexpr int dual_stride(int lvl) { return lvl == 0 ? 4 : lvl == 1 ? 8 : lvl <= 3 ? 12 : 16; }   // sq_stride of the level's size (16 above the square sizes)
constexpr bool dual_stride_ok() {
  for (int l = 0; l < DUAL_LEVELS; l++) if (dual_stride(l) != sq_stride(kDualRows[l < DUAL_SQ_LEVELS ? l : DUAL_SQ_LEVELS - 1])) return false;
  return true;
}
static_assert(dual_stride_ok(), "dual_stride is written out (a select chain the compiler keeps as it is): it must agree with the table");
// (The switch over the level stays written out in the two solve_pgs_dual: as one dispatch_level(lvl, f) calling f(IC<rows>) it changed both
// step kernels' code, profiles/HISTORY.md.)
#if defined(__HIP_DEVICE_COMPILE__)
typedef float pgs_v2f __attribute__((ext_vector_type(2)));
typedef float pgs_v4f __attribute__((ext_vector_type(4)));
template <int Q, int N> __device__ __forceinline__ void pin_v4(pgs_v4f (&a)[N]) { if constexpr (Q < N) { asm volatile("" : "+v"(a[Q])); pin_v4<Q + 1>(a); } }
__device__ __forceinline__ void pin_v2(pgs_v2f& x) { asm volatile("" : "+v"(x)); }
#endif
template <int NC, class T>
REX_HD int pgs_sweeps_sq(const Model<T>& m, const T* col, T (&f)[DUAL_NMAX]) {
  constexpr int NP = sq_stride(NC), BOFF = NP * NP, DOFF = BOFF + NP;
  static_assert(DOFF + NP <= DUAL_WORDS && NC <= DUAL_NMAX, "square layout must fit the LDS column");
  const T scale = T(1) / (m.meaninertia * T(NV));
  int it = 0;
#if defined(__HIP_DEVICE_COMPILE__) && !defined(REX_NO_PK)
  if constexpr (sizeof(T) == 4) {
    typedef pgs_v2f v2f; typedef pgs_v4f v4f;
    // Residual form: res_r = b_r + sum_j A_rj f_j is kept current for every row; an update of f_k by df pushes A_rk df into
    // all of them (column k = row k, A is symmetric).  The same multiply-adds as a row dot product per update, but they are
    // independent of one another: the dependent chain from one row's update to the next is fma, max, sub, pk_fma instead of
    // a whole dot product and its reduction -- what counts for a lone wave on its SIMD.
    v2f rp[NP / 2]; float fv[NC];
    static_for<0, NP / 4>([&](auto QQ) { constexpr int q = QQ; const v4f b4 = *(const v4f*)(col + BOFF + 4 * q); rp[2 * q] = v2f{b4.x, b4.y}; rp[2 * q + 1] = v2f{b4.z, b4.w}; });
    static_for<0, NC>([&](auto II) { fv[II] = 0.0f; });
    v4f buf[NP / 4]; float dnext;
    auto load_row = [&](auto II, v4f (&a)[NP / 4], float& d) {
      constexpr int i = II;
      static_for<0, NP / 4>([&](auto QQ) { constexpr int q = QQ; a[q] = *(const v4f*)(col + i * NP + 4 * q); });
      d = col[DOFF + i];
    };
    load_row(IC<0>{}, buf, dnext);
    // [3P] mj_solPGS stops after the first sweep whose cost decrease falls under the tolerance.  Computing the decrease costs four
    // of a row update's instructions and -- worse -- keeps the matrix from living in registers across the sweeps: without it a
    // 12-row sweep is 125 instructions (6 v_pk_fma + fma, max, sub per row, no LDS read, no move) instead of 257.  A wave runs
    // until its LAST lane stops (one that hits the 50-sweep cap in most waves), so the criterion is evaluated in every
    // PGS_CHECK-th sweep only: a lane that would have stopped after sweep k stops after sweep PGS_CHECK * ceil(k / PGS_CHECK) <= 50
    // instead -- up to PGS_CHECK - 1 more sweeps of a system already converged to the tolerance (1e-8 of the cost scale: far
    // below fp32 rounding of the result; the unchecked sweeps cost half, so even those lanes do not pay), never more than
    // MuJoCo's cap.  Humanoid step kernel 2.17 -> 1.99 ms (every 5th sweep, square sizes) -> 1.91 (packed sizes too) -> 1.86 (10th).
    float improvement = 0;
    auto sweep = [&](auto CHECK) {
      static_for<0, NC>([&](auto II) {
        constexpr int i = II, nxt = (i + 1) % NC;
        v4f a[NP / 4]; const float di = dnext;
        static_for<0, NP / 4>([&](auto QQ) { a[QQ] = buf[QQ]; });
        load_row(IC<nxt>{}, buf, dnext);   // next row in flight while this one is consumed
        const float res = (i & 1) ? rp[i / 2].y : rp[i / 2].x;
        const float old = fv[i], nf = __builtin_fmaxf(0.0f, old - res * di), df = nf - old;   // a NaN residual (non-finite state: the lane is flagged) gives 0
        fv[i] = nf;
        if constexpr (decltype(CHECK)::value) { const float aii = a[i / 4][i & 3]; improvement -= df * (0.5f * df * aii + res); }
        const v2f dfp = {df, df};
        static_for<0, NP / 4>([&](auto QQ) {
          constexpr int q = QQ;
          rp[2 * q] = __builtin_elementwise_fma(v2f{a[q].x, a[q].y}, dfp, rp[2 * q]);
          rp[2 * q + 1] = __builtin_elementwise_fma(v2f{a[q].z, a[q].w}, dfp, rp[2 * q + 1]);
        });
      });
    };
    REX_PGS_SCHEDULE(PGS_CHECK, it, m, scale, sweep, improvement, (void)0)
    static_for<0, NC>([&](auto II) { f[II] = fv[II]; });
    return it;
  } else
#endif
  {
    for (; it < m.iterations; it++) {
      T improvement = 0;
      for (int i = 0; i < NC; i++) {
        T res = col[BOFF + i];
        for (int j = 0; j < NC; j++) res += col[i * NP + j] * f[j];
        const T old = f[i], nf = hmax(T(0), old - res * col[DOFF + i]), df = nf - old;
        f[i] = nf;
        improvement -= df * (T(0.5) * df * col[i * NP + i] + res);
      }
      if (pgs_checked<T>(it, m.iterations) && improvement * scale < m.tolerance) { it++; break; }
    }
    return it;
  }
}

// The same Gauss-Seidel sweeps on the dual: res_i = sum_j A_ij f_j + b_i with A = J M^-1 J^T + diag(R),
// b = J qacc_smooth - aref ([3P] mj_solPGS works on exactly this matrix).  A, f and b sit in the lane's LDS column, so a
// sweep costs n^2 LDS reads instead of 2 n nv reads of J / M^-1 J^T rows from scratch (which miss every cache level);
// J is read once per row pair to build A and once more for qacc = qacc_smooth + M^-1 J^T f.
template <class T>
REX_HD int solve_pgs_dual(const Model<T>& m, const MassFactor<T>& F, Kin<T>& K, Scratch<T>& s, T* qacc) {
  const int n = K.nefc;
  T* const col = (T*)__builtin_assume_aligned(&dual(s, 0), 16);
  REX_HSTAMP(p0);
  // Sweeps run over the smallest of eight fixed sizes that holds every lane of the wave (the launch ends with its slowest wave
  // and sweeps cost 50 x NC rows: sizes in steps of two above 8).  Sizes up to 16 keep A square (pgs_sweeps_sq), the two largest
  // the packed lower triangle; the level is wave-uniform, so the layout is known before A is built.
  const int lvl = dual_level([](bool b) { return REX_WAVE_ANY(b); }, n);
  const bool sq = dual_square(lvl);
  const int stride = dual_stride(lvl);
  const int boff = sq ? stride * stride : DUAL_B, doff = sq ? boff + stride : DUAL_DI;
  static_for<0, DUAL_WORDS>([&](auto KK) { col[KK] = T(0); });   // padding rows / columns must read as zero
  // A = J M^-1 J^T = Y D^-1 Y^T with Y^T = L^-T J^T ([3P] mj_solveM2): only the backward half of the solve per row, four rows
  // per trip (one pass over the factor for all four).  Row j of the scratch array is overwritten with z_j = D^-1 y_j: the
  // dots with later rows and the final M^-1 J^T f = L^-1 sum_j f_j z_j need nothing else (J_j is dead once b_j is formed).
  // Every earlier row is read once per group of four, two rows per read batch, a batch ahead of its dot products.
  for (int j0 = 0; j0 < n; j0 += 4) {
    T y0[NV], y1[NV], y2[NV], y3[NV], Rr[4];
    bool ok[4]; int jj[4];
    static_for<0, 4>([&](auto TT) { constexpr int t = TT; ok[t] = j0 + t < n; jj[t] = ok[t] ? j0 + t : j0; });   // rows past the lane's count duplicate the group's first row and are dropped
    { T ar[4];
      for (int k = 0; k < NV; k++) { y0[k] = s.J[jj[0]][k]; y1[k] = s.J[jj[1]][k]; y2[k] = s.J[jj[2]][k]; y3[k] = s.J[jj[3]][k]; }
      static_for<0, 4>([&](auto TT) { constexpr int t = TT; Rr[t] = s.R[jj[t]]; ar[t] = s.aref[jj[t]]; });
      pin_row<0>(y0); pin_row<0>(y1); pin_row<0>(y2); pin_row<0>(y3);
      const T b0 = dot_nv(y0, K.qacc_smooth) - ar[0], b1 = dot_nv(y1, K.qacc_smooth) - ar[1], b2 = dot_nv(y2, K.qacc_smooth) - ar[2], b3 = dot_nv(y3, K.qacc_smooth) - ar[3];
      col[boff + j0] = b0; if (ok[1]) col[boff + j0 + 1] = b1; if (ok[2]) col[boff + j0 + 2] = b2; if (ok[3]) col[boff + j0 + 3] = b3; }
    solve_back4(F, y0, y1, y2, y3);
    auto rowp = [&](int r) -> T* { return col + (sq ? r * stride : tri(r)); };   // row r of A, columns 0..r
    auto put = [&](int r, int c, T v) { rowp(r)[c] = v; if (sq && c != r) col[c * stride + r] = v; };   // (r, c) with c <= r, and its mirror in the square layout
    // entries inside the group: z_u = D^-1 y_u is formed, stored (row j0 + u of the scratch array) and dotted with y_t, t >= u
    auto within = [&](auto UU, T (&yu)[NV]) {
      constexpr int u = UU;
      T z[NV];
      static_for<0, NV>([&](auto KK) { constexpr int k = KK; z[k] = yu[k] * F.a[midx(k, k)]; });
      if (ok[u]) {
        for (int k = 0; k < NV; k++) s.J[j0 + u][k] = z[k];
        const T d = Rr[u] + dot_nv(z, yu);
        rowp(j0 + u)[j0 + u] = d; col[doff + j0 + u] = rcp_t(d);
      }
      if constexpr (u < 1) { const T v = dot_nv(z, y1); if (ok[1]) put(j0 + 1, j0 + u, v); }
      if constexpr (u < 2) { const T v = dot_nv(z, y2); if (ok[2]) put(j0 + 2, j0 + u, v); }
      if constexpr (u < 3) { const T v = dot_nv(z, y3); if (ok[3]) put(j0 + 3, j0 + u, v); }
    };
    within(IC<0>{}, y0); within(IC<1>{}, y1); within(IC<2>{}, y2); within(IC<3>{}, y3);
    // earlier rows (already z rows): two per batch, the next batch in flight while this one is dotted with the four y
    T ra[NV], rb[NV], rc[NV], rd[NV];
    auto fetch2 = [&](int i, T (&u)[NV], T (&v)[NV]) {
      const int i0 = i < j0 ? i : 0, i1 = i + 1 < j0 ? i + 1 : i0;
      for (int k = 0; k < NV; k++) { u[k] = s.J[i0][k]; v[k] = s.J[i1][k]; }
    };
    auto use1 = [&](int i, T (&u)[NV]) {
      const T a0 = dot_nv(u, y0), a1 = dot_nv(u, y1), a2 = dot_nv(u, y2), a3 = dot_nv(u, y3);
      if (i < j0) { put(j0, i, a0); if (ok[1]) put(j0 + 1, i, a1); if (ok[2]) put(j0 + 2, i, a2); if (ok[3]) put(j0 + 3, i, a3); }
    };
    fetch2(0, ra, rb);
    for (int i = 0; i < j0; i += 4) {
      fetch2(i + 2, rc, rd);
      pin_row<0>(ra); pin_row<0>(rb); use1(i, ra); use1(i + 1, rb);
      fetch2(i + 4, ra, rb);
      pin_row<0>(rc); pin_row<0>(rd); use1(i + 2, rc); use1(i + 3, rd);
    }
  }
  REX_HSTAMP(p1); REX_HACC(K, HT_BUILD_A, p0, p1);
  int it;
  T f[DUAL_NMAX];
  static_for<0, DUAL_NMAX>([&](auto II) { f[II] = T(0); });
  switch (lvl) {   // (kDualRows; the same switch with the pair's callees for levels 5 - 7: humanoid_pair_pgs.hpp::solve_pgs_dual)
    case 0: it = pgs_sweeps_sq<4>(m, col, f); break;
    case 1: it = pgs_sweeps_sq<8>(m, col, f); break;
    case 2: it = pgs_sweeps_sq<10>(m, col, f); break;
    case 3: it = pgs_sweeps_sq<12>(m, col, f); break;
    case 4: it = pgs_sweeps_sq<14>(m, col, f); break;
    case 5: it = pgs_sweeps_sq<16>(m, col, f); break;
    case 6: it = pgs_sweeps<18>(m, col, n, f); break;
    default: it = pgs_sweeps<DUAL_NMAX>(m, col, n, f); break;
  }
  REX_HSTAMP(p2); REX_HACC(K, HT_SWEEPS, p1, p2); REX_HCNT(K, HC_SWEEPS, it);
  T x[NV];
  for (int k = 0; k < NV; k++) x[k] = 0;
  static_for<0, DUAL_NMAX / 3>([&](auto CC) {   // sum_j f_j z_j, three rows per trip (reads batched; rows >= n re-read row 0 with f = 0)
    constexpr int i0 = 3 * CC;
    if (REX_WAVE_ANY(i0 < n)) {
      T r[3][NV], fi[3];
      static_for<0, 3>([&](auto RR) { constexpr int r_ = RR, i = i0 + r_; const int ii = i < n ? i : 0; fi[r_] = i < n ? f[i] : T(0);
        if (i < n) s.force[i] = fi[r_];
        for (int k = 0; k < NV; k++) r[r_][k] = s.J[ii][k]; });
      pin_row<0>(r[0]); pin_row<0>(r[1]); pin_row<0>(r[2]);
      for (int k = 0; k < NV; k++) x[k] += r[0][k] * fi[0] + r[1][k] * fi[1] + r[2][k] * fi[2];
    }
  });
  solve_fwd(F, x);
  for (int k = 0; k < NV; k++) qacc[k] = K.qacc_smooth[k] + x[k];
  REX_HSTAMP(p3); REX_HACC(K, HT_QACC, p2, p3);
  return it;
}

}  // namespace hum
}  // namespace rex
