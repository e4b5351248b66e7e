// humanoid_pair_host.cpp -- TEST HARNESS ONLY (never loaded by the product): the two-lanes-per-env humanoid engine
// (random-envs_amd/csrc/humanoid_pair.hpp) on the host.  The two lanes of a pair run as two threads in lock step: an exchange
// is a rendezvous (write own slot, barrier, read the partner's), the env's LDS column is an array both threads see.
#include <atomic>
#include <cstring>
#include <thread>
#include "../../random-envs_amd/csrc/humanoid_model.hpp"
#include "../../random-envs_amd/csrc/humanoid_pair.hpp"

using namespace rex::hum;

struct Barrier2 {   // sense-reversing spin barrier for two threads
  std::atomic<int> count{0}; std::atomic<int> sense{0};
  void wait(int& local) {
    local ^= 1;
    if (count.fetch_add(1, std::memory_order_acq_rel) == 1) { count.store(0, std::memory_order_relaxed); sense.store(local, std::memory_order_release); }
    else while (sense.load(std::memory_order_acquire) != local) { }
  }
};
template <class T> struct Shared { Barrier2 bar; alignas(16) T col[pr::PAIR_WORDS]; unsigned char slot[2][16]; };
template <class T> struct HostPair {
  Shared<T>* sh; int s; mutable int sense = 0;
  int side() const { return s; }
  template <class U> U xchg(U x) const { memcpy(sh->slot[s], &x, sizeof(U)); sh->bar.wait(sense); U r; memcpy(&r, sh->slot[s ^ 1], sizeof(U)); sh->bar.wait(sense); return r; }
  bool any(bool b) const { const unsigned o = xchg<unsigned>(b ? 1u : 0u); return b || o != 0u; }   // (the device asks the whole wave: any superset of the pair is correct)
  T* col() const { return sh->col; }
  void sync() const { sh->bar.wait(sense); }
};

template <class T> struct Ctx { Model<T> m; };
template <class T> static Ctx<T>* ctx() {
  static Ctx<T>* c = nullptr;
  if (!c) { c = new Ctx<T>(); Model<double> md; build_model(md); convert_model(md, c->m); }
  return c;
}

// One env's element of the rows of the SoA blocks ([row][n] doubles; a null block reads as 0 and swallows writes): what load_lane /
// store_lane / reset_lane see, as on the device.  `lane` receives each side's PLane and local controls (hp_roundtrip).
struct Io { int n; const double *xi, *qpos, *qvel, *act, *aux; double *qpos_out, *qvel_out, *aux_out, *obs; };
template <class T> static auto reader(const Io& io, int i) {
  return [&io, i](int blk, int row) { const double* b = blk == pr::XI ? io.xi : blk == pr::QPOS ? io.qpos : blk == pr::QVEL ? io.qvel : blk == pr::ACTION ? io.act : io.aux;
                                      return b ? T(b[(size_t)row * io.n + i]) : T(0); };
}
template <class T> static auto writer(const Io& io, int i) {
  return [&io, i](int blk, int row, T val) { double* b = blk == pr::QPOS ? io.qpos_out : blk == pr::QVEL ? io.qvel_out : io.aux_out; if (b) b[(size_t)row * io.n + i] = double(val); };
}
template <class T, class P> static void put_obs(const P& p, const Io& io, int i, const T (&ql)[pr::LQ], const T (&vl)[pr::LD], const pr::PObs<T>& park) {
  pr::emit_obs(p, ql, vl, park, [&](auto RR, auto RL, T val) { constexpr int rr = RR, rl = RL; io.obs[(size_t)(p.side() ? rl : rr) * io.n + i] = double(val); });
}

template <class T>
static void step_lane(int s, Shared<T>* sh, const Io& io, double* reward, unsigned char* done, int* overflow, int* nrows) {
  const Model<T>& m = ctx<T>()->m;
  HostPair<T> p{sh, s};
  const bool left = s != 0;
  pr::PKin<T>* K = new pr::PKin<T>(); pr::PScratch<T>* sc = new pr::PScratch<T>();
  for (int i = 0; i < io.n; i++) {
    pr::PLane<T> L; T ql[pr::LQ], vl[pr::LD], cl[pr::LU], xp[pr::LB];
    pr::load_lane(left, reader<T>(io, i), L, ql, vl, cl, xp);
    if (!io.aux || io.aux[i] != io.aux[i]) {   // set_state's sim.forward(): the one-lane engine (both threads compute the same)
      Lane<T> L1; L1.mass[0] = 0; for (int b = 1; b < NBODY; b++) L1.mass[b] = T(io.xi[(size_t)(b - 1) * io.n + i]);
      for (int d = 0; d < NV; d++) L1.damping[d] = d < 6 ? T(0) : T(io.xi[(size_t)(13 + d - 6) * io.n + i]);
      T q[NQ], v[NV], x14[NBODY]; Kin<T>* k1 = new Kin<T>(); Scratch<T>* s1 = new Scratch<T>();
      for (int k = 0; k < NQ; k++) q[k] = T(io.qpos[(size_t)k * io.n + i]);
      for (int k = 0; k < NV; k++) v[k] = T(io.qvel[(size_t)k * io.n + i]);
      env_reset_obs(m, L1, q, v, x14, *k1, *s1, [](int, T) {});
      for (int lb = 0; lb < pr::LB; lb++) xp[lb] = x14[pr::row_aux(left, lb)];
      delete k1; delete s1;
    }
    pr::PObs<T> park; T r; bool d;
    pr::env_step(p, m, L, ql, vl, cl, pr::ctrl_sq(p, cl), xp, *K, *sc, park, r, d);
    put_obs(p, io, i, ql, vl, park);
    pr::store_lane(left, writer<T>(io, i), ql, vl, xp);
    if (!left) { reward[i] = double(r); done[i] = d; if (overflow) overflow[i] = K->overflow; if (nrows) nrows[i] = K->nefc; }
    p.sync();
  }
  delete K; delete sc;
}

// reset_model on the pair: the kernel's fused auto-reset without its Philox set-up (draws: NQ then NV uniforms per env, [47][n])
template <class T>
static void reset_lane_main(int s, Shared<T>* sh, const Io& io, const double* draws) {
  HostPair<T> p{sh, s};
  const bool left = s != 0;
  for (int i = 0; i < io.n; i++) {
    pr::PLane<T> L; T ql[pr::LQ], vl[pr::LD], cl[pr::LU], xp[pr::LB]; pr::PObs<T> park;
    pr::load_lane(left, reader<T>(io, i), L, ql, vl, cl, xp);
    int k = 0;
    pr::reset_lane(p, ctx<T>()->m, L, [&]() { return T(draws[(size_t)(k++) * io.n + i]); }, ql, vl, xp, park);
    put_obs(p, io, i, ql, vl, park);
    pr::store_lane(left, writer<T>(io, i), ql, vl, xp);
    p.sync();
  }
}

template <class T, class F>
static void run_pair(F&& lane) {   // lane(side, shared): the two lanes of a pair as two threads in lock step
  (void)ctx<T>();   // build the model before the lanes start
  Shared<T>* sh = new Shared<T>();
  std::thread t1([&] { lane(1, sh); });
  lane(0, sh);
  t1.join();
  delete sh;
}

extern "C" {
int hp_step(int f32, int n, const double* qpos, const double* qvel, const double* act, const double* xi, const double* xprev,
            double* qpos_out, double* qvel_out, double* obs, double* reward, unsigned char* done, double* xout, int* overflow, int* nrows) {
  const Io io{n, xi, qpos, qvel, act, xprev, qpos_out, qvel_out, xout, obs};
  if (f32) run_pair<float>([&](int s, Shared<float>* sh) { step_lane<float>(s, sh, io, reward, done, overflow, nrows); });
  else run_pair<double>([&](int s, Shared<double>* sh) { step_lane<double>(s, sh, io, reward, done, overflow, nrows); });
  return 0;
}
int hp_reset(int f32, int n, const double* draws, const double* xi, double* qpos_out, double* qvel_out, double* obs, double* xout) {
  const Io io{n, xi, nullptr, nullptr, nullptr, nullptr, qpos_out, qvel_out, xout, obs};
  if (f32) run_pair<float>([&](int s, Shared<float>* sh) { reset_lane_main<float>(s, sh, io, draws); });
  else run_pair<double>([&](int s, Shared<double>* sh) { reset_lane_main<double>(s, sh, io, draws); });
  return 0;
}
// load_lane then store_lane with nothing between; lane_out[side][8 masses, 16 dampings, 10 controls][n]: what each lane loaded beside the state
int hp_roundtrip(int n, const double* qpos, const double* qvel, const double* act, const double* xi, const double* aux,
                 double* qpos_out, double* qvel_out, double* aux_out, double* lane_out) {
  const Io io{n, xi, qpos, qvel, act, aux, qpos_out, qvel_out, aux_out, nullptr};
  for (int s = 0; s < 2; s++) for (int i = 0; i < n; i++) {
    pr::PLane<double> L; double ql[pr::LQ], vl[pr::LD], cl[pr::LU], xp[pr::LB];
    pr::load_lane(s != 0, reader<double>(io, i), L, ql, vl, cl, xp);
    pr::store_lane(s != 0, writer<double>(io, i), ql, vl, xp);
    double* o = lane_out + (size_t)s * (pr::LB + pr::LD + pr::LU) * n + i;
    for (int k = 0; k < pr::LB; k++) o[(size_t)k * n] = L.mass[k];
    for (int k = 0; k < pr::LD; k++) o[(size_t)(pr::LB + k) * n] = L.damping[k];
    for (int k = 0; k < pr::LU; k++) o[(size_t)(pr::LB + pr::LD + k) * n] = cl[k];
  }
  return 0;
}
int hp_check_model() { Model<double> md; build_model(md); return pr::check_pair_model(md) ? 1 : 0; }
}
