// abi_replay.hpp -- host code of rex_hip.hip: rex_rbuf_* (replay_buffer.hpp), rex_per_* (priority_replay.hpp) and the sample family with its n-step
// (nstep_replay.hpp) and sequence (seq_replay.hpp) windows, nine exported calls over one path: sample_call.
#pragma once

// ------------------------------------------------------------------------------------------
// off-policy replay buffer (replay_buffer.hpp): fused transposing add and on-device sampling over caller-owned transition-major buffers
// ------------------------------------------------------------------------------------------
// allocate once, synchronise, zero: the n device counters an opt-in layer keeps on the handle
static int enable_counters(void** mem, int n) {
  if (!*mem) HIP_TRY(hipMalloc(mem, sizeof(unsigned long long) * n));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemset(*mem, 0, sizeof(unsigned long long) * n));
  return REX_OK;
}

extern "C" int rex_rbuf_enable(rex_t* h) {
  REX_ENTER(h, "rex_rbuf_enable");
  return enable_counters(&h->rbuf_mem, 1);
}

// the caller's struct with the handle's sizes; every buffer is required
static int rbuf_buf(const rex_env* h, const rex_rbuf_buffers* b, const char* fn, rbuf::Buf* out) {
  if (!b) return set_err(REX_ERR_ARG, "%s: null buffer description", fn);
  if (!b->obs || !b->next_obs || !b->action || !b->reward || !b->done || !b->timeout)
    return set_err(REX_ERR_ARG, "%s: every pointer of rex_rbuf_buffers is required", fn);
  if (b->T <= 0) return set_err(REX_ERR_ARG, "%s: T must be > 0 (got %lld)", fn, (long long)b->T);
  *out = rbuf::Buf{(uint32_t*)b->obs, (uint32_t*)b->next_obs, (uint32_t*)b->action, b->reward, b->done, b->timeout,
                   (long long)b->T, h->B, h->dims.obs_dim, h->dims.act_dim};
  return REX_OK;
}

extern "C" int rex_rbuf_add(rex_t* h, const rex_rbuf_buffers* buf, int64_t t, const float* obs, const void* action, const float* reward,
                            const uint8_t* done, const float* next_obs, const float* terminal_obs, const uint8_t* truncated, void* stream) {
  REX_ENTER(h, "rex_rbuf_add");
  REX_NEEDS(h, rbuf_mem, "rex_rbuf_add", "rex_rbuf_enable");
  rbuf::AddParams p{};
  if (int rc = rbuf_buf(h, buf, "rex_rbuf_add", &p.buf)) return rc;
  if (t < 0 || t >= buf->T) return set_err(REX_ERR_ARG, "rex_rbuf_add: slot %lld outside [0, %lld)", (long long)t, (long long)buf->T);
  if (!obs || !action || !reward || !done || !next_obs) return set_err(REX_ERR_ARG, "rex_rbuf_add: null input");
  p.src = rbuf::AddSrc{(const uint32_t*)obs, (const uint32_t*)action, reward, done, (const uint32_t*)next_obs, (const uint32_t*)terminal_obs, truncated};
  p.slot = t;
  const long long tiles = rbuf::add_tiles(h->B);
  if (!grid_fits(tiles)) return set_err(REX_ERR_ARG, "rex_rbuf_add: batch %lld is more than one launch takes", h->B);
  const unsigned groups = (unsigned)rbuf::add_groups(p.buf.obs_dim, p.buf.act_dim);
  hipLaunchKernelGGL(rbuf::rb_add_kernel, dim3((unsigned)tiles, groups), dim3(rbuf::BLOCK), 0, (hipStream_t)stream, p);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

extern "C" int rex_rbuf_read_bad_indices(rex_t* h, int64_t* out, int clear) {
  REX_ENTER(h, "rex_rbuf_read_bad_indices");
  REX_NEEDS(h, rbuf_mem, "rex_rbuf_read_bad_indices", "rex_rbuf_enable");
  if (!out) return set_err(REX_ERR_ARG, "rex_rbuf_read_bad_indices: null argument");
  return read_counters(h->rbuf_mem, 1, out, clear);
}

// ------------------------------------------------------------------------------------------
// prioritised replay (priority_replay.hpp): per-transition priorities under a 64-ary fp64 sum tree in caller-owned memory, stratified
// proportional draws, priority updates
// ------------------------------------------------------------------------------------------
extern "C" int64_t rex_per_tree_len(int64_t N) {
  per::Tree t;
  if (!per::tree_of((long long)N, &t)) return set_err(REX_ERR_ARG, "rex_per_tree_len: N = %lld outside [1, 2^30]", (long long)N);
  return (int64_t)t.len;
}

extern "C" int rex_per_enable(rex_t* h) {
  REX_ENTER(h, "rex_per_enable");
  return enable_counters(&h->per_mem, per::N_COUNTERS);
}

// the caller's struct with the handle's batch and the tree's shape; every buffer is required
static int per_buf(const rex_env* h, const rex_per_buffers* b, const char* fn, per::Buf* out) {
  if (!b) return set_err(REX_ERR_ARG, "%s: null buffer description", fn);
  if (!b->priority || !b->tree || !b->max_priority) return set_err(REX_ERR_ARG, "%s: every pointer of rex_per_buffers is required", fn);
  if (b->T <= 0) return set_err(REX_ERR_ARG, "%s: T must be > 0 (got %lld)", fn, (long long)b->T);
  *out = per::Buf{b->priority, b->tree, b->max_priority, (long long)b->T, h->B, {}};
  if (b->T > per::MAX_LEAVES / h->B || !per::tree_of((long long)b->T * h->B, &out->tr))
    return set_err(REX_ERR_ARG, "%s: T * batch = %lld * %lld is more than 2^30 transitions", fn, (long long)b->T, h->B);
  return REX_OK;
}

// one launch per level below the top two over `n` threads -- the ancestors of index[0 .. n), or of the leaves [s0, s1] when index is
// null -- then the single block that takes the top
static void launch_per_refresh(const per::Buf& b, const long long* index, long long n, long long s0, long long s1, hipStream_t st) {
  for (int l = 1; l < per::top_first_level(b.tr); l++) {
    per::RefreshParams r{b, index, index ? n : per::range_count(s0, s1, l), index ? 0 : per::range_first(s0, l), l, 0};
    hipLaunchKernelGGL(per::per_refresh_kernel, dim3(blocks_for(r.n, per::BLOCK)), dim3(per::BLOCK), 0, st, r);
  }
  hipLaunchKernelGGL(per::per_top_kernel, dim3(1), dim3(per::BLOCK), 0, st, b);
}

extern "C" int rex_per_init(rex_t* h, const rex_per_buffers* buf, void* stream) {
  REX_ENTER(h, "rex_per_init");
  REX_NEEDS(h, per_mem, "rex_per_init", "rex_per_enable");
  per::Buf b;
  if (int rc = per_buf(h, buf, "rex_per_init", &b)) return rc;
  hipLaunchKernelGGL(per::per_init_kernel, dim3(blocks_for(per::init_items(b), per::BLOCK)), dim3(per::BLOCK), 0, (hipStream_t)stream, b, (int)per::INIT_ALL);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

extern "C" int rex_per_add(rex_t* h, const rex_per_buffers* buf, int64_t t, void* stream) {
  REX_ENTER(h, "rex_per_add");
  REX_NEEDS(h, per_mem, "rex_per_add", "rex_per_enable");
  per::Buf b;
  if (int rc = per_buf(h, buf, "rex_per_add", &b)) return rc;
  if (t < 0 || t >= buf->T) return set_err(REX_ERR_ARG, "rex_per_add: slot %lld outside [0, %lld)", (long long)t, (long long)buf->T);
  hipLaunchKernelGGL(per::per_fill_kernel, dim3(blocks_for(b.B, per::BLOCK)), dim3(per::BLOCK), 0, (hipStream_t)stream, b, (long long)t);
  launch_per_refresh(b, nullptr, 0, (long long)t * b.B, (long long)(t + 1) * b.B - 1, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

extern "C" int rex_per_update(rex_t* h, const rex_per_buffers* buf, const int64_t* index, const float* priority, int64_t n, void* stream) {
  REX_ENTER(h, "rex_per_update");
  REX_NEEDS(h, per_mem, "rex_per_update", "rex_per_enable");
  per::UpdateParams p{};
  if (int rc = per_buf(h, buf, "rex_per_update", &p.buf)) return rc;
  if (n < 0 || (n > 0 && (!index || !priority))) return set_err(REX_ERR_ARG, "rex_per_update: n must be >= 0 and index and priority given");
  if (n == 0) return REX_OK;
  if (!grid_fits((n + per::BLOCK - 1) / per::BLOCK)) return set_err(REX_ERR_ARG, "rex_per_update: n = %lld is more than one launch takes", (long long)n);
  p.index = (const long long*)index; p.value = priority; p.n = n; p.counters = (unsigned long long*)h->per_mem;
  const dim3 grid(blocks_for(n, per::BLOCK)), block(per::BLOCK);
  hipLaunchKernelGGL(per::per_clear_kernel, grid, block, 0, (hipStream_t)stream, p);
  hipLaunchKernelGGL(per::per_scatter_kernel, grid, block, 0, (hipStream_t)stream, p);
  launch_per_refresh(p.buf, p.index, n, 0, 0, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

extern "C" int rex_per_rebuild(rex_t* h, const rex_per_buffers* buf, void* stream) {
  REX_ENTER(h, "rex_per_rebuild");
  REX_NEEDS(h, per_mem, "rex_per_rebuild", "rex_per_enable");
  per::Buf b;
  if (int rc = per_buf(h, buf, "rex_per_rebuild", &b)) return rc;
  hipLaunchKernelGGL(per::per_init_kernel, dim3(1), dim3(per::BLOCK), 0, (hipStream_t)stream, b, (int)per::INIT_MAX);
  for (int l = 1; l <= b.tr.D; l++) {
    per::RefreshParams r{b, nullptr, b.tr.n[l], 0, l, l == 1 ? 1 : 0};
    hipLaunchKernelGGL(per::per_refresh_kernel, dim3(blocks_for(r.n, per::BLOCK)), dim3(per::BLOCK), 0, (hipStream_t)stream, r);
  }
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

// the draw launch of rex_per_draw and of the prioritised sample calls
static int launch_per_draw(const char* fn, const per::Buf& b, int64_t n, uint64_t seed, uint64_t draw, int64_t* index_out, float* prob_out, hipStream_t st) {
  if (n < 0 || (n > 0 && (!index_out || !prob_out))) return set_err(REX_ERR_ARG, "%s: n must be >= 0 and index_out and prob_out given", fn);
  if (n == 0) return REX_OK;
  if (!grid_fits((n + per::DRAW_BLOCK - 1) / per::DRAW_BLOCK)) return set_err(REX_ERR_ARG, "%s: n = %lld is more than one launch takes", fn, (long long)n);
  per::DrawParams p{b, (long long)n, seed, draw, (long long*)index_out, prob_out};
  hipLaunchKernelGGL(per::per_draw_kernel, dim3(blocks_for(n, per::DRAW_BLOCK)), dim3(per::DRAW_BLOCK), 0, st, p);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

extern "C" int rex_per_draw(rex_t* h, const rex_per_buffers* buf, int64_t n, uint64_t seed, uint64_t draw, int64_t* index_out, float* prob_out,
                            void* stream) {
  REX_ENTER(h, "rex_per_draw");
  REX_NEEDS(h, per_mem, "rex_per_draw", "rex_per_enable");
  per::Buf b;
  if (int rc = per_buf(h, buf, "rex_per_draw", &b)) return rc;
  return launch_per_draw("rex_per_draw", b, n, seed, draw, index_out, prob_out, (hipStream_t)stream);
}

static_assert(per::C_INVALID == 0 && per::C_BAD_ID == 1 && per::N_COUNTERS == 2, "rex_per_read_counters reports the counters in device order");
extern "C" int rex_per_read_counters(rex_t* h, int64_t* out, int clear) {
  REX_ENTER(h, "rex_per_read_counters");
  REX_NEEDS(h, per_mem, "rex_per_read_counters", "rex_per_enable");
  if (!out) return set_err(REX_ERR_ARG, "rex_per_read_counters: null argument");
  return read_counters(h->per_mem, per::N_COUNTERS, out, clear);
}

// ------------------------------------------------------------------------------------------
// the sample family: rex_rbuf_sample / _gather / rex_per_sample through rb_sample_kernel, their _nstep forms through rb_nstep_kernel (a window of up to
// 32 steps behind every id), their _seq forms through rb_seq_kernel (up to 64 consecutive steps copied behind every id)
// ------------------------------------------------------------------------------------------
// The one launch: `p` is what the kernel takes, `s` the rbuf::SampleParams inside it (p itself for the plain kernel); a kernel with a grid of two
// dimensions gives `grid_y`
template <class P>
static int launch_sample(const rex_env* h, const char* fn, void (*kernel)(P), P& p, rbuf::SampleParams& s, int normalise, void* stream,
                         long long (*grid_y)(P&) = nullptr) {
  if (normalise) {
    if (!h->norm_mem) return set_err(REX_ERR_STATE, "%s: normalise needs rex_norm_enable on this handle", fn);
    const rex_norm_config& c = h->norm_cfg;
    s.norm = rbuf::Norm{h->norm.stats, h->norm.rows, c.norm_obs ? 1 : 0, c.norm_reward ? 1 : 0, c.epsilon, c.clip_obs, c.clip_reward};
  }
  if (s.n == 0) return REX_OK;
  const long long blocks = grid_y ? s.n : rbuf::sample_blocks(s.n);   // a kernel with a grid of two dimensions takes a block row per sample
  if (!grid_fits(blocks)) return set_err(REX_ERR_ARG, "%s: n = %lld is more than one launch takes", fn, s.n);
  // 16-byte accesses: with dim a multiple of 4 every row of a 16-byte aligned buffer starts 16-byte aligned
  const rbuf::Buf& b = s.buf;
  s.vec_obs = (b.obs_dim % 4 == 0 && postpass::all_aligned16(b.obs, b.next_obs, s.out.obs, s.out.next_obs)) ? 1 : 0;
  s.vec_act = (b.act_dim % 4 == 0 && postpass::all_aligned16(b.action, s.out.action)) ? 1 : 0;
  s.bad = (unsigned long long*)h->rbuf_mem;
  const long long rows = grid_y ? grid_y(p) : 1;                       // ... and says how many blocks serve it, once the access widths are known
  if (rows > 65535) return set_err(REX_ERR_ARG, "%s: a sample of %lld blocks is more than one launch takes", fn, rows);
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks, (unsigned)rows), dim3(rbuf::BLOCK), 0, (hipStream_t)stream, p);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

// Where the ids come from: given by the caller, drawn uniformly from `size` filled slots, or drawn by priority (which needs both descriptions,
// agreeing on T, and enqueues the draw whose ids become the gather's).
struct GivenIds { const int64_t* index; int64_t n; };
struct UniformIds { int64_t size, n; uint64_t seed, draw; int64_t* index_out; };
struct PriorityIds { const rex_per_buffers* buf; int64_t n; uint64_t seed, draw; int64_t* index_out; float* prob_out; };

// The window behind every id.  A window type names what its kernel takes (Params, with the rbuf::SampleParams at sample()), the kernel and its
// grid_y; set() checks the window arguments against the buffer and puts them, with the outputs only this window has, into the parameters.
static int check_head(const char* fn, int64_t head, long long T) {
  if (head < 0 || head >= T) return set_err(REX_ERR_ARG, "%s: head %lld outside [0, %lld)", fn, (long long)head, T);
  return REX_OK;
}
struct NoWin {
  using Params = rbuf::SampleParams;
  static constexpr bool present = false;
  static constexpr void (*kernel)(Params) = rbuf::rb_sample_kernel;
  static constexpr long long (*grid_y)(Params&) = nullptr;
  static rbuf::SampleParams& sample(Params& p) { return p; }
  int set(const char*, Params&) const { return REX_OK; }
};
struct NstepWin {
  int64_t head; int n_step; double gamma; float* discount; int32_t* steps;
  using Params = nstep::Params;
  static constexpr bool present = true;
  static constexpr void (*kernel)(Params) = nstep::rb_nstep_kernel;
  static constexpr long long (*grid_y)(Params&) = nullptr;
  static rbuf::SampleParams& sample(Params& p) { return p.s; }
  int set(const char* fn, Params& p) const {
    if (n_step < 1 || n_step > nstep::MAX_STEPS) return set_err(REX_ERR_ARG, "%s: n_step %d outside [1, %d]", fn, n_step, nstep::MAX_STEPS);
    if (!(gamma >= 0.0 && gamma <= 1.0)) return set_err(REX_ERR_ARG, "%s: gamma %g is not a finite number in [0, 1]", fn, gamma);
    if (int rc = check_head(fn, head, p.s.buf.T)) return rc;
    p.win = nstep::Win{(long long)head, n_step, gamma}; p.discount = discount; p.steps = steps;
    return REX_OK;
  }
};
struct SeqWin {   // (the obs output of a sequence call holds the next_obs row too; the steps of a thread follow the access widths launch_sample settles)
  int64_t head; int seq_len; float* mask; int32_t* length;
  using Params = seq::Params;
  static constexpr bool present = true;
  static constexpr void (*kernel)(Params) = seq::rb_seq_kernel;
  static long long grid_y(Params& p) { seq::set_steps(&p); return seq::chunks(p); }
  static rbuf::SampleParams& sample(Params& p) { return p.s; }
  int set(const char* fn, Params& p) const {
    if (seq_len < 1 || seq_len > seq::MAX_LEN) return set_err(REX_ERR_ARG, "%s: seq_len %d outside [1, %d]", fn, seq_len, seq::MAX_LEN);
    if (int rc = check_head(fn, head, p.s.buf.T)) return rc;
    p.win = seq::Win{(long long)head, seq_len}; p.mask = mask; p.length = length;
    return REX_OK;
  }
};

// the row outputs every sample call has (next_obs null for a sequence call)
struct SampleOut { float* obs; float* next_obs; void* action; float* reward; float* done; };

// Every sample call behind its REX_ENTER / REX_NEEDS.  The order of the checks is the contract (the first error of a call with several bad arguments):
// the buffer description(s), the window, the id source, then launch_sample's.
template <class Ids, class Win>
static int sample_call(const rex_env* h, const char* fn, const rex_rbuf_buffers* rb, const Ids& ids, const Win& win, int normalise, const SampleOut& out,
                       void* stream) {
  constexpr bool uniform = std::is_same_v<Ids, UniformIds>, priority = std::is_same_v<Ids, PriorityIds>;
  typename Win::Params p{};
  rbuf::SampleParams& s = Win::sample(p);
  per::Buf pb;
  if constexpr (priority) {
    if (int rc = per_buf(h, ids.buf, fn, &pb)) return rc;
    if (int rc = rbuf_buf(h, rb, fn, &s.buf)) return rc;
    if (rb->T != ids.buf->T) return set_err(REX_ERR_ARG, "%s: the two descriptions disagree on T (%lld and %lld)", fn, (long long)rb->T, (long long)ids.buf->T);
  } else if (int rc = rbuf_buf(h, rb, fn, &s.buf)) return rc;
  if (int rc = win.set(fn, p)) return rc;
  const int64_t* index = nullptr;   // where the kernel finds the ids (null: it draws them) ...
  int64_t filled = s.buf.T;         // ... out of how many slots
  if constexpr (uniform) {
    if (ids.size < 1 || ids.size > s.buf.T) return set_err(REX_ERR_ARG, "%s: size %lld outside [1, %lld]", fn, (long long)ids.size, s.buf.T);
    if constexpr (Win::present)
      if (ids.size < s.buf.T && win.head != ids.size - 1)
        return set_err(REX_ERR_ARG, "%s: a ring that is not full (size %lld < %lld) has head == size - 1, not %lld", fn, (long long)ids.size, s.buf.T,
                       (long long)win.head);
    if (ids.n < 0) return set_err(REX_ERR_ARG, "%s: n must be >= 0", fn);
    filled = ids.size; s.seed = ids.seed; s.draw = ids.draw;
  } else if constexpr (priority) {   // the normalise state BEFORE the draw is enqueued
    if (normalise && !h->norm_mem) return set_err(REX_ERR_STATE, "%s: normalise needs rex_norm_enable on this handle", fn);
    if (int rc = launch_per_draw(fn, pb, ids.n, ids.seed, ids.draw, ids.index_out, ids.prob_out, (hipStream_t)stream)) return rc;
    index = ids.index_out;
  } else {
    if (ids.n < 0 || (ids.n > 0 && !ids.index)) return set_err(REX_ERR_ARG, "%s: n must be >= 0 and index given", fn);
    index = ids.index;
  }
  s.index = (const long long*)index; s.n = ids.n; s.N = (long long)filled * h->B;
  int64_t* index_out = nullptr;     // a uniform draw reports its ids; the other callers have them
  if constexpr (uniform) index_out = ids.index_out;
  s.out = rbuf::Out{(uint32_t*)out.obs, (uint32_t*)out.next_obs, (uint32_t*)out.action, out.reward, out.done, (long long*)index_out};
  return launch_sample(h, fn, Win::kernel, p, s, normalise, stream, Win::grid_y);
}

extern "C" int rex_rbuf_sample(rex_t* h, const rex_rbuf_buffers* buf, int64_t size, int64_t n, uint64_t seed, uint64_t draw, int normalise,
                               float* obs_out, float* next_obs_out, void* action_out, float* reward_out, float* done_out, int64_t* index_out,
                               void* stream) {
  REX_ENTER(h, "rex_rbuf_sample");
  REX_NEEDS(h, rbuf_mem, "rex_rbuf_sample", "rex_rbuf_enable");
  return sample_call(h, "rex_rbuf_sample", buf, UniformIds{size, n, seed, draw, index_out}, NoWin{}, normalise,
                     SampleOut{obs_out, next_obs_out, action_out, reward_out, done_out}, stream);
}

extern "C" int rex_rbuf_gather(rex_t* h, const rex_rbuf_buffers* buf, const int64_t* index, int64_t n, int normalise, float* obs_out,
                               float* next_obs_out, void* action_out, float* reward_out, float* done_out, void* stream) {
  REX_ENTER(h, "rex_rbuf_gather");
  REX_NEEDS(h, rbuf_mem, "rex_rbuf_gather", "rex_rbuf_enable");
  return sample_call(h, "rex_rbuf_gather", buf, GivenIds{index, n}, NoWin{}, normalise, SampleOut{obs_out, next_obs_out, action_out, reward_out, done_out},
                     stream);
}

extern "C" int rex_per_sample(rex_t* h, const rex_rbuf_buffers* rb, const rex_per_buffers* buf, int64_t n, uint64_t seed, uint64_t draw,
                              int normalise, float* obs_out, float* next_obs_out, void* action_out, float* reward_out, float* done_out,
                              int64_t* index_out, float* prob_out, void* stream) {
  REX_ENTER(h, "rex_per_sample");
  REX_NEEDS(h, per_mem, "rex_per_sample", "rex_per_enable");
  REX_NEEDS(h, rbuf_mem, "rex_per_sample", "rex_rbuf_enable");
  return sample_call(h, "rex_per_sample", rb, PriorityIds{buf, n, seed, draw, index_out, prob_out}, NoWin{}, normalise,
                     SampleOut{obs_out, next_obs_out, action_out, reward_out, done_out}, stream);
}

extern "C" int rex_rbuf_gather_nstep(rex_t* h, const rex_rbuf_buffers* buf, const int64_t* index, int64_t n, int64_t head, int n_step, double gamma,
                                     int normalise, float* obs_out, float* next_obs_out, void* action_out, float* reward_out, float* done_out,
                                     float* discount_out, int32_t* steps_out, void* stream) {
  REX_ENTER(h, "rex_rbuf_gather_nstep");
  REX_NEEDS(h, rbuf_mem, "rex_rbuf_gather_nstep", "rex_rbuf_enable");
  return sample_call(h, "rex_rbuf_gather_nstep", buf, GivenIds{index, n}, NstepWin{head, n_step, gamma, discount_out, steps_out}, normalise,
                     SampleOut{obs_out, next_obs_out, action_out, reward_out, done_out}, stream);
}

extern "C" int rex_rbuf_sample_nstep(rex_t* h, const rex_rbuf_buffers* buf, int64_t size, int64_t head, int64_t n, uint64_t seed, uint64_t draw,
                                     int n_step, double gamma, int normalise, float* obs_out, float* next_obs_out, void* action_out,
                                     float* reward_out, float* done_out, float* discount_out, int32_t* steps_out, int64_t* index_out, void* stream) {
  REX_ENTER(h, "rex_rbuf_sample_nstep");
  REX_NEEDS(h, rbuf_mem, "rex_rbuf_sample_nstep", "rex_rbuf_enable");
  return sample_call(h, "rex_rbuf_sample_nstep", buf, UniformIds{size, n, seed, draw, index_out}, NstepWin{head, n_step, gamma, discount_out, steps_out},
                     normalise, SampleOut{obs_out, next_obs_out, action_out, reward_out, done_out}, stream);
}

extern "C" int rex_per_sample_nstep(rex_t* h, const rex_rbuf_buffers* rb, const rex_per_buffers* buf, int64_t n, int64_t head, uint64_t seed, uint64_t draw,
                                    int n_step, double gamma, int normalise, float* obs_out, float* next_obs_out, void* action_out, float* reward_out,
                                    float* done_out, float* discount_out, int32_t* steps_out, int64_t* index_out, float* prob_out, void* stream) {
  REX_ENTER(h, "rex_per_sample_nstep");
  REX_NEEDS(h, per_mem, "rex_per_sample_nstep", "rex_per_enable");
  REX_NEEDS(h, rbuf_mem, "rex_per_sample_nstep", "rex_rbuf_enable");
  return sample_call(h, "rex_per_sample_nstep", rb, PriorityIds{buf, n, seed, draw, index_out, prob_out},
                     NstepWin{head, n_step, gamma, discount_out, steps_out}, normalise, SampleOut{obs_out, next_obs_out, action_out, reward_out, done_out}, stream);
}

extern "C" int rex_rbuf_gather_seq(rex_t* h, const rex_rbuf_buffers* buf, const int64_t* index, int64_t n, int64_t head, int seq_len, int normalise,
                                   float* obs_out, void* action_out, float* reward_out, float* done_out, float* mask_out, int32_t* length_out,
                                   void* stream) {
  REX_ENTER(h, "rex_rbuf_gather_seq");
  REX_NEEDS(h, rbuf_mem, "rex_rbuf_gather_seq", "rex_rbuf_enable");
  return sample_call(h, "rex_rbuf_gather_seq", buf, GivenIds{index, n}, SeqWin{head, seq_len, mask_out, length_out}, normalise,
                     SampleOut{obs_out, nullptr, action_out, reward_out, done_out}, stream);
}

extern "C" int rex_rbuf_sample_seq(rex_t* h, const rex_rbuf_buffers* buf, int64_t size, int64_t head, int64_t n, uint64_t seed, uint64_t draw,
                                   int seq_len, int normalise, float* obs_out, void* action_out, float* reward_out, float* done_out,
                                   float* mask_out, int32_t* length_out, int64_t* index_out, void* stream) {
  REX_ENTER(h, "rex_rbuf_sample_seq");
  REX_NEEDS(h, rbuf_mem, "rex_rbuf_sample_seq", "rex_rbuf_enable");
  return sample_call(h, "rex_rbuf_sample_seq", buf, UniformIds{size, n, seed, draw, index_out}, SeqWin{head, seq_len, mask_out, length_out}, normalise,
                     SampleOut{obs_out, nullptr, action_out, reward_out, done_out}, stream);
}

extern "C" int rex_per_sample_seq(rex_t* h, const rex_rbuf_buffers* rb, const rex_per_buffers* buf, int64_t n, int64_t head, uint64_t seed, uint64_t draw,
                                  int seq_len, int normalise, float* obs_out, void* action_out, float* reward_out, float* done_out, float* mask_out,
                                  int32_t* length_out, int64_t* index_out, float* prob_out, void* stream) {
  REX_ENTER(h, "rex_per_sample_seq");
  REX_NEEDS(h, per_mem, "rex_per_sample_seq", "rex_per_enable");
  REX_NEEDS(h, rbuf_mem, "rex_per_sample_seq", "rex_rbuf_enable");
  return sample_call(h, "rex_per_sample_seq", rb, PriorityIds{buf, n, seed, draw, index_out, prob_out}, SeqWin{head, seq_len, mask_out, length_out}, normalise,
                     SampleOut{obs_out, nullptr, action_out, reward_out, done_out}, stream);
}
