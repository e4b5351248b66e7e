/*
 * rex.h -- C-ABI of the MI355X-native batched domain-randomised locomotion simulator.
 *
 * This is the drop-in boundary for the hot path named in BASELINE.json:north_star:
 * the per-instance forward-dynamics step() and the reset()-time xi sampling of the
 * random_envs environments, batched one environment per GPU lane.
 *
 * The reference (gabrieletiboni/random-envs) has no FFI of its own: its native boundary is
 * mujoco-py's Cython binding (MjSim.step / forward / reset / get_state / set_state and raw
 * views into MjModel / MjData).  Each entry point below cites the reference interface it
 * replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - plain C, no C++ / torch types; every pointer marked [dev] is a caller-owned DEVICE
 *     pointer (e.g. torch.Tensor.data_ptr()), every pointer marked [host] is host memory.
 *   - all calls return 0 on success or a negative rex_status; rex_last_error() gives the
 *     message (thread-local).  No C++ exception crosses this boundary.  (The reference raises
 *     Python exceptions, or drops into pdb on MujocoException: jinja_mujoco_env.py:153-164.)
 *   - kernels are enqueued asynchronously on the caller's HIP stream (`stream`, a hipStream_t
 *     passed as void*, NULL = default stream).  No allocation or synchronisation in
 *     rex_step / rex_reset.
 *   - internal state is SoA [field][env]; I/O buffers are SoA too: obs is [obs_dim][batch],
 *     action is [act_dim][batch], xi is [task_dim][batch] (a torch [batch, dim] view is the
 *     zero-copy transpose).  reward is float[batch], done / truncated are uint8[batch].  The row-major calls (rex_step_rows,
 *     rex_reset_rows) take action [batch][act_dim] and obs [batch][obs_dim] instead; everything else keeps its shape.
 *   - a handle is bound to one device; calls on one handle are not re-entrant.  Every entry point that enqueues work, copies or
 *     synchronises makes the handle's device the calling thread's current device first, so one thread may drive one handle per GPU.
 *   - environment: REX_LANES / REX_PAIR / REX_ROLLED / REX_HUM_PAIR / REX_HUM_FUSED_RESET / REX_FUSED_DERIVE (launch shape) and
 *     REX_FAST / REX_LS_MAX / REX_LS_FREE / REX_WARM / REX_CORR (solver schedule) are A/B and test knobs: rex_create honours them only
 *     with REX_ALLOW_TUNING=1 and otherwise REFUSES to create a handle while one is set (REX_ERR_STATE).  Nothing else is read from
 *     the environment.
 */
#ifndef REX_H_
#define REX_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rex_env rex_t;

/* env_kind: one per kinematic chain of the reference. */
enum rex_env_kind {
  REX_CARTPOLE    = 0, /* random_envs/random_cartpole.py:19            */
  REX_HOPPER      = 1, /* random_envs/jinja/random_hopper.py:16        */
  REX_HALFCHEETAH = 2, /* random_envs/jinja/random_half_cheetah.py:17  */
  REX_WALKER2D    = 3, /* random_envs/jinja/random_walker2d.py:19      */
  REX_HUMANOID    = 4  /* random_envs/jinja/random_humanoid.py:27      */
};

/* dr_type of RandomEnv.set_dr_distribution (random_envs/random_env.py:72-90). */
enum rex_dr_type {
  REX_DR_NONE         = 0,
  REX_DR_UNIFORM      = 1, /* params = [lo0,hi0,lo1,hi1,...]     random_env.py:102-107 */
  REX_DR_TRUNCNORM    = 2, /* params = [mean0,std0,...]          random_env.py:109-114 */
  REX_DR_GAUSSIAN     = 3, /* params = [mean0,std0,...]          random_env.py:116-121 */
  REX_DR_FULLGAUSSIAN = 4  /* params = [mean(d), chol(cov)(d*d, row-major lower), lo(d), hi(d)]
                              random_env.py:123-127,192-198,205-220 */
};

enum rex_status {
  REX_OK            =  0,
  REX_ERR_ARG       = -1, /* bad argument (unknown env kind / dr type / sizes)   */
  REX_ERR_HIP       = -2, /* a HIP runtime call failed                           */
  REX_ERR_STATE     = -3, /* call sequence error (e.g. sampling before set_dr)   */
  REX_ERR_UNSUPPORTED = -4
};

/* Static description of an env kind (dims of SURVEY.md section 8 table). */
typedef struct rex_dims {
  int nq, nv, act_dim, obs_dim, task_dim;
  int frame_skip;
  int max_episode_steps; /* 500 for all 13 ids, e.g. random_hopper.py:155-166 */
  int discrete_action;   /* 1 for CartPole (Discrete(2), random_cartpole.py:96) */
  float dt;              /* model timestep * frame_skip, jinja_mujoco_env.py:166-168 */
  float act_low, act_high; /* actuator_ctrlrange, jinja_mujoco_env.py:99-103 */
  int n_info;            /* per-term reward rows rex_set_info_buffer exposes: 2 for the planar chains
                            (reward_run, reward_ctrl: random_half_cheetah.py:105-110), 4 for the humanoid
                            (reward_linvel, reward_quadctrl, reward_alive, reward_impact: random_humanoid.py:182-187), 0 CartPole */
  int n_aux;             /* rows of sim data that outlive a step besides (qpos, qvel): the humanoid's data.xipos[:,0]
                            (14 bodies) left by the last mj_forward, which mass_center() reads BEFORE the next
                            do_simulation (random_humanoid.py:22-25,162); 0 for the other chains */
} rex_dims;

/* variant: 0 = regular id, 1 = the "Unmodeled" id of the same chain (e.g. random_hopper_unmodeled.py:16-43): a
 * prefix of xi is frozen at 0.8x nominal and leaves the task vector, so task_dim shrinks (3 / 5 / 9). */
int rex_get_dims(int env_kind, int variant, rex_dims* out);

/* Replaces MujocoEnv.__init__ / build_model (jinja_mujoco_env.py:43-97): load_model_from_xml +
 * MjSim for `batch` environments at once.  `env_offset` is the global index of this handle's
 * first env: RNG streams are keyed by the GLOBAL env index so results do not depend on how a
 * batch is sharded over GPUs.  `variant` 0 = regular id, 1 = "Unmodeled" id. */
int rex_create(int env_kind, int variant, int64_t batch, int device_id, uint64_t seed,
               int64_t env_offset, rex_t** out);
int rex_destroy(rex_t* h);

/* RandomEnv.set_dr_distribution (random_env.py:72-127).  `params` [host] layout per rex_dr_type;
 * `lower_bounds` [host, task_dim] = get_task_lower_bound(i) (e.g. random_hopper.py:60-72), used by
 * the truncnorm resampling rule (random_env.py:153-171). May be NULL for the other types. */
int rex_set_dr(rex_t* h, int dr_type, const float* params, int n_params, const float* lower_bounds);
/* RandomEnv.set_dr_training (random_env.py:41-46). */
int rex_set_dr_training(rex_t* h, int flag);
/* set_endless (random_env.py:51-60); `noisy` ctor kwarg + noise_level (random_hopper.py:17-28);
 * noise_var < 0 keeps the env's reference default. */
int rex_set_flags(rex_t* h, int endless, int noisy, float noise_var);
/* auto-reset of finished lanes inside rex_step (SB3 VecEnv convention used by the reference's
 * downstream, README.md:68); time-limit truncation at max_episode_steps (gym TimeLimit). */
int rex_set_autoreset(rex_t* h, int autoreset, int time_limit);
/* seed(): MujocoEnv.seed (jinja_mujoco_env.py:109-111). Re-keys the Philox streams. */
int rex_seed(rex_t* h, uint64_t seed);

/* MujocoEnv.reset + reset_model (jinja_mujoco_env.py:141-144, random_hopper.py:112-120):
 * lanes with mask[i]!=0 (all lanes if mask==NULL) get qpos0/qvel0 + init noise, a fresh xi when
 * dr_training is on, and their observation written to obs_out [dev, obs_dim*batch] (may be NULL). */
int rex_reset(rex_t* h, const uint8_t* mask, float* obs_out, void* stream);

/* step(): RandomHopperEnv.step etc. (random_hopper.py:83-98) = do_simulation
 * (jinja_mujoco_env.py:170-173: ctrl <- a; frame_skip x sim.step()) + reward + done + _get_obs.
 * action [dev]: float[act_dim*batch] (CartPole: int32[batch], values 0/1).
 * Optional outputs (NULL to skip): truncated_out (TimeLimit.truncated), terminal_obs_out
 * (observation before auto-reset). */
int rex_step(rex_t* h, const void* action, float* obs_out, float* reward_out, uint8_t* done_out,
             uint8_t* truncated_out, float* terminal_obs_out, void* stream);

/* Row-major calls: the reference's own loop, `obs, reward, done, info = env.step(action)` over action[batch, act_dim] and
 * obs[batch, obs_dim] (test_random_policy.py:25-32, random_hopper.py:83-98), with nothing between the caller's buffers and the kernels: the
 * planar chains' and the cart-pole's step and reset kernels read and write the rows themselves (a compile-time layout of the same kernels, so
 * the state, the counters and every value are those of rex_step / rex_reset, bit for bit), and either layout may be used on a handle at any
 * time.  reward, done, truncated and the info buffer keep their [batch] and [n_info][batch] shapes.
 *
 * rex_rows_enable allocates what the handle's kind needs for these calls and is idempotent; rex_destroy frees it.  Only the humanoid needs
 * anything: its kernels keep their SoA buffers, so its row-major calls run them into staging of the handle -- action [17][batch], obs and
 * terminal obs [376][batch] each, 769 floats per env, roughly 100 MB at 32 768 envs -- between an action kernel and a tiled transposer (three
 * launches beside a 1.9 ms step; the reset launch as well where the auto-reset is not fused).  Elsewhere it is a no-op and optional.  The
 * call allocates (and so synchronises the device). */
int rex_rows_enable(rex_t* h);
/* MujocoEnv.reset + reset_model (jinja_mujoco_env.py:141-144, random_hopper.py:112-120) as rex_reset does it, the observation of the
 * masked lanes (all lanes if mask==NULL) written to obs_rows [dev, batch*obs_dim, row-major; required].  Rows of unmasked envs are not
 * written.  CartPole: obs_rows 16-byte aligned (one store per row). */
int rex_reset_rows(rex_t* h, const uint8_t* mask, float* obs_rows /*[B, obs_dim]*/, void* stream);
/* step() (random_hopper.py:83-98; the loop of test_random_policy.py:25-32) as rex_step does it -- same state transitions, counters, timing
 * bracket and auto-reset -- with action_rows [dev]: float[batch*act_dim] row-major (CartPole: int32[batch]), obs_rows and terminal_obs_rows
 * [dev, batch*obs_dim, row-major].  done_out / truncated_out bytes are 0 or 1 (a caller may allocate them as bool).  terminal_obs_rows
 * (NULL to skip, like truncated_out) is DEFINED ON THE ROWS WHOSE done IS SET; the other rows are left as they were.  REX_ERR_ARG for a null required buffer (or a misaligned CartPole row buffer),
 * REX_ERR_STATE for a humanoid handle without rex_rows_enable; neither launches anything. */
int rex_step_rows(rex_t* h, const void* action_rows, float* obs_rows, float* reward_out, uint8_t* done_out,
                  uint8_t* truncated_out /*nullable*/, float* terminal_obs_rows /*nullable*/, void* stream);

/* Offline replay of logged transitions under candidate xi (get_full_mjstate + set_sim_state + step: random_hopper.py:128-152,
 * random_half_cheetah.py:136-158, random_walker2d.py:161-185, random_humanoid.py:244-270, and the Unmodeled task files'
 * copies of them): one env.step per lane from the CALLER's qpos [dev, nq*batch], qvel [dev, nv*batch], xi [dev, task_dim*batch]
 * (the reduced task for the Unmodeled ids), action [dev, act_dim*batch] into obs_out / reward_out / done_out.  Nothing of the
 * handle is read back or changed: state, task, step / episode counters, diagnostic counters, RNG position.  Hopper and
 * half-cheetah: ONE launch.  Walker2d: its per-env geometry follows the xi lengths (set_task rebuilds the model,
 * random_walker2d.py:106-113), so a derive launch into replay scratch precedes the step launch.  Humanoid: the forward
 * launch of set_state (data.xipos for mass_center(), jinja_mujoco_env.py:154) precedes it.  Unmodeled ids: one scatter
 * launch places the reduced task over the handle's frozen rows in a scratch copy of the full xi block.  The scratch is
 * allocated by the first such call (which therefore synchronises the device) and belongs to the handle: issue the replays of one
 * handle on one stream at a time.  RandomCartPole: REX_ERR_UNSUPPORTED (the reference has no such helpers for it). */
int rex_replay(rex_t* h, const float* qpos, const float* qvel, const float* xi, const float* action,
               float* obs_out, float* reward_out, uint8_t* done_out, void* stream);

/* get_sim_state / set_sim_state (random_hopper.py:148-152), MujocoEnv.set_state
 * (jinja_mujoco_env.py:146-154), state_vector (:231-235). qpos [dev, nq*batch], qvel [dev, nv*batch].
 * CartPole: qpos = (x, theta), qvel = (x_dot, theta_dot). */
int rex_get_state(rex_t* h, float* qpos, float* qvel, void* stream);
int rex_set_state(rex_t* h, const float* qpos, const float* qvel, void* stream);
/* get_task / set_task (random_hopper.py:75-80 etc.). xi [dev, task_dim*batch]. */
int rex_get_task(rex_t* h, float* xi, void* stream);
int rex_set_task(rex_t* h, const float* xi, void* stream);
/* set_random_task (random_env.py:37-39) for the masked lanes, without touching their state. */
int rex_set_random_task(rex_t* h, const uint8_t* mask, void* stream);
/* current observation of every lane (_get_obs, random_hopper.py:100-110), without noise. */
int rex_get_obs(rex_t* h, float* obs_out, void* stream);

/* The rest of the sim state get_sim_state returns (random_hopper.py:148-152: MjSimState incl. time) and the
 * TimeLimit wrapper's elapsed-step count: per-lane step counter t [dev, int32 batch], episode index
 * [dev, uint32 batch] (together they key the Philox streams, so restoring them makes a resume RNG-exact and
 * time-limit-exact) and the done flags [dev, uint8 batch]. */
int rex_get_counters_state(rex_t* h, int32_t* t, uint32_t* episode, uint8_t* done, void* stream);
int rex_set_counters_state(rex_t* h, const int32_t* t, const uint32_t* episode, const uint8_t* done, void* stream);
/* The remaining MjData a bit-exact resume needs (rex_dims.n_aux rows, [dev, n_aux*batch]); rex_set_state refreshes it
 * with sim.forward() like the reference's set_state, so restore it AFTER the state. */
int rex_get_aux(rex_t* h, float* aux, void* stream);
int rex_set_aux(rex_t* h, const float* aux, void* stream);
/* RandomEnv.sample_task / sample_tasks (random_env.py:145-203) WITHOUT set_task: one xi per lane into
 * xi_out [dev, task_dim*batch]; `draw_index` selects the draw (stream family separate from the reset streams);
 * neither the current task nor the episode counters change. */
int rex_sample_task(rex_t* h, float* xi_out, uint64_t draw_index, void* stream);
/* The `info` dict of step(): per-term rewards (random_half_cheetah.py:110 reward_run / reward_ctrl,
 * random_humanoid.py:182-187 reward_linvel / reward_quadctrl / reward_alive / reward_impact) written by every
 * later rex_step into info [dev, n_info*batch] (rex_dims.n_info rows; NULL switches it off). */
int rex_set_info_buffer(rex_t* h, float* info);
/* One lane's (qpos, qvel, xi) to HOST memory for an external viewer: the data MujocoEnv.render reads from the
 * sim (jinja_mujoco_env.py:175-226; CartPole: random_cartpole.py:231-283). Synchronises the device. */
int rex_export_lane(rex_t* h, int64_t lane, float* qpos /*[host, nq]*/, float* qvel /*[host, nv]*/, float* xi /*[host, task_dim]*/);

/* number of env-steps executed by this handle (host counter; the only quantity the multi-GPU
 * path reduces across ranks). */
int64_t rex_step_count(const rex_t* h);
/* device-side diagnostics accumulated since creation: [0] lane-steps that left a non-finite element in qpos or qvel -- in every kind such a
 * step returns terminated = 1 and TimeLimit.truncated = 0, under set_endless as well, so the auto-reset restarts the lane; with the auto-reset
 * off the lane stays done and is counted once per step (rex_replay counts nothing); a non-finite action that leaves the state finite is not counted,
 * [1] gaussian-DR draws that failed the reference's 3-attempt rule (random_env.py:173-190),
 * [2] constraint solves that hit the iteration cap. Copies 4 int64 to `out` [host]; synchronises. */
int rex_get_counters(rex_t* h, int64_t* out);

/* the launch shape rex_create picked for this handle from its batch and the GPU's SIMD count (rex_set_launch_shape and,
 * under REX_ALLOW_TUNING=1, the REX_LANES / REX_PAIR / REX_ROLLED / REX_HUM_PAIR knobs override): out[0] lanes per workgroup of the step launch (two lanes per env: 64; 32 / 16 for a
 * walker2d / half-cheetah batch of 8 .. 16 envs per SIMD, where narrower waves still all get a SIMD; one lane
 * per env: 32, 64 past 32 768 envs), out[1] 1 = the planar step runs
 * two lanes per env, out[2] 1 = hopper step on the 256-register kernel with the rolled general solver (two waves per SIMD), out[3] 1 = the
 * humanoid step runs two lanes per env.  No reference counterpart (the reference steps one MjSim on one core); bench.py names the launched
 * kernel from it.  Writes 4 int32 to `out` [host]. */
int rex_get_launch_shape(const rex_t* h, int32_t* out);
/* Pins the launch shape of a handle (same four int32 as rex_get_launch_shape, [host]; -1 keeps a field): every shape runs the same solver to
 * the same minimiser, but which solver instantiation a wave enters depends on the shape, so two runs agree bit for bit only under the same
 * shape.  Unpinned is the default: every handle runs the shape rex_create picked for its own batch.  sharding.pin_global_shape (opt-in; shard_strong
 * only places the shard boundaries) pins a shard to the shape the GLOBAL batch would get on one GPU, which makes an index-sharded run reproduce the
 * single-GPU trajectories exactly.  The walker2d auto-reset under DR derives the new geometry inside the step kernel below 524 288 envs per GPU and
 * in a launch of its own from there; that choice is not part of the shape and the two give the same bits.  Pure host bookkeeping (the shape is read at launch time); REX_ERR_ARG for a shape the env kind has no kernel
 * for.  No reference counterpart. */
int rex_set_launch_shape(rex_t* h, const int32_t* shape);

/* duration in ms of the sampled rex_step kernel launches since the last enable / read (at most the last 8192), measured
 * with HIP events on the launch stream; returns the number of samples written.  The two event packets of a bracketed launch
 * cost about 8 us of stream time, so throughput runs sample every n-th launch.  rex_enable_timing(1) creates
 * the event pool (the only allocation of the timing path: rex_step itself never allocates). */
int rex_enable_timing(rex_t* h, int every);   /* 0 = off, n >= 1 = bracket every n-th rex_step launch */
int rex_read_timing(rex_t* h, float* ms_out, int max_n);

/* ---- observation / reward normalisation and episode statistics: an opt-in post-pass of rex_step / rex_reset -------------------
 * What an RL loop places directly above step(): stable-baselines3's VecNormalize (common/vec_env/vec_normalize.py) with its
 * RunningMeanStd (common/running_mean_std.py), and VecMonitor (common/vec_env/vec_monitor.py) -- the reference's users train
 * through SB3 (README.md:68).  No reference counterpart of its own.  rex_step, rex_reset and their outputs are untouched: the calls
 * below READ the raw buffers rex_step wrote and write normalised values to buffers of the caller (which may be the same buffers:
 * in place works).
 *
 * State: one running (count, mean, var) per observation row and one for the discounted return (obs_dim + 1 rows; initial count
 * 1e-4, mean 0, var 1), and per lane the discounted return `ret`, the episode's raw return and its length.
 *
 * rex_norm_step, with training on:  (1) the observation statistics take in the batch's obs_in (Chan merge with the batch's
 *   population moments; after an auto-reset these are the new episode's first observations, as in SB3), (2) ret = ret*gamma + reward,
 *   (3) the return statistic takes in ret.  Always: obs_out = clip((obs_in - mean) / sqrt(var + epsilon), +-clip_obs),
 *   reward_out = clip(reward_in / sqrt(var_ret + epsilon), +-clip_reward), term_obs_out of the lanes with done != 0 the same way as
 *   obs_out (other lanes of term_obs_out are left as they were), and finally ret = 0 on the done lanes.
 *   Episode statistics: ep_return += reward_in, ep_len += 1; a done lane writes its totals to ep_return_out [dev, double batch] /
 *   ep_len_out [dev, int32 batch] (other lanes are left as they were), adds them to three device aggregates (episodes finished, sum of
 *   returns, sum of lengths) and starts again from 0.
 *   A switch that is off (norm_obs / norm_reward) leaves its statistic, and its output buffers, alone; with norm_reward off ret stays 0.
 *   Optional pointers: obs_in + obs_out (together; NULL skips the observation rows), term_obs_in + term_obs_out (together), reward_out,
 *   ep_return_out, ep_len_out.
 * rex_norm_reset: the lanes with mask[i] != 0 (all when mask == NULL) get ret = 0 and fresh episode totals; with training on the
 *   observation statistics take in obs_in of THOSE lanes (the batch count is their number); their normalised observations go to
 *   obs_out (other lanes of obs_out are left as they were).
 * A non-finite input element is left out of its row's batch moments (so the count is kept per row; all rows agree while inputs are
 *   finite) and counted; its normalised output is whatever the arithmetic gives.
 *
 * Two launches per call on `stream`, no allocation, no synchronisation; results do not depend on anything but the data (fixed
 * reduction order: two runs agree bit for bit).  rex_norm_enable is the only allocating call (it synchronises; calling it again
 * re-initialises the state under the new config); every other rex_norm_* call before it returns REX_ERR_STATE. */
typedef struct rex_norm_config {
  double gamma;        /* 0.99 */
  double epsilon;      /* 1e-8 */
  double clip_obs;     /* 10   */
  double clip_reward;  /* 10   */
  int norm_obs, norm_reward, training;   /* 1, 1, 1 */
} rex_norm_config;
int rex_norm_enable(rex_t* h, const rex_norm_config* cfg /* NULL = the defaults above */);
int rex_norm_set_training(rex_t* h, int flag);
int rex_norm_reset(rex_t* h, const uint8_t* mask, const float* obs_in, float* obs_out, void* stream);
int rex_norm_step(rex_t* h, const float* obs_in, const float* reward_in, const uint8_t* done, const float* term_obs_in,
                  float* obs_out, float* reward_out, float* term_obs_out, double* ep_return_out, int32_t* ep_len_out, void* stream);
/* the running statistics as [host] double[3 * (obs_dim + 1)]: the counts of every row, then the means, then the variances (the
 * return row last in each).  Both synchronise the device. */
int rex_norm_get_stats(rex_t* h, double* out);
int rex_norm_set_stats(rex_t* h, const double* in);
/* the per-lane state [dev]: ret, ep_return (double batch), ep_len (int32 batch); with the statistics it makes a resume exact. */
int rex_norm_get_lane_state(rex_t* h, double* ret, double* ep_return, int32_t* ep_len, void* stream);
int rex_norm_set_lane_state(rex_t* h, const double* ret, const double* ep_return, const int32_t* ep_len, void* stream);
/* out [host, 4 doubles] since the last clearing read: episodes finished, sum of their returns, sum of their lengths, non-finite
 * input elements left out of the statistics.  Synchronises. */
int rex_norm_read_episodes(rex_t* h, double* out, int clear);

/* ---- on-policy rollout buffer: fused store of a step, GAE(lambda), advantage statistics, minibatch gather ----------------------
 * The layer above step() (and above rex_norm_step, when used) in every on-policy loop: stable-baselines3's RolloutBuffer
 * (common/buffers.py: add, compute_returns_and_advantage, get) and the time-limit bootstrap of collect_rollouts
 * (common/on_policy_algorithm.py).  No reference counterpart of its own.  rex_step and rex_norm_* are untouched.
 *
 * Storage belongs to the caller and uses the SoA layout of this interface, T = steps per rollout, B = the handle's batch:
 *   obs [T][obs_dim][B] f32, action [T][act_dim][B] 4-byte words (copied bit for bit: float, or the cart-pole's int32),
 *   reward / value / log_prob / advantage / returns [T][B] f32, done [T][B] uint8.
 * The handle contributes the device, the dims and B, and holds no rollout state: slot indices are arguments, so a rollout captured
 * into a graph replays correctly.  rex_rollout_enable makes the only allocation (a fixed-size scratch for the reduction partials,
 * independent of T, plus the result and counter words; it synchronises); every other rex_rollout_* call before it returns
 * REX_ERR_STATE.  The launching calls neither allocate nor synchronise. */
typedef struct rex_rollout_buffers {
  float* obs;
  void* action;
  float* reward;
  float* value;
  float* log_prob;
  float* advantage;
  float* returns;
  uint8_t* done;
  int64_t T;
} rex_rollout_buffers;
int rex_rollout_enable(rex_t* h);
/* RolloutBuffer.add: ONE launch copies obs (the observation the action was computed from), action, reward, done, value, log_prob
 * [dev, one step each, SoA] into slot t.  truncated [dev, uint8 batch] and terminal_value [dev, float batch] are optional and go
 * together: on lanes with truncated != 0 the stored reward is (float)((double)reward + gamma * (double)terminal_value) -- a product
 * and a sum in fp64, not fused, rounded once.  t outside [0, T): REX_ERR_ARG. */
int rex_rollout_add(rex_t* h, const rex_rollout_buffers* buf, int64_t t, const float* obs, const void* action, const float* reward,
                    const uint8_t* done, const float* value, const float* log_prob, const uint8_t* truncated, const float* terminal_value,
                    double gamma, void* stream);
/* RolloutBuffer.compute_returns_and_advantage in ONE launch (one thread per env, serial in t); done[t] is the flag step t returned,
 * last_value [dev, float batch] the value of the observation after the last step.  For t = T-1 .. 0 per lane, every operand widened
 * to fp64 and every operation a separate IEEE fp64 operation in the order written (A = 0 before t = T-1):
 *   nnt = done[t] ? 0 : 1;  nv = (t == T-1) ? last_value : value[t+1];
 *   delta = (reward[t] + (gamma * nv) * nnt) - value[t];  A = delta + ((gamma * lambda) * nnt) * A;
 *   advantage[t] = (float)A;  returns[t] = (float)(A + value[t]).
 * The result does not depend on the launch shape and equals a numpy fp64 restatement bit for bit. */
int rex_rollout_gae(rex_t* h, const rex_rollout_buffers* buf, const float* last_value, double gamma, double lambda, void* stream);
/* (n, mean, M2) of the whole advantage buffer in fp64, TWO launches: one partial per block (the count is a function of T * B only),
 * merged in a fixed order -- runs of 4 partials in index order, then the runs pairwise over neighbours, a tree whose shape depends on the
 * partial count only -- so two runs agree bit for bit.
 * Non-finite elements are left out and counted.  normalise != 0: the second launch also rewrites advantage in place as
 * (float)((A - mean) / (sqrt(M2 / (n - 1)) + 1e-8)) (the unbiased deviation, as torch.std gives it to SB3's PPO; NaN for n <= 1). */
int rex_rollout_adv_stats(rex_t* h, const rex_rollout_buffers* buf, int normalise, void* stream);
/* out [host, 4 doubles] of the last rex_rollout_adv_stats: n, mean, M2, non-finite elements left out.  Synchronises. */
int rex_rollout_get_adv_stats(rex_t* h, double* out);
/* RolloutBuffer.get for one minibatch, ONE launch: index [dev, int64 n] holds flat sample ids s = t * B + b; the outputs use the
 * learner's layout and are each optional (NULL skips): obs_out [n][obs_dim] and action_out [n][act_dim] ROW-MAJOR, advantage_out /
 * returns_out / value_out / log_prob_out [n].  A pure copy.  An id outside [0, T * B) is never dereferenced: that sample's outputs
 * are zeros and a device counter is incremented (rex_rollout_read_bad_indices). */
int rex_rollout_gather(rex_t* h, const rex_rollout_buffers* buf, const int64_t* index, int64_t n, float* obs_out, void* action_out,
                       float* advantage_out, float* returns_out, float* value_out, float* log_prob_out, void* stream);
/* out [host, 1 int64]: out-of-range sample ids rex_rollout_gather met since the last clearing read.  Synchronises. */
int rex_rollout_read_bad_indices(rex_t* h, int64_t* out, int clear);

/* ---- episode ledger: task, return and length of every finished episode, appended on the device --------------------------------
 * What every domain-randomisation method consumes is WHICH TASK GOT WHICH RETURN (active DR, DORAEMON-style distribution updates,
 * BayRn / SimOpt-style outer loops, return-as-a-function-of-xi evaluation).  With auto-reset and dr_training on, the rex_step launch
 * that finishes an episode also stores the next episode's task over the lane's xi, so after rex_step the finished episode's task is
 * gone; pairing it on the host costs a rex_get_task per step plus a data-dependent nonzero(), i.e. one synchronisation per step.  No
 * reference counterpart of its own.  rex_step, rex_norm_* and rex_rollout_* are untouched; the ledger is an independent opt-in (it
 * duplicates the 12 B per lane of episode totals rex_norm_* keeps).
 *
 * A LEDGER is an append-only table of finished episodes in caller-owned DEVICE memory, SoA over its capacity N:
 *   task      [task_dim][N] f32  the task the episode ran under, rows in rex_get_task's order (the reduced task of the Unmodeled ids)
 *   ep_return [N] f64            sum of the raw rewards of the episode, accumulated in fp64 in step order
 *   ep_len    [N] i32            steps
 *   flags     [N] u8             bit 0: the episode ended by time-limit truncation
 *   env       [N] i64            GLOBAL env index (env_offset + lane)
 *   step      [N] i64            serial number of the rex_eplog_step call that recorded it (0-based, counted since enable)
 * The handle keeps per lane ep_return (f64), ep_len (i32) and a SHADOW TASK [task_dim][B] f32 -- the task in force when the lane's
 * current episode began -- and two device words: `total` (records appended since the last clear, dropped ones included) and `serial`.
 *
 * rex_eplog_step reads the buffers rex_step just wrote (reward [dev, float batch], done [dev, uint8 batch], truncated [dev, uint8
 * batch] or NULL).  For every lane i, in this order:
 *   1. ep_return[i] += (double)reward[i];  ep_len[i] += 1.
 *   2. if done[i] != 0:  r = number of lanes j < i with done[j] != 0, slot = total + r.  If slot < N the record (shadow task of i,
 *      ep_return[i], ep_len[i], flags = (truncated && truncated[i]) ? 1 : 0, env_offset + i, serial) is written to `slot`; otherwise
 *      nothing is written.  Then ep_return[i] = 0, ep_len[i] = 0 and the shadow task of i becomes the lane's CURRENT task: the next
 *      episode's, which the step launch or the masked reset behind it has already stored.
 *   3. after all lanes: total += number of done lanes, then serial += 1.
 * Order: the records of one call are in env-index order and calls are in call order; the table does not depend on launch shape,
 *   block scheduling or timing, so two runs agree bit for bit.
 * Overflow: the earliest N records are kept, the rest are counted (rex_eplog_read).
 * Non-finite rewards accumulate as the arithmetic gives.
 *
 * rex_eplog_sync: the lanes with mask[i] != 0 (all when mask == NULL) re-read their shadow task from the handle's current task;
 *   with restart != 0 their ep_return / ep_len start again from 0.  It is the companion of rex_reset, rex_set_task,
 *   rex_set_random_task, rex_set_state and rex_set_counters_state, in the role rex_norm_reset plays for rex_reset.  A task changed
 *   from outside WITHOUT a sync is not seen: the episode in progress is recorded with the stale shadow task.
 *
 * rex_eplog_enable registers the caller's six pointers and the capacity, allocates the per-lane state and the scan scratch (one count
 *   per block of 256 lanes: a function of the batch only), sets total = serial = 0, zeroes the totals, sets shadow = current task and
 *   synchronises.  It is the only allocating call; calling it again re-initialises under the new buffers; every other rex_eplog_*
 *   call before it returns REX_ERR_STATE; a NULL pointer or capacity <= 0 returns REX_ERR_ARG.
 * rex_eplog_step is TWO launches and rex_eplog_sync ONE on `stream`; neither allocates nor synchronises, and neither keeps host-side
 *   state that changes between calls (total and serial live on the device; no kernel argument differs from call to call).
 *   No atomics and no waiting between blocks: the launch boundary is the barrier. */
typedef struct rex_eplog_buffers {
  float* task;
  double* ep_return;
  int32_t* ep_len;
  uint8_t* flags;
  int64_t* env;
  int64_t* step;
  int64_t capacity;
} rex_eplog_buffers;
int rex_eplog_enable(rex_t* h, const rex_eplog_buffers* buf);
int rex_eplog_step(rex_t* h, const float* reward, const uint8_t* done, const uint8_t* truncated /* may be NULL */, void* stream);
int rex_eplog_sync(rex_t* h, const uint8_t* mask, int restart, void* stream);
/* out [host, 4 int64]: total, dropped = max(0, total - capacity), serial, capacity.  clear != 0 sets total = 0 (the next record goes
 * to slot 0); serial keeps counting.  Synchronises. */
int rex_eplog_read(rex_t* h, int64_t* out, int clear);
/* the per-lane state [dev]: ep_return (double batch), ep_len (int32 batch), shadow_task (float task_dim*batch, SoA); with a drained
 * ledger it makes a resume exact, as rex_norm_get_lane_state / rex_norm_set_lane_state do. */
int rex_eplog_get_lane_state(rex_t* h, double* ep_return, int32_t* ep_len, float* shadow_task, void* stream);
int rex_eplog_set_lane_state(rex_t* h, const double* ep_return, const int32_t* ep_len, const float* shadow_task, void* stream);

/* ---- off-policy replay buffer: fused store of a transition per env, on-device sampling -----------------------------------------
 * The layer above step() in every off-policy loop (SAC / TD3 / DDPG, and every domain-randomisation loop that reuses data across
 * distribution updates): stable-baselines3's ReplayBuffer (common/buffers.py: add, sample, _get_samples) and
 * OffPolicyAlgorithm._store_transition (common/off_policy_algorithm.py).  No reference counterpart of its own.  rex_step, rex_norm_*,
 * rex_rollout_* and rex_eplog_* are untouched.  The names say "rbuf": rex_replay is something else -- the offline replay of LOGGED
 * transitions under candidate xi -- and shares nothing with these calls.
 *
 * Storage belongs to the caller: a ring of T time slots over the handle's batch B in device memory, TRANSITION-MAJOR (a buffer is
 * written once per transition and read at random many times; a whole transition is one contiguous row).  Transition id s = t * B + b:
 *   obs, next_obs [T][B][obs_dim] f32, action [T][B][act_dim] 4-byte words (copied bit for bit: float, or the cart-pole's int32),
 *   reward [T][B] f32, done / timeout [T][B] uint8.
 * The handle contributes the device, the dims and B, and holds no buffer state: slot, fill level, seed and draw number are arguments,
 * as in rex_rollout_*.  rex_rbuf_enable makes the only allocation (the bad-index counter; it synchronises); every other rex_rbuf_* call
 * before it returns REX_ERR_STATE.  The launching calls neither allocate nor synchronise. */
typedef struct rex_rbuf_buffers {
  float* obs;
  float* next_obs;
  void* action;
  float* reward;
  uint8_t* done;
  uint8_t* timeout;
  int64_t T;
} rex_rbuf_buffers;
int rex_rbuf_enable(rex_t* h);
/* ReplayBuffer.add, ONE launch: the SoA buffers rex_step reads and writes -- obs [obs_dim][B] (the observation the action was computed
 * from), action [act_dim][B], reward [B], done [B], next_obs [obs_dim][B] (what rex_step returned, i.e. after the auto-reset), and
 * optionally terminal_obs [obs_dim][B] and truncated [B] -- are transposed into slot t.  For lane b, s = t * B + b:
 *   obs[s][:] = obs[:, b];  action[s][:] = action[:, b];  reward[s] = reward[b];  done[s] = done[b] != 0;
 *   next_obs[s][:] = (terminal_obs && done[b]) ? terminal_obs[:, b] : next_obs[:, b];  timeout[s] = truncated ? truncated[b] != 0 : 0.
 * A pure copy.  t outside [0, T): REX_ERR_ARG. */
int rex_rbuf_add(rex_t* h, const rex_rbuf_buffers* buf, int64_t t, const float* obs, const void* action, const float* reward,
                 const uint8_t* done, const float* next_obs, const float* terminal_obs, const uint8_t* truncated, void* stream);
/* ReplayBuffer.sample, ONE launch, no host-side randomness: `size` is the number of valid slots (1 <= size <= T, else REX_ERR_ARG),
 * N = size * B.  Sample j (0-based) evaluates Philox4x32-10 with key (lo32(seed), hi32(seed)) and counter (lo32(j), hi32(j), lo32(draw),
 * hi32(draw)), takes u = w0 | (w1 << 32), and its id is the high 64 bits of the 128-bit product u * N (bias at most N / 2^64); draws are
 * with replacement and depend on (seed, draw, size, B, j) only.
 * The outputs use the learner's layout and are each optional (NULL skips): obs_out, next_obs_out [n][obs_dim] and action_out
 * [n][act_dim] ROW-MAJOR, reward_out [n] f32, done_out [n] f32 = (done && !timeout) ? 1 : 0 (SB3's dones * (1 - timeouts): a time-limit
 * end still bootstraps), index_out [n] int64 the ids used.
 * normalise != 0 is SB3's sample(batch_size, env=vec_normalize) and needs rex_norm_enable on the handle (else REX_ERR_STATE): the stored
 * values stay raw; the kernel reads the running statistics from device memory as they stand when it runs (stream-ordered behind the last
 * rex_norm_step).  With norm_obs on, obs_out and next_obs_out are clip((x - mean) / sqrt(var + epsilon), +-clip_obs) of their row's
 * statistic; with norm_reward on, reward_out is clip(r / sqrt(var_ret + epsilon), +-clip_reward) -- the arithmetic of rex_norm_step, so
 * under frozen statistics the bits equal what rex_norm_step returns for those values.  A switch that is off leaves its output raw. */
int rex_rbuf_sample(rex_t* h, const rex_rbuf_buffers* buf, int64_t size, int64_t n, uint64_t seed, uint64_t draw, int normalise,
                    float* obs_out, float* next_obs_out, void* action_out, float* reward_out, float* done_out, int64_t* index_out,
                    void* stream);
/* The same launch with the caller's ids: index [dev, int64 n] (prioritised schemes, tests).  An id outside [0, T * B) is never
 * dereferenced: that sample's outputs are zeros and a device counter is incremented (rex_rbuf_read_bad_indices). */
int rex_rbuf_gather(rex_t* h, const rex_rbuf_buffers* buf, const int64_t* index, int64_t n, int normalise, float* obs_out,
                    float* next_obs_out, void* action_out, float* reward_out, float* done_out, void* stream);
/* out [host, 1 int64]: out-of-range ids rex_rbuf_gather met since the last clearing read.  Synchronises. */
int rex_rbuf_read_bad_indices(rex_t* h, int64_t* out, int clear);

/* ---- prioritised replay: per-transition priorities, a sum tree, stratified proportional draws, priority updates --------------------
 * Proportional prioritised experience replay (Schaul et al. 2016, "Prioritized Experience Replay") beside rex_rbuf_*, which stays as it
 * is: the caller of rex_rbuf_gather that draws ids with probability priority / sum of priorities.  No reference counterpart of its own.
 *
 * Storage belongs to the caller, in device memory, for the N = T * B transition ids s = t * B + b of rex_rbuf_* (N <= 2^30, else
 * REX_ERR_ARG):
 *   priority     [N] f32.  A valid priority is finite and > 0; +0.0f marks a slot that is never drawn (empty, or given an invalid value).
 *   tree         [rex_per_tree_len(N)] f64, a 64-ary sum tree.  n_0 = N, n_l = ceil(n_(l-1) / 64) up to the level D >= 1 with n_D = 1
 *                (N = 1 still has a root above its leaf); the array holds the n_1 nodes of level 1 first and the root last;
 *                rex_per_tree_len(N) = sum of n_l over l >= 1 (a host function without a handle; N outside [1, 2^30]: REX_ERR_ARG, i.e. D <= 5).
 *                Node m of level l is the fp64 sum of its children 64 m .. 64 m + 63 of level l - 1 (leaves widened from f32), formed
 *                SERIALLY in index order starting from 0.0; children past n_(l-1) count as 0.0.  That order is the whole definition of a
 *                node's bits: an incremental update, rex_per_rebuild and a restatement in numpy agree bit for bit.
 *   max_priority [1] f32: the largest valid priority seen since rex_per_init (at least 1.0f); what a new transition gets.
 * The handle contributes the device and B and holds no buffer state.  rex_per_enable makes the only allocation (two device counters; it
 * synchronises); every other rex_per_* call that takes a handle returns REX_ERR_STATE before it.  The launching calls neither allocate nor
 * synchronise and keep no host state that changes between calls -- slot, seed and draw number are arguments, so a captured loop
 * replays.  The number of launches of a call depends on D only and is given beside it.  No float atomics and no waiting between blocks:
 * the launch boundary is the barrier; the only atomics are integer atomicMax on the bit patterns of non-negative finite floats (which
 * order like unsigned integers) and integer atomicAdd on the counters.  Two threads that refresh the same node store identical bits. */
typedef struct rex_per_buffers {
  float* priority;
  double* tree;
  float* max_priority;
  int64_t T;
} rex_per_buffers;
int64_t rex_per_tree_len(int64_t N);
int rex_per_enable(rex_t* h);
/* ONE launch: priority <- +0.0f, tree <- 0.0, *max_priority <- 1.0f. */
int rex_per_init(rex_t* h, const rex_per_buffers* buf, void* stream);
/* The companion of rex_rbuf_add for slot t, 2 + max(D - 2, 0) launches: the B leaves t * B .. t * B + B - 1 take *max_priority as it
 * stands in stream order, then every ancestor of them is recomputed (one launch per level below the top two over the nodes above the
 * range, one single-block launch for levels max(1, D - 1) .. D).  t outside [0, T): REX_ERR_ARG. */
int rex_per_add(rex_t* h, const rex_per_buffers* buf, int64_t t, void* stream);
/* 3 + max(D - 2, 0) launches; index [dev, int64 n], priority [dev, f32 n].  Pair j with an id outside [0, N) is never dereferenced, is
 * counted (rex_per_read_counters, out[1]) and plays no further part.  Otherwise a value that is not finite and > 0 becomes +0.0f and is
 * counted as invalid (out[0]) unless it is +-0.  Leaf index[j] <- that value; when an id occurs more than once in one call the LARGEST
 * of its new values is stored (not a max with the old leaf: launch 1 clears the touched leaves, launch 2 is an integer atomicMax on the
 * bits).  *max_priority <- max(*max_priority, every valid new value stored).  Then every ancestor of a touched leaf is recomputed, as in
 * rex_per_add with the nodes above index[j] in place of the range.  n == 0 does nothing. */
int rex_per_update(rex_t* h, const rex_per_buffers* buf, const int64_t* index, const float* priority, int64_t n, void* stream);
/* 1 + D launches: every node recomputed from the leaves as they are (one launch per level), *max_priority <- max(1.0f, every valid
 * leaf).  For buffers restored from a checkpoint, and the cross-check of the incremental path. */
int rex_per_rebuild(rex_t* h, const rex_per_buffers* buf, void* stream);
/* Stratified proportional sampling, ONE launch, no host-side randomness.  Sample j (0-based) of n evaluates the Philox4x32-10 block of
 * rex_rbuf_sample -- key (lo32(seed), hi32(seed)), counter (lo32(j), hi32(j), lo32(draw), hi32(draw)) -- and takes the two words that
 * call leaves unused: u = w2 | (w3 << 32), U = (double)(u >> 11) * 2^-53, x = ((double)j + U) * (total / (double)n) with total = the
 * root; every operation a separate IEEE fp64 operation.  Descent from the root: at a node with children v_0 .. v_63 start with r = 0 and
 * walk k = 0 .. 63: if x < r + v_k choose k, set x <- x - r and descend, else r <- r + v_k.  If no child is chosen (rounding at the upper
 * edge) choose the largest k with v_k > 0 and leave x as it is.  If no child is positive (total == 0): index_out[j] = -1, prob_out[j] = 0.
 * Otherwise index_out[j] = the leaf reached (its priority is > 0) and prob_out[j] = (float)((double)priority[id] / total).
 * index_out [dev, int64 n] and prob_out [dev, f32 n] are required when n > 0.  The result depends on (seed, draw, n, j) and the tree only. */
int rex_per_draw(rex_t* h, const rex_per_buffers* buf, int64_t n, uint64_t seed, uint64_t draw, int64_t* index_out, float* prob_out,
                 void* stream);
/* TWO launches: the draw above, then the launch of rex_rbuf_gather over index_out (outputs and normalise as there; needs rex_rbuf_enable
 * too, and the same T in both descriptions).  An id of -1 meets that launch's guard: zeros, counted in rex_rbuf_read_bad_indices. */
int rex_per_sample(rex_t* h, const rex_rbuf_buffers* rbuf, const rex_per_buffers* per, int64_t n, uint64_t seed, uint64_t draw,
                   int normalise, float* obs_out, float* next_obs_out, void* action_out, float* reward_out, float* done_out,
                   int64_t* index_out, float* prob_out, void* stream);
/* out [host, 2 int64]: invalid priorities and out-of-range ids rex_per_update met since the last clearing read.  Synchronises. */
int rex_per_read_counters(rex_t* h, int64_t* out, int clear);

/* ---- n-step returns sampled from the replay buffer ---------------------------------------------------------------------------------
 * The n-step variant of rex_rbuf_sample / rex_rbuf_gather / rex_per_sample, which stay as they are: what Rainbow, D4PG, R2D2 and n-step
 * SAC / TD3 bootstrap from, r_0 + gamma r_1 + ... + gamma^(m-1) r_(m-1) + gamma^m Q(s_m), formed inside the launch that copies the rows.
 * Storage, handle, rex_rbuf_enable and the rules of the family are those of rex_rbuf_*: REX_ERR_STATE before rex_rbuf_enable, no
 * allocation, no synchronisation, no host state between calls, n == 0 does nothing.
 *
 * New arguments: n_step, an int in [1, 32]; gamma, a finite double in [0, 1]; head, an int64 in [0, T): the slot written most recently.
 * Anything else is REX_ERR_ARG.
 *
 * Sample j has the guarded id s, with t0 = s / B and b = s % B.  Its window is the steps k = 0, 1, ... with t_k = (t0 + k) mod T and
 * s_k = t_k * B + b (the next step of the same env lies B ids further on, modulo T * B).  Step k is the LAST step of the window (so
 * m = k + 1) when the first of these holds:
 *   done[s_k] != 0 || timeout[s_k] != 0   the episode ends there;
 *   t_k == head                           the next slot holds the oldest data of a full ring, or nothing at all;
 *   k == n_step - 1.
 * Every operand is widened to fp64 and every operation is a separate IEEE fp64 operation, never contracted:
 *   acc = reward[s_0];  g = gamma;
 *   for k = 1 .. m-1:   acc = acc + g * reward[s_k];   g = g * gamma;
 * Outputs, each optional (NULL skips), in the layout of rex_rbuf_gather:
 *   obs_out[j]      = the obs row of s_0;            action_out[j] = the action row of s_0;
 *   next_obs_out[j] = the next_obs row of s_(m-1);
 *   reward_out[j]   = (float)acc;
 *   done_out[j]     = (done[s_(m-1)] && !timeout[s_(m-1)]) ? 1 : 0 (a window cut by the head or by a time limit still bootstraps);
 *   discount_out[j] = (float)g, that is gamma^m: what the learner multiplies its target value by;   [n] f32
 *   steps_out[j]    = m;                                                                              [n] int32
 *   index_out[j]    = s in the sampling calls.
 * normalise != 0 behaves as in rex_rbuf_sample: obs / next_obs are normalised with the running statistics as they stand; reward_out is
 * the normalisation of the float32 n-step sum with the return row's statistic -- the return is normalised once, not each term;
 * discount_out, steps_out and done_out are never normalised.
 * An id outside [0, T * B) is never turned into an address: every output of that sample is zero, discount_out and steps_out included,
 * and it is counted in the counter rex_rbuf_read_bad_indices reads.
 * With n_step == 1 the five outputs the plain launch has are bit-identical to rex_rbuf_gather for any head, discount_out is
 * (float)gamma and steps_out is 1. */
/* ONE launch over the caller's ids: index [dev, int64 n]. */
int rex_rbuf_gather_nstep(rex_t* h, const rex_rbuf_buffers* buf, const int64_t* index, int64_t n, int64_t head, int n_step, double gamma,
                          int normalise, float* obs_out, float* next_obs_out, void* action_out, float* reward_out, float* done_out,
                          float* discount_out, int32_t* steps_out, void* stream);
/* ONE launch.  The ids are exactly those of rex_rbuf_sample for the same (seed, draw, size, B, j); every stored id is a valid start,
 * because the window shortens instead.  size outside [1, T], or size < T && head != size - 1 (a ring that has not wrapped was filled from
 * slot 0): REX_ERR_ARG. */
int rex_rbuf_sample_nstep(rex_t* h, const rex_rbuf_buffers* buf, int64_t size, int64_t head, int64_t n, uint64_t seed, uint64_t draw,
                          int n_step, double gamma, int normalise, float* obs_out, float* next_obs_out, void* action_out,
                          float* reward_out, float* done_out, float* discount_out, int32_t* steps_out, int64_t* index_out, void* stream);
/* TWO launches: the unchanged launch of rex_per_draw, then the n-step launch over index_out (needs rex_per_enable too, and the same T
 * in both descriptions).  An id of -1 meets the guard: zeros, counted. */
int rex_per_sample_nstep(rex_t* h, const rex_rbuf_buffers* rbuf, const rex_per_buffers* per, int64_t n, int64_t head, uint64_t seed,
                         uint64_t draw, int n_step, double gamma, int normalise, float* obs_out, float* next_obs_out, void* action_out,
                         float* reward_out, float* done_out, float* discount_out, int32_t* steps_out, int64_t* index_out, float* prob_out,
                         void* stream);

/* ---- sequence windows sampled from the replay buffer -------------------------------------------------------------------------------
 * The sequence variant of rex_rbuf_sample / rex_rbuf_gather / rex_per_sample, which stay as they are: what a recurrent actor / critic
 * (R2D2, recurrent SAC / TD3) or a network fed a history of observations and actions (RMA's adaptation module, UP-OSI, sequence models)
 * trains on -- up to L consecutive steps of one env behind every id, cut at the episode's end, zero-padded, with a validity mask --
 * copied inside one launch.  Storage, handle, rex_rbuf_enable and the rules of the family are those of rex_rbuf_*: REX_ERR_STATE before
 * rex_rbuf_enable, no allocation, no synchronisation, no host state between calls, n == 0 does nothing.
 *
 * New argument: seq_len = L, an int in [1, 64]; head, an int64 in [0, T), is the slot written most recently, as in the n-step calls.
 * Anything else is REX_ERR_ARG.
 *
 * Sample j has the guarded id s, with t0 = s / B and b = s % B.  Its window is the steps k = 0, 1, ... with t_k = (t0 + k) mod T and
 * s_k = t_k * B + b.  Step k is the LAST step of the window (so m = k + 1) when the first of these holds -- the n-step rule with n_step
 * replaced by L:
 *   done[s_k] != 0 || timeout[s_k] != 0   the episode ends there;
 *   t_k == head                           the next slot holds the oldest data of a full ring, or nothing at all;
 *   k == L - 1.
 * Outputs, batch-first, each optional (NULL skips; a skipped buffer is left untouched):
 *   obs_out    [n][L+1][obs_dim] f32           row k < m: the obs row of s_k; row m: the next_obs row of s_(m-1), the observation to
 *                                              bootstrap from; rows > m: zeros.  obs_out[:, :-1] and obs_out[:, 1:] are then obs and
 *                                              next_obs of every valid step
 *   action_out [n][L][act_dim] 4-byte words    row k < m: the action row of s_k, bit for bit; else zeros
 *   reward_out [n][L] f32                      reward[s_k] for k < m, else 0
 *   done_out   [n][L] f32                      (done[s_k] && !timeout[s_k]) ? 1 : 0 for k < m, else 0
 *   mask_out   [n][L] f32                      1 for k < m, else 0
 *   length_out [n] int32                       m
 *   index_out  [n] int64                       s, in the sampling calls
 * The launch writes the padding zeros itself: the outputs need no initialisation.
 * normalise != 0 behaves as in rex_rbuf_sample (REX_ERR_STATE without rex_norm_enable): with norm_obs every written row of obs_out, row m
 * included, is normalised with its column's statistic and the padding stays zero; with norm_reward each term of reward_out is normalised
 * as rex_rbuf_sample normalises a reward; done_out, mask_out, length_out and action_out are never normalised.  Under frozen statistics a
 * normalised row of a window equals the normalised row rex_rbuf_gather returns for the same id, bit for bit.
 * An id outside [0, T * B) is never turned into an address: every output of that sample is zero, length_out included, and it is counted
 * in the counter rex_rbuf_read_bad_indices reads.
 * With seq_len == 1, obs_out[:, 0], obs_out[:, 1], action_out[:, 0], reward_out[:, 0] and done_out[:, 0] are bit-identical to the five
 * outputs of rex_rbuf_gather, for any head. */
/* ONE launch over the caller's ids: index [dev, int64 n]. */
int rex_rbuf_gather_seq(rex_t* h, const rex_rbuf_buffers* buf, const int64_t* index, int64_t n, int64_t head, int seq_len, int normalise,
                        float* obs_out, void* action_out, float* reward_out, float* done_out, float* mask_out, int32_t* length_out,
                        void* stream);
/* ONE launch.  The ids are exactly those of rex_rbuf_sample for the same (seed, draw, size, B, j); every stored id is a valid start,
 * because the window shortens instead.  size / head are validated as in rex_rbuf_sample_nstep. */
int rex_rbuf_sample_seq(rex_t* h, const rex_rbuf_buffers* buf, int64_t size, int64_t head, int64_t n, uint64_t seed, uint64_t draw,
                        int seq_len, int normalise, float* obs_out, void* action_out, float* reward_out, float* done_out, float* mask_out,
                        int32_t* length_out, int64_t* index_out, void* stream);
/* TWO launches: the unchanged launch of rex_per_draw, then the sequence launch over index_out (needs rex_per_enable too, and the same T
 * in both descriptions).  An id of -1 meets the guard: zeros, counted. */
int rex_per_sample_seq(rex_t* h, const rex_rbuf_buffers* rbuf, const rex_per_buffers* per, int64_t n, int64_t head, uint64_t seed,
                       uint64_t draw, int seq_len, int normalise, float* obs_out, void* action_out, float* reward_out, float* done_out,
                       float* mask_out, int32_t* length_out, int64_t* index_out, float* prob_out, void* stream);

/* ---- acting-time history: a mirrored ring of (observation, previous action) frames -------------------------------------------------
 * The other half of the sequence windows above: at ACTING time a recurrent or history-fed policy needs the last K frames of every env
 * (stable-baselines3's VecFrameStack is the CPU counterpart).  An opt-in layer beside the others: rex_step, rex_norm_*, rex_rollout_*,
 * rex_rbuf_*, rex_per_* and rex_eplog_* are untouched, and there is no enable call -- the handle contributes its batch B, obs_dim,
 * act_dim and the action type only.  No rex_hist_* call allocates, synchronises or keeps host state between calls; each is ONE launch
 * on `stream`, so a captured revolution of K steps replays.
 *
 * Storage is caller-owned device memory, batch-first like the outputs of the sequence calls:
 *   frames [B][2K][W] f32   W = obs_dim + (with_action ? act_dim : 0).  A frame is the observation row followed by the action that led
 *                           to it; the cart-pole's int32 action is converted, (float)a (a frame is network input, not a bit copy).
 *   length [B] int32        valid frames of the lane's window, saturating at K
 *   K                       an int in [1, 64], the range of seq_len
 * All envs step in lockstep, so one ring position serves the batch.  A push at slot c (0 <= c < K) writes the new frame to rows c and
 * c + K: rows r and r + K of a lane are always equal.  Before the push the lane's window is rows [c, c + K - 1]; after it rows
 * [c + 1, c + K], oldest first, newest last, of which the first K - length[b] are zero.  frames[:, c + 1 : c + K + 1, :] is therefore a
 * zero-copy [B][K][W] view with strides (2KW, W, 1), and a step writes 2 W words per env where a shift moves (2K - 1) W.  The caller
 * passes slot = (number of pushes so far) mod K, as t in rex_rollout_add.
 *
 * Input layout: rows == 0 -- obs / terminal_obs [obs_dim][B] and action [act_dim][B], as rex_step reads and writes them; rows != 0 --
 * [B][obs_dim] and [B][act_dim], as rex_step_rows does.  The cart-pole's action is int32 [B] either way.
 *
 * rex_hist_push, for every lane b, in this order:
 *   1. if done != NULL && done[b] (the lane was auto-reset; obs[b] is the first observation of its next episode):
 *        with term_out, term_out[b][k] = frames[b][slot + 1 + k] for k = 0 .. K - 2 and term_out[b][K - 1] = (terminal_obs[b], action[b]):
 *        the window the finished episode would have seen, which a history-fed critic bootstraps a time-limit end from.  Rows of term_out
 *        whose done is clear are left as they were.  Then all 2K rows of the lane become 0 and length[b] = 0.
 *   2. frame = (obs[b], with_action ? (done lane ? 0 : action[b]) : nothing); rows slot and slot + K take it; length[b] = min(length[b] + 1, K).
 * rex_hist_reset is the companion of rex_reset: slot is the slot of the most recent push (any slot after rex_hist_init or for a full
 *   reset; the next push then goes to slot + 1, as after a push).  The lanes with mask[b] != 0 (all when mask == NULL) are cleared,
 *   their frame (obs[b], zeros) goes to rows slot and slot + K -- the newest row of the current window -- and length[b] = 1.  The
 *   other lanes are not touched and the ring does not advance.
 * rex_hist_window copies out[b][k] = frames[b][slot + 1 + k], slot being that of the most recent push: for callers that need a
 *   contiguous tensor or a fixed address.
 * rex_hist_init: frames <- 0, length <- 0.
 * Everything is a pure copy: the bits do not depend on the launch shape.
 *
 * REX_ERR_ARG, with nothing launched: a null description, frames, length or obs (out in rex_hist_window); K outside [1, 64]; slot outside
 * [0, K); with_action with a null action in rex_hist_push; term_out without terminal_obs. */
typedef struct rex_hist_buffers {
  float* frames;        /* [B][2K][W] */
  int32_t* length;      /* [B] */
  int K;
  int with_action;
} rex_hist_buffers;
int rex_hist_init(rex_t* h, const rex_hist_buffers* buf, void* stream);
int rex_hist_push(rex_t* h, const rex_hist_buffers* buf, int64_t slot, const float* obs, const void* action, const uint8_t* done /* may be NULL */,
                  const float* terminal_obs /* may be NULL */, float* term_out /* may be NULL, [B][K][W] */, int rows, void* stream);
int rex_hist_reset(rex_t* h, const rex_hist_buffers* buf, int64_t slot, const uint8_t* mask /* NULL = all */, const float* obs, int rows,
                   void* stream);
int rex_hist_window(rex_t* h, const rex_hist_buffers* buf, int64_t slot, float* out /* [B][K][W] */, void* stream);

/* ---- automatic domain randomisation: a box over the task that widens and narrows by itself --------------------------------------
 * Automatic Domain Randomization (OpenAI et al. 2019, "Solving Rubik's Cube with a Robot Hand", Algorithm 1) decides PER EPISODE: an
 * episode may pin one task dimension to a boundary of the current box, its return lands in that boundary's buffer, a full buffer moves
 * the boundary, and the next episode is drawn from the moved box.  With auto-reset on the step launch has already restarted the finished
 * lanes, so on the host this costs a done.nonzero() -- one synchronisation -- per step.  Here it is a post-pass: call order
 * rex_step -> rex_adr_record (-> rex_eplog_step).  The handle runs with dr_training OFF and auto-reset on; the layer stores the finished
 * lanes' next task into the handle's xi rows itself.  rex_step and every other family are untouched.  No reference counterpart.
 *
 * SETTINGS (rex_adr_config, fixed at enable; d = the handle's task_dim, arrays by task index k < d in rex_get_task's order):
 *   act[0 .. n_act)  the randomised task indices, strictly increasing, 1 <= n_act <= d.  J = 2 n_act BOUNDARIES: boundary a is dimension
 *                    act[a >> 1], side a & 1 (0 lower, 1 upper).
 *   p_b in [0, 1] (f32), m >= 1 (the buffer size), t_lo <= t_hi (f64), delta[k] > 0 on every active k (f32),
 *   lim_lo[k] <= centre[k] <= lim_hi[k] and the initial box lim_lo <= init_lo <= centre <= init_hi <= lim_hi (f32), seed (u64).
 * STATE (handle-owned): the box lo[d], hi[d] f32; per boundary a tally n[J] i64, s[J] f64 and the counters expanded[J], shrunk[J],
 *   held[J] i64; per lane ret f64, len i32, bnd i32 (-1, or the boundary its episode is pinned to), ep u32 (assignments the lane has had);
 *   scratch: block partials [blocks of 256 lanes][J] and a mask byte per lane.
 *
 * rex_adr_record(reward, done, apply): three launches (+ walker2d's derive launch), no synchronisation, no atomics, no host randomness:
 *   1. TALLY   every lane i: ret[i] += (double)reward[i]; len[i] += 1.  A lane CONTRIBUTES (bnd[i], ret[i]) if done[i] != 0 and bnd[i] >= 0.
 *              Block b (256 consecutive lanes) writes P[b][a] = (count, sum): the sum is the serial f64 sum of the contributors of boundary a
 *              in ascending lane order, started from 0.0.
 *   2. FOLD    for every boundary a, for b ascending with count > 0: n[a] += count; s[a] = s[a] + sum.  Then, if apply != 0 and n[a] >= m:
 *              mean = s[a] / (double)n[a];
 *              mean >= t_hi: EXPAND  lower: lo = max(lim_lo, lo - delta)   upper: hi = min(lim_hi, hi + delta)
 *              mean <= t_lo: SHRINK  lower: lo = min(centre, lo + delta)   upper: hi = max(centre, hi - delta)
 *              otherwise (a NaN mean included): HOLD.  One of expanded[a] / shrunk[a] / held[a] goes up by one; n[a] = 0, s[a] = 0.0.
 *   3. ASSIGN  every lane with done[i] != 0 runs assign(i) and sets its mask byte; the others clear theirs.
 *   4. walker2d: the geometry rows of the masked lanes are re-derived from their new lengths, as rex_set_task does for every lane.
 * assign(i): e = ep[i]; ep[i] = e + 1.  Philox4x32-10 stream in the map of the other device draws: key = seed ^ 0xD1B54A32D192ED03 (a family
 *   of its own), subsequence = env_offset + i, offset = 64 e.  u = rocRAND's uniform of a word, in (0, 1].  Word 0 is the coin: a BOUNDARY
 *   episode iff 1 - u0 < p_b.  Word 1 picks the boundary: a = min((int)((1 - u1) * (float)J), J - 1).  Word 4 + k gives
 *   xi_k = lo_k + (hi_k - lo_k) * (1 - u_k) for EVERY task index k < d (f32, each operation rounded, nothing fused).  On a boundary
 *   episode the pinned dimension takes hi (upper) or lo (lower) instead and bnd[i] = a; otherwise bnd[i] = -1.  xi_k goes to the task's row
 *   of the handle's xi block (the frozen rows of the Unmodeled ids stay untouched).  ret[i] = 0, len[i] = 0.
 * rex_adr_assign(mask): assign(i) for the lanes with mask[i] != 0 (all when NULL) without a tally -- after rex_reset or a masked reset; a
 *   boundary episode in progress on such a lane is dropped.  One launch (+ derive).
 * rex_adr_update: the fold launch with apply = 1 and no partials -- after rex_adr_record(apply = 0) and a merge of the ranks' tallies
 *   through rex_adr_get_state / rex_adr_set_state, every rank's box then moves identically.
 * The result depends on the inputs and the call order only: two runs agree bit for bit.
 *
 * rex_adr_enable is the only allocating call (rex_destroy frees); it sets the box to init_lo / init_hi, zeroes everything else and
 *   synchronises, and assigns nothing: call rex_adr_assign(NULL) to start every lane on a task of the box.  Enabling twice, any other
 *   rex_adr_* call before it, and rex_adr_record while dr_training is on return REX_ERR_STATE; a null pointer, n_act outside [1, d], an
 *   unsorted or out-of-range act, m < 1, p_b outside [0, 1] or NaN, t_lo > t_hi (or NaN), delta <= 0 on an active dimension and a violated
 *   limit / centre / box ordering return REX_ERR_ARG.  Nothing is launched or changed on an error. */
typedef struct rex_adr_config {
  int32_t n_act;
  const int32_t* act;          /* [n_act] */
  float p_b;
  int64_t m;
  double t_lo, t_hi;
  const float* delta;          /* [d]; read on the active dimensions */
  const float* lim_lo;         /* [d] */
  const float* lim_hi;         /* [d] */
  const float* centre;         /* [d] */
  const float* init_lo;        /* [d] */
  const float* init_hi;        /* [d] */
  uint64_t seed;
} rex_adr_config;
int rex_adr_enable(rex_t* h, const rex_adr_config* cfg);
int rex_adr_record(rex_t* h, const float* reward, const uint8_t* done, int apply, void* stream);
int rex_adr_assign(rex_t* h, const uint8_t* mask /* NULL = all */, void* stream);
int rex_adr_update(rex_t* h, void* stream);
/* box, tallies and counters through HOST arrays: lo, hi [d] float; n [J] int64; s [J] double; counters [3][J] int64 (expanded, shrunk,
 * held).  Synchronises.  set: REX_ERR_ARG for a box outside lim_lo <= lo <= centre <= hi <= lim_hi or a negative count. */
int rex_adr_get_state(rex_t* h, float* lo, float* hi, int64_t* n, double* s, int64_t* counters);
int rex_adr_set_state(rex_t* h, const float* lo, const float* hi, const int64_t* n, const double* s, const int64_t* counters);
/* the per-lane state [dev], stream-ordered: ret (double batch), len (int32 batch), bnd (int32 batch), ep (uint32 batch) */
int rex_adr_get_lane_state(rex_t* h, double* ret, int32_t* len, int32_t* bnd, uint32_t* ep, void* stream);
int rex_adr_set_lane_state(rex_t* h, const double* ret, const int32_t* len, const int32_t* bnd, const uint32_t* ep, void* stream);

/* ---- on-device actor: a fused MLP policy, its Gaussian draw, log-probability and value in one launch ------------------------------
 * What runs BETWEEN two rex_step calls in every on-policy loop: stable-baselines3's default MlpPolicy for continuous actions
 * (common/policies.py ActorCriticPolicy: mlp_extractor.policy_net / value_net, action_net, value_net, log_std, DiagGaussianDistribution) --
 * two separate towers of at most three hidden layers, about fifteen eager torch launches.  Here it is ONE launch on `stream`, without an
 * allocation, a synchronisation or host state, so a captured loop replays.  Inference only: the learner stays in torch ON THE SAME
 * PARAMETERS (the pointers below are read at every call, so an in-place optimiser step is seen by the next call).  No reference
 * counterpart.  There is no enable call; the handle contributes B, act_dim, env_offset and the action type and nothing else; rex_step and
 * every other family are untouched.  Out of scope: categorical heads (a discrete-action handle -- the cart-pole -- returns REX_ERR_STATE),
 * recurrent cells, squashed-Gaussian actors, a state-dependent std, widths above 64, any backward pass.
 *
 * NETWORK (rex_actor_net, a HOST struct of DEVICE pointers, fp32): in_dim in [1, 1024] (not tied to obs_dim: a flattened history window is
 *   a legal input); activation 0 = tanh, 1 = relu; towers pi and vf, either of which may be NULL -- a null pi computes the value only (the
 *   bootstrap call on terminal_observation), a null vf computes no value.  A tower has n_hidden in [1, 3] hidden layers of width[l] in
 *   [1, 64] and a head: layer l < n_hidden is W[l] [width[l]][fan_in] ROW-MAJOR, exactly as nn.Linear.weight stores it (fan_in = in_dim for
 *   l = 0, width[l - 1] after it) with b[l] [width[l]]; W[n_hidden], b[n_hidden] are the head, [act_dim][width[n_hidden - 1]] for pi and
 *   [1][...] for vf.  log_std [act_dim] and std [act_dim] = exp(log_std) are BOTH passed in: the device never evaluates exp.  seed keys the draws.
 * INPUT in [dev]: rows != 0 -- [B][in_dim]; rows == 0 -- [in_dim][B].
 * ARITHMETIC, per env i, fp32, fully ordered, nothing contracted beyond the fmaf written here (a g++ host build restates it bit for bit):
 *   layer:   y_j = b_j; for i ascending y_j = fmaf(W[j][i], x_i, y_j); then the activation on the hidden layers, none on the heads.
 *   relu(x) = fmaxf(x, 0) (so a NaN becomes 0 there, as IEEE maxNum has it).
 *   tanh32(x), the project's own (csrc/actor.hpp; coefficients from profiles/actor_tanh_fit.py): a NaN returns itself; otherwise it is
 *     evaluated on a = |x| and the sign of x is copied onto the result, so it is exactly odd.  a < 0.625: fmaf(a * u, P(u), a) with u = a * a
 *     and P of degree 6 by Horner fmaf; otherwise t = 2 min(a, 10), n = rintf(t * log2 e), r = fmaf(-n, ln2_lo, fmaf(-n, ln2_hi, t)),
 *     e = Q(r) * 2^n (Q of degree 6 by Horner fmaf, the scaling exact), 1 - 2 / (e + 1) with one IEEE division.  It saturates to +-1 where
 *     fp32 does.  Error against fp64 tanh over EVERY fp32 in [-10, 10] (the exhaustive sweep of the host build, profiles/actor_tanh_sweep.py):
 *     at most 1.371 ulp of the result, at x = 0.63022083; T = 1.5 ulp is the bound tests/test_actor_host.py holds a subsample to.
 *   mean_k (pi head) and value (vf head) by the layer rule.
 *   eps_k: rocRAND's normal of the Philox4x32-10 stream in the map of the other device draws: key = seed ^ 0xA0761D6478BD642F (a family of
 *     its own), subsequence = env_offset + i, offset = 32 * draw (mod 2^64); draws in rocrand_normal's pairing (words 2 p, 2 p + 1 give
 *     eps_2p = .x and eps_(2p+1) = .y).  draw is the caller's call counter, like the draw number of rex_rbuf_sample.
 *   action_k = fmaf(std_k, eps_k, mean_k);  S = 0, for k ascending S = fmaf(eps_k, eps_k, S);
 *   s = 0, for k ascending s = s + log_std_k;  c = s + (float)act_dim * 0.91893853f (a product, then a sum);  logp = fmaf(-0.5f, S, -c).
 *   deterministic != 0: no draw is made, eps = 0, action = mean, logp = -c.
 *   Actions are NOT clipped: the step kernels clamp ctrl themselves.
 * OUTPUTS [dev]: action_out [B][act_dim] (rows != 0) or [act_dim][B] (rows == 0); logp_out [B] (may be NULL); value_out [B]; noise_out
 *   [B][act_dim] (may be NULL) receives eps as drawn (zeros when deterministic).  Outputs of an absent tower are never written.
 * A non-finite input makes that lane's mean, action and value whatever the arithmetic gives (non-finite under tanh; relu's fmaxf drops a NaN)
 *   -- logp is a function of the noise and log_std alone -- and touches no other lane.  Under relu a NaN input therefore leaves the lane
 *   FINITE: every first-layer unit it reaches becomes fmaxf(NaN, 0) = 0 (an inf input stays visible unless its weights cancel).  The tests pin
 *   both activations; a caller that must see a non-finite observation tests the observation.  The bits
 *   do not depend on the launch shape, on rows, or on how the batch is sharded over handles (env_offset).
 *
 * Checks, in this order, nothing launched on a failure: null handle (REX_ERR_ARG); a discrete-action handle (REX_ERR_STATE); then
 *   REX_ERR_ARG for: a null net; both towers null; in_dim outside [1, 1024]; an activation other than 0 / 1; per present tower, pi first:
 *   n_hidden outside [1, 3], a width outside [1, 64], a null W or b of a layer or of the head; pi without log_std, std or action_out; vf
 *   without value_out; a negative draw; a null input; then REX_ERR_UNSUPPORTED for a handle whose act_dim is above 32, the
 *   number of action rows the kernel's epilogue is built for (no env kind has more than 17); and last REX_ERR_ARG for a batch of more than
 *   2^31 - 1 waves of 64 envs, which one launch does not take. */
#define REX_ACTOR_MAX_HIDDEN 3
typedef struct rex_actor_tower {
  int n_hidden;
  int width[REX_ACTOR_MAX_HIDDEN];
  const float* W[REX_ACTOR_MAX_HIDDEN + 1];   /* [dev] hidden layers, then the head at index n_hidden */
  const float* b[REX_ACTOR_MAX_HIDDEN + 1];
} rex_actor_tower;
typedef struct rex_actor_net {
  int in_dim;
  int activation;                /* 0 tanh, 1 relu */
  const rex_actor_tower* pi;     /* [host], may be NULL */
  const rex_actor_tower* vf;     /* [host], may be NULL */
  const float* log_std;          /* [dev, act_dim] */
  const float* std;              /* [dev, act_dim] */
  uint64_t seed;
} rex_actor_net;
int rex_actor_act(rex_t* h, const rex_actor_net* net, const float* in, int rows, int64_t draw, int deterministic, float* action_out,
                  float* logp_out /* may be NULL */, float* value_out, float* noise_out /* may be NULL */, void* stream);

const char* rex_last_error(void);
const char* rex_version(void);

#ifdef __cplusplus
}
#endif
#endif /* REX_H_ */
