// cartpole_kernels.hpp -- the CartPole kernels: step, reset, observation.  One env per lane.
#pragma once
#include "device_rng.hpp"

// ------------------------------------------------------------------------------------------
// CartPole (random_envs/random_cartpole.py:172-229).  qpos = (x, theta), qvel = (x_dot, theta_dot).
// ------------------------------------------------------------------------------------------
// ROWS: action stays int32[B]; obs and term_obs are row-major [B][4], one 16-byte store per env (rex_step_rows / rex_reset_rows; the buffers are
// 16-byte aligned, which the entry points check)
template <bool ROWS = false>
__global__ void __launch_bounds__(64) cartpole_step_kernel(DevState s, StepFlags fl, const int* __restrict__ action,
                                                           float* __restrict__ obs, float* __restrict__ reward,
                                                           unsigned char* __restrict__ done_out, unsigned char* __restrict__ trunc_out,
                                                           float* __restrict__ term_obs) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;   // 32-bit lane offset + uniform (SGPR) row bases
  if (i >= s.B) return;
  const long long B = s.B;
  float x = s.qpos[i], th = s.qpos[B + i], xd = s.qvel[i], thd = s.qvel[B + i];
  float g = s.xi[i], mc = s.xi[B + i], mp = s.xi[2 * B + i], l = s.xi[3 * B + i];
  float total = mp + mc;                                  // set_task :166
  const float pml = 0.1f * 0.5f;                          // :79, not refreshed by set_task
  float force = action[i] == 1 ? 10.0f : -10.0f;          // :80,178
  float st, ct; sincosf(th, &st, &ct);
  float temp = (force + pml * thd * thd * st) / total;    // :184
  float thacc = (g * st - ct * temp) / (l * (4.0f / 3.0f - mp * ct * ct / total));   // :185
  float xacc = temp - pml * thacc * ct / total;           // :186
  const float tau = 0.02f;
  x = x + tau * xd; xd = xd + tau * xacc; th = th + tau * thd; thd = thd + tau * thacc;   // :188-192
  s.qpos[i] = x; s.qpos[B + i] = th; s.qvel[i] = xd; s.qvel[B + i] = thd;
  const float th_thr = 12.0f * 2.0f * 3.14159265358979323846f / 360.0f, x_thr = 2.4f;   // :84-85
  bool was_done = s.done[i] != 0;                          // steps_beyond_done bookkeeping :208-222
  // (every comparison of the rule is false on a NaN: a non-finite lane ends its episode and is counted, as in every other kind -- rex.h, rex_get_counters)
  const bool finite = isfinite(x) && isfinite(th) && isfinite(xd) && isfinite(thd);
  bool dn = (x < -x_thr) || (x > x_thr) || (th < -th_thr) || (th > th_thr) || !finite;
  if (!finite) atomicAdd(s.counters + 0, 1ull);
  float r = (!dn) ? 1.0f : (was_done ? 0.0f : 1.0f);
  int t = s.t[i] + 1; s.t[i] = t;
  bool trunc = fl.time_limit && t >= fl.max_steps && !dn;
  bool d = dn || trunc;
  s.done[i] = (unsigned char)((dn || was_done) ? 1 : 0) | (unsigned char)(d ? 2 : 0);
  if constexpr (ROWS) {
    reinterpret_cast<float4*>(obs)[i] = make_float4(x, xd, th, thd);
    if (term_obs && d) reinterpret_cast<float4*>(term_obs)[i] = make_float4(x, xd, th, thd);   // (defined on the done rows only, rex.h)
  } else {
    obs[i] = x; obs[B + i] = xd; obs[2 * B + i] = th; obs[3 * B + i] = thd;   // np.array(self.state) :224
    if (term_obs) { term_obs[i] = x; term_obs[B + i] = xd; term_obs[2 * B + i] = th; term_obs[3 * B + i] = thd; }
  }
  reward[i] = r; done_out[i] = d ? 1 : 0;
  if (trunc_out) trunc_out[i] = trunc ? 1 : 0;
}

// reset(): state ~ U(-0.05, 0.05)^4 (random_cartpole.py:226-229). `resample` = set_random_task.
template <bool ROWS = false>
__global__ void __launch_bounds__(64) cartpole_reset_kernel(DevState s, DRParams dr, int resample, int reset_state,
                                                            const unsigned char* __restrict__ mask, int mask_bit,
                                                            float* __restrict__ obs) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;   // 32-bit lane offset + uniform (SGPR) row bases
  if (i >= s.B) return;
  if (mask && !(mask[i] & mask_bit)) return;
  const long long B = s.B;
  unsigned ep = s.episode[i] + 1; s.episode[i] = ep;
  rocrand_state_philox4x32_10 st;
  rocrand_init(s.seed, (unsigned long long)(s.env_offset + i), philox_episode(ep), &st);
  if (reset_state) {
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = -0.05f + 0.1f * (1.0f - rocrand_uniform(&st));
    s.qpos[i] = v[0]; s.qvel[i] = v[1]; s.qpos[B + i] = v[2]; s.qvel[B + i] = v[3];
    s.t[i] = 0; s.done[i] = 0;
    if (obs) {
      if constexpr (ROWS) reinterpret_cast<float4*>(obs)[i] = make_float4(v[0], v[1], v[2], v[3]);
      else { obs[i] = v[0]; obs[B + i] = v[1]; obs[2 * B + i] = v[2]; obs[3 * B + i] = v[3]; }
    }
  }
  if (resample && dr.type != REX_DR_NONE) {
    sample_task(dr, s.seed, (unsigned long long)(s.env_offset + i), philox_task(ep), s.xi, (size_t)B, i, s.counters);
  }
}

__global__ void __launch_bounds__(64) cartpole_obs_kernel(DevState s, float* __restrict__ obs) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;   // 32-bit lane offset + uniform (SGPR) row bases
  if (i >= s.B) return;
  const long long B = s.B;
  obs[i] = s.qpos[i]; obs[B + i] = s.qvel[i]; obs[2 * B + i] = s.qpos[B + i]; obs[3 * B + i] = s.qvel[B + i];
}
