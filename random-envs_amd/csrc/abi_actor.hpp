// abi_actor.hpp -- host code of rex_hip.hip: rex_actor_act, the on-device actor (actor.hpp): both towers of an MLP policy, the Gaussian draw,
// its log-probability and the value in one launch over the caller's parameters; nothing is kept in the handle.
#pragma once

extern "C" int rex_actor_act(rex_t* h, const rex_actor_net* net, const float* in, int rows, int64_t draw, int deterministic, float* action_out,
                             float* logp_out, float* value_out, float* noise_out, void* stream) {
  REX_ENTER(h, "rex_actor_act");
  if (h->dims.discrete_action) return set_err(REX_ERR_STATE, "rex_actor_act: a discrete-action handle (the categorical head is out of scope)");
  if (const char* why = actor::arg_error(net, in, draw, action_out, value_out)) return set_err(REX_ERR_ARG, "rex_actor_act: %s", why);
  if (h->dims.act_dim > actor::MAX_ACT) return set_err(REX_ERR_UNSUPPORTED, "rex_actor_act: act_dim %d is more than the epilogue is built for", h->dims.act_dim);
  const long long blocks = actor::block_count(h->B);
  if (!grid_fits(blocks)) return set_err(REX_ERR_ARG, "rex_actor_act: batch %lld is more than one launch takes", h->B);
  actor::Params p{};
  p.B = h->B; p.env_offset = h->env_offset;
  p.seed = net->seed ^ actor::ACTOR_SALT; p.block0 = actor::draw_block(draw);
  p.in_dim = net->in_dim; p.act_dim = h->dims.act_dim; p.rows = rows ? 1 : 0; p.deterministic = deterministic ? 1 : 0; p.activation = net->activation;
  p.first_tower = net->pi ? 0 : 1;
  p.tower[0] = actor::tower_of(net->pi ? net->pi : net->vf); p.tower[1] = actor::tower_of(net->pi ? net->vf : nullptr);
  p.log_std = net->log_std; p.std = net->std; p.in = in;
  p.action = action_out; p.logp = logp_out; p.value = value_out; p.noise = noise_out;
  hipLaunchKernelGGL(actor::actor_kernel, dim3((unsigned)blocks, net->pi && net->vf ? 2u : 1u), dim3(actor::LANES), 0, (hipStream_t)stream, p);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}
