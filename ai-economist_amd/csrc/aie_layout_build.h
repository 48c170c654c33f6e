/*
 * aie_layout_build.h -- host only: builds the parameter block (aie_params) and the tensor table of a configuration.
 * aie_build_params is the single source of truth for where everything lives in the arena and in a replica's record;
 * aie_layout.h declares what it fills in.
 *
 * Plain C99 (also included from HIP C++ host code).  Included by aie_capi.hip, by the build-time tool aie_specgen.c
 * and by the CPU restatement oracle/aie_oracle.c -- by no kernel file and no device header: what is decided here
 * reaches a kernel through the parameter block only, so this file is in no specialisation cache key (aie_jit.h).
 */
#ifndef AIE_LAYOUT_BUILD_H_
#define AIE_LAYOUT_BUILD_H_

#include <stdio.h>
#include <string.h>

#ifndef AIE_LAYOUT_H_ONLY
#define AIE_LAYOUT_H_ONLY 1 /* aie_layout.h brings nothing along (its last lines) */
#endif
#include "aie_layout.h"

typedef struct aie_tensor_table {
  int32_t n;
  aie_tensor_desc t[AIE_MAX_TENSORS];
} aie_tensor_table;

#define AIE__FAIL(...)                                   \
  do {                                                   \
    if (err) snprintf(err, errlen, __VA_ARGS__);         \
    return AIE_E_INVALID;                                \
  } while (0)

/* record field allocator */
static inline int32_t aie__rec(int32_t* cur, int32_t bytes, int32_t align) {
  int32_t o = (int32_t)aie__align(*cur, align);
  *cur = o + bytes;
  return o;
}

static inline void aie__add(aie_tensor_table* tt, const char* name, int dtype, int64_t off,
                            int64_t env_stride, int ndim_inner, int64_t d0, int64_t d1,
                            int64_t d2, int64_t d3, int64_t E) {
  if (!tt || tt->n >= AIE_MAX_TENSORS) return;
  aie_tensor_desc* d = &tt->t[tt->n++];
  memset(d, 0, sizeof(*d));
  snprintf(d->name, sizeof(d->name), "%s", name);
  d->dtype = dtype;
  d->ndim = 1 + ndim_inner;
  int64_t dims[4] = {d0, d1, d2, d3};
  d->shape[0] = E;
  d->stride[0] = env_stride;
  int64_t st = aie__dtype_size(dtype);
  for (int i = ndim_inner - 1; i >= 0; --i) {
    d->shape[1 + i] = dims[i];
    d->stride[1 + i] = st;
    st *= dims[i];
  }
  d->arena_offset = off;
  d->data = NULL;
}

static inline void aie__add_shared(aie_tensor_table* tt, const char* name, int dtype, int64_t off,
                                   int nd, int64_t d0, int64_t d1) {
  aie__add(tt, name, dtype, off, 0, nd, d0, d1, 0, 0, 1);
}

static inline int aie__build_covid(const aie_config* c, aie_params* p, aie_tensor_table* tt,
                                   char* err, size_t errlen) {
  const aie_covid_config* v = &c->covid;
  if (c->n_agents > AIE_MAX_AGENTS)
    AIE__FAIL("n_agents = %d: the COVID scenario holds at most %d states per replica here (one lane each)", c->n_agents, AIE_MAX_AGENTS);
  if (c->multi_action_mode_agents || c->multi_action_mode_planner)
    AIE__FAIL("the COVID scenario uses single-action mode for agents and planner");
  static const int want[3] = {AIE_COMP_COVID_CONTROL, AIE_COMP_COVID_SUBSIDY, AIE_COMP_COVID_VACCINE};
  if (c->n_components != 3) AIE__FAIL("the COVID scenario needs exactly its three components");
  if (c->dense_log_replicas != 0) AIE__FAIL("dense logs are not available for the COVID scenario");
  /* each of the three exactly once, in any order: their steps touch disjoint state and the reference's rewards and
   * observations do not depend on the order (live reference, tests/test_covid_component_order.py); the fused kernel runs
   * them in the canonical one */
  for (int k = 0; k < 3; ++k) {
    int seen = 0;
    for (int i = 0; i < 3; ++i) seen += c->components[i] == want[k];
    if (seen != 1)
      AIE__FAIL("COVID components must be ControlUSStateOpenCloseStatus, FederalGovernmentSubsidy and VaccinationCampaign, each once");
  }
  if (v->num_stringency_levels < 1 || v->num_stringency_levels > 100) AIE__FAIL("num_stringency_levels out of range");
  if (v->beta_delay < 1 || v->beta_delay > 4096) AIE__FAIL("beta_delay out of range");
  if (v->filter_len < 1 || v->filter_len > 65536) AIE__FAIL("filter_len out of range");
  if (v->num_filters < 1 || v->num_filters > AIE_COVID_MAX_FILTERS) AIE__FAIL("num_filters out of range");
  if (v->filter_len < v->beta_delay) AIE__FAIL("filter_len < beta_delay is not supported");
  /* the window sums keep a state's level changes as events `history day | delta << 16` (aie_kernels_covid.hip): the day
   * index runs to filter_len + episode_length and must fit 16 bits (the reference has no such bound) */
  if (!v->filter_recurrence && (int64_t)v->filter_len + (int64_t)c->episode_length > 65535)
    AIE__FAIL("filter_len + episode_length = %lld: the reference-exact window sums index history days with 16 bits "
              "(<= 65535); use filter_recurrence or a shorter episode", (long long)v->filter_len + c->episode_length);
  if (v->action_cooldown_period < 1) AIE__FAIL("action_cooldown_period must be >= 1 (covid19_components.py:57)");
  if (v->subsidy_interval < 1) AIE__FAIL("subsidy_interval must be >= 1 (covid19_components.py:278)");
  if (v->num_subsidy_levels < 1 || v->num_subsidy_levels > 255) AIE__FAIL("num_subsidy_levels out of range");
  if (v->delivery_interval < 1) AIE__FAIL("delivery_interval must be >= 1 (covid19_components.py:505)");
  if (v->time_when_vaccine_delivery_begins < 0) AIE__FAIL("vaccine delivery must not begin before the start date");
  if (!(v->economic_reward_crra_eta >= 0.0)) AIE__FAIL("economic_reward_crra_eta must be >= 0");
  if (v->economic_reward_crra_eta == 1.0) AIE__FAIL("economic_reward_crra_eta == 1 divides by zero (covid19_env.py:1074)");
  if (!(v->reward_normalization_factor != 0.0)) AIE__FAIL("reward_normalization_factor must be non-zero");
  if (v->replay_data && !v->replay_policies) AIE__FAIL("replay_data (use_real_world_data) needs replay_policies (covid19_env.py:126-135)");
  if (v->filter_recurrence)
    for (int f = 0; f < v->num_filters; ++f)
      if (!(v->filter_decay[f] > 0.0 && v->filter_decay[f] < 1.0)) AIE__FAIL("filter_decay[%d] must be in (0, 1)", f);

  p->c = *c;
  p->E = c->n_envs;
  p->n = c->n_agents;
  p->H = c->world_h; p->W = c->world_w; p->HW = p->H * p->W;
  const int n = p->n;
  p->cv_L = v->filter_len;
  p->cv_F = v->num_filters;
  p->cv_NL = v->num_stringency_levels;
  p->cv_NS = v->num_subsidy_levels;
  /* + slack: the last prefetch group of the last step reads (zero-tap) chunks past day T */
  p->cv_nch = (v->filter_len + 1 + c->episode_length + 15) / 16 + AIE_CV_GROUP + 3;
  p->cv_row = (int32_t)aie__align(16 * n, 64);
  p->cv_nrow_obs = AIE_CV_OB_MASK + 1 + p->cv_NL;
  {
    int t = v->time_when_vaccine_delivery_begins;        /* covid19_components.py:640-646 */
    while (t % v->delivery_interval != 0) t++;
    p->cv_t_first_delivery = t;
  }
  p->A = 1 + p->cv_NL;  p->MA = p->A;  p->act_a_width = 1;  p->n_sub_a = 1;
  p->sub_a_dim[0] = p->cv_NL; p->sub_a_base[0] = 1;
  p->n_sub_p = 1; p->sub_p_dim = p->cv_NS; p->MP = 1 + p->cv_NS; p->act_p_width = 1;
  p->AP = 1 + p->cv_NS; p->p_row_dim = p->cv_NS; p->p_rows_uniform = 1; p->tax_p_base = 1; p->tax_p_moff = 1;
  if (c->host_a_n || c->host_p_n) AIE__FAIL("host components' action subspaces: gather-trade-build scenarios only");
  p->planner_acts = 1;

  int32_t cur = 0;
  p->cv_pitch = n;
  p->o_cv_state = aie__rec(&cur, 4 * n * AIE_CV_ST_COUNT, 256);
  p->o_cv_cooldown = aie__rec(&cur, 4 * n, 4);
  p->o_cv_sums = aie__rec(&cur, 8 * n * AIE_CV_SUM_COUNT, 8);
  p->o_cv_acc = aie__rec(&cur, 8 * n * v->num_filters, 8);  /* recurrence: A_t; window sums: the coming step's sums over the days before its own */
  p->o_cv_ring = aie__rec(&cur, 32 * 64, 256);
  p->cv_ev_groups = v->filter_recurrence ? 0 : AIE_CV_EVENT_CAP / 4;
  p->o_cv_ev_ht = aie__rec(&cur, p->cv_ev_groups ? 4 * n : 0, 4);
  p->o_cv_dense = aie__rec(&cur, 4, 4);
  p->o_cv_tail_pending = aie__rec(&cur, 4, 4);
  p->o_cv_subsidy_level = aie__rec(&cur, 4, 4);
  p->o_cv_p_index = aie__rec(&cur, 8, 4);
  p->o_timestep = aie__rec(&cur, 4, 4);
  p->o_completions = aie__rec(&cur, 4, 4);
  p->o_sample_t = aie__rec(&cur, 4, 4);
  p->o_rew_slot = aie__rec(&cur, 4, 4);
  p->o_rew_epoch = aie__rec(&cur, 4, 4);
  p->rec_bytes = (int32_t)aie__align(cur, 256);

  const int64_t E = p->E;
  const int64_t no = (int64_t)p->cv_nrow_obs * n * 4, po = (int64_t)(4 + p->MP) * 4;
  int64_t a = 0;
  p->a_records = a;    a = aie__align(a + E * (int64_t)p->rec_bytes, 256);
  p->a_cv_consts = a;  a = aie__align(a + (int64_t)AIE_CV_K_COUNT * 64 * 8, 256);
  p->a_cv_filters = a;
  a = aie__align(a + (int64_t)(AIE_CV_TAP_PAD_FRONT + p->cv_L + AIE_CV_TAP_PAD_BACK) * p->cv_F * 8, 256);
  p->a_cv_hist0 = a;   a = aie__align(a + (int64_t)(p->cv_L + 1) * n, 256);
  p->a_cv_hist0c = a;  a = aie__align(a + (int64_t)p->cv_nch * p->cv_row, 256);
  p->a_cv_acc0 = a;    a = aie__align(a + (int64_t)AIE_COVID_MAX_FILTERS * 64 * 8, 256);
  p->a_cv_lag_obs = a; a = aie__align(a + (int64_t)v->beta_delay * n, 256);
  p->a_cv_replay_a = p->a_cv_replay_p = p->a_cv_replay_state = 0;
  if (v->replay_policies) {
    p->a_cv_replay_a = a; a = aie__align(a + (int64_t)c->episode_length * 64, 256);
    p->a_cv_replay_p = a; a = aie__align(a + (int64_t)c->episode_length * 4, 256);
  }
  if (v->replay_data) {
    p->a_cv_replay_state = a; a = aie__align(a + (int64_t)6 * (c->episode_length + 1) * 64 * 8, 256);
  }
  p->a_cv_hist = a;    a = aie__align(a + E * (int64_t)p->cv_nch * p->cv_row, 256);
  p->a_cv_ev0 = a;     a = aie__align(a + (int64_t)p->cv_ev_groups * 1024 + 256 + 16, 256);
  p->a_cv_events = a;  a = aie__align(a + E * (int64_t)p->cv_ev_groups * 1024, 256);
  p->a_cv_obs_a = a;   a = aie__align(a + E * no, 256);
  p->a_cv_obs_p = a;   a = aie__align(a + E * po, 256);
  p->a_rew_a = a; a = aie__align(a + E * n * 4, 256);
  p->a_rew_p = a; a = aie__align(a + E * 4, 256);
  p->a_done = a;  a = aie__align(a + E, 256);
  p->arena_bytes = a;

  if (tt) {
    const int64_t rs = p->rec_bytes, r0 = p->a_records;
    static const char* st_name[AIE_CV_ST_COUNT] = {"susceptible", "infected", "recovered", "deaths", "vaccinated",
                                                   "unemployed", "postsubsidy_productivity", "subsidy",
                                                   "health_index", "economic_index"};
    static const char* sum_name[AIE_CV_SUM_COUNT] = {"sum_unemployed", "sum_stringency_level",
                                                     "sum_postsubsidy_productivity", "sum_subsidy"};
    for (int k = 0; k < AIE_CV_SUM_COUNT; ++k)
      aie__add(tt, sum_name[k], AIE_F64, r0 + p->o_cv_sums + 8 * n * k, rs, 1, n, 0, 0, 0, E);
    aie__add(tt, "planner_health_economic_index", AIE_F32, r0 + p->o_cv_p_index, rs, 1, 2, 0, 0, 0, E);
    /* recurrence: each filter's discounted delta sum A_t; window sums: each filter's sum over the NEXT step's window
     * without that step's own day (formed at the end of a step, when the registers are free; the step adds its day) */
    aie__add(tt, v->filter_recurrence ? "filter_discounted_delta_sums" : "filter_window_sums_before_today", AIE_F64,
             r0 + p->o_cv_acc, rs, 2, p->cv_F, n, 0, 0, E);
    tt->t[tt->n - 1].stride[1] = 8 * n;
    for (int k = 0; k < AIE_CV_ST_COUNT; ++k)
      aie__add(tt, st_name[k], AIE_F32, r0 + p->o_cv_state + 4 * n * k, rs, 1, n, 0, 0, 0, E);
    aie__add(tt, "cooldown_until", AIE_I32, r0 + p->o_cv_cooldown, rs, 1, n, 0, 0, 0, E);
    aie__add(tt, "subsidy_level", AIE_I32, r0 + p->o_cv_subsidy_level, rs, 0, 0, 0, 0, 0, E);
    aie__add(tt, "timestep", AIE_I32, r0 + p->o_timestep, rs, 0, 0, 0, 0, 0, E);
    aie__add(tt, "completions", AIE_I32, r0 + p->o_completions, rs, 0, 0, 0, 0, 0, E);
    aie__add(tt, "sample_t", AIE_I32, r0 + p->o_sample_t, rs, 0, 0, 0, 0, 0, E);
    aie__add(tt, "rew_log_slot", AIE_I32, r0 + p->o_rew_slot, rs, 0, 0, 0, 0, 0, E);
    /* stringency level of the 32 most recent days: row (filter_len + day) & 31 (always current) */
    aie__add(tt, "stringency_ring", AIE_U8, r0 + p->o_cv_ring, rs, 2, 32, n, 0, 0, E);
    tt->t[tt->n - 1].stride[1] = 64;
    /* stringency level on day (16*chunk + j - filter_len) of the episode, per state.  With filter_recurrence a chunk
     * is written when its 16th day is over (from the ring); without, every day (the window sums stream it) */
    if (p->cv_ev_groups) {
      /* level-change events per state: list positions [head, tail) are inside the current filter window */
      aie__add(tt, "stringency_change_head_tail", AIE_I32, r0 + p->o_cv_ev_ht, rs, 1, n, 0, 0, 0, E);
      aie__add(tt, "stringency_change_events", AIE_U32, p->a_cv_events, (int64_t)p->cv_ev_groups * 1024, 3, p->cv_ev_groups,
               n, 4, 0, E);
      tt->t[tt->n - 1].stride[1] = 1024;
      tt->t[tt->n - 1].stride[2] = 16;
    }
    aie__add(tt, "window_streams_whole_history", AIE_I32, r0 + p->o_cv_dense, rs, 0, 0, 0, 0, 0, E);
    aie__add(tt, "stringency_history_chunks", AIE_U8, p->a_cv_hist, (int64_t)p->cv_nch * p->cv_row, 3,
             p->cv_nch, n, 16, 0, E);
    tt->t[tt->n - 1].stride[1] = p->cv_row;

    static const char* k_name[AIE_CV_K_CONV_W0] = {
        "model_us_state_population", "model_beta_slopes", "model_beta_intercepts", "model_unemployment_bias",
        "model_maximum_productivity", "model_agents_health_norm", "model_agents_economic_norm",
        "model_min_marginal_agent_health_index", "model_max_marginal_agent_health_index",
        "model_min_marginal_agent_economic_index", "model_max_marginal_agent_economic_index",
        "model_weightage_on_marginal_agent_health_index", "model_weightage_on_marginal_agent_economic_index",
        "model_max_daily_subsidy_per_state", "model_num_vaccines_per_delivery",
        "model_susceptible_0", "model_infected_0", "model_recovered_0", "model_deaths_0", "model_unemployed_0",
        "model_vaccinated_0"};
    for (int k = 0; k < AIE_CV_K_CONV_W0; ++k)
      aie__add_shared(tt, k_name[k], AIE_F64, p->a_cv_consts + (int64_t)k * 512, 1, n, 0);
    aie__add_shared(tt, "model_conv_weights", AIE_F64, p->a_cv_consts + (int64_t)AIE_CV_K_CONV_W0 * 512, 2, p->cv_F, n);
    tt->t[tt->n - 1].stride[1] = 512;
    /* stored tap-major ([L][F]) so that the F taps of one day, and 16 days, are contiguous;
     * zero rows before and after (the arena is zero-initialised) */
    aie__add_shared(tt, "model_unemp_conv_filters", AIE_F64,
                    p->a_cv_filters + (int64_t)AIE_CV_TAP_PAD_FRONT * p->cv_F * 8, 2, p->cv_F, p->cv_L);
    tt->t[tt->n - 1].stride[1] = 8;
    tt->t[tt->n - 1].stride[2] = 8 * (int64_t)p->cv_F;
    aie__add_shared(tt, "model_stringency_level_history_0", AIE_U8, p->a_cv_hist0, 2, p->cv_L + 1, n);
    aie__add_shared(tt, "model_policy_before_start_obs", AIE_U8, p->a_cv_lag_obs, 2, v->beta_delay, n);
    if (v->replay_policies) {
      aie__add_shared(tt, "replay_stringency_policy", AIE_U8, p->a_cv_replay_a, 2, c->episode_length, n);
      tt->t[tt->n - 1].stride[1] = 64;
      aie__add_shared(tt, "replay_subsidy_level", AIE_I32, p->a_cv_replay_p, 1, c->episode_length, 0);
    }
    if (v->replay_data) {
      aie__add(tt, "replay_state", AIE_F64, p->a_cv_replay_state, 0, 3, 6, c->episode_length + 1, n, 0, 1);
      tt->t[tt->n - 1].stride[1] = (int64_t)(c->episode_length + 1) * 64 * 8;
      tt->t[tt->n - 1].stride[2] = 64 * 8;
    }

#define OBA(name, row, nd, d0) aie__add(tt, name, AIE_F32, p->a_cv_obs_a + (int64_t)(row) * n * 4, no, nd, d0, (nd) == 2 ? n : 0, 0, 0, E)
    OBA("obs_a_world-agent_state", AIE_CV_OB_STATE, 2, 6);
    OBA("obs_a_world-agent_postsubsidy_productivity", AIE_CV_OB_PROD, 1, n);
    OBA("obs_a_world-lagged_stringency_level", AIE_CV_OB_LAG, 1, n);
    OBA("obs_a_time", AIE_CV_OB_TIME, 1, n);
    OBA("obs_a_ControlUSStateOpenCloseStatus-agent_policy_indicators", AIE_CV_OB_POLICY, 1, n);
    OBA("obs_a_FederalGovernmentSubsidy-t_until_next_subsidy", AIE_CV_OB_T_SUBSIDY, 1, n);
    OBA("obs_a_FederalGovernmentSubsidy-current_subsidy_level", AIE_CV_OB_SUBSIDY_LEVEL, 1, n);
    OBA("obs_a_VaccinationCampaign-t_until_next_vaccines", AIE_CV_OB_T_VACCINE, 1, n);
    OBA("obs_a_action_mask", AIE_CV_OB_MASK, 2, 1 + p->cv_NL);
    /* the planner sees the same per-state arrays (covid19_env.py:986-992, covid19_components.py:167-168) */
    OBA("obs_p_world-agent_state", AIE_CV_OB_STATE, 2, 6);
    OBA("obs_p_world-agent_postsubsidy_productivity", AIE_CV_OB_PROD, 1, n);
    OBA("obs_p_world-lagged_stringency_level", AIE_CV_OB_LAG, 1, n);
    OBA("obs_p_ControlUSStateOpenCloseStatus-agent_policy_indicators", AIE_CV_OB_POLICY, 1, n);
#undef OBA
#define OBP(name, idx, nd, d0) aie__add(tt, name, AIE_F32, p->a_cv_obs_p + 4 * (idx), po, nd, d0, 0, 0, 0, E)
    OBP("obs_p_time", 0, 1, 1);
    OBP("obs_p_FederalGovernmentSubsidy-t_until_next_subsidy", 1, 0, 0);
    OBP("obs_p_FederalGovernmentSubsidy-current_subsidy_level", 2, 0, 0);
    OBP("obs_p_VaccinationCampaign-t_until_next_vaccines", 3, 0, 0);
    OBP("obs_p_action_mask", 4, 1, p->MP);
#undef OBP
    aie__add(tt, "rewards_a", AIE_F32, p->a_rew_a, (int64_t)n * 4, 1, n, 0, 0, 0, E);
    aie__add(tt, "rewards_p", AIE_F32, p->a_rew_p, 4, 0, 0, 0, 0, 0, E);
    aie__add(tt, "done", AIE_U8, p->a_done, 1, 0, 0, 0, 0, 0, E);
  }
  return AIE_OK;
}

/* per-replica episode accumulators (see aie_params.a_metrics): allocation + tensor views */
static inline void aie__alloc_metrics(aie_params* p, int64_t* a) {
  const int n = p->n;
  int32_t m = 0;
  p->mo_tax_sched = m;  m += 8 * (p->has_tax ? p->NB : 0);
  p->mo_tax_income = m; m += 8 * (p->has_tax ? n : 0);
  p->mo_tax_paid = m;   m += 8 * (p->has_tax ? n : 0);
  p->mo_tax_eff = m;    m += 8;
  p->mo_cda = m;        m += 4 * (p->has_cda ? 2 * AIE_N_RES * n * 2 : 0);
  p->mo_tax_occ = m;    m += 4 * (p->has_tax ? p->NB : 0);
  p->mo_tax_days = m;   m += 4;
  p->met_bytes = (int32_t)aie__align(m, 16);
  p->a_metrics = *a;
  *a = aie__align(*a + (int64_t)p->E * p->met_bytes, 256);
}

static inline void aie__alloc_saez(const aie_config* c, aie_params* p, int64_t* a) {
  p->a_saez = 0; p->saez_stride = 0; p->saez_cap = 0; p->a_saez_global = 0; p->saez_global_cap = 0;
  if (!p->has_tax || c->tax_model != AIE_TAX_SAEZ) return;
  p->saez_cap = c->saez_buffer_size + p->n; /* a tax day appends n pairs before the oldest are dropped */
  p->saez_stride = (int32_t)aie__align(AIE_SAEZ_OFF_BUF + (int64_t)p->saez_cap * 16, 64);
  p->a_saez = *a;
  *a = aie__align(*a + (int64_t)p->E * p->saez_stride, 256);
  p->saez_global_cap = c->saez_global_capacity > 0 ? c->saez_global_capacity : 0;
  p->a_saez_global = *a;
  *a = aie__align(*a + 16 + (int64_t)p->saez_global_cap * 16, 256);
  const double top = c->tax_bracket_cutoffs[p->NB - 1], step = top / (double)AIE_SAEZ_BINS;
  for (int i = 0; i <= AIE_SAEZ_BINS; ++i) p->saez_edges[i] = (double)i * step + 0.0; /* np.linspace */
  p->saez_edges[AIE_SAEZ_BINS] = top;
}
static inline void aie__add_saez_tensors(const aie_params* p, aie_tensor_table* tt) {
  if (!p->saez_stride) return;
  const int64_t s0 = p->a_saez, ss = p->saez_stride, E = p->E;
  aie__add(tt, "saez_buffer_len", AIE_I32, s0, ss, 0, 0, 0, 0, 0, E);
  aie__add(tt, "saez_reached_min_samples", AIE_I32, s0 + 4, ss, 0, 0, 0, 0, 0, E);
  aie__add(tt, "saez_additions", AIE_I32, s0 + 8, ss, 0, 0, 0, 0, 0, E);  /* _additions_this_episode :541 */
  aie__add_shared(tt, "saez_global_len", AIE_I32, p->a_saez_global, 1, 1, 0);
  if (p->saez_global_cap)
    aie__add_shared(tt, "saez_global_buffer", AIE_F64, p->a_saez_global + 16, 2, p->saez_global_cap, 2);
  aie__add(tt, "saez_elas", AIE_F64, s0 + AIE_SAEZ_OFF_ELAS, ss, 1, 4, 0, 0, 0, E);
  aie__add(tt, "saez_running_avg_tax_rates", AIE_F64, s0 + AIE_SAEZ_OFF_AVG, ss, 1, p->NB, 0, 0, 0, E);
  aie__add(tt, "saez_next_rates", AIE_F64, s0 + AIE_SAEZ_OFF_NEXT, ss, 1, p->NB, 0, 0, 0, E);
  aie__add(tt, "saez_buffer", AIE_F64, s0 + AIE_SAEZ_OFF_BUF, ss, 2, p->saez_cap, 2, 0, 0, E);
}

/* dense-log event rows (include/aie.h: AIE_EV_*): at most n builds, 2n gathers, NB + n tax rows
 * and one trade per resting order of a commodity in a step */
static inline void aie__alloc_events(const aie_config* c, aie_params* p, int64_t* a) {
  const int n = p->n;
  p->ev_replicas = c->dense_log_replicas;
  p->ev_cap = p->ev_stride = 0;
  p->a_events = 0;
  if (p->ev_replicas <= 0) return;
  p->ev_cap = 4 * n + (p->has_tax ? p->NB : 0) + (p->has_cda ? AIE_N_RES * n * c->cda_max_num_orders : 0);
  p->ev_stride = (int32_t)aie__align(16 + (int64_t)p->ev_cap * AIE_EV_WORDS * 4, 64);
  p->a_events = *a;
  *a = aie__align(*a + (int64_t)p->ev_replicas * p->ev_stride, 256);
}
static inline void aie__add_event_tensors(const aie_params* p, aie_tensor_table* tt) {
  if (p->ev_replicas <= 0) return;
  aie__add(tt, "log_event_count", AIE_I32, p->a_events, p->ev_stride, 0, 0, 0, 0, 0, p->ev_replicas);
  aie__add(tt, "log_events", AIE_I32, p->a_events + 16, p->ev_stride, 2, p->ev_cap, AIE_EV_WORDS, 0, 0,
           p->ev_replicas);
}
static inline void aie__add_metrics_tensors(const aie_params* p, aie_tensor_table* tt) {
  const int64_t ms = p->met_bytes, m0 = p->a_metrics, E = p->E;
  const int n = p->n;
  if (p->has_cda) aie__add(tt, "metrics_cda_trades", AIE_I32, m0 + p->mo_cda, ms, 4, 2, AIE_N_RES, n, 2, E);
  if (p->has_tax) {
    aie__add(tt, "metrics_tax_schedule_sum", AIE_F64, m0 + p->mo_tax_sched, ms, 1, p->NB, 0, 0, 0, E);
    aie__add(tt, "metrics_tax_income_sum", AIE_F64, m0 + p->mo_tax_income, ms, 1, n, 0, 0, 0, E);
    aie__add(tt, "metrics_tax_paid_sum", AIE_F64, m0 + p->mo_tax_paid, ms, 1, n, 0, 0, 0, E);
    aie__add(tt, "metrics_tax_effective_rate_sum", AIE_F64, m0 + p->mo_tax_eff, ms, 0, 0, 0, 0, 0, E);
    aie__add(tt, "metrics_tax_bracket_occupancy", AIE_I32, m0 + p->mo_tax_occ, ms, 1, p->NB, 0, 0, 0, E);
    aie__add(tt, "metrics_tax_days", AIE_I32, m0 + p->mo_tax_days, ms, 0, 0, 0, 0, 0, E);
  }
}

/* one-step-economy (F/scenarios/one_step_economy/one_step_economy.py): no map, agents
 * hold coin / labor / skill / production; flat observations in sorted-key order:
 *   agent   PeriodicBracketTax-{curr_rates,is_first_day,is_tax_day,last_incomes,
 *           marginal_rate,tax_phase}, SimpleLabor-skill, time
 *   planner PeriodicBracketTax-{curr_rates,is_first_day,is_tax_day,last_incomes,tax_phase},
 *           time, world-equality, world-normalized_per_capita_productivity
 *   p{i}    PeriodicBracketTax-{curr_marginal_rate,last_income,last_marginal_rate}      */
static inline int aie__build_one_step_economy(const aie_config* c, aie_params* p, aie_tensor_table* tt) {
  const int n = p->n;
  int f = 0;
  p->fa_tax = f;   if (p->has_tax) f += AIE_FA_TAX_LEN(p->NB, n);
  p->fa_labor = f; if (p->has_labor) f += 1;
  p->fa_time = f;  f += 1;
  p->fa_world = f;
  p->FA = f;
  f = 0;
  p->fp_tax = f;   if (p->has_tax) f += AIE_FP_TAX_LEN(p->NB, n);
  p->fp_time = f;  f += 1;
  p->fp_world = f; f += 2;
  p->FP = f;
  p->fpa_tax = 0;
  p->fpa_world = p->has_tax ? AIE_FPA_TAX_LEN : 0;
  p->FPA = p->has_tax ? AIE_FPA_TAX_LEN : 0;
  p->mg_FA = aie__magic(p->FA);
  p->mg_MA = aie__magic(p->MA);

  int32_t cur = 0;
  p->o_inv_coin = aie__rec(&cur, 8 * n, 16);
  p->o_labor = aie__rec(&cur, 8 * n, 8);
  p->o_production = aie__rec(&cur, 8 * n, 8);
  p->o_util = aie__rec(&cur, 8 * (n + 1), 8);
  if (p->has_tax) {
    p->o_tax_last_coin = aie__rec(&cur, 8 * n, 8);
    p->o_tax_last_income = aie__rec(&cur, 8 * n, 8);
    p->o_tax_last_marginal_rate = aie__rec(&cur, 8 * n, 8);
    /* aie_kernels_ose.hip (ose_load_record) skips [o_tax_last_income, o_tax_last_marginal_rate + 8 n) as one dead range
     * when every step is a tax day: the two fields have to stay adjacent */
    if (p->o_tax_last_marginal_rate != p->o_tax_last_income + 8 * n) return AIE_E_INVALID;
    p->o_tax_total_collected = aie__rec(&cur, 8, 8);
    p->o_tax_cycle_pos = aie__rec(&cur, 4, 4);
    p->o_tax_last_completions = aie__rec(&cur, 4, 4);
    p->o_tax_rate_idx = aie__rec(&cur, 4 * p->NB, 4);
    if (c->tax_model == AIE_TAX_SAEZ) {
      p->o_tax_saez_rates = aie__rec(&cur, 8 * p->NB, 8);
      p->o_tax_saez_obs_rates = aie__rec(&cur, 8 * p->NB, 8);
    }
  }
  p->o_timestep = aie__rec(&cur, 4, 4);
  p->o_completions = aie__rec(&cur, 4, 4);
  p->o_auto_warmup = aie__rec(&cur, 4, 4);
  p->o_first_step = aie__rec(&cur, 4, 4);
  p->o_error_flags = aie__rec(&cur, 4, 4);
  p->o_sample_t = aie__rec(&cur, 4, 4);
  p->o_rew_slot = aie__rec(&cur, 4, 4);
  p->o_rew_epoch = aie__rec(&cur, 4, 4);
  p->o_mt_gauss = aie__rec(&cur, 8, 8);
  p->o_mt_pos = aie__rec(&cur, 4, 4);
  p->o_mt_has_gauss = aie__rec(&cur, 4, 4);
  p->o_mt = aie__rec(&cur, 4 * aie__rng_state_words(c), 16);
  /* behind the generator: per-agent fields a step only reads (SimpleLabor's skills; the escrow account, which no
   * component of this scenario moves) -- the kernels keep them in registers, they are not part of the LDS image
   * (everything before o_mt), which is what decides how many replicas a CU holds at once */
  p->o_skill = aie__rec(&cur, 8 * n, 16);
  p->o_esc_coin = aie__rec(&cur, 8 * n, 8);
  p->rec_bytes = (int32_t)aie__align(cur, 16);

  const int64_t E = p->E;
  int64_t a = 0;
  p->a_records = a;      a = aie__align(a + E * (int64_t)p->rec_bytes, 256);
  p->a_obs_a_flat = a;   a = aie__align(a + E * n * p->FA * 4, 256);
  p->a_obs_a_mask = a;   a = aie__align(a + E * n * p->MA * 4, 256);
  p->a_obs_a_time = a;   a = aie__align(a + E * n * 4, 256);
  p->a_obs_p_flat = a;   a = aie__align(a + E * p->FP * 4, 256);
  p->a_obs_p_mask = a;   a = aie__align(a + E * p->MP * 4, 256);
  p->a_obs_p_time = a;   a = aie__align(a + E * 4, 256);
  p->a_obs_p_agents = a; a = aie__align(a + E * n * (p->FPA ? p->FPA : 1) * 4, 256);
  p->a_rew_a = a; a = aie__align(a + E * n * 4, 256);
  p->a_rew_p = a; a = aie__align(a + E * 4, 256);
  p->a_done = a;  a = aie__align(a + E, 256);
  aie__alloc_metrics(p, &a);
  aie__alloc_events(c, p, &a);
  aie__alloc_saez(c, p, &a);
  p->arena_bytes = a;

  if (tt) {
    const int64_t rs = p->rec_bytes, r0 = p->a_records;
    aie__add_metrics_tensors(p, tt);
    aie__add_event_tensors(p, tt);
    aie__add_saez_tensors(p, tt);
#define REC(name, dt, off, nd, d0) aie__add(tt, name, dt, r0 + (off), rs, nd, d0, 0, 0, 0, E)
    REC("inv_coin", AIE_F64, p->o_inv_coin, 1, n);
    REC("esc_coin", AIE_F64, p->o_esc_coin, 1, n);
    REC("labor", AIE_F64, p->o_labor, 1, n);
    REC("skill", AIE_F64, p->o_skill, 1, n);
    REC("production", AIE_F64, p->o_production, 1, n);
    REC("util", AIE_F64, p->o_util, 1, n + 1);
    if (p->has_tax) {
      REC("tax_cycle_pos", AIE_I32, p->o_tax_cycle_pos, 0, 0);
      REC("tax_last_completions", AIE_I32, p->o_tax_last_completions, 0, 0);
      REC("tax_rate_idx", AIE_I32, p->o_tax_rate_idx, 1, p->NB);
      if (c->tax_model == AIE_TAX_SAEZ) {
        REC("tax_saez_bracket_rates", AIE_F64, p->o_tax_saez_rates, 1, p->NB);
        REC("tax_saez_observed_rates", AIE_F64, p->o_tax_saez_obs_rates, 1, p->NB);
      }
      REC("tax_last_coin", AIE_F64, p->o_tax_last_coin, 1, n);
      REC("tax_last_income", AIE_F64, p->o_tax_last_income, 1, n);
      REC("tax_last_marginal_rate", AIE_F64, p->o_tax_last_marginal_rate, 1, n);
      REC("tax_total_collected", AIE_F64, p->o_tax_total_collected, 0, 0);
    }
    REC("timestep", AIE_I32, p->o_timestep, 0, 0);
    REC("completions", AIE_I32, p->o_completions, 0, 0);
    REC("sample_t", AIE_I32, p->o_sample_t, 0, 0);
    REC("rew_log_slot", AIE_I32, p->o_rew_slot, 0, 0);
    REC("labor_first_step", AIE_I32, p->o_first_step, 0, 0);
    REC("error_flags", AIE_I32, p->o_error_flags, 0, 0);
    REC("mt", AIE_U32, p->o_mt, 1, aie__rng_state_words(&p->c));
    REC("mt_pos", AIE_I32, p->o_mt_pos, 0, 0);
    REC("mt_has_gauss", AIE_I32, p->o_mt_has_gauss, 0, 0);
    REC("mt_gauss", AIE_F64, p->o_mt_gauss, 0, 0);
#undef REC
#define DENSE(name, dt, off, nd, d0, d1)                                                    \
  do {                                                                                      \
    int64_t dd[2] = {d0, d1};                                                               \
    int64_t es = aie__dtype_size(dt);                                                       \
    for (int q = 0; q < nd; ++q) es *= dd[q];                                               \
    aie__add(tt, name, dt, off, es, nd, d0, d1, 0, 0, E);                                   \
  } while (0)
    DENSE("obs_a_flat", AIE_F32, p->a_obs_a_flat, 2, n, p->FA);
    DENSE("obs_a_action_mask", AIE_F32, p->a_obs_a_mask, 2, n, p->MA);
    DENSE("obs_a_time", AIE_F32, p->a_obs_a_time, 2, n, 1);
    DENSE("obs_p_flat", AIE_F32, p->a_obs_p_flat, 1, p->FP, 0);
    DENSE("obs_p_action_mask", AIE_F32, p->a_obs_p_mask, 1, p->MP, 0);
    DENSE("obs_p_time", AIE_F32, p->a_obs_p_time, 1, 1, 0);
    if (p->FPA) DENSE("obs_p_agents", AIE_F32, p->a_obs_p_agents, 2, n, p->FPA);
    DENSE("rewards_a", AIE_F32, p->a_rew_a, 1, n, 0);
    DENSE("rewards_p", AIE_F32, p->a_rew_p, 0, 0, 0);
    DENSE("done", AIE_U8, p->a_done, 0, 0, 0);
#undef DENSE
  }
  (void)c;
  return AIE_OK;
}

/* Validates the config (mirrors the reference's constructor asserts) and derives
 * every dimension / offset.  `tt` may be NULL. */
static inline int aie_build_params(const aie_config* c, aie_params* p, aie_tensor_table* tt,
                                   char* err, size_t errlen) {
  memset(p, 0, sizeof(*p));
  if (tt) tt->n = 0;
  if (c->abi_version != AIE_ABI_VERSION) AIE__FAIL("abi_version %d != %d", c->abi_version, AIE_ABI_VERSION);
  if (c->n_envs < 1) AIE__FAIL("n_envs must be >= 1");
  if (c->n_agents < 2) AIE__FAIL("n_agents must be >= 2 (base_env.py:223)");
  if (c->scenario != AIE_SCN_GTB && c->scenario != AIE_SCN_ONE_STEP_ECONOMY && c->scenario != AIE_SCN_COVID)
    AIE__FAIL("unknown scenario %d", c->scenario);
  if (c->rng_mode != AIE_RNG_NUMPY && c->rng_mode != AIE_RNG_FAST) AIE__FAIL("unknown rng_mode %d", c->rng_mode);
  if (c->scenario == AIE_SCN_COVID) {
    if (c->episode_length < 1) AIE__FAIL("episode_length must be >= 1 (base_env.py:254)");
    return aie__build_covid(c, p, tt, err, errlen);
  }
  if (c->scenario == AIE_SCN_GTB && c->n_agents > AIE_MAX_AGENTS - 2)
    AIE__FAIL("n_agents = %d: the spatial scenarios hold at most %d mobile agents per replica here (one lane of a 64-lane "
              "wavefront each; the reference has no upper bound, base_env.py:221-224)", c->n_agents, AIE_MAX_AGENTS - 2);
  if (c->scenario == AIE_SCN_ONE_STEP_ECONOMY && c->n_agents > AIE_MAX_AGENTS_WIDE)
    AIE__FAIL("n_agents = %d: one-step-economy holds at most %d agents per replica here (the reference has no upper "
              "bound, base_env.py:221-224)", c->n_agents, AIE_MAX_AGENTS_WIDE);
  if (c->world_h < 1 || c->world_w < 1 || c->world_h > 255 || c->world_w > 255)
    AIE__FAIL("world_size out of range");
  if (c->episode_length < 1) AIE__FAIL("episode_length must be >= 1 (base_env.py:254)");
  if (c->dense_log_replicas < 0 || c->dense_log_replicas > c->n_envs)
    AIE__FAIL("dense_log_replicas must be in [0, n_envs]");
  if (c->n_components < 0 || c->n_components > AIE_MAX_COMPONENTS) AIE__FAIL("bad n_components");
  for (int i = 0; i < c->n_components; ++i) {
    int k = c->components[i];
    if (k < AIE_COMP_BUILD || (k > AIE_COMP_SIMPLE_LABOR && k != AIE_COMP_WEALTH_REDISTRIBUTION))
      AIE__FAIL("unknown component id %d", k);
    if (c->scenario == AIE_SCN_GTB && k == AIE_COMP_SIMPLE_LABOR)
      AIE__FAIL("SimpleLabor is only supported with the one-step-economy scenario");
    if (c->scenario == AIE_SCN_ONE_STEP_ECONOMY && k != AIE_COMP_SIMPLE_LABOR && k != AIE_COMP_TAX &&
        k != AIE_COMP_WEALTH_REDISTRIBUTION)
      AIE__FAIL("one-step-economy supports SimpleLabor, PeriodicBracketTax and WealthRedistribution only");
    for (int j = 0; j < i; ++j)
      if (c->components[j] == k) AIE__FAIL("component %d listed twice", k);
  }
  const int gtb = c->scenario == AIE_SCN_GTB;
  if (gtb && (c->obs_range < 0 || c->obs_range > 15)) AIE__FAIL("mobile_agent_observation_range out of range");
  for (int r = 0; gtb && r < AIE_N_RES; ++r) {
    if (c->regen_halfwidth[r] < 0 || c->regen_halfwidth[r] > 3)
      AIE__FAIL("regen_halfwidth must be in [0, 3] (dynamic_layout.py:152-153)");
    if (!(c->regen_weight[r] >= 0.0 && c->regen_weight[r] <= 1.0)) AIE__FAIL("regen_weight not in [0,1]");
    if (c->max_health[r] < 1 || c->max_health[r] > 255) AIE__FAIL("max_health out of range");
  }
  if (c->layout_gen != AIE_LAYOUT_FIXED) {
    if (!gtb) AIE__FAIL("layout_gen needs a gather-trade-build scenario");
    if (c->layout_gen < 0 || c->layout_gen > AIE_LAYOUT_MULTI_ZONE) AIE__FAIL("unknown layout_gen %d", c->layout_gen);
    if (c->shared_layout) AIE__FAIL("generated layouts are per replica: shared_layout must be 0");
    if (c->world_h * c->world_w > 4096) {  /* (the generator's planes live in LDS: 18 B per cell beside the record image) */
      if (err) snprintf(err, errlen, "layouts are generated on the device for worlds of up to 4096 cells (64 x 64)");
      return AIE_E_UNSUPPORTED;
    }
    for (int r = 0; r < AIE_N_RES; ++r) {
      if (!(c->layout_coverage[r] > 0.0 && c->layout_coverage[r] < 1.0)) AIE__FAIL("layout_coverage not in (0, 1)");
      if (!(c->layout_clump[r] > 0.0 && c->layout_clump[r] <= 1.0)) AIE__FAIL("layout_clump not in (0, 1]");
    }
    if (c->layout_gen == AIE_LAYOUT_MULTI_ZONE) {
      const int regions = c->mz_rows * c->mz_cols, zones = c->mz_zones[0] + c->mz_zones[1] + c->mz_zones[2];
      if (c->mz_rows < 1 || c->mz_cols < 1 || regions > 256 || zones > regions || c->mz_zones[0] < 0 ||
          c->mz_zones[1] < 0 || c->mz_zones[2] < 0)
        AIE__FAIL("multi_zone: partitions / zone counts out of range");
    }
  }
  if (!(c->starting_agent_coin >= 0.0)) AIE__FAIL("starting_agent_coin must be >= 0");
  if (!(c->isoelastic_eta >= 0.0 && c->isoelastic_eta <= 1.0)) AIE__FAIL("isoelastic_eta not in [0,1]");
  if (gtb && !(c->energy_cost >= 0.0)) AIE__FAIL("energy_cost must be >= 0");
  if (gtb && !(c->energy_warmup_constant >= 0.0)) AIE__FAIL("energy_warmup_constant must be >= 0");
  if (!(c->mixing_weight_gini_vs_coin >= 0.0 && c->mixing_weight_gini_vs_coin <= 1.0))
    AIE__FAIL("mixing_weight_gini_vs_coin not in [0,1]");

  p->c = *c;
  p->sh_energy_warmup = c->energy_warmup_constant > 0.0 ? 1 : 0;
  p->sh_eta_is_one = c->isoelastic_eta == 1.0 ? 1 : 0;
  p->E = c->n_envs;
  p->n = c->n_agents;
  p->H = c->world_h;
  p->W = c->world_w;
  p->HW = c->world_h * c->world_w;
  p->has_build = aie__has(c, AIE_COMP_BUILD);
  p->has_cda = aie__has(c, AIE_COMP_CDA);
  p->has_gather = aie__has(c, AIE_COMP_GATHER);
  p->has_tax = aie__has(c, AIE_COMP_TAX);
  p->has_labor = aie__has(c, AIE_COMP_SIMPLE_LABOR);
  if (p->has_labor) {
    /* an agent's mask row is [NO-OP, hours...]: the one-step-economy kernels store a row with one 16-byte quad per lane
     * of a wavefront (ose_store_rows), which holds 256 floats */
    if (c->labor_num_hours < 1 || c->labor_num_hours > 255)
      AIE__FAIL("SimpleLabor.num_labor_hours out of range (%d: 1 .. 255, an agent's mask row is at most 256 entries)", c->labor_num_hours);
    if (!(c->labor_pmsm > 0.0)) AIE__FAIL("SimpleLabor.payment_max_skill_multiplier must be > 0");
  }
  if (!gtb) {
    if (c->ose_agent_reward_type == AIE_AGENT_REW_COIN_MINUS_LABOR_COST && !(c->ose_labor_exponent > 1.0))
      AIE__FAIL("labor_exponent must be > 1 (rewards.py:69)");
    if (c->ose_agent_reward_type != AIE_AGENT_REW_COIN_MINUS_LABOR_COST && c->ose_agent_reward_type != AIE_AGENT_REW_ISOELASTIC)
      AIE__FAIL("unknown agent_reward_type");
  }
  p->CM = c->has_water ? 6 : 5;
  p->WV = 2 * c->obs_range + 1;

  if (p->has_build) {
    if (c->build_payment < 0) AIE__FAIL("Build.payment must be >= 0");
    if (c->build_payment_max_skill_multiplier < 1) AIE__FAIL("Build.payment_max_skill_multiplier must be >= 1");
    if (!(c->build_labor >= 0.0)) AIE__FAIL("Build.build_labor must be >= 0");
    if (c->build_skill_dist < 0 || c->build_skill_dist > 2) AIE__FAIL("Build.skill_dist invalid");
  }
  if (p->has_gather) {
    if (!(c->move_labor >= 0.0) || !(c->collect_labor >= 0.0)) AIE__FAIL("Gather labor must be >= 0");
    if (c->gather_skill_dist < 0 || c->gather_skill_dist > 2) AIE__FAIL("Gather.skill_dist invalid");
  }
  if (c->split_water_line) {
    if (c->scenario != AIE_SCN_GTB) AIE__FAIL("split_water_line only applies to the gather-trade-build scenarios");
    if (c->split_water_line <= 0 || c->split_water_line >= c->world_h - 1) AIE__FAIL("water_row out of range (layout_from_file.py:722)");
    if (c->fixed_four_skill_and_loc) AIE__FAIL("The split layout scenario does not support fixed_four_skill_and_loc (layout_from_file.py:712-716)");
    if (!(p->has_build && c->build_skill_dist == AIE_SKILL_PARETO)) AIE__FAIL("split layout requires Build with skill_dist='pareto' (layout_from_file.py:748)");
    if (!c->has_water) AIE__FAIL("split layout needs the Water landmark");
  }
  if (c->fixed_four_skill_and_loc && !(p->has_build && c->build_skill_dist == AIE_SKILL_PARETO))
    AIE__FAIL("fixed_four_skill_and_loc requires Build with skill_dist='pareto' (layout_from_file.py:177-178)");
  if (p->has_cda) {
    if (c->cda_max_bid_ask < 1 || c->cda_max_bid_ask > 126) AIE__FAIL("CDA.max_bid_ask out of range");
    if (c->cda_order_duration < 1 || c->cda_order_duration > 32000) AIE__FAIL("CDA.order_duration out of range");
    if (c->cda_max_num_orders < 1 || c->cda_max_num_orders > 255) AIE__FAIL("CDA.max_num_orders out of range");
    if (!(c->cda_order_labor >= 0.0)) AIE__FAIL("CDA.order_labor must be >= 0");
    p->P = c->cda_max_bid_ask + 1;
    p->M = c->n_agents * c->cda_max_num_orders;
  }
  if (p->has_tax) {
    if (c->tax_period < 1) AIE__FAIL("Tax.period must be > 0");
    if (c->tax_n_brackets < 2 || c->tax_n_brackets > AIE_MAX_BRACKETS) AIE__FAIL("Tax.n_brackets out of range");
    if (c->tax_model < AIE_TAX_MODEL_WRAPPER || c->tax_model > AIE_TAX_SAEZ) AIE__FAIL("unknown tax_model");
    if (c->tax_model == AIE_TAX_SAEZ) {
      if (c->saez_buffer_size < 1 || c->saez_buffer_size > 4096) AIE__FAIL("saez_buffer_size out of range");
      if (!(c->tax_rate_min >= 0.0 && c->tax_rate_min <= c->tax_rate_max)) AIE__FAIL("rate_min / rate_max");
      if (c->saez_fixed_elas_given && !(c->saez_fixed_elas >= 0.0)) AIE__FAIL("saez_fixed_elas must be >= 0");
    }
    if (c->tax_bracket_cutoffs[0] != 0.0) AIE__FAIL("bracket_cutoffs[0] must be 0 (redistribution.py:243)");
    if (c->tax_model == AIE_TAX_MODEL_WRAPPER && !c->tax_disable) {
      if (c->tax_n_disc_rates < 2 || c->tax_n_disc_rates > AIE_MAX_RATES) AIE__FAIL("Tax.n_disc_rates out of range");
      p->planner_acts = 1;
    } else if (c->tax_model == AIE_TAX_MODEL_WRAPPER) {
      if (c->tax_n_disc_rates < 1 || c->tax_n_disc_rates > AIE_MAX_RATES) AIE__FAIL("Tax.n_disc_rates out of range");
    }
    p->NB = c->tax_n_brackets;
  }

  /* ---- action subspaces, registration order = component order ----------------- */
  if (c->host_a_n < 0 || c->host_a_n > AIE_MAX_HOST_SUBSPACES || c->host_p_n < 0 || c->host_p_n > AIE_MAX_HOST_SUBSPACES)
    AIE__FAIL("host components: at most %d action subspaces per agent class (%d for the agents, %d for the planner)",
              AIE_MAX_HOST_SUBSPACES, c->host_a_n, c->host_p_n);
  if ((c->host_a_n || c->host_p_n) && !gtb)
    AIE__FAIL("host components' action subspaces: gather-trade-build scenarios only");
  for (int k = 0; k < c->host_a_n + c->host_p_n; ++k) {
    const int pl = k >= c->host_a_n, q = pl ? k - c->host_a_n : k;
    const int32_t* dim = pl ? c->host_p_dim : c->host_a_dim;
    const int32_t* bef = pl ? c->host_p_before : c->host_a_before;
    if (dim[q] < 1 || dim[q] > AIE_MAX_MASK) AIE__FAIL("host components: %s subspace %d has %d choices", pl ? "planner" : "agent", q, dim[q]);
    if (bef[q] < 0 || bef[q] > c->n_components || (q > 0 && bef[q] < bef[q - 1]))
      AIE__FAIL("host components: %s subspace %d sits behind %d built-in components (of %d; non-decreasing)",
                pl ? "planner" : "agent", q, bef[q], c->n_components);
  }
  p->n_host_a = c->host_a_n;
  p->n_host_p = c->host_p_n;
  int ns = 0, base = 1, hk = 0;
  for (int i = 0; i <= c->n_components; ++i) {
    /* the foreign subspaces listed ahead of built-in component i (i == n_components: behind the last one) */
    for (; hk < c->host_a_n && c->host_a_before[hk] == i; ++hk) {
      if (ns >= AIE_MAX_SUBSPACES) AIE__FAIL("more than %d agent action subspaces", AIE_MAX_SUBSPACES);
      p->sub_a_slot[ns] = AIE_SUB_HOST; p->sub_a_dim[ns] = c->host_a_dim[hk]; ns++;
    }
    if (i == c->n_components) break;
    switch (c->components[i]) {  /* (at most 7 built-in slots + AIE_MAX_HOST_SUBSPACES <= AIE_MAX_SUBSPACES) */
      case AIE_COMP_BUILD:
        p->sub_a_slot[ns] = AIE_SUB_BUILD; p->sub_a_dim[ns] = 1; ns++; break;
      case AIE_COMP_CDA:
        for (int r = 0; r < AIE_N_RES; ++r) {
          p->sub_a_slot[ns] = r ? AIE_SUB_BUY1 : AIE_SUB_BUY0; p->sub_a_dim[ns] = p->P; ns++;
          p->sub_a_slot[ns] = r ? AIE_SUB_SELL1 : AIE_SUB_SELL0; p->sub_a_dim[ns] = p->P; ns++;
        }
        break;
      case AIE_COMP_GATHER:
        p->sub_a_slot[ns] = AIE_SUB_GATHER; p->sub_a_dim[ns] = 4; ns++; break;
      case AIE_COMP_SIMPLE_LABOR:
        p->sub_a_slot[ns] = AIE_SUB_LABOR; p->sub_a_dim[ns] = c->labor_num_hours; ns++; break;
      default: break;
    }
  }
  p->n_sub_a = ns;
  for (int s = 0; s < ns; ++s) { p->sub_a_base[s] = base; base += p->sub_a_dim[s]; }
  p->A = base;
  if (c->multi_action_mode_agents) {
    if (ns == 0) { p->act_a_width = 1; }      /* PassiveAgentPlaceholder, base_agent.py:158-161 */
    else p->act_a_width = ns;
  } else {
    p->act_a_width = 1;
  }
  p->n_sub_p = p->planner_acts ? p->NB : 0;
  p->sub_p_dim = p->planner_acts ? c->tax_n_disc_rates : 0;
  {
    /* the planner's rows: the foreign ones listed ahead of the tax component, the tax brackets, the other foreign ones */
    int tax_at = c->n_components;  /* (no acting tax component: every foreign row counts as "ahead", the block is empty) */
    for (int i = 0; i < c->n_components; ++i)
      if (c->components[i] == AIE_COMP_TAX && p->n_sub_p) tax_at = i;
    const int multi = c->multi_action_mode_planner ? 1 : 0;
    int row = 0, sbase = 1, moff = multi ? 0 : 1, placed = 0;
    p->p_rows_uniform = 1;
    p->p_row_dim = p->n_sub_p ? p->sub_p_dim : (c->host_p_n ? c->host_p_dim[0] : 0);
    for (int k = 0; k <= c->host_p_n; ++k) {
      if (!placed && (k == c->host_p_n || c->host_p_before[k] > tax_at)) {
        p->tax_p_row0 = row; p->tax_p_base = sbase; p->tax_p_moff = moff;
        row += p->n_sub_p; sbase += p->n_sub_p * p->sub_p_dim; moff += p->n_sub_p * (multi + p->sub_p_dim);
        placed = 1;
      }
      if (k == c->host_p_n) break;
      p->hp_dim[k] = c->host_p_dim[k]; p->hp_row[k] = row; p->hp_base[k] = sbase; p->hp_moff[k] = moff;
      if (p->hp_dim[k] != p->p_row_dim) p->p_rows_uniform = 0;
      row += 1; sbase += p->hp_dim[k]; moff += multi + p->hp_dim[k];
    }
    p->AP = sbase;
    /* (at most AIE_MAX_BRACKETS + AIE_MAX_HOST_SUBSPACES rows; no table on the planner's side is sized by a row count) */
    if (multi) { p->act_p_width = row ? row : 1; p->MP = row ? moff : 1; }
    else { p->act_p_width = 1; p->MP = moff; }
  }

  /* ---- flattened masks (base_agent.py:440-460) -------------------------------- */
  if (c->multi_action_mode_agents) {
    p->MA = 0;
    for (int s = 0; s < ns; ++s) p->MA += 1 + p->sub_a_dim[s];
    if (ns == 0) p->MA = 1;
  } else {
    p->MA = p->A;
  }
  if (p->MA > AIE_MAX_MASK) AIE__FAIL("flattened action mask too long (%d > %d)", p->MA, AIE_MAX_MASK);
  /* (nothing on the planner's side is sized by AIE_MAX_MASK -- the tax rows alone may reach 16 x 65 entries; the bound
   * only keeps foreign subspaces within what the agents' side accepts) */
  if (p->n_host_p) {
    const int foreign = p->MP - p->n_sub_p * ((c->multi_action_mode_planner ? 1 : 0) + p->sub_p_dim);
    if (foreign > AIE_MAX_MASK)
      AIE__FAIL("flattened planner action mask too long (%d entries outside the tax brackets' > %d)", foreign, AIE_MAX_MASK);
  }
  {
    /* mask bits (kernel): 0 build | 1..4 move L,R,U,D | 5,6 sell Stone,Wood | 8..15, 16..23:
     * number of affordable bid prices for Stone, Wood */
    const int multi = c->multi_action_mode_agents ? 1 : 0;
    int m = 0;
    if (!multi) p->mask_test[m++] = 0;                                 /* leading NO-OP: always 1 */
    for (int sub = 0; sub < ns; ++sub) {
      if (multi) p->mask_test[m++] = 0;                                /* the subspace's NO-OP   */
      for (int l = 0; l < p->sub_a_dim[sub]; ++l) {
        uint32_t sh = 0, msk = 1, thr = 1;
        switch (p->sub_a_slot[sub]) {
          case AIE_SUB_BUILD: sh = 0; break;
          case AIE_SUB_GATHER: sh = 1 + (uint32_t)l; break;
          case AIE_SUB_SELL0: sh = 5; break;
          case AIE_SUB_SELL1: sh = 6; break;
          case AIE_SUB_BUY0: sh = 8; msk = 0xff; thr = (uint32_t)l + 1; break;
          case AIE_SUB_BUY1: sh = 16; msk = 0xff; thr = (uint32_t)l + 1; break;
          default: msk = 0; thr = 0; break;                            /* unmasked subspace      */
        }
        p->mask_test[m++] = sh | (msk << 8) | (thr << 16);
      }
    }
    if (ns == 0 && multi) p->mask_test[m++] = 0;
  }

  /* ---- flat observations: sorted keys ----------------------------------------- */
  {
    int f = 0;
    p->fa_build = f;  if (p->has_build) f += 2;
    p->fa_cda = f;    if (p->has_cda) f += AIE_FA_CDA_LEN(p->P);
    p->fa_gather = f; if (p->has_gather) f += 1;
    p->fa_tax = f;    if (p->has_tax) f += AIE_FA_TAX_LEN(p->NB, p->n);
    p->fa_time = f;   f += 1;
    /* inventory-Coin,-Stone,-Wood, loc-col, loc-row; with full_observability the location is
     * only conveyed through the maps (layout_from_file.py:466-472) */
    p->fa_world = f;  f += c->full_observability ? 3 : 5;
    p->FA = f;
    f = 0;
    p->fp_cda = f;    if (p->has_cda) f += AIE_FP_CDA_LEN(p->P);
    p->fp_tax = f;    if (p->has_tax) f += AIE_FP_TAX_LEN(p->NB, p->n);
    p->fp_time = f;   f += 1;
    p->fp_world = f;  f += 3;
    p->FP = f;
    f = 0;
    p->fpa_tax = f;   if (p->has_tax) f += AIE_FPA_TAX_LEN;
    /* the scenario's per-agent planner fragments only exist with egocentric observations (:508-515) */
    p->fpa_world = f; if (!c->full_observability) f += 3 + (c->planner_gets_spatial_info ? 2 : 0);
    p->FPA = f;
  }

  p->mg_WV2 = aie__magic((int64_t)p->WV * p->WV);
  p->mg_WV = aie__magic(p->WV);
  p->mg_MA = aie__magic(p->MA);
  p->mg_FA = aie__magic(p->FA);
  p->mg_P = aie__magic(p->P);
  p->mg_2P = aie__magic(2 * p->P);
  p->mg_taxA = aie__magic(AIE_FA_TAX_LEN(p->NB, p->n));
  p->mg_HW = aie__magic(p->HW);
  p->mg_W = aie__magic(p->W);
  p->mg_sub_p = aie__magic(1 + p->sub_p_dim);
  p->mg_sub_p_dim = aie__magic(p->sub_p_dim > 0 ? p->sub_p_dim : 1);

  if (!gtb) return aie__build_one_step_economy(c, p, tt);

  /* ---- per-replica record ------------------------------------------------------ */
  const int n = p->n, HW = p->HW, R = AIE_N_RES;
  int32_t cur = 0;
  p->o_cells = aie__rec(&cur, 4 * HW, 16);
  p->regen_conv = c->regen_halfwidth[0] > 0 || c->regen_halfwidth[1] > 0;
  p->regen_general = (c->regen_halfwidth[0] > 0 && c->max_health[0] > 1) || (c->regen_halfwidth[1] > 0 && c->max_health[1] > 1);
  if (p->regen_conv) p->o_regen_count = aie__rec(&cur, AIE_N_RES * HW, 16);
  for (int r = 0; r < AIE_N_RES; ++r) {
    /* convolve2d accumulates sum += health * kernel over the window: m equal terms k, in sequence */
    const int d = 1 + 2 * c->regen_halfwidth[r];
    const double k = c->regen_weight[r] / (double)(d * d);
    p->regen_p[r][0] = 0.0;
    for (int m = 1; m < 50; ++m) p->regen_p[r][m] = p->regen_p[r][m - 1] + k;
  }
  p->o_inv_coin = aie__rec(&cur, 8 * n, 8);
  p->o_esc_coin = aie__rec(&cur, 8 * n, 8);
  p->o_labor = aie__rec(&cur, 8 * n, 8);
  p->o_build_payment = aie__rec(&cur, 8 * n, 8);
  p->o_build_skill = aie__rec(&cur, 8 * n, 8);
  p->o_bonus_gather_prob = aie__rec(&cur, 8 * n, 8);
  p->o_util = aie__rec(&cur, 8 * (n + 1), 8);
  p->o_loc_r = aie__rec(&cur, 4 * n, 4);
  p->o_loc_c = aie__rec(&cur, 4 * n, 4);
  p->o_inv_res = aie__rec(&cur, 4 * R * n, 4);
  p->o_esc_res = aie__rec(&cur, 4 * R * n, 4);
  if (p->has_cda) {
    p->o_cda_price_history = aie__rec(&cur, 8 * R * n * p->P, 8);
    p->o_cda_n_bids = aie__rec(&cur, 4 * R, 4);
    p->o_cda_n_asks = aie__rec(&cur, 4 * R, 4);
    p->o_cda_bids = aie__rec(&cur, 4 * R * p->M, 4);
    p->o_cda_asks = aie__rec(&cur, 4 * R * p->M, 4);
    p->o_cda_n_orders = aie__rec(&cur, 4 * R * n, 4);
    p->o_cda_bid_hist = aie__rec(&cur, R * n * p->P, 4);
    p->o_cda_ask_hist = aie__rec(&cur, R * n * p->P, 4);
  }
  if (p->has_tax) {
    p->o_tax_last_coin = aie__rec(&cur, 8 * n, 8);
    p->o_tax_last_income = aie__rec(&cur, 8 * n, 8);
    p->o_tax_last_marginal_rate = aie__rec(&cur, 8 * n, 8);
    p->o_tax_total_collected = aie__rec(&cur, 8, 8);
    p->o_tax_cycle_pos = aie__rec(&cur, 4, 4);
    p->o_tax_last_completions = aie__rec(&cur, 4, 4);
    p->o_tax_rate_idx = aie__rec(&cur, 4 * p->NB, 4);
    if (c->tax_model == AIE_TAX_SAEZ) {
      p->o_tax_saez_rates = aie__rec(&cur, 8 * p->NB, 8);
      p->o_tax_saez_obs_rates = aie__rec(&cur, 8 * p->NB, 8);
    }
  }
  p->o_timestep = aie__rec(&cur, 4, 4);
  p->o_completions = aie__rec(&cur, 4, 4);
  p->o_auto_warmup = aie__rec(&cur, 4, 4);
  p->o_obs_valid = aie__rec(&cur, 4, 4);
  p->o_error_flags = aie__rec(&cur, 4, 4);
  p->o_sample_t = aie__rec(&cur, 4, 4);
  p->o_rew_slot = aie__rec(&cur, 4, 4);
  p->o_rew_epoch = aie__rec(&cur, 4, 4);
  p->o_mask_bits = aie__rec(&cur, 4 * n, 4);
  p->o_mask_p_open = aie__rec(&cur, 4, 4);
  p->o_mt_gauss = aie__rec(&cur, 8, 8);
  p->o_mt_pos = aie__rec(&cur, 4, 4);
  p->o_mt_has_gauss = aie__rec(&cur, 4, 4);
  p->o_mt = aie__rec(&cur, 4 * aie__rng_state_words(c), 16);
  p->o_src_n = p->o_src_list = 0;
  if (aie__record_src_list(c)) {  /* behind the generator's state: not part of the LDS image (everything before o_mt) */
    p->o_src_n = aie__rec(&cur, 16, 16);
    p->o_src_list = aie__rec(&cur, 2 * AIE_SRC_CAP, 16);
  }
  p->o_cells8 = aie__cell_plane(c) ? aie__rec(&cur, (int32_t)aie__align(HW, 16), 16) : 0;  /* (likewise outside the image) */
  p->rec_bytes = (int32_t)aie__align(cur, 16);

  /* ---- arena ------------------------------------------------------------------- */
  const int64_t E = p->E;
  int64_t a = 0;
  p->a_records = a; a = aie__align(a + E * (int64_t)p->rec_bytes, 256); /* (0: the step kernel's record copies rely on it) */
  p->am_ch = c->full_observability ? p->CM : p->CM + 1;
  p->am_h = c->full_observability ? p->H : p->WV;
  p->am_w = c->full_observability ? p->W : p->WV;
  const int64_t wv2 = (int64_t)p->am_h * p->am_w;
  p->a_obs_a_map = a;  a = aie__align(a + E * n * p->am_ch * wv2 * 4, 256);
  p->a_obs_a_idx = a;  a = aie__align(a + E * n * 2 * wv2 * 2, 256);
  p->a_obs_a_flat = a; a = aie__align(a + E * n * p->FA * 4, 256);
  p->a_obs_a_mask = a; a = aie__align(a + E * n * p->MA * 4, 256);
  p->a_obs_a_time = a; a = aie__align(a + E * n * 4, 256);
  if (c->planner_gets_spatial_info) {
    p->a_obs_p_map = a; a = aie__align(a + E * p->CM * HW * 4, 256);
    p->a_obs_p_idx = a; a = aie__align(a + E * 2 * HW * 2, 256);
  }
  p->a_obs_p_flat = a;   a = aie__align(a + E * p->FP * 4, 256);
  p->a_obs_p_mask = a;   a = aie__align(a + E * p->MP * 4, 256);
  p->a_obs_p_time = a;   a = aie__align(a + E * 4, 256);
  p->a_obs_p_agents = a; a = aie__align(a + E * n * (p->FPA ? p->FPA : 1) * 4, 256);
  p->a_rew_a = a; a = aie__align(a + E * n * 4, 256);
  p->a_rew_p = a; a = aie__align(a + E * 4, 256);
  p->a_done = a;  a = aie__align(a + E, 256);
  aie__alloc_metrics(p, &a);
  aie__alloc_events(c, p, &a);
  aie__alloc_saez(c, p, &a);
  p->a_layout_prob = a;
  if (c->layout_gen != AIE_LAYOUT_FIXED) a = aie__align(a + (int64_t)AIE_N_RES * HW * 8, 256);
  p->layout_stage_stride = (HW + 15) / 16 * 16;
  p->a_layout_stage = p->a_layout_tag = p->a_layout_ctl = a;
  if (aie__layout_staged(c)) {
    p->a_layout_stage = a; a = aie__align(a + E * p->layout_stage_stride, 256);
    p->a_layout_tag = a;   a = aie__align(a + E * 8, 256);
    p->a_layout_ctl = a;   a = aie__align(a + 16, 256);
  }
  p->a_src_list = a;
  if (aie__shared_src_list(c)) a = aie__align(a + 16 + 2 * AIE_SRC_CAP, 256);
  p->a_host_act_a = p->a_host_act_p = a;
  if (p->n_host_a) { p->a_host_act_a = a; a = aie__align(a + E * n * p->n_host_a * 4, 256); }
  if (p->n_host_p) { p->a_host_act_p = a; a = aie__align(a + E * p->n_host_p * 4, 256); }
  p->arena_bytes = a;

  /* ---- tensor table ------------------------------------------------------------ */
  if (tt) {
    const int64_t rs = p->rec_bytes, r0 = p->a_records;
#define REC(name, dt, off, nd, d0, d1, d2) aie__add(tt, name, dt, r0 + (off), rs, nd, d0, d1, d2, 0, E)
    REC("cells", AIE_U32, p->o_cells, 2, p->H, p->W, 0);
    /* byte-plane views into the packed cell words (element stride 4) */
    {
      static const char* nm[4] = {"stone", "wood", "house_owner", "cell_flags"};
      for (int b = 0; b < 4; ++b) {
        REC(nm[b], b == 2 ? AIE_I8 : AIE_U8, p->o_cells + b, 2, p->H, p->W, 0);
        aie_tensor_desc* d = &tt->t[tt->n - 1];
        d->stride[2] = 4;
        d->stride[1] = 4 * (int64_t)p->W;
      }
    }
    if (p->regen_conv) REC("regen_source_count", AIE_U8, p->o_regen_count, 3, R, p->H, p->W);
    REC("loc_r", AIE_I32, p->o_loc_r, 1, n, 0, 0);
    REC("loc_c", AIE_I32, p->o_loc_c, 1, n, 0, 0);
    REC("inv_res", AIE_I32, p->o_inv_res, 2, R, n, 0);
    REC("esc_res", AIE_I32, p->o_esc_res, 2, R, n, 0);
    REC("inv_coin", AIE_F64, p->o_inv_coin, 1, n, 0, 0);
    REC("esc_coin", AIE_F64, p->o_esc_coin, 1, n, 0, 0);
    REC("labor", AIE_F64, p->o_labor, 1, n, 0, 0);
    REC("build_payment", AIE_F64, p->o_build_payment, 1, n, 0, 0);
    REC("build_skill", AIE_F64, p->o_build_skill, 1, n, 0, 0);
    REC("bonus_gather_prob", AIE_F64, p->o_bonus_gather_prob, 1, n, 0, 0);
    REC("util", AIE_F64, p->o_util, 1, n + 1, 0, 0);
    if (p->has_cda) {
      REC("cda_n_bids", AIE_I32, p->o_cda_n_bids, 1, R, 0, 0);
      REC("cda_n_asks", AIE_I32, p->o_cda_n_asks, 1, R, 0, 0);
      REC("cda_bids", AIE_I32, p->o_cda_bids, 2, R, p->M, 0);
      REC("cda_asks", AIE_I32, p->o_cda_asks, 2, R, p->M, 0);
      REC("cda_n_orders", AIE_I32, p->o_cda_n_orders, 2, R, n, 0);
      REC("cda_bid_hist", AIE_U8, p->o_cda_bid_hist, 3, R, n, p->P);
      REC("cda_ask_hist", AIE_U8, p->o_cda_ask_hist, 3, R, n, p->P);
      REC("cda_price_history", AIE_F64, p->o_cda_price_history, 3, R, n, p->P);
    }
    if (p->has_tax) {
      REC("tax_cycle_pos", AIE_I32, p->o_tax_cycle_pos, 0, 0, 0, 0);
    REC("tax_last_completions", AIE_I32, p->o_tax_last_completions, 0, 0, 0, 0);
      REC("tax_rate_idx", AIE_I32, p->o_tax_rate_idx, 1, p->NB, 0, 0);
      if (c->tax_model == AIE_TAX_SAEZ) {
        REC("tax_saez_bracket_rates", AIE_F64, p->o_tax_saez_rates, 1, p->NB, 0, 0);
        REC("tax_saez_observed_rates", AIE_F64, p->o_tax_saez_obs_rates, 1, p->NB, 0, 0);
      }
      REC("tax_last_coin", AIE_F64, p->o_tax_last_coin, 1, n, 0, 0);
      REC("tax_last_income", AIE_F64, p->o_tax_last_income, 1, n, 0, 0);
      REC("tax_last_marginal_rate", AIE_F64, p->o_tax_last_marginal_rate, 1, n, 0, 0);
      REC("tax_total_collected", AIE_F64, p->o_tax_total_collected, 0, 0, 0, 0);
    }
    REC("timestep", AIE_I32, p->o_timestep, 0, 0, 0, 0);
    REC("completions", AIE_I32, p->o_completions, 0, 0, 0, 0);
    REC("sample_t", AIE_I32, p->o_sample_t, 0, 0, 0, 0);
    REC("rew_log_slot", AIE_I32, p->o_rew_slot, 0, 0, 0, 0);
    REC("auto_warmup", AIE_I32, p->o_auto_warmup, 0, 0, 0, 0);
    REC("obs_valid", AIE_I32, p->o_obs_valid, 0, 0, 0, 0);
    REC("error_flags", AIE_I32, p->o_error_flags, 0, 0, 0, 0);
    if (p->o_src_list) {
      REC("regen_src_n", AIE_I32, p->o_src_n, 0, 0, 0, 0);
      REC("regen_src_list", AIE_I16, p->o_src_list, 1, AIE_SRC_CAP, 0, 0);
    }
    if (p->o_cells8) REC("cells_packed", AIE_U8, p->o_cells8, 2, p->H, p->W, 0);
    REC("mt", AIE_U32, p->o_mt, 1, aie__rng_state_words(&p->c), 0, 0);
    REC("mt_pos", AIE_I32, p->o_mt_pos, 0, 0, 0, 0);
    REC("mt_has_gauss", AIE_I32, p->o_mt_has_gauss, 0, 0, 0, 0);
    REC("mt_gauss", AIE_F64, p->o_mt_gauss, 0, 0, 0, 0);
#undef REC
#define DENSE(name, dt, off, nd, d0, d1, d2, d3)                                            \
  do {                                                                                      \
    int64_t dd[4] = {d0, d1, d2, d3};                                                       \
    int64_t es = aie__dtype_size(dt);                                                       \
    for (int q = 0; q < nd; ++q) es *= dd[q];                                               \
    aie__add(tt, name, dt, off, es, nd, d0, d1, d2, d3, E);                                 \
  } while (0)
    DENSE("obs_a_world-map", AIE_F32, p->a_obs_a_map, 4, n, p->am_ch, p->am_h, p->am_w);
    DENSE("obs_a_world-idx_map", AIE_I16, p->a_obs_a_idx, 4, n, 2, p->am_h, p->am_w);
    DENSE("obs_a_flat", AIE_F32, p->a_obs_a_flat, 2, n, p->FA, 0, 0);
    DENSE("obs_a_action_mask", AIE_F32, p->a_obs_a_mask, 2, n, p->MA, 0, 0);
    DENSE("obs_a_time", AIE_F32, p->a_obs_a_time, 2, n, 1, 0, 0);
    if (c->planner_gets_spatial_info) {
      DENSE("obs_p_world-map", AIE_F32, p->a_obs_p_map, 3, p->CM, p->H, p->W, 0);
      DENSE("obs_p_world-idx_map", AIE_I16, p->a_obs_p_idx, 3, 2, p->H, p->W, 0);
    }
    DENSE("obs_p_flat", AIE_F32, p->a_obs_p_flat, 1, p->FP, 0, 0, 0);
    DENSE("obs_p_action_mask", AIE_F32, p->a_obs_p_mask, 1, p->MP, 0, 0, 0);
    DENSE("obs_p_time", AIE_F32, p->a_obs_p_time, 1, 1, 0, 0, 0);
    if (p->FPA) DENSE("obs_p_agents", AIE_F32, p->a_obs_p_agents, 2, n, p->FPA, 0, 0);
    DENSE("rewards_a", AIE_F32, p->a_rew_a, 1, n, 0, 0, 0);
    DENSE("rewards_p", AIE_F32, p->a_rew_p, 0, 0, 0, 0, 0);
    DENSE("done", AIE_U8, p->a_done, 0, 0, 0, 0, 0);
    aie__add_metrics_tensors(p, tt);
    aie__add_event_tensors(p, tt);
    aie__add_saez_tensors(p, tt);
    if (c->layout_gen != AIE_LAYOUT_FIXED)
      aie__add_shared(tt, "layout_source_prob", AIE_F64, p->a_layout_prob, 2, AIE_N_RES, HW);
    if (aie__layout_staged(c)) aie__add_shared(tt, "layout_stage_ctl", AIE_I32, p->a_layout_ctl, 1, 4, 0);
    if (p->n_host_a) DENSE("host_actions_a", AIE_I32, p->a_host_act_a, 2, n, p->n_host_a, 0, 0);
    if (p->n_host_p) DENSE("host_actions_p", AIE_I32, p->a_host_act_p, 1, p->n_host_p, 0, 0, 0);
#undef DENSE
  }
  return AIE_OK;
}

#endif /* AIE_LAYOUT_BUILD_H_ */
