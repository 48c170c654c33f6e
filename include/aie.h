/*
 * aie.h -- C ABI of the MI355X-native batched Foundation env.step().
 *
 * One `aie_env` owns E independent replicas of one Foundation environment on one
 * GPU.  The reference has no such seam for gather-trade-build; the closest thing it
 * has is the WarpDrive wrapper used by the COVID scenario, and every entry point below
 * cites the reference interface it stands in for (paths relative to the reference
 * tree, F/ = ai_economist/foundation/):
 *
 *   aie_create            F/__init__.py:16-18 (make_env_instance) +
 *                         F/base/base_env.py:178-366 (BaseEnvironment.__init__) +
 *                         F/env_wrapper.py:96-265 (FoundationEnvWrapper.__init__)
 *   aie_seed              F/base/base_env.py:481-494 (BaseEnvironment.seed ->
 *                         np.random.seed), one legacy MT19937 stream PER replica
 *   aie_seed_fast         the same seam for environments created with rng_mode = AIE_RNG_FAST: a counter-based
 *                         stream (Philox2x32-10) per replica instead of NumPy's MT19937 -- a throughput mode the
 *                         reference does not have (its trainers only ever call np.random.seed, base_env.py:481-494);
 *                         NOT stream-compatible with NumPy
 *   aie_set_rng_state     F/base/base_env.py:871-881 / 968-978 (seed_state injection)
 *   aie_reset             F/base/base_env.py:852-927 (reset) +
 *                         F/env_wrapper.py:267-353 (reset_all_envs/reset_only_done_envs)
 *   aie_step              F/base/base_env.py:929-1032 (step) +
 *                         F/env_wrapper.py:355-377 (step_all_envs)
 *   aie_get_tensor        F/env_wrapper.py:297-326 (get_data_dictionary /
 *                         get_tensor_dictionary -> CUDADataManager.push_data_to_device,
 *                         torch_accessible=True)
 *   aie_upload/_download  F/env_wrapper.py:291-329 (one-time host -> device push)
 *
 * Conventions: every function returns 0 on success or a negative AIE_E_* code;
 * aie_last_error() gives the message.  The library owns all state / observation /
 * reward buffers (one arena, optionally caller-provided so that it can be a
 * torch-owned allocation); the caller owns action buffers.  All kernels are enqueued
 * asynchronously on the caller's HIP stream; there are no hidden synchronisations
 * except in aie_upload/aie_download/aie_destroy.  Calls on one handle are not
 * thread-safe; distinct handles are independent.  No process-global RNG.
 */
#ifndef AIE_H_
#define AIE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the functions declared in this header are exported
 * (tests/test_cabi_symbols.py compares `nm -D` with this file). */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define AIE_ABI_VERSION 11

#define AIE_MAX_AGENTS 64      /* mobile agents per replica, spatial scenarios (one lane each) */
#define AIE_MAX_AGENTS_WIDE 128 /* mobile agents per replica, map-less one-step-economy        */
#define AIE_MAX_COMPONENTS 8
#define AIE_MAX_BRACKETS 16
#define AIE_MAX_RATES 64       /* discretised tax rates per bracket                     */
#define AIE_MAX_SUBSPACES 16   /* action subspaces per agent class                      */
#define AIE_MAX_HOST_SUBSPACES 8 /* of them: subspaces of host components per agent class (aie_config.host_*) */
#define AIE_N_RES 2            /* collectible resources, sorted: 0 = Stone, 1 = Wood    */
#define AIE_MT_N 624
/* aie_config.rng_mode: which generator feeds the replicas' np.random.* draws (agent orders, pick-up bonus, resource
 * regeneration, reset placement / skills / layouts).
 *   AIE_RNG_NUMPY  NumPy's legacy MT19937 stream per replica, bit for bit (the parity mode; the default).
 *   AIE_RNG_FAST   a counter-based stream per replica: 32-bit word number g of replica e is element g & 1 of
 *                  Philox2x32-10(counter = (lo32(g >> 1), hi32(g >> 1) | salt), key = key32) with
 *                  key32 = lo32(seed + e_global) and salt = (bits 32..47 of seed + e_global) << 16 (Salmon et al.,
 *                  "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants).  Every consumer of
 *                  the stream (53-bit doubles from two words, masked-rejection integers, Fisher-Yates permutations,
 *                  polar Gauss) is unchanged, so a run differs from the parity mode ONLY in the words drawn.  The
 *                  record carries 16 bytes of generator state instead of 2 496, and a step computes only the words it
 *                  uses (the resource regeneration addresses the words of its source cells directly instead of
 *                  advancing MT19937 through all 4 H W of them).  Checked bit for bit against oracle/'s restatement of
 *                  the same generator; not stream-compatible with NumPy.  COVID draws no random numbers: ignored there.
 *                  Scenarios that draw a new source layout at every reset (uniform/, quadrant/, multi_zone/) take the
 *                  layout of a replica's k-th reset (k = 0, 1, ... since seeding) from a stream of its own -- the same
 *                  function with key32 + 0x9E3779B9 (k >> 15) and the counter's high word salt | 0x8000 | (k & 0x7fff),
 *                  from its word 0 -- so the layout does not depend on what the episode's steps drew, and the library
 *                  draws layouts AHEAD of their resets (one refill launch behind a reset once a quarter of the
 *                  replicas have used theirs up; a reset whose layout is not there yet draws it itself: same result).
 * The position bookkeeping is shared: the stream is consumed in blocks of AIE_MT_N words ("mt_pos" counts inside the
 * block, 624 = block exhausted); in fast mode tensor "mt" is uint32 [E, 4] = key32, block number, salt, resets so far. */
#define AIE_RNG_NUMPY 0
#define AIE_RNG_FAST 1
#define AIE_COVID_MAX_FILTERS 8 /* unemployment filter bank size (covid19_env.py:242)    */

/* ---- error codes ---------------------------------------------------------------- */
#define AIE_OK 0
#define AIE_E_INVALID (-1)     /* bad argument / config (reference: assert/ValueError)  */
#define AIE_E_NOTFOUND (-2)    /* unknown tensor name (reference: KeyError)             */
#define AIE_E_HIP (-3)         /* HIP runtime error                                     */
#define AIE_E_NOMEM (-4)
#define AIE_E_UNSUPPORTED (-5)

/* Per-replica `error_flags` tensor (int32 [E]): conditions on which the reference RAISES from inside step() / reset()
 * while a batched launch cannot (it carries on as documented and leaves the evidence here; sticky until the replica is
 * reset).  The host mirror's env.check_errors() turns them into the reference's exceptions. */
#define AIE_ERR_AGENT_ACTION 1    /* an agent's action index outside its action space: treated as NO-OP (reference:
                                     ValueError, F/components/move.py:133-134, build.py:158-159; TypeError from
                                     base_agent.py:407-438 in single-action mode)                                   */
#define AIE_ERR_PLANNER_ACTION 2  /* likewise for the planner (redistribution.py:953-960)                             */
#define AIE_ERR_RESET_PLACEMENT 4 /* reset could not find a free tile for an agent in 200 tries (reference: TimeoutError,
                                     layout_from_file.py:366-368); the agent was put on the last tile tried           */

/* ---- component ids (registry names in the reference, F/components/*.py) -------- */
enum {
  AIE_COMP_BUILD = 1,          /* "Build"                     F/components/build.py:15        */
  AIE_COMP_CDA = 2,            /* "ContinuousDoubleAuction"   F/components/continuous_double_auction.py:16 */
  AIE_COMP_GATHER = 3,         /* "Gather"                    F/components/move.py:16         */
  AIE_COMP_TAX = 4,            /* "PeriodicBracketTax"        F/components/redistribution.py:78 */
  AIE_COMP_SIMPLE_LABOR = 5,   /* "SimpleLabor"               F/components/simple_labor.py:15  */
  AIE_COMP_COVID_CONTROL = 6,  /* "ControlUSStateOpenCloseStatus" F/components/covid19_components.py:32  */
  AIE_COMP_COVID_SUBSIDY = 7,  /* "FederalGovernmentSubsidy"      F/components/covid19_components.py:244 */
  AIE_COMP_COVID_VACCINE = 8,  /* "VaccinationCampaign"           F/components/covid19_components.py:472 */
  AIE_COMP_WEALTH_REDISTRIBUTION = 9 /* "WealthRedistribution"     F/components/redistribution.py:21-75 */
};

/* ---- scenario families (registry names in the reference, F/scenarios) ----------- */
enum {
  AIE_SCN_GTB = 0,             /* "layout_from_file/simple_wood_and_stone" (+ uniform: next)   */
  AIE_SCN_ONE_STEP_ECONOMY = 1,/* "one-step-economy"  F/scenarios/one_step_economy/one_step_economy.py:15 */
  AIE_SCN_COVID = 2            /* "CovidAndEconomySimulation"  F/scenarios/covid19/covid19_env.py:33 */
};
enum { AIE_AGENT_REW_COIN_MINUS_LABOR_COST = 0, AIE_AGENT_REW_ISOELASTIC = 1 };

enum { AIE_SKILL_NONE = 0, AIE_SKILL_PARETO = 1, AIE_SKILL_LOGNORMAL = 2 };
enum {
  AIE_TAX_MODEL_WRAPPER = 0,   /* "model_wrapper": planner actions pick the rates       */
  AIE_TAX_US_FEDERAL = 1,      /* "us-federal-single-filer-2018-scaled"                 */
  AIE_TAX_FIXED = 2,           /* "fixed-bracket-rates"                                 */
  AIE_TAX_SAEZ = 3             /* "saez": rates from the Saez formula on a buffer of observed
                                  (income, marginal rate) pairs, redistribution.py:436-823 */
};
#define AIE_SAEZ_BINS 100      /* _saez_n_estimation_bins, redistribution.py:284         */
enum { AIE_WARMUP_DECAY = 0, AIE_WARMUP_AUTO = 1 };
enum {
  AIE_PLANNER_REW_COIN_EQ_TIMES_PROD = 0,
  AIE_PLANNER_REW_INV_INCOME_COIN = 1,
  AIE_PLANNER_REW_INV_INCOME_UTIL = 2
};

enum {
  AIE_U8 = 0, AIE_I8 = 1, AIE_I16 = 2, AIE_I32 = 3, AIE_U32 = 4, AIE_F32 = 5, AIE_F64 = 6
};

/* ---- COVID-19 scenario: the scalar constants CovidAndEconomyEnvironment.__init__ derives
 * (covid19_env.py:68-330) + the kwargs of its three components.  Per-state constants and
 * tables are named tensors ("model_*", leading dim 1) filled with aie_upload after
 * aie_create -- the counterpart of the reference's get_data_dictionary() push
 * (covid19_env.py:436-560, covid19_components.py:110-143,330-359,560-591).  Floating-point
 * constants the reference holds as float32 are passed as doubles holding the float32 value. */
typedef struct aie_covid_config {
  int32_t num_stringency_levels;          /* model_constants NUM_STRINGENCY_LEVELS (10)        */
  int32_t beta_delay;                     /* fitted BETA_DELAY (days)                          */
  int32_t filter_len;                     /* fitted FILTER_LEN (600)                           */
  int32_t num_filters;                    /* len(CONV_LAMBDAS) <= AIE_COVID_MAX_FILTERS        */
  int32_t action_cooldown_period;         /* ControlUSStateOpenCloseStatus kwarg               */
  int32_t subsidy_interval;               /* FederalGovernmentSubsidy kwargs                   */
  int32_t num_subsidy_levels;
  int32_t delivery_interval;              /* VaccinationCampaign kwarg                         */
  int32_t time_when_vaccine_delivery_begins; /* days from start_date to vaccine_delivery_start_date */
  int32_t filter_recurrence;              /* 1: the unemployment filters are exp(-age / lambda_f) (covid19_env.py:242-247)
                                             and filter_decay[] holds exp(-1 / lambda_f): the step updates each
                                             filter's discounted delta sum in O(1) (A_t = r (A_{t-1} - r^{L-1} d_old)
                                             + d_new) instead of re-summing the filter_len-day window; 0: direct sum
                                             over the uploaded taps (any filter shape)                              */
  double death_rate, gamma;               /* SIR_MORTALITY, SIR_GAMMA                          */
  double value_of_life;
  double daily_production_per_worker;
  double infection_too_sick_to_work_rate;
  double population_between_age_18_65;
  double risk_free_interest_rate;
  double economic_reward_crra_eta;
  double planner_health_norm, planner_economic_norm;
  double min_marginal_planner_health_index, max_marginal_planner_health_index;
  double min_marginal_planner_economic_index, max_marginal_planner_economic_index;
  double weightage_on_marginal_planner_health_index, weightage_on_marginal_planner_economic_index;
  double reward_normalization_factor;
  double filter_decay[AIE_COVID_MAX_FILTERS]; /* r_f = exp(-1 / CONV_LAMBDAS[f]), used iff filter_recurrence      */
  double filter_tail[AIE_COVID_MAX_FILTERS];  /* r_f^(filter_len - 1): the weight with which a delta leaves the window */
  int32_t replay_policies;                /* use_real_world_policies (covid19_env.py:56-60, covid19_components.py:181-186,
                                             394-425): actions are ignored; the states' stringency actions come from tensor
                                             "replay_stringency_policy" [episode_length][n] (row t-1 acts at step t), the
                                             planner's subsidy level of every step from "replay_subsidy_level"
                                             [episode_length]; every action mask is fully open                       */
  int32_t replay_data;                    /* use_real_world_data (covid19_env.py:52-55, 734-757, 815-818; implies
                                             replay_policies): susceptible / infected / recovered / vaccinated / deaths /
                                             unemployed of day t are read from tensor "replay_state" (float64 [6][episode_length + 1][n],
                                             clamped at 0) instead of being simulated                                 */
} aie_covid_config;

/* ---- configuration: the kwargs of make_env_instance + component kwargs ---------- */
typedef struct aie_config {
  int32_t abi_version;
  int32_t n_envs;                    /* E replicas on this device                      */
  int32_t n_agents;                  /* base_env.py:221-224 (>= 2)                      */
  int32_t world_h, world_w;          /* base_env.py:215-219                             */
  int32_t episode_length;            /* base_env.py:253                                 */
  int32_t multi_action_mode_agents;  /* base_env.py:258                                 */
  int32_t multi_action_mode_planner; /* base_env.py:259                                 */
  int32_t allow_observation_scaling; /* base_env.py:262 -> inv_scale 0.01 / time scale  */
  int32_t n_components;
  int32_t components[AIE_MAX_COMPONENTS]; /* AIE_COMP_*, in config order (=dynamics order) */

  /* scenario: layout_from_file / uniform simple_wood_and_stone
   * (F/scenarios/simple_wood_and_stone/layout_from_file.py:68-167) */
  int32_t has_water;                 /* "Water" landmark registered (LayoutFromFile)    */
  int32_t shared_layout;             /* 1: source/water planes identical in all replicas */
  int32_t planner_gets_spatial_info;
  int32_t full_observability;
  int32_t obs_range;                 /* mobile_agent_observation_range                  */
  int32_t fixed_four_skill_and_loc;
  int32_t reset_random_order;        /* agents are placed in a random order at reset
                                      * (uniform/..., dynamic_layout.py:420-431)        */
  int32_t energy_warmup_method;
  int32_t planner_reward_type;
  int32_t regen_halfwidth[AIE_N_RES];/* 0..3 (dynamic_layout.py:150-153); > 0 needs max_health == 1 */
  int32_t max_health[AIE_N_RES];
  double regen_weight[AIE_N_RES];
  double starting_agent_coin;
  double isoelastic_eta;
  double energy_cost;
  double energy_warmup_constant;
  double mixing_weight_gini_vs_coin;
  int32_t ranked_locs[AIE_MAX_AGENTS][2]; /* fixed_four_skill_and_loc, :196-247         */
  double avg_ranked_skill[AIE_MAX_AGENTS];/* already multiplied by Build.payment, :192  */

  /* Build (F/components/build.py:41-68) */
  int32_t build_payment;
  int32_t build_payment_max_skill_multiplier;
  int32_t build_skill_dist;
  double build_labor;

  /* Gather (F/components/move.py:41-64) */
  int32_t gather_skill_dist;
  double move_labor, collect_labor;

  /* ContinuousDoubleAuction (continuous_double_auction.py:42-77) */
  int32_t cda_max_bid_ask;
  int32_t cda_order_duration;
  int32_t cda_max_num_orders;
  double cda_order_labor;

  /* PeriodicBracketTax (redistribution.py:137-346) */
  int32_t tax_disable;
  int32_t tax_model;
  int32_t tax_period;
  int32_t tax_n_brackets;
  int32_t tax_n_disc_rates;
  double tax_bracket_cutoffs[AIE_MAX_BRACKETS];
  double tax_disc_rates[AIE_MAX_RATES];       /* np.arange(rate_min, rate_max+disc, disc) */
  double tax_fixed_rates[AIE_MAX_BRACKETS];   /* us-federal / fixed models, <= rate_max  */

  /* scenario family + one-step-economy (one_step_economy.py:55-78) */
  int32_t scenario;                  /* AIE_SCN_*                                       */
  int32_t ose_agent_reward_type;     /* AIE_AGENT_REW_*                                 */
  double ose_labor_exponent;
  double ose_labor_cost;

  /* SimpleLabor (F/components/simple_labor.py:41-74) */
  int32_t labor_mask_first_step;
  int32_t labor_num_hours;           /* 100; 1 .. 255 (an agent's mask row, [NO-OP, hours...], is at most 256 entries) */
  double labor_pmsm;                 /* payment_max_skill_multiplier                    */
  double labor_skills[AIE_MAX_AGENTS_WIDE]; /* per-agent skill (sorted Pareto means, :66-74) */

  aie_covid_config covid;            /* scenario == AIE_SCN_COVID only                  */

  /* "split_layout/simple_wood_and_stone" (layout_from_file.py:653-800): a water row; at reset the
   * agents get the ranked build skills (avg_ranked_skill[], highest first) in a random order and
   * are placed above the water row if their skill rank is listed, else below it. */
  int32_t split_water_line;          /* 0: not a split layout; else 0 < row < world_h - 1 */
  uint32_t split_top_ranks[2];       /* bit k: skill rank k starts in the top part        */
  int32_t rng_mode;                  /* AIE_RNG_NUMPY (0, parity with the reference) or AIE_RNG_FAST              */

  /* PeriodicBracketTax tax_annealing_schedule=[warmup, slope] (redistribution.py:311-330,
   * utils.py:10-118): the highest allowed rate grows with the number of completed episodes */
  int32_t tax_annealing;             /* 1: schedule given                                 */
  /* dense logs (base_env.py:984-1016, component get_dense_log): replicas [0, dense_log_replicas)
   * record the component events of the current step (AIE_EV_*) in the tensors
   * "log_event_count" / "log_events"; 0 = off. */
  int32_t dense_log_replicas;
  double tax_annealing_warmup, tax_annealing_slope;
  double tax_rate_max;               /* rate_max kwarg (0 when taxes are disabled)        */

  /* tax_model="saez" (redistribution.py:262-296) */
  double tax_rate_min;               /* rate_min kwarg (0 when taxes are disabled)        */
  int32_t saez_buffer_size;          /* _buffer_size: samples before the formula is used (500) */
  int32_t saez_pareto_weight_uniform;/* pareto_weight_type: 0 "inverse_income", 1 "uniform" */
  int32_t saez_fixed_elas_given;     /* saez_fixed_elas is not None                        */
  int32_t saez_global_capacity;      /* > 0: room (pairs) for the cross-replica sample buffer of the reference's trainer
                                      * (set_global_saez_buffer, redistribution.py:530-533); 0: feature off        */
  double saez_fixed_elas;

  /* Source layouts drawn at every reset, on the device, from the replica's own stream ("uniform/", "quadrant/",
   * "multi_zone/simple_wood_and_stone": Uniform.reset_starting_layout, dynamic_layout.py:313-392; MultiZone
   * :778-872; Quadrant :992-1024).  Index 0 = Stone, 1 = Wood as everywhere else. */
  int32_t layout_gen;                /* AIE_LAYOUT_FIXED (planes from aie_set_layout), _UNIFORM, _QUADRANT, _MULTI_ZONE */
  int32_t layout_checker;            /* checker_source_blocks                                                        */
  double layout_coverage[AIE_N_RES]; /* layout_specs[r]["starting_coverage"] (already doubled under checker)           */
  double layout_clump[AIE_N_RES];    /* 1 - clip(clumpiness, 0, 0.99)                                                */
  int32_t mz_rows, mz_cols;          /* multi_zone: num_partitions_row / _col                                        */
  int32_t mz_zones[3];               /* multi_zone: number of Wood, Stone, Wood+Stone zones                          */
  int32_t layout_pad_;

  /* Action subspaces of HOST components (ABI 11; foundation.ActingComponent): a component of the user's that runs as
   * host code between two aie_step_range launches may own action subspaces the way the reference's components do
   * (get_n_actions, F/base/base_component.py:159-176; F/base/base_agent.py:97-180 lays the subspaces of every listed
   * component out in registration order).  The library knows nothing of such a component but where its subspaces sit:
   * subspace k of the mobile agents has host_a_dim[k] >= 1 choices (NO-OP not counted) and host_a_before[k] of the
   * built-in `components` are listed ahead of it (0 .. n_components, non-decreasing in k; equal values keep the order
   * of k); host_p_* likewise for the planner.  All zero: the layout of ABI 10.  Such subspaces take their single-action
   * indices, multi-action columns and flattened-mask entries in that order; the step kernel decodes their sub-actions
   * (0 = NO-OP, 1 .. dim = the choice; out of range: AIE_ERR_*_ACTION and NO-OP) into the tensors
   *   host_actions_a  int32 [E, n_agents, host_a_n]      host_actions_p  int32 [E, host_p_n]
   * (present when the count is > 0; plain arena regions, outside the replicas' records) in the step's first launch
   * (AIE_STEP_HEAD) and writes 1.0 into their mask entries whenever it rewrites a mask row; the host overwrites those
   * entries with the component's own masks (generate_masks, F/base/base_component.py:262-290) behind every launch that
   * writes observations.  Gather-trade-build scenarios; such an environment always runs the full-featured kernel.
   * Samplers: the agents' rows follow the layout in both action modes, and so does a single-action planner's one row.
   * A multi-action planner's rows must be equally long for the samplers (aie_sample_random_actions,
   * aie_sample_masked_actions, aie_sample_policy_actions): with a foreign planner subspace whose dimension differs from
   * the tax rows' (or from another foreign one's) they return AIE_E_UNSUPPORTED and aie_last_error says so. */
  int32_t host_a_n, host_p_n;
  int32_t host_a_dim[AIE_MAX_HOST_SUBSPACES], host_a_before[AIE_MAX_HOST_SUBSPACES];
  int32_t host_p_dim[AIE_MAX_HOST_SUBSPACES], host_p_before[AIE_MAX_HOST_SUBSPACES];
} aie_config;
#define AIE_LAYOUT_FIXED 0
#define AIE_LAYOUT_UNIFORM 1
#define AIE_LAYOUT_QUADRANT 2
#define AIE_LAYOUT_MULTI_ZONE 3

/* ---- dense-log events: one row of "log_events" int32 [L, cap, AIE_EV_WORDS] ------- */
#define AIE_EV_WORDS 12 /* [0] type, [1..8] integers, [10..11] one float64 (bit pattern)          */
enum aie_event {
  AIE_EV_BUILD = 1,  /* builder, row, col; f64 income              build.py:149-155                */
  AIE_EV_TRADE = 2,  /* commodity (0 Stone, 1 Wood), seller, buyer, ask, bid, price, ask_lifetime,
                        bid_lifetime                               continuous_double_auction.py:289-305 */
  AIE_EV_GATHER = 3, /* agent, resource (0 Stone, 1 Wood), n, row, col   move.py:141-149          */
  AIE_EV_TAX = 4,    /* agent; f64 tax_paid (income, marginal rate: tensors "tax_last_*")
                                                                  redistribution.py:878-883        */
  AIE_EV_TAX_BRACKET = 5 /* bracket; f64 marginal rate in force (the tax day's "schedule"; precedes
                        that day's AIE_EV_TAX rows)              redistribution.py:856-859        */
};

/* ---- tensor descriptor ---------------------------------------------------------- */
typedef struct aie_tensor_desc {
  char name[64];
  void* data;            /* device pointer of element [0,...,0] (NULL before aie_create)*/
  int32_t dtype;         /* AIE_U8 ...                                                  */
  int32_t ndim;          /* includes the leading env dimension                         */
  int64_t shape[6];
  int64_t stride[6];     /* in BYTES (state fields live in per-env records => strided)  */
  int64_t arena_offset;  /* byte offset of element [0,...] inside the arena             */
} aie_tensor_desc;

typedef struct aie_env aie_env;

/* Validates cfg and returns the arena size in bytes (> 0) or a negative error code. */
int64_t aie_arena_bytes(const aie_config* cfg);

/* Creates E replicas on HIP device `device`.  If `arena` is non-NULL it must be a
 * device allocation of at least aie_arena_bytes(cfg) bytes, 256-byte aligned, that
 * outlives the env (e.g. a torch uint8 tensor); otherwise the library allocates it: hipMalloc, or -- from
 * $AIE_ARENA_VMM_MIN_MB (default 1024) MiB on -- a virtual range backed by physical pieces of $AIE_ARENA_PIECE_MB
 * (default 64) MiB each (hipMemCreate / hipMemMap), on which the store-bound one-step-economy launch runs 14 % faster
 * than on one big allocation.  For a configuration outside every compile-time instance's family aie_create also starts
 * the run-time specialisation in the background (see aie_specialize; $AIE_JIT_AUTO=0 switches that off). */
int aie_create(const aie_config* cfg, int device, void* arena, int64_t arena_bytes,
               aie_env** out);
int aie_destroy(aie_env* env);
const char* aie_last_error(const aie_env* env /* NULL: last create error */);

/* Number of exported tensors and their descriptors (index or name lookup).  Names (aie_num_tensors /
 * aie_tensor_at enumerate what a configuration has; csrc/aie_layout_build.h is where they are defined):
 *   observations  obs_a_world-map, obs_a_world-idx_map, obs_a_flat, obs_a_action_mask, obs_a_time, obs_p_* (flat,
 *                 action_mask, time, world-map, world-idx_map, agents = the planner's per-agent p{i} fragments)
 *   outputs       rewards_a [E, n], rewards_p [E], done [E]
 *   state         cells (+ byte-plane views stone / wood / house_owner / cell_flags), loc_r/c, inv_res, esc_res,
 *                 inv_coin, esc_coin, labor, build_payment, build_skill, bonus_gather_prob, util, cda_* (books,
 *                 histograms, price history), tax_* (cycle position, rate indices, last coin / income / marginal
 *                 rate, total collected; tax_saez_bracket_rates / tax_saez_observed_rates), timestep, completions,
 *                 mt / mt_pos / mt_has_gauss / mt_gauss (the replica's NumPy-legacy generator), regen_source_count
 *   episode       metrics_cda_trades, metrics_tax_* (accumulators behind env.metrics)
 *   Saez          saez_buffer, saez_buffer_len, saez_reached_min_samples, saez_elas, saez_running_avg_tax_rates,
 *                 saez_next_rates
 *   dense log     log_event_count [L], log_events [L, cap, AIE_EV_WORDS]
 *   COVID         susceptible ... economic_index state rows, stringency_history_chunks, model_* constants
 *   host actions  host_actions_a [E, n, host_a_n], host_actions_p [E, host_p_n]: the decoded sub-actions of host
 *                 components' action subspaces (aie_config.host_*), written by the first launch of a step */
int aie_num_tensors(const aie_env* env);
int aie_tensor_at(const aie_env* env, int index, aie_tensor_desc* out);
int aie_get_tensor(const aie_env* env, const char* name, aie_tensor_desc* out);

/* Host <-> device copies of one named tensor (dense, C-order, leading dim = E).
 * Synchronous; meant for initial state injection and parity dumps.  The COVID tables "model_stringency_level_history_0"
 * and "model_unemp_conv_filters" have to be written through aie_upload (not through a view of the arena): the library
 * derives data from them at that point (the history-format image and the pre-episode change events every reset copies;
 * whether the taps are float32 values, which selects the tap-table format of the window-sum kernel).
 * Between steps the observation tensors belong to the kernels: aie_step updates maps, masks and flat vectors IN PLACE,
 * writing only what the step changed, while the record field obs_valid is 1.  aie_upload of any record field other
 * than obs_valid clears obs_valid for every replica (the next step rewrites all observations in full); code that edits
 * state through a view of the arena clears it itself (per replica), and so does code that overwrote an observation
 * tensor and wants it back. */
int aie_upload(aie_env* env, const char* name, const void* host, int64_t bytes);
int aie_download(aie_env* env, const char* name, void* host, int64_t bytes);

/* Source-block / water planes (HOST pointers, u8 [H*W] each; with shared_layout=1 one
 * replica's planes which are broadcast, else E of them).  They are packed into the
 * static flag byte of every map cell (layout_from_file.py:103-112, 323-334).  With shared_layout=1 (fixed layouts) the
 * call also derives the batch's one list of regeneration draws that target a source block (rng_mode AIE_RNG_FAST: the
 * step kernels read it instead of scanning the flag bytes every step): change such a layout through this call, not by
 * writing the `cell_flags` tensor. */
int aie_set_layout(aie_env* env, const uint8_t* stone_src, const uint8_t* wood_src,
                   const uint8_t* water);

/* Replica e gets the stream np.random.seed(base_seed + e) would give. */
int aie_seed(aie_env* env, uint32_t base_seed, void* stream);
/* rng_mode == AIE_RNG_FAST only (AIE_E_UNSUPPORTED otherwise): replica e gets the counter stream keyed by
 * seed + global_env_offset + e (48 bits are used); aie_seed(env, s, ...) is aie_seed_fast(env, s, 0, ...) there. */
int aie_seed_fast(aie_env* env, uint64_t seed, int64_t global_env_offset, void* stream);
/* Raw legacy-MT19937 state per replica: key[E][624], pos[E] (np.random.get_state()); rng_mode == AIE_RNG_FAST:
 * key[E][4] (key32, block number, salt, resets so far), pos[E]. */
int aie_set_rng_state(aie_env* env, const uint32_t* key, const int32_t* pos);

/* Resets the replicas whose env_mask byte is non-zero (NULL = all); env_mask is a
 * DEVICE pointer [E] u8 (e.g. the `done` tensor).  Writes reset observations. */
int aie_reset(aie_env* env, const uint8_t* d_env_mask, void* stream);

/* One env.step() for all replicas.  d_actions_a: device int32 [E, n_agents]
 * (single-action mode) or [E, n_agents, n_subspaces] (multi-action mode);
 * d_actions_p: device int32 [E, n_planner_subspaces] (multi-action planner) or [E].
 * Either may be NULL (= all NO-OP, base_env.py:964-966). */
int aie_step(aie_env* env, const int32_t* d_actions_a, const int32_t* d_actions_p,
             void* stream);

/* Fills caller-owned action buffers with the bench's synthetic uniform random policy:
 * counter RNG keyed (seed, global env id, t, agent) -- SURVEY.md section 8(d). */
int aie_sample_random_actions(aie_env* env, uint64_t seed, int64_t global_env_offset,
                              int32_t* d_actions_a, int32_t* d_actions_p, void* stream);

/* aie_step + aie_sample_random_actions for the NEXT step in one launch: steps with
 * d_actions_a/p and, while the replica's first wavefront runs the serial dynamics, lets the
 * otherwise idle second wavefront fill d_next_a/p (caller-owned, must differ from the current
 * action buffers) with exactly what aie_sample_random_actions would write next.  A rollout loop
 * of the uniform random policy then needs one launch per step instead of two. */
int aie_step_sample_next(aie_env* env, const int32_t* d_actions_a, const int32_t* d_actions_p, uint64_t seed,
                         int64_t global_env_offset, int32_t* d_next_a, int32_t* d_next_p, void* stream);

/* The same with the NEXT actions drawn as aie_sample_masked_actions would draw them from the masks this step writes
 * (a state's stringency levels only outside its cooldown, the planner's subsidy levels only on the first day of an
 * interval, NO-OP always): the random policy of a trainer that applies `action_mask` to its logits, one launch per
 * step.  COVID scenario; AIE_E_UNSUPPORTED elsewhere (there: aie_step, then aie_sample_masked_actions). */
int aie_step_sample_next_masked(aie_env* env, const int32_t* d_actions_a, const int32_t* d_actions_p, uint64_t seed,
                                int64_t global_env_offset, int32_t* d_next_a, int32_t* d_next_p, void* stream);

/* Part of a step, for components that live on the HOST (round 6: ai_economist_amd.foundation.BatchedComponent -- a user's
 * registered component whose component_step runs as torch code on the state tensors between two launches; the
 * reference's registries are open, F/base/base_component.py:378, F/base/registrar.py:48-66).  Runs the built-in components
 * [comp_lo, comp_hi) of aie_config.components, in order, and of the rest of a step what `phases` names:
 *   AIE_STEP_HEAD     timestep += 1 (base_env.py:981: before the first component of a step)
 *   AIE_STEP_TAIL     scenario_step (regeneration), observations, masks, rewards, done (+ auto-reset) -- the end of a step
 *   AIE_STEP_OBSERVE  observations and masks of the state as it stands, nothing else (after a host-side edit, e.g. a
 *                     component's additional_reset_steps); with AIE_STEP_REBASE also the utilities the next rewards are
 *                     measured from, as a reset leaves them (layout_from_file.py:347-349 runs behind the components' resets)
 * The end of a step in three parts, for scenario hooks that run INSIDE it (the reference's scenario_step,
 * generate_observations and compute_reward, F/base/base_env.py:1005-1011):
 *   AIE_STEP_REGEN    the built-in scenario_step: resource regeneration (the replica's generator advances and is stored).
 *                     May share a launch with HEAD and a component range; it runs behind that launch's components.
 *   AIE_STEP_EMIT     flat and spatial observations, action masks, and the built-in rewards into rewards_a / rewards_p
 *                     (utility baseline and auto-warmup integrator included).  No reward-log slot, no done, no completions.
 *   AIE_STEP_CLOSE    claims the reward-log slot and fills it from rewards_a / rewards_p AS THEY STAND in the arena (the host
 *                     may have edited them behind EMIT), writes done, completions and the slot's done flag (+ auto-reset).
 * REGEN, EMIT, CLOSE in one, two or three calls with no host edit in between leave every tensor bit-identical to TAIL;
 * EMIT | CLOSE in one call is TAIL without regeneration.  They exclude TAIL and OBSERVE; CLOSE takes no component range and
 * goes with REGEN or HEAD only when EMIT is set too; EMIT and CLOSE take an empty range unless REGEN rides along.
 * obs_valid: a call that changes state without EMIT clears it (the EMIT that follows rewrites maps and masks in full), EMIT
 * sets it, a CLOSE-only call leaves it alone.  The flat vectors are rewritten in full by EVERY aie_step_range call that
 * writes them; only a whole aie_step with obs_valid == 1 updates them (and the maps and masks) in place.
 * (phases == 0: components only, a stretch in the middle of a step.)
 * One step = any sequence of calls whose first carries HEAD, whose last carries TAIL (or CLOSE) and whose ranges tile the list;
 * aie_step(a, p) == aie_step_range(a, p, 0, n_components, HEAD | TAIL).  Every call takes the same action buffers.
 * Between two calls of a step the caller may edit state tensors; the TAIL call rewrites all observations.  Always the
 * full-featured kernel (no compile-time / run-time instance).  Gather-trade-build scenarios; AIE_E_UNSUPPORTED elsewhere,
 * with tax_model "saez" and while a dense-log replica records.
 * d_env_mask: the replicas the call touches (uint8 [n_envs], nonzero = yes), NULL = every replica -- the convention of
 * aie_reset.  The OBSERVE calls behind a masked aie_reset pass its mask: the replicas it did not reset keep their
 * observations, reward baseline and tax snapshot.  The calls of a step pass NULL. */
#define AIE_STEP_HEAD 1
#define AIE_STEP_TAIL 2
#define AIE_STEP_OBSERVE 4
#define AIE_STEP_REBASE 8
#define AIE_STEP_REGEN 64  /* (32 is taken: the library marks ranged launches with it) */
#define AIE_STEP_EMIT 128
#define AIE_STEP_CLOSE 256
#define AIE_STEP_RETAX 16 /* with OBSERVE: PeriodicBracketTax's reset-time snapshot of the agents' coin (redistribution.py:1106-1110) taken
                           * again -- a host component listed AHEAD of the tax component edited coin in its reset hook */
int aie_step_range(aie_env* env, const int32_t* d_actions_a, const int32_t* d_actions_p, int32_t comp_lo, int32_t comp_hi,
                   int32_t phases, void* stream, const uint8_t* d_env_mask);

/* Reward log for learners on another device: every following aie_step / aie_step_sample_next ALSO
 * writes replica e's (agent rewards [n_agents], planner reward, done as 0/1) as n_agents + 2 floats to
 * d_log[((slot * n_envs) + e) * (n_agents + 2) + ...], slot = 0, 1, ... n_slots - 1, 0, ... advancing by one per
 * step (this call resets it to 0).  The caller owns d_log (n_slots * n_envs * (n_agents + 2) floats) and ships
 * whole ranges of slots to the learner rank with one collective per many steps instead of one per step
 * (ai_economist_amd/sharding.py).  d_log == NULL switches the log off.  All scenarios.
 * The log's address, slot count and restart live in device memory, not in the step's kernel arguments: step launches
 * captured in a hipGraph BEFORE this call write to the log this call names when they are replayed after it, and a
 * replica that sits a launch out (COVID: stepped past its episode's end without a reset) still moves its slot with the
 * batch's.  The call waits for the device to go idle (call it between steps, not under stream capture). */
int aie_set_reward_log(aie_env* env, float* d_log, int32_t n_slots);

/* Auto-reset (the vectorised-trainer convention, reference analogue: F/env_wrapper.py:341-353 reset_only_done_envs):
 * with on != 0 a replica whose episode ends in a step restarts before the step call returns control of the stream --
 * its state and observations are those of the fresh episode, `done` and the rewards stay the terminal step's.
 * one-step-economy does it inside the step launch (the terminal observations, which nothing could read before they
 * are overwritten, are not written at all); the other scenarios enqueue their reset kernel, masked with `done`,
 * right behind the step (uniform/, quadrant/ and multi_zone/ layouts are drawn inside that reset kernel).
 * AIE_E_UNSUPPORTED only when the HOST supplies a new layout per episode (per-replica layouts passed to
 * aie_set_layout: worlds too large for the device-side generator).  Episode metrics of a finished episode are gone
 * once it restarts. */
int aie_set_auto_reset(aie_env* env, int on);

/* tax_model "saez": the cross-replica sample buffer (reference: PeriodicBracketTax.set_global_saez_buffer,
 * redistribution.py:515-533; filled by the trainer with the concatenation of every replica's local buffer,
 * tutorials/rllib/utils/remote.py:56-73).  d_pairs: n_pairs (income, marginal rate) float64 pairs in DEVICE memory
 * (n_pairs <= aie_config.saez_global_capacity); n_pairs == 0 clears it.  From then on every replica's period start
 * uses global + its own samples added since the buffers were last reset (`saez_additions` tensor), as the
 * reference's `saez_buffer` property does. */
int aie_set_global_saez_buffer(aie_env* env, const double* d_pairs, int64_t n_pairs);

/* Dense logs (aie_config.dense_log_replicas > 0; reference: F/base/base_env.py:273-283, 883-891 -- only every
 * `dense_log_frequency`-th episode is logged): with on == 0 the dense-log replicas stop recording AIE_EV_* rows and
 * step with the rest of the batch on the environment's fast kernel; with on != 0 (the default) they -- and only they
 * -- take the full-featured kernel.  State and observations are bit-identical either way; the host mirror switches
 * it per episode (foundation/base_env.py: reset).  Gather-trade-build only: the one-step-economy kernel records its
 * (few) events for the dense-log replicas regardless of this switch -- there is no separate full-featured kernel to
 * leave -- and COVID has no event rows. */
int aie_set_dense_log_active(aie_env* env, int on);

/* Where the arena lives: *bytes = its size, *allocator = AIE_ARENA_CALLER (passed to aie_create), AIE_ARENA_HIPMALLOC
 * (one hipMalloc) or AIE_ARENA_VMM (a virtual range backed by physical pieces of *piece_bytes each; see aie_create).
 * Any out pointer may be NULL.  (Launch times of the store-bound kernels depend on it: a measurement names it.) */
#define AIE_ARENA_CALLER 0
#define AIE_ARENA_HIPMALLOC 1
#define AIE_ARENA_VMM 2
int aie_arena_info(const aie_env* env, int64_t* bytes, int32_t* allocator, int64_t* piece_bytes);

/* sizeof(aie_config) as this library was built: a binding checks its mirror of the struct against it. */
int aie_sizeof_config(void);

/* Which step kernel runs this environment: 0 .. 999 = a compile-time instance (the code-shaping part of the
 * configuration's parameter block folded into the code, csrc/aie_spec_generated.h; an instance stands for the family of
 * configurations that differ in scalars only), AIE_KERNEL_INSTANCE_JIT = the run-time specialisation, -1 = the generic
 * kernel. */
int aie_step_kernel_instance(aie_env* env);

/* Chooses between the step kernels that can run this environment: AIE_KERNEL_AUTO (default) = the specialised
 * instance when one matches the configuration's family (compile-time) or once its run-time specialisation is ready,
 * AIE_KERNEL_GENERIC = pinned to the generic kernel that reads the parameter block at run time.  Both produce the same arena bit for bit (tests/test_gpu_parity.py steps them side by side); the
 * switch exists so that a user can check exactly that on their own configuration. */
#define AIE_KERNEL_AUTO 0
#define AIE_KERNEL_GENERIC 1
int aie_select_step_kernel(aie_env* env, int which);

/* Specialises the step and reset kernels on THIS environment's configuration family at run time, the way the build does
 * for the BASELINE configurations: the code-shaping part of the parameter block (component tuple, agent count, world
 * size, capacities, flags; NOT scalars such as starting coin, eta, episode length, labor costs, tax period / cutoffs,
 * which every specialised kernel reads at run time) becomes a compile-time constant of the kernels (hiprtc compiles
 * csrc/aie_kernels.hip and the aie_gtb_*.h it includes with it as a constant image, a few seconds once; the code object is cached under
 * $AIE_JIT_CACHE / ~/.cache/ai_economist_amd -- private directories only -- keyed by the image, the sources, the
 * architecture, the compiler version and options).  aie_create already starts this in the background and a later
 * aie_reset (an episode boundary, outside stream capture; never aie_step) adopts the result; this call WAITS for it.  Afterwards AIE_KERNEL_AUTO runs
 * the specialised kernels (aie_step_kernel_instance() == AIE_KERNEL_INSTANCE_JIT); results are bit-identical to the
 * generic kernel's.  Gather-trade-build and one-step-economy environments.  AIE_E_UNSUPPORTED -- and the environment simply keeps the
 * generic kernel -- when hiprtc, the kernel sources beside the library ($AIE_JIT_SOURCE_DIR) or the toolchain headers
 * are not there, or when the configuration needs the full-featured kernel (tax_model "saez", order books beyond a
 * wavefront, general regeneration; dense-log replicas do NOT: they take the full-featured kernel alone and only while an
 * episode is being logged, aie_set_dense_log_active). */
#define AIE_KERNEL_INSTANCE_JIT 1000
int aie_specialize(aie_env* env);

/* Categorical sampling from the CALLER's policy logits under the current action masks (the step a trainer
 * performs between two env steps -- the reference's trainers apply `action_mask` to the logits and sample,
 * base_env.py:141-145, tutorials/rllib/env_wrapper.py:50-211, training_script.py:88-133).
 *   d_logits_a  float32 [E, n, MA]  in the layout of obs_a_action_mask (single-action agents: one row of MA entries,
 *               entry 0 = NO-OP; multi-action: the subspaces' (1 + dim) entries back to back; COVID: [E, n, 1 + levels])
 *   d_logits_p  float32 [E, MP]     in the layout of obs_p_action_mask
 * Sub-action = a draw from softmax(logits) restricted to the mask by inverse CDF: weights exp(logit_k - max) of the allowed
 * entries, their prefix sums in a fixed order, the first entry whose sum passes u x total, u in (0, 1) from a counter hash
 * keyed (seed, global env id, the replica's draw index, slot); NaN logits count as masked, NO-OP if nothing is allowed.
 * Everything is float32 and a fixed sequence of IEEE add / multiply / fused multiply-add operations (csrc/aie_trainer_math.h:
 * aie_sampler_expf, aie_sampler_uniform, aie_sampler_entry_rng, the scan's order), so the CPU restatement (oracle/:
 * aie_oracle_sample_policy_actions) picks the same entries; a probability is resolved to 2^-24 of its row's total and u
 * has 23 bits.  Rows of up to 64 entries with single-action agents (every BASELINE configuration, COVID) run on
 * instances with compile-time row shapes, anything else on a generic kernel with the same results.  One launch; the
 * draw index is the replica's record field `sample_t`, advanced by the kernel (replayable from a hipGraph).  Either pair
 * (logits, actions) may be NULL. */
int aie_sample_policy_actions(aie_env* env, const float* d_logits_a, const float* d_logits_p, uint64_t seed,
                              int64_t global_env_offset, int32_t* d_actions_a, int32_t* d_actions_p, void* stream);

/* aie_sample_policy_actions that also returns log pi(a|s) of every pick: the same picks and the same advance of
 * `sample_t`, bit for bit (the same kernels with one more store per action slot), one launch, replayable from a hipGraph.
 *   d_logp_a  float32 [E, n, width_a]   d_logp_p  float32 [E, width_p]   (the action buffers' shapes)
 * logp = y_a - log T (aie_sampler_logf) with the sampler's own y = logit - max, weights and total T (csrc/aie_trainer_math.h: a
 * fixed sequence of float32 operations, no libm; the CPU twin aie_policy_row_logp gives the same bits); 0 for a slot
 * where nothing is allowed (the pick there is NO-OP).  Either actor class (logits, actions, logp) may be NULL. */
int aie_sample_policy_actions_logp(aie_env* env, const float* d_logits_a, const float* d_logits_p, uint64_t seed,
                                   int64_t global_env_offset, int32_t* d_actions_a, int32_t* d_actions_p, float* d_logp_a,
                                   float* d_logp_p, void* stream);

/* Learning-time evaluation of STORED actions under STORED masks for new logits: what a policy-gradient trainer (PPO,
 * A2C: training_script.py:88-133 builds one on masked logits) needs of the categorical distribution, in the sampler's own
 * arithmetic -- evaluating the logits an action was sampled from under the masks it was sampled under returns the logp
 * aie_sample_policy_actions_logp returned, bit for bit (importance ratio exactly 1).
 *   B batch elements (replica-steps), any B >= 1, not tied to the environment's E;
 *   d_logits_a [B, n, MA] / d_logits_p [B, MP]: aie_sample_policy_actions' layouts with B for E;
 *   d_masks_a / d_masks_p: contiguous float32 in the LOGITS' layout (> 0.5 = allowed; COVID: [B, n, 1 + levels], not the
 *       arena's collated rows); NULL = the arena's current masks, B == E only;
 *   d_actions_a int32 [B, n, width_a] / d_actions_p int32 [B, width_p]: the stored sub-actions;
 *   d_logp_* / d_entropy_*: float32, the actions' shapes: log pi of the stored sub-action and the entropy H of its slot.
 * Per slot (csrc/aie_trainer_math.h states every operation): allowed = mask > 0.5 and logit not NaN; logp_k = y_k - log T;
 * H = log T - S / T, S = sum of w_k y_k in the scan's order.  A slot where nothing is allowed: logp 0, H 0.  A stored
 * action its mask does not allow (or outside the row): logp -INFINITY.  An allowed entry 80 or more below the maximum has
 * weight 0 and a finite logp.  Either actor class may be NULL, and so may any output.  One launch, asynchronous on
 * `stream`, no synchronisation; aie_sample_policy_actions' refusals (AIE_E_UNSUPPORTED) apply. */
int aie_policy_evaluate(aie_env* env, int64_t B, const float* d_logits_a, const float* d_logits_p, const float* d_masks_a,
                        const float* d_masks_p, const int32_t* d_actions_a, const int32_t* d_actions_p, float* d_logp_a,
                        float* d_logp_p, float* d_entropy_a, float* d_entropy_p, void* stream);

/* Its backward: d_grad_logits_* (the logits' shapes) = the gradient of sum(d_glogp * logp + d_gentropy * H) with respect
 * to the logits,  g_k = g_logp ([k = a] - p_k) - g_H p_k (logp_k + H)  for allowed entries (p_k = w_k / T; the operation
 * order is in csrc/aie_trainer_math.h) and exactly 0 for the others; every entry of the buffers is written.  M, T and S are
 * recomputed (nothing is kept from the forward).  A slot where nothing is allowed has a zero gradient row; the g_logp of
 * a stored action its mask does not allow contributes nothing.  d_glogp_* / d_gentropy_* may be NULL (= zeros), either
 * actor class may be NULL.  One launch, asynchronous on `stream`. */
int aie_policy_evaluate_backward(aie_env* env, int64_t B, const float* d_logits_a, const float* d_logits_p,
                                 const float* d_masks_a, const float* d_masks_p, const int32_t* d_actions_a,
                                 const int32_t* d_actions_p, const float* d_glogp_a, const float* d_glogp_p,
                                 const float* d_gentropy_a, const float* d_gentropy_p, float* d_grad_logits_a,
                                 float* d_grad_logits_p, void* stream);

/* Generalised advantage estimation straight from a reward log: advantages and returns of T steps for every (replica, actor)
 * column, one launch -- what PPO with use_gae does between a rollout and its update (the reference's training configurations:
 * gamma 0.998, lambda 0.98, fragments of 200 steps), where torch takes ~6 elementwise launches per step of the fragment.
 *   d_log      float32 [n_slots][E][n + 2] in aie_set_reward_log's layout (agents' rewards, the planner's reward, done as
 *              0/1); it need not be the log currently installed.  Time t (0 <= t < T <= n_slots) lives in ring slot
 *              (first_slot + t) % n_slots;
 *   d_values_a float32 [T + 1][E][n], d_values_p float32 [T + 1][E]: row T is the bootstrap value of the observation behind
 *              the last step;
 *   d_adv_* / d_ret_*: the values' shapes with T rows.
 * float32, every product and sum rounded on its own (no fma), a fixed order (csrc/aie_trainer_math.h states it once; the CPU test
 * compiles the same helper): with gl = gamma * lambda rounded once and done_t = log[t][e][n + 1] > 0.5,
 *   delta_t = done_t ? r_t - V_t : (r_t + gamma V_{t+1}) - V_t,   A_t = done_t ? delta_t : delta_t + gl A_{t+1}  (A_T = 0),
 *   ret_t = A_t + V_t
 * -- the bits of the plain serial float32 loop; the recurrence is not re-associated across time.  A done step SELECTS (it
 * does not multiply by zero): under auto-reset V_{t+1} and A_{t+1} behind an episode's end belong to the restarted episode
 * and do not enter the arithmetic, so a NaN or an infinity there does not leak.
 * Either actor class may be NULL (values and outputs), either d_ret_* may be NULL, and d_adv_* may be NULL when its d_ret_*
 * is not; a class with no output is left out.  All scenarios (E and n are the environment's).  One launch, asynchronous on
 * `stream`, no synchronisation, capturable.  AIE_E_INVALID for T < 1, T > n_slots, first_slot outside the ring, a NULL log
 * or an output without its values. */
int aie_gae(aie_env* env, int32_t T, const float* d_log, int32_t n_slots, int32_t first_slot, const float* d_values_a,
            const float* d_values_p, float gamma, float lambda, float* d_adv_a, float* d_adv_p, float* d_ret_a, float* d_ret_p,
            void* stream);

/* The PPO loss of both actor classes with its gradients, two launches: the clipped surrogate over the JOINT log-probability
 * of an actor's action slots, the clipped value loss and the entropy bonus (the loss RLlib's PPO is configured with in the
 * reference's tutorials: clip_param 0.3, vf_clip_param 50, vf_loss_coeff 0.05, entropy_coeff 0.025; vf_clip = 0 is the plain
 * squared error), forward and backward together -- what a trainer otherwise writes as several dozen elementwise torch
 * launches with their autograd twins around aie_policy_evaluate and its backward.
 *   B batch elements, any B >= 1, not tied to the environment's E.  An ACTOR is one agent, or the planner, of one batch
 *   element; it has width_a / width_p action slots whose rows are aie_policy_evaluate's.  Per class (aie_ppo_class):
 *   logits [B, n, MA] / [B, MP], values [B, n] / [B] (NULL: no value term): the network's outputs for batch element b;
 *   the STORED operands -- masks (the logits' layout), actions and logp_old (int32 / float32 [R, n, width_a] /
 *   [R, width_p]), adv, values_old, returns (float32 [R, n] / [R]) -- are read at row d_index[b] of tensors of R rows
 *   (a whole fragment, say), or at row b with d_index NULL: a minibatch is an index, not a copy.  d_index: int32 [B] in
 *   device memory; a row outside the stored tensors is the caller's error, like a bad pointer;
 *   adv_moments: NULL, or {mean, rstd} in DEVICE memory: the advantage enters as (A - mean) * rstd;
 *   grad_logits (the logits' shape), grad_values ([B, n] / [B]; NULL exactly when values is): the gradient of stats[0]
 *   with respect to the logits and the values, every entry written (exactly 0 at entries the mask does not allow);
 *   stats: AIE_PPO_N_STATS float32: [0] loss = P + vf_coef V - ent_coef E, [1] P the mean policy term, [2] V the mean value
 *   term, [3] E the mean joint entropy, [4] the mean of logp_old - logp (the kl estimate), [5] the fraction of actors whose
 *   ratio left [1 - clip, 1 + clip], [6] the number of skipped actors, [7] the largest |logp - logp_old| of the others.
 * The means are over all N = B x actors of the class.  An actor whose joint logp or stored old logp is not finite, or whose
 * log-ratio exceeds 80 in magnitude, is SKIPPED: it adds 0 to [1], [4], [5] and has no policy gradient, but keeps its
 * entropy and value terms.  csrc/aie_trainer_math.h states every operation (float32, each rounded on its own, in the sampler's
 * arithmetic: a step evaluated under the logits it was sampled from has ratio exactly 1); the sums are float64 over the
 * float32 terms in an order that is fixed for a given B, so two runs give the same bits; no atomics.
 * d_workspace: device memory, 8-byte aligned, the call's own until it has run: calls that may run at the same time (two
 * streams) need one each, and a captured call keeps the pointer.  Each wavefront (at most AIE_PPO_MAX_WAVES) leaves one partial record of 128 bytes there; the second launch adds them.  The size to give is
 * what the workspace_bytes function returns for B: never more than AIE_PPO_MAX_WAVES * 128 (1 MiB, enough for every B), or
 * the negative AIE_E_INVALID for a NULL env or B < 1.
 * Either class may be NULL; with both NULL the call checks B and the samplers' refusals, launches nothing and returns AIE_OK.  All scenarios.  Asynchronous on `stream`, no allocation, no synchronisation, capturable in a
 * hipGraph.  AIE_E_INVALID for B < 1, a class without logits, masks, actions, logp_old, adv, grad_logits or stats, values
 * without values_old, returns or grad_values (or grad_values without values), clip <= 0, a workspace that is NULL,
 * misaligned or too small; aie_sample_policy_actions' refusals (AIE_E_UNSUPPORTED) apply. */
#define AIE_PPO_N_STATS 8
#define AIE_PPO_MAX_WAVES 8192
typedef struct aie_ppo_class {          /* one actor class; layouts as aie_policy_evaluate, B for E */
  const float *logits, *values;         /* row b: the network's outputs for batch element b; values NULL: no value term */
  const float* masks;                   /* the "stored" operands: row d_index[b] */
  const int32_t* actions;
  const float *logp_old, *adv, *values_old, *returns;
  const float* adv_moments;             /* NULL, or 2 floats in device memory {mean, rstd} */
  float *grad_logits, *grad_values, *stats;   /* the logits' shape, [B, actors], AIE_PPO_N_STATS; grad_values NULL iff values NULL */
  float clip, vf_clip, vf_coef, ent_coef;
} aie_ppo_class;
int64_t aie_ppo_workspace_bytes(const aie_env* env, int64_t B);
int aie_ppo_loss(aie_env* env, int64_t B, const aie_ppo_class* agents, const aie_ppo_class* planner, const int32_t* d_index,
                 void* d_workspace, int64_t workspace_bytes, void* stream);

/* The policy network's forward pass for both actor classes, ONE launch: per row x[F] -> relu -> H -> relu -> H -> M logits
 * and, optionally, one value -- the two-hidden-layer MLP a rollout evaluates between two environment steps, which as a
 * torch formulation is about fourteen small launches.  Rows are B * n_agents for the agents and B for the planner (any
 * B >= 1, not tied to the environment's E).  Per class (aie_mlp_class): x [rows, F] float32 with a leading dimension in
 * floats (an arena tensor or any device memory, 4-byte aligned); weights row-major [in, out] float32, the leading dimension
 * the out width (what x @ w takes): w1 [F, H], w2 [H, H], w3 [H, M], biases b1 [H], b2 [H], b3 [M]; wv [H] and bv [1] (device
 * memory) the value column, both NULL for none; logits [rows, M] and values [rows] contiguous.
 * THE ARITHMETIC (csrc/aie_trainer_math.h states it once, aie_mlp_row; the CPU test compiles that helper): all float32,
 *   chain(c; a, w) = acc after acc = c; for k ascending: acc = fmaf(a[k], w[k], acc)   -- one accumulator, one rounding per term
 *   h1[j] = relu(chain(b1[j]; x, W1[:, j])), h2[j] = relu(chain(b2[j]; h1, W2[:, j])), relu(v) = v > 0 ? v : 0 (NaN -> 0),
 *   logits[j] = chain(b3[j]; h2, W3[:, j]), value = chain(bv; h2, wv).
 * The kernel's f32 MFMA is that chain; it may pad K with zero weights behind the real terms, which changes no value except
 * the sign of an exact zero: the device equals the helper under float == wherever no NaN occurs.  Two runs give the same
 * bits.  The weights are read from the caller's buffers at every launch (nothing is repacked or cached by the library): an
 * in-place update of them is seen by the next launch, or the next replay of a captured one.  Exactly [rows, M] and [rows]
 * are written.  Either class may be NULL; with both NULL the call launches nothing and returns AIE_OK.  Asynchronous on
 * `stream`, no atomics, no allocation, no synchronisation, capturable in a hipGraph.
 * AIE_E_UNSUPPORTED: H not a multiple of 16, or outside 16 .. 256.  AIE_E_INVALID: B < 1, F or M outside 1 .. 1024,
 * x_ld < F, a NULL among x, the six weight and bias pointers and logits, values without wv or wv without values, wv
 * without bv.  A refused call launches nothing. */
typedef struct aie_mlp_class {
  const float* x; int64_t x_ld;          /* [rows, F] observations (arena tensors included), leading dimension in floats */
  const float *w1, *b1, *w2, *b2, *w3, *b3;   /* [F,H] [H] [H,H] [H] [H,M] [M], leading dimensions = out width */
  const float *wv, *bv;                  /* [H], [1] in device memory; both NULL: no value column */
  float *logits, *values;                /* [rows, M] contiguous; [rows] or NULL iff wv NULL */
  int32_t F, H, M;
} aie_mlp_class;
int aie_policy_mlp_forward(aie_env* env, int64_t B, const aie_mlp_class* agents, const aie_mlp_class* planner, void* stream);

/* The same network's backward pass for both actor classes, THREE launches: the gradients of the eight weight tensors from
 * the gradients with respect to logits and values (aie_ppo_loss's grad_logits and grad_values, say).  Rows, B and the
 * classes as for the forward.  Per class (aie_mlp_grad_class): net -- x, x_ld, the weights, F, H and M as for the forward
 * (net.logits and net.values are ignored); g_logits [rows, M] contiguous and g_values [rows] (NULL exactly when net.wv is);
 * the outputs gw1 .. gbv in the weights' shapes (gwv and gbv NULL exactly when net.wv is).  Nothing is produced for x.
 * THE ARITHMETIC (csrc/aie_trainer_math.h states it once -- aie_mlp_row_backward, aie_mlp_grad_entry -- and the CPU test compiles
 * those helpers): all float32 unless said otherwise; chain0(a, w) = chain(+0; a, w), the forward's chain from zero.  Per row r:
 *   h1, h2 are recomputed exactly as the forward computes them;   dz3[m] = g_logits[r][m], dv = g_values[r];
 *   dh2[j] = chain0 over m ascending of (dz3[m], W3[j][m]), with a value column one last term fmaf(dv, wv[j], acc);
 *   dz2[j] = h2[j] > 0 ? dh2[j] : 0;   dh1[j] = chain0 over k ascending of (dz2[k], W2[j][k]);   dz1[j] = h1[j] > 0 ? dh1[j] : 0.
 * Across rows: segments of AIE_MLP_BWD_SEG consecutive rows (the last may be short); with a_1 = x, a_2 = h1, a_3 = h2,
 *   partial_s(gW_L[k][j]) = chain0 over segment s's rows ascending of (a_L[r][k], dz_L[r][j]);   gwv[k] pairs (h2[r][k], dv[r]);
 *   a bias gradient is the same chain with the activation 1 (acc = acc + dz, rounded once per row);
 *   an entry = the sum of its segment partials in float64, ascending, rounded to float32 once (aie_ppo_loss's convention).
 * The segment length is a compile-time constant: the bits do not depend on the device, on B or on how many compute units
 * ran the call.  A kernel may pad a chain with zero-times-zero terms behind the real ones, which changes nothing except the
 * sign of an exact zero: the device equals the helpers under float == wherever no NaN occurs.  No float atomics; two runs
 * give the same bits.  Every gradient entry is overwritten, not accumulated into.
 * d_workspace: device memory, 16-byte aligned, the call's own until it has run (two streams: one each; a captured call keeps
 * the pointer).  It holds h1, h2, dz2 and dz1 and the segments' partial sums, so it GROWS LINEARLY WITH THE ROW COUNT: per
 * class, with v = 1 with a value column and 0 without,
 *   floats = 4 rows H + ceil(rows / AIE_MLP_BWD_SEG) P,   P = (F + 1) H + (H + 1) H + (H + 1)(M + v),
 * rounded up to a multiple of 64 floats; the sum over the classes given, times 4 bytes, is what the workspace_bytes function
 * returns (or the negative code of the call's own refusal; 0 with no class).
 * Either class may be NULL; with both NULL the call launches nothing and returns AIE_OK.  Asynchronous on `stream`, no
 * allocation, no synchronisation, capturable in a hipGraph.  The forward's refusals for B, F, H, M, x_ld and NULL pointers;
 * AIE_E_INVALID also for a NULL g_logits or required gradient pointer, a g_values, gwv or gbv that is there without net.wv or
 * missing with it, and a workspace that is NULL, misaligned or too small.  A refused call launches and writes nothing. */
#define AIE_MLP_BWD_SEG 256
typedef struct aie_mlp_grad_class {
  aie_mlp_class net;                       /* x, x_ld, weights, F, H, M as for the forward; net.logits / net.values are ignored */
  const float *g_logits, *g_values;        /* [rows, M]; [rows], NULL iff net.wv is NULL */
  float *gw1, *gb1, *gw2, *gb2, *gw3, *gb3, *gwv, *gbv;   /* the weights' shapes; gwv / gbv NULL iff net.wv is NULL */
} aie_mlp_grad_class;
int64_t aie_policy_mlp_backward_workspace_bytes(const aie_env* env, int64_t B, const aie_mlp_grad_class* agents,
                                                const aie_mlp_grad_class* planner);
int aie_policy_mlp_backward(aie_env* env, int64_t B, const aie_mlp_grad_class* agents, const aie_mlp_grad_class* planner,
                            void* d_workspace, int64_t workspace_bytes, void* stream);

/* The one gradient aie_policy_mlp_backward leaves out, ONE launch: the gradient with respect to the first `ncols` columns
 * of x, for a network in front of the MLP (aie_policy_conv_backward takes it as g_feat).  Per row r and column j < ncols,
 *   g_x[r][j] = chain0 over k = 0 .. H-1 ascending of (dz1[r][k], W1[j][k])      (entry (r, j) at g_x[r * ld + j]),
 * with dz1 READ FROM THE WORKSPACE where aie_policy_mlp_backward left it: the call is valid only directly behind
 * aie_policy_mlp_backward with the same classes, B, workspace and stream (nothing else may have written the workspace in
 * between).  It reads the workspace and w1 and writes exactly [rows, ncols] per class; the three launches of the backward
 * are not touched and their outputs do not depend on whether this call follows.  A NULL g_x leaves that class out (both
 * NULL: nothing is launched, AIE_OK).  Asynchronous on `stream`, no atomics, no allocation, capturable in a hipGraph.
 * aie_policy_mlp_backward's refusals for the classes, B and the workspace; AIE_E_INVALID also for a g_x without its class,
 * ncols outside 1 .. F, ld < ncols or a g_x that is not 4-byte aligned.  A refused call launches and writes nothing. */
int aie_policy_mlp_input_grad(aie_env* env, int64_t B, const aie_mlp_grad_class* agents, const aie_mlp_grad_class* planner,
                              void* d_workspace, int64_t workspace_bytes, float* d_g_x_a, int64_t ld_a, int32_t ncols_a,
                              float* d_g_x_p, int64_t ld_p, int32_t ncols_p, void* stream);

/* The convolutional encoder of the agents' egocentric crop, in front of the MLP, ONE launch: per row (one agent of one
 * batch element; any row count >= 1) the crop's C_map float32 planes and two planes of int16 indices go through an
 * embedding and two 3x3 stride-2 convolutions (AIE_CONV_F1, then AIE_CONV_F2 filters, no padding, ReLU each), and the
 * flattened result is written beside a copy of the row's flat observation: x_out is then a legal x of
 * aie_policy_mlp_forward with F = NF + F_flat.  This is the network of the reference's tutorials (num_conv 2, idx_emb_dim 4,
 * input_emb_vocab 100 on the 11 x 11 crop: NF = 128).
 * Per class record (aie_conv_class): map [rows][C_map][h][w] float32 with the row stride map_ld in floats; idx
 * [rows][2][h][w] int16 with the row stride idx_ld in int16 elements (the arena's obs_a_world-map / obs_a_world-idx_map
 * and a trajectory's stored copies differ only in these strides; map 4-byte, idx 2-byte aligned); emb [V, D], w1
 * [9 C, F1], b1 [F1], w2 [9 F1, F2], b2 [F2] float32, contiguous, read where they lie at every launch; flat [rows, F_flat]
 * with the leading dimension flat_ld (NULL: no copy, F_flat is then 0); x_out [rows] with the leading dimension x_ld.
 * THE ARITHMETIC (csrc/aie_trainer_math.h states it once -- aie_conv_input_at, aie_conv1_out, aie_conv2_out -- and the CPU
 * test compiles those helpers): all float32; chain and relu are aie_policy_mlp_forward's.
 *   input     C = C_map + 2 D channels on h x w cells: channel c < C_map is the map's plane c; channel C_map + i D + d is
 *             emb[v][d], v = idx[i][y][x] clamped into 0 .. V-1 (plane i = 0, 1): the reference's concatenation order;
 *   conv1     oh1 = (h - 3) / 2 + 1, ow1 likewise; a1[oy][ox][f] = relu(chain(b1[f]; over k = (ky 3 + kx) C + c ascending of
 *             (in[c][2 oy + ky][2 ox + kx], w1[k][f]))): w1 is Keras' HWIO kernel flattened, no permutation;
 *   conv2     the same on a1 with its F1 channels: oh2 = (oh1 - 3) / 2 + 1, a2[oy][ox][f] with k = (ky 3 + kx) F1 + c;
 *   features  Keras' Flatten of [oh2, ow2, F2]: x_out[r][(y ow2 + x) F2 + f] = a2[y][x][f]; NF = oh2 ow2 F2;
 *   flat      x_out[r][NF + j] = flat[r][j], j < F_flat, the same bits.
 * The device equals the helpers bit for bit: nothing is padded or split.  Exactly [rows, NF + F_flat] is written (with
 * x_ld larger, the columns behind are left alone).  Two runs give the same bits.
 * Supported: C_map 1 .. 32, D 1 .. 8, h and w 7 .. 15, V 1 .. 128; anything else (a full_observability crop of 25 x 25,
 * say) is AIE_E_UNSUPPORTED and the message names the limit.  AIE_E_INVALID: rows < 1, a NULL among map, idx, the five
 * weight pointers and x_out, strides smaller than a row, F_flat < 0 or > 1024, F_flat without flat or flat with F_flat 0,
 * misaligned pointers.  Asynchronous on `stream`, no atomics, no allocation, capturable.  A refused call launches nothing.
 * All scenarios: the environment only carries the device and the error text. */
#define AIE_CONV_F1 16
#define AIE_CONV_F2 32
typedef struct aie_conv_class {
  const float* map; int64_t map_ld;        /* [rows][C_map][h][w], row stride in floats */
  const int16_t* idx; int64_t idx_ld;      /* [rows][2][h][w], row stride in int16 elements */
  const float *emb, *w1, *b1, *w2, *b2;    /* [V,D] [9C,F1] [F1] [9F1,F2] [F2] */
  const float* flat; int64_t flat_ld;      /* [rows, F_flat] or NULL */
  float* x_out; int64_t x_ld;              /* [rows, >= NF + F_flat] */
  int32_t C_map, D, h, w, V, F_flat;
} aie_conv_class;
int aie_policy_conv_forward(aie_env* env, int64_t rows, const aie_conv_class* cls, void* stream);

/* The encoder's backward pass, THREE launches: the gradients of emb, w1, b1, w2 and b2 from g_feat, the gradient with
 * respect to the NF feature columns (aie_policy_mlp_input_grad's output: entry (r, j) at g_feat[r * g_ld + j]).  net: as
 * for the forward (flat, x_out and their strides are ignored).  Every entry of the five outputs, in the weights' shapes,
 * is overwritten.  conv1's activations are recomputed.
 * THE ARITHMETIC (csrc/aie_trainer_math.h: aie_conv_da1, aie_conv_dx, aie_conv_row_emb, aie_conv_backward_host).  Per row:
 *   dz2[p][f] = a2[p][f] > 0 ? g_feat[p F2 + f] : 0;
 *   da1[y][x][c] = chain0 over the conv2 outputs (oy, ox) ascending whose window holds (y, x) (ky = y - 2 oy, kx = x - 2 ox
 *                  in 0 .. 2), and inside one over f = 0 .. F2-1 ascending, of (dz2[oy][ox][f], w2[(ky 3 + kx) F1 + c][f]);
 *   dz1 = a1 > 0 ? da1 : 0;   dx[c][y][x], for the embedding's channels c >= C_map only: the same chain over conv1's
 *   outputs and f = 0 .. F1-1 of (dz1[oy][ox][f], w1[(ky 3 + kx) C + c][f]);
 *   e_r[v][d] = acc after acc = +0; for (i, y, x) ascending with clamped idx[i][y][x] == v: acc = acc + dx[C_map + i D + d][y][x].
 * Across rows, in segments of AIE_MLP_BWD_SEG rows: partial_s(gw2[k][f]) = chain0 over the segment's rows ascending, and
 * inside a row over conv2's outputs (oy, ox) ascending, of (a1[2 oy + ky][2 ox + kx][c], dz2[oy][ox][f]); gw1 likewise with
 * the input and dz1 over conv1's outputs; a bias gradient is the same chain with the activation 1 (acc = acc + dz);
 * partial_s(gemb[v][d]) = acc after acc = +0; for the segment's rows ascending: acc = acc + e_r[v][d].  An entry is the sum
 * of its segment partials in float64, ascending, rounded to float32 once.  The order is a function of the row number and
 * the constant only; no float atomics; two runs give the same bits, and the device equals the helpers bit for bit
 * wherever no NaN occurs.
 * d_workspace: device memory, 16-byte aligned, the call's own until it has run; it holds a1, dz1, dz2 and dx of every row
 * and the segments' partials: floats = rows (2 P1 F1 + NF + 2 h w D) + ceil(rows / AIE_MLP_BWD_SEG) (((9 C + 1) F1 +
 * (9 F1 + 1) F2 + V D) rounded up to 4), P1 = oh1 ow1, rounded up to a multiple of 64; times 4 bytes is what the
 * workspace_bytes function returns (or the negative code of the call's own refusal).  The forward's refusals; AIE_E_INVALID
 * also for a NULL g_feat or gradient pointer, g_ld < NF, and a workspace that is NULL, misaligned or too small.  A refused
 * call launches and writes nothing.  Asynchronous on `stream`, no allocation, capturable in a hipGraph. */
typedef struct aie_conv_grad_class {
  aie_conv_class net;                      /* map, idx, strides, weights and shape as for the forward */
  const float* g_feat; int64_t g_ld;       /* [rows, >= NF] */
  float *gemb, *gw1, *gb1, *gw2, *gb2;     /* the weights' shapes */
} aie_conv_grad_class;
int64_t aie_policy_conv_backward_workspace_bytes(const aie_env* env, int64_t rows, const aie_conv_grad_class* cls);
int aie_policy_conv_backward(aie_env* env, int64_t rows, const aie_conv_grad_class* cls, void* d_workspace,
                             int64_t workspace_bytes, void* stream);

/* Adam with gradient-norm clipping, in place, for up to two parameter groups (one per actor class), TWO launches for both
 * groups together: the last step of an update -- what a trainer otherwise writes as clip_grad_norm_ and a capturable
 * torch.optim.Adam, several dozen small launches over the sixteen tensors of aie_policy_mlp_backward (the reference's
 * tutorials train with Adam, lr 0.0003, grad_clip 10).  No weight decay, no AMSGrad.
 * Per group (aie_opt_group): `tensors`, an array in HOST memory of n_tensors (1 .. AIE_OPT_MAX_TENSORS) descriptors, copied
 * into the kernel argument: w (the weights), g (their gradient), m and v (Adam's moments, zeroed by the caller before the
 * first step): n >= 1 float32 each, any device memory, 4-byte aligned; beta1, beta2 in [0, 1), eps > 0, max_norm (<= 0, or a
 * NaN: no clipping); d_lr: ONE float32 in device memory, read at every launch -- a learning-rate schedule is a fill of that
 * float, not a recapture; d_state: AIE_OPT_STATE_BYTES of device memory, 8-byte aligned, {int64 t; double p1, p2; 8 bytes
 * unused}, zeroed by the caller before the first step: the step count and the running products beta1^t, beta2^t, advanced
 * by every call, replays of a captured one included; d_stats: AIE_OPT_N_STATS float32 in device memory, written by every call.
 * THE ARITHMETIC (csrc/aie_trainer_math.h states it once -- aie_opt_chunk_sumsq, aie_opt_scalars, aie_opt_element -- and the
 * CPU test compiles those helpers):
 *   sum of squares, float64 throughout (the square (double)g * (double)g is exact): a tensor is cut into chunks of
 *     AIE_OPT_CHUNK consecutive elements (the last may be short).  Slot s = 0 .. 255 of a chunk adds its elements 4s .. 4s + 3
 *     in ascending order from +0 (an element past the chunk's end counts as +0); the 256 slots are combined by the binary
 *     tree slot[i] += slot[i ^ 2^L] for L = 0 .. 7, all i at once per level (addition commutes: every slot ends with the same
 *     bits); the group's n2 = its chunks' sums added in ascending order from +0, tensor after tensor, chunk after chunk.
 *     Nothing depends on the device or on how many compute units ran the call.
 *   scalars, float64:  norm = sqrt(n2);  coef = max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1 (torch's formula);
 *     with t == 0: p1 = p2 = 1;  then t += 1, p1 *= beta1, p2 *= beta2;  step = lr / (1 - p1);  b2s = sqrt(1 - p2);
 *     coef, step and b2s are rounded to float32 once, where the elements take them.
 *   per element, float32, every operation rounded on its own (fmaf: rounded once; division and square root correctly rounded):
 *     gc = g * coef;  m = fmaf(1 - beta1, gc, beta1 * m);  v = fmaf((1 - beta2) * gc, gc, beta2 * v);
 *     d = sqrtf(v) / b2s + eps;  w = fmaf(-step, m / d, w).          g is not modified.
 *   A group whose n2 is not finite (a NaN or an infinity among its gradients) is SKIPPED: w, m, v and the state keep their
 *     bits; the other group proceeds (aie_ppo_loss's treatment of a non-finite actor, one level up).
 *   stats: [0] the norm before clipping, [1] coef (0 for a skipped group), [2] t after the call, [3] 1 if skipped, else 0.
 * Two runs from equal starts give the same bits.  No atomics and no ordering between workgroups: the first launch reads g
 * and d_state and writes only the workspace (one float64 per chunk, and a copy of the state); the second reads the workspace,
 * g and d_lr and writes w, m, v, d_state and d_stats.  d_workspace: device memory, 8-byte aligned, the call's own until it has
 * run (two streams: one each; a captured call keeps the pointer), of 8 * (4 + chunks) bytes per group given, chunks = the sum
 * of ceil(n / AIE_OPT_CHUNK) over its tensors: what the workspace_bytes function returns (0 with no group, or the negative
 * code of the call's own refusal).  Accesses are 16 bytes per lane for a tensor whose w, g, m and v are all 16-byte aligned,
 * else 4 bytes; nothing is read or written past n.  Tensors must not overlap one another.
 * Either group may be NULL; with both NULL the call launches nothing and returns AIE_OK.  Asynchronous on `stream`, no
 * allocation, no synchronisation, capturable in a hipGraph.  AIE_E_INVALID, checked in this order (the agents' group first):
 * n_tensors outside 1 .. AIE_OPT_MAX_TENSORS or a NULL `tensors`; a beta outside [0, 1) or eps <= 0 (a NaN included); a NULL
 * or misaligned d_lr, d_state or d_stats; per tensor in order a NULL or misaligned w, g, m or v, or n < 1; more chunks than
 * one launch takes; at last a workspace that is NULL, not 8-byte aligned or too small.  A refused call launches and writes
 * nothing.  All scenarios: the environment only carries the device and the error text. */
#define AIE_OPT_CHUNK 1024        /* elements per workgroup: 256 threads x 4 consecutive */
#define AIE_OPT_MAX_TENSORS 16
#define AIE_OPT_N_STATS 4
#define AIE_OPT_STATE_BYTES 32
typedef struct aie_opt_tensor {
  float* w; const float* g; float *m, *v;   /* weights, their gradient, first and second moment: n float32 each */
  int64_t n;
} aie_opt_tensor;
typedef struct aie_opt_group {
  const aie_opt_tensor* tensors; int32_t n_tensors;   /* host memory */
  float beta1, beta2, eps, max_norm;                  /* max_norm <= 0: no clipping */
  const float* d_lr; void* d_state; float* d_stats;   /* device memory: 1 float32; AIE_OPT_STATE_BYTES; AIE_OPT_N_STATS float32 */
} aie_opt_group;
int64_t aie_adam_workspace_bytes(const aie_env* env, const aie_opt_group* agents, const aie_opt_group* planner);
int aie_adam_step(aie_env* env, const aie_opt_group* agents, const aie_opt_group* planner, void* d_workspace,
                  int64_t workspace_bytes, void* stream);

/* Trajectory storage with the slot index on the device: one launch per step copies up to AIE_TRAJ_MAX_SEGMENTS per-replica
 * blocks (observations, masks, actions, log-probabilities, values -- any device memory, arena tensors included) into
 * replica e's slot d_slot[e] of the caller's ring buffers, then d_slot[e] becomes (d_slot[e] + 1) % n_slots.
 *   d_slot  caller-owned int32 [n_envs] in device memory, zeroed by the caller (a value outside the ring counts as 0).
 * Nothing that changes from step to step travels by value: a launch captured in a hipGraph walks the ring on replay, like
 * the reward log's slot and the samplers' draw index.  Exactly one workgroup reads and advances replica e's counter, after
 * all of its threads have read it.  Copies use 16-byte lane accesses where a segment's source, destination, stride and size
 * allow it for every replica and slot, else 4-byte ones; plain vector loads and stores.  One launch, asynchronous on
 * `stream`, no synchronisation.  AIE_E_INVALID for n_segs outside 1 .. AIE_TRAJ_MAX_SEGMENTS, sizes or strides that are not
 * multiples of 4, rows that do not divide the element count, n_slots < 1, NULL or misaligned pointers. */
#define AIE_TRAJ_MAX_SEGMENTS 16
typedef struct aie_traj_segment {
  const void* src;     /* replica e's block starts at src + e * src_stride                                  */
  void* dst;           /* slot s, replica e: dst + ((int64_t)s * n_envs + e) * bytes                          */
  int64_t src_stride;  /* bytes, a multiple of 4 (an arena tensor's replica stride, or the record stride)     */
  int32_t bytes;       /* per replica, a multiple of 4                                                        */
  int32_t rows;        /* 0 or 1: plain copy.  > 1: the block is [rows][bytes / 4 / rows] 4-byte elements and  */
                       /* is stored transposed (COVID's collated agent masks -> the logits' layout)           */
} aie_traj_segment;
int aie_trajectory_store(aie_env* env, const aie_traj_segment* segs, int32_t n_segs, int32_t n_slots, int32_t* d_slot,
                         void* stream);

/* Same counter RNG, but each sub-action is drawn uniformly among the entries that the
 * CURRENT action masks allow (obs_a_action_mask / obs_p_action_mask; NO-OP is always
 * allowed).  This is the random policy a trainer starts from when it applies the
 * `action_mask` observation to its logits (F/base/base_env.py:141-145,
 * tutorials/rllib/env_wrapper.py:50-211 hand the mask to the policy network). */
int aie_sample_masked_actions(aie_env* env, uint64_t seed, int64_t global_env_offset, int32_t* d_actions_a,
                              int32_t* d_actions_p, void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* AIE_H_ */
