/*
 * aie_layout.h -- what a kernel reads of the layout, and nothing else: the parameter block aie_params (where (a) the
 * per-replica state record that lives in HBM, (b) the dense observation / reward tensors and (c) the action-space and
 * flat-observation bookkeeping that the reference derives at construction time are), aie_spec_normalize, the
 * development switches, the offsets inside the flat observation blocks, the COVID and Saez constants, the counter
 * hashes and the packing of map cells and orders.  Every step and reset kernel is compiled from this file, and it is
 * part of both specialisation cache keys (aie_jit.h), so what no kernel reads lives elsewhere:
 *   aie_layout_build.h  (host only) aie_build_params and its helpers, which fill aie_params and the tensor table;
 *   aie_trainer_math.h  the sampler's, the evaluator's, the PPO loss's, GAE's and the policy MLP's arithmetic and
 *                       kernel arguments -- the trainer kernels and their CPU twins.
 *
 * Plain C99 (also included from HIP C++).  Included by the HIP library
 * (aie_capi.hip / aie_kernels*.hip) and by the CPU restatement oracle/aie_oracle.c so
 * that both step byte-identical records.  (Host C of before the cut: the file's last lines.)
 *
 * Reference logic restated here:
 *   action subspace registration order + single-action map
 *       F/base/base_agent.py:97-169  (_incorporate_component / register_components)
 *   per-component action counts
 *       F/components/build.py:88-98, move.py:69-79,
 *       continuous_double_auction.py:411-431, redistribution.py:920-939
 *   flat observation = concatenation in SORTED key order
 *       F/base/base_env.py:561-612 (_build_packager/_package), keys prefixed with
 *       "<Component.name>-" / "world-" at base_env.py:644-673
 *   flattened masks  F/base/base_agent.py:440-460
 *   map key order    F/base/world.py:59-93 (resources first, then sorted landmarks,
 *                    then <Res>SourceBlock appended at :66)
 */
#ifndef AIE_LAYOUT_H_
#define AIE_LAYOUT_H_

#include <math.h>
#include <stdio.h>
#include <string.h>

#include "aie.h"

#if defined(__HIPCC__)
#define AIE_HD __host__ __device__
#else
#define AIE_HD
#endif

#define AIE_MAX_TENSORS 160
#define AIE_MAX_MASK 544   /* entries of one agent's flattened action mask (4 x 127 prices + ...) */

/* internal action-subspace slots of a mobile agent */
enum {
  AIE_SUB_BUILD = 0,
  AIE_SUB_BUY0 = 1,  /* Buy_Stone  */
  AIE_SUB_SELL0 = 2, /* Sell_Stone */
  AIE_SUB_BUY1 = 3,  /* Buy_Wood   */
  AIE_SUB_SELL1 = 4, /* Sell_Wood  */
  AIE_SUB_GATHER = 5,
  AIE_SUB_LABOR = 6, /* SimpleLabor (one-step-economy) */
  AIE_SUB_HOST = 7,  /* a host component's subspace (aie_config.host_a_*): no bits in the packed action word, no mask
                      * test (always 1) -- its sub-action goes to the tensor host_actions_a, in the order of the slots */
  AIE_N_SUB_SLOTS = 8
};

/* ---- development switches (-DAIE_DEV build only: the shipping kernels compile every test of them to "off") ----
 * aie_params.dev_skip_mask, set by aie_dev_set_skip_mask, switches parts of the scenario's step kernel off so that a
 * launch can be timed without them; the results are then wrong by design.  One bit set per kernel family, named here
 * once: the kernels test these names and tools/devlib.py reads them out of this file.
 *
 * Gather-trade-build (step_body: the full-featured kernel and the traced instances). */
#define AIE_DEV_SKIP_COMPONENTS (1 << 0)       /* every component step, and the CDA price-history decay ahead of them */
#define AIE_DEV_SKIP_REGEN (1 << 1)            /* the resource regeneration (scenario_step_regen) */
#define AIE_DEV_SKIP_MAP_OBS (1 << 2)          /* the map observations; the masks are then rewritten in full */
#define AIE_DEV_SKIP_FLAT_AND_MASKS (1 << 3)   /* BOTH the flat observation vectors (first wave) and the mask writer (second wave) */
#define AIE_DEV_SKIP_REWARDS (1 << 4)          /* compute_rewards (the reward log's slot and `done` are still written) */
#define AIE_DEV_SKIP_RECORD_STORE (1 << 5)     /* record LDS -> HBM of both waves, and the generator's rows */
#define AIE_DEV_SKIP_FLAT_STAGE_A (1 << 6)     /* flat vectors: the per-(commodity, price) sums and the per-agent scalars */
#define AIE_DEV_SKIP_FLAT_CDA (1 << 7)         /* flat vectors: the CDA fill (market rates, order counts, price history) */
#define AIE_DEV_SKIP_FLAT_TAX (1 << 8)         /* flat vectors: the tax fill (rates, calendar, sorted incomes) */
#define AIE_DEV_SKIP_MASKS (1 << 9)            /* the action masks alone (write_action_masks returns at once) */
#define AIE_DEV_SKIP_PLANNER_COPY_OUT (1 << 10) /* full flat rewrite: the planner's staged vectors LDS -> HBM */
#define AIE_DEV_SKIP_BUILD (1 << 11)           /* the Build component */
#define AIE_DEV_SKIP_CDA (1 << 12)             /* the ContinuousDoubleAuction component (its decay still runs) */
#define AIE_DEV_SKIP_GATHER (1 << 13)          /* the Gather component */
#define AIE_DEV_SKIP_TAX (1 << 14)             /* the PeriodicBracketTax component */
#define AIE_DEV_MAP_OBS_FULL (1 << 15)         /* no skip: map observations and masks rewritten in full, not in place */
#define AIE_DEV_SKIP_DRAW_WINDOW (1 << 16)     /* second wave: publishing the components' draw window */
#define AIE_DEV_SKIP_LOCMAP (1 << 17)          /* second wave: the occupancy map (rebuild_locmap) */
#define AIE_DEV_SKIP_ACTION_DECODE (1 << 18)   /* first wave: decode_actions (every agent then does nothing) */
#define AIE_DEV_SKIP_GENERATOR_ROWS (1 << 19)  /* second wave: the MT19937 rows HBM -> registers */
#define AIE_DEV_FLAT_FULL (1 << 20)            /* no skip: flat vectors rewritten in full, not updated in place */
/* One-step-economy (aie_kernels_ose.hip). */
#define AIE_OSE_SKIP_FLAT_ROWS (1 << 0)        /* the agents' flat observation rows */
#define AIE_OSE_SKIP_MASK_ROWS (1 << 1)        /* the agents' mask rows */
#define AIE_OSE_SKIP_METRICS (1 << 2)          /* the metrics block's atomics */
#define AIE_OSE_SKIP_SMALL_OBS (1 << 3)        /* the small observation tensors (time, planner's per-agent and flat rows) */
#define AIE_OSE_SKIP_RECORD_STORE (1 << 4)     /* record LDS -> HBM */
#define AIE_OSE_SKIP_RECORD_LOAD (1 << 5)      /* record HBM -> LDS (the image is then garbage: timing only) */
/* COVID (aie_kernels_covid.hip). */
#define AIE_CV_SKIP_HISTORY_STORE (1 << 0)     /* today's stringency-history byte (and the long history's tail write) */
#define AIE_CV_SKIP_HISTORY_LOADS (1 << 1)     /* the history byte loads (a constant level instead) */
#define AIE_CV_SKIP_OBS (1 << 2)               /* the observation stores */
#define AIE_CV_SKIP_EPISODE_SUMS (1 << 3)      /* the per-state episode sums (read-modify-write) */
#define AIE_CV_SKIP_STATE_ROWS (1 << 4)        /* the state row stores */
/* Policy sampler: not in dev_skip_mask -- AIE_SAMPLER_DEV_SKIP in the environment, which travels above bit 8 of the
 * kernels' wave-count argument (sampler_dev_skip). */
#define AIE_SAMPLER_SKIP_LOADS (1 << 0)        /* the logit / mask entry loads (made-up values instead) */
#define AIE_SAMPLER_SKIP_DRAW_INDEX (1 << 1)   /* reading and advancing the replica's draw index */
#define AIE_SAMPLER_SKIP_ARITHMETIC (1 << 2)   /* everything behind the loads */
#define AIE_SAMPLER_SKIP_ALL (1 << 3)          /* an empty kernel */

/* Everything a kernel needs, passed BY VALUE as the kernel argument. */
typedef struct aie_params {
  aie_config c;

  /* dims */
  int32_t E, n, H, W, HW;
  int32_t P;        /* price levels = max_bid_ask + 1                                  */
  int32_t NB;       /* tax brackets                                                    */
  int32_t M;        /* order-book capacity per commodity side = n * max_num_orders     */
  int32_t CM;       /* map channels in Maps.state: 5 (no water) or 6                   */
  int32_t WV;       /* egocentric window edge = 2*obs_range + 1                        */
  int32_t am_ch, am_h, am_w; /* agents' "world-map": CM+1 x WV x WV (egocentric, last channel =
                              * in-bounds) or, with full_observability, CM x H x W          */
  int32_t has_build, has_cda, has_gather, has_tax, has_labor;
  int32_t planner_acts; /* 1 if the planner has tax action subspaces                   */

  /* action spaces */
  int32_t n_sub_a;                      /* registered agent subspaces, in order        */
  int32_t sub_a_slot[AIE_MAX_SUBSPACES];/* -> AIE_SUB_*                                */
  int32_t sub_a_dim[AIE_MAX_SUBSPACES]; /* number of non-NO-OP actions                 */
  int32_t sub_a_base[AIE_MAX_SUBSPACES];/* first single-action index of the subspace   */
  int32_t A;                            /* single-action mode: total actions incl NO-OP */
  int32_t n_sub_p;                      /* planner subspaces (NB or 0)                 */
  int32_t sub_p_dim;
  int32_t AP;                           /* planner, single-action mode: total actions incl NO-OP */
  int32_t p_row_dim;                    /* entries (NO-OP not counted) of a multi-action planner's rows where they are equally
                                         * long (p_rows_uniform, below): sub_p_dim without foreign rows                  */
  int32_t act_a_width;                  /* ints per agent in d_actions_a               */
  int32_t act_p_width;                  /* ints per replica in d_actions_p             */

  /* flat observation sizes and fragment offsets (in f32 elements) */
  int32_t FA, FP, FPA;                  /* agent flat, planner flat, planner p{i}      */
  int32_t fa_build, fa_cda, fa_gather, fa_tax, fa_time, fa_world;
  int32_t fp_cda, fp_tax, fp_time, fp_world;
  int32_t fpa_tax, fpa_world;
  int32_t fa_labor;                     /* one-step-economy: SimpleLabor-skill            */
  int32_t MA, MP;                       /* flattened mask sizes                        */

  /* per-replica record: byte offsets */
  int32_t rec_bytes;
  int32_t o_cells;  /* u32 [HW]: byte0 stone, byte1 wood, byte2 house owner (i8, -1 none),
                       byte3 static flags (AIE_CELL_WATER | _STONE_SRC | _WOOD_SRC)        */
  int32_t o_loc_r, o_loc_c, o_inv_res, o_esc_res;
  int32_t o_inv_coin, o_esc_coin, o_labor, o_build_payment, o_build_skill, o_bonus_gather_prob;
  int32_t o_util;
  int32_t o_cda_n_bids, o_cda_n_asks, o_cda_bids, o_cda_asks, o_cda_n_orders;
  int32_t o_cda_bid_hist, o_cda_ask_hist, o_cda_price_history;
  int32_t o_tax_cycle_pos, o_tax_rate_idx, o_tax_last_coin, o_tax_last_income;
  int32_t o_tax_last_marginal_rate, o_tax_total_collected;
  int32_t o_timestep, o_completions, o_auto_warmup;
  int32_t o_mask_bits, o_mask_p_open; /* gather-trade-build: the per-agent mask bits (int32 [n]) and the planner's "rates may be
                          * set today" flag the action-mask tensors currently show -- a step rewrites only the masks of agents
                          * whose bits changed and the planner's when the flag flips (round 6); 0 = fields absent */
  int32_t o_skill, o_production, o_first_step; /* one-step-economy / SimpleLabor           */
  int32_t o_mt, o_mt_pos, o_mt_has_gauss, o_mt_gauss;
  int32_t o_tax_last_completions; /* PeriodicBracketTax._last_completions (tax annealing)     */
  int32_t o_error_flags; /* AIE_ERR_* bits (include/aie.h), sticky until reset */
  int32_t o_src_n, o_src_list; /* the regeneration's source doubles of THIS replica (round 6): int32 count, uint16 [AIE_SRC_CAP]
                          * ascending -- double d of a step's 2 H W np.random.rand values targets Wood cell d (d < H W) or Stone
                          * cell d - H W, and only source-block cells can respawn.  Derived from the cells' flag bytes by the
                          * reset kernel (and by aie_set_layout / aie_upload of the cells; load_state on the host), read by every
                          * step -- straight into the registers of the wave that regenerates, while the components run -- instead
                          * of a scan of the flags.  Behind the generator's state, i.e. outside the record's LDS image.  Absent
                          * (0) where the batch shares one list (a_src_list). */
  int32_t o_obs_valid;   /* 1: the observation tensors -- maps, action masks and (round 7) the flat vectors --
                          * hold this replica's current state (a whole step then only rewrites what it
                          * changes); cleared by anything that edits state from outside the kernels:
                          * aie_upload of a record field, Backend.invalidate_observations             */

  /* arena: byte offsets of the dense regions */
  int64_t a_records;
  int64_t a_obs_a_map, a_obs_a_idx, a_obs_a_flat, a_obs_a_mask, a_obs_a_time;
  int64_t a_obs_p_map, a_obs_p_idx, a_obs_p_flat, a_obs_p_mask, a_obs_p_time, a_obs_p_agents;
  int64_t a_rew_a, a_rew_p, a_done;
  int64_t arena_bytes;

  /* exact unsigned division by run-time constants: q / d == __umulhi(q, mg_d) for
   * q < 2^32 / d (d >= 2); see aie__magic() */
  uint32_t mg_WV2, mg_WV, mg_MA, mg_FA, mg_P, mg_2P, mg_taxA, mg_HW, mg_W, mg_sub_p, mg_sub_p_dim;

  /* per-replica episode accumulators behind env.metrics (component get_metrics): touched only
   * when a trade executes / on tax days, so they live outside the streamed record */
  /* regen_halfwidth > 0 (dynamic_layout.py:446-463): the regeneration probability of a source block
   * is signal.convolve2d(max(map, source blocks), regen_weight / d^2 * ones(d, d), "same"), d = 1 + 2 *
   * halfwidth.  With max_health == 1 the convolved plane IS the source-block plane, so the
   * probability is regen_p[resource][number of source blocks in the d x d window]; the reset kernel
   * counts the window once per episode into the record plane o_regen_count. */
  int32_t regen_conv;    /* 1: some regen_halfwidth > 0 */
  int32_t regen_general; /* 1: some resource has regen_halfwidth > 0 AND max_health > 1: the convolved plane changes
                          * with the map, so its probabilities are true window sums (scipy's accumulation order)
                          * over a pre-step snapshot of max(map, source blocks); aie_step_kernel_log only */
  int32_t o_regen_count; /* u8 [AIE_N_RES][H*W] */
  double regen_p[AIE_N_RES][50];
  /* tax_model "saez" (redistribution.py:436-823): per-replica block outside the streamed record,
   * touched on tax days and period starts only.  Layout (bytes): int32 len, int32 reached_min_samples,
   * pad to 16; f64 elas[4] = {elas_t, elas_tm1, log_z0_t, log_z0_tm1}; f64 running_avg[AIE_MAX_BRACKETS];
   * f64 next_rates[AIE_MAX_BRACKETS] (formula output for the coming period start, written by
   * aie_saez_kernel); f64 buffer[saez_cap][2] = (income, marginal rate), oldest first. */
  int64_t a_saez;
  int32_t saez_stride, saez_cap;
  int64_t a_saez_global; /* shared: int32 len (16 B), then f64 [saez_global_cap][2]: the trainer's cross-replica buffer */
  int32_t saez_global_cap, saez_pad_;
  int64_t a_layout_prob; /* shared f64 [AIE_N_RES][H*W]: source probability maps of the generated layouts (layout_gen
                          * UNIFORM / QUADRANT: uploaded once by the host, tensor "layout_source_prob") */
  /* Generated layouts under AIE_RNG_FAST (aie__layout_staged): a replica's k-th reset draws its source layout from a
   * stream of its own (aie_layout_stream: keyed by the replica's stream and k, the record's fourth state word), so the
   * layout does not depend on what the episode's steps drew and can be made AHEAD of the reset.  Staging area:
   *   a_layout_stage  u8 [E][layout_stage_stride]: bit 0 Stone source, bit 1 Wood source per cell (before the checker /
   *                   water-line cuts), valid iff the tag equals the tag of the replica's coming reset;
   *   a_layout_tag    u64 [E]: aie_layout_tag of the staged layout (0: none);
   *   a_layout_ctl    int32 [4]: staged layouts consumed since the last refill, the refill's go flag, installs from the
   *                   staging area, layouts drawn inside a reset (development counters).
   * A reset installs the staged layout when the tag matches and draws the layout itself otherwise (same stream, same
   * result); behind every reset launch a one-thread kernel decides whether enough layouts were consumed for a refill
   * launch to pay (its duration is that of the slowest replica, however many it draws). */
  int64_t a_layout_stage, a_layout_tag, a_layout_ctl;
  int32_t layout_stage_stride;
  int32_t o_cells8;      /* record: u8 [H*W] padded to 16, tensor "cells_packed": one byte per map cell (aie_cell_pack8,
                          * below), derived from o_cells and kept beside it by the reset and step kernels, so that a step
                          * fetches a byte per cell on its way in and expands it into the LDS image's words.  Holds
                          * WHENEVER obs_valid != 0; a step that finds obs_valid == 0 reads the words and rewrites the
                          * plane.  Behind the generator's state like o_src_list, i.e. outside the LDS image.  0 = absent
                          * (aie__cell_plane: the byte cannot hold the configuration's cells) */
  int64_t a_src_list;    /* shared, fixed layouts with shared_layout only (aie__shared_src_list): int32 count (16 B), then
                          * uint16 [AIE_SRC_CAP]: the regeneration draws that target a source block (double d of a step's
                          * 2 H W np.random.rand values: Wood cell d, or Stone cell d - H W), derived once by
                          * aie_set_layout instead of by every step from the cells' flag bytes; count > AIE_SRC_CAP: no
                          * list (row-by-row regeneration) */
  int32_t o_tax_saez_rates; /* record: f64 [NB] curr_bracket_tax_rates */
  int32_t o_tax_saez_obs_rates; /* record: f64 [NB] _curr_rates_obs: the rates the "curr_rates" observation shows,
                                   refreshed at period starts and -- BEFORE the running average replaces the
                                   bracket rates -- at reset (redistribution.py:1123, 1136-1137) */
  double saez_edges[AIE_SAEZ_BINS + 1]; /* np.linspace(0, top cutoff, 101), :286-288 */
  int64_t a_events;      /* dense-log events of replicas [0, ev_replicas): int32 count (16 B), then rows */
  int32_t ev_replicas, ev_cap, ev_stride, ev_pad_;
  int64_t a_metrics;
  int32_t met_bytes;
  int32_t mo_cda;        /* int32 [2: sell, buy][AIE_N_RES][n][2: n_sales, sum of prices]         */
  int32_t mo_tax_sched;  /* f64 [NB] sum over tax days of the bracket rates                       */
  int32_t mo_tax_income; /* f64 [n]  sum over tax days of max(0, income)                          */
  int32_t mo_tax_paid;   /* f64 [n]  sum over tax days of the tax paid                            */
  int32_t mo_tax_eff;    /* f64      sum of all effective tax rates (n per tax day)               */
  int32_t mo_tax_occ;    /* int32 [NB] incomes observed per bracket                               */
  int32_t mo_tax_days;   /* int32    tax days so far                                              */
  /* flattened agent action mask, element m: allowed iff ((mask_bits >> sh) & msk) >= thr with
   * sh = test & 31, msk = (test >> 8) & 0xff, thr = test >> 16 (mask_bits: write_action_masks) */
  uint32_t mask_test[AIE_MAX_MASK];
  int32_t dev_skip_mask; /* development: AIE_DEV_SKIP_* / AIE_OSE_SKIP_* / AIE_CV_SKIP_* bits (above); 0 in normal operation */
  uint64_t* dev_trace;   /* development: 8 clock stamps per workgroup (start, components.., regen, end), or NULL */
  /* aie_set_reward_log: the caller's reward log, f32 [rew_slots][E][n + 2] = agents' rewards, the planner's reward, done --
   * or NULL.  In the device-side block (not a kernel argument) so that a launch captured in a hipGraph sees a later
   * aie_set_reward_log call (round 6).  rew_epoch: bumped by every such call, restarts the replicas' slot
   * counters (record fields o_rew_slot / o_rew_epoch). */
  float* rew_log;
  int32_t rew_slots, rew_epoch;

  /* ---- COVID-19 scenario (aie__build_covid) ---- */
  int32_t cv_L;          /* filter_len                                                     */
  int32_t cv_F;          /* num_filters                                                    */
  int32_t cv_NL;         /* num_stringency_levels                                          */
  int32_t cv_NS;         /* num_subsidy_levels                                             */
  int32_t cv_nch;        /* 16-day chunks in the per-replica stringency history           */
  int32_t cv_row;        /* bytes per history chunk = 16 * n rounded up to 64              */
  int32_t cv_nrow_obs;   /* rows of the per-replica agent observation block               */
  int32_t cv_pitch;      /* lanes per row of the record's per-state rows (= n: packed; the kernel is HBM-bound and a
                          * 64-lane pitch would move 20 % idle bytes)                       */
  int32_t cv_t_first_delivery;
  int32_t o_cv_state;    /* record: AIE_CV_ST_* float32 rows of 64 lanes                  */
  int32_t o_cv_cooldown; /* record: int32 row                                              */
  int32_t o_cv_subsidy_level;
  int32_t o_cv_sums;     /* record: AIE_CV_SUM_* float64 rows of 64 lanes                 */
  int32_t o_cv_p_index;  /* record: planner Health Index, Economic Index (float32 x 2)    */
  int32_t o_cv_ring;     /* record: uint8 [32][64]: the stringency levels of the 32 most recent days, row = (filter_len + day) & 31,
                          * one 64-byte row per day (what a step reads of the recent past -- yesterday, beta_delay days
                          * ago, the lagged observation -- and writes for today are single rows, not 51 scattered bytes) */
  int32_t o_cv_acc;      /* record: float64 [F] rows of n lanes: filter_recurrence: each filter's discounted sum of stringency
                          * deltas over the current window; else: each filter's sum over the NEXT step's window without that
                          * step's own day, formed by the tail of the previous step (or by reset) */
  /* window sums (filter_recurrence == 0) over the NON-ZERO level changes only: per replica and state the change events
   * (history day tau, delta) of the episode so far + the pre-episode days, oldest first.  A day without a change adds
   * fma(0, tap, acc) == acc to the reference's sum, so the sum over the events in the same order is the SAME float64,
   * bit for bit.  A state that would exceed the list's capacity makes its replica "dense" until the next reset: the
   * kernel then streams the 600-day history as before.                                                          */
  int32_t cv_ev_groups;  /* capacity of a state's event list in groups of 4 (0: filter_recurrence)                */
  int32_t o_cv_ev_ht;    /* record: int32 row: head | tail << 16 of every state's list                           */
  int32_t o_cv_dense;    /* record: int32: 1 = this replica streams the whole window (list overflow)              */
  int32_t o_cv_tail_pending; /* record: int32: the step kernel took a step that aie_covid_window_kernel has to follow up  */
  int64_t a_cv_events;   /* uint32 [E][cv_ev_groups][64 lanes][4]: tau | (delta & 0xff) << 16                     */
  int64_t a_cv_ev0;      /* shared: the pre-episode days' lists in the same format, then int32 [64] head/tail row,
                          * then int32 dense flag (a pre-episode list overflowed); aie_covid_prepare_kernel       */
  int64_t a_cv_consts;   /* AIE_CV_K_* float64 rows of 64 (shared by all replicas)         */
  int64_t a_cv_filters;  /* float64 [pad+L+pad][F]                                              */
  int64_t a_cv_hist0;    /* uint8 [L+1][n]   stringency levels of the L days before t=0 + t=0 */
  int64_t a_cv_hist0c;   /* uint8 [nch][cv_row]: the same days in the per-replica history format (what reset copies);
                          * derived from a_cv_hist0 by aie_covid_prepare_kernel whenever that table is uploaded  */
  int64_t a_cv_acc0;     /* float64 [F][64]: what reset puts into o_cv_acc (recurrence: A_0; window sums: step 1's sums over
                          * the pre-episode days), ditto */
  int64_t a_cv_lag_obs;  /* uint8 [beta_delay][n]                                          */
  int64_t a_cv_replay_a; /* uint8 [T][64]: replay_policies: the states' stringency action of step t in row t - 1 */
  int64_t a_cv_replay_p; /* int32 [T]: replay_policies: the planner's subsidy level of step t at t - 1            */
  int64_t a_cv_replay_state; /* float64 [6: S, I, R, V, D, U][T + 1][64]: replay_data                             */
  int64_t a_cv_hist;     /* uint8 [E][nch][cv_row]                                         */
  int64_t a_cv_obs_a;    /* float32 [E][cv_nrow_obs][n]                                    */
  int64_t a_cv_obs_p;    /* float32 [E][4 + 1 + NS]                                        */
  /* properties of run-time scalars that DO shape the code (they stay in the instances' images, the values do not) */
  int32_t sh_energy_warmup; /* energy_warmup_constant > 0: the labor cost is weighted by 1 - exp(-v / constant)   */
  int32_t sh_eta_is_one;    /* isoelastic_eta == 1: log utility instead of the power form                        */
  int32_t auto_reset;    /* run-time switch (aie_set_auto_reset): replicas restart inside the launch that ends their episode */
  /* per-replica call counters (record fields, so that nothing a step needs travels by value from a host-side counter: a
   * captured hipGraph of aie_step / aie_step_sample_next replays correctly): o_sample_t = draws of the synthetic random
   * policy so far (the `t` of its counter RNG), o_rew_slot = the reward-log slot the next step fills, o_rew_epoch = the
   * aie_set_reward_log call that slot counter belongs to (a new call restarts the slots at 0 without touching memory) */
  int32_t o_sample_t, o_rew_slot, o_rew_epoch;
  int32_t dev_draw_window; /* development (tests): capacity of the components' draw window in words, 0 = stage_window_words();
                            * honoured by aie_step_kernel_log only */
  /* ---- action subspaces of host components (aie_config.host_*; all zero without them) ----
   * Agents: slots AIE_SUB_HOST among sub_a_*; the k-th such slot is column k of host_actions_a.
   * Planner: its rows are the n_sub_p tax rows (one block: PeriodicBracketTax is one component) with the foreign rows
   * listed ahead of that component in front of the block and the others behind it.  Row r is column r of d_actions_p
   * in multi-action mode; in single-action mode the one index runs over NO-OP and then the rows' entries in order. */
  int32_t n_host_a, n_host_p;
  int32_t tax_p_row0;    /* row (multi-action column) of the first tax bracket                                  */
  int32_t tax_p_base;    /* single-action index of the first tax entry (1 without foreign rows ahead)            */
  int32_t tax_p_moff;    /* flattened planner mask: offset of the tax block (multi-action: of its first row's NO-OP
                          * entry; single-action: of its first rate entry == tax_p_base)                         */
  int32_t p_rows_uniform;/* 1: every planner row has p_row_dim entries + NO-OP (what the samplers' planner group needs) */
  int32_t hp_dim[AIE_MAX_HOST_SUBSPACES];  /* foreign planner row k: choices,                                    */
  int32_t hp_row[AIE_MAX_HOST_SUBSPACES];  /* its row,                                                           */
  int32_t hp_base[AIE_MAX_HOST_SUBSPACES]; /* its first single-action index,                                     */
  int32_t hp_moff[AIE_MAX_HOST_SUBSPACES]; /* the offset of its first entry in the flattened mask (multi-action: its NO-OP) */
  int64_t a_host_act_a, a_host_act_p;      /* arena: int32 [E][n][n_host_a], int32 [E][n_host_p]                 */
} aie_params;

/* Compile-time instances of the step kernel (aie_spec_generated.h) bake a CONSTANT image of aie_params into the code.
 * An image stands for a FAMILY of configurations: everything that shapes the code (component tuple, agent count,
 * world size, observation window, book capacity, bracket / rate counts, every flag, every record offset and table
 * derived from those) is in it; what does not is read from the run-time block (Ctx::R) and is blanked in the image:
 *   - what depends on the batch: the replica count, every arena offset, the dense-log event buffer, development hooks;
 *   - the configuration's SCALARS and value tables: episode_length, starting_agent_coin, isoelastic_eta, energy_cost,
 *     energy_warmup_constant, mixing weight, every labor cost, Build payment / multiplier, order_duration, tax period
 *     (gather-trade-build), bracket cutoffs, the discretised / fixed rates, rate_min / rate_max, the annealing schedule,
 *     regeneration weights (and regen_p derived from them), fixed-four locations and skills, split-layout ranks,
 *     starting coverages / clumpiness of generated layouts, SimpleLabor's skills and multiplier, labor exponent / cost.
 * The blanked scalars are POISONED (0x5A bytes), not zeroed: a kernel line that still read one of them from the
 * image would compute with 1 515 870 810 / 2.6e130 and fail every parity test, instead of passing by accident where
 * the configuration's value happens to be 0.
 * An environment runs on an instance iff its normalised block equals the instance's image byte for byte
 * (aie_capi.hip: aie_create): same family, any scalars, any replica count, any seed. */
static inline void aie_spec_normalize(aie_params* p) {
  p->E = 0;
  p->c.n_envs = 0;
  p->a_records = 0;
  p->a_obs_a_map = p->a_obs_a_idx = p->a_obs_a_flat = p->a_obs_a_mask = p->a_obs_a_time = 0;
  p->a_obs_p_map = p->a_obs_p_idx = p->a_obs_p_flat = p->a_obs_p_mask = p->a_obs_p_time = p->a_obs_p_agents = 0;
  p->a_rew_a = p->a_rew_p = p->a_done = 0;
  p->arena_bytes = 0;
  p->a_saez = p->a_events = p->a_metrics = p->a_saez_global = 0;
  p->a_cv_consts = p->a_cv_filters = p->a_cv_hist0 = p->a_cv_lag_obs = p->a_cv_hist = p->a_cv_obs_a = p->a_cv_obs_p = 0;
  p->a_cv_hist0c = p->a_cv_acc0 = 0;
  p->a_cv_events = p->a_cv_ev0 = 0;
  p->a_cv_replay_a = p->a_cv_replay_p = p->a_cv_replay_state = 0;
  p->a_layout_prob = 0;
  p->a_layout_stage = p->a_layout_tag = p->a_layout_ctl = 0;
  p->a_src_list = 0;
  p->a_host_act_a = p->a_host_act_p = 0;
  p->dev_skip_mask = 0;
  p->dev_trace = 0;
  p->rew_log = 0;
  p->rew_slots = p->rew_epoch = 0;
  p->dev_draw_window = 0;
  p->auto_reset = 0;
  p->ev_replicas = p->ev_cap = p->ev_stride = 0;  /* dense-log replicas: the fast kernels never record events */
  p->c.dense_log_replicas = 0;
  memset(p->c.labor_skills, 0, sizeof(p->c.labor_skills));  /* SimpleLabor's skills are data, read from the run-time block */
#define AIE__BLANK(field) memset(&(field), 0x5A, sizeof(field))
  {
    aie_config* c = &p->c;
    AIE__BLANK(c->episode_length); AIE__BLANK(c->starting_agent_coin); AIE__BLANK(c->isoelastic_eta);
    AIE__BLANK(c->energy_cost); AIE__BLANK(c->energy_warmup_constant); AIE__BLANK(c->mixing_weight_gini_vs_coin);
    AIE__BLANK(c->build_payment); AIE__BLANK(c->build_payment_max_skill_multiplier); AIE__BLANK(c->build_labor);
    AIE__BLANK(c->move_labor); AIE__BLANK(c->collect_labor); AIE__BLANK(c->cda_order_labor);
    AIE__BLANK(c->cda_order_duration);
    /* one-step-economy keeps its tax period in the image: with period 1 two record fields are dead and are neither
     * loaded nor stored (aie_kernels_ose.hip: ose_load_record) -- there the period shapes the code */
    if (c->scenario != AIE_SCN_ONE_STEP_ECONOMY) AIE__BLANK(c->tax_period);
    AIE__BLANK(c->tax_bracket_cutoffs); AIE__BLANK(c->tax_disc_rates); AIE__BLANK(c->tax_fixed_rates);
    AIE__BLANK(c->tax_rate_max); AIE__BLANK(c->tax_rate_min); AIE__BLANK(c->tax_annealing_warmup);
    AIE__BLANK(c->tax_annealing_slope); AIE__BLANK(c->regen_weight); AIE__BLANK(c->ranked_locs);
    AIE__BLANK(c->avg_ranked_skill); AIE__BLANK(c->split_top_ranks); AIE__BLANK(c->layout_coverage);
    AIE__BLANK(c->layout_clump); AIE__BLANK(c->ose_labor_exponent); AIE__BLANK(c->ose_labor_cost);
    AIE__BLANK(c->labor_pmsm); AIE__BLANK(c->saez_buffer_size); AIE__BLANK(c->saez_fixed_elas);
    AIE__BLANK(p->regen_p); AIE__BLANK(p->saez_edges);
  }
#undef AIE__BLANK
}

/* ---- inside a component's block of the flat observation vectors ----
 * Where each of the block's sorted keys starts, in f32 elements from the block's own offset (aie_params: fa_cda,
 * fp_tax, fpa_tax, ...), and how long the block is; P = price levels, NB = tax brackets, n = agents.  The kernels and
 * the oracle address the entries through these names only (foundation/obs_keys.py derives the same layout from the
 * reference's keys and is pinned against it).
 * ContinuousDoubleAuction (continuous_double_auction.py:491-542): a key holds (commodity r, price k) at r * P + k,
 * market_rate one entry per commodity. */
#define AIE_FA_CDA_AVAILABLE_ASKS(P) 0
#define AIE_FA_CDA_AVAILABLE_BIDS(P) (2 * (P))
#define AIE_FA_CDA_MARKET_RATE(P) (4 * (P))
#define AIE_FA_CDA_MY_ASKS(P) (4 * (P) + 2)
#define AIE_FA_CDA_MY_BIDS(P) (6 * (P) + 2)
#define AIE_FA_CDA_PRICE_HISTORY(P) (8 * (P) + 2)
#define AIE_FA_CDA_LEN(P) (10 * (P) + 2)
#define AIE_FP_CDA_FULL_ASKS(P) 0
#define AIE_FP_CDA_FULL_BIDS(P) (2 * (P))
#define AIE_FP_CDA_MARKET_RATE(P) (4 * (P))
#define AIE_FP_CDA_PRICE_HISTORY(P) (4 * (P) + 2)
#define AIE_FP_CDA_LEN(P) (6 * (P) + 2)
/* PeriodicBracketTax (redistribution.py:974-1023): the planner's block is the agents' without marginal_rate, so the
 * keys ahead of it (AIE_F_TAX_*) sit at the same place in both */
#define AIE_F_TAX_CURR_RATES 0
#define AIE_F_TAX_IS_FIRST_DAY(NB) (NB)
#define AIE_F_TAX_IS_TAX_DAY(NB) ((NB) + 1)
#define AIE_F_TAX_LAST_INCOMES(NB) ((NB) + 2)     /* n entries, ascending */
#define AIE_FA_TAX_MARGINAL_RATE(NB, n) ((NB) + 2 + (n))
#define AIE_FA_TAX_PHASE(NB, n) ((NB) + 3 + (n))
#define AIE_FA_TAX_LEN(NB, n) ((NB) + (n) + 4)
#define AIE_FP_TAX_PHASE(NB, n) ((NB) + 2 + (n))
#define AIE_FP_TAX_LEN(NB, n) ((NB) + (n) + 3)
/* ... and its fragment of the planner's per-agent vector p{i} */
enum { AIE_FPA_TAX_CURR_MARGINAL_RATE = 0, AIE_FPA_TAX_LAST_INCOME = 1, AIE_FPA_TAX_LAST_MARGINAL_RATE = 2, AIE_FPA_TAX_LEN = 3 };

static inline uint32_t aie__magic(int64_t d) {
  return d <= 1 ? 0u : (uint32_t)((0x100000000ll + d - 1) / d);
}

static inline int64_t aie__align(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

static inline int aie__dtype_size(int dt) {
  switch (dt) {
    case AIE_U8: case AIE_I8: return 1;
    case AIE_I16: return 2;
    case AIE_I32: case AIE_U32: case AIE_F32: return 4;
    default: return 8;
  }
}

static inline int aie__has(const aie_config* c, int comp) {
  for (int i = 0; i < c->n_components; ++i)
    if (c->components[i] == comp) return 1;
  return 0;
}

/* source-block doubles the sparse regeneration handles (else: row-by-row) */
#define AIE_SRC_CAP 128
/* One list of the regeneration's source doubles for the whole batch (aie_params.a_src_list): every replica has the same,
 * never-changing source blocks */
static inline int aie__shared_src_list(const aie_config* c) {
  return c->scenario == AIE_SCN_GTB && c->shared_layout && c->layout_gen == AIE_LAYOUT_FIXED;
}
/* ... which the kernels use with the counter stream only (aie_device.h: shared_src_list); everybody else keeps a list
 * per replica in the record (o_src_n / o_src_list) */
static inline int aie__record_src_list(const aie_config* c) {
  return c->scenario == AIE_SCN_GTB && !(aie__shared_src_list(c) && c->rng_mode == AIE_RNG_FAST);
}
/* Whether a map cell fits the byte of aie_cell_pack8 (record field o_cells8): Stone and Wood are 0 or 1 and the owner is
 * one of at most 7 agents.  Everybody else keeps the word-per-cell way in and the record's bytes as they were. */
static inline int aie__cell_plane(const aie_config* c) {
  return c->scenario == AIE_SCN_GTB && c->max_health[0] == 1 && c->max_health[1] == 1 && c->n_agents <= 7;
}
/* words of generator state in a replica's record ("mt"): MT19937's key, or (key32, block number, salt, 0) of the
 * counter stream (include/aie.h: AIE_RNG_FAST) */
static inline int32_t aie__rng_state_words(const aie_config* c) { return c->rng_mode == AIE_RNG_FAST ? 4 : AIE_MT_N; }
/* generated layouts come from a stream of their own, drawn ahead of the reset (aie_params: a_layout_stage) */
AIE_HD static inline int aie__layout_staged(const aie_config* c) {
  return c->scenario == AIE_SCN_GTB && c->layout_gen != AIE_LAYOUT_FIXED && c->rng_mode == AIE_RNG_FAST;
}
/* The layout stream of a replica's k-th reset, k = st[3], from its stream's state st = (key, block, salt, k): the same
 * Philox function with key + 0x9E3779B9 (k >> 15) and the counter's high word salt | 0x8000 | (k & 0x7fff) -- bit 15 is
 * never set in the replica's own stream (its pair index stays below 2^47).  out = (key, salt); the stream starts at its
 * block 0 (state block 0xffffffff, position 624: the first draw opens block 0). */
AIE_HD static inline void aie_layout_stream(const uint32_t st[4], uint32_t out[2]) {
  out[0] = st[0] + 0x9E3779B9u * (st[3] >> 15);
  out[1] = st[2] | 0x8000u | (st[3] & 0x7fffu);
}
AIE_HD static inline uint64_t aie_layout_tag(const uint32_t st[4]) {  /* never 0: bit 15 */
  uint32_t ks[2];
  aie_layout_stream(st, ks);
  return ((uint64_t)ks[0] << 32) | (uint64_t)ks[1];
}

/* ---- COVID-19 (F/scenarios/covid19/covid19_env.py + F/components/covid19_components.py) ----
 * One wavefront per replica, one lane per US state.  Per-state model constants are float64
 * rows of 64 lanes (values the reference holds as float32 / int32 are exactly representable);
 * the stringency history is kept per replica as [16-day chunk][state][16 bytes] so that a
 * lane streams its own 601-day window with 16-byte loads that are contiguous across lanes. */
enum {
  AIE_CV_K_POP = 0, AIE_CV_K_BETA_SLOPE, AIE_CV_K_BETA_INTERCEPT, AIE_CV_K_UNEMP_BIAS,
  AIE_CV_K_MAX_PROD, AIE_CV_K_HEALTH_NORM, AIE_CV_K_ECON_NORM,
  AIE_CV_K_MIN_HEALTH, AIE_CV_K_MAX_HEALTH, AIE_CV_K_MIN_ECON, AIE_CV_K_MAX_ECON,
  AIE_CV_K_W_HEALTH, AIE_CV_K_W_ECON, AIE_CV_K_MAX_DAILY_SUBSIDY, AIE_CV_K_VACCINES_PER_DELIVERY,
  AIE_CV_K_S0, AIE_CV_K_I0, AIE_CV_K_R0, AIE_CV_K_D0, AIE_CV_K_U0, AIE_CV_K_V0,
  AIE_CV_K_CONV_W0,                                       /* + f, f < AIE_COVID_MAX_FILTERS */
  AIE_CV_K_COUNT = AIE_CV_K_CONV_W0 + AIE_COVID_MAX_FILTERS
};
enum { AIE_CV_ST_S = 0, AIE_CV_ST_I, AIE_CV_ST_R, AIE_CV_ST_D, AIE_CV_ST_V, AIE_CV_ST_U,
       AIE_CV_ST_PROD, AIE_CV_ST_SUBSIDY,
       AIE_CV_ST_HEALTH_INDEX, AIE_CV_ST_ECONOMIC_INDEX, /* agent.state["Health/Economic Index"], float32 running sums */
       AIE_CV_ST_COUNT };
/* float64 per-state sums over the episode's days (scenario_metrics, covid19_env.py:1613-1687) */
enum { AIE_CV_SUM_UNEMPLOYED = 0, AIE_CV_SUM_STRINGENCY, AIE_CV_SUM_PRODUCTIVITY, AIE_CV_SUM_SUBSIDY, AIE_CV_SUM_COUNT };
/* rows of the agent observation block */
enum { AIE_CV_OB_STATE = 0, AIE_CV_OB_PROD = 6, AIE_CV_OB_LAG = 7, AIE_CV_OB_TIME = 8, AIE_CV_OB_POLICY = 9,
       AIE_CV_OB_T_SUBSIDY = 10, AIE_CV_OB_SUBSIDY_LEVEL = 11, AIE_CV_OB_T_VACCINE = 12, AIE_CV_OB_MASK = 13 };

#define AIE_CV_GROUP 2            /* history chunks fetched per prefetch group                 */
#define AIE_CV_EVENT_CAP 64       /* level changes per state a replica's event list holds (multiple of 4)      */
#ifndef AIE_CV_WIN_WAVES
#define AIE_CV_WIN_WAVES 8        /* replicas per workgroup of the window-sum kernel (they share the LDS tap table) */
#endif
#define AIE_CV_TAP_PAD_FRONT 16   /* zero rows before tap 0 in the filter-tap table            */
#define AIE_CV_TAP_PAD_BACK (16 * (AIE_CV_GROUP + 3))

#define AIE_SAEZ_OFF_ELAS 16
#define AIE_SAEZ_OFF_AVG (AIE_SAEZ_OFF_ELAS + 32)
#define AIE_SAEZ_OFF_NEXT (AIE_SAEZ_OFF_AVG + 8 * AIE_MAX_BRACKETS)
#define AIE_SAEZ_OFF_BUF (AIE_SAEZ_OFF_NEXT + 8 * AIE_MAX_BRACKETS)

/* Counter-based RNG of the benchmark's synthetic uniform random policy
 * (SURVEY.md 8(d)): splitmix64 finaliser over (seed, global replica id, t, slot). */
AIE_HD static inline uint32_t aie_counter_rng(uint64_t seed, uint64_t env, uint64_t t, uint64_t slot) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (env + 1ull);
  z ^= (t + 1ull) * 0xBF58476D1CE4E5B9ull;
  z ^= (slot + 1ull) * 0x94D049BB133111EBull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (uint32_t)(z >> 32);
}

/* annealed_tax_limit, F/components/utils.py:10-56 */
AIE_HD static inline double aie_annealed_tax_limit(int completions, double warmup, double slope, double final_max) {
  double pv = slope * ((double)completions - warmup);
  pv = pv < 1.0 ? pv : 1.0;
  pv = pv > 0.0 ? pv : 0.0;
  return pv * final_max;
}

/* packed map cell */
#define AIE_CELL_WATER 1u
#define AIE_CELL_STONE_SRC 2u
#define AIE_CELL_WOOD_SRC 4u
#define AIE_CELL_STONE(w) ((w) & 0xffu)
#define AIE_CELL_WOOD(w) (((w) >> 8) & 0xffu)
#define AIE_CELL_OWNER(w) ((int)(int8_t)(((w) >> 16) & 0xffu))
#define AIE_CELL_FLAGS(w) (((w) >> 24) & 0xffu)
#define AIE_CELL_PACK(st, wd, own, fl) \
  ((uint32_t)(st) | ((uint32_t)(wd) << 8) | (((uint32_t)(own) & 0xffu) << 16) | ((uint32_t)(fl) << 24))

/* ... and its byte (o_cells8, where aie__cell_plane holds): bits 0-2 the flag byte, bit 3 Stone, bit 4 Wood, bits 5-7 the
 * owner -- 0 none (0xff in the word), k + 1 agent k.  unpack8(pack8(w)) == w for every word such a configuration holds. */
AIE_HD static inline uint32_t aie_cell_pack8(uint32_t w) {
  return (AIE_CELL_FLAGS(w) & 7u) | ((w & 1u) << 3) | (((w >> 8) & 1u) << 4) | (((((w >> 16) & 0xffu) + 1u) & 7u) << 5);
}
AIE_HD static inline uint32_t aie_cell_unpack8(uint32_t b) {
  return AIE_CELL_PACK((b >> 3) & 1u, (b >> 4) & 1u, (b >> 5) - 1u, b & 7u);
}

/* order word packing: agent | price << 8 | lifetime << 16 */
#define AIE_ORD_AGENT(o) ((o) & 0xff)
#define AIE_ORD_PRICE(o) (((o) >> 8) & 0xff)
#define AIE_ORD_LIFE(o) (((o) >> 16) & 0xffff)
#define AIE_ORD_PACK(a, p, l) ((int32_t)((a) | ((p) << 8) | ((l) << 16)))

/* The test suite and the CPU restatement of the commit before the cut include this header alone and call
 * aie_build_params, aie_mlp_row and the rest; they are run against this library as they stand, so for host C that
 * reaches this header without having named the builders the other two follow (that suite's plan shim comes in through
 * aie_trainer_plan.h and aie_trainer_math.h, so that way stays open too).  Nothing follows under HIP (the library,
 * hiprtc: no kernel file, run-time unit or cache key sees them), nor behind aie_layout_build.h, which defines
 * AIE_LAYOUT_H_ONLY ahead of including this header: the spec generator compiles no trainer arithmetic. */
#if !defined(__HIPCC__) && !defined(AIE_LAYOUT_H_ONLY)
#include "aie_layout_build.h"
#include "aie_trainer_math.h"
#endif

#endif /* AIE_LAYOUT_H_ */
