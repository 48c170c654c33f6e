// aie_kernels.hip -- hand-written CDNA4 (gfx950) kernels for the batched Foundation env.step() / env.reset() of the
// gather-trade-build family: step_body and reset_body, the step, reset, layout-decide, layout-refill and seed kernels,
// and the two entry points of a run-time specialisation (-DAIE_JIT, at the end).  The device functions they call are in
// four headers without kernels, each of which includes what it uses:
//   aie_gtb_state.h       world helpers, the agents' registers, action decode, the step's change log   <- aie_device.h
//   aie_gtb_components.h  Build, Gather, the auction, taxes, regeneration                              <- aie_gtb_state.h
//   aie_gtb_observe.h     metrics, rewards, map and flat observations, masks, locmap, source list      <- aie_gtb_state.h
//   aie_gtb_layoutgen.h   the four-wave source-layout generator                                        <- aie_device.h
// Components and observation writers do not see each other, the layout generator sees neither, and only this file sees
// all four (tests/test_kernel_sources.py).  The five files are the gather-trade-build UNIT: the library includes this
// file, a run-time specialisation compiles it, and the hashes of all five and of what they include are in the key of
// every cached gather-trade-build code object (aie_jit.h).  What other scenarios and the trainer-side kernels need as
// well is aie_device.h.
//
// Each __device__ function of the family cites the reference function it implements (paths relative to the reference
// tree, F/ = ai_economist/foundation/).
//
// Execution model.  One replica per workgroup, its state record (aie_layout.h) in LDS: the step runs two wavefronts per
// replica (the picture above step_body is the authority), the reset one, or four where it draws a source layout.
//   * the record is streamed HBM -> LDS with 16-byte lane loads; the MT19937 key (624 words) of the wave that twists
//     it goes HBM -> REGISTERS instead (10 VGPRs: lane l of row j holds word 64*j + l),
//   * agent i's scalars (location, inventories, coin, labor, decoded action) live in the registers of lane i of the
//     first wave; "agent j acts next" is a v_readlane broadcast, never an LDS round trip; random agent orders are
//     lane-distributed permutations,
//   * the order book is matched with wave ballots: "best bid of a not-yet-flagged buyer" and "best ask of another
//     agent" are find-first-set over 64 book slots at a time, insertions / removals / expiry compaction are
//     one-instruction lane shifts,
//   * the MT19937 twist is 10 register rows x (3 ds_bpermute + ~10 VALU) with no memory traffic and no barriers;
//     np.random.rand(H, W) is consumed straight from the rows,
//   * observations are written to their dense [E, ...] tensors with lane-contiguous (coalesced) stores, and a step
//     rewrites only what it changed.
// The path is integer / branchy and HBM-bound on the observation writes: no MFMA.
#pragma once
#include "aie_gtb_state.h"
#include "aie_gtb_components.h"
#include "aie_gtb_observe.h"
#include "aie_gtb_layoutgen.h"

// ======================================================================================
// The step
// ======================================================================================

// BaseEnvironment.step, F/base/base_env.py:929-1032: parse actions, timestep += 1,
// components in list order, scenario_step, observations, masks, rewards, done.
//
// A replica is a workgroup of TWO wavefronts sharing the LDS record.
//   both   record HBM -> LDS (alternate 16-byte units;  ||
//          cells: a byte each, expanded -- o_cells8)   ||  wave 1 also: the next 128+ tempered MT19937 words ->
//                                                        ||         the LDS draw window (rows fetched from HBM)
//   wave 0 action decode, price-history decay          ||  wave 1 occupancy map
//   wave 0 components (draws read the draw window)     ||  wave 1 generator rows HBM -> registers, next step's
//                                                      ||         random actions (opt.)
//   wave 0 flat observation vectors, rewards, done     ||  wave 1 regeneration (rows in registers, 4 twists),
//          (none of them looks at the map)             ||         incremental map observations, action masks
//   both   record LDS -> HBM (wave 1 also the generator's rows)
// After the components the two halves touch disjoint state: wave 0 reads agents / auction / tax
// fields and writes util + warm-up counters, wave 1 reads and writes the map cells and the
// generator.  With <= 64 VGPRs all 2 x 4096 waves of the C2 / C3 batch are resident at once (8 per SIMD).
// (Tried and dropped: writing the map observations speculatively during the dynamics and
// repairing the changed cells afterwards -- parity-clean, but the co-resident second waves'
// instruction stream slows the serial dynamics of the first waves by as much as it saves.)

// The three libm tables behind the utilities (aie_glibc_math.h: pow's log and exp tables, log's: 7 KB) touched once per
// workgroup, 64 bytes apart: the step's second wave calls this while the first one runs the components, so that the
// utilities' dependent table look-ups at the end of the step (two or three per pow, each a round trip to wherever the
// streaming traffic has pushed the tables) find them in this CU's vector cache.  Returns a value to keep alive.
__device__ __forceinline__ uint32_t glibc_tables_touch(int lane) {
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int line = 2 * lane + k;  // 112 lines of 64 bytes
    const uint8_t* p = line < 48 ? reinterpret_cast<const uint8_t*>(aie_glibc_powlog_tab) + 64 * line
                     : line < 80 ? reinterpret_cast<const uint8_t*>(aie_glibc_exp_tab) + 64 * (line - 48)
                                 : reinterpret_cast<const uint8_t*>(aie_glibc_log_tab) + 64 * (line - 80);
    if (line < 112) v ^= *reinterpret_cast<const volatile uint32_t*>(p);
  }
  return v;
}

// rewards of the step (compute_reward, layout_from_file.py:519-559), the reward log's slot, `done` and the completed-episode
// count: one wave
// (emit / close: the halves of a split tail, include/aie.h AIE_STEP_EMIT / AIE_STEP_CLOSE -- both true in a whole step.  EMIT
// alone computes the rewards into the arena and claims nothing; CLOSE alone fills the slot from the arena's rewards as
// they stand, which the host may have edited in between)
__device__ __forceinline__ void step_rewards_and_done(const aie::Ctx& c, uint8_t* __restrict__ arena, const NextActions& next, int skip,
                                                      bool emit = true, bool close = true) {
  using namespace aie;
  float* const rew_log = close ? rew_log_claim(c.R, R_I32(c, o_rew_slot), R_I32(c, o_rew_epoch), c.R.E, c.P.n, c.tid == 0) : nullptr;
  if (emit) {
    if (!(skip & AIE_DEV_SKIP_REWARDS)) compute_rewards(c, arena, rew_log);
  } else if (rew_log && c.tid <= c.P.n) {
    const int n = c.P.n, i = c.tid;
    rew_log[(int64_t)c.e * (n + 2) + i] = i < n ? reinterpret_cast<const float*>(arena + c.R.a_rew_a)[(int64_t)c.e * n + i]
                                                : reinterpret_cast<const float*>(arena + c.R.a_rew_p)[c.e];
  }
  AIE_WSYNC();
  if (close && c.tid == 0) {
    const int done = *R_I32(c, o_timestep) >= c.R.c.episode_length;
    (arena + c.R.a_done)[c.e] = (uint8_t)done;
    if (rew_log) rew_log[(int64_t)c.e * (c.P.n + 2) + c.P.n + 1] = done ? 1.0f : 0.0f;
    if (done) *R_I32(c, o_completions) += 1;
  }
}
// SPEC >= 0: a compile-time instance (aie_spec_generated.h): P is a constant image of the parameter block of one
// configuration -- every dimension, record offset, component list, mask table and magic divisor folds into the
// instruction stream (no scalar loads of parameters, fully unrolled per-agent loops) -- and only what depends on
// the batch (R: E, arena offsets) is read at run time.  SPEC < 0: the generic kernel, P == R == *params.
template <bool LOG, int SPEC = -1, bool TRACE = LOG>
__device__ __forceinline__ void step_body(const aie_params* __restrict__ params, uint8_t* __restrict__ arena,
                                          const int32_t* __restrict__ act_a, const int32_t* __restrict__ act_p,
                                          uint8_t* lds, const NextActions& next) {
  using namespace aie;
  // The parameter block lives in device memory (uniform scalar loads).  Passing the 2.7 KB
  // struct by value made the compiler copy it to scratch on every launch (5x slower).
  // (round 6: requesting every kernel argument in one batch up here cost 2 us -- scalar-cache misses are served one at a
  // time, and most arguments are not needed before the record is on its way; see the sampler for the opposite case)
  const aie_params& R = *params;
  const aie_params& P = aie_spec_params<SPEC>(params);
  const int wid = uni((int)(threadIdx.x >> 6));
#ifdef AIE_DEV  // phases switched off by aie_dev_set_skip_mask (the generic kernel with hooks and the traced instances)
  const int skip = (LOG || TRACE) ? R.dev_skip_mask : 0;
#else
  const int skip = 0;
#endif
  const int e_blk = replica_of_block((int)blockIdx.x, next.E);  // (the replica count travels as a kernel argument)
  if (next.e_hi > 0 && (e_blk < next.e_lo || e_blk >= next.e_hi)) return;  // (uniform over the workgroup, ahead of every barrier)
  if (LOG && next.mask && !next.mask[e_blk]) return;  // (likewise: a replica outside an aie_step_range mask, as in reset_body)
  const bool FAST = rng_fast(P);  // the counter stream (include/aie.h: AIE_RNG_FAST); compile-time in the instances
  const int tid0 = (int)(threadIdx.x & (AIE_NT - 1));
  uint8_t* grec = arena + (int64_t)e_blk * P.rec_bytes;  // (a_records == 0: the records open the arena, aie_layout.h)
  uint32_t* gkey = reinterpret_cast<uint32_t*>(grec + P.o_mt);
  const Ctx c = make_ctx(P, R, lds, e_blk, tid0, arena, LOG, skip,
                         /*lds_tables=*/SPEC >= 0);  // (the generic kernel keeps the parameter block's arrays: a pointer
                                                     // that may be LDS or global at run time costs it flat accesses and spills)
  const bool SHL = shared_src_list(P);  // one list of source doubles for the whole batch (a_src_list)
  uint32_t* const draw_w = reinterpret_cast<uint32_t*>(c.stage);  // the components' draw window (LDS)
  int draw_cap = stage_window_words(P);
  if (LOG && R.dev_draw_window > 0 && R.dev_draw_window < draw_cap) draw_cap = R.dev_draw_window;  // tests: force refills
  // With many agents the first wave's tail (flat vectors of every agent, utilities) is the longer one: it then keeps a
  // priority above the waves that are still loading (measured at 10 agents: 42.3 -> 41.9 us; at 4 agents any
  // priority above 0 costs 0.8-1.4 us)
  const int w0_tail_prio = P.n >= 8 ? 2 : 0;
  // Where the rewards run.  With MT19937 the second wave's tail (four twists of regeneration, map observations, masks) is
  // as long as the first wave's (flat vectors, rewards); with the counter stream the regeneration shrinks to a few Philox
  // blocks and the first wave's tail is the long pole (tools/block_trace.py: 7.1 us against 3.7 us), so the rewards move
  // behind the masks on the second wave -- up to 7 agents (A/B on one box, tools/ab_variants.sh: C2f 22.1 -> 21.7 us; with
  // ten agents the utilities' n^2 gini terms make them the longer piece: C3f 35.3 -> 37.4 us, so they stay where they
  // were).  They share no scratch slot with the flat-vector writer (current_metrics).
  const bool REW_ON_W1 = FAST && P.n < 8;
  // partial steps (aie_step_range): compile-time "whole step" everywhere but in the full-featured kernel
  const int ph = LOG ? next.phase : 0;
  const bool HEAD = ph == 0 || (ph & 1), TAIL = ph == 0 || (ph & 2), OBSERVE = ph != 0 && (ph & 4) && !(ph & 2);
  const bool REBASE = OBSERVE && (ph & 8);  // utilities := current (the reward baseline a reset leaves, layout_from_file.py:347-349)
  const bool RETAX = OBSERVE && (ph & 16);  // PeriodicBracketTax's reset-time snapshot of the agents' coin (redistribution.py:1106-1110)
  // the split tail (AIE_STEP_REGEN / EMIT / CLOSE): TAIL is all three
  const bool REGEN = TAIL || (ph & 64), EMIT = TAIL || (ph & 128), CLOSE = TAIL || (ph & 256);
  const bool CLOSE_ONLY = CLOSE && !EMIT;  // (aie_step_range: then without HEAD, REGEN or components -- the state stays as it is)
  const int c_lo = ph ? next.comp_lo : 0, c_hi = ph ? next.comp_hi : P.c.n_components;
  // A compile-time instance knows its component list, so its component loop is unrolled in full: each component then
  // stands once in straight-line code.  Left as a loop around the switch, the compiler turns it into a state machine and
  // hoists every lane mask and address that two components share out of it -- 22 scalar values that did not fit the 80
  // scalar registers a wave has at 8 waves per SIMD and were parked in the lanes of a vector register, which in turn
  // pushed three vector dwords to scratch.  The generic kernels (run-time bounds) keep the loop.
  constexpr int COMP_UNROLL = (SPEC >= 0 && !LOG) ? AIE_MAX_COMPONENTS : 1;
  // The two waves run two separate ARMS from here to the end, each with its own copy of the four workgroup barriers
  // (the branch is wave-uniform, every wave passes the same number of them): a value that only one wave carries --
  // the agents' registers and the draw cache of the first, the generator's ten rows of the second -- is then live in
  // its own arm only and does not count against the other wave's code in the 64-register budget.
  if (wid == 0) {
    // ---------------- first wave: actions, components, flat vectors, rewards ----------------
    Agents A;
    A.hist_dirty = 0;
    A.tax_dirty = false;
    int act_err = 0;
    // Everything this wave fetches ahead of barrier (2) is asked for before anything is waited for: a lane's action
    // word and planner word (action_words_request), its unit of the record and its plane dwords -- or, without the
    // plane, its first three units (load_record_step_request).  The decode waits for the two words alone, the loads
    // behind them stay in flight under it; then the LDS writes.
    // (profiles/prologue_loads_ab.txt, one MI355X, 4096 replicas: decode_actions' two load-wait-decode rounds and then
    // the record batch, 19.37 us per launch; both action words at once, ahead of the record batch, 18.96; everything in
    // one batch, as here, 18.89.  Round 6 had measured the opposite -- 22.5 -> 23.5 us, milder orders 22.7 and 22.9 --
    // on the word-per-cell image of 4.3 KB, whose copy was a loop of load, wait, LDS write per unit; with the loads of a
    // lane in flight together the same holds without the plane: ten agents 35.66 -> 35.16 us.)
    ActionWords aw = {0, 0, false};
    if (!(skip & AIE_DEV_SKIP_ACTION_DECODE)) aw = action_words_request(c, act_a, act_p, arena);
    const RecordIn rin = load_record_step_request(c, arena, 0, 2);
    if (!(skip & AIE_DEV_SKIP_ACTION_DECODE)) act_err = decode_actions(c, A, act_a, act_p, arena, &aw);  // (c.act_p is LDS scratch)
    else A.act = 0;
    if (TRACE && R.dev_trace && c.tid == 0) R.dev_trace[12 * blockIdx.x] = wall_clock64();
    if (TRACE && R.dev_trace && c.tid == 0) R.dev_trace[12 * blockIdx.x + 9] = wall_clock64();
    load_record_step_commit(c, arena, 2, rin);
    __syncthreads();  // (2) the record is in LDS
    // (the cells came as bytes, aie_gtb_state.h: load_record_step_request -- unless something outside the kernels touched the
    // state: then both waves fetch the words, and a change log that starts out overflowed makes the way out write every
    // cell and the whole plane.  Uniform over the workgroup: nobody writes obs_valid before barrier (4).)
    const bool cells_stale = P.o_cells8 != 0 && uni(*R_I32(c, o_obs_valid)) == 0;
    if (cells_stale) {
      load_record_cells(c, arena, 0, 2);
      __syncthreads();
    }
    if (TRACE && R.dev_trace && c.tid == 0) R.dev_trace[12 * blockIdx.x + 8] = wall_clock64();
    MTL ml{draw_w, 0, 0u, -AIE_MT_N, cells_stale ? AIE_DIRTY_CAP + 1 : 0, 0u, 0u, 0, 0, 0, FAST ? reinterpret_cast<uint32_t*>(c.rec + P.o_mt) : gkey, draw_cap, FAST};
    ml.pos = ml.base = uni(*R_I32(c, o_mt_pos));
    ml.avail = ml.cap < AIE_MT_N - ml.pos ? ml.cap : AIE_MT_N - ml.pos;  // what the second wave's draw_window_publish left
    if (FAST) {  // (draw_window_publish_fast: whole pairs, one word less when the position is odd)
      const int covered = 128 * ((ml.cap + 127) >> 7) - (ml.pos & 1);
      if (ml.avail > covered) ml.avail = covered;
    }
    agents_load(c, A);
    // The flat vectors are updated in place (update_flat_observations) on a whole step whose tensors still show the
    // previous step -- the rule of the map observations and the masks.  obs_valid is read HERE, while the image is
    // fresh: the second wave rewrites the field in its tail, which runs beside this wave's.
#ifdef AIE_FLAT_FULL  // (A/B builds: every step rewrites the vectors in full, as before round 7)
    const bool flat_in_place = false;
#else
    const bool flat_in_place = ph == 0 && uni(*R_I32(c, o_obs_valid)) != 0 && !(skip & AIE_DEV_FLAT_FULL);
#endif
    if (act_err && c.tid == 0) *R_I32(c, o_error_flags) |= act_err;
    bool cda_in_range = ph == 0;  // (the decay opens ContinuousDoubleAuction.component_step: with the component)
    if (ph != 0)
      for (int k = c_lo; k < c_hi; ++k) cda_in_range |= P.c.components[k] == AIE_COMP_CDA;
    if (P.has_cda && !(skip & AIE_DEV_SKIP_COMPONENTS) && cda_in_range) cda_decay_price_history(c);
    __syncthreads();  // (3) occupancy map rebuilt
    if (c.tid == 0 && HEAD) *R_I32(c, o_timestep) += 1;
    if (c.ev && c.tid == 0) c.srcn[2] = 0;
    __builtin_amdgcn_s_setprio(3);  // the serial dynamics are the replica's critical path (at any batch size: round 6 A/B)
    if (TRACE && R.dev_trace && c.tid == 0) R.dev_trace[12 * blockIdx.x + 1] = wall_clock64();
    if (!(skip & AIE_DEV_SKIP_COMPONENTS)) {
#pragma unroll COMP_UNROLL
      for (int k = c_lo; k < c_hi; ++k) {
        switch (P.c.components[k]) {
          case AIE_COMP_BUILD: if (!(skip & AIE_DEV_SKIP_BUILD)) build_component_step(c, ml, A); break;
          case AIE_COMP_CDA: if (!(skip & AIE_DEV_SKIP_CDA)) cda_component_step(c, A); break;
          case AIE_COMP_GATHER: if (!(skip & AIE_DEV_SKIP_GATHER)) gather_component_step(c, ml, A); break;
          case AIE_COMP_TAX: if (!(skip & AIE_DEV_SKIP_TAX)) tax_component_step(c, ml, A); break;
          case AIE_COMP_WEALTH_REDISTRIBUTION: wealth_component_step(c, A); break;
          default: break;
        }
        if (TRACE && R.dev_trace && c.tid == 0 && k < 4) R.dev_trace[12 * blockIdx.x + 2 + k] = wall_clock64();
      }
    }
    __builtin_amdgcn_s_setprio(0);
    agents_store(c, A);
    if (c.ev && c.tid == 0) c.ev[0] = c.srcn[2];
    if (c.tid == 0) {
      *R_I32(c, o_mt_pos) = ml.pos;
      c.dirty[0] = ml.dn;
      c.dirty[1] = (int32_t)ml.mv0;
      c.dirty[2] = (int32_t)ml.mv1;
      c.dirty[3] = ml.tw;
    }
    if (TRACE && R.dev_trace && c.tid == 0) R.dev_trace[12 * blockIdx.x + 5] = wall_clock64();
    __syncthreads();  // (4) components done; the generator's position (and, after a refill that twisted, its state in HBM) is final
    // flat observation vectors and rewards: neither looks at the map
    if (w0_tail_prio) __builtin_amdgcn_s_setprio(2);
    if (RETAX && P.has_tax) {  // (ahead of the flat observations: the marginal rate they show is measured from the snapshot)
      if (c.tid < P.n) R_F64(c, o_tax_last_coin)[c.tid] = R_F64(c, o_inv_coin)[c.tid] + R_F64(c, o_esc_coin)[c.tid];
      AIE_WSYNC();
    }
    if (!(skip & AIE_DEV_SKIP_FLAT_AND_MASKS) && (EMIT || OBSERVE)) {
      // An annealed tax schedule caps the rates by the completions count the reset latches BEHIND its own observations
      // (reset_body: o_tax_last_completions, generate_masks' order): the episode's first step shows new curr_rates
      // although no tax day has passed.
      const bool annealed_first = P.has_tax && P.c.tax_annealing && uni(*R_I32(c, o_timestep)) == 1;
      if (flat_in_place && !A.tax_dirty && !annealed_first) update_flat_observations(c, arena, A.hist_dirty);
      else write_flat_observations(c, arena);
    }
    if (TRACE && R.dev_trace && c.tid == 0) R.dev_trace[12 * blockIdx.x + 10] = wall_clock64();
    if (!REW_ON_W1 && (EMIT || CLOSE)) step_rewards_and_done(c, arena, next, skip, EMIT, CLOSE);
    if (REBASE) {  // (reset_body's last lines: the metrics of the state as the host's reset hooks left it)
      AIE_WSYNC();
      current_metrics(c);
      AIE_WSYNC();
      if (c.tid <= P.n) R_F64(c, o_util)[c.tid] = scr_part(c)[c.tid];
      AIE_WSYNC();
    }
    if (w0_tail_prio) __builtin_amdgcn_s_setprio(0);
    __syncthreads();  // (5)
    if (!(skip & AIE_DEV_SKIP_RECORD_STORE)) store_record_step(c, arena, 0, 2);
    if (TRACE && R.dev_trace && c.tid == 0) R.dev_trace[12 * blockIdx.x + 7] = wall_clock64();
  } else {
    // ---------------- second wave: generator, occupancy map, regeneration, map observations, masks ----------------
    MT m;
    mt_init(m, P);
    const int gpos = *reinterpret_cast<const int32_t*>(grec + P.o_mt_pos);
    // Everything this wave fetches ahead of barrier (2) is asked for before anything is waited for: its unit of the
    // record and a lane's first entry of the two small constant tables (Ctx.rtab / mtab -> LDS) at once, then -- they
    // hang on the position, a scalar load -- the words the components will draw (up to three rows of the generator's
    // state; the state itself follows while the components run).  One wait, then the LDS writes.
    const bool TABS = SPEC >= 0 && const_tables_in_lds(P);
    const bool RATES = TABS && P.has_tax && P.c.tax_model == AIE_TAX_MODEL_WRAPPER;
    const bool ROWS = !FAST && !(skip & AIE_DEV_SKIP_DRAW_WINDOW);  // (development: the load phase without the draw window)
    const RecordIn rin = load_record_step_request(c, arena, 1, 2);
    double rate0 = 0.0;
    uint32_t mask0 = 0u;
    if (RATES && c.tid < P.c.tax_n_disc_rates) rate0 = R.c.tax_disc_rates[c.tid];
    if (TABS && c.tid < P.MA) mask0 = P.mask_test[c.tid];
    DrawRows rows = {{0u, 0u, 0u}};
    if (ROWS) rows = draw_rows_request(draw_cap, gkey, uni(gpos), c.tid);
    load_record_step_commit(c, arena, 2, rin);
    if (ROWS) draw_rows_commit(draw_w, draw_cap, rows, gkey, uni(gpos), c.tid);
    else if (FAST && !(skip & AIE_DEV_SKIP_DRAW_WINDOW))  // (the counter stream: computed, nothing to fetch)
      draw_window_publish_fast(draw_w, draw_cap, (uint32_t)uni((int)gkey[0]), (uint32_t)uni((int)gkey[1]), (uint32_t)uni((int)gkey[2]), uni(gpos), c.tid);
    if (RATES) {
      if (c.tid < P.c.tax_n_disc_rates) const_cast<double*>(c.rtab)[c.tid] = rate0;
      for (int q = c.tid + AIE_NT; q < P.c.tax_n_disc_rates; q += AIE_NT) const_cast<double*>(c.rtab)[q] = R.c.tax_disc_rates[q];
    }
    if (TABS) {
      if (c.tid < P.MA) const_cast<uint32_t*>(c.mtab)[c.tid] = mask0;
      for (int q = c.tid + AIE_NT; q < P.MA; q += AIE_NT) const_cast<uint32_t*>(c.mtab)[q] = P.mask_test[q];
    }
    __syncthreads();  // (2)
    if (P.o_cells8 != 0 && uni(*R_I32(c, o_obs_valid)) == 0) {  // (the first wave's cells_stale)
      load_record_cells(c, arena, 1, 2);
      __syncthreads();
    }
    if (!(skip & AIE_DEV_SKIP_LOCMAP)) rebuild_locmap(c);
    __syncthreads();  // (3)
    // nothing to do until the components are done but the next step's random actions
    SrcList src;
    src.S = 0;
#pragma unroll
    for (int k = 0; k < AIE_SRC_CAP / AIE_NT; ++k) src.d[k] = 0;
    src = SHL ? src_list_from_arena(c, arena) : src_list_from_record(c, arena);  // (the loads ride under the first wave's dynamics)
    // (round 6: six scalar touches here, for the parameter-block lines the two tails read, cost 1.2 us -- this wave is not
    // idle enough to absorb six misses served one at a time; removing a_records / a_metrics from the prologue and sharing
    // one argument line gave 0.2 - 0.3 us each)
    const uint32_t warm = glibc_tables_touch(c.tid);
    // (tried in round 6: all ten rows with the record burst and the window from the registers -- one dependent round trip
    // and 768 redundant bytes less, but 1.7 KB more in the burst every workgroup starts with: C2 23.0 -> 23.5 us)
    if (!FAST && !(skip & AIE_DEV_SKIP_GENERATOR_ROWS)) {  // the generator's rows -> registers (re-read after the barrier if the components twisted the state)
#pragma unroll
      for (int j = 0; j < 9; ++j) m.r[j] = gkey[64 * j + c.tid];
      m.r[9] = c.tid < 48 ? gkey[576 + c.tid] : 0u;
    }
    if ((next.a || next.p) && TAIL) {
      const int per_env = P.n * P.act_a_width + P.act_p_width;
      const int st = uni(*R_I32(c, o_sample_t));  // (the first wave does not touch this field)
      for (int j = c.tid; j < per_env; j += AIE_NT) sample_action_slot(P, next.seed, next.env_offset, (int64_t)st, c.e, j, next.a, next.p);
      if (c.tid == 0) *R_I32(c, o_sample_t) = st + 1;
    }
    asm volatile("" ::"v"(warm));
    __syncthreads();  // (4)
    // resource regeneration (the generator's rows are in this wave's registers), then what depends on the map:
    // incremental map observations, action masks
    // A batch that fits the device in one go (4096 workgroups at 8 waves per SIMD) is a race to the last workgroup's end:
    // from here on this wave is the critical one (the first has slack) and goes ahead of the waves still loading.  A
    // larger batch is a stream of workgroups, bound by the vector pipes: there a raised tail only delays the next
    // workgroups' start (tools/ab2.sh, round 6: 16 384 replicas 74.5 -> 72.8 us without it, 65 536: 318 -> 314 us;
    // 4096: 22.5 -> 23.0 us WITHOUT it).
    if (next.E > 6144) __builtin_amdgcn_s_setprio(0);
    else __builtin_amdgcn_s_setprio(2);
    if (FAST) {  // the stream's state is in the LDS image (the components may have moved it to the next block)
      const uint32_t* st = R_U32(c, o_mt);
      m.fkey = (uint32_t)uni((int)st[0]);
      m.fblk = (uint32_t)uni((int)st[1]);
      m.fsalt = (uint32_t)uni((int)st[2]);
    } else if (uni(c.dirty[3]) != 0) {  // a refill that twisted (components drew past word 623) left the new state in HBM
      mt_rows_from_hbm(m, gkey, c.tid);
    }
    m.pos = uni(*R_I32(c, o_mt_pos));
    if (REGEN) {
      bool rows_in_window = false;  // (a skipped regeneration leaves the window as it was)
      if (!(skip & AIE_DEV_SKIP_REGEN)) rows_in_window = scenario_step_regen(c, m, src);
      if (c.tid == 0) {
        *R_I32(c, o_mt_pos) = m.pos;
        if (FAST) R_U32(c, o_mt)[1] = m.fblk;
      }
      if (!(skip & AIE_DEV_SKIP_RECORD_STORE)) store_generator_rows(c, arena, m, rows_in_window);  // (the rows' registers are free from here on)
    }
    if (TRACE && R.dev_trace && c.tid == 0) R.dev_trace[12 * blockIdx.x + 6] = wall_clock64();
    AIE_WSYNC();
    // (the masks follow the map observations' rule: in place unless something outside the kernels touched the state)
    const bool masks_all = OBSERVE || !uni(*R_I32(c, o_obs_valid)) || (skip & (AIE_DEV_SKIP_MAP_OBS | AIE_DEV_MAP_OBS_FULL)) != 0;
    if (!(skip & AIE_DEV_SKIP_MAP_OBS) && (EMIT || OBSERVE)) {
      // the map observations of the previous step are still in the arena: update them in place,
      // unless something outside the kernels touched the state (obs_valid == 0; an AIE_STEP_OBSERVE launch: always)
      if (uni(*R_I32(c, o_obs_valid)) && !(skip & AIE_DEV_MAP_OBS_FULL) && !OBSERVE) update_spatial_observations(c, arena);
      else write_spatial_observations(c, arena);
      if (c.tid == 0) *R_I32(c, o_obs_valid) = 1;
    } else if (!EMIT && !OBSERVE && !CLOSE_ONLY && c.tid == 0) {
      *R_I32(c, o_obs_valid) = 0;  // a partial step changed the state and wrote no observations: the launch that does starts over
    }
    if (!(skip & AIE_DEV_SKIP_FLAT_AND_MASKS) && (EMIT || OBSERVE)) write_action_masks(c, arena, /*all=*/masks_all);
    if (TRACE && R.dev_trace && c.tid == 0) R.dev_trace[12 * blockIdx.x + 11] = wall_clock64();
    if (REW_ON_W1 && (EMIT || CLOSE)) step_rewards_and_done(c, arena, next, skip, EMIT, CLOSE);
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();  // (5)
    if (!(skip & AIE_DEV_SKIP_RECORD_STORE)) store_record_step(c, arena, 1, 2);
  }
}

#ifndef AIE_JIT  // (a run-time specialisation compiles the two entry points at the end of this file only)
extern "C" __global__ void __launch_bounds__(2 * AIE_NT) __attribute__((amdgpu_waves_per_eu(8, 8)))
aie_step_kernel(const aie_params* __restrict__ params, uint8_t* __restrict__ arena,
                const int32_t* __restrict__ act_a, const int32_t* __restrict__ act_p, NextActions next) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  step_body<false>(params, arena, act_a, act_p, lds, next);
}
// the same kernel for records whose LDS footprint keeps a CU at 12 workgroups or fewer anyway (aie_capi.hip:
// aie_step): 6 waves per SIMD buy 80 VGPRs, i.e. no scratch traffic
extern "C" __global__ void __launch_bounds__(2 * AIE_NT) __attribute__((amdgpu_waves_per_eu(6, 6)))
aie_step_kernel_r6(const aie_params* __restrict__ params, uint8_t* __restrict__ arena,
                   const int32_t* __restrict__ act_a, const int32_t* __restrict__ act_p, NextActions next) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  step_body<false>(params, arena, act_a, act_p, lds, next);
}
// the same step for environments with dense-log replicas (aie_config.dense_log_replicas > 0): records AIE_EV_* rows
extern "C" __global__ void __launch_bounds__(2 * AIE_NT) __attribute__((amdgpu_waves_per_eu(8, 8)))
aie_step_kernel_log(const aie_params* __restrict__ params, uint8_t* __restrict__ arena,
                    const int32_t* __restrict__ act_a, const int32_t* __restrict__ act_p, NextActions next) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  step_body<true>(params, arena, act_a, act_p, lds, next);
}
// compile-time instances for the configurations listed in ai-economist_amd/_specs.py (BASELINE configs[1], [2], ...)
#define AIE_SPEC_WAVES(S) aie_spec_image<S>::waves
template <int SPEC>
__global__ void __launch_bounds__(2 * AIE_NT)
__attribute__((amdgpu_waves_per_eu(AIE_SPEC_WAVES(SPEC), AIE_SPEC_WAVES(SPEC))))
aie_step_kernel_spec(const aie_params* __restrict__ params, uint8_t* __restrict__ arena,
                     const int32_t* __restrict__ act_a, const int32_t* __restrict__ act_p, NextActions next) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  step_body<false, SPEC>(params, arena, act_a, act_p, lds, next);
}
#ifdef AIE_DEV
// development: the compile-time instances with per-workgroup clock stamps (tools/block_trace.py, aie_dev_set_trace)
template <int SPEC>
__global__ void __launch_bounds__(2 * AIE_NT)
__attribute__((amdgpu_waves_per_eu(aie_spec_image<SPEC>::waves, aie_spec_image<SPEC>::waves)))
aie_step_kernel_spec_trace(const aie_params* __restrict__ params, uint8_t* __restrict__ arena,
                           const int32_t* __restrict__ act_a, const int32_t* __restrict__ act_p, NextActions next) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  step_body<false, SPEC, true>(params, arena, act_a, act_p, lds, next);
}
#endif
#endif  // !AIE_JIT

// BaseEnvironment.reset, F/base/base_env.py:852-927, with LayoutFromFile
// reset_starting_layout / reset_agent_states / additional_reset_steps
// (layout_from_file.py:323-370, 564-593) and the component resets (build.py:224-254,
// move.py:193-210, continuous_double_auction.py:643-668, redistribution.py:1109-1139).
// Runs once per episode: the sequential part is executed wave-uniformly out of LDS.
namespace aie {
template <int SPEC, bool LAYOUT = true>  // LAYOUT == false: compiled without the layout generator (fixed layouts only)
__device__ __forceinline__ void reset_body(const aie_params* __restrict__ params, uint8_t* __restrict__ arena,
                                           const uint8_t* __restrict__ mask, int keep_rewards, uint8_t* lds) {
  const aie_params& R = *params;                      // run-time block: replica count, arena offsets
  const aie_params& P = aie_spec_params<SPEC>(params);  // the configuration: a constant image in the instances
  const int e = replica_of_block((int)blockIdx.x, R.E);
  if (mask && !mask[e]) return;
  // One wavefront resets a replica; environments whose reset draws a new source layout (uniform/, quadrant/,
  // multi_zone/) are launched with LG_NW wavefronts per replica: all of them generate the layout, then the first
  // one carries on alone (a barrier only waits for the waves of a workgroup that are still running).
  const int gtid = (int)threadIdx.x, wave = gtid >> 6, nwaves = (int)blockDim.x >> 6;
  const Ctx c = make_ctx(P, R, lds, e, gtid & 63, arena);
  const int n = P.n, HW = P.HW, tid = c.tid;
  if (wave == 0) {
    for (int q = tid; q < (P.met_bytes >> 2); q += AIE_NT) reinterpret_cast<uint32_t*>(C_MET(c))[q] = 0u;  // new episode
    if (c.ev && tid == 0) c.ev[0] = 0;
  }
  MT m;
  mt_init(m, P);
  load_record(c, arena, m, wave, nwaves, wave);  // every wave takes its own copy of the generator's rows
  __syncthreads();
  m.pos = uni(*R_I32(c, o_mt_pos));
  mt_fast_attach(c, m);
  if (LAYOUT && P.c.layout_gen != AIE_LAYOUT_FIXED) {  // a fresh source layout, drawn before anything else of the reset
    if (aie__layout_staged(&P.c)) {
      // the counter-stream mode: this reset's layout is a function of (the replica's stream, resets so far) alone
      // (aie_layout.h: aie_layout_stream) -- already in the staging area if a refill launch came by since the last
      // reset, else drawn here from the same stream; the replica's own stream is not touched either way
      uint32_t st[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) st[k] = (uint32_t)uni((int)R_U32(c, o_mt)[k]);
      const uint64_t tag = aie_layout_tag(st);
      const uint64_t* tags = reinterpret_cast<const uint64_t*>(arena + R.a_layout_tag);
      int32_t* ctl = reinterpret_cast<int32_t*>(arena + R.a_layout_ctl);
      const uint64_t have = tags[e];
      const bool staged = (uint32_t)uni((int)(uint32_t)have) == (uint32_t)tag && (uint32_t)uni((int)(uint32_t)(have >> 32)) == (uint32_t)(tag >> 32);
      __syncthreads();  // (every wave has read the state words before the first one counts the reset)
      if (staged) {
        const uint8_t* sp = arena + R.a_layout_stage + (int64_t)e * R.layout_stage_stride;
        layout_install(c, gtid, LG_NW * AIE_NT, [&](int cell) -> uint32_t { return sp[cell]; });
        __syncthreads();
      } else {
        LgShared* sh = lg_shared(lds + lds_bytes(P), P);
        if (gtid == 0) {
          sh->lhas = 0;
          sh->lcache = 0.0;
        }
        __syncthreads();
        uint32_t ks[2];
        aie_layout_stream(st, ks);
        MT ml;
        mt_init(ml, P);
        ml.fkey = ks[0];
        ml.fblk = 0xffffffffu;
        ml.fsalt = ks[1];
        layout_generate(c, ml, arena, lds + lds_bytes(P), gtid, &sh->lhas, &sh->lcache);
      }
      if (gtid == 0) {
        R_U32(c, o_mt)[3] = st[3] + 1u;  // resets so far
        atomicAdd(&ctl[0], 1);           // one more replica without a staged layout for its coming reset
        atomicAdd(&ctl[staged ? 2 : 3], 1);
      }
    } else {
      layout_generate(c, m, arena, lds + lds_bytes(P), gtid, R_I32(c, o_mt_has_gauss), R_F64(c, o_mt_gauss));
    }
    if (wave != 0) return;
  }
  {  // layout_from_file.py:323-334: resources back on every source block, no houses
    uint32_t* cells = R_CELLS(c);
    for (int q = tid; q < HW; q += AIE_NT) {
      const uint32_t fl = cells[q] >> 24;
      cells[q] = AIE_CELL_PACK((fl & AIE_CELL_STONE_SRC) ? 1 : 0, (fl & AIE_CELL_WOOD_SRC) ? 1 : 0, 0xff, fl);
    }
    if (tid < n) {
      R_I32(c, o_inv_res)[tid] = 0; R_I32(c, o_inv_res)[n + tid] = 0;
      R_I32(c, o_esc_res)[tid] = 0; R_I32(c, o_esc_res)[n + tid] = 0;
      R_F64(c, o_inv_coin)[tid] = c.R.c.starting_agent_coin;
      R_F64(c, o_esc_coin)[tid] = 0;
      R_F64(c, o_labor)[tid] = 0;
      R_I32(c, o_loc_r)[tid] = -1;
      R_I32(c, o_loc_c)[tid] = -1;
      if (!P.has_build) { R_F64(c, o_build_payment)[tid] = 0; R_F64(c, o_build_skill)[tid] = 0; }
      if (!P.has_gather) R_F64(c, o_bonus_gather_prob)[tid] = 0;
    }
    if (P.has_cda) {
      for (int q = tid; q < 2 * P.M; q += AIE_NT) { R_I32(c, o_cda_bids)[q] = 0; R_I32(c, o_cda_asks)[q] = 0; }
      for (int q = tid; q < 2 * n * P.P; q += AIE_NT) {
        R_U8(c, o_cda_bid_hist)[q] = 0; R_U8(c, o_cda_ask_hist)[q] = 0;
        R_F64(c, o_cda_price_history)[q] = 0;
      }
      for (int q = tid; q < 2 * n; q += AIE_NT) R_I32(c, o_cda_n_orders)[q] = 0;
      if (tid < 2) { R_I32(c, o_cda_n_bids)[tid] = 0; R_I32(c, o_cda_n_asks)[tid] = 0; }
    }
  }
  __syncthreads();
  build_src_list(c, arena);  // the regeneration's source doubles of this episode's layout
  if (P.regen_conv) {  // source blocks per d x d window, zero-padded ("same"), once per episode
    const uint8_t* cb = reinterpret_cast<const uint8_t*>(R_CELLS(c));
    for (int q = tid; q < AIE_N_RES * HW; q += AIE_NT) {
      const int rs = q >= HW ? 1 : 0, cell = q - rs * HW, r0 = cell / P.W, c0 = cell - r0 * P.W;
      const int hw = P.c.regen_halfwidth[rs];
      const uint32_t bit = rs ? AIE_CELL_WOOD_SRC : AIE_CELL_STONE_SRC;
      int cnt = 0;
      for (int r = max(r0 - hw, 0); r <= min(r0 + hw, P.H - 1); ++r)
        for (int cc = max(c0 - hw, 0); cc <= min(c0 + hw, P.W - 1); ++cc)
          cnt += (cb[4 * (r * P.W + cc) + 3] & bit) ? 1 : 0;
      R_U8(c, o_regen_count)[q] = (uint8_t)cnt;
    }
  }
  rebuild_locmap(c);  // all agents off the board
  // ---- wave-uniform sequential part (every lane performs the same LDS updates) ----
  *R_I32(c, o_timestep) = 0;
  *R_I32(c, o_error_flags) = 0;
  // layout_from_file.py:360-370 places agents in index order, dynamic_layout.py:420-431
  // (uniform/...) in a random order
  const int place_perm = P.c.reset_random_order ? rng_permutation(m, tid, n) : tid;
  for (int k = 0; k < n; ++k) {
    const int i = bcast(place_perm, k);
    int r = (int)rng_interval(m, tid, (uint32_t)(P.H - 1)), col = (int)rng_interval(m, tid, (uint32_t)(P.W - 1)), tries = 0;
    while (!can_agent_occupy(c, r, col, i)) {
      r = (int)rng_interval(m, tid, (uint32_t)(P.H - 1));
      col = (int)rng_interval(m, tid, (uint32_t)(P.W - 1));
      if (++tries > 200) {  // the reference raises TimeoutError (layout_from_file.py:366-368): flagged, see AIE_ERR_*
        *R_I32(c, o_error_flags) |= AIE_ERR_RESET_PLACEMENT;
        break;
      }
    }
    R_I32(c, o_loc_r)[i] = r;
    R_I32(c, o_loc_c)[i] = col;
    c.locmap[r * P.W + col] = (uint8_t)(i + 1);
  }
  for (int k = 0; k < P.c.n_components; ++k) {
    switch (P.c.components[k]) {
      case AIE_COMP_BUILD:
        for (int i = 0; i < n; ++i) {
          double skill = 1, pay = 1;
          const double pm = (double)c.R.c.build_payment_max_skill_multiplier;
          if (P.c.build_skill_dist == AIE_SKILL_PARETO) {
            skill = rng_pareto(m, tid, 4.0);
            pay = (pm - 1) * skill + 1; if (pm < pay) pay = pm;
          } else if (P.c.build_skill_dist == AIE_SKILL_LOGNORMAL) {
            skill = rng_lognormal(c, m, -1.0, 0.5);
            pay = (pm - 1) * skill + 1; if (pm < pay) pay = pm;
          }
          R_F64(c, o_build_payment)[i] = pay * (double)c.R.c.build_payment;
          R_F64(c, o_build_skill)[i] = skill;
        }
        break;
      case AIE_COMP_GATHER:
        for (int i = 0; i < n; ++i) {
          double b = 0.0;
          if (P.c.gather_skill_dist == AIE_SKILL_PARETO) { b = rng_pareto(m, tid, 3.0); b = (b < 2 ? b : 2) / 2; }
          else if (P.c.gather_skill_dist == AIE_SKILL_LOGNORMAL) { b = rng_lognormal(c, m, -2.022, 0.938); b = (b < 2 ? b : 2) / 2; }
          R_F64(c, o_bonus_gather_prob)[i] = b;
        }
        break;
      case AIE_COMP_TAX:
        for (int b = 0; b < P.NB; ++b) R_I32(c, o_tax_rate_idx)[b] = 0;
        *R_I32(c, o_tax_cycle_pos) = 1;
        for (int i = 0; i < n; ++i) {
          R_F64(c, o_tax_last_coin)[i] = R_F64(c, o_inv_coin)[i] + R_F64(c, o_esc_coin)[i];
          R_F64(c, o_tax_last_income)[i] = 0;
          R_F64(c, o_tax_last_marginal_rate)[i] = 0;
        }
        *R_F64(c, o_tax_total_collected) = 0;
        if (P.c.tax_model == AIE_TAX_SAEZ) {
          // _curr_rates_obs first (:1123, still the previous episode's rates), then
          // curr_bracket_tax_rates = running_avg_tax_rates (:1136-1137)
          for (int b = 0; b < P.NB; ++b) R_F64(c, o_tax_saez_obs_rates)[b] = tax_rate(c, b);
          AIE_WSYNC();
          for (int b = 0; b < P.NB; ++b)
            R_F64(c, o_tax_saez_rates)[b] = reinterpret_cast<const double*>(saez_block(c) + AIE_SAEZ_OFF_AVG)[b];
        }
        break;
      default: break;
    }
  }
  if (P.c.fixed_four_skill_and_loc) {  // layout_from_file.py:582-586
    for (int i = 0; i < n; ++i) {
      c.locmap[R_I32(c, o_loc_r)[i] * P.W + R_I32(c, o_loc_c)[i]] = 0;
      R_I32(c, o_loc_r)[i] = -1;
      R_I32(c, o_loc_c)[i] = -1;
    }
    const int perm = rng_permutation(m, tid, n);
    for (int k = 0; k < n; ++k) {
      const int i = bcast(perm, k);
      const int r = c.R.c.ranked_locs[k][0], col = c.R.c.ranked_locs[k][1];
      if (can_agent_occupy(c, r, col, i)) {
        R_I32(c, o_loc_r)[i] = r;
        R_I32(c, o_loc_c)[i] = col;
        c.locmap[r * P.W + col] = (uint8_t)(i + 1);
      }
      R_F64(c, o_build_payment)[i] = c.R.c.avg_ranked_skill[k];
    }
  }
  if (P.c.split_water_line > 0) {  // SplitLayout.additional_reset_steps layout_from_file.py:759-793
    for (int i = 0; i < n; ++i) {
      c.locmap[R_I32(c, o_loc_r)[i] * P.W + R_I32(c, o_loc_c)[i]] = 0;
      R_I32(c, o_loc_r)[i] = -1;
      R_I32(c, o_loc_c)[i] = -1;
    }
    const int perm = rng_permutation(m, tid, n);
    const int wl = P.c.split_water_line;
    for (int k = 0; k < n; ++k) {
      const int i = bcast(perm, k);
      R_F64(c, o_build_payment)[i] = c.R.c.avg_ranked_skill[k];
      const bool top = (c.R.c.split_top_ranks[k >> 5] >> (k & 31)) & 1u;
      const int r_min = top ? 0 : wl + 1, r_max = top ? wl : P.H;
      int r = r_min + (int)rng_interval(m, tid, (uint32_t)(r_max - r_min - 1));
      int col = (int)rng_interval(m, tid, (uint32_t)(P.W - 1)), tries = 0;
      while (!can_agent_occupy(c, r, col, i)) {
        r = r_min + (int)rng_interval(m, tid, (uint32_t)(r_max - r_min - 1));
        col = (int)rng_interval(m, tid, (uint32_t)(P.W - 1));
        if (++tries > 200) {  // the reference raises TimeoutError
          *R_I32(c, o_error_flags) |= AIE_ERR_RESET_PLACEMENT;
          break;
        }
      }
      R_I32(c, o_loc_r)[i] = r;
      R_I32(c, o_loc_c)[i] = col;
      c.locmap[r * P.W + col] = (uint8_t)(i + 1);
    }
  }
  *R_I32(c, o_mt_pos) = m.pos;
  mt_fast_detach(c, m);
  __syncthreads();
  current_metrics(c);
  __syncthreads();
  if (tid <= n) R_F64(c, o_util)[tid] = scr_part(c)[tid];
  __syncthreads();
  write_spatial_observations(c, arena);
  if (tid == 0) *R_I32(c, o_obs_valid) = 1;
  write_flat_observations(c, arena);
  AIE_WSYNC();
  if (P.has_tax && P.c.tax_annealing && tid == 0) *R_I32(c, o_tax_last_completions) = *R_I32(c, o_completions);  // generate_masks :1036-1046
  AIE_WSYNC();
  write_action_masks(c, arena);
  if (!keep_rewards) {  // (auto-reset right behind the step that ended the episode: its rewards / done stay)
    if (tid < n) reinterpret_cast<float*>(arena + R.a_rew_a)[(int64_t)e * n + tid] = 0.0f;
    if (tid == 0) {
      reinterpret_cast<float*>(arena + R.a_rew_p)[e] = 0.0f;
      (arena + R.a_done)[e] = 0;
    }
  }
  __syncthreads();
  store_record(c, arena, m);
  if (P.o_cells8) store_cells8(c, arena);  // the plane goes with the words it is derived from
}
}  // namespace aie

#ifndef AIE_JIT
extern "C" __global__ void __launch_bounds__(AIE_NT)
aie_reset_kernel(const aie_params* __restrict__ params, uint8_t* __restrict__ arena,
                 const uint8_t* __restrict__ mask, int keep_rewards) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  aie::reset_body<-1, false>(params, arena, mask, keep_rewards, lds);
}
// environments whose reset draws a new source layout (uniform/, quadrant/, multi_zone/): LG_NW wavefronts per replica
extern "C" __global__ void __launch_bounds__(LG_NW * AIE_NT)
aie_reset_kernel_layout(const aie_params* __restrict__ params, uint8_t* __restrict__ arena,
                        const uint8_t* __restrict__ mask, int keep_rewards) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  aie::reset_body<-1, true>(params, arena, mask, keep_rewards, lds);
}
// Generated layouts in the counter-stream mode, ahead of their resets (aie_layout.h: a_layout_stage).  Behind every reset
// launch: one thread decides whether a refill pays -- a refill launch lasts as long as its slowest replica (0.3 ms at
// BASELINE configs[0]'s scenario, 1 - 10 tries of the coverage check) however many layouts it draws, so it waits until
// `threshold` replicas have used theirs up (a de-phased rollout resets 2 % of the replicas per launch: one 0.3 ms
// chain per ~12 reset launches instead of one in each) -- then every replica whose coming reset has no staged layout
// yet draws it.  Replicas that reset twice between two refills draw the second layout inside the reset, as before:
// the layout is the same function of (stream, resets so far) wherever it is drawn.
extern "C" __global__ void aie_layout_decide_kernel(const aie_params* __restrict__ params, uint8_t* __restrict__ arena, int threshold) {
  int32_t* ctl = reinterpret_cast<int32_t*>(arena + params->a_layout_ctl);
  const bool go = ctl[0] >= threshold;
  ctl[1] = go ? 1 : 0;
  if (go) ctl[0] = 0;
}
extern "C" __global__ void __launch_bounds__(LG_NW * AIE_NT)
aie_layout_refill_kernel(const aie_params* __restrict__ params, uint8_t* __restrict__ arena) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const aie_params& P = *params;
  const int32_t* ctl = reinterpret_cast<const int32_t*>(arena + P.a_layout_ctl);
  if (!ctl[1]) return;
  const int e = (int)blockIdx.x, gtid = (int)threadIdx.x;
  const uint32_t* stg = reinterpret_cast<const uint32_t*>(arena + P.a_records + (int64_t)e * P.rec_bytes + P.o_mt);
  uint32_t st[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) st[k] = (uint32_t)aie::uni((int)stg[k]);
  const uint64_t tag = aie_layout_tag(st);
  uint64_t* tags = reinterpret_cast<uint64_t*>(arena + P.a_layout_tag);
  const uint64_t have = tags[e];
  if ((uint32_t)aie::uni((int)(uint32_t)have) == (uint32_t)tag && (uint32_t)aie::uni((int)(uint32_t)(have >> 32)) == (uint32_t)(tag >> 32)) return;
  const aie::Ctx c = aie::make_ctx(P, P, lds, e, gtid & 63, arena);
  aie::LgShared* sh = aie::lg_shared(lds + aie::lds_bytes(P), P);
  if (gtid == 0) {
    sh->lhas = 0;
    sh->lcache = 0.0;
  }
  __syncthreads();
  uint32_t ks[2];
  aie_layout_stream(st, ks);
  aie::MT ml;
  aie::mt_init(ml, P);
  ml.fkey = ks[0];
  ml.fblk = 0xffffffffu;
  ml.fsalt = ks[1];
  aie::layout_generate(c, ml, arena, lds + aie::lds_bytes(P), gtid, &sh->lhas, &sh->lcache,
                       arena + P.a_layout_stage + (int64_t)e * P.layout_stage_stride);
  if (gtid == 0) tags[e] = tag;  // (behind layout_generate's closing barrier: the staged bytes are written)
}
// compile-time instances (aie_spec_generated.h), as for the step kernel
template <int SPEC>
__global__ void __launch_bounds__(LG_NW * AIE_NT)
aie_reset_kernel_spec(const aie_params* __restrict__ params, uint8_t* __restrict__ arena,
                      const uint8_t* __restrict__ mask, int keep_rewards) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  aie::reset_body<SPEC>(params, arena, mask, keep_rewards, lds);
}

// np.random.seed(base_seed + e): init_genrand (Knuth LCG), pos = 624.
// BaseEnvironment.seed, F/base/base_env.py:481-494.  One thread per replica.
// AIE_RNG_FAST (aie_seed_fast; aie_seed with base_seed < 2^32): the counter stream keyed by base_seed + e (48 bits): key32,
// block number 0 with pos = 624 (the first draw opens block 1), salt.
extern "C" __global__ void aie_seed_kernel(const aie_params P, uint8_t* __restrict__ arena, uint64_t base_seed) {
  const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (e >= P.E) return;
  uint8_t* rec = arena + P.a_records + (int64_t)e * P.rec_bytes;
  uint32_t* mt = reinterpret_cast<uint32_t*>(rec + P.o_mt);
  if (aie::rng_fast(P)) {
    const uint64_t s = base_seed + (uint64_t)e;
    mt[0] = (uint32_t)s;
    mt[1] = 0u;
    mt[2] = ((uint32_t)(s >> 32) & 0xffffu) << 16;
    mt[3] = 0u;
  } else {
    uint32_t x = (uint32_t)base_seed + (uint32_t)e;
    mt[0] = x;
    for (int i = 1; i < AIE_MT_N; ++i) {
      x = 1812433253u * (x ^ (x >> 30)) + (uint32_t)i;
      mt[i] = x;
    }
  }
  *reinterpret_cast<int32_t*>(rec + P.o_mt_pos) = AIE_MT_N;
  *reinterpret_cast<int32_t*>(rec + P.o_mt_has_gauss) = 0;
  *reinterpret_cast<double*>(rec + P.o_mt_gauss) = 0.0;
}
#endif  // !AIE_JIT

#if defined(AIE_JIT) && !defined(AIE_JIT_OSE)
#ifdef AIE_JIT_PAD_NOPS  // development (AIE_JIT_PAD_NOPS=N in the environment): N no-ops ahead of the kernels shift their
                         // placement in the code object -- does a launch's duration follow where its code lies?
extern "C" __global__ void aie_jit_pad() {
#define AIE_STR2(x) #x
#define AIE_STR(x) AIE_STR2(x)
  asm volatile(".rept " AIE_STR(AIE_JIT_PAD_NOPS) "\n s_nop 0\n .endr");
}
#endif
// A second caller, never launched, for the out-of-line helpers.  Round 5 found what rounds 2 - 4 could not: a run-time
// instance was 3 - 6 % slower than the build's instance of the same family because in THIS translation unit the helpers
// have one caller each with compile-time arguments (n, the draw window's capacity ...), interprocedural constant
// propagation specialises them, and the kernels' register allocation around the call sites changes with them (16
// instead of 29 spilled VGPRs, 100 more instructions; same compiler, same flags -- hipcc --genco of this file gave
// hiprtc's code byte for byte).  In the build the helpers are shared by every instance and stay generic.  With this
// caller (run-time arguments; np_sum_leaf's mode is 1 at every call site of the build, too) the step and reset kernels
// come out instruction for instruction as the build's (llvm-objdump, tools/jit_gap_experiment.py).
extern "C" __global__ void aie_jit_keep_helpers_generic(const double* a, int n, uint32_t M, int o, int m, uint32_t* gkey,
                                                        uint32_t* w, int cap, int pos, double* out) {
  const int lane = (int)threadIdx.x & 63;
  out[0] = aie::np_sum_leaf(a, n, 1, M, o, m, lane);
  const aie::Refill r = aie::rng_refill(gkey, w, cap, pos, lane);
  const aie::Refill rf = aie::rng_refill_fast(gkey, w, cap, pos, lane);
  out[1] = (double)(r.pos + r.avail + r.twisted + rf.pos + rf.avail + rf.twisted);
  aie::MTRows t;
  for (int j = 0; j < 10; ++j) t.r[j] = gkey[64 * j + lane];
  t = aie::mt_twist_rows(t, lane);
  const aie::MTRows f = aie::mt_fast_rows_of(gkey[0], gkey[1], gkey[2], lane);
  for (int j = 0; j < 10; ++j) gkey[64 * j + lane] = t.r[j] ^ f.r[j];
}
// Run-time specialisation (aie_specialize): the step and reset kernels with THIS environment's parameter block as the
// constant image (aie_jit_image.h is generated per configuration), exactly what the build's compile-time instances
// are for the BASELINE configurations.
extern "C" __global__ void __launch_bounds__(2 * AIE_NT)
__attribute__((amdgpu_waves_per_eu(aie_spec_image<0>::waves, aie_spec_image<0>::waves)))
aie_jit_step(const aie_params* __restrict__ params, uint8_t* __restrict__ arena,
             const int32_t* __restrict__ act_a, const int32_t* __restrict__ act_p, NextActions next) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  step_body<false, 0>(params, arena, act_a, act_p, lds, next);
}
extern "C" __global__ void __launch_bounds__(LG_NW * AIE_NT)
aie_jit_reset(const aie_params* __restrict__ params, uint8_t* __restrict__ arena,
              const uint8_t* __restrict__ mask, int keep_rewards) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  aie::reset_body<0>(params, arena, mask, keep_rewards, lds);
}
#endif  // AIE_JIT
