// aie_kernels.hip -- hand-written CDNA4 (gfx950) kernels for the batched Foundation
// env.step() / env.reset() of the gather-trade-build family.
//
// Execution model: ONE WAVEFRONT (64 lanes) PER ENV REPLICA, one replica per workgroup.
//   * the replica's state record (layout in aie_layout.h) is streamed HBM -> LDS with
//     16-byte lane loads; its MT19937 key (624 words) goes HBM -> REGISTERS instead
//     (10 VGPRs: lane l of row j holds word 64*j + l),
//   * agent i's scalars (location, inventories, coin, labor, decoded action) live in the
//     registers of lane i; "agent j acts next" is a v_readlane broadcast, never an LDS
//     round trip; random agent orders are lane-distributed permutations,
//   * the order book is matched with wave ballots: "best bid of a not-yet-flagged buyer"
//     and "best ask of another agent" are find-first-set over 64 book slots at a time,
//     insertions / removals / expiry compaction are one-instruction lane shifts,
//   * the MT19937 twist is 10 register rows x (3 ds_bpermute + ~10 VALU) with no memory
//     traffic and no barriers; np.random.rand(H, W) is consumed straight from the rows,
//   * observations are written to their dense [E, ...] tensors with lane-contiguous
//     (coalesced) stores; small vectors are staged in LDS and streamed out.
// The path is integer / branchy and HBM-bound on the observation writes: no MFMA.
//
// Each __device__ function cites the reference function it implements (paths relative
// to the reference tree, F/ = ai_economist/foundation/).
//
// This file is the gather-trade-build UNIT: the family's device functions and its step, reset, layout and seed kernels,
// which the library includes and which a run-time specialisation compiles under -DAIE_JIT with the two entry points at
// the end (aie_jit.h: the hashes of this file and of everything it includes are in the key of every cached
// gather-trade-build code object).  What other scenarios and the trainer-side kernels need as well is aie_device.h.
#pragma once
#include "aie_device.h"

namespace aie {
// ------------------------------------------------------------------------------------
// World helpers (F/base/world.py)
// ------------------------------------------------------------------------------------
// World.can_agent_occupy, world.py:424-440: in bounds, no Water, House only if owner
// (world.py:213-217, 256-258, 300-305), and unoccupied.
__device__ __forceinline__ bool can_agent_occupy(const Ctx& c, int r, int col, int agent) {
  if (r < 0 || r >= c.P.H || col < 0 || col >= c.P.W) return false;
  const int cell = r * c.P.W + col;
  const uint32_t w = R_CELLS(c)[cell];
  if (AIE_CELL_FLAGS(w) & AIE_CELL_WATER) return false;
  const int o = AIE_CELL_OWNER(w);
  if (!(o < 0 || o == agent)) return false;
  const int occ = c.locmap[cell];
  return occ == 0 || occ == agent + 1;
}

// Dense-log event of a logged replica (include/aie.h: AIE_EV_*): wave-uniform arguments, lane 0
// writes the row; the per-step row count lives in LDS (c.srcn[2]) until the components are done.
__device__ __forceinline__ void log_event(const Ctx& c, int type, int a1, int a2, int a3, int a4, int a5,
                                          int a6, int a7, int a8, double f) {
  if (c.tid != 0) return;
  const int k = c.srcn[2];
  if (k >= c.R.ev_cap) return;
  int32_t* row = c.ev + 4 + k * AIE_EV_WORDS;
  row[0] = type; row[1] = a1; row[2] = a2; row[3] = a3; row[4] = a4;
  row[5] = a5; row[6] = a6; row[7] = a7; row[8] = a8; row[9] = 0;
  *reinterpret_cast<double*>(row + 10) = f;
  c.srcn[2] = k + 1;
}

// Build.agent_can_build, F/components/build.py:70-83 (+ world.py:284-293)
__device__ __forceinline__ bool agent_can_build(const Ctx& c, int i) {
  const int n = c.P.n;
  const int32_t* inv = R_I32(c, o_inv_res);
  if (inv[n + i] < 1 || inv[i] < 1) return false;
  const uint32_t w = R_CELLS(c)[R_I32(c, o_loc_r)[i] * c.P.W + R_I32(c, o_loc_c)[i]];
  // no resource, no house (owner byte 0xff = none), no water / source block
  return (w & 0xffffu) == 0 && ((w >> 16) & 0xffu) == 0xffu && (w >> 24) == 0;
}

// ------------------------------------------------------------------------------------
// Agent state in registers: lane i < n holds agent i.
// ------------------------------------------------------------------------------------
struct Agents {
  int lr, lc;            // location
  int inv0, inv1;        // Stone, Wood in inventory
  int esc0, esc1;        // Stone, Wood in escrow
  int no0, no1;          // open orders per commodity (CDA n_orders)
  uint32_t act;          // bit 0 build | gather << 1 (3 bits) | buy0 << 4 | sell0 << 11 | buy1 << 18 | sell1 << 25
  double coin, esc_coin, labor;
  // What the step's components did to the slow-moving entries of the flat observation vectors (wave-uniform; zeroed by
  // step_body, read by update_flat_observations -- the record has no such field):
  uint64_t hist_dirty;   // order-count histogram columns that changed (hist_bit)
  bool tax_dirty;        // PeriodicBracketTax latched new rates or enacted taxes in this step
};
// Bit of Agents::hist_dirty for a change of cda_ask_hist (side 0) / cda_bid_hist (side 1) of commodity r at `price`: one
// bit per (commodity, side, price) while those fit one 64-bit word (P <= 16; 44 bits with the default 11 price levels),
// one per (commodity, side) beyond.  hist_col_dirty: the test for one column.
__device__ __forceinline__ uint64_t hist_bit(const aie_params& P, int r, int side, int price) {
  return 4 * P.P <= 64 ? 1ull << ((2 * r + side) * P.P + price) : 1ull << (2 * r + side);
}
__device__ __forceinline__ bool hist_col_dirty(const aie_params& P, uint64_t dirty, int r, int side, int price) {
  return ((dirty >> (4 * P.P <= 64 ? (2 * r + side) * P.P + price : 2 * r + side)) & 1ull) != 0;
}
#define AIE_ACT_BUILD(a) ((a) & 1u)
#define AIE_ACT_GATHER(a) (((a) >> 1) & 7u)
#define AIE_ACT_BUY(a, r) (((a) >> (4 + 14 * (r))) & 0x7fu)
#define AIE_ACT_SELL(a, r) (((a) >> (11 + 14 * (r))) & 0x7fu)

__device__ __forceinline__ void agents_load(const Ctx& c, Agents& A) {
  const int n = c.P.n, i = c.tid < n ? c.tid : 0;
  A.lr = R_I32(c, o_loc_r)[i];
  A.lc = R_I32(c, o_loc_c)[i];
  A.inv0 = R_I32(c, o_inv_res)[i];
  A.inv1 = R_I32(c, o_inv_res)[n + i];
  A.esc0 = R_I32(c, o_esc_res)[i];
  A.esc1 = R_I32(c, o_esc_res)[n + i];
  A.no0 = c.P.has_cda ? R_I32(c, o_cda_n_orders)[i] : 0;
  A.no1 = c.P.has_cda ? R_I32(c, o_cda_n_orders)[n + i] : 0;
  A.coin = R_F64(c, o_inv_coin)[i];
  A.esc_coin = R_F64(c, o_esc_coin)[i];
  A.labor = R_F64(c, o_labor)[i];
}
__device__ __forceinline__ void agents_store(const Ctx& c, const Agents& A) {
  const int n = c.P.n, i = c.tid;
  if (i < n) {
    R_I32(c, o_loc_r)[i] = A.lr;
    R_I32(c, o_loc_c)[i] = A.lc;
    R_I32(c, o_inv_res)[i] = A.inv0;
    R_I32(c, o_inv_res)[n + i] = A.inv1;
    R_I32(c, o_esc_res)[i] = A.esc0;
    R_I32(c, o_esc_res)[n + i] = A.esc1;
    if (c.P.has_cda) {
      R_I32(c, o_cda_n_orders)[i] = A.no0;
      R_I32(c, o_cda_n_orders)[n + i] = A.no1;
    }
    R_F64(c, o_inv_coin)[i] = A.coin;
    R_F64(c, o_esc_coin)[i] = A.esc_coin;
    R_F64(c, o_labor)[i] = A.labor;
  }
}

// parse_actions base_env.py:552-556 -> base_agent.py:407-438: lane i decodes agent i's
// action into its packed per-subspace word; lane b decodes planner bracket b.
// Returns the AIE_ERR_* bits of out-of-range indices (wave-uniform); the caller ORs them into the record's error_flags
// once the record is in LDS -- the action loads themselves leave ahead of it (step_body).
//
// Subspaces of host components (slot AIE_SUB_HOST; the planner's rows hp_*, aie_layout.h) have no place in the packed
// word: in the full-featured kernel (Ctx::full; the only one such an environment runs) lane i stores agent i's foreign
// sub-actions as int32 [n_host_a] into the tensor host_actions_a and lane k the planner's k-th into host_actions_p --
// plain vector stores to the arena, outside the record; without a buffer (aa / ap null: a launch that only observes)
// the tensors keep what the step's first launch wrote.  No other kernel ever runs an environment with such subspaces
// (aie_capi.hip: aie_step_impl sends it to the full-featured kernel, aie_jit_eligible keeps it off the run-time
// instances); elsewhere the decode is the plain one, which leaves foreign slots out of the packed word.
__device__ __forceinline__ int decode_actions(const Ctx& c, Agents& A, const int32_t* __restrict__ aa,
                               const int32_t* __restrict__ ap, uint8_t* __restrict__ arena = nullptr) {
  const aie_params& P = c.P;
  const bool host = c.full && arena;  // (compile-time false in the common step kernel, see Ctx::full)
  const int i = c.tid;
  uint32_t act = 0;
  bool bad_a = false, bad_p = false;  // out-of-range indices: NO-OP here, an exception in the reference (AIE_ERR_*)
  if (i < P.n && aa) {
    const int32_t* a = aa + ((int64_t)c.e * P.n + i) * P.act_a_width;
    static const int shift[AIE_N_SUB_SLOTS] = {0, 4, 11, 18, 25, 1, 0, 0};  // ([AIE_SUB_HOST]: never shifted by, both paths skip the slot)
    int32_t* ha = (host && P.n_host_a) ? reinterpret_cast<int32_t*>(arena + c.R.a_host_act_a) + ((int64_t)c.e * P.n + i) * P.n_host_a : nullptr;
    int h = 0;  // (uniform: the foreign slots so far)
    if (!ha) {
      if (P.c.multi_action_mode_agents) {
        for (int s = 0; s < P.n_sub_a; ++s) {
          const int v = a[s];
          if (v < 0 || v > P.sub_a_dim[s]) bad_a = true;
          else if (P.sub_a_slot[s] != AIE_SUB_HOST) act |= (uint32_t)v << shift[P.sub_a_slot[s]];
        }
      } else {
        const int v = a[0];
        bad_a = v < 0 || v >= P.A;
        for (int s = 0; s < P.n_sub_a; ++s)
          if (P.sub_a_slot[s] != AIE_SUB_HOST && v >= P.sub_a_base[s] && v < P.sub_a_base[s] + P.sub_a_dim[s])
            act |= (uint32_t)(v - P.sub_a_base[s] + 1) << shift[P.sub_a_slot[s]];
      }
    } else if (P.c.multi_action_mode_agents) {
      for (int s = 0; s < P.n_sub_a; ++s) {
        const int v = a[s];
        const bool ok = v >= 0 && v <= P.sub_a_dim[s];
        if (P.sub_a_slot[s] == AIE_SUB_HOST) ha[h++] = ok ? v : 0;
        else if (ok) act |= (uint32_t)v << shift[P.sub_a_slot[s]];
        if (!ok) bad_a = true;
      }
    } else {
      const int v = a[0];
      bad_a = v < 0 || v >= P.A;
      for (int s = 0; s < P.n_sub_a; ++s) {
        const bool in = v >= P.sub_a_base[s] && v < P.sub_a_base[s] + P.sub_a_dim[s];
        if (P.sub_a_slot[s] == AIE_SUB_HOST) ha[h++] = in ? v - P.sub_a_base[s] + 1 : 0;
        else if (in) act |= (uint32_t)(v - P.sub_a_base[s] + 1) << shift[P.sub_a_slot[s]];
      }
    }
  }
  A.act = act;
  if (i < AIE_MAX_BRACKETS) {
    int v = 0;
    if (ap && i < P.n_sub_p) {
      const int32_t* a = ap + (int64_t)c.e * P.act_p_width;
      // (the tax block's first row / first single-action index: 0 / 1 without foreign planner rows ahead of it)
      const int row0 = (host && P.n_host_p) ? P.tax_p_row0 : 0, x0 = (host && P.n_host_p) ? P.tax_p_base : 1;
      if (P.c.multi_action_mode_planner) {
        v = a[row0 + i];
        bad_p = v < 0 || v > P.sub_p_dim;  // (the tax component ignores what its mask forbids; out of range is an error)
        if (bad_p) v = 0;
      } else {
        const int x = a[0];
        bad_p = x < 0 || x >= ((host && P.n_host_p) ? P.AP : 1 + P.n_sub_p * P.sub_p_dim);
        if (x >= x0 && x < x0 + P.n_sub_p * P.sub_p_dim && (x - x0) / P.sub_p_dim == i) v = (x - x0) % P.sub_p_dim + 1;
      }
    }
    c.act_p[i] = v;
  }
  if (host && P.n_host_p && ap && i < P.n_host_p) {  // the planner's foreign rows: lane k decodes row hp_row[k]
    const int32_t* a = ap + (int64_t)c.e * P.act_p_width;
    int v;
    if (P.c.multi_action_mode_planner) {
      v = a[P.hp_row[i]];
      if (v < 0 || v > P.hp_dim[i]) { bad_p = true; v = 0; }
    } else {
      const int x = a[0];
      if (x < 0 || x >= P.AP) bad_p = true;
      v = (x >= P.hp_base[i] && x < P.hp_base[i] + P.hp_dim[i]) ? x - P.hp_base[i] + 1 : 0;
    }
    reinterpret_cast<int32_t*>(arena + c.R.a_host_act_p)[(int64_t)c.e * P.n_host_p + i] = v;
  }
  return (__ballot(bad_a) ? AIE_ERR_AGENT_ACTION : 0) | (__ballot(bad_p) ? AIE_ERR_PLANNER_ACTION : 0);
}

// ------------------------------------------------------------------------------------
// Change log of one step.  The map observations (egocentric crops, planner map: 85 % of a
// step's output bytes) live in the arena from one step to the next, and a step changes only a
// handful of map cells, so the step kernel rewrites just those (update_spatial_observations)
// instead of all of them.  Every map cell whose packed word or occupant changes is appended
// to a short LDS list, every agent that moves gets a bit in the moved mask; a list overflow
// makes the step fall back to the full rewrite.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ uint16_t* dirty_list(const Ctx& c) { return reinterpret_cast<uint16_t*>(c.dirty + 4); }
// wave-uniform call site (all lanes pass the same cell): lane 0 appends
__device__ __forceinline__ void dirty_add_uniform(const Ctx& c, MTL& m, int cell) {
  if (c.tid == 0 && m.dn < AIE_DIRTY_CAP) dirty_list(c)[m.dn] = (uint16_t)cell;
  m.dn += 1;
}
// divergent call site (each active lane its own cell)
__device__ __forceinline__ void dirty_add_lane(const Ctx& c, int cell) {
  const int s = atomicAdd(&c.dirty[0], 1);
  if (s < AIE_DIRTY_CAP) dirty_list(c)[s] = (uint16_t)cell;
}
__device__ __forceinline__ void dirty_agent_moved(MTL& m, int i) {
  if (i < 32) m.mv0 |= 1u << i; else m.mv1 |= 1u << (i - 32);
}
// The step's way out (round 6).  A step changes a handful of the H W map cells -- the ones its change log lists for the
// in-place map observations (dirty_*: every cell whose word or occupant changed) -- so the 16-byte units that hold
// nothing but cells stay as they are in HBM and the listed cells go out one word per lane: 2.4 of the 4.2 KB image of
// BASELINE configs[1] are not written.  A log overflow writes everything.  (The generator's rows left right behind the
// regeneration: store_generator_rows.)
__device__ __forceinline__ void store_record_step(const Ctx& c, uint8_t* __restrict__ arena, int wave, int nwaves) {
  uint8_t* g = arena + (int64_t)c.e * c.P.rec_bytes;
  uint4* dst = reinterpret_cast<uint4*>(g);
  const uint4* src = reinterpret_cast<const uint4*>(c.rec);
  const int nq = rec_lds_bytes(c.P) >> 4;
  const int cnt = uni(c.dirty[0]);
  const int q0 = (c.P.o_cells == 0 && cnt <= AIE_DIRTY_CAP) ? (4 * c.P.HW) >> 4 : 0;  // units [0, q0): cells only
  for (int q = q0 + wave * AIE_NT + c.tid; q < nq; q += nwaves * AIE_NT) dst[q] = src[q];
  if (wave == nwaves - 1 && q0 > 0 && c.tid < cnt) {
    const int cell = (int)dirty_list(c)[c.tid];
    reinterpret_cast<uint32_t*>(g + c.P.o_cells)[cell] = R_CELLS(c)[cell];
  }
}

// ------------------------------------------------------------------------------------
// Build.component_step, F/components/build.py:112-161.  Wave-uniform control flow; the
// builders are found with one ballot, so the common "nobody builds" step costs only the
// permutation draw (which the reference consumes regardless, build.py:121).
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void build_component_step(const Ctx& c, MTL& m, Agents& A) {
  const int n = c.P.n, lane = c.tid;
  const int perm = rng_permutation(m, lane, n);
  const uint64_t builders = __ballot(lane < n && AIE_ACT_BUILD(A.act));
  if (builders == 0) return;
  uint32_t* cells = R_CELLS(c);
  for (int k = 0; k < n; ++k) {
    const int i = bcast(perm, k);
    if (!((builders >> i) & 1ull)) continue;
    // agent_can_build, build.py:70-83 (+ world.py:284-293)
    const int cell = bcast(A.lr, i) * c.P.W + bcast(A.lc, i);
    const uint32_t w = cells[cell];
    const bool ok = bcast(A.inv0, i) >= 1 && bcast(A.inv1, i) >= 1 && (w & 0xffffu) == 0 &&
                    ((w >> 16) & 0xffu) == 0xffu && (w >> 24) == 0;
    if (!ok) continue;
    if (lane == i) {
      A.inv0 -= 1;
      A.inv1 -= 1;
      A.coin += R_F64(c, o_build_payment)[i];
      A.labor += c.R.c.build_labor;
    }
    cells[cell] = (w & 0xff00ffffu) | ((uint32_t)i << 16);  // world.py:474-479 (every lane, same value)
    dirty_add_uniform(c, m, cell);
    if (c.ev) log_event(c, AIE_EV_BUILD, i, cell / c.P.W, cell % c.P.W, 0, 0, 0, 0, 0, R_F64(c, o_build_payment)[i]);
  }
}

// ------------------------------------------------------------------------------------
// Gather.component_step, F/components/move.py:93-153 (wave-uniform control flow)
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void gather_component_step_serial(const Ctx& c, MTL& m, Agents& A) {
  const int n = c.P.n, W = c.P.W, H = c.P.H, lane = c.tid;
  const int perm = rng_permutation(m, lane, n);
  uint32_t* cells = R_CELLS(c);
  const double my_bonus = R_F64(c, o_bonus_gather_prob)[lane < n ? lane : 0];
  for (int k = 0; k < n; ++k) {
    const int i = bcast(perm, k);
    const int a = (int)AIE_ACT_GATHER(bcast(A.act, i));
    const int r = bcast(A.lr, i), col = bcast(A.lc, i);
    int land = r * W + col;
    if (a != 0) {
      // 1 Left, 2 Right, 3 Up, 4 Down (move.py:116-123)
      const int nr = r + (a == 3 ? -1 : a == 4 ? 1 : 0);
      const int nc = col + (a == 1 ? -1 : a == 2 ? 1 : 0);
      if (nr >= 0 && nr < H && nc >= 0 && nc < W) {
        // World.can_agent_occupy, world.py:424-440
        const int tcell = nr * W + nc;
        const uint32_t tw = cells[tcell];
        const int occ = c.locmap[tcell];
        const int own = AIE_CELL_OWNER(tw);
        if (!(AIE_CELL_FLAGS(tw) & AIE_CELL_WATER) && (own < 0 || own == i) && occ == 0) {
          c.locmap[land] = 0;
          c.locmap[tcell] = (uint8_t)(i + 1);
          dirty_add_uniform(c, m, land);
          dirty_add_uniform(c, m, tcell);
          dirty_agent_moved(m, i);
          if (lane == i) {
            A.lr = nr;
            A.lc = nc;
            A.labor += c.R.c.move_labor;
          }
          land = tcell;
        }
      }
    }
    // collect on the landing tile, also on a NO-OP (move.py:112-113,136)
    uint32_t w = cells[land];
    if ((w & 0xffffu) != 0) {
      const int health[2] = {(int)AIE_CELL_STONE(w), (int)AIE_CELL_WOOD(w)};
      const double bonus = bcast(my_bonus, i);
#pragma unroll
      for (int rs = 0; rs < 2; ++rs) {
        if (health[rs] >= 1) {
          // rand() is consumed even when bonus_gather_prob == 0 (move.py:138)
          const int got = 1 + (rng_double(m, lane) < bonus ? 1 : 0);
          if (lane == i) {
            if (rs == 0) A.inv0 += got; else A.inv1 += got;
            A.labor += c.R.c.collect_labor;
          }
          w -= (1u << (8 * rs));  // consume_resource, world.py:481-483
          if (c.ev) log_event(c, AIE_EV_GATHER, i, rs, got, land / W, land % W, 0, 0, 0, 0.0);
        }
      }
      cells[land] = w;
      dirty_add_uniform(c, m, land);
    }
  }
}

__device__ __forceinline__ void gather_component_step_lookahead(const Ctx& c, MTL& m, Agents& A) {
  const int n = c.P.n, W = c.P.W, H = c.P.H, lane = c.tid;
  const int perm = rng_permutation(m, lane, n);
  uint32_t* cells = R_CELLS(c);
  const double my_bonus = R_F64(c, o_bonus_gather_prob)[lane < n ? lane : 0];
  // The reference resolves the agents one after the other, and what agent i sees -- the target tile's cell word and
  // occupancy, then the landing tile's resources -- are two dependent LDS round trips per agent.  Every lane looks
  // its OWN agent's tiles up first (one round trip for all agents), and the serial loop works on broadcasts of those
  // as long as no earlier agent of this step's order moved out of or into the agent's target tile (`stale`: then the
  // agent goes the slow way, through LDS).  Nothing else an earlier agent does is visible to a later one: resources
  // are only taken from the tile an agent stands on, and nobody else can enter that tile.
  int my_tcell = -1;     // target tile of my move, -1: none (NO-OP or out of the world)
  uint32_t my_tw = 0;    // its cell word
  int my_occ = 1;        // its occupant (0: free)
  uint32_t my_ow = 0;    // the cell word of the tile I stand on
  int my_land = 0;
  if (lane < n) {
    const int a = (int)AIE_ACT_GATHER(A.act);
    my_land = A.lr * W + A.lc;
    my_ow = cells[my_land];
    // 1 Left, 2 Right, 3 Up, 4 Down (move.py:116-123)
    const int nr = A.lr + (a == 3 ? -1 : a == 4 ? 1 : 0);
    const int nc = A.lc + (a == 1 ? -1 : a == 2 ? 1 : 0);
    if (a != 0 && nr >= 0 && nr < H && nc >= 0 && nc < W) {
      my_tcell = nr * W + nc;
      my_tw = cells[my_tcell];
      my_occ = c.locmap[my_tcell];
    }
  }
  // World.can_agent_occupy, world.py:424-440, on the looked-up values
  const int my_own = AIE_CELL_OWNER(my_tw);
  const bool my_can = my_tcell >= 0 && !(AIE_CELL_FLAGS(my_tw) & AIE_CELL_WATER) && (my_own < 0 || my_own == lane) && my_occ == 0;
  const uint32_t my_pk = (uint32_t)my_land | (my_can ? (uint32_t)my_tcell << 16 : 0xffff0000u);  // (cells fit 16 bits: uint16 lists)
  const uint32_t my_lw = my_can ? my_tw : my_ow;  // the landing tile's cell word
  uint64_t stale = 0;
  for (int k = 0; k < n; ++k) {
    const int i = bcast(perm, k);
    int land, tcell;
    uint32_t w;
    bool moves;
    if (!((stale >> i) & 1ull)) {
      const uint32_t pk = bcast(my_pk, i);
      land = (int)(pk & 0xffffu);
      tcell = (int)(pk >> 16);
      moves = tcell != 0xffff;
      w = bcast(my_lw, i);
    } else {
      const int a = (int)AIE_ACT_GATHER(bcast(A.act, i));
      const int r = bcast(A.lr, i), col = bcast(A.lc, i);
      land = r * W + col;
      tcell = 0xffff;
      moves = false;
      if (a != 0) {
        const int nr = r + (a == 3 ? -1 : a == 4 ? 1 : 0);
        const int nc = col + (a == 1 ? -1 : a == 2 ? 1 : 0);
        if (nr >= 0 && nr < H && nc >= 0 && nc < W) {
          const int t = nr * W + nc;
          const uint32_t tw = cells[t];
          const int occ = c.locmap[t];
          const int own = AIE_CELL_OWNER(tw);
          if (!(AIE_CELL_FLAGS(tw) & AIE_CELL_WATER) && (own < 0 || own == i) && occ == 0) {
            tcell = t;
            moves = true;
          }
        }
      }
      w = cells[moves ? tcell : land];
    }
    if (moves) {
      c.locmap[land] = 0;
      c.locmap[tcell] = (uint8_t)(i + 1);
      dirty_add_uniform(c, m, land);
      dirty_add_uniform(c, m, tcell);
      dirty_agent_moved(m, i);
      if (lane == i) {
        A.lr = udiv(tcell, W, c.P.mg_W);
        A.lc = tcell - A.lr * W;
        A.labor += c.R.c.move_labor;
      }
      // whoever targets the tile this agent left or the one it entered no longer knows that tile's occupancy
      stale |= __ballot(my_tcell == land || my_tcell == tcell);
      land = tcell;
    }
    // collect on the landing tile, also on a NO-OP (move.py:112-113,136)
    if ((w & 0xffffu) != 0) {
      const int health[2] = {(int)AIE_CELL_STONE(w), (int)AIE_CELL_WOOD(w)};
      const double bonus = bcast(my_bonus, i);
#pragma unroll
      for (int rs = 0; rs < 2; ++rs) {
        if (health[rs] >= 1) {
          // rand() is consumed even when bonus_gather_prob == 0 (move.py:138)
          const int got = 1 + (rng_double(m, lane) < bonus ? 1 : 0);
          if (lane == i) {
            if (rs == 0) A.inv0 += got; else A.inv1 += got;
            A.labor += c.R.c.collect_labor;
          }
          w -= (1u << (8 * rs));  // consume_resource, world.py:481-483
          if (c.ev) log_event(c, AIE_EV_GATHER, i, rs, got, land / W, land % W, 0, 0, 0, 0.0);
        }
      }
      cells[land] = w;
      dirty_add_uniform(c, m, land);
    }
  }
}

// Few agents: the plain serial loop (two dependent LDS round trips per agent).  Eight and more: every lane looks its
// own agent's tiles up first (measured: 10 agents 43.3 -> 42.3 us per launch, 4 agents 25.2 -> 26.9).
__device__ __forceinline__ void gather_component_step(const Ctx& c, MTL& m, Agents& A) {
  if (c.P.n >= 8) gather_component_step_lookahead(c, m, A);
  else gather_component_step_serial(c, m, A);
}

// ------------------------------------------------------------------------------------
// ContinuousDoubleAuction, F/components/continuous_double_auction.py
// ------------------------------------------------------------------------------------
// price_history *= 0.995 for every (commodity, agent, price) -- :451, all lanes
__device__ __forceinline__ void cda_decay_price_history(const Ctx& c) {
  double* ph = R_F64(c, o_cda_price_history);
  const int tot = 2 * c.P.n * c.P.P;
  for (int q = c.tid; q < tot; q += AIE_NT) ph[q] *= 0.995;
}

// Sort keys: bids by (price desc, lifetime desc, book position asc), asks by
// (price asc, lifetime desc, book position asc) == Python's stable sorted() at :249-256.
template <bool BIDS>
__device__ __forceinline__ bool order_before(int32_t a, int32_t b) {
  const int pa = AIE_ORD_PRICE(a), pb = AIE_ORD_PRICE(b);
  if (pa != pb) return BIDS ? pa > pb : pa < pb;
  return AIE_ORD_LIFE(a) > AIE_ORD_LIFE(b);
}

// Inserts v[q] into the sorted prefix v[0..q): one ballot per 64 slots finds the
// insertion point, one lane shift per 64 slots makes room (high slices first).
template <bool BIDS>
__device__ __forceinline__ void book_insert(int32_t* v, int q, int lane) {
  const int32_t x = v[q];
  int p = 0;
  for (int base = 0; base < q; base += AIE_NT) {
    const int idx = base + lane;
    const bool stays = idx < q && !order_before<BIDS>(x, v[idx < q ? idx : 0]);
    p += __popcll(__ballot(stays));
  }
  if (p == q) return;
  for (int base = ((q - 1) / AIE_NT) * AIE_NT; base >= 0; base -= AIE_NT) {
    const int idx = base + lane;
    const bool mv = idx >= p && idx < q;
    const int32_t t = mv ? v[idx] : 0;
    if (mv) v[idx + 1] = t;
  }
  v[p] = x;
}
// Removes slot `at` from v[0..len): lane shift towards the front, low slices first.
__device__ __forceinline__ void book_remove(int32_t* v, int len, int at, int lane) {
  for (int base = (at / AIE_NT) * AIE_NT; base < len; base += AIE_NT) {
    const int idx = base + lane;
    const bool mv = idx > at && idx < len;
    const int32_t t = mv ? v[idx] : 0;
    if (mv) v[idx - 1] = t;
  }
}
// First slot of v[0..len) whose order satisfies pred (wave ballot + find-first-set).
template <typename Pred>
__device__ __forceinline__ int book_find_first(const int32_t* v, int len, int lane, Pred pred) {
  for (int base = 0; base < len; base += AIE_NT) {
    const int idx = base + lane;
    const uint64_t hit = __ballot(idx < len && pred(v[idx < len ? idx : 0]));
    if (hit) return base + __ffsll((unsigned long long)hit) - 1;
  }
  return -1;
}

// Order-count histograms are bytes; they are updated through 32-bit LDS atomics on the containing word
// (no carry / borrow between bytes: counts stay within [0, max_num_orders]), which, unlike a byte
// read-modify-write, does not make the wave wait for LDS.
__device__ __forceinline__ void hist_add(uint8_t* hist, int idx, int lane) {  // wave-uniform idx
  if (lane == 0) atomicAdd(reinterpret_cast<uint32_t*>(hist + (idx & ~3)), 1u << (8 * (idx & 3)));
}
__device__ __forceinline__ void hist_sub_lane(uint8_t* hist, int idx) {  // one decrement per calling lane
  atomicSub(reinterpret_cast<uint32_t*>(hist + (idx & ~3)), 1u << (8 * (idx & 3)));
}

// ContinuousDoubleAuction.component_step :440-489 (decay of :451 already applied)
__device__ __forceinline__ void cda_component_step(const Ctx& c, Agents& A) {
  const int n = c.P.n, M = c.P.M, P = c.P.P, lane = c.tid;
  const int maxo = c.P.c.cda_max_num_orders, dur = c.R.c.cda_order_duration;
  uint8_t* bid_hist = R_U8(c, o_cda_bid_hist);
  uint8_t* ask_hist = R_U8(c, o_cda_ask_hist);
  int nb[2] = {uni(R_I32(c, o_cda_n_bids)[0]), uni(R_I32(c, o_cda_n_bids)[1])};
  int na[2] = {uni(R_I32(c, o_cda_n_asks)[0]), uni(R_I32(c, o_cda_n_asks)[1])};
  const int nb0[2] = {nb[0], nb[1]}, na0[2] = {na[0], na[1]};

  // ---- create_bid :168-198 / create_ask :200-229, commodity-major, agents in index order
#pragma unroll
  for (int r = 0; r < AIE_N_RES; ++r) {
    int32_t* bids = R_I32(c, o_cda_bids) + r * M;
    int32_t* asks = R_I32(c, o_cda_asks) + r * M;
    const uint32_t buy = AIE_ACT_BUY(A.act, r), sell = AIE_ACT_SELL(A.act, r);
    const uint64_t mb = __ballot(lane < n && buy > 0), ms = __ballot(lane < n && sell > 0);
    uint64_t mm = mb | ms;
    while (mm) {
      const int i = __ffsll((unsigned long long)mm) - 1;
      mm &= mm - 1;
      const int no = bcast(r ? A.no1 : A.no0, i);
      if ((mb >> i) & 1ull) {
        const int price = (int)bcast(buy, i) - 1;
        if (no < maxo && !(bcast(A.coin, i) < (double)price)) {
          bids[nb[r]] = AIE_ORD_PACK(i, price, 0);
          nb[r] += 1;
          hist_add(bid_hist, (r * n + i) * P + price, lane);
          A.hist_dirty |= hist_bit(c.P, r, 1, price);
          if (lane == i) {
            if (r) A.no1 += 1; else A.no0 += 1;
            const double tr = A.coin < (double)price ? A.coin : (double)price;  // base_agent.py:279-299
            A.coin -= tr;
            A.esc_coin += tr;
            A.labor += c.R.c.cda_order_labor;
          }
        }
      }
      if ((ms >> i) & 1ull) {
        const int price = (int)bcast(sell, i) - 1;
        const int no2 = bcast(r ? A.no1 : A.no0, i);
        if (no2 < maxo && bcast(r ? A.inv1 : A.inv0, i) > 0) {
          asks[na[r]] = AIE_ORD_PACK(i, price, 0);
          na[r] += 1;
          hist_add(ask_hist, (r * n + i) * P + price, lane);
          A.hist_dirty |= hist_bit(c.P, r, 0, price);
          if (lane == i) {
            if (r) { A.no1 += 1; A.inv1 -= 1; A.esc1 += 1; }
            else { A.no0 += 1; A.inv0 -= 1; A.esc0 += 1; }
            A.labor += c.R.c.cda_order_labor;
          }
        }
      }
    }
  }

  // ---- match_orders :231-350
#pragma unroll
  for (int r = 0; r < AIE_N_RES; ++r) {
    int32_t* bids = R_I32(c, o_cda_bids) + r * M;
    int32_t* asks = R_I32(c, o_cda_asks) + r * M;
    // the book is kept sorted; only this step's new orders (appended) need inserting
    // Without a new order nothing can match: last step's loop ended with every buyer's
    // best bid below the cheapest ask of another agent, and expiry only removes orders.
    if (nb[r] == nb0[r] && na[r] == na0[r]) continue;
    uint64_t possible = (n >= 64) ? ~0ull : ((1ull << n) - 1ull);
    if (!c.full || M <= AIE_NT) {
      // Both books fit one wavefront: lane q keeps order q in a register.  This step's new orders
      // (appended behind the sorted part) are inserted with a ballot (position) and a one-lane shift; the
      // matching loop works on "alive" lane masks -- the best eligible bid / ask is a ballot +
      // find-first-set, a trade clears two bits; nothing in the loop's control flow waits on LDS.  The
      // survivors go back to LDS once, in order.
      int32_t bv = lane < nb[r] ? bids[lane] : 0;
      int32_t av = lane < na[r] ? asks[lane] : 0;
      for (int q = nb0[r]; q < nb[r]; ++q) {
        const int32_t x = bcast(bv, q);
        const int pb = __popcll(__ballot(lane < q && !order_before<true>(x, bv)));
        const int32_t up = (int32_t)__builtin_amdgcn_update_dpp(0, bv, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
        bv = (lane > pb && lane <= q) ? up : bv;
        bv = (lane == pb) ? x : bv;
      }
      for (int q = na0[r]; q < na[r]; ++q) {
        const int32_t x = bcast(av, q);
        const int pa = __popcll(__ballot(lane < q && !order_before<false>(x, av)));
        const int32_t up = (int32_t)__builtin_amdgcn_update_dpp(0, av, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
        av = (lane > pa && lane <= q) ? up : av;
        av = (lane == pa) ? x : av;
      }
      uint64_t alive_b = nb[r] >= 64 ? ~0ull : ((1ull << nb[r]) - 1ull);
      uint64_t alive_a = na[r] >= 64 ? ~0ull : ((1ull << na[r]) - 1ull);
      if (nb[r] == 0 || na[r] == 0) possible = 0;
      const int my_buyer = AIE_ORD_AGENT(bv), my_seller = AIE_ORD_AGENT(av);
      int ntrades = 0, trade = 0;
      while (possible) {
        const uint64_t bh = __ballot((possible >> my_buyer) & 1ull) & alive_b;
        if (!bh) break;  // out of bids to check (:262-264)
        const int ib = __ffsll((unsigned long long)bh) - 1;
        const int32_t bid = bcast(bv, ib);
        const int buyer = AIE_ORD_AGENT(bid), bprice = AIE_ORD_PRICE(bid);
        const uint64_t ah = __ballot(my_seller != buyer) & alive_a;
        int ia = -1;
        int32_t ask = 0;
        if (ah) { ia = __ffsll((unsigned long long)ah) - 1; ask = bcast(av, ia); }
        if (ia < 0 || bprice < AIE_ORD_PRICE(ask)) {  // :273-286
          possible &= ~(1ull << buyer);
          continue;
        }
        // TRADE :289-346.  Only the agents' registers change inside the loop; the book-keeping in LDS
        // (order histograms, price history) and the episode accumulators are applied after it, one lane
        // per trade, through atomics (equal addends / no byte borrow: the order of arrival is immaterial).
        alive_b &= ~(1ull << ib);
        alive_a &= ~(1ull << ia);
        const int seller = AIE_ORD_AGENT(ask), aprice = AIE_ORD_PRICE(ask);
        const bool at_ask = AIE_ORD_LIFE(bid) <= AIE_ORD_LIFE(ask);  // :297-304
        const int price = at_ask ? aprice : bprice;
        if (lane == ntrades) trade = buyer | (seller << 6) | (bprice << 12) | (aprice << 20) | ((int)at_ask << 28);
        A.hist_dirty |= hist_bit(c.P, r, 1, bprice) | hist_bit(c.P, r, 0, aprice);  // (the decrements behind the loop)
        ntrades += 1;
        if (c.ev) log_event(c, AIE_EV_TRADE, r, seller, buyer, aprice, bprice, price, AIE_ORD_LIFE(ask), AIE_ORD_LIFE(bid), 0.0);
        if (lane == seller) {
          if (r) { A.no1 -= 1; A.esc1 -= 1; } else { A.no0 -= 1; A.esc0 -= 1; }
          A.coin += (double)price;
        }
        if (lane == buyer) {
          if (r) { A.no1 -= 1; A.inv1 += 1; } else { A.no0 -= 1; A.inv0 += 1; }
          A.esc_coin -= (double)bprice;
          A.coin += (double)(bprice - price);
        }
      }
      if (lane < ntrades) {
        const int buyer = trade & 63, seller = (trade >> 6) & 63, bprice = (trade >> 12) & 255, aprice = (trade >> 20) & 255;
        const int price = ((trade >> 28) & 1) ? aprice : bprice;
        const int bi = (r * n + buyer) * P + bprice, ai = (r * n + seller) * P + aprice;
        atomicSub(reinterpret_cast<uint32_t*>(bid_hist + (bi & ~3)), 1u << (8 * (bi & 3)));
        atomicSub(reinterpret_cast<uint32_t*>(ask_hist + (ai & ~3)), 1u << (8 * (ai & 3)));
        unsafeAtomicAdd(R_F64(c, o_cda_price_history) + (r * n + seller) * P + price, 1.0);
        if (C_MET(c)) {  // get_metrics :585-641: fire-and-forget integer atomics
          int32_t* tm = reinterpret_cast<int32_t*>(C_MET(c) + c.P.mo_cda);
          int32_t* sell = tm + ((0 * AIE_N_RES + r) * n + seller) * 2;
          int32_t* buy = tm + ((1 * AIE_N_RES + r) * n + buyer) * 2;
          atomicAdd(sell, 1); atomicAdd(sell + 1, price);
          atomicAdd(buy, 1); atomicAdd(buy + 1, price);
        }
      }
      // leftover orders keep their (sorted) order: slot = number of survivors in front
      AIE_WSYNC();
      if ((alive_b >> lane) & 1ull) bids[__popcll(alive_b & ((1ull << lane) - 1ull))] = bv;
      if ((alive_a >> lane) & 1ull) asks[__popcll(alive_a & ((1ull << lane) - 1ull))] = av;
      nb[r] = __popcll(alive_b);
      na[r] = __popcll(alive_a);
      AIE_WSYNC();
      continue;
    }
    for (int q = nb0[r]; q < nb[r]; ++q) book_insert<true>(bids, q, lane);
    for (int q = na0[r]; q < na[r]; ++q) book_insert<false>(asks, q, lane);
    if (nb[r] == 0 || na[r] == 0) continue;
    while (possible) {
      const uint64_t poss = possible;
      const int ib = book_find_first(bids, nb[r], lane, [poss](int32_t o) { return ((poss >> AIE_ORD_AGENT(o)) & 1ull) != 0; });
      if (ib < 0) break;  // out of bids to check (:262-264)
      const int32_t bid = uni(bids[ib]);
      const int buyer = AIE_ORD_AGENT(bid), bprice = AIE_ORD_PRICE(bid);
      const int ia = book_find_first(asks, na[r], lane, [buyer](int32_t o) { return AIE_ORD_AGENT(o) != buyer; });
      int32_t ask = 0;
      if (ia >= 0) ask = uni(asks[ia]);
      if (ia < 0 || bprice < AIE_ORD_PRICE(ask)) {  // :273-286
        possible &= ~(1ull << buyer);
        continue;
      }
      // TRADE :289-346
      book_remove(bids, nb[r], ib, lane);
      nb[r] -= 1;
      book_remove(asks, na[r], ia, lane);
      na[r] -= 1;
      const int seller = AIE_ORD_AGENT(ask), aprice = AIE_ORD_PRICE(ask);
      const int price = (AIE_ORD_LIFE(bid) <= AIE_ORD_LIFE(ask)) ? aprice : bprice;  // :297-304
      bid_hist[(r * n + buyer) * P + bprice] -= 1;
      ask_hist[(r * n + seller) * P + aprice] -= 1;
      A.hist_dirty |= hist_bit(c.P, r, 1, bprice) | hist_bit(c.P, r, 0, aprice);
      R_F64(c, o_cda_price_history)[(r * n + seller) * P + price] += 1.0;
      if (lane == 0 && C_MET(c)) {  // get_metrics :585-641: fire-and-forget integer atomics
        int32_t* tm = reinterpret_cast<int32_t*>(C_MET(c) + c.P.mo_cda);
        int32_t* sell = tm + ((0 * AIE_N_RES + r) * n + seller) * 2;
        int32_t* buy = tm + ((1 * AIE_N_RES + r) * n + buyer) * 2;
        atomicAdd(sell, 1); atomicAdd(sell + 1, price);
        atomicAdd(buy, 1); atomicAdd(buy + 1, price);
      }
      if (c.ev) log_event(c, AIE_EV_TRADE, r, seller, buyer, aprice, bprice, price, AIE_ORD_LIFE(ask), AIE_ORD_LIFE(bid), 0.0);
      if (lane == seller) {
        if (r) { A.no1 -= 1; A.esc1 -= 1; } else { A.no0 -= 1; A.esc0 -= 1; }
        A.coin += (double)price;
      }
      if (lane == buyer) {
        if (r) { A.no1 -= 1; A.inv1 += 1; } else { A.no0 -= 1; A.inv0 += 1; }
        A.esc_coin -= (double)bprice;
        A.coin += (double)(bprice - price);
      }
    }
  }

  // ---- remove_expired_orders :352-406: lifetime += 1 everywhere, compaction by ballot
  if (!c.full || M <= AIE_NT) {
    // one lane per resting order: the four books are read back to back, survivors are scattered to their new
    // slots, expired orders decrement their histogram byte themselves (LDS atomics); only the owners'
    // registers are updated one expiry after the other, in book order (coin additions do not commute)
    int32_t ob[2][2];
#pragma unroll
    for (int r = 0; r < AIE_N_RES; ++r) {
      ob[r][0] = lane < nb[r] ? (R_I32(c, o_cda_bids) + r * M)[lane] : 0;
      ob[r][1] = lane < na[r] ? (R_I32(c, o_cda_asks) + r * M)[lane] : 0;
    }
    AIE_WSYNC();
#pragma unroll
    for (int r = 0; r < AIE_N_RES; ++r) {
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        int32_t* v = (side == 0 ? R_I32(c, o_cda_bids) : R_I32(c, o_cda_asks)) + r * M;
        const int len = side == 0 ? nb[r] : na[r];
        const int32_t o = ob[r][side];
        const bool valid = lane < len;
        const int life = AIE_ORD_LIFE(o) + 1;
        const bool keep = valid && life <= dur;
        const uint64_t km = __ballot(keep);
        uint64_t em = __ballot(valid && !keep);
        if (keep) v[__popcll(km & lanemask_lt(lane))] = AIE_ORD_PACK(AIE_ORD_AGENT(o), AIE_ORD_PRICE(o), life);
        if (valid && !keep) hist_sub_lane(side == 0 ? bid_hist : ask_hist, (r * n + AIE_ORD_AGENT(o)) * P + AIE_ORD_PRICE(o));
        while (em) {
          const int q = __ffsll((unsigned long long)em) - 1;
          em &= em - 1;
          const int32_t eo = bcast(o, q);
          const int ag = AIE_ORD_AGENT(eo), pr = AIE_ORD_PRICE(eo);
          A.hist_dirty |= hist_bit(c.P, r, side == 0 ? 1 : 0, pr);  // (hist_sub_lane above)
          if (lane == ag) {
            if (side == 0) {
              const double tr = A.esc_coin < (double)pr ? A.esc_coin : (double)pr;  // escrow_to_inventory
              A.esc_coin -= tr;
              A.coin += tr;
              if (r) A.no1 -= 1; else A.no0 -= 1;
            } else {
              if (r) { A.esc1 -= 1; A.inv1 += 1; A.no1 -= 1; }
              else { A.esc0 -= 1; A.inv0 += 1; A.no0 -= 1; }
            }
          }
        }
        if (side == 0) nb[r] = __popcll(km); else na[r] = __popcll(km);
      }
    }
  } else {
#pragma unroll
  for (int r = 0; r < AIE_N_RES; ++r) {
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      int32_t* v = (side == 0 ? R_I32(c, o_cda_bids) : R_I32(c, o_cda_asks)) + r * M;
      const int len = side == 0 ? nb[r] : na[r];
      int kept = 0;
      for (int base = 0; base < len; base += AIE_NT) {
        const int idx = base + lane;
        const bool valid = idx < len;
        const int32_t o = valid ? v[idx] : 0;
        const int life = AIE_ORD_LIFE(o) + 1;
        const bool keep = valid && life <= dur;
        const uint64_t km = __ballot(keep);
        uint64_t em = __ballot(valid && !keep);
        if (keep) v[kept + __popcll(km & lanemask_lt(lane))] = AIE_ORD_PACK(AIE_ORD_AGENT(o), AIE_ORD_PRICE(o), life);
        kept += __popcll(km);
        while (em) {  // expiries are rare: handled one by one, in book order
          const int q = __ffsll((unsigned long long)em) - 1;
          em &= em - 1;
          const int32_t eo = bcast(o, q);
          const int ag = AIE_ORD_AGENT(eo), pr = AIE_ORD_PRICE(eo);
          A.hist_dirty |= hist_bit(c.P, r, side == 0 ? 1 : 0, pr);
          if (side == 0) {
            bid_hist[(r * n + ag) * P + pr] -= 1;
            if (lane == ag) {
              const double tr = A.esc_coin < (double)pr ? A.esc_coin : (double)pr;  // escrow_to_inventory
              A.esc_coin -= tr;
              A.coin += tr;
              if (r) A.no1 -= 1; else A.no0 -= 1;
            }
          } else {
            ask_hist[(r * n + ag) * P + pr] -= 1;
            if (lane == ag) {
              if (r) { A.esc1 -= 1; A.inv1 += 1; A.no1 -= 1; }
              else { A.esc0 -= 1; A.inv0 += 1; A.no0 -= 1; }
            }
          }
        }
      }
      if (side == 0) nb[r] = kept; else na[r] = kept;
    }
  }
  }
  R_I32(c, o_cda_n_bids)[0] = nb[0];
  R_I32(c, o_cda_n_bids)[1] = nb[1];
  R_I32(c, o_cda_n_asks)[0] = na[0];
  R_I32(c, o_cda_n_asks)[1] = na[1];
}

// ------------------------------------------------------------------------------------
// PeriodicBracketTax, F/components/redistribution.py: enactment and component step
// (the schedule -- tax_rate ... tax_due -- is shared with the other scenarios: aie_device.h)
// ------------------------------------------------------------------------------------
// enact_taxes :853-915: lane i computes agent i's income / tax; the revenue is summed
// in agent order (the reference's running `net_tax_revenue +=`).
__device__ __forceinline__ void tax_enact(const Ctx& c, Agents& A) {
  const int n = c.P.n, i = c.tid;
  double eff = 0, eff_rate = 0;
  if (i < n) {
    const double income = (A.coin + A.esc_coin) - R_F64(c, o_tax_last_coin)[i];
    const double due = tax_due(c, income);
    eff = A.coin < due ? A.coin : due;  // escrow is not taxed
    R_F64(c, o_tax_last_marginal_rate)[i] = tax_marginal_rate(c, income);
    R_F64(c, o_tax_last_income)[i] = income;
    A.coin -= eff;
    eff_rate = eff / (income > 0.000001 ? income : 0.000001);  // :880
    if (C_MET(c)) {  // episode accumulators for get_metrics :1141-1186 (no-return atomics)
      unsafeAtomicAdd(reinterpret_cast<double*>(C_MET(c) + c.P.mo_tax_income) + i, income > 0 ? income : 0.0);
      unsafeAtomicAdd(reinterpret_cast<double*>(C_MET(c) + c.P.mo_tax_paid) + i, eff);
      int bin = 0;  // income_bin :828-835
      if (income >= 0)
        for (int b = 0; b < c.P.NB; ++b)
          if (income >= c.R.c.tax_bracket_cutoffs[b] && (b + 1 == c.P.NB || income < c.R.c.tax_bracket_cutoffs[b + 1])) { bin = b; break; }
      atomicAdd(reinterpret_cast<int32_t*>(C_MET(c) + c.P.mo_tax_occ) + bin, 1);
    }
  }
  if (C_MET(c)) {
    if (i < c.P.NB) unsafeAtomicAdd(reinterpret_cast<double*>(C_MET(c) + c.P.mo_tax_sched) + i, tax_rate(c, i));
    double day = 0;
    for (int j = 0; j < n; ++j) day += bcast(eff_rate, j);
    if (i == 0) {
      unsafeAtomicAdd(reinterpret_cast<double*>(C_MET(c) + c.P.mo_tax_eff), day);
      atomicAdd(reinterpret_cast<int32_t*>(C_MET(c) + c.P.mo_tax_days), 1);
    }
  }
  if (c.ev) {
    for (int b = 0; b < c.P.NB; ++b) log_event(c, AIE_EV_TAX_BRACKET, b, 0, 0, 0, 0, 0, 0, 0, tax_rate(c, b));
    for (int j = 0; j < n; ++j) log_event(c, AIE_EV_TAX, j, 0, 0, 0, 0, 0, 0, 0, bcast(eff, j));
  }
  double net = 0;
  for (int j = 0; j < n; ++j) net += bcast(eff, j);
  *R_F64(c, o_tax_total_collected) += net;
  const double lump = net / (double)n;
  if (i < n) {
    A.coin += lump;
    R_F64(c, o_tax_last_coin)[i] = A.coin + A.esc_coin;
  }
  if (c.saez) {  // _update_saez_buffer :533-541 (global memory, tax days only)
    uint8_t* blk = saez_block(c);
    int32_t* hdr = reinterpret_cast<int32_t*>(blk);
    double* buf = reinterpret_cast<double*>(blk + AIE_SAEZ_OFF_BUF);
    int len = uni(hdr[0]);
    if (i < n) {
      buf[2 * (len + i)] = R_F64(c, o_tax_last_income)[i];
      buf[2 * (len + i) + 1] = R_F64(c, o_tax_last_marginal_rate)[i];
    }
    len += n;
    const int size = c.R.c.saez_buffer_size;
    if (len > size) {  // drop the oldest: move down chunk by chunk (a chunk's loads precede its stores;
      const int shift = 2 * (len - size);  // later chunks only read above what earlier ones wrote)
      __builtin_amdgcn_s_waitcnt(0);
      for (int base = 0; base < 2 * size; base += AIE_NT) {
        const int q = base + i;
        double v = 0;
        if (q < 2 * size) v = buf[q + shift];
        __builtin_amdgcn_s_waitcnt(0);
        if (q < 2 * size) buf[q] = v;
      }
      len = size;
    }
    if (i == 0) {
      hdr[0] = len;
      hdr[2] += n;  // _additions_this_episode :541 (only reset_saez_buffers zeroes it)
    }
  }
}
// component_step :945-972 + set_new_period_rates_model :419-434
__device__ __forceinline__ void tax_component_step(const Ctx& c, MTL& ml, Agents& A) {
  int pos = uni(*R_I32(c, o_tax_cycle_pos));
  // the flat vectors' tax block follows the latched rates (Saez, the model wrapper: pos == 1) and what tax_enact leaves
  A.tax_dirty |= (pos == 1 && (c.saez || (c.P.c.tax_model == AIE_TAX_MODEL_WRAPPER && !c.P.c.tax_disable))) ||
                 pos >= c.R.c.tax_period;
  if (pos == 1 && c.saez) {  // compute_and_set_new_period_rates_from_saez_formula
    uint8_t* blk = saez_block(c);
    if (uni(reinterpret_cast<const int32_t*>(blk)[1])) {  // the formula ran in aie_saez_kernel just before this launch
      if (c.tid < c.P.NB) R_F64(c, o_tax_saez_rates)[c.tid] = reinterpret_cast<const double*>(blk + AIE_SAEZ_OFF_NEXT)[c.tid];
    } else {  // np.random.uniform(low=rate_min, high=curr_rate_max, size=n_brackets) :451-457
      const double lo = c.R.c.tax_rate_min;
      const double hi = c.P.c.tax_annealing ? tax_curr_rate_max(c) : c.R.c.tax_rate_max;
      for (int b = 0; b < c.P.NB; ++b) {
        const double r = lo + (hi - lo) * rng_double(ml, c.tid);
        if (c.tid == b) R_F64(c, o_tax_saez_rates)[b] = r;
      }
    }
    AIE_WSYNC();
    if (c.tid < c.P.NB) R_F64(c, o_tax_saez_obs_rates)[c.tid] = tax_rate(c, c.tid);  // _curr_rates_obs :959
    AIE_WSYNC();
  }
  if (pos == 1 && c.P.c.tax_model == AIE_TAX_MODEL_WRAPPER && !c.P.c.tax_disable) {
    if (c.tid < c.P.NB) {
      const int a = c.act_p[c.tid];
      if (a > 0 && a <= c.P.c.tax_n_disc_rates) R_I32(c, o_tax_rate_idx)[c.tid] = a - 1;
    }
    AIE_WSYNC();
  }
  if (pos >= c.R.c.tax_period) {
    tax_enact(c, A);
    pos = 0;
  }
  *R_I32(c, o_tax_cycle_pos) = pos + 1;
}

// WealthRedistribution.component_step, F/components/redistribution.py:46-65: inventory coin
// := np.sum(inventory + escrow) / n - escrow.  The sum follows NumPy's pairwise order
// (np_sum_small) with the lanes' values read through wave broadcasts.
__device__ __forceinline__ void wealth_component_step(const Ctx& c, Agents& A) {
  const int n = c.P.n;
  const double v = A.coin + A.esc_coin;
  double tot;
  if (n < 8) {
    tot = -0.0;
    for (int j = 0; j < n; ++j) tot += bcast(v, j);
  } else {
    double r[8];
    for (int q = 0; q < 8; ++q) r[q] = bcast(v, q);
    int j = 8;
    for (; j < n - (n % 8); j += 8)
      for (int q = 0; q < 8; ++q) r[q] += bcast(v, j + q);
    tot = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; j < n; ++j) tot += bcast(v, j);
  }
  if (c.tid < n) A.coin = tot / (double)n - A.esc_coin;
}

// (contraction stays off, see the top of the file)

// ------------------------------------------------------------------------------------
// LayoutFromFile.scenario_step, layout_from_file.py:372-410.
// regen_halfwidth == 0: p = regen_weight * max(map, src); only source blocks spawn.
// regen_halfwidth > 0 (dynamic_layout.py:446-463): p from the per-episode window counts.
// np.random.rand(H, W) is consumed for Wood, then for Stone: 4*H*W MT19937 words per
// step, read row by row straight from the state registers (pairs of adjacent lanes
// form one 53-bit double); a double that straddles a twist is carried over.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void regen_cell(const Ctx& c, uint32_t ta, uint32_t tb, int d) {
  const int HW = c.P.HW;
  const int rs = d >= HW ? 0 : 1;  // first H*W doubles are Wood's, then Stone's
  const int cell = d - (d >= HW ? HW : 0);
  uint8_t* cb = reinterpret_cast<uint8_t*>(R_CELLS(c)) + 4 * cell;
  const uint32_t fl = cb[3];
  if (fl & (rs ? AIE_CELL_WOOD_SRC : AIE_CELL_STONE_SRC)) {
    const uint32_t mval = cb[rs];
    const uint32_t health = mval > 1u ? mval : 1u;  // max(map, source block = 1)
    const double u = u53(ta, tb);
    // halfwidth 0: p = regen_weight * health; else regen_p[source blocks in the window] (aie_layout.h: regen_conv)
    double p;
    const int hwid = c.P.regen_conv ? c.P.c.regen_halfwidth[rs] : 0;
    if (c.full && c.snap && hwid > 0 && c.P.c.max_health[rs] > 1) {
      // signal.convolve2d(max(map, source blocks), regen_weight / d^2 * ones(d, d), "same") at this cell, one
      // multiply-add per kernel element in scipy's order (input rows r0+hw .. r0-hw, columns c0+hw .. c0-hw, zeros
      // outside the world), over the pre-step snapshot (dynamic_layout.py:446-463)
      const int dd = 1 + 2 * hwid, W = c.P.W, r0 = cell / W, c0 = cell - r0 * W;
      const double kern = c.R.c.regen_weight[rs] / (double)(dd * dd);
      const uint8_t* sp = c.snap + rs * ((HW + 15) / 16 * 16);
      p = 0.0;
      for (int r = r0 + hwid; r >= r0 - hwid; --r)
        for (int cc = c0 + hwid; cc >= c0 - hwid; --cc)
          if (r >= 0 && r < c.P.H && cc >= 0 && cc < W) p += kern * (double)sp[r * W + cc];
    } else if (hwid > 0) {
      p = c.R.regen_p[rs][R_U8(c, o_regen_count)[rs * HW + cell]];
    } else {
      p = c.R.c.regen_weight[rs] * (double)health;
    }
    if (u < p && mval < (uint32_t)c.P.c.max_health[rs]) {
      cb[rs] = (uint8_t)(mval + 1);
      dirty_add_lane(c, cell);
    }
  }
}
__device__ __forceinline__ void scenario_step_regen_rows(const Ctx& c, MT& m) {
  const int lane = c.tid;
  const int total = 4 * c.P.HW;  // words to consume
  int done = 0;
  bool carry = false;
  uint32_t carry_t = 0;
  int carry_d = 0;
  while (true) {
    if (m.pos >= AIE_MT_N) {
      mt_twist(m, lane);
      m.pos = 0;
    }
    const int pos = m.pos;
    if (carry) {  // second half of a double whose first word was word 623 of the old state
      if (lane == 0) regen_cell(c, carry_t, mt_word(m, m.r[0]), carry_d);
      carry = false;
    }
#pragma unroll
    for (int J = 0; J < 10; ++J) {
      if (64 * J + 63 < pos) continue;              // row fully consumed already
      if (done + (64 * J - pos) >= total) continue;  // row entirely beyond this step's needs
      const int a_idx = 64 * J + lane;
      const int q = done + (a_idx - pos);           // regen-relative word number
      const uint32_t t = mt_word(m, m.r[J]);
      uint32_t tn = lane_get(t, (lane + 1) & 63);
      if (J < 9) tn = (lane == 63) ? mt_word(m, bcast(m.r[J + 1], 0)) : tn;
      const bool first = a_idx >= pos && a_idx < AIE_MT_N - 1 && (q & 1) == 0 && q < total;
      if (first) regen_cell(c, t, tn, q >> 1);
    }
    const int avail = AIE_MT_N - pos;
    const int take = (total - done) < avail ? (total - done) : avail;
    if (take == avail) {  // consumed word 623: is it the first half of a double?
      const int q623 = done + (AIE_MT_N - 1 - pos);
      if ((q623 & 1) == 0 && q623 < total) {
        carry = true;
        carry_t = mt_word(m, bcast(m.r[9], 47));
        carry_d = q623 >> 1;
      }
    }
    done += take;
    m.pos = pos + take;
    if (done >= total) break;
  }
}

// Sparse variant (the normal case: a few dozen source blocks): lane j owns source double d_j and needs stream words
// pos+2*d_j, +1.  The state is advanced window by window (one twist each) in registers; in every window each lane
// fetches the word(s) that fall into it straight from the row registers: one permute per row, the lane keeps the
// one of its own row (word i of a window sits in row i >> 6, lane i & 63).  No LDS copy of the window.
__device__ __forceinline__ uint32_t mt_window_word(const MT& m, int idx) {
  const int row = idx >> 6, ln = idx & 63;
  uint32_t v = 0;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t t = lane_get(m.r[r], ln);
    v = (row == r) ? t : v;
  }
  return v;
}
// The source doubles of this replica: the LDS list load_record collected, or -- fixed layouts shared by the batch -- the
// caller's registers (entry k * 64 + lane of aie_params.a_src_list, fetched while the components ran) and their count.
struct SrcList {
  int S;                            // number of source doubles (may exceed AIE_SRC_CAP: row-by-row regeneration)
  int d[AIE_SRC_CAP / AIE_NT];      // this lane's entries
};
__device__ __forceinline__ SrcList src_list_from_record(const Ctx& c, const uint8_t* __restrict__ arena) {
  SrcList L;
  const uint8_t* g = arena + (int64_t)c.e * c.P.rec_bytes;
  L.S = uni(*reinterpret_cast<const int32_t*>(g + c.P.o_src_n));
  const uint16_t* lst = reinterpret_cast<const uint16_t*>(g + c.P.o_src_list);
#pragma unroll
  for (int k = 0; k < AIE_SRC_CAP / AIE_NT; ++k) L.d[k] = (int)lst[k * AIE_NT + c.tid];  // (entries past the count are zero)
  return L;
}
__device__ __forceinline__ SrcList src_list_from_arena(const Ctx& c, const uint8_t* __restrict__ arena) {
  SrcList L;
  const uint8_t* g = arena + c.R.a_src_list;
  L.S = uni(*reinterpret_cast<const int32_t*>(g));
  const uint16_t* lst = reinterpret_cast<const uint16_t*>(g + 16);
#pragma unroll
  for (int k = 0; k < AIE_SRC_CAP / AIE_NT; ++k) L.d[k] = (int)lst[k * AIE_NT + c.tid];  // (entries past the count are zero)
  return L;
}
__device__ __forceinline__ void scenario_step_regen(const Ctx& c, MT& m, const SrcList& src) {
  if (c.full && c.snap) {  // P.regen_general: the planes the reference convolves, before any of this step's respawns
    const int HW = c.P.HW, stride = (HW + 15) / 16 * 16;
    const uint8_t* cb = reinterpret_cast<const uint8_t*>(R_CELLS(c));
    for (int q = c.tid; q < HW; q += AIE_NT) {
      const uint32_t fl = cb[4 * q + 3];
      const uint8_t s0 = cb[4 * q], s1 = cb[4 * q + 1];
      c.snap[q] = (fl & AIE_CELL_STONE_SRC) ? (s0 > 1 ? s0 : 1) : s0;
      c.snap[stride + q] = (fl & AIE_CELL_WOOD_SRC) ? (s1 > 1 ? s1 : 1) : s1;
    }
    AIE_WSYNC();
  }
  const int S = src.S;
  if (S > AIE_SRC_CAP) {
    if (m.fast && m.pos < AIE_MT_N) mt_fast_rows(m, c.tid);  // (the counter stream keeps no rows between steps)
    scenario_step_regen_rows(c, m);
    return;
  }
  const int lane = c.tid;
  const int total = 4 * c.P.HW;
  const int pos0 = m.pos;  // <= 624
  const int nchunk = (S + AIE_NT - 1) / AIE_NT;
  if (m.fast) {
    // AIE_RNG_FAST: source double d is words pos0 + 2 d, + 1 of the linear stream -- computed where they are needed.  One
    // Philox block per lane when pos0 is even (both words in one pair), two when it is odd (wave-uniform).
    const int odd = pos0 & 1;
#pragma unroll
    for (int k = 0; k < AIE_SRC_CAP / AIE_NT; ++k) {
      if (k >= nchunk) continue;
      const int j = k * AIE_NT + lane;
      const int d = j < S ? src.d[k] : 0;
      const int h = (pos0 >> 1) + d;  // pair that holds word pos0 + 2 d
      uint32_t a0, a1, b0 = 0, b1 = 0;
      fast_pair(m.fkey, m.fblk, m.fsalt, h, a0, a1);
      if (odd) fast_pair(m.fkey, m.fblk, m.fsalt, h + 1, b0, b1);
      if (j < S) regen_cell(c, odd ? a1 : a0, odd ? b0 : a1, d);
    }
    const int last_win = (pos0 + total - 1) / AIE_MT_N;
    m.pos = pos0 + total - last_win * AIE_MT_N;
    m.fblk += (uint32_t)last_win;
    AIE_WSYNC();
    return;
  }
  int off_a[AIE_SRC_CAP / AIE_NT];
  uint32_t wa[AIE_SRC_CAP / AIE_NT], wb[AIE_SRC_CAP / AIE_NT];
#pragma unroll
  for (int k = 0; k < AIE_SRC_CAP / AIE_NT; ++k) {
    const int j = k * AIE_NT + lane;
    off_a[k] = (k < nchunk && j < S) ? pos0 + 2 * src.d[k] : -16;  // stream offset of word A
    wa[k] = wb[k] = 0;
  }
  const int last_win = (pos0 + total - 1) / AIE_MT_N;
  for (int w = 0; w <= last_win; ++w) {
    if (w > 0) mt_twist_body(m, lane);  // the hot site: inlined (4 twists per step)
    const int lo = w * AIE_MT_N;
    if (c.mtwin) {
      // the window through LDS (mt_window_in_lds): ten row stores, then one two-word read per lane and chunk.  LDS
      // operations of a wave execute in order, so the reads see the stores, and the next window's stores the reads.
#pragma unroll
      for (int j = 0; j < 10; ++j) c.mtwin[64 * j + lane] = m.r[j];
#pragma unroll
      for (int k = 0; k < AIE_SRC_CAP / AIE_NT; ++k) {
        if (k >= nchunk) continue;
        const int ia = off_a[k] - lo;  // word A's index in this window (-1: A was the previous window's last word)
        const bool ha = (unsigned)ia < (unsigned)AIE_MT_N, hb = (unsigned)(ia + 1) < (unsigned)AIE_MT_N;
        if (__ballot(ha || hb) == 0) continue;
        const int at = ia < 0 ? 0 : (ia > AIE_MT_N - 1 ? AIE_MT_N - 1 : ia);
        const uint32_t x0 = c.mtwin[at], x1 = c.mtwin[at + 1];  // (word 624 is padding: read, never used)
        if (ha) wa[k] = x0;
        if (hb) wb[k] = ia < 0 ? x0 : x1;
      }
      continue;
    }
#pragma unroll
    for (int k = 0; k < AIE_SRC_CAP / AIE_NT; ++k) {
      if (k >= nchunk) continue;  // (uniform: the usual map lists < 64 draws)
      const int ia = off_a[k] - lo, ib = ia + 1;
      const bool ha = ia >= 0 && ia < AIE_MT_N, hb = off_a[k] >= 0 && ib >= 0 && ib < AIE_MT_N;
      if (__ballot(ha || hb) == 0) continue;
      const uint32_t va = mt_window_word(m, ha ? ia : 0), vb = mt_window_word(m, hb ? ib : 0);
      if (ha) wa[k] = va;
      if (hb) wb[k] = vb;
    }
  }
  m.pos = pos0 + total - last_win * AIE_MT_N;
#pragma unroll
  for (int k = 0; k < AIE_SRC_CAP / AIE_NT; ++k)
    if (k < nchunk && off_a[k] >= 0) regen_cell(c, mt_temper(wa[k]), mt_temper(wb[k]), (off_a[k] - pos0) >> 1);
  AIE_WSYNC();
}

// ------------------------------------------------------------------------------------
// Utilities / rewards
// ------------------------------------------------------------------------------------
__device__ __forceinline__ double energy_weight(const Ctx& c) {  // layout_from_file.py:249-267
  if (!c.P.sh_energy_warmup) return 1.0;  // (energy_warmup_constant <= 0: a property of the instance's family)
  const int v = c.P.c.energy_warmup_method == AIE_WARMUP_DECAY ? *R_I32(c, o_completions) : *R_I32(c, o_auto_warmup);
  return 1.0 - aie_exp_glibc(-(double)v / c.R.c.energy_warmup_constant);  // libm's exp, bit for bit (aie_glibc_math.h)
}

// get_current_optimization_metrics layout_from_file.py:269-318 with
// rewards.isoelastic_coin_minus_labor (F/scenarios/utils/rewards.py:12-48),
// coin_eq_times_productivity (:84-101), inv_income_weighted_* (:104-133),
// social_metrics.get_gini (social_metrics.py:10-46).
// Lane i < n computes agent i's utility; lane 0 finishes the planner's.
// Results are left in scr_part()[0..n]; must be followed by AIE_WSYNC().
__device__ __forceinline__ void current_metrics(const Ctx& c) {
  const int n = c.P.n, i = c.tid;
  double* coin = scr_coin(c);
  double* out = scr_part(c);
  double* tmp = scr_gini_sort(c);  // (its own slot: only the other planner reward type sorts there, and the flat-vector
                                   // writer -- which may run on the other wave meanwhile -- ranks incomes in scr_cmr)
  const double lcf = energy_weight(c) * c.R.c.energy_cost;
  const double eta = c.R.c.isoelastic_eta;
  if (i < n) {
    const double ci = R_F64(c, o_inv_coin)[i] + R_F64(c, o_esc_coin)[i];
    coin[i] = ci;
    double util_c;
    if (c.P.sh_eta_is_one) util_c = aie_log_glibc(ci > 1 ? ci : 1);
    else util_c = (aie_pow_glibc(ci, 1 - eta) - 1) / (1 - eta);  // libm's pow bit for bit: the sign of a ~1e-16 mean reward
                                                                  // feeds the integer auto_warmup counter (aie_glibc_math.h)
    out[i] = util_c - R_F64(c, o_labor)[i] * lcf;
  }
  AIE_WSYNC();
  const int prt = c.P.c.planner_reward_type;
  // every sum below follows NumPy's pairwise add.reduce order (np_sum_small / np_sum_seq): the planner's utility is
  // state (`util`), compared with the reference bit for bit
  if (prt == AIE_PLANNER_REW_COIN_EQ_TIMES_PROD) {
    double gini;
    const double tot = np_sum_small(coin, n);
    if (n < 30) {
      const double diff = np_sum_seq<3>(coin, n, 1, 65536u / (uint32_t)n + 1u, 0, n * n, i);
      const double unscaled = diff / (2 * n * tot + 1e-10);
      gini = unscaled / ((double)(n - 1) / (double)n);
    } else {
      // sorted-cumsum branch (social_metrics.py:43-46)
      double* s = scr_gini_sort(c);
      if (i == 0) {
        for (int j = 0; j < n; ++j) s[j] = coin[j];
        for (int a = 1; a < n; ++a) {
          double x = s[a]; int b = a - 1;
          while (b >= 0 && s[b] > x) { s[b + 1] = s[b]; --b; }
          s[b + 1] = x;
        }
        const double tots = np_sum_small(s, n) + 1e-10;
        double run = 0;
        for (int j = 0; j < n; ++j) { run += s[j]; s[j] = run / tots; }
      }
      AIE_WSYNC();
      gini = 1 - (2.0 / (n + 1)) * np_sum_small(s, n);
    }
    if (i == 0) {
      const double ew = 1 - c.R.c.mixing_weight_gini_vs_coin;
      out[n] = (ew * (1 - gini) + (1 - ew)) * (tot / n);
    }
  } else {
    if (i < n) tmp[i] = 1 / (coin[i] > 1 ? coin[i] : 1);
    AIE_WSYNC();
    const double sw = np_sum_small(tmp, n);
    AIE_WSYNC();
    if (i < n) tmp[i] = (prt == AIE_PLANNER_REW_INV_INCOME_COIN ? coin[i] : out[i]) * (tmp[i] / sw);
    AIE_WSYNC();
    if (i == 0) out[n] = np_sum_small(tmp, n);
  }
}

// compute_reward layout_from_file.py:519-559
__device__ __forceinline__ void compute_rewards(const Ctx& c, uint8_t* __restrict__ arena, float* rew_log = nullptr) {
  const int n = c.P.n, i = c.tid;
  current_metrics(c);
  AIE_WSYNC();
  double* cur = scr_part(c);
  double* util = R_F64(c, o_util);
  double* rew = scr_coin(c);  // reuse
  if (i <= n) {
    const double r = cur[i] - util[i];
    util[i] = cur[i];
    rew[i] = r;
    if (i < n) reinterpret_cast<float*>(arena + c.R.a_rew_a)[(int64_t)c.e * n + i] = (float)r;
    else reinterpret_cast<float*>(arena + c.R.a_rew_p)[c.e] = (float)r;
    if (rew_log) rew_log[(int64_t)c.e * (n + 2) + i] = (float)r;
  }
  AIE_WSYNC();
  if (i == 0) {
    if (np_sum_small(rew, n) / n > 0) *R_I32(c, o_auto_warmup) += 1;
  }
}

// ------------------------------------------------------------------------------------
// Observations
// ------------------------------------------------------------------------------------
// Channels of Maps.state (world.py:59-93): Stone, Wood, House, [Water], StoneSourceBlock,
// WoodSourceBlock.  `ch[]` receives CM values for one packed cell word.
template <bool WATER>
__device__ __forceinline__ void cell_channels(uint32_t w, float* ch) {
  const uint32_t fl = w >> 24;
  ch[0] = (float)AIE_CELL_STONE(w);
  ch[1] = (float)AIE_CELL_WOOD(w);
  ch[2] = (((w >> 16) & 0xffu) != 0xffu) ? 1.0f : 0.0f;
  int k = 3;
  if (WATER) ch[k++] = (fl & AIE_CELL_WATER) ? 1.0f : 0.0f;
  ch[k++] = (fl & AIE_CELL_STONE_SRC) ? 1.0f : 0.0f;
  ch[k++] = (fl & AIE_CELL_WOOD_SRC) ? 1.0f : 0.0f;
}

// LayoutFromFile.generate_observations layout_from_file.py:412-517: the egocentric
// (2w+1)^2 crop for every agent and the full map for the planner.
//   crop:    one lane per (agent, window cell): one LDS word read feeds CM+1 coalesced f32
//            stores and 2 i16 stores (the out-of-world ring: all 0, in-bounds channel 0);
//   planner: one lane per 4 consecutive cells: one 16-byte LDS read feeds CM 16-byte
//            stores and two 8-byte stores.
// All stores go through buffer descriptors of this replica's observation blocks: one
// 32-bit lane offset per item + a scalar offset per (agent, channel) plane, instead of a
// 64-bit VGPR pointer per plane.
struct SpatialOut {
  BufRsrc amap, aidx, pmap, pidx;
};
template <bool WATER>
__device__ __forceinline__ SpatialOut spatial_out(const Ctx& c, uint8_t* __restrict__ arena) {
  constexpr int CM = WATER ? 6 : 5;
  const int n = c.P.n, HW = c.P.HW, WV2 = c.P.WV * c.P.WV;
  (void)WV2;
  const int plane = c.P.am_h * c.P.am_w;
  const uint32_t amap_bytes = (uint32_t)(n * c.P.am_ch * plane * 4), aidx_bytes = (uint32_t)(n * 2 * plane * 2);
  SpatialOut o;
  o.amap = make_rsrc(arena + c.R.a_obs_a_map + (int64_t)c.e * amap_bytes, amap_bytes);
  o.aidx = make_rsrc(arena + c.R.a_obs_a_idx + (int64_t)c.e * aidx_bytes, aidx_bytes);
  const bool pl = c.P.c.planner_gets_spatial_info != 0;
  o.pmap = make_rsrc(arena + c.R.a_obs_p_map + (int64_t)c.e * CM * HW * 4, pl ? (uint32_t)(CM * HW * 4) : 0u);
  o.pidx = make_rsrc(arena + c.R.a_obs_p_idx + (int64_t)c.e * 2 * HW * 2, pl ? (uint32_t)(2 * HW * 2) : 0u);
  return o;
}

// one (agent i, window cell d) item of the egocentric crop, layout_from_file.py:470-505
template <bool WATER>
__device__ __forceinline__ void crop_item(const Ctx& c, const SpatialOut& o, int i, int d, int r, int col) {
  constexpr int CM = WATER ? 6 : 5;
  const int H = c.P.H, W = c.P.W, WV2 = c.P.WV * c.P.WV;
  const int so = i * (CM + 1) * WV2 * 4, si = i * 2 * WV2 * 2;
  const bool in = (r >= 0) & (r < H) & (col >= 0) & (col < W);
  const int cell = in ? r * W + col : 0;
  const uint32_t cw = in ? R_CELLS(c)[cell] : 0x00ff0000u;  // :480-485
  float ch[6];
  cell_channels<WATER>(cw, ch);
#pragma unroll
  for (int k = 0; k < CM; ++k) buf_store_f32(o.amap, ch[k], 4 * d, so + k * WV2 * 4);
  buf_store_f32(o.amap, in ? 1.0f : 0.0f, 4 * d, so + CM * WV2 * 4);
  const int own = AIE_CELL_OWNER(cw);
  int v0 = own >= 0 ? own + 2 : 0;
  int v1 = in ? (int)c.locmap[cell] : 0;
  v1 = v1 ? v1 + 1 : 0;     // agent k -> k + 2
  if (v0 == i + 2) v0 = 1;  // :503
  if (v1 == i + 2) v1 = 1;
  buf_store_i16(o.aidx, v0, 2 * d, si);
  buf_store_i16(o.aidx, v1, 2 * d, si + WV2 * 2);
}
// the whole crop of agent i (wave-uniform i; lanes over the window cells)
template <bool WATER>
__device__ __forceinline__ void crop_agent(const Ctx& c, const SpatialOut& o, int i) {
  const int WV = c.P.WV, WV2 = WV * WV, w = c.P.c.obs_range;
  const int r0 = R_I32(c, o_loc_r)[i] - w, c0 = R_I32(c, o_loc_c)[i] - w;  // LDS broadcast reads
  for (int d = c.tid; d < WV2; d += AIE_NT) {
    const int dr = udiv(d, WV, c.P.mg_WV), dc = d - dr * WV;
    crop_item<WATER>(c, o, i, d, r0 + dr, c0 + dc);
  }
}
// one cell of the planner's full map (:507-517)
template <bool WATER>
__device__ __forceinline__ void planner_cell(const Ctx& c, const SpatialOut& o, int cell) {
  constexpr int CM = WATER ? 6 : 5;
  const int HW = c.P.HW;
  float ch[6];
  const uint32_t cw = R_CELLS(c)[cell];
  cell_channels<WATER>(cw, ch);
#pragma unroll
  for (int k = 0; k < CM; ++k) buf_store_f32(o.pmap, ch[k], 4 * cell, k * HW * 4);
  const int own = AIE_CELL_OWNER(cw);
  const int occ = c.locmap[cell];
  buf_store_i16(o.pidx, own >= 0 ? own + 2 : 0, 2 * cell, 0);
  buf_store_i16(o.pidx, occ ? occ + 1 : 0, 2 * cell, HW * 2);
}

// LayoutFromFile.generate_observations layout_from_file.py:412-517: the egocentric
// (2w+1)^2 crop for every agent and the full map for the planner.
//   crop:    one lane per window cell of a (wave-uniform) agent: one LDS word read feeds
//            CM+1 coalesced f32 stores and 2 i16 stores (the out-of-world ring: all 0);
//   planner: one lane per 4 consecutive cells: one 16-byte LDS read feeds CM 16-byte
//            stores and two 8-byte stores.
template <bool WATER>
__device__ __forceinline__ void write_spatial_observations_t(const Ctx& c, uint8_t* __restrict__ arena) {
  constexpr int CM = WATER ? 6 : 5;
  const int n = c.P.n, HW = c.P.HW;
  const uint32_t* cells = R_CELLS(c);
  const SpatialOut o = spatial_out<WATER>(c, arena);
  if (c.P.c.full_observability) {
    // layout_from_file.py:466-472: every agent gets the whole map (CM channels, no in-bounds
    // channel) and the owner / occupant planes with its own id replaced by 1
    const uint32_t* lm4f = reinterpret_cast<const uint32_t*>(c.locmap);
    for (int i = 0; i < n; ++i) {
      const int so = i * CM * HW * 4, si = i * 2 * HW * 2;
      for (int q = c.tid; q < (HW >> 2); q += AIE_NT) {
        const uint4 cw = reinterpret_cast<const uint4*>(cells)[q];
        const uint32_t cws[4] = {cw.x, cw.y, cw.z, cw.w};
        float ch[4][6];
#pragma unroll
        for (int u = 0; u < 4; ++u) cell_channels<WATER>(cws[u], ch[u]);
#pragma unroll
        for (int k = 0; k < CM; ++k) buf_store_f32x4(o.amap, ch[0][k], ch[1][k], ch[2][k], ch[3][k], 16 * q, so + k * HW * 4);
        const uint32_t occ4 = lm4f[q];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int own = AIE_CELL_OWNER(cws[u]);
          int v0 = own >= 0 ? own + 2 : 0;
          const int occ = (int)((occ4 >> (8 * u)) & 0xffu);
          int v1 = occ ? occ + 1 : 0;
          if (v0 == i + 2) v0 = 1;
          if (v1 == i + 2) v1 = 1;
          buf_store_i16(o.aidx, v0, 8 * q + 2 * u, si);
          buf_store_i16(o.aidx, v1, 8 * q + 2 * u, si + HW * 2);
        }
      }
      for (int cell = 4 * (HW >> 2) + c.tid; cell < HW; cell += AIE_NT) {  // tail cells
        float ch[6];
        const uint32_t cw = cells[cell];
        cell_channels<WATER>(cw, ch);
#pragma unroll
        for (int k = 0; k < CM; ++k) buf_store_f32(o.amap, ch[k], 4 * cell, so + k * HW * 4);
        const int own = AIE_CELL_OWNER(cw);
        int v0 = own >= 0 ? own + 2 : 0;
        const int occ = c.locmap[cell];
        int v1 = occ ? occ + 1 : 0;
        if (v0 == i + 2) v0 = 1;
        if (v1 == i + 2) v1 = 1;
        buf_store_i16(o.aidx, v0, 2 * cell, si);
        buf_store_i16(o.aidx, v1, 2 * cell, si + HW * 2);
      }
    }
  } else {
    for (int i = 0; i < n; ++i) crop_agent<WATER>(c, o, i);
  }
  if (c.P.c.planner_gets_spatial_info) {
    // f32 channel planes: 4 consecutive cells per lane -> CM 16-byte stores.  The planes
    // are only dword-aligned (H*W need not be a multiple of 4): dwordx4 stores need no more
    // than that on gfx950.  The i16 owner / location planes of the same 4 cells: 8-byte stores.
    const int nq4 = HW >> 2;
    const uint32_t* lm4 = reinterpret_cast<const uint32_t*>(c.locmap);
    for (int q = c.tid; q < nq4; q += AIE_NT) {
      const uint4 cw = reinterpret_cast<const uint4*>(cells)[q];
      const uint32_t cws[4] = {cw.x, cw.y, cw.z, cw.w};
      float ch[4][6];
#pragma unroll
      for (int u = 0; u < 4; ++u) cell_channels<WATER>(cws[u], ch[u]);
#pragma unroll
      for (int k = 0; k < CM; ++k) buf_store_f32x4(o.pmap, ch[0][k], ch[1][k], ch[2][k], ch[3][k], 16 * q, k * HW * 4);
      const uint32_t occ4 = lm4[q];
      uint32_t ow[2], oc[2];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int own = AIE_CELL_OWNER(cws[u]);
        const uint32_t vo = (uint32_t)(own >= 0 ? own + 2 : 0);
        const uint32_t occ = (occ4 >> (8 * u)) & 0xffu;
        const uint32_t vc = occ ? occ + 1 : 0;
        if (u & 1) { ow[u >> 1] |= vo << 16; oc[u >> 1] |= vc << 16; }
        else { ow[u >> 1] = vo; oc[u >> 1] = vc; }
      }
      buf_store_u32x2(o.pidx, ow[0], ow[1], 8 * q, 0);
      if ((HW & 1) == 0) {  // second plane starts 4-byte aligned too
        buf_store_u32x2(o.pidx, oc[0], oc[1], 8 * q, HW * 2);
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) buf_store_i16(o.pidx, (int)((oc[u >> 1] >> (16 * (u & 1))) & 0xffffu), 8 * q + 2 * u, HW * 2);
      }
    }
    for (int cell = 4 * nq4 + c.tid; cell < HW; cell += AIE_NT) planner_cell<WATER>(c, o, cell);  // tail cells
  }
}

// one cell of agent i's whole-map observation (full_observability, layout_from_file.py:466-472)
template <bool WATER>
__device__ __forceinline__ void agent_full_cell(const Ctx& c, const SpatialOut& o, int i, int cell) {
  constexpr int CM = WATER ? 6 : 5;
  const int HW = c.P.HW;
  const int so = i * CM * HW * 4, si = i * 2 * HW * 2;
  float ch[6];
  const uint32_t cw = R_CELLS(c)[cell];
  cell_channels<WATER>(cw, ch);
#pragma unroll
  for (int k = 0; k < CM; ++k) buf_store_f32(o.amap, ch[k], 4 * cell, so + k * HW * 4);
  const int own = AIE_CELL_OWNER(cw);
  int v0 = own >= 0 ? own + 2 : 0;
  const int occ = c.locmap[cell];
  int v1 = occ ? occ + 1 : 0;
  if (v0 == i + 2) v0 = 1;
  if (v1 == i + 2) v1 = 1;
  buf_store_i16(o.aidx, v0, 2 * cell, si);
  buf_store_i16(o.aidx, v1, 2 * cell, si + HW * 2);
}

// Incremental form of write_spatial_observations: the tensors still hold the previous step's
// values; rewrite the crops of the agents that moved and every item that shows one of the
// cells the dynamics logged (dirty_*).  One lane per logged cell.
template <bool WATER>
__device__ __forceinline__ void update_spatial_observations_t(const Ctx& c, uint8_t* __restrict__ arena) {
  const int n = c.P.n, W = c.P.W, WV = c.P.WV, w = c.P.c.obs_range;
  const int cnt = uni(c.dirty[0]);
  if (cnt > AIE_DIRTY_CAP) {  // log overflow: start over
    write_spatial_observations_t<WATER>(c, arena);
    return;
  }
  const SpatialOut o = spatial_out<WATER>(c, arena);
  const uint32_t mv0 = (uint32_t)uni(c.dirty[1]), mv1 = (uint32_t)uni(c.dirty[2]);
  const uint16_t* dl = dirty_list(c);
  const int cell = c.tid < cnt ? (int)dl[c.tid] : -1;  // AIE_DIRTY_CAP == wave size
  const int r = cell >= 0 ? udiv(cell, W, c.P.mg_W) : 0, col = cell - r * W;
  for (int i = 0; i < n; ++i) {
    if (c.P.c.full_observability) {
      if (cell >= 0) agent_full_cell<WATER>(c, o, i, cell);
      continue;
    }
    const bool moved = ((i < 32 ? mv0 >> i : mv1 >> (i - 32)) & 1u) != 0;
    if (moved) {
      crop_agent<WATER>(c, o, i);
    } else if (cell >= 0) {
      const int dr = r - (R_I32(c, o_loc_r)[i] - w), dc = col - (R_I32(c, o_loc_c)[i] - w);
      if (dr >= 0 && dr < WV && dc >= 0 && dc < WV) crop_item<WATER>(c, o, i, dr * WV + dc, r, col);
    }
  }
  if (c.P.c.planner_gets_spatial_info && cell >= 0) planner_cell<WATER>(c, o, cell);
}
__device__ __forceinline__ void write_spatial_observations(const Ctx& c, uint8_t* __restrict__ arena) {
  if (c.P.c.has_water) write_spatial_observations_t<true>(c, arena);
  else write_spatial_observations_t<false>(c, arena);
}
__device__ __forceinline__ void update_spatial_observations(const Ctx& c, uint8_t* __restrict__ arena) {
  if (c.P.c.has_water) update_spatial_observations_t<true>(c, arena);
  else update_spatial_observations_t<false>(c, arena);
}

// ---- the parts of the flat vectors that write_flat_observations and update_flat_observations both write; the planner's
// vector and its per-agent fragments arrive as pointers (LDS staging in the former, the tensors in the latter) ----
__device__ __forceinline__ void flat_a(const BufRsrc& aflat, int idx, float v) { buf_store_f32(aflat, v, 4 * idx, 0); }

__device__ __forceinline__ float flat_time_value(const Ctx& c) {
  const int t = *R_I32(c, o_timestep);
  return (float)((double)t / (c.P.c.allow_observation_scaling ? (double)c.R.c.episode_length : 1.0));
}

// Agent i's block: what the record holds behind time / world-* and the marginal rate, loaded ahead of the caller's own
// stores; q = the planner's p{i}.
struct AgentScalars {
  double coin; int inv0, inv1, lr, lc;
  __device__ __forceinline__ AgentScalars(const Ctx& c, int i)
      : coin(R_F64(c, o_inv_coin)[i]), inv0(R_I32(c, o_inv_res)[i]), inv1(R_I32(c, o_inv_res)[c.P.n + i]),
        lr(R_I32(c, o_loc_r)[i]), lc(R_I32(c, o_loc_c)[i]) {}
  // time and world-* of the agent's vector, their copy in p{i}, obs_a_time
  __device__ __forceinline__ void write(const Ctx& c, uint8_t* __restrict__ arena, const BufRsrc& aflat, float* q, int i,
                                        float tval, double isc) const {
    const aie_params& P = c.P;
    const int f0 = i * P.FA;
    flat_a(aflat, f0 + P.fa_time, tval);
    const float w0 = (float)(coin * isc);
    const float w1 = (float)((double)inv0 * isc);
    const float w2 = (float)((double)inv1 * isc);
    const float w3 = (float)((double)lc / (double)P.W);
    const float w4 = (float)((double)lr / (double)P.H);
    flat_a(aflat, f0 + P.fa_world + 0, w0); flat_a(aflat, f0 + P.fa_world + 1, w1); flat_a(aflat, f0 + P.fa_world + 2, w2);
    if (!P.c.full_observability) {  // locations and the planner's per-agent fragments: egocentric mode only
      flat_a(aflat, f0 + P.fa_world + 3, w3); flat_a(aflat, f0 + P.fa_world + 4, w4);
      q[P.fpa_world + 0] = w0; q[P.fpa_world + 1] = w1; q[P.fpa_world + 2] = w2;
      if (P.c.planner_gets_spatial_info) { q[P.fpa_world + 3] = w3; q[P.fpa_world + 4] = w4; }
    }
    reinterpret_cast<float*>(arena + c.R.a_obs_a_time)[(int64_t)c.e * P.n + i] = tval;
  }
  // the current marginal rate: the agent's own vector and p{i}
  __device__ __forceinline__ void write_marginal_rate(const Ctx& c, const BufRsrc& aflat, float* q, int i) const {
    const double cmr = tax_marginal_rate(c, (coin + R_F64(c, o_esc_coin)[i]) - R_F64(c, o_tax_last_coin)[i]);
    flat_a(aflat, i * c.P.FA + c.P.fa_tax + AIE_FA_TAX_MARGINAL_RATE(c.P.NB, c.P.n), (float)cmr);
    q[c.P.fpa_tax + AIE_FPA_TAX_CURR_MARGINAL_RATE] = (float)cmr;
  }
};
// Net price history of column (commodity r, price k): np.sum(np.stack(...), axis=0) adds row by row, from the first
// row's value and not from 0.  row(at) runs on every agent's entry `at` of the [2][n][P] record tables along the way.
template <class Row>
__device__ __forceinline__ double price_history_column(const Ctx& c, int r, int k, Row row) {
  double s = 0;
  for (int i = 0; i < c.P.n; ++i) {
    const int at = (r * c.P.n + i) * c.P.P + k;
    const double v = R_F64(c, o_cda_price_history)[at];
    s = (i == 0) ? v : s + v;
    row(at);
  }
  return s;
}
// market_rate of commodity r from the column sums in scr_net_ph (continuous_double_auction.py:491-542); tot = their sum
__device__ __forceinline__ float cda_market_rate(const Ctx& c, int r, double& tot) {
  const double* a = scr_net_ph(c) + r * c.P.P;
  double dot = 0;
  for (int k = 0; k < c.P.P; ++k) dot += (double)k * a[k];
  tot = np_sum_small(a, c.P.P);
  return (float)(dot / (tot > 0.001 ? tot : 0.001));
}
// the tax calendar (redistribution.py:974-1023)
struct TaxCalendar { float is_tax_day, is_first_day, tax_phase; };
__device__ __forceinline__ TaxCalendar tax_calendar(const Ctx& c) {
  const int pos = *R_I32(c, o_tax_cycle_pos);
  return {pos >= c.R.c.tax_period ? 1.0f : 0.0f, pos == 1 ? 1.0f : 0.0f, (float)((double)pos / (double)c.R.c.tax_period)};
}

// Component + scalar observations, packed in SORTED key order (base_env.py:561-612):
// Build (build.py:163-178), CDA (continuous_double_auction.py:491-542), Gather
// (move.py:155-165), PeriodicBracketTax (redistribution.py:974-1023), time, world-*.
// Built in LDS (c.stage) then streamed out.
__device__ __forceinline__ void write_flat_observations(const Ctx& c, uint8_t* __restrict__ arena) {
  const aie_params& P = c.P;
  const int n = P.n, tid = c.tid, Pp = P.P, NB = P.NB;
  const double isc = P.c.allow_observation_scaling ? 0.01 : 1.0;
  // The agents' vectors (n x FA floats) go straight to HBM through a buffer descriptor; only the
  // planner's vector (read back by the agents' CDA fragment) and its per-agent fragments are
  // staged in LDS, behind the components' draw window (the first region of the staging area, see step_body).
  float* s_pag = c.stage + stage_window_words(P);
  float* s_pflat = s_pag + pad4(n * P.FPA);
  const BufRsrc aflat = make_rsrc(arena + c.R.a_obs_a_flat + (int64_t)c.e * n * P.FA * 4, (uint32_t)(n * P.FA * 4));
  auto AF = [&](int idx, float v) { flat_a(aflat, idx, v); };
  const float tval = flat_time_value(c);

  const int skip = c.skipm;
  // ================= stage A: per-(commodity, price) sums, per-agent scalars ===========
  if (P.has_cda && !(skip & AIE_DEV_SKIP_FLAT_STAGE_A)) {
    // lanes over (commodity r, price k): net price history and full bid / ask histograms
    double* net_ph = scr_net_ph(c);
    for (int q = tid; q < 2 * Pp; q += AIE_NT) {
      const int r = q >= Pp ? 1 : 0, k = q - r * Pp;
      int fa = 0, fb = 0;
      const double s = price_history_column(
          c, r, k, [&](int at) { fa += R_U8(c, o_cda_ask_hist)[at], fb += R_U8(c, o_cda_bid_hist)[at]; });
      net_ph[q] = s;
      float* g = s_pflat + P.fp_cda;
      g[AIE_FP_CDA_FULL_ASKS(Pp) + q] = (float)fa;
      g[AIE_FP_CDA_FULL_BIDS(Pp) + q] = (float)fb;
      g[AIE_FP_CDA_PRICE_HISTORY(Pp) + q] = (float)(s * isc);
    }
  }
  if (tid < n && !(skip & AIE_DEV_SKIP_FLAT_STAGE_A)) {
    const int i = tid;
    const int f0 = i * P.FA;
    const AgentScalars a(c, i);
    if (P.has_build) {  // build.py:163-178
      AF(f0 + P.fa_build + 0, (float)(R_F64(c, o_build_payment)[i] / (double)c.R.c.build_payment));
      AF(f0 + P.fa_build + 1, (float)R_F64(c, o_build_skill)[i]);
    }
    if (P.has_gather) AF(f0 + P.fa_gather, (float)R_F64(c, o_bonus_gather_prob)[i]);  // move.py:155-165
    float* q = s_pag + i * P.FPA;
    a.write(c, arena, aflat, q, i, tval, isc);
    if (P.has_tax) {
      // last_incomes sorted ascending (redistribution.py:908-911): rank by counting
      const double per = (double)c.R.c.tax_period;
      const double x = R_F64(c, o_tax_last_income)[i] / per;
      double* xs = scr_cmr(c);  // (free until the rewards: one division per agent, not one per pair)
      xs[i] = x;
      AIE_WSYNC();
      int rank = 0;
      for (int j = 0; j < n; ++j) {
        const double y = xs[j];
        rank += (y < x || (y == x && j < i)) ? 1 : 0;
      }
      scr_sorted_inc(c)[rank] = x;
      a.write_marginal_rate(c, aflat, q, i);
      q[P.fpa_tax + AIE_FPA_TAX_LAST_INCOME] = (float)x;
      q[P.fpa_tax + AIE_FPA_TAX_LAST_MARGINAL_RATE] = (float)R_F64(c, o_tax_last_marginal_rate)[i];
    }
  }
  if (tid == 0) {
    s_pflat[P.fp_time] = tval;
    s_pflat[P.fp_world + 0] = 0.0f;  // the planner's inventory never changes
    s_pflat[P.fp_world + 1] = 0.0f;
    s_pflat[P.fp_world + 2] = 0.0f;
    reinterpret_cast<float*>(arena + c.R.a_obs_p_time)[c.e] = tval;
  }
  AIE_WSYNC();

  // ================= stage B: fill the vectors, one lane per element =====================
  if (P.has_cda && !(skip & AIE_DEV_SKIP_FLAT_CDA)) {
    // continuous_double_auction.py:491-542
    if (tid < 2) {
      const int r = tid;
      double tot;
      const float mr = cda_market_rate(c, r, tot);
      s_pflat[P.fp_cda + AIE_FP_CDA_MARKET_RATE(Pp) + r] = mr;
      for (int i = 0; i < n; ++i) AF(i * P.FA + P.fa_cda + AIE_FA_CDA_MARKET_RATE(Pp) + r, mr);
    }
    const float* g = s_pflat + P.fp_cda;
    for (int it = tid; it < n * 2 * Pp; it += AIE_NT) {
      const int i = udiv(it, 2 * Pp, P.mg_2P);
      const int q = it - i * 2 * Pp;  // (commodity, price)
      const int r = q >= Pp ? 1 : 0, k = q - r * Pp;
      const float mya = (float)R_U8(c, o_cda_ask_hist)[(r * n + i) * Pp + k];
      const float myb = (float)R_U8(c, o_cda_bid_hist)[(r * n + i) * Pp + k];
      const int fc = i * P.FA + P.fa_cda;
      AF(fc + AIE_FA_CDA_AVAILABLE_ASKS(Pp) + q, g[AIE_FP_CDA_FULL_ASKS(Pp) + q] - mya);
      AF(fc + AIE_FA_CDA_AVAILABLE_BIDS(Pp) + q, g[AIE_FP_CDA_FULL_BIDS(Pp) + q] - myb);
      AF(fc + AIE_FA_CDA_MY_ASKS(Pp) + q, mya);
      AF(fc + AIE_FA_CDA_MY_BIDS(Pp) + q, myb);
      AF(fc + AIE_FA_CDA_PRICE_HISTORY(Pp) + q, g[AIE_FP_CDA_PRICE_HISTORY(Pp) + q]);
    }
  }
  if (P.has_tax && !(skip & AIE_DEV_SKIP_FLAT_TAX)) {
    // redistribution.py:974-1023; lanes over (agent or planner, element of the fragment)
    const TaxCalendar cal = tax_calendar(c);
    const int fragA = AIE_FA_TAX_LEN(NB, n);
    for (int q = tid; q < (n + 1) * fragA; q += AIE_NT) {
      const int i = udiv(q, fragA, P.mg_taxA);
      const int j = q - i * fragA;
      const bool planner = i == n;
      if (j == AIE_FA_TAX_MARGINAL_RATE(NB, n)) {  // written in stage A (agents), absent for the planner
        if (planner) s_pflat[P.fp_tax + AIE_FP_TAX_PHASE(NB, n)] = cal.tax_phase;
        continue;
      }
      if (planner && j == AIE_FA_TAX_PHASE(NB, n)) continue;
      float v;
      if (j < AIE_F_TAX_IS_FIRST_DAY(NB)) v = (float)tax_rate_obs(c, j - AIE_F_TAX_CURR_RATES);
      else if (j == AIE_F_TAX_IS_FIRST_DAY(NB)) v = cal.is_first_day;
      else if (j == AIE_F_TAX_IS_TAX_DAY(NB)) v = cal.is_tax_day;
      else if (j < AIE_FA_TAX_MARGINAL_RATE(NB, n)) v = (float)scr_sorted_inc(c)[j - AIE_F_TAX_LAST_INCOMES(NB)];
      else v = cal.tax_phase;
      if (planner) s_pflat[P.fp_tax + j] = v;  // (AIE_F_TAX_*: the same place in both blocks)
      else AF(i * P.FA + P.fa_tax + j, v);
    }
  }

  AIE_WSYNC();

  // ---- stream the staged vectors out: 16-byte LDS reads, dword-aligned 16-byte stores ----
  if (!(skip & AIE_DEV_SKIP_PLANNER_COPY_OUT)) {
    stream_out(s_pag, reinterpret_cast<float*>(arena + c.R.a_obs_p_agents) + (int64_t)c.e * n * P.FPA, n * P.FPA, tid);
    stream_out(s_pflat, reinterpret_cast<float*>(arena + c.R.a_obs_p_flat) + (int64_t)c.e * P.FP, P.FP, tid);
  }
}

// Incremental form of write_flat_observations (what update_spatial_observations is to the maps): the tensors still hold
// the previous step's vectors, and a whole step changes few of their entries -- on BASELINE configs[1] about 10 of an
// agent's 136 floats.  Written on every step, untracked: time, the world scalars, the current marginal rate, the tax
// calendar (first day, tax day, phase), and a price-history column / a market rate whose sum is nonzero (a zero sum
// means no trade since the reset, whose full rewrite stored the zeros; 0.995^t never reaches zero from above before
// its float32 image has).  Written when the CDA component touched them (Agents::hist_dirty): the order-count columns
// -- one lane per (commodity, price) rewrites the 2n + 1 entries per side that show its column.  Never: build payment,
// skill, gather bonus, the planner's inventory (resets only).  The tax block's slow entries (rates, sorted incomes, the
// planner's per-agent last income / last marginal rate) change on two steps of a tax period: step_body sends those
// steps down the full path instead (Agents::tax_dirty), as it does with everything that obs_valid == 0 stands for.
// No LDS staging: every entry goes straight to the tensors.
__device__ __forceinline__ void update_flat_observations(const Ctx& c, uint8_t* __restrict__ arena, uint64_t hist_dirty) {
  const aie_params& P = c.P;
  const int n = P.n, tid = c.tid, Pp = P.P, NB = P.NB;
  const double isc = P.c.allow_observation_scaling ? 0.01 : 1.0;
  const BufRsrc aflat = make_rsrc(arena + c.R.a_obs_a_flat + (int64_t)c.e * n * P.FA * 4, (uint32_t)(n * P.FA * 4));
  auto AF = [&](int idx, float v) { flat_a(aflat, idx, v); };
  float* const pflat = reinterpret_cast<float*>(arena + c.R.a_obs_p_flat) + (int64_t)c.e * P.FP;
  float* const pag = reinterpret_cast<float*>(arena + c.R.a_obs_p_agents) + (int64_t)c.e * n * P.FPA;
  const float tval = flat_time_value(c);
  const int skip = c.skipm;
  if (P.has_cda && !(skip & AIE_DEV_SKIP_FLAT_STAGE_A)) {
    // lanes over (commodity r, price k): the column's net price history; its order counts where they changed
    double* net_ph = scr_net_ph(c);
    for (int q = tid; q < 2 * Pp; q += AIE_NT) {
      const int r = q >= Pp ? 1 : 0, k = q - r * Pp;
      const double s = price_history_column(c, r, k, [](int) {});
      net_ph[q] = s;
      if (s != 0 && !(skip & AIE_DEV_SKIP_FLAT_CDA)) {
        const float v = (float)(s * isc);
        pflat[P.fp_cda + AIE_FP_CDA_PRICE_HISTORY(Pp) + q] = v;
        for (int i = 0; i < n; ++i) AF(i * P.FA + P.fa_cda + AIE_FA_CDA_PRICE_HISTORY(Pp) + q, v);
      }
#pragma unroll
      for (int side = 0; side < 2; ++side) {  // 0: asks, 1: bids
        if (!hist_col_dirty(P, hist_dirty, r, side, k) || (skip & AIE_DEV_SKIP_FLAT_CDA)) continue;
        const uint8_t* h = side ? R_U8(c, o_cda_bid_hist) : R_U8(c, o_cda_ask_hist);
        int f = 0;
        for (int i = 0; i < n; ++i) f += h[(r * n + i) * Pp + k];
        const float full = (float)f;
        pflat[P.fp_cda + (side ? AIE_FP_CDA_FULL_BIDS(Pp) : AIE_FP_CDA_FULL_ASKS(Pp)) + q] = full;
        for (int i = 0; i < n; ++i) {
          const float my = (float)h[(r * n + i) * Pp + k];
          const int fc = i * P.FA + P.fa_cda;
          AF(fc + (side ? AIE_FA_CDA_AVAILABLE_BIDS(Pp) : AIE_FA_CDA_AVAILABLE_ASKS(Pp)) + q, full - my);
          AF(fc + (side ? AIE_FA_CDA_MY_BIDS(Pp) : AIE_FA_CDA_MY_ASKS(Pp)) + q, my);
        }
      }
    }
  }
  if (tid < n && !(skip & AIE_DEV_SKIP_FLAT_STAGE_A)) {
    const int i = tid;
    const AgentScalars a(c, i);
    float* q = pag + i * P.FPA;
    a.write(c, arena, aflat, q, i, tval, isc);
    if (P.has_tax) a.write_marginal_rate(c, aflat, q, i);
  }
  if (tid == 0) {
    pflat[P.fp_time] = tval;
    reinterpret_cast<float*>(arena + c.R.a_obs_p_time)[c.e] = tval;
  }
  if (P.has_tax && !(skip & AIE_DEV_SKIP_FLAT_TAX)) {  // the calendar entries of the n agents' and the planner's tax block
    const TaxCalendar cal = tax_calendar(c);
    for (int i = tid; i <= n; i += AIE_NT) {
      if (i == n) {
        pflat[P.fp_tax + AIE_F_TAX_IS_FIRST_DAY(NB)] = cal.is_first_day;
        pflat[P.fp_tax + AIE_F_TAX_IS_TAX_DAY(NB)] = cal.is_tax_day;
        pflat[P.fp_tax + AIE_FP_TAX_PHASE(NB, n)] = cal.tax_phase;
      } else {
        AF(i * P.FA + P.fa_tax + AIE_F_TAX_IS_FIRST_DAY(NB), cal.is_first_day);
        AF(i * P.FA + P.fa_tax + AIE_F_TAX_IS_TAX_DAY(NB), cal.is_tax_day);
        AF(i * P.FA + P.fa_tax + AIE_FA_TAX_PHASE(NB, n), cal.tax_phase);
      }
    }
  }
  if (P.has_cda && !(skip & AIE_DEV_SKIP_FLAT_CDA)) {
    AIE_WSYNC();  // (net_ph)
    if (tid < 2) {
      const int r = tid;
      double tot;
      const float mr = cda_market_rate(c, r, tot);
      if (tot != 0) {
        pflat[P.fp_cda + AIE_FP_CDA_MARKET_RATE(Pp) + r] = mr;
        for (int i = 0; i < n; ++i) AF(i * P.FA + P.fa_cda + AIE_FA_CDA_MARKET_RATE(Pp) + r, mr);
      }
    }
  }
}


// Action masks (own staging slots, own per-agent mask bits): independent of the flat vectors
// above, so the second wave of a replica builds them while the first one does those.
// `all` == false (a step whose observation tensors still show the previous step): only what changed is rewritten -- the
// rows of the agents whose mask bits differ from the ones the tensor shows (record field o_mask_bits), the planner's when
// its "rates may be set today" flag flips (o_mask_p_open; which rates are visible only changes at a reset, and a reset
// writes everything).  Round 6: 1.4 KB of stores and ~100 vector instructions per replica-step less on BASELINE configs[1].
__device__ __forceinline__ void write_action_masks(const Ctx& c, uint8_t* __restrict__ arena, bool all = true) {
  const aie_params& P = c.P;
  const int n = P.n, tid = c.tid, Pp = P.P;
  const int skip = c.skipm;
  if (skip & AIE_DEV_SKIP_MASKS) return;
  if (!P.o_mask_bits) all = true;
  if (tid < n) {
    const int i = tid;
    const double coin = R_F64(c, o_inv_coin)[i];
    const int inv0 = R_I32(c, o_inv_res)[i], inv1 = R_I32(c, o_inv_res)[n + i];
    const int lr = R_I32(c, o_loc_r)[i], lc = R_I32(c, o_loc_c)[i];
    // mask bits: Build build.py:180-193, Gather move.py:167-188, CDA :544-580
    uint32_t mf = 0;
    if (P.has_build) mf |= agent_can_build(c, i) ? 1u : 0u;
    if (P.has_gather) {
      mf |= can_agent_occupy(c, lr, lc - 1, i) ? 2u : 0u;
      mf |= can_agent_occupy(c, lr, lc + 1, i) ? 4u : 0u;
      mf |= can_agent_occupy(c, lr - 1, lc, i) ? 8u : 0u;
      mf |= can_agent_occupy(c, lr + 1, lc, i) ? 16u : 0u;
    }
    if (P.has_cda) {
      int kmax = coin >= (double)(Pp - 1) ? Pp - 1 : (int)coin;  // price k is affordable iff k <= coin
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const bool quota = R_I32(c, o_cda_n_orders)[r * n + i] < P.c.cda_max_num_orders;
        if (quota && (r ? inv1 : inv0) > 0) mf |= 32u << r;
        if (quota) mf |= (uint32_t)(kmax + 1) << (8 + 8 * r);
      }
    }
    // bit 31 of the staged word: this agent's row has to be written
    const bool changed = all || (int32_t)mf != R_I32(c, o_mask_bits)[i];
    if (P.o_mask_bits) R_I32(c, o_mask_bits)[i] = (int32_t)mf;
    c.mflags[i] = (int32_t)(mf | (changed ? 0x80000000u : 0u));
  }
  AIE_WSYNC();
  // ---- masks: _generate_masks base_env.py:706-756 + flatten_masks base_agent.py:440-460,
  // planner PeriodicBracketTax.generate_masks redistribution.py:1025-1104 ----
  // Element m of the flattened mask means the same thing for every agent: one host-built (shift, mask, threshold)
  // test against each agent's mask bits.  Written straight from registers: lane q owns elements 4q .. 4q + 3 of the
  // replica's [n][MA] block (dword-aligned 16-byte stores).
  {
    float* dst = reinterpret_cast<float*>(arena + c.R.a_obs_a_mask) + (int64_t)c.e * n * P.MA;
    const int count = n * P.MA;
    auto elem = [&](int idx) -> float {
      const int i = udiv(idx, P.MA, P.mg_MA), m = idx - i * P.MA;
      const uint32_t t = c.mtab[m];  // host-built test for element m (aie_layout.h)
      const uint32_t sh = t & 31u, msk = (t >> 8) & 0xffu, thr = t >> 16;
      return (((uint32_t)c.mflags[i] >> sh) & msk) >= thr ? 1.0f : 0.0f;
    };
    auto dirty = [&](int idx) -> bool { return c.mflags[udiv(idx, P.MA, P.mg_MA)] < 0; };  // (bit 31)
    const int n4 = count >> 2;
    for (int q = tid; q < n4; q += AIE_NT) {
      if (!all && !dirty(4 * q) && !dirty(4 * q + 3)) continue;  // (a quad spans at most two agents' rows)
      f32x4_a4 o = {elem(4 * q), elem(4 * q + 1), elem(4 * q + 2), elem(4 * q + 3)};
      reinterpret_cast<f32x4_a4*>(dst)[q] = o;
    }
    for (int q = 4 * n4 + tid; q < count; q += AIE_NT)
      if (all || dirty(q)) dst[q] = elem(q);
    float* pdst = reinterpret_cast<float*>(arena + c.R.a_obs_p_mask) + (int64_t)c.e * P.MP;
    const bool pmulti = P.c.multi_action_mode_planner != 0;
    const float open = (P.n_sub_p && *R_I32(c, o_tax_cycle_pos) == 1) ? 1.0f : 0.0f;
    if (P.o_mask_bits) {
      const int was = uni(*R_I32(c, o_mask_p_open));
      AIE_WSYNC();
      if (tid == 0) *R_I32(c, o_mask_p_open) = open != 0.0f ? 1 : 0;
      if (!all && was == (open != 0.0f ? 1 : 0)) return;
    }
    for (int q = tid; q < P.MP; q += AIE_NT) {
      float v;
      int j = -1;  // index of the discretised rate this entry stands for (-1: a NO-OP entry, or a foreign row's)
      if (P.n_sub_p == 0) j = -1;
      else if (c.full && P.n_host_p) {
        // the tax block sits at tax_p_moff among foreign rows (aie_layout.h): everything outside it is written as 1.0
        // (the host puts its components' masks there behind the launch)
        const int w = pmulti ? 1 + P.sub_p_dim : P.sub_p_dim, tq = q - P.tax_p_moff;
        if (tq >= 0 && tq < P.n_sub_p * w) j = tq - udiv(tq, w, pmulti ? P.mg_sub_p : P.mg_sub_p_dim) * w - (pmulti ? 1 : 0);
      }
      else if (pmulti) j = q - udiv(q, 1 + P.sub_p_dim, P.mg_sub_p) * (1 + P.sub_p_dim) - 1;
      else if (q > 0) j = (q - 1) - udiv(q - 1, P.sub_p_dim, P.mg_sub_p_dim) * P.sub_p_dim;
      if (j < 0) v = 1.0f;
      else v = (open != 0.0f && tax_rate_action_visible(c, j)) ? 1.0f : 0.0f;
      pdst[q] = v;
    }
  }
}

__device__ __forceinline__ void rebuild_locmap(const Ctx& c) {
  uint32_t* lm = reinterpret_cast<uint32_t*>(c.locmap);
  const int nw = (c.P.HW + 3) >> 2;
  for (int q = c.tid; q < nw; q += AIE_NT) lm[q] = 0;
  AIE_WSYNC();
  if (c.tid < c.P.n) {
    const int r = R_I32(c, o_loc_r)[c.tid], col = R_I32(c, o_loc_c)[c.tid];
    if (r >= 0 && col >= 0) c.locmap[r * c.P.W + col] = (uint8_t)(c.tid + 1);
  }
  AIE_WSYNC();
}

// The replica's source doubles from the cells' flag bytes (LDS image), ascending: Wood cells, then Stone cells
// (layout_from_file.py:394-403: np.random.rand(2, H, W) is consumed for Wood first).  One wave; count and list go to
// the record in HBM (o_src_n, o_src_list; a count above AIE_SRC_CAP selects the row-by-row regeneration).
__device__ __forceinline__ void build_src_list(const Ctx& c, uint8_t* __restrict__ arena) {
  if (!c.P.o_src_list) return;
  const int HW = c.P.HW;
  uint8_t* g = arena + (int64_t)c.e * c.P.rec_bytes;
  uint16_t* lst = reinterpret_cast<uint16_t*>(g + c.P.o_src_list);
  const uint8_t* cb = reinterpret_cast<const uint8_t*>(R_CELLS(c));
  for (int k = c.tid; k < AIE_SRC_CAP; k += AIE_NT) lst[k] = 0;
  int base = 0;
  for (int rs = 0; rs < 2; ++rs) {
    const uint32_t bit = rs == 0 ? AIE_CELL_WOOD_SRC : AIE_CELL_STONE_SRC;
    for (int q0 = 0; q0 < HW; q0 += AIE_NT) {
      const int q = q0 + c.tid;
      const bool on = q < HW && (cb[4 * q + 3] & bit);
      const uint64_t mask = __ballot(on);
      const int slot = base + __popcll(mask & lanemask_lt(c.tid));
      if (on && slot < AIE_SRC_CAP) lst[slot] = (uint16_t)(rs * HW + q);
      base += __popcll(mask);
    }
  }
  if (c.tid == 0) *reinterpret_cast<int32_t*>(g + c.P.o_src_n) = base;
}

}  // namespace aie

// ======================================================================================
// Kernels
// ======================================================================================

// BaseEnvironment.step, F/base/base_env.py:929-1032: parse actions, timestep += 1,
// components in list order, scenario_step, observations, masks, rewards, done.
//
// A replica is a workgroup of TWO wavefronts sharing the LDS record.
//   both   record HBM -> LDS (alternate 16-byte units)  ||  wave 1 also: the next 128+ tempered MT19937 words ->
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
#ifdef AIE_W0_TAIL_PRIO  // (A/B builds)
  const int w0_tail_prio = AIE_W0_TAIL_PRIO;
#else
  const int w0_tail_prio = P.n >= 8 ? 2 : 0;
#endif
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
    if (!(skip & AIE_DEV_SKIP_ACTION_DECODE)) act_err = decode_actions(c, A, act_a, act_p, arena);  // (c.act_p is LDS scratch)
    else A.act = 0;
    if (TRACE && R.dev_trace && c.tid == 0) R.dev_trace[12 * blockIdx.x] = wall_clock64();
    if (TRACE && R.dev_trace && c.tid == 0) R.dev_trace[12 * blockIdx.x + 9] = wall_clock64();
    // (round 6, tools/ab2.sh: requesting the action words and the wave's whole share of the image before anything waits
    // -- the loop below comes out as load, wait, LDS write per unit, behind decode_actions' two load-wait-decode rounds --
    // made the launch SLOWER, 22.5 -> 23.5 us, and so did milder orders (both action loads first: 22.7; the record ahead of
    // the decode: 22.9): 4096 workgroups start together, and what their first microseconds are short of is the memory
    // system's capacity for requests, not patience -- the loop's own pace spreads them)
    MT none;
    load_record(c, arena, none, 0, 2, /*key_wave=*/-1);
    __syncthreads();  // (2) the record is in LDS
    if (TRACE && R.dev_trace && c.tid == 0) R.dev_trace[12 * blockIdx.x + 8] = wall_clock64();
    MTL ml{draw_w, 0, 0u, -AIE_MT_N, 0, 0u, 0u, 0, 0, 0, FAST ? reinterpret_cast<uint32_t*>(c.rec + P.o_mt) : gkey, draw_cap, FAST};
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
    load_record(c, arena, m, 1, 2, /*key_wave=*/-1);
    // behind its share of the copy: the words the components will draw -> the LDS draw window (two or three rows of the
    // generator's state, fetched from HBM; the state itself follows while the components run)
    if (skip & AIE_DEV_SKIP_DRAW_WINDOW) {}  // (development: the load phase without the draw window)
    else if (FAST) draw_window_publish_fast(draw_w, draw_cap, (uint32_t)uni((int)gkey[0]), (uint32_t)uni((int)gkey[1]), (uint32_t)uni((int)gkey[2]), uni(gpos), c.tid);
    else draw_window_publish_from_hbm(draw_w, draw_cap, gkey, uni(gpos), c.tid);

    if (SPEC >= 0 && const_tables_in_lds(P)) {
      // the small constant tables (Ctx.rtab / mtab) -> LDS, published by the barrier below
      if (P.has_tax && P.c.tax_model == AIE_TAX_MODEL_WRAPPER)
        for (int q = c.tid; q < P.c.tax_n_disc_rates; q += AIE_NT) const_cast<double*>(c.rtab)[q] = R.c.tax_disc_rates[q];
      for (int q = c.tid; q < P.MA; q += AIE_NT) const_cast<uint32_t*>(c.mtab)[q] = P.mask_test[q];
    }
    __syncthreads();  // (2)
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
#ifndef AIE_NO_TABLE_TOUCH  // (A/B builds)
    const uint32_t warm = glibc_tables_touch(c.tid);
#else
    const uint32_t warm = 0;
#endif
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
#ifdef AIE_W1_TAIL_PRIO  // (A/B builds)
    __builtin_amdgcn_s_setprio(AIE_W1_TAIL_PRIO);
#else
    // A batch that fits the device in one go (4096 workgroups at 8 waves per SIMD) is a race to the last workgroup's end:
    // from here on this wave is the critical one (the first has slack) and goes ahead of the waves still loading.  A
    // larger batch is a stream of workgroups, bound by the vector pipes: there a raised tail only delays the next
    // workgroups' start (tools/ab2.sh, round 6: 16 384 replicas 74.5 -> 72.8 us without it, 65 536: 318 -> 314 us;
    // 4096: 22.5 -> 23.0 us WITHOUT it).
    if (next.E > 6144) __builtin_amdgcn_s_setprio(0);
    else __builtin_amdgcn_s_setprio(2);
#endif
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
      if (!(skip & AIE_DEV_SKIP_REGEN)) scenario_step_regen(c, m, src);
      if (c.tid == 0) {
        *R_I32(c, o_mt_pos) = m.pos;
        if (FAST) R_U32(c, o_mt)[1] = m.fblk;
      }
      if (!(skip & AIE_DEV_SKIP_RECORD_STORE)) store_generator_rows(c, arena, m);  // (the rows' registers are free from here on)
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

namespace aie {
// ------------------------------------------------------------------------------------------------------------------
// Reset-time source layouts (uniform/, quadrant/, multi_zone/): FOUR wavefronts per replica.
//
// The algorithm (dynamic_layout.py:313-392) is a chain of whole-plane passes -- rand plane, threshold search, growth by
// 7x7 random-kernel convolutions, coverage check, retry -- whose lengths depend on the draws, so one replica's
// generation cannot be cut shorter than its chain; a masked reset lasts as long as its slowest replica (82 of 4096
// replicas per reset at BASELINE configs[0]'s scenario: round 2's single wave took 0.26 ms on average and 1.2 ms for
// the slowest).  What shortens the chain is running every plane pass cell-parallel over LG_NW x 64 lanes:
//   * every wave keeps its own copy of the generator (three consecutive windows in registers) and advances it
//     identically, so no random word ever crosses a wave boundary;
//   * rand planes: 256 doubles per pass; legacy_gauss: 256 polar attempts per pass (an attempt's acceptance does not
//     depend on the others; the waves exchange their 64-bit accept masks through LDS, rank the accepted attempts with
//     a prefix over the masks and stop behind the attempt that completes the request, cache semantics included);
//   * the threshold search ("tmp *= 0.9 until enough cells pass") advances every cell eight iterations at a time in
//     registers and finds the stopping iteration from eight per-iteration counters: one barrier pair per eight
//     iterations instead of an LDS round trip + ballot per iteration;
//   * convolutions and coverage counts: one cell per lane (15x15: 225 of 256 lanes), counts meet in LDS.
// Results are bit-identical to the sequential restatement (oracle/aie_oracle.c: layout_generate), which the CPU tests
// pin to the live reference: every draw is consumed at the same stream offset, np.mean of a 0/1 plane is count / size,
// signal.convolve2d(x, kernel, "same") is one add per kernel one in scipy's order over the zero-filled 7x7 window.
// ------------------------------------------------------------------------------------------------------------------
#define LG_NW 4
#ifdef AIE_DEV  // per-replica phase clocks of layout_generate (tools/c1_reset_trace.py): dev_trace[12 e + k]
#define LG_T0() const uint64_t lg_t0_ = wall_clock64()
#define LG_ACC(k) do { lg_acc[k] += wall_clock64() - lg_t0_; } while (0)
#define LG_CNT(k) do { lg_acc[k] += 1; } while (0)
#else
#define LG_T0() do { } while (0)
#define LG_ACC(k) do { } while (0)
#define LG_CNT(k) do { } while (0)
#endif

// Lane-parallel reads of the stream: a lane wants the word at stream offset o (counted from the start of window 0,
// o < 3 * 624).  Window k + 1 is the twisted copy of window k (valid for k < have); consuming words moves `pos`
// and shifts the windows down when it passes 624.  Everything here is wave-uniform except `o`.
struct MT3 {
  MT w[3];
  int have;  // valid windows (>= 1)
  int pos;   // next unused word of window 0
};
__device__ __forceinline__ void mt3_need(MT3& s, int k, int lane) {  // make windows 0..k valid (k <= 2)
  if (s.have <= 1 && k >= 1) {
    mt_copy(s.w[1], s.w[0]);
    mt_twist(s.w[1], lane);
    s.have = 2;
  }
  if (s.have <= 2 && k >= 2) {
    mt_copy(s.w[2], s.w[1]);
    mt_twist(s.w[2], lane);
    s.have = 3;
  }
}
// raw word i of one window for the lanes in `want` (a ballot; the lanes' rows lie in [rlo, rhi], wave-uniform)
__device__ __forceinline__ uint32_t mt3_window_word(const MT& m, int i, uint32_t v, bool mine, int rlo, int rhi) {
  const int row = i >> 6, ln = i & 63;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r >= rlo && r <= rhi) {  // (wave-uniform)
      const uint32_t t = lane_get(m.r[r], ln);
      v = (mine && row == r) ? t : v;
    }
  }
  return v;
}
// tempered word at offset o; o must be non-decreasing in the lane index (all call sites: o = base + stride * lane)
__device__ __forceinline__ uint32_t mt3_word(const MT3& s, int o) {
  const int win = o >= 2 * AIE_MT_N ? 2 : (o >= AIE_MT_N ? 1 : 0);
  const int i = o - win * AIE_MT_N;
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint64_t want = __ballot(win == k);
    if (want) {  // (wave-uniform) the first / last lane that reads this window bound the rows it touches
      const int first = __ffsll((unsigned long long)want) - 1, last = 63 - __clzll((long long)want);
      const int rlo = bcast(i, first) >> 6, rhi = bcast(i, last) >> 6;
      v = mt3_window_word(s.w[k], i, v, win == k, rlo, rhi);
    }
  }
  return mt_word(s.w[0], v);
}
// the four tempered words o .. o + 3 (one polar attempt): the window / row bookkeeping once for all four
__device__ __forceinline__ void mt3_words4(const MT3& s, int o, uint32_t out[4]) {
  uint32_t v[4] = {0, 0, 0, 0};
  int win[4], idx[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    win[j] = o + j >= 2 * AIE_MT_N ? 2 : (o + j >= AIE_MT_N ? 1 : 0);
    idx[j] = o + j - win[j] * AIE_MT_N;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint64_t want = __ballot(win[0] == k || win[3] == k);  // (offsets are monotone in the lane and in j)
    if (want) {
      const int first = __ffsll((unsigned long long)want) - 1, last = 63 - __clzll((long long)want);
      // rows touched in window k: from the first lane's first word that lies in it to the last lane's last word
      const int lo_i = bcast(win[0], first) == k ? bcast(idx[0], first) : 0;
      const int hi_i = bcast(win[3], last) == k ? bcast(idx[3], last) : AIE_MT_N - 1;
      const int rlo = lo_i >> 6, rhi = hi_i >> 6;
#pragma unroll
      for (int r = 0; r < 10; ++r) {
        if (r >= rlo && r <= rhi) {  // (wave-uniform)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t t = lane_get(s.w[k].r[r], idx[j] & 63);
            v[j] = (win[j] == k && (idx[j] >> 6) == r) ? t : v[j];
          }
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) out[j] = mt_word(s.w[0], v[j]);
}
__device__ __forceinline__ void mt3_consume(MT3& s, int nwords, int lane) {  // nwords <= 2 * 624
  s.pos += nwords;
  while (s.pos >= AIE_MT_N) {
    mt3_need(s, 1, lane);
    mt_copy(s.w[0], s.w[1]);
    mt_copy(s.w[1], s.w[2]);
    s.have -= 1;
    s.pos -= AIE_MT_N;
  }
}

struct LgShared {      // cross-wave scratch in LDS (behind the planes)
  int32_t cnt[2][LG_NW];    // block_count: per-wave counts, two parities
  uint32_t am[2][LG_NW][2]; // gauss: per-wave accept masks, two parities
  int32_t thr[32];          // threshold search: cells on after iteration k of the current block
  uint32_t kbits[2];        // growth kernel: sign bits of the 49 randn values
  double lcache;            // legacy_gauss's one-value cache of a layout stream of its own (aie_layout_stream): the
  int32_t lhas, lpad_;      //   replica's own cache, a record field, belongs to the replica's stream
};
__host__ __device__ inline size_t layout_gen_lds_bytes(const aie_params& P) {
  if (P.c.layout_gen == AIE_LAYOUT_FIXED) return 0;
  const size_t hwp = ((size_t)P.HW + 15) / 16 * 16;
  // tmp, x (f64), two byte planes, the multi_zone grid, the cross-wave scratch
  return 2 * hwp * 8 + 2 * hwp + 256 * 4 + ((sizeof(LgShared) + 15) / 16 * 16);
}
__device__ __forceinline__ LgShared* lg_shared(uint8_t* extra, const aie_params& P) {  // (layout_generate's carve-up of `extra`)
  const size_t hwp = ((size_t)P.HW + 15) / 16 * 16;
  return reinterpret_cast<LgShared*>(extra + 2 * hwp * 8 + 2 * hwp + 256 * 4);
}
// number of lanes of the whole workgroup for which `on` holds (every wave calls it; one barrier)
__device__ __forceinline__ int lg_block_count(bool on, LgShared* sh, int& par, int wave, int lane) {
  const int c = __popcll(__ballot(on));
  if (lane == 0) sh->cnt[par][wave] = c;
  __syncthreads();
  int tot = 0;
#pragma unroll
  for (int w = 0; w < LG_NW; ++w) tot += sh->cnt[par][w];
  par ^= 1;
  return uni(tot);
}
// position (0-based) of the k-th set bit (k >= 1) of a wave-uniform mask, computed by the lanes
__device__ __forceinline__ int lg_kth_bit(uint64_t mask, int k, int lane) {
  const int before = __popcll(mask & lanemask_lt(lane));
  const uint64_t hit = __ballot(((mask >> lane) & 1ull) && before == k - 1);
  return __ffsll((unsigned long long)hit) - 1;
}

// The next `count` values of legacy_gauss (polar Box-Muller with a one-value cache, as rng_gauss): emit(k, value) is
// called once for k = 0 .. count - 1 by the lane that owns the value.  LG_NW x 64 attempts per pass: attempt a reads
// the four words at pos + 4 a.  Called by all waves; contains barriers.
template <typename Emit>
__device__ __forceinline__ void lg_gauss(MT3& s, int count, LgShared* sh, int& par, int wave, int lane, int32_t* has,
                                         double* cache, Emit emit) {
  int produced = 0;
  const bool cached = count > 0 && uni(*has) != 0;
  __syncthreads();  // every wave has looked at the cache flag before anybody changes it
  if (cached) {
    if (wave == 0 && lane == 0) {
      emit(0, *cache);
      *has = 0;
      *cache = 0.0;
    }
    produced = 1;
  }
  while (produced < count) {
    const int pairs = (count - produced + 1) >> 1;  // accepted attempts still needed
    mt3_need(s, (s.pos + 4 * LG_NW * AIE_NT - 1) / AIE_MT_N, lane);
    const int a = wave * AIE_NT + lane, o = s.pos + 4 * a;
    uint32_t w4[4];
    mt3_words4(s, o, w4);
    const double x1 = 2.0 * u53(w4[0], w4[1]) - 1.0;
    const double x2 = 2.0 * u53(w4[2], w4[3]) - 1.0;
    const double r2 = x1 * x1 + x2 * x2;
    const bool acc = !(r2 >= 1.0 || r2 == 0.0);
    const uint64_t am = __ballot(acc);
    if (lane == 0) {
      sh->am[par][wave][0] = (uint32_t)am;
      sh->am[par][wave][1] = (uint32_t)(am >> 32);
    }
    __syncthreads();
    int before_wave = 0, total = 0, used = LG_NW * AIE_NT;  // attempts consumed by this pass
    bool found = false;
#pragma unroll
    for (int w = 0; w < LG_NW; ++w) {
      const uint64_t mw = (uint64_t)sh->am[par][w][0] | ((uint64_t)sh->am[par][w][1] << 32);
      const int cw = __popcll(mw);
      if (w == wave) before_wave = total;
      if (!found && total + cw >= pairs) {  // the attempt holding the pairs-th accepted one ends the request
        used = w * AIE_NT + lg_kth_bit(mw, pairs - total, lane) + 1;
        found = true;
      }
      total += cw;
    }
    par ^= 1;
    if (acc && a < used) {
      const double f = sqrt(-2.0 * aie_log_glibc(r2) / r2);  // libm's log bit for bit; sqrt and / are IEEE-exact
      const int k = produced + 2 * (before_wave + __popcll(am & lanemask_lt(lane)));
      emit(k, f * x2);
      if (k + 1 < count) emit(k + 1, f * x1);
      else {  // the request ends on the first value of the pair: the second one stays cached
        *cache = f * x1;
        *has = 1;
      }
    }
    produced += 2 * (found ? pairs : total);  // (may exceed count by one: the cached value)
    mt3_consume(s, 4 * used, lane);
  }
  __syncthreads();  // emitted values / cache visible to every wave
}

// Source layouts drawn at reset from the replica's own stream: Uniform.reset_starting_layout (dynamic_layout.py:313-392),
// MultiZone's per-reset zone shuffle (:778-872), Quadrant's empty water lines (:992-1024).  Called by all LG_NW waves
// of the replica's workgroup (gtid = 0 .. LG_NW * 64 - 1); `m` is every wave's copy of the generator, advanced
// identically.  c.tid is the lane.
// (cell flags of the record image <- the two source planes, with the checker / water-line cuts of the scenario)
template <typename Planes>
__device__ __forceinline__ void layout_install(const Ctx& c, int gtid, int nthreads, Planes planes) {
  const aie_params& P = c.P;
  const aie_config& g = P.c;
  const int H = P.H, W = P.W, HW = P.HW;
  uint8_t* cb = reinterpret_cast<uint8_t*>(R_CELLS(c));
  for (int cell = gtid; cell < HW; cell += nthreads) {
    const int r = cell / W, col = cell - r * W;
    const uint32_t bits = planes(cell);  // bit 0 Stone, bit 1 Wood
    bool st = (bits & 1u) != 0, wd = (bits & 2u) != 0;
    if (g.layout_checker && ((r & 1) + (col & 1)) != 1) st = wd = false;
    if (g.layout_gen == AIE_LAYOUT_QUADRANT && (col == H / 2 || r == W / 2)) st = wd = false;  // nothing on the water lines
    cb[4 * cell + 3] = (uint8_t)((cb[4 * cell + 3] & AIE_CELL_WATER) | (st ? AIE_CELL_STONE_SRC : 0) | (wd ? AIE_CELL_WOOD_SRC : 0));
  }
}
// `ghas` / `gcache`: legacy_gauss's cache of the stream the layout is drawn from (the record's for the replica's own
// stream, LgShared's for a layout stream).  `stage_out` != nullptr: the planes go to the staging area (one byte per cell:
// bit 0 Stone, bit 1 Wood) instead of into the record image's cell flags.
__device__ __forceinline__ void layout_generate(const Ctx& c, MT& m, const uint8_t* __restrict__ arena, uint8_t* extra, int gtid,
                                                int32_t* ghas, double* gcache, uint8_t* __restrict__ stage_out = nullptr) {
  const aie_params& P = c.P;
  const aie_config& g = P.c;
  const int H = P.H, W = P.W, HW = P.HW, lane = gtid & 63, wave = gtid >> 6;
  constexpr int NT = LG_NW * AIE_NT;
  const int hwp = (HW + 15) / 16 * 16;
  double* tmp = reinterpret_cast<double*>(extra);
  double* x = tmp + hwp;
  uint8_t* mbp[2] = {reinterpret_cast<uint8_t*>(x + hwp), reinterpret_cast<uint8_t*>(x + hwp) + hwp};
  int32_t* grid = reinterpret_cast<int32_t*>(mbp[1] + hwp);
  LgShared* sh = reinterpret_cast<LgShared*>(grid + 256);
  int par = 0, gpar = 0;
  const double* shared_prob = reinterpret_cast<const double*>(arena + c.R.a_layout_prob);
  const bool mz = g.layout_gen == AIE_LAYOUT_MULTI_ZONE;
  double mz_scale[2] = {0.0, 0.0};
  int size_r = 1, size_c = 1;
  if (mz) {  // np.random.shuffle of the flat zone grid, then prob / np.mean(prob) * Wood's coverage
    const int regions = g.mz_rows * g.mz_cols;
    for (int k = gtid; k < regions; k += NT) {
      int z = -1;
      if (k < g.mz_zones[0]) z = 0;
      else if (k < g.mz_zones[0] + g.mz_zones[1]) z = 1;
      else if (k < g.mz_zones[0] + g.mz_zones[1] + g.mz_zones[2]) z = 2;
      grid[k] = z;
    }
    __syncthreads();
    for (int i = regions - 1; i >= 1; --i) {  // every wave draws; the first one swaps (nobody else reads the grid yet)
      const int j = (int)rng_interval(m, lane, (uint32_t)i);
      if (gtid == 0) { const int t = grid[i]; grid[i] = grid[j]; grid[j] = t; }
      AIE_WSYNC();
    }
    __syncthreads();
    size_r = (H + g.mz_rows - 1) / g.mz_rows;
    size_c = (W + g.mz_cols - 1) / g.mz_cols;
    for (int rs = 0; rs < 2; ++rs) {
      const int own = rs == 1 ? 0 : 1;  // zone index: Wood 0, Stone 1, WoodStone 2
      int cnt = 0;
      for (int base = 0; base < HW; base += NT) {
        const int cell = base + gtid;
        bool in = false;
        if (cell < HW) {
          const int r = cell / W, col = cell - r * W;
          const int z = grid[(r / size_r) * g.mz_cols + col / size_c];
          in = z == own || z == 2;
        }
        cnt += lg_block_count(in, sh, par, wave, lane);
      }
      mz_scale[rs] = (1.0 / ((double)cnt / (double)HW)) * c.R.c.layout_coverage[1];
    }
  }
  auto source_prob = [&](int rs, int cell, double clump) -> double {
    double v;
    if (mz) {
      const int r = cell / W, col = cell - r * W;
      const int z = grid[(r / size_r) * g.mz_cols + col / size_c];
      v = (z == (rs == 1 ? 0 : 1) || z == 2) ? mz_scale[rs] : 0.0;
    } else {
      v = shared_prob[rs * HW + cell];
    }
    return v * 0.1 * clump;
  };
#ifdef AIE_DEV
  uint64_t lg_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const uint64_t lg_start = wall_clock64();
#endif
  MT3 s3;
  mt_copy(s3.w[0], m);
  s3.pos = m.pos;
  s3.have = 1;  // (pos == 624, a freshly seeded generator: every word then comes from window 1, the first twist)
  bool happy = false;
  for (int tries = 0; tries < 100 && !happy; ++tries) {
    LG_CNT(5);
    for (int q = 0; q < 2; ++q) {
      const int rs = q == 0 ? 1 : 0;  // ["Wood", "Stone"]
      const double cov = c.R.c.layout_coverage[rs], clump = c.R.c.layout_clump[rs];
      uint8_t* mb = mbp[rs];
      const uint8_t* other = q == 0 ? nullptr : mbp[1];  // empty = nothing placed on the tile yet
      // tmp = rs.rand(H, W): NT doubles per pass, thread t takes words pos + 2 t, + 1
      { LG_T0();
      for (int base = 0; base < HW; base += NT) {
        const int nb = HW - base < NT ? HW - base : NT;
        mt3_need(s3, (s3.pos + 2 * nb - 1) / AIE_MT_N, lane);
        const int o = s3.pos + 2 * (gtid < nb ? gtid : nb - 1);  // (idle threads repeat the last one's words: offsets stay monotone)
        const uint32_t a = mt3_word(s3, o), b = mt3_word(s3, o + 1);
        if (gtid < nb) tmp[base + gtid] = u53(a, b);
        mt3_consume(s3, 2 * nb, lane);
      }
      __syncthreads();
      LG_ACC(1); }
      int count = 0;
      for (int base = 0; base < HW; base += NT) {
        const int cell = base + gtid;
        bool on = false;
        if (cell < HW) {
          on = (tmp[cell] < source_prob(rs, cell, clump)) && !(other && other[cell]);
          mb[cell] = on ? 1 : 0;
        }
        count += lg_block_count(on, sh, par, wave, lane);
      }
      // while np.mean(maybe) < coverage * clump: tmp *= 0.9; maybe = (tmp < prob) * empty; stop after 201 rounds --
      // eight rounds at a time: a cell's eight outcomes become a bit mask (parked in its `maybe` byte), the rounds'
      // counts meet in sh->thr, and the first round that reaches the target is the one the loop would have stopped at
      int n_tries = 0;
      if (HW <= NT) {  // one cell per thread: the cell's value, threshold and "tile still free" stay in registers, 32 rounds a block
        const int cell = gtid < HW ? gtid : HW - 1;
        double t = tmp[cell];
        const double sp = source_prob(rs, cell, clump);
        const bool free_tile = gtid < HW && !(other && other[cell]);
        while ((double)count / (double)HW < cov * clump && n_tries <= 200) {
          LG_T0();
          LG_CNT(7);
          const int B = 201 - n_tries < 32 ? 201 - n_tries : 32;
          if (gtid < 32) sh->thr[gtid] = 0;
          __syncthreads();
          // tmp only shrinks, so a cell that passes stays on: its rounds are summed up by the FIRST round it passes
          // in (32 = not in this block); the rounds' counts are the prefix sums of that histogram
          int first_on = 32;
          {
            double tk = t;
#pragma unroll
            for (int k = 0; k < 32; ++k) {
              tk = tk * 0.9;
              first_on = (first_on == 32 && (tk < sp) && k < B) ? k : first_on;
            }
            t = tk;
          }
          if (!free_tile) first_on = 32;
          if (first_on < 32) atomicAdd(&sh->thr[first_on], 1);
          __syncthreads();
          int mine = lane < 32 ? sh->thr[lane] : 0;  // lane k: cells whose first round is k ...
#pragma unroll
          for (int d = 1; d < 32; d <<= 1) {         // ... inclusive prefix over lanes 0..31: cells on after round k
            const int up = __shfl_up(mine, d, 64);
            mine += lane >= d ? up : 0;
          }
          const uint64_t reached = __ballot(lane < B && !((double)mine / (double)HW < cov * clump));
          const int stop = reached ? __ffsll((unsigned long long)reached) - 1 : B - 1;  // the earliest round that reaches the target
          count = bcast(mine, stop);
          const uint32_t bits = first_on <= stop ? ~0u : 0u;
          n_tries += stop + 1;
          if (gtid < HW) mb[gtid] = (bits >> stop) & 1u;
          __syncthreads();
          LG_ACC(2);
        }
      } else
      while ((double)count / (double)HW < cov * clump && n_tries <= 200) {
        LG_T0();
        LG_CNT(7);
        const int B = 201 - n_tries < 8 ? 201 - n_tries : 8;
        if (gtid < 8) sh->thr[gtid] = 0;
        __syncthreads();
        for (int base = 0; base < HW; base += NT) {
          const int cell = base + gtid;
          uint32_t bits = 0;
          if (cell < HW) {
            double t = tmp[cell];
            const double sp = source_prob(rs, cell, clump);
            const bool free_tile = !(other && other[cell]);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
              t = t * 0.9;
              bits |= ((t < sp) && free_tile && k < B) ? (1u << k) : 0u;
            }
            tmp[cell] = t;  // (rounds past the stopping one included: tmp is dead once the search ends)
            mb[cell] = (uint8_t)bits;
          }
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const int ck = __popcll(__ballot((bits >> k) & 1u));
            if (lane == 0 && ck) atomicAdd(&sh->thr[k], ck);
          }
        }
        __syncthreads();
        int stop = B - 1;  // the round whose outcome stands
        for (int k = B - 1; k >= 0; --k)
          if (!((double)sh->thr[k] / (double)HW < cov * clump)) stop = k;  // the earliest round that reaches the target
        stop = uni(stop);
        count = uni(sh->thr[stop]);
        n_tries += stop + 1;
        for (int base = 0; base < HW; base += NT) {
          const int cell = base + gtid;
          if (cell < HW) mb[cell] = (mb[cell] >> stop) & 1u;
        }
        __syncthreads();
        LG_ACC(2);
      }
      while ((double)count / (double)HW < cov) {
        // kernel = rs.randn(7, 7) > 0 (row-major), then maybe + 0.2 * rs.randn(H, W) - 0.25: one request of 49 + HW values
        LG_CNT(6);
        if (gtid < 2) sh->kbits[gtid] = 0;
        { LG_T0();
        lg_gauss(s3, 49 + HW, sh, gpar, wave, lane, ghas, gcache, [&](int k, double gs) {
          if (k < 49) {
            if (gs > 0) atomicOr(&sh->kbits[k >> 5], 1u << (k & 31));
          } else {
            const int cell = k - 49;
            x[cell] = ((double)mb[cell] + (0.2 * gs)) - 0.25;
          }
        });
        LG_ACC(3); }
        LG_T0();
        const uint64_t kmask = (uint64_t)sh->kbits[0] | ((uint64_t)sh->kbits[1] << 32);
        count = 0;
        for (int base = 0; base < HW; base += NT) {
          const int cell = base + gtid;
          bool on = false;
          if (cell < HW) {
            const int r0 = cell / W, c0 = cell - r0 * W;
            // the 7x7 window first (49 LDS reads in flight at once: the additions below are a dependent chain, the
            // reads need not be), then one add per kernel one in scipy's order; window cells outside the world add nothing
            double win[49];
            uint32_t rowok = 0, colok = 0;
#pragma unroll
            for (int j = 0; j < 7; ++j) {
              rowok |= (r0 + 3 - j >= 0 && r0 + 3 - j < H) ? (1u << j) : 0u;
              colok |= (c0 + 3 - j >= 0 && c0 + 3 - j < W) ? (1u << j) : 0u;
            }
#pragma unroll
            for (int t = 0; t < 49; ++t) {
              const int j = t / 7, k = t - 7 * j;
              const bool inb = ((rowok >> j) & 1u) && ((colok >> k) & 1u);
              win[t] = inb ? x[cell + (3 - j) * W + (3 - k)] : 0.0;
            }
            double sum = 0.0;
#pragma unroll
            for (int t = 0; t < 49; ++t) {
              const int j = t / 7, k = t - 7 * j;
              if ((kmask >> t) & 1ull) {  // (wave-uniform)
                const bool inb = ((rowok >> j) & 1u) && ((colok >> k) & 1u);
                sum = inb ? sum + win[t] : sum;
              }
            }
            on = ((sum > 0) || mb[cell]) && !(other && other[cell]);
            mb[cell] = on ? 1 : 0;  // (a cell's new value depends on x and its own old value only; the count's barrier publishes it)
          }
          count += lg_block_count(on, sh, par, wave, lane);
        }
        LG_ACC(4);
      }
    }
    happy = true;
    for (int q = 0; q < 2; ++q) {
      const int rs = q == 0 ? 1 : 0;
      int count = 0;
      for (int base = 0; base < HW; base += NT) {
        const int cell = base + gtid;
        count += lg_block_count(cell < HW && mbp[rs][cell], sh, par, wave, lane);
      }
      const double ratio = ((double)count / (double)HW) / c.R.c.layout_coverage[rs];
      if (!((1 / 1.4) <= ratio && ratio <= 1.4)) happy = false;
    }
  }
  mt_copy(m, s3.w[0]);
  m.pos = s3.pos;
  if (stage_out) {
    for (int cell = gtid; cell < HW; cell += NT) stage_out[cell] = (uint8_t)((mbp[0][cell] ? 1u : 0u) | (mbp[1][cell] ? 2u : 0u));
  } else {
    layout_install(c, gtid, NT, [&](int cell) -> uint32_t { return (mbp[0][cell] ? 1u : 0u) | (mbp[1][cell] ? 2u : 0u); });
  }
  __syncthreads();
#ifdef AIE_DEV
  if (c.R.dev_trace && gtid == 0) {
    lg_acc[0] = wall_clock64() - lg_start;
    for (int k = 0; k < 8; ++k) c.R.dev_trace[12 * c.e + k] = lg_acc[k];
  }
#endif
}
}  // namespace aie

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
