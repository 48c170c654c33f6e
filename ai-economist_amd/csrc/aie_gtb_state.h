// aie_gtb_state.h -- the gather-trade-build family's per-replica state helpers: the world helpers (can_agent_occupy,
// log_event, agent_can_build), the agents' registers (Agents, agents_load / agents_store, hist_bit, decode_actions), the
// change log of one step (dirty_*) and the record's way in and out of a step with the cells' byte plane
// (load_record_step_request / _commit, store_record_step).  The foot of the family's headers: it includes aie_device.h only, and
// aie_gtb_components.h and aie_gtb_observe.h both include it.  No kernel.  Part of the gather-trade-build cache key
// (aie_jit.h: kSourcesGtb).
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
// The loads of a lane that has one word to decode -- a single-action agent, a planner bracket -- can be asked for ahead
// of the decode (action_words_request) and handed to it; a multi-action agent's words and everything of the `host`
// branches are loaded where they are decoded.
struct ActionWords { int32_t a, p; bool pre; };
__device__ __forceinline__ ActionWords action_words_request(const Ctx& c, const int32_t* __restrict__ aa,
                                                            const int32_t* __restrict__ ap, uint8_t* __restrict__ arena = nullptr) {
  const aie_params& P = c.P;
  ActionWords w = {0, 0, !(c.full && arena)};
  if (!w.pre) return w;
  const int i = c.tid;
  if (i < P.n && aa && !P.c.multi_action_mode_agents) w.a = aa[((int64_t)c.e * P.n + i) * P.act_a_width];
  if (i < AIE_MAX_BRACKETS && ap && i < P.n_sub_p) w.p = ap[(int64_t)c.e * P.act_p_width + (P.c.multi_action_mode_planner ? i : 0)];
  return w;
}
__device__ __forceinline__ int decode_actions(const Ctx& c, Agents& A, const int32_t* __restrict__ aa,
                               const int32_t* __restrict__ ap, uint8_t* __restrict__ arena = nullptr,
                               const ActionWords* pre = nullptr) {
  const aie_params& P = c.P;
  const bool host = c.full && arena;  // (compile-time false in the common step kernel, see Ctx::full)
  if (pre && !pre->pre) pre = nullptr;
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
        const int v = pre ? pre->a : a[0];
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
        v = pre ? pre->p : a[row0 + i];
        bad_p = v < 0 || v > P.sub_p_dim;  // (the tax component ignores what its mask forbids; out of range is an error)
        if (bad_p) v = 0;
      } else {
        const int x = pre ? pre->p : a[0];
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
// ------------------------------------------------------------------------------------
// The record's way in and out of a step, and the cells' byte plane (aie_layout.h: o_cells8, aie_cell_pack8).
// ------------------------------------------------------------------------------------
// Four cells of the plane -> their four words.  Byte-parallel arithmetic on the dword (the four Stone bytes, Wood bytes,
// owner bytes, flag bytes), then a 4 x 4 byte transpose with v_perm_b32 (selector bytes 0-3: second operand, 4-7: first).
__device__ __forceinline__ uint4 cells8_expand(uint32_t d) {
  const uint32_t st = (d >> 3) & 0x01010101u, wd = (d >> 4) & 0x01010101u, fl = d & 0x07070707u;
  // per byte 0 -> 0xff (no house), k + 1 -> k: the borrow stops at bit 7 of each byte
  const uint32_t ow = ((((d >> 5) & 0x07070707u) | 0x80808080u) - 0x01010101u) ^ 0x80808080u;
  const uint32_t sw01 = __builtin_amdgcn_perm(wd, st, 0x05010400u), sw23 = __builtin_amdgcn_perm(wd, st, 0x07030602u);
  const uint32_t of01 = __builtin_amdgcn_perm(fl, ow, 0x05010400u), of23 = __builtin_amdgcn_perm(fl, ow, 0x07030602u);
  uint4 w;
  w.x = __builtin_amdgcn_perm(of01, sw01, 0x05040100u);
  w.y = __builtin_amdgcn_perm(of01, sw01, 0x07060302u);
  w.z = __builtin_amdgcn_perm(of23, sw23, 0x05040100u);
  w.w = __builtin_amdgcn_perm(of23, sw23, 0x07060302u);
  return w;
}
// The step's way in.  The cells are 2.5 of the 4.3 KB image of BASELINE configs[1], and the burst of record loads that
// every workgroup of a launch starts with is priced by its bytes: where the record has the byte plane, the 16-byte units
// that hold nothing but cells are not fetched -- plane dword k expands into unit k -- and only the rest of the image
// comes as it is (the unit the cells share with the next field brings the last H W % 4 words).  The plane holds while
// obs_valid != 0, which is known once the image is in LDS: load_record_cells is the other case.
// (A/B on one MI355X, BASELINE configs[1] at 4096 replicas, profiles/cell_plane_ab.txt: with one wait per load, as the
// word-per-cell copy has them, the plane gains nothing -- 19.97 us per launch, the parent's 19.96 -- however the two waves
// share it; with the loads below requested together 19.62 us.)
// In two halves, so that a wave has its other loads in flight beside these and waits once for all of them (step_body;
// profiles/prologue_loads_ab.txt): load_record_step_request says which units and plane dwords the lane owns -- the one
// statement of it -- and asks for a lane's first three loads of either kind; load_record_step_commit writes them to the
// image and copies what a larger image has beyond them, one by one.  A record without the plane (more than 7 agents,
// max_health > 1) is 16-byte units throughout, every nwaves-th group of 64 a wave's: there the three are a lane's first
// three units (BASELINE configs[2], ten agents, at 4096 replicas: 35.66 -> 35.16 us per launch against load, wait, LDS
// write per unit -- round 6 had found the opposite with the whole share of a 4.3 KB image requested at once, step_body).
struct RecordIn {
  int q, k0;            // the lane's first unit of the image; with the plane: its first plane dword (k0 == q0: none)
  bool hu, h0, h1, h2;  // which of unit q and plane dwords k0, k0 + 64, k0 + 128 exist; without the plane: units q, q + st, q + 2 st
  uint4 u, u1, u2;      // (u1, u2: without the plane only)
  uint32_t d0, d1, d2;
};
__device__ __forceinline__ RecordIn load_record_step_request(const Ctx& c, const uint8_t* __restrict__ arena, int wave,
                                                             int nwaves) {
  RecordIn in;
  in.u = in.u1 = in.u2 = uint4{0u, 0u, 0u, 0u};
  in.d0 = in.d1 = in.d2 = 0u;
  const uint8_t* g = arena + (int64_t)c.e * c.P.rec_bytes;  // (a_records == 0, see load_record)
  const uint4* src = reinterpret_cast<const uint4*>(g);
  const int nq = rec_lds_bytes(c.P) >> 4, st = nwaves * AIE_NT;
  if (!c.P.o_cells8) {
    in.q = wave * AIE_NT + c.tid;
    in.k0 = 0;
    in.hu = false;
    in.h0 = in.q < nq;
    in.h1 = in.q + st < nq;
    in.h2 = in.q + 2 * st < nq;
    if (in.h0) in.u = src[in.q];
    if (in.h1) in.u1 = src[in.q + st];
    if (in.h2) in.u2 = src[in.q + 2 * st];
    return in;
  }
  const uint32_t* plane = reinterpret_cast<const uint32_t*>(g + c.P.o_cells8);
  const int q0 = (4 * c.P.HW) >> 4;  // units [0, q0): cells only (o_cells == 0)
  // The first wave takes the whole plane: the second has the draw window and the constant tables to fetch beside its
  // units.  A lane's first unit and its first three plane dwords are all there is up to 27 x 27.
  in.q = q0 + wave * AIE_NT + c.tid;
  in.k0 = wave == 0 ? c.tid : q0;
  in.hu = in.q < nq;
  in.h0 = in.k0 < q0;
  in.h1 = in.k0 + AIE_NT < q0;
  in.h2 = in.k0 + 2 * AIE_NT < q0;
  if (in.hu) in.u = src[in.q];
  if (in.h0) in.d0 = plane[in.k0];
  if (in.h1) in.d1 = plane[in.k0 + AIE_NT];
  if (in.h2) in.d2 = plane[in.k0 + 2 * AIE_NT];
  return in;
}
__device__ __forceinline__ void load_record_step_commit(const Ctx& c, const uint8_t* __restrict__ arena, int nwaves,
                                                        const RecordIn& in) {
  const uint8_t* g = arena + (int64_t)c.e * c.P.rec_bytes;
  const uint4* src = reinterpret_cast<const uint4*>(g);
  uint4* dst = reinterpret_cast<uint4*>(c.rec);
  const int nq = rec_lds_bytes(c.P) >> 4, st = nwaves * AIE_NT;
  if (!c.P.o_cells8) {
    if (in.h0) dst[in.q] = in.u;
    if (in.h1) dst[in.q + st] = in.u1;
    if (in.h2) dst[in.q + 2 * st] = in.u2;
    for (int qq = in.q + 3 * st; qq < nq; qq += st) dst[qq] = src[qq];
    return;
  }
  const uint32_t* plane = reinterpret_cast<const uint32_t*>(g + c.P.o_cells8);
  const int q0 = (4 * c.P.HW) >> 4;
  if (in.hu) dst[in.q] = in.u;
  if (in.h0) dst[in.k0] = cells8_expand(in.d0);
  if (in.h1) dst[in.k0 + AIE_NT] = cells8_expand(in.d1);
  if (in.h2) dst[in.k0 + 2 * AIE_NT] = cells8_expand(in.d2);
  for (int qq = in.q + st; qq < nq; qq += st) dst[qq] = src[qq];
  for (int k = in.k0 + 3 * AIE_NT; k < q0; k += AIE_NT) dst[k] = cells8_expand(plane[k]);
}
// ... and the cell units themselves, over what the plane gave: the launch found obs_valid == 0, so something outside the
// kernels may have edited the words and the plane is not to be trusted.  Such a launch writes the whole plane on its
// way out (step_body starts its change log past AIE_DIRTY_CAP).
__device__ __forceinline__ void load_record_cells(const Ctx& c, const uint8_t* __restrict__ arena, int wave, int nwaves) {
  const uint4* src = reinterpret_cast<const uint4*>(arena + (int64_t)c.e * c.P.rec_bytes);
  uint4* dst = reinterpret_cast<uint4*>(c.rec);
  const int q0 = (4 * c.P.HW) >> 4;
  for (int q = wave * AIE_NT + c.tid; q < q0; q += nwaves * AIE_NT) dst[q] = src[q];
}
// the whole plane (padding: zero) from the LDS image's words
__device__ __forceinline__ void store_cells8(const Ctx& c, uint8_t* __restrict__ arena, int wave = 0, int nwaves = 1) {
  uint32_t* plane = reinterpret_cast<uint32_t*>(arena + (int64_t)c.e * c.P.rec_bytes + c.P.o_cells8);
  const int nd = ((c.P.HW + 15) >> 4) << 2;
  for (int k = wave * AIE_NT + c.tid; k < nd; k += nwaves * AIE_NT) {
    uint32_t d = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * k + j < c.P.HW) d |= aie_cell_pack8(R_CELLS(c)[4 * k + j]) << (8 * j);
    plane[k] = d;
  }
}
// The step's way out (round 6).  A step changes a handful of the H W map cells -- the ones its change log lists for the
// in-place map observations (dirty_*: every cell whose word or occupant changed) -- so the 16-byte units that hold
// nothing but cells stay as they are in HBM and the listed cells go out one word per lane, each with its byte of the
// plane: 2.4 of the 4.2 KB image of BASELINE configs[1] are not written.  A log overflow writes everything, the plane
// included.  (The generator's rows left right behind the regeneration: store_generator_rows.)
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
    const uint32_t w = R_CELLS(c)[cell];
    reinterpret_cast<uint32_t*>(g + c.P.o_cells)[cell] = w;
    if (c.P.o_cells8) (g + c.P.o_cells8)[cell] = (uint8_t)aie_cell_pack8(w);
  }
  if (c.P.o_cells8 && q0 == 0) store_cells8(c, arena, wave, nwaves);
}

}  // namespace aie
