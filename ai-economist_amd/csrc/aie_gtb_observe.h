// aie_gtb_observe.h -- what a gather-trade-build step or reset writes out from the state: metrics and rewards
// (current_metrics, compute_rewards), the map observations (write_ / update_spatial_observations), the flat observation
// vectors (write_ / update_flat_observations), the action masks, and the two reset-time rebuilds from the cells
// (rebuild_locmap, build_src_list).  Includes aie_gtb_state.h only: it sees neither the components
// (aie_gtb_components.h) nor the layout generator (aie_gtb_layoutgen.h).  No kernel.  Part of the gather-trade-build
// cache key (aie_jit.h: kSourcesGtb).
#pragma once
#include "aie_gtb_state.h"

namespace aie {
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
