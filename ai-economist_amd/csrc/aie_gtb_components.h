// aie_gtb_components.h -- the gather-trade-build dynamics, one component_step per Foundation component (Build, Gather,
// ContinuousDoubleAuction with its order book, PeriodicBracketTax, WealthRedistribution) and the scenario's resource
// regeneration with its source list (SrcList, scenario_step_regen*).  Includes aie_gtb_state.h only: it sees neither
// the observation writers (aie_gtb_observe.h) nor the layout generator (aie_gtb_layoutgen.h).  No kernel.  Part of the
// gather-trade-build cache key (aie_jit.h: kSourcesGtb).
#pragma once
#include "aie_gtb_state.h"

namespace aie {
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
// Returns whether the generator's LDS window (Ctx.mtwin) holds the rows as this call leaves them, words 0 .. 623 in
// order: store_generator_rows then sends them out from there.  Only the sparse MT19937 path with the window does.
__device__ __forceinline__ bool scenario_step_regen(const Ctx& c, MT& m, const SrcList& src) {
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
    return false;
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
    return false;
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
  // (the loop above runs at least once, and its last round stored the rows behind the last twist: nothing twists after it)
  return c.mtwin != nullptr;
}

}  // namespace aie
