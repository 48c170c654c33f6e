// aie_gtb_layoutgen.h -- the reset-time source-layout generator of the gather-trade-build family (uniform/, quadrant/,
// multi_zone/): four wavefronts per replica, the generator's three windows in registers (MT3), legacy_gauss across the
// waves (lg_*), layout_install and layout_generate.  Includes aie_device.h only: it sees none of the family's other
// headers (the record layout is aie_layout.h -- another file).  No kernel.  Part of the gather-trade-build cache key
// (aie_jit.h: kSourcesGtb).
#pragma once
#include "aie_device.h"

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
