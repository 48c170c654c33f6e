// aie_kernels_rollout.hip -- what a PPO rollout needs between the sampler and the loss: policy evaluation (forward and
// backward) under stored masks, GAE and the trajectory store.  The evaluator runs in the sampler's arithmetic and on its
// cross-lane steps (sampler_segment_max, sampler_scan), hence the include.
#pragma once
#include "aie_kernels_sampler.hip"

// ---- policy evaluation: log pi(a|s), entropy and their logit gradient under stored masks (include/aie.h:
// aie_policy_evaluate, aie_policy_evaluate_backward) ---------------------------------------------------------------------
// The learning-time half of the sampler: for B stored replica-steps (any B) the log-probability of the stored sub-action
// and the entropy of every action slot, from new logits under the stored masks, in the sampler's own arithmetic
// (aie_trainer_math.h: M, y, w, T in the scan's order, aie_sampler_logf, S, H, the backward's operation order), so that what is
// evaluated is the distribution that was drawn from -- bit for bit the CPU twin's values.  The layout is the fast
// sampler's: a lane per entry, as many whole rows to a wave as fit in aligned segments of 16 / 32 / 64 lanes (the shape is
// a wave-uniform switch to compile-time instances), the row maximum and both sums (T and S) by the sampler's DPP steps, the
// totals to the row's lanes by a swizzle or a readlane: no LDS, no barrier.  One wave = one work item (a batch element's
// agents' items, then its planner's); all of the item's loads (entry, mask, stored action, the backward's two incoming
// gradients) issue before any arithmetic.  The backward recomputes M, T and S (two scans) instead of reading stored
// probabilities and every lane writes its own entry's gradient: the stores of a wave cover its rows back to back.
// Rows of multi-action agents (ragged) and rows of more than 64 entries take the generic path: one row per wave in chunks
// of 64 with the scan's carries, the same values.  The argument is the small struct the host fills (the sampler's lesson:
// DESIGN section 3), requested in one batch.
template <int LSH>
__device__ __forceinline__ float policy_segment_total(float c) {  // the segment's last lane to all of it
  if (LSH == 6) return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, c), 63));
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, c), LSH == 5 ? 0x3E0 : 0x1F0));
}
template <int LSH, bool BWD>
__device__ __forceinline__ void policy_eval_fast(const aie_policy_eval_group& G, uint32_t b, uint32_t gi, int lane) {
  constexpr int SEG = 1 << LSH, RPW = 64 >> LSH;
  const int sub = lane >> LSH, kk = lane & (SEG - 1);
  const uint32_t r0 = gi << (6 - LSH);
  const int rows = (int)((uint32_t)G.rows - r0) < RPW ? (int)((uint32_t)G.rows - r0) : RPW;
  const bool in = sub < rows && kk < G.len;
  // scalar bases (the item's first row), 32-bit lane offsets; a lane without an entry reads the item's first one
  const float* lgb = G.lg + ((uint64_t)b * G.lg_bstride + (uint64_t)r0 * (uint32_t)G.lrs);
  const float* mkb = G.mk + ((uint64_t)b * G.mk_bstride + (uint64_t)r0 * (uint32_t)G.mrs);
  const uint64_t row0 = (uint64_t)b * (uint32_t)G.rows + r0;
  const uint32_t lgo = in ? (uint32_t)(__mul24(sub, G.lrs) + kk) : 0u;
  const uint32_t mko = in ? (uint32_t)(__mul24(sub, G.mrs) + __mul24(kk, G.mks)) : 0u;
  const uint32_t ro = sub < rows ? (uint32_t)sub : 0u;
  const float x = lgb[lgo];
  const float mv = mkb[mko];
  int a = 0;
  if (G.act) a = G.act[row0 + ro];
  float gl = 0.0f, gh = 0.0f;
  if (BWD) {
    if (G.g_logp) gl = G.g_logp[row0 + ro];
    if (G.g_ent) gh = G.g_ent[row0 + ro];
  }
  // ---- the row's shared values ----
  const bool ok = in && mv > 0.5f && x == x;
  const float M = sampler_segment_max(ok ? x : -INFINITY, SEG);
  const float y = x - M;
  const float w = ok ? aie_sampler_expf(y) : 0.0f;
  const bool live = ok && y > -80.0f;
  const float v = live ? w * y : 0.0f;
  const float T = policy_segment_total<LSH>(sampler_scan(w, SEG));
  const float S = policy_segment_total<LSH>(sampler_scan(v, SEG));
  const bool any = T > 0.0f;
  const float Ts = any ? T : 1.0f;
  const float L = aie_sampler_logf(Ts);
  const float H = any ? L - __fdiv_rn(S, Ts) : 0.0f;
  const bool a_in = a >= 0 && a < G.len;
  if (!BWD) {
    // one lane per row writes: the stored action's (lane 0 of the segment for an action outside the row)
    if (G.logp && sub < rows && kk == (a_in ? a : 0))
      G.logp[row0 + sub] = !any ? 0.0f : (a_in && ok) ? y - L : -INFINITY;
    if (G.ent && sub < rows && kk == 0) G.ent[row0 + sub] = H;
  } else {
    // is the stored action allowed?  (its lane's `ok`, to the lanes of its segment)
    const uint64_t hit = __ballot(ok && kk == a);
    const bool a_ok = LSH == 6 ? hit != 0ull : ((hit >> (lane & ~(SEG - 1))) & ((1ull << (SEG & 63)) - 1ull)) != 0ull;
    float g = 0.0f;
    if (ok && any) g = aie_policy_entry_grad(y, w, Ts, L, H, kk == a, a_ok ? gl : 0.0f, gh);
    if (in) (G.grad + ((uint64_t)b * G.lg_bstride + (uint64_t)r0 * (uint32_t)G.lrs))[lgo] = g;
  }
}
// one row per wave, any length: chunks of 64 entries with the scan's carries (and multi-action agents' rows)
template <bool BWD>
__device__ __forceinline__ void policy_eval_generic(const aie_policy_eval_args& A, const aie_policy_eval_group& G, bool agents,
                                                    uint32_t b, uint32_t row, int lane) {
  int len = G.len;
  uint32_t lo = row * (uint32_t)G.lrs, mlo = row * (uint32_t)G.mrs;
  if (agents && A.ragged) {  // lrs / mrs: from agent to agent
    const int i = (int)row / A.act_a_width, s = (int)row - i * A.act_a_width;
    int off = 0;
    for (int k = 0; k < s; ++k) off += 1 + A.params->sub_a_dim[k];
    len = A.params->n_sub_a ? 1 + A.params->sub_a_dim[s] : 1;
    lo = (uint32_t)(i * G.lrs + off);
    mlo = (uint32_t)(i * G.mrs + off * G.mks);
  }
  const float* lg = G.lg + ((uint64_t)b * G.lg_bstride + lo);
  const float* mk = G.mk + ((uint64_t)b * G.mk_bstride + mlo);
  const uint64_t ri = (uint64_t)b * (uint32_t)G.rows + row;
  const int nch = (len + 63) >> 6, seg = nch > 1 ? 64 : aie_sampler_segment(len);
  const int a = G.act ? G.act[ri] : 0;
  const bool a_in = a >= 0 && a < len;
  const float xa = lg[a_in ? a : 0], ma = mk[(a_in ? a : 0) * G.mks];
  const bool a_ok = a_in && ma > 0.5f && xa == xa;
  float m = -INFINITY;
  for (int ch = 0; ch < nch; ++ch) {
    const int k = 64 * ch + lane;
    if (k < len) {
      const float x = lg[k];
      if (mk[k * G.mks] > 0.5f && x > m) m = x;  // (x > m: not a NaN)
    }
  }
  const float M = sampler_segment_max(m, 64);
  float T = 0.0f, S = 0.0f;
  for (int ch = 0; ch < nch; ++ch) {
    const int k = 64 * ch + lane;
    float w = 0.0f, v = 0.0f;
    if (k < len) {
      const float x = lg[k];
      if (mk[k * G.mks] > 0.5f && x == x) {
        const float y = x - M;
        w = aie_sampler_expf(y);
        v = y > -80.0f ? w * y : 0.0f;
      }
    }
    const float c = T + sampler_scan(w, seg), cs = S + sampler_scan(v, seg);
    T = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, c), seg - 1));
    S = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, cs), seg - 1));
  }
  const bool any = T > 0.0f;
  const float Ts = any ? T : 1.0f;
  const float L = aie_sampler_logf(Ts);
  const float H = any ? L - __fdiv_rn(S, Ts) : 0.0f;
  if (!BWD) {
    if (lane == 0) {
      if (G.logp) G.logp[ri] = !any ? 0.0f : a_ok ? (xa - M) - L : -INFINITY;
      if (G.ent) G.ent[ri] = H;
    }
  } else {
    const float gl = (G.g_logp && a_ok) ? G.g_logp[ri] : 0.0f, gh = G.g_ent ? G.g_ent[ri] : 0.0f;
    float* gr = G.grad + ((uint64_t)b * G.lg_bstride + lo);
    for (int ch = 0; ch < nch; ++ch) {
      const int k = 64 * ch + lane;
      if (k < len) {
        const float x = lg[k];
        float g = 0.0f;
        if (any && mk[k * G.mks] > 0.5f && x == x) {
          const float y = x - M;
          g = aie_policy_entry_grad(y, aie_sampler_expf(y), Ts, L, H, k == a, gl, gh);
        }
        gr[k] = g;
      }
    }
  }
}
template <bool BWD>
__device__ __forceinline__ void policy_eval_body(const aie_policy_eval_args& A) {
  const int lane = (int)threadIdx.x & 63;
  const uint32_t wv = (uint32_t)aie::uni((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  // every kernel argument is requested here, in one batch (the fast sampler's finding)
  asm volatile("" ::"s"(A.agents.lg), "s"(A.agents.mk), "s"(A.agents.act), "s"(A.agents.logp), "s"(A.agents.ent), "s"(A.agents.grad),
               "s"(A.agents.g_logp), "s"(A.agents.g_ent), "s"(A.agents.lg_bstride), "s"(A.agents.mk_bstride), "s"(A.agents.len),
               "s"(A.agents.lrs), "s"(A.agents.mrs), "s"(A.agents.mks), "s"(A.agents.lsh), "s"(A.agents.rows), "s"(A.agents.items),
               "s"(A.agents.generic));
  asm volatile("" ::"s"(A.planner.lg), "s"(A.planner.mk), "s"(A.planner.act), "s"(A.planner.logp), "s"(A.planner.ent),
               "s"(A.planner.grad), "s"(A.planner.g_logp), "s"(A.planner.g_ent), "s"(A.planner.lg_bstride), "s"(A.planner.mk_bstride),
               "s"(A.planner.len), "s"(A.planner.lrs), "s"(A.planner.mrs), "s"(A.planner.mks), "s"(A.planner.lsh), "s"(A.planner.rows),
               "s"(A.planner.items), "s"(A.planner.generic), "s"(A.B), "s"(A.items));
  const uint32_t b = wv / A.items, it = wv - b * A.items;
  if (b >= A.B) return;  // (whole waves: no barrier below)
  const bool ag = it < (uint32_t)A.agents.items;
  const aie_policy_eval_group G = ag ? A.agents : A.planner;  // (by value: its fields are scalar selects)
  const uint32_t gi = ag ? it : it - (uint32_t)A.agents.items;
  if (G.generic) policy_eval_generic<BWD>(A, G, ag, b, gi, lane);
  else if (G.lsh == 4) policy_eval_fast<4, BWD>(G, b, gi, lane);
  else if (G.lsh == 5) policy_eval_fast<5, BWD>(G, b, gi, lane);
  else policy_eval_fast<6, BWD>(G, b, gi, lane);
}
extern "C" __global__ void __launch_bounds__(256) aie_policy_eval_kernel(const aie_policy_eval_args A) { policy_eval_body<false>(A); }
extern "C" __global__ void __launch_bounds__(256) aie_policy_eval_bwd_kernel(const aie_policy_eval_args A) { policy_eval_body<true>(A); }

// ---- generalised advantage estimation from the reward log (include/aie.h: aie_gae) ---------------------------------------
// The recurrence (aie_trainer_math.h: aie_gae_step) is serial in t down a column (replica, actor) and is NOT re-associated across
// time: these are the bits of the plain float32 loop.  What is parallel is the loads.  A lane per float of a log row
// (lane c = e (n + 2) + j), so a wave's reward loads are 256 contiguous bytes of the row whatever n is; the done flag is a
// second load of the same lines (the lane's replica's last column); the values come from one load per step through a
// per-lane pointer (agents' and planner's tensors), consecutive lanes on consecutive floats within a class.  The lanes on
// the done column (one in n + 2) and those of a class the caller left out retire at once.  Time runs backwards in chunks of
// AIE_GAE_U steps, two register buffers: the 3 x AIE_GAE_U loads of the NEXT chunk are issued before the two dependent
// operations per step of the current one, so with one or two waves per CU (C2: 4096 x 6 lanes = 384 waves) there are
// ~6 KB per wave in flight -- memory-level parallelism from loads, not from waves.  Workgroups of one wave spread the few
// waves over every CU.
#define AIE_GAE_U 8
struct GaeLane {
  const float *r, *d, *v;  // the lane's reward / done column in slot 0 of the log; its value in row 0
  float *adv, *ret;
  uint32_t row, vstride;   // floats per log row; per value row
};
__device__ __forceinline__ void gae_load(const GaeLane& L, int t0, int slot0, int slots, float (&r)[AIE_GAE_U], float (&d)[AIE_GAE_U],
                                         float (&v)[AIE_GAE_U]) {
#pragma unroll
  for (int k = 0; k < AIE_GAE_U; ++k) {
    const int t = t0 - k;
    r[k] = d[k] = v[k] = 0.0f;
    if (t >= 0) {  // (wave-uniform; k <= t < slots: one wrap)
      const int s = slot0 - k < 0 ? slot0 - k + slots : slot0 - k;
      r[k] = L.r[(size_t)s * L.row];
      d[k] = L.d[(size_t)s * L.row];
      v[k] = L.v[(size_t)t * L.vstride];
    }
  }
}
__device__ __forceinline__ void gae_chunk(const GaeLane& L, int t0, const float (&r)[AIE_GAE_U], const float (&d)[AIE_GAE_U],
                                          const float (&v)[AIE_GAE_U], float gamma, float gl, float& v_next, float& a_next) {
#pragma unroll
  for (int k = 0; k < AIE_GAE_U; ++k) {
    const int t = t0 - k;
    if (t >= 0) {
      const float a = aie_gae_step(r[k], v[k], v_next, a_next, d[k] > 0.5f, gamma, gl);
      if (L.adv) L.adv[(size_t)t * L.vstride] = a;
      if (L.ret) L.ret[(size_t)t * L.vstride] = aie_gae_return(a, v[k]);
      a_next = a;
      v_next = v[k];
    }
  }
}
extern "C" __global__ void __launch_bounds__(64) aie_gae_kernel(const aie_gae_args A) {
  asm volatile("" ::"s"(A.log), "s"(A.va), "s"(A.vp), "s"(A.adv_a), "s"(A.adv_p), "s"(A.ret_a), "s"(A.ret_p), "s"(A.T), "s"(A.slots),
               "s"(A.first), "s"(A.E), "s"(A.n), "s"(A.gamma), "s"(A.gl));
  const uint32_t W = (uint32_t)A.n + 2u, row = (uint32_t)A.E * W;
  const uint32_t c = blockIdx.x * 64u + threadIdx.x;
  if (c >= row) return;
  const uint32_t e = c / W, j = c - e * W;
  const bool agent = j < (uint32_t)A.n;
  const float* vals = agent ? A.va : A.vp;
  if (j > (uint32_t)A.n || !vals) return;  // the done column; a class that is left out (no barrier below)
  GaeLane L;
  L.row = row;
  L.vstride = agent ? (uint32_t)A.E * (uint32_t)A.n : (uint32_t)A.E;
  const uint32_t vo = agent ? e * (uint32_t)A.n + j : e;
  L.r = A.log + c;
  L.d = A.log + (e * W + (uint32_t)A.n + 1u);
  L.v = vals + vo;
  L.adv = agent ? A.adv_a : A.adv_p;
  L.ret = agent ? A.ret_a : A.ret_p;
  if (L.adv) L.adv += vo;
  if (L.ret) L.ret += vo;
  const int T = A.T, slots = A.slots;
  float v_next = L.v[(size_t)T * L.vstride], a_next = 0.0f;  // row T: the bootstrap value; A_T = 0
  int t0 = T - 1;
  int slot0 = (int)((uint32_t)A.first + (uint32_t)t0);  // first, t0 < slots: one wrap
  if (slot0 < 0 || slot0 >= slots) slot0 = (int)((uint32_t)slot0 - (uint32_t)slots);
  float r0[AIE_GAE_U], d0[AIE_GAE_U], v0[AIE_GAE_U], r1[AIE_GAE_U], d1[AIE_GAE_U], v1[AIE_GAE_U];
  gae_load(L, t0, slot0, slots, r0, d0, v0);
  while (t0 >= 0) {
    int sn = slot0 - AIE_GAE_U;
    if (sn < 0) sn += slots;  // (used only while t0 - U >= 0, i.e. U < slots: one wrap)
    gae_load(L, t0 - AIE_GAE_U, sn, slots, r1, d1, v1);
    gae_chunk(L, t0, r0, d0, v0, A.gamma, A.gl, v_next, a_next);
    t0 -= AIE_GAE_U;
    slot0 = sn - AIE_GAE_U;
    if (slot0 < 0) slot0 += slots;
    if (t0 < 0) break;
    gae_load(L, t0 - AIE_GAE_U, slot0, slots, r0, d0, v0);
    gae_chunk(L, t0, r1, d1, v1, A.gamma, A.gl, v_next, a_next);
    t0 -= AIE_GAE_U;
  }
}

// ---- trajectory store: this step's blocks into the replica's ring slot (include/aie.h: aie_trajectory_store) -------------
// A workgroup per replica.  Every thread reads the replica's slot counter, the barrier, then thread 0 -- the only writer of
// that counter in the launch -- advances it: nothing that changes from step to step is a kernel argument, so a captured launch
// walks the ring on replay (the reward log's slot and the sampler's draw index work the same way).  A counter outside the
// ring counts as 0 (nothing is written out of bounds whatever the caller left there).  The segments are dealt to the
// workgroup's four waves, which copy side by side: 16 bytes per lane where the host found source, destination, stride and
// size aligned for every replica and slot (a wave-uniform flag per segment), else 4 bytes per lane; a segment with rows > 1
// is a [rows][cols] block stored as [cols][rows] (4-byte elements; stores coalesced, the strided loads come out of a block of
// a few hundred bytes).
extern "C" __global__ void __launch_bounds__(256) aie_trajectory_store_kernel(const aie_traj_args A) {
  const uint32_t e = blockIdx.x;
  int32_t s = A.slot[e];
  __syncthreads();
  if (threadIdx.x == 0) A.slot[e] = (uint32_t)s + 1u < (uint32_t)A.n_slots ? s + 1 : 0;
  if ((uint32_t)s >= (uint32_t)A.n_slots) s = 0;
  const int lane = (int)threadIdx.x & 63;
  for (int g = aie::uni((int)(threadIdx.x >> 6)); g < A.n_segs; g += 4) {
    const uint8_t* src = A.seg[g].src + (int64_t)e * A.seg[g].src_stride;
    const int32_t bytes = A.seg[g].bytes, rows = A.seg[g].rows;
    uint8_t* dst = A.seg[g].dst + ((int64_t)s * A.E + e) * bytes;
    if (rows > 1) {
      const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src);
      uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
      const uint32_t count = (uint32_t)bytes >> 2, cols = count / (uint32_t)rows;
      for (uint32_t i = (uint32_t)lane; i < count; i += 64u) {
        const uint32_t cc = i / (uint32_t)rows, rr = i - cc * (uint32_t)rows;
        d32[i] = s32[rr * cols + cc];
      }
    } else if (A.seg[g].wide) {
      const uint4* s128 = reinterpret_cast<const uint4*>(src);
      uint4* d128 = reinterpret_cast<uint4*>(dst);
      for (uint32_t i = (uint32_t)lane; i < ((uint32_t)bytes >> 4); i += 64u) d128[i] = s128[i];
    } else {
      const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src);
      uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
      for (uint32_t i = (uint32_t)lane; i < ((uint32_t)bytes >> 2); i += 64u) d32[i] = s32[i];
    }
  }
}
