// ---- the PPO loss of both actor classes with its gradients (include/aie.h: aie_ppo_loss) --------------------------------
// Forward and backward of the clipped surrogate, the clipped value loss and the entropy bonus in two launches.  The
// arithmetic is aie_trainer_math.h's (aie_ppo_actor_terms, aie_ppo_value_terms over the evaluator's row values: M, T, S, L, H and
// aie_policy_entry_grad), so the gradients are the CPU twin's bit for bit.
//
// Launch 1, aie_ppo_loss_kernel.  A work item is the evaluator's: for single-slot actors with rows of at most 64 entries
// (every BASELINE agent class, COVID's classes, single-action planners) a lane per entry and as many whole rows -- here
// whole ACTORS -- to a wave as fit aligned segments of 16 / 32 / 64 lanes: one read of the logits and the mask gives the
// row's M, T, S by the sampler's DPP steps, the stored action's y reaches its segment by one ds_bpermute, every lane of a
// segment then holds its actor's scalar terms and writes its own entry's gradient.  Actors of several slots (C2's planner:
// 7 rows of 22; multi-action agents' ragged rows) and rows of more than 64 entries take the generic path, a wave per actor:
// a first pass over the slots forms ln, lo and He and leaves slot s's M, T, L, H in lane s; a second pass writes the
// gradient rows (the logits come from the cache the second time).  All loads of an item that do not depend on its
// arithmetic (index, stored action, old logp, advantage, values) issue first.
// The grid is bounded (at most AIE_PPO_MAX_WAVES wavefronts: 2048 workgroups); a wavefront strides over its work items,
// keeps the float64 sums of each class in registers -- a lane adds the terms of the actor it leads, the others add 0 -- and
// at the end stores ONE record of 2 x 8 float64 into the workspace: lanes 0, 16, 32, 48 (every segment's leader is one of
// them) added in that order, by plain vector stores of lane 0.  No atomics: the order of every sum is fixed by B.
// Launch 2, aie_ppo_reduce_kernel: one workgroup adds the records (thread (q, j): records q, q + 64, ... of sum j, sixteen
// loads in flight, then q = 0 .. 63 in order) and writes both classes' statistics (aie_ppo_finish_stats).
#pragma once
#include "aie_kernels_rollout.hip"  // the evaluator's row values: sampler_segment_max, sampler_scan, policy_segment_total

#pragma clang fp contract(off)

struct PpoTerms {  // what one work item adds to its class's sums, per lane (0 in a lane that leads no actor)
  float pol, vf, ent, kl, clipf, skip, absd;
};
struct PpoSums {
  double pol, vf, ent, kl, clipf, skip, maxd;
};
__device__ __forceinline__ PpoTerms ppo_terms_of(bool lead, const aie_ppo_actor& t, float vf, float He) {
  PpoTerms r;
  r.pol = lead ? t.pol : 0.0f;
  r.vf = lead ? vf : 0.0f;
  r.ent = lead ? He : 0.0f;
  r.kl = lead ? t.kl : 0.0f;
  r.clipf = lead ? t.clipf : 0.0f;
  r.skip = (lead && !t.valid) ? 1.0f : 0.0f;
  r.absd = lead ? t.absd : 0.0f;
  return r;
}
__device__ __forceinline__ void ppo_accumulate(PpoSums& S, const PpoTerms& t) {
  S.pol += (double)t.pol;
  S.vf += (double)t.vf;
  S.ent += (double)t.ent;
  S.kl += (double)t.kl;
  S.clipf += (double)t.clipf;
  S.skip += (double)t.skip;
  const double ad = (double)t.absd;
  S.maxd = ad > S.maxd ? ad : S.maxd;
}
__device__ __forceinline__ float ppo_readlane(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
__device__ __forceinline__ double ppo_readlane(double v, int l) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), l);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double ppo_leaders_sum(double v) {  // lanes 0, 16, 32, 48 in that order
  return ((ppo_readlane(v, 0) + ppo_readlane(v, 16)) + ppo_readlane(v, 32)) + ppo_readlane(v, 48);
}
__device__ __forceinline__ double ppo_leaders_max(double v) {
  double m = ppo_readlane(v, 0);
  for (int l = 16; l < 64; l += 16) {
    const double o = ppo_readlane(v, l);
    m = o > m ? o : m;
  }
  return m;
}
__device__ __forceinline__ void ppo_record(const PpoSums& S, double* rec) {  // a class's half of the wave's record
  rec[0] = 0.0;
  rec[1] = ppo_leaders_sum(S.pol);
  rec[2] = ppo_leaders_sum(S.vf);
  rec[3] = ppo_leaders_sum(S.ent);
  rec[4] = ppo_leaders_sum(S.kl);
  rec[5] = ppo_leaders_sum(S.clipf);
  rec[6] = ppo_leaders_sum(S.skip);
  rec[7] = ppo_leaders_max(S.maxd);
}

// single-slot actors, rows of at most 64 entries: a lane per entry, 64 >> LSH actors to a wave
template <int LSH>
__device__ __forceinline__ PpoTerms ppo_fast(const aie_ppo_group& G, const int32_t* index, uint32_t b, uint32_t gi, int lane,
                                             int has_mom, float mean, float rstd) {
  constexpr int SEG = 1 << LSH, RPW = 64 >> LSH;
  const int sub = lane >> LSH, kk = lane & (SEG - 1);
  const uint32_t r0 = gi << (6 - LSH);
  const int rows = (int)((uint32_t)G.rows - r0) < RPW ? (int)((uint32_t)G.rows - r0) : RPW;
  const bool in = sub < rows && kk < G.len;
  const uint32_t ix = index ? (uint32_t)index[b] : b;  // the stored operands' row
  // scalar bases (the item's first row), 32-bit lane offsets; a lane without an entry reads the item's first one
  const float* lgb = G.lg + ((uint64_t)b * G.lg_bstride + (uint64_t)r0 * (uint32_t)G.lrs);
  const float* mkb = G.mk + ((uint64_t)ix * G.lg_bstride + (uint64_t)r0 * (uint32_t)G.lrs);
  const uint64_t srow0 = (uint64_t)ix * (uint32_t)G.rows + r0, brow0 = (uint64_t)b * (uint32_t)G.rows + r0;
  const uint32_t lgo = in ? (uint32_t)(__mul24(sub, G.lrs) + kk) : 0u;
  const uint32_t ro = sub < rows ? (uint32_t)sub : 0u;
  const float x = lgb[lgo];
  const float mv = mkb[lgo];
  const int a = G.act[srow0 + ro];
  const float lo = G.lp_old[srow0 + ro];
  const float adv = G.adv[srow0 + ro];
  float v = 0.0f, vo = 0.0f, rt = 0.0f;
  if (G.val) {
    v = G.val[brow0 + ro];
    vo = G.val_old[srow0 + ro];
    rt = G.ret[srow0 + ro];
  }
  // ---- the row's shared values (policy_eval_fast's) ----
  const bool ok = in && mv > 0.5f && x == x;
  const float M = sampler_segment_max(ok ? x : -INFINITY, SEG);
  const float y = x - M;
  const float w = ok ? aie_sampler_expf(y) : 0.0f;
  const bool live = ok && y > -80.0f;
  const float vv = live ? w * y : 0.0f;
  const float T = policy_segment_total<LSH>(sampler_scan(w, SEG));
  const float S = policy_segment_total<LSH>(sampler_scan(vv, SEG));
  const bool any = T > 0.0f;
  const float Ts = any ? T : 1.0f;
  const float L = aie_sampler_logf(Ts);
  const float H = any ? L - __fdiv_rn(S, Ts) : 0.0f;
  // the stored action's y and whether it is allowed, to every lane of its segment
  const bool a_in = a >= 0 && a < G.len;
  const int src = ((lane & ~(SEG - 1)) + (a_in ? a : 0)) << 2;
  const float ya = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, y)));
  const bool a_ok = a_in && __builtin_amdgcn_ds_bpermute(src, ok ? 1 : 0) != 0;
  const float logp = !any ? 0.0f : a_ok ? ya - L : -INFINITY;
  // ---- the actor's terms, by every lane of its segment ----
  const float Ap = aie_ppo_advantage(adv, has_mom, mean, rstd);
  const aie_ppo_actor t = aie_ppo_actor_terms(logp, lo, aie_ppo_finite(logp) && aie_ppo_finite(lo), Ap, G.clip, G.scale);
  float g = 0.0f;
  if (ok && any) g = aie_policy_entry_grad(y, w, Ts, L, H, kk == a, a_ok ? t.g_logp : 0.0f, G.g_H);
  if (in) (G.grad + ((uint64_t)b * G.lg_bstride + (uint64_t)r0 * (uint32_t)G.lrs))[lgo] = g;
  const bool lead = sub < rows && kk == 0;
  float vf = 0.0f;
  if (G.val) {
    const aie_ppo_value q = aie_ppo_value_terms(v, vo, rt, G.vf_clip, G.kv);
    vf = q.vf;
    if (lead) G.grad_v[brow0 + (uint32_t)sub] = q.grad;
  }
  return ppo_terms_of(lead, t, vf, H);
}

// one actor per wave: any number of slots (at most 64), rows of any length in chunks of 64 with the scan's carries
__device__ __forceinline__ void ppo_slot_shape(const aie_ppo_args& A, const aie_ppo_group& G, bool agents, uint32_t i, int s, int& off,
                                               int& len, uint32_t& lo) {
  if (agents && A.ragged) {  // multi-action agents: the slots of agent i follow one another in its MA logits
    len = A.params->n_sub_a ? 1 + A.params->sub_a_dim[s] : 1;
    lo = i * (uint32_t)G.lrs + (uint32_t)off;
    off += len;
  } else {
    len = G.len;
    lo = (i * (uint32_t)G.w + (uint32_t)s) * (uint32_t)G.lrs;
  }
}
__device__ __forceinline__ PpoTerms ppo_generic(const aie_ppo_args& A, const aie_ppo_group& G, bool agents, uint32_t b, uint32_t i,
                                                int lane, int has_mom, float mean, float rstd) {
  const uint32_t ix = A.index ? (uint32_t)A.index[b] : b;
  const int W = G.w;
  const uint64_t sact = (uint64_t)ix * (uint32_t)G.actors + i, bact = (uint64_t)b * (uint32_t)G.actors + i;
  const uint64_t srow = (uint64_t)ix * (uint32_t)G.rows + (uint64_t)i * (uint32_t)W;
  const float* lgb = G.lg + (uint64_t)b * G.lg_bstride;
  const float* mkb = G.mk + (uint64_t)ix * G.lg_bstride;
  const float adv = G.adv[sact];
  float v = 0.0f, vo = 0.0f, rt = 0.0f;
  if (G.val) {
    v = G.val[bact];
    vo = G.val_old[sact];
    rt = G.ret[sact];
  }
  int a_l = 0;        // lane s: slot s's stored action and old logp
  float lo_l = 0.0f;
  if (lane < W) {
    a_l = G.act[srow + (uint32_t)lane];
    lo_l = G.lp_old[srow + (uint32_t)lane];
  }
  // ---- first pass: the joint terms; slot s's row values stay in lane s ----
  float ln = 0.0f, lo = 0.0f, He = 0.0f;
  bool fin = true;
  float Mv = 0.0f, Tv = 1.0f, Lv = 0.0f, Hv = 0.0f;
  int fl = 0;  // bit 0: any, bit 1: the stored action is allowed
  int off = 0;
  for (int s = 0; s < W; ++s) {
    int len;
    uint32_t ro;
    ppo_slot_shape(A, G, agents, i, s, off, len, ro);
    const float *lg = lgb + ro, *mk = mkb + ro;
    const int a = __builtin_amdgcn_readlane(a_l, s);
    const float lold = ppo_readlane(lo_l, s);
    const int nch = (len + 63) >> 6, seg = nch > 1 ? 64 : aie_sampler_segment(len);
    const bool a_in = a >= 0 && a < len;
    const float xa = lg[a_in ? a : 0], ma = mk[a_in ? a : 0];
    const bool a_ok = a_in && ma > 0.5f && xa == xa;
    float m = -INFINITY;
    for (int ch = 0; ch < nch; ++ch) {
      const int k = 64 * ch + lane;
      if (k < len) {
        const float x = lg[k];
        if (mk[k] > 0.5f && x > m) m = x;  // (x > m: not a NaN)
      }
    }
    const float M = sampler_segment_max(m, 64);
    float T = 0.0f, S = 0.0f;
    for (int ch = 0; ch < nch; ++ch) {
      const int k = 64 * ch + lane;
      float w = 0.0f, vv = 0.0f;
      if (k < len) {
        const float x = lg[k];
        if (mk[k] > 0.5f && x == x) {
          const float y = x - M;
          w = aie_sampler_expf(y);
          vv = y > -80.0f ? w * y : 0.0f;
        }
      }
      const float c = T + sampler_scan(w, seg), cs = S + sampler_scan(vv, seg);
      T = ppo_readlane(c, seg - 1);
      S = ppo_readlane(cs, seg - 1);
    }
    const bool any = T > 0.0f;
    const float Ts = any ? T : 1.0f;
    const float L = aie_sampler_logf(Ts);
    const float H = any ? L - __fdiv_rn(S, Ts) : 0.0f;
    const float logp = !any ? 0.0f : a_ok ? (xa - M) - L : -INFINITY;
    ln = aie_ppo_joint_add(ln, logp, s);
    lo = aie_ppo_joint_add(lo, lold, s);
    He = aie_ppo_joint_add(He, H, s);
    fin = fin && aie_ppo_finite(logp) && aie_ppo_finite(lold);
    if (lane == s) {
      Mv = M;
      Tv = Ts;
      Lv = L;
      Hv = H;
      fl = (any ? 1 : 0) | (a_ok ? 2 : 0);
    }
  }
  const float Ap = aie_ppo_advantage(adv, has_mom, mean, rstd);
  const aie_ppo_actor t = aie_ppo_actor_terms(ln, lo, fin, Ap, G.clip, G.scale);
  // ---- second pass: the gradient rows ----
  off = 0;
  for (int s = 0; s < W; ++s) {
    int len;
    uint32_t ro;
    ppo_slot_shape(A, G, agents, i, s, off, len, ro);
    const float *lg = lgb + ro, *mk = mkb + ro;
    float* gr = G.grad + ((uint64_t)b * G.lg_bstride + ro);
    const int a = __builtin_amdgcn_readlane(a_l, s);
    const float M = ppo_readlane(Mv, s), Ts = ppo_readlane(Tv, s), L = ppo_readlane(Lv, s), H = ppo_readlane(Hv, s);
    const int f = __builtin_amdgcn_readlane(fl, s);
    const float gl = (f & 2) ? t.g_logp : 0.0f;
    const int nch = (len + 63) >> 6;
    for (int ch = 0; ch < nch; ++ch) {
      const int k = 64 * ch + lane;
      if (k < len) {
        const float x = lg[k];
        float g = 0.0f;
        if ((f & 1) && mk[k] > 0.5f && x == x) {
          const float y = x - M;
          g = aie_policy_entry_grad(y, aie_sampler_expf(y), Ts, L, H, k == a, gl, G.g_H);
        }
        gr[k] = g;
      }
    }
  }
  float vf = 0.0f;
  if (G.val) {
    const aie_ppo_value q = aie_ppo_value_terms(v, vo, rt, G.vf_clip, G.kv);
    vf = q.vf;
    if (lane == 0) G.grad_v[bact] = q.grad;
  }
  return ppo_terms_of(lane == 0, t, vf, He);
}

extern "C" __global__ void __launch_bounds__(256) aie_ppo_loss_kernel(const aie_ppo_args A) {
  const int lane = (int)threadIdx.x & 63;
  const uint32_t wave = (uint32_t)aie::uni((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (wave >= A.waves) return;  // (whole waves: no barrier below)
  // the advantages' moments: two floats in device memory per class, read once
  float mean[2] = {0.0f, 0.0f}, rstd[2] = {1.0f, 1.0f};
  if (A.agents.mom) {
    mean[0] = A.agents.mom[0];
    rstd[0] = A.agents.mom[1];
  }
  if (A.planner.mom) {
    mean[1] = A.planner.mom[0];
    rstd[1] = A.planner.mom[1];
  }
  PpoSums SA = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, SP = SA;
  const uint32_t total = A.B * A.items;
  const uint32_t db = A.waves / A.items, di = A.waves - db * A.items;  // one stride, in (batch element, item)
  uint32_t b = wave / A.items, it = wave - b * A.items;
  for (uint32_t wv = wave; wv < total; wv += A.waves) {
    const bool ag = it < (uint32_t)A.agents.items;
    const aie_ppo_group G = ag ? A.agents : A.planner;  // (by value: its fields are scalar selects)
    const uint32_t gi = ag ? it : it - (uint32_t)A.agents.items;
    const int hm = G.mom != nullptr;
    const float mu = ag ? mean[0] : mean[1], rs = ag ? rstd[0] : rstd[1];
    PpoTerms t;
    if (G.generic) t = ppo_generic(A, G, ag, b, gi, lane, hm, mu, rs);
    else if (G.lsh == 4) t = ppo_fast<4>(G, A.index, b, gi, lane, hm, mu, rs);
    else if (G.lsh == 5) t = ppo_fast<5>(G, A.index, b, gi, lane, hm, mu, rs);
    else t = ppo_fast<6>(G, A.index, b, gi, lane, hm, mu, rs);
    if (ag) ppo_accumulate(SA, t);
    else ppo_accumulate(SP, t);
    b += db;
    it += di;
    if (it >= A.items) {
      it -= A.items;
      ++b;
    }
  }
  // the wave's record: every segment's leader is one of lanes 0, 16, 32, 48
  double rec[AIE_PPO_RECORD];
  ppo_record(SA, rec);
  ppo_record(SP, rec + 8);
  if (lane == 0) {
    double* out = A.ws + (uint64_t)wave * AIE_PPO_RECORD;
#pragma unroll
    for (int j = 0; j < AIE_PPO_RECORD; ++j) out[j] = rec[j];
  }
}

extern "C" __global__ void __launch_bounds__(1024) aie_ppo_reduce_kernel(const aie_ppo_args A) {
  __shared__ double part[64][AIE_PPO_RECORD];
  __shared__ double tot[AIE_PPO_RECORD];
  const int t = (int)threadIdx.x, j = t & (AIE_PPO_RECORD - 1), q = t >> 4;
  const bool is_max = (j & 7) == 7;
  double acc = 0.0;
  // (sixteen loads in flight per thread: a record past the last counts as 0, which changes neither a sum nor a maximum)
  for (uint32_t r0 = (uint32_t)q; r0 < A.waves; r0 += 64u * 16u) {
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const uint32_t r = r0 + 64u * (uint32_t)k;
      v[k] = r < A.waves ? A.ws[(uint64_t)r * AIE_PPO_RECORD + j] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) acc = is_max ? (v[k] > acc ? v[k] : acc) : acc + v[k];
  }
  part[q][j] = acc;
  __syncthreads();
  if (t < AIE_PPO_RECORD) {
    double s = 0.0;
    for (int k = 0; k < 64; ++k) {
      const double v = part[k][t];
      s = is_max ? (v > s ? v : s) : s + v;
    }
    tot[t] = s;
  }
  __syncthreads();
  if (t < 2) {
    const aie_ppo_group& G = t ? A.planner : A.agents;
    if (G.stats) aie_ppo_finish_stats(&tot[8 * t], (double)A.B * (double)G.actors, G.vf_coef, G.ent_coef, G.stats);
  }
}
