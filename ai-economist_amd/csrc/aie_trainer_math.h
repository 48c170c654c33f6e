/*
 * aie_trainer_math.h -- the trainer side's arithmetic, stated once: the policy sampler and evaluator, the PPO loss,
 * generalised advantage estimation, the policy MLP's forward and backward rows, the convolutional encoder and the optimizer step (Adam under a
 * gradient-norm clip), with the kernels' argument records
 * (aie_sampler_args, aie_sampler_check, aie_sampler_args_of).  The long comment below defines the sampler's and the
 * evaluator's operations; the comments above aie_ppo_*, aie_gae_step, aie_mlp_* and aie_opt_* define the others.
 *
 * Plain C99 with AIE_HD (also included from HIP C++): the device kernels, the host plans (aie_trainer_plan.h), the CPU
 * restatement (oracle/aie_oracle.c) and the CPU tests compile the same helpers.  Included by aie_kernels_sampler.hip
 * and aie_kernels_mlp.hip (the roots of the two trainer chains), aie_kernels_optim.hip, aie_kernels_conv.hip, aie_trainer_plan.h and the oracle -- not by
 * aie_device.h, so no step or reset kernel is compiled from it and it is in no specialisation cache key (aie_jit.h).
 */
#ifndef AIE_TRAINER_MATH_H_
#define AIE_TRAINER_MATH_H_

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "aie_layout.h"

/* Floating-point contraction under HIP: this header states its own mode, so that its code does not depend on where it
 * is included from, and ends in the library's (aie_device.h switches contraction off for every kernel).  Its own is
 * HIP's default: a helper whose products must be rounded before they are added says so itself (AIE_NOCONTRACT below);
 * in the others a fused multiply-add changes no result (aie_sampler_uniform: product and sum are both exact).  The
 * host's C compilers take their mode from the command line (-ffp-contract=off).  The `off` at the end is assumed, not
 * restored (this target has no push / pop of the mode): every HIP file of the library reaches aie_device.h first,
 * and one that did not would be left in the library's mode from here on, not in the compiler's default. */
#if defined(__HIPCC__)
#pragma clang fp contract(fast)
#endif

/* ---- the policy sampler (aie_sample_policy_actions; round 6: inverse CDF in float32) ---------------------------------
 * A row (one action slot: `len` entries k = 0 .. len - 1 with logits x_k, of which some are allowed: mask > 0.5 and x_k
 * not a NaN) is sampled as
 *     M = max of the allowed x_k;  w_k = aie_sampler_expf(x_k - M) for allowed k, 0 otherwise (and for k >= len);
 *     c_k = inclusive prefix sums of w in the FIXED order below;  T = the total in that order;
 *     u = aie_sampler_uniform(aie_sampler_entry_rng(base, slot)) in (0, 1), 23 bits;
 *     choice = the first allowed k with c_k > u T  (the last allowed k if rounding leaves none; NO-OP if nothing is allowed),
 * base = one 64-bit counter hash per replica and call (aie_counter_rng), slot = the row's index in the replica.  Every
 * operation is an IEEE float32 add / multiply / fused multiply-add (fmaf: exact, rounded once) in a fixed order -- no
 * libm exponential, no table -- so the kernel, the CPU restatement (oracle/) and a Python transcription pick the same entry:
 *   * prefix sums: rows are cut into chunks of 64 entries; inside a chunk, over the entry's index r in its chunk and the
 *     row's segment size seg = aie_sampler_segment(len) (16, 32 or 64: what the kernel's cross-lane primitives span; 64
 *     for every chunk of a row of more than 64 entries):
 *     steps d = 1, 2, 4, 8: v_r <- v_r + v_{r-d} for (r mod 16) >= d (all r at once, inputs = the previous step's values);
 *     seg >= 32: v_r <- v_r + v_{16 (r div 16) - 1} for r div 16 odd;  seg = 64: v_r <- v_r + v_31 for r >= 32;
 *     c_k = carry + v_r;  the chunk's total = carry + v_{seg-1};  carry = 0 for the first chunk, then the previous total;
 *   * aie_sampler_expf(y), y <= 0: 0 at or below -80; n = rint(y log2(e)); r = fma(n, -ln2_lo, fma(n, -ln2_hi, y)); the
 *     Taylor polynomial of e^r through r^6 by Horner in fma (|r| <= 0.35: the first dropped term is 1.3e-7 of the sum);
 *     times 2^n (ldexp: exact, n >= -116).
 * Per entry: one exponential of 14 vector instructions, a row maximum and a prefix sum of 6 - 10 data-parallel-primitive
 * instructions each (DPP row rotates / shifts / broadcasts and gfx950's permlane swaps: no LDS), one comparison -- where
 * round 5's Gumbel-max spent two float64 logarithms (each with an IEEE division) and a 64-bit key per entry.  float32
 * resolves a probability to 2^-24 of the row's total; u itself has 23 bits.
 *
 * The same row, evaluated (aie_sample_policy_actions_logp, aie_policy_evaluate and its backward; the row helpers below are
 * the CPU twin): with the allowed set, M, w_k and T of above, y_k = x_k - M and "live" = allowed with y_k > -80 (w_k > 0),
 *     L = aie_sampler_logf(T);   logp_k = y_k - L;   p_k = w_k / T (IEEE division, rounded to nearest);
 *     S = sum of v_k, v_k = w_k * y_k (the product rounded) for live k and 0 otherwise, in the scan's order (the same
 *         steps and carries as T: the total is the scan's last value);   H = L - S / T.
 *   * aie_sampler_logf(T), T >= 2^-116 (the smallest non-zero total; a total that counts an allowed maximum is >= 1):
 *     T = m 2^e exactly with m in (sqrt(1/2), sqrt(2)] (mantissa field > 0x3504f3: m = mantissa / 2, e + 1);
 *     f = m - 1 (exact); h = the polynomial of degree 9 below by Horner in fma, highest coefficient first
 *     (log(1 + f) = f + f^2 h(f) to 1.5e-9 on the interval); t = f * f; lp = fma(t, h, f);
 *     L = fma(e, ln2_hi, fma(e, ln2_lo, lp)) with aie_sampler_expf's two-part ln 2 (e ln2_hi is exact).  T = 1 gives 0.
 *   * backward, the gradient of (g_logp logp_a + g_H H) with respect to x_k, a = the stored action:
 *     allowed k:  t1 = [k = a] - p_k;  a1 = g_logp * t1;  lh = logp_k + H;  t2 = p_k * lh for live k, 0 otherwise;
 *                 t3 = g_H * t2;  g_k = a1 - t3   (every operation rounded, nothing fused);
 *     k not allowed: exactly 0.
 *   * edges: a row where nothing is allowed, or whose total is 0 (every allowed logit -inf), has logp 0 whatever the
 *     stored action, H 0 and a zero gradient row (the sampler's choice there is NO-OP or the last allowed entry); a stored
 *     action the mask does not allow (or outside 0 .. len - 1) has logp -INFINITY and its g_logp counts as 0; an allowed
 *     entry with y <= -80 has w = 0 and the finite logp y - L (-INFINITY for a logit of -inf). */
AIE_HD static inline uint32_t aie_sampler_entry_rng(uint32_t base, uint32_t k) {  /* "lowbias32", C. Wellons' hash prospector */
  uint32_t h = base + k * 0x9E3779B1u;
  h ^= h >> 16;
  h *= 0x7feb352du;
  h ^= h >> 15;
  h *= 0x846ca68bu;
  h ^= h >> 16;
  return h;
}
AIE_HD static inline float aie_sampler_uniform(uint32_t rnd) {  /* ((rnd >> 9) + 1/2) / 2^23: exact in float32 */
  return (float)(rnd >> 9) * 0x1p-23f + 0x1p-24f;
}
AIE_HD static inline float aie_sampler_expf(float y) {
  /* (the guard is a select at the end: one straight line of 14 instructions on the device) */
  const float n = rintf(y * 0x1.715476p+0f);      /* round half to even */
  float r = fmaf(n, -0x1.62e4p-1f, y);            /* ln 2 = 0x1.62e4p-1 + 0x1.7f7d1cp-20: the first product is exact */
  r = fmaf(n, -0x1.7f7d1cp-20f, r);
  float p = 0x1.6c16c2p-10f;                      /* 1/6! */
  p = fmaf(p, r, 0x1.111112p-7f);                 /* 1/5! */
  p = fmaf(p, r, 0x1.555556p-5f);                 /* 1/4! */
  p = fmaf(p, r, 0x1.555556p-3f);                 /* 1/3! */
  p = fmaf(p, r, 0.5f);
  p = fmaf(p, r, 1.0f);
  p = fmaf(p, r, 1.0f);
  const int ni = y > -80.0f ? (int)n : 0;
  return y > -80.0f ? ldexpf(p, ni) : 0.0f;
}
/* the aligned lane segment a row of `len` entries is scanned in, and how many such rows share a wavefront */
AIE_HD static inline int aie_sampler_segment(int len) { return len <= 16 ? 16 : len <= 32 ? 32 : 64; }
AIE_HD static inline int aie_sampler_rows_per_wave(int len) { return 64 / aie_sampler_segment(len); }
/* products are rounded before they are added, wherever this header is included from (gcc: -ffp-contract=off) */
#if defined(__clang__)
#define AIE_NOCONTRACT _Pragma("clang fp contract(off)")
#else
#define AIE_NOCONTRACT
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define AIE_FDIV_RN(a, b) __fdiv_rn((a), (b)) /* the correctly rounded sequence whatever the compiler's flags */
#else
#define AIE_FDIV_RN(a, b) ((a) / (b))
#endif
AIE_HD static inline float aie_sampler_logf(float T) {
  AIE_NOCONTRACT
  uint32_t b;
  memcpy(&b, &T, 4);
  const uint32_t mant = b & 0x7fffffu;
  const int big = mant > 0x3504f3u;               /* m > sqrt(2): halve it */
  const int e = (int)(b >> 23) - 127 + big;
  const uint32_t mb = (big ? 0x3f000000u : 0x3f800000u) | mant;
  float m;
  memcpy(&m, &mb, 4);
  const float f = m - 1.0f;                       /* exact */
  float h = 0x1.07826ep-4f;
  h = fmaf(h, f, -0x1.dbcd16p-4f);
  h = fmaf(h, f, 0x1.ec6694p-4f);
  h = fmaf(h, f, -0x1.fd3baep-4f);
  h = fmaf(h, f, 0x1.22db42p-3f);
  h = fmaf(h, f, -0x1.554b4ap-3f);
  h = fmaf(h, f, 0x1.99a98p-3f);
  h = fmaf(h, f, -0x1.000064p-2f);
  h = fmaf(h, f, 0x1.55553cp-2f);
  h = fmaf(h, f, -0x1.fffffep-2f);
  const float t = f * f;
  const float lp = fmaf(t, h, f);
  const float fe = (float)e;
  return fmaf(fe, 0x1.62e4p-1f, fmaf(fe, 0x1.7f7d1cp-20f, lp));
}
/* One 64-entry chunk's inclusive prefix sums in the sampler's fixed order, in place (the CPU twin of the kernels' scan). */
AIE_HD static inline void aie_sampler_scan64(float* v, int seg) {
  float u[64];
  for (int d = 1; d <= 8; d <<= 1) {
    for (int r = 0; r < 64; ++r) u[r] = v[r] + ((r & 15) >= d ? v[r - d] : 0.0f);  /* (+ 0: what the kernel's row shift adds) */
    for (int r = 0; r < 64; ++r) v[r] = u[r];
  }
  if (seg >= 32) {
    for (int r = 0; r < 64; ++r) u[r] = ((r >> 4) & 1) ? v[r] + v[(r & ~15) - 1] : v[r];
    for (int r = 0; r < 64; ++r) v[r] = u[r];
  }
  if (seg >= 64)
    for (int r = 63; r >= 32; --r) v[r] = v[r] + v[31];
}
/* What a row's evaluation shares between its entries (the comment block above).  any = 0: nothing allowed or T = 0. */
typedef struct aie_policy_row {
  float M, T, S, L, H;
  int32_t any;
} aie_policy_row;
AIE_HD static inline int aie_policy_allowed(const float* x, const float* mask, int mks, int len, int k) {
  return k >= 0 && k < len && mask[(int64_t)k * mks] > 0.5f && x[k] == x[k];
}
AIE_HD static inline aie_policy_row aie_policy_row_stats(const float* x, const float* mask, int mks, int len) {
  AIE_NOCONTRACT
  aie_policy_row R;
  R.M = -INFINITY;
  R.T = R.S = R.L = R.H = 0.0f;
  R.any = 0;
  int n_ok = 0;
  for (int k = 0; k < len; ++k)
    if (aie_policy_allowed(x, mask, mks, len, k)) {
      if (!n_ok || x[k] > R.M) R.M = x[k];
      ++n_ok;
    }
  if (!n_ok) return R;
  const int nch = (len + 63) >> 6, seg = nch > 1 ? 64 : aie_sampler_segment(len);
  float cT = 0.0f, cS = 0.0f;
  for (int ch = 0; ch < nch; ++ch) {
    float w[64], v[64];
    for (int r = 0; r < 64; ++r) {
      const int k = 64 * ch + r;
      w[r] = v[r] = 0.0f;
      if (aie_policy_allowed(x, mask, mks, len, k)) {
        const float y = x[k] - R.M;
        w[r] = aie_sampler_expf(y);
        if (y > -80.0f) v[r] = w[r] * y;
      }
    }
    aie_sampler_scan64(w, seg);
    aie_sampler_scan64(v, seg);
    cT = cT + w[seg - 1];
    cS = cS + v[seg - 1];
  }
  R.T = cT;
  R.S = cS;
  if (!(R.T > 0.0f)) return R;
  R.any = 1;
  R.L = aie_sampler_logf(R.T);
  R.H = R.L - AIE_FDIV_RN(R.S, R.T);
  return R;
}
AIE_HD static inline float aie_policy_row_logp(const aie_policy_row* R, const float* x, const float* mask, int mks, int len, int a) {
  if (!R->any) return 0.0f;
  if (!aie_policy_allowed(x, mask, mks, len, a)) return -INFINITY;
  return (x[a] - R->M) - R->L;
}
/* one entry's gradient: w, y of an ALLOWED entry k of a row with any = 1; ind = [k = a]; g_logp already 0 for a stored
 * action that is not allowed */
AIE_HD static inline float aie_policy_entry_grad(float y, float w, float T, float L, float H, int ind, float g_logp, float g_H) {
  AIE_NOCONTRACT
  const float p = AIE_FDIV_RN(w, T);
  const float t1 = (ind ? 1.0f : 0.0f) - p;
  const float a1 = g_logp * t1;
  const float lh = (y - L) + H;
  const float t2 = y > -80.0f ? p * lh : 0.0f;
  const float t3 = g_H * t2;
  return a1 - t3;
}
/* What the evaluation kernels need, as their kernel argument (aie_policy_evaluate fills it): per actor class the caller's
 * pointers and the rows' shape.  Entry k of row r of batch element b: logit (and gradient) at b lg_bstride + r lrs + k, mask
 * at mk[b mk_bstride + r mrs + k mks] (mk: the caller's masks in the logits' layout, or the arena's own), action, logp,
 * entropy and their gradients at b rows + r.  items = wavefronts per batch element: as many whole rows as fit 64 lanes in
 * aligned segments of 1 << lsh lanes, or (generic: multi-action agents, rows of more than 64 entries) one row each. */
typedef struct aie_policy_eval_group {
  const float *lg, *mk;
  const int32_t* act;
  const float *g_logp, *g_ent;
  float *logp, *ent, *grad;
  uint32_t lg_bstride, mk_bstride;
  int32_t len, lrs, mrs, mks, lsh, rows, items, generic;
} aie_policy_eval_group;
typedef struct aie_policy_eval_args {
  aie_policy_eval_group agents, planner;
  const aie_params* params; /* the device copy: read for multi-action agents only */
  uint32_t B, items;        /* batch elements; wavefronts per batch element (both classes) */
  int32_t act_a_width, ragged; /* ragged: multi-action agents (rows of different lengths) */
} aie_policy_eval_args;
AIE_HD static inline void aie_policy_row_backward(const aie_policy_row* R, const float* x, const float* mask, int mks, int len,
                                                  int a, float g_logp, float g_H, float* g) {
  const float gl = aie_policy_allowed(x, mask, mks, len, a) ? g_logp : 0.0f;
  for (int k = 0; k < len; ++k) {
    g[k] = 0.0f;
    if (R->any && aie_policy_allowed(x, mask, mks, len, k)) {
      const float y = x[k] - R->M;
      g[k] = aie_policy_entry_grad(y, aie_sampler_expf(y), R->T, R->L, R->H, k == a, gl, g_H);
    }
  }
}
/* Generalised advantage estimation (include/aie.h: aie_gae), one step of the reverse recurrence down one column (replica,
 * actor): the plain serial float32 loop of every trainer, stated once -- the kernel calls it, tests/test_trajectory_cpu.py
 * compiles it.  gl = gamma * lambda as ONE rounded float32 product (aie_gae_gl), formed once per call;
 *   delta_t = done_t ? r_t - V_t : (r_t + gamma V_{t+1}) - V_t       A_t = done_t ? delta_t : delta_t + gl A_{t+1}
 * with every product and sum rounded on its own.  A done step SELECTS: V_{t+1} and A_{t+1} behind an episode end are the
 * restarted episode's (auto-reset) and take no part -- a NaN or an infinity there does not reach A_t (0 x NaN would).
 * The return is aie_gae_return(A_t, V_t) = A_t + V_t. */
AIE_HD static inline float aie_gae_gl(float gamma, float lambda) {
  AIE_NOCONTRACT
  return gamma * lambda;
}
AIE_HD static inline float aie_gae_step(float r, float v, float v_next, float a_next, int done, float gamma, float gl) {
  AIE_NOCONTRACT
  const float gv = gamma * v_next;
  const float rv = r + gv;
  const float delta = (done ? r : rv) - v;
  const float ga = gl * a_next;
  const float run = delta + ga;
  return done ? delta : run;
}
AIE_HD static inline float aie_gae_return(float a, float v) { return a + v; }
/* The kernel's argument (aie_gae fills it): 88 bytes.  A lane per float of a log row, lane c = e (n + 2) + j: j < n agent j,
 * j == n the planner, j == n + 1 (the done flag itself) idle.  Time t is ring slot (first + t) % slots. */
typedef struct aie_gae_args {
  const float *log, *va, *vp; /* the log; values [T + 1][E][n] / [T + 1][E] (NULL: the class is left out) */
  float *adv_a, *adv_p, *ret_a, *ret_p;
  int32_t T, slots, first, E, n;
  float gamma, gl;
} aie_gae_args;
/* The PPO loss (include/aie.h: aie_ppo_loss), stated once -- the kernels call these helpers, tests/test_ppo_loss_cpu.py
 * compiles them, tests/ppo_ref.py transcribes this comment.  float32, every operation rounded on its own (nothing fused
 * outside aie_sampler_expf / aie_sampler_logf), selects instead of min / max so that a NaN takes one stated way.
 * An ACTOR is one agent, or the planner, of one batch element, with w action slots (act_a_width / act_p_width) whose rows
 * are the evaluator's: slot s gives logp_s (aie_policy_row_logp) and H_s (aie_policy_row_stats) with their conventions.
 *   joint terms   ln = logp_0, then ln = ln + logp_s for s = 1 .. w - 1;  lo: the same sum over the stored old
 *                 log-probabilities;  He: the same sum over H_s;  d = ln - lo;
 *                 valid = every logp_s and every stored old logp finite, and |d| <= 80;
 *   advantage     A' = A, or (A - mean) * rstd with moments {mean, rstd} given;
 *   ratio         r = aie_sampler_expf(d) (exactly 1 at d = 0; good to 2.7 ulp over -80 .. 80);
 *                 lo_c = 1 - clip, hi_c = 1 + clip;  rc = r < lo_c ? lo_c : r, then rc > hi_c ? hi_c : rc;
 *                 u = r * A';  c = rc * A';  unclipped = (u <= c) (a tie goes to u, a NaN gives false);
 *                 surr = unclipped ? u : c;
 *   per actor     valid: policy term -surr, kl term -d, clip flag (r < lo_c || r > hi_c), |d|;  not valid: 0 each, and the
 *                 actor counts as skipped;
 *   slot gradient g_logp = (valid && unclipped) ? -(scale * u) : 0 for every slot of the actor;
 *                 g_H = -(scale * ent_coef) for every slot of every actor (the product formed once per call);
 *                 an entry's gradient is aie_policy_entry_grad with these two (aie_policy_row_backward is the row's loop
 *                 over it): exactly 0 at entries that are not allowed;
 *                 scale = 1.0f / (float)N, N = B x the class's actors per batch element;
 *   value         e1 = v - ret;  q1 = e1 * e1;  with vf_clip <= 0: vf = q1, dq = e1;  with vf_clip > 0:
 *                 dv = v - v_old;  dc = dv < -vf_clip ? -vf_clip : dv, then dc > vf_clip ? vf_clip : dc;  vc = v_old + dc;
 *                 e2 = vc - ret;  q2 = e2 * e2;  first = (q1 >= q2);  vf = first ? q1 : q2;
 *                 dq = first ? e1 : (dc == dv ? e2 : 0);
 *                 grad_v = kv * (dq + dq), kv = scale * vf_coef (formed once per call); for every actor, valid or not;
 *   statistics    float64 sums over the float32 terms of all N actors (an actor that is not valid adds 0 to the policy, kl
 *                 and clip sums), each mean = sum / N in float64 rounded once to float32 (aie_ppo_finish_stats):
 *                 [0] loss = P + vf_coef V - ent_coef E from the float64 means, rounded once;  [1] P, the mean policy term;
 *                 [2] V, the mean vf (0 without values);  [3] E, the mean He;  [4] the mean kl term;  [5] the mean clip
 *                 flag;  [6] the number of skipped actors;  [7] the maximum |d| over valid actors (0 if none).
 * Non-finite advantages, values and returns are the caller's own: they propagate. */
AIE_HD static inline int aie_ppo_finite(float x) {
  uint32_t b;
  memcpy(&b, &x, 4);
  return (b & 0x7f800000u) != 0x7f800000u;
}
/* one step of a joint term (ln, lo, He): slot s's value joins the sum of the slots before it */
AIE_HD static inline float aie_ppo_joint_add(float acc, float term, int s) {
  AIE_NOCONTRACT
  return s ? acc + term : term;
}
AIE_HD static inline float aie_ppo_scale(int64_t N) { return 1.0f / (float)N; }
AIE_HD static inline float aie_ppo_product(float a, float b) {  /* scale * ent_coef, scale * vf_coef: one rounded product */
  AIE_NOCONTRACT
  return a * b;
}
AIE_HD static inline float aie_ppo_advantage(float A, int has_moments, float mean, float rstd) {
  AIE_NOCONTRACT
  const float c = A - mean;
  const float s = c * rstd;
  return has_moments ? s : A;
}
typedef struct aie_ppo_actor {
  float pol, kl, clipf, absd, g_logp; /* the per-actor terms (0 for an actor that is not valid); every slot's g_logp */
  int32_t valid;
} aie_ppo_actor;
/* finite: every logp_s and every stored old logp of the actor is finite (aie_ppo_finite) */
AIE_HD static inline aie_ppo_actor aie_ppo_actor_terms(float ln, float lo, int finite, float Ap, float clip, float scale) {
  AIE_NOCONTRACT
  aie_ppo_actor R;
  const float d = ln - lo;
  const int valid = finite && fabsf(d) <= 80.0f;
  const float r = aie_sampler_expf(valid ? d : 0.0f);
  const float lo_c = 1.0f - clip, hi_c = 1.0f + clip;
  float rc = r < lo_c ? lo_c : r;
  rc = rc > hi_c ? hi_c : rc;
  const float u = r * Ap;
  const float c = rc * Ap;
  const int unclipped = u <= c;
  const float surr = unclipped ? u : c;
  const float su = scale * u;
  R.valid = valid;
  R.pol = valid ? -surr : 0.0f;
  R.kl = valid ? -d : 0.0f;
  R.clipf = (valid && (r < lo_c || r > hi_c)) ? 1.0f : 0.0f;
  R.absd = valid ? fabsf(d) : 0.0f;
  R.g_logp = (valid && unclipped) ? -su : 0.0f;
  return R;
}
typedef struct aie_ppo_value {
  float vf, grad;
} aie_ppo_value;
AIE_HD static inline aie_ppo_value aie_ppo_value_terms(float v, float v_old, float ret, float vf_clip, float kv) {
  AIE_NOCONTRACT
  aie_ppo_value R;
  const float e1 = v - ret;
  const float q1 = e1 * e1;
  float vf = q1, dq = e1;
  if (vf_clip > 0.0f) {
    const float dv = v - v_old;
    float dc = dv < -vf_clip ? -vf_clip : dv;
    dc = dc > vf_clip ? vf_clip : dc;
    const float vc = v_old + dc;
    const float e2 = vc - ret;
    const float q2 = e2 * e2;
    const int first = q1 >= q2;
    vf = first ? q1 : q2;
    dq = first ? e1 : (dc == dv ? e2 : 0.0f);
  }
  const float dq2 = dq + dq;
  R.vf = vf;
  R.grad = kv * dq2;
  return R;
}
/* sums: the class's eight float64 totals ([1] .. [5] sums of the terms, [6] the skipped count, [7] the maximum; [0] unused) */
AIE_HD static inline void aie_ppo_finish_stats(const double* sums, double N, float vf_coef, float ent_coef, float* stats) {
  AIE_NOCONTRACT
  const double P = sums[1] / N, V = sums[2] / N, E = sums[3] / N;
  const double cv = (double)vf_coef * V, ce = (double)ent_coef * E;
  const double pv = P + cv;
  stats[0] = (float)(pv - ce);
  stats[1] = (float)P;
  stats[2] = (float)V;
  stats[3] = (float)E;
  stats[4] = (float)(sums[4] / N);
  stats[5] = (float)(sums[5] / N);
  stats[6] = (float)sums[6];
  stats[7] = (float)sums[7];
}
/* The kernels' argument (aie_ppo_loss fills it; the rows' shape is the evaluator's, aie_policy_eval_group).  Batch element
 * b reads logits, values and writes both gradients at row b; everything stored (masks in the logits' layout, actions, old
 * logp, advantages, old values, returns) at row index[b] (index NULL: b).  An actor has w slots; items = wavefront-sized
 * work items per batch element: whole single-slot rows in aligned segments of 1 << lsh lanes, or (generic: w > 1, ragged
 * rows, rows of more than 64 entries) one actor each.  `waves` wavefronts (at most AIE_PPO_MAX_WAVES, at most the work
 * items) stride over B x items work items and leave one
 * record of 2 x 8 float64 (agents, planner) each in the workspace; the second launch adds the records in index order. */
typedef struct aie_ppo_group {
  const float *lg, *val, *mk;
  const int32_t* act;
  const float *lp_old, *adv, *val_old, *ret, *mom;
  float *grad, *grad_v, *stats;
  float clip, vf_clip, vf_coef, ent_coef, scale, g_H, kv;
  uint32_t lg_bstride;
  int32_t len, lrs, lsh, rows, w, actors, items, generic;
} aie_ppo_group;
typedef struct aie_ppo_args {
  aie_ppo_group agents, planner;
  const aie_params* params; /* the device copy: read for multi-action agents only */
  const int32_t* index;
  double* ws;
  uint32_t B, items, waves;
  int32_t act_a_width, ragged;
} aie_ppo_args;
#define AIE_PPO_RECORD 16 /* float64 per wavefront's record */

/* The policy network's forward pass (include/aie.h: aie_policy_mlp_forward), stated once -- the kernel's MFMA chains equal
 * these helpers value for value, tests/test_policy_mlp_cpu.py compiles them with the host compiler against an independent
 * transcription (tests/policy_mlp_ref.py).  A row x[F] goes through two hidden layers of width H and a head of width M,
 * with an optional value column; every number is float32:
 *   chain(c; a, w) = acc, where acc = c and then, for k = 0, 1, ... ascending, acc = fmaf(a[k], w[k], acc): ONE accumulator,
 *                    one rounding per term, nothing wider in between and no other order;
 *   relu(v)        = v > 0 ? v : 0 (so a NaN becomes 0);
 *   h1[j] = relu(chain(b1[j]; x, column j of W1)),  h2[j] = relu(chain(b2[j]; h1, column j of W2)),
 *   logits[j] = chain(b3[j]; h2, column j of W3),   value = chain(bv; h2, wv).
 * Weights are row-major [in, out] with a leading dimension (entry (k, j) at w[k * ld + j]): what x @ w takes.
 * A kernel may append terms with a zero weight behind the real ones (K padded to the MFMA's depth): fmaf(a, 0, acc) = acc
 * for finite a, except that an accumulator of -0 becomes +0 -- so the device equals these helpers under float ==, with no
 * NaN anywhere, not in the bit pattern of an exact zero.  It may not split K across accumulators. */
AIE_HD static inline float aie_mlp_relu(float v) { return v > 0.0f ? v : 0.0f; }
AIE_HD static inline float aie_mlp_chain(float c, const float* a, const float* w, int64_t w_ld, int K) {
  float acc = c;
  for (int k = 0; k < K; ++k) acc = fmaf(a[k], w[(int64_t)k * w_ld], acc);
  return acc;
}
/* one row; h1 and h2 are the caller's scratch of H floats each; wv NULL: no value (value is not written) */
AIE_HD static inline void aie_mlp_row(const float* x, int F, int H, int M, const float* w1, const float* b1, const float* w2,
                                      const float* b2, const float* w3, const float* b3, const float* wv, const float* bv,
                                      float* h1, float* h2, float* logits, float* value) {
  for (int j = 0; j < H; ++j) h1[j] = aie_mlp_relu(aie_mlp_chain(b1[j], x, w1 + j, H, F));
  for (int j = 0; j < H; ++j) h2[j] = aie_mlp_relu(aie_mlp_chain(b2[j], h1, w2 + j, H, H));
  for (int j = 0; j < M; ++j) logits[j] = aie_mlp_chain(b3[j], h2, w3 + j, M, H);
  if (wv) *value = aie_mlp_chain(bv[0], h2, wv, 1, H);
}
/* The kernel's argument (aie_policy_mlp_forward fills it).  A workgroup owns AIE_MLP_TILE_ROWS rows of one class: workgroups
 * [0, agents.blocks) the agents' tiles, the rest the planner's.  lds_a / lds_h: the row strides (floats) of its two LDS
 * images, [tile][lds_a] (the observation chunk, later h2) and [tile][lds_h] (h1); both are 2 mod 4, which spreads a
 * fragment read's 16 rows x 2 columns over 32 banks. */
#ifndef AIE_MLP_TILE_ROWS
#define AIE_MLP_TILE_ROWS 32   /* rows per workgroup, 32 or 64 (DESIGN.md section 3 has the measurement behind the choice) */
#endif
#define AIE_MLP_CHUNK 256      /* observation columns staged at a time: F <= 256 is one chunk */
typedef struct aie_mlp_group {
  const float *x, *w1, *b1, *w2, *b2, *w3, *b3, *wv, *bv;
  float *logits, *values;
  int64_t x_ld, rows;
  int32_t F, H, M, blocks, lds_a, lds_h;
} aie_mlp_group;
typedef struct aie_mlp_args {
  aie_mlp_group agents, planner;
} aie_mlp_args;

/* The policy network's backward pass (include/aie.h: aie_policy_mlp_backward), stated once -- the weights' gradients from
 * the gradients with respect to logits and values; tests/test_policy_mlp_backward_cpu.py compiles these helpers against an
 * independent transcription (tests/policy_mlp_bwd_ref.py).  All float32 unless said otherwise; chain0(a, w) = chain(+0; a, w).
 * Per row r (g_logits [rows, M] contiguous, g_values [rows], NULL exactly when wv is):
 *   h1, h2       recomputed exactly as aie_mlp_row computes them;
 *   dz3[m] = g_logits[r][m], dv = g_values[r];
 *   dh2[j] = chain0 over m = 0 .. M-1 ascending of (dz3[m], W3[j][m]), with a value column one last term fmaf(dv, wv[j], acc)
 *            (the value column is column M, as in the forward);
 *   dz2[j] = h2[j] > 0 ? dh2[j] : 0;
 *   dh1[j] = chain0 over k = 0 .. H-1 ascending of (dz2[k], W2[j][k]);   dz1[j] = h1[j] > 0 ? dh1[j] : 0.
 * Across rows: rows are cut into segments of AIE_MLP_BWD_SEG consecutive rows (the last may be short).  With the layers'
 * activations a_1 = x, a_2 = h1, a_3 = h2,
 *   partial_s(gW_L[k][j]) = chain0 over the rows r of segment s, ascending, of (a_L[r][k], dz_L[r][j]),
 * gwv[k] pairs (h2[r][k], dv[r]), and the bias gradients are the same chain with the activation 1 (acc = acc + dz, rounded
 * once per row).  A gradient entry is the sum of its segment partials in float64, in ascending segment order, rounded to
 * float32 once (aie_ppo_loss's convention).  Nothing is produced for x.  Every entry is overwritten.
 * AIE_MLP_BWD_SEG is this constant and nothing else -- not the device, not B, not the launch geometry -- so the bits do
 * not depend on how many compute units ran the call.  As in the forward, a kernel may pad a chain with zero-times-zero
 * terms behind the real ones: that changes nothing except the sign of an exact zero.  No float atomics anywhere. */
#if AIE_MLP_BWD_SEG % AIE_MLP_TILE_ROWS   /* (include/aie.h defines it, 256: the formula of the workspace needs it there) */
#error "AIE_MLP_BWD_SEG is a multiple of AIE_MLP_TILE_ROWS"
#endif
/* one row: h1, h2 (as aie_mlp_row's), dz2 and dz1, H floats each; g_values_r is read only with wv */
AIE_HD static inline void aie_mlp_row_backward(const float* x, int F, int H, int M, const float* w1, const float* b1, const float* w2,
                                               const float* b2, const float* w3, const float* wv, const float* g_logits_r,
                                               float g_value_r, float* h1, float* h2, float* dz2, float* dz1) {
  for (int j = 0; j < H; ++j) h1[j] = aie_mlp_relu(aie_mlp_chain(b1[j], x, w1 + j, H, F));
  for (int j = 0; j < H; ++j) h2[j] = aie_mlp_relu(aie_mlp_chain(b2[j], h1, w2 + j, H, H));
  for (int j = 0; j < H; ++j) {
    float acc = aie_mlp_chain(0.0f, g_logits_r, w3 + (int64_t)j * M, 1, M);
    if (wv) acc = fmaf(g_value_r, wv[j], acc);
    dz2[j] = h2[j] > 0.0f ? acc : 0.0f;
  }
  for (int j = 0; j < H; ++j) {
    const float acc = aie_mlp_chain(0.0f, dz2, w2 + (int64_t)j * H, 1, H);
    dz1[j] = h1[j] > 0.0f ? acc : 0.0f;
  }
}
/* one gradient entry: a (NULL: the constant 1, a bias) and d are columns of row-major arrays, entry r at a[r * a_ld] */
AIE_HD static inline float aie_mlp_grad_entry(const float* a, int64_t a_ld, const float* d, int64_t d_ld, int64_t rows) {
  double sum = 0.0;
  for (int64_t r0 = 0; r0 < rows; r0 += AIE_MLP_BWD_SEG) {
    const int64_t r1 = r0 + AIE_MLP_BWD_SEG < rows ? r0 + AIE_MLP_BWD_SEG : rows;
    float acc = 0.0f;
    for (int64_t r = r0; r < r1; ++r) acc = fmaf(a ? a[r * a_ld] : 1.0f, d[r * d_ld], acc);
    sum += (double)acc;
  }
  return (float)sum;
}
/* The whole pass of one class on the host.  scratch: 4 * rows * H floats (h1, h2, dz2, dz1 as [rows, H] each). */
static inline void aie_mlp_backward_host(const float* x, int64_t x_ld, int64_t rows, int F, int H, int M, const float* w1,
                                         const float* b1, const float* w2, const float* b2, const float* w3, const float* wv,
                                         const float* g_logits, const float* g_values, float* scratch, float* gw1, float* gb1,
                                         float* gw2, float* gb2, float* gw3, float* gb3, float* gwv, float* gbv) {
  float *h1 = scratch, *h2 = h1 + rows * H, *dz2 = h2 + rows * H, *dz1 = dz2 + rows * H;
  for (int64_t r = 0; r < rows; ++r)
    aie_mlp_row_backward(x + r * x_ld, F, H, M, w1, b1, w2, b2, w3, wv, g_logits + r * M, wv ? g_values[r] : 0.0f, h1 + r * H,
                         h2 + r * H, dz2 + r * H, dz1 + r * H);
  for (int j = 0; j < H; ++j) {
    for (int k = 0; k < F; ++k) gw1[(int64_t)k * H + j] = aie_mlp_grad_entry(x + k, x_ld, dz1 + j, H, rows);
    for (int k = 0; k < H; ++k) gw2[(int64_t)k * H + j] = aie_mlp_grad_entry(h1 + k, H, dz2 + j, H, rows);
    gb1[j] = aie_mlp_grad_entry(0, 0, dz1 + j, H, rows);
    gb2[j] = aie_mlp_grad_entry(0, 0, dz2 + j, H, rows);
  }
  for (int j = 0; j < M; ++j) {
    for (int k = 0; k < H; ++k) gw3[(int64_t)k * M + j] = aie_mlp_grad_entry(h2 + k, H, g_logits + j, M, rows);
    gb3[j] = aie_mlp_grad_entry(0, 0, g_logits + j, M, rows);
  }
  if (wv) {
    for (int k = 0; k < H; ++k) gwv[k] = aie_mlp_grad_entry(h2 + k, H, g_values, 1, rows);
    gbv[0] = aie_mlp_grad_entry(0, 0, g_values, 1, rows);
  }
}
/* The kernels' argument (aie_policy_mlp_backward fills it).  net: the forward's group (logits / values unused; blocks the
 * row tiles).  The workspace per class: h1, h2, dz2, dz1 as [rows, H] each, then the segments' partials [nseg][P], one
 * float per gradient entry in three blocks [(K + 1), N] -- (F + 1, H), (H + 1, H), (H + 1, M + value) -- whose last row
 * is the bias and, in the third, whose column M is the value head.  An ITEM is one workgroup's work in the second launch:
 * four 16-row bands of a layer's block (one per wave) by up to four 16-column tiles, over one segment's rows. */
typedef struct aie_mlp_bwd_group {
  aie_mlp_group net;
  const float *g_logits, *g_values;
  float *h1, *h2, *dz2, *dz1, *partial;
  float *gw1, *gb1, *gw2, *gb2, *gw3, *gb3, *gwv, *gbv;
  int32_t lds_c, nseg, P, off2, off3, N3;   /* the staged dz3 chunk's row stride; segments; entries; the blocks' offsets; M + value */
  int32_t cg[3], items[3], per_seg;         /* per layer: column groups, items per segment; their sum */
  int64_t n_items;                          /* nseg * per_seg */
} aie_mlp_bwd_group;
typedef struct aie_mlp_bwd_args {
  aie_mlp_bwd_group agents, planner;
  int32_t reduce_blocks_a;                  /* the third launch: workgroups [0, reduce_blocks_a) are the agents' */
} aie_mlp_bwd_args;
/* The gradient with respect to the MLP's input (include/aie.h: aie_policy_mlp_input_grad), one entry: dz1_r is row r of
 * aie_mlp_row_backward's dz1, w1 the first layer's [F, H] weights. */
AIE_HD static inline float aie_mlp_input_grad_entry(const float* dz1_r, const float* w1, int H, int j) {
  return aie_mlp_chain(0.0f, dz1_r, w1 + (int64_t)j * H, 1, H);
}
typedef struct aie_mlp_igrad_group {
  const float *dz1, *w1;
  float* g_x;
  int64_t ld, rows;
  int32_t H, ncols, tiles, cgroups, blocks, pad_; /* row tiles of AIE_IGRAD_TILE; groups of 256 columns; their product */
} aie_mlp_igrad_group;
typedef struct aie_mlp_igrad_args {
  aie_mlp_igrad_group agents, planner;
} aie_mlp_igrad_args;
#define AIE_IGRAD_TILE 16 /* rows a workgroup carries per weight it reads */

/* The convolutional encoder (include/aie.h: aie_policy_conv_forward / _backward), stated once -- the kernels call these
 * helpers output by output, tests/test_policy_conv_cpu.py compiles them against an independent transcription
 * (tests/policy_conv_ref.py).  A row's images, in the layouts the helpers and the kernels' LDS share:
 *   X  [h w][C]     the input, cell-major: X[(y w + x) C + c] (aie_conv_input_at gives one entry from the caller's tensors)
 *   a1 [oh1 ow1][F1], a2 = the features [oh2 ow2][F2];  dz1, dz2 likewise;
 *   dxe [2 h w][D]  the input gradient of the embedding's channels: dxe[(i h w + y w + x) D + d] is channel C_map + i D + d.
 * Every chain is the MLP's: one accumulator, ascending, one fmaf per term. */
typedef struct aie_conv_shape {
  int32_t C_map, D, h, w, V, C, oh1, ow1, oh2, ow2, P1, P2, NF, hw;
} aie_conv_shape;
AIE_HD static inline aie_conv_shape aie_conv_shape_of(int C_map, int D, int h, int w, int V) {
  aie_conv_shape S;
  S.C_map = C_map, S.D = D, S.h = h, S.w = w, S.V = V, S.C = C_map + 2 * D, S.hw = h * w;
  S.oh1 = (h - 3) / 2 + 1, S.ow1 = (w - 3) / 2 + 1;
  S.oh2 = (S.oh1 - 3) / 2 + 1, S.ow2 = (S.ow1 - 3) / 2 + 1;
  S.P1 = S.oh1 * S.ow1, S.P2 = S.oh2 * S.ow2, S.NF = S.P2 * AIE_CONV_F2;
  return S;
}
AIE_HD static inline int aie_conv_clamp(int v, int V) { return v < 0 ? 0 : v >= V ? V - 1 : v; }
/* channel c of cell `cell` of a row's input: map_r and idx_r are the row's [C_map][h w] and [2][h w] */
AIE_HD static inline float aie_conv_input_at(const aie_conv_shape* S, const float* map_r, const int16_t* idx_r, const float* emb,
                                             int c, int cell) {
  if (c < S->C_map) return map_r[c * S->hw + cell];
  const int e = c - S->C_map, i = e / S->D, d = e - i * S->D;
  return emb[aie_conv_clamp(idx_r[i * S->hw + cell], S->V) * S->D + d];
}
/* one output of a 3x3 stride-2 convolution over src [.. sw][sc] (cell-major), weights [9 sc][nf], from its bias, with ReLU */
AIE_HD static inline float aie_conv_out(const float* src, int sw, int sc, const float* wt, int nf, float bias, int oy, int ox, int f) {
  float acc = bias;
  for (int ky = 0; ky < 3; ++ky)
    for (int kx = 0; kx < 3; ++kx) {
      const float* s = src + ((2 * oy + ky) * sw + 2 * ox + kx) * sc;
      const float* q = wt + (ky * 3 + kx) * sc * nf + f;
      for (int c = 0; c < sc; ++c) acc = fmaf(s[c], q[c * nf], acc);
    }
  return aie_mlp_relu(acc);
}
AIE_HD static inline float aie_conv1_out(const aie_conv_shape* S, const float* X, const float* w1, const float* b1, int p, int f) {
  return aie_conv_out(X, S->w, S->C, w1, AIE_CONV_F1, b1[f], p / S->ow1, p % S->ow1, f);
}
AIE_HD static inline float aie_conv2_out(const aie_conv_shape* S, const float* a1, const float* w2, const float* b2, int p, int f) {
  return aie_conv_out(a1, S->ow1, AIE_CONV_F1, w2, AIE_CONV_F2, b2[f], p / S->ow2, p % S->ow2, f);
}
/* the gradient with respect to input (y, x, c) of such a convolution with on x ow outputs: over the outputs (oy, ox)
 * ascending whose window holds (y, x), and inside one over f ascending, of (dz[oy][ox][f], wt[(ky 3 + kx) sc + c][f]) */
AIE_HD static inline float aie_conv_input_grad(const float* dz, int on, int ow, const float* wt, int sc, int nf, int y, int x, int c) {
  float acc = 0.0f;
  for (int oy = 0; oy < on; ++oy) {
    const int ky = y - 2 * oy;
    if (ky < 0 || ky > 2) continue;
    for (int ox = 0; ox < ow; ++ox) {
      const int kx = x - 2 * ox;
      if (kx < 0 || kx > 2) continue;
      const float* d = dz + (oy * ow + ox) * nf;
      const float* q = wt + ((ky * 3 + kx) * sc + c) * nf;
      for (int f = 0; f < nf; ++f) acc = fmaf(d[f], q[f], acc);
    }
  }
  return acc;
}
AIE_HD static inline float aie_conv_da1(const aie_conv_shape* S, const float* dz2, const float* w2, int p, int c) {
  return aie_conv_input_grad(dz2, S->oh2, S->ow2, w2, AIE_CONV_F1, AIE_CONV_F2, p / S->ow1, p % S->ow1, c);
}
/* e = i D + d: the embedding's channel C_map + e */
AIE_HD static inline float aie_conv_dx(const aie_conv_shape* S, const float* dz1, const float* w1, int cell, int e) {
  return aie_conv_input_grad(dz1, S->oh1, S->ow1, w1, S->C, AIE_CONV_F1, cell / S->w, cell % S->w, S->C_map + e);
}
/* a row's forward on the host: X [h w C], a1 [P1 F1], feat [NF] */
static inline void aie_conv_row_forward(const aie_conv_shape* S, const float* map_r, const int16_t* idx_r, const float* emb,
                                        const float* w1, const float* b1, const float* w2, const float* b2, float* X, float* a1,
                                        float* feat) {
  for (int cell = 0; cell < S->hw; ++cell)
    for (int c = 0; c < S->C; ++c) X[cell * S->C + c] = aie_conv_input_at(S, map_r, idx_r, emb, c, cell);
  for (int p = 0; p < S->P1; ++p)
    for (int f = 0; f < AIE_CONV_F1; ++f) a1[p * AIE_CONV_F1 + f] = aie_conv1_out(S, X, w1, b1, p, f);
  for (int p = 0; p < S->P2; ++p)
    for (int f = 0; f < AIE_CONV_F2; ++f) feat[p * AIE_CONV_F2 + f] = aie_conv2_out(S, a1, w2, b2, p, f);
}
/* a row's share of the embedding's gradient: table [V D], every entry written */
AIE_HD static inline void aie_conv_row_emb(const aie_conv_shape* S, const int16_t* idx_r, const float* dxe, float* table) {
  for (int j = 0; j < S->V * S->D; ++j) table[j] = 0.0f;
  for (int ic = 0; ic < 2 * S->hw; ++ic) {
    float* t = table + aie_conv_clamp(idx_r[ic], S->V) * S->D;
    for (int d = 0; d < S->D; ++d) t[d] = t[d] + dxe[ic * S->D + d];
  }
}
/* one weight-gradient entry's segment chain continued over one row: act(p) is the entry's activation at output p (the
 * constant 1 for a bias: acc + dz, which fmaf(1, dz, acc) equals) */
#define AIE_CONV_GRAD_ROW(acc, P, nf, f, dz_r, ACT)                                              \
  for (int p_ = 0; p_ < (P); ++p_) (acc) = fmaf((ACT), (dz_r)[p_ * (nf) + (f)], (acc))
/* The whole backward on the host.  scratch: rows (h w C + 2 P1 F1 + 2 NF + 2 h w D) + V D floats. */
static inline void aie_conv_backward_host(const aie_conv_shape* S, int64_t rows, const float* map, int64_t map_ld, const int16_t* idx,
                                          int64_t idx_ld, const float* emb, const float* w1, const float* b1, const float* w2,
                                          const float* b2, const float* g_feat, int64_t g_ld, float* scratch, float* gemb, float* gw1,
                                          float* gb1, float* gw2, float* gb2) {
  const int C = S->C, P1 = S->P1, P2 = S->P2, NF = S->NF, hwC = S->hw * C, n1 = P1 * AIE_CONV_F1, nx = 2 * S->hw * S->D;
  float *X = scratch, *a1 = X + rows * hwC, *dz1 = a1 + rows * n1, *a2 = dz1 + rows * n1, *dz2 = a2 + rows * NF,
        *dxe = dz2 + rows * NF, *table = dxe + rows * nx;
  for (int64_t r = 0; r < rows; ++r) {
    float *Xr = X + r * hwC, *a1r = a1 + r * n1, *dz1r = dz1 + r * n1, *a2r = a2 + r * NF, *dz2r = dz2 + r * NF;
    aie_conv_row_forward(S, map + r * map_ld, idx + r * idx_ld, emb, w1, b1, w2, b2, Xr, a1r, a2r);
    for (int j = 0; j < NF; ++j) dz2r[j] = a2r[j] > 0.0f ? g_feat[r * g_ld + j] : 0.0f;
    for (int p = 0; p < P1; ++p)
      for (int c = 0; c < AIE_CONV_F1; ++c)
        dz1r[p * AIE_CONV_F1 + c] = a1r[p * AIE_CONV_F1 + c] > 0.0f ? aie_conv_da1(S, dz2r, w2, p, c) : 0.0f;
    for (int cell = 0; cell < S->hw; ++cell)
      for (int e = 0; e < 2 * S->D; ++e)
        dxe[r * nx + ((e / S->D) * S->hw + cell) * S->D + e % S->D] = aie_conv_dx(S, dz1r, w1, cell, e);
  }
  /* the weights: k = (ky 3 + kx) sc + c reads the activation at (2 oy + ky, 2 ox + kx, c); the last row is the bias */
  for (int L = 0; L < 2; ++L) {
    const int sc = L ? AIE_CONV_F1 : C, nf = L ? AIE_CONV_F2 : AIE_CONV_F1, P = L ? P2 : P1, ow = L ? S->ow2 : S->ow1,
              sw = L ? S->ow1 : S->w;
    const float *act = L ? a1 : X, *dz = L ? dz2 : dz1;
    const int64_t act_ld = L ? n1 : hwC, dz_ld = (int64_t)P * nf;
    float *gw = L ? gw2 : gw1, *gb = L ? gb2 : gb1;
    for (int k = 0; k <= 9 * sc; ++k)
      for (int f = 0; f < nf; ++f) {
        const int t = k / sc, ky = t / 3, kx = t % 3, c = k % sc;
        double sum = 0.0;
        for (int64_t r0 = 0; r0 < rows; r0 += AIE_MLP_BWD_SEG) {
          const int64_t r1 = r0 + AIE_MLP_BWD_SEG < rows ? r0 + AIE_MLP_BWD_SEG : rows;
          float acc = 0.0f;
          for (int64_t r = r0; r < r1; ++r) {
            const float* ar = act + r * act_ld;
            if (k < 9 * sc) AIE_CONV_GRAD_ROW(acc, P, nf, f, dz + r * dz_ld, ar[((2 * (p_ / ow) + ky) * sw + 2 * (p_ % ow) + kx) * sc + c]);
            else AIE_CONV_GRAD_ROW(acc, P, nf, f, dz + r * dz_ld, 1.0f);
          }
          sum += (double)acc;
        }
        if (k < 9 * sc) gw[k * nf + f] = (float)sum;
        else gb[f] = (float)sum;
      }
  }
  /* the embedding: a row's table, then the segment's rows ascending, then the segments in float64 */
  const int VD = S->V * S->D;
  for (int j = 0; j < VD; ++j) gemb[j] = 0.0f;
  double* sums = (double*)malloc(sizeof(double) * (size_t)VD);
  float* accs = (float*)malloc(sizeof(float) * (size_t)VD);
  for (int j = 0; j < VD; ++j) sums[j] = 0.0;
  for (int64_t r0 = 0; r0 < rows; r0 += AIE_MLP_BWD_SEG) {
    const int64_t r1 = r0 + AIE_MLP_BWD_SEG < rows ? r0 + AIE_MLP_BWD_SEG : rows;
    for (int j = 0; j < VD; ++j) accs[j] = 0.0f;
    for (int64_t r = r0; r < r1; ++r) {
      aie_conv_row_emb(S, idx + r * idx_ld, dxe + r * nx, table);
      for (int j = 0; j < VD; ++j) accs[j] = accs[j] + table[j];
    }
    for (int j = 0; j < VD; ++j) sums[j] += (double)accs[j];
  }
  for (int j = 0; j < VD; ++j) gemb[j] = (float)sums[j];
  free(sums);
  free(accs);
}
/* The kernels' arguments (aie_policy_conv_forward / _backward fill them: aie_trainer_plan.h).  A workgroup of the forward
 * and of the backward's first launch owns `tr` consecutive rows, staged in LDS as [tr][lds_row] floats: X, a1, and in the
 * backward a2, dz2 and dz1 behind them.  The backward's workspace: a1, dz1 [rows][P1 F1], dz2 [rows][NF], dxe
 * [rows][2 h w D], then the segments' partials [nseg][Pn]: three blocks [(9 C + 1), F1], [(9 F1 + 1), F2], [V, D]. */
typedef struct aie_conv_args {
  const float* map;
  const int16_t* idx;
  const float *emb, *w1, *b1, *w2, *b2, *flat;
  float* x_out;
  int64_t map_ld, idx_ld, flat_ld, x_ld, rows;
  aie_conv_shape S;
  int32_t F_flat, tr, lds_row, pad_;
} aie_conv_args;
typedef struct aie_conv_bwd_args {
  aie_conv_args net;
  const float* g_feat;
  int64_t g_ld;
  float *a1, *dz1, *dz2, *dxe, *partial;
  float *gemb, *gw1, *gb1, *gw2, *gb2;
  int32_t nseg, Pn, off2, off3, chunks, pad_;   /* segments; entries; the blocks' offsets; workgroups per segment of the weights' blocks */
} aie_conv_bwd_args;
#define AIE_CONV_EMB_TILE 16 /* rows whose embedding tables a segment's workgroup holds in LDS at a time */

/* Adam with gradient-norm clipping (include/aie.h: aie_adam_step), stated once -- the kernels call these helpers,
 * tests/test_adam_cpu.py compiles them, tests/optim_ref.py transcribes include/aie.h's text.
 *   aie_opt_chunk_sumsq  one chunk's sum of squares in float64: 256 slots of four consecutive elements each, added ascending
 *                        from +0, then the butterfly slot[i] += slot[i ^ 2^L], L = 0 .. 7 (the kernel's six cross-lane steps
 *                        and its four wave sums through LDS: (s0 + s1) + (s2 + s3)).  The product (double)g * (double)g is
 *                        exact (48 bits), so fusing it into the addition changes nothing;
 *   aie_opt_scalars      the group's float64 scalars from n2 (its chunks' sums added ascending from +0) and the old state,
 *                        rounded to float32 once; skipped = n2 is not finite: the new state is the old one;
 *   aie_opt_element      one element's float32 step, every operation rounded on its own. */
/* sqrtf is the correctly rounded one on the device too: hipcc's default (-fhip-fp32-correctly-rounded-divide-sqrt), which
 * the library's build leaves alone; HIP's __fsqrt_rn is the hardware's approximation here, so it is not used */
#define AIE_OPT_SLOTS (AIE_OPT_CHUNK / 4)
#if AIE_OPT_SLOTS != 256
#error "a chunk is 256 slots of four elements: the butterfly has eight levels"
#endif
typedef struct aie_opt_state {   /* d_state: AIE_OPT_STATE_BYTES */
  int64_t t;
  double p1, p2;                 /* beta1^t, beta2^t (unused while t == 0) */
  int64_t pad_;
} aie_opt_state;
/* (a comparison, false for a NaN and for both infinities -- not the bits through an 8-byte memcpy: on the device memcpy is a
 * function the compiler specialises on its callers' sizes, and a second size beside aie_sampler_logf's 4 reorders the
 * instructions of every kernel that inlines that one: profiles/adam_step_isa.txt) */
AIE_HD static inline int aie_opt_finite(double x) {
  return fabs(x) <= 1.7976931348623157e308;
}
/* a slot's four elements: count = how many of them exist (1 .. 4) */
AIE_HD static inline double aie_opt_slot_sumsq(const float* g, int count) {
  double acc = 0.0;
  for (int k = 0; k < count; ++k) acc += (double)g[k] * (double)g[k];
  return acc;
}
AIE_HD static inline double aie_opt_chunk_sumsq(const float* g, int64_t count) {   /* count: 1 .. AIE_OPT_CHUNK */
  double slot[AIE_OPT_SLOTS], next[AIE_OPT_SLOTS];
  for (int s = 0; s < AIE_OPT_SLOTS; ++s) {
    const int64_t left = count - 4 * (int64_t)s;
    slot[s] = left > 0 ? aie_opt_slot_sumsq(g + 4 * s, left < 4 ? (int)left : 4) : 0.0;
  }
  for (int L = 0; L < 8; ++L) {
    for (int i = 0; i < AIE_OPT_SLOTS; ++i) next[i] = slot[i] + slot[i ^ (1 << L)];
    for (int i = 0; i < AIE_OPT_SLOTS; ++i) slot[i] = next[i];
  }
  return slot[0];
}
typedef struct aie_opt_step {
  float coef, step, b2s;                 /* the float64 scalars, rounded once */
  float beta1, beta2, omb1, omb2, eps;   /* omb = 1 - beta in float32 */
  float norm;                            /* stats[0] */
  int32_t skipped;
  aie_opt_state next;                    /* the state after the call (the old one for a skipped group) */
} aie_opt_step;
AIE_HD static inline aie_opt_step aie_opt_scalars(double n2, float max_norm, float beta1, float beta2, float eps, float lr,
                                                  aie_opt_state old) {
  AIE_NOCONTRACT
  aie_opt_step S;
  const double norm = sqrt(n2);
  const double sum = norm + 1e-6;
  const double ratio = (double)max_norm / sum;
  const double coef = max_norm > 0.0f ? (ratio < 1.0 ? ratio : 1.0) : 1.0;
  S.skipped = !aie_opt_finite(n2);
  S.norm = (float)norm;
  S.next = old;
  double p1 = old.t == 0 ? 1.0 : old.p1, p2 = old.t == 0 ? 1.0 : old.p2;
  p1 = p1 * (double)beta1;
  p2 = p2 * (double)beta2;
  if (!S.skipped) S.next.t = old.t + 1, S.next.p1 = p1, S.next.p2 = p2;
  const double c1 = 1.0 - p1, c2 = 1.0 - p2;
  S.coef = S.skipped ? 0.0f : (float)coef;
  S.step = (float)((double)lr / c1);
  S.b2s = (float)sqrt(c2);
  S.beta1 = beta1, S.beta2 = beta2, S.eps = eps;
  S.omb1 = 1.0f - beta1;
  S.omb2 = 1.0f - beta2;
  return S;
}
AIE_HD static inline void aie_opt_element(const aie_opt_step* S, float g, float* w, float* m, float* v) {
  AIE_NOCONTRACT
  const float gc = g * S->coef;
  const float bm = S->beta1 * *m;
  const float mn = fmaf(S->omb1, gc, bm);
  const float bv = S->beta2 * *v;
  const float og = S->omb2 * gc;
  const float vn = fmaf(og, gc, bv);
  const float rt = sqrtf(vn);
  const float q = AIE_FDIV_RN(rt, S->b2s);
  const float d = q + S->eps;
  const float u = AIE_FDIV_RN(mn, d);
  *w = fmaf(-S->step, u, *w);
  *m = mn;
  *v = vn;
}
AIE_HD static inline void aie_opt_stats(const aie_opt_step* S, float* stats) {
  stats[0] = S->norm;
  stats[1] = S->coef;
  stats[2] = (float)S->next.t;
  stats[3] = S->skipped ? 1.0f : 0.0f;
}
/* The whole step of one group on the host: every pointer of the descriptor is host memory here. */
static inline void aie_adam_group_host(const aie_opt_group* G) {
  double n2 = 0.0;
  for (int i = 0; i < G->n_tensors; ++i)
    for (int64_t e = 0; e < G->tensors[i].n; e += AIE_OPT_CHUNK) {
      const int64_t left = G->tensors[i].n - e;
      n2 += aie_opt_chunk_sumsq(G->tensors[i].g + e, left < AIE_OPT_CHUNK ? left : AIE_OPT_CHUNK);
    }
  aie_opt_state* st = (aie_opt_state*)G->d_state;
  const aie_opt_step S = aie_opt_scalars(n2, G->max_norm, G->beta1, G->beta2, G->eps, *G->d_lr, *st);
  aie_opt_stats(&S, G->d_stats);
  if (S.skipped) return;
  *st = S.next;
  for (int i = 0; i < G->n_tensors; ++i) {
    const aie_opt_tensor* T = &G->tensors[i];
    for (int64_t e = 0; e < T->n; ++e) aie_opt_element(&S, T->g[e], T->w + e, T->m + e, T->v + e);
  }
}
/* The kernels' argument (aie_adam_step fills it: aie_plan_adam).  Workgroup b of either launch owns one chunk: b <
 * grp[0].chunks the agents' group's chunk b, else the planner's chunk b - grp[0].chunks; a group's chunk c belongs to the last
 * tensor i with t[i].first <= c and is that tensor's chunk c - t[i].first.  wide != 0: w, g, m and v are all 16-byte
 * aligned (16-byte lane accesses on whole quads), else 4-byte ones.  ws: the group's share of the workspace, 4 float64
 * words for the state's copy {t, p1, p2, 0}, then one float64 per chunk. */
typedef struct aie_opt_tensor_k {
  float* w;
  const float* g;
  float *m, *v;
  int64_t n;
  int32_t first, wide;
} aie_opt_tensor_k;
typedef struct aie_opt_group_k {
  aie_opt_tensor_k t[AIE_OPT_MAX_TENSORS];
  const float* lr;
  aie_opt_state* state;
  float* stats;
  double* ws;
  float beta1, beta2, eps, max_norm;
  int32_t n_tensors, chunks;   /* chunks 0: the group is left out */
} aie_opt_group_k;
typedef struct aie_adam_args {
  aie_opt_group_k grp[2];
} aie_adam_args;
#define AIE_OPT_WS_HEAD 4 /* float64 words ahead of a group's chunk sums */
/* aie_trajectory_store's kernel argument: the caller's segments (include/aie.h: aie_traj_segment, 32 bytes each) with the
 * copy width decided on the host: wide != 0 = 16-byte lane accesses (source, destination, stride and size allow it for
 * every replica and slot), else 4-byte ones. */
#define AIE_TRAJ_SEGMENTS 16
typedef struct aie_traj_seg_k {
  const uint8_t* src;
  uint8_t* dst;
  int64_t src_stride;
  int32_t bytes;
  int16_t rows, wide;
} aie_traj_seg_k;
typedef struct aie_traj_args {
  aie_traj_seg_k seg[AIE_TRAJ_SEGMENTS];
  int32_t* slot;
  int32_t n_segs, n_slots, E, pad_;
} aie_traj_args;
/* What the sampler kernel needs of the parameter block, as its kernel argument (aie_sampler_args_of fills it).  A group
 * is a replica's agent rows or its planner rows: row r's entry k has its logit at logits[e lg_estride + r lrs + k] and its
 * mask at the arena's float mk_off / 4 + e mk_estride + r mrs + k mks (COVID's collated agent masks: mrs 1, mks n). */
typedef struct aie_sampler_group {
  int64_t mk_off;
  uint32_t mk_estride, lg_estride;       /* (32 bits: a replica's rows x entries) */
  int32_t len, lrs, mrs, mks, lsh, rows; /* entries per row; strides; log2 of the lanes a row takes; rows per replica */
} aie_sampler_group;
typedef struct aie_sampler_args {
  aie_sampler_group agents, planner;
  int64_t t_off, rec_bytes;   /* replica e's draw index: the arena's int32 at t_off + e rec_bytes */
  const aie_params* params;   /* the device copy: read for multi-action agents only (rows of different lengths) */
  int32_t E, ragged, act_a_width, pad_;
} aie_sampler_args;
/* The samplers' planner group is rows of ONE length.  A multi-action planner with a foreign row (aie_config.host_p_*) of
 * another length than the tax rows' is refused (the choice stated in include/aie.h): 0 = fine, else the message is in err. */
static inline int aie_sampler_check(const aie_params* p, char* err, size_t errlen) {
  if (p->c.multi_action_mode_planner && p->n_host_p && !p->p_rows_uniform) {
    if (err) snprintf(err, errlen, "samplers: a multi-action planner whose foreign action subspaces differ in size from its other "
                      "rows (%d entries) is not supported: sample the planner's actions on the host", 1 + p->p_row_dim);
    return AIE_E_UNSUPPORTED;
  }
  return AIE_OK;
}
static inline aie_sampler_args aie_sampler_args_of(const aie_params* p, const aie_params* d_params) {
  aie_sampler_args S;
  memset(&S, 0, sizeof(S));
  const int covid = p->c.scenario == AIE_SCN_COVID;
  const int wa = covid ? 1 + p->cv_NL : p->MA; /* logits per agent, in the mask's own (flattened) layout */
  aie_sampler_group* A = &S.agents;
  aie_sampler_group* Q = &S.planner;
  S.ragged = p->c.multi_action_mode_agents != 0;
  A->len = wa;
  A->lsh = S.ragged ? 6 : (aie_sampler_segment(wa) == 16 ? 4 : aie_sampler_segment(wa) == 32 ? 5 : 6);
  A->rows = p->n * p->act_a_width;
  A->lrs = wa;
  A->lg_estride = (uint32_t)(p->n * wa);
  if (covid) {
    A->mk_off = p->a_cv_obs_a + 4 * (int64_t)AIE_CV_OB_MASK * p->n;
    A->mk_estride = (uint32_t)(p->cv_nrow_obs * p->n);
    A->mks = p->n;
    A->mrs = 1;
  } else {
    A->mk_off = p->a_obs_a_mask;
    A->mk_estride = (uint32_t)(p->n * p->MA);
    A->mks = 1;
    A->mrs = p->MA;
  }
  /* a multi-action planner's rows are 1 + p_row_dim entries each (the tax brackets' 1 + sub_p_dim without foreign rows);
   * rows of different lengths (p_rows_uniform == 0) do not reach this function: aie_sampler_check refuses them */
  Q->len = p->c.multi_action_mode_planner ? 1 + p->p_row_dim : p->MP;
  Q->lsh = aie_sampler_segment(Q->len) == 16 ? 4 : aie_sampler_segment(Q->len) == 32 ? 5 : 6;
  Q->rows = p->act_p_width;
  Q->lrs = Q->mrs = p->c.multi_action_mode_planner ? 1 + p->p_row_dim : p->MP; /* (a multi-action planner's rows: 1 + p_row_dim apart) */
  Q->mks = 1;
  Q->lg_estride = (uint32_t)p->MP;
  Q->mk_off = covid ? p->a_cv_obs_p + 16 : p->a_obs_p_mask;
  Q->mk_estride = (uint32_t)(covid ? 4 + p->MP : p->MP);
  S.t_off = p->a_records + p->o_sample_t;
  S.rec_bytes = p->rec_bytes;
  S.params = d_params;
  S.E = p->E;
  S.act_a_width = p->act_a_width;
  return S;
}

#if defined(__HIPCC__)
#pragma clang fp contract(off) /* the library's mode again */
#endif

#endif /* AIE_TRAINER_MATH_H_ */
