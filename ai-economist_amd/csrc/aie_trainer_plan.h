/* The trainer calls' host plans (include/aie.h: aie_policy_evaluate .. aie_trajectory_store): the operand checks, the kernel
 * argument, grid, block and LDS sizes, the workspace's size and carve-up -- each a pure function of the parameter block and
 * the caller's pointers, in plain C like aie_sampler_args_of.  No HIP types and no aie_env: aie_capi.hip's entry points
 * call a plan, then launch what it says; tests/test_trainer_plan_cpu.py compiles this file with the host compiler.
 * Nothing here dereferences an operand.  err: where a refusal names itself (NULL: nowhere).  A plan whose grid is 0 has
 * nothing to launch (no class asked for): the call returns AIE_OK. */
#ifndef AIE_TRAINER_PLAN_H_
#define AIE_TRAINER_PLAN_H_

#include "aie.h"
#include "aie_trainer_math.h"

#if AIE_TRAJ_SEGMENTS != AIE_TRAJ_MAX_SEGMENTS
#error "aie_trainer_math.h and aie.h disagree on the segment count"
#endif
#if AIE_MLP_TILE_ROWS != 32 && AIE_MLP_TILE_ROWS != 64
#error "the MLP kernels' row tile is 2 or 4 MFMA tiles"
#endif

#define AIE_PLAN_REFUSE(code, ...) \
  do { if (err) snprintf(err, errlen, __VA_ARGS__); return (code); } while (0)
#define AIE_PLAN_GRID_MAX 0x7fffff00ll /* workgroups (or wavefronts) one launch takes */

/* ---- aie_policy_evaluate / aie_policy_evaluate_backward ---- */
typedef struct aie_eval_plan { aie_policy_eval_args A; uint32_t grid, block; } aie_eval_plan;

/* The rows' shape of B batch elements: the sampler's (aie_sampler_args_of) with the caller's logits and masks.  A class whose
 * logits are NULL is left out (items 0).  aie_ppo_loss plans on top of it. */
static inline int aie_plan_eval_rows(const aie_params* P, const aie_params* d_params, const uint8_t* arena, const char* who,
                                     int64_t B, const float* lg_a, const float* lg_p, const float* mk_a, const float* mk_p,
                                     char* err, size_t errlen, aie_policy_eval_args* out) {
  if (aie_sampler_check(P, err, errlen) != AIE_OK) return AIE_E_UNSUPPORTED;
  if (B < 1 || (((lg_a && !mk_a) || (lg_p && !mk_p)) && B != P->E))
    AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: B = %lld; without the caller's masks (the arena's current ones) B must be the "
                    "environment's %d replicas", who, (long long)B, P->E);
  const aie_sampler_args S = aie_sampler_args_of(P, d_params);
  aie_policy_eval_args A;
  memset(&A, 0, sizeof(A));
  const aie_sampler_group* sg[2] = {&S.agents, &S.planner};
  aie_policy_eval_group* eg[2] = {&A.agents, &A.planner};
  const float* lg[2] = {lg_a, lg_p};
  const float* mk[2] = {mk_a, mk_p};
  for (int c = 0; c < 2; ++c) {
    aie_policy_eval_group* G = eg[c];
    const aie_sampler_group* s = sg[c];
    G->lg = lg[c], G->lg_bstride = s->lg_estride;
    G->len = s->len, G->lrs = s->lrs, G->lsh = s->lsh, G->rows = s->rows;
    G->generic = (c == 0 && S.ragged) || s->len > 64;
    if (mk[c]) { /* the caller's masks: the logits' layout */
      G->mk = mk[c];
      G->mk_bstride = s->lg_estride, G->mrs = s->lrs, G->mks = 1;
    } else {     /* the arena's current masks */
      G->mk = (const float*)((uintptr_t)arena + (uintptr_t)s->mk_off);
      G->mk_bstride = s->mk_estride, G->mrs = s->mrs, G->mks = s->mks;
    }
    const int rpw = G->generic ? 1 : 64 >> s->lsh;
    G->items = lg[c] ? (s->rows + rpw - 1) / rpw : 0;
  }
  A.params = d_params, A.B = (uint32_t)B, A.items = (uint32_t)(A.agents.items + A.planner.items);
  A.act_a_width = S.act_a_width, A.ragged = S.ragged;
  if (A.items && B * (int64_t)A.items > AIE_PLAN_GRID_MAX)
    AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: B = %lld is more than one launch takes (%u wavefronts per batch element)", who,
                    (long long)B, A.items);
  *out = A;
  return AIE_OK;
}

static inline int aie_plan_policy_evaluate(const aie_params* P, const aie_params* d_params, const uint8_t* arena, int64_t B,
                                           const float* d_logits_a, const float* d_logits_p, const float* d_masks_a,
                                           const float* d_masks_p, const int32_t* d_actions_a, const int32_t* d_actions_p,
                                           float* d_logp_a, float* d_logp_p, float* d_entropy_a, float* d_entropy_p, char* err,
                                           size_t errlen, aie_eval_plan* p) {
  memset(p, 0, sizeof(*p));
  if ((d_logp_a && !(d_logits_a && d_actions_a)) || (d_logp_p && !(d_logits_p && d_actions_p)) || (d_entropy_a && !d_logits_a) ||
      (d_entropy_p && !d_logits_p))
    AIE_PLAN_REFUSE(AIE_E_INVALID, "aie_policy_evaluate: an output without its logits (logp: and its stored actions)");
  /* (an actor class none of whose outputs is asked for is left out of the launch) */
  const int rc = aie_plan_eval_rows(P, d_params, arena, "aie_policy_evaluate", B, (d_logp_a || d_entropy_a) ? d_logits_a : NULL,
                                    (d_logp_p || d_entropy_p) ? d_logits_p : NULL, d_masks_a, d_masks_p, err, errlen, &p->A);
  if (rc != AIE_OK || !p->A.items) return rc;
  p->A.agents.act = d_actions_a, p->A.planner.act = d_actions_p;
  p->A.agents.logp = d_logp_a, p->A.planner.logp = d_logp_p;
  p->A.agents.ent = d_entropy_a, p->A.planner.ent = d_entropy_p;
  p->grid = (uint32_t)((B * (int64_t)p->A.items + 3) / 4), p->block = 256; /* an item a wavefront, four a workgroup */
  return AIE_OK;
}

static inline int aie_plan_policy_evaluate_backward(const aie_params* P, const aie_params* d_params, const uint8_t* arena,
                                                    int64_t B, const float* d_logits_a, const float* d_logits_p,
                                                    const float* d_masks_a, const float* d_masks_p, const int32_t* d_actions_a,
                                                    const int32_t* d_actions_p, const float* d_glogp_a, const float* d_glogp_p,
                                                    const float* d_gentropy_a, const float* d_gentropy_p, float* d_grad_logits_a,
                                                    float* d_grad_logits_p, char* err, size_t errlen, aie_eval_plan* p) {
  memset(p, 0, sizeof(*p));
  if ((d_grad_logits_a && !d_logits_a) || (d_grad_logits_p && !d_logits_p) || (d_glogp_a && !d_actions_a) ||
      (d_glogp_p && !d_actions_p))
    AIE_PLAN_REFUSE(AIE_E_INVALID, "aie_policy_evaluate_backward: a gradient buffer without its logits, or a logp gradient "
                    "without the stored actions");
  const int rc = aie_plan_eval_rows(P, d_params, arena, "aie_policy_evaluate_backward", B, d_grad_logits_a ? d_logits_a : NULL,
                                    d_grad_logits_p ? d_logits_p : NULL, d_masks_a, d_masks_p, err, errlen, &p->A);
  if (rc != AIE_OK || !p->A.items) return rc;
  p->A.agents.act = d_actions_a, p->A.planner.act = d_actions_p;
  p->A.agents.g_logp = d_glogp_a, p->A.planner.g_logp = d_glogp_p;
  p->A.agents.g_ent = d_gentropy_a, p->A.planner.g_ent = d_gentropy_p;
  p->A.agents.grad = d_grad_logits_a, p->A.planner.grad = d_grad_logits_p;
  p->grid = (uint32_t)((B * (int64_t)p->A.items + 3) / 4), p->block = 256; /* an item a wavefront, four a workgroup */
  return AIE_OK;
}

/* ---- aie_gae: a lane per float of a log row, wavefront-sized workgroups ---- */
typedef struct aie_gae_plan { aie_gae_args A; uint32_t grid, block; } aie_gae_plan;

static inline int aie_plan_gae(const aie_params* P, int32_t T, const float* d_log, int32_t n_slots, int32_t first_slot,
                               const float* d_values_a, const float* d_values_p, float gamma, float lambda, float* d_adv_a,
                               float* d_adv_p, float* d_ret_a, float* d_ret_p, char* err, size_t errlen, aie_gae_plan* p) {
  memset(p, 0, sizeof(*p));
  if (T < 1 || T > n_slots || first_slot < 0 || first_slot >= n_slots || !d_log)
    AIE_PLAN_REFUSE(AIE_E_INVALID, "aie_gae: T = %d steps from slot %d of a log of %d slots at %p (needs a log, 1 <= T <= "
                    "n_slots, 0 <= first_slot < n_slots)", T, first_slot, n_slots, (const void*)d_log);
  if (((d_adv_a || d_ret_a) && !d_values_a) || ((d_adv_p || d_ret_p) && !d_values_p))
    AIE_PLAN_REFUSE(AIE_E_INVALID, "aie_gae: an output without its values");
  const int64_t row = (int64_t)P->E * (P->n + 2);
  if (row > AIE_PLAN_GRID_MAX)
    AIE_PLAN_REFUSE(AIE_E_INVALID, "aie_gae: %lld floats per log row are more than one launch takes", (long long)row);
  aie_gae_args* A = &p->A;
  A->log = d_log;
  /* (an actor class none of whose outputs is asked for is left out of the launch) */
  A->va = (d_adv_a || d_ret_a) ? d_values_a : NULL;
  A->vp = (d_adv_p || d_ret_p) ? d_values_p : NULL;
  if (!A->va && !A->vp) return AIE_OK;
  A->adv_a = d_adv_a, A->adv_p = d_adv_p, A->ret_a = d_ret_a, A->ret_p = d_ret_p;
  A->T = T, A->slots = n_slots, A->first = first_slot, A->E = P->E, A->n = P->n;
  A->gamma = gamma, A->gl = aie_gae_gl(gamma, lambda);
  p->grid = (uint32_t)((row + 63) / 64), p->block = 64;
  return AIE_OK;
}

/* ---- aie_ppo_loss: `waves` wavefronts stride over B x items work items and leave a record each; one workgroup adds them ---- */
typedef struct aie_ppo_plan {
  aie_ppo_args A; uint32_t grid, block, reduce_grid, reduce_block; int64_t need; /* need: workspace bytes of this call */
} aie_ppo_plan;

static inline uint32_t aie_plan_ppo_waves(int64_t work) { return (uint32_t)(work < AIE_PPO_MAX_WAVES ? work : AIE_PPO_MAX_WAVES); }
/* what aie_ppo_workspace_bytes returns: an upper bound that knows no classes (at most one work item per actor: n agents and
 * the planner) */
static inline int64_t aie_plan_ppo_workspace_bytes(const aie_params* P, int64_t B) {
  if (B < 1) return AIE_E_INVALID;
  const int64_t per = (int64_t)P->n + 1;
  const int64_t work = B > AIE_PPO_MAX_WAVES / per ? (int64_t)AIE_PPO_MAX_WAVES : B * per;
  return (int64_t)aie_plan_ppo_waves(work) * AIE_PPO_RECORD * (int64_t)sizeof(double);
}

static inline int aie_plan_ppo_loss(const aie_params* P, const aie_params* d_params, const uint8_t* arena, int64_t B,
                                    const aie_ppo_class* agents, const aie_ppo_class* planner, const int32_t* d_index,
                                    void* d_workspace, char* err, size_t errlen, aie_ppo_plan* p) {
  memset(p, 0, sizeof(*p));
  const aie_ppo_class* cls[2] = {agents, planner};
  for (int c = 0; c < 2; ++c) {
    const aie_ppo_class* k = cls[c];
    if (!k) continue;
    if (!k->logits || !k->masks || !k->actions || !k->logp_old || !k->adv || !k->grad_logits || !k->stats ||
        (k->values && (!k->values_old || !k->returns || !k->grad_values)) || (!k->values && k->grad_values) || !(k->clip > 0.0f))
      AIE_PLAN_REFUSE(AIE_E_INVALID, "aie_ppo_loss: the %s class needs logits, masks, actions, logp_old, adv, grad_logits and "
                      "stats, with values also values_old, returns and grad_values (and no grad_values without), and clip > 0 (%g)",
                      c ? "planner's" : "agents'", (double)k->clip);
  }
  /* the rows' shape is the evaluator's (B < 1 and the samplers' refusals are its own) */
  aie_policy_eval_args E;
  const int rc = aie_plan_eval_rows(P, d_params, arena, "aie_ppo_loss", B, agents ? agents->logits : NULL,
                                    planner ? planner->logits : NULL, agents ? agents->masks : NULL,
                                    planner ? planner->masks : NULL, err, errlen, &E);
  if (rc != AIE_OK || !E.items) return rc;
  aie_ppo_args* A = &p->A;
  const aie_policy_eval_group* eg[2] = {&E.agents, &E.planner};
  aie_ppo_group* pg[2] = {&A->agents, &A->planner};
  const int width[2] = {P->act_a_width, P->act_p_width};
  for (int c = 0; c < 2; ++c) {
    const aie_ppo_class* k = cls[c];
    if (!k) continue;
    const aie_policy_eval_group* e = eg[c];
    aie_ppo_group* G = pg[c];
    G->lg = k->logits, G->val = k->values;                          /* the network's outputs */
    G->mk = k->masks, G->act = k->actions, G->lp_old = k->logp_old;   /* the stored operands */
    G->adv = k->adv, G->mom = k->adv_moments, G->val_old = k->values_old, G->ret = k->returns;
    G->grad = k->grad_logits, G->grad_v = k->grad_values, G->stats = k->stats;
    G->lg_bstride = e->lg_bstride, G->len = e->len, G->lrs = e->lrs, G->lsh = e->lsh, G->rows = e->rows; /* the evaluator's rows */
    G->w = width[c] > 0 ? width[c] : 1;
    G->actors = e->rows / G->w;
    if (G->w > 64 || G->actors * G->w != e->rows)
      AIE_PLAN_REFUSE(AIE_E_UNSUPPORTED, "aie_ppo_loss: %d action slots per actor (%d rows) are more than a wavefront holds",
                      G->w, e->rows);
    G->generic = e->generic || G->w > 1;
    const int rpw = G->generic ? 1 : 64 >> e->lsh;
    G->items = G->generic ? G->actors : (e->rows + rpw - 1) / rpw;
    G->clip = k->clip, G->vf_clip = k->vf_clip, G->vf_coef = k->vf_coef, G->ent_coef = k->ent_coef;
    G->scale = aie_ppo_scale(B * (int64_t)G->actors);
    G->g_H = -aie_ppo_product(G->scale, k->ent_coef);
    G->kv = aie_ppo_product(G->scale, k->vf_coef);
  }
  A->params = d_params, A->index = d_index, A->ws = (double*)d_workspace;
  A->B = (uint32_t)B, A->items = (uint32_t)(A->agents.items + A->planner.items);
  A->act_a_width = E.act_a_width, A->ragged = E.ragged;
  const int64_t work = B * (int64_t)A->items;
  if (work > AIE_PLAN_GRID_MAX)
    AIE_PLAN_REFUSE(AIE_E_INVALID, "aie_ppo_loss: B = %lld is more than one call takes (%u work items per batch element)",
                    (long long)B, A->items);
  /* (the whole bound, although 89 registers leave only 5120 wavefronts resident at once: sized to residency the kernel took
   * 2.4 x as long on a fragment of 819 200 rows -- DESIGN_HISTORY.md, item 10 -- it lives on loads in flight, not on rounds) */
  A->waves = aie_plan_ppo_waves(work);
  p->need = (int64_t)A->waves * AIE_PPO_RECORD * (int64_t)sizeof(double);
  p->grid = (A->waves + 3u) / 4u, p->block = 256, p->reduce_grid = 1, p->reduce_block = 1024;
  return AIE_OK;
}

/* ---- the policy MLP, forward and backward ---- */
/* ONE class of either pass: the checks of its aie_mlp_class and the fill of its aie_mlp_group, so that the backward's
 * recomputed h1 and h2 see the forward's geometry.  q NULL: the forward (logits and values are operands); else the backward
 * (net.logits / net.values ignored, the gradient pointers checked where the backward checks them: ahead of the hidden width). */
static inline int aie_plan_mlp_class(const char* fn, const aie_params* P, int64_t B, int c, const aie_mlp_class* k,
                                     const aie_mlp_grad_class* q, char* err, size_t errlen, aie_mlp_group* G) {
  const char* who = c ? "planner's" : "agents'";
  const int v = k->wv != NULL;
  if (k->F < 1 || k->F > 1024 || k->M < 1 || k->M > 1024 || k->x_ld < k->F || !k->x || !k->w1 || !k->b1 || !k->w2 || !k->b2 ||
      !k->w3 || !k->b3 || v != (k->bv != NULL) || (!q && (!k->logits || v != (k->values != NULL))))
    AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: the %s class needs F (%d) and M (%d) in 1 .. 1024, x_ld (%lld) >= F, x, w1, b1, w2, b2, w3%s",
                    fn, who, k->F, k->M, (long long)k->x_ld,
                    q ? " and b3, and wv and bv both or neither" : ", b3 and logits, and wv, bv and values all three or none");
  if (q && (!q->g_logits || !q->gw1 || !q->gb1 || !q->gw2 || !q->gb2 || !q->gw3 || !q->gb3 || v != (q->g_values != NULL) ||
            v != (q->gwv != NULL) || v != (q->gbv != NULL)))
    AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: the %s class needs g_logits, gw1, gb1, gw2, gb2, gw3 and gb3, and g_values, gwv and gbv "
                    "exactly when it has wv", fn, who);
  if (k->H < 16 || k->H > 256 || (k->H & 15))
    AIE_PLAN_REFUSE(AIE_E_UNSUPPORTED, "%s: the %s hidden width %d is not a multiple of 16 in 16 .. 256", fn, who, k->H);
  G->x = k->x, G->x_ld = k->x_ld;
  G->w1 = k->w1, G->b1 = k->b1, G->w2 = k->w2, G->b2 = k->b2, G->w3 = k->w3, G->b3 = k->b3, G->wv = k->wv, G->bv = k->bv;
  if (!q) G->logits = k->logits, G->values = k->values;
  G->F = k->F, G->H = k->H, G->M = k->M;
  G->rows = c ? B : B * (int64_t)P->n;
  const int kpad = (k->F + 3) & ~3, chunk = kpad < AIE_MLP_CHUNK ? kpad : AIE_MLP_CHUNK;
  G->lds_a = (chunk > k->H ? chunk : k->H) + 2;
  G->lds_h = k->H + 2;
  const int64_t nb = (G->rows + AIE_MLP_TILE_ROWS - 1) / AIE_MLP_TILE_ROWS;
  if (nb > 0x3fffffffll) AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: B = %lld is more than one call takes", fn, (long long)B);
  G->blocks = (int32_t)nb;
  return AIE_OK;
}

typedef struct aie_mlp_fwd_plan { aie_mlp_args A; uint32_t grid, block; size_t lds; } aie_mlp_fwd_plan;

static inline int aie_plan_mlp_forward(const aie_params* P, int64_t B, const aie_mlp_class* agents, const aie_mlp_class* planner,
                                       char* err, size_t errlen, aie_mlp_fwd_plan* p) {
  const char* fn = "aie_policy_mlp_forward";
  memset(p, 0, sizeof(*p));
  if (B < 1) AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: B = %lld (needs B >= 1)", fn, (long long)B);
  const aie_mlp_class* cls[2] = {agents, planner};
  aie_mlp_group* grp[2] = {&p->A.agents, &p->A.planner};
  int64_t blocks = 0;
  for (int c = 0; c < 2; ++c) {
    if (!cls[c]) continue;
    const aie_mlp_group* G = grp[c];
    const int rc = aie_plan_mlp_class(fn, P, B, c, cls[c], NULL, err, errlen, grp[c]);
    if (rc != AIE_OK) return rc;
    blocks += G->blocks;
    const size_t need = (size_t)AIE_MLP_TILE_ROWS * (size_t)(G->lds_a + G->lds_h) * sizeof(float);
    p->lds = need > p->lds ? need : p->lds;
  }
  if (blocks > AIE_PLAN_GRID_MAX)
    AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: B = %lld is more than one launch takes (%lld workgroups)", fn, (long long)B, (long long)blocks);
  p->grid = (uint32_t)blocks, p->block = 256;
  return AIE_OK;
}

/* The backward in two steps (the workspace-bytes query stops after the first): aie_plan_mlp_backward checks the classes, fills
 * the kernels' argument without the workspace pointers and sizes each class's share; aie_plan_mlp_backward_launch carves the
 * caller's workspace and sizes the three launches (row tiles; items; the reduction of P entries per class, 256 a workgroup). */
typedef struct aie_mlp_bwd_plan {
  aie_mlp_bwd_args A;
  int64_t ws_floats[2], need; /* each class's share, a multiple of 64 floats; workspace bytes of this call */
  uint32_t grid_rows, grid_atd, grid_reduce, block;
  size_t lds;                 /* of the first launch */
} aie_mlp_bwd_plan;

static inline int aie_plan_mlp_backward(const aie_params* P, int64_t B, const aie_mlp_grad_class* agents,
                                        const aie_mlp_grad_class* planner, char* err, size_t errlen, aie_mlp_bwd_plan* p) {
  const char* fn = "aie_policy_mlp_backward";
  memset(p, 0, sizeof(*p));
  if (B < 1) AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: B = %lld (needs B >= 1)", fn, (long long)B);
  const aie_mlp_grad_class* cls[2] = {agents, planner};
  aie_mlp_bwd_group* grp[2] = {&p->A.agents, &p->A.planner};
  for (int c = 0; c < 2; ++c) {
    const aie_mlp_grad_class* q = cls[c];
    if (!q) continue;
    const aie_mlp_class* k = &q->net;
    aie_mlp_bwd_group* Q = grp[c];
    const int rc = aie_plan_mlp_class(fn, P, B, c, k, q, err, errlen, &Q->net);
    if (rc != AIE_OK) return rc;
    const int mpad = (k->M + 3) & ~3;
    Q->lds_c = (mpad < AIE_MLP_CHUNK ? mpad : AIE_MLP_CHUNK) + 2;
    const int64_t nseg = (Q->net.rows + AIE_MLP_BWD_SEG - 1) / AIE_MLP_BWD_SEG;
    Q->nseg = (int32_t)nseg;
    Q->g_logits = q->g_logits, Q->g_values = q->g_values;
    Q->gw1 = q->gw1, Q->gb1 = q->gb1, Q->gw2 = q->gw2, Q->gb2 = q->gb2;
    Q->gw3 = q->gw3, Q->gb3 = q->gb3, Q->gwv = q->gwv, Q->gbv = q->gbv;
    Q->N3 = k->M + (k->wv ? 1 : 0);
    Q->off2 = (k->F + 1) * k->H;
    Q->off3 = Q->off2 + (k->H + 1) * k->H;
    Q->P = Q->off3 + (k->H + 1) * Q->N3;
    const int Ks[3] = {k->F, k->H, k->H}, Ns[3] = {k->H, k->H, Q->N3};
    for (int L = 0; L < 3; ++L) {
      Q->cg[L] = (((Ns[L] + 15) >> 4) + 3) >> 2;
      Q->items[L] = ((((Ks[L] + 1 + 15) >> 4) + 3) >> 2) * Q->cg[L]; /* groups of four bands x column groups */
      Q->per_seg += Q->items[L];
    }
    Q->n_items = nseg * Q->per_seg;
    const int64_t fl = 4 * Q->net.rows * k->H + nseg * Q->P;
    p->ws_floats[c] = (fl + 63) & ~(int64_t)63;
  }
  p->need = (p->ws_floats[0] + p->ws_floats[1]) * (int64_t)sizeof(float);
  return AIE_OK;
}

static inline int aie_plan_mlp_backward_launch(aie_mlp_bwd_plan* p, int64_t B, const aie_mlp_grad_class* agents,
                                               const aie_mlp_grad_class* planner, void* d_workspace, char* err, size_t errlen) {
  const aie_mlp_grad_class* cls[2] = {agents, planner};
  aie_mlp_bwd_group* grp[2] = {&p->A.agents, &p->A.planner};
  float* ws = (float*)d_workspace;
  int64_t blocks = 0, items = 0, rblocks = 0;
  for (int c = 0; c < 2; ++c) {
    aie_mlp_bwd_group* Q = grp[c];
    if (!cls[c]) continue;
    const int64_t rh = Q->net.rows * Q->net.H;
    Q->h1 = ws, Q->h2 = ws + rh, Q->dz2 = ws + 2 * rh, Q->dz1 = ws + 3 * rh, Q->partial = ws + 4 * rh;
    ws += p->ws_floats[c];
    blocks += Q->net.blocks;
    items += Q->n_items;
    const int64_t rb = (Q->P + 255) / 256;
    if (!c) p->A.reduce_blocks_a = (int32_t)rb;
    rblocks += rb;
    const size_t l = (size_t)AIE_MLP_TILE_ROWS * (size_t)(Q->net.lds_a + Q->net.lds_h + Q->lds_c) * sizeof(float);
    p->lds = l > p->lds ? l : p->lds;
  }
  if (blocks > AIE_PLAN_GRID_MAX || items > AIE_PLAN_GRID_MAX)
    AIE_PLAN_REFUSE(AIE_E_INVALID, "aie_policy_mlp_backward: B = %lld is more than one call takes", (long long)B);
  p->grid_rows = (uint32_t)blocks, p->grid_atd = (uint32_t)items, p->grid_reduce = (uint32_t)rblocks, p->block = 256;
  return AIE_OK;
}

/* ---- aie_policy_mlp_input_grad: the backward's own plan finds dz1 in the workspace; a workgroup per AIE_IGRAD_TILE rows and
 * 256 columns ---- */
typedef struct aie_mlp_igrad_plan { aie_mlp_igrad_args A; int64_t need; uint32_t grid, block; size_t lds; } aie_mlp_igrad_plan;

static inline int aie_plan_mlp_input_grad(const aie_params* P, int64_t B, const aie_mlp_grad_class* agents,
                                          const aie_mlp_grad_class* planner, void* d_workspace, int64_t workspace_bytes,
                                          float* g_x_a, int64_t ld_a, int32_t ncols_a, float* g_x_p, int64_t ld_p, int32_t ncols_p, char* err, size_t errlen,
                                          aie_mlp_igrad_plan* p) {
  const char* fn = "aie_policy_mlp_input_grad";
  memset(p, 0, sizeof(*p));
  aie_mlp_bwd_plan b;
  int rc = aie_plan_mlp_backward(P, B, agents, planner, err, errlen, &b);
  if (rc != AIE_OK) return rc;
  const aie_mlp_grad_class* cls[2] = {agents, planner};
  float* gx[2] = {g_x_a, g_x_p};
  const int64_t ld[2] = {ld_a, ld_p};
  const int32_t nc[2] = {ncols_a, ncols_p};
  for (int c = 0; c < 2; ++c) {
    if (!gx[c]) continue;
    if (!cls[c] || nc[c] < 1 || nc[c] > cls[c]->net.F || ld[c] < nc[c] || ((uintptr_t)gx[c] & 3))
      AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: the %s g_x (%p, ld %lld, ncols %d) needs its class, 1 <= ncols <= F, ld >= ncols and a "
                      "4-byte aligned pointer", fn, c ? "planner's" : "agents'", (void*)gx[c], (long long)ld[c], nc[c]);
  }
  p->need = b.need;
  if (!agents && !planner) return AIE_OK;
  if (!d_workspace || ((uintptr_t)d_workspace & 15) || workspace_bytes < b.need)
    AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: the workspace (%p, %lld bytes) must be aie_policy_mlp_backward's: device memory, 16-byte "
                    "aligned, of at least %lld bytes", fn, d_workspace, (long long)workspace_bytes, (long long)b.need);
  rc = aie_plan_mlp_backward_launch(&b, B, agents, planner, d_workspace, err, errlen);
  if (rc != AIE_OK) return rc;
  const aie_mlp_bwd_group* bg[2] = {&b.A.agents, &b.A.planner};
  aie_mlp_igrad_group* ig[2] = {&p->A.agents, &p->A.planner};
  int64_t blocks = 0;
  for (int c = 0; c < 2; ++c) {
    if (!gx[c]) continue;
    aie_mlp_igrad_group* G = ig[c];
    G->dz1 = bg[c]->dz1, G->w1 = bg[c]->net.w1, G->g_x = gx[c], G->ld = ld[c], G->rows = bg[c]->net.rows;
    G->H = bg[c]->net.H, G->ncols = nc[c];
    const int64_t tiles = (G->rows + AIE_IGRAD_TILE - 1) / AIE_IGRAD_TILE;
    G->cgroups = (nc[c] + 255) / 256;
    if (tiles * G->cgroups > AIE_PLAN_GRID_MAX) AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: B = %lld is more than one launch takes", fn, (long long)B);
    G->tiles = (int32_t)tiles, G->blocks = (int32_t)(tiles * G->cgroups);
    blocks += G->blocks;
    const size_t l = (size_t)AIE_IGRAD_TILE * (size_t)G->H * sizeof(float);
    p->lds = l > p->lds ? l : p->lds;
  }
  if (blocks > AIE_PLAN_GRID_MAX) AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: B = %lld is more than one launch takes", fn, (long long)B);
  p->grid = (uint32_t)blocks, p->block = 256;
  return AIE_OK;
}

/* ---- the convolutional encoder: a workgroup per `tr` rows (as many as 64 KB of LDS hold, at most 16) ---- */
#define AIE_CONV_LDS_BUDGET 65536
typedef struct aie_conv_fwd_plan { aie_conv_args A; uint32_t grid, block; size_t lds; } aie_conv_fwd_plan;

/* the checks and the fill the two passes share; extra: floats per row the pass stages in LDS behind X and a1 */
static inline int aie_plan_conv_class(const char* fn, int64_t rows, const aie_conv_class* k, int backward, char* err, size_t errlen,
                                      aie_conv_args* A, uint32_t* grid, size_t* lds) {
  if (rows < 1 || !k) AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: rows = %lld with the class at %p (needs rows >= 1 and a class)", fn,
                                      (long long)rows, (const void*)k);
  if (!k->map || !k->idx || !k->emb || !k->w1 || !k->b1 || !k->w2 || !k->b2)
    AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: map, idx, emb, w1, b1, w2 and b2 must not be NULL", fn);
  if (k->C_map < 1 || k->C_map > 32)
    AIE_PLAN_REFUSE(AIE_E_UNSUPPORTED, "%s: C_map = %d map channels (supported: 1 .. 32)", fn, k->C_map);
  if (k->D < 1 || k->D > 8) AIE_PLAN_REFUSE(AIE_E_UNSUPPORTED, "%s: D = %d embedding dimensions (supported: 1 .. 8)", fn, k->D);
  if (k->h < 7 || k->h > 15 || k->w < 7 || k->w > 15)
    AIE_PLAN_REFUSE(AIE_E_UNSUPPORTED, "%s: a crop of %d x %d cells (supported: 7 .. 15 each way; full observability's whole "
                    "map is not)", fn, k->h, k->w);
  if (k->V < 1 || k->V > 128) AIE_PLAN_REFUSE(AIE_E_UNSUPPORTED, "%s: V = %d embedding rows (supported: 1 .. 128)", fn, k->V);
  const aie_conv_shape S = aie_conv_shape_of(k->C_map, k->D, k->h, k->w, k->V);
  if (k->map_ld < (int64_t)S.C_map * S.hw || k->idx_ld < 2 * (int64_t)S.hw)
    AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: row strides map_ld = %lld (needs >= %d floats) and idx_ld = %lld (needs >= %d elements)", fn,
                    (long long)k->map_ld, S.C_map * S.hw, (long long)k->idx_ld, 2 * S.hw);
  if ((((uintptr_t)k->map | (uintptr_t)k->emb | (uintptr_t)k->w1 | (uintptr_t)k->b1 | (uintptr_t)k->w2 | (uintptr_t)k->b2) & 3) ||
      ((uintptr_t)k->idx & 1))
    AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: map and the weights must be 4-byte aligned, idx 2-byte aligned", fn);
  if (!backward) {
    if (!k->x_out || ((uintptr_t)k->x_out & 3) || ((uintptr_t)k->flat & 3) || k->F_flat < 0 || k->F_flat > 1024 ||
        (k->flat != NULL) != (k->F_flat > 0) || k->x_ld < (int64_t)S.NF + k->F_flat || (k->flat && k->flat_ld < k->F_flat))
      AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: x_out (%p, x_ld %lld) must be 4-byte aligned with x_ld >= NF + F_flat = %d + %d; flat (%p, "
                      "flat_ld %lld) goes with F_flat in 1 .. 1024 and flat_ld >= F_flat, or is NULL with F_flat 0", fn,
                      (void*)k->x_out, (long long)k->x_ld, S.NF, k->F_flat, (const void*)k->flat, (long long)k->flat_ld);
  }
  memset(A, 0, sizeof(*A));
  A->map = k->map, A->idx = k->idx, A->emb = k->emb, A->w1 = k->w1, A->b1 = k->b1, A->w2 = k->w2, A->b2 = k->b2;
  A->map_ld = k->map_ld, A->idx_ld = k->idx_ld, A->rows = rows, A->S = S;
  if (!backward) A->flat = k->flat, A->flat_ld = k->flat_ld, A->x_out = k->x_out, A->x_ld = k->x_ld, A->F_flat = k->F_flat;
  A->lds_row = S.hw * S.C + S.P1 * AIE_CONV_F1 + (backward ? S.NF + S.P1 * AIE_CONV_F1 : 0);
  int tr = 16;
  while (tr > 1 && (size_t)tr * (size_t)A->lds_row * sizeof(float) > AIE_CONV_LDS_BUDGET) tr >>= 1;
  A->tr = tr;
  const int64_t nb = (rows + tr - 1) / tr;
  if (nb > AIE_PLAN_GRID_MAX) AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: %lld rows are more than one launch takes", fn, (long long)rows);
  *grid = (uint32_t)nb;
  *lds = (size_t)tr * (size_t)A->lds_row * sizeof(float);
  return AIE_OK;
}

static inline int aie_plan_conv_forward(int64_t rows, const aie_conv_class* k, char* err, size_t errlen, aie_conv_fwd_plan* p) {
  memset(p, 0, sizeof(*p));
  p->block = 256;
  return aie_plan_conv_class("aie_policy_conv_forward", rows, k, 0, err, errlen, &p->A, &p->grid, &p->lds);
}

/* the backward: rows (recompute, dz2, dz1, dx into the workspace); a segment's partials (`chunks` workgroups of 256 weight
 * entries and one for the embedding per segment); the float64 sums of the segments (256 entries a workgroup) */
typedef struct aie_conv_bwd_plan {
  aie_conv_bwd_args A;
  int64_t need;
  uint32_t grid_rows, grid_seg, grid_reduce, block;
  size_t lds_rows, lds_seg;
} aie_conv_bwd_plan;

static inline int aie_plan_conv_backward(int64_t rows, const aie_conv_grad_class* q, int query, void* d_workspace,
                                         int64_t workspace_bytes, char* err, size_t errlen, aie_conv_bwd_plan* p) {
  const char* fn = "aie_policy_conv_backward";
  memset(p, 0, sizeof(*p));
  p->block = 256;
  const int rc = aie_plan_conv_class(fn, rows, q ? &q->net : NULL, 1, err, errlen, &p->A.net, &p->grid_rows, &p->lds_rows);
  if (rc != AIE_OK) return rc;
  const aie_conv_shape* S = &p->A.net.S;
  if (!q->g_feat || !q->gemb || !q->gw1 || !q->gb1 || !q->gw2 || !q->gb2 || q->g_ld < S->NF ||
      (((uintptr_t)q->g_feat | (uintptr_t)q->gemb | (uintptr_t)q->gw1 | (uintptr_t)q->gb1 | (uintptr_t)q->gw2 | (uintptr_t)q->gb2) & 3))
    AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: g_feat (g_ld %lld >= NF = %d), gemb, gw1, gb1, gw2 and gb2 must be 4-byte aligned and not NULL",
                    fn, (long long)q->g_ld, S->NF);
  aie_conv_bwd_args* A = &p->A;
  A->g_feat = q->g_feat, A->g_ld = q->g_ld;
  A->gemb = q->gemb, A->gw1 = q->gw1, A->gb1 = q->gb1, A->gw2 = q->gw2, A->gb2 = q->gb2;
  const int64_t nseg = (rows + AIE_MLP_BWD_SEG - 1) / AIE_MLP_BWD_SEG;
  A->nseg = (int32_t)nseg;
  A->off2 = (9 * S->C + 1) * AIE_CONV_F1;
  A->off3 = A->off2 + (9 * AIE_CONV_F1 + 1) * AIE_CONV_F2;
  A->Pn = (A->off3 + S->V * S->D + 3) & ~3;
  A->chunks = (A->off3 + 255) / 256;
  const int64_t n1 = (int64_t)S->P1 * AIE_CONV_F1, nx = 2 * (int64_t)S->hw * S->D;
  const int64_t fl = rows * (2 * n1 + S->NF + nx) + nseg * A->Pn;
  p->need = ((fl + 63) & ~(int64_t)63) * (int64_t)sizeof(float);
  if (nseg * (A->chunks + 1) > AIE_PLAN_GRID_MAX)
    AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: %lld rows are more than one call takes", fn, (long long)rows);
  if (query) return AIE_OK;   /* (the workspace-bytes query stops here) */
  if (!d_workspace || ((uintptr_t)d_workspace & 15) || workspace_bytes < p->need)
    AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: the workspace (%p, %lld bytes) must be device memory, 16-byte aligned, of at least %lld "
                    "bytes (aie_policy_conv_backward_workspace_bytes)", fn, d_workspace, (long long)workspace_bytes, (long long)p->need);
  float* ws = (float*)d_workspace;
  A->a1 = ws, A->dz1 = ws + rows * n1, A->dz2 = ws + 2 * rows * n1, A->dxe = A->dz2 + rows * S->NF, A->partial = A->dxe + rows * nx;
  p->grid_seg = (uint32_t)(nseg * (A->chunks + 1));
  p->grid_reduce = (uint32_t)((A->Pn + 255) / 256);
  p->lds_seg = (size_t)AIE_CONV_EMB_TILE * (size_t)(S->V * S->D) * sizeof(float);
  return AIE_OK;
}

/* ---- aie_adam_step: a workgroup per chunk of AIE_OPT_CHUNK elements, the same grid for both launches ----
 * aie_plan_adam_groups checks the descriptors in include/aie.h's order, fills the kernels' argument without the workspace
 * pointers -- the chunk table (a tensor's first chunk in its group), the `wide` flags -- and sizes each group's share of the
 * workspace (the workspace-bytes query stops here); aie_plan_adam adds the workspace's own check and carves it. */
typedef struct aie_adam_plan {
  aie_adam_args A;
  int64_t ws_bytes[2], need;   /* each group's share (0: left out); workspace bytes of this call */
  uint32_t grid, block;
} aie_adam_plan;

static inline int aie_plan_adam_groups(const aie_opt_group* agents, const aie_opt_group* planner, char* err, size_t errlen,
                                       aie_adam_plan* p) {
  const char* fn = "aie_adam_step";
  memset(p, 0, sizeof(*p));
  const aie_opt_group* grp[2] = {agents, planner};
  int64_t total = 0;
  for (int c = 0; c < 2; ++c) {
    const aie_opt_group* g = grp[c];
    if (!g) continue;
    const char* who = c ? "planner's" : "agents'";
    aie_opt_group_k* G = &p->A.grp[c];
    if (g->n_tensors < 1 || g->n_tensors > AIE_OPT_MAX_TENSORS || !g->tensors)
      AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: the %s group has %d tensors at %p (needs 1 .. %d, not NULL)", fn, who, g->n_tensors,
                      (const void*)g->tensors, AIE_OPT_MAX_TENSORS);
    if (!(g->beta1 >= 0.0f && g->beta1 < 1.0f) || !(g->beta2 >= 0.0f && g->beta2 < 1.0f) || !(g->eps > 0.0f))
      AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: the %s group needs beta1 (%g) and beta2 (%g) in [0, 1) and eps (%g) > 0", fn, who,
                      (double)g->beta1, (double)g->beta2, (double)g->eps);
    if (!g->d_lr || ((uintptr_t)g->d_lr & 3) || !g->d_state || ((uintptr_t)g->d_state & 7) || !g->d_stats || ((uintptr_t)g->d_stats & 3))
      AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: the %s group needs d_lr (%p) and d_stats (%p) 4-byte aligned and d_state (%p) 8-byte "
                      "aligned, none NULL", fn, who, (const void*)g->d_lr, (const void*)g->d_stats, (const void*)g->d_state);
    int64_t chunks = 0;
    for (int i = 0; i < g->n_tensors; ++i) {
      const aie_opt_tensor* t = &g->tensors[i];
      const uintptr_t any = (uintptr_t)t->w | (uintptr_t)t->g | (uintptr_t)t->m | (uintptr_t)t->v;
      if (!t->w || !t->g || !t->m || !t->v || (any & 3) || t->n < 1)
        AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: tensor %d of the %s group (w %p, g %p, m %p, v %p, n %lld) needs four 4-byte aligned "
                        "pointers, none NULL, and n >= 1", fn, i, who, (const void*)t->w, (const void*)t->g, (const void*)t->m,
                        (const void*)t->v, (long long)t->n);
      const int64_t nc = t->n / AIE_OPT_CHUNK + (t->n % AIE_OPT_CHUNK ? 1 : 0);
      if (nc > AIE_PLAN_GRID_MAX - total - chunks)
        AIE_PLAN_REFUSE(AIE_E_INVALID, "%s: tensor %d of the %s group (n %lld) brings the call over the %lld chunks one launch "
                        "takes", fn, i, who, (long long)t->n, (long long)AIE_PLAN_GRID_MAX);
      aie_opt_tensor_k* k = &G->t[i];
      k->w = t->w, k->g = t->g, k->m = t->m, k->v = t->v, k->n = t->n;
      k->first = (int32_t)chunks, k->wide = !(any & 15);
      chunks += nc;
    }
    G->lr = g->d_lr, G->state = (aie_opt_state*)g->d_state, G->stats = g->d_stats;
    G->beta1 = g->beta1, G->beta2 = g->beta2, G->eps = g->eps, G->max_norm = g->max_norm;
    G->n_tensors = g->n_tensors, G->chunks = (int32_t)chunks;
    p->ws_bytes[c] = (AIE_OPT_WS_HEAD + chunks) * (int64_t)sizeof(double);
    total += chunks;
  }
  p->need = p->ws_bytes[0] + p->ws_bytes[1];
  p->grid = (uint32_t)total, p->block = AIE_OPT_SLOTS;
  return AIE_OK;
}

static inline int aie_plan_adam(const aie_opt_group* agents, const aie_opt_group* planner, void* d_workspace,
                                int64_t workspace_bytes, char* err, size_t errlen, aie_adam_plan* p) {
  const int rc = aie_plan_adam_groups(agents, planner, err, errlen, p);
  if (rc != AIE_OK || !p->grid) return rc;
  if (!d_workspace || ((uintptr_t)d_workspace & 7) || workspace_bytes < p->need)
    AIE_PLAN_REFUSE(AIE_E_INVALID, "aie_adam_step: the workspace (%p, %lld bytes) must be device memory, 8-byte aligned, of at "
                    "least %lld bytes (aie_adam_workspace_bytes)", d_workspace, (long long)workspace_bytes, (long long)p->need);
  p->A.grp[0].ws = (double*)d_workspace;
  p->A.grp[1].ws = (double*)((uint8_t*)d_workspace + p->ws_bytes[0]);
  return AIE_OK;
}

/* ---- aie_trajectory_store: a workgroup per replica ---- */
typedef struct aie_traj_plan { aie_traj_args A; uint32_t grid, block; } aie_traj_plan;

static inline int aie_plan_trajectory_store(const aie_params* P, const aie_traj_segment* segs, int32_t n_segs, int32_t n_slots,
                                            int32_t* d_slot, char* err, size_t errlen, aie_traj_plan* p) {
  memset(p, 0, sizeof(*p));
  if (!segs || n_segs < 1 || n_segs > AIE_TRAJ_MAX_SEGMENTS || n_slots < 1 || !d_slot)
    AIE_PLAN_REFUSE(AIE_E_INVALID, "aie_trajectory_store: %d segments (1 .. %d), %d slots (>= 1), segments and slot counters "
                    "not NULL", n_segs, AIE_TRAJ_MAX_SEGMENTS, n_slots);
  for (int g = 0; g < n_segs; ++g) {
    const aie_traj_segment* s = &segs[g];
    const uintptr_t sp = (uintptr_t)s->src, dp = (uintptr_t)s->dst;
    const int64_t count = s->bytes / 4;
    if (!s->src || !s->dst || s->bytes < 4 || (s->bytes & 3) || (s->src_stride & 3) || (sp & 3) || (dp & 3) || s->rows < 0 ||
        s->rows > 32767 || (s->rows > 1 && count % s->rows))
      AIE_PLAN_REFUSE(AIE_E_INVALID, "aie_trajectory_store: segment %d (%d bytes per replica, source stride %lld, rows %d): "
                      "pointers not NULL and 4-byte aligned, sizes and strides multiples of 4, rows dividing the element count", g,
                      s->bytes, (long long)s->src_stride, s->rows);
    aie_traj_seg_k* k = &p->A.seg[g];
    k->src = (const uint8_t*)s->src, k->dst = (uint8_t*)s->dst, k->src_stride = s->src_stride, k->bytes = s->bytes;
    k->rows = (int16_t)s->rows;
    k->wide = (int16_t)(s->rows <= 1 && !((sp | dp | (uintptr_t)s->src_stride | (uintptr_t)s->bytes) & 15));
  }
  p->A.slot = d_slot, p->A.n_segs = n_segs, p->A.n_slots = n_slots, p->A.E = P->E;
  p->grid = (uint32_t)P->E, p->block = 256;
  return AIE_OK;
}

#endif /* AIE_TRAINER_PLAN_H_ */
