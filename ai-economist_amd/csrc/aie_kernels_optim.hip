// ---- Adam under a gradient-norm clip, in place, for both actor classes' parameter groups (include/aie.h: aie_adam_step) ----
// Two launches over one grid: a workgroup per chunk of AIE_OPT_CHUNK consecutive elements of one tensor, thread s owning the
// chunk's elements 4s .. 4s + 3 (one 16-byte access per operand in a whole chunk of a tensor whose four pointers allow it,
// else 4-byte ones; an element past the tensor's end is neither read nor written and counts as +0).  The arithmetic is
// aie_trainer_math.h's (aie_opt_slot_sumsq, aie_opt_scalars, aie_opt_element), so the weights are the CPU twin's bit for bit.
//
// Launch 1, aie_adam_norm_kernel: the chunk's sum of squares in float64 -- the slot's four squares ascending, the butterfly
// over the wave's 64 lanes (six exchanges), the four wave sums through LDS as (s0 + s1) + (s2 + s3) -- goes to the
// workspace; a group's first workgroup also copies the group's state {t, p1, p2} there.
// Launch 2, aie_adam_update_kernel: every workgroup adds its group's chunk sums in ascending order (eight loads in flight,
// then eight additions; a word past the last counts as +0), forms the group's scalars from them, the state's copy and the
// learning rate, and updates its chunk; the group's first workgroup writes the new state and the statistics.
//
// Why this needs no atomics and no ordering between workgroups: d_state is READ in launch 1 only (one thread) and WRITTEN
// in launch 2 only (one thread), and the stream orders the launches; every workspace word has one writer in launch 1 and
// only readers in launch 2; every element of w, m and v is read and then written by the one thread that owns it; g, d_lr
// and the kernel argument are only read.  So every workgroup of launch 2 sees the same old state and the same sums,
// whichever of them runs first -- the one that writes the new state included.
#pragma once
#include "aie_device.h"
#include "aie_trainer_math.h"

#pragma clang fp contract(off)

struct OptChunk {       // what a workgroup owns
  int group, chunk;     // the group (0 agents, 1 planner) and the chunk's index in it
  aie_opt_tensor_k T;   // its tensor
  int64_t e0;           // this thread's first element
  int count;            // how many of its four elements exist
  bool quads;           // the whole chunk lies inside the tensor and 16-byte accesses are allowed: the same for every thread
};
__device__ __forceinline__ OptChunk opt_locate(const aie_adam_args& A) {
  OptChunk c;
  const int b = (int)blockIdx.x;
  c.group = b >= A.grp[0].chunks ? 1 : 0;
  const aie_opt_group_k& G = A.grp[c.group];
  c.chunk = b - (c.group ? A.grp[0].chunks : 0);
  int ti = 0;
  for (int i = 1; i < G.n_tensors; ++i)
    if (c.chunk >= G.t[i].first) ti = i;
  c.T = G.t[ti];
  const int64_t base = (int64_t)(c.chunk - c.T.first) * AIE_OPT_CHUNK;
  c.e0 = base + 4 * (int64_t)threadIdx.x;
  const int64_t left = c.T.n - c.e0;
  c.count = left >= 4 ? 4 : left > 0 ? (int)left : 0;
  c.quads = c.T.wide && base + AIE_OPT_CHUNK <= c.T.n;
  return c;
}
// The thread's four elements of one operand (0 where there is none).  QUADS is c.quads as a template argument: the
// kernels branch on it ONCE, around everything they do with memory, so that the common path is four 16-byte loads, the
// arithmetic and three 16-byte stores in a straight line (with the branch inside each access hipcc merges the two paths'
// loads into 12- and 4-byte pieces).
template <bool QUADS>
__device__ __forceinline__ void opt_load4(const float* p, const OptChunk& c, float q[4]) {
  if (QUADS) {
    const float4 f = *reinterpret_cast<const float4*>(p + c.e0);
    q[0] = f.x, q[1] = f.y, q[2] = f.z, q[3] = f.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = k < c.count ? p[c.e0 + k] : 0.0f;
  }
}
template <bool QUADS>
__device__ __forceinline__ void opt_store4(float* p, const OptChunk& c, const float q[4]) {
  if (QUADS) {
    *reinterpret_cast<float4*>(p + c.e0) = make_float4(q[0], q[1], q[2], q[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < c.count) p[c.e0 + k] = q[k];
  }
}
template <bool QUADS>
__device__ __forceinline__ double opt_slot(const OptChunk& c) {
  float g[4];
  opt_load4<QUADS>(c.T.g, c, g);
  return aie_opt_slot_sumsq(g, 4);  // (a missing element is +0: its square adds nothing to a sum that is never -0)
}
template <bool QUADS>
__device__ __forceinline__ void opt_update(const OptChunk& c, const aie_opt_step& S) {
  float g[4], w[4], m[4], v[4];
  opt_load4<QUADS>(c.T.g, c, g);
  opt_load4<QUADS>(c.T.w, c, w);
  opt_load4<QUADS>(c.T.m, c, m);
  opt_load4<QUADS>(c.T.v, c, v);
#pragma unroll
  for (int k = 0; k < 4; ++k) aie_opt_element(&S, g[k], &w[k], &m[k], &v[k]);
  opt_store4<QUADS>(c.T.w, c, w);
  opt_store4<QUADS>(c.T.m, c, m);
  opt_store4<QUADS>(c.T.v, c, v);
}

extern "C" __global__ void __launch_bounds__(256) aie_adam_norm_kernel(const aie_adam_args A) {
  __shared__ double wave_sum[4];
  const OptChunk c = opt_locate(A);
  const aie_opt_group_k& G = A.grp[c.group];
  double acc = c.quads ? opt_slot<true>(c) : opt_slot<false>(c);
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) acc += __shfl_xor(acc, d, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    G.ws[AIE_OPT_WS_HEAD + c.chunk] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
    if (c.chunk == 0) {  // the state's copy: launch 2 reads this, never d_state
      const uint64_t* src = reinterpret_cast<const uint64_t*>(G.state);
      uint64_t* dst = reinterpret_cast<uint64_t*>(G.ws);
      dst[0] = src[0], dst[1] = src[1], dst[2] = src[2], dst[3] = 0;
    }
  }
}

extern "C" __global__ void __launch_bounds__(256) aie_adam_update_kernel(const aie_adam_args A) {
  const OptChunk c = opt_locate(A);
  const aie_opt_group_k& G = A.grp[c.group];
  const double* part = G.ws + AIE_OPT_WS_HEAD;
  double n2 = 0.0;
  for (int c0 = 0; c0 < G.chunks; c0 += 8) {
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {  // (a clamped address, then the select: no load past the last word, no branch)
      const int i = c0 + k < G.chunks ? c0 + k : G.chunks - 1;
      const double x = part[i];
      v[k] = c0 + k < G.chunks ? x : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) n2 += v[k];
  }
  aie_opt_state old;
  old.t = (int64_t)reinterpret_cast<const uint64_t*>(G.ws)[0];
  old.p1 = G.ws[1], old.p2 = G.ws[2], old.pad_ = 0;
  const aie_opt_step S = aie_opt_scalars(n2, G.max_norm, G.beta1, G.beta2, G.eps, G.lr[0], old);
  if (c.chunk == 0 && threadIdx.x == 0) {
    aie_opt_stats(&S, G.stats);
    if (!S.skipped) G.state->t = S.next.t, G.state->p1 = S.next.p1, G.state->p2 = S.next.p2;
  }
  if (S.skipped) return;
  if (c.quads) opt_update<true>(c, S);
  else opt_update<false>(c, S);
}
