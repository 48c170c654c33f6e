// ---- the policy network's forward pass of both actor classes in one launch (include/aie.h: aie_policy_mlp_forward) ------
// x[F] -> relu -> H -> relu -> H -> M logits (+ 1 value) per row; the arithmetic is aie_trainer_math.h's (aie_mlp_row): every
// output is ONE ascending-k fmaf chain that starts from the bias.  v_mfma_f32_16x16x4_f32 is exactly that chain (one
// rounding per product, nothing wider in between), so the accumulator is initialised with the bias and a tile's K is
// walked in order by one accumulator; MFMA latency is hidden by the independent output tiles a wave owns, never by a
// second accumulator for the same output.
//
// A workgroup (4 waves) owns AIE_MLP_TILE_ROWS rows of one class -- the block index range is split between the classes --
// and carries them through all three layers: the observation tile is staged into LDS (in chunks of AIE_MLP_CHUNK columns,
// zero-padded to a multiple of 4), h1 and h2 live in LDS, and only logits and values leave the chip.  Wave w owns the 16-
// column output tiles w, w + 4, ... of a layer, two at a time, each over all the row tiles (2 x RT accumulators of 4
// registers).  A fragments come from LDS (lane l: row l & 15, k = l >> 4), B fragments straight from the caller's weights
// in global memory (lane l: k = l >> 4, column l & 15: 64 contiguous bytes per k), eight k-steps ahead of their use: the
// weights are read at every launch (L2-resident, 160 - 190 KB per class), so an in-place optimizer step is seen by the
// next launch or replay.  The value head is column M of the head's matrix.
// Ragged edges: rows past the class's last are staged as zeros and never stored; k past F multiplies a staged 0 by a 0
// weight; columns past M (+ 1) compute on clamped addresses and are never stored (columns do not mix in an MFMA).
// LDS: dynamic, 16 x RT x (lds_a + lds_h) floats -- 34 KB at H = 128, 66 KB at H = 256 with 32 rows: above the 64 KB of older
// parts; the launch relies on gfx950's 160 KB per workgroup, the only target this library is built for.
// No atomics, no allocation, no synchronisation with the host.
#pragma once
#include "aie_device.h"
#include "aie_trainer_math.h"

typedef float aie_mlp_f4 __attribute__((ext_vector_type(4)));
typedef const float __attribute__((address_space(1))) * aie_mlp_gptr;  // global memory, said so: a walked pointer otherwise loads as flat

constexpr int MLP_KC = 8;  // k-steps (of 4) of B fragments in flight per column tile

// a lane's view of one 16-column tile of a layer's weights: entry k at p[k * stride]
struct MlpCol {
  const float* p;
  uint32_t stride;
  float bias;
  int col;  // the lane's column in the layer's output (may be past the last: never stored)
};
__device__ __forceinline__ MlpCol mlp_col(int tile, int lane, const float* w, int n, const float* b, const float* wv, const float* bv) {
  MlpCol c;
  c.col = tile * 16 + (lane & 15);
  if (c.col < n) {
    c.p = w + c.col;
    c.stride = (uint32_t)n;
    c.bias = b[c.col];
  } else if (c.col == n && wv) {
    c.p = wv;
    c.stride = 1u;
    c.bias = bv[0];
  } else {  // a column nobody stores: any address in bounds
    c.p = w;
    c.stride = (uint32_t)n;
    c.bias = 0.0f;
  }
  return c;
}

// The B fragments of MLP_KC k-steps.  Guarded: any k, the lane's k past K gives 0 (the address is clamped, the select
// follows the load: no branch around a load).  Fast: every k is inside K; a pointer walks down the lane's column.
template <int CT>
__device__ __forceinline__ void mlp_load_b_guarded(float (&b)[2][MLP_KC], const MlpCol (&c)[2], int kq, int K) {
#pragma unroll
  for (int t = 0; t < CT; ++t) {
#pragma unroll
    for (int j = 0; j < MLP_KC; ++j) {
      const int k = kq + 4 * j;
      const float v = c[t].p[(uint32_t)(k < K ? k : K - 1) * c[t].stride];
      b[t][j] = k < K ? v : 0.0f;
    }
  }
}
template <int CT>
__device__ __forceinline__ void mlp_load_b_fast(float (&b)[2][MLP_KC], aie_mlp_gptr (&pk)[2], const uint32_t (&st4)[2]) {
#pragma unroll
  for (int t = 0; t < CT; ++t) {
#pragma unroll
    for (int j = 0; j < MLP_KC; ++j) {
      b[t][j] = *pk[t];
      pk[t] += st4[t];
    }
  }
}

// one k-step: a fragment per row tile from LDS, CT x RT MFMAs
template <int RT, int CT>
__device__ __forceinline__ void mlp_step(const float* a_lane, int S, int s, const float (&b)[2][MLP_KC], int j, aie_mlp_f4 (&acc)[2][RT]) {
  float a[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) a[r] = a_lane[r * 16 * S + 4 * s];
#pragma unroll
  for (int t = 0; t < CT; ++t) {
#pragma unroll
    for (int r = 0; r < RT; ++r) acc[t][r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], b[t][j], acc[t][r], 0, 0, 0);
  }
}

// acc[t][r] += act[16 r .. 16 r + 15][0 .. 4 nsteps) x W[k .. k + 4 nsteps)[tile t], k ascending; the first nfull k-steps lie
// wholly inside K.  Whole groups of MLP_KC such steps run without a branch, each behind the loads of the group after it,
// which are issued first (the scheduling barrier keeps them there: left alone, the compiler sinks them to the end of the
// group, where the wait for them follows at once); the last, partial or ragged group steps under its count.
template <int RT, int CT>
__device__ __forceinline__ void mlp_tiles(const float* a_lane, int S, int nsteps, int nfull, const MlpCol (&c)[2], int kq, int K,
                                          aie_mlp_f4 (&acc)[2][RT]) {
  float b0[2][MLP_KC], b1[2][MLP_KC];  // two register sets, used in turn: no copies, and each wait counts exactly
  const int G = nfull / MLP_KC;
  aie_mlp_gptr pk[2] = {(aie_mlp_gptr)c[0].p, (aie_mlp_gptr)c[1].p};
  const uint32_t st4[2] = {4u * c[0].stride, 4u * c[1].stride};
  if (G > 0) {
#pragma unroll
    for (int t = 0; t < 2; ++t) pk[t] += (uint32_t)kq * c[t].stride;
    mlp_load_b_fast<CT>(b0, pk, st4);
  } else {
    mlp_load_b_guarded<CT>(b0, c, kq, K);
  }
  int g = 0, s0 = 0;
  for (; g + 1 < G; g += 2, s0 += 2 * MLP_KC) {  // b0 holds group g
    mlp_load_b_fast<CT>(b1, pk, st4);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < MLP_KC; ++j) mlp_step<RT, CT>(a_lane, S, s0 + j, b0, j, acc);
    if (g + 2 < G) mlp_load_b_fast<CT>(b0, pk, st4);
    else mlp_load_b_guarded<CT>(b0, c, kq + 4 * (s0 + 2 * MLP_KC), K);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < MLP_KC; ++j) mlp_step<RT, CT>(a_lane, S, s0 + MLP_KC + j, b1, j, acc);
  }
  if (g < G) {  // one whole group left in b0; the ragged end goes through b1 and back
    mlp_load_b_guarded<CT>(b1, c, kq + 4 * (s0 + MLP_KC), K);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < MLP_KC; ++j) mlp_step<RT, CT>(a_lane, S, s0 + j, b0, j, acc);
    s0 += MLP_KC;
#pragma unroll
    for (int t = 0; t < CT; ++t) {
#pragma unroll
      for (int j = 0; j < MLP_KC; ++j) b0[t][j] = b1[t][j];
    }
  }
#pragma unroll
  for (int j = 0; j < MLP_KC; ++j) {
    if (s0 + j < nsteps) mlp_step<RT, CT>(a_lane, S, s0 + j, b0, j, acc);
  }
}

// One layer of the tile.  Source: `act` [TM][S] in LDS -- staged here from xg (the first layer: global rows, chunk by
// chunk) or left there by the layer before.  Output: relu into `dst` [TM][SD] in LDS (a hidden layer), or logits / values
// in global memory (dst nullptr).  Every wave runs the same loops (the barriers are inside them).
template <int RT>
__device__ __forceinline__ void mlp_layer(float* act, int S, int K, const float* xg, int64_t x_ld, int nrows, const float* w, int n,
                                          const float* b, const float* wv, const float* bv, float* dst, int SD, float* logits,
                                          float* values) {
  constexpr int TM = 16 * RT;
  const int lane = (int)threadIdx.x & 63, wave = aie::uni((int)(threadIdx.x >> 6));
  const int NT = (n + (wv ? 1 : 0) + 15) >> 4, ngroups = (NT + 7) >> 3;
  const int Kpad = (K + 3) & ~3;
  const int nchunks = xg ? (Kpad + AIE_MLP_CHUNK - 1) / AIE_MLP_CHUNK : 1;
  const float* a_lane = act + (lane & 15) * S + (lane >> 4);
  for (int g = 0; g < ngroups; ++g) {
    const int t0 = 8 * g + wave, t1 = t0 + 4;
    MlpCol c[2] = {mlp_col(t0 < NT ? t0 : 0, lane, w, n, b, wv, bv), mlp_col(t1 < NT ? t1 : 0, lane, w, n, b, wv, bv)};
    aie_mlp_f4 acc[2][RT];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int r = 0; r < RT; ++r) acc[t][r] = aie_mlp_f4{c[t].bias, c[t].bias, c[t].bias, c[t].bias};
    }
    for (int ch = 0; ch < nchunks; ++ch) {
      const int k0 = ch * AIE_MLP_CHUNK, kc = Kpad - k0 < AIE_MLP_CHUNK ? Kpad - k0 : AIE_MLP_CHUNK;
      if (xg && (nchunks > 1 || g == 0)) {  // (one chunk: staged once, for every group)
        if (g || ch) __syncthreads();       // the chunk before has been read by every wave
        // the wave's rows 4 i + wave, 64 columns per pass: every load of the chunk is issued before the first LDS store
        constexpr int NP = AIE_MLP_CHUNK / 64;
        float v[NP][TM / 4];
#pragma unroll
        for (int u = 0; u < NP; ++u) {
          if (64 * u < kc) {
            const int col = k0 + 64 * u + lane;
#pragma unroll
            for (int i = 0; i < TM / 4; ++i) {
              const int row = 4 * i + wave;
              v[u][i] = xg[(int64_t)(row < nrows ? row : nrows - 1) * x_ld + (col < K ? col : K - 1)];
            }
          }
        }
#pragma unroll
        for (int u = 0; u < NP; ++u) {
          const int cc = 64 * u + lane, col = k0 + cc;
          if (cc < kc) {
#pragma unroll
            for (int i = 0; i < TM / 4; ++i) {
              const int row = 4 * i + wave;
              act[row * S + cc] = (row < nrows && col < K) ? v[u][i] : 0.0f;
            }
          }
        }
        __syncthreads();
      }
      const int nsteps = kc >> 2, nfull = (K - k0) >> 2 < nsteps ? (K - k0) >> 2 : nsteps;
      if (t1 < NT) mlp_tiles<RT, 2>(a_lane, S, nsteps, nfull, c, k0 + (lane >> 4), K, acc);
      else if (t0 < NT) mlp_tiles<RT, 1>(a_lane, S, nsteps, nfull, c, k0 + (lane >> 4), K, acc);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if ((t ? t1 : t0) >= NT) continue;
      const int col = c[t].col;
#pragma unroll
      for (int r = 0; r < RT; ++r) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int row = 16 * r + 4 * (lane >> 4) + j;
          const float v = acc[t][r][j];
          if (dst) {
            dst[row * SD + col] = aie_mlp_relu(v);
          } else if (row < nrows) {
            if (col < n) logits[(int64_t)row * n + col] = v;
            else if (col == n && wv) values[row] = v;
          }
        }
      }
    }
  }
}

// (three waves per SIMD: the 640 workgroups of C2 at 4096 replicas are then resident at once)
extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) aie_policy_mlp_kernel(const aie_mlp_args A) {
  extern __shared__ float mlp_lds[];
  constexpr int TM = AIE_MLP_TILE_ROWS, RT = TM / 16;
  const bool ag = blockIdx.x < (uint32_t)A.agents.blocks;
  const aie_mlp_group& G = ag ? A.agents : A.planner;
  const int64_t row0 = (int64_t)(ag ? blockIdx.x : blockIdx.x - (uint32_t)A.agents.blocks) * TM;
  const int nrows = G.rows - row0 < TM ? (int)(G.rows - row0) : TM;
  const int SA = G.lds_a, SH = G.lds_h, H = G.H;
  float* buf_a = mlp_lds;            // the observation chunk, then h2
  float* buf_h = mlp_lds + TM * SA;  // h1
  mlp_layer<RT>(buf_a, SA, G.F, G.x + row0 * G.x_ld, G.x_ld, nrows, G.w1, H, G.b1, nullptr, nullptr, buf_h, SH, nullptr, nullptr);
  __syncthreads();
  mlp_layer<RT>(buf_h, SH, H, nullptr, 0, nrows, G.w2, H, G.b2, nullptr, nullptr, buf_a, SA, nullptr, nullptr);
  __syncthreads();
  mlp_layer<RT>(buf_a, SA, H, nullptr, 0, nrows, G.w3, G.M, G.b3, G.wv, G.bv, nullptr, 0, G.logits + row0 * G.M,
                G.values ? G.values + row0 : nullptr);
}
