// ---- the policy network's backward pass: the weights' gradients of both actor classes, three launches ---------------------
// (include/aie.h: aie_policy_mlp_backward; the arithmetic is aie_trainer_math.h's: aie_mlp_row_backward and aie_mlp_grad_entry)
//
// A. aie_policy_mlp_bwd_rows_kernel: the forward's row tiles (AIE_MLP_TILE_ROWS rows of one class per workgroup, the block
//    range split between the classes).  h1 and h2 are recomputed with the forward's machinery (mlp_tiles: the same MFMA
//    chains from the bias), dz3 = g_logits is staged into LDS in chunks like the observations, and the two transposed
//    products run through the same mlp_tiles from a zero accumulator.  THE TRANSPOSED OPERAND is read straight from global
//    memory as the B fragment: lane l needs W[j = tile + (l & 15)][k = l >> 4, + 4, ...], which is a walk ALONG row j of
//    the row-major weights (stride 1 in k).  Lanes of one k are a row apart (not coalesced), but a lane's MLP_KC loads in
//    flight are 4 floats apart each: they cover its 128-byte line, so every line that comes from L2 is used whole, and
//    the weights (160 - 190 KB per class) are L2- and mostly L1-resident.  A transposed LDS tile would cost a barrier pair
//    and 16 x RT x H more floats of LDS per layer for an operand each wave reads once.  The value column's term, the LAST of
//    dh2's chain, is one fmaf in the epilogue.  h1, h2, dz2 and dz1 go to the workspace as [rows, H].
// B. aie_policy_mlp_bwd_atd_kernel: gW = a^T dz per segment of AIE_MLP_BWD_SEG rows.  A workgroup (4 waves) owns an item: four
//    16-row bands of one layer's [(K + 1), N] block (one per wave) by up to four 16-column tiles, K running over the
//    segment's rows ascending in ONE accumulator per tile (a wave's four tiles are the independent MFMAs that hide the
//    latency).  The two 64-column panels -- a[r][64 bgroup ..] and dz[r][64 group ..] -- are staged through LDS 32 rows at a
//    time, 256 contiguous bytes per row, the next chunk's loads in flight during this chunk's MFMAs; fragments are LDS
//    reads (A lane l = panel[4 s + (l >> 4)][16 wave + (l & 15)], B likewise per tile), conflict-free at a row stride of 80.
//    Row K of the block is the bias: a constant 1.  Column M of the head's block is the value head: dz = g_values.
// C. aie_policy_mlp_bwd_reduce_kernel: one thread per gradient entry adds its segment partials in float64, ascending.
// No atomics, no allocation, no scratch; rows, columns and k outside the arrays read clamped addresses and contribute zeros.
#pragma once
#include "aie_kernels_mlp.hip"  // the forward's machinery: MlpCol, mlp_tiles, aie_mlp_f4

// A hidden layer of the forward (fwd: acc from the bias, relu) or a transposed product of the backward (acc from 0, the
// value term, the ReLU mask) on the tile.  Source: `act` [TM][S] in LDS, staged here from xg (global rows of K floats) or
// left there by the layer before.  w: fwd [K, H] (column j at w + j, stride H); bwd [H, K] (row j at w + j K, stride 1).
// Output (row, j): into dst [TM][SD] in LDS (or none) and into gout [rows, H] for the rows that exist.
template <int RT, bool FWD>
__device__ __forceinline__ void mlp_bwd_layer(float* act, int S, int K, const float* xg, int64_t x_ld, int nrows, const float* w, int H,
                                              const float* b, const float* wv, const float* gv, const float* mask, int SM, float* dst,
                                              int SD, float* gout) {
  constexpr int TM = 16 * RT;
  const int lane = (int)threadIdx.x & 63, wave = aie::uni((int)(threadIdx.x >> 6));
  const int NT = H >> 4, ngroups = (NT + 7) >> 3;
  const int Kpad = (K + 3) & ~3;
  const int nchunks = xg ? (Kpad + AIE_MLP_CHUNK - 1) / AIE_MLP_CHUNK : 1;
  const float* a_lane = act + (lane & 15) * S + (lane >> 4);
  for (int g = 0; g < ngroups; ++g) {
    const int t0 = 8 * g + wave, t1 = t0 + 4;
    MlpCol c[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int tile = (t ? t1 : t0) < NT ? (t ? t1 : t0) : 0;
      c[t].col = tile * 16 + (lane & 15);
      c[t].p = FWD ? w + c[t].col : w + (int64_t)c[t].col * K;
      c[t].stride = FWD ? (uint32_t)H : 1u;
      c[t].bias = FWD ? b[c[t].col] : 0.0f;
    }
    aie_mlp_f4 acc[2][RT];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int r = 0; r < RT; ++r) acc[t][r] = aie_mlp_f4{c[t].bias, c[t].bias, c[t].bias, c[t].bias};
    }
    for (int ch = 0; ch < nchunks; ++ch) {
      const int k0 = ch * AIE_MLP_CHUNK, kc = Kpad - k0 < AIE_MLP_CHUNK ? Kpad - k0 : AIE_MLP_CHUNK;
      if (xg && (nchunks > 1 || g == 0)) {
        if (g || ch) __syncthreads();
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
      const float wvj = (!FWD && wv) ? wv[col] : 0.0f;
#pragma unroll
      for (int r = 0; r < RT; ++r) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int row = 16 * r + 4 * (lane >> 4) + j;
          float v = acc[t][r][j];
          if (FWD) {
            v = aie_mlp_relu(v);
          } else {
            if (wv) v = fmaf(row < nrows ? gv[row] : 0.0f, wvj, v);
            v = mask[row * SM + col] > 0.0f ? v : 0.0f;
          }
          if (dst) dst[row * SD + col] = v;
          if (row < nrows) gout[(int64_t)row * H + col] = v;
        }
      }
    }
  }
}

extern "C" __global__ void __launch_bounds__(256) aie_policy_mlp_bwd_rows_kernel(const aie_mlp_bwd_args A) {
  extern __shared__ float mlp_bwd_lds[];
  constexpr int TM = AIE_MLP_TILE_ROWS, RT = TM / 16;
  const bool ag = blockIdx.x < (uint32_t)A.agents.net.blocks;
  const aie_mlp_bwd_group& Q = ag ? A.agents : A.planner;
  const aie_mlp_group& G = Q.net;
  const int64_t row0 = (int64_t)(ag ? blockIdx.x : blockIdx.x - (uint32_t)A.agents.net.blocks) * TM;
  const int nrows = G.rows - row0 < TM ? (int)(G.rows - row0) : TM;
  const int SA = G.lds_a, SH = G.lds_h, SC = Q.lds_c, H = G.H;
  float* buf_a = mlp_bwd_lds;            // the observation chunk, then h2, then dz2 (in place: an entry's own thread)
  float* buf_h = buf_a + TM * SA;        // h1
  float* buf_c = buf_h + TM * SH;        // the dz3 chunk
  mlp_bwd_layer<RT, true>(buf_a, SA, G.F, G.x + row0 * G.x_ld, G.x_ld, nrows, G.w1, H, G.b1, nullptr, nullptr, nullptr, 0, buf_h, SH,
                          Q.h1 + row0 * H);
  __syncthreads();
  mlp_bwd_layer<RT, true>(buf_h, SH, H, nullptr, 0, nrows, G.w2, H, G.b2, nullptr, nullptr, nullptr, 0, buf_a, SA, Q.h2 + row0 * H);
  __syncthreads();
  mlp_bwd_layer<RT, false>(buf_c, SC, G.M, Q.g_logits + row0 * G.M, G.M, nrows, G.w3, H, nullptr, G.wv,
                           Q.g_values ? Q.g_values + row0 : nullptr, buf_a, SA, buf_a, SA, Q.dz2 + row0 * H);
  __syncthreads();
  mlp_bwd_layer<RT, false>(buf_a, SA, H, nullptr, 0, nrows, G.w2, H, nullptr, nullptr, nullptr, buf_h, SH, nullptr, 0, Q.dz1 + row0 * H);
}

// a thread's staging column of one operand of the a^T dz product: entry r at p[r * ld]; load: from memory, else `other`
struct MlpBwdCol {
  aie_mlp_gptr p;
  int64_t ld;
  bool load;
  float other;
};
constexpr int MLP_BWD_R = 32;   // rows staged at a time
constexpr int MLP_BWD_S = 80;   // the LDS images' row stride (floats): 64 columns + 16, so that a fragment's 4 rows x 16 columns fall on 64 banks
constexpr int MLP_BWD_CT = 4;   // column tiles per wave

// rows c R + sr, + 4, ... of the column, zeros past the segment's last row (the address is clamped, the select follows the load)
__device__ __forceinline__ void mlp_bwd_fetch(float (&v)[MLP_BWD_R / 4], const MlpBwdCol& col, int c, int sr, int nr) {
#pragma unroll
  for (int i = 0; i < MLP_BWD_R / 4; ++i) {
    const int r = c * MLP_BWD_R + sr + 4 * i;
    const float x = col.p[(r < nr ? r : nr - 1) * col.ld];
    v[i] = r < nr ? (col.load ? x : col.other) : 0.0f;
  }
}

extern "C" __global__ void __launch_bounds__(256) aie_policy_mlp_bwd_atd_kernel(const aie_mlp_bwd_args A) {
  __shared__ float sa[MLP_BWD_R * MLP_BWD_S], sd[MLP_BWD_R * MLP_BWD_S];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = aie::uni(tid >> 6);
  int64_t item = blockIdx.x;
  const bool ag = item < A.agents.n_items;
  const aie_mlp_bwd_group& Q = ag ? A.agents : A.planner;
  if (!ag) item -= A.agents.n_items;
  if (item >= Q.n_items) return;
  const aie_mlp_group& G = Q.net;
  const int seg = (int)(item / Q.per_seg);
  int rem = (int)(item - (int64_t)seg * Q.per_seg);
  const int L = rem < Q.items[0] ? 0 : rem < Q.items[0] + Q.items[1] ? 1 : 2;
  rem -= L > 0 ? Q.items[0] : 0;
  rem -= L > 1 ? Q.items[1] : 0;
  const int bgroup = rem / Q.cg[L], group = rem - bgroup * Q.cg[L];
  // the layer's operands: a [rows, K] with leading dimension a_ld, dz [rows, Nd] contiguous (+ the value column)
  const float* a = L == 0 ? G.x : L == 1 ? Q.h1 : Q.h2;
  const int64_t a_ld = L == 0 ? G.x_ld : G.H;
  const int K = L == 0 ? G.F : G.H;
  const float* d = L == 0 ? Q.dz1 : L == 1 ? Q.dz2 : Q.g_logits;
  const int Nd = L == 2 ? G.M : G.H;           // the columns of d
  const int N = L == 2 ? Q.N3 : G.H;           // the columns of the block
  const int off = L == 0 ? 0 : L == 1 ? Q.off2 : Q.off3;
  const int64_t r0 = (int64_t)seg * AIE_MLP_BWD_SEG;
  const int nr = G.rows - r0 < AIE_MLP_BWD_SEG ? (int)(G.rows - r0) : AIE_MLP_BWD_SEG;

  // staging: thread t brings column t & 63 of both 64-column panels, rows (t >> 6) + 4 i of the chunk: 256 contiguous bytes per row
  const int sc = tid & 63, sr = tid >> 6;
  const int ka = bgroup * 64 + sc, jd = group * 64 + sc;
  MlpBwdCol ca, cd;
  ca.load = ka < K, ca.other = ka == K ? 1.0f : 0.0f;  // row K of the block: the bias, a constant 1
  ca.p = (aie_mlp_gptr)(a + r0 * a_ld + (ca.load ? ka : 0)), ca.ld = a_ld;
  cd.other = 0.0f;
  if (jd < Nd) {
    cd.load = true, cd.p = (aie_mlp_gptr)(d + r0 * Nd + jd), cd.ld = Nd;
  } else if (jd == Nd && jd < N) {  // the value head's column: g_values [rows]
    cd.load = true, cd.p = (aie_mlp_gptr)(Q.g_values + r0), cd.ld = 1;
  } else {
    cd.load = false, cd.p = (aie_mlp_gptr)(d + r0 * Nd), cd.ld = Nd;
  }
  const int band = bgroup * 4 + wave;
  const bool has_band = band * 16 <= K;                                  // (uniform in the wave)
  const int ntiles = (N + 15) >> 4, nct = ntiles - group * MLP_BWD_CT;   // this workgroup's column tiles (uniform)
  aie_mlp_f4 acc[MLP_BWD_CT];
#pragma unroll
  for (int t = 0; t < MLP_BWD_CT; ++t) acc[t] = aie_mlp_f4{0.0f, 0.0f, 0.0f, 0.0f};
  const float* fa = sa + (lane >> 4) * MLP_BWD_S + wave * 16 + (lane & 15);
  const float* fb = sd + (lane >> 4) * MLP_BWD_S + (lane & 15);
  const int nchunks = (nr + MLP_BWD_R - 1) / MLP_BWD_R;
  float va[MLP_BWD_R / 4], vd[MLP_BWD_R / 4];
  mlp_bwd_fetch(va, ca, 0, sr, nr);
  mlp_bwd_fetch(vd, cd, 0, sr, nr);
  for (int c = 0; c < nchunks; ++c) {
    if (c) __syncthreads();  // the chunk before has been read by every wave
#pragma unroll
    for (int i = 0; i < MLP_BWD_R / 4; ++i) {
      sa[(sr + 4 * i) * MLP_BWD_S + sc] = va[i];
      sd[(sr + 4 * i) * MLP_BWD_S + sc] = vd[i];
    }
    __syncthreads();
    if (c + 1 < nchunks) {  // the next chunk's loads fly during this one's MFMAs
      mlp_bwd_fetch(va, ca, c + 1, sr, nr);
      mlp_bwd_fetch(vd, cd, c + 1, sr, nr);
    }
    if (has_band) {
      const int left = nr - c * MLP_BWD_R, nsteps = ((left < MLP_BWD_R ? left : MLP_BWD_R) + 3) >> 2;
#pragma unroll
      for (int s = 0; s < MLP_BWD_R / 4; ++s) {
        if (s < nsteps) {
          const float x = fa[4 * s * MLP_BWD_S];
#pragma unroll
          for (int t = 0; t < MLP_BWD_CT; ++t) {
            if (t < nct) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(x, fb[4 * s * MLP_BWD_S + 16 * t], acc[t], 0, 0, 0);
          }
        }
      }
    }
  }
  if (!has_band) return;
  float* out = Q.partial + (int64_t)seg * Q.P + off;
#pragma unroll
  for (int t = 0; t < MLP_BWD_CT; ++t) {
    const int j = (group * MLP_BWD_CT + t) * 16 + (lane & 15);
    if (t < nct && j < N) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = band * 16 + 4 * (lane >> 4) + i;
        if (k <= K) out[k * N + j] = acc[t][i];
      }
    }
  }
}

extern "C" __global__ void __launch_bounds__(256) aie_policy_mlp_bwd_reduce_kernel(const aie_mlp_bwd_args A) {
  const bool ag = blockIdx.x < (uint32_t)A.reduce_blocks_a;
  const aie_mlp_bwd_group& Q = ag ? A.agents : A.planner;
  const aie_mlp_group& G = Q.net;
  const int e = (int)(ag ? blockIdx.x : blockIdx.x - (uint32_t)A.reduce_blocks_a) * 256 + (int)threadIdx.x;
  if (e >= Q.P) return;
  double sum = 0.0;
  const float* p = Q.partial + e;
  for (int s = 0; s < Q.nseg; ++s) sum += (double)p[(int64_t)s * Q.P];
  const float v = (float)sum;
  const int L = e < Q.off2 ? 0 : e < Q.off3 ? 1 : 2;
  const int K = L == 0 ? G.F : G.H, N = L == 2 ? Q.N3 : G.H;
  const int q = e - (L == 0 ? 0 : L == 1 ? Q.off2 : Q.off3);
  const int k = q / N, j = q - k * N;
  if (L == 2) {
    if (j == G.M) (k == K ? Q.gbv : Q.gwv + k)[0] = v;
    else (k == K ? Q.gb3 + j : Q.gw3 + (int64_t)k * G.M + j)[0] = v;
  } else {
    float* gw = L == 0 ? Q.gw1 : Q.gw2;
    float* gb = L == 0 ? Q.gb1 : Q.gb2;
    (k == K ? gb + j : gw + (int64_t)k * G.H + j)[0] = v;
  }
}
