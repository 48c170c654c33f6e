// ---- the convolutional encoder of the agents' egocentric crop, and the MLP's input gradient that feeds its backward ------
// (include/aie.h: aie_policy_conv_forward, aie_policy_conv_backward, aie_policy_mlp_input_grad; the arithmetic is
// aie_trainer_math.h's, and every output here is computed BY that header's helper -- aie_conv1_out, aie_conv2_out,
// aie_conv_da1, aie_conv_dx, aie_mlp_chain's order -- one thread per output, one accumulator per chain: the device's bits
// are the host's by construction, with nothing padded and nothing split.)
//
// Forward, one launch.  A workgroup (256 threads) owns A.tr consecutive rows (as many as 64 KB of LDS hold: 4 on the 11 x 11
// crop).  The rows' input -- the map's planes and the embedded indices, C channels -- is staged once into LDS cell-major
// ([h w][C]: a window's C channels are contiguous, and the 16 lanes that share an output position read one address), conv1
// writes a1 into LDS beside it, conv2 reads a1 and writes the features straight to x_out; the flat row is copied behind
// them.  Lanes run along the filters: a weight read is 64 (conv1) or 128 (conv2) contiguous bytes from the caller's
// buffers at every launch (27 KB for both layers: L2- and mostly L1-resident), so an in-place optimizer step is seen by the
// next launch or replay.  Rows past the last are staged as zeros and neither computed nor stored.
// Backward, three launches.  A: the forward's tiles again -- a1 and a2 recomputed, dz2 from g_feat under a2's mask, dz1 =
// conv2's transposed product under a1's mask, dx of the embedding's channels -- with a1, dz1, dz2 and dx left in the
// workspace.  B: per segment of AIE_MLP_BWD_SEG rows, a thread per weight-gradient entry walks the segment's rows and
// output positions in one ascending chain; one more workgroup per segment scatters the rows' dx into per-row [V][D] tables
// in LDS (a thread owns one (row, d) column of the tables: no two threads touch one word) and adds the tables row by row.
// C: a thread per entry adds the segments' partials in float64, ascending.  No atomics, no allocation, no scratch.
#pragma once
#include "aie_device.h"
#include "aie_trainer_math.h"

// the tile's input into LDS: X of local row rl at lds + rl * A.lds_row, [h w][C]; rows past the last are zeros
__device__ __forceinline__ void conv_stage_input(const aie_conv_args& A, int64_t row0, int nrows, float* lds) {
  const aie_conv_shape& S = A.S;
  const int hwC = S.hw * S.C;
  for (int o = (int)threadIdx.x; o < A.tr * hwC; o += 256) {
    const int rl = o / hwC, rem = o - rl * hwC, c = rem / S.hw, cell = rem - c * S.hw;  // cell fastest: the planes are read in order
    float v = 0.0f;
    if (rl < nrows) v = aie_conv_input_at(&S, A.map + (row0 + rl) * A.map_ld, A.idx + (row0 + rl) * A.idx_ld, A.emb, c, cell);
    lds[rl * A.lds_row + cell * S.C + c] = v;
  }
}
// a1 of the tile's rows into LDS behind X
__device__ __forceinline__ void conv_layer1(const aie_conv_args& A, int nrows, float* lds) {
  const aie_conv_shape& S = A.S;
  const int n1 = S.P1 * AIE_CONV_F1, hwC = S.hw * S.C;
  for (int o = (int)threadIdx.x; o < nrows * n1; o += 256) {
    const int rl = o / n1, rem = o - rl * n1;
    const float* X = lds + rl * A.lds_row;
    lds[rl * A.lds_row + hwC + rem] = aie_conv1_out(&S, X, A.w1, A.b1, rem / AIE_CONV_F1, rem % AIE_CONV_F1);
  }
}

extern "C" __global__ void __launch_bounds__(256) aie_policy_conv_kernel(const aie_conv_args A) {
  extern __shared__ float conv_lds[];
  const aie_conv_shape& S = A.S;
  const int64_t row0 = (int64_t)blockIdx.x * A.tr;
  const int nrows = A.rows - row0 < A.tr ? (int)(A.rows - row0) : A.tr;
  const int hwC = S.hw * S.C;
  conv_stage_input(A, row0, nrows, conv_lds);
  __syncthreads();
  conv_layer1(A, nrows, conv_lds);
  __syncthreads();
  for (int o = (int)threadIdx.x; o < nrows * S.NF; o += 256) {
    const int rl = o / S.NF, rem = o - rl * S.NF;
    const float* a1 = conv_lds + rl * A.lds_row + hwC;
    A.x_out[(row0 + rl) * A.x_ld + rem] = aie_conv2_out(&S, a1, A.w2, A.b2, rem / AIE_CONV_F2, rem % AIE_CONV_F2);
  }
  for (int o = (int)threadIdx.x; o < nrows * A.F_flat; o += 256) {
    const int rl = o / A.F_flat, j = o - rl * A.F_flat;
    A.x_out[(row0 + rl) * A.x_ld + S.NF + j] = A.flat[(row0 + rl) * A.flat_ld + j];
  }
}

// ---- backward A: per row tile; LDS per row: X [h w C], a1 [P1 F1], dz2 [NF], dz1 [P1 F1] ----
extern "C" __global__ void __launch_bounds__(256) aie_policy_conv_bwd_rows_kernel(const aie_conv_bwd_args B) {
  extern __shared__ float conv_lds[];
  const aie_conv_args& A = B.net;
  const aie_conv_shape& S = A.S;
  const int64_t row0 = (int64_t)blockIdx.x * A.tr;
  const int nrows = A.rows - row0 < A.tr ? (int)(A.rows - row0) : A.tr;
  const int hwC = S.hw * S.C, n1 = S.P1 * AIE_CONV_F1, NF = S.NF, nx = 2 * S.hw * S.D;
  conv_stage_input(A, row0, nrows, conv_lds);
  __syncthreads();
  conv_layer1(A, nrows, conv_lds);
  __syncthreads();
  for (int o = (int)threadIdx.x; o < nrows * NF; o += 256) {
    const int rl = o / NF, rem = o - rl * NF;
    float* L = conv_lds + rl * A.lds_row;
    const float a2 = aie_conv2_out(&S, L + hwC, A.w2, A.b2, rem / AIE_CONV_F2, rem % AIE_CONV_F2);
    const float d = a2 > 0.0f ? B.g_feat[(row0 + rl) * B.g_ld + rem] : 0.0f;
    L[hwC + n1 + rem] = d;
    B.dz2[(row0 + rl) * NF + rem] = d;
  }
  __syncthreads();
  for (int o = (int)threadIdx.x; o < nrows * n1; o += 256) {
    const int rl = o / n1, rem = o - rl * n1;
    float* L = conv_lds + rl * A.lds_row;
    const float a1 = L[hwC + rem];
    const float d = a1 > 0.0f ? aie_conv_da1(&S, L + hwC + n1, A.w2, rem / AIE_CONV_F1, rem % AIE_CONV_F1) : 0.0f;
    L[hwC + n1 + NF + rem] = d;
    B.a1[(row0 + rl) * n1 + rem] = a1;
    B.dz1[(row0 + rl) * n1 + rem] = d;
  }
  __syncthreads();
  const int D2 = 2 * S.D;
  for (int o = (int)threadIdx.x; o < nrows * nx; o += 256) {
    const int rl = o / nx, rem = o - rl * nx, cell = rem / D2, e = rem - cell * D2;  // e fastest: a cell's windows are shared
    const float* L = conv_lds + rl * A.lds_row;
    const int i = e / S.D, d = e - i * S.D;
    B.dxe[(row0 + rl) * nx + (i * S.hw + cell) * S.D + d] = aie_conv_dx(&S, L + hwC + n1 + NF, A.w1, cell, e);
  }
}

// ---- backward B: a segment's partials ----
extern "C" __global__ void __launch_bounds__(256) aie_policy_conv_bwd_seg_kernel(const aie_conv_bwd_args B) {
  extern __shared__ float conv_lds[];
  const aie_conv_args& A = B.net;
  const aie_conv_shape& S = A.S;
  const int per = B.chunks + 1;
  const int seg = (int)(blockIdx.x / (uint32_t)per), j = (int)(blockIdx.x % (uint32_t)per);
  const int64_t r0 = (int64_t)seg * AIE_MLP_BWD_SEG, r1 = r0 + AIE_MLP_BWD_SEG < A.rows ? r0 + AIE_MLP_BWD_SEG : A.rows;
  const int n1 = S.P1 * AIE_CONV_F1, NF = S.NF, nx = 2 * S.hw * S.D, VD = S.V * S.D;
  float* out = B.partial + (int64_t)seg * B.Pn;
  if (j < B.chunks) {  // 256 entries of the weights' two blocks, [(9 C + 1), F1] then [(9 F1 + 1), F2]
    const int e0 = j * 256 + (int)threadIdx.x;
    if (e0 >= B.off3) return;
    const int L = e0 >= B.off2, e = L ? e0 - B.off2 : e0;
    const int nf = L ? AIE_CONV_F2 : AIE_CONV_F1, sc = L ? AIE_CONV_F1 : S.C, P = L ? S.P2 : S.P1, ow = L ? S.ow2 : S.ow1,
              sw = L ? S.ow1 : S.w;
    const int k = e / nf, f = e - k * nf, bias = k == 9 * sc, t = bias ? 0 : k / sc, ky = t / 3, kx = t - 3 * ky, c = bias ? 0 : k - t * sc;
    const float* dz = L ? B.dz2 : B.dz1;
    const int dz_ld = P * nf;
    float acc = 0.0f;
    for (int64_t r = r0; r < r1; ++r) {
      const float* dr = dz + r * dz_ld + f;
      const float* map_r = A.map + r * A.map_ld;
      const int16_t* idx_r = A.idx + r * A.idx_ld;
      const float* a1_r = B.a1 + r * n1;
#pragma unroll 5
      for (int p = 0; p < P; ++p) {
        const int oy = p / ow, ox = p - oy * ow, cell = (2 * oy + ky) * sw + 2 * ox + kx;
        float a = 1.0f;
        if (!bias) a = L ? a1_r[cell * AIE_CONV_F1 + c] : aie_conv_input_at(&S, map_r, idx_r, A.emb, c, cell);
        acc = fmaf(a, dr[p * nf], acc);
      }
    }
    out[e0] = acc;
    return;
  }
  // the embedding: AIE_CONV_EMB_TILE rows' tables [V D] at a time; thread (rl, d) owns column d of row rl's table
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  const int tid = (int)threadIdx.x;
  for (int64_t t0 = r0; t0 < r1; t0 += AIE_CONV_EMB_TILE) {
    const int nt = r1 - t0 < AIE_CONV_EMB_TILE ? (int)(r1 - t0) : AIE_CONV_EMB_TILE;
    for (int o = tid; o < nt * VD; o += 256) conv_lds[o] = 0.0f;
    __syncthreads();
    if (tid < nt * S.D) {
      const int rl = tid / S.D, d = tid - rl * S.D;
      const int16_t* idx_r = A.idx + (t0 + rl) * A.idx_ld;
      const float* dx_r = B.dxe + (t0 + rl) * nx + d;
      float* tab = conv_lds + rl * VD + d;
      for (int ic = 0; ic < 2 * S.hw; ++ic) {
        float* w = tab + aie_conv_clamp(idx_r[ic], S.V) * S.D;
        *w = *w + dx_r[ic * S.D];
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = tid + 256 * q;
      if (e < VD)
        for (int rl = 0; rl < nt; ++rl) acc[q] = acc[q] + conv_lds[rl * VD + e];
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = tid + 256 * q;
    if (e < VD) out[B.off3 + e] = acc[q];
  }
}

// ---- backward C: an entry = its segments' partials added in float64, ascending, rounded once ----
extern "C" __global__ void __launch_bounds__(256) aie_policy_conv_bwd_reduce_kernel(const aie_conv_bwd_args B) {
  const aie_conv_shape& S = B.net.S;
  const int e = (int)(blockIdx.x * 256u + threadIdx.x), VD = S.V * S.D;
  if (e >= B.off3 + VD) return;
  double sum = 0.0;
  for (int s = 0; s < B.nseg; ++s) sum += (double)B.partial[(int64_t)s * B.Pn + e];
  const float v = (float)sum;
  const int nw1 = 9 * S.C * AIE_CONV_F1, nw2 = 9 * AIE_CONV_F1 * AIE_CONV_F2;
  if (e < nw1) B.gw1[e] = v;
  else if (e < B.off2) B.gb1[e - nw1] = v;
  else if (e < B.off2 + nw2) B.gw2[e - B.off2] = v;
  else if (e < B.off3) B.gb2[e - B.off2 - nw2] = v;
  else B.gemb[e - B.off3] = v;
}

// ---- the MLP's input gradient: g_x[r][j] = chain0 over k of (dz1[r][k], W1[j][k]) ----
// A workgroup stages AIE_IGRAD_TILE rows of dz1 in LDS; a thread owns column j and walks ALONG row j of the row-major w1,
// one weight read for the tile's rows (each its own accumulator: the rows are the independent chains that hide the latency).
extern "C" __global__ void __launch_bounds__(256) aie_policy_mlp_input_grad_kernel(const aie_mlp_igrad_args A) {
  extern __shared__ float conv_lds[];
  const bool ag = blockIdx.x < (uint32_t)A.agents.blocks;
  const aie_mlp_igrad_group& G = ag ? A.agents : A.planner;
  const int b = (int)(ag ? blockIdx.x : blockIdx.x - (uint32_t)A.agents.blocks);
  const int tile = b / G.cgroups, cg = b - tile * G.cgroups, H = G.H;
  const int64_t row0 = (int64_t)tile * AIE_IGRAD_TILE;
  const int nrows = G.rows - row0 < AIE_IGRAD_TILE ? (int)(G.rows - row0) : AIE_IGRAD_TILE;
  for (int o = (int)threadIdx.x; o < AIE_IGRAD_TILE * H; o += 256) conv_lds[o] = o < nrows * H ? G.dz1[row0 * H + o] : 0.0f;
  __syncthreads();
  const int j = cg * 256 + (int)threadIdx.x;
  if (j >= G.ncols) return;
  const float* wr = G.w1 + (int64_t)j * H;
  float acc[AIE_IGRAD_TILE];
#pragma unroll
  for (int r = 0; r < AIE_IGRAD_TILE; ++r) acc[r] = 0.0f;
  for (int k = 0; k < H; ++k) {
    const float w = wr[k];
#pragma unroll
    for (int r = 0; r < AIE_IGRAD_TILE; ++r) acc[r] = fmaf(conv_lds[r * H + k], w, acc[r]);
  }
#pragma unroll
  for (int r = 0; r < AIE_IGRAD_TILE; ++r)
    if (r < nrows) G.g_x[(row0 + r) * G.ld + j] = acc[r];
}
