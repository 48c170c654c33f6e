// aie_device.h -- the device library every kernel file is written against: Ctx and the LDS carve-up, the wave helpers
// and buffer stores, the record's way in and out, the generators (Philox, MT19937 in registers, the draw window, rng_*),
// the NumPy-order sums, the tax schedule, NextActions and the reward log's slot.  No kernel and nothing of one scenario
// belongs here: what only the gather-trade-build family uses is in aie_gtb_*.h and aie_kernels.hip.  Part of
// both run-time units (aie_jit.h): its hash is in every cached code object's key.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aie_layout.h"
#include "aie_glibc_math.h"

// Floating-point contraction is OFF for every kernel of this library: NumPy (and the C oracle) round a product before
// they add it, and state such as coin, labor and utilities has to come out bit for bit -- the sign of a ~1e-16 reward
// decides an integer state field (layout_from_file.py:553-557).  Fused multiply-adds appear only where libm itself
// fuses them (aie_glibc_math.h, written out with __builtin_fma).
#pragma clang fp contract(off)

// constant images of the parameter block: the build's compile-time instances (aie_spec_generated.h), or -- in a
// run-time specialisation (AIE_JIT, aie_specialize() in aie_capi.hip) -- the one image of the caller's environment
#ifdef AIE_JIT
#include "aie_jit_image.h"
#else
#include "aie_spec_generated.h"
#endif
template <int SPEC>
__device__ __forceinline__ const aie_params& aie_spec_params(const aie_params* run_time) {
  if constexpr (SPEC < 0) return *run_time;
  else return *reinterpret_cast<const aie_params*>(aie_spec_image<SPEC>::bytes);
}

#define AIE_NT 64  // threads per replica (one wavefront)
#define AIE_DIRTY_CAP 64  // map cells one step may change before the incremental map observations give up (= one lane each)
// (AIE_SRC_CAP, aie_layout.h: source-block doubles handled by the gather regen, else row regen)

namespace aie {

// NOTE: every __device__ function below is __forceinline__: a non-inlined call that takes
// `const aie_params&` forces the compiler to copy the whole by-value kernel argument
// (2.7 KB) to scratch memory on every launch -- measured 5x slower.

struct Ctx {
  const aie_params& P;  // everything a kernel needs; in the compile-time instances of the step kernel (aie_spec_generated.h)
                        // a CONSTANT image of the block, so that dims, offsets and component lists fold into the code
  const aie_params& R;  // the run-time block in device memory: what depends on the batch (E, arena offsets a_*)
  uint8_t* rec;      // LDS copy of the record (everything before the MT19937 key)
  int32_t* act_p;    // LDS [AIE_MAX_BRACKETS] decoded planner actions
  uint8_t* locmap;   // LDS [HW] 0 = empty, i+1 = agent i
  double* fscr;      // LDS f64 scratch
  float* stage;      // LDS staging of the small observation vectors (also: MT word dump during regen)
  int32_t* srcn;     // LDS [4] scratch words ([2]: the dense log's event rows of this step)
  int32_t* mflags;   // LDS [n] per-agent mask bits
  int32_t* dirty;    // LDS [4 + AIE_DIRTY_CAP/2]: count, moved-agent mask (2 words), pad, uint16 cell list
  uint8_t* snap;     // LDS [2][HW]: pre-step max(map, source block) per resource (P.regen_general only), else nullptr
  uint8_t* met;      // (one-step-economy: this replica's episode accumulators; everybody else: C_MET)
  uint8_t* met_arena;  // GLOBAL: the arena where the replica has episode accumulators (aie_layout.h: a_metrics), else nullptr
  int32_t* ev;       // GLOBAL: this replica's dense-log event rows (a_events), or nullptr (not logged)
  bool saez;         // tax_model == "saez" (compile-time false in the common step kernel, like ev == nullptr)
  bool full;         // compile-time: false in the common step kernel (aie_step_kernel), which leaves out what
                     // only some environments need -- dense-log rows, Saez hooks, order books larger than a
                     // wavefront, development hooks -- to keep its code small (the kernel does not fit the
                     // instruction cache, and rarely taken paths pay for every line they add)
  int tid;
  int e;
  const double* rtab;    // the discretised tax rates (aie_config.tax_disc_rates) and ...
  const uint32_t* mtab;  // ... the action-mask element tests (aie_params.mask_test): LDS copies in the step kernel where
                         // the LDS budget allows (const_tables_in_lds), else the parameter block's own arrays
  uint32_t* mtwin;   // LDS [640]: the generator's current window for the regeneration's sparse reads, or nullptr (mt_window_in_lds)
  int skipm;         // development (-DAIE_DEV builds: aie_dev_set_skip_mask): phases switched off; constant 0 otherwise
};

#define R_F64(c, off) (reinterpret_cast<double*>((c).rec + (c).P.off))
#define R_I32(c, off) (reinterpret_cast<int32_t*>((c).rec + (c).P.off))
#define R_U8(c, off) (reinterpret_cast<uint8_t*>((c).rec + (c).P.off))
#define R_CELLS(c) (reinterpret_cast<uint32_t*>((c).rec + (c).P.o_cells))

// f64 scratch slots: net price history [2][P], then four per-agent vectors
__device__ __forceinline__ double* scr_net_ph(const Ctx& c) { return c.fscr; }
__device__ __forceinline__ double* scr_sorted_inc(const Ctx& c) { return c.fscr + 2 * c.P.P; }
__device__ __forceinline__ double* scr_cmr(const Ctx& c) { return c.fscr + 2 * c.P.P + c.P.n; }
__device__ __forceinline__ double* scr_coin(const Ctx& c) { return c.fscr + 2 * c.P.P + 2 * c.P.n; }
__device__ __forceinline__ double* scr_part(const Ctx& c) { return c.fscr + 2 * c.P.P + 3 * c.P.n; }  // [n+1]
// sort buffer of the planner's gini (n >= 30): its own slot, because the rewards run on the
// second wave of a replica while the first one uses scr_sorted_inc for the tax observations
__device__ __forceinline__ double* scr_gini_sort(const Ctx& c) { return c.fscr + 2 * c.P.P + 4 * c.P.n + 2; }
__host__ __device__ inline int fscr_doubles(const aie_params& P) { return 2 * P.P + 5 * P.n + 2; }

// The LDS image of the record stops where the MT19937 key starts (it lives in VGPRs).  The counter stream's state
// (AIE_RNG_FAST: key32, block number, salt, 0 -- 16 bytes) is part of the image.
__host__ __device__ inline bool rng_fast(const aie_params& P) { return P.c.rng_mode == AIE_RNG_FAST; }
// One list of the regeneration's source doubles for the whole batch (aie_layout.h: aie__shared_src_list, a_src_list)
// instead of a scan of the cells' flag bytes in every step -- used in the counter-stream mode only: A/B on one box
// (tools/ab_variants.sh, round 5) C2f 22.35 -> 22.0 us, but C2 24.7 -> 25.4 us and C3 40.5 -> 40.7 us with MT19937, whose
// second wave already holds the generator's ten rows while the list's registers wait for the regeneration.
__host__ __device__ inline bool shared_src_list(const aie_params& P) {
#ifdef AIE_NO_SHARED_SRC_LIST  // (A/B builds)
  return false;
#endif
  return rng_fast(P) && P.c.scenario == AIE_SCN_GTB && P.c.shared_layout && P.c.layout_gen == AIE_LAYOUT_FIXED;
}
__host__ __device__ inline int rec_lds_bytes(const aie_params& P) { return P.o_mt + (rng_fast(P) ? 16 : 0); }

// staging area: the components' draw window (the next tempered MT19937 words, see MTL) and the small
// observation vectors the flat-vector writer stages
__host__ __device__ inline int pad4(int x) { return (x + 3) & ~3; }
__host__ __device__ inline int stage_window_words(const aie_params& P) {
  // words the components of one step draw at most in the common case: two agent-order permutations (n - 1 masked
  // rejection draws each, < 2 words per draw on average) and a pickup draw per agent and resource; a step that needs
  // more refills the window from the generator state in HBM (rng_refill)
  int w = (4 * P.n + 4 * P.n + 63) / 64 * 64;
  if (w < 128) w = 128;
  return w > 576 ? 576 : w;
}
__host__ __device__ inline size_t stage_bytes(const aie_params& P) {
  // [0, window): tempered words pos ... of the generator's current window (filled by the wave that holds the state);
  // behind it: the planner's flat vector + per-agent fragments (write_flat_observations)
  const size_t b = (size_t)(stage_window_words(P) + pad4(P.n * P.FPA) + pad4(P.FP)) * 4;
  return (b + 15) / 16 * 16;
}

__host__ __device__ inline size_t lds_bytes_base(const aie_params& P) {
  size_t b = (size_t)rec_lds_bytes(P);
  b += AIE_MAX_BRACKETS * 4;
  b = (b + 15) / 16 * 16;
  b += ((size_t)P.HW + 15) / 16 * 16;
  b += (size_t)fscr_doubles(P) * 8;
  b += stage_bytes(P);
  b += 16 + (size_t)pad4(P.n) * 4;  // (the source list is part of the record image since round 6)
  b += 16 + AIE_DIRTY_CAP * 2;
  b = (b + 15) / 16 * 16;
  return b;
}
// The regeneration reads ~80 of a step's 2 500 generator words, scattered over five consecutive windows.  Where a
// workgroup's LDS footprint leaves room for it WITHOUT costing residency (16 workgroups per CU need <= 10 240 B each),
// the second wave publishes each window's ten rows to LDS (ten stores) and every lane fetches its two adjacent words
// with one ds_read2 -- instead of selecting them out of the row registers with ten lane permutes and ten selects per
// word (scenario_step_regen).  Larger records (ten agents and more) keep the register gather.
#define AIE_MT_WINDOW_LDS_BYTES 2560  // 10 rows x 64 lanes x 4 B (row 9's upper 16 lanes are padding)
// Two small tables of the parameter block are indexed with run-time values on the replica's critical path: the
// discretised tax rates (by the planner's latched rate indices: every marginal-rate / tax-due evaluation and the
// curr_rates observation) and the per-element tests of the flattened action mask.  In a compile-time instance the
// block is a constant image in device memory, so each such lookup is a global (or scalar) memory round trip behind the
// LDS read of its index.  The step kernel's second wave copies both tables to LDS while the record streams in --
// where that does not cost residency, like the generator's window below (which takes what room is left).
__host__ __device__ inline size_t const_table_bytes(const aie_params& P) {
  const size_t r = (P.has_tax && P.c.tax_model == AIE_TAX_MODEL_WRAPPER) ? (size_t)P.c.tax_n_disc_rates * 8 : 0;
  return (r + (size_t)P.MA * 4 + 15) / 16 * 16;
}
__host__ __device__ inline bool const_tables_in_lds(const aie_params& P) {
#ifdef AIE_NO_CONST_TABLES_LDS  // (A/B builds)
  return false;
#else
  return lds_bytes_base(P) + const_table_bytes(P) <= 10240;
#endif
}
__host__ __device__ inline bool mt_window_in_lds(const aie_params& P) {
#ifdef AIE_NO_MT_WINDOW_LDS  // (A/B builds)
  return false;
#else
  return !P.regen_general && !rng_fast(P) &&  // (the counter stream addresses its words directly)
         lds_bytes_base(P) + (const_tables_in_lds(P) ? const_table_bytes(P) : 0) + AIE_MT_WINDOW_LDS_BYTES <= 10240;
#endif
}
__host__ __device__ inline size_t lds_bytes(const aie_params& P) {
  size_t b = lds_bytes_base(P);
  if (const_tables_in_lds(P)) b += const_table_bytes(P);
  if (mt_window_in_lds(P)) b += AIE_MT_WINDOW_LDS_BYTES;
  if (P.regen_general) b += 2 * (((size_t)P.HW + 15) / 16 * 16);
  return (b + 15) / 16 * 16;
}

// the accumulators' address where it is used (rarely: a trade, a tax day) instead of in every prologue: a_metrics was a
// scalar load ahead of the step kernel's first record load (0.2 us of the launch, round 6)
#define C_MET(c) ((c).met_arena ? (c).met_arena + (c).R.a_metrics + (int64_t)(c).e * (c).P.met_bytes : nullptr)
__device__ __forceinline__ Ctx make_ctx(const aie_params& P, const aie_params& R, uint8_t* lds, int e, int tid,
                                        uint8_t* arena = nullptr, bool with_events = true, int skipm = 0,
                                        bool lds_tables = false) {
  uint8_t* q = lds + rec_lds_bytes(P);
  int32_t* act_p = reinterpret_cast<int32_t*>(q);
  q += AIE_MAX_BRACKETS * 4;
  q = lds + ((q - lds) + 15) / 16 * 16;
  uint8_t* locmap = q;
  q += (P.HW + 15) / 16 * 16;
  double* fscr = reinterpret_cast<double*>(q);
  q += fscr_doubles(P) * 8;
  float* stage = reinterpret_cast<float*>(q);
  q += stage_bytes(P);
  int32_t* srcn = reinterpret_cast<int32_t*>(q);
  q += 16;
  int32_t* mflags = reinterpret_cast<int32_t*>(q);
  q += pad4(P.n) * 4;
  int32_t* dirty = reinterpret_cast<int32_t*>(q);
  q += 16 + AIE_DIRTY_CAP * 2;
  q = lds + ((q - lds) + 15) / 16 * 16;
  // (the kernel that asks for the LDS tables fills them: step_body; everyone else reads the parameter block)
  const double* rtab = R.c.tax_disc_rates;
  const uint32_t* mtab = P.mask_test;
  if (const_tables_in_lds(P)) {
    if (lds_tables) {
      const bool rates = P.has_tax && P.c.tax_model == AIE_TAX_MODEL_WRAPPER;
      rtab = reinterpret_cast<const double*>(q);
      mtab = reinterpret_cast<const uint32_t*>(q + (rates ? P.c.tax_n_disc_rates * 8 : 0));
    }
    q += const_table_bytes(P);
  }
  uint32_t* mtwin = mt_window_in_lds(P) ? reinterpret_cast<uint32_t*>(q) : nullptr;
  if (mt_window_in_lds(P)) q += AIE_MT_WINDOW_LDS_BYTES;
  uint8_t* snap = P.regen_general ? q : nullptr;
  uint8_t* met = nullptr;  // (C_MET)
  // with_events == false is a compile-time constant in the common step kernel: every `if (c.ev)` / `if (c.saez)`
  // folds away (environments with dense-log replicas or tax_model "saez" run aie_step_kernel_log)
  int32_t* ev = (with_events && arena && e < R.ev_replicas)  // (the event buffer is a property of the batch, not of an
                    ? reinterpret_cast<int32_t*>(arena + R.a_events + (int64_t)e * R.ev_stride) : nullptr;  // instance's family)
  const bool saez = with_events && P.c.tax_model == AIE_TAX_SAEZ;
  return Ctx{P, R, lds, act_p, locmap, fscr, stage, srcn, mflags, dirty, snap, met, arena, ev, saez, with_events, tid, e, rtab, mtab, mtwin, skipm};
}

// ------------------------------------------------------------------------------------
// wave helpers
// ------------------------------------------------------------------------------------
// Ordering point inside a section that ONE wavefront executes (every __device__ function
// below is such a section: lane loops stride by AIE_NT = 64).  LDS instructions of a wave are
// issued and executed in order, so a later ds_read of any lane sees an earlier ds_write of any
// other lane of the same wave; what is needed is that the compiler keeps that order.  Block-
// level barriers (__syncthreads) only appear in the kernels, between sections that different
// waves of a replica's workgroup execute.
#define AIE_WSYNC() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int bcast(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ uint32_t bcast(uint32_t v, int lane) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}
__device__ __forceinline__ double bcast(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}
// Buffer-descriptor stores: base + num_records in 4 SGPRs, a 32-bit VGPR byte offset and a
// scalar byte offset per instruction (gfx9 raw buffer, DATA_FORMAT = 32 in word 3).
typedef __amdgpu_buffer_rsrc_t BufRsrc;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
// (base and size are wave-uniform at every call site.  They go through v_readfirstlane -- free for a value that already
// sits in scalar registers -- because a descriptor the instruction selector happened to build in vector registers makes
// EVERY store through it a "waterfall" loop over its distinct values: round 6 met that when the kernels' first address
// computations moved, +900 vector instructions in one instance.)
__device__ __forceinline__ BufRsrc make_rsrc(void* base, uint32_t bytes) {
  const uint64_t b = reinterpret_cast<uint64_t>(base);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b >> 32));
  return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>((uint64_t)lo | ((uint64_t)hi << 32)), 0,
                                           __builtin_amdgcn_readfirstlane((int)bytes), 0x00020000);
}
__device__ __forceinline__ void buf_store_f32(BufRsrc r, float v, int voff, int soff) {
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, voff, soff, 0);
}
__device__ __forceinline__ void buf_store_i16(BufRsrc r, int v, int voff, int soff) {
  __builtin_amdgcn_raw_buffer_store_b16((unsigned short)v, r, voff, soff, 0);
}
__device__ __forceinline__ void buf_store_u32x2(BufRsrc r, uint32_t a, uint32_t b, int voff, int soff) {
  const u32x2 v = {a, b};
  __builtin_amdgcn_raw_buffer_store_b64(v, r, voff, soff, 0);
}
// 16-byte buffer stores never carry a scalar offset REGISTER: measured on MI355X (round 3), `buffer_store_dwordx4
// v[6:9], v25, s[8:11], s7 offen` followed directly by `v_mov_b32 v6, 2` stored the 2 in lanes 12-15 of every 16 --
// the ">64-bit store data, then VALU write of those VGPRs" hazard exists on this part with an SGPR soffset too, while
// the compiler (ROCm 7.2 clang, GCNHazardRecognizer::createsVALUHazard) only spaces the pair out when soffset is an
// immediate.  With the offset folded into the vector offset and soffset = 0 the compiler inserts the wait state.
// (tests/test_gpu_parity.py::test_reset_is_deterministic_across_environments is the check that found it.)
__device__ __forceinline__ void buf_store_f32x4(BufRsrc r, float a, float b, float c, float d, int voff, int soff) {
  const u32x4 v = {__float_as_uint(a), __float_as_uint(b), __float_as_uint(c), __float_as_uint(d)};
  __builtin_amdgcn_raw_buffer_store_b128(v, r, voff + soff, 0, 0);
}
// 16 bytes, write-through (aux 16 = sc1: `buffer_store_dwordx4 ... sc1`): the line leaves the XCD's L2 with the store
// instead of staying dirty until the end of the launch, whose write-back the next launch on the stream waits for.  For
// bytes that nothing in the launch reads again, and for 16-byte stores ONLY: a narrower sc1 store is one fabric write
// each, 2.7 (8 bytes) to 6 times (4 bytes) the time per byte.  No scalar offset register (buf_store_f32x4).
// It pays in the middle of a wave's work, not as its last act: the generator's rows gain 0.40 us per launch of BASELINE
// configs[1] (store_generator_rows), the record image behind the last barrier LOSES 0.09 us on its own and stays plain
// (profiles/record_write_through_ab.txt).
__device__ __forceinline__ void buf_store_u32x4_wt(BufRsrc r, uint4 v, int voff) {
  const u32x4 d = {v.x, v.y, v.z, v.w};
  __builtin_amdgcn_raw_buffer_store_b128(d, r, voff, 0, 16);
}
// 16 bytes with dword alignment: global dwordx4 accesses need no more on gfx950
struct __attribute__((packed, aligned(4))) f32x4_a4 { float x, y, z, w; };

// LDS (16-byte aligned) -> global (dword aligned) copy of `count` floats
__device__ __forceinline__ void stream_out(const float* __restrict__ lds_src, float* __restrict__ dst, int count, int tid) {
  const int n4 = count >> 2;
  for (int q = tid; q < n4; q += AIE_NT) {
    const float4 v = reinterpret_cast<const float4*>(lds_src)[q];
    f32x4_a4 o = {v.x, v.y, v.z, v.w};
    reinterpret_cast<f32x4_a4*>(dst)[q] = o;
  }
  for (int q = 4 * n4 + tid; q < count; q += AIE_NT) dst[q] = lds_src[q];
}

// q / d for a run-time constant d with host-computed magic (aie_layout.h: aie__magic)
__device__ __forceinline__ int udiv(int q, int d, uint32_t magic) {
  return d == 1 ? q : (int)__umulhi((uint32_t)q, magic);
}
// XCD-aware workgroup -> replica mapping.  The dispatcher places workgroup b on XCD b % 8
// (observed, used for speed only): give every XCD a CONTIGUOUS range of replicas so that
// the 128-byte lines shared by neighbouring replicas in the env-major tensors (rewards,
// done, flat vectors whose per-replica size is not a multiple of 128 B) are completed
// inside one L2 instead of being written back as partial lines by two of them.
__device__ __forceinline__ int replica_of_block(int b, int E) {
  if (E & 7) return b;
  return (b & 7) * (E >> 3) + (b >> 3);
}
__device__ __forceinline__ uint64_t lanemask_lt(int lane) { return (1ull << lane) - 1ull; }

// One action slot j of replica e under the benchmark's uniform random policy (slots: the
// agents' sub-actions in order, then the planner's).
__device__ __forceinline__ void sample_action_slot(const aie_params& P, uint64_t seed, int64_t env_offset, int64_t t,
                                                   int e, int j, int32_t* __restrict__ act_a,
                                                   int32_t* __restrict__ act_p) {
  const uint32_t u = aie_counter_rng(seed, (uint64_t)(env_offset + e), (uint64_t)t, (uint64_t)j);
  if (j < P.n * P.act_a_width) {
    if (!act_a) return;
    int range;
    if (P.c.multi_action_mode_agents) range = P.n_sub_a ? P.sub_a_dim[j % P.act_a_width] + 1 : 1;
    else range = P.A;
    act_a[(int64_t)e * P.n * P.act_a_width + j] = (int32_t)(((uint64_t)u * (uint64_t)range) >> 32);
  } else {
    if (!act_p) return;
    const int range = P.c.multi_action_mode_planner ? P.p_row_dim + 1 : P.AP;  // (rows of one length: aie_sampler_check)
    act_p[(int64_t)e * P.act_p_width + (j - P.n * P.act_a_width)] = (int32_t)(((uint64_t)u * (uint64_t)range) >> 32);
  }
}

// ------------------------------------------------------------------------------------
// record streaming HBM <-> LDS (16 B per lane, fully coalesced); MT key HBM <-> VGPRs
// ------------------------------------------------------------------------------------
struct MT {
  uint32_t r[10];  // word 64*j + lane (row 9: lanes 0..47)
  int pos;         // wave-uniform index of the next unused word (624 = twist first)
  int twists;      // mt_twist calls since the owner zeroed it (one-step-economy: the rows go back to HBM only then)
  // AIE_RNG_FAST (include/aie.h): the stream is Philox2x32-10 keyed per replica, consumed in blocks of 624 words with
  // the same position bookkeeping; `r` then holds the FINAL words of block `fblk` (no tempering), "twist" = next block
  bool fast;       // (a compile-time constant in the instances: P.c.rng_mode folds)
  uint32_t fkey, fblk, fsalt;  // wave-uniform
};
#define R_U32(c, off) (reinterpret_cast<uint32_t*>((c).rec + (c).P.off))

// ---- AIE_RNG_FAST: Philox2x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11;
// multiplier and Weyl key increment of Random123).  Word g of a replica's stream = element g & 1 of
// philox(counter = (lo32(g >> 1), hi32(g >> 1) | salt), key32).  One 32 x 32 -> 64 multiply and one three-input xor
// per round.
__device__ __forceinline__ void philox2x32_10(uint32_t c0, uint32_t c1, uint32_t key, uint32_t& o0, uint32_t& o1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p = (uint64_t)0xD256D193u * (uint64_t)c0;
    c0 = (uint32_t)(p >> 32) ^ key ^ c1;
    c1 = (uint32_t)p;
    key += 0x9E3779B9u;
  }
  o0 = c0;
  o1 = c1;
}
// words 2 h and 2 h + 1 of block `blk` (h may run past the block's 312 pairs: the stream is linear, block b starts at
// pair 312 b)
__device__ __forceinline__ void fast_pair(uint32_t key, uint32_t blk, uint32_t salt, int h, uint32_t& o0, uint32_t& o1) {
  const uint64_t pair = (uint64_t)blk * 312ull + (uint64_t)(uint32_t)h;
  philox2x32_10((uint32_t)pair, (uint32_t)(pair >> 32) | salt, key, o0, o1);
}

// (Until round 5 this copy also scanned the cells' flag bytes for the regeneration's source doubles, every step: 250 of a
// replica-step's 2 150 vector instructions on BASELINE configs[1].  The list is a record field now, o_src_list, kept by
// the reset kernel.)
// `wave` of `nwaves` copies every nwaves-th 16-byte unit; wave `key_wave` also takes the MT19937 key (registers).
__device__ __forceinline__ void load_record(const Ctx& c, const uint8_t* __restrict__ arena, MT& m, int wave = 0,
                                            int nwaves = 1, int key_wave = 0) {
  // (a_records == 0: the records open the arena, aie_layout.h -- not read from the parameter block: every scalar load a
  // workgroup needs before its first record load costs the launch 0.2 - 0.3 us, round 6)
  const uint8_t* g = arena + (int64_t)c.e * c.P.rec_bytes;
  const uint4* src = reinterpret_cast<const uint4*>(g);
  uint4* dst = reinterpret_cast<uint4*>(c.rec);
  const int nq = rec_lds_bytes(c.P) >> 4;
  for (int q = wave * AIE_NT + c.tid; q < nq; q += nwaves * AIE_NT) dst[q] = src[q];
  if (wave != key_wave || rng_fast(c.P)) return;  // (the counter stream's state came with the image: mt_fast_attach)
  const uint32_t* key = reinterpret_cast<const uint32_t*>(g + c.P.o_mt);
#pragma unroll
  for (int j = 0; j < 9; ++j) m.r[j] = key[64 * j + c.tid];
  m.r[9] = c.tid < 48 ? key[576 + c.tid] : 0u;
}
__device__ __forceinline__ void store_record(const Ctx& c, uint8_t* __restrict__ arena, const MT& m, int wave = 0,
                                             int nwaves = 1, int key_wave = 0) {
  uint8_t* g = arena + (int64_t)c.e * c.P.rec_bytes;  // (a_records == 0, see load_record)
  uint4* dst = reinterpret_cast<uint4*>(g);
  const uint4* src = reinterpret_cast<const uint4*>(c.rec);
  const int nq = rec_lds_bytes(c.P) >> 4;
  for (int q = wave * AIE_NT + c.tid; q < nq; q += nwaves * AIE_NT) dst[q] = src[q];
  if (wave != key_wave || rng_fast(c.P)) return;  // the generator's rows are in that wave's registers
  uint32_t* key = reinterpret_cast<uint32_t*>(g + c.P.o_mt);
#pragma unroll
  for (int j = 0; j < 9; ++j) key[64 * j + c.tid] = m.r[j];
  if (c.tid < 48) key[576 + c.tid] = m.r[9];
}
// The step kernel's second wave, behind the regeneration.  `from_window`: the LDS window holds the rows (the result of
// scenario_step_regen) -- 624 words are 156 16-byte units and o_mt is 16-byte aligned, so a lane sends three units,
// write-through (buf_store_u32x4_wt: nothing in the launch reads the rows again) where it sent ten dwords; the
// descriptor ends with word 623, the source count starts right behind it.  Everyone else -- the row-by-row
// regeneration, a skipped regeneration, records without the window -- keeps the ten dword stores, and those stay plain.
// (One MI355X, BASELINE configs[1] at 4096 replicas: 18.87 -> 18.47 us per launch; the same three stores WITHOUT the
// write-through bit 18.85 -- the width alone is nothing, the 2.5 KB per replica that no longer wait dirty in L2 for the
// end of the launch are the gain.)
__device__ __forceinline__ void store_generator_rows(const Ctx& c, uint8_t* __restrict__ arena, const MT& m,
                                                     bool from_window = false) {
  if (rng_fast(c.P)) return;
  if (from_window && c.mtwin) {
    const BufRsrc rows = make_rsrc(arena + (int64_t)c.e * c.P.rec_bytes + c.P.o_mt, AIE_MT_N * 4);
    const uint4* win = reinterpret_cast<const uint4*>(c.mtwin);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int q = k * AIE_NT + c.tid;
      if (q < AIE_MT_N / 4) buf_store_u32x4_wt(rows, win[q], q << 4);
    }
    return;
  }
  uint32_t* key = reinterpret_cast<uint32_t*>(arena + (int64_t)c.e * c.P.rec_bytes + c.P.o_mt);
#pragma unroll
  for (int j = 0; j < 9; ++j) key[64 * j + c.tid] = m.r[j];
  if (c.tid < 48) key[576 + c.tid] = m.r[9];
}

// ------------------------------------------------------------------------------------
// NumPy legacy RandomState stream (MT19937), one per replica.
// The reference draws from the process-global np.random (F/base/base_env.py:493,
// F/base/world.py:420, F/components/move.py:138, layout_from_file.py:361-366,400).
// ------------------------------------------------------------------------------------
// one word of the twist: y = (a & UPPER) | (b & LOWER); m ^ (y >> 1) ^ (y & 1 ? MATRIX_A : 0) -- five VALU operations
// (bit-field insert, shift, sign-extended bit 0, one three-input bit operation, xor); the compiler's own selection of
// the plain C expression takes seven, and the twist is a third of the step kernel's vector instructions
__device__ __forceinline__ uint32_t mt_mix(uint32_t a, uint32_t b, uint32_t m) {
  uint32_t y;
  asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(y) : "s"(0x7fffffffu), "v"(b), "v"(a));  // (b & mask) | (a & ~mask)
  const uint32_t low = (uint32_t)__builtin_amdgcn_sbfe((int)b, 0, 1);           // y & 1 ? 0xffffffff : 0
  return __builtin_amdgcn_bitop3_b32(low, 0x9908b0dfu, y >> 1, 0x6a) ^ m;        // ((low & MATRIX_A) ^ (y >> 1)) ^ m
}
__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
  y ^= (y >> 11);
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= (y >> 18);
  return y;
}
__device__ __forceinline__ uint32_t lane_get(uint32_t v, int src_lane) { return (uint32_t)__shfl((int)v, src_lane, 64); }

// Whole-state twist in registers.  Word k = 64*J + l of the next state needs words k,
// k+1 and k+397 (mod 624, with the sequential in-place semantics: indices that wrap
// refer to ALREADY UPDATED words).  k+397 = 64*(J+6) + l+13 and k-227 = 64*(J-4) + l+29,
// so every row is two lane rotations (by 13 or by 29) of two other rows.
// The two source rows of a row feed DISJOINT source lanes (l < SPLIT reads lanes [ROT, 64) of ROW_LO, the rest
// lanes [0, ROT) of ROW_HI), so they are merged per source lane first and fetched with one permute; the
// neighbour word k+1 is a one-lane wave rotation (DPP), with the last lane patched from the next row.
__device__ __forceinline__ uint32_t lane_rol1(uint32_t v) {  // lane l <- lane (l + 1) & 63
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x134 /* wave_rol:1 */, 0xf, 0xf, false);
}
// lane l <- lane l + 1 of `v`, lane LAST <- the (wave-uniform) first word of the next row.  LAST == 63: ONE DPP move --
// a wavefront shift leaves the last lane, which has no source, at the destination's previous value (bound_ctrl off);
// a select on `lane == 63` compiles to a branch around a move
template <int LAST>
__device__ __forceinline__ uint32_t lane_next_word(uint32_t v, uint32_t next0, int lane) {
  if (LAST == 63) return (uint32_t)__builtin_amdgcn_update_dpp((int)next0, (int)v, 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
  const uint32_t b = lane_rol1(v);
  return (lane == LAST) ? next0 : b;
}
#define AIE_MT_ROW(J, ROT, SPLIT, ROW_LO, ROW_HI, NEXT0)                                      \
  {                                                                                          \
    const uint32_t a = m.r[J];                                                               \
    const uint32_t b = lane_next_word<(J) == 9 ? 47 : 63>(a, (NEXT0), lane);                 \
    const uint32_t src = lane >= (ROT) ? (ROW_LO) : (ROW_HI);                                \
    const uint32_t x = lane_get(src, (lane + (ROT)) & 63);                                   \
    m.r[J] = mt_mix(a, b, x);                                                                \
  }
__device__ __forceinline__ void mt_twist_body(MT& m, int lane) {
  // rows 0..2: old[k+397] from rows J+6 (l < 51) / J+7 (l >= 51), rotation 13
  AIE_MT_ROW(0, 13, 51, m.r[6], m.r[7], bcast(m.r[1], 0))
  AIE_MT_ROW(1, 13, 51, m.r[7], m.r[8], bcast(m.r[2], 0))
  AIE_MT_ROW(2, 13, 51, m.r[8], m.r[9], bcast(m.r[3], 0))
  {  // row 3: l < 35 old row 9 (rotation 13), l >= 35 NEW row 0 (rotation 29)
    const uint32_t a = m.r[3];
    const uint32_t b = lane_next_word<63>(a, bcast(m.r[4], 0), lane);
    const uint32_t x_lo = lane_get(m.r[9], (lane + 13) & 63);
    const uint32_t x_hi = lane_get(m.r[0], (lane + 29) & 63);
    m.r[3] = mt_mix(a, b, lane < 35 ? x_lo : x_hi);
  }
  // rows 4..9: NEW[k-227] from rows J-4 (l < 35) / J-3 (l >= 35), rotation 29
  AIE_MT_ROW(4, 29, 35, m.r[0], m.r[1], bcast(m.r[5], 0))
  AIE_MT_ROW(5, 29, 35, m.r[1], m.r[2], bcast(m.r[6], 0))
  AIE_MT_ROW(6, 29, 35, m.r[2], m.r[3], bcast(m.r[7], 0))
  AIE_MT_ROW(7, 29, 35, m.r[3], m.r[4], bcast(m.r[8], 0))
  AIE_MT_ROW(8, 29, 35, m.r[4], m.r[5], bcast(m.r[9], 0))
  AIE_MT_ROW(9, 29, 35, m.r[5], m.r[6], bcast(m.r[0], 0))  // word 623 pairs with NEW word 0
}

// One out-of-line copy of the twist (rows travel in VGPRs by value): it is reached from
// every draw site, and inlining ~150 instructions x 8 sites would overflow the I-cache.
struct MTRows { uint32_t r[10]; };
__device__ __attribute__((noinline)) MTRows mt_twist_rows(MTRows in, int lane) {
  MT m;
  m.fast = false;
#pragma unroll
  for (int j = 0; j < 10; ++j) m.r[j] = in.r[j];
  m.pos = 0;
  mt_twist_body(m, lane);
  MTRows out;
#pragma unroll
  for (int j = 0; j < 10; ++j) out.r[j] = m.r[j];
  return out;
}
// AIE_RNG_FAST: the 624 words of block m.fblk in the row layout (word 64 J + l in r[J], lane l).  Lane l computes the
// pairs 64 j + l (j = 0..4: words 128 j + 2 l, + 1); row 2 j takes its words from lanes l >> 1, row 2 j + 1 from lanes
// 32 + (l >> 1).  Five Philox blocks and twenty lane permutes per 624 words: costlier than an MT19937 twist (the
// sequential consumers -- resets, layout generation -- pay that; the step kernel never comes here, it addresses the
// words it needs directly).
__device__ __attribute__((noinline)) MTRows mt_fast_rows_of(uint32_t key, uint32_t blk, uint32_t salt, int lane) {
  MTRows out;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    uint32_t x0, x1;
    fast_pair(key, blk, salt, 64 * j + lane, x0, x1);
    const uint32_t lo0 = lane_get(x0, lane >> 1), lo1 = lane_get(x1, lane >> 1);
    const uint32_t hi0 = lane_get(x0, 32 + (lane >> 1)), hi1 = lane_get(x1, 32 + (lane >> 1));
    out.r[2 * j] = (lane & 1) ? lo1 : lo0;
    out.r[2 * j + 1] = (lane & 1) ? hi1 : hi0;
  }
  return out;
}
__device__ __forceinline__ void mt_fast_rows(MT& m, int lane) {
  const MTRows t = mt_fast_rows_of(m.fkey, m.fblk, m.fsalt, lane);
#pragma unroll
  for (int j = 0; j < 10; ++j) m.r[j] = t.r[j];
}
__device__ __forceinline__ void mt_twist(MT& m, int lane) {
  if (m.fast) {
    m.fblk += 1;
    mt_fast_rows(m, lane);
    m.twists += 1;
    return;
  }
  MTRows t;
#pragma unroll
  for (int j = 0; j < 10; ++j) t.r[j] = m.r[j];
  t = mt_twist_rows(t, lane);
#pragma unroll
  for (int j = 0; j < 10; ++j) m.r[j] = t.r[j];
  m.twists += 1;
}

// a row register's value as the stream's word: MT19937 tempers its state words, the counter stream's rows are final
__device__ __forceinline__ uint32_t mt_word(const MT& m, uint32_t raw) { return m.fast ? raw : mt_temper(raw); }
// A generator for a kernel section: MT19937 (rows arrive with load_record) or the counter stream (mt_fast_attach once the
// record is in LDS).
__device__ __forceinline__ void mt_init(MT& m, const aie_params& P) {
  m.fast = rng_fast(P);
  m.pos = AIE_MT_N;
  m.twists = 0;
  m.fkey = m.fblk = m.fsalt = 0u;
}
__device__ __forceinline__ void mt_copy(MT& d, const MT& s) {  // (rows and, for the counter stream, which block they are)
#pragma unroll
  for (int j = 0; j < 10; ++j) d.r[j] = s.r[j];
  d.fast = s.fast;
  d.fkey = s.fkey;
  d.fblk = s.fblk;
  d.fsalt = s.fsalt;
  d.twists = s.twists;
}
// AIE_RNG_FAST, once the record is in LDS and m.pos is set: the stream's identity from the image, and the current
// block's rows if words of it are still to come (pos == 624: the next draw starts a block anyway).  detach: the block
// number goes back into the image (every lane stores the same value).
__device__ __forceinline__ void mt_fast_attach(const Ctx& c, MT& m) {
  if (!m.fast) return;
  const uint32_t* st = R_U32(c, o_mt);
  m.fkey = (uint32_t)uni((int)st[0]);
  m.fblk = (uint32_t)uni((int)st[1]);
  m.fsalt = (uint32_t)uni((int)st[2]);
  if (m.pos < AIE_MT_N) mt_fast_rows(m, c.tid & (AIE_NT - 1));
}
__device__ __forceinline__ void mt_fast_detach(const Ctx& c, const MT& m) {
  if (m.fast) R_U32(c, o_mt)[1] = m.fblk;
}
// sequential draws (wave-uniform: every lane gets the same value)
__device__ __forceinline__ uint32_t rng_u32(MT& m, int lane) {
  if (m.pos >= AIE_MT_N) {
    mt_twist(m, lane);
    m.pos = 0;
  }
  const int row = m.pos >> 6;
  uint32_t v = m.r[0];
#pragma unroll
  for (int j = 1; j < 10; ++j) v = (row == j) ? m.r[j] : v;
  const uint32_t w = bcast(v, m.pos & 63);
  m.pos += 1;
  return mt_word(m, w);
}
__device__ __forceinline__ double u53(uint32_t a, uint32_t b) {
  return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}

// numpy float64 add.reduce over n <= 128 contiguous values (pairwise summation with an
// 8-way unrolled head, numpy/_core/src/umath/loops_utils.h.src): decisions such as
// "mean agent reward > 0" (layout_from_file.py:554-557) depend on this exact order.
__device__ __forceinline__ double np_sum_small(const double* a, int n) {
  if (n < 8) {
    double res = -0.0;
    for (int i = 0; i < n; ++i) res += a[i];
    return res;
  }
  double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
    r0 += a[i + 0]; r1 += a[i + 1]; r2 += a[i + 2]; r3 += a[i + 3];
    r4 += a[i + 4]; r5 += a[i + 5]; r6 += a[i + 6]; r7 += a[i + 7];
  }
  double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < n; ++i) res += a[i];
  return res;
}

// The same reduction over sequences of up to 1024 elements that are not stored anywhere, evaluated by the whole wave:
// element idx is a[idx] (mode 0) or |a[idx / n] - a[idx % n]| (mode 1: the flattened n x n matrix
// np.abs(endowments[:, None] - endowments[None, :]) of social_metrics.get_gini, social_metrics.py:36-41).
// Lanes 0..7 carry numpy's eight accumulators; blocks above 128 elements split as numpy's recursion does.
// M = 65536 / n + 1 (exact idx / n for idx < 2259 and n <= 29).  The result is wave-uniform.
__device__ __forceinline__ double np_seq_elem(const double* a, int n, int mode, uint32_t M, int idx) {
  if (mode == 0) return a[idx];
  const int r = (int)(((uint32_t)idx * M) >> 16);
  return fabs(a[r] - a[idx - r * n]);
}
__device__ __attribute__((noinline)) double np_sum_leaf(const double* a, int n, int mode, uint32_t M, int o, int m,
                                                        int lane) {
  if (m < 8) {
    double res = -0.0;
    for (int i = 0; i < m; ++i) res += np_seq_elem(a, n, mode, M, o + i);
    return res;
  }
  const int k = lane & 7, body = m - (m % 8);
  double r = np_seq_elem(a, n, mode, M, o + k);
  for (int i = 8; i < body; i += 8) r += np_seq_elem(a, n, mode, M, o + i + k);
  const double r0 = bcast(r, 0), r1 = bcast(r, 1), r2 = bcast(r, 2), r3 = bcast(r, 3);
  const double r4 = bcast(r, 4), r5 = bcast(r, 5), r6 = bcast(r, 6), r7 = bcast(r, 7);
  double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (int i = body; i < m; ++i) res += np_seq_elem(a, n, mode, M, o + i);
  return res;
}
template <int D>
__device__ __forceinline__ double np_sum_seq(const double* a, int n, int mode, uint32_t M, int o, int m, int lane) {
  if constexpr (D == 0) {
    return np_sum_leaf(a, n, mode, M, o, m, lane);
  } else {
    if (m <= 128) return np_sum_leaf(a, n, mode, M, o, m, lane);
    int n2 = m / 2;
    n2 -= n2 % 8;
    const double lo = np_sum_seq<D - 1>(a, n, mode, M, o, n2, lane);
    return lo + np_sum_seq<D - 1>(a, n, mode, M, o + n2, m - n2, lane);
  }
}

__device__ __forceinline__ double rng_double(MT& m, int lane) {
  const uint32_t a = rng_u32(m, lane);
  const uint32_t b = rng_u32(m, lane);
  return u53(a, b);
}
// random_interval(max): masked rejection on 32-bit words
__device__ __forceinline__ uint32_t rng_interval(MT& m, int lane, uint32_t max) {
  if (max == 0) return 0;
  uint32_t mask = max, v;
  mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
  while ((v = (rng_u32(m, lane) & mask)) > max) {}
  return v;
}
// np.random.permutation(n): World.get_random_order_agents, F/base/world.py:418-422.
// Returned lane-distributed: lane k holds the k-th agent of the random order.
__device__ __forceinline__ int rng_permutation(MT& m, int lane, int n) {
  int p = lane;
  for (int i = n - 1; i >= 1; --i) {
    const int j = (int)rng_interval(m, lane, (uint32_t)i);
    const int vi = bcast(p, i), vj = bcast(p, j);
    p = (lane == i) ? vj : ((lane == j) ? vi : p);
  }
  return p;
}
// ---- the same draws for the step kernel's components.  The generator state (624 words) never enters LDS: the
// wave that regenerates the resources afterwards holds it in 10 VGPRs from the record load on, and publishes the
// next stage_window_words() TEMPERED words of the stream in a small LDS draw window for the wave that runs the
// components (register-starved under the 64-VGPR budget): a draw is one LDS broadcast read per 64 draws plus a
// v_readlane.  A step that draws past the window (many agents) or past word 623 refills it from the state in HBM
// (rng_refill; a twist there writes the new state back, and the holder of the registers re-reads it).
struct MTL {
  uint32_t* w;  // LDS draw window: tempered words base ... base + avail - 1 of the generator's current window
  int pos;      // wave-uniform index of the next unused word of the generator's window (624 = twist first)
  // 64 words of the draw window in a register (lane j: word cbase + j): a draw is a v_readlane
  uint32_t cache;
  int cbase;
  // this step's changes to the maps, kept in registers until the components are done (-> c.dirty):
  int dn;             // cells appended to the change list
  uint32_t mv0, mv1;  // agents that moved
  int base, avail;    // what the draw window holds
  int tw;             // twists rng_refill performed this step (-> c.dirty[3])
  uint32_t* gkey;     // the replica's generator state in HBM (record + o_mt); AIE_RNG_FAST: in the record's LDS image
  int cap;            // capacity of the draw window in words
  bool fast;          // AIE_RNG_FAST (compile-time in the instances)
};
// Tempered words [pos, pos + avail) of the state in m -> w[0, avail); returns avail = min(cap, 624 - pos).
__device__ __forceinline__ int draw_window_publish(uint32_t* w, int cap, const MT& m, int pos, int lane) {
  const int avail = cap < AIE_MT_N - pos ? cap : AIE_MT_N - pos;
  const int r0 = pos >> 6;
  // (the rows as opaque register values: left to itself the optimiser turns the select chain below into ONE load with a
  // run-time index -- and the ten rows into a stack array in scratch memory for it)
  uint32_t rr[10];
#pragma unroll
  for (int j = 0; j < 10; ++j) {
    rr[j] = m.r[j];
    asm("" : "+v"(rr[j]));
  }
  for (int d = 0; d * 64 < cap + 64; ++d) {  // lane l of row r holds word 64 r + l
    const int r = r0 + d;
    if (r > 9) break;
    uint32_t v = rr[0];
#pragma unroll
    for (int j = 1; j < 10; ++j) v = (r == j) ? rr[j] : v;
    const int slot = 64 * r + lane - pos;
    if (slot >= 0 && slot < avail) w[slot] = v;  // (raw state words: the reader tempers the 64 it caches, rng_u32)
  }
  AIE_WSYNC();
  return avail;
}
// The same from the state in HBM: only the rows the window covers are fetched (step start: the wave that will hold
// the state later has nothing but the record copy to do, and the fetch rides behind it).  In two halves, so that the
// fetch can be in flight together with the caller's other loads and everything is waited for once (step_body):
// draw_rows_request asks for a lane's word of each of the first three rows the window covers -- all there are up to a
// window of 128 words -- and waits for nothing; draw_rows_commit writes them to the window and fetches what a larger
// window has beyond them, row by row.  Word i of the state is addressed as the (wave-uniform) state pointer plus an
// unsigned 32-bit byte offset of the lane.
struct DrawRows { uint32_t v[3]; };
__device__ __forceinline__ const uint32_t* draw_row_word(const uint32_t* __restrict__ gkey, int i) {
  return reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(gkey) + 4u * (uint32_t)i);
}
// (slot < avail implies i < 624; the words are raw: see draw_window_publish)
__device__ __forceinline__ bool draw_row_has(int cap, int pos, int d, int lane) {
  const int avail = cap < AIE_MT_N - pos ? cap : AIE_MT_N - pos;
  const int slot = 64 * ((pos >> 6) + d) + lane - pos;
  return pos >= 0 && d * 64 < cap + 64 && slot >= 0 && slot < avail;
}
__device__ __forceinline__ DrawRows draw_rows_request(int cap, const uint32_t* __restrict__ gkey, int pos, int lane) {
  DrawRows rows = {{0u, 0u, 0u}};
#pragma unroll
  for (int d = 0; d < 3; ++d)
    if (draw_row_has(cap, pos, d, lane)) rows.v[d] = *draw_row_word(gkey, 64 * ((pos >> 6) + d) + lane);
  return rows;
}
__device__ __forceinline__ int draw_rows_commit(uint32_t* w, int cap, const DrawRows& rows, const uint32_t* __restrict__ gkey,
                                                int pos, int lane) {
  const int r0 = pos >> 6;
#pragma unroll
  for (int d = 0; d < 3; ++d)
    if (draw_row_has(cap, pos, d, lane)) w[64 * (r0 + d) + lane - pos] = rows.v[d];
  for (int d = 3; d * 64 < cap + 64; ++d) {
    if (r0 + d > 9) break;
    if (draw_row_has(cap, pos, d, lane)) w[64 * (r0 + d) + lane - pos] = *draw_row_word(gkey, 64 * (r0 + d) + lane);
  }
  return cap < AIE_MT_N - pos ? cap : AIE_MT_N - pos;
}
__device__ __forceinline__ void mt_rows_from_hbm(MT& m, const uint32_t* gkey, int lane) {
  // agent-scope loads: the rows may have been rewritten by the other wave of the workgroup during this launch
#pragma unroll
  for (int j = 0; j < 9; ++j) m.r[j] = __hip_atomic_load(gkey + 64 * j + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  m.r[9] = lane < 48 ? __hip_atomic_load(gkey + 576 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
}
struct Refill { int pos, avail, twisted; };
// Out of line (rare: a step in ~30 crosses word 623 with 4 agents; steps with ~100 agents outrun the window): the
// state comes from HBM -- the record's copy, or what an earlier refill of this step wrote back.
__device__ __attribute__((noinline, cold)) Refill rng_refill(uint32_t* gkey, uint32_t* w, int cap, int pos, int lane) {
  MT m;
  m.fast = false;  // (MT19937 only: the counter stream refills through rng_refill_fast)
  mt_rows_from_hbm(m, gkey, lane);
  int twisted = 0;
  if (pos >= AIE_MT_N) {
    mt_twist_body(m, lane);
    pos = 0;
    twisted = 1;
#pragma unroll
    for (int j = 0; j < 9; ++j) __hip_atomic_store(gkey + 64 * j + lane, m.r[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lane < 48) __hip_atomic_store(gkey + 576 + lane, m.r[9], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  const int avail = draw_window_publish(w, cap, m, pos, lane);
  return Refill{pos, avail, twisted};
}
// ---- AIE_RNG_FAST: the draw window straight from the counter stream.  Words [pos, pos + avail) of block `blk` -> w[0,
// avail): lane l of pass d computes pair (pos >> 1) + 64 d + l, i.e. window slots 2 (64 d + l) - (pos & 1) and the next.
__device__ __forceinline__ int draw_window_publish_fast(uint32_t* w, int cap, uint32_t key, uint32_t blk, uint32_t salt, int pos,
                                                        int lane) {
  const int npass = (cap + 127) >> 7;
  int avail = cap < AIE_MT_N - pos ? cap : AIE_MT_N - pos;
  if (avail > 128 * npass - (pos & 1)) avail = 128 * npass - (pos & 1);
  for (int d = 0; d < npass; ++d) {
    if (128 * d - (pos & 1) >= avail) break;
    uint32_t x0, x1;
    fast_pair(key, blk, salt, (pos >> 1) + 64 * d + lane, x0, x1);
    const int slot = 2 * (64 * d + lane) - (pos & 1);
    if (slot >= 0 && slot < avail) w[slot] = x0;
    if (slot + 1 < avail) w[slot + 1] = x1;
  }
  return avail;
}
// `st`: the stream's state in the record's LDS image (key32, block number, salt).  The wave that runs the components
// moves to the next block here; the other wave of the replica picks the block number up behind the workgroup barrier.
__device__ __attribute__((noinline, cold)) Refill rng_refill_fast(uint32_t* st, uint32_t* w, int cap, int pos, int lane) {
  uint32_t blk = (uint32_t)uni((int)st[1]);
  int twisted = 0;
  if (pos >= AIE_MT_N) {
    blk += 1u;
    pos = 0;
    twisted = 1;
    if (lane == 0) st[1] = blk;
  }
  const int avail = draw_window_publish_fast(w, cap, (uint32_t)uni((int)st[0]), blk, (uint32_t)uni((int)st[2]), pos, lane);
  AIE_WSYNC();
  return Refill{pos, avail, twisted};
}
__device__ __forceinline__ uint32_t rng_u32(MTL& l, int lane) {
  if (__builtin_expect(l.pos >= l.base + l.avail, 0)) {
    const Refill r = l.fast ? rng_refill_fast(l.gkey, l.w, l.cap, l.pos, lane) : rng_refill(l.gkey, l.w, l.cap, l.pos, lane);
    l.pos = uni(r.pos);  // (a function's results come back in vector registers: keep the bookkeeping scalar)
    l.base = l.pos;
    l.avail = uni(r.avail);
    l.tw += uni(r.twisted);
    l.cbase = -AIE_MT_N;
  }
  int k = l.pos - l.cbase;
  if ((unsigned)k >= (unsigned)AIE_NT) {  // the next (up to) 64 words of the draw window
    const int idx = l.pos - l.base + lane;
    // MT19937's window holds RAW state words (round 6): a step draws one or two dozen of the 128+ the window offers, so the
    // tempering happens here, once per 64 cached words, instead of over the whole window on the way in
    const uint32_t raw = l.w[idx < l.avail ? idx : l.avail - 1];
    l.cache = l.fast ? raw : mt_temper(raw);
    l.cbase = l.pos;
    k = 0;
  }
  l.pos += 1;
  return bcast(l.cache, k);
}
__device__ __forceinline__ double rng_double(MTL& l, int lane) {
  const uint32_t a = rng_u32(l, lane);
  const uint32_t b = rng_u32(l, lane);
  return u53(a, b);
}
// (Tried: finding the first acceptable word of the cached block with one ballot instead of a readlane / compare / branch
// per attempt -- bit-identical, but the unrolled permutation loops grow and the launch gets slower: C2 24.9 -> 25.7 us,
// C3 41.6 -> 43.7 us.)
__device__ __forceinline__ uint32_t rng_interval(MTL& l, int lane, uint32_t max) {
  if (max == 0) return 0;
  uint32_t mask = max, v;
  mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
  while ((v = (rng_u32(l, lane) & mask)) > max) {}
  return v;
}
__device__ __forceinline__ int rng_permutation(MTL& l, int lane, int n) {
  int p = lane;
  for (int i = n - 1; i >= 1; --i) {
    const int j = (int)rng_interval(l, lane, (uint32_t)i);
    const int vi = bcast(p, i), vj = bcast(p, j);
    p = (lane == i) ? vj : ((lane == j) ? vi : p);
  }
  return p;
}
__device__ __forceinline__ double rng_gauss(const Ctx& c, MT& m) {  // legacy_gauss (polar Box-Muller, cached)
  int32_t* has = R_I32(c, o_mt_has_gauss);
  double* g = R_F64(c, o_mt_gauss);
  if (*has) {
    const double t = *g;
    *has = 0;
    *g = 0.0;
    return t;
  }
  double f, x1, x2, r2;
  do {
    x1 = 2.0 * rng_double(m, c.tid) - 1.0;
    x2 = 2.0 * rng_double(m, c.tid) - 1.0;
    r2 = x1 * x1 + x2 * x2;
  } while (r2 >= 1.0 || r2 == 0.0);
  f = sqrt(-2.0 * aie_log_glibc(r2) / r2);  // libm's log bit for bit (aie_glibc_math.h); sqrt and / are IEEE-exact
  *g = f * x1;
  *has = 1;
  return f * x2;
}
__device__ __forceinline__ double rng_pareto(MT& m, int lane, double a) { return aie_exp_glibc(-aie_log_glibc(1.0 - rng_double(m, lane)) / a) - 1.0; }
__device__ __forceinline__ double rng_lognormal(const Ctx& c, MT& m, double mean, double sigma) { return aie_exp_glibc(mean + sigma * rng_gauss(c, m)); }

// ------------------------------------------------------------------------------------
// PeriodicBracketTax, F/components/redistribution.py
// ------------------------------------------------------------------------------------
// Coin arithmetic of the tax / redistribution components without multiply-add contraction: the
// reference (and the restatement, built with -ffp-contract=off) round every product, and a one-ulp
// difference in an agent's coin flips discrete decisions later on (income residues of +-1e-15 decide
// `income < 0` in marginal_rate and `z_t > 0` in the Saez sample filter).
#pragma clang fp contract(off)
// curr_rate_max :390-394: the annealed limit follows _last_completions, which generate_masks
// refreshes AFTER the observations of a reset are built (:1036-1046) -- kept as a state field.
__device__ __forceinline__ double tax_curr_rate_max(const Ctx& c) {
  return aie_annealed_tax_limit(*R_I32(c, o_tax_last_completions), c.R.c.tax_annealing_warmup,
                                c.R.c.tax_annealing_slope, c.R.c.tax_rate_max);
}
// this replica's Saez block (tax_model "saez", aie_layout.h: a_saez); step / reset kernels only (c.met set)
__device__ __forceinline__ uint8_t* saez_block(const Ctx& c) {
  return C_MET(c) - c.R.a_metrics - (int64_t)c.e * c.P.met_bytes + c.R.a_saez + (int64_t)c.e * c.P.saez_stride;
}
__device__ __forceinline__ double tax_rate(const Ctx& c, int b) {  // curr_marginal_rates :396-417
  if (c.P.c.tax_model == AIE_TAX_MODEL_WRAPPER) return c.rtab[R_I32(c, o_tax_rate_idx)[b]];
  if (c.saez) {  // np.minimum(curr_bracket_tax_rates, curr_rate_max) :406-409
    const double r = R_F64(c, o_tax_saez_rates)[b];
    const double cap = c.P.c.tax_annealing ? tax_curr_rate_max(c) : c.R.c.tax_rate_max;
    return r < cap ? r : cap;
  }
  const double r = c.R.c.tax_fixed_rates[b];
  if (!c.P.c.tax_annealing) return r;
  const double cap = tax_curr_rate_max(c);
  return r < cap ? r : cap;
}
// _curr_rates_obs: the rates the "curr_rates" observation shows (cached at period starts and resets)
__device__ __forceinline__ double tax_rate_obs(const Ctx& c, int b) {
  if (c.saez) return R_F64(c, o_tax_saez_obs_rates)[b];
  return tax_rate(c, b);
}
// planner tax-rate action j of a bracket: allowed by the annealing schedule? (annealed_tax_mask,
// utils.py:59-118, evaluated with the completions count of the episode's reset)
__device__ __forceinline__ bool tax_rate_action_visible(const Ctx& c, int j) {
  if (!c.P.c.tax_annealing) return true;
  double full = 0;
  for (int k = 0; k < c.P.c.tax_n_disc_rates; ++k) full = fmax(full, fabs(c.rtab[k]));
  const double vis = aie_annealed_tax_limit(*R_I32(c, o_tax_last_completions), c.R.c.tax_annealing_warmup,
                                            c.R.c.tax_annealing_slope, full);
  return fabs(c.rtab[j]) <= vis;
}
__device__ __forceinline__ double tax_marginal_rate(const Ctx& c, double income) {  // marginal_rate :837-844
  if (income < 0) return 0.0;
  const int NB = c.P.NB;
  for (int b = 0; b < NB; ++b) {
    const double lo = c.R.c.tax_bracket_cutoffs[b];
    const bool under = (b + 1 < NB) ? (income < c.R.c.tax_bracket_cutoffs[b + 1]) : (income < __builtin_huge_val());
    if (income >= lo && under) return tax_rate(c, b);
  }
  return tax_rate(c, 0);
}
__device__ __forceinline__ double tax_bin(const Ctx& c, double income, int b) {
  const int NB = c.P.NB;
  const double cut = c.R.c.tax_bracket_cutoffs[b];
  const double size = (b + 1 < NB) ? c.R.c.tax_bracket_cutoffs[b + 1] - cut : __builtin_huge_val();
  double past = income - cut;
  if (past < 0) past = 0;
  return tax_rate(c, b) * (size < past ? size : past);
}
__device__ __forceinline__ double tax_due(const Ctx& c, double income) {  // taxes_due :846-851
  const int NB = c.P.NB;
  // np.sum of NB values (pairwise summation, loops_utils.h.src)
  if (NB < 8) {
    double res = -0.0;
    for (int b = 0; b < NB; ++b) res += tax_bin(c, income, b);
    return res;
  }
  double r0 = tax_bin(c, income, 0), r1 = tax_bin(c, income, 1), r2 = tax_bin(c, income, 2),
         r3 = tax_bin(c, income, 3), r4 = tax_bin(c, income, 4), r5 = tax_bin(c, income, 5),
         r6 = tax_bin(c, income, 6), r7 = tax_bin(c, income, 7);
  int b = 8;
  for (; b < NB - (NB % 8); b += 8) {
    r0 += tax_bin(c, income, b + 0); r1 += tax_bin(c, income, b + 1);
    r2 += tax_bin(c, income, b + 2); r3 += tax_bin(c, income, b + 3);
    r4 += tax_bin(c, income, b + 4); r5 += tax_bin(c, income, b + 5);
    r6 += tax_bin(c, income, b + 6); r7 += tax_bin(c, income, b + 7);
  }
  double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; b < NB; ++b) res += tax_bin(c, income, b);
  return res;
}

}  // namespace aie

struct NextActions {  // aie_step_sample_next: where and how to sample the next step's random actions
  // The replica count (and the replica range) FIRST: a workgroup needs them for its very first decision (which replica it
  // is), and here they share the argument segment's first 64 bytes with the parameter block's and the arena's pointers
  // -- one scalar-cache miss instead of two at the head of every workgroup (round 6; as a field of the parameter block
  // the count had been a second, dependent round trip: the caches are cold at every launch).
  int32_t E;
  // replicas this launch steps: [e_lo, e_hi), or all of them when e_hi == 0.  An environment with dense-log replicas
  // whose current episode is being logged steps those replicas with aie_step_kernel_log and the rest with its fast
  // kernel (aie_capi.hip: aie_step_impl)
  int32_t e_lo, e_hi;
  int32_t masked;  // aie_step_sample_next_masked (COVID): the next actions are drawn among what the new masks allow
  int32_t* a;
  int32_t* p;
  uint64_t seed;
  int64_t env_offset;  // (the draw index `t` of the counter RNG is the replica's own record field o_sample_t)
  // aie_step_range (custom host components, include/aie.h): the built-in components [comp_lo, comp_hi) of the list and
  // the parts of a step this launch performs -- AIE_STEP_HEAD (timestep += 1), AIE_STEP_TAIL (regeneration, observations,
  // masks, rewards, done; or its three parts AIE_STEP_REGEN / EMIT / CLOSE, which scenario hooks run between),
  // AIE_STEP_OBSERVE (observations and masks of the state as it stands, nothing else); phase == 0: a whole step.  Honoured by the full-featured kernel only (aie_step_kernel_log); everybody else steps whole steps.
  int32_t comp_lo, comp_hi, phase;
  // aie_step_range: the replicas the launch touches (uint8 [E], nonzero = yes), nullptr = all of them -- a masked reset's
  // follow-up launches leave the replicas it did not reset alone.  The full-featured kernel only, like the ranges above.
  const uint8_t* mask;
};
// This step's slot of the reward log: the replica's slot counter selects it and moves on (`writer`: the one lane that
// stores the counter back; every lane of the wave calls this with the same fields).
// (`R`: the run-time parameter block in device memory, where aie_set_reward_log keeps the log's address, slot count and
// epoch -- nothing of it travels by value, so a captured launch follows a later aie_set_reward_log call)
__device__ __forceinline__ float* rew_log_claim(const aie_params& R, int32_t* slot_field, int32_t* epoch_field, int E,
                                                int n, bool writer) {
  float* const log = R.rew_log;
  if (!log) return nullptr;
  const int epoch = R.rew_epoch;
  int slot = __builtin_amdgcn_readfirstlane(*slot_field);
  if (__builtin_amdgcn_readfirstlane(*epoch_field) != epoch) slot = 0;
  if (writer) {
    *epoch_field = epoch;
    *slot_field = slot + 1 >= R.rew_slots ? 0 : slot + 1;
  }
  return log + (int64_t)slot * E * (n + 2);
}
