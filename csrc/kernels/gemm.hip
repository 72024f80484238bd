// bf16 GEMM on CDNA4 MFMA with fused epilogues (SURVEY K9/K10 epilogue targets).
//
//   C[M, N] = A[M, K] . B[N, K]^T     (both operands K-contiguous: "NT"; fp32 accumulate)
//
// Workgroup tile 256 x 256 x 64, 8 waves (2 along M x 4 along N, 128 x 64 outputs per wave, 32
// v_mfma_f32_16x16x32_bf16 accumulators). Operands stream global -> LDS by LDS-DMA
// (global_load_lds_dwordx4: one 1 KiB piece = 8 rows x 128 B per wave-instruction), double
// buffered. The LDS image is lane-linear (the DMA writes base + 16*lane), so the XOR swizzle that
// makes the fragment reads bank-conflict-free is applied to the per-lane SOURCE address:
// physical 16-byte chunk c of row r holds logical chunk c ^ swz(r), swz(r) = (r >> 1) & 7 -- the 16
// rows x 1 chunk read by each ds_read_b128 lane group then land on 16 distinct bank slots.
// Workgroups walk the output tiles in an XCD-aware, column-grouped order (B column panels stay in
// one XCD's L2 while its A row panels stream).
//
// Three kernels: gemm_nt_kernel, the simple double-buffered form (the bitwise reference of the tests),
// gemm_nt_phased_kernel, a 4-phase pipeline (1042 vs 1073 TF for the 8-phase schedule at M=61440, N=3072,
// K=1024, profiles/r1_gemm_8phase.jsonl; kept as a tested variant), and gemm_nt_8ph_kernel, the 8-phase one.
// Epilogues of the latter (template EPI): 0 = bf16 store (+bias), 1 = QKV + rotary into the attention storage,
// 2 = GEGLU backward fused into the FF-out dgrad GEMM (see gemm_store_epilogue). The training step runs its
// GEMMs on the generated assembly kernels (csrc/asm); these serve d_model < 1024 and DALLE_AMD_ASM_GEMM=0,
// where production reaches EPI 2 (ff_dgrad_geglu); the fused QKV path runs on gemm_pt.hip's register-direct
// epilogue (both timed in profiles/r3_gemm_pt_vs_hipblaslt_8ph.jsonl), EPI 1 here is its tested predecessor.
//
// Measured and rejected, the code removed (numbers under profiles/):
//   * a persistent form (one workgroup per CU walking the tiles, the next tile's first K-tile DMA issued
//     before the current tile's epilogue): 1-7 % SLOWER than one tile per workgroup on every training shape
//     and on both fused epilogues -- keeping the loop-invariant fragment / DMA offsets live across the
//     epilogue pushed it past 256 VGPRs (r2_gemm_persistent_vs_8ph_vs_hipblaslt.jsonl);
//   * two co-resident 4-wave workgroups per CU (256 x 128 tiles, K-step 32) so one's epilogue runs beside
//     the other's MFMAs: main loop ~25 % slower on plain products (r2_gemm_2wg_variant.hip.txt), and
//     2266-2322 vs 2171 us on the GEGLU-backward GEMM, with or without start staggers (r4_geglu_bwd_2wg.jsonl,
//     r4_geglu_bwd_2wg_stagger.jsonl);
//   * non-temporal output stores: -5 % on the plain-store kernel at the large shapes, no gain on the fused
//     epilogues or the full step (r2_gemm_epilogue_cost.jsonl);
//   * a start-time stagger of the first wave of workgroups: slower on every training shape
//     (r3_gemm_stagger.jsonl);
//   * MN-major operands for the weight gradients (ds_read_b64_tr_b16 fragments): hipBLASLt was faster
//     (r2_wgrad_mn_major_vs_hipblaslt.jsonl).
#include "common.h"

namespace dalle {

typedef __attribute__((ext_vector_type(4))) float f32x4_t;

constexpr int GBM = 256, GBN = 256, GBK = 64;
constexpr int G_THREADS = 512;

__device__ __forceinline__ int gswz(int r) { return (r >> 1) & 7; }

// one operand tile (256 rows x 64 k) of buffer `buf` into LDS via 4 DMA pieces per wave
__device__ __forceinline__ void gemm_stage(const __bf16* __restrict__ src, int ld, int row0, int k0, __bf16* lds_tile,
                                           int wave, int lane) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int piece = wave * 4 + i;           // 0..31, rows 8*piece .. 8*piece+7
    const int row = piece * 8 + (lane >> 3);  // this lane's row in the tile
    const int lchunk = (lane & 7) ^ gswz(row);  // logical chunk that lands in physical chunk (lane & 7)
    const __bf16* g = src + (size_t)(row0 + row) * ld + k0 + lchunk * 8;
    __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)g,
                                     (void __attribute__((address_space(3)))*)(lds_tile + piece * 512), 16, 0, 0);
  }
}

__device__ __forceinline__ bf16x8 gemm_frag(const __bf16* tile, int row, int chunk) {
  return *reinterpret_cast<const bf16x8*>(tile + row * 64 + ((chunk ^ gswz(row)) << 3));
}

// XCD-aware tile order: linear id -> XCD slot; within an XCD, tiles sweep M inside groups of
// `group` column panels (group > 0), or sweep N inside groups of -group row panels (group < 0)
__device__ __forceinline__ void gemm_tile_of(int& tm, int& tn, int tiles_m, int tiles_n, int group = 4) {
  const int nwg = tiles_m * tiles_n;
  int id = blockIdx.x;
  if ((nwg & 7) == 0) id = (id & 7) * (nwg >> 3) + (id >> 3);  // bijective when nwg % 8 == 0
  if (group > 0) {
    const int g = id / (group * tiles_m);
    const int first_n = g * group;
    const int gn = min(tiles_n - first_n, group);
    const int in_group = id - g * group * tiles_m;
    tn = first_n + in_group % gn;
    tm = in_group / gn;
  } else {
    const int gm_size = -group;
    const int g = id / (gm_size * tiles_n);
    const int first_m = g * gm_size;
    const int gm = min(tiles_m - first_m, gm_size);
    const int in_group = id - g * gm_size * tiles_n;
    tm = first_m + in_group % gm;
    tn = in_group / gm;
  }
}

// The simple double-buffered kernel: whole K-tiles, one wait and one barrier per K-step. It is the bitwise
// reference the pipelined kernel below is tested against.
__global__ __launch_bounds__(G_THREADS, 1) void gemm_nt_kernel(const __bf16* __restrict__ A, const __bf16* __restrict__ B,
                                                               __bf16* __restrict__ C, const __bf16* __restrict__ bias,
                                                               int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) __bf16 smem[2 * 2 * GBM * GBK];  // [buf][A | B] 128 KiB
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 2, wn = wave & 3;
  int tm, tn;
  gemm_tile_of(tm, tn, M / GBM, N / GBN);
  const int row0 = tm * GBM, col0 = tn * GBN;

  f32x4_t acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int nk = K / GBK;
  gemm_stage(A, K, row0, 0, smem, wave, lane);
  gemm_stage(B, K, col0, 0, smem + GBM * GBK, wave, lane);
  __builtin_amdgcn_s_waitcnt(0);  // vmcnt(0) lgkmcnt(0)
  __syncthreads();

  const int fr = lane & 15, fq = lane >> 4;
  for (int t = 0; t < nk; ++t) {
    const int buf = t & 1;
    if (t + 1 < nk) {
      __bf16* nb = smem + (buf ^ 1) * (2 * GBM * GBK);
      gemm_stage(A, K, row0, (t + 1) * GBK, nb, wave, lane);
      gemm_stage(B, K, col0, (t + 1) * GBK, nb + GBM * GBK, wave, lane);
    }
    const __bf16* As = smem + buf * (2 * GBM * GBK);
    const __bf16* Bs = As + GBM * GBK;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 a[8], b[4];
#pragma unroll
      for (int i = 0; i < 8; ++i) a[i] = gemm_frag(As, wm * 128 + i * 16 + fr, kk * 4 + fq);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = gemm_frag(Bs, wn * 64 + j * 16 + fr, kk * 4 + fq);
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
  }

  // ---- epilogue: stage the wave's 128 x 64 tile (bf16) through LDS, then 16-byte row stores ----
  __bf16* ep = smem + wave * (128 * 64);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = j * 16 + fr;  // column within the wave tile
    float bv = 0.f;
    if (bias != nullptr) bv = (float)bias[col0 + wn * 64 + c];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = i * 16 + fq * 4 + r;
        // row-major [128][64] image with the 16-byte chunk XOR-swizzled by row (conflict-free reads below)
        ep[row * 64 + (((c >> 3) ^ (row & 7)) << 3) + (c & 7)] = (__bf16)(acc[i][j][r] + bv);
      }
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __bf16* Cw = C + (size_t)(row0 + wm * 128) * N + col0 + wn * 64;
#pragma unroll
  for (int it = 0; it < 16; ++it) {
    const int idx = it * 64 + lane;  // 128 rows x 8 chunks
    const int row = idx >> 3, ch = idx & 7;
    const s16x8 v = *reinterpret_cast<const s16x8*>(ep + row * 64 + ((ch ^ (row & 7)) << 3));
    *reinterpret_cast<s16x8*>(Cw + (size_t)row * N + ch * 8) = v;
  }
}

// Epilogue parameters of the pipelined kernels
struct EpiArgs {
  // EPI 1 (QKV projection with the 3-axis rotary fused in): the GEMM writes q (rotated, pre-scaled), k, v
  // (rotated) straight into the padded attention storage layout (B*H, Np, 64) instead of a (M, 3*H*64) tensor
  __bf16* q;
  __bf16* k;
  __bf16* v;
  const float* cosT;
  const float* sinT;
  int T, Tp, S, logS, n, Np, H, col_major;
  float qscale;
  // EPI 2 (GEGLU backward fused into the FF-out dgrad GEMM, see gemm_geglu_bwd): h = the FF-in
  // pre-activation [value | gate] (M, 2F), dh its gradient, part = per-128-row partial bias grads
  const __bf16* gh;
  __bf16* gdh;
  float* gpart;
  int F;
  int drain = 0;  // s_waitcnt vmcnt(0) after the epilogue (gemm_pt.hip gemm_set_drain)
  int cpol = 0;   // cache policy of the output stores (common.h cstore16; gemm_pt.hip gemm_set_cpol)
};

__device__ __forceinline__ int rope_epi_seq2st(const EpiArgs& e, int p) {
  if (p < e.T) return p;
  const int kk = p - e.T;
  const int kst = e.col_major ? ((kk & (e.S - 1)) << e.logS) + (kk >> e.logS) : kk;
  return e.Tp + kst;
}

// ------------------------------------------------------------------------------------------------
// The pipelined kernel splits each operand tile into half-tiles and each K-tile into 4 phases, one per
// 64 x 32 quadrant of the wave's 128 x 64 output (16 MFMAs each); a wave only ever reads ITS A half and
// B half of a phase:
//   phase 1: read B[cols 0-31] + A[rows 0-63] -> MFMA quadrant (lo, lo)
//   phase 2: read B[cols 32-63]               -> MFMA quadrant (lo, hi)
//   phase 3: read A[rows 64-127]              -> MFMA quadrant (hi, hi)
//   phase 4: (registers only)                 -> MFMA quadrant (hi, lo)
// ------------------------------------------------------------------------------------------------
constexpr int HALF = 128 * GBK;  // elements of one half-tile image

// Half-tile image of 128 operand rows: the rows one PHASE reads across all 8 waves. For A (blk = 64)
// the "lo" half holds tile rows 0-63 and 128-191 (rows 0-63 of both wave rows), "hi" the other 128;
// for B (blk = 32) "lo" holds columns {0-31, 64-95, 128-159, 192-223} (the first 32 of each wave's
// 64), "hi" the rest. Image row hr <-> tile row (hr / blk) * 2 blk + off + hr % blk.
__device__ __forceinline__ void stage_half(const __bf16* __restrict__ src, int ld, int row0, int k0, __bf16* lds_half,
                                           int wave, int lane, int blk, int off) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int piece = wave * 2 + i;           // 0..15: image rows 8*piece .. 8*piece+7
    const int hr = piece * 8 + (lane >> 3);
    const int row = (hr / blk) * 2 * blk + off + (hr % blk);
    const int lchunk = (lane & 7) ^ gswz(hr);
    const __bf16* g = src + (size_t)(row0 + row) * ld + k0 + lchunk * 8;
    __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)g,
                                     (void __attribute__((address_space(3)))*)(lds_half + piece * 512), 16, 0, 0);
  }
}

// Epilogue of the pipelined kernel: stage each wave's 128 x 64 accumulator tile (bf16) through its private
// 16 KB of LDS, then EPI 0 = 16-byte row stores (+bias), EPI 1 = rotary + scatter into the attention storage,
// EPI 2 = GEGLU backward (below).
// All LDS operand reads and DMA must be retired by the caller (the whole 128 KiB is reused).
template <int EPI>
__device__ __forceinline__ void gemm_store_epilogue(f32x4_t (&acc)[8][4], __bf16* smem, __bf16* __restrict__ C,
                                                    const __bf16* __restrict__ bias, int N, int row0, int col0, int wave,
                                                    int lane, const EpiArgs& e) {
  static_assert(EPI >= 0 && EPI <= 2, "epilogues: 0 = bf16 store (+bias), 1 = QKV + rotary, 2 = GEGLU backward");
  const int wm = wave >> 2, wn = wave & 3;  // the wave's 128 x 64 block of the tile
  __bf16* ep = smem + wave * (128 * 64);
  const int fr = lane & 15, fq = lane >> 4;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = j * 16 + fr;
    float bv = 0.f;
    if (bias != nullptr) bv = (float)bias[col0 + wn * 64 + c];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = i * 16 + fq * 4 + r;
        ep[row * 64 + (((c >> 3) ^ (row & 7)) << 3) + (c & 7)] = (__bf16)(acc[i][j][r] + bv);
      }
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xC07F);
  if constexpr (EPI == 0) {
    const __amdgpu_buffer_rsrc_t oc = uniform_rsrc(C);
    __bf16* Cw = C + (size_t)(row0 + wm * 128) * N + col0 + wn * 64;
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int idx = it * 64 + lane;
      const int row = idx >> 3, ch = idx & 7;
      const s16x8 v = *reinterpret_cast<const s16x8*>(ep + row * 64 + ((ch ^ (row & 7)) << 3));
      if (e.cpol) cstore16(C, oc, (uint32_t)(((size_t)(row0 + wm * 128 + row) * N + col0 + wn * 64 + ch * 8) * 2),
                           __builtin_bit_cast(u32x4_vs, v), e.cpol);
      else *reinterpret_cast<s16x8*>(Cw + (size_t)row * N + ch * 8) = v;
    }
  } else if constexpr (EPI == 1) {
    // the wave's 64 columns are exactly one (part, head): rotate each 8-column chunk of each row and
    // scatter the row to its storage slot
    const int HD = e.H * 64;
    const int c0 = col0 + wn * 64;
    const int part = c0 / HD, h = (c0 - part * HD) >> 6;
    __bf16* dstT = part == 0 ? e.q : (part == 1 ? e.k : e.v);
    const float sc = part == 0 ? e.qscale : 1.0f;
    const __amdgpu_buffer_rsrc_t oq = uniform_rsrc(dstT);
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {
      const int idx = it * 64 + lane;
      const int row = idx >> 3, ch = idx & 7;
      const int r = row0 + wm * 128 + row;
      const int b = r / e.n, p = r - b * e.n;
      float x[8], cs[8], sn[8];
      unpack8(*reinterpret_cast<const s16x8*>(ep + row * 64 + ((ch ^ (row & 7)) << 3)), x);
      const float* cp = e.cosT + (size_t)p * 64 + ch * 8;
      const float* sp = e.sinT + (size_t)p * 64 + ch * 8;
      *reinterpret_cast<f32x4*>(cs) = *reinterpret_cast<const f32x4*>(cp);
      *reinterpret_cast<f32x4*>(cs + 4) = *reinterpret_cast<const f32x4*>(cp + 4);
      *reinterpret_cast<f32x4*>(sn) = *reinterpret_cast<const f32x4*>(sp);
      *reinterpret_cast<f32x4*>(sn + 4) = *reinterpret_cast<const f32x4*>(sp + 4);
#pragma unroll
      for (int i = 0; i < 8; i += 2) {
        const float a0 = x[i], a1 = x[i + 1];
        x[i] = (a0 * cs[i] + a1 * sn[i]) * sc;
        x[i + 1] = (a1 * cs[i + 1] + a0 * sn[i + 1]) * sc;
      }
      const int srow = rope_epi_seq2st(e, p);
      const size_t o = ((size_t)(b * e.H + h) * e.Np + srow) * 64 + ch * 8;
      if (e.cpol) cstore16(dstT, oq, (uint32_t)(o * 2), __builtin_bit_cast(u32x4_vs, pack8(x)), e.cpol);
      else *reinterpret_cast<s16x8*>(dstT + o) = pack8(x);
    }
  } else {
    // all 32 [value | gate] pre-activation loads of a lane (16 rows x 2 halves) are issued before any math
    // instead of the 8 a partially unrolled loop keeps in flight (the epilogue does not overlap this
    // workgroup's MFMA work, so its HBM latency is exposed once per tile)
    s16x8 hv[2][8], hg[2][8];
    const int gcol = col0 + wn * 64 + (lane & 7) * 8;
    auto load_h = [&](int half) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const size_t r = (size_t)(row0 + wm * 128 + (half * 8 + k) * 8 + (lane >> 3));
        hv[half][k] = *reinterpret_cast<const s16x8*>(e.gh + r * 2 * e.F + gcol);
        hg[half][k] = *reinterpret_cast<const s16x8*>(e.gh + r * 2 * e.F + e.F + gcol);
      }
    };
    // GEGLU backward: the staged tile is du = dy . W2 (bf16, as the unfused path rounds it) for F-columns
    // [c0, c0 + 64); each lane owns one 8-column chunk of 16 rows: da_value = du * gelu(gate),
    // da_gate = du * value * gelu'(gate) straight into dh, and the chunk's column sums of the propagated
    // (bf16) values -- the FF-in bias gradient -- reduced over the 8 lanes sharing it (fixed xor tree)
    // into one partial row per 128-row wave block.
    const int F = e.F;
    const int c = gcol;
    const __amdgpu_buffer_rsrc_t od = uniform_rsrc(e.gdh);
    float sv[8] = {}, sg[8] = {};
    load_h(0);
    load_h(1);
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int row = it * 8 + (lane >> 3), ch = lane & 7;
      const size_t r = (size_t)(row0 + wm * 128 + row);
      float d[8], a[8], gg[8], da[8], dg[8];
      unpack8(*reinterpret_cast<const s16x8*>(ep + row * 64 + ((ch ^ (row & 7)) << 3)), d);
      unpack8(hv[it >> 3][it & 7], a);
      unpack8(hg[it >> 3][it & 7], gg);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float ge, gr;
        gelu_and_grad(gg[i], ge, gr);
        da[i] = d[i] * ge;
        dg[i] = d[i] * a[i] * gr;
      }
      const s16x8 pa = pack8(da), pg = pack8(dg);
      if (e.cpol) {
        cstore16(e.gdh, od, (uint32_t)((r * 2 * F + c) * 2), __builtin_bit_cast(u32x4_vs, pa), e.cpol);
        cstore16(e.gdh, od, (uint32_t)((r * 2 * F + F + c) * 2), __builtin_bit_cast(u32x4_vs, pg), e.cpol);
      } else {
        *reinterpret_cast<s16x8*>(e.gdh + r * 2 * F + c) = pa;
        *reinterpret_cast<s16x8*>(e.gdh + r * 2 * F + F + c) = pg;
      }
      unpack8(pa, da);
      unpack8(pg, dg);
#pragma unroll
      for (int i = 0; i < 8; ++i) { sv[i] += da[i]; sg[i] += dg[i]; }
    }
#pragma unroll
    for (int o = 8; o < 64; o <<= 1)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        sv[i] += __shfl_xor(sv[i], o, 64);
        sg[i] += __shfl_xor(sg[i], o, 64);
      }
    if (lane < 8) {
      float* pr = e.gpart + (size_t)((row0 >> 7) + wm) * 2 * F;
#pragma unroll
      for (int i = 0; i < 8; ++i) { pr[c + i] = sv[i]; pr[F + c + i] = sg[i]; }
    }
  }
}

// The 4-phase pipeline (variants 200-207, OPT = schedule options): every phase issues the LDS-DMA of one half-tile
// of the NEXT K-tile into the other buffer in consumption order (A-lo, B-lo, B-hi, A-hi); a counted vmcnt(4) before
// each phase's barrier keeps two half-tiles in flight while retiring exactly the half the next phase reads.
template <int EPI, int OPT>
__global__ __launch_bounds__(G_THREADS, 1) void gemm_nt_phased_kernel(const __bf16* __restrict__ A, const __bf16* __restrict__ B,
                                                                      __bf16* __restrict__ C, const __bf16* __restrict__ bias,
                                                                      int M, int N, int K, EpiArgs e) {
  // [buf][A0 | A1 | B0 | B1] half-tile images, 128 KiB in ONE array (a second __shared__ object can
  // make hipcc drain vmcnt before every ds_read)
  __shared__ __attribute__((aligned(16))) __bf16 smem[2 * 4 * HALF];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 2, wn = wave & 3;
  int tm, tn;
  gemm_tile_of(tm, tn, M / GBM, N / GBN);
  const int row0 = tm * GBM, col0 = tn * GBN;
  const int fr = lane & 15, fq = lane >> 4;

  f32x4_t acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // half-tile images per buffer, in consumption order: 0 A-lo (phase 0), 1 B-lo (phase 0),
  // 2 B-hi (phase 1), 3 A-hi (phase 2)
  auto slot = [&](int buf, int which) { return smem + (buf * 4 + which) * HALF; };
  auto stage = [&](int t, int p) {
    const int buf = t & 1, k0 = t * GBK;
    if (p == 0) stage_half(A, K, row0, k0, slot(buf, 0), wave, lane, 64, 0);
    else if (p == 1) stage_half(B, K, col0, k0, slot(buf, 1), wave, lane, 32, 0);
    else if (p == 2) stage_half(B, K, col0, k0, slot(buf, 2), wave, lane, 32, 32);
    else stage_half(A, K, row0, k0, slot(buf, 3), wave, lane, 64, 64);
  };

  const int nk = K / GBK;
  for (int p = 0; p < 4; ++p) stage(0, p);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  asm volatile("s_barrier" ::: "memory");

  bf16x8 a[4][2], b0[2][2], b1[2][2];  // [m-tile][kk], [n-tile][kk]
  for (int t = 0; t < nk; ++t) {
    const int buf = t & 1;
    const __bf16* Alo = slot(buf, 0);
    const __bf16* Blo = slot(buf, 1);
    const __bf16* Bhi = slot(buf, 2);
    const __bf16* Ahi = slot(buf, 3);
    const bool more = t + 1 < nk;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      // 1) fragment reads of this phase (data retired one phase earlier)
      if (p == 0) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) b0[j][kk] = gemm_frag(Blo, wn * 32 + j * 16 + fr, kk * 4 + fq);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) a[i][kk] = gemm_frag(Alo, wm * 64 + i * 16 + fr, kk * 4 + fq);
      } else if (p == 1) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) b1[j][kk] = gemm_frag(Bhi, wn * 32 + j * 16 + fr, kk * 4 + fq);
      } else if (p == 2) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) a[i][kk] = gemm_frag(Ahi, wm * 64 + i * 16 + fr, kk * 4 + fq);
      }
      // 2) LDS-DMA of one half-tile of the next K-tile, then retire all but the two youngest halves
      if (more) {
        stage(t + 1, p);
        // phase 3 reads nothing from LDS, so phase 2 need not retire anything (OPT & 1)
        if (!((OPT & 1) && p == 2)) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      // a compiler-visible barrier: the builtin s_barrier does not order memory operations, and a
      // ds_read of the next phase hoisted above it would race with other waves' DMA retirement
      asm volatile("s_barrier" ::: "memory");
      // 3) the quadrant's 16 MFMAs
      if (!(OPT & 2)) __builtin_amdgcn_s_setprio(1);
      const int mi0 = (p >= 2) ? 4 : 0;
      const bool right = (p == 1 || p == 2);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            f32x4_t& c = acc[mi0 + i][(right ? 2 : 0) + j];
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][kk], right ? b1[j][kk] : b0[j][kk], c, 0, 0, 0);
          }
      if (!(OPT & 2)) __builtin_amdgcn_s_setprio(0);
      if (OPT & 4) asm volatile("s_barrier" ::: "memory");
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();

  gemm_store_epilogue<EPI>(acc, smem, C, bias, N, row0, col0, wave, lane, e);
}

// ------------------------------------------------------------------------------------------------
// 8-phase template (cdna_hip_programming.md §5 "The 256^2 8-phase template", T3+T4+T5), re-derived:
// the 256x256x64 tile, half-tile images and quadrant order described above, where
//   * each phase is {ds_read subtile ; 1 half-tile LDS-DMA ; s_barrier ; lgkmcnt(0) ; 16 MFMA ;
//     s_barrier} and the two wave rows run STAGGERED by one barrier (wm == 1 enters one barrier
//     late), so on every SIMD one wave issues MFMAs while its partner reads LDS / issues DMA;
//   * three half-tiles stay in flight: the counted vmcnt(6) runs once per K-tile (phase 4), never 0
//     in the steady state. Staging order per K-tile t (consumption order is A-lo B-lo | B-hi | A-hi):
//       phase 1: A-hi(t+1) -> buf^1   (A-hi of buf^1 last read 2 phases ago)
//       phase 2: B-lo(t+2) -> buf     (B-lo read in phase 1, retired by its lgkmcnt(8) before phase 1's
//                                      first barrier, so 1 phase later is safe for both wave rows)
//       phase 3: A-lo(t+2) -> buf     (read in phase 1, 2 phases ago)
//       phase 4: B-hi(t+2) -> buf     (read in phase 2, 2 phases ago); then vmcnt(6) retires A-hi(t+1),
//                                      the last half of K-tile t+1, before phase 4's first barrier
//     so K-tile t+1 is complete for every wave before any wave's phase-5 reads (RAW), even for the
//     lagging wave row.
// ------------------------------------------------------------------------------------------------
template <int EPI>
__global__ __launch_bounds__(G_THREADS, 1) void gemm_nt_8ph_kernel(const __bf16* __restrict__ A, const __bf16* __restrict__ B,
                                                                   __bf16* __restrict__ C, const __bf16* __restrict__ bias,
                                                                   int M, int N, int K, EpiArgs e, int group) {
  __shared__ __attribute__((aligned(16))) __bf16 smem[2 * 4 * HALF];  // [buf][A-lo | B-lo | B-hi | A-hi]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 2, wn = wave & 3;
  int tm, tn;
  gemm_tile_of(tm, tn, M / GBM, N / GBN, group);
  const int row0 = tm * GBM, col0 = tn * GBN;
  const int fr = lane & 15, fq = lane >> 4;

  f32x4_t acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  auto slot = [&](int buf, int which) { return smem + (buf * 4 + which) * HALF; };
  // which: 0 A-lo, 1 B-lo, 2 B-hi, 3 A-hi
  auto stage = [&](int t, int which) {
    const int buf = t & 1, k0 = t * GBK;
    if (which == 0) stage_half(A, K, row0, k0, slot(buf, 0), wave, lane, 64, 0);
    else if (which == 1) stage_half(B, K, col0, k0, slot(buf, 1), wave, lane, 32, 0);
    else if (which == 2) stage_half(B, K, col0, k0, slot(buf, 2), wave, lane, 32, 32);
    else stage_half(A, K, row0, k0, slot(buf, 3), wave, lane, 64, 64);
  };
  // operand fragment: image rows r0 .. r0+15, k-half kk
  auto frag = [&](const __bf16* img, int r0, int kk) { return gemm_frag(img, r0 + fr, kk * 4 + fq); };

  const int nk = K / GBK;
  stage(0, 1); stage(0, 0); stage(0, 2); stage(0, 3);
  if (nk > 1) {
    stage(1, 1); stage(1, 0); stage(1, 2);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  asm volatile("s_barrier" ::: "memory");
  if (wm == 1) asm volatile("s_barrier" ::: "memory");

  bf16x8 a[4][2], b0[2][2], b1[2][2];  // [m-tile][kk], [n-tile][kk]
  for (int t = 0; t < nk; ++t) {
    const int buf = t & 1;
    const __bf16* Alo = slot(buf, 0);
    const __bf16* Blo = slot(buf, 1);
    const __bf16* Bhi = slot(buf, 2);
    const __bf16* Ahi = slot(buf, 3);
    const bool s1 = t + 1 < nk, s2 = t + 2 < nk;

    // ---- phase 1: B-lo then A-lo -> quadrant (lo, lo)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) b0[j][kk] = frag(Blo, wn * 32 + j * 16, kk);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) a[i][kk] = frag(Alo, wm * 64 + i * 16, kk);
    if (s1) stage(t + 1, 3);
    // the B reads (issued first: 4 fragments) have retired
    asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
    asm volatile("s_barrier" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][kk], b0[j][kk], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    asm volatile("s_barrier" ::: "memory");

    // ---- phase 2: B-hi -> quadrant (lo, hi)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) b1[j][kk] = frag(Bhi, wn * 32 + j * 16, kk);
    if (s2) stage(t + 2, 1);
    asm volatile("s_barrier" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][kk], b1[j][kk], acc[i][2 + j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    asm volatile("s_barrier" ::: "memory");

    // ---- phase 3: A-hi -> quadrant (hi, hi)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) a[i][kk] = frag(Ahi, wm * 64 + i * 16, kk);
    if (s2) stage(t + 2, 0);
    asm volatile("s_barrier" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[4 + i][2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][kk], b1[j][kk], acc[4 + i][2 + j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    asm volatile("s_barrier" ::: "memory");

    // ---- phase 4: registers only -> quadrant (hi, lo); retire K-tile t+1
    if (s2) {
      stage(t + 2, 2);
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    asm volatile("s_barrier" ::: "memory");
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[4 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][kk], b0[j][kk], acc[4 + i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    asm volatile("s_barrier" ::: "memory");
  }
  if (wm == 0) asm volatile("s_barrier" ::: "memory");
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();
  gemm_store_epilogue<EPI>(acc, smem, C, bias, N, row0, col0, wave, lane, e);
  if (e.drain) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// zero the storage rows that have no sequence position (text padding [T, Tp) and the last image slot)
__global__ void rope_pad_zero_kernel(__bf16* q, __bf16* k, __bf16* v, int Tp, int T, int Np, int BH) {
  const int bh = blockIdx.x, t = threadIdx.x;  // 256 threads: (pad row, 8-chunk)
  const int npad = Tp - T + 1;
  const int pr = t >> 3, ch = t & 7;
  if (pr >= npad) return;
  const int srow = pr < Tp - T ? T + pr : Np - 1;
  const size_t off = ((size_t)bh * Np + srow) * 64 + ch * 8;
  const s16x8 z = {};
  *reinterpret_cast<s16x8*>(q + off) = z;
  *reinterpret_cast<s16x8*>(k + off) = z;
  *reinterpret_cast<s16x8*>(v + off) = z;
}

void rope_pad_zero(void* q, void* k, void* v, int Tp, int T, int Np, int BH, hipStream_t st) {
  hipLaunchKernelGGL(rope_pad_zero_kernel, dim3(BH), dim3(256), 0, st, (__bf16*)q, (__bf16*)k, (__bf16*)v, Tp, T, Np, BH);
}

int gemm_cpol();   // gemm_pt.hip
int gemm_drain();  // gemm_pt.hip

// variant 0 = the simple kernel; 200..207 = the 4-phase kernel; otherwise the 8-phase kernel, the variant picking its
// tile order:
// 300 -> column groups of 4, 301..332 -> column groups of (variant - 300), 400 + g -> row groups of g
bool gemm_nt(const void* A, const void* B, void* C, const void* bias, int M, int N, int K, int variant, hipStream_t st) {
  if (M % GBM || N % GBN || K % GBK) return false;
  const int nwg = (M / GBM) * (N / GBN);
  if (variant == 0) {
    hipLaunchKernelGGL(gemm_nt_kernel, dim3(nwg), dim3(G_THREADS), 0, st, (const __bf16*)A, (const __bf16*)B, (__bf16*)C,
                       (const __bf16*)bias, M, N, K);
    return true;
  }
  EpiArgs e{};
  if (variant >= 200 && variant < 208) {
    switch (variant - 200) {
#define PHASED_CASE(o)                                                                                                   \
  case o:                                                                                                                \
    hipLaunchKernelGGL((gemm_nt_phased_kernel<0, o>), dim3(nwg), dim3(G_THREADS), 0, st, (const __bf16*)A, (const __bf16*)B, \
                       (__bf16*)C, (const __bf16*)bias, M, N, K, e);                                                     \
    break;
      PHASED_CASE(0) PHASED_CASE(1) PHASED_CASE(2) PHASED_CASE(3) PHASED_CASE(4) PHASED_CASE(5) PHASED_CASE(6) PHASED_CASE(7)
#undef PHASED_CASE
    }
    return true;
  }
  int group;
  if (variant >= 300 && variant < 333) {
    group = variant == 300 ? 4 : variant - 300;
    e.cpol = (size_t)M * N * 2 < (1ull << 32) ? gemm_cpol() : 0;  // buffer stores: 32-bit byte offsets
    e.drain = gemm_drain();
  } else if (variant > 400 && variant < 433) {
    group = -(variant - 400);
  } else {
    return false;
  }
  hipLaunchKernelGGL((gemm_nt_8ph_kernel<0>), dim3(nwg), dim3(G_THREADS), 0, st, (const __bf16*)A, (const __bf16*)B,
                     (__bf16*)C, (const __bf16*)bias, M, N, K, e, group);
  return true;
}

// FF-out dgrad with the GEGLU backward in the epilogue: du = dy (M, K) . W2^T where w2t = W2^T (F, K)
// bf16, then dh (M, 2F) = GEGLU'(h, du) and part ((M / 128), 2F) = partial FF-in bias grads. The
// (M, F) du intermediate never exists.
bool gemm_geglu_bwd(const void* dy, const void* w2t, const void* h, void* dh, float* part, int M, int F, int K,
                    hipStream_t st) {
  if (M % GBM || F % GBN || K % GBK) return false;
  EpiArgs e{};
  e.gh = (const __bf16*)h;
  e.gdh = (__bf16*)dh;
  e.gpart = part;
  e.F = F;
  e.cpol = (size_t)M * F * 4 < (1ull << 32) ? gemm_cpol() : 0;  // buffer stores: 32-bit byte offsets
  e.drain = gemm_drain();
  const int nwg = (M / GBM) * (F / GBN);
  hipLaunchKernelGGL((gemm_nt_8ph_kernel<2>), dim3(nwg), dim3(G_THREADS), 0, st, (const __bf16*)dy, (const __bf16*)w2t,
                     (__bf16*)nullptr, (const __bf16*)nullptr, M, F, K, e, 4);
  return true;
}

// QKV projection + rotary into the attention storage layout (q pre-scaled); M = B*n rows
bool gemm_qkv_rope(const void* A, const void* W, void* q, void* k, void* v, const float* cosT, const float* sinT, int M, int K,
                   int H, int T, int S, int n, int col_major, float qscale, hipStream_t st) {
  const int N = 3 * H * 64;
  if (M % GBM || N % GBN || K % GBK || M % n) return false;
  int logS = 0;
  while ((1 << logS) < S) ++logS;
  const int Tp = (T + 31) / 32 * 32;
  EpiArgs e{(__bf16*)q, (__bf16*)k, (__bf16*)v, cosT, sinT, T, Tp, S, logS, n, Tp + S * S, H, col_major, qscale};
  e.cpol = (size_t)M * N * 4 < (1ull << 32) ? gemm_cpol() : 0;  // buffer stores: 32-bit byte offsets
  e.drain = gemm_drain();
  const int nwg = (M / GBM) * (N / GBN);
  // 8-phase staggered template: 1073 vs 1042 TF for the phased kernel at M=61440, N=3072, K=1024
  // (profiles/r1_gemm_8phase.jsonl)
  hipLaunchKernelGGL((gemm_nt_8ph_kernel<1>), dim3(nwg), dim3(G_THREADS), 0, st, (const __bf16*)A, (const __bf16*)W,
                     (__bf16*)nullptr, (const __bf16*)nullptr, M, N, K, e, 4);
  const int BH = (M / n) * H;
  hipLaunchKernelGGL(rope_pad_zero_kernel, dim3(BH), dim3(256), 0, st, (__bf16*)q, (__bf16*)k, (__bf16*)v, Tp, T, Tp + S * S, BH);
  return true;
}

}  // namespace dalle
