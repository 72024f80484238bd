// bf16 GEMM with register-direct fused epilogues (SURVEY K5/K6 GEMM + epilogue fusion target).
//
//   C[M, N] = A[M, K] . B[N, K]^T     (both operands K-contiguous; fp32 accumulate)
//
// Main loop: the 256 x 256 x 64 8-phase schedule of gemm.hip (8 waves, 2 along M x 4 along N, half-tile
// LDS-DMA images, counted vmcnt, the two wave rows staggered by one barrier), with one change that targets
// the epilogue, which cost the LDS-staged kernel 16-26 % of its time
// (profiles/r2_gemm_epilogue_cost.jsonl):
//
//   Transposed accumulators: the MFMA is issued as B-fragment x A-fragment, so every lane ends up holding
//   4 CONSECUTIVE output columns of one row (C^T layout) instead of 4 rows of one column. The epilogue
//   converts straight from the accumulators: no LDS staging pass (no 2-byte ds_write per element), and
//   v_permlane16_swap pairs two 16-column sub-tiles so each lane issues one 16-byte store per pair.
//
// Epilogues (template EPI): 0 = bf16 store (+bias), 1 = QKV + 3-axis rotary scattered into the attention
// storage (q pre-scaled). The training step runs its GEMMs on the generated assembly kernels (csrc/asm);
// this file serves d_model < 1024 and DALLE_AMD_ASM_GEMM=0, where production reaches EPI 1 (qkv_rope_pt);
// EPI 0 (gemm_pt) is the tested main loop that EPI 1 shares.
//
// "pt" stands for "persistent tiles": one workgroup per CU walking its tiles (template PERSIST). Production
// runs one tile per workgroup, which measured faster at the training shapes
// (profiles/r3_gemm_pt_vs_hipblaslt_8ph.jsonl, pt_* vs np_* columns); the persistent form is kept for the tests
// that hold both forms to the same results. Measured and rejected, the code removed (numbers under profiles/):
//   * the persistent form with the finished tile's stores deferred past the next tile's first DMA, with and
//     without a start stagger: slower at every shape (r4_gemm_overlap.jsonl);
//   * a start-time stagger of the first wave of workgroups: slower on every training shape
//     (r3_gemm_stagger.jsonl);
//   * 16 rows x 64 B plain stores instead of whole 128-B lines: 14-15 vs 41-51 B/clk of store issue per CU
//     (r4_store_patterns.jsonl, r4_gemm_lines_b128.jsonl); the form survives only where the QKV epilogue
//     needs it (n % 16 != 0);
//   * the FF GEGLU epilogues (forward and backward) on this main loop: production serves them from the
//     assembly kernels and, in the fallback, from gemm.hip;
//   * per-workgroup timestamps and a no-store epilogue were measurement builds
//     (r3_gemm_epilogue_stamps.jsonl, r3_gemm_epilogue_grid.jsonl).
#include "common.h"

namespace dalle {

namespace pt {

typedef __attribute__((ext_vector_type(4))) float f4;
constexpr int BM = 256, BN = 256, BK = 64;
constexpr int THREADS = 512;
constexpr int HALF = 128 * BK;  // elements of one half-tile image (128 operand rows x 64 k)

__device__ __forceinline__ int swz(int r) { return (r >> 1) & 7; }

// Half-tile image of 128 operand rows (see gemm.hip stage_half): image row hr <-> tile row
// (hr / blk) * 2 blk + off + hr % blk; the 16-byte chunk index is XOR-swizzled by image row on the
// per-lane SOURCE address (the DMA writes LDS lane-linearly).
__device__ __forceinline__ void stage_half(const __bf16* __restrict__ src, int ld, int row0, int k0, __bf16* lds_half,
                                           int wave, int lane, int blk, int off) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int piece = wave * 2 + i;
    const int hr = piece * 8 + (lane >> 3);
    const int row = (hr / blk) * 2 * blk + off + (hr % blk);
    const int lchunk = (lane & 7) ^ swz(hr);
    const __bf16* g = src + (size_t)(row0 + row) * ld + k0 + lchunk * 8;
    __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)g,
                                     (void __attribute__((address_space(3)))*)(lds_half + piece * 512), 16, 0, 0);
  }
}

__device__ __forceinline__ bf16x8 frag(const __bf16* tile, int row, int chunk) {
  return *reinterpret_cast<const bf16x8*>(tile + row * 64 + ((chunk ^ swz(row)) << 3));
}

// tile id (= workgroup id) -> (tm, tn): XCD slot first (blocks b and b + 8 share an XCD: when the tile count
// is a multiple of 8 each XCD gets a contiguous range), then column groups of `group` panels swept along M
// (group > 0) or row groups of -group panels swept along N (group < 0)
__device__ __forceinline__ void tile_of(int id, int tiles_m, int tiles_n, int group, int& tm, int& tn) {
  const int nwg = tiles_m * tiles_n;
  if ((nwg & 7) == 0) id = (id & 7) * (nwg >> 3) + (id >> 3);
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

__device__ __forceinline__ unsigned pk2(float a, float b) {
  const __bf16 x = (__bf16)a, y = (__bf16)b;
  return (unsigned)__builtin_bit_cast(unsigned short, x) | ((unsigned)__builtin_bit_cast(unsigned short, y) << 16);
}
__device__ __forceinline__ float lo_f(unsigned v) { return __uint_as_float(v << 16); }
__device__ __forceinline__ float hi_f(unsigned v) { return __uint_as_float(v & 0xffff0000u); }

// v_permlane16_swap: rows (16 lanes) 1 and 3 of x trade places with rows 0 and 2 of y. Applied to
// the packed columns of sub-tiles j (x) and j + 1 (y) it leaves lanes of row q = 0, 2 holding 8
// consecutive columns of j and lanes of row 1, 3 holding 8 consecutive columns of j + 1; the swap is
// an involution, so the same call turns 16-byte loads of that arrangement back into per-lane columns.
__device__ __forceinline__ void swap16(unsigned& x, unsigned& y) {
  const auto r = __builtin_amdgcn_permlane16_swap(x, y, false, false);
  x = r[0];
  y = r[1];
}

// DPP row_ror:8 -- lane l of every 16-lane row reads lane (l + 8) & 15 of the same row
__device__ __forceinline__ unsigned ror8(unsigned v) { return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xf, 0xf, false); }

// Whole-line re-layout of one 16-row sub-tile (round 4, profiles/r4_store_patterns.jsonl): on entry lane
// (fr, q) holds two 16-byte chunks of ITS row fr, c0 from column pair jp = 0 and c1 from jp = 1 (the
// layout after swap16); on exit c0 is the chunk of row (fr & 7) and c1 the chunk of row 8 + (fr & 7), both
// at element column lines_col(lane) of the wave's 64. The lanes of row halves fr < 8 / fr >= 8 trade their
// jp = 1 / jp = 0 chunks through one DPP row rotate per dword, so each store instruction covers 8 rows x
// 128 B (whole lines) instead of 16 rows x 64 B: 41-51 vs 14-15 B/clk of store issue per CU.
__device__ __forceinline__ void lines16(u32x4_vs& c0, u32x4_vs& c1, bool low) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned r = ror8(low ? c1[k] : c0[k]);
    const unsigned a = low ? c0[k] : r, b = low ? r : c1[k];
    c0[k] = a;
    c1[k] = b;
  }
}
__device__ __forceinline__ int lines_col(int lane) {
  const int fr = lane & 15, q = lane >> 4;
  return (fr >> 3) * 32 + (q & 1) * 16 + (q >> 1) * 8;
}

// epilogue output stream: a wave-uniform base, its buffer descriptor and the store cache policy
struct Out {
  __bf16* base;
  __amdgpu_buffer_rsrc_t rsrc;
  int cpol;
  __device__ __forceinline__ Out(__bf16* b, int cp) : base(b), rsrc(uniform_rsrc(b)), cpol(cp) {}
  __device__ __forceinline__ void st(__bf16* p, unsigned x0, unsigned x1, unsigned y0, unsigned y1) const {
    const u32x4_vs v = {x0, x1, y0, y1};
    cstore16(base, rsrc, (uint32_t)((char*)p - (char*)base), v, cpol);
  }
  __device__ __forceinline__ void st4(__bf16* p, const u32x4_vs& v) const {
    cstore16(base, rsrc, (uint32_t)((char*)p - (char*)base), v, cpol);
  }
};

}  // namespace pt

struct PtArgs {
  // EPI 0: C (M, ldc) bf16 (+ bias (N,) bf16, may be null)
  __bf16* C;
  const __bf16* bias;
  int ldc;
  // EPI 1 (QKV + rotary): storage (B*H, Np, 64); cs (n + 1, 32, 2) fp32 = (cos, sin) per rotary pair
  __bf16* q;
  __bf16* k;
  __bf16* v;
  const float* cs;
  int T, Tp, S, logS, n, Np, H, col_major;
  float qscale;
  int group;  // tile order (pt::tile_of)
  int cpol;   // cache policy of the output stores (common.h cstore16)
  int drain;  // wait for the output stores before the workgroup ends (gemm_set_drain)
};

__device__ __forceinline__ int pt_seq2st(const PtArgs& e, int p) {
  if (p < e.T) return p;
  const int kk = p - e.T;
  const int kst = e.col_major ? ((kk & (e.S - 1)) << e.logS) + (kk >> e.logS) : kk;
  return e.Tp + kst;
}

// Epilogue of one finished tile (origin r0, c0) straight from the transposed accumulators: lane l of
// wave (wm, wn) holds, for sub-tile (i, j), row r0 + wm*128 + i*16 + (l & 15) and the 4 columns
// c0 + wn*64 + j*16 + (l >> 4)*4 + 0..3.
template <int EPI, bool LINES>
__device__ __forceinline__ void pt_epilogue(pt::f4 (&acc)[8][4], int r0, int c0, int wm, int wn, int lane, const PtArgs& e) {
  using namespace pt;
  const int fr = lane & 15, q = lane >> 4;
  const int cw = c0 + wn * 64;  // first column of the wave's 64
  if constexpr (EPI == 0) {
    static_assert(LINES, "the plain store always goes out in whole lines");
    const pt::Out oc(e.C, e.cpol);
    float bv[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) bv[j][r] = 0.f;
    if (e.bias != nullptr) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint2 b = *reinterpret_cast<const uint2*>(e.bias + cw + j * 16 + q * 4);
        bv[j][0] = lo_f(b.x); bv[j][1] = hi_f(b.x); bv[j][2] = lo_f(b.y); bv[j][3] = hi_f(b.y);
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      u32x4_vs ch[2];
#pragma unroll
      for (int jp = 0; jp < 2; ++jp) {
        const int j0 = 2 * jp, j1 = j0 + 1;
        unsigned x0 = pk2(acc[i][j0][0] + bv[j0][0], acc[i][j0][1] + bv[j0][1]);
        unsigned x1 = pk2(acc[i][j0][2] + bv[j0][2], acc[i][j0][3] + bv[j0][3]);
        unsigned y0 = pk2(acc[i][j1][0] + bv[j1][0], acc[i][j1][1] + bv[j1][1]);
        unsigned y1 = pk2(acc[i][j1][2] + bv[j1][2], acc[i][j1][3] + bv[j1][3]);
        swap16(x0, y0);
        swap16(x1, y1);
        ch[jp] = u32x4_vs{x0, x1, y0, y1};
      }
      lines16(ch[0], ch[1], fr < 8);
      __bf16* lp = e.C + (size_t)(r0 + wm * 128 + i * 16 + (fr & 7)) * e.ldc + cw + lines_col(lane);
      oc.st4(lp, ch[0]);
      oc.st4(lp + (size_t)8 * e.ldc, ch[1]);
    }
  } else if constexpr (EPI == 1) {
    // the wave's 64 columns are one (part, head); rotary pairs (2t, 2t+1) sit in one lane
    const int HD = e.H * 64;
    const int part = cw / HD, hh = (cw - part * HD) >> 6;
    __bf16* dstT = part == 0 ? e.q : (part == 1 ? e.k : e.v);
    const float sc = part == 0 ? e.qscale : 1.0f;
    const pt::Out oc(dstT, e.cpol);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = r0 + wm * 128 + i * 16 + fr;
      const int b = r / e.n, p = r - b * e.n;
      __bf16* rowp = dstT + ((size_t)(b * e.H + hh) * e.Np + pt_seq2st(e, p)) * 64 + (q & 2) * 4;
      const float* csp = e.cs + (size_t)p * 64 + q * 4;  // (cos, sin) of pairs j*8 + 2q, j*8 + 2q + 1
      f4 t[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) t[j] = *reinterpret_cast<const f4*>(csp + j * 16);
      unsigned w[4][2];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float x0 = acc[i][j][0], x1 = acc[i][j][1], x2 = acc[i][j][2], x3 = acc[i][j][3];
        w[j][0] = pk2((x0 * t[j][0] - x1 * t[j][1]) * sc, (x1 * t[j][0] + x0 * t[j][1]) * sc);
        w[j][1] = pk2((x2 * t[j][2] - x3 * t[j][3]) * sc, (x3 * t[j][2] + x2 * t[j][3]) * sc);
      }
#pragma unroll
      for (int jp = 0; jp < 2; ++jp) {
        const int j0 = 2 * jp, j1 = j0 + 1;
        swap16(w[j0][0], w[j1][0]);
        swap16(w[j0][1], w[j1][1]);
        if constexpr (!LINES) oc.st(rowp + ((q & 1) ? j1 : j0) * 16, w[j0][0], w[j0][1], w[j1][0], w[j1][1]);
      }
      if constexpr (LINES) {
        // the 16 rows of a sub-tile are 16 consecutive positions of one sample (n % 16 == 0, host-checked)
        u32x4_vs c0v = {w[0][0], w[0][1], w[1][0], w[1][1]}, c1v = {w[2][0], w[2][1], w[3][0], w[3][1]};
        lines16(c0v, c1v, fr < 8);
        const int p0 = p - (fr & 8);
        __bf16* base = dstT + (size_t)(b * e.H + hh) * e.Np * 64 + lines_col(lane);
        oc.st4(base + (size_t)pt_seq2st(e, p0) * 64, c0v);
        oc.st4(base + (size_t)pt_seq2st(e, p0 + 8) * 64, c1v);
      }
      __builtin_amdgcn_sched_barrier(0);  // bound the live loads to one row sub-tile
    }
  }
}

// PERSIST = true: one workgroup per CU walks its tiles (grid = pt_grid), the DMA stream running on across tile
// boundaries and a finished tile's epilogue issued while the next tile's first K-steps are in flight.
// PERSIST = false (what production runs): one tile per workgroup (grid = tile count), the same main loop and
// epilogue -- a workgroup's stores then drain while the NEXT workgroup on that CU already streams its first
// K-tiles.
template <int EPI, bool PERSIST, bool LINES>
__global__ __launch_bounds__(pt::THREADS, 1) void gemm_pt_kernel(const __bf16* __restrict__ A, const __bf16* __restrict__ B,
                                                                 int M, int N, int K, PtArgs e) {
  using namespace pt;
  // [buf][A-lo | B-lo | B-hi | A-hi] half-tile images, 128 KiB in ONE array (a second __shared__
  // object can make hipcc drain vmcnt before every ds_read)
  __shared__ __attribute__((aligned(16))) __bf16 smem[2 * 4 * HALF];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 2, wn = wave & 3;
  const int tiles_m = M / BM, tiles_n = N / BN, ntiles = tiles_m * tiles_n;
  const int nk = K / BK;  // >= 2 (host-checked)
  const int G = gridDim.x;
  const int my_tiles = PERSIST ? (ntiles - (int)blockIdx.x + G - 1) / G : 1;
  const int total = my_tiles * nk;

  auto origin = [&](int it, int& r0, int& c0) {
    int tm, tn;
    tile_of((int)blockIdx.x + it * G, tiles_m, tiles_n, e.group, tm, tn);
    r0 = tm * BM;
    c0 = tn * BN;
  };
  auto slot = [&](int buf, int which) { return smem + (buf * 4 + which) * HALF; };
  // which: 0 A-lo, 1 B-lo, 2 B-hi, 3 A-hi
  auto stage = [&](int r0, int c0, int kt, int buf, int which) {
    const int k0 = kt * BK;
    if (which == 0) stage_half(A, K, r0, k0, slot(buf, 0), wave, lane, 64, 0);
    else if (which == 1) stage_half(B, K, c0, k0, slot(buf, 1), wave, lane, 32, 0);
    else if (which == 2) stage_half(B, K, c0, k0, slot(buf, 2), wave, lane, 32, 32);
    else stage_half(A, K, r0, k0, slot(buf, 3), wave, lane, 64, 64);
  };
  auto fragA = [&](const __bf16* img, int i, int kk) { return frag(img, wm * 64 + i * 16 + (lane & 15), kk * 4 + (lane >> 4)); };
  auto fragB = [&](const __bf16* img, int j, int kk) { return frag(img, wn * 32 + j * 16 + (lane & 15), kk * 4 + (lane >> 4)); };

  int cr, cc, nr, nc;  // origins of the current and the next tile
  origin(0, cr, cc);
  if (my_tiles > 1) origin(1, nr, nc);
  else { nr = cr; nc = cc; }

  // prologue: K-step 0 complete, three halves of K-step 1 in flight
  stage(cr, cc, 0, 0, 1); stage(cr, cc, 0, 0, 0); stage(cr, cc, 0, 0, 2); stage(cr, cc, 0, 0, 3);
  stage(cr, cc, 1, 1, 1); stage(cr, cc, 1, 1, 0); stage(cr, cc, 1, 1, 2);
  asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  asm volatile("s_barrier" ::: "memory");
  if (wm == 1) asm volatile("s_barrier" ::: "memory");

  f4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

  bf16x8 a[4][2], b0[2][2], b1[2][2];
  int pr = 0, pc = 0;  // origin of the finished tile whose epilogue is pending
  int g = 0;
  for (int it = 0; it < my_tiles; ++it) {
    for (int kt = 0; kt < nk; ++kt, ++g) {
      const int buf = g & 1;
      const __bf16* Alo = slot(buf, 0);
      const __bf16* Blo = slot(buf, 1);
      const __bf16* Bhi = slot(buf, 2);
      const __bf16* Ahi = slot(buf, 3);
      // sources of K-steps g + 1 and g + 2 (the next tile's first K-steps near the end of a tile)
      const bool x1 = PERSIST && kt + 1 >= nk, x2 = PERSIST && kt + 2 >= nk;
      const int r1 = x1 ? nr : cr, c1 = x1 ? nc : cc, k1 = x1 ? kt + 1 - nk : kt + 1;
      const int r2 = x2 ? nr : cr, c2 = x2 ? nc : cc, k2 = x2 ? kt + 2 - nk : kt + 2;
      const bool s1 = g + 1 < total, s2 = g + 2 < total;

      // ---- phase 1: B-lo then A-lo -> quadrant (lo, lo)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) b0[j][kk] = fragB(Blo, j, kk);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) a[i][kk] = fragA(Alo, i, kk);
      if (s1) stage(r1, c1, k1, buf ^ 1, 3);
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
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b0[j][kk], a[i][kk], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      asm volatile("s_barrier" ::: "memory");

      // ---- phase 2: B-hi -> quadrant (lo, hi)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) b1[j][kk] = fragB(Bhi, j, kk);
      if (s2) stage(r2, c2, k2, buf, 1);
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
            acc[i][2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b1[j][kk], a[i][kk], acc[i][2 + j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      asm volatile("s_barrier" ::: "memory");

      // ---- phase 3: A-hi -> quadrant (hi, hi)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) a[i][kk] = fragA(Ahi, i, kk);
      if (s2) stage(r2, c2, k2, buf, 0);
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
            acc[4 + i][2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b1[j][kk], a[i][kk], acc[4 + i][2 + j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      asm volatile("s_barrier" ::: "memory");

      // ---- phase 4: registers only -> quadrant (hi, lo); retire K-step g + 1
      if (s2) {
        stage(r2, c2, k2, buf, 2);
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
            acc[4 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b0[j][kk], a[i][kk], acc[4 + i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      asm volatile("s_barrier" ::: "memory");
    }
    // ---- the finished tile's epilogue, straight from the accumulators (no LDS), while the next tile's
    // first K-steps are in flight; then re-zero
    if (it + 1 < my_tiles) {
      __builtin_amdgcn_sched_barrier(0);
      pt_epilogue<EPI, LINES>(acc, cr, cc, wm, wn, lane, e);
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
      __builtin_amdgcn_sched_barrier(0);
    }
    pr = cr;
    pc = cc;
    cr = nr;
    cc = nc;
    if (it + 2 < my_tiles) origin(it + 2, nr, nc);
  }
  if (wm == 0) asm volatile("s_barrier" ::: "memory");
  pt_epilogue<EPI, LINES>(acc, pr, pc, wm, wn, lane, e);
  if (e.drain) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// cache policy of every hand-written GEMM's output stores (common.h cstore16), 0 = plain stores; set at run
// time by gemm_set_cpol (benchmarks, tests)
static int g_gemm_cpol = 0;
void gemm_set_cpol(int c) { g_gemm_cpol = c; }
int gemm_cpol() { return g_gemm_cpol; }

// every hand-written GEMM workgroup waits for its output stores (s_waitcnt vmcnt(0)) before it ends: a
// one-tile-per-workgroup GEMM whose waves end with their epilogue stores still in flight runs 4-11 % slower
// than the same kernel draining them first (profiles/r3_gemm_epilogue_stamps.jsonl); gemm_set_drain
// overrides it at run time
static int g_gemm_drain = 1;
void gemm_set_drain(int d) { g_gemm_drain = d; }
int gemm_drain() { return g_gemm_drain; }

// one workgroup per CU (128 KiB of LDS); a multiple of 8 keeps each workgroup on one XCD's range
static int pt_grid(int ntiles) {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (cus <= 0) cus = 256;
  }
  int g = cus < ntiles ? cus : ntiles;
  if (g > 8 && ntiles > g) g &= ~7;
  return g;
}

template <int EPI, bool LINES>
static void pt_launch(const void* A, const void* B, int M, int N, int K, PtArgs& e, hipStream_t st, bool persist) {
  const int ntiles = (M / pt::BM) * (N / pt::BN);
  // buffer-store policies address the output with a 32-bit byte offset: plain stores past 2 GiB of output
  e.cpol = (size_t)M * N * 4 < (1ull << 32) ? g_gemm_cpol : 0;
  e.drain = g_gemm_drain;
  if (persist)
    hipLaunchKernelGGL((gemm_pt_kernel<EPI, true, LINES>), dim3(pt_grid(ntiles)), dim3(pt::THREADS), 0, st, (const __bf16*)A,
                       (const __bf16*)B, M, N, K, e);
  else
    hipLaunchKernelGGL((gemm_pt_kernel<EPI, false, LINES>), dim3(ntiles), dim3(pt::THREADS), 0, st, (const __bf16*)A,
                       (const __bf16*)B, M, N, K, e);
}

static bool pt_shape_ok(int M, int N, int K) { return M > 0 && N > 0 && M % pt::BM == 0 && N % pt::BN == 0 && K % pt::BK == 0 && K >= 2 * pt::BK; }

// C (M, ldc) = A B^T (+ bias); variant 0 or 10 = one tile per workgroup, 20 = persistent; group = tile order
// (0: the default, column groups of 4)
bool gemm_pt(const void* A, const void* B, void* C, const void* bias, int M, int N, int K, int ldc, int variant, int group,
             hipStream_t st) {
  if (!pt_shape_ok(M, N, K) || ldc < N || ldc % 8) return false;
  if (variant != 0 && variant != 10 && variant != 20) return false;
  PtArgs e{};
  e.C = (__bf16*)C;
  e.bias = (const __bf16*)bias;
  e.ldc = ldc;
  e.group = group ? group : 4;
  pt_launch<0, true>(A, B, M, N, K, e, st, variant == 20);
  return true;
}

// QKV projection + rotary into the attention storage layout (q pre-scaled); cs = (n + 1, 32, 2) fp32;
// persist = 1: the persistent form (tests), otherwise one tile per workgroup
bool gemm_pt_qkv_rope(const void* A, const void* W, void* q, void* k, void* v, const float* cs, int M, int K, int H, int T,
                      int S, int n, int col_major, float qscale, hipStream_t st, int persist) {
  const int N = 3 * H * 64;
  if (!pt_shape_ok(M, N, K) || M % n) return false;
  int logS = 0;
  while ((1 << logS) < S) ++logS;
  PtArgs e{};
  e.q = (__bf16*)q;
  e.k = (__bf16*)k;
  e.v = (__bf16*)v;
  e.cs = cs;
  e.T = T;
  e.Tp = (T + 31) / 32 * 32;
  e.S = S;
  e.logS = logS;
  e.n = n;
  e.Np = e.Tp + S * S;
  e.H = H;
  e.col_major = col_major;
  e.qscale = qscale;
  e.group = 4;
  // whole-line stores pair rows 8 apart inside a 16-row sub-tile: one sample's positions when n % 16 == 0
  if (n % 16 == 0) pt_launch<1, true>(A, W, M, N, K, e, st, persist == 1);
  else pt_launch<1, false>(A, W, M, N, K, e, st, persist == 1);
  return true;
}

// device probe of the v_permlane16_swap lane convention the epilogues rely on: out[0:64] = x, out[64:128] = y
// after swap16(x = lane, y = 100 + lane)
__global__ void permlane16_probe_kernel(unsigned* out) {
  unsigned x = threadIdx.x, y = 100 + threadIdx.x;
  pt::swap16(x, y);
  out[threadIdx.x] = x;
  out[64 + threadIdx.x] = y;
}
void permlane16_probe(unsigned* out, hipStream_t st) { hipLaunchKernelGGL(permlane16_probe_kernel, dim3(1), dim3(64), 0, st, out); }

}  // namespace dalle
