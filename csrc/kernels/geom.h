// Launch geometry structs shared by the HIP kernels and the (host-compiled) bindings.
#pragma once
#include <stdint.h>
namespace dalle {
struct AttnGeom {
  int T;        // text positions incl. BOS (257)
  int Tp;       // padded text rows (288)
  int S;        // image side (32)
  int logS;     // log2(S)
  int I;        // S*S
  int Np;       // Tp + I
  int n;        // unpadded sequence length (1280)
  int K;        // conv window
  int H;        // heads
  int pattern;  // 0 full, 1 axial_row, 2 axial_col, 3 conv_like
};
struct RopeGeom {
  int T, Tp, S, logS, n, Np, H, col_major;
};
struct DecodeGeom {
  int T;        // text positions incl. BOS
  int S;        // image side
  int n;        // cache length (seq_len)
  int H;        // heads
  int K;        // conv window
  int pattern;  // 0 full, 1 axial_row, 2 axial_col, 3 conv_like
};
struct ShiftGeom {
  int n;      // sequence length
  int T;      // text_len (BOS + text)
  int S;      // image side
  int shift;  // 0 = plain LayerNorm
};
// VQGAN 3x3 convolution (conv.hip): bf16 tensors passed as void pointers (host-compiled header)
struct ConvArgs {
  const void* x;       // [N, Hs, Ws, Cin] NHWC (Hs = H / 2 when ups)
  const void* w;       // [Cout, 9 * Cin] tap-major, channel-contiguous
  const float* bias;   // [Cout] or nullptr
  const void* res;     // [N, H, W, Cout] or nullptr
  void* y;             // [N, H, W, Cout]
  const float* mean;   // [N, 32] GroupNorm statistics (gn)
  const float* rstd;   // [N, 32]
  const float* gamma;  // [Cin]
  const float* beta;   // [Cin]
  int N, H, W, Cin, Cout, ups, gn;
  int down;            // stride-2 Downsample: x is [N, 2H, 2W, Cin], zero pad right / bottom (no ups / gn / res)
};

// Destination of a column-reduced parameter gradient (see column_sum_kernel)
struct GradSink {
  float* out0;        // columns [0, split)
  float* out1;        // columns [split, width) (nullptr: dropped)
  const float* mul1;  // optional per-column multiplier for out1
  int split;
  int accumulate;     // 1: dst += v (the fp32 grad arena), 0: dst = v
};

// Decode-step skinny GEMM (skinny.hip): Y (M <= 64, N) = X (M, K) . W (N, K)^T + fused epilogue.
// bf16 operands are passed as void pointers (this header is also compiled by the host compiler).
struct SkinnyArgs {
  const void* X;
  const void* W;
  const void* bias;  // bf16, may be null
  int M, N, K, ldx;  // N: output columns (F for GEGLU: W holds 2F rows)
  int KS;            // cross-workgroup split-K factor (must equal skinny_ks(M, N, K, G))
  int steps;         // 128-wide K chunks per wave (set by skinny_gemm)
  float* ws;         // KS * (N / 16) * ceil16(M) * 16 * (1 or 2) floats
  int* cnt;          // >= N / 16 zero-initialised counters (self-resetting)
  void* out;         // EPI 0 (bf16 or fp32), EPI 1 (bf16), EPI 4 (fp32 slabs (KS, M, N))
  int out_f32;
  float* resid;        // EPI 2: resid += scale * (y + bias), fp32 (M, N)
  const float* scale;
  void* q;           // EPI 3: rotary q (pre-scaled) -> q (M*H, 64); k, v -> caches (M*H, n, 64) at *pos
  void* kc;
  void* vc;
  const float* cosT;
  const float* sinT;
  const int* pos;
  int H, n;
  float qscale;
};

// Fused decode sampler (sample.hip): top-k / top-p / temperature / Gumbel-max + token bookkeeping.
struct SampleArgs {
  const float* logits;  // (B, V) fp32
  int B, V;
  int top_k;            // <= 0 or >= V: off
  float top_p;          // >= 1: off
  float temperature;    // <= 1e-10: greedy
  const int64_t* seed;  // device scalar
  const int* pos;       // device scalar: the position this step ran
  const int64_t* text;  // (B, T) caption ids (BOS first)
  int T, img_len;
  int64_t vt;           // text vocabulary size (image token id offset)
  int64_t* codes;       // (B, img_len), may be null
  int64_t* tok;         // (B,) next input token, may be null
  int64_t* sampled;     // (B,) the raw sample, may be null
  const int64_t* prime; // (B, img_len) forced image codes, may be null
  const int* n_prime;   // device scalar: image positions [0, *n_prime) take prime's code instead of the sample
  const uint8_t* keep;  // (pictures, img_len), may be null: nonzero = this position takes prime's code too
  // classifier-free guidance (may be null: off). With it B = 2 b rows: [0, b) conditional, [b, 2 b) unconditional;
  // workgroup r samples from u + *cond_scale * (c - u) of rows r / r + b and writes both rows' codes and tokens
  const float* cond_scale;  // device scalar
  int b;                    // pictures (guided only)
  // per-picture sampling parameters (all null: off; else all given, row_cond_scale when guided). Workgroup r reads
  // entry r of each in place of top_k / top_p / temperature / *seed / *cond_scale above
  const float* row_temperature;  // (pictures,)
  const int* row_top_k;          // (pictures,)
  const float* row_top_p;        // (pictures,)
  const int64_t* row_seed;       // (pictures,)
  const int* noise_row;          // (pictures,) the row of the noise key (seed, position, row, token), 24 bits
  const float* row_cond_scale;   // (pictures,), guided only
};

}  // namespace dalle
