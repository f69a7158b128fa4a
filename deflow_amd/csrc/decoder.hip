// LinearDecoder forward ([REF decoder.py:72-120]) as one fused kernel, and the weight-row split of the ConvGRU decoder's
// bf16x2 form.  (The ConvGRU decoder itself: decoder4.hip, lean, and decoder3.hip, all planes saved.)
//
// One workgroup = 64 valid pc0 points (4 waves x 16 points).  [before | after | offset encoding] of a wave's 16 points sits in a
// wave-private LDS region that is the A operand of the hidden layer's GEMM (v_mfma_f32_16x16x4_f32, exact f32); the weight rows
// are streamed L2 -> registers -> LDS in 32-deep k chunks, double buffered, and shared by the four waves (gemm_stream.h).
// Gather is one contiguous 256-byte read per point per image (NHWC), instead of the reference's 128 strided 4-byte reads from
// NCHW [REF decoder.py:165-168].
//
// k permutation: MFMA step s of a 16-wide k group uses k = 16g + 4*(lane>>4) + s on both operands,
// so every fragment fetch is one ds_read_b128.
#include "common.h"
#include "gemm_stream.h"

namespace {

using namespace gs;

// ------------------------------------------------------------------------- LinearDecoder ---
// [REF decoder.py:72-120]: flow = W2 gelu(W1 [before | after | offset_enc(128)] + b1) + b2.  K = 256.
struct LinFwdParams {
  df_img before, after;
  const int32_t* coords;
  const float* offs;
  const int32_t* counts;
  int N;
  const float *w_off, *b_off, *w_1, *b_1, *w_2, *b_2;
  float* flow;
};
constexpr int LDA_L = 260;
constexpr int BSZ_L = 32 * LDB;  // B buffer of the 32-row weight tile  // 384 + 4; 97 slots of 16 B, 97 mod 16 = 1

__global__ __launch_bounds__(256) void linear_fwd_kernel(LinFwdParams p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* Bs = lds;
  float* As = lds + 2 * BSZ_L;  // [4][16][LDA_L]
  const int b = blockIdx.y;
  const int cnt = p.counts[b];
  const int p0 = blockIdx.x * 64;
  if (p0 >= cnt) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lq = lane >> 4;
  float* Aw = As + wave * 16 * LDA_L;
  const int wp0 = p0 + wave * 16;
  const int64_t grow0 = (int64_t)b * p.N + wp0;
  Stager stg;
  int par = 0;
  stage_load<32>(stg, p.w_1, 256, 0);
  const float* bp = reinterpret_cast<const float*>(p.before.ptr) + df_img_base(p.before, b);
  const float* ap = reinterpret_cast<const float*>(p.after.ptr) + df_img_base(p.after, b);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int f = lane + 64 * j;
    const int pt = f >> 5, c4 = f & 31;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (wp0 + pt < cnt) {
      const int32_t* cc = p.coords + (grow0 + pt) * 3;
      const int64_t cell = (int64_t)cc[1] * p.before.w + cc[2];
      v = (c4 < 16) ? ld4(bp + cell * p.before.ld + c4 * 4) : ld4(ap + cell * p.after.ld + (c4 - 16) * 4);
    }
    st4(Aw + pt * LDA_L + c4 * 4, v);
  }
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int o = lane + 64 * half;
    const float w0 = p.w_off[o * 3 + 0], w1 = p.w_off[o * 3 + 1], w2 = p.w_off[o * 3 + 2], bo = p.b_off[o];
    for (int pt = 0; pt < 16; ++pt) {
      float x = 0.f;
      if (wp0 + pt < cnt) {
        const float* of = p.offs + (grow0 + pt) * 3;
        x = fmaf(w2, of[2], fmaf(w1, of[1], fmaf(w0, of[0], bo)));
      }
      Aw[pt * LDA_L + 128 + o] = x;
    }
  }
  stage_store<32>(stg, Bs);
  __syncthreads();
  f32x4 hid[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float bia = p.b_1[16 * t + li];
    hid[t] = f32x4{bia, bia, bia, bia};
  }
  gemm_stream<32, 32, BSZ_L>(p.w_1, 256, 8, nullptr, 0, Aw + li * LDA_L + lq * 4, Bs, par, hid, stg);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) Aw[(4 * lq + r) * LDA_L + 16 * t + li] = df_gelu(hid[t][r]);
  __syncthreads();
  if (lane < 48) {
    const int pt = lane / 3, o = lane - pt * 3;
    if (wp0 + pt < cnt) {
      float a = p.b_2[o];
      for (int c = 0; c < 32; ++c) a = fmaf(p.w_2[o * 32 + c], Aw[pt * LDA_L + c], a);
      p.flow[(grow0 + pt) * 3 + o] = a;
    }
  }
}

}  // namespace

// w [rows][ld] fp32 -> out [rows][hi (ld) | lo (ld)] bf16, hi = bf16(w), lo = bf16(w - hi): the pre-split weight rows of the
// decoder kernels' mfma_bf16 = 3 form (gemm_dma.h, WStreamT<3>); one pass per optimizer step and weight matrix
__global__ __launch_bounds__(256) void split_bf16x2_rows_kernel(const float* __restrict__ w, __bf16* __restrict__ out, int64_t n, int ld) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / ld;
    const int c = (int)(i - r * ld);
    const float v = w[i];
    const __bf16 hi = (__bf16)v;
    out[r * 2 * ld + c] = hi;
    out[r * 2 * ld + ld + c] = (__bf16)(v - (float)hi);
  }
}

extern "C" int df_split_bf16x2_rows(const float* w, void* out, int64_t rows, int ld, void* stream) {
  DF_REQUIRE(w && out && rows > 0 && ld > 0 && (ld % 32) == 0 && df_aligned16(out), DF_E_ARG);
  const int64_t n = rows * ld;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(split_bf16x2_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), w,
                     reinterpret_cast<__bf16*>(out), n, ld);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

extern "C" int df_linear_decoder_fwd(df_img before, df_img after, const int32_t* coords, const float* offs,
                                     const int32_t* counts, int B, int N, const float* w_off, const float* b_off,
                                     const float* w_1, const float* b_1, const float* w_2, const float* b_2, float* flow,
                                     void* stream) {
  DF_REQUIRE(df_img64_ok(before, B) && df_img64_ok(after, B), DF_E_SHAPE);
  DF_REQUIRE(before.h == after.h && before.w == after.w, DF_E_SHAPE);
  DF_REQUIRE(coords && offs && counts && flow && w_off && b_off && w_1 && b_1 && w_2 && b_2 && df_aligned16(w_1), DF_E_ARG);
  LinFwdParams p;
  p.before = before; p.after = after; p.coords = coords; p.offs = offs; p.counts = counts; p.N = N;
  p.w_off = w_off; p.b_off = b_off; p.w_1 = w_1; p.b_1 = b_1; p.w_2 = w_2; p.b_2 = b_2; p.flow = flow;
  const size_t lds_bytes = (size_t)(2 * BSZ_L + 4 * 16 * LDA_L) * sizeof(float);
  DF_SET_LDS_ONCE((linear_fwd_kernel), (int)lds_bytes);
  hipLaunchKernelGGL(linear_fwd_kernel, dim3((N + 63) / 64, B), dim3(256), lds_bytes,
                     reinterpret_cast<hipStream_t>(stream), p);
  DF_CHECK_LAUNCH();
  return DF_OK;
}
