// det_ops.hip -- what a PP-OCRv4 mobile text detector (PP-LCNetV3 + RSE-FPN + DB head) needs from the generic ONNX executor beyond the operators of
// graph_ops.hip / rect_ops.hip (pdf_table_amd/onnx_exec.py; entry points added under ABI 18):
//   affine_act_kernel   y = s2[c] act(s1[c] x + b1[c]) + b2[c] over an NHWC 16-bit map: PP-LCNetV3's LearnableAffineBlock (scale x + bias with two
//                       learned scalars) where it cannot be folded into a convolution -- behind an activation and in front of a zero-padded
//                       convolution -- with the stand-alone activation in front of it in the same launch.  Memory-bound: 16-byte loads and stores.
//   db_tail_kernel      the DB head's tail in one launch: ConvT 2x2 / 2 (C -> C1) + ReLU, ConvT 2x2 / 2 (C1 -> 1), Sigmoid.  Layer by layer that
//                       writes a [2H, 2W, 64] map, a [4H, 4W, 64] map for ONE real channel and a sigmoid pass over it; here every input pixel is read
//                       once and its 4 x 4 output pixels are written as fp32, the C1-channel intermediate never leaves the registers (and stays fp32).
#include "common.h"

namespace PT_FMT_NS {

namespace {

__device__ __forceinline__ void d_load8(const bf16_t* p, int lo, float* v) {
  const uint4 h = *reinterpret_cast<const uint4*>(p);
  const uint32_t hw[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) { v[2 * k] = a16lo_f32(hw[k]); v[2 * k + 1] = a16hi_f32(hw[k]); }
  if (lo) {
    const uint4 l = *reinterpret_cast<const uint4*>(p + lo);
    const uint32_t lw[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[2 * k] += a16lo_f32(lw[k]); v[2 * k + 1] += a16hi_f32(lw[k]); }
  }
}

__device__ __forceinline__ void d_store8(bf16_t* p, int lo, const float* v) {
  uint32_t h[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) h[k] = f32_to_a16(v[k]);
  *reinterpret_cast<uint4*>(p) = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
  if (lo) {
    uint32_t l[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) l[k] = f32_to_a16(v[k] - a16_to_f32(h[k]));
    *reinterpret_cast<uint4*>(p + lo) = make_uint4(l[0] | (l[1] << 16), l[2] | (l[3] << 16), l[4] | (l[5] << 16), l[6] | (l[7] << 16));
  }
}

// One thread = 8 consecutive channels of one pixel.  The four vectors are fp32 [Cp]; channels c >= C (the padding up to Cp) are written as zeros
// whatever the vectors hold there.  act: 0 none, 1 ReLU, 2 hardswish (the formula of act_kernel).  Pair mode: hi + lo in, fp32 arithmetic, split again.
__global__ __launch_bounds__(256) void affine_act_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ out, long long total8, int Cp, int C,
                                                         const float* __restrict__ s1, const float* __restrict__ b1, const float* __restrict__ s2,
                                                         const float* __restrict__ b2, int act, int split) {
  a16_kernel_enter();
  const int cg = Cp >> 3, lo = split ? Cp : 0, cs = split ? 2 * Cp : Cp;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total8; i += (long long)gridDim.x * blockDim.x) {
    const int c0 = (int)(i % cg) * 8;
    const long long off = (i / cg) * cs + c0;
    float v[8];
    d_load8(x + off, lo, v);
    const float4 s1a = *reinterpret_cast<const float4*>(s1 + c0), s1b = *reinterpret_cast<const float4*>(s1 + c0 + 4);
    const float4 b1a = *reinterpret_cast<const float4*>(b1 + c0), b1b = *reinterpret_cast<const float4*>(b1 + c0 + 4);
    const float4 s2a = *reinterpret_cast<const float4*>(s2 + c0), s2b = *reinterpret_cast<const float4*>(s2 + c0 + 4);
    const float4 b2a = *reinterpret_cast<const float4*>(b2 + c0), b2b = *reinterpret_cast<const float4*>(b2 + c0 + 4);
    const float S1[8] = {s1a.x, s1a.y, s1a.z, s1a.w, s1b.x, s1b.y, s1b.z, s1b.w}, B1[8] = {b1a.x, b1a.y, b1a.z, b1a.w, b1b.x, b1b.y, b1b.z, b1b.w};
    const float S2[8] = {s2a.x, s2a.y, s2a.z, s2a.w, s2b.x, s2b.y, s2b.z, s2b.w}, B2[8] = {b2a.x, b2a.y, b2a.z, b2a.w, b2b.x, b2b.y, b2b.z, b2b.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float t = S1[j] * v[j] + B1[j];
      if (act == 1) t = fmaxf(t, 0.f);
      else if (act == 2) t = t * fminf(fmaxf(t + 3.f, 0.f), 6.f) / 6.f;
      t = S2[j] * t + B2[j];
      v[j] = (c0 + j < C) ? t : 0.f;
    }
    d_store8(out + off, lo, v);
  }
}

struct DbTail {
  const bf16_t* x;      // [npix][cs]: cs = Cp, or 2 Cp = [hi | lo] when split
  const float* w1;      // [C][C1][2][2]
  const float* b1;      // [C1]
  const float* w2;      // [C1][1][2][2]
  const float* b2;      // [1]
  float* out;           // [B][4H][4W]
  long long npix;       // B H W
  int H, W, Cp, C, C1, split;
};

// One thread = one input pixel -> its 4 x 4 output pixels.  CG = groups of 8 input channels held in registers (C <= 8 CG <= Cp; the stored padding
// channels are zeros and their LDS weights are zeros).  LDS: W1 as [q = dy 2 + dx][c1][8 CG] fp32 -- every lane of a wave reads the SAME address
// (q and c1 are loop counters), so the 16-byte reads broadcast and cost no bank conflicts; b1 / W2 / b2 (5 C1 + 1 floats) stay in global memory:
// with them the C = C1 = 64 case would need 66816 bytes, past the 64 KB a launch gets without a per-device attribute call, and their addresses are
// wave-uniform (c1 is a loop counter), so the compiler reads them with scalar loads -- one per wave, not per lane -- from the scalar cache.
// out[b, 4y + 2dy + ey, 4x + 2dx + ex] = sigmoid(b2 + sum_c1 W2[c1, ey, ex] relu(b1[c1] + sum_c W1[c, c1, dy, dx] x[c])), fp32 throughout (fused multiply-adds; the
// inner sum in two chains, even and odd channels).  A thread writes four 16-byte row pieces; neighbouring lanes are neighbouring pixels of a row, so a wave's store is one
// contiguous run per output row.  Workgroups are persistent (grid-stride over 256-pixel tiles): the weights are staged once per workgroup.
template <int CG>
__global__ __launch_bounds__(256) void db_tail_kernel(const DbTail p) {
  a16_kernel_enter();
  extern __shared__ __attribute__((aligned(16))) float w1s[];
  constexpr int CC = CG * 8;
  const int C1 = p.C1;
  for (int i = threadIdx.x; i < 4 * C1 * CC; i += 256) {
    const int c = i % CC, c1 = (i / CC) % C1, q = i / (CC * C1);
    w1s[i] = c < p.C ? p.w1[((size_t)c * C1 + c1) * 4 + q] : 0.f;
  }
  __syncthreads();
  const int lo = p.split ? p.Cp : 0, cs = p.split ? 2 * p.Cp : p.Cp;
  const float bias2 = p.b2[0];
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < p.npix; pix += (long long)gridDim.x * 256) {
    float xv[CC];
#pragma unroll
    for (int g = 0; g < CG; ++g) d_load8(p.x + pix * cs + g * 8, lo, xv + g * 8);
    float o[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) o[k] = bias2;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      for (int c1 = 0; c1 < C1; ++c1) {
        const float4* wr = reinterpret_cast<const float4*>(w1s + (size_t)(q * C1 + c1) * CC);
        // explicit FMAs (the library is built with -ffp-contract=off: a * b + c would be two instructions) in two chains, even and odd channels
        float h0 = p.b1[c1], h1 = 0.f;
#pragma unroll
        for (int c4 = 0; c4 < CC / 4; ++c4) {
          const float4 w = wr[c4];
          h0 = __builtin_fmaf(w.x, xv[4 * c4], h0);
          h1 = __builtin_fmaf(w.y, xv[4 * c4 + 1], h1);
          h0 = __builtin_fmaf(w.z, xv[4 * c4 + 2], h0);
          h1 = __builtin_fmaf(w.w, xv[4 * c4 + 3], h1);
        }
        const float h = fmaxf(h0 + h1, 0.f);
        const float4 w2 = *reinterpret_cast<const float4*>(p.w2 + 4 * c1);
        o[4 * q] = __builtin_fmaf(w2.x, h, o[4 * q]);
        o[4 * q + 1] = __builtin_fmaf(w2.y, h, o[4 * q + 1]);
        o[4 * q + 2] = __builtin_fmaf(w2.z, h, o[4 * q + 2]);
        o[4 * q + 3] = __builtin_fmaf(w2.w, h, o[4 * q + 3]);
      }
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) o[k] = 1.f / (1.f + expf(-o[k]));
    const int xx = (int)(pix % p.W);
    const long long row = pix / p.W;                     // b H + y: the output rows 4 row .. 4 row + 3 (a batch is 4 H output rows)
    float* ob = p.out + (row * 4) * (4ll * p.W) + 4ll * xx;
#pragma unroll
    for (int r = 0; r < 4; ++r) {                        // output row r = 2 dy + ey, columns 2 dx + ex: o[(dy 2 + dx) 4 + ey 2 + ex]
      const int dy = r >> 1, ey = r & 1;
      *reinterpret_cast<float4*>(ob + (long long)r * 4 * p.W) =
          make_float4(o[(dy * 2) * 4 + ey * 2], o[(dy * 2) * 4 + ey * 2 + 1], o[(dy * 2 + 1) * 4 + ey * 2], o[(dy * 2 + 1) * 4 + ey * 2 + 1]);
    }
  }
}

template <int CG>
int launch_db_tail(const DbTail& p, hipStream_t s) {
  const size_t lds = (size_t)4 * p.C1 * CG * 8 * sizeof(float);          // <= 64 KB at C = C1 = 64
  long long g = (p.npix + 255) / 256;
  g = g < 1 ? 1 : (g > 2048 ? 2048 : g);
  hipLaunchKernelGGL((db_tail_kernel<CG>), dim3((unsigned)g), dim3(256), lds, s, p);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

}  // namespace

namespace api {

int pt_op_affine_act(pt_engine* e, const uint16_t* d_in, long long npix, int Cpad, int C, const float* d_s1, const float* d_b1, const float* d_s2,
                     const float* d_b2, int act, uint16_t* d_out, int split, pt_stream stream) {
  PT_REQUIRE(e && d_in && d_out && d_s1 && d_b1 && d_s2 && d_b2, "pt_op_affine_act: null pointer");
  PT_REQUIRE(npix > 0 && Cpad > 0 && Cpad % 8 == 0 && C > 0 && C <= Cpad, "pt_op_affine_act: npix=%lld Cpad=%d C=%d unsupported (Cpad a multiple of 8, 0 < C <= Cpad)",
             npix, Cpad, C);
  PT_REQUIRE(act >= 0 && act <= 2, "pt_op_affine_act: act=%d unsupported (0 none, 1 ReLU, 2 hardswish)", act);
  const long long total8 = npix * (Cpad >> 3);
  long long g = (total8 + 255) / 256;
  g = g < 1 ? 1 : (g > 65536 ? 65536 : g);
  hipLaunchKernelGGL(affine_act_kernel, dim3((unsigned)g), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), d_in, d_out, total8, Cpad, C, d_s1, d_b1,
                     d_s2, d_b2, act, split ? 1 : 0);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

int pt_op_db_tail(pt_engine* e, const uint16_t* d_in, int B, int H, int W, int Cpad, int C, int C1, const float* d_w1, const float* d_b1,
                  const float* d_w2, const float* d_b2, float* d_out, int split, pt_stream stream) {
  PT_REQUIRE(e && d_in && d_w1 && d_b1 && d_w2 && d_b2 && d_out, "pt_op_db_tail: null pointer");
  PT_REQUIRE(B > 0 && H > 0 && W > 0 && Cpad > 0 && Cpad % 8 == 0, "pt_op_db_tail: B=%d H=%d W=%d Cpad=%d unsupported (positive sizes, Cpad a multiple of 8)", B, H,
             W, Cpad);
  PT_REQUIRE(C >= 1 && C <= 64 && C1 >= 1 && C1 <= 64 && C <= Cpad, "pt_op_db_tail: C=%d C1=%d unsupported (1 <= C, C1 <= 64, C <= Cpad=%d)", C, C1, Cpad);
  DbTail p;
  p.x = d_in; p.w1 = d_w1; p.b1 = d_b1; p.w2 = d_w2; p.b2 = d_b2; p.out = d_out;
  p.npix = (long long)B * H * W; p.H = H; p.W = W; p.Cp = Cpad; p.C = C; p.C1 = C1; p.split = split ? 1 : 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // the kernel is built for 1, 2, 3, 4, 6 and 8 groups of 8 input channels and reads that many from every pixel: the smallest that holds C
  const int need = (C + 7) / 8, cg = need <= 4 ? need : (need <= 6 ? 6 : 8);
  PT_REQUIRE(8 * cg <= Cpad, "pt_op_db_tail: C=%d is read as %d channels, the rows hold Cpad=%d", C, 8 * cg, Cpad);
  switch (cg) {
    case 1: return launch_db_tail<1>(p, s);
    case 2: return launch_db_tail<2>(p, s);
    case 3: return launch_db_tail<3>(p, s);
    case 4: return launch_db_tail<4>(p, s);
    case 6: return launch_db_tail<6>(p, s);
    default: return launch_db_tail<8>(p, s);
  }
}

}  // namespace api
}  // namespace PT_FMT_NS
