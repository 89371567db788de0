// large_conv.hip -- dense convolutions with a kernel side of 5, 7 or 9 (pdf_table_amd/onnx_exec.py; added under ABI 19): the neck of the PP-OCRv4
// SERVER detector (LKPAN, "large" mode) reads every pyramid level through 9x9 kernels, and its IntraCL blocks add 7x7 / 7x1 / 1x7 and 5x5 / 5x1 / 1x5.
//   conv_large_kernel   dense NHWC implicit GEMM on the matrix pipe: kh, kw in {1, 3, 5, 7, 9} independently (at least one of them >= 5), stride 1,
//                       no dilation, zero padding k / 2 per axis.  Operand conventions of conv_rect_kernel (csrc/rect_ops.hip): the same weight tiles
//                       [N/64][KC][kh kw][64][32], fp32 bias, none / ReLU / hardswish, a channel slice of a wider output, the three-section pair mode.
// conv_rect_kernel keeps all kh kw weight tiles of a K chunk in LDS (4 KB each): 324 KB at 9x9.  Here the working set is cut per TAP ROW instead.
#include "common.h"

#include <atomic>
#include <mutex>

namespace PT_FMT_NS {

namespace {

typedef a16_bf16x8 bf16x8;
typedef a16_f32x16 f32x16;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

struct LargeConv {
  const bf16_t* in;     // [B, H, W, in_cs]: in_cs = Cin, or 2 Cin = [hi | lo] when split
  const bf16_t* w;      // tiles [N/64][KC][kh kw][64][32], KC = Cin/32 (x3 when split: w_hi for x_hi, w_hi for x_lo, w_lo for x_hi)
  const float* bias;    // [N]
  bf16_t* out;          // pixel stride out_cs, first channel out_coff, lo half out_lo_off further
  int B, H, W, Cin, in_cs, nC, N, kh, kw, out_cs, out_coff, out_lo_off, act, split;
};

// 16-byte slot q (0..3) of a 64-byte LDS record at index i, rotated by (i >> 2) & 3 as in rect_ops.hip: 16 consecutive records read at one slot
// cover the 256-byte bank row
__device__ __forceinline__ int lrec_off(int i, int q) { return i * 64 + ((q ^ ((i >> 2) & 3)) << 4); }

constexpr int LC_RW = 2;                  // output rows per wave
constexpr int LC_ROWS = 4 * LC_RW;        // output rows per workgroup

// One workgroup = 4 waves = LC_ROWS = 8 consecutive output rows of ONE image x 32 output columns x 64 output channels; a wave owns two rows.
// D = [channel][pixel] as in conv_rect_kernel: weights are the A operand, pixels the B operand, 8-byte stores of 4 consecutive channels.
// Reuse chosen: the input rows are staged ONCE per 32-channel K chunk for the whole workgroup -- the kh + 7 rows (b, iy) its eight output rows read,
// 31 + KW pixels wide, zeros where the row or the column lies outside the image (rows are addressed through (b, iy), never through a neighbouring
// image) -- and every tap row dy of every wave reads its B fragments from that one patch: output row o reads patch row o + dy.  A staged row serves up
// to kh tap rows of up to 8 output rows.  The weights go through LDS one GROUP of TR tap rows at a time (TR KW tiles of 4 KB; TR = 1 for KW >= 5,
// 3 for the narrow 9x3 / 7x1 kind so that a step still has work between its barriers), and an A fragment is used for both rows of the wave.
// LDS per workgroup at 9x9: 9 tiles = 36 KB + 16 rows x 40 pixels x 64 B = 40 KB, 76 KB in all: two workgroups share a CU's 160 KB.
// Pipeline, as conv_rect_kernel: the global loads of the next step's weight tiles are issued into registers before the MFMAs of this step and written
// to LDS after them; the next chunk's patch is issued right after this chunk's was written and flies under all of the chunk's tap rows.
// KW is a template parameter (the tap loop unrolls, the staging registers are counted at compile time); kh is a run-time loop bound.
template <int KW, int TR>
__global__ __launch_bounds__(256, 2) void conv_large_kernel(const LargeConv p) {
  a16_kernel_enter();
  extern __shared__ __attribute__((aligned(16))) char lc_lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  constexpr int NT = TR * KW, PW = 31 + KW;
  constexpr int NP = ((9 + LC_ROWS - 1) * PW * 4 + 255) / 256;              // 16-byte pieces of the patch per thread, sized for kh = 9
  const int kh = p.kh, PR = kh + LC_ROWS - 1, NG = (kh + TR - 1) / TR, taps = kh * KW;
  char* wl = lc_lds;                                                        // [NT][64 channels] records
  char* pl = lc_lds + NT * 4096;                                            // [PR][PW pixels] records
  const int nRB = (p.H + LC_ROWS - 1) / LC_ROWS;
  const int b = blockIdx.x / nRB, oy0 = (blockIdx.x - b * nRB) * LC_ROWS;
  const int ox0 = blockIdx.y * 32, nt = blockIdx.z;
  const int iy0 = oy0 - kh / 2, ix0 = ox0 - KW / 2;
  const int oyw = oy0 + wave * LC_RW;                                       // the wave's first output row
  const bool valid = oyw < p.H;
  const int KC = p.nC * (p.split ? 3 : 1);
  f32x16 acc[LC_RW][2];
#pragma unroll
  for (int m = 0; m < LC_RW; ++m)
#pragma unroll
    for (int nh = 0; nh < 2; ++nh)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[m][nh][i] = 0.f;

  // Staging plan of this thread, the same for every K chunk: piece tid + 256 i of the PR x PW x 4 pieces of the patch.
  // goff: element offset inside image b (-1: padding, a zero is staged), loff: byte offset inside the patch (-1: past the patch)
  int goff[NP], loff[NP];
  {
    const int total = PR * PW * 4;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int j = tid + 256 * i, q = j & 3, pp = j >> 2, pr = pp / PW, px = pp - pr * PW;
      const int iy = iy0 + pr, ix = ix0 + px;
      loff[i] = j < total ? pr * PW * 64 + lrec_off(px, q) : -1;
      goff[i] = ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) ? (iy * p.W + ix) * p.in_cs + q * 8 : -1;
    }
  }
  const bf16_t* img = p.in + (size_t)b * p.H * p.W * p.in_cs;
  const bf16_t* wbase = p.w + (size_t)nt * KC * taps * 2048 + tid * 8;
  const int wlds = lrec_off(tid >> 2, tid & 3);
  u32x4 wv[NT], pv[NP];
#pragma unroll
  for (int t = 0; t < NT; ++t) wv[t] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < NP; ++i) pv[i] = u32x4{0u, 0u, 0u, 0u};

  // global -> registers: the patch of chunk kn
  auto load_patch = [&](int kn) {
    const int sec = kn / p.nC, c = kn - sec * p.nC;
    const int coff = c * 32 + (sec == 1 ? p.Cin : 0);                       // section 1 multiplies w_hi with the lo half of x
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      pv[i] = u32x4{0u, 0u, 0u, 0u};
      if (loff[i] >= 0 && goff[i] >= 0) pv[i] = *reinterpret_cast<const u32x4*>(img + goff[i] + coff);
    }
  };

  // a step = one group of TR tap rows of one K chunk; (kc, g) is the step being multiplied, (kn, gn) the one whose weights are in flight
  const int S = KC * NG;
  int kc = 0, g = 0, kn = 0, gn = 0;
  for (int st = -1; st < S; ++st) {
    if (st >= 0) {
      __syncthreads();                                                     // the previous step's fragments have been read
#pragma unroll
      for (int t = 0; t < NT; ++t)
        *reinterpret_cast<u32x4*>(wl + t * 4096 + wlds) = wv[t];
      if (g == 0) {
#pragma unroll
        for (int i = 0; i < NP; ++i)
          if (loff[i] >= 0) *reinterpret_cast<u32x4*>(pl + loff[i]) = pv[i];
      }
      __syncthreads();
    }
    if (st < 0) load_patch(0);
    else if (g == 0 && kc + 1 < KC) load_patch(kc + 1);
    if (st + 1 < S) {
      // global -> registers for the next step's weight tiles: issued a whole step ahead, so the loads fly while the matrix pipe works on this one
      const bf16_t* wsrc = wbase + ((size_t)kn * taps + (size_t)gn * TR * KW) * 2048;
#pragma unroll
      for (int tr = 0; tr < TR; ++tr)
#pragma unroll
        for (int dx = 0; dx < KW; ++dx) {
          const int t = tr * KW + dx;
          wv[t] = u32x4{0u, 0u, 0u, 0u};
          if (gn * TR + tr < kh) wv[t] = *reinterpret_cast<const u32x4*>(wsrc + t * 2048);
        }
    }
    if (st >= 0 && valid) {
#pragma unroll
      for (int tr = 0; tr < TR; ++tr) {
        const int dy = g * TR + tr;
        if (dy >= kh) break;
        const char* pr0 = pl + (wave * LC_RW + dy) * (PW * 64);
#pragma unroll
        for (int dx = 0; dx < KW; ++dx) {
          const char* wt = wl + (tr * KW + dx) * 4096;
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            const int q = 2 * s + h;
            const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(wt + lrec_off(r, q));
            const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(wt + lrec_off(32 + r, q));
#pragma unroll
            for (int m = 0; m < LC_RW; ++m) {
              const bf16x8 x = *reinterpret_cast<const bf16x8*>(pr0 + m * (PW * 64) + lrec_off(r + dx, q));
              acc[m][0] = mfma_32x32x16_a16(a0, x, acc[m][0]);
              acc[m][1] = mfma_32x32x16_a16(a1, x, acc[m][1]);
            }
          }
        }
      }
    }
    kc = kn; g = gn;
    if (++gn == NG) { gn = 0; ++kn; }
  }
  if (!valid) return;
  const int ox = ox0 + r;
  if (ox >= p.W) return;
#pragma unroll
  for (int m = 0; m < LC_RW; ++m) {
    const int oy = oyw + m;
    if (oy >= p.H) continue;
    bf16_t* op = p.out + (((size_t)b * p.H + oy) * p.W + ox) * p.out_cs + p.out_coff;
#pragma unroll
    for (int nh = 0; nh < 2; ++nh)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const int ch = nt * 64 + nh * 32 + 8 * gq + 4 * h;                 // D row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
        const float4 bv = *reinterpret_cast<const float4*>(p.bias + ch);
        float v[4] = {acc[m][nh][4 * gq] + bv.x, acc[m][nh][4 * gq + 1] + bv.y, acc[m][nh][4 * gq + 2] + bv.z, acc[m][nh][4 * gq + 3] + bv.w};
        uint32_t hb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (p.act == 1) v[j] = fmaxf(v[j], 0.f);
          else if (p.act == 2) v[j] = v[j] * fminf(fmaxf(v[j] + 3.f, 0.f), 6.f) / 6.f;
          hb[j] = f32_to_a16(v[j]);
        }
        *reinterpret_cast<uint2*>(op + ch) = make_uint2(hb[0] | (hb[1] << 16), hb[2] | (hb[3] << 16));
        if (p.split) {
          uint32_t lb[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) lb[j] = f32_to_a16(v[j] - a16_to_f32(hb[j]));
          *reinterpret_cast<uint2*>(op + ch + p.out_lo_off) = make_uint2(lb[0] | (lb[1] << 16), lb[2] | (lb[3] << 16));
        }
      }
  }
}

// Dynamic LDS beyond the default limit has to be allowed per kernel and device (9x9 needs 76 KB).  A host-side setting, not stream work: made on the
// first launch of an instantiation on a device, and that launch must not be inside a stream capture (refused with a message, never set behind a
// capture's back); afterwards launches are plain and capturable.  The rule of pt_op_conv2d_rect.
template <int KW, int TR>
int allow_large_lds(hipStream_t s) {
  static std::atomic<unsigned long long> done{0ull};          // one bit per device
  int dev = 0;
  PT_HIP_CHECK(hipGetDevice(&dev));
  PT_REQUIRE(dev >= 0 && dev < 64, "pt_op_conv2d_large: device %d out of range", dev);
  if ((done.load(std::memory_order_acquire) >> dev) & 1ull) return PT_OK;
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  if ((done.load(std::memory_order_acquire) >> dev) & 1ull) return PT_OK;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  PT_HIP_CHECK(hipStreamIsCapturing(s, &st));
  if (st != hipStreamCaptureStatusNone) {
    pt_set_error("pt_op_conv2d_large: the first call with kw = %d on device %d sets the kernel's LDS limit and cannot be captured: call it once outside the capture", KW, dev);
    return PT_ERR_STATE;
  }
  PT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_large_kernel<KW, TR>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
  done.fetch_or(1ull << dev, std::memory_order_release);
  return PT_OK;
}

template <int KW, int TR>
int launch_conv_large(const LargeConv& p, hipStream_t s) {
  const size_t lds = (size_t)TR * KW * 4096 + (size_t)(p.kh + LC_ROWS - 1) * (31 + KW) * 64;
  PT_REQUIRE(lds <= 80 * 1024, "pt_op_conv2d_large: %d x %d needs %zu bytes of LDS", p.kh, p.kw, lds);
  if (lds > 48 * 1024) {
    const int rc = allow_large_lds<KW, TR>(s);
    if (rc != PT_OK) return rc;
  }
  const long long blocks = (long long)p.B * ((p.H + LC_ROWS - 1) / LC_ROWS);
  PT_REQUIRE(blocks < (1ll << 31) && (p.W + 31) / 32 <= 65535 && p.N / 64 <= 65535, "pt_op_conv2d_large: grid out of range");
  const dim3 grid((unsigned)blocks, (unsigned)((p.W + 31) / 32), (unsigned)(p.N / 64));
  hipLaunchKernelGGL((conv_large_kernel<KW, TR>), grid, dim3(256), lds, s, p);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

}  // namespace

namespace api {

int pt_op_conv2d_large(pt_engine* e, const uint16_t* d_in, int B, int H, int W, int Cin, const uint16_t* d_w_tiled, const float* d_bias, int N, int kh,
                       int kw, uint16_t* d_out, int out_cstride, int out_coff, int act, int split, int out_lo_off, pt_stream stream) {
  PT_REQUIRE(e && d_in && d_w_tiled && d_bias && d_out, "pt_op_conv2d_large: null pointer");
  const bool kh_ok = kh == 1 || kh == 3 || kh == 5 || kh == 7 || kh == 9, kw_ok = kw == 1 || kw == 3 || kw == 5 || kw == 7 || kw == 9;
  PT_REQUIRE(kh_ok && kw_ok && (kh >= 5 || kw >= 5),
             "pt_op_conv2d_large: kernel kh=%d kw=%d unsupported (each of kh, kw is 1, 3, 5, 7 or 9 and at least one of them is 5 or more)", kh, kw);
  PT_REQUIRE(B > 0 && H > 0 && W > 0 && Cin > 0 && Cin % 32 == 0 && N > 0 && N % 64 == 0,
             "pt_op_conv2d_large: B=%d H=%d W=%d Cin=%d N=%d unsupported (positive sizes, Cin a multiple of 32, N a multiple of 64)", B, H, W, Cin, N);
  PT_REQUIRE(act >= 0 && act <= 2, "pt_op_conv2d_large: act=%d unsupported (0 none, 1 ReLU, 2 hardswish)", act);
  PT_REQUIRE(out_cstride % 4 == 0 && out_coff >= 0 && out_coff % 4 == 0 && out_coff + N <= out_cstride &&
                 (!split || (out_lo_off % 4 == 0 && out_lo_off >= N && out_coff + out_lo_off + N <= out_cstride)),
             "pt_op_conv2d_large: out_cstride=%d out_coff=%d out_lo_off=%d do not hold N=%d channels%s (multiples of 4)", out_cstride, out_coff,
             out_lo_off, N, split ? " twice" : "");
  LargeConv p;
  p.in = d_in; p.w = d_w_tiled; p.bias = d_bias; p.out = d_out;
  p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.in_cs = split ? 2 * Cin : Cin; p.nC = Cin / 32; p.N = N;
  p.kh = kh; p.kw = kw;
  p.out_cs = out_cstride; p.out_coff = out_coff; p.out_lo_off = out_lo_off; p.act = act; p.split = split ? 1 : 0;
  PT_REQUIRE((long long)H * W * p.in_cs < (1ll << 31), "pt_op_conv2d_large: H=%d W=%d Cin=%d: an image of more than 2^31 values (the kernel indexes inside an image in 32 bits)",
             H, W, Cin);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  switch (kw) {
    case 9: return launch_conv_large<9, 1>(p, s);
    case 7: return launch_conv_large<7, 1>(p, s);
    case 5: return launch_conv_large<5, 1>(p, s);
    case 3: return launch_conv_large<3, 3>(p, s);
    default: return launch_conv_large<1, 3>(p, s);
  }
}

}  // namespace api
}  // namespace PT_FMT_NS
