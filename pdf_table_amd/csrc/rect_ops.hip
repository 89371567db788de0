// rect_ops.hip -- the operators a text-line recogniser needs beyond the square ones (pdf_table_amd/onnx_exec.py; ABI 18): PaddleOCR's recognisers
// shrink the image HEIGHT and keep the width, so their graphs hold convolutions whose stride differs per axis ((2,1), (1,2)), 1x3 / 3x1 kernels
// on token rows, and pools over kh x kw windows on maps of three rows.
//   conv_rect_kernel   dense NHWC implicit GEMM on the matrix pipe: kh, kw in {1, 3} and sh, sw in {1, 2} independently, pad k / 2 per axis.
//                      Only the outputs that are kept are computed (a (2,1) layer is not a stride-1 pass with rows dropped) and only the taps that
//                      exist are multiplied (a 1x3 layer is not a zero-filled 3x3).
//   pool_rect_kernel   max / average over kh x kw windows, stride = window, no padding, floor semantics.
// pt_op_dwconv_rect is the depthwise launcher of layout_kernels.hip with its per-axis stride word.
#include "common.h"

#include <atomic>
#include <mutex>

namespace PT_FMT_NS {

namespace {

typedef a16_bf16x8 bf16x8;
typedef a16_f32x16 f32x16;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

struct RectConv {
  const bf16_t* in;     // [B, H, W, in_cs]: in_cs = Cin, or 2 Cin = [hi | lo] when split
  const bf16_t* w;      // tiles [N/64][KC][kh kw][64][32], KC = Cin/32 (x3 when split: w_hi for x_hi, w_hi for x_lo, w_lo for x_hi)
  const float* bias;    // [N]
  bf16_t* out;          // pixel stride out_cs, first channel out_coff, lo half out_lo_off further
  int B, H, W, Cin, in_cs, nC, N, kh, kw, sh, sw, Ho, Wo, out_cs, out_coff, out_lo_off, act, split;
};

// 16-byte slot q (0..3) of a 64-byte LDS record (32 channels of one pixel / one output channel's 32 weights) at index i: records i and i + 4 share
// their banks, so the slot is rotated by (i >> 2) & 3 -- 16 consecutive records read at one slot then cover the 256-byte bank row
__device__ __forceinline__ int rec_off(int i, int q) { return i * 64 + ((q ^ ((i >> 2) & 3)) << 4); }

// One workgroup = 4 waves = 4 output rows (b, oy) x 32 output columns x 64 output channels; a wave owns one row.  D = [channel][pixel]: the
// weights are the A operand, the pixels the B operand, so a lane ends with 4 consecutive channels of one pixel per register quad (8-byte stores).
// Per 32-channel K chunk: the kh kw weight tiles of the chunk go to LDS once for the four waves, every wave stages ITS patch -- the kh input
// rows its output row reads, 31 sw + kw pixels wide, zeros where the row or column lies outside the image (a row is addressed through
// (b, iy), never through a neighbouring image) -- and the B fragments are read from the patch at pixel stride sw.  The global loads of chunk
// kc + 1 are issued into registers before the MFMAs of chunk kc and written to LDS after them.
// The kernel size is a template parameter (1x1, 1x3, 3x1, 3x3): the tap loops unroll and the staging registers are counted at compile time.
// One 32-pixel tile per wave: a 3 x 3 workgroup at column stride 1 then needs 62 KB of LDS and two workgroups share a CU, which hides the staging
// latency.  Two tiles per wave halve the weight-fragment reads per MFMA but need 87 KB, one workgroup per CU, and measured slower on every shape
// (the A/B is recorded in profiles/r09/onnx_rect.txt); PX stays a constant so that the tile loops read as what they are.
template <int KH, int KW>
__global__ __launch_bounds__(256) void conv_rect_kernel(const RectConv p) {
  a16_kernel_enter();
  extern __shared__ __attribute__((aligned(16))) char rc_lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  constexpr int taps = KH * KW, PX = 1;
  const int PW = (32 * PX - 1) * p.sw + KW;
  char* wl = rc_lds;                                                       // [taps][64 channels] records
  char* pl = rc_lds + taps * 4096 + wave * (KH * PW * 64);               // [kh][PW pixels] records, one patch per wave
  const long long R = (long long)blockIdx.x * 4 + wave;                     // output row over the batch: b Ho + oy
  const bool valid = R < (long long)p.B * p.Ho;
  const int b = valid ? (int)(R / p.Ho) : 0, oy = valid ? (int)(R % p.Ho) : 0;
  const int ox0 = blockIdx.y * 32 * PX, nt = blockIdx.z;
  const int iy0 = oy * p.sh - KH / 2, ix0 = ox0 * p.sw - KW / 2;
  const int KC = p.nC * (p.split ? 3 : 1);
  f32x16 acc[PX][2];
#pragma unroll
  for (int m = 0; m < PX; ++m)
#pragma unroll
    for (int nh = 0; nh < 2; ++nh)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[m][nh][i] = 0.f;

  // Staging plan of this lane, the same for every K chunk: slot i of the patch is 16-byte piece (lane + 64 i) of the wave's kh x PW x 4 pieces.
  // goff: element offset inside image b (-1: padding, a zero is staged), loff: byte offset inside the wave's patch (-1: past the patch)
  constexpr int NT = taps, NP = (KH * (31 * 2 + KW) * 4 + 63) / 64;     // sized for column stride 2
  int goff[NP], loff[NP];
  {
    const int total = KH * PW * 4;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int j = lane + 64 * i, q = j & 3, pp = j >> 2, dy = pp / PW, px = pp - dy * PW;
      const int iy = iy0 + dy, ix = ix0 + px;
      loff[i] = (valid && j < total) ? dy * PW * 64 + rec_off(px, q) : -1;
      goff[i] = ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) ? (iy * p.W + ix) * p.in_cs + q * 8 : -1;
    }
  }
  const bf16_t* img = p.in + (size_t)b * p.H * p.W * p.in_cs;
  const bf16_t* wbase = p.w + (size_t)nt * KC * taps * 2048 + tid * 8;
  const int wlds = rec_off(tid >> 2, tid & 3);
  u32x4 wv[NT], pv[NP];
#pragma unroll
  for (int t = 0; t < NT; ++t) wv[t] = u32x4{0u, 0u, 0u, 0u};
  // kc = -1 is the prologue: nothing to multiply yet, only the first chunk's loads
  for (int kc = -1; kc < KC; ++kc) {
    if (kc >= 0) {
      __syncthreads();                                                     // the previous chunk's fragments have been read
#pragma unroll
      for (int t = 0; t < NT; ++t)
        *reinterpret_cast<u32x4*>(wl + t * 4096 + wlds) = wv[t];
#pragma unroll
      for (int i = 0; i < NP; ++i)
        if (loff[i] >= 0) *reinterpret_cast<u32x4*>(pl + loff[i]) = pv[i];
      __syncthreads();
    }
    if (kc + 1 < KC) {
      // global -> registers for chunk kc + 1: issued a whole chunk ahead, so the loads fly while the matrix pipe works on chunk kc
      const int kn = kc + 1, sec = kn / p.nC, c = kn - sec * p.nC;
      const int coff = c * 32 + (sec == 1 ? p.Cin : 0);                    // section 1 multiplies w_hi with the lo half of x
      const bf16_t* wsrc = wbase + (size_t)kn * taps * 2048;
#pragma unroll
      for (int t = 0; t < NT; ++t)
        wv[t] = *reinterpret_cast<const u32x4*>(wsrc + t * 2048);
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        pv[i] = u32x4{0u, 0u, 0u, 0u};
        if (loff[i] >= 0 && goff[i] >= 0) pv[i] = *reinterpret_cast<const u32x4*>(img + goff[i] + coff);
      }
    }
    if (kc < 0) continue;
    if (valid) {
#pragma unroll
      for (int dy = 0; dy < KH; ++dy)
#pragma unroll
        for (int dx = 0; dx < KW; ++dx) {
          const char* wt = wl + (dy * KW + dx) * 4096;
          const char* pr = pl + dy * PW * 64;
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            const int q = 2 * s + h;
            const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(wt + rec_off(r, q));
            const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(wt + rec_off(32 + r, q));
#pragma unroll
            for (int m = 0; m < PX; ++m) {
              const bf16x8 x = *reinterpret_cast<const bf16x8*>(pr + rec_off((m * 32 + r) * p.sw + dx, q));
              acc[m][0] = mfma_32x32x16_a16(a0, x, acc[m][0]);
              acc[m][1] = mfma_32x32x16_a16(a1, x, acc[m][1]);
            }
          }
        }
    }
  }
  if (!valid) return;
#pragma unroll
  for (int m = 0; m < PX; ++m) {
    const int ox = ox0 + m * 32 + r;
    if (ox >= p.Wo) continue;
    bf16_t* op = p.out + ((size_t)R * p.Wo + ox) * p.out_cs + p.out_coff;
#pragma unroll
    for (int nh = 0; nh < 2; ++nh)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int ch = nt * 64 + nh * 32 + 8 * g + 4 * h;                  // D row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
        const float4 bv = *reinterpret_cast<const float4*>(p.bias + ch);
        float v[4] = {acc[m][nh][4 * g] + bv.x, acc[m][nh][4 * g + 1] + bv.y, acc[m][nh][4 * g + 2] + bv.z, acc[m][nh][4 * g + 3] + bv.w};
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

// kh x kw windows, stride = window, no padding, Ho = H / kh and Wo = W / kw rounded down (trailing rows / columns are dropped).  kind 0: max -- the
// winner's stored bits are copied (both halves in the pair mode, compared on hi + lo; the first of equal values wins, as in maxpool_kxk_kernel);
// kind 1: average -- fp32 sum of hi + lo, times 1 / (kh kw), rounded (split again) once.
__global__ __launch_bounds__(256) void pool_rect_kernel(const bf16_t* __restrict__ in, bf16_t* __restrict__ out, int B, int H, int W, int C, int kind,
                                                        int kh, int kw, int split) {
  a16_kernel_enter();
  const int Ho = H / kh, Wo = W / kw, cg = C >> 3, lo = split ? C : 0, cs = split ? 2 * C : C;
  const long long total = (long long)B * Ho * Wo * cg;
  const float inv = 1.f / (float)(kh * kw);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c8 = (int)(i % cg);
    long long t = i / cg;
    const int ox = (int)(t % Wo);
    t /= Wo;
    const int oy = (int)(t % Ho), b = (int)(t / Ho);
    uint32_t bh[8], bl[8];
    float best[8], sum[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { bh[k] = 0u; bl[k] = 0u; best[k] = 0.f; sum[k] = 0.f; }
    bool first = true;
    for (int dy = 0; dy < kh; ++dy)
      for (int dx = 0; dx < kw; ++dx) {
        const bf16_t* px = in + (((size_t)b * H + oy * kh + dy) * W + ox * kw + dx) * cs + c8 * 8;
        const uint4 vh = *reinterpret_cast<const uint4*>(px);
        uint4 vl = make_uint4(0u, 0u, 0u, 0u);
        if (lo) vl = *reinterpret_cast<const uint4*>(px + lo);
        const uint32_t hw[4] = {vh.x, vh.y, vh.z, vh.w}, lw[4] = {vl.x, vl.y, vl.z, vl.w};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const uint32_t hb = (k & 1) ? (hw[k >> 1] >> 16) : (hw[k >> 1] & 0xFFFFu);
          const uint32_t lb = (k & 1) ? (lw[k >> 1] >> 16) : (lw[k >> 1] & 0xFFFFu);
          const float v = a16_to_f32(hb) + a16_to_f32(lb);
          sum[k] += v;
          if (first || v > best[k]) { best[k] = v; bh[k] = hb; bl[k] = lb; }
        }
        first = false;
      }
    if (kind == 1) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float v = sum[k] * inv;
        bh[k] = f32_to_a16(v);
        bl[k] = f32_to_a16(v - a16_to_f32(bh[k]));
      }
    }
    bf16_t* o = out + (i / cg) * cs + c8 * 8;
    *reinterpret_cast<uint4*>(o) = make_uint4(bh[0] | (bh[1] << 16), bh[2] | (bh[3] << 16), bh[4] | (bh[5] << 16), bh[6] | (bh[7] << 16));
    if (lo) *reinterpret_cast<uint4*>(o + lo) = make_uint4(bl[0] | (bl[1] << 16), bl[2] | (bl[3] << 16), bl[4] | (bl[5] << 16), bl[6] | (bl[7] << 16));
  }
}

// Dynamic LDS beyond the default limit has to be allowed per kernel and device (3 x 3 needs 62 KB at column stride 1, 87 KB at stride 2).  That is a
// host-side setting, not stream work: it is made on the first such launch on a device, and that launch must not be inside a stream capture (refused
// with a message, never set behind a capture's back); afterwards launches are plain and capturable.
template <int KH, int KW>
int allow_large_lds(hipStream_t s) {
  static std::atomic<unsigned long long> done{0ull};          // one bit per device
  int dev = 0;
  PT_HIP_CHECK(hipGetDevice(&dev));
  PT_REQUIRE(dev >= 0 && dev < 64, "pt_op_conv2d_rect: device %d out of range", dev);
  if ((done.load(std::memory_order_acquire) >> dev) & 1ull) return PT_OK;
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  if ((done.load(std::memory_order_acquire) >> dev) & 1ull) return PT_OK;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  PT_HIP_CHECK(hipStreamIsCapturing(s, &st));
  if (st != hipStreamCaptureStatusNone) {
    pt_set_error("pt_op_conv2d_rect: the first %d x %d call on device %d sets the kernel's LDS limit and cannot be captured: call it once outside the capture", KH, KW, dev);
    return PT_ERR_STATE;
  }
  PT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_rect_kernel<KH, KW>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
  done.fetch_or(1ull << dev, std::memory_order_release);
  return PT_OK;
}

template <int KH, int KW>
int launch_conv_rect(const RectConv& p, hipStream_t s) {
  const int PW = 31 * p.sw + KW;
  const size_t lds = (size_t)KH * KW * 4096 + (size_t)4 * KH * PW * 64;
  if (lds > 48 * 1024) {
    const int rc = allow_large_lds<KH, KW>(s);
    if (rc != PT_OK) return rc;
  }
  const long long rows = (long long)p.B * p.Ho;
  const dim3 grid((unsigned)((rows + 3) / 4), (unsigned)((p.Wo + 31) / 32), (unsigned)(p.N / 64));
  hipLaunchKernelGGL((conv_rect_kernel<KH, KW>), grid, dim3(256), lds, s, p);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

}  // namespace

namespace api {

int pt_op_conv2d_rect(pt_engine* e, const uint16_t* d_in, int B, int H, int W, int Cin, const uint16_t* d_w_tiled, const float* d_bias, int N, int kh,
                      int kw, int sh, int sw, uint16_t* d_out, int out_cstride, int out_coff, int act, int split, int out_lo_off, pt_stream stream) {
  PT_REQUIRE(e && d_in && d_w_tiled && d_bias && d_out, "pt_op_conv2d_rect: null pointer");
  PT_REQUIRE((kh == 1 || kh == 3) && (kw == 1 || kw == 3), "pt_op_conv2d_rect: kernel kh=%d kw=%d unsupported (each of kh, kw is 1 or 3)", kh, kw);
  PT_REQUIRE((sh == 1 || sh == 2) && (sw == 1 || sw == 2), "pt_op_conv2d_rect: stride sh=%d sw=%d unsupported (each of sh, sw is 1 or 2)", sh, sw);
  PT_REQUIRE(B > 0 && H > 0 && W > 0 && Cin > 0 && Cin % 32 == 0 && N > 0 && N % 64 == 0,
             "pt_op_conv2d_rect: B=%d H=%d W=%d Cin=%d N=%d unsupported (positive sizes, Cin a multiple of 32, N a multiple of 64)", B, H, W, Cin, N);
  PT_REQUIRE(act >= 0 && act <= 2, "pt_op_conv2d_rect: act=%d unsupported (0 none, 1 ReLU, 2 hardswish)", act);
  PT_REQUIRE(out_cstride % 4 == 0 && out_coff >= 0 && out_coff % 4 == 0 && out_coff + N <= out_cstride &&
                 (!split || (out_lo_off % 4 == 0 && out_lo_off >= N && out_coff + out_lo_off + N <= out_cstride)),
             "pt_op_conv2d_rect: out_cstride=%d out_coff=%d out_lo_off=%d do not hold N=%d channels%s (multiples of 4)", out_cstride, out_coff,
             out_lo_off, N, split ? " twice" : "");
  RectConv p;
  p.in = d_in; p.w = d_w_tiled; p.bias = d_bias; p.out = d_out;
  p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.in_cs = split ? 2 * Cin : Cin; p.nC = Cin / 32; p.N = N;
  p.kh = kh; p.kw = kw; p.sh = sh; p.sw = sw;
  p.Ho = (H + 2 * (kh / 2) - kh) / sh + 1; p.Wo = (W + 2 * (kw / 2) - kw) / sw + 1;
  p.out_cs = out_cstride; p.out_coff = out_coff; p.out_lo_off = out_lo_off; p.act = act; p.split = split ? 1 : 0;
  PT_REQUIRE((long long)B * p.Ho < (1ll << 33) && (p.Wo + 31) / 32 <= 65535 && N / 64 <= 65535, "pt_op_conv2d_rect: grid out of range");
  PT_REQUIRE((long long)H * W * p.in_cs < (1ll << 31), "pt_op_conv2d_rect: H=%d W=%d Cin=%d: an image of more than 2^31 values (the kernel indexes inside an image in 32 bits)",
             H, W, Cin);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (kh == 1) return kw == 1 ? launch_conv_rect<1, 1>(p, s) : launch_conv_rect<1, 3>(p, s);
  return kw == 1 ? launch_conv_rect<3, 1>(p, s) : launch_conv_rect<3, 3>(p, s);
}

int pt_op_dwconv_rect(pt_engine* e, const uint16_t* d_in, int B, int H, int W, int C, const float* d_w_taps, const float* d_bias, int k, int sh, int sw,
                      int act, uint16_t* d_out, int split, pt_stream stream) {
  PT_REQUIRE(e && d_in && d_w_taps && d_bias && d_out, "pt_op_dwconv_rect: null pointer");
  PT_REQUIRE((k == 3 || k == 5) && (sh == 1 || sh == 2) && (sw == 1 || sw == 2) && B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && act >= 0 && act <= 2,
             "pt_op_dwconv_rect: k=%d sh=%d sw=%d B=%d H=%d W=%d C=%d act=%d unsupported (k 3/5, strides 1/2, C a multiple of 8, act 0/1/2)", k, sh, sw, B,
             H, W, C, act);
  return pt_launch_dwconv(d_in, d_w_taps, d_bias, d_out, B, H, W, C, k, (sh << 8) | sw, act, split ? 1 : 0, reinterpret_cast<hipStream_t>(stream), nullptr);
}

int pt_op_pool_rect(pt_engine* e, const uint16_t* d_in, int B, int H, int W, int C, int kind, int kh, int kw, uint16_t* d_out, int split,
                    pt_stream stream) {
  PT_REQUIRE(e != nullptr, "pt_op_pool_rect: null engine");
  PT_REQUIRE(kind == 0 || kind == 1, "pt_op_pool_rect: kind=%d unsupported (0 max, 1 average)", kind);
  PT_REQUIRE(kh >= 1 && kh <= 4 && kw >= 1 && kw <= 4 && kh * kw >= 2, "pt_op_pool_rect: window kh=%d kw=%d unsupported (1 <= kh, kw <= 4, kh kw >= 2)", kh, kw);
  PT_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "pt_op_pool_rect: B=%d H=%d W=%d C=%d unsupported (positive sizes, C a multiple of 8)", B, H, W, C);
  const long long total = (long long)B * (H / kh) * (W / kw) * (C / 8);
  if (total == 0) return PT_OK;        // a window that does not fit the map: floor semantics give an empty result
  PT_REQUIRE(d_in && d_out, "pt_op_pool_rect: null pointer");
  long long g = (total + 255) / 256;
  g = g < 1 ? 1 : (g > 65536 ? 65536 : g);
  hipLaunchKernelGGL(pool_rect_kernel, dim3((unsigned)g), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), d_in, d_out, B, H, W, C, kind, kh, kw, split ? 1 : 0);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

}  // namespace api
}  // namespace PT_FMT_NS
