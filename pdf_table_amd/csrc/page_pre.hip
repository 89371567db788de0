// page_pre.hip -- image-page straightening before detection (OcrSystemTask.image_pre_process, ocr_system_task.py:441-491):
// the line mask of the small-angle deskew, the cubic warp that undoes it, and cv2.rotate's three quarter turns.
//
// These kernels read and write uint8 RGB pages only, so this translation unit is compiled ONCE (build.py: ONCE_HIP_SOURCES), as namespace
// pt_bf16: the entry points take no engine, so api_dispatch.cpp calls pt_bf16::api's copy whatever the precision.  The cv2 arithmetic restated here (fixed-point gray, GaussianBlur,
// adaptiveThreshold, erode / dilate, warpAffine INTER_CUBIC) is unpinned: tests/page_pre_ref.py states every assumption and is what the
// GPU tests compare against bit for bit.
#include <math.h>

#include <mutex>

#include "common.h"

using PT_FMT_NS::a16_kernel_enter;

namespace {

constexpr int kBlurTaps = 15;       // adaptiveThreshold block size
constexpr int kBlurHalf = 7;
constexpr int kMaskThreads = 256;   // 4 waves of 64 lanes: one ballot = one 64-column word of one row

struct BlurTaps {
  int k[kBlurTaps];                 // ufixedpoint16 taps (8 fractional bits), sum 256
};

// OpenCV getGaussianKernelBitExact (sigma = n * 0.15 + 0.35, fused) + getGaussianKernelFixedPoint_ED (error diffusion over the outer taps,
// the centre tap takes the remainder): tests/page_pre_ref.py gaussian_taps() is the same computation.
BlurTaps gaussian_taps() {
  const int n = kBlurTaps, n2 = n / 2;
  const double sigma = fma((double)n, 0.15, 0.35);
  const double scale2 = -0.125 / (sigma * sigma);
  double v[kBlurTaps];
  double sum = 0;
  for (int i = 0, x = 1 - n; i < n2; ++i, x += 2) {
    v[i] = exp((double)(x * x) * scale2);
    sum += v[i];
  }
  sum *= 2;
  sum += 1;
  const double mul1 = 1.0 / sum;
  BlurTaps t;
  double err = 0;
  int s = 0;
  for (int i = 0; i < n2; ++i) {
    const double adj = v[i] * mul1 * 256.0 + err;
    const int v0 = (int)nearbyint(adj);   // cvRound: half to even
    err = adj - v0;
    t.k[i] = t.k[n - 1 - i] = v0;
    s += v0;
  }
  t.k[n2] = 256 - 2 * s;
  return t;
}

// cv2 initInterTab2D(INTER_CUBIC): 32 x 32 positions x 16 taps of 15-bit weights, each entry adjusted to sum to exactly 32768 on the largest
// (or smallest) of its four central taps.  float32 arithmetic as in interpolateCubic (-ffp-contract=off keeps it unfused).
void cubic_table(int16_t* tab) {
  float t1[32][4];
  for (int i = 0; i < 32; ++i) {
    const float x = i * (1.f / 32), A = -0.75f;
    t1[i][0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
    t1[i][1] = ((A + 2) * x - (A + 3)) * x * x + 1;
    t1[i][2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
    t1[i][3] = 1.f - t1[i][0] - t1[i][1] - t1[i][2];
  }
  for (int i = 0; i < 32; ++i)
    for (int j = 0; j < 32; ++j) {
      int16_t* it = tab + (i * 32 + j) * 16;
      int isum = 0;
      for (int k1 = 0; k1 < 4; ++k1)
        for (int k2 = 0; k2 < 4; ++k2) {
          const float v = t1[i][k1] * t1[j][k2];
          long r = lrintf(v * 32768.f);
          r = r < -32768 ? -32768 : (r > 32767 ? 32767 : r);
          it[k1 * 4 + k2] = (int16_t)r;
          isum += (int)r;
        }
      if (isum != 32768) {
        const int diff = isum - 32768;
        int Mk1 = 2, Mk2 = 2, mk1 = 2, mk2 = 2;
        for (int k1 = 2; k1 < 4; ++k1)
          for (int k2 = 2; k2 < 4; ++k2) {
            if (it[k1 * 4 + k2] < it[mk1 * 4 + mk2]) mk1 = k1, mk2 = k2;
            else if (it[k1 * 4 + k2] > it[Mk1 * 4 + Mk2]) Mk1 = k1, Mk2 = k2;
          }
        if (diff < 0) it[Mk1 * 4 + Mk2] = (int16_t)(it[Mk1 * 4 + Mk2] - diff);
        else it[mk1 * 4 + mk2] = (int16_t)(it[mk1 * 4 + mk2] - diff);
      }
    }
}


__device__ __forceinline__ int gray_inv(const uint8_t* p) {
  // 255 - cv2.cvtColor(BGR2GRAY) on the reference's BGR page = the same weights on our RGB page's (R, G, B)
  return 255 - ((p[0] * 4899 + p[1] * 9617 + p[2] * 1868 + 8192) >> 14);
}

// bits [s, s + 64) of a bit row of nw words; words outside the row read as `fill`
__device__ __forceinline__ uint64_t bits_at(const uint64_t* row, int nw, int s, uint64_t fill) {
  const int q = s >> 6, r = s & 63;     // arithmetic shift: floor for negative s
  const uint64_t lo = (q >= 0 && q < nw) ? row[q] : fill;
  if (r == 0) return lo;
  const uint64_t hi = (q + 1 >= 0 && q + 1 < nw) ? row[q + 1] : fill;
  return (lo >> r) | (hi << (64 - r));
}

// One workgroup = BR rows of one page, full width.  LDS: the column-blurred rows V (uint16: sum k_j g <= 255 * 256) [BR][W], then the
// thresholded bits T and the eroded bits E [BR][nw] 64-bit words.  The row pass of cv2's fixed-point blur is exact (no rounding before
// the column pass), so the 2-D sum may be taken columns first: mean = (sum_i k_i sum_j k_j g + 2^15) >> 16.  Gray is recomputed from the
// page where it is needed (the 14-row halo re-reads what the cache holds).  The opening's 1-row structuring element makes erosion and
// dilation per-row operations on the bit rows: an AND (OR) of L shifted 64-bit windows per output word.
template <int BR>
__global__ __launch_bounds__(kMaskThreads) void page_line_mask_kernel(const uint8_t* __restrict__ pages, int h, int w, BlurTaps taps, int L,
                                                                      unsigned long long* __restrict__ out) {
  a16_kernel_enter();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nw = (w + 63) >> 6;
  uint64_t* T = reinterpret_cast<uint64_t*>(smem);
  uint64_t* E = T + BR * nw;
  uint16_t* V = reinterpret_cast<uint16_t*>(E + BR * nw);
  const int page = blockIdx.y, y0 = blockIdx.x * BR, tid = threadIdx.x;
  const int rows = min(BR, h - y0);
  const uint8_t* pg = pages + (size_t)page * h * w * 3;
  // 1. column pass: one thread per column, the BR + 14 clamped rows (BORDER_REPLICATE) once each
  for (int x = tid; x < w; x += kMaskThreads) {
    int acc[BR];
#pragma unroll
    for (int r = 0; r < BR; ++r) acc[r] = 0;
#pragma unroll
    for (int r = 0; r < BR + 2 * kBlurHalf; ++r) {
      int yy = y0 - kBlurHalf + r;
      yy = yy < 0 ? 0 : (yy >= h ? h - 1 : yy);
      const int g = gray_inv(pg + ((size_t)yy * w + x) * 3);
#pragma unroll
      for (int o = 0; o < BR; ++o) {
        const int j = r - o;
        if (j >= 0 && j < kBlurTaps) acc[o] += taps.k[j] * g;
      }
    }
#pragma unroll
    for (int r = 0; r < BR; ++r) V[r * w + x] = (uint16_t)acc[r];
  }
  __syncthreads();
  // 2. row pass + threshold (gray - mean > 2): lane = column within a 64-column word, ballot = the word.  Columns past the page end read 1
  //    so that erosion sees the constant border of cv2's erode (255) there as well.
  for (int idx = tid; idx < BR * nw * 64; idx += kMaskThreads) {
    const int r = idx / (nw * 64), x = idx - r * (nw * 64);
    bool on = true;
    if (x < w && r < rows) {
      int s = 0;
#pragma unroll
      for (int i = 0; i < kBlurTaps; ++i) {
        int xx = x - kBlurHalf + i;
        xx = xx < 0 ? 0 : (xx >= w ? w - 1 : xx);
        s += taps.k[i] * V[r * w + xx];
      }
      const int mean = (s + (1 << 15)) >> 16;
      on = gray_inv(pg + ((size_t)(y0 + r) * w + x) * 3) - mean > 2;
    }
    const unsigned long long m = __ballot(on);
    if ((threadIdx.x & 63) == 0) T[r * nw + (x >> 6)] = m;
  }
  __syncthreads();
  // 3. erode: dst(x) = min_{0 <= i < L} src(x + i - L/2), outside the row = 255; bits past the page end cleared for the dilation
  const int a = L / 2;
  const uint64_t tail = (w & 63) ? ((1ull << (w & 63)) - 1) : ~0ull;
  for (int idx = tid; idx < BR * nw; idx += kMaskThreads) {
    const int r = idx / nw, q = idx - r * nw;
    uint64_t e = ~0ull;
    for (int i = 0; i < L; ++i) e &= bits_at(T + r * nw, nw, q * 64 + i - a, ~0ull);
    E[idx] = q == nw - 1 ? (e & tail) : e;
  }
  __syncthreads();
  // 4. dilate with the same element, outside the row = 0
  for (int idx = tid; idx < rows * nw; idx += kMaskThreads) {
    const int r = idx / nw, q = idx - r * nw;
    uint64_t d = 0;
    for (int i = 0; i < L; ++i) d |= bits_at(E + r * nw, nw, q * 64 + i - a, 0ull);
    out[((size_t)page * h + y0 + r) * nw + q] = q == nw - 1 ? (d & tail) : d;
  }
}

// cv2.warpAffine(page, M, (w, h), INTER_CUBIC, BORDER_REPLICATE) with minv = the inverse map warpAffine computes in fp64.  Coordinates as in
// tsr_preprocess_kernel (lore_kernels.hip): 10-bit fixed point, 1/32-pixel positions; 16 taps at (sx - 1 .. sx + 2, sy - 1 .. sy + 2)
// clamped to the page, 15-bit weights from tab (the device's copy of cubic_table), (acc + 2^14) >> 15 saturated.  blockIdx.y = output page j, taken from page idx[j].
__global__ __launch_bounds__(256) void page_warp_cubic_kernel(const uint8_t* __restrict__ pages, int n, int h, int w,
                                                              const double* __restrict__ minv, const int* __restrict__ idx,
                                                              const int16_t* __restrict__ tab, uint8_t* __restrict__ out) {
  a16_kernel_enter();
  const int j = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= h * w) return;
  const int src = idx[j];
  if (src < 0 || src >= n) return;
  const int y = i / w, x = i - y * w;
  const double* M = minv + (size_t)j * 6;
  auto sat = [](double v) { return (long long)fmin(fmax(rint(v), -2147483648.0), 2147483647.0); };
  const long long adelta = sat(M[0] * x * 1024.0), bdelta = sat(M[3] * x * 1024.0);
  const long long X0 = sat((M[1] * y + M[2]) * 1024.0) + 16, Y0 = sat((M[4] * y + M[5]) * 1024.0) + 16;
  const long long X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
  long long sx = X >> 5, sy = Y >> 5;
  sx = sx < -32768 ? -32768 : (sx > 32767 ? 32767 : sx);
  sy = sy < -32768 ? -32768 : (sy > 32767 ? 32767 : sy);
  const int16_t* wt = tab + (((int)(Y & 31) << 5) | (int)(X & 31)) * 16;
  const uint8_t* pg = pages + (size_t)src * h * w * 3;
  int xs[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long xx = sx - 1 + k;
    xs[k] = (int)(xx < 0 ? 0 : (xx >= w ? w - 1 : xx)) * 3;
  }
  int acc[3] = {0, 0, 0};
#pragma unroll
  for (int k1 = 0; k1 < 4; ++k1) {
    long long yy = sy - 1 + k1;
    yy = yy < 0 ? 0 : (yy >= h ? h - 1 : yy);
    const uint8_t* row = pg + (size_t)yy * w * 3;
#pragma unroll
    for (int k2 = 0; k2 < 4; ++k2) {
      const int c = wt[k1 * 4 + k2];
      const uint8_t* s = row + xs[k2];
      acc[0] += s[0] * c; acc[1] += s[1] * c; acc[2] += s[2] * c;
    }
  }
  uint8_t* o = out + ((size_t)j * h * w + i) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    int u = (acc[c] + (1 << 14)) >> 15;
    o[c] = (uint8_t)(u < 0 ? 0 : (u > 255 ? 255 : u));
  }
}

// cv2.rotate: code 0 = ROTATE_90_CLOCKWISE, 1 = ROTATE_180, 2 = ROTATE_90_COUNTERCLOCKWISE (cv2's own numbering).  A workgroup moves one
// 32 x 32 pixel tile through LDS: read along input rows, written along output rows.  Output [n, w, h, 3] for 0 and 2, [n, h, w, 3] for 1.
__global__ __launch_bounds__(256) void page_quarter_turn_kernel(const uint8_t* __restrict__ pages, int h, int w, int code,
                                                                uint8_t* __restrict__ out) {
  a16_kernel_enter();
  __shared__ uint8_t tile[32][32 * 3 + 1];
  const int page = blockIdx.z;
  const int oh = code == 1 ? h : w, ow = code == 1 ? w : h;
  const int oy0 = blockIdx.y * 32, ox0 = blockIdx.x * 32;
  const uint8_t* pg = pages + (size_t)page * h * w * 3;
  uint8_t* op = out + (size_t)page * oh * ow * 3;
  // input rectangle of the output tile [oy0, oy0 + 32) x [ox0, ox0 + 32)
  //   code 0: out(y, x) = in(h - 1 - x, y)   code 1: out(y, x) = in(h - 1 - y, w - 1 - x)   code 2: out(y, x) = in(x, w - 1 - y)
  int iy0, ix0;
  if (code == 0) { iy0 = h - ox0 - 32; ix0 = oy0; }
  else if (code == 1) { iy0 = h - oy0 - 32; ix0 = w - ox0 - 32; }
  else { iy0 = ox0; ix0 = w - oy0 - 32; }
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int iy = iy0 + r, ix = ix0 + tx;
    if (iy >= 0 && iy < h && ix >= 0 && ix < w) {
      const uint8_t* s = pg + ((size_t)iy * w + ix) * 3;
      tile[r][tx * 3] = s[0]; tile[r][tx * 3 + 1] = s[1]; tile[r][tx * 3 + 2] = s[2];
    }
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int oy = oy0 + r, ox = ox0 + tx;
    if (oy >= oh || ox >= ow) continue;
    int ty_, tx_;          // tile coordinates of the input pixel
    if (code == 0) { ty_ = 31 - tx; tx_ = r; }
    else if (code == 1) { ty_ = 31 - r; tx_ = 31 - tx; }
    else { ty_ = tx; tx_ = 31 - r; }
    uint8_t* d = op + ((size_t)oy * ow + ox) * 3;
    d[0] = tile[ty_][tx_ * 3]; d[1] = tile[ty_][tx_ * 3 + 1]; d[2] = tile[ty_][tx_ * 3 + 2];
  }
}

// the bicubic table in the memory of the CURRENT device, built and uploaded on the first warp there (one copy per device for the process's
// lifetime; a process may drive engines on several GPUs)
int device_cubic_table(const int16_t** out) {
  static std::mutex mu;
  static std::map<int, int16_t*> tabs;
  int dev = 0;
  PT_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  auto it = tabs.find(dev);
  if (it == tabs.end()) {
    std::vector<int16_t> h(1024 * 16);
    cubic_table(h.data());
    int16_t* d = nullptr;
    PT_HIP_CHECK(hipMalloc(&d, h.size() * sizeof(int16_t)));
    const hipError_t e = hipMemcpy(d, h.data(), h.size() * sizeof(int16_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(d);
      pt_set_error("pt_page_warp_cubic: could not upload the bicubic weight table: %s", hipGetErrorString(e));
      return PT_ERR_HIP;
    }
    it = tabs.emplace(dev, d).first;
  }
  *out = it->second;
  return PT_OK;
}

template <int BR>
size_t mask_lds(int w) {
  const int nw = (w + 63) >> 6;
  return (size_t)BR * nw * 8 * 2 + (size_t)BR * w * 2;
}

template <int BR>
int launch_mask(const uint8_t* d_pages, int n, int h, int w, unsigned long long* d_bits, hipStream_t st) {
  static const BlurTaps taps = gaussian_taps();
  const dim3 grid((h + BR - 1) / BR, n);
  hipLaunchKernelGGL(page_line_mask_kernel<BR>, grid, dim3(kMaskThreads), mask_lds<BR>(w), st, d_pages, h, w, taps, w / 40, d_bits);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

}  // namespace

// host half of the deskew (db_post.cpp, next to the contour tracer)
int page_line_angles_batch(const uint64_t* h_bits, int n, int h, int w, int min_width, int n_threads, double* h_angles, int cap,
                           int32_t* h_counts);

namespace PT_FMT_NS {
namespace api {

int pt_page_line_angles(const uint64_t* h_bits, int n, int h, int w, int min_width, int n_threads, double* h_angles, int cap,
                        int32_t* h_counts) {
  return page_line_angles_batch(h_bits, n, h, w, min_width, n_threads, h_angles, cap, h_counts);
}

int pt_page_line_mask(const uint8_t* d_pages, int n, int h, int w, uint64_t* d_bits, pt_stream stream) {
  PT_REQUIRE(d_pages && d_bits && n > 0 && h > 0 && w >= 40, "pt_page_line_mask: bad arguments (n %d, h %d, w %d; w must be >= 40)", n, h, w);
  PT_REQUIRE((size_t)n * h * w * 3 < ((size_t)1 << 40), "pt_page_line_mask: batch too large");
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* bits = reinterpret_cast<unsigned long long*>(d_bits);
  // the largest band of rows whose LDS fits 64 KiB
  if (mask_lds<16>(w) <= 65536) return launch_mask<16>(d_pages, n, h, w, bits, st);
  if (mask_lds<8>(w) <= 65536) return launch_mask<8>(d_pages, n, h, w, bits, st);
  if (mask_lds<4>(w) <= 65536) return launch_mask<4>(d_pages, n, h, w, bits, st);
  if (mask_lds<2>(w) <= 65536) return launch_mask<2>(d_pages, n, h, w, bits, st);
  pt_set_error("pt_page_line_mask: page width %d exceeds the kernel's limit", w);
  return PT_ERR_INVALID;
}

int pt_page_warp_cubic(const uint8_t* d_pages, int n, int h, int w, const double* d_minv, const int32_t* d_idx, int m, uint8_t* d_out,
                       pt_stream stream) {
  PT_REQUIRE(d_pages && d_minv && d_idx && d_out && n > 0 && h > 0 && w > 0 && m > 0 && m <= 65535 && (long long)h * w < (1ll << 31),
             "pt_page_warp_cubic: bad arguments (n %d, h %d, w %d, m %d)", n, h, w, m);
  const int16_t* tab = nullptr;
  const int rc = device_cubic_table(&tab);
  if (rc != PT_OK) return rc;
  const dim3 grid((unsigned)(((long long)h * w + 255) / 256), m);
  hipLaunchKernelGGL(page_warp_cubic_kernel, grid, dim3(256), 0, (hipStream_t)stream, d_pages, n, h, w, d_minv, d_idx, tab, d_out);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

int pt_page_quarter_turn(const uint8_t* d_pages, int n, int h, int w, int code, uint8_t* d_out, pt_stream stream) {
  PT_REQUIRE(d_pages && d_out && n > 0 && n <= 65535 && h > 0 && w > 0 && (code == PT_ROTATE_90_CLOCKWISE || code == PT_ROTATE_180 ||
             code == PT_ROTATE_90_COUNTERCLOCKWISE), "pt_page_quarter_turn: bad arguments (n %d, h %d, w %d, code %d)", n, h, w, code);
  const int oh = code == PT_ROTATE_180 ? h : w, ow = code == PT_ROTATE_180 ? w : h;
  const dim3 grid((ow + 31) / 32, (oh + 31) / 32, n);
  hipLaunchKernelGGL(page_quarter_turn_kernel, grid, dim3(256), 0, (hipStream_t)stream, d_pages, h, w, code, d_out);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

// Host copies of the two restated tables, for the tests (tests/page_pre_ref.py builds its own and compares).
int pt_page_pre_tables(int32_t* h_blur_taps, int16_t* h_cubic) {
  PT_REQUIRE(h_blur_taps || h_cubic, "pt_page_pre_tables: bad arguments");
  if (h_blur_taps) {
    const BlurTaps t = gaussian_taps();
    for (int i = 0; i < kBlurTaps; ++i) h_blur_taps[i] = t.k[i];
  }
  if (h_cubic) cubic_table(h_cubic);
  return PT_OK;
}

}  // namespace api
}  // namespace PT_FMT_NS
