// lore_match.hip -- text lines -> table cells for the Lore structure model: OcrTableToHtmlTask's find_top1_mach_box (ocr_table_to_html_task.py:48-77;
// pdf_table_amd/table_text_match.py: find_top1_match) over the decode's quads and the processor's logical axes while both are still on the device, so
// that a call's tables cost one launch behind pt_tsr_process and four bytes per line on the copy the stage makes anyway, instead of [lines, cells]
// float64 matrices in numpy per table on the thread that also queues the next batches.  One new entry point under ABI 20, no existing signature
// changed.  tests/test_lore_match_host.py states the same rule in numpy (a key reduction over the cells in input order); the tests compare as integers.
//
// Shape built: ONE WORKGROUP PER TABLE (4 waves).  Pass 1 stages every valid row r < n of the table in LDS once: the bottom-left and top-right vertex
// through the table's inverse affine map as float32 (16 bytes) and the four logical axes rounded like process_logic_output, kept as float32 in the
// order the host sorts by (top, left, bottom, right; 16 bytes).  Pass 2: the waves take the table's lines in turn, the lanes stride the rows and keep
// their smallest key, a __shfl_xor butterfly reduces the full key.  32 bytes per row: PT_TSR_MAX_CELLS = 3000 rows are 96,000 bytes of the CU's 160 KB,
// above the 64 KB a kernel gets unasked (the first call on a device raises the kernel's limit).  int16 axes would make it 24 bytes (72 KB, two
// workgroups per CU instead of one) but would round differently from the host for an axis outside int16; with one workgroup per table and at most a
// few hundred tables per call the second workgroup per CU buys nothing.  Whole waves leave loops together (every bound is wave-uniform), there are no
// atomics and no cross-workgroup state, every loop is bounded by the clamped cell count or the line count.
//
// Arithmetic (-ffp-contract=off keeps every product and sum unfused; tsr_stage.py: transform_quads, collect, process_logic_output):
//   vertex   = fl32((t00 * px + t01 * py) + t02) with px, py float32 widened to double (y: t10, t11, t12), then + the crop offset in double
//   cell box = (x1, y1, x2, y2) = (vertex 3, vertex 1) = bottom-left, top-right: usually y1 > y2
//   axis     = floor(a) + 1 if a - floor(a) > 0.5 else floor(a), float32
//   inside   = t0 >= x1 - 2 && t2 <= x2 + 2 && min(y1, y2) - 2 <= min(t1, t3) && max(t1, t3) <= max(y1, y2) + 2
//   distance = (d1 + d2) + min(d1, d2), d1 = |x1 - t0| + |y1 - t1|, d2 = |x2 - t2| + |y2 - t3|
//   k1       = 1 - inter / (((a_t + a_c) - inter) + 1e-6), inter = max(min(t2, x2) - max(t0, x1), 0) * max(min(t3, y2) - max(t1, y1), 0)
// The host walks the cells in sorted(key = (top, left, bottom, right)) order, a stable sort: "the first containing cell, else the first minimum of
// (k1, distance)" is the smallest (containing first, k1, distance, top, left, bottom, right, input row) -- no sort on the device.
// fp32 / fp64 / int32 arrays only: compiled ONCE (build.py: ONCE_HIP_SOURCES), as namespace pt_bf16.
#include <math.h>

#include <atomic>
#include <mutex>

#include "common.h"

using PT_FMT_NS::a16_kernel_enter;

namespace {

constexpr int kLoreMatchThreads = 256;                 // 4 waves
constexpr int kLoreMatchMaxCells = PT_TSR_MAX_CELLS;   // 32 bytes of LDS per row
constexpr size_t kLoreMatchLds = (size_t)kLoreMatchMaxCells * 32;

struct LoreKey {
  double k1, dist;          // a containing cell: (-inf, 0)
  float top, left, bottom, right;
  int row;
};

__device__ __forceinline__ bool lore_key_less(const LoreKey& a, const LoreKey& b) {
  if (a.k1 != b.k1) return a.k1 < b.k1;
  if (a.dist != b.dist) return a.dist < b.dist;
  if (a.top != b.top) return a.top < b.top;
  if (a.left != b.left) return a.left < b.left;
  if (a.bottom != b.bottom) return a.bottom < b.bottom;
  if (a.right != b.right) return a.right < b.right;
  return a.row < b.row;
}

__device__ __forceinline__ float lore_round_axis(float a) {
  const float fl = floorf(a);
  return (a - fl > 0.5f) ? fl + 1.0f : fl;
}

__global__ __launch_bounds__(kLoreMatchThreads) void lore_match_kernel(const float* __restrict__ dets, const float* __restrict__ axes,
                                                                       const int32_t* __restrict__ counts, const double* __restrict__ affine,
                                                                       const double* __restrict__ offset, const float* __restrict__ lines,
                                                                       const int32_t* __restrict__ offsets, int M, int32_t* __restrict__ out) {
  a16_kernel_enter();
  extern __shared__ float4 lds_vert[];                                  // [n] (x1, y1, x2, y2) before the crop offset
  float4* lds_axis = lds_vert + kLoreMatchMaxCells;                     // [n] (top, left, bottom, right), rounded
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int n = counts[b];
  n = n < 0 ? 0 : (n > kLoreMatchMaxCells ? kLoreMatchMaxCells : n);
  const double t00 = affine[6 * b], t01 = affine[6 * b + 1], t02 = affine[6 * b + 2];
  const double t10 = affine[6 * b + 3], t11 = affine[6 * b + 4], t12 = affine[6 * b + 5];
  const double ox = offset[2 * b], oy = offset[2 * b + 1];
  for (int r = tid; r < n; r += kLoreMatchThreads) {
    const float* p = dets + ((size_t)b * kLoreMatchMaxCells + r) * 9;
    const double blx = p[6], bly = p[7], trx = p[2], try_ = p[3];
    const float x1 = (float)((t00 * blx + t01 * bly) + t02), y1 = (float)((t10 * blx + t11 * bly) + t12);
    const float x2 = (float)((t00 * trx + t01 * try_) + t02), y2 = (float)((t10 * trx + t11 * try_) + t12);
    lds_vert[r] = make_float4(x1, y1, x2, y2);
    const float* a = axes + ((size_t)b * kLoreMatchMaxCells + r) * 4;      // [left, right, top, bottom]
    lds_axis[r] = make_float4(lore_round_axis(a[2]), lore_round_axis(a[0]), lore_round_axis(a[3]), lore_round_axis(a[1]));
  }
  __syncthreads();

  int m0 = offsets[b], m1 = offsets[b + 1];
  m0 = m0 < 0 ? 0 : m0;                                                  // whatever the offsets hold, no line outside [0, M) is touched
  m1 = m1 > M ? M : m1;
  for (int m = m0 + wave; m < m1; m += kLoreMatchThreads / 64) {         // wave-uniform: all 64 lanes reach the shuffles below
    if (n == 0) {
      if (lane == 0) out[m] = -1;
      continue;
    }
    const float4 lf = reinterpret_cast<const float4*>(lines)[m];
    const double t0 = lf.x, t1 = lf.y, t2 = lf.z, t3 = lf.w;
    const double ty_lo = fmin(t1, t3), ty_hi = fmax(t1, t3);
    const double a_t = fabs((t2 - t0) * (t3 - t1));
    LoreKey best;
    best.k1 = INFINITY;
    best.dist = INFINITY;
    best.top = best.left = best.bottom = best.right = INFINITY;
    best.row = 0x7fffffff;
    for (int r = lane; r < n; r += 64) {
      const float4 v = lds_vert[r];
      const float4 ax = lds_axis[r];
      const double c0 = (double)v.x + ox, c1 = (double)v.y + oy, c2 = (double)v.z + ox, c3 = (double)v.w + oy;
      LoreKey k;
      k.top = ax.x;
      k.left = ax.y;
      k.bottom = ax.z;
      k.right = ax.w;
      k.row = r;
      const double cy_lo = fmin(c1, c3), cy_hi = fmax(c1, c3);
      if (t0 >= c0 - 2.0 && t2 <= c2 + 2.0 && cy_lo - 2.0 <= ty_lo && ty_hi <= cy_hi + 2.0) {
        k.k1 = -INFINITY;
        k.dist = 0.0;
      } else {
        const double d1 = fabs(c0 - t0) + fabs(c1 - t1), d2 = fabs(c2 - t2) + fabs(c3 - t3);
        k.dist = (d1 + d2) + fmin(d1, d2);
        const double ix = fmax(fmin(t2, c2) - fmax(t0, c0), 0.0), iy = fmax(fmin(t3, c3) - fmax(t1, c1), 0.0);
        const double inter = ix * iy;
        const double a_c = fabs((c2 - c0) * (c3 - c1));
        k.k1 = 1.0 - inter / (((a_t + a_c) - inter) + 1e-6);
      }
      if (lore_key_less(k, best)) best = k;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      LoreKey other;
      other.k1 = __shfl_xor(best.k1, o);
      other.dist = __shfl_xor(best.dist, o);
      other.top = __shfl_xor(best.top, o);
      other.left = __shfl_xor(best.left, o);
      other.bottom = __shfl_xor(best.bottom, o);
      other.right = __shfl_xor(best.right, o);
      other.row = __shfl_xor(best.row, o);
      if (lore_key_less(other, best)) best = other;
    }
    if (lane == 0) out[m] = best.row == 0x7fffffff ? -1 : best.row;
  }
}

// 96,000 bytes of dynamic LDS are above the 64 KB a kernel may ask for by default: raised once per device, outside any capture
int lore_match_allow_lds(hipStream_t s) {
  static std::atomic<uint64_t> done{0};
  int dev = 0;
  PT_HIP_CHECK(hipGetDevice(&dev));
  PT_REQUIRE(dev >= 0 && dev < 64, "pt_op_lore_match: device %d out of range", dev);
  if ((done.load(std::memory_order_acquire) >> dev) & 1ull) return PT_OK;
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  if ((done.load(std::memory_order_acquire) >> dev) & 1ull) return PT_OK;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  PT_HIP_CHECK(hipStreamIsCapturing(s, &st));
  if (st != hipStreamCaptureStatusNone) {
    pt_set_error("pt_op_lore_match: the first call on device %d sets the kernel's LDS limit and cannot be captured: call it once outside the capture", dev);
    return PT_ERR_STATE;
  }
  PT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&lore_match_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLoreMatchLds));
  done.fetch_or(1ull << dev, std::memory_order_release);
  return PT_OK;
}

}  // namespace

namespace PT_FMT_NS {
namespace api {

int pt_op_lore_match(const float* d_dets, const float* d_axes, const int32_t* d_counts, int B, const double* d_affine, const double* d_offset,
                     const float* d_lines, const int32_t* d_offsets, int M, int32_t* d_out, pt_stream stream) {
  PT_REQUIRE(d_dets && d_axes && d_counts && d_affine && d_offset && d_offsets, "pt_op_lore_match: null pointer");
  PT_REQUIRE(B >= 1 && B <= 65535 && M >= 0, "pt_op_lore_match: bad arguments (B %d: 1 .. 65535, M %d >= 0)", B, M);
  if (M == 0) return PT_OK;
  PT_REQUIRE(d_lines && d_out, "pt_op_lore_match: null pointer (%d lines)", M);
  PT_REQUIRE((reinterpret_cast<uintptr_t>(d_lines) & 15) == 0, "pt_op_lore_match: line boxes must be 16-byte aligned");
  PT_REQUIRE((reinterpret_cast<uintptr_t>(d_affine) & 7) == 0 && (reinterpret_cast<uintptr_t>(d_offset) & 7) == 0,
             "pt_op_lore_match: the float64 arrays must be 8-byte aligned");
  const int rc = lore_match_allow_lds((hipStream_t)stream);
  if (rc != PT_OK) return rc;
  hipLaunchKernelGGL(lore_match_kernel, dim3(B), dim3(kLoreMatchThreads), kLoreMatchLds, (hipStream_t)stream, d_dets, d_axes, d_counts, d_affine, d_offset,
                     d_lines, d_offsets, M, d_out);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

}  // namespace api
}  // namespace PT_FMT_NS
