// table_match.hip -- text lines -> table cells for the structure models that give one box per cell (SLANet): PP-Structure's
// TableMatch(filter_ocr_result=True).match_result (ocr_pdf/table/matcher.py:79-100, _filter_ocr_result :185-195) over the head's outputs as
// pt_op_sla_decode left them on the device, so that a micro-batch of tables costs one launch behind the head and a few bytes per line on the copy
// the stage makes anyway, instead of numpy passes over [lines, cells] per table on the host.  Entry point added under ABI 19 (one new entry point, no
// existing signature changed).  pdf_table_amd/table_structure_match.py states the same arithmetic in numpy; tests compare the two as integers.
//
// Shape built: ONE WORKGROUP PER TABLE (4 waves).  Pass 1 stages every row t of the table in LDS once -- is it a cell row (t < steps[b], id flagged), its
// box (min / max over its 2 or 4 points in page pixels) and the box's float32 area -- and reduces the smallest cell y.  Pass 2: the workgroup's waves take
// the table's lines in turn; the lanes stride the rows in increasing t and replace their candidate only on a strictly smaller key; a __shfl_xor
// butterfly orders by (1 - iou, distance) first and by the smaller t second.  A row costs 24 bytes of LDS (T = 501: 12 KB), and a table's rows are read
// from HBM once however many lines it has; the alternative (a wave per line, no staging) decodes the cell boxes again for every line.  Whole waves leave
// loops together (every bound is wave-uniform), there are no atomics and no cross-workgroup state, and every loop is bounded by T or by the line count.
//
// Arithmetic (what matcher.py computes with float32 cell polygons and text boxes widened to double; -ffp-contract=off keeps every product and sum
// unfused):
//   cell coordinate = fl32(fl32(loc * w) + x0) (h, y0 at odd positions): TableLabelDecode's scaling, then the page-frame shift, bit for bit
//   distance        = ((|cx1 - tx1| + |cy1 - ty1|) + |cx2 - tx2|) + |cy2 - ty2| + min(first pair, second pair), double
//   cell area       = fl32(fl32(cx2 - cx1) * fl32(cy2 - cy1));  text area and the sum of both: double
//   intersection    = Python's max / min return one operand (the text box's on equality): an extent whose two edges both come from the cell is the
//                     float32 difference, an intersection whose two extents are both float32 is the float32 product; everything else double
//   key             = (1 - inter / (sum - inter), distance), 1 where the boxes do not overlap; the smallest (key, t) wins
// These kernels read fp32 / int32 arrays only, so the translation unit is compiled ONCE (build.py: ONCE_HIP_SOURCES), as namespace pt_bf16.
#include <math.h>

#include "common.h"

using PT_FMT_NS::a16_kernel_enter;

namespace {

constexpr int kMatchThreads = 256;      // 4 waves
constexpr int kMatchMaxT = 2048;        // 24 bytes of LDS per row: 48 KB

struct MatchKey {
  double k1, dist;
  int t;
};

__device__ __forceinline__ bool key_less(double k1, double dist, int t, const MatchKey& b) {
  return k1 < b.k1 || (k1 == b.k1 && (dist < b.dist || (dist == b.dist && t < b.t)));
}

__global__ __launch_bounds__(kMatchThreads) void table_match_kernel(const float* __restrict__ loc, const int32_t* __restrict__ ids,
                                                                    const int32_t* __restrict__ steps, int T, int L,
                                                                    const uint8_t* __restrict__ cell_flags, int V, const float* __restrict__ frames,
                                                                    const float* __restrict__ lines, const int32_t* __restrict__ offsets, int M,
                                                                    int32_t* __restrict__ out) {
  a16_kernel_enter();
  extern __shared__ float4 lds_box[];                                  // [T] (x1, y1, x2, y2)
  float* lds_area = reinterpret_cast<float*>(lds_box + T);              // [T]
  int* lds_cell = reinterpret_cast<int*>(lds_area + T);                 // [T] 1 = cell row
  float* lds_red = reinterpret_cast<float*>(lds_cell + T);              // [4] per-wave smallest y, then [4] per-wave "has a cell"
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float fw = frames[4 * b], fh = frames[4 * b + 1], fx = frames[4 * b + 2], fy = frames[4 * b + 3];
  int nst = steps ? steps[b] : T;
  nst = nst < 0 ? 0 : (nst > T ? T : nst);
  const int np = L >> 1;                                               // points per row: 2 or 4
  float ymin = INFINITY;
  int any = 0;
  for (int t = tid; t < T; t += kMatchThreads) {
    int cell = 0;
    if (t < nst) {
      const int id = ids[(size_t)b * T + t];
      cell = id >= 0 && id < V && cell_flags[id] != 0;
    }
    float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
    if (cell) {
      const float* p = loc + ((size_t)b * T + t) * L;
      x1 = x2 = p[0] * fw + fx;
      y1 = y2 = p[1] * fh + fy;
      for (int q = 1; q < np; ++q) {
        const float x = p[2 * q] * fw + fx, y = p[2 * q + 1] * fh + fy;
        x1 = fminf(x1, x);
        x2 = fmaxf(x2, x);
        y1 = fminf(y1, y);
        y2 = fmaxf(y2, y);
      }
      ymin = fminf(ymin, y1);
      any = 1;
    }
    lds_box[t] = make_float4(x1, y1, x2, y2);
    lds_area[t] = (x2 - x1) * (y2 - y1);
    lds_cell[t] = cell;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ymin = fminf(ymin, __shfl_xor(ymin, o));
    any |= __shfl_xor(any, o);
  }
  if (lane == 0) {
    lds_red[wave] = ymin;
    lds_red[4 + wave] = any ? 1.f : 0.f;
  }
  __syncthreads();
  ymin = fminf(fminf(lds_red[0], lds_red[1]), fminf(lds_red[2], lds_red[3]));
  any = (lds_red[4] + lds_red[5] + lds_red[6] + lds_red[7]) > 0.f;

  int m0 = offsets[b], m1 = offsets[b + 1];
  m0 = m0 < 0 ? 0 : m0;                                                 // whatever the offsets hold, no line outside [0, M) is touched
  m1 = m1 > M ? M : m1;
  for (int m = m0 + wave; m < m1; m += kMatchThreads / 64) {           // wave-uniform: all 64 lanes reach the shuffles below
    const float4 lf = reinterpret_cast<const float4*>(lines)[m];
    const double tx1 = lf.x, ty1 = lf.y, tx2 = lf.z, ty2 = lf.w;
    if (!any || fmax(ty1, ty2) < (double)ymin) {                       // no cell row, or _filter_ocr_result drops the line
      if (lane == 0) out[m] = -1;
      continue;
    }
    const double s1 = (tx2 - tx1) * (ty2 - ty1);
    MatchKey best;
    best.k1 = INFINITY;
    best.dist = INFINITY;
    best.t = 0x7fffffff;
    for (int t = lane; t < T; t += 64) {
      if (!lds_cell[t]) continue;
      const float4 c = lds_box[t];
      const double cx1 = c.x, cy1 = c.y, cx2 = c.z, cy2 = c.w;
      const double a0 = fabs(cx1 - tx1), a1 = fabs(cy1 - ty1), a2 = fabs(cx2 - tx2), a3 = fabs(cy2 - ty2);
      const double d2 = a0 + a1, d3 = a2 + a3;
      const double dist = ((d2 + a2) + a3) + fmin(d2, d3);
      const float area = lds_area[t];
      const double total = s1 + (double)area;
      // compute_iou(rec1 = text, rec2 = cell): indices 1 / 3 are "left / right", 0 / 2 "top / bottom" whatever they mean geometrically
      const bool l_c = cy1 > ty1, r_c = cy2 < ty2, t_c = cx1 > tx1, b_c = cx2 < tx2;
      const double left = l_c ? cy1 : ty1, right = r_c ? cy2 : ty2, top = t_c ? cx1 : tx1, bottom = b_c ? cx2 : tx2;
      double k1 = 1.0;
      if (!(left >= right || top >= bottom)) {
        const bool f1 = l_c && r_c, f0 = t_c && b_c;
        const double e1 = f1 ? (double)(c.w - c.y) : right - left;
        const double e0 = f0 ? (double)(c.z - c.x) : bottom - top;
        const double inter = (f1 && f0) ? (double)area : e1 * e0;
        k1 = 1.0 - inter / (total - inter);
      }
      if (key_less(k1, dist, t, best)) {
        best.k1 = k1;
        best.dist = dist;
        best.t = t;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      MatchKey other;
      other.k1 = __shfl_xor(best.k1, o);
      other.dist = __shfl_xor(best.dist, o);
      other.t = __shfl_xor(best.t, o);
      if (key_less(other.k1, other.dist, other.t, best)) best = other;
    }
    if (lane == 0) out[m] = best.t == 0x7fffffff ? -1 : best.t;
  }
}

}  // namespace

namespace PT_FMT_NS {
namespace api {

int pt_op_table_match(const float* d_loc, const int32_t* d_ids, const int32_t* d_steps, int B, int T, int L, const uint8_t* d_cell_flags, int V,
                      const float* d_frames, const float* d_lines, const int32_t* d_offsets, int M, int32_t* d_out, pt_stream stream) {
  PT_REQUIRE(d_loc && d_ids && d_cell_flags && d_frames && d_offsets, "pt_op_table_match: null pointer");
  PT_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && T <= kMatchMaxT && (L == 4 || L == 8) && V >= 1 && M >= 0,
             "pt_op_table_match: bad arguments (B %d: 1 .. 65535, T %d: 1 .. %d, L %d: 4 or 8, V %d >= 1, M %d >= 0)", B, T, kMatchMaxT, L, V, M);
  if (M == 0) return PT_OK;
  PT_REQUIRE(d_lines && d_out, "pt_op_table_match: null pointer (%d lines)", M);
  PT_REQUIRE((reinterpret_cast<uintptr_t>(d_lines) & 15) == 0, "pt_op_table_match: line boxes must be 16-byte aligned");
  const size_t lds = (size_t)T * 24 + 8 * sizeof(float);
  hipLaunchKernelGGL(table_match_kernel, dim3(B), dim3(kMatchThreads), lds, (hipStream_t)stream, d_loc, d_ids, d_steps, T, L, d_cell_flags, V, d_frames,
                     d_lines, d_offsets, M, d_out);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

}  // namespace api
}  // namespace PT_FMT_NS
