// docx_order.hip -- the host half of DocXLayout's post-processor on the device: docx_page_result (pdf_table_amd/docxlayout_stage.py) step for step, over
// the records pt_docx_decode leaves in device memory.  Entry point pt_op_docx_order, added under the current ABI number; no engine, one launch, no
// scratch, no host synchronisation.  The host code is the specification; tests/docx_order_ref.py restates the sort replay in Python.
//
// Shape built: ONE WORKGROUP PER PAGE (4 waves), about 29 KB of static LDS (budget: 32 KB, five workgroups a CU by LDS).
//   1. row t of the 2 K rows of both branches: kept?  vertices through the float64 map ((a x + b y) + c, stored as float32), class (the sub branch
//      shifted by n_main), float32 score > thresh.
//   2. rows per class, one zero placeholder per empty class; above top_k rows the cut score is the (rows - top_k)-th smallest, found by COUNTING (a row's
//      score is the cut when fewer-or-equal rows lie strictly below it than the rank and more lie at or below it); ties at the cut stay.
//   3. the survivors are compacted by counting into "items" in (class, list order): layouts (class < n_main) first, then the sub-fields; vertices
//      through rintf.
//   4. the sub-fields are sorted (below); every layout x sorted field pair gets its quad_intersection_rate in float64 -- a wave per layout, a lane per
//      field, the clipped polygon (<= 8 vertices) in registers -- and the first field of the largest rate wins if that rate is > 0.1.
//   5. the loose layouts and every field's layouts are sorted, a list per wave at a time; then the blocks (sorted fields + sorted loose singles); the
//      layouts are written block by block.
// The sort is CPython's list.sort for fewer than 64 elements with a comparator that is NOT a total order, so the device makes the interpreter's
// comparisons in the interpreter's order: per list the main angle (a median by rank counting), every block's turned rectangle once, then the n x n bits of
// `<` in parallel (one uint64 row mask per block), and ONE lane replays count_run + binarysort reading bits.  Every loop is bounded by n < 64.
// A page the kernel does not serve gets flag 1 and no rows: a list of 64 or more blocks, a non-positive threshold (placeholders would pass it), a
// vertex that is not finite, a clipped polygon above 8 vertices, or a comparison in which the host divides by zero (it raises there).
// Barriers are reached by all threads: every branch around one is workgroup-uniform.
//
// Arithmetic (-ffp-contract=off): float64 in the host's operation order, IEEE division and square root; atan2 / sin / cos are the device library's
// (exact for an axis-aligned page: angle 0, sin 0, cos 1).  fp32 / fp64 / int32 arrays only: compiled ONCE (build.py: ONCE_HIP_SOURCES).
#include <math.h>

#include "common.h"

using PT_FMT_NS::a16_kernel_enter;

namespace {

constexpr int kDoThreads = 256;                    // 4 waves; one thread per row of both branches
constexpr int kDoWaves = kDoThreads / 64;
constexpr int kDoMaxK = PT_DOCX_MAX_K;
constexpr int kDoRows = 2 * kDoMaxK;
constexpr int kDoMaxCls = 16;
constexpr int kDoSort = 64;                        // a list must be SHORTER than this

static_assert(kDoRows <= kDoThreads, "one thread per row");
static_assert(kDoRows <= 256, "item ids are bytes");

struct DoArgs {
  const int32_t* counts;
  const float* recs;
  const uint8_t* keep;
  int K;
  double m[6];
  float thresh;
  int top_k, ncls, n_main, use_nms;
  int32_t* nout;
  int32_t* flag;
  float* rows;
};

// ---- _relation / _compare_rects ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int do_relation(double lo_a, double len_a, double lo_b, double len_b) {
  const double hi_a = lo_a + len_a, hi_b = lo_b + len_b;
  const int start = lo_a < lo_b ? 1 : (lo_a > lo_b ? -1 : 0);
  const int end = hi_a > hi_b ? 1 : (hi_a < hi_b ? -1 : 0);
  if (hi_a < lo_b + 1e-4 && hi_a < hi_b - 1e-4) return 1;
  if (lo_a > hi_b - 1e-4 && lo_a > lo_b + 1e-4) return 2;
  if (start == 1 && end == -1) return 3;
  if (start == -1 && end == 1) return 4;
  if (start >= 0 && end >= 0) return 5;
  if (start <= 0 && end <= 0) return 6;
  return 0;
}

// rectangles (min x, min y, width, height); *bad: the host would divide by zero here
__device__ __forceinline__ int do_compare(const double* ra, const double* rb, bool* bad) {
  const double lx_a = ra[0], ly_a = ra[1], hx_a = ra[0] + ra[2], hy_a = ra[1] + ra[3];
  const double lx_b = rb[0], ly_b = rb[1], hx_b = rb[0] + rb[2], hy_b = rb[1] + rb[3];
  const int xt = do_relation(ra[0], ra[2], rb[0], rb[2]), yt = do_relation(ra[1], ra[3], rb[1], rb[3]);
  if (yt == 1) return -1;
  if (yt == 2) return 1;
  const double ha = hy_a - ly_a, hb = hy_b - ly_b;
  if (yt == 3 || yt == 4) {
    const double low = hb < ha ? hb : ha;
    if (low == 0.0) { *bad = true; return 0; }
    if (yt == 3) {
      const double near = (hy_a - ly_b) / low;
      return (xt == 2 || xt == 4) ? (near < 0.5 ? -1 : 1) : -1;
    }
    const double near = (hy_b - ly_a) / low;
    return (xt == 1 || xt == 3) ? (near < 0.5 ? 1 : -1) : 1;
  }
  if (xt == 1 || xt == 3) return -1;
  if (xt == 2 || xt == 4) return 1;
  const double diff = fabs(0.5 * (ly_a + hy_a) - 0.5 * (ly_b + hy_b));
  const double tall = hb > ha ? hb : ha;
  const bool same_row = tall == 0.0 ? diff == 0.0 : diff / tall < 0.1;
  const double ka = same_row ? lx_a + hx_a : ly_a + hy_a, kb = same_row ? lx_b + hx_b : ly_b + hy_b;
  return ka < kb ? -1 : (ka > kb ? 1 : 0);
}

// ---- list.sort for n < 64 (Objects/listobject.c: count_run, then one binarysort), on the bits of `<`: mask[x] bit y = (block x < block y) ---------------
__device__ void do_replay(const unsigned long long* mask, uint8_t* a, int n) {
  for (int i = 0; i < n; ++i) a[i] = (uint8_t)i;
  if (n < 2) return;
  int run = 2;
  if ((mask[a[1]] >> a[0]) & 1ull) {               // strictly descending prefix, reversed in place
    while (run < n && ((mask[a[run]] >> a[run - 1]) & 1ull)) ++run;
    for (int lo = 0, hi = run - 1; lo < hi; ++lo, --hi) {
      const uint8_t t = a[lo];
      a[lo] = a[hi];
      a[hi] = t;
    }
  } else {
    while (run < n && !((mask[a[run]] >> a[run - 1]) & 1ull)) ++run;
  }
  for (int start = run; start < n; ++start) {
    int l = 0, r = start;
    const uint8_t pivot = a[start];
    const unsigned long long pm = mask[pivot];
    do {
      const int p = l + ((r - l) >> 1);
      if ((pm >> a[p]) & 1ull) r = p; else l = p + 1;
    } while (l < r);
    for (int p = start; p > l; --p) a[p] = a[p - 1];
    a[l] = pivot;
  }
}

// sort_blocks for the calling WAVE's list ids[0 .. n) of item indices (n < kDoSort; 0: the wave only keeps the barriers company) -> out[0 .. n), which may
// be ids.  Called by every thread of the workgroup the same number of times.  rect / mask / perm: the wave's own scratch
__device__ void do_sort(const uint8_t* ids, int n, uint8_t* out, const float (*pts)[8], double (*rect)[4], unsigned long long* mask, uint8_t* perm,
                        int* s_bad) {
  const int lane = threadIdx.x & 63;
  const bool on = lane < n;
  double p[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) p[k] = on ? (double)pts[ids[lane]][k] : 0.0;
  // _main_angle: the median direction of the first edge, of the wide blocks if there are any
  const double ex = p[2] - p[0], ey = p[3] - p[1], fx = p[4] - p[2], fy = p[5] - p[3];
  const bool wide = on && __dsqrt_rn(ex * ex + ey * ey) > __dsqrt_rn(fx * fx + fy * fy) * 3.0;
  const double ang = atan2(ey, ex);
  const unsigned long long wmask = __ballot(wide);
  const unsigned long long pick = wmask ? wmask : __ballot(on);
  const int m = __popcll(pick);
  int below = 0, upto = 0;
  for (int i = 0; i < n; ++i) {                    // n is wave-uniform
    const double other = __shfl(ang, i);
    if ((pick >> i) & 1ull) {
      below += other < ang ? 1 : 0;
      upto += other <= ang ? 1 : 0;
    }
  }
  const unsigned long long is_med = __ballot(((pick >> lane) & 1ull) && below <= m / 2 && m / 2 < upto);
  double med = 0.0;
  if (is_med) med = __shfl(ang, __ffsll((long long)is_med) - 1);
  const double sn = sin(med), cs = cos(med);
  double xlo = 0.0, xhi = 0.0, ylo = 0.0, yhi = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double x = p[2 * k] * cs + p[2 * k + 1] * sn, y = p[2 * k + 1] * cs - p[2 * k] * sn;
    xlo = (k == 0 || x < xlo) ? x : xlo;
    xhi = (k == 0 || x > xhi) ? x : xhi;
    ylo = (k == 0 || y < ylo) ? y : ylo;
    yhi = (k == 0 || y > yhi) ? y : yhi;
  }
  const double mine[4] = {xlo, ylo, xhi - xlo, yhi - ylo};
  if (on) {
#pragma unroll
    for (int k = 0; k < 4; ++k) rect[lane][k] = mine[k];
  }
  __syncthreads();
  bool bad = false;
  for (int i = 0; i < n; ++i) {
    const double ri[4] = {rect[i][0], rect[i][1], rect[i][2], rect[i][3]};
    const bool lt = on && lane != i && do_compare(ri, mine, &bad) == -1;
    const unsigned long long row = __ballot(lt);
    if (lane == 0) mask[i] = row;
  }
  if (bad) *s_bad = 1;
  __syncthreads();
  if (lane == 0) do_replay(mask, perm, n);
  __syncthreads();
  const uint8_t v = on ? ids[perm[lane]] : (uint8_t)0;
  __syncthreads();
  if (on) out[lane] = v;
  __syncthreads();
}

// ---- quad_intersection_rate -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool do_is_convex(const double* x, const double* y) {
  int sign = 0;
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = (i + 1) & 3, k = (i + 2) & 3;
    const double cr = (x[j] - x[i]) * (y[k] - y[j]) - (y[j] - y[i]) * (x[k] - x[j]);
    if (cr != 0.0) {
      if (sign != 0 && (cr > 0.0) != (sign > 0)) ok = false;
      if (ok) sign = cr > 0.0 ? 1 : -1;            // the host has returned at the first disagreement
    }
  }
  return ok;
}

__device__ __forceinline__ void do_bbox(double* x, double* y) {
  double xl = x[0], xh = x[0], yl = y[0], yh = y[0];
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    xl = x[k] < xl ? x[k] : xl;
    xh = x[k] > xh ? x[k] : xh;
    yl = y[k] < yl ? y[k] : yl;
    yh = y[k] > yh ? y[k] : yh;
  }
  x[0] = xl; y[0] = yl; x[1] = xh; y[1] = yl; x[2] = xh; y[2] = yh; x[3] = xl; y[3] = yh;
}

__device__ __forceinline__ double do_shoelace4(const double* x, const double* y) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) s += x[i] * y[(i + 1) & 3] - x[(i + 1) & 3] * y[i];
  return 0.5 * s;
}

__device__ __forceinline__ void do_reverse4(double* x, double* y) {
  double t;
  t = x[0]; x[0] = x[3]; x[3] = t; t = x[1]; x[1] = x[2]; x[2] = t;
  t = y[0]; y[0] = y[3]; y[3] = t; t = y[1]; y[1] = y[2]; y[2] = t;
}

// area(src & tgt) / area(src); src / tgt: 8 coordinates each.  *bad: the clipped polygon would not fit 8 vertices
__device__ double do_rate(const double* src, const double* tgt, bool* bad) {
  double ax[4], ay[4], bx[4], by[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { ax[k] = src[2 * k]; ay[k] = src[2 * k + 1]; bx[k] = tgt[2 * k]; by[k] = tgt[2 * k + 1]; }
  if (!(do_is_convex(ax, ay) && do_is_convex(bx, by))) {
    do_bbox(ax, ay);
    do_bbox(bx, by);
  }
  const double area_a = do_shoelace4(ax, ay), area_b = do_shoelace4(bx, by);
  if (area_a == 0.0 || area_b == 0.0) return 0.0;
  if (area_a < 0.0) do_reverse4(ax, ay);
  if (area_b < 0.0) do_reverse4(bx, by);
  // Sutherland-Hodgman: the subject (a) cut by every edge of the clip polygon (b); the polygon lives in registers (every index is a constant)
  double ox[8], oy[8];
  int len = 4;
#pragma unroll
  for (int k = 0; k < 8; ++k) { ox[k] = k < 4 ? ax[k] : 0.0; oy[k] = k < 4 ? ay[k] : 0.0; }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double cx = bx[i], cy = by[i];
    const double ex = bx[(i + 1) & 3] - cx, ey = by[(i + 1) & 3] - cy;
    double ix[8], iy[8], side[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      ix[k] = ox[k];
      iy[k] = oy[k];
      side[k] = ex * (iy[k] - cy) - ey * (ix[k] - cx);
    }
    const int ilen = len;
    len = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (k < ilen) {
        const bool wrap = k + 1 >= ilen;
        const double qx = wrap ? ix[0] : ix[(k + 1) & 7], qy = wrap ? iy[0] : iy[(k + 1) & 7], sq = wrap ? side[0] : side[(k + 1) & 7];
        const double sp = side[k];
        if (sp >= 0.0) {
          if (len >= 8) *bad = true;
#pragma unroll
          for (int s = 0; s < 8; ++s)
            if (s == len) { ox[s] = ix[k]; oy[s] = iy[k]; }
          ++len;
        }
        if ((sp > 0.0 && sq < 0.0) || (sp < 0.0 && sq > 0.0)) {
          const double t = sp / (sp - sq);
          const double nx = ix[k] + t * (qx - ix[k]), ny = iy[k] + t * (qy - iy[k]);
          if (len >= 8) *bad = true;
#pragma unroll
          for (int s = 0; s < 8; ++s)
            if (s == len) { ox[s] = nx; oy[s] = ny; }
          ++len;
        }
      }
    }
    if (len > 8) len = 8;                          // (flagged above; never past the registers)
  }
  if (len < 3) return 0.0;
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (k < len) {
      const bool wrap = k + 1 >= len;
      const double qx = wrap ? ox[0] : ox[(k + 1) & 7], qy = wrap ? oy[0] : oy[(k + 1) & 7];
      s += ox[k] * qy - qx * oy[k];
    }
  }
  return fabs(0.5 * s) / fabs(area_a);
}

// ---- the page ---------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDoThreads) void docx_order_kernel(DoArgs a) {
  a16_kernel_enter();
  __shared__ float s_sc[kDoThreads];                // a row's score (rows of no class: s_cl < 0)
  __shared__ int s_cl[kDoThreads];
  __shared__ int s_ccnt[kDoMaxCls];
  __shared__ float s_pts[kDoRows][8];               // items: rounded vertices
  __shared__ float s_iscore[kDoRows];
  __shared__ int s_icls[kDoRows];
  __shared__ double s_rect[kDoWaves][kDoSort][4];
  __shared__ unsigned long long s_mask[kDoWaves][kDoSort];
  __shared__ uint8_t s_perm[kDoWaves][kDoSort];
  __shared__ uint8_t s_fields[kDoSort];             // field items in sorted order
  __shared__ uint8_t s_seg[kDoMaxK];                // layout items, grouped: segment k < NF = field k's, segment NF = the loose ones
  __shared__ int s_where[kDoMaxK];
  __shared__ int s_size[kDoSort + 1], s_off[kDoSort + 1];
  __shared__ uint8_t s_blk[kDoSort];                // blocks: an item each (a field, or a loose layout)
  __shared__ int s_boff[kDoSort];
  __shared__ uint8_t s_order[kDoMaxK];              // layout items in the final order
  __shared__ float s_cut;
  __shared__ int s_bad;

  const int page = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, ncls = a.ncls, n_main = a.n_main;
  const float (*pts)[8] = s_pts;

  if (tid == 0) { s_bad = a.thresh > 0.f ? 0 : 1; s_cut = 0.f; }
  if (tid < kDoMaxCls) s_ccnt[tid] = 0;

  // 1. the thread's row
  const int b = tid >= K ? 1 : 0, r = tid - b * K;
  float q[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float score = 0.f;
  int cl = -1;
  if (tid < 2 * K) {
    int cnt = a.counts[page * 2 + b];
    cnt = cnt < 0 ? 0 : (cnt > K ? K : cnt);
    const size_t row = ((size_t)page * 2 + b) * K + r;
    if (r < cnt && (!a.use_nms || a.keep[row] != 0)) {
      const float* rec = a.recs + row * PT_DOCX_REC_FLOATS;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double x = (double)rec[2 * k], y = (double)rec[2 * k + 1];
        q[2 * k] = (float)((a.m[0] * x + a.m[1] * y) + a.m[2]);
        q[2 * k + 1] = (float)((a.m[3] * x + a.m[4] * y) + a.m[5]);
      }
      score = rec[8];
      const float cf = b ? rec[9] + (float)n_main : rec[9];
      if (cf >= 0.f && cf < (float)ncls && cf == (float)(int)cf && ((int)cf >= n_main) == (b == 1) && score > a.thresh) cl = (int)cf;
    }
  }
  s_sc[tid] = score;
  s_cl[tid] = cl;
  __syncthreads();

  // 2. rows per class and the cut
  if (tid < ncls) {
    int c = 0;
    for (int i = 0; i < kDoThreads; ++i) c += s_cl[i] == tid ? 1 : 0;
    s_ccnt[tid] = c;
  }
  __syncthreads();
  int total = 0, holes = 0;
  for (int c = 0; c < ncls; ++c) {
    total += s_ccnt[c] > 0 ? s_ccnt[c] : 1;
    holes += s_ccnt[c] > 0 ? 0 : 1;
  }
  const bool cutting = total > a.top_k;              // workgroup-uniform
  if (cutting) {
    const int kth = total - a.top_k;
    // the thread's own score as the candidate; thread 0 also tries the placeholders' zero
    const bool zero_too = tid == 0 && holes > 0;
    int below = 0, upto = 0, below0 = 0, upto0 = holes;
    for (int i = 0; i < kDoThreads; ++i) {
      if (s_cl[i] < 0) continue;
      const float v = s_sc[i];
      below += v < score ? 1 : 0;
      upto += v <= score ? 1 : 0;
      below0 += v < 0.f ? 1 : 0;
      upto0 += v <= 0.f ? 1 : 0;
    }
    below += 0.f < score ? holes : 0;
    upto += 0.f <= score ? holes : 0;
    if (cl >= 0 && below <= kth && kth < upto) s_cut = score;      // equal scores write the same value
    if (zero_too && below0 <= kth && kth < upto0) s_cut = 0.f;
  }
  __syncthreads();
  if (cutting && cl >= 0 && !(score >= s_cut)) cl = -1;
  s_cl[tid] = cl;                                    // (every read of the loop above lies before the barrier)
  __syncthreads();

  // 3. items in (class, list order): rows of one branch are in list order, and every class belongs to one branch
  int pos = 0, NL = 0, NF = 0;
  for (int i = 0; i < kDoThreads; ++i) {
    const int ci = s_cl[i];
    if (ci < 0) continue;
    NL += ci < n_main ? 1 : 0;
    NF += ci < n_main ? 0 : 1;
    pos += (ci < cl || (ci == cl && i < tid)) ? 1 : 0;
  }
  if (cl >= 0) {
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float v = rintf(q[k]);
      finite = finite && isfinite(v);
      s_pts[pos][k] = v;
    }
    s_iscore[pos] = score;
    s_icls[pos] = cl;
    if (!finite) s_bad = 1;
  }
  if (tid == 0 && NF >= kDoSort) s_bad = 1;
  __syncthreads();
  if (s_bad) {                                       // workgroup-uniform
    if (tid == 0) { a.flag[page] = 1; a.nout[page] = 0; }
    return;
  }

  // 4. the fields in reading order, then every layout's field
  if (tid < NF) s_fields[tid] = (uint8_t)(NL + tid);
  __syncthreads();
  do_sort(s_fields, wave == 0 ? NF : 0, s_fields, pts, s_rect[wave], s_mask[wave], s_perm[wave], &s_bad);
  {
    double tgt[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) tgt[k] = lane < NF ? (double)s_pts[s_fields[lane]][k] : 0.0;
    bool bad = false;
    for (int i = wave; i < NL; i += kDoWaves) {      // wave-uniform
      double src[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) src[k] = (double)s_pts[i][k];
      double rate = lane < NF ? do_rate(src, tgt, &bad) : 0.0;
      int who = lane;
      if (!(rate > 0.0)) { rate = 0.0; who = kDoSort; }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {      // the largest rate; of equal rates the first field
        const double r2 = __shfl_xor(rate, off);
        const int w2 = __shfl_xor(who, off);
        if (r2 > rate || (r2 == rate && w2 < who)) { rate = r2; who = w2; }
      }
      if (lane == 0) s_where[i] = (who < kDoSort && rate > 0.1) ? who : NF;
    }
    if (bad) s_bad = 1;
  }
  __syncthreads();

  // 5. the segments
  if (tid <= NF) {
    int c = 0;
    for (int i = 0; i < NL; ++i) c += s_where[i] == tid ? 1 : 0;
    s_size[tid] = c;
  }
  __syncthreads();
  if (tid <= NF) {
    int o = 0;
    for (int g = 0; g < tid; ++g) o += s_size[g];
    s_off[tid] = o;
    if (s_size[tid] >= kDoSort || (tid == NF && NF + s_size[NF] >= kDoSort)) s_bad = 1;
  }
  __syncthreads();
  if (s_bad) {
    if (tid == 0) { a.flag[page] = 1; a.nout[page] = 0; }
    return;
  }
  if (tid < NL) {
    const int g = s_where[tid];
    int within = 0;
    for (int i = 0; i < tid; ++i) within += s_where[i] == g ? 1 : 0;
    s_seg[s_off[g] + within] = (uint8_t)tid;
  }
  __syncthreads();
  for (int base = 0; base <= NF; base += kDoWaves) {   // uniform trip count; a wave per list
    const int g = base + wave;
    const int n = g <= NF ? s_size[g] : 0;
    uint8_t* lst = s_seg + (g <= NF ? s_off[g] : 0);
    do_sort(lst, n, lst, pts, s_rect[wave], s_mask[wave], s_perm[wave], &s_bad);
  }

  // the blocks: sorted fields, then the sorted loose layouts as blocks of their own
  const int nloose = s_size[NF], nblk = NF + nloose;
  if (tid < nblk) s_blk[tid] = tid < NF ? s_fields[tid] : s_seg[s_off[NF] + tid - NF];
  __syncthreads();
  do_sort(s_blk, wave == 0 ? nblk : 0, s_blk, pts, s_rect[wave], s_mask[wave], s_perm[wave], &s_bad);
  // where a block's layouts start: a field item (>= NL) brings its segment, a loose item itself
  if (tid < nblk) {
    int o = 0;
    for (int j = 0; j < tid; ++j) {
      const int it = s_blk[j];
      int sz = 1;
      if (it >= NL) {
        int k = 0;
        for (; k < NF && s_fields[k] != it; ++k) {}
        sz = k < NF ? s_size[k] : 0;
      }
      o += sz;
    }
    s_boff[tid] = o;
  }
  __syncthreads();
  if (tid < nblk) {
    const int it = s_blk[tid];
    if (it >= NL) {
      int k = 0;
      for (; k < NF && s_fields[k] != it; ++k) {}
      if (k < NF)
        for (int e = 0; e < s_size[k]; ++e) s_order[s_boff[tid] + e] = s_seg[s_off[k] + e];
    } else {
      s_order[s_boff[tid]] = (uint8_t)it;
    }
  }
  __syncthreads();
  if (s_bad) {
    if (tid == 0) { a.flag[page] = 1; a.nout[page] = 0; }
    return;
  }
  if (tid < NL) {
    const int it = s_order[tid];
    float* o = a.rows + ((size_t)page * 2 * K + tid) * 6;
    o[0] = s_pts[it][0]; o[1] = s_pts[it][1]; o[2] = s_pts[it][4]; o[3] = s_pts[it][5];
    o[4] = s_iscore[it];
    o[5] = (float)s_icls[it];
  }
  if (tid == 0) { a.flag[page] = 0; a.nout[page] = NL; }
}

}  // namespace

namespace PT_FMT_NS {
namespace api {

int pt_op_docx_order(const int32_t* d_counts, const float* d_recs, const uint8_t* d_keep, int B, int K, double a00, double a01, double a02, double a10,
                     double a11, double a12, float scores_thresh, int top_k, int num_classes, int n_main, int use_nms, int32_t* d_nout, int32_t* d_flag,
                     float* d_rows, pt_stream stream) {
  PT_REQUIRE(B >= 1 && B <= 65535, "pt_op_docx_order: B = %d outside 1 .. 65535", B);
  PT_REQUIRE(d_counts && d_recs && d_keep && d_nout && d_flag && d_rows, "pt_op_docx_order: null pointer");
  PT_REQUIRE(K >= 1 && K <= kDoMaxK, "pt_op_docx_order: K = %d outside 1 .. %d", K, kDoMaxK);
  PT_REQUIRE(num_classes >= 1 && num_classes <= kDoMaxCls, "pt_op_docx_order: num_classes = %d outside 1 .. %d", num_classes, kDoMaxCls);
  PT_REQUIRE(n_main >= 0 && n_main < num_classes, "pt_op_docx_order: n_main = %d outside 0 .. num_classes - 1 = %d", n_main, num_classes - 1);
  PT_REQUIRE(top_k >= 1, "pt_op_docx_order: top_k = %d is not positive", top_k);
  DoArgs a;
  a.counts = d_counts; a.recs = d_recs; a.keep = d_keep; a.K = K;
  a.m[0] = a00; a.m[1] = a01; a.m[2] = a02; a.m[3] = a10; a.m[4] = a11; a.m[5] = a12;
  a.thresh = scores_thresh; a.top_k = top_k; a.ncls = num_classes; a.n_main = n_main; a.use_nms = use_nms ? 1 : 0;
  a.nout = d_nout; a.flag = d_flag; a.rows = d_rows;
  hipLaunchKernelGGL(docx_order_kernel, dim3(B), dim3(kDoThreads), 0, (hipStream_t)stream, a);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

}  // namespace api
}  // namespace PT_FMT_NS
