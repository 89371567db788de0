// det_poly_score.hip -- box_score_slow (db_pp/processor_ocr_db_pp.py:270-289) on the device: the mean of the probability map over the cv2.fillPoly
// mask of a candidate's own traced contour, inside the contour's bounding rectangle clipped to the map.  Entry points pt_op_det_poly_scores and the host
// call that produces its input, pt_db_contour_candidates_batch (the work is in db_post.cpp), added under the current ABI number; no engine, no
// allocation, no host synchronisation.  fillPoly as oracle/db_post.fill_poly_mask restates it (OpenCV drawing.cpp, shift 0, 8-connected): the Bresenham
// outline of every edge united with the scan-line interior.  tests/db_slow_ref.py states the row formulation below in Python.
//
// The quad kernel (det_kernels.hip: box_score_kernel) tests every pixel against every edge; a contour has any number of vertices (a ruled table is one
// component with thousands), so here a ROW is the unit of work and nothing is sorted:
//   * outline: the pixels of one edge on one row are one x-interval -- a run for an x-major edge, one pixel for a y-major one, both closed forms of
//     the left-to-right iteration with the half rule.  The interval's ends go into the row buffer as +1 / -1; a prefix sum gives the cover count.
//   * interior: drawing.cpp sorts the row's crossings and fills [round(x0), round(x1)], [round(x2), round(x3)], ...  With c[x] the number of
//     crossings whose rounded position is x and B(x) the number whose rounded position is < x (those left of the rectangle included), a pixel is in a
//     span iff c[x] > 0 or B(x) is odd: only the PARITY of the counts and whether one is zero matter.
//   One int32 per pixel holds all of it: bit 0 the parity of c[x] (atomic xor), bit 1 c[x] > 0 (atomic or), bits 2.. the signed interval ends (atomic
//   add of +-4, which never carries into the low bits).  Integer atomics in LDS commute, so the buffer is the same in every run.
// Shape built: grid (candidate, band); a workgroup of 4 waves takes one band of rows of one candidate, each WAVE a row at a time: its lanes stride the
// candidate's edges (two compares reject an edge that misses the row), then the row in chunks of 64 pixels -- a shuffle scan of the cover count, a
// ballot for the parity -- and add the covered pixels in double.  A candidate of up to kPsBandRows rows is one band; a taller one is split evenly
// over up to PT_DET_POLY_BANDS bands.  Every band (also those a candidate does not use: they write zero) leaves (sum, count) in the caller's work
// buffer; a second, tiny kernel adds a candidate's bands in band order and divides.  No floating-point atomics, no hand-over between workgroups inside
// a launch: two calls give the same bits.  Every loop is bounded by a count read from the inputs (vertices: the offsets; rows and pixels: the map),
// every index is clamped (offsets into the point list, the page, the rectangle into the map).
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): 77 VGPRs, 87 SGPRs, no scratch, 6 waves a SIMD by registers; dynamic LDS
// 4 x round_up(W, 64) x 4 bytes (15 KiB for a 960-wide map, 64 KiB at the limit W = PT_DET_POLY_MAX_W).  The finish kernel: 54 VGPRs, no LDS, no scratch.
// fp32 / fp64 / int32 arrays only: compiled ONCE (build.py: ONCE_HIP_SOURCES).
#include "common.h"

using PT_FMT_NS::a16_kernel_enter;

namespace {

constexpr int kPsThreads = 256;                    // 4 waves, a row each at a time
constexpr int kPsWaves = kPsThreads / 64;
constexpr int kPsChunk = 64;                       // pixels a wave scans at once; edges a wave looks at at once
constexpr int kPsBandRows = 8;                     // a candidate of at most this many rows is never split
constexpr int kPsBands = PT_DET_POLY_BANDS;        // bands (workgroups) of the tallest candidate
constexpr int kPsMaxW = PT_DET_POLY_MAX_W;         // what 64 KiB of row buffers hold

static_assert(kPsWaves * kPsMaxW * 4 <= 65536, "the row buffers are dynamic LDS below the 64 KiB a launch gets without an attribute");

struct PsArgs {
  const float* prob;
  int n, H, W, wpad;
  const int32_t* points;
  int n_points;
  const int32_t* offsets;
  const int32_t* pages;
  int nb;
  double* part_sum;                                // [nb][kPsBands]
  int32_t* part_cnt;                               // [nb][kPsBands]
};

// C's truncating division; both operands fit 32 bits for every coordinate below 2^15 in magnitude, where the 64-bit divide is never taken
__device__ __forceinline__ long long ps_div(long long a, long long b) {
  if (a == (int)a && b == (int)b && a != (long long)INT32_MIN) return (long long)((int)a / (int)b);
  return a / b;
}

__device__ __forceinline__ int ps_wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(v, o); v = t < v ? t : v; }
  return v;
}
__device__ __forceinline__ int ps_wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(v, o); v = t > v ? t : v; }
  return v;
}

__global__ __launch_bounds__(kPsThreads) void det_poly_score_kernel(PsArgs a) {
  a16_kernel_enter();
  extern __shared__ __attribute__((aligned(16))) int32_t ps_lds[];
  const int ci = blockIdx.x, band = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (ci >= a.nb) return;
  // the candidate's vertices: offsets clamped into the point list
  int o0 = a.offsets[ci], o1 = a.offsets[ci + 1];
  o0 = o0 < 0 ? 0 : (o0 > a.n_points ? a.n_points : o0);
  o1 = o1 < o0 ? o0 : (o1 > a.n_points ? a.n_points : o1);
  const int K = o1 - o0;
  const int32_t* pts = a.points + 2 * (size_t)o0;
  int page = a.pages[ci];
  page = page < 0 ? 0 : (page >= a.n ? a.n - 1 : page);
  // extent of the vertices; every wave computes it for itself (no barrier in front of the early return below)
  int vx0 = INT32_MAX, vx1 = INT32_MIN, vy0 = INT32_MAX, vy1 = INT32_MIN;
  for (int k = lane; k < K; k += 64) {
    const int x = pts[2 * k], y = pts[2 * k + 1];
    vx0 = x < vx0 ? x : vx0; vx1 = x > vx1 ? x : vx1;
    vy0 = y < vy0 ? y : vy0; vy1 = y > vy1 ? y : vy1;
  }
  vx0 = ps_wave_min(vx0); vx1 = ps_wave_max(vx1); vy0 = ps_wave_min(vy0); vy1 = ps_wave_max(vy1);
  auto clampi = [](int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); };
  const int xmin = clampi(vx0, 0, a.W - 1), xmax = clampi(vx1, 0, a.W - 1);
  const int ymin = clampi(vy0, 0, a.H - 1), ymax = clampi(vy1, 0, a.H - 1);
  const int mw = xmax - xmin + 1, mh = ymax - ymin + 1;
  // bands: as few as give each at least kPsBandRows rows, at most kPsBands; rows split evenly
  int nbands = (mh + kPsBandRows - 1) / kPsBandRows;
  nbands = nbands > kPsBands ? kPsBands : (nbands < 1 ? 1 : nbands);      // < 1: a candidate without a vertex (K == 0, nothing is read below)
  const int rows = (mh + nbands - 1) / nbands;
  double sum = 0.0;
  int cnt = 0;
  if (K > 0 && band < nbands) {
    const int r0 = ymin + band * rows;
    int r1 = r0 + rows;
    r1 = r1 > ymax + 1 ? ymax + 1 : r1;
    int32_t* buf = ps_lds + (size_t)wave * a.wpad;
    const int mwp = (mw + kPsChunk - 1) & ~(kPsChunk - 1);      // <= wpad
    const float* pm = a.prob + (size_t)page * a.H * a.W;
    // rows r0 + wave, + kPsWaves, ...: the trip count is the same for the four waves, so the barriers below are reached by all of them
    const int trips = (rows + kPsWaves - 1) / kPsWaves;
    for (int t = 0; t < trips; ++t) {
      const int y = r0 + t * kPsWaves + wave;
      const bool live = y < r1;
      if (live)
        for (int x = lane; x < mwp; x += 64) buf[x] = 0;
      __syncthreads();
      int left = 0;                                   // parity of the crossings left of the rectangle, this lane's edges
      if (live) {
        const bool scan = y >= vy0 && y < vy1;        // FillEdgeCollection's rows: ymin <= y < ymax of the polygon
        for (int k = lane; k < K; k += 64) {
          const int kp = k == 0 ? K - 1 : k - 1;
          int ax = pts[2 * kp], ay = pts[2 * kp + 1], bx = pts[2 * k], by = pts[2 * k + 1];
          if ((y < ay && y < by) || (y > ay && y > by)) continue;
          // ---- scan-line crossing: 16.16 fixed point, truncated slope, active for y0 <= y < y1
          if (scan && ay != by) {
            const long long X0 = (long long)ax << 16, X1 = (long long)bx << 16;
            const long long slope = ps_div(X1 - X0, (long long)by - ay);
            const int ey0 = ay < by ? ay : by, ey1 = ay < by ? by : ay;
            if (y >= ey0 && y < ey1) {
              const long long X = (ay < by ? X0 : X1) + ((long long)y - ey0) * slope;
              const long long r = (X + 32768) >> 16;
              if (r < xmin) {
                left ^= 1;
              } else if (r <= xmax) {
                atomicXor(&buf[(int)r - xmin], 1);
                atomicOr(&buf[(int)r - xmin], 2);
              }
            }
          }
          // ---- outline: the edge's Bresenham pixels on this row, iterated left to right
          if (bx < ax) { int q = ax; ax = bx; bx = q; q = ay; ay = by; by = q; }
          const long long dx = (long long)bx - ax;
          const long long dy = by >= ay ? (long long)by - ay : (long long)ay - by;
          const long long u = by >= ay ? (long long)y - ay : (long long)ay - y;      // 0 <= u <= dy: the row lies between the end points
          long long lo, hi;
          if (dy > dx) {                              // y-major: one pixel, minor position floor((2 dx u + dy - 1) / (2 dy))
            lo = hi = ax + ps_div(2 * dx * u + dy - 1, 2 * dy);
          } else if (dy == 0) {                       // horizontal, or a single point
            lo = ax; hi = bx;
          } else {                                    // x-major: the steps j whose minor position floor((2 dy j + dx - 1) / (2 dx)) is u
            const long long num = 2 * dx * u - dx + 1;
            const long long jlo = num <= 0 ? 0 : ps_div(num + 2 * dy - 1, 2 * dy);
            long long jhi = ps_div(2 * dx * (u + 1) - dx, 2 * dy);
            jhi = jhi > dx ? dx : jhi;
            lo = ax + jlo; hi = ax + jhi;
          }
          lo = lo < xmin ? xmin : lo;
          hi = hi > xmax ? xmax : hi;
          if (lo <= hi) {
            atomicAdd(&buf[(int)lo - xmin], 4);
            if (hi < xmax) atomicAdd(&buf[(int)hi - xmin + 1], -4);
          }
        }
      }
      __syncthreads();
      if (live) {
        int before = __popcll(__ballot(left)) & 1;    // parity of B(x) in front of the chunk
        int cover = 0;                                // cover count in front of the chunk
        const float* prow = pm + (size_t)y * a.W + xmin;
        for (int x0 = 0; x0 < mw; x0 += kPsChunk) {
          const int x = x0 + lane;
          const int v = buf[x];                       // x < mwp <= wpad: zero beyond mw
          int c = v >> 2;                             // inclusive scan of the interval ends
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(c, o);
            if (lane >= o) c += t;
          }
          const unsigned long long odd = __ballot(v & 1);
          const int b = (before + __popcll(odd & ((1ull << lane) - 1ull))) & 1;
          if (x < mw && (cover + c > 0 || (v & 2) || b)) {
            sum += (double)prow[x];
            ++cnt;
          }
          cover += __shfl(c, 63);
          before = (before + __popcll(odd)) & 1;
        }
      }
    }
  }
  // lanes, then waves, in a fixed order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o);
    cnt += __shfl_xor(cnt, o);
  }
  __syncthreads();                                    // the row buffers are done with: their first bytes carry the four partial results
  double* s_sum = reinterpret_cast<double*>(ps_lds);
  int32_t* s_cnt = ps_lds + 2 * kPsWaves;
  if (lane == 0) { s_sum[wave] = sum; s_cnt[wave] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kPsWaves; ++k) { sum += s_sum[k]; cnt += s_cnt[k]; }
    a.part_sum[(size_t)ci * kPsBands + band] = sum;
    a.part_cnt[(size_t)ci * kPsBands + band] = cnt;
  }
}

__global__ __launch_bounds__(256) void det_poly_finish_kernel(const double* __restrict__ part_sum, const int32_t* __restrict__ part_cnt, int nb,
                                                              float* __restrict__ scores, double* __restrict__ sums, int32_t* __restrict__ counts) {
  a16_kernel_enter();
  const int ci = blockIdx.x * 256 + threadIdx.x;
  if (ci >= nb) return;
  double sum = 0.0;
  int cnt = 0;
  for (int b = 0; b < kPsBands; ++b) {
    sum += part_sum[(size_t)ci * kPsBands + b];
    cnt += part_cnt[(size_t)ci * kPsBands + b];
  }
  scores[ci] = cnt > 0 ? (float)(sum / (double)cnt) : 0.f;
  if (sums) sums[ci] = sum;
  if (counts) counts[ci] = cnt;
}

}  // namespace

// host half (db_post.cpp, next to the contour tracer)
int db_contour_candidates_batch(const uint32_t* h_bitmaps, int n, int net_h, int net_w, int max_candidates, float min_size, int n_threads,
                                float* h_boxes, float* h_sside, int cap, int* n_out, int32_t* h_points, long long point_cap, int32_t* h_offsets,
                                long long* n_points_needed);

namespace PT_FMT_NS {
namespace api {

int pt_db_contour_candidates_batch(const uint32_t* h_bitmaps, int n, int net_h, int net_w, int max_candidates, float min_size, int n_threads,
                                   float* h_boxes, float* h_sside, int cap, int* n_out, int32_t* h_points, long long point_cap,
                                   int32_t* h_offsets, long long* n_points_needed) {
  return db_contour_candidates_batch(h_bitmaps, n, net_h, net_w, max_candidates, min_size, n_threads, h_boxes, h_sside, cap, n_out, h_points,
                                     point_cap, h_offsets, n_points_needed);
}

int pt_op_det_poly_scores(const float* d_prob, int n, int net_h, int net_w, const int32_t* d_points, int n_points, const int32_t* d_offsets,
                          const int32_t* h_offsets, const int32_t* d_pages, const int32_t* h_pages, int nb, float* d_scores, double* d_sums,
                          int32_t* d_counts, void* d_work, long long work_bytes, pt_stream stream) {
  PT_REQUIRE(nb >= 0, "pt_op_det_poly_scores: nb = %d is negative", nb);
  PT_REQUIRE(n >= 1 && net_h >= 1 && net_w >= 1 && n_points >= 0, "pt_op_det_poly_scores: bad sizes (n %d, map %d x %d, points %d)", n, net_h, net_w,
             n_points);
  PT_REQUIRE(net_w <= kPsMaxW, "pt_op_det_poly_scores: a map %d wide is beyond the row buffers (PT_DET_POLY_MAX_W = %d)", net_w, kPsMaxW);
  PT_REQUIRE((long long)n * net_h * net_w < (1LL << 40), "pt_op_det_poly_scores: batch too large");
  if (nb == 0) return PT_OK;
  PT_REQUIRE(d_prob && d_offsets && h_offsets && d_pages && h_pages && d_scores && d_work && (d_points || n_points == 0),
             "pt_op_det_poly_scores: null pointer");
  PT_REQUIRE(work_bytes >= (long long)nb * PT_DET_POLY_WORK_BYTES, "pt_op_det_poly_scores: work buffer of %lld bytes, %lld needed", work_bytes,
             (long long)nb * PT_DET_POLY_WORK_BYTES);
  PT_REQUIRE(h_offsets[0] >= 0 && h_offsets[nb] <= n_points, "pt_op_det_poly_scores: offsets %d .. %d outside the %d points", h_offsets[0],
             h_offsets[nb], n_points);
  for (int i = 0; i < nb; ++i) {
    PT_REQUIRE(h_offsets[i] <= h_offsets[i + 1], "pt_op_det_poly_scores: offsets decrease at candidate %d (%d, then %d)", i, h_offsets[i],
               h_offsets[i + 1]);
    PT_REQUIRE(h_pages[i] >= 0 && h_pages[i] < n, "pt_op_det_poly_scores: candidate %d names page %d of %d", i, h_pages[i], n);
  }
  PsArgs a;
  a.prob = d_prob; a.n = n; a.H = net_h; a.W = net_w; a.wpad = (net_w + kPsChunk - 1) & ~(kPsChunk - 1);
  a.points = d_points; a.n_points = n_points; a.offsets = d_offsets; a.pages = d_pages; a.nb = nb;
  a.part_sum = static_cast<double*>(d_work);
  a.part_cnt = reinterpret_cast<int32_t*>(a.part_sum + (size_t)nb * kPsBands);
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)kPsWaves * a.wpad * sizeof(int32_t);
  hipLaunchKernelGGL(det_poly_score_kernel, dim3(nb, kPsBands), dim3(kPsThreads), lds, st, a);
  PT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(det_poly_finish_kernel, dim3((nb + 255) / 256), dim3(256), 0, st, a.part_sum, a.part_cnt, nb, d_scores, d_sums, d_counts);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

}  // namespace api
}  // namespace PT_FMT_NS
