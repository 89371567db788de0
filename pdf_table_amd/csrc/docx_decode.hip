// docx_decode.hip -- the device half of DocXLayout's post-processor: DocXLayoutImagePostProcessor.post_process_model (docx_layout/
// image_processing_docxlayout.py:265-308: sigmoid, ctdet_4ps_decode = 3x3 peaks + joint top-100 + corner arithmetic, the cls / ftype arg-max) and pnms
// (processor_utils.py:121-158) over the head maps pt_docx_forward_net leaves in device memory, so that a page costs its two lists of at most K records
// (about 10 KB) on the copy the stage makes anyway.  Entry point pt_docx_decode, added under the current ABI number; no engine, one launch, no scratch.
// pdf_table_amd/docxlayout_stage.py holds the host half; tests/docxlayout_ref.py states the same arithmetic in torch / numpy.
//
// Shape built: ONE WORKGROUP PER (PAGE, BRANCH) (16 waves), 31 KB of static LDS.  A branch is a heat map (main: 11 classes at channel stride 16, sub: 2 at
// stride 8) with its wh and reg maps.
//   1. scan: every (pixel, class) of the map once, coalesced in memory order; a value with sigmoid >= thr_lo is tested against its in-map 3 x 3
//      neighbours of the same class (on the sigmoid values: distinct logits may round to one score) and a peak's key
//          score_bits << 32 | ~(class * h * w + pixel)          (pt_heat_peaks_topk's layout: larger key = earlier in the list)
//      is appended to an LDS list of kCap keys: a wave ballots its peaks and reserves popcount slots with ONE LDS atomic.  Every peak is counted, also
//      those that find the list full.
//   2. a page like any other has a few dozen peaks: the list holds them all and step 3 follows.  When MORE than kCap peaks were counted (a flat map
//      makes every value a peak) the K-th largest key is found exactly by a radix select -- five more scans, each a histogram of one digit of the keys
//      that agree with the digits fixed so far -- and a last scan collects the keys >= it: exactly K, whatever the number of peaks.  Seven scans at
//      most, no loop whose length depends on the data beyond that.
//   3. rank by counting: an entry's place is the number of larger keys in the list (keys are distinct); the first K places are written.
//   4. records: place r decodes its key, reads reg / wh (and cls / ftype) at its pixel, writes its 12 floats and leaves quad and score in LDS.
//   5. pnms on wave 0: lanes stride the records, the inner loop runs over the list (<= K).
// Barriers between the steps only, reached by all threads (every branch around them is workgroup-uniform).
//
// Arithmetic (-ffp-contract=off):
//   score   = pt_heat_sigmoid (common.h: the project's one fp32 sigmoid)
//   corners = single fp32 adds and subtracts: xs = float(x) + reg[0], ys = float(y) + reg[1], (xs - wh[2i], ys - wh[2i + 1])
//   arg-max = first maximum of the sigmoid values, as torch.argmax on the CPU returns
//   pnms    = float64 on the float32 records, as numpy does once the int64 arg-max columns have promoted the array: centre = (((x0 + x2) + x4) + x6) / 4,
//             edge products in the reference's operand order, strictly inside = all four > 0 or all four < 0.  The reference's loop reduces to: row i
//             (score >= 0.3) is dropped iff some other row j (score >= 0.3) holds i's centre strictly inside and has s_j > s_i.  Equal scores drop nothing.
// fp32 / fp64 / int32 arrays only: compiled ONCE (build.py: ONCE_HIP_SOURCES), as namespace pt_bf16.
#include <math.h>

#include "common.h"

using PT_FMT_NS::a16_kernel_enter;
using PT_FMT_NS::pt_heat_sigmoid;

namespace {

constexpr int kDxThreads = 1024;                   // 16 waves
constexpr int kDxUnroll = 4;                       // map values a thread has in flight per turn of a scan
constexpr int kDxCap = 2048;                       // keys the LDS list holds
constexpr int kDxBins = 2048;                      // 11-bit digits
constexpr int kDxMaxK = PT_DOCX_MAX_K;
constexpr int kDxIdxBits = 22;                     // class * h * w + pixel < 16 * 512 * 512
constexpr unsigned long long kDxIdxHigh = 0xFFFFFFFFull & ~((1ull << kDxIdxBits) - 1ull);      // bits of ~index that are always set

struct DxBranch {
  const float *hm, *wh, *reg, *cls, *ftype;        // cls / ftype: null for the sub branch
  int cs, ncls;                                    // channel stride and classes of hm
};

struct DxArgs {
  DxBranch br[2];
  int h, w, K;
  float thr_lo;
  int32_t* counts;
  float* recs;
  int32_t* inds;
  uint8_t* keep;
};

__device__ __forceinline__ unsigned long long dx_key(float s, int idx) {
  return ((unsigned long long)__float_as_uint(s) << 32) | (unsigned long long)(~(uint32_t)idx);
}

// One pass over the page's heat map: f(is_peak, key) is called kDxUnroll times per turn by every thread of the workgroup (wave-uniform trip count), so
// that f may ballot.  hm: the page's map [h * w][cs]
template <class F>
__device__ __forceinline__ void dx_scan(const float* __restrict__ hm, int h, int w, int cs, int ncls, float thr_lo, F&& f) {
  const int hw = h * w;
  const int total = hw * cs;
  const int turns = (total + kDxThreads * kDxUnroll - 1) / (kDxThreads * kDxUnroll);
  for (int t = 0; t < turns; ++t) {
    float x[kDxUnroll];
    int e[kDxUnroll];
#pragma unroll
    for (int u = 0; u < kDxUnroll; ++u) {
      e[u] = (t * kDxUnroll + u) * kDxThreads + (int)threadIdx.x;
      x[u] = hm[e[u] < total ? e[u] : total - 1];
    }
#pragma unroll
    for (int u = 0; u < kDxUnroll; ++u) {
      const int pix = (e[u] < total ? e[u] : total - 1) / cs;
      const int c = (e[u] < total ? e[u] : total - 1) - pix * cs;
      const float s = pt_heat_sigmoid(x[u]);
      bool peak = e[u] < total && c < ncls && s >= thr_lo;      // a NaN score is no peak
      if (peak) {
        const int y = pix / w, xx = pix - y * w;
#pragma unroll
        for (int d = 0; d < 9; ++d) {
          const int ny = y + d / 3 - 1, nx = xx + d % 3 - 1;
          if (d == 4 || ny < 0 || ny >= h || nx < 0 || nx >= w) continue;
          const float sn = pt_heat_sigmoid(hm[(ny * w + nx) * cs + c]);
          if (!(s >= sn)) peak = false;
        }
      }
      f(peak, dx_key(s, c * hw + pix));
    }
  }
}

// the wave's `take` lanes append `key` to list[0 .. cap): one LDS atomic per wave; *count counts every arrival
__device__ __forceinline__ void dx_append(bool take, unsigned long long key, unsigned long long* list, int cap, int* count) {
  const unsigned long long mask = __ballot(take);
  if (mask == 0ull) return;
  const int lane = threadIdx.x & 63;
  int base = 0;
  if (lane == __ffsll((long long)mask) - 1) base = atomicAdd(count, __popcll(mask));
  base = __shfl(base, __ffsll((long long)mask) - 1);
  const int slot = base + __popcll(mask & ((1ull << lane) - 1ull));
  if (take && slot < cap) list[slot] = key;
}

__global__ __launch_bounds__(kDxThreads) void docx_decode_kernel(DxArgs a) {
  a16_kernel_enter();
  __shared__ unsigned long long s_list[kDxCap];
  __shared__ unsigned long long s_sorted[kDxMaxK];
  __shared__ int s_hist[kDxBins];
  __shared__ int s_sums[256];
  __shared__ float s_quad[kDxMaxK][9];             // x0 y0 .. x3 y3, score
  __shared__ int s_count;
  __shared__ unsigned long long s_known, s_kmask;
  __shared__ int s_need;

  const int page = blockIdx.x >> 1, b = blockIdx.x & 1;
  const int tid = threadIdx.x, lane = tid & 63;
  const DxBranch br = b ? a.br[1] : a.br[0];
  const int h = a.h, w = a.w, hw = h * w, K = a.K;
  const float* hm = br.hm + (size_t)page * hw * br.cs;

  if (tid == 0) s_count = 0;
  __syncthreads();
  dx_scan(hm, h, w, br.cs, br.ncls, a.thr_lo, [&](bool peak, unsigned long long key) { dx_append(peak, key, s_list, kDxCap, &s_count); });
  __syncthreads();
  int cnt = s_count;                               // workgroup-uniform
  __syncthreads();

  if (cnt > kDxCap) {
    // radix select of the K-th largest key (cnt > kDxCap >= K): digits from the top; bits 22 .. 31 are set in every key
    if (tid == 0) { s_known = kDxIdxHigh; s_kmask = kDxIdxHigh; s_need = K; }
    const int shifts[5] = {53, 42, 32, 11, 0}, widths[5] = {11, 11, 10, 11, 11};
#pragma unroll 1
    for (int p = 0; p < 5; ++p) {
      for (int i = tid; i < kDxBins; i += kDxThreads) s_hist[i] = 0;
      __syncthreads();
      const unsigned long long known = s_known, kmask = s_kmask;
      const int shift = shifts[p], nb = 1 << widths[p];
      dx_scan(hm, h, w, br.cs, br.ncls, a.thr_lo, [&](bool peak, unsigned long long key) {
        const bool in = peak && (key & kmask) == known;
        const int digit = (int)((key >> shift) & (unsigned long long)(nb - 1));
        // the lanes that share the first such lane's digit add once (a flat map puts every key of a pass into one bin); the others one by one
        const unsigned long long m = __ballot(in);
        if (m == 0ull) return;
        const int d0 = __shfl(digit, __ffsll((long long)m) - 1);
        const unsigned long long same = __ballot(in && digit == d0);
        if (lane == __ffsll((long long)m) - 1) atomicAdd(&s_hist[d0], __popcll(same));
        if (in && digit != d0) atomicAdd(&s_hist[digit], 1);
      });
      __syncthreads();
      if (tid < 256) {
        int sum = 0;
#pragma unroll
        for (int k = 0; k < kDxBins / 256; ++k) sum += s_hist[tid * (kDxBins / 256) + k];
        s_sums[tid] = sum;
      }
      __syncthreads();
      if (tid == 0) {
        int need = s_need, g = 255;
        for (; g > 0 && s_sums[g] < need; --g) need -= s_sums[g];
        int d = g * (kDxBins / 256) + kDxBins / 256 - 1;
        for (; d > g * (kDxBins / 256) && s_hist[d] < need; --d) need -= s_hist[d];
        s_known = known | ((unsigned long long)d << shift);
        s_kmask = kmask | ((unsigned long long)(nb - 1) << shift);
        s_need = need;
      }
      __syncthreads();
    }
    const unsigned long long kth = s_known;
    if (tid == 0) s_count = 0;
    __syncthreads();
    dx_scan(hm, h, w, br.cs, br.ncls, a.thr_lo, [&](bool peak, unsigned long long key) { dx_append(peak && key >= kth, key, s_list, kDxCap, &s_count); });
    __syncthreads();
    cnt = s_count;
    cnt = cnt < kDxCap ? cnt : kDxCap;             // (exactly K by construction; never past the list)
  }

  // rank by counting; keys are distinct
  for (int i = tid; i < cnt; i += kDxThreads) {
    const unsigned long long mine = s_list[i];
    int rank = 0;
    for (int j = 0; j < cnt; ++j) rank += s_list[j] > mine ? 1 : 0;
    if (rank < K) s_sorted[rank] = mine;
  }
  const int M = cnt < K ? cnt : K;
  __syncthreads();

  const size_t row0 = ((size_t)page * 2 + b) * K;
  if (tid == 0) a.counts[page * 2 + b] = M;
  if (tid < M) {
    const unsigned long long key = s_sorted[tid];
    const float score = __uint_as_float((uint32_t)(key >> 32));
    int idx = (int)(~(uint32_t)key);
    idx = idx < 0 ? 0 : (idx > br.ncls * hw - 1 ? br.ncls * hw - 1 : idx);
    const int c = idx / hw, pix = idx - c * hw;
    const int y = pix / w, x = pix - y * w;
    const size_t p8 = ((size_t)page * hw + pix) * 8;
    const float xs = (float)x + br.reg[p8], ys = (float)y + br.reg[p8 + 1];
    float* o = a.recs + (row0 + tid) * PT_DOCX_REC_FLOATS;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float qx = xs - br.wh[p8 + 2 * k], qy = ys - br.wh[p8 + 2 * k + 1];
      o[2 * k] = qx; o[2 * k + 1] = qy;
      s_quad[tid][2 * k] = qx; s_quad[tid][2 * k + 1] = qy;
    }
    s_quad[tid][8] = score;
    int am_cls = 0, am_ft = 0;
    if (br.cls && br.ftype) {
      float best = pt_heat_sigmoid(br.cls[p8]);
#pragma unroll
      for (int k = 1; k < 4; ++k) {
        const float v = pt_heat_sigmoid(br.cls[p8 + k]);
        if (v > best) { best = v; am_cls = k; }
      }
      best = pt_heat_sigmoid(br.ftype[p8]);
#pragma unroll
      for (int k = 1; k < 3; ++k) {
        const float v = pt_heat_sigmoid(br.ftype[p8 + k]);
        if (v > best) { best = v; am_ft = k; }
      }
    }
    o[8] = score; o[9] = (float)c; o[10] = (float)am_cls; o[11] = (float)am_ft;
    if (a.inds) a.inds[row0 + tid] = idx;
  }
  __syncthreads();

  if (tid < 64) {
#pragma clang fp contract(off)
    for (int i = lane; i < M; i += 64) {
      const double si = (double)s_quad[i][8];
      bool keep = !(si < 0.3);
      if (keep) {
        const double ctx = ((((double)s_quad[i][0] + (double)s_quad[i][2]) + (double)s_quad[i][4]) + (double)s_quad[i][6]) / 4.0;
        const double cty = ((((double)s_quad[i][1] + (double)s_quad[i][3]) + (double)s_quad[i][5]) + (double)s_quad[i][7]) / 4.0;
        for (int j = 0; j < M; ++j) {
          const double sj = (double)s_quad[j][8];
          if (j == i || sj < 0.3) continue;
          const double x1 = s_quad[j][0], y1 = s_quad[j][1], x2 = s_quad[j][2], y2 = s_quad[j][3];
          const double x3 = s_quad[j][4], y3 = s_quad[j][5], x4 = s_quad[j][6], y4 = s_quad[j][7];
          const double ea = (x2 - x1) * (cty - y1) - (y2 - y1) * (ctx - x1);
          const double eb = (x3 - x2) * (cty - y2) - (y3 - y2) * (ctx - x2);
          const double ec = (x4 - x3) * (cty - y3) - (y4 - y3) * (ctx - x3);
          const double ed = (x1 - x4) * (cty - y4) - (y1 - y4) * (ctx - x4);
          const bool inside = (ea > 0 && eb > 0 && ec > 0 && ed > 0) || (ea < 0 && eb < 0 && ec < 0 && ed < 0);
          if (inside && si < sj) keep = false;
        }
      }
      a.keep[row0 + i] = keep ? 1 : 0;
    }
  }
}

}  // namespace

namespace PT_FMT_NS {
namespace api {

int pt_docx_decode(const float* d_hm, const float* d_wh, const float* d_reg, const float* d_cls, const float* d_ftype, const float* d_hm_sub,
                   const float* d_wh_sub, const float* d_reg_sub, int n, int h, int w, int ncls_main, int ncls_sub, int K, float thr_lo,
                   int32_t* d_counts, float* d_recs, int32_t* d_inds, uint8_t* d_keep, pt_stream stream) {
  PT_REQUIRE(d_hm && d_wh && d_reg && d_cls && d_ftype && d_hm_sub && d_wh_sub && d_reg_sub && d_counts && d_recs && d_keep,
             "pt_docx_decode: null pointer");
  PT_REQUIRE(n >= 1 && n <= 32767 && h >= 1 && w >= 1 && h <= 512 && w <= 512, "pt_docx_decode: bad arguments (n %d: 1 .. 32767, map %d x %d: 1 .. 512)", n, h,
             w);
  PT_REQUIRE(K >= 1 && K <= kDxMaxK, "pt_docx_decode: K = %d outside 1 .. %d", K, kDxMaxK);
  PT_REQUIRE(ncls_main >= 1 && ncls_main <= 16 && ncls_sub >= 1 && ncls_sub <= 8,
             "pt_docx_decode: %d main / %d sub classes outside the head maps' channel strides (16 / 8)", ncls_main, ncls_sub);
  PT_REQUIRE(thr_lo >= 0.f && thr_lo <= 1.f, "pt_docx_decode: thr_lo %g outside [0, 1]", (double)thr_lo);
  DxArgs a;
  a.br[0] = DxBranch{d_hm, d_wh, d_reg, d_cls, d_ftype, 16, ncls_main};
  a.br[1] = DxBranch{d_hm_sub, d_wh_sub, d_reg_sub, nullptr, nullptr, 8, ncls_sub};
  a.h = h; a.w = w; a.K = K; a.thr_lo = thr_lo;
  a.counts = d_counts; a.recs = d_recs; a.inds = d_inds; a.keep = d_keep;
  hipLaunchKernelGGL(docx_decode_kernel, dim3(2 * n), dim3(kDxThreads), 0, (hipStream_t)stream, a);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

}  // namespace api
}  // namespace PT_FMT_NS
