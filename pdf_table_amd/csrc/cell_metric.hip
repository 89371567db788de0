// cell_metric.hip -- the WTW cell metric's matching (TableEval.bubble_sort + PairTable.matching / eval_axis of the reference's utils/eval/eval_utils.py
// and entity/table_entity.py; pdf_table_amd/cell_metric.py states the same rule on the host) for a chunk of (prediction, truth) table pairs in one
// launch.  One new entry point under ABI 21, no existing signature changed.
//
// The rule: the reference sorts each table's cells with a bubble sort whose comparison is strict on (axis[2], axis[0], axis[3], axis[1]) -- a STABLE
// sort on that key -- and gives every truth cell the FIRST prediction cell, in that order, whose IoU reaches the threshold.  The first, not the best: a
// later cell with a higher IoU loses, and nothing is removed, so one prediction may serve several truth cells.
//
// Shape built: ONE WORKGROUP PER PAIR (4 waves), nothing shared between workgroups, no atomics, no spins.
//   phase 1  ranks the prediction cells BY COUNTING, no sort: rank(i) = #{j : key(j) < key(i)} over the key (axis[2], axis[0], axis[3], axis[1], input
//            index), folded into two biased uint64 words and the index.  The keys go through LDS in tiles of 3072 (48 KB); a thread owns up to 16
//            cells and compares every staged key (one broadcast LDS read) against all of them.  perm[rank] = input index, uint16 in LDS (8 KB).
//   phase 2  places the boxes with their axes in rank order in LDS, 1024 cells a tile (32 + 16 bytes a cell, 48 KB: the same LDS as phase 1's keys),
//            gathered through perm from the caller's arrays: no scratch.  A table of at most 1024 cells -- WTW's tables -- is placed whole, once.
//   phase 3  a truth cell is a lane: it walks the tile in ascending rank (every lane reads the same LDS address: a broadcast) and stops at its first
//            iou >= thr; a bit per owned truth cell remembers the match, so later tiles skip it.
//   tp / truep: __shfl_xor inside the wave, four partial sums through LDS.
// 56 KB + 32 bytes of static LDS: below the 64 KB a kernel gets unasked, two workgroups a CU.  Every loop is bounded by the clamped n_pred / n_gt, every
// index read from device memory (pair records, offsets, perm) is clamped before use.
//
// Arithmetic: float64, -ffp-contract=off, IEEE division; PairTable.compute_iou operation for operation on rec = (x1, y1, x3, y3):
//   l = max(g0, p0)  r = min(g2, p2)  u = max(g1, p1)  d = min(g3, p3);   l >= r or d <= u: 0
//   S1 = (g2 - g0) * (g3 - g1)   S2 = (p2 - p0) * (p3 - p1)   Sx = (d - u) * (r - l);   iou = Sx / ((S1 + S2) - Sx)
// Coordinates are finite (the host checks), so max / min need no NaN rule; a NaN quotient (inf / inf) fails >= on both routes.
// fp64 / int32 / int64 arrays only: compiled ONCE (build.py: ONCE_HIP_SOURCES), as namespace pt_bf16.
#include <math.h>

#include "common.h"

using PT_FMT_NS::a16_kernel_enter;

namespace {

constexpr int kCmThreads = 256;        // 4 waves
constexpr int kCmMax = PT_CELL_METRIC_MAX;
constexpr int kCmOwn = kCmMax / kCmThreads;      // cells a thread ranks: 16
constexpr int kCmTile = 1024;          // phase 2 / 3: cells per tile, 48 bytes each
constexpr int kCmKeyTile = 3072;       // phase 1: keys per tile, 16 bytes each
static_assert(kCmKeyTile * 16 == kCmTile * 48, "the two phases share one LDS region");
static_assert(kCmMax <= 65536, "perm is uint16");

__device__ __forceinline__ long long cm_clampl(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct CmKey {
  unsigned long long hi, lo;      // (axis[2], axis[0]) and (axis[3], axis[1]), each int32 biased by 2^31: unsigned order = signed lexicographic order
};

__device__ __forceinline__ CmKey cm_key(const int4 a) {
  CmKey k;
  k.hi = ((unsigned long long)((unsigned)a.z ^ 0x80000000u) << 32) | ((unsigned)a.x ^ 0x80000000u);
  k.lo = ((unsigned long long)((unsigned)a.w ^ 0x80000000u) << 32) | ((unsigned)a.y ^ 0x80000000u);
  return k;
}

__global__ __launch_bounds__(kCmThreads) void cell_metric_kernel(const double* __restrict__ boxes, const int32_t* __restrict__ axes, long long N,
                                                                 const long long* __restrict__ pairs, const long long* __restrict__ moff,
                                                                 long long match_elems, double thr, int32_t* __restrict__ match,
                                                                 int32_t* __restrict__ counts) {
  a16_kernel_enter();
  __shared__ __align__(16) unsigned char s_raw[kCmTile * 48];
  __shared__ uint16_t s_perm[kCmMax];
  __shared__ int s_red[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long* q = pairs + (size_t)blockIdx.x * 4;
  const int np = (int)cm_clampl(q[1], 0, kCmMax < N ? kCmMax : N), ng = (int)cm_clampl(q[3], 0, kCmMax < N ? kCmMax : N);
  const long long p0 = cm_clampl(q[0], 0, N - np), g0 = cm_clampl(q[2], 0, N - ng);
  const long long m0 = cm_clampl(moff[blockIdx.x], 0, match_elems - ng);
  if (m0 < 0 || p0 != q[0] || g0 != q[2] || m0 != moff[blockIdx.x]) return;      // block-uniform; the host refused this already: write nothing
  const int4* pax = reinterpret_cast<const int4*>(axes) + p0;
  const int4* gax = reinterpret_cast<const int4*>(axes) + g0;
  const double2* pbox = reinterpret_cast<const double2*>(boxes) + 2 * p0;
  const double2* gbox = reinterpret_cast<const double2*>(boxes) + 2 * g0;
  int32_t* out = match + m0;

  // ---- phase 1: rank by counting ----
  {
    CmKey* s_key = reinterpret_cast<CmKey*>(s_raw);
    CmKey mine[kCmOwn];
    int cnt[kCmOwn];
#pragma unroll
    for (int k = 0; k < kCmOwn; ++k) {
      const int i = tid + k * kCmThreads;
      cnt[k] = 0;
      mine[k].hi = mine[k].lo = 0;
      if (i < np) mine[k] = cm_key(pax[i]);
    }
    for (int t0 = 0; t0 < np; t0 += kCmKeyTile) {                         // block-uniform
      const int tn = np - t0 < kCmKeyTile ? np - t0 : kCmKeyTile;
      for (int j = tid; j < tn; j += kCmThreads) s_key[j] = cm_key(pax[t0 + j]);
      __syncthreads();
      for (int j = 0; j < tn; ++j) {
        const CmKey kj = s_key[j];
        const int ij = t0 + j;
#pragma unroll
        for (int k = 0; k < kCmOwn; ++k) {
          if (k * kCmThreads < np) {                                       // block-uniform
            const int i = tid + k * kCmThreads;
            const bool less = kj.hi < mine[k].hi || (kj.hi == mine[k].hi && (kj.lo < mine[k].lo || (kj.lo == mine[k].lo && ij < i)));
            cnt[k] += less ? 1 : 0;
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < kCmOwn; ++k) {
      const int i = tid + k * kCmThreads;
      if (i < np) s_perm[cnt[k] < np ? cnt[k] : np - 1] = (uint16_t)i;   // the ranks are a permutation of 0 .. np - 1; the clamp is for the eye
    }
  }
  for (int g = tid; g < ng; g += kCmThreads) out[g] = -1;
  __syncthreads();

  // ---- phases 2 and 3, tile by tile ----
  double2* s_box = reinterpret_cast<double2*>(s_raw);                      // [kCmTile][2]: (x1, y1), (x3, y3)
  int4* s_ax = reinterpret_cast<int4*>(s_raw + kCmTile * 32);              // [kCmTile]
  int tp = 0, truep = 0;
  unsigned done = 0;                                                       // bit k: this thread's truth cell tid + k * 256 has its match
  for (int t0 = 0; t0 < np; t0 += kCmTile) {                              // block-uniform
    const int tn = np - t0 < kCmTile ? np - t0 : kCmTile;
    for (int r = tid; r < tn; r += kCmThreads) {
      int i = s_perm[t0 + r];
      i = i < np ? i : np - 1;
      s_box[2 * r] = pbox[2 * i];
      s_box[2 * r + 1] = pbox[2 * i + 1];
      s_ax[r] = pax[i];
    }
    __syncthreads();
    for (int k = 0, g = tid; g < ng; ++k, g += kCmThreads) {              // k < kCmOwn: ng <= kCmMax
      if ((done >> k) & 1u) continue;                                      // matched in an earlier tile
      const double2 ga = gbox[2 * g], gb = gbox[2 * g + 1];
      const double S1 = (gb.x - ga.x) * (gb.y - ga.y);
      int found = -1;
      for (int r = 0; r < tn; ++r) {
        const double2 pa = s_box[2 * r], pb = s_box[2 * r + 1];
        const double l = fmax(ga.x, pa.x), rt = fmin(gb.x, pb.x), u = fmax(ga.y, pa.y), d = fmin(gb.y, pb.y);
        if (l >= rt || d <= u) continue;
        const double S2 = (pb.x - pa.x) * (pb.y - pa.y);
        const double Sx = (d - u) * (rt - l);
        if (Sx / ((S1 + S2) - Sx) >= thr) {
          found = r;
          break;
        }
      }
      if (found >= 0) {
        int i = s_perm[t0 + found];
        out[g] = i < np ? i : np - 1;
        done |= 1u << k;
        const int4 a = s_ax[found], b = gax[g];
        tp += 1;
        truep += (a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w) ? 1 : 0;
      }
    }
    __syncthreads();
  }

  // ---- tp / truep ----
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    tp += __shfl_xor(tp, o);
    truep += __shfl_xor(truep, o);
  }
  if (lane == 0) {
    s_red[2 * wave] = tp;
    s_red[2 * wave + 1] = truep;
  }
  __syncthreads();
  if (tid == 0) {
    counts[2 * blockIdx.x] = s_red[0] + s_red[2] + s_red[4] + s_red[6];
    counts[2 * blockIdx.x + 1] = s_red[1] + s_red[3] + s_red[5] + s_red[7];
  }
}

}  // namespace

namespace PT_FMT_NS {
namespace api {

int pt_op_cell_metric(const double* d_boxes, const int32_t* d_axes, long long N, const int64_t* d_pairs, const int64_t* h_pairs, int P,
                      const int64_t* d_moff, const int64_t* h_moff, double iou_threshold, int32_t* d_match, long long match_elems, int32_t* d_counts,
                      pt_stream stream) {
  PT_REQUIRE(P >= 0 && P <= 65535 && N >= 0 && match_elems >= 0, "pt_op_cell_metric: bad arguments (P %d: 0 .. 65535, N %lld, match_elems %lld)", P, N,
             match_elems);
  PT_REQUIRE(iou_threshold > 0.0, "pt_op_cell_metric: the IoU threshold must be positive (not %g)", iou_threshold);
  if (P == 0) return PT_OK;
  PT_REQUIRE(d_pairs && h_pairs && d_moff && h_moff && d_counts, "pt_op_cell_metric: null pointer");
  long long end = 0;
  for (int p = 0; p < P; ++p) {
    const int64_t* q = h_pairs + (size_t)p * 4;
    PT_REQUIRE(q[1] >= 0 && q[1] <= kCmMax && q[3] >= 0 && q[3] <= kCmMax, "pt_op_cell_metric: pair %d has %lld and %lld cells, outside 0 .. %d", p,
               (long long)q[1], (long long)q[3], kCmMax);
    PT_REQUIRE(q[0] >= 0 && q[0] <= N - q[1] && q[2] >= 0 && q[2] <= N - q[3], "pt_op_cell_metric: pair %d names cells %lld + %lld and %lld + %lld of %lld",
               p, (long long)q[0], (long long)q[1], (long long)q[2], (long long)q[3], N);
    PT_REQUIRE(h_moff[p] >= end && h_moff[p] <= match_elems - q[3], "pt_op_cell_metric: pair %d writes %lld matches at %lld (after %lld), d_match holds %lld",
               p, (long long)q[3], (long long)h_moff[p], end, match_elems);
    end = h_moff[p] + q[3];
  }
  PT_REQUIRE(N == 0 || (d_boxes && d_axes), "pt_op_cell_metric: null pointer (cells)");
  PT_REQUIRE(end == 0 || d_match, "pt_op_cell_metric: null pointer (d_match)");
  PT_REQUIRE((reinterpret_cast<uintptr_t>(d_boxes) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_axes) & 15) == 0,
             "pt_op_cell_metric: boxes and axes must be 16-byte aligned");
  hipLaunchKernelGGL(cell_metric_kernel, dim3((unsigned)P), dim3(kCmThreads), 0, (hipStream_t)stream, d_boxes, d_axes, N,
                     reinterpret_cast<const long long*>(d_pairs), reinterpret_cast<const long long*>(d_moff), match_elems, iou_threshold, d_match,
                     d_counts);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

}  // namespace api
}  // namespace PT_FMT_NS
