// layout_decode.hip -- the PicoDet post-processor behind the candidate records, on the device: LayoutStage.decode_page (pdf_table_amd/layout_stage.py;
// OCRPicodetPostProcessor.__call__, picodet/processor_picodet.py:184-298) -- sigmoid, the DFL soft-max, the boxes, the per-level top-K, the per-class
// score threshold, the candidate_size best and the greedy hard NMS (pt_hard_nms, db_post.cpp), the clip and the rescale -- over the records
// pt_layout_candidates / pt_op_pico_candidates leave in device memory, so that a page costs ncls * keep_top_k detections of 48 bytes on the copy the
// stage makes anyway instead of max_cands records of 192 bytes and a Python pass per page.  One new entry point under ABI 20, no existing signature changed.
//
// Shape built: ONE WORKGROUP PER PAGE (4 waves), everything in 47 KB of static LDS, no scratch.
//   1. every record once: level and anchor (clamped; a level outside [0, levels) drops the record), the class scores, their maximum -> LDS (8 bytes per
//      record), the records per level counted with LDS atomics.
//   2. a level with more than nms_top_k records ranks them BY COUNTING: a record stays when fewer than nms_top_k records of its level precede it in the
//      key (max score descending, anchor ascending).  Levels the cut does not touch skip the pass.
//   3. classes in rounds of four.  Per class the workgroup compacts the records whose class score is > score_threshold into LDS (ballot + one LDS atomic
//      per wave; the arrival order does not matter), ranks them by counting in the key (score descending, then level, then anchor ascending) and writes
//      the candidate_size best, in that order, into the list of the wave that owns the class.  The wave then decodes its <= 256 candidates (lane e owns
//      entries e, e + 64, ...: DFL soft-max and box in registers) and runs the greedy loop: the first live entry is picked (ballot), its box is broadcast
//      (__shfl), every lane tests its live entries against it.  No workgroup barrier inside that loop; at most candidate_size turns.  Barriers between
//      the phases only, all reached by all 256 threads (every loop bound around them is workgroup-uniform).
//   4. after a round's four classes the picks are written at the page's running offset, classes ascending, within a class in pick order.
// A candidate that passes in two classes is decoded twice (rare); nobody decodes a record no class keeps.
//
// EQUAL SCORES.  numpy's default arg-sort is not stable, so the host has no tie rule one could match: among equal scores it keeps and orders whatever its
// introsort leaves.  The rule here is the key above -- (score descending, level ascending, anchor ascending) -- which makes the result independent of
// the order in which the records arrived.  (Two records with the same level AND anchor never come out of the candidate kernels; they would be ordered by
// their position in the buffer.)  A NaN class score is never a candidate (NaN > threshold is false, as on the host); the per-level maximum skips NaN.
//
// Arithmetic (-ffp-contract=off; decode_page line by line):
//   score    = probs ? the record's float32 : 1.0f / (1.0f + e) with e = fl32(exp(-(double)x)): torch.sigmoid's float32 formula with a correctly rounded exp
//   fm_w     = ceil(inp_w / stride) (np.arange(608 / 64) has ten elements); centre = ((a % fm_w) + 0.5) * stride, ((a / fm_w) + 0.5) * stride, exact
//   soft-max = float32: m = max of the 8 bins, e_k = fl32(exp((double)(x_k - m))), s = ((e0+e1)+(e2+e3))+((e4+e5)+(e6+e7)) (numpy's pairwise order), p_k = e_k / s
//   distance = float64: p_k * k widened (numpy promotes float32 * int64 to float64), summed in the same pairwise order, * stride
//   box      = float64 (cx - d0, cy - d1, cx + d2, cy + d3)
//   iou      = float64, pt_hard_nms's order: inter / (((bw * bh + cw * ch) - inter) + 1e-5), widths and heights clamped at 0; an entry stays when iou <= thr
//   output   = min / max per axis, clip to [0, org_w] x [0, org_h], round to float32, divide in float64 by fl32(inp_w / org_w), fl32(inp_h / org_h)
// fp32 / fp64 / int32 arrays only: compiled ONCE (build.py: ONCE_HIP_SOURCES), as namespace pt_bf16.
#include <math.h>

#include "common.h"

using PT_FMT_NS::a16_kernel_enter;

namespace {

constexpr int kLdThreads = 256;                    // 4 waves
constexpr int kLdWaves = kLdThreads / 64;
constexpr int kLdMaxCands = 4096;                  // records per page the LDS plan holds: 10 bytes each
constexpr int kLdPerThread = kLdMaxCands / kLdThreads;
constexpr int kLdMaxSel = 256;                     // candidate_size the plan holds: 4 entries per lane, 6 bytes each per wave
constexpr int kLdPerLane = kLdMaxSel / 64;
constexpr int kLdDist = 32;                        // 4 sides x 8 bins
constexpr int kLdMaxCls = PT_LAYOUT_CAND_FLOATS - 2 - kLdDist;      // 14
constexpr int kLdMaxLevels = 4;
constexpr uint32_t kLdDropped = 0xffffffffu;       // key of a record that takes no further part
constexpr int kLdAnchorMax = 0x3ffffffe;           // level << 30 | anchor never equals kLdDropped

struct LdArgs {
  int max_cands, ncls, levels, stride[kLdMaxLevels];
  int inp_h, inp_w, org_h, org_w, probs;
  float score_threshold;
  double nms_threshold;
  int nms_top_k, candidate_size, keep_top_k, max_dets;
};

__device__ __forceinline__ float ld_score(float x, int probs) {
  if (probs) return x;
  const float e = (float)exp(-(double)x);
  return 1.0f / (1.0f + e);
}

// (score descending, key ascending, position ascending): does a precede b?
__device__ __forceinline__ bool ld_before(float sa, uint32_t ka, int ia, float sb, uint32_t kb, int ib) {
  if (sa != sb) return sa > sb;
  if (ka != kb) return ka < kb;
  return ia < ib;
}

// one side's expected bin: the float32 soft-max of 8 logits, then sum(p_k * k) in float64
__device__ __forceinline__ double ld_side(const float* __restrict__ x) {
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = x[k];
  float m = v[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) m = (v[k] > m || v[k] != v[k]) ? v[k] : m;      // np.max: a NaN wins and stays
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = (float)exp((double)(v[k] - m));
  const float s = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
  double t[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) t[k] = (double)(v[k] / s) * (double)k;
  return ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
}

__global__ __launch_bounds__(kLdThreads) void layout_decode_kernel(const int32_t* __restrict__ counts, const float* __restrict__ cands, LdArgs a,
                                                                   int32_t* __restrict__ ndet, double* __restrict__ dets) {
  a16_kernel_enter();
  __shared__ float lds_s[kLdMaxCands];             // phase 1-2: a record's best class score; phase 3: the compacted class scores
  __shared__ uint32_t lds_key[kLdMaxCands];        // level << 30 | anchor, or kLdDropped
  __shared__ uint16_t lds_idx[kLdMaxCands];        // phase 3: the compacted records' positions
  __shared__ uint16_t lds_sel[kLdWaves][kLdMaxSel];   // per wave: its class's best candidates in key order
  __shared__ float lds_sel_s[kLdWaves][kLdMaxSel];
  __shared__ int lds_level_n[kLdMaxLevels];
  __shared__ int lds_m;                            // compacted records of the class in work
  __shared__ int lds_nsel[kLdWaves], lds_npick[kLdWaves];

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int n = counts[b];
  n = n < 0 ? 0 : (n > a.max_cands ? a.max_cands : n);        // max_cands <= kLdMaxCands (checked before the launch)
  const float* __restrict__ rec0 = cands + (size_t)b * a.max_cands * PT_LAYOUT_CAND_FLOATS;
  const int ncls = a.ncls;

  // ---- 1: keys, best scores, records per level
  if (tid < kLdMaxLevels) lds_level_n[tid] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += kLdThreads) {
    const float* r = rec0 + (size_t)i * PT_LAYOUT_CAND_FLOATS;
    const int level = __float_as_int(r[0]);
    int anchor = __float_as_int(r[1]);
    anchor = anchor < 0 ? 0 : (anchor > kLdAnchorMax ? kLdAnchorMax : anchor);
    const bool valid = level >= 0 && level < a.levels;
    float best = -INFINITY;
    for (int c = 0; c < ncls; ++c) best = fmaxf(best, ld_score(r[2 + c], a.probs));      // fmaxf skips NaN
    lds_s[i] = best;
    lds_key[i] = valid ? ((uint32_t)level << 30) | (uint32_t)anchor : kLdDropped;
    if (valid) atomicAdd(&lds_level_n[level], 1);
  }
  __syncthreads();

  // ---- 2: the per-level top nms_top_k, by counting; only where a level has more
  bool cut = false;
#pragma unroll
  for (int l = 0; l < kLdMaxLevels; ++l) cut = cut || lds_level_n[l] > a.nms_top_k;
  if (cut) {                                                  // workgroup-uniform
    uint32_t drop = 0;                                        // bit k: record tid + k * 256 falls behind the cut
#pragma unroll 1
    for (int k = 0; k < kLdPerThread; ++k) {
      const int i = tid + k * kLdThreads;
      if (i >= n) break;
      const uint32_t ki = lds_key[i];
      if (ki == kLdDropped || lds_level_n[ki >> 30] <= a.nms_top_k) continue;
      const float si = lds_s[i];
      int before = 0;
      for (int j = 0; j < n; ++j) {
        const uint32_t kj = lds_key[j];
        before += (kj != kLdDropped && (kj >> 30) == (ki >> 30) && ld_before(lds_s[j], kj, j, si, ki, i)) ? 1 : 0;
      }
      if (before >= a.nms_top_k) drop |= 1u << k;
    }
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < kLdPerThread; ++k)
      if (drop & (1u << k)) lds_key[tid + k * kLdThreads] = kLdDropped;
    __syncthreads();
  }

  // ---- 3: classes in rounds of four, one wave per class
  const double ow = (double)(float)a.org_w, oh = (double)(float)a.org_h;
  const double sf_h = (double)(float)((double)a.inp_h / (double)a.org_h), sf_w = (double)(float)((double)a.inp_w / (double)a.org_w);
  int base = 0;                                               // detections of the classes before this round
  for (int c0 = 0; c0 < ncls; c0 += kLdWaves) {
    // 3a: the lists, class by class, by the whole workgroup
    for (int w = 0; w < kLdWaves; ++w) {
      const int c = c0 + w;
      if (c >= ncls) {                                        // uniform
        if (tid == 0) lds_nsel[w] = 0;
        continue;
      }
      if (tid == 0) lds_m = 0;
      __syncthreads();
      for (int i0 = wave * 64; i0 < n; i0 += kLdThreads) {    // wave-uniform bound: every lane reaches the ballot
        const int i = i0 + lane;
        float s = 0.f;
        bool pass = false;
        if (i < n && lds_key[i] != kLdDropped) {
          s = ld_score(rec0[(size_t)i * PT_LAYOUT_CAND_FLOATS + 2 + c], a.probs);
          pass = s > a.score_threshold;                       // float32, strict; false for NaN
        }
        const unsigned long long mask = __ballot(pass);
        int slot = 0;
        if (lane == 0 && mask) slot = atomicAdd(&lds_m, __popcll(mask));
        slot = __shfl(slot, 0) + __popcll(mask & ((1ull << lane) - 1ull));
        if (pass) {                                           // at most n <= kLdMaxCands records pass
          lds_s[slot] = s;
          lds_idx[slot] = (uint16_t)i;
        }
      }
      __syncthreads();
      const int m = lds_m;
      for (int e = tid; e < m; e += kLdThreads) {
        const float se = lds_s[e];
        const int ie = lds_idx[e];
        const uint32_t ke = lds_key[ie];
        int before = 0;
        for (int f = 0; f < m; ++f) {
          const float sf = lds_s[f];
          if (sf > se) ++before;
          else if (sf == se) {
            const int jf = lds_idx[f];
            before += ld_before(sf, lds_key[jf], jf, se, ke, ie) ? 1 : 0;
          }
        }
        if (before < a.candidate_size) {                      // candidate_size <= kLdMaxSel; ranks are distinct
          lds_sel[w][before] = (uint16_t)ie;
          lds_sel_s[w][before] = se;
        }
      }
      if (tid == 0) lds_nsel[w] = m < a.candidate_size ? m : a.candidate_size;
      __syncthreads();
    }
    __syncthreads();

    // 3b: the wave's class: decode its candidates, greedy NMS
    const int nsel = lds_nsel[wave];
    double bx0[kLdPerLane], by0[kLdPerLane], bx1[kLdPerLane], by1[kLdPerLane];
    float sc[kLdPerLane];
    bool live[kLdPerLane];
    int pos[kLdPerLane];                                      // pick order, -1: not picked
#pragma unroll
    for (int k = 0; k < kLdPerLane; ++k) {
      const int e = lane + 64 * k;
      live[k] = e < nsel;
      pos[k] = -1;
      bx0[k] = by0[k] = bx1[k] = by1[k] = 0.0;
      sc[k] = 0.f;
      if (live[k]) {
        const int i = lds_sel[wave][e];                       // < n: written from a record position above
        sc[k] = lds_sel_s[wave][e];
        const uint32_t key = lds_key[i];
        int level = (int)(key >> 30);
        level = level < a.levels ? level : a.levels - 1;
        const int anchor = (int)(key & 0x3fffffffu);
        int stride = a.stride[0];
#pragma unroll
        for (int l = 1; l < kLdMaxLevels; ++l)
          if (level == l) stride = a.stride[l];
        const int fm_w = (a.inp_w + stride - 1) / stride;
        const double cx = ((double)(anchor % fm_w) + 0.5) * (double)stride, cy = ((double)(anchor / fm_w) + 0.5) * (double)stride;
        const float* d = rec0 + (size_t)i * PT_LAYOUT_CAND_FLOATS + 2 + ncls;
        bx0[k] = cx - ld_side(d) * (double)stride;
        by0[k] = cy - ld_side(d + 8) * (double)stride;
        bx1[k] = cx + ld_side(d + 16) * (double)stride;
        by1[k] = cy + ld_side(d + 24) * (double)stride;
      }
    }
    int npick = 0;
    for (int t = 0; t < kLdMaxSel; ++t) {                     // every turn picks one entry: at most nsel <= kLdMaxSel turns
      int cur_k = -1, cur_lane = 0;
#pragma unroll
      for (int k = kLdPerLane - 1; k >= 0; --k) {
        const unsigned long long mask = __ballot(live[k]);
        if (mask) { cur_k = k; cur_lane = __ffsll((long long)mask) - 1; }
      }
      if (cur_k < 0) break;                                   // wave-uniform
      double c0x = bx0[0], c0y = by0[0], c1x = bx1[0], c1y = by1[0];
#pragma unroll
      for (int k = 1; k < kLdPerLane; ++k)
        if (cur_k == k) { c0x = bx0[k]; c0y = by0[k]; c1x = bx1[k]; c1y = by1[k]; }
      c0x = __shfl(c0x, cur_lane);
      c0y = __shfl(c0y, cur_lane);
      c1x = __shfl(c1x, cur_lane);
      c1y = __shfl(c1y, cur_lane);
#pragma unroll
      for (int k = 0; k < kLdPerLane; ++k)
        if (cur_k == k && lane == cur_lane) { live[k] = false; pos[k] = npick; }
      ++npick;
      if (a.keep_top_k > 0 && npick == a.keep_top_k) break;
      double cw = c1x - c0x, ch = c1y - c0y;
      cw = cw < 0.0 ? 0.0 : cw;
      ch = ch < 0.0 ? 0.0 : ch;
      const double a1 = cw * ch;
#pragma unroll
      for (int k = 0; k < kLdPerLane; ++k) {
        if (!live[k]) continue;
        double w_ = (bx1[k] < c1x ? bx1[k] : c1x) - (bx0[k] > c0x ? bx0[k] : c0x);
        double h_ = (by1[k] < c1y ? by1[k] : c1y) - (by0[k] > c0y ? by0[k] : c0y);
        w_ = w_ < 0.0 ? 0.0 : w_;
        h_ = h_ < 0.0 ? 0.0 : h_;
        const double inter = w_ * h_;
        double bw = bx1[k] - bx0[k], bh = by1[k] - by0[k];
        bw = bw < 0.0 ? 0.0 : bw;
        bh = bh < 0.0 ? 0.0 : bh;
        const double iou = inter / (((bw * bh + a1) - inter) + 1e-5);
        live[k] = iou <= a.nms_threshold;
      }
    }
    if (lane == 0) lds_npick[wave] = npick;
    __syncthreads();

    // 4: this round's picks behind those of the classes before
    int off = base, total = 0;
#pragma unroll
    for (int w = 0; w < kLdWaves; ++w) {
      const int np = lds_npick[w];
      off += w < wave ? np : 0;
      total += np;
    }
    const int cls = c0 + wave;
#pragma unroll
    for (int k = 0; k < kLdPerLane; ++k) {
      if (pos[k] < 0) continue;
      const int o = off + pos[k];
      if (o >= a.max_dets) continue;                          // counted in ndet, not written
      double x0 = bx0[k] < bx1[k] ? bx0[k] : bx1[k], x1 = bx0[k] > bx1[k] ? bx0[k] : bx1[k];
      double y0 = by0[k] < by1[k] ? by0[k] : by1[k], y1 = by0[k] > by1[k] ? by0[k] : by1[k];
      x0 = x0 < 0.0 ? 0.0 : (x0 > ow ? ow : x0);
      x1 = x1 < 0.0 ? 0.0 : (x1 > ow ? ow : x1);
      y0 = y0 < 0.0 ? 0.0 : (y0 > oh ? oh : y0);
      y1 = y1 < 0.0 ? 0.0 : (y1 > oh ? oh : y1);
      double* out = dets + ((size_t)b * a.max_dets + o) * 6;
      out[0] = (double)(float)x0 / sf_w;
      out[1] = (double)(float)y0 / sf_h;
      out[2] = (double)(float)x1 / sf_w;
      out[3] = (double)(float)y1 / sf_h;
      out[4] = (double)sc[k];
      out[5] = (double)cls;
    }
    base += total;
    __syncthreads();                                          // the lists and counters are rewritten by the next round
  }
  if (tid == 0) ndet[b] = base;
}

}  // namespace

namespace PT_FMT_NS {
namespace api {

int pt_op_layout_decode(const int32_t* d_counts, const float* d_cands, int B, int max_cands, int ncls, int levels, const int32_t* h_strides, int inp_h,
                        int inp_w, int org_h, int org_w, int probs, float score_threshold, double nms_threshold, int nms_top_k, int candidate_size,
                        int keep_top_k, int max_dets, int32_t* d_ndet, double* d_dets, pt_stream stream) {
  PT_REQUIRE(d_counts && d_cands && h_strides && d_ndet && d_dets, "pt_op_layout_decode: null pointer");
  PT_REQUIRE(ncls >= 1 && ncls <= kLdMaxCls, "pt_op_layout_decode: %d classes: a candidate record holds 1 .. %d", ncls, kLdMaxCls);
  PT_REQUIRE(levels >= 1 && levels <= kLdMaxLevels, "pt_op_layout_decode: %d levels: 1 .. %d are built", levels, kLdMaxLevels);
  PT_REQUIRE(candidate_size >= 1 && candidate_size <= kLdMaxSel, "pt_op_layout_decode: candidate_size %d: the kernel's LDS plan holds 1 .. %d per class",
             candidate_size, kLdMaxSel);
  PT_REQUIRE(max_cands >= 1 && max_cands <= kLdMaxCands, "pt_op_layout_decode: max_cands %d: the kernel's LDS plan holds 1 .. %d records per page", max_cands,
             kLdMaxCands);
  PT_REQUIRE(B >= 1 && B <= 65535 && nms_top_k >= 1 && max_dets >= 1 && inp_h >= 1 && inp_w >= 1 && org_h >= 1 && org_w >= 1,
             "pt_op_layout_decode: bad arguments (B %d: 1 .. 65535; nms_top_k %d, max_dets %d, input %d x %d, page %d x %d: all >= 1)", B, nms_top_k,
             max_dets, inp_h, inp_w, org_h, org_w);
  PT_REQUIRE((reinterpret_cast<uintptr_t>(d_dets) & 7) == 0, "pt_op_layout_decode: dets must be 8-byte aligned");
  LdArgs a;
  a.max_cands = max_cands;
  a.ncls = ncls;
  a.levels = levels;
  for (int l = 0; l < kLdMaxLevels; ++l) {
    a.stride[l] = h_strides[l < levels ? l : levels - 1];
    PT_REQUIRE(a.stride[l] >= 1, "pt_op_layout_decode: stride %d of level %d", a.stride[l], l);
  }
  a.inp_h = inp_h;
  a.inp_w = inp_w;
  a.org_h = org_h;
  a.org_w = org_w;
  a.probs = probs ? 1 : 0;
  a.score_threshold = score_threshold;
  a.nms_threshold = nms_threshold;
  a.nms_top_k = nms_top_k;
  a.candidate_size = candidate_size;
  a.keep_top_k = keep_top_k;
  a.max_dets = max_dets;
  hipLaunchKernelGGL(layout_decode_kernel, dim3(B), dim3(kLdThreads), 0, (hipStream_t)stream, d_counts, d_cands, a, d_ndet, d_dets);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

}  // namespace api
}  // namespace PT_FMT_NS
