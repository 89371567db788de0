// layout_ops.hip -- the tail of a PicoDet ONNX export in one launch (pdf_table_amd/layout_stage.py: OnnxLayoutStage; entry point added under ABI 19).
// The graph ends in 2 L token-row activations: per level l the class PROBABILITIES [B, A_l, Cp_s] (ncls real channels) and the box-distribution logits
// [B, A_l, Cp_d] (32 real channels), 16-bit in the engine's storage format.  The host post-processor keeps only anchors whose best class probability
// passes the score threshold -- a few dozen of the ten thousand anchors of a page -- so bringing every anchor to the host costs 2 L blocking copies per
// batch.  Here the anchors that can pass are compacted on the device into the 48-float records of pt_layout_candidates:
//   (int32 level, int32 anchor, ncls class probabilities, 32 distribution logits, zeros up to 48)
// The kernel converts and copies only: value = float(hi) (+ float(lo), one fp32 add, in the pair mode).  Sigmoid, soft-max and box arithmetic stay on
// the host (LayoutStage.decode_page), which is what keeps the results equal to the host route's bit for bit.
// One thread per anchor of one page (blockIdx.y = page, so a wave never straddles two pages; it may straddle two levels).  A wave ballots its kept
// anchors, lane 0 reserves popcount slots with ONE atomicAdd on the page's counter, every kept lane's slot is the base plus the number of kept lanes below
// it.  The wave then writes its records one after the other, lane j the j-th float: 48 consecutive floats per record, the 32 distribution values
// converted by 32 lanes (the values are re-read by the lane that stores them: same bits, and the score rows are in the cache from the ballot
// pass).  Channels ncls .. Cp_s - 1 and 32 .. Cp_d - 1 are padding that may hold anything: they are never loaded.
// Loops: ncls (<= 14), the wave's popcount (<= 64, eight records per turn so that their loads overlap).  No flags, no spins; workgroups share the counters only.
#include "common.h"

namespace PT_FMT_NS {

namespace {

constexpr int kPicoMaxLevels = 4;
constexpr int kPicoDist = 32;         // 4 sides x (reg_max + 1 = 8) bins
constexpr int kPicoMaxCls = PT_LAYOUT_CAND_FLOATS - 2 - kPicoDist;      // 14
constexpr int kPicoTurn = 8;          // records a wave writes per turn of its store loop

struct PicoLevels {                   // by value in the kernel arguments: no device-side table to upload
  const bf16_t* score[kPicoMaxLevels];
  const bf16_t* dist[kPicoMaxLevels];
  int end[kPicoMaxLevels];            // anchors of levels 0 .. l (cumulative); levels past the last repeat the total
};

// level pointers by comparison, not by a run-time index into the argument struct (which would move it to private memory)
__device__ __forceinline__ const bf16_t* pico_pick(const bf16_t* const (&p)[kPicoMaxLevels], int l) {
  const bf16_t* r = p[0];
#pragma unroll
  for (int k = 1; k < kPicoMaxLevels; ++k)
    if (l == k) r = p[k];
  return r;
}

typedef const __attribute__((address_space(1))) bf16_t* pico_gptr;      // the level pointers travel inside a struct: say that they are global memory

// Both passes load WITHOUT a branch around the load, so that a lane's loads are in flight together (one memory round trip per pass and turn, not one
// per value): where a lane has nothing of its own to read it re-reads a real channel of a valid row and drops the value.
template <bool SPLIT>
__global__ __launch_bounds__(256) void pico_candidates_kernel(PicoLevels lv, int total, int cp_s, int cp_d, int ncls, float thr_lo, int max_cands,
                                                              int32_t* __restrict__ counts, float* __restrict__ cands) {
  a16_kernel_enter();
  const int page = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int g = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64 + lane;       // anchor of the page, levels laid end to end
  if (g - lane >= total) return;                                         // whole waves leave: lane 0 of a wave that stays owns an anchor
  const int lo_s = SPLIT ? cp_s : 0, rs_s = SPLIT ? 2 * cp_s : cp_s;     // offset of the lo half, row stride
  const int lo_d = SPLIT ? cp_d : 0, rs_d = SPLIT ? 2 * cp_d : cp_d;
  const int gc = g < total ? g : total - 1;                              // lanes past the last anchor re-read it and keep nothing
  int level = 0, first = 0, last = lv.end[0];
#pragma unroll
  for (int l = 0; l < kPicoMaxLevels - 1; ++l)
    if (gc >= lv.end[l]) { level = l + 1; first = lv.end[l]; last = lv.end[l + 1]; }
  const int anchor = gc - first;
  const int na = last - first;                                           // anchors of this lane's level
  // pass 1: the fp32 maximum of the ncls real channels.  Channel min(c, ncls - 1) for c < 14: a repeated channel does not change a maximum
  const pico_gptr sr = (pico_gptr)(pico_pick(lv.score, level) + ((long long)page * na + anchor) * rs_s);
  uint32_t hi[kPicoMaxCls], lo[kPicoMaxCls];
#pragma unroll
  for (int c = 0; c < kPicoMaxCls; ++c) {
    const int cc = c < ncls ? c : ncls - 1;
    hi[c] = sr[cc];
    lo[c] = SPLIT ? sr[lo_s + cc] : 0u;
  }
  float m = SPLIT ? a16_to_f32(hi[0]) + a16_to_f32(lo[0]) : a16_to_f32(hi[0]);
#pragma unroll
  for (int c = 1; c < kPicoMaxCls; ++c) m = fmaxf(m, SPLIT ? a16_to_f32(hi[c]) + a16_to_f32(lo[c]) : a16_to_f32(hi[c]));
  const bool keep = g < total && m > thr_lo;                             // strict, fp32; a NaN row is not a candidate
  unsigned long long mask = __ballot(keep);
  if (mask == 0ull) return;
  int base = 0;
  if (lane == 0) base = atomicAdd(counts + page, __popcll(mask));        // counts every candidate, also those beyond max_cands
  base = __shfl(base, 0);
  const int slot = base + __popcll(mask & ((1ull << lane) - 1ull));
  // pass 2: lane j writes float j of every kept record of the wave.  What it reads is fixed but for the row: a score channel (j = 2 .. 2 + ncls - 1), a
  // distribution channel (the 32 after them), or nothing (level, anchor, the zeros, lanes 48 .. 63: they re-read score channel 0)
  const bool is_score = lane >= 2 && lane < 2 + ncls;
  const bool is_dist = lane >= 2 + ncls && lane < 2 + ncls + kPicoDist;
  const int ch = is_dist ? lane - 2 - ncls : (is_score ? lane - 2 : 0);
  const int rs = is_dist ? rs_d : rs_s, lo_off = is_dist ? lo_d : lo_s;
  const bf16_t* src_l[kPicoMaxLevels];                                   // this lane's source tensor per level, in registers before the loop
#pragma unroll
  for (int l = 0; l < kPicoMaxLevels; ++l) src_l[l] = is_dist ? lv.dist[l] : lv.score[l];
  float* out = cands + (long long)page * max_cands * PT_LAYOUT_CAND_FLOATS + lane;
  while (mask) {                                                         // kPicoTurn kept anchors per turn
    int t_slot[kPicoTurn], t_level[kPicoTurn], t_anchor[kPicoTurn], t_na[kPicoTurn];
    uint32_t t_hi[kPicoTurn], t_lo[kPicoTurn];
#pragma unroll
    for (int k = 0; k < kPicoTurn; ++k) {                                // who: every cross-lane read of the turn before its first load
      const bool live = mask != 0ull;                                    // wave-uniform; a dead slot re-reads lane 0's row and stores nothing
      const int src = live ? __ffsll((long long)mask) - 1 : 0;
      mask &= mask - 1ull;                                               // 0 stays 0
      t_slot[k] = live ? __shfl(slot, src) : max_cands;
      t_level[k] = __shfl(level, src);
      t_anchor[k] = __shfl(anchor, src);
      t_na[k] = __shfl(na, src);
    }
#pragma unroll
    for (int k = 0; k < kPicoTurn; ++k) {                                // what: kPicoTurn (twice that in the pair mode) loads in flight
      const pico_gptr p = (pico_gptr)(pico_pick(src_l, t_level[k]) + ((long long)page * t_na[k] + t_anchor[k]) * rs + ch);
      t_hi[k] = p[0];
      t_lo[k] = SPLIT ? p[lo_off] : 0u;
    }
    // the loaded bits are pinned here, after the last load of the turn was issued: without it the compiler moves each load down into the predicated
    // store that uses it, and the turn's memory round trips follow one another again
#pragma unroll
    for (int k = 0; k < kPicoTurn; ++k) asm volatile("" : "+v"(t_hi[k]), "+v"(t_lo[k]));
#pragma unroll
    for (int k = 0; k < kPicoTurn; ++k) {
      const float val = SPLIT ? a16_to_f32(t_hi[k]) + a16_to_f32(t_lo[k]) : a16_to_f32(t_hi[k]);
      const float v = lane == 0 ? __int_as_float(t_level[k]) : lane == 1 ? __int_as_float(t_anchor[k]) : (is_score || is_dist) ? val : 0.f;
      if (t_slot[k] < max_cands && lane < PT_LAYOUT_CAND_FLOATS)         // only the first max_cands arrivals are stored
        out[(long long)t_slot[k] * PT_LAYOUT_CAND_FLOATS] = v;
    }
  }
}

}  // namespace

namespace api {

int pt_op_pico_candidates(pt_engine* e, const uint16_t* const* h_scores, const uint16_t* const* h_dists, const int32_t* h_anchors, int levels, int B,
                          int c_pad_s, int c_pad_d, int ncls, float thr_lo, int max_cands, int32_t* d_counts, float* d_cands, int split,
                          pt_stream stream) {
  PT_REQUIRE(e && h_scores && h_dists && h_anchors && d_counts && d_cands, "pt_op_pico_candidates: null argument");
  PT_REQUIRE(levels >= 1 && levels <= kPicoMaxLevels && B >= 1 && B <= 65535 && max_cands >= 1,
             "pt_op_pico_candidates: bad arguments (1 <= levels <= 4, 1 <= B <= 65535, max_cands >= 1)");
  PT_REQUIRE(ncls >= 1 && ncls <= kPicoMaxCls && ncls <= c_pad_s && kPicoDist <= c_pad_d,
             "pt_op_pico_candidates: %d classes + 32 distribution values do not fit a %d-float record behind (level, anchor), or exceed the row "
             "widths %d / %d", ncls, (int)PT_LAYOUT_CAND_FLOATS, c_pad_s, c_pad_d);
  PicoLevels lv;
  long long total = 0;
  for (int l = 0; l < kPicoMaxLevels; ++l) {
    if (l < levels) {
      PT_REQUIRE(h_scores[l] && h_dists[l] && h_anchors[l] >= 1, "pt_op_pico_candidates: level %d: null pointer or no anchors", l);
      total += h_anchors[l];
    }
    PT_REQUIRE(total < (1ll << 30), "pt_op_pico_candidates: more than 2^30 anchors per page");
    lv.score[l] = reinterpret_cast<const bf16_t*>(h_scores[l < levels ? l : levels - 1]);
    lv.dist[l] = reinterpret_cast<const bf16_t*>(h_dists[l < levels ? l : levels - 1]);
    lv.end[l] = (int)total;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  PT_HIP_CHECK(hipMemsetAsync(d_counts, 0, (size_t)B * sizeof(int32_t), s));     // a call is self-contained: nothing accumulates across calls
  const dim3 grid((unsigned)((total + 255) / 256), (unsigned)B), block(256);
  if (split) hipLaunchKernelGGL(pico_candidates_kernel<true>, grid, block, 0, s, lv, (int)total, c_pad_s, c_pad_d, ncls, thr_lo, max_cands, d_counts, d_cands);
  else hipLaunchKernelGGL(pico_candidates_kernel<false>, grid, block, 0, s, lv, (int)total, c_pad_s, c_pad_d, ncls, thr_lo, max_cands, d_counts, d_cands);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

}  // namespace api
}  // namespace PT_FMT_NS
