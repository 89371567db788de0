// ctc_ops.hip -- the tail of a CTC recognition head in one pass (pdf_table_amd/onnx_exec.py, ctc_tail=True; entry point added under ABI 19).
// A CTC decode (CTCLabelDecode: preds.argmax(axis=2), preds.max(axis=2)) needs ONE class id and ONE probability per token.  Layer by layer that is a
// soft-max that reads every 16-bit logit row three times and writes [rows, C] fp32 probabilities (softmax_rows_kernel), then a max / arg-max that reads
// them back: about 10 bytes per logit.  Here every logit is read once (2 bytes; 4 in the (hi | lo) mode) and 8 bytes per ROW are written:
//   id   = the lowest index of the largest of the first C logits (numpy's argmax rule: the first of equal values)
//   conf = that class's soft-max probability = 1 / sum_c exp(l_c - l_max), fp32
// One wave per row, four rows per workgroup.  Each lane keeps a running (max, index of its first occurrence, sum of exp(l - max)) over its own channels
// and rescales the sum when its maximum moves (online soft-max); the wave then agrees on (max, lowest index) with a butterfly that orders by value first
// and by the smaller index second, every lane rescales its sum to that maximum once, and the sums are added.
// Channels C .. Cp - 1 of a row are padding that may hold anything: they are never loaded.
#include "common.h"

namespace PT_FMT_NS {

namespace {

// lane-local state: m = the largest logit so far, idx = its first index, s = sum of exp(l - m) over the logits so far
struct CtcRun {
  float m, s;
  int idx;
};

// eight consecutive logits starting at channel c0: one comparison chain for the chunk's (max, first index), at most one rescale, eight exponentials
__device__ __forceinline__ void ctc_take8(CtcRun& r, const float* v, int c0) {
  float cm = v[0];
  int ci = 0;
#pragma unroll
  for (int q = 1; q < 8; ++q)
    if (v[q] > cm) { cm = v[q]; ci = q; }
  if (cm > r.m) {                    // strictly larger only: an equal value further right never takes the index
    r.s *= expf(r.m - cm);
    r.m = cm;
    r.idx = c0 + ci;
  }
  float a = 0.f;
#pragma unroll
  for (int q = 0; q < 8; ++q) a += expf(v[q] - r.m);
  r.s += a;
}

__device__ __forceinline__ void ctc_take1(CtcRun& r, float v, int c) {
  if (v > r.m) {
    r.s = r.s * expf(r.m - v) + 1.f;
    r.m = v;
    r.idx = c;
  } else {
    r.s += expf(v - r.m);
  }
}

__device__ __forceinline__ float ctc_ld(const bf16_t* p, int lo) { return lo ? a16_to_f32(p[0]) + a16_to_f32(p[lo]) : a16_to_f32(p[0]); }

// vec: rows are 16-byte aligned and Cp % 8 == 0 (the caller checked): lane l takes the 8-channel chunks l, l + 64, ... with one 16-byte load each (two in
// the pair mode); the chunk that straddles C, if any, is read channel by channel up to C.  Otherwise lane l takes channels l, l + 64, ... with 2-byte loads.
// Either way a lane's channels come in increasing order, so "strictly larger" keeps the first of equal values within a lane.
template <bool VEC>
__global__ __launch_bounds__(256) void ctc_greedy_kernel(const bf16_t* __restrict__ x, long long rows, int Cp, int C, int32_t* __restrict__ ids,
                                                         float* __restrict__ conf, int split) {
  a16_kernel_enter();
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, lo = split ? Cp : 0, cs = split ? 2 * Cp : Cp;
  if (row >= rows) return;           // whole waves leave: the shuffles below always see 64 live lanes
  const bf16_t* xr = x + row * cs;
  CtcRun r;
  r.m = -3.0e38f;                    // finite, below every storable logit: differences of maxima stay finite in lanes that saw no channel
  r.s = 0.f;
  r.idx = 0x7fffffff;
  if (VEC) {
    const int full = C >> 3;         // chunks that lie wholly below C
#pragma unroll 2
    for (int j = lane; j < full; j += 64) {
      float v[8];
      const uint4 h = *reinterpret_cast<const uint4*>(xr + j * 8);
      const uint32_t hw[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) { v[2 * k] = a16lo_f32(hw[k]); v[2 * k + 1] = a16hi_f32(hw[k]); }
      if (lo) {
        const uint4 l = *reinterpret_cast<const uint4*>(xr + lo + j * 8);
        const uint32_t lw[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[2 * k] += a16lo_f32(lw[k]); v[2 * k + 1] += a16hi_f32(lw[k]); }
      }
      ctc_take8(r, v, j * 8);
    }
    if ((C & 7) && lane == (full & 63))         // the straddling chunk belongs to the lane whose turn it is: its earlier chunks all lie to the left
      for (int c = full * 8; c < C; ++c) ctc_take1(r, ctc_ld(xr + c, lo), c);
  } else {
    for (int c = lane; c < C; c += 64) ctc_take1(r, ctc_ld(xr + c, lo), c);
  }
  // the wave's (max, lowest index of it): larger value first, smaller index among equal values
  float M = r.m;
  int I = r.idx;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(M, o);
    const int oi = __shfl_xor(I, o);
    if (om > M || (om == M && oi < I)) { M = om; I = oi; }
  }
  float s = r.s * expf(r.m - M);      // lanes without a channel: 0 * exp(0)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) {
    ids[row] = I;
    conf[row] = 1.f / s;
  }
}

}  // namespace

namespace api {

int pt_op_ctc_greedy(pt_engine* e, const uint16_t* d_in, long long rows, int c_pad, int c, int32_t* d_ids, float* d_conf, int split, pt_stream stream) {
  PT_REQUIRE(e && d_in && d_ids && d_conf && rows > 0 && rows <= (1ll << 32) && c > 0 && c <= c_pad, "pt_op_ctc_greedy: bad arguments (rows > 0, 0 < c <= c_pad)");
  const bool vec = c_pad % 8 == 0 && (reinterpret_cast<uintptr_t>(d_in) & 15) == 0;
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (vec) hipLaunchKernelGGL(ctc_greedy_kernel<true>, grid, block, 0, s, d_in, rows, c_pad, c, d_ids, d_conf, split ? 1 : 0);
  else hipLaunchKernelGGL(ctc_greedy_kernel<false>, grid, block, 0, s, d_in, rows, c_pad, c, d_ids, d_conf, split ? 1 : 0);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

}  // namespace api
}  // namespace PT_FMT_NS
