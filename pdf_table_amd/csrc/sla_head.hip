// sla_head.hip -- PaddleOCR's SLAHead (the table-structure head of SLANet: an attention-GRU cell walked T times, the arg-max of step t fed back as the
// one-hot input of step t + 1) as ONE launch: pt_op_sla_decode (entry points added under ABI 19).  Layer by layer the walk is about 15 launches per
// step; here a workgroup owns one table for all T steps and shares nothing with any other workgroup -- no flags, no spins, no grid barrier; the step
// loop is `for (t = 0; t < T; ++t)` and a table that has ended only writes zeros.
//
// The recurrence (SLAHead.forward in eval mode + AttentionGRUCell), fp32 throughout; only the weights and fea are 16-bit ((hi | lo) pairs when split):
//   once     P = fea W_i2h^T                                     [N, H]
//   step t   q = W_h2h h + b_h2h;  e_n = w_score . tanh(P_n + q);  alpha = softmax_n(e);  ctx = sum_n alpha_n fea_n
//            x = [ctx, onehot(p)];  r, z = sigma(W_i x + b_i + W_h h + b_h);  c = tanh(W_ic x + b_ic + r (W_hc h + b_hc));  h <- (h - c) z + c
//            s = W_s2 (W_s1 h + b_s1) + b_s2;  probs = softmax(s);  p <- lowest arg-max of s (or the forced id);  loc = sigma(W_l2 (W_l1 h + b_l1) + b_l2)
//
// What lives where (512 threads, 8 waves, one table):
//   * Every product is a mat-vec, so it runs on the VALU (fp32 FMAs, 16-byte weight loads, x broadcast out of LDS); there is no 16-row operand for an MFMA.
//   * The four products that read the same h -- W_h2h (next step's q), W_hr | W_hz | W_hc (next step's hidden gate sums), W_s1, W_l1 -- are ONE
//     [6H, H] mat-vec per step ("A" below); the packer stores it k-chunk-major [H / 8][6H][8], so thread r reads row r's eight values with one 16-byte
//     load and neighbouring threads read neighbouring 16 bytes.  No reduction across lanes.
//   * The weights (about 1 MB in 16 bits at the model's sizes, 2 MB as pairs) do not fit the 160 KB of LDS: they stream from L2 every step.
//   * P (fp32, N H 4 bytes = 256 KB at the model's sizes) lives in caller-provided scratch, written once and re-read every step from L2; it stays fp32
//     so that the pair mode keeps its accuracy.  fea (48 KB; 96 KB as pairs) is re-read from L2 as well.  LDS holds only the step's vectors.
//   * e_n: wave w takes tokens w, w + 8, ..; lane l the four units 4l .. 4l + 3 (one 16-byte load of P), then a wave reduction.
//   * Both soft-maxes subtract the maximum; the token soft-max is computed by every wave redundantly (four LDS reads per lane) instead of a barrier.
// hipcc (gfx950, -O3) reports for sla_decode_kernel: 24,360 bytes of LDS per workgroup and no scratch in every variant; VGPRs: 121 (bf16), 131 (f16),
// 106 (pairs).  A workgroup puts two waves on every SIMD, so up to 256 VGPRs would do: nothing here is bound by occupancy within the workgroup.
#include "common.h"

namespace PT_FMT_NS {

namespace {

constexpr int SLA_NT = 512;          // threads per workgroup
constexpr int SLA_NW = SLA_NT / 64;  // waves
constexpr int SLA_HMAX = 256, SLA_CMAX = 128, SLA_VMAX = 64, SLA_NMAX = 256, SLA_LMAX = 8;
constexpr int SLA_PB = 16;           // tokens staged per batch of the P product

struct SlaArgs {
  const bf16_t* fea;        // [B][N][cs], cs = c_pad (2 c_pad when split: [hi | lo])
  const bf16_t* w16;        // packed 16-bit image (weights.py::pack_sla_head); the lo image n16 values further when split
  const float* f32;         // packed fp32 vectors
  float* P;                 // scratch [B][N][H]
  const int32_t* force;     // [B][T] or null
  float* probs;             // [B][T][V]
  float* loc;               // [B][T][L]
  int32_t* ids;             // [B][T]
  int32_t* steps;           // [B]
  long long n16;
  int B, N, Cp, C, C8, H, V, L, T, eos;
};

// eight consecutive 16-bit values (16-byte aligned) as fp32; the pair mode adds the lo image's
template <bool SPLIT>
__device__ __forceinline__ void sla_ld8(const bf16_t* p, long long lo, float v[8]) {
  const uint4 h = *reinterpret_cast<const uint4*>(p);
  const uint32_t hw[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) { v[2 * k] = a16lo_f32(hw[k]); v[2 * k + 1] = a16hi_f32(hw[k]); }
  if (SPLIT) {
    const uint4 l = *reinterpret_cast<const uint4*>(p + lo);
    const uint32_t lw[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[2 * k] += a16lo_f32(lw[k]); v[2 * k + 1] += a16hi_f32(lw[k]); }
  }
}

// out[r] = bias[r] + sum_k W[r][k] x[k] for r < R; W packed [K8][R][8] (k-chunk-major), x fp32 in LDS (K8 * 8 values), out in LDS.
// Thread r owns row r: four partial sums (two k of every eight each), added pairwise at the end.
template <bool SPLIT>
__device__ __forceinline__ void sla_matvec(const bf16_t* W, long long lo, int R, int K8, const float* x, const float* bias, float* out) {
  for (int r = threadIdx.x; r < R; r += SLA_NT) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    const bf16_t* wp = W + (size_t)r * 8;
#pragma unroll 8
    for (int kc = 0; kc < K8; ++kc) {
      float v[8];
      sla_ld8<SPLIT>(wp + (size_t)kc * R * 8, lo, v);
      const float4 x0 = *reinterpret_cast<const float4*>(x + kc * 8), x1 = *reinterpret_cast<const float4*>(x + kc * 8 + 4);
      a0 = fmaf(v[0], x0.x, a0); a1 = fmaf(v[1], x0.y, a1); a2 = fmaf(v[2], x0.z, a2); a3 = fmaf(v[3], x0.w, a3);
      a0 = fmaf(v[4], x1.x, a0); a1 = fmaf(v[5], x1.y, a1); a2 = fmaf(v[6], x1.z, a2); a3 = fmaf(v[7], x1.w, a3);
    }
    out[r] = ((a0 + a1) + (a2 + a3)) + bias[r];
  }
}

__device__ __forceinline__ float sla_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float sla_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float sla_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

template <bool SPLIT>
__global__ __launch_bounds__(SLA_NT) void sla_decode_kernel(const SlaArgs a) {
  a16_kernel_enter();
  __shared__ __attribute__((aligned(16))) float s_h[SLA_HMAX];            // the hidden state
  __shared__ __attribute__((aligned(16))) float s_a[6 * SLA_HMAX];        // A's result: q | gh_r gh_z gh_c | s1 | l1
  __shared__ __attribute__((aligned(16))) float s_gi[3 * SLA_HMAX];       // W_i x + b_i
  __shared__ __attribute__((aligned(16))) float s_e[SLA_NMAX];            // attention scores
  __shared__ __attribute__((aligned(16))) float s_ctxp[SLA_NW][SLA_CMAX]; // per-wave partial contexts
  __shared__ __attribute__((aligned(16))) float s_ctx[SLA_CMAX];
  __shared__ __attribute__((aligned(16))) float s_x[SLA_PB][SLA_CMAX];    // staged fea rows of the P product
  __shared__ float s_sl[SLA_VMAX + SLA_LMAX];                             // logits | box pre-activations
  __shared__ int s_p, s_done;

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N, H = a.H, C = a.C, C8 = a.C8, Cp = a.Cp, V = a.V, L = a.L, T = a.T;
  const int cs = SPLIT ? 2 * Cp : Cp;
  const long long lo = SPLIT ? a.n16 : 0;
  const bf16_t* feab = a.fea + (size_t)b * N * cs;
  float* Pb = a.P + (size_t)b * N * H;
  // sections of the packed images (pt_op_sla_packed_elems / weights.py::pack_sla_head keep the same order)
  const bf16_t* WA = a.w16;
  const bf16_t* WI = WA + (size_t)6 * H * H;
  const bf16_t* WCOL = WI + (size_t)3 * H * C8;
  const bf16_t* WP = WCOL + (size_t)3 * H * V;
  const bf16_t* WS2 = WP + (size_t)H * C8;
  const bf16_t* WL2 = WS2 + (size_t)V * H;
  const float* bA = a.f32;
  const float* bI = bA + 6 * H;
  const float* wsc = bI + 3 * H;
  const float* bS2 = wsc + H;
  const float* bL2 = bS2 + SLA_VMAX;

  // ---- once: P = fea W_i2h^T.  SLA_PB tokens are staged as fp32 (channels >= C read as zero: the padding of a row may hold anything); thread group
  // g = tid / H takes tokens g, g + G, .. of the batch, thread tid % H one unit.
  {
    const int G = SLA_NT / H, g = tid / H, j = tid - g * H;
    for (int n0 = 0; n0 < N; n0 += SLA_PB) {
      for (int i = tid; i < SLA_PB * C8; i += SLA_NT) {
        const int nn = i / C8, c = i - nn * C8, n = n0 + nn;
        float v = 0.f;
        if (n < N && c < C) {
          const bf16_t* p = feab + (size_t)n * cs + c;
          v = a16_to_f32(p[0]);
          if (SPLIT) v += a16_to_f32(p[Cp]);
        }
        s_x[nn][c] = v;
      }
      __syncthreads();
      if (g < G) {
        for (int nn = g; nn < SLA_PB && n0 + nn < N; nn += G) {
          float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
          const float* x = s_x[nn];
          for (int kc = 0; kc < C8 / 8; ++kc) {
            float v[8];
            sla_ld8<SPLIT>(WP + ((size_t)kc * H + j) * 8, lo, v);
            a0 = fmaf(v[0], x[kc * 8 + 0], a0); a1 = fmaf(v[1], x[kc * 8 + 1], a1); a2 = fmaf(v[2], x[kc * 8 + 2], a2); a3 = fmaf(v[3], x[kc * 8 + 3], a3);
            a0 = fmaf(v[4], x[kc * 8 + 4], a0); a1 = fmaf(v[5], x[kc * 8 + 5], a1); a2 = fmaf(v[6], x[kc * 8 + 6], a2); a3 = fmaf(v[7], x[kc * 8 + 7], a3);
          }
          Pb[(size_t)(n0 + nn) * H + j] = (a0 + a1) + (a2 + a3);
        }
      }
      __syncthreads();
    }
  }
  if (tid < H) s_h[tid] = 0.f;
  if (tid == 0) { s_p = 0; s_done = 0; }
  __syncthreads();          // also orders this workgroup's writes of P before its reads below (same workgroup: the barrier makes them visible)
  sla_matvec<SPLIT>(WA, lo, 6 * H, H / 8, s_h, bA, s_a);      // h0 = 0: q and the hidden gate sums of step 0 (s1 / l1 of h0 are not used)
  __syncthreads();

  const int j4 = lane * 4;
  const bool unit_on = j4 < H;
  float4 wj = make_float4(0.f, 0.f, 0.f, 0.f);
  if (unit_on) wj = *reinterpret_cast<const float4*>(wsc + j4);

  int t = 0;
  for (; t < T; ++t) {
    if (s_done) break;      // uniform: s_done is written before a barrier every thread passes; the rows from t on are zero-filled below
    // ---- attention scores e_n = w_score . tanh(P_n + q)
    {
      float4 qj = make_float4(0.f, 0.f, 0.f, 0.f);
      if (unit_on) qj = *reinterpret_cast<const float4*>(s_a + j4);
      for (int n = wave; n < N; n += SLA_NW) {
        float acc = 0.f;
        if (unit_on) {
          const float4 p = *reinterpret_cast<const float4*>(Pb + (size_t)n * H + j4);
          acc = fmaf(wj.x, tanhf(p.x + qj.x), acc);
          acc = fmaf(wj.y, tanhf(p.y + qj.y), acc);
          acc = fmaf(wj.z, tanhf(p.z + qj.z), acc);
          acc = fmaf(wj.w, tanhf(p.w + qj.w), acc);
        }
        acc = sla_wave_sum(acc);
        if (lane == 0) s_e[n] = acc;
      }
    }
    __syncthreads();
    // ---- alpha = softmax_n(e) (every wave computes the maximum and the sum itself), ctx partials: wave w takes tokens 64 i + w, 64 i + w + 8, ..
    {
      float ex[4], m = -3.0e38f;
#pragma unroll
      for (int i = 0; i < 4; ++i) { const int n = lane + 64 * i; ex[i] = n < N ? s_e[n] : -3.0e38f; m = fmaxf(m, ex[i]); }
      m = sla_wave_max(m);
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) { const int n = lane + 64 * i; ex[i] = n < N ? expf(ex[i] - m) : 0.f; s += ex[i]; }
      s = sla_wave_sum(s);
      const float inv = 1.f / s;
      float c0 = 0.f, c1 = 0.f;
      const bool pair_on = lane < Cp / 2;
      const uint32_t* f32p = reinterpret_cast<const uint32_t*>(feab);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        for (int l = wave; l < 64; l += SLA_NW) {
          const int n = 64 * i + l;
          if (n >= N) break;
          const float al = __shfl(ex[i], l) * inv;
          if (pair_on) {
            const uint32_t d = f32p[(size_t)n * (cs / 2) + lane];
            float v0 = a16lo_f32(d), v1 = a16hi_f32(d);
            if (SPLIT) {
              const uint32_t d2 = f32p[(size_t)n * (cs / 2) + Cp / 2 + lane];
              v0 += a16lo_f32(d2); v1 += a16hi_f32(d2);
            }
            c0 = fmaf(al, v0, c0); c1 = fmaf(al, v1, c1);
          }
        }
      }
      if (pair_on) { s_ctxp[wave][2 * lane] = c0; s_ctxp[wave][2 * lane + 1] = c1; }
    }
    __syncthreads();
    if (tid < C8) {
      float v = 0.f;
      if (tid < C) {
#pragma unroll
        for (int w = 0; w < SLA_NW; ++w) v += s_ctxp[w][tid];
      }
      s_ctx[tid] = v;       // channels C .. C8 - 1 meet zero weights; they are zero here too, whatever the row's padding holds
    }
    __syncthreads();
    // ---- input gate sums: W_i[:, :C] ctx + b_i, plus the one-hot part as a column read of W_i[:, C + p]
    sla_matvec<SPLIT>(WI, lo, 3 * H, C8 / 8, s_ctx, bI, s_gi);
    {
      const int p = s_p;
      for (int r = tid; r < 3 * H; r += SLA_NT) {       // the rows this thread wrote itself in sla_matvec
        const bf16_t* wc = WCOL + (size_t)p * 3 * H + r;
        float v = a16_to_f32(wc[0]);
        if (SPLIT) v += a16_to_f32(wc[lo]);
        s_gi[r] += v;
      }
    }
    __syncthreads();
    // ---- GRU cell, gates r, z, c
    if (tid < H) {
      const float r = sla_sigmoid(s_gi[tid] + s_a[H + tid]);
      const float z = sla_sigmoid(s_gi[H + tid] + s_a[2 * H + tid]);
      const float c = tanhf(s_gi[2 * H + tid] + r * s_a[3 * H + tid]);
      s_h[tid] = (s_h[tid] - c) * z + c;
    }
    __syncthreads();
    // ---- A: everything that reads the new h
    sla_matvec<SPLIT>(WA, lo, 6 * H, H / 8, s_h, bA, s_a);
    __syncthreads();
    // ---- generators' second layers: wave per output row, lane l the units 4l .. 4l + 3
    for (int v = wave; v < V + L; v += SLA_NW) {
      const bool is_s = v < V;
      const bf16_t* wr = is_s ? WS2 + (size_t)v * H : WL2 + (size_t)(v - V) * H;
      const float* x = s_a + (is_s ? 4 : 5) * H;
      float acc = 0.f;
      if (unit_on) {
        const uint2 d = *reinterpret_cast<const uint2*>(wr + j4);
        float w0 = a16lo_f32(d.x), w1 = a16hi_f32(d.x), w2 = a16lo_f32(d.y), w3 = a16hi_f32(d.y);
        if (SPLIT) {
          const uint2 d2 = *reinterpret_cast<const uint2*>(wr + lo + j4);
          w0 += a16lo_f32(d2.x); w1 += a16hi_f32(d2.x); w2 += a16lo_f32(d2.y); w3 += a16hi_f32(d2.y);
        }
        const float4 xv = *reinterpret_cast<const float4*>(x + j4);
        acc = fmaf(w0, xv.x, acc); acc = fmaf(w1, xv.y, acc); acc = fmaf(w2, xv.z, acc); acc = fmaf(w3, xv.w, acc);
      }
      acc = sla_wave_sum(acc);
      if (lane == 0) s_sl[is_s ? v : SLA_VMAX + (v - V)] = acc + (is_s ? bS2[v] : bL2[v - V]);
    }
    __syncthreads();
    const size_t row = (size_t)b * T + t;
    if (wave == 0) {
      // soft-max over the V classes and the lowest index of the largest logit: larger value first, smaller index among equal values
      const float sv = lane < V ? s_sl[lane] : -3.0e38f;
      float M = sv;
      int I = lane < V ? lane : 0x7fffffff;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(M, o);
        const int oi = __shfl_xor(I, o);
        if (om > M || (om == M && oi < I)) { M = om; I = oi; }
      }
      const float ev = lane < V ? expf(sv - M) : 0.f;
      const float sum = sla_wave_sum(ev);
      if (lane < V) a.probs[row * V + lane] = ev / sum;
      if (lane == 0) {
        a.ids[row] = I;
        int pn = a.force ? a.force[row] : I;
        pn = pn < 0 ? 0 : (pn >= V ? V - 1 : pn);       // a forced id outside [0, V) is the caller's error; it never becomes an address
        s_p = pn;
        if (a.eos >= 0 && t > 0 && I == a.eos) s_done = 1;
      }
    } else if (wave == 1) {
      if (lane < L) a.loc[row * L + lane] = sla_sigmoid(s_sl[SLA_VMAX + lane]);
    }
    __syncthreads();
  }
  // t = rows written.  After a stop, zeros in the rows that were not walked
  for (long long i = (long long)t * V + tid; i < (long long)T * V; i += SLA_NT) a.probs[(size_t)b * T * V + i] = 0.f;
  for (long long i = (long long)t * L + tid; i < (long long)T * L; i += SLA_NT) a.loc[(size_t)b * T * L + i] = 0.f;
  for (long long i = (long long)t + tid; i < (long long)T; i += SLA_NT) a.ids[(size_t)b * T + i] = 0;
  if (tid == 0) a.steps[b] = t;
}

// ---- SLANetPreprocessor on resident pages (model/slanet/processor_slanet.py: ResizeTableImage, NormalizeImage, PaddingTableImage) -------------------
// Per table: the integer crop read as BGR, ratio = size / max(h, w) in double, cv2.resize (8-bit bilinear: the fixed-point arithmetic of
// rec_kernels.hip / det_kernels.hip, with OpenCV's two short cuts: same size = copy, exactly half = 2x2 mean) to (int(w ratio), int(h ratio)),
// (v * (1 / 255) - mean[c]) / std[c] in fp32 with mean / std indexed in that BGR order (a 3 x 256 table per workgroup, the reference's operation
// order), zeros right of and below the resized crop.  out: fp32 NHWC [n, size, size, 3], channel order B, G, R.
struct SlaCoef {
  int s0, s1, a0, a1;
};
__device__ __forceinline__ SlaCoef sla_coef(int d, double scale, int ssize, bool clamp_frac) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (clamp_frac) {
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
  }
  SlaCoef c;
  c.a0 = (int)rintf((1.f - f) * 2048.f);
  c.a1 = (int)rintf(f * 2048.f);
  const int t0 = s, t1 = s + 1;
  c.s0 = t0 < 0 ? 0 : (t0 >= ssize ? ssize - 1 : t0);
  c.s1 = t1 < 0 ? 0 : (t1 >= ssize ? ssize - 1 : t1);
  return c;
}

__global__ __launch_bounds__(256) void sla_preprocess_kernel(const uint8_t* __restrict__ pages, int ph, int pw, const pt_tsr_table* __restrict__ tabs,
                                                             int size, float* __restrict__ out) {
  a16_kernel_enter();
  __shared__ float lut[3][256];
  {
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    const float scale = 1.0f / 255.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) lut[c][threadIdx.x] = ((float)threadIdx.x * scale - mean[c]) / stdv[c];
  }
  __syncthreads();
  const pt_tsr_table tb = tabs[blockIdx.y];
  const int cw = tb.crop_w, ch = tb.crop_h;
  const double ratio = (double)size / ((double)(ch > cw ? ch : cw) * 1.0);
  const int nh = (int)((double)ch * ratio), nw = (int)((double)cw * ratio);
  const uint8_t* src = pages + ((size_t)tb.page * ph + tb.y0) * (size_t)pw * 3 + (size_t)tb.x0 * 3;      // rows pw * 3 bytes apart
  const size_t rs = (size_t)pw * 3;
  float* o = out + (size_t)blockIdx.y * size * size * 3;
  const bool same = cw == nw && ch == nh, half = cw == 2 * nw && ch == 2 * nh;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < size * size; i += gridDim.x * blockDim.x) {
    const int x = i % size, y = i / size;
    float r[3] = {0.f, 0.f, 0.f};
    if (x < nw && y < nh) {
      int v[3];      // R, G, B as stored
      if (same) {
        const uint8_t* p = src + y * rs + (size_t)x * 3;
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
      } else if (half) {
        const uint8_t* p0 = src + (size_t)(2 * y) * rs + (size_t)(2 * x) * 3;
        const uint8_t* p1 = p0 + rs;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (p0[c] + p0[3 + c] + p1[c] + p1[3 + c] + 2) >> 2;
      } else {
        const SlaCoef cx = sla_coef(x, (double)cw / nw, cw, true);
        const SlaCoef cy = sla_coef(y, (double)ch / nh, ch, false);
        const uint8_t* r0 = src + (size_t)cy.s0 * rs;
        const uint8_t* r1 = src + (size_t)cy.s1 * rs;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int S0 = r0[cx.s0 * 3 + c] * cx.a0 + r0[cx.s1 * 3 + c] * cx.a1;
          const int S1 = r1[cx.s0 * 3 + c] * cx.a0 + r1[cx.s1 * 3 + c] * cx.a1;
          const int q = (((cy.a0 * (S0 >> 4)) >> 16) + ((cy.a1 * (S1 >> 4)) >> 16) + 2) >> 2;
          v[c] = q < 0 ? 0 : (q > 255 ? 255 : q);
        }
      }
      r[0] = lut[0][v[2]]; r[1] = lut[1][v[1]]; r[2] = lut[2][v[0]];      // channel 0 of the BGR image is B and takes mean[0] / std[0]
    }
    o[(size_t)i * 3] = r[0]; o[(size_t)i * 3 + 1] = r[1]; o[(size_t)i * 3 + 2] = r[2];
  }
}

// the built range; message in pt_last_error otherwise
int sla_check_dims(const char* who, int H, int C, int V, int L) {
  PT_REQUIRE(H >= 32 && H <= SLA_HMAX && H % 32 == 0, "%s: hidden size %d: a multiple of 32 up to %d is built", who, H, SLA_HMAX);
  PT_REQUIRE(C >= 1 && C <= SLA_CMAX, "%s: %d feature channels: 1 .. %d are built", who, C, SLA_CMAX);
  PT_REQUIRE(V >= 1 && V <= SLA_VMAX, "%s: %d classes: 1 .. %d are built", who, V, SLA_VMAX);
  PT_REQUIRE(L == 4 || L == 8, "%s: %d box values: 4 or 8 are built", who, L);
  return PT_OK;
}

}  // namespace

namespace api {

int pt_op_sla_packed_elems(int H, int C, int V, int L, long long* n16, long long* n32) {
  if (int rc = sla_check_dims("pt_op_sla_packed_elems", H, C, V, L)) return rc;
  PT_REQUIRE(n16 && n32, "pt_op_sla_packed_elems: null pointer");
  const long long C8 = (C + 7) / 8 * 8;
  *n16 = 6ll * H * H + 3ll * H * C8 + 3ll * H * V + (long long)H * C8 + (long long)V * H + (long long)L * H;
  *n32 = 10ll * H + SLA_VMAX + SLA_LMAX;
  return PT_OK;
}

int pt_op_sla_scratch_bytes(int B, int N, int H, long long* bytes) {
  PT_REQUIRE(bytes && B >= 1 && N >= 1 && N <= SLA_NMAX && H >= 32 && H <= SLA_HMAX && H % 32 == 0,
             "pt_op_sla_scratch_bytes: B=%d N=%d H=%d: B >= 1, 1 <= N <= %d, H a multiple of 32 up to %d", B, N, H, SLA_NMAX, SLA_HMAX);
  *bytes = (long long)B * N * H * 4;
  return PT_OK;
}

int pt_op_sla_decode(pt_engine* e, const uint16_t* d_fea, int B, int N, int c_pad, int C, int H, int V, int L, int T, const uint16_t* d_w16,
                     const float* d_f32, void* d_scratch, long long scratch_bytes, int eos_id, const int32_t* d_force_ids, float* d_probs, float* d_loc,
                     int32_t* d_ids, int32_t* d_steps, int split, pt_stream stream) {
  PT_REQUIRE(e && d_fea && d_w16 && d_f32 && d_scratch && d_probs && d_loc && d_ids && d_steps, "pt_op_sla_decode: null pointer");
  if (int rc = sla_check_dims("pt_op_sla_decode", H, C, V, L)) return rc;
  PT_REQUIRE(N >= 1 && N <= SLA_NMAX, "pt_op_sla_decode: %d tokens: 1 .. %d are built", N, SLA_NMAX);
  PT_REQUIRE(B >= 1 && T >= 1, "pt_op_sla_decode: B=%d T=%d: both must be at least 1", B, T);
  PT_REQUIRE(c_pad % 8 == 0 && c_pad >= C && c_pad <= SLA_CMAX, "pt_op_sla_decode: token rows of %d channels for C=%d: a multiple of 8, C .. %d", c_pad, C, SLA_CMAX);
  PT_REQUIRE(eos_id < V, "pt_op_sla_decode: eos_id %d with %d classes", eos_id, V);
  PT_REQUIRE((long long)B * T * (V > L ? V : L) < (1ll << 40), "pt_op_sla_decode: outputs too large");
  PT_REQUIRE(scratch_bytes >= (long long)B * N * H * 4, "pt_op_sla_decode: %lld bytes of scratch, %lld are needed (pt_op_sla_scratch_bytes)", scratch_bytes,
             (long long)B * N * H * 4);
  PT_REQUIRE(((uintptr_t)d_fea & 15) == 0 && ((uintptr_t)d_w16 & 15) == 0 && ((uintptr_t)d_f32 & 15) == 0 && ((uintptr_t)d_scratch & 15) == 0,
             "pt_op_sla_decode: unaligned pointer (16 bytes)");
  SlaArgs a;
  a.fea = d_fea; a.w16 = d_w16; a.f32 = d_f32; a.P = static_cast<float*>(d_scratch); a.force = d_force_ids;
  a.probs = d_probs; a.loc = d_loc; a.ids = d_ids; a.steps = d_steps;
  a.B = B; a.N = N; a.Cp = c_pad; a.C = C; a.C8 = (C + 7) / 8 * 8; a.H = H; a.V = V; a.L = L; a.T = T; a.eos = eos_id;
  long long n32 = 0;
  if (int rc = pt_op_sla_packed_elems(H, C, V, L, &a.n16, &n32)) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (split) hipLaunchKernelGGL(sla_decode_kernel<true>, dim3((unsigned)B), dim3(SLA_NT), 0, s, a);
  else hipLaunchKernelGGL(sla_decode_kernel<false>, dim3((unsigned)B), dim3(SLA_NT), 0, s, a);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

int pt_slanet_preprocess(pt_engine* e, const uint8_t* d_pages_rgb, int n_pages, int ph, int pw, const pt_tsr_table* d_tables, const pt_tsr_table* h_tables,
                         int n, int size, float* d_out, pt_stream stream) {
  PT_REQUIRE(e && d_pages_rgb && d_tables && h_tables && d_out && n >= 1 && n_pages >= 1 && ph >= 1 && pw >= 1, "pt_slanet_preprocess: bad arguments");
  PT_REQUIRE(size >= 32 && size <= 4096, "pt_slanet_preprocess: network input side %d: 32 .. 4096", size);
  for (int i = 0; i < n; ++i) {      // the crops are read as they are given: every one must lie on its page
    const pt_tsr_table& t = h_tables[i];
    PT_REQUIRE(t.page >= 0 && t.page < n_pages && t.crop_w >= 1 && t.crop_h >= 1 && t.x0 >= 0 && t.y0 >= 0 && t.x0 + t.crop_w <= pw && t.y0 + t.crop_h <= ph,
               "pt_slanet_preprocess: table %d (page %d, x0 %d, y0 %d, %d x %d) does not lie on a %d x %d page of %d", i, t.page, t.x0, t.y0, t.crop_w,
               t.crop_h, pw, ph, n_pages);
    const int lo = t.crop_w < t.crop_h ? t.crop_w : t.crop_h, hi = t.crop_w < t.crop_h ? t.crop_h : t.crop_w;
    PT_REQUIRE((long long)lo * size >= hi, "pt_slanet_preprocess: table %d of %d x %d pixels has no row or column left at a side of %d", i, t.crop_w, t.crop_h, size);
  }
  int bx = (size * size + 255) / 256;
  bx = bx > 128 ? 128 : bx;
  hipLaunchKernelGGL(sla_preprocess_kernel, dim3(bx, n), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), d_pages_rgb, ph, pw, d_tables, size, d_out);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

}  // namespace api
}  // namespace PT_FMT_NS
