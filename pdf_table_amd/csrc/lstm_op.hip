// lstm_op.hip -- the recurrence of an ONNX LSTM layer for the generic layer-list executor (pdf_table_amd/onnx_exec.py): narrow LSTMs
// (hidden size <= 128) of CRNN-type recognisers such as the PP-OCR mobile / table recognisers, and any nn.LSTM a user exports.
//
// Split of the work: the input projection X W^T + (Wb + Rb) of all T steps and both directions is ONE call of the row GEMM (pt_op_conv2d,
// 4 Hp D output channels); this file does h_{t-1} R^T, the gate arithmetic and the state update.
//
// Ownership: one workgroup (4 waves) owns one direction and one tile of 16 sequences for all T steps.  Nothing is shared between
// workgroups: no cross-workgroup synchronisation, no spin-wait, no co-residency assumption, no device time-out -- a step is synchronised
// by ONE workgroup barrier (h is double-buffered in LDS).  (The engine's own 256-unit kernels in rec_kernels.hip split a direction over
// co-resident workgroups because their R does not fit one CU; here it does.)
//
// Sizes: Hp = H rounded up to 16 (<= 128), Kp = Hp rounded up to 32 (the K of the 16x16x32 MFMA).  Padded units have zero R rows / columns,
// zero W rows and zero bias, so their gates are 0, c stays 0 and h = sigmoid(0) tanh(0) stays exactly 0.
//
// R in LDS: packed on the host (pdf_table_amd/weights.py::pack_lstm_r) in MFMA operand order -- fragment f = (ub * 4 + gate) * KS + kk
// (ub: block of 16 units, gate in ONNX order i, o, f, c, kk: K step of 32) holds for lane l the 8 values
// R[gate * H + ub * 16 + (l & 15)][kk * 32 + 8 (l >> 4) + j]: the A operand of v_mfma_f32_16x16x32 (rows = units, k = previous h).  A
// fragment is 1 KiB read by 64 lanes at consecutive 16-byte addresses (conflict-free ds_read_b128); the whole R is 4 (Hp / 16) (Kp / 32) KiB:
// 128 KiB at Hp = 128, loaded once.  The B operand is h_{t-1}: lane l reads h[sequence l & 15][kk * 32 + 8 (l >> 4) ..] from an LDS image
// whose rows are padded by 16 bytes.  D: column (l & 15) = sequence, rows 4 (l >> 4) + r = four consecutive units -- so a lane reads its
// pre-gates, writes h to LDS and Y to HBM 8 bytes at a time, and holds i, o, f, c of the same (sequence, unit) in the same register slot.
//
// A step: acc = pre-gates (fp32, as the C input) -> KS MFMAs per gate and unit block -> i, o, f = sigmoid, g = tanh -> c = f c + i g (fp32
// registers for the whole sequence) -> h = o tanh(c), rounded ONCE to the storage format, written to Y and to the other h buffer -> barrier.
// The R fragments of the next gate are read while the current gate's MFMAs run, and the pre-gates of step t + 1 are loaded during step t, so
// no MFMA waits on a read issued just before it.
//
// MODE 1 / 2 (the tolerance mode, BF16X3): pre-gates, h and R are (hi | lo) pairs; three passes R_hi h_hi + R_hi h_lo + R_lo h_hi.  MODE 1
// keeps both halves of R in LDS (Hp <= 96); MODE 2 (Hp 112, 128: 2 x 112 KiB does not fit) keeps R_hi in LDS and streams the R_lo fragments
// from L2 each step -- the packed order makes that a fully coalesced 1 KiB read per fragment.
#include "common.h"

namespace PT_FMT_NS {

namespace {

constexpr int LSTM_NW = 4;          // waves per workgroup: one per SIMD
constexpr int LSTM_SEQ = 16;        // sequences per workgroup (the N of the MFMA)

__device__ __forceinline__ float lstm_sigmoid(float x) { return __fdividef(1.f, 1.f + __expf(-x)); }
__device__ __forceinline__ float lstm_tanh(float x) { return 1.f - __fdividef(2.f, 1.f + __expf(2.f * x)); }

__host__ __device__ constexpr int lstm_h_stride(int KS) { return KS * 32 + 8; }        // elements per h row in LDS (16 bytes of padding)

// pg: pre-gates [B T rows][pg_cs] (row b T + t; channel d 4 Hp + gate Hp + unit; lo half pg_lo further when MODE), rp: packed R of every direction,
// y: [B T rows][y_cs] (channel d H + unit; lo half y_lo further when MODE)
template <int KS, int MODE>
__global__ __launch_bounds__(LSTM_NW * 64) void lstm_narrow_kernel(const bf16_t* __restrict__ pg, int pg_cs, int pg_lo, const uint4* __restrict__ rp, int T, int B,
                                                                   int H, int Hp, int dirs, int reverse, bf16_t* __restrict__ y, int y_cs, int y_lo) {
  a16_kernel_enter();
  constexpr int NUW = KS > 2 ? 2 : 1;            // unit blocks per wave (Hp <= 64: one, else two)
  constexpr int NH = MODE ? 2 : 1;               // halves of h and of the pre-gates
  constexpr int HS = lstm_h_stride(KS);
  extern __shared__ __attribute__((aligned(16))) char lsm[];
  const int NU = Hp >> 4;
  const int nfrag = NU * 4 * KS;                 // fragments of one half of R
  uint4* r_hi = reinterpret_cast<uint4*>(lsm);
  uint4* r_lo = r_hi + (MODE == 1 ? nfrag * 64 : 0);
  bf16_t* hbuf = reinterpret_cast<bf16_t*>(r_hi + (MODE == 1 ? 2 : 1) * nfrag * 64);      // [2 buffers][NH][16][HS]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d = blockIdx.y, b0 = blockIdx.x * LSTM_SEQ;
  const bool rev = dirs == 2 ? d == 1 : reverse != 0;
  const uint4* rsrc = rp + (size_t)d * (MODE ? 2 : 1) * nfrag * 64;
  for (int i = tid; i < (MODE == 1 ? 2 : 1) * nfrag * 64; i += LSTM_NW * 64) r_hi[i] = rsrc[i];
  const uint4* r_lo_g = rsrc + nfrag * 64;       // MODE 2: the lo fragments stay in global memory
  for (int i = tid; i < 2 * NH * LSTM_SEQ * HS / 2; i += LSTM_NW * 64) reinterpret_cast<uint32_t*>(hbuf)[i] = 0u;      // h_0 = 0; the K padding stays 0
  __syncthreads();

  const int s = lane & 15, q4 = lane >> 4;
  const int b = b0 + s;
  const bool live = b < B;
  const bool y_vec = (H & 3) == 0 && (y_cs & 3) == 0 && (y_lo & 3) == 0;
  bool act_u[NUW];
  int unit0[NUW];                                 // first of this lane's four units
#pragma unroll
  for (int u = 0; u < NUW; ++u) {
    act_u[u] = wave + LSTM_NW * u < NU;           // wave-uniform
    unit0[u] = (wave + LSTM_NW * u) * 16 + 4 * q4;
  }
  float c[NUW][4];
#pragma unroll
  for (int u = 0; u < NUW; ++u)
#pragma unroll
    for (int r = 0; r < 4; ++r) c[u][r] = 0.f;

  // pre-gates of one step: [unit block][gate][half] 4 values each
  uint2 pgn[NUW][4][NH];
  auto load_pg = [&](int t) {
    const bf16_t* row = pg + ((size_t)b * T + t) * pg_cs + (size_t)d * 4 * Hp;
#pragma unroll
    for (int u = 0; u < NUW; ++u)
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int h = 0; h < NH; ++h)
          pgn[u][g][h] = (live && act_u[u]) ? *reinterpret_cast<const uint2*>(row + h * pg_lo + g * Hp + unit0[u]) : make_uint2(0u, 0u);
  };
  load_pg(rev ? T - 1 : 0);

  for (int step = 0; step < T; ++step) {
    const int t = rev ? T - 1 - step : step;
    const bf16_t* hc = hbuf + (step & 1) * NH * LSTM_SEQ * HS;
    bf16_t* hn = hbuf + ((step + 1) & 1) * NH * LSTM_SEQ * HS;
    a16_f32x4 acc[NUW][4];
#pragma unroll
    for (int u = 0; u < NUW; ++u)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const uint2 p = pgn[u][g][0];
        acc[u][g] = a16_f32x4{a16lo_f32(p.x), a16hi_f32(p.x), a16lo_f32(p.y), a16hi_f32(p.y)};
        if (MODE) {
          const uint2 q = pgn[u][g][NH - 1];
          acc[u][g] += a16_f32x4{a16lo_f32(q.x), a16hi_f32(q.x), a16lo_f32(q.y), a16hi_f32(q.y)};
        }
      }
    if (step + 1 < T) load_pg(rev ? t - 1 : t + 1);         // in flight during this step's MFMAs
    // B operand: h_{t-1} of the 16 sequences
    a16_bf16x8 hb[NH][KS];
#pragma unroll
    for (int h = 0; h < NH; ++h)
#pragma unroll
      for (int kk = 0; kk < KS; ++kk)
        hb[h][kk] = *reinterpret_cast<const a16_bf16x8*>(hc + (h * LSTM_SEQ + s) * HS + kk * 32 + 8 * q4);
#pragma unroll
    for (int u = 0; u < NUW; ++u) {
      if (!act_u[u]) continue;
      const int f0 = (wave + LSTM_NW * u) * 4 * KS;
      a16_bf16x8 ra[2][KS], rl[2][KS];
      auto load_r = [&](int g, int slot) {
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
          const int f = (f0 + g * KS + kk) * 64 + lane;
          ra[slot][kk] = __builtin_bit_cast(a16_bf16x8, r_hi[f]);
          if (MODE == 1) rl[slot][kk] = __builtin_bit_cast(a16_bf16x8, r_lo[f]);
          if (MODE == 2) rl[slot][kk] = __builtin_bit_cast(a16_bf16x8, r_lo_g[f]);
        }
      };
      load_r(0, 0);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        if (g + 1 < 4) load_r(g + 1, (g + 1) & 1);          // the next gate's fragments are read under this gate's MFMAs
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
          acc[u][g] = mfma_16x16x32_a16(ra[g & 1][kk], hb[0][kk], acc[u][g]);
          if (MODE) {
            acc[u][g] = mfma_16x16x32_a16(ra[g & 1][kk], hb[NH - 1][kk], acc[u][g]);
            acc[u][g] = mfma_16x16x32_a16(rl[g & 1][kk], hb[0][kk], acc[u][g]);
          }
        }
      }
      // gates in ONNX order i, o, f, c
      float hv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float ig = lstm_sigmoid(acc[u][0][r]), og = lstm_sigmoid(acc[u][1][r]), fg = lstm_sigmoid(acc[u][2][r]), gg = lstm_tanh(acc[u][3][r]);
        c[u][r] = fg * c[u][r] + ig * gg;
        hv[r] = og * lstm_tanh(c[u][r]);
      }
      uint2 hi = make_uint2(pack_a16x2(hv[0], hv[1]), pack_a16x2(hv[2], hv[3])), lo = make_uint2(0u, 0u);
      if (MODE) {
        lo = make_uint2(pack_a16x2(hv[0] - a16lo_f32(hi.x), hv[1] - a16hi_f32(hi.x)), pack_a16x2(hv[2] - a16lo_f32(hi.y), hv[3] - a16hi_f32(hi.y)));
        *reinterpret_cast<uint2*>(hn + (LSTM_SEQ + s) * HS + unit0[u]) = lo;
      }
      *reinterpret_cast<uint2*>(hn + s * HS + unit0[u]) = hi;
      if (live) {
        bf16_t* yr = y + ((size_t)b * T + t) * y_cs + (size_t)d * H + unit0[u];
        if (y_vec && unit0[u] + 4 <= H) {
          *reinterpret_cast<uint2*>(yr) = hi;
          if (MODE) *reinterpret_cast<uint2*>(yr + y_lo) = lo;
        } else {
          const uint32_t hw[2] = {hi.x, hi.y}, lw[2] = {lo.x, lo.y};
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (unit0[u] + r < H) {
              yr[r] = (bf16_t)((hw[r >> 1] >> (16 * (r & 1))) & 0xFFFFu);
              if (MODE) yr[y_lo + r] = (bf16_t)((lw[r >> 1] >> (16 * (r & 1))) & 0xFFFFu);
            }
        }
      }
    }
    __syncthreads();
  }
}

inline size_t lstm_smem(int Hp, int KS, int mode) {
  const size_t rbytes = (size_t)(Hp / 16) * 4 * KS * 1024;
  return (mode == 1 ? 2 : 1) * rbytes + (size_t)2 * (mode ? 2 : 1) * LSTM_SEQ * lstm_h_stride(KS) * 2;
}

template <int KS, int MODE>
int launch_lstm_narrow(const bf16_t* pg, int pg_cs, int pg_lo, const uint4* rp, int T, int B, int H, int Hp, int dirs, int reverse, bf16_t* y, int y_cs,
                       int y_lo, hipStream_t s) {
  static int attr_for = 0;                       // the largest dynamic LDS size this instantiation has been allowed
  const int smem = (int)lstm_smem(Hp, KS, MODE);
  if (smem > attr_for) {
    PT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&lstm_narrow_kernel<KS, MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    attr_for = smem;
  }
  hipLaunchKernelGGL((lstm_narrow_kernel<KS, MODE>), dim3((B + LSTM_SEQ - 1) / LSTM_SEQ, dirs), dim3(LSTM_NW * 64), smem, s, pg, pg_cs, pg_lo, rp, T, B, H, Hp,
                     dirs, reverse, y, y_cs, y_lo);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

template <int MODE>
int launch_lstm_mode(int KS, const bf16_t* pg, int pg_cs, int pg_lo, const uint4* rp, int T, int B, int H, int Hp, int dirs, int reverse, bf16_t* y, int y_cs,
                     int y_lo, hipStream_t s) {
  switch (KS) {
    case 1: return launch_lstm_narrow<1, MODE>(pg, pg_cs, pg_lo, rp, T, B, H, Hp, dirs, reverse, y, y_cs, y_lo, s);
    case 2: return launch_lstm_narrow<2, MODE>(pg, pg_cs, pg_lo, rp, T, B, H, Hp, dirs, reverse, y, y_cs, y_lo, s);
    case 3: return launch_lstm_narrow<3, MODE>(pg, pg_cs, pg_lo, rp, T, B, H, Hp, dirs, reverse, y, y_cs, y_lo, s);
    default: return launch_lstm_narrow<4, MODE>(pg, pg_cs, pg_lo, rp, T, B, H, Hp, dirs, reverse, y, y_cs, y_lo, s);
  }
}

}  // namespace

namespace api {

int pt_op_lstm_packed_elems(int H, int dirs, int split) {
  if (H <= 0 || H > 128 || dirs < 1 || dirs > 2) return 0;
  const int Hp = (H + 15) / 16 * 16, KS = (Hp + 31) / 32;
  return dirs * (split ? 2 : 1) * (Hp / 16) * 4 * KS * 512;
}

int pt_op_lstm(pt_engine* e, const uint16_t* d_pregates, int pg_cstride, const uint16_t* d_r_packed, int T, int B, int H, int dirs, int reverse,
               uint16_t* d_y, int y_cstride, int split, pt_stream stream) {
  PT_REQUIRE(e && d_pregates && d_r_packed && d_y, "pt_op_lstm: null pointer");
  PT_REQUIRE(T > 0 && B > 0 && (dirs == 1 || dirs == 2), "pt_op_lstm: T=%d B=%d dirs=%d unsupported", T, B, dirs);
  PT_REQUIRE(H > 0 && H <= 128, "pt_op_lstm: hidden size %d: this kernel keeps the recurrent weights of one direction in LDS, 128 units at the most", H);
  const int Hp = (H + 15) / 16 * 16, KS = (Hp + 31) / 32, m = split ? 2 : 1;
  PT_REQUIRE(pg_cstride % (4 * m) == 0 && pg_cstride >= m * dirs * 4 * Hp, "pt_op_lstm: pre-gate rows of %d channels, %d x %d x 4 x %d are needed", pg_cstride, m,
             dirs, Hp);
  PT_REQUIRE(y_cstride % m == 0 && y_cstride >= m * dirs * H, "pt_op_lstm: output rows of %d channels, %d x %d x %d are needed", y_cstride, m, dirs, H);
  PT_REQUIRE(((uintptr_t)d_pregates & 7) == 0 && ((uintptr_t)d_r_packed & 15) == 0 && ((uintptr_t)d_y & 7) == 0, "pt_op_lstm: unaligned pointer");
  PT_REQUIRE((long long)B * T * (long long)(pg_cstride > y_cstride ? pg_cstride : y_cstride) < (1ll << 40), "pt_op_lstm: tensor too large");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint4* rp = reinterpret_cast<const uint4*>(d_r_packed);
  if (!split) return launch_lstm_mode<0>(KS, d_pregates, pg_cstride, 0, rp, T, B, H, Hp, dirs, reverse, d_y, y_cstride, 0, s);
  if (Hp <= 96) return launch_lstm_mode<1>(KS, d_pregates, pg_cstride, pg_cstride / 2, rp, T, B, H, Hp, dirs, reverse, d_y, y_cstride, y_cstride / 2, s);
  return launch_lstm_mode<2>(KS, d_pregates, pg_cstride, pg_cstride / 2, rp, T, B, H, Hp, dirs, reverse, d_y, y_cstride, y_cstride / 2, s);
}

}  // namespace api
}  // namespace PT_FMT_NS
