// lore_processor.hip -- Lore's logical-location processor (two 4-layer pre-norm transformer regressors) for a batch
// of tables in one pass.
//
// Reference: LoreProcessModel.forward lore/lore_processor.py:465-514 (evaluation branch): Transformer :81-114 =
// Linear -> L x EncoderLayer :286-313 (x += MHA(Norm(x)); x += FFN(Norm(x))) -> Decoder :64-78; Norm :117-131 (unbiased
// std, eps added to the std); MultiHeadAttention :172-226 (8 heads x 32, softmax(QK^T / sqrt(32)) V); Stacker :342-396.
// The reference runs one table at a time; here the cells of all tables of a batch are concatenated into one token
// matrix for every token-wise op (all GEMMs on the MFMA conv kernel as 1x1 convolutions, fp32 residual stream), and
// only the attention kernel looks at table boundaries (a tile list built on the host from the decode's counts).
#include <math.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "net_ctx.h"

namespace PT_FMT_NS {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

namespace {

// 16 stored bits <-> fp32 in the storage format of this namespace (act16.h: bf16, or IEEE half in pt_f16)
__device__ __forceinline__ float bf2f(uint32_t b) { return a16_to_f32(b); }
__device__ __forceinline__ uint32_t f2bf(float f) { return f32_to_a16(f); }
__device__ __forceinline__ void put(bf16_t* p, int lo_off, int split, float v) {
  const uint32_t h = f2bf(v);
  p[0] = (bf16_t)h;
  if (split) p[lo_off] = (bf16_t)f2bf(v - bf2f(h));
}
__device__ __forceinline__ float get(const bf16_t* p, int lo_off, int split) {
  float v = bf2f(p[0]);
  if (split) v += bf2f(p[lo_off]);
  return v;
}

// token t of the batch = row tok[2t+1] of table tok[2t]; writes its 256 features (+ the four 2-D position embeddings
// when pe_dets != null, lore_processor.py:486-491) to x0 [Npad,256] and to channels [256,512) of cat [Npad,512]
__global__ __launch_bounds__(256) void tok_prepare_kernel(const float* __restrict__ logi, const float* __restrict__ dets,
                                                           const int* __restrict__ tok, int N, int use_pe,
                                                           const float* __restrict__ x_pe, const float* __restrict__ y_pe,
                                                           bf16_t* __restrict__ x0, bf16_t* __restrict__ cat, int split) {
  a16_kernel_enter();
  const int t = blockIdx.x, c = threadIdx.x;
  float v = 0.f;
  if (t < N) {
    const int tb = tok[2 * t], r = tok[2 * t + 1];
    v = logi[((size_t)tb * PT_TSR_MAX_CELLS + r) * 256 + c];
    if (use_pe) {
      // filter() casts the float quad to int32 (truncation, :576-580), normalized_ps rounds and clamps to [0, 255] (:585-589)
      const float* d = dets + ((size_t)tb * PT_TSR_MAX_CELLS + r) * 9;
      int p0 = (int)d[0], p1 = (int)d[1], p2 = (int)d[2], p5 = (int)d[5];
      p0 = min(max(p0, 0), 255); p1 = min(max(p1, 0), 255); p2 = min(max(p2, 0), 255); p5 = min(max(p5, 0), 255);
      v = v + x_pe[p0 * 256 + c] + y_pe[p1 * 256 + c] + x_pe[p2 * 256 + c] + y_pe[p5 * 256 + c];
    }
  }
  put(x0 + (size_t)t * (split ? 512 : 256) + c, 256, split, v);
  put(cat + (size_t)t * (split ? 1024 : 512) + 256 + c, 512, split, v);
}

// Norm.forward (:126-131) over 256 channels, or a plain fp32 -> bf16 conversion when alpha == null.  One wave per token.
__global__ __launch_bounds__(256) void norm_kernel(const float* __restrict__ x, const float* __restrict__ alpha,
                                                    const float* __restrict__ bias, bf16_t* __restrict__ out, int Npad,
                                                    int split) {
  a16_kernel_enter();
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= Npad) return;
  const float4 v = *reinterpret_cast<const float4*>(x + (size_t)t * 256 + lane * 4);
  float o[4] = {v.x, v.y, v.z, v.w};
  if (alpha) {
    float s = v.x + v.y + v.z + v.w;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
    const float mean = s / 256.f;
    float d[4] = {v.x - mean, v.y - mean, v.z - mean, v.w - mean};
    float q = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3];
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) q += __shfl_xor(q, m);
    const float den = sqrtf(q / 255.f) + 1e-6f;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = alpha[lane * 4 + k] * d[k] / den + bias[lane * 4 + k];
  }
  bf16_t* op = out + (size_t)t * (split ? 512 : 256) + lane * 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) put(op + k, 256, split, o[k]);
}

// fp32 [Npad, 8] (4 valid) -> bf16 [Npad, 32] zero padded: the stacker's logi_encoder input (:383)
__global__ __launch_bounds__(256) void cvt_logic_kernel(const float* __restrict__ x, bf16_t* __restrict__ out, int Npad,
                                                         int split) {
  a16_kernel_enter();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Npad * 32) return;
  const int t = i >> 5, c = i & 31;
  put(out + (size_t)t * (split ? 64 : 32) + c, 32, split, c < 4 ? x[(size_t)t * 8 + c] : 0.f);
}

// attention (:134-163) for one head and 32 queries of one table, one wave, on the matrix cores.
// tiles[3i..] = (first token of the table, query offset inside it, cells in the table).
// qkv [Npad, 768] = [q | k | v] (split: [hi 768 | lo 768]); out [Npad, 256].
//   S^T (32 keys x 32 queries) = K_tile Q^T: two v_mfma_f32_32x32x16_bf16 over d = 32 (A = key rows, B = query rows,
//   both 16-byte row chunks straight from global).  In the D layout a lane owns ONE query (column lane & 31) and 16 of
//   the 32 keys, so the online soft-max is in-lane plus one exchange with lane ^ 32.
//   O^T (32 d x 32 queries) += V^T P^T: the B operand is exactly the 8 probabilities a lane already holds per
//   k-step (keys taken in the D layout's own order -- a sum does not care), the A operand gathers V[key][d] in that
//   same key order.  BF16X3 mode: three passes each (hi*hi + hi*lo + lo*hi), fp32 soft-max.
typedef __attribute__((ext_vector_type(8))) __bf16 abf16x8;
typedef __attribute__((ext_vector_type(16))) float af32x16;

__device__ __forceinline__ abf16x8 ld8(const bf16_t* p) { return *reinterpret_cast<const abf16x8*>(p); }

template <int SPLIT>
__global__ __launch_bounds__(64) void attention_kernel(const bf16_t* __restrict__ qkv, const int* __restrict__ tiles,
                                                        bf16_t* __restrict__ out) {
  a16_kernel_enter();
  const int tile = blockIdx.x, head = blockIdx.y, lane = threadIdx.x;
  const int tok0 = tiles[3 * tile], q0 = tiles[3 * tile + 1], nseg = tiles[3 * tile + 2];
  constexpr int cs = SPLIT ? 1536 : 768;
  const int col = lane & 31, half = lane >> 5;
  const int qi = q0 + col;
  const bf16_t* qrow = qkv + (size_t)(tok0 + (qi < nseg ? qi : nseg - 1)) * cs + head * 32 + half * 8;
  abf16x8 qh[2], ql[2];
  qh[0] = ld8(qrow); qh[1] = ld8(qrow + 16);
  if (SPLIT) { ql[0] = ld8(qrow + 768); ql[1] = ld8(qrow + 768 + 16); }
  af32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < nseg; k0 += 32) {
    // ---- scores: rows = keys k0 + (r & 3) + 8 (r >> 2) + 4 half, column = this lane's query
    const int krow = k0 + col;
    const bf16_t* kp = qkv + (size_t)(tok0 + (krow < nseg ? krow : nseg - 1)) * cs + 256 + head * 32 + half * 8;
    af32x16 sc;
#pragma unroll
    for (int r = 0; r < 16; ++r) sc[r] = 0.f;
    {
      const abf16x8 k0h = ld8(kp), k1h = ld8(kp + 16);
      sc = mfma_32x32x16_a16(k0h, qh[0], sc);
      sc = mfma_32x32x16_a16(k1h, qh[1], sc);
      if (SPLIT) {
        sc = mfma_32x32x16_a16(k0h, ql[0], sc);
        sc = mfma_32x32x16_a16(k1h, ql[1], sc);
        const abf16x8 k0l = ld8(kp + 768), k1l = ld8(kp + 768 + 16);
        sc = mfma_32x32x16_a16(k0l, qh[0], sc);
        sc = mfma_32x32x16_a16(k1l, qh[1], sc);
      }
    }
    float mt = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * half;
      sc[r] = key < nseg ? sc[r] / 5.656854249492381f : -INFINITY;      // scores / math.sqrt(32) (:135)
      mt = fmaxf(mt, sc[r]);
    }
    mt = fmaxf(mt, __shfl_xor(mt, 32));
    const float mn = fmaxf(m, mt);
    const float scale = expf(m - mn);
    float p[16], lt = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { p[r] = expf(sc[r] - mn); lt += p[r]; }
    lt += __shfl_xor(lt, 32);
    l = l * scale + lt;
    m = mn;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] *= scale;
    // ---- O^T += V^T P^T; k-step s covers this half's registers 8s .. 8s+7, i.e. keys k0 + (j & 3) + 8 (2s + (j >> 2)) + 4 half
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      abf16x8 ph, pl, vh, vl;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float pv = p[8 * s2 + j];
        const uint32_t hb = f2bf(pv);
        ph[j] = __builtin_bit_cast(__bf16, (uint16_t)hb);
        if (SPLIT) pl[j] = __builtin_bit_cast(__bf16, (uint16_t)f2bf(pv - bf2f(hb)));
        int key = k0 + (j & 3) + 8 * (2 * s2 + (j >> 2)) + 4 * half;
        if (key >= nseg) key = nseg - 1;                 // its probability is exactly 0
        const bf16_t* vp = qkv + (size_t)(tok0 + key) * cs + 512 + head * 32 + col;     // A row = d = lane & 31
        vh[j] = __builtin_bit_cast(__bf16, vp[0]);
        if (SPLIT) vl[j] = __builtin_bit_cast(__bf16, vp[768]);
      }
      acc = mfma_32x32x16_a16(vh, ph, acc);
      if (SPLIT) {
        acc = mfma_32x32x16_a16(vh, pl, acc);
        acc = mfma_32x32x16_a16(vl, ph, acc);
      }
    }
  }
  if (qi < nseg) {
    bf16_t* op = out + (size_t)(tok0 + qi) * (SPLIT ? 512 : 256) + head * 32;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d = (r & 3) + 8 * (r >> 2) + 4 * half;
      put(op + d, 256, SPLIT, acc[r] / l);
    }
  }
}

// fp32 [Npad, 8] token rows -> out[table][row][4]
__global__ __launch_bounds__(256) void scatter4_kernel(const float* __restrict__ x, const int* __restrict__ tok, int N,
                                                        float* __restrict__ out) {
  a16_kernel_enter();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * 4) return;
  const int t = i >> 2, c = i & 3;
  out[((size_t)tok[2 * t] * PT_TSR_MAX_CELLS + tok[2 * t + 1]) * 4 + c] = x[(size_t)t * 8 + c];
}

// Token map (table, row) of every cell and the attention's tile list (first token of the table, query offset inside it, cells in
// the table: one tile per 32 queries) of a batch of tables; *N = the token count.  pt_lore_process and pt_op_lore_* both get them here.
int build_maps(const char* who, const int32_t* h_counts, int n_tables, std::vector<int>& tok, std::vector<int>& tiles, int* N) {
  tok.clear();
  tiles.clear();
  int n = 0;
  for (int t = 0; t < n_tables; ++t) {
    const int c = h_counts[t];
    PT_REQUIRE(c >= 0 && c <= PT_TSR_MAX_CELLS, "%s: bad cell count %d", who, c);
    for (int q0 = 0; q0 < c; q0 += 32) { tiles.push_back(n); tiles.push_back(q0); tiles.push_back(c); }
    for (int r = 0; r < c; ++r) { tok.push_back(t); tok.push_back(r); }
    n += c;
  }
  *N = n;
  return PT_OK;
}

// ... to the device (either destination may be null: not wanted) through an engine-owned pinned slot: the vectors die with the call, and a
// stream synchronise here would make the host wait for everything queued on s
int upload_maps(pt_engine* e, const char* who, const std::vector<int>& tok, const std::vector<int>& tiles, int* d_tok, int* d_tiles,
                hipStream_t s) {
  const size_t nt = d_tok ? tok.size() * 4 : 0, nl = d_tiles ? tiles.size() * 4 : 0;
  if (nt + nl == 0) return PT_OK;
  char* hs = static_cast<char*>(e->stage_ring.acquire(nt + nl));
  PT_REQUIRE(hs, "%s: pinned staging (%s)", who, hipGetErrorString(hipGetLastError()));
  if (nt) memcpy(hs, tok.data(), nt);
  if (nl) memcpy(hs + nt, tiles.data(), nl);
  if (nt) PT_HIP_CHECK(hipMemcpyAsync(d_tok, hs, nt, hipMemcpyHostToDevice, s));
  if (nl) PT_HIP_CHECK(hipMemcpyAsync(d_tiles, hs + nt, nl, hipMemcpyHostToDevice, s));
  PT_REQUIRE(e->stage_ring.release(s) == 0, "%s: event record failed", who);
  return PT_OK;
}

// the five launches, shared by pt_lore_process and the op-level entry points
void launch_tok_prepare(const float* logi, const float* dets, const int* d_tok, int N, int Npad, int use_pe, const float* x_pe,
                        const float* y_pe, bf16_t* x0, bf16_t* cat, int x3, hipStream_t s) {
  hipLaunchKernelGGL(tok_prepare_kernel, dim3(Npad), dim3(256), 0, s, logi, dets, d_tok, N, use_pe, x_pe, y_pe, x0, cat, x3);
}
void launch_norm(const float* x, const float* alpha, const float* bias, bf16_t* out, int rows, int x3, hipStream_t s) {
  hipLaunchKernelGGL(norm_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, alpha, bias, out, rows, x3);
}
void launch_cvt_logic(const float* x, bf16_t* out, int Npad, int x3, hipStream_t s) {
  hipLaunchKernelGGL(cvt_logic_kernel, dim3((Npad * 32 + 255) / 256), dim3(256), 0, s, x, out, Npad, x3);
}
void launch_attention(const bf16_t* qkv, const int* d_tiles, int ntiles, bf16_t* out, int x3, hipStream_t s) {
  if (x3) hipLaunchKernelGGL(attention_kernel<1>, dim3(ntiles, 8), dim3(64), 0, s, qkv, d_tiles, out);
  else hipLaunchKernelGGL(attention_kernel<0>, dim3(ntiles, 8), dim3(64), 0, s, qkv, d_tiles, out);
}
void launch_scatter4(const float* x, const int* d_tok, int N, float* out, hipStream_t s) {
  hipLaunchKernelGGL(scatter4_kernel, dim3((N * 4 + 255) / 256), dim3(256), 0, s, x, d_tok, N, out);
}

struct P : NetCtx {
  int Npad;
  // y = x W^T + b over all tokens: x bf16 [Npad, cin] -> bf16 [Npad, out_c] at channel out_coff, or fp32 [Npad, f32_cs]
  void gemm(const bf16_t* x, int cin, const std::string& q, int N, int relu, bf16_t* out, int out_c, int out_coff,
            float* out_f32 = nullptr, int f32_cs = 0, const float* res_f32 = nullptr, int nv = 0) {
    ConvDesc c;
    if (!conv_desc(c, rows_map(x, Npad, cin), q, N, 1, 1, relu)) return;
    c.n_valid = nv;
    if (out_f32) {
      to_f32(c, out_f32, f32_cs);
      c.res_f32 = res_f32;
    } else {
      to_map(c, rows_map(out, Npad, out_c));
      c.out_coff = out_coff;
    }
    launch(c);
  }
};

}  // namespace

int pt_lore_process(pt_engine* e, const float* d_logi, const float* d_dets, const int32_t* h_counts, int n_tables,
                    int use_2dpe, float* d_logic, float* d_stacked, hipStream_t s) {
  PT_REQUIRE(d_logi && h_counts && n_tables > 0 && d_logic && d_stacked, "tsr process: null pointer");
  PT_REQUIRE(!use_2dpe || d_dets, "tsr process: 2-D position embeddings need the cell quads");
  const PtModel* M = pt_find_model(e, PT_MODEL_LORE_PROCESSOR, "Lore processor", "PT_MODEL_LORE_PROCESSOR");
  if (!M) return PT_ERR_STATE;
  std::vector<int> tok, tiles;
  int N = 0;
  if (int rc = build_maps("tsr process", h_counts, n_tables, tok, tiles, &N)) return rc;
  if (N == 0) return PT_OK;
  P p;
  p.init(e, M, "Lore processor", s, 1, PT_ARENA_TSRP);      // n = 1: every GEMM sees the tokens as one [Npad / 32, 32] map
  p.Npad = (N + 127) / 128 * 128;
  const int Npad = p.Npad, x3 = p.x3;
  const PtTensor* meta = p.get("meta");
  if (p.rc != PT_OK) return p.rc;
  int layers[2];
  {
    // the two layer counts: read from the blob once per loaded model (a per-call hipMemcpy would wait for the whole default stream)
    std::vector<int32_t>& hw = e->models[PT_MODEL_LORE_PROCESSOR].host_words["meta"];
    if (hw.size() != 2) {
      hw.assign(2, 0);
      PT_HIP_CHECK(hipMemcpy(hw.data(), meta->d_ptr, 8, hipMemcpyDeviceToHost));
    }
    layers[0] = hw[0];
    layers[1] = hw[1];
  }

  // activations from the arena (grown once if needed)
  const size_t be = sizeof(bf16_t) * p.mul;
  float *x, *lg, *sk;
  bf16_t *x0, *xb, *qkv, *att, *hbuf, *cat, *l32, *le;
  int *d_tok, *d_tiles;
  const int prc = pt_arena_plan(e, PT_ARENA_TSRP, "tsr process", [&](auto&& take) {
    auto act = [&](int C) { return reinterpret_cast<bf16_t*>(take((size_t)Npad * C * be)); };
    x = reinterpret_cast<float*>(take((size_t)Npad * 256 * 4));
    x0 = act(256); xb = act(256); qkv = act(768); att = act(256); hbuf = act(2048); cat = act(512); l32 = act(32); le = act(256);
    lg = reinterpret_cast<float*>(take((size_t)Npad * 8 * 4));
    sk = reinterpret_cast<float*>(take((size_t)Npad * 8 * 4));
    d_tok = reinterpret_cast<int*>(take(tok.size() * 4));
    d_tiles = reinterpret_cast<int*>(take(tiles.size() * 4));
  });
  if (prc != PT_OK) return prc;
  if (int rc = upload_maps(e, "tsr process", tok, tiles, d_tok, d_tiles, s)) return rc;

  const PtTensor *xpe = p.get("x_pe"), *ype = p.get("y_pe");
  if (p.rc != PT_OK) return p.rc;
  const int ntiles = (int)tiles.size() / 3;
  {
    PtProfScope ps(e, s, PT_PROF_OTHER, 0, "tsr tok prepare");
    launch_tok_prepare(d_logi, d_dets, d_tok, N, Npad, use_2dpe, F(xpe), F(ype), x0, cat, x3, s);
  }
  auto norm = [&](const std::string& q) {
    const PtTensor* a = q.empty() ? nullptr : p.get(q + ".alpha");
    const PtTensor* b = q.empty() ? nullptr : p.get(q + ".bias");
    if (p.rc != PT_OK) return;
    PtProfScope ps(e, s, PT_PROF_OTHER, 0, "tsr norm");
    launch_norm(x, a ? F(a) : nullptr, b ? F(b) : nullptr, xb, Npad, x3, s);
  };
  auto transformer = [&](const std::string& q, const bf16_t* in, int cin, int nl, float* out4) {
    p.gemm(in, cin, q + ".linear", 256, 0, nullptr, 0, 0, x, 256);
    for (int l = 0; l < nl; ++l) {
      const std::string lq = q + ".l" + std::to_string(l);
      norm(lq + ".norm_1");
      p.gemm(xb, 256, lq + ".qkv", 768, 0, qkv, 768, 0);
      if (p.rc == PT_OK) {
        PtProfScope ps(e, s, PT_PROF_OTHER, 0, "tsr attention");
        launch_attention(qkv, d_tiles, ntiles, att, x3, s);
      }
      p.gemm(att, 256, lq + ".out", 256, 0, nullptr, 0, 0, x, 256, x);
      norm(lq + ".norm_2");
      p.gemm(xb, 256, lq + ".ff1", 2048, 1, hbuf, 2048, 0);
      p.gemm(hbuf, 2048, lq + ".ff2", 256, 0, nullptr, 0, 0, x, 256, x);
    }
    norm("");                                                         // fp32 stream -> bf16 for the decoder GEMMs
    p.gemm(xb, 256, q + ".dec0", 256, 1, att, 256, 0);
    p.gemm(att, 256, q + ".dec2", 64, 1, nullptr, 0, 0, out4, 8, nullptr, 8);
  };
  // attention output rows of pad tokens are never written: clear once so that no NaN bit pattern reaches a GEMM
  PT_HIP_CHECK(hipMemsetAsync(att, 0, (size_t)Npad * 256 * be, s));
  transformer("axis", x0, 256, layers[0], lg);
  {
    PtProfScope ps(e, s, PT_PROF_OTHER, 0, "tsr cvt logic");
    launch_cvt_logic(lg, l32, Npad, x3, s);
  }
  p.gemm(l32, 32, "stk.le0", 256, 1, le, 256, 0);
  p.gemm(le, 256, "stk.le2", 256, 1, cat, 512, 0);                    // channels [0, 256) of the concat (:385)
  transformer("stk", cat, 512, layers[1], sk);
  if (p.rc != PT_OK) return p.rc;
  launch_scatter4(lg, d_tok, N, d_logic, s);
  launch_scatter4(sk, d_tok, N, d_stacked, s);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

// ---- the kernels above one at a time (tests/test_gpu_lore_proc_ops.py): engine handle and stream only, no model loaded, the launch helpers and
// the map builder of pt_lore_process on caller-owned buffers.  No allocation on the device and no host synchronisation.  Everything a kernel
// would index with is checked here: a refused call launches nothing.
namespace api {

namespace {
int op_counts(const char* who, const int32_t* h_counts, int n_tables, int Npad, std::vector<int>& tok, std::vector<int>& tiles, int* N) {
  PT_REQUIRE(h_counts && n_tables >= 1 && n_tables <= 65535, "%s: n_tables = %d (1 .. 65535) with its host counts", who, n_tables);
  if (int rc = build_maps(who, h_counts, n_tables, tok, tiles, N)) return rc;
  PT_REQUIRE(Npad >= 128 && Npad % 128 == 0 && Npad >= *N && Npad <= (1 << 24), "%s: Npad = %d must be a multiple of 128 and hold the %d tokens", who, Npad, *N);
  return PT_OK;
}
}  // namespace

int pt_op_lore_tok_prepare(pt_engine* e, const float* d_logi, const float* d_dets, const int32_t* h_counts, int n_tables, int use_pe, const float* d_x_pe,
                           const float* d_y_pe, int Npad, int32_t* d_tok, uint16_t* d_x0, uint16_t* d_cat, int split, pt_stream stream) {
  PT_REQUIRE(e && d_logi && d_tok && d_x0 && d_cat, "pt_op_lore_tok_prepare: null argument");
  PT_REQUIRE(!use_pe || (d_dets && d_x_pe && d_y_pe), "pt_op_lore_tok_prepare: position embeddings need the cell quads and both tables");
  std::vector<int> tok, tiles;
  int N = 0;
  if (int rc = op_counts("pt_op_lore_tok_prepare", h_counts, n_tables, Npad, tok, tiles, &N)) return rc;
  if (N == 0) return PT_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (int rc = upload_maps(e, "pt_op_lore_tok_prepare", tok, tiles, d_tok, nullptr, s)) return rc;
  launch_tok_prepare(d_logi, d_dets, d_tok, N, Npad, use_pe ? 1 : 0, d_x_pe, d_y_pe, reinterpret_cast<bf16_t*>(d_x0), reinterpret_cast<bf16_t*>(d_cat), split ? 1 : 0, s);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

int pt_op_lore_norm(pt_engine* e, const float* d_x, int rows, const float* d_alpha, const float* d_bias, uint16_t* d_out, int split, pt_stream stream) {
  PT_REQUIRE(e && d_x && d_out, "pt_op_lore_norm: null argument");
  PT_REQUIRE((d_alpha == nullptr) == (d_bias == nullptr), "pt_op_lore_norm: alpha and bias go together (both null: conversion only)");
  PT_REQUIRE(rows >= 1 && rows <= (1 << 24), "pt_op_lore_norm: rows = %d", rows);
  PT_REQUIRE(((uintptr_t)d_x & 15) == 0, "pt_op_lore_norm: unaligned pointer");
  launch_norm(d_x, d_alpha, d_bias, reinterpret_cast<bf16_t*>(d_out), rows, split ? 1 : 0, reinterpret_cast<hipStream_t>(stream));
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

int pt_op_lore_cvt_logic(pt_engine* e, const float* d_x, uint16_t* d_out, int Npad, int split, pt_stream stream) {
  PT_REQUIRE(e && d_x && d_out, "pt_op_lore_cvt_logic: null argument");
  PT_REQUIRE(Npad >= 128 && Npad % 128 == 0 && Npad <= (1 << 24), "pt_op_lore_cvt_logic: Npad = %d must be a positive multiple of 128", Npad);
  launch_cvt_logic(d_x, reinterpret_cast<bf16_t*>(d_out), Npad, split ? 1 : 0, reinterpret_cast<hipStream_t>(stream));
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

int pt_op_lore_attention(pt_engine* e, const uint16_t* d_qkv, const int32_t* h_counts, int n_tables, int Npad, int32_t* d_tiles, uint16_t* d_out, int split,
                         pt_stream stream) {
  PT_REQUIRE(e && d_qkv && d_tiles && d_out, "pt_op_lore_attention: null argument");
  PT_REQUIRE(((uintptr_t)d_qkv & 15) == 0, "pt_op_lore_attention: unaligned pointer");
  std::vector<int> tok, tiles;
  int N = 0;
  if (int rc = op_counts("pt_op_lore_attention", h_counts, n_tables, Npad, tok, tiles, &N)) return rc;
  if (N == 0) return PT_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (int rc = upload_maps(e, "pt_op_lore_attention", tok, tiles, nullptr, d_tiles, s)) return rc;
  launch_attention(reinterpret_cast<const bf16_t*>(d_qkv), d_tiles, (int)tiles.size() / 3, reinterpret_cast<bf16_t*>(d_out), split ? 1 : 0, s);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

int pt_op_lore_scatter4(pt_engine* e, const float* d_x, const int32_t* d_tok, int N, float* d_out, pt_stream stream) {
  PT_REQUIRE(e && d_x && d_tok && d_out, "pt_op_lore_scatter4: null argument");
  PT_REQUIRE(N >= 0 && N <= (1 << 24), "pt_op_lore_scatter4: N = %d", N);
  if (N == 0) return PT_OK;
  launch_scatter4(d_x, d_tok, N, d_out, reinterpret_cast<hipStream_t>(stream));
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

}  // namespace api

}  // namespace PT_FMT_NS
