// teds.hip -- the TEDS table metric (Tree-Edit-Distance-based Similarity, Zhong et al. 2020) on the device: the two hot parts of
// pdf_table_amd/table_metric.py for a batch of (prediction, truth) table pairs.  Entry points added under ABI 21 (new entry points, no existing
// signature changed).  pdf_table_amd/table_metric.py states the same arithmetic on the host; tests compare the two.
//
// pt_op_teds_cost -- the rename cost of two cells, levenshtein(tokens1, tokens2) / max(len1, len2) in float64, for every (row content, column content)
//   of every table pair.  Contents are token-id runs in one CSR store; a table pair names a range of row contents and a range of column contents.
//   grid = (blocks, table pairs), one THREAD per content pair: the same store index on both sides is 0 without a token read; else the common prefix
//   and suffix are stripped (equal contents end here with distance 0: a good prediction is mostly equal cells), and what is left runs
//     - min(len) <= 64: the two-row recurrence with the shorter content's row in LDS (uint16, lane-interleaved: no bank conflicts), serial per thread;
//     - both > 64 (up to 1024): queued in an LDS list, then ONE WAVE per content pair with the row in registers, 17 columns per lane: per row of the
//       table t[j] = min(up + 1, diag + sub) is local (the diagonal of a lane's first column comes by __shfl_up), and the insert chain
//       cur[j] = min_k<=j (t[k] + j - k) is a prefix minimum of t[k] - k: serial inside the lane, a shuffle scan over the 64 lane totals.
//   The division is one float64 division of two exact integers, so the result is bit-equal to the host's.
//
// pt_op_teds_dist -- the ordered tree edit distance (insert = delete = 1) of every table pair: Zhang-Shasha, ONE WORKGROUP per pair, workgroups share
//   nothing (no flags, no spins, no grid barrier, no atomics).  Trees come flattened in postorder (tag, colspan, rowspan, content id, leftmost leaf per
//   node) with their keyroots grouped by height, within a height by size descending.  The keyroot pairs are scheduled IN PHASES by (height group of
//   keyroot 1, height group of keyroot 2) in lexicographic order: the keyroots of one height have disjoint subtrees, so the pairs of a phase write
//   disjoint rectangles [l(k1), k1] x [l(k2), k2] of ONE N1 x N2 forest-distance plane and disjoint entries of ONE N1 x N2 tree-distance plane (both
//   in the caller's scratch), and every tree distance a pair reads was written in an earlier phase: entry (i, j) off the spines of (k1, k2) belongs to
//   the keyroots (kr(i), kr(j)), of which kr(i) is k1 or lower than k1, and where it is k1, kr(j) is lower than k2.  The forest distances against the
//   empty forest are the node counts (unit costs) and are not stored: that is why the plane needs no border row shared by neighbouring rectangles.
//     - a pair with a side narrower than 64 nodes (cell x cell, row x row, row x table) goes to ONE LANE, walked serially;
//     - a pair with both sides >= 64 nodes (section x section, table x table) goes to the WHOLE WORKGROUP on anti-diagonals, one barrier per
//       diagonal: every dependency of (i, j) -- (i-1, j), (i, j-1), (i-1, j-1), (l(i)-1, l(j)-1) -- lies on an earlier diagonal.
//   Every loop is bounded by a node, keyroot or group count the host checked; every index read from device memory is clamped before use.
//   float64 throughout, -ffp-contract=off: each entry is one addition and a minimum, the same operations as the host route's.
// These kernels read int32 / int64 / fp64 arrays only, so the translation unit is compiled ONCE (build.py: ONCE_HIP_SOURCES), as namespace pt_bf16.
#include <math.h>

#include "common.h"

using PT_FMT_NS::a16_kernel_enter;

namespace {

constexpr int kTedsThreads = 256;       // 4 waves
constexpr int kTedsMaxNodes = 4096;
constexpr int kTedsMaxTokens = 1024;
constexpr int kTedsShort = 64;          // cost: a content pair whose shorter side is at most this long runs in one thread
constexpr int kTedsChunk = 17;          // cost, wave path: columns per lane, 64 * 17 = 1088 >= 1024 + 1
constexpr int kTedsWide = 64;           // dist: both sides at least this many nodes -> anti-diagonals of the workgroup
constexpr int kTedsBig = 1 << 20;
constexpr int kCostPairInts = 5;        // r0, nr, c0, nc, out_off
constexpr int kDistPairInts = 16;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ long long clampl(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- cost ---------------------------------------------------------------------------------------------------------------------------------------
struct TedsRun {
  const int32_t* p;
  int len;
};

__device__ __forceinline__ TedsRun teds_content(const int32_t* __restrict__ tok, long long n_tok, const int32_t* __restrict__ coff, int idx) {
  long long a0 = clampl(coff[idx], 0, n_tok), a1 = clampl(coff[idx + 1], 0, n_tok);
  int len = a1 > a0 ? (int)(a1 - a0 > kTedsMaxTokens ? kTedsMaxTokens : a1 - a0) : 0;
  TedsRun r;
  r.p = tok + a0;
  r.len = len;
  return r;
}

// strips the common prefix and suffix (the distance does not change); a ends up the shorter run
__device__ __forceinline__ void teds_strip(TedsRun& a, TedsRun& b) {
  int pre = 0;
  const int lim = a.len < b.len ? a.len : b.len;
  while (pre < lim && a.p[pre] == b.p[pre]) ++pre;
  a.p += pre;
  b.p += pre;
  a.len -= pre;
  b.len -= pre;
  while (a.len > 0 && b.len > 0 && a.p[a.len - 1] == b.p[b.len - 1]) {
    --a.len;
    --b.len;
  }
  if (a.len > b.len) {
    const TedsRun t = a;
    a = b;
    b = t;
  }
}

// one wave, both runs longer than kTedsShort and at most kTedsMaxTokens: returns the distance in every lane
__device__ int teds_lev_wave(const TedsRun a, const TedsRun b, int lane) {
  const int n = b.len;
  int prev[kTedsChunk], bt[kTedsChunk];
#pragma unroll
  for (int c = 0; c < kTedsChunk; ++c) {
    const int j = lane * kTedsChunk + c;
    prev[c] = j <= n ? j : kTedsBig;
    bt[c] = (j >= 1 && j <= n) ? b.p[j - 1] : 0;
  }
  for (int i = 1; i <= a.len; ++i) {
    const int ai = a.p[i - 1];
    int left = __shfl_up(prev[kTedsChunk - 1], 1);
    int u[kTedsChunk];
    int run = kTedsBig;
#pragma unroll
    for (int c = 0; c < kTedsChunk; ++c) {
      const int j = lane * kTedsChunk + c;
      const int diag = c == 0 ? left : prev[c - 1];
      int t = min(prev[c] + 1, diag + (ai != bt[c] ? 1 : 0));
      if (j == 0) t = i;
      if (j > n) t = kTedsBig;
      run = min(run, t - j);
      u[c] = run;
    }
    int tot = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(tot, o);
      if (lane >= o) tot = min(tot, v);
    }
    int excl = __shfl_up(tot, 1);
    if (lane == 0) excl = kTedsBig;
#pragma unroll
    for (int c = 0; c < kTedsChunk; ++c) prev[c] = min(u[c], excl) + lane * kTedsChunk + c;
  }
  int res = 0;
#pragma unroll
  for (int c = 0; c < kTedsChunk; ++c)
    if (lane * kTedsChunk + c == n) res = prev[c];
  return __shfl(res, n / kTedsChunk);
}

__global__ __launch_bounds__(kTedsThreads) void teds_cost_kernel(const int32_t* __restrict__ tok, long long n_tok, const int32_t* __restrict__ coff,
                                                                 int n_cont, const long long* __restrict__ pairs, double* __restrict__ C,
                                                                 long long c_elems) {
  a16_kernel_enter();
  __shared__ uint16_t row[(kTedsShort + 1) * kTedsThreads];
  __shared__ int long_list[kTedsThreads];
  __shared__ int n_long;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long* pr = pairs + (size_t)blockIdx.y * kCostPairInts;
  const int nr = (int)clampl(pr[1], 0, n_cont), nc = (int)clampl(pr[3], 0, n_cont);
  const int r0 = (int)clampl(pr[0], 0, n_cont - nr), c0 = (int)clampl(pr[2], 0, n_cont - nc);
  const long long total = (long long)nr * nc;
  if (total == 0) return;
  const long long out_off = clampl(pr[4], 0, c_elems - total);
  if (out_off < 0 || pr[4] != out_off) return;                          // the host refused this already; never write outside C
  for (long long base = (long long)blockIdx.x * kTedsThreads; base < total; base += (long long)gridDim.x * kTedsThreads) {   // block-uniform
    if (tid == 0) n_long = 0;
    __syncthreads();
    const long long idx = base + tid;
    if (idx < total) {
      const int ia = r0 + (int)(idx / nc), ib = c0 + (int)(idx % nc);
      TedsRun a = teds_content(tok, n_tok, coff, ia), b = teds_content(tok, n_tok, coff, ib);
      const int longest = a.len > b.len ? a.len : b.len;
      int dist = -1;
      if (ia == ib) {
        dist = 0;
      } else {
        teds_strip(a, b);
        if (a.len == 0) {
          dist = b.len;
        } else if (a.len <= kTedsShort) {
          uint16_t* rw = row + tid;
          for (int k = 0; k <= a.len; ++k) rw[k * kTedsThreads] = (uint16_t)k;
          int left = a.len;
          for (int j = 0; j < b.len; ++j) {
            const int bj = b.p[j];
            int diag = j;
            left = j + 1;
            rw[0] = (uint16_t)left;
            for (int k = 1; k <= a.len; ++k) {
              const int up = rw[k * kTedsThreads];
              const int v = min(min(up + 1, left + 1), diag + (a.p[k - 1] != bj ? 1 : 0));
              rw[k * kTedsThreads] = (uint16_t)v;
              diag = up;
              left = v;
            }
          }
          dist = left;
        } else {
          long_list[atomicAdd(&n_long, 1)] = tid;                       // LDS counter: at most kTedsThreads entries per round
        }
      }
      if (dist >= 0) C[out_off + idx] = longest > 0 ? (double)dist / (double)longest : 0.0;
    }
    __syncthreads();
    const int nl = n_long < kTedsThreads ? n_long : kTedsThreads;
    for (int q = wave; q < nl; q += kTedsThreads / 64) {               // wave-uniform
      const long long idx2 = base + clampi(long_list[q], 0, kTedsThreads - 1);
      if (idx2 >= total) continue;
      const int ia = r0 + (int)(idx2 / nc), ib = c0 + (int)(idx2 % nc);
      TedsRun a = teds_content(tok, n_tok, coff, ia), b = teds_content(tok, n_tok, coff, ib);
      const int longest = a.len > b.len ? a.len : b.len;
      teds_strip(a, b);
      const int dist = teds_lev_wave(a, b, lane);
      if (lane == 0) C[out_off + idx2] = (double)dist / (double)longest;
    }
    __syncthreads();
  }
}

// ---- dist ---------------------------------------------------------------------------------------------------------------------------------------
struct TedsTree {
  const int4* node;       // (tag, colspan, rowspan, content id or -1)
  const int32_t* lml;
  const int32_t* kr;
  const int32_t* grp;
  int n, nkr, ngrp;
};

struct TedsCtx {
  TedsTree t1, t2;
  const double* C;
  int crows, ccols;
  double* FD;             // [n1, n2] forest distances of the keyroot pair that owns the entry
  double* TD;             // [n1, n2] tree distances
};

__device__ __forceinline__ double teds_rename(const TedsCtx& x, int i, int j) {
  const int4 a = x.t1.node[i], b = x.t2.node[j];
  if (a.x != b.x || a.y != b.y || a.z != b.z) return 1.0;
  if (a.w >= 0 && b.w >= 0 && x.crows > 0 && x.ccols > 0) return x.C[(size_t)min(a.w, x.crows - 1) * x.ccols + min(b.w, x.ccols - 1)];
  return 0.0;
}

// forest distance of (l1 .. i, l2 .. j); i < l1 or j < l2: an empty side, the other side's node count
__device__ __forceinline__ double teds_fd(const TedsCtx& x, int i, int j, int l1, int l2) {
  if (i < l1) return j < l2 ? 0.0 : (double)(j - l2 + 1);
  if (j < l2) return (double)(i - l1 + 1);
  return x.FD[(size_t)i * x.t2.n + j];
}

__device__ __forceinline__ void teds_cell(const TedsCtx& x, int i, int j, int l1, int l2) {
  const int li = clampi(x.t1.lml[i], 0, i), lj = clampi(x.t2.lml[j], 0, j);
  const size_t at = (size_t)i * x.t2.n + j;
  const double del = teds_fd(x, i - 1, j, l1, l2) + 1.0, ins = teds_fd(x, i, j - 1, l1, l2) + 1.0;
  double v = fmin(del, ins);
  if (li == l1 && lj == l2) {
    v = fmin(v, teds_fd(x, i - 1, j - 1, l1, l2) + teds_rename(x, i, j));
    x.TD[at] = v;
  } else {
    v = fmin(v, teds_fd(x, li - 1, lj - 1, l1, l2) + x.TD[at]);
  }
  x.FD[at] = v;
}

__device__ __forceinline__ TedsTree teds_tree(const long long* m, int side, const int32_t* node, const int32_t* lml, long long n_nodes, const int32_t* kr,
                                              long long n_kr, const int32_t* grp, long long n_grp) {
  TedsTree t;
  const long long* q = side ? m + 2 : m;
  const long long* k = side ? m + 8 : m + 4;
  t.n = (int)clampl(q[0], 1, kTedsMaxNodes < n_nodes ? kTedsMaxNodes : n_nodes);
  const long long noff = clampl(q[1], 0, n_nodes - t.n);
  t.node = reinterpret_cast<const int4*>(node) + noff;
  t.lml = lml + noff;
  t.nkr = (int)clampl(k[1], 0, t.n < n_kr ? t.n : n_kr);
  t.kr = kr + clampl(k[0], 0, n_kr - t.nkr);
  t.ngrp = (int)clampl(k[3], 0, t.nkr < n_grp - 1 ? t.nkr : n_grp - 1);
  t.grp = grp + clampl(k[2], 0, n_grp - 1 - t.ngrp);
  return t;
}

__global__ __launch_bounds__(kTedsThreads) void teds_dist_kernel(const long long* __restrict__ pairs, const int32_t* __restrict__ node,
                                                                 const int32_t* __restrict__ lml, long long n_nodes, const int32_t* __restrict__ kr,
                                                                 long long n_kr, const int32_t* __restrict__ grp, long long n_grp,
                                                                 const double* __restrict__ C, long long c_elems, double* scratch,
                                                                 long long scratch_elems, double* __restrict__ out) {
  a16_kernel_enter();
  const int tid = threadIdx.x;
  const long long* m = pairs + (size_t)blockIdx.x * kDistPairInts;
  TedsCtx x;
  x.t1 = teds_tree(m, 0, node, lml, n_nodes, kr, n_kr, grp, n_grp);
  x.t2 = teds_tree(m, 1, node, lml, n_nodes, kr, n_kr, grp, n_grp);
  const int n1 = x.t1.n, n2 = x.t2.n;
  x.crows = (int)clampl(m[13], 0, 2 * kTedsMaxNodes);
  x.ccols = (int)clampl(m[14], 0, 2 * kTedsMaxNodes);
  const long long cneed = (long long)x.crows * x.ccols;
  if (cneed > c_elems) x.crows = x.ccols = 0;
  x.C = C + clampl(m[12], 0, c_elems - (long long)x.crows * x.ccols);
  const long long plane = (long long)n1 * n2;
  if (2 * plane > scratch_elems) return;                                // block-uniform; the host refused this already
  x.FD = scratch + clampl(m[15], 0, scratch_elems - 2 * plane);
  x.TD = x.FD + plane;

  for (int g1 = 0; g1 < x.t1.ngrp; ++g1) {
    const int a0 = clampi(x.t1.grp[g1], 0, x.t1.nkr), a1 = clampi(x.t1.grp[g1 + 1], a0, x.t1.nkr);
    for (int g2 = 0; g2 < x.t2.ngrp; ++g2) {
      const int b0 = clampi(x.t2.grp[g2], 0, x.t2.nkr), b1 = clampi(x.t2.grp[g2 + 1], b0, x.t2.nkr);
      const int na = a1 - a0, nb = b1 - b0;
      // narrow pairs: one lane each, serial
      for (long long q = tid; q < (long long)na * nb; q += kTedsThreads) {
        const int k1 = clampi(x.t1.kr[a0 + (int)(q / nb)], 0, n1 - 1), k2 = clampi(x.t2.kr[b0 + (int)(q % nb)], 0, n2 - 1);
        const int l1 = clampi(x.t1.lml[k1], 0, k1), l2 = clampi(x.t2.lml[k2], 0, k2);
        if (k1 - l1 + 1 >= kTedsWide && k2 - l2 + 1 >= kTedsWide) continue;
        for (int i = l1; i <= k1; ++i)
          for (int j = l2; j <= k2; ++j) teds_cell(x, i, j, l1, l2);
      }
      // wide pairs: the workgroup on anti-diagonals (keyroots of a group come by size descending, so the first narrow one ends the scan)
      for (int ia = 0; ia < na; ++ia) {                                 // block-uniform: every thread reaches every barrier below
        const int k1 = clampi(x.t1.kr[a0 + ia], 0, n1 - 1), l1 = clampi(x.t1.lml[k1], 0, k1), s1 = k1 - l1 + 1;
        if (s1 < kTedsWide) break;
        for (int ib = 0; ib < nb; ++ib) {
          const int k2 = clampi(x.t2.kr[b0 + ib], 0, n2 - 1), l2 = clampi(x.t2.lml[k2], 0, k2), s2 = k2 - l2 + 1;
          if (s2 < kTedsWide) break;
          for (int d = 0; d <= s1 + s2 - 2; ++d) {
            const int lo = d - (s2 - 1) > 0 ? d - (s2 - 1) : 0, hi = d < s1 - 1 ? d : s1 - 1;
            for (int a = lo + tid; a <= hi; a += kTedsThreads) teds_cell(x, l1 + a, l2 + (d - a), l1, l2);
            __syncthreads();
          }
        }
      }
      __syncthreads();
    }
  }
  if (tid == 0) out[blockIdx.x] = x.TD[plane - 1];
}

bool teds_tree_ok(const int64_t* q, const int64_t* k, long long n_nodes, long long n_kr, long long n_grp) {
  return q[0] >= 1 && q[0] <= kTedsMaxNodes && q[1] >= 0 && q[1] + q[0] <= n_nodes && k[1] >= 1 && k[1] <= q[0] && k[0] >= 0 && k[0] + k[1] <= n_kr &&
         k[3] >= 1 && k[3] <= k[1] && k[2] >= 0 && k[2] + k[3] + 1 <= n_grp;
}

}  // namespace

namespace PT_FMT_NS {
namespace api {

int pt_op_teds_scratch_bytes(int n1, int n2, long long* bytes) {
  PT_REQUIRE(bytes, "pt_op_teds_scratch_bytes: null pointer");
  PT_REQUIRE(n1 >= 1 && n1 <= kTedsMaxNodes && n2 >= 1 && n2 <= kTedsMaxNodes, "pt_op_teds_scratch_bytes: node counts %d, %d outside 1 .. %d", n1, n2,
             kTedsMaxNodes);
  *bytes = 2ll * n1 * n2 * (long long)sizeof(double);
  return PT_OK;
}

int pt_op_teds_cost(const int32_t* d_tok, long long n_tok, const int32_t* d_coff, const int32_t* h_coff, int n_cont, const int64_t* d_pairs,
                    const int64_t* h_pairs, int P, double* d_C, long long c_elems, pt_stream stream) {
  PT_REQUIRE(P >= 0 && P <= 65535 && n_cont >= 0 && n_tok >= 0 && c_elems >= 0, "pt_op_teds_cost: bad arguments (P %d: 0 .. 65535, n_cont %d, n_tok %lld, "
             "c_elems %lld)", P, n_cont, n_tok, c_elems);
  if (P == 0) return PT_OK;
  PT_REQUIRE(d_pairs && h_pairs && d_coff && h_coff, "pt_op_teds_cost: null pointer");
  PT_REQUIRE(h_coff[0] == 0, "pt_op_teds_cost: content offsets must start at 0");
  for (int k = 0; k < n_cont; ++k) {
    const long long len = (long long)h_coff[k + 1] - h_coff[k];
    PT_REQUIRE(len >= 0 && h_coff[k + 1] <= n_tok, "pt_op_teds_cost: content %d has offsets %d .. %d (tokens: %lld)", k, h_coff[k], h_coff[k + 1], n_tok);
    PT_REQUIRE(len <= kTedsMaxTokens, "pt_op_teds_cost: content %d has %lld tokens, more than %d", k, len, kTedsMaxTokens);
  }
  long long most = 0;
  for (int p = 0; p < P; ++p) {
    const int64_t* q = h_pairs + (size_t)p * kCostPairInts;
    PT_REQUIRE(q[1] >= 0 && q[3] >= 0 && q[0] >= 0 && q[2] >= 0 && q[0] + q[1] <= n_cont && q[2] + q[3] <= n_cont,
               "pt_op_teds_cost: pair %d names contents %lld + %lld and %lld + %lld of %d", p, (long long)q[0], (long long)q[1], (long long)q[2],
               (long long)q[3], n_cont);
    const long long total = (long long)q[1] * q[3];
    PT_REQUIRE(q[4] >= 0 && q[4] + total <= c_elems, "pt_op_teds_cost: pair %d writes %lld costs at %lld, C holds %lld", p, total, (long long)q[4], c_elems);
    most = total > most ? total : most;
  }
  if (most == 0) return PT_OK;
  PT_REQUIRE(d_tok || n_tok == 0, "pt_op_teds_cost: null pointer (tokens)");
  PT_REQUIRE(d_C, "pt_op_teds_cost: null pointer (C)");
  long long bx = (most + kTedsThreads - 1) / kTedsThreads;
  bx = bx > 1024 ? 1024 : bx;
  hipLaunchKernelGGL(teds_cost_kernel, dim3((unsigned)bx, (unsigned)P), dim3(kTedsThreads), 0, (hipStream_t)stream, d_tok, n_tok, d_coff, n_cont,
                     reinterpret_cast<const long long*>(d_pairs), d_C, c_elems);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

int pt_op_teds_dist(const int64_t* d_pairs, const int64_t* h_pairs, int P, const int32_t* d_node, const int32_t* d_lml, long long n_nodes,
                    const int32_t* d_kr, long long n_kr, const int32_t* d_grp, long long n_grp, const double* d_C, long long c_elems, double* d_scratch,
                    long long scratch_bytes, double* d_out, pt_stream stream) {
  PT_REQUIRE(P >= 0 && P <= 65535 && n_nodes >= 0 && n_kr >= 0 && n_grp >= 0 && c_elems >= 0 && scratch_bytes >= 0,
             "pt_op_teds_dist: bad arguments (P %d: 0 .. 65535)", P);
  if (P == 0) return PT_OK;
  PT_REQUIRE(d_pairs && h_pairs && d_node && d_lml && d_kr && d_grp && d_scratch && d_out, "pt_op_teds_dist: null pointer");
  PT_REQUIRE((reinterpret_cast<uintptr_t>(d_node) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_scratch) & 7) == 0,
             "pt_op_teds_dist: node records must be 16-byte aligned, the scratch 8-byte");
  long long end = 0;
  for (int p = 0; p < P; ++p) {
    const int64_t* q = h_pairs + (size_t)p * kDistPairInts;
    PT_REQUIRE(q[0] >= 1 && q[0] <= kTedsMaxNodes && q[2] >= 1 && q[2] <= kTedsMaxNodes, "pt_op_teds_dist: pair %d has %lld and %lld nodes, outside 1 .. %d",
               p, (long long)q[0], (long long)q[2], kTedsMaxNodes);
    PT_REQUIRE(teds_tree_ok(q, q + 4, n_nodes, n_kr, n_grp) && teds_tree_ok(q + 2, q + 8, n_nodes, n_kr, n_grp),
               "pt_op_teds_dist: pair %d names nodes, keyroots or groups outside the arrays", p);
    PT_REQUIRE(q[13] >= 0 && q[14] >= 0 && q[13] <= 2 * kTedsMaxNodes && q[14] <= 2 * kTedsMaxNodes && q[12] >= 0 && q[12] + q[13] * q[14] <= c_elems,
               "pt_op_teds_dist: pair %d reads a %lld x %lld cost matrix at %lld, C holds %lld", p, (long long)q[13], (long long)q[14], (long long)q[12],
               c_elems);
    PT_REQUIRE(q[13] * q[14] == 0 || d_C, "pt_op_teds_dist: null pointer (C)");
    const long long need = 2ll * q[0] * q[2];
    PT_REQUIRE(q[15] >= end && (q[15] + need) * (long long)sizeof(double) <= scratch_bytes,
               "pt_op_teds_dist: pair %d needs %lld bytes of scratch at %lld (after %lld), the scratch holds %lld", p, need * (long long)sizeof(double),
               (long long)q[15] * (long long)sizeof(double), end * (long long)sizeof(double), scratch_bytes);
    end = q[15] + need;
  }
  hipLaunchKernelGGL(teds_dist_kernel, dim3((unsigned)P), dim3(kTedsThreads), 0, (hipStream_t)stream, reinterpret_cast<const long long*>(d_pairs), d_node,
                     d_lml, n_nodes, d_kr, n_kr, d_grp, n_grp, d_C, c_elems, d_scratch, scratch_bytes / (long long)sizeof(double), d_out);
  PT_HIP_CHECK(hipGetLastError());
  return PT_OK;
}

}  // namespace api
}  // namespace PT_FMT_NS
