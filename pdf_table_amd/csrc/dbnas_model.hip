// dbnas_model.hip -- launch graph of the DB-ProxylessNAS text detector (`DBNasModel`, db_net/dbnet.py:693-712):
// CompactDetBackbone (db_net/proxyless.py:92-178, searched block list :118-127) -> LightSegDetector (dbnet.py:338-481),
// eval branch (`binary` only).
//
// Engine mapping (weights.pack_db_nas folds every BatchNorm):
//   * first_conv 3x3 s2 (3 -> 32) + ReLU: direct VALU kernel;
//   * each inverted-residual block = 1x1 expand on the MFMA kernel (PReLU epilogue), ONE depthwise k x k kernel -- the
//     `rep` blocks' sum of 1x1 / 3x3 / 5x5 depthwise branches (layers.py:732-745) is a single 5x5 depthwise conv after
//     folding, the same re-parameterisation the reference's own `deploy` switch stands for -- with PReLU, and the 1x1
//     projection on the MFMA kernel with the identity shortcut added in its epilogue;
//   * SE blocks: two-level average pool, gate = 1 + sigmoid(..) (the block's identity shortcut folded in), scale;
//   * decoder: the four 1x1 lateral convs run coarse to fine, each adding the nearest-x2 up-sampled running sum in its
//     epilogue (up8(a) + up4(b) + up2(c) + d == up2(up2(up2(a) + b) + c) + d for nearest up-sampling); depthwise 5x5 +
//     ReLU; 1x1 64 -> 16 + ReLU on the MFMA kernel; everything after that in dbnas_tail_kernel.
// Channel counts are stored padded to multiples of 64 (32 -> 64, 96 -> 128) with zero weights, so that a residual has
// the GEMM's own channel stride; PReLU(0) = 0 and x * gate keep the padding zero.
#include <string>

#include "net_ctx.h"

namespace PT_FMT_NS {

namespace {

// kind (0 conv block, 1 SE), cin, cout, expand ratio, depthwise kernel after folding, stride, SE squeeze factor
// proxyless.py:107-127: conv_candidates[conv_op_ids[i]] per block; '135'/'35' RepConv fold to k = 5
struct Blk { int kind, cin, cout, expand, k, stride, squeeze; };
const Blk kBlocks[24] = {
    {0, 32, 32, 2, 5, 2, 0},  {0, 32, 32, 2, 5, 1, 0},  {0, 32, 32, 2, 5, 1, 0},  {0, 32, 32, 2, 5, 1, 0},  {0, 32, 32, 2, 5, 1, 0},
    {1, 32, 32, 0, 0, 1, 2},
    {0, 32, 64, 4, 5, 2, 0},  {0, 64, 64, 4, 5, 1, 0},  {0, 64, 64, 4, 5, 1, 0},  {0, 64, 64, 4, 5, 1, 0},  {0, 64, 64, 4, 5, 1, 0},
    {1, 64, 64, 0, 0, 1, 8},
    {0, 64, 96, 4, 5, 2, 0},  {0, 96, 96, 4, 5, 1, 0},  {0, 96, 96, 4, 5, 1, 0},  {0, 96, 96, 4, 5, 1, 0},  {0, 96, 96, 4, 5, 1, 0},
    {1, 96, 96, 0, 0, 1, 8},
    {0, 96, 128, 4, 5, 2, 0}, {0, 128, 128, 4, 5, 1, 0}, {0, 128, 128, 4, 5, 1, 0}, {0, 128, 128, 4, 5, 1, 0}, {0, 128, 128, 4, 5, 1, 0},
    {1, 128, 128, 0, 0, 1, 8}};

inline int pad64(int c) { return (c + 63) / 64 * 64; }

struct Ctx : NetCtx {
  // 1x1 conv (+ folded BN); act 0 none / 1 ReLU / 3 PReLU(slope tensor q.slope); res_mode 1: + res, 2: + nearest-x2(res)
  void pw(const T& in, const std::string& q, int N, const T& out, int act, const T* res = nullptr, int res_mode = 1, int nv = 0) {
    const PtTensor* sl = act == 3 ? get(q + ".slope") : nullptr;
    ConvDesc c;
    if (!conv_desc(c, in, q, N, 1, 1, act)) return;
    c.n_valid = nv;
    if (sl) c.slope = F(sl);
    to_map(c, out);
    if (res) { c.res = res->p; c.res_mode = res_mode; }
    launch(c);
  }
  T dw(const T& in, const std::string& q, int k, int stride, int act) {
    const int pad = k / 2;
    T o = alloc((in.H + 2 * pad - k) / stride + 1, (in.W + 2 * pad - k) / stride + 1, in.C);
    const PtTensor* w = get(q + ".wf32");
    const PtTensor* b = get(q + ".b");
    const PtTensor* sl = act == 3 ? get(q + ".slope") : nullptr;
    if (go()) {
      PtProfScope ps(e, s, PT_PROF_OTHER, 0, "dbnas dwconv");
      const int r = pt_launch_dwconv(in.p, F(w), F(b), o.p, n, in.H, in.W, in.C, k, stride, act, x3, s, sl ? F(sl) : nullptr);
      if (r != PT_OK) rc = r;
    }
    return o;
  }
};

}  // namespace

// x: NHWC4 bf16 [n, H, W, 4] (8 channels in BF16X3 mode); prob / logits: fp32 [n, H, W] (either may be null)
int pt_dbnas_forward_net(pt_engine* e, const bf16_t* x, int n, int H, int W, float* prob, float* logits, hipStream_t s) {
  PT_REQUIRE(x && (prob || logits) && n > 0, "DB-NAS net: null pointer");
  PT_REQUIRE(H % 32 == 0 && W % 32 == 0 && H > 0 && W > 0, "DB-NAS net: input %dx%d must be multiples of 32", H, W);
  const PtModel* m = pt_find_model(e, PT_MODEL_DB_NAS, "DB-NAS", "PT_MODEL_DB_NAS");
  if (!m) return PT_ERR_STATE;
  Ctx c;
  c.init(e, m, "DB-NAS", s, n, PT_ARENA_DET);
  return pt_plan_then_launch(c, "DB-NAS net", [&]() -> int {
    float* gate = c.take<float>((size_t)n * 512 * sizeof(float));
    float* part = c.take<float>((size_t)n * PT_SE_CHUNKS * 512 * sizeof(float));
    T t = c.alloc(H / 2, W / 2, 64);
    {
      const PtTensor* w = c.get("stem.wf32");
      const PtTensor* b = c.get("stem.b");
      if (c.go()) {
        PtProfScope ps(e, s, PT_PROF_STEM, 0, "dbnas stem3x3");
        const int r = pt_launch_stem3x3s2(x, c.F(w), c.F(b), t.p, n, H, W, c.x3, s, 1);
        if (r != PT_OK) c.rc = r;
      }
    }
    T feats[4];
    for (int i = 0; i < 24; ++i) {
      const Blk& b = kBlocks[i];
      const std::string q = "b" + std::to_string(i);
      if (b.kind == 1) {
        const PtTensor *w1 = c.get(q + ".se.w1"), *b1 = c.get(q + ".se.b1"), *w2 = c.get(q + ".se.w2"), *b2 = c.get(q + ".se.b2");
        T g = c.alloc(t.H, t.W, t.C);
        if (c.go()) {
          PtProfScope ps(e, s, PT_PROF_OTHER, 0, "dbnas SE");
          const int r = pt_launch_se(t.p, c.F(w1), c.F(b1), c.F(w2), c.F(b2), gate, g.p, n, t.H * t.W, t.C, c.x3, s,
                                     b.cin / b.squeeze, 1, part);
          if (r != PT_OK) c.rc = r;
        }
        t = g;
        feats[i / 6] = t;       // NasRecBackbone.forward: outputs after blocks 5, 11, 17, 23 (proxyless.py:21-31)
        continue;
      }
      const int mid = b.cin * b.expand, coutp = pad64(b.cout);
      T ex = c.alloc(t.H, t.W, mid);
      c.pw(t, q + ".exp", mid, ex, 3);
      T d = c.dw(ex, q + ".dw", b.k, b.stride, 3);
      T o = c.alloc(d.H, d.W, coutp);
      const bool shortcut = b.stride == 1 && b.cin == b.cout;
      c.pw(d, q + ".proj", coutp, o, 0, shortcut ? &t : nullptr, 1);
      t = o;
    }
    // ---- LightSegDetector (dbnet.py:458-469)
    T acc = c.alloc(feats[3].H, feats[3].W, 64);
    c.pw(feats[3], "dec.in5", 64, acc, 0);
    static const char* lat[3] = {"dec.in4", "dec.in3", "dec.in2"};
    for (int l = 2; l >= 0; --l) {
      PT_REQUIRE(feats[l].H == 2 * acc.H && feats[l].W == 2 * acc.W, "DB-NAS net: feature maps are not exact halves");
      T nx = c.alloc(feats[l].H, feats[l].W, 64);
      c.pw(feats[l], lat[2 - l], 64, nx, 0, &acc, 2);
      acc = nx;
    }
    T d = c.dw(acc, "dec.dw", 5, 1, 1);
    T y16 = c.alloc(d.H, d.W, 16);
    c.pw(d, "dec.pw", 64, y16, 1, nullptr, 1, 16);
    {
      const PtTensor* tw = c.get("dec.tail");
      if (c.go()) {
        PtProfScope ps(e, s, PT_PROF_OTHER, 0, "dbnas tail");
        const int r = pt_launch_dbnas_tail(y16.p, c.F(tw), n, y16.H, y16.W, c.x3, prob, logits, s);
        if (r != PT_OK) c.rc = r;
      }
    }
    return c.rc;
  });
}

}  // namespace PT_FMT_NS
